// mph_list.h -- the neighbour lists as the search (mph_search.hip) writes them and the list passes
// (mph_passes.hip) read them: the blocks of the list kernels and their XCD maps, the ELL tiles and
// their entries, the aligned rows' decoding (RowMask), and pass B's gather record.
#pragma once

#include "mph_device.h"

namespace mph {

// Threads per block of the three list kernels (search, pass A, pass B): MPH_LB / 64 wavefronts
#ifndef MPH_LB
#define MPH_LB 256
#endif
constexpr int kWB = MPH_LB / 64;
__device__ __forceinline__ int list_blocks(int n) { return (n + MPH_LB - 1) / MPH_LB; }

// Work-balanced XCD map of the two list passes.  The waves' work is not uniform along the sorted
// order (walls, the free surface, a slab's ghost waves), so equal block counts per XCD leave some
// XCDs idle while the last one finishes (tools/xcd_diag.py: the XCDs' end times spread 8-29 %).
// The launch has list_grid() blocks (a multiple of 8 with 25 % slack); logical XCD j = b & 7 (the
// hardware deals blocks round-robin) takes the contiguous range [lo_j, lo_j+1) of the nb live
// blocks, lo_j = xcd_frac[j] * nb / 2^16 from DevState (k_xcd_split, from this step's search:
// a wave's work = its longest list + kWaveCost), and its blocks past the range exit.  Any range
// past the grid's share, or no split yet, falls back to the equal ranges of xcd_block: each live
// block is taken exactly once either way.  Returns the block's index among the live blocks, or -1.
// The search itself keeps the equal ranges: its cost follows the candidates it scans, not the
// lists it writes (balanced by list length it ran 8 % slower at D1M; by the previous step's wave
// durations all three kernels oscillated, profiles/r03/xcd_balance/).
constexpr int kWaveCost = 16;   // a wave's fixed cost, in list entries, for the work histogram

// rev: each XCD takes its range from the far end (pass A: it starts on the list tiles the search
// wrote last, which the Infinity Cache still holds)
// fr: the map's fractions (DevState.xcd_frac for the passes; xcd_sfrac for a lazy step's search)
__device__ __forceinline__ int list_block(const int* fr, int n, bool rev = false)
{
    const int nb = list_blocks(n);
    const int b = blockIdx.x;
    if (fr) {
        const int cap = gridDim.x >> 3;
        const int j = b & 7;
        bool ok = fr[0] == 0 && fr[8] == 65536;
        int lo = 0, mine_lo = 0, mine_c = 0;
        for (int x = 0; x < 8; ++x) {
            const int hi = (int)(((long long)fr[x + 1] * nb) >> 16);
            const int c = hi - lo;
            ok = ok && c >= 0 && c <= cap;
            if (x == j) { mine_lo = lo; mine_c = c; }
            lo = hi;
        }
        if (ok) {
            const int q = b >> 3;
            return q < mine_c ? mine_lo + (rev ? mine_c - 1 - q : q) : -1;
        }
    }
    if (b >= nb) return -1;
    if (!rev) return xcd_block(b, nb);
    // xcd_block's range of XCD b & 7 from its end
    const int xcd = b & 7, q = nb >> 3, r = nb & 7;
    const int lo = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    const int cnt = q + (xcd < r ? 1 : 0);
    return lo + cnt - 1 - (b >> 3);
}
__device__ __forceinline__ int list_block(const DevState* st, int n, bool rev = false)
{
    return list_block(st ? st->xcd_frac : nullptr, n, rev);
}

// Grid of the two list passes: the XCD map (list_block) needs a multiple of 8 blocks, with 25 %
// slack for its unequal ranges.  Below Launch.xcd_bal_min particles (default 2^20) the split
// kernel's ~7 us costs more than the balance gains (Bar 400k, 0.23 ms per step: 1.76e9 p-steps/s
// with it, 1.80e9 without), so the passes keep the equal ranges and the search feeds no histogram.
// A lazy step's maps (DevState.seg_lwork, seg_swork) need more: its idle waves weigh next to nothing
// and lie together, so the XCD that holds them takes a range of ~30 % of the blocks at D1M at rest
// (22 % of the waves idle, the far half of the tank), which 25 % slack cannot hold -- list_block
// would fall back to the equal ranges and leave that XCD idle.  lazy: three blocks per live block,
// any range up to 3/8 of them; the blocks past a range exit at once.
static inline int list_grid(int n, bool lazy = false)
{
    const int nb = blocks(n, MPH_LB);
    return ((lazy ? 3 * nb : nb + nb / 4) + 15) / 8 * 8;
}

// a lazy step's search (DevState.seg_swork): a searched wave's cost and an idle wave's (its type and
// position loads and the coarse map's bytes against 49 stencil columns)
constexpr int kSearchCost = 16, kIdleCost = 2;

// The search's contribution to a work histogram (seg: DevState.seg_work, or a lazy step's
// seg_lwork): its wave's longest list (all lanes converged; one atomic per wave, spread over the
// 4096 runs); sseg set (a lazy step): the wave's search cost too.
__device__ __forceinline__ void add_wave_work(int* seg, int cnt, int i, int n, int* sseg = nullptr, bool idle = false)
{
    int m = cnt;
    for (int o = 32; o; o >>= 1) m = max(m, __shfl_xor(m, o));
    const int tile = __builtin_amdgcn_readfirstlane(i >> 6);
    const int ntile = (n + 63) >> 6;
    if ((threadIdx.x & 63) == 0 && tile < ntile) {
        const int r = (int)(((long long)tile * kXcdSegs) / ntile);
        atomicAdd(&seg[r], m + kWaveCost);
        if (sseg) atomicAdd(&sseg[r], idle ? kIdleCost : kSearchCost);
    }
}

__device__ __forceinline__ int nbr_entry(int j, int type) { return j | (type << kTypeShift); }
// (the search's per-lane store counter and its constants per format: mph_params.h soff_*)

__device__ __forceinline__ const int* ell_row(const int* nbr, int i)
{
    return nbr + (size_t)(i >> 6) * kTileStride + (i & 63);
}

// entry k of a lane from the lane's ell_row pointer: row k of the wave's tile
__device__ __forceinline__ const int* ell_at(const int* row, int lane, int k)
{
    return row - lane + ell_slot(k, lane);
}

// The wave's ELL tile and the lane: entry k of the lane at row k, by a 32-bit byte offset from the
// tile's (SGPR) base -- one shift-or per entry instead of 64-bit address arithmetic.
struct NbrList {
    const int* tile;   // the wave's list tile (wave-uniform)
    int lane;
};

__device__ __forceinline__ NbrList nbr_list(const int* nbr, int i)
{
    NbrList L;
    L.tile = nbr + (size_t)__builtin_amdgcn_readfirstlane(i >> 6) * kTileStride;
    L.lane = i & 63;
    return L;
}

// entry k of the lane: neighbour index j and type t.  (A buffer descriptor here, to skip the loads
// past a lane's end, costs pass A 4 more SGPRs than it has: spills inside its loop.)
__device__ __forceinline__ void nbr_at(const NbrList& L, int k, int& j, int& t)
{
    using gcchar = const __attribute__((address_space(1))) char;
    using gcint = const __attribute__((address_space(1))) int;
    const int e = *(gcint*)((gcchar*)L.tile + ((unsigned)ell_slot(k, L.lane) << 2));
    j = e & kIndexMask;
    t = e >> kTypeShift;
}
// the same of a short wave (16-bit rows): the entry's offset from its group's base, and its type
__device__ __forceinline__ void nbr_at16(const NbrList& L, int k, int& off, int& t)
{
    using gcchar = const __attribute__((address_space(1))) char;
    using gcshort = const __attribute__((address_space(1))) unsigned short;
    const unsigned e = *(gcshort*)((gcchar*)L.tile + ((unsigned)ell_slot(k, L.lane) << 1));
    off = entry16_off(e);
    t = entry16_type(e);
}

// A short wave's list loop keeps the stencil group of its (wave-uniform) row as scalars: the group,
// the row its successor starts on (header byte g; none after the last) and the group's base scaled
// to the loop's gather stride, re-read from the wave's bases where the row passes a group start --
// kMaxJumps times per wave, a compare and a branch on the other rows.
struct GroupWalk {
    const int* base;   // the wave's kBaseInts bases
    unsigned long long hdr;
    int stride;        // bytes per gathered record
    GroupCursor cur;   // (mph_params.h)
    unsigned sb;       // base[cur.g] * stride
    int j0;            // base[cur.g]
    __device__ __forceinline__ void load()
    {
        j0 = __builtin_amdgcn_readfirstlane(base[cur.g]);
        sb = (unsigned)j0 * (unsigned)stride;
    }
    __device__ __forceinline__ void init(const int* lbase, int i, unsigned long long h, int st)
    {
        base = lbase + (size_t)__builtin_amdgcn_readfirstlane(i >> 6) * kBaseInts;
        hdr = h;
        stride = st;
        cur.init(h);
        load();
    }
    // on to row k (k wave-uniform, never below an earlier call's)
    __device__ __forceinline__ void seek(int k)
    {
        if (cur.seek(hdr, k)) load();
    }
};

// Aligned rows (mph_params.h kAlignRows).  A wave's jumps are recorded in two places: the wave's
// header word lhdr[tile] (byte k < kMaxJumps: the row the lanes moved on to at jump k; byte 7: the
// number of jumps J), and per lane lgap[i] (byte k: the lane's own row when it jumped), so the
// lane's gap k is the rows [lgap byte k, lhdr byte k).  Every row of [0, end) outside the gaps
// holds an entry (end = the lane's ncount), in the lane's list order.  A wave that never jumps
// (J = 0: on the lattice, and every wave of the per-lane search) has plain rows, entry k at row k.
// RowMask: the rows below kAlignRows that hold an entry, one bit each; rows from kAlignRows on
// hold one exactly when they are below end.
struct RowMask {
    unsigned long long lo, hi;
};

// bits [k, 64) of a 64-bit word, k clamped to [0, 64]
__device__ __forceinline__ unsigned long long bits_from(int k)
{
    return k <= 0 ? ~0ull : (k >= 64 ? 0ull : (~0ull << k));
}

__device__ __forceinline__ RowMask row_mask(unsigned long long hdr, const unsigned long long* lgap, int i, int end)
{
    RowMask m;
    m.lo = ~bits_from(end);
    m.hi = ~bits_from(end - 64);
    const int J = gap_count(hdr);
    if (J) {   // wave-uniform
        const unsigned long long g = lgap[i];
        for (int k = 0; k < J; ++k) {
            const int a = gap_begin(g, k), b = gap_end(hdr, k);
            m.lo &= ~(bits_from(a) & ~bits_from(b));
            m.hi &= ~(bits_from(a - 64) & ~bits_from(b - 64));
        }
    }
    return m;
}

// whether row r holds one of the lane's entries
__device__ __forceinline__ bool row_ok(const RowMask& m, int r, int end)
{
    if (r < 64) return (m.lo >> r) & 1;
    if (r < kAlignRows) return (m.hi >> (r - 64)) & 1;
    return r < end;
}

// rows [k0 + a, k0 + b) as bits 0..31, a, b clamped to [0, 32]
__device__ __forceinline__ unsigned bit_range(int a, int b)
{
    auto low = [](int n) { return n <= 0 ? 0u : (n >= 32 ? ~0u : (1u << n) - 1u); };
    return low(b) & ~low(a);
}

// the rows from kAlignRows on: bit u set when row k0 + u holds an entry there (k0 + u < end)
__device__ __forceinline__ unsigned tail_bits(int k0, int end)
{
    return bit_range(kAlignRows - k0, end - k0);
}

// bit u: row k0 + u holds one of the lane's entries (k0 wave-uniform in the list loops; bits
// 0..31), without branches
__device__ __forceinline__ unsigned row_bits(const RowMask& m, int k0, int end)
{
    const int k = k0 < kAlignRows ? k0 : kAlignRows - 1;
    const unsigned long long lo = k < 64 ? m.lo : m.hi, hi = k < 64 ? m.hi : 0ull;
    const int sh = k & 63;
    const unsigned b = (unsigned)((lo >> sh) | (sh ? hi << (64 - sh) : 0ull));
    return (b & bit_range(0, kAlignRows - k0)) | tail_bits(k0, end);
}

// The 128 mask bits of the lanes of a wave in LDS, 6 dwords per lane (the last two zero; a 24-byte
// stride keeps the 32 lanes of a read group on distinct banks): pass A, whose registers are full
constexpr int kMaskWords = 6;
__device__ __forceinline__ void mask_to_lds(unsigned* lm, const RowMask& m)
{
    lm[0] = (unsigned)m.lo;
    lm[1] = (unsigned)(m.lo >> 32);
    lm[2] = (unsigned)m.hi;
    lm[3] = (unsigned)(m.hi >> 32);
    lm[4] = 0u;
    lm[5] = 0u;
}
__device__ __forceinline__ unsigned row_bits_lds(const unsigned* lm, int k0, int end)
{
    const int d = k0 < kAlignRows ? k0 >> 5 : 3;
    const unsigned long long v = (unsigned long long)lm[d] | ((unsigned long long)lm[d + 1] << 32);
    return ((unsigned)(v >> (k0 & 31)) & bit_range(0, kAlignRows - k0)) | tail_bits(k0, end);
}


// the wave's header word (scalar load)
__device__ __forceinline__ unsigned long long wave_hdr(const unsigned long long* lhdr, int i)
{
    return lhdr[__builtin_amdgcn_readfirstlane(i >> 6)];
}

// The search's row jumps: a jump at a stencil group end only when the wave's rows have drifted at
// least this far apart (highest - lowest row of the live lanes); 1 = at every group end where the
// rows differ, a value > kAlignRows = never (plain rows)
#ifndef MPH_ALIGN_DRIFT
#define MPH_ALIGN_DRIFT 1
#endif
constexpr int kAlignDrift = MPH_ALIGN_DRIFT;

// Slab mode: true when no lane of the wave holds an owned particle (ghost ids are negative).
// With the (z, x, y) cell order of z slabs (DevParams.perm) the ghosts beyond the two faces fill
// whole wavefronts at the ends of the sorted arrays; their lists and pass-A/pass-B sums are not
// needed (their pass-A values arrive in the halo, their pass-B results are dropped), so the list
// kernels skip them.
__device__ __forceinline__ bool wave_all_ghosts(const DevParams& P, const Soa& A, bool live, int ii)
{
    if (P.slab_axis < 0) return false;
    return __all(!live || A.id[ii] < 0);
}

// Pass B's gather record {x, y, z, PressureP} (Launch.rec) lives in two 16-byte planes: {x, y} of
// particle j at [j], {z, P} at [ps + j], ps = the array capacity (DevParams.n).  A 16-byte gather
// instruction of a wavefront then reads one plane: 64 lanes whose neighbours are consecutive
// particles touch 1 KB (8 lines of 128 B) instead of 2 KB of whole records (same box: D1M pass B
// 0.271 -> 0.251 ms, D16M 2.89 -> 2.66 ms, profiles/r05/planes/).  Pass A's 48-byte records
// {x, y, z, vx, vy, vz} (Soa.p6) stay whole: in three planes pass A lost (0.376 -> 0.446 ms).

// pass B's gather record {x, y, z, PressureP} of sorted particle i (planes {x, y} and {z, P}, see
// above; ps = DevParams.n), and its PressureP alone (the halo)
__device__ __forceinline__ void rec_store(double4* rec, int ps, int i, double x, double y, double z, double p)
{
    double2* r = reinterpret_cast<double2*>(rec);
    r[i] = make_double2(x, y);
    r[(size_t)ps + i] = make_double2(z, p);
}
__device__ __forceinline__ void rec_store_p(double4* rec, int ps, int i, double p)
{
    reinterpret_cast<double2*>(rec)[(size_t)ps + i].y = p;
}
__device__ __forceinline__ void rec_load(const double4* rec, int ps, int j, double& x, double& y, double& z, double& p)
{
    const double2* r = reinterpret_cast<const double2*>(rec);
    const double2 a = r[j], b = r[(size_t)ps + j];
    x = a.x; y = a.y; z = b.x; p = b.y;
}


}  // namespace mph
