// mph_search.hip -- the linked-cell neighbour search k_neighbors (mph_kernels.h has the step-to-
// launch map): it writes the ELL neighbour lists that the list passes read (mph_list.h).
#include "mph_list.h"

// Tuning parameters (A/B builds: tools/ab.sh).  The rejected variants of rounds 1-5 (staged pass A,
// row spreading, CU-affine tiles, paired / half-wave / compact 16-bit lists, chunked search, cache-
// policy hints, record planes for pass A, block totals from k_prep, the diagnostic builds) were
// removed in round 6; they are kept under the git tag r05-variants (profiles/r05/README.md).
#ifndef MPH_SB
// candidates per batch in the search: 2 (64 VGPRs) with the LDS capacity below gives 8 waves per
// SIMD (round 3: D1M 0.355 -> 0.347 ms, D16M 4.11 -> 3.86, profiles/r03/search/sb2/); 3 took
// 72 VGPRs and 7 waves (round 2: 0.395 ms against 0.433 at 4)
#define MPH_SB 2
#endif
#ifndef MPH_LDS_CAP
// staging area per wave and stencil column, in FP64 candidates: 176 keeps a wave's staging at
// 5,072 B, so 32 waves (8 per SIMD) fit the 160 KB of LDS; it holds 313 of the 16-byte FP32
// records (kCap32), wider windows take the global-gather loop
#define MPH_LDS_CAP 176
#endif

namespace mph {

// A 4-byte load through a buffer descriptor that hipcc does not count (the search's start[]
// loads, scan_candidates_lds): no s_waitcnt is emitted for it, so the caller waits for it with an
// explicit vmcnt(0) on every path before start_landed() and the first use of the value.
// Both bounds of a column range in one statement: the descriptor may come from SGPRs that a VALU
// instruction (v_readlane of an SGPR spill) has just written, which a VMEM instruction may read only
// 5 wait states later (hipcc pads only what it sees: s_nop 4 opens the string).
__device__ __forceinline__ void start_load2(__amdgpu_buffer_rsrc_t r, unsigned ob, unsigned oe, int& b, int& e)
{
    asm volatile("s_nop 4\n\tbuffer_load_dword %0, %2, %4, 0 offen\n\tbuffer_load_dword %1, %3, %4, 0 offen"
                 : "=&v"(b), "=&v"(e) : "v"(ob), "v"(oe), "s"(r) : "memory");
}
// marks the start_load2 results as landed: no consumer is scheduled above this point
__device__ __forceinline__ void start_landed(int& a, int& b) { asm volatile("" : "+v"(a), "+v"(b)); }

// LDS staging area of one wavefront in the search, in doubles: sized as the FP64 staging of CAP
// candidates (x, y, z: stage_d doubles each, types: stage_t ints) of rounds 1-4, which it holds the
// FP32 records of (16 bytes each, scan_candidates_lds kCap32).
__host__ __device__ constexpr int stage_d(int cap, int sb) { return (cap + sb + 2 + 1) & ~1; }
__host__ __device__ constexpr int stage_t(int cap, int sb) { return (cap + sb + 8 + 3) & ~3; }
__host__ __device__ constexpr int stage_words(int cap, int sb) { return 3 * stage_d(cap, sb) + stage_t(cap, sb) / 2; }
// the group bases of a wave with 16-bit rows (3-D kernels; wave_list16): kBaseInts ints behind the staging area
__device__ __forceinline__ int* stage_bases(double* stage)
{
    return reinterpret_cast<int*>(stage + stage_words(MPH_LDS_CAP, MPH_SB));
}


// Logical axes of the cell order for the search: the two column axes (A0 slowest, A1) and the
// contiguous axis A2 (cells half as wide); 2-D: x columns, y contiguous.
template <int DIM, int PERM> struct CellAxes {
    static constexpr int A0 = DIM == 3 ? order_axis(PERM, 0) : 0;
    static constexpr int A1 = DIM == 3 ? order_axis(PERM, 1) : 1;
    static constexpr int A2 = DIM == 3 ? order_axis(PERM, 2) : 1;
};

// ---------------------------------------------------------------------- neighbour search ----

// calculateNeighbor (main.cpp:1743-1810).  The reference scans (2*3+1)^d cells of width dx; here
// cells are >= rc/kReach (rc/3) wide across the two column axes and >= rc/kContigReach (rc/2)
// along the contiguous one, so a +-kReach stencil covers the acceptance sphere: (2 kReach + 1)^2
// = 49 columns (3-D) or 7 (2-D), each one contiguous index range of +-kContigReach cells of the
// last axis.  Acceptance is the reference's own test  q0^2+q1^2+q2^2 <= (MaxRadius+MARGIN)^2
// with the Mod-based minimum image.
// Offset of x from the grid origin, wrapped once into [0, w) (as cell_axis).
__device__ __forceinline__ double grid_offset(double x, double org, double w)
{
    const double u = x - org;
    return u < 0.0 ? u + w : (u >= w ? u - w : u);
}

// Gap between grid offset u (inside cell c) and cell c + d along one axis (0 for d == 0).
__device__ __forceinline__ double cell_gap(double u, int c, int d, double cw)
{
    const double g = d > 0 ? (c + d) * cw - u : (d < 0 ? u - (c + d + 1) * cw : 0.0);
    return g > 0.0 ? g : 0.0;
}

// calculateNeighbor's acceptance (main.cpp:1760-1765) for an interior pair, bit-exact but cheap:
// r2 from the raw difference d = x_j - x_i (FMA) differs from the reference's
// q = (d + W/2) - W/2, r2 = q0^2+q1^2+q2^2 by < 1e-13 relative, so outside a +-1e-10 band
// around rc^2 the answer is decided; inside it (rare) the reference expression is evaluated.
__device__ __forceinline__ bool accept_interior(const DevParams& P, double dx, double dy, double dz,
                                                double lo2, double hi2)
{
    const double r2a = fma(dx, dx, fma(dy, dy, dz * dz));
    bool a = r2a <= lo2;
    if (!a && r2a <= hi2) {   // two compares: the band is "<= hi2 and not <= lo2"
        const double q0 = image_exact<true>(dx, P.dw[0], P.hw[0], P.w075[0]);
        const double q1 = image_exact<true>(dy, P.dw[1], P.hw[1], P.w075[1]);
        const double q2 = image_exact<true>(dz, P.dw[2], P.hw[2], P.w075[2]);
        a = r2_exact(q0, q1, q2) <= P.rc2;
    }
    return a;
}

// the reference's own acceptance expression (as accept_interior inside its band)
__device__ __forceinline__ bool accept_band(const DevParams& P, double dx, double dy, double dz)
{
    const double q0 = image_exact<true>(dx, P.dw[0], P.hw[0], P.w075[0]);
    const double q1 = image_exact<true>(dy, P.dw[1], P.hw[1], P.w075[1]);
    const double q2 = image_exact<true>(dz, P.dw[2], P.hw[2], P.w075[2]);
    return r2_exact(q0, q1, q2) <= P.rc2;
}

template <int DIM, int PERM, int SB = MPH_SB>
__device__ __forceinline__ int scan_candidates(const DevParams& P, const Soa& A, const int* start,
                                               int i, double xi, double yi, double zi, int cx,
                                               int cy, int cz, int* out)
{
    using X = CellAxes<DIM, PERM>;
    int cnt = 0;
    constexpr int NCOL = DIM == 3 ? kGroups * kGroups : kGroups;
    const int cc[3] = {cx, cy, cz};
    const int gca = P.gc[X::A2];   // contiguous axis
    const int cca = cc[X::A2];
    // Column trimming: skip the cells of a column (and whole columns) that lie entirely beyond
    // the cutoff.  Conservative (cutoff enlarged by 1e-6 relative, far above the roundoff of the
    // cell geometry), so the accepted set and its order are unchanged.
    const double rcm2 = P.rc2_trim;
    const double cw0 = P.cwid[X::A0], cw1 = P.cwid[X::A1];
    const double uu[3] = {grid_offset(xi, P.corg[0], P.dw[0]), grid_offset(yi, P.corg[1], P.dw[1]),
                          DIM == 3 ? grid_offset(zi, P.corg[2], P.dw[2]) : 0.0};
    const double ua = uu[X::A2];                      // offset along the contiguous axis
    const double ginva = P.ginv[X::A2];
    for (int col = 0; col < NCOL; ++col) {
        int base;
        double d2;
        if (DIM == 3) {
            const int dxc = col / kGroups - kReach, dyc = col % kGroups - kReach;
            const int c0 = cc[X::A0], c1 = cc[X::A1];
            const double gx = cell_gap(uu[X::A0], c0, dxc, cw0), gy = cell_gap(uu[X::A1], c1, dyc, cw1);
            d2 = gx * gx + gy * gy;
            if (d2 > rcm2) continue;
            const int jx = wrap_cell(c0 + dxc, P.gc[X::A0]);
            const int jy = wrap_cell(c1 + dyc, P.gc[X::A1]);
            base = (jx * P.gc[X::A1] + jy) * P.gc[X::A2];
        } else {
            const int dxc = col - kReach;
            const double gx = cell_gap(uu[0], cx, dxc, cw0);
            d2 = gx * gx;
            if (d2 > rcm2) continue;
            base = wrap_cell(cx + dxc, P.gc[0]) * P.gc[1];
        }
        const double ra = sqrt(rcm2 - d2);
        const int lo = (int)fmax(floor((ua - ra) * ginva), (double)(cca - P.sa));
        const int hi = (int)fmin(floor((ua + ra) * ginva), (double)(cca + P.sa));
        int seg_a[2], seg_b[2], nseg;
        if (lo < 0) { seg_a[0] = lo + gca; seg_b[0] = gca - 1; seg_a[1] = 0; seg_b[1] = hi; nseg = 2; }
        else if (hi >= gca) { seg_a[0] = lo; seg_b[0] = gca - 1; seg_a[1] = 0; seg_b[1] = hi - gca; nseg = 2; }
        else { seg_a[0] = lo; seg_b[0] = hi; seg_a[1] = 0; seg_b[1] = -1; nseg = 1; }
        for (int sg = 0; sg < nseg; ++sg) {
            const int jb = start[base + seg_a[sg]];
            const int je = start[base + seg_b[sg] + 1];
            // batches of SB candidates: all loads issued before the first test (memory-level
            // parallelism; the loop is bound by the gathers, not by the FP64 arithmetic)
            for (int j0 = jb; j0 < je; j0 += SB) {
                double xs[SB], ys[SB], zs[SB];
                {
#pragma unroll
                    for (int u = 0; u < SB; ++u) {
                        const int j = j0 + u < je ? j0 + u : je - 1;
                        xs[u] = A.x[j];
                        ys[u] = A.y[j];
                        zs[u] = A.z[j];
                    }
                }
#pragma unroll
                for (int u = 0; u < SB; ++u) {
                    const int j = j0 + u;
                    const double q0 = image_exact<false>(xs[u] - xi, P.dw[0], P.hw[0], P.w075[0]);
                    const double q1 = image_exact<false>(ys[u] - yi, P.dw[1], P.hw[1], P.w075[1]);
                    const double q2 = image_exact<DIM == 2>(zs[u] - zi, P.dw[2], P.hw[2], P.w075[2]);
                    const bool a = r2_exact(q0, q1, q2) <= P.rc2;
                    if (a && j < je && j != i) {
                        if (cnt < kMaxNeighbor) out[ell_slot(cnt, 0)] = nbr_entry(j, A.type[j]);
                        ++cnt;
                    }
                }
            }
        }
    }
    return cnt;
}

// The search of a wave whose particles are all interior (FAST): per stencil column the union of
// the 64 lanes' candidate ranges is one short index range (the lanes are consecutive in cell
// order, mostly inside one or two cell columns), so the wave stages it in LDS with coalesced
// loads and every lane then tests its own candidates from LDS.  The global gathers of the
// per-lane loop cost ~19 L1 tag lookups per load instruction (PMC, profiles/r01) and the
// texture-address unit was the bound; a staged column costs 4.  Same candidates, same order and,
// where it decides, the same FP64 test as scan_candidates, so the list is identical.  Every lane of
// the wave must call this (act = live particle); the column loop and the staging are wave-uniform.
//
// Per column the wave waits for memory once: the start[] loads of column col + 1 are issued before
// column col's staging loads, so the one wait for the staging also covers them and the next
// column's window is ready at once.  hipcc would wait for them at their first use instead (round 3:
// predicated loads, a register copy at the loop latch, a merge with the list stores pending on
// the same counter -- each made it emit vmcnt(0) right after issuing them: two round trips per
// column), so they are issued in asm (start_load), which hipcc does not count, and every path of a
// column ends in an explicit vmcnt(0) before the next column reads them (start_landed).
//
// LEAN (a lean step's search, enqueue_step; the caller has checked lean_search_ok): the stored list
// is {live && r2f <= rlf} (the full form stores live && a && r2f <= rlf, and rlf <= rc2f_lo makes a
// true wherever r2f <= rlf), and NeighborCount has no reader on such a step.  So the columns are
// trimmed to the list radius (DevParams.rl_trimf: every stored candidate lies inside, set_uniforms),
// a candidate is accepted by that one compare -- no band, no ballots, no FP64 test -- and the
// counter's total field advances with the stored one.  Candidate order, group ends, row jumps and
// the lhdr / lgap bytes are the full form's, so every lane stores the same entries in the same
// rows; the return value counts the stored entries.  (A window that only the wider ranges push past
// the staging area takes the gather loop in the full form alone, which then also stores the
// shell's pairs: more rows, the same entries within the passes' radii in the same order.)
//
// S16 (3-D; the caller has found every stencil group's candidates within DevParams.list16_span
// indices of the group's base, sbase[group], in the wave's LDS): the wave's rows are 16-bit ones
// (mph_params.h kOff16Bits).  A column's range, its window and the candidate loop run on indices
// relative to the group's base (subtracted once per column), so an entry is formed by the one
// instruction it costs in the wide format, and every group end is a jump -- taken whether or not
// the lanes' rows differ -- so that each group starts on a wave-uniform row (header byte g - 1)
// and the passes decode a row with one scalar base.  Returns -1, wave-uniformly, when the wave's
// highest row has reached kAlignRows at a group end (a very dense cluster) or a column's window
// does not fit the staging area: the caller then runs the wide form from column 0 over the same
// tile (restarted).
template <int DIM, int PERM, bool LEAN, bool S16, int SB = MPH_SB, int CAP = MPH_LDS_CAP>
__device__ __forceinline__ int scan_candidates_lds(const DevParams& P, const Soa& A, const int* start,
                                                   int i, bool act, double xi, double yi, double zi,
                                                   int cx, int cy, int cz, int* out, double* sx, int* stored,
                                                   unsigned long long* lgap, unsigned long long* lhdr)
{
    // S16: the groups' bases, behind the wave's staging area (stage_bases)
    const int* sbase = reinterpret_cast<const int*>(sx + stage_words(CAP, SB));
    static_assert(!S16 || DIM == 3, "the 16-bit rows are the 3-D search's");
    // the staging area holds the window's 16-byte FP32 records, SB past the window's end
    constexpr int kCap32 = stage_words(CAP, SB) / 2 - SB - 1;
    const int lane = threadIdx.x & 63;
    // buffer descriptor of the wave's ELL tile (out - lane, wave-uniform): list stores take a 32-bit
    // lane offset instead of a 64-bit address; a store past the tile is dropped by the hardware
    const unsigned long long tb = (unsigned long long)(out - lane);
    const unsigned tlo = __builtin_amdgcn_readfirstlane((unsigned)tb);
    const unsigned thi = __builtin_amdgcn_readfirstlane((unsigned)(tb >> 32));
    const __amdgpu_buffer_rsrc_t tile_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<void*>(((unsigned long long)thi << 32) | tlo), 0,
        kTile * kTileRows * (int)(S16 ? sizeof(short) : sizeof(int)), 0x00020000);
    // the entry of candidate j (S16: relative to the group's base) and its store
    auto put = [&](int j, int type, int off) {
        if constexpr (S16)
            __builtin_amdgcn_raw_buffer_store_b16((short)(j | (type << kOff16Bits)), tile_rsrc, off, 0, 0);
        else
            __builtin_amdgcn_raw_buffer_store_b32(nbr_entry(j, type), tile_rsrc, off, 0, 0);
    };
    constexpr int kListKeep = soff_keep(S16);
    const double lo2 = P.rc2_lo, hi2 = P.rc2_hi;
    using X = CellAxes<DIM, PERM>;
    constexpr int NCOL = DIM == 3 ? kGroups * kGroups : kGroups;
    const int cc[3] = {cx, cy, cz};
    const int cca = cc[X::A2];
    const double cw0 = P.cwid[X::A0], cw1 = P.cwid[X::A1];
    const double uu[3] = {grid_offset(xi, P.corg[0], P.dw[0]), grid_offset(yi, P.corg[1], P.dw[1]),
                          DIM == 3 ? grid_offset(zi, P.corg[2], P.dw[2]) : 0.0};
    const double ua = uu[X::A2];
    const double ginva = P.ginv[X::A2];
    // Candidate range of this lane in stencil column col (cell ranges -> start[] loads).  The
    // trimming is only a bound (the exact test decides), so it runs in FP32 from per-lane values
    // computed once (the offsets inside the own cell across the columns and along the contiguous
    // axis, the row base), every rounding outwards by an absolute margin: the squared cell gaps
    // down (2^-20 cell widths), the cutoff and the half range up, the range ends out by 1e-3
    // cells.  Each range therefore holds the FP64 one (a superset: same candidates, same list).
    // The contiguous-axis offset is taken relative to the own cell in FP64 before the conversion
    // (ua ginv - c lies in [0, 1) for an interior lane), so the margin holds on any grid size.
    // The gap along the slowest axis changes once per group of columns (visited in order).
    // An inactive lane gets a negative cutoff (no column opens); the gap margin mu is folded into
    // the subtracted offsets; the range ends carry a bias of kBias cells, so truncation is floor
    // (the ends lie within a few cells of the own cell) and the bias comes off in the row base.
    // Each added rounding is below 1e-5 cells or 2^-24 of a cell width, far inside the margins.
    constexpr float kDn = 1.0f - 1.0f / (1 << 20), kUp = 1.0f + 1.0f / (1 << 19);
    constexpr float kBias = 32.0f;
    const float rcm2f = act ? (LEAN ? P.rl_trimf : (float)P.rc2_trim) * kUp : -1.0f;
    float gx2f = 0.0f;
    const int c0l = cc[X::A0], c1l = DIM == 3 ? cc[X::A1] : 0;
    const float cw0f = (float)cw0, cw1f = (float)cw1;
    const float f0 = (float)(uu[X::A0] - c0l * cw0), f1 = DIM == 3 ? (float)(uu[X::A1] - c1l * cw1) : 0.0f;
    const float mu0 = cw0f * (1.0f / (1 << 20)), mu1 = cw1f * (1.0f / (1 << 20));
    const float g0p = f0 + mu0, g0m = (cw0f - f0) + mu0, g1p = f1 + mu1, g1m = (cw1f - f1) + mu1;
    const float ginvaf = (float)ginva;
    const float caf = (float)(ua * ginva - (double)cca);   // offset inside the own cell, cells
    const float cal = (caf - 1e-3f) + kBias, cah = (caf + 1e-3f) + kBias;
    const float rgf = kUp * ginvaf;
    const int rowbase = (DIM == 3 ? (c0l * P.gc[X::A1] + c1l) * P.gc[X::A2] : c0l * P.gc[1]) + cca - (int)kBias;
    const int sa = P.sa;
    const __amdgpu_buffer_rsrc_t srs = arr_rsrc(start);
    auto gap32 = [](int d, float cwf, float gp, float gm) {
        if (d == 0) return 0.0f;
        const float v = (float)(d > 0 ? d : -d) * cwf - (d > 0 ? gp : gm);
        return v > 0.0f ? v : 0.0f;
    };
    auto col_range = [&](int col, int& jb, int& je) {
        int cofs;
        float d2f;
        if (DIM == 3) {
            const int dxc = col / kGroups - kReach, dyc = col % kGroups - kReach;
            if (dyc == -kReach) {
                const float gx = gap32(dxc, cw0f, g0p, g0m);
                gx2f = gx * gx * kDn;
            }
            const float gy = gap32(dyc, cw1f, g1p, g1m);
            d2f = (gx2f + gy * gy * kDn) * kDn;
            cofs = (dxc * P.gc[X::A1] + dyc) * P.gc[X::A2];
        } else {
            const int dxc = col - kReach;
            const float gx = gap32(dxc, cw0f, g0p, g0m);
            d2f = gx * gx * kDn;
            cofs = dxc * P.gc[1];
        }
        const bool ok = d2f <= rcm2f;
        const float rc = __builtin_amdgcn_sqrtf(fmaxf(rcm2f - d2f, 0.0f)) * rgf;   // half range, cells
        const int lo = max((int)(cal - rc), (int)kBias - sa);
        const int hi = min((int)(cah + rc), (int)kBias + sa);
        const int b = rowbase + cofs;
        // a lane without candidates reads start[0] twice (empty range)
        start_load2(srs, ok ? (unsigned)(b + lo) * 4u : 0u, ok ? (unsigned)(b + hi + 1) * 4u : 0u, jb, je);
    };
    // the lane's next list slot (mph_params.h soff_*): soff = stored * 256 + lane * 4 (S16: * 128,
    // * 2; one add per entry, no address arithmetic); bits 18 and up count every accepted neighbour
    // (NeighborCount), the bits below them the stored ones (the FP32 path keeps only r^2 <= P.rlf:
    // kListTotal, kListKeep), so the store offset is soff & kSoffMask
    int soff = soff_first(S16, lane);
    // S16: bit 8 of `jumps` is set once a lane's row differed from the wave's at a group end
    constexpr int kGapsBit = 0x100;
    // Row jumps (aligned rows, see RowMask): at the end of a stencil group (3-D: the 7 columns of
    // one slowest-axis offset; 2-D: a column) the lanes' next rows move on to the wave's highest
    // row, so the next group's entries start on one row for all lanes however far their counts
    // drifted (off the lattice a store instruction otherwise touches as many rows as it has lanes,
    // and the list lines leave L2 partly written).  Only while the highest
    // row is below kAlignRows and the rows differ by kAlignDrift or more; on the lattice the lanes'
    // counts agree and the wave keeps plain rows.
    // The jumps are recorded as they happen (byte stores: the wave's header byte k, the lane's gap
    // byte k), so that no register holds them across the columns (the search is at its 64-VGPR
    // budget); the jump count goes to header byte 7 at the end.
    // jumps: the jumps so far, plus kMaxJumps + 1 once the wave stops jumping (one SGPR)
    constexpr int GSZ = DIM == 3 ? kGroups : 1;
    // (3-D only: the 2-D lists, ~20 entries in 7 columns, drift little, and the checks cost the Bar
    // search 9 %)
    int jumps = DIM == 3 && kAlignDrift <= kAlignRows ? 0 : kMaxJumps + 1;   // (stopped, none made)
    // the wave's header bytes, formed where they are stored (not held in SGPRs across the columns)
    auto hdr_byte = [&](int k) {
        int ii = i;
        asm volatile("" : "+v"(ii));
        return reinterpret_cast<unsigned char*>(lhdr + __builtin_amdgcn_readfirstlane(ii >> 6)) + k;
    };
    // (true: a short wave starts over in the wide format)
    auto group_end = [&]() {
        if (!S16 && jumps >= kMaxJumps) return false;
        const int row = soff_stored(S16, soff);
        const int m = __builtin_amdgcn_readfirstlane(wave_max(row));
        if (m >= kAlignRows) {
            if (S16) return true;
            jumps += kMaxJumps + 1;   // no more jumps
            return false;
        }
        if (S16) {
            // The lanes' gap bytes are stored from the wave's first real gap on: until a lane's row
            // differs from the wave's nothing reads them (kHdrNoGap), and the wave that first differs
            // at jump k stores the whole gap word, the bytes of the jumps before it 0xff -- an empty
            // gap [255, header byte), which the row masks and the host readers take as none.
            const int k = jumps & (kGapsBit - 1);
            if (!(jumps & kGapsBit)) {
                if (__ballot(act && row != m)) {
                    int ii = i;
                    asm volatile("" : "+v"(ii));
                    lgap[ii] = ((unsigned long long)(unsigned)row << (8 * k)) | ~(~0ull << (8 * k));
                    jumps |= kGapsBit;
                }
            } else {
                int ii = i;
                asm volatile("" : "+v"(ii));
                reinterpret_cast<unsigned char*>(lgap + ii)[k] = (unsigned char)row;
            }
            if (lane == 0) *hdr_byte(k) = (unsigned char)m;
            soff += (m - row) << soff_row_shift(S16);
            ++jumps;
            return false;
        } else if (kAlignDrift <= 1) {
            if (!__ballot(act && row != m)) return false;   // the rows agree
        } else {
            const int mn = __builtin_amdgcn_readfirstlane(wave_min(act ? row : m));
            if (m - mn < kAlignDrift) return false;
        }
        // the address formed here, not hoisted out of the column loop as a register pair
        int ii = i;
        asm volatile("" : "+v"(ii));
        reinterpret_cast<unsigned char*>(lgap + ii)[jumps] = (unsigned char)row;   // the lane's gap [row, m)
        if (lane == 0) *hdr_byte(jumps) = (unsigned char)m;
        soff += (m - row) << soff_row_shift(S16);
        ++jumps;
        return false;
    };
    constexpr int kSelfCol = DIM == 3 ? kReach * kGroups + kReach : kReach;   // the lane's own column
    // one stencil column: its range [jb, je) was loaded one column ahead; (nb_jb, nb_je) receive
    // column col + 1's.  The loop below is unrolled by two with the roles of the two register pairs
    // swapped, so no copy at the loop latch waits for the loads in flight.
    int gb = 0;   // S16: the current group's base
    // (true: group_end's)
    auto column = [&](int col, int jb, int je, int& nb_jb, int& nb_je) {
        start_landed(jb, je);   // loaded one column ahead; every path below ended in vmcnt(0)
        if (col > 0 && col % GSZ == 0)
            if (group_end()) return true;   // (no start[] load is in flight here)
        if (col + 1 < NCOL) col_range(col + 1, nb_jb, nb_je);
        // S16: the group's base gb (read at the group's first column, one scalar held through the
        // group); everything below on indices relative to it
        if constexpr (S16) {
            if (col % GSZ == 0) gb = __builtin_amdgcn_readfirstlane(sbase[col / GSZ]);
            jb -= gb;
            je -= gb;
        }
        const bool any = je > jb;
        // the wave's window [mn, mx): the lanes are in cell order, so the first lane with candidates
        // normally has the lowest jb and the last the highest je -- read those two lanes, and take
        // the DPP reductions only when a lane says otherwise (wave-uniform check)
        const unsigned long long am = __ballot(any);
        if (!am) {   // wave-uniform: no lane has candidates in this column
            // wait here for column col + 1's start[] loads, so that every path into the next column
            // has them landed and its first use needs no wait (which would also wait for this
            // column's list stores: loads and stores share vmcnt)
            __builtin_amdgcn_s_waitcnt(0x0F70);
            return false;
        }
        int mn = __builtin_amdgcn_readlane(jb, __ffsll((long long)am) - 1);
        int mx = __builtin_amdgcn_readlane(je, 63 - __clzll(am));
        if (__ballot(any && (jb < mn || je > mx))) {
            mn = wave_min(any ? jb : 0x7fffffff);
            mx = wave_max(any ? je : -1);
        }
        const int span = mx - mn;
        // A window wider than the staging area is mostly a wave across two cell rows: its lanes' ranges
        // form two runs far apart.  Split the lanes at the widest gap (a lane whose range starts past
        // every earlier lane's end) and stage each run's window, one after the other, when both fit.
        int lbase = mn, n1 = span, m2 = 0, n2 = 0;   // lane's record index j - lbase; the two windows
        bool two = false;
        if (span > kCap32) {   // wave-uniform, rare
            int pm = any ? je : -1;   // running max of the ends over the lanes below and at this one
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(pm, o, 64);
                if (lane >= o) pm = max(pm, v);
            }
            int ex = __shfl_up(pm, 1, 64);
            if (lane == 0) ex = -1;
            const int gap = any && ex >= 0 ? jb - ex : -1;
            const int gmax = wave_max(gap);
            if (gmax > 0) {
                const int sl = __ffsll((long long)__ballot(gap == gmax)) - 1;
                const bool hi_run = lane >= sl;
                const int m1 = wave_min(any && !hi_run ? jb : 0x7fffffff);
                const int x1 = __builtin_amdgcn_readlane(ex, sl);   // the low run's end
                m2 = wave_min(any && hi_run ? jb : 0x7fffffff);
                n1 = x1 - m1;
                n2 = mx - m2;
                if (n1 + n2 <= kCap32) {
                    two = true;
                    lbase = hi_run ? m2 - n1 : m1;
                    mn = m1;
                }
            }
        }
        if (span <= kCap32 || two) {
            // FP32 records: candidate j at record j - lbase, 64 records (1 KB) per instruction
            float4* s4 = reinterpret_cast<float4*>(sx);
            for (int p = 0; p * 64 < n1; ++p)   // wave-uniform
                if (p * 64 + lane < n1) __builtin_amdgcn_global_load_lds(A.f4 + gb + mn + p * 64 + lane, s4 + p * 64, 16, 0, 0);
            for (int p = 0; p * 64 < n2; ++p)   // the second run (two), after the first
                if (p * 64 + lane < n2)
                    __builtin_amdgcn_global_load_lds(A.f4 + gb + m2 + p * 64 + lane, s4 + n1 + p * 64, 16, 0, 0);
            __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): the records (and column col + 1's start[]) landed
            __builtin_amdgcn_wave_barrier();
            const float xf = (float)(xi - P.cref[0]), yf = (float)(yi - P.cref[1]), zf = (float)(zi - P.cref[2]);
            const float lof = P.rc2f_lo, hif = P.rc2f_hi;
            auto test32 = [&](auto self_tag) {
                constexpr bool SELF = decltype(self_tag)::value;
                const int self = SELF ? i - gb : 0;
                for (int j0 = jb; j0 < je; j0 += SB) {
                    float4 r[SB];
#pragma unroll
                    for (int u = 0; u < SB; ++u) r[u] = s4[j0 - lbase + u];
#pragma unroll
                    for (int u = 0; u < SB; ++u) {
                        const int j = j0 + u;
                        const float dx = r[u].x - xf, dy = r[u].y - yf, dz = r[u].z - zf;
                        const float r2f = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
                        bool live = true;
                        if (u > 0) live = j < je;
                        if (SELF) live = live & (j != self);
                        if constexpr (LEAN) {
                            if (live & (r2f <= P.rlf)) {
                                put(j, __float_as_int(r[u].w), soff & kSoffMask);
                                soff += kListKeep;
                            }
                            continue;
                        }
                        // two compares; the band as wave masks (SALU), its lane bit read only inside
                        // the rare branch
                        const bool le_lo = r2f <= lof, le_hi = r2f <= hif;
                        bool a = live & le_lo;
                        const unsigned long long mband = __builtin_amdgcn_ballot_w64(le_hi) &
                                                         ~__builtin_amdgcn_ballot_w64(le_lo) &
                                                         __builtin_amdgcn_ballot_w64(live);
                        if (mband) {   // rare (wave-uniform): the FP64 test on the global positions
                            // the band lanes straight from the mask (no per-lane compare)
                            if (__builtin_amdgcn_inverse_ballot_w64(mband)) {
                                // the index hidden from the loop's induction analysis, so the addresses
                                // are formed here and not carried through the loop
                                // (S16: the base read again here, not held through the loop)
                                int jj = S16 ? j + sbase[col / GSZ] : j;
                                asm volatile("" : "+v"(jj));
                                const double ddx = A.x[jj] - xi, ddy = A.y[jj] - yi, ddz = A.z[jj] - zi;
                                const double r2a = fma(ddx, ddx, fma(ddy, ddy, ddz * ddz));
                                const bool in = r2a <= lo2;
                                a = in;
                                if ((r2a <= hi2) != in) a = accept_band(P, ddx, ddy, ddz);
                            }
                        }
                        if (a) {
                            // stored when within the passes' largest radius (FP32, an upper bound:
                            // the passes' own exact tests decide); counted always
                            const bool keep = r2f <= P.rlf;
                            if (keep) put(j, __float_as_int(r[u].w), soff & kSoffMask);
                            soff += keep ? kListKeep : kListTotal;
                        }
                    }
                }
            };
            if (col == kSelfCol) test32(std::true_type{});
            else test32(std::false_type{});
            __builtin_amdgcn_wave_barrier();   // every lane done reading before the next staging
        } else if constexpr (S16) {
            // a window wider than the staging area (rare): the wave starts over in the wide format,
            // whose gather loop takes it
            __builtin_amdgcn_s_waitcnt(0x0F70);   // column col + 1's start[] loads
            return true;
        } else {
            // a window wider than the staging area: per-lane gathers, every accepted pair stored
            for (int j0 = jb; j0 < je; j0 += SB) {
                double xs[SB], ys[SB], zs[SB];
#pragma unroll
                for (int u = 0; u < SB; ++u) {
                    const int j = j0 + u < je ? j0 + u : je - 1;
                    xs[u] = A.x[j];
                    ys[u] = A.y[j];
                    zs[u] = A.z[j];
                }
#pragma unroll
                for (int u = 0; u < SB; ++u) {
                    const int j = j0 + u;
                    if (accept_interior(P, xs[u] - xi, ys[u] - yi, zs[u] - zi, lo2, hi2) && j < je && j != i) {
                        const int row = soff_stored(S16, soff);
                        if (soff_total(soff) < kMaxNeighbor && row < kTileRows)
                            out[(size_t)row * kTile] = nbr_entry(j, A.type[j]);
                        soff += kListKeep;
                    }
                }
            }
            __builtin_amdgcn_s_waitcnt(0x0F70);   // column col + 1's start[] loads (wide windows are rare)
        }
        return false;
    };
    int ra_b, ra_e, rb_b = 0, rb_e = 0;   // the two register pairs of the column ranges
    col_range(0, ra_b, ra_e);
    __builtin_amdgcn_s_waitcnt(0x0F70);
    for (int col = 0; col < NCOL; col += 2) {
        bool again = column(col, ra_b, ra_e, rb_b, rb_e);
        if (!again && col + 1 < NCOL) again = column(col + 1, rb_b, rb_e, ra_b, ra_e);
        if (S16 && again) {
            if (lane == 0) *hdr_byte(kHdrRestartByte) = 1;
            __builtin_amdgcn_s_waitcnt(0x0F70);   // the 16-bit stores done before the wide ones over them
            return -1;
        }
    }
    *stored = soff_stored(S16, soff);  // the list's rows, gaps included (entries: r^2 <= P.rlf)
    // header byte 7: the jumps and the wave's flags (mph_params.h kHdrShort)
    if (S16) {
        if (lane == 0) *hdr_byte(7) = (unsigned char)(kMaxJumps | kHdrShort | (jumps & kGapsBit ? 0u : kHdrNoGap));
    } else {
        if (lane == 0) *hdr_byte(7) = (unsigned char)(jumps > kMaxJumps ? jumps - kMaxJumps - 1 : jumps);
    }
    return soff_total(soff);      // every neighbour (NeighborCount; LEAN: the stored entries)
}

// Slab mode: wface[w] = 1 when wave w holds an owned particle within slab_h of a slab face (pass B
// runs it after the halo, phase 2, and the early send takes its particles), else 0 (interior
// waves and waves of ghosts only, phase 1).  Written by the search, so that each pass-B launch
// drops the other's waves with one load; the redistribution of the next step reads it too.
__device__ __forceinline__ void slab_wave_flag(const DevParams& P, const Soa& A, int i, int n, int* wface)
{
    if (P.slab_axis < 0 || !wface) return;
    const bool live = i < n;
    const int ii = live ? i : n - 1;
    const bool own = live && A.id[ii] >= 0;
    const double c = P.slab_axis == 0 ? A.x[ii] : (P.slab_axis == 1 ? A.y[ii] : A.z[ii]);
    const bool inner = c - P.slab_lo > P.slab_h && P.slab_hi - c > P.slab_h;
    const bool face = !__all(!own || inner);
    if ((threadIdx.x & 63) == 0) wface[i >> 6] = face ? 1 : 0;
}

// Lazy wall steps (mph_params.h kCoarseShift; cmap: this step's coarse map of the non-wall
// particles, from k_prep): true when the wave is idle -- every live lane is a wall, the wave is
// interior (wave_search_interior: no stencil wraps), and no coarse cell that a lane's stencil can
// reach holds a non-wall particle.  The bound is geometric and conservative: each lane takes the
// box of its own cell widened by kReach cells on every axis (the stencil reaches kReach cells
// across the columns and kContigReach <= kReach along the contiguous axis; clamping the box to the
// grid loses nothing for an interior lane), at most 3 x 3 x 3 coarse cells, and one ballot decides.
// (The lanes' own boxes, not the box of the wave's cells shared out over the lanes: no wave-wide
// minima and maxima, no cap for a wave that straddles two walls, and a tighter bound; the wave-box
// form took the 3-D search from 63 VGPRs to 13 spilled ones.)  No list of a non-wall particle then
// holds a lane of this wave, and on a step that stores no output-only field nothing else reads
// what the search and pass A compute for it (enqueue_step).  The wave gets empty lists, as a wave
// of ghosts does, and is counted in its run of the waves like the work histogram (never one same-
// address atomic per wave, see neighbors_body).  It runs ahead of neighbors_body on values of its
// own, which end with it: the search's register budget is the parent's.
template <int DIM, bool LEAN>
__device__ __forceinline__ bool wave_idle_walls(const DevParams& P, const Soa& A, const unsigned char* cmap,
                                                DevState* st, int* ncount, int* nbcount,
                                                unsigned long long* lhdr, int i, int n)
{
    static_assert(kContigReach <= kReach, "the box is widened by kReach on every axis");
    static_assert(2 * kReach < 2 << kCoarseShift, "a lane's box spans at most 3 coarse cells per axis");
    const int tile = __builtin_amdgcn_readfirstlane(i >> 6);
    if (tile * kTile >= n) return false;
    const bool live = i < n;
    int ii = live ? i : n - 1;
    asm volatile("" : "+v"(ii));   // (its loads are not kept for neighbors_body)
    if (!__all(!live || dev_is_wall(A.type[ii]))) return false;
    const double xi = A.x[ii], yi = A.y[ii], zi = A.z[ii];
    if (!wave_search_interior(P, st, live, xi, yi, zi)) return false;
    const int cx = cell_axis(xi, P.corg[0], P.dw[0], P.ginv[0], P.gc[0]);
    const int cy = cell_axis(yi, P.corg[1], P.dw[1], P.ginv[1], P.gc[1]);
    const int cz = DIM == 3 ? cell_axis(zi, P.corg[2], P.dw[2], P.ginv[2], P.gc[2]) : 0;
    const int ax = max(cx - kReach, 0) >> kCoarseShift, bx = min(cx + kReach, P.gc[0] - 1) >> kCoarseShift;
    const int ay = max(cy - kReach, 0) >> kCoarseShift, by = min(cy + kReach, P.gc[1] - 1) >> kCoarseShift;
    const int az = DIM == 3 ? max(cz - kReach, 0) >> kCoarseShift : 0;
    const int bz = DIM == 3 ? min(cz + kReach, P.gc[2] - 1) >> kCoarseShift : 0;
    const int ny = coarse_cells(P.gc[1]), nz = coarse_cells(P.gc[2]);
    int hit = 0;
#pragma unroll 1
    for (int kx = 0; kx < 3; ++kx) {
#pragma unroll 1
        for (int ky = 0; ky < 3; ++ky) {
            const unsigned char* row = cmap + (min(ax + kx, bx) * ny + min(ay + ky, by)) * nz;
            hit |= row[az] | row[min(az + 1, bz)] | row[bz];
        }
    }
    if (__ballot(hit != 0)) return false;
    if (live) ncount[i] = 0;
    if (!LEAN && live) nbcount[i] = 0;   // (a lean step stores no NeighborCount)
    if ((threadIdx.x & 63) == 0) {
        lhdr[tile] = 0;
        atomicAdd(&st->idle_waves[(int)(((long long)tile * kXcdSegs) / ((n + 63) >> 6))], 1u);
    }
    return true;
}

// The format of an interior 3-D wave's rows, decided before its first store: for each stencil group
// (slowest-axis offset g - kReach) every index a lane can store lies in [start[lo_g], start[hi_g]),
// the cell-order indices of the group's first cell seen from the wave's lowest cell and of the cell
// past its last seen from the wave's highest (an interior wave's stencil wraps nowhere, so a cell's
// index is the lane's own plus the stencil offset, and start[] is monotone).  Lane g loads the lower
// bound and lane 8 + g the upper one, one load instruction for the wave; the wave is short when
// every span is at most DevParams.list16_span, and then the lower bounds are the groups' bases:
// sbase (the wave's LDS, for its search) and lbase (the passes').
template <int PERM>
__device__ __forceinline__ bool wave_list16(const DevParams& P, const int* start, bool own, int cx, int cy, int cz,
                                            int tile, int* sbase, int* lbase, unsigned long long* lhdr)
{
    using X = CellAxes<3, PERM>;
    if (P.list16_span <= 0 || !__ballot(own)) return false;   // wave-uniform
    const int cc[3] = {cx, cy, cz};
    const int g1 = P.gc[X::A1], g2 = P.gc[X::A2];
    const int lin = (cc[X::A0] * g1 + cc[X::A1]) * g2 + cc[X::A2];
    const int lmin = __builtin_amdgcn_readfirstlane(wave_min(own ? lin : 0x7fffffff));
    const int lmax = __builtin_amdgcn_readfirstlane(wave_max(own ? lin : -1));
    const int lane = threadIdx.x & 63;
    const int g = lane & 7, dg = g - kReach;
    const bool hi = lane >= 8;
    int idx = hi ? lmax + (dg * g1 + kReach) * g2 + P.sa + 1 : lmin + (dg * g1 - kReach) * g2 - P.sa;
    idx = min(max(idx, 0), P.ncell);   // (an interior wave's are inside; start[] has ncell + 1 entries)
    const int v = lane < 16 && g < kGroups ? start[idx] : 0;
    const int span = __shfl_down(v, 8, 64) - v;
    if (__ballot(lane < kGroups && (span < 0 || span > P.list16_span))) {
        // (counted apart from the waves that never decide: mph_list_span_misses)
        if (lane == 0) reinterpret_cast<unsigned char*>(lhdr + tile)[kHdrRestartByte] = kHdrSpanMiss;
        return false;
    }
    if (lane < kGroups) {
        sbase[lane] = v;
        lbase[(size_t)tile * kBaseInts + lane] = v;
    }
    __builtin_amdgcn_wave_barrier();
    return true;
}

// ncount: the rows of each particle's stored list, gaps included (what the passes walk; the
// entries, r^2 <= P.rlf, are the rows outside the gaps, RowMask); nbcount: NeighborCount, every
// neighbour within the search radius; lhdr / lgap: the row jumps (RowMask)
// LEAN (a lean step, scan_candidates_lds): nbcount is not stored -- it has no reader before the
// batch's last step, which is full -- and the overflow flag follows the stored entries.
template <int DIM, int PERM, bool LEAN>
__device__ __forceinline__ int neighbors_body(const DevParams& P, const Soa& A, const int* start, int* nbr,
                                               int* ncount, int* nbcount, unsigned long long* lhdr,
                                               unsigned long long* lgap, DevState* st, double* stage, int i,
                                               int* lbase)
{
    const int n = dev_n(P);
    const bool live = i < n;
    const int ii = live ? i : n - 1;
    const int tile = __builtin_amdgcn_readfirstlane(i >> 6);
    // a wave past the last particle (the launch has whole blocks of 4 waves): nothing to do, and its
    // tile lies past the list array (sized for the particles' tiles)
    if (tile * kTile >= n) return 0;
    if (wave_all_ghosts(P, A, live, ii)) {
        if (live) ncount[i] = 0;
        if (live) nbcount[i] = 0;
        if ((threadIdx.x & 63) == 0) lhdr[tile] = 0;
        return 0;
    }
    // the ghost lanes of a mixed wave take no part either (empty list)
    const bool own = live && !(P.slab_axis >= 0 && A.id[ii] < 0);
    const double xi = A.x[ii], yi = A.y[ii], zi = A.z[ii];
    const bool fast = wave_search_interior(P, st, own, xi, yi, zi);
    int cnt = 0, stored = 0;
    const int cx = cell_axis(xi, P.corg[0], P.dw[0], P.ginv[0], P.gc[0]);
    const int cy = cell_axis(yi, P.corg[1], P.dw[1], P.ginv[1], P.gc[1]);
    const int cz = DIM == 3 ? cell_axis(zi, P.corg[2], P.dw[2], P.ginv[2], P.gc[2]) : 0;
    // the lane's column of its wave's tile (formed where it is used: no register holds it across
    // the format decision or the short form)
    auto tile_out = [&](int iv) { return nbr + (size_t)(iv >> 6) * kTileStride + (iv & 63); };
    if (fast) {
        // 16-bit rows where the wave's spans allow (3-D); a short wave that runs out of aligned rows
        // starts over in the wide format
        bool s16 = false;
        if constexpr (DIM == 3) {
            // (header byte kHdrRestartByte: cleared here, set by a short wave that starts over)
            if ((threadIdx.x & 63) == 0) reinterpret_cast<unsigned char*>(lhdr + tile)[kHdrRestartByte] = 0;
            s16 = wave_list16<PERM>(P, start, own, cx, cy, cz, tile, stage_bases(stage), lbase, lhdr);
            cnt = -1;
            if (s16) {
                int is = i;
                asm volatile("" : "+v"(is));
                cnt = scan_candidates_lds<DIM, PERM, LEAN, true>(P, A, start, i, own, xi, yi, zi, cx, cy, cz,
                                                                 tile_out(is), stage, &stored, lgap, lhdr);
            }
        }
        if (DIM != 3 || cnt < 0) {
            // (3-D: the cells and the tile pointer are formed again from the position and the index,
            // so that the short form holds no register for a restart)
            double xw = xi, yw = yi, zw = zi;
            int iw = i;
            int g0 = P.gc[0], g1 = P.gc[1], g2 = P.gc[2];   // (likewise what cell_axis derives from them)
            if (DIM == 3) asm volatile("" : "+v"(xw), "+v"(yw), "+v"(zw), "+v"(iw), "+s"(g0), "+s"(g1), "+s"(g2));
            const int cxw = DIM == 3 ? cell_axis(xw, P.corg[0], P.dw[0], P.ginv[0], g0) : cx;
            const int cyw = DIM == 3 ? cell_axis(yw, P.corg[1], P.dw[1], P.ginv[1], g1) : cy;
            const int czw = DIM == 3 ? cell_axis(zw, P.corg[2], P.dw[2], P.ginv[2], g2) : 0;
            cnt = scan_candidates_lds<DIM, PERM, LEAN, false>(P, A, start, i, own, xw, yw, zw, cxw, cyw, czw,
                                                              tile_out(iw), stage, &stored, lgap, lhdr);
        }
    } else {
        if (own)
            cnt = scan_candidates<DIM, PERM>(P, A, start, i, xi, yi, zi, cx, cy, cz, tile_out(i));
        stored = cnt;
        if ((threadIdx.x & 63) == 0) lhdr[tile] = 0;   // plain rows
    }
    if (live) ncount[i] = stored;
    if (!LEAN && live) nbcount[i] = cnt;
    // overflow flag (main.cpp:1766-1768 is the reference's limit).  No per-step statistics here:
    // one same-address device atomic per wave serialises at ~11 ns each (21.8k waves at D1M took
    // 0.5 ms); mph_neighbor_stats reduces ncount on demand.
    if (cnt > kMaxNeighbor) atomicOr(&st->overflow, 1);
    return stored;
}

// one kernel per cell order (DevParams.perm), so each keeps its own register budget; held to 64
// VGPRs (8 waves per SIMD: the search waits on its start[] and staging loads).  bal: the passes'
// XCD split runs (launch_sort), so the waves feed its histogram.
#ifndef MPH_NB_WPE
#define MPH_NB_WPE 8
#endif
// LAZY: a lazy wall step's search (cmap set); a full step's is a kernel of its own, so that it keeps
// the registers it had before the lazy steps (their map and histograms cost the search ~50 SGPR
// spills and 1.3 % at D1M when both were one kernel).
// LEAN: a lean step's search (LAZY too: scan_candidates_lds<.., LEAN>, neighbors_body), a third kernel.
template <int DIM, int PERM, bool LAZY, bool LEAN = false>
__global__ __launch_bounds__(MPH_LB) __attribute__((amdgpu_waves_per_eu(MPH_NB_WPE))) void k_neighbors(
    DevParams P, Soa A, const int* __restrict__ start, int* __restrict__ nbr, int* __restrict__ ncount,
    int* __restrict__ nbcount, unsigned long long* __restrict__ lhdr, unsigned long long* __restrict__ lgap,
    DevState* __restrict__ st, int* __restrict__ wface, int bal, const unsigned char* __restrict__ cmap_arg,
    int* __restrict__ lbase)
{
    const unsigned char* cmap = LAZY ? cmap_arg : nullptr;
    const int n = dev_n(P);
    static_assert(LAZY || !LEAN, "only a lazy step is lean");
    if (cmap && blockIdx.x == 0 && threadIdx.x == 0) {   // (the one writer)
        st->lazy_steps += 1;
        if (LEAN) st->lean_search_steps += 1;
    }
    // the wave's block: a lazy step with the XCD split takes the map made from the last lazy step's
    // search costs (list_block over xcd_sfrac, a list_grid launch), else the equal ranges
    int tb;
    if (cmap && bal) {
        tb = list_block(st->xcd_sfrac, n);
        if (tb < 0) return;
    } else {
        if ((int)blockIdx.x >= list_blocks(n)) return;
        tb = xcd_block(blockIdx.x, list_blocks(n));
    }
    // (3-D: a short wave's group bases behind its staging area, stage_bases: 32 bytes per wave,
    // inside what the staging areas leave of a CU's LDS at 8 waves per SIMD)
    __shared__ __attribute__((aligned(16))) double stage[kWB][stage_words(MPH_LDS_CAP, MPH_SB) +
                                                              (DIM == 3 ? kBaseInts / 2 : 0)];
    const int i = tb * blockDim.x + threadIdx.x;
    slab_wave_flag(P, A, i, n, wface);
    // a lazy wall step (cmap set): an idle wave of walls only adds its fixed costs to the histograms
    const bool idle = cmap && wave_idle_walls<DIM, LEAN>(P, A, cmap, st, ncount, nbcount, lhdr, i, n);
    const int cnt = idle ? 0
                         : neighbors_body<DIM, PERM, LEAN>(P, A, start, nbr, ncount, nbcount, lhdr, lgap, st,
                                                     stage[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)], i, lbase);
    if (bal) {
        if (cmap) add_wave_work(st->seg_lwork, cnt, i, n, st->seg_swork, idle);
        else add_wave_work(st->seg_work, cnt, i, n);
    }
}

// ---------------------------------------------------------------------------- launchers -----

void launch_neighbors(const Launch& L)
{
    const DevParams& P = *L.P;
    if (P.n == 0) return;
    // a lean step's search (lean_search_ok is asked again here for a caller that changed rlf after
    // the context was filled, as virial_full_lists does)
    const bool lean = L.form.lazy && L.form.lean_search && lean_search_ok(P);
    by_dim(P.dim, [&](auto D) {
        constexpr int DIM = decltype(D)::value;
        auto go = [&](auto PERM) {
            by_flag(L.form.lazy, [&](auto LAZY) {
                by_flag(lean, [&](auto LEAN) {
                    if constexpr (decltype(LAZY)::value || !decltype(LEAN)::value)   // (only a lazy step is lean)
                        launch(L.prof, "neighbors", L.stream,
                               k_neighbors<DIM, decltype(PERM)::value, decltype(LAZY)::value, decltype(LEAN)::value>,
                               dim3(lazy_bal(L) ? list_grid(P.n, true) : blocks(P.n, MPH_LB)), dim3(MPH_LB), P, L.A,
                               L.start, L.nbr, L.ncount, L.nbcount, L.lhdr, L.lgap, L.st, L.wface, (int)xcd_bal(L),
                               lazy_cmap(L), L.lbase);
                });
            });
        };
        if constexpr (DIM == 3) {   // (the 2-D grid has the one cell order)
            switch (P.perm) {
            case 1: go(Int<1>{}); break;
            case 2: go(Int<2>{}); break;
            case 3: go(Int<3>{}); break;
            case 4: go(Int<4>{}); break;
            default: go(Int<0>{}); break;
            }
        } else {
            go(Int<0>{});
        }
    });
}

}  // namespace mph
