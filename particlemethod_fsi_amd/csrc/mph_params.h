// mph_params.h -- plain-old-data structures shared by the host layer (mph_host.cpp) and the
// HIP kernels (mph_kernels.h).  No HIP types here, so the host files build with g++/hipcc alike.
#pragma once
#include <cmath>

#include <cstddef>
#include <cstdint>

#include "../../include/mph_gpu.h"


namespace mph {

constexpr int kTypes = MPH_TYPE_COUNT;
constexpr int kMaxNeighbor = MPH_MAX_NEIGHBOR_COUNT;
constexpr int kTile = 64;  // ELL neighbour-list tile = one wavefront of i-particles
// Aligned rows (round 6): at the end of a stencil group the search may move
// every lane of a wave on to the wave's highest row, so that the lanes write (and the passes read)
// the rows of the next group together however far their per-column counts drifted apart.  The
// rows a lane skips are gaps; they all lie below kAlignRows (a wave jumps only while its highest
// row is below it), so a lane's list is its rows [0, end) minus at most kMaxJumps gaps, and from
// kAlignRows on it is contiguous.  A tile therefore holds kMaxNeighbor + kAlignRows rows.
constexpr int kAlignRows = 128;
constexpr int kMaxJumps = 6;   // one per interior stencil group end (7 groups)
#ifndef MPH_TILE_EXTRA
#define MPH_TILE_EXTRA kAlignRows   // (A/B diagnostics only: the tile's rows past kMaxNeighbor)
#endif
constexpr int kTileRows = kMaxNeighbor + MPH_TILE_EXTRA;
// Ints from one wave's list tile to the next: kTileRows rows of 64, plus MPH_TILE_PAD rows, so
// that the tiles do not all start on the same power-of-two boundary.  One row: the search 3-4 %
// faster at rest and in the developed flow (five same-box rounds; 4 and 9 rows no faster; the
// list's write-backs unchanged), steps within noise (profiles/r05/tile_pad/)
#ifndef MPH_TILE_PAD
#define MPH_TILE_PAD 1
#endif
constexpr int kTileStride = kTile * (kTileRows + MPH_TILE_PAD);
// Slot of entry k of lane `lane` in its wave's tile (ints): entry k of the 64 lanes in one 256-byte
// row, [k][lane].  (Entries in pairs or fours side by side, rows per half-wave and rows spread by the
// last step's NeighborCount were measured in round 5 and rejected: DESIGN.md section 3.3.)
#if defined(__HIPCC__)
__host__ __device__
#endif
constexpr inline int ell_slot(int k, int lane)
{
    return (k << 6) | lane;
}
// Stencil reach along the contiguous axis: cells there are >= rc / kContigReach wide, and a
// column is the one index range of +-kContigReach cells (thin cells only sharpen the cutoff
// trimming of each column)
#ifndef MPH_SA
#define MPH_SA 2   // rc/2 cells along the contiguous axis (D1M scans 0.048 -> 0.036 ms; rc/3: search -0.006 ms)
#endif
constexpr int kContigReach = MPH_SA;
// Stencil reach across the two outer (column) axes: cells there are >= rc / kReach wide, so a
// +-kReach stencil of (2 kReach + 1)^2 columns covers the acceptance sphere.  kReach = 3 makes the
// cells (rc / 3 = 0.87 dx at RadiusRatio 2.5) narrower than the lattice spacing, so a cell row
// holds one lattice line and a wavefront is a run along that line: the 64 lanes' k-th neighbours
// are then consecutive particles of one neighbour row (coherent gathers in the list passes).
#ifndef MPH_R
#define MPH_R 3
#endif
constexpr int kReach = MPH_R;
constexpr int kGroups = 2 * kReach + 1;   // stencil columns per axis across the column axes
// ELL list entry = sorted index | (type << kTypeShift): pass A reads the neighbour's type with
// its index instead of gathering it (requires fewer than 2^28 particles per context)
constexpr int kTypeShift = 28;
// The list passes gather through buffer descriptors with 32-bit byte offsets; a row without an
// entry of the lane takes this offset, past every record, so the hardware returns zeros without a
// memory access (no cache lookup)
constexpr unsigned kGatherOob = 0xFFFFFFC0u;
constexpr int kIndexMask = (1 << kTypeShift) - 1;
// 16-bit list rows: a 3-D interior wave whose candidates of every stencil
// group (the kGroups columns of one slowest-axis offset) lie within kList16Span indices of a wave-
// uniform base stores its entries as (index - base[group]) | type << kOff16Bits in rows of 64
// uint16 (128 bytes, the first half of its tile); its kBaseInts bases live in a per-wave array
// beside the header words.
constexpr int kOff16Bits = 13;
constexpr int kOff16Mask = (1 << kOff16Bits) - 1;
constexpr int kList16Span = kOff16Mask;
constexpr int kBaseInts = 8;   // kGroups bases and one spare int per wave
static_assert(MPH_TYPE_COUNT <= (1 << (16 - kOff16Bits)), "a 16-bit list entry has 3 type bits");
static_assert(2 * MPH_R + 1 < kBaseInts, "one base per stencil group");
constexpr int kPad = 8;         // extra elements behind every per-particle array (vector over-reads)

inline bool is_fluid(int t) { return t >= 0 && t < 2; }   // main.cpp:69-70
inline bool is_struct(int t) { return t >= 2 && t < 4; }  // main.cpp:71-72
inline bool is_wall(int t) { return t >= 4 && t < 6; }    // main.cpp:73-74

// Axis of the 3-D cell order DevParams.perm at position k (0 slowest, 2 contiguous):
// 0 (x, y, z); for z slabs 1 (z, x, y), 2 (z, y, x), 3 (y, z, x), 4 (x, z, y)
inline constexpr int order_axis(int perm, int k)
{
    return perm == 1 ? (k == 0 ? 2 : k == 1 ? 0 : 1)
         : perm == 2 ? (k == 0 ? 2 : k == 1 ? 1 : 0)
         : perm == 3 ? (k == 0 ? 1 : k == 1 ? 2 : 0)
         : perm == 4 ? (k == 0 ? 0 : k == 1 ? 2 : 1)
                     : k;
}
// the contiguous (half-width-cell) axis of the cell order
inline constexpr int contig_axis(int dim, int perm) { return dim == 2 ? 1 : order_axis(perm, 2); }

// Every constant the reference derives in initializeWeight/Fluid/Wall/Domain
// (main.cpp:1191-1469), in the reference's own arithmetic, plus what the GPU path precomputes.
// Passed by value as a kernel argument (kernarg segment -> scalar loads).
struct DevParams {
    int n;             // particles held by this context (slab mode: the array capacity, a bound)
    // slab mode: the device-resident particle count (DistLayout.n), which the kernels read so
    // that a step needs no host round trip for sizes; null on a single GPU (n is exact)
    const int* n_dev;
    int dim;           // 2 or 3
    int module;        // MphModule
    int wall_motion;   // MphWallMotion
    int surface;      // any CofA != 0 -> surface-tension terms live (K12/K13)
    int n_struct;      // structure particles (types 2,3)
    int gc[3];         // GPU linked-cell grid (gc[2] == 1 in 2-D)
    int ncell;         // gc[0]*gc[1]*gc[2]
    int substeps;      // (int)(Dt/Elastic_Dt + 0.5), main.cpp:653
    int sa;            // stencil half-width (cells) along the contiguous axis (kContigReach)
    // linear order of the 3-D cell grid (order_axis above): 0 = (x, y, z) with z contiguous; z
    // slabs (mph_dist.hip) put z in the middle, 3 = (y, z, x) or 4 = (x, z, y), so that the ghosts
    // beyond both faces form long runs at the two ends of every plane of the slowest axis (whole
    // wavefronts the list kernels skip) while every XCD's contiguous share of the sorted arrays
    // stays a band of that slowest axis through the whole slab (L2 locality); 1, 2 put z slowest
    int perm;
    int fast_ok;       // every active axis has > 12 GPU cells: interior waves may skip the
                       // periodic branch of the minimum image (see k_neighbors)
    double inner_lo[3], inner_hi[3];   // interior box: >= 3 GPU cells from every periodic face
    // the search's interior box in grid offsets (position - corg, wrapped into [0, dw)): >= 3
    // cells from the grid's faces.  The grid origin corg may sit inside an empty band of the
    // domain (choose_grid_origin), so particles at a periodic face of the domain can be interior
    // to the grid; their waves then need the face box above only while particles lie within it at
    // both ends of that axis (DevState.seam_occ) or on the slab axis (seam_always bit)
    double sinner_lo[3], sinner_hi[3];
    int seam_always;
    // 16-bit list rows (kOff16Bits below): the widest index span of a stencil group's candidates a
    // wave may have and still take them; 0: every wave keeps the 32-bit rows (MPH_LIST16=0, 2-D,
    // slab contexts).  (In the padding behind seam_always: every other member keeps its offset.)
    int list16_span;
    double dmin[3], dw[3], hw[3], w075[3];   // domain min / width / half width / 0.75 width
    double corg[3];    // origin of the GPU cell grid (dmin, or the slab window's lower edge)
    double ginv[3];    // 1 / GPU cell width per axis
    // slab mode: particles within slab_h of a slab face may have ghost neighbours (pass B runs
    // them after the halo exchange); slab_axis = -1 outside slab mode
    int slab_axis;
    double slab_lo, slab_hi, slab_h;
    double rc2;        // (MaxRadius + MARGIN)^2, main.cpp:1765
    double ra, rg, rp, rv;                   // radii (main.cpp:1195-1198)
    double ra2, rg2, rp2, rv2;               // radius*radius as the reference compares them
    double inv_ra, inv_rg, inv_rp, inv_rv;
    // kernel prefactors: wa = ca*t*(1-t)^2, dwa = cda*(1-t)*(1-3t), w_x = c_x*(1-t)^2,
    // dw_x = cd_x*(1-t)  with t = r/h (main.cpp:298-368)
    double ca, cda, cg, cdg, cp, cdp, cv, cdv;
    double cw;          // weight(): (1/Swp)/rp^dim (main.cpp:268-295)
    double n0a, n0p, r2g, cofk, dx, vol, dt, edt, cvis;
    double cw_pair;    // (1/Swp)(1/RadiusP^dim) of weight() for the elastic pairs (main.cpp:268-295)
    double gravity[3];
    double ratio[kTypes][kTypes];   // InteractionRatio
    double mu_ij[kTypes][kTypes];   // 2 mu_i mu_j / (mu_i + mu_j) from ShearViscosity
    double cofa[kTypes];            // CofA (main.cpp:1339-1341)
    double mass[kTypes], inv_mass[kTypes], density[kTypes], inv_density[kTypes];
    double bulk[kTypes], bulk_visc[kTypes];
    double wall_rot[kTypes][3][3];  // initializeWall (main.cpp:1371-1410)
    double wall_omega[kTypes][3];
    double wall_vel[kTypes][3];
    // Uniform FP64 constants the kernels would otherwise derive per lane (gfx9 has no scalar FP64
    // ALU: a value computed on the device occupies a VGPR pair for the whole loop it is hoisted
    // out of; from the kernel arguments it stays in SGPRs).  set_uniforms fills them.
    double rc2_lo, rc2_hi;   // rc2 (1 - 1e-10), rc2 (1 + 1e-10): the search's exact-test band
    double rc2_trim;         // rc2 (1 + 4e-6): the column-trimming bound
    double cwid[3];          // 1 / ginv: GPU cell widths
    double rg_r2g;           // rg / r2g (GravityCenter, DiffuseInterface)
    double cref[3];          // the domain centre the search's FP32 records are taken from
    float rc2f_lo, rc2f_hi;  // below lo the FP32 r^2 accepts, above hi it rejects (FP64 between)
    // The search stores a neighbour in the list only if its FP32 r^2 <= rlf: the largest radius of
    // the passes' sums (MaxRadius, main.cpp:1199) squared, widened by the FP32 records' error band,
    // so the list holds every pair any sum can take (the passes' exact tests decide) and not the
    // shell MaxRadius < r <= MaxRadius + MARGIN that the reference's list carries and NeighborCount
    // counts.  FLT_MAX (MPH_LIST_FULL=1): the reference's whole list.
    float rlf;
    // The lean search's column-trimming bound (a lean step: mph_kernels.h Launch.lean), in the place
    // rc2_trim has in the full search, as the FP32 value the trimming runs in.  (The last member, in
    // the struct's tail padding: the kernels' argument offsets are those of the builds before it.)
    float rl_trimf;
};
static_assert(offsetof(DevParams, rl_trimf) == offsetof(DevParams, rlf) + sizeof(float) &&
              offsetof(DevParams, rl_trimf) + sizeof(float) == sizeof(DevParams),
              "rl_trimf fills the tail padding behind rlf: the size is the one without it");
static_assert(offsetof(DevParams, list16_span) == offsetof(DevParams, seam_always) + sizeof(int) &&
              offsetof(DevParams, dmin) == offsetof(DevParams, list16_span) + sizeof(int),
              "list16_span fills the padding behind seam_always");

// Derived uniforms of DevParams (same expressions the kernels used, so the same bits).
inline void set_uniforms(DevParams& P)
{
    P.rc2_lo = P.rc2 * (1.0 - 1e-10);
    P.rc2_hi = P.rc2 * (1.0 + 1e-10);
    P.rc2_trim = P.rc2 * (1.0 + 4e-6);
    for (int d = 0; d < 3; ++d) P.cwid[d] = 1.0 / P.ginv[d];
    P.rg_r2g = P.rg / P.r2g;
    // FP32 records (the search's): coordinates within half a domain width of the centre, each
    // rounded once (<= 2^-24 x that); a difference is off by <= 2^-23 hw, r^2 near the cutoff by
    // <= 2 sqrt(3) 2^-23 hw / rc relative plus the FP32 sum's few ulp: the band is twice that
    double hwm = 0.0;
    for (int d = 0; d < 3; ++d) {
        P.cref[d] = P.dmin[d] + P.hw[d];
        hwm = P.hw[d] > hwm ? P.hw[d] : hwm;
    }
    const double rc = std::sqrt(P.rc2);
    const double delta = 2.0 * (2.0 * 1.7320508 * hwm * 1.1920929e-7 / rc) + 4.0e-6;
    P.rc2f_lo = (float)(P.rc2 * (1.0 - delta));
    P.rc2f_hi = (float)(P.rc2 * (1.0 + delta));
    const double rmax = std::fmax(std::fmax(P.ra, P.rg), std::fmax(P.rp, P.rv));
    P.rlf = (float)(rmax * rmax * (1.0 + delta));
    // The lean search trims its columns to the list radius.  It stores candidate j exactly when the
    // FP32 r^2 of the records, r2f, is <= rlf.  r2f is within delta (relative) of the exact r^2, and
    // rlf within 2^-24 of rmax^2 (1 + delta), so
    //     r2f <= rlf  =>  r^2 <= r2f (1 + delta) <= rmax^2 (1 + delta)^2 (1 + 2^-24) < rmax^2 (1 + delta)^3,
    // and with the cell geometry's 4e-6 of rc2_trim the bound is rmax^2 (1 + delta)^3 (1 + 4e-6): every
    // stored candidate lies inside the ranges trimmed to it.  Never wider than the full search's
    // bound (it is narrower whenever the lean search runs, lean_search_ok below); scan_candidates_lds
    // rounds it outwards once more (kUp), as it does rc2_trim.
    const double d1 = 1.0 + delta;
    P.rl_trimf = (float)std::fmin(rmax * rmax * d1 * d1 * d1 * (1.0 + 4e-6), P.rc2_trim);
}

// The lean search (mph_search.hip scan_candidates_lds<.., LEAN>) accepts with the one test
// r2f <= rlf.  That is the full search's stored set only while the list radius lies below the FP32
// band of the search radius: the full search stores live && a && r2f <= rlf, and r2f <= rlf <=
// rc2f_lo gives a = true without the FP64 test.  False under MPH_LIST_FULL=1 (rlf = FLT_MAX) and
// for a MARGIN so small that the two radii meet: the lazy steps then keep the full acceptance.
inline bool lean_search_ok(const DevParams& P) { return P.rlf <= P.rc2f_lo; }

// Lazy wall steps.  On a step whose output-only fields are not stored, a
// wall particle with no fluid or structure particle in reach is read by nobody: its neighbours are
// walls, and a wall walks no list in pass B on such a step.  k_prep marks, per step, the coarse
// cells that hold a non-wall particle (one byte each, blocks of 2^kCoarseShift grid cells per
// axis: 4 cells are 3.5 dx across the columns and 5.2 dx along the contiguous axis at RadiusRatio
// 2.5), and the search skips an interior wave of walls none of whose lanes' stencil boxes touches a
// marked cell (mph_search.hip wave_idle_walls).
constexpr int kCoarseShift = 2;
#if defined(__HIPCC__)
__host__ __device__
#endif
constexpr inline int coarse_cells(int g) { return (g + (1 << kCoarseShift) - 1) >> kCoarseShift; }
// bytes of the coarse map of a grid, a multiple of 16 (pass A clears it in 16-byte stores)
inline size_t coarse_map_bytes(const int gc[3])
{
    const size_t b = (size_t)coarse_cells(gc[0]) * coarse_cells(gc[1]) * coarse_cells(gc[2]);
    return (b + 15) & ~(size_t)15;
}

// work histogram of the XCD map: waves in 4096 equal runs (D16M: ~60 waves per run, so the
// search's per-wave atomics spread over ~100 addresses at a time; 512 runs cost its search 7 %)
constexpr int kXcdSegs = 4096;

// Mutable per-step device scalars (so a captured hipGraph can replay many steps).
struct DevState {
    double time;                 // Time
    double wall_c[kTypes][3];    // WallCenter (advanced by V*Dt every step, main.cpp:3066-3070)
    double wall_vel[kTypes][3];  // WallVelocity
    double wall_omega[kTypes][3];// WallOmega
    double wall_rot[kTypes][3][3];  // WallRotation (initializeWall)
    int overflow;                // error bits: 1 neighbour overflow (> MAX_NEIGHBOR_COUNT),
                                 // 2 slab jump (mph_dist), 4 non-finite position, 8 message
                                 // capacity (mph_dist), 64 inconsistent cell histogram
    int pad0;
    // particles within the face box margin of a periodic face, per axis (bit 2k: low face, 2k+1:
    // high face), gathered by k_prep into seam_occ[seam_step & 1]; k_place clears the other word
    // and advances seam_step, so the search reads seam_occ[(seam_step - 1) & 1]
    int seam_occ[2];
    int seam_step;
    int seam_pad;
    // work-balanced XCD map of the two list passes (mph_list.h, list_block): the search adds
    // each wave's work (its longest list + a fixed cost) into seg_work[its 1/kXcdSegs of the waves];
    // the next step's k_rank_scatter turns that into the XCDs' contiguous block ranges (xcd_frac:
    // fractions of 2^16, 0 ... 65536) for the passes and clears seg_work
    int seg_work[kXcdSegs];
    int xcd_frac[9];
    int xcd_pad[3];
    // lazy wall steps (kCoarseShift above): the steps searched with the idle-wave exit since the
    // creation, and the waves that took it -- counted like seg_work, one add per idle wave into
    // its run of the waves, summed on the host (mph_idle_wall_stats)
    unsigned long long lazy_steps;
    unsigned idle_waves[kXcdSegs];
    // The XCD maps of a lazy step.  Its idle waves are no work, and they lie together (at D1M the
    // far half of the tank: the last XCD's whole equal share of the search), so a lazy step keeps
    // histograms of its own, each turned into a map by the next lazy step's k_rank_scatter: the
    // passes' work as seg_work (seg_lwork -> xcd_frac, which a full step takes from seg_work, fed
    // by the last full step), and the search's -- a fixed cost per searched wave, a small one per
    // idle wave (kSearchCost, kIdleCost) -- for the search itself (seg_swork -> xcd_sfrac; a full
    // step's search keeps the equal ranges of xcd_block, mph_list.h)
    int seg_lwork[kXcdSegs];
    int seg_swork[kXcdSegs];
    int xcd_sfrac[9];
    int xcd_spad[3];
    // lean steps (Launch.lean), counted like lazy_steps: the lazy steps whose search ran its lean
    // form, and those whose pass A did, since the creation -- each bumped by block 0 of its kernel
    // (mph_lean_step_stats).  Behind every older member, whose offsets the other kernels keep.
    unsigned long long lean_search_steps, lean_pass_a_steps;
    // the key fold (mph_kernels.h seq_step), counted the same way since the creation: the steps whose
    // pass B left the next step's cell keys (bumped by block 0 of k_pass_b's KEYS form), and the
    // steps that opened with a k_prep launch (by k_place) -- mph_key_fold_stats
    unsigned long long key_fold_steps, prep_steps;
};
// the part of DevState the host reads back after steps (the error bits and the step scalars)
constexpr size_t kStateHead = offsetof(DevState, seg_work);

#if defined(__HIPCC__)
#define MPH_HD __host__ __device__
#else
#define MPH_HD
#endif

// The lists' row jumps (kAlignRows above; mph_list.h RowMask), decoded alike by the kernels and
// the host readers: byte 7 of a wave's header word is its jump count J; gap k < J of a lane is the
// rows [byte k of the lane's gap word, byte k of the header).
// The bits of byte 7 above the count are the wave's flags: kHdrShort, its rows are 16-bit ones (then
// J = kMaxJumps: every group end is a jump, so header byte g - 1 is the first row of group g);
// kHdrNoGap, none of a short wave's lanes has a gap (its rows are plain, no mask needed);
// Byte kHdrRestartByte (no jump's) is 1 in a wide wave that began in the 16-bit format and started over.
constexpr unsigned kHdrShort = 0x80, kHdrNoGap = 0x40;
constexpr int kHdrRestartByte = 6;
// (the same byte is kHdrSpanMiss in an interior wave that stayed wide because a group's span
// passed DevParams.list16_span)
constexpr unsigned kHdrSpanMiss = 2;
MPH_HD inline int jump_count(unsigned long long hdr) { return (int)(hdr >> 56) & 7; }
MPH_HD inline bool hdr_short(unsigned long long hdr) { return ((hdr >> 56) & kHdrShort) != 0; }
MPH_HD inline bool hdr_restarted(unsigned long long hdr) { return ((hdr >> (8 * kHdrRestartByte)) & 1) != 0; }
MPH_HD inline bool hdr_span_miss(unsigned long long hdr) { return ((hdr >> (8 * kHdrRestartByte)) & kHdrSpanMiss) != 0; }
// the jumps that may have left a gap in a lane (what a row mask is built from)
MPH_HD inline int gap_count(unsigned long long hdr) { return ((hdr >> 56) & kHdrNoGap) ? 0 : jump_count(hdr); }
MPH_HD inline int gap_begin(unsigned long long gap, int k) { return (int)((gap >> (8 * k)) & 0xff); }
MPH_HD inline int gap_end(unsigned long long hdr, int k) { return (int)((hdr >> (8 * k)) & 0xff); }

// A 16-bit entry and its parts; the stencil group of row k of a short wave (header byte g - 1 is
// the first row of group g; equal bytes: empty groups).
MPH_HD inline unsigned entry16(int off, int type) { return (unsigned)off | ((unsigned)type << kOff16Bits); }
MPH_HD inline int entry16_off(unsigned e) { return (int)(e & kOff16Mask); }
MPH_HD inline int entry16_type(unsigned e) { return (int)(e >> kOff16Bits); }
MPH_HD inline int row_group(unsigned long long hdr, int k)
{
    int g = 0;
    while (g < kMaxJumps && k >= gap_end(hdr, g)) ++g;
    return g;
}
// The same for rows visited in ascending order (the passes' list loops): the group of the last row
// asked for and the row its successor starts on (none after the last group).
struct GroupCursor {
    int g, nxt;
    MPH_HD void init(unsigned long long hdr)
    {
        g = 0;
        nxt = gap_end(hdr, 0);
    }
    // moves on to row k's group; true when the group changed
    MPH_HD bool seek(unsigned long long hdr, int k)
    {
        bool moved = false;
        while (k >= nxt) {
            ++g;
            nxt = g < kMaxJumps ? gap_end(hdr, g) : 0x7fffffff;
            moved = true;
        }
        return moved;
    }
};

// The search's per-lane store counter (mph_search.hip scan_candidates_lds), per format (s16: rows of
// 64 uint16): the lane's byte offset inside a row in the low bits (lane x 4 in bits 0-7, or lane x 2
// in bits 0-6), above it the row of the next stored entry -- the stored entries so far plus the
// gaps of the row jumps, up to 1023 (or 2047), so a lane that keeps all 512 entries the reference
// allows does not carry into the total -- and every accepted neighbour from bit 18.  The next list
// slot's byte offset in the wave's ELL tile is soff & kSoffMask; a row past the tile's kTileRows
// (only an overflowing lane, > 512 entries, the step's MPH_ERR_NEIGHBOR_OVERFLOW) is dropped by
// the tile's buffer descriptor, which spans kTileRows rows of the wave's format.
constexpr int kListTotal = 1 << 18, kSoffMask = 0x3FFFF;
MPH_HD constexpr int soff_row_shift(bool s16) { return s16 ? 7 : 8; }
MPH_HD constexpr int soff_first(bool s16, int lane) { return lane << (s16 ? 1 : 2); }
MPH_HD constexpr int soff_keep(bool s16) { return (1 << soff_row_shift(s16)) + kListTotal; }
MPH_HD constexpr int soff_total(int soff) { return (int)((unsigned)soff >> 18); }
MPH_HD constexpr int soff_stored(bool s16, int soff) { return (soff & kSoffMask) >> soff_row_shift(s16); }

// Pass A's single-cutoff form (pass_a_term<.., true>) when RadiusA = RadiusP = RadiusV (RadiusG =
// RadiusA, main.cpp:1195-1198), as in every BASELINE config.
#ifndef MPH_PA_EQR
#define MPH_PA_EQR 1
#endif
MPH_HD inline bool pass_a_equal_radii(const DevParams& P)
{
    return MPH_PA_EQR && P.ra == P.rp && P.rv == P.rp && P.rg == P.rp;
}

// Slab decomposition along one axis (multi-GPU, mph_dist.hip).  Rank r owns the particles whose
// (periodically wrapped) coordinate c satisfies lo <= c < hi, with the first/last rank also
// owning any roundoff spill below dmin / above dmax.  `h` is the halo width (>= the neighbour
// cutoff): owned particles within h of a face are mirrored to that neighbour as ghosts.
struct SlabGeom {
    int axis;
    int first, last, lfirst, llast, rfirst, rlast;   // first/last-rank flags: me, left, right
    double lo, hi, llo, lhi, rlo, rhi;               // slabs of me and my periodic neighbours
    double h;
    // elastic-solid particles are owned by the slab of their InitialPosition for good (their
    // fixed Lagrangian lists then never change rank); w = domain width along the axis, smargin =
    // how far beyond a face such a particle may be displaced (h includes it)
    double w, smargin;
};

// Particle classes of one step's redistribution, in the order of their segment in the local
// arrays: [migrate right | band right | inner | band left | migrate left]; kSlabDrop marks ghosts
// of the previous step, kSlabLost a particle that jumped past a neighbour's slab.
enum SlabClass { kMigR = 0, kBandR = 1, kInner = 2, kBandL = 3, kMigL = 4, kSlabDrop = 5,
                 kSlabClasses = 6, kSlabLost = 7 };

MPH_HD inline bool slab_owns(double c, double lo, double hi, int first, int last)
{
    return (first || c >= lo) && (last || c < hi);
}

MPH_HD inline int slab_class(const SlabGeom& g, double c)
{
    if (slab_owns(c, g.lo, g.hi, g.first, g.last)) {
        if (c - g.lo < g.h) return kBandL;
        if (g.hi - c <= g.h) return kBandR;
        return kInner;
    }
    if (slab_owns(c, g.llo, g.lhi, g.lfirst, g.llast)) return kMigL;
    if (slab_owns(c, g.rlo, g.rhi, g.rfirst, g.rlast)) return kMigR;
    return kSlabLost;
}

// Elastic-solid particle of this rank (never migrates): band by its periodic distance from the
// faces, lost if displaced more than smargin beyond one.
MPH_HD inline int slab_class_static(const SlabGeom& g, double c)
{
    const double half = 0.5 * (g.hi - g.lo);
    double off = c - (g.lo + half);
    off -= g.w * __builtin_floor(off / g.w + 0.5);
    const double dl = off + half, dr = half - off;
    if (dl < -g.smargin || dr < -g.smargin) return kSlabLost;
    if (dl < g.h) return kBandL;
    if (dr <= g.h) return kBandR;
    return kInner;
}

// Particle selections (include/mph_gpu.h MphSelection).  One body for the host's
// mph_selection_accepts and the device's k_sel_flag, so the two cannot drift apart.
// sel_valid: the argument rules; sel_accepts: the predicate of a valid selection, x the coordinates
// its box tests (Position for box 1, InitialPosition for box 2; not read for box 0).
MPH_HD inline bool sel_valid(const MphSelection& s, int dim)
{
    if (dim != 2 && dim != 3) return false;
    if (s.every < 1 || s.phase < 0 || s.phase >= s.every) return false;
    if (s.box < 0 || s.box > 2 || (s.type_mask & ~0x3f)) return false;
    if (s.box)
        for (int d = 0; d < 3; ++d)
            if (d < dim && !(s.lo[d] <= s.hi[d])) return false;
    return true;
}
MPH_HD inline bool sel_accepts(const MphSelection& s, int dim, int index, int type, const double* x)
{
    if (s.type_mask && (type < 0 || type >= kTypes || !((s.type_mask >> type) & 1))) return false;
    if (index % s.every != s.phase) return false;
    // (three rounds whatever dim is: the device unrolls them and x stays in registers)
    bool in = true;
    if (s.box)
        for (int d = 0; d < 3; ++d) in = in && (d >= dim || (x[d] >= s.lo[d] && x[d] < s.hi[d]));
    return in;
}

// Kinematics (include/mph_gpu.h MphKinematics; kernel: mph_kinematics.hip k_kinematics, host:
// mph_kinematics_arrays).  One body each for the argument rules, a pair's contribution and the
// finishing step, so the device and the host's double loop cannot drift apart: only the order in
// which a particle's pairs arrive differs.  All of it without contraction.
// The resolved arguments, passed to the kernel by value.
struct KinDev {
    double h, n0, beta, det_floor;
    int mask;   // classes summed: bit 0 fluid, 1 structure, 2 walls
};
// the argument rules but the radius's upper bound (MaxRadius: the caller's)
MPH_HD inline bool kin_valid(const MphKinematics& k)
{
    return k.radius >= 0.0 && k.surface_beta >= 0.0 && k.det_floor >= 0.0 && k.det_floor < 1.0 && k.classes >= 0 &&
           k.classes <= 7 && k.reserved == 0;
}
// the defaults resolved (rv: RadiusRatioV * dx; n0: mph_kinematics_n0 of the resolved radius)
MPH_HD inline KinDev kin_resolve(const MphKinematics& k, double rv, double n0)
{
    KinDev K;
    K.h = k.radius > 0.0 ? k.radius : rv;
    K.n0 = n0;
    K.beta = k.surface_beta > 0.0 ? k.surface_beta : 0.97;
    K.det_floor = k.det_floor > 0.0 ? k.det_floor : 1e-6;
    K.mask = k.classes ? k.classes : 7;
    return K;
}
MPH_HD inline bool kin_class(int mask, int type) { return (unsigned)type < (unsigned)kTypes && ((mask >> (type >> 1)) & 1); }
// the periodic minimum image of every pair loop, Mod(d + w/2, w) - w/2 (mph_device.h image_exact's
// general branch; its short cut for 0 <= s < 0.75 w gives the same bits: floor(s / w) is 0 there)
MPH_HD inline double image_hd(double d, double w, double hw)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double s = d + hw;
    return (s - w * floor(s / w)) - hw;
}
MPH_HD inline double r2_hd(double q0, double q1, double q2)   // (mph_device.h r2_exact)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return q0 * q0 + q1 * q1 + q2 * q2;
}
// a particle's sums: COUNT, WSUM, c, G and the upper triangle of M {00, 01, 02, 11, 12, 22}
template <int DIM> struct KinAcc {
    double cnt = 0.0, sw = 0.0;
    double c[DIM] = {}, G[DIM][DIM] = {}, M[DIM * (DIM + 1) / 2] = {};
};
// neighbour j of an accepted class: q its minimum image (q[2] = 0 in 2-D), r2 = r2_exact(q), dv = v_j - v_i
template <int DIM> MPH_HD inline void kin_pair(KinAcc<DIM>& a, double h, const double (&q)[3], double r2, const double (&dv)[3])
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double r = sqrt(r2);
    if (!(r < h)) return;
    const double u = 1.0 - r / h;
    const double w = u * u;
    a.cnt += 1.0;
    a.sw += w;
    int m = 0;
    for (int d = 0; d < DIM; ++d) {
        const double wq = w * q[d];
        a.c[d] += wq;
        for (int e = d; e < DIM; ++e) a.M[m++] += wq * q[e];
        const double wv = w * dv[d];
        for (int e = 0; e < DIM; ++e) a.G[d][e] += wv * q[e];
    }
}
// the record of a particle's sums: o[MPH_KIN_CHANNELS]
template <int DIM> MPH_HD inline void kin_finish(const KinAcc<DIM>& a, const KinDev& K, double* o)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    for (int k = 0; k < MPH_KIN_CHANNELS; ++k) o[k] = 0.0;
    const bool any = a.sw > 0.0;
    const double fill = a.sw / K.n0;
    o[MPH_KIN_COUNT] = a.cnt;
    o[MPH_KIN_WSUM] = a.sw;
    o[MPH_KIN_FILL] = fill;
    for (int d = 0; d < DIM; ++d) o[MPH_KIN_CX + d] = any ? a.c[d] / a.sw : 0.0;
    double A[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, det, floor_;
    if constexpr (DIM == 3) {
        const double m00 = a.M[0], m01 = a.M[1], m02 = a.M[2], m11 = a.M[3], m12 = a.M[4], m22 = a.M[5];
        A[0][0] = m11 * m22 - m12 * m12;
        A[0][1] = m02 * m12 - m01 * m22;
        A[0][2] = m01 * m12 - m02 * m11;
        A[1][1] = m00 * m22 - m02 * m02;
        A[1][2] = m01 * m02 - m00 * m12;
        A[2][2] = m00 * m11 - m01 * m01;
        A[1][0] = A[0][1];
        A[2][0] = A[0][2];
        A[2][1] = A[1][2];
        det = m00 * A[0][0] + m01 * A[0][1] + m02 * A[0][2];
        const double t = (m00 + m11 + m22) / 3.0;
        floor_ = K.det_floor * (t * t * t);
    } else {
        const double m00 = a.M[0], m01 = a.M[1], m11 = a.M[2];
        A[0][0] = m11;
        A[0][1] = -m01;
        A[1][0] = -m01;
        A[1][1] = m00;
        det = m00 * m11 - m01 * m01;
        const double t = (m00 + m11) / 2.0;
        floor_ = K.det_floor * (t * t);
    }
    const bool degenerate = a.cnt < (double)(DIM + 1) || !(det > floor_);
    double L[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    if (!degenerate) {
        for (int d = 0; d < DIM; ++d)
            for (int e = 0; e < DIM; ++e) {
                double s = a.G[d][0] * A[0][e] + a.G[d][1] * A[1][e];
                if constexpr (DIM == 3) s += a.G[d][2] * A[2][e];
                L[d][e] = s / det;
            }
        for (int d = 0; d < 3; ++d)
            for (int e = 0; e < 3; ++e) o[MPH_KIN_L + 3 * d + e] = L[d][e];
        o[MPH_KIN_DIV] = DIM == 3 ? L[0][0] + L[1][1] + L[2][2] : L[0][0] + L[1][1];
        o[MPH_KIN_WX] = L[2][1] - L[1][2];
        o[MPH_KIN_WY] = L[0][2] - L[2][0];
        o[MPH_KIN_WZ] = L[1][0] - L[0][1];
        double s2 = 0.0;
        for (int d = 0; d < 3; ++d)
            for (int e = 0; e < 3; ++e) {
                const double D = 0.5 * (L[d][e] + L[e][d]);
                s2 += D * D;
            }
        o[MPH_KIN_SHEAR] = sqrt(2.0 * s2);
    }
    o[MPH_KIN_FLAGS] = (double)((degenerate ? MPH_KIN_FLAG_DEGENERATE : 0) | (fill < K.beta ? MPH_KIN_FLAG_SURFACE : 0) |
                                (a.cnt == 0.0 ? MPH_KIN_FLAG_ALONE : 0));
}

// Device-resident sizes of one slab redistribution (mph_dist.hip), written by the kernels of the
// step itself, so that a whole step -- RCCL calls included -- can be captured into a hipGraph.
// send/recv double as the count messages of the exchange (2 ints to each neighbour).
struct DistLayout {
    int n;                        // local particles (owned + ghosts) after the last redistribution
    int n_own;
    int seg[kSlabClasses + 1];    // class segment starts in C (k_dist_scatter)
    int send[4];                  // to the left {bandL, migL}, to the right {migR, bandR}
    int recv[4];                  // from the left their {migR, bandR}, from the right their {bandL, migL}
    int hw[5];                    // high-water marks since the last reset: send_l, send_r, recv_l,
                                  // recv_r, n (capacity tuning between step batches)
    int pad;
};

// Per-type tables read with per-lane type indices (device memory; staged through LDS where hot).
struct DevTables {
    double ratio[kTypes * kTypes];   // InteractionRatio[ti][tj]
    double mu_ij[kTypes * kTypes];   // 2 mu_i mu_j / (mu_i + mu_j)
    double cofa[kTypes], mass[kTypes], inv_mass[kTypes], bulk[kTypes], bulk_visc[kTypes];
};

// Host-side derived constants (reference arithmetic, bit-identical to the reference's globals).
struct HostDerived {
    double ra, rg, rp, rv, max_radius;
    double swa, swg, swp, swv, n0a, n0p, r2g, cofk, cofa[kTypes];
    double vol, dx;
    double dmin[3], dmax[3], dw[3];
    double cell_w;
    int cell_n[3];
    double wall_rot[kTypes][3][3];
};

}  // namespace mph
