// mph_kernels.h -- launch interface of the hand-written HIP/CDNA4 (gfx950) kernels of the MPH explicit
// hot path, the one host-visible interface of the kernel units (mph_sort.hip, mph_search.hip,
// mph_passes.hip, mph_elastic.hip, mph_slab.hip, mph_monitor.hip, mph_sample.hip, mph_gauge.hip,
// mph_select.hip, mph_kinematics.hip), used by the context's
// host units (mph_ctx.h) and the slab layer's (mph_dist.h).  It also decides a step's form
// (seq_step): plain host C++, so a host compiler can include this header and test it.
#pragma once

#include <hip/hip_runtime.h>

#include "mph_params.h"

namespace mph {

// Device arrays of the elastic solid, in structure-slot order (see StructureInit).  The fixed
// Lagrangian lists are stored ELL-tiled like the fluid list: entry k of slot s at
// [(s >> 6) * W + k][s & 63], so the 64 lanes of a wavefront read entry k with one coalesced load.
struct StructDev {
    int* orig = nullptr;          // slot -> original particle index
    int* slot_of = nullptr;       // original particle index -> slot (-1: not structure / not owned)
    int* bidx = nullptr;          // slot -> index of its B entry this step (written by pass B)
    int n_own = 0;                // slots computed here (slab mode: owned, then ghost slots)
    // slab mode: the owned slots [0, n_inner) have no ghost slot in their out- or in-list (their
    // substep halves run while the ghost exchange travels); [n_inner, n_own) have one
    int n_inner = 0;
    int wo = 0, wi = 0;           // ELL widths (max out / in count)
    int* ocnt = nullptr;          // InitialStructureNeighborCount per slot
    int* icnt = nullptr;          // in-degree (how many slots list s)
    int* eo_nb = nullptr;         // out-list neighbour slots, ELL [ntile * wo][64]
    int* ei_nb = nullptr;         // in-list (senders i of the reference's scatter), ELL [ntile * wi][64]
    double4* wx0 = nullptr;       // sum_j w_sj x0_sj (the P_s half of StressForce, fixed)
    double* L = nullptr;          // Normalizer [ns][9]
    double2* lame = nullptr;      // (LambdaLames, MuLames)
    double* inv_rho = nullptr;    // 1/Density[type]
    int* clamp = nullptr;         // 0 free, 1 clamped + force zeroed, 2 clamped
    double4* x0 = nullptr;        // InitialPosition
    double4* x = nullptr;         // current position (valid during the substeps)
    double4* v = nullptr;
    double4* u = nullptr;         // displacement Mod(x - x0) (main.cpp:2700-2712), per substep
    double4* P = nullptr;         // first Piola-Kirchhoff F S L: 2-D one double4 {P00,P01,P10,P11}, 3-D 3 rows
    // DeformGradient, Strain, Stress: nine planes each, element 3a + b of slot s at [(3a + b) fes + s]
    double* F = nullptr;
    double* E = nullptr;
    double* S = nullptr;
    int fes = 0;                  // their plane stride (slots allocated)
};

// Per-kernel HIP event timing (mph_profile_steps); nullptr in normal runs.  `events` hands out a
// start/stop pair for one launch and says how to set them: true, from the dispatch packet's own
// timestamps (hipExtLaunchKernelGGL); false, recorded on the stream around the launch.
struct Profiler {
    virtual bool events(const char* name, hipStream_t s, hipEvent_t* start, hipEvent_t* stop) = 0;
    // `waiting` is about to wait for an event `from` has just recorded: the next launch on
    // `waiting` starts no earlier than `from` reaches this point (mph_profile_steps)
    virtual void join(hipStream_t waiting, hipStream_t from) { (void)waiting; (void)from; }
    virtual ~Profiler() = default;
};

// Persistent particle state, one FP64 array per component (structure of arrays): in the
// neighbour loops consecutive lanes gather consecutive elements, so one 8-byte load per lane
// touches ~8-10 cache lines per wavefront instead of ~40 for 32-byte records.
struct Soa {
    double *x = nullptr, *y = nullptr, *z = nullptr;
    double *vx = nullptr, *vy = nullptr, *vz = nullptr;
    int *type = nullptr, *id = nullptr;
    // gather record of the sorted set A (null for B/C): {x, y, z, vx, vy, vz}, 48 bytes, read
    // with three 16-byte loads.  The neighbour loops are bound by the texture-address/data path
    // (profiles/r01: TA ~64 % busy in pass A); the type of j travels in the list entry instead
    // (kTypeShift), so a neighbour costs 48 gathered bytes instead of 64.
    double2* p6 = nullptr;
    // {x, y, z} - domain centre in FP32 and the type's bits, 16 bytes, the search's staged
    // candidate records (sorted set A only)
    float4* f4 = nullptr;
};

// Slab mode: the kept part [0, *n) of the redistributed set C is not copied -- entry v lives in
// the integrated set V at idx[v] (-1 - q: a migrant leaving as a ghost, its id negated on read);
// only the received tail [*n, ...) is in C itself.  idx null: C holds everything (single context).
struct VSrc {
    const int* idx = nullptr;
    const int* n = nullptr;
    Soa V;
};

// Pass B hands the integrated structure particles straight to the slot-ordered elastic arrays
// (null slot_of: no structure particles) and records where each slot's B entry lives (bidx), so
// the last substep can write the result back.
struct StructHook {
    const int* slot_of;
    double4 *sx, *sv, *su;
    const double4* sx0;
    int* bidx;
};

// Per-step monitors (mph_monitor.hip): the configuration and device buffers of
// mph_monitor_configure, passed to the monitor kernels by value.
constexpr int kMonFirst = 2;      // head slots [kMonFirst, kMonFirst + kMonPartial) are reduced over particles
constexpr int kMonPartial = 28;   // entries of a block's partial record
// How entry k of a partial record (head slot kMonFirst + k) combines: 0 sum, 1 min, 2 max -- over the
// blocks of a launch (mph_monitor.hip) and over the ranks' records (mph_monitor_combine).
__host__ __device__ constexpr int mon_op(int k)
{
    return k < 18 ? (k % 6 == 5 ? 2 : 0) : (k < 24 ? (k % 2 == 0 ? 1 : 2) : (k == 24 ? 1 : (k < 27 ? 2 : 0)));
}
// a slab rank's record (mph_dist_monitor_configure): its tracked row {present, x, y, z, vx, vy, vz}
// (trk holds rows of either length), and where its flag of probe q lies: probes[kMonProbeOwn + q],
// behind the coordinates, nonzero where this rank's slab holds the probe
constexpr int kDistMonRow = 7;
constexpr int kMonProbeOwn = 3 * MPH_MONITOR_MAX_PROBES;
struct MonitorDev {
    int stride = 1, capacity = 1, ntrack = 0, nprobe = 0;
    int width = 0;                     // doubles per sample
    double probe_h = 0.0;
    long long* counters = nullptr;     // {steps since the configuration, samples written}
    double* ring = nullptr;            // [capacity][width]
    double* partial = nullptr;         // [monitor_blocks(n)][kMonPartial]
    double* trk = nullptr;             // rows {x, y, z, vx, vy, vz} of the distinct tracked ids
    double* prb = nullptr;             // {value, count} per probe
    const int* track_sorted = nullptr; // the distinct tracked ids ascending, padded with INT_MAX to 64
    const int* track_map = nullptr;    // tracked entry k -> its row of trk
    const double* probes = nullptr;    // [nprobe][3] (and a slab rank's flags, kMonProbeOwn)
    // free-surface gauges (mph_gauge.hip, mph_gauge_configure), behind every older member: a
    // default-constructed MonitorDev is a configuration without gauges
    int ngauge = 0, gauge_axis = 0;
    int gauge_nbins = 1;               // bins of particle_spacing along gauge_axis (<= MPH_GAUGE_MAX_BINS)
    double gauge_h = 0.0;              // radius
    const double* gauges = nullptr;    // [ngauge][3]
    double* gau = nullptr;             // {COUNT, TOP, BOTTOM, WET} per gauge
};

// A step's form: which variant of its kernels a step launches.  Decided by
// seq_step below and nowhere else; all false in the context's own Launch, in the slab steps and
// in every launch outside a step.
struct StepForm {
    // a lazy wall step (mph_params.h kCoarseShift): k_prep marks the coarse map, the search skips the
    // idle wall waves, pass A clears the map again; the passes run on the lazy step's XCD map
    bool lazy = false;
    // lean steps: a lazy step whose search accepts only the pairs it stores
    // and counts no NeighborCount / whose pass A leaves out the DensityA and GravityCenter sums
    bool lean_search = false, lean_pass_a = false;
    // the key fold (seq_step below): keys_done, the previous step's pass B has moved and wrapped the
    // particles and left this step's cell keys, slots and histogram, so the sort launches no k_prep;
    // keys_next, this step's pass B does that for the next step
    bool keys_done = false, keys_next = false;
};

// Everything one launch sequence needs.
struct Launch {
    const DevParams* P = nullptr;
    const DevTables* T = nullptr;
    DevState* st = nullptr;
    hipStream_t stream = nullptr;
    Profiler* prof = nullptr;
    // B set: integrated state in the previous order; A set: cell-sorted current order
    Soa A, B;
    int* dst_of = nullptr;        // slab mode: pre-sort index -> sorted index
    int *key = nullptr, *slot = nullptr, *tmp = nullptr, *cnt = nullptr, *start = nullptr, *bsum = nullptr;
    // ncount: each list's rows (what the passes walk); nbcount: NeighborCount (every neighbour within
    // the search radius; the lists keep only r^2 <= DevParams.rlf)
    int *nbr = nullptr, *ncount = nullptr, *nbcount = nullptr;
    // the row jumps of the lists (mph_list.h RowMask): one header word per wave, one word of gap
    // starts per particle; ncount counts rows, gaps included
    unsigned long long *lhdr = nullptr, *lgap = nullptr;
    // the group bases of the waves with 16-bit rows (mph_params.h kOff16Bits): kBaseInts per wave
    int* lbase = nullptr;
    int* wface = nullptr;         // slab mode: face-wavefront flags written by pass B (early send)
    VSrc vsrc;                    // slab mode: where the sort finds the kept entries of its input
    // fewest particles for the work-balanced XCD map of the passes (split in k_rank_scatter);
    // MPH_XCD_BAL_MIN overrides it at creation (tests force the map on small cases)
    int xcd_bal_min = 1 << 20;
    // lazy wall steps: the coarse map of the non-wall particles (null: the context never takes a
    // lazy step) and its size
    unsigned char* cmap = nullptr;
    int cmap_bytes = 0;
    // lean steps, the context's capabilities (set at creation, ctx_fill_launch): lean_ok, it takes
    // them (MPH_LEAN_STEPS); lean_search, and its radii let the search (lean_search_ok)
    bool lean_ok = false, lean_search = false;
    // the key fold, the context's choice (MPH_KEY_FOLD, ctx_fill_launch); seq_step has the rest
    bool key_fold = false;
    // keys_next: the coarse map the next step's search reads -- set where that step is lazy, else null
    unsigned char* cmap_next = nullptr;
    StepForm form;   // this step's (seq_step)
    // pass A products (A order): pressure values, gravity centre (GC, PressureA), sums
    double *pres = nullptr, *gx = nullptr, *gy = nullptr, *gz = nullptr, *pa = nullptr;
    double *dens_a = nullptr, *vstrain = nullptr, *divp = nullptr;
    double4 *fpart = nullptr;   // pass A: P_i half of the pressure force + viscous force
    double4 *rec = nullptr;     // pass A: {x, y, z, PressureP}, the pass-B gather record
    double4 *force = nullptr, *acc = nullptr;   // outputs (A order)
    const StructDev* S = nullptr;
    const MonitorDev* mon = nullptr;   // monitors on: sampled at the end of every step
};

// The Launch of a step that is not the last of its batch.  Force and Acceleration (main.cpp:2085-2096,
// 2892-2956) are outputs only: no kernel reads them, and every step overwrites all of them, so only
// a batch's last step stores them (pass B -6 % at D1M); mph_get after any mph_step sees the last
// step's values as before.  The same holds in pass A for DensityA, VolStrainP, DivergenceP and,
// without surface tension (pass B then reads neither), GravityCenter and PressureA.
inline Launch trim_outputs(Launch L)
{
    L.dens_a = L.vstrain = L.divp = nullptr;
    if (!L.P->surface) L.gx = L.gy = L.gz = L.pa = nullptr;
    L.force = L.acc = nullptr;
    return L;
}
// whether a step's Launch is an untrimmed one (Force is allocated at every creation)
inline bool stores_outputs(const Launch& S) { return S.force != nullptr; }

// Steps enqueued together with nothing between them (a captured graph, a phase-timed or profiled
// batch): their number and whether the last one stores the output-only fields.
struct StepSeq {
    int steps = 1;
    bool store_last = true;
};
// The four kinds a context replays, in replay_plan's launch order; the profiler's batch of n steps is
// StepSeq{n, true}.
enum SeqKind { kSeq8t = 0, kSeq8, kSeq1t, kSeq1, kSeqKinds };
constexpr StepSeq kSeqs[kSeqKinds] = {{8, false}, {8, true}, {1, false}, {1, true}};

// The key fold.  A step opens with k_prep: wall motion, periodic wrap, cell
// key, histogram -- all of it from what the previous step's pass B had in registers when it stored
// them.  Where nothing can come between the two, pass B does k_prep's work before its stores
// (k_pass_b<.., KEYS>) and the next step's sort starts at the scan.  Nothing comes between them
// inside one sequence.  Never across the sequence's end (the state a caller reads is the unmoved
// one), never with structure particles (the elastic substeps write the set after pass B), monitors
// (they read the unmoved set) or a slab context (vsrc).
inline bool key_fold_ok(const Launch& L)
{
    return L.key_fold && L.P->n_struct == 0 && !L.mon && !L.vsrc.idx;
}

// The Launch of step k of a sequence of a single context, from the context's: the outputs trimmed
// unless the step is the storing last one, and the step's form -- decided here and nowhere else.
// Lazy wall steps take the output rule one kernel further up.  On a step that does not store, a wall
// walks no list in pass B, so what the search and pass A compute for a wall particle whose
// neighbours are all walls -- its list, PressureP, the pass-B record, fpart -- has no reader; the
// next storing step computes all of it again.  Off (every step full) without the map (slab mode,
// MPH_LAZY_WALLS=0) and while the monitor kernels run, which read the walls' pressure on every step.
// A lean step is a lazy step that also leaves out what it would compute only to drop it: the search
// where the context's radii allow (Launch.lean_search), pass A where GravityCenter is not stored
// (DensityA never is on a lazy step).
// The key fold: a step's keys come from the step before it in the sequence and it leaves the keys of
// the step after it, with the coarse map where that step is lazy (cmap_next).
inline Launch seq_step(const Launch& L, StepSeq seq, int k)
{
    const auto stores = [&](int j) { return seq.store_last && j == seq.steps - 1; };
    const auto lazy = [&](int j) { return !stores(j) && L.cmap && !L.mon; };
    Launch S = stores(k) ? L : trim_outputs(L);
    S.form.lazy = lazy(k);
    S.form.lean_search = S.form.lazy && L.lean_ok && L.lean_search;
    S.form.lean_pass_a = S.form.lazy && L.lean_ok && !L.P->surface;
    S.form.keys_done = key_fold_ok(L) && k > 0;
    S.form.keys_next = key_fold_ok(L) && k + 1 < seq.steps;
    S.cmap_next = S.form.keys_next && lazy(k + 1) ? L.cmap : nullptr;
    return S;
}

// What the launchers read off a step's Launch instead of deriving it again: the coarse map a lazy
// step's kernels take (null on every other launch), and whether a launch over the lazy step's
// balanced XCD map (list_grid's lazy grid, the sort's split 2, the search's xcd_sfrac).
inline unsigned char* lazy_cmap(const Launch& L) { return L.form.lazy ? L.cmap : nullptr; }
inline bool xcd_bal(const Launch& L) { return L.P->n >= L.xcd_bal_min; }
inline bool lazy_bal(const Launch& L) { return L.form.lazy && xcd_bal(L); }

// How n steps of one call are cut into sequences: the count of each kind,
// launched in the kinds' order -- whole batches of eight steps none of which stores the output-only
// fields, batches of eight whose last step stores them, single steps that store none, single steps
// that do.  A call can only be observed after it returns, so only its last step needs them: with
// `lean8` (the context has the all-lean 8-step graph) every whole batch but the last is a kSeq8t, and
// with `lean1` every step of the remainder but the last is a kSeq1t.  Without either, every batch and
// every single step ends in a storing step of its own (a slab context's sequence).  Plain host C++,
// no HIP call.
struct ReplayPlan {
    int count[kSeqKinds] = {0, 0, 0, 0};
};
inline ReplayPlan replay_plan(int n, bool lean8, bool lean1)
{
    ReplayPlan p;
    if (n <= 0) return p;
    const int whole = n / 8, rest = n % 8;
    p.count[kSeq8t] = lean8 && whole >= 2 ? whole - 1 : 0;
    p.count[kSeq8] = whole - p.count[kSeq8t];
    p.count[kSeq1t] = lean1 && rest > 1 ? rest - 1 : 0;
    p.count[kSeq1] = rest - p.count[kSeq1t];
    return p;
}

// Lattice sampling (mph_sample.hip, mph_sample_grid): the lattice, the wave tiling chosen for it
// (sample_tiling) and the resolved radius and class mask, passed to the kernel by value.
struct SampleDev {
    double origin[3], spacing[3];
    int count[3];
    int tile[3];     // lattice points of one wave's tile per axis (powers of two, product <= 64)
    int tiles[3];    // tiles per axis
    int mask;        // classes summed: bit 0 fluid, 1 structure, 2 walls
    double h;        // radius
};
// A slab rank's run of lattice planes (mph_dist_sample_grid_partial): count[slab axis] is the run's
// number of planes (tile / tiles chosen for the run), `first` the index of its first plane in the
// whole lattice, which a point's coordinates are computed from.  Behind SampleDev, so the
// single-context kernel keeps its argument layout.
struct SampleRunDev : SampleDev {
    int first;
};

// The elevation map (mph_gauge.hip, mph_gauge_grid): the lattice of lines with the resolved axis, bin
// count and radius, passed to the kernel by value.
struct GaugeGridDev {
    double origin[3], spacing[3];
    int count[3];
    int nlines;      // count[0] count[1] count[2] (<= MPH_GAUGE_GRID_MAX_LINES)
    int axis, nbins;
    int waves;       // lines (waves) per block: 1 or 4
    double h;        // radius
};
// A slab rank's lines (mph_dist_gauge_grid_partial).  Lines not parallel to the slab axis: a run of
// the planes the rank owns, as SampleRunDev (count[slab axis] the run's, nlines its lines, `first`
// its first plane).  Lines parallel to it: the whole lattice, first = 0.
struct GaugeRunDev : GaugeGridDev {
    int first;
};
// doubles of a slab rank's line record {COUNT, TOP, BOTTOM, WET, LOBIN, HIBIN} (MPH_DIST_GAUGE_RECORD)
constexpr int kDistGaugeRec = MPH_DIST_GAUGE_RECORD;

// Particle selections (mph_select.hip, mph_select): the device buffers of a context's selection,
// passed to the kernels by value.  Index spaces: i an original particle index (< n), q an index
// into the sorted arrays (< n), r a rank among the selected (< count).
constexpr int kSelTotals = MPH_TOTALS;   // doubles of a totals record (MphTotalSlot)
struct SelectDev {
    int* flag = nullptr;           // [n] by i: 1 selected, 0 not
    int* slot_a_of = nullptr;      // [n] i -> q in the sorted set A (pass-A products, Force, virial)
    int* slot_b_of = nullptr;      // [n] i -> q in the integrated set B (Position, Velocity)
    unsigned* mask = nullptr;      // [(n + 31) / 32] a box on InitialPosition: the host's verdict, bit i
    int* bsum = nullptr;           // [select_blocks(n) + 1] selected per block of i, then their offsets; last: count
    int *ids = nullptr, *slot_a = nullptr, *slot_b = nullptr;   // [count] by r: i ascending, and its two q
    int count = 0;
};
int select_blocks(int n);          // blocks of original indices of the scan (k_sel_count / k_sel_fill)
int select_total_blocks(int count);// partial records of the totals
// flag (with_mask: from D.mask, else the predicate on the device), count and scan: leaves D.flag, the
// two maps, the block offsets and the count in D.bsum[select_blocks(n)]; L.P->n > 0
void launch_select_scan(const Launch& L, const Soa& X, const MphSelection& s, bool with_mask, const SelectDev& D);
// D.ids / slot_a / slot_b of the D.count selected; D.count > 0
void launch_select_fill(const Launch& L, const SelectDev& D);
// The same on a slab rank (mph_dist_select): X holds n slots, ghosts (id < 0) among them; D.flag and the
// two maps are indexed by the whole problem's original index, [n_glob] -- flag rounded up to a multiple
// of 4 ints, cleared here first (only the owned indices are visited) -- and D.bsum has
// select_blocks(n_glob) + 1 entries; n_glob > 0, n >= 0
void launch_dist_select_scan(const Launch& L, int n, int n_glob, const Soa& X, const MphSelection& s, bool with_mask,
                             const SelectDev& D);
void launch_dist_select_fill(const Launch& L, int n_glob, const SelectDev& D);
// out[r][e] = src[e][slot[r] * stride] for r < count, e < nc (1, 3 or 9; ints: 1)
void launch_select_gather(const Launch& L, const double* const* src, int nc, int stride, const int* slot, int count,
                          double* out);
void launch_select_gather_int(const Launch& L, const int* src, const int* slot, int count, int* out);
// the totals about `center` into out[kSelTotals] (device); partial: select_total_blocks(D.count) records
void launch_select_totals(const Launch& L, const Soa& X, const SelectDev& D, const double* center, double* partial,
                          double* out);

// One time step of the reference (main.cpp:597-686) is mapped onto these launches:
//
//   k_prep           calculateWall (3031-3071) + calculatePeriodicBoundary (3322-3333) + cell key
//                    + cell histogram (first half of the counting sort that replaces the
//                    reference's bitonic sort, 1683-1708)
//   k_scan_*         exclusive scan of the cell histogram -> cell start offsets (1711-1728)
//   k_place          scatter particle ids into their cells (unordered) + Time/WallCenter advance
//   k_rank_scatter   deterministic in-cell rank (by previous sorted index) and particle reorder
//   k_neighbors      linked-cell search (1743-1810): 7x7(x5) stencil (2 kReach + 1 columns of cells
//                    >= rc/3, 2 kContigReach + 1 cells >= rc/2 along the contiguous axis), the
//                    reference's exact FP64 acceptance test, ELL neighbour list per wavefront
//   k_pass_a         the pass-A sums over the list: DensityA (2141), GravityCenter (2174), DensityP
//                    (2314), DivergenceP (2343), PhysicalCoefficients (2099), pressure values
//                    PressureP (2384) / PressureA (2218)
//   k_pass_b         PressureP force (2394), PressureA force (2225), DiffuseInterface (2261),
//                    ViscosityV (2478), InterfaceForce (2427), Gravity (2917), Acceleration (2938),
//                    Convection (1892)
//   k_struct_*       elastic substeps: DeformationVector (2673) + Stress (2756) -> PK1 stress;
//                    StressForce (2812) in gather form + updateElasticPosition (1910); pass B
//                    hands the structure particles to them and the last substep writes back
//
// One unit per phase: mph_sort.hip (k_prep ... k_rank_scatter), mph_search.hip (k_neighbors),
// mph_passes.hip (k_pass_a, k_pass_b, k_virial), mph_elastic.hip (k_struct_*, and k_sinit_* at
// creation), mph_slab.hip (the slab decomposition's k_dist_*, k_halo_*, k_struct_pack / _unpack).  What
// two or more units share is in mph_device.h and, for the neighbour lists' layout, mph_list.h.
//
// All arithmetic is FP64.  Neighbour membership and every per-kernel radius test reproduce the
// reference's FP64 expressions bit for bit (no contraction, IEEE division), so NeighborCount is
// exact; the weighted sums are reassociated (own order, FMA) and agree within the tolerances
// written in tests/.
//
// Memory layout: particle state is structure-of-arrays FP64 in cell-sorted order (Soa).  The
// neighbour loops are bound by the per-CU texture-address path (profiles/r01: TA ~75% busy with
// 32-byte records); SoA makes consecutive lanes gather consecutive doubles.

int monitor_blocks(int n);   // blocks (partial records) of k_monitor_partial
void launch_monitor(const Launch& L, const MonitorDev& M);
// a slab rank's record of the step that has just run on L (mph_dist.hip)
void launch_dist_monitor(const Launch& L, const MonitorDev& M);
// the gauges' records of a sampled step into M.gau (launch_monitor calls it; M.ngauge > 0, L.P->n > 0)
void launch_monitor_gauge(const Launch& L, const MonitorDev& M);
// the four channels of every line into out ([nz][ny][nx][4], device); L.P->n > 0
void launch_gauge_grid(const Launch& L, const GaugeGridDev& G, double* out);
// a slab rank's records of the G.nlines lines of G into out ([G.nlines][kDistGaugeRec], device)
void launch_dist_gauge_grid(const Launch& L, const GaugeRunDev& G, double* out);
// fills G.tile / G.tiles from G.count / G.spacing (run_axis: the contiguous cell axis); returns the
// number of tiles (waves)
long long sample_tiling(SampleDev& G, int run_axis);
// the six channels of every lattice point into out ([nz][ny][nx][6], device); L.P->n > 0
void launch_sample_grid(const Launch& L, const SampleDev& G, double* out);
// a slab rank's run of planes into out ([run's points][6], device); recorded as "dist_sample_grid"
void launch_dist_sample_grid(const Launch& L, const SampleRunDev& G, double* out);
void launch_sort(const Launch& L, int mode);   // mode 0 init, 1 step, 2 step (motion done)
void launch_neighbors(const Launch& L);
void launch_pass_a(const Launch& L);
// launch_neighbors + launch_pass_a
void launch_search_pass_a(const Launch& L);
void launch_pass_b(const Launch& L, int phase = 0);   // phase: 0 all, 1/2 slab inner/near-face
void launch_structure(const Launch& L, bool last);   // last: the batch's last step (output tensors)
// calculateInitialNeighbor + calculateNormalizer of the ns structure slots (x0 in slot order) on
// the device: counts (ocnt), ELL out-rows (*eo, width *wo) and their transpose (*ei, *wi), both
// sorted ascending, Normalizer (Lm [ns][9]) and sum_j w_sj x0_sj (wx0).  The ELL arrays are
// allocated through alloc(actx, bytes) once their widths are known.  key/slot/tmp/sorted: ns
// ints of scratch each.  Returns 0, -1 (HIP error), -2 (a slot reached 512 neighbours), -3 (OOM).
int launch_struct_init(const Launch& L, int ns, const double4* x0, int* key, int* slot, int* tmp, int* sorted,
                       int* ocnt, int* icnt, int** eo, int* wo, int** ei, int* wi, double* Lm, double4* wx0,
                       void* (*alloc)(void*, size_t), void* actx);
// over the slots [s0, s1) (s1 < 0: every computed slot, [0, n_own))
// store: also write the output-only tensors F, E, S (the last substep of a batch's last step)
void launch_struct_stress(const Launch& L, bool store, int s0 = 0, int s1 = -1);
void launch_struct_velocity(const Launch& L, bool last, int s0 = 0, int s1 = -1);
// slab mode: rows of per-slot double4 records (w per slot) gathered into / scattered from a message
void launch_struct_pack(const Launch& L, const double4* src, int w, const int* idx, int m, double4* buf);
void launch_struct_unpack(const Launch& L, const double4* buf, int w, const int* idx, int m, double4* dst);
void launch_virial(const Launch& L, const Soa& X, double* vir, double* vpres);   // X: state in A order
// kinematics (mph_kinematics.hip): the MPH_KIN_CHANNELS doubles of every particle into out (A order)
// over the lists as they stand, of the state in A order -- stepped: the integrated set B, else (before
// the first step) the sorted set A's records; and out[r] = kin[slot[r]] for r < count
void launch_kinematics(const Launch& L, bool stepped, const KinDev& K, double* out);
void launch_kin_gather(const Launch& L, const double* kin, const int* slot, int count, double* out);

// slab decomposition (mph_dist.hip; the left / right arguments are the two DistSide records' values)
struct HaloFields {
    double* f[5];
    int nf;
    double4* rec;   // f[0] (PressureP) is also the P of the pass-B record (its plane stride rec_stride)
    int rec_stride;
};
// exclusive scan of cnt[ncell] into start (start[ncell] = total, or *n_dev when non-null); re-zeroes cnt
void launch_scan(int* cnt, int ncell, int* bsum, int* start, int total, const int* n_dev, hipStream_t stream,
                 Profiler* prof);
int dist_blocks(int n);
// slab redistribution; every size is read from the device layout (graph-capturable).  cap = local
// array capacity, cap_msg = capacity (particles) of the message of that side.
void launch_dist_classify(const Launch& L, const SlabGeom& g, int cap, const DistLayout* lay, int move, int* cls,
                          int* bcnt, const int* wface = nullptr);
void launch_dist_early_classify(const Launch& L, const SlabGeom& g, int cap, const DistLayout* lay,
                                const int* wface, int* cls, int* bcnt);
void launch_dist_early_pack(const Launch& L, int cap, DistLayout* lay, const int* cls, const int* boff, int cap_l,
                            int cap_r, char* buf_l, char* buf_r);
// vidx non-null: record the B index of every kept entry (VSrc) instead of copying it into C
void launch_dist_scatter(const Launch& L, int cap, DistLayout* lay, const int* cls, const int* boff,
                         const Soa& C, int* dseg, int* vidx = nullptr);
// both sides / directions in one launch each (blockIdx.y)
void launch_dist_pack(const Launch& L, const Soa& C, DistLayout* lay, int cap_l, int cap_r, char* buf_l,
                      char* buf_r, const VSrc& vs = VSrc{});
void launch_dist_unpack(const Launch& L, const char* buf_l, const char* buf_r, DistLayout* lay, int cap_l,
                        int cap_r, int cap, const Soa& C);
void launch_halo_pack(const Launch& L, const int* dst_of, const DistLayout* lay, int cap_l, int cap_r,
                      const HaloFields& F, double* buf_l, double* buf_r);
void launch_halo_unpack(const Launch& L, const double* buf_l, const double* buf_r, const int* dst_of,
                        const DistLayout* lay, int cap_l, int cap_r, const HaloFields& F);

}  // namespace mph
