// mph_ctx.hip -- the C ABI of include/mph_gpu.h: device context, uploads, graph-replayed steps,
// field download in the reference's AoS layout and original particle order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "mph_dist.h"
#include "mph_env.h"
#include "mph_rows.h"

using namespace mph;

namespace mph {

int ctx_fail(MphCtx* c, int code, const std::string& msg)
{
    if (c) c->err = msg;
    return code;
}

int ctx_hip_fail(MphCtx* c, hipError_t e, const char* what)
{
    return ctx_fail(c, e == hipErrorOutOfMemory ? MPH_ERR_DEVICE_OOM : MPH_ERR_HIP,
                    std::string(what) + ": " + hipGetErrorString(e));
}

void* ctx_alloc(MphCtx* c, size_t bytes, int* status)
{
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) {
        *status = ctx_fail(c, e == hipErrorOutOfMemory ? MPH_ERR_DEVICE_OOM : MPH_ERR_HIP,
                           "hipMalloc(" + std::to_string(bytes) + " B): " + hipGetErrorString(e));
        return nullptr;
    }
    c->allocs.push_back(q);
    *status = MPH_OK;
    return q;
}

void ctx_dfree(MphCtx* c, void* p)
{
    if (!p) return;
    c->allocs.erase(std::remove(c->allocs.begin(), c->allocs.end(), p), c->allocs.end());
    (void)hipFree(p);
}

// Error flags raised by the kernels (DevState.overflow bits).
int ctx_state_status(MphCtx* c, const DevState& hs)
{
    if (hs.overflow & 4)
        return ctx_fail(c, MPH_ERR_NONFINITE, "non-finite particle position (diverged state)");
    if (hs.overflow & 1)
        return ctx_fail(c, MPH_ERR_NEIGHBOR_OVERFLOW, "a particle has more than 512 neighbours");
    if (hs.overflow & 2) return ctx_fail(c, MPH_ERR_CAPACITY, "a particle moved past a neighbouring slab");
    if (hs.overflow & 64)   // k_place: a cell start + slot past the particle count (never a fault)
        return ctx_fail(c, MPH_ERR_HIP, "cell sort: histogram inconsistent with the keys (placement out of range)");
    return MPH_OK;
}

int drop_graphs(MphCtx* c)
{
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    for (hipGraphExec_t* g : {&c->graph1, &c->graph1t, &c->graph8})
        if (*g) {
            MPH_HIP_OK(c, hipGraphExecDestroy(*g));
            *g = nullptr;
        }
    return MPH_OK;
}

void ctx_fill_launch(MphCtx* c)
{
    Launch& L = c->L;
    set_uniforms(c->P);
    // MPH_LIST_FULL=1: the lists keep every neighbour within the search radius, like the reference's
    // Neighbor[] (mph_neighbor_rows needs them); else only those the passes' sums can take
    if (env_int("MPH_LIST_FULL", 0) == 1) c->P.rlf = 3.0e38f;
    // MPH_LAZY_WALLS=0: no lazy wall steps (enqueue_step), every step searches and sums every wall
    // wave; slab contexts never take them (a halo wall may have a fluid neighbour on the next rank)
    c->lazy_walls = !c->dist && env_int("MPH_LAZY_WALLS", 1) != 0;
    // MPH_LEAN_STEPS=0: the lazy steps launch the kernels of the full steps' arithmetic (enqueue_step);
    // the lean search also needs the list radius below the search radius' FP32 band (lean_search_ok:
    // not with MPH_LIST_FULL=1)
    L.lean_ok = env_int("MPH_LEAN_STEPS", 1) != 0;
    L.lean_search = L.lean_ok && lean_search_ok(c->P);
    L.P = &c->P;
    L.stream = c->stream;
    // work-balanced XCD map of the passes from this many particles (MPH_XCD_BAL_MIN: tests force it
    // on small cases, the default keeps it off below 2^20 where the split kernel costs more)
    L.xcd_bal_min = env_is("MPH_XCD_BAL_MIN", "") ? (1 << 20) : env_int("MPH_XCD_BAL_MIN", 1 << 20);
    L.S = &c->Sd;
}

// calculateVirialStressAtParticle evaluates the step's lists at the positions after the step
// (main.cpp:672-673, 3077-3318): a pair of the shell MaxRadius < r <= MaxRadius + MARGIN at the search
// may have moved inside a radius by then, so the virial needs the reference's whole lists.  With
// the lists kept to the passes' radius (DevParams.rlf) the step's search is repeated over the same
// sorted set A and cell table (unchanged since the step's sort) storing every neighbour -- the
// lists the step would have built with MPH_LIST_FULL=1; the XCD work histogram is left alone.
int virial_full_lists(MphCtx* c)
{
    if (c->P.rlf >= 3.0e38f) return MPH_OK;
    DevParams Pf = c->P;
    Pf.rlf = 3.0e38f;
    Launch L = c->L;
    L.P = &Pf;
    L.xcd_bal_min = 0x7fffffff;
    launch_neighbors(L);
    MPH_HIP_OK(c, hipGetLastError());
    return MPH_OK;
}
}  // namespace mph

namespace {

// Force and Acceleration (main.cpp:2085-2096, 2892-2956) are outputs only: no kernel reads them,
// and every step overwrites all of them.  So only the last step of a replayed batch stores them
// (pass B -6 % at D1M); mph_get after any mph_step sees the last step's values as before.  The
// same holds in pass A for DensityA, VolStrainP, DivergenceP and, without surface tension (pass B
// then reads neither), GravityCenter and PressureA.  The virial (k_virial) runs after a batch.
// ev (phase timing, else null): three events recorded on the stream at the step's phase
// boundaries -- before the sort, after the search (neighbour search = sort + search, as the
// reference's calculateNeighbor holds its own cell sort), after the elastic substeps.
//
// Lazy wall steps take the same rule one kernel further up.  On a step that is not `last`, a wall
// walks no list in pass B, so what the search and pass A compute for a wall particle whose
// neighbours are all walls -- its list, PressureP, the pass-B record, fpart -- has no reader; the
// batch's last step computes all of it again.  Such a step marks the coarse cells of the non-wall
// particles in its sort, and its search skips the wall waves out of their reach (wave_idle_walls).
// Off (every step full) without the map (slab mode, MPH_LAZY_WALLS=0) and while the monitor kernels
// run, which read the walls' pressure on every step.
void enqueue_step(const Launch& L, bool last, hipEvent_t* ev = nullptr)
{
    if (ev) (void)hipEventRecord(ev[0], L.stream);
    Launch La = L;
    La.lazy = !last && L.cmap && !L.mon;
    // a lean step: a lazy step that also leaves out what it would compute only to drop it -- the
    // search NeighborCount and the shell's candidates, pass A the DensityA and GravityCenter sums when
    // they are not stored (below).  Under the conditions of a lazy step and no others.
    La.lean = La.lazy && L.lean_ok;
    launch_sort(La, 1);
    if (!last) {
        La.dens_a = La.vstrain = La.divp = nullptr;
        if (!L.P->surface) La.gx = La.gy = La.gz = La.pa = nullptr;
    }
    if (ev) {   // phase timing: the boundary between the search and pass A
        launch_neighbors(La);
        (void)hipEventRecord(ev[1], L.stream);
        launch_pass_a(La);
    } else {
        launch_search_pass_a(La);
    }
    if (last) {
        launch_pass_b(L);
    } else {
        Launch Lb = L;
        Lb.force = nullptr;
        Lb.acc = nullptr;
        Lb.lazy = La.lazy;   // (the grid of a lazy step's XCD map, list_grid)
        launch_pass_b(Lb);
    }
    launch_structure(L, last);
    if (ev) (void)hipEventRecord(ev[2], L.stream);
    if (L.mon) launch_monitor(L, *L.mon);   // monitors on: this step's sample (mph_monitor.hip)
}

// store_last = false: no step of the graph stores the output-only fields (graph1t, the steps of a
// remainder before its last one)
int capture(MphCtx* c, int steps, hipGraphExec_t* out, bool store_last = true)
{
    hipGraph_t g = nullptr;
    MPH_HIP_OK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    for (int k = 0; k < steps; ++k) enqueue_step(c->L, store_last && k == steps - 1);
    MPH_HIP_OK(c, hipStreamEndCapture(c->stream, &g));
    MPH_HIP_OK(c, hipGraphInstantiate(out, g, nullptr, nullptr, 0));
    MPH_HIP_OK(c, hipGraphDestroy(g));
    MPH_HIP_OK(c, hipGraphUpload(*out, c->stream));   // so the first launch costs what later ones do
    return MPH_OK;
}

// The step graphs, captured at the first mph_step whatever its count: a caller that warms up with
// fewer than 8 steps (the driver's bench: 5) would otherwise capture and upload the 8-step graph
// inside its first long run.
static int capture_graphs(MphCtx* c)
{
    if (!c->graph1) MPH_CK(capture(c, 1, &c->graph1));
    if (!c->graph1t) MPH_CK(capture(c, 1, &c->graph1t, false));
    if (!c->graph8) MPH_CK(capture(c, 8, &c->graph8));
    return MPH_OK;
}

// `left` (< 8) single steps: the output-only stores on the last one only, as in an 8-step batch
static int launch_singles(MphCtx* c, int left)
{
    for (; left > 1; --left) MPH_HIP_OK(c, hipGraphLaunch(c->graph1t, c->stream));
    if (left == 1) MPH_HIP_OK(c, hipGraphLaunch(c->graph1, c->stream));
    return MPH_OK;
}

// phase timing: the events of a batch of `steps` steps (three per step) into the neighbour /
// explicit sums
int accumulate_phases(MphCtx* c, const std::vector<hipEvent_t>& ev, int steps)
{
    MPH_HIP_OK(c, hipEventSynchronize(ev[3 * (size_t)steps - 1]));
    for (size_t k = 0; k + 2 < 3 * (size_t)steps; k += 3) {
        float a = 0.0f, b = 0.0f;
        MPH_HIP_OK(c, hipEventElapsedTime(&a, ev[k], ev[k + 1]));
        MPH_HIP_OK(c, hipEventElapsedTime(&b, ev[k + 1], ev[k + 2]));
        c->phase_ms[0] += a;
        c->phase_ms[1] += b;
    }
    return MPH_OK;
}

// Sorted device arrays -> host original order: the first `len` elements of each array of src and
// the id array of their order (A.id / B.id); put(h, i, id) copies particle i's elements from the
// host copies to where original index id belongs.  h is an array of N vectors, one per source
// array: h[k][i] is element i of src[k] (a single array: h[0][i]).  Slab mode: ghosts (id < 0) skipped.
template <typename T, size_t N, typename Put>
int download(MphCtx* c, T* const (&src)[N], size_t len, const int* ids, Put put)
{
    std::vector<T> h[N];
    std::vector<int> id;
    for (size_t k = 0; k < N; ++k) MPH_CK(fetch(c, (const T*)src[k], h[k], len));
    MPH_CK(fetch(c, ids, id, (size_t)c->n));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < id.size(); ++i)
        if (id[i] >= 0) put(h, i, (size_t)id[i]);
    return MPH_OK;
}

int download_struct_m33(MphCtx* c, const double* d, double* out)
{
    const int ns = c->Sd.n_own;   // slots computed here (slab mode: owned)
    std::memset(out, 0, sizeof(double) * 9 * (size_t)c->n_glob);
    if (ns == 0) return MPH_OK;
    const size_t fes = (size_t)c->Sd.fes;   // nine element planes (StructDev)
    std::vector<double> h(fes * 9);
    MPH_HIP_OK(c, hipMemcpyAsync(h.data(), d, sizeof(double) * 9 * fes, hipMemcpyDeviceToHost, c->stream));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    for (int s = 0; s < ns; ++s) {
        double* o = out + (size_t)9 * c->sl_orig[s];
        for (int e = 0; e < 9; ++e) o[e] = h[e * fes + s];
    }
    return MPH_OK;
}

// A launch's start event behind a cross-stream wait reads as early as the wait packet itself (the
// time the stream went idle), so each launch that follows a join also keeps a floor: an event on
// the other stream at the joined point; its start is the later of the two.
struct EventProfiler final : Profiler {
    struct Rec { std::string name; hipEvent_t a, b; int floor; };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> floors;
    std::map<hipStream_t, int> pending;
    bool events(const char* name, hipStream_t s, hipEvent_t* start, hipEvent_t* stop) override
    {
        Rec r{name, nullptr, nullptr, -1};
        const auto it = pending.find(s);
        if (it != pending.end()) {
            r.floor = it->second;
            pending.erase(it);
        }
        (void)hipEventCreate(&r.a);
        (void)hipEventCreate(&r.b);
        recs.push_back(r);
        *start = r.a;
        *stop = r.b;
        return true;
    }
    void join(hipStream_t waiting, hipStream_t from) override
    {
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        (void)hipEventRecord(e, from);
        floors.push_back(e);
        pending[waiting] = (int)floors.size() - 1;
    }
    ~EventProfiler() override
    {
        for (auto& r : recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
        for (auto e : floors) (void)hipEventDestroy(e);
    }
};

}  // namespace

namespace mph {

// Shared body of mph_create (dist == nullptr) and the slab-mode constructors of mph_dist.hip
// (dist != nullptr: only this rank's particles are uploaded, the cell grid covers its window).
static thread_local std::string g_create_error;   // mph_last_error(NULL) after a failed create

// The arguments of a create, and what one phase of ctx_init hands to the later ones.
struct CreateArgs {
    const MphConfig* cfg;
    int n;
    const int* property;
    const double *pos, *pos0, *vel;
    int device;
    const int* ids;
    int n_glob;
    bool gpu_init = false;     // the fixed elastic lists are built on the device (init_host_state)
    std::vector<int> owned;    // slab mode: the inputs this rank owns (init_capacity)
    int cap = 0;               // capacity of every per-particle array (init_capacity)
};

template <typename T, typename V>
static hipError_t upload(MphCtx* c, T* d, const V& v)
{
    return hipMemcpyAsync(d, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice, c->stream);
}

static int init_check_args(MphCtx* c, const CreateArgs& a)
{
    if (a.cfg->dim != 2 && a.cfg->dim != 3) return MPH_ERR_ARG;
    if (a.cfg->module < 0 || a.cfg->module > MPH_MODULE_NONE) return MPH_ERR_ARG;
    if (!(a.cfg->particle_spacing > 0.0) || !(a.cfg->dt > 0.0) || !(a.cfg->elastic_dt > 0.0)) return MPH_ERR_ARG;
    for (int i = 0; i < a.n; ++i)
        if (a.property[i] < 0 || a.property[i] >= kTypes) return MPH_ERR_ARG;
    c->cfg = *a.cfg;
    c->n = a.n;
    c->n_glob = a.n;
    if (a.ids) {
        if (!c->dist || a.n_glob < a.n) return MPH_ERR_ARG;
        for (int i = 0; i < a.n; ++i)
            if (a.ids[i] < 0 || a.ids[i] >= a.n_glob || (i > 0 && a.ids[i] <= a.ids[i - 1]))
                return ctx_fail(c, MPH_ERR_ARG, "slab-local creation: ids must be ascending original indices below n_glob");
        c->gid.assign(a.ids, a.ids + a.n);
        c->n_glob = a.n_glob;
    }
    c->device = a.device;
    c->time = a.cfg->time;
    return MPH_OK;
}

// device and stream, derived constants, host copies of the static inputs, the elastic lists' host
// part and the kernels' parameters
static int init_host_state(MphCtx* c, CreateArgs& a)
{
    MPH_HIP_OK(c, hipSetDevice(a.device));
    MPH_HIP_OK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    derive_constants(c->cfg, c->h);
    c->prop.assign(a.property, a.property + a.n);
    c->pos0.assign(a.pos0, a.pos0 + 3 * (size_t)a.n);
    std::string err;
    // the fixed Lagrangian structure lists: on the device for a single context (calculate-
    // InitialNeighbor + calculateNormalizer as kernels, launch_struct_init); in slab mode on the
    // host over the particles this rank was given, which also routes the static ghost slots
    // (dist_struct_setup).  MPH_STRUCT_INIT=host selects the host build everywhere.
    a.gpu_init = !c->dist && !env_is("MPH_STRUCT_INIT", "host");
    MPH_CK(ctx_fail(c, build_structure(c->cfg, c->h, a.n, a.property, a.pos0, c->S, err, !a.gpu_init), err));
    make_dev_params(c->cfg, c->h, a.n, (int)c->S.orig.size(), c->P);
    return MPH_OK;
}

// the cell grid (order, cell counts, origin) and the interior boxes of the fast minimum image
static int init_grid(MphCtx* c, const CreateArgs& a)
{
    const double rc = std::sqrt(c->P.rc2);
    std::string err;
    {
        // z slabs of a 3-D problem: z in the middle of the cell order, so the ghosts beyond both
        // faces are long runs (whole wavefronts) at the ends of every plane (DevParams.perm;
        // MPH_SLAB_PERM=0 keeps (x, y, z); =1..4 force an order on any 3-D context, =force
        // orders a single 3-D context the z-slab way -- A/B timing and the parity tests)
        const std::string pv = env_str("MPH_SLAB_PERM");
        const bool zslab = a.cfg->dim == 3 && c->dist && c->dist->g.axis == 2;
        const bool forced = pv.size() == 1 && pv[0] >= '1' && pv[0] <= '4';
        c->P.perm = 0;
        if (a.cfg->dim == 3 && (forced || pv == "force" || (zslab && pv != "0")))
            c->P.perm = forced ? pv[0] - '0' : choose_cell_order(c->h, a.n, a.pos, rc);
        int r = choose_grid(c->h, a.cfg->dim, rc, kContigReach, c->P.gc, c->P.ginv, err, c->P.perm);
        if (r != MPH_OK) return ctx_fail(c, r, err);
        set_uniforms(c->P);
    }
    // interior box for the wave-uniform fast minimum image (k_neighbors / passes): >= 3 cells
    // (+1e-9 relative margin) from every periodic face; needs > 12 cells on every active axis
    // (stencil half-width + 1 cells from every periodic face; the candidate offsets then stay
    // below a quarter of the domain width, which needs > 4 x that many cells on every axis)
    c->P.sa = kContigReach;
    c->P.fast_ok = 1;
    c->P.seam_always = 0;
    // the grid's origin in an empty band of the initial particles (choose_grid_origin;
    // MPH_GRID_SHIFT=0 keeps dmin): the search's interior box is then in grid offsets
    const bool shift = env_str("MPH_GRID_SHIFT")[0] != '0';
    for (int d = 0; d < 3; ++d) {
        if (d == 2 && a.cfg->dim == 2) {
            c->P.inner_lo[d] = c->P.sinner_lo[d] = -1e300;
            c->P.inner_hi[d] = c->P.sinner_hi[d] = 1e300;
            continue;
        }
        const int m = stencil_margin(c->P, d);
        if (c->P.gc[d] <= 4 * m) c->P.fast_ok = 0;
        const double cw = c->h.dw[d] / c->P.gc[d];
        c->P.inner_lo[d] = c->h.dmin[d] + m * cw * (1.0 + 1e-9);
        c->P.inner_hi[d] = c->h.dmax[d] - m * cw * (1.0 + 1e-9);
        const int s0 = shift && c->P.fast_ok ? choose_grid_origin(c->h, a.n, a.pos, d, c->P.gc[d], m) : 0;
        c->P.corg[d] = c->h.dmin[d] + s0 * cw;
        c->P.sinner_lo[d] = m * cw * (1.0 + 1e-9);
        c->P.sinner_hi[d] = c->h.dw[d] - m * cw * (1.0 + 1e-9);
    }
    return MPH_OK;
}

static int init_capacity(MphCtx* c, CreateArgs& a)
{
    // slab mode: owned subset, local window grid along the slab axis, array capacity
    a.cap = a.n;
    if (c->dist) {
        MPH_CK(dist_setup(c, a.pos, a.owned));
        a.cap = c->dist->cap;
        c->n = (int)a.owned.size();
        c->P.n = c->n;
    }
    if (a.cap > kIndexMask)
        return ctx_fail(c, MPH_ERR_UNSUPPORTED, "more than 2^28 particles in one context (neighbour-list entries "
                                            "carry the type in their top bits)");
    if ((long long)a.cap * 48 >= (long long)kGatherOob)
        return ctx_fail(c, MPH_ERR_UNSUPPORTED, "more than 89 million particles in one context (the list passes "
                                            "gather with 32-bit byte offsets)");
    {
        // the search addresses the cell table with 32-bit byte offsets (buffer descriptors)
        const long long nc = (long long)c->P.gc[0] * c->P.gc[1] * c->P.gc[2];
        if (nc + 1 > (1LL << 30))
            return ctx_fail(c, MPH_ERR_UNSUPPORTED, "cell grid of " + std::to_string(nc) +
                                                    " cells: more than 2^30 (4 GiB of cell starts)");
        c->P.ncell = (int)nc;
    }
    return MPH_OK;
}

// the per-type tables, every array of c->L, and the initial DevState
static int init_alloc(MphCtx* c, const CreateArgs& a)
{
    DevTables& T = c->tables;
    for (int t = 0; t < kTypes; ++t) {
        for (int u = 0; u < kTypes; ++u) {
            T.ratio[t * kTypes + u] = c->P.ratio[t][u];
            T.mu_ij[t * kTypes + u] = c->P.mu_ij[t][u];
        }
        T.cofa[t] = c->P.cofa[t];
        T.mass[t] = c->P.mass[t];
        T.inv_mass[t] = c->P.inv_mass[t];
        T.bulk[t] = c->P.bulk[t];
        T.bulk_visc[t] = c->P.bulk_visc[t];
    }
    // device allocations (capacity `cap` per particle array)
    const int cap = a.cap;
    const size_t ntile = ((size_t)cap + kTile - 1) / kTile;
    DevTables* dT = nullptr;
    MPH_CK(ctx_dalloc(c, &dT, 1));
    c->L.T = dT;
    MPH_CK(ctx_dalloc(c, &c->L.st, 1));
    for (Soa* s : {&c->L.A, &c->L.B}) {
        const size_t m = (size_t)cap + kPad;
        MPH_CK(ctx_dalloc(c, &s->x, m)); MPH_CK(ctx_dalloc(c, &s->y, m)); MPH_CK(ctx_dalloc(c, &s->z, m));
        MPH_CK(ctx_dalloc(c, &s->vx, m)); MPH_CK(ctx_dalloc(c, &s->vy, m)); MPH_CK(ctx_dalloc(c, &s->vz, m));
        MPH_CK(ctx_dalloc(c, &s->type, m)); MPH_CK(ctx_dalloc(c, &s->id, m));
    }
    MPH_CK(ctx_dalloc(c, &c->L.A.p6, 3 * (size_t)cap));
    // the search's FP32 candidate records (kPad past the last)
    MPH_CK(ctx_dalloc(c, &c->L.A.f4, (size_t)cap + kPad));
    MPH_CK(ctx_dalloc(c, &c->order, cap));
    MPH_CK(ctx_dalloc(c, &c->L.key, cap)); MPH_CK(ctx_dalloc(c, &c->L.slot, cap));
    MPH_CK(ctx_dalloc(c, &c->L.tmp, cap));
    MPH_CK(ctx_dalloc(c, &c->L.cnt, c->P.ncell)); MPH_CK(ctx_dalloc(c, &c->L.start, (size_t)c->P.ncell + 1));
    // the cell scan's block totals (k_scan_reduce; structure init)
    const size_t bs = (size_t)c->P.ncell / 4096 + 2;   // bsum_stride (mph_sort.hip)
    MPH_CK(ctx_dalloc(c, &c->L.bsum, bs));
    MPH_CK(ctx_dalloc(c, &c->L.nbr, ntile * kTileStride)); MPH_CK(ctx_dalloc(c, &c->L.ncount, cap));
    MPH_CK(ctx_dalloc(c, &c->L.nbcount, cap));
    // the lists' row jumps: a header word per wave, a word of gap starts per lane (whole tiles)
    MPH_CK(ctx_dalloc(c, &c->L.lhdr, ntile)); MPH_CK(ctx_dalloc(c, &c->L.lgap, ntile * kTile));
    for (double** p : {&c->L.pres, &c->L.gx, &c->L.gy, &c->L.gz, &c->L.pa}) MPH_CK(ctx_dalloc(c, p, cap));
    for (double4** p : {&c->L.force, &c->L.acc, &c->L.fpart, &c->L.rec}) MPH_CK(ctx_dalloc(c, p, cap));
    for (double** p : {&c->L.dens_a, &c->L.vstrain, &c->L.divp}) MPH_CK(ctx_dalloc(c, p, cap));
    MPH_HIP_OK(c, hipMemsetAsync(c->L.cnt, 0, sizeof(int) * c->P.ncell, c->stream));
    MPH_HIP_OK(c, hipMemsetAsync(c->L.bsum, 0, sizeof(int) * bs, c->stream));
    MPH_HIP_OK(c, hipMemsetAsync(c->L.force, 0, sizeof(double4) * std::max(cap, 1), c->stream));
    MPH_HIP_OK(c, hipMemsetAsync(c->L.acc, 0, sizeof(double4) * std::max(cap, 1), c->stream));
    MPH_HIP_OK(c, hipMemcpyAsync(dT, &T, sizeof(DevTables), hipMemcpyHostToDevice, c->stream));
    DevState st{};
    st.time = a.cfg->time;
    for (int t = 0; t < kTypes; ++t)
        for (int d = 0; d < 3; ++d) {
            st.wall_c[t][d] = a.cfg->wall_center[t][d];
            st.wall_vel[t][d] = a.cfg->wall_velocity[t][d];
            st.wall_omega[t][d] = a.cfg->wall_omega[t][d];
            for (int e = 0; e < 3; ++e) st.wall_rot[t][d][e] = c->h.wall_rot[t][d][e];
        }
    MPH_HIP_OK(c, hipMemcpyAsync(c->L.st, &st, sizeof(DevState), hipMemcpyHostToDevice, c->stream));
    return MPH_OK;
}

static int init_upload_particles(MphCtx* c, const CreateArgs& a)
{
    // upload into the B set (original order, id = file index); the init sort reorders it
    const int m = c->n;
    std::vector<int> sel(m);
    for (int i = 0; i < m; ++i) sel[i] = c->dist ? a.owned[i] : i;
    std::vector<double> comp(m);
    std::vector<int> gids(m), types(m);
    double* dstc[6] = {c->L.B.x, c->L.B.y, c->L.B.z, c->L.B.vx, c->L.B.vy, c->L.B.vz};
    for (int k = 0; k < 6; ++k) {
        const double* src = k < 3 ? a.pos : a.vel;
        for (int i = 0; i < m; ++i) comp[i] = src[3 * (size_t)sel[i] + (k % 3)];
        MPH_HIP_OK(c, hipMemcpy(dstc[k], comp.data(), sizeof(double) * m, hipMemcpyHostToDevice));
    }
    for (int i = 0; i < m; ++i) { gids[i] = glob_id(c, sel[i]); types[i] = a.property[sel[i]]; }
    MPH_HIP_OK(c, hipMemcpy(c->L.B.type, types.data(), sizeof(int) * m, hipMemcpyHostToDevice));
    MPH_HIP_OK(c, hipMemcpy(c->L.B.id, gids.data(), sizeof(int) * m, hipMemcpyHostToDevice));
    return MPH_OK;
}

// calculateInitialNeighbor + calculateNormalizer on the device (single context: the local slots
// are all slots, in file order); the host keeps counts and normalizers for mph_get
static int elastic_device_build(MphCtx* c, int ns)
{
    StructDev& D = c->Sd;
    StructureInit& S = c->S;
    ctx_fill_launch(c);
    auto alloc = [](void* ctx, size_t bytes) -> void* {
        int st = MPH_OK;
        return ctx_alloc((MphCtx*)ctx, bytes, &st);
    };
    const int r = launch_struct_init(c->L, ns, D.x0, c->L.key, c->L.slot, c->L.tmp, c->order, D.ocnt, D.icnt,
                                     &D.eo_nb, &D.wo, &D.ei_nb, &D.wi, D.L, D.wx0, alloc, c);
    if (r == -2) return ctx_fail(c, MPH_ERR_NEIGHBOR_OVERFLOW, "a structure particle has >= 512 initial neighbours");
    if (r == -3) return ctx_fail(c, MPH_ERR_DEVICE_OOM, "structure list allocation failed");
    if (r != 0) return ctx_fail(c, MPH_ERR_HIP, "structure initialisation kernels failed");
    S.count.resize(ns);
    S.normalizer.resize((size_t)ns * 9);
    MPH_HIP_OK(c, hipMemcpyAsync(S.count.data(), D.ocnt, sizeof(int) * ns, hipMemcpyDeviceToHost, c->stream));
    MPH_HIP_OK(c, hipMemcpyAsync(S.normalizer.data(), D.L, sizeof(double) * 9 * ns, hipMemcpyDeviceToHost,
                             c->stream));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    return MPH_OK;
}

// ELL tiles of the host-built fixed out-list and of its transpose (StructDev), computed slots only
static int elastic_host_build(MphCtx* c, const std::vector<int>& lsl, int no)
{
    StructDev& D = c->Sd;
    const StructureInit& S = c->S;
    const int nl = (int)lsl.size();
    std::vector<int> loc(S.orig.size(), -1);
    for (int k = 0; k < nl; ++k) loc[lsl[k]] = k;
    const size_t ntile_s = ((size_t)std::max(no, 1) + 63) / 64;
    std::vector<int> ocnt(std::max(no, 1), 0), icnt(std::max(no, 1), 0);
    int wo = 0, wi = 0;
    for (int s = 0; s < no; ++s) {
        const int g = lsl[s];
        ocnt[s] = S.offset[g + 1] - S.offset[g];
        icnt[s] = S.in_offset[g + 1] - S.in_offset[g];
        wo = std::max(wo, ocnt[s]);
        wi = std::max(wi, icnt[s]);
    }
    wo = std::max(wo, 1);
    wi = std::max(wi, 1);
    D.wo = wo;
    D.wi = wi;
    std::vector<int> eo_nb(ntile_s * wo * 64, 0), ei_nb(ntile_s * wi * 64, 0);
    std::vector<double4> wx0(nl, make_double4(0.0, 0.0, 0.0, 0.0));
    for (int s = 0; s < no; ++s) {
        const int g = lsl[s];
        const size_t base_o = (size_t)(s >> 6) * wo * 64 + (s & 63);
        double c3[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < ocnt[s]; ++k) {
            const size_t q = S.offset[g] + k;
            const double* pr = &S.pair_out[4 * q];
            eo_nb[base_o + (size_t)k * 64] = loc[S.nbr[q]];
            for (int d = 0; d < 3; ++d) c3[d] += pr[3] * pr[d];
        }
        wx0[s] = make_double4(c3[0], c3[1], c3[2], 0.0);
        const size_t base_i = (size_t)(s >> 6) * wi * 64 + (s & 63);
        for (int k = 0; k < icnt[s]; ++k) {
            const size_t q = S.in_offset[g] + k;
            ei_nb[base_i + (size_t)k * 64] = loc[S.in_nbr[q]];
        }
    }
    for (int e : eo_nb) if (e < 0) return ctx_fail(c, MPH_ERR_DOMAIN, "structure list leaves the ghost slots");
    for (int e : ei_nb) if (e < 0) return ctx_fail(c, MPH_ERR_DOMAIN, "structure list leaves the ghost slots");
    std::vector<double> Lm((size_t)nl * 9);
    for (int s = 0; s < nl; ++s)
        std::memcpy(&Lm[(size_t)9 * s], &S.normalizer[(size_t)9 * lsl[s]], sizeof(double) * 9);
    MPH_CK(ctx_dalloc(c, &D.eo_nb, eo_nb.size()));
    MPH_CK(ctx_dalloc(c, &D.ei_nb, ei_nb.size()));
    MPH_HIP_OK(c, upload(c, D.ocnt, ocnt)); MPH_HIP_OK(c, upload(c, D.icnt, icnt));
    MPH_HIP_OK(c, upload(c, D.eo_nb, eo_nb));
    MPH_HIP_OK(c, upload(c, D.ei_nb, ei_nb));
    MPH_HIP_OK(c, upload(c, D.wx0, wx0));
    MPH_HIP_OK(c, upload(c, D.L, Lm));
    return MPH_OK;
}

// elastic solid: local slots = [computed here | ghosts] (single GPU: every slot, no ghosts)
static int init_elastic(MphCtx* c, const CreateArgs& a)
{
    const int ns = (int)c->S.orig.size();
    if (ns == 0) return MPH_OK;
    StructDev& D = c->Sd;
    StructureInit& S = c->S;
    std::vector<int> lsl;   // local slot -> global slot
    int no = ns, ni = ns;
    if (c->dist) {
        MPH_CK(dist_struct_setup(c, lsl, no, ni));
    } else {
        lsl.resize(ns);
        for (int s = 0; s < ns; ++s) lsl[s] = s;
    }
    const int nl = (int)lsl.size();
    D.n_own = no;
    D.n_inner = ni;
    c->sl_orig.resize(nl);
    for (int k = 0; k < nl; ++k) c->sl_orig[k] = glob_id(c, S.orig[lsl[k]]);
    c->sl_s.assign(lsl.begin(), lsl.begin() + no);
    const int sd = c->P.dim;
    MPH_CK(ctx_dalloc(c, &D.orig, nl));
    MPH_CK(ctx_dalloc(c, &D.ocnt, std::max(no, 1))); MPH_CK(ctx_dalloc(c, &D.icnt, std::max(no, 1)));
    MPH_CK(ctx_dalloc(c, &D.bidx, nl));
    MPH_CK(ctx_dalloc(c, &D.wx0, nl));
    MPH_CK(ctx_dalloc(c, &D.L, (size_t)nl * 9)); MPH_CK(ctx_dalloc(c, &D.lame, nl)); MPH_CK(ctx_dalloc(c, &D.inv_rho, nl));
    MPH_CK(ctx_dalloc(c, &D.clamp, nl));
    for (double4** p : {&D.x0, &D.x, &D.v, &D.u}) MPH_CK(ctx_dalloc(c, p, nl));
    MPH_CK(ctx_dalloc(c, &D.P, (size_t)nl * (sd == 2 ? 1 : 3)));
    for (double** p : {&D.F, &D.E, &D.S}) MPH_CK(ctx_dalloc(c, p, (size_t)nl * 9));
    D.fes = nl;
    std::vector<double2> lame(nl);
    std::vector<double> irho(nl);
    std::vector<int> clamp(nl);
    std::vector<double4> x0(nl);
    for (int s = 0; s < nl; ++s) {
        const int g = lsl[s];
        const int i = S.orig[g];
        const int t = a.property[i];
        lame[s] = make_double2(S.lame_l[g], S.lame_m[g]);
        irho[s] = 1.0 / a.cfg->density[t];
        const double* p0 = a.pos0 + 3 * (size_t)i;
        int cl = 0;   // updateElasticPosition module clamps (main.cpp:1918-2044)
        switch (a.cfg->module) {
        case MPH_MODULE_BAR: cl = p0[0] < 0.001 ? 1 : 0; break;
        case MPH_MODULE_DAM: cl = p0[1] < 0.002 ? 1 : 0; break;
        case MPH_MODULE_TUREK_HRON: cl = p0[0] < 0.205 ? 2 : 0; break;
        case MPH_MODULE_ROLLING1: cl = p0[1] < 0.003 ? 1 : 0; break;
        case MPH_MODULE_HYDROELASTIC: cl = (p0[0] < 0.01 || p0[0] > 1.99) ? 1 : 0; break;
        default: cl = 0;
        }
        clamp[s] = cl;
        x0[s] = make_double4(p0[0], p0[1], p0[2], (double)t);
    }
    MPH_HIP_OK(c, upload(c, D.x0, x0));
    MPH_CK(a.gpu_init ? elastic_device_build(c, ns) : elastic_host_build(c, lsl, no));
    MPH_HIP_OK(c, hipMemcpyAsync(D.orig, c->sl_orig.data(), sizeof(int) * nl, hipMemcpyHostToDevice, c->stream));
    {
        std::vector<int> slot_of((size_t)c->n_glob, -1);
        for (int s = 0; s < no; ++s) slot_of[c->sl_orig[s]] = s;
        MPH_CK(ctx_dalloc(c, &D.slot_of, slot_of.size()));
        MPH_HIP_OK(c, hipMemcpy(D.slot_of, slot_of.data(), sizeof(int) * slot_of.size(), hipMemcpyHostToDevice));
    }
    MPH_HIP_OK(c, upload(c, D.lame, lame));
    MPH_HIP_OK(c, upload(c, D.inv_rho, irho));
    MPH_HIP_OK(c, upload(c, D.clamp, clamp));
    MPH_HIP_OK(c, hipMemsetAsync(D.P, 0, sizeof(double4) * (sd == 2 ? 1 : 3) * nl, c->stream));
    MPH_HIP_OK(c, hipMemsetAsync(D.u, 0, sizeof(double4) * nl, c->stream));
    MPH_HIP_OK(c, hipMemsetAsync(D.bidx, 0, sizeof(int) * nl, c->stream));
    for (double* m : {D.F, D.E, D.S})
        MPH_HIP_OK(c, hipMemsetAsync(m, 0, sizeof(double) * 9 * nl, c->stream));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    return MPH_OK;
}

// slab mode: the exchange's allocations, the initial ghost exchange and the init sums; else the
// initialisation sums of main.cpp:565-568 (calculateNeighbor, DensityA, GravityCenter, DensityP)
static int init_first_sums(MphCtx* c)
{
    ctx_fill_launch(c);
    if (c->dist) {
        MPH_CK(dist_alloc(c));
        MPH_CK(dist_init(c));
    } else {
        launch_sort(c->L, 0);
        launch_search_pass_a(c->L);
        if (c->lazy_walls) {   // the coarse map of the lazy wall steps: all zero between steps
            const size_t mb = coarse_map_bytes(c->P.gc);
            MPH_CK(ctx_dalloc(c, &c->L.cmap, mb));
            MPH_HIP_OK(c, hipMemsetAsync(c->L.cmap, 0, mb, c->stream));
            c->L.cmap_bytes = (int)mb;
        }
    }
    MPH_HIP_OK(c, hipGetLastError());
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    DevState hs;
    MPH_HIP_OK(c, hipMemcpy(&hs, c->L.st, kStateHead, hipMemcpyDeviceToHost));
    return ctx_state_status(c, hs);
}

static int ctx_init(MphCtx* c, CreateArgs& a)
{
    MPH_CK(init_check_args(c, a));
    MPH_CK(init_host_state(c, a));
    MPH_CK(init_grid(c, a));
    MPH_CK(init_capacity(c, a));
    MPH_CK(init_alloc(c, a));
    MPH_CK(init_upload_particles(c, a));
    MPH_CK(init_elastic(c, a));
    return init_first_sums(c);
}

void ctx_set_global_error(const std::string& msg) { g_create_error = msg; }

int ctx_create(MphCtx** out, const MphConfig* cfg, int n, const int* property, const double* pos,
               const double* pos0, const double* vel, int device, MphDist* dist, const int* ids, int n_glob)
{
    g_create_error.clear();
    if (!out || !cfg || n < 0 || (n > 0 && (!property || !pos || !pos0 || !vel))) {
        delete dist;
        g_create_error = "invalid argument";
        return MPH_ERR_ARG;
    }
    *out = nullptr;
    MphCtx* c = new MphCtx();
    c->dist = dist;
    CreateArgs a{cfg, n, property, pos, pos0, vel, device, ids, n_glob};
    const int r = ctx_init(c, a);
    if (r != MPH_OK) {
        g_create_error = c->err.empty() ? "mph_create failed with status " + std::to_string(r) : c->err;
        mph_destroy(c);
        return r;
    }
    *out = c;
    return MPH_OK;
}

}  // namespace mph

extern "C" {

int mph_create(MphCtx** out, const MphConfig* cfg, int n, const int* property, const double* pos,
               const double* pos0, const double* vel, int device)
{
    return ctx_create(out, cfg, n, property, pos, pos0, vel, device, nullptr);
}

// Step batching: launch the steps accepted but not launched (single-step graphs, each storing the
// output-only fields, so the last one leaves them current) and read the error flags of everything
// launched.  Every entry point that reads or changes the state, or waits for it, calls this first.
static int ctx_flush(MphCtx* c)
{
    if (!c->pending && !c->unchecked) return MPH_OK;
    MPH_HIP_OK(c, hipSetDevice(c->device));
    if (c->pending) MPH_CK(capture_graphs(c));
    if (c->pending) MPH_CK(launch_singles(c, c->pending));
    c->pending = 0;
    c->unchecked = false;
    DevState hs;
    MPH_HIP_OK(c, hipMemcpyAsync(&hs, c->L.st, kStateHead, hipMemcpyDeviceToHost, c->stream));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    return ctx_state_status(c, hs);
}

// mph_step with batching on: the steps are counted and launched 8 at a time from the 8-step graph
// (output-only fields stored on each batch's last step, as a multi-step mph_step does); the error
// flags of the last launched batch are copied back behind it and read without waiting once they
// have landed, so an error surfaces at most a batch or two late, and at the latest at the next
// flush point (mph_synchronize, mph_get, the writers, ...).
static int step_batched(MphCtx* c, int nsteps)
{
    for (int k = 0; k < nsteps; ++k) c->time += c->cfg.dt;
    c->stepped = true;
    c->a_current = true;
    c->pending += nsteps;
    bool launched = false;
    MPH_CK(capture_graphs(c));
    while (c->pending >= 8) {
        MPH_HIP_OK(c, hipGraphLaunch(c->graph8, c->stream));
        c->pending -= 8;
        launched = true;
    }
    if (launched) {
        MPH_HIP_OK(c, hipMemcpyAsync(c->hs_pin, c->L.st, kStateHead, hipMemcpyDeviceToHost, c->stream));
        MPH_HIP_OK(c, hipEventRecord(c->ev_status, c->stream));
        c->unchecked = true;
    }
    if (c->unchecked && hipEventQuery(c->ev_status) == hipSuccess) {
        DevState hs;
        std::memcpy(&hs, c->hs_pin, kStateHead);
        MPH_CK(ctx_state_status(c, hs));
    }
    return MPH_OK;
}

int mph_set_step_batching(MphCtx* c, int on)
{
    if (!c) return MPH_ERR_ARG;
    if (c->dist) return on ? ctx_fail(c, MPH_ERR_ARG, "step batching is not available in slab mode") : MPH_OK;
    MPH_HIP_OK(c, hipSetDevice(c->device));
    if (!on) {
        c->batch_steps = false;
        return ctx_flush(c);
    }
    if (!c->hs_pin) MPH_HIP_OK(c, hipHostMalloc(&c->hs_pin, kStateHead, hipHostMallocDefault));
    if (!c->ev_status) MPH_HIP_OK(c, hipEventCreateWithFlags(&c->ev_status, hipEventDisableTiming));
    c->batch_steps = true;
    return MPH_OK;
}

int mph_step(MphCtx* c, int nsteps)
{
    if (!c || nsteps < 0) return MPH_ERR_ARG;
    MPH_HIP_OK(c, hipSetDevice(c->device));
    if (c->dist) return dist_step(c, nsteps);
    if (nsteps == 0 || c->n == 0) {
        for (int k = 0; k < nsteps; ++k) c->time += c->cfg.dt;
        return MPH_OK;
    }
    if (c->batch_steps && !c->phase_timing) return step_batched(c, nsteps);
    MPH_CK(ctx_flush(c));
    int left = nsteps;
    if (c->phase_timing) {
        // the graphs' batches (8 steps, then single steps; the output-only stores on each batch's
        // last step) as direct launches with the phase events (HIP cannot time events recorded
        // inside a captured graph), read after every batch
        while (left > 0) {
            const int b = left >= 8 ? 8 : 1;
            for (int k = 0; k < b; ++k) enqueue_step(c->L, k == b - 1, c->ev8.data() + 3 * k);
            MPH_HIP_OK(c, hipGetLastError());
            MPH_CK(accumulate_phases(c, c->ev8, b));
            left -= b;
        }
    } else {
        MPH_CK(capture_graphs(c));
        while (left >= 8) { MPH_HIP_OK(c, hipGraphLaunch(c->graph8, c->stream)); left -= 8; }
        MPH_CK(launch_singles(c, left));
    }
    for (int k = 0; k < nsteps; ++k) c->time += c->cfg.dt;
    c->stepped = true;
    c->a_current = true;
    // the error flags, copied into pinned memory behind the steps (a pageable copy is staged by the
    // runtime).  Polling the stream instead of the blocking wait measured the same per call
    // (profiles/r05/sync_path/).
    if (!c->hs_pin) MPH_HIP_OK(c, hipHostMalloc(&c->hs_pin, kStateHead, hipHostMallocDefault));
    MPH_HIP_OK(c, hipMemcpyAsync(c->hs_pin, c->L.st, kStateHead, hipMemcpyDeviceToHost, c->stream));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    DevState hs;
    std::memcpy(&hs, c->hs_pin, kStateHead);
    MPH_CK(ctx_state_status(c, hs));
    return MPH_OK;
}

int mph_synchronize(MphCtx* c)
{
    if (!c) return MPH_ERR_ARG;
    MPH_CK(ctx_flush(c));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    // slab mode: the second stream too (halo, face pass B, early send, elastic ghost exchanges)
    if (c->dist && c->dist->stream2) MPH_HIP_OK(c, hipStreamSynchronize(c->dist->stream2));
    return MPH_OK;
}

int mph_particle_count(const MphCtx* c) { return c ? c->n_glob : -1; }
double mph_time(const MphCtx* c) { return c ? c->time : 0.0; }
const char* mph_last_error(const MphCtx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int mph_get_scalars(const MphCtx* c, double* out)
{
    if (!c || !out) return MPH_ERR_ARG;
    fill_scalars(c->h, c->cfg, out);
    return MPH_OK;
}

int mph_get(MphCtx* c, int field, void* out)
{
    if (!c || !out) return MPH_ERR_ARG;
    MPH_CK(ctx_flush(c));
    MPH_HIP_OK(c, hipSetDevice(c->device));
    double* o = (double*)out;
    int* oi = (int*)out;
    // structure rows: every list built here (single context), or the slots this rank computes
    // (slab mode: its owned elastic particles; the lists of ghost slots are partial)
    const int ns = c->dist ? (int)c->sl_s.size() : (int)c->S.orig.size();
    auto sidx = [c](int k) { return c->dist ? c->sl_s[k] : k; };
    // static inputs: every particle, or (slab-local creation) the ones this rank was created with
    const int nin = (int)c->prop.size();
    // sorted device arrays -> original order (download; in its callbacks h[k][i] is element i of
    // the k-th array given): get3 three component arrays into [id][3], get4 the xyz of a double4
    // array in A order into [id][3], get1 a scalar array in A order into out[id]
    const size_t n = (size_t)c->n;
    auto get3 = [&](double* x, double* y, double* z, const int* ids) {
        double* const src[3] = {x, y, z};
        return download(c, src, n, ids, [o](auto* h, size_t i, size_t id) {
            for (int k = 0; k < 3; ++k) o[3 * id + k] = h[k][i];
        });
    };
    auto get4 = [&](double4* d) {
        double4* const src[1] = {d};
        return download(c, src, n, c->L.A.id, [o](auto* h, size_t i, size_t id) {
            o[3 * id] = h[0][i].x; o[3 * id + 1] = h[0][i].y; o[3 * id + 2] = h[0][i].z;
        });
    };
    auto get1 = [&](auto* d, auto* out) {
        decltype(d) const src[1] = {d};   // (an array of one pointer to d's element type)
        return download(c, src, n, c->L.A.id, [out](auto* h, size_t i, size_t id) { out[id] = h[0][i]; });
    };
    switch (field) {
    case MPH_FIELD_POSITION: return get3(c->L.B.x, c->L.B.y, c->L.B.z, c->L.B.id);
    case MPH_FIELD_VELOCITY: return get3(c->L.B.vx, c->L.B.vy, c->L.B.vz, c->L.B.id);
    case MPH_FIELD_INITIAL_POSITION:
        for (int k = 0; k < nin; ++k) std::memcpy(o + 3 * (size_t)glob_id(c, k), &c->pos0[3 * (size_t)k], 3 * sizeof(double));
        return MPH_OK;
    case MPH_FIELD_FORCE: return get4(c->L.force);
    case MPH_FIELD_ACCELERATION: return get4(c->L.acc);
    case MPH_FIELD_GRAVITY_CENTER: return get3(c->L.gx, c->L.gy, c->L.gz, c->L.A.id);
    case MPH_FIELD_PRESSURE_P: return get1(c->L.pres, o);
    case MPH_FIELD_PRESSURE_A: return get1(c->L.pa, o);
    case MPH_FIELD_DENSITY_A: return get1(c->L.dens_a, o);
    case MPH_FIELD_VOL_STRAIN_P: return get1(c->L.vstrain, o);
    case MPH_FIELD_DIVERGENCE_P: return get1(c->L.divp, o);
    case MPH_FIELD_NEIGHBOR_COUNT: return get1(c->L.nbcount, oi);
    case MPH_FIELD_MASS:
        for (int k = 0; k < nin; ++k) o[glob_id(c, k)] = c->cfg.density[c->prop[k]] * c->h.vol;
        return MPH_OK;
    case MPH_FIELD_KAPPA: {
        // initializeFluid (1317-1319) before the first step, calculatePhysicalCoefficients after
        std::vector<double> vs(c->stepped ? (size_t)c->n_glob : 0, 0.0);
        if (c->stepped) MPH_CK(get1(c->L.vstrain, vs.data()));
        for (int k = 0; k < nin; ++k) {
            const int i = glob_id(c, k);
            o[i] = (c->stepped && vs[i] < 0.0) ? 0.0 : c->cfg.bulk_modulus[c->prop[k]];
        }
        return MPH_OK;
    }
    case MPH_FIELD_LAMBDA:
        for (int k = 0; k < nin; ++k) o[glob_id(c, k)] = c->cfg.bulk_viscosity[c->prop[k]];
        return MPH_OK;
    case MPH_FIELD_MU:
        for (int k = 0; k < nin; ++k) o[glob_id(c, k)] = c->cfg.shear_viscosity[c->prop[k]];
        return MPH_OK;
    case MPH_FIELD_PROPERTY:
        for (int k = 0; k < nin; ++k) oi[glob_id(c, k)] = c->prop[k];
        return MPH_OK;
    case MPH_FIELD_INITIAL_STRUCTURE_NEIGHBOR_COUNT:
        for (int k = 0; k < nin; ++k) oi[glob_id(c, k)] = 0;
        for (int k = 0; k < ns; ++k) oi[glob_id(c, c->S.orig[sidx(k)])] = c->S.count[sidx(k)];
        return MPH_OK;
    case MPH_FIELD_DEFORM_GRADIENT: return download_struct_m33(c, c->Sd.F, o);
    case MPH_FIELD_STRAIN: return download_struct_m33(c, c->Sd.E, o);
    case MPH_FIELD_STRESS: return download_struct_m33(c, c->Sd.S, o);
    case MPH_FIELD_NORMALIZER:
        for (int k = 0; k < nin; ++k) std::memset(o + (size_t)9 * glob_id(c, k), 0, sizeof(double) * 9);
        for (int k = 0; k < ns; ++k)
            std::memcpy(o + (size_t)9 * glob_id(c, c->S.orig[sidx(k)]), &c->S.normalizer[(size_t)9 * sidx(k)],
                        sizeof(double) * 9);
        return MPH_OK;
    case MPH_FIELD_VIRIAL_STRESS:
    case MPH_FIELD_VIRIAL_PRESSURE: {
        const size_t w = field == MPH_FIELD_VIRIAL_STRESS ? 9 : 1;
        std::memset(o, 0, sizeof(double) * w * (size_t)c->n_glob);
        if (!c->vir) return MPH_OK;   // never computed (the reference's array is uninitialised)
        double* const src[1] = {w == 9 ? c->vir : c->vpres};
        return download(c, src, w * n, c->L.A.id, [o, w](auto* h, size_t i, size_t id) {
            std::memcpy(o + w * id, &h[0][w * i], sizeof(double) * w);
        });
    }
    case MPH_FIELD_LAMBDA_LAMES:
    case MPH_FIELD_MU_LAMES:
        for (int k = 0; k < nin; ++k) o[glob_id(c, k)] = 0.0;
        for (int k = 0; k < ns; ++k)
            o[glob_id(c, c->S.orig[sidx(k)])] =
                field == MPH_FIELD_LAMBDA_LAMES ? c->S.lame_l[sidx(k)] : c->S.lame_m[sidx(k)];
        return MPH_OK;
    default: return ctx_fail(c, MPH_ERR_ARG, "unknown field " + std::to_string(field));
    }
}

int mph_compute_virial(MphCtx* c)
{
    if (!c) return MPH_ERR_ARG;
    MPH_CK(ctx_flush(c));
    MPH_HIP_OK(c, hipSetDevice(c->device));
    if (!c->vir) {
        // slab mode: the array capacity (c->P.n), the held count changes every step
        const size_t cap = (size_t)std::max(c->dist ? c->P.n : c->n, 1);
        MPH_CK(ctx_dalloc(c, &c->vir, 9 * cap));
        MPH_CK(ctx_dalloc(c, &c->vpres, cap));
    }
    if (c->dist) return dist_virial(c);
    // after a step the integrated state B is in A (list) order; before the first step A is current
    if (c->phase_timing) MPH_HIP_OK(c, hipEventRecord(c->ev_vir[0], c->stream));
    MPH_CK(virial_full_lists(c));
    launch_virial(c->L, c->stepped ? c->L.B : c->L.A, c->vir, c->vpres);
    MPH_HIP_OK(c, hipGetLastError());
    if (c->phase_timing) MPH_HIP_OK(c, hipEventRecord(c->ev_vir[1], c->stream));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    if (c->phase_timing) {
        float ms = 0.0f;
        MPH_HIP_OK(c, hipEventElapsedTime(&ms, c->ev_vir[0], c->ev_vir[1]));
        c->phase_ms[2] += ms;
    }
    return MPH_OK;
}

int mph_set(MphCtx* c, int field, const void* in)
{
    if (!c || !in) return MPH_ERR_ARG;
    MPH_CK(ctx_flush(c));
    if (field != MPH_FIELD_POSITION && field != MPH_FIELD_VELOCITY)
        return ctx_fail(c, MPH_ERR_ARG, "mph_set supports Position and Velocity");
    MPH_HIP_OK(c, hipSetDevice(c->device));
    c->a_current = false;   // the sorted set A is the last step's, no longer this state's (mph_sample_grid)
    const int n = c->n;
    const double* v = (const double*)in;
    // current state lives in the B set in the order of B.id: rewrite it in that order
    std::vector<double> h(n);
    std::vector<int> id(n);
    MPH_HIP_OK(c, hipMemcpy(id.data(), c->L.B.id, sizeof(int) * n, hipMemcpyDeviceToHost));
    double* dst[3] = {c->L.B.x, c->L.B.y, c->L.B.z};
    if (field == MPH_FIELD_VELOCITY) { dst[0] = c->L.B.vx; dst[1] = c->L.B.vy; dst[2] = c->L.B.vz; }
    for (int k = 0; k < 3; ++k) {
        for (int i = 0; i < n; ++i) h[i] = id[i] >= 0 ? v[3 * (size_t)id[i] + k] : 0.0;
        MPH_HIP_OK(c, hipMemcpy(dst[k], h.data(), sizeof(double) * n, hipMemcpyHostToDevice));
    }
    return MPH_OK;
}

int mph_set_initial_velocity_profile(MphCtx* c)
{
    if (!c) return MPH_ERR_ARG;
    MPH_CK(ctx_flush(c));
    MPH_HIP_OK(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->n_glob;
    // slab mode: mph_get fills the owned entries and mph_set writes only those back
    std::vector<double> pos(3 * n, 0.0), vel(3 * n, 0.0);
    MPH_CK(mph_get(c, MPH_FIELD_POSITION, pos.data()));
    MPH_CK(mph_get(c, MPH_FIELD_VELOCITY, vel.data()));
    // the static inputs this context holds, with the current state of the same particles
    const int nin = (int)c->prop.size();
    std::vector<double> p(3 * (size_t)nin), v(3 * (size_t)nin);
    for (int k = 0; k < nin; ++k)
        for (int d = 0; d < 3; ++d) {
            p[3 * (size_t)k + d] = pos[3 * (size_t)glob_id(c, k) + d];
            v[3 * (size_t)k + d] = vel[3 * (size_t)glob_id(c, k) + d];
        }
    MPH_CK(mph_velocity_profile_arrays(&c->cfg, c->time, nin, c->prop.data(), p.data(), c->pos0.data(), v.data()));
    for (int k = 0; k < nin; ++k)
        for (int d = 0; d < 3; ++d) vel[3 * (size_t)glob_id(c, k) + d] = v[3 * (size_t)k + d];
    return mph_set(c, MPH_FIELD_VELOCITY, vel.data());
}

int mph_write_prof(MphCtx* c, const char* path)
{
    if (!c || !path) return MPH_ERR_ARG;
    if (c->dist) return dist_write_output(c, path, kOutProf);   // collective; rank 0 writes
    const int n = c->n_glob;
    std::vector<double> pos(3 * (size_t)n), vel(3 * (size_t)n);
    MPH_CK(mph_get(c, MPH_FIELD_POSITION, pos.data()));
    MPH_CK(mph_get(c, MPH_FIELD_VELOCITY, vel.data()));
    return mph_write_prof_arrays(path, &c->cfg, c->time, n, c->prop.data(), pos.data(), c->pos0.data(),
                                 vel.data());
}

// the per-particle fields of a .vtk / .vtu file, in original order
struct Snap {
    std::vector<double> pos, vel, acc, force, stress, strain;
    std::vector<int> isnc, nc;
};

static int snapshot(MphCtx* c, Snap& s)
{
    const size_t n = (size_t)c->n_glob;
    for (auto* v : {&s.pos, &s.vel, &s.acc, &s.force}) v->resize(3 * n);
    s.stress.resize(9 * n); s.strain.resize(9 * n); s.isnc.resize(n); s.nc.resize(n);
    MPH_CK(mph_get(c, MPH_FIELD_POSITION, s.pos.data()));
    MPH_CK(mph_get(c, MPH_FIELD_VELOCITY, s.vel.data()));
    MPH_CK(mph_get(c, MPH_FIELD_ACCELERATION, s.acc.data()));
    MPH_CK(mph_get(c, MPH_FIELD_FORCE, s.force.data()));
    MPH_CK(mph_get(c, MPH_FIELD_STRESS, s.stress.data()));
    MPH_CK(mph_get(c, MPH_FIELD_STRAIN, s.strain.data()));
    MPH_CK(mph_get(c, MPH_FIELD_INITIAL_STRUCTURE_NEIGHBOR_COUNT, s.isnc.data()));
    return mph_get(c, MPH_FIELD_NEIGHBOR_COUNT, s.nc.data());
}

static int write_vtk_any(MphCtx* c, const char* path, bool xml)
{
    if (!c || !path) return MPH_ERR_ARG;
    if (c->dist) return dist_write_output(c, path, xml ? kOutVtu : kOutVtk);   // collective; rank 0 writes
    Snap s;
    MPH_CK(snapshot(c, s));
    auto writer = xml ? mph_write_vtu_arrays : mph_write_vtk_arrays;
    return writer(path, c->n_glob, c->prop.data(), s.pos.data(), c->pos0.data(), s.vel.data(), s.acc.data(),
                  s.force.data(), s.stress.data(), s.strain.data(), s.isnc.data(), s.nc.data());
}

int mph_write_vtk(MphCtx* c, const char* path) { return write_vtk_any(c, path, false); }

int mph_write_vtu(MphCtx* c, const char* path) { return write_vtk_any(c, path, true); }

int mph_output_wait(MphCtx* c)
{
    if (!c) return MPH_ERR_ARG;
    if (c->out_thread.joinable()) c->out_thread.join();
    const int rc = c->out_rc;
    c->out_rc = MPH_OK;
    if (rc) return ctx_fail(c, rc, "asynchronous .vtk write failed");
    return MPH_OK;
}

int mph_write_vtk_async(MphCtx* c, const char* path)
{
    if (!c || !path) return MPH_ERR_ARG;
    MPH_CK(mph_output_wait(c));   // at most one file in flight
    if (c->dist) return dist_write_output(c, path, kOutVtkAsync);   // collective; rank 0 formats and writes
    auto s = std::make_shared<Snap>();
    MPH_CK(snapshot(c, *s));
    // the thread owns copies of everything it reads
    c->out_thread = std::thread([c, s, nn = c->n_glob, file = std::string(path), prop = c->prop, pos0 = c->pos0] {
        c->out_rc = mph_write_vtk_arrays(file.c_str(), nn, prop.data(), s->pos.data(), pos0.data(), s->vel.data(),
                                         s->acc.data(), s->force.data(), s->stress.data(), s->strain.data(),
                                         s->isnc.data(), s->nc.data());
    });
    return MPH_OK;
}

int mph_phase_timing(MphCtx* c, int on)
{
    if (!c) return MPH_ERR_ARG;
    MPH_CK(ctx_flush(c));
    if (c->dist) return on ? ctx_fail(c, MPH_ERR_ARG, "phase timing is not available in slab mode") : MPH_OK;
    MPH_HIP_OK(c, hipSetDevice(c->device));
    const bool want = on != 0;
    if (want == c->phase_timing) return MPH_OK;
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    c->phase_timing = want;   // (mph_step then launches directly; the graphs stay for later)
    if (want && c->ev_vir.empty()) {
        c->ev_vir.assign(2, nullptr);
        for (auto& e : c->ev_vir) MPH_HIP_OK(c, hipEventCreate(&e));
        c->ev8.assign(3 * 8, nullptr);
        for (auto& e : c->ev8) MPH_HIP_OK(c, hipEventCreate(&e));
    }
    return MPH_OK;
}

int mph_phase_times(const MphCtx* c, double* out3)
{
    if (!c || !out3) return MPH_ERR_ARG;
    for (int k = 0; k < 3; ++k) out3[k] = c->phase_ms[k];
    return MPH_OK;
}

int mph_profile_steps(MphCtx* c, int nsteps, double* avg_ms, int* launches, char* names32)
{
    if (!c || nsteps <= 0 || !avg_ms || !launches || !names32) return MPH_ERR_ARG;
    MPH_CK(ctx_flush(c));
    MPH_HIP_OK(c, hipSetDevice(c->device));
    EventProfiler prof;
    if (c->dist) {
        MPH_CK(dist_step(c, nsteps, &prof));
    } else {
        Launch L = c->L;
        L.prof = &prof;
        for (int k = 0; k < nsteps; ++k) enqueue_step(L, k == nsteps - 1);
        MPH_HIP_OK(c, hipGetLastError());
        MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
        for (int k = 0; k < nsteps; ++k) c->time += c->cfg.dt;
        c->stepped = true;
        c->a_current = true;
    }
    std::vector<std::string> order;
    std::map<std::string, std::pair<double, int>> acc;
    // the kernels' intervals from the first event on, for their union (kernels of the two streams
    // of a slab step run concurrently, so the sum of their times overstates the GPU time)
    std::vector<std::pair<float, float>> span;
    for (auto& r : prof.recs) {
        float ms = 0.0f, t0 = 0.0f;
        MPH_HIP_OK(c, hipEventElapsedTime(&ms, r.a, r.b));
        MPH_HIP_OK(c, hipEventElapsedTime(&t0, prof.recs[0].a, r.a));
        if (r.floor >= 0) {
            float tf = 0.0f;
            MPH_HIP_OK(c, hipEventElapsedTime(&tf, prof.recs[0].a, prof.floors[r.floor]));
            if (tf > t0) {
                ms = std::max(0.0f, ms - (tf - t0));
                t0 = tf;
            }
        }
        span.emplace_back(t0, t0 + ms);
        if (!acc.count(r.name)) order.push_back(r.name);
        acc[r.name].first += ms;
        acc[r.name].second += 1;
    }
    std::sort(span.begin(), span.end());
    double busy = 0.0, hi = -1e30;
    for (auto& iv : span) {
        if (iv.first > hi) { busy += iv.second - iv.first; hi = iv.second; }
        else if (iv.second > hi) { busy += iv.second - hi; hi = iv.second; }
    }
    int k = 0;
    for (auto& name : order) {
        if (k >= MPH_PROFILE_MAX - 1) break;
        avg_ms[k] = acc[name].first / acc[name].second;
        launches[k] = acc[name].second;
        std::snprintf(names32 + 32 * k, 32, "%s", name.c_str());
        ++k;
    }
    // last entry: "gpu_busy", the union of the kernel intervals per step (launches = steps)
    avg_ms[k] = busy / nsteps;
    launches[k] = nsteps;
    std::snprintf(names32 + 32 * k, 32, "%s", "gpu_busy");
    ++k;
    DevState hs;
    MPH_HIP_OK(c, hipMemcpy(&hs, c->L.st, kStateHead, hipMemcpyDeviceToHost));
    MPH_CK(ctx_state_status(c, hs));
    return k;
}

// The list kernels as the timed steps run them: each one captured `reps` times into a graph of
// its own (the output-only stores on every 8th, as in the 8-step graph), replayed once to warm,
// then once between two HIP events.  Each replay recomputes what the last step left (the lists,
// pass A's products, B from A), bit for bit, so the state does not change; pass B is skipped with
// elastic slots (the substeps after it have moved them in B).  Slab contexts: the same on the
// rank's local set, pass B as its single launch and before pass A (whose replay clears the
// ghosts' halo pressure in the pass-B records until the next step's halo).  Needs one step done.
int mph_profile_graphs(MphCtx* c, int reps, double* avg_ms3)
{
    if (!c || reps <= 0 || reps > 64 || !avg_ms3) return MPH_ERR_ARG;
    MPH_CK(ctx_flush(c));
    if (!c->stepped) return ctx_fail(c, MPH_ERR_ARG, "mph_profile_graphs: run a step first");
    MPH_HIP_OK(c, hipSetDevice(c->device));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    MPH_HIP_OK(c, hipEventCreate(&e0));
    MPH_HIP_OK(c, hipEventCreate(&e1));
    int rc = MPH_OK;
    for (int k = 0; k < 3; ++k) avg_ms3[k] = -1.0;
    // pass B before pass A: in slab mode pass A zeroes the pressure of the ghosts' pass-B records,
    // which the halo had filled (the next step's halo fills them again)
    for (int kk = 0; kk < 3 && rc == MPH_OK; ++kk) {
        const int k = kk == 0 ? 0 : (kk == 1 ? 2 : 1);
        if (k == 2 && c->P.n_struct > 0) continue;
        hipGraph_t g = nullptr;
        hipGraphExec_t ge = nullptr;
        bool ok = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
        if (ok) {
            for (int r = 0; r < reps; ++r) {
                const bool last = r % 8 == 7 || r == reps - 1;
                Launch La = c->L;
                if (c->dist) La.wface = c->dist->wface;   // slab mode: pass B in one launch (phase 0)
                if (!last) {
                    La.dens_a = La.vstrain = La.divp = nullptr;
                    if (!c->P.surface) La.gx = La.gy = La.gz = La.pa = nullptr;
                    La.force = La.acc = nullptr;
                }
                if (k == 0) launch_neighbors(La);
                else if (k == 1) launch_pass_a(La);
                else launch_pass_b(La);
            }
            ok = hipStreamEndCapture(c->stream, &g) == hipSuccess && g;
        }
        ok = ok && hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) == hipSuccess;
        if (g) (void)hipGraphDestroy(g);
        float ms = 0.0f;
        ok = ok && hipGraphUpload(ge, c->stream) == hipSuccess && hipGraphLaunch(ge, c->stream) == hipSuccess &&
             hipEventRecord(e0, c->stream) == hipSuccess && hipGraphLaunch(ge, c->stream) == hipSuccess &&
             hipEventRecord(e1, c->stream) == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
             hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
        if (ge) (void)hipGraphExecDestroy(ge);
        if (ok) avg_ms3[k] = ms / reps;
        else rc = ctx_fail(c, MPH_ERR_HIP, "mph_profile_graphs: graph capture or replay failed");
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    MPH_CK(rc);
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    DevState hs;
    MPH_HIP_OK(c, hipMemcpy(&hs, c->L.st, kStateHead, hipMemcpyDeviceToHost));
    return ctx_state_status(c, hs);
}

static void mean_max(const std::vector<int>& h, double* mean, int* mx)
{
    long long sum = 0;
    *mx = 0;
    for (int v : h) { sum += v; *mx = v > *mx ? v : *mx; }
    *mean = h.empty() ? 0.0 : (double)sum / h.size();
}

int mph_neighbor_stats(MphCtx* c, double* mean, int* mx)
{
    if (!c || !mean || !mx) return MPH_ERR_ARG;
    MPH_CK(ctx_flush(c));
    MPH_HIP_OK(c, hipSetDevice(c->device));
    // NeighborCount of the particles held here (slab mode: owned + ghosts), reduced on the host
    std::vector<int> h(c->n);
    if (c->n) MPH_HIP_OK(c, hipMemcpy(h.data(), c->L.nbcount, sizeof(int) * c->n, hipMemcpyDeviceToHost));
    mean_max(h, mean, mx);
    return MPH_OK;
}

// the last search's rows and row jumps (mph_rows.h), copied from the device
static int host_rows(MphCtx* c, HostRows& R)
{
    const int n = c->n;
    const size_t ntile = ((size_t)n + kTile - 1) / kTile;
    R.rows.resize(n);
    R.hdr.resize(ntile);
    R.gap.resize(ntile * kTile);
    if (!n) return MPH_OK;
    MPH_HIP_OK(c, hipMemcpy(R.rows.data(), c->L.ncount, sizeof(int) * n, hipMemcpyDeviceToHost));
    MPH_HIP_OK(c, hipMemcpy(R.hdr.data(), c->L.lhdr, sizeof(R.hdr[0]) * ntile, hipMemcpyDeviceToHost));
    MPH_HIP_OK(c, hipMemcpy(R.gap.data(), c->L.lgap, sizeof(R.gap[0]) * n, hipMemcpyDeviceToHost));
    return MPH_OK;
}

int mph_list_stats(MphCtx* c, double* mean, int* mx)
{
    if (!c || !mean || !mx) return MPH_ERR_ARG;
    MPH_CK(ctx_flush(c));
    MPH_HIP_OK(c, hipSetDevice(c->device));
    HostRows R;   // stored list lengths (the rows outside the gaps), reduced on the host
    MPH_CK(host_rows(c, R));
    std::vector<int> h(c->n);
    for (int s = 0; s < c->n; ++s) h[s] = R.entries(s);
    mean_max(h, mean, mx);
    return MPH_OK;
}

int mph_list_layout(MphCtx* c, long long out[6])
{
    if (!c || !out) return MPH_ERR_ARG;
    MPH_CK(ctx_flush(c));
    if (c->dist) return ctx_fail(c, MPH_ERR_UNSUPPORTED, "mph_list_layout: single contexts only");
    MPH_HIP_OK(c, hipSetDevice(c->device));
    HostRows R;   // the last search's rows and row jumps, reduced on the host
    MPH_CK(host_rows(c, R));
    const int n = c->n;
    const long long waves = ((long long)n + kTile - 1) / kTile;
    long long jumped = 0, jumps = 0, max_jumps = 0, gap_rows = 0, max_rows = 0;
    for (long long t = 0; t < waves; ++t) {
        const int J = jump_count(R.hdr[t]);
        jumped += J > 0;
        jumps += J;
        max_jumps = std::max<long long>(max_jumps, J);
    }
    for (int s = 0; s < n; ++s) {
        const int rows = std::min(R.rows[s], kTileRows);
        gap_rows += rows - R.entries(s);
        max_rows = std::max<long long>(max_rows, rows);
    }
    out[0] = waves; out[1] = jumped; out[2] = jumps; out[3] = max_jumps; out[4] = gap_rows; out[5] = max_rows;
    return MPH_OK;
}

int mph_idle_wall_stats(MphCtx* c, long long out[2])
{
    if (!c || !out) return MPH_ERR_ARG;
    MPH_CK(ctx_flush(c));
    MPH_HIP_OK(c, hipSetDevice(c->device));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    // the tail of DevState: the lazy steps, then the idle waves per run of the waves
    unsigned long long steps = 0;
    std::vector<unsigned> seg(kXcdSegs);
    const char* st = reinterpret_cast<const char*>(c->L.st);
    MPH_HIP_OK(c, hipMemcpy(&steps, st + offsetof(DevState, lazy_steps), sizeof(steps), hipMemcpyDeviceToHost));
    MPH_HIP_OK(c, hipMemcpy(seg.data(), st + offsetof(DevState, idle_waves), sizeof(unsigned) * kXcdSegs,
                            hipMemcpyDeviceToHost));
    long long idle = 0;
    for (unsigned v : seg) idle += v;
    out[0] = idle;
    out[1] = (long long)steps;
    return MPH_OK;
}

int mph_lean_step_stats(MphCtx* c, long long out[2])
{
    if (!c || !out) return MPH_ERR_ARG;
    MPH_CK(ctx_flush(c));
    MPH_HIP_OK(c, hipSetDevice(c->device));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    unsigned long long steps[2] = {0, 0};   // lean_search_steps, lean_pass_a_steps
    static_assert(offsetof(DevState, lean_pass_a_steps) == offsetof(DevState, lean_search_steps) + sizeof(steps[0]),
                  "the two counters are read in one copy");
    MPH_HIP_OK(c, hipMemcpy(steps, reinterpret_cast<const char*>(c->L.st) + offsetof(DevState, lean_search_steps),
                            sizeof(steps), hipMemcpyDeviceToHost));
    out[0] = (long long)steps[0];
    out[1] = (long long)steps[1];
    return MPH_OK;
}

int mph_neighbor_rows(MphCtx* c, int first, int count, int* counts, int* ids, long long ids_cap)
{
    if (!c || first < 0 || count < 0 || !counts || (!ids && ids_cap > 0)) return MPH_ERR_ARG;
    MPH_CK(ctx_flush(c));
    if (c->dist) return ctx_fail(c, MPH_ERR_UNSUPPORTED, "mph_neighbor_rows: single contexts only");
    if ((long long)first + count > c->n) return ctx_fail(c, MPH_ERR_ARG, "mph_neighbor_rows: range past the particle count");
    if (!count) return 0;
    MPH_HIP_OK(c, hipSetDevice(c->device));
    const int n = c->n;
    if (c->P.rlf < 3.0e38f)
        return ctx_fail(c, MPH_ERR_UNSUPPORTED, "mph_neighbor_rows: the lists keep only the pairs within the passes' "
                                            "radius (create the context with MPH_LIST_FULL=1 for the reference's lists)");
    // the last search's rows are in its sorted order A: A.id maps a row (and an entry) back to the
    // original index, ncount holds the list's length and nbcount NeighborCount in the same order
    std::vector<int> id(n), nv(n);
    MPH_HIP_OK(c, hipMemcpy(id.data(), c->L.A.id, sizeof(int) * n, hipMemcpyDeviceToHost));
    MPH_HIP_OK(c, hipMemcpy(nv.data(), c->L.nbcount, sizeof(int) * n, hipMemcpyDeviceToHost));
    HostRows R;
    MPH_CK(host_rows(c, R));
    const std::vector<int>& nc = R.rows;
    std::vector<int> row_of(count, -1);
    for (int s = 0; s < n; ++s)
        if (id[s] >= first && id[s] < first + count) row_of[id[s] - first] = s;
    long long total = 0;
    for (int k = 0; k < count; ++k) {
        if (row_of[k] < 0) return ctx_fail(c, MPH_ERR_HIP, "mph_neighbor_rows: particle missing from the sorted set");
        counts[k] = nv[row_of[k]];
        total += std::min(counts[k], kMaxNeighbor);
    }
    if (total > ids_cap) return ctx_fail(c, MPH_ERR_ARG, "mph_neighbor_rows: ids_cap too small (" + std::to_string(total) + " needed)");
    // every ELL tile holding a requested row, down to the longest row of its lanes (entry k of lane l
    // at [k][l], 64 ints per entry: one contiguous copy per tile)
    std::map<int, std::vector<int>> tiles;
    for (int k = 0; k < count; ++k) {
        const int t = row_of[k] >> 6;
        if (tiles.count(t)) continue;
        int m = 0;
        for (int s = t * kTile; s < std::min(n, (t + 1) * kTile); ++s) m = std::max(m, std::min(nc[s], kTileRows));
        std::vector<int>& buf = tiles[t];
        buf.resize((size_t)m * kTile);
        if (m) MPH_HIP_OK(c, hipMemcpy(buf.data(), c->L.nbr + (size_t)t * kTileStride, sizeof(int) * buf.size(),
                                   hipMemcpyDeviceToHost));
    }
    long long w = 0;
    for (int k = 0; k < count; ++k) {
        const int s = row_of[k], m = std::min(counts[k], kMaxNeighbor), rows = std::min(nc[s], kTileRows);
        const std::vector<int>& buf = tiles[s >> 6];
        int q = 0;
        for (int e = 0; e < rows; ++e) {
            if (!R.ok(s, e)) continue;   // a gap of the row jumps
            const int v = buf[(size_t)ell_slot(e, s & 63)];
            const int j = v & kIndexMask;
            if (j >= n || q >= m) return ctx_fail(c, MPH_ERR_HIP, "mph_neighbor_rows: list entry past the particle count");
            ids[w + q++] = id[j];
        }
        if (q != m) return ctx_fail(c, MPH_ERR_HIP, "mph_neighbor_rows: list rows disagree with NeighborCount");
        std::sort(ids + w, ids + w + m);
        w += m;
    }
    return (int)std::min<long long>(w, 0x7fffffff);
}

// ---- per-step monitors (kernels: mph_monitor.hip) ----------------------------------------------

int mph_monitor_configure(MphCtx* c, const MphMonitorConfig* m)
{
    if (!c) return MPH_ERR_ARG;
    MPH_CK(ctx_flush(c));
    if (c->dist)
        return ctx_fail(c, MPH_ERR_UNSUPPORTED, "monitors are not available in slab mode (no cross-rank reduction yet)");
    MPH_HIP_OK(c, hipSetDevice(c->device));
    if (!m) {
        if (c->mon_on) MPH_CK(drop_graphs(c));
        c->mon_on = false;
        c->L.mon = nullptr;
        return MPH_OK;
    }
    if (m->stride < 1 || m->capacity < 1) return ctx_fail(c, MPH_ERR_ARG, "monitors: stride and capacity must be >= 1");
    if (m->ntrack < 0 || m->ntrack > MPH_MONITOR_MAX_TRACK || (m->ntrack > 0 && !m->track))
        return ctx_fail(c, MPH_ERR_ARG, "monitors: 0.." + std::to_string(MPH_MONITOR_MAX_TRACK) + " tracked particles");
    if (m->nprobe < 0 || m->nprobe > MPH_MONITOR_MAX_PROBES || (m->nprobe > 0 && !m->probes))
        return ctx_fail(c, MPH_ERR_ARG, "monitors: 0.." + std::to_string(MPH_MONITOR_MAX_PROBES) + " probes");
    for (int k = 0; k < m->ntrack; ++k)
        if (m->track[k] < 0 || m->track[k] >= c->n_glob)
            return ctx_fail(c, MPH_ERR_ARG, "monitors: tracked index " + std::to_string(m->track[k]) + " outside [0, n)");
    const double reach = c->h.max_radius + 0.1 * c->h.dx;   // MaxRadius + MARGIN (make_dev_params)
    if (!(m->probe_radius >= 0.0) || m->probe_radius > reach)
        return ctx_fail(c, MPH_ERR_ARG, "monitors: probe radius outside [0, MaxRadius + MARGIN = " + std::to_string(reach) + "]");
    MPH_CK(drop_graphs(c));
    MonitorDev& D = c->mon;
    if (!D.counters) {   // once, for the maxima
        MPH_CK(ctx_dalloc(c, &D.counters, 2));
        MPH_CK(ctx_dalloc(c, &D.partial, (size_t)kMonPartial * monitor_blocks(c->n)));
        MPH_CK(ctx_dalloc(c, &D.trk, 6 * (size_t)MPH_MONITOR_MAX_TRACK));
        MPH_CK(ctx_dalloc(c, &D.prb, 2 * (size_t)MPH_MONITOR_MAX_PROBES));
        MPH_CK(ctx_dalloc(c, &c->mon_sorted, MPH_MONITOR_MAX_TRACK));
        MPH_CK(ctx_dalloc(c, &c->mon_map, MPH_MONITOR_MAX_TRACK));
        MPH_CK(ctx_dalloc(c, &c->mon_probes, 3 * (size_t)MPH_MONITOR_MAX_PROBES));
        D.track_sorted = c->mon_sorted;
        D.track_map = c->mon_map;
        D.probes = c->mon_probes;
    }
    const int width = MPH_MONITOR_HEAD + 6 * m->ntrack + 2 * m->nprobe;
    const size_t need = (size_t)m->capacity * width;
    if (need > c->mon_ring_cap) {
        ctx_dfree(c, D.ring);
        D.ring = nullptr;
        c->mon_ring_cap = 0;
        MPH_CK(ctx_dalloc(c, &D.ring, need));
        c->mon_ring_cap = need;
    }
    // the distinct tracked ids ascending (the kernel's search), and each entry's row among them
    std::vector<int> sorted(m->track, m->track + m->ntrack);
    std::sort(sorted.begin(), sorted.end());
    sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
    std::vector<int> map(MPH_MONITOR_MAX_TRACK, 0);
    for (int k = 0; k < m->ntrack; ++k)
        map[k] = (int)(std::lower_bound(sorted.begin(), sorted.end(), m->track[k]) - sorted.begin());
    sorted.resize(MPH_MONITOR_MAX_TRACK, 0x7fffffff);
    std::vector<double> probes(3 * (size_t)MPH_MONITOR_MAX_PROBES, 0.0);
    std::copy(m->probes, m->probes + 3 * (size_t)m->nprobe, probes.begin());
    MPH_HIP_OK(c, hipMemcpy(c->mon_sorted, sorted.data(), sizeof(int) * sorted.size(), hipMemcpyHostToDevice));
    MPH_HIP_OK(c, hipMemcpy(c->mon_map, map.data(), sizeof(int) * map.size(), hipMemcpyHostToDevice));
    MPH_HIP_OK(c, hipMemcpy(c->mon_probes, probes.data(), sizeof(double) * probes.size(), hipMemcpyHostToDevice));
    MPH_HIP_OK(c, hipMemset(D.counters, 0, 2 * sizeof(long long)));
    MPH_HIP_OK(c, hipMemset(D.trk, 0, sizeof(double) * 6 * MPH_MONITOR_MAX_TRACK));
    MPH_HIP_OK(c, hipMemset(D.prb, 0, sizeof(double) * 2 * MPH_MONITOR_MAX_PROBES));
    D.stride = m->stride;
    D.capacity = m->capacity;
    D.ntrack = m->ntrack;
    D.nprobe = m->nprobe;
    D.width = width;
    D.probe_h = m->probe_radius > 0.0 ? m->probe_radius : c->h.rp;
    c->mon_read = 0;
    c->mon_on = true;
    c->L.mon = &c->mon;
    return MPH_OK;
}

int mph_monitor_sample_doubles(const MphCtx* c) { return c && c->mon_on ? c->mon.width : 0; }

long long mph_monitor_read(MphCtx* c, double* out, long long max_samples, long long* lost)
{
    if (!c || max_samples < 0 || (max_samples > 0 && !out)) return MPH_ERR_ARG;
    if (lost) *lost = 0;
    MPH_CK(ctx_flush(c));
    if (!c->mon_on) return 0;
    MPH_HIP_OK(c, hipSetDevice(c->device));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    const MonitorDev& D = c->mon;
    long long cnt[2] = {0, 0};
    MPH_HIP_OK(c, hipMemcpy(cnt, D.counters, sizeof(cnt), hipMemcpyDeviceToHost));
    const long long unread = cnt[1] - c->mon_read;
    const long long avail = std::min<long long>(unread, D.capacity);
    if (lost) *lost = unread - avail;
    const long long first = cnt[1] - avail, k = std::min(avail, max_samples);
    // samples first .. first + k - 1, sample i in ring slot i mod capacity: at most two runs
    for (long long i = first; i < first + k;) {
        const long long slot = i % D.capacity;
        const long long run = std::min<long long>(first + k - i, D.capacity - slot);
        MPH_HIP_OK(c, hipMemcpy(out + (size_t)(i - first) * D.width, D.ring + (size_t)slot * D.width,
                                sizeof(double) * (size_t)run * D.width, hipMemcpyDeviceToHost));
        i += run;
    }
    c->mon_read = first + k;
    return k;
}

// ---- lattice sampling (kernel: mph_sample.hip) --------------------------------------------------

// prof set: the kernel's launch is recorded by it (its events are read by the caller)
static int sample_grid(MphCtx* c, const MphSampleGrid* g, double* out, Profiler* prof)
{
    if (!c || !g || !out) return MPH_ERR_ARG;
    MPH_CK(ctx_flush(c));
    if (c->dist)
        return ctx_fail(c, MPH_ERR_UNSUPPORTED, "sampling is not available in slab mode (a lattice spans the ranks)");
    long long points = 1;
    for (int d = 0; d < 3; ++d) {
        if (g->count[d] < 1 || !(g->spacing[d] > 0.0) || !std::isfinite(g->spacing[d]) || !std::isfinite(g->origin[d]))
            return ctx_fail(c, MPH_ERR_ARG, "sample grid: counts must be >= 1, spacings > 0 and the origin finite");
        points *= g->count[d];   // (at most 2^24 before each factor below 2^31)
        if (points > MPH_SAMPLE_MAX_POINTS)
            return ctx_fail(c, MPH_ERR_ARG, "sample grid: more than MPH_SAMPLE_MAX_POINTS = " +
                                                std::to_string(MPH_SAMPLE_MAX_POINTS) + " points");
    }
    if (c->cfg.dim == 2 && g->count[2] != 1) return ctx_fail(c, MPH_ERR_ARG, "sample grid: count[2] must be 1 in 2-D");
    if (g->classes < 0 || g->classes > 7) return ctx_fail(c, MPH_ERR_ARG, "sample grid: class mask outside 0..7");
    const double reach = c->h.max_radius + 0.1 * c->h.dx;   // MaxRadius + MARGIN (make_dev_params)
    if (!(g->radius >= 0.0) || g->radius > reach)
        return ctx_fail(c, MPH_ERR_ARG, "sample grid: radius outside [0, MaxRadius + MARGIN = " + std::to_string(reach) + "]");
    const size_t need = (size_t)points * MPH_SAMPLE_CHANNELS;
    if (c->n == 0) {
        std::memset(out, 0, sizeof(double) * need);
        return MPH_OK;
    }
    if (!c->a_current)
        return ctx_fail(c, MPH_ERR_ARG, "sample grid: run a step first (none since creation or since the last mph_set)");
    MPH_HIP_OK(c, hipSetDevice(c->device));
    if (need > c->sample_cap) {
        MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
        ctx_dfree(c, c->sample_out);
        c->sample_out = nullptr;
        c->sample_cap = 0;
        MPH_CK(ctx_dalloc(c, &c->sample_out, need));
        c->sample_cap = need;
    }
    SampleDev G{};
    for (int d = 0; d < 3; ++d) {
        G.origin[d] = g->origin[d];
        G.spacing[d] = g->spacing[d];
        G.count[d] = g->count[d];
    }
    G.mask = g->classes ? g->classes : 1;
    G.h = g->radius > 0.0 ? g->radius : c->h.rp;
    if (sample_tiling(G, contig_axis(c->P.dim, c->P.perm)) > 0x7fffffffLL) return ctx_fail(c, MPH_ERR_ARG, "sample grid: too many tiles");
    Launch L = c->L;
    L.prof = prof;
    launch_sample_grid(L, G, c->sample_out);
    MPH_HIP_OK(c, hipGetLastError());
    MPH_HIP_OK(c, hipMemcpyAsync(out, c->sample_out, sizeof(double) * need, hipMemcpyDeviceToHost, c->stream));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    return MPH_OK;
}

int mph_sample_grid(MphCtx* c, const MphSampleGrid* g, double* out) { return sample_grid(c, g, out, nullptr); }

int mph_sample_grid_timed(MphCtx* c, const MphSampleGrid* g, double* out, double* kernel_ms, char* name32)
{
    EventProfiler prof;
    if (kernel_ms) *kernel_ms = 0.0;
    if (name32) name32[0] = 0;
    MPH_CK(sample_grid(c, g, out, &prof));
    if (prof.recs.empty()) return MPH_OK;
    float ms = 0.0f;
    MPH_HIP_OK(c, hipEventElapsedTime(&ms, prof.recs[0].a, prof.recs[0].b));
    if (kernel_ms) *kernel_ms = ms;
    if (name32) std::snprintf(name32, 32, "%s", prof.recs[0].name.c_str());
    return MPH_OK;
}

void mph_destroy(MphCtx* c)
{
    if (!c) return;
    if (c->out_thread.joinable()) c->out_thread.join();
    (void)hipSetDevice(c->device);
    (void)ctx_flush(c);   // steps accepted under batching still run (their errors are dropped)
    if (c->hs_pin) (void)hipHostFree(c->hs_pin);
    if (c->ev_status) (void)hipEventDestroy(c->ev_status);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->graph1) (void)hipGraphExecDestroy(c->graph1);
    if (c->graph1t) (void)hipGraphExecDestroy(c->graph1t);
    if (c->graph8) (void)hipGraphExecDestroy(c->graph8);
    for (auto* v : {&c->ev8, &c->ev_vir})
        for (hipEvent_t e : *v) (void)hipEventDestroy(e);
    if (c->dist) dist_free(c);
    for (void* p : c->allocs) (void)hipFree(p);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

}  // extern "C"

// ---- multi-GPU slab decomposition: see mph_dist.hip ------------------------------------------
