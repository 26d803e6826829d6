// mph_ctx.h -- the device context behind the C ABI (include/mph_gpu.h) and what its host units share:
// mph_ctx.hip (errors, allocation, the helpers below, destroy), mph_create.hip (the create phases),
// mph_step.hip (the step sequencer: graphs, batching, phase timing), mph_fields.hip (download, upload,
// virial, writers, selections, kinematics), mph_profile.hip (per-kernel profilers, list and counter diagnostics),
// mph_observe.hip (host half of the monitors and of the lattice sampling), and the slab-decomposed
// multi-GPU step (mph_dist.h and its units).
#pragma once

#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <thread>
#include <vector>

#include "mph_internal.h"
#include "mph_kernels.h"

struct MphDist;   // the slab decomposition's state of one rank (mph_dist.h)

struct MphCtx {
    int device = 0;
    int n = 0;                   // particles held on the device (single GPU: all; slab: owned+ghosts)
    int n_glob = 0;              // particles of the whole problem (length of mph_get arrays)
    MphConfig cfg{};
    mph::HostDerived h{};
    mph::DevParams P{};
    mph::DevTables tables{};     // host copy of the per-type tables (uploaded to L.T at creation)
    std::string err;
    std::thread out_thread;      // mph_write_vtk_async: the file of the previous output step
    int out_rc = 0;
    double time = 0.0;           // host mirror of Time (same additions as the device)
    bool stepped = false;
    hipStream_t stream = nullptr;
    // the step graphs by kind (mph_kernels.h kSeqs).  The two without the output-only stores belong
    // to a single context alone, and kSeq8t -- every whole batch of a call but its last
    // (replay_plan) -- only where lean_calls (MPH_LEAN_CALLS not 0 at creation: ctx_fill_launch)
    hipGraphExec_t graph[mph::kSeqKinds] = {};
    bool lean_calls = false;
    // step batching (mph_set_step_batching): single mph_step calls accumulate into 8-step graphs;
    // `pending` steps are accepted but not launched yet, `unchecked`: batches launched whose error
    // flags have not been read (ev_status: their copy has landed)
    bool batch_steps = false;
    int pending = 0;
    bool unchecked = false;
    void* hs_pin = nullptr;      // pinned: where every status read lands (ctx_status_enqueue)
    hipEvent_t ev_status = nullptr;
    // phase timing (mph_phase_timing): steps launched directly (no graph) with events at every
    // step's phase boundaries -- before the sort, after the search, after the elastic substeps --
    // three per step of a batch of up to 8 (ev8), and around the virial (ev_vir)
    bool phase_timing = false;
    std::vector<hipEvent_t> ev8, ev_vir;
    double phase_ms[3] = {0.0, 0.0, 0.0};   // neighbour search, explicit calculation, virial
    // host copies of the static inputs: original order, or -- slab-local creation -- the
    // particles this rank was created with, whose original indices are gid (ascending)
    std::vector<int> prop;
    std::vector<double> pos0;
    std::vector<int> gid;
    mph::StructureInit S;
    std::vector<int> sl_orig;    // local structure slot -> original particle index
    std::vector<int> sl_s;       // local structure slot -> index into S (the lists built here)
    // device: the arrays every launch sequence uses live in L (mph_kernels.h Launch), allocated at
    // creation; what only this layer touches is here
    int* order = nullptr;        // cap ints: the slab sort's dst_of, scratch of the structure init
    double *vir = nullptr, *vpres = nullptr;   // VirialStress [cap][9] / VirialPressure (A order), lazy
    mph::StructDev Sd;
    std::vector<void*> allocs;
    mph::Launch L;
    // monitors (mph_monitor_configure): the kernels' arguments (L.mon points here while they are
    // on), the device buffers behind them (allocated once, the ring regrown when too small) and
    // how many samples the host has read
    bool mon_on = false;
    mph::MonitorDev mon;
    size_t mon_ring_cap = 0;     // doubles the ring allocation holds
    int *mon_sorted = nullptr, *mon_map = nullptr;
    double* mon_probes = nullptr;
    double* mon_gauges = nullptr;   // the gauge points (mph_gauge_configure), allocated at its first call
    long long mon_read = 0;
    // slab monitors (mph_dist_monitor_configure): a slab rank's records through the same arguments,
    // buffers and read count (mon_on stays false: the single-context calls go on refusing a slab
    // context)
    bool dmon_on = false;
    // lattice sampling and the elevation map (mph_sample_grid, mph_gauge_grid): the device result buffer (allocated at the first call,
    // regrown when a larger lattice arrives) and whether the sorted set A and pres are the current
    // state's -- a step has run since creation and no mph_set since
    double* sample_out = nullptr;
    size_t sample_cap = 0;       // doubles the allocation holds
    bool a_current = false;
    // the selection (mph_select, mph_select.hip): the kernels' buffers (allocated at the first
    // mph_select, regrown when a larger selection or result arrives), the host copy of the selected
    // ids, and whether the selection is the current state's -- made since the last step or mph_set
    mph::SelectDev sel;
    size_t sel_rank_cap = 0;     // ranks sel.ids / slot_a / slot_b hold
    double* sel_out = nullptr;   // a gathered field; the totals' partial records behind kSelTotals doubles
    size_t sel_out_cap = 0;      // doubles it holds
    std::vector<int> sel_ids;
    bool sel_current = false;
    // kinematics (mph_compute_kinematics, mph_kinematics.hip): the records [n][MPH_KIN_CHANNELS] in A
    // order (allocated at the first call, like vir), whether they are the current state's -- computed
    // since the last step or mph_set -- and whether an mph_set has changed the state since the last
    // step or the creation (the lists and the sorted set are then not that state's)
    double* kin = nullptr;
    bool kin_current = false;
    bool set_since_step = false;
    bool lazy_walls = false;     // lazy wall steps on (ctx_fill_launch; L.cmap allocated at creation)
    MphDist* dist = nullptr;     // non-null in slab mode
};

#define MPH_HIP_OK(ctx, expr)                                                \
    do {                                                                     \
        hipError_t _e = (expr);                                              \
        if (_e != hipSuccess) return mph::ctx_hip_fail(ctx, _e, #expr);      \
    } while (0)

#define MPH_CK(expr)                   \
    do {                               \
        int _r = (expr);               \
        if (_r != MPH_OK) return _r;   \
    } while (0)

namespace mph {

int ctx_fail(MphCtx* c, int code, const std::string& msg);
int ctx_hip_fail(MphCtx* c, hipError_t e, const char* what);
void* ctx_alloc(MphCtx* c, size_t bytes, int* status);
void ctx_dfree(MphCtx* c, void* p);   // free one ctx_alloc allocation now

template <typename T>
int ctx_dalloc(MphCtx* c, T** p, size_t count)
{
    int st = MPH_OK;
    *p = (T*)ctx_alloc(c, (count ? count : 1) * sizeof(T), &st);
    return st;
}

// what c->L holds besides the arrays: P (set_uniforms applied), stream, S and the environment's
// MPH_LIST_FULL / MPH_XCD_BAL_MIN
void ctx_fill_launch(MphCtx* c);
// cells between a fast-path interior particle and a grid face along axis d: stencil half-width + 1
inline int stencil_margin(const DevParams& P, int d)
{
    const int ca = contig_axis(P.dim, P.perm);
    return (d == ca ? P.sa : kReach) + 1;
}
int ctx_state_status(MphCtx* c, const DevState& hs);   // kernel error flags -> MphStatus
// the step graphs hold sizes and kernel arguments (monitors, slab message capacities): wait for
// the stream and destroy them; the next step captures again
int drop_graphs(MphCtx* c);

// The status read.  ctx_status_enqueue copies the kernels' error flags (the head of DevState) into
// the pinned hs_pin behind the stream, allocating it on first use (a pageable copy is staged by the
// runtime); ctx_status_landed maps the flags that have arrived to an MphStatus; ctx_status is both
// with the wait for the stream between them.  Polling the stream instead of the blocking wait
// measured the same per call (profiles/r05/sync_path/).
int ctx_status_enqueue(MphCtx* c);
int ctx_status_landed(MphCtx* c);
int ctx_status(MphCtx* c);

// The host's bookkeeping of nsteps steps: Time by the device's own repeated additions (the host
// mirror keeps them bit for bit), and that a step has run; a_current: the sorted set A and pres are
// now the current state's (mph_sample_grid; single contexts)
inline void ctx_advance_time(MphCtx* c, int nsteps)
{
    for (int k = 0; k < nsteps; ++k) c->time += c->cfg.dt;
}
inline void ctx_stepped(MphCtx* c, int nsteps, bool a_current)
{
    ctx_advance_time(c, nsteps);
    c->stepped = true;
    c->sel_current = false;   // the selection was the state's before these steps (mph_select)
    c->kin_current = false;   // and so were the kinematics (mph_compute_kinematics)
    c->set_since_step = false;
    if (a_current) c->a_current = true;
}

// A sequence of steps captured from the context's stream into an uploaded graph (so the first launch
// costs what later ones do): enqueue() puts the steps on the stream and returns MPH_OK or the status
// that ends the capture, whose graph is then destroyed.
template <typename Enqueue>
int ctx_capture(MphCtx* c, hipGraphExec_t* out, Enqueue enqueue)
{
    hipGraph_t g = nullptr;
    MPH_HIP_OK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue();
    const hipError_t e = hipStreamEndCapture(c->stream, &g);
    if (rc != MPH_OK) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
    }
    MPH_HIP_OK(c, e);
    const hipError_t ei = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    MPH_HIP_OK(c, ei);
    MPH_HIP_OK(c, hipGraphUpload(*out, c->stream));
    return MPH_OK;
}

// n steps replayed from the captured graphs in the order of replay_plan (mph_kernels.h): kSeq8t (no
// output-only stores) for every whole batch but the last where the context has it, kSeq8 for the
// last, then single steps -- kSeq1t for all but the last where the context has it, kSeq1 for the
// last, so the outputs are stored on the call's last step; a slab context has kSeq8 and kSeq1 only
int ctx_replay(MphCtx* c, int n);

// Step batching: launch the steps accepted but not launched and read the error flags of everything
// launched (mph_step.hip).  Every entry point that reads or changes the state, or waits for it,
// calls this first.
int ctx_flush(MphCtx* c);
// the entry of an extern "C" function on a context: null check, flush, device
inline int ctx_enter(MphCtx* c)
{
    if (!c) return MPH_ERR_ARG;
    MPH_CK(ctx_flush(c));
    MPH_HIP_OK(c, hipSetDevice(c->device));
    return MPH_OK;
}

// Per-kernel HIP event timing (mph_profile_steps, mph_sample_grid_timed).  A launch's start event
// behind a cross-stream wait reads as early as the wait packet itself (the time the stream went
// idle), so each launch that follows a join also keeps a floor: an event on the other stream at the
// joined point; its start is the later of the two.
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

// the steps of one sequence of a single context on L's stream (mph_step.hip); ev: phase timing's
// events, three per step, else null
void enqueue_steps(const Launch& L, StepSeq seq, hipEvent_t* ev = nullptr);

void ctx_set_global_error(const std::string& msg);   // mph_last_error(NULL)
// ids/n_glob: slab-local creation (the arrays hold n of n_glob particles, original indices ids)
int ctx_create(MphCtx** out, const MphConfig* cfg, int n, const int* property, const double* pos,
               const double* pos0, const double* vel, int device, MphDist* dist, const int* ids = nullptr,
               int n_glob = 0);
// count elements of a device array into h, on the context's stream (synchronize before reading h)
template <typename T>
int fetch(MphCtx* c, const T* d, std::vector<T>& h, size_t count)
{
    h.resize(count);
    if (count) MPH_HIP_OK(c, hipMemcpyAsync(h.data(), d, sizeof(T) * count, hipMemcpyDeviceToHost, c->stream));
    return MPH_OK;
}

// original index of host input k (identity unless created slab-local)
inline int glob_id(const MphCtx* c, int k) { return c->gid.empty() ? k : c->gid[k]; }

// slab mode (setup: mph_slab_geom.hip; steps: mph_dist.hip; output: mph_dist_output.hip; what those
// units share among themselves: mph_dist.h)
int dist_setup(MphCtx* c, const double* pos, std::vector<int>& owned);   // geometry + owned set
// elastic slots of this rank: lsl = [owned | ghosts from the left | ghosts from the right] (global
// slot ids), n_own owned; records the per-substep ghost exchange lists
int dist_struct_setup(MphCtx* c, std::vector<int>& lsl, int& n_own, int& n_inner);
int dist_alloc(MphCtx* c);                                               // exchange buffers
int dist_init(MphCtx* c);                                                // first exchange + init sums
int dist_step(MphCtx* c, int nsteps, Profiler* prof = nullptr);
// host mirror of the layout + error flags after a batch; grows message capacities past 90 %
int dist_sync(MphCtx* c, bool grow_ok = true);
// output in slab mode (collective): every rank's owned records gathered on rank 0, which writes
// `path` with the single-context writers (kind: kOut*); the virial over the owned particles
constexpr int kOutProf = 0, kOutVtk = 1, kOutVtu = 2, kOutVtkAsync = 3;
int dist_write_output(MphCtx* c, const char* path, int kind);
int dist_virial(MphCtx* c);
int virial_full_lists(MphCtx* c);   // the step's lists again with every neighbour (mph_fields.hip)
void dist_free(MphCtx* c);

}  // namespace mph
