// mph_ctx.h -- the device context behind the C ABI (include/mph_gpu.h), shared by the single-GPU
// implementation (mph_ctx.hip) and the slab-decomposed multi-GPU step (mph_dist.hip).
#pragma once

#include <hip/hip_runtime.h>

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
    hipGraphExec_t graph1 = nullptr, graph8 = nullptr;
    hipGraphExec_t graph1t = nullptr;   // one step without the output-only stores (single context)
    // step batching (mph_set_step_batching): single mph_step calls accumulate into 8-step graphs;
    // `pending` steps are accepted but not launched yet, `unchecked`: batches launched whose error
    // flags have not been read; the flags of the last launched batch land in hs_pin (pinned)
    bool batch_steps = false;
    int pending = 0;
    bool unchecked = false;
    void* hs_pin = nullptr;
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
    long long mon_read = 0;
    // lattice sampling (mph_sample_grid): the device result buffer (allocated at the first call,
    // regrown when a larger lattice arrives) and whether the sorted set A and pres are the current
    // state's -- a step has run since creation and no mph_set since
    double* sample_out = nullptr;
    size_t sample_cap = 0;       // doubles the allocation holds
    bool a_current = false;
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
int virial_full_lists(MphCtx* c);   // the step's lists again with every neighbour (mph_ctx.hip)
void dist_free(MphCtx* c);

}  // namespace mph
