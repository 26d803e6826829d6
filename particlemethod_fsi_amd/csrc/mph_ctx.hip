// mph_ctx.hip -- the core of the device context behind include/mph_gpu.h: errors, allocation, the
// launch record, the host helpers every other context unit uses (mph_ctx.h), synchronize, the
// trivial getters and destroy.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "mph_dist.h"
#include "mph_env.h"

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

int ctx_status_enqueue(MphCtx* c)
{
    if (!c->hs_pin) MPH_HIP_OK(c, hipHostMalloc(&c->hs_pin, kStateHead, hipHostMallocDefault));
    MPH_HIP_OK(c, hipMemcpyAsync(c->hs_pin, c->L.st, kStateHead, hipMemcpyDeviceToHost, c->stream));
    return MPH_OK;
}

int ctx_status_landed(MphCtx* c)
{
    DevState hs;
    std::memcpy(&hs, c->hs_pin, kStateHead);
    return ctx_state_status(c, hs);
}

int ctx_status(MphCtx* c)
{
    MPH_CK(ctx_status_enqueue(c));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    return ctx_status_landed(c);
}

int drop_graphs(MphCtx* c)
{
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    for (hipGraphExec_t& g : c->graph)
        if (g) {
            MPH_HIP_OK(c, hipGraphExecDestroy(g));
            g = nullptr;
        }
    return MPH_OK;
}

int ctx_replay(MphCtx* c, int n)
{
    const ReplayPlan p = replay_plan(n, c->graph[kSeq8t] != nullptr, c->graph[kSeq1t] != nullptr);
    for (int kind = 0; kind < kSeqKinds; ++kind)
        for (int k = 0; k < p.count[kind]; ++k) MPH_HIP_OK(c, hipGraphLaunch(c->graph[kind], c->stream));
    return MPH_OK;
}

void ctx_fill_launch(MphCtx* c)
{
    Launch& L = c->L;
    set_uniforms(c->P);
    // MPH_LIST_FULL=1: the lists keep every neighbour within the search radius, like the reference's
    // Neighbor[] (mph_neighbor_rows needs them); else only those the passes' sums can take
    if (env_int("MPH_LIST_FULL", 0) == 1) c->P.rlf = 3.0e38f;
    // MPH_LAZY_WALLS=0: no lazy wall steps (seq_step), every step searches and sums every wall
    // wave; slab contexts never take them (a halo wall may have a fluid neighbour on the next rank)
    c->lazy_walls = !c->dist && env_int("MPH_LAZY_WALLS", 1) != 0;
    // MPH_LEAN_STEPS=0: the lazy steps launch the kernels of the full steps' arithmetic (seq_step);
    // the lean search also needs the list radius below the search radius' FP32 band (lean_search_ok:
    // not with MPH_LIST_FULL=1)
    L.lean_ok = env_int("MPH_LEAN_STEPS", 1) != 0;
    L.lean_search = L.lean_ok && lean_search_ok(c->P);
    // MPH_LEAN_CALLS=0: every whole batch of a call ends in a step that stores the output-only fields
    // (no kSeq8t graph, replay_plan), not only the call's last; slab contexts never take the lean batches
    c->lean_calls = !c->dist && env_int("MPH_LEAN_CALLS", 1) != 0;
    // MPH_KEY_FOLD=0: every step opens with k_prep, no pass B leaves the next step's cell keys
    // (seq_step); slab contexts never fold
    L.key_fold = !c->dist && env_int("MPH_KEY_FOLD", 1) != 0;
    // MPH_LIST16=0: every wave keeps the 32-bit list rows; else the 3-D interior waves whose group
    // spans allow take the 16-bit ones (mph_params.h kOff16Bits).  MPH_LIST16_SPAN (tests): a lower
    // span limit, so that small cases mix the formats.  Slab contexts keep the wide rows.
    c->P.list16_span = 0;
    if (!c->dist && c->P.dim == 3 && env_int("MPH_LIST16", 1) != 0) {
        const int span = env_is("MPH_LIST16_SPAN", "") ? kList16Span : env_int("MPH_LIST16_SPAN", kList16Span);
        c->P.list16_span = span < 0 ? 0 : (span > kList16Span ? kList16Span : span);
    }
    L.P = &c->P;
    L.stream = c->stream;
    // work-balanced XCD map of the passes from this many particles (MPH_XCD_BAL_MIN: tests force it
    // on small cases, the default keeps it off below 2^20 where the split kernel costs more)
    L.xcd_bal_min = env_is("MPH_XCD_BAL_MIN", "") ? (1 << 20) : env_int("MPH_XCD_BAL_MIN", 1 << 20);
    L.S = &c->Sd;
}

}  // namespace mph

extern "C" {

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

int mph_get_scalars(const MphCtx* c, double* out)
{
    if (!c || !out) return MPH_ERR_ARG;
    fill_scalars(c->h, c->cfg, out);
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
    for (hipGraphExec_t g : c->graph)
        if (g) (void)hipGraphExecDestroy(g);
    for (auto* v : {&c->ev8, &c->ev_vir})
        for (hipEvent_t e : *v) (void)hipEventDestroy(e);
    if (c->dist) dist_free(c);
    for (void* p : c->allocs) (void)hipFree(p);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

}  // extern "C"
