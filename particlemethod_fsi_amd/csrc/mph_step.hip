// mph_step.hip -- the step sequencer of a single context: a sequence's launches (enqueue_steps), the
// captured step graphs and their replay, step batching, mph_step, phase timing.
#include <hip/hip_runtime.h>

#include <vector>

#include "mph_dist.h"

using namespace mph;

namespace mph {

// One step: its Launch (seq_step: the outputs it stores and its form, decided there and nowhere
// else) goes to the sort, the search and the two passes.  The elastic substeps and the monitors take
// the context's own: the last substep zeroes the Force of the clamped slots on every step
// (k_struct_velocity), and neither reads a trimmed field or the form otherwise.  The virial
// (k_virial) runs after a batch.
// ev (phase timing, else null): three events recorded on the stream at the step's phase
// boundaries -- before the sort, after the search (neighbour search = sort + search, as the
// reference's calculateNeighbor holds its own cell sort), after the elastic substeps.
static void enqueue_step(const Launch& L, const Launch& S, hipEvent_t* ev)
{
    if (ev) (void)hipEventRecord(ev[0], L.stream);
    launch_sort(S, 1);
    if (ev) {   // phase timing: the boundary between the search and pass A
        launch_neighbors(S);
        (void)hipEventRecord(ev[1], L.stream);
        launch_pass_a(S);
    } else {
        launch_search_pass_a(S);
    }
    launch_pass_b(S);
    launch_structure(L, stores_outputs(S));
    if (ev) (void)hipEventRecord(ev[2], L.stream);
    if (L.mon) launch_monitor(L, *L.mon);   // monitors on: this step's sample (mph_monitor.hip)
}

void enqueue_steps(const Launch& L, StepSeq seq, hipEvent_t* ev)
{
    for (int k = 0; k < seq.steps; ++k) enqueue_step(L, seq_step(L, seq, k), ev ? ev + 3 * k : nullptr);
}

// The step graphs, captured at the first mph_step whatever its count: a caller that warms up with
// fewer than 8 steps (the driver's bench: 5) would otherwise capture and upload the 8-step graph
// inside its first long run.  kSeq8t only where the context takes the lean batches.
static int capture_graphs(MphCtx* c)
{
    for (int kind = 0; kind < kSeqKinds; ++kind) {
        if (c->graph[kind] || (kind == kSeq8t && !c->lean_calls)) continue;
        MPH_CK(ctx_capture(c, &c->graph[kind], [&] {
            enqueue_steps(c->L, kSeqs[kind]);
            return MPH_OK;
        }));
    }
    return MPH_OK;
}

// phase timing: the events of a batch of `steps` steps (three per step) into the neighbour /
// explicit sums
static int accumulate_phases(MphCtx* c, const std::vector<hipEvent_t>& ev, int steps)
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

// The pending steps go as single-step graphs, the last one storing the output-only fields, so it
// leaves them current.
int ctx_flush(MphCtx* c)
{
    if (!c->pending && !c->unchecked) return MPH_OK;
    MPH_HIP_OK(c, hipSetDevice(c->device));
    if (c->pending) MPH_CK(capture_graphs(c));
    MPH_CK(ctx_replay(c, c->pending));
    c->pending = 0;
    c->unchecked = false;
    return ctx_status(c);
}

// mph_step with batching on: the steps are counted and launched 8 at a time from the 8-step graph
// (output-only fields stored on each batch's last step, as a multi-step mph_step does); the error
// flags of the last launched batch are copied back behind it and read without waiting once they
// have landed, so an error surfaces at most a batch or two late, and at the latest at the next
// flush point (mph_synchronize, mph_get, the writers, ...).
static int step_batched(MphCtx* c, int nsteps)
{
    ctx_stepped(c, nsteps, true);
    c->pending += nsteps;
    MPH_CK(capture_graphs(c));
    const int full = c->pending - c->pending % 8;
    MPH_CK(ctx_replay(c, full));
    c->pending -= full;
    if (full) {
        MPH_CK(ctx_status_enqueue(c));
        MPH_HIP_OK(c, hipEventRecord(c->ev_status, c->stream));
        c->unchecked = true;
    }
    if (c->unchecked && hipEventQuery(c->ev_status) == hipSuccess) MPH_CK(ctx_status_landed(c));
    return MPH_OK;
}

}  // namespace mph

extern "C" {

int mph_set_step_batching(MphCtx* c, int on)
{
    if (!c) return MPH_ERR_ARG;
    if (c->dist) return on ? ctx_fail(c, MPH_ERR_ARG, "step batching is not available in slab mode") : MPH_OK;
    MPH_HIP_OK(c, hipSetDevice(c->device));
    if (!on) {
        c->batch_steps = false;
        return ctx_flush(c);
    }
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
        ctx_advance_time(c, nsteps);
        return MPH_OK;
    }
    if (c->batch_steps && !c->phase_timing) return step_batched(c, nsteps);
    MPH_CK(ctx_flush(c));
    if (c->phase_timing) {
        // the graphs' batches (replay_plan: the same steps store the output-only fields) as direct
        // launches with the phase events (HIP cannot time events recorded inside a captured graph),
        // read after every batch
        const ReplayPlan p = replay_plan(nsteps, c->lean_calls, true);
        for (int kind = 0; kind < kSeqKinds; ++kind)
            for (int r = 0; r < p.count[kind]; ++r) {
                enqueue_steps(c->L, kSeqs[kind], c->ev8.data());
                MPH_HIP_OK(c, hipGetLastError());
                MPH_CK(accumulate_phases(c, c->ev8, kSeqs[kind].steps));
            }
    } else {
        MPH_CK(capture_graphs(c));
        MPH_CK(ctx_replay(c, nsteps));
    }
    ctx_stepped(c, nsteps, true);
    return ctx_status(c);
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

}  // extern "C"
