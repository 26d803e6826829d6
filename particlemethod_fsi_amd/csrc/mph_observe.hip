// mph_observe.hip -- the host half of what observes a run without downloading its fields: the
// per-step monitors (kernels: mph_monitor.hip) and the lattice sampling (kernel: mph_sample.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mph_ctx.h"

using namespace mph;

extern "C" {

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

}  // extern "C"
