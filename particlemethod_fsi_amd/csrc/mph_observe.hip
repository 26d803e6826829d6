// mph_observe.hip -- the host half of what observes a run without downloading its fields: the
// per-step monitors (kernels: mph_monitor.hip), the free-surface gauges (kernels: mph_gauge.hip) and
// the lattice sampling (kernel: mph_sample.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mph_dist.h"
#include "mph_env.h"

using namespace mph;

// A monitor configuration's ring: `capacity` samples of `width` doubles (the allocation regrown when
// too small), emptied -- the counters zeroed, so STEP counts from here -- and nothing read yet.
static int monitor_ring(MphCtx* c, int capacity, int width)
{
    MonitorDev& D = c->mon;
    const size_t need = (size_t)capacity * width;
    if (need > c->mon_ring_cap) {
        ctx_dfree(c, D.ring);
        D.ring = nullptr;
        c->mon_ring_cap = 0;
        MPH_CK(ctx_dalloc(c, &D.ring, need));
        c->mon_ring_cap = need;
    }
    MPH_HIP_OK(c, hipMemset(D.counters, 0, 2 * sizeof(long long)));
    D.capacity = capacity;
    D.width = width;
    c->mon_read = 0;
    return MPH_OK;
}

// What the gauges of mph_gauge_configure and the lines of mph_gauge_grid share: the axis (-1: the
// largest |gravity| component's), the radius (0: RadiusP) and the bins along the axis.
static int gauge_resolve(MphCtx* c, int axis, double radius, int* ax, double* h, int* nbins)
{
    const int dim = c->cfg.dim;
    if (axis == -1) {
        double best = 0.0;
        for (int d = 0; d < dim; ++d)
            if (std::fabs(c->cfg.gravity[d]) > best) {
                best = std::fabs(c->cfg.gravity[d]);
                axis = d;
            }
        if (axis < 0) return ctx_fail(c, MPH_ERR_ARG, "gauges: axis -1 needs a gravity component");
    }
    if (axis < 0 || axis >= dim)
        return ctx_fail(c, MPH_ERR_ARG, "gauges: axis " + std::to_string(axis) + " outside 0.." + std::to_string(dim - 1));
    const double reach = c->h.max_radius + 0.1 * c->h.dx;   // MaxRadius + MARGIN (make_dev_params)
    if (!(radius >= 0.0) || radius > reach)
        return ctx_fail(c, MPH_ERR_ARG, "gauges: radius outside [0, MaxRadius + MARGIN = " + std::to_string(reach) + "]");
    const double bins = std::ceil((c->cfg.domain_max[axis] - c->cfg.domain_min[axis]) / c->cfg.particle_spacing);
    if (!(bins >= 1.0) || bins > (double)MPH_GAUGE_MAX_BINS)
        return ctx_fail(c, MPH_ERR_ARG, "gauges: the domain has " + std::to_string(bins) + " bins of particle_spacing along axis " +
                                            std::to_string(axis) + ", outside 1..MPH_GAUGE_MAX_BINS = " +
                                            std::to_string(MPH_GAUGE_MAX_BINS));
    *ax = axis;
    *h = radius > 0.0 ? radius : c->h.rp;
    *nbins = (int)bins;
    return MPH_OK;
}

// the unread samples of the ring, oldest first (mph_monitor_read, mph_dist_monitor_read_partial)
static long long monitor_read_ring(MphCtx* c, double* out, long long max_samples, long long* lost)
{
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

// What mph_monitor_configure and mph_dist_monitor_configure share: the argument rules, then the
// buffers (once, for the maxima of either), the emptied ring of `capacity` samples of head + `row`
// doubles per tracked entry + 2 per probe, and the uploaded configuration in c->mon.
static int monitor_setup(MphCtx* c, const MphMonitorConfig* m, int row)
{
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
        // (a slab rank's launches are sized for its capacity; its tracked rows are the longer ones)
        MPH_CK(ctx_dalloc(c, &D.partial, (size_t)kMonPartial * monitor_blocks(c->dist ? c->dist->cap : c->n)));
        MPH_CK(ctx_dalloc(c, &D.trk, kDistMonRow * (size_t)MPH_MONITOR_MAX_TRACK));
        MPH_CK(ctx_dalloc(c, &D.prb, 2 * (size_t)MPH_MONITOR_MAX_PROBES));
        MPH_CK(ctx_dalloc(c, &c->mon_sorted, MPH_MONITOR_MAX_TRACK));
        MPH_CK(ctx_dalloc(c, &c->mon_map, MPH_MONITOR_MAX_TRACK));
        MPH_CK(ctx_dalloc(c, &c->mon_probes, kMonProbeOwn + (size_t)MPH_MONITOR_MAX_PROBES));
        D.track_sorted = c->mon_sorted;
        D.track_map = c->mon_map;
        D.probes = c->mon_probes;
    }
    // (the whole configuration is replaced: no gauges until the next mph_gauge_configure)
    MPH_CK(monitor_ring(c, m->capacity, MPH_MONITOR_HEAD + row * m->ntrack + 2 * m->nprobe));
    D.ngauge = 0;
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
    MPH_HIP_OK(c, hipMemset(D.trk, 0, sizeof(double) * kDistMonRow * MPH_MONITOR_MAX_TRACK));
    MPH_HIP_OK(c, hipMemset(D.prb, 0, sizeof(double) * 2 * MPH_MONITOR_MAX_PROBES));
    D.stride = m->stride;
    D.ntrack = m->ntrack;
    D.nprobe = m->nprobe;
    D.probe_h = m->probe_radius > 0.0 ? m->probe_radius : c->h.rp;
    return MPH_OK;
}

extern "C" {

// ---- per-step monitors (kernels: mph_monitor.hip) ----------------------------------------------

int mph_monitor_configure(MphCtx* c, const MphMonitorConfig* m)
{
    if (!c) return MPH_ERR_ARG;
    MPH_CK(ctx_flush(c));
    if (c->dist)
        return ctx_fail(c, MPH_ERR_UNSUPPORTED, "monitors are not available in slab mode: a rank's record is a partial "
                                                "one (mph_dist_monitor_configure)");
    MPH_HIP_OK(c, hipSetDevice(c->device));
    if (!m) {
        if (c->mon_on) MPH_CK(drop_graphs(c));
        c->mon_on = false;
        c->L.mon = nullptr;
        return MPH_OK;
    }
    MPH_CK(monitor_setup(c, m, 6));
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
    return monitor_read_ring(c, out, max_samples, lost);
}

// ---- slab monitors: rank records and their combine (kernels: mph_monitor.hip, the slab forms) -----

int mph_dist_monitor_configure(MphCtx* c, const MphMonitorConfig* m)
{
    if (!c) return MPH_ERR_ARG;
    MPH_CK(ctx_flush(c));
    if (!c->dist)
        return ctx_fail(c, MPH_ERR_UNSUPPORTED, "slab monitors need a slab context (a single context: mph_monitor_configure)");
    MPH_HIP_OK(c, hipSetDevice(c->device));
    if (!m) {
        if (c->dmon_on) MPH_CK(drop_graphs(c));
        c->dmon_on = false;
        return MPH_OK;
    }
    // (a probe's radius is at most MaxRadius + MARGIN = sqrt(rc2) up to its rounding, below the halo
    // sqrt(rc2) (1 + 1e-6): the owner's ghosts hold every particle within it of a point of its slab)
    MPH_CK(monitor_setup(c, m, kDistMonRow));
    // who evaluates a probe: the rank whose slab holds its coordinate, wrapped like a particle's --
    // decided here, once, with the context's cuts; the kernels take the verdict as a flag
    const MphDist& D = *c->dist;
    std::vector<double> own(MPH_MONITOR_MAX_PROBES, 0.0);
    for (int q = 0; q < m->nprobe; ++q)
        own[q] = owner_rank(c->h, D.g.axis, D.nranks, dist_cuts(D), m->probes[3 * q + D.g.axis]) == D.rank ? 1.0 : 0.0;
    MPH_HIP_OK(c, hipMemcpy(c->mon_probes + kMonProbeOwn, own.data(), sizeof(double) * own.size(), hipMemcpyHostToDevice));
    c->dmon_on = true;
    return MPH_OK;
}

int mph_dist_monitor_record_doubles(const MphCtx* c) { return c && c->dmon_on ? c->mon.width : 0; }

long long mph_dist_monitor_read_partial(MphCtx* c, double* out, long long max_samples, long long* lost)
{
    if (!c || max_samples < 0 || (max_samples > 0 && !out)) return MPH_ERR_ARG;
    if (lost) *lost = 0;
    MPH_CK(ctx_flush(c));
    if (!c->dmon_on) return 0;
    return monitor_read_ring(c, out, max_samples, lost);
}

int mph_monitor_combine(int nranks, int ntrack, int nprobe, long long nsamples, const double* const* records,
                        double* out)
{
#pragma clang fp contract(off)
    if (nranks < 1 || ntrack < 0 || ntrack > MPH_MONITOR_MAX_TRACK || nprobe < 0 || nprobe > MPH_MONITOR_MAX_PROBES ||
        nsamples < 0 || !records || (nsamples > 0 && !out))
        return MPH_ERR_ARG;
    for (int r = 0; r < nranks && nsamples > 0; ++r)
        if (!records[r]) return MPH_ERR_ARG;
    const size_t wr = MPH_MONITOR_HEAD + (size_t)kDistMonRow * ntrack + 2 * (size_t)nprobe;
    const size_t wo = MPH_MONITOR_HEAD + 6 * (size_t)ntrack + 2 * (size_t)nprobe;
    for (long long s = 0; s < nsamples; ++s) {
        const auto rec = [&](int r) { return records[r] + (size_t)s * wr; };
        double* o = out + (size_t)s * wo;
        for (int r = 1; r < nranks; ++r)
            if (rec(r)[MPH_MON_STEP] != rec(0)[MPH_MON_STEP]) return MPH_ERR_ARG;
        o[MPH_MON_STEP] = rec(0)[MPH_MON_STEP];
        o[MPH_MON_TIME] = rec(0)[MPH_MON_TIME];
        // rank 0's value, then ranks 1, 2, ... in order (EPOT: each rank's own negated sum)
        for (int k = 0; k < kMonPartial; ++k) {
            double v = rec(0)[kMonFirst + k];
            for (int r = 1; r < nranks; ++r) {
                const double a = rec(r)[kMonFirst + k];
                v = mon_op(k) == 0 ? v + a : (mon_op(k) == 1 ? std::fmin(v, a) : std::fmax(v, a));
            }
            o[kMonFirst + k] = v;
        }
        for (int e = kMonFirst + kMonPartial; e < MPH_MONITOR_HEAD; ++e) o[e] = 0.0;
        // a tracked entry from the one rank that holds the particle, a probe from the one that owns it
        for (int k = 0; k < ntrack; ++k) {
            int from = -1, count = 0;
            for (int r = 0; r < nranks; ++r)
                if (rec(r)[MPH_MONITOR_HEAD + kDistMonRow * k] == 1.0) {
                    from = r;
                    ++count;
                }
            if (count != 1) return MPH_ERR_ARG;
            for (int e = 0; e < 6; ++e) o[MPH_MONITOR_HEAD + 6 * k + e] = rec(from)[MPH_MONITOR_HEAD + kDistMonRow * k + 1 + e];
        }
        for (int q = 0; q < nprobe; ++q) {
            int from = -1, count = 0;
            for (int r = 0; r < nranks; ++r)
                if (rec(r)[MPH_MONITOR_HEAD + kDistMonRow * ntrack + 2 * q + 1] >= 0.0) {
                    from = r;
                    ++count;
                }
            if (count != 1) return MPH_ERR_ARG;
            for (int e = 0; e < 2; ++e)
                o[MPH_MONITOR_HEAD + 6 * ntrack + 2 * q + e] = rec(from)[MPH_MONITOR_HEAD + kDistMonRow * ntrack + 2 * q + e];
        }
    }
    return MPH_OK;
}

long long mph_dist_monitor_read(MphCtx* c, double* out, long long max_samples, long long* lost)
{
    if (!c || max_samples < 0 || (max_samples > 0 && !out)) return MPH_ERR_ARG;
    if (lost) *lost = 0;
    MPH_CK(ctx_flush(c));
    if (!c->dist)
        return ctx_fail(c, MPH_ERR_UNSUPPORTED, "slab monitors need a slab context (a single context: mph_monitor_read)");
    if (!c->dmon_on) return 0;
    MphDist& D = *c->dist;
    const size_t w = (size_t)c->mon.width;
    // this rank's message: its count, then its records
    std::vector<double> rows((size_t)std::min<long long>(max_samples, c->mon.capacity) * w + 1);
    const long long k = monitor_read_ring(c, rows.data() + 1, max_samples, lost);
    if (k < 0) return k;
    static_assert(sizeof(long long) == sizeof(double), "the count travels in a record's slot");
    std::memcpy(rows.data(), &k, sizeof(k));
    const char* b = reinterpret_cast<const char*>(rows.data());
    std::vector<char> mine(b, b + sizeof(double) * (1 + (size_t)k * w)), all;
    MPH_CK(D.tr->gather_root(c, c->stream, mine, all));
    if (D.rank != 0) return 0;
    std::vector<double> recs(all.size() / sizeof(double));
    if (!all.empty()) std::memcpy(recs.data(), all.data(), recs.size() * sizeof(double));
    std::vector<const double*> of(D.nranks);
    size_t at = 0;
    for (int r = 0; r < D.nranks; ++r) {
        long long kr = -1;
        if (at < recs.size()) std::memcpy(&kr, &recs[at], sizeof(kr));
        if (kr != k || at + 1 + (size_t)k * w > recs.size())
            return ctx_fail(c, MPH_ERR_TRANSPORT, "slab monitors: rank " + std::to_string(r) + " holds " + std::to_string(kr) +
                                                      " unread records, rank 0 " + std::to_string(k));
        of[r] = recs.data() + at + 1;
        at += 1 + (size_t)k * w;
    }
    const int rc = mph_monitor_combine(D.nranks, c->mon.ntrack, c->mon.nprobe, k, of.data(), out);
    if (rc != MPH_OK) return ctx_fail(c, rc, "slab monitors: the ranks' records do not combine (a tracked particle or a probe on no rank or on several, or unequal steps)");
    return k;
}

// ---- free-surface gauges (kernels: mph_gauge.hip) -----------------------------------------------

int mph_gauge_configure(MphCtx* c, const MphGaugeConfig* g)
{
    if (!c) return MPH_ERR_ARG;
    MPH_CK(ctx_flush(c));
    if (c->dist)
        return ctx_fail(c, MPH_ERR_UNSUPPORTED, "gauges are not available in slab mode (a line spans the ranks)");
    if (!c->mon_on) return ctx_fail(c, MPH_ERR_ARG, "gauges: the monitors are off (mph_monitor_configure first)");
    MPH_HIP_OK(c, hipSetDevice(c->device));
    const int ngauge = g ? g->ngauge : 0;
    if (ngauge < 0 || ngauge > MPH_GAUGE_MAX || (ngauge > 0 && !g->points))
        return ctx_fail(c, MPH_ERR_ARG, "gauges: 0.." + std::to_string(MPH_GAUGE_MAX) + " gauges");
    int axis = 0, nbins = 1;
    double h = 0.0;
    if (ngauge > 0) MPH_CK(gauge_resolve(c, g->axis, g->radius, &axis, &h, &nbins));
    MPH_CK(drop_graphs(c));
    MonitorDev& D = c->mon;
    if (!D.gau) {   // once, for the maximum
        MPH_CK(ctx_dalloc(c, &c->mon_gauges, 3 * (size_t)MPH_GAUGE_MAX));
        MPH_CK(ctx_dalloc(c, &D.gau, (size_t)MPH_GAUGE_CHANNELS * MPH_GAUGE_MAX));
        D.gauges = c->mon_gauges;
    }
    MPH_CK(monitor_ring(c, D.capacity, MPH_MONITOR_HEAD + 6 * D.ntrack + 2 * D.nprobe + MPH_GAUGE_CHANNELS * ngauge));
    std::vector<double> points(3 * (size_t)MPH_GAUGE_MAX, 0.0);
    if (ngauge > 0) std::copy(g->points, g->points + 3 * (size_t)ngauge, points.begin());
    MPH_HIP_OK(c, hipMemcpy(c->mon_gauges, points.data(), sizeof(double) * points.size(), hipMemcpyHostToDevice));
    MPH_HIP_OK(c, hipMemset(D.gau, 0, sizeof(double) * MPH_GAUGE_CHANNELS * MPH_GAUGE_MAX));
    D.ngauge = ngauge;
    D.gauge_axis = axis;
    D.gauge_nbins = nbins;
    D.gauge_h = h;
    return MPH_OK;
}

int mph_gauge_grid(MphCtx* c, const MphGaugeGrid* g, double* out)
{
    if (!c || !g || !out) return MPH_ERR_ARG;
    MPH_CK(ctx_flush(c));
    if (c->dist)
        return ctx_fail(c, MPH_ERR_UNSUPPORTED, "gauge grid: not available in slab mode (a line spans the ranks)");
    long long lines = 1;
    for (int d = 0; d < 3; ++d) {
        if (g->count[d] < 1 || !std::isfinite(g->spacing[d]) || !std::isfinite(g->origin[d]) ||
            (g->count[d] > 1 && !(g->spacing[d] > 0.0)))
            return ctx_fail(c, MPH_ERR_ARG, "gauge grid: counts must be >= 1, the origin finite and a spacing > 0 where its count is above 1");
        lines *= g->count[d];   // (at most 2^20 before each factor below 2^31)
        if (lines > MPH_GAUGE_GRID_MAX_LINES)
            return ctx_fail(c, MPH_ERR_ARG, "gauge grid: more than MPH_GAUGE_GRID_MAX_LINES = " +
                                                std::to_string(MPH_GAUGE_GRID_MAX_LINES) + " lines");
    }
    GaugeGridDev G{};
    MPH_CK(gauge_resolve(c, g->axis, g->radius, &G.axis, &G.h, &G.nbins));
    if (g->count[G.axis] != 1) return ctx_fail(c, MPH_ERR_ARG, "gauge grid: the count along the lines' axis must be 1");
    if (c->cfg.dim == 2 && g->count[2] != 1) return ctx_fail(c, MPH_ERR_ARG, "gauge grid: count[2] must be 1 in 2-D");
    const size_t need = (size_t)lines * MPH_GAUGE_CHANNELS;
    if (c->n == 0) {
        const double empty[MPH_GAUGE_CHANNELS] = {0.0, -INFINITY, INFINITY, 0.0};
        for (size_t k = 0; k < need; ++k) out[k] = empty[k % MPH_GAUGE_CHANNELS];
        return MPH_OK;
    }
    if (!c->a_current)
        return ctx_fail(c, MPH_ERR_ARG, "gauge grid: run a step first (none since creation or since the last mph_set)");
    MPH_HIP_OK(c, hipSetDevice(c->device));
    if (need > c->sample_cap) {
        MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
        ctx_dfree(c, c->sample_out);
        c->sample_out = nullptr;
        c->sample_cap = 0;
        MPH_CK(ctx_dalloc(c, &c->sample_out, need));
        c->sample_cap = need;
    }
    for (int d = 0; d < 3; ++d) {
        G.origin[d] = g->origin[d];
        G.spacing[d] = g->spacing[d];
        G.count[d] = g->count[d];
    }
    G.nlines = (int)lines;
    // four lines to a 256-thread block, as measured; 1: one line per block (A/B)
    G.waves = env_int("MPH_GAUGE_GRID_WAVES", 4) == 1 ? 1 : 4;
    launch_gauge_grid(c->L, G, c->sample_out);
    MPH_HIP_OK(c, hipGetLastError());
    MPH_HIP_OK(c, hipMemcpyAsync(out, c->sample_out, sizeof(double) * need, hipMemcpyDeviceToHost, c->stream));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    return MPH_OK;
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
