// mph_observe.hip -- the host half of what observes a run without downloading its fields: the
// per-step monitors (kernels: mph_monitor.hip), the free-surface gauges (kernels: mph_gauge.hip) and
// the lattice sampling (kernel: mph_sample.hip) -- on a single context and, through entry points of
// their own (mph_dist_*), on slab ranks, where a lattice's planes are dealt to the ranks by the slab
// that holds them and the collective calls gather on rank 0.
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

// The device result buffer of the lattice calls holds at least `need` doubles.
static int sample_buffer(MphCtx* c, size_t need)
{
    if (need <= c->sample_cap) return MPH_OK;
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    ctx_dfree(c, c->sample_out);
    c->sample_out = nullptr;
    c->sample_cap = 0;
    MPH_CK(ctx_dalloc(c, &c->sample_out, need));
    c->sample_cap = need;
    return MPH_OK;
}

// The argument rules of mph_sample_grid, shared with the slab ranks' calls; *points: the lattice's.
static int sample_args(MphCtx* c, const MphSampleGrid* g, long long* points)
{
    *points = 1;
    for (int d = 0; d < 3; ++d) {
        if (g->count[d] < 1 || !(g->spacing[d] > 0.0) || !std::isfinite(g->spacing[d]) || !std::isfinite(g->origin[d]))
            return ctx_fail(c, MPH_ERR_ARG, "sample grid: counts must be >= 1, spacings > 0 and the origin finite");
        *points *= g->count[d];   // (at most 2^24 before each factor below 2^31)
        if (*points > MPH_SAMPLE_MAX_POINTS)
            return ctx_fail(c, MPH_ERR_ARG, "sample grid: more than MPH_SAMPLE_MAX_POINTS = " +
                                                std::to_string(MPH_SAMPLE_MAX_POINTS) + " points");
    }
    if (c->cfg.dim == 2 && g->count[2] != 1) return ctx_fail(c, MPH_ERR_ARG, "sample grid: count[2] must be 1 in 2-D");
    if (g->classes < 0 || g->classes > 7) return ctx_fail(c, MPH_ERR_ARG, "sample grid: class mask outside 0..7");
    const double reach = c->h.max_radius + 0.1 * c->h.dx;   // MaxRadius + MARGIN (make_dev_params)
    if (!(g->radius >= 0.0) || g->radius > reach)
        return ctx_fail(c, MPH_ERR_ARG, "sample grid: radius outside [0, MaxRadius + MARGIN = " + std::to_string(reach) + "]");
    return MPH_OK;
}

// the lattice, the resolved class mask and the radius of *g (the tiling is the caller's)
static void sample_dev(const MphCtx* c, const MphSampleGrid* g, SampleDev& G)
{
    for (int d = 0; d < 3; ++d) {
        G.origin[d] = g->origin[d];
        G.spacing[d] = g->spacing[d];
        G.count[d] = g->count[d];
    }
    G.mask = g->classes ? g->classes : 1;
    G.h = g->radius > 0.0 ? g->radius : c->h.rp;
}

// The argument rules of mph_gauge_grid, shared with the slab ranks' calls: *lines the lattice's, and G
// filled but for its launch shape (nlines, waves).
static int gauge_args(MphCtx* c, const MphGaugeGrid* g, long long* lines, GaugeGridDev& G)
{
    *lines = 1;
    for (int d = 0; d < 3; ++d) {
        if (g->count[d] < 1 || !std::isfinite(g->spacing[d]) || !std::isfinite(g->origin[d]) ||
            (g->count[d] > 1 && !(g->spacing[d] > 0.0)))
            return ctx_fail(c, MPH_ERR_ARG, "gauge grid: counts must be >= 1, the origin finite and a spacing > 0 where its count is above 1");
        *lines *= g->count[d];   // (at most 2^20 before each factor below 2^31)
        if (*lines > MPH_GAUGE_GRID_MAX_LINES)
            return ctx_fail(c, MPH_ERR_ARG, "gauge grid: more than MPH_GAUGE_GRID_MAX_LINES = " +
                                                std::to_string(MPH_GAUGE_GRID_MAX_LINES) + " lines");
    }
    MPH_CK(gauge_resolve(c, g->axis, g->radius, &G.axis, &G.h, &G.nbins));
    if (g->count[G.axis] != 1) return ctx_fail(c, MPH_ERR_ARG, "gauge grid: the count along the lines' axis must be 1");
    if (c->cfg.dim == 2 && g->count[2] != 1) return ctx_fail(c, MPH_ERR_ARG, "gauge grid: count[2] must be 1 in 2-D");
    for (int d = 0; d < 3; ++d) {
        G.origin[d] = g->origin[d];
        G.spacing[d] = g->spacing[d];
        G.count[d] = g->count[d];
    }
    return MPH_OK;
}

// ---- the planes of a lattice on slab ranks ---------------------------------------------------------

// a run of consecutive lattice planes along the slab axis
struct PlaneRun {
    int first, count;
};

// the runs of planes `rank` owns, ascending (owner: lattice_owners)
static std::vector<PlaneRun> plane_runs(const std::vector<int>& owner, int rank)
{
    std::vector<PlaneRun> runs;
    for (int i = 0; i < (int)owner.size(); ++i) {
        if (owner[i] != rank) continue;
        if (!runs.empty() && runs.back().first + runs.back().count == i) ++runs.back().count;
        else runs.push_back({i, 1});
    }
    return runs;
}

// points of one plane across `axis`
static size_t plane_points(const int* count, int axis)
{
    size_t n = 1;
    for (int d = 0; d < 3; ++d)
        if (d != axis) n *= (size_t)count[d];
    return n;
}

// The planes of run r, packed as a lattice of their own ([k][j][i], count[axis] = r.count, ch doubles a
// point), written to their rows of the whole lattice `whole`; every other row stays as it is.
static void planes_unpack(const int* count, int axis, PlaneRun r, int ch, const double* packed, double* whole)
{
    int lc[3] = {count[0], count[1], count[2]};
    lc[axis] = r.count;
    const size_t row = (size_t)lc[0] * ch;
    for (int k = 0; k < lc[2]; ++k)
        for (int j = 0; j < lc[1]; ++j) {
            const size_t gk = k + (axis == 2 ? r.first : 0), gj = j + (axis == 1 ? r.first : 0);
            const size_t gi = axis == 0 ? r.first : 0;
            std::memcpy(whole + ((gk * count[1] + gj) * count[0] + gi) * ch,
                        packed + ((size_t)k * lc[1] + j) * row, sizeof(double) * row);
        }
}

// every rank's packed runs, one behind the other in run order, to their rows of `whole`
static void planes_unpack_all(const int* count, int axis, const std::vector<PlaneRun>& runs, int ch,
                              const double* packed, double* whole)
{
    const size_t plane = plane_points(count, axis);
    for (const PlaneRun& r : runs) {
        planes_unpack(count, axis, r, ch, packed, whole);
        packed += (size_t)r.count * plane * ch;
    }
}

// A rank's message of the collective lattice calls: its number of doubles, then the doubles.  Rank 0
// gathers them (MPH_ERR_TRANSPORT where that fails) and finds rank r's doubles at of[r], n[r] of them.
static int gather_doubles(MphCtx* c, const std::vector<double>& mine, std::vector<double>& all,
                          std::vector<const double*>& of, std::vector<size_t>& n)
{
    MphDist& D = *c->dist;
    static_assert(sizeof(long long) == sizeof(double), "the count travels in a double's slot");
    std::vector<char> msg(sizeof(double) * (1 + mine.size())), got;
    const long long k = (long long)mine.size();
    std::memcpy(msg.data(), &k, sizeof(k));
    if (k) std::memcpy(msg.data() + sizeof(double), mine.data(), sizeof(double) * mine.size());
    MPH_CK(D.tr->gather_root(c, c->stream, msg, got));
    if (D.rank != 0) return MPH_OK;
    all.resize(got.size() / sizeof(double));
    if (!all.empty()) std::memcpy(all.data(), got.data(), all.size() * sizeof(double));
    of.assign(D.nranks, nullptr);
    n.assign(D.nranks, 0);
    size_t at = 0;
    for (int r = 0; r < D.nranks; ++r) {
        long long kr = -1;
        if (at < all.size()) std::memcpy(&kr, &all[at], sizeof(kr));
        if (kr < 0 || at + 1 + (size_t)kr > all.size())
            return ctx_fail(c, MPH_ERR_TRANSPORT, "slab lattice: the message of rank " + std::to_string(r) + " is incomplete");
        of[r] = all.data() + at + 1;
        n[r] = (size_t)kr;
        at += 1 + (size_t)kr;
    }
    return MPH_OK;
}

// What the slab ranks' lattice calls open with: the flush, a slab context, the device.
static int dist_lattice_enter(MphCtx* c, const char* single)
{
    MPH_CK(ctx_flush(c));
    if (!c->dist)
        return ctx_fail(c, MPH_ERR_UNSUPPORTED, std::string("slab lattice calls need a slab context (a single context: ") + single + ")");
    MPH_HIP_OK(c, hipSetDevice(c->device));
    return MPH_OK;
}

// This rank's planes of the lattice *g, sampled: `owner` the planes' owners, `packed` the rank's runs
// one behind the other (planes_unpack_all).  One launch and one copy per run, each of the run's
// planes alone.
static int dist_sample_packed(MphCtx* c, const MphSampleGrid* g, std::vector<int>& owner, std::vector<double>& packed)
{
    long long points = 1;
    MPH_CK(sample_args(c, g, &points));
    if (!c->a_current)
        return ctx_fail(c, MPH_ERR_ARG, "sample grid: run a step first (none since creation or since the last mph_set)");
    const MphDist& D = *c->dist;
    const int axis = D.g.axis;
    owner.resize(g->count[axis]);
    lattice_owners(c->h, axis, D.nranks, dist_cuts(D), g->origin[axis], g->spacing[axis], g->count[axis], owner.data());
    const std::vector<PlaneRun> runs = plane_runs(owner, D.rank);
    const size_t plane = plane_points(g->count, axis) * MPH_SAMPLE_CHANNELS;
    size_t total = 0, most = 0;
    for (const PlaneRun& r : runs) {
        total += (size_t)r.count * plane;
        most = std::max(most, (size_t)r.count * plane);
    }
    packed.resize(total);
    if (runs.empty()) return MPH_OK;
    MPH_CK(sample_buffer(c, most));
    size_t at = 0;
    for (const PlaneRun& r : runs) {
        SampleRunDev G{};
        sample_dev(c, g, G);
        G.count[axis] = r.count;
        G.first = r.first;
        if (sample_tiling(G, contig_axis(c->P.dim, c->P.perm)) > 0x7fffffffLL) return ctx_fail(c, MPH_ERR_ARG, "sample grid: too many tiles");
        launch_dist_sample_grid(c->L, G, c->sample_out);
        MPH_HIP_OK(c, hipGetLastError());
        const size_t n = (size_t)r.count * plane;
        MPH_HIP_OK(c, hipMemcpyAsync(packed.data() + at, c->sample_out, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
        // (the next run's launch overwrites the buffer: the copy has left it)
        MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
        at += n;
    }
    return MPH_OK;
}

// This rank's records of the lines of *g ([lines][MPH_DIST_GAUGE_RECORD]).  Lines parallel to the slab
// axis: one launch over every line.  Other lines: one launch per run of the planes the rank owns; the
// lines of every other plane get the record of a rank that does not own them.
static int dist_gauge_records(MphCtx* c, const MphGaugeGrid* g, std::vector<double>& records, long long* nlines)
{
    GaugeRunDev G{};
    MPH_CK(gauge_args(c, g, nlines, G));
    if (!c->a_current)
        return ctx_fail(c, MPH_ERR_ARG, "gauge grid: run a step first (none since creation or since the last mph_set)");
    const MphDist& D = *c->dist;
    const int axis = D.g.axis;
    const size_t lines = (size_t)*nlines;
    const double other[MPH_DIST_GAUGE_RECORD] = {-1.0, -INFINITY, INFINITY, 0.0, -1.0, -1.0};
    records.resize(lines * MPH_DIST_GAUGE_RECORD);
    for (size_t k = 0; k < records.size(); ++k) records[k] = other[k % MPH_DIST_GAUGE_RECORD];
    std::vector<PlaneRun> runs;
    if (G.axis == axis) {
        runs.push_back({0, 1});   // (count[axis] is 1: the whole lattice)
    } else {
        std::vector<int> owner(g->count[axis]);
        // (a count of 1 may come with a spacing of 0: the one plane is the origin's)
        lattice_owners(c->h, axis, D.nranks, dist_cuts(D), g->origin[axis], g->spacing[axis], g->count[axis], owner.data());
        runs = plane_runs(owner, D.rank);
    }
    const size_t plane = plane_points(g->count, axis) * MPH_DIST_GAUGE_RECORD;
    size_t most = 0;
    for (const PlaneRun& r : runs) most = std::max(most, (size_t)r.count * plane);
    if (runs.empty()) return MPH_OK;
    MPH_CK(sample_buffer(c, most));
    std::vector<double> packed(most);
    G.waves = env_int("MPH_GAUGE_GRID_WAVES", 4) == 1 ? 1 : 4;
    for (const PlaneRun& r : runs) {
        GaugeRunDev R = G;
        R.count[axis] = r.count;
        R.first = r.first;
        R.nlines = (int)((size_t)r.count * plane / MPH_DIST_GAUGE_RECORD);
        launch_dist_gauge_grid(c->L, R, c->sample_out);
        MPH_HIP_OK(c, hipGetLastError());
        MPH_HIP_OK(c, hipMemcpyAsync(packed.data(), c->sample_out, sizeof(double) * (size_t)r.count * plane,
                                     hipMemcpyDeviceToHost, c->stream));
        MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
        planes_unpack(g->count, axis, r, MPH_DIST_GAUGE_RECORD, packed.data(), records.data());
    }
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
    GaugeGridDev G{};
    MPH_CK(gauge_args(c, g, &lines, G));
    const size_t need = (size_t)lines * MPH_GAUGE_CHANNELS;
    if (c->n == 0) {
        const double empty[MPH_GAUGE_CHANNELS] = {0.0, -INFINITY, INFINITY, 0.0};
        for (size_t k = 0; k < need; ++k) out[k] = empty[k % MPH_GAUGE_CHANNELS];
        return MPH_OK;
    }
    if (!c->a_current)
        return ctx_fail(c, MPH_ERR_ARG, "gauge grid: run a step first (none since creation or since the last mph_set)");
    MPH_HIP_OK(c, hipSetDevice(c->device));
    MPH_CK(sample_buffer(c, need));
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
    MPH_CK(sample_args(c, g, &points));
    const size_t need = (size_t)points * MPH_SAMPLE_CHANNELS;
    if (c->n == 0) {
        std::memset(out, 0, sizeof(double) * need);
        return MPH_OK;
    }
    if (!c->a_current)
        return ctx_fail(c, MPH_ERR_ARG, "sample grid: run a step first (none since creation or since the last mph_set)");
    MPH_HIP_OK(c, hipSetDevice(c->device));
    MPH_CK(sample_buffer(c, need));
    SampleDev G{};
    sample_dev(c, g, G);
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

// ---- lattice sampling and elevation maps on slab ranks (kernels: the slab forms) ---------------------

int mph_dist_sample_grid_partial(MphCtx* c, const MphSampleGrid* g, double* out, long long* owned_points)
{
    if (!c || !g || !out) return MPH_ERR_ARG;
    if (owned_points) *owned_points = 0;
    MPH_CK(dist_lattice_enter(c, "mph_sample_grid"));
    std::vector<int> owner;
    std::vector<double> packed;
    MPH_CK(dist_sample_packed(c, g, owner, packed));
    const MphDist& D = *c->dist;
    planes_unpack_all(g->count, D.g.axis, plane_runs(owner, D.rank), MPH_SAMPLE_CHANNELS, packed.data(), out);
    if (owned_points) *owned_points = (long long)(packed.size() / MPH_SAMPLE_CHANNELS);
    return MPH_OK;
}

int mph_dist_sample_grid(MphCtx* c, const MphSampleGrid* g, double* out)
{
    if (!c || !g) return MPH_ERR_ARG;
    MPH_CK(dist_lattice_enter(c, "mph_sample_grid"));
    const MphDist& D = *c->dist;
    if (D.rank == 0 && !out) return ctx_fail(c, MPH_ERR_ARG, "sample grid: rank 0 receives the lattice and needs out");
    std::vector<int> owner;
    std::vector<double> packed, all;
    MPH_CK(dist_sample_packed(c, g, owner, packed));
    std::vector<const double*> of;
    std::vector<size_t> n;
    MPH_CK(gather_doubles(c, packed, all, of, n));
    if (D.rank != 0) return MPH_OK;
    const size_t plane = plane_points(g->count, D.g.axis) * MPH_SAMPLE_CHANNELS;
    for (int r = 0; r < D.nranks; ++r) {
        const std::vector<PlaneRun> runs = plane_runs(owner, r);
        size_t want = 0;
        for (const PlaneRun& q : runs) want += (size_t)q.count * plane;
        if (n[r] != want)
            return ctx_fail(c, MPH_ERR_TRANSPORT, "sample grid: rank " + std::to_string(r) + " sent " + std::to_string(n[r]) +
                                                      " doubles, its planes hold " + std::to_string(want));
        planes_unpack_all(g->count, D.g.axis, runs, MPH_SAMPLE_CHANNELS, of[r], out);
    }
    return MPH_OK;
}

int mph_dist_gauge_grid_partial(MphCtx* c, const MphGaugeGrid* g, double* records)
{
    if (!c || !g || !records) return MPH_ERR_ARG;
    MPH_CK(dist_lattice_enter(c, "mph_gauge_grid"));
    std::vector<double> rec;
    long long lines = 0;
    MPH_CK(dist_gauge_records(c, g, rec, &lines));
    std::memcpy(records, rec.data(), sizeof(double) * rec.size());
    return MPH_OK;
}

int mph_gauge_combine(int nranks, long long nlines, const double* const* records, double* out)
{
    if (nranks < 1 || nlines < 0 || !records || (nlines > 0 && !out)) return MPH_ERR_ARG;
    for (int r = 0; r < nranks && nlines > 0; ++r)
        if (!records[r]) return MPH_ERR_ARG;
    for (long long l = 0; l < nlines; ++l) {
        double count = 0.0, top = -INFINITY, bottom = INFINITY, wet = 0.0;
        bool any = false;
        double hibin = -1.0;   // of the last non-empty rank so far; -1: none yet
        for (int r = 0; r < nranks; ++r) {
            const double* q = records[r] + (size_t)l * MPH_DIST_GAUGE_RECORD;
            if (!(q[0] >= 0.0)) continue;
            any = true;
            count += q[0];
            top = std::fmax(top, q[1]);
            bottom = std::fmin(bottom, q[2]);
            wet += q[3];
            if (q[0] > 0.0) {
                if (hibin >= 0.0 && hibin == q[4]) wet -= 1.0;   // the bin the two ranks share
                hibin = q[5];
            }
        }
        if (!any) return MPH_ERR_ARG;
        double* o = out + (size_t)l * MPH_GAUGE_CHANNELS;
        o[MPH_GAUGE_COUNT] = count;
        o[MPH_GAUGE_TOP] = top;
        o[MPH_GAUGE_BOTTOM] = bottom;
        o[MPH_GAUGE_WET] = wet;
    }
    return MPH_OK;
}

int mph_dist_gauge_grid(MphCtx* c, const MphGaugeGrid* g, double* out)
{
    if (!c || !g) return MPH_ERR_ARG;
    MPH_CK(dist_lattice_enter(c, "mph_gauge_grid"));
    const MphDist& D = *c->dist;
    if (D.rank == 0 && !out) return ctx_fail(c, MPH_ERR_ARG, "gauge grid: rank 0 receives the map and needs out");
    std::vector<double> rec, all;
    long long lines = 0;
    MPH_CK(dist_gauge_records(c, g, rec, &lines));
    std::vector<const double*> of;
    std::vector<size_t> n;
    MPH_CK(gather_doubles(c, rec, all, of, n));
    if (D.rank != 0) return MPH_OK;
    for (int r = 0; r < D.nranks; ++r)
        if (n[r] != (size_t)lines * MPH_DIST_GAUGE_RECORD)
            return ctx_fail(c, MPH_ERR_TRANSPORT, "gauge grid: rank " + std::to_string(r) + " sent " + std::to_string(n[r]) +
                                                      " doubles for " + std::to_string(lines) + " lines");
    const int rc = mph_gauge_combine(D.nranks, lines, of.data(), out);
    if (rc != MPH_OK) return ctx_fail(c, rc, "gauge grid: the ranks' records do not combine (a line computed on no rank)");
    return MPH_OK;
}

}  // extern "C"
