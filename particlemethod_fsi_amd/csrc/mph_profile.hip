// mph_profile.hip -- measurement and diagnostics of a context: the per-kernel profilers
// (mph_profile_steps, mph_profile_graphs) and the list and counter readers (mph_neighbor_stats,
// mph_list_stats, mph_list_layout, mph_idle_wall_stats, mph_lean_step_stats, mph_key_fold_stats,
// mph_list_format_stats, mph_list_span_misses, mph_list_wave_formats, mph_neighbor_rows).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "mph_dist.h"
#include "mph_rows.h"

using namespace mph;

extern "C" {

int mph_profile_steps(MphCtx* c, int nsteps, double* avg_ms, int* launches, char* names32)
{
    if (nsteps <= 0 || !avg_ms || !launches || !names32) return MPH_ERR_ARG;
    MPH_CK(ctx_enter(c));
    EventProfiler prof;
    if (c->dist) {
        MPH_CK(dist_step(c, nsteps, &prof));
    } else {
        Launch L = c->L;
        L.prof = &prof;
        enqueue_steps(L, StepSeq{nsteps, true});
        MPH_HIP_OK(c, hipGetLastError());
        MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
        ctx_stepped(c, nsteps, true);
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
    MPH_CK(ctx_status(c));
    return k;
}

// The list kernels as the timed steps run them: each one captured `reps` times into a graph of
// its own (the output-only stores on every 8th, as in the 8-step graph; never a lazy step's form,
// there is no sort in front of it to mark the map), replayed once to warm, then once between two
// HIP events.  Each replay recomputes what the last step left (the lists,
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
    Launch full = c->L;
    if (c->dist) full.wface = c->dist->wface;   // slab mode: pass B in one launch (phase 0)
    const Launch trimmed = trim_outputs(full);
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
                const Launch& La = last ? full : trimmed;
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
    return ctx_status(c);
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
    if (!mean || !mx) return MPH_ERR_ARG;
    MPH_CK(ctx_enter(c));
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
    R.base.resize(ntile * kBaseInts);
    if (!n) return MPH_OK;
    MPH_HIP_OK(c, hipMemcpy(R.rows.data(), c->L.ncount, sizeof(int) * n, hipMemcpyDeviceToHost));
    MPH_HIP_OK(c, hipMemcpy(R.hdr.data(), c->L.lhdr, sizeof(R.hdr[0]) * ntile, hipMemcpyDeviceToHost));
    MPH_HIP_OK(c, hipMemcpy(R.gap.data(), c->L.lgap, sizeof(R.gap[0]) * n, hipMemcpyDeviceToHost));
    MPH_HIP_OK(c, hipMemcpy(R.base.data(), c->L.lbase, sizeof(int) * R.base.size(), hipMemcpyDeviceToHost));
    return MPH_OK;
}

int mph_list_stats(MphCtx* c, double* mean, int* mx)
{
    if (!mean || !mx) return MPH_ERR_ARG;
    MPH_CK(ctx_enter(c));
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
        // the jumps that left a gap in some lane: every jump of a wide wave; of a short wave, which
        // jumps at every group end, only those (so the counts compare with MPH_LIST16=0)
        int J = 0;
        for (int k = 0; k < gap_count(R.hdr[t]); ++k) {
            bool gap = false;
            for (long long s = t * kTile; s < std::min<long long>(n, (t + 1) * kTile) && !gap; ++s)
                gap = gap_begin(R.gap[s], k) < std::min(gap_end(R.hdr[t], k), std::min(R.rows[s], kTileRows));
            J += gap;
        }
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

// the counter readers' entry: the context entered and its stream drained, so the counters at the tail
// of DevState are those of every step launched
static int counters_enter(MphCtx* c, const long long* out)
{
    if (!out) return MPH_ERR_ARG;
    MPH_CK(ctx_enter(c));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    return MPH_OK;
}

// two adjacent unsigned long long counters of DevState, the first at byte offset `first`, in one copy
static int counter_pair(MphCtx* c, size_t first, long long out[2])
{
    MPH_CK(counters_enter(c, out));
    unsigned long long v[2] = {0, 0};
    MPH_HIP_OK(c, hipMemcpy(v, reinterpret_cast<const char*>(c->L.st) + first, sizeof(v), hipMemcpyDeviceToHost));
    out[0] = (long long)v[0];
    out[1] = (long long)v[1];
    return MPH_OK;
}

int mph_idle_wall_stats(MphCtx* c, long long out[2])
{
    MPH_CK(counters_enter(c, out));
    // the lazy steps, then the idle waves per run of the waves
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
    static_assert(offsetof(DevState, lean_pass_a_steps) == offsetof(DevState, lean_search_steps) + sizeof(long long),
                  "the two counters are read in one copy");
    return counter_pair(c, offsetof(DevState, lean_search_steps), out);
}

int mph_list_format_stats(MphCtx* c, long long out[3])
{
    MPH_CK(counters_enter(c, out));
    // the header words of the last search: the waves' flags
    const size_t ntile = ((size_t)c->n + kTile - 1) / kTile;
    std::vector<unsigned long long> hdr(ntile);
    if (ntile) MPH_HIP_OK(c, hipMemcpy(hdr.data(), c->L.lhdr, sizeof(hdr[0]) * ntile, hipMemcpyDeviceToHost));
    out[0] = out[1] = out[2] = 0;
    // (only the 3-D search chooses a format and keeps the restart byte)
    for (unsigned long long h : hdr) {
        const bool d3 = c->P.dim == 3;
        out[d3 && hdr_short(h) ? 0 : 1] += 1;
        out[2] += d3 && hdr_restarted(h);
    }
    return MPH_OK;
}

int mph_list_span_misses(MphCtx* c, long long* out)
{
    MPH_CK(counters_enter(c, out));
    const size_t ntile = ((size_t)c->n + kTile - 1) / kTile;
    std::vector<unsigned long long> hdr(ntile);
    if (ntile) MPH_HIP_OK(c, hipMemcpy(hdr.data(), c->L.lhdr, sizeof(hdr[0]) * ntile, hipMemcpyDeviceToHost));
    *out = 0;
    for (unsigned long long h : hdr) *out += c->P.dim == 3 && !hdr_short(h) && hdr_span_miss(h);
    return MPH_OK;
}

int mph_list_wave_formats(MphCtx* c, int* out)
{
    if (!out) return MPH_ERR_ARG;
    MPH_CK(ctx_enter(c));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    // the header words and the group bases of the last search, wave by wave
    const size_t ntile = ((size_t)c->n + kTile - 1) / kTile;
    std::vector<unsigned long long> hdr(ntile);
    std::vector<int> base(ntile * kBaseInts);
    if (ntile) {
        MPH_HIP_OK(c, hipMemcpy(hdr.data(), c->L.lhdr, sizeof(hdr[0]) * ntile, hipMemcpyDeviceToHost));
        MPH_HIP_OK(c, hipMemcpy(base.data(), c->L.lbase, sizeof(int) * base.size(), hipMemcpyDeviceToHost));
    }
    static_assert(kGroups < kBaseInts && kBaseInts == 8, "a wave's record: the format and its kGroups bases");
    for (size_t t = 0; t < ntile; ++t) {
        int* o = out + t * kBaseInts;
        const unsigned long long h = hdr[t];
        // (only the 3-D search chooses a format and keeps the restart byte)
        const bool d3 = c->P.dim == 3;
        o[0] = !d3 ? 0 : hdr_short(h) ? 1 : hdr_restarted(h) ? 2 : hdr_span_miss(h) ? 3 : 0;
        for (int g = 0; g < kGroups; ++g) o[1 + g] = o[0] == 1 ? base[t * kBaseInts + g] : 0;
    }
    return MPH_OK;
}

int mph_key_fold_stats(MphCtx* c, long long out[2])
{
    static_assert(offsetof(DevState, prep_steps) == offsetof(DevState, key_fold_steps) + sizeof(long long),
                  "the two counters are read in one copy");
    return counter_pair(c, offsetof(DevState, key_fold_steps), out);
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
            const int j = R.entry(s, e, buf.data());
            if (j >= n || q >= m) return ctx_fail(c, MPH_ERR_HIP, "mph_neighbor_rows: list entry past the particle count");
            ids[w + q++] = id[j];
        }
        if (q != m) return ctx_fail(c, MPH_ERR_HIP, "mph_neighbor_rows: list rows disagree with NeighborCount");
        std::sort(ids + w, ids + w + m);
        w += m;
    }
    return (int)std::min<long long>(w, 0x7fffffff);
}

}  // extern "C"
