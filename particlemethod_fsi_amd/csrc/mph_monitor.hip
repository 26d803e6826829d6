// mph_monitor.hip -- per-step monitors (include/mph_gpu.h mph_monitor_*): sums, extrema, tracked
// particles and pressure probes of the state a step leaves, reduced on the device into one record
// per sampled step of a ring buffer.  Launched at the end of every step (enqueue_steps) while
// monitors are on, so a sample is taken by whichever path runs the step (captured graphs, direct
// launches) and the host reads the ring without breaking a batch.
//
// Three plain launches per step (the probe kernel only with probes; with gauges a fourth, the gauge
// kernel of mph_gauge.hip, before the final one) and no floating-point atomics:
// every block of k_monitor_partial owns a fixed range of particles and stores one partial record;
// k_monitor_final adds the records in a fixed order.  A sample is therefore a function of the state
// alone, bit for bit, in any batch shape.
//
// On a slab rank (mph_dist_monitor_configure; launched by mph_dist.hip at the end of every slab step)
// the same three kernels run in their SLAB forms and leave the rank's record: the head over the
// particles the rank owns, a {present, x, y, z, vx, vy, vz} row per tracked entry, the probes its slab
// holds; mph_monitor_combine (mph_observe.hip) makes samples of the ranks' records on the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "mph_device.h"
#include "mph_kernels.h"
#include "mph_params.h"

namespace mph {

constexpr int kMonThreads = 256;
constexpr int kMonItems = 4;                         // particles per thread of k_monitor_partial
constexpr int kMonBlock = kMonThreads * kMonItems;   // particles per block
constexpr int kMonWaves = kMonThreads / 64;
// a probe's stencil columns, one lane each
static_assert(kGroups * kGroups <= 64, "one lane per stencil column of a probe");

int monitor_blocks(int n) { return blocks(n, kMonBlock); }

// Partial record: entry k is head slot kMonFirst + k; mon_op(k) (mph_kernels.h) says how it combines.
// Identity of entry k (VMAX2 of an empty class is 0: v.v >= 0)
__device__ __forceinline__ double mon_init(int k)
{
    return mon_op(k) == 0 || k < 18 ? 0.0 : (mon_op(k) == 1 ? __builtin_inf() : -__builtin_inf());
}
__device__ __forceinline__ double mon_combine(int k, double a, double b)
{
    return mon_op(k) == 0 ? a + b : (mon_op(k) == 1 ? fmin(a, b) : fmax(a, b));
}

// A lane's accumulators, by kind: the sums (class c's COUNT, KE, PX, PY, PZ at 5 c + q, EPOT last),
// the minima (XMIN, YMIN, ZMIN, the fluid's PMIN) and the maxima (VMAX2 per class, XMAX, YMAX, ZMAX,
// the fluid's and the walls' PMAX); mon_entry_* give each one's entry in the partial record.
constexpr int kMonSums = 16, kMonMins = 4, kMonMaxs = 8;
static_assert(kMonSums + kMonMins + kMonMaxs == kMonPartial, "the three kinds make the record");
__host__ __device__ constexpr int mon_entry_sum(int i) { return i == 15 ? 27 : 6 * (i / 5) + i % 5; }
__host__ __device__ constexpr int mon_entry_min(int i) { return i == 3 ? 24 : 18 + 2 * i; }
__host__ __device__ constexpr int mon_entry_max(int i) { return i < 3 ? 6 * i + 5 : (i < 6 ? 19 + 2 * (i - 3) : 19 + i); }

// a block's record from its lanes' accumulators: the waves' records through LDS, combined in wave
// order; entry k in thread k (k < kMonPartial)
__device__ __forceinline__ double mon_block_reduce(double (&sum)[kMonSums], double (&mn)[kMonMins],
                                                   double (&mx)[kMonMaxs], double (*red)[kMonPartial])
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double ws = mon_wave_fold<0>(sum), wn = mon_wave_fold<1>(mn), wx = mon_wave_fold<2>(mx);
    if (lane < kMonSums) red[wave][mon_entry_sum(lane)] = ws;
    if (lane < kMonMins) red[wave][mon_entry_min(lane)] = wn;
    if (lane < kMonMaxs) red[wave][mon_entry_max(lane)] = wx;
    __syncthreads();
    double v = 0.0;
    if (threadIdx.x < kMonPartial) {
        const int k = threadIdx.x;
        v = red[0][k];
        for (int w = 1; w < kMonWaves; ++w) v = mon_combine(k, v, red[w][k]);
    }
    return v;
}

// One partial record per block over its kMonBlock particles of the integrated set B (in the sorted
// order of this step, as `pres`), and the tracked particles' rows.
// SLAB, a slab rank's record (launch_dist_monitor): B is [owned | ghosts], n is the capacity the grid
// is sized for and the live count is read here.  Only the owned particles count: a ghost (id < 0) is
// skipped like a slot past n, so an owned particle goes through the arithmetic of a single context,
// in the order of B.  A block past the live count stores the identities (k_monitor_final adds every
// record of the grid).  A tracked row is {present, x, y, z, vx, vy, vz}.
template <bool SLAB>
__global__ __launch_bounds__(kMonThreads) void k_monitor_partial(DevParams P, MonitorDev M, int n, Soa B,
                                                                 const double* __restrict__ pres)
{
#pragma clang fp contract(off)
    long long step;
    if (!mon_sampled(M, step)) return;
    __shared__ int s_ids[MPH_MONITOR_MAX_TRACK];
    __shared__ double s_mass[kTypes];
    __shared__ double s_red[kMonWaves][kMonPartial];
    const int tid = threadIdx.x;
    if (SLAB) {
        n = dev_n(P);
        if (blockIdx.x * kMonBlock >= n) {
            if (tid < kMonPartial) M.partial[(size_t)blockIdx.x * kMonPartial + tid] = mon_init(tid);
            return;
        }
    }
    if (tid < MPH_MONITOR_MAX_TRACK) s_ids[tid] = M.track_sorted[tid];
    if (tid < kTypes) s_mass[tid] = P.mass[tid];
    __syncthreads();
    // the block's loads first (8-byte SoA loads, consecutive lanes consecutive elements)
    double x[kMonItems], y[kMonItems], z[kMonItems], vx[kMonItems], vy[kMonItems], vz[kMonItems], pr[kMonItems];
    int ty[kMonItems], id[kMonItems];
    const int base = blockIdx.x * kMonBlock + tid;
#pragma unroll
    for (int it = 0; it < kMonItems; ++it) {
        const int p = base + it * kMonThreads;
        ty[it] = -1;
        if (p < n) {
            x[it] = B.x[p]; y[it] = B.y[p]; z[it] = B.z[p];
            vx[it] = B.vx[p]; vy[it] = B.vy[p]; vz[it] = B.vz[p];
            pr[it] = pres[p];
            ty[it] = B.type[p];
            id[it] = B.id[p];
            if (SLAB && id[it] < 0) ty[it] = -1;
        }
    }
    double sum[kMonSums], mn[kMonMins], mx[kMonMaxs];
#pragma unroll
    for (int k = 0; k < kMonSums; ++k) sum[k] = 0.0;
#pragma unroll
    for (int k = 0; k < kMonMins; ++k) mn[k] = __builtin_inf();
#pragma unroll
    for (int k = 0; k < kMonMaxs; ++k) mx[k] = k < 3 ? 0.0 : -__builtin_inf();   // (VMAX2 of no particle: 0)
#pragma unroll
    for (int it = 0; it < kMonItems; ++it) {
        const int t = ty[it];
        if (t < 0 || t >= kTypes) continue;
        const int cls = t >> 1;   // 0 fluid (types 0, 1), 1 structure (2, 3), 2 wall (4, 5)
        const double m = s_mass[t];
        const double v2 = vx[it] * vx[it] + vy[it] * vy[it] + vz[it] * vz[it];
        const double ke = 0.5 * m * v2;
        const double px = m * vx[it], py = m * vy[it], pz = m * vz[it];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const bool s = cls == c;
            sum[5 * c + 0] += s ? 1.0 : 0.0;
            sum[5 * c + 1] += s ? ke : 0.0;
            sum[5 * c + 2] += s ? px : 0.0;
            sum[5 * c + 3] += s ? py : 0.0;
            sum[5 * c + 4] += s ? pz : 0.0;
            mx[c] = s ? fmax(mx[c], v2) : mx[c];
        }
        if (cls == 0) {
            mn[0] = fmin(mn[0], x[it]); mx[3] = fmax(mx[3], x[it]);
            mn[1] = fmin(mn[1], y[it]); mx[4] = fmax(mx[4], y[it]);
            mn[2] = fmin(mn[2], z[it]); mx[5] = fmax(mx[5], z[it]);
            mn[3] = fmin(mn[3], pr[it]); mx[6] = fmax(mx[6], pr[it]);
        }
        if (cls == 2) mx[7] = fmax(mx[7], pr[it]);
        // m (g . x); k_monitor_final negates the sum
        if (cls < 2) sum[15] += m * (P.gravity[0] * x[it] + P.gravity[1] * y[it] + P.gravity[2] * z[it]);
        if (M.ntrack > 0) {
            // lower bound among the 64 sorted ids (padded with INT_MAX)
            int lo = 0;
#pragma unroll
            for (int w = MPH_MONITOR_MAX_TRACK / 2; w > 0; w >>= 1)
                if (s_ids[lo + w - 1] < id[it]) lo += w;
            if (s_ids[lo] == id[it]) {
                double* o = M.trk + (SLAB ? kDistMonRow * lo + 1 : 6 * lo);
                if (SLAB) o[-1] = 1.0;
                o[0] = x[it]; o[1] = y[it]; o[2] = z[it];
                o[3] = vx[it]; o[4] = vy[it]; o[5] = vz[it];
            }
        }
    }
    const double v = mon_block_reduce(sum, mn, mx, s_red);
    if (tid < kMonPartial) M.partial[(size_t)blockIdx.x * kMonPartial + tid] = v;
}

// One wavefront per probe: the Shepard average of PressureP over the fluid particles of the sorted
// set A (the positions PressureP was computed at) within M.probe_h of the probe.  Lane c takes
// stencil column c: along the contiguous axis its cells are one index range of start[], two where
// the column wraps; the lanes then stride the concatenated runs.
// SLAB: only on the rank that owns the probe (the flag behind the probes, kMonProbeOwn).  A is the
// rank's sorted set, owned and ghosts, on its window grid, which is not periodic along the slab axis:
// there the stencil is clipped at the window's two ends instead of wrapped (a cell past an end would
// be one from the window's other end, not the domain's).  The distance stays the minimum image.
template <int DIM, bool SLAB>
__global__ __launch_bounds__(64) void k_monitor_probe(DevParams P, MonitorDev M, int n, Soa A,
                                                      const int* __restrict__ start,
                                                      const double* __restrict__ pres)
{
#pragma clang fp contract(off)
    long long step;
    if (!mon_sampled(M, step)) return;
    constexpr int kSeg = 128;   // two runs per lane
    __shared__ int s_off[kSeg], s_beg[kSeg];
    const int q = blockIdx.x, lane = threadIdx.x;
    if (SLAB) {
        if (M.probes[kMonProbeOwn + q] == 0.0) return;
        n = dev_n(P);
    }
    // the probe, wrapped into the periodic domain like a particle
    const double pq[3] = {M.probes[3 * q], M.probes[3 * q + 1], DIM == 3 ? M.probes[3 * q + 2] : 0.0};
    double p[3];
    wrap_point(P, DIM, pq, p);
    // lane c's column of the probe's stencil: one run of start[], two where the column wraps
    PointStencil<DIM> S(P, p);
    bool column = lane < PointStencil<DIM>::ncol;
    if (SLAB) {
        const int ax = P.slab_axis, g = ax == 0 ? P.gc[0] : (ax == 1 ? P.gc[1] : P.gc[2]);
        const int cc = ax == 0 ? S.c[0] : (ax == 1 ? S.c[1] : S.c[2]);
        if (ax == S.ca) {
            S.lo = max(cc - P.sa, 0);
            S.hi = min(cc + P.sa, g - 1);
            S.lo1 = 0;
            S.hi1 = -1;
        } else {
            // (the column's offset along the slab axis, as PointStencil::column takes it)
            const int d = (ax == S.a0 ? (DIM == 3 ? lane / kGroups : lane) : lane % kGroups) - kReach;
            column = column && cc + d >= 0 && cc + d < g;
        }
    }
    int b0 = 0, len0 = 0, b1 = 0, len1 = 0;
    if (column) {
        const int cell0 = S.column(P, lane);
        b0 = start[cell0 + S.lo];
        len0 = start[cell0 + S.hi + 1] - b0;
        if (S.hi1 >= S.lo1) {
            b1 = start[cell0 + S.lo1];
            len1 = start[cell0 + S.hi1 + 1] - b1;
        }
    }
    // exclusive offsets of the runs
    int incl = len0 + len1;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const int u = __shfl_up(incl, m, 64);
        if (lane >= m) incl += u;
    }
    const int excl = incl - (len0 + len1);
    const int total = __shfl(incl, 63, 64);
    s_off[2 * lane] = excl;
    s_beg[2 * lane] = b0;
    s_off[2 * lane + 1] = excl + len0;
    s_beg[2 * lane + 1] = b1;
    __syncthreads();
    const double h = M.probe_h;
    double swp = 0.0, sw = 0.0, cnt = 0.0;
    for (int t = lane; t < total; t += 64) {
        // the last run that starts at or before t (empty runs share their successor's offset)
        int s = 0;
#pragma unroll
        for (int w = kSeg / 2; w > 0; w >>= 1)
            if (s + w < kSeg && s_off[s + w] <= t) s += w;
        const int j = s_beg[s] + (t - s_off[s]);
        if (j < 0 || j >= n) continue;
        if (A.type[j] >= 2) continue;
        double w;
        if (shepard_weight<DIM>(P, p, h, A.x[j], A.y[j], DIM == 3 ? A.z[j] : 0.0, w)) {
            swp += w * pres[j];
            sw += w;
            cnt += 1.0;
        }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        swp += __shfl_xor(swp, m, 64);
        sw += __shfl_xor(sw, m, 64);
        cnt += __shfl_xor(cnt, m, 64);
    }
    if (lane == 0) {
        M.prb[2 * q] = sw > 0.0 ? swp / sw : 0.0;
        M.prb[2 * q + 1] = cnt;
    }
}

// One block: the partial records combined in a fixed order, the sample written to its ring slot,
// the counters advanced.  Thread (g, k) of 32 groups of 32 takes entry k of the records g, g + 32,
// ... (a record's 28 entries are one contiguous read), then thread k the 32 groups' results in
// order.  The only writer of the counters, on every step.
// SLAB: the rank record -- the head over the owned particles (nb: every block of the capacity-sized
// grid; those past the live count hold the identities, so a record's place in the order is the one it
// has among the live blocks), {present, x, y, z, vx, vy, vz} per tracked entry, all zero unless the
// particle is owned here at this step (the rows are cleared behind the read), {value, count} per probe
// owned here and {0, -1} per other probe.
constexpr int kMonFinalThreads = 1024, kMonGroups = kMonFinalThreads / 32;
static_assert(kDistMonRow * MPH_MONITOR_MAX_TRACK <= kMonFinalThreads, "one thread per double of the tracked rows");
template <bool SLAB>
__global__ __launch_bounds__(kMonFinalThreads) void k_monitor_final(MonitorDev M, int nb,
                                                                    const DevState* __restrict__ st)
{
#pragma clang fp contract(off)
    __shared__ double s_red[kMonGroups][kMonPartial];
    const int tid = threadIdx.x, g = tid >> 5, k = tid & 31;
    long long step;
    const bool sampled = mon_sampled(M, step);
    if (sampled) {
        if (k < kMonPartial) {
            double a = mon_init(k);
            // eight records' loads in flight at a time (the adds stay in record order)
            constexpr int U = 8;
            for (int b = g; b < nb; b += U * kMonGroups) {
                double r[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int bu = b + u * kMonGroups;
                    r[u] = bu < nb ? M.partial[(size_t)bu * kMonPartial + k] : mon_init(k);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) a = mon_combine(k, a, r[u]);
            }
            s_red[g][k] = a;
        }
        __syncthreads();
        double* out = M.ring + (size_t)(M.counters[1] % M.capacity) * M.width;
        if (tid < kMonPartial) {
            double v = s_red[0][tid];
            for (int w = 1; w < kMonGroups; ++w) v = mon_combine(tid, v, s_red[w][tid]);
            out[kMonFirst + tid] = tid == kMonPartial - 1 ? -v : v;
        }
        if (tid == 0) {
            out[0] = (double)step;
            out[1] = st->time;
            for (int e = kMonFirst + kMonPartial; e < MPH_MONITOR_HEAD; ++e) out[e] = 0.0;
        }
        constexpr int row = SLAB ? kDistMonRow : 6;
        if (tid < M.ntrack) {
            const double* r = M.trk + row * M.track_map[tid];
            for (int e = 0; e < row; ++e) out[MPH_MONITOR_HEAD + row * tid + e] = r[e];
        }
        if (tid < M.nprobe) {
            const bool mine = !SLAB || M.probes[kMonProbeOwn + tid] != 0.0;
            out[MPH_MONITOR_HEAD + row * M.ntrack + 2 * tid] = mine ? M.prb[2 * tid] : 0.0;
            out[MPH_MONITOR_HEAD + row * M.ntrack + 2 * tid + 1] = mine ? M.prb[2 * tid + 1] : -1.0;
        }
        // the gauges' records (k_monitor_gauge, mph_gauge.hip) behind the probes
        if (!SLAB && tid < MPH_GAUGE_CHANNELS * M.ngauge)
            out[MPH_MONITOR_HEAD + 6 * M.ntrack + 2 * M.nprobe + tid] = M.gau[tid];
    }
    __syncthreads();   // every thread has read the counters
    if (tid == 0) {
        M.counters[0] = step;
        if (sampled) M.counters[1] += 1;
    }
    // (and the tracked rows: a particle that has left the rank leaves no row behind)
    if (SLAB && sampled && tid < kDistMonRow * MPH_MONITOR_MAX_TRACK) M.trk[tid] = 0.0;
}

void launch_monitor(const Launch& L, const MonitorDev& M)
{
    const DevParams& P = *L.P;
    const int n = P.n;
    if (n == 0) return;
    const int nb = monitor_blocks(n);
    launch(L.prof, "monitor_partial", L.stream, k_monitor_partial<false>, dim3(nb), dim3(kMonThreads), P, M, n, L.B,
           L.pres);
    if (M.nprobe > 0)
        by_dim(P.dim, [&](auto D) {
            launch(L.prof, "monitor_probe", L.stream, k_monitor_probe<decltype(D)::value, false>, dim3(M.nprobe),
                   dim3(64), P, M, n, L.A, L.start, L.pres);
        });
    if (M.ngauge > 0) launch_monitor_gauge(L, M);
    launch(L.prof, "monitor_final", L.stream, k_monitor_final<false>, dim3(1), dim3(kMonFinalThreads), M, nb, L.st);
}

// A slab rank's record of the step that has just run on L (mph_dist_monitor_configure): the same
// three launches in their slab forms.  The grids are sized for the capacity L.P->n (at least one
// block); the kernels read the live count.  k_monitor_final, the only writer of the counters, runs on
// every step, whatever the rank holds.
void launch_dist_monitor(const Launch& L, const MonitorDev& M)
{
    const DevParams& P = *L.P;
    const int n = P.n, nb = std::max(monitor_blocks(n), 1);
    launch(L.prof, "monitor_partial", L.stream, k_monitor_partial<true>, dim3(nb), dim3(kMonThreads), P, M, n, L.B,
           L.pres);
    if (M.nprobe > 0)
        by_dim(P.dim, [&](auto D) {
            launch(L.prof, "monitor_probe", L.stream, k_monitor_probe<decltype(D)::value, true>, dim3(M.nprobe),
                   dim3(64), P, M, n, L.A, L.start, L.pres);
        });
    launch(L.prof, "monitor_final", L.stream, k_monitor_final<true>, dim3(1), dim3(kMonFinalThreads), M, nb, L.st);
}

}  // namespace mph
