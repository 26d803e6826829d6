// mph_sort.hip -- the counting sort into cell order that opens every step (mph_kernels.h has the
// step-to-launch map): k_prep, the histogram's exclusive scan, k_place, k_rank_scatter.
#include "mph_device.h"

namespace mph {

// ------------------------------------------------------------------------- sort phase -------

constexpr int kScanThreads = 256;
#ifndef MPH_SCAN_ITEMS
#define MPH_SCAN_ITEMS 16
#endif
constexpr int kScanItems = MPH_SCAN_ITEMS;   // cells per thread (a multiple of 4)
constexpr int kScanBlock = kScanThreads * kScanItems;   // 4096 cells per block
// ints of the scan's block totals (mph_create.hip allocates them)
__host__ __device__ inline int bsum_stride(int ncell) { return ncell / kScanBlock + 2; }
static_assert(kScanBlock == 4096, "mph_create.hip sizes the bsum buffer for 4096-cell blocks");

// The XCD split of the list passes (see list_block) from the search's work histogram: an inclusive
// scan of the runs' work (kXcdSegs / blockDim.x consecutive runs per thread), the 7 inner cut
// points at equal shares of the total (interpolated inside their run), then the histogram cleared.
// Block 0 of the next step's k_rank_scatter calls it (see there).
// seg / fr: the histogram and the map it becomes (DevState: seg_work or a lazy step's seg_lwork ->
// xcd_frac; a lazy step's seg_swork -> xcd_sfrac).
template <int T>
__device__ __forceinline__ void xcd_split_block(int* seg, int* fr)
{
    constexpr int R = kXcdSegs / T;
    static_assert(kXcdSegs % T == 0, "whole runs per thread");
    __shared__ long long s[T];
    const int t = threadIdx.x;
    long long sum = 0;
    for (int r = 0; r < R; ++r) sum += max(seg[t * R + r], 0);
    s[t] = sum;
    __syncthreads();
    for (int o = 1; o < T; o <<= 1) {
        const long long v = t >= o ? s[t - o] : 0;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    const long long tot = s[T - 1];
    if (tot < 8) {
        if (t < 9) fr[t] = 8192 * t;
    } else {
        for (int x = 1; x < 8; ++x) {
            const long long tgt = tot * x / 8;
            long long prev = t ? s[t - 1] : 0;
            if (!(prev < tgt && s[t] >= tgt)) continue;
            for (int r = 0; r < R; ++r) {
                const int w = max(seg[t * R + r], 0);
                if (w > 0 && prev < tgt && prev + w >= tgt) {
                    const double f = (t * R + r + (double)(tgt - prev) / (double)w) / kXcdSegs;
                    fr[x] = min(65536, max(0, (int)(f * 65536.0 + 0.5)));
                }
                prev += w;
            }
        }
        if (t == 0) {
            fr[0] = 0;
            fr[8] = 65536;
        }
    }
    __syncthreads();   // every thread has read its runs
    for (int r = 0; r < R; ++r) seg[t * R + r] = 0;
    __syncthreads();   // (a second split may follow: the scan's LDS is free again)
}

// calculateWall (main.cpp:3031-3060) + calculatePeriodicBoundary (3322-3333) + cell histogram.
// mode 0: initialisation (no motion), 1: time step, 2: time step whose motion was already applied
// (slab mode, k_dist_prep).  cmap: a lazy wall step's coarse map of the non-wall particles
// (mph_params.h kCoarseShift), else null.  Held to 64 VGPRs (8 waves per SIMD) as before the map:
// without the hint the marking took it to 66 and 7 waves.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void k_prep(
    DevParams P, const DevState* __restrict__ st, Soa C, int* __restrict__ key, int* __restrict__ slot,
    int* __restrict__ cnt, int mode, VSrc vs, unsigned char* __restrict__ cmap)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = dev_n(P);
    Soa B = C;
    bool mig = false;
    const int b = p < n ? vsrc_entry(vs, C, p, B, mig) : p;
    {
        // the lanes past n stay for the run detection (prep_slot), with keys of their own
        const bool live = p < n;
        const int lane = threadIdx.x & 63;
        int k = -1 - lane;
        int occ = 0;
        if (live) {
            double x = B.x[b], y = B.y[b], z = B.z[b];
            if (mode == 1) move_and_wrap(P, st, B, b, x, y, z);
            // (the type is loaded only with the map set)
            k = prep_cell(P, st, x, y, z, &key[p], cmap, [&] { return !dev_is_wall(B.type[b]); }, occ);
        }
        const int s = prep_slot(k, live, cnt);
        if (live) slot[p] = s;
        // the block's face bits: OR-ed in LDS, then one device atomic per block, only for bits the
        // step's word does not hold yet (few blocks: the particles near a periodic face)
        __shared__ int s_occ;
        if (threadIdx.x == 0) s_occ = 0;
        __syncthreads();
        if (__ballot(occ != 0)) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) occ |= __shfl_xor(occ, o, 64);
            if (lane == 0) atomicOr(&s_occ, occ);
        }
        __syncthreads();
        if (threadIdx.x == 0 && s_occ) {
            int* w = const_cast<int*>(&st->seam_occ[st->seam_step & 1]);
            const int cur = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (s_occ & ~cur) atomicOr(w, s_occ);
        }
    }
}

// Exclusive scan of the cell histogram (constants above k_prep): block totals (k_scan_reduce), the
// top-level scan (inside k_scan_down up to kScanFusedTop blocks, else a
// k_scan_top launch) and the down-sweep.

__device__ __forceinline__ int block_exclusive_scan(int v, int* lds, int& total)
{
    // wave-level inclusive scan (64 lanes) + cross-wave via LDS
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) lds[wid] = x;
    __syncthreads();
    int wsum = 0;
    const int nw = blockDim.x >> 6;
    total = 0;
    for (int w = 0; w < nw; ++w) {
        const int s = lds[w];
        if (w < wid) wsum += s;
        total += s;
    }
    __syncthreads();
    return wsum + x - v;
}

// 16 consecutive counts of one thread: four 16-byte loads when the run is inside the array
// (cell arrays are 16-int aligned per thread), element loads at the tail.
__device__ __forceinline__ void load16(const int* __restrict__ a, int base, int n, int (&v)[kScanItems])
{
    if (base + kScanItems <= n) {
        const int4* q = reinterpret_cast<const int4*>(a + base);
#pragma unroll
        for (int k = 0; k < kScanItems / 4; ++k) {
            const int4 t = q[k];
            v[4 * k] = t.x; v[4 * k + 1] = t.y; v[4 * k + 2] = t.z; v[4 * k + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kScanItems; ++k) v[k] = base + k < n ? a[base + k] : 0;
    }
}

__global__ __launch_bounds__(kScanThreads) void k_scan_reduce(const int* __restrict__ cnt, int ncell,
                                                              int* __restrict__ bsum)
{
    __shared__ int lds[kScanThreads / 64];
    const int base = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    int v[kScanItems];
    load16(cnt, base, ncell, v);
    int s = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) s += v[k];
    int total;
    block_exclusive_scan(s, lds, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void k_scan_top(int* __restrict__ bsum, int nb)
{
    // each thread a run of R consecutive totals: its sum, one block scan of the sums, then the
    // run's exclusive prefixes (one round trip to memory instead of nb / blockDim.x of them)
    __shared__ int lds[16];
    const int t = threadIdx.x;
    const int R = (nb + (int)blockDim.x - 1) / (int)blockDim.x;
    const int b0 = min(nb, t * R), b1 = min(nb, b0 + R);
    int sum = 0;
#pragma unroll 8
    for (int b = b0; b < b1; ++b) sum += bsum[b];
    int total;
    int run = block_exclusive_scan(sum, lds, total);
#pragma unroll 8
    for (int b = b0; b < b1; ++b) {
        const int v = bsum[b];
        bsum[b] = run;
        run += v;
    }
}

// top: bsum holds the raw block totals and every block sums its predecessors' itself (no
// k_scan_top launch; used while the block count is small, kScanFusedTop)
#ifndef MPH_SCAN_FUSED_TOP
#define MPH_SCAN_FUSED_TOP 8192   // (the D16M / 8 slab ranks: no k_scan_top launch)
#endif
constexpr int kScanFusedTop = MPH_SCAN_FUSED_TOP;
__global__ __launch_bounds__(kScanThreads) void k_scan_down(int* __restrict__ cnt, int ncell,
                                                            const int* __restrict__ bsum,
                                                            int* __restrict__ start, int n,
                                                            const int* __restrict__ n_dev, int top)
{
    __shared__ int lds[kScanThreads / 64];
    const int base = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    int v[kScanItems];
    load16(cnt, base, ncell, v);
    int pre = 0;
    if (top) {
        int t = 0;
        for (int b = threadIdx.x; b < (int)blockIdx.x; b += kScanThreads) t += bsum[b];
        block_exclusive_scan(t, lds, pre);
    } else {
        pre = bsum[blockIdx.x];
    }
    int s = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) s += v[k];
    int total;
    int run = block_exclusive_scan(s, lds, total) + pre;
    int o[kScanItems];
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        o[k] = run;
        run += v[k];
    }
    if (base + kScanItems <= ncell) {
        int4* st = reinterpret_cast<int4*>(start + base);
        int4* ct = reinterpret_cast<int4*>(cnt + base);
#pragma unroll
        for (int k = 0; k < kScanItems / 4; ++k) {
            st[k] = make_int4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
            // histogram ready for the next step; all-zero runs of 16 cells (most of the D1M tank is
            // empty, ~7 cells per particle) are left alone, so their lines are not written
            if (s != 0) ct[k] = make_int4(0, 0, 0, 0);
        }
    } else {
#pragma unroll
        for (int k = 0; k < kScanItems; ++k)
            if (base + k < ncell) {
                start[base + k] = o[k];
                if (v[k] != 0) cnt[base + k] = 0;
            }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) start[ncell] = n_dev ? *n_dev : n;
}

// Unordered placement; block 0 also advances Time and WallCenter (main.cpp:685, 3066-3070)
// after k_prep consumed them.  prep: a step (mode 1) that opened with k_prep, counted for
// mph_key_fold_stats -- 0 where the previous step's pass B left the keys (StepForm.keys_done).
__global__ __launch_bounds__(256) void k_place(DevParams P, DevState* __restrict__ st,
                                               const int* __restrict__ key, const int* __restrict__ slot,
                                               const int* __restrict__ start, int* __restrict__ tmp,
                                               int mode, int prep)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // this step's face bits are complete (k_prep): the searches read them; the next step's
        // k_prep gathers into the other word
        st->seam_occ[(st->seam_step + 1) & 1] = 0;
        st->seam_step += 1;
        if (mode) {
#pragma clang fp contract(off)
            for (int t = 4; t < 6; ++t)
                for (int d = 0; d < 3; ++d) st->wall_c[t][d] += st->wall_vel[t][d] * P.dt;
            st->time += P.dt;
        }
        if (prep) st->prep_steps += 1;
    }
    const int n = dev_n(P);
    if (p >= n) return;
    // a histogram inconsistent with the keys (it cannot happen while the block totals and the
    // counts agree) becomes an error flag, never a store out of range
    const int d = start[key[p]] + slot[p];
    if ((unsigned)d >= (unsigned)n) {
        atomicOr(&st->overflow, 64);
        return;
    }
    tmp[d] = p;
}

// Deterministic stable order inside a cell: rank = number of cell-mates with a smaller previous
// sorted index.  Reorders the persistent particle state into the new cell order.
__global__ __launch_bounds__(256) void k_rank_scatter(DevParams P, const int* __restrict__ key,
                                                      const int* __restrict__ start,
                                                      const int* __restrict__ tmp, Soa C, Soa A,
                                                      int* __restrict__ rank_of, int* __restrict__ dst_of,
                                                      int mode, VSrc vs, DevState* __restrict__ st, int split)
{
    // The passes' XCD split (list_block) runs here, in block 0 of the longest sort kernel, from
    // the previous step's search: a wave's work changes little from one step to the next and the
    // map only decides which block runs which wave, so no launch of its own sits between the
    // search and pass A (its own launch after the search cost 0.45 % at rest, 0.24 % developed,
    // profiles/r05/split_in_sort/)
    // (split 2, a lazy step: the histograms its own kind of step fed last, and its search's map)
    if (split && blockIdx.x == 0) {
        xcd_split_block<256>(split == 2 ? st->seg_lwork : st->seg_work, st->xcd_frac);
        if (split == 2) xcd_split_block<256>(st->seg_swork, st->xcd_sfrac);
    }
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= dev_n(P)) return;
    const int k = key[p];
    const int s = start[k], e = start[k + 1];
    int r = 0;
    for (int q = s; q < e; ++q) r += tmp[q] < p;
    const int dst = s + r;
    Soa B;
    bool mig;
    const int b = vsrc_entry(vs, C, p, B, mig);
    A.x[dst] = B.x[b];
    A.y[dst] = B.y[b];
    A.z[dst] = B.z[b];
    // the sorted velocities are read only through the 48-byte records (own_velocity), except at a
    // slab context's initialisation sort (mode 0: dist_init copies the sorted set into B)
    if (dst_of && mode == 0) {
        A.vx[dst] = B.vx[b];
        A.vy[dst] = B.vy[b];
        A.vz[dst] = B.vz[b];
    }
    A.type[dst] = B.type[b];
    const int id = mig ? -1 - B.id[b] : B.id[b];
    A.id[dst] = id;
    A.p6[3 * (size_t)dst] = make_double2(B.x[b], B.y[b]);
    A.p6[3 * (size_t)dst + 1] = make_double2(B.z[b], B.vx[b]);
    A.p6[3 * (size_t)dst + 2] = make_double2(B.vy[b], B.vz[b]);
    A.f4[dst] = make_float4((float)(B.x[b] - P.cref[0]), (float)(B.y[b] - P.cref[1]),
                            (float)(B.z[b] - P.cref[2]), __int_as_float(B.type[b]));
    if (dst_of) dst_of[p] = dst;   // slab mode: ids are global (ghosts negative)
    else if (rank_of) rank_of[id] = dst;
}

// ---------------------------------------------------------------------------- launchers -----

void launch_scan(int* cnt, int ncell, int* bsum, int* start, int total, const int* n_dev, hipStream_t stream,
                 Profiler* prof)
{
    const int nb = blocks(ncell, kScanBlock);
    const int top = nb <= kScanFusedTop;
    launch(prof, "scan_reduce", stream, k_scan_reduce, dim3(nb), dim3(kScanThreads), cnt, ncell, bsum);
    if (!top) launch(prof, "scan_top", stream, k_scan_top, dim3(1), dim3(1024), bsum, nb);
    launch(prof, "scan_down", stream, k_scan_down, dim3(nb), dim3(kScanThreads), cnt, ncell, bsum, start, total,
           n_dev, top);
}

void launch_sort(const Launch& L, int mode)
{
    const DevParams& P = *L.P;
    const int n = P.n;
    if (n == 0) return;
    // the passes' XCD split (list_grid, k_rank_scatter): 0 none, 1 a full step's, 2 a lazy step's
    const int split = lazy_bal(L) ? 2 : xcd_bal(L);
    const dim3 g(blocks(n, 256)), b(256);
    // keys_done (seq_step): the previous step's pass B has done k_prep's work
    const bool prep = !(mode == 1 && L.form.keys_done);
    if (prep)
        launch(L.prof, "prep", L.stream, k_prep, g, b, P, L.st, L.B, L.key, L.slot, L.cnt, mode, L.vsrc,
               lazy_cmap(L));
    launch_scan(L.cnt, P.ncell, L.bsum, L.start, n, P.n_dev, L.stream, L.prof);
    launch(L.prof, "place", L.stream, k_place, g, b, P, L.st, L.key, L.slot, L.start, L.tmp, mode,
           (int)(prep && mode == 1));
    launch(L.prof, "rank_scatter", L.stream, k_rank_scatter, g, b, P, L.key, L.start, L.tmp, L.B, L.A,
           nullptr /* rank_of: no reader (fields return through A.id, slab mode uses dst_of) */, L.dst_of, mode,
           L.vsrc, L.st, split);
}

}  // namespace mph
