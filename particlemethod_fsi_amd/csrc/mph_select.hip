// mph_select.hip -- particle selections (include/mph_gpu.h mph_select*): a subset of the particles
// built on the device on demand -- the selected original indices, ascending, with each one's place in
// the sorted arrays -- then any field gathered for the subset alone, and sums and extrema over it.
// Every launch goes through launch(prof, ...) on the context's stream, outside every step graph; no
// kernel of a step is touched.
//
//   k_sel_flag            over the sorted arrays: flag[i] (the shared predicate sel_accepts, or the
//                         host's bit mask for a box on InitialPosition) and the two maps i -> q.
//                         The slab form (mph_dist_select) runs over the slots a rank holds, skips its
//                         ghosts and indexes flag and the maps by the whole problem's original index;
//                         only owned indices are visited, so k_sel_clear zeroes the flags before it
//   k_sel_count           selected per block of kSelBlock original indices
//   k_sel_scan_blocks     one block: exclusive scan of the block counts, and the count
//   k_sel_fill            ids[r] = i, slot_a[r], slot_b[r]: each block scans its own flags again and
//                         starts at its offset -- a two-level scan, no hand-off between workgroups
//   k_sel_gather          out[r][e] = src_e[slot[r] stride]
//   k_sel_totals_partial  one record per block of kSelBlock ranks; k_sel_totals_final adds the
//                         records in order.  No floating-point atomics: the totals are a function of
//                         the state, the selection and the centre alone, bit for bit.
#include <hip/hip_runtime.h>

#include "mph_device.h"
#include "mph_kernels.h"
#include "mph_params.h"

namespace mph {

constexpr int kSelThreads = 256;
constexpr int kSelItems = 4;                         // indices (ranks) per thread
constexpr int kSelBlock = kSelThreads * kSelItems;   // per block
constexpr int kSelWaves = kSelThreads / 64;

int select_blocks(int n) { return blocks(n, kSelBlock); }
int select_total_blocks(int count) { return blocks(count, kSelBlock); }

// ------------------------------------------------------------------------------- flag, scan ---

// How many: the slots q the kernel visits (n) and the original indices i it may meet.  A single
// context holds every particle, so both are n; a slab rank holds n of the whole problem's ng.
template <bool SLAB> struct SelFlagN { int n; };
template <> struct SelFlagN<true> { int n, ng; };
__device__ __forceinline__ int sel_indices(const SelFlagN<false>& N) { return N.n; }
__device__ __forceinline__ int sel_indices(const SelFlagN<true>& N) { return N.ng; }

// SLAB: a ghost (id < 0) is skipped like any index out of range, and an index no slot holds keeps the
// flag k_sel_clear left
template <bool SLAB>
__global__ __launch_bounds__(kSelThreads) void k_sel_flag(SelFlagN<SLAB> N, int dim, MphSelection s, int with_mask, Soa X,
                                                          const int* __restrict__ a_id, SelectDev D)
{
    const int n = sel_indices(N);
    const int q = blockIdx.x * kSelThreads + threadIdx.x;
    if (q >= N.n) return;
    const int ia = a_id[q];
    if (ia >= 0 && ia < n) D.slot_a_of[ia] = q;
    const int i = X.id[q];
    if (i < 0 || i >= n) return;
    D.slot_b_of[i] = q;
    bool in;
    if (with_mask) {
        in = (D.mask[i >> 5] >> (i & 31)) & 1u;
    } else {
        const double x[3] = {X.x[q], X.y[q], X.z[q]};
        in = sel_accepts(s, dim, i, X.type[q], x);
    }
    D.flag[i] = in ? 1 : 0;
}

// flag[0, 4 n4) = 0 (the allocation is a whole number of int4)
__global__ __launch_bounds__(kSelThreads) void k_sel_clear(int n4, int4* __restrict__ flag)
{
    const int k = blockIdx.x * kSelThreads + threadIdx.x;
    if (k < n4) flag[k] = make_int4(0, 0, 0, 0);
}

// the four flags of thread t of block b: original indices b kSelBlock + 4 t + (0..3), 0 past n
__device__ __forceinline__ int4 sel_flags4(const int* __restrict__ flag, int n, int i0)
{
    if (i0 + 3 < n) return *reinterpret_cast<const int4*>(flag + i0);   // (i0 is a multiple of 4)
    int4 f = make_int4(0, 0, 0, 0);
    if (i0 < n) f.x = flag[i0];
    if (i0 + 1 < n) f.y = flag[i0 + 1];
    if (i0 + 2 < n) f.z = flag[i0 + 2];
    return f;
}

// inclusive scan of v over the block's threads (T threads, T / 64 <= 16 waves); *total: the block's sum
template <int T> __device__ __forceinline__ int sel_block_scan(int v, int* s_wave, int* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const int u = __shfl_up(incl, m, 64);
        if (lane >= m) incl += u;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < T / 64; ++w) {
        const int t = s_wave[w];
        before += w < wave ? t : 0;
        all += t;
    }
    __syncthreads();   // (s_wave may be written again by the caller's next round)
    *total = all;
    return incl + before;
}

__global__ __launch_bounds__(kSelThreads) void k_sel_count(int n, SelectDev D)
{
    __shared__ int s_wave[kSelWaves];
    const int4 f = sel_flags4(D.flag, n, blockIdx.x * kSelBlock + kSelItems * threadIdx.x);
    int total;
    (void)sel_block_scan<kSelThreads>(f.x + f.y + f.z + f.w, s_wave, &total);
    if (threadIdx.x == 0) D.bsum[blockIdx.x] = total;
}

// One block: bsum[b] <- the selected before block b, bsum[nb] <- the count.
constexpr int kSelScanThreads = 1024;
__global__ __launch_bounds__(kSelScanThreads) void k_sel_scan_blocks(int nb, int* __restrict__ bsum)
{
    __shared__ int s_wave[kSelScanThreads / 64];
    int carry = 0;
    for (int base = 0; base < nb; base += kSelScanThreads) {
        const int b = base + threadIdx.x;
        const int v = b < nb ? bsum[b] : 0;
        int total;
        const int incl = sel_block_scan<kSelScanThreads>(v, s_wave, &total);
        if (b < nb) bsum[b] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) bsum[nb] = carry;
}

__global__ __launch_bounds__(kSelThreads) void k_sel_fill(int n, SelectDev D)
{
    __shared__ int s_wave[kSelWaves];
    const int i0 = blockIdx.x * kSelBlock + kSelItems * threadIdx.x;
    const int4 f = sel_flags4(D.flag, n, i0);
    const int mine = f.x + f.y + f.z + f.w;
    int total;
    int r = D.bsum[blockIdx.x] + sel_block_scan<kSelThreads>(mine, s_wave, &total) - mine;
    const int fl[kSelItems] = {f.x, f.y, f.z, f.w};
#pragma unroll
    for (int k = 0; k < kSelItems; ++k) {
        if (!fl[k]) continue;
        if (r < D.count) {   // (always: the flags are the ones counted)
            const int i = i0 + k;
            D.ids[r] = i;
            D.slot_a[r] = D.slot_a_of[i];
            D.slot_b[r] = D.slot_b_of[i];
        }
        ++r;
    }
}

// count and scan over the n original indices of D.flag
static void select_scan(const Launch& L, int n, const SelectDev& D)
{
    const int nb = select_blocks(n);
    launch(L.prof, "sel_count", L.stream, k_sel_count, dim3(nb), dim3(kSelThreads), n, D);
    launch(L.prof, "sel_scan_blocks", L.stream, k_sel_scan_blocks, dim3(1), dim3(kSelScanThreads), nb, D.bsum);
}

void launch_select_scan(const Launch& L, const Soa& X, const MphSelection& s, bool with_mask, const SelectDev& D)
{
    const int n = L.P->n;
    launch(L.prof, "sel_flag", L.stream, k_sel_flag<false>, dim3(blocks(n, kSelThreads)), dim3(kSelThreads),
           SelFlagN<false>{n}, L.P->dim, s, with_mask ? 1 : 0, X, L.A.id, D);
    select_scan(L, n, D);
}

void launch_select_fill(const Launch& L, const SelectDev& D)
{
    const int n = L.P->n;
    launch(L.prof, "sel_fill", L.stream, k_sel_fill, dim3(select_blocks(n)), dim3(kSelThreads), n, D);
}

void launch_dist_select_scan(const Launch& L, int n, int n_glob, const Soa& X, const MphSelection& s, bool with_mask,
                             const SelectDev& D)
{
    const int n4 = blocks(n_glob, 4);
    launch(L.prof, "sel_clear", L.stream, k_sel_clear, dim3(blocks(n4, kSelThreads)), dim3(kSelThreads), n4,
           reinterpret_cast<int4*>(D.flag));
    if (n > 0)
        launch(L.prof, "sel_flag_slab", L.stream, k_sel_flag<true>, dim3(blocks(n, kSelThreads)), dim3(kSelThreads),
               SelFlagN<true>{n, n_glob}, L.P->dim, s, with_mask ? 1 : 0, X, L.A.id, D);
    select_scan(L, n_glob, D);
}

void launch_dist_select_fill(const Launch& L, int n_glob, const SelectDev& D)
{
    launch(L.prof, "sel_fill", L.stream, k_sel_fill, dim3(select_blocks(n_glob)), dim3(kSelThreads), n_glob, D);
}

// ----------------------------------------------------------------------------------- gather ---

template <typename T, int NC> struct GatherSrc { const T* p[NC]; };

template <typename T, int NC>
__global__ __launch_bounds__(kSelThreads) void k_sel_gather(GatherSrc<T, NC> S, int stride, const int* __restrict__ slot,
                                                            int count, T* __restrict__ out)
{
    const int r = blockIdx.x * kSelThreads + threadIdx.x;
    if (r >= count) return;
    const size_t q = (size_t)slot[r] * (size_t)stride;
    T v[NC];
#pragma unroll
    for (int e = 0; e < NC; ++e) v[e] = S.p[e][q];
#pragma unroll
    for (int e = 0; e < NC; ++e) out[(size_t)r * NC + e] = v[e];
}

template <typename T, int NC>
static void gather(const Launch& L, const char* name, const T* const* src, int stride, const int* slot, int count, T* out)
{
    GatherSrc<T, NC> S;
    for (int e = 0; e < NC; ++e) S.p[e] = src[e];
    launch(L.prof, name, L.stream, k_sel_gather<T, NC>, dim3(blocks(count, kSelThreads)), dim3(kSelThreads), S, stride,
           slot, count, out);
}

void launch_select_gather(const Launch& L, const double* const* src, int nc, int stride, const int* slot, int count,
                          double* out)
{
    if (count <= 0) return;
    if (nc == 1) gather<double, 1>(L, "sel_gather1", src, stride, slot, count, out);
    else if (nc == 3) gather<double, 3>(L, "sel_gather3", src, stride, slot, count, out);
    else gather<double, 9>(L, "sel_gather9", src, stride, slot, count, out);
}

void launch_select_gather_int(const Launch& L, const int* src, const int* slot, int count, int* out)
{
    if (count <= 0) return;
    const int* const s1[1] = {src};
    gather<int, 1>(L, "sel_gather_int", s1, 1, slot, count, out);
}

// ----------------------------------------------------------------------------------- totals ---

// How slot k of a record combines (MphTotalSlot): 0 sum, 1 min, 2 max; and its identity (VMAX2 of no
// particle is 0: v.v >= 0).
__host__ __device__ constexpr int sel_op(int k)
{
    return k < MPH_TOT_XMIN || k > MPH_TOT_VMAX2 ? 0 : (k == MPH_TOT_VMAX2 ? 2 : ((k - MPH_TOT_XMIN) % 2 == 0 ? 1 : 2));
}
__device__ __forceinline__ double sel_init(int k)
{
    return sel_op(k) == 0 || k == MPH_TOT_VMAX2 ? 0.0 : (sel_op(k) == 1 ? __builtin_inf() : -__builtin_inf());
}
__device__ __forceinline__ double sel_combine(int k, double a, double b)
{
#pragma clang fp contract(off)
    return sel_op(k) == 0 ? a + b : (sel_op(k) == 1 ? fmin(a, b) : fmax(a, b));
}

// a lane's accumulators: the sums are slots 0..14 (one pad), the minima X, Y, Z (one pad), the maxima
// X, Y, Z and VMAX2
constexpr int kSelSums = 16, kSelMins = 4, kSelMaxs = 4;
__host__ __device__ constexpr int sel_slot_min(int i) { return MPH_TOT_XMIN + 2 * i; }
__host__ __device__ constexpr int sel_slot_max(int i) { return i == 3 ? MPH_TOT_VMAX2 : MPH_TOT_XMAX + 2 * i; }

struct SelTotalsArgs {
    double mass[kTypes];
    double c[3];
};

// One record per block over its kSelBlock ranks: rank r's Position, Velocity and type from the set X
// at slot_b[r], its Force from the A-ordered array at slot_a[r].
__global__ __launch_bounds__(kSelThreads) void k_sel_totals_partial(SelTotalsArgs G, Soa X,
                                                                    const double4* __restrict__ force, SelectDev D,
                                                                    double* __restrict__ partial)
{
#pragma clang fp contract(off)
    __shared__ double s_mass[kTypes];
    __shared__ double s_red[kSelWaves][kSelTotals];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < kTypes) s_mass[tid] = G.mass[tid];
    __syncthreads();
    double x[kSelItems], y[kSelItems], z[kSelItems], vx[kSelItems], vy[kSelItems], vz[kSelItems];
    double4 f[kSelItems];
    int ty[kSelItems];
    const int base = blockIdx.x * kSelBlock + tid;
#pragma unroll
    for (int it = 0; it < kSelItems; ++it) {
        const int r = base + it * kSelThreads;
        ty[it] = -1;
        if (r < D.count) {
            const int qb = D.slot_b[r], qa = D.slot_a[r];
            x[it] = X.x[qb]; y[it] = X.y[qb]; z[it] = X.z[qb];
            vx[it] = X.vx[qb]; vy[it] = X.vy[qb]; vz[it] = X.vz[qb];
            ty[it] = X.type[qb] & 0xff;   // (>= 0: a selected rank always counts)
            f[it] = force[qa];
        }
    }
    double sum[kSelSums], mn[kSelMins], mx[kSelMaxs];
#pragma unroll
    for (int k = 0; k < kSelSums; ++k) sum[k] = 0.0;
#pragma unroll
    for (int k = 0; k < kSelMins; ++k) mn[k] = __builtin_inf();
#pragma unroll
    for (int k = 0; k < kSelMaxs; ++k) mx[k] = k == 3 ? 0.0 : -__builtin_inf();
#pragma unroll
    for (int it = 0; it < kSelItems; ++it) {
        if (ty[it] < 0) continue;
        const double m = ty[it] < kTypes ? s_mass[ty[it]] : 0.0;
        const double v2 = vx[it] * vx[it] + vy[it] * vy[it] + vz[it] * vz[it];
        const double d0 = x[it] - G.c[0], d1 = y[it] - G.c[1], d2 = z[it] - G.c[2];
        sum[MPH_TOT_COUNT] += 1.0;
        sum[MPH_TOT_MASS] += m;
        sum[MPH_TOT_PX] += m * vx[it];
        sum[MPH_TOT_PY] += m * vy[it];
        sum[MPH_TOT_PZ] += m * vz[it];
        sum[MPH_TOT_KE] += (0.5 * m) * v2;
        sum[MPH_TOT_FX] += f[it].x;
        sum[MPH_TOT_FY] += f[it].y;
        sum[MPH_TOT_FZ] += f[it].z;
        sum[MPH_TOT_TX] += d1 * f[it].z - d2 * f[it].y;
        sum[MPH_TOT_TY] += d2 * f[it].x - d0 * f[it].z;
        sum[MPH_TOT_TZ] += d0 * f[it].y - d1 * f[it].x;
        sum[MPH_TOT_MX] += m * x[it];
        sum[MPH_TOT_MY] += m * y[it];
        sum[MPH_TOT_MZ] += m * z[it];
        mn[0] = fmin(mn[0], x[it]); mx[0] = fmax(mx[0], x[it]);
        mn[1] = fmin(mn[1], y[it]); mx[1] = fmax(mx[1], y[it]);
        mn[2] = fmin(mn[2], z[it]); mx[2] = fmax(mx[2], z[it]);
        mx[3] = fmax(mx[3], v2);
    }
    const double ws = mon_wave_fold<0>(sum), wn = mon_wave_fold<1>(mn), wx = mon_wave_fold<2>(mx);
    if (tid < kSelWaves * 2) s_red[tid >> 1][MPH_TOT_RESERVED0 + (tid & 1)] = 0.0;
    if (lane < MPH_TOT_XMIN) s_red[wave][lane] = ws;
    if (lane < 3) s_red[wave][sel_slot_min(lane)] = wn;
    if (lane < kSelMaxs) s_red[wave][sel_slot_max(lane)] = wx;
    __syncthreads();
    if (tid < kSelTotals) {
        double v = s_red[0][tid];
        for (int w = 1; w < kSelWaves; ++w) v = sel_combine(tid, v, s_red[w][tid]);
        partial[(size_t)blockIdx.x * kSelTotals + tid] = v;
    }
}

// One block: the nb records combined in a fixed order (as k_monitor_final): thread (g, k) of 32 groups
// of 32 takes slot k of the records g, g + 32, ..., then thread k the 32 groups' results in order.
constexpr int kSelFinalThreads = 1024, kSelGroups = kSelFinalThreads / 32;
__global__ __launch_bounds__(kSelFinalThreads) void k_sel_totals_final(const double* __restrict__ partial, int nb,
                                                                      double* __restrict__ out)
{
#pragma clang fp contract(off)
    __shared__ double s_red[kSelGroups][kSelTotals];
    const int tid = threadIdx.x, g = tid >> 5, k = tid & 31;
    if (k < kSelTotals) {
        double a = sel_init(k);
        for (int b = g; b < nb; b += kSelGroups) a = sel_combine(k, a, partial[(size_t)b * kSelTotals + k]);
        s_red[g][k] = a;
    }
    __syncthreads();
    if (tid < kSelTotals) {
        double v = s_red[0][tid];
        for (int w = 1; w < kSelGroups; ++w) v = sel_combine(tid, v, s_red[w][tid]);
        out[tid] = v;
    }
}

void launch_select_totals(const Launch& L, const Soa& X, const SelectDev& D, const double* center, double* partial,
                          double* out)
{
    SelTotalsArgs G;
    for (int t = 0; t < kTypes; ++t) G.mass[t] = L.P->mass[t];
    for (int d = 0; d < 3; ++d) G.c[d] = center[d];
    const int nb = select_total_blocks(D.count);
    if (nb > 0)
        launch(L.prof, "sel_totals_partial", L.stream, k_sel_totals_partial, dim3(nb), dim3(kSelThreads), G, X, L.force,
               D, partial);
    launch(L.prof, "sel_totals_final", L.stream, k_sel_totals_final, dim3(1), dim3(kSelFinalThreads), partial, nb, out);
}

}  // namespace mph
