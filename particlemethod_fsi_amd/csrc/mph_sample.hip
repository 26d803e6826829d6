// mph_sample.hip -- lattice sampling (include/mph_gpu.h mph_sample_grid): the monitors' probe at
// every point of an axis-aligned lattice, on demand.  k_monitor_probe gives a whole wavefront to one
// point, right for 64 probes; here a lattice has up to 2^24 points, so every lane takes one point
// and walks the probe's stencil itself: the stencil columns in the probe's order, each column's one
// or two index ranges of start[] front to back.  A point's sums are therefore taken in an order
// fixed by the point and the state alone -- no atomics, no cross-lane reduction -- and its six
// values do not depend on the lattice around it or on the wave that holds it.
//
// Points to waves: a wave takes a tile of tile[0] x tile[1] x tile[2] lattice points (powers of
// two, product <= 64; sample_tiling): a run along the contiguous cell axis where the lattice has
// points along it -- its lanes share their stencil columns, which the wave then stages in LDS -- and
// otherwise (a slice across that axis) a tile as compact in space as the lattice allows, whose lanes
// walk nearly the same columns and read the same few lines of the 48-byte records, which the vector
// L1 then serves.  Points many cells apart (every lane in another region) or many to a cell change
// only which of the two ways a wave takes and what the caches see.  DESIGN.md section 11 has the
// measurements, with the version that only walks.
//
// On a slab rank (mph_dist_sample_grid, mph_dist_sample_grid_partial) the same kernel runs in its SLAB
// form over the runs of lattice planes the rank owns, one launch per run, on the rank's sorted set --
// owned particles and ghosts -- and its window grid: see k_sample_grid.
#include <hip/hip_runtime.h>

#include "mph_device.h"
#include "mph_kernels.h"
#include "mph_params.h"

namespace mph {

// The tile of one wave, from one point up to 64 by doubling: first along the contiguous cell axis
// `run_axis` while the lattice has more points along it than the tile (a run along it shares its
// stencil columns); then the axis whose tile is shortest in space (ties: the lower axis), likewise.
// A lattice of fewer than 64 points gets a smaller tile (the other lanes idle).
long long sample_tiling(SampleDev& G, int run_axis)
{
    for (int d = 0; d < 3; ++d) G.tile[d] = 1;
    int lanes = 1;
    for (; lanes < 64 && G.tile[run_axis] < G.count[run_axis]; lanes *= 2) G.tile[run_axis] *= 2;
    for (; lanes < 64; lanes *= 2) {
        int best = -1;
        for (int d = 0; d < 3; ++d)
            if (G.tile[d] < G.count[d] &&
                (best < 0 || G.tile[d] * G.spacing[d] < G.tile[best] * G.spacing[best]))
                best = d;
        if (best < 0) break;
        G.tile[best] *= 2;
    }
    long long total = 1;
    for (int d = 0; d < 3; ++d) {
        G.tiles[d] = (G.count[d] + G.tile[d] - 1) / G.tile[d];
        total *= G.tiles[d];
    }
    return total;
}

// A point's running sums, and one candidate's terms added to them; both kernels below add the same
// terms in the same order, so they give the same bits.
struct SampleAcc {
    double cnt = 0.0, sw = 0.0, swp = 0.0, sv0 = 0.0, sv1 = 0.0, sv2 = 0.0;
};

// the lane's lattice point: its indices and its position wrapped into the periodic domain like a
// particle (2-D: z is ignored); false for a lane without a point.  SLAB: G.count holds the planes of
// one run along the slab axis, the first of them plane `first` of the whole lattice: pt is the
// point's place in the run, its coordinates come from its indices in the whole lattice.
// (GRID: the kernel's own argument type, so that no copy of it is made)
template <bool SLAB, typename GRID>
__device__ __forceinline__ bool sample_point(const GRID& G, const DevParams& P, int dim, long long tile, int lane,
                                             int first, size_t& pt, double (&p)[3])
{
#pragma clang fp contract(off)
    const int t0 = (int)(tile % G.tiles[0]);
    const int t1 = (int)((tile / G.tiles[0]) % G.tiles[1]);
    const int t2 = (int)(tile / ((long long)G.tiles[0] * G.tiles[1]));
    const int i = t0 * G.tile[0] + lane % G.tile[0];
    const int j = t1 * G.tile[1] + (lane / G.tile[0]) % G.tile[1];
    const int l2 = lane / (G.tile[0] * G.tile[1]);
    const int k = t2 * G.tile[2] + l2;
    if (l2 >= G.tile[2] || i >= G.count[0] || j >= G.count[1] || k >= G.count[2]) return false;
    pt = ((size_t)k * G.count[1] + j) * G.count[0] + i;
    const int gi = SLAB && P.slab_axis == 0 ? i + first : i, gj = SLAB && P.slab_axis == 1 ? j + first : j;
    const int gk = SLAB && P.slab_axis == 2 ? k + first : k;
    const double q[3] = {G.origin[0] + (double)gi * G.spacing[0], G.origin[1] + (double)gj * G.spacing[1],
                         G.origin[2] + (double)gk * G.spacing[2]};
    wrap_point(P, dim, q, p);
    return true;
}

template <int DIM>
__device__ __forceinline__ void sample_term(SampleAcc& a, const DevParams& P, const double (&p)[3], double h, int mask,
                                            int t, double2 r0, double2 r1, double2 r2, double pj)
{
#pragma clang fp contract(off)
    if ((unsigned)t >= (unsigned)kTypes || !((mask >> (t >> 1)) & 1)) return;
    double w;
    if (shepard_weight<DIM>(P, p, h, r0.x, r0.y, r1.x, w)) {
        a.cnt += 1.0;
        a.sw += w;
        a.swp += w * pj;
        a.sv0 += w * r1.y;
        a.sv1 += w * r2.x;
        a.sv2 += w * r2.y;
    }
}

// the point's 48-byte record {COUNT, WSUM, P, VX, VY, VZ}; no contributor: zeros
__device__ __forceinline__ void sample_store(double2* __restrict__ out, size_t pt, const SampleAcc& a)
{
#pragma clang fp contract(off)
    const bool any = a.sw > 0.0;
    out[3 * pt] = make_double2(a.cnt, a.sw);
    out[3 * pt + 1] = make_double2(any ? a.swp / a.sw : 0.0, any ? a.sv0 / a.sw : 0.0);
    out[3 * pt + 2] = make_double2(any ? a.sv1 / a.sw : 0.0, any ? a.sv2 / a.sw : 0.0);
}

// component `axis` of three values, by selects on the values (a chain of conditional member reads
// becomes a runtime-indexed load, and the stencil then lives in scratch)
__device__ __forceinline__ int sample_ipick(int axis, int v0, int v1, int v2)
{
    return axis == 0 ? v0 : (axis == 1 ? v1 : v2);
}
// A slab rank's window grid is not periodic along the slab axis: a stencil is clipped at the window's
// two ends there instead of wrapped, as in k_monitor_probe<DIM, true> (a cell past an end would be one
// from the window's other end, not the domain's).  The slab axis the contiguous one: one clamped run.
template <int DIM>
__device__ __forceinline__ void sample_slab_clip(const DevParams& P, PointStencil<DIM>& S)
{
    if (P.slab_axis != S.ca) return;
    const int g = sample_ipick(P.slab_axis, P.gc[0], P.gc[1], P.gc[2]);
    const int cc = sample_ipick(P.slab_axis, S.c[0], S.c[1], S.c[2]);
    S.lo = max(cc - P.sa, 0);
    S.hi = min(cc + P.sa, g - 1);
    S.lo1 = 0;
    S.hi1 = -1;
}
// The slab axis a column axis: is column col's cell along it (its offset as PointStencil::column takes
// it) inside the window?
template <int DIM>
__device__ __forceinline__ bool sample_slab_column(const DevParams& P, const PointStencil<DIM>& S, int col)
{
    const int ax = P.slab_axis;
    if (ax == S.ca) return true;
    const int g = sample_ipick(ax, P.gc[0], P.gc[1], P.gc[2]);
    const int cc = sample_ipick(ax, S.c[0], S.c[1], S.c[2]);
    const int d = (ax == S.a0 ? (DIM == 3 ? col / kGroups : col) : col % kGroups) - kReach;
    return cc + d >= 0 && cc + d < g;
}

// a lane walks its point's whole stencil through global memory
template <int DIM, bool SLAB>
__device__ __forceinline__ void sample_walk(SampleAcc& acc, const DevParams& P, const PointStencil<DIM>& S,
                                            const double (&p)[3], double h, int mask, int n, const Soa& A,
                                            const int* __restrict__ start, const double* __restrict__ pres)
{
    for (int col = 0; col < PointStencil<DIM>::ncol; ++col) {
        if (SLAB && !sample_slab_column<DIM>(P, S, col)) continue;
        const int cell0 = S.column(P, col);
        for (int run = 0; run < 2; ++run) {
            if (run == 1 && S.hi1 < S.lo1) break;
            const int b = start[cell0 + (run ? S.lo1 : S.lo)];
            const int e = start[cell0 + (run ? S.hi1 : S.hi) + 1];
            for (int q = b < 0 ? 0 : b; q < e && q < n; ++q)
                sample_term<DIM>(acc, P, p, h, mask, A.type[q], A.p6[3 * (size_t)q], A.p6[3 * (size_t)q + 1],
                                 A.p6[3 * (size_t)q + 2], pres[q]);
        }
    }
}

// One wave per block.  Where the wave's points share their stencil columns -- the same cells across
// the column axes, no wrap along the contiguous one: a run of points along that axis, or many points
// in one cell -- each column's window, the union of the lanes' ranges, is staged in LDS 64 records
// at a time with coalesced loads, as k_neighbors stages its windows, and every lane tests its own
// sub-range of what is staged, in index order.  The lanes of any other wave walk their stencils
// themselves.  Both ways add the same terms in the same order.
// SLAB, a slab rank's planes (mph_dist_sample_grid_partial): one launch per run of planes the rank
// owns, G the run (SampleRunDev), out the run's points alone; n is the capacity and the live count is
// read here; A is the rank's sorted set, owned and ghosts, and the stencil is clipped at the window's
// ends along the slab axis in both ways through a wave.  The distance stays the minimum image.
constexpr int kSampleStage = 64;   // records staged at a time: one per lane
template <bool SLAB> struct SampleArg { using type = SampleDev; };
template <> struct SampleArg<true> { using type = SampleRunDev; };
template <int DIM, bool SLAB>
__global__ __launch_bounds__(64) void k_sample_grid(DevParams P, typename SampleArg<SLAB>::type G, int n, Soa A,
                                                    const int* __restrict__ start, const double* __restrict__ pres,
                                                    double2* __restrict__ out)
{
    __shared__ double2 s_r[3][kSampleStage];
    __shared__ double s_p[kSampleStage];
    __shared__ int s_t[kSampleStage];
    const int lane = threadIdx.x;
    const long long tile = blockIdx.x;
    size_t pt = 0;
    double p[3] = {0.0, 0.0, 0.0};
    if (SLAB) n = dev_n(P);
    int plane0 = 0;   // the run's first plane
    if constexpr (SLAB) plane0 = G.first;
    const bool active = sample_point<SLAB>(G, P, DIM, tile, lane, plane0, pt, p);
    if (!__any(active)) return;
    PointStencil<DIM> S(P, p);
    if (SLAB) sample_slab_clip<DIM>(P, S);
    SampleAcc acc;
    // the first active lane's column cells; do all active lanes share them, none wrapping along ca?
    const int first = __ffsll((unsigned long long)__ballot(active)) - 1;
    const int k0 = S.a0 == 0 ? S.c[0] : S.c[1], k1 = S.a1 < 0 ? 0 : (S.a1 == 1 ? S.c[1] : S.c[2]);
    const bool same = k0 == __shfl(k0, first, 64) && k1 == __shfl(k1, first, 64) && S.hi1 < S.lo1;
    if (!__all(same || !active)) {
        if (active) {
            sample_walk<DIM, SLAB>(acc, P, S, p, G.h, G.mask, n, A, start, pres);
            sample_store(out, pt, acc);
        }
        return;
    }
    // the window of the wave along ca
    int wlo = active ? S.lo : 0x7fffffff, whi = active ? S.hi : -1;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        wlo = min(wlo, __shfl_xor(wlo, m, 64));
        whi = max(whi, __shfl_xor(whi, m, 64));
    }
    // (every lane's stencil has the first active lane's column cells: inactive lanes take its whole
    // stencil so that column() is the same in all of them)
    PointStencil<DIM> W = S;
#pragma unroll
    for (int d = 0; d < 3; ++d) W.c[d] = __shfl(S.c[d], first, 64);
    for (int col = 0; col < PointStencil<DIM>::ncol; ++col) {
        if (SLAB && !sample_slab_column<DIM>(P, W, col)) continue;
        const int cell0 = W.column(P, col);
        const int wb = max(start[cell0 + wlo], 0), we = min(start[cell0 + whi + 1], n);
        int b = 0, e = 0;
        if (active) {
            b = max(start[cell0 + S.lo], 0);
            e = min(start[cell0 + S.hi + 1], n);
        }
        for (int base = wb; base < we; base += kSampleStage) {
            const int m = min(kSampleStage, we - base);
            __syncthreads();
            if (lane < m) {
                const size_t q = (size_t)(base + lane);
                s_r[0][lane] = A.p6[3 * q];
                s_r[1][lane] = A.p6[3 * q + 1];
                s_r[2][lane] = A.p6[3 * q + 2];
                s_p[lane] = pres[q];
                s_t[lane] = A.type[q];
            }
            __syncthreads();
            const int qe = min(e, base + m);
            for (int q = max(b, base); q < qe; ++q) {
                const int t = q - base;
                sample_term<DIM>(acc, P, p, G.h, G.mask, s_t[t], s_r[0][t], s_r[1][t], s_r[2][t], s_p[t]);
            }
        }
    }
    if (active) sample_store(out, pt, acc);
}

void launch_sample_grid(const Launch& L, const SampleDev& G, double* out)
{
    const DevParams& P = *L.P;
    const long long ntiles = (long long)G.tiles[0] * G.tiles[1] * G.tiles[2];
    by_dim(P.dim, [&](auto D) {
        launch(L.prof, "sample_grid", L.stream, k_sample_grid<decltype(D)::value, false>, dim3((unsigned)ntiles),
               dim3(64), P, G, P.n, L.A, L.start, L.pres, (double2*)out);
    });
}

void launch_dist_sample_grid(const Launch& L, const SampleRunDev& G, double* out)
{
    const DevParams& P = *L.P;
    const long long ntiles = (long long)G.tiles[0] * G.tiles[1] * G.tiles[2];
    by_dim(P.dim, [&](auto D) {
        launch(L.prof, "dist_sample_grid", L.stream, k_sample_grid<decltype(D)::value, true>, dim3((unsigned)ntiles),
               dim3(64), P, G, P.n, L.A, L.start, L.pres, (double2*)out);
    });
}

}  // namespace mph
