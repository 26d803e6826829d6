// mph_gauge.hip -- free-surface gauges (include/mph_gpu.h mph_gauge_*): the fluid particles within a
// radius of a straight line parallel to a coordinate axis, reduced to the line's record {COUNT, TOP,
// BOTTOM, WET}.  One routine, gauge_line, and two kernels around it: k_monitor_gauge writes the
// gauges of the per-step monitors (launched by launch_monitor between the probe kernel and
// k_monitor_final), k_gauge_grid an elevation map over a lattice of lines on demand
// (mph_gauge_grid).  Both take the particles from the last step's sorted set A through that step's
// start[], like k_monitor_probe and k_sample_grid.
//
// One wavefront per line.  The four channels are an integer count, a maximum, a minimum and the
// population of a bit set (one bit per bin of particle_spacing along the line, in the wave's LDS), so
// they do not depend on the order the wave meets the particles in: a record is a function of the
// state, the line and the radius alone, bit for bit, whichever kernel computes it.  No global
// atomics, no floating-point atomics.
//
// On a slab rank (mph_dist_gauge_grid, mph_dist_gauge_grid_partial) gauge_line and k_gauge_grid run in
// their SLAB forms and leave the rank's record {COUNT, TOP, BOTTOM, WET, LOBIN, HIBIN} of a line;
// mph_gauge_combine (mph_observe.hip) makes the map of the ranks' records on the host.
#include <hip/hip_runtime.h>

#include "mph_device.h"
#include "mph_kernels.h"
#include "mph_params.h"

namespace mph {

constexpr int kGaugeWords = MPH_GAUGE_MAX_BINS / 32;   // a line's bit set: 1 KB of LDS
// a line's stencil columns, one lane each (gauge_line's contiguous form)
static_assert(kGroups * kGroups <= 64, "one lane per stencil column of a line");

// component `axis` of (v0, v1, v2), by selects (no runtime-indexed array)
__device__ __forceinline__ double gauge_pick(int axis, double v0, double v1, double v2)
{
    return axis == 0 ? v0 : (axis == 1 ? v1 : v2);
}

// (by value: a reference into the kernel's argument struct would make the compiler copy it to scratch)
__device__ __forceinline__ int gauge_ipick(int axis, int v0, int v1, int v2)
{
    return axis == 0 ? v0 : (axis == 1 ? v1 : v2);
}

// A wave's running record of one line; every lane holds its own share until gauge_line folds them.
struct GaugeAcc {
    int cnt = 0;
    double top = -__builtin_inf(), bot = __builtin_inf();
};

// A candidate of the sorted set A, of type t at (x, y, z): a fluid particle whose minimum-image
// distance r from the line through p along `axis` -- over the DIM - 1 other axes, lower axis first
// -- is below h joins the record and sets its bin's bit.  (t = -1: no candidate.)
template <int DIM>
__device__ __forceinline__ void gauge_term(GaugeAcc& acc, const DevParams& P, int t, double x, double y, double z,
                                           int axis, const double (&p)[3], double h, int nbins, unsigned* bits)
{
#pragma clang fp contract(off)
    if (t < 0 || t >= 2) return;
    // one across component: the minimum image of the particle's offset from the line along axis u
    const auto image = [&](int u) {
        return image_exact<false>(gauge_pick(u, x, y, z) - gauge_pick(u, p[0], p[1], p[2]),
                                  gauge_pick(u, P.dw[0], P.dw[1], P.dw[2]), gauge_pick(u, P.hw[0], P.hw[1], P.hw[2]),
                                  gauge_pick(u, P.w075[0], P.w075[1], P.w075[2]));
    };
    double r;
    if (DIM == 3) {
        // the across axes, lower first: (1, 2), (0, 2), (0, 1)
        const double q0 = image(axis == 0 ? 1 : 0), q1 = image(axis == 2 ? 1 : 2);
        r = sqrt(q0 * q0 + q1 * q1);
    } else {
        const double q0 = image(1 - axis);
        r = sqrt(q0 * q0);
    }
    if (!(r < h)) return;
    const double xa = gauge_pick(axis, x, y, z);
    acc.cnt += 1;
    acc.top = fmax(acc.top, xa);
    acc.bot = fmin(acc.bot, xa);
    // bin min(max((int)floor((xa - dmin) / dx), 0), nbins - 1), clamped before the conversion
    const double b = floor((xa - gauge_pick(axis, P.dmin[0], P.dmin[1], P.dmin[2])) / P.dx);
    const int bin = (int)fmin(fmax(b, 0.0), (double)(nbins - 1));
    atomicOr(&bits[bin >> 5], 1u << (bin & 31));
}

// The candidates j0, j0 + step, ... below je.  A line's walk is a chain of trips to memory, so
// kGaugeLoads candidates' loads -- type and position together -- are in flight before the first is
// tested (a candidate past je repeats j0's loads and counts as none).
// SLAB with `own` (a line parallel to the slab axis): only the particles the rank owns count, A.id >=
// 0, the test of k_monitor_partial<true>; a ghost counts as no candidate.
constexpr int kGaugeLoads = 4;
template <int DIM, bool SLAB>
__device__ __forceinline__ void gauge_range(GaugeAcc& acc, const DevParams& P, const Soa& A, int j0, int je, int step,
                                            int axis, const double (&p)[3], double h, int nbins, unsigned* bits,
                                            bool own)
{
    for (int j = j0; j < je; j += kGaugeLoads * step) {
        int t[kGaugeLoads];
        double x[kGaugeLoads], y[kGaugeLoads], z[kGaugeLoads];
#pragma unroll
        for (int u = 0; u < kGaugeLoads; ++u) {
            const bool ok = j + u * step < je;
            const int jc = ok ? j + u * step : j;
            const int tt = A.type[jc];
            t[u] = ok ? tt : -1;
            if (SLAB && own && A.id[jc] < 0) t[u] = -1;
            x[u] = A.x[jc];
            y[u] = A.y[jc];
            z[u] = DIM == 3 ? A.z[jc] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kGaugeLoads; ++u) gauge_term<DIM>(acc, P, t[u], x[u], y[u], z[u], axis, p, h, nbins, bits);
    }
}

// The stencil of a line across one axis d: the cells within `reach` of the line's cell cc, each once.
// n cells; cell i is at(i).  Where the stencil covers the whole axis (2 reach + 1 >= g, as the
// hi - lo + 1 >= g case of PointStencil) the cells are 0 .. g - 1; otherwise cc - reach + i, wrapped.
// clip (the slab axis of a slab rank's window grid, which is not periodic along it): the cells of
// cc - reach .. cc + reach inside 0 .. g - 1, none wrapped.
struct GaugeSpan {
    int n, first, g;
    __device__ __forceinline__ GaugeSpan(int cc, int reach, int g_, bool clip = false) : g(g_)
    {
        const bool whole = 2 * reach + 1 >= g_;
        n = whole ? g_ : 2 * reach + 1;
        first = whole ? 0 : cc - reach;
        if (clip) {
            first = max(cc - reach, 0);
            n = min(cc + reach, g_ - 1) - first + 1;
        }
    }
    __device__ __forceinline__ int at(int i) const { return wrap_cell(first + i, g); }
};

// The record of the line through `point` (wrapped into the periodic domain here) along `axis`, over
// the fluid particles of the sorted set A within h of it: {COUNT, TOP, BOTTOM, WET} in rec[0..3] of
// every lane.  Called by all 64 lanes of one wave per line, the block's waves together (two block
// barriers, at the same places for every line); bits: the wave's own kGaugeWords words of LDS.
//
// The cells of the line: the stencil columns within kReach cells across (P.sa along the contiguous
// cell axis ca) of the line's cell, over the whole extent of the grid along `axis`.
//   axis == ca: each column is one range of start[] over the full column; lane c loads column c's
//     range, then the wave streams the columns' particles, consecutive lanes consecutive indices.
//   axis != ca: ca is an across axis, so the cells of one cell index along `axis` and one offset
//     across the other axis are a run of 2 P.sa + 1 cells of start[], two where it wraps.  The
//     lanes take the runs.
// SLAB, a slab rank's record {COUNT, TOP, BOTTOM, WET, LOBIN, HIBIN} over its sorted set A on its
// window grid (n: the live count).  A line parallel to the slab axis runs through every rank: the rank
// counts the particles it owns alone, over the whole extent of its window along the axis.  Any other
// line is computed by the rank that owns its plane, over owned particles and ghosts; the slab axis is
// then an across axis, and its span -- the GaugeSpan, or the run along the contiguous axis -- is
// clipped at the window's two ends instead of wrapped, as in k_monitor_probe<DIM, true>.  LOBIN and
// HIBIN: the lowest and highest occupied bin, -1 with none (mph_gauge_combine's overlap term).
template <int DIM, bool SLAB>
__device__ __forceinline__ void gauge_line(const DevParams& P, const Soa& A, const int* __restrict__ start, int n,
                                           int axis, const double (&point)[3], double h, int nbins,
                                           unsigned* bits, double (&rec)[SLAB ? kDistGaugeRec : MPH_GAUGE_CHANNELS])
{
    const int lane = threadIdx.x & 63;
    const int nwords = (nbins + 31) >> 5;
    for (int w = lane; w < nwords; w += 64) bits[w] = 0u;
    __syncthreads();
    double p[3];
    wrap_point(P, DIM, point, p);
    const int g0 = P.gc[0], g1 = P.gc[1], g2 = P.gc[2];
    const int c0 = cell_axis(p[0], P.corg[0], P.dw[0], P.ginv[0], g0);
    const int c1 = cell_axis(p[1], P.corg[1], P.dw[1], P.ginv[1], g1);
    const int c2 = DIM == 3 ? cell_axis(p[2], P.corg[2], P.dw[2], P.ginv[2], g2) : 0;
    // the line's cell and the grid's extent along axis a
    const auto cell = [&](int a) { return gauge_ipick(a, c0, c1, c2); };
    const auto grid = [&](int a) { return gauge_ipick(a, g0, g1, g2); };
    const int ca = contig_axis(DIM, P.perm);
    // (sl: the slab axis where it is an across axis of the line, else -1)
    const bool own = SLAB && axis == P.slab_axis;
    const int sl = SLAB && !own ? P.slab_axis : -1;
    GaugeAcc acc;
    if (axis == ca) {
        // the across axes (a0, a1), both column axes; 2-D: a0 = 0 alone
        const int a0 = DIM == 3 ? (ca == 0 ? 1 : 0) : 0, a1 = DIM == 3 ? (ca == 2 ? 1 : 2) : -1;
        const GaugeSpan s0(cell(a0), kReach, grid(a0), SLAB && sl == a0);
        const GaugeSpan s1 = DIM == 3 ? GaugeSpan(cell(a1), kReach, grid(a1), SLAB && sl == a1) : GaugeSpan(0, 0, 1);
        const int ncol = s0.n * s1.n;
        int b = 0, e = 0;
        if (lane < ncol) {
            const int q0 = s0.at(lane / s1.n), q1 = s1.at(lane % s1.n);
            int q[3] = {0, 0, 0};
#pragma unroll
            for (int d = 0; d < 3; ++d) q[d] = d == a0 ? q0 : (d == a1 ? q1 : 0);
            const int cell0 = cell_index(P, q[0], q[1], q[2]);
            b = max(start[cell0], 0);
            e = min(start[cell0 + grid(ca)], n);
        }
        for (int col = 0; col < ncol; ++col) {
            const int cb = __shfl(b, col, 64), ce = __shfl(e, col, 64);
            gauge_range<DIM, SLAB>(acc, P, A, cb + lane, ce, 64, axis, p, h, nbins, bits, own);
        }
    } else {
        // the across axes: ca and, in 3-D, the third axis o
        const int o = DIM == 3 ? 3 - axis - ca : -1;
        const GaugeSpan so = DIM == 3 ? GaugeSpan(cell(o), kReach, grid(o), SLAB && sl == o) : GaugeSpan(0, 0, 1);
        // the run along ca, the same for every cell index along the line (PointStencil's ranges)
        const int cc = cell(ca), g = grid(ca);
        int lo = cc - P.sa, hi = cc + P.sa, lo1 = 0, hi1 = -1;
        if (SLAB && sl == ca) { lo = max(lo, 0); hi = min(hi, g - 1); }
        else if (hi - lo + 1 >= g) { lo = 0; hi = g - 1; }
        else if (lo < 0) { lo1 = lo + g; hi1 = g - 1; lo = 0; }
        else if (hi >= g) { lo1 = 0; hi1 = hi - g; hi = g - 1; }
        const int nrun = grid(axis) * so.n;
        for (int r = lane; r < nrun; r += 64) {
            const int m = r / so.n, qo = so.at(r % so.n);
            int q[3] = {0, 0, 0};
#pragma unroll
            for (int d = 0; d < 3; ++d) q[d] = d == axis ? m : (d == o ? qo : 0);
            const int cell0 = cell_index(P, q[0], q[1], q[2]);
            const int b0 = max(start[cell0 + lo], 0), e0 = min(start[cell0 + hi + 1], n);
            gauge_range<DIM, SLAB>(acc, P, A, b0, e0, 1, axis, p, h, nbins, bits, own);
            if (hi1 >= lo1) {
                const int b1 = max(start[cell0 + lo1], 0), e1 = min(start[cell0 + hi1 + 1], n);
                gauge_range<DIM, SLAB>(acc, P, A, b1, e1, 1, axis, p, h, nbins, bits, own);
            }
        }
    }
    __syncthreads();
    int wet = 0;
    // (SLAB) the lane's lowest and highest set bit: its words ascend, so the first one with a bit
    // gives the lowest and the last one the highest
    int lob = 0x7fffffff, hib = -1;
    for (int w = lane; w < nwords; w += 64) {
        const unsigned b = bits[w];
        wet += __popc(b);
        if (SLAB && b) {
            lob = min(lob, 32 * w + __ffs(b) - 1);
            hib = 32 * w + 31 - __clz(b);
        }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        acc.cnt += __shfl_xor(acc.cnt, m, 64);
        wet += __shfl_xor(wet, m, 64);
        acc.top = fmax(acc.top, __shfl_xor(acc.top, m, 64));
        acc.bot = fmin(acc.bot, __shfl_xor(acc.bot, m, 64));
        if (SLAB) {
            lob = min(lob, __shfl_xor(lob, m, 64));
            hib = max(hib, __shfl_xor(hib, m, 64));
        }
    }
    rec[0] = (double)acc.cnt;
    rec[1] = acc.top;
    rec[2] = acc.bot;
    rec[3] = (double)wet;
    if constexpr (SLAB) {
        rec[4] = hib < 0 ? -1.0 : (double)lob;
        rec[5] = (double)hib;
    }
}

// One wave per gauge of the monitors: M.gau[4 q ..] on a sampled step.
template <int DIM>
__global__ __launch_bounds__(64) void k_monitor_gauge(DevParams P, MonitorDev M, int n, Soa A,
                                                      const int* __restrict__ start)
{
    long long step;
    if (!mon_sampled(M, step)) return;
    __shared__ unsigned s_bits[kGaugeWords];
    const int q = blockIdx.x;
    const double point[3] = {M.gauges[3 * q], M.gauges[3 * q + 1], DIM == 3 ? M.gauges[3 * q + 2] : 0.0};
    double rec[4];
    gauge_line<DIM, false>(P, A, start, n, M.gauge_axis, point, M.gauge_h, M.gauge_nbins, s_bits, rec);
    if (threadIdx.x < MPH_GAUGE_CHANNELS) {
        const int k = threadIdx.x;
        M.gau[MPH_GAUGE_CHANNELS * q + k] = k == 0 ? rec[0] : (k == 1 ? rec[1] : (k == 2 ? rec[2] : rec[3]));
    }
}

// One wave per line of the lattice, W lines to a block (the last block's spare waves take its last
// line again and store nothing).  Line l = (k count[1] + j) count[0] + i passes through origin +
// (i, j, k) spacing, each product and sum rounded.
// SLAB, a slab rank's records (mph_dist_gauge_grid_partial): G is the rank's lines (GaugeRunDev: a run
// of the planes it owns, line l the l-th of the run and its point computed from its indices in the
// whole lattice; or, for lines parallel to the slab axis, the whole lattice), n the capacity -- the
// live count is read here -- and a record has kDistGaugeRec doubles.
template <bool SLAB> struct GaugeArg { using type = GaugeGridDev; };
template <> struct GaugeArg<true> { using type = GaugeRunDev; };
template <int DIM, int W, bool SLAB>
__global__ __launch_bounds__(64 * W) void k_gauge_grid(DevParams P, typename GaugeArg<SLAB>::type G, int n, Soa A,
                                                       const int* __restrict__ start, double* __restrict__ out)
{
#pragma clang fp contract(off)
    __shared__ unsigned s_bits[W][kGaugeWords];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int line = blockIdx.x * W + wave;
    const int l = min(line, G.nlines - 1);
    int i = l % G.count[0], j = (l / G.count[0]) % G.count[1], k = l / (G.count[0] * G.count[1]);
    if constexpr (SLAB) {
        n = dev_n(P);
        const int first = G.first;
        i += P.slab_axis == 0 ? first : 0;
        j += P.slab_axis == 1 ? first : 0;
        k += P.slab_axis == 2 ? first : 0;
    }
    const double point[3] = {G.origin[0] + (double)i * G.spacing[0], G.origin[1] + (double)j * G.spacing[1],
                             G.origin[2] + (double)k * G.spacing[2]};
    constexpr int R = SLAB ? kDistGaugeRec : MPH_GAUGE_CHANNELS;
    double rec[R];
    gauge_line<DIM, SLAB>(P, A, start, n, G.axis, point, G.h, G.nbins, s_bits[wave], rec);
    if (line < G.nlines && lane < R) {
        double v = lane == 0 ? rec[0] : (lane == 1 ? rec[1] : (lane == 2 ? rec[2] : rec[3]));
        if constexpr (SLAB) v = lane == 4 ? rec[4] : (lane == 5 ? rec[5] : v);
        out[(size_t)R * l + lane] = v;
    }
}

void launch_monitor_gauge(const Launch& L, const MonitorDev& M)
{
    const DevParams& P = *L.P;
    by_dim(P.dim, [&](auto D) {
        launch(L.prof, "monitor_gauge", L.stream, k_monitor_gauge<decltype(D)::value>, dim3(M.ngauge), dim3(64), P, M,
               P.n, L.A, L.start);
    });
}

void launch_gauge_grid(const Launch& L, const GaugeGridDev& G, double* out)
{
    const DevParams& P = *L.P;
    by_dim(P.dim, [&](auto D) {
        constexpr int DIM = decltype(D)::value;
        if (G.waves == 4)
            launch(L.prof, "gauge_grid", L.stream, k_gauge_grid<DIM, 4, false>, dim3((G.nlines + 3) / 4), dim3(256), P, G, P.n,
                   L.A, L.start, out);
        else
            launch(L.prof, "gauge_grid", L.stream, k_gauge_grid<DIM, 1, false>, dim3(G.nlines), dim3(64), P, G, P.n, L.A,
                   L.start, out);
    });
}

void launch_dist_gauge_grid(const Launch& L, const GaugeRunDev& G, double* out)
{
    const DevParams& P = *L.P;
    by_dim(P.dim, [&](auto D) {
        constexpr int DIM = decltype(D)::value;
        if (G.waves == 4)
            launch(L.prof, "dist_gauge_grid", L.stream, k_gauge_grid<DIM, 4, true>, dim3((G.nlines + 3) / 4), dim3(256),
                   P, G, P.n, L.A, L.start, out);
        else
            launch(L.prof, "dist_gauge_grid", L.stream, k_gauge_grid<DIM, 1, true>, dim3(G.nlines), dim3(64), P, G, P.n,
                   L.A, L.start, out);
    });
}

}  // namespace mph
