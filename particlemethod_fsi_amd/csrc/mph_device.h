// mph_device.h -- device helpers and the host-side launcher shared by the kernel translation units
// (mph_sort.hip, mph_search.hip, mph_passes.hip, mph_elastic.hip, mph_slab.hip, mph_monitor.hip,
// mph_sample.hip, mph_gauge.hip, mph_select.hip, mph_kinematics.hip): the reference's exact periodic arithmetic, the cell
// grid's indexing, buffer-descriptor loads, the type predicates, wave-level helpers, a particle's wall
// motion and wrap, the prep tail, the reductions' wave fold, the stencil around a point, and launch /
// blocks / by_dim / by_flag.  A helper used by one unit alone stays in that
// unit; the neighbour lists' layout is mph_list.h.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <climits>
#include <type_traits>

#include "mph_kernels.h"
#include "mph_params.h"

namespace mph {

// Mod(x,w) of main.cpp:98, exact (IEEE division, floor, no contraction).
__device__ __forceinline__ double mod_exact(double x, double w)
{
#pragma clang fp contract(off)
    return x - w * floor(x / w);
}

// Periodic minimum image Mod(d + w/2, w) - w/2 of every pair loop (e.g. main.cpp:1762), bit-
// identical to the reference.  For 0 <= s < 0.75 w, floor(s/w) == 0 exactly and
// Mod(s,w) == s - w*0 == s; FAST (wave-uniform, interior particles only) relies on that always.
template <bool FAST>
__device__ __forceinline__ double image_exact(double d, double w, double hw, double w075)
{
#pragma clang fp contract(off)
    const double s = d + hw;
    double m;
    if (FAST || __builtin_expect(s >= 0.0 && s < w075, 1)) {
        m = s;
    } else {
        m = s - w * floor(s / w);
    }
    return m - hw;
}

__device__ __forceinline__ int wrap_cell(int c, int g)
{
    c = c < 0 ? c + g : c;
    return c >= g ? c - g : c;
}

// Cell index along one axis.  The offset from the grid origin is wrapped once into [0, w) (w =
// periodic domain width), so a slab window that straddles the periodic seam (multi-GPU) sees its
// ghosts from the far side at the right place; for the full-domain grid the wrap changes nothing.
// Out-of-window offsets clamp into the edge cells (only far ghosts, never needed as neighbours).
__device__ __forceinline__ int cell_axis(double x, double org, double w, double ginv, int g)
{
    double u = x - org;
    u = u < 0.0 ? u + w : (u >= w ? u - w : u);
    // clamp before the conversion: a NaN / infinite coordinate (diverged input) maps to cell 0
    // instead of an undefined float->int conversion
    const double t = fmin(fmax(floor(u * ginv), 0.0), (double)(g - 1));
    return (int)t;
}

// linear cell index in the cell order DevParams.perm (order_axis; the last axis contiguous, with
// half-width cells)
__device__ __forceinline__ int cell_index(const DevParams& P, int cx, int cy, int cz)
{
    const int* g = P.gc;
    switch (P.perm) {
    case 1: return (cz * g[0] + cx) * g[1] + cy;   // (z, x, y)
    case 2: return (cz * g[1] + cy) * g[0] + cx;   // (z, y, x)
    case 3: return (cy * g[2] + cz) * g[0] + cx;   // (y, z, x)
    case 4: return (cx * g[2] + cz) * g[1] + cy;   // (x, z, y)
    default: return (cx * g[1] + cy) * g[2] + cz;  // (x, y, z)
    }
}

// Buffer descriptor of a device array (gfx9 raw-buffer format word, 4 GiB of records): loads through
// it take a 32-bit unsigned byte offset from a VGPR instead of a 64-bit address.  The cell table
// (ncell + 1 ints, checked at creation) and the particle arrays (< 2^28 entries) stay below 4 GiB.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t arr_rsrc(const void* p)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, -1, 0x00020000);
}
// a buffer descriptor over `bytes` bytes: loads past them return zeros without a memory access
__device__ __forceinline__ __amdgpu_buffer_rsrc_t sized_rsrc(const void* p, unsigned bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}
// 16 bytes at byte offset off of a buffer, as two doubles
__device__ __forceinline__ double2 buf_ld16(__amdgpu_buffer_rsrc_t r, unsigned off)
{
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    const u4 v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
    return __builtin_bit_cast(double2, v);
}

// ------------------------------------------------------------------------------ helpers ------

__device__ __forceinline__ double r2_exact(double q0, double q1, double q2)
{
#pragma clang fp contract(off)
    return q0 * q0 + q1 * q1 + q2 * q2;
}

// r = sqrt(r2) and 1/r from v_rsq_f64 plus one Newton step (relative error ~1e-16).
__device__ __forceinline__ void rsqrt_pair(double r2, double& r, double& ir)
{
    double y = __builtin_amdgcn_rsq(r2);
    const double e = fma(-(r2 * y), y, 1.0);
    y = fma(0.5 * y, e, y);
    ir = y;
    r = r2 * y;
}

__device__ __forceinline__ int cell_id(const DevParams& P, double x, double y, double z)
{
    const int cx = cell_axis(x, P.corg[0], P.dw[0], P.ginv[0], P.gc[0]);
    const int cy = cell_axis(y, P.corg[1], P.dw[1], P.ginv[1], P.gc[1]);
    const int cz = P.dim == 3 ? cell_axis(z, P.corg[2], P.dw[2], P.ginv[2], P.gc[2]) : 0;
    return cell_index(P, cx, cy, cz);
}

// byte of coarse cell (qx, qy, qz) in the coarse map of the non-wall particles (mph_params.h
// kCoarseShift; (x, y, z) order whatever the cell order)
__device__ __forceinline__ int coarse_index(const DevParams& P, int qx, int qy, int qz)
{
    return (qx * coarse_cells(P.gc[1]) + qy) * coarse_cells(P.gc[2]) + qz;
}

__device__ __forceinline__ bool dev_is_struct(int t) { return t == 2 || t == 3; }
__device__ __forceinline__ bool dev_is_fluid(int t) { return t == 0 || t == 1; }
__device__ __forceinline__ bool dev_is_wall(int t) { return t == 4 || t == 5; }

// wave-uniform, for the fast paths of the search and of the passes: every live lane is >= 3 cells
// inside the cell grid's faces (so no stencil row wraps) and, on every axis with particles near BOTH periodic faces (this step's
// seam_occ) or on the slab axis, also >= 3 cells from the domain's faces (so no candidate pair
// straddles the periodic seam and the raw differences are the minimum image).  With the grid
// origin at dmin that is >= 3 cells from every periodic face; with the origin in an empty band it
// also admits the waves at a wall on a periodic face whose far side is empty (the dam's bottom wall).
__device__ __forceinline__ bool wave_search_interior(const DevParams& P, const DevState* st, bool live,
                                                     double x, double y, double z)
{
    const int occ = st->seam_occ[(st->seam_step - 1) & 1];
    const double v[3] = {x, y, z};
    bool in = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (k == 2 && P.dim == 2) break;
        double u = v[k] - P.corg[k];
        u = u < 0.0 ? u + P.dw[k] : (u >= P.dw[k] ? u - P.dw[k] : u);
        in = in && u >= P.sinner_lo[k] && u <= P.sinner_hi[k];
        const bool seam = ((P.seam_always >> k) & 1) || ((occ >> (2 * k)) & 3) == 3;
        if (seam) in = in && v[k] >= P.inner_lo[k] && v[k] <= P.inner_hi[k];
    }
    return P.fast_ok && __all(!live || in);
}

// XCD-aware block order: hardware deals consecutive blocks round-robin over the 8 XCDs; remap so
// that each XCD sweeps one contiguous 1/8 of the (cell-sorted) particles and neighbour gathers
// hit its own L2 (cdna_hip_programming.md T1, bijective form).
__device__ __forceinline__ int xcd_block(int b, int nb)
{
    const int xcd = b & 7;
    const int q = nb >> 3, r = nb & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
}

// Particles held by this context: exact on a single GPU; in slab mode the device-resident count
// of the last redistribution (P.n is then only the capacity the grids are sized for).
__device__ __forceinline__ int dev_n(const DevParams& P) { return P.n_dev ? *P.n_dev : P.n; }

// Blocks of 256 that hold live particles; the rest of a capacity-sized grid exits at once.  The
// XCD remap runs over the live blocks only, so the work stays spread over all 8 XCDs.
__device__ __forceinline__ int live_blocks(int n) { return (n + 255) >> 8; }

// Wave-wide min / max (result in every lane).  DPP form: shifts within 16-lane rows, then
// row_bcast:15 / :31 carry the partial results across rows (gfx9 family), lane 63 holds the
// total; 7 dependent VALU steps instead of 6 dependent LDS permutes.
template <bool MAX>
__device__ __forceinline__ int wave_reduce_dpp(int v)
{
    const int id = MAX ? INT_MIN : INT_MAX;
    auto op = [](int a, int b) { return MAX ? max(a, b) : min(a, b); };
    v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x111, 0xf, 0xf, false));   // row_shr:1
    v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x112, 0xf, 0xf, false));   // row_shr:2
    v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x113, 0xf, 0xf, false));   // row_shr:3
    v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x114, 0xf, 0xe, false));   // row_shr:4
    v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x118, 0xf, 0xc, false));   // row_shr:8
    v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x142, 0xa, 0xf, false));   // row_bcast:15
    v = op(v, __builtin_amdgcn_update_dpp(id, v, 0x143, 0xc, 0xf, false));   // row_bcast:31
    return __builtin_amdgcn_readlane(v, 63);
}

__device__ __forceinline__ int wave_min(int v) { return wave_reduce_dpp<false>(v); }
__device__ __forceinline__ int wave_max(int v) { return wave_reduce_dpp<true>(v); }

// Particles of this lane within the face box margin of a periodic face: bit 2k low face, 2k + 1
// high face of axis k (k_prep, or the previous step's pass B, gathers them per step into DevState.seam_occ).
__device__ __forceinline__ int seam_bits(const DevParams& P, double x, double y, double z)
{
    const double v[3] = {x, y, z};
    int b = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (k == 2 && P.dim == 2) break;
        if ((P.seam_always >> k) & 1) continue;   // (the slab axis: the face box always applies)
        b |= (v[k] < P.inner_lo[k] ? 1 : 0) << (2 * k);
        b |= (v[k] > P.inner_hi[k] ? 2 : 0) << (2 * k);
    }
    return b;
}

// calculateWall (3031-3060) then calculatePeriodicBoundary (3322-3333) for particle p of B.
__device__ __forceinline__ void move_and_wrap(const DevParams& P, const DevState* st, Soa& B, int p,
                                              double& x, double& y, double& z)
{
#pragma clang fp contract(off)
    const int t = B.type[p];
    if (P.module == MPH_MODULE_TUREK_HRON && dev_is_fluid(t)) {
        // Turek_Hron: setInitialVelocityProfile (main.cpp:419-441) runs every step before
        // calculateWall (592-594): parabolic inlet for x <= 0.01 and, while Time < 0.7, the same
        // profile (without the 1.5 factor) for x > 1.5; YMIN/YMAX/UMAX from main.cpp:374-377
        const double ymin = 0.0, ymax = 0.41, umax = 1.0, h = ymax - ymin;
        if (x <= 0.01) {
            const double uy = y - ymin;
            B.vx[p] = (1.5 * 4.0 * umax / (h * h)) * uy * (h - uy);
            B.vy[p] = 0.0;
            B.vz[p] = 0.0;
        }
        if (x > 1.5 && st->time < 0.7) {
            const double uy = y - ymin;
            B.vx[p] = (4.0 * umax / (h * h)) * uy * (h - uy);
            B.vy[p] = 0.0;
            B.vz[p] = 0.0;
        }
    }
    if (dev_is_wall(t) && P.wall_motion == MPH_WALL_ROLLING) {
        // the Rolling branch of calculateWall (main.cpp:2974-3022): rotate about z through
        // WallCenter by the step's angle increment; the velocity is omega(t) x r_rot
        const double max_angle = 2.0 * M_PI / 180.0, period = 1.646;   // main.cpp:2959-2960
        const double omega_t = 2.0 * M_PI / period;
        const double theta = max_angle * sin(omega_t * st->time);
        const double dtheta_dt = max_angle * omega_t * cos(omega_t * st->time);
        const double theta_prev = max_angle * sin(omega_t * (st->time - P.dt));
        const double delta_theta = theta - theta_prev;
        const double cosD = cos(delta_theta), sinD = sin(delta_theta);
        const double* C = st->wall_c[t];
        const double r0 = x - C[0], r1 = y - C[1], r2 = z - C[2];
        const double a0 = cosD * r0 + -sinD * r1;
        const double a1 = sinD * r0 + cosD * r1;
        const double a2 = r2;
        const double w0 = 0.0, w1 = 0.0, w2 = dtheta_dt;
        B.vx[p] = w1 * a2 - w2 * a1;
        B.vy[p] = w2 * a0 - w0 * a2;
        B.vz[p] = w0 * a1 - w1 * a0;
        x = a0 + C[0];
        y = a1 + C[1];
        z = a2 + C[2];
    } else if (dev_is_wall(t) && st->time < 0.2) {
        const double* C = st->wall_c[t];
        const double* V = st->wall_vel[t];
        const double* w = st->wall_omega[t];
        const double (*R)[3] = st->wall_rot[t];
        const double r0 = x - C[0], r1 = y - C[1], r2 = z - C[2];
        const double a0 = R[0][0] * r0 + R[0][1] * r1 + R[0][2] * r2;
        const double a1 = R[1][0] * r0 + R[1][1] * r1 + R[1][2] * r2;
        const double a2 = R[2][0] * r0 + R[2][1] * r1 + R[2][2] * r2;
        B.vx[p] = w[1] * a2 - w[2] * a1 + V[0];
        B.vy[p] = w[2] * a0 - w[0] * a2 + V[1];
        B.vz[p] = w[0] * a1 - w[1] * a0 + V[2];
        x = a0 + C[0] + V[0] * P.dt;
        y = a1 + C[1] + V[1] * P.dt;
        z = a2 + C[2] + V[2] * P.dt;
    }
    x = mod_exact(x - P.dmin[0], P.dw[0]) + P.dmin[0];
    y = mod_exact(y - P.dmin[1], P.dw[1]) + P.dmin[1];
    z = mod_exact(z - P.dmin[2], P.dw[2]) + P.dmin[2];
    B.x[p] = x;
    B.y[p] = y;
    B.z[p] = z;
}

// ---------------------------------------------------------------------------- prep tail -----
// What opens a step's sort from a particle's moved and wrapped position, shared by k_prep and by the
// KEYS tail of the previous step's pass B: one body, so the two leave the
// same bits.

// The non-finite flag, the cell key (stored to *key and returned), the coarse map's mark and the face
// bits (occ).  cmap: a lazy wall step's coarse map (mph_params.h kCoarseShift), else null; a non-wall
// particle marks its coarse cell -- a plain store of the same byte by every marker, no atomic (the
// search reads the map, pass A clears it).  not_wall() is asked only with the map set.
template <typename NotWall>
__device__ __forceinline__ int prep_cell(const DevParams& P, const DevState* st, double x, double y, double z,
                                         int* key, unsigned char* cmap, NotWall not_wall, int& occ)
{
    if (!isfinite(x + y + z)) atomicOr(const_cast<int*>(&st->overflow), 4);   // MPH_ERR_NONFINITE
    const int cx = cell_axis(x, P.corg[0], P.dw[0], P.ginv[0], P.gc[0]);
    const int cy = cell_axis(y, P.corg[1], P.dw[1], P.ginv[1], P.gc[1]);
    const int cz = P.dim == 3 ? cell_axis(z, P.corg[2], P.dw[2], P.ginv[2], P.gc[2]) : 0;
    const int k = cell_index(P, cx, cy, cz);   // (cell_id)
    *key = k;
    if (cmap && not_wall())
        cmap[coarse_index(P, cx >> kCoarseShift, cy >> kCoarseShift, cz >> kCoarseShift)] = 1;
    occ = seam_bits(P, x, y, z);
    return k;
}

// The particles arrive in the previous cell order, so consecutive lanes often share a cell: one
// histogram atomic per run of equal keys; returns the lane's slot in its cell (run base + rank in the
// run).  Every lane of the wave takes part in the shuffles; the lanes past n (live false) come with
// k = -1 - lane, so they form runs of their own, and their result is not a slot.
__device__ __forceinline__ int prep_slot(int k, bool live, int* __restrict__ cnt)
{
    const int lane = threadIdx.x & 63;
    const int kprev = __shfl_up(k, 1, 64);
    const bool head = lane == 0 || kprev != k;
    const unsigned long long heads = __ballot(head);
    const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
    const int hl = 63 - __clzll(heads & upto);
    const unsigned long long above = heads & ~upto;
    const int next = above ? __ffsll((long long)above) - 1 : 64;
    int base = 0;
    if (live && head) base = atomicAdd(&cnt[k], next - lane);
    base = __shfl(base, hl, 64);
    return base + (lane - hl);
}

// entry p of a sort input C: its set (C or the VSrc's V) and index there; mig: a kept migrant
// (its id is read negated)
__device__ __forceinline__ int vsrc_entry(const VSrc& vs, const Soa& C, int p, Soa& S, bool& mig)
{
    S = C;
    mig = false;
    if (vs.idx && p < *vs.n) {
        const int q = vs.idx[p];
        mig = q < 0;
        S = vs.V;
        return mig ? -1 - q : q;
    }
    return p;
}

// Displacement u = Mod(x - x0 + W/2, W) - W/2 of calculateElasticDeformationVector (2700-2712),
// computed once per slot and substep instead of once per pair (same expression, same bits).
__device__ __forceinline__ double4 struct_disp(const DevParams& P, double4 x, double4 x0)
{
    return make_double4(image_exact<false>(x.x - x0.x, P.dw[0], P.hw[0], P.w075[0]),
                        image_exact<false>(x.y - x0.y, P.dw[1], P.hw[1], P.w075[1]),
                        image_exact<false>(x.z - x0.z, P.dw[2], P.hw[2], P.w075[2]), 0.0);
}

// The monitor kernels (mph_monitor.hip, mph_gauge.hip): is this step (the one the counters do not
// count yet) a sampled one?
__device__ __forceinline__ bool mon_sampled(const MonitorDev& M, long long& step)
{
    step = M.counters[0] + 1;
    return step % M.stride == 0;
}

// The wave fold of the deterministic reductions (the monitors' k_monitor_partial, the selection
// totals' k_sel_totals_partial).  OP: 0 sum, 1 min, 2 max.
template <int OP> __device__ __forceinline__ double mon_op2(double a, double b)
{
#pragma clang fp contract(off)
    return OP == 0 ? a + b : (OP == 1 ? fmin(a, b) : fmax(a, b));
}

// N (a power of two) accumulators per lane over the 64 lanes: every xor stage halves what a lane
// holds -- it keeps the entries of its side and hands the others across -- so N values cost N - 1 +
// (6 - log2 N) exchanges instead of 6 N.  Returns entry (lane & (N - 1)) over the whole wave; the
// order of the additions is fixed by the lane numbers alone.
template <int OP, int N> __device__ __forceinline__ double mon_wave_fold(double (&v)[N])
{
    const int lane = threadIdx.x & 63;
    int m = 1;
#pragma unroll
    for (int n = N; n > 1; n >>= 1, m <<= 1) {
        const bool hi = (lane & m) != 0;
#pragma unroll
        for (int i = 0; i < n / 2; ++i) {
            const double keep = hi ? v[2 * i + 1] : v[2 * i];
            const double send = hi ? v[2 * i] : v[2 * i + 1];
            v[i] = mon_op2<OP>(keep, __shfl_xor(send, m, 64));
        }
    }
#pragma unroll
    for (; m < 64; m <<= 1) v[0] = mon_op2<OP>(v[0], __shfl_xor(v[0], m, 64));
    return v[0];
}

// ------------------------------------------------------------------------ point stencil -----
// A point that is no particle -- a monitor probe, a lattice point -- and the particles around it.

// the point q wrapped into the periodic domain like a particle (2-D: z is ignored)
__device__ __forceinline__ void wrap_point(const DevParams& P, int dim, const double (&q)[3], double (&p)[3])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int d = 0; d < 3; ++d) p[d] = d < dim ? mod_exact(q[d] - P.dmin[d], P.dw[d]) + P.dmin[d] : 0.0;
}

// The Shepard weight w = (1 - r / h)^2 of a particle at (x, y, z) for the point p, r their distance on
// the minimum image (2-D: z is ignored); false when the particle is not within h.
template <int DIM>
__device__ __forceinline__ bool shepard_weight(const DevParams& P, const double (&p)[3], double h, double x, double y,
                                               double z, double& w)
{
#pragma clang fp contract(off)
    const double q0 = image_exact<false>(x - p[0], P.dw[0], P.hw[0], P.w075[0]);
    const double q1 = image_exact<false>(y - p[1], P.dw[1], P.hw[1], P.w075[1]);
    const double q2 = DIM == 3 ? image_exact<false>(z - p[2], P.dw[2], P.hw[2], P.w075[2]) : 0.0;
    const double r = sqrt(q0 * q0 + q1 * q1 + q2 * q2);
    if (!(r < h)) return false;
    const double u = 1.0 - r / h;
    w = u * u;
    return true;
}

// The stencil of k_sinit_search around the cell of the point p: kReach cells across the column axes
// a0 (, a1), P.sa cells along the contiguous axis ca -- the same cells for every column: one range
// [lo, hi], a second one [lo1, hi1] where the stencil wraps.
template <int DIM> struct PointStencil {
    int ca, a0, a1, c[3], lo, hi, lo1, hi1;
    static constexpr int ncol = DIM == 3 ? kGroups * kGroups : kGroups;
    __device__ __forceinline__ PointStencil(const DevParams& P, const double (&p)[3])
    {
        c[0] = cell_axis(p[0], P.corg[0], P.dw[0], P.ginv[0], P.gc[0]);
        c[1] = cell_axis(p[1], P.corg[1], P.dw[1], P.ginv[1], P.gc[1]);
        c[2] = DIM == 3 ? cell_axis(p[2], P.corg[2], P.dw[2], P.ginv[2], P.gc[2]) : 0;
        ca = contig_axis(DIM, P.perm);
        a0 = DIM == 3 ? (ca == 0 ? 1 : 0) : 0;
        a1 = DIM == 3 ? (ca == 2 ? 1 : 2) : -1;
        const int cc = ca == 0 ? c[0] : (ca == 1 ? c[1] : c[2]), g = ca == 0 ? P.gc[0] : (ca == 1 ? P.gc[1] : P.gc[2]);
        lo = cc - P.sa; hi = cc + P.sa; lo1 = 0; hi1 = -1;
        if (hi - lo + 1 >= g) { lo = 0; hi = g - 1; }
        else if (lo < 0) { lo1 = lo + g; hi1 = g - 1; lo = 0; }
        else if (hi >= g) { lo1 = 0; hi1 = hi - g; hi = g - 1; }
    }
    // column col's first cell: cell (.., m along ca, ..) is column(col) + m, the contiguous axis
    // being the fastest of cell_index
    __device__ __forceinline__ int column(const DevParams& P, int col) const
    {
        const int d0 = (DIM == 3 ? col / kGroups : col) - kReach, d1 = DIM == 3 ? col % kGroups - kReach : 0;
        int q[3] = {c[0], c[1], c[2]};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            if (d == a0) q[d] = wrap_cell(q[d] + d0, P.gc[d]);
            else if (d == a1) q[d] = wrap_cell(q[d] + d1, P.gc[d]);
        }
        return cell_index(P, ca == 0 ? 0 : q[0], ca == 1 ? 0 : q[1], ca == 2 ? 0 : q[2]);
    }
};

// ---------------------------------------------------------------------------- launchers -----

static inline int blocks(int n, int t) { return (n + t - 1) / t; }

// (non-deduced: launch's arguments convert to the kernel's own parameter types, as in a call)
template <typename T> struct Same { using type = T; };

// One launch, profiled when prof is set (mph_profile_steps): its start/stop events come from the
// kernel's dispatch packet (hipExtLaunchKernelGGL), or are recorded around it (Profiler::events).
// Direct launches run ~9 us apart and start with a written-back L2, so they take 3-8 % longer than
// the same kernels replayed from a graph (profiles/r05/final/prof: rocprofv3 trace);
// mph_profile_graphs times the list kernels as graph replays.
template <typename... A>
static void launch(Profiler* prof, const char* name, hipStream_t stream, void (*kernel)(A...), dim3 grid, dim3 block,
                   typename Same<A>::type... args)
{
    if (!prof) {
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, args...);
        return;
    }
    hipEvent_t a, b;
    if (prof->events(name, stream, &a, &b)) {
        hipExtLaunchKernelGGL(kernel, grid, block, 0, stream, a, b, 0u, args...);
    } else {
        (void)hipEventRecord(a, stream);
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, args...);
        (void)hipEventRecord(b, stream);
    }
}

// f(Int<2>{}) or f(Int<3>{}): the kernels are instantiated per dimension
template <int N> using Int = std::integral_constant<int, N>;

template <typename F>
static void by_dim(int dim, F&& f)
{
    if (dim == 3) f(Int<3>{});
    else f(Int<2>{});
}

// f(std::true_type{}) or f(std::false_type{}): a kernel's template flag from a step's form
template <typename F>
static void by_flag(bool on, F&& f)
{
    if (on) f(std::true_type{});
    else f(std::false_type{});
}

}  // namespace mph
