// mph_elastic.hip -- the elastic solid (mph_kernels.h has the step-to-launch map): the substep
// kernels k_struct_stress / k_struct_velocity and the one-time construction of the fixed
// Lagrangian lists on the device, k_sinit_*.
#include <cstdlib>
#include <vector>

#include "mph_device.h"
#include "mph_env.h"

namespace mph {

// ------------------------------------------------------------------------ elastic solid ----

#ifndef MPH_US
#define MPH_US 4   // batch width of the elastic list loops
#endif

// x0_ij = Mod(x0_j - x0_i + W/2, W) - W/2 and weight(x0_ij, RadiusP) of the fixed Lagrangian
// pair (main.cpp:2705-2716; weight() 268-295, norm over dim components): the same expressions as
// the host's former per-pair table (mph_host.cpp build_structure), recomputed from the 32-byte
// x0 records so that no per-pair table is streamed from HBM every substep.
template <int DIM>
__device__ __forceinline__ double4 struct_pair(const DevParams& P, double4 x0i, double4 x0j)
{
#pragma clang fp contract(off)
    double q[3] = {0.0, 0.0, 0.0};
    q[0] = image_exact<false>(x0j.x - x0i.x, P.dw[0], P.hw[0], P.w075[0]);
    q[1] = image_exact<false>(x0j.y - x0i.y, P.dw[1], P.hw[1], P.w075[1]);
    if (DIM == 3) q[2] = image_exact<false>(x0j.z - x0i.z, P.dw[2], P.hw[2], P.w075[2]);
    double r2 = 0.0;
#pragma unroll
    for (int d = 0; d < DIM; ++d) r2 += q[d] * q[d];
    const double t = sqrt(r2) / P.rp;
    return make_double4(q[0], q[1], q[2], P.cw_pair * ((1.0 - t) * (1.0 - t)));
}

// ELL entry k of slot s (tile width w)
__device__ __forceinline__ size_t sell(int s, int w, int k)
{
    return ((size_t)(s >> 6) * w + k) * 64 + (s & 63);
}

// the G lanes of one structure slot (G | 64, adjacent lanes) sum their strided shares of its list
// in a butterfly: every lane of the group ends with the same total (a + b == b + a exactly)
template <int G>
__device__ __forceinline__ double group_sum(double v)
{
#pragma unroll
    for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

// calculateElasticDeformationVector (2673-2754) + calculateStress (2756-2809) + the first
// Piola-Kirchhoff tensor P = F S L of calculateStressForce (2837-2852).  G lanes per structure
// slot (struct_lanes: enough waves to cover the latency of a small structure), each summing every
// G-th entry of the fixed list, read ELL-tiled in batches of MPH_US; per neighbour only the
// 32-byte displacement record u_j and the x0 record are gathered.
template <int DIM, int G, int U = MPH_US>
__global__ __launch_bounds__(256) void k_struct_stress(DevParams P, int s0, int ns, int wo, const int* __restrict__ ocnt,
                                                       const int* __restrict__ eo_nb,
                                                       const double4* __restrict__ sx0,
                                                       const double4* __restrict__ su,
                                                       const double* __restrict__ L,
                                                       const double2* __restrict__ lame,
                                                       double4* __restrict__ sP, double* __restrict__ sF,
                                                       double* __restrict__ sE, double* __restrict__ sS,
                                                       int fes, int store)
{
    const int s = s0 + (int)((blockIdx.x * blockDim.x + threadIdx.x) / G);   // slots [s0, ns)
    const int g = (int)threadIdx.x & (G - 1);
    if (s >= ns) return;   // whole groups: G divides the block
    const double4 u4 = su[s];
    const double4 x0s = sx0[s];
    const double ui[3] = {u4.x, u4.y, u4.z};
    double Fr[DIM][DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
        for (int b = 0; b < DIM; ++b) Fr[a][b] = 0.0;
    const int cnt = ocnt[s];
    for (int k0 = g; k0 < cnt; k0 += G * U) {
        int t[U];
        double4 pr[U], uj[U], xj[U];
#pragma unroll
        for (int u = 0; u < U; ++u) t[u] = eo_nb[sell(s, wo, k0 + G * u < cnt ? k0 + G * u : cnt - 1)];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            uj[u] = su[t[u]];
            xj[u] = sx0[t[u]];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) pr[u] = struct_pair<DIM>(P, x0s, xj[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (k0 + G * u >= cnt) break;
            const double x0ij[3] = {pr[u].x, pr[u].y, pr[u].z};
            const double ujv[3] = {uj[u].x, uj[u].y, uj[u].z};
#pragma unroll
            for (int a = 0; a < DIM; ++a) {
                const double xa = x0ij[a] + (ujv[a] - ui[a]);
#pragma unroll
                for (int b = 0; b < DIM; ++b) Fr[a][b] += pr[u].w * xa * x0ij[b];
            }
        }
    }
    if (G > 1) {
#pragma unroll
        for (int a = 0; a < DIM; ++a)
#pragma unroll
            for (int b = 0; b < DIM; ++b) Fr[a][b] = group_sum<G>(Fr[a][b]);
        if (g != 0) return;
    }
    double Lm[DIM][DIM], F[DIM][DIM], E[DIM][DIM], S[DIM][DIM], PK[DIM][DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
        for (int b = 0; b < DIM; ++b) Lm[a][b] = L[(size_t)s * 9 + 3 * a + b];
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
        for (int b = 0; b < DIM; ++b) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < DIM; ++k) acc += Fr[a][k] * Lm[k][b];
            F[a][b] = acc;
        }
    double tr = 0.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
        for (int b = 0; b < DIM; ++b) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < DIM; ++k) acc += F[k][a] * F[k][b];
            E[a][b] = 0.5 * (acc - (a == b ? 1.0 : 0.0));
            if (a == b) tr += E[a][b];
        }
    const double2 lm = lame[s];   // (lambda, mu)
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
        for (int b = 0; b < DIM; ++b) S[a][b] = 2.0 * lm.y * E[a][b] + (a == b ? lm.x * tr : 0.0);
    // P = F S L
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
        for (int b = 0; b < DIM; ++b) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < DIM; ++k)
#pragma unroll
                for (int l = 0; l < DIM; ++l) acc += F[a][k] * S[k][l] * Lm[l][b];
            PK[a][b] = acc;
        }
    if (DIM == 2) {
        sP[s] = make_double4(PK[0][0], PK[0][1], PK[1 % DIM][0], PK[1 % DIM][1 % DIM]);
    } else {
#pragma unroll
        for (int a = 0; a < DIM; ++a) sP[(size_t)s * 3 + a] = make_double4(PK[a][0], PK[a][1], PK[a][DIM - 1], 0.0);
    }
    if (!store) return;   // F, E, S are outputs only: the last substep of a batch's last step
    // element planes (StructDev): consecutive slots of the wave store one run per element; in 2-D
    // the third row and column stay the zeros set at creation
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
        for (int b = 0; b < DIM; ++b) {
            const size_t o = (size_t)(3 * a + b) * fes + s;
            sF[o] = F[a][b];
            sE[o] = E[a][b];
            sS[o] = S[a][b];
        }
}

// calculateStressForce (2854-2887) in gather form: v_s += dt_e/rho_s * [P_s sum_j w_sj x0_sj -
// sum_{i lists s} w_is P_i x0_is] (the reference's scatter regrouped by receiver; the first sum is
// fixed, wx0), followed by updateElasticPosition (1910-2082): module clamp, then the always-
// compiled second drift of 2070-2079 (free particles drift twice per substep; structure
// acceleration is zero).  Also refreshes the displacement u for the next substep.
// first Piola-Kirchhoff rows of slot s (2-D: one packed double4, 3-D: three rows)
template <int DIM>
__device__ __forceinline__ void struct_P(const double4* sP, int s, double (&Pm)[DIM][3])
{
    if (DIM == 2) {
        const double4 r = sP[s];
        Pm[0][0] = r.x; Pm[0][1] = r.y; Pm[0][2] = 0.0;
        Pm[1 % DIM][0] = r.z; Pm[1 % DIM][1] = r.w; Pm[1 % DIM][2] = 0.0;
    } else {
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            const double4 r = sP[(size_t)s * 3 + a];
            Pm[a][0] = r.x; Pm[a][1] = r.y; Pm[a][2] = r.z;
        }
    }
}

template <int DIM, int G, int U = MPH_US>
__global__ __launch_bounds__(256) void k_struct_velocity(DevParams P, int s0, int ns, int wi,
                                                         const int* __restrict__ icnt,
                                                         const int* __restrict__ ei_nb,
                                                         const double4* __restrict__ wx0,
                                                         const double4* __restrict__ sP,
                                                         const double* __restrict__ inv_rho,
                                                         const int* __restrict__ clamp,
                                                         const double4* __restrict__ sx0,
                                                         double4* __restrict__ sx, double4* __restrict__ sv,
                                                         double4* __restrict__ su, int last,
                                                         const int* __restrict__ bidx, Soa B,
                                                         double4* __restrict__ force)
{
    const int s = s0 + (int)((blockIdx.x * blockDim.x + threadIdx.x) / G);   // slots [s0, ns)
    const int g = (int)threadIdx.x & (G - 1);
    if (s >= ns) return;   // whole groups: G divides the block
    double dv[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) dv[a] = 0.0;
    if (g == 0) {   // the receiver's own half, once per slot (G > 1: added to lane 0's share)
        const double4 c = wx0[s];
        const double cv[3] = {c.x, c.y, c.z};
        double Ps[DIM][3];
        struct_P<DIM>(sP, s, Ps);
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            double f = 0.0;
#pragma unroll
            for (int b = 0; b < DIM; ++b) f += Ps[a][b] * cv[b];
            dv[a] = f;
        }
    }
    const int cnt = icnt[s];
    const double4 x0me = sx0[s];
    for (int k0 = g; k0 < cnt; k0 += G * U) {
        int t[U];
        double4 xi0[U];
        double Pi[U][DIM][3];
#pragma unroll
        for (int u = 0; u < U; ++u) t[u] = ei_nb[sell(s, wi, k0 + G * u < cnt ? k0 + G * u : cnt - 1)];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            struct_P<DIM>(sP, t[u], Pi[u]);
            xi0[u] = sx0[t[u]];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (k0 + G * u >= cnt) break;
            // the sender i's pair {x0_is, w_is} (main.cpp:2862-2880, from i's side)
            const double4 pr = struct_pair<DIM>(P, xi0[u], x0me);
            const double x0[3] = {pr.x, pr.y, pr.z};
#pragma unroll
            for (int a = 0; a < DIM; ++a) {
                double f = 0.0;
#pragma unroll
                for (int b = 0; b < DIM; ++b) f += Pi[u][a][b] * x0[b];
                dv[a] -= f * pr.w;
            }
        }
    }
    if (G > 1) {
#pragma unroll
        for (int a = 0; a < DIM; ++a) dv[a] = group_sum<G>(dv[a]);
        if (g != 0) return;
    }
    double4 v = sv[s];
    double4 xo = sx[s];
    const double ir = inv_rho[s];
    double vv[3] = {v.x, v.y, v.z};
#pragma unroll
    for (int a = 0; a < DIM; ++a) vv[a] += ir * dv[a] * P.edt;
    double xx[3] = {xo.x, xo.y, xo.z};
    const int cl = clamp[s];
    const double4 x0s = sx0[s];
    if (cl) {
        xx[0] = x0s.x; xx[1] = x0s.y; xx[2] = x0s.z;
        vv[0] = vv[1] = vv[2] = 0.0;
    } else if (P.module != MPH_MODULE_NONE) {
        for (int d = 0; d < 3; ++d) xx[d] += vv[d] * P.edt;
    }
    for (int d = 0; d < 3; ++d) xx[d] += vv[d] * P.edt;
    if (last) {
        // back into the integrated state (A order) at the entry pass B took it from
        const int r = bidx[s];
        B.x[r] = xx[0]; B.y[r] = xx[1]; B.z[r] = xx[2];
        B.vx[r] = vv[0]; B.vy[r] = vv[1]; B.vz[r] = vv[2];
        if (cl == 1) force[r] = make_double4(0.0, 0.0, 0.0, 0.0);
        return;
    }
    sv[s] = make_double4(vv[0], vv[1], vv[2], 0.0);
    const double4 xn = make_double4(xx[0], xx[1], xx[2], xo.w);
    sx[s] = xn;
    su[s] = struct_disp(P, xn, x0s);
}

// --------------------------------------------------------- elastic-solid initialisation ----
// calculateInitialNeighbor (main.cpp:1497-1658), calculateNormalizer (2544-2653) on the device.
// The structure slots (x0 in slot = file order) are binned on the GPU cell grid of the fluid
// search (cells >= rc/2, the contiguous axis halved); each slot scans the 5x5(x9) stencil of
// slot cells with the reference's exact test  q0^2+q1^2+q2^2 <= (MaxRadius+MARGIN)^2  on the
// Mod image of InitialPosition (2-D: q2 = 0, main.cpp:1605), structure j only (the binned set).
// Rows are then sorted ascending, the transpose (the senders of calculateStressForce's scatter)
// is built with atomics and sorted, and the normalizer sums run over the sorted rows in the
// host's order -- so lists, counts, Normalizer and the fixed sum w x0 equal the host build.

__global__ __launch_bounds__(256) void k_sinit_bin(DevParams P, int ns, const double4* __restrict__ x0,
                                                   int* __restrict__ key, int* __restrict__ cnt,
                                                   int* __restrict__ slot)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= ns) return;
    const double4 p = x0[s];
    const int k = cell_id(P, p.x, p.y, p.z);
    key[s] = k;
    slot[s] = atomicAdd(&cnt[k], 1);
}

// cell order, slot-ascending inside a cell (deterministic)
__global__ __launch_bounds__(256) void k_sinit_place(int ns, const int* __restrict__ key,
                                                     const int* __restrict__ slot,
                                                     const int* __restrict__ start, int* __restrict__ tmp,
                                                     int* __restrict__ sorted, int phase)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= ns) return;
    const int k = key[s];
    if (phase == 0) {
        tmp[start[k] + slot[s]] = s;
        return;
    }
    const int b = start[k], e = start[k + 1];
    int r = 0;
    for (int q = b; q < e; ++q) r += tmp[q] < s;
    sorted[b + r] = s;
}

// mode 0: count the row of every slot; mode 1: write it into the ELL tile rows (width w, stencil
// order) -- per-slot overflow (>= 512, main.cpp:1609-1611) raises the error flag
template <int DIM>
__global__ __launch_bounds__(256) void k_sinit_search(DevParams P, int ns, const double4* __restrict__ x0,
                                                      const int* __restrict__ start,
                                                      const int* __restrict__ sorted, int* __restrict__ ocnt,
                                                      int* __restrict__ ell, int w, int mode,
                                                      DevState* __restrict__ st)
{
#pragma clang fp contract(off)
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= ns) return;
    const double4 xi = x0[s];
    const int cx = cell_axis(xi.x, P.corg[0], P.dw[0], P.ginv[0], P.gc[0]);
    const int cy = cell_axis(xi.y, P.corg[1], P.dw[1], P.ginv[1], P.gc[1]);
    const int cz = DIM == 3 ? cell_axis(xi.z, P.corg[2], P.dw[2], P.ginv[2], P.gc[2]) : 0;
    // stencil half-widths in cells: kReach across (cells >= rc/kReach), P.sa along the contiguous axis
    const int ca = contig_axis(DIM, P.perm);
    const int rx = ca == 0 ? P.sa : kReach, ry = ca == 1 ? P.sa : kReach,
              rz = DIM == 3 ? (ca == 2 ? P.sa : kReach) : 0;
    int c = 0;
    for (int dx = -rx; dx <= rx; ++dx) {
        const int jx = wrap_cell(cx + dx, P.gc[0]);
        for (int dy = -ry; dy <= ry; ++dy) {
            const int jy = wrap_cell(cy + dy, P.gc[1]);
            for (int dz = -rz; dz <= rz; ++dz) {
                const int jz = DIM == 3 ? wrap_cell(cz + dz, P.gc[2]) : 0;
                const int cell = cell_index(P, jx, jy, jz);
                for (int q = start[cell], e = start[cell + 1]; q < e; ++q) {
                    const int t = sorted[q];
                    if (t == s) continue;
                    const double4 xj = x0[t];
                    const double q0 = image_exact<false>(xj.x - xi.x, P.dw[0], P.hw[0], P.w075[0]);
                    const double q1 = image_exact<false>(xj.y - xi.y, P.dw[1], P.hw[1], P.w075[1]);
                    const double q2 = DIM == 3 ? image_exact<false>(xj.z - xi.z, P.dw[2], P.hw[2], P.w075[2]) : 0.0;
                    if (r2_exact(q0, q1, q2) <= P.rc2) {
                        if (mode == 1 && c < w) ell[sell(s, w, c)] = t;
                        ++c;
                    }
                }
            }
        }
    }
    if (mode == 0) {
        ocnt[s] = c;
        if (c >= kMaxNeighbor) atomicOr(&st->overflow, 1);
    }
}

// ascending order inside each ELL row (insertion sort in place; rows are <= ~80 long)
__global__ __launch_bounds__(256) void k_sinit_sort_rows(int ns, const int* __restrict__ cnt, int* __restrict__ ell,
                                                         int w)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= ns) return;
    const int n = cnt[s];
    for (int a = 1; a < n; ++a) {
        const int v = ell[sell(s, w, a)];
        int b = a - 1;
        while (b >= 0 && ell[sell(s, w, b)] > v) {
            ell[sell(s, w, b + 1)] = ell[sell(s, w, b)];
            --b;
        }
        ell[sell(s, w, b + 1)] = v;
    }
}

// transpose: mode 0 counts the in-degree, mode 1 appends s to the in-row of every t it lists
__global__ __launch_bounds__(256) void k_sinit_transpose(int ns, const int* __restrict__ ocnt,
                                                         const int* __restrict__ eo, int wo,
                                                         int* __restrict__ icnt, int* __restrict__ ei, int wi,
                                                         int mode)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= ns) return;
    const int n = ocnt[s];
    for (int k = 0; k < n; ++k) {
        const int t = eo[sell(s, wo, k)];
        const int pos = atomicAdd(&icnt[t], 1);
        if (mode == 1) ei[sell(t, wi, pos)] = s;
    }
}

// calculateNormalizer (main.cpp:2555-2651) over the sorted row: the 3x3 accumulation in both
// dimensions (the TWO_DIMENSION typo of 2545), 2-D inverse with the identity fallback, 3-D
// cofactor inverse (left unchanged when det = 0, like the reference); plus the fixed sum of
// w_sj x0_sj that the P_s half of the gather-form stress force uses
template <int DIM>
__global__ __launch_bounds__(256) void k_sinit_normalizer(DevParams P, int ns, const double4* __restrict__ x0,
                                                          const int* __restrict__ ocnt,
                                                          const int* __restrict__ eo, int wo,
                                                          double* __restrict__ L, double4* __restrict__ wx0)
{
#pragma clang fp contract(off)
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= ns) return;
    const double4 xi = x0[s];
    double N[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    double c3[3] = {0.0, 0.0, 0.0};
    const int n = ocnt[s];
    for (int k = 0; k < n; ++k) {
        const double4 xj = x0[eo[sell(s, wo, k)]];
        const double4 pr = struct_pair<DIM>(P, xi, xj);
        // the accumulation runs over all three components: in 2-D the z image of equal z is 0
        const double q[3] = {pr.x, pr.y, image_exact<false>(xj.z - xi.z, P.dw[2], P.hw[2], P.w075[2])};
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) N[a][b] += pr.w * q[a] * q[b];
        c3[0] += pr.w * pr.x;
        c3[1] += pr.w * pr.y;
        c3[2] += pr.w * pr.z;
    }
    if (DIM == 2) {
        const double a = N[0][0], b = N[0][1], cc = N[1][0], d = N[1][1];
        const double det = a * d - b * cc;
        if (det != 0.0) {
            N[0][0] = d / det; N[0][1] = -b / det; N[1][0] = -cc / det; N[1][1] = a / det;
        } else {
            N[0][0] = 1.0; N[0][1] = 0.0; N[1][0] = 0.0; N[1][1] = 1.0;
        }
    } else {
        const double det = N[0][0] * (N[1][1] * N[2][2] - N[1][2] * N[2][1])
                         - N[0][1] * (N[1][0] * N[2][2] - N[1][2] * N[2][0])
                         + N[0][2] * (N[1][0] * N[2][1] - N[1][1] * N[2][0]);
        if (det != 0.0) {
            double adj[3][3];
            adj[0][0] = N[1][1] * N[2][2] - N[1][2] * N[2][1];
            adj[0][1] = -N[1][0] * N[2][2] + N[1][2] * N[2][0];
            adj[0][2] = N[1][0] * N[2][1] - N[1][1] * N[2][0];
            adj[1][0] = -N[0][1] * N[2][2] + N[0][2] * N[2][1];
            adj[1][1] = N[0][0] * N[2][2] - N[0][2] * N[2][0];
            adj[1][2] = -N[0][0] * N[2][1] + N[0][1] * N[2][0];
            adj[2][0] = N[0][1] * N[1][2] - N[0][2] * N[1][1];
            adj[2][1] = -N[0][0] * N[1][2] + N[0][2] * N[1][0];
            adj[2][2] = N[0][0] * N[1][1] - N[0][1] * N[1][0];
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) N[a][b] = adj[a][b] / det;
        }
    }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) L[(size_t)s * 9 + 3 * a + b] = N[a][b];
    wx0[s] = make_double4(c3[0], c3[1], c3[2], 0.0);
}

// ---------------------------------------------------------------------------- launchers -----

// lanes per structure slot: one lane per slot while the launch has >= kStructLanesTarget lanes
// (eight waves per SIMD), else the smallest power of two up to 4 that reaches it -- a few ten
// thousand slots (a gate, a rank's share of one) would otherwise run one long serial list loop per
// lane on a fraction of the SIMDs.  Same box (profiles/r03/struct_lanes/): FSI gate (40 k slots,
// 3-D) stress + velocity 0.089 ms at 1 lane, 0.052 at 4, 0.055 at 8; Bar (400 k slots, 2-D)
// 0.094 at 1, 0.091 at 2, 0.102 at 4.  MPH_STRUCT_LANES=1|2|4|8 fixes it (A/B timing, tests).
constexpr long kStructLanesTarget = 8L * 1024 * 64;

int struct_lanes(int nslots)
{
    const int forced = env_int("MPH_STRUCT_LANES", 0);   // read per launch (graphs capture once)
    if (forced == 1 || forced == 2 || forced == 4 || forced == 8) return forced;
    int g = 1;
    while (g < 4 && (long)nslots * g < kStructLanesTarget) g *= 2;
    return g;
}

// f(Int<dim>{}, Int<lanes per slot>{}) of a structure kernel over the slots [s0, s1): its grid
template <typename F>
static void by_dim_lanes(const Launch& L, F&& f)
{
    const int lanes = struct_lanes(L.S->n_own);   // not the range: the halves sum alike
    by_dim(L.P->dim, [&](auto D) {
        switch (lanes) {
        case 8: f(D, Int<8>{}); break;
        case 4: f(D, Int<4>{}); break;
        case 2: f(D, Int<2>{}); break;
        default: f(D, Int<1>{}); break;
        }
    });
}

void launch_struct_stress(const Launch& L, bool store, int s0, int s1)
{
    const DevParams& P = *L.P;
    const StructDev& S = *L.S;
    if (s1 < 0) s1 = S.n_own;
    if (s1 <= s0) return;
    by_dim_lanes(L, [&](auto D, auto G) {
        launch(L.prof, "struct_stress", L.stream, k_struct_stress<decltype(D)::value, decltype(G)::value>,
               dim3(blocks((s1 - s0) * G(), 256)), dim3(256), P, s0, s1, S.wo, S.ocnt, S.eo_nb, S.x0, S.u, S.L, S.lame,
               S.P, S.F, S.E, S.S, S.fes, store ? 1 : 0);
    });
}

void launch_struct_velocity(const Launch& L, bool last, int s0, int s1)
{
    const DevParams& P = *L.P;
    const StructDev& S = *L.S;
    if (s1 < 0) s1 = S.n_own;
    if (s1 <= s0) return;
    by_dim_lanes(L, [&](auto D, auto G) {
        launch(L.prof, "struct_velocity", L.stream, k_struct_velocity<decltype(D)::value, decltype(G)::value>,
               dim3(blocks((s1 - s0) * G(), 256)), dim3(256), P, s0, s1, S.wi, S.icnt, S.ei_nb, S.wx0, S.P, S.inv_rho,
               S.clamp, S.x0, S.x, S.v, S.u, last ? 1 : 0, S.bidx, L.B, L.force);
    });
}

void launch_structure(const Launch& L, bool last)
{
    if (L.P->n_struct == 0) return;
    for (int sub = 0; sub < L.P->substeps; ++sub) {
        const bool final_sub = sub == L.P->substeps - 1;
        launch_struct_stress(L, last && final_sub);
        launch_struct_velocity(L, final_sub);
    }
}

int launch_struct_init(const Launch& L, int ns, const double4* x0, int* key, int* slot, int* tmp, int* sorted,
                       int* ocnt, int* icnt, int** eo, int* wo, int** ei, int* wi, double* Lm, double4* wx0,
                       void* (*alloc)(void*, size_t), void* actx)
{
    Profiler* prof = L.prof;
    const DevParams& P = *L.P;
    if (ns <= 0) return 0;
    const dim3 g(blocks(ns, 256)), b(256);
    // the rows of every slot: counted (ell null), then stored
    auto search = [&](int* ell, int w, int store) {
        by_dim(P.dim, [&](auto D) {
            launch(prof, "sinit_search", L.stream, k_sinit_search<decltype(D)::value>, g, b, P, ns, x0, L.start,
                   sorted, ocnt, ell, w, store, L.st);
        });
    };
    // bin the slots on the grid (L.cnt is zero between steps and the scan re-zeroes it)
    launch(prof, "sinit_bin", L.stream, k_sinit_bin, g, b, P, ns, x0, key, L.cnt, slot);
    launch_scan(L.cnt, P.ncell, L.bsum, L.start, ns, nullptr, L.stream, prof);
    launch(prof, "sinit_place", L.stream, k_sinit_place, g, b, ns, key, slot, L.start, tmp, sorted, 0);
    launch(prof, "sinit_place", L.stream, k_sinit_place, g, b, ns, key, slot, L.start, tmp, sorted, 1);
    search(nullptr, 0, 0);
    // ELL width = the longest row (one host read at initialisation)
    std::vector<int> h(ns);
    if (hipMemcpyAsync(h.data(), ocnt, sizeof(int) * ns, hipMemcpyDeviceToHost, L.stream) != hipSuccess ||
        hipStreamSynchronize(L.stream) != hipSuccess)
        return -1;
    int w = 1;
    for (int v : h) w = v > w ? v : w;
    if (w >= kMaxNeighbor) return -2;
    const size_t ntile = ((size_t)ns + 63) / 64;
    *eo = (int*)alloc(actx, ntile * w * 64 * sizeof(int));
    if (!*eo) return -3;
    if (hipMemsetAsync(*eo, 0, ntile * w * 64 * sizeof(int), L.stream) != hipSuccess) return -1;
    search(*eo, w, 1);
    launch(prof, "sinit_sort_rows", L.stream, k_sinit_sort_rows, g, b, ns, ocnt, *eo, w);
    *wo = w;
    // transpose: in-degrees, width, then the rows (atomic order) sorted ascending
    if (hipMemsetAsync(icnt, 0, sizeof(int) * ns, L.stream) != hipSuccess) return -1;
    launch(prof, "sinit_transpose", L.stream, k_sinit_transpose, g, b, ns, ocnt, *eo, w, icnt, nullptr, 0, 0);
    if (hipMemcpyAsync(h.data(), icnt, sizeof(int) * ns, hipMemcpyDeviceToHost, L.stream) != hipSuccess ||
        hipStreamSynchronize(L.stream) != hipSuccess)
        return -1;
    int wi2 = 1;
    for (int v : h) wi2 = v > wi2 ? v : wi2;
    *ei = (int*)alloc(actx, ntile * wi2 * 64 * sizeof(int));
    if (!*ei) return -3;
    if (hipMemsetAsync(*ei, 0, ntile * wi2 * 64 * sizeof(int), L.stream) != hipSuccess) return -1;
    if (hipMemsetAsync(icnt, 0, sizeof(int) * ns, L.stream) != hipSuccess) return -1;
    launch(prof, "sinit_transpose", L.stream, k_sinit_transpose, g, b, ns, ocnt, *eo, w, icnt, *ei, wi2, 1);
    launch(prof, "sinit_sort_rows", L.stream, k_sinit_sort_rows, g, b, ns, icnt, *ei, wi2);
    *wi = wi2;
    by_dim(P.dim, [&](auto D) {
        launch(prof, "sinit_normalizer", L.stream, k_sinit_normalizer<decltype(D)::value>, g, b, P, ns, x0, ocnt, *eo,
               w, Lm, wx0);
    });
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace mph
