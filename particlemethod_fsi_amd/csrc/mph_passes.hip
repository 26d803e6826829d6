// mph_passes.hip -- the passes over the neighbour lists (mph_list.h): k_pass_a, k_pass_b and
// k_virial (mph_kernels.h has the step-to-launch map).
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "mph_list.h"

namespace mph {

// Velocity of sorted particle i for the list passes, from its gather record {x, y, z, vx, vy, vz}
// (k_rank_scatter then skips the SoA velocity stores).
__device__ __forceinline__ void own_velocity(const Soa& A, int i, double& vx, double& vy, double& vz)
{
    const double2 b = A.p6[3 * (size_t)i + 1], c = A.p6[3 * (size_t)i + 2];
    vx = b.y; vy = c.x; vz = c.y;
}

// ----------------------------------------------------------------------------- pass A sums --

struct PassA {
    double da = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0, vs = 0.0, dv = 0.0;
    // force sums that need no pass-A value of j: S = sum_j [r<RP] dwp(r)/r V q_ij (the P_i half
    // of calculatePressureP's (P_i+P_j) term, 2394-2424) and the viscous force (2478-2522)
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, v0 = 0.0, v1 = 0.0, v2 = 0.0;
};

// One neighbour's contribution to DensityA (2141-2171), GravityCenter (2174-2210), DensityP
// (2314-2341), DivergenceP (2343-2379), and (FORCE) the P_i half of the pressure force and the
// viscous force; (dvx, dvy, dvz) = v_j - v_i.  No implicit contraction: every accumulation is an
// explicit fma, so this branching form and the selecting form of the round-3 fused kernel
// give the same bits (a deselected fma(a, 0, acc) leaves acc unchanged).
// LEAN (a lean step's pass A, launch_pass_a): neither DensityA nor GravityCenter is stored, so their
// sums (o.da, o.g0..g2) and the InteractionRatio they read are left out; every other sum is the
// same expression in the same order.
template <bool FORCE, bool EQR = false, bool LEAN = false>
__device__ __forceinline__ void pass_a_term(const DevParams& P, const double* s_ratio, const double* s_mu, int ti,
                                            int tj, bool solid, double q0, double q1, double q2, double r2,
                                            double dvx, double dvy, double dvz, PassA& o)
{
#pragma clang fp contract(off)
    double r, ir;
    rsqrt_pair(r2, r, ir);
    const double dot = fma(dvz, q2, fma(dvy, q1, dvx * q0));
    if (EQR) {
        // RadiusA = RadiusP = RadiusV (pass_a_equal_radii): one cutoff test and one 1 - r/h for
        // all four kernels; same expressions otherwise
        if (r2 <= P.rp2) {
            const double t = r * P.inv_rp;
            const double omt = 1.0 - t;
            const double omt2 = omt * omt;
            const double u = (P.cdp * omt) * ir;
            o.vs = fma(P.cp, omt2, o.vs);
            o.dv = fma(-dot, u, o.dv);
            const bool strict = r2 < P.rp2;
            if (FORCE && strict && !(solid && dev_is_struct(tj))) {
                const double c = u * P.vol;
                o.s0 = fma(c, q0, o.s0);
                o.s1 = fma(c, q1, o.s1);
                o.s2 = fma(c, q2, o.s2);
            }
            if (!solid) {
                if (!LEAN) {
                    const double ratio = s_ratio[ti * kTypes + tj];
                    o.da = fma(ratio, (P.ca * t) * omt2, o.da);
                    const double w = (ratio * (P.cg * omt2)) * P.rg_r2g;
                    o.g0 = fma(q0, w, o.g0);
                    o.g1 = fma(q1, w, o.g1);
                    o.g2 = fma(q2, w, o.g2);
                }
                if (FORCE && strict) {
                    const double c = ((s_mu[ti * kTypes + tj] * omt) * dot) * ((ir * ir) * ir);
                    o.v0 = fma(c, q0, o.v0);
                    o.v1 = fma(c, q1, o.v1);
                    o.v2 = fma(c, q2, o.v2);
                }
            }
        }
        return;
    }
    if (r2 <= P.rp2) {
        const double omt = 1.0 - r * P.inv_rp;
        const double u = (P.cdp * omt) * ir;   // dw_p(r) / r
        o.vs = fma(P.cp * omt, omt, o.vs);
        o.dv = fma(-dot, u, o.dv);
        // strict test of the force loops (2402), and structure i sees only non-structure j
        // (InterfaceForce 2439-2472)
        if (FORCE && r2 < P.rp2 && !(solid && dev_is_struct(tj))) {
            const double c = u * P.vol;
            o.s0 = fma(c, q0, o.s0);
            o.s1 = fma(c, q1, o.s1);
            o.s2 = fma(c, q2, o.s2);
        }
    }
    if (!solid) {
        if (!LEAN) {
            const double ratio = s_ratio[ti * kTypes + tj];
            if (r2 <= P.ra2) {
                const double t = r * P.inv_ra;
                const double omt = 1.0 - t;
                o.da = fma(ratio, ((P.ca * t) * omt) * omt, o.da);
            }
            if (r2 <= P.rg2) {
                const double omt = 1.0 - r * P.inv_rg;
                const double w = (ratio * ((P.cg * omt) * omt)) * P.rg_r2g;
                o.g0 = fma(q0, w, o.g0);
                o.g1 = fma(q1, w, o.g1);
                o.g2 = fma(q2, w, o.g2);
            }
        }
        if (FORCE && r2 < P.rv2) {
            // s_mu holds -cvis cdv vol mu_ij (k_pass_a): dw_v(r) = -cdv (1 - r / rv)
            const double c = ((s_mu[ti * kTypes + tj] * (1.0 - r * P.inv_rv)) * dot) * ((ir * ir) * ir);
            o.v0 = fma(c, q0, o.v0);
            o.v1 = fma(c, q1, o.v1);
            o.v2 = fma(c, q2, o.v2);
        }
    }
}

// Epilogue: PhysicalCoefficients (2099-2137) and the pressure values of calculatePressureP
// (2384-2392) and calculatePressureA (2218-2223); with fpart, the neighbour-independent part of
// the force P_i S_i + viscous force, and the pass-B gather record {x, y, z, P}.
struct PassAOut {
    double *pres, *gx, *gy, *gz, *pa, *dens_a, *vstrain, *divp;
    double4 *fpart, *rec;
};

__device__ __forceinline__ void pass_a_finish(const DevParams& P, const DevTables* T, int ti, int i,
                                              const PassA& o, const PassAOut& out, double xi = 0.0,
                                              double yi = 0.0, double zi = 0.0)
{
    const double vstr = o.vs - P.n0p;
    const double kappa = vstr < 0.0 ? 0.0 : T->bulk[ti];
    double p = -T->bulk_visc[ti] * o.dv;
    if (vstr > 0.0) p += kappa * vstr;
    double pa = T->cofa[ti] * (o.da - P.n0a) / P.dx;
    if (P.n0a <= o.da) pa = 0.0;
    out.pres[i] = p;
    // null on the non-last steps of a replayed batch when nothing downstream reads them
    // (enqueue_step): GravityCenter/PressureA without surface tension, the three diagnostics
    if (out.gx) {
        out.gx[i] = o.g0;
        out.gy[i] = o.g1;
        out.gz[i] = o.g2;
        out.pa[i] = pa;
    }
    if (out.dens_a) {
        out.dens_a[i] = o.da;
        out.vstrain[i] = vstr;
        out.divp[i] = o.dv;
    }
    if (out.fpart) {
        out.fpart[i] = make_double4(p * o.s0 + o.v0, p * o.s1 + o.v1, p * o.s2 + o.v2, 0.0);
        rec_store(out.rec, P.n, i, xi, yi, zi, p);
    }
}

// ---------------------------------------------------------------------------- pass A -------

// List pass: the neighbour loops gather U neighbours' fields
// before the first use (all loads in flight at once; the loops are memory-latency bound).
#ifndef MPH_UA
#define MPH_UA 5   // pass A (with MPH_PA_WPE 4; coherent gathers at kReach 3: 0.355 ms against 0.376 at U = 8, 3 waves)
#endif
#ifndef MPH_UB
#define MPH_UB 8
#endif
#ifndef MPH_PASS_A_REV
#define MPH_PASS_A_REV 1
#endif
// The rows of a lane's list (RowMask): the lane walks rows [0, end); a row that holds no entry of
// it (a gap of its row jumps, or past its end) gathers nothing and is not summed.
// The batch of U rows from k0: the entries' loads first, then which rows hold entries (bits_of(),
// from the lane's mask in LDS or registers) -- so the loads are in flight while the bits are formed
// S16 (a short wave, mph_params.h kOff16Bits): jj is the entry's offset from its group's base and
// sb[u] row k0 + u's base scaled to the gather stride (GroupWalk; scalars), j0[u] the base itself
template <int U, bool S16, typename Bits>
__device__ __forceinline__ void list_batch(const NbrList& NL, Bits bits_of, int k0, int end,
                                           bool (&ok)[U], int (&jj)[U], int (&TT)[U], GroupWalk& W,
                                           unsigned (&sb)[U], int (&j0)[U])
{
    int e[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if constexpr (S16) nbr_at16(NL, k0 + u < end ? k0 + u : end - 1, e[u], TT[u]);
        else nbr_at(NL, k0 + u < end ? k0 + u : end - 1, e[u], TT[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if constexpr (S16) {
            W.seek(k0 + u);
            sb[u] = W.sb;
            j0[u] = W.j0;
        } else {
            sb[u] = 0u;
            j0[u] = 0;
        }
    }
    const unsigned bits = bits_of();
#pragma unroll
    for (int u = 0; u < U; ++u) {
        ok[u] = (bits & (1u << u)) != 0;
        jj[u] = e[u];
    }
}

template <bool FAST, int DIM, bool EQR, bool LEAN, bool S16 = false, int U = MPH_UA>
__device__ __forceinline__ void pass_a_loop(const DevParams& P, const double* s_ratio, const double* s_mu,
                                            const Soa& A,
                                            NbrList NL, bool plain, const unsigned* lm, int end, int ti,
                                            bool solid, double xi, double yi, double zi, double vxi, double vyi,
                                            double vzi, PassA& o, GroupWalk W = GroupWalk{})
{
    const __amdgpu_buffer_rsrc_t p6r = sized_rsrc(A.p6, (unsigned)P.n * 48u);
    for (int k0 = 0; k0 < end; k0 += U) {
        int jj[U];
        double X[U], Y[U], Z[U], VX[U], VY[U], VZ[U];
        int TT[U];
        bool ok[U];
        unsigned sb[U];
        int j0[U];
        list_batch<U, S16>(NL, [&] { return plain ? bit_range(0, end - k0) : row_bits_lds(lm, k0, end); }, k0, end,
                           ok, jj, TT, W, sb, j0);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            // a row without an entry of the lane (a gap, or past its end) reads past the buffer:
            // zeros, no cache lookup
            // (S16: the offset within the group times the stride plus the group's scaled base, a scalar)
            const unsigned off = ok[u] ? (S16 ? (unsigned)jj[u] * 48u + sb[u] : (unsigned)jj[u] * 48u) : kGatherOob;
            const double2 a = buf_ld16(p6r, off), b = buf_ld16(p6r, off + 16u), c = buf_ld16(p6r, off + 32u);
            X[u] = a.x; Y[u] = a.y; Z[u] = b.x;
            VX[u] = b.y; VY[u] = c.x; VZ[u] = c.y;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            // the gathered values used on every path, so that hipcc does not sink a row's loads into
            // its `ok` branch (issued there, late, they would not overlap the batch's other loads)
            asm volatile("" ::"v"(X[u]), "v"(Y[u]), "v"(Z[u]), "v"(VX[u]), "v"(VY[u]), "v"(VZ[u]));
            if (!ok[u]) continue;
            const double q0 = image_exact<FAST>(X[u] - xi, P.dw[0], P.hw[0], P.w075[0]);
            const double q1 = image_exact<FAST>(Y[u] - yi, P.dw[1], P.hw[1], P.w075[1]);
            const double q2 = image_exact<FAST || DIM == 2>(Z[u] - zi, P.dw[2], P.hw[2], P.w075[2]);
            pass_a_term<true, EQR, LEAN>(P, s_ratio, s_mu, ti, TT[u], solid, q0, q1, q2, r2_exact(q0, q1, q2),
                                         VX[u] - vxi, VY[u] - vyi, VZ[u] - vzi, o);
        }
    }
}

#ifndef MPH_PA_WPE
#define MPH_PA_WPE 4   // pass A at <= 128 VGPRs: 4 waves per SIMD
#endif
#if MPH_PA_WPE
#define MPH_PA_ATTR __attribute__((amdgpu_waves_per_eu(MPH_PA_WPE)))
#else
#define MPH_PA_ATTR
#endif
// LEAN: a lean step's pass A (pass_a_term; pout.gx and pout.dens_a are null), a kernel of its own, so
// that the full one keeps its code.
template <int DIM, bool LEAN = false>
__global__ __launch_bounds__(MPH_LB) MPH_PA_ATTR void k_pass_a(DevParams P, const DevTables* __restrict__ T, Soa A,
                                                const int* __restrict__ nbr,
                                                const int* __restrict__ ncount,
                                                const unsigned long long* __restrict__ lhdr,
                                                const unsigned long long* __restrict__ lgap, PassAOut pout,
                                                const DevState* __restrict__ st,
                                                unsigned char* __restrict__ cmap, int cmap_bytes,
                                                const int* __restrict__ lbase)
{
    const int n = dev_n(P);
    // counted like the lazy steps in the search (one writer; st is written by no other kernel of
    // the step from here on)
    if (LEAN && blockIdx.x == 0 && threadIdx.x == 0) const_cast<DevState*>(st)->lean_pass_a_steps += 1;
    // a lazy wall step (cmap set): its search, the coarse map's only reader, is done -- back to
    // all zero for the next step's k_prep, 16 bytes per thread of the grid's first blocks
    if (cmap)
        for (int q = blockIdx.x * MPH_LB + threadIdx.x; q * 16 < cmap_bytes; q += gridDim.x * MPH_LB)
            reinterpret_cast<int4*>(cmap)[q] = make_int4(0, 0, 0, 0);
    const int lb = list_block(st, n, MPH_PASS_A_REV);
    if (lb < 0) return;
    __shared__ double s_ratio[kTypes * kTypes];
    __shared__ double s_mu[kTypes * kTypes];
    if (threadIdx.x < kTypes * kTypes) {
        s_ratio[threadIdx.x] = T->ratio[threadIdx.x];
        s_mu[threadIdx.x] = T->mu_ij[threadIdx.x] * (-P.cvis * P.cdv * P.vol);   // pass_a_term's viscous factor
    }
    __syncthreads();
    const int i = lb * blockDim.x + threadIdx.x;
    const bool live = i < n;
    const int ii = live ? i : n - 1;
    const double xi = A.x[ii], yi = A.y[ii], zi = A.z[ii];
    if (wave_all_ghosts(P, A, live, ii)) {
        // ghosts: PressureP (+ GravityCenter, PressureA) arrive in the halo, which also fills the
        // .w of the pass-B record; its position part is written here
        if (live && pout.rec) rec_store(pout.rec, P.n, i, xi, yi, zi, 0.0);
        return;
    }
    // likewise the ghost lanes of a mixed wave
    const bool ghost = live && P.slab_axis >= 0 && A.id[ii] < 0;
    if (ghost && pout.rec) rec_store(pout.rec, P.n, i, xi, yi, zi, 0.0);
    const bool own = live && !ghost;
    // the search's rule (its list order and the fast minimum image go together)
    const bool fast = wave_search_interior(P, st, own, xi, yi, zi);
    if (!own) return;
    double vxi, vyi, vzi;
    own_velocity(A, i, vxi, vyi, vzi);
    const int ti = A.type[i];
    const bool solid = dev_is_struct(ti);
    const int end = ncount[i] < kTileRows ? ncount[i] : kTileRows;
    __shared__ unsigned s_mask[kWB][kTile * kMaskWords];
    unsigned* lm = &s_mask[threadIdx.x >> 6][(threadIdx.x & 63) * kMaskWords];
    // a wave without jumps (plain rows: on the lattice, in 2-D) needs no mask, only its lanes' ends
    const unsigned long long hdr = wave_hdr(lhdr, i);
    const bool plain = gap_count(hdr) == 0;
    if (!plain) mask_to_lds(lm, row_mask(hdr, lgap, i, end));   // (each lane reads back only its own)
    const NbrList NL = nbr_list(nbr, i);
    PassA o;
    // wave-uniform: equal radii (every BASELINE config) take the single-cutoff form of the sums in
    // the interior waves; waves at a periodic face keep the general form
    const bool eqr = pass_a_equal_radii(P);
    // a short wave (interior, 3-D): the same loops over its 16-bit rows
    if (DIM == 3 && hdr_short(hdr)) {
        GroupWalk W;
        W.init(lbase, i, hdr, 48);
        if (eqr)
            pass_a_loop<true, DIM, true, LEAN, true>(P, s_ratio, s_mu, A, NL, plain, lm, end, ti, solid, xi, yi, zi, vxi,
                                                     vyi, vzi, o, W);
        else
            pass_a_loop<true, DIM, false, LEAN, true>(P, s_ratio, s_mu, A, NL, plain, lm, end, ti, solid, xi, yi, zi, vxi,
                                                      vyi, vzi, o, W);
    } else if (fast && eqr)
        pass_a_loop<true, DIM, true, LEAN>(P, s_ratio, s_mu, A, NL, plain, lm, end, ti, solid, xi, yi, zi, vxi, vyi,
                                           vzi, o);
    else if (fast)
        pass_a_loop<true, DIM, false, LEAN>(P, s_ratio, s_mu, A, NL, plain, lm, end, ti, solid, xi, yi, zi, vxi, vyi,
                                            vzi, o);
    else
        pass_a_loop<false, DIM, false, LEAN>(P, s_ratio, s_mu, A, NL, plain, lm, end, ti, solid, xi, yi, zi, vxi, vyi,
                                             vzi, o);
    pass_a_finish(P, T, ti, i, o, pout, xi, yi, zi);
}

// ---------------------------------------------------------------------------- pass B -------

// Pass B needs, per neighbour, only what pass A could not know: P_j (and, with surface tension,
// GC_j and PA_j).  The P_i half of the pressure force and the viscous force were summed in pass A
// (fpart), so the gather per neighbour is one 32-byte record {x, y, z, P} (two 16-byte planes,
// rec_load); the type of j (in the list entry) only for structure i (InterfaceForce) or surface
// tension.
// One neighbour's pair forces for pass B (see k_pass_b): PressureP's P_j half, and with surface
// tension PressureA and DiffuseInterface; structure i takes non-structure j only.
template <bool FAST, bool SURF, int DIM>
__device__ __forceinline__ void pass_b_term(const DevParams& P, const double* s_ratio, const double* gx,
                                            const double* gy, const double* gz, const double* pa, int j, int tj,
                                            double X, double Y, double Z, double PJ, int ti, bool solid,
                                            double xi, double yi, double zi, double gxi, double gyi, double gzi,
                                            double pai, double ai, double dscale, double cpv, double& f0,
                                            double& f1, double& f2)
{
    if (solid && dev_is_struct(tj)) return;
    const double q0 = image_exact<FAST>(X - xi, P.dw[0], P.hw[0], P.w075[0]);
    const double q1 = image_exact<FAST>(Y - yi, P.dw[1], P.hw[1], P.w075[1]);
    const double q2 = image_exact<FAST || DIM == 2>(Z - zi, P.dw[2], P.hw[2], P.w075[2]);
    const double r2 = r2_exact(q0, q1, q2);
    if (!SURF || solid) {
        if (r2 < P.rp2) {
            double r, ir;
            rsqrt_pair(r2, r, ir);
            // dw_p(r) / r = cdp (1 - r / rp) / r = cdp (1/r - 1/rp): r itself is not needed
            const double c = PJ * cpv * (ir - P.inv_rp);
            f0 += c * q0;
            f1 += c * q1;
            f2 += c * q2;
        }
        return;
    }
    double r, ir;
    rsqrt_pair(r2, r, ir);
    double c = 0.0;
    if (r2 < P.rp2) c += PJ * (cpv * (1.0 - r * P.inv_rp)) * ir;
    const double rij = s_ratio[ti * kTypes + tj];
    const double rji = s_ratio[tj * kTypes + ti];
    const double gxj = gx[j], gyj = gy[j], gzj = gz[j], paj = pa[j];
    if (r2 < P.ra2) {
        const double t = r * P.inv_ra;
        const double dwa = P.cda * (1.0 - t) * (1.0 - 3.0 * t);
        c += (pai * rij + paj * rji) * dwa * ir * P.vol;
    }
    if (r2 < P.rg2) {
        const double omt = 1.0 - r * P.inv_rg;
        const double wg = P.cg * omt * omt;
        const double dwg = P.cdg * omt;
        const double wij = rij * wg, wji = rji * wg;
        f0 -= (ai * gxj * wji - ai * gxi * wij) * dscale;
        f1 -= (ai * gyj * wji - ai * gyi * wij) * dscale;
        f2 -= (ai * gzj * wji - ai * gzi * wij) * dscale;
        const double dwij = rij * dwg, dwji = rji * dwg;
        const double gr = (ai * gxj * dwji - ai * gxi * dwij) * q0 +
                          (ai * gyj * dwji - ai * gyi * dwij) * q1 +
                          (ai * gzj * dwji - ai * gzi * dwij) * q2;
        c -= gr * ir * dscale;
    }
    f0 += c * q0;
    f1 += c * q1;
    f2 += c * q2;
}

template <bool FAST, bool SURF, int DIM, bool S16 = false, int U = MPH_UB>
__device__ __forceinline__ void pass_b_loop(const DevParams& P, const double* s_ratio,
                                            const double4* rec, const double* gx,
                                            const double* gy, const double* gz, const double* pa,
                                            NbrList NL, bool plain, const RowMask& M, int end, int ti, bool solid,
                                            double xi, double yi, double zi, double gxi, double gyi, double gzi,
                                            double pai, double ai, double& f0, double& f1, double& f2,
                                            GroupWalk W = GroupWalk{})
{
    const double dscale = P.rg_r2g * (P.vol / P.dx);
    const double cpv = P.cdp * P.vol;
    // the record's two planes {x, y} at [j], {z, P} at [ps + j] (rec_load), 16 bytes each
    const unsigned ps16 = (unsigned)P.n * 16u;
    const __amdgpu_buffer_rsrc_t recr = sized_rsrc(rec, 2u * ps16);
    for (int k0 = 0; k0 < end; k0 += U) {
        int jj[U];
        double X[U], Y[U], Z[U], PJ[U];
        int TT[U];
        bool ok[U];
        unsigned sb[U];
        int j0[U];
        list_batch<U, S16>(NL, [&] { return plain ? bit_range(0, end - k0) : row_bits(M, k0, end); }, k0, end, ok, jj,
                           TT, W, sb, j0);
#pragma unroll
        for (int u = 0; u < U; ++u) {   // (rows without an entry: past the buffer, as in pass_a_loop)
            const unsigned off = ok[u] ? (S16 ? (unsigned)jj[u] * 16u + sb[u] : (unsigned)jj[u] * 16u) : kGatherOob;
            const double2 a = buf_ld16(recr, off), b = buf_ld16(recr, off == kGatherOob ? off : off + ps16);
            X[u] = a.x; Y[u] = a.y; Z[u] = b.x; PJ[u] = b.y;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            asm volatile("" ::"v"(X[u]), "v"(Y[u]), "v"(Z[u]), "v"(PJ[u]));   // (see pass_a_loop)
            if (!ok[u]) continue;
            pass_b_term<FAST, SURF, DIM>(P, s_ratio, gx, gy, gz, pa, S16 ? jj[u] + j0[u] : jj[u], TT[u], X[u], Y[u], Z[u], PJ[u], ti,
                                         solid, xi, yi, zi, gxi, gyi, gzi, pai, ai, dscale, cpv, f0, f1, f2);
        }
    }
}

// What pass B's KEYS form writes for the next step's sort: key and slot per particle, the cell
// histogram, the coarse map where that step is lazy (else null).
struct KeyOut {
    int *key, *slot, *cnt;
    unsigned char* cmap;
};

// Pair forces of PressureP (2394-2424), PressureA (2225-2258), DiffuseInterface (2261-2312),
// ViscosityV (2478-2522) for non-structure i; InterfaceForce (2439-2472) for structure i; then
// Gravity (2917-2936), Acceleration/kick (2938-2956) and Convection/drift (1892-1907).  The sums
// start from pass A's fpart (P_i half of the pressure force + viscous force).
// KEYS (the key fold, mph_kernels.h seq_step; single contexts without structure particles): the
// kernel ends with the next step's k_prep on the values it is about to store -- the same
// move_and_wrap, prep_cell and prep_slot (mph_device.h), so the same bits -- and leaves key, slot, the cell
// histogram, the non-finite flag, the face bits and (cmap set: the next step is lazy) the coarse
// map.  This step's k_place has advanced Time, WallCenter and seam_step, its k_scan_down has
// re-zeroed cnt and its pass A has cleared the map, so the tail sees what that k_prep would.  The
// run detection needs every lane of the wave, so the lanes past n stay to the end -- they read
// particle n - 1's entries (ir) and store nothing -- and no barrier follows the list loop: the face
// bits are reduced per wave.
template <bool SURF, int DIM, bool KEYS = false>
#ifndef MPH_PB_WPE
#define MPH_PB_WPE 0   // pass B occupancy hint (0: the compiler's choice, 112 VGPRs / 4 waves at U = 8)
#endif
#if MPH_PB_WPE
#define MPH_PB_ATTR __attribute__((amdgpu_waves_per_eu(MPH_PB_WPE)))
#else
#define MPH_PB_ATTR
#endif
__global__ __launch_bounds__(MPH_LB) MPH_PB_ATTR void k_pass_b(DevParams P, const DevTables* __restrict__ T, Soa A,
                                                const double4* __restrict__ rec,
                                                const double4* __restrict__ fpart,
                                                const double* __restrict__ gx,
                                                const double* __restrict__ gy,
                                                const double* __restrict__ gz,
                                                const double* __restrict__ pa,
                                                const int* __restrict__ nbr,
                                                const int* __restrict__ ncount,
                                                const unsigned long long* __restrict__ lhdr,
                                                const unsigned long long* __restrict__ lgap,
                                                double4* __restrict__ force, double4* __restrict__ acc,
                                                Soa B, int phase, int* __restrict__ wface, StructHook H,
                                                const DevState* __restrict__ st, KeyOut K,
                                                const int* __restrict__ lbase)
{
    const int n = dev_n(P);
    const int lb = list_block(st, n);
    if (lb < 0) return;
    if (KEYS && lb == 0 && threadIdx.x == 0) const_cast<DevState*>(st)->key_fold_steps += 1;
    __shared__ double s_ratio[kTypes * kTypes];
    if (SURF) {
        if (threadIdx.x < kTypes * kTypes) s_ratio[threadIdx.x] = T->ratio[threadIdx.x];
        __syncthreads();
    }
    const int i = lb * blockDim.x + threadIdx.x;
    const int ii = i < n ? i : n - 1;
    const double xi = A.x[ii], yi = A.y[ii], zi = A.z[ii];
    bool live = i < n;
    if (phase) {
        // slab mode: phase 1 = the waves without a particle near a face (run while the halo of
        // pass-A values is in flight; also the waves of ghosts only), phase 2 = the rest, after the
        // halo arrived -- split by whole waves (wface, written by the search), so that no wave runs
        // its list loop twice
        const int f = wface[__builtin_amdgcn_readfirstlane(i >> 6)];
        if (phase == 1 ? f != 0 : f == 0) return;
    }
    if (wave_all_ghosts(P, A, live, ii)) {
        if (live) B.id[i] = A.id[i];
        return;
    }
    if (live && P.slab_axis >= 0 && A.id[ii] < 0) {   // a ghost lane of a mixed wave
        B.id[i] = A.id[i];
        live = false;
    }
    const bool fast = wave_search_interior(P, st, live, xi, yi, zi);
    if (!KEYS && !live) return;
    if (KEYS && !__any(live)) return;
    const int ir = KEYS ? ii : i;   // the entry this lane reads
    const int ti = A.type[ii];
    const bool solid = dev_is_struct(ti);
    const double4 fp = fpart[ii];
    double f0 = fp.x, f1 = fp.y, f2 = fp.z;
    double gxi = 0.0, gyi = 0.0, gzi = 0.0, pai = 0.0, ai = 0.0;
    if (SURF) {
        gxi = gx[ii]; gyi = gy[ii]; gzi = gz[ii]; pai = pa[ii];
        ai = T->cofa[ti] * P.cofk * P.cofk;
    }
    // a wall's pair forces only go to the Force output (walls are not kicked or drifted, K17/K18):
    // on the steps that do not store it (force null, enqueue_step) its list loop is skipped
    const int end = !force && dev_is_wall(ti) ? 0 : (ncount[ir] < kTileRows ? ncount[ir] : kTileRows);
    const unsigned long long hdr = wave_hdr(lhdr, ir);
    const bool plain = gap_count(hdr) == 0;   // no gaps: rows [0, end) (see k_pass_a)
    const RowMask M = row_mask(hdr, lgap, ir, end);
    const NbrList NL = nbr_list(nbr, ir);
    if (DIM == 3 && hdr_short(hdr)) {   // a short wave (interior): the same loop over its 16-bit rows
        GroupWalk W;
        W.init(lbase, ir, hdr, 16);
        pass_b_loop<true, SURF, DIM, true>(P, s_ratio, rec, gx, gy, gz, pa, NL, plain, M, end, ti, solid, xi, yi, zi,
                                           gxi, gyi, gzi, pai, ai, f0, f1, f2, W);
    } else if (fast)
        pass_b_loop<true, SURF, DIM>(P, s_ratio, rec, gx, gy, gz, pa, NL, plain, M, end, ti, solid, xi, yi, zi, gxi,
                                     gyi, gzi, pai, ai, f0, f1, f2);
    else
        pass_b_loop<false, SURF, DIM>(P, s_ratio, rec, gx, gy, gz, pa, NL, plain, M, end, ti, solid, xi, yi, zi, gxi,
                                      gyi, gzi, pai, ai, f0, f1, f2);
    double vxi, vyi, vzi;
    own_velocity(A, ir, vxi, vyi, vzi);
    double vo0 = vxi, vo1 = vyi, vo2 = vzi;
    double xo0 = xi, xo1 = yi, xo2 = zi;
    double4 ao = make_double4(0.0, 0.0, 0.0, 0.0);
    if (dev_is_fluid(ti) || solid) {
        const double m = T->mass[ti], im = T->inv_mass[ti];
        f0 += m * P.gravity[0];
        f1 += m * P.gravity[1];
        f2 += m * P.gravity[2];
        vo0 += f0 * im * P.dt;
        vo1 += f1 * im * P.dt;
        vo2 += f2 * im * P.dt;
        if (!solid) {
            ao = make_double4(f0 * im, f1 * im, f2 * im, 0.0);
            xo0 += vo0 * P.dt;
            xo1 += vo1 * P.dt;
            xo2 += vo2 * P.dt;
        }
    }
    if (KEYS) {
        // (force is null and no particle is a structure's: launch_pass_b)
        const int lane = threadIdx.x & 63;
        int k = -1 - lane;   // the lanes past n: runs of their own, as in k_prep
        int occ = 0;
        if (live) {
            B.vx[i] = vo0;
            B.vy[i] = vo1;
            B.vz[i] = vo2;
            B.type[i] = ti;
            B.id[i] = A.id[i];
            double x = xo0, y = xo1, z = xo2;
            move_and_wrap(P, st, B, i, x, y, z);   // (reads the type just stored; stores the position)
            k = prep_cell(P, st, x, y, z, &K.key[i], K.cmap, [&] { return !dev_is_wall(ti); }, occ);
        }
        // one histogram atomic per run of equal keys (prep_slot)
        const int s = prep_slot(k, live, K.cnt);
        if (live) K.slot[i] = s;
        // the wave's face bits: one device atomic, only for bits the next step's word does not hold
        if (__ballot(occ != 0)) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) occ |= __shfl_xor(occ, o, 64);
            if (lane == 0) {
                int* w = const_cast<int*>(&st->seam_occ[st->seam_step & 1]);
                const int cur = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (occ & ~cur) atomicOr(w, occ);
            }
        }
        return;
    }
    if (force) {   // null on all but the last step of a replayed batch (enqueue_step)
        force[i] = make_double4(f0, f1, f2, 0.0);
        acc[i] = ao;
    }
    B.x[i] = xo0;
    B.y[i] = xo1;
    B.z[i] = xo2;
    B.vx[i] = vo0;
    B.vy[i] = vo1;
    B.vz[i] = vo2;
    B.type[i] = ti;
    B.id[i] = A.id[i];
    const int id = A.id[i];
    if (solid && H.slot_of && id >= 0) {
        // the elastic substeps' slot-ordered state (structure particles do not drift here);
        // slab mode: slots of owned particles only (ghost ids are negative)
        const int s = H.slot_of[id];
        if (s >= 0) {
            const double4 x4 = make_double4(xo0, xo1, xo2, (double)ti);
            H.sx[s] = x4;
            H.sv[s] = make_double4(vo0, vo1, vo2, 0.0);
            H.su[s] = struct_disp(P, x4, H.sx0[s]);
            H.bidx[s] = i;
        }
    }
}

// ------------------------------------------------------------------------ virial stress ----

// calculateVirialStressAtParticle (main.cpp:3077-3318) for particle i of the current (post-step)
// state: B holds the integrated positions and velocities in A order, the list and the pass-A
// products (PressureP, PressureA, GravityCenter) are this step's.  The reference's four pair
// loops (PressureP 3093-3125, PressureA 3127-3163, viscosity 3165-3206, diffuse interface
// 3208-3282) are one sweep here; every term keeps its own radius test.  All particles, any type.
template <int DIM>
__global__ __launch_bounds__(256) void k_virial(DevParams P, const DevTables* __restrict__ T, Soa A, Soa B,
                                                const double* __restrict__ pres, const double* __restrict__ pa,
                                                const double* __restrict__ gx, const double* __restrict__ gy,
                                                const double* __restrict__ gz, const int* __restrict__ nbr,
                                                const int* __restrict__ ncount,
                                                const unsigned long long* __restrict__ lhdr,
                                                const unsigned long long* __restrict__ lgap,
                                                double* __restrict__ vir, double* __restrict__ vpres,
                                                const int* __restrict__ lbase)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= dev_n(P)) return;
    if (P.slab_axis >= 0 && A.id[i] < 0) return;   // slab mode: a ghost (its owner computes it)
    const int ti = A.type[i];
    const double xi = B.x[i], yi = B.y[i], zi = B.z[i];
    const double vxi = B.vx[i], vyi = B.vy[i], vzi = B.vz[i];
    const double pi = pres[i], pai = pa[i];
    const double gi[3] = {gx[i], gy[i], gz[i]};
    const double a = T->cofa[ti] * P.cofk * P.cofk;
    const double dscale = P.rg_r2g * (P.vol / P.dx);
    const double cvis = DIM == 2 ? 8.0 : 10.0;
    double S[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    const int end = ncount[i] < kTileRows ? ncount[i] : kTileRows;
    const unsigned long long hdr = lhdr[i >> 6];
    const RowMask M = row_mask(hdr, lgap, i, end);
    const int* row = ell_row(nbr, i);
    const bool s16 = hdr_short(hdr);   // 16-bit rows: the entry's offset on its group's base
    const unsigned short* row16 = reinterpret_cast<const unsigned short*>(nbr + (size_t)(i >> 6) * kTileStride);
    for (int k = 0; k < end; ++k) {
        if (!row_ok(M, k, end)) continue;
        int j, tj;
        if (s16) {
            const unsigned e = row16[ell_slot(k, (int)(i & 63))];
            j = entry16_off(e) + lbase[(size_t)(i >> 6) * kBaseInts + row_group(hdr, k)];
            tj = entry16_type(e);
        } else {
            const int e = *ell_at(row, (int)(i & 63), k);
            j = e & kIndexMask;
            tj = e >> kTypeShift;
        }
        double q[3];
        q[0] = image_exact<false>(B.x[j] - xi, P.dw[0], P.hw[0], P.w075[0]);
        q[1] = image_exact<false>(B.y[j] - yi, P.dw[1], P.hw[1], P.w075[1]);
        q[2] = image_exact<DIM == 2>(B.z[j] - zi, P.dw[2], P.hw[2], P.w075[2]);
        const double r2 = r2_exact(q[0], q[1], q[2]);
        if (!(r2 < P.rp2 || r2 < P.ra2 || r2 < P.rv2 || r2 < P.rg2)) continue;
        const double r = sqrt(r2), ir = 1.0 / r;
        const double ratio = T->ratio[ti * kTypes + tj];
        // pair force f_ij = c q_ij + g1 (every term is along q_ij except the first
        // diffuse-interface term); the virial adds f_ij (x) q_ij / V
        double c = 0.0;
        if (r2 < P.rp2) c += pi * (P.cdp * (1.0 - r * P.inv_rp)) * ir * P.vol;          // 3111-3120
        if (r2 < P.ra2) {                                                                // 3147-3156
            const double t = r * P.inv_ra;
            c += pai * (ratio * (P.cda * (1.0 - t) * (1.0 - 3.0 * t))) * ir * P.vol;
        }
        if (r2 < P.rv2) {                                                                // 3183-3199 (x 0.5)
            const double dv = (B.vx[j] - vxi) * q[0] + (B.vy[j] - vyi) * q[1] + (B.vz[j] - vzi) * q[2];
            const double dwij = -(P.cdv * (1.0 - r * P.inv_rv));
            c += 0.5 * (cvis * T->mu_ij[ti * kTypes + tj] * dv * dwij * (ir * ir * ir) * P.vol);
        }
        double g1[3] = {0.0, 0.0, 0.0};
        if (r2 < P.rg2) {                                                                // 3225-3276
            const double omt = 1.0 - r * P.inv_rg;
            const double w = ratio * (P.cg * omt * omt);
            const double dw = ratio * (P.cdg * omt);
            const double gr = -(gi[0] * q[0] + gi[1] * q[1] + gi[2] * q[2]);
            for (int d = 0; d < 3; ++d) g1[d] = a * gi[d] * w * dscale;                 // -a (-GC_i) w
            c += -a * gr * dw * ir * dscale;
        }
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
            for (int v = 0; v < 3; ++v) S[u][v] += (c * q[u] + g1[u]) * q[v] / P.vol;
    }
    double* o = vir + (size_t)i * 9;
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int v = 0; v < 3; ++v) o[3 * u + v] = S[u][v];
    vpres[i] = DIM == 2 ? -1.0 / 2.0 * (S[0][0] + S[1][1]) : -1.0 / 3.0 * (S[0][0] + S[1][1] + S[2][2]);
}

// ---------------------------------------------------------------------------- launchers -----

static PassAOut pass_a_out(const Launch& L)
{
    return PassAOut{L.pres, L.gx, L.gy, L.gz, L.pa, L.dens_a, L.vstrain, L.divp, L.fpart, L.rec};
}

void launch_pass_a(const Launch& L)
{
    const DevParams& P = *L.P;
    if (P.n == 0) return;
    // a lean step stores neither GravityCenter / PressureA nor the diagnostics (seq_step) and
    // leaves their sums out
    by_flag(L.form.lean_pass_a, [&](auto LEAN) {
        by_dim(P.dim, [&](auto D) {
            launch(L.prof, "pass_a", L.stream, k_pass_a<decltype(D)::value, decltype(LEAN)::value>,
                   dim3(list_grid(P.n, lazy_bal(L))), dim3(MPH_LB), P, L.T, L.A, L.nbr, L.ncount, L.lhdr, L.lgap,
                   pass_a_out(L), L.st, lazy_cmap(L), L.cmap_bytes, L.lbase);
        });
    });
}

// calculateNeighbor + the pass-A sums
void launch_search_pass_a(const Launch& L)
{
    launch_neighbors(L);
    launch_pass_a(L);
}

static StructHook struct_hook(const Launch& L)
{
    StructHook h{};
    if (L.P->n_struct > 0 && L.S && L.S->slot_of) {
        h.slot_of = L.S->slot_of;
        h.sx = L.S->x;
        h.sv = L.S->v;
        h.su = L.S->u;
        h.sx0 = L.S->x0;
        h.bidx = L.S->bidx;
    }
    return h;
}

void launch_pass_b(const Launch& L, int phase)
{
    const DevParams& P = *L.P;
    if (P.n == 0) return;
    // pass B reads GravityCenter and PressureA of every neighbour with surface tension; trim_outputs
    // leaves them unstored on the non-last steps of a batch only without it
    if (P.surface && !(L.gx && L.gy && L.gz && L.pa)) {
        std::fprintf(stderr, "mph: launch_pass_b with surface tension needs GravityCenter/PressureA\n");
        std::abort();
    }
    // the key fold (seq_step): never on a step that stores Force, with structure particles, in a
    // slab's phases or on a slab's set
    const bool keys = L.form.keys_next;
    if (keys && (L.force || P.n_struct > 0 || phase || P.slab_axis >= 0 || P.n_dev)) {
        std::fprintf(stderr, "mph: launch_pass_b: the key fold on a step that cannot take it\n");
        std::abort();
    }
    by_flag(P.surface, [&](auto SURF) {
        by_flag(keys, [&](auto KEYS) {
            by_dim(P.dim, [&](auto D) {
                launch(L.prof, phase == 2 ? "pass_b_face" : "pass_b", L.stream,
                       k_pass_b<decltype(SURF)::value, decltype(D)::value, decltype(KEYS)::value>,
                       dim3(list_grid(P.n, lazy_bal(L))), dim3(MPH_LB), P, L.T, L.A, L.rec, L.fpart, L.gx, L.gy, L.gz,
                       L.pa, L.nbr, L.ncount, L.lhdr, L.lgap, L.force, L.acc, L.B, phase, L.wface, struct_hook(L),
                       L.st, keys ? KeyOut{L.key, L.slot, L.cnt, L.cmap_next} : KeyOut{}, L.lbase);
            });
        });
    });
}

void launch_virial(const Launch& L, const Soa& X, double* vir, double* vpres)
{
    const DevParams& P = *L.P;
    if (P.n == 0) return;
    by_dim(P.dim, [&](auto D) {
        launch(L.prof, "virial", L.stream, k_virial<decltype(D)::value>, dim3(blocks(P.n, 256)), dim3(256), P, L.T,
               L.A, X, L.pres, L.pa, L.gx, L.gy, L.gz, L.nbr, L.ncount, L.lhdr, L.lgap, vir, vpres, L.lbase);
    });
}

}  // namespace mph
