// mph_kinematics.hip -- velocity gradient, vorticity and free-surface fields (include/mph_gpu.h
// MphKinematics): an on-demand pass over the step's neighbour lists next to k_virial, outside every
// step graph; no kernel of a step is touched.
//
//   k_kinematics<DIM>   one lane per particle in list order: the sums of kin_pair over the lane's
//                       list, then kin_finish (both mph_params.h, shared with the host's
//                       mph_kinematics_arrays), the record stored as 24 consecutive doubles
//   k_kin_gather        out[r][e] = kin[slot[r]][e]: the selection's rows
#include <hip/hip_runtime.h>

#include "mph_device.h"
#include "mph_kernels.h"
#include "mph_list.h"
#include "mph_params.h"

namespace mph {

// Position and velocity of particle j of the state in list order.  After a step that is the integrated
// set B, whose component arrays are in A order; before the first step it is the sorted set A itself,
// whose velocities a single context keeps only in the 48-byte records {x, y}, {z, vx}, {vy, vz}
// (k_rank_scatter) -- the positions there are the bits of A.x, A.y, A.z.
template <bool REC> struct KinState {
    double x, y, z, vx, vy, vz;
    __device__ __forceinline__ void position(const Soa& X, int j)
    {
        if (REC) {
            const double2 a = X.p6[3 * (size_t)j], b = X.p6[3 * (size_t)j + 1], c = X.p6[3 * (size_t)j + 2];
            x = a.x; y = a.y; z = b.x; vx = b.y; vy = c.x; vz = c.y;
        } else {
            x = X.x[j]; y = X.y[j]; z = X.z[j];
        }
    }
    __device__ __forceinline__ void velocity(const Soa& X, int j)
    {
        if (!REC) { vx = X.vx[j]; vy = X.vy[j]; vz = X.vz[j]; }
    }
};

// X: the state in list (A) order (KinState).  The row walk is k_virial's: the gaps of the row jumps
// (row_mask / row_ok), 32-bit entries, and 16-bit entries on the wave's group bases.
template <int DIM, bool REC>
__global__ __launch_bounds__(256) void k_kinematics(DevParams P, Soa X, const int* __restrict__ nbr,
                                                    const int* __restrict__ ncount,
                                                    const unsigned long long* __restrict__ lhdr,
                                                    const unsigned long long* __restrict__ lgap,
                                                    const int* __restrict__ lbase, KinDev K, double* __restrict__ out)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= dev_n(P)) return;
    KinState<REC> si;
    si.position(X, i);
    si.velocity(X, i);
    const double xi = si.x, yi = si.y, zi = si.z;
    const double vxi = si.vx, vyi = si.vy, vzi = si.vz;
    KinAcc<DIM> acc;
    const int end = ncount[i] < kTileRows ? ncount[i] : kTileRows;
    const unsigned long long hdr = lhdr[i >> 6];
    const RowMask M = row_mask(hdr, lgap, i, end);
    const int* row = ell_row(nbr, i);
    const bool s16 = hdr_short(hdr);
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
        if (!kin_class(K.mask, tj)) continue;
        KinState<REC> sj;
        sj.position(X, j);
        double q[3];
        q[0] = image_exact<false>(sj.x - xi, P.dw[0], P.hw[0], P.w075[0]);
        q[1] = image_exact<false>(sj.y - yi, P.dw[1], P.hw[1], P.w075[1]);
        q[2] = DIM == 3 ? image_exact<false>(sj.z - zi, P.dw[2], P.hw[2], P.w075[2]) : 0.0;
        const double r2 = r2_exact(q[0], q[1], q[2]);
        if (!(r2 < P.rc2)) continue;   // (far outside every legal h: no gather of the velocity)
        sj.velocity(X, j);
        const double dv[3] = {sj.vx - vxi, sj.vy - vyi, DIM == 3 ? sj.vz - vzi : 0.0};
        kin_pair<DIM>(acc, K.h, q, r2, dv);
    }
    double o[MPH_KIN_CHANNELS];
    kin_finish<DIM>(acc, K, o);
    double2* dst = reinterpret_cast<double2*>(out + (size_t)i * MPH_KIN_CHANNELS);
#pragma unroll
    for (int k = 0; k < MPH_KIN_CHANNELS / 2; ++k) dst[k] = make_double2(o[2 * k], o[2 * k + 1]);
}

__global__ __launch_bounds__(256) void k_kin_gather(const double* __restrict__ kin, const int* __restrict__ slot,
                                                    int count, double* __restrict__ out)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)count * MPH_KIN_CHANNELS) return;
    const size_t r = t / MPH_KIN_CHANNELS, e = t % MPH_KIN_CHANNELS;
    out[t] = kin[(size_t)slot[r] * MPH_KIN_CHANNELS + e];
}

void launch_kinematics(const Launch& L, bool stepped, const KinDev& K, double* out)
{
    const DevParams& P = *L.P;
    if (P.n == 0) return;
    by_flag(!stepped, [&](auto REC) {
        by_dim(P.dim, [&](auto D) {
            launch(L.prof, "kinematics", L.stream, k_kinematics<decltype(D)::value, decltype(REC)::value>,
                   dim3(blocks(P.n, 256)), dim3(256), P, stepped ? L.B : L.A, L.nbr, L.ncount, L.lhdr, L.lgap, L.lbase, K,
                   out);
        });
    });
}

void launch_kin_gather(const Launch& L, const double* kin, const int* slot, int count, double* out)
{
    if (count <= 0) return;
    const long long total = (long long)count * MPH_KIN_CHANNELS;
    launch(L.prof, "kin_gather", L.stream, k_kin_gather, dim3((unsigned)((total + 255) / 256)), dim3(256), kin, slot, count,
           out);
}

}  // namespace mph
