// mph_slab.hip -- kernels of the slab decomposition (mph_dist.hip): the redistribution's classify /
// scatter / pack / unpack, the elastic ghost rows' pack / unpack and the halo's pack / unpack.
#include <algorithm>

#include "mph_list.h"

namespace mph {

// ------------------------------------------------------------------ slab decomposition -----
// Multi-GPU redistribution (mph_dist.hip).  Every B entry is classified by its slab coordinate
// after this step's wall motion + periodic wrap; a stable partition then writes the owned and
// outgoing particles into C as [migrate R | band R | inner | band L | migrate L] (ghosts of the
// previous step are dropped).  Migrants keep a copy here as ghosts (id -> -1-id).

__device__ __forceinline__ unsigned long long lanemask_lt() { return (1ull << (threadIdx.x & 63)) - 1ull; }

__device__ __forceinline__ bool dist_sends(int c) { return c == kMigR || c == kBandR || c == kBandL || c == kMigL; }
constexpr int kMsgHeader = 16;   // redistribution message header: the two class counts

// wface (early send, see k_dist_early_classify): the face wavefronts of the previous step, whose
// particles were moved and sent already -- not moved again here, and no other particle may be
// of a sending class (it would have moved more than the face margin: an error)
__global__ __launch_bounds__(256) void k_dist_classify(DevParams P, DevState* __restrict__ st, SlabGeom g,
                                                       Soa B, const DistLayout* __restrict__ lay, int move,
                                                       int* __restrict__ cls, int* __restrict__ bcnt, int nb,
                                                       const int* __restrict__ wface)
{
    __shared__ int wc[4][kSlabClasses];
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = lay->n;   // entries of B: the previous redistribution's count
    int c = -1;
    if (p < n) {
        if (B.id[p] < 0) {
            c = kSlabDrop;
        } else {
            const bool face = wface && wface[p >> 6] == 1;
            double x = B.x[p], y = B.y[p], z = B.z[p];
            if (move && !face) move_and_wrap(P, st, B, p, x, y, z);
            const double a = g.axis == 0 ? x : (g.axis == 1 ? y : z);
            c = dev_is_struct(B.type[p]) ? slab_class_static(g, a) : slab_class(g, a);
            if (c == kSlabLost) {
                atomicOr(&st->overflow, 2);
                c = kInner;
            }
            if (wface && !face && dist_sends(c)) atomicOr(&st->overflow, 8);
        }
        cls[p] = c;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kSlabClasses; ++k) {
        const unsigned long long m = __ballot(c == k);
        if (lane == 0) wc[wave][k] = __popcll(m);
    }
    __syncthreads();
    if (threadIdx.x < kSlabClasses) {
        int t = 0;
        for (int w = 0; w < 4; ++w) t += wc[w][threadIdx.x];
        bcnt[threadIdx.x * nb + blockIdx.x] = t;
    }
}

// Early send (mph_dist.hip): at the end of a step, once pass B has integrated the face wavefronts
// (wface, written by pass B), their owned particles are moved (calculateWall / periodic wrap, as
// k_dist_classify would at the next step) and classified; the others count as nothing here.
__global__ __launch_bounds__(256) void k_dist_early_classify(DevParams P, DevState* __restrict__ st, SlabGeom g,
                                                             Soa B, const DistLayout* __restrict__ lay,
                                                             const int* __restrict__ wface,
                                                             int* __restrict__ cls, int* __restrict__ bcnt, int nb)
{
    __shared__ int wc[4][kSlabClasses];
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = lay->n;
    int c = -1;
    if (p < n && B.id[p] >= 0 && wface[p >> 6] == 1) {
        double x = B.x[p], y = B.y[p], z = B.z[p];
        move_and_wrap(P, st, B, p, x, y, z);
        const double a = g.axis == 0 ? x : (g.axis == 1 ? y : z);
        c = dev_is_struct(B.type[p]) ? slab_class_static(g, a) : slab_class(g, a);   // as k_dist_classify
        if (c == kSlabLost) c = kInner;   // reported by k_dist_classify at the next step
    }
    if (p < n) cls[p] = c;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kSlabClasses; ++k) {
        const unsigned long long m = __ballot(c == k);
        if (lane == 0) wc[wave][k] = __popcll(m);
    }
    __syncthreads();
    if (threadIdx.x < kSlabClasses) {
        int t = 0;
        for (int w = 0; w < 4; ++w) t += wc[w][threadIdx.x];
        bcnt[threadIdx.x * nb + blockIdx.x] = t;
    }
}

// The messages straight from B, in the order k_dist_scatter + k_dist_pack give them (stable by
// B index within each class): to the left [bandL | migL], to the right [migR | bandR], each behind
// its count header; migrants travel with negated ids, as from C.
__global__ __launch_bounds__(256) void k_dist_early_pack(Soa B, DistLayout* __restrict__ lay,
                                                         const int* __restrict__ cls,
                                                         const int* __restrict__ boff, int nb, int cap_l,
                                                         int cap_r, DevState* __restrict__ st,
                                                         char* __restrict__ buf_l, char* __restrict__ buf_r)
{
    __shared__ int wc[4][kSlabClasses];
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = lay->n;
    const int c = p < n ? cls[p] : -1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int rank = 0;
#pragma unroll
    for (int k = 0; k < kSlabClasses; ++k) {
        const unsigned long long m = __ballot(c == k);
        if (c == k) rank = __popcll(m & lanemask_lt());
        if (lane == 0) wc[wave][k] = __popcll(m);
    }
    __syncthreads();
    const int sMigR = boff[kMigR * nb], sBandR = boff[kBandR * nb], sInner = boff[kInner * nb];
    const int sBandL = boff[kBandL * nb], sMigL = boff[kMigL * nb], sDrop = boff[kSlabDrop * nb];
    const int mr = sInner - sMigR, ml = sDrop - sBandL;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int* hl = (int*)buf_l;
        int* hr = (int*)buf_r;
        hl[0] = sMigL - sBandL; hl[1] = sDrop - sMigL;   // {bandL, migL}
        hr[0] = sBandR - sMigR; hr[1] = sInner - sBandR; // {migR, bandR}
        lay->send[0] = hl[0]; lay->send[1] = hl[1]; lay->send[2] = hr[0]; lay->send[3] = hr[1];
        atomicMax(&lay->hw[0], min(ml, cap_l));
        atomicMax(&lay->hw[1], min(mr, cap_r));
        if (ml > cap_l || mr > cap_r) atomicOr(&st->overflow, 8);
    }
    if (!dist_sends(c)) return;
    int o = boff[c * nb + blockIdx.x] + rank;
    for (int w = 0; w < wave; ++w) o += wc[w][c];
    const bool left = c == kBandL || c == kMigL;
    // the stride is clamped to the capacity like k_dist_pack's (the header keeps the true counts,
    // so a receiver skips an overfull message): an overflow is MPH_ERR_CAPACITY, never a write
    // past the buffer
    const int cap = left ? cap_l : cap_r;
    const int m = min(left ? ml : mr, cap);
    const int j = left ? o - sBandL : o - sMigR;
    if (j >= m) return;
    double* d = (double*)((left ? buf_l : buf_r) + kMsgHeader);
    int* q = (int*)(d + 6 * (size_t)m);
    d[j] = B.x[p]; d[m + j] = B.y[p]; d[2 * m + j] = B.z[p];
    d[3 * m + j] = B.vx[p]; d[4 * m + j] = B.vy[p]; d[5 * m + j] = B.vz[p];
    q[j] = B.type[p];
    const int id = B.id[p];
    q[m + j] = (c == kMigR || c == kMigL) ? -1 - id : id;
}

// also writes the layout's send counts (left-going {bandL, migL}, right-going {migR, bandR}) from
// the class starts (block 0), which the pack kernels and the count exchange of mph_create read
__global__ __launch_bounds__(256) void k_dist_scatter(Soa B, DistLayout* __restrict__ lay,
                                                      const int* __restrict__ cls,
                                                      const int* __restrict__ boff, int nb, Soa C,
                                                      int* __restrict__ dseg, int* __restrict__ vidx)
{
    __shared__ int wc[4][kSlabClasses];
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = lay->n;
    const int c = p < n ? cls[p] : -1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int rank = 0;
#pragma unroll
    for (int k = 0; k < kSlabClasses; ++k) {
        const unsigned long long m = __ballot(c == k);
        if (c == k) rank = __popcll(m & lanemask_lt());
        if (lane == 0) wc[wave][k] = __popcll(m);
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x <= kSlabClasses) dseg[threadIdx.x] = boff[threadIdx.x * nb];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        auto len = [&](int k) { return boff[(k + 1) * nb] - boff[k * nb]; };
        lay->send[0] = len(kBandL);
        lay->send[1] = len(kMigL);
        lay->send[2] = len(kMigR);
        lay->send[3] = len(kBandR);
    }
    if (c < 0 || c == kSlabDrop) return;
    int o = boff[c * nb + blockIdx.x] + rank;
    for (int w = 0; w < wave; ++w) o += wc[w][c];
    if (vidx) {   // VSrc: only where the entry lives
        vidx[o] = (c == kMigR || c == kMigL) ? -1 - p : p;
        return;
    }
    C.x[o] = B.x[p]; C.y[o] = B.y[p]; C.z[o] = B.z[p];
    C.vx[o] = B.vx[p]; C.vy[o] = B.vy[p]; C.vz[o] = B.vz[p];
    C.type[o] = B.type[p];
    const int id = B.id[p];
    C.id[o] = (c == kMigR || c == kMigL) ? -1 - id : id;
}

// Messages of a redistribution travel with a fixed capacity (so the exchange has host-known
// sizes and can sit inside a captured graph); the live counts are the 2-int count messages.
// side 0: [bandL | migL] to the left, side 1: [migR | bandR] to the right.
__device__ __forceinline__ void dist_send_range(const DistLayout* lay, int side, int& off, int& m)
{
    off = side == 0 ? lay->seg[kBandL] : lay->seg[kMigR];
    m = side == 0 ? lay->send[0] + lay->send[1] : lay->send[2] + lay->send[3];
}

// side 0: from the left (their {migR, bandR}) appended at nc, side 1: from the right after it;
// r[4] = the received counts (the message headers)
__device__ __forceinline__ void dist_recv_range(const DistLayout* lay, const int* r, int side, int& off, int& m)
{
    const int nc = lay->seg[kSlabDrop];
    const int fl = r[0] + r[1];
    off = side == 0 ? nc : nc + fl;
    m = side == 0 ? fl : r[2] + r[3];
}

// message layout: a 16-byte header with the two class counts (so no separate count message is
// needed per step), then x[m] y[m] z[m] vx[m] vy[m] vz[m] (double) type[m] id[m] (int), 56 B per
// particle (kMsgHeader above)
// both messages in one launch: blockIdx.y = side
__global__ __launch_bounds__(256) void k_dist_pack(Soa C, DistLayout* __restrict__ lay, int cap_l, int cap_r,
                                                   DevState* __restrict__ st, char* __restrict__ buf_l,
                                                   char* __restrict__ buf_r, VSrc vs)
{
    const int side = blockIdx.y;
    const int cap = side ? cap_r : cap_l;
    char* buf = side ? buf_r : buf_l;
    int off, m;
    dist_send_range(lay, side, off, m);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int* h = (int*)buf;
        h[0] = lay->send[2 * side];
        h[1] = lay->send[2 * side + 1];
    }
    if (m > cap) {   // more than the message capacity: an error (MPH_ERR_CAPACITY), never a fault
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&st->overflow, 8);
        m = cap;
    }
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicMax(&lay->hw[side], m);
    if (k >= m) return;
    double* d = (double*)(buf + kMsgHeader);
    int* q = (int*)(d + 6 * (size_t)m);
    Soa S;
    bool mig;
    const int s = vsrc_entry(vs, C, off + k, S, mig);   // the sent classes are all kept entries
    d[k] = S.x[s]; d[m + k] = S.y[s]; d[2 * m + k] = S.z[s];
    d[3 * m + k] = S.vx[s]; d[4 * m + k] = S.vy[s]; d[5 * m + k] = S.vz[s];
    q[k] = S.type[s];
    q[m + k] = mig ? -1 - S.id[s] : S.id[s];
}

// received message -> C[off, off+m); ownership flips (their migrants are ours, their band
// particles are our ghosts): id -> -1-id for every entry.  The right-hand message completes the
// layout: n = kept + received, n_own = the kept owned classes + the received migrants.
// both messages in one launch: blockIdx.y = side (0 from the left with capacity cap_l, 1 from the right)
__global__ __launch_bounds__(256) void k_dist_unpack(const char* __restrict__ buf_l, const char* __restrict__ buf_r,
                                                     DistLayout* __restrict__ lay, int cap_l, int cap_r, int cap,
                                                     DevState* __restrict__ st, Soa C)
{
    const int side = blockIdx.y;
    const int cap_msg = side ? cap_r : cap_l;
    // the received counts, from the two message headers (from the left: {migR, bandR} of the left
    // neighbour, from the right: {bandL, migL} of the right neighbour)
    const int* hl = (const int*)buf_l;
    const int* hr = (const int*)buf_r;
    const int r[4] = {hl[0], hl[1], hr[0], hr[1]};
    const char* buf = side == 0 ? buf_l : buf_r;
    int off, m;
    dist_recv_range(lay, r, side, off, m);
    const int mm = m;   // the sender's count = the stride of its message
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (mm > cap_msg || off + m > cap) {   // the sender flagged it too; read nothing out of range
        if (first) atomicOr(&st->overflow, 8);
        m = mm > cap_msg ? 0 : max(0, min(m, cap - off));
    }
    if (first) {
        atomicMax(&lay->hw[2 + side], mm);
        if (side == 0) {
            // the layout's receive counts, for the halo ranges of this step
            lay->recv[0] = r[0]; lay->recv[1] = r[1]; lay->recv[2] = r[2]; lay->recv[3] = r[3];
        } else {
            const int* seg = lay->seg;
            const int n = min(off + m, cap);
            lay->n = n;
            lay->n_own = (seg[kBandR + 1] - seg[kBandR]) + (seg[kInner + 1] - seg[kInner]) +
                         (seg[kBandL + 1] - seg[kBandL]) + r[0] + r[3];
            atomicMax(&lay->hw[4], off + (r[2] + r[3]));
        }
    }
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const double* d = (const double*)(buf + kMsgHeader);
    const int* q = (const int*)(d + 6 * (size_t)mm);
    const int s = off + k;
    C.x[s] = d[k]; C.y[s] = d[mm + k]; C.z[s] = d[2 * mm + k];
    C.vx[s] = d[3 * mm + k]; C.vy[s] = d[4 * mm + k]; C.vz[s] = d[5 * mm + k];
    C.type[s] = q[k];
    C.id[s] = -1 - q[mm + k];
}

// Elastic ghost slots (slab mode): w double4 rows per slot, slot k of the message = idx[k].
__global__ __launch_bounds__(256) void k_struct_pack(const double4* __restrict__ src, int w,
                                                     const int* __restrict__ idx, int m,
                                                     double4* __restrict__ buf)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m * w) return;
    const int k = t / w, r = t - k * w;
    buf[t] = src[(size_t)idx[k] * w + r];
}

__global__ __launch_bounds__(256) void k_struct_unpack(const double4* __restrict__ buf, int w,
                                                       const int* __restrict__ idx, int m,
                                                       double4* __restrict__ dst)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m * w) return;
    const int k = t / w, r = t - k * w;
    dst[(size_t)idx[k] * w + r] = buf[t];
}

// C-index ranges of the pass-A halo (mph_dist.hip step 5), from the device layout: dir 0 = to the
// left [the left neighbour's migrants we now own | our band-left], 1 = to the right [the right
// neighbour's migrants we now own | our band-right], 2 = from the left [our migrants that went
// left | the left neighbour's band-right ghosts], 3 = from the right (mirror image).
__device__ __forceinline__ void halo_ranges(const DistLayout* L, int dir, int& o1, int& n1, int& o2, int& n2)
{
    const int* seg = L->seg;
    const int nc = seg[kSlabDrop];
    const int fl = L->recv[0] + L->recv[1];
    if (dir == 0) { o1 = nc; n1 = L->recv[0]; o2 = seg[kBandL]; n2 = seg[kBandL + 1] - seg[kBandL]; }
    else if (dir == 1) { o1 = nc + fl + L->recv[2]; n1 = L->recv[3]; o2 = seg[kBandR]; n2 = seg[kBandR + 1] - seg[kBandR]; }
    else if (dir == 2) { o1 = seg[kMigL]; n1 = seg[kMigL + 1] - seg[kMigL]; o2 = nc + L->recv[0]; n2 = L->recv[1]; }
    else { o1 = seg[kMigR]; n1 = seg[kMigR + 1] - seg[kMigR]; o2 = nc + fl; n2 = L->recv[2]; }
}

// pass-A values of two C-index ranges, read at their sorted position dst_of[c]; cap bounds the
// message (the counts are within it once the redistribution's capacity checks passed)
// both directions in one launch: dir = blockIdx.y (0 to the left into buf_a with capacity cap_a,
// 1 to the right into buf_b)
__global__ __launch_bounds__(256) void k_halo_pack(const int* __restrict__ dst_of, const DistLayout* __restrict__ lay,
                                                   int cap_a, int cap_b, HaloFields F, double* __restrict__ buf_a,
                                                   double* __restrict__ buf_b)
{
    const int dir = blockIdx.y;
    const int cap = dir ? cap_b : cap_a;
    double* buf = dir ? buf_b : buf_a;
    int o1, n1, o2, n2;
    halo_ranges(lay, dir, o1, n1, o2, n2);
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int m = min(n1 + n2, cap);
    if (k >= m) return;
    const int a = dst_of[k < n1 ? o1 + k : o2 + (k - n1)];
    for (int f = 0; f < F.nf; ++f) buf[(size_t)f * m + k] = F.f[f][a];
}

// both directions in one launch: dir = 2 + blockIdx.y (2 from the left out of buf_a, 3 from the right)
__global__ __launch_bounds__(256) void k_halo_unpack(const double* __restrict__ buf_a, const double* __restrict__ buf_b,
                                                     const int* __restrict__ dst_of, const DistLayout* __restrict__ lay,
                                                     int cap_a, int cap_b, HaloFields F)
{
    const int dir = 2 + blockIdx.y;
    const int cap = blockIdx.y ? cap_b : cap_a;
    const double* buf = blockIdx.y ? buf_b : buf_a;
    int o1, n1, o2, n2;
    halo_ranges(lay, dir, o1, n1, o2, n2);
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int m = min(n1 + n2, cap);
    if (k >= m) return;
    const int a = dst_of[k < n1 ? o1 + k : o2 + (k - n1)];
    for (int f = 0; f < F.nf; ++f) F.f[f][a] = buf[(size_t)f * m + k];
    if (F.rec) rec_store_p(F.rec, F.rec_stride, a, buf[k]);
}

// ---------------------------------------------------------------------------- launchers -----

void launch_struct_pack(const Launch& L, const double4* src, int w, const int* idx, int m, double4* buf)
{
    if (m <= 0) return;
    launch(L.prof, "struct_pack", L.stream, k_struct_pack, dim3(blocks(m * w, 256)), dim3(256), src, w, idx, m,
           buf);
}

void launch_struct_unpack(const Launch& L, const double4* buf, int w, const int* idx, int m, double4* dst)
{
    if (m <= 0) return;
    launch(L.prof, "struct_unpack", L.stream, k_struct_unpack, dim3(blocks(m * w, 256)), dim3(256), buf, w, idx,
           m, dst);
}

int dist_blocks(int n) { return blocks(n > 0 ? n : 1, 256); }

void launch_dist_classify(const Launch& L, const SlabGeom& g, int cap, const DistLayout* lay, int move, int* cls,
                          int* bcnt, const int* wface)
{
    const int nb = dist_blocks(cap);
    launch(L.prof, "dist_classify", L.stream, k_dist_classify, dim3(nb), dim3(256), *L.P, L.st, g, L.B, lay, move,
           cls, bcnt, nb, wface);
}

void launch_dist_early_classify(const Launch& L, const SlabGeom& g, int cap, const DistLayout* lay,
                                const int* wface, int* cls, int* bcnt)
{
    const int nb = dist_blocks(cap);
    launch(L.prof, "dist_early_classify", L.stream, k_dist_early_classify, dim3(nb), dim3(256), *L.P, L.st, g, L.B,
           lay, wface, cls, bcnt, nb);
}

void launch_dist_early_pack(const Launch& L, int cap, DistLayout* lay, const int* cls, const int* boff, int cap_l,
                            int cap_r, char* buf_l, char* buf_r)
{
    const int nb = dist_blocks(cap);
    launch(L.prof, "dist_early_pack", L.stream, k_dist_early_pack, dim3(nb), dim3(256), L.B, lay, cls, boff, nb,
           cap_l, cap_r, L.st, buf_l, buf_r);
}

void launch_dist_scatter(const Launch& L, int cap, DistLayout* lay, const int* cls, const int* boff,
                         const Soa& C, int* dseg, int* vidx)
{
    const int nb = dist_blocks(cap);
    launch(L.prof, "dist_scatter", L.stream, k_dist_scatter, dim3(nb), dim3(256), L.B, lay, cls, boff, nb, C, dseg,
           vidx);
}

void launch_dist_pack(const Launch& L, const Soa& C, DistLayout* lay, int cap_l, int cap_r, char* buf_l,
                      char* buf_r, const VSrc& vs)
{
    launch(L.prof, "dist_pack", L.stream, k_dist_pack, dim3(dist_blocks(std::max(cap_l, cap_r)), 2), dim3(256), C, lay,
           cap_l, cap_r, L.st, buf_l, buf_r, vs);
}

void launch_dist_unpack(const Launch& L, const char* buf_l, const char* buf_r, DistLayout* lay, int cap_l,
                        int cap_r, int cap, const Soa& C)
{
    launch(L.prof, "dist_unpack", L.stream, k_dist_unpack, dim3(dist_blocks(std::max(cap_l, cap_r)), 2), dim3(256),
           buf_l, buf_r, lay, cap_l, cap_r, cap, L.st, C);
}

void launch_halo_pack(const Launch& L, const int* dst_of, const DistLayout* lay, int cap_l, int cap_r,
                      const HaloFields& F, double* buf_l, double* buf_r)
{
    launch(L.prof, "halo_pack", L.stream, k_halo_pack, dim3(dist_blocks(std::max(cap_l, cap_r)), 2), dim3(256), dst_of,
           lay, cap_l, cap_r, F, buf_l, buf_r);
}

void launch_halo_unpack(const Launch& L, const double* buf_l, const double* buf_r, const int* dst_of,
                        const DistLayout* lay, int cap_l, int cap_r, const HaloFields& F)
{
    launch(L.prof, "halo_unpack", L.stream, k_halo_unpack, dim3(dist_blocks(std::max(cap_l, cap_r)), 2), dim3(256),
           buf_l, buf_r, dst_of, lay, cap_l, cap_r, F);
}

}  // namespace mph
