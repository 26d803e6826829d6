// mph_dist.hip -- multi-GPU slab decomposition of the hot path (one process per GPU, RCCL).
//
// The reference has no domain decomposition (one OpenMP/OpenACC process, main.cpp:597-686).  The
// update of a particle depends only on neighbours within the cutoff rc = MaxRadius + MARGIN
// (main.cpp:1765), so the periodic domain is cut into `nranks` slabs along one axis (equal widths,
// or the cuts of MphSlabOptions).  Each rank holds
//
//   owned   particles inside its slab [lo, hi)                (computed, returned by mph_get)
//   ghosts  copies of the neighbours' particles within h >= rc of a face, and of its own
//           particles that crossed a face this step (now owned next door)
//
// One step (this file, dist_step), all on the context's stream:
//
//   1. k_dist_classify: wall motion + periodic wrap (calculateWall / calculatePeriodicBoundary
//      exactly as the single-GPU k_prep), then the slab class of every owned particle; ghosts of
//      the previous step are dropped.
//   2. stable partition into C = [migR | bandR | inner | bandL | migL]     (scan + scatter)
//   3. exchange: to the left neighbour [bandL | migL], to the right [migR | bandR] (56 B per
//      particle, behind a header with the two class counts); received messages are appended to C:
//      [.. | from left: their migR (ours now), their bandR (ghosts) | from right: their bandL
//      (ghosts), their migL (ours now)].  Our own migrants stay in C as ghosts.
//   4. cell sort of C (owned + ghosts) into A, neighbour search, pass A -- the single-GPU kernels
//      on the local window grid (DevParams.corg / gc along the slab axis).
//   5. halo exchange of the pass-A values every neighbour's ghosts need in pass B: PressureP
//      (+ GravityCenter, PressureA with surface tension), 8 or 40 B per ghost.
//   6. pass B (forces, kick, drift) into B.
//
// Owned particles see every neighbour (band width h >= rc), run the same FP64 expressions as
// the single-GPU path, and get bit-identical neighbour sets; sums may be ordered differently
// (local cell grid), so values agree with the single-GPU run to reassociation roundoff.
//
// Elastic-solid particles (types 2, 3) are owned by the slab of their InitialPosition for good:
// their fixed Lagrangian lists (calculateInitialNeighbor, main.cpp:1497-1658) then map to a static
// set of ghost slots owned by the two neighbours (dist_struct_setup).  They never migrate; they
// are mirrored as fluid-pass ghosts like any particle near a face, and may sit up to kStructMargin
// beyond their slab's face (the band width grows by that much).  Each elastic substep
// (main.cpp:653-660) becomes
//   7. ghost displacements u -> k_struct_stress on the owned slots -> ghost stresses P ->
//      k_struct_velocity on the owned slots (the last substep writes the owned B entries).
// With slab monitors on (mph_dist_monitor_configure) a step ends with
//   8. the monitor kernels over B and the pass-A pressure: this rank's record of the step
//      (mph_monitor.hip, the slab forms); nothing is exchanged.
// Transport: RCCL ncclSend/ncclRecv (xGMI) or a host callback (tests, mph_create_dist_host), behind
// one interface (mph_dist.h, mph_transport.hip).  The slabs themselves: mph_slab_geom.hip; the
// collective output: mph_dist_output.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "mph_dist.h"
#include "mph_env.h"

using namespace mph;

namespace {

// the redistribution messages of both sides, at their capacities
int redist_exchange(MphCtx* c, hipStream_t stream)
{
    const DistSide* S = c->dist->side;
    return c->dist->tr->exchange(
        c, stream, S[kLeft].wire(kMsgHead + kMsgBytes * S[kLeft].cap_s, kMsgHead + kMsgBytes * S[kLeft].cap_r),
        S[kRight].wire(kMsgHead + kMsgBytes * S[kRight].cap_s, kMsgHead + kMsgBytes * S[kRight].cap_r));
}

int copy_soa(MphCtx* c, const Soa& dst, const Soa& src, int n)
{
    double* dd[6] = {dst.x, dst.y, dst.z, dst.vx, dst.vy, dst.vz};
    const double* sd[6] = {src.x, src.y, src.z, src.vx, src.vy, src.vz};
    for (int k = 0; k < 6; ++k)
        MPH_HIP_OK(c, hipMemcpyAsync(dd[k], sd[k], sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
    MPH_HIP_OK(c, hipMemcpyAsync(dst.type, src.type, sizeof(int) * n, hipMemcpyDeviceToDevice, c->stream));
    MPH_HIP_OK(c, hipMemcpyAsync(dst.id, src.id, sizeof(int) * n, hipMemcpyDeviceToDevice, c->stream));
    return MPH_OK;
}

// Steps between two capacity checks inside one mph_step call: a long call (the steps between two
// VTK outputs) must not outrun its message capacities while the flow changes, so dist_step
// replays at most this many steps before dist_sync reads the high-water marks and grows them.
constexpr int kSyncSteps = 32;

// a cross-stream wait for an event `from` has just recorded (the profiler keeps the point as the
// earliest start of the next launch on `waiting`, see EventProfiler)
hipError_t stream_wait(Profiler* prof, hipStream_t waiting, hipEvent_t ev, hipStream_t from)
{
    if (prof) prof->join(waiting, from);
    return hipStreamWaitEvent(waiting, ev, 0);
}

// the redistributed set's kept entries: where they live in B (VSrc, D.virt) or nowhere (in C)
VSrc dist_vsrc(MphCtx* c)
{
    MphDist& D = *c->dist;
    VSrc vs;
    if (D.virt) {
        vs.idx = D.vidx;
        vs.n = lay_field<int>(D.lay, offsetof(DistLayout, seg)) + kSlabDrop;
        vs.V = c->L.B;
    }
    return vs;
}

// Steps 1-3 of the protocol: classify, partition, exchange migrants + ghosts.  Leaves the new
// local set (owned and ghosts) in D.C and its sizes in D.lay -- on the device: nothing here reads
// a size on the host, so the step can be captured.  init: first redistribution of mph_create,
// which reads the counts once to size the message buffers.
// early_in: the messages left at the end of the previous step (early_send); here only the local
// partition, then the wait for them and the unpack
int redistribute(MphCtx* c, bool move, bool init, Profiler* prof, bool early_in = false)
{
    MphDist& D = *c->dist;
    DistSide &l = D.side[kLeft], &r = D.side[kRight];
    Launch L = c->L;
    L.prof = prof;
    const int nb = dist_blocks(D.cap);
    // see early_send (no profiler floor: the second stream has moved on to the exchange since)
    if (early_in) MPH_HIP_OK(c, hipStreamWaitEvent(c->stream, D.ev_s, 0));
    launch_dist_classify(L, D.g, D.cap, D.lay, move ? 1 : 0, D.cls, D.bcnt, early_in ? D.wface : nullptr);
    launch_scan(D.bcnt, kSlabClasses * nb, D.bsum, D.boff, 0, nullptr, c->stream, prof);
    launch_dist_scatter(L, D.cap, D.lay, D.cls, D.boff, D.C, lay_field<int>(D.lay, offsetof(DistLayout, seg)),
                        D.virt ? D.vidx : nullptr);
    if (early_in) {
        MPH_HIP_OK(c, stream_wait(prof, c->stream, D.ev_x, D.stream2));
        launch_dist_unpack(L, l.recv, r.recv, D.lay, l.cap_r, r.cap_r, D.cap, D.C);
        return MPH_OK;
    }
    if (init) {
        // the first redistribution exchanges the counts alone, to size the message buffers; later
        // ones find them in the message headers (one exchange per redistribution)
        int* snd = lay_field<int>(D.lay, offsetof(DistLayout, send));
        int* rcv = lay_field<int>(D.lay, offsetof(DistLayout, recv));
        MPH_CK(D.tr->exchange(c, c->stream, Wire{l.peer, snd, 2 * sizeof(int), rcv, 2 * sizeof(int)},
                              Wire{r.peer, snd + 2, 2 * sizeof(int), rcv + 2, 2 * sizeof(int)}));
        MPH_HIP_OK(c, hipMemcpyAsync(D.hlay, D.lay, sizeof(DistLayout), hipMemcpyDeviceToHost, c->stream));
        MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
        const DistLayout& h = *D.hlay;
        for (int s = 0; s < 2; ++s) {
            D.side[s].cap_s = msg_capacity0(D, h.send[2 * s] + h.send[2 * s + 1]);
            D.side[s].cap_r = msg_capacity0(D, h.recv[2 * s] + h.recv[2 * s + 1]);
        }
        MPH_CK(msg_alloc(c));
    }
    const VSrc vs = dist_vsrc(c);
    launch_dist_pack(L, D.C, D.lay, l.cap_s, r.cap_s, l.send, r.send, vs);
    MPH_CK(redist_exchange(c, c->stream));
    launch_dist_unpack(L, l.recv, r.recv, D.lay, l.cap_r, r.cap_r, D.cap, D.C);
    return MPH_OK;
}

// The next step's redistribution messages, sent from the face wavefronts of this step's pass B
// on the second stream (joined by the next step's redistribute(early_in)); the same bytes as
// k_dist_pack would send from C.
int early_send(MphCtx* c, Profiler* prof, hipStream_t stream)
{
    MphDist& D = *c->dist;
    Launch L = c->L;
    L.prof = prof;
    L.stream = stream;
    const int nb = dist_blocks(D.cap);
    launch_dist_early_classify(L, D.g, D.cap, D.lay, D.wface, D.cls, D.bcnt);
    launch_scan(D.bcnt, kSlabClasses * nb, D.bsum, D.boff, 0, nullptr, stream, prof);
    launch_dist_early_pack(L, D.cap, D.lay, D.cls, D.boff, D.side[kLeft].cap_s, D.side[kRight].cap_s,
                           D.side[kLeft].send, D.side[kRight].send);
    // ev_s: the face waves' pass B and these kernels are done (the next step's partition, on the
    // main stream, waits for it before it reads B and wface); ev_x: the messages have landed
    MPH_HIP_OK(c, hipEventRecord(D.ev_s, stream));
    if (stream != D.stream2) MPH_HIP_OK(c, stream_wait(prof, D.stream2, D.ev_s, stream));
    MPH_CK(redist_exchange(c, D.stream2));
    MPH_HIP_OK(c, hipEventRecord(D.ev_x, D.stream2));
    return MPH_OK;
}

// cell sort of C into A (slab-local grid), recording dst_of = pre-sort -> sorted index
void sort_local(MphCtx* c, int mode, Profiler* prof)
{
    Launch L = c->L;
    L.prof = prof;
    L.B = c->dist->C;
    L.vsrc = dist_vsrc(c);
    L.dst_of = c->order;
    launch_sort(L, mode);
}

HaloFields halo_fields(MphCtx* c)
{
    HaloFields F{};
    F.f[0] = c->L.pres;
    F.nf = 1;
    F.rec = c->L.rec;
    F.rec_stride = c->P.n;   // the plane stride of the pass-B records (capacity)
    if (c->P.surface) {
        F.f[1] = c->L.gx; F.f[2] = c->L.gy; F.f[3] = c->L.gz; F.f[4] = c->L.pa;
        F.nf = 5;
    }
    return F;
}

// One static ghost exchange of per-slot double4 records (w rows per slot) of the elastic arrays.
int struct_exchange(MphCtx* c, double4* a, int w, Profiler* prof, hipStream_t stream)
{
    MphDist& D = *c->dist;
    const DistSide &l = D.side[kLeft], &r = D.side[kRight];
    Launch L = c->L;
    L.prof = prof;
    L.stream = stream;
    for (const DistSide& S : D.side) launch_struct_pack(L, a, w, S.ss, S.nss, (double4*)S.send);
    const size_t b = sizeof(double4) * w;
    MPH_CK(D.tr->exchange(c, stream, l.wire(b * l.nss, b * l.nsr), r.wire(b * r.nss, b * r.nsr)));
    for (const DistSide& S : D.side) launch_struct_unpack(L, (const double4*)S.recv, w, S.sr, S.nsr, a);
    return MPH_OK;
}

// Step 7: the elastic substeps on the owned slots, ghosts refreshed before each half.  Each ghost
// exchange (displacements u before DeformationVector/Stress, first Piola-Kirchhoff rows P before
// StressForce) travels on the second stream while the owned slots whose lists hold no ghost slot
// ([0, n_inner), dist_struct_setup) run their half on the main stream; the others follow once it
// has landed.  The slots a neighbour needs are all among the latter (symmetric lists), so a pack
// never waits for an inner half.
int struct_substeps(MphCtx* c, Profiler* prof)
{
    if (c->P.n_struct == 0) return MPH_OK;
    MphDist& D = *c->dist;
    Launch L = c->L;
    L.prof = prof;
    StructDev& S = c->Sd;
    const int wP = c->P.dim == 2 ? 1 : 3;
    // launch(s0, s1): the half-substep over owned slots [s0, s1)
    auto half = [&](double4* a, int w, auto&& launch) -> int {
        if (!D.overlap) {
            MPH_CK(struct_exchange(c, a, w, prof, c->stream));
            launch(0, S.n_own);
            return MPH_OK;
        }
        MPH_HIP_OK(c, hipEventRecord(D.ev_a, c->stream));
        MPH_HIP_OK(c, stream_wait(prof, D.stream2, D.ev_a, c->stream));
        launch(0, S.n_inner);   // enqueued before a host-staged exchange blocks the host
        MPH_CK(struct_exchange(c, a, w, prof, D.stream2));
        MPH_HIP_OK(c, hipEventRecord(D.ev_h, D.stream2));
        MPH_HIP_OK(c, stream_wait(prof, c->stream, D.ev_h, D.stream2));
        launch(S.n_inner, S.n_own);
        return MPH_OK;
    };
    for (int sub = 0; sub < c->P.substeps; ++sub) {
        const bool last = sub == c->P.substeps - 1;
        MPH_CK(half(S.u, 1, [&](int s0, int s1) { launch_struct_stress(L, last, s0, s1); }));
        MPH_CK(half(S.P, wP, [&](int s0, int s1) { launch_struct_velocity(L, last, s0, s1); }));
    }
    return MPH_OK;
}

// MPH_SLAB_OVERLAP unset ("auto"): the ranks choose the pass-B mode together at creation, from
// what this machine and transport do.  On the initial state (after the init sums) every rank times,
// with events on its stream, best of three after a warm-up:
//   th  the halo exchange of the pass-A values,
//   tr  an exchange of the redistribution messages,
//   ts  pass B as the overlap splits it (interior, then face waves) minus pass B in one launch;
// the maxima over ranks decide: overlap when th + tr > ts, i.e. when the exchanges it can hide
// behind the interior pass B (and, with the early send, behind the next partition) cost more than
// splitting pass B does.  The exchanges are timed at their message capacities, which is what the
// steps send: the messages of a step have fixed, capacity-sized lengths (the live counts travel in
// their headers), so that RCCL steps can be replayed from captured graphs.
// The probe touches no live state: its halo packs from and unpacks into the redistribution
// scratch set C (which every step rewrites before reading, dist_enqueue_step), its redistribution
// exchange moves the message buffers only, and its trial pass B integrates into C with the output
// stores (Force, Acceleration) off.  Every rank takes part or none: a rank holding elastic
// particles (whose pass B also hands them to the substep slots) keeps the overlap off on all ranks,
// agreed through a collective max, since the structure need not reach every slab.
int overlap_probe(MphCtx* c)
{
    MphDist& D = *c->dist;
    D.overlap = D.overlap_mode == 1;
    if (D.overlap_mode >= 0) return MPH_OK;
    double any_struct = c->P.n_struct > 0 ? 1.0 : 0.0;
    MPH_CK(D.tr->max(c, c->stream, &any_struct, 1));
    if (any_struct > 0.0) return MPH_OK;
    Launch L = c->L;
    L.wface = D.wface;
    L.B = D.C;                   // the trial pass B's integrated state: scratch
    L.force = L.acc = nullptr;   // no output stores
    HaloFields F = halo_fields(c);
    double* scratch[5] = {D.C.x, D.C.y, D.C.z, D.C.vx, D.C.vy};
    for (int k = 0; k < F.nf; ++k) F.f[k] = scratch[k];
    F.rec = nullptr;
    hipEvent_t e[5] = {};
    struct Ev {
        hipEvent_t* e;
        ~Ev() { for (int k = 0; k < 5; ++k) if (e[k]) (void)hipEventDestroy(e[k]); }
    } guard{e};
    for (auto& x : e) MPH_HIP_OK(c, hipEventCreate(&x));
    double best[3] = {1e30, 1e30, 1e30};
    for (int rep = 0; rep < 4; ++rep) {
        MPH_HIP_OK(c, hipEventRecord(e[0], c->stream));
        MPH_CK(halo_exchange(c, nullptr, c->stream, &F));
        MPH_HIP_OK(c, hipEventRecord(e[1], c->stream));
        MPH_CK(redist_exchange(c, c->stream));
        MPH_HIP_OK(c, hipEventRecord(e[2], c->stream));
        launch_pass_b(L, 0);
        MPH_HIP_OK(c, hipEventRecord(e[3], c->stream));
        launch_pass_b(L, 1);
        launch_pass_b(L, 2);
        MPH_HIP_OK(c, hipEventRecord(e[4], c->stream));
        MPH_HIP_OK(c, hipGetLastError());
        MPH_HIP_OK(c, hipEventSynchronize(e[4]));
        float ms[4];
        for (int k = 0; k < 4; ++k) MPH_HIP_OK(c, hipEventElapsedTime(&ms[k], e[k], e[k + 1]));
        if (rep == 0) continue;   // warm-up: the first exchanges set up the transport
        best[0] = std::min(best[0], (double)ms[0]);
        best[1] = std::min(best[1], (double)ms[1]);
        best[2] = std::min(best[2], (double)ms[3] - (double)ms[2]);
    }
    MPH_CK(D.tr->max(c, c->stream, best, 3));
    for (int k = 0; k < 3; ++k) D.probe_ms[k] = best[k];
    D.overlap = best[0] + best[1] > best[2];
    return MPH_OK;
}

}  // namespace

namespace mph {

// Step 5: the pass-A values of every neighbour's ghosts (ranges from the device layout, fixed
// message capacities: to/from a side the particles of its send and its receive capacity).
int halo_exchange(MphCtx* c, Profiler* prof, hipStream_t stream, const HaloFields* fields)
{
    MphDist& D = *c->dist;
    const DistSide &l = D.side[kLeft], &r = D.side[kRight];
    Launch L = c->L;
    L.prof = prof;
    L.stream = stream;
    const HaloFields F = fields ? *fields : halo_fields(c);
    const int capl = l.cap_s + l.cap_r, capr = r.cap_s + r.cap_r;
    launch_halo_pack(L, c->order, D.lay, capl, capr, F, (double*)l.send, (double*)r.send);
    const size_t b = sizeof(double) * F.nf;
    MPH_CK(D.tr->exchange(c, stream, l.wire(b * capl, b * capl), r.wire(b * capr, b * capr)));
    launch_halo_unpack(L, (const double*)l.recv, (const double*)r.recv, c->order, D.lay, capl, capr, F);
    return MPH_OK;
}

int dist_alloc(MphCtx* c)
{
    MphDist& D = *c->dist;
    const int cap = D.cap;
    Soa& C = D.C;
    MPH_CK(ctx_dalloc(c, &C.x, cap)); MPH_CK(ctx_dalloc(c, &C.y, cap)); MPH_CK(ctx_dalloc(c, &C.z, cap));
    MPH_CK(ctx_dalloc(c, &C.vx, cap)); MPH_CK(ctx_dalloc(c, &C.vy, cap)); MPH_CK(ctx_dalloc(c, &C.vz, cap));
    MPH_CK(ctx_dalloc(c, &C.type, cap)); MPH_CK(ctx_dalloc(c, &C.id, cap));
    MPH_CK(ctx_dalloc(c, &D.cls, cap));
    MPH_CK(ctx_dalloc(c, &D.vidx, cap));
    MPH_CK(ctx_dalloc(c, &D.wface, (size_t)cap / 64 + 2));
    MPH_HIP_OK(c, hipMemsetAsync(D.wface, 0, sizeof(int) * ((size_t)cap / 64 + 2), c->stream));
    const size_t nslots = (size_t)kSlabClasses * dist_blocks(cap);
    MPH_CK(ctx_dalloc(c, &D.bcnt, nslots + 1));
    MPH_CK(ctx_dalloc(c, &D.boff, nslots + 1));
    MPH_CK(ctx_dalloc(c, &D.bsum, nslots / 4096 + 2));
    MPH_CK(ctx_dalloc(c, &D.lay, 1));
    MPH_HIP_OK(c, hipHostMalloc((void**)&D.hlay, sizeof(DistLayout), hipHostMallocDefault));
    std::memset(D.hlay, 0, sizeof(DistLayout));
    D.hlay->n = c->n;   // the uploaded owned set, classified by the first redistribution
    MPH_HIP_OK(c, hipMemcpyAsync(D.lay, D.hlay, sizeof(DistLayout), hipMemcpyHostToDevice, c->stream));
    // every kernel of a slab step reads the live particle count from the layout; P.n is the
    // capacity the launch grids are sized for
    c->P.n = cap;
    c->P.n_dev = lay_field<int>(D.lay, offsetof(DistLayout, n));
    // first message buffers (the count exchange of the first redistribution uses them); their
    // capacities follow from the first counts (redistribute, init)
    for (DistSide& S : D.side) S.cap_s = S.cap_r = msg_capacity(D, 0);
    MPH_CK(msg_alloc(c));
    MPH_HIP_OK(c, hipStreamCreateWithFlags(&D.stream2, hipStreamNonBlocking));
    MPH_HIP_OK(c, hipEventCreateWithFlags(&D.ev_a, hipEventDisableTiming));
    MPH_HIP_OK(c, hipEventCreateWithFlags(&D.ev_h, hipEventDisableTiming));
    MPH_HIP_OK(c, hipEventCreateWithFlags(&D.ev_s, hipEventDisableTiming));
    MPH_HIP_OK(c, hipEventCreateWithFlags(&D.ev_x, hipEventDisableTiming));
    return D.tr->start(c);
}

int dist_sync(MphCtx* c, bool grow_ok)
{
    MphDist& D = *c->dist;
    DevState hs;
    MPH_HIP_OK(c, hipMemcpyAsync(&hs, c->L.st, kStateHead, hipMemcpyDeviceToHost, c->stream));
    MPH_HIP_OK(c, hipMemcpyAsync(D.hlay, D.lay, sizeof(DistLayout), hipMemcpyDeviceToHost, c->stream));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    if (hs.overflow & 8)
        return ctx_fail(c, MPH_ERR_CAPACITY, "slab mode: a redistribution exceeded the message or local capacity");
    MPH_CK(ctx_state_status(c, hs));
    const DistLayout& h = *D.hlay;
    c->n = h.n;
    D.n_own = h.n_own;
    if (h.hw[4] > D.cap)
        return ctx_fail(c, MPH_ERR_CAPACITY, "slab mode: local particle capacity " + std::to_string(D.cap) +
                                                 " exceeded (" + std::to_string(h.hw[4]) + ")");
    // capacity check between batches: a direction above 90 % of its message capacity grows (both
    // ranks of the pair see the same counts, so they grow the shared direction alike); the
    // captured graphs hold the old sizes and are re-captured by the next step.  Capacities are
    // 1.25 c + 4096: every message travels at its capacity (fixed sizes in the graphs)
    bool grow = false;
    auto check = [&](int hw, int& cap) {
        if ((long long)hw * 10 > (long long)cap * 9) {
            cap = msg_capacity(D, hw);
            grow = true;
        }
    };
    for (int s = 0; s < 2 && grow_ok; ++s) {   // hw: sent left, sent right, received left, received right
        check(h.hw[s], D.side[s].cap_s);
        check(h.hw[2 + s], D.side[s].cap_r);
    }
    if (grow) {
        MPH_CK(msg_alloc(c));
        MPH_CK(drop_graphs(c));
        MPH_HIP_OK(c, hipMemsetAsync(lay_field<int>(D.lay, offsetof(DistLayout, hw)), 0, 4 * sizeof(int),
                                     c->stream));
    }
    return MPH_OK;
}

int dist_init(MphCtx* c)
{
    // calculateNeighbor, DensityA, GravityCenter, DensityP of the initialisation (main.cpp:565-568)
    // on owned + ghosts (no motion, no time advance)
    MPH_CK(redistribute(c, false, true, nullptr));
    sort_local(c, 0, nullptr);
    launch_search_pass_a(c->L);
    // no capacity growth yet: the first sizing came from these very counts (and a test sizing,
    // MPH_SLAB_MSG_CAP0_FRAC, is meant to grow at the first check after real steps)
    MPH_CK(dist_sync(c, false));
    // the integrated-state set B starts as the sorted local set (owned + ghosts, ids signed)
    MPH_CK(copy_soa(c, c->L.B, c->L.A, c->n));
    MPH_HIP_OK(c, hipGetLastError());
    MPH_CK(dist_sync(c, false));
    MPH_CK(overlap_probe(c));   // MPH_SLAB_OVERLAP auto: the pass-B mode, the same on every rank
    return dist_sync(c, false);
}

// One slab step on the context's stream (no host synchronisation inside: RCCL transport steps
// are captured into graphs by dist_step; the host transport stages each message through host
// memory and so synchronises in its exchange, mph_transport.hip).
// early_in / early_out: inside a batch of steps, this step's redistribution messages were sent by
// the previous step / the next step's are sent here (early_send), beside the interior pass B.
int dist_enqueue_step(MphCtx* c, Profiler* prof, bool early_in, bool early_out)
{
    Launch L = c->L;
    L.prof = prof;
    MphDist& D = *c->dist;
    L.wface = D.wface;
    MPH_CK(redistribute(c, true, false, prof, early_in));
    sort_local(c, 2, prof);
    launch_search_pass_a(L);
    // slab monitors: the rank's record of the state this step leaves (what mph_get returns after it),
    // so behind the substeps and before an early send, whose classify moves the face waves'
    // particles of B for the next step; on the main stream, both pass-B streams joined
    const auto monitors = [&] {
        if (c->dmon_on) launch_dist_monitor(L, c->mon);
    };
    if (!D.overlap) {   // MPH_SLAB_OVERLAP=0: halo first, then one pass B over every particle
        MPH_CK(halo_exchange(c, prof, c->stream));
        launch_pass_b(L, 0);
        if (early_out) MPH_CK(early_send(c, prof, c->stream));   // (never: early_at needs the overlap)
        MPH_CK(struct_substeps(c, prof));
        monitors();
        return MPH_OK;
    }
    // pass B of the wavefronts without ghost neighbours runs on the main stream while, on the
    // second stream, the pass-A halo travels and the wavefronts near a face follow as soon as it
    // has landed: the two pass-B kernels run concurrently, so neither launch's tail idles the GPU
    // (the interior one is enqueued first, so that a host-staged exchange, which blocks the host,
    // also overlaps with it).  With the early send the face waves' particles then leave for the
    // next step's redistribution, still on the second stream.
    Launch L2 = L;
    L2.stream = D.stream2;
    MPH_HIP_OK(c, hipEventRecord(D.ev_a, c->stream));
    MPH_HIP_OK(c, stream_wait(prof, D.stream2, D.ev_a, c->stream));
    launch_pass_b(L, 1);
    MPH_CK(halo_exchange(c, prof, D.stream2));
    launch_pass_b(L2, 2);
    // joined by the next step's redistribute (ev_s, ev_x)
    if (early_out && c->P.n_struct == 0 && !c->dmon_on) return early_send(c, prof, D.stream2);
    MPH_HIP_OK(c, hipEventRecord(D.ev_h, D.stream2));
    MPH_HIP_OK(c, stream_wait(prof, c->stream, D.ev_h, D.stream2));
    MPH_CK(struct_substeps(c, prof));
    monitors();
    // elastic particles take their positions from the substeps, and the monitors read B as the step
    // leaves it: the face waves are classified and packed after them (main stream); the messages
    // still travel on the second stream beside the next step's partition
    if (early_out) return early_send(c, prof, c->stream);
    return MPH_OK;
}

// the early send chains the steps of one batch (one graph or one mph_step call): step k receives
// early if k > 0 and sends early if k < steps - 1, so every batch ends joined
bool early_at(const MphCtx* c, int k, int steps, int out)
{
    const MphDist& D = *c->dist;
    if (!D.early || !D.overlap) return false;
    return out ? k < steps - 1 : k > 0;
}

int dist_capture(MphCtx* c, int steps, hipGraphExec_t* out)
{
    return ctx_capture(c, out, [&] {
        int rc = MPH_OK;
        for (int k = 0; k < steps && rc == MPH_OK; ++k)
            rc = dist_enqueue_step(c, nullptr, early_at(c, k, steps, 0), early_at(c, k, steps, 1));
        return rc;
    });
}

int dist_step_batch(MphCtx* c, int nsteps, Profiler* prof);

int dist_step(MphCtx* c, int nsteps, Profiler* prof)
{
    // sub-batches of kSyncSteps (a multiple of the 8-step graph), each ending in dist_sync
    for (int done = 0; done < nsteps;) {
        const int k = std::min(kSyncSteps, nsteps - done);
        MPH_CK(dist_step_batch(c, k, prof));
        done += k;
    }
    return MPH_OK;
}

int dist_step_batch(MphCtx* c, int nsteps, Profiler* prof)
{
    MphDist& D = *c->dist;
    // the 8-step graph at the first call whatever its count (every rank makes the same calls),
    // so a short warm-up does not leave its capture to the first long run.  A capture the runtime
    // refuses (an RCCL build without graph support) falls back to the same steps as direct
    // launches, reported by mph_dist_info
    if (D.graphs && !prof &&
        ((!c->graph[kSeq1] && dist_capture(c, 1, &c->graph[kSeq1]) != MPH_OK) ||
         (!c->graph[kSeq8] && dist_capture(c, 8, &c->graph[kSeq8]) != MPH_OK))) {
        (void)hipGetLastError();
        D.graphs = false;
        c->err.clear();
    }
    if (D.graphs && !prof) {
        MPH_CK(ctx_replay(c, nsteps));
    } else {
        for (int k = 0; k < nsteps; ++k)
            MPH_CK(dist_enqueue_step(c, prof, early_at(c, k, nsteps, 0), early_at(c, k, nsteps, 1)));
    }
    MPH_HIP_OK(c, hipGetLastError());
    // (a batch ends joined, early_at: the sorted set A, its ghosts' PressureP included, is the last
    // step's -- what the slab ranks' lattice calls read, mph_dist_sample_grid)
    ctx_stepped(c, nsteps, true);
    return dist_sync(c);
}

void dist_free(MphCtx* c)
{
    MphDist* D = c->dist;
    if (!D) return;
    if (D->stream2) (void)hipStreamSynchronize(D->stream2);
    D->tr.reset();   // the communicator, or the host staging; the message buffers go with the context's arrays
    for (hipEvent_t e : {D->ev_a, D->ev_h, D->ev_s, D->ev_x})
        if (e) (void)hipEventDestroy(e);
    if (D->stream2) (void)hipStreamDestroy(D->stream2);
    if (D->hlay) (void)hipHostFree(D->hlay);
    delete D;
    c->dist = nullptr;
}

}  // namespace mph

// the rank's state before ctx_create: who it is, its transport (rccl: the unique id, else the host
// callback -- the one place that chooses) and the environment's slab knobs
static MphDist* make_dist(int rank, int nranks, int axis, const double* cuts, const char* unique_id128,
                          mph_host_exchange_fn fn, void* user)
{
    MphDist* D = new MphDist();
    D->rank = rank;
    D->nranks = nranks;
    D->g.axis = axis;
    if (cuts) D->cuts.assign(cuts, cuts + std::max(nranks - 1, 0));
    D->tr.reset(unique_id128 ? make_rccl_transport(rank, nranks, unique_id128)
                             : make_host_transport(rank, nranks, fn, user));
    D->graphs = D->tr->graphs_ok() && !env_is("MPH_SLAB_GRAPHS", "0");
    D->virt = !env_is("MPH_SLAB_VIRTUAL_C", "0");
    D->early = !env_is("MPH_SLAB_EARLY", "0");
    D->overlap_mode = env_is("MPH_SLAB_OVERLAP", "1") ? 1 : (env_is("MPH_SLAB_OVERLAP", "0") ? 0 : -1);
    D->msg_slack = std::max(0, env_int("MPH_SLAB_MSG_SLACK", 4096));
    D->msg_fixed = std::max(0, env_int("MPH_SLAB_MSG_CAP", 0));
    D->msg_cap0_frac = env_double("MPH_SLAB_MSG_CAP0_FRAC", 0.0);
    return D;
}

extern "C" {

int mph_create_dist(MphCtx** ctx, const MphConfig* cfg, int n, const int* property, const double* pos,
                    const double* pos0, const double* vel, int device, int rank, int nranks,
                    const char* unique_id128, int axis)
{
    if (!unique_id128 || rank < 0 || rank >= nranks) return MPH_ERR_ARG;
    return ctx_create(ctx, cfg, n, property, pos, pos0, vel, device,
                      make_dist(rank, nranks, axis, nullptr, unique_id128, nullptr, nullptr));
}

int mph_create_slab(MphCtx** ctx, const MphConfig* cfg, int n, const int* property, const double* pos,
                    const double* pos0, const double* vel, int device, const MphSlabOptions* opt)
{
    if (!opt || opt->rank < 0 || opt->rank >= opt->nranks) return MPH_ERR_ARG;
    if ((opt->unique_id128 == nullptr) == (opt->host_fn == nullptr)) return MPH_ERR_ARG;
    if (opt->n_glob > 0 && !opt->ids) return MPH_ERR_ARG;
    MphDist* D = make_dist(opt->rank, opt->nranks, opt->axis, opt->cuts, opt->unique_id128, opt->host_fn,
                           opt->host_user);
    return ctx_create(ctx, cfg, n, property, pos, pos0, vel, device, D, opt->n_glob > 0 ? opt->ids : nullptr,
                      opt->n_glob);
}

int mph_create_dist_host(MphCtx** ctx, const MphConfig* cfg, int n, const int* property, const double* pos,
                         const double* pos0, const double* vel, int device, int rank, int nranks, int axis,
                         mph_host_exchange_fn fn, void* user)
{
    if (!fn || rank < 0 || rank >= nranks) return MPH_ERR_ARG;
    return ctx_create(ctx, cfg, n, property, pos, pos0, vel, device,
                      make_dist(rank, nranks, axis, nullptr, nullptr, fn, user));
}

int mph_dist_overlap(const MphCtx* c, double* out5)
{
    if (!c || !out5) return MPH_ERR_ARG;
    for (int k = 0; k < 5; ++k) out5[k] = -1.0;
    if (!c->dist) return MPH_OK;
    const MphDist& D = *c->dist;
    out5[0] = D.overlap ? 1.0 : 0.0;
    out5[1] = D.overlap_mode;
    for (int k = 0; k < 3; ++k) out5[2 + k] = D.probe_ms[k];
    return MPH_OK;
}

int mph_dist_info(const MphCtx* c, int* out8)
{
    if (!c || !out8) return MPH_ERR_ARG;
    std::memset(out8, 0, 8 * sizeof(int));
    if (!c->dist) {
        out8[0] = 1;
        return MPH_OK;
    }
    const MphDist& D = *c->dist;
    out8[0] = D.nranks;
    out8[1] = D.rank;
    // the RCCL communicator's own size (0 under the host-staged transport, which has none)
    out8[2] = D.tr->comm_count();
    out8[3] = D.graphs ? 1 : 0;
    out8[4] = D.cap;
    out8[5] = std::max(D.side[kLeft].cap_s, D.side[kRight].cap_s);
    out8[6] = std::max(D.side[kLeft].cap_r, D.side[kRight].cap_r);
    out8[7] = c->n;
    return MPH_OK;
}

int mph_owned_count(const MphCtx* c)
{
    if (!c) return -1;
    return c->dist ? c->dist->n_own : c->n_glob;
}

int mph_owned_ids(MphCtx* c, int* out)
{
    if (!c || !out) return MPH_ERR_ARG;
    if (!c->dist) {
        for (int i = 0; i < c->n_glob; ++i) out[i] = i;
        return MPH_OK;
    }
    MPH_HIP_OK(c, hipSetDevice(c->device));
    std::vector<int> id(c->n);
    MPH_HIP_OK(c, hipMemcpyAsync(id.data(), c->L.B.id, sizeof(int) * c->n, hipMemcpyDeviceToHost, c->stream));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    int k = 0;
    for (int i = 0; i < c->n; ++i)
        if (id[i] >= 0) {
            if (k >= c->dist->n_own) return ctx_fail(c, MPH_ERR_CAPACITY, "owned id count mismatch");
            out[k++] = id[i];
        }
    std::sort(out, out + k);
    return k == c->dist->n_own ? MPH_OK : ctx_fail(c, MPH_ERR_CAPACITY, "owned id count mismatch");
}

}  // extern "C"
