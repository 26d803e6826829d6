// mph_transport.hip -- who moves the bytes of the slab decomposition (host only, no kernels): the two
// implementations of Transport (mph_dist.h) -- RCCL ncclSend/ncclRecv, or a host callback with
// pinned staging -- the message buffers they carry, and the RCCL self-test.  The choice is made
// once, at creation (make_dist); nothing outside this unit asks which one is in use.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "mph_dist.h"

using namespace mph;

namespace {

#define RCCL_OK(ctx, expr)                                                                     \
    do {                                                                                       \
        ncclResult_t _r = (expr);                                                              \
        if (_r != ncclSuccess)                                                                 \
            return ctx_fail(ctx, MPH_ERR_RCCL, std::string(#expr) + ": " + ncclGetErrorString(_r)); \
    } while (0)

struct RcclTransport final : Transport {
    int rank, nranks;
    ncclUniqueId id;
    ncclComm_t comm = nullptr;

    RcclTransport(int rank_, int nranks_, const char* unique_id128) : rank(rank_), nranks(nranks_)
    {
        static_assert(sizeof(id) == 128, "ncclUniqueId size");
        std::memcpy(&id, unique_id128, sizeof(id));
    }
    ~RcclTransport() override
    {
        if (comm) (void)ncclCommDestroy(comm);
    }
    bool graphs_ok() const override { return true; }
    int comm_count() const override
    {
        int count = 0;
        if (comm && ncclCommCount(comm, &count) != ncclSuccess) count = -1;
        return count;
    }
    int start(MphCtx* c) override
    {
        RCCL_OK(c, ncclCommInitRank(&comm, nranks, id, rank));
        return MPH_OK;
    }

    int exchange(MphCtx* c, hipStream_t stream, const Wire& l, const Wire& r) override
    {
        RCCL_OK(c, ncclGroupStart());
        // per-peer order: first the left-going message, then the right-going one (matters when
        // left == right, nranks == 2): a rank's first receive from a peer matches that peer's
        // first send, i.e. its left-going message = our from-right message
        if (l.nsend) RCCL_OK(c, ncclSend(l.send, l.nsend, ncclChar, l.peer, comm, stream));
        if (r.nrecv) RCCL_OK(c, ncclRecv(r.recv, r.nrecv, ncclChar, r.peer, comm, stream));
        if (r.nsend) RCCL_OK(c, ncclSend(r.send, r.nsend, ncclChar, r.peer, comm, stream));
        if (l.nrecv) RCCL_OK(c, ncclRecv(l.recv, l.nrecv, ncclChar, l.peer, comm, stream));
        RCCL_OK(c, ncclGroupEnd());
        return MPH_OK;
    }

    // all-reduce
    int max(MphCtx* c, hipStream_t stream, double* v, int n) override
    {
        double* d = nullptr;
        MPH_HIP_OK(c, hipMalloc((void**)&d, sizeof(double) * n));
        std::unique_ptr<double, void (*)(double*)> guard(d, [](double* q) { (void)hipFree(q); });
        MPH_HIP_OK(c, hipMemcpyAsync(d, v, sizeof(double) * n, hipMemcpyHostToDevice, stream));
        RCCL_OK(c, ncclAllReduce(d, d, n, ncclDouble, ncclMax, comm, stream));
        MPH_HIP_OK(c, hipMemcpyAsync(v, d, sizeof(double) * n, hipMemcpyDeviceToHost, stream));
        MPH_HIP_OK(c, hipStreamSynchronize(stream));
        return MPH_OK;
    }

    // the sizes by all-gather, then one receive from every rank
    int gather_root(MphCtx* c, hipStream_t stream, const std::vector<char>& mine, std::vector<char>& all) override
    {
        const int R = nranks;
        all.clear();
        if (R == 1) {
            all = mine;
            return MPH_OK;
        }
        struct DevBuf {
            void* p = nullptr;
            ~DevBuf() { if (p) (void)hipFree(p); }
        } dsz, dsend, drecv;
        MPH_HIP_OK(c, hipMalloc(&dsz.p, sizeof(long long) * R));
        long long* sz = (long long*)dsz.p;
        const long long my = (long long)mine.size();
        MPH_HIP_OK(c, hipMemcpyAsync(sz + rank, &my, sizeof(my), hipMemcpyHostToDevice, stream));
        RCCL_OK(c, ncclAllGather(sz + rank, sz, 1, ncclInt64, comm, stream));
        std::vector<long long> h(R);
        MPH_HIP_OK(c, hipMemcpyAsync(h.data(), sz, sizeof(long long) * R, hipMemcpyDeviceToHost, stream));
        MPH_HIP_OK(c, hipStreamSynchronize(stream));
        long long total = 0;
        std::vector<long long> off(R);
        for (int r = 0; r < R; ++r) { off[r] = total; total += h[r]; }
        if (rank != 0 && my > 0) {
            MPH_HIP_OK(c, hipMalloc(&dsend.p, (size_t)my));
            MPH_HIP_OK(c, hipMemcpy(dsend.p, mine.data(), (size_t)my, hipMemcpyHostToDevice));
        }
        if (rank == 0 && total > my) MPH_HIP_OK(c, hipMalloc(&drecv.p, (size_t)(total - my)));
        RCCL_OK(c, ncclGroupStart());
        for (int r = 1; r < R; ++r) {
            if (!h[r]) continue;
            if (rank == 0)
                RCCL_OK(c, ncclRecv((char*)drecv.p + (off[r] - my), (size_t)h[r], ncclChar, r, comm, stream));
            else if (rank == r)
                RCCL_OK(c, ncclSend(dsend.p, (size_t)h[r], ncclChar, 0, comm, stream));
        }
        RCCL_OK(c, ncclGroupEnd());
        MPH_HIP_OK(c, hipStreamSynchronize(stream));
        if (rank == 0) {
            all.resize((size_t)total);
            std::memcpy(all.data(), mine.data(), mine.size());
            if (total > my)
                MPH_HIP_OK(c, hipMemcpy(all.data() + my, drecv.p, (size_t)(total - my), hipMemcpyDeviceToHost));
        }
        return MPH_OK;
    }
};

// Every message is staged through pinned host memory and handed to the caller's callback, which
// blocks the host: no graphs.
struct HostTransport final : Transport {
    int rank, nranks;
    mph_host_exchange_fn fn;
    void* user;
    char* stage = nullptr;   // pinned: 4 messages of `region` bytes (send l, send r, recv l, recv r)
    size_t region = 0;
    // the last exchange's copies into the device (they read `stage`): the next exchange, possibly
    // on the other stream, waits for them before the callback refills it
    hipEvent_t ev_stage = nullptr;
    bool stage_busy = false;

    HostTransport(int rank_, int nranks_, mph_host_exchange_fn fn_, void* user_)
        : rank(rank_), nranks(nranks_), fn(fn_), user(user_) {}
    ~HostTransport() override
    {
        if (ev_stage) (void)hipEventDestroy(ev_stage);
        if (stage) (void)hipHostFree(stage);
    }
    bool graphs_ok() const override { return false; }
    int comm_count() const override { return 0; }   // no communicator
    int start(MphCtx*) override { return MPH_OK; }

    int resize(MphCtx* c, size_t bytes) override
    {
        if (stage_busy) MPH_HIP_OK(c, hipEventSynchronize(ev_stage));   // no copy still reads it
        stage_busy = false;
        if (stage) (void)hipHostFree(stage);
        stage = nullptr;
        region = 0;
        MPH_HIP_OK(c, hipHostMalloc((void**)&stage, 4 * bytes, hipHostMallocDefault));
        region = bytes;
        return MPH_OK;
    }

    int exchange(MphCtx* c, hipStream_t stream, const Wire& l, const Wire& r) override
    {
        if (l.nsend > region || r.nsend > region || l.nrecv > region || r.nrecv > region)
            return ctx_fail(c, MPH_ERR_CAPACITY, "slab mode: message larger than the staging buffers");
        char* hs_l = stage;
        char* hs_r = stage + region;
        char* hr_l = stage + 2 * region;
        char* hr_r = stage + 3 * region;
        // the previous exchange's host-to-device copies may still read the receive halves (when it ran
        // on the other stream, this stream's synchronisation below does not cover them)
        if (stage_busy) MPH_HIP_OK(c, hipEventSynchronize(ev_stage));
        if (l.nsend) MPH_HIP_OK(c, hipMemcpyAsync(hs_l, l.send, l.nsend, hipMemcpyDeviceToHost, stream));
        if (r.nsend) MPH_HIP_OK(c, hipMemcpyAsync(hs_r, r.send, r.nsend, hipMemcpyDeviceToHost, stream));
        MPH_HIP_OK(c, hipStreamSynchronize(stream));
        if (fn(user, hs_l, l.nsend, hs_r, r.nsend, hr_l, l.nrecv, hr_r, r.nrecv) != 0)
            return ctx_fail(c, MPH_ERR_TRANSPORT, "host exchange callback failed");
        if (l.nrecv) MPH_HIP_OK(c, hipMemcpyAsync(l.recv, hr_l, l.nrecv, hipMemcpyHostToDevice, stream));
        if (r.nrecv) MPH_HIP_OK(c, hipMemcpyAsync(r.recv, hr_r, r.nrecv, hipMemcpyHostToDevice, stream));
        if (!ev_stage) MPH_HIP_OK(c, hipEventCreateWithFlags(&ev_stage, hipEventDisableTiming));
        MPH_HIP_OK(c, hipEventRecord(ev_stage, stream));
        stage_busy = true;
        return MPH_OK;
    }

    // n-1 rounds along the ring: each rank passes its running max left
    int max(MphCtx* c, hipStream_t, double* v, int n) override
    {
        std::vector<double> in((size_t)n);
        for (int round = 1; round < nranks; ++round) {
            if (fn(user, v, sizeof(double) * n, nullptr, 0, nullptr, 0, in.data(), sizeof(double) * n) != 0)
                return ctx_fail(c, MPH_ERR_TRANSPORT, "host exchange callback failed (collective max)");
            for (int k = 0; k < n; ++k) v[k] = std::max(v[k], in[k]);
        }
        return MPH_OK;
    }

    // R - 1 rounds along the ring; in round k every rank passes to its left neighbour what it
    // received in round k - 1 (first its own bytes), so rank 0 receives the bytes of rank k in round k
    int gather_root(MphCtx* c, hipStream_t, const std::vector<char>& mine, std::vector<char>& all) override
    {
        all.clear();
        std::vector<char> carry = rank == 0 ? std::vector<char>() : mine;
        if (rank == 0) all = mine;
        for (int round = 1; round < nranks; ++round) {
            long long so = (long long)carry.size(), si = 0;
            if (fn(user, &so, sizeof(so), nullptr, 0, nullptr, 0, &si, sizeof(si)) != 0)
                return ctx_fail(c, MPH_ERR_TRANSPORT, "host exchange callback failed (output gather sizes)");
            std::vector<char> in((size_t)si);
            if (fn(user, carry.data(), (size_t)so, nullptr, 0, nullptr, 0, in.data(), (size_t)si) != 0)
                return ctx_fail(c, MPH_ERR_TRANSPORT, "host exchange callback failed (output gather)");
            if (rank == 0) all.insert(all.end(), in.begin(), in.end());
            else carry.swap(in);
        }
        return MPH_OK;
    }
};

}  // namespace

namespace mph {

Transport* make_rccl_transport(int rank, int nranks, const char* unique_id128)
{
    return new RcclTransport(rank, nranks, unique_id128);
}

Transport* make_host_transport(int rank, int nranks, mph_host_exchange_fn fn, void* user)
{
    return new HostTransport(rank, nranks, fn, user);
}

// Message capacity (particles) of a direction whose live count is c: 25 % + 4096 particles of room
// to grow before the next capacity check (dist_sync, at most kSyncSteps steps later).  The slack
// can be lowered (MPH_SLAB_MSG_SLACK, tests of the growth path); both ranks of a pair read the same
// environment, so they still derive equal capacities for their shared direction.
// MPH_SLAB_MSG_CAP: one fixed capacity for every direction (tests of the overflow report)
int msg_capacity(const MphDist& D, int c) { return D.msg_fixed > 0 ? D.msg_fixed : c + c / 4 + D.msg_slack; }

// MPH_SLAB_MSG_CAP0_FRAC: the first sizing (mph_create) gives frac x the counts and no slack, so
// the first capacity check grows them (tests of the growth path)
int msg_capacity0(const MphDist& D, int c)
{
    return D.msg_cap0_frac > 0.0 ? std::max(1, (int)std::ceil(D.msg_cap0_frac * c)) : msg_capacity(D, c);
}

// (Re)allocate the four message buffers for the current capacities: redistribution (56 B per
// particle), pass-A halo (up to 40 B per particle of both directions' capacities), elastic ghosts.
int msg_alloc(MphCtx* c)
{
    MphDist& D = *c->dist;
    size_t region = 0;
    for (const DistSide& S : D.side) {
        region = std::max(region, kMsgHead + kMsgBytes * (size_t)std::max(S.cap_s, S.cap_r));
        region = std::max(region, sizeof(double) * 5 * (size_t)(S.cap_s + S.cap_r));
        region = std::max(region, 3 * sizeof(double4) * (size_t)std::max(S.nss, S.nsr));
    }
    region = (region + 255) & ~(size_t)255;
    if (region <= D.region && D.side[kLeft].send) return MPH_OK;
    for (DistSide& S : D.side)
        for (char** b : {&S.send, &S.recv}) {
            ctx_dfree(c, *b);
            *b = nullptr;
            MPH_CK(ctx_dalloc(c, b, region));
        }
    MPH_CK(D.tr->resize(c, region));   // (the host staging only after its wait for the last copies)
    D.region = region;
    return MPH_OK;
}

}  // namespace mph

extern "C" {

int mph_dist_unique_id(char* out128)
{
    if (!out128) return MPH_ERR_ARG;
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return MPH_ERR_RCCL;
    std::memcpy(out128, &id, sizeof(id));
    return MPH_OK;
}

int mph_dist_selftest(int device)
{
    // one-rank RCCL communicator whose left and right neighbour are itself: exercises the
    // group send/recv of the RCCL exchange including the per-peer message order that nranks == 2
    // relies on (our first receive from a peer = its first, left-going, send).  c: the error text
    // and the owner of the device buffers only
    MphCtx c;
    std::unique_ptr<Transport> tr;
    auto run = [&]() -> int {
        MPH_HIP_OK(&c, hipSetDevice(device));
        MPH_HIP_OK(&c, hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
        char uid[128];
        if (mph_dist_unique_id(uid) != MPH_OK) return ctx_fail(&c, MPH_ERR_RCCL, "ncclGetUniqueId failed");
        tr.reset(make_rccl_transport(0, 1, uid));
        MPH_CK(tr->start(&c));
        const size_t nl = 1000, nr = 37;
        std::vector<char> hl(nl), hr(nr), gl(nr), gr(nl);
        for (size_t i = 0; i < nl; ++i) hl[i] = (char)(i * 7 + 1);
        for (size_t i = 0; i < nr; ++i) hr[i] = (char)(i * 5 + 2);
        char *sl, *sr, *rl, *rr;
        MPH_CK(ctx_dalloc(&c, &sl, nl)); MPH_CK(ctx_dalloc(&c, &sr, nr));
        MPH_CK(ctx_dalloc(&c, &rl, nr)); MPH_CK(ctx_dalloc(&c, &rr, nl));
        MPH_HIP_OK(&c, hipMemcpy(sl, hl.data(), nl, hipMemcpyHostToDevice));
        MPH_HIP_OK(&c, hipMemcpy(sr, hr.data(), nr, hipMemcpyHostToDevice));
        // left-going (sl) must arrive as from-right (rr); right-going (sr) as from-left (rl)
        const Wire left{0, sl, nl, rl, nr}, right{0, sr, nr, rr, nl};
        MPH_CK(tr->exchange(&c, c.stream, left, right));
        // a zero-byte direction is skipped on both sides
        MPH_CK(tr->exchange(&c, c.stream, Wire{0, sl, 0, rl, nr}, Wire{0, sr, nr, rr, 0}));
        MPH_HIP_OK(&c, hipStreamSynchronize(c.stream));
        MPH_HIP_OK(&c, hipMemcpy(gl.data(), rl, nr, hipMemcpyDeviceToHost));
        MPH_HIP_OK(&c, hipMemcpy(gr.data(), rr, nl, hipMemcpyDeviceToHost));
        if (gl != hr || gr != hl) return ctx_fail(&c, MPH_ERR_RCCL, "RCCL self-exchange delivered wrong bytes");
        // the max-reduction (overlap_probe) over the one rank: the values come back as they were
        const double want[3] = {1.5, -2.0, 3.25e10};
        double got[3] = {want[0], want[1], want[2]};
        MPH_CK(tr->max(&c, c.stream, got, 3));
        if (std::memcmp(got, want, sizeof(want)) != 0)
            return ctx_fail(&c, MPH_ERR_RCCL, "RCCL max-reduction over one rank changed the values");
        // the same exchange captured into a hipGraph and replayed (slab steps replay RCCL calls
        // from captured graphs)
        MPH_HIP_OK(&c, hipMemset(rl, 0, nr));
        MPH_HIP_OK(&c, hipMemset(rr, 0, nl));
        hipGraph_t g = nullptr;
        hipGraphExec_t ge = nullptr;
        MPH_HIP_OK(&c, hipStreamBeginCapture(c.stream, hipStreamCaptureModeThreadLocal));
        const int rc = tr->exchange(&c, c.stream, left, right);
        const hipError_t e = hipStreamEndCapture(c.stream, &g);
        MPH_CK(rc);
        MPH_HIP_OK(&c, e);
        const hipError_t ei = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        MPH_HIP_OK(&c, ei);
        for (int rep = 0; rep < 2; ++rep) MPH_HIP_OK(&c, hipGraphLaunch(ge, c.stream));
        MPH_HIP_OK(&c, hipStreamSynchronize(c.stream));
        (void)hipGraphExecDestroy(ge);
        MPH_HIP_OK(&c, hipMemcpy(gl.data(), rl, nr, hipMemcpyDeviceToHost));
        MPH_HIP_OK(&c, hipMemcpy(gr.data(), rr, nl, hipMemcpyDeviceToHost));
        if (gl != hr || gr != hl) return ctx_fail(&c, MPH_ERR_RCCL, "graph-replayed RCCL exchange delivered wrong bytes");
        // the early send's pattern (dist_enqueue_step): per step the exchange forks onto a second
        // stream after an event of the main stream, main-stream work runs beside it, and the
        // next step joins it -- three chained steps in one captured graph, replayed twice
        hipStream_t s2 = nullptr;
        hipEvent_t es = nullptr, ex = nullptr;
        MPH_HIP_OK(&c, hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
        MPH_HIP_OK(&c, hipEventCreateWithFlags(&es, hipEventDisableTiming));
        MPH_HIP_OK(&c, hipEventCreateWithFlags(&ex, hipEventDisableTiming));
        char* side;
        MPH_CK(ctx_dalloc(&c, &side, 1 << 20));
        MPH_HIP_OK(&c, hipMemset(rl, 0, nr));
        MPH_HIP_OK(&c, hipMemset(rr, 0, nl));
        MPH_HIP_OK(&c, hipStreamBeginCapture(c.stream, hipStreamCaptureModeThreadLocal));
        int rc2 = MPH_OK;
        for (int k = 0; k < 3 && rc2 == MPH_OK; ++k) {
            if (k > 0) (void)hipStreamWaitEvent(c.stream, ex, 0);
            (void)hipEventRecord(es, c.stream);
            (void)hipStreamWaitEvent(s2, es, 0);
            rc2 = tr->exchange(&c, s2, left, right);
            (void)hipEventRecord(ex, s2);
            (void)hipMemsetAsync(side, k, 1 << 20, c.stream);   // work beside the exchange
        }
        (void)hipStreamWaitEvent(c.stream, ex, 0);
        const hipError_t e2 = hipStreamEndCapture(c.stream, &g);
        MPH_CK(rc2);
        MPH_HIP_OK(&c, e2);
        const hipError_t ei2 = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        MPH_HIP_OK(&c, ei2);
        for (int rep = 0; rep < 2; ++rep) MPH_HIP_OK(&c, hipGraphLaunch(ge, c.stream));
        MPH_HIP_OK(&c, hipStreamSynchronize(c.stream));
        (void)hipGraphExecDestroy(ge);
        (void)hipEventDestroy(es);
        (void)hipEventDestroy(ex);
        (void)hipStreamDestroy(s2);
        MPH_HIP_OK(&c, hipMemcpy(gl.data(), rl, nr, hipMemcpyDeviceToHost));
        MPH_HIP_OK(&c, hipMemcpy(gr.data(), rr, nl, hipMemcpyDeviceToHost));
        if (gl != hr || gr != hl)
            return ctx_fail(&c, MPH_ERR_RCCL, "forked graph-replayed RCCL exchanges delivered wrong bytes");
        return MPH_OK;
    };
    const int status = run();
    ctx_set_global_error(c.err);
    (void)hipStreamSynchronize(c.stream);
    tr.reset();
    for (void* p : c.allocs) (void)hipFree(p);
    if (c.stream) (void)hipStreamDestroy(c.stream);
    return status;
}

}  // extern "C"
