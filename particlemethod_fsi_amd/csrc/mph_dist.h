// mph_dist.h -- what the units of the slab decomposition share: the per-rank state (MphDist), the
// transport interface (mph_transport.hip), the slab geometry (mph_slab_geom.hip), the step protocol
// (mph_dist.hip) and the collective output (mph_dist_output.hip).
#pragma once

#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "mph_ctx.h"

namespace mph {

constexpr size_t kMsgBytes = 56;   // per particle, k_dist_pack layout
constexpr size_t kMsgHead = 16;    // message header: the two class counts
constexpr double kStructMargin = 4.0;   // x ParticleSpacing: elastic particle displacement across a face

enum { kLeft = 0, kRight = 1 };   // the two sides of a slab (index of MphDist::side)

// one neighbour's half of an exchange: nsend bytes of send go to peer, nrecv bytes from it land in recv
struct Wire {
    int peer;
    const void* send;
    size_t nsend;
    void* recv;
    size_t nrecv;
};

// The three operations the step protocol and the output need from whatever moves the bytes; RCCL
// (ncclSend/ncclRecv over xGMI) or a host callback (tests, hosts without RCCL).  c: where errors go.
struct Transport {
    virtual ~Transport() = default;
    // join the ranks (collective; the context's device is current)
    virtual int start(MphCtx* c) = 0;
    // to the left neighbour (arrives there as its from-right message) and to the right one (its
    // from-left), on `stream`; a zero-byte direction is skipped on both sides
    virtual int exchange(MphCtx* c, hipStream_t stream, const Wire& left, const Wire& right) = 0;
    // element-wise max of v[0..n) over all ranks (every rank ends with the same values)
    virtual int max(MphCtx* c, hipStream_t stream, double* v, int n) = 0;
    // rank 0 receives the concatenation of every rank's bytes in rank order; the others get nothing
    virtual int gather_root(MphCtx* c, hipStream_t stream, const std::vector<char>& mine, std::vector<char>& all) = 0;
    // the message buffers now hold `region` bytes each (msg_alloc)
    virtual int resize(MphCtx* c, size_t region) { return MPH_OK; }
    virtual bool graphs_ok() const = 0;   // exchanges may be captured into step graphs
    virtual int comm_count() const = 0;   // the communicator's own size (mph_dist_info)
};
Transport* make_rccl_transport(int rank, int nranks, const char* unique_id128);
Transport* make_host_transport(int rank, int nranks, mph_host_exchange_fn fn, void* user);

// what a rank keeps per neighbour
struct DistSide {
    int peer = 0;
    char *send = nullptr, *recv = nullptr;   // device message buffers (MphDist::region bytes each)
    int cap_s = 0, cap_r = 0;                // message capacities (particles) to / from the neighbour
    // elastic ghost slots (static): local slot indices sent to / received from the neighbour
    int *ss = nullptr, *sr = nullptr;
    int nss = 0, nsr = 0;
    Wire wire(size_t nsend, size_t nrecv) const { return {peer, send, nsend, recv, nrecv}; }
};

}  // namespace mph

// Multi-GPU state of one rank (one process per GPU).  Local particle arrays hold
// [owned | ghosts] in cell order; see mph_dist.hip for the step protocol.
struct MphDist {
    int rank = 0, nranks = 1;
    mph::SlabGeom g{};
    std::vector<double> cuts;     // interior slab boundaries (MphSlabOptions.cuts); empty: equal widths
    int cap = 0;                  // capacity of every local per-particle array
    int n_own = 0;                // owned particles after the last redistribution (host mirror)
    // Every size of a step lives on the device (DistLayout), so a step has no host round trip and
    // the RCCL transport replays whole steps from captured graphs.  Messages travel with fixed
    // capacities (particles) per direction; a pair of neighbours derives the same capacity for
    // its shared direction from the same counts (send of one = receive of the other).
    mph::DistLayout* lay = nullptr;    // device
    mph::DistLayout* hlay = nullptr;   // pinned host mirror (read after a step batch)
    mph::DistSide side[2];        // kLeft, kRight
    size_t region = 0;            // bytes of each of the four message buffers
    // MPH_SLAB_MSG_SLACK / _CAP0_FRAC / _CAP (msg_capacity, mph_transport.hip)
    int msg_slack = 4096, msg_fixed = 0;
    double msg_cap0_frac = 0.0;
    mph::Soa C;                   // redistributed state (pre-sort order)
    int* cls = nullptr;           // class of every B entry
    // the kept entries of C stay in B (VSrc: C holds the received tail only, vidx[v] = where
    // entry v lives in B); MPH_SLAB_VIRTUAL_C=0 copies them into C
    int* vidx = nullptr;
    bool virt = true;
    int* bcnt = nullptr;          // per (class, block) counts -> offsets
    int* boff = nullptr;
    int* bsum = nullptr;
    hipStream_t stream2 = nullptr;                   // halo exchange beside the inner pass B
    hipEvent_t ev_a = nullptr, ev_h = nullptr;       // pass A done / halo landed
    std::unique_ptr<mph::Transport> tr;
    bool graphs = false;          // steps replayed from captured graphs (RCCL transport)
    // overlap: pass B of the inner particles overlaps the pass-A halo (and the early send below);
    // off: halo, then one pass B over all particles.  MPH_SLAB_OVERLAP=1 / =0 forces the mode;
    // unset (or "auto") the ranks choose it together at creation (overlap_probe, mph_dist.hip): on
    // when the measured exchanges take longer than the split pass B costs over the single one
    bool overlap = false;
    int overlap_mode = -1;
    // the probe's measurements, max over ranks (ms): halo exchange, redistribution exchange (both at
    // their message capacities), pass B split in two launches minus pass B in one; -1: not probed
    double probe_ms[3] = {-1.0, -1.0, -1.0};
    // early send: within a batch of steps, the redistribution messages of the next step leave
    // while the interior pass B of this one runs (no elastic particles; MPH_SLAB_EARLY=0: off)
    bool early = true;
    int* wface = nullptr;                             // face-wavefront flags of the last pass B
    hipEvent_t ev_s = nullptr, ev_x = nullptr;       // early messages packed / exchanged
};

namespace mph {

// -- slab geometry (mph_slab_geom.hip) ----------------------------------------------------------
// Slab of `rank` along `axis`: equal widths, or the caller's cuts (nranks - 1 interior
// coordinates, ascending; MphSlabOptions.cuts); hi(r) and lo(r+1) are the same expression.
void slab_of(const HostDerived& h, int axis, int rank, int nranks, const double* cuts, double& lo, double& hi);
// cuts strictly ascending inside the domain (NULL: equal widths)
int check_cuts(const HostDerived& h, int axis, int nranks, const double* cuts, std::string& err);
SlabGeom make_geom(const HostDerived& h, int axis, int rank, int nranks, const double* cuts, double halo);
double wrap_coord(const HostDerived& h, int axis, double x);
int owner_rank(const HostDerived& h, int axis, int nranks, const double* cuts, double x);
// owner[i] = owner_rank of origin_a + (double)i * spacing_a, each rounded: who owns plane i of an
// axis-aligned lattice along the slab axis (mph_slab_lattice_owner, the mph_dist_* lattice calls)
void lattice_owners(const HostDerived& h, int axis, int nranks, const double* cuts, double origin_a, double spacing_a,
                    int count_a, int* owner);
// signed periodic offset of x from the centre of rank r's slab
double slab_offset(const HostDerived& h, int axis, int r, int nranks, const double* cuts, double x);
int check_geometry(const MphConfig& cfg, int nranks, int axis, std::string& err);
inline double halo_width(const DevParams& P) { return std::sqrt(P.rc2) * (1.0 + 1e-6); }
inline const double* dist_cuts(const MphDist& D) { return D.cuts.empty() ? nullptr : D.cuts.data(); }

// -- message buffers (mph_transport.hip) --------------------------------------------------------
int msg_capacity(const MphDist& D, int c);    // of a direction whose live count is c
int msg_capacity0(const MphDist& D, int c);   // the first sizing (mph_create)
int msg_alloc(MphCtx* c);                     // (re)allocate for the current capacities

// -- step protocol (mph_dist.hip) ---------------------------------------------------------------
template <typename T>
T* lay_field(DistLayout* lay, size_t off) { return reinterpret_cast<T*>(reinterpret_cast<char*>(lay) + off); }
// step 5, or any per-particle fields of the ghosts
int halo_exchange(MphCtx* c, Profiler* prof, hipStream_t stream, const HaloFields* fields = nullptr);

}  // namespace mph
