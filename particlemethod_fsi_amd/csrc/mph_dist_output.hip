// mph_dist_output.hip -- output in slab mode (collective calls: every rank enters them at the same
// step; host only, no kernels).
//
// The reference writes .prof before a step, runs calculateVirialStressAtParticle and writes .vtk
// after one (main.cpp:583-589, 672-683, 957-1189), always for the whole problem.  Here every rank
// packs the records of the particles it owns, rank 0 gathers them (RCCL: one receive from every
// rank; host transport: forwarded along the ring of neighbour exchanges), restores the original
// order and writes the file with the single-context writers, so the bytes are the reference's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "mph_dist.h"

using namespace mph;

namespace {

// one owned particle of an output gather (original index, and what the writers print)
struct OutRec {
    int id, prop, nc, pad;
    double pos[3], pos0[3], vel[3], acc[3], force[3];
};
// one owned elastic slot: InitialStructureNeighborCount, Stress, Strain
struct OutSlot {
    int id, isnc;
    double S[9], E[9];
};

// the records of the particles (and elastic slots) this rank owns, behind two counts
int pack_owned(MphCtx* c, std::vector<char>& buf)
{
    const int n = c->n;
    std::vector<int> id, nc;
    std::vector<double> x, y, z, vx, vy, vz;
    std::vector<double4> f, a;
    MPH_CK(fetch(c, (const int*)c->L.A.id, id, n));
    MPH_CK(fetch(c, (const int*)c->L.nbcount, nc, n));
    MPH_CK(fetch(c, (const double*)c->L.B.x, x, n));
    MPH_CK(fetch(c, (const double*)c->L.B.y, y, n));
    MPH_CK(fetch(c, (const double*)c->L.B.z, z, n));
    MPH_CK(fetch(c, (const double*)c->L.B.vx, vx, n));
    MPH_CK(fetch(c, (const double*)c->L.B.vy, vy, n));
    MPH_CK(fetch(c, (const double*)c->L.B.vz, vz, n));
    MPH_CK(fetch(c, (const double4*)c->L.force, f, n));
    MPH_CK(fetch(c, (const double4*)c->L.acc, a, n));
    const int ns = c->Sd.n_own;
    std::vector<double> S, E;
    const size_t fes = (size_t)c->Sd.fes;   // nine element planes (StructDev)
    if (ns) {
        MPH_CK(fetch(c, (const double*)c->Sd.S, S, 9 * fes));
        MPH_CK(fetch(c, (const double*)c->Sd.E, E, 9 * fes));
    }
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    std::vector<OutRec> rec;
    rec.reserve((size_t)c->dist->n_own);
    for (int i = 0; i < n; ++i) {
        if (id[i] < 0) continue;   // a ghost
        OutRec r{};
        r.id = id[i];
        // host index of the static inputs (original order, or the slab-local creation's ids)
        const size_t k = c->gid.empty() ? (size_t)id[i]
                                        : (size_t)(std::lower_bound(c->gid.begin(), c->gid.end(), id[i]) - c->gid.begin());
        if (k >= c->prop.size()) return ctx_fail(c, MPH_ERR_ARG, "slab output: an owned particle without static inputs");
        r.prop = c->prop[k];
        r.nc = nc[i];
        const double p[3] = {x[i], y[i], z[i]}, v[3] = {vx[i], vy[i], vz[i]};
        const double ac[3] = {a[i].x, a[i].y, a[i].z}, fo[3] = {f[i].x, f[i].y, f[i].z};
        for (int d = 0; d < 3; ++d) {
            r.pos[d] = p[d];
            r.pos0[d] = c->pos0[3 * k + d];
            r.vel[d] = v[d];
            r.acc[d] = ac[d];
            r.force[d] = fo[d];
        }
        rec.push_back(r);
    }
    std::vector<OutSlot> sl((size_t)ns);
    for (int s = 0; s < ns; ++s) {
        sl[s].id = c->sl_orig[s];
        sl[s].isnc = c->S.count[c->sl_s[s]];
        for (int e = 0; e < 9; ++e) {
            sl[s].S[e] = S[e * fes + s];
            sl[s].E[e] = E[e * fes + s];
        }
    }
    const long long cnt[2] = {(long long)rec.size(), (long long)sl.size()};
    buf.resize(sizeof(cnt) + sizeof(OutRec) * rec.size() + sizeof(OutSlot) * sl.size());
    char* o = buf.data();
    std::memcpy(o, cnt, sizeof(cnt));
    o += sizeof(cnt);
    if (!rec.empty()) std::memcpy(o, rec.data(), sizeof(OutRec) * rec.size());
    o += sizeof(OutRec) * rec.size();
    if (!sl.empty()) std::memcpy(o, sl.data(), sizeof(OutSlot) * sl.size());
    return MPH_OK;
}

// the arrays of the single-context writers, in original order, from every rank's records
struct OutArrays {
    std::vector<int> prop, isnc, nc;
    std::vector<double> pos, pos0, vel, acc, force, stress, strain;
};

int unpack_all(MphCtx* c, const std::vector<char>& all, int nranks, OutArrays& o)
{
    const size_t n = (size_t)c->n_glob;
    o.prop.assign(n, 0); o.isnc.assign(n, 0); o.nc.assign(n, 0);
    o.pos.assign(3 * n, 0.0); o.pos0.assign(3 * n, 0.0); o.vel.assign(3 * n, 0.0);
    o.acc.assign(3 * n, 0.0); o.force.assign(3 * n, 0.0);
    o.stress.assign(9 * n, 0.0); o.strain.assign(9 * n, 0.0);
    std::vector<char> seen(n, 0);
    size_t got = 0;
    const char* p = all.data();
    const char* end = p + all.size();
    for (int r = 0; r < nranks; ++r) {
        long long cnt[2];
        if ((size_t)(end - p) < sizeof(cnt)) return ctx_fail(c, MPH_ERR_TRANSPORT, "slab output: truncated gather");
        std::memcpy(cnt, p, sizeof(cnt));
        p += sizeof(cnt);
        if ((size_t)(end - p) < sizeof(OutRec) * cnt[0] + sizeof(OutSlot) * cnt[1])
            return ctx_fail(c, MPH_ERR_TRANSPORT, "slab output: truncated gather");
        for (long long k = 0; k < cnt[0]; ++k, p += sizeof(OutRec)) {
            OutRec q;
            std::memcpy(&q, p, sizeof(q));
            if (q.id < 0 || (size_t)q.id >= n || seen[q.id])
                return ctx_fail(c, MPH_ERR_CAPACITY, "slab output: ownership is not a partition");
            seen[q.id] = 1;
            ++got;
            const size_t i = (size_t)q.id;
            o.prop[i] = q.prop;
            o.nc[i] = q.nc;
            for (int d = 0; d < 3; ++d) {
                o.pos[3 * i + d] = q.pos[d];
                o.pos0[3 * i + d] = q.pos0[d];
                o.vel[3 * i + d] = q.vel[d];
                o.acc[3 * i + d] = q.acc[d];
                o.force[3 * i + d] = q.force[d];
            }
        }
        for (long long k = 0; k < cnt[1]; ++k, p += sizeof(OutSlot)) {
            OutSlot q;
            std::memcpy(&q, p, sizeof(q));
            if (q.id < 0 || (size_t)q.id >= n) return ctx_fail(c, MPH_ERR_TRANSPORT, "slab output: bad slot record");
            const size_t i = (size_t)q.id;
            o.isnc[i] = q.isnc;
            std::memcpy(&o.stress[9 * i], q.S, sizeof(q.S));
            std::memcpy(&o.strain[9 * i], q.E, sizeof(q.E));
        }
    }
    if (got != n) return ctx_fail(c, MPH_ERR_CAPACITY, "slab output: " + std::to_string(n - got) + " particles owned by no rank");
    return MPH_OK;
}

}  // namespace

namespace mph {

int dist_write_output(MphCtx* c, const char* path, int kind)
{
    MphDist& D = *c->dist;
    std::vector<char> mine, all;
    MPH_CK(pack_owned(c, mine));
    MPH_CK(D.tr->gather_root(c, c->stream, mine, all));
    mine.clear();
    mine.shrink_to_fit();
    if (D.rank != 0) return MPH_OK;
    auto o = std::make_shared<OutArrays>();
    MPH_CK(unpack_all(c, all, D.nranks, *o));
    all.clear();
    all.shrink_to_fit();
    const int n = c->n_glob;
    if (kind == kOutProf)
        return mph_write_prof_arrays(path, &c->cfg, c->time, n, o->prop.data(), o->pos.data(), o->pos0.data(),
                                     o->vel.data());
    auto write = [o, n](const std::string& pth, bool xml) {
        auto writer = xml ? mph_write_vtu_arrays : mph_write_vtk_arrays;
        return writer(pth.c_str(), n, o->prop.data(), o->pos.data(), o->pos0.data(), o->vel.data(), o->acc.data(),
                      o->force.data(), o->stress.data(), o->strain.data(), o->isnc.data(), o->nc.data());
    };
    if (kind == kOutVtkAsync) {
        const std::string pth = path;
        c->out_thread = std::thread([c, write, pth] { c->out_rc = write(pth, false); });
        return MPH_OK;
    }
    const int rc = write(path, kind == kOutVtu);
    return rc ? ctx_fail(c, rc, std::string("writing ") + path) : MPH_OK;
}

// calculateVirialStressAtParticle (main.cpp:3077-3318) in slab mode: the owned particles' sums need
// their ghost neighbours' post-step positions and velocities, which the owners computed -- one
// halo exchange of B (the pass-A values the virial reads are the particle's own)
int dist_virial(MphCtx* c)
{
    HaloFields F{};
    F.nf = 3;
    F.f[0] = c->L.B.x; F.f[1] = c->L.B.y; F.f[2] = c->L.B.z;
    MPH_CK(halo_exchange(c, nullptr, c->stream, &F));
    F.f[0] = c->L.B.vx; F.f[1] = c->L.B.vy; F.f[2] = c->L.B.vz;
    MPH_CK(halo_exchange(c, nullptr, c->stream, &F));
    MPH_CK(virial_full_lists(c));
    launch_virial(c->L, c->L.B, c->vir, c->vpres);
    MPH_HIP_OK(c, hipGetLastError());
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    return MPH_OK;
}

}  // namespace mph
