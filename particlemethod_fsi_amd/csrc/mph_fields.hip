// mph_fields.hip -- the fields of a context: download in the reference's AoS layout and original
// particle order (mph_get), upload (mph_set), the virial diagnostic, the file writers, the host half
// of the particle selections (mph_select*; kernels: mph_select.hip) and of the kinematics
// (mph_compute_kinematics and its readers; kernels: mph_kinematics.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "mph_dist.h"

using namespace mph;

namespace mph {

// calculateVirialStressAtParticle evaluates the step's lists at the positions after the step
// (main.cpp:672-673, 3077-3318): a pair of the shell MaxRadius < r <= MaxRadius + MARGIN at the search
// may have moved inside a radius by then, so the virial needs the reference's whole lists.  With
// the lists kept to the passes' radius (DevParams.rlf) the step's search is repeated over the same
// sorted set A and cell table (unchanged since the step's sort) storing every neighbour -- the
// lists the step would have built with MPH_LIST_FULL=1; the XCD work histogram is left alone.
int virial_full_lists(MphCtx* c)
{
    if (c->P.rlf >= 3.0e38f) return MPH_OK;
    DevParams Pf = c->P;
    Pf.rlf = 3.0e38f;
    Launch L = c->L;
    L.P = &Pf;
    L.xcd_bal_min = 0x7fffffff;
    launch_neighbors(L);
    MPH_HIP_OK(c, hipGetLastError());
    return MPH_OK;
}

}  // namespace mph

namespace {

// Sorted device arrays -> host original order: the first `len` elements of each array of src and
// the id array of their order (A.id / B.id); put(h, i, id) copies particle i's elements from the
// host copies to where original index id belongs.  h is an array of N vectors, one per source
// array: h[k][i] is element i of src[k] (a single array: h[0][i]).  Slab mode: ghosts (id < 0) skipped.
template <typename T, size_t N, typename Put>
int download(MphCtx* c, T* const (&src)[N], size_t len, const int* ids, Put put)
{
    std::vector<T> h[N];
    std::vector<int> id;
    for (size_t k = 0; k < N; ++k) MPH_CK(fetch(c, (const T*)src[k], h[k], len));
    MPH_CK(fetch(c, ids, id, (size_t)c->n));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < id.size(); ++i)
        if (id[i] >= 0) put(h, i, (size_t)id[i]);
    return MPH_OK;
}

int download_struct_m33(MphCtx* c, const double* d, double* out)
{
    const int ns = c->Sd.n_own;   // slots computed here (slab mode: owned)
    std::memset(out, 0, sizeof(double) * 9 * (size_t)c->n_glob);
    if (ns == 0) return MPH_OK;
    const size_t fes = (size_t)c->Sd.fes;   // nine element planes (StructDev)
    std::vector<double> h(fes * 9);
    MPH_HIP_OK(c, hipMemcpyAsync(h.data(), d, sizeof(double) * 9 * fes, hipMemcpyDeviceToHost, c->stream));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    for (int s = 0; s < ns; ++s) {
        double* o = out + (size_t)9 * c->sl_orig[s];
        for (int e = 0; e < 9; ++e) o[e] = h[e * fes + s];
    }
    return MPH_OK;
}

}  // namespace

extern "C" {

int mph_get(MphCtx* c, int field, void* out)
{
    if (!out) return MPH_ERR_ARG;
    MPH_CK(ctx_enter(c));
    double* o = (double*)out;
    int* oi = (int*)out;
    // structure rows: every list built here (single context), or the slots this rank computes
    // (slab mode: its owned elastic particles; the lists of ghost slots are partial)
    const int ns = c->dist ? (int)c->sl_s.size() : (int)c->S.orig.size();
    auto sidx = [c](int k) { return c->dist ? c->sl_s[k] : k; };
    // static inputs: every particle, or (slab-local creation) the ones this rank was created with
    const int nin = (int)c->prop.size();
    // sorted device arrays -> original order (download; in its callbacks h[k][i] is element i of
    // the k-th array given): get3 three component arrays into [id][3], get4 the xyz of a double4
    // array in A order into [id][3], get1 a scalar array in A order into out[id]
    const size_t n = (size_t)c->n;
    auto get3 = [&](double* x, double* y, double* z, const int* ids) {
        double* const src[3] = {x, y, z};
        return download(c, src, n, ids, [o](auto* h, size_t i, size_t id) {
            for (int k = 0; k < 3; ++k) o[3 * id + k] = h[k][i];
        });
    };
    auto get4 = [&](double4* d) {
        double4* const src[1] = {d};
        return download(c, src, n, c->L.A.id, [o](auto* h, size_t i, size_t id) {
            o[3 * id] = h[0][i].x; o[3 * id + 1] = h[0][i].y; o[3 * id + 2] = h[0][i].z;
        });
    };
    auto get1 = [&](auto* d, auto* out) {
        decltype(d) const src[1] = {d};   // (an array of one pointer to d's element type)
        return download(c, src, n, c->L.A.id, [out](auto* h, size_t i, size_t id) { out[id] = h[0][i]; });
    };
    switch (field) {
    case MPH_FIELD_POSITION: return get3(c->L.B.x, c->L.B.y, c->L.B.z, c->L.B.id);
    case MPH_FIELD_VELOCITY: return get3(c->L.B.vx, c->L.B.vy, c->L.B.vz, c->L.B.id);
    case MPH_FIELD_INITIAL_POSITION:
        for (int k = 0; k < nin; ++k) std::memcpy(o + 3 * (size_t)glob_id(c, k), &c->pos0[3 * (size_t)k], 3 * sizeof(double));
        return MPH_OK;
    case MPH_FIELD_FORCE: return get4(c->L.force);
    case MPH_FIELD_ACCELERATION: return get4(c->L.acc);
    case MPH_FIELD_GRAVITY_CENTER: return get3(c->L.gx, c->L.gy, c->L.gz, c->L.A.id);
    case MPH_FIELD_PRESSURE_P: return get1(c->L.pres, o);
    case MPH_FIELD_PRESSURE_A: return get1(c->L.pa, o);
    case MPH_FIELD_DENSITY_A: return get1(c->L.dens_a, o);
    case MPH_FIELD_VOL_STRAIN_P: return get1(c->L.vstrain, o);
    case MPH_FIELD_DIVERGENCE_P: return get1(c->L.divp, o);
    case MPH_FIELD_NEIGHBOR_COUNT: return get1(c->L.nbcount, oi);
    case MPH_FIELD_MASS:
        for (int k = 0; k < nin; ++k) o[glob_id(c, k)] = c->cfg.density[c->prop[k]] * c->h.vol;
        return MPH_OK;
    case MPH_FIELD_KAPPA: {
        // initializeFluid (1317-1319) before the first step, calculatePhysicalCoefficients after
        std::vector<double> vs(c->stepped ? (size_t)c->n_glob : 0, 0.0);
        if (c->stepped) MPH_CK(get1(c->L.vstrain, vs.data()));
        for (int k = 0; k < nin; ++k) {
            const int i = glob_id(c, k);
            o[i] = (c->stepped && vs[i] < 0.0) ? 0.0 : c->cfg.bulk_modulus[c->prop[k]];
        }
        return MPH_OK;
    }
    case MPH_FIELD_LAMBDA:
        for (int k = 0; k < nin; ++k) o[glob_id(c, k)] = c->cfg.bulk_viscosity[c->prop[k]];
        return MPH_OK;
    case MPH_FIELD_MU:
        for (int k = 0; k < nin; ++k) o[glob_id(c, k)] = c->cfg.shear_viscosity[c->prop[k]];
        return MPH_OK;
    case MPH_FIELD_PROPERTY:
        for (int k = 0; k < nin; ++k) oi[glob_id(c, k)] = c->prop[k];
        return MPH_OK;
    case MPH_FIELD_INITIAL_STRUCTURE_NEIGHBOR_COUNT:
        for (int k = 0; k < nin; ++k) oi[glob_id(c, k)] = 0;
        for (int k = 0; k < ns; ++k) oi[glob_id(c, c->S.orig[sidx(k)])] = c->S.count[sidx(k)];
        return MPH_OK;
    case MPH_FIELD_DEFORM_GRADIENT: return download_struct_m33(c, c->Sd.F, o);
    case MPH_FIELD_STRAIN: return download_struct_m33(c, c->Sd.E, o);
    case MPH_FIELD_STRESS: return download_struct_m33(c, c->Sd.S, o);
    case MPH_FIELD_NORMALIZER:
        for (int k = 0; k < nin; ++k) std::memset(o + (size_t)9 * glob_id(c, k), 0, sizeof(double) * 9);
        for (int k = 0; k < ns; ++k)
            std::memcpy(o + (size_t)9 * glob_id(c, c->S.orig[sidx(k)]), &c->S.normalizer[(size_t)9 * sidx(k)],
                        sizeof(double) * 9);
        return MPH_OK;
    case MPH_FIELD_VIRIAL_STRESS:
    case MPH_FIELD_VIRIAL_PRESSURE: {
        const size_t w = field == MPH_FIELD_VIRIAL_STRESS ? 9 : 1;
        std::memset(o, 0, sizeof(double) * w * (size_t)c->n_glob);
        if (!c->vir) return MPH_OK;   // never computed (the reference's array is uninitialised)
        double* const src[1] = {w == 9 ? c->vir : c->vpres};
        return download(c, src, w * n, c->L.A.id, [o, w](auto* h, size_t i, size_t id) {
            std::memcpy(o + w * id, &h[0][w * i], sizeof(double) * w);
        });
    }
    case MPH_FIELD_LAMBDA_LAMES:
    case MPH_FIELD_MU_LAMES:
        for (int k = 0; k < nin; ++k) o[glob_id(c, k)] = 0.0;
        for (int k = 0; k < ns; ++k)
            o[glob_id(c, c->S.orig[sidx(k)])] =
                field == MPH_FIELD_LAMBDA_LAMES ? c->S.lame_l[sidx(k)] : c->S.lame_m[sidx(k)];
        return MPH_OK;
    default: return ctx_fail(c, MPH_ERR_ARG, "unknown field " + std::to_string(field));
    }
}

int mph_compute_virial(MphCtx* c)
{
    MPH_CK(ctx_enter(c));
    if (!c->vir) {
        // slab mode: the array capacity (c->P.n), the held count changes every step
        const size_t cap = (size_t)std::max(c->dist ? c->P.n : c->n, 1);
        MPH_CK(ctx_dalloc(c, &c->vir, 9 * cap));
        MPH_CK(ctx_dalloc(c, &c->vpres, cap));
    }
    if (c->dist) return dist_virial(c);
    // after a step the integrated state B is in A (list) order; before the first step A is current
    if (c->phase_timing) MPH_HIP_OK(c, hipEventRecord(c->ev_vir[0], c->stream));
    MPH_CK(virial_full_lists(c));
    launch_virial(c->L, c->stepped ? c->L.B : c->L.A, c->vir, c->vpres);
    MPH_HIP_OK(c, hipGetLastError());
    if (c->phase_timing) MPH_HIP_OK(c, hipEventRecord(c->ev_vir[1], c->stream));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    if (c->phase_timing) {
        float ms = 0.0f;
        MPH_HIP_OK(c, hipEventElapsedTime(&ms, c->ev_vir[0], c->ev_vir[1]));
        c->phase_ms[2] += ms;
    }
    return MPH_OK;
}

int mph_set(MphCtx* c, int field, const void* in)
{
    if (!c || !in) return MPH_ERR_ARG;
    MPH_CK(ctx_flush(c));
    if (field != MPH_FIELD_POSITION && field != MPH_FIELD_VELOCITY)
        return ctx_fail(c, MPH_ERR_ARG, "mph_set supports Position and Velocity");
    MPH_HIP_OK(c, hipSetDevice(c->device));
    c->a_current = false;   // the sorted set A is the last step's, no longer this state's (mph_sample_grid)
    c->sel_current = false; // nor is the selection this state's (mph_select)
    c->kin_current = false; // nor the kinematics, and none can be computed before the next step
    c->set_since_step = true;
    const int n = c->n;
    const double* v = (const double*)in;
    // current state lives in the B set in the order of B.id: rewrite it in that order
    std::vector<double> h(n);
    std::vector<int> id(n);
    MPH_HIP_OK(c, hipMemcpy(id.data(), c->L.B.id, sizeof(int) * n, hipMemcpyDeviceToHost));
    double* dst[3] = {c->L.B.x, c->L.B.y, c->L.B.z};
    if (field == MPH_FIELD_VELOCITY) { dst[0] = c->L.B.vx; dst[1] = c->L.B.vy; dst[2] = c->L.B.vz; }
    for (int k = 0; k < 3; ++k) {
        for (int i = 0; i < n; ++i) h[i] = id[i] >= 0 ? v[3 * (size_t)id[i] + k] : 0.0;
        MPH_HIP_OK(c, hipMemcpy(dst[k], h.data(), sizeof(double) * n, hipMemcpyHostToDevice));
    }
    return MPH_OK;
}

int mph_set_initial_velocity_profile(MphCtx* c)
{
    MPH_CK(ctx_enter(c));
    const size_t n = (size_t)c->n_glob;
    // slab mode: mph_get fills the owned entries and mph_set writes only those back
    std::vector<double> pos(3 * n, 0.0), vel(3 * n, 0.0);
    MPH_CK(mph_get(c, MPH_FIELD_POSITION, pos.data()));
    MPH_CK(mph_get(c, MPH_FIELD_VELOCITY, vel.data()));
    // the static inputs this context holds, with the current state of the same particles
    const int nin = (int)c->prop.size();
    std::vector<double> p(3 * (size_t)nin), v(3 * (size_t)nin);
    for (int k = 0; k < nin; ++k)
        for (int d = 0; d < 3; ++d) {
            p[3 * (size_t)k + d] = pos[3 * (size_t)glob_id(c, k) + d];
            v[3 * (size_t)k + d] = vel[3 * (size_t)glob_id(c, k) + d];
        }
    MPH_CK(mph_velocity_profile_arrays(&c->cfg, c->time, nin, c->prop.data(), p.data(), c->pos0.data(), v.data()));
    for (int k = 0; k < nin; ++k)
        for (int d = 0; d < 3; ++d) vel[3 * (size_t)glob_id(c, k) + d] = v[3 * (size_t)k + d];
    return mph_set(c, MPH_FIELD_VELOCITY, vel.data());
}

int mph_write_prof(MphCtx* c, const char* path)
{
    if (!c || !path) return MPH_ERR_ARG;
    if (c->dist) return dist_write_output(c, path, kOutProf);   // collective; rank 0 writes
    const int n = c->n_glob;
    std::vector<double> pos(3 * (size_t)n), vel(3 * (size_t)n);
    MPH_CK(mph_get(c, MPH_FIELD_POSITION, pos.data()));
    MPH_CK(mph_get(c, MPH_FIELD_VELOCITY, vel.data()));
    return mph_write_prof_arrays(path, &c->cfg, c->time, n, c->prop.data(), pos.data(), c->pos0.data(),
                                 vel.data());
}

// the per-particle fields of a .vtk / .vtu file, in original order
struct Snap {
    std::vector<double> pos, vel, acc, force, stress, strain;
    std::vector<int> isnc, nc;
};

static int snapshot(MphCtx* c, Snap& s)
{
    const size_t n = (size_t)c->n_glob;
    for (auto* v : {&s.pos, &s.vel, &s.acc, &s.force}) v->resize(3 * n);
    s.stress.resize(9 * n); s.strain.resize(9 * n); s.isnc.resize(n); s.nc.resize(n);
    MPH_CK(mph_get(c, MPH_FIELD_POSITION, s.pos.data()));
    MPH_CK(mph_get(c, MPH_FIELD_VELOCITY, s.vel.data()));
    MPH_CK(mph_get(c, MPH_FIELD_ACCELERATION, s.acc.data()));
    MPH_CK(mph_get(c, MPH_FIELD_FORCE, s.force.data()));
    MPH_CK(mph_get(c, MPH_FIELD_STRESS, s.stress.data()));
    MPH_CK(mph_get(c, MPH_FIELD_STRAIN, s.strain.data()));
    MPH_CK(mph_get(c, MPH_FIELD_INITIAL_STRUCTURE_NEIGHBOR_COUNT, s.isnc.data()));
    return mph_get(c, MPH_FIELD_NEIGHBOR_COUNT, s.nc.data());
}

static int write_vtk_any(MphCtx* c, const char* path, bool xml)
{
    if (!c || !path) return MPH_ERR_ARG;
    if (c->dist) return dist_write_output(c, path, xml ? kOutVtu : kOutVtk);   // collective; rank 0 writes
    Snap s;
    MPH_CK(snapshot(c, s));
    auto writer = xml ? mph_write_vtu_arrays : mph_write_vtk_arrays;
    return writer(path, c->n_glob, c->prop.data(), s.pos.data(), c->pos0.data(), s.vel.data(), s.acc.data(),
                  s.force.data(), s.stress.data(), s.strain.data(), s.isnc.data(), s.nc.data());
}

int mph_write_vtk(MphCtx* c, const char* path) { return write_vtk_any(c, path, false); }

int mph_write_vtu(MphCtx* c, const char* path) { return write_vtk_any(c, path, true); }

int mph_output_wait(MphCtx* c)
{
    if (!c) return MPH_ERR_ARG;
    if (c->out_thread.joinable()) c->out_thread.join();
    const int rc = c->out_rc;
    c->out_rc = MPH_OK;
    if (rc) return ctx_fail(c, rc, "asynchronous .vtk write failed");
    return MPH_OK;
}

int mph_write_vtk_async(MphCtx* c, const char* path)
{
    if (!c || !path) return MPH_ERR_ARG;
    MPH_CK(mph_output_wait(c));   // at most one file in flight
    if (c->dist) return dist_write_output(c, path, kOutVtkAsync);   // collective; rank 0 formats and writes
    auto s = std::make_shared<Snap>();
    MPH_CK(snapshot(c, *s));
    // the thread owns copies of everything it reads
    c->out_thread = std::thread([c, s, nn = c->n_glob, file = std::string(path), prop = c->prop, pos0 = c->pos0] {
        c->out_rc = mph_write_vtk_arrays(file.c_str(), nn, prop.data(), s->pos.data(), pos0.data(), s->vel.data(),
                                         s->acc.data(), s->force.data(), s->stress.data(), s->strain.data(),
                                         s->isnc.data(), s->nc.data());
    });
    return MPH_OK;
}

}  // extern "C"

// ---- particle selections (kernels: mph_select.hip) ----------------------------------------------

namespace {

// a device array of the selection regrown to hold `need` elements (its contents are not kept)
template <typename T>
int sel_grow(MphCtx* c, T** p, size_t* cap, size_t need)
{
    if (need <= *cap && *p) return MPH_OK;
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    ctx_dfree(c, *p);
    *p = nullptr;
    *cap = 0;
    MPH_CK(ctx_dalloc(c, p, need));
    *cap = need;
    return MPH_OK;
}

// the entry of a consumer of the selection: flush, single contexts (slab: slab contexts, the
// mph_dist_* calls), a current selection
int sel_enter(MphCtx* c, const char* who, bool slab = false)
{
    MPH_CK(ctx_enter(c));
    if (slab && !c->dist)
        return ctx_fail(c, MPH_ERR_UNSUPPORTED, std::string(who) + ": slab selections need a slab context (a single context: "
                                                    "mph_select and its readers)");
    if (!slab && c->dist)
        return ctx_fail(c, MPH_ERR_UNSUPPORTED, std::string(who) + ": selections are not available in slab mode");
    if (!c->sel_current)
        return ctx_fail(c, MPH_ERR_ARG, std::string(who) + ": no current selection (none was made, or the state has changed "
                                            "since: mph_select again after mph_step / mph_set)");
    return MPH_OK;
}

// rows of the selection gathered on the device into sel_out and copied to out: nc doubles per row
// from src[e][slot[r] * stride]
int sel_gather(MphCtx* c, const double* const* src, int nc, int stride, const int* slot, double* out)
{
    const size_t cnt = (size_t)c->sel.count;
    if (cnt == 0) return MPH_OK;
    MPH_CK(sel_grow(c, &c->sel_out, &c->sel_out_cap, cnt * nc));
    launch_select_gather(c->L, src, nc, stride, slot, (int)cnt, c->sel_out);
    MPH_HIP_OK(c, hipGetLastError());
    MPH_HIP_OK(c, hipMemcpyAsync(out, c->sel_out, sizeof(double) * cnt * nc, hipMemcpyDeviceToHost, c->stream));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    return MPH_OK;
}

// the selected row of original index i, or -1
long sel_row(const MphCtx* c, int i)
{
    const auto it = std::lower_bound(c->sel_ids.begin(), c->sel_ids.end(), i);
    return it != c->sel_ids.end() && *it == i ? (long)(it - c->sel_ids.begin()) : -1;
}

// DeformGradient / Strain / Stress: the element planes fetched whole, as download_struct_m33 does
// (the structure is a small part of a case), and the selected slots' rows picked on the host
int sel_struct_m33(MphCtx* c, const double* d, double* out)
{
    const int ns = c->Sd.n_own;
    std::memset(out, 0, sizeof(double) * 9 * c->sel_ids.size());
    if (ns == 0 || c->sel_ids.empty()) return MPH_OK;
    const size_t fes = (size_t)c->Sd.fes;
    std::vector<double> h(fes * 9);
    MPH_HIP_OK(c, hipMemcpyAsync(h.data(), d, sizeof(double) * 9 * fes, hipMemcpyDeviceToHost, c->stream));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    for (int s = 0; s < ns; ++s) {
        const long r = sel_row(c, c->sl_orig[s]);
        if (r < 0) continue;
        for (int e = 0; e < 9; ++e) out[9 * (size_t)r + e] = h[e * fes + s];
    }
    return MPH_OK;
}

// What follows the flags of mph_select and mph_dist_select: the count of the scan over nidx original
// indices, the rank arrays regrown for it, the fill (fill(): its launch) and the host copy of the ids
template <typename Fill>
int sel_collect(MphCtx* c, int nidx, const char* who, Fill fill)
{
    SelectDev& D = c->sel;
    int cnt = 0;
    MPH_HIP_OK(c, hipMemcpyAsync(&cnt, D.bsum + select_blocks(nidx), sizeof(int), hipMemcpyDeviceToHost, c->stream));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    if (cnt < 0 || cnt > nidx) return ctx_fail(c, MPH_ERR_HIP, std::string(who) + ": the scan returned " + std::to_string(cnt));
    if ((size_t)cnt > c->sel_rank_cap || !D.ids) {
        size_t cap = 0;
        for (int** p : {&D.ids, &D.slot_a, &D.slot_b}) {
            cap = 0;
            MPH_CK(sel_grow(c, p, &cap, (size_t)std::max(cnt, 1)));
        }
        c->sel_rank_cap = cap;
    }
    D.count = cnt;
    if (cnt > 0) {
        fill();
        MPH_HIP_OK(c, hipGetLastError());
        MPH_CK(fetch(c, (const int*)D.ids, c->sel_ids, (size_t)cnt));
        MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    }
    return MPH_OK;
}

// host index of the static inputs of original index i (prop, pos0), or -1: this rank was created
// without them (slab-local creation, a particle from outside its window)
long sel_input(const MphCtx* c, int i)
{
    if (c->gid.empty()) return i;
    const auto it = std::lower_bound(c->gid.begin(), c->gid.end(), i);
    return it != c->gid.end() && *it == i ? (long)(it - c->gid.begin()) : -1;
}

// mph_get_selected and mph_dist_get_selected behind their entries.  What mph_get takes from the host's
// static inputs comes, on a slab rank, from where every owned particle has it: Property is the device's
// type (gathered through slot_b), and Mass, Lambda, Mu and Kappa's modulus follow from it through the
// per-type tables -- a rank created from its window alone (slab-local creation) has no inputs for a
// particle that came from outside it.  InitialPosition has no such source.
int sel_get(MphCtx* c, int field, void* out)
{
    const std::vector<int>& ids = c->sel_ids;
    const size_t m = ids.size();
    if (field < 0 || field >= MPH_FIELD_COUNT) return ctx_fail(c, MPH_ERR_ARG, "unknown field " + std::to_string(field));
    if (m == 0) return MPH_OK;
    if (!out) return MPH_ERR_ARG;
    double* o = (double*)out;
    int* oi = (int*)out;
    const Launch& L = c->L;
    const SelectDev& D = c->sel;
    // the sorted arrays through the slot maps, as mph_get reads them: Position and Velocity from
    // the set B in B.id order, everything else in A.id order
    auto planes = [&](const double* x, const double* y, const double* z, const int* slot) {
        const double* const src[3] = {x, y, z};
        return sel_gather(c, src, 3, 1, slot, o);
    };
    auto xyz4 = [&](const double4* d) {
        const double* b = (const double*)d;
        const double* const src[3] = {b, b + 1, b + 2};
        return sel_gather(c, src, 3, 4, D.slot_a, o);
    };
    auto scalar = [&](const double* d, double* to) {
        const double* const src[1] = {d};
        return sel_gather(c, src, 1, 1, D.slot_a, to);
    };
    // the structure's host tables: row k of S belongs to original index S.orig[k] (slab mode: of the
    // lists built here, sl_s, as mph_get; a ghost slot's particle is never selected)
    auto struct_rows = [&](auto put) {
        const size_t ns = c->dist ? c->sl_s.size() : c->S.orig.size();
        for (size_t j = 0; j < ns; ++j) {
            const size_t k = c->dist ? (size_t)c->sl_s[j] : j;
            const long r = sel_row(c, glob_id(c, c->S.orig[k]));
            if (r >= 0) put((size_t)r, k);
        }
    };
    // the selected particles' types
    std::vector<int> ty;
    auto types = [&]() {
        ty.resize(m);
        if (!c->dist) {
            for (size_t r = 0; r < m; ++r) ty[r] = c->prop[ids[r]];
            return (int)MPH_OK;
        }
        MPH_CK(sel_grow(c, &c->sel_out, &c->sel_out_cap, m));
        launch_select_gather_int(L, L.B.type, D.slot_b, (int)m, (int*)c->sel_out);
        MPH_HIP_OK(c, hipGetLastError());
        MPH_HIP_OK(c, hipMemcpyAsync(ty.data(), c->sel_out, sizeof(int) * m, hipMemcpyDeviceToHost, c->stream));
        MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
        for (size_t r = 0; r < m; ++r)
            if (ty[r] < 0 || ty[r] >= kTypes) return ctx_fail(c, MPH_ERR_HIP, "selection: a particle of type " + std::to_string(ty[r]));
        return (int)MPH_OK;
    };
    switch (field) {
    case MPH_FIELD_POSITION: return planes(L.B.x, L.B.y, L.B.z, D.slot_b);
    case MPH_FIELD_VELOCITY: return planes(L.B.vx, L.B.vy, L.B.vz, D.slot_b);
    case MPH_FIELD_INITIAL_POSITION:
        for (size_t r = 0; r < m; ++r)
            if (sel_input(c, ids[r]) < 0)
                return ctx_fail(c, MPH_ERR_ARG, "slab selection: an owned particle without static inputs");
        for (size_t r = 0; r < m; ++r) std::memcpy(o + 3 * r, &c->pos0[3 * (size_t)sel_input(c, ids[r])], 3 * sizeof(double));
        return MPH_OK;
    case MPH_FIELD_FORCE: return xyz4(L.force);
    case MPH_FIELD_ACCELERATION: return xyz4(L.acc);
    case MPH_FIELD_GRAVITY_CENTER: return planes(L.gx, L.gy, L.gz, D.slot_a);
    case MPH_FIELD_PRESSURE_P: return scalar(L.pres, o);
    case MPH_FIELD_PRESSURE_A: return scalar(L.pa, o);
    case MPH_FIELD_DENSITY_A: return scalar(L.dens_a, o);
    case MPH_FIELD_VOL_STRAIN_P: return scalar(L.vstrain, o);
    case MPH_FIELD_DIVERGENCE_P: return scalar(L.divp, o);
    case MPH_FIELD_NEIGHBOR_COUNT:
        MPH_CK(sel_grow(c, &c->sel_out, &c->sel_out_cap, m));
        launch_select_gather_int(L, L.nbcount, D.slot_a, (int)m, (int*)c->sel_out);
        MPH_HIP_OK(c, hipGetLastError());
        MPH_HIP_OK(c, hipMemcpyAsync(oi, c->sel_out, sizeof(int) * m, hipMemcpyDeviceToHost, c->stream));
        MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
        return MPH_OK;
    case MPH_FIELD_MASS:
        MPH_CK(types());
        for (size_t r = 0; r < m; ++r) o[r] = c->cfg.density[ty[r]] * c->h.vol;
        return MPH_OK;
    case MPH_FIELD_KAPPA: {
        std::vector<double> vs(c->stepped ? m : 0, 0.0);
        if (c->stepped) MPH_CK(scalar(L.vstrain, vs.data()));
        MPH_CK(types());
        for (size_t r = 0; r < m; ++r) o[r] = (c->stepped && vs[r] < 0.0) ? 0.0 : c->cfg.bulk_modulus[ty[r]];
        return MPH_OK;
    }
    case MPH_FIELD_LAMBDA:
        MPH_CK(types());
        for (size_t r = 0; r < m; ++r) o[r] = c->cfg.bulk_viscosity[ty[r]];
        return MPH_OK;
    case MPH_FIELD_MU:
        MPH_CK(types());
        for (size_t r = 0; r < m; ++r) o[r] = c->cfg.shear_viscosity[ty[r]];
        return MPH_OK;
    case MPH_FIELD_PROPERTY:
        MPH_CK(types());
        std::memcpy(oi, ty.data(), sizeof(int) * m);
        return MPH_OK;
    case MPH_FIELD_INITIAL_STRUCTURE_NEIGHBOR_COUNT:
        std::memset(oi, 0, sizeof(int) * m);
        struct_rows([&](size_t r, size_t k) { oi[r] = c->S.count[k]; });
        return MPH_OK;
    case MPH_FIELD_DEFORM_GRADIENT: return sel_struct_m33(c, c->Sd.F, o);
    case MPH_FIELD_STRAIN: return sel_struct_m33(c, c->Sd.E, o);
    case MPH_FIELD_STRESS: return sel_struct_m33(c, c->Sd.S, o);
    case MPH_FIELD_NORMALIZER:
        std::memset(o, 0, sizeof(double) * 9 * m);
        struct_rows([&](size_t r, size_t k) { std::memcpy(o + 9 * r, &c->S.normalizer[9 * k], sizeof(double) * 9); });
        return MPH_OK;
    case MPH_FIELD_VIRIAL_STRESS:
    case MPH_FIELD_VIRIAL_PRESSURE: {
        const int w = field == MPH_FIELD_VIRIAL_STRESS ? 9 : 1;
        std::memset(o, 0, sizeof(double) * w * m);
        if (!c->vir) return MPH_OK;   // never computed: zeros, as mph_get
        const double* src[9];
        for (int e = 0; e < w; ++e) src[e] = (w == 9 ? c->vir : c->vpres) + e;
        return sel_gather(c, src, w, w, D.slot_a, o);
    }
    case MPH_FIELD_LAMBDA_LAMES:
    case MPH_FIELD_MU_LAMES:
        for (size_t r = 0; r < m; ++r) o[r] = 0.0;
        struct_rows([&](size_t r, size_t k) { o[r] = field == MPH_FIELD_LAMBDA_LAMES ? c->S.lame_l[k] : c->S.lame_m[k]; });
        return MPH_OK;
    default: return ctx_fail(c, MPH_ERR_ARG, "unknown field " + std::to_string(field));
    }
}

int write_selected(MphCtx* c, const char* path, bool xml)
{
    if (!c || !path) return MPH_ERR_ARG;
    MPH_CK(sel_enter(c, xml ? "mph_write_vtu_selected" : "mph_write_vtk_selected"));
    const size_t m = c->sel_ids.size(), m1 = std::max<size_t>(m, 1);
    Snap s;
    for (auto* v : {&s.pos, &s.vel, &s.acc, &s.force}) v->resize(3 * m1);
    s.stress.resize(9 * m1); s.strain.resize(9 * m1); s.isnc.resize(m1); s.nc.resize(m1);
    std::vector<int> prop(m1);
    std::vector<double> pos0(3 * m1);
    MPH_CK(mph_get_selected(c, MPH_FIELD_POSITION, s.pos.data()));
    MPH_CK(mph_get_selected(c, MPH_FIELD_VELOCITY, s.vel.data()));
    MPH_CK(mph_get_selected(c, MPH_FIELD_ACCELERATION, s.acc.data()));
    MPH_CK(mph_get_selected(c, MPH_FIELD_FORCE, s.force.data()));
    MPH_CK(mph_get_selected(c, MPH_FIELD_STRESS, s.stress.data()));
    MPH_CK(mph_get_selected(c, MPH_FIELD_STRAIN, s.strain.data()));
    MPH_CK(mph_get_selected(c, MPH_FIELD_INITIAL_STRUCTURE_NEIGHBOR_COUNT, s.isnc.data()));
    MPH_CK(mph_get_selected(c, MPH_FIELD_NEIGHBOR_COUNT, s.nc.data()));
    MPH_CK(mph_get_selected(c, MPH_FIELD_PROPERTY, prop.data()));
    MPH_CK(mph_get_selected(c, MPH_FIELD_INITIAL_POSITION, pos0.data()));
    auto writer = xml ? mph_write_vtu_arrays : mph_write_vtk_arrays;
    return writer(path, (int)m, prop.data(), s.pos.data(), pos0.data(), s.vel.data(), s.acc.data(), s.force.data(),
                  s.stress.data(), s.strain.data(), s.isnc.data(), s.nc.data());
}

}  // namespace

extern "C" {

int mph_select(MphCtx* c, const MphSelection* s, int* count)
{
    if (!s) return MPH_ERR_ARG;
    MPH_CK(ctx_enter(c));
    if (c->dist) return ctx_fail(c, MPH_ERR_UNSUPPORTED, "mph_select: selections are not available in slab mode");
    if (!sel_valid(*s, c->cfg.dim))
        return ctx_fail(c, MPH_ERR_ARG, "mph_select: every must be >= 1, phase in [0, every), box in 0..2, type_mask within "
                                        "0x3f and lo <= hi on every axis of a box");
    SelectDev& D = c->sel;
    c->sel_current = false;
    c->sel_ids.clear();
    D.count = 0;
    const int n = c->n;
    if (n > 0) {
        const int nb = select_blocks(n);
        if (!D.flag) {   // once: these are sized by the particle count
            MPH_CK(ctx_dalloc(c, &D.flag, (size_t)n));
            MPH_CK(ctx_dalloc(c, &D.slot_a_of, (size_t)n));
            MPH_CK(ctx_dalloc(c, &D.slot_b_of, (size_t)n));
            MPH_CK(ctx_dalloc(c, &D.mask, ((size_t)n + 31) / 32));
            MPH_CK(ctx_dalloc(c, &D.bsum, (size_t)nb + 1));
        }
        // a box on InitialPosition: that array lives on the host (only the structure's is on the
        // device), so the host decides with the shared predicate and uploads one bit per particle
        const bool with_mask = s->box == 2;
        std::vector<unsigned> mask;
        if (with_mask) {
            mask.assign(((size_t)n + 31) / 32, 0u);
            for (int i = 0; i < n; ++i)
                if (sel_accepts(*s, c->cfg.dim, i, c->prop[i], &c->pos0[3 * (size_t)i])) mask[i >> 5] |= 1u << (i & 31);
            MPH_HIP_OK(c, hipMemcpyAsync(D.mask, mask.data(), sizeof(unsigned) * mask.size(), hipMemcpyHostToDevice, c->stream));
        }
        // Position as mph_get reads it: the integrated set B in the order of B.id
        launch_select_scan(c->L, c->L.B, *s, with_mask, D);
        MPH_HIP_OK(c, hipGetLastError());
        MPH_CK(sel_collect(c, n, "mph_select", [&] { launch_select_fill(c->L, D); }));
    }
    c->sel_current = true;
    if (count) *count = D.count;
    return MPH_OK;
}

int mph_selected_ids(MphCtx* c, int* out)
{
    MPH_CK(sel_enter(c, "mph_selected_ids"));
    if (!out && !c->sel_ids.empty()) return MPH_ERR_ARG;
    if (!c->sel_ids.empty()) std::memcpy(out, c->sel_ids.data(), sizeof(int) * c->sel_ids.size());
    return MPH_OK;
}

int mph_get_selected(MphCtx* c, int field, void* out)
{
    MPH_CK(sel_enter(c, "mph_get_selected"));
    return sel_get(c, field, out);
}

int mph_selection_totals(MphCtx* c, const double center[3], double out[MPH_TOTALS])
{
    if (!center || !out) return MPH_ERR_ARG;
    MPH_CK(sel_enter(c, "mph_selection_totals"));
    if (c->n == 0) {   // (no device arrays)
        for (int k = 0; k < MPH_TOTALS; ++k)
            out[k] = k >= MPH_TOT_XMIN && k <= MPH_TOT_ZMAX ? ((k - MPH_TOT_XMIN) % 2 ? -INFINITY : INFINITY) : 0.0;
        return MPH_OK;
    }
    const size_t nb = (size_t)select_total_blocks(c->sel.count);
    MPH_CK(sel_grow(c, &c->sel_out, &c->sel_out_cap, (size_t)kSelTotals * (nb + 1)));
    launch_select_totals(c->L, c->L.B, c->sel, center, c->sel_out + kSelTotals, c->sel_out);
    MPH_HIP_OK(c, hipGetLastError());
    MPH_HIP_OK(c, hipMemcpyAsync(out, c->sel_out, sizeof(double) * kSelTotals, hipMemcpyDeviceToHost, c->stream));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    return MPH_OK;
}

int mph_select_profile(MphCtx* c, const MphSelection* s, const double center[3], int max, double* ms, char* names32)
{
    if (!s || !center || max < 0 || (max > 0 && (!ms || !names32))) return MPH_ERR_ARG;
    MPH_CK(ctx_enter(c));
    EventProfiler prof;
    c->L.prof = &prof;
    int rc = mph_select(c, s, nullptr);
    std::vector<double> buf(3 * std::max<size_t>(c->sel_ids.size(), 1));
    double tot[MPH_TOTALS];
    for (int f : {MPH_FIELD_POSITION, MPH_FIELD_VELOCITY, MPH_FIELD_PRESSURE_P})
        if (rc == MPH_OK) rc = mph_get_selected(c, f, buf.data());
    if (rc == MPH_OK) rc = mph_selection_totals(c, center, tot);
    c->L.prof = nullptr;
    MPH_CK(rc);
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    const int k = (int)prof.recs.size();
    for (int i = 0; i < std::min(k, max); ++i) {
        float t = 0.0f;
        MPH_HIP_OK(c, hipEventElapsedTime(&t, prof.recs[i].a, prof.recs[i].b));
        ms[i] = t;
        std::snprintf(names32 + 32 * (size_t)i, 32, "%s", prof.recs[i].name.c_str());
    }
    return k;
}

int mph_write_vtk_selected(MphCtx* c, const char* path) { return write_selected(c, path, false); }

int mph_write_vtu_selected(MphCtx* c, const char* path) { return write_selected(c, path, true); }

// ---- selections on slab ranks: the calls without communication (collective ones: mph_dist_select.hip)

int mph_dist_select(MphCtx* c, const MphSelection* s, int* count)
{
    if (!s) return MPH_ERR_ARG;
    MPH_CK(ctx_enter(c));
    if (!c->dist)
        return ctx_fail(c, MPH_ERR_UNSUPPORTED, "mph_dist_select: slab selections need a slab context (a single context: mph_select)");
    if (!sel_valid(*s, c->cfg.dim))
        return ctx_fail(c, MPH_ERR_ARG, "mph_dist_select: every must be >= 1, phase in [0, every), box in 0..2, type_mask "
                                        "within 0x3f and lo <= hi on every axis of a box");
    // the flush has left the held count and the owned count current (dist_sync)
    const int n = c->n, ng = c->n_glob, nb = select_blocks(ng);
    const size_t words = ((size_t)ng + 31) / 32;
    // a box on InitialPosition: the host's verdict over the particles this rank has static inputs
    // for, by original index.  Created from its window alone, the rank may own a particle without
    // them; one the rest of the selection accepts cannot be decided, and the call is refused before
    // anything of the earlier selection is touched.
    const bool with_mask = s->box == 2;
    std::vector<unsigned> mask;
    if (with_mask) {
        if (!c->gid.empty()) {
            std::vector<int> id, ty;
            MPH_CK(fetch(c, (const int*)c->L.B.id, id, (size_t)n));
            MPH_CK(fetch(c, (const int*)c->L.B.type, ty, (size_t)n));
            MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
            MphSelection rest = *s;
            rest.box = 0;
            for (int q = 0; q < n; ++q)
                if (id[q] >= 0 && sel_input(c, id[q]) < 0 && sel_accepts(rest, c->cfg.dim, id[q], ty[q], nullptr))
                    return ctx_fail(c, MPH_ERR_ARG, "mph_dist_select: a box on InitialPosition and an owned particle without "
                                                    "static inputs");
        }
        mask.assign(words, 0u);
        for (size_t k = 0; k < c->prop.size(); ++k) {
            const int i = glob_id(c, (int)k);
            if (sel_accepts(*s, c->cfg.dim, i, c->prop[k], &c->pos0[3 * k])) mask[i >> 5] |= 1u << (i & 31);
        }
    }
    SelectDev& D = c->sel;
    if (!D.flag) {   // once: these are sized by the whole problem's particle count
        const size_t n4 = 4 * (((size_t)ng + 3) / 4);   // (k_sel_clear stores int4)
        MPH_CK(ctx_dalloc(c, &D.flag, n4));
        MPH_CK(ctx_dalloc(c, &D.slot_a_of, (size_t)ng));
        MPH_CK(ctx_dalloc(c, &D.slot_b_of, (size_t)ng));
        MPH_CK(ctx_dalloc(c, &D.mask, words));
        MPH_CK(ctx_dalloc(c, &D.bsum, (size_t)nb + 1));
        // an index this rank has never held maps to slot 0 (never read: its flag is 0)
        MPH_HIP_OK(c, hipMemsetAsync(D.slot_a_of, 0, sizeof(int) * (size_t)ng, c->stream));
        MPH_HIP_OK(c, hipMemsetAsync(D.slot_b_of, 0, sizeof(int) * (size_t)ng, c->stream));
    }
    c->sel_current = false;
    c->sel_ids.clear();
    D.count = 0;
    if (with_mask)
        MPH_HIP_OK(c, hipMemcpyAsync(D.mask, mask.data(), sizeof(unsigned) * words, hipMemcpyHostToDevice, c->stream));
    // Position as mph_get reads it: the integrated set B in the order of B.id, ghosts skipped
    launch_dist_select_scan(c->L, n, ng, c->L.B, *s, with_mask, D);
    MPH_HIP_OK(c, hipGetLastError());
    MPH_CK(sel_collect(c, ng, "mph_dist_select", [&] { launch_dist_select_fill(c->L, ng, D); }));
    c->sel_current = true;
    if (count) *count = D.count;
    return MPH_OK;
}

int mph_dist_selected_ids(MphCtx* c, int* out)
{
    MPH_CK(sel_enter(c, "mph_dist_selected_ids", true));
    if (!out && !c->sel_ids.empty()) return MPH_ERR_ARG;
    if (!c->sel_ids.empty()) std::memcpy(out, c->sel_ids.data(), sizeof(int) * c->sel_ids.size());
    return MPH_OK;
}

int mph_dist_get_selected(MphCtx* c, int field, void* out)
{
    MPH_CK(sel_enter(c, "mph_dist_get_selected", true));
    return sel_get(c, field, out);
}

int mph_dist_selection_totals_partial(MphCtx* c, const double center[3], double out[MPH_TOTALS])
{
    if (!center || !out) return MPH_ERR_ARG;
    MPH_CK(sel_enter(c, "mph_dist_selection_totals_partial", true));
    // (an empty selection: no partial record, and k_sel_totals_final leaves the identities)
    const size_t nb = (size_t)select_total_blocks(c->sel.count);
    MPH_CK(sel_grow(c, &c->sel_out, &c->sel_out_cap, (size_t)kSelTotals * (nb + 1)));
    launch_select_totals(c->L, c->L.B, c->sel, center, c->sel_out + kSelTotals, c->sel_out);
    MPH_HIP_OK(c, hipGetLastError());
    MPH_HIP_OK(c, hipMemcpyAsync(out, c->sel_out, sizeof(double) * kSelTotals, hipMemcpyDeviceToHost, c->stream));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    return MPH_OK;
}

}  // extern "C"

// ---- kinematics (kernels: mph_kinematics.hip) ----------------------------------------------------

namespace {

// the entry of a reader of the kinematics: flush, single contexts, a current snapshot
int kin_enter(MphCtx* c, const char* who)
{
    MPH_CK(ctx_enter(c));
    if (c->dist) return ctx_fail(c, MPH_ERR_UNSUPPORTED, std::string(who) + ": kinematics are not available in slab mode");
    if (!c->kin_current)
        return ctx_fail(c, MPH_ERR_ARG, std::string(who) + ": no current kinematics (none were computed, or the state has "
                                            "changed since: mph_compute_kinematics again after mph_step / mph_set)");
    return MPH_OK;
}

// prof set: the kernel's launch is recorded by it (its events are read by the caller)
int compute_kinematics(MphCtx* c, const MphKinematics* k, Profiler* prof)
{
    if (!k) return MPH_ERR_ARG;
    MPH_CK(ctx_enter(c));
    if (c->dist) return ctx_fail(c, MPH_ERR_UNSUPPORTED, "mph_compute_kinematics: not available in slab mode");
    if (!kin_valid(*k) || k->radius > c->h.max_radius)
        return ctx_fail(c, MPH_ERR_ARG, "mph_compute_kinematics: radius in [0, MaxRadius = " + std::to_string(c->h.max_radius) +
                                            "], surface_beta >= 0, det_floor in [0, 1), classes in 0..7, reserved 0");
    if (c->set_since_step)
        return ctx_fail(c, MPH_ERR_ARG, "mph_compute_kinematics: run a step first (none since the last mph_set: the lists "
                                        "are not that state's)");
    c->kin_current = false;
    double n0 = 0.0;
    MPH_CK(mph_kinematics_n0(&c->cfg, k->radius, &n0));
    const KinDev K = kin_resolve(*k, c->h.rv, n0);
    if (c->n > 0) {
        if (!c->kin) MPH_CK(ctx_dalloc(c, &c->kin, (size_t)MPH_KIN_CHANNELS * c->n));
        // after a step the integrated state B is in A (list) order; before the first step A is current
        MPH_CK(virial_full_lists(c));
        Launch L = c->L;
        L.prof = prof;
        launch_kinematics(L, c->stepped, K, c->kin);
        MPH_HIP_OK(c, hipGetLastError());
        MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    }
    c->kin_current = true;
    return MPH_OK;
}

int write_kinematics(MphCtx* c, const char* path, bool selected)
{
    if (!c || !path) return MPH_ERR_ARG;
    const char* who = selected ? "mph_write_vtu_kinematics_selected" : "mph_write_vtu_kinematics";
    MPH_CK(kin_enter(c, who));
    if (selected) MPH_CK(sel_enter(c, who));
    const size_t m = selected ? c->sel_ids.size() : (size_t)c->n_glob, m1 = std::max<size_t>(m, 1);
    std::vector<double> pos(3 * m1), kin((size_t)MPH_KIN_CHANNELS * m1);
    std::vector<int> prop(m1);
    if (selected) {
        MPH_CK(mph_get_selected(c, MPH_FIELD_POSITION, pos.data()));
        MPH_CK(mph_get_selected(c, MPH_FIELD_PROPERTY, prop.data()));
        MPH_CK(mph_get_kinematics_selected(c, kin.data()));
    } else {
        MPH_CK(mph_get(c, MPH_FIELD_POSITION, pos.data()));
        MPH_CK(mph_get(c, MPH_FIELD_PROPERTY, prop.data()));
        MPH_CK(mph_get_kinematics(c, kin.data()));
    }
    const int rc = mph_write_vtu_kinematics_arrays(path, (int)m, prop.data(), pos.data(), kin.data());
    if (rc) return ctx_fail(c, rc, std::string(who) + ": writing " + path);
    return MPH_OK;
}

}  // namespace

extern "C" {

int mph_compute_kinematics(MphCtx* c, const MphKinematics* k) { return compute_kinematics(c, k, nullptr); }

int mph_compute_kinematics_timed(MphCtx* c, const MphKinematics* k, double* kernel_ms, char* name32)
{
    EventProfiler prof;
    if (kernel_ms) *kernel_ms = 0.0;
    if (name32) name32[0] = 0;
    MPH_CK(compute_kinematics(c, k, &prof));
    if (prof.recs.empty()) return MPH_OK;
    float ms = 0.0f;
    MPH_HIP_OK(c, hipEventElapsedTime(&ms, prof.recs[0].a, prof.recs[0].b));
    if (kernel_ms) *kernel_ms = ms;
    if (name32) std::snprintf(name32, 32, "%s", prof.recs[0].name.c_str());
    return MPH_OK;
}

int mph_get_kinematics(MphCtx* c, double* out)
{
    MPH_CK(kin_enter(c, "mph_get_kinematics"));
    if (c->n == 0) return MPH_OK;
    if (!out) return MPH_ERR_ARG;
    constexpr size_t w = MPH_KIN_CHANNELS;
    double* const src[1] = {c->kin};
    return download(c, src, w * (size_t)c->n, c->L.A.id, [out](auto* h, size_t i, size_t id) {
        std::memcpy(out + w * id, &h[0][w * i], sizeof(double) * w);
    });
}

int mph_get_kinematics_selected(MphCtx* c, double* out)
{
    MPH_CK(kin_enter(c, "mph_get_kinematics_selected"));
    MPH_CK(sel_enter(c, "mph_get_kinematics_selected"));
    const size_t cnt = (size_t)c->sel.count;
    if (cnt == 0) return MPH_OK;
    if (!out) return MPH_ERR_ARG;
    MPH_CK(sel_grow(c, &c->sel_out, &c->sel_out_cap, cnt * MPH_KIN_CHANNELS));
    launch_kin_gather(c->L, c->kin, c->sel.slot_a, (int)cnt, c->sel_out);
    MPH_HIP_OK(c, hipGetLastError());
    MPH_HIP_OK(c, hipMemcpyAsync(out, c->sel_out, sizeof(double) * cnt * MPH_KIN_CHANNELS, hipMemcpyDeviceToHost, c->stream));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    return MPH_OK;
}

int mph_write_vtu_kinematics(MphCtx* c, const char* path) { return write_kinematics(c, path, false); }

int mph_write_vtu_kinematics_selected(MphCtx* c, const char* path) { return write_kinematics(c, path, true); }

}  // extern "C"
