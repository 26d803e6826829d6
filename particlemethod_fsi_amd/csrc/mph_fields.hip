// mph_fields.hip -- the fields of a context: download in the reference's AoS layout and original
// particle order (mph_get), upload (mph_set), the virial diagnostic, and the file writers.
#include <hip/hip_runtime.h>

#include <algorithm>
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
