// mph_create.hip -- creation of a device context in phases (ctx_init): the shared body of mph_create
// (dist == nullptr) and of the slab-mode constructors of mph_slab_geom.hip (dist != nullptr: only this
// rank's particles are uploaded, the cell grid covers its window).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "mph_dist.h"
#include "mph_env.h"

using namespace mph;

namespace mph {

static thread_local std::string g_create_error;   // mph_last_error(NULL) after a failed create

// The arguments of a create, and what one phase of ctx_init hands to the later ones.
struct CreateArgs {
    const MphConfig* cfg;
    int n;
    const int* property;
    const double *pos, *pos0, *vel;
    int device;
    const int* ids;
    int n_glob;
    bool gpu_init = false;     // the fixed elastic lists are built on the device (init_host_state)
    std::vector<int> owned;    // slab mode: the inputs this rank owns (init_capacity)
    int cap = 0;               // capacity of every per-particle array (init_capacity)
};

template <typename T, typename V>
static hipError_t upload(MphCtx* c, T* d, const V& v)
{
    return hipMemcpyAsync(d, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice, c->stream);
}

static int init_check_args(MphCtx* c, const CreateArgs& a)
{
    if (a.cfg->dim != 2 && a.cfg->dim != 3) return MPH_ERR_ARG;
    if (a.cfg->module < 0 || a.cfg->module > MPH_MODULE_NONE) return MPH_ERR_ARG;
    if (!(a.cfg->particle_spacing > 0.0) || !(a.cfg->dt > 0.0) || !(a.cfg->elastic_dt > 0.0)) return MPH_ERR_ARG;
    for (int i = 0; i < a.n; ++i)
        if (a.property[i] < 0 || a.property[i] >= kTypes) return MPH_ERR_ARG;
    c->cfg = *a.cfg;
    c->n = a.n;
    c->n_glob = a.n;
    if (a.ids) {
        if (!c->dist || a.n_glob < a.n) return MPH_ERR_ARG;
        for (int i = 0; i < a.n; ++i)
            if (a.ids[i] < 0 || a.ids[i] >= a.n_glob || (i > 0 && a.ids[i] <= a.ids[i - 1]))
                return ctx_fail(c, MPH_ERR_ARG, "slab-local creation: ids must be ascending original indices below n_glob");
        c->gid.assign(a.ids, a.ids + a.n);
        c->n_glob = a.n_glob;
    }
    c->device = a.device;
    c->time = a.cfg->time;
    return MPH_OK;
}

// device and stream, derived constants, host copies of the static inputs, the elastic lists' host
// part and the kernels' parameters
static int init_host_state(MphCtx* c, CreateArgs& a)
{
    MPH_HIP_OK(c, hipSetDevice(a.device));
    MPH_HIP_OK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    derive_constants(c->cfg, c->h);
    c->prop.assign(a.property, a.property + a.n);
    c->pos0.assign(a.pos0, a.pos0 + 3 * (size_t)a.n);
    std::string err;
    // the fixed Lagrangian structure lists: on the device for a single context (calculate-
    // InitialNeighbor + calculateNormalizer as kernels, launch_struct_init); in slab mode on the
    // host over the particles this rank was given, which also routes the static ghost slots
    // (dist_struct_setup).  MPH_STRUCT_INIT=host selects the host build everywhere.
    a.gpu_init = !c->dist && !env_is("MPH_STRUCT_INIT", "host");
    MPH_CK(ctx_fail(c, build_structure(c->cfg, c->h, a.n, a.property, a.pos0, c->S, err, !a.gpu_init), err));
    make_dev_params(c->cfg, c->h, a.n, (int)c->S.orig.size(), c->P);
    return MPH_OK;
}

// the cell grid (order, cell counts, origin) and the interior boxes of the fast minimum image
static int init_grid(MphCtx* c, const CreateArgs& a)
{
    const double rc = std::sqrt(c->P.rc2);
    std::string err;
    {
        // z slabs of a 3-D problem: z in the middle of the cell order, so the ghosts beyond both
        // faces are long runs (whole wavefronts) at the ends of every plane (DevParams.perm;
        // MPH_SLAB_PERM=0 keeps (x, y, z); =1..4 force an order on any 3-D context, =force
        // orders a single 3-D context the z-slab way -- A/B timing and the parity tests)
        const std::string pv = env_str("MPH_SLAB_PERM");
        const bool zslab = a.cfg->dim == 3 && c->dist && c->dist->g.axis == 2;
        const bool forced = pv.size() == 1 && pv[0] >= '1' && pv[0] <= '4';
        c->P.perm = 0;
        if (a.cfg->dim == 3 && (forced || pv == "force" || (zslab && pv != "0")))
            c->P.perm = forced ? pv[0] - '0' : choose_cell_order(c->h, a.n, a.pos, rc);
        int r = choose_grid(c->h, a.cfg->dim, rc, kContigReach, c->P.gc, c->P.ginv, err, c->P.perm);
        if (r != MPH_OK) return ctx_fail(c, r, err);
        set_uniforms(c->P);
    }
    // interior box for the wave-uniform fast minimum image (k_neighbors / passes): >= 3 cells
    // (+1e-9 relative margin) from every periodic face; needs > 12 cells on every active axis
    // (stencil half-width + 1 cells from every periodic face; the candidate offsets then stay
    // below a quarter of the domain width, which needs > 4 x that many cells on every axis)
    c->P.sa = kContigReach;
    c->P.fast_ok = 1;
    c->P.seam_always = 0;
    // the grid's origin in an empty band of the initial particles (choose_grid_origin;
    // MPH_GRID_SHIFT=0 keeps dmin): the search's interior box is then in grid offsets
    const bool shift = env_str("MPH_GRID_SHIFT")[0] != '0';
    for (int d = 0; d < 3; ++d) {
        if (d == 2 && a.cfg->dim == 2) {
            c->P.inner_lo[d] = c->P.sinner_lo[d] = -1e300;
            c->P.inner_hi[d] = c->P.sinner_hi[d] = 1e300;
            continue;
        }
        const int m = stencil_margin(c->P, d);
        if (c->P.gc[d] <= 4 * m) c->P.fast_ok = 0;
        const double cw = c->h.dw[d] / c->P.gc[d];
        c->P.inner_lo[d] = c->h.dmin[d] + m * cw * (1.0 + 1e-9);
        c->P.inner_hi[d] = c->h.dmax[d] - m * cw * (1.0 + 1e-9);
        const int s0 = shift && c->P.fast_ok ? choose_grid_origin(c->h, a.n, a.pos, d, c->P.gc[d], m) : 0;
        c->P.corg[d] = c->h.dmin[d] + s0 * cw;
        c->P.sinner_lo[d] = m * cw * (1.0 + 1e-9);
        c->P.sinner_hi[d] = c->h.dw[d] - m * cw * (1.0 + 1e-9);
    }
    return MPH_OK;
}

static int init_capacity(MphCtx* c, CreateArgs& a)
{
    // slab mode: owned subset, local window grid along the slab axis, array capacity
    a.cap = a.n;
    if (c->dist) {
        MPH_CK(dist_setup(c, a.pos, a.owned));
        a.cap = c->dist->cap;
        c->n = (int)a.owned.size();
        c->P.n = c->n;
    }
    if (a.cap > kIndexMask)
        return ctx_fail(c, MPH_ERR_UNSUPPORTED, "more than 2^28 particles in one context (neighbour-list entries "
                                            "carry the type in their top bits)");
    if ((long long)a.cap * 48 >= (long long)kGatherOob)
        return ctx_fail(c, MPH_ERR_UNSUPPORTED, "more than 89 million particles in one context (the list passes "
                                            "gather with 32-bit byte offsets)");
    {
        // the search addresses the cell table with 32-bit byte offsets (buffer descriptors)
        const long long nc = (long long)c->P.gc[0] * c->P.gc[1] * c->P.gc[2];
        if (nc + 1 > (1LL << 30))
            return ctx_fail(c, MPH_ERR_UNSUPPORTED, "cell grid of " + std::to_string(nc) +
                                                    " cells: more than 2^30 (4 GiB of cell starts)");
        c->P.ncell = (int)nc;
    }
    return MPH_OK;
}

// the per-type tables, every array of c->L, and the initial DevState
static int init_alloc(MphCtx* c, const CreateArgs& a)
{
    DevTables& T = c->tables;
    for (int t = 0; t < kTypes; ++t) {
        for (int u = 0; u < kTypes; ++u) {
            T.ratio[t * kTypes + u] = c->P.ratio[t][u];
            T.mu_ij[t * kTypes + u] = c->P.mu_ij[t][u];
        }
        T.cofa[t] = c->P.cofa[t];
        T.mass[t] = c->P.mass[t];
        T.inv_mass[t] = c->P.inv_mass[t];
        T.bulk[t] = c->P.bulk[t];
        T.bulk_visc[t] = c->P.bulk_visc[t];
    }
    // device allocations (capacity `cap` per particle array)
    const int cap = a.cap;
    const size_t ntile = ((size_t)cap + kTile - 1) / kTile;
    DevTables* dT = nullptr;
    MPH_CK(ctx_dalloc(c, &dT, 1));
    c->L.T = dT;
    MPH_CK(ctx_dalloc(c, &c->L.st, 1));
    for (Soa* s : {&c->L.A, &c->L.B}) {
        const size_t m = (size_t)cap + kPad;
        MPH_CK(ctx_dalloc(c, &s->x, m)); MPH_CK(ctx_dalloc(c, &s->y, m)); MPH_CK(ctx_dalloc(c, &s->z, m));
        MPH_CK(ctx_dalloc(c, &s->vx, m)); MPH_CK(ctx_dalloc(c, &s->vy, m)); MPH_CK(ctx_dalloc(c, &s->vz, m));
        MPH_CK(ctx_dalloc(c, &s->type, m)); MPH_CK(ctx_dalloc(c, &s->id, m));
    }
    MPH_CK(ctx_dalloc(c, &c->L.A.p6, 3 * (size_t)cap));
    // the search's FP32 candidate records (kPad past the last)
    MPH_CK(ctx_dalloc(c, &c->L.A.f4, (size_t)cap + kPad));
    MPH_CK(ctx_dalloc(c, &c->order, cap));
    MPH_CK(ctx_dalloc(c, &c->L.key, cap)); MPH_CK(ctx_dalloc(c, &c->L.slot, cap));
    MPH_CK(ctx_dalloc(c, &c->L.tmp, cap));
    MPH_CK(ctx_dalloc(c, &c->L.cnt, c->P.ncell)); MPH_CK(ctx_dalloc(c, &c->L.start, (size_t)c->P.ncell + 1));
    // the cell scan's block totals (k_scan_reduce; structure init)
    const size_t bs = (size_t)c->P.ncell / 4096 + 2;   // bsum_stride (mph_sort.hip)
    MPH_CK(ctx_dalloc(c, &c->L.bsum, bs));
    MPH_CK(ctx_dalloc(c, &c->L.nbr, ntile * kTileStride)); MPH_CK(ctx_dalloc(c, &c->L.ncount, cap));
    MPH_CK(ctx_dalloc(c, &c->L.nbcount, cap));
    // the lists' row jumps: a header word per wave, a word of gap starts per lane (whole tiles)
    MPH_CK(ctx_dalloc(c, &c->L.lhdr, ntile)); MPH_CK(ctx_dalloc(c, &c->L.lgap, ntile * kTile));
    MPH_CK(ctx_dalloc(c, &c->L.lbase, ntile * kBaseInts));
    for (double** p : {&c->L.pres, &c->L.gx, &c->L.gy, &c->L.gz, &c->L.pa}) MPH_CK(ctx_dalloc(c, p, cap));
    for (double4** p : {&c->L.force, &c->L.acc, &c->L.fpart, &c->L.rec}) MPH_CK(ctx_dalloc(c, p, cap));
    for (double** p : {&c->L.dens_a, &c->L.vstrain, &c->L.divp}) MPH_CK(ctx_dalloc(c, p, cap));
    MPH_HIP_OK(c, hipMemsetAsync(c->L.cnt, 0, sizeof(int) * c->P.ncell, c->stream));
    MPH_HIP_OK(c, hipMemsetAsync(c->L.bsum, 0, sizeof(int) * bs, c->stream));
    MPH_HIP_OK(c, hipMemsetAsync(c->L.force, 0, sizeof(double4) * std::max(cap, 1), c->stream));
    MPH_HIP_OK(c, hipMemsetAsync(c->L.acc, 0, sizeof(double4) * std::max(cap, 1), c->stream));
    MPH_HIP_OK(c, hipMemcpyAsync(dT, &T, sizeof(DevTables), hipMemcpyHostToDevice, c->stream));
    DevState st{};
    st.time = a.cfg->time;
    for (int t = 0; t < kTypes; ++t)
        for (int d = 0; d < 3; ++d) {
            st.wall_c[t][d] = a.cfg->wall_center[t][d];
            st.wall_vel[t][d] = a.cfg->wall_velocity[t][d];
            st.wall_omega[t][d] = a.cfg->wall_omega[t][d];
            for (int e = 0; e < 3; ++e) st.wall_rot[t][d][e] = c->h.wall_rot[t][d][e];
        }
    MPH_HIP_OK(c, hipMemcpyAsync(c->L.st, &st, sizeof(DevState), hipMemcpyHostToDevice, c->stream));
    return MPH_OK;
}

static int init_upload_particles(MphCtx* c, const CreateArgs& a)
{
    // upload into the B set (original order, id = file index); the init sort reorders it
    const int m = c->n;
    std::vector<int> sel(m);
    for (int i = 0; i < m; ++i) sel[i] = c->dist ? a.owned[i] : i;
    std::vector<double> comp(m);
    std::vector<int> gids(m), types(m);
    double* dstc[6] = {c->L.B.x, c->L.B.y, c->L.B.z, c->L.B.vx, c->L.B.vy, c->L.B.vz};
    for (int k = 0; k < 6; ++k) {
        const double* src = k < 3 ? a.pos : a.vel;
        for (int i = 0; i < m; ++i) comp[i] = src[3 * (size_t)sel[i] + (k % 3)];
        MPH_HIP_OK(c, hipMemcpy(dstc[k], comp.data(), sizeof(double) * m, hipMemcpyHostToDevice));
    }
    for (int i = 0; i < m; ++i) { gids[i] = glob_id(c, sel[i]); types[i] = a.property[sel[i]]; }
    MPH_HIP_OK(c, hipMemcpy(c->L.B.type, types.data(), sizeof(int) * m, hipMemcpyHostToDevice));
    MPH_HIP_OK(c, hipMemcpy(c->L.B.id, gids.data(), sizeof(int) * m, hipMemcpyHostToDevice));
    return MPH_OK;
}

// calculateInitialNeighbor + calculateNormalizer on the device (single context: the local slots
// are all slots, in file order); the host keeps counts and normalizers for mph_get
static int elastic_device_build(MphCtx* c, int ns)
{
    StructDev& D = c->Sd;
    StructureInit& S = c->S;
    ctx_fill_launch(c);
    auto alloc = [](void* ctx, size_t bytes) -> void* {
        int st = MPH_OK;
        return ctx_alloc((MphCtx*)ctx, bytes, &st);
    };
    const int r = launch_struct_init(c->L, ns, D.x0, c->L.key, c->L.slot, c->L.tmp, c->order, D.ocnt, D.icnt,
                                     &D.eo_nb, &D.wo, &D.ei_nb, &D.wi, D.L, D.wx0, alloc, c);
    if (r == -2) return ctx_fail(c, MPH_ERR_NEIGHBOR_OVERFLOW, "a structure particle has >= 512 initial neighbours");
    if (r == -3) return ctx_fail(c, MPH_ERR_DEVICE_OOM, "structure list allocation failed");
    if (r != 0) return ctx_fail(c, MPH_ERR_HIP, "structure initialisation kernels failed");
    S.count.resize(ns);
    S.normalizer.resize((size_t)ns * 9);
    MPH_HIP_OK(c, hipMemcpyAsync(S.count.data(), D.ocnt, sizeof(int) * ns, hipMemcpyDeviceToHost, c->stream));
    MPH_HIP_OK(c, hipMemcpyAsync(S.normalizer.data(), D.L, sizeof(double) * 9 * ns, hipMemcpyDeviceToHost,
                             c->stream));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    return MPH_OK;
}

// ELL tiles of the host-built fixed out-list and of its transpose (StructDev), computed slots only
static int elastic_host_build(MphCtx* c, const std::vector<int>& lsl, int no)
{
    StructDev& D = c->Sd;
    const StructureInit& S = c->S;
    const int nl = (int)lsl.size();
    std::vector<int> loc(S.orig.size(), -1);
    for (int k = 0; k < nl; ++k) loc[lsl[k]] = k;
    const size_t ntile_s = ((size_t)std::max(no, 1) + 63) / 64;
    std::vector<int> ocnt(std::max(no, 1), 0), icnt(std::max(no, 1), 0);
    int wo = 0, wi = 0;
    for (int s = 0; s < no; ++s) {
        const int g = lsl[s];
        ocnt[s] = S.offset[g + 1] - S.offset[g];
        icnt[s] = S.in_offset[g + 1] - S.in_offset[g];
        wo = std::max(wo, ocnt[s]);
        wi = std::max(wi, icnt[s]);
    }
    wo = std::max(wo, 1);
    wi = std::max(wi, 1);
    D.wo = wo;
    D.wi = wi;
    std::vector<int> eo_nb(ntile_s * wo * 64, 0), ei_nb(ntile_s * wi * 64, 0);
    std::vector<double4> wx0(nl, make_double4(0.0, 0.0, 0.0, 0.0));
    for (int s = 0; s < no; ++s) {
        const int g = lsl[s];
        const size_t base_o = (size_t)(s >> 6) * wo * 64 + (s & 63);
        double c3[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < ocnt[s]; ++k) {
            const size_t q = S.offset[g] + k;
            const double* pr = &S.pair_out[4 * q];
            eo_nb[base_o + (size_t)k * 64] = loc[S.nbr[q]];
            for (int d = 0; d < 3; ++d) c3[d] += pr[3] * pr[d];
        }
        wx0[s] = make_double4(c3[0], c3[1], c3[2], 0.0);
        const size_t base_i = (size_t)(s >> 6) * wi * 64 + (s & 63);
        for (int k = 0; k < icnt[s]; ++k) {
            const size_t q = S.in_offset[g] + k;
            ei_nb[base_i + (size_t)k * 64] = loc[S.in_nbr[q]];
        }
    }
    for (int e : eo_nb) if (e < 0) return ctx_fail(c, MPH_ERR_DOMAIN, "structure list leaves the ghost slots");
    for (int e : ei_nb) if (e < 0) return ctx_fail(c, MPH_ERR_DOMAIN, "structure list leaves the ghost slots");
    std::vector<double> Lm((size_t)nl * 9);
    for (int s = 0; s < nl; ++s)
        std::memcpy(&Lm[(size_t)9 * s], &S.normalizer[(size_t)9 * lsl[s]], sizeof(double) * 9);
    MPH_CK(ctx_dalloc(c, &D.eo_nb, eo_nb.size()));
    MPH_CK(ctx_dalloc(c, &D.ei_nb, ei_nb.size()));
    MPH_HIP_OK(c, upload(c, D.ocnt, ocnt)); MPH_HIP_OK(c, upload(c, D.icnt, icnt));
    MPH_HIP_OK(c, upload(c, D.eo_nb, eo_nb));
    MPH_HIP_OK(c, upload(c, D.ei_nb, ei_nb));
    MPH_HIP_OK(c, upload(c, D.wx0, wx0));
    MPH_HIP_OK(c, upload(c, D.L, Lm));
    return MPH_OK;
}

// elastic solid: local slots = [computed here | ghosts] (single GPU: every slot, no ghosts)
static int init_elastic(MphCtx* c, const CreateArgs& a)
{
    const int ns = (int)c->S.orig.size();
    if (ns == 0) return MPH_OK;
    StructDev& D = c->Sd;
    StructureInit& S = c->S;
    std::vector<int> lsl;   // local slot -> global slot
    int no = ns, ni = ns;
    if (c->dist) {
        MPH_CK(dist_struct_setup(c, lsl, no, ni));
    } else {
        lsl.resize(ns);
        for (int s = 0; s < ns; ++s) lsl[s] = s;
    }
    const int nl = (int)lsl.size();
    D.n_own = no;
    D.n_inner = ni;
    c->sl_orig.resize(nl);
    for (int k = 0; k < nl; ++k) c->sl_orig[k] = glob_id(c, S.orig[lsl[k]]);
    c->sl_s.assign(lsl.begin(), lsl.begin() + no);
    const int sd = c->P.dim;
    MPH_CK(ctx_dalloc(c, &D.orig, nl));
    MPH_CK(ctx_dalloc(c, &D.ocnt, std::max(no, 1))); MPH_CK(ctx_dalloc(c, &D.icnt, std::max(no, 1)));
    MPH_CK(ctx_dalloc(c, &D.bidx, nl));
    MPH_CK(ctx_dalloc(c, &D.wx0, nl));
    MPH_CK(ctx_dalloc(c, &D.L, (size_t)nl * 9)); MPH_CK(ctx_dalloc(c, &D.lame, nl)); MPH_CK(ctx_dalloc(c, &D.inv_rho, nl));
    MPH_CK(ctx_dalloc(c, &D.clamp, nl));
    for (double4** p : {&D.x0, &D.x, &D.v, &D.u}) MPH_CK(ctx_dalloc(c, p, nl));
    MPH_CK(ctx_dalloc(c, &D.P, (size_t)nl * (sd == 2 ? 1 : 3)));
    for (double** p : {&D.F, &D.E, &D.S}) MPH_CK(ctx_dalloc(c, p, (size_t)nl * 9));
    D.fes = nl;
    std::vector<double2> lame(nl);
    std::vector<double> irho(nl);
    std::vector<int> clamp(nl);
    std::vector<double4> x0(nl);
    for (int s = 0; s < nl; ++s) {
        const int g = lsl[s];
        const int i = S.orig[g];
        const int t = a.property[i];
        lame[s] = make_double2(S.lame_l[g], S.lame_m[g]);
        irho[s] = 1.0 / a.cfg->density[t];
        const double* p0 = a.pos0 + 3 * (size_t)i;
        int cl = 0;   // updateElasticPosition module clamps (main.cpp:1918-2044)
        switch (a.cfg->module) {
        case MPH_MODULE_BAR: cl = p0[0] < 0.001 ? 1 : 0; break;
        case MPH_MODULE_DAM: cl = p0[1] < 0.002 ? 1 : 0; break;
        case MPH_MODULE_TUREK_HRON: cl = p0[0] < 0.205 ? 2 : 0; break;
        case MPH_MODULE_ROLLING1: cl = p0[1] < 0.003 ? 1 : 0; break;
        case MPH_MODULE_HYDROELASTIC: cl = (p0[0] < 0.01 || p0[0] > 1.99) ? 1 : 0; break;
        default: cl = 0;
        }
        clamp[s] = cl;
        x0[s] = make_double4(p0[0], p0[1], p0[2], (double)t);
    }
    MPH_HIP_OK(c, upload(c, D.x0, x0));
    MPH_CK(a.gpu_init ? elastic_device_build(c, ns) : elastic_host_build(c, lsl, no));
    MPH_HIP_OK(c, hipMemcpyAsync(D.orig, c->sl_orig.data(), sizeof(int) * nl, hipMemcpyHostToDevice, c->stream));
    {
        std::vector<int> slot_of((size_t)c->n_glob, -1);
        for (int s = 0; s < no; ++s) slot_of[c->sl_orig[s]] = s;
        MPH_CK(ctx_dalloc(c, &D.slot_of, slot_of.size()));
        MPH_HIP_OK(c, hipMemcpy(D.slot_of, slot_of.data(), sizeof(int) * slot_of.size(), hipMemcpyHostToDevice));
    }
    MPH_HIP_OK(c, upload(c, D.lame, lame));
    MPH_HIP_OK(c, upload(c, D.inv_rho, irho));
    MPH_HIP_OK(c, upload(c, D.clamp, clamp));
    MPH_HIP_OK(c, hipMemsetAsync(D.P, 0, sizeof(double4) * (sd == 2 ? 1 : 3) * nl, c->stream));
    MPH_HIP_OK(c, hipMemsetAsync(D.u, 0, sizeof(double4) * nl, c->stream));
    MPH_HIP_OK(c, hipMemsetAsync(D.bidx, 0, sizeof(int) * nl, c->stream));
    for (double* m : {D.F, D.E, D.S})
        MPH_HIP_OK(c, hipMemsetAsync(m, 0, sizeof(double) * 9 * nl, c->stream));
    MPH_HIP_OK(c, hipStreamSynchronize(c->stream));
    return MPH_OK;
}

// slab mode: the exchange's allocations, the initial ghost exchange and the init sums; else the
// initialisation sums of main.cpp:565-568 (calculateNeighbor, DensityA, GravityCenter, DensityP)
static int init_first_sums(MphCtx* c)
{
    ctx_fill_launch(c);
    if (c->dist) {
        MPH_CK(dist_alloc(c));
        MPH_CK(dist_init(c));
    } else {
        launch_sort(c->L, 0);
        launch_search_pass_a(c->L);
        if (c->lazy_walls) {   // the coarse map of the lazy wall steps: all zero between steps
            const size_t mb = coarse_map_bytes(c->P.gc);
            MPH_CK(ctx_dalloc(c, &c->L.cmap, mb));
            MPH_HIP_OK(c, hipMemsetAsync(c->L.cmap, 0, mb, c->stream));
            c->L.cmap_bytes = (int)mb;
        }
    }
    MPH_HIP_OK(c, hipGetLastError());
    return ctx_status(c);
}

static int ctx_init(MphCtx* c, CreateArgs& a)
{
    MPH_CK(init_check_args(c, a));
    MPH_CK(init_host_state(c, a));
    MPH_CK(init_grid(c, a));
    MPH_CK(init_capacity(c, a));
    MPH_CK(init_alloc(c, a));
    MPH_CK(init_upload_particles(c, a));
    MPH_CK(init_elastic(c, a));
    return init_first_sums(c);
}

void ctx_set_global_error(const std::string& msg) { g_create_error = msg; }

int ctx_create(MphCtx** out, const MphConfig* cfg, int n, const int* property, const double* pos,
               const double* pos0, const double* vel, int device, MphDist* dist, const int* ids, int n_glob)
{
    g_create_error.clear();
    if (!out || !cfg || n < 0 || (n > 0 && (!property || !pos || !pos0 || !vel))) {
        delete dist;
        g_create_error = "invalid argument";
        return MPH_ERR_ARG;
    }
    *out = nullptr;
    MphCtx* c = new MphCtx();
    c->dist = dist;
    CreateArgs a{cfg, n, property, pos, pos0, vel, device, ids, n_glob};
    const int r = ctx_init(c, a);
    if (r != MPH_OK) {
        g_create_error = c->err.empty() ? "mph_create failed with status " + std::to_string(r) : c->err;
        mph_destroy(c);
        return r;
    }
    *out = c;
    return MPH_OK;
}

}  // namespace mph

extern "C" {

int mph_create(MphCtx** out, const MphConfig* cfg, int n, const int* property, const double* pos,
               const double* pos0, const double* vel, int device)
{
    return ctx_create(out, cfg, n, property, pos, pos0, vel, device, nullptr);
}

const char* mph_last_error(const MphCtx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

}  // extern "C"
