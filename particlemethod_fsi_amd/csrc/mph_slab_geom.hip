// mph_slab_geom.hip -- where the slabs of the decomposition lie, who owns a coordinate, and what
// follows from that for a rank at creation: its window grid and owned set (dist_setup) and the
// static routing of its elastic ghost slots (dist_struct_setup).  Host only, no kernels.  Built
// with the flags of the device units, not the host layer's: a cut that moved by an ulp would
// change the owner of a particle on a face.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "mph_dist.h"

namespace mph {

void slab_of(const HostDerived& h, int axis, int rank, int nranks, const double* cuts, double& lo, double& hi)
{
    const double W = h.dw[axis];
    if (cuts) {
        lo = rank == 0 ? h.dmin[axis] : cuts[rank - 1];
        hi = rank == nranks - 1 ? h.dmax[axis] : cuts[rank];
        return;
    }
    lo = rank == 0 ? h.dmin[axis] : h.dmin[axis] + W * rank / nranks;
    hi = rank == nranks - 1 ? h.dmax[axis] : h.dmin[axis] + W * (rank + 1) / nranks;
}

int check_cuts(const HostDerived& h, int axis, int nranks, const double* cuts, std::string& err)
{
    if (!cuts) return MPH_OK;
    for (int k = 0; k < nranks - 1; ++k) {
        const double lo = k == 0 ? h.dmin[axis] : cuts[k - 1];
        if (!(cuts[k] > lo) || !(cuts[k] < h.dmax[axis])) {
            err = "slab cuts must ascend strictly inside the domain";
            return MPH_ERR_ARG;
        }
    }
    return MPH_OK;
}

SlabGeom make_geom(const HostDerived& h, int axis, int rank, int nranks, const double* cuts, double halo)
{
    SlabGeom g{};
    g.axis = axis;
    g.w = h.dw[axis];
    const int l = (rank + nranks - 1) % nranks, r = (rank + 1) % nranks;
    slab_of(h, axis, rank, nranks, cuts, g.lo, g.hi);
    slab_of(h, axis, l, nranks, cuts, g.llo, g.lhi);
    slab_of(h, axis, r, nranks, cuts, g.rlo, g.rhi);
    g.first = rank == 0; g.last = rank == nranks - 1;
    g.lfirst = l == 0; g.llast = l == nranks - 1;
    g.rfirst = r == 0; g.rlast = r == nranks - 1;
    g.h = halo;
    return g;
}

double wrap_coord(const HostDerived& h, int axis, double x)
{
#pragma clang fp contract(off)
    const double w = h.dw[axis];
    const double u = x - h.dmin[axis];
    return u - w * std::floor(u / w) + h.dmin[axis];
}

int owner_rank(const HostDerived& h, int axis, int nranks, const double* cuts, double x)
{
    const double a = wrap_coord(h, axis, x);
    for (int r = 0; r < nranks; ++r) {
        double lo, hi;
        slab_of(h, axis, r, nranks, cuts, lo, hi);
        if (slab_owns(a, lo, hi, r == 0, r == nranks - 1)) return r;
    }
    return nranks - 1;
}

void lattice_owners(const HostDerived& h, int axis, int nranks, const double* cuts, double origin_a, double spacing_a,
                    int count_a, int* owner)
{
#pragma clang fp contract(off)
    for (int i = 0; i < count_a; ++i) {
        // (the kernels' expression: sample_point, k_gauge_grid)
        const double prod = (double)i * spacing_a;
        const double x = origin_a + prod;
        owner[i] = owner_rank(h, axis, nranks, cuts, x);
    }
}

double slab_offset(const HostDerived& h, int axis, int r, int nranks, const double* cuts, double x)
{
    double lo, hi;
    slab_of(h, axis, r, nranks, cuts, lo, hi);
    const double W = h.dw[axis];
    double off = x - 0.5 * (lo + hi);
    off -= W * std::floor(off / W + 0.5);
    return off;
}

int check_geometry(const MphConfig& cfg, int nranks, int axis, std::string& err)
{
    if (nranks < 2) { err = "slab mode needs nranks >= 2 (use mph_create)"; return MPH_ERR_ARG; }
    if (axis < 0 || axis > 2 || (cfg.dim == 2 && axis == 2)) { err = "invalid slab axis"; return MPH_ERR_ARG; }
    return MPH_OK;
}

// -- a rank's share at creation: its geometry, window grid and owned set; its elastic slots --------

int dist_setup(MphCtx* c, const double* pos, std::vector<int>& owned)
{
    MphDist& D = *c->dist;
    const HostDerived& h = c->h;
    const int axis = D.g.axis;
    std::string err;
    MPH_CK(ctx_fail(c, check_geometry(c->cfg, D.nranks, axis, err), err));
    D.side[kLeft].peer = (D.rank + D.nranks - 1) % D.nranks;
    D.side[kRight].peer = (D.rank + 1) % D.nranks;
    // elastic particles may be displaced up to kStructMargin dx beyond their static slab
    const bool has_struct = !c->S.orig.empty();
    const double smargin = has_struct ? kStructMargin * h.dx : 0.0;
    const double halo = halo_width(c->P) + smargin;
    MPH_CK(ctx_fail(c, check_cuts(h, axis, D.nranks, dist_cuts(D), err), err));
    D.g = make_geom(h, axis, D.rank, D.nranks, dist_cuts(D), halo);
    D.g.smargin = smargin;
    const double W = h.dw[axis];
    const double cw = W / c->P.gc[axis];
    // slabs must be wider than two halos plus a migration margin, so that a band particle is
    // mirrored to one neighbour only and a migrant reaches only the adjacent slab
    for (int r = 0; r < D.nranks; ++r) {
        double lo, hi;
        slab_of(h, axis, r, D.nranks, dist_cuts(D), lo, hi);
        if (hi - lo < 2.0 * halo + 2.0 * h.dx)
            return ctx_fail(c, MPH_ERR_DOMAIN, "slab width " + std::to_string(hi - lo) + " below two halo widths (" +
                                                   std::to_string(2.0 * halo) + ")");
    }
    // local window grid along the slab axis: [lo - h - cw, hi + h + cw)
    const double wlo = D.g.lo - halo - cw, whi = D.g.hi + halo + cw;
    const int gloc = (int)std::ceil((whi - wlo) / cw);
    const int m = stencil_margin(c->P, axis);
    if (gloc < 2 * m - 1) return ctx_fail(c, MPH_ERR_DOMAIN, "slab window narrower than the cell stencil");
    c->P.corg[axis] = wlo;
    c->P.slab_axis = axis;
    c->P.slab_lo = D.g.lo;
    c->P.slab_hi = D.g.hi;
    // pass B's face wavefronts (particles within slab_h of a face, integrated after the halo) also
    // carry every particle the next redistribution can send: one step moves a particle far less
    // than the 2 dx margin (checked: k_dist_classify flags a sender outside them)
    c->P.slab_h = halo + 2.0 * h.dx;
    c->P.gc[axis] = std::min(gloc, c->P.gc[axis] + 1);
    // fast-path interior: >= 3 cells inside both the window and the periodic domain
    c->P.inner_lo[axis] = std::max(wlo, h.dmin[axis]) + m * cw * (1.0 + 1e-9);
    c->P.inner_hi[axis] = std::min(whi, h.dmax[axis]) - m * cw * (1.0 + 1e-9);
    // the search's box in offsets from the window's edge; the face box always applies on this axis
    c->P.sinner_lo[axis] = std::max(wlo, h.dmin[axis]) - wlo + m * cw * (1.0 + 1e-9);
    c->P.sinner_hi[axis] = std::min(whi, h.dmax[axis]) - wlo - m * cw * (1.0 + 1e-9);
    c->P.seam_always |= 1 << axis;
    // initial owned set and a capacity for owned + ghosts (+ headroom for migration imbalance)
    owned.clear();
    size_t near = 0;
    const int nin = (int)c->prop.size();   // the particles passed in (all, or this rank's window)
    for (int i = 0; i < nin; ++i) {
        const double a = wrap_coord(h, axis, pos[3 * (size_t)i + axis]);
        if (is_struct(c->prop[i])) {
            // static owner: the slab of the InitialPosition
            if (owner_rank(h, axis, D.nranks, dist_cuts(D), c->pos0[3 * (size_t)i + axis]) == D.rank)
                owned.push_back(i);
            else ++near;
            continue;
        }
        if (slab_owns(a, D.g.lo, D.g.hi, D.g.first, D.g.last)) {
            owned.push_back(i);
        } else {
            // within h + 2 dx outside a face (periodic distance): a ghost candidate
            double dl = D.g.lo - a, dh = a - D.g.hi;
            dl -= W * std::floor(dl / W);
            dh -= W * std::floor(dh / W);
            if (std::min(dl, dh) <= halo + 2.0 * h.dx) ++near;
        }
    }
    const size_t want = (size_t)((owned.size() + near) * 1.25) + 65536;
    D.cap = (int)std::min<size_t>(want, (size_t)c->n_glob);
    D.n_own = (int)owned.size();
    return MPH_OK;
}

int dist_struct_setup(MphCtx* c, std::vector<int>& lsl, int& n_own, int& n_inner)
{
    MphDist& D = *c->dist;
    const HostDerived& h = c->h;
    const StructureInit& S = c->S;
    const int axis = D.g.axis, R = D.nranks;
    const int ns = (int)S.orig.size();
    std::vector<int> owner(ns);
    const double* cuts = dist_cuts(D);
    for (int s = 0; s < ns; ++s) owner[s] = owner_rank(h, axis, R, cuts, c->pos0[3 * (size_t)S.orig[s] + axis]);
    // ghost slots of rank r: the list neighbours (out- and in-lists) of its owned slots that other
    // ranks own, split by side (periodic offset of x0 from r's slab centre), ascending slot id
    std::string err;
    auto ghosts = [&](int r, std::vector<int>& gl, std::vector<int>& gr) {
        std::vector<char> seen(ns, 0);
        gl.clear();
        gr.clear();
        const int left = (r + R - 1) % R, right = (r + 1) % R;
        auto visit = [&](int j) {
            if (owner[j] == r || seen[j]) return;
            seen[j] = 1;
            const bool lside = slab_offset(h, axis, r, R, cuts, c->pos0[3 * (size_t)S.orig[j] + axis]) < 0.0;
            if (owner[j] != (lside ? left : right)) err = "structure list spans more than one slab";
            (lside ? gl : gr).push_back(j);
        };
        for (int s = 0; s < ns; ++s) {
            if (owner[s] != r) continue;
            for (int q = S.offset[s]; q < S.offset[s + 1]; ++q) visit(S.nbr[q]);
            for (int q = S.in_offset[s]; q < S.in_offset[s + 1]; ++q) visit(S.in_nbr[q]);
        }
        std::sort(gl.begin(), gl.end());
        std::sort(gr.begin(), gr.end());
    };
    std::vector<int> gl, gr, lgl, lgr, rgl, rgr;
    ghosts(D.rank, gl, gr);
    ghosts(D.side[kLeft].peer, lgl, lgr);
    ghosts(D.side[kRight].peer, rgl, rgr);
    if (!err.empty()) return ctx_fail(c, MPH_ERR_DOMAIN, "slab mode: " + err);
    // the owned slots, those without a ghost slot in their out- or in-list first (the lists are
    // symmetric, so every slot a neighbour needs is among the others): their substep halves run
    // while the ghost exchange travels (struct_substeps)
    lsl.clear();
    std::vector<int> outer;
    for (int s = 0; s < ns; ++s) {
        if (owner[s] != D.rank) continue;
        bool ghost = false;
        for (int q = S.offset[s]; q < S.offset[s + 1] && !ghost; ++q) ghost = owner[S.nbr[q]] != D.rank;
        for (int q = S.in_offset[s]; q < S.in_offset[s + 1] && !ghost; ++q) ghost = owner[S.in_nbr[q]] != D.rank;
        (ghost ? outer : lsl).push_back(s);
    }
    n_inner = (int)lsl.size();
    lsl.insert(lsl.end(), outer.begin(), outer.end());
    n_own = (int)lsl.size();
    std::vector<int> loc(ns, -1);
    for (int k = 0; k < n_own; ++k) loc[lsl[k]] = k;
    std::vector<int> snd[2], rcv[2];   // per side
    for (int j : gl) { rcv[kLeft].push_back((int)lsl.size()); loc[j] = (int)lsl.size(); lsl.push_back(j); }
    for (int j : gr) { rcv[kRight].push_back((int)lsl.size()); loc[j] = (int)lsl.size(); lsl.push_back(j); }
    // to the left: the left rank's from-right ghosts (ours); to the right: its from-left ghosts
    for (int j : lgr) snd[kLeft].push_back(loc[j]);
    for (int j : rgl) snd[kRight].push_back(loc[j]);
    for (const auto& v : snd)
        for (int k : v) if (k < 0 || k >= n_own) return ctx_fail(c, MPH_ERR_DOMAIN, "slab mode: elastic ghost routing");
    auto up = [&](int** d, int* count, const std::vector<int>& v) -> int {
        *count = (int)v.size();
        MPH_CK(ctx_dalloc(c, d, v.size()));
        if (!v.empty()) MPH_HIP_OK(c, hipMemcpy(*d, v.data(), sizeof(int) * v.size(), hipMemcpyHostToDevice));
        return MPH_OK;
    };
    for (int s = 0; s < 2; ++s) {
        MPH_CK(up(&D.side[s].ss, &D.side[s].nss, snd[s]));
        MPH_CK(up(&D.side[s].sr, &D.side[s].nsr, rcv[s]));
    }
    return MPH_OK;
}

}  // namespace mph

using namespace mph;

extern "C" {

int mph_slab_bounds(const MphConfig* cfg, int rank, int nranks, int axis, const double* cuts, double* out3)
{
    if (!cfg || !out3 || nranks < 1 || rank < 0 || rank >= nranks || axis < 0 || axis > 2) return MPH_ERR_ARG;
    HostDerived h{};
    derive_constants(*cfg, h);
    std::string err;
    if (check_cuts(h, axis, nranks, cuts, err) != MPH_OK) return MPH_ERR_ARG;
    DevParams P{};
    make_dev_params(*cfg, h, 0, 0, P);
    slab_of(h, axis, rank, nranks, cuts, out3[0], out3[1]);
    out3[2] = halo_width(P);
    return MPH_OK;
}

int mph_slab_window(const MphConfig* cfg, int rank, int nranks, int axis, const double* cuts, double* out2)
{
    double b[3];
    const int rc = mph_slab_bounds(cfg, rank, nranks, axis, cuts, b);
    if (rc != MPH_OK) return rc;
    if (!out2) return MPH_ERR_ARG;
    // two halo widths, each including the elastic particles' displacement margin, so that the
    // first redistribution's capacity estimate (dist_setup) and the structure lists of the owned
    // elastic particles (calculateInitialNeighbor reach) see every particle they need
    const double m = 2.0 * (b[2] + kStructMargin * cfg->particle_spacing);
    out2[0] = b[0] - m;
    out2[1] = b[1] + m;
    return MPH_OK;
}

int mph_slab_owner(const MphConfig* cfg, int nranks, int axis, const double* cuts, double x)
{
    if (!cfg || nranks < 1 || axis < 0 || axis > 2) return MPH_ERR_ARG;
    HostDerived h{};
    derive_constants(*cfg, h);
    std::string err;
    if (check_cuts(h, axis, nranks, cuts, err) != MPH_OK) return MPH_ERR_ARG;
    const double a = wrap_coord(h, axis, x);
    for (int r = 0; r < nranks; ++r) {
        double lo, hi;
        slab_of(h, axis, r, nranks, cuts, lo, hi);
        if (slab_owns(a, lo, hi, r == 0, r == nranks - 1)) return r;
    }
    return MPH_ERR_DOMAIN;
}

int mph_slab_lattice_owner(const MphConfig* cfg, int nranks, int axis, const double* cuts, double origin_a,
                           double spacing_a, int count_a, int* owner)
{
    if (!cfg || !owner || nranks < 1 || axis < 0 || axis > 2 || count_a < 1) return MPH_ERR_ARG;
    if (!std::isfinite(origin_a) || !std::isfinite(spacing_a) || !(spacing_a > 0.0)) return MPH_ERR_ARG;
    HostDerived h{};
    derive_constants(*cfg, h);
    std::string err;
    if (check_cuts(h, axis, nranks, cuts, err) != MPH_OK) return MPH_ERR_ARG;
    lattice_owners(h, axis, nranks, cuts, origin_a, spacing_a, count_a, owner);
    return MPH_OK;
}

}  // extern "C"
