// mph_dist_select.hip -- particle selections on slab ranks, the collective calls (every rank enters
// them with the same selection made; host only, no kernels) and the host-only combine of the ranks'
// totals.  The calls without communication -- mph_dist_select, mph_dist_selected_ids,
// mph_dist_get_selected, mph_dist_selection_totals_partial -- are in mph_fields.hip beside the single
// context's; the kernels in mph_select.hip.
//
// A rank's selection is a subset of the particles it owns, as ascending original indices, and
// ownership is a partition: the ranks' lists are disjoint, and merged by index they are the whole
// problem's selection.  Every collective call sends one message per rank -- a head, the rank's ids,
// then its rows of every field asked for, gathered on the device (mph_dist_get_selected) -- over
// Transport::gather_root, and rank 0 merges the rows by ascending index.  Only selected rows travel: no
// rank fetches a whole array and rank 0 builds nothing of n_glob rows (unlike pack_owned,
// mph_dist_output.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "mph_dist.h"

using namespace mph;

namespace {

// the head of a rank's message: its selected count, and the bytes of a row of each of nf fields;
// behind it count ids (int), then per field count rows
constexpr int kSelMsgFields = 10;   // the fields of a frame (write_selected)
struct SelMsgHead {
    long long count;
    int nf;
    int row[kSelMsgFields];
    int pad;
};

// bytes of a row of mph_get_selected(field)
int field_row_bytes(int field)
{
    switch (field) {
    case MPH_FIELD_NEIGHBOR_COUNT:
    case MPH_FIELD_INITIAL_STRUCTURE_NEIGHBOR_COUNT:
    case MPH_FIELD_PROPERTY: return (int)sizeof(int);
    case MPH_FIELD_POSITION:
    case MPH_FIELD_INITIAL_POSITION:
    case MPH_FIELD_VELOCITY:
    case MPH_FIELD_FORCE:
    case MPH_FIELD_ACCELERATION:
    case MPH_FIELD_GRAVITY_CENTER: return 3 * (int)sizeof(double);
    case MPH_FIELD_DEFORM_GRADIENT:
    case MPH_FIELD_STRAIN:
    case MPH_FIELD_STRESS:
    case MPH_FIELD_NORMALIZER:
    case MPH_FIELD_VIRIAL_STRESS: return 9 * (int)sizeof(double);
    default: return (int)sizeof(double);
    }
}

// The merged selection on rank 0: the ids ascending, and per field the rows in that order.
struct Merged {
    std::vector<int> ids;
    std::vector<std::vector<char>> rows;   // [nf][count * row bytes]
};

// Every rank: its ids and its rows of `fields` packed and gathered; rank 0: merged by ascending index
// into *m (the other ranks leave it empty).
int gather_rows(MphCtx* c, const char* who, const int* fields, int nf, Merged* m)
{
    MphDist& D = *c->dist;
    const size_t cnt = c->sel_ids.size();
    SelMsgHead h{};
    h.count = (long long)cnt;
    h.nf = nf;
    size_t bytes = sizeof(h) + sizeof(int) * cnt;
    for (int f = 0; f < nf; ++f) {
        h.row[f] = field_row_bytes(fields[f]);
        bytes += (size_t)h.row[f] * cnt;
    }
    std::vector<char> mine(bytes), all;
    char* o = mine.data();
    std::memcpy(o, &h, sizeof(h));
    o += sizeof(h);
    if (cnt) std::memcpy(o, c->sel_ids.data(), sizeof(int) * cnt);
    o += sizeof(int) * cnt;
    int rc = MPH_OK;
    for (int f = 0; f < nf && rc == MPH_OK; ++f) {
        rc = mph_dist_get_selected(c, fields[f], o);   // (cnt == 0: nothing is written)
        o += (size_t)h.row[f] * cnt;
    }
    if (rc != MPH_OK) {
        // a rank that cannot read its rows (InitialPosition of a particle it has no static inputs for)
        // still takes part, with a head alone that rank 0 refuses: no rank is left waiting
        const std::string err = c->err;
        h.count = -1;
        mine.resize(sizeof(h));
        std::memcpy(mine.data(), &h, sizeof(h));
        (void)D.tr->gather_root(c, c->stream, mine, all);
        return ctx_fail(c, rc, err);
    }
    MPH_CK(D.tr->gather_root(c, c->stream, mine, all));
    if (D.rank != 0) return MPH_OK;
    // the ranks' messages, one behind the other
    std::vector<SelMsgHead> head(D.nranks);
    std::vector<const char*> at(D.nranks);
    const char* p = all.data();
    const char* end = p + all.size();
    size_t total = 0;
    for (int r = 0; r < D.nranks; ++r) {
        bool ok = (size_t)(end - p) >= sizeof(SelMsgHead);
        if (ok) {
            std::memcpy(&head[r], p, sizeof(SelMsgHead));
            p += sizeof(SelMsgHead);
            ok = head[r].count >= 0 && head[r].count <= c->n_glob && head[r].nf == nf;
            size_t need = ok ? sizeof(int) * (size_t)head[r].count : 0;
            for (int f = 0; ok && f < nf; ++f) {
                ok = head[r].row[f] == h.row[f];
                need += (size_t)h.row[f] * (size_t)head[r].count;
            }
            ok = ok && (size_t)(end - p) >= need;
            at[r] = p;
            if (ok) p += need;
        }
        if (!ok)
            return ctx_fail(c, MPH_ERR_TRANSPORT, std::string(who) + ": the message of rank " + std::to_string(r) + " is incomplete");
        total += (size_t)head[r].count;
    }
    if (total > (size_t)c->n_glob) return ctx_fail(c, MPH_ERR_CAPACITY, std::string(who) + ": ownership is not a partition");
    m->ids.resize(total);
    m->rows.assign(nf, std::vector<char>());
    for (int f = 0; f < nf; ++f) m->rows[f].resize(total * (size_t)h.row[f]);
    // every rank's list ascends: the smallest head among the ranks is next
    std::vector<size_t> k(D.nranks, 0);
    auto id_of = [&](int r, size_t j) {
        int v;
        std::memcpy(&v, at[r] + sizeof(int) * j, sizeof(v));
        return v;
    };
    int last = -1;
    for (size_t t = 0; t < total; ++t) {
        int from = -1, best = 0;
        for (int r = 0; r < D.nranks; ++r) {
            if (k[r] >= (size_t)head[r].count) continue;
            const int v = id_of(r, k[r]);
            if (from < 0 || v < best) { from = r; best = v; }
        }
        if (best <= last || best >= c->n_glob)
            return ctx_fail(c, MPH_ERR_CAPACITY, std::string(who) + ": ownership is not a partition");
        last = best;
        m->ids[t] = best;
        const char* rows = at[from] + sizeof(int) * (size_t)head[from].count;
        for (int f = 0; f < nf; ++f) {
            const size_t w = (size_t)h.row[f];
            std::memcpy(&m->rows[f][t * w], rows + k[from] * w, w);
            rows += (size_t)head[from].count * w;
        }
        ++k[from];
    }
    return MPH_OK;
}

// what the collective calls open with: the flush, a slab context, a current selection
int coll_enter(MphCtx* c, const char* who)
{
    if (!c) return MPH_ERR_ARG;
    MPH_CK(ctx_flush(c));
    if (!c->dist)
        return ctx_fail(c, MPH_ERR_UNSUPPORTED, std::string(who) + ": slab selections need a slab context (a single context: "
                                                    "mph_select and its readers)");
    MPH_HIP_OK(c, hipSetDevice(c->device));
    if (!c->sel_current)
        return ctx_fail(c, MPH_ERR_ARG, std::string(who) + ": no current selection (none was made, or the state has changed "
                                            "since: mph_dist_select again after mph_step / mph_set)");
    return MPH_OK;
}

int write_selected(MphCtx* c, const char* path, bool xml)
{
    if (!c || !path) return MPH_ERR_ARG;
    const char* who = xml ? "mph_dist_write_vtu_selected" : "mph_dist_write_vtk_selected";
    MPH_CK(coll_enter(c, who));
    // the arrays of the writers, in the order of their arguments
    const int fields[kSelMsgFields] = {MPH_FIELD_PROPERTY, MPH_FIELD_POSITION, MPH_FIELD_INITIAL_POSITION, MPH_FIELD_VELOCITY,
                                       MPH_FIELD_ACCELERATION, MPH_FIELD_FORCE, MPH_FIELD_STRESS, MPH_FIELD_STRAIN,
                                       MPH_FIELD_INITIAL_STRUCTURE_NEIGHBOR_COUNT, MPH_FIELD_NEIGHBOR_COUNT};
    Merged m;
    MPH_CK(gather_rows(c, who, fields, kSelMsgFields, &m));
    if (c->dist->rank != 0) return MPH_OK;
    for (auto& v : m.rows)
        if (v.empty()) v.resize(9 * sizeof(double));   // (the writers are handed non-null arrays)
    auto ints = [&](int f) { return reinterpret_cast<const int*>(m.rows[f].data()); };
    auto dbls = [&](int f) { return reinterpret_cast<const double*>(m.rows[f].data()); };
    auto writer = xml ? mph_write_vtu_arrays : mph_write_vtk_arrays;
    const int rc = writer(path, (int)m.ids.size(), ints(0), dbls(1), dbls(2), dbls(3), dbls(4), dbls(5), dbls(6), dbls(7),
                          ints(8), ints(9));
    return rc ? ctx_fail(c, rc, std::string(who) + ": writing " + path) : MPH_OK;
}

}  // namespace

extern "C" {

int mph_totals_combine(int nranks, const double* const* records, double out[MPH_TOTALS])
{
#pragma clang fp contract(off)
    if (nranks < 1 || !records || !out) return MPH_ERR_ARG;
    for (int r = 0; r < nranks; ++r)
        if (!records[r]) return MPH_ERR_ARG;
    for (int k = 0; k < MPH_TOTALS; ++k) {
        if (k >= MPH_TOT_RESERVED0) {
            out[k] = 0.0;
            continue;
        }
        // the extent alternates minimum, maximum from XMIN; VMAX2 is a maximum; everything before a sum
        const bool sum = k < MPH_TOT_XMIN, mn = !sum && k < MPH_TOT_VMAX2 && (k - MPH_TOT_XMIN) % 2 == 0;
        double v = records[0][k];
        for (int r = 1; r < nranks; ++r) {
            const double b = records[r][k];
            v = sum ? v + b : (mn ? std::fmin(v, b) : std::fmax(v, b));
        }
        out[k] = v;
    }
    return MPH_OK;
}

int mph_dist_selection_totals(MphCtx* c, const double center[3], double out[MPH_TOTALS])
{
    if (!c || !center) return MPH_ERR_ARG;
    MPH_CK(coll_enter(c, "mph_dist_selection_totals"));
    MphDist& D = *c->dist;
    if (D.rank == 0 && !out) return MPH_ERR_ARG;
    double rec[MPH_TOTALS];
    MPH_CK(mph_dist_selection_totals_partial(c, center, rec));
    const char* b = reinterpret_cast<const char*>(rec);
    std::vector<char> mine(b, b + sizeof(rec)), all;
    MPH_CK(D.tr->gather_root(c, c->stream, mine, all));
    if (D.rank != 0) return MPH_OK;
    if (all.size() != sizeof(rec) * (size_t)D.nranks)
        return ctx_fail(c, MPH_ERR_TRANSPORT, "mph_dist_selection_totals: the gather brought " + std::to_string(all.size()) + " bytes");
    std::vector<double> recs((size_t)MPH_TOTALS * D.nranks);
    std::memcpy(recs.data(), all.data(), all.size());
    std::vector<const double*> of(D.nranks);
    for (int r = 0; r < D.nranks; ++r) of[r] = recs.data() + (size_t)MPH_TOTALS * r;
    return mph_totals_combine(D.nranks, of.data(), out);
}

long long mph_dist_gather_selected(MphCtx* c, int field, void* out, int* ids, long long cap_rows)
{
    if (!c || cap_rows < 0) return MPH_ERR_ARG;
    MPH_CK(coll_enter(c, "mph_dist_gather_selected"));
    if (field < 0 || field >= MPH_FIELD_COUNT) return ctx_fail(c, MPH_ERR_ARG, "unknown field " + std::to_string(field));
    Merged m;
    MPH_CK(gather_rows(c, "mph_dist_gather_selected", &field, 1, &m));
    if (c->dist->rank != 0) return 0;
    const size_t total = m.ids.size();
    if (total > (size_t)cap_rows || (total > 0 && (!out || !ids)))
        return ctx_fail(c, MPH_ERR_ARG, "mph_dist_gather_selected: " + std::to_string(total) + " rows selected, room for " +
                                            std::to_string(cap_rows));
    if (total) {
        std::memcpy(ids, m.ids.data(), sizeof(int) * total);
        std::memcpy(out, m.rows[0].data(), m.rows[0].size());
    }
    return (long long)total;
}

int mph_dist_write_vtk_selected(MphCtx* c, const char* path) { return write_selected(c, path, false); }

int mph_dist_write_vtu_selected(MphCtx* c, const char* path) { return write_selected(c, path, true); }

}  // extern "C"
