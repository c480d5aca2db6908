// calipso_trajectory_tables.hpp — the host tables of a trajectory problem's device evaluator (calipso.jl_amd/trajectory.py, calipso_trajectory.hpp): plain C++17 with
// ONE copy, no HIP call, so that tests/trajectory_host/tables_main.cpp runs it under the sanitizers without a GPU.  It checks every index a user hands in (the int32
// blob of TrajectoryProblem.tables()) and computes every address the kernels later store through:
//   parse_tables   the blob -> Tables, or false when it does not fit the library's Shape or an index lies outside its range
//   dense_route    the int32 table of a route for the dense layout (calipso_device_problem_data, leading dimension jacobian_ld)
//   block_route    the same for the packed blocks of a structured handle (calipso_device_block_data)
//   sparse_route   the same for the three non-zero arrays of a sparse handle on their stored patterns (calipso_device_sparse_data)
// A route's table: per template its index tables as they are and its ADDRESS TABLE (entry -> offset in the destination), the finishing pass's addresses, field and
// slot lists, and the fill's chunks (offset, length <= CHUNK) by category.  Return codes: 0, 1 an argument that does not fit, 4 a non-zero outside the declared
// structure or a destination beyond 2^31 entries, 5 segments out of order (2 and 3 belong to calipso_trajectory.hpp: a HIP call failed, the layout changed).
#pragma once
#include <stdint.h>

#include <vector>

#include "calipso_hip.h"

namespace calipso {
namespace trajectory {

// destinations.  D_FX .. D_HP have one writer per address, D_F .. D_LGP are summed by the finishing pass
enum { D_FX, D_G, D_H, D_GX, D_HX, D_GP, D_HP, D_F, D_GYX, D_HZX, D_LXX, D_LGP, N_DEST };
constexpr int CHUNK = 1024;                    // elements one workgroup of the fill zeroes
constexpr int N_FILL = 6;                      // equality Jacobian, cone Jacobian, Hessian, dg/dtheta, dh/dtheta, the Lagrangian's theta-gradient

// what a generated library knows about its problem: per template its kind (trajectory.py: KINDS) and the sizes of its local variables, rows, parameters, direct
// entries and partials
struct Shape { int nt; const int *kind, *nv, *m, *nth, *nd, *nq; };

struct Tables {
    int G = 0, W = 0, n_obj = 0, nx = 0, ne = 0, nc = 0, np = 0;
    int64_t n_part = 0;
    std::vector<int> n;                                                    // per template: its instances
    std::vector<std::vector<int32_t>> vi, ri, pi, d_field, d_i, d_j;     // per template, stage-minor
    std::vector<int32_t> g_field, g_i, g_j, g_slots, obj_slots;
};

inline bool parse_tables(const Shape& sh, const int32_t* blob, int64_t words, Tables& u) {
    const int NT = sh.nt;
    if (!blob || words < 10 + 8 * (int64_t)NT || blob[0] != 0x43545250 || blob[1] != NT) return false;
    u.G = blob[2]; u.W = blob[3]; u.n_obj = blob[4]; u.n_part = blob[5]; u.nx = blob[6]; u.ne = blob[7]; u.nc = blob[8]; u.np = blob[9];
    u.n.assign((size_t)NT, 0);
    for (auto* v : {&u.vi, &u.ri, &u.pi, &u.d_field, &u.d_i, &u.d_j}) v->assign((size_t)NT, std::vector<int32_t>());
    int64_t at = 10, slots = 0;
    bool ok = u.G >= 0 && u.W >= 1 && u.n_obj >= 0 && u.n_part >= 0;
    for (int k = 0; k < NT && ok; ++k, at += 8) {
        const int32_t* h = blob + at;
        u.n[k] = h[1];
        ok = h[0] == sh.kind[k] && h[1] >= 0 && h[2] == sh.nv[k] && h[3] == sh.m[k] && h[4] == sh.nth[k] && h[5] == sh.nd[k] && h[6] == sh.nq[k];
        slots += (int64_t)sh.nq[k] * h[1];
    }
    ok = ok && slots == u.n_part && slots < (1 << 29);
    auto take = [&](std::vector<int32_t>& v, int64_t count, int64_t lo, int64_t hi) {       // every entry in [lo, hi)
        if (!ok || count < 0 || at + count > words) { ok = false; return; }
        v.assign(blob + at, blob + at + count); at += count;
        for (int32_t e : v) if (e < lo || e >= hi) { ok = false; return; }
    };
    for (int k = 0; k < NT && ok; ++k) {
        const int64_t n = u.n[k], rows = (sh.kind[k] == 1 || sh.kind[k] == 2) ? u.ne : u.nc;
        take(u.vi[k], sh.nv[k] * n, 0, u.nx); take(u.ri[k], sh.m[k] * n, 0, rows); take(u.pi[k], sh.nth[k] * n, 0, u.np);
        take(u.d_field[k], sh.nd[k], D_GX, D_HP + 1); take(u.d_i[k], sh.nd[k] * n, 0, rows);
        take(u.d_j[k], sh.nd[k] * n, 0, u.nx > u.np ? u.nx : u.np);
        for (int e = 0; e < sh.nd[k] && ok; ++e) {
            const int f = u.d_field[k][e];
            const int64_t cols = (f == D_GX || f == D_HX) ? u.nx : u.np;
            for (int64_t s = 0; s < n; ++s) if (u.d_j[k][(size_t)(e * n + s)] >= cols) ok = false;
        }
    }
    take(u.g_field, u.G, D_GYX, D_LGP + 1); take(u.g_i, u.G, 0, u.nx); take(u.g_j, u.G, 0, u.nx > u.np ? u.nx : u.np);
    if (ok && at + (int64_t)u.W * u.G <= words) {
        u.g_slots.assign(blob + at, blob + at + (int64_t)u.W * u.G); at += (int64_t)u.W * u.G;
        for (int32_t w : u.g_slots) if (w != -1 && (w < 0 || (w & ((1 << 29) - 1)) >= slots || (w >> 29) > 2)) ok = false;
    } else ok = false;
    take(u.obj_slots, u.n_obj, 0, slots);
    for (int g = 0; g < u.G && ok; ++g) if (u.g_j[g] >= (u.g_field[g] == D_LGP ? u.np : u.nx)) ok = false;
    return ok && at == words;
}

struct Segment { int cat; int64_t off, len; };

inline void add_segment(std::vector<Segment>& segs, int cat, int64_t off, int64_t len) {
    if (len <= 0) return;
    if (!segs.empty() && segs.back().cat == cat && segs.back().off + segs.back().len == off) { segs.back().len += len; return; }
    segs.push_back({cat, off, len});
}

// where (dest, i, j) lives: an offset from the destination's base, or -1
struct DenseLayout {
    int64_t ld, nx, ne, nc;
    int64_t operator()(int dest, int64_t i, int64_t j) const {
        switch (dest) {
        case D_GX: case D_HX: return i + j * ld;
        case D_LXX: return i + j * nx;
        case D_GP: return i + j * ne;
        case D_HP: return i + j * nc;
        case D_LGP: return i + j * nx;
        default: return -1;
        }
    }
};
struct BlockLayout {
    const calipso_device_block_data* o; double* base;
    std::vector<int> jrow, hcol;              // the block of every row of [equality; cone] and of every column of the Hessian (-1: none)
    explicit BlockLayout(const calipso_device_block_data* out) : o(out), base(nullptr) {
        jrow.assign((size_t)(o->ne + o->nc), -1); hcol.assign((size_t)o->nx, -1);
        for (int64_t b = 0; b < o->n_jacobian_blocks; ++b) {
            const calipso_device_block& k = o->jacobian_blocks[b];
            if (!base || k.values < base) base = k.values;
            for (int64_t r = k.row0; r < k.row0 + k.nrows; ++r) if (r >= 0 && r < o->ne + o->nc) jrow[(size_t)r] = (int)b;
        }
        for (int64_t b = 0; b < o->n_hessian_blocks; ++b) {
            const calipso_device_block& k = o->hessian_blocks[b];
            if (!base || k.values < base) base = k.values;
            for (int64_t c = k.col0; c < k.col0 + k.ncols; ++c) if (c >= 0 && c < o->nx) hcol[(size_t)c] = (int)b;
        }
    }
    int64_t in(const calipso_device_block& k, int64_t r, int64_t c) const {
        if (r < k.row0 || r >= k.row0 + k.nrows || c < k.col0 || c >= k.col0 + k.ncols) return -1;
        return (k.values - base) + (r - k.row0) + (c - k.col0) * k.ld;
    }
    int64_t operator()(int dest, int64_t i, int64_t j) const {
        switch (dest) {
        case D_GX: case D_HX: { const int64_t r = dest == D_GX ? i : i + o->ne; const int b = jrow[(size_t)r]; return b < 0 ? -1 : in(o->jacobian_blocks[b], r, j); }
        case D_LXX: { const int b = hcol[(size_t)j]; return b < 0 ? -1 : in(o->hessian_blocks[b], i, j); }
        case D_GP: return i + j * o->ne;
        case D_HP: return i + j * o->nc;
        case D_LGP: return i + j * o->nx;
        default: return -1;
        }
    }
};

// the stored patterns of a sparse handle (calipso_device_sparse_data: CSC, 1-based, rows ascending within a column): a non-zero's address is its position in the
// nzval array, found by binary search in its column; -1 where the pattern has no such entry.  D_GP, D_HP and D_LGP are addressed the same way in the stored parameter
// patterns (calipso_hip_sparse_kkt_set_parameter_patterns) when the handle has them; without them they have no destination on this route — the flags that would store
// through them are refused and their base is NULL — so they get address 0, which nothing stores through
struct SparseLayout {
    const calipso_device_sparse_data* o;
    bool parameters() const { return o->Lp_colptr && o->gp_colptr && o->hp_colptr; }
    static int64_t find(const int64_t* colptr, const int64_t* rowval, int64_t i, int64_t j) {
        int64_t lo = colptr[j] - 1, hi = colptr[j + 1] - 1;
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (rowval[mid] < i + 1) lo = mid + 1; else hi = mid;
        }
        return lo < colptr[j + 1] - 1 && rowval[lo] == i + 1 ? lo : -1;
    }
    int64_t operator()(int dest, int64_t i, int64_t j) const {
        switch (dest) {
        case D_GX: return find(o->gx_colptr, o->gx_rowval, i, j);
        case D_HX: return find(o->hx_colptr, o->hx_rowval, i, j);
        case D_LXX: return find(o->Lxx_colptr, o->Lxx_rowval, i, j);
        case D_GP: return parameters() ? find(o->gp_colptr, o->gp_rowval, i, j) : 0;
        case D_HP: return parameters() ? find(o->hp_colptr, o->hp_rowval, i, j) : 0;
        case D_LGP: return parameters() ? find(o->Lp_colptr, o->Lp_rowval, i, j) : 0;
        default: return -1;
        }
    }
};

struct RouteTable {                            // one layout of the destinations: the words to upload and where each table starts in them
    std::vector<int32_t> words;
    std::vector<int> vi, ri, pi, ad;           // per template
    int g_addr = 0, g_field = 0, g_slots = 0, obj_slots = 0, c_off = 0, c_len = 0;
    int fill_first[N_FILL] = {0}, fill_count[N_FILL] = {0};
};

// the index tables as they are, the address table and the finishing pass's addresses through `where`, the fill's chunks from `segs` (sorted by category)
template <class Where>
int build_table(const Shape& sh, const Tables& u, const Where& where, const std::vector<Segment>& segs, RouteTable& r) {
    std::vector<int32_t>& t = r.words;
    t.clear();
    auto put = [&](const std::vector<int32_t>& v) { const int at = (int)t.size(); t.insert(t.end(), v.begin(), v.end()); return at; };
    for (auto* v : {&r.vi, &r.ri, &r.pi, &r.ad}) v->assign((size_t)sh.nt, 0);
    for (int k = 0; k < sh.nt; ++k) {
        r.vi[k] = put(u.vi[k]); r.ri[k] = put(u.ri[k]); r.pi[k] = put(u.pi[k]);
        std::vector<int32_t> ad((size_t)sh.nd[k] * u.n[k]);
        for (int e = 0; e < sh.nd[k]; ++e)
            for (int s = 0; s < u.n[k]; ++s) {
                const size_t at = (size_t)e * u.n[k] + s;
                const int64_t off = where(u.d_field[k][e], u.d_i[k][at], u.d_j[k][at]);
                if (off < 0 || off > INT32_MAX) return 4;            // a non-zero outside the declared structure, or a destination beyond 2^31 entries
                ad[at] = (int32_t)off;
            }
        r.ad[k] = put(ad);
    }
    std::vector<int32_t> ga((size_t)u.G);
    for (int g = 0; g < u.G; ++g) {
        const int f = u.g_field[g];
        const int64_t off = (f == D_GYX || f == D_HZX) ? u.g_i[g] : where(f, u.g_i[g], u.g_j[g]);
        if (off < 0 || off > INT32_MAX) return 4;
        ga[g] = (int32_t)off;
    }
    r.g_addr = put(ga); r.g_field = put(u.g_field); r.g_slots = put(u.g_slots); r.obj_slots = put(u.obj_slots);
    std::vector<int32_t> c_off, c_len;
    int cat = -1;
    for (const Segment& sg : segs) {
        if (sg.cat < cat) return 5;
        while (cat < sg.cat) { ++cat; r.fill_first[cat] = (int)c_off.size(); r.fill_count[cat] = 0; }
        for (int64_t at = 0; at < sg.len; at += CHUNK) {
            if (sg.off + at > INT32_MAX) return 4;
            c_off.push_back((int32_t)(sg.off + at)); c_len.push_back((int32_t)(sg.len - at < CHUNK ? sg.len - at : CHUNK));
            ++r.fill_count[cat];
        }
    }
    while (cat < N_FILL - 1) { ++cat; r.fill_first[cat] = (int)c_off.size(); r.fill_count[cat] = 0; }
    r.c_off = put(c_off); r.c_len = put(c_len);
    return 0;
}

inline void add_parameter_segments(std::vector<Segment>& segs, const Tables& u) {
    add_segment(segs, 3, 0, (int64_t)u.ne * u.np); add_segment(segs, 4, 0, (int64_t)u.nc * u.np); add_segment(segs, 5, 0, (int64_t)u.nx * u.np);
}

inline int dense_route(const Shape& sh, const Tables& u, int64_t jacobian_ld, RouteTable& r) {
    if (jacobian_ld < u.ne + u.nc) return 1;
    std::vector<Segment> segs;
    for (int64_t j = 0; j < u.nx; ++j) add_segment(segs, 0, j * jacobian_ld, u.ne);
    for (int64_t j = 0; j < u.nx; ++j) add_segment(segs, 1, j * jacobian_ld, u.nc);
    add_segment(segs, 2, 0, (int64_t)u.nx * u.nx);
    add_parameter_segments(segs, u);
    return build_table(sh, u, DenseLayout{jacobian_ld, u.nx, u.ne, u.nc}, segs, r);
}

// *base: the lowest block's values, which the offsets of the Jacobians and of the Hessian count from
inline int block_route(const Shape& sh, const Tables& u, const calipso_device_block_data* out, RouteTable& r, double** base) {
    const BlockLayout where(out);
    std::vector<Segment> segs;
    for (int cat = 0; cat < 2; ++cat)                     // the equality rows of every Jacobian block, then the cone rows: column by column, merged where contiguous
        for (int64_t b = 0; b < out->n_jacobian_blocks; ++b) {
            const calipso_device_block& k = out->jacobian_blocks[b];
            const int64_t lo = cat == 0 ? k.row0 : (k.row0 > out->ne ? k.row0 : out->ne);
            const int64_t hi = cat == 0 ? (k.row0 + k.nrows < out->ne ? k.row0 + k.nrows : out->ne) : k.row0 + k.nrows;
            for (int64_t j = 0; j < k.ncols; ++j) add_segment(segs, cat, (k.values - where.base) + (lo - k.row0) + j * k.ld, hi - lo);
        }
    for (int64_t b = 0; b < out->n_hessian_blocks; ++b) {
        const calipso_device_block& k = out->hessian_blocks[b];
        for (int64_t j = 0; j < k.ncols; ++j) add_segment(segs, 2, (k.values - where.base) + j * k.ld, k.nrows);
    }
    add_parameter_segments(segs, u);
    *base = where.base;
    return build_table(sh, u, where, segs, r);
}

// a stored pattern as a route can address it: 1-based, column pointers from 1 to nnz + 1 without a decrease, rows in range, ascending and duplicate-free within a
// column (what the binary search of SparseLayout relies on), fewer than 2^31 non-zeros
inline bool sparse_pattern_ok(const int64_t* colptr, const int64_t* rowval, int64_t rows, int64_t cols, int64_t nnz) {
    if (nnz < 0 || nnz >= (int64_t)1 << 31 || rows < 0 || cols < 0 || !colptr || (nnz > 0 && !rowval) || colptr[0] != 1 || colptr[cols] != nnz + 1) return false;
    for (int64_t j = 0; j < cols; ++j) {
        if (colptr[j + 1] < colptr[j] || colptr[j + 1] > nnz + 1) return false;
        for (int64_t p = colptr[j] - 1; p < colptr[j + 1] - 1; ++p)
            if (rowval[p] < 1 || rowval[p] > rows || (p > colptr[j] - 1 && rowval[p - 1] >= rowval[p])) return false;
    }
    return true;
}

// the route of a sparse handle: one fill segment per nzval array; 1 for sizes that are not the tables' or a pattern sparse_pattern_ok refuses
inline int sparse_route(const Shape& sh, const Tables& u, const calipso_device_sparse_data* out, RouteTable& r) {
    if (!out || out->nx != u.nx || out->ne != u.ne || out->nc != u.nc || out->np != u.np) return 1;
    if (!sparse_pattern_ok(out->Lxx_colptr, out->Lxx_rowval, u.nx, u.nx, out->nnz_Lxx) || !sparse_pattern_ok(out->gx_colptr, out->gx_rowval, u.ne, u.nx, out->nnz_gx) ||
        !sparse_pattern_ok(out->hx_colptr, out->hx_rowval, u.nc, u.nx, out->nnz_hx)) return 1;
    std::vector<Segment> segs;
    add_segment(segs, 0, 0, out->nnz_gx); add_segment(segs, 1, 0, out->nnz_hx); add_segment(segs, 2, 0, out->nnz_Lxx);
    const SparseLayout where{out};
    if (where.parameters()) {                             // ... and one per stored parameter array
        if (!sparse_pattern_ok(out->gp_colptr, out->gp_rowval, u.ne, u.np, out->nnz_gp) || !sparse_pattern_ok(out->hp_colptr, out->hp_rowval, u.nc, u.np, out->nnz_hp) ||
            !sparse_pattern_ok(out->Lp_colptr, out->Lp_rowval, u.nx, u.np, out->nnz_Lp)) return 1;
        add_segment(segs, 3, 0, out->nnz_gp); add_segment(segs, 4, 0, out->nnz_hp); add_segment(segs, 5, 0, out->nnz_Lp);
    }
    return build_table(sh, u, where, segs, r);
}

}  // namespace trajectory
}  // namespace calipso
