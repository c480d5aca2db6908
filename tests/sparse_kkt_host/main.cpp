// The analysis of the sparse search_direction! handle on the CPU: analyses one case (a text file written by tests/test_sparse_kkt_cpu.py: sizes, cone layout,
// the three CSC patterns) with calipso.jl_amd/csrc/sparse_kkt.hpp and checks every table by brute force: the pattern of triu(K) against one rebuilt from dense
// 0/1 masks, every slot map by a round trip to (row, column), the row views against the column views.  Prints the sizes, then "sparse kkt ok"; a refusal is
// printed with its status and text.  Built by the host compiler under the address and undefined-behaviour sanitizers; no HIP.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../calipso.jl_amd/csrc/sparse_kkt.hpp"

using namespace calipso::sparse_kkt;
using calipso::i64;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

struct Pattern { std::vector<i64> colptr, rowval; };
struct Case { i64 nx = 0, ne = 0, nc = 0, q = 0; std::vector<i64> dims; Pattern L, g, h; };

static Case read_case(const char* path) {
    std::ifstream in(path);
    CHECK(in.good());
    Case c; std::string key;
    auto list = [&](std::vector<i64>& v) { size_t k; in >> k; v.resize(k); for (auto& x : v) in >> x; };
    while (in >> key) {
        if (key == "nx") in >> c.nx; else if (key == "ne") in >> c.ne; else if (key == "nc") in >> c.nc; else if (key == "nonnegative") in >> c.q;
        else if (key == "dims") list(c.dims);
        else if (key == "Lxx_colptr") list(c.L.colptr); else if (key == "Lxx_rowval") list(c.L.rowval);
        else if (key == "gx_colptr") list(c.g.colptr); else if (key == "gx_rowval") list(c.g.rowval);
        else if (key == "hx_colptr") list(c.h.colptr); else if (key == "hx_rowval") list(c.h.rowval);
        else CHECK(!"unknown key");
    }
    return c;
}

typedef std::vector<std::vector<char>> Mask;
static Mask dense_mask(i64 rows, i64 cols, const Pattern& p) {
    Mask M((size_t)rows, std::vector<char>((size_t)cols, 0));
    for (i64 c = 0; c < cols; ++c) for (i64 k = p.colptr[(size_t)c] - 1; k < p.colptr[(size_t)c + 1] - 1; ++k) M[(size_t)p.rowval[(size_t)k] - 1][(size_t)c] = 1;
    return M;
}

// a row view against its pattern: a permutation of the non-zeros, every row's columns ascending, every entry where its source is
static void check_views(i64 rows, i64 cols, const Pattern& p, const ColView& C, const RowView& R) {
    const size_t nnz = p.rowval.size();
    CHECK(C.ptr.size() == (size_t)cols + 1 && C.row.size() == nnz && R.ptr.size() == (size_t)rows + 1 && R.col.size() == nnz && R.src.size() == nnz);
    for (i64 c = 0; c <= cols; ++c) CHECK(C.ptr[(size_t)c] == p.colptr[(size_t)c] - 1);
    for (size_t k = 0; k < nnz; ++k) CHECK(C.row[k] == p.rowval[k] - 1);
    std::vector<int> column_of(nnz, -1);
    for (i64 c = 0; c < cols; ++c) for (int k = C.ptr[(size_t)c]; k < C.ptr[(size_t)c + 1]; ++k) column_of[(size_t)k] = (int)c;
    std::vector<char> seen(nnz, 0);
    CHECK(R.ptr[0] == 0 && R.ptr[(size_t)rows] == (int)nnz);
    for (i64 r = 0; r < rows; ++r) {
        CHECK(R.ptr[(size_t)r] <= R.ptr[(size_t)r + 1]);
        for (int k = R.ptr[(size_t)r]; k < R.ptr[(size_t)r + 1]; ++k) {
            const int src = R.src[(size_t)k];
            CHECK(src >= 0 && (size_t)src < nnz && !seen[(size_t)src]);
            seen[(size_t)src] = 1;
            CHECK(C.row[(size_t)src] == r && column_of[(size_t)src] == R.col[(size_t)k]);
            if (k > R.ptr[(size_t)r]) CHECK(R.col[(size_t)k - 1] < R.col[(size_t)k]);
        }
    }
}

int main(int argc, char** argv) {
    CHECK(argc == 2);
    const Case c = read_case(argv[1]);
    const Analysis a = analyse(c.nx, c.ne, c.nc, c.q, (i64)c.dims.size(), c.dims.data(), c.L.colptr.data(), c.L.rowval.data(), c.g.colptr.data(), c.g.rowval.data(),
                               c.h.colptr.data(), c.h.rowval.data());
    if (a.status) { std::printf("refused %d %s\n", a.status, a.message.c_str()); return 0; }
    const i64 nx = c.nx, ne = c.ne, nc = c.nc, n = nx + ne + nc;
    CHECK(a.n == n && a.N == nx + 2 * ne + 3 * nc && a.nx == nx && a.ne == ne && a.nc == nc);
    // ---- triu(K) rebuilt from dense masks
    const Mask L = dense_mask(nx, nx, c.L), G = dense_mask(ne, nx, c.g), H = dense_mask(nc, nx, c.h);
    Mask K((size_t)n, std::vector<char>((size_t)n, 0));
    for (i64 i = 0; i < nx; ++i) for (i64 j = i; j < nx; ++j) K[(size_t)i][(size_t)j] = L[(size_t)i][(size_t)j] || i == j;
    for (i64 e = 0; e < ne; ++e) { for (i64 j = 0; j < nx; ++j) K[(size_t)j][(size_t)(nx + e)] = G[(size_t)e][(size_t)j]; K[(size_t)(nx + e)][(size_t)(nx + e)] = 1; }
    for (i64 r = 0; r < nc; ++r) { for (i64 j = 0; j < nx; ++j) K[(size_t)j][(size_t)(nx + ne + r)] = H[(size_t)r][(size_t)j]; K[(size_t)(nx + ne + r)][(size_t)(nx + ne + r)] = 1; }
    i64 start = c.q, max_dim = 0, columns = 0;
    for (i64 d : c.dims) {
        for (i64 i = 0; i < d; ++i) for (i64 j = i; j < d; ++j) K[(size_t)(nx + ne + start + i)][(size_t)(nx + ne + start + j)] = 1;
        start += d; columns += d; if (d > max_dim) max_dim = d;
    }
    CHECK(a.max_dim == max_dim && a.n_cone_columns == columns && a.n_soc == (i64)c.dims.size() && a.n_nonnegative == c.q);
    CHECK((i64)a.colptr.size() == n + 1 && a.colptr[0] == 1);
    std::vector<std::pair<int, int>> at;                                                     // (row, column) of every slot
    for (i64 j = 0; j < n; ++j) {
        std::vector<i64> want;
        for (i64 i = 0; i <= j; ++i) if (K[(size_t)i][(size_t)j]) want.push_back(i + 1);
        CHECK(a.colptr[(size_t)j + 1] - a.colptr[(size_t)j] == (i64)want.size());
        for (size_t k = 0; k < want.size(); ++k) { CHECK(a.rowval[(size_t)(a.colptr[(size_t)j] - 1) + k] == want[k]); at.push_back({(int)want[k] - 1, (int)j}); }
    }
    CHECK((i64)at.size() == a.nnzK() && a.colptr[(size_t)n] - 1 == a.nnzK());
    // ---- every map, round trip: each slot of K is written by exactly one source
    std::vector<int> writers(at.size(), 0);
    const auto slot_is = [&](int slot, i64 row, i64 col) { CHECK(slot >= 0 && (size_t)slot < at.size() && at[(size_t)slot].first == row && at[(size_t)slot].second == col); };
    CHECK(a.slot_Lxx.size() == c.L.rowval.size() && a.slot_gx.size() == c.g.rowval.size() && a.slot_hx.size() == c.h.rowval.size());
    CHECK((i64)a.diag_x.size() == nx && (i64)a.diag_x_src.size() == nx && (i64)a.diag_e.size() == ne && (i64)a.diag_c.size() == nc);
    for (i64 j = 0; j < nx; ++j)
        for (i64 k = c.L.colptr[(size_t)j] - 1; k < c.L.colptr[(size_t)j + 1] - 1; ++k) {
            const i64 r = c.L.rowval[(size_t)k] - 1;
            if (r > j) { CHECK(a.slot_Lxx[(size_t)k] == -1); continue; }
            slot_is(a.slot_Lxx[(size_t)k], r, j);
            if (r < j) ++writers[(size_t)a.slot_Lxx[(size_t)k]];
            else CHECK(a.diag_x_src[(size_t)j] == k && a.diag_x[(size_t)j] == a.slot_Lxx[(size_t)k]);
        }
    for (i64 j = 0; j < nx; ++j) {
        slot_is(a.diag_x[(size_t)j], j, j); ++writers[(size_t)a.diag_x[(size_t)j]];
        if (!L[(size_t)j][(size_t)j]) CHECK(a.diag_x_src[(size_t)j] == -1);
    }
    for (i64 j = 0; j < nx; ++j) {
        for (i64 k = c.g.colptr[(size_t)j] - 1; k < c.g.colptr[(size_t)j + 1] - 1; ++k) { slot_is(a.slot_gx[(size_t)k], j, nx + c.g.rowval[(size_t)k] - 1); ++writers[(size_t)a.slot_gx[(size_t)k]]; }
        for (i64 k = c.h.colptr[(size_t)j] - 1; k < c.h.colptr[(size_t)j + 1] - 1; ++k) { slot_is(a.slot_hx[(size_t)k], j, nx + ne + c.h.rowval[(size_t)k] - 1); ++writers[(size_t)a.slot_hx[(size_t)k]]; }
    }
    for (i64 e = 0; e < ne; ++e) { slot_is(a.diag_e[(size_t)e], nx + e, nx + e); ++writers[(size_t)a.diag_e[(size_t)e]]; }
    for (i64 r = 0; r < nc; ++r) slot_is(a.diag_c[(size_t)r], nx + ne + r, nx + ne + r);
    for (i64 r = 0; r < c.q; ++r) ++writers[(size_t)a.diag_c[(size_t)r]];                     // nonnegative rows ...
    for (i64 r = c.q + columns; r < nc; ++r) ++writers[(size_t)a.diag_c[(size_t)r]];           // ... and rows in no cone: their diagonal item
    CHECK((i64)a.col_cone.size() == columns && (i64)a.col_index.size() == columns && (i64)a.col_slot.size() == columns);
    CHECK(a.soc_start.size() == c.dims.size() && a.soc_dim.size() == c.dims.size());
    i64 e = 0; start = c.q;
    for (size_t j = 0; j < c.dims.size(); ++j) {
        CHECK(a.soc_start[j] == start && a.soc_dim[j] == c.dims[j]);
        for (i64 i = 0; i < c.dims[j]; ++i, ++e) {
            CHECK(a.col_cone[(size_t)e] == (int)j && a.col_index[(size_t)e] == i);
            for (i64 r = 0; r <= i; ++r) { slot_is(a.col_slot[(size_t)e] + (int)r, nx + ne + start + r, nx + ne + start + i); ++writers[(size_t)(a.col_slot[(size_t)e] + r)]; }
            CHECK(a.diag_c[(size_t)(start + i)] == a.col_slot[(size_t)e] + i);
        }
        start += c.dims[j];
    }
    for (size_t k = 0; k < writers.size(); ++k) CHECK(writers[k] == 1);
    check_views(nx, nx, c.L, a.Lxx_cols, a.Lxx_rows);
    check_views(ne, nx, c.g, a.gx_cols, a.gx_rows);
    check_views(nc, nx, c.h, a.hx_cols, a.hx_rows);
    std::printf("sizes n=%lld N=%lld nnzK=%lld cone_columns=%lld max_dim=%lld\nsparse kkt ok\n", (long long)n, (long long)a.N, (long long)a.nnzK(), (long long)columns, (long long)max_dim);
    return 0;
}
