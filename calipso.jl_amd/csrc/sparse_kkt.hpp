// sparse_kkt.hpp — the analysis behind the sparse search_direction! handle (sparse_kkt.hip) as plain host C++: no HIP header, no handle, so
// tests/sparse_kkt_host/main.cpp can build every table on the CPU under the sanitizers.  From nx, ne, nc, the cone layout and the CSC patterns of the
// Lagrangian Hessian Lxx (both triangles, as the reference holds it), of gx and of hx: the CSC pattern of triu(K) for the reference's
// jacobian_variables_symmetric (residual_jacobian_variables.jl:110-167; order idx.variables, idx.symmetric_equality, idx.symmetric_cone), the slot of
// K.nzval every input non-zero, every diagonal and every cone-block entry is written to, and a row view of each input pattern as a permutation of the
// caller's non-zero order, so that A v and A' v are both gathered per output entry without atomics and in a fixed summation order.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace calipso {
typedef int64_t i64;      // (as in calipso_options.hpp)
namespace sparse_kkt {

constexpr int REFUSED_ARGUMENT = -4;            // CALIPSO_ERR_ARGUMENT (sparse_kkt.hip asserts the value)

// the caller's CSC pattern, 0-based, and its row view: row r holds the columns col[ptr[r] .. ptr[r + 1]) ascending, src = position in the caller's nzval
struct ColView { std::vector<int> ptr, row; };
struct RowView { std::vector<int> ptr, col, src; };

struct Analysis {
    int status = 0; std::string message;        // status != 0: refused, nothing else is valid
    i64 nx = 0, ne = 0, nc = 0, n = 0, N = 0, n_nonnegative = 0, n_soc = 0, max_dim = 0, n_cone_columns = 0;
    std::vector<i64> colptr, rowval;            // triu(K), 1-based, rows ascending
    std::vector<int> slot_Lxx, slot_gx, slot_hx;                 // per input non-zero: its slot of K.nzval (0-based), -1 = not written (strict lower triangle of Lxx)
    std::vector<int> diag_x, diag_e, diag_c;                     // slot of the diagonal entry of every variable, equality and cone row
    std::vector<int> diag_x_src;                                 // the diagonal non-zero of Lxx in column j (position in the caller's nzval), -1 where the pattern has none
    std::vector<int> soc_start, soc_dim;                         // per second-order cone: first cone-local row, dimension
    std::vector<int> col_cone, col_index, col_slot;              // per (cone, column i): the cone, i, and the slot of block entry (0, i); rows 0 .. i follow contiguously
    ColView Lxx_cols, gx_cols, hx_cols;
    RowView Lxx_rows, gx_rows, hx_rows;
    i64 nnzK() const { return (i64)rowval.size(); }
};

// sorted, in range, duplicate-free, 1-based; fills the 0-based copy and the row view
inline bool read_pattern(const char* name, i64 rows, i64 cols, const i64* colptr, const i64* rowval, ColView& C, RowView& R, Analysis& a) {
    const std::string who = name;
    const auto refuse = [&](const std::string& text) { a.status = REFUSED_ARGUMENT; a.message = who + ": " + text; return false; };
    if (!colptr) return refuse("no column pointers");
    if (colptr[0] != 1) return refuse("colptr must be 1-based (Julia SparseMatrixCSC)");
    for (i64 c = 0; c < cols; ++c) if (colptr[c + 1] < colptr[c]) return refuse("colptr must be non-decreasing");
    const i64 nnz = colptr[cols] - 1;
    if (nnz > 0x7ffffff0) return refuse("more than 2^31 non-zeros");
    if (nnz > 0 && !rowval) return refuse("no row indices");
    C.ptr.assign((size_t)cols + 1, 0); C.row.resize((size_t)nnz);
    R.ptr.assign((size_t)rows + 1, 0); R.col.resize((size_t)nnz); R.src.resize((size_t)nnz);
    for (i64 c = 0; c < cols; ++c) {
        for (i64 p = colptr[c] - 1; p < colptr[c + 1] - 1; ++p) {
            const i64 r = rowval[p] - 1;
            if (r < 0 || r >= rows) return refuse("row index out of range");
            if (p > colptr[c] - 1 && rowval[p - 1] == rowval[p]) return refuse("duplicate entry in the CSC pattern");
            if (p > colptr[c] - 1 && rowval[p - 1] > rowval[p]) return refuse("row indices must ascend within a column");
            C.row[(size_t)p] = (int)r;
            ++R.ptr[(size_t)r + 1];
        }
        C.ptr[(size_t)c + 1] = (int)(colptr[c + 1] - 1);
    }
    for (i64 r = 0; r < rows; ++r) R.ptr[(size_t)r + 1] += R.ptr[(size_t)r];
    std::vector<int> next(R.ptr.begin(), R.ptr.end() - 1);
    for (i64 c = 0; c < cols; ++c)                       // columns in ascending order: every row's columns come out ascending
        for (int p = C.ptr[(size_t)c]; p < C.ptr[(size_t)c + 1]; ++p) {
            const int at = next[(size_t)C.row[(size_t)p]]++;
            R.col[(size_t)at] = (int)c; R.src[(size_t)at] = p;
        }
    return true;
}

// dims: n_soc dimensions >= 2 of contiguous cones after the n_nonnegative nonnegative rows (the layout calipso_hip_smallnewton_set_cones takes); no upper limit
inline Analysis analyse(i64 nx, i64 ne, i64 nc, i64 n_nonnegative, i64 n_soc, const i64* dims, const i64* Lxx_colptr, const i64* Lxx_rowval,
                        const i64* gx_colptr, const i64* gx_rowval, const i64* hx_colptr, const i64* hx_rowval) {
    Analysis a;
    const auto refuse = [&](const std::string& text) { a.status = REFUSED_ARGUMENT; a.message = text; return a; };
    if (nx < 1 || ne < 0 || nc < 0 || nx + ne + nc > 0x3fffffff) return refuse("nx >= 1, ne >= 0, nc >= 0 and nx + ne + nc < 2^30");
    if (n_nonnegative < 0 || n_nonnegative > nc || n_soc < 0 || (n_soc > 0 && !dims)) return refuse("the cone layout: 0 <= n_nonnegative <= nc, n_soc >= 0 with its dimensions");
    i64 used = n_nonnegative;
    for (i64 j = 0; j < n_soc; ++j) {
        if (dims[j] < 2) return refuse("a second-order cone has dimension >= 2 (cone " + std::to_string(j + 1) + " has " + std::to_string(dims[j]) + ")");
        if (dims[j] > nc - used) return refuse("the cone dimensions exceed nc = " + std::to_string(nc));
        used += dims[j];
    }
    a.nx = nx; a.ne = ne; a.nc = nc; a.n = nx + ne + nc; a.N = nx + 2 * ne + 3 * nc; a.n_nonnegative = n_nonnegative; a.n_soc = n_soc;
    if (!read_pattern("Lxx", nx, nx, Lxx_colptr, Lxx_rowval, a.Lxx_cols, a.Lxx_rows, a)) return a;
    if (!read_pattern("gx", ne, nx, gx_colptr, gx_rowval, a.gx_cols, a.gx_rows, a)) return a;
    if (!read_pattern("hx", nc, nx, hx_colptr, hx_rowval, a.hx_cols, a.hx_rows, a)) return a;
    // cone-local row -> rows of its block above the diagonal (0 for nonnegative rows and rows in no cone)
    std::vector<int> above((size_t)nc, 0);
    i64 start = n_nonnegative;
    for (i64 j = 0; j < n_soc; ++j) {
        a.soc_start.push_back((int)start); a.soc_dim.push_back((int)dims[j]);
        if (dims[j] > a.max_dim) a.max_dim = dims[j];
        for (i64 i = 0; i < dims[j]; ++i) { above[(size_t)(start + i)] = (int)i; a.col_cone.push_back((int)j); a.col_index.push_back((int)i); }
        start += dims[j];
    }
    a.n_cone_columns = (i64)a.col_cone.size();
    // ---- the columns of triu(K), in order
    const size_t nnzL = a.Lxx_cols.row.size(), nnzg = a.gx_cols.row.size(), nnzh = a.hx_cols.row.size();
    a.slot_Lxx.assign(nnzL, -1); a.slot_gx.assign(nnzg, -1); a.slot_hx.assign(nnzh, -1);
    a.diag_x.assign((size_t)nx, -1); a.diag_x_src.assign((size_t)nx, -1); a.diag_e.assign((size_t)ne, -1); a.diag_c.assign((size_t)nc, -1);
    a.col_slot.assign((size_t)a.n_cone_columns, -1);
    a.colptr.assign((size_t)a.n + 1, 1);
    const auto push = [&](i64 row) { a.rowval.push_back(row + 1); return (int)a.rowval.size() - 1; };
    for (i64 j = 0; j < nx; ++j) {                       // upper triangle of Lxx, the diagonal whether or not the pattern has it: ep lands there
        for (int p = a.Lxx_cols.ptr[(size_t)j]; p < a.Lxx_cols.ptr[(size_t)j + 1]; ++p) {
            const int r = a.Lxx_cols.row[(size_t)p];
            if (r > j) break;
            a.slot_Lxx[(size_t)p] = push(r);
            if (r == j) { a.diag_x[(size_t)j] = a.slot_Lxx[(size_t)p]; a.diag_x_src[(size_t)j] = p; }
        }
        if (a.diag_x[(size_t)j] < 0) a.diag_x[(size_t)j] = push(j);
        a.colptr[(size_t)j + 1] = (i64)a.rowval.size() + 1;
    }
    for (i64 e = 0; e < ne; ++e) {                       // gx' in the columns of its rows, then the equality diagonal
        for (int p = a.gx_rows.ptr[(size_t)e]; p < a.gx_rows.ptr[(size_t)e + 1]; ++p) a.slot_gx[(size_t)a.gx_rows.src[(size_t)p]] = push(a.gx_rows.col[(size_t)p]);
        a.diag_e[(size_t)e] = push(nx + e);
        a.colptr[(size_t)(nx + e) + 1] = (i64)a.rowval.size() + 1;
    }
    i64 cone_column = 0;
    for (i64 c = 0; c < nc; ++c) {                       // hx' likewise, then the rows <= c of the row's cone block (a diagonal entry for every row)
        for (int p = a.hx_rows.ptr[(size_t)c]; p < a.hx_rows.ptr[(size_t)c + 1]; ++p) a.slot_hx[(size_t)a.hx_rows.src[(size_t)p]] = push(a.hx_rows.col[(size_t)p]);
        const int up = above[(size_t)c];
        int first = -1;
        for (int i = up; i >= 0; --i) { const int s = push(nx + ne + c - i); if (first < 0) first = s; }
        a.diag_c[(size_t)c] = first + up;
        if (c >= n_nonnegative && c < used) a.col_slot[(size_t)cone_column++] = first;
        a.colptr[(size_t)(nx + ne + c) + 1] = (i64)a.rowval.size() + 1;
    }
    if (a.rowval.size() > 0x7ffffff0) return refuse("triu(K) has more than 2^31 non-zeros");
    return a;
}

}  // namespace sparse_kkt
}  // namespace calipso
