// sparse_parameters.hpp — the host side of the parameter Jacobians on the sparse handle (sparse_solve.hip: set_parameter_patterns, evaluate_parameters;
// sparse_differentiate.hip: differentiate_parameters, differentiate_adjoint_parameters): the checks of the three stored patterns and of a column selection, the
// split of the parameters into short and long columns and the launch geometry of the two kernels that walk them.  Plain C++, no HIP, no handle:
// tests/sparse_parameters_host/main.cpp runs it on the CPU under the sanitizers.
//
// dR/dtheta (residual_jacobian_parameters.jl:1-40) has three non-zero blocks: Lx,theta in the x rows, g,theta in the y rows, h,theta in the z rows.  The handle keeps
// them as values on three CSC patterns with np columns — nothing of size N x np, nx x np, ne x np or nc x np exists.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/calipso_trajectory_tables.hpp"   // sparse_pattern_ok: the rule the patterns given to a route are checked by

namespace calipso {
namespace sparse_parameters {

constexpr int WAVE = 64, THREADS = 256;
// A parameter whose column holds at least this many non-zeros (over the three arrays) is a wavefront's in the gradient kernel, a shorter one a thread's.
// UNMEASURED: 64 is the length from which every lane of a wavefront has an entry of its own; nobody has timed other values on the hardware.
constexpr int SPLIT_LENGTH = 64;
constexpr int64_t COLUMNS_MAX = 65535;      // blockIdx.y carries the column (sparse_differentiate.hpp: COLUMNS_MAX)

inline const char* array_name(int m) {
    static const char* const names[3] = {"lagrangian_gradient_parameters", "equality_jacobian_parameters", "cone_jacobian_parameters"};
    return m >= 0 && m < 3 ? names[m] : "";
}
inline int array_by_name(const char* name) {
    if (name) for (int m = 0; m < 3; ++m) if (std::string(name) == array_name(m)) return m;
    return -1;
}

// the three patterns as the caller hands them in: 1-based CSC with np columns, rows ascending and duplicate-free within a column
struct Patterns { const int64_t* colptr[3]; const int64_t* rowval[3]; };

// an empty string, or the refusal's text naming the array (Lp_*, gp_*, hp_*)
inline std::string check_patterns(const char* entry, int64_t np, const int64_t rows[3], const Patterns& p) {
    static const char* const pre[3] = {"Lp", "gp", "hp"};
    if (np < 1) return std::string(entry) + ": the evaluator has no parameters (np = " + std::to_string(np) + ")";
    for (int m = 0; m < 3; ++m) {
        if (!p.colptr[m]) return std::string(entry) + ": " + pre[m] + "_colptr is NULL";
        if (p.colptr[m][0] != 1) return std::string(entry) + ": " + pre[m] + "_colptr: the first column pointer is " + std::to_string(p.colptr[m][0]) + ", not 1 (the patterns are 1-based)";
        const int64_t nnz = p.colptr[m][np] - 1;
        if (nnz < 0 || nnz >= (int64_t)1 << 31) return std::string(entry) + ": " + pre[m] + "_colptr: " + std::to_string(nnz) + " non-zeros";
        for (int64_t j = 0; j < np; ++j)
            if (p.colptr[m][j + 1] < p.colptr[m][j] || p.colptr[m][j + 1] > nnz + 1)
                return std::string(entry) + ": " + pre[m] + "_colptr: column " + std::to_string(j + 1) + " ends at " + std::to_string(p.colptr[m][j + 1]) + " (pointers must not decrease nor pass nnz + 1)";
        if (nnz > 0 && !p.rowval[m]) return std::string(entry) + ": " + pre[m] + "_rowval is NULL";
        if (!trajectory::sparse_pattern_ok(p.colptr[m], p.rowval[m], rows[m], np, nnz))
            return std::string(entry) + ": " + pre[m] + "_rowval: rows lie in 1 .. " + std::to_string(rows[m]) + ", ascending and without duplicates within a column";
    }
    return "";
}

// a column selection: k 1-based parameter indices (repeats allowed), or NULL for all np parameters
inline std::string check_selection(const char* entry, int64_t np, int64_t k, const int64_t* columns) {
    if (k < 1) return std::string(entry) + ": k: at least one column, not " + std::to_string(k);
    if (k > COLUMNS_MAX) return std::string(entry) + ": k: at most " + std::to_string(COLUMNS_MAX) + " columns in one call (the multi-column solve's grid limit), not " + std::to_string(k);
    if (!columns) {
        if (k != np) return std::string(entry) + ": k: columns = NULL selects all " + std::to_string(np) + " parameters, k is " + std::to_string(k);
        return "";
    }
    for (int64_t c = 0; c < k; ++c)
        if (columns[c] < 1 || columns[c] > np)
            return std::string(entry) + ": columns[" + std::to_string(c) + "] = " + std::to_string(columns[c]) + " is no parameter index (1 .. " + std::to_string(np) + ")";
    return "";
}

// ---- short and long columns ---------------------------------------------------------------------------------------------------------------------------------------
inline bool is_long(int64_t length) { return length >= SPLIT_LENGTH; }

struct Split {
    std::vector<int32_t> long_columns;      // 0-based, ascending: the parameters a wavefront sums
    int64_t longest = 0;                    // non-zeros of the longest column over the three arrays: the scatter's item count per column
};
inline Split split_columns(int64_t np, const Patterns& p) {
    Split s;
    for (int64_t j = 0; j < np; ++j) {
        int64_t len = 0;
        for (int m = 0; m < 3; ++m) len += p.colptr[m][j + 1] - p.colptr[m][j];
        if (len > s.longest) s.longest = len;
        if (is_long(len)) s.long_columns.push_back((int32_t)j);
    }
    return s;
}

// the gradient kernel's items per cotangent column: [0, np) one thread per parameter (a long one's thread returns at once), [long0, long0 + 64 n_long) one
// wavefront per long parameter.  long0 is a multiple of 64, so a wavefront never spans the two sections
struct Geometry { int64_t long0 = 0, items = 0; unsigned blocks = 1; };
inline Geometry geometry(int64_t np, int64_t n_long) {
    Geometry g;
    g.long0 = (np + WAVE - 1) / WAVE * WAVE;
    g.items = g.long0 + (int64_t)WAVE * n_long;
    g.blocks = (unsigned)((g.items + THREADS - 1) / THREADS);
    if (g.blocks < 1) g.blocks = 1;
    return g;
}
// the scatter of selected columns of dR/dtheta into V: one thread per (entry of the column, selected column)
inline unsigned scatter_blocks(int64_t longest) { const int64_t b = (longest + THREADS - 1) / THREADS; return (unsigned)(b < 1 ? 1 : b); }

}  // namespace sparse_parameters
}  // namespace calipso
