// sparse_solve.hpp — the host-side pieces of solve! on the sparse handle (sparse_solve.hip) that need no HIP and no handle: the filter as a value, the layout of
// the published scalar block, the item space of the kernels and the layout of their reduction workspace (every address the kernels store through that is not a
// plain row index), the names of the resident vectors, the argument checks of the entries.  Plain C++: tests/sparse_solve_host runs it on the CPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "step_decisions.hpp"              // filter_accepts, CONE_MASK_WORDS

namespace calipso {
namespace sparse_solve {

// ---- the filter (filter.jl:1-89) as a value -------------------------------------------------------------------------------------------------------------------
// reset (filter.jl:22-41), check (:43-50, through filter_accepts of step_decisions.hpp), augment (:52-79).  The reference's augment has no overflow guard and raises a
// BoundsError on a full filter; this one grows, as the dense handle's does (host_logic.hpp: augment_filter)
struct Filter {
    std::vector<double> theta, merit, cache_theta, cache_merit;
    i64 index = 0;
    explicit Filter(i64 capacity = 1000) { resize(capacity); }
    i64 capacity() const { return (i64)theta.size(); }
    void resize(i64 n) {
        if (n < 1) n = 1;
        theta.resize((size_t)n, 1.0e8); merit.resize((size_t)n, 1.0e8); cache_theta.resize((size_t)n, 1.0e8); cache_merit.resize((size_t)n, 1.0e8);
        if (index > n) index = n;
    }
    void reset() {
        for (i64 i = 0; i < index; ++i) { cache_theta[(size_t)i] = 1.0e8; cache_merit[(size_t)i] = 1.0e8; theta[(size_t)i] = 1.0e8; merit[(size_t)i] = 1.0e8; }
        index = 0;
    }
    bool accepts(double th, double m) const { return filter_accepts(theta.data(), merit.data(), capacity(), th, m); }
    void augment(double th, double m) {
        if (index >= capacity() && accepts(th, m)) resize(2 * capacity());      // every kept pair plus the new one must fit
        if (index == 0) { theta[0] = th; merit[0] = m; index = 1; return; }
        if (!accepts(th, m)) return;
        const i64 nold = index;
        for (i64 i = 0; i < nold; ++i) { cache_theta[(size_t)i] = theta[(size_t)i]; cache_merit[(size_t)i] = merit[(size_t)i]; theta[(size_t)i] = 1.0e8; merit[(size_t)i] = 1.0e8; }
        theta[0] = th; merit[0] = m; index = 1;
        for (i64 i = 0; i < nold; ++i)
            if (!(cache_theta[(size_t)i] >= th && cache_merit[(size_t)i] >= m)) { theta[(size_t)index] = cache_theta[(size_t)i]; merit[(size_t)index] = cache_merit[(size_t)i]; index += 1; }
    }
};

// ---- the published block: what the finishing kernels write and ONE copy brings to the host ----------------------------------------------------------------------
// doubles first; [8..15] are the eight norms in the positions step_norms() reads them at
enum Pub {
    PUB_OBJECTIVE = 0, PUB_BARRIER = 1, PUB_DUAL_DOT_R = 2, PUB_R_DOT_R = 3, PUB_MERIT = 4, PUB_THETA = 5, PUB_DD = 6,
    PUB_RES_1 = 8, PUB_RES_N_INF = 9, PUB_RES_Y_INF = 10, PUB_RES_Z_INF = 11, PUB_RES_T_INF = 12, PUB_Y_1 = 13, PUB_Z_1 = 14, PUB_T_1 = 15,
    PUB_G_INF = 16, PUB_PRODUCT_INF = 17,
    PUB_CAND_OBJECTIVE = 18, PUB_CAND_BARRIER = 19, PUB_CAND_MERIT = 20, PUB_CAND_THETA = 21,
    PUB_STEP_S = 22, PUB_STEP_T = 23, PUB_CONE_SEARCH_FAILED = 24,
    PUB_DOUBLES = 32
};
constexpr int PUB_MASK_INTS = 2 * CONE_MASK_WORDS;                      // slack masks, then slack-dual masks: behind the doubles
constexpr size_t PUB_BYTES = sizeof(double) * PUB_DOUBLES + sizeof(int) * PUB_MASK_INTS;
constexpr size_t PUB_ALLOC_DOUBLES = (PUB_BYTES + sizeof(double) - 1) / sizeof(double);

// ---- item space and reduction workspace -------------------------------------------------------------------------------------------------------------------------
constexpr int THREADS = 256, WAVE = 64;
constexpr int GRID_CAP = 512;              // workgroups of a kernel at the most: beyond, the threads stride over the items
constexpr int SMALL_CONE_MAX = 16;         // a second-order cone up to this dimension is one thread's, a wider one a wavefront's

// partial sums (or maxima) per kernel: one double per (quantity, workgroup)
enum ProloguePartial { PP_OBJECTIVE, PP_DUAL_DOT_R, PP_R_DOT_R, PP_BARRIER, PP_THETA, PP_RES_1, PP_Y_1, PP_Z_1, PP_T_1, PP_RES_N_INF, PP_RES_Y_INF, PP_RES_Z_INF, PP_RES_T_INF, PP_COUNT };
constexpr int PP_FIRST_MAX = PP_RES_N_INF;
enum CandidatePartial { CP_OBJECTIVE, CP_DUAL_DOT_R, CP_R_DOT_R, CP_BARRIER, CP_THETA, CP_DD, CP_COUNT };
enum AcceptPartial { AP_G_INF, AP_PRODUCT_INF, AP_COUNT };

inline i64 round_up(i64 v, i64 m) { return (v + m - 1) / m * m; }

// Items of every grid kernel: [0, rows) one thread per row of [x; equality; cone]; [small0, small0 + n_small) one thread per small second-order cone;
// [wide0, wide0 + 64 n_wide) one wavefront per wide cone.  The sections begin at multiples of 64, so a wavefront never spans two of them.
struct Layout {
    i64 rows = 0, n_small = 0, n_wide = 0, small0 = 0, wide0 = 0, items = 0;
    int grid = 1;
    i64 off_prologue = 0, off_candidate = 0, off_accept = 0, doubles = 0;      // partial q of workgroup b: off + q * grid + b
    i64 mask_ints = 0;                                                         // word m of workgroup b: m * grid + b
    i64 prologue(int q, int b) const { return off_prologue + (i64)q * grid + b; }
    i64 candidate(int q, int b) const { return off_candidate + (i64)q * grid + b; }
    i64 accept(int q, int b) const { return off_accept + (i64)q * grid + b; }
    i64 mask(int m, int b) const { return (i64)m * grid + b; }
};
inline Layout layout(i64 nx, i64 ne, i64 nc, i64 n_small, i64 n_wide) {
    Layout l;
    l.rows = nx + ne + nc; l.n_small = n_small; l.n_wide = n_wide;
    l.small0 = round_up(l.rows, WAVE);
    l.wide0 = round_up(l.small0 + n_small, WAVE);
    l.items = l.wide0 + (i64)WAVE * n_wide;
    l.grid = (int)std::min<i64>(GRID_CAP, std::max<i64>(1, (l.items + THREADS - 1) / THREADS));
    l.off_prologue = 0;
    l.off_candidate = l.off_prologue + (i64)PP_COUNT * l.grid;
    l.off_accept = l.off_candidate + (i64)CP_COUNT * l.grid;
    l.doubles = l.off_accept + (i64)AP_COUNT * l.grid;
    l.mask_ints = (i64)PUB_MASK_INTS * l.grid;
    return l;
}

// ---- the resident vectors by their reference names (solver.jl, problem data) -----------------------------------------------------------------------------------
enum Vector { V_SOLUTION, V_CANDIDATE, V_DUAL, V_RESIDUAL, V_MERIT_GRADIENT, V_STEP, V_CONE_PRODUCT, V_CONE_TARGET, V_BARRIER_GRADIENT, V_EQUALITY_CONSTRAINT,
              V_CONE_CONSTRAINT, V_OBJECTIVE_GRADIENT_VARIABLES, V_COUNT,
              // not a vector of the reference's solver: the s, t that differentiate! forms the cone blocks at (sparse_differentiate.hip), s then t; read only
              V_DIFFERENTIATE_SLACKS = V_COUNT,
              // ... nor these: the evaluator's objective at the solution (1) and the three resident non-zero arrays on their stored patterns; read only
              V_OBJECTIVE, V_LAGRANGIAN_HESSIAN, V_EQUALITY_JACOBIAN_VARIABLES, V_CONE_JACOBIAN_VARIABLES, V_NAMED };
inline const char* vector_name(int v) {
    static const char* const names[V_NAMED] = {"solution", "candidate", "dual", "residual", "merit_gradient", "step", "cone_product", "cone_target", "barrier_gradient",
                                               "equality_constraint", "cone_constraint", "objective_gradient_variables", "differentiate_slacks",
                                               "objective", "lagrangian_hessian", "equality_jacobian_variables", "cone_jacobian_variables"};
    return v >= 0 && v < V_NAMED ? names[v] : "";
}
inline int vector_by_name(const char* name) {
    if (name) for (int v = 0; v < V_NAMED; ++v) if (!std::strcmp(name, vector_name(v))) return v;
    return -1;
}
inline i64 vector_length(int v, i64 nx, i64 ne, i64 nc, const i64* nnz = nullptr) {      // nnz: the non-zeros of Lxx, gx, hx (the three matrices have no length without)
    switch (v) {
        case V_OBJECTIVE: return 1;
        case V_LAGRANGIAN_HESSIAN: case V_EQUALITY_JACOBIAN_VARIABLES: case V_CONE_JACOBIAN_VARIABLES: return nnz ? nnz[v - V_LAGRANGIAN_HESSIAN] : -1;
        case V_SOLUTION: case V_CANDIDATE: case V_RESIDUAL: case V_STEP: return nx + 2 * ne + 3 * nc;
        case V_DUAL: case V_EQUALITY_CONSTRAINT: return ne;
        case V_MERIT_GRADIENT: return nx + ne + nc;
        case V_CONE_PRODUCT: case V_CONE_TARGET: case V_BARRIER_GRADIENT: case V_CONE_CONSTRAINT: return nc;
        case V_OBJECTIVE_GRADIENT_VARIABLES: return nx;
        case V_DIFFERENTIATE_SLACKS: return 2 * nc;
        default: return -1;
    }
}

// ---- argument checks: an empty string, or the refusal's text (the entry returns CALIPSO_ERR_ARGUMENT with it) ---------------------------------------------------
constexpr i64 TRACE_ROWS_MAX = 1 << 20;
inline std::string check_named_vector(const char* entry, const char* name, const void* data, i64 len, i64 nx, i64 ne, i64 nc, bool writable_only, const i64* nnz = nullptr) {
    const int v = vector_by_name(name);
    if (v < 0) return std::string(entry) + ": name: no resident vector called " + (name ? name : "(null)");
    if (writable_only && v != V_SOLUTION && v != V_DUAL && v != V_STEP) return std::string(entry) + ": name: only solution, dual and step can be set, not " + name;
    const i64 want = vector_length(v, nx, ne, nc, nnz);
    if (len != want) return std::string(entry) + ": len: " + name + " has " + std::to_string(want) + " entries, not " + std::to_string(len);
    if (!data && want > 0) return std::string(entry) + ": the array is NULL";
    return "";
}
inline std::string check_keep_trace(i64 rows) {
    if (rows < 1 || rows > TRACE_ROWS_MAX) return "calipso_hip_sparse_kkt_keep_trace: rows: 1 .. " + std::to_string(TRACE_ROWS_MAX) + " rows can be kept, not " + std::to_string(rows);
    return "";
}
inline std::string check_trace(const void* out, i64 cap_rows) {
    if (cap_rows < 0) return "calipso_hip_sparse_kkt_trace: cap_rows is negative";
    if (!out && cap_rows > 0) return "calipso_hip_sparse_kkt_trace: out is NULL with cap_rows > 0";
    return "";
}
// ---- the evaluator's entries ------------------------------------------------------------------------------------------------------------------------------------
// the bits calipso_hip_sparse_kkt_evaluate may carry: no dual gradient (the handle gathers them), no parameter Jacobian (those are evaluate_parameters' and the
// _parameters entries' of differentiate!, on the stored patterns of sparse_parameters.hpp)
constexpr uint32_t EVAL_DUAL_GRADIENTS = (1u << 5) | (1u << 9);
constexpr uint32_t EVAL_PARAMETER_BITS = 0x1fu << 11;
constexpr uint32_t EVAL_MATRIX_BITS[3] = {(1u << 2) | (1u << 6) | (1u << 10), 1u << 4, 1u << 8};      // what writes Lxx, gx, hx
constexpr uint32_t EVAL_POINT = (1u << 0) | (1u << 3) | (1u << 7);                                    // objective, equality, cone: what a candidate asks for
constexpr uint32_t EVAL_EVERYTHING = EVAL_POINT | (1u << 1) | EVAL_MATRIX_BITS[0] | EVAL_MATRIX_BITS[1] | EVAL_MATRIX_BITS[2];
inline std::string check_evaluate(int which, uint32_t flags) {
    static const char* const entry = "calipso_hip_sparse_kkt_evaluate";
    if (which != 0 && which != 1) return std::string(entry) + ": which: 0 the solution, 1 the candidate, not " + std::to_string(which);
    if (flags & EVAL_PARAMETER_BITS) return std::string(entry) + ": flags: parameter-Jacobian bits " + std::to_string(flags & EVAL_PARAMETER_BITS) +
                                            ": the sparse handle asks its evaluator for no parameter Jacobian; differentiate takes the caller's dR/dtheta";
    if (flags & EVAL_DUAL_GRADIENTS) return std::string(entry) + ": flags: a dual-gradient bit: (g'y)x and (h'z)x are formed by the handle from its column views, the evaluator has no destination for them";
    if (flags >> 16) return std::string(entry) + ": flags: bits beyond CALIPSO_EVAL_CONE_DUAL_JACOBIAN_PARAMETERS";
    if (!flags) return std::string(entry) + ": flags: nothing asked for";
    return "";
}
inline std::string check_set_evaluator(i64 np) {
    if (np < 0 || np > 0x7ffffff0) return "calipso_hip_sparse_kkt_set_evaluator: np: " + std::to_string(np) + " parameters";
    return "";
}
inline std::string check_set_parameters(const char* entry, bool evaluator, i64 np, const void* theta) {
    if (!evaluator) return std::string(entry) + ": no evaluator attached (calipso_hip_sparse_kkt_set_evaluator first): a QP has no parameters";
    if (!theta && np > 0) return std::string(entry) + ": theta is NULL, the evaluator takes " + std::to_string(np) + " parameters";
    return "";
}
inline std::string check_step_sizes(const char* entry, double a_s, double a_t) {
    if (!(a_s > 0.0 && a_s <= 1.0)) return std::string(entry) + ": a_s: a step size lies in (0, 1]";
    if (!(a_t > 0.0 && a_t <= 1.0)) return std::string(entry) + ": a_t: a step size lies in (0, 1]";
    return "";
}

}  // namespace sparse_solve
}  // namespace calipso
