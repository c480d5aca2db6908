// step_decisions.hpp — every decision the host takes inside a Newton step and between the steps of a solve, as free functions on values: the ONE copy that the
// single-handle driver (api.hip), the group driver (group.hip) and the sparse handle's drivers (sparse_kkt.hip, sparse_solve.hip; for groups sparse_kkt_group.hpp) all call.  Plain C++ (no HIP, no handle, no device, no error string): tests/step_decisions runs it
// on the CPU.  Every floating-point expression is the reference's, operand order and parentheses included — the drivers' results are compared bit for bit.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/calipso_options.hpp"     // calipso::i64, calipso::Options

namespace calipso {

constexpr int CONE_MASK_WORDS = 26;                     // icount[6..31] (slack) and icount[32..57] (slack dual): one bit per trial step size
constexpr int CONE_MASK_TRIALS = 32 * CONE_MASK_WORDS;  // => max_cone_line_search <= 831

// scalars the host owns and passes to kernels by value (solver.jl:81-127)
struct Scalars { double kappa = 0.1, tau = 0.99, rho = 10.0, ep = 0.0, ep_last = 0.0, ed = 0.0; };

// ---- the norms of the exit tests, from the read-back hs = hscal (hs[8..15]: vectors.hip: k_violations) ------------------------------------------------------
struct StepNorms { double residual_violation, optimality, slack_violation; };
inline StepNorms step_norms(const double* hs, i64 N, i64 ne, i64 nc) {
    const double sd = (ne + nc > 0) ? std::max(100.0, (hs[13] + hs[14]) / (double)(ne + nc)) / 100.0 : 1.0;   // optimality_error.jl:8
    const double scn = (nc > 0) ? std::max(100.0, hs[15] / (double)nc) / 100.0 : 1.0;                         // :9
    return {hs[8] / (double)N, std::max(std::max(hs[9] / sd, hs[10]), std::max(hs[11], hs[12] / scn)), std::max(hs[10], hs[11])};
}
// what the optimality error is compared with at solve.jl:165
inline double inner_exit_threshold(const Options& o, double kappa) { return std::max(o.central_path_update_tolerance * kappa, o.optimality_tolerance); }
// 0: go on to a search direction, 1: outer convergence (solve.jl:138-143), 2: inner convergence (:165).  test_outer = false: a benchmark step, which has no violations
// of an earlier step to test
inline int exit_kind(const Options& o, double kappa, const StepNorms& n, double equality_violation, double cone_product_violation, bool test_outer) {
    if (test_outer && n.residual_violation < o.residual_tolerance && n.slack_violation < o.slack_tolerance &&
        equality_violation <= o.equality_tolerance && cone_product_violation <= o.complementarity_tolerance) return 1;
    return n.optimality <= inner_exit_threshold(o, kappa) ? 2 : 0;
}

// ---- cone search (solve.jl:190-221) -------------------------------------------------------------------------------------------------------------------------
// first trial index k in 0..max_cone_line_search whose violation bit is clear (cones.hip: violation_masks), -1 if none: the
// reference raises "cone search failure" once cone_iteration exceeds max_cone_line_search (solve.jl:204-221)
inline int first_feasible_trial(const int* mask, i64 max_cone_line_search) {
    const int nk = (int)std::min<i64>(max_cone_line_search + 1, CONE_MASK_TRIALS);
    for (int k = 0; k < nk; ++k) if (!(mask[k >> 5] & (1 << (k & 31)))) return k;
    return -1;
}
// step sizes as the reference forms them: repeated multiplication by scaling_line_search (the kernels tested — and k_first_candidate_masks formed — exactly these).
// false: "cone search failure" (solve.jl:210,220), *as / *at untouched
inline bool cone_step_sizes(const int* mask_s, const int* mask_t, const Options& o, double* as, double* at) {
    const int ks = first_feasible_trial(mask_s, o.max_cone_line_search), kt = first_feasible_trial(mask_t, o.max_cone_line_search);
    if (ks < 0 || kt < 0) return false;
    double a = 1.0, b = 1.0;
    for (int k = 0; k < ks; ++k) a = o.scaling_line_search * a;
    for (int k = 0; k < kt; ++k) b = o.scaling_line_search * b;
    *as = a; *at = b;
    return true;
}

// ---- inertia_correction! (inertia.jl:30-80) as two calls round the caller's factorisations ------------------------------------------------------------------
inline bool inertia_ok(const int64_t in[3], i64 nx, i64 m) { return in[0] == nx && in[1] == m && in[2] == 0; }   // inertia.jl:7-11
inline void ic_begin(const Options& o, Scalars& sc) { sc.ep = o.primal_regularization_initial; sc.ed = o.dual_regularization_initial; }   // before IC-1
enum IcVerdict { IC_DONE, IC_AGAIN /* factorise again with the new regularisation (IC-4) */, IC_FAILED /* "inertia correction failure" */ };
// after a factorisation with inertia `in`; first: it was IC-1.  Quirk kept: the `primal_regularization_last == 0.0` test of :48 compares a Vector with a Float64 and is
// always false, so IC-3 always takes max(min_regularization, scaling_regularization_last * eps_last).
inline IcVerdict ic_after(const Options& o, Scalars& sc, const int64_t in[3], i64 nx, i64 m, bool first) {
    if (inertia_ok(in, nx, m)) { if (!first) sc.ep_last = sc.ep; return IC_DONE; }
    if (first) {
        if (in[2] != 0) sc.ed = o.dual_regularization * std::pow(sc.kappa, o.dual_regularization_exponent);   // IC-2
        sc.ep = std::max(o.min_regularization, o.scaling_regularization_last * sc.ep_last);                   // IC-3
        return IC_AGAIN;
    }
    if (sc.ep_last == 0.0) sc.ep = o.scaling_regularization_initial * sc.ep;   // IC-5
    else sc.ep = o.scaling_regularization * sc.ep;
    return sc.ep > o.max_regularization ? IC_FAILED : IC_AGAIN;                // IC-6
}

// ---- iterative_refinement! (iterative_refinement.jl:14-51): the verdict on a residual norm after *it rounds ------------------------------------------------
enum RefineVerdict { REFINE_DONE, REFINE_ROUND /* run one more round, then ++*it */, REFINE_FAILED /* -> the H \ residual fallback */ };
inline RefineVerdict refine_next(const Options& o, double norm, double norm0, int* it) {
    if (*it <= o.max_iterative_refinement) {
        if (norm <= o.iterative_refinement_tolerance && *it >= o.min_iterative_refinement) return REFINE_DONE;
        // a residual with a NaN in it reports +inf (vectors.hip: rabs).  The reference's norm is NaN there: `norm <= tol` is never true, so its loop (`while iteration <=
        // max_iterative_refinement`, :14-44) runs ALL its rounds on NaNs before it fails (:45-51).  DEVIATION, same outcome: the rounds that cannot change the verdict are
        // not run — the loop leaves as soon as the minimum number of rounds is done, fails and reports the reference's round count (max_iterative_refinement + 1)
        const bool hopeless = !std::isfinite(norm) && *it >= o.min_iterative_refinement;
        if (!hopeless) return REFINE_ROUND;
        *it = (int)std::max<i64>(*it, o.max_iterative_refinement + 1);
    }
    return std::isfinite(norm) && norm <= norm0 ? REFINE_DONE : REFINE_FAILED;   // loop exhausted: fail <=> the final error exceeds the initial one
}

// ---- residual line search (solve.jl:254-302), filter.jl, line_search.jl -------------------------------------------------------------------------------------
// filter.jl:43-50 over the n kept pairs
inline bool filter_accepts(const double* filter_theta, const double* filter_merit, i64 n, double theta, double merit) {
    for (i64 i = 0; i < n; ++i)
        if (!(theta < filter_theta[i] || merit < filter_merit[i])) return false;
    return true;
}
// line_search.jl:2-18 with d = dot(merit_gradient, step.primals) precomputed on the device
inline bool switching_condition(double step_size, double dd, double merit_exponent, double violation, double violation_exponent, double reg) {
    return dd < 0.0 && step_size * std::pow(-dd, merit_exponent) > reg * std::pow(violation, violation_exponent);
}
inline bool sufficient_progress(double v, double vc, double m, double mc, double vt, double mt, double mach) {
    return vc - 10.0 * mach * std::fabs(v) <= (1.0 - vt) * v || mc - 10.0 * mach * std::fabs(m) <= m - mt * v;
}
inline bool armijo(double m, double mc, double dd, double step_size, double at, double mach) {
    return mc - m - 10.0 * mach * std::fabs(m) <= at * step_size * dd;
}
inline bool switching_and_armijo(const Options& o, double theta, double M, double Mh, double dd, double step_size) {
    return switching_condition(step_size, dd, o.merit_exponent, theta, o.violation_exponent, 1.0) && armijo(M, Mh, dd, step_size, o.armijo_tolerance, o.machine_tolerance);
}
// does the line search stop at the candidate (thetah, Mh) reached with step_size from (theta, M)?  filter_ok: the filter accepts (thetah, Mh)   solve.jl:256-266
inline bool line_search_accepts(const Options& o, bool filter_ok, double theta, double M, double thetah, double Mh, double dd, double step_size) {
    if (!filter_ok) return false;
    if (theta <= o.slack_tolerance && switching_and_armijo(o, theta, M, Mh, dd, step_size)) return true;
    return sufficient_progress(theta, thetah, M, Mh, o.violation_tolerance, o.merit_tolerance, o.machine_tolerance);
}
// augment_filter!(solver, ...) filter.jl:81-89: after the line search the filter is augmented unless the step taken was a switching + Armijo one
inline bool filter_needs_augment(const Options& o, double theta, double M, double Mh, double dd, double step_size) { return !switching_and_armijo(o, theta, M, Mh, dd, step_size); }

// ---- the scalars of a solve ---------------------------------------------------------------------------------------------------------------------------------
inline void initial_scalars(const Options& o, Scalars& sc) {
    sc.kappa = o.central_path_initial; sc.tau = std::max(0.99, 1.0 - sc.kappa);          // initialize.jl:38-42
    sc.rho = o.penalty_initial;                                                         // :44-48
}
inline void central_path_update(const Options& o, Scalars& sc) {
    sc.kappa = std::max(o.residual_tolerance / 10.0, std::min(o.central_path_scaling * sc.kappa, std::pow(sc.kappa, o.central_path_exponent)));   // solve.jl:356
    sc.tau = std::max(0.99, 1.0 - sc.kappa);                                                                                                      // :359
}
// (after central_path_update and after the dual update with the OLD rho: solve.jl:362-365)
inline void penalty_update(const Options& o, Scalars& sc) { sc.rho = std::min(std::max(o.penalty_scaling * sc.rho, 1.0 / sc.kappa), o.max_penalty); }
// a step that did not advance: everything as before it, except the regularisation it ended with (eps_last restored: every such step repeats IC-1)
inline void restore_scalars_keeping_regularization(Scalars& sc, const Scalars& saved) {
    const double keep_ep = sc.ep, keep_ed = sc.ed;
    sc = saved; sc.ep = keep_ep; sc.ed = keep_ed;
}

}  // namespace calipso
