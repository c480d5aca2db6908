// sparse_solve_group.hpp — the host bookkeeping of solve! for a GROUP of same-pattern sparse conic QPs stepped in lockstep (sparse_solve_group.hip), as plain C++:
// no HIP header, no handle, so tests/sparse_solve_group_host/main.cpp runs it on the CPU under the sanitizers.  Here: the layout of the member-major slab of the
// solve's own arrays, the per-member scalars a launch reads from the device, the argument checks with their messages, and the lockstep itself — solve! of
// sparse_solve.hip (solve.jl:8-377) cut at its read-backs into a state machine per member, every decision through step_decisions.hpp on that member's own Scalars,
// Filter and published block.  The driver only enqueues what this says and feeds it the read-backs.
//
// One tick: classify (exit_kind on the published prologue) -> outer-update rounds for the members that need one, until none does -> search_direction! of the
// stepping members (sparse_kkt_group.hpp: Lockstep, begun for that subset) -> verdicts -> cone masks + first candidate -> line-search trial rounds for the members
// that reject, at their own step sizes -> accept + next prologue.  A member that has ended is in no list any more.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "sparse_kkt_group.hpp"            // MAX_MEMBERS, check_member, check_required; the search_direction lockstep a tick runs for its stepping members
#include "sparse_solve.hpp"                // Filter, the published block, the single handle's Layout (item space and workspace)

namespace calipso {
namespace sparse_solve_group {

using sparse_solve::Filter;
namespace ss = calipso::sparse_solve;

// member statuses: solve!'s own (1 solved, 0 iteration caps), the reference's error()s, the refinement failure without a fallback (-100 - CALIPSO_WARN_REFINEMENT)
constexpr int STATUS_SOLVED = 1, STATUS_CAPS = 0, STATUS_INERTIA = -1, STATUS_CONE_SEARCH = -2, STATUS_DEVICE = -5, STATUS_REFINEMENT = -102;
constexpr int WARN_REFINEMENT = 2, WARN_LINE_SEARCH = 3;
constexpr int INFO_DOUBLES = 16;                 // per member, the layout of calipso_hip_sparse_kkt_solve's info

// ---- the member-major slab of the solve's own arrays (the point, the residual and the step are the search_direction slab's: sparse_kkt_group.hpp) ------------------
enum Array { A_CAND, A_DUAL, A_MGRAD, A_BGRAD, A_CPROD, A_CTARGET, A_G, A_H, A_GCAND, A_HCAND, A_FX, A_Q, A_B, A_HVEC, A_WS, A_WSM, A_PUB, A_SCALARS, A_CONSTANT, A_COUNT };
// the scalars of member m that a launch reads from the device: A_SCALARS, DS_STRIDE doubles per member, filled from a pinned host block by ONE stream-ordered copy at
// the head of every read-back group (so the block is never rewritten while a copy of it is in flight)
enum DeviceScalar { DS_KAPPA, DS_TAU, DS_STEP_S, DS_STEP_T, DS_RHO_BEFORE, DS_RHO, DS_TRACE_ROW /* of the member's kept trace, < 0: none */, DS_STRIDE = 8 };
constexpr long long PUB_STRIDE = (long long)ss::PUB_ALLOC_DOUBLES;       // doubles per member of the published blocks, on the device and in the pinned host copy

struct Layout {
    long long members = 0;
    long long stride[A_COUNT] = {0};             // doubles per member
    long long offset[A_COUNT] = {0};             // of member 0's piece
    long long doubles = 0;                       // of the whole slab
    long long at(Array a, long long member) const { return offset[a] + member * stride[a]; }
};
// `one`: the single handle's layout for this pattern — every member runs on its grid with a workspace of its own
inline Layout layout(long long members, long long nx, long long ne, long long nc, const ss::Layout& one) {
    Layout l;
    l.members = members;
    const long long N = nx + 2 * ne + 3 * nc, n = nx + ne + nc;
    const long long each[A_COUNT] = {N, ne, n, nc, nc, nc, ne, nc, ne, nc, nx, nx, ne, nc, one.doubles, (one.mask_ints + 1) / 2, PUB_STRIDE, DS_STRIDE, 1};
    long long at = 0;
    for (int a = 0; a < A_COUNT; ++a) { l.stride[a] = each[a]; l.offset[a] = at; at += each[a] * members; }
    l.doubles = at;
    return l;
}

// ---- the argument checks: an empty string passes, anything else is the refusal's text ----------------------------------------------------------------------------
inline std::string check_attach(const char* entry, long long nx, long long ne, long long nc, const void* q, const void* b, const void* hvec) {
    if (nx > 0 && !q) return std::string(entry) + ": q is NULL";
    if (ne > 0 && !b) return std::string(entry) + ": b is NULL";
    if (nc > 0 && !hvec) return std::string(entry) + ": hvec is NULL";
    return "";
}
inline std::string check_initialize(const char* entry, long long nx, const void* x0) { return nx > 0 && !x0 ? std::string(entry) + ": x0 is NULL" : ""; }
// what a solve needs resident: the three matrices (have[0..2] where they have non-zeros), q, b, hvec, a point
inline std::string check_ready(const char* entry, const bool have_matrix[3], const long long nnz[3], bool attached, bool point, bool need_point) {
    static const char* const names[3] = {"Lxx", "gx", "hx"};
    for (int i = 0; i < 3; ++i) if (nnz[i] > 0 && !have_matrix[i]) return std::string(entry) + ": no " + names[i] + " resident (calipso_hip_sparse_kkt_group_set_values first)";
    if (!attached) return std::string(entry) + ": no q, b, hvec resident (calipso_hip_sparse_kkt_group_qp_attach first)";
    if (need_point && !point) return std::string(entry) + ": no point resident (calipso_hip_sparse_kkt_group_initialize, or set_values with w, first)";
    return "";
}
inline std::string check_solve(const char* entry, const void* status) { return status ? "" : std::string(entry) + ": status is NULL"; }
inline std::string check_keep_trace(const char* entry, long long rows) {
    if (rows < 1 || rows > ss::TRACE_ROWS_MAX) return std::string(entry) + ": rows: 1 .. " + std::to_string(ss::TRACE_ROWS_MAX) + " rows can be kept, not " + std::to_string(rows);
    return "";
}
inline std::string check_trace(const char* entry, const void* out, long long cap_rows) {
    if (cap_rows < 0) return std::string(entry) + ": cap_rows is negative";
    if (!out && cap_rows > 0) return std::string(entry) + ": out is NULL with cap_rows > 0";
    return "";
}
// the named vectors of calipso_hip_sparse_kkt_get that a group member has: the solve's vectors (not the differentiate slacks, the evaluator's objective, the matrices)
inline std::string check_named_vector(const char* entry, const char* name, const void* data, long long len, long long nx, long long ne, long long nc) {
    const int v = ss::vector_by_name(name);
    if (v < 0 || v >= ss::V_COUNT) return std::string(entry) + ": name: no resident vector of a group member called " + (name ? name : "(null)");
    return ss::check_named_vector(entry, name, data, len, nx, ne, nc, false);
}

// ---- the lockstep ------------------------------------------------------------------------------------------------------------------------------------------------
enum Phase { LIVE /* holds a published prologue, to be classified */, NEEDS_OUTER, STEPPING, ENDED };
struct Member {
    Scalars sc;                                  // kappa, tau, rho, and the regularisation search_direction carries from step to step
    Filter filter;
    Phase phase = ENDED;
    int status = STATUS_CAPS, worst = 0;
    i64 total_iterations = 1, outer = 0, inner = 1, accepted = 0, factorizations = 0, max_rounds = 0, refinement_failures = 0, trials = 0, waits = 0;
    double equality_violation = 0.0, cone_product_violation = 0.0;
    // the step in flight
    double M = 0.0, theta = 0.0, Mh = 0.0, thetah = 0.0, dd = 0.0, step_size = 1.0, step_size_t = 1.0, rho_before = 0.0;
    i64 line_search = 0;
};

// report of calipso_hip_sparse_kkt_group_solve: the eight of search_direction (summed over the ticks; the two "last active" counts are the last tick's), then these
enum Report { R_TICKS = sparse_kkt_group::R_COUNT, R_OUTER_ROUNDS, R_TRIAL_ROUNDS, R_SOLVE_HOST_WAITS, R_SOLVE_LAUNCHES, R_VECTOR_MS, R_SEARCH_DIRECTION_MS, R_SOLVE_WALL_MS, R_SOLVE_COUNT };

struct Lockstep {
    Options opt;
    bool continue_after_refinement_failure = false;
    i64 N = 0, ne = 0, nc = 0;
    std::vector<Member> m;
    i64 ticks = 0, outer_rounds = 0, trial_rounds = 0, host_waits = 0;      // host_waits: the read-backs of the vector half (search_direction counts its own)

    explicit Lockstep(int members = 0) : m((size_t)members) {}
    int members() const { return (int)m.size(); }
    std::vector<int> in_phase(Phase p) const { std::vector<int> out; for (int k = 0; k < members(); ++k) if (m[(size_t)k].phase == p) out.push_back(k); return out; }
    static const double* block(const double* pub, int k) { return pub + (long long)k * PUB_STRIDE; }
    static const int* masks(const double* pub, int k) { return reinterpret_cast<const int*>(block(pub, k) + ss::PUB_DOUBLES); }
    void read_back(const std::vector<int>& who) { ++host_waits; for (int k : who) ++m[(size_t)k].waits; }

    // initialize.jl:38-48 for every member (kappa, tau and rho start from the options, whatever the members held: as the single handle's solve)
    void begin(const Options& o, bool continue_after_failure, i64 N_, i64 ne_, i64 nc_) {
        opt = o; continue_after_refinement_failure = continue_after_failure; N = N_; ne = ne_; nc = nc_;
        ticks = outer_rounds = trial_rounds = host_waits = 0;
        for (Member& q : m) {
            const Scalars keep = q.sc;
            q = Member();
            q.sc = keep;
            initial_scalars(opt, q.sc);
            q.sc.ep_last = 0.0;                      // (every solve starts as a fresh solver does)
            q.filter = Filter((i64)opt.max_filter);
            q.phase = LIVE;
        }
    }
    std::vector<int> everyone() const { std::vector<int> all((size_t)members()); for (int k = 0; k < members(); ++k) all[(size_t)k] = k; return all; }
    // the start group's read-back (solve.jl:85-95): the two violations as they lie, the first prologue
    void after_start(const double* pub) {
        read_back(everyone());
        for (int k = 0; k < members(); ++k) {
            Member& q = m[(size_t)k];
            q.equality_violation = block(pub, k)[ss::PUB_G_INF]; q.cone_product_violation = block(pub, k)[ss::PUB_PRODUCT_INF];
            q.filter.reset();
            q.outer = 1; q.inner = 1;
            if (opt.max_outer_iterations < 1) { q.outer = 0; end(k, STATUS_CAPS); }
        }
    }
    bool any_live() const { for (const Member& q : m) if (q.phase != ENDED) return true; return false; }
    void end(int k, int status) { m[(size_t)k].phase = ENDED; m[(size_t)k].status = status; }

    // every LIVE member from its published prologue (solve.jl:138-143, :165; the residual-iteration cap of :99): solved members leave, the others step or need
    // an outer update; returns those that need one
    std::vector<int> classify(const double* pub) {
        for (int k : in_phase(LIVE)) {
            Member& q = m[(size_t)k];
            if (q.inner > opt.max_residual_iterations) { q.phase = NEEDS_OUTER; continue; }
            const double* p = block(pub, k);
            const StepNorms norms = step_norms(p, N, ne, nc);
            const int kind = exit_kind(opt, q.sc.kappa, norms, q.equality_violation, q.cone_product_violation, true);
            if (kind == 1) { end(k, STATUS_SOLVED); continue; }
            if (kind == 2) { q.phase = NEEDS_OUTER; continue; }
            q.phase = STEPPING; q.M = p[ss::PUB_MERIT]; q.theta = p[ss::PUB_THETA];
        }
        return in_phase(NEEDS_OUTER);
    }
    // solve.jl:356-368 for the members that need it: the central path, the penalty (rho_before: what the dual update multiplies with), the filter; returns those that
    // get a prologue behind it (all but the members in their last outer iteration)
    std::vector<int> outer_begin(const std::vector<int>& who) {
        std::vector<int> with_prologue;
        ++outer_rounds;
        for (int k : who) {
            Member& q = m[(size_t)k];
            central_path_update(opt, q.sc);
            q.rho_before = q.sc.rho;
            penalty_update(opt, q.sc);
            q.filter.reset();
            if (q.outer < opt.max_outer_iterations) with_prologue.push_back(k);
        }
        return with_prologue;
    }
    // ... and after the batch's ONE read-back (none where nobody got a prologue): a member past its outer cap ends with status 0, the others are LIVE again
    void outer_after(const std::vector<int>& who, const std::vector<int>& with_prologue) {
        if (!with_prologue.empty()) read_back(with_prologue);
        else ++host_waits;                           // (the driver ends the group with a wait of its own; no member's count: the single handle has none there)
        for (int k : who) {
            Member& q = m[(size_t)k];
            if (q.outer >= opt.max_outer_iterations) { end(k, STATUS_CAPS); continue; }
            q.outer += 1; q.inner = 1; q.phase = LIVE;
        }
    }
    std::vector<int> stepping() const { return in_phase(STEPPING); }
    // the regularisation a member's search_direction starts from (regularization[3 k ..]) and what it left there
    void regularization_in(const std::vector<int>& who, double* regularization) const {
        for (int k : who) { const Scalars& sc = m[(size_t)k].sc; regularization[3 * k] = sc.ep; regularization[3 * k + 1] = sc.ep_last; regularization[3 * k + 2] = sc.ed; }
    }
    // the verdicts of search_direction (status, info[4], regularization[3] per member): an inertia failure ends the member; a refinement failure ends it with -102 at
    // its last accepted iterate unless the group continues past it.  Returns the members that go on to the cone search
    std::vector<int> after_search_direction(const std::vector<int>& who, const int32_t* status, const double* info, const double* regularization) {
        std::vector<int> on;
        for (int k : who) {
            Member& q = m[(size_t)k];
            q.sc.ep = regularization[3 * k]; q.sc.ep_last = regularization[3 * k + 1]; q.sc.ed = regularization[3 * k + 2];
            q.factorizations += (i64)info[4 * k]; q.max_rounds = std::max(q.max_rounds, (i64)info[4 * k + 1]);
            if (status[k] == sparse_kkt_group::STATUS_INERTIA) { end(k, STATUS_INERTIA); continue; }
            if (status[k] == sparse_kkt_group::STATUS_REFINEMENT) {
                q.refinement_failures += 1; q.worst = std::max(q.worst, WARN_REFINEMENT);
                if (!continue_after_refinement_failure) { end(k, STATUS_REFINEMENT); continue; }
            }
            on.push_back(k);
        }
        return on;
    }
    // the ONE read-back behind the cone masks and the first candidate (solve.jl:190-250): the member's step sizes from its masks
    void after_first_candidate(const std::vector<int>& who, const double* pub) {
        read_back(who);
        for (int k : who) {
            Member& q = m[(size_t)k];
            const double* p = block(pub, k);
            q.step_size = 1.0; q.step_size_t = 1.0;
            if (!cone_step_sizes(masks(pub, k), masks(pub, k) + CONE_MASK_WORDS, opt, &q.step_size, &q.step_size_t)) { end(k, STATUS_CONE_SEARCH); continue; }
            if (q.step_size != p[ss::PUB_STEP_S] || q.step_size_t != p[ss::PUB_STEP_T]) { end(k, STATUS_DEVICE); continue; }      // the device formed other step sizes than cone_step_sizes()
            q.Mh = p[ss::PUB_CAND_MERIT]; q.thetah = p[ss::PUB_CAND_THETA]; q.dd = p[ss::PUB_DD];
            q.line_search = 0;
        }
    }
    // the members whose filter or line search rejects their candidate (solve.jl:254-266): their step size is scaled here, once per round
    std::vector<int> rejecting() {
        std::vector<int> out;
        for (int k : in_phase(STEPPING)) {
            Member& q = m[(size_t)k];
            if (q.line_search >= opt.max_residual_line_search) continue;
            if (line_search_accepts(opt, q.filter.accepts(q.thetah, q.Mh), q.theta, q.M, q.thetah, q.Mh, q.dd, q.step_size)) continue;
            q.step_size = opt.scaling_line_search * q.step_size;
            out.push_back(k);
        }
        if (!out.empty()) ++trial_rounds;
        return out;
    }
    void after_trial(const std::vector<int>& who, const double* pub) {
        read_back(who);
        for (int k : who) {
            Member& q = m[(size_t)k];
            q.Mh = block(pub, k)[ss::PUB_CAND_MERIT]; q.thetah = block(pub, k)[ss::PUB_CAND_THETA];
            q.line_search += 1; q.trials += 1;
        }
    }
    // the members that take their step (solve.jl:299-333): the line-search warning, the filter (filter.jl:81-89); their step size is Member::step_size
    std::vector<int> accepting() {
        const std::vector<int> who = in_phase(STEPPING);
        for (int k : who) {
            Member& q = m[(size_t)k];
            if (q.line_search >= opt.max_residual_line_search) q.worst = std::max(q.worst, WARN_LINE_SEARCH);
            if (filter_needs_augment(opt, q.theta, q.M, q.Mh, q.dd, q.step_size)) q.filter.augment((1.0 - opt.violation_tolerance) * q.theta, q.M - opt.merit_tolerance * q.theta);
        }
        return who;
    }
    // the ONE read-back behind accept and the next prologue
    void after_accept(const std::vector<int>& who, const double* pub) {
        read_back(who);
        for (int k : who) {
            Member& q = m[(size_t)k];
            q.equality_violation = block(pub, k)[ss::PUB_G_INF]; q.cone_product_violation = block(pub, k)[ss::PUB_PRODUCT_INF];
            q.total_iterations += 1; q.accepted += 1; q.inner += 1;
            q.phase = LIVE;
        }
    }
    // info[16] of member k in the single entry's layout (the three times are the group's: the members share them); the worst member status
    void info(int k, double vector_ms, double search_direction_ms, double wall_ms, double* out) const {
        const Member& q = m[(size_t)k];
        const double v[INFO_DOUBLES] = {(double)q.total_iterations, (double)q.outer, (double)q.accepted, (double)q.factorizations, (double)q.max_rounds, (double)q.refinement_failures,
                                        (double)q.worst, (double)q.waits, (double)q.trials, q.sc.kappa, q.sc.rho, q.sc.ep_last, vector_ms, search_direction_ms, wall_ms, (double)q.status};
        std::copy(v, v + INFO_DOUBLES, out);
    }
    int worst_status() const {
        int w = STATUS_SOLVED;
        for (const Member& q : m) if (q.status < w) w = q.status;
        return w;
    }
};

}  // namespace sparse_solve_group
}  // namespace calipso
