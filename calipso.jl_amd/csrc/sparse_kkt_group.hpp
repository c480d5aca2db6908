// sparse_kkt_group.hpp — the host bookkeeping of search_direction! for a GROUP of same-pattern sparse problems stepped in lockstep (sparse_kkt_group.hip), as plain
// C++: no HIP header, no handle, so tests/sparse_kkt_group_host/main.cpp runs it on the CPU under the sanitizers.  Here: the layout of the member-major slabs, the
// argument checks with their messages, and the lockstep itself — which members a round covers, what ic_after / refine_next (step_decisions.hpp) decide for each
// member on that member's own Scalars, the per-member statuses and the worst-status rule.  The driver only enqueues what this says and feeds it the read-backs.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "step_decisions.hpp"

namespace calipso {
namespace sparse_kkt_group {

constexpr int MAX_MEMBERS = 128;                 // MAX_BATCH (internal.hpp; sparse_kkt_group.hip asserts the value)
constexpr int STATUS_OK = 0, STATUS_REFINEMENT = 2, STATUS_INERTIA = -1, REFUSED = -4;      // CALIPSO_OK, _WARN_REFINEMENT, _ERR_INERTIA, _ERR_ARGUMENT (asserted there too)

// ---- the member-major slabs: every array holds `members` pieces of one stride, one after the other, in ONE allocation of doubles ---------------------------------
enum Array { A_LXX, A_GX, A_HX, A_W, A_RHO, A_RES, A_STEP, A_CORR, A_ERR, A_RSYM, A_NORM, A_COUNT };
struct Layout {
    long long members = 0;
    long long stride[A_COUNT] = {0};             // doubles per member
    long long offset[A_COUNT] = {0};             // of member 0's piece
    long long doubles = 0;                       // of the whole slab
    long long at(Array a, long long member) const { return offset[a] + member * stride[a]; }
};
// nnz of Lxx, gx, hx; N = nx + 2 ne + 3 nc; n = nx + ne + nc.  Strides are the arrays' own lengths (the penalty and the norm slot: one double)
inline Layout layout(long long members, long long nnzL, long long nnzg, long long nnzh, long long N, long long n) {
    Layout l;
    l.members = members;
    const long long each[A_COUNT] = {nnzL, nnzg, nnzh, N, 1, N, N, N, N, n, 1};
    long long at = 0;
    for (int a = 0; a < A_COUNT; ++a) { l.stride[a] = each[a]; l.offset[a] = at; at += each[a] * members; }
    l.doubles = at;
    return l;
}

// ---- the argument checks: an empty string passes, anything else is the refusal's text ----------------------------------------------------------------------------
inline std::string check_members(const char* entry, long long members) {
    if (members >= 1 && members <= MAX_MEMBERS) return "";
    return std::string(entry) + ": members: a group holds 1 .. " + std::to_string(MAX_MEMBERS) + " members, not " + std::to_string(members);
}
// info[4] of calipso_hip_sparse_kkt_info: 2 = multifrontal.  The column method factors a batch one matrix after the other: a group would gain nothing
inline std::string check_numeric_phase(const char* entry, long long phase) {
    if (phase == 2) return "";
    return std::string(entry) + ": method: a group needs the multifrontal numeric phase (method 4, nested dissection), this plan has the column method (numeric phase " +
           std::to_string(phase) + "), which factors a batch one matrix after the other";
}
inline std::string check_member(const char* entry, long long member, long long members) {
    if (member >= 0 && member < members) return "";
    return std::string(entry) + ": member: " + std::to_string(member) + " is not in 0 .. " + std::to_string(members - 1);
}
// options the group shares; `H \ residual` by GMRES is the single handle's
inline std::string check_option(const char* entry, const char* name, double value) {
    const std::string n = name ? name : "";
    if (n == "krylov_fallback" && value != 0.0) return std::string(entry) + ": krylov_fallback: the `H \\ residual` fallback is not built for groups (a member whose refinement fails gets status 2 and its last refined step)";
    if (n == "krylov_restart" || n == "krylov_max_cycles") return std::string(entry) + ": " + n + ": the `H \\ residual` fallback is not built for groups";
    return "";
}
inline std::string check_required(const char* entry, const char* name, const void* p) { return p ? "" : std::string(entry) + ": " + name + " is NULL"; }

// ---- the lockstep ------------------------------------------------------------------------------------------------------------------------------------------------
enum Phase { WALKING /* inertia correction */, PASSED /* factor in place */, REFINING, FINISHED, FAILED_INERTIA };
struct Member {
    Scalars sc;                                  // kappa (IC-2), ep / ed of the member's last assemble, ep_last
    Phase phase = FINISHED;
    int factorizations = 0, rounds = 0, status = STATUS_OK;
    double norm = 0.0, norm0 = 0.0;
    bool first = true;
};

// report[8] of calipso_hip_sparse_kkt_group_search_direction
enum Report { R_FACTOR_ROUNDS, R_REFINE_ROUNDS, R_HOST_WAITS, R_LAUNCHES, R_DEVICE_MS, R_WALL_MS, R_LAST_FACTOR_ACTIVE, R_LAST_REFINE_ACTIVE, R_COUNT };

struct Lockstep {
    Options opt;
    std::vector<Member> m;
    int factor_rounds = 0, refine_rounds = 0, last_factor_active = 0, last_refine_active = 0;

    explicit Lockstep(int members = 0) : m((size_t)members) {}
    int members() const { return (int)m.size(); }
    std::vector<int> in_phase(Phase p) const { std::vector<int> out; for (int k = 0; k < members(); ++k) if (m[(size_t)k].phase == p) out.push_back(k); return out; }

    // search_direction.jl:1 / inertia.jl:30-41: every member starts IC-1 from the ep_last the caller carries (regularization[3 k + 1])
    void begin(const double* regularization) { begin(regularization, everyone()); }
    // ... for a subset `who` of the members (a whole solve! in lockstep steps only those still walking): members outside it stay FINISHED and are not touched,
    // neither their scalars nor their counts nor their status; regularization is indexed by member all the same
    void begin(const double* regularization, const std::vector<int>& who) {
        factor_rounds = refine_rounds = last_factor_active = last_refine_active = 0;
        for (Member& q : m) q.phase = FINISHED;
        for (int k : who) {
            Member& q = m[(size_t)k];
            q.sc.ep_last = regularization[3 * k + 1];
            ic_begin(opt, q.sc);
            q.phase = WALKING; q.first = true; q.factorizations = q.rounds = 0; q.status = STATUS_OK; q.norm = q.norm0 = 0.0;
        }
    }
    std::vector<int> everyone() const { std::vector<int> all((size_t)members()); for (int k = 0; k < members(); ++k) all[(size_t)k] = k; return all; }
    // the members a factorisation round assembles and factors
    std::vector<int> walking() const { return in_phase(WALKING); }
    // ... and what their inertias (inertia[3 k ..] of member k: entries of other members are not read) make of them: done and failed members leave the set
    void after_factorizations(const std::vector<int>& active, const int64_t* inertia, i64 nx, i64 m_rows) {
        if (active.empty()) return;
        ++factor_rounds; last_factor_active = (int)active.size();
        for (int k : active) {
            Member& q = m[(size_t)k];
            ++q.factorizations;
            const IcVerdict v = ic_after(opt, q.sc, inertia + 3 * (size_t)k, nx, m_rows, q.first);
            q.first = false;
            if (v == IC_DONE) q.phase = PASSED;
            else if (v == IC_FAILED) { q.phase = FAILED_INERTIA; q.status = STATUS_INERTIA; }
        }
    }
    // the members the condensed solve covers: all that passed
    std::vector<int> passed() const { return in_phase(PASSED); }
    // after the first solve: with refinement they are held against their residual norms, without they are finished
    void after_solve() {
        for (Member& q : m) if (q.phase == PASSED) q.phase = opt.iterative_refinement ? REFINING : FINISHED;
    }
    std::vector<int> refining() const { return in_phase(REFINING); }
    // the norms |res - H step|_inf of the refining members (norm[k] of member k): refine_next per member; returns those that run a correction round, which the
    // driver solves and adds before the next norms.  A member's count goes up when its NEXT norm arrives, as the single driver's does after its round
    std::vector<int> after_norms(const std::vector<int>& active, const double* norm, bool first) {
        std::vector<int> round;
        for (int k : active) {
            Member& q = m[(size_t)k];
            q.norm = norm[k];
            if (first) q.norm0 = q.norm; else ++q.rounds;
            const RefineVerdict v = refine_next(opt, q.norm, q.norm0, &q.rounds);
            if (v == REFINE_ROUND) { round.push_back(k); continue; }
            q.phase = FINISHED;
            if (v == REFINE_FAILED) q.status = STATUS_REFINEMENT;       // no `H \ residual` in a group: the last refined step stays
        }
        if (!round.empty()) { ++refine_rounds; last_refine_active = (int)round.size(); }
        return round;
    }
    // the worst member status: an inertia failure before a refinement warning before success
    int worst() const { return worst(everyone()); }
    int worst(const std::vector<int>& who) const {
        int w = STATUS_OK;
        for (int k : who) { const Member& q = m[(size_t)k]; if (q.status == STATUS_INERTIA) return STATUS_INERTIA; if (q.status == STATUS_REFINEMENT) w = STATUS_REFINEMENT; }
        return w;
    }
    // what the entry writes per member (of `who`: the entries of other members are left alone): regularization[3], info[4], status
    void outputs(double* regularization, double* info, int32_t* status) const { outputs(regularization, info, status, everyone()); }
    void outputs(double* regularization, double* info, int32_t* status, const std::vector<int>& who) const {
        for (int k : who) {
            const Member& q = m[(size_t)k];
            regularization[3 * k] = q.sc.ep; regularization[3 * k + 1] = q.sc.ep_last; regularization[3 * k + 2] = q.sc.ed;
            if (info) { info[4 * k] = q.factorizations; info[4 * k + 1] = q.rounds; info[4 * k + 2] = q.norm; info[4 * k + 3] = 0.0; }
            if (status) status[k] = q.status;
        }
    }
};

}  // namespace sparse_kkt_group
}  // namespace calipso
