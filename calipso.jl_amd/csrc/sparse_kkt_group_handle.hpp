// sparse_kkt_group_handle.hpp — the handle behind calipso_hip_sparse_kkt_group_* as the two translation units that work on it see it: sparse_kkt_group.hip
// (search_direction! in lockstep) and sparse_solve_group.hip (solve! in lockstep); how a group kernel reaches a member's data (Strides, member_data); what the
// units call of each other.
#pragma once
#include <string>
#include <vector>

#include "sparse_kkt_handle.hpp"
#include "sparse_kkt_group.hpp"

namespace calipso {
namespace sparse_kkt_group {
struct SolveGroupState;                        // sparse_solve_group.hip: the members' resident vectors, workspaces, published blocks and the solve's lockstep
}
}

struct calipso_hip_sparse_kkt_group {
    calipso::sparse_kkt::KH* base = nullptr;   // the analysis, the plan, its stream, the tables on the device, the owner of every allocation here, the error text
    int members = 0;
    calipso::sparse_kkt_group::Layout lay;
    double* slab = nullptr;                    // lay.doubles
    double* K = nullptr; long long strideK = 0;      // the plan's own values: member m's K at K + m * strideK
    long long* inertia = nullptr;              // members x 3 on the device
    calipso::sparse_kkt_group::Lockstep ls;    // the shared options and every member's scalars, phase and counts
    bool have[5] = {false, false, false, false, false};
    bool assembled = false, factored = false;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    double ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int launches_factor = 0, launches_solve = 0;     // of one batched factorisation / solve of the plan (per level of its schedule; the two permutations)
    std::vector<int64_t> inertia_host;
    std::vector<double> norm_host;
    calipso::sparse_kkt_group::SolveGroupState* solve = nullptr;      // made by the first solve entry that needs it (sparse_solve_group.hip), released with the group
    bool continue_after_refinement_failure = false;
};

namespace calipso {
namespace sparse_kkt_group {

typedef calipso_hip_sparse_kkt_group GH;

// ---- how a group kernel reaches member m: the pointers of member 0 shifted by the member's strides ---------------------------------------------------------------
struct Strides { long long L, g, h, N, n, K; };

__device__ __forceinline__ calipso::sparse_kkt::KktDev member_data(const calipso::sparse_kkt::KktDev& d, const Strides& s, int m) {
    calipso::sparse_kkt::KktDev r = d;
    r.Lxx += (size_t)m * s.L; r.gx += (size_t)m * s.g; r.hx += (size_t)m * s.h; r.w += (size_t)m * s.N; r.rho += m;
    return r;
}

// ---- sparse_kkt_group.hip, for sparse_solve_group.hip ---------------------------------------------------------------------------------------------------------
int group_fail(GH* g, int rc, const std::string& text);                                                     // sets last_error, returns rc
double* group_array(GH* g, Array a);                                                                        // member 0's piece of a slab array
Strides group_strides(const GH* g);
// search_direction! of `members` (ascending) on device vectors (group members x N each); regularization (3), info (4), status per member of the GROUP: entries of
// members outside the set are not touched; the return value is the worst status of the set
int group_search_direction(GH* g, const std::vector<int>& members, const double* res, double* step, double* regularization, double* info, int32_t* status, double* report);
// ---- sparse_solve_group.hip, for sparse_kkt_group.hip ---------------------------------------------------------------------------------------------------------
void group_solve_release(GH* g);
int group_solve_set_option(GH* g, const char* name, double value);                                          // 1 taken, 0 unknown, < 0 refused

}  // namespace sparse_kkt_group
}  // namespace calipso
