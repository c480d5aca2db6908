// sparse_solve_group.hip — solve! (src/solver/solve.jl:8-377) of the sparse conic QP for every member of a GROUP of same-pattern problems in lockstep: the entries
// calipso_hip_sparse_kkt_group_qp_attach / _initialize / _solve / _get / _solution_device / _keep_trace / _trace (include/calipso_hip.h) on the group handle of
// sparse_kkt_group.hip.  Every member's result is bit for bit what calipso_hip_sparse_kkt_solve gives on the same data.
//
//   kernels        the group forms of sparse_solve.hip's: the member on blockIdx.z through the list of ACTIVE members (Members, by value), KktDev shifted by
//                  member_data, SolveDev by member_solve (every vector, the reduction workspace, the mask words and the published block have a piece per member),
//                  then the SAME __device__ bodies (sparse_solve_kernels.hpp: solve_body, the QP instantiation).  The grid per member is the single handle's
//                  Layout::grid: the two-stage reductions add their partials in workgroup order, so a member's sums are the single handle's.  No atomics on doubles.
//   scalars        members walk with different kappa, tau, rho and step sizes: a launch reads them from a member-major device array (A_SCALARS), which ONE
//                  stream-ordered copy from a pinned host block fills at the head of every read-back group.  Nothing waits for it, and the block is rewritten only
//                  after the group's read-back has come in.
//   driver         the lockstep of sparse_solve_group.hpp: the host decides per member, this file enqueues for the lists it is given and reads all published blocks
//                  back in ONE copy per group.  The host waits of a tick are those of its slowest member; its launches do not depend on the number of members.
// Evaluated members, differentiate!, the GMRES fallback and a captured-graph replay of the factorisation are the single handle's.
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "sparse_kkt_group_handle.hpp"
#include "sparse_solve_kernels.hpp"
#include "sparse_solve_group.hpp"

using calipso::i64;
using namespace calipso::sparse_kkt;
namespace grp = calipso::sparse_kkt_group;
namespace sg = calipso::sparse_solve_group;
namespace ss = calipso::sparse_solve;
using grp::GH;
using grp::Strides;
static_assert(sg::STATUS_INERTIA == CALIPSO_ERR_INERTIA && sg::STATUS_CONE_SEARCH == CALIPSO_ERR_CONE_SEARCH && sg::STATUS_DEVICE == CALIPSO_ERR_HIP &&
              sg::STATUS_REFINEMENT == -100 - CALIPSO_WARN_REFINEMENT && sg::WARN_REFINEMENT == CALIPSO_WARN_REFINEMENT && sg::WARN_LINE_SEARCH == CALIPSO_WARN_LINE_SEARCH, "statuses");
static_assert(KT == ss::THREADS, "the workspace layout counts workgroups of KT threads");

namespace {

struct Members { int n; int member[calipso::MAX_BATCH]; };
// the doubles (unsigned words for wsm) between two members' pieces of the solve's arrays, and the two member-major arrays of scalars
struct SolveStrides { long long N, n, nx, ne, nc, ws, wsm, pub; const double* constant; const double* scalars; };

}  // namespace

struct calipso::sparse_kkt_group::SolveGroupState {
    ss::Layout one;                            // the single handle's item space, grid and workspace for this pattern: every member's
    sg::Layout lay;
    double* slab = nullptr;                    // lay.doubles
    SolveDev v{};                              // member 0's
    SolveStrides st{};
    sg::Lockstep ls;
    bool attached = false;
    double* hpub = nullptr;                    // pinned: every member's published block on the host
    double* hscalars = nullptr;                // pinned: every member's device scalars
    Grown<double> trace;                       // members x trace_cap rows of N
    i64 trace_cap = 0;
    std::vector<i64> trace_rows, trace_total;  // of the last solve, per member
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool open = false;
    double vector_ms = 0.0;
    i64 launches = 0;
    std::vector<double> regularization, sd_info;
    std::vector<int32_t> sd_status;
};

namespace {

typedef grp::SolveGroupState ST;

__device__ __forceinline__ SolveDev member_solve(const SolveDev& v, const SolveStrides& s, int m) {
    SolveDev r = v;
    const size_t k = (size_t)m;
    r.q += k * s.nx; r.b += k * s.ne; r.hvec += k * s.nc;
    r.objective_constant = s.constant[m];
    r.w += k * s.N; r.cand += k * s.N; r.res += k * s.N; r.step += k * s.N; r.mgrad += k * s.n;
    r.dual += k * s.ne; r.g += k * s.ne; r.gcand += k * s.ne;
    r.bgrad += k * s.nc; r.cprod += k * s.nc; r.ctarget += k * s.nc; r.h += k * s.nc; r.hcand += k * s.nc;
    r.fx += k * s.nx;
    r.ws += k * s.ws; r.wsm += k * s.wsm;
    r.pub += k * s.pub; r.pub_masks = reinterpret_cast<unsigned*>(r.pub + ss::PUB_DOUBLES);
    return r;
}
__device__ __forceinline__ double member_scalar(const SolveStrides& s, int m, int which) { return s.scalars[(size_t)m * sg::DS_STRIDE + which]; }

// ---- the group kernels: blockIdx.z = place in the active list; blockIdx.x runs over the single handle's grid ------------------------------------------------------
#define MEMBER const int m = a.member[blockIdx.z]; const KktDev dm = grp::member_data(d, ks, m); const SolveDev vm = member_solve(v, s, m)

__global__ __launch_bounds__(KT) void k_solve_group_init(const KktDev d, const SolveDev v, const Strides ks, const SolveStrides s, const Members a) {
    MEMBER;
    solve_body::init<false>(dm, vm);
}
__global__ __launch_bounds__(KT) void k_solve_group_fill_dual(const KktDev d, const SolveDev v, const Strides ks, const SolveStrides s, const Members a, double value) {
    MEMBER;
    solve_body::fill(dm.ne, vm.dual, value);
}
// the penalty lives on the device (KktDev::rho of the member): written by a kernel, stream-ordered
__global__ __launch_bounds__(KT) void k_solve_group_penalty(double* __restrict__ rho, const SolveStrides s, const Members a) {
    const int m = a.member[blockIdx.z];
    solve_body::fill(1, rho + m, member_scalar(s, m, sg::DS_RHO));
}
__global__ __launch_bounds__(KT) void k_solve_group_prologue(const KktDev d, const SolveDev v, const Strides ks, const SolveStrides s, const Members a) {
    MEMBER;
    solve_body::prologue<false>(dm, vm, member_scalar(s, m, sg::DS_KAPPA));
}
__global__ __launch_bounds__(64) void k_solve_group_prologue_finish(const KktDev d, const SolveDev v, const Strides ks, const SolveStrides s, const Members a) {
    MEMBER;
    solve_body::prologue_finish<false>(dm, vm, member_scalar(s, m, sg::DS_KAPPA));
}
__global__ __launch_bounds__(KT) void k_solve_group_cone_masks(const KktDev d, const SolveDev v, const Strides ks, const SolveStrides s, const Members a, double sls, int nk) {
    MEMBER;
    solve_body::cone_masks(dm, vm, member_scalar(s, m, sg::DS_TAU), sls, nk);
}
__global__ __launch_bounds__(64) void k_solve_group_masks_finish(const SolveDev v, const SolveStrides s, const Members a, double sls, int nk) {
    const int m = a.member[blockIdx.z];
    solve_body::masks_finish(member_solve(v, s, m), sls, nk);
}
// from_masks: the step sizes are those the masks' finishing kernel left in the member's published block (the first candidate); else the member's own scalars
__global__ __launch_bounds__(KT) void k_solve_group_candidate(const KktDev d, const SolveDev v, const Strides ks, const SolveStrides s, const Members a, int from_masks, int first) {
    MEMBER;
    solve_body::candidate(dm, vm, from_masks ? (const double*)vm.pub : (const double*)nullptr, member_scalar(s, m, sg::DS_STEP_S), member_scalar(s, m, sg::DS_STEP_T), first);
}
__global__ __launch_bounds__(64) void k_solve_group_candidate_finish(const KktDev d, const SolveDev v, const Strides ks, const SolveStrides s, const Members a, int first) {
    MEMBER;
    solve_body::candidate_finish<false>(dm, vm, member_scalar(s, m, sg::DS_KAPPA), first);
}
__global__ __launch_bounds__(KT) void k_solve_group_accept(const KktDev d, const SolveDev v, const Strides ks, const SolveStrides s, const Members a, int start) {
    MEMBER;
    solve_body::accept<false>(dm, vm, member_scalar(s, m, sg::DS_STEP_S), start);
}
__global__ __launch_bounds__(64) void k_solve_group_accept_finish(const SolveDev v, const SolveStrides s, const Members a) {
    const int m = a.member[blockIdx.z];
    solve_body::accept_finish(member_solve(v, s, m));
}
__global__ __launch_bounds__(KT) void k_solve_group_outer_update(const KktDev d, const SolveDev v, const Strides ks, const SolveStrides s, const Members a) {
    MEMBER;
    solve_body::outer_update(dm, vm, member_scalar(s, m, sg::DS_RHO_BEFORE));
}
// the member's accepted iterate into row DS_TRACE_ROW of its kept trace (rows x N per member, `cap` rows each); a negative row: nothing is kept
__global__ __launch_bounds__(KT) void k_solve_group_trace(const SolveDev v, const SolveStrides s, const Members a, double* __restrict__ trace, long long cap) {
    const int m = a.member[blockIdx.z];
    const double row = member_scalar(s, m, sg::DS_TRACE_ROW);
    if (row < 0.0) return;
    const long long k = (long long)blockIdx.x * KT + threadIdx.x;
    if (k < s.N) trace[((size_t)m * (size_t)cap + (size_t)row) * (size_t)s.N + (size_t)k] = v.w[(size_t)m * (size_t)s.N + (size_t)k];
}
#undef MEMBER
// (a launch's argument block holds 4 KiB: the active list is the large part, the members' scalars are on the device for that reason)
static_assert(sizeof(KktDev) + sizeof(SolveDev) + sizeof(Strides) + sizeof(SolveStrides) + sizeof(Members) + 64 <= 4096, "the arguments of a group kernel");

// ---- host -------------------------------------------------------------------------------------------------------------------------------------------------------
#define GK(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return grp::group_fail(g, CALIPSO_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); } while (0)
#define GREFUSE(text) do { const std::string t__ = (text); if (!t__.empty()) return grp::group_fail(g, CALIPSO_ERR_ARGUMENT, t__); } while (0)

unsigned blocks_of(long long items) { return (unsigned)std::max<long long>((items + KT - 1) / KT, 1); }
double* arr(ST* t, sg::Array a) { return t->slab + t->lay.offset[a]; }
Members members_of(const std::vector<int>& who) {
    Members a;
    a.n = (int)who.size();
    for (int z = 0; z < a.n; ++z) a.member[z] = who[(size_t)z];
    return a;
}

// the members' vectors, workspaces and published blocks: made once per group, by the first entry that needs them, from the group's one memory owner
int solve_state(GH* g) {
    if (g->solve) return CALIPSO_OK;
    KH* s = g->base;
    ST* t = new ST();
    g->solve = t;                                            // (released with the group, whatever happens below)
    const KktDev& d = s->d;
    std::vector<int> small, wide;
    for (int j = 0; j < d.nsoc; ++j) (s->an.soc_dim[(size_t)j] <= ss::SMALL_CONE_MAX ? small : wide).push_back(j);
    t->one = ss::layout(d.nx, d.ne, d.nc, (i64)small.size(), (i64)wide.size());
    t->lay = sg::layout(g->members, d.nx, d.ne, d.nc, t->one);
    SolveDev& v = t->v;
    v.rows = t->one.rows; v.small0 = t->one.small0; v.wide0 = t->one.wide0; v.items = t->one.items;
    v.n_small = (int)small.size(); v.n_wide = (int)wide.size(); v.grid = t->one.grid;
    v.off_prologue = t->one.off_prologue; v.off_candidate = t->one.off_candidate; v.off_accept = t->one.off_accept;
    int rc;
    if ((rc = device_upload(s, small, &v.small_cones)) || (rc = device_upload(s, wide, &v.wide_cones)) || (rc = device_fixed(s, &t->slab, (size_t)t->lay.doubles))) return rc;
    v.cand = arr(t, sg::A_CAND); v.dual = arr(t, sg::A_DUAL); v.mgrad = arr(t, sg::A_MGRAD); v.bgrad = arr(t, sg::A_BGRAD); v.cprod = arr(t, sg::A_CPROD);
    v.ctarget = arr(t, sg::A_CTARGET); v.g = arr(t, sg::A_G); v.h = arr(t, sg::A_H); v.gcand = arr(t, sg::A_GCAND); v.hcand = arr(t, sg::A_HCAND); v.fx = arr(t, sg::A_FX);
    v.q = arr(t, sg::A_Q); v.b = arr(t, sg::A_B); v.hvec = arr(t, sg::A_HVEC);
    v.ws = arr(t, sg::A_WS); v.wsm = reinterpret_cast<unsigned*>(arr(t, sg::A_WSM));
    v.pub = arr(t, sg::A_PUB); v.pub_masks = reinterpret_cast<unsigned*>(v.pub + ss::PUB_DOUBLES);
    v.w = grp::group_array(g, grp::A_W); v.res = grp::group_array(g, grp::A_RES); v.step = grp::group_array(g, grp::A_STEP);
    v.objective_constant = 0.0; v.fobj = nullptr;
    t->st = SolveStrides{d.N, d.n, d.nx, d.ne, d.nc, t->lay.stride[sg::A_WS], 2 * t->lay.stride[sg::A_WSM], sg::PUB_STRIDE, arr(t, sg::A_CONSTANT), arr(t, sg::A_SCALARS)};
    const size_t B = (size_t)g->members;
    GK(hipHostMalloc((void**)&t->hpub, sizeof(double) * B * (size_t)sg::PUB_STRIDE));
    std::memset(t->hpub, 0, sizeof(double) * B * (size_t)sg::PUB_STRIDE);
    GK(hipHostMalloc((void**)&t->hscalars, sizeof(double) * B * sg::DS_STRIDE));
    std::memset(t->hscalars, 0, sizeof(double) * B * sg::DS_STRIDE);
    GK(hipEventCreate(&t->ev[0])); GK(hipEventCreate(&t->ev[1]));
    t->ls = sg::Lockstep(g->members);
    t->trace_rows.assign(B, 0); t->trace_total.assign(B, 0);
    t->regularization.assign(3 * B, 0.0); t->sd_info.assign(4 * B, 0.0); t->sd_status.assign(B, 0);
    GK(hipStreamSynchronize(s->st));
    return CALIPSO_OK;
}

// ---- enqueues: the first of a group records its beginning and sends the members' scalars; the read-back closes it -------------------------------------------------
int open_group(GH* g) {
    ST* t = g->solve; KH* s = g->base;
    if (t->open) return CALIPSO_OK;
    GK(hipEventRecord(t->ev[0], s->st));
    for (int k = 0; k < g->members; ++k) {
        const sg::Member& q = t->ls.m[(size_t)k];
        double* h = t->hscalars + (size_t)k * sg::DS_STRIDE;
        h[sg::DS_KAPPA] = q.sc.kappa; h[sg::DS_TAU] = q.sc.tau; h[sg::DS_STEP_S] = q.step_size; h[sg::DS_STEP_T] = q.step_size_t;
        h[sg::DS_RHO_BEFORE] = q.rho_before; h[sg::DS_RHO] = q.sc.rho;
        h[sg::DS_TRACE_ROW] = q.phase == sg::STEPPING && t->trace_rows[(size_t)k] < t->trace_cap ? (double)t->trace_rows[(size_t)k] : -1.0;
    }
    GK(hipMemcpyAsync(arr(t, sg::A_SCALARS), t->hscalars, sizeof(double) * (size_t)g->members * sg::DS_STRIDE, hipMemcpyHostToDevice, s->st));
    t->open = true;
    return CALIPSO_OK;
}
#define LAUNCH(kernel, gridx, block, who, ...)                                                                                                            \
    do { hipLaunchKernelGGL(kernel, dim3((unsigned)(gridx), 1, (unsigned)(who).size()), dim3(block), 0, s->st, __VA_ARGS__); t->launches += 1; } while (0)
#define COMMON s->d, t->v, grp::group_strides(g), t->st, members_of(who)

void enqueue_prologue(GH* g, const std::vector<int>& who) {
    ST* t = g->solve; KH* s = g->base;
    LAUNCH(k_solve_group_prologue, t->v.grid, KT, who, COMMON);
    LAUNCH(k_solve_group_prologue_finish, 1, 64, who, COMMON);
}
int mask_trials(const calipso::Options& o) { return (int)std::min<i64>(o.max_cone_line_search + 1, calipso::CONE_MASK_TRIALS); }
void enqueue_cone_masks(GH* g, const std::vector<int>& who) {
    ST* t = g->solve; KH* s = g->base;
    const calipso::Options& o = t->ls.opt;
    LAUNCH(k_solve_group_cone_masks, t->v.grid, KT, who, COMMON, o.scaling_line_search, mask_trials(o));
    LAUNCH(k_solve_group_masks_finish, 1, 64, who, t->v, t->st, members_of(who), o.scaling_line_search, mask_trials(o));
}
void enqueue_candidate(GH* g, const std::vector<int>& who, bool from_masks, bool first) {
    ST* t = g->solve; KH* s = g->base;
    LAUNCH(k_solve_group_candidate, t->v.grid, KT, who, COMMON, from_masks ? 1 : 0, first ? 1 : 0);
    LAUNCH(k_solve_group_candidate_finish, 1, 64, who, COMMON, first ? 1 : 0);
}
void enqueue_accept(GH* g, const std::vector<int>& who, bool start) {
    ST* t = g->solve; KH* s = g->base;
    LAUNCH(k_solve_group_accept, t->v.grid, KT, who, COMMON, start ? 1 : 0);
    LAUNCH(k_solve_group_accept_finish, 1, 64, who, t->v, t->st, members_of(who));
}
void enqueue_penalty(GH* g, const std::vector<int>& who) {
    ST* t = g->solve; KH* s = g->base;
    LAUNCH(k_solve_group_penalty, 1, KT, who, grp::group_array(g, grp::A_RHO), t->st, members_of(who));
}
// the ONE read-back of a group: every member's published block, in one copy
int read_published(GH* g) {
    ST* t = g->solve; KH* s = g->base;
    GK(hipEventRecord(t->ev[1], s->st));
    GK(hipMemcpyAsync(t->hpub, t->v.pub, sizeof(double) * (size_t)g->members * (size_t)sg::PUB_STRIDE, hipMemcpyDeviceToHost, s->st));
    GK(hipStreamSynchronize(s->st));
    GK(hipGetLastError());
    float ms = 0.f; GK(hipEventElapsedTime(&ms, t->ev[0], t->ev[1]));
    t->vector_ms += ms; t->open = false;
    return CALIPSO_OK;
}
// ... and a group that reads nothing back: it ends all the same, so that the next one sends the scalars again and times only itself.  The wait keeps the pinned
// block's rule: it is rewritten only when no copy of it is in flight
int close_group(GH* g) {
    ST* t = g->solve; KH* s = g->base;
    GK(hipEventRecord(t->ev[1], s->st));
    GK(hipStreamSynchronize(s->st));
    GK(hipGetLastError());
    float ms = 0.f; GK(hipEventElapsedTime(&ms, t->ev[0], t->ev[1]));
    t->vector_ms += ms; t->open = false;
    return CALIPSO_OK;
}
#define TRY(call) do { const int rc__ = (call); if (rc__ < 0) return rc__; } while (0)

// solve! of every member: sparse_solve.hip's solve() cut at its read-backs, over the lists the lockstep gives
int solve(GH* g, int32_t* status, double* info, double* report) {
    const auto wall0 = std::chrono::steady_clock::now();
    ST* t = g->solve; KH* s = g->base;
    const KktDev& d = s->d;
    sg::Lockstep& ls = t->ls;
    t->vector_ms = 0.0; t->launches = 0; t->open = false;
    double sd[grp::R_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::fill(t->trace_rows.begin(), t->trace_rows.end(), 0); std::fill(t->trace_total.begin(), t->trace_total.end(), 0);
    for (int k = 0; k < g->members; ++k) ls.m[(size_t)k].sc = g->ls.m[(size_t)k].sc;
    ls.begin(g->ls.opt, g->continue_after_refinement_failure, d.N, d.ne, d.nc);
    {   // initialize.jl:15-48 and solve.jl:85-95 for everyone
        const std::vector<int> who = ls.everyone();
        TRY(open_group(g));
        if (ls.opt.warmstart == 0.0) LAUNCH(k_solve_group_init, t->v.grid, KT, who, COMMON);
        enqueue_penalty(g, who);
        g->have[4] = true;
        if (d.ne) LAUNCH(k_solve_group_fill_dual, blocks_of(d.ne), KT, who, COMMON, ls.opt.dual_initial);
        enqueue_accept(g, who, true);
        enqueue_prologue(g, who);
        TRY(read_published(g));
        ls.after_start(t->hpub);
    }
    g->assembled = false; g->factored = false;
    while (ls.any_live()) {
        ++ls.ticks;
        for (;;) {                                             // classify; outer-update rounds (solve.jl:356-368) until nobody needs one
            const std::vector<int> who = ls.classify(t->hpub);
            if (who.empty()) break;
            const std::vector<int> with_prologue = ls.outer_begin(who);
            TRY(open_group(g));
            if (d.ne) LAUNCH(k_solve_group_outer_update, blocks_of(d.ne), KT, who, COMMON);
            enqueue_penalty(g, who);
            if (!with_prologue.empty()) { enqueue_prologue(g, with_prologue); TRY(read_published(g)); }
            else TRY(close_group(g));                          // (everyone here ends at its outer cap: nothing to read back, but the group and its timed interval end)
            ls.outer_after(who, with_prologue);
        }
        const std::vector<int> stepping = ls.stepping();
        if (stepping.empty()) continue;
        // search_direction! (solve.jl:187) of the stepping members on the slab's residual and step
        for (int k : stepping) g->ls.m[(size_t)k].sc = ls.m[(size_t)k].sc;
        ls.regularization_in(stepping, t->regularization.data());
        double sdr[grp::R_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};
        const int rc = grp::group_search_direction(g, stepping, t->v.res, t->v.step, t->regularization.data(), t->sd_info.data(), t->sd_status.data(), sdr);
        if (rc < 0 && rc != CALIPSO_ERR_INERTIA) return rc;
        for (int i = 0; i <= grp::R_WALL_MS; ++i) sd[i] += sdr[i];
        sd[grp::R_LAST_FACTOR_ACTIVE] = sdr[grp::R_LAST_FACTOR_ACTIVE]; sd[grp::R_LAST_REFINE_ACTIVE] = sdr[grp::R_LAST_REFINE_ACTIVE];
        const std::vector<int> on = ls.after_search_direction(stepping, t->sd_status.data(), t->sd_info.data(), t->regularization.data());
        if (on.empty()) continue;
        {   // cone search (solve.jl:190-221) and the first candidate (:206-250) behind it: one read-back
            const std::vector<int>& who = on;
            TRY(open_group(g));
            enqueue_cone_masks(g, who);
            enqueue_candidate(g, who, true, true);
            TRY(read_published(g));
            ls.after_first_candidate(who, t->hpub);
        }
        for (;;) {                                             // line-search trial rounds (:254-302) for the members that reject, at their own step sizes
            const std::vector<int> who = ls.rejecting();
            if (who.empty()) break;
            TRY(open_group(g));
            enqueue_candidate(g, who, false, false);
            TRY(read_published(g));
            ls.after_trial(who, t->hpub);
        }
        const std::vector<int> who = ls.accepting();
        if (who.empty()) continue;
        TRY(open_group(g));                                    // (carries every accepting member's trace row)
        enqueue_accept(g, who, false);                         // :309-333
        if (t->trace_cap > 0) LAUNCH(k_solve_group_trace, blocks_of(d.N), KT, who, t->v, t->st, members_of(who), t->trace.p, (long long)t->trace_cap);
        for (int k : who) { if (t->trace_rows[(size_t)k] < t->trace_cap) t->trace_rows[(size_t)k] += 1; t->trace_total[(size_t)k] += 1; }
        enqueue_prologue(g, who);                              // the next step's, at the same scalars: read back with the two violations
        TRY(read_published(g));
        ls.after_accept(who, t->hpub);
    }
    GK(hipStreamSynchronize(s->st));
    GK(hipGetLastError());
    t->open = false;
    for (int k = 0; k < g->members; ++k) g->ls.m[(size_t)k].sc = ls.m[(size_t)k].sc;
    g->assembled = false; g->factored = false;               // the members left at different ticks: their K and factors are of mixed age, none is offered as current
    const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    for (int k = 0; k < g->members; ++k) {
        status[k] = ls.m[(size_t)k].status;
        if (info) ls.info(k, t->vector_ms, sd[grp::R_DEVICE_MS], wall, info + (size_t)k * sg::INFO_DOUBLES);
    }
    if (report) {
        std::copy(sd, sd + grp::R_COUNT, report);
        report[sg::R_TICKS] = (double)ls.ticks; report[sg::R_OUTER_ROUNDS] = (double)ls.outer_rounds; report[sg::R_TRIAL_ROUNDS] = (double)ls.trial_rounds;
        report[sg::R_SOLVE_HOST_WAITS] = (double)ls.host_waits + sd[grp::R_HOST_WAITS]; report[sg::R_SOLVE_LAUNCHES] = (double)t->launches + sd[grp::R_LAUNCHES];
        report[sg::R_VECTOR_MS] = t->vector_ms; report[sg::R_SEARCH_DIRECTION_MS] = sd[grp::R_DEVICE_MS]; report[sg::R_SOLVE_WALL_MS] = wall;
    }
    const int worst = ls.worst_status();
    if (worst < 0) {
        std::string who;
        for (int k = 0; k < g->members; ++k) if (ls.m[(size_t)k].status < 0) who += (who.empty() ? "" : ", ") + std::to_string(k) + " (" + std::to_string(ls.m[(size_t)k].status) + ")";
        grp::group_fail(g, worst, "calipso_hip_sparse_kkt_group_solve: members ended with an error status: " + who +
                                      "; -102: iterative refinement failed (iterative_refinement.jl:50) and a group has no `H \\ residual` fallback, the point is the last accepted iterate");
    }
    return worst;
}

int ready(GH* g, const char* entry, bool need_point) {
    const KktDev& d = g->base->d;
    const long long nnz[3] = {d.nnzL, d.nnzg, d.nnzh};
    GREFUSE(sg::check_ready(entry, g->have, nnz, g->solve && g->solve->attached, g->have[3], need_point));
    return CALIPSO_OK;
}

int qp_attach(GH* g, const char* entry, const double* q, const double* b, const double* hvec, const double* objective_constants, bool device) {
    if (!g) return CALIPSO_ERR_ARGUMENT;
    KH* s = g->base;
    const KktDev& d = s->d;
    GREFUSE(sg::check_attach(entry, d.nx, d.ne, d.nc, q, b, hvec));
    GK(hipSetDevice(s->device));
    DEVPTR(q); DEVPTR(b); DEVPTR(hvec);
    TRY(solve_state(g));
    ST* t = g->solve;
    const hipMemcpyKind kind = device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const double* src[3] = {q, b, hvec};
    const sg::Array dst[3] = {sg::A_Q, sg::A_B, sg::A_HVEC};
    for (int i = 0; i < 3; ++i) {
        const size_t count = (size_t)t->lay.stride[dst[i]] * (size_t)g->members;
        if (count) GK(hipMemcpyAsync(arr(t, dst[i]), src[i], sizeof(double) * count, kind, s->st));
    }
    // (the constants are a host array on both routes, as set_values' central_path is)
    if (objective_constants) GK(hipMemcpyAsync(arr(t, sg::A_CONSTANT), objective_constants, sizeof(double) * (size_t)g->members, hipMemcpyHostToDevice, s->st));
    else GK(hipMemsetAsync(arr(t, sg::A_CONSTANT), 0, sizeof(double) * (size_t)g->members, s->st));
    GK(hipStreamSynchronize(s->st));
    t->attached = true;
    return CALIPSO_OK;
}

int initialize(GH* g, const char* entry, const double* x0, bool device) {
    if (!g) return CALIPSO_ERR_ARGUMENT;
    KH* s = g->base;
    const KktDev& d = s->d;
    GREFUSE(sg::check_initialize(entry, d.nx, x0));
    GK(hipSetDevice(s->device));
    DEVPTR(x0);
    TRY(ready(g, entry, false));
    ST* t = g->solve;
    (void)hipGetLastError();
    if (d.nx) GK(hipMemcpy2DAsync(t->v.w, sizeof(double) * (size_t)d.N, x0, sizeof(double) * (size_t)d.nx, sizeof(double) * (size_t)d.nx, (size_t)g->members,
                                  device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->st));
    const std::vector<int> who = t->ls.everyone();
    LAUNCH(k_solve_group_init, t->v.grid, KT, who, COMMON);
    GK(hipStreamSynchronize(s->st));
    GK(hipGetLastError());
    g->have[3] = true;
    g->assembled = false; g->factored = false;               // every K and factor belongs to the points before
    return CALIPSO_OK;
}

double* resident(GH* g, int vec) {
    const SolveDev& v = g->solve->v;
    double* const p[ss::V_COUNT] = {v.w, v.cand, v.dual, v.res, v.mgrad, v.step, v.cprod, v.ctarget, v.bgrad, v.g, v.h, v.fx};
    return p[vec];
}

}  // namespace

void grp::group_solve_release(GH* g) {
    ST* t = g->solve;
    if (!t) return;
    if (t->hpub) (void)hipHostFree(t->hpub);
    if (t->hscalars) (void)hipHostFree(t->hscalars);
    for (hipEvent_t e : t->ev) if (e) (void)hipEventDestroy(e);
    delete t;
    g->solve = nullptr;
}

int grp::group_solve_set_option(GH* g, const char* name, double value) {
    if (calipso::set_solve_option(g->ls.opt, name, value)) return 1;
    const std::string n(name);
    if (n == "continue_after_refinement_failure") { g->continue_after_refinement_failure = value != 0.0; return 1; }
    if (n == "fraction_to_boundary") { for (grp::Member& q : g->ls.m) q.sc.tau = value; return 1; }
    if (n == "penalty") {                                    // every member's resident scalar
        KH* s = g->base;
        GK(hipSetDevice(s->device));
        const std::vector<double> rho((size_t)g->members, value);
        GK(hipMemcpyAsync(grp::group_array(g, grp::A_RHO), rho.data(), sizeof(double) * rho.size(), hipMemcpyHostToDevice, s->st));
        GK(hipStreamSynchronize(s->st));
        for (grp::Member& q : g->ls.m) q.sc.rho = value;
        g->have[4] = true;
        return 1;
    }
    return 0;
}

extern "C" {

int32_t calipso_hip_sparse_kkt_group_qp_attach(calipso_hip_sparse_kkt_group* g, const double* q, const double* b, const double* hvec, const double* objective_constants) {
    return qp_attach(g, "calipso_hip_sparse_kkt_group_qp_attach", q, b, hvec, objective_constants, false);
}
int32_t calipso_hip_sparse_kkt_group_qp_attach_device(calipso_hip_sparse_kkt_group* g, const double* q, const double* b, const double* hvec, const double* objective_constants) {
    return qp_attach(g, "calipso_hip_sparse_kkt_group_qp_attach_device", q, b, hvec, objective_constants, true);
}
int32_t calipso_hip_sparse_kkt_group_initialize(calipso_hip_sparse_kkt_group* g, const double* x0) { return initialize(g, "calipso_hip_sparse_kkt_group_initialize", x0, false); }
int32_t calipso_hip_sparse_kkt_group_initialize_device(calipso_hip_sparse_kkt_group* g, const double* x0) { return initialize(g, "calipso_hip_sparse_kkt_group_initialize_device", x0, true); }

int32_t calipso_hip_sparse_kkt_group_solve(calipso_hip_sparse_kkt_group* g, int32_t* status, double* info, double* report) {
    static const char* const entry = "calipso_hip_sparse_kkt_group_solve";
    if (!g) return CALIPSO_ERR_ARGUMENT;
    GREFUSE(sg::check_solve(entry, status));
    GK(hipSetDevice(g->base->device));
    TRY(ready(g, entry, true));
    (void)hipGetLastError();
    return solve(g, status, info, report);
}

int32_t calipso_hip_sparse_kkt_group_get(calipso_hip_sparse_kkt_group* g, const char* name, int64_t member, double* out, int64_t len) {
    static const char* const entry = "calipso_hip_sparse_kkt_group_get";
    if (!g) return CALIPSO_ERR_ARGUMENT;
    KH* s = g->base;
    const KktDev& d = s->d;
    GREFUSE(grp::check_member(entry, member, g->members));
    GREFUSE(sg::check_named_vector(entry, name, out, len, d.nx, d.ne, d.nc));
    GK(hipSetDevice(s->device));
    TRY(solve_state(g));
    if (len) GK(hipMemcpyAsync(out, resident(g, ss::vector_by_name(name)) + (size_t)member * (size_t)len, sizeof(double) * (size_t)len, hipMemcpyDeviceToHost, s->st));
    GK(hipStreamSynchronize(s->st));
    return CALIPSO_OK;
}

int32_t calipso_hip_sparse_kkt_group_solution_device(calipso_hip_sparse_kkt_group* g, double** p) {
    if (!g) return CALIPSO_ERR_ARGUMENT;
    if (!p) return grp::group_fail(g, CALIPSO_ERR_ARGUMENT, "calipso_hip_sparse_kkt_group_solution_device: p is NULL");
    GK(hipSetDevice(g->base->device));
    GK(hipStreamSynchronize(g->base->st));
    *p = grp::group_array(g, grp::A_W);
    return CALIPSO_OK;
}

int32_t calipso_hip_sparse_kkt_group_keep_trace(calipso_hip_sparse_kkt_group* g, int64_t rows) {
    static const char* const entry = "calipso_hip_sparse_kkt_group_keep_trace";
    if (!g) return CALIPSO_ERR_ARGUMENT;
    GREFUSE(sg::check_keep_trace(entry, rows));
    KH* s = g->base;
    GK(hipSetDevice(s->device));
    TRY(solve_state(g));
    ST* t = g->solve;
    if (rows != t->trace_cap) {                              // another row count: the members' pieces move, the trace starts again
        if (const int rc = device_grown(s, t->trace, (size_t)g->members * (size_t)rows * (size_t)std::max(s->d.N, 1)); rc < 0) return rc;
        std::fill(t->trace_rows.begin(), t->trace_rows.end(), 0); std::fill(t->trace_total.begin(), t->trace_total.end(), 0);
    }
    t->trace_cap = rows;
    return CALIPSO_OK;
}

int32_t calipso_hip_sparse_kkt_group_trace(calipso_hip_sparse_kkt_group* g, int64_t member, double* out, int64_t cap_rows, int64_t* accepted) {
    static const char* const entry = "calipso_hip_sparse_kkt_group_trace";
    if (!g) return CALIPSO_ERR_ARGUMENT;
    GREFUSE(grp::check_member(entry, member, g->members));
    GREFUSE(sg::check_trace(entry, out, cap_rows));
    KH* s = g->base;
    GK(hipSetDevice(s->device));
    TRY(solve_state(g));
    ST* t = g->solve;
    const i64 rows = std::min<i64>(t->trace_rows[(size_t)member], cap_rows);
    if (rows > 0 && s->d.N)
        GK(hipMemcpyAsync(out, t->trace.p + (size_t)member * (size_t)t->trace_cap * (size_t)s->d.N, sizeof(double) * (size_t)rows * (size_t)s->d.N, hipMemcpyDeviceToHost, s->st));
    GK(hipStreamSynchronize(s->st));
    if (accepted) *accepted = t->trace_total[(size_t)member];
    return (int32_t)rows;
}

}  // extern "C"
