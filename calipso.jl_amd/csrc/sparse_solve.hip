// sparse_solve.hip — the vector half of solve! (src/solver/solve.jl:8-377) on the sparse handle of sparse_kkt.hip, and its host driver: a whole solve! of the sparse
// conic QP   min 1/2 x'Lxx x + q'x   s.t.  gx x - b = 0,  hx x + hvec in K   with every vector resident on the device from initialize! to the converged point.
//
//   item space (sparse_solve.hpp: Layout)  every grid kernel runs over the same items: one thread per row of [x; equality; cone], then one thread per SMALL second-order
//                                      cone (dimension <= SMALL_CONE_MAX), then one WAVEFRONT per wider cone — O(dimension) work per cone either way; a cone's
//                                      barrier, gradient, product, target and violation come from its cone item, the nonnegative rows' from their row item.  Sections
//                                      begin at multiples of 64; at most GRID_CAP workgroups of 256 threads, striding beyond that.
//   QP evaluation                      evaluate! (evaluate.jl:37-121) for this problem class is a gather over the row views of Lxx, gx, hx and the column views of gx, hx
//                                      that the handle holds: qp_hessian_row / qp_equality_row / qp_cone_row / qp_dual_rows, at the solution or, on the fly, at a
//                                      candidate.  The driver reaches evaluation through these alone.
//   evaluated problems                 with a calipso_device_sparse_eval_fn (set_evaluator) the kernels that evaluate are instantiated a second time (EVAL = true): they
//                                      READ fx, g, h and the objective the evaluator wrote instead of gathering; gx'y and hx'z are still gathered, from the resident
//                                      non-zero arrays the evaluator wrote into.  The candidate splits in two kernels around the evaluator's call.  Every call is an
//                                      enqueue on the handle's stream in front of the kernel that reads it (enqueue_evaluator): no host wait is added.  The QP
//                                      instantiation (EVAL = false) is the code as it was, bit for bit.
//   reductions                         every sum is two-stage in a fixed order: a thread adds its items in stride order, a workgroup its threads by a butterfly, and
//                                      stores one partial per (quantity, workgroup) into the workspace; ONE small finishing kernel adds the partials in workgroup order,
//                                      forms the scalars and writes them into the published block.  Maxima and the cone-search masks take the same route (masks are
//                                      gathered in LDS by atomicOr on integers, which is order-independent).  No floating-point atomics: reproducible bit for bit.
//   driver (host)                      solve! through step_decisions.hpp (initial_scalars, step_norms, exit_kind, cone_step_sizes, line_search_accepts,
//                                      filter_needs_augment, central_path_update, penalty_update), the filter of sparse_solve.hpp, search_direction() of sparse_kkt.hip.
//                                      Host waits outside search_direction: accept and the next step's prologue are read back together, the masks with the first
//                                      candidate, and every further line-search trial once: 2 accepted + outer + trials in all.
// Every kernel runs on the sparse handle's stream.
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "sparse_kkt_handle.hpp"
#include "sparse_solve.hpp"                // filter, published block, item space, workspace layout, argument checks: plain host C++
#include "sparse_solve_kernels.hpp"        // SolveDev and the bodies of every kernel here (solve_body): device code, shared with sparse_solve_group.hip
#include "sparse_parameters.hpp"           // the stored patterns of dR/dtheta: their checks and the split into short and long columns: plain host C++

using calipso::i64;
using calipso::Options;
using calipso::Scalars;
using namespace calipso::sparse_kkt;
using namespace calipso::sparse_solve;
static_assert(KT == THREADS, "the workspace layout counts workgroups of KT threads");

struct calipso::sparse_kkt::SolveState {
    Layout lay;
    SolveDev v{};
    double *q = nullptr, *b = nullptr, *hvec = nullptr;
    Grown<double> trace;                          // trace_cap rows of N
    bool have_qp[3] = {false, false, false};
    i64 trace_cap = 0, trace_rows = 0, trace_total = 0;
    Filter filter;
    double* hpub = nullptr;                       // pinned: the published block on the host
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool group_open = false;
    double vector_ms = 0.0;
    i64 waits = 0;
    // the evaluated problem class: a user's evaluator instead of the QP's gathers
    calipso_device_sparse_eval_fn eval_fn = nullptr;
    void* eval_user = nullptr;
    i64 eval_np = 0;
    Grown<double> theta;                          // np parameters
    double* fobj = nullptr;                       // the objective at the solution and at the candidate
    std::vector<int64_t> pattern[6];              // host copies of the patterns, 1-based as given to create: Lxx, gx, hx (colptr, rowval)
};

namespace {

typedef calipso::sparse_kkt::SolveState SS;

// ---- the kernels: each is its body of sparse_solve_kernels.hpp (solve_body), which the group's kernels (sparse_solve_group.hip) call too ---------------------------
// EVAL: false the QP, whose evaluate! is the gathers of solve_body; true a user's evaluator, which wrote fx, g, h and the objective before the kernel runs
template <bool EVAL> __global__ __launch_bounds__(KT) void k_solve_init(const KktDev d, const SolveDev v) { solve_body::init<EVAL>(d, v); }
__global__ __launch_bounds__(KT) void k_solve_keep_slacks(const KktDev d, double* __restrict__ kept) { solve_body::keep_slacks(d, kept); }
__global__ __launch_bounds__(KT) void k_solve_fill(int count, double* __restrict__ out, double value) { solve_body::fill(count, out, value); }
template <bool EVAL> __global__ __launch_bounds__(KT) void k_solve_prologue(const KktDev d, const SolveDev v, double kappa) { solve_body::prologue<EVAL>(d, v, kappa); }
template <bool EVAL> __global__ __launch_bounds__(64) void k_solve_prologue_finish(const KktDev d, const SolveDev v, double kappa) { solve_body::prologue_finish<EVAL>(d, v, kappa); }
__global__ __launch_bounds__(KT) void k_solve_cone_masks(const KktDev d, const SolveDev v, double tau, double sls, int nk) { solve_body::cone_masks(d, v, tau, sls, nk); }
__global__ __launch_bounds__(64) void k_solve_masks_finish(const SolveDev v, double sls, int nk) { solve_body::masks_finish(v, sls, nk); }
__global__ __launch_bounds__(KT) void k_solve_candidate(const KktDev d, const SolveDev v, const double* __restrict__ alpha, double a_s, double a_t, int first) { solve_body::candidate(d, v, alpha, a_s, a_t, first); }
__global__ __launch_bounds__(KT) void k_solve_candidate_point(const KktDev d, const SolveDev v, const double* __restrict__ alpha, double a_s, double a_t, int first) { solve_body::candidate_point(d, v, alpha, a_s, a_t, first); }
__global__ __launch_bounds__(KT) void k_solve_candidate_merit(const KktDev d, const SolveDev v) { solve_body::candidate_merit(d, v); }
template <bool EVAL> __global__ __launch_bounds__(64) void k_solve_candidate_finish(const KktDev d, const SolveDev v, double kappa, int first) { solve_body::candidate_finish<EVAL>(d, v, kappa, first); }
template <bool EVAL> __global__ __launch_bounds__(KT) void k_solve_accept(const KktDev d, const SolveDev v, double a, int start) { solve_body::accept<EVAL>(d, v, a, start); }
__global__ __launch_bounds__(64) void k_solve_accept_finish(const SolveDev v) { solve_body::accept_finish(v); }
__global__ __launch_bounds__(KT) void k_solve_outer_update(const KktDev d, const SolveDev v, double rho) { solve_body::outer_update(d, v, rho); }

// ---- host -------------------------------------------------------------------------------------------------------------------------------------------------------
unsigned blocks_of(long long items) { return (unsigned)std::max<long long>((items + KT - 1) / KT, 1); }

}  // namespace

// the resident vectors, the workspace and the published block: made once per handle, by the first entry that needs them (on the handle's device: enter)
int calipso::sparse_kkt::solve_state(KH* s) {
    if (s->solve) return CALIPSO_OK;
    SS* t = new SS();
    s->solve = t;                                            // (released with the handle, whatever happens below)
    const KktDev& d = s->d;
    std::vector<int> small, wide;
    for (int j = 0; j < d.nsoc; ++j) (s->an.soc_dim[(size_t)j] <= SMALL_CONE_MAX ? small : wide).push_back(j);
    t->lay = layout(d.nx, d.ne, d.nc, (i64)small.size(), (i64)wide.size());
    t->filter = Filter((i64)s->opt.max_filter);
    SolveDev& v = t->v;
    v.rows = t->lay.rows; v.small0 = t->lay.small0; v.wide0 = t->lay.wide0; v.items = t->lay.items;
    v.n_small = (int)small.size(); v.n_wide = (int)wide.size(); v.grid = t->lay.grid;
    v.off_prologue = t->lay.off_prologue; v.off_candidate = t->lay.off_candidate; v.off_accept = t->lay.off_accept;
    int rc;
    if ((rc = device_upload(s, small, &v.small_cones)) || (rc = device_upload(s, wide, &v.wide_cones))) return rc;
    if ((rc = device_fixed(s, &t->q, (size_t)d.nx)) || (rc = device_fixed(s, &t->b, (size_t)d.ne)) || (rc = device_fixed(s, &t->hvec, (size_t)d.nc)) ||
        (rc = device_fixed(s, &v.cand, (size_t)d.N)) || (rc = device_fixed(s, &v.dual, (size_t)d.ne)) || (rc = device_fixed(s, &v.mgrad, (size_t)d.n)) ||
        (rc = device_fixed(s, &v.bgrad, (size_t)d.nc)) || (rc = device_fixed(s, &v.cprod, (size_t)d.nc)) || (rc = device_fixed(s, &v.ctarget, (size_t)d.nc)) ||
        (rc = device_fixed(s, &v.g, (size_t)d.ne)) || (rc = device_fixed(s, &v.h, (size_t)d.nc)) || (rc = device_fixed(s, &v.gcand, (size_t)d.ne)) ||
        (rc = device_fixed(s, &v.hcand, (size_t)d.nc)) || (rc = device_fixed(s, &v.fx, (size_t)d.nx)) || (rc = device_fixed(s, &v.ws, (size_t)t->lay.doubles)) ||
        (rc = device_fixed(s, &v.wsm, (size_t)t->lay.mask_ints)) || (rc = device_fixed(s, &v.pub, PUB_ALLOC_DOUBLES)) || (rc = device_fixed(s, &t->fobj, 2))) return rc;
    v.fobj = t->fobj;
    v.q = t->q; v.b = t->b; v.hvec = t->hvec; v.w = s->w; v.res = s->res; v.step = s->step;
    v.pub_masks = reinterpret_cast<unsigned*>(v.pub + PUB_DOUBLES);      // (the mask words lie inside the published block: it is read back in one copy)
    v.objective_constant = 0.0;
    KK(hipHostMalloc((void**)&t->hpub, sizeof(double) * PUB_ALLOC_DOUBLES));
    std::memset(t->hpub, 0, sizeof(double) * PUB_ALLOC_DOUBLES);
    KK(hipEventCreate(&t->ev[0])); KK(hipEventCreate(&t->ev[1]));
    return CALIPSO_OK;
}

namespace {

// ---- enqueues: each records the beginning of a timed group, the read-back closes it -----------------------------------------------------------------------------
void open_group(KH* s) { SS* t = s->solve; if (!t->group_open) { (void)hipEventRecord(t->ev[0], s->st); t->group_open = true; } }

// the evaluator at the solution (which = 0) or at the candidate (1): a stream-ordered enqueue, no host wait.  The three matrices are the handle's resident arrays: an
// evaluation that writes one leaves K and its factor behind
int enqueue_evaluator(KH* s, int which, uint32_t flags) {
    SS* t = s->solve; SolveDev& v = t->v; const KktDev& d = s->d;
    open_group(s);
    calipso_device_sparse_data out;
    out.objective = t->fobj + which; out.objective_gradient_variables = v.fx;
    out.equality_constraint = which ? v.gcand : v.g; out.cone_constraint = which ? v.hcand : v.h;
    out.lagrangian_hessian = s->Lxx; out.equality_jacobian_variables = s->gx; out.cone_jacobian_variables = s->hx;
    out.Lxx_colptr = t->pattern[0].data(); out.Lxx_rowval = t->pattern[1].data(); out.gx_colptr = t->pattern[2].data(); out.gx_rowval = t->pattern[3].data();
    out.hx_colptr = t->pattern[4].data(); out.hx_rowval = t->pattern[5].data();
    out.nx = d.nx; out.np = t->eval_np; out.ne = d.ne; out.nc = d.nc; out.nnz_Lxx = d.nnzL; out.nnz_gx = d.nnzg; out.nnz_hx = d.nnzh;
    const ParameterPatterns& pp = s->par;                    // NULL / 0 without set_parameter_patterns
    out.lagrangian_gradient_parameters = pp.set ? pp.val[0].p : nullptr; out.equality_jacobian_parameters = pp.set ? pp.val[1].p : nullptr;
    out.cone_jacobian_parameters = pp.set ? pp.val[2].p : nullptr;
    out.Lp_colptr = pp.set ? pp.host[0].data() : nullptr; out.Lp_rowval = pp.set ? pp.host[1].data() : nullptr;
    out.gp_colptr = pp.set ? pp.host[2].data() : nullptr; out.gp_rowval = pp.set ? pp.host[3].data() : nullptr;
    out.hp_colptr = pp.set ? pp.host[4].data() : nullptr; out.hp_rowval = pp.set ? pp.host[5].data() : nullptr;
    out.nnz_Lp = pp.set ? pp.nnz[0] : 0; out.nnz_gp = pp.set ? pp.nnz[1] : 0; out.nnz_hp = pp.set ? pp.nnz[2] : 0;
    const int32_t r = t->eval_fn(t->eval_user, flags, which ? v.cand : s->w, s->w + d.o_y, s->w + d.o_z, t->theta.p, &out, (void*)s->st);
    for (int i = 0; i < 3; ++i) if (flags & EVAL_MATRIX_BITS[i]) { s->have[i] = r == 0; s->assembled = false; s->factored = false; }
    if (r != 0) {
        (void)hipStreamSynchronize(s->st); (void)hipGetLastError();
        t->group_open = false;
        return fail(s, r == 1 ? CALIPSO_ERR_ARGUMENT : CALIPSO_ERR_HIP, "the device evaluator returned " + std::to_string(r) + " (flags " + std::to_string(flags) + ", " +
                                                                                (which ? "candidate" : "solution") + ")");
    }
    return CALIPSO_OK;
}
// every variable-side bit: what solve.jl:100-135 and :175-185 evaluate at a point, the dual Hessians iff constraint_tensor (residual_jacobian_variables.jl:10-16)
uint32_t prologue_flags(const Options& o) {
    return o.constraint_tensor != 0.0 ? EVAL_EVERYTHING : EVAL_EVERYTHING & ~(uint32_t)(CALIPSO_EVAL_EQUALITY_DUAL_HESSIAN | CALIPSO_EVAL_CONE_DUAL_HESSIAN);
}
#define LAUNCH_CLASS(kernel, grid, block, ...)                                                                         \
    do { if (t->eval_fn) hipLaunchKernelGGL(kernel<true>, grid, block, 0, s->st, __VA_ARGS__); else hipLaunchKernelGGL(kernel<false>, grid, block, 0, s->st, __VA_ARGS__); } while (0)

int enqueue_init(KH* s) {
    SS* t = s->solve; open_group(s);
    if (t->eval_fn) { const int rc = enqueue_evaluator(s, 0, CALIPSO_EVAL_EQUALITY); if (rc < 0) return rc; }      // r <- g(x): the point must be evaluated first
    LAUNCH_CLASS(k_solve_init, dim3((unsigned)t->v.grid), dim3(KT), s->d, t->v);
    return CALIPSO_OK;
}
int enqueue_prologue(KH* s) {
    SS* t = s->solve; open_group(s);
    if (t->eval_fn) { const int rc = enqueue_evaluator(s, 0, prologue_flags(s->opt)); if (rc < 0) return rc; }
    LAUNCH_CLASS(k_solve_prologue, dim3((unsigned)t->v.grid), dim3(KT), s->d, t->v, s->sc.kappa);
    LAUNCH_CLASS(k_solve_prologue_finish, dim3(1), dim3(64), s->d, t->v, s->sc.kappa);
    return CALIPSO_OK;
}
int mask_trials(const Options& o) { return (int)std::min<i64>(o.max_cone_line_search + 1, calipso::CONE_MASK_TRIALS); }
void enqueue_cone_masks(KH* s) {
    SS* t = s->solve; open_group(s);
    hipLaunchKernelGGL(k_solve_cone_masks, dim3((unsigned)t->v.grid), dim3(KT), 0, s->st, s->d, t->v, s->sc.tau, s->opt.scaling_line_search, mask_trials(s->opt));
    hipLaunchKernelGGL(k_solve_masks_finish, dim3(1), dim3(64), 0, s->st, t->v, s->opt.scaling_line_search, mask_trials(s->opt));
}
int enqueue_candidate(KH* s, bool from_masks, double a_s, double a_t, bool first) {
    SS* t = s->solve; open_group(s);
    const double* alpha = from_masks ? (const double*)t->v.pub : (const double*)nullptr;
    if (t->eval_fn) {
        hipLaunchKernelGGL(k_solve_candidate_point, dim3((unsigned)t->v.grid), dim3(KT), 0, s->st, s->d, t->v, alpha, a_s, a_t, first ? 1 : 0);
        { const int rc = enqueue_evaluator(s, 1, EVAL_POINT); if (rc < 0) return rc; }
        hipLaunchKernelGGL(k_solve_candidate_merit, dim3((unsigned)t->v.grid), dim3(KT), 0, s->st, s->d, t->v);
    } else hipLaunchKernelGGL(k_solve_candidate, dim3((unsigned)t->v.grid), dim3(KT), 0, s->st, s->d, t->v, alpha, a_s, a_t, first ? 1 : 0);
    LAUNCH_CLASS(k_solve_candidate_finish, dim3(1), dim3(64), s->d, t->v, s->sc.kappa, first ? 1 : 0);
    return CALIPSO_OK;
}
int enqueue_accept(KH* s, double a, bool start) {
    SS* t = s->solve; open_group(s);
    if (start && t->eval_fn) { const int rc = enqueue_evaluator(s, 0, CALIPSO_EVAL_EQUALITY); if (rc < 0) return rc; }
    LAUNCH_CLASS(k_solve_accept, dim3((unsigned)t->v.grid), dim3(KT), s->d, t->v, a, start ? 1 : 0);
    hipLaunchKernelGGL(k_solve_accept_finish, dim3(1), dim3(64), 0, s->st, t->v);
    return CALIPSO_OK;
}
void enqueue_outer_update(KH* s, double rho) {
    SS* t = s->solve; open_group(s);
    if (s->d.ne) hipLaunchKernelGGL(k_solve_outer_update, dim3(blocks_of(s->d.ne)), dim3(KT), 0, s->st, s->d, t->v, rho);
}
// the penalty lives on the device (KktDev::rho): the kernels of both halves read it there.  Written by a kernel: stream-ordered, no host wait
void enqueue_penalty(KH* s) {
    open_group(s);
    hipLaunchKernelGGL(k_solve_fill, dim3(1), dim3(KT), 0, s->st, 1, s->rho, s->sc.rho);
    s->have[4] = true;
}
// the ONE read-back of a group: the published block, whole
int read_published(KH* s) {
    SS* t = s->solve;
    open_group(s);
    KK(hipEventRecord(t->ev[1], s->st));
    KK(hipMemcpyAsync(t->hpub, t->v.pub, PUB_BYTES, hipMemcpyDeviceToHost, s->st));
    KK(hipStreamSynchronize(s->st));
    KK(hipGetLastError());
    float ms = 0.f; KK(hipEventElapsedTime(&ms, t->ev[0], t->ev[1]));
    t->vector_ms += ms; t->group_open = false; t->waits += 1;
    return CALIPSO_OK;
}
const int* host_masks(const SS* t) { return reinterpret_cast<const int*>(t->hpub + PUB_DOUBLES); }

}  // namespace

// what an entry needs resident before it enqueues anything
int calipso::sparse_kkt::solve_ready(KH* s, const char* entry, bool point) {
    static const char* const names[3] = {"Lxx", "gx", "hx"};
    const size_t need[3] = {(size_t)s->d.nnzL, (size_t)s->d.nnzg, (size_t)s->d.nnzh};
    SS* t = s->solve;
    const bool evaluated = t->eval_fn != nullptr;              // (an evaluator writes the three matrices itself, and stands where q, b, hvec stand for the QP)
    for (int i = 0; i < 3 && !evaluated; ++i) if (need[i] && !s->have[i]) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": no " + names[i] + " resident (calipso_hip_sparse_kkt_set_values first)");
    static const char* const qp[3] = {"q", "b", "hvec"};
    const size_t len[3] = {(size_t)s->d.nx, (size_t)s->d.ne, (size_t)s->d.nc};
    for (int i = 0; i < 3 && !evaluated; ++i) if (len[i] && !t->have_qp[i]) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": no " + qp[i] + " resident (calipso_hip_sparse_kkt_qp_attach first)");
    if (point && !s->have[3]) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": no point resident (calipso_hip_sparse_kkt_initialize, or set_values with w, first)");
    if (point && s->d.ne && !s->have[4]) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": no penalty resident");
    return CALIPSO_OK;
}

namespace {

int qp_attach(KH* s, const char* entry, const double* q, const double* b, const double* hvec, double objective_constant, bool device) {
    ENTER(STATE);
    DEVPTR(q); DEVPTR(b); DEVPTR(hvec);
    SS* t = s->solve;
    const hipMemcpyKind kind = device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const double* src[3] = {q, b, hvec};
    double* dst[3] = {t->q, t->b, t->hvec};
    const size_t count[3] = {(size_t)s->d.nx, (size_t)s->d.ne, (size_t)s->d.nc};
    for (int i = 0; i < 3; ++i) if (src[i] && count[i]) { KK(hipMemcpyAsync(dst[i], src[i], sizeof(double) * count[i], kind, s->st)); t->have_qp[i] = true; }
    KK(hipStreamSynchronize(s->st));
    t->v.objective_constant = objective_constant;
    t->eval_fn = nullptr; t->eval_user = nullptr;           // a handle holds one problem class: the QP replaces an evaluator
    s->par.set = false;                                      // ... and its parameter patterns go with it
    s->qp_attached = true;
    for (int i = 0; i < 3; ++i) if (count[i] && !t->have_qp[i]) s->qp_attached = false;
    return CALIPSO_OK;
}
int initialize(KH* s, const char* entry, const double* x0, bool device) {
    ENTER(STATE_READY);
    if (!x0 && s->d.nx) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": x0 is NULL");
    DEVPTR(x0);
    SS* t = s->solve;
    if (s->d.nx) KK(hipMemcpyAsync(s->w, x0, sizeof(double) * (size_t)s->d.nx, device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->st));
    { const int rc = enqueue_init(s); if (rc < 0) return rc; }
    KK(hipStreamSynchronize(s->st));
    KK(hipGetLastError());
    t->group_open = false;
    s->have[3] = true;
    s->assembled = false; s->factored = false;               // K and its factor belong to the point before
    s->slacks_kept = false;                                  // the differentiate slacks are the new point's own
    return CALIPSO_OK;
}
int set_parameters(KH* s, const char* entry, const double* theta, bool device) {
    ENTER(STATE);
    SS* t = s->solve;
    REFUSE(check_set_parameters(entry, t->eval_fn != nullptr, t->eval_np, theta));
    if (t->eval_np) DEVPTR(theta);
    if (t->eval_np) KK(hipMemcpyAsync(t->theta.p, theta, sizeof(double) * (size_t)t->eval_np, device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->st));
    KK(hipStreamSynchronize(s->st));
    return CALIPSO_OK;
}
double* resident(KH* s, int vec) {
    SolveDev& v = s->solve->v;
    double* const p[V_NAMED] = {s->w, v.cand, v.dual, s->res, v.mgrad, s->step, v.cprod, v.ctarget, v.bgrad, v.g, v.h, v.fx, nullptr,
                                s->solve->fobj, s->Lxx, s->gx, s->hx};
    return p[vec];
}

// solve!(solver)  solve.jl:8-377, laid out as calipso_hip_solve / inner_iteration of api.hip
int solve(KH* s, double info[16]) {
    const auto wall0 = std::chrono::steady_clock::now();
    SS* t = s->solve;
    const Options& o = s->opt; Scalars& sc = s->sc; const KktDev& d = s->d;
    const double* pub = t->hpub;
    t->vector_ms = 0.0; t->waits = 0; t->trace_rows = 0; t->trace_total = 0; t->group_open = false;
    s->fallback.begin_solve();
    i64 total_iterations = 1, outer = 0, accepted = 0, nfact = 0, max_rounds = 0, refine_fail = 0, trials = 0;
    int worst = 0;
    double sd_ms = 0.0;
    const auto leave = [&](int rc) {
        if (info) {
            const double out[16] = {(double)total_iterations, (double)outer, (double)accepted, (double)nfact, (double)max_rounds, (double)refine_fail, (double)worst, (double)t->waits,
                                    (double)trials, sc.kappa, sc.rho, sc.ep_last, t->vector_ms, sd_ms, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count(),
                                    (double)rc};
            std::copy(out, out + 16, info);
        }
        return rc;
    };
    int rc;
    if (o.warmstart == 0.0 && (rc = enqueue_init(s)) < 0) return leave(rc);                   // initialize.jl:15-36
    calipso::initial_scalars(o, sc);                                                          // initialize.jl:38-48
    sc.ep_last = 0.0;                                                                         // (every solve starts as a fresh solver does)
    enqueue_penalty(s);
    if (d.ne) hipLaunchKernelGGL(k_solve_fill, dim3(blocks_of(d.ne)), dim3(KT), 0, s->st, d.ne, t->v.dual, o.dual_initial);
    if ((rc = enqueue_accept(s, 0.0, true)) < 0) return leave(rc);                            // :85-86: |g|_inf, and the cone product as it lies (stale on first use)
    if ((rc = enqueue_prologue(s)) < 0) return leave(rc);                                     // (forms the cone product and target of :88-91 too)
    if ((rc = read_published(s)) < 0) return leave(rc);
    double equality_violation = pub[PUB_G_INF], cone_product_violation = pub[PUB_PRODUCT_INF];
    t->filter.reset();                                                                        // :95
    for (i64 j = 1; j <= o.max_outer_iterations; ++j) {
        outer = j;
        for (i64 i = 1; i <= o.max_residual_iterations; ++i) {
            // the published block holds the prologue of this step (:100-135, 170-172)
            const double M = pub[PUB_MERIT], theta = pub[PUB_THETA];
            const calipso::StepNorms norms = calipso::step_norms(pub, d.N, d.ne, d.nc);
            const int kind = calipso::exit_kind(o, sc.kappa, norms, equality_violation, cone_product_violation, true);      // :138-143, :165
            if (kind == 1) return leave(1);
            if (kind == 2) break;
            // :175-185: on a QP the Hessian and Jacobians are constant and the dual Hessians zero; with an evaluator they are the resident arrays the call in front of
            // this step's prologue wrote, at this point and its y, z.  The cone Jacobians are formed inside the kernels of sparse_kkt.hip
            double reg[3] = {sc.ep, sc.ep_last, sc.ed}, sdinfo[4] = {0, 0, 0, 0};
            diff_keep_slacks(s);                                                              // what differentiate! forms the cone blocks at: no host wait
            rc = search_direction(s, s->res, s->step, reg, sdinfo);                       // :187
            nfact += (i64)sdinfo[0]; max_rounds = std::max(max_rounds, (i64)sdinfo[1]);
            for (int k = 0; k < 5; ++k) sd_ms += s->ms[k];
            sd_ms += s->fallback.v[calipso::sparse_krylov::FI_DEVICE_MS];                     // (0 where no fallback ran: its events are its own, not the eight slots')
            if (rc < 0) return leave(rc);
            if (rc == CALIPSO_WARN_REFINEMENT) {
                refine_fail += 1; worst = std::max(worst, rc);
                // the reference goes on to `H \ residual` (search_direction.jl:22): with the option krylov_fallback search_direction did, by GMRES, and its step
                // (converged or not, but finite) is taken; else there is no such fallback on this handle
                if (s->fallback.step_taken) s->fallback.count_in_solve();
                else if (!s->continue_after_refinement_failure) {
                    fail(s, -100 - CALIPSO_WARN_REFINEMENT, "calipso_hip_sparse_kkt_solve: iterative refinement failed (iterative_refinement.jl:50) and this handle has no `H \\ residual` fallback; the point is the last accepted iterate");
                    return leave(-100 - CALIPSO_WARN_REFINEMENT);
                }
            }
            // cone search (:190-221) and the first candidate (:206-250) behind it, its step sizes taken from the masks on the device: one read-back
            enqueue_cone_masks(s);
            if ((rc = enqueue_candidate(s, true, 0.0, 0.0, true)) < 0) return leave(rc);
            if ((rc = read_published(s)) < 0) return leave(rc);
            double step_size = 1.0, step_size_t = 1.0;
            if (!calipso::cone_step_sizes(host_masks(t), host_masks(t) + calipso::CONE_MASK_WORDS, o, &step_size, &step_size_t)) {
                fail(s, CALIPSO_ERR_CONE_SEARCH, "cone search failure (solve.jl:210,220)");
                return leave(CALIPSO_ERR_CONE_SEARCH);
            }
            if (step_size != pub[PUB_STEP_S] || step_size_t != pub[PUB_STEP_T])
                return leave(fail(s, CALIPSO_ERR_HIP, "calipso_hip_sparse_kkt_solve: the step sizes formed on the device are not those of cone_step_sizes()"));
            double Mh = pub[PUB_CAND_MERIT], thetah = pub[PUB_CAND_THETA];
            const double dd = pub[PUB_DD];
            i64 residual_iteration = 0;
            while (residual_iteration < o.max_residual_line_search) {                         // :254-302
                if (calipso::line_search_accepts(o, t->filter.accepts(thetah, Mh), theta, M, thetah, Mh, dd, step_size)) break;
                step_size = o.scaling_line_search * step_size;
                if ((rc = enqueue_candidate(s, false, step_size, step_size_t, false)) < 0) return leave(rc);   // :268-297
                if ((rc = read_published(s)) < 0) return leave(rc);
                Mh = pub[PUB_CAND_MERIT]; thetah = pub[PUB_CAND_THETA];
                residual_iteration += 1; trials += 1;
            }
            if (residual_iteration >= o.max_residual_line_search) worst = std::max(worst, (int)CALIPSO_WARN_LINE_SEARCH);
            if (calipso::filter_needs_augment(o, theta, M, Mh, dd, step_size))                // filter.jl:81-89
                t->filter.augment((1.0 - o.violation_tolerance) * theta, M - o.merit_tolerance * theta);
            if ((rc = enqueue_accept(s, step_size, false)) < 0) return leave(rc);             // :309-333
            if (t->trace_rows < t->trace_cap) {
                KK(hipMemcpyAsync(t->trace.p + (size_t)t->trace_rows * (size_t)d.N, s->w, sizeof(double) * (size_t)d.N, hipMemcpyDeviceToDevice, s->st));
                t->trace_rows += 1;
            }
            t->trace_total += 1;
            if ((rc = enqueue_prologue(s)) < 0) return leave(rc);                             // the next step's, at the same scalars: read back with the two violations
            if ((rc = read_published(s)) < 0) return leave(rc);
            equality_violation = pub[PUB_G_INF]; cone_product_violation = pub[PUB_PRODUCT_INF];
            total_iterations += 1; accepted += 1;
        }
        calipso::central_path_update(o, sc);                                                  // :356-359
        enqueue_outer_update(s, sc.rho);                                                      // :362-364
        calipso::penalty_update(o, sc);                                                       // :365
        enqueue_penalty(s);
        t->filter.reset();                                                                    // :368
        if (j < o.max_outer_iterations) {
            if ((rc = enqueue_prologue(s)) < 0) return leave(rc);
            if ((rc = read_published(s)) < 0) return leave(rc);
        }
    }
    KK(hipStreamSynchronize(s->st));
    t->group_open = false;
    return leave(0);
}

}  // namespace

namespace calipso {
namespace sparse_kkt {

void diff_keep_slacks(KH* s) {
    if (s->d.nc) hipLaunchKernelGGL(k_solve_keep_slacks, dim3(blocks_of(2ll * s->d.nc)), dim3(KT), 0, s->st, s->d, s->dslack);
    s->slacks_kept = true;
}

int parameters_enqueue(KH* s, const char* entry) {
    if (!s->par.set || !s->solve || !s->solve->eval_fn)
        return fail(s, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": no parameter patterns set (calipso_hip_sparse_kkt_set_parameter_patterns first)");
    if (!s->have[3]) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": no point resident (calipso_hip_sparse_kkt_initialize, or set_values with w, first)");
    SS* t = s->solve;
    const bool open = t->group_open;                         // (the call belongs to no timed group of solve!)
    const int rc = enqueue_evaluator(s, 0, EVAL_PARAMETER_BITS);
    if (rc >= 0) t->group_open = open;
    return rc;
}

void solve_state_release(KH* s) {
    SS* t = s->solve;
    if (!t) return;
    if (t->hpub) (void)hipHostFree(t->hpub);
    for (hipEvent_t e : t->ev) if (e) (void)hipEventDestroy(e);
    delete t;
    s->solve = nullptr;
}

int solve_set_option(KH* s, const char* name, double value) {
    if (calipso::set_solve_option(s->opt, name, value)) {
        if (s->solve && !std::strcmp(name, "max_filter")) s->solve->filter = Filter((i64)s->opt.max_filter);
        return 1;
    }
    const std::string n(name);
    if (n == "continue_after_refinement_failure") { s->continue_after_refinement_failure = value != 0.0; return 1; }
    if (n == "fraction_to_boundary") { s->sc.tau = value; return 1; }
    if (n == "penalty") {
        if (hipSetDevice(s->device) != hipSuccess) return fail(s, CALIPSO_ERR_HIP, "hipSetDevice");
        { const int rc = solve_state(s); if (rc < 0) return rc; }
        s->sc.rho = value;
        enqueue_penalty(s);
        if (hipStreamSynchronize(s->st) != hipSuccess) return fail(s, CALIPSO_ERR_HIP, "hipStreamSynchronize");
        s->solve->group_open = false;
        return 1;
    }
    return 0;
}

}  // namespace sparse_kkt
}  // namespace calipso

extern "C" {

int32_t calipso_hip_sparse_kkt_qp_attach(calipso_hip_sparse_kkt* s, const double* q, const double* b, const double* hvec, double objective_constant) {
    return qp_attach(s, "calipso_hip_sparse_kkt_qp_attach", q, b, hvec, objective_constant, false);
}
int32_t calipso_hip_sparse_kkt_qp_attach_device(calipso_hip_sparse_kkt* s, const double* q, const double* b, const double* hvec, double objective_constant) {
    return qp_attach(s, "calipso_hip_sparse_kkt_qp_attach_device", q, b, hvec, objective_constant, true);
}

int32_t calipso_hip_sparse_kkt_initialize(calipso_hip_sparse_kkt* s, const double* x0) { return initialize(s, "calipso_hip_sparse_kkt_initialize", x0, false); }
int32_t calipso_hip_sparse_kkt_initialize_device(calipso_hip_sparse_kkt* s, const double* x0) { return initialize(s, "calipso_hip_sparse_kkt_initialize_device", x0, true); }

int32_t calipso_hip_sparse_kkt_solve(calipso_hip_sparse_kkt* s, double info[16]) {
    static const char* const entry = "calipso_hip_sparse_kkt_solve";
    ENTER(STATE);
    if (s->d.ne && !s->have[4]) s->have[4] = true;           // (solve! sets the penalty itself: initialize.jl:44-48)
    { const int rc = solve_ready(s, entry, true); if (rc < 0) return rc; }
    (void)hipGetLastError();
    return solve(s, info);
}

int32_t calipso_hip_sparse_kkt_step_prologue(calipso_hip_sparse_kkt* s, int32_t which, double scalars[16]) {
    static const char* const entry = "calipso_hip_sparse_kkt_step_prologue";
    ENTER(STATE_POINT);
    SS* t = s->solve;
    if (which != 0) return fail(s, CALIPSO_ERR_ARGUMENT, "calipso_hip_sparse_kkt_step_prologue: which: the prologue is taken at the solution (0); calipso_hip_sparse_kkt_candidate evaluates a candidate");
    { const int rc = enqueue_prologue(s); if (rc < 0) return rc; }
    { const int rc = read_published(s); if (rc < 0) return rc; }
    if (scalars) {
        const double* p = t->hpub;
        const calipso::StepNorms n = calipso::step_norms(p, s->d.N, s->d.ne, s->d.nc);
        const double out[16] = {p[PUB_OBJECTIVE], p[PUB_BARRIER], p[PUB_MERIT], p[PUB_THETA], n.residual_violation, n.optimality, n.slack_violation, 0.0,
                                p[8], p[9], p[10], p[11], p[12], p[13], p[14], p[15]};
        std::copy(out, out + 16, scalars);
    }
    return CALIPSO_OK;
}

int32_t calipso_hip_sparse_kkt_cone_search(calipso_hip_sparse_kkt* s, double a[2]) {
    static const char* const entry = "calipso_hip_sparse_kkt_cone_search";
    ENTER(STATE_POINT);
    SS* t = s->solve;
    if (!a) return fail(s, CALIPSO_ERR_ARGUMENT, "calipso_hip_sparse_kkt_cone_search: a is NULL");
    enqueue_cone_masks(s);
    { const int rc = read_published(s); if (rc < 0) return rc; }
    if (!calipso::cone_step_sizes(host_masks(t), host_masks(t) + calipso::CONE_MASK_WORDS, s->opt, &a[0], &a[1])) return fail(s, CALIPSO_ERR_CONE_SEARCH, "cone search failure (solve.jl:210,220)");
    return CALIPSO_OK;
}

int32_t calipso_hip_sparse_kkt_candidate(calipso_hip_sparse_kkt* s, double a_s, double a_t, double out[3]) {
    static const char* const entry = "calipso_hip_sparse_kkt_candidate";
    ENTER(STATE_POINT);
    SS* t = s->solve;
    REFUSE(check_step_sizes(entry, a_s, a_t));
    { const int rc = enqueue_candidate(s, false, a_s, a_t, true); if (rc < 0) return rc; }
    { const int rc = read_published(s); if (rc < 0) return rc; }
    if (out) { out[0] = t->hpub[PUB_CAND_MERIT]; out[1] = t->hpub[PUB_CAND_THETA]; out[2] = t->hpub[PUB_DD]; }
    return CALIPSO_OK;
}

int32_t calipso_hip_sparse_kkt_accept(calipso_hip_sparse_kkt* s, double a, double violations[2]) {
    static const char* const entry = "calipso_hip_sparse_kkt_accept";
    ENTER(STATE_POINT);
    SS* t = s->solve;
    REFUSE(check_step_sizes(entry, a, 1.0));
    { const int rc = enqueue_accept(s, a, false); if (rc < 0) return rc; }
    { const int rc = read_published(s); if (rc < 0) return rc; }
    if (violations) { violations[0] = t->hpub[PUB_G_INF]; violations[1] = t->hpub[PUB_PRODUCT_INF]; }
    s->assembled = false; s->factored = false;
    return CALIPSO_OK;
}

int32_t calipso_hip_sparse_kkt_outer_update(calipso_hip_sparse_kkt* s) {
    static const char* const entry = "calipso_hip_sparse_kkt_outer_update";
    ENTER(STATE_POINT);
    SS* t = s->solve;
    double rho = 0.0;
    KK(hipMemcpyAsync(&rho, s->rho, sizeof(double), hipMemcpyDeviceToHost, s->st));
    KK(hipStreamSynchronize(s->st));
    enqueue_outer_update(s, rho);
    KK(hipStreamSynchronize(s->st));
    t->group_open = false;
    return CALIPSO_OK;
}

int32_t calipso_hip_sparse_kkt_get(calipso_hip_sparse_kkt* s, const char* name, double* out, int64_t len) {
    static const char* const entry = "calipso_hip_sparse_kkt_get";
    ENTER(STATE);
    const i64 nnz[3] = {s->d.nnzL, s->d.nnzg, s->d.nnzh};
    if (const int m = calipso::sparse_parameters::array_by_name(name); m >= 0) {      // the three resident arrays of dR/dtheta on their stored patterns
        const std::string what = std::string(entry) + ": " + name;
        if (!s->par.set) return fail(s, CALIPSO_ERR_ARGUMENT, what + ": no parameter patterns set (calipso_hip_sparse_kkt_set_parameter_patterns first)");
        if (len != s->par.nnz[m]) return fail(s, CALIPSO_ERR_ARGUMENT, what + ": len: the stored pattern has " + std::to_string(s->par.nnz[m]) + " non-zeros, not " + std::to_string(len));
        if (!out && len > 0) return fail(s, CALIPSO_ERR_ARGUMENT, what + ": the array is NULL");
        if (len) KK(hipMemcpyAsync(out, s->par.val[m].p, sizeof(double) * (size_t)len, hipMemcpyDeviceToHost, s->st));
        KK(hipStreamSynchronize(s->st));
        return CALIPSO_OK;
    }
    REFUSE(check_named_vector(entry, name, out, len, s->d.nx, s->d.ne, s->d.nc, false, nnz));
    if (vector_by_name(name) == V_DIFFERENTIATE_SLACKS) {
        const size_t nc = (size_t)s->d.nc;
        const double* from[2] = {s->slacks_kept ? s->dslack : s->w + s->d.o_s, s->slacks_kept ? s->dslack + nc : s->w + s->d.o_t};
        for (int i = 0; i < 2 && nc; ++i) KK(hipMemcpyAsync(out + (size_t)i * nc, from[i], sizeof(double) * nc, hipMemcpyDeviceToHost, s->st));
    } else if (len) KK(hipMemcpyAsync(out, resident(s, vector_by_name(name)), sizeof(double) * (size_t)len, hipMemcpyDeviceToHost, s->st));
    KK(hipStreamSynchronize(s->st));
    return CALIPSO_OK;
}
int32_t calipso_hip_sparse_kkt_set(calipso_hip_sparse_kkt* s, const char* name, const double* in, int64_t len) {
    static const char* const entry = "calipso_hip_sparse_kkt_set";
    ENTER(STATE);
    REFUSE(check_named_vector(entry, name, in, len, s->d.nx, s->d.ne, s->d.nc, true));
    const int vec = vector_by_name(name);
    if (len) KK(hipMemcpyAsync(resident(s, vec), in, sizeof(double) * (size_t)len, hipMemcpyHostToDevice, s->st));
    KK(hipStreamSynchronize(s->st));
    if (vec == V_SOLUTION) { s->have[3] = true; s->assembled = false; s->factored = false; s->slacks_kept = false; }
    return CALIPSO_OK;
}
int32_t calipso_hip_sparse_kkt_solution_device(calipso_hip_sparse_kkt* s, double** p) {
    if (!s || !p) return fail(s, CALIPSO_ERR_ARGUMENT, "calipso_hip_sparse_kkt_solution_device: p is NULL");
    KK(hipSetDevice(s->device));
    KK(hipStreamSynchronize(s->st));
    *p = s->w;
    return CALIPSO_OK;
}

// ---- the evaluated problem class ------------------------------------------------------------------------------------------------------------------------------------
int32_t calipso_hip_sparse_kkt_set_evaluator(calipso_hip_sparse_kkt* s, calipso_device_sparse_eval_fn fn, void* user, int64_t np) {
    static const char* const entry = "calipso_hip_sparse_kkt_set_evaluator";
    ENTER(STATE);
    REFUSE(check_set_evaluator(np));
    SS* t = s->solve;
    KK(hipStreamSynchronize(s->st));                         // (nothing of the evaluator before is in flight when its user object changes hands)
    s->par.set = false;                                      // the parameter patterns belong to the evaluator they were set for
    if (!fn) { t->eval_fn = nullptr; t->eval_user = nullptr; return CALIPSO_OK; }
    if (np != t->eval_np || !t->theta.p) {                     // another count of parameters: they start as zeros
        const size_t count = (size_t)std::max<i64>(np, 1);
        if (const int rc = device_grown(s, t->theta, count); rc < 0) return rc;
        KK(hipMemsetAsync(t->theta.p, 0, sizeof(double) * count, s->st));
        t->eval_np = np;
    }
    if (t->pattern[0].empty()) {                              // the host copies an evaluator builds its address table from: 1-based, as create took them
        const ColView* cols[3] = {&s->an.Lxx_cols, &s->an.gx_cols, &s->an.hx_cols};
        for (int m = 0; m < 3; ++m) {
            for (int p : cols[m]->ptr) t->pattern[2 * m].push_back((int64_t)p + 1);
            for (int r : cols[m]->row) t->pattern[2 * m + 1].push_back((int64_t)r + 1);
        }
    }
    t->eval_fn = fn; t->eval_user = user;
    for (int i = 0; i < 3; ++i) t->have_qp[i] = false;       // a handle holds one problem class: the evaluator replaces the QP
    s->qp_attached = false;
    return CALIPSO_OK;
}
int32_t calipso_hip_sparse_kkt_set_parameters(calipso_hip_sparse_kkt* s, const double* theta) { return set_parameters(s, "calipso_hip_sparse_kkt_set_parameters", theta, false); }
int32_t calipso_hip_sparse_kkt_set_parameters_device(calipso_hip_sparse_kkt* s, const double* theta) { return set_parameters(s, "calipso_hip_sparse_kkt_set_parameters_device", theta, true); }
int32_t calipso_hip_sparse_kkt_evaluate(calipso_hip_sparse_kkt* s, int32_t which, uint32_t flags) {
    static const char* const entry = "calipso_hip_sparse_kkt_evaluate";
    ENTER(STATE);
    SS* t = s->solve;
    if (!t->eval_fn) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": no evaluator attached (calipso_hip_sparse_kkt_set_evaluator first)");
    REFUSE(check_evaluate(which, flags));
    if (!s->have[3]) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": no point resident (calipso_hip_sparse_kkt_initialize, or set_values with w, first)");
    (void)hipGetLastError();
    { const int rc = enqueue_evaluator(s, which, flags); if (rc < 0) return rc; }
    KK(hipStreamSynchronize(s->st));
    KK(hipGetLastError());
    t->group_open = false;
    return CALIPSO_OK;
}

// ---- the parameter Jacobians on their stored patterns (sparse_parameters.hpp) ----------------------------------------------------------------------------------------
int32_t calipso_hip_sparse_kkt_set_parameter_patterns(calipso_hip_sparse_kkt* s, const int64_t* Lp_colptr, const int64_t* Lp_rowval, const int64_t* gp_colptr,
                                                      const int64_t* gp_rowval, const int64_t* hp_colptr, const int64_t* hp_rowval) {
    static const char* const entry = "calipso_hip_sparse_kkt_set_parameter_patterns";
    ENTER(STATE);
    SS* t = s->solve;
    if (!t->eval_fn) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": no evaluator attached (calipso_hip_sparse_kkt_set_evaluator first)");
    namespace sp = calipso::sparse_parameters;
    const sp::Patterns in{{Lp_colptr, gp_colptr, hp_colptr}, {Lp_rowval, gp_rowval, hp_rowval}};
    const int64_t rows[3] = {s->d.nx, s->d.ne, s->d.nc};
    const i64 np = t->eval_np;
    REFUSE(sp::check_patterns(entry, np, rows, in));
    KK(hipStreamSynchronize(s->st));                         // (no evaluation that reads the patterns before is in flight)
    ParameterPatterns& pp = s->par;
    pp.set = false;
    const sp::Split split = sp::split_columns(np, in);
    const sp::Geometry geo = sp::geometry(np, (int64_t)split.long_columns.size());
    std::vector<int> host[7];                                // 0-based device copies: (ptr, idx) x 3, the long columns
    ParamDev d{};
    d.np = (int)np; d.n_long = (int)split.long_columns.size(); d.long0 = geo.long0;
    for (int m = 0; m < 3; ++m) {
        const i64 nnz = in.colptr[m][np] - 1;
        pp.nnz[m] = nnz;
        pp.host[2 * m].assign(in.colptr[m], in.colptr[m] + np + 1);
        pp.host[2 * m + 1].assign(in.rowval[m], in.rowval[m] + nnz);
        for (i64 j = 0; j <= np; ++j) host[2 * m].push_back((int)(in.colptr[m][j] - 1));
        for (i64 p = 0; p < nnz; ++p) host[2 * m + 1].push_back((int)(in.rowval[m][p] - 1));
    }
    host[6].assign(split.long_columns.begin(), split.long_columns.end());
    // the arrays of an earlier call are taken again where they are large enough: setting patterns repeatedly does not grow the handle
    for (int i = 0; i < 7; ++i) if (const int rc = device_grown(s, pp.ints[i], std::max<size_t>(host[i].size(), 1)); rc < 0) return rc;
    for (int m = 0; m < 3; ++m) if (const int rc = device_grown(s, pp.val[m], (size_t)std::max<i64>(pp.nnz[m], 1)); rc < 0) return rc;
    for (int i = 0; i < 7; ++i) if (!host[i].empty()) KK(hipMemcpyAsync(pp.ints[i].p, host[i].data(), sizeof(int) * host[i].size(), hipMemcpyHostToDevice, s->st));
    for (int m = 0; m < 3; ++m) {
        KK(hipMemsetAsync(pp.val[m].p, 0, sizeof(double) * (size_t)std::max<i64>(pp.nnz[m], 1), s->st));      // the values start as zeros
        d.ptr[m] = pp.ints[2 * m].p; d.idx[m] = pp.ints[2 * m + 1].p; d.val[m] = pp.val[m].p;
    }
    d.long_columns = pp.ints[6].p;
    KK(hipStreamSynchronize(s->st));                         // (the host copies above leave scope)
    pp.d = d; pp.longest = split.longest;
    pp.set = true;
    return CALIPSO_OK;
}
int32_t calipso_hip_sparse_kkt_evaluate_parameters(calipso_hip_sparse_kkt* s) {
    static const char* const entry = "calipso_hip_sparse_kkt_evaluate_parameters";
    ENTER(HANDLE);
    (void)hipGetLastError();
    { const int rc = parameters_enqueue(s, entry); if (rc < 0) return rc; }
    KK(hipStreamSynchronize(s->st));
    KK(hipGetLastError());
    return CALIPSO_OK;
}

int32_t calipso_hip_sparse_kkt_keep_trace(calipso_hip_sparse_kkt* s, int64_t rows) {
    static const char* const entry = "calipso_hip_sparse_kkt_keep_trace";
    ENTER(STATE);
    REFUSE(check_keep_trace(rows));
    SS* t = s->solve;
    if (rows > t->trace_cap) {                                // more rows than were kept: the trace starts again
        if (const int rc = device_grown(s, t->trace, (size_t)rows * (size_t)std::max(s->d.N, 1)); rc < 0) return rc;
        t->trace_rows = 0; t->trace_total = 0;
    }
    t->trace_cap = rows;
    t->trace_rows = std::min(t->trace_rows, rows);
    return CALIPSO_OK;
}
int32_t calipso_hip_sparse_kkt_trace(calipso_hip_sparse_kkt* s, double* out, int64_t cap_rows, int64_t* accepted) {
    static const char* const entry = "calipso_hip_sparse_kkt_trace";
    ENTER(STATE);
    REFUSE(check_trace(out, cap_rows));
    SS* t = s->solve;
    const i64 rows = std::min<i64>(t->trace_rows, cap_rows);
    if (rows > 0 && s->d.N) KK(hipMemcpyAsync(out, t->trace.p, sizeof(double) * (size_t)rows * (size_t)s->d.N, hipMemcpyDeviceToHost, s->st));
    KK(hipStreamSynchronize(s->st));
    if (accepted) *accepted = t->trace_total;
    return (int32_t)rows;
}

}  // extern "C"
