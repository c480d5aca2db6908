// smallnewton.hip — solve! for a BATCH of small conic QPs: one workgroup per problem instance, the whole Newton iteration resident in the compute unit's LDS.
//
// What it is: the inner loop body of solve! (src/solver/solve.jl:98-353) and its outer updates (:356-368) — evaluate!, cone!, merit / merit gradient, residual!,
// optimality_error, inertia_correction! (inertia.jl:30-80), the condensed assemble + LDL^T + search_direction_symmetric! (search_direction.jl:25-104),
// iterative_refinement! (iterative_refinement.jl:1-52), the fraction-to-boundary cone search (:190-221), the filter line search (:224-302, line_search.jl, filter.jl)
// and the accept (:309-333) — for problems so small that the general path (one launch per kernel of the step, ~130 launches, five host read-backs) is nothing but
// latency: the MPC-sized problems of the reference's auto-tuning loop (examples/autotuning/cartpole.jl:179-227: n = 89) by the thousand.  EVERY decision the
// reference's host code takes (exit tests, regularisation loop, refinement loop, step-size searches, filter) is taken on the device; ONE launch carries whole solve!s
// (or `count` Newton steps) of all instances.
//
// Scope: the device-resident QP evaluator of qp.hip (f = c x'Px + q'x, g = Ax - b, cone constraint h - Gx), or a device evaluator compiled into the caller's own
// library against include/calipso_smallnewton.hpp (set_evaluator: its entry launches its own builds of the same kernels), with nonnegative and second-order cones;
// residual_norm = constraint_norm = 1 (the defaults of options.jl).  When iterative refinement fails, the reference falls back to
// `H \ residual` (search_direction.jl:22): by default such an instance stops with status CALIPSO_WARN_REFINEMENT and is left to the general path; with the option
// lu_fallback = 1 the kernel's LU builds take the fallback themselves (a pivoted LU of the unreduced H in per-instance global scratch) and the iteration goes on.
//
// Arithmetic: the condensed system in the constraint-first order [z | y | x] of DESIGN.md 4 — closed-form pivots for the y and z blocks, S = Lsym + ep I +
// [A; -G]' Omega [A; -G] factored without pivoting in LDS, inertia = signs of the closed-form pivots + signs of D(S) (negative = #(d <= 0) as compute_inertia!).
// Iterates agree with the oracle's per accepted step to 1e-8 (tests/test_gpu_smallnewton.py); not bit for bit with the general path (other summation orders).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "internal.hpp"
#include "device_utils.hpp"
#include "smallnewton_handle.hpp"                      // the handle; include/calipso_smallnewton.hpp: Dm, Lay, Args, the device code, QpEval

namespace {
using calipso::Options;
using namespace calipso::sn;
using namespace calipso::snh;

thread_local std::string g_sn_err;

}  // namespace

namespace calipso {
namespace snh {
int fail(SN* s, int code, const std::string& msg) { s->err = msg; return code; }

Dm dims_of(const SN* s) {
    Dm d; d.nx = s->nx; d.ne = s->ne; d.nc = s->nc; d.m = s->ne + s->nc; d.n = s->nx + d.m; d.N = s->nx + 2 * s->ne + 3 * s->nc;
    d.ldz = (d.m > 0 ? d.m : 1) | 1;
    d.q = s->nq; d.nsoc = (int)s->soc_dim.size(); d.wsz = s->wsz; d.maxd = s->maxd;
    return d;
}

// a device buffer of at least `need` doubles (grown, never shrunk)
int grow(SN* s, double** p, size_t* cap, size_t need, const char* who) {
    if (need <= *cap) return CALIPSO_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr; *cap = 0;
    if (hipMalloc((void**)p, sizeof(double) * need) != hipSuccess) {
        (void)hipGetLastError(); *p = nullptr;
        return fail(s, CALIPSO_ERR_HIP, std::string(who) + ": device allocation of " + std::to_string(sizeof(double) * need) + " bytes failed");
    }
    *cap = need;
    return CALIPSO_OK;
}
}  // namespace snh
}  // namespace calipso

namespace {
// threads per instance.  The kernel is a chain of dependent phases: a compute unit's throughput is (resident instances) / (latency of one), the latency grows slowly as
// wavefronts are taken away (C5 shape at equal residency: 92.7 / 99.7 / 121.4 us a step with 4 / 2 / 1 wavefronts), and with 256 registers per thread a compute unit
// holds 8 wavefronts.  So: as many instances as the LDS footprint allows, and the most wavefronts each that still fit — one wavefront from 6 instances per compute unit,
// two from 3, four otherwise (profiles/r06_small_newton_threads.txt; options.threads forces a count)
int sn_threads(const SN* s) {
    if (s->threads == 64 || s->threads == 128 || s->threads == 256) return s->threads;
    const size_t per = s->lds_bytes + 1280, lds = 160 * 1024;
    return 6 * per <= lds ? 64 : 3 * per <= lds ? 128 : 256;
}
// a request to the entry of the handle's evaluator (include/calipso_hip.h: calipso_smallnewton_launch)
calipso_smallnewton_launch ev_request(const SN* s, int op, int64_t* out) {
    calipso_smallnewton_launch L;
    std::memset(&L, 0, sizeof(L));
    L.op = op; L.abi = CALIPSO_SMALLNEWTON_ABI; L.out = out; L.args_bytes = (int64_t)sizeof(Args);
    L.threads = sn_threads(s); L.soc = !s->soc_dim.empty(); L.lu = s->lu; L.grid = s->batch; L.lds_bytes = (int64_t)s->lds_bytes; L.stream = (void*)s->stream;
    return L;
}
int grant_lds(SN* s) {
    if (s->lds_bytes <= 64 * 1024) return CALIPSO_OK;
    for (const bool soc : {false, true}) for (const int nt : {64, 128, 256}) {
        for (const bool lu : {false, true}) (void)calipso::lds_attribute(kernel_of<QpEval>(nt, soc, lu), 160 * 1024);
        (void)calipso::lds_attribute(diff_kernel_of<QpEval>(nt, soc), 160 * 1024);
        (void)calipso::lds_attribute(adj_kernel_of<QpEval>(nt, soc), 160 * 1024);
    }
    if (s->ev) { int64_t out[5] = {0, 0, 0, 0, 0}; calipso_smallnewton_launch L = ev_request(s, CALIPSO_SMALLNEWTON_GRANT_LDS, out); L.lds_bytes = 160 * 1024; (void)s->ev(&L); }
    return CALIPSO_OK;
}

}  // namespace

namespace calipso {
namespace snh {
using sn::QpEval;      // (calipso::QpEval is the general path's)

int launch(SN* s, int mode, int count, int advance, bool eval_rtheta, const AdjArgs* adj, bool timed) {
    if (!s->have_qp && !s->ev) return fail(s, CALIPSO_ERR_ARGUMENT, "calipso_hip_smallnewton: no problem data (calipso_hip_smallnewton_set_qp or calipso_hip_smallnewton_set_evaluator)");
    if (s->ev && s->np > 0 && !s->have_theta) return fail(s, CALIPSO_ERR_ARGUMENT, "calipso_hip_smallnewton: the evaluator takes " + std::to_string(s->np) + " parameters and none were set (calipso_hip_smallnewton_set_parameters)");
    SK(hipSetDevice(s->device));
    Args a;
    a.d = dims_of(s); a.o = s->opt;
    a.P = s->P; a.q = s->q; a.Z = s->Z; a.bh = s->bh;
    a.sP = s->sP; a.sq = s->sq; a.sZ = s->sZ; a.sbh = s->sbh;
    a.w = s->w; a.lam = s->lam; a.sc = s->sc; a.filt = s->filt; a.info = s->info; a.trace = s->trace; a.prof = s->prof; a.cnt = s->cnt; a.status = s->status;
    { const int ns = (int)s->soc_dim.size(); a.soc_start = s->d_soc; a.soc_dim = s->d_soc ? s->d_soc + ns : nullptr; a.soc_woff = s->d_soc ? s->d_soc + 2 * ns : nullptr; }
    a.batch = s->batch; a.mode = mode; a.count = count; a.advance = advance; a.trace_rows = s->trace_rows;
    a.rtheta = s->rtheta; a.sens = s->sens; a.stf = s->stf; a.srtheta = s->diff_shared ? 0 : (long long)a.d.N * (long long)count;
    a.Hs = s->Hs;
    a.theta = s->theta; a.stheta = s->theta_shared ? 0 : (long long)s->np; a.hess = s->hess; a.dpt = s->dpt; a.eval_rtheta = eval_rtheta ? 1 : 0;
    static_assert(sizeof(Args) <= 3800 && sizeof(AdjArgs) <= 3800, "kernel arguments");
    AdjArgs aa;
    if (mode == MODE_ADJ) {      // (dR/dtheta of the reverse mode in a buffer of its own, count = n_parameters columns per instance)
        aa = *adj; aa.base = a;
        aa.base.rtheta = s->adj_rt; aa.base.srtheta = (long long)a.d.N * (long long)count;
    }
    void* block = mode == MODE_ADJ ? (void*)&aa : (void*)&a;      // the kernel's one argument
    if (timed) SK(hipEventRecord(s->ev0, s->stream));
    if (s->ev) {      // the evaluator's own builds of the kernels, launched by its entry on the handle's stream
        int64_t out[5] = {0, 0, 0, 0, 0};
        calipso_smallnewton_launch L = ev_request(s, CALIPSO_SMALLNEWTON_LAUNCH, out);
        L.args = block; L.mode = mode; L.eval_rtheta = eval_rtheta ? 1 : 0;
        const int rc = s->ev(&L);
        if (rc != CALIPSO_OK) return fail(s, rc, "calipso_hip_smallnewton: the evaluator's entry refused or failed the launch (" + std::to_string(rc) + ")");
    } else {
        const int nt = sn_threads(s);
        const bool soc = !s->soc_dim.empty();
        const void* kernel = mode == MODE_ADJ ? adj_kernel_of<QpEval>(nt, soc) : mode == MODE_DIFF ? diff_kernel_of<QpEval>(nt, soc) : kernel_of<QpEval>(nt, soc, s->lu);
        void* args[] = {block};
        SK(hipLaunchKernel(kernel, dim3((unsigned)s->batch), dim3((unsigned)nt), args, s->lds_bytes, s->stream));
    }
    SK(hipGetLastError());
    if (timed) SK(hipEventRecord(s->ev1, s->stream));
    if (mode == MODE_SOLVE) SK(hipMemcpyAsync(s->solve_status, s->status, sizeof(int) * (size_t)s->batch, hipMemcpyDeviceToDevice, s->stream));
    if (!timed) return CALIPSO_OK;
    SK(hipStreamSynchronize(s->stream));
    float ms = 0.f;
    SK(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    s->last_ms = ms;
    return CALIPSO_OK;
}

}  // namespace snh
}  // namespace calipso

extern "C" {

const char* calipso_hip_smallnewton_last_error(calipso_hip_smallnewton* s) { return s ? s->err.c_str() : g_sn_err.c_str(); }

int32_t calipso_hip_smallnewton_create(int64_t nx, int64_t ne, int64_t nc, int64_t batch, int32_t device, calipso_hip_smallnewton** out) {
    if (!out) return CALIPSO_ERR_ARGUMENT;
    *out = nullptr;
    if (nx < 1 || ne < 0 || nc < 0 || batch < 1 || nx > 128 || batch > (1 << 22)) { g_sn_err = "calipso_hip_smallnewton_create: 1 <= nx <= 128, ne, nc >= 0, batch >= 1"; return CALIPSO_ERR_ARGUMENT; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) { g_sn_err = "no HIP device available (libcalipso_hip has no CPU path)"; return CALIPSO_ERR_HIP; }
    SN* s = new SN();
    s->nx = (int)nx; s->ne = (int)ne; s->nc = (int)nc; s->batch = (int)batch; s->device = device;
    s->nq = (int)nc;                                  // all cone entries nonnegative until calipso_hip_smallnewton_set_cones says otherwise
    *out = s;
    const Dm d = dims_of(s);
    s->lds_bytes = sizeof(double) * (size_t)layout(d).total;
    if (s->lds_bytes > 160 * 1024) return fail(s, CALIPSO_ERR_ARGUMENT, "calipso_hip_smallnewton_create: the problem does not fit the 160 KB of LDS of a compute unit (" + std::to_string(s->lds_bytes) + " bytes): the general path takes it");
    SK(hipSetDevice(device));
    grant_lds(s);
    SK(hipStreamCreateWithFlags(&s->own_stream, hipStreamNonBlocking));
    s->stream = s->own_stream;
    SK(hipEventCreate(&s->ev0)); SK(hipEventCreate(&s->ev1)); SK(hipEventCreateWithFlags(&s->ev_order, hipEventDisableTiming));
    const size_t B = (size_t)batch, N = (size_t)d.N;
    auto alloc = [&](double** p, size_t n) { if (hipMalloc((void**)p, sizeof(double) * std::max<size_t>(n, 1)) != hipSuccess) return false; return hipMemsetAsync(*p, 0, sizeof(double) * std::max<size_t>(n, 1), s->stream) == hipSuccess; };
    if (!alloc(&s->w, B * N) || !alloc(&s->lam, B * std::max(1, d.ne)) || !alloc(&s->sc, B * SC_COUNT) || !alloc(&s->filt, B * 6 * (size_t)s->opt.max_filter) || !alloc(&s->info, B * IN_COUNT) || !alloc(&s->prof, 16) || !alloc(&s->stf, B * 2 * (size_t)std::max(1, d.nc)))
        return fail(s, CALIPSO_ERR_HIP, "calipso_hip_smallnewton_create: device allocation failed");
    SK(hipMalloc((void**)&s->cnt, sizeof(long long) * B * CN_COUNT)); SK(hipMemsetAsync(s->cnt, 0, sizeof(long long) * B * CN_COUNT, s->stream));
    SK(hipMalloc((void**)&s->status, sizeof(int) * B)); SK(hipMemsetAsync(s->status, 0, sizeof(int) * B, s->stream));
    SK(hipMalloc((void**)&s->solve_status, sizeof(int) * B)); SK(hipMemsetAsync(s->solve_status, 0, sizeof(int) * B, s->stream));
    {   // solver.jl:81-85 defaults of the scalars
        std::vector<double> sc(B * SC_COUNT, 0.0);
        for (size_t k = 0; k < B; ++k) { sc[k * SC_COUNT + SC_KAPPA] = 0.1; sc[k * SC_COUNT + SC_TAU] = 0.99; sc[k * SC_COUNT + SC_RHO] = 10.0; }
        SK(hipMemcpyAsync(s->sc, sc.data(), sizeof(double) * sc.size(), hipMemcpyHostToDevice, s->stream));
        SK(hipStreamSynchronize(s->stream));
    }
    return CALIPSO_OK;
}

int32_t calipso_hip_smallnewton_destroy(calipso_hip_smallnewton* s) {
    if (!s) return CALIPSO_OK;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    if (s->own_stream && s->own_stream != s->stream) (void)hipStreamSynchronize(s->own_stream);
    for (double* p : {s->P, s->q, s->Z, s->bh, s->theta, s->hess, s->dpt, s->w, s->lam, s->sc, s->filt, s->info, s->trace, s->prof, s->rtheta, s->sens, s->stf, s->Hs,
                      s->adj_rt, s->adj_in, s->adj_out, s->adj_gth, s->adj_gqp, s->red, s->stage}) if (p) (void)hipFree(p);
    if (s->cnt) (void)hipFree(s->cnt);
    if (s->d_soc) (void)hipFree(s->d_soc);
    if (s->status) (void)hipFree(s->status);
    if (s->solve_status) (void)hipFree(s->solve_status);
    if (s->ev0) (void)hipEventDestroy(s->ev0);
    if (s->ev1) (void)hipEventDestroy(s->ev1);
    if (s->ev_order) (void)hipEventDestroy(s->ev_order);
    if (s->own_stream) (void)hipStreamDestroy(s->own_stream);
    delete s;
    return CALIPSO_OK;
}

// The cone layout (indices.jl:45-63 in the only arrangement the reference is self-consistent for): the first n_nonnegative cone entries are nonnegative,
// the rest are n_soc second-order cones of the given dimensions, one after the other.  Dimensions 2 .. 16 (one thread per cone forms its d x d block: wider cones belong to
// the general path); n_nonnegative + sum(dims) must be nc.
int32_t calipso_hip_smallnewton_set_cones(calipso_hip_smallnewton* s, int64_t n_nonnegative, int64_t n_soc, const int64_t* dims) {
    if (!s || n_nonnegative < 0 || n_soc < 0 || (n_soc > 0 && !dims)) return CALIPSO_ERR_ARGUMENT;
    long long total = n_nonnegative;
    for (int64_t j = 0; j < n_soc; ++j) { if (dims[j] < 2 || dims[j] > 16) return fail(s, CALIPSO_ERR_ARGUMENT, "calipso_hip_smallnewton_set_cones: second-order cones of dimension 2 .. 16"); total += dims[j]; }
    if (total != s->nc) return fail(s, CALIPSO_ERR_LAYOUT, "calipso_hip_smallnewton_set_cones: n_nonnegative + sum(dims) must equal nc");
    SK(hipSetDevice(s->device));
    s->nq = (int)n_nonnegative;
    s->soc_start.clear(); s->soc_dim.clear(); s->soc_woff.clear(); s->wsz = 0; s->maxd = 0;
    int at = s->nq;
    for (int64_t j = 0; j < n_soc; ++j) { s->soc_start.push_back(at); s->soc_dim.push_back((int)dims[j]); s->soc_woff.push_back(s->wsz); at += (int)dims[j]; s->wsz += (int)(dims[j] * dims[j]); s->maxd = std::max(s->maxd, (int)dims[j]); }
    if (s->d_soc) { (void)hipFree(s->d_soc); s->d_soc = nullptr; }
    if (n_soc > 0) {
        std::vector<int> h;
        h.insert(h.end(), s->soc_start.begin(), s->soc_start.end()); h.insert(h.end(), s->soc_dim.begin(), s->soc_dim.end()); h.insert(h.end(), s->soc_woff.begin(), s->soc_woff.end());
        SK(hipMalloc((void**)&s->d_soc, sizeof(int) * h.size()));
        SK(hipMemcpy(s->d_soc, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice));
    }
    s->lds_bytes = sizeof(double) * (size_t)layout(dims_of(s)).total;
    if (s->lds_bytes > 160 * 1024) return fail(s, CALIPSO_ERR_ARGUMENT, "calipso_hip_smallnewton_set_cones: the problem no longer fits the 160 KB of LDS of a compute unit");
    grant_lds(s);
    return CALIPSO_OK;
}

// options.jl:6-59 by name (the hot-path subset)
int32_t calipso_hip_smallnewton_set_option(calipso_hip_smallnewton* s, const char* name, double value) {
    if (!s || !name) return CALIPSO_ERR_ARGUMENT;
    Options& o = s->opt;
    const std::string n = name;
#define OD(f) if (n == #f) { o.f = value; return CALIPSO_OK; }
#define OI(f) if (n == #f) { o.f = (calipso::i64)value; return CALIPSO_OK; }
    OD(scaling_line_search) OD(iterative_refinement_tolerance) OD(central_path_initial) OD(central_path_update_tolerance) OD(central_path_scaling) OD(central_path_exponent)
    OD(penalty_initial) OD(penalty_scaling) OD(dual_initial) OD(residual_tolerance) OD(optimality_tolerance) OD(slack_tolerance) OD(equality_tolerance)
    OD(complementarity_tolerance) OD(min_regularization) OD(primal_regularization_initial) OD(dual_regularization_initial) OD(max_regularization) OD(dual_regularization)
    OD(dual_regularization_exponent) OD(scaling_regularization_initial) OD(scaling_regularization) OD(scaling_regularization_last) OD(max_penalty) OD(violation_tolerance)
    OD(violation_exponent) OD(merit_tolerance) OD(merit_exponent) OD(armijo_tolerance) OD(machine_tolerance) OD(warmstart)
    OI(max_outer_iterations) OI(max_residual_iterations) OI(max_residual_line_search) OI(max_cone_line_search) OI(iterative_refinement) OI(max_iterative_refinement)
    OI(min_iterative_refinement)
#undef OD
#undef OI
    if (n == "residual_norm" || n == "constraint_norm") { if (value == 1.0) return CALIPSO_OK; return fail(s, CALIPSO_ERR_ARGUMENT, "calipso_hip_smallnewton: only the 1-norm (the default) for " + n); }
    if (n == "threads") {         // (not an option of the reference) threads per instance: 0 = chosen by the LDS footprint, 64, 128 or 256
        if (value != 0.0 && value != 64.0 && value != 128.0 && value != 256.0) return fail(s, CALIPSO_ERR_ARGUMENT, "calipso_hip_smallnewton: threads is 0 (automatic), 64, 128 or 256");
        s->threads = (int)value; return CALIPSO_OK;
    }
    if (n == "lu_fallback") {     // (not an option of the reference) 1: H \ residual in the kernel where iterative refinement fails (search_direction.jl:22), 0: stop there
        if (value != 0.0 && value != 1.0) return fail(s, CALIPSO_ERR_ARGUMENT, "calipso_hip_smallnewton: lu_fallback is 0 or 1");
        SK(hipSetDevice(s->device));
        if (value == 1.0 && !s->Hs) {
            const size_t N = (size_t)dims_of(s).N;
            SK(hipStreamSynchronize(s->stream));
            if (hipMalloc((void**)&s->Hs, sizeof(double) * (size_t)s->batch * N * N) != hipSuccess) {
                s->Hs = nullptr;
                return fail(s, CALIPSO_ERR_HIP, "calipso_hip_smallnewton: lu_fallback needs batch x N x N doubles of device memory (" + std::to_string(sizeof(double) * (size_t)s->batch * N * N) + " bytes)");
            }
        } else if (value == 0.0 && s->Hs) {
            SK(hipStreamSynchronize(s->stream));
            (void)hipFree(s->Hs); s->Hs = nullptr;
        }
        s->lu = value == 1.0;
        return CALIPSO_OK;
    }
    if (n == "max_filter") {      // filter.jl:7-13: the instances' filter pairs live in global memory (6 x max_filter doubles each): re-sized here, emptied
        if (value < 1.0 || value > 1.0e6) return fail(s, CALIPSO_ERR_ARGUMENT, "calipso_hip_smallnewton: 1 <= max_filter <= 1e6");
        if ((calipso::i64)value == (calipso::i64)o.max_filter) return CALIPSO_OK;
        SK(hipSetDevice(s->device));
        SK(hipStreamSynchronize(s->stream));
        double* nf = nullptr;
        const size_t cnt = (size_t)s->batch * 6 * (size_t)value;
        SK(hipMalloc((void**)&nf, sizeof(double) * cnt));
        SK(hipMemset(nf, 0, sizeof(double) * cnt));
        if (s->filt) (void)hipFree(s->filt);
        s->filt = nf;
        o.max_filter = (double)(calipso::i64)value;
        std::vector<long long> cn((size_t)s->batch * CN_COUNT);
        SK(hipMemcpy(cn.data(), s->cnt, sizeof(long long) * cn.size(), hipMemcpyDeviceToHost));
        for (int k = 0; k < s->batch; ++k) cn[(size_t)k * CN_COUNT + CN_FILTER] = 0;
        SK(hipMemcpy(s->cnt, cn.data(), sizeof(long long) * cn.size(), hipMemcpyHostToDevice));
        return CALIPSO_OK;
    }
    return fail(s, CALIPSO_ERR_ARGUMENT, "calipso_hip_smallnewton_set_option: unknown option " + n);
}

// min c x'Px + q'x  s.t.  Ax = b, h - Gx >= 0  (qp.hip's conventions; column-major host arrays).  shared != 0: ONE problem for all instances (the arrays hold one
// problem), else batch-major arrays (instance k at offset k * size).  The arrays go to the device as they are, into a block that lives for this call; pack_qp
// builds Lxx, Z and bh from them there.
int32_t calipso_hip_smallnewton_set_qp(calipso_hip_smallnewton* s, const double* P, const double* q, const double* A, const double* b, const double* G, const double* h,
                                       double objective_scale, int32_t shared) {
    if (!s || !P || !q || (s->ne && (!A || !b)) || (s->nc && (!G || !h))) return CALIPSO_ERR_ARGUMENT;
    SK(hipSetDevice(s->device));
    const size_t nx = s->nx, ne = s->ne, nc = s->nc, K = shared ? 1 : (size_t)s->batch;
    const double* host[6] = {P, q, A, b, G, h};
    const size_t len[6] = {K * nx * nx, K * nx, K * ne * nx, K * ne, K * nc * nx, K * nc};
    struct Block { double* p = nullptr; ~Block() { if (p) (void)hipFree(p); } } block;
    if (hipMalloc((void**)&block.p, sizeof(double) * K * qp_entries(dims_of(s))) != hipSuccess) {
        (void)hipGetLastError(); block.p = nullptr;
        return fail(s, CALIPSO_ERR_HIP, "calipso_hip_smallnewton_set_qp: device allocation of " + std::to_string(sizeof(double) * K * qp_entries(dims_of(s))) + " bytes failed");
    }
    const double* src[6];
    size_t at = 0;
    for (int i = 0; i < 6; ++i) {
        src[i] = len[i] ? block.p + at : nullptr;
        if (len[i]) SK(hipMemcpyAsync(block.p + at, host[i], sizeof(double) * len[i], hipMemcpyHostToDevice, s->stream));
        at += len[i];
    }
    const int rc = pack_qp(s, src, objective_scale, shared ? 63 : 0, 0, "calipso_hip_smallnewton_set_qp");
    SK(hipStreamSynchronize(s->stream));      // (also after a refusal: the copies read the caller's arrays and the block goes)
    return rc;
}

// a device evaluator (include/calipso_smallnewton.hpp): its entry's handshake, then the per-instance Lagrangian Hessians; replaces the QP
int32_t calipso_hip_smallnewton_set_evaluator(calipso_hip_smallnewton* s, calipso_smallnewton_kernels_fn fn, int64_t n_parameters) {
    if (!s || !fn || n_parameters < 0 || n_parameters > (1 << 20)) return CALIPSO_ERR_ARGUMENT;
    int64_t out[5] = {0, 0, 0, 0, 0};      // (out[4]: reverse mode built; an entry compiled before it answers the first four)
    calipso_smallnewton_launch L = ev_request(s, CALIPSO_SMALLNEWTON_QUERY, out);
    const int rc = fn(&L);
    if (rc != CALIPSO_OK) return fail(s, CALIPSO_ERR_ARGUMENT, "calipso_hip_smallnewton_set_evaluator: the entry refused the query (" + std::to_string(rc) + ")");
    if (out[0] != CALIPSO_SMALLNEWTON_ABI || out[1] != (int64_t)sizeof(Args) || out[2] != SN_JB)
        return fail(s, CALIPSO_ERR_ARGUMENT, "calipso_hip_smallnewton_set_evaluator: the entry was built against another calipso_smallnewton.hpp (ABI " + std::to_string(out[0]) + ", sizeof(Args) " +
                    std::to_string(out[1]) + ", SN_JB " + std::to_string(out[2]) + "; this library: ABI " + std::to_string(CALIPSO_SMALLNEWTON_ABI) + ", " + std::to_string(sizeof(Args)) + ", " +
                    std::to_string(SN_JB) + ")");
    SK(hipSetDevice(s->device));
    SK(hipStreamSynchronize(s->stream));
    for (double** p : {&s->P, &s->q, &s->Z, &s->bh, &s->theta, &s->hess, &s->dpt}) if (*p) { (void)hipFree(*p); *p = nullptr; }
    s->cap_P = s->cap_q = s->cap_Z = s->cap_bh = s->cap_theta = 0;
    s->have_qp = false; s->ev = nullptr; s->have_theta = false;
    const size_t bytes = sizeof(double) * (size_t)s->batch * (size_t)s->nx * (size_t)s->nx;
    if (hipMalloc((void**)&s->hess, bytes) != hipSuccess) {
        (void)hipGetLastError(); s->hess = nullptr;
        return fail(s, CALIPSO_ERR_HIP, "calipso_hip_smallnewton_set_evaluator: the Lagrangian Hessians need batch x nx^2 doubles of device memory (" + std::to_string(bytes) + " bytes)");
    }
    SK(hipMemset(s->hess, 0, bytes));
    const size_t pbytes = sizeof(double) * (size_t)s->batch * (size_t)(s->nx + s->ne + s->nc);
    SK(hipMalloc((void**)&s->dpt, pbytes)); SK(hipMemset(s->dpt, 0, pbytes));
    s->ev = fn; s->np = (int)n_parameters; s->ev_rtheta = out[3] != 0; s->ev_adj = out[4] == 1;
    grant_lds(s);
    return CALIPSO_OK;
}

// the parameters theta of the evaluator: batch x np (row k for instance k) or one row for all (shared != 0)
int32_t calipso_hip_smallnewton_set_parameters(calipso_hip_smallnewton* s, const double* theta, int32_t shared) {
    if (!s || !theta) return CALIPSO_ERR_ARGUMENT;
    SK(hipSetDevice(s->device));
    const int rc = put_parameters(s, theta, shared, hipMemcpyHostToDevice, "calipso_hip_smallnewton_set_parameters");
    SK(hipStreamSynchronize(s->stream));
    return rc;
}

// the points (batch x N, the layout of point.jl:13-22), the multiplier estimates lambda (batch x ne) and per instance [central_path, fraction_to_boundary, penalty]
// (batch x 3); NULL leaves what is resident.  initialize!(solver, guess) = set_state with x in the first nx entries of every point, then solve (cold start).
int32_t calipso_hip_smallnewton_set_state(calipso_hip_smallnewton* s, const double* w, const double* lambda, const double* scalars) {
    if (!s) return CALIPSO_ERR_ARGUMENT;
    SK(hipSetDevice(s->device));
    const Dm d = dims_of(s);
    const size_t B = s->batch;
    const double* host[3] = {w, d.ne ? lambda : nullptr, scalars};
    const size_t len[3] = {B * d.N, B * d.ne, B * 3};
    { const int rc = grow(s, &s->stage, &s->cap_stage, len[0] + len[1] + len[2], "calipso_hip_smallnewton_set_state"); if (rc < 0) return rc; }
    const double* dev[3];
    size_t at = 0;
    for (int i = 0; i < 3; ++i) {
        dev[i] = host[i] ? s->stage + at : nullptr;
        if (host[i]) SK(hipMemcpyAsync(s->stage + at, host[i], sizeof(double) * len[i], hipMemcpyHostToDevice, s->stream));
        at += len[i];
    }
    const int rc = put_state(s, dev[0], nullptr, w ? 1 : 0, dev[1], dev[2]);
    SK(hipStreamSynchronize(s->stream));
    return rc;
}

// points, lambda, scalars [central_path, fraction_to_boundary, penalty, primal_regularization, primal_regularization_last, dual_regularization] (batch x 6),
// counters [total_iterations, outer, factorizations, refinement_failures, max_refinement_rounds, last_refinement_rounds, newton_steps, accepted iterates] (batch x 8); NULLs skipped
int32_t calipso_hip_smallnewton_get_state(calipso_hip_smallnewton* s, double* w, double* lambda, double* scalars, int64_t* counters) {
    if (!s) return CALIPSO_ERR_ARGUMENT;
    SK(hipSetDevice(s->device));
    const Dm d = dims_of(s);
    const size_t B = s->batch;
    if (w) SK(hipMemcpyAsync(w, s->w, sizeof(double) * B * d.N, hipMemcpyDeviceToHost, s->stream));
    if (lambda && d.ne) SK(hipMemcpyAsync(lambda, s->lam, sizeof(double) * B * d.ne, hipMemcpyDeviceToHost, s->stream));
    std::vector<double> sc(B * SC_COUNT); std::vector<long long> cn(B * CN_COUNT);
    SK(hipMemcpyAsync(sc.data(), s->sc, sizeof(double) * sc.size(), hipMemcpyDeviceToHost, s->stream));
    SK(hipMemcpyAsync(cn.data(), s->cnt, sizeof(long long) * cn.size(), hipMemcpyDeviceToHost, s->stream));
    SK(hipStreamSynchronize(s->stream));
    for (size_t k = 0; k < B; ++k) {
        if (scalars) { const double* r = sc.data() + k * SC_COUNT; double* o = scalars + 6 * k; o[0] = r[SC_KAPPA]; o[1] = r[SC_TAU]; o[2] = r[SC_RHO]; o[3] = r[SC_EP]; o[4] = r[SC_EPLAST]; o[5] = r[SC_ED]; }
        if (counters) { const long long* r = cn.data() + k * CN_COUNT; int64_t* o = counters + 8 * k; o[0] = r[CN_TOTAL]; o[1] = r[CN_OUTER]; o[2] = r[CN_FACT]; o[3] = r[CN_RFAIL]; o[4] = r[CN_RMAX]; o[5] = r[CN_RLAST]; o[6] = r[CN_STEPS]; o[7] = r[CN_TRACE]; }
    }
    return CALIPSO_OK;
}

// keep the first `rows` accepted iterates of every instance (solution.all after each accepted inner iteration, solve.jl:309-326): what tests compare with the oracle's trace
int32_t calipso_hip_smallnewton_trace(calipso_hip_smallnewton* s, int32_t rows, double* out) {
    if (!s || rows < 0) return CALIPSO_ERR_ARGUMENT;
    SK(hipSetDevice(s->device));
    const Dm d = dims_of(s);
    if (out) {      // read the rows recorded so far
        if (!s->trace || rows > s->trace_rows) return fail(s, CALIPSO_ERR_ARGUMENT, "calipso_hip_smallnewton_trace: no trace of that many rows was requested");
        std::vector<double> all((size_t)s->batch * s->trace_rows * d.N);
        SK(hipMemcpy(all.data(), s->trace, sizeof(double) * all.size(), hipMemcpyDeviceToHost));
        for (int k = 0; k < s->batch; ++k) std::memcpy(out + (size_t)k * rows * d.N, all.data() + (size_t)k * s->trace_rows * d.N, sizeof(double) * (size_t)rows * d.N);
        return CALIPSO_OK;
    }
    if (s->trace) { (void)hipFree(s->trace); s->trace = nullptr; }
    s->trace_rows = rows;
    if (rows > 0) { SK(hipMalloc((void**)&s->trace, sizeof(double) * (size_t)s->batch * rows * d.N)); SK(hipMemset(s->trace, 0, sizeof(double) * (size_t)s->batch * rows * d.N)); }
    return CALIPSO_OK;
}

// solve!(solver) for every instance in ONE launch (cold start unless opt.warmstart: x from the resident points).  result[k] = 1 converged, 0 iteration caps reached,
// CALIPSO_ERR_INERTIA / CALIPSO_ERR_CONE_SEARCH as the reference's error()s, -100 - CALIPSO_WARN_REFINEMENT where the reference would fall back to H \ residual
// (lu_fallback = 0), -100 - CALIPSO_WARN_ZERO_PIVOT where that fallback met an exactly singular H (lu_fallback = 1).
int32_t calipso_hip_smallnewton_solve(calipso_hip_smallnewton* s, int32_t* result, double* ms) {
    if (!s) return CALIPSO_ERR_ARGUMENT;
    const int rc = launch(s, MODE_SOLVE, 0, 1, false, nullptr, true);
    if (rc < 0) return rc;
    if (result) SK(hipMemcpy(result, s->status, sizeof(int) * (size_t)s->batch, hipMemcpyDeviceToHost));
    if (ms) *ms = s->last_ms;
    return CALIPSO_OK;
}

// `count` Newton steps (the inner loop body of solve!) of every instance in ONE launch from the resident state; advance = 0: every step starts from the same state
// (the benchmark step of calipso_hip_newton_step).  info: batch x 8 [step_size, step_size_t, refinement rounds, factorisations, merit and violation of the accepted
// candidate, exit kind (2: inner-loop exit of solve.jl:165, no step), optimality error] of the LAST step; status as calipso_hip_smallnewton_solve (0: stepped).
int32_t calipso_hip_smallnewton_steps(calipso_hip_smallnewton* s, int32_t count, int32_t advance, double* info, int32_t* status, double* ms) {
    if (!s || count < 0) return CALIPSO_ERR_ARGUMENT;
    const int rc = launch(s, MODE_STEPS, count, advance, false, nullptr, true);
    if (rc < 0) return rc;
    if (info) SK(hipMemcpy(info, s->info, sizeof(double) * (size_t)s->batch * IN_COUNT, hipMemcpyDeviceToHost));
    if (status) SK(hipMemcpy(status, s->status, sizeof(int) * (size_t)s->batch, hipMemcpyDeviceToHost));
    if (ms) *ms = s->last_ms;
    return CALIPSO_OK;
}

// differentiate!(solver) for every instance in ONE launch (differentiate.jl:1-61) at the resident points (after calipso_hip_smallnewton_solve): one factorisation of
// the condensed matrix with the regularisation solve! left, then search_direction_symmetric! per column of dR/dtheta and sensitivity = -1.0 * the result.
// jacobian_parameters: batch x (N x p), column-major per instance (host), or ONE N x p matrix for all instances (shared != 0: the model of an MPC loop is the same
// for every problem); sensitivity: batch x (N x p).  status[k]: 0, or 1 when the factorisation's inertia is not (nx, ne + nc, 0).
namespace {
// the dR/dtheta buffer and the sensitivities (batch x N x p each)
int diff_buffers(SN* s, size_t need) {
    const int rc = grow(s, &s->rtheta, &s->cap_rtheta, need, "calipso_hip_smallnewton_differentiate");
    return rc < 0 ? rc : grow(s, &s->sens, &s->cap_sens, need, "calipso_hip_smallnewton_differentiate");
}
}  // namespace

int32_t calipso_hip_smallnewton_differentiate(calipso_hip_smallnewton* s, int64_t p, int32_t shared, const double* jacobian_parameters, double* sensitivity, int32_t* status, double* ms) {
    if (!s || p < 1 || p > (1 << 20) || !jacobian_parameters || !sensitivity) return CALIPSO_ERR_ARGUMENT;
    SK(hipSetDevice(s->device));
    const Dm d = dims_of(s);
    const size_t need = (size_t)s->batch * (size_t)d.N * (size_t)p;
    { const int rc = diff_buffers(s, need); if (rc < 0) return rc; }
    SK(hipMemcpyAsync(s->rtheta, jacobian_parameters, sizeof(double) * (shared ? (size_t)d.N * (size_t)p : need), hipMemcpyHostToDevice, s->stream));
    s->diff_shared = shared != 0;
    const int rc = launch(s, MODE_DIFF, (int)p, 0, false, nullptr, true);
    if (rc < 0) return rc;
    SK(hipMemcpy(sensitivity, s->sens, sizeof(double) * need, hipMemcpyDeviceToHost));
    if (status) SK(hipMemcpy(status, s->status, sizeof(int) * (size_t)s->batch, hipMemcpyDeviceToHost));
    if (ms) *ms = s->last_ms;
    return CALIPSO_OK;
}

// differentiate! with dR/dtheta from the evaluator (residual_jacobian_parameters.jl:1-40 at the resident points, p = n_parameters columns): as above otherwise
int32_t calipso_hip_smallnewton_differentiate_parameters(calipso_hip_smallnewton* s, double* sensitivity, int32_t* status, double* ms) {
    if (!s || !sensitivity) return CALIPSO_ERR_ARGUMENT;
    if (!s->ev || !s->ev_rtheta || s->np < 1)
        return fail(s, CALIPSO_ERR_ARGUMENT, "calipso_hip_smallnewton_differentiate_parameters: needs an evaluator that provides dR/dtheta and has parameters");
    SK(hipSetDevice(s->device));
    const Dm d = dims_of(s);
    const size_t need = (size_t)s->batch * (size_t)d.N * (size_t)s->np;
    { const int rc = diff_buffers(s, need); if (rc < 0) return rc; }
    s->diff_shared = false;
    const int rc = launch(s, MODE_DIFF, s->np, 0, true, nullptr, true);
    if (rc < 0) return rc;
    SK(hipMemcpy(sensitivity, s->sens, sizeof(double) * need, hipMemcpyDeviceToHost));
    if (status) SK(hipMemcpy(status, s->status, sizeof(int) * (size_t)s->batch, hipMemcpyDeviceToHost));
    if (ms) *ms = s->last_ms;
    return CALIPSO_OK;
}

// differentiate! in reverse mode (differentiate.jl:1-61 transposed): for k cotangents v per instance, lambda = M' v for the map M that
// calipso_hip_smallnewton_differentiate applies to a column of dR/dtheta (the same factorisation; refinement against H' for batches without second-order
// cones, none with them: quirk B-3), then grad = -R_theta' lambda = S' v for the S that differentiate would return.  R_theta: the evaluator's dR/dtheta at the
// resident points (grad_theta), or the built-in QP's data (grad_qp: P, q, A, b, G, h in set_qp's column-major block order, P's gradient symmetric).
int32_t calipso_hip_smallnewton_differentiate_adjoint(calipso_hip_smallnewton* s, int64_t k, const double* cotangent, double* adjoint, double* grad_theta, double* grad_qp,
                                                      int32_t* status, double* ms) {
    if (!s) return CALIPSO_ERR_ARGUMENT;
    const char* me = "calipso_hip_smallnewton_differentiate_adjoint";
    int rc = adjoint_refusals(s, k, cotangent != nullptr, grad_theta != nullptr, grad_qp != nullptr);
    if (rc < 0) return rc;
    SK(hipSetDevice(s->device));
    const Dm d = dims_of(s);
    const size_t B = (size_t)s->batch, N = (size_t)d.N, K = (size_t)k;
    rc = grow(s, &s->adj_in, &s->cap_adj_in, B * N * K, me);
    if (rc == CALIPSO_OK && adjoint) rc = grow(s, &s->adj_out, &s->cap_adj_out, B * N * K, me);
    if (rc == CALIPSO_OK && grad_theta) rc = grow(s, &s->adj_gth, &s->cap_adj_gth, B * K * (size_t)s->np, me);
    if (rc < 0) return rc;
    SK(hipMemcpyAsync(s->adj_in, cotangent, sizeof(double) * B * N * K, hipMemcpyHostToDevice, s->stream));
    rc = calipso::snh::adjoint(s, k, s->adj_in, adjoint ? s->adj_out : nullptr, grad_theta ? s->adj_gth : nullptr, grad_qp != nullptr, true);
    if (rc < 0) return rc;
    if (adjoint) SK(hipMemcpy(adjoint, s->adj_out, sizeof(double) * B * N * K, hipMemcpyDeviceToHost));
    if (grad_theta) SK(hipMemcpy(grad_theta, s->adj_gth, sizeof(double) * B * K * (size_t)s->np, hipMemcpyDeviceToHost));
    if (grad_qp) SK(hipMemcpy(grad_qp, s->adj_gqp, sizeof(double) * B * K * qp_entries(d), hipMemcpyDeviceToHost));
    if (status) SK(hipMemcpy(status, s->status, sizeof(int) * B, hipMemcpyDeviceToHost));
    if (ms) *ms = s->last_ms;
    return CALIPSO_OK;
}

// phase clocks of instance 0 in the last launch, microseconds (a build with -DSN_TRACE; zeros otherwise): [0] evaluation + residual + norms, [1] inertia logic, [2] cone
// weights + assembly of S, [3] LDL^T, [4] first condensed solve, [5] refinement, [6] cone search + candidate, [7] candidate merit + line search, [8] accept, [9] of the LDL^T: the panels (one wavefront), [3] then holds its trailing updates, [11] between steps
// out = {threads per instance, LDS bytes per instance, instances a compute unit holds (the runtime's occupancy query for the kernel launch() would pick), compute units}
int32_t calipso_hip_debug_smallnewton_describe(calipso_hip_smallnewton* s, double out[4]) {
    if (!s || !out) return CALIPSO_ERR_ARGUMENT;
    SK(hipSetDevice(s->device));
    const int nt = sn_threads(s);
    int per = 0, cus = 0;
    if (s->ev) {      // the evaluator's build: its entry answers
        int64_t o1[5] = {0, 0, 0, 0, 0};
        const calipso_smallnewton_launch L = ev_request(s, CALIPSO_SMALLNEWTON_OCCUPANCY, o1);
        const int rc = s->ev(&L);
        if (rc != CALIPSO_OK) return fail(s, rc, "calipso_hip_debug_smallnewton_describe: the evaluator's entry failed the occupancy query");
        per = (int)o1[0];
    } else SK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel_of<QpEval>(nt, !s->soc_dim.empty(), s->lu), nt, s->lds_bytes));
    SK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device));
    out[0] = nt; out[1] = (double)s->lds_bytes; out[2] = per; out[3] = cus;
    return CALIPSO_OK;
}

int32_t calipso_hip_debug_smallnewton_profile(calipso_hip_smallnewton* s, double out[12]) {
    if (!s || !out) return CALIPSO_ERR_ARGUMENT;
    SK(hipMemcpy(out, s->prof, sizeof(double) * 12, hipMemcpyDeviceToHost));
    return CALIPSO_OK;
}

}  // extern "C"
