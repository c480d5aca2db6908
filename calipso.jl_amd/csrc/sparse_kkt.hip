// sparse_kkt.hip — search_direction! (src/solver/search_direction.jl:1-23) on SPARSE problem data resident on the device: the handle behind
// calipso_hip_sparse_kkt_* (include/calipso_hip.h).  Nothing here is dense: memory is O(nnz(Lxx) + nnz(gx) + nnz(hx) + nnz(L)).
//
//   analyse (host, once per pattern)   sparse_kkt.hpp: the pattern of triu(K) of jacobian_variables_symmetric, the slot of K.nzval of every input non-zero,
//                                      diagonal and cone-block entry, row views of Lxx, gx, hx; then a calipso_hip_sparse of that pattern (sparse.hip).
//   assemble (device, ONE launch)      residual_jacobian_variables! + residual_jacobian_variables_symmetric! (residual_jacobian_variables.jl:1-167) without ever
//                                      forming H: one thread per written entry of K.nzval; the second-order blocks one thread per (cone, column) through the closed
//                                      form of second_order_matrix_inverse (cones/second_order.jl:50-65, first-row quirk kept), O(dimension) per column.
//   H v (device, two launches)         the unreduced N x N matrix applied from the same data: the rows that gather from Lxx, gx, hx (one thread per row, or one
//                                      wavefront per row where the rows are long), and the r-, s-, t-rows (one thread each); fused with residual - H step and
//                                      its infinity norm, so a refinement round reads back one double.
//   the condensed map, k columns       step = M residual of search_direction_symmetric! (search_direction.jl:25-104) and its transpose: map_columns — a "pre" launch
//                                      (residual_symmetric!, residual.jl:53-101), ONE calipso_hip_sparse_solve_device for all k columns, a "post" launch (the recovery,
//                                      search_direction.jl:59-101).  One thread per (row, column), one per (second-order cone, column); blockIdx.y carries the column.  The
//                                      row arithmetic is sparse_differentiate.hpp's, the only copy: solve_symmetric is the forward map with one column.
//   driver (host)                      inertia_correction! (inertia.jl:30-80) and iterative_refinement! (iterative_refinement.jl:1-52) through ic_begin / ic_after /
//                                      refine_next of step_decisions.hpp; every retry is one assemble + one calipso_hip_sparse_factorize_device.
//   H \ residual (option krylov_fallback)  where the refinement fails (search_direction.jl:22): restarted right-preconditioned GMRES on H with solve_symmetric as
//                                      preconditioner, gmres() below over the kernels of sparse_krylov.hip and the host logic of sparse_krylov.hpp; also the entry
//                                      calipso_hip_sparse_kkt_solve_nonsymmetric.
// Every kernel runs on the sparse handle's stream.  Gathers only: no atomics on values, a fixed summation order, results reproducible bit for bit.
// The kernels' bodies are the __device__ functions of sparse_kkt_kernels.hpp: sparse_kkt_group.hip steps groups of same-pattern problems through the same arithmetic.
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "sparse_kkt_handle.hpp"           // the handle, KktDev, and (through sparse_kkt.hpp) the analysis: plain host C++
#include "sparse_kkt_kernels.hpp"          // the kernels' bodies (and through it sparse_differentiate.hpp: the row arithmetic of the condensed maps, arrow_inverse)

using calipso::i64;
using calipso::Options;
using calipso::Scalars;
using namespace calipso::sparse_kkt;
using namespace calipso::sparse_differentiate;
static_assert(REFUSED_ARGUMENT == CALIPSO_ERR_ARGUMENT, "a refused pattern is an argument error");

namespace {

// the kernels: one thread per item, the arithmetic in sparse_kkt_kernels.hpp (the copy the group's kernels call too)
__global__ __launch_bounds__(KT) void k_kkt_assemble(const KktDev d, double ep, double ed, double* __restrict__ K) { assemble_item(d, ep, ed, K); }

template <bool WAVE>
__global__ __launch_bounds__(KT) void k_kkt_mul_gathered(const KktDev d, double ep, double ed, const double* __restrict__ v, const Sink sink) { mul_gathered_item<WAVE>(d, ep, ed, v, sink); }

__global__ __launch_bounds__(KT) void k_kkt_mul_local(const KktDev d, double ep, double ed, const double* __restrict__ v, const Sink sink) { mul_local_item(d, ep, ed, v, sink); }

// the condensed solve's outer halves: G (n x k) from V (N x k) before the LDL^T solve, OUT (N x k) from its solution Hs (n x k) and V after it; blockIdx.y: the column
template <bool TRANSPOSED>
__global__ __launch_bounds__(KT) void k_kkt_map_pre(const KktDev d, double ep, double ed, const double* __restrict__ V, double* __restrict__ G, double* __restrict__ OUT) {
    const size_t col = blockIdx.y;
    map_pre_item<TRANSPOSED>(d, ep, ed, V + col * (size_t)d.N, G + col * (size_t)d.n, OUT + col * (size_t)d.N);
}

template <bool TRANSPOSED>
__global__ __launch_bounds__(KT) void k_kkt_map_post(const KktDev d, double ep, double ed, const double* __restrict__ Hs, const double* __restrict__ V, double* __restrict__ OUT) {
    const size_t col = blockIdx.y;
    map_post_item<TRANSPOSED>(d, ep, ed, Hs + col * (size_t)d.n, V + col * (size_t)d.N, OUT + col * (size_t)d.N);
}

__global__ __launch_bounds__(KT) void k_kkt_add(int N, double* __restrict__ step, const double* __restrict__ corr) { add_item(N, step, corr); }


thread_local std::string g_kkt_err;

}  // namespace

// ---- what the other units of the handle call too (sparse_kkt_handle.hpp) -----------------------------------------------------------------------------------------
namespace calipso::sparse_kkt {

int fail(KH* s, int rc, const std::string& text) { (s ? s->err_text : g_kkt_err) = text; return rc; }

// every non-NULL pointer of a device entry must be device memory of the handle's device: checked before anything is enqueued
int device_pointer(KH* s, const void* p, const char* entry, const char* arg) {
    if (!p) return CALIPSO_OK;
    hipPointerAttribute_t at;
    std::memset(&at, 0, sizeof(at));
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return fail(s, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": " + arg + " is not device memory (a host pointer?): the device entries take device pointers only");
    }
    if (at.type != hipMemoryTypeDevice) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": " + arg + " is not device memory: the device entries take device pointers only");
    if (at.device != s->device) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": " + arg + " lives on device " + std::to_string(at.device) + ", the handle on device " + std::to_string(s->device));
    return CALIPSO_OK;
}

int values_missing(KH* s, const char* entry) {
    static const char* const names[5] = {"Lxx", "gx", "hx", "w", "penalty"};
    const size_t need[5] = {(size_t)s->d.nnzL, (size_t)s->d.nnzg, (size_t)s->d.nnzh, (size_t)s->d.N, (size_t)(s->d.ne > 0)};
    for (int i = 0; i < 5; ++i) if (need[i] && !s->have[i]) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": no " + names[i] + " resident (calipso_hip_sparse_kkt_set_values first)");
    return CALIPSO_OK;
}

int enter(KH* s, const char* entry, Need need) {
    if (!s) return CALIPSO_ERR_ARGUMENT;
    KK(hipSetDevice(s->device));
    if (need == VALUES) return values_missing(s, entry);
    if (need >= STATE) { const int rc = solve_state(s); if (rc < 0) return rc; }
    return need > STATE ? solve_ready(s, entry, need == STATE_POINT) : CALIPSO_OK;
}

}  // namespace calipso::sparse_kkt

namespace {

int sparse_failed(KH* s, int rc, const char* what) { return fail(s, rc, std::string(what) + ": " + calipso_hip_sparse_last_error(s->sp)); }

int set_values(KH* s, const char* entry, const double* Lxx, const double* gx, const double* hx, const double* w, const double* penalty, bool device) {
    ENTER(HANDLE);
    DEVPTR(Lxx); DEVPTR(gx); DEVPTR(hx); DEVPTR(w); DEVPTR(penalty);
    const hipMemcpyKind kind = device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const double* src[5] = {Lxx, gx, hx, w, penalty};
    double* dst[5] = {s->Lxx, s->gx, s->hx, s->w, s->rho};
    const size_t count[5] = {(size_t)s->d.nnzL, (size_t)s->d.nnzg, (size_t)s->d.nnzh, (size_t)s->d.N, 1};
    for (int i = 0; i < 5; ++i) if (src[i] && count[i]) { KK(hipMemcpyAsync(dst[i], src[i], sizeof(double) * count[i], kind, s->st)); s->have[i] = true; }
    KK(hipStreamSynchronize(s->st));
    s->assembled = false; s->factored = false;      // K and its factor belong to the values before
    if (w) s->slacks_kept = false;                  // the differentiate slacks are the new point's own
    return CALIPSO_OK;
}

void enqueue_assemble(KH* s, const KktDev& d, double ep, double ed) {
    const long long items = (long long)d.nnzL + d.nnzg + d.nnzh + d.nx + d.ne + d.nc + d.ncc;
    hipLaunchKernelGGL(k_kkt_assemble, dim3(blocks(items)), dim3(KT), 0, s->st, d, ep, ed, s->K);
}
}  // namespace

namespace calipso::sparse_kkt {

// one assemble + factorisation at (ep, ed); inertia as compute_inertia! (linear_solver.jl:33-44)
int assemble_factorize(KH* s, const KktDev& d, double ep, double ed, int64_t inertia[3]) {
    KK(hipEventRecord(s->ev[0], s->st));
    enqueue_assemble(s, d, ep, ed);
    KK(hipEventRecord(s->ev[1], s->st));
    s->sc.ep = ep; s->sc.ed = ed; s->assembled = true; s->factored = false;
    const int rc = calipso_hip_sparse_factorize_device(s->sp, s->K, inertia);      // (returns synchronised)
    if (rc < 0) return sparse_failed(s, rc, "factorize");
    s->factored = true;
    float ms = 0.f; KK(hipEventElapsedTime(&ms, s->ev[0], s->ev[1])); s->ms[0] += ms;
    double t[2] = {0.0, 0.0}; (void)calipso_hip_sparse_timing(s->sp, t); s->ms[1] += t[0];
    return rc;
}

int map_columns(KH* s, const KktDev& d, bool transposed, int k, const double* V, double* rsym, double* dsym, double* OUT, const hipEvent_t* around) {
    const dim3 grid(blocks((long long)d.n + d.nsoc), (unsigned)k), block(KT);
    if (around) KK(hipEventRecord(around[0], s->st));
    if (transposed) hipLaunchKernelGGL(k_kkt_map_pre<true>, grid, block, 0, s->st, d, s->sc.ep, s->sc.ed, V, rsym, OUT);
    else hipLaunchKernelGGL(k_kkt_map_pre<false>, grid, block, 0, s->st, d, s->sc.ep, s->sc.ed, V, rsym, OUT);
    const int rc = calipso_hip_sparse_solve_device(s->sp, k, rsym, dsym);
    if (rc < 0) return sparse_failed(s, rc, "solve");
    if (transposed) hipLaunchKernelGGL(k_kkt_map_post<true>, grid, block, 0, s->st, d, s->sc.ep, s->sc.ed, dsym, V, OUT);
    else hipLaunchKernelGGL(k_kkt_map_post<false>, grid, block, 0, s->st, d, s->sc.ep, s->sc.ed, dsym, V, OUT);
    if (around) KK(hipEventRecord(around[1], s->st));
    return CALIPSO_OK;
}

}  // namespace calipso::sparse_kkt

namespace {

// search_direction_symmetric! (search_direction.jl:25-104) with the current factorisation: out (N) from res (N), both on the device — the forward map, one column
int solve_symmetric(KH* s, const double* res, double* out, double* ms) {
    const int rc = map_columns(s, s->d, false, 1, res, s->rsym, s->dsym, out, s->ev);
    if (rc < 0) return rc;
    KK(hipStreamSynchronize(s->st));
    float t = 0.f; KK(hipEventElapsedTime(&t, s->ev[0], s->ev[1])); *ms += t;
    return CALIPSO_OK;
}
void enqueue_mul(KH* s, const double* v, const Sink& sink) {
    if (s->wave_rows) hipLaunchKernelGGL(k_kkt_mul_gathered<true>, dim3(blocks(s->d.n, KT / 64)), dim3(KT), 0, s->st, s->d, s->sc.ep, s->sc.ed, v, sink);
    else hipLaunchKernelGGL(k_kkt_mul_gathered<false>, dim3(blocks(s->d.n)), dim3(KT), 0, s->st, s->d, s->sc.ep, s->sc.ed, v, sink);
    if (s->d.ne + s->d.nc > 0) hipLaunchKernelGGL(k_kkt_mul_local, dim3(blocks((long long)s->d.ne + 2ll * s->d.nc)), dim3(KT), 0, s->st, s->d, s->sc.ep, s->sc.ed, v, sink);
}
// err = res - H step and its infinity norm: one double comes back
int residual_error(KH* s, const double* res, const double* step, double* norm, double* ms) {
    KK(hipEventRecord(s->ev[0], s->st));
    KK(hipMemsetAsync(s->norm, 0, sizeof(double), s->st));
    enqueue_mul(s, step, Sink{nullptr, res, s->err, reinterpret_cast<unsigned long long*>(s->norm)});
    KK(hipEventRecord(s->ev[1], s->st));
    KK(hipMemcpyAsync(norm, s->norm, sizeof(double), hipMemcpyDeviceToHost, s->st));
    KK(hipStreamSynchronize(s->st));
    float t = 0.f; KK(hipEventElapsedTime(&t, s->ev[0], s->ev[1])); *ms += t;
    return CALIPSO_OK;
}

// ---- `H \ residual` (search_direction.jl:22, search_direction_nonsymmetric!) by restarted right-preconditioned GMRES: H the unreduced matrix at the regularisation
// of the last assemble, M = solve_symmetric with the current factorisation, started from zero.  V and Z = M V are kept, so a cycle ends with x += Z y and no further
// solve; one read-back per iteration (the Hessenberg column, |w|, the cycle's |r0|), one per cycle (the true |res - H x|_inf of residual_error).  x is built in
// s->corr and copied into `step` only where everything stayed finite: otherwise `step` is left as it was.  Kernels: sparse_krylov.hip; decisions: sparse_krylov.hpp
namespace kry = calipso::sparse_krylov;

int gmres(KH* s, const double* res, double* step) {
    kry::FallbackReport& fr = s->fallback;
    const kry::Layout lay = kry::layout(s->d.N, s->kry.restart);
    if (!s->kry_ev[0]) { KK(hipEventCreate(&s->kry_ev[0])); KK(hipEventCreate(&s->kry_ev[1])); }
    if (const int rc = device_grown(s, s->kry_ws, (size_t)lay.doubles); rc < 0) return rc;
    double* const ws = s->kry_ws.p;
    double* const V = ws + lay.off_V; double* const Z = ws + lay.off_Z; double* const x = s->corr;
    const size_t N = (size_t)s->d.N, bytes = sizeof(double) * N;
    const double tolerance = s->opt.iterative_refinement_tolerance;
    int iterations = 0, cycles = 0, launches = 0;
    double true_norm = 0.0, unused_ms = 0.0;
    bool converged = false, finite = true;
    fr.v[kry::FI_TAKEN] = 1.0;
    KK(hipEventRecord(s->kry_ev[0], s->st));
    KK(hipMemsetAsync(x, 0, bytes, s->st));
    const double* r0 = res;
    for (;;) {
        krylov_enqueue_update(s->st, lay, ws, 0, r0, V, false, true);                       // v0 = r0 / |r0|_2
        krylov_enqueue_norm_scale(s->st, lay, ws, kry::COEF_BETA, V);
        launches += 3;
        kry::Cycle cycle;
        kry::ColumnVerdict verdict = kry::COLUMN_CONTINUE;
        double coef[kry::COEF_DOUBLES];
        for (int j = 0; verdict == kry::COLUMN_CONTINUE; ++j) {
            double* const w = V + (size_t)(j + 1) * N;
            int rc = solve_symmetric(s, V + (size_t)j * N, Z + (size_t)j * N, &unused_ms);   // z_j = M v_j
            if (rc < 0) return rc;
            enqueue_mul(s, Z + (size_t)j * N, Sink{w, nullptr, nullptr, nullptr});            // w = H z_j (every row of w is written)
            for (int pass = 0; pass < 2; ++pass) {                                           // classical Gram-Schmidt, twice
                krylov_enqueue_dots(s->st, lay, ws, j + 1, w);
                krylov_enqueue_update(s->st, lay, ws, j + 1, w, w, pass == 1, pass == 1);
            }
            krylov_enqueue_norm_scale(s->st, lay, ws, kry::COEF_NORM, w);                     // v_{j+1} = w / |w|_2
            launches += 6;
            KK(hipMemcpyAsync(coef, ws + lay.off_coef, sizeof(coef), hipMemcpyDeviceToHost, s->st));
            KK(hipStreamSynchronize(s->st));
            if (j == 0) {
                const double beta = coef[kry::COEF_BETA];
                if (!std::isfinite(beta)) { verdict = kry::COLUMN_NONFINITE; break; }
                cycle.begin(s->kry.restart, beta);
                if (beta == 0.0) { verdict = kry::COLUMN_BREAKDOWN; break; }                  // x is exact already
            }
            verdict = cycle.push(coef, coef[kry::COEF_NORM], tolerance);
            iterations += 1;
        }
        double y[kry::RESTART_MAX];
        if (verdict == kry::COLUMN_NONFINITE || !cycle.solve(y)) { finite = false; break; }
        if (cycle.j > 0) { krylov_enqueue_combine(s->st, lay, ws, cycle.j, y, x); launches += 1; }
        cycles += 1;
        { const int rc = residual_error(s, res, x, &true_norm, &unused_ms); if (rc < 0) return rc; }      // s->err = res - H x
        const kry::CycleVerdict next = kry::after_cycle(true_norm, tolerance, cycles, s->kry.max_cycles);
        if (next == kry::CYCLE_NONFINITE) { finite = false; break; }
        if (next == kry::CYCLE_CONVERGED) { converged = true; break; }
        if (next == kry::CYCLE_UNCONVERGED) break;
        r0 = s->err;
    }
    if (finite) KK(hipMemcpyAsync(step, x, bytes, hipMemcpyDeviceToDevice, s->st));
    KK(hipEventRecord(s->kry_ev[1], s->st));
    KK(hipStreamSynchronize(s->st));
    KK(hipGetLastError());
    float ms = 0.f; KK(hipEventElapsedTime(&ms, s->kry_ev[0], s->kry_ev[1]));
    fr.step_taken = finite;
    fr.v[kry::FI_ITERATIONS] = iterations; fr.v[kry::FI_CYCLES] = cycles; fr.v[kry::FI_NORM] = true_norm; fr.v[kry::FI_CONVERGED] = converged ? 1.0 : 0.0;
    fr.v[kry::FI_DEVICE_MS] = ms; fr.v[kry::FI_LAUNCHES] = launches; fr.v[kry::FI_WORKSPACE_BYTES] = (double)(sizeof(double) * s->kry_ws.cap);
    return CALIPSO_OK;
}

}  // namespace

// search_direction! (search_direction.jl:1-23) on device vectors
int calipso::sparse_kkt::search_direction(KH* s, const double* res, double* step, double regularization[3], double info[4]) {
    const auto wall0 = std::chrono::steady_clock::now();
    for (double& m : s->ms) m = 0.0;
    const Options& o = s->opt;
    Scalars& sc = s->sc;
    sc.ep_last = regularization[1];
    s->fallback.begin_call();
    const auto leave = [&](int rc, double nfact, double rounds, double norm) {
        regularization[0] = sc.ep; regularization[1] = sc.ep_last; regularization[2] = sc.ed;
        if (info) { info[0] = nfact; info[1] = rounds; info[2] = norm; info[3] = s->fallback.v[kry::FI_ITERATIONS]; }
        s->ms[5] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
        return rc;
    };
    // inertia_correction! (inertia.jl:30-80)
    calipso::ic_begin(o, sc);
    int nfact = 0;
    for (bool first = true;; first = false) {
        int64_t in[3] = {0, 0, 0};
        const double ep = sc.ep, ed = sc.ed;
        const int rc = assemble_factorize(s, s->d, ep, ed, in);
        if (rc < 0) return leave(rc, nfact, 0, 0.0);
        ++nfact;
        const calipso::IcVerdict v = calipso::ic_after(o, sc, in, s->d.nx, (i64)s->d.ne + s->d.nc, first);
        if (v == calipso::IC_DONE) break;
        if (v == calipso::IC_FAILED) { fail(s, CALIPSO_ERR_INERTIA, "inertia correction failure (inertia.jl:72)"); return leave(CALIPSO_ERR_INERTIA, nfact, 0, 0.0); }
    }
    int rc = solve_symmetric(s, res, step, &s->ms[2]);
    if (rc < 0) return leave(rc, nfact, 0, 0.0);
    if (!o.iterative_refinement) return leave(CALIPSO_OK, nfact, 0, 0.0);
    // iterative_refinement! (iterative_refinement.jl:1-52)
    double norm = 0.0;
    if ((rc = residual_error(s, res, step, &norm, &s->ms[4])) < 0) return leave(rc, nfact, 0, 0.0);
    const double norm0 = norm;
    int it = 0, status = CALIPSO_OK;
    for (;;) {
        const calipso::RefineVerdict v = calipso::refine_next(o, norm, norm0, &it);
        if (v == calipso::REFINE_DONE) break;
        if (v == calipso::REFINE_FAILED) {                                                   // the reference goes on to `H \ residual` (search_direction.jl:22)
            status = CALIPSO_WARN_REFINEMENT;
            if (s->kry.fallback) {                                                           // ... here: by GMRES, where the option asks for it
                if ((rc = gmres(s, res, step)) < 0) return leave(rc, nfact, it, norm);
                if (s->fallback.step_taken) norm = s->fallback.v[kry::FI_NORM];
            }
            break;
        }
        if ((rc = solve_symmetric(s, s->err, s->corr, &s->ms[3])) < 0) return leave(rc, nfact, it, norm);
        hipLaunchKernelGGL(k_kkt_add,dim3(blocks(s->d.N)), dim3(KT), 0, s->st, s->d.N, step, s->corr);
        if ((rc = residual_error(s, res, step, &norm, &s->ms[4])) < 0) return leave(rc, nfact, it, norm);
        ++it;
    }
    KK(hipGetLastError());
    return leave(status, nfact, it, norm);
}

extern "C" {

const char* calipso_hip_sparse_kkt_last_error(calipso_hip_sparse_kkt* s) { return s ? s->err_text.c_str() : g_kkt_err.c_str(); }

int32_t calipso_hip_sparse_kkt_destroy(calipso_hip_sparse_kkt* s) {
    if (!s) return CALIPSO_OK;
    (void)hipSetDevice(s->device);
    if (s->st) (void)hipStreamSynchronize(s->st);
    solve_state_release(s);
    diff_state_release(s);
    for (void* p : s->dev) if (p) (void)hipFree(p);
    for (hipEvent_t e : s->ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : s->kry_ev) if (e) (void)hipEventDestroy(e);
    if (s->sp) (void)calipso_hip_sparse_destroy(s->sp);
    delete s;
    return CALIPSO_OK;
}

}  // extern "C"

// the plan of triu(K), its stream, the events and the ONE device copy of the analysis tables: what a single handle and a group (sparse_kkt_group.hip) both start from
int calipso::sparse_kkt::create_tables(KH* s, int32_t method, const int64_t* perm) {
    const Analysis& a = s->an;
    KK(hipSetDevice(s->device));
    const int rc0 = calipso_hip_sparse_create(a.n, a.colptr.data(), a.rowval.data(), method, perm, s->device, &s->sp);
    if (rc0 != CALIPSO_OK) return fail(s, rc0, std::string("calipso_hip_sparse_create: ") + calipso_hip_sparse_last_error(s->sp));
    s->st = calipso::sparse_stream(s->sp);
    KK(hipEventCreate(&s->ev[0])); KK(hipEventCreate(&s->ev[1]));
    KktDev& d = s->d;
    d.nx = (int)a.nx; d.ne = (int)a.ne; d.nc = (int)a.nc; d.n = (int)a.n; d.N = (int)a.N; d.q = (int)a.n_nonnegative; d.nsoc = (int)a.n_soc; d.ncc = (int)a.n_cone_columns;
    d.o_r = d.nx; d.o_s = d.nx + d.ne; d.o_y = d.o_s + d.nc; d.o_z = d.o_y + d.ne; d.o_t = d.o_z + d.nc;
    d.nnzL = (int)a.slot_Lxx.size(); d.nnzg = (int)a.slot_gx.size(); d.nnzh = (int)a.slot_hx.size();
    std::vector<int> slotL = a.slot_Lxx;                    // the diagonal's entries are written with ep, by the diagonal's own items
    for (i64 j = 0; j < a.nx; ++j) if (a.diag_x_src[(size_t)j] >= 0) slotL[(size_t)a.diag_x_src[(size_t)j]] = -1;
    std::vector<int> row_cone((size_t)a.nc, -2);
    for (i64 c = 0; c < a.n_nonnegative; ++c) row_cone[(size_t)c] = -1;
    for (i64 j = 0; j < a.n_soc; ++j) for (int i = 0; i < a.soc_dim[(size_t)j]; ++i) row_cone[(size_t)(a.soc_start[(size_t)j] + i)] = (int)j;
    int rc;
    if ((rc = device_upload(s, slotL, &d.slotL)) || (rc = device_upload(s, a.slot_gx, &d.slotg)) || (rc = device_upload(s, a.slot_hx, &d.sloth)) || (rc = device_upload(s, a.diag_x, &d.diag_x)) ||
        (rc = device_upload(s, a.diag_x_src, &d.diag_x_src)) || (rc = device_upload(s, a.diag_e, &d.diag_e)) || (rc = device_upload(s, a.diag_c, &d.diag_c)) || (rc = device_upload(s, row_cone, &d.row_cone)) ||
        (rc = device_upload(s, a.soc_start, &d.soc_start)) || (rc = device_upload(s, a.soc_dim, &d.soc_dim)) || (rc = device_upload(s, a.col_cone, &d.col_cone)) ||
        (rc = device_upload(s, a.col_index, &d.col_index)) || (rc = device_upload(s, a.col_slot, &d.col_slot)) ||
        (rc = device_upload(s, a.Lxx_rows.ptr, &d.Lr.ptr)) || (rc = device_upload(s, a.Lxx_rows.col, &d.Lr.idx)) || (rc = device_upload(s, a.Lxx_rows.src, &d.Lr.src)) ||
        (rc = device_upload(s, a.gx_rows.ptr, &d.gr.ptr)) || (rc = device_upload(s, a.gx_rows.col, &d.gr.idx)) || (rc = device_upload(s, a.gx_rows.src, &d.gr.src)) ||
        (rc = device_upload(s, a.hx_rows.ptr, &d.hr.ptr)) || (rc = device_upload(s, a.hx_rows.col, &d.hr.idx)) || (rc = device_upload(s, a.hx_rows.src, &d.hr.src)) ||
        (rc = device_upload(s, a.gx_cols.ptr, &d.gc.ptr)) || (rc = device_upload(s, a.gx_cols.row, &d.gc.idx)) || (rc = device_upload(s, a.hx_cols.ptr, &d.hc.ptr)) || (rc = device_upload(s, a.hx_cols.row, &d.hc.idx)) ||
        (rc = device_upload(s, a.Lxx_cols.ptr, &d.Lc.ptr)) || (rc = device_upload(s, a.Lxx_cols.row, &d.Lc.idx)))
        return rc;
    d.gc.src = nullptr; d.hc.src = nullptr; d.Lc.src = nullptr;
    // a wavefront per gathered row where the rows are long (a dense-pattern problem), a thread per row where they are short (stage-structured ones)
    s->wave_rows = ((long long)d.nnzL + 2ll * d.nnzg + 2ll * d.nnzh) / std::max(d.n, 1) >= WAVE_ROW_MIN;
    return CALIPSO_OK;
}

extern "C" {

static int32_t kkt_create_impl(KH* s, int32_t method, const int64_t* perm) {
    int rc = create_tables(s, method, perm);
    if (rc) return rc;
    const Analysis& a = s->an;
    KktDev& d = s->d;
    if ((rc = device_fixed(s, &s->Lxx, (size_t)d.nnzL)) || (rc = device_fixed(s, &s->gx, (size_t)d.nnzg)) || (rc = device_fixed(s, &s->hx, (size_t)d.nnzh)) || (rc = device_fixed(s, &s->w, (size_t)d.N)) ||
        (rc = device_fixed(s, &s->rho, 1)) || (rc = device_fixed(s, &s->K, (size_t)a.nnzK())) || (rc = device_fixed(s, &s->res, (size_t)d.N)) || (rc = device_fixed(s, &s->step, (size_t)d.N)) ||
        (rc = device_fixed(s, &s->corr, (size_t)d.N)) || (rc = device_fixed(s, &s->err, (size_t)d.N)) || (rc = device_fixed(s, &s->rsym, (size_t)d.n)) || (rc = device_fixed(s, &s->dsym, (size_t)d.n)) ||
        (rc = device_fixed(s, &s->norm, 1)) || (rc = device_fixed(s, &s->dslack, 2 * (size_t)d.nc))) return rc;
    d.Lxx = s->Lxx; d.gx = s->gx; d.hx = s->hx; d.w = s->w; d.rho = s->rho;
    return CALIPSO_OK;
}

int32_t calipso_hip_sparse_kkt_create(int64_t nx, int64_t ne, int64_t nc, int64_t n_nonnegative, int64_t n_soc, const int64_t* dims, const int64_t* Lxx_colptr,
                                      const int64_t* Lxx_rowval, const int64_t* gx_colptr, const int64_t* gx_rowval, const int64_t* hx_colptr, const int64_t* hx_rowval,
                                      int32_t method, const int64_t* perm, int32_t device, calipso_hip_sparse_kkt** out) {
    if (!out) return CALIPSO_ERR_ARGUMENT;
    *out = nullptr;
    if (method < 0 || method > 5 || (method == 3 && !perm)) return fail(nullptr, CALIPSO_ERR_ARGUMENT, "calipso_hip_sparse_kkt_create: method is 0 .. 5, and 3 comes with a perm");
    Analysis a = analyse(nx, ne, nc, n_nonnegative, n_soc, dims, Lxx_colptr, Lxx_rowval, gx_colptr, gx_rowval, hx_colptr, hx_rowval);
    if (a.status) return fail(nullptr, a.status, "calipso_hip_sparse_kkt_create: " + a.message);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return fail(nullptr, CALIPSO_ERR_HIP, "no HIP device available (libcalipso_hip has no CPU path)"); }
    if (device < 0 || device >= ndev) return fail(nullptr, CALIPSO_ERR_ARGUMENT, "device ordinal out of range");
    KH* s = new KH();
    s->an = std::move(a); s->device = device;
    const int32_t rc = kkt_create_impl(s, method, perm);
    if (rc != CALIPSO_OK) { g_kkt_err = s->err_text; (void)calipso_hip_sparse_kkt_destroy(s); return rc; }      // no half-built handle leaves here
    *out = s;
    return CALIPSO_OK;
}

int32_t calipso_hip_sparse_kkt_info(calipso_hip_sparse_kkt* s, int64_t info[8]) {
    if (!s || !info) return CALIPSO_ERR_ARGUMENT;
    int64_t sp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    (void)calipso_hip_sparse_info(s->sp, sp);
    info[0] = s->an.n; info[1] = s->an.nnzK(); info[2] = sp[2]; info[3] = sp[3]; info[4] = sp[7]; info[5] = 1; info[6] = s->an.max_dim; info[7] = s->an.N;
    return CALIPSO_OK;
}

int32_t calipso_hip_sparse_kkt_pattern(calipso_hip_sparse_kkt* s, int64_t* colptr, int64_t* rowval) {
    if (!s) return CALIPSO_ERR_ARGUMENT;
    if (colptr) std::copy(s->an.colptr.begin(), s->an.colptr.end(), colptr);
    if (rowval) std::copy(s->an.rowval.begin(), s->an.rowval.end(), rowval);
    return CALIPSO_OK;
}

int32_t calipso_hip_sparse_kkt_set_option(calipso_hip_sparse_kkt* s, const char* name, double value) {
    if (!s || !name) return CALIPSO_ERR_ARGUMENT;
    if (calipso::set_search_direction_option(s->opt, name, value)) return CALIPSO_OK;
    if (std::string(name) == "central_path") { s->sc.kappa = value; return CALIPSO_OK; }      // (the solver's scalar, not an option: IC-2 reads it, inertia.jl:44)
    {                                                                                          // krylov_fallback, krylov_restart, krylov_max_cycles (sparse_krylov.hpp)
        std::string why;
        const int rc = calipso::sparse_krylov::set_option(s->kry, name, value, &why);
        if (rc < 0) return fail(s, CALIPSO_ERR_ARGUMENT, "calipso_hip_sparse_kkt_set_option: " + why);
        if (rc > 0) return CALIPSO_OK;
    }
    { const int rc = solve_set_option(s, name, value); if (rc != 0) return rc < 0 ? rc : CALIPSO_OK; }      // what solve! reads besides (sparse_solve.hip)
    { const int rc = diff_set_option(s, name, value); if (rc != 0) return rc < 0 ? rc : CALIPSO_OK; }       // differentiate_refinement (sparse_differentiate.hip)
    return fail(s, CALIPSO_ERR_ARGUMENT, std::string("calipso_hip_sparse_kkt_set_option: unknown option ") + name);
}

int32_t calipso_hip_sparse_kkt_set_values(calipso_hip_sparse_kkt* s, const double* Lxx, const double* gx, const double* hx, const double* w, const double* penalty) {
    return set_values(s, "calipso_hip_sparse_kkt_set_values", Lxx, gx, hx, w, penalty, false);
}
int32_t calipso_hip_sparse_kkt_set_values_device(calipso_hip_sparse_kkt* s, const double* Lxx, const double* gx, const double* hx, const double* w, const double* penalty) {
    return set_values(s, "calipso_hip_sparse_kkt_set_values_device", Lxx, gx, hx, w, penalty, true);
}

int32_t calipso_hip_sparse_kkt_factorize(calipso_hip_sparse_kkt* s, double ep, double ed, int64_t inertia[3]) {
    static const char* const entry = "calipso_hip_sparse_kkt_factorize";
    ENTER(VALUES);
    int64_t in[3] = {0, 0, 0};
    const int rc = assemble_factorize(s, s->d, ep, ed, in);
    if (inertia) std::copy(in, in + 3, inertia);
    return rc;
}

int32_t calipso_hip_sparse_kkt_get_matrix(calipso_hip_sparse_kkt* s, double* nzval) {
    if (!s || !nzval) return CALIPSO_ERR_ARGUMENT;
    if (!s->assembled) return fail(s, CALIPSO_ERR_ARGUMENT, "calipso_hip_sparse_kkt_get_matrix: factorize first");
    KK(hipSetDevice(s->device));
    KK(hipMemcpyAsync(nzval, s->K, sizeof(double) * (size_t)s->an.nnzK(), hipMemcpyDeviceToHost, s->st));
    KK(hipStreamSynchronize(s->st));
    return CALIPSO_OK;
}

int32_t calipso_hip_sparse_kkt_mul(calipso_hip_sparse_kkt* s, const double* v, double* out) {
    if (!s || !v || !out) return CALIPSO_ERR_ARGUMENT;
    if (!s->assembled) return fail(s, CALIPSO_ERR_ARGUMENT, "calipso_hip_sparse_kkt_mul: factorize first (H is taken at the regularisation of the last assemble)");
    KK(hipSetDevice(s->device));
    const size_t bytes = sizeof(double) * (size_t)s->d.N;
    KK(hipMemcpyAsync(s->corr, v, bytes, hipMemcpyHostToDevice, s->st));
    KK(hipMemsetAsync(s->err, 0, bytes, s->st));
    enqueue_mul(s, s->corr, Sink{s->err, nullptr, nullptr, nullptr});
    KK(hipMemcpyAsync(out, s->err, bytes, hipMemcpyDeviceToHost, s->st));
    KK(hipStreamSynchronize(s->st));
    KK(hipGetLastError());
    return CALIPSO_OK;
}

int32_t calipso_hip_sparse_kkt_solve_symmetric(calipso_hip_sparse_kkt* s, const double* residual, double* step) {
    if (!s || !residual || !step) return CALIPSO_ERR_ARGUMENT;
    if (!s->factored) return fail(s, CALIPSO_ERR_ARGUMENT, "calipso_hip_sparse_kkt_solve_symmetric: factorize first");
    KK(hipSetDevice(s->device));
    const size_t bytes = sizeof(double) * (size_t)s->d.N;
    KK(hipMemcpyAsync(s->res, residual, bytes, hipMemcpyHostToDevice, s->st));
    double ms = 0.0;
    const int rc = solve_symmetric(s, s->res, s->step, &ms);
    if (rc < 0) return rc;
    KK(hipMemcpyAsync(step, s->step, bytes, hipMemcpyDeviceToHost, s->st));
    KK(hipStreamSynchronize(s->st));
    KK(hipGetLastError());
    return CALIPSO_OK;
}

// search_direction_nonsymmetric! for this handle: `H \ residual` by GMRES with the current factorisation, whatever the option krylov_fallback says.  A host call
// goes through the handle's own res and step; a device call works on the caller's vectors
static int32_t solve_nonsymmetric(KH* s, const char* entry, const double* residual, double* step, bool device) {
    if (!s || !residual || !step) return CALIPSO_ERR_ARGUMENT;
    if (!s->factored) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": factorize first");
    KK(hipSetDevice(s->device));
    DEVPTR(residual); DEVPTR(step);
    const size_t bytes = sizeof(double) * (size_t)s->d.N;
    const double* res = device ? residual : s->res;
    double* out = device ? step : s->step;
    if (!device) KK(hipMemcpyAsync(s->res, residual, bytes, hipMemcpyHostToDevice, s->st));
    s->fallback.begin_call();
    KK(hipMemsetAsync(out, 0, bytes, s->st));                                  // (a step that is not finite is not taken: zeros then)
    const int rc = gmres(s, res, out);
    if (rc < 0) return rc;
    if (!device) {
        KK(hipMemcpyAsync(step, s->step, bytes, hipMemcpyDeviceToHost, s->st));
        KK(hipStreamSynchronize(s->st));
        KK(hipGetLastError());
    }
    return s->fallback.v[calipso::sparse_krylov::FI_CONVERGED] != 0.0 ? CALIPSO_OK : CALIPSO_WARN_REFINEMENT;
}
int32_t calipso_hip_sparse_kkt_solve_nonsymmetric(calipso_hip_sparse_kkt* s, const double* residual, double* step) {
    return solve_nonsymmetric(s, "calipso_hip_sparse_kkt_solve_nonsymmetric", residual, step, false);
}
int32_t calipso_hip_sparse_kkt_solve_nonsymmetric_device(calipso_hip_sparse_kkt* s, const double* residual, double* step) {
    return solve_nonsymmetric(s, "calipso_hip_sparse_kkt_solve_nonsymmetric_device", residual, step, true);
}
int32_t calipso_hip_sparse_kkt_fallback_info(calipso_hip_sparse_kkt* s, double out[12]) {
    if (!s || !out) return CALIPSO_ERR_ARGUMENT;
    static_assert(calipso::sparse_krylov::FI_COUNT == 12, "out[12]");
    std::copy(s->fallback.v, s->fallback.v + 12, out);
    return CALIPSO_OK;
}

static int32_t search_direction_entry(KH* s, const char* entry, const double* residual, double* step, double regularization[3], double info[4], bool device) {
    if (!s || !residual || !step || !regularization) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": residual, step and regularization are required");
    ENTER(HANDLE);
    DEVPTR(residual); DEVPTR(step);
    if (const int rc = values_missing(s, entry); rc < 0) return rc;
    if (device) return search_direction(s, residual, step, regularization, info);
    const size_t bytes = sizeof(double) * (size_t)s->d.N;
    KK(hipMemcpyAsync(s->res, residual, bytes, hipMemcpyHostToDevice, s->st));
    const int rc = search_direction(s, s->res, s->step, regularization, info);
    if (rc < 0) return rc;
    KK(hipMemcpyAsync(step, s->step, bytes, hipMemcpyDeviceToHost, s->st));
    KK(hipStreamSynchronize(s->st));
    return rc;
}
int32_t calipso_hip_sparse_kkt_search_direction(calipso_hip_sparse_kkt* s, const double* residual, double* step, double regularization[3], double info[4]) {
    return search_direction_entry(s, "calipso_hip_sparse_kkt_search_direction", residual, step, regularization, info, false);
}
int32_t calipso_hip_sparse_kkt_search_direction_device(calipso_hip_sparse_kkt* s, const double* residual, double* step, double regularization[3], double info[4]) {
    return search_direction_entry(s, "calipso_hip_sparse_kkt_search_direction_device", residual, step, regularization, info, true);
}

int32_t calipso_hip_sparse_kkt_timing(calipso_hip_sparse_kkt* s, double ms[8]) {
    if (!s || !ms) return CALIPSO_ERR_ARGUMENT;
    std::copy(s->ms, s->ms + 8, ms);
    return CALIPSO_OK;
}

}  // extern "C"
