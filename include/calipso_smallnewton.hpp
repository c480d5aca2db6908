// calipso_smallnewton.hpp — the batched small-problem solve! kernels (csrc/smallnewton.hip, include/calipso_hip.h "solve! for a batch of SMALL conic
// problems") as HIP C++ for gfx950: the common types (Dm, Lay, Args, Options), the device code once per workgroup size, the built-in QP evaluator and the
// entry a user library exports to run the kernels with an evaluator of its own.  libcalipso_hip.so builds the kernels with QpEval; a user's translation unit
// includes this header, defines an evaluator type and writes
//
//     CALIPSO_SMALLNEWTON_EVALUATOR(MyEvaluator, my_problem_kernels)
//
// which emits  extern "C" int32_t my_problem_kernels(const calipso_smallnewton_launch*)  and instantiates every build of the kernels (64 / 128 / 256 threads
// per instance x second-order cones x lu_fallback, differentiate! and its reverse mode) for MyEvaluator in the user's own code object: the evaluator is inlined into the Newton
// loop, no device function pointer crosses the two libraries.  calipso_hip_smallnewton_set_evaluator(handle, my_problem_kernels, n_parameters) registers it.
//
// An evaluator (the hooks are workgroup-cooperative: EVERY thread of the instance calls each one, with the inputs written and synchronised; the kernel puts a
// barrier after each hook that writes; `c` is the instance's context, c.tid the thread, C::threads the workgroup size, c.d the dimensions (nx, ne, nc, m = ne + nc,
// N, ldz), c.theta the instance's parameter row (global, n_parameters doubles), c.red / c.ycol scratch (64 and SN_JB nx doubles of LDS), c.sum(v) a workgroup sum
// of a double[K] into every thread):
//
//   struct MyEvaluator {
//       static constexpr bool constant_derivatives = false;            // (true only for QpEval)
//       static constexpr bool provides_jacobian_parameters = true;     // jacobian_parameters below exists
//       // f(x; theta), the same value in every thread
//       template <class C> __device__ static double objective(C& c, const double* x);
//       // [g; h](x; theta) -> out (m = ne + nc entries, LDS)
//       template <class C> __device__ static void constraints(C& c, const double* x, double* out);
//       // at the point w = [x; r; s; y; z; t] (point.jl:13-22, LDS): fx -> c.fx (nx), [gx; hx] -> c.Z (m x nx, column-major, leading dimension c.d.ldz, LDS) and the
//       // Lagrangian Hessian fxx + (y'g)xx + (z'h)xx -> c.Hw (nx x nx, column-major, every entry, global memory)
//       template <class C> __device__ static void derivatives(C& c, const double* w);
//       // dR/dtheta at w (residual_jacobian_parameters.jl:1-40): rows 0 .. nx-1 fxθ + (y'g)xθ + (z'h)xθ, rows oy() .. oy()+ne-1 gθ, rows oz() .. oz()+nc-1 hθ of the
//       // N x n_parameters column-major matrix J (global; every other entry is zero on entry)
//       template <class C> __device__ static void jacobian_parameters(C& c, const double* w, double* J);
//   };
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "calipso_hip.h"
#include "calipso_options.hpp"
#include "calipso_wave.hpp"

#ifndef SN_JB
#define SN_JB 8          // columns per panel of the LDL^T (bench/small_newton_phases.sh builds other values; part of the handshake of an evaluator's entry)
#endif

namespace calipso {
namespace sn {

enum { SC_KAPPA = 0, SC_TAU, SC_RHO, SC_EP, SC_EPLAST, SC_ED, SC_EQV, SC_CPV, SC_F, SC_COUNT = 16 };
enum { CN_TOTAL = 0, CN_OUTER, CN_INNER, CN_FACT, CN_RFAIL, CN_RMAX, CN_RLAST, CN_STEPS, CN_FILTER, CN_TRACE, CN_COUNT = 16 };
enum { IN_STEP = 0, IN_STEP_T, IN_ROUNDS, IN_NFACT, IN_MH, IN_THETAH, IN_EXIT, IN_OPT, IN_COUNT = 8 };
enum { MODE_SOLVE = 0, MODE_STEPS = 1, MODE_DIFF = 2, MODE_ADJ = 3 };

struct Dm {
    int nx, ne, nc, m, n, N, ldz, q, nsoc, wsz, maxd;      // q nonnegative entries first, then nsoc second-order cones (contiguous ranges); wsz = sum of dim^2; ldz: leading dimension of Z in LDS (odd: conflict-free column walks)
    __host__ __device__ int orr() const { return nx; }
    __host__ __device__ int os() const { return nx + ne; }
    __host__ __device__ int oy() const { return nx + ne + nc; }
    __host__ __device__ int oz() const { return nx + ne + nc + ne; }
    __host__ __device__ int ot() const { return nx + ne + nc + ne + nc; }
};

// LDS carve-up (offsets in doubles): the same function sizes the launch on the host and places the pointers on the device
struct Lay { int Z, S, q, bh, lam, sol, cand, step, res, rerr, corr, rsym, fx, gzx, gh, ghc, cprod, bgrad, wz, wsoc, bsoc, vsoc, D, Dinv, xb, t1, t2, ycol, red, total; };
__host__ __device__ inline Lay layout(const Dm& d) {
    Lay L; int o = 0;
    auto take = [&](int n) { const int at = o; o += (n + 1) & ~1; return at; };
    L.Z = take(d.ldz * d.nx); L.S = take(d.nx * (d.nx + 1) / 2);
    L.q = take(d.nx); L.bh = take(d.m); L.lam = take(d.ne);
    L.sol = take(d.N); L.cand = take(d.N); L.step = take(d.N); L.res = take(d.N); L.rerr = take(d.N); L.corr = take(d.N);
    L.rsym = take(d.n);
    L.fx = take(d.nx); L.gzx = take(d.nx); L.gh = take(d.m); L.ghc = take(d.m);
    L.cprod = take(d.nc); L.bgrad = take(d.nc); L.wz = take(d.nc); L.wsoc = take(d.wsz); L.bsoc = take(d.wsz); L.vsoc = take(4 * d.maxd * d.nsoc);
    L.D = take(d.nx); L.Dinv = take(d.nx); L.xb = take(d.nx); L.t1 = take(d.m); L.t2 = take(d.m);
    L.ycol = take(SN_JB * d.nx);
    L.red = take(64);
    L.total = o;
    return L;
}

struct Args {
    Dm d; Options o;
    const double *P, *q, *Z, *bh; long long sP, sq, sZ, sbh;      // element strides per instance (0: one problem shared by all)
    double *w, *lam, *sc, *filt, *info, *trace, *prof; long long* cnt; int* status;
    const int *soc_start, *soc_dim, *soc_woff;      // per second-order cone: first cone-local index, dimension, offset of its dim x dim blocks
    int batch, mode, count, advance, trace_rows;
    double* stf;                                    // batch x 2 nc: s and t at the last search direction (calipso_smallnewton_device.hpp: quirk B-12)
    double* rtheta; double* sens; long long srtheta;                   // differentiate!: dR/dtheta and the sensitivities, per instance N x count, column-major
    double* Hs;                                     // lu_fallback: per instance N x N (the unreduced H, then its LU factors)
    // evaluators other than the QP
    const double* theta; long long stheta;          // parameters, per instance (stride 0: one row for all)
    double* hess;                                   // the Lagrangian Hessian, batch x nx x nx
    double* dpt;                                    // batch x (nx + m): x and [y; z] where the last search direction evaluated the derivatives (differentiate! reads them there)
    int eval_rtheta;                                // differentiate!: 1 = dR/dtheta from the evaluator into rtheta (count = n_parameters), 0 = the caller's
};

// the argument block of differentiate! in reverse mode (k_smallnewton_adj only: Args itself, which every build shares with entries compiled before it, keeps its
// size).  Per instance, column-major: cotangents N x k in; lambda = M' v (N x k), -R_theta' lambda (n_parameters x k, base.count = n_parameters) and the QP data's
// gradients ((nx^2 + nx + ne nx + ne + nc nx + nc) x k) out, each skipped when NULL
struct AdjArgs {
    Args base;
    const double* cot; double* adjoint; double* grad_theta; double* grad_qp;
    double objective_scale;                         // c of the QP's f = c x'Px + q'x
    int k, reserved;
};

// the built-in evaluator: the QP of qp.hip (f = 1/2 x'Lxx x + q'x with Lxx = 2cP, [g; h] = [A; -G] x + [-b; h]).  Its derivatives are constant: Z = [A; -G]
// and q, [-b; h] are loaded into LDS once, the Hessian block Lg stays the problem data in L2, and no hook runs in the Newton step except the gradients.  At a
// line-search candidate f's two sums join the merit's reduction (candidate_begin / candidate_terms / candidate_objective).
struct QpEval {
    static constexpr bool constant_derivatives = true;
    static constexpr bool provides_jacobian_parameters = false;
    template <class C> __device__ __forceinline__ static void bind(C& c, const Args& a, int inst) {
        const Dm& d = c.d; const int tid = c.tid;
        c.Lg = a.P + (size_t)inst * a.sP;
        const double* q = a.q + (size_t)inst * a.sq;
        const double* Zg = a.Z + (size_t)inst * a.sZ; const double* bh = a.bh + (size_t)inst * a.sbh;
        for (int e = tid; e < d.m * d.nx; e += C::threads) c.Z[(e % d.m) + (e / d.m) * d.ldz] = Zg[e];
        for (int i = tid; i < d.nx; i += C::threads) c.q[i] = q[i];
        for (int i = tid; i < d.m; i += C::threads) c.bh[i] = bh[i];
    }
    template <class C> __device__ __forceinline__ static double objective(C& c, const double* p) {          // f = 1/2 x'Lxx x + q'x   (ycol as scratch)
        C::hess_partial(c.Lg, c.d.nx, p, c.ycol);
        __syncthreads();
        double v[2] = {0.0, 0.0};
        for (int i = c.tid; i < c.d.nx; i += C::threads) { v[0] += p[i] * C::hess_sum(c.ycol, c.d.nx, i); v[1] += c.q[i] * p[i]; }
        c.sum(v);
        return 0.5 * v[0] + v[1];
    }
    template <class C> __device__ __forceinline__ static void constraints(C& c, const double* p, double* out) {      // [g; h] = [A; -G] x + [-b; hvec]
        C::matvec(c.Z, c.d.ldz, c.d.m, c.d.nx, p, out, c.bh);
    }
    template <class C> __device__ __forceinline__ static void gradients(C& c, const double* p) {                    // fx = Lxx x + q ; gzx = A'y + (-G)'z
        const Dm& d = c.d;
        C::hess_partial(c.Lg, d.nx, p, c.ycol);
        C::matvec_t(c.Z, d.ldz, d.m, d.nx, p + d.oy(), c.gzx, nullptr);
        __syncthreads();
        for (int i = c.tid; i < d.nx; i += C::threads) c.fx[i] = C::hess_sum(c.ycol, d.nx, i) + c.q[i];
        __syncthreads();
    }
    template <class C> __device__ __forceinline__ static void candidate_begin(C& c, const double* p, double* gh) {
        C::hess_partial(c.Lg, c.d.nx, p, c.ycol);
        C::matvec(c.Z, c.d.ldz, c.d.m, c.d.nx, p, gh, c.bh);
    }
    template <class C> __device__ __forceinline__ static void candidate_terms(C& c, const double* p, int i, double& a, double& b) { a += p[i] * C::hess_sum(c.ycol, c.d.nx, i); b += c.q[i] * p[i]; }
    __device__ __forceinline__ static double candidate_objective(double a, double b) { return 0.5 * a + b; }
};

// the device code, once per workgroup size (the host picks: csrc/smallnewton.hip sn_threads)
#define SN_THREADS 64
namespace t64 {
#include "calipso_smallnewton_device.hpp"
}
#undef SN_THREADS
#define SN_THREADS 128
namespace t128 {
#include "calipso_smallnewton_device.hpp"
}
#undef SN_THREADS
#define SN_THREADS 256
namespace t256 {
#include "calipso_smallnewton_device.hpp"
}
#undef SN_THREADS

// the build of k_smallnewton for an evaluator, a workgroup size, a cone layout (second-order cones or not) and lu_fallback; of k_smallnewton_diff
template <class Ev> inline const void* kernel_of(int nt, bool soc, bool lu) {
    if (lu) {
        if (nt == 64) return soc ? (const void*)t64::k_smallnewton<Ev, true, true> : (const void*)t64::k_smallnewton<Ev, false, true>;
        if (nt == 128) return soc ? (const void*)t128::k_smallnewton<Ev, true, true> : (const void*)t128::k_smallnewton<Ev, false, true>;
        return soc ? (const void*)t256::k_smallnewton<Ev, true, true> : (const void*)t256::k_smallnewton<Ev, false, true>;
    }
    if (nt == 64) return soc ? (const void*)t64::k_smallnewton<Ev, true, false> : (const void*)t64::k_smallnewton<Ev, false, false>;
    if (nt == 128) return soc ? (const void*)t128::k_smallnewton<Ev, true, false> : (const void*)t128::k_smallnewton<Ev, false, false>;
    return soc ? (const void*)t256::k_smallnewton<Ev, true, false> : (const void*)t256::k_smallnewton<Ev, false, false>;
}
template <class Ev> inline const void* adj_kernel_of(int nt, bool soc) {
    if (nt == 64) return soc ? (const void*)t64::k_smallnewton_adj<Ev, true> : (const void*)t64::k_smallnewton_adj<Ev, false>;
    if (nt == 128) return soc ? (const void*)t128::k_smallnewton_adj<Ev, true> : (const void*)t128::k_smallnewton_adj<Ev, false>;
    return soc ? (const void*)t256::k_smallnewton_adj<Ev, true> : (const void*)t256::k_smallnewton_adj<Ev, false>;
}
template <class Ev> inline const void* diff_kernel_of(int nt, bool soc) {
    if (nt == 64) return soc ? (const void*)t64::k_smallnewton_diff<Ev, true> : (const void*)t64::k_smallnewton_diff<Ev, false>;
    if (nt == 128) return soc ? (const void*)t128::k_smallnewton_diff<Ev, true> : (const void*)t128::k_smallnewton_diff<Ev, false>;
    return soc ? (const void*)t256::k_smallnewton_diff<Ev, true> : (const void*)t256::k_smallnewton_diff<Ev, false>;
}

// what the entry of CALIPSO_SMALLNEWTON_EVALUATOR does for each request of libcalipso_hip.so (include/calipso_hip.h: calipso_smallnewton_launch)
template <class Ev> inline int32_t entry(const calipso_smallnewton_launch* L) {
    if (!L || !L->out) return CALIPSO_ERR_ARGUMENT;
    if (L->op == CALIPSO_SMALLNEWTON_QUERY) {
        L->out[0] = CALIPSO_SMALLNEWTON_ABI; L->out[1] = (int64_t)sizeof(Args); L->out[2] = SN_JB; L->out[3] = Ev::provides_jacobian_parameters ? 1 : 0;
        L->out[4] = 1;                                  // (the caller's buffer has five entries, pre-zeroed: an entry built before the reverse mode leaves a 0 here)
        return CALIPSO_OK;
    }
    if (L->abi != CALIPSO_SMALLNEWTON_ABI || L->args_bytes != (int64_t)sizeof(Args)) return CALIPSO_ERR_ARGUMENT;
    const bool diff = L->mode == MODE_DIFF, adj = L->mode == MODE_ADJ;      // (MODE_ADJ: L->args is an AdjArgs)
    if (L->op == CALIPSO_SMALLNEWTON_GRANT_LDS) {       // every build may take the LDS the handle asks for
        for (const bool soc : {false, true}) for (const int nt : {64, 128, 256}) {
            for (const bool lu : {false, true}) if (hipFuncSetAttribute(kernel_of<Ev>(nt, soc, lu), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L->lds_bytes) != hipSuccess) (void)hipGetLastError();
            if (hipFuncSetAttribute(diff_kernel_of<Ev>(nt, soc), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L->lds_bytes) != hipSuccess) (void)hipGetLastError();
            if (hipFuncSetAttribute(adj_kernel_of<Ev>(nt, soc), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L->lds_bytes) != hipSuccess) (void)hipGetLastError();
        }
        return CALIPSO_OK;
    }
    if (L->threads != 64 && L->threads != 128 && L->threads != 256) return CALIPSO_ERR_ARGUMENT;
    if ((diff || adj) && L->eval_rtheta && !Ev::provides_jacobian_parameters) return CALIPSO_ERR_ARGUMENT;
    const void* k = adj ? adj_kernel_of<Ev>(L->threads, L->soc != 0) : diff ? diff_kernel_of<Ev>(L->threads, L->soc != 0) : kernel_of<Ev>(L->threads, L->soc != 0, L->lu != 0);
    if (L->op == CALIPSO_SMALLNEWTON_OCCUPANCY) {
        int per = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, k, L->threads, (size_t)L->lds_bytes) != hipSuccess) return CALIPSO_ERR_HIP;
        L->out[0] = per;
        return CALIPSO_OK;
    }
    if (L->op != CALIPSO_SMALLNEWTON_LAUNCH || !L->args) return CALIPSO_ERR_ARGUMENT;
    void* args[] = {const_cast<void*>(L->args)};
    if (hipLaunchKernel(k, dim3((unsigned)L->grid), dim3((unsigned)L->threads), args, (size_t)L->lds_bytes, (hipStream_t)L->stream) != hipSuccess) return CALIPSO_ERR_HIP;
    return hipGetLastError() == hipSuccess ? CALIPSO_OK : CALIPSO_ERR_HIP;
}

}  // namespace sn
}  // namespace calipso

#define CALIPSO_SMALLNEWTON_EVALUATOR(Ev, symbol) \
    extern "C" __attribute__((visibility("default"))) int32_t symbol(const calipso_smallnewton_launch* L) { return calipso::sn::entry<Ev>(L); }
