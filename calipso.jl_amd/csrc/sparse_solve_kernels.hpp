// sparse_solve_kernels.hpp — the bodies of the kernels of solve!'s vector half on sparse data (sparse_solve.hip) as __device__ functions of (d, v, scalars): the ONE
// copy of the arithmetic that the single handle's kernels (sparse_solve.hip) and the group's kernels (sparse_solve_group.hip) both call, the group's after shifting
// KktDev and SolveDev by the member's strides.  A member of a group therefore computes, operation for operation, what a single handle computes on the same data —
// as long as it runs on the single handle's grid (Layout::grid): the two-stage reductions add their partials in workgroup order.  Device code only.
#pragma once
#include "sparse_kkt_handle.hpp"           // KktDev, KT
#include "sparse_kkt_kernels.hpp"          // rabs
#include "sparse_solve.hpp"                // the published block, the item space, the workspace layout: plain host C++

namespace calipso {
namespace sparse_kkt {

// what the solve kernels read and write besides KktDev
struct SolveDev {
    long long rows, small0, wide0, items;
    int n_small, n_wide, grid;
    const int *small_cones, *wide_cones;
    const double *q, *b, *hvec;
    double objective_constant;
    double *w, *cand, *dual, *res, *step, *mgrad, *bgrad, *cprod, *ctarget, *g, *h, *gcand, *hcand, *fx;
    double* ws; unsigned* wsm;                    // reduction workspace: doubles and mask words
    long long off_prologue, off_candidate, off_accept;
    double* pub; unsigned* pub_masks;             // the published block
    const double* fobj;                           // the evaluator's objective: [0] at the solution, [1] at the candidate (evaluated mode only)
};

namespace solve_body {

using namespace calipso::sparse_solve;

// ---- the QP's evaluate! (evaluate.jl:37-121) row by row; X(j) gives entry j of the variables ---------------------------------------------------------------------
template <typename FX> __device__ __forceinline__ double qp_hessian_row(const KktDev& d, int k, FX X) {          // (Lxx x)_k
    double a = 0.0;
    for (int p = d.Lr.ptr[k]; p < d.Lr.ptr[k + 1]; ++p) a += d.Lxx[d.Lr.src[p]] * X(d.Lr.idx[p]);
    return a;
}
template <typename FX> __device__ __forceinline__ double qp_equality_row(const KktDev& d, const SolveDev& v, int i, FX X) {      // g_i = (gx x)_i - b_i
    double a = 0.0;
    for (int p = d.gr.ptr[i]; p < d.gr.ptr[i + 1]; ++p) a += d.gx[d.gr.src[p]] * X(d.gr.idx[p]);
    return a - v.b[i];
}
template <typename FX> __device__ __forceinline__ double qp_cone_row(const KktDev& d, const SolveDev& v, int c, FX X) {          // h_c = (hx x)_c + hvec_c
    double a = 0.0;
    for (int p = d.hr.ptr[c]; p < d.hr.ptr[c + 1]; ++p) a += d.hx[d.hr.src[p]] * X(d.hr.idx[p]);
    return a + v.hvec[c];
}
__device__ __forceinline__ void qp_dual_rows(const KktDev& d, int k, const double* __restrict__ y, const double* __restrict__ z, double* gy, double* hz) {      // (gx'y)_k, (hx'z)_k
    double a = 0.0, b = 0.0;
    for (int p = d.gc.ptr[k]; p < d.gc.ptr[k + 1]; ++p) a += d.gx[p] * y[d.gc.idx[p]];
    for (int p = d.hc.ptr[k]; p < d.hc.ptr[k + 1]; ++p) b += d.hx[p] * z[d.hc.idx[p]];
    *gy = a; *hz = b;
}

// ---- items ------------------------------------------------------------------------------------------------------------------------------------------------------
// what item `it` is: 0 a row (*index = the row of [x; equality; cone]), 1 a second-order cone (*index = the cone, its entries q = *lane, *lane + *nl, ...), -1 padding.
// Wave-uniform except inside the row section.
__device__ __forceinline__ int item_kind(const SolveDev& v, long long it, int* index, int* lane, int* nl) {
    if (it < v.rows) { *index = (int)it; return 0; }
    if (it >= v.small0 && it < v.small0 + v.n_small) { *index = v.small_cones[it - v.small0]; *lane = 0; *nl = 1; return 1; }
    if (it >= v.wide0) { *index = v.wide_cones[(it - v.wide0) >> 6]; *lane = (int)((it - v.wide0) & 63); *nl = 64; return 1; }
    return -1;
}
__device__ __forceinline__ double cone_sum(double a, int nl) {       // over the lanes that share a cone (a whole wavefront, or the thread alone)
    if (nl > 1) for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    return a;
}

// the workgroup's partials: quantities [0, FIRST_MAX) are sums, the rest maxima; one double per (quantity, workgroup) at ws[off + q * grid + workgroup]
template <int NQ, int FIRST_MAX>
__device__ __forceinline__ void store_partials(double (&val)[NQ], double* __restrict__ ws, long long off, int grid) {
    __shared__ double part[NQ][KT / 64];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        double a = val[q];
        for (int o = 32; o > 0; o >>= 1) { const double other = __shfl_xor(a, o); a = q < FIRST_MAX ? a + other : fmax(a, other); }
        if ((threadIdx.x & 63) == 0) part[q][threadIdx.x >> 6] = a;
    }
    __syncthreads();
    if (threadIdx.x < NQ) {
        const int q = threadIdx.x;
        double a = part[q][0];
        for (int k = 1; k < KT / 64; ++k) a = q < FIRST_MAX ? a + part[q][k] : fmax(a, part[q][k]);
        ws[off + (long long)q * grid + blockIdx.x] = a;
    }
}
// the finishing kernels' first half: thread q < NQ combines the partials of quantity q in workgroup order into tot[q]
template <int NQ, int FIRST_MAX>
__device__ __forceinline__ void combine_partials(const double* __restrict__ ws, long long off, int grid, double* tot) {
    if (threadIdx.x < NQ) {
        const int q = threadIdx.x;
        double a = ws[off + (long long)q * grid];
        for (int b = 1; b < grid; ++b) { const double p = ws[off + (long long)q * grid + b]; a = q < FIRST_MAX ? a + p : fmax(a, p); }
        tot[q] = a;
    }
    __syncthreads();
}

// ---- initialize! (initialize.jl:9-48): initialize_slacks! r <- g(x), s <- cone interior; initialize_duals! y, z <- 0, t <- cone interior ------------------------------
// EVAL (here and below): false the QP, whose evaluate! is the gathers above; true a user's evaluator, which wrote fx, g, h and the objective before the kernel runs
template <bool EVAL> __device__ __forceinline__ void init(const KktDev& d, const SolveDev& v) {
    for (long long it = (long long)blockIdx.x * KT + threadIdx.x; it < v.rows; it += (long long)v.grid * KT) {
        const int k = (int)it;
        if (k < d.nx) continue;
        if (k < d.nx + d.ne) {
            const int i = k - d.nx;
            if constexpr (EVAL) v.w[d.o_r + i] = v.g[i];
            else v.w[d.o_r + i] = qp_equality_row(d, v, i, [&](int j) { return v.w[j]; });
            v.w[d.o_y + i] = 0.0;
            continue;
        }
        const int c = k - d.nx - d.ne, kind = d.row_cone[c];
        const double e = kind == -1 ? 1.0 : (kind >= 0 ? (c == d.soc_start[kind] ? 1.0 : 0.1) : 0.0);      // nonnegative.jl:2-8, second_order.jl:2-10
        v.w[d.o_s + c] = e; v.w[d.o_t + c] = e; v.w[d.o_z + c] = 0.0;
    }
}
// the s, t a search_direction is about to be assembled at, kept for differentiate! (quirk B-12): s, then t
__device__ __forceinline__ void keep_slacks(const KktDev& d, double* __restrict__ kept) {
    const long long k = (long long)blockIdx.x * KT + threadIdx.x;
    if (k < d.nc) kept[k] = d.w[d.o_s + k];
    else if (k < 2ll * d.nc) kept[k] = d.w[d.o_t + (k - d.nc)];
}
__device__ __forceinline__ void fill(int count, double* __restrict__ out, double value) {
    const long long k = (long long)blockIdx.x * KT + threadIdx.x;
    if (k < count) out[k] = value;
}

// ---- prologue of a step (solve.jl:100-135, 170-172): evaluate! at the solution, cone!(barrier, barrier_gradient, product, target), merit (merit.jl:2-15) and its
// gradient (:17-31), residual! (residual.jl:1-51), constraint_violation! (constraint_violation.jl:1-13), the norms of optimality_error (optimality_error.jl:1-27) -----
template <bool EVAL> __device__ __forceinline__ void prologue(const KktDev& d, const SolveDev& v, double kappa) {
    double val[PP_COUNT];
#pragma unroll
    for (int q = 0; q < PP_COUNT; ++q) val[q] = 0.0;
    const double rho = d.rho[0];
    const double* __restrict__ w = v.w;
    for (long long it = (long long)blockIdx.x * KT + threadIdx.x; it < v.items; it += (long long)v.grid * KT) {
        int k = 0, lane = 0, nl = 1;
        const int kind = item_kind(v, it, &k, &lane, &nl);
        if (kind == 0) {
            if (k < d.nx) {
                double Lx = 0.0, gy, hz;
                if constexpr (!EVAL) Lx = qp_hessian_row(d, k, [&](int j) { return w[j]; });
                qp_dual_rows(d, k, w + d.o_y, w + d.o_z, &gy, &hz);
                double fx;
                if constexpr (EVAL) fx = v.fx[k]; else fx = Lx + v.q[k];
                const double r = (fx + gy) + hz;                                                            // residual.jl:10-14
                if constexpr (!EVAL) v.fx[k] = fx;
                v.mgrad[k] = fx; v.res[k] = r;
                if constexpr (!EVAL) val[PP_OBJECTIVE] += 0.5 * w[k] * Lx + v.q[k] * w[k];
                val[PP_RES_1] += rabs(r); val[PP_RES_N_INF] = fmax(val[PP_RES_N_INF], rabs(r));
            } else if (k < d.nx + d.ne) {
                const int i = k - d.nx;
                double g;
                if constexpr (EVAL) g = v.g[i]; else g = qp_equality_row(d, v, i, [&](int j) { return w[j]; });
                const double r = w[d.o_r + i], y = w[d.o_y + i], lam = v.dual[i];
                const double rr = lam + rho * r - y, ry = g - r;                                            // :17-19, :29-33
                if constexpr (!EVAL) v.g[i] = g;
                v.res[d.o_r + i] = rr; v.res[d.o_y + i] = ry; v.mgrad[d.nx + i] = lam + rho * r;
                val[PP_DUAL_DOT_R] += lam * r; val[PP_R_DOT_R] += r * r; val[PP_THETA] += rabs(g - r); val[PP_Y_1] += rabs(y);
                val[PP_RES_1] += rabs(rr) + rabs(ry);
                val[PP_RES_N_INF] = fmax(val[PP_RES_N_INF], rabs(rr)); val[PP_RES_Y_INF] = fmax(val[PP_RES_Y_INF], rabs(ry));
            } else {
                const int c = k - d.nx - d.ne, ck = d.row_cone[c];
                double h;
                if constexpr (EVAL) h = v.h[c]; else h = qp_cone_row(d, v, c, [&](int j) { return w[j]; });
                const double sl = w[d.o_s + c], z = w[d.o_z + c], t = w[d.o_t + c];
                const double rs = -z - t, rz = h - sl;                                                      // :22-26, :36-40
                if constexpr (!EVAL) v.h[c] = h;
                v.res[d.o_s + c] = rs; v.res[d.o_z + c] = rz;
                val[PP_THETA] += rabs(h - sl); val[PP_Z_1] += rabs(z); val[PP_T_1] += rabs(t);
                val[PP_RES_1] += rabs(rs) + rabs(rz);
                val[PP_RES_N_INF] = fmax(val[PP_RES_N_INF], rabs(rs)); val[PP_RES_Z_INF] = fmax(val[PP_RES_Z_INF], rabs(rz));
                if (ck < 0) {                                                                               // nonnegative.jl:11-26; a row in no cone holds zeros
                    const bool nn = ck == -1;
                    const double prod = nn ? sl * t : 0.0, target = nn ? 1.0 : 0.0, bg = nn ? 1.0 / sl : 0.0;
                    const double rt = prod - kappa * target;                                                // :43-48
                    v.cprod[c] = prod; v.ctarget[c] = target; v.bgrad[c] = bg; v.res[d.o_t + c] = rt; v.mgrad[d.nx + d.ne + c] = -1.0 * kappa * bg;
                    if (nn) val[PP_BARRIER] += log(sl);
                    val[PP_RES_1] += rabs(rt); val[PP_RES_T_INF] = fmax(val[PP_RES_T_INF], rabs(rt));
                }
            }
        } else if (kind == 1) {                                                                             // second_order.jl:13-42
            const int st = d.soc_start[k], dm = d.soc_dim[k];
            const double* sl = w + d.o_s + st; const double* t = w + d.o_t + st;
            double tail = 0.0, dot = 0.0;
            for (int q = lane; q < dm; q += nl) { if (q > 0) tail += sl[q] * sl[q]; dot += sl[q] * t[q]; }
            tail = cone_sum(tail, nl); dot = cone_sum(dot, nl);
            const double det = sl[0] * sl[0] - tail, sc = 1.0 / det;
            if (lane == 0) val[PP_BARRIER] += 0.5 * log(det);
            for (int q = lane; q < dm; q += nl) {
                const double prod = q == 0 ? dot : sl[0] * t[q] + t[0] * sl[q], target = q == 0 ? 1.0 : 0.0, bg = q == 0 ? sc * sl[0] : sc * (-sl[q]);
                const double rt = prod - kappa * target;
                v.cprod[st + q] = prod; v.ctarget[st + q] = target; v.bgrad[st + q] = bg; v.res[d.o_t + st + q] = rt; v.mgrad[d.nx + d.ne + st + q] = -1.0 * kappa * bg;
                val[PP_RES_1] += rabs(rt); val[PP_RES_T_INF] = fmax(val[PP_RES_T_INF], rabs(rt));
            }
        }
    }
    store_partials<PP_COUNT, PP_FIRST_MAX>(val, v.ws, v.off_prologue, v.grid);
}
template <bool EVAL> __device__ __forceinline__ void prologue_finish(const KktDev& d, const SolveDev& v, double kappa) {
    __shared__ double tot[PP_COUNT];
    combine_partials<PP_COUNT, PP_FIRST_MAX>(v.ws, v.off_prologue, v.grid, tot);
    if (threadIdx.x != 0) return;
    double* pub = v.pub;
    double f;
    if constexpr (EVAL) f = v.fobj[0]; else f = tot[PP_OBJECTIVE] + v.objective_constant;
    double M = 0.0;                                                                                         // merit.jl:2-15
    M += f;
    M += tot[PP_DUAL_DOT_R] + 0.5 * d.rho[0] * tot[PP_R_DOT_R];
    M -= kappa * tot[PP_BARRIER];
    pub[PUB_OBJECTIVE] = f; pub[PUB_BARRIER] = tot[PP_BARRIER]; pub[PUB_DUAL_DOT_R] = tot[PP_DUAL_DOT_R]; pub[PUB_R_DOT_R] = tot[PP_R_DOT_R];
    pub[PUB_MERIT] = M; pub[PUB_THETA] = tot[PP_THETA] / (double)(d.ne + d.nc);                             // constraint_violation.jl:12
    pub[PUB_RES_1] = tot[PP_RES_1]; pub[PUB_RES_N_INF] = tot[PP_RES_N_INF]; pub[PUB_RES_Y_INF] = tot[PP_RES_Y_INF]; pub[PUB_RES_Z_INF] = tot[PP_RES_Z_INF];
    pub[PUB_RES_T_INF] = tot[PP_RES_T_INF]; pub[PUB_Y_1] = tot[PP_Y_1]; pub[PUB_Z_1] = tot[PP_Z_1]; pub[PUB_T_1] = tot[PP_T_1];
}

// ---- cone search (solve.jl:190-221): for every trial step size scaling_line_search^k, k < nk, whether s - a Ds (and t - a Dt) violates a cone
// (nonnegative.jl:29-34, second_order.jl:45-47); a is formed as the reference forms it, a <- scaling_line_search * a (cones.hip: violation_masks) ----------------------
__device__ __forceinline__ void mask_set(unsigned* lm, int which, int k) { atomicOr(&lm[which * calipso::CONE_MASK_WORDS + (k >> 5)], 1u << (k & 31)); }

__device__ __forceinline__ void cone_masks(const KktDev& d, const SolveDev& v, double tau, double sls, int nk) {
    __shared__ unsigned lm[PUB_MASK_INTS];
    if (threadIdx.x < PUB_MASK_INTS) lm[threadIdx.x] = 0u;
    __syncthreads();
    const double* __restrict__ w = v.w;
    const double keep = 1.0 - tau;
    for (long long it = (long long)blockIdx.x * KT + threadIdx.x; it < v.items; it += (long long)v.grid * KT) {
        int k = 0, lane = 0, nl = 1;
        const int kind = item_kind(v, it, &k, &lane, &nl);
        if (kind == 0) {
            const int c = k - d.nx - d.ne;
            if (c < 0 || d.row_cone[c] != -1) continue;
            for (int which = 0; which < 2; ++which) {
                const int o = which == 0 ? d.o_s : d.o_t;
                const double x = w[o + c], D = v.step[o + c];
                double a = 1.0;
                for (int tr = 0; tr < nk; ++tr) { if (x - a * D <= keep * x) mask_set(lm, which, tr); a = sls * a; }
            }
        } else if (kind == 1) {
            const int st = d.soc_start[k], dm = d.soc_dim[k];
            for (int which = 0; which < 2; ++which) {
                const int o = (which == 0 ? d.o_s : d.o_t) + st;
                const double* x = w + o; const double* D = v.step + o;
                double a = 1.0;
                for (int tr = 0; tr < nk; ++tr) {
                    double nrm = 0.0;
                    for (int q = (lane == 0 ? nl : lane); q < dm; q += nl) { const double e = (x[q] - a * D[q]) - keep * x[q]; nrm += e * e; }
                    nrm = cone_sum(nrm, nl);
                    if (lane == 0 && (x[0] - a * D[0]) - keep * x[0] <= sqrt(nrm)) mask_set(lm, which, tr);
                    a = sls * a;
                }
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < PUB_MASK_INTS) v.wsm[(long long)threadIdx.x * v.grid + blockIdx.x] = lm[threadIdx.x];
}
// the masks of all workgroups, and the two step sizes the first candidate takes (as cone_step_sizes of step_decisions.hpp forms them; the host decides on the masks)
__device__ __forceinline__ void masks_finish(const SolveDev& v, double sls, int nk) {
    __shared__ unsigned m[PUB_MASK_INTS];
    if (threadIdx.x < PUB_MASK_INTS) {
        unsigned a = 0u;
        for (int b = 0; b < v.grid; ++b) a |= v.wsm[(long long)threadIdx.x * v.grid + b];
        m[threadIdx.x] = a; v.pub_masks[threadIdx.x] = a;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    bool failed = false;
    for (int which = 0; which < 2; ++which) {
        int first = -1;
        for (int k = 0; k < nk && first < 0; ++k) if (!(m[which * calipso::CONE_MASK_WORDS + (k >> 5)] & (1u << (k & 31)))) first = k;
        double a = 1.0;
        for (int k = 0; k < first; ++k) a = sls * a;
        if (first < 0) failed = true;
        v.pub[which == 0 ? PUB_STEP_S : PUB_STEP_T] = a;
    }
    v.pub[PUB_CONE_SEARCH_FAILED] = failed ? 1.0 : 0.0;
}

// ---- candidate (solve.jl:206-229, 268-276) and what is evaluated at it (:231-250, 278-297): x^, r^, s^ with a_s (t^ with a_t, first candidate only), f, g, h, the
// barrier, merit and constraint violation there; first: also dd = merit_gradient . step.primals (line_search.jl:2-18).  alpha: the step sizes on the device (the
// published block, behind the masks' finishing kernel) or NULL for the values given ---------------------------------------------------------------------------------
__device__ __forceinline__ void candidate(const KktDev& d, const SolveDev& v, const double* __restrict__ alpha, double a_s, double a_t, int first) {
    if (alpha) { a_s = alpha[PUB_STEP_S]; a_t = alpha[PUB_STEP_T]; }
    double val[CP_COUNT];
#pragma unroll
    for (int q = 0; q < CP_COUNT; ++q) val[q] = 0.0;
    const double* __restrict__ w = v.w;
    const double* __restrict__ D = v.step;
    const auto X = [&](int j) { return w[j] - a_s * D[j]; };
    for (long long it = (long long)blockIdx.x * KT + threadIdx.x; it < v.items; it += (long long)v.grid * KT) {
        int k = 0, lane = 0, nl = 1;
        const int kind = item_kind(v, it, &k, &lane, &nl);
        if (kind == 0) {
            if (first) val[CP_DD] += v.mgrad[k] * D[k];                                                     // (the primals are the first n entries of the step: point.jl:20)
            if (k < d.nx) {
                const double xh = X(k), Lx = qp_hessian_row(d, k, X);
                v.cand[k] = xh;
                val[CP_OBJECTIVE] += 0.5 * xh * Lx + v.q[k] * xh;
            } else if (k < d.nx + d.ne) {
                const int i = k - d.nx;
                const double rh = w[d.o_r + i] - a_s * D[d.o_r + i], g = qp_equality_row(d, v, i, X), lam = v.dual[i];
                v.cand[d.o_r + i] = rh; v.gcand[i] = g;
                val[CP_DUAL_DOT_R] += lam * rh; val[CP_R_DOT_R] += rh * rh; val[CP_THETA] += rabs(g - rh);
            } else {
                const int c = k - d.nx - d.ne;
                const double sh = w[d.o_s + c] - a_s * D[d.o_s + c], h = qp_cone_row(d, v, c, X);
                v.cand[d.o_s + c] = sh; v.hcand[c] = h;
                if (first) v.cand[d.o_t + c] = w[d.o_t + c] - a_t * D[d.o_t + c];
                val[CP_THETA] += rabs(h - sh);
                if (d.row_cone[c] == -1) val[CP_BARRIER] += log(sh);
            }
        } else if (kind == 1) {
            const int st = d.soc_start[k], dm = d.soc_dim[k];
            const double* sl = w + d.o_s + st; const double* Ds = D + d.o_s + st;
            double tail = 0.0;
            for (int q = (lane == 0 ? nl : lane); q < dm; q += nl) { const double e = sl[q] - a_s * Ds[q]; tail += e * e; }
            tail = cone_sum(tail, nl);
            const double s0 = sl[0] - a_s * Ds[0];
            if (lane == 0) val[CP_BARRIER] += 0.5 * log(s0 * s0 - tail);
        }
    }
    store_partials<CP_COUNT, CP_COUNT>(val, v.ws, v.off_candidate, v.grid);
}
// ---- the candidate in evaluated mode: the point must exist before it can be evaluated, so the kernel above splits.  candidate_point forms x^, r^, s^ (t^ when
// first) and the partials of dd; the evaluator then runs at v.cand into the candidate's objective, gcand and hcand; candidate_merit reduces dual . r^, r^ . r^, the
// constraint violation and the barrier from what both left, reading the candidate where candidate() recomputes it (the same bits) -------------------------------------
__device__ __forceinline__ void candidate_point(const KktDev& d, const SolveDev& v, const double* __restrict__ alpha, double a_s, double a_t, int first) {
    if (alpha) { a_s = alpha[PUB_STEP_S]; a_t = alpha[PUB_STEP_T]; }
    double val[1] = {0.0};
    const double* __restrict__ w = v.w;
    const double* __restrict__ D = v.step;
    for (long long it = (long long)blockIdx.x * KT + threadIdx.x; it < v.rows; it += (long long)v.grid * KT) {
        const int k = (int)it;
        if (first) val[0] += v.mgrad[k] * D[k];
        if (k < d.nx + d.ne) v.cand[k] = w[k] - a_s * D[k];                                                 // x^, r^ (o_r = nx)
        else {
            const int c = k - d.nx - d.ne;
            v.cand[d.o_s + c] = w[d.o_s + c] - a_s * D[d.o_s + c];
            if (first) v.cand[d.o_t + c] = w[d.o_t + c] - a_t * D[d.o_t + c];
        }
    }
    if (first) store_partials<1, 1>(val, v.ws, v.off_candidate + (long long)CP_DD * v.grid, v.grid);        // (uniform: every workgroup stores, or none)
}
__device__ __forceinline__ void candidate_merit(const KktDev& d, const SolveDev& v) {
    static_assert(CP_DD == CP_COUNT - 1, "the partials of dd are the point kernel's: they lie behind the ones stored here");
    double val[CP_DD];
#pragma unroll
    for (int q = 0; q < CP_DD; ++q) val[q] = 0.0;
    const double* __restrict__ ch = v.cand;
    for (long long it = (long long)blockIdx.x * KT + threadIdx.x; it < v.items; it += (long long)v.grid * KT) {
        int k = 0, lane = 0, nl = 1;
        const int kind = item_kind(v, it, &k, &lane, &nl);
        if (kind == 0) {
            if (k < d.nx) continue;
            if (k < d.nx + d.ne) {
                const int i = k - d.nx;
                const double rh = ch[d.o_r + i], g = v.gcand[i], lam = v.dual[i];
                val[CP_DUAL_DOT_R] += lam * rh; val[CP_R_DOT_R] += rh * rh; val[CP_THETA] += rabs(g - rh);
            } else {
                const int c = k - d.nx - d.ne;
                const double sh = ch[d.o_s + c], h = v.hcand[c];
                val[CP_THETA] += rabs(h - sh);
                if (d.row_cone[c] == -1) val[CP_BARRIER] += log(sh);
            }
        } else if (kind == 1) {
            const int st = d.soc_start[k], dm = d.soc_dim[k];
            const double* sh = ch + d.o_s + st;
            double tail = 0.0;
            for (int q = (lane == 0 ? nl : lane); q < dm; q += nl) tail += sh[q] * sh[q];
            tail = cone_sum(tail, nl);
            if (lane == 0) val[CP_BARRIER] += 0.5 * log(sh[0] * sh[0] - tail);
        }
    }
    store_partials<CP_DD, CP_DD>(val, v.ws, v.off_candidate, v.grid);
}
template <bool EVAL> __device__ __forceinline__ void candidate_finish(const KktDev& d, const SolveDev& v, double kappa, int first) {
    __shared__ double tot[CP_COUNT];
    combine_partials<CP_COUNT, CP_COUNT>(v.ws, v.off_candidate, v.grid, tot);
    if (threadIdx.x != 0) return;
    double f;
    if constexpr (EVAL) f = v.fobj[1]; else f = tot[CP_OBJECTIVE] + v.objective_constant;
    double M = 0.0;
    M += f;
    M += tot[CP_DUAL_DOT_R] + 0.5 * d.rho[0] * tot[CP_R_DOT_R];
    M -= kappa * tot[CP_BARRIER];
    v.pub[PUB_CAND_OBJECTIVE] = f; v.pub[PUB_CAND_BARRIER] = tot[CP_BARRIER]; v.pub[PUB_CAND_MERIT] = M; v.pub[PUB_CAND_THETA] = tot[CP_THETA] / (double)(d.ne + d.nc);
    if (first) v.pub[PUB_DD] = tot[CP_DD];
}

// ---- accept (solve.jl:309-333): x, r, s, t <- candidate, y <- y - a Dy, z <- z - a Dz, the constraints evaluated at the candidate become the solution's,
// cone!(product), |g|_inf and |s o t|_inf.  start: nothing moves — g is evaluated at the solution and the cone product is taken as it LIES in its buffer
// (solve.jl:85-86 read it before :88 forms it: stale on first use, kept) ---------------------------------------------------------------------------------------------
template <bool EVAL> __device__ __forceinline__ void accept(const KktDev& d, const SolveDev& v, double a, int start) {
    double val[AP_COUNT] = {0.0, 0.0};
    for (long long it = (long long)blockIdx.x * KT + threadIdx.x; it < v.items; it += (long long)v.grid * KT) {
        int k = 0, lane = 0, nl = 1;
        const int kind = item_kind(v, it, &k, &lane, &nl);
        if (kind == 0) {
            if (k < d.nx) { if (!start) v.w[k] = v.cand[k]; }
            else if (k < d.nx + d.ne) {
                const int i = k - d.nx;
                double g;
                if (start) { if constexpr (EVAL) g = v.g[i]; else g = qp_equality_row(d, v, i, [&](int j) { return v.w[j]; }); }
                else { g = v.gcand[i]; v.w[d.o_r + i] = v.cand[d.o_r + i]; v.w[d.o_y + i] = v.w[d.o_y + i] - a * v.step[d.o_y + i]; }
                v.g[i] = g;
                val[AP_G_INF] = fmax(val[AP_G_INF], rabs(g));
            } else {
                const int c = k - d.nx - d.ne;
                if (start) { val[AP_PRODUCT_INF] = fmax(val[AP_PRODUCT_INF], rabs(v.cprod[c])); continue; }
                const double sh = v.cand[d.o_s + c], th = v.cand[d.o_t + c];
                v.w[d.o_s + c] = sh; v.w[d.o_t + c] = th; v.w[d.o_z + c] = v.w[d.o_z + c] - a * v.step[d.o_z + c];
                v.h[c] = v.hcand[c];
                if (d.row_cone[c] < 0) {
                    const double prod = d.row_cone[c] == -1 ? sh * th : 0.0;
                    v.cprod[c] = prod;
                    val[AP_PRODUCT_INF] = fmax(val[AP_PRODUCT_INF], rabs(prod));
                }
            }
        } else if (kind == 1 && !start) {                                                                   // (the cone reads the candidate, which nobody writes here)
            const int st = d.soc_start[k], dm = d.soc_dim[k];
            const double* sh = v.cand + d.o_s + st; const double* th = v.cand + d.o_t + st;
            double dot = 0.0;
            for (int q = lane; q < dm; q += nl) dot += sh[q] * th[q];
            dot = cone_sum(dot, nl);
            for (int q = lane; q < dm; q += nl) {
                const double prod = q == 0 ? dot : sh[0] * th[q] + th[0] * sh[q];
                v.cprod[st + q] = prod;
                val[AP_PRODUCT_INF] = fmax(val[AP_PRODUCT_INF], rabs(prod));
            }
        }
    }
    store_partials<AP_COUNT, 0>(val, v.ws, v.off_accept, v.grid);
}
__device__ __forceinline__ void accept_finish(const SolveDev& v) {
    __shared__ double tot[AP_COUNT];
    combine_partials<AP_COUNT, 0>(v.ws, v.off_accept, v.grid, tot);
    if (threadIdx.x == 0) { v.pub[PUB_G_INF] = tot[AP_G_INF]; v.pub[PUB_PRODUCT_INF] = tot[AP_PRODUCT_INF]; }
}

// ---- outer update (solve.jl:362-364): lambda <- lambda + rho r, with the penalty BEFORE its own update (:365) -----------------------------------------------------------
__device__ __forceinline__ void outer_update(const KktDev& d, const SolveDev& v, double rho) {
    const long long i = (long long)blockIdx.x * KT + threadIdx.x;
    if (i < d.ne) v.dual[i] = v.dual[i] + rho * v.w[d.o_r + i];
}

}  // namespace solve_body
}  // namespace sparse_kkt
}  // namespace calipso
