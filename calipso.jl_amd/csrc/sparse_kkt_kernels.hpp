// sparse_kkt_kernels.hpp — the bodies of the kernels of search_direction! on sparse data as __device__ functions of (d, ep, ed, pointers): the ONE copy of the
// arithmetic that the single handle's kernels (sparse_kkt.hip) and the group's kernels (sparse_kkt_group.hip) both call, the group's after shifting the pointers
// by the member's strides.  A member of a group therefore computes, operation for operation, what a single handle computes on the same data.  Device code only.
#pragma once
#include "sparse_kkt_handle.hpp"           // KktDev, KT
#include "sparse_differentiate.hpp"        // the row arithmetic of the condensed maps and arrow_inverse, the closed-form arrow inverse: device and host

namespace calipso {
namespace sparse_kkt {

constexpr int WAVE_ROW_MIN = 32;           // mean non-zeros per gathered row from which a wavefront takes a row instead of a thread

__device__ __forceinline__ double rabs(double x) { return x != x ? __builtin_huge_val() : fabs(x); }      // a NaN reports +inf (step_decisions.hpp: refine_next)

// ---- assemble: K.nzval from the three non-zero vectors, the point, rho, ep, ed ------------------------------------------------------------------------------
__device__ __forceinline__ void assemble_item(const KktDev& d, double ep, double ed, double* __restrict__ K) {
    using namespace calipso::sparse_differentiate;
    long long e = (long long)blockIdx.x * KT + threadIdx.x;
    if (e < d.nnzL) { const int s = d.slotL[e]; if (s >= 0) K[s] = d.Lxx[e]; return; }                      // Hessian, strict upper triangle
    e -= d.nnzL;
    if (e < d.nnzg) { K[d.slotg[e]] = d.gx[e]; return; }                                                    // Jacobians
    e -= d.nnzg;
    if (e < d.nnzh) { K[d.sloth[e]] = d.hx[e]; return; }
    e -= d.nnzh;
    if (e < d.nx) { const int p = d.diag_x_src[e]; K[d.diag_x[e]] = (p >= 0 ? d.Lxx[p] : 0.0) + ep; return; }   // Hessian diagonal + ep   :82-85
    e -= d.nx;
    if (e < d.ne) { K[d.diag_e[e]] = -1.0 / (d.rho[0] + ep) + (0.0 - ed); return; }                         // :127-131
    e -= d.ne;
    if (e < d.nc) {
        const int kind = d.row_cone[e];
        if (kind == -1) {                                                                                   // nonnegative: -Sb / (T + Sb P) + D   :139-143
            const double Sb = d.w[d.o_s + e] - ed, T = d.w[d.o_t + e];
            K[d.diag_c[e]] = -1.0 * Sb / (T + Sb * ep) + (0.0 - ed);
        } else if (kind == -2) K[d.diag_c[e]] = 0.0;                                                        // a cone row in no cone: the structural diagonal only
        return;
    }
    e -= d.nc;
    if (e >= d.ncc) return;
    // second-order blocks (:145-164): column i of -(Cs + Cbar_t P)^-1 Cbar_t + D, rows <= i
    const int c = d.col_cone[e], i = d.col_index[e], st = d.soc_start[c], dm = d.soc_dim[c];
    const double* sl = d.w + d.o_s + st; const double* t = d.w + d.o_t + st;
    double* Kc = K + d.col_slot[e];
    const double S0 = sl[0] - ed;
    arrow_inverse(dm,
                  [&](int k) { return t[k] + (k == 0 ? S0 : sl[k]) * ep; },
                  [&](int a) { return i == 0 ? (a == 0 ? S0 : sl[a]) : (a == 0 ? sl[i] : (a == i ? S0 : 0.0)); },      // column i of Cbar_t = arrow(s) - ed I
                  [&](int a, double v) { if (a <= i) Kc[a] = -v + (a == i ? (0.0 - ed) : 0.0); });
}

// ---- H v ----------------------------------------------------------------------------------------------------------------------------------------------------
// what a row's result becomes: out[row] = value (calipso_hip_sparse_kkt_mul), or err[row] = res[row] - value with its magnitude folded into *norm
struct Sink { double* out; const double* res; double* err; unsigned long long* norm; };

__device__ __forceinline__ void sink_store(const Sink& k, int row, bool live, double value) {
    double mag = 0.0;
    if (live) {
        if (k.out) k.out[row] = value;
        if (k.err) { const double e = k.res[row] - value; k.err[row] = e; mag = rabs(e); }
    }
    if (!k.norm) return;                                                       // (uniform)
    __shared__ double part[KT / 64];
    for (int o = 32; o > 0; o >>= 1) mag = fmax(mag, __shfl_xor(mag, o));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mag;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = part[0];
        for (int k2 = 1; k2 < KT / 64; ++k2) m = fmax(m, part[k2]);
        if (m > 0.0) atomicMax(k.norm, (unsigned long long)__double_as_longlong(m));      // non-negative doubles order as their bit patterns
    }
}

// row k of [x; y; z] (the rows that gather from Lxx, gx, hx): the terms of lane `l` of `nl` lanes
__device__ __forceinline__ double gathered_terms(const KktDev& d, const double* __restrict__ v, int k, int l, int nl) {
    double a = 0.0;
    if (k < d.nx) {                                                            // Lxx v_x + gx' v_y + hx' v_z
        for (int p = d.Lr.ptr[k] + l; p < d.Lr.ptr[k + 1]; p += nl) a += d.Lxx[d.Lr.src[p]] * v[d.Lr.idx[p]];
        for (int p = d.gc.ptr[k] + l; p < d.gc.ptr[k + 1]; p += nl) a += d.gx[p] * v[d.o_y + d.gc.idx[p]];
        for (int p = d.hc.ptr[k] + l; p < d.hc.ptr[k + 1]; p += nl) a += d.hx[p] * v[d.o_z + d.hc.idx[p]];
    } else if (k < d.nx + d.ne) {
        const int e = k - d.nx;
        for (int p = d.gr.ptr[e] + l; p < d.gr.ptr[e + 1]; p += nl) a += d.gx[d.gr.src[p]] * v[d.gr.idx[p]];
    } else {
        const int c = k - d.nx - d.ne;
        for (int p = d.hr.ptr[c] + l; p < d.hr.ptr[c + 1]; p += nl) a += d.hx[d.hr.src[p]] * v[d.hr.idx[p]];
    }
    return a;
}
// ... and what the row adds to them: ep on the diagonal, the -1 couplings, -ed
__device__ __forceinline__ double gathered_tail(const KktDev& d, const double* __restrict__ v, int k, double ep, double ed) {
    if (k < d.nx) return ep * v[k];
    if (k < d.nx + d.ne) { const int e = k - d.nx; return -v[d.o_r + e] + (0.0 - ed) * v[d.o_y + e]; }
    const int c = k - d.nx - d.ne;
    return -v[d.o_s + c] + (0.0 - ed) * v[d.o_z + c];
}
__device__ __forceinline__ int gathered_row(const KktDev& d, int k) { return k < d.nx ? k : (k < d.nx + d.ne ? d.o_y + (k - d.nx) : d.o_z + (k - d.nx - d.ne)); }

template <bool WAVE>
__device__ __forceinline__ void mul_gathered_item(const KktDev& d, double ep, double ed, const double* __restrict__ v, const Sink& sink) {
    if (WAVE) {                                                                // one wavefront per row: KT / 64 rows per workgroup
        const int k = blockIdx.x * (KT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
        const bool live = k < d.n;
        double a = live ? gathered_terms(d, v, k, lane, 64) : 0.0;
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        const bool writer = live && lane == 0;
        sink_store(sink, writer ? gathered_row(d, k) : 0, writer, writer ? a + gathered_tail(d, v, k, ep, ed) : 0.0);
    } else {
        const long long k = (long long)blockIdx.x * KT + threadIdx.x;
        const bool live = k < d.n;
        sink_store(sink, live ? gathered_row(d, (int)k) : 0, live, live ? gathered_terms(d, v, (int)k, 0, 1) + gathered_tail(d, v, (int)k, ep, ed) : 0.0);
    }
}

// the r-, s- and t-rows: rho, the -1 couplings, the cone product Jacobians arrow(t), arrow(s) - ed I (residual_jacobian_variables.jl:59-105)
__device__ __forceinline__ void mul_local_item(const KktDev& d, double ep, double ed, const double* __restrict__ v, const Sink& sink) {
    const long long k = (long long)blockIdx.x * KT + threadIdx.x;
    const bool live = k < d.ne + 2ll * d.nc;
    int row = 0; double a = 0.0;
    if (live) {
        if (k < d.ne) { row = d.o_r + (int)k; a = (d.rho[0] + ep) * v[row] - v[d.o_y + k]; }
        else if (k < d.ne + d.nc) { const int c = (int)k - d.ne; row = d.o_s + c; a = ep * v[row] - v[d.o_z + c] - v[d.o_t + c]; }
        else {
            const int c = (int)k - d.ne - d.nc, kind = d.row_cone[c];
            row = d.o_t + c;
            if (kind == -1) a = d.w[d.o_t + c] * v[d.o_s + c] + (d.w[d.o_s + c] - ed) * v[d.o_t + c];
            else if (kind >= 0) {
                const int st = d.soc_start[kind], dm = d.soc_dim[kind], i = c - st;
                const double* sl = d.w + d.o_s + st; const double* t = d.w + d.o_t + st;
                const double* vs = v + d.o_s + st; const double* vt = v + d.o_t + st;
                if (i == 0) for (int b = 0; b < dm; ++b) a += t[b] * vs[b] + (b == 0 ? sl[0] - ed : sl[b]) * vt[b];
                else a = (t[i] * vs[0] + sl[i] * vt[0]) + (t[0] * vs[i] + (sl[0] - ed) * vt[i]);
            }
        }
    }
    sink_store(sink, row, live, a);
}

// ---- the condensed solve's outer halves for ONE column: g (n) from v (N) before the LDL^T solve, out (N) from its solution h (n) and v after it -------------------
// items: [0, nx) variables, [nx, nx + ne) equality rows, [.., n) cone rows, [n, n + nsoc) second-order cones
template <bool TRANSPOSED>
__device__ __forceinline__ void map_pre_item(const KktDev& d, double ep, double ed, const double* __restrict__ v, double* __restrict__ g, double* __restrict__ out) {
    using namespace calipso::sparse_differentiate;
    long long k = (long long)blockIdx.x * KT + threadIdx.x;
    if (k < d.nx) { g[k] = v[k]; return; }
    k -= d.nx;
    const MapScalars c{ep, ed, d.ne ? d.rho[0] : 0.0};
    if (k < d.ne) { g[d.nx + k] = TRANSPOSED ? equality_transposed_pre(c, v[d.o_r + k], v[d.o_y + k]) : equality_forward_pre(c, v[d.o_r + k], v[d.o_y + k]); return; }
    k -= d.ne;
    const int oc = d.nx + d.ne;
    if (k < d.nc) {
        const int kind = d.row_cone[k];
        if (kind == -1) {
            const double sl = d.w[d.o_s + k], t = d.w[d.o_t + k];
            g[oc + k] = TRANSPOSED ? nonnegative_transposed_pre(c, sl, t, v[d.o_s + k], v[d.o_z + k], v[d.o_t + k]) : nonnegative_forward_pre(c, sl, t, v[d.o_s + k], v[d.o_z + k], v[d.o_t + k]);
        } else if (kind == -2) g[oc + k] = v[d.o_z + k];
        return;
    }
    k -= d.nc;
    if (k >= d.nsoc) return;
    const int st = d.soc_start[k], dm = d.soc_dim[k];
    const double* sl = d.w + d.o_s + st; const double* t = d.w + d.o_t + st;
    if (TRANSPOSED)         // the temporaries in the cone's entries of the output column, which the post launch writes
        soc_transposed_pre(c, dm, sl, t, v + d.o_s + st, v + d.o_z + st, v + d.o_t + st, g + oc + st, out + d.o_t + st, out + d.o_s + st);
    else soc_forward_pre(c, dm, sl, t, v + d.o_s + st, v + d.o_z + st, v + d.o_t + st, g + oc + st);
}

template <bool TRANSPOSED>
__device__ __forceinline__ void map_post_item(const KktDev& d, double ep, double ed, const double* __restrict__ h, const double* __restrict__ v, double* __restrict__ out) {
    using namespace calipso::sparse_differentiate;
    long long k = (long long)blockIdx.x * KT + threadIdx.x;
    if (k < d.nx) { out[k] = h[k]; return; }
    k -= d.nx;
    const MapScalars c{ep, ed, d.ne ? d.rho[0] : 0.0};
    if (k < d.ne) {
        const double he = h[d.nx + k];
        out[d.o_y + k] = he;
        out[d.o_r + k] = TRANSPOSED ? equality_transposed_post(c, he, v[d.o_r + k]) : equality_forward_post(c, he, v[d.o_r + k]);
        return;
    }
    k -= d.ne;
    const int oc = d.nx + d.ne;
    if (k < d.nc) {
        const int kind = d.row_cone[k];
        const double hc = h[oc + k];
        out[d.o_z + k] = hc;
        if (kind == -1) {
            const double sl = d.w[d.o_s + k], t = d.w[d.o_t + k];
            if (TRANSPOSED) nonnegative_transposed_post(c, sl, t, hc, v[d.o_s + k], v[d.o_t + k], &out[d.o_s + k], &out[d.o_t + k]);
            else nonnegative_forward_post(c, sl, t, hc, v[d.o_s + k], v[d.o_t + k], &out[d.o_s + k], &out[d.o_t + k]);
        } else if (kind == -2) { out[d.o_s + k] = 0.0; out[d.o_t + k] = 0.0; }
        return;
    }
    k -= d.nc;
    if (k >= d.nsoc) return;
    const int st = d.soc_start[k], dm = d.soc_dim[k];
    const double* sl = d.w + d.o_s + st; const double* t = d.w + d.o_t + st;
    if (TRANSPOSED) soc_transposed_post(c, dm, sl, t, h + oc + st, v + d.o_s + st, v + d.o_t + st, out + d.o_s + st, out + d.o_t + st);
    else soc_forward_post(c, dm, sl, t, h + oc + st, v + d.o_s + st, v + d.o_t + st, out + d.o_s + st, out + d.o_t + st);
}

__device__ __forceinline__ void add_item(int N, double* __restrict__ step, const double* __restrict__ corr) {
    const long long k = (long long)blockIdx.x * KT + threadIdx.x;
    if (k < N) step[k] += corr[k];
}

// workgroups for `items` items: computed in 64 bits, at least one
inline unsigned blocks(long long items, int per_block = KT) { return (unsigned)std::max<long long>((items + per_block - 1) / per_block, 1); }

}  // namespace sparse_kkt
}  // namespace calipso
