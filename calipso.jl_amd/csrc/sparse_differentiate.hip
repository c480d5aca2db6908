// sparse_differentiate.hip — differentiate! (src/solver/differentiate.jl:1-61) in both directions on the sparse handle of sparse_kkt.hip: the entries behind
// calipso_hip_sparse_kkt_solve_columns / _differentiate / _differentiate_adjoint (include/calipso_hip.h).  Nothing here is dense: besides the N x k columns themselves
// the memory is that of the handle, and the data gradients live on the stored patterns.
//
//   the map, k columns at once     step = M residual of search_direction_symmetric! (search_direction.jl:25-104) and its transpose: map_columns of sparse_kkt.hip,
//                                  which a Newton step's solve_symmetric goes through with one column.  No loop over columns anywhere.
//   H X, H' X, k columns           the unreduced matrix applied from the same data, one thread per (row, column), fused with E = R - H X and the per-column infinity
//                                  norms (k doubles, read back once per round).  Transposed: Lxx through its column view, the s and t couplings of the local rows swapped.
//   correction rounds              iterative_refinement.jl:14-44 on all columns with the decisions of sensitivity_columns.hpp and the masked accumulate / restore of
//                                  vectors.hip (the ones columns.hip launches).
//   data gradients                 one launch, one thread per (stored non-zero or vector entry, column), the entry index fastest.
//   parameter Jacobians            with set_parameter_patterns the evaluator writes Lx,theta, g,theta, h,theta as values on three stored CSC patterns (np columns).  Forward:
//                                  a clear of V and one launch scatter the selected columns of dR/dtheta into it, one writer per address.  Reverse: grad_theta = -R_theta' lambda
//                                  is a gather over the three columns in stored order — a thread per (short parameter, column), a wavefront with a fixed-order cross-lane
//                                  sum per (long parameter, column); the split length is sparse_parameters.hpp's SPLIT_LENGTH.
// Gathers only: no floating-point atomics (the norm: atomicMax on the bit patterns of non-negative doubles, which is order-independent); a call repeats bit for bit.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "sparse_kkt_handle.hpp"
#include "sparse_differentiate.hpp"
#include "sparse_parameters.hpp"           // the stored patterns of dR/dtheta: the column selection's check, the short / long split, the launch geometry
#include "../../include/calipso_wave.hpp"  // wave_sum_l63

using calipso::i64;
using namespace calipso::sparse_kkt;
using namespace calipso::sparse_differentiate;
static_assert(KT == calipso::sparse_parameters::THREADS && KT % calipso::sparse_parameters::WAVE == 0,
              "sparse_parameters.hpp counts workgroups of KT threads, and a wavefront of the gradient kernel lies within one of them");

struct calipso::sparse_kkt::DiffState {
    Grown<double> ws;                             // the workspace of a k-column pass (sparse_differentiate.hpp: Layout)
    Grown<int> masks;
    double* wd = nullptr;                         // N: the resident point with the kept slacks in its s and t rows (what the kernels read the cone blocks from)
    Grown<double> gbuf;                           // the gradients of a host call before they are copied out
    Grown<int> sel;                               // the selected parameters of a differentiate_parameters call, 0-based
    std::vector<int> sel_host;
    calipso::SensitivityColumns cols;
    std::vector<double> norms;
    double info_forward[4] = {0, 0, 0, 0}, info_reverse[4] = {0, 0, 0, 0}, times[3] = {0, 0, 0};
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};      // a reverse call: entry, last kernel, around the gradient kernel, after the copies
    hipEvent_t ev_pass[4] = {nullptr, nullptr, nullptr, nullptr};          // around the first pre + solve + post of a call, around its correction rounds
    bool rounds_ran = false;
};

namespace {

typedef calipso::sparse_kkt::DiffState DS;

__device__ __forceinline__ double rabs(double x) { return x != x ? __builtin_huge_val() : fabs(x); }      // a NaN reports +inf, as in sparse_kkt.hip

// ---- H X (TRANSPOSED: H' X) for k columns, one thread per (row of the point's layout, column): E = R - H X and the columns' infinity norms, or (R NULL) E = H X -----
// row i of arrow(a) v over the cone's dm entries
__device__ __forceinline__ double arrow_row(const double* __restrict__ a, double a0, const double* __restrict__ v, int dm, int i) {
    if (i == 0) { double r = 0.0; for (int b = 0; b < dm; ++b) r += (b == 0 ? a0 : a[b]) * v[b]; return r; }
    return a[i] * v[0] + a0 * v[i];
}
// (C v)_c for the cone block C = arrow(a) - shift I of cone row c (a: the s or the t rows of the point)
__device__ __forceinline__ double cone_block_row(const KktDev& d, const double* __restrict__ a, double shift, const double* __restrict__ v, int c) {
    const int kind = d.row_cone[c];
    if (kind == -1) return (a[c] - shift) * v[c];
    if (kind < 0) return 0.0;
    const int st = d.soc_start[kind];
    return arrow_row(a + st, a[st] - shift, v + st, d.soc_dim[kind], c - st);
}

template <bool TRANSPOSED>
__global__ __launch_bounds__(KT) void k_diff_mul(const KktDev d, double ep, double ed, const double* __restrict__ X, const double* __restrict__ R, double* __restrict__ E,
                                                 unsigned long long* __restrict__ norms) {
    const long long j = (long long)blockIdx.x * KT + threadIdx.x;
    const size_t col = blockIdx.y;
    const double* v = X + col * (size_t)d.N;
    double mag = 0.0;
    if (j < d.N) {
        double a = 0.0;
        const int i = (int)j;
        if (i < d.o_r) {                                                        // Lxx v_x (Lxx' v_x) + gx' v_y + hx' v_z + ep v_x
            if (TRANSPOSED) for (int p = d.Lc.ptr[i]; p < d.Lc.ptr[i + 1]; ++p) a += d.Lxx[p] * v[d.Lc.idx[p]];
            else for (int p = d.Lr.ptr[i]; p < d.Lr.ptr[i + 1]; ++p) a += d.Lxx[d.Lr.src[p]] * v[d.Lr.idx[p]];
            for (int p = d.gc.ptr[i]; p < d.gc.ptr[i + 1]; ++p) a += d.gx[p] * v[d.o_y + d.gc.idx[p]];
            for (int p = d.hc.ptr[i]; p < d.hc.ptr[i + 1]; ++p) a += d.hx[p] * v[d.o_z + d.hc.idx[p]];
            a += ep * v[i];
        } else if (i < d.o_s) { const int e = i - d.o_r; a = (d.rho[0] + ep) * v[i] - v[d.o_y + e]; }
        else if (i < d.o_y) {                                                   // the s rows: ep v_s - v_z - v_t; transposed: the column of H, arrow(t) v_t in place of -v_t
            const int c = i - d.o_s;
            a = ep * v[i] - v[d.o_z + c];
            a = TRANSPOSED ? a + cone_block_row(d, d.w + d.o_t, 0.0, v + d.o_t, c) : a - v[d.o_t + c];
        } else if (i < d.o_z) {
            const int e = i - d.o_y;
            for (int p = d.gr.ptr[e]; p < d.gr.ptr[e + 1]; ++p) a += d.gx[d.gr.src[p]] * v[d.gr.idx[p]];
            a += -v[d.o_r + e] + (0.0 - ed) * v[i];
        } else if (i < d.o_t) {
            const int c = i - d.o_z;
            for (int p = d.hr.ptr[c]; p < d.hr.ptr[c + 1]; ++p) a += d.hx[d.hr.src[p]] * v[d.hr.idx[p]];
            a += -v[d.o_s + c] + (0.0 - ed) * v[i];
        } else {                                                                // the t rows: arrow(t) v_s + (arrow(s) - ed I) v_t; transposed: -v_s in place of arrow(t) v_s
            const int c = i - d.o_t;
            a = cone_block_row(d, d.w + d.o_s, ed, v + d.o_t, c);
            a = TRANSPOSED ? a - v[d.o_s + c] : a + cone_block_row(d, d.w + d.o_t, 0.0, v + d.o_s, c);
        }
        const size_t at = col * (size_t)d.N + (size_t)i;
        if (R) { const double e = R[at] - a; E[at] = e; mag = rabs(e); }
        else E[at] = a;
    }
    if (!norms) return;                                                         // (uniform)
    __shared__ double part[KT / 64];
    for (int o = 32; o > 0; o >>= 1) mag = fmax(mag, __shfl_xor(mag, o));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mag;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = part[0];
        for (int q = 1; q < KT / 64; ++q) m = fmax(m, part[q]);
        if (m > 0.0) atomicMax(&norms[col], (unsigned long long)__double_as_longlong(m));      // non-negative doubles order as their bit patterns
    }
}

// ---- the data gradients on the stored patterns: one thread per (entry, column), the entry fastest --------------------------------------------------------------
struct GradOut { double* p[6]; };                                               // Lxx, q, gx, b, hx, hvec; NULL: not asked for
// the column of non-zero p of a CSC pattern: the last c with ptr[c] <= p
__device__ __forceinline__ int column_of(const int* __restrict__ ptr, int ncols, int p) {
    int lo = 0, hi = ncols;                                                     // ptr[lo] <= p < ptr[hi]
    while (hi - lo > 1) { const int mid = lo + ((hi - lo) >> 1); if (ptr[mid] <= p) lo = mid; else hi = mid; }
    return lo;
}
__global__ __launch_bounds__(KT) void k_diff_gradients(const KktDev d, const double* __restrict__ w, const double* __restrict__ LAM, const GradOut out) {
    long long e = (long long)blockIdx.x * KT + threadIdx.x;
    const size_t col = blockIdx.y;
    const double* lam = LAM + col * (size_t)d.N;
    const double *x = w, *y = w + d.o_y, *z = w + d.o_z, *lx = lam, *ly = lam + d.o_y, *lz = lam + d.o_z;
    if (e < d.nnzL) { if (out.p[0]) { const int p = (int)e; out.p[0][col * (size_t)d.nnzL + p] = -lx[d.Lc.idx[p]] * x[column_of(d.Lc.ptr, d.nx, p)]; } return; }
    e -= d.nnzL;
    if (e < d.nx) { if (out.p[1]) out.p[1][col * (size_t)d.nx + e] = -lx[e]; return; }
    e -= d.nx;
    if (e < d.nnzg) {
        if (out.p[2]) { const int p = (int)e, r = d.gc.idx[p], c = column_of(d.gc.ptr, d.nx, p); out.p[2][col * (size_t)d.nnzg + p] = -(ly[r] * x[c] + y[r] * lx[c]); }
        return;
    }
    e -= d.nnzg;
    if (e < d.ne) { if (out.p[3]) out.p[3][col * (size_t)d.ne + e] = ly[e]; return; }
    e -= d.ne;
    if (e < d.nnzh) {
        if (out.p[4]) { const int p = (int)e, r = d.hc.idx[p], c = column_of(d.hc.ptr, d.nx, p); out.p[4][col * (size_t)d.nnzh + p] = -(lz[r] * x[c] + z[r] * lx[c]); }
        return;
    }
    e -= d.nnzh;
    if (e < d.nc && out.p[5]) out.p[5][col * (size_t)d.nc + e] = -lz[e];
}

// ---- dR/dtheta on its stored patterns ------------------------------------------------------------------------------------------------------------------------------
// the selected columns into V (N x k, cleared before): thread e of column `col` writes entry e of parameter sel[col] (NULL: col itself) — the entries of Lx,theta into the
// x rows, then those of g,theta into the y rows, then those of h,theta into the z rows.  Rows are duplicate-free within a column: one writer per address
__global__ __launch_bounds__(KT) void k_diff_parameter_columns(const KktDev d, const ParamDev p, const int* __restrict__ sel, double* __restrict__ V) {
    long long e = (long long)blockIdx.x * KT + threadIdx.x;
    const size_t col = blockIdx.y;
    const int j = sel ? sel[col] : (int)col;
    double* v = V + col * (size_t)d.N;
    const int off[3] = {0, d.o_y, d.o_z};
    for (int m = 0; m < 3; ++m) {
        const int lo = p.ptr[m][j], len = p.ptr[m][j + 1] - lo;
        if (e < len) { v[off[m] + p.idx[m][lo + e]] = p.val[m][lo + e]; return; }
        e -= len;
    }
}
// grad_theta(j, col) = -(sum Lx,theta(i, j) lam_x[i] + sum g,theta(e, j) lam_y[e] + sum h,theta(m, j) lam_z[m]), the three columns in stored order.  Items
// [0, np): one thread per parameter, whole sum in stored order (a long parameter's thread returns); [long0, ..): one wavefront per long parameter, lane l the entries
// l, l + 64, ... of each array in turn, then the fixed tree of wave_sum_l63.  No atomics: one writer per (parameter, column)
__global__ __launch_bounds__(KT) void k_diff_parameter_gradient(const KktDev d, const ParamDev p, const double* __restrict__ LAM, double* __restrict__ out) {
    const long long item = (long long)blockIdx.x * KT + threadIdx.x;
    const size_t col = blockIdx.y;
    const double* lam = LAM + col * (size_t)d.N;
    const int off[3] = {0, d.o_y, d.o_z};
    if (item < p.long0) {
        if (item >= p.np) return;
        const int j = (int)item;
        int len = 0;
        for (int m = 0; m < 3; ++m) len += p.ptr[m][j + 1] - p.ptr[m][j];
        if (len >= calipso::sparse_parameters::SPLIT_LENGTH) return;
        double acc = 0.0;
        for (int m = 0; m < 3; ++m)
            for (int q = p.ptr[m][j]; q < p.ptr[m][j + 1]; ++q) acc += p.val[m][q] * lam[off[m] + p.idx[m][q]];
        out[col * (size_t)p.np + j] = -acc;
        return;
    }
    const long long w = (item - p.long0) >> 6;                                  // (wavefront-uniform: long0 and KT are multiples of 64)
    if (w >= p.n_long) return;
    const int lane = threadIdx.x & 63, j = p.long_columns[w];
    double acc = 0.0;
    for (int m = 0; m < 3; ++m)
        for (int q = p.ptr[m][j] + lane; q < p.ptr[m][j + 1]; q += 64) acc += p.val[m][q] * lam[off[m] + p.idx[m][q]];
    acc = calipso::wave_sum_l63(acc);
    if (lane == 63) out[col * (size_t)p.np + j] = -acc;
}

__global__ __launch_bounds__(KT) void k_diff_scale(size_t count, const double* __restrict__ x, double* __restrict__ y, double a) {
    const size_t i = (size_t)blockIdx.x * KT + threadIdx.x;
    if (i < count) y[i] = a * x[i];
}
// the resident point's s, t rows of `wd` from the kept slacks (s, then t)
__global__ __launch_bounds__(KT) void k_diff_place_slacks(const KktDev d, const double* __restrict__ kept, double* __restrict__ wd) {
    const long long k = (long long)blockIdx.x * KT + threadIdx.x;
    if (k < d.nc) wd[d.o_s + k] = kept[k];
    else if (k < 2ll * d.nc) wd[d.o_t + (k - d.nc)] = kept[k];
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------------------------------

unsigned blocks_of(long long items) { return (unsigned)std::max<long long>((items + KT - 1) / KT, 1); }

int ensure_state(KH* s) {
    if (s->diff) return CALIPSO_OK;
    DS* t = new DS();
    s->diff = t;                                             // (released with the handle, whatever happens below)
    for (hipEvent_t& e : t->ev) KK(hipEventCreate(&e));
    for (hipEvent_t& e : t->ev_pass) KK(hipEventCreate(&e));
    return device_fixed(s, &t->wd, (size_t)s->d.N);
}
int reserve_pass(KH* s, const Layout& L, size_t k) {
    DS* t = s->diff;
    int rc = device_grown(s, t->ws, std::max<size_t>(L.doubles, 1));
    if (rc >= 0 && L.ints) rc = device_grown(s, t->masks, L.ints);
    t->rounds_ran = false;                                   // (a new pass: pass_times reads the rounds' events only where they ran)
    if (t->norms.size() < k) t->norms.assign(k, 0.0);
    return rc;
}

// what the kernels read: the handle's data with the point whose s, t rows are the differentiate slacks
KktDev slacks_view(KH* s) {
    KktDev d = s->d;
    if (s->slacks_kept && d.nc) {
        hipLaunchKernelGGL(k_diff_place_slacks, dim3(blocks_of(2ll * d.nc)), dim3(KT), 0, s->st, s->d, s->dslack, s->diff->wd);
        d.w = s->diff->wd;
    }
    return d;
}

// after the entry's last synchronise: the pass and its rounds into the handle's timing, slots 6 and 7 (calipso_hip_sparse_kkt_timing)
int pass_times(KH* s) {
    DS* t = s->diff;
    float ms = 0.f;
    KK(hipEventElapsedTime(&ms, t->ev_pass[0], t->ev_pass[1])); s->ms[6] = ms;
    s->ms[7] = 0.0;
    if (t->rounds_ran) { KK(hipEventElapsedTime(&ms, t->ev_pass[2], t->ev_pass[3])); s->ms[7] = ms; }
    return CALIPSO_OK;
}
void enqueue_mul(KH* s, const KktDev& d, bool transposed, int k, const double* X, const double* R, double* E, double* norms) {
    const dim3 grid(blocks_of(d.N), (unsigned)k), block(KT);
    unsigned long long* nm = reinterpret_cast<unsigned long long*>(norms);
    if (transposed) hipLaunchKernelGGL(k_diff_mul<true>, grid, block, 0, s->st, d, s->sc.ep, s->sc.ed, X, R, E, nm);
    else hipLaunchKernelGGL(k_diff_mul<false>, grid, block, 0, s->st, d, s->sc.ep, s->sc.ed, X, R, E, nm);
}

// iterative_refinement.jl:14-44 over the k columns of X at once (columns.hip: refine_columns, on this handle's kernels): E = R - H X (H' X), the columns' norms read
// back once per round, the correction through the same factors, X(:, j) += correction(:, j) for the columns sensitivity_columns.hpp keeps active
int refine_columns(KH* s, const KktDev& d, const Layout& L, const double* R, bool transposed, int k, double info[4]) {
    DS* t = s->diff;
    double *w = t->ws.p, *X = w + L.X.off, *E = w + L.E.off, *C = w + L.C.off, *Xsave = w + L.Xsave.off, *norms = w + L.norms.off;
    int *active = t->masks.p, *restore = active + k;
    calipso::SensitivityColumns& cols = t->cols;
    cols.begin(k);
    KK(hipEventRecord(t->ev_pass[2], s->st));
    for (;;) {
        KK(hipMemsetAsync(norms, 0, sizeof(double) * (size_t)k, s->st));
        enqueue_mul(s, d, transposed, k, X, R, E, norms);
        KK(hipMemcpyAsync(t->norms.data(), norms, sizeof(double) * (size_t)k, hipMemcpyDeviceToHost, s->st));
        KK(hipStreamSynchronize(s->st));
        KK(hipGetLastError());
        cols.judge(s->opt, t->norms.data());
        if (cols.n_restore) {
            KK(hipMemcpyAsync(restore, cols.restore.data(), sizeof(int) * (size_t)k, hipMemcpyHostToDevice, s->st));
            calipso::launch_restore_masked(s->st, d.N, restore, Xsave, k, X);
            KK(hipStreamSynchronize(s->st));              // (cols.restore is rewritten by the next judge)
        }
        if (cols.finished()) break;
        KK(hipMemcpyAsync(active, cols.active.data(), sizeof(int) * (size_t)k, hipMemcpyHostToDevice, s->st));
        const int rc = map_columns(s, d, transposed, k, E, w + L.rsym.off, w + L.dsym.off, C);
        if (rc < 0) return rc;
        calipso::launch_accumulate_masked(s->st, d.N, active, C, k, X, Xsave);
    }
    cols.report(info);
    KK(hipEventRecord(t->ev_pass[3], s->st));
    t->rounds_ran = true;
    return CALIPSO_OK;
}
// not with second-order cones, where the reference's answer IS the unrefined solve (quirk B-3, columns.hip: rounds_wanted), and not with iterative_refinement = 0
bool rounds_wanted(const KH* s) { return s->differentiate_refinement && s->opt.iterative_refinement && s->d.nsoc == 0; }

// the columns of a call into the workspace: the caller's (host or device) -> L.V
int take_columns(KH* s, const Layout& L, const double* B, bool device) {
    KK(hipMemcpyAsync(s->diff->ws.p + L.V.off, B, sizeof(double) * L.V.len, device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->st));
    return CALIPSO_OK;
}
int give_columns(KH* s, const double* from, size_t count, double* to, bool device) {
    if (to && count) KK(hipMemcpyAsync(to, from, sizeof(double) * count, device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s->st));
    return CALIPSO_OK;
}

int factorize_held(KH* s, const KktDev& d) {
    int64_t in[3] = {0, 0, 0};
    const int rc = assemble_factorize(s, d, s->sc.ep, s->sc.ed, in);
    return rc < 0 ? rc : CALIPSO_OK;
}
// K and its factor were formed at the differentiate slacks: where those are not the resident point's, the single-column entries must assemble again
void leave_factorization(KH* s) { if (s->slacks_kept) { s->assembled = false; s->factored = false; } }

int solve_columns(KH* s, const char* entry, int64_t k, int32_t transposed, const double* B, double* X, bool device) {
    if (!s) return CALIPSO_ERR_ARGUMENT;
    REFUSE(check_columns(entry, k));
    REFUSE(check_array(entry, "B", B)); REFUSE(check_array(entry, "X", X));
    KK(hipSetDevice(s->device));
    DEVPTR(B); DEVPTR(X);
    if (!s->factored) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": factorize first (the columns go through the current factorisation)");
    int rc = ensure_state(s);
    if (rc < 0) return rc;
    const Layout L = layout((size_t)s->d.N, (size_t)s->d.n, (size_t)k, false);
    if ((rc = reserve_pass(s, L, (size_t)k)) < 0 || (rc = take_columns(s, L, B, device)) < 0) return rc;
    double* w = s->diff->ws.p;
    if ((rc = map_columns(s, s->d, transposed != 0, (int)k, w + L.V.off, w + L.rsym.off, w + L.dsym.off, w + L.X.off, s->diff->ev_pass)) < 0) return rc;
    if ((rc = give_columns(s, w + L.X.off, L.X.len, X, device)) < 0) return rc;
    KK(hipStreamSynchronize(s->st));
    KK(hipGetLastError());
    return pass_times(s);
}

// the selected columns of the evaluator's dR/dtheta -> L.V: the evaluator's call, a clear, one launch (columns: k 1-based host indices, NULL = all)
int take_parameter_columns(KH* s, const char* entry, const Layout& L, int64_t k, const int64_t* columns) {
    DS* t = s->diff;
    int rc = parameters_enqueue(s, entry);
    if (rc < 0) return rc;
    const int* sel = nullptr;
    if (columns) {
        if ((rc = device_grown(s, t->sel, (size_t)k)) < 0) return rc;
        t->sel_host.resize((size_t)k);
        for (int64_t c = 0; c < k; ++c) t->sel_host[(size_t)c] = (int)(columns[c] - 1);
        KK(hipMemcpyAsync(t->sel.p, t->sel_host.data(), sizeof(int) * (size_t)k, hipMemcpyHostToDevice, s->st));
        sel = t->sel.p;
    }
    double* V = t->ws.p + L.V.off;
    KK(hipMemsetAsync(V, 0, sizeof(double) * L.V.len, s->st));
    hipLaunchKernelGGL(k_diff_parameter_columns, dim3(calipso::sparse_parameters::scatter_blocks(s->par.longest), (unsigned)k), dim3(KT), 0, s->st, s->d, s->par.d, sel, V);
    return CALIPSO_OK;
}

// jacobian_parameters: the caller's N x k block; NULL (parameters = true): the selected columns of the evaluator's dR/dtheta
int differentiate(KH* s, const char* entry, int64_t k, const double* jacobian_parameters, double* sensitivity, bool device, bool parameters = false, const int64_t* columns = nullptr) {
    if (!s) return CALIPSO_ERR_ARGUMENT;
    if (parameters) {
        if (!s->par.set) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": no parameter patterns set (calipso_hip_sparse_kkt_set_parameter_patterns first)");
        REFUSE(calipso::sparse_parameters::check_selection(entry, s->par.d.np, k, columns));
    } else {
        REFUSE(check_columns(entry, k));
        REFUSE(check_array(entry, "jacobian_parameters", jacobian_parameters));
    }
    REFUSE(check_array(entry, "sensitivity", sensitivity));
    KK(hipSetDevice(s->device));
    if (!parameters) DEVPTR(jacobian_parameters);
    DEVPTR(sensitivity);
    int rc = values_missing(s, entry);
    if (rc < 0 || (rc = ensure_state(s)) < 0) return rc;
    DS* t = s->diff;
    const bool rounds = rounds_wanted(s);
    const Layout L = layout((size_t)s->d.N, (size_t)s->d.n, (size_t)k, rounds);
    if ((rc = reserve_pass(s, L, (size_t)k)) < 0) return rc;
    if ((rc = parameters ? take_parameter_columns(s, entry, L, k, columns) : take_columns(s, L, jacobian_parameters, device)) < 0) return rc;
    const double info0[4] = {(double)k, 0, 0, 0};
    std::copy(info0, info0 + 4, t->info_forward);
    const KktDev d = slacks_view(s);
    if ((rc = factorize_held(s, d)) < 0) return rc;                                           // differentiate.jl:21-27
    double *w = t->ws.p, *X = w + L.X.off;
    rc = map_columns(s, d, false, (int)k, w + L.V.off, w + L.rsym.off, w + L.dsym.off, X, t->ev_pass);     // :29-53 for all columns
    if (rc >= 0 && rounds) rc = refine_columns(s, d, L, w + L.V.off, false, (int)k, t->info_forward);
    leave_factorization(s);
    if (rc < 0) return rc;
    hipLaunchKernelGGL(k_diff_scale, dim3(blocks_of((long long)L.X.len)), dim3(KT), 0, s->st, L.X.len, X, X, -1.0);      // :54-56 sensitivity = -step
    if ((rc = give_columns(s, X, L.X.len, sensitivity, device)) < 0) return rc;
    KK(hipStreamSynchronize(s->st));
    KK(hipGetLastError());
    return pass_times(s);
}

// parameters: grad_theta (np x k) = -R_theta' lambda from the evaluator's dR/dtheta on its stored patterns, instead of the QP's data gradients
int differentiate_adjoint(KH* s, const char* entry, int64_t k, const double* cotangent, double* adjoint, double* const* grad, bool device, bool parameters = false,
                          double* grad_theta = nullptr) {
    if (!s) return CALIPSO_ERR_ARGUMENT;
    REFUSE(check_columns(entry, k));
    REFUSE(check_array(entry, "cotangent", cotangent));
    if (parameters) {
        if (!s->par.set) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": no parameter patterns set (calipso_hip_sparse_kkt_set_parameter_patterns first)");
        REFUSE(check_array(entry, "grad_theta", grad_theta));
    }
    KK(hipSetDevice(s->device));
    DEVPTR(cotangent); DEVPTR(adjoint);
    if (parameters) DEVPTR(grad_theta);
    static const char* const names[6] = {"grad[0] (Lxx)", "grad[1] (q)", "grad[2] (gx)", "grad[3] (b)", "grad[4] (hx)", "grad[5] (hvec)"};
    bool wanted = false;
    for (int i = 0; grad && i < 6; ++i) if (grad[i]) { wanted = true; if (device) { const int rc = device_pointer(s, grad[i], entry, names[i]); if (rc < 0) return rc; } }
    int rc = values_missing(s, entry);
    if (rc < 0 || (rc = ensure_state(s)) < 0) return rc;
    DS* t = s->diff;
    REFUSE(check_gradients(entry, wanted, s->qp_attached, s->have[3]));
    const KktDev& h = s->d;
    const bool rounds = rounds_wanted(s);
    const Layout L = layout((size_t)h.N, (size_t)h.n, (size_t)k, rounds);
    if ((rc = reserve_pass(s, L, (size_t)k)) < 0) return rc;
    const size_t sizes[6] = {(size_t)h.nnzL, (size_t)h.nx, (size_t)h.nnzg, (size_t)h.ne, (size_t)h.nnzh, (size_t)h.nc};
    GradOut out{};
    if (wanted && !device) {                                                                  // a host call's gradients are staged on the device
        size_t total = 0;
        for (int i = 0; i < 6; ++i) if (grad[i]) total += sizes[i] * (size_t)k;
        if ((rc = device_grown(s, t->gbuf, std::max<size_t>(total, 1))) < 0) return rc;
        size_t at = 0;
        for (int i = 0; i < 6; ++i) if (grad[i]) { out.p[i] = t->gbuf.p + at; at += sizes[i] * (size_t)k; }
    } else if (wanted) for (int i = 0; i < 6; ++i) out.p[i] = grad[i];
    const size_t theta_count = parameters ? (size_t)s->par.d.np * (size_t)k : 0;
    double* theta_out = grad_theta;
    if (parameters && !device) {                                                              // ... and so is a host call's grad_theta
        if ((rc = device_grown(s, t->gbuf, theta_count)) < 0) return rc;
        theta_out = t->gbuf.p;
    }
    const double info0[4] = {(double)k, 0, 0, 0};
    std::copy(info0, info0 + 4, t->info_reverse);
    t->times[0] = t->times[1] = t->times[2] = 0.0;
    KK(hipEventRecord(t->ev[0], s->st));
    if ((rc = take_columns(s, L, cotangent, device)) < 0) return rc;
    if (parameters && (rc = parameters_enqueue(s, entry)) < 0) return rc;                     // dR/dtheta at the resident point and theta, on the handle's stream
    const KktDev d = slacks_view(s);
    if ((rc = factorize_held(s, d)) < 0) return rc;
    double *w = t->ws.p, *V = w + L.V.off, *X = w + L.X.off;
    rc = map_columns(s, d, true, (int)k, V, w + L.rsym.off, w + L.dsym.off, X, t->ev_pass);          // differentiate.jl:29-58 transposed, all columns at once
    if (rc >= 0 && rounds) rc = refine_columns(s, d, L, V, true, (int)k, t->info_reverse);
    leave_factorization(s);
    if (rc < 0) return rc;
    if (wanted) {
        const long long items = (long long)h.nnzL + h.nx + h.nnzg + h.ne + h.nnzh + h.nc;
        KK(hipEventRecord(t->ev[2], s->st));
        hipLaunchKernelGGL(k_diff_gradients, dim3(blocks_of(items), (unsigned)k), dim3(KT), 0, s->st, h, s->w, X, out);      // x, y, z: the resident point's
        KK(hipEventRecord(t->ev[3], s->st));
    }
    if (parameters) {
        const calipso::sparse_parameters::Geometry geo = calipso::sparse_parameters::geometry(s->par.d.np, s->par.d.n_long);
        KK(hipEventRecord(t->ev[2], s->st));
        hipLaunchKernelGGL(k_diff_parameter_gradient, dim3(geo.blocks, (unsigned)k), dim3(KT), 0, s->st, h, s->par.d, X, theta_out);
        KK(hipEventRecord(t->ev[3], s->st));
    }
    KK(hipEventRecord(t->ev[1], s->st));
    if ((rc = give_columns(s, X, L.X.len, adjoint, device)) < 0) return rc;
    if (parameters && !device && (rc = give_columns(s, theta_out, theta_count, grad_theta, false)) < 0) return rc;
    if (wanted && !device) for (int i = 0; i < 6; ++i) if (grad[i] && (rc = give_columns(s, out.p[i], sizes[i] * (size_t)k, grad[i], false)) < 0) return rc;
    KK(hipEventRecord(t->ev[4], s->st));
    KK(hipStreamSynchronize(s->st));
    KK(hipGetLastError());
    float ms = 0.f;
    KK(hipEventElapsedTime(&ms, t->ev[0], t->ev[1])); t->times[0] = ms;
    KK(hipEventElapsedTime(&ms, t->ev[1], t->ev[4])); t->times[1] = ms;
    if (wanted || parameters) { KK(hipEventElapsedTime(&ms, t->ev[2], t->ev[3])); t->times[2] = ms; }
    return pass_times(s);
}

}  // namespace

namespace calipso {
namespace sparse_kkt {

void diff_state_release(KH* s) {
    DS* t = s->diff;
    if (!t) return;
    for (hipEvent_t e : t->ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : t->ev_pass) if (e) (void)hipEventDestroy(e);
    delete t;
    s->diff = nullptr;
}

int diff_set_option(KH* s, const char* name, double value) {
    if (std::strcmp(name, "differentiate_refinement")) return 0;
    if (!refinement_option(value)) return fail(s, CALIPSO_ERR_ARGUMENT, "calipso_hip_sparse_kkt_set_option: differentiate_refinement is 0 or 1");
    s->differentiate_refinement = value == 1.0;
    return 1;
}

}  // namespace sparse_kkt
}  // namespace calipso

extern "C" {

int32_t calipso_hip_sparse_kkt_solve_columns(calipso_hip_sparse_kkt* s, int64_t k, int32_t transposed, const double* B, double* X) {
    return solve_columns(s, "calipso_hip_sparse_kkt_solve_columns", k, transposed, B, X, false);
}
int32_t calipso_hip_sparse_kkt_solve_columns_device(calipso_hip_sparse_kkt* s, int64_t k, int32_t transposed, const double* B, double* X) {
    return solve_columns(s, "calipso_hip_sparse_kkt_solve_columns_device", k, transposed, B, X, true);
}
int32_t calipso_hip_sparse_kkt_differentiate(calipso_hip_sparse_kkt* s, int64_t k, const double* jacobian_parameters, double* sensitivity) {
    return differentiate(s, "calipso_hip_sparse_kkt_differentiate", k, jacobian_parameters, sensitivity, false);
}
int32_t calipso_hip_sparse_kkt_differentiate_device(calipso_hip_sparse_kkt* s, int64_t k, const double* jacobian_parameters, double* sensitivity) {
    return differentiate(s, "calipso_hip_sparse_kkt_differentiate_device", k, jacobian_parameters, sensitivity, true);
}
int32_t calipso_hip_sparse_kkt_differentiate_adjoint(calipso_hip_sparse_kkt* s, int64_t k, const double* cotangent, double* adjoint, double* const* grad) {
    return differentiate_adjoint(s, "calipso_hip_sparse_kkt_differentiate_adjoint", k, cotangent, adjoint, grad, false);
}
int32_t calipso_hip_sparse_kkt_differentiate_adjoint_device(calipso_hip_sparse_kkt* s, int64_t k, const double* cotangent, double* adjoint, double* const* grad) {
    return differentiate_adjoint(s, "calipso_hip_sparse_kkt_differentiate_adjoint_device", k, cotangent, adjoint, grad, true);
}
int32_t calipso_hip_sparse_kkt_differentiate_parameters(calipso_hip_sparse_kkt* s, int64_t k, const int64_t* columns, double* sensitivity) {
    return differentiate(s, "calipso_hip_sparse_kkt_differentiate_parameters", k, nullptr, sensitivity, false, true, columns);
}
int32_t calipso_hip_sparse_kkt_differentiate_parameters_device(calipso_hip_sparse_kkt* s, int64_t k, const int64_t* columns, double* sensitivity) {
    return differentiate(s, "calipso_hip_sparse_kkt_differentiate_parameters_device", k, nullptr, sensitivity, true, true, columns);
}
int32_t calipso_hip_sparse_kkt_differentiate_adjoint_parameters(calipso_hip_sparse_kkt* s, int64_t k, const double* cotangent, double* adjoint, double* grad_theta) {
    return differentiate_adjoint(s, "calipso_hip_sparse_kkt_differentiate_adjoint_parameters", k, cotangent, adjoint, nullptr, false, true, grad_theta);
}
int32_t calipso_hip_sparse_kkt_differentiate_adjoint_parameters_device(calipso_hip_sparse_kkt* s, int64_t k, const double* cotangent, double* adjoint, double* grad_theta) {
    return differentiate_adjoint(s, "calipso_hip_sparse_kkt_differentiate_adjoint_parameters_device", k, cotangent, adjoint, nullptr, true, true, grad_theta);
}
int32_t calipso_hip_sparse_kkt_differentiate_info(calipso_hip_sparse_kkt* s, double out[4]) {
    if (!s || !out) return CALIPSO_ERR_ARGUMENT;
    const double zero[4] = {0, 0, 0, 0};
    const double* from = s->diff ? s->diff->info_forward : zero;
    std::copy(from, from + 4, out);
    return CALIPSO_OK;
}
int32_t calipso_hip_sparse_kkt_differentiate_adjoint_info(calipso_hip_sparse_kkt* s, double out[4]) {
    if (!s || !out) return CALIPSO_ERR_ARGUMENT;
    const double zero[4] = {0, 0, 0, 0};
    const double* from = s->diff ? s->diff->info_reverse : zero;
    std::copy(from, from + 4, out);
    return CALIPSO_OK;
}
int32_t calipso_hip_sparse_kkt_differentiate_bytes(calipso_hip_sparse_kkt* s, int64_t* out) {
    if (!s || !out) return CALIPSO_ERR_ARGUMENT;
    const DS* t = s->diff;
    *out = t ? (int64_t)(sizeof(double) * (t->ws.cap + t->gbuf.cap + (size_t)s->d.N) + sizeof(int) * (t->masks.cap + t->sel.cap)) : 0;
    return CALIPSO_OK;
}
int32_t calipso_hip_sparse_kkt_differentiate_adjoint_times(calipso_hip_sparse_kkt* s, double out[3]) {
    if (!s || !out) return CALIPSO_ERR_ARGUMENT;
    const double zero[3] = {0, 0, 0};
    const double* from = s->diff ? s->diff->times : zero;
    std::copy(from, from + 3, out);
    return CALIPSO_OK;
}

}  // extern "C"
