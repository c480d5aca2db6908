// columns.hip — p columns through the current factors together: the condensed solve of differentiate.jl:29-58 for differentiate! (parameter columns), for its reverse
// mode (the same pipeline stage by stage in reverse order, on cotangent columns) and the correction rounds of iterative_refinement.jl:14-44 on either.  ONE pipeline
// with two directions: a direction only chooses the kernels before and after the middle.  Either direction has a second caller, a group in lockstep
// (differentiate_columns_group, differentiate_columns_t_group: the members' columns side by side in the group's workspace, every launch covering all members).  Host code;
// the kernels are vectors / adjoint / soc_wide / gemm / blocks.hip's.
#include <cstdio>
#include "internal.hpp"
#include "host_logic.hpp"
#include "column_layout.hpp"

namespace calipso {

// Every buffer of a p-column pass: grown on demand, never shrunk, kept (a call that repeats its shapes allocates nothing), a fresh allocation zero-filled on the
// handle's stream (non-blocking: a fill on the null stream would not be ordered with what follows), counted in scratch_bytes but for its first `uncounted` elements
int reserve_device(H* s, void** buf, size_t* have, size_t want, size_t elem, size_t uncounted, const char* caller, const char* what) {
    if (want <= *have) return CALIPSO_OK;
    CK(hipStreamSynchronize(s->stream));           // (nothing queued may still use the buffer that goes)
    if (*buf) { (void)hipFree(*buf); *buf = nullptr; s->scratch_bytes -= (*have - uncounted) * elem; *have = 0; }
    if (hipMalloc(buf, want * elem) != hipSuccess) {
        (void)hipGetLastError(); *buf = nullptr;
        char msg[192];
        snprintf(msg, sizeof msg, "%s: %s (%zu bytes) could not be allocated", caller, what, want * elem);
        s->err = msg; return CALIPSO_ERR_HIP;
    }
    CK(hipMemsetAsync(*buf, 0, want * elem, s->stream));
    *have = want; s->scratch_bytes += (want - uncounted) * elem;
    return CALIPSO_OK;
}
static ColumnLayout layout_of(const H* s, int p, bool transposed, bool rounds, size_t extra) {
    return column_layout((size_t)s->d.n, (size_t)s->d.N, (size_t)s->d.NP, (size_t)s->d.m, (size_t)p, transposed, rounds, (size_t)refine_multi_parts(s), extra);
}
static int reserve_pass(H* s, ColumnWorkspace& ws, const ColumnLayout& L, int p, bool rounds, size_t uncounted, const char* caller) {
    int rc = reserve_device(s, (void**)&ws.d, &ws.doubles, L.total, sizeof(double), uncounted, caller, "the workspace of the column solve");
    if (rc < 0 || !rounds) return rc;
    if (ws.norms.size() < (size_t)p) ws.norms.assign((size_t)p, 0.0);
    return reserve_device(s, (void**)&ws.active, &ws.ints, 2 * (size_t)p, sizeof(int), 0, caller, "the column masks of the correction rounds");
}

// The products with p columns, each choice made once: the stage blocks where the handle works on them (every structured handle: all columns in one launch), else a
// structured handle has no dense arrays to fall back to, else the dense GEMM (gemm_columns: a group's pass takes its batched form, all members in one launch)
static int refuse(H* s, const char* msg) { s->err = msg; return CALIPSO_ERR_HIP; }
static const char* const NO_BLOCK_PRODUCTS = "calipso_hip_differentiate: the block products are not available on this structured handle";
static int constraints_t_columns(H* s, const double* U, long long ldu, double* Y, long long ldy, int p, double beta) {      // Y = [gx; hx]' U + beta Y
    const Dims& d = s->d;
    if (!d.m || blocks_gemm_t(s, U, ldu, Y, ldy, p, beta)) return CALIPSO_OK;
    if (s->compact) return refuse(s, NO_BLOCK_PRODUCTS);
    gemm_columns(s, d.nx, p, d.m, 1.0, s->Z, d.m, true, U, (int)ldu, beta, Y, (int)ldy);
    return CALIPSO_OK;
}
static int constraints_columns(H* s, const double* X, long long ldx, double* Y, int p) {                                    // Y (m apart) = [gx; hx] X
    const Dims& d = s->d;
    if (!d.m || blocks_gemm_n(s, X, ldx, Y, d.m, p)) return CALIPSO_OK;
    if (s->compact) return refuse(s, NO_BLOCK_PRODUCTS);
    gemm_columns(s, d.m, p, d.nx, 1.0, s->Z, d.m, false, X, (int)ldx, 0.0, Y, d.m);
    return CALIPSO_OK;
}
static int hessian_columns(H* s, const double* X, long long ldx, double* Y, long long ldy, int p, bool transposed) {       // Y = Lxx X (transposed: Lxx' X)
    if (blocks_gemm_l(s, X, ldx, Y, ldy, p, transposed)) return CALIPSO_OK;
    if (s->compact) return refuse(s, "calipso_hip_differentiate: the Hessian block product is not available on this structured handle");
    gemm_columns(s, s->d.nx, p, s->d.nx, 1.0, s->Lxx, s->d.nx, transposed, X, (int)ldx, 0.0, Y, (int)ldy);
    return CALIPSO_OK;
}

// The middle of the condensed pipeline, the same in both directions (S is symmetric): xbuf += [gx; hx]' seed, xbuf = S^-1 xbuf, out = [gx; hx] xbuf (a structured handle's
// factor lives in the fronts of the multifrontal LDL^T, which take all columns through the tree together: trsm_multi).  matvec_for_one: a single column takes the
// triangular solve and the mat-vecs of a Newton step's condensed solve (linear_solve_device) instead — the transposed direction asks for it, the forward one keeps the
// GEMM forms' bits, and so does a group's pass (the mat-vecs work on the handles' own vectors: they cannot address the group's workspace)
static int condensed_middle(H* s, const double* seed, double* xbuf, double* u, double* z, double* out, int p, bool matvec_for_one) {
    const Dims& d = s->d;
    if (matvec_for_one && p == 1 && !s->compact && !s->group_columns) {
        if (d.m) gemv_t(s, d.m, d.nx, s->Z, d.m, seed, xbuf, 1.0, 1.0, SP_Z);
        launch_trsv(s, xbuf);
        if (d.m) gemv_n(s, d.m, d.nx, s->Z, d.m, xbuf, out, 1.0, 0.0, SP_Z);
        return CALIPSO_OK;
    }
    const int rc = constraints_t_columns(s, seed, d.m, xbuf, d.NP, p, 1.0);
    if (rc < 0) return rc;
    trsm_multi(s, xbuf, p, u, z);
    return constraints_columns(s, xbuf, d.NP, out, p);
}
// out = scale * H^-1 rhs for p right-hand-side columns (N apart), as far as the condensed, constraint-first solve gets.  The reference solves one condensed system per
// parameter column; here condensation per column, mat-vecs as GEMMs, block triangular solves as TRSMs.  A group's pass: p columns of every member the launches cover — rhs and
// out in the members' slabs, L the layout of all members' columns (every region is reached by the member's slot)
static int solve_columns(H* s, double* w, const ColumnLayout& L, const double* rhs, int p, double* out, double scale) {
    double *rsym = w + L.rsym.off, *xbuf = w + L.xbuf.off, *t1 = w + L.t1.off, *t2 = w + L.t2.off;
    launch_residual_symmetric_multi(s, rhs, p, rsym, xbuf, t1);                             // rsym, xbuf = [b_x; 0], t1 = Omega b_m
    const int rc = condensed_middle(s, t1, xbuf, w + L.u.off, w + L.z.off, t2, p, false);   // xbuf = dx, t2 = [gx; hx] dx
    if (rc < 0) return rc;
    launch_recover_multi(s, rhs, p, rsym, xbuf, t2, w + L.dsym.off, out, scale);
    return CALIPSO_OK;
}
// lam = M' V for the map M solve_columns applies to a column (scale 1), p cotangent columns V (N apart): its stages in reverse order
static int solve_columns_t(H* s, double* w, const ColumnLayout& L, const double* V, int p, double* lam) {
    double *xbuf = w + L.xbuf.off, *g = w + L.t1.off, *t2 = w + L.t2.off;
    launch_recover_t_multi(s, V, p, lam, g, xbuf);                                          // g: the seed of the x-system, xbuf = [V_x; 0]
    const int rc = condensed_middle(s, g, xbuf, w + L.u.off, w + L.z.off, t2, p, true);     // xbuf = xb, t2 = [gx; hx] xb
    if (rc < 0) return rc;
    launch_residual_symmetric_t_multi(s, p, g, xbuf, t2, lam);
    return CALIPSO_OK;
}
// E = R - H X for all p columns with the unreduced, matrix-free H (what k_refine_local / k_refine_x form for one vector), and their infinity norms
// (transposed: E = R - H' X — Lxx' X_x in the x rows, the (s, t) rows swapped (k_refine_rows_multi); every other block of H is symmetric)
static int residual_columns(H* s, double* w, const ColumnLayout& L, const double* R, bool transposed, int p) {
    const Dims& d = s->d;
    double *X = w + L.X.off, *hx = w + L.hx.off, *zx = w + L.zx.off, *E = w + L.E.off, *part = w + L.part.off;
    int rc = hessian_columns(s, X, d.N, hx, d.NP, p, transposed);                           // Lxx X_x (Lxx' X_x)
    if (rc >= 0) rc = constraints_t_columns(s, X + d.oy(), d.N, hx, d.NP, p, 1.0);          // + [gx; hx]' X_yz (y and z are adjacent in a Point)
    if (rc >= 0) rc = constraints_columns(s, X, d.N, zx, p);                                // [gx; hx] X_x
    if (rc < 0) return rc;
    launch_refine_rows_multi(s, X, R, zx, p, E, part, transposed);
    launch_refine_x_multi(s, X, R, hx, d.NP, p, E, part, w + L.norms.off);
    return CALIPSO_OK;
}
// The loop of iterative_refinement.jl:14-44 over the p columns of X at once: residual against the unreduced matrix, column norms (one read-back of p doubles per round),
// the correction through the same factors and the same pipeline, X(:, j) += correction(:, j) for the columns still active.  The per-column decisions are
// sensitivity_columns.hpp's: a column that fails its test keeps its last iterate and is counted (differentiate! has no fallback); a column already within the tolerance
// takes the round min_iterative_refinement asks for only if that does not raise its norm (its iterate is saved and put back)
static int refine_columns(H* s, ColumnWorkspace& ws, const ColumnLayout& L, const double* R, bool transposed, int p, const char* refused) {
    double *w = ws.d, *X = w + L.X.off, *E = w + L.E.off, *C = w + L.C.off, *Xsave = w + L.Xsave.off;
    SensitivityColumns& cols = ws.cols;
    cols.begin(p);
    for (;;) {
        int rc = residual_columns(s, w, L, R, transposed, p);
        if (rc < 0) return rc;
        CK(hipMemcpyAsync(ws.norms.data(), w + L.norms.off, sizeof(double) * (size_t)p, hipMemcpyDeviceToHost, s->stream));
        if (launch_errors(s, refused)) return CALIPSO_ERR_HIP;
        SYNC();
        cols.judge(s->opt, ws.norms.data());
        if (cols.n_restore) {      // a round that only min_iterative_refinement asked for raised these columns' norms: they go back to the iterate they had
            CK(hipMemcpyAsync(ws.active + p, cols.restore.data(), sizeof(int) * (size_t)p, hipMemcpyHostToDevice, s->stream));
            launch_restore_masked(s, ws.active + p, Xsave, p, X);
            SYNC();                // (cols.restore is rewritten by the next judge)
        }
        if (cols.finished()) break;
        CK(hipMemcpyAsync(ws.active, cols.active.data(), sizeof(int) * (size_t)p, hipMemcpyHostToDevice, s->stream));
        rc = transposed ? solve_columns_t(s, w, L, E, p, C) : solve_columns(s, w, L, E, p, C, 1.0);
        if (rc < 0) return rc;
        launch_accumulate_masked(s, ws.active, C, p, X, Xsave);
    }
    cols.report(ws.info);
    return CALIPSO_OK;
}

// "opt.differentiate_refinement": correction rounds on all columns — not with second-order cones, where the reference's answer IS the unrefined solve with its
// triu-symmetrised cone blocks (quirk B-3: refining would move away from it, towards H^-1; the batch kernel does the same), and not with iterative_refinement = 0
static bool rounds_wanted(const H* s) { return s->differentiate_refinement && s->opt.iterative_refinement && s->d.n_soc == 0; }

// The forward pass for `members` x np parameter columns in the workspace ws: a handle alone (members = 1, its own workspace, the rounds where it asks for them) or the members
// of a group (the group's workspace, laid out for members x np columns; no rounds).  R and solution_sensitivity are the members' own (Batch::delta)
static int columns_pass(H* s, ColumnWorkspace& ws, int members, bool rounds, const char* caller) {
    const int p = s->d.np, cols = members * p;
    const ColumnLayout L = layout_of(s, cols, false, rounds, 0);
    // (a handle's unrefined pipeline's share of the buffer is left out of scratch_bytes, as it always was: counting it is a correction for a change of its own)
    int rc = reserve_pass(s, ws, L, cols, rounds, members == 1 ? layout_of(s, p, false, false, 0).total : 0, caller);
    if (rc < 0) return rc;
    double *w = ws.d, *R = s->jacobian_parameters;
    // one condensed solve for all np columns, unrefined as the reference's (its QDLDL works on the (nx + ne + nc) symmetric matrix and does not need more)
    if (!rounds) return solve_columns(s, w, L, R, p, s->solution_sensitivity, -1.0);       // :54-56 sensitivity = -step
    rc = solve_columns(s, w, L, R, p, w + L.X.off, 1.0);                                    // the unrefined pass kept as the step matrix X
    if (rc >= 0) rc = refine_columns(s, ws, L, R, false, p, "a kernel launch of differentiate!'s correction rounds was refused");
    if (rc >= 0) launch_scale_into(s, w + L.X.off, s->solution_sensitivity, L.X.len, -1.0);
    return rc < 0 ? rc : CALIPSO_OK;
}
int differentiate_columns(H* s) { return columns_pass(s, s->fwd, 1, rounds_wanted(s), "calipso_hip_differentiate"); }
// (tile = 0: the 64-column form of the batched products from GROUP_WIDE_TILE_COLUMNS parameter columns per member on.  Measured: the 16-column form is faster at 24, 48
// and 102 columns, the two tie at 540, the 64-column form is faster at 770 and 1200 — DESIGN.md, "Forward mode for a group")
constexpr int GROUP_WIDE_TILE_COLUMNS = 512;
int differentiate_columns_group(H* s, ColumnWorkspace& ws, int count, int tile) {
    s->group_columns = true;
    s->group_tile = tile ? tile : (s->d.np >= GROUP_WIDE_TILE_COLUMNS ? 64 : 16);
    const int rc = columns_pass(s, ws, count, false, "calipso_hip_group_differentiate");
    s->group_columns = false; s->group_tile = 0;
    return rc;
}
// The reverse pass for `members` x p cotangent columns in the workspace ws: a handle alone (members = 1, its own workspace, the rounds where it asks for them) or the members
// of a group (the group's workspace: the layout of members x p columns IS the group's — every region holds the members' columns slot after slot —, no rounds)
static int columns_t_pass(H* s, ColumnWorkspace& ws, int members, int p, const double* cotangent, bool with_theta, bool rounds, const char* caller, const double** lam,
                          const double** grad_theta) {
    const Dims& d = s->d;
    const int cols = members * p;
    const ColumnLayout L = layout_of(s, cols, true, rounds, with_theta ? (size_t)d.np * (size_t)cols : 0);
    int rc = reserve_pass(s, ws, L, cols, rounds, 0, caller);
    if (rc < 0) return rc;
    double *w = ws.d, *V = w + L.V.off, *X = w + L.X.off, *gth = w + L.grad_theta.off;
    CK(hipMemcpyAsync(V, cotangent, sizeof(double) * L.V.len, hipMemcpyHostToDevice, s->stream));
    rc = solve_columns_t(s, w, L, V, p, X);        // :29-58 transposed, all p columns (of every member) at once
    if (rc >= 0 && rounds) rc = refine_columns(s, ws, L, V, true, p, "a kernel launch of the reverse mode's correction rounds was refused");
    if (rc < 0) return rc;
    if (with_theta) gemm_columns(s, d.np, p, d.N, -1.0, s->jacobian_parameters, d.N, true, X, d.N, 0.0, gth, d.np);      // -R_theta' lam = S' v
    *lam = X; *grad_theta = gth;
    return CALIPSO_OK;
}
int differentiate_columns_t(H* s, int p, const double* cotangent, bool with_theta, const double** lam, const double** grad_theta) {
    return columns_t_pass(s, s->rev, 1, p, cotangent, with_theta, rounds_wanted(s), "calipso_hip_differentiate_adjoint", lam, grad_theta);
}
int differentiate_columns_t_group(H* s, ColumnWorkspace& ws, int count, int p, const double* cotangent, bool with_theta, const double** lam, const double** grad_theta) {
    s->group_columns = true;
    const int rc = columns_t_pass(s, ws, count, p, cotangent, with_theta, false, "calipso_hip_group_differentiate_adjoint", lam, grad_theta);
    s->group_columns = false;
    return rc;
}

}  // namespace calipso
