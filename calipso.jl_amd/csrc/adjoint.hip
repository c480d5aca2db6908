// adjoint.hip — differentiate! in reverse mode on a Solver handle (api.hip: calipso_hip_differentiate_adjoint): the first and the last stage of the condensed solve
// of differentiate.jl:29-58, transposed, for p cotangent columns in grid.y, and the gradients with respect to the data of an attached QP.
//   search_direction.jl:38-101 (k_recover: back-substitution through the constraint pivots, recovery of dr, ds, dt)   transposed -> k_recover_t
//   residual.jl:53-101 (k_residual_symmetric: the condensed right-hand side b and t1 = Omega b_m)                    transposed -> k_residual_symmetric_t
//   residual_jacobian_parameters.jl:1-40 for the data of min c x'Px + q'x, Ax = b, h - Gx in K (qp.hip)               transposed -> k_qp_grad_matrix / k_qp_grad_vectors
// The stages between the two (Z'., S^-1, Z.) are their own transposes (S is factored from one triangle).  With M the map a column of differentiate! goes through
// (step = M residual), lam = M' v is formed in two passes over the constraint rows: k_recover_t writes the first contributions to the r, s, t rows of lam and the
// m-vector g that seeds the x-system; behind xb = S^-1 (v_x + Z' g) and t1 = Z xb, k_residual_symmetric_t writes lam_x, lam_y, lam_z and ADDS the second contributions to
// the r, s, t rows — the same work item that wrote the first ones, so nothing is atomic.  Second-order cones of dimension <= 4: one lane per cone, registers, loops
// unrolled to constant indices (as the forward kernels of vectors.hip); wider cones: one wavefront per cone (soc_wide.hip).  W (the cone's block of Omega) is applied
// transposed by swapping its indices: nothing here assumes that it is symmetric.  The dt recovery keeps the reference's quirk (second_order.jl:63-65: the arrow inverse
// sees the first row of Cbar_t only), so this is the transpose of the map the forward kernels compute, not of H^-1.
// Every kernel takes the instance from blockIdx.z (a handle alone is a batch of one): the point, the cone weights and the scalars are the member's (Batch::delta,
// BatchSc::scal), the column regions hold the members' columns slot after slot (device_utils.hpp: column_shift) — calipso_hip_group_differentiate_adjoint (group.hip).
#include "internal.hpp"
#include "device_utils.hpp"

namespace calipso {

constexpr int ADJ_THREADS = 128;

// work items: [0, NP) xbuf = [v_x; 0]; then one per equality row, per nonnegative entry, per second-order cone
__global__ __launch_bounds__(ADJ_THREADS) void k_recover_t(BatchSc bt, Dims d, ConeDev cd, const double* __restrict__ w, const double* __restrict__ V_,
                                                            const double* __restrict__ wz, const double* __restrict__ Wsoc, double* __restrict__ lam_,
                                                            double* __restrict__ g_, double* __restrict__ xbuf_) {
    inst_shift(bt.b, w, wz, Wsoc);
    const Scalars sc = bt.scal(blockIdx.z);
    const size_t col = column_shift(bt.b, gridDim.y) + blockIdx.y;      // the column among the columns of all members
    const double* v = V_ + col * d.N;
    double* lam = lam_ + col * d.N;
    double* g = g_ + col * d.m;
    double* xbuf = xbuf_ + col * d.NP;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const double Hrr = sc.rho + sc.ep, Hss = 0.0 + sc.ep;
    if (i < d.NP) { xbuf[i] = i < d.nx ? v[i] : 0.0; return; }
    const int e = i - d.NP;
    if (e < d.ne) {
        // dr = (r_r + dy) / Hrr, dy = -omega_y (b_y - t2_y)
        const double omega_y = -1.0 / (-1.0 / (sc.rho + sc.ep) + (0.0 - sc.ed));
        const double vr = v[d.orr() + e] / Hrr;
        lam[d.orr() + e] = vr;
        g[e] = omega_y * (v[d.oy() + e] + vr);
    } else if (e < d.ne + d.q) {
        // dt = (r_t - T ds) / Sb, ds = (r_t + Sb (r_s + dz)) / den, dz = -wz (b_z - t2_z)
        const int k = e - d.ne;
        const double Sb = w[d.os() + k] - sc.ed, Ti = w[d.ot() + k], den = Ti + Sb * Hss;
        const double vt = v[d.ot() + k] / Sb;
        const double gg = (v[d.os() + k] - Ti * vt) / den;
        lam[d.ot() + k] = vt + gg;
        lam[d.os() + k] = Sb * gg;
        g[d.ne + k] = wz[k] * (v[d.oz() + k] + Sb * gg);
    } else if (e < d.ne + d.q + d.n_soc) {
        const int j = e - d.ne - d.q;
        const int st = cd.soc_start[j], dim = cd.soc_dim[j];
        if (dim > 4) return;                       // k_recover_t_wide (soc_wide.hip)
        constexpr int MD = 4;
        double sl[MD], t[MD], vs[MD], vt[MD], vz[MD], u[MD], ct[MD], a[MD], b[MD], a2[MD], W[MD * MD];
        const int woff = cd.soc_woff[j];
#pragma unroll
        for (int k = 0; k < MD; ++k) {
            const bool in = k < dim;
            sl[k] = in ? w[d.os() + st + k] : 0.0; t[k] = in ? w[d.ot() + st + k] : 0.0;
            vs[k] = in ? v[d.os() + st + k] : 0.0; vt[k] = in ? v[d.ot() + st + k] : 0.0; vz[k] = in ? v[d.oz() + st + k] : 0.0;
            u[k] = 0.0; ct[k] = 0.0; a[k] = 0.0; b[k] = 0.0; a2[k] = 0.0;
        }
#pragma unroll
        for (int e2 = 0; e2 < MD * MD; ++e2) W[e2] = 0.0;
#pragma unroll
        for (int c = 0; c < MD; ++c)
#pragma unroll
            for (int r = 0; r < MD; ++r) if (r < dim && c < dim) W[r + c * MD] = Wsoc[woff + r + c * dim];
        const double sb1 = sl[0] - sc.ed;
        ct[0] = sb1; u[0] = t[0] + sb1 * Hss;
#pragma unroll
        for (int k = 1; k < MD; ++k) if (k < dim) { ct[k] = sl[k]; u[k] = t[k] + sl[k] * Hss; }
        arrow_inverse_t_small<MD>(dim, ct, vt, a);                 // dt = arrow_inverse(first row of Cbar_t, r_t - arrow(t) ds)
        double acc = t[0] * a[0];
#pragma unroll
        for (int k = 1; k < MD; ++k) if (k < dim) acc += t[k] * a[k];
        b[0] = vs[0] - acc;
#pragma unroll
        for (int k = 1; k < MD; ++k) if (k < dim) b[k] = vs[k] - (t[k] * a[0] + t[0] * a[k]);
        arrow_inverse_t_small<MD>(dim, u, b, a2);                  // ds = arrow_inverse(u, r_t + Cbar_t (r_s + dz))
        acc = sb1 * a2[0];
#pragma unroll
        for (int k = 1; k < MD; ++k) if (k < dim) acc += sl[k] * a2[k];
        b[0] = acc;                                               // Cbar_t' a2
#pragma unroll
        for (int k = 1; k < MD; ++k) if (k < dim) b[k] = sl[k] * a2[0] + sb1 * a2[k];
#pragma unroll
        for (int k = 0; k < MD; ++k) if (k < dim) {
            lam[d.ot() + st + k] = a[k] + a2[k];
            lam[d.os() + st + k] = b[k];
            b[k] = vz[k] + b[k];
        }
#pragma unroll
        for (int c = 0; c < MD; ++c) if (c < dim) {                // dz = -W (b_z - t2_z): W' by swapped indices
            double ss = 0.0;
#pragma unroll
            for (int r = 0; r < MD; ++r) if (r < dim) ss += W[r + c * MD] * b[r];
            g[d.ne + st + c] = ss;
        }
    }
}

// work items: [0, nx) lam_x = xb; then one per equality row, per nonnegative entry, per second-order cone (the item that wrote the row's first contributions)
__global__ __launch_bounds__(ADJ_THREADS) void k_residual_symmetric_t(BatchSc bt, Dims d, ConeDev cd, const double* __restrict__ w, const double* __restrict__ g_,
                                                                       const double* __restrict__ xb_, const double* __restrict__ t1_, const double* __restrict__ wz,
                                                                       const double* __restrict__ Wsoc, double* __restrict__ lam_) {
    inst_shift(bt.b, w, wz, Wsoc);
    const Scalars sc = bt.scal(blockIdx.z);
    const size_t col = column_shift(bt.b, gridDim.y) + blockIdx.y;
    const double* g = g_ + col * d.m;
    const double* xb = xb_ + col * d.NP;
    const double* t1 = t1_ + col * d.m;
    double* lam = lam_ + col * d.N;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const double Hrr = sc.rho + sc.ep, Hss = 0.0 + sc.ep;
    if (i < d.nx) { lam[i] = xb[i]; return; }
    const int e = i - d.nx;
    if (e < d.ne) {
        // b_y = r_y + r_r / Hrr, t1_y = omega_y b_y
        const double omega_y = -1.0 / (-1.0 / (sc.rho + sc.ep) + (0.0 - sc.ed));
        const double tot = -g[e] + omega_y * t1[e];
        lam[d.oy() + e] = tot;
        lam[d.orr() + e] += tot / Hrr;
    } else if (e < d.ne + d.q) {
        // b_z = r_z + (r_t + Sb r_s) / den, t1_z = wz b_z
        const int k = e - d.ne;
        const double Sb = w[d.os() + k] - sc.ed, Ti = w[d.ot() + k], den = Ti + Sb * Hss;
        const double tot = -g[d.ne + k] + wz[k] * t1[d.ne + k];
        lam[d.oz() + k] = tot;
        lam[d.ot() + k] += tot / den;
        lam[d.os() + k] += Sb * tot / den;
    } else if (e < d.ne + d.q + d.n_soc) {
        // b_z = r_z + arrow_inverse(u, Cbar_t r_s + r_t), t1_z = W b_z
        const int j = e - d.ne - d.q;
        const int st = cd.soc_start[j], dim = cd.soc_dim[j];
        if (dim > 4) return;                       // k_residual_symmetric_t_wide (soc_wide.hip)
        constexpr int MD = 4;
        double sl[MD], t[MD], gg[MD], tt[MD], ls[MD], lt[MD], u[MD], bz[MD], a[MD], W[MD * MD];
        const int woff = cd.soc_woff[j];
#pragma unroll
        for (int k = 0; k < MD; ++k) {
            const bool in = k < dim;
            sl[k] = in ? w[d.os() + st + k] : 0.0; t[k] = in ? w[d.ot() + st + k] : 0.0;
            gg[k] = in ? g[d.ne + st + k] : 0.0; tt[k] = in ? t1[d.ne + st + k] : 0.0;
            ls[k] = in ? lam[d.os() + st + k] : 0.0; lt[k] = in ? lam[d.ot() + st + k] : 0.0;
            u[k] = 0.0; bz[k] = 0.0; a[k] = 0.0;
        }
#pragma unroll
        for (int e2 = 0; e2 < MD * MD; ++e2) W[e2] = 0.0;
#pragma unroll
        for (int c = 0; c < MD; ++c)
#pragma unroll
            for (int r = 0; r < MD; ++r) if (r < dim && c < dim) W[r + c * MD] = Wsoc[woff + r + c * dim];
        const double sb1 = sl[0] - sc.ed;
        u[0] = t[0] + sb1 * Hss;
#pragma unroll
        for (int k = 1; k < MD; ++k) if (k < dim) u[k] = t[k] + sl[k] * Hss;
#pragma unroll
        for (int c = 0; c < MD; ++c) if (c < dim) {
            double ss = 0.0;
#pragma unroll
            for (int r = 0; r < MD; ++r) if (r < dim) ss += W[r + c * MD] * tt[r];
            bz[c] = -gg[c] + ss;
        }
        arrow_inverse_t_small<MD>(dim, u, bz, a);
        double acc = sb1 * a[0];
#pragma unroll
        for (int k = 1; k < MD; ++k) if (k < dim) acc += sl[k] * a[k];
        ls[0] += acc;
#pragma unroll
        for (int k = 1; k < MD; ++k) if (k < dim) ls[k] += sl[k] * a[0] + sb1 * a[k];
#pragma unroll
        for (int k = 0; k < MD; ++k) if (k < dim) {
            lam[d.oz() + st + k] = bz[k];
            lam[d.os() + st + k] = ls[k];
            lam[d.ot() + st + k] = lt[k] + a[k];
        }
    }
}

void launch_recover_t_multi(calipso_hip_solver* s, const double* V, int p, double* lam, double* g, double* xbuf) {
    const Dims& d = s->d;
    const int work = d.NP + d.ne + d.q + d.n_soc;
    const BatchSc B = batch_of(s);
    hipLaunchKernelGGL(k_recover_t, dim3((work + ADJ_THREADS - 1) / ADJ_THREADS, p, B.b.n), dim3(ADJ_THREADS), 0, s->stream, B, d, s->cone, s->solution, V, s->wz, s->Wsoc,
                       lam, g, xbuf);
    launch_recover_t_wide(s, V, p, lam, g);
}
void launch_residual_symmetric_t_multi(calipso_hip_solver* s, int p, const double* g, const double* xbuf, const double* t1, double* lam) {
    const Dims& d = s->d;
    const int work = d.nx + d.ne + d.q + d.n_soc;
    const BatchSc B = batch_of(s);
    hipLaunchKernelGGL(k_residual_symmetric_t, dim3((work + ADJ_THREADS - 1) / ADJ_THREADS, p, B.b.n), dim3(ADJ_THREADS), 0, s->stream, B, d, s->cone, s->solution, g, xbuf,
                       t1, s->wz, s->Wsoc, lam);
    launch_residual_symmetric_t_wide(s, p, g, t1, lam);
}

// ---- gradients with respect to the data of an attached QP -----------------------------------------------------------------------------------------------------
// R_x = 2c P x + q + A'y - G'z, R_y = A x - b - r, R_z = h - G x - s (qp.hip), so for a loss with dLoss/dw = v and lam = M' v the gradient with respect to a datum D is
// -(dR/dD)' lam (the closed forms and signs of k_smallnewton_adj's grad_qp block).  The matrices are write-bound (nx^2 doubles per column for P): one pass, every
// element written once, consecutive rows of a matrix column by consecutive lanes.
//   out[row + col * rows] = alpha * (lrow[row] * x[col] + prow[row] * lam_x[col])        P: (lam_x, x, -c); A: (lam_y, y, -1); G: (lam_z, z, +1)
// a b + c d with both products rounded on their own (no fused multiply-add): symmetric in (a, b, c, d) -> (d, c, b, a) to the bit
__device__ __forceinline__ double two_products(double a, double b, double c, double d) {
#pragma clang fp contract(off)
    const double p = a * b, q = c * d;
    return p + q;
}
// grid: x = row blocks x column lanes (a lane of the matrix's columns strides over them), y = the cotangent column, z = the instance
__global__ __launch_bounds__(256) void k_qp_grad_matrix(Batch bt, int rows, int cols, int N, int row_blocks, const double* __restrict__ lam_, int lrow_off, const double* __restrict__ w,
                                                         int prow_off, double alpha, double* __restrict__ out_, size_t size) {
    inst_shift(bt, w);
    const size_t col = column_shift(bt, gridDim.y) + blockIdx.y;
    const double* lam = lam_ + col * N;
    double* out = out_ + col * size;
    const int rb = blockIdx.x % row_blocks, c0 = blockIdx.x / row_blocks, cstep = gridDim.x / row_blocks;
    const int r = rb * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const double lr = lam[lrow_off + r], pr = w[prow_off + r];
    // (the two products rounded on their own, two_products: entry (r, c) of the gradient of P is then entry (c, r) to the bit)
    for (int c = c0; c < cols; c += cstep) out[(size_t)r + (size_t)c * rows] = alpha * two_products(lr, w[c], pr, lam[c]);
}
// q: -lam_x; b: lam_y; h: -lam_z
__global__ __launch_bounds__(256) void k_qp_grad_vector(Batch bt, int rows, int N, const double* __restrict__ lam_, int off, double alpha, double* __restrict__ out_) {
    const size_t col = column_shift(bt, gridDim.y) + blockIdx.y;
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < rows) out_[col * rows + r] = alpha * lam_[col * N + off + r];
}

void launch_qp_data_gradients(calipso_hip_solver* s, const double* lam, int p, double* const out[6], double scale) {
    const Dims& d = s->d;
    const double* w = s->solution;
    const Batch B = batch_of(s).b;
    auto mat = [&](double* o, int rows, int loff, int poff, double alpha) {
        const int rb = (rows + 255) / 256, lanes = d.nx < 65535 ? d.nx : 65535;
        if (o && rows > 0) hipLaunchKernelGGL(k_qp_grad_matrix, dim3(rb * lanes, p, B.n), dim3(256), 0, s->stream, B, rows, d.nx, d.N, rb, lam, loff, w, poff, alpha, o, (size_t)rows * d.nx);
    };
    auto vec = [&](double* o, int rows, int off, double alpha) {
        if (o && rows > 0) hipLaunchKernelGGL(k_qp_grad_vector, dim3((rows + 255) / 256, p, B.n), dim3(256), 0, s->stream, B, rows, d.N, lam, off, alpha, o);
    };
    mat(out[0], d.nx, 0, 0, -scale);
    vec(out[1], d.nx, 0, -1.0);
    mat(out[2], d.ne, d.oy(), d.oy(), -1.0);
    vec(out[3], d.ne, d.oy(), 1.0);
    mat(out[4], d.nc, d.oz(), d.oz(), 1.0);
    vec(out[5], d.nc, d.oz(), -1.0);
}

}  // namespace calipso
