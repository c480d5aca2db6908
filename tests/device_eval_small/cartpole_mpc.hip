// cartpole_mpc.hip — test fixture: the cart-pole MPC problem of tests/problems.py: cartpole_mpc (examples/autotuning/cartpole.jl:85-146, BASELINE config C5) as a
// device evaluator of the batched small-problem kernel.  nx = 49 (10 stages of 4 states, 9 actions: z = [x1; u1; x2; u2; ...; x10]), ne = 40 (36 explicit-midpoint
// dynamics rows x_{t+1} - f(x_t, u_t), then x_1 - x_init), nc = 0, np = 102 parameters theta_t = [xbar(4); ubar; w_Q(4); w_R; x_init(4) if t = 1] for t < 10 and
// theta_10 = [xbar(4); w_Q(4)].  Jacobian and Hessian of the dynamics by hyper-dual numbers; dR/dtheta in closed form.
#include "calipso_smallnewton.hpp"
#include "hyperdual.hpp"

namespace {

constexpr int T = 10, NS = 4, NA = 1, NZ = NS * T + NA * (T - 1), NDYN = NS * (T - 1);
constexpr double MC = 1.0, MP = 0.2, LEN = 0.5, GRAV = 9.81, H = 0.05;

__device__ __forceinline__ int stage_offset(int t) { return t == 0 ? 0 : 14 + 10 * (t - 1); }      // first parameter of stage t

// models/cartpole.jl:2-33: the continuous dynamics, then one explicit-midpoint step
template <class S> __device__ __forceinline__ void fcont(const S (&x)[4], const S& u, S (&out)[4]) {
    const S s = sin(x[1]), c = cos(x[1]);
    constexpr double h11 = MC + MP, h22 = MP * LEN * LEN;
    const S h12 = (MP * LEN) * c;
    const S det = h11 * h22 - h12 * h12;
    const S r0 = (-MP * LEN) * (x[3] * s * x[3]) - u;
    const S r1 = (MP * GRAV * LEN) * s;
    out[0] = x[2]; out[1] = x[3];
    out[2] = -((h22 * r0 - h12 * r1) / det);
    out[3] = -((-1.0 * (h12 * r0) + h11 * r1) / det);
}
template <class S> __device__ __forceinline__ void fdisc(const S (&x)[4], const S& u, S (&out)[4]) {
    S k1[4], xm[4], k2[4];
    fcont(x, u, k1);
    for (int i = 0; i < 4; ++i) xm[i] = x[i] + (0.5 * H) * k1[i];
    fcont(xm, u, k2);
    for (int i = 0; i < 4; ++i) out[i] = x[i] + H * k2[i];
}

struct CartpoleMPC {
    static constexpr bool constant_derivatives = false;
    static constexpr bool provides_jacobian_parameters = true;

    // weight of variable i (its stage's w_Q or w_R) and its tracking target
    __device__ __forceinline__ static void weight(const double* th, int i, double& w, double& ref) {
        const int t = i / 5, j = i % 5;
        if (t < T - 1) { const double* p = th + stage_offset(t); w = j < 4 ? p[5 + j] : p[9]; ref = j < 4 ? p[j] : p[4]; }
        else { const double* p = th + stage_offset(T - 1); w = p[4 + j]; ref = p[j]; }
    }
    template <class C> __device__ static double objective(C& c, const double* x) {
        double v[1] = {0.0};
        for (int i = c.tid; i < NZ; i += C::threads) { double w, r; weight(c.theta, i, w, r); v[0] += 0.5 * w * w * (x[i] - r) * (x[i] - r); }
        c.sum(v);
        return v[0];
    }
    template <class C> __device__ static void constraints(C& c, const double* x, double* out) {
        for (int r = c.tid; r < NDYN + NS; r += C::threads) {
            if (r < NDYN) {
                const int t = r / 4, i = r % 4;
                const double xs[4] = {x[5 * t], x[5 * t + 1], x[5 * t + 2], x[5 * t + 3]};
                double f[4];
                fdisc(xs, x[5 * t + 4], f);
                out[r] = x[5 * (t + 1) + i] - f[i];
            } else out[r] = x[r - NDYN] - c.theta[10 + r - NDYN];
        }
    }
    // (y'g)xx on the (x_t, u_t) block of stage t, entry (a, b): -sum_i y_i d2 f_i / da db
    __device__ static double dyn_hessian(const double* x, const double* y, int t, int a, int b) {
        const double v[5] = {x[5 * t], x[5 * t + 1], x[5 * t + 2], x[5 * t + 3], x[5 * t + 4]};
        HD in[5];
        seed(v, a < b ? a : b, a < b ? b : a, in);
        const HD xs[4] = {in[0], in[1], in[2], in[3]};
        HD f[4];
        fdisc(xs, in[4], f);
        double s = 0.0;
        for (int i = 0; i < 4; ++i) s += -(y[4 * t + i] * f[i].d);
        return s;
    }
    template <class C> __device__ static void derivatives(C& c, const double* w) {
        const auto& d = c.d;
        const double* y = w + d.oy();
        for (int i = c.tid; i < NZ; i += C::threads) { double wt, r; weight(c.theta, i, wt, r); c.fx[i] = wt * wt * (w[i] - r); }
        for (int e = c.tid; e < d.m * NZ; e += C::threads) {      // [gx; hx] = gx: a column of Z per thread group
            const int r = e % d.m, col = e / d.m;
            double v = 0.0;
            if (r < NDYN) {
                const int t = r / 4, i = r % 4;
                if (col == 5 * (t + 1) + i) v = 1.0;
                else if (col >= 5 * t && col < 5 * t + 5) {
                    const double xv[5] = {w[5 * t], w[5 * t + 1], w[5 * t + 2], w[5 * t + 3], w[5 * t + 4]};
                    HD in[5];
                    seed(xv, col - 5 * t, -1, in);
                    const HD xs[4] = {in[0], in[1], in[2], in[3]};
                    HD f[4];
                    fdisc(xs, in[4], f);
                    v = -f[i].b;
                }
            } else if (col == r - NDYN) v = 1.0;
            c.Z[r + col * d.ldz] = v;
        }
        for (int e = c.tid; e < NZ * NZ; e += C::threads) {       // the Lagrangian Hessian: the objective's diagonal + the dynamics' stage blocks
            const int r = e % NZ, col = e / NZ;
            double v = 0.0;
            if (r == col) { double wt, ref; weight(c.theta, r, wt, ref); v = wt * wt; }
            if (r / 5 == col / 5 && r < 5 * (T - 1)) v += dyn_hessian(w, y, r / 5, r % 5, col % 5);
            c.Hw[e] = v;
        }
    }
    // residual_jacobian_parameters.jl:1-40: x rows = fxθ (the dynamics do not depend on theta), the y rows of x_1 - x_init = -I on the x_init columns
    template <class C> __device__ static void jacobian_parameters(C& c, const double* w, double* J) {
        const auto& d = c.d;
        const int N = d.N;
        for (int i = c.tid; i < NZ; i += C::threads) {
            const int t = i / 5, j = i % 5;
            const int off = stage_offset(t);
            const int cref = t < T - 1 ? off + (j < 4 ? j : 4) : off + j;
            const int cw = t < T - 1 ? off + (j < 4 ? 5 + j : 9) : off + 4 + j;
            double wt, ref; weight(c.theta, i, wt, ref);
            J[i + (size_t)cref * N] = -(wt * wt);
            J[i + (size_t)cw * N] = 2.0 * wt * (w[i] - ref);
        }
        for (int i = c.tid; i < NS; i += C::threads) J[d.oy() + NDYN + i + (size_t)(10 + i) * N] = -1.0;
    }
};

}  // namespace

CALIPSO_SMALLNEWTON_EVALUATOR(CartpoleMPC, cartpole_mpc_kernels)
