// friction_cone.hip — test fixture: a second-order-cone problem parametrised by theta = [v (3); mu; gamma] (its Python twin: tests/test_gpu_smallnewton_evaluator.py:
// friction_cone):  min 1/2 |x - v|^2 + gamma/4 x0^4   s.t.  [mu (x0 + 1); x1; x2] in the second-order cone of dimension 3.
// nx = 3, ne = 0, nc = 3 (one cone), np = 5.  Thread 0 of the instance writes every derivative.
#include "calipso_smallnewton.hpp"

namespace {

struct FrictionCone {
    static constexpr bool constant_derivatives = false;
    static constexpr bool provides_jacobian_parameters = true;
    template <class C> __device__ static double objective(C& c, const double* x) {
        const double* th = c.theta;
        const double a = x[0] - th[0], b = x[1] - th[1], e = x[2] - th[2];
        return 0.5 * (a * a + b * b + e * e) + 0.25 * th[4] * (x[0] * x[0] * x[0] * x[0]);
    }
    template <class C> __device__ static void constraints(C& c, const double* x, double* out) {
        if (c.tid != 0) return;
        out[0] = c.theta[3] * (x[0] + 1.0); out[1] = x[1]; out[2] = x[2];
    }
    template <class C> __device__ static void derivatives(C& c, const double* w) {
        if (c.tid != 0) return;
        const auto& d = c.d;
        const double* th = c.theta;
        const double x0 = w[0];
        c.fx[0] = (x0 - th[0]) + th[4] * (x0 * x0 * x0); c.fx[1] = w[1] - th[1]; c.fx[2] = w[2] - th[2];
        double* Z = c.Z; const int ld = d.ldz;
        for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) Z[r + k * ld] = 0.0;
        Z[0] = th[3]; Z[1 + ld] = 1.0; Z[2 + 2 * ld] = 1.0;
        double* Hh = c.Hw;                                                             // h is linear in x
        for (int e = 0; e < 9; ++e) Hh[e] = 0.0;
        Hh[0] = 1.0 + 3.0 * th[4] * (x0 * x0); Hh[4] = 1.0; Hh[8] = 1.0;
    }
    template <class C> __device__ static void jacobian_parameters(C& c, const double* w, double* J) {
        if (c.tid != 0) return;
        const auto& d = c.d;
        const int N = d.N;
        const double x0 = w[0], z0 = w[d.oz()];
        for (int i = 0; i < 3; ++i) J[i + i * N] = -1.0;                             // fx by v
        J[0 + 3 * N] = z0;                                                            // (z'h)x by mu
        J[0 + 4 * N] = x0 * x0 * x0;                                                  // fx by gamma
        J[d.oz() + 3 * N] = x0 + 1.0;                                                 // h by mu
    }
};

}  // namespace

CALIPSO_SMALLNEWTON_EVALUATOR(FrictionCone, friction_cone_kernels)
