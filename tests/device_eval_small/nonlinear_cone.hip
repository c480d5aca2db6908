// nonlinear_cone.hip — test fixture: a nonconvex problem with nonlinear f and h over nonnegative cones, parametrised by theta (its Python twin:
// tests/test_gpu_smallnewton_evaluator.py: nonlinear_cone):
//   min (1 - x0)^2 + 10 (x1 - x0^2)^2 + 1/2 x2^2   s.t.  x0 + x1 + x2 - theta0 = 0,  [theta1 - x0^2 - x1^2; x2 + theta2 - x0 x1] >= 0
// nx = 3, ne = 1, nc = 2, np = 3.  Tiny: thread 0 of the instance writes every derivative (closed forms).
#include "calipso_smallnewton.hpp"

namespace {

struct NonlinearCone {
    static constexpr bool constant_derivatives = false;
    static constexpr bool provides_jacobian_parameters = true;
    template <class C> __device__ static double objective(C& c, const double* x) {
        const double a = 1.0 - x[0], b = x[1] - x[0] * x[0];
        return a * a + 10.0 * (b * b) + 0.5 * (x[2] * x[2]);
    }
    template <class C> __device__ static void constraints(C& c, const double* x, double* out) {
        if (c.tid != 0) return;
        const double* th = c.theta;
        out[0] = x[0] + x[1] + x[2] - th[0];
        out[1] = th[1] - x[0] * x[0] - x[1] * x[1];
        out[2] = x[2] + th[2] - x[0] * x[1];
    }
    template <class C> __device__ static void derivatives(C& c, const double* w) {
        if (c.tid != 0) return;
        const auto& d = c.d;
        const double x0 = w[0], x1 = w[1], x2 = w[2];
        const double z0 = w[d.oz()], z1 = w[d.oz() + 1];
        const double b = x1 - x0 * x0;
        c.fx[0] = -2.0 * (1.0 - x0) - 40.0 * x0 * b; c.fx[1] = 20.0 * b; c.fx[2] = x2;
        double* Z = c.Z; const int ld = d.ldz;
        Z[0] = 1.0; Z[ld] = 1.0; Z[2 * ld] = 1.0;                                      // gx
        Z[1] = -2.0 * x0; Z[1 + ld] = -2.0 * x1; Z[1 + 2 * ld] = 0.0;                  // hx
        Z[2] = -x1; Z[2 + ld] = -x0; Z[2 + 2 * ld] = 1.0;
        double* Hh = c.Hw;                                                             // fxx + (z'h)xx  (g is linear)
        Hh[0] = 2.0 - 40.0 * b + 80.0 * x0 * x0 - 2.0 * z0; Hh[1] = -40.0 * x0 - z1; Hh[2] = 0.0;
        Hh[3] = -40.0 * x0 - z1; Hh[4] = 20.0 - 2.0 * z0; Hh[5] = 0.0;
        Hh[6] = 0.0; Hh[7] = 0.0; Hh[8] = 1.0;
    }
    template <class C> __device__ static void jacobian_parameters(C& c, const double* w, double* J) {      // theta enters g and h additively
        if (c.tid != 0) return;
        const auto& d = c.d;
        J[d.oy() + 0 * d.N] = -1.0;
        J[d.oz() + 1 * d.N] = 1.0;
        J[d.oz() + 1 + 2 * d.N] = 1.0;
    }
};

}  // namespace

CALIPSO_SMALLNEWTON_EVALUATOR(NonlinearCone, nonlinear_cone_kernels)

// an entry that answers the handshake with another ABI version: what a library built against a different calipso_smallnewton.hpp looks like
extern "C" __attribute__((visibility("default"))) int32_t mismatched_abi_kernels(const calipso_smallnewton_launch* L) {
    if (L && L->op == CALIPSO_SMALLNEWTON_QUERY && L->out) {
        L->out[0] = CALIPSO_SMALLNEWTON_ABI + 1; L->out[1] = (int64_t)sizeof(calipso::sn::Args); L->out[2] = SN_JB; L->out[3] = 0;
        return CALIPSO_OK;
    }
    return CALIPSO_ERR_ARGUMENT;
}
