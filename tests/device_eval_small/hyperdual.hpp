// hyperdual.hpp — hyper-dual numbers a + b e1 + c e2 + d e1e2 (e1^2 = e2^2 = 0): one evaluation of a function with e1 along input i and e2 along input j gives the
// value, the first derivatives along i and j and the second derivative d2/didj, exactly up to rounding.  The fixture evaluators take their Jacobians and
// Lagrangian Hessians from it.
#pragma once
#include <hip/hip_runtime.h>

struct HD {
    double a, b, c, d;
};
__device__ __forceinline__ HD hd(double a) { return {a, 0.0, 0.0, 0.0}; }
__device__ __forceinline__ HD operator+(HD x, HD y) { return {x.a + y.a, x.b + y.b, x.c + y.c, x.d + y.d}; }
__device__ __forceinline__ HD operator-(HD x, HD y) { return {x.a - y.a, x.b - y.b, x.c - y.c, x.d - y.d}; }
__device__ __forceinline__ HD operator-(HD x) { return {-x.a, -x.b, -x.c, -x.d}; }
__device__ __forceinline__ HD operator*(HD x, HD y) { return {x.a * y.a, x.a * y.b + x.b * y.a, x.a * y.c + x.c * y.a, x.a * y.d + x.b * y.c + x.c * y.b + x.d * y.a}; }
__device__ __forceinline__ HD operator*(double s, HD x) { return {s * x.a, s * x.b, s * x.c, s * x.d}; }
__device__ __forceinline__ HD operator+(double s, HD x) { return {s + x.a, x.b, x.c, x.d}; }
__device__ __forceinline__ HD operator-(double s, HD x) { return {s - x.a, -x.b, -x.c, -x.d}; }
__device__ __forceinline__ HD operator-(HD x, double s) { return {x.a - s, x.b, x.c, x.d}; }
// f(x) from f(a), f'(a), f''(a)
__device__ __forceinline__ HD chain(HD x, double f0, double f1, double f2) { return {f0, f1 * x.b, f1 * x.c, f1 * x.d + f2 * x.b * x.c}; }
__device__ __forceinline__ HD operator/(HD x, HD y) { const double r = 1.0 / y.a; return x * chain(y, r, -r * r, 2.0 * r * r * r); }
__device__ __forceinline__ HD sin(HD x) { const double s = ::sin(x.a), c = ::cos(x.a); return chain(x, s, c, -s); }
__device__ __forceinline__ HD cos(HD x) { const double s = ::sin(x.a), c = ::cos(x.a); return chain(x, c, -s, -c); }
__device__ __forceinline__ HD exp(HD x) { const double e = ::exp(x.a); return chain(x, e, e, e); }
// the inputs of a two-direction evaluation: v with e1 on entry i and e2 on entry j (i == j: the second derivative along one input)
template <int K> __device__ __forceinline__ void seed(const double* v, int i, int j, HD (&out)[K]) {
    for (int k = 0; k < K; ++k) out[k] = {v[k], k == i ? 1.0 : 0.0, k == j ? 1.0 : 0.0, 0.0};
}
