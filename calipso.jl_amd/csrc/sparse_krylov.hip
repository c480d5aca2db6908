// sparse_krylov.hip — the vector kernels of the `H \ residual` fallback of the sparse handle (search_direction.jl:22): restarted right-preconditioned GMRES on the
// unreduced H, driven by search_direction() of sparse_kkt.hip through the host logic of sparse_krylov.hpp.  One iteration is one condensed solve (z = M v), one H z
// (both of sparse_kkt.hip) and, here, classical Gram-Schmidt applied twice:
//   k_gmres_dots     V[:, 0..j]' w for up to RESTART_MAX vectors in ONE pass over w: a thread takes rows in stride order with one accumulator per vector in registers
//   k_gmres_update   w <- w - V h (h from the partials of the dots, summed in workgroup order by every workgroup); the second pass accumulates |w|^2
//   k_gmres_finish   one workgroup: |w|_2 from its partials into the coefficient block      k_gmres_scale   v <- w / |w|_2
//   k_gmres_combine  x <- x + Z y at the end of a cycle, y passed by value: no further solve
// Each pass is two launches whatever j is.  Every sum is two-stage in a fixed order (a thread its rows in stride order, a workgroup its threads by a butterfly, one
// partial per (quantity, workgroup), the partials added in workgroup order): no floating-point atomics, a call repeats bit for bit.  Bound by bandwidth and launches.
#include "sparse_kkt_handle.hpp"

using namespace calipso::sparse_kkt;
using namespace calipso::sparse_krylov;
static_assert(KT == THREADS, "the workspace layout counts workgroups of KT threads");

namespace {

struct Coefficients { double v[RESTART_MAX]; };

// the workgroup's sums of quantities q < nq: one double per (quantity, workgroup) at part[q * grid + workgroup]
template <int NQ>
__device__ __forceinline__ void store_partials(double (&val)[NQ], int nq, double* __restrict__ part) {
    __shared__ double lds[NQ][KT / 64];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        double a = val[q];
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        if ((threadIdx.x & 63) == 0) lds[q][threadIdx.x >> 6] = a;
    }
    __syncthreads();
    if (threadIdx.x < NQ && (int)threadIdx.x < nq) {
        const int q = threadIdx.x;
        double a = lds[q][0];
        for (int k = 1; k < KT / 64; ++k) a += lds[q][k];
        part[(long long)q * gridDim.x + blockIdx.x] = a;
    }
}
// the partials of quantity q added in workgroup order
__device__ __forceinline__ double combine_partials(const double* __restrict__ part, int q, int grid) {
    double a = part[(long long)q * grid];
    for (int b = 1; b < grid; ++b) a += part[(long long)q * grid + b];
    return a;
}

template <int NV>
__global__ __launch_bounds__(KT) void k_gmres_dots(int N, int nv, const double* __restrict__ V, const double* __restrict__ w, double* __restrict__ part) {
    double acc[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) acc[q] = 0.0;
    for (long long k = (long long)blockIdx.x * KT + threadIdx.x; k < N; k += (long long)gridDim.x * KT) {
        const double wk = w[k];
#pragma unroll
        for (int q = 0; q < NV; ++q) if (q < nv) acc[q] += V[(long long)q * N + k] * wk;
    }
    store_partials<NV>(acc, nv, part);
}

// dst <- src - V[:, 0..nv) h with h[q] = the dots' partials of q in workgroup order (the dots ran on this grid); workgroup 0 keeps h in coef (the first pass) or
// adds it there (the second); norm_part: also this workgroup's share of |dst|^2.  src and dst may be the same vector
template <int NV>
__global__ __launch_bounds__(KT) void k_gmres_update(int N, int nv, const double* __restrict__ V, const double* src, double* dst, const double* __restrict__ part,
                                                     double* __restrict__ coef, int accumulate, double* __restrict__ norm_part) {
    __shared__ double h[NV];
    if ((int)threadIdx.x < nv) {
        const double a = combine_partials(part, threadIdx.x, gridDim.x);
        h[threadIdx.x] = a;
        if (blockIdx.x == 0) coef[threadIdx.x] = accumulate ? coef[threadIdx.x] + a : a;
    }
    __syncthreads();
    double nrm[1] = {0.0};
    for (long long k = (long long)blockIdx.x * KT + threadIdx.x; k < N; k += (long long)gridDim.x * KT) {
        double a = src[k];
#pragma unroll
        for (int q = 0; q < NV; ++q) if (q < nv) a -= V[(long long)q * N + k] * h[q];
        dst[k] = a;
        nrm[0] += a * a;
    }
    if (norm_part) store_partials<1>(nrm, 1, norm_part);      // (uniform)
}

// |w|_2 into coef[slot]
__global__ __launch_bounds__(64) void k_gmres_finish(int grid, const double* __restrict__ norm_part, double* __restrict__ coef, int slot) {
    if (threadIdx.x == 0) coef[slot] = sqrt(combine_partials(norm_part, 0, grid));
}

// v <- v / coef[slot]; a zero (or NaN) norm leaves zeros: the host reads the same norm and ends the cycle
__global__ __launch_bounds__(KT) void k_gmres_scale(int N, double* __restrict__ v, const double* __restrict__ coef, int slot) {
    const double nrm = coef[slot];
    for (long long k = (long long)blockIdx.x * KT + threadIdx.x; k < N; k += (long long)gridDim.x * KT) v[k] = nrm > 0.0 ? v[k] / nrm : 0.0;
}

template <int NV>
__global__ __launch_bounds__(KT) void k_gmres_combine(int N, int nv, const double* __restrict__ Z, double* __restrict__ x, const Coefficients y) {
    for (long long k = (long long)blockIdx.x * KT + threadIdx.x; k < N; k += (long long)gridDim.x * KT) {
        double a = x[k];
#pragma unroll
        for (int q = 0; q < NV; ++q) if (q < nv) a += Z[(long long)q * N + k] * y.v[q];
        x[k] = a;
    }
}

// the smallest compiled bound that holds nv vectors
#define BY_BOUND(nv, CALL) do { if ((nv) <= 4) { CALL(4); } else if ((nv) <= 8) { CALL(8); } else if ((nv) <= 16) { CALL(16); } else { CALL(32); } } while (0)

}  // namespace

namespace calipso {
namespace sparse_kkt {

static_assert(RESTART_MAX == 32, "BY_BOUND's largest instance");

void krylov_enqueue_dots(hipStream_t st, const Layout& l, double* ws, int nv, const double* w) {
#define CALL(B) hipLaunchKernelGGL(k_gmres_dots<B>, dim3((unsigned)l.grid), dim3(KT), 0, st, (int)l.N, nv, ws + l.off_V, w, ws + l.off_dots)
    BY_BOUND(nv, CALL);
#undef CALL
}
void krylov_enqueue_update(hipStream_t st, const Layout& l, double* ws, int nv, const double* src, double* dst, bool accumulate, bool norm) {
#define CALL(B) hipLaunchKernelGGL(k_gmres_update<B>, dim3((unsigned)l.grid), dim3(KT), 0, st, (int)l.N, nv, ws + l.off_V, src, dst, ws + l.off_dots, ws + l.off_coef, \
                                   accumulate ? 1 : 0, norm ? ws + l.off_norm : (double*)nullptr)
    BY_BOUND(nv, CALL);
#undef CALL
}
void krylov_enqueue_norm_scale(hipStream_t st, const Layout& l, double* ws, int slot, double* v) {
    hipLaunchKernelGGL(k_gmres_finish, dim3(1), dim3(64), 0, st, (int)l.grid, ws + l.off_norm, ws + l.off_coef, slot);
    hipLaunchKernelGGL(k_gmres_scale, dim3((unsigned)l.grid), dim3(KT), 0, st, (int)l.N, v, ws + l.off_coef, slot);
}
void krylov_enqueue_combine(hipStream_t st, const Layout& l, double* ws, int nv, const double* y, double* x) {
    Coefficients c;
    for (int q = 0; q < RESTART_MAX; ++q) c.v[q] = q < nv ? y[q] : 0.0;
#define CALL(B) hipLaunchKernelGGL(k_gmres_combine<B>, dim3((unsigned)l.grid), dim3(KT), 0, st, (int)l.N, nv, ws + l.off_Z, x, c)
    BY_BOUND(nv, CALL);
#undef CALL
}

}  // namespace sparse_kkt
}  // namespace calipso
