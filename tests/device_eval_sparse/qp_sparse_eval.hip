// test fixture and example: a hand-written calipso_device_sparse_eval_fn — the sparse conic QP of calipso_hip_sparse_kkt_qp_attach,
//     f = 1/2 x'Lxx x + q'x + constant,  g = gx x - b,  h = hx x + hvec,
// as a user of calipso_hip_sparse_kkt_set_evaluator would write it.  The user object holds the problem on the device: CSR copies of the three matrices for the
// products (one thread per row, a fixed order per row), their non-zeros in the handle's own (CSC) order for the three nzval arrays, q, b, hvec.  Everything is
// enqueued on the stream the handle passes; nothing waits.  Sums are in a fixed order, so a solve through it repeats bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/calipso_hip.h"

namespace {

struct Csr { int rows = 0; int *ptr = nullptr, *col = nullptr; double* val = nullptr; };      // device arrays
struct Dev {                                                     // what the kernels read, by value
    int nx = 0, ne = 0, nc = 0;
    Csr L, g, h;
    double *q = nullptr, *b = nullptr, *hvec = nullptr, *fpart = nullptr;
};
struct User : Dev {
    double *Lnz = nullptr, *gnz = nullptr, *hnz = nullptr;      // the non-zeros in the handle's order
    long long nnz[3] = {0, 0, 0};
    double constant = 0.0;
    int fail_with = 0;                                          // tests: the next calls return this instead of evaluating
    std::vector<void*> owned;
};

__device__ double row_dot(const Csr m, int r, const double* __restrict__ x) {
    double a = 0.0;
    for (int p = m.ptr[r]; p < m.ptr[r + 1]; ++p) a += m.val[p] * x[m.col[p]];
    return a;
}
// one thread per row of [x; equality; cone]
__global__ __launch_bounds__(256) void k_rows(Dev u, uint32_t flags, const double* __restrict__ x, calipso_device_sparse_data out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < u.nx) {
        if (!(flags & (CALIPSO_EVAL_OBJECTIVE | CALIPSO_EVAL_OBJECTIVE_GRADIENT))) return;
        const double Lx = row_dot(u.L, k, x);
        if (flags & CALIPSO_EVAL_OBJECTIVE_GRADIENT) out.objective_gradient_variables[k] = Lx + u.q[k];
        if (flags & CALIPSO_EVAL_OBJECTIVE) u.fpart[k] = 0.5 * x[k] * Lx + u.q[k] * x[k];
    } else if (k < u.nx + u.ne) {
        const int i = k - u.nx;
        if (flags & CALIPSO_EVAL_EQUALITY) out.equality_constraint[i] = row_dot(u.g, i, x) - u.b[i];
    } else if (k < u.nx + u.ne + u.nc) {
        const int c = k - u.nx - u.ne;
        if (flags & CALIPSO_EVAL_CONE) out.cone_constraint[c] = row_dot(u.h, c, x) + u.hvec[c];
    }
}
// the objective: one workgroup, thread t adds the terms t, t + 256, ..., then a fixed tree
__global__ __launch_bounds__(256) void k_objective(int nx, const double* __restrict__ fpart, double constant, double* __restrict__ f) {
    __shared__ double tree[256];
    double a = 0.0;
    for (int k = threadIdx.x; k < nx; k += 256) a += fpart[k];
    tree[threadIdx.x] = a;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) tree[threadIdx.x] += tree[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) f[0] = tree[0] + constant;
}

template <typename T> T* to_device(User* u, const T* host, size_t count) {
    T* p = nullptr;
    if (hipMalloc((void**)&p, sizeof(T) * (count ? count : 1)) != hipSuccess) return nullptr;
    u->owned.push_back(p);
    if (count && hipMemcpy(p, host, sizeof(T) * count, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return p;
}

}  // namespace

extern "C" {

// sizes = nx, ne, nc; per matrix (Lxx, gx, hx): CSR row pointers, columns and values (0-based), and the non-zeros in the order of the pattern given to the handle
__attribute__((visibility("default"))) void* qp_sparse_create(const int32_t* sizes, const int32_t* const* ptr, const int32_t* const* col, const double* const* val,
                                                              const double* const* nz, const double* q, const double* b, const double* hvec, double constant) {
    User* u = new User();
    u->nx = sizes[0]; u->ne = sizes[1]; u->nc = sizes[2]; u->constant = constant;
    Csr* m[3] = {&u->L, &u->g, &u->h};
    double** nzd[3] = {&u->Lnz, &u->gnz, &u->hnz};
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        m[k]->rows = sizes[k];
        const size_t count = (size_t)ptr[k][sizes[k]];
        u->nnz[k] = (long long)count;
        ok = ok && (m[k]->ptr = to_device(u, ptr[k], (size_t)sizes[k] + 1)) && (m[k]->col = to_device(u, col[k], count)) && (m[k]->val = to_device(u, val[k], count)) &&
             (*nzd[k] = to_device(u, nz[k], count));
    }
    ok = ok && (u->q = to_device(u, q, (size_t)u->nx)) && (u->b = to_device(u, b, (size_t)u->ne)) && (u->hvec = to_device(u, hvec, (size_t)u->nc));
    if (ok && (ok = hipMalloc((void**)&u->fpart, sizeof(double) * (size_t)(u->nx ? u->nx : 1)) == hipSuccess)) u->owned.push_back(u->fpart);
    if (!ok) { for (void* p : u->owned) (void)hipFree(p); delete u; return nullptr; }
    return u;
}
__attribute__((visibility("default"))) void qp_sparse_destroy(void* user) {
    User* u = (User*)user;
    if (!u) return;
    for (void* p : u->owned) (void)hipFree(p);
    delete u;
}
__attribute__((visibility("default"))) void qp_sparse_fail_with(void* user, int32_t code) { ((User*)user)->fail_with = code; }

__attribute__((visibility("default"))) int32_t qp_sparse_eval(void* user, uint32_t flags, const double* x, const double* y, const double* z, const double* theta,
                                                              const calipso_device_sparse_data* out, void* hip_stream) {
    User* u = (User*)user;
    (void)y; (void)z; (void)theta;                            // a QP: the dual Hessians are zero, and it has no parameters
    if (!u || !out || out->nx != u->nx || out->ne != u->ne || out->nc != u->nc || out->nnz_Lxx != u->nnz[0] || out->nnz_gx != u->nnz[1] || out->nnz_hx != u->nnz[2]) return 1;
    if (u->fail_with) return u->fail_with;
    hipStream_t stream = (hipStream_t)hip_stream;
    const int rows = u->nx + u->ne + u->nc;
    if (rows && (flags & (CALIPSO_EVAL_OBJECTIVE | CALIPSO_EVAL_OBJECTIVE_GRADIENT | CALIPSO_EVAL_EQUALITY | CALIPSO_EVAL_CONE)))
        hipLaunchKernelGGL(k_rows, dim3((rows + 255) / 256), dim3(256), 0, stream, (Dev)*u, flags, x, *out);
    if (flags & CALIPSO_EVAL_OBJECTIVE) hipLaunchKernelGGL(k_objective, dim3(1), dim3(256), 0, stream, u->nx, u->fpart, u->constant, out->objective);
    // the matrices are constant: the non-zeros as they were given, into the handle's arrays (the dual Hessians add nothing)
    const size_t D = sizeof(double);
    if ((flags & CALIPSO_EVAL_OBJECTIVE_HESSIAN) && u->nnz[0] && hipMemcpyAsync(out->lagrangian_hessian, u->Lnz, D * (size_t)u->nnz[0], hipMemcpyDeviceToDevice, stream) != hipSuccess) return 2;
    if (!(flags & CALIPSO_EVAL_OBJECTIVE_HESSIAN) && (flags & (CALIPSO_EVAL_EQUALITY_DUAL_HESSIAN | CALIPSO_EVAL_CONE_DUAL_HESSIAN)) && u->nnz[0] &&
        hipMemsetAsync(out->lagrangian_hessian, 0, D * (size_t)u->nnz[0], stream) != hipSuccess) return 2;
    if ((flags & CALIPSO_EVAL_EQUALITY_JACOBIAN) && u->nnz[1] && hipMemcpyAsync(out->equality_jacobian_variables, u->gnz, D * (size_t)u->nnz[1], hipMemcpyDeviceToDevice, stream) != hipSuccess) return 2;
    if ((flags & CALIPSO_EVAL_CONE_JACOBIAN) && u->nnz[2] && hipMemcpyAsync(out->cone_jacobian_variables, u->hnz, D * (size_t)u->nnz[2], hipMemcpyDeviceToDevice, stream) != hipSuccess) return 2;
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
