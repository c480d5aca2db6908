// test fixture and example: a hand-written calipso_device_sparse_eval_fn WITH PARAMETERS — the sparse conic QP whose vectors are affine in theta,
//     f = 1/2 x'Lxx x + q(theta)'x,  g = gx x - b(theta),  h = hx x + hvec(theta),    q = q0 + Qt theta,  b = b0 + Bt theta,  hvec = h0 + Ht theta
// with sparse Qt (nx x np), Bt (ne x np), Ht (nc x np), as a user of calipso_hip_sparse_kkt_set_evaluator + set_parameter_patterns would write it.  Hence
//     Lx,theta = Qt,   g,theta = -Bt,   h,theta = Ht,   all constant:
// asked for a parameter bit, the evaluator copies the non-zeros (in the order of the patterns given to set_parameter_patterns) into the handle's resident arrays; the
// dual terms of Lx,theta are zero.  The user object holds CSR copies of the six matrices for the row products (one thread per row, a fixed order per row).  Everything
// is enqueued on the stream the handle passes; nothing waits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/calipso_hip.h"

namespace {

struct Csr { int rows = 0; int *ptr = nullptr, *col = nullptr; double* val = nullptr; };      // device arrays
struct Dev {                                                     // what the kernels read, by value
    int nx = 0, ne = 0, nc = 0, np = 0;
    Csr L, g, h, Qt, Bt, Ht;
    double *q0 = nullptr, *b0 = nullptr, *h0 = nullptr, *fpart = nullptr;
};
struct User : Dev {
    double* nz[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // Lxx, gx, hx, Lx,theta, g,theta, h,theta: the non-zeros in the handle's order
    long long nnz[6] = {0, 0, 0, 0, 0, 0};
    std::vector<void*> owned;
};

__device__ double row_dot(const Csr m, int r, const double* __restrict__ x) {
    double a = 0.0;
    for (int p = m.ptr[r]; p < m.ptr[r + 1]; ++p) a += m.val[p] * x[m.col[p]];
    return a;
}
// one thread per row of [x; equality; cone]
__global__ __launch_bounds__(256) void k_rows(Dev u, uint32_t flags, const double* __restrict__ x, const double* __restrict__ theta, calipso_device_sparse_data out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < u.nx) {
        if (!(flags & (CALIPSO_EVAL_OBJECTIVE | CALIPSO_EVAL_OBJECTIVE_GRADIENT))) return;
        const double Lx = row_dot(u.L, k, x), q = u.q0[k] + row_dot(u.Qt, k, theta);
        if (flags & CALIPSO_EVAL_OBJECTIVE_GRADIENT) out.objective_gradient_variables[k] = Lx + q;
        if (flags & CALIPSO_EVAL_OBJECTIVE) u.fpart[k] = 0.5 * x[k] * Lx + q * x[k];
    } else if (k < u.nx + u.ne) {
        const int i = k - u.nx;
        if (flags & CALIPSO_EVAL_EQUALITY) out.equality_constraint[i] = row_dot(u.g, i, x) - (u.b0[i] + row_dot(u.Bt, i, theta));
    } else if (k < u.nx + u.ne + u.nc) {
        const int c = k - u.nx - u.ne;
        if (flags & CALIPSO_EVAL_CONE) out.cone_constraint[c] = row_dot(u.h, c, x) + (u.h0[c] + row_dot(u.Ht, c, theta));
    }
}
// the objective: one workgroup, thread t adds the terms t, t + 256, ..., then a fixed tree
__global__ __launch_bounds__(256) void k_objective(int nx, const double* __restrict__ fpart, double* __restrict__ f) {
    __shared__ double tree[256];
    double a = 0.0;
    for (int k = threadIdx.x; k < nx; k += 256) a += fpart[k];
    tree[threadIdx.x] = a;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) tree[threadIdx.x] += tree[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) f[0] = tree[0];
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

// sizes = nx, ne, nc, np.  Six matrices in the order Lxx, gx, hx, Qt, Bt, Ht: CSR row pointers, columns and values (0-based), and the non-zeros in the order of the
// pattern given to the handle (create for the first three, set_parameter_patterns for the last three; the fixture negates Bt's to get g,theta).  q0, b0, h0
__attribute__((visibility("default"))) void* qp_sparse_parameters_create(const int32_t* sizes, const int32_t* const* ptr, const int32_t* const* col, const double* const* val,
                                                                         const double* const* nz, const double* q0, const double* b0, const double* h0) {
    User* u = new User();
    u->nx = sizes[0]; u->ne = sizes[1]; u->nc = sizes[2]; u->np = sizes[3];
    Csr* m[6] = {&u->L, &u->g, &u->h, &u->Qt, &u->Bt, &u->Ht};
    const int rows[6] = {u->nx, u->ne, u->nc, u->nx, u->ne, u->nc};
    bool ok = true;
    for (int k = 0; k < 6 && ok; ++k) {
        m[k]->rows = rows[k];
        const size_t count = (size_t)ptr[k][rows[k]];
        u->nnz[k] = (long long)count;
        std::vector<double> ordered(nz[k], nz[k] + count);
        if (k == 4) for (double& v : ordered) v = -v;             // g,theta = -Bt
        ok = (m[k]->ptr = to_device(u, ptr[k], (size_t)rows[k] + 1)) && (m[k]->col = to_device(u, col[k], count)) && (m[k]->val = to_device(u, val[k], count)) &&
             (u->nz[k] = to_device(u, ordered.data(), count));
    }
    ok = ok && (u->q0 = to_device(u, q0, (size_t)u->nx)) && (u->b0 = to_device(u, b0, (size_t)u->ne)) && (u->h0 = to_device(u, h0, (size_t)u->nc));
    if (ok && (ok = hipMalloc((void**)&u->fpart, sizeof(double) * (size_t)(u->nx ? u->nx : 1)) == hipSuccess)) u->owned.push_back(u->fpart);
    if (!ok) { for (void* p : u->owned) (void)hipFree(p); delete u; return nullptr; }
    return u;
}
__attribute__((visibility("default"))) void qp_sparse_parameters_destroy(void* user) {
    User* u = (User*)user;
    if (!u) return;
    for (void* p : u->owned) (void)hipFree(p);
    delete u;
}

__attribute__((visibility("default"))) int32_t qp_sparse_parameters_eval(void* user, uint32_t flags, const double* x, const double* y, const double* z, const double* theta,
                                                                         const calipso_device_sparse_data* out, void* hip_stream) {
    User* u = (User*)user;
    (void)y; (void)z;                                         // the constraints are affine: the dual Hessians and the dual terms of Lx,theta are zero
    if (!u || !out || out->nx != u->nx || out->ne != u->ne || out->nc != u->nc || out->np != u->np || out->nnz_Lxx != u->nnz[0] || out->nnz_gx != u->nnz[1] ||
        out->nnz_hx != u->nnz[2]) return 1;
    const uint32_t LPAR = CALIPSO_EVAL_OBJECTIVE_JACOBIAN_PARAMETERS | CALIPSO_EVAL_EQUALITY_DUAL_JACOBIAN_PARAMETERS | CALIPSO_EVAL_CONE_DUAL_JACOBIAN_PARAMETERS;
    const uint32_t PAR = LPAR | CALIPSO_EVAL_EQUALITY_JACOBIAN_PARAMETERS | CALIPSO_EVAL_CONE_JACOBIAN_PARAMETERS;
    if ((flags & PAR) && (!out->Lp_colptr || !out->gp_colptr || !out->hp_colptr || out->nnz_Lp != u->nnz[3] || out->nnz_gp != u->nnz[4] || out->nnz_hp != u->nnz[5])) return 1;
    hipStream_t stream = (hipStream_t)hip_stream;
    const int rows = u->nx + u->ne + u->nc;
    if (rows && (flags & (CALIPSO_EVAL_OBJECTIVE | CALIPSO_EVAL_OBJECTIVE_GRADIENT | CALIPSO_EVAL_EQUALITY | CALIPSO_EVAL_CONE)))
        hipLaunchKernelGGL(k_rows, dim3((rows + 255) / 256), dim3(256), 0, stream, (Dev)*u, flags, x, theta, *out);
    if (flags & CALIPSO_EVAL_OBJECTIVE) hipLaunchKernelGGL(k_objective, dim3(1), dim3(256), 0, stream, u->nx, u->fpart, out->objective);
    // every matrix is constant: the non-zeros as they were given, into the handle's arrays
    const size_t D = sizeof(double);
    struct Copy { uint32_t copy, zero; double* to; int k; };
    const Copy copies[6] = {{CALIPSO_EVAL_OBJECTIVE_HESSIAN, CALIPSO_EVAL_EQUALITY_DUAL_HESSIAN | CALIPSO_EVAL_CONE_DUAL_HESSIAN, out->lagrangian_hessian, 0},
                            {CALIPSO_EVAL_EQUALITY_JACOBIAN, 0, out->equality_jacobian_variables, 1},
                            {CALIPSO_EVAL_CONE_JACOBIAN, 0, out->cone_jacobian_variables, 2},
                            {CALIPSO_EVAL_OBJECTIVE_JACOBIAN_PARAMETERS, LPAR, out->lagrangian_gradient_parameters, 3},
                            {CALIPSO_EVAL_EQUALITY_JACOBIAN_PARAMETERS, 0, out->equality_jacobian_parameters, 4},
                            {CALIPSO_EVAL_CONE_JACOBIAN_PARAMETERS, 0, out->cone_jacobian_parameters, 5}};
    for (const Copy& c : copies) {
        if (!u->nnz[c.k]) continue;
        if (flags & c.copy) { if (hipMemcpyAsync(c.to, u->nz[c.k], D * (size_t)u->nnz[c.k], hipMemcpyDeviceToDevice, stream) != hipSuccess) return 2; }
        else if (flags & c.zero) { if (hipMemsetAsync(c.to, 0, D * (size_t)u->nnz[c.k], stream) != hipSuccess) return 2; }      // only the zero terms were asked for
    }
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
