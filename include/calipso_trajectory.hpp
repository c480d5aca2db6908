// calipso_trajectory.hpp — the runtime of a trajectory problem's device evaluators for libcalipso_hip.so.  calipso.jl_amd/trajectory.py generates, per problem, the
// per-template device functions and a problem type, includes this header and ends in
//
//     CALIPSO_TRAJECTORY_EVALUATOR(my_problem_type, my_problem)
//
// which emits the six entries
//     my_problem_device_eval          calipso_device_eval_fn        (dense layout)
//     my_problem_block_eval           calipso_device_block_eval_fn  (the packed blocks of a structured handle)
//     my_problem_sparse_eval          calipso_device_sparse_eval_fn (the non-zero arrays of a sparse handle, on their stored patterns)
//     my_problem_user_create          (the int32 blob of TrajectoryProblem.tables(), words) -> the user object, NULL when the blob is refused
//     my_problem_user_destroy         (user object)
//     my_problem_debug_last_enqueued  (user object) -> operations the last evaluation call enqueued
// The three evaluators run the same kernels; they differ in the address table (entry -> offset in the destination), built once per handle on the first call by
// calipso_trajectory_tables.hpp — the plain C++ half: the blob's checks and every address computed on the host — and uploaded from pinned memory in one copy.  One call
// enqueues at most four operations: that upload, the fill, the evaluation kernel, the finishing pass.
//
// The problem type (S below):
//     struct my_problem_type {
//         static constexpr int NT = ...;                                       // templates, at most 96 (EvalArgs travels by value)
//         static constexpr int KIND[NT], NV[NT], M[NT], NTH[NT], ND[NT], NQ[NT] = ...;   // calipso::trajectory::Shape
//         __device__ static void call(int k, unsigned flags, int s, int n, const double* x, const double* y, const double* z, const double* th, const int* vi,
//                                     const int* ri, const int* pi, const int* ad, double* const* base, double* part);   // instance s of template k
//     };
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "calipso_hip.h"
#include "calipso_trajectory_tables.hpp"

namespace calipso {
namespace trajectory {

constexpr uint32_t HESS = CALIPSO_EVAL_OBJECTIVE_HESSIAN | CALIPSO_EVAL_EQUALITY_DUAL_HESSIAN | CALIPSO_EVAL_CONE_DUAL_HESSIAN;
constexpr uint32_t LPAR = CALIPSO_EVAL_OBJECTIVE_JACOBIAN_PARAMETERS | CALIPSO_EVAL_EQUALITY_DUAL_JACOBIAN_PARAMETERS | CALIPSO_EVAL_CONE_DUAL_JACOBIAN_PARAMETERS;
constexpr int FILL_DEST[N_FILL] = {D_GX, D_HX, D_LXX, D_GP, D_HP, D_LGP};
constexpr uint32_t FILL_FLAGS[N_FILL] = {CALIPSO_EVAL_EQUALITY_JACOBIAN, CALIPSO_EVAL_CONE_JACOBIAN, HESS, CALIPSO_EVAL_EQUALITY_JACOBIAN_PARAMETERS,
                                         CALIPSO_EVAL_CONE_JACOBIAN_PARAMETERS, LPAR};

template <int NT> struct EvalArgs {            // (by value: a few hundred bytes)
    const double *x, *y, *z, *th;
    double* part;
    const int* tab;                            // the device tables
    double* base[N_DEST];
    uint32_t flags;
    int n[NT], wg0[NT + 1], part0[NT], vi[NT], ri[NT], pi[NT], ad[NT];      // per template: instances, first workgroup, first partial, offsets of its tables in tab
};
struct FinishArgs {
    const double* part;
    const int* tab;
    double* base[N_DEST];
    uint32_t flags;
    int G, W, n_obj, g_addr, g_field, g_slots, obj_slots;
};
struct FillArgs {
    const int* tab;
    double* base[N_FILL];
    int first[N_FILL], wg0[N_FILL + 1];        // per selected category: its first chunk in the chunk table, its first workgroup
    int count, c_off, c_len;
};

// a lane per stage instance of a template; different templates in different workgroup ranges of the same launch
template <class S> __global__ __launch_bounds__(64) void k_evaluate(EvalArgs<S::NT> a) {
    const int b = blockIdx.x;
    int k = 0;
    while (k + 1 < S::NT && b >= a.wg0[k + 1]) ++k;            // workgroup-uniform
    const int s = (b - a.wg0[k]) * 64 + threadIdx.x;
    S::call(k, a.flags, s, a.n[k], a.x, a.y, a.z, a.th, a.tab + a.vi[k], a.tab + a.ri[k], a.tab + a.pi[k], a.tab + a.ad[k], a.base, a.part + a.part0[k]);
}

// the sums: a lane per summed output adds its partials in the order of the list; the last workgroup adds the stage costs (lane l the costs l, l + 64, ..., then a
// fixed tree)
static __global__ __launch_bounds__(64) void k_finish(FinishArgs a) {
    __shared__ double tree[64];
    if (blockIdx.x == gridDim.x - 1) {
        if (!(a.flags & CALIPSO_EVAL_OBJECTIVE)) return;
        double acc = 0.0;
        for (int i = threadIdx.x; i < a.n_obj; i += 64) acc += a.part[a.tab[a.obj_slots + i]];
        tree[threadIdx.x] = acc;
        __syncthreads();
        for (int w = 32; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) tree[threadIdx.x] += tree[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) a.base[D_F][0] = tree[0];
        return;
    }
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= a.G) return;
    const int f = a.tab[a.g_field + g];
    const uint32_t need = f == D_GYX ? CALIPSO_EVAL_EQUALITY_DUAL_GRADIENT : f == D_HZX ? CALIPSO_EVAL_CONE_DUAL_GRADIENT : f == D_LXX ? HESS : LPAR;
    if (!(a.flags & need)) return;
    double acc = 0.0;
    for (int w = 0; w < a.W; ++w) {
        const int word = a.tab[a.g_slots + w * a.G + g];
        if (word < 0) break;
        const int cls = word >> 29, slot = word & ((1 << 29) - 1);
        uint32_t bit = need;
        if (f == D_LXX) bit = cls == 0 ? CALIPSO_EVAL_OBJECTIVE_HESSIAN : cls == 1 ? CALIPSO_EVAL_EQUALITY_DUAL_HESSIAN : CALIPSO_EVAL_CONE_DUAL_HESSIAN;
        if (f == D_LGP) bit = cls == 0 ? CALIPSO_EVAL_OBJECTIVE_JACOBIAN_PARAMETERS : cls == 1 ? CALIPSO_EVAL_EQUALITY_DUAL_JACOBIAN_PARAMETERS : CALIPSO_EVAL_CONE_DUAL_JACOBIAN_PARAMETERS;
        if (a.flags & bit) acc += a.part[slot];
    }
    a.base[f][a.tab[a.g_addr + g]] = acc;
}

static __global__ __launch_bounds__(256) void k_fill(FillArgs a) {
    const int b = blockIdx.x;
    int c = 0;
    while (c + 1 < a.count && b >= a.wg0[c + 1]) ++c;
    const int chunk = a.first[c] + (b - a.wg0[c]);
    const int off = a.tab[a.c_off + chunk], len = a.tab[a.c_len + chunk];
    double* dst = a.base[c] + off;
    for (int i = threadIdx.x; i < len; i += 256) dst[i] = 0.0;
}

struct Route {                                 // one layout of the destinations: its table on the host and on the device, and where it came from
    bool ready = false;
    RouteTable t;
    int* pinned = nullptr; int* device = nullptr;
    const void* key0 = nullptr; int64_t key1 = 0;      // the layout it was built for: (descriptor array, first block's values) or (nullptr, jacobian_ld)
    const void* key2 = nullptr; const void* key3 = nullptr;      // ... or, with key0, the three nzval arrays of a sparse handle
    double* block_base = nullptr;
};

struct User {
    Tables t;
    double* part = nullptr;
    Route dense, block, sparse;
    int last_enqueued = 0;
};

template <class S> inline Shape shape_of() { return Shape{S::NT, S::KIND, S::NV, S::M, S::NTH, S::ND, S::NQ}; }

// one pinned block, one device block, one copy
inline int upload(User* u, Route& r, hipStream_t stream) {
    const size_t words = r.t.words.size() ? r.t.words.size() : 1;
    if (hipHostMalloc((void**)&r.pinned, words * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) return 2;
    if (hipMalloc((void**)&r.device, words * sizeof(int32_t)) != hipSuccess) return 2;
    if (!r.t.words.empty()) memcpy(r.pinned, r.t.words.data(), r.t.words.size() * sizeof(int32_t));
    if (hipMemcpyAsync(r.device, r.pinned, words * sizeof(int32_t), hipMemcpyHostToDevice, stream) != hipSuccess) return 2;
    ++u->last_enqueued;
    r.ready = true;
    return 0;
}

// fill, evaluate, finish on the stream: at most three launches
template <class S>
int run(User* u, const Route& r, uint32_t flags, const double* x, const double* y, const double* z, const double* th, double* const* base, hipStream_t stream) {
    const Tables& t = u->t;
    FillArgs fa;
    fa.tab = r.device; fa.count = 0; fa.c_off = r.t.c_off; fa.c_len = r.t.c_len; fa.wg0[0] = 0;
    for (int c = 0; c < N_FILL; ++c)
        if ((flags & FILL_FLAGS[c]) && r.t.fill_count[c] > 0 && base[FILL_DEST[c]]) {
            fa.base[fa.count] = base[FILL_DEST[c]]; fa.first[fa.count] = r.t.fill_first[c]; fa.wg0[fa.count + 1] = fa.wg0[fa.count] + r.t.fill_count[c]; ++fa.count;
        }
    if (fa.count > 0) { hipLaunchKernelGGL(k_fill, dim3(fa.wg0[fa.count]), dim3(256), 0, stream, fa); ++u->last_enqueued; }
    EvalArgs<S::NT> ea;
    ea.x = x; ea.y = y; ea.z = z; ea.th = th; ea.part = u->part; ea.tab = r.device; ea.flags = flags;
    for (int d = 0; d < N_DEST; ++d) ea.base[d] = base[d];
    int wg = 0; int64_t p0 = 0;
    for (int k = 0; k < S::NT; ++k) {
        ea.n[k] = t.n[k]; ea.wg0[k] = wg; ea.part0[k] = (int)p0; ea.vi[k] = r.t.vi[k]; ea.ri[k] = r.t.ri[k]; ea.pi[k] = r.t.pi[k]; ea.ad[k] = r.t.ad[k];
        wg += (t.n[k] + 63) / 64; p0 += (int64_t)S::NQ[k] * t.n[k];
    }
    ea.wg0[S::NT] = wg;
    if (wg > 0) { hipLaunchKernelGGL(k_evaluate<S>, dim3(wg), dim3(64), 0, stream, ea); ++u->last_enqueued; }
    if (flags & (CALIPSO_EVAL_OBJECTIVE | CALIPSO_EVAL_EQUALITY_DUAL_GRADIENT | CALIPSO_EVAL_CONE_DUAL_GRADIENT | HESS | LPAR)) {
        FinishArgs fi;
        fi.part = u->part; fi.tab = r.device; fi.flags = flags; fi.G = t.G; fi.W = t.W; fi.n_obj = t.n_obj;
        for (int d = 0; d < N_DEST; ++d) fi.base[d] = base[d];
        fi.g_addr = r.t.g_addr; fi.g_field = r.t.g_field; fi.g_slots = r.t.g_slots; fi.obj_slots = r.t.obj_slots;
        hipLaunchKernelGGL(k_finish, dim3((t.G + 63) / 64 + 1), dim3(64), 0, stream, fi);
        ++u->last_enqueued;
    }
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

inline void free_route(Route& r) {
    if (r.device) (void)hipFree(r.device);
    if (r.pinned) (void)hipHostFree(r.pinned);
    r = Route();
}

// tables: the int32 blob of TrajectoryProblem.tables(); returns NULL when it does not fit this library or an index lies outside its range
template <class S> void* user_create(const int32_t* blob, int64_t words) {
    User* u = new User();
    bool ok = parse_tables(shape_of<S>(), blob, words, u->t);
    if (ok && hipMalloc((void**)&u->part, sizeof(double) * (size_t)(u->t.n_part ? u->t.n_part : 1)) != hipSuccess) ok = false;
    if (!ok) { delete u; return nullptr; }
    return u;
}

inline void user_destroy(void* p) {
    User* u = (User*)p;
    if (!u) return;
    free_route(u->dense); free_route(u->block); free_route(u->sparse);
    if (u->part) (void)hipFree(u->part);
    delete u;
}

inline int32_t last_enqueued(void* p) { return p ? ((User*)p)->last_enqueued : -1; }

template <class S>
int32_t device_eval(void* user, uint32_t flags, const double* x, const double* y, const double* z, const double* theta, const calipso_device_problem_data* out,
                    void* hip_stream) {
    User* u = (User*)user;
    if (!u || !out || out->nx != u->t.nx || out->ne != u->t.ne || out->nc != u->t.nc || out->np != u->t.np) return 1;
    hipStream_t stream = (hipStream_t)hip_stream;
    u->last_enqueued = 0;
    Route& r = u->dense;
    if (r.ready && (r.key1 != out->jacobian_ld)) return 3;               // the layout changed under the handle
    if (!r.ready) {
        r.key1 = out->jacobian_ld;
        int rc = dense_route(shape_of<S>(), u->t, out->jacobian_ld, r.t);
        if (!rc) rc = upload(u, r, stream);
        if (rc) { free_route(r); return rc; }
    }
    double* base[N_DEST] = {out->objective_gradient_variables, out->equality_constraint, out->cone_constraint, out->equality_jacobian_variables,
                            out->cone_jacobian_variables, out->equality_jacobian_parameters, out->cone_jacobian_parameters, out->objective,
                            out->equality_dual_jacobian_variables, out->cone_dual_jacobian_variables, out->lagrangian_hessian, out->lagrangian_gradient_parameters};
    return run<S>(u, r, flags, x, y, z, theta, base, stream);
}

template <class S>
int32_t block_eval(void* user, uint32_t flags, const double* x, const double* y, const double* z, const double* theta, const calipso_device_block_data* out,
                   void* hip_stream) {
    User* u = (User*)user;
    if (!u || !out || out->nx != u->t.nx || out->ne != u->t.ne || out->nc != u->t.nc || out->np != u->t.np) return 1;
    if (out->n_jacobian_blocks + out->n_hessian_blocks < 1 || (out->n_jacobian_blocks && !out->jacobian_blocks) || (out->n_hessian_blocks && !out->hessian_blocks)) return 1;
    hipStream_t stream = (hipStream_t)hip_stream;
    u->last_enqueued = 0;
    Route& r = u->block;
    const void* key0 = out->n_hessian_blocks ? (const void*)out->hessian_blocks : (const void*)out->jacobian_blocks;
    const int64_t key1 = (int64_t)(intptr_t)(out->n_hessian_blocks ? out->hessian_blocks[0].values : out->jacobian_blocks[0].values);
    if (r.ready && (r.key0 != key0 || r.key1 != key1)) return 3;
    if (!r.ready) {
        r.key0 = key0; r.key1 = key1;
        int rc = block_route(shape_of<S>(), u->t, out, r.t, &r.block_base);
        if (!rc) rc = upload(u, r, stream);
        if (rc) { free_route(r); return rc; }
    }
    double* base[N_DEST] = {out->objective_gradient_variables, out->equality_constraint, out->cone_constraint, r.block_base, r.block_base,
                            out->equality_jacobian_parameters, out->cone_jacobian_parameters, out->objective, out->equality_dual_jacobian_variables,
                            out->cone_dual_jacobian_variables, r.block_base, out->lagrangian_gradient_parameters};
    return run<S>(u, r, flags, x, y, z, theta, base, stream);
}

// the sparse handle's route: the Jacobians' and the Hessian's non-zeros go to their positions in the handle's nzval arrays.  It has no destination for the dual
// gradients (the handle gathers them): such flags are code 1.  The derivatives with respect to theta go to the handle's stored parameter patterns when it has them
// (the three parameter pattern pointers of calipso_device_sparse_data are non-NULL); without them those flags are code 1 as well
template <class S>
int32_t sparse_eval(void* user, uint32_t flags, const double* x, const double* y, const double* z, const double* theta, const calipso_device_sparse_data* out,
                    void* hip_stream) {
    User* u = (User*)user;
    if (!u || !out || out->nx != u->t.nx || out->ne != u->t.ne || out->nc != u->t.nc || out->np != u->t.np) return 1;
    const bool parameters = SparseLayout{out}.parameters();
    if (flags & (CALIPSO_EVAL_EQUALITY_DUAL_GRADIENT | CALIPSO_EVAL_CONE_DUAL_GRADIENT)) return 1;
    if (!parameters && (flags & (CALIPSO_EVAL_EQUALITY_JACOBIAN_PARAMETERS | CALIPSO_EVAL_CONE_JACOBIAN_PARAMETERS | LPAR))) return 1;
    hipStream_t stream = (hipStream_t)hip_stream;
    u->last_enqueued = 0;
    Route& r = u->sparse;
    if (r.ready && (r.key0 != out->lagrangian_hessian || r.key2 != out->equality_jacobian_variables || r.key3 != out->cone_jacobian_variables)) return 3;
    if (r.ready && r.key1 != (int64_t)(intptr_t)out->lagrangian_gradient_parameters) {      // the handle's parameter patterns were set or replaced: the addresses are others
        if (hipStreamSynchronize(stream) != hipSuccess) return 2;
        free_route(r);
    }
    if (!r.ready) {
        r.key0 = out->lagrangian_hessian; r.key2 = out->equality_jacobian_variables; r.key3 = out->cone_jacobian_variables;
        r.key1 = (int64_t)(intptr_t)out->lagrangian_gradient_parameters;
        int rc = sparse_route(shape_of<S>(), u->t, out, r.t);
        if (!rc) rc = upload(u, r, stream);
        if (rc) { free_route(r); return rc; }
    }
    double* base[N_DEST] = {out->objective_gradient_variables, out->equality_constraint, out->cone_constraint, out->equality_jacobian_variables,
                            out->cone_jacobian_variables, parameters ? out->equality_jacobian_parameters : nullptr, parameters ? out->cone_jacobian_parameters : nullptr,
                            out->objective, nullptr, nullptr, out->lagrangian_hessian, parameters ? out->lagrangian_gradient_parameters : nullptr};
    return run<S>(u, r, flags, x, y, z, theta, base, stream);
}

}  // namespace trajectory
}  // namespace calipso

#define CALIPSO_TRAJECTORY_EVALUATOR(S, name) \
    extern "C" { \
    __attribute__((visibility("default"))) void* name##_user_create(const int32_t* blob, int64_t words) { return calipso::trajectory::user_create<S>(blob, words); } \
    __attribute__((visibility("default"))) void name##_user_destroy(void* user) { calipso::trajectory::user_destroy(user); } \
    __attribute__((visibility("default"))) int32_t name##_debug_last_enqueued(void* user) { return calipso::trajectory::last_enqueued(user); } \
    __attribute__((visibility("default"))) int32_t name##_device_eval(void* user, uint32_t flags, const double* x, const double* y, const double* z, const double* theta, \
                                                                      const calipso_device_problem_data* out, void* hip_stream) { \
        return calipso::trajectory::device_eval<S>(user, flags, x, y, z, theta, out, hip_stream); \
    } \
    __attribute__((visibility("default"))) int32_t name##_block_eval(void* user, uint32_t flags, const double* x, const double* y, const double* z, const double* theta, \
                                                                     const calipso_device_block_data* out, void* hip_stream) { \
        return calipso::trajectory::block_eval<S>(user, flags, x, y, z, theta, out, hip_stream); \
    } \
    __attribute__((visibility("default"))) int32_t name##_sparse_eval(void* user, uint32_t flags, const double* x, const double* y, const double* z, const double* theta, \
                                                                      const calipso_device_sparse_data* out, void* hip_stream) { \
        return calipso::trajectory::sparse_eval<S>(user, flags, x, y, z, theta, out, hip_stream); \
    } \
    }
