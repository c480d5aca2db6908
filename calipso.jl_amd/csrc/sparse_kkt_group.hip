// sparse_kkt_group.hip — search_direction! (src/solver/search_direction.jl:1-23) for a GROUP of same-pattern sparse problems in lockstep: the handle behind
// calipso_hip_sparse_kkt_group_* (include/calipso_hip.h).  One analysis (sparse_kkt.hpp), one device copy of its tables, one multifrontal plan with
// set_batch(members); per member its own Lxx, gx, hx, point, penalty, kappa and work vectors, member-major in one slab (sparse_kkt_group.hpp: Layout).  The assembled K
// of member m is the plan's own value storage (sparse_values(): stride nnz(triu K)): the assemble writes in place, nothing is copied.
//
//   kernels        the group forms of sparse_kkt.hip's: the member on blockIdx.z through the list of ACTIVE members (Active: members, and their (ep, ed), by value),
//                  the pointers shifted by the member's strides, then the SAME __device__ bodies (sparse_kkt_kernels.hpp): a member's arithmetic is the single
//                  handle's, operation for operation, whatever the group's size and the member's place in it.  One norm slot per member.
//   driver         search_direction of sparse_kkt.hip line for line over sets of members (sparse_kkt_group.hpp: Lockstep): every inertia-correction round assembles
//                  and factors only the members still walking and reads all their inertias back at once; one pre launch, one batched solve, one post launch for all
//                  that passed; a refinement round is one fused H v / norm pass, ONE read-back of the norms, refine_next per member, the correction solve and add
//                  for those that go on.  The host waits of a call are those of its slowest member and its launches do not depend on the number of members.
// No `H \ residual` fallback here: a member whose refinement fails gets status 2 and its last refined step.
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "sparse_kkt_group_handle.hpp"     // the group handle, Strides, member_data: shared with sparse_solve_group.hip
#include "sparse_kkt_kernels.hpp"

using calipso::Batch;
using calipso::i64;
using namespace calipso::sparse_kkt;
namespace grp = calipso::sparse_kkt_group;
using grp::GH;
using grp::Strides;
using grp::member_data;
static_assert(grp::MAX_MEMBERS == calipso::MAX_BATCH, "a group is a batch of the multifrontal plan");
static_assert(grp::STATUS_OK == CALIPSO_OK && grp::STATUS_REFINEMENT == CALIPSO_WARN_REFINEMENT && grp::STATUS_INERTIA == CALIPSO_ERR_INERTIA && grp::REFUSED == CALIPSO_ERR_ARGUMENT, "statuses");

namespace {

// ---- the group kernels: blockIdx.z = place in the active list ---------------------------------------------------------------------------------------------------
struct Active { int n; int member[calipso::MAX_BATCH]; double ep[calipso::MAX_BATCH], ed[calipso::MAX_BATCH]; };      // members walk different regularisations

__device__ __forceinline__ Sink member_sink(const Sink& k, const Strides& s, int m) {
    const size_t o = (size_t)m * s.N;
    return Sink{k.out ? k.out + o : nullptr, k.res ? k.res + o : nullptr, k.err ? k.err + o : nullptr, k.norm ? k.norm + m : nullptr};
}

__global__ __launch_bounds__(KT) void k_kkt_group_assemble(const KktDev d, const Strides s, const Active a, double* __restrict__ K) {
    const int z = blockIdx.z, m = a.member[z];
    assemble_item(member_data(d, s, m), a.ep[z], a.ed[z], K + (size_t)m * s.K);
}
template <bool WAVE>
__global__ __launch_bounds__(KT) void k_kkt_group_mul_gathered(const KktDev d, const Strides s, const Active a, const double* __restrict__ V, const Sink sink) {
    const int z = blockIdx.z, m = a.member[z];
    mul_gathered_item<WAVE>(member_data(d, s, m), a.ep[z], a.ed[z], V + (size_t)m * s.N, member_sink(sink, s, m));
}
__global__ __launch_bounds__(KT) void k_kkt_group_mul_local(const KktDev d, const Strides s, const Active a, const double* __restrict__ V, const Sink sink) {
    const int z = blockIdx.z, m = a.member[z];
    mul_local_item(member_data(d, s, m), a.ep[z], a.ed[z], V + (size_t)m * s.N, member_sink(sink, s, m));
}
// forward only, one column per member: G (members x n) from V (members x N); OUT (members x N) from the solution Hs (members x n) and V
__global__ __launch_bounds__(KT) void k_kkt_group_map_pre(const KktDev d, const Strides s, const Active a, const double* __restrict__ V, double* __restrict__ G) {
    const int z = blockIdx.z, m = a.member[z];
    map_pre_item<false>(member_data(d, s, m), a.ep[z], a.ed[z], V + (size_t)m * s.N, G + (size_t)m * s.n, nullptr);
}
__global__ __launch_bounds__(KT) void k_kkt_group_map_post(const KktDev d, const Strides s, const Active a, const double* __restrict__ Hs, const double* __restrict__ V, double* __restrict__ OUT) {
    const int z = blockIdx.z, m = a.member[z];
    map_post_item<false>(member_data(d, s, m), a.ep[z], a.ed[z], Hs + (size_t)m * s.n, V + (size_t)m * s.N, OUT + (size_t)m * s.N);
}
__global__ __launch_bounds__(KT) void k_kkt_group_add(const Strides s, const Active a, int N, double* __restrict__ step, const double* __restrict__ corr) {
    const size_t o = (size_t)a.member[blockIdx.z] * s.N;
    add_item(N, step + o, corr + o);
}

thread_local std::string g_group_err;

int gfail(GH* g, int rc, const std::string& text) { if (g && g->base) g->base->err_text = text; else g_group_err = text; return rc; }
#define GREFUSE(text) do { const std::string t__ = (text); if (!t__.empty()) return gfail(g, CALIPSO_ERR_ARGUMENT, t__); } while (0)

double* arr(GH* g, grp::Array a) { return g->slab + g->lay.offset[a]; }
Strides strides(const GH* g) { return Strides{g->lay.stride[grp::A_LXX], g->lay.stride[grp::A_GX], g->lay.stride[grp::A_HX], g->base->d.N, g->base->d.n, g->strideK}; }

// the launch arguments of a set of members: the list, and every member's (ep, ed) as its last ic_begin / ic_after / factorize left them
Active active_of(const GH* g, const std::vector<int>& members) {
    Active a;
    a.n = (int)members.size();
    for (int z = 0; z < a.n; ++z) { const calipso::Scalars& sc = g->ls.m[(size_t)members[(size_t)z]].sc; a.member[z] = members[(size_t)z]; a.ep[z] = sc.ep; a.ed[z] = sc.ed; }
    return a;
}
// ... and for the plan: the storage slot of a member is its index; `stride` doubles between the members' pieces of the vector a solve works on
Batch batch_of(const std::vector<int>& members, long long stride) {
    Batch b;
    b.n = (int)members.size();
    for (int z = 0; z < b.n; ++z) { b.slot[z] = members[(size_t)z]; b.delta[z] = (long long)members[(size_t)z] * stride; }
    return b;
}
std::vector<int> everyone(const GH* g) { std::vector<int> all((size_t)g->members); for (int k = 0; k < g->members; ++k) all[(size_t)k] = k; return all; }

int values_missing(GH* g, const char* entry) {
    static const char* const names[5] = {"Lxx", "gx", "hx", "w", "penalty"};
    const KktDev& d = g->base->d;
    const size_t need[5] = {(size_t)d.nnzL, (size_t)d.nnzg, (size_t)d.nnzh, (size_t)d.N, (size_t)(d.ne > 0)};
    for (int i = 0; i < 5; ++i) if (need[i] && !g->have[i]) return gfail(g, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": no " + names[i] + " resident (calipso_hip_sparse_kkt_group_set_values first)");
    return CALIPSO_OK;
}

// ---- what the driver enqueues: nothing here waits for the device ---------------------------------------------------------------------------------------------------
// one assemble + one batched factorisation of `members` at their own (ep, ed); their inertias into g->inertia
int enqueue_assemble_factorize(GH* g, const std::vector<int>& members, int* launches) {
    KH* s = g->base;
    const KktDev& d = s->d;
    const long long items = (long long)d.nnzL + d.nnzg + d.nnzh + d.nx + d.ne + d.nc + d.ncc;
    const Active a = active_of(g, members);
    hipLaunchKernelGGL(k_kkt_group_assemble, dim3(blocks(items), 1, (unsigned)a.n), dim3(KT), 0, s->st, d, strides(g), a, g->K);
    const Batch bt = batch_of(members, 0);
    int rc = calipso::sparse_factor_from_dense(s->sp, s->st, bt, nullptr, nullptr, nullptr, true);      // the entries are in place already
    if (rc == CALIPSO_OK) rc = calipso::sparse_inertia_enqueue(s->sp, s->st, bt, g->inertia);
    if (rc < 0) return gfail(g, rc, "the batched factorisation refused its arguments");
    *launches += 2 + g->launches_factor;
    return CALIPSO_OK;
}
// search_direction_symmetric! (search_direction.jl:25-104) with the current factors of `members`: OUT (members x N) from V (members x N), both on the device
int enqueue_solve(GH* g, const std::vector<int>& members, const double* V, double* OUT, int* launches) {
    KH* s = g->base;
    const KktDev& d = s->d;
    const Active a = active_of(g, members);
    const dim3 grid(blocks((long long)d.n + d.nsoc), 1, (unsigned)a.n), block(KT);
    double* rsym = arr(g, grp::A_RSYM);
    hipLaunchKernelGGL(k_kkt_group_map_pre, grid, block, 0, s->st, d, strides(g), a, V, rsym);
    const int rc = calipso::sparse_solve_inplace(s->sp, s->st, batch_of(members, d.n), rsym);
    if (rc < 0) return gfail(g, rc, "the batched solve refused its arguments");
    hipLaunchKernelGGL(k_kkt_group_map_post, grid, block, 0, s->st, d, strides(g), a, rsym, V, OUT);
    *launches += 2 + g->launches_solve;
    return CALIPSO_OK;
}
void enqueue_mul(GH* g, const std::vector<int>& members, const double* V, const Sink& sink, int* launches) {
    KH* s = g->base;
    const KktDev& d = s->d;
    const Active a = active_of(g, members);
    const unsigned nz = (unsigned)a.n;
    if (s->wave_rows) hipLaunchKernelGGL(k_kkt_group_mul_gathered<true>, dim3(blocks(d.n, KT / 64), 1, nz), dim3(KT), 0, s->st, d, strides(g), a, V, sink);
    else hipLaunchKernelGGL(k_kkt_group_mul_gathered<false>, dim3(blocks(d.n), 1, nz), dim3(KT), 0, s->st, d, strides(g), a, V, sink);
    *launches += 1;
    if (d.ne + d.nc > 0) { hipLaunchKernelGGL(k_kkt_group_mul_local, dim3(blocks((long long)d.ne + 2ll * d.nc), 1, nz), dim3(KT), 0, s->st, d, strides(g), a, V, sink); *launches += 1; }
}

#define GK(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return gfail(g, CALIPSO_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); } while (0)

// search_direction! for the members `who` on device vectors (members x N each); the others are left as they are
int search_direction(GH* g, const std::vector<int>& who, const double* res, double* step, double* regularization, double* info, int32_t* status, double* report) {
    const auto wall0 = std::chrono::steady_clock::now();
    KH* s = g->base;
    const KktDev& d = s->d;
    grp::Lockstep& ls = g->ls;
    int waits = 0, launches = 0;
    for (double& m : g->ms) m = 0.0;
    ls.begin(regularization, who);
    GK(hipEventRecord(g->ev[0], s->st));
    // inertia_correction! (inertia.jl:30-80): a round per retry of the slowest member
    for (;;) {
        const std::vector<int> walking = ls.walking();
        if (walking.empty()) break;
        if (const int rc = enqueue_assemble_factorize(g, walking, &launches); rc < 0) return rc;
        GK(hipMemcpyAsync(g->inertia_host.data(), g->inertia, sizeof(int64_t) * 3 * (size_t)g->members, hipMemcpyDeviceToHost, s->st));
        GK(hipStreamSynchronize(s->st)); ++waits;
        ls.after_factorizations(walking, g->inertia_host.data(), d.nx, (i64)d.ne + d.nc);
    }
    g->assembled = true; g->factored = ls.in_phase(grp::FAILED_INERTIA).empty();
    GK(hipEventRecord(g->ev[1], s->st));
    const std::vector<int> passed = ls.passed();
    if (!passed.empty()) if (const int rc = enqueue_solve(g, passed, res, step, &launches); rc < 0) return rc;
    ls.after_solve();
    GK(hipEventRecord(g->ev[2], s->st));
    // iterative_refinement! (iterative_refinement.jl:1-52)
    double* err = arr(g, grp::A_ERR); double* corr = arr(g, grp::A_CORR); double* norm = arr(g, grp::A_NORM);
    std::vector<int> refining = ls.refining();
    for (bool first = true; !refining.empty(); first = false) {
        GK(hipMemsetAsync(norm, 0, sizeof(double) * (size_t)g->members, s->st));
        enqueue_mul(g, refining, step, Sink{nullptr, res, err, reinterpret_cast<unsigned long long*>(norm)}, &launches);      // err = res - H step and its infinity norm
        GK(hipMemcpyAsync(g->norm_host.data(), norm, sizeof(double) * (size_t)g->members, hipMemcpyDeviceToHost, s->st));
        GK(hipStreamSynchronize(s->st)); ++waits;
        refining = ls.after_norms(refining, g->norm_host.data(), first);
        if (refining.empty()) break;
        if (const int rc = enqueue_solve(g, refining, err, corr, &launches); rc < 0) return rc;
        hipLaunchKernelGGL(k_kkt_group_add, dim3(blocks(d.N), 1, (unsigned)refining.size()), dim3(KT), 0, s->st, strides(g), active_of(g, refining), d.N, step, corr);
        ++launches;
    }
    GK(hipEventRecord(g->ev[3], s->st));
    GK(hipStreamSynchronize(s->st)); ++waits;
    GK(hipGetLastError());
    float t[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < 3; ++k) GK(hipEventElapsedTime(&t[k], g->ev[k], g->ev[k + 1]));
    g->ms[0] = t[0]; g->ms[1] = t[1]; g->ms[2] = t[2]; g->ms[6] = (double)t[0] + t[1] + t[2];
    g->ms[5] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    ls.outputs(regularization, info, status, who);
    if (report) {
        report[grp::R_FACTOR_ROUNDS] = ls.factor_rounds; report[grp::R_REFINE_ROUNDS] = ls.refine_rounds; report[grp::R_HOST_WAITS] = waits; report[grp::R_LAUNCHES] = launches;
        report[grp::R_DEVICE_MS] = g->ms[6]; report[grp::R_WALL_MS] = g->ms[5]; report[grp::R_LAST_FACTOR_ACTIVE] = ls.last_factor_active; report[grp::R_LAST_REFINE_ACTIVE] = ls.last_refine_active;
    }
    const int worst = ls.worst(who);
    if (worst == CALIPSO_ERR_INERTIA) {
        std::string who;
        for (int k : ls.in_phase(grp::FAILED_INERTIA)) who += (who.empty() ? "" : ", ") + std::to_string(k);
        gfail(g, worst, "inertia correction failure (inertia.jl:72) of members " + who);
    }
    return worst;
}

int set_values(GH* g, const char* entry, const double* Lxx, const double* gx, const double* hx, const double* w, const double* penalty, const double* central_path, bool device) {
    if (!g) return CALIPSO_ERR_ARGUMENT;
    KH* s = g->base;
    GK(hipSetDevice(s->device));
    DEVPTR(Lxx); DEVPTR(gx); DEVPTR(hx); DEVPTR(w); DEVPTR(penalty);
    const hipMemcpyKind kind = device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const double* src[5] = {Lxx, gx, hx, w, penalty};
    const grp::Array dst[5] = {grp::A_LXX, grp::A_GX, grp::A_HX, grp::A_W, grp::A_RHO};
    for (int i = 0; i < 5; ++i) {
        const size_t count = (size_t)g->lay.stride[dst[i]] * (size_t)g->members;
        if (src[i] && count) { GK(hipMemcpyAsync(arr(g, dst[i]), src[i], sizeof(double) * count, kind, s->st)); g->have[i] = true; }
    }
    GK(hipStreamSynchronize(s->st));
    if (central_path) for (int k = 0; k < g->members; ++k) g->ls.m[(size_t)k].sc.kappa = central_path[k];      // (a host array on both routes: IC-2 reads it on the host)
    g->assembled = false; g->factored = false;      // every K and factor belongs to the values before
    return CALIPSO_OK;
}

int search_direction_entry(GH* g, const char* entry, const double* residual, double* step, double* regularization, double* info, int32_t* status, double* report, bool device) {
    if (!g) return CALIPSO_ERR_ARGUMENT;
    KH* s = g->base;
    if (!residual || !step || !regularization || !status) return gfail(g, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": residual, step, regularization and status are required");
    GK(hipSetDevice(s->device));
    DEVPTR(residual); DEVPTR(step);
    if (const int rc = values_missing(g, entry); rc < 0) return rc;
    if (device) return search_direction(g, everyone(g), residual, step, regularization, info, status, report);
    const size_t N = (size_t)s->d.N, bytes = sizeof(double) * N * (size_t)g->members;
    double* res = arr(g, grp::A_RES); double* stp = arr(g, grp::A_STEP);
    GK(hipMemcpyAsync(res, residual, bytes, hipMemcpyHostToDevice, s->st));
    GK(hipMemcpyAsync(stp, step, bytes, hipMemcpyHostToDevice, s->st));          // a member whose inertia correction fails keeps the caller's step
    const int rc = search_direction(g, everyone(g), res, stp, regularization, info, status, report);
    if (rc < 0 && rc != CALIPSO_ERR_INERTIA) return rc;
    GK(hipMemcpyAsync(step, stp, bytes, hipMemcpyDeviceToHost, s->st));
    GK(hipStreamSynchronize(s->st));
    return rc;
}

}  // namespace

// what sparse_solve_group.hip calls here (sparse_kkt_group_handle.hpp)
int grp::group_fail(GH* g, int rc, const std::string& text) { return gfail(g, rc, text); }
double* grp::group_array(GH* g, grp::Array a) { return arr(g, a); }
Strides grp::group_strides(const GH* g) { return strides(g); }
int grp::group_search_direction(GH* g, const std::vector<int>& members, const double* res, double* step, double* regularization, double* info, int32_t* status, double* report) {
    return search_direction(g, members, res, step, regularization, info, status, report);
}

extern "C" {

const char* calipso_hip_sparse_kkt_group_last_error(calipso_hip_sparse_kkt_group* g) { return g && g->base ? g->base->err_text.c_str() : g_group_err.c_str(); }

int32_t calipso_hip_sparse_kkt_group_destroy(calipso_hip_sparse_kkt_group* g) {
    if (!g) return CALIPSO_OK;
    if (g->base) {
        (void)hipSetDevice(g->base->device);
        if (g->base->st) (void)hipStreamSynchronize(g->base->st);
        for (hipEvent_t e : g->ev) if (e) (void)hipEventDestroy(e);
        grp::group_solve_release(g);
        (void)calipso_hip_sparse_kkt_destroy(g->base);      // the tables, the slab, the plan
    }
    delete g;
    return CALIPSO_OK;
}

static int32_t group_create_impl(GH* g, int32_t method, const int64_t* perm) {
    static const char* const entry = "calipso_hip_sparse_kkt_group_create";
    KH* s = g->base;
    if (const int rc = create_tables(s, method, perm); rc) return rc;
    int64_t sp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    (void)calipso_hip_sparse_info(s->sp, sp);
    GREFUSE(grp::check_numeric_phase(entry, sp[7]));
    int rc = calipso_hip_sparse_set_batch(s->sp, g->members);
    if (rc == CALIPSO_OK) rc = calipso::sparse_reserve_solve(s->sp, g->members);
    if (rc != CALIPSO_OK) return gfail(g, rc, std::string(entry) + ": no room for " + std::to_string(g->members) + " sets of values and factors: " + calipso_hip_sparse_last_error(s->sp));
    calipso::sparse_values(s->sp, &g->K, &g->strideK);
    if (g->strideK != s->an.nnzK()) return gfail(g, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": the plan's values are not those of triu(K)");
    g->launches_factor = (int)sp[4]; g->launches_solve = 2 * (int)sp[4] + 2;
    const KktDev& d = s->d;
    g->lay = grp::layout(g->members, d.nnzL, d.nnzg, d.nnzh, d.N, d.n);
    if ((rc = device_fixed(s, &g->slab, (size_t)g->lay.doubles)) || (rc = device_fixed(s, &g->inertia, 3 * (size_t)g->members))) return rc;
    KktDev& dv = s->d;                          // what the kernels read of member 0: the group kernels shift these by the member's strides
    dv.Lxx = arr(g, grp::A_LXX); dv.gx = arr(g, grp::A_GX); dv.hx = arr(g, grp::A_HX); dv.w = arr(g, grp::A_W); dv.rho = arr(g, grp::A_RHO);
    for (hipEvent_t& e : g->ev) GK(hipEventCreate(&e));
    GK(hipStreamSynchronize(s->st));
    g->ls = grp::Lockstep(g->members);
    g->inertia_host.assign(3 * (size_t)g->members, 0); g->norm_host.assign((size_t)g->members, 0.0);
    return CALIPSO_OK;
}

int32_t calipso_hip_sparse_kkt_group_create(int64_t nx, int64_t ne, int64_t nc, int64_t n_nonnegative, int64_t n_soc, const int64_t* dims, const int64_t* Lxx_colptr,
                                            const int64_t* Lxx_rowval, const int64_t* gx_colptr, const int64_t* gx_rowval, const int64_t* hx_colptr, const int64_t* hx_rowval,
                                            int32_t method, const int64_t* perm, int32_t device, int64_t members, calipso_hip_sparse_kkt_group** out) {
    static const char* const entry = "calipso_hip_sparse_kkt_group_create";
    GH* g = nullptr;
    if (!out) return CALIPSO_ERR_ARGUMENT;
    *out = nullptr;
    GREFUSE(grp::check_members(entry, members));
    if (method < 0 || method > 5 || (method == 3 && !perm)) return gfail(nullptr, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": method is 0 .. 5, and 3 comes with a perm");
    Analysis a = analyse(nx, ne, nc, n_nonnegative, n_soc, dims, Lxx_colptr, Lxx_rowval, gx_colptr, gx_rowval, hx_colptr, hx_rowval);
    if (a.status) return gfail(nullptr, a.status, std::string(entry) + ": " + a.message);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return gfail(nullptr, CALIPSO_ERR_HIP, "no HIP device available (libcalipso_hip has no CPU path)"); }
    if (device < 0 || device >= ndev) return gfail(nullptr, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": device ordinal out of range");
    g = new GH();
    g->base = new KH();
    g->base->an = std::move(a); g->base->device = device; g->members = (int)members;
    const int32_t rc = group_create_impl(g, method, perm);
    if (rc != CALIPSO_OK) { g_group_err = g->base->err_text; (void)calipso_hip_sparse_kkt_group_destroy(g); return rc; }      // no half-built handle leaves here
    *out = g;
    return CALIPSO_OK;
}

int32_t calipso_hip_sparse_kkt_group_info(calipso_hip_sparse_kkt_group* g, int64_t info[9]) {
    if (!g || !info) return CALIPSO_ERR_ARGUMENT;
    int64_t sp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    (void)calipso_hip_sparse_info(g->base->sp, sp);
    const Analysis& an = g->base->an;
    info[0] = an.n; info[1] = an.nnzK(); info[2] = sp[2]; info[3] = sp[3]; info[4] = sp[7]; info[5] = 1; info[6] = an.max_dim; info[7] = an.N; info[8] = g->members;
    return CALIPSO_OK;
}

int32_t calipso_hip_sparse_kkt_group_pattern(calipso_hip_sparse_kkt_group* g, int64_t* colptr, int64_t* rowval) {
    return g ? calipso_hip_sparse_kkt_pattern(g->base, colptr, rowval) : CALIPSO_ERR_ARGUMENT;
}

int32_t calipso_hip_sparse_kkt_group_set_option(calipso_hip_sparse_kkt_group* g, const char* name, double value) {
    static const char* const entry = "calipso_hip_sparse_kkt_group_set_option";
    if (!g || !name) return CALIPSO_ERR_ARGUMENT;
    GREFUSE(grp::check_option(entry, name, value));
    if (std::string(name) == "krylov_fallback") return CALIPSO_OK;                                          // (0: what a group does anyway)
    if (calipso::set_search_direction_option(g->ls.opt, name, value)) return CALIPSO_OK;
    if (std::string(name) == "central_path") { for (grp::Member& q : g->ls.m) q.sc.kappa = value; return CALIPSO_OK; }      // every member's; set_values takes one per member
    { const int rc = grp::group_solve_set_option(g, name, value); if (rc != 0) return rc < 0 ? rc : CALIPSO_OK; }         // what solve! reads besides (sparse_solve_group.hip)
    return gfail(g, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": unknown option " + name);
}

int32_t calipso_hip_sparse_kkt_group_set_values(calipso_hip_sparse_kkt_group* g, const double* Lxx, const double* gx, const double* hx, const double* w, const double* penalty, const double* central_path) {
    return set_values(g, "calipso_hip_sparse_kkt_group_set_values", Lxx, gx, hx, w, penalty, central_path, false);
}
int32_t calipso_hip_sparse_kkt_group_set_values_device(calipso_hip_sparse_kkt_group* g, const double* Lxx, const double* gx, const double* hx, const double* w, const double* penalty, const double* central_path) {
    return set_values(g, "calipso_hip_sparse_kkt_group_set_values_device", Lxx, gx, hx, w, penalty, central_path, true);
}

int32_t calipso_hip_sparse_kkt_group_factorize(calipso_hip_sparse_kkt_group* g, const double* ep, const double* ed, int64_t* inertia) {
    static const char* const entry = "calipso_hip_sparse_kkt_group_factorize";
    if (!g) return CALIPSO_ERR_ARGUMENT;
    GREFUSE(grp::check_required(entry, "ep", ep)); GREFUSE(grp::check_required(entry, "ed", ed));
    KH* s = g->base;
    GK(hipSetDevice(s->device));
    if (const int rc = values_missing(g, entry); rc < 0) return rc;
    for (int k = 0; k < g->members; ++k) { g->ls.m[(size_t)k].sc.ep = ep[k]; g->ls.m[(size_t)k].sc.ed = ed[k]; }
    int launches = 0;
    g->assembled = true; g->factored = false;
    if (const int rc = enqueue_assemble_factorize(g, everyone(g), &launches); rc < 0) return rc;
    GK(hipMemcpyAsync(g->inertia_host.data(), g->inertia, sizeof(int64_t) * 3 * (size_t)g->members, hipMemcpyDeviceToHost, s->st));
    GK(hipStreamSynchronize(s->st));
    GK(hipGetLastError());
    g->factored = true;
    int rc = CALIPSO_OK;
    for (int k = 0; k < g->members; ++k) if (g->inertia_host[3 * (size_t)k] < 0) rc = CALIPSO_WARN_ZERO_PIVOT;
    if (inertia) std::copy(g->inertia_host.begin(), g->inertia_host.end(), inertia);
    return rc;
}

int32_t calipso_hip_sparse_kkt_group_get_matrix(calipso_hip_sparse_kkt_group* g, int64_t member, double* nzval) {
    static const char* const entry = "calipso_hip_sparse_kkt_group_get_matrix";
    if (!g) return CALIPSO_ERR_ARGUMENT;
    GREFUSE(grp::check_member(entry, member, g->members)); GREFUSE(grp::check_required(entry, "nzval", nzval));
    if (!g->assembled) return gfail(g, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": factorize first");
    KH* s = g->base;
    GK(hipSetDevice(s->device));
    GK(hipMemcpyAsync(nzval, g->K + (size_t)member * (size_t)g->strideK, sizeof(double) * (size_t)s->an.nnzK(), hipMemcpyDeviceToHost, s->st));
    GK(hipStreamSynchronize(s->st));
    return CALIPSO_OK;
}

int32_t calipso_hip_sparse_kkt_group_mul(calipso_hip_sparse_kkt_group* g, const double* v, double* out) {
    static const char* const entry = "calipso_hip_sparse_kkt_group_mul";
    if (!g) return CALIPSO_ERR_ARGUMENT;
    GREFUSE(grp::check_required(entry, "v", v)); GREFUSE(grp::check_required(entry, "out", out));
    if (!g->assembled) return gfail(g, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": factorize first (H is taken at the regularisation of every member's last assemble)");
    KH* s = g->base;
    GK(hipSetDevice(s->device));
    const size_t bytes = sizeof(double) * (size_t)s->d.N * (size_t)g->members;
    double* corr = arr(g, grp::A_CORR); double* err = arr(g, grp::A_ERR);
    int launches = 0;
    GK(hipMemcpyAsync(corr, v, bytes, hipMemcpyHostToDevice, s->st));
    GK(hipMemsetAsync(err, 0, bytes, s->st));
    enqueue_mul(g, everyone(g), corr, Sink{err, nullptr, nullptr, nullptr}, &launches);
    GK(hipMemcpyAsync(out, err, bytes, hipMemcpyDeviceToHost, s->st));
    GK(hipStreamSynchronize(s->st));
    GK(hipGetLastError());
    return CALIPSO_OK;
}

int32_t calipso_hip_sparse_kkt_group_solve_symmetric(calipso_hip_sparse_kkt_group* g, const double* residual, double* step) {
    static const char* const entry = "calipso_hip_sparse_kkt_group_solve_symmetric";
    if (!g) return CALIPSO_ERR_ARGUMENT;
    GREFUSE(grp::check_required(entry, "residual", residual)); GREFUSE(grp::check_required(entry, "step", step));
    if (!g->factored) return gfail(g, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": factorize first");
    KH* s = g->base;
    GK(hipSetDevice(s->device));
    const size_t bytes = sizeof(double) * (size_t)s->d.N * (size_t)g->members;
    double* res = arr(g, grp::A_RES); double* stp = arr(g, grp::A_STEP);
    int launches = 0;
    GK(hipMemcpyAsync(res, residual, bytes, hipMemcpyHostToDevice, s->st));
    if (const int rc = enqueue_solve(g, everyone(g), res, stp, &launches); rc < 0) return rc;
    GK(hipMemcpyAsync(step, stp, bytes, hipMemcpyDeviceToHost, s->st));
    GK(hipStreamSynchronize(s->st));
    GK(hipGetLastError());
    return CALIPSO_OK;
}

int32_t calipso_hip_sparse_kkt_group_search_direction(calipso_hip_sparse_kkt_group* g, const double* residual, double* step, double* regularization, double* info, int32_t* status, double report[8]) {
    return search_direction_entry(g, "calipso_hip_sparse_kkt_group_search_direction", residual, step, regularization, info, status, report, false);
}
int32_t calipso_hip_sparse_kkt_group_search_direction_device(calipso_hip_sparse_kkt_group* g, const double* residual, double* step, double* regularization, double* info, int32_t* status, double report[8]) {
    return search_direction_entry(g, "calipso_hip_sparse_kkt_group_search_direction_device", residual, step, regularization, info, status, report, true);
}

int32_t calipso_hip_sparse_kkt_group_timing(calipso_hip_sparse_kkt_group* g, double ms[8]) {
    if (!g || !ms) return CALIPSO_ERR_ARGUMENT;
    std::copy(g->ms, g->ms + 8, ms);
    return CALIPSO_OK;
}

}  // extern "C"
