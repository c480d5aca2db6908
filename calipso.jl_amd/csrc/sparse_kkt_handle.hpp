// sparse_kkt_handle.hpp — the handle behind calipso_hip_sparse_kkt_* as the translation units that work on it see it: sparse_kkt.hip (search_direction!),
// sparse_solve.hip (the vector half of solve! and its driver), sparse_differentiate.hip (differentiate!) and sparse_krylov.hip.  What every kernel reads (KktDev), the
// handle itself, the first lines of every entry (enter) and what the units call of each other.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "internal.hpp"
#include "device_memory.hpp"               // the one owner of the handle's device memory: device_fixed, device_upload, device_grown
#include "sparse_kkt.hpp"                  // the analysis: plain host C++
#include "sparse_krylov.hpp"               // the `H \ residual` fallback's options, workspace layout and Hessenberg cycle: plain host C++

namespace calipso {
namespace sparse_kkt {

constexpr int KT = 256;                    // threads per workgroup of every kernel on this handle

struct View { const int *ptr, *idx, *src; };      // a row view (idx = column, src = position in the caller's nzval) or a column view (idx = row, src unused)

// what every kernel reads: sizes, the point's offsets (point.jl:13-22), the resident data and the tables of the analysis
struct KktDev {
    int nx, ne, nc, n, N, q, nsoc, ncc;           // q = nonnegative rows, ncc = cone columns (sum of the dimensions)
    int o_r, o_s, o_y, o_z, o_t;
    int nnzL, nnzg, nnzh;
    const double *Lxx, *gx, *hx, *w, *rho;
    const int *slotL, *slotg, *sloth;             // slotL: -1 for the strict lower triangle AND for the diagonal (diag_x_src carries that one)
    const int *diag_x, *diag_x_src, *diag_e, *diag_c;
    const int *row_cone;                          // per cone row: its second-order cone, -1 nonnegative, -2 in no cone
    const int *soc_start, *soc_dim, *col_cone, *col_index, *col_slot;
    View Lr, gr, hr, gc, hc;
    View Lc;                                      // the column view of Lxx: Lxx' v, and the (row, column) of a stored non-zero (sparse_differentiate.hip)
};

// the parameter Jacobians on their stored patterns (sparse_parameters.hpp) as the kernels of sparse_differentiate.hip read them: 0-based device copies of the three
// CSC patterns (Lx,theta: nx rows; g,theta: ne rows; h,theta: nc rows; np columns each), the resident values, the parameters a wavefront sums
struct ParamDev {
    int np, n_long;
    long long long0;                              // first item of the wavefront section of the gradient kernel (sparse_parameters.hpp: Geometry)
    const int *ptr[3], *idx[3];
    const double* val[3];
    const int* long_columns;
};
using calipso::Grown;                             // device_memory.hpp: a buffer that grows on demand, is never shrunk and is kept
using calipso::device_fixed;
using calipso::device_upload;
using calipso::device_grown;

// set_parameter_patterns (sparse_solve.hip) fills it; set_evaluator and qp_attach drop it
struct ParameterPatterns {
    bool set = false;
    ParamDev d{};
    Grown<double> val[3];                         // the resident values; kept when the patterns are dropped and taken again by the next call, as are
    Grown<int> ints[7];                           // (ptr, idx) x 3 and the long columns on the device
    long long nnz[3] = {0, 0, 0}, longest = 0;
    std::vector<int64_t> host[6];                 // the HOST copies the evaluator is given: 1-based, (colptr, rowval) of Lp, gp, hp
};

struct SolveState;                                // sparse_solve.hip: the resident vectors, workspace and counters of solve!
struct DiffState;                                 // sparse_differentiate.hip: the column workspace and reports of differentiate!

}  // namespace sparse_kkt
}  // namespace calipso

struct calipso_hip_sparse_kkt {
    calipso::sparse_kkt::Analysis an;
    calipso::Options opt;
    calipso::Scalars sc;                       // kappa (IC-2), ep / ed of the last assemble, ep_last; tau and rho of a solve
    int device = 0;
    calipso_hip_sparse* sp = nullptr;          // LDL^T of the pattern of triu(K); its stream orders everything here
    hipStream_t st = nullptr;
    calipso::sparse_kkt::KktDev d{};
    bool wave_rows = false;
    double *Lxx = nullptr, *gx = nullptr, *hx = nullptr, *w = nullptr, *rho = nullptr, *K = nullptr;
    double *res = nullptr, *step = nullptr, *corr = nullptr, *err = nullptr, *rsym = nullptr, *dsym = nullptr, *norm = nullptr;
    std::vector<void*> dev;                    // every device allocation of the handle (device_fixed, device_grown): freed with it
    std::vector<void*>& device_allocations() { return dev; }                                  // what device_memory.hpp asks of a handle
    hipStream_t device_stream() const { return st; }
    int device_error(const std::string& text) { err_text = text; return CALIPSO_ERR_HIP; }
    bool have[5] = {false, false, false, false, false};      // Lxx, gx, hx, w, penalty resident
    bool assembled = false, factored = false;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::string err_text;
    calipso::sparse_kkt::SolveState* solve = nullptr;        // made by the first solve entry that needs it (sparse_solve.hip), released with the handle
    bool continue_after_refinement_failure = false;
    calipso::sparse_kkt::DiffState* diff = nullptr;          // made by the first differentiate entry (sparse_differentiate.hip), released with the handle
    double* dslack = nullptr;                                // s, then t (2 nc) as the last search_direction of a solve! was assembled at (quirk B-12)
    bool slacks_kept = false;                                // false: the differentiate slacks are the resident point's own
    bool differentiate_refinement = false;
    bool qp_attached = false;                                // q, b, hvec resident (qp_attach): what the data gradients ask for
    calipso::sparse_krylov::KrylovOptions kry;               // krylov_fallback, krylov_restart, krylov_max_cycles
    calipso::sparse_krylov::FallbackReport fallback;         // what calipso_hip_sparse_kkt_fallback_info reports
    calipso::sparse_kkt::Grown<double> kry_ws;               // the fallback's workspace (sparse_krylov.hpp: Layout), reserved on the first fallback and kept
    hipEvent_t kry_ev[2] = {nullptr, nullptr};
    calipso::sparse_kkt::ParameterPatterns par;              // the stored patterns and resident values of dR/dtheta (set_parameter_patterns)
};

namespace calipso {
namespace sparse_kkt {

typedef calipso_hip_sparse_kkt KH;

// sparse_kkt.hip, for the other units
int fail(KH* s, int rc, const std::string& text);                                                           // sets last_error, returns rc
int device_pointer(KH* s, const void* p, const char* entry, const char* arg);                               // the check of every _device entry
int search_direction(KH* s, const double* res, double* step, double regularization[3], double info[4]);
int create_tables(KH* s, int32_t method, const int64_t* perm);                                              // the plan of triu(K), stream, events, the analysis tables on the device (also the group's)
int values_missing(KH* s, const char* entry);                                                               // Lxx, gx, hx, w, penalty resident, or the refusal
int assemble_factorize(KH* s, const KktDev& d, double ep, double ed, int64_t inertia[3]);                    // one assemble from `d` (the handle's, or with other slacks) + factorisation
// OUT = M V (transposed: M' V) for k columns on the device: the "pre" launch, ONE k-column LDL^T solve, the "post" launch; `around`: two events recorded around them
int map_columns(KH* s, const KktDev& d, bool transposed, int k, const double* V, double* rsym, double* dsym, double* OUT, const hipEvent_t* around = nullptr);
// the first lines of an entry: the handle, its device and, by `need`, the solve state and what must be resident — or the refusal, under the entry's name
enum Need { HANDLE, VALUES, STATE, STATE_READY, STATE_POINT };      // VALUES: values_missing; STATE: the solve state; _READY: + the problem's data; _POINT: + a point and the penalty
int enter(KH* s, const char* entry, Need need);

#define KK(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return fail(s, CALIPSO_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); } while (0)
#define REFUSE(text) do { const std::string t__ = (text); if (!t__.empty()) return fail(s, CALIPSO_ERR_ARGUMENT, t__); } while (0)
#define ENTER(need) do { const int rc__ = enter(s, entry, need); if (rc__ < 0) return rc__; } while (0)      // (`entry`: the entry's name)
// in the one body of a host / _device pair of entries (`device`: which of the two)
#define DEVPTR(p) do { if (device) { const int rc__ = device_pointer(s, (const void*)(p), entry, #p); if (rc__ < 0) return rc__; } } while (0)

// sparse_solve.hip, for sparse_kkt.hip
int solve_state(KH* s);                                                                                     // the resident vectors of solve!: made by the first entry that needs them
int solve_ready(KH* s, const char* entry, bool point);                                                      // what a solve entry needs resident before it enqueues anything, or the refusal
void solve_state_release(calipso_hip_sparse_kkt* s);
int solve_set_option(calipso_hip_sparse_kkt* s, const char* name, double value);                            // 1 taken, 0 unknown, < 0 refused
int parameters_enqueue(calipso_hip_sparse_kkt* s, const char* entry);                                       // enqueue: the evaluator's five parameter bits at the resident point into s->par (no host wait), or the refusal
void diff_keep_slacks(calipso_hip_sparse_kkt* s);                                                           // enqueue: dslack <- the resident s, t (no host wait)
// sparse_krylov.hip, for sparse_kkt.hip: the fallback's vector kernels on the workspace `ws` laid out by `l` (enqueues, no host wait)
void krylov_enqueue_dots(hipStream_t st, const sparse_krylov::Layout& l, double* ws, int nv, const double* w);                  // partials of V[:, 0..nv)' w
void krylov_enqueue_update(hipStream_t st, const sparse_krylov::Layout& l, double* ws, int nv, const double* src, double* dst, bool accumulate, bool norm);
void krylov_enqueue_norm_scale(hipStream_t st, const sparse_krylov::Layout& l, double* ws, int slot, double* v);                // coef[slot] = |v|_2, v <- v / |v|_2
void krylov_enqueue_combine(hipStream_t st, const sparse_krylov::Layout& l, double* ws, int nv, const double* y, double* x);     // x <- x + Z[:, 0..nv) y
// sparse_differentiate.hip, for sparse_kkt.hip
void diff_state_release(calipso_hip_sparse_kkt* s);
int diff_set_option(calipso_hip_sparse_kkt* s, const char* name, double value);                             // 1 taken, 0 unknown, < 0 refused

}  // namespace sparse_kkt
}  // namespace calipso
