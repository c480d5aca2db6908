// smallnewton_handle.hpp — the handle of the one-launch batch kernel, shared by its host entries (smallnewton.hip) and its device-resident entries (smallnewton_io.hip)
#pragma once
#include <string>
#include <vector>

#include "internal.hpp"
#include "../../include/calipso_smallnewton.hpp"      // Dm, Lay, Args, the device code, QpEval

struct calipso_hip_smallnewton {
    int nx = 0, ne = 0, nc = 0, batch = 0, device = 0;
    int nq = 0; std::vector<int> soc_start, soc_dim, soc_woff; int wsz = 0, maxd = 0;      // cone layout: nq nonnegative entries, then the second-order cones (contiguous)
    int *d_soc = nullptr;                                                                   // device: [start | dim | woff], nsoc each
    calipso::Options opt;
    double objective_scale = 0.5;
    bool have_qp = false;
    calipso_smallnewton_kernels_fn ev = nullptr; int np = 0; bool ev_rtheta = false, ev_adj = false;      // set_evaluator: the user library's entry, parameters per instance, dR/dtheta provided, reverse mode built
    double *theta = nullptr, *hess = nullptr, *dpt = nullptr; bool theta_shared = false, have_theta = false;      // parameters (batch x np or one row), Lagrangian Hessians (batch x nx^2), the points they were evaluated at (batch x (nx + m))
    size_t cap_theta = 0;
    hipStream_t stream = nullptr;    // where the handle's work goes: own_stream, or the caller's (calipso_hip_smallnewton_set_stream: borrowed, never destroyed here)
    hipStream_t own_stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_order = nullptr;      // (ev_order: the new stream waits for what the old one holds when set_stream changes it)
    double *P = nullptr, *q = nullptr, *Z = nullptr, *bh = nullptr;      // Lxx = 2 c P (nx x nx), q, Z = [A; -G] (m x nx, ld m), bh = [-b; h]: per instance or shared
    long long sP = 0, sq = 0, sZ = 0, sbh = 0;                           // their element strides per instance (0: stored once for all)
    size_t cap_P = 0, cap_q = 0, cap_Z = 0, cap_bh = 0;                  // their capacities in doubles (pack_qp grows them on demand and keeps them)
    double *w = nullptr, *lam = nullptr, *sc = nullptr, *filt = nullptr, *info = nullptr, *trace = nullptr, *prof = nullptr;
    double *rtheta = nullptr, *sens = nullptr, *stf = nullptr; size_t cap_rtheta = 0, cap_sens = 0; bool diff_shared = false;      // differentiate!: batch x N x p each
    double* stage = nullptr; size_t cap_stage = 0;                                                                 // where the host set_state lands its arrays before put_state (batch x (N + ne + 3))
    double *adj_rt = nullptr, *adj_in = nullptr, *adj_out = nullptr, *adj_gth = nullptr, *adj_gqp = nullptr;      // reverse mode: dR/dtheta, cotangents, lambda, gradients
    size_t cap_adj_rt = 0, cap_adj_in = 0, cap_adj_out = 0, cap_adj_gth = 0, cap_adj_gqp = 0;                      // (their capacities in doubles, grown on demand)
    double* red = nullptr; size_t cap_red = 0;                                                                     // partial sums of the batch reduction of grad_qp (chunks x k x nqp)
    long long* cnt = nullptr; int* status = nullptr;
    int* solve_status = nullptr;     // status of the last solve! (a differentiate launch overwrites `status`): the device entries turn the gradients of status != 1 into NaN
    int trace_rows = 0;
    size_t lds_bytes = 0;
    int threads = 0;                 // options.threads: 0 = by the LDS footprint (sn_threads), 64 / 128 / 256 forced
    bool lu = false; double* Hs = nullptr;      // options.lu_fallback: H \ residual in the kernel, batch x N x N doubles of scratch for H and its factors
    double last_ms = 0.0;
    std::string err;
};

// (in a function that returns a code and has the handle `s`)
#define SK(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return calipso::snh::fail(s, CALIPSO_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); } while (0)

namespace calipso {
namespace snh {
typedef calipso_hip_smallnewton SN;
int fail(SN* s, int code, const std::string& msg);
sn::Dm dims_of(const SN* s);
// entries of P, q, A, b, G, h of one instance: a column of the adjoint kernel's grad_qp block
inline size_t qp_entries(const sn::Dm& d) { return (size_t)d.nx * d.nx + d.nx + (size_t)d.ne * d.nx + d.ne + (size_t)d.nc * d.nx + d.nc; }
// one launch of the batch kernel on the handle's stream.  adj: MODE_ADJ's extra arguments (its `base` is filled by the launch).  timed: between two events, waited
// for, last_ms set (the host entries); else enqueued only (the device entries)
int launch(SN* s, int mode, int count, int advance, bool eval_rtheta, const sn::AdjArgs* adj, bool timed);
// a device buffer of at least `need` doubles (grown, never shrunk)
int grow(SN* s, double** p, size_t* cap, size_t need, const char* who);
// The one data path (smallnewton_io.hip): device pointers in, everything enqueued on the handle's stream, no wait.  A device entry checks its pointers and calls;
// a host entry copies its arrays to the device, calls, waits and reads back.  src = {P, q, A, b, G, h}; w_mode 0: the points stay, 1: w, 2: initialize! from x0.
int pack_qp(SN* s, const double* const src[6], double objective_scale, int shared_mask, int row_major, const char* who);
int put_state(SN* s, const double* w, const double* x0, int w_mode, const double* lambda, const double* scalars);
int put_parameters(SN* s, const double* theta, int shared, hipMemcpyKind kind, const char* who);
// the reverse mode: its refusals (they need no buffer: asked before an entry sizes any), then grad_qp's block and dR/dtheta's buffer, AdjArgs and the launch
int adjoint_refusals(SN* s, int64_t k, bool have_cotangent, bool grad_theta, bool grad_qp);
int adjoint(SN* s, int64_t k, const double* cot, double* adjoint, double* grad_theta, bool want_grad_qp, bool timed);
}  // namespace snh
}  // namespace calipso
