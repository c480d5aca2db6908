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
    size_t cap_P = 0, cap_q = 0, cap_Z = 0, cap_bh = 0;                  // their capacities in doubles (set_qp_device grows them on demand and keeps them)
    double *w = nullptr, *lam = nullptr, *sc = nullptr, *filt = nullptr, *info = nullptr, *trace = nullptr, *prof = nullptr;
    double *rtheta = nullptr, *sens = nullptr, *stf = nullptr; size_t cap_diff = 0; bool diff_shared = false;      // differentiate!: batch x N x p each
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

namespace calipso {
namespace snh {
typedef calipso_hip_smallnewton SN;
int fail(SN* s, int code, const std::string& msg);
sn::Dm dims_of(const SN* s);
// one launch of the batch kernel on the handle's stream.  adj: MODE_ADJ's extra arguments (its `base` is filled by the launch).  enqueue_only: no events, no
// synchronisation, no timing (the device entries); else the launch is timed and waited for (the host entries)
int launch(SN* s, int mode, int count, int advance, bool eval_rtheta, const sn::AdjArgs* adj, bool enqueue_only);
// a device buffer of at least `need` doubles (grown, never shrunk)
int grow(SN* s, double** p, size_t* cap, size_t need, const char* who);
}  // namespace snh
}  // namespace calipso
