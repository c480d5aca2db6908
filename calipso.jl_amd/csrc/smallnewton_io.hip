// smallnewton_io.hip — the ONE data path around the launches of the batch kernel (k_smallnewton / k_smallnewton_adj), and its device-resident, stream-ordered
// entries.  The cores (calipso::snh: pack_qp, put_state, put_parameters, adjoint) take device pointers, enqueue on the handle's stream (its own, or the caller's
// after calipso_hip_smallnewton_set_stream) and do not wait.  A *_device entry checks that its pointers are device memory of the handle's device and calls the
// core: NO device entry waits.  A host entry (smallnewton.hip) copies its arrays to the device, calls the same core, waits and reads back.  The kernels here:
//   k_sn_pack          the kernel's form of the QP — Lxx = (2c) P, Z = [A; -G] (ld m, column-major), bh = [-b; h]: one multiply (by 2c, rounded once on the host),
//                      two negations; per array shared or per instance, row- or column-major sources
//   k_sn_state         set_state / initialize!: the points, lambda, and the three scalars scattered into their SC_* slots
//   k_sn_gather        x, y, z out of the point.jl layout, the whole w, the status of the last solve
//   k_sn_cot           cotangent parts (x, y, z) into the N-layout the adjoint kernel reads, zeros elsewhere
//   k_sn_gqp_unpack    per-instance gradients of the QP's data out of the adjoint kernel's batch x (nqp x k) block, transposed for row-major callers
//   k_sn_gqp_partial / k_sn_gqp_final   gradients of shared data summed over the batch: the batch is cut into chunks of SN_RED_CHUNK instances (a constant: the sum
//                      does not depend on the grid or the device), a thread adds its element over the chunk in instance order, a second kernel adds the chunks in
//                      order.  No atomics; two runs give the same bits.  The first stage is the one HBM-bound kernel here (the block is read once, lanes along
//                      its contiguous index).
// Transposes put the lanes along the contiguous index of the destination; the strided side is a matrix of at most 128 x 128 doubles that one workgroup reads
// whole, so it is served by L2 / the vector cache after the first touch of each line.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "smallnewton_handle.hpp"
#include "device_utils.hpp"

namespace {
using namespace calipso::sn;
using namespace calipso::snh;

constexpr int IO_NT = 256;
constexpr int SN_RED_CHUNK = 64;      // instances per partial sum of the batch reduction: fixed, so the summation order is a function of the batch size alone

struct PackArgs {
    const double *P, *q, *A, *b, *G, *h; long long iP, iq, iA, ib, iG, ih;      // sources and their element strides per instance (0: one array for all)
    double *oP, *oq, *oZ, *obh; long long sP, sq, sZ, sbh;                      // destinations and theirs
    int nx, ne, nc, row_major; double two_c;
};

__global__ __launch_bounds__(IO_NT) void k_sn_pack(PackArgs a) {
    const size_t k = blockIdx.x;
    const int tid = threadIdx.x, nx = a.nx, ne = a.ne, nc = a.nc, m = ne + nc;
    if (a.sP != 0 || k == 0) {
        const double* src = a.P + k * (size_t)a.iP; double* dst = a.oP + k * (size_t)a.sP;
        for (int e = tid; e < nx * nx; e += IO_NT) { const int r = e % nx, c = e / nx; dst[e] = a.two_c * src[a.row_major ? r * nx + c : e]; }
    }
    if (a.sq != 0 || k == 0) {
        const double* src = a.q + k * (size_t)a.iq; double* dst = a.oq + k * (size_t)a.sq;
        for (int e = tid; e < nx; e += IO_NT) dst[e] = src[e];
    }
    if (m > 0 && (a.sZ != 0 || k == 0)) {
        const double* A = ne ? a.A + k * (size_t)a.iA : nullptr; const double* G = nc ? a.G + k * (size_t)a.iG : nullptr;
        double* dst = a.oZ + k * (size_t)a.sZ;
        for (int e = tid; e < m * nx; e += IO_NT) {
            const int r = e % m, c = e / m;
            dst[e] = r < ne ? A[a.row_major ? r * nx + c : r + c * ne] : -G[a.row_major ? (r - ne) * nx + c : (r - ne) + c * nc];
        }
    }
    if (m > 0 && (a.sbh != 0 || k == 0)) {
        const double* b = ne ? a.b + k * (size_t)a.ib : nullptr; const double* h = nc ? a.h + k * (size_t)a.ih : nullptr;
        double* dst = a.obh + k * (size_t)a.sbh;
        for (int e = tid; e < m; e += IO_NT) dst[e] = e < ne ? -b[e] : h[e - ne];
    }
}

struct StateArgs {
    const double *w_src, *x0, *lam_src, *sc_src; double *w, *lam, *sc;
    int N, nx, ne, batch, w_mode;      // w_mode: 0 leave the points, 1 copy w_src, 2 initialize! (x0 or zeros in the first nx entries, zeros behind)
};

__global__ __launch_bounds__(IO_NT) void k_sn_state(StateArgs a) {
    const size_t g = (size_t)blockIdx.x * IO_NT + threadIdx.x, step = (size_t)gridDim.x * IO_NT;
    const size_t B = (size_t)a.batch;
    if (a.w_mode == 1) for (size_t i = g; i < B * a.N; i += step) a.w[i] = a.w_src[i];
    if (a.w_mode == 2) for (size_t i = g; i < B * a.N; i += step) { const size_t k = i / a.N; const int j = (int)(i % a.N); a.w[i] = (a.x0 && j < a.nx) ? a.x0[k * a.nx + j] : 0.0; }
    if (a.lam_src) for (size_t i = g; i < B * a.ne; i += step) a.lam[i] = a.lam_src[i];
    if (a.sc_src) for (size_t i = g; i < B * 3; i += step) { const size_t k = i / 3; const int j = (int)(i % 3); a.sc[k * SC_COUNT + (j == 0 ? SC_KAPPA : j == 1 ? SC_TAU : SC_RHO)] = a.sc_src[i]; }
}

struct GatherArgs { const double* w; const int* st; double *x, *y, *z, *wout; int* status; int N, nx, ne, nc, batch; };

__global__ __launch_bounds__(IO_NT) void k_sn_gather(GatherArgs a) {
    const size_t g = (size_t)blockIdx.x * IO_NT + threadIdx.x, step = (size_t)gridDim.x * IO_NT;
    const size_t B = (size_t)a.batch;
    const int oy = a.nx + a.ne + a.nc, oz = oy + a.ne;
    for (size_t i = g; i < B * a.N; i += step) {
        const size_t k = i / a.N; const int j = (int)(i % a.N);
        const double v = a.w[i];
        if (a.wout) a.wout[i] = v;
        if (j < a.nx) { if (a.x) a.x[k * a.nx + j] = v; }
        else if (j >= oy && j < oy + a.ne) { if (a.y) a.y[k * a.ne + (j - oy)] = v; }
        else if (j >= oz && j < oz + a.nc) { if (a.z) a.z[k * a.nc + (j - oz)] = v; }
    }
    if (a.status) for (size_t i = g; i < B; i += step) a.status[i] = a.st[i];
}

struct CotArgs { const double *cx, *cy, *cz; double* out; int N, nx, ne, nc; long long rows; };      // rows = batch x k columns of N entries

__global__ __launch_bounds__(IO_NT) void k_sn_cot(CotArgs a) {
    const size_t g = (size_t)blockIdx.x * IO_NT + threadIdx.x, step = (size_t)gridDim.x * IO_NT;
    const int oy = a.nx + a.ne + a.nc, oz = oy + a.ne;
    for (size_t i = g; i < (size_t)a.rows * a.N; i += step) {
        const size_t r = i / a.N; const int j = (int)(i % a.N);
        double v = 0.0;
        if (j < a.nx) { if (a.cx) v = a.cx[r * a.nx + j]; }
        else if (j >= oy && j < oy + a.ne) { if (a.cy) v = a.cy[r * a.ne + (j - oy)]; }
        else if (j >= oz && j < oz + a.nc) { if (a.cz) v = a.cz[r * a.nc + (j - oz)]; }
        a.out[i] = v;
    }
}

// rows of `len` doubles of the instances whose solve status is not 1 become NaN (grad_theta, which the adjoint kernel writes straight into the caller's buffer)
__global__ __launch_bounds__(IO_NT) void k_sn_nan_rows(double* g, const int* st, long long len, int batch) {
    const size_t k = blockIdx.x;
    if (st[k] == 1) return;
    for (long long i = threadIdx.x; i < len; i += IO_NT) g[k * (size_t)len + i] = __builtin_nan("");
}

struct GqpArgs {
    const double* g; const int* st; double* part;
    double* out[6]; int off[6], rows[6], cols[6];      // array i: entries [off, off + rows * max(cols, 1)) of a column of the block; cols = 0: a vector
    int mask;                                           // bit i: array i is summed over the batch (the partial / final kernels take it), else per instance (unpack)
    int row_major, K, batch, nqp, nchunks, tblocks;
};

// entry e2 of the caller's layout of array i -> its entry in the block's column-major layout
__device__ inline int gqp_src(const GqpArgs& a, int i, int e2) {
    if (!a.row_major || a.cols[i] == 0) return e2;
    const int r = e2 / a.cols[i], c = e2 % a.cols[i];
    return r + c * a.rows[i];
}

__global__ __launch_bounds__(IO_NT) void k_sn_gqp_unpack(GqpArgs a) {
    const size_t bj = blockIdx.x;                       // (instance, cotangent column)
    const bool bad = a.st[bj / (size_t)a.K] != 1;
    const double* src = a.g + bj * (size_t)a.nqp;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        if (!a.out[i] || ((a.mask >> i) & 1)) continue;
        const int n = a.rows[i] * (a.cols[i] ? a.cols[i] : 1);
        double* dst = a.out[i] + bj * (size_t)n;
        for (int e2 = threadIdx.x; e2 < n; e2 += IO_NT) dst[e2] = bad ? __builtin_nan("") : src[a.off[i] + gqp_src(a, i, e2)];
    }
}

// part[chunk][t] = sum over the chunk's instances, in instance order, of entry t = (column j, entry e) of the block — NaN for an instance whose solve status is not 1
__global__ __launch_bounds__(IO_NT) void k_sn_gqp_partial(GqpArgs a) {
    const int c = blockIdx.x / a.tblocks, tb = blockIdx.x % a.tblocks;
    const long long T = (long long)a.K * a.nqp, t = (long long)tb * IO_NT + threadIdx.x;
    if (t >= T) return;
    const int e = (int)(t % a.nqp);
    bool take = false;
#pragma unroll
    for (int i = 0; i < 6; ++i) take = take || (a.out[i] && ((a.mask >> i) & 1) && e >= a.off[i] && e < a.off[i] + a.rows[i] * (a.cols[i] ? a.cols[i] : 1));
    if (!take) return;
    const int b0 = c * SN_RED_CHUNK, b1 = min(b0 + SN_RED_CHUNK, a.batch);
    double acc = 0.0;
    for (int b = b0; b < b1; b += 8) {                  // (eight loads in flight, added in instance order)
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = b + u < b1 ? a.g[(size_t)(b + u) * (size_t)T + (size_t)t] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) if (b + u < b1) acc += a.st[b + u] != 1 ? __builtin_nan("") : v[u];
    }
    a.part[(size_t)c * (size_t)T + (size_t)t] = acc;
}

// out_i[j][e2] = sum of the chunks' partial sums in chunk order
__global__ __launch_bounds__(IO_NT) void k_sn_gqp_final(GqpArgs a) {
    const size_t g = (size_t)blockIdx.x * IO_NT + threadIdx.x, step = (size_t)gridDim.x * IO_NT;
    const size_t T = (size_t)a.K * a.nqp;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        if (!a.out[i] || !((a.mask >> i) & 1)) continue;
        const int n = a.rows[i] * (a.cols[i] ? a.cols[i] : 1);
        for (size_t idx = g; idx < (size_t)a.K * n; idx += step) {
            const size_t j = idx / n; const int e2 = (int)(idx % n);
            const size_t t = j * a.nqp + a.off[i] + gqp_src(a, i, e2);
            double acc = 0.0;
            for (int c = 0; c < a.nchunks; ++c) acc += a.part[(size_t)c * T + t];
            a.out[i][idx] = acc;
        }
    }
}

unsigned blocks_for(size_t elements) { return (unsigned)std::min<size_t>(std::max<size_t>((elements + IO_NT - 1) / IO_NT, 1), 4096); }

// every non-NULL pointer of a device entry must be device memory of the handle's device: checked before anything is enqueued
int device_pointer(SN* s, const void* p, const char* entry, const char* arg) {
    if (!p) return CALIPSO_OK;
    hipPointerAttribute_t at;
    std::memset(&at, 0, sizeof(at));
    const hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(s, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": " + arg + " is not device memory (a host pointer?): the device entries take device pointers only");
    }
    if (at.type != hipMemoryTypeDevice) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": " + arg + " is not device memory: the device entries take device pointers only");
    if (at.device != s->device) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(entry) + ": " + arg + " lives on device " + std::to_string(at.device) + ", the handle on device " + std::to_string(s->device));
    return CALIPSO_OK;
}
#define DEVPTR(entry, p) do { const int rc__ = device_pointer(s, (const void*)(p), entry, #p); if (rc__ < 0) return rc__; } while (0)

}  // namespace

namespace calipso {
namespace snh {

int pack_qp(SN* s, const double* const src[6], double objective_scale, int shared_mask, int row_major, const char* who) {
    const size_t nx = s->nx, ne = s->ne, nc = s->nc, m = ne + nc, m1 = std::max<size_t>(m, 1), B = (size_t)s->batch;
    const auto sh = [&](int i) { return ((shared_mask >> i) & 1) != 0; };
    const bool zP = sh(0), zq = sh(1), zZ = (ne == 0 || sh(2)) && (nc == 0 || sh(4)), zbh = (ne == 0 || sh(3)) && (nc == 0 || sh(5));
    if (s->ev) {      // (replaces an evaluator: its buffers go — the one case that waits for the device)
        SK(hipStreamSynchronize(s->stream));
        for (double** p : {&s->theta, &s->hess, &s->dpt}) if (*p) { (void)hipFree(*p); *p = nullptr; }
        s->cap_theta = 0;
        s->ev = nullptr; s->np = 0; s->ev_rtheta = false; s->ev_adj = false; s->have_theta = false;
    }
    s->have_qp = false;
    int rc = grow(s, &s->P, &s->cap_P, (zP ? 1 : B) * nx * nx, who);
    if (rc == CALIPSO_OK) rc = grow(s, &s->q, &s->cap_q, (zq ? 1 : B) * nx, who);
    if (rc == CALIPSO_OK) rc = grow(s, &s->Z, &s->cap_Z, (zZ ? 1 : B) * m1 * nx, who);
    if (rc == CALIPSO_OK) rc = grow(s, &s->bh, &s->cap_bh, (zbh ? 1 : B) * m1, who);
    if (rc < 0) return rc;
    PackArgs a;
    std::memset(&a, 0, sizeof(a));
    a.P = src[0]; a.q = src[1]; a.A = src[2]; a.b = src[3]; a.G = src[4]; a.h = src[5];
    a.iP = sh(0) ? 0 : (long long)(nx * nx); a.iq = sh(1) ? 0 : (long long)nx; a.iA = sh(2) ? 0 : (long long)(ne * nx); a.ib = sh(3) ? 0 : (long long)ne;
    a.iG = sh(4) ? 0 : (long long)(nc * nx); a.ih = sh(5) ? 0 : (long long)nc;
    a.oP = s->P; a.oq = s->q; a.oZ = s->Z; a.obh = s->bh;
    a.sP = zP ? 0 : (long long)(nx * nx); a.sq = zq ? 0 : (long long)nx; a.sZ = zZ ? 0 : (long long)(m1 * nx); a.sbh = zbh ? 0 : (long long)m1;
    a.nx = s->nx; a.ne = s->ne; a.nc = s->nc; a.row_major = row_major != 0; a.two_c = 2.0 * objective_scale;
    const bool any = a.sP || a.sq || (m > 0 && (a.sZ || a.sbh));
    hipLaunchKernelGGL(k_sn_pack, dim3(any ? (unsigned)B : 1u), dim3(IO_NT), 0, s->stream, a);
    SK(hipGetLastError());
    s->sP = a.sP; s->sq = a.sq; s->sZ = a.sZ; s->sbh = a.sbh;
    s->have_qp = true; s->objective_scale = objective_scale;
    return CALIPSO_OK;
}

int put_state(SN* s, const double* w, const double* x0, int w_mode, const double* lambda, const double* scalars) {
    const Dm d = dims_of(s);
    StateArgs a;
    std::memset(&a, 0, sizeof(a));
    a.w_src = w; a.x0 = x0; a.lam_src = d.ne ? lambda : nullptr; a.sc_src = scalars; a.w = s->w; a.lam = s->lam; a.sc = s->sc;
    a.N = d.N; a.nx = d.nx; a.ne = d.ne; a.batch = s->batch; a.w_mode = w_mode;
    if (!w_mode && !a.lam_src && !a.sc_src) return CALIPSO_OK;
    hipLaunchKernelGGL(k_sn_state, dim3(blocks_for((size_t)s->batch * d.N)), dim3(IO_NT), 0, s->stream, a);
    SK(hipGetLastError());
    return CALIPSO_OK;
}

int put_parameters(SN* s, const double* theta, int shared, hipMemcpyKind kind, const char* who) {
    if (!s->ev) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(who) + ": no evaluator (calipso_hip_smallnewton_set_evaluator)");
    if (s->np == 0) return CALIPSO_OK;
    const size_t n = (size_t)s->np * (shared ? 1 : (size_t)s->batch);
    { const int rc = grow(s, &s->theta, &s->cap_theta, n, who); if (rc < 0) return rc; }
    SK(hipMemcpyAsync(s->theta, theta, sizeof(double) * n, kind, s->stream));
    s->theta_shared = shared != 0; s->have_theta = true;
    return CALIPSO_OK;
}

// (the messages name the host entry, whichever entry asked)
int adjoint_refusals(SN* s, int64_t k, bool have_cotangent, bool grad_theta, bool grad_qp) {
    const std::string me = "calipso_hip_smallnewton_differentiate_adjoint: ";
    if (k < 1 || k > (1 << 20)) return fail(s, CALIPSO_ERR_ARGUMENT, me + "k >= 1 cotangent columns");
    if (!have_cotangent) return fail(s, CALIPSO_ERR_ARGUMENT, me + "no cotangent");
    if (!s->have_qp && !s->ev) return fail(s, CALIPSO_ERR_ARGUMENT, me + "no problem data (calipso_hip_smallnewton_set_qp or calipso_hip_smallnewton_set_evaluator)");
    if (s->ev && !s->ev_adj) return fail(s, CALIPSO_ERR_ARGUMENT, me + "the evaluator's entry was built without the reverse mode: rebuild it against the current include/calipso_smallnewton.hpp");
    if (grad_theta && (!s->ev || !s->ev_rtheta || s->np < 1)) return fail(s, CALIPSO_ERR_ARGUMENT, me + "grad_theta needs an evaluator that provides dR/dtheta and has parameters");
    if (grad_qp && s->ev) return fail(s, CALIPSO_ERR_ARGUMENT, me + "grad_qp is for the built-in QP (set_qp), not an evaluator");
    return CALIPSO_OK;
}

int adjoint(SN* s, int64_t k, const double* cot, double* adjoint, double* grad_theta, bool want_grad_qp, bool timed) {
    const char* me = "calipso_hip_smallnewton_differentiate_adjoint";
    const Dm d = dims_of(s);
    const size_t B = (size_t)s->batch;
    int rc = CALIPSO_OK;
    if (grad_theta) rc = grow(s, &s->adj_rt, &s->cap_adj_rt, B * (size_t)d.N * (size_t)s->np, me);
    if (rc == CALIPSO_OK && want_grad_qp) rc = grow(s, &s->adj_gqp, &s->cap_adj_gqp, B * (size_t)k * qp_entries(d), me);
    if (rc < 0) return rc;
    AdjArgs aa;
    std::memset(&aa, 0, sizeof(aa));
    aa.cot = cot; aa.adjoint = adjoint; aa.grad_theta = grad_theta; aa.grad_qp = want_grad_qp ? s->adj_gqp : nullptr;
    aa.objective_scale = s->objective_scale; aa.k = (int)k;
    return launch(s, MODE_ADJ, grad_theta ? s->np : 0, 0, grad_theta != nullptr, &aa, timed);
}

}  // namespace snh
}  // namespace calipso

extern "C" {

// All later work of the handle goes to the caller's stream (borrow != 0; hip_stream may be NULL: the legacy default stream, which is torch's default stream) or back
// to the handle's own (borrow == 0).  The new stream first waits, on the device, for what the old one still holds: an event is recorded on the OLD stream here, so
// a borrowed stream must still exist when the handle is taken off it (include/calipso_hip.h: set_stream before destroying it).  It is never destroyed here.
int32_t calipso_hip_smallnewton_set_stream(calipso_hip_smallnewton* s, void* hip_stream, int32_t borrow) {
    if (!s) return CALIPSO_ERR_ARGUMENT;
    const hipStream_t ns = borrow ? (hipStream_t)hip_stream : s->own_stream;
    if (ns == s->stream) return CALIPSO_OK;
    SK(hipSetDevice(s->device));
    SK(hipEventRecord(s->ev_order, s->stream));
    SK(hipStreamWaitEvent(ns, s->ev_order, 0));
    s->stream = ns;
    return CALIPSO_OK;
}

// set_qp with the arrays on the device.  Bit i of shared_mask: array i of P, q, A, b, G, h is ONE array for all instances; row_major != 0: matrices as
// (rows, cols) row-major (torch), else column-major as set_qp takes them.  P and q are stored once when shared; Z = [A; -G] once only when A and G are both shared
// (or absent), bh = [-b; h] likewise for b and h — otherwise the shared half is written into every instance's copy.  Buffers grow on demand and are kept.
int32_t calipso_hip_smallnewton_set_qp_device(calipso_hip_smallnewton* s, const double* P, const double* q, const double* A, const double* b, const double* G, const double* h,
                                              double objective_scale, int32_t shared_mask, int32_t row_major) {
    if (!s) return CALIPSO_ERR_ARGUMENT;
    const char* me = "calipso_hip_smallnewton_set_qp_device";
    if (!P || !q || (s->ne && (!A || !b)) || (s->nc && (!G || !h))) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(me) + ": P, q and, for ne > 0, A, b and, for nc > 0, G, h are required");
    if (shared_mask < 0 || shared_mask > 63) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(me) + ": shared_mask has one bit per array of P, q, A, b, G, h (0 .. 63)");
    SK(hipSetDevice(s->device));
    DEVPTR(me, P); DEVPTR(me, q); DEVPTR(me, A); DEVPTR(me, b); DEVPTR(me, G); DEVPTR(me, h);
    const double* src[6] = {P, q, A, b, G, h};
    return pack_qp(s, src, objective_scale, shared_mask, row_major, me);
}

// initialize!(solver, guess) for every instance: x0 (batch x nx) in the first nx entries of the points, zeros behind; x0 = NULL: zeros (what set_state does with such points)
int32_t calipso_hip_smallnewton_initialize_device(calipso_hip_smallnewton* s, const double* x0) {
    if (!s) return CALIPSO_ERR_ARGUMENT;
    SK(hipSetDevice(s->device));
    DEVPTR("calipso_hip_smallnewton_initialize_device", x0);
    return put_state(s, nullptr, x0, 2, nullptr, nullptr);
}

// set_state with the arrays on the device, the same layouts: w batch x N, lambda batch x ne, scalars batch x 3; NULL leaves what is resident
int32_t calipso_hip_smallnewton_set_state_device(calipso_hip_smallnewton* s, const double* w, const double* lambda, const double* scalars) {
    if (!s) return CALIPSO_ERR_ARGUMENT;
    const char* me = "calipso_hip_smallnewton_set_state_device";
    SK(hipSetDevice(s->device));
    DEVPTR(me, w); DEVPTR(me, lambda); DEVPTR(me, scalars);
    return put_state(s, w, nullptr, w ? 1 : 0, lambda, scalars);
}

// set_parameters with theta on the device: copied (device to device, on the stream) into the handle's buffer, which is kept while the size repeats
int32_t calipso_hip_smallnewton_set_parameters_device(calipso_hip_smallnewton* s, const double* theta, int32_t shared) {
    if (!s || !theta) return CALIPSO_ERR_ARGUMENT;
    SK(hipSetDevice(s->device));
    if (s->ev && s->np > 0) DEVPTR("calipso_hip_smallnewton_set_parameters_device", theta);
    return put_parameters(s, theta, shared, hipMemcpyDeviceToDevice, "calipso_hip_smallnewton_set_parameters_device");
}

// the launch of calipso_hip_smallnewton_solve, enqueued: no events, no wait, no status read back (get_solution_device hands it out on the device)
int32_t calipso_hip_smallnewton_solve_device(calipso_hip_smallnewton* s) {
    if (!s) return CALIPSO_ERR_ARGUMENT;
    return launch(s, MODE_SOLVE, 0, 1, false, nullptr, false);
}

// x (batch x nx), y (batch x ne), z (batch x nc) out of the resident points, the points themselves (batch x N), the status of the last solve (batch, int32): NULLs skipped
int32_t calipso_hip_smallnewton_get_solution_device(calipso_hip_smallnewton* s, double* x, double* y, double* z, double* w, int32_t* status) {
    if (!s) return CALIPSO_ERR_ARGUMENT;
    const char* me = "calipso_hip_smallnewton_get_solution_device";
    SK(hipSetDevice(s->device));
    DEVPTR(me, x); DEVPTR(me, y); DEVPTR(me, z); DEVPTR(me, w); DEVPTR(me, status);
    const Dm d = dims_of(s);
    GatherArgs a;
    std::memset(&a, 0, sizeof(a));
    a.w = s->w; a.st = s->solve_status; a.x = x; a.y = d.ne ? y : nullptr; a.z = d.nc ? z : nullptr; a.wout = w; a.status = status;
    a.N = d.N; a.nx = d.nx; a.ne = d.ne; a.nc = d.nc; a.batch = s->batch;
    if (!a.x && !a.y && !a.z && !a.wout && !a.status) return CALIPSO_OK;
    hipLaunchKernelGGL(k_sn_gather, dim3(blocks_for((size_t)s->batch * d.N)), dim3(IO_NT), 0, s->stream, a);
    SK(hipGetLastError());
    return CALIPSO_OK;
}

// differentiate_adjoint with everything on the device (the same launch of k_smallnewton_adj).  The cotangent: cot_w, batch x (N x k), read by the kernel where it
// lies — or the parts cot_x / cot_y / cot_z (batch x (nx | ne | nc) x k, each may be NULL), scattered into the N-layout.  adjoint and grad_theta are written by
// the launch into the caller's buffers.  grad_qp: NULL, or six pointers (P, q, A, b, G, h; NULLs skipped): without bit i of reduce_mask array i's gradient per
// instance, batch x k x size (matrices row-major when row_major != 0, else column-major); with it, summed over the batch on the device: k x size.  Every gradient
// (grad_qp, grad_theta) of an instance whose last SOLVE status is not 1 is NaN, before any sum.  status: as differentiate_adjoint (batch, int32; NULL: skipped).
int32_t calipso_hip_smallnewton_differentiate_adjoint_device(calipso_hip_smallnewton* s, int64_t k, const double* cot_w, const double* cot_x, const double* cot_y, const double* cot_z,
                                                             double* adjoint, double* grad_theta, double* const* grad_qp, int32_t reduce_mask, int32_t row_major, int32_t* status) {
    if (!s) return CALIPSO_ERR_ARGUMENT;
    const char* dev = "calipso_hip_smallnewton_differentiate_adjoint_device";
    { const int rc = adjoint_refusals(s, k, cot_w || cot_x || cot_y || cot_z, grad_theta != nullptr, grad_qp != nullptr); if (rc < 0) return rc; }
    if (reduce_mask < 0 || reduce_mask > 63) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(dev) + ": reduce_mask has one bit per array of P, q, A, b, G, h (0 .. 63)");
    SK(hipSetDevice(s->device));
    DEVPTR(dev, cot_w); DEVPTR(dev, cot_x); DEVPTR(dev, cot_y); DEVPTR(dev, cot_z); DEVPTR(dev, adjoint); DEVPTR(dev, grad_theta); DEVPTR(dev, status);
    const Dm d = dims_of(s);
    const size_t B = (size_t)s->batch, N = (size_t)d.N, K = (size_t)k;
    const size_t nqp = qp_entries(d);
    GqpArgs ga;
    std::memset(&ga, 0, sizeof(ga));
    bool any_qp = false, any_red = false, any_per = false;
    if (grad_qp) {
        static const char* names[6] = {"grad_qp[0] (P)", "grad_qp[1] (q)", "grad_qp[2] (A)", "grad_qp[3] (b)", "grad_qp[4] (G)", "grad_qp[5] (h)"};
        const int rows[6] = {d.nx, d.nx, d.ne, d.ne, d.nc, d.nc}, cols[6] = {d.nx, 0, d.nx, 0, d.nx, 0};
        int at = 0;
        for (int i = 0; i < 6; ++i) {
            ga.rows[i] = rows[i]; ga.cols[i] = cols[i]; ga.off[i] = at; at += rows[i] * (cols[i] ? cols[i] : 1);
            ga.out[i] = rows[i] > 0 ? grad_qp[i] : nullptr;
            { const int rc = device_pointer(s, ga.out[i], dev, names[i]); if (rc < 0) return rc; }
            if (ga.out[i]) { any_qp = true; if ((reduce_mask >> i) & 1) any_red = true; else any_per = true; }
        }
    }
    if (B * K > 0x7fffffffull) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(dev) + ": batch x k exceeds a launch grid");
    const size_t nchunks = (B + SN_RED_CHUNK - 1) / SN_RED_CHUNK, tblocks = (K * nqp + IO_NT - 1) / IO_NT;
    if (any_red && nchunks * tblocks > 0x7fffffffull) return fail(s, CALIPSO_ERR_ARGUMENT, std::string(dev) + ": the batch reduction exceeds a launch grid");
    int rc = CALIPSO_OK;
    if (!cot_w) rc = grow(s, &s->adj_in, &s->cap_adj_in, B * N * K, dev);
    if (rc == CALIPSO_OK && any_red) rc = grow(s, &s->red, &s->cap_red, nchunks * K * nqp, dev);
    if (rc < 0) return rc;
    if (!cot_w) {
        CotArgs ca;
        std::memset(&ca, 0, sizeof(ca));
        ca.cx = cot_x; ca.cy = d.ne ? cot_y : nullptr; ca.cz = d.nc ? cot_z : nullptr; ca.out = s->adj_in; ca.N = d.N; ca.nx = d.nx; ca.ne = d.ne; ca.nc = d.nc; ca.rows = (long long)(B * K);
        hipLaunchKernelGGL(k_sn_cot, dim3(blocks_for(B * K * N)), dim3(IO_NT), 0, s->stream, ca);
        SK(hipGetLastError());
    }
    rc = calipso::snh::adjoint(s, k, cot_w ? cot_w : s->adj_in, adjoint, grad_theta, any_qp, false);
    if (rc < 0) return rc;
    if (grad_theta) {
        hipLaunchKernelGGL(k_sn_nan_rows, dim3((unsigned)B), dim3(IO_NT), 0, s->stream, grad_theta, (const int*)s->solve_status, (long long)(K * (size_t)s->np), s->batch);
        SK(hipGetLastError());
    }
    if (any_qp) {
        ga.g = s->adj_gqp; ga.st = s->solve_status; ga.part = s->red; ga.mask = reduce_mask; ga.row_major = row_major != 0; ga.K = (int)k; ga.batch = s->batch; ga.nqp = (int)nqp;
        ga.nchunks = (int)nchunks; ga.tblocks = (int)tblocks;
        if (any_per) { hipLaunchKernelGGL(k_sn_gqp_unpack, dim3((unsigned)(B * K)), dim3(IO_NT), 0, s->stream, ga); SK(hipGetLastError()); }
        if (any_red) {
            hipLaunchKernelGGL(k_sn_gqp_partial, dim3((unsigned)(nchunks * tblocks)), dim3(IO_NT), 0, s->stream, ga); SK(hipGetLastError());
            hipLaunchKernelGGL(k_sn_gqp_final, dim3(blocks_for(K * nqp)), dim3(IO_NT), 0, s->stream, ga); SK(hipGetLastError());
        }
    }
    if (status) SK(hipMemcpyAsync(status, s->status, sizeof(int) * B, hipMemcpyDeviceToDevice, s->stream));
    return CALIPSO_OK;
}

// out = {addresses of Lxx, q, Z, bh; their element strides per instance}: what tests read to see that a repeated set_qp / set_qp_device keeps its buffers and which arrays are stored once
int32_t calipso_hip_debug_smallnewton_buffers(calipso_hip_smallnewton* s, int64_t out[8]) {
    if (!s || !out) return CALIPSO_ERR_ARGUMENT;
    out[0] = (int64_t)(uintptr_t)s->P; out[1] = (int64_t)(uintptr_t)s->q; out[2] = (int64_t)(uintptr_t)s->Z; out[3] = (int64_t)(uintptr_t)s->bh;
    out[4] = s->sP; out[5] = s->sq; out[6] = s->sZ; out[7] = s->sbh;
    return CALIPSO_OK;
}

}  // extern "C"
