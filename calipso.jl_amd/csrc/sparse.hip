// sparse.hip — sparse LDL^T on the device for the LinearSolver seam: what the reference does with its vendored QDLDL
// (src/solver/qdldl.jl:134-188 analyse, :400-589 factor, :330-351,592-640 solve) for a sparse symmetric quasi-definite matrix, WITHOUT the dense
// n x n storage of ldlsolver.hip: memory is O(nnz(L)).
//
//   analyse (host, once per pattern)   order (ordering.hip: natural / RCM / minimum degree / nested dissection / the caller's), P A P' as a
//                                      LOWER CSC with a gather map from the caller's nzval, elimination tree, the row-sorted pattern of L, its
//                                      row view (which columns k < j update column j), and the LEVELS of the tree: level(j) = 1 + max level of
//                                      j's children.  Every column that updates column j lies in j's subtree, hence on a lower level.
//   factor  (device)                   left-looking by levels: one launch per level, one workgroup per column.  Column j is gathered into a
//                                      dense accumulator in LDS (n <= 20 000; global scratch beyond), the updates  w -= L(:,k) D_k L(j,k)  are
//                                      applied in ascending k (a fixed order: no atomics, bit-reproducible), then D_j = w_j, L(:,j) = w / D_j.
//                                      Runs of levels that hold a single column (the separators of a nested dissection, a dense tail) are
//                                      merged into ONE single-workgroup launch that walks the chain.  No pivoting (quasi-definite: any symmetric
//                                      order has an LDL^T, qdldl.jl:134-143); inertia from the signs of D, an exact zero pivot as qdldl.jl:456,579.
//   solve   (device)                   L y = b by levels (one wavefront per row, pull form over the row view), x = L^-T (y ./ D) by levels in
//                                      reverse (one wavefront per column); all right-hand sides of a call in the same launches.
// QDLDL is up-looking (row by row); the factor is unique, the summation order differs, so L and D agree with the oracle's restatement to
// rounding (tests/test_gpu_sparse.py: 1e-11 relative), not bit for bit.
#include <algorithm>
#include <numeric>
#include <string>
#include <utility>
#include <vector>

#include "internal.hpp"
#include "device_utils.hpp"
#include "device_memory.hpp"               // the one owner of the plan's device memory
#include "pivot16.hpp"
#include "ldl_device.hpp"
#include "sparse_plan.hpp"                 // the analyse phase and the records the kernels read: plain host C++

using calipso::i64;
using calipso::Grown;
using calipso::device_fixed;
using calipso::device_upload;
using calipso::device_grown;
using calipso::device_release;
using namespace calipso::sparse_plan;
static_assert(REFUSED_ARGUMENT == CALIPSO_ERR_ARGUMENT, "a refused pattern is an argument error");

namespace {

constexpr Limits LIMITS{};                 // what the kernels are built for; a plan is made under these and the two debug switches
constexpr int SP_THREADS = 256;
constexpr int SP_REC = 256;                // update records staged in LDS at a time
constexpr int SP_LDS_MAX_N = LIMITS.lds_max_n;

struct SpDev {
    int n;
    const int* order;                      // columns sorted by (level, index)
    const int *Alp, *Ali, *Asrc;           // P A P' lower CSC (diagonal included), Asrc = index into the caller's nzval
    const double* Aval;                    // the caller's nzval on the device
    const int *Lp, *Li;                    // strictly lower pattern of L, rows ascending
    double *Lx, *D;
    const int *Rp, *Rk, *Rpos, *Rend;      // row view: for row j the columns k < j with L(j,k) != 0 (ascending), the slot of L(j,k), the end of column k
    double* work;                          // global accumulators (gridDim.x x n) when n > SP_LDS_MAX_N
};

// barrier that orders the accumulator only: LDS traffic when the accumulator is in LDS (outstanding global PREFETCHES must not be waited for),
// everything otherwise
template <bool LDSW>
__device__ __forceinline__ void acc_barrier() {
    if (LDSW) { __builtin_amdgcn_s_waitcnt(0xc07f); __builtin_amdgcn_s_barrier(); }   // lgkmcnt(0)
    else __syncthreads();
}

template <bool LDSW>
__global__ __launch_bounds__(SP_THREADS) void k_sp_factor(SpDev d, int first, int ncols) {
    extern __shared__ __attribute__((aligned(16))) double wl[];
    __shared__ int rpos[SP_REC], rend[SP_REC];
    __shared__ double rf[SP_REC];
    double* w = LDSW ? wl : d.work + (size_t)blockIdx.x * d.n;
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < ncols; c += gridDim.x) {
        const int j = d.order[first + c];
        const int l0 = d.Lp[j], l1 = d.Lp[j + 1];
        for (int p = l0 + tid; p < l1; p += SP_THREADS) w[d.Li[p]] = 0.0;
        if (tid == 0) w[j] = 0.0;
        __syncthreads();
        for (int p = d.Alp[j] + tid; p < d.Alp[j + 1]; p += SP_THREADS) w[d.Ali[p]] = d.Aval[d.Asrc[p]];
        const int r0 = d.Rp[j], r1 = d.Rp[j + 1];
        __syncthreads();
        // The updates of column j are a dependent chain (they all touch w_j), one barrier each.  What must NOT be on that chain is global-memory
        // latency: the records (column k, slot of L(j,k), end of column k) and the factors L(j,k) D_k of up to SP_REC updates are staged in LDS
        // with one parallel load, and the first 256 (row, value) pairs of update q + 4 travel while update q is applied.
        for (int qc = r0; qc < r1; qc += SP_REC) {
            const int m = min(SP_REC, r1 - qc);
            if (tid < m) {
                const int k = d.Rk[qc + tid], pos = d.Rpos[qc + tid];
                rpos[tid] = pos; rend[tid] = d.Rend[qc + tid];
                rf[tid] = d.Lx[pos] * d.D[k];
            }
            __syncthreads();
            int li[4]; double lx[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                li[u] = 0; lx[u] = 0.0;
                if (u < m) { const int p = rpos[u] + tid; if (p < rend[u]) { li[u] = d.Li[p]; lx[u] = d.Lx[p]; } }
            }
            for (int q = 0; q < m; q += 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (q + u < m) {                                                        // (wave-uniform)
                        const int pos = rpos[q + u], end = rend[q + u];
                        const double f = rf[q + u];
                        const int cli = li[u]; const double clx = lx[u];
                        if (q + u + 4 < m) { const int p = rpos[q + u + 4] + tid; if (p < rend[q + u + 4]) { li[u] = d.Li[p]; lx[u] = d.Lx[p]; } }
                        if (pos + tid < end) w[cli] -= clx * f;                             // rows >= j of column k (the slot of L(j,k) is the first of them)
                        for (int p = pos + tid + SP_THREADS; p < end; p += SP_THREADS) w[d.Li[p]] -= d.Lx[p] * f;
                        acc_barrier<LDSW>();
                    }
                }
            }
            __syncthreads();                                                                // the record stage is refilled
        }
        const double dj = w[j];
        const double dinv = 1.0 / dj;                                               // L = y * Dinv as qdldl.jl:560-566
        for (int p = l0 + tid; p < l1; p += SP_THREADS) d.Lx[p] = w[d.Li[p]] * dinv;
        if (tid == 0) d.D[j] = dj;
        __syncthreads();                                                            // a chain's next column reads what this one wrote
    }
}

// forward substitution, rows of one level (or a chain, sequentially): x_j -= sum_k L(j,k) x_k.  One wavefront per row; blockIdx.y = right-hand side.
__global__ __launch_bounds__(64) void k_sp_forward(SpDev d, int first, int ncols, double* __restrict__ X) {
    double* x = X + (size_t)blockIdx.y * d.n;
    const int lane = threadIdx.x;
    for (int c = blockIdx.x; c < ncols; c += gridDim.x) {
        const int j = d.order[first + c];
        double acc = 0.0;
        for (int q = d.Rp[j] + lane; q < d.Rp[j + 1]; q += 64) acc += d.Lx[d.Rpos[q]] * x[d.Rk[q]];
        acc = calipso::wave_sum(acc);
        if (lane == 0) x[j] -= acc;
        __syncthreads();
    }
}
// backward substitution with the diagonal scaling folded in: x_j = y_j / D_j - sum_i L(i,j) x_i, levels (and chains) in reverse
__global__ __launch_bounds__(64) void k_sp_backward(SpDev d, int first, int ncols, double* __restrict__ X) {
    double* x = X + (size_t)blockIdx.y * d.n;
    const int lane = threadIdx.x;
    for (int c = blockIdx.x; c < ncols; c += gridDim.x) {
        const int j = d.order[first + ncols - 1 - c];
        double acc = 0.0;
        for (int p = d.Lp[j] + lane; p < d.Lp[j + 1]; p += 64) acc += d.Lx[p] * x[d.Li[p]];
        acc = calipso::wave_sum(acc);
        if (lane == 0) x[j] = x[j] / d.D[j] - acc;
        __syncthreads();
    }
}

// ---- multifrontal path (nested-dissection orders) ---------------------------------------------------------------------------------------------
// The pieces of the dissection (leaf pieces of <= 48 vertices, separators) are the SUPERNODES: node s owns the contiguous columns
// [first, first + c) and the rows R_s below them (r of them); its frontal matrix F_s (m = c + r) is assembled in the LDS of one workgroup from
// the entries of A in its columns and the update matrices U of its children (extend-add through precomputed relative indices, children in
// ascending order: fixed summation order), the first c columns are eliminated by a dense LDL^T in LDS (one barrier per pivot column), the
// m x c panel of L goes to global memory and U_s = F_s[c.., c..] to the node's slot of the update pool.  One launch per LEVEL of the node tree:
// for a T-stage trajectory problem that is ~log2 T launches for the whole factorisation — the stages are eliminated in parallel, level by level.
// (the records MfNode / MfChild / MfXItem / MfRowItem and the tables below are built on the host by sparse_plan.hpp)
struct MfDev {
    int nnodes;
    const MfNode* nrec;                       // [launch position]
    const MfChild* crec;                      // [chfirst + q], children in ascending order
    const int* order;                         // nodes sorted by level
    const int *nfirst, *ncols, *nrows;        // per node: first column, c, r
    const int *rowptr, *rows;                 // R_s (global, permuted row indices), ascending
    const int* rel;                           // per node, aligned with rows: local index of R_s[k] in the PARENT's front
    const int *childptr, *children;
    const long long *panel_off, *upd_off, *u_off;
    const int* Aloc;                          // per entry of the permuted lower CSC: offset inside its node's packed front (row (row + 1) / 2 + column)
    const int *Alp, *Asrc;
    const double* Aval;
    double *panel, *upd, *D, *uvec;
    double* fpool;                            // global-memory fronts (levels whose fronts exceed the LDS): packed lower triangles, per instance
    const long long* foff;                    // per node: offset of its front in fpool (levels reuse the pool)
    long long sPool;
    long long sA, sPanel, sUpd, sD;           // instance strides (batched factorisation of matrices with one pattern)
    // fronts factored by many workgroups (sparse_wide.hpp): per row of such a front (MfNode::pad0 + row) its entries of A and its child rows
    const int *wptrE, *wptrC;                 // [pad0 + row .. + 1]: ranges in wEcol / wEsrc and in wC
    const int *wEcol, *wEsrc;                 // local column in the front, index into Aval
    const MfRowItem* wC;                      // children in ascending order
    const MfXItem* xit;                       // extend-add items of the LDS fronts (nullptr: none)
    double* wscr;                             // X, M, L11, D of the diagonal blocks of one level: (matrix, node of the level)
};

// storage slot of launch instance z: z itself, or — for the members of a group's (shrinking) active set — slot[z].  A separate read-only kernel
// argument: indexing an array inside a struct the kernel also modifies would push the whole struct to scratch memory.
struct MfSlots { int use; int slot[calipso::MAX_BATCH]; };

typedef double calipso_v4d __attribute__((ext_vector_type(4)));
// threads per front: 256 for small fronts (several workgroups share a CU), 512 for fronts of more than Limits::big rows (one front fills the CU's LDS
// anyway; more waves shorten the panel, assembly and matrix-core phases).  The front limits (Limits::max_front, max_front_wide, max_front_global) are the plan's.
constexpr int MF_PY = LIMITS.py;              // row stride of the exchange rows of an in-register panel (pivot16.hpp)

// The front is symmetric: only its lower triangle is held, packed row by row (row i starts at i (i + 1) / 2), which lets fronts of up to 196 rows
// fit the 160 KiB of LDS (a full square would stop at 141).
// i (i + 1) / 2 for a row index below 4096 by the full-rate 24-bit multiply (a 32-bit integer multiply issues at a quarter of the rate, and the trailing
// update of a front is bound by exactly this index arithmetic)
__device__ __forceinline__ int tri0(int i) { return (int)(__umul24((unsigned)i, (unsigned)(i + 1)) >> 1); }
__device__ __forceinline__ int tri(int i, int k) { return tri0(i) + k; }     // i >= k

// Optional timeline of one front per level (build with -DCALIPSO_LDL_TRACE: `make trace`; bench/mf_trace.py reads it through calipso_hip_debug_mf_trace):
// 100 MHz wall-clock stamps of workgroup (0, 0) of every k_mf_factor launch, keyed by the launch's `first` node index.
#ifdef CALIPSO_LDL_TRACE
__device__ long long g_mf_trace[64 * 12];
__device__ int g_mf_trace_n;
#define MF_STAMP(slot) do { if (mf_traced && threadIdx.x == 0) { g_mf_trace[(mf_tr & 63) * 12 + (slot)] = wall_clock64(); if ((slot) == 0) g_mf_trace[(mf_tr & 63) * 12 + 6] = __builtin_readcyclecounter(); if ((slot) == 5) g_mf_trace[(mf_tr & 63) * 12 + 7] = __builtin_readcyclecounter(); } } while (0)   // ([6], [7]: the core clock's counter at the first and the last stamp)
// ... and of workgroup (0, 0) of the sweeps' launches (bench/mf_solve_trace.py, calipso_hip_debug_mfs_trace): [0 .. 5] stamps, [6] 0 forward / 1 backward, [7] c | m << 16
__device__ long long g_mfs_trace[128 * 8];
__device__ int g_mfs_trace_n;
#define MFS_BEGIN(kind) __shared__ int mfs_tr_s; const bool mfs_on = blockIdx.x == 0 && blockIdx.y == 0; if (threadIdx.x == 0) mfs_tr_s = mfs_on ? (atomicAdd(&g_mfs_trace_n, 1) & 127) : 0; \
    __syncthreads(); const int mfs_tr = mfs_tr_s; if (mfs_on && threadIdx.x == 0) { g_mfs_trace[mfs_tr * 8 + 6] = (kind); g_mfs_trace[mfs_tr * 8 + 7] = nd.c | ((nd.c + nd.r) << 16); }
#define MFS_STAMP(slot) do { if (mfs_on && threadIdx.x == 0) g_mfs_trace[mfs_tr * 8 + (slot)] = wall_clock64(); } while (0)
#else
#define MF_STAMP(slot) do { } while (0)
#define MFS_STAMP(slot) do { } while (0)
#endif

// The trailing update of one panel (columns kb .. pe - 1, pe - kb = 4 NK) by one wavefront: its 16 x 16 tiles of the lower triangle beyond pe, row-major, every NW-th.
// F[i][j] -= sum_k (y_ik / d_k) y_jk on the fp64 matrix cores (first operand = scaled rows of the i tile, second = rows of the j tile; two accumulator chains per tile:
// a dependent v_mfma_f64_16x16x4 issues every 64 cycles).  (bi, bj) advance on scalar registers; a tile needs ONE triangular index per operand and one for its
// results (the others follow by i -> i + 4: + 4 i + 10); everything up to the stores is branch-free — rows past the front are clamped for the loads and masked for the stores.  (Requesting the NEXT tile's operands ahead of the
// current tile's matrix instructions was measured: nothing.)
struct MfTile { double af[4], bf[4], old[4]; int o[4]; bool s[4]; };
// LDSF: the front lives in LDS.  Its operand reads are explicit ds_read_b64 then: left to the compiler, the four k-steps of an operand become ds_read2_b64 pairs — half the
// rate and other lane groups (16 contiguous lanes = 16 different rows of the packed triangle at one k: bank conflicts), which is what the update phase was waiting for
template <int NK, bool LDSF>
__device__ __forceinline__ void mf_tile_load(MfTile& T, const double* __restrict__ F, int m, int kb, int pe, int bi, int bj, int fr, int fk) {
    const int i0 = pe + 16 * bi + fk, j = pe + 16 * bj + fr;
    const double* Fa = F + tri0(min(pe + 16 * bi + fr, m - 1)) + kb + fk;
    const double* Fb = F + tri0(min(j, m - 1)) + kb + fk;
    int t = tri0(i0);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int i = i0 + 4 * rr;
        T.s[rr] = j <= i && i < m;
        T.o[rr] = T.s[rr] ? t + j : 0;
        t += 4 * i + 10;
    }
    if constexpr (LDSF) {
        const unsigned ea = (unsigned)(uintptr_t)Fa, eb = (unsigned)(uintptr_t)Fb;
#pragma unroll
        for (int kk = 0; kk < NK; ++kk) {
            asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(T.af[kk]) : "v"(ea), "n"(32 * kk) : "memory");
            asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(T.bf[kk]) : "v"(eb), "n"(32 * kk) : "memory");
        }
    } else {
#pragma unroll
        for (int kk = 0; kk < NK; ++kk) { T.af[kk] = Fa[4 * kk]; T.bf[kk] = Fb[4 * kk]; }
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) T.old[rr] = F[T.o[rr]];
}
// (what the explicit reads of a tile return is there after this: the compiler does not count them)
template <int NK> __device__ __forceinline__ void mf_tile_wait(MfTile& T) {
    if constexpr (NK == 4) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(T.af[0]), "+v"(T.af[1]), "+v"(T.af[2]), "+v"(T.af[3]), "+v"(T.bf[0]), "+v"(T.bf[1]), "+v"(T.bf[2]), "+v"(T.bf[3]) :: "memory");
    else if constexpr (NK == 3) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(T.af[0]), "+v"(T.af[1]), "+v"(T.af[2]), "+v"(T.bf[0]), "+v"(T.bf[1]), "+v"(T.bf[2]) :: "memory");
    else if constexpr (NK == 2) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(T.af[0]), "+v"(T.af[1]), "+v"(T.bf[0]), "+v"(T.bf[1]) :: "memory");
    else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(T.af[0]), "+v"(T.bf[0]) :: "memory");
}
template <int NK, int NW, bool LDSF>
__device__ __forceinline__ void mf_update_tiles(double* __restrict__ F, const double (&rfh)[4], int m, int kb, int pe, int wv, int ntile, int fr, int fk) {
    if (wv >= ntile) return;
    int bi = 0, bj = wv;
    while (bj > bi) { bj -= bi + 1; ++bi; }
    for (int t = wv; t < ntile; t += NW) {
        MfTile A;
        mf_tile_load<NK, LDSF>(A, F, m, kb, pe, bi, bj, fr, fk);
        bj += NW;
        while (bj > bi) { bj -= bi + 1; ++bi; }
        if constexpr (LDSF) mf_tile_wait<NK>(A);
        calipso_v4d acc = {0.0, 0.0, 0.0, 0.0}, acc2 = {0.0, 0.0, 0.0, 0.0};
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A.af[0] * rfh[0], A.bf[0], acc, 0, 0, 0);
        if constexpr (NK > 1) acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(A.af[1] * rfh[1], A.bf[1], acc2, 0, 0, 0);
        if constexpr (NK > 2) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A.af[2] * rfh[2], A.bf[2], acc, 0, 0, 0);
        if constexpr (NK > 3) acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(A.af[3] * rfh[3], A.bf[3], acc2, 0, 0, 0);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) if (A.s[rr]) F[A.o[rr]] = A.old[rr] - (acc[rr] + acc2[rr]);
    }
}
// the barriers of the factorisation loop: a front in LDS needs the LDS traffic ordered, not the global stores in flight (the panel of L leaves column block by
// column block under the loop, and __syncthreads() would wait for every store at every barrier); a front in global memory needs the full one
template <bool GF> __device__ __forceinline__ void mf_barrier() {
    if constexpr (GF) __syncthreads();
    else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
// one front: assembly, the partial LDL^T of its first c columns, the panel and the update matrix to global memory (every thread of the workgroup arrives)
template <int MF_THREADS, bool GF>
__device__ __forceinline__ void mf_factor_node(const MfDev& d, const MfNode& nd, const size_t z, const int ypan, double* __restrict__ Flds, const bool mf_traced, const int mf_tr) {
    MF_STAMP(0);
    constexpr int MF_RC = MF_THREADS / 16;        // row classes of the panel step (16 panel columns x MF_RC rows at a time)
    __shared__ int relS[256];                                                  // relative indices of the child being extend-added (LDS fronts: r <= 196)
    __shared__ double rinvS[64];                                               // GF: reciprocal pivots (a node has at most 64 columns)
    const int f = nd.f, c = nd.c, r = nd.r, m = c + r, nt = tri0(m);
    const int tid = threadIdx.x;
    double* F = GF ? d.fpool + z * d.sPool + nd.foff : Flds;                    // GF: the front lives in global memory (L2-resident)
    double* ycol = GF ? rinvS : F + nt;
    const double* Aval = d.Aval + z * d.sA;
    double* upd = d.upd + z * d.sUpd; double* panel = d.panel + z * d.sPanel; double* Dg = d.D + z * d.sD;
    // Assembly.  LDS fronts whose node carries extend-add items (MfXItem, built with the pattern): EVERY global load of the assembly is issued before anything waits —
    // the node's entries of A (Aloc / Asrc, then the values they point to) and the children's update matrices (items, then the pool entries they name): two memory
    // round trips for the whole front, the zero fill of the front under the first.  (Before: a round trip per 16 rows of a child, two for the own entries, one after
    // the other: 10 of a front's 30 us.)  Same operations on every entry in the same order (children ascending; a child's entries land on distinct places), so the
    // assembled front has the same bits.
    bool fast = false;
    if constexpr (!GF) fast = nd.xa0 >= 0;
    if (fast) {
        constexpr int AK = 8, XK = 8;
        const unsigned* __restrict__ xit = reinterpret_cast<const unsigned*>(d.xit);
        int al[AK], as[AK];
        uint2 it[XK];
        const int alast = max(nd.alp1 - 1, 0), xlast = max(nd.xa1 - 1, 0);
#pragma unroll
        for (int u = 0; u < AK; ++u) { const int p = min(nd.alp0 + tid + u * MF_THREADS, alast); al[u] = d.Aloc[p]; as[u] = d.Asrc[p]; }
#pragma unroll
        for (int u = 0; u < XK; ++u) { const int e = min(nd.xa0 + tid + u * MF_THREADS, xlast); it[u] = reinterpret_cast<const uint2*>(xit)[e]; }
        unsigned qw0 = xit[2 * (size_t)min(nd.xa0, xlast) + 1], qw1 = xit[2 * (size_t)min(nd.xa0 + XK * MF_THREADS - 1, xlast) + 1];   // first / last child of the chunk
        for (int e = tid; e < nt; e += MF_THREADS) F[e] = 0.0;
        double av[AK], uv[XK];
#pragma unroll
        for (int u = 0; u < AK; ++u) av[u] = Aval[as[u]];
#pragma unroll
        for (int u = 0; u < XK; ++u) uv[u] = upd[it[u].x];
        __syncthreads();
        MF_STAMP(1);
#pragma unroll
        for (int u = 0; u < AK; ++u) if (nd.alp0 + tid + u * MF_THREADS < nd.alp1) F[al[u]] = av[u];
        for (int p = nd.alp0 + AK * MF_THREADS + tid; p < nd.alp1; p += MF_THREADS) F[d.Aloc[p]] = Aval[d.Asrc[p]];
        __syncthreads();
        MF_STAMP(2);
        for (int cb = nd.xa0; cb < nd.xa1; cb += XK * MF_THREADS) {
            if (cb > nd.xa0) {
#pragma unroll
                for (int u = 0; u < XK; ++u) { const int e = min(cb + tid + u * MF_THREADS, xlast); it[u] = reinterpret_cast<const uint2*>(xit)[e]; }
#pragma unroll
                for (int u = 0; u < XK; ++u) uv[u] = upd[it[u].x];
                qw0 = xit[2 * (size_t)cb + 1]; qw1 = xit[2 * (size_t)min(cb + XK * MF_THREADS - 1, xlast) + 1];
            }
            // the children present in this chunk, in turn (a barrier between two children: both may add to one place, and the order of the sum is the children's)
            const int qlo = (int)(qw0 >> 16), qhi = (int)(qw1 >> 16);
            for (int q = qlo; q <= qhi; ++q) {
                double cur[XK];                                                   // (all reads of the round before its writes: the places of ONE child are distinct)
#pragma unroll
                for (int u = 0; u < XK; ++u) cur[u] = F[it[u].y & 0xffffu];
#pragma unroll
                for (int u = 0; u < XK; ++u)
                    if (cb + tid + u * MF_THREADS < nd.xa1 && (int)(it[u].y >> 16) == q) F[it[u].y & 0xffffu] = cur[u] + uv[u];
                __syncthreads();
            }
        }
    } else {
        for (int e = tid; e < nt; e += MF_THREADS) F[e] = 0.0;
        __syncthreads();
        MF_STAMP(1);
        for (int p = nd.alp0 + tid; p < nd.alp1; p += MF_THREADS) F[d.Aloc[p]] = Aval[d.Asrc[p]];
        __syncthreads();
        MF_STAMP(2);
        for (int q = 0; q < nd.nch; ++q) {                                         // extend-add, children in ascending order
            const MfChild cr = d.crec[nd.chfirst + q];
            const int rc = cr.rc;
            const double* U = upd + cr.upd_off;
            const int* rel = d.rel + cr.rowptr;
            if (!GF) { for (int a = tid; a < rc; a += MF_THREADS) relS[a] = rel[a]; }
            __syncthreads();
            if (GF) {
                for (int a = tid >> 5; a < rc; a += MF_THREADS / 32) {             // a row of the child's update matrix per 32 lanes, coalesced along b
                    const int rla = rel[a];
                    const int ra = tri0(rla);                            // rel is increasing: the lower triangle lands in the lower triangle
                    const double* Ua = U + (size_t)a * rc;
                    for (int b = tid & 31; b <= a; b += 32) F[ra + rel[b]] += Ua[b];
                }
            } else {
                // a row of the child's update matrix per 32 lanes (rc <= 196: at most seven chunks of 32 columns); the values of the NEXT row of this lane group
                // travel while the current one is added into the front (one memory round trip per row otherwise: 7 rows x 0.8 us per child)
                const int lb = tid & 31;
                int a = tid >> 5;
                double uv[7];
    #pragma unroll
                for (int q = 0; q < 7; ++q) { const int b = lb + 32 * q; uv[q] = (a < rc && b <= a) ? U[(size_t)a * rc + b] : 0.0; }
                while (a < rc) {
                    const int an = a + MF_THREADS / 32;
                    double un[7];
    #pragma unroll
                    for (int q = 0; q < 7; ++q) { const int b = lb + 32 * q; un[q] = (an < rc && b <= an) ? U[(size_t)an * rc + b] : 0.0; }
                    const int rla = relS[a];
                    const int ra = tri0(rla);                            // rel is increasing: the lower triangle lands in the lower triangle
    #pragma unroll
                    for (int q = 0; q < 7; ++q) { const int b = lb + 32 * q; if (b <= a) F[ra + relS[b]] += uv[q]; }
    #pragma unroll
                    for (int q = 0; q < 7; ++q) uv[q] = un[q];
                    a = an;
                }
            }
            __syncthreads();
        }
    }
    // Partial dense LDL^T of the first c columns, blocked: panels of 16 columns.
    //   panel   column j is left UNSCALED in F (y_ij = l_ij d_j; nothing overwrites what the other rows still read, so ONE barrier per column);
    //           256 threads as 16 row classes x 16 panel columns apply  F[i][k] -= y_ij (y_kj / d_j)  to the panel columns k > j, rows i >= k.
    //   update  F[i][j] -= sum_k (y_ik / d_k) y_jk over the panel, for every 16 x 16 tile of the trailing lower triangle on the fp64 matrix cores
    //           (v_mfma_f64_16x16x4: first operand = scaled rows of the i tile, second = rows of the j tile, K = 16 = one panel).
    double* rinv = ycol;                                                       // c reciprocal pivots (the 2 m doubles behind the front)
    double* P = panel + nd.panel_off;                                          // the node's panel of L, column-major m x c: column k contiguous over the rows
    int p_done = 0;                                                            // columns of it already written
    const int lane = tid & 63, wave = tid >> 6, fr = lane & 15, fk = lane >> 4;
    MF_STAMP(3);
#ifdef CALIPSO_LDL_TRACE
    long long mf_pan = 0, mf_upd = 0, mf_t0 = 0;
#endif
    for (int kb = 0; kb < c; kb += 16) {
        const int pe = min(kb + 16, c);
#ifdef CALIPSO_LDL_TRACE
        mf_t0 = wall_clock64();
#endif
        if (!GF && ypan && (pe - kb == 16 || pe - kb == 8) && m >= 32) {
            // A full panel through registers (pivot16.hpp; ldl.hip: diag_block has the design notes): wavefront 0 takes rows kb .. kb + 63 with lane = row and
            // factors the 16 columns alone — no barrier between pivots.  The rows further down go to the wavefronts behind it AT THE SAME TIME: wavefront e >= 1 puts the
            // 16 rows of the diagonal block in its lanes 0 .. 15 and rows kb + 64 + 48 (e - 1) ... in the other 48, and runs the same instruction sequence — the diagonal
            // block is factored redundantly, to the same bits, so nobody waits for wavefront 0's pivots (m <= 196: at most three such wavefronts; they share the exchange
            // rows: every writer of a diagonal row writes the same value, the other rows are never read).  Two barriers per panel instead of sixteen; the columns stay
            // UNSCALED in the front, as the loop below leaves them.  (Before: the rows beyond the first 64 FOLLOWED in a phase of their own, 0.9 us and a barrier per panel.)
            double* Yp = F + nt + 2 * m;                                       // 64 exchange rows of MF_PY doubles (the pivot columns, read back replicated)
            const bool half = pe - kb == 8;                                    // (a node of 56 columns ends in a half panel)
            mf_barrier<GF>();
            const int xrow0 = kb + 64 + 48 * (wave - 1);
            if (wave == 0 || xrow0 < m) {
                const int row = (wave == 0 || lane < 16) ? kb + lane : xrow0 + lane - 16;
                const bool in = row < m, mine = wave == 0 || lane >= 16;
                const int rowc = min(row, m - 1);
                const int trow = tri0(rowc) + kb;                   // (loads unconditional from a valid address, then selected: no exec-masked blocks)
                const int below = rowc - kb;                        // columns 0 .. min(below, 15) of the panel exist in this row
                double a[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) a[q] = F[trow + min(q, below)];
#pragma unroll
                for (int q = 0; q < 16; ++q) a[q] = (in && below >= q && (q < 8 || !half)) ? a[q] : 0.0;
                const int drow = min(kb + (lane & 15), m - 1);
                const double y0 = F[tri0(drow) + kb];
                const int lo = __builtin_amdgcn_readlane(__double2loint(a[0]), 0), hi = __builtin_amdgcn_readlane(__double2hiint(a[0]), 0);
                if (half) calipso::Pivot<0, false, 8>::run(a, (unsigned)(uintptr_t)(Yp + lane * MF_PY), (unsigned)(uintptr_t)(Yp + (lane & 15) * MF_PY), nullptr, 0,
                                                           calipso::fast_rcp(__hiloint2double(hi, lo)), y0);
                else calipso::Pivot<0, false, 16>::run(a, (unsigned)(uintptr_t)(Yp + lane * MF_PY), (unsigned)(uintptr_t)(Yp + (lane & 15) * MF_PY), nullptr, 0,
                                                       calipso::fast_rcp(__hiloint2double(hi, lo)), y0);
                if (in && mine) {
#pragma unroll
                    for (int q = 0; q < 16; ++q) if (below >= q && (q < 8 || !half)) F[trow + q] = a[q];
                }
                if (wave == 0 && lane < (half ? 8 : 16)) {
                    double dd = a[0];
#pragma unroll
                    for (int q = 1; q < 16; ++q) dd = (lane == q) ? a[q] : dd;
                    rinv[kb + lane] = calipso::fast_rcp(dd);
                    Dg[f + kb + lane] = dd;
                }
            } else {
                // the wavefronts without rows of this panel send the columns of the panels BEFORE it to the panel of L (they are final, and this step does not touch
                // them): most of the write-out runs under the pivots instead of in the tail of the kernel
                const int first_idle = 1 + max(0, (m - kb - 64 + 47) / 48), nidle = MF_THREADS / 64 - first_idle;
                for (int k = p_done + (wave - first_idle); k < kb; k += nidle) {
                    const double rk = rinv[k];
                    for (int i = lane; i < m; i += 64) P[i + (size_t)k * m] = i > k ? F[tri0(i) + k] * rk : 0.0;
                }
            }
            if (1 + max(0, (m - kb - 64 + 47) / 48) < MF_THREADS / 64) p_done = kb;
        } else
        for (int j = kb; j < pe; ++j) {
            mf_barrier<GF>();
            const double dj = F[tri(j, j)];
            const double rj = 1.0 / dj;
            if (tid == 0) { Dg[f + j] = dj; rinv[j] = rj; }
            const int k = j + 1 + (tid & 15);                                  // MF_RC x 16 threads over (row, panel column)
            if (k < pe) {
                const double ykj = F[tri(k, j)] * rj;
                int i = j + 1 + (tid >> 4);                                      // rows i >= k of this thread's residue class
                if (i < k) i += ((k - i + MF_RC - 1) / MF_RC) * MF_RC;
                for (; i < m; i += MF_RC) {
                    double* Fi = F + tri0(i);
                    Fi[k] -= Fi[j] * ykj;
                }
            }
        }
        mf_barrier<GF>();
#ifdef CALIPSO_LDL_TRACE
        { const long long t1 = wall_clock64(); mf_pan += t1 - mf_t0; mf_t0 = t1; }
#endif
        const int ntl = (m - pe + 15) / 16;                                    // 16-row tiles of the trailing part
        // the tiles of the lower triangle (bi >= bj), row-major, dealt round-robin to the wavefronts: every wavefront gets the same number of tiles to within
        // one (whole tile rows per wavefront left the one with the longest rows 1.7 x the average).  Two accumulator chains per tile (a dependent
        // v_mfma_f64_16x16x4 issues every 64 cycles).
        const int ntile = tri0(ntl);
        const int wv = __builtin_amdgcn_readfirstlane(wave);
        const int nk4 = ((pe - kb) & 3) == 0 ? (pe - kb) >> 2 : 0;            // k-steps of the panel when every lane of a step is inside it (0: the general body below)
        if (nk4) {
            double rfh[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) rfh[kk] = rinv[min(kb + 4 * kk + fk, pe - 1)];
            if (nk4 == 4) mf_update_tiles<4, MF_THREADS / 64, !GF>(F, rfh, m, kb, pe, wv, ntile, fr, fk);
            else if (nk4 == 2) mf_update_tiles<2, MF_THREADS / 64, !GF>(F, rfh, m, kb, pe, wv, ntile, fr, fk);
            else if (nk4 == 3) mf_update_tiles<3, MF_THREADS / 64, !GF>(F, rfh, m, kb, pe, wv, ntile, fr, fk);
            else mf_update_tiles<1, MF_THREADS / 64, !GF>(F, rfh, m, kb, pe, wv, ntile, fr, fk);
        } else
        for (int t = wave; t < ntile; t += MF_THREADS / 64) {
            // panels whose width is not a multiple of four: every read is unconditional, from a clamped address, the k steps outside the panel are zeroed
            int bi = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
            while ((bi + 1) * (bi + 2) / 2 <= t) ++bi;
            while (tri0(bi) > t) --bi;
            const int bj = t - tri0(bi);
            const int ia = pe + 16 * bi + fr;                                  // the row this lane feeds to the first operand
            const int jbr = pe + 16 * bj + fr;                                  // ... to the second operand
            // every LDS read below is unconditional, from a clamped (always valid) address, and all of them are issued before the first use: a load inside a
            // conditional becomes an exec-masked block with its own wait (measured: 2400 cycles per tile that way)
            const int iac = min(ia, m - 1), jbc = min(jbr, m - 1);
            const int ra = tri0(iac), rb = tri0(jbc);
            double af[4], bf[4], rf[4], old[4];
            int oidx[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int kc = min(kb + 4 * kk + fk, pe - 1);
                af[kk] = F[ra + kc]; bf[kk] = F[rb + kc]; rf[kk] = rinv[kc];
            }
            const int j = pe + 16 * bj + fr;                                    // result column (second operand's tile)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int i = pe + 16 * bi + fk + 4 * rr;                       // result row (first operand's tile)
                const int ic = min(i, m - 1), jc = min(j, ic);
                oidx[rr] = tri0(ic) + jc;
                old[rr] = F[oidx[rr]];
            }
            double av[4], bv[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const bool kin = kb + 4 * kk + fk < pe;
                av[kk] = (kin && ia < m) ? af[kk] * rf[kk] : 0.0;
                bv[kk] = (kin && jbr < m) ? bf[kk] : 0.0;
            }
            calipso_v4d acc = {0.0, 0.0, 0.0, 0.0}, acc2 = {0.0, 0.0, 0.0, 0.0};
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0], bv[0], acc, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[1], bv[1], acc2, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[2], bv[2], acc, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[3], bv[3], acc2, 0, 0, 0);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int i = pe + 16 * bi + fk + 4 * rr;
                if (i < m && j <= i) F[oidx[rr]] = old[rr] - (acc[rr] + acc2[rr]);
            }
        }
#ifdef CALIPSO_LDL_TRACE
        mf_barrier<GF>();
        mf_upd += wall_clock64() - mf_t0;
#endif
    }
    mf_barrier<GF>();
    MF_STAMP(4);
#ifdef CALIPSO_LDL_TRACE
    if (mf_traced && tid == 0) { g_mf_trace[(mf_tr & 63) * 12 + 8] = mf_pan; g_mf_trace[(mf_tr & 63) * 12 + 9] = mf_upd; }
#endif
    // write-out: what is left of the panel (a wavefront per column, lanes along the rows: contiguous stores) and the update matrix (a wavefront per row, lanes along
    // the columns)
    for (int k = p_done + wave; k < c; k += MF_THREADS / 64) {
        const double rk = rinv[k];
        for (int i = lane; i < m; i += 64) P[i + (size_t)k * m] = i > k ? F[tri0(i) + k] * rk : 0.0;
    }
    double* U = upd + nd.upd_off;
    for (int a = wave; a < r; a += MF_THREADS / 64) {
        const double* Fa = F + tri0(c + a) + c;
        for (int b = lane; b <= a; b += 64) U[(size_t)a * r + b] = Fa[b];
    }
    MF_STAMP(5);
}

template <int MF_THREADS, bool GF>
__global__ __launch_bounds__(MF_THREADS) void k_mf_factor(const MfDev d, const MfSlots sl, int first, int ypan) {
    extern __shared__ __attribute__((aligned(16))) double Flds[];
    bool mf_traced = false; int mf_tr = 0;
#ifdef CALIPSO_LDL_TRACE
    __shared__ int mf_tr_s;
    mf_traced = blockIdx.x == 0 && blockIdx.y == 0;
    if (threadIdx.x == 0) mf_tr_s = mf_traced ? atomicAdd(&g_mf_trace_n, 1) : 0;
    __syncthreads();
    mf_tr = mf_tr_s;
    if (mf_traced && threadIdx.x == 0) { g_mf_trace[(mf_tr & 63) * 12 + 10] = d.nrec[first].c; g_mf_trace[(mf_tr & 63) * 12 + 11] = d.nrec[first].c + d.nrec[first].r; }
#endif
    const MfNode nd = d.nrec[first + blockIdx.x];
    const size_t z = sl.use ? (size_t)sl.slot[blockIdx.y] : (size_t)blockIdx.y;   // storage slot of this instance of the batch
    mf_factor_node<MF_THREADS, GF>(d, nd, z, ypan, Flds, mf_traced, mf_tr);
}

// forward: v = [b_C ; 0] + children's contributions;  y_C = L11^-1 v_C;  v_R -= L21 y_C  -> the node's contribution to its ancestors.
// The c <= 64 dependent steps of the triangular solve run in ONE wavefront (lane = row, y_k by v_readlane, no barrier: ~20 cycles per step instead of a
// workgroup barrier); the product with L21 is spread over all threads (four k-slices per row, combined in a fixed order).  The panel is read where it
// lies (every entry is used once): the LDS holds only the vector.  (GP, the former "panel too large for the LDS" variant, is the same code now.)
__device__ __forceinline__ double mf_readlane_d(double v, int lane) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, lane);
    hi = __builtin_amdgcn_readlane(hi, lane);
    return __hiloint2double(hi, lo);
}
// (one node and right-hand side: yi = instance * nrhs + right-hand side, zs = the instance's storage slot; every thread of the workgroup arrives)
template <int MF_THREADS>
__device__ __forceinline__ void mf_forward_node(const MfDev& d, const MfNode& nd, const size_t yi, const size_t zs, int n, long long usum, double* __restrict__ X,
                                                double* __restrict__ sm, const bool mfs_on = false, const int mfs_tr = 0) {
    MFS_STAMP(0);
    const int f = nd.f, c = nd.c, r = nd.r, m = c + r;
    double* v = sm;                                                            // m
    double* part = sm + m;                                                     // 4 r
    double* x = X + yi * n;
    double* ubase = d.uvec + yi * usum;
    const double* panel = d.panel + zs * d.sPanel;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* P = panel + nd.panel_off;
    // Every entry of the panel this thread will need is requested FIRST (the panel does not depend on the vector): the lower triangle of L11 by wavefront 0
    // (two batches of 32 columns), the first slice of L21 by everybody; the assembly of the vector runs while they travel.
    const int cs = (c + 3) / 4;                                                // columns per slice of the product with L21 (c <= 64: at most 16)
    double pl0[32], pl1[32], pv0[16];
    if (wave == 0) {
#pragma unroll
        for (int q = 0; q < 32; ++q) { pl0[q] = (q < c && lane > q && lane < c) ? P[lane + (size_t)q * m] : 0.0; }
#pragma unroll
        for (int q = 0; q < 32; ++q) { const int k = 32 + q; pl1[q] = (k < c && lane > k && lane < c) ? P[lane + (size_t)k * m] : 0.0; }
    }
    {
        const int idx = tid, a = r > 0 ? idx % r : 0, q4 = r > 0 ? idx / r : 0, kbeg = q4 * cs, kend = min(c, kbeg + cs);
        const double* Pi = P + (c + a);
#pragma unroll
        for (int q = 0; q < 16; ++q) pv0[q] = (idx < 4 * r && kbeg + q < kend) ? Pi[(size_t)(kbeg + q) * m] : 0.0;
    }
    for (int i = tid; i < m; i += MF_THREADS) v[i] = i < c ? x[f + i] : 0.0;
    __syncthreads();
    MFS_STAMP(1);
    // the children's contributions, two children at a time: both records, then both children's values and places travel together (one memory round trip per PAIR
    // after the records instead of one per child); the sums stay in the children's order (a barrier between the two)
    for (int q = 0; q < nd.nch; q += 2) {
        const MfChild cr0 = d.crec[nd.chfirst + q];
        const MfChild cr1 = d.crec[nd.chfirst + min(q + 1, nd.nch - 1)];
        const int rc0 = cr0.rc, rc1 = q + 1 < nd.nch ? cr1.rc : 0;
        const double* u0 = ubase + cr0.u_off; const double* u1 = ubase + cr1.u_off;
        const int* rel0 = d.rel + cr0.rowptr; const int* rel1 = d.rel + cr1.rowptr;
        const int a0 = min(tid, max(rc0 - 1, 0)), a1 = min(tid, max(rc1 - 1, 0));
        const double w0 = u0[a0], w1 = rc1 ? u1[a1] : 0.0;
        const int p0 = rel0[a0], p1 = rc1 ? rel1[a1] : 0;
        if (tid < rc0) v[p0] += w0;
        for (int a = tid + MF_THREADS; a < rc0; a += MF_THREADS) v[rel0[a]] += u0[a];
        __syncthreads();
        if (rc1) {
            if (tid < rc1) v[p1] += w1;
            for (int a = tid + MF_THREADS; a < rc1; a += MF_THREADS) v[rel1[a]] += u1[a];
            __syncthreads();
        }
    }
    MFS_STAMP(2);
    if (wave == 0) {
        double vi = lane < c ? v[lane] : 0.0;
#pragma unroll
        for (int q = 0; q < 32; ++q) { if (q < c) vi = fma(-pl0[q], mf_readlane_d(vi, q), vi); }
#pragma unroll
        for (int q = 0; q < 32; ++q) { const int k = 32 + q; if (k < c) vi = fma(-pl1[q], mf_readlane_d(vi, k), vi); }
        if (lane < c) { v[lane] = vi; x[f + lane] = vi; }
    }
    __syncthreads();
    MFS_STAMP(3);
    for (int idx = tid; idx < 4 * r; idx += MF_THREADS) {
        const int a = idx % r, q4 = idx / r, kbeg = q4 * cs, kend = min(c, kbeg + cs);
        const double* Pi = P + (c + a);
        double acc = 0.0;
        if (idx == tid) {                                                       // the slice fetched at the top
#pragma unroll
            for (int q = 0; q < 16; ++q) acc += pv0[q] * (kbeg + q < kend ? v[kbeg + q] : 0.0);
        } else {
            double pv[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) pv[q] = kbeg + q < kend ? Pi[(size_t)(kbeg + q) * m] : 0.0;
#pragma unroll
            for (int q = 0; q < 16; ++q) acc += pv[q] * (kbeg + q < kend ? v[kbeg + q] : 0.0);
        }
        part[idx] = acc;
    }
    __syncthreads();
    double* u = ubase + nd.u_off;
    for (int a = tid; a < r; a += MF_THREADS) u[a] = v[c + a] - ((part[a] + part[r + a]) + (part[2 * r + a] + part[3 * r + a]));
    MFS_STAMP(4);
}
template <int MF_THREADS, bool GP>
__global__ __launch_bounds__(MF_THREADS) void k_mf_forward(const MfDev d, const MfSlots sl, int first, int n, int nrhs, long long usum, double* __restrict__ X) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const MfNode nd = d.nrec[first + blockIdx.x];                              // blockIdx.y = instance * nrhs + right-hand side
#ifdef CALIPSO_LDL_TRACE
    MFS_BEGIN(0)
    mf_forward_node<MF_THREADS>(d, nd, (size_t)blockIdx.y, (size_t)(sl.use ? sl.slot[blockIdx.y / nrhs] : (int)(blockIdx.y / nrhs)), n, usum, X, sm, mfs_on, mfs_tr);
#else
    mf_forward_node<MF_THREADS>(d, nd, (size_t)blockIdx.y, (size_t)(sl.use ? sl.slot[blockIdx.y / nrhs] : (int)(blockIdx.y / nrhs)), n, usum, X, sm);
#endif
}
// backward: z_C = y_C / D_C - L21' x_R (x_R final: it belongs to ancestors);  x_C = L11^-T z_C.  One wavefront per column for the product with L21'
// (lanes along the rows, contiguous), then the c dependent steps in one wavefront (lane = column, x_i by v_readlane).
template <int MF_THREADS>
__device__ __forceinline__ void mf_backward_node(const MfDev& d, const MfNode& nd, const size_t yi, const size_t zs, int n, double* __restrict__ X, double* __restrict__ sm,
                                                 const bool mfs_on = false, const int mfs_tr = 0) {
    MFS_STAMP(0);
    const int f = nd.f, c = nd.c, r = nd.r, m = c + r;
    double* v = sm;
    double* x = X + yi * n;
    const double* panel = d.panel + zs * d.sPanel; const double* Dg = d.D + zs * d.sD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* P = panel + nd.panel_off;
    const int* R = d.rows + nd.rowptr;
    constexpr int NW = MF_THREADS / 64, CPW = 64 / NW;                         // columns per wavefront: k = wave + NW q (c <= 64); their loads travel together
    // the panel entries of the first row chunk (and, wavefront 0, the rows of L11 it will walk) are requested before the vector is assembled
    double pvf[CPW], pl0[32], pl1[32];
#pragma unroll
    for (int q = 0; q < CPW; ++q) { const int k = wave + NW * q; pvf[q] = (k < c && lane < r) ? P[(c + lane) + (size_t)k * m] : 0.0; }
    if (wave == 0) {
#pragma unroll
        for (int q = 0; q < 32; ++q) { const int i = c - 1 - q; pl0[q] = (i >= 1 && lane < i) ? P[i + (size_t)lane * m] : 0.0; }
#pragma unroll
        for (int q = 0; q < 32; ++q) { const int i = c - 33 - q; pl1[q] = (i >= 1 && lane < i) ? P[i + (size_t)lane * m] : 0.0; }
    }
    for (int i = tid; i < m; i += MF_THREADS) v[i] = i < c ? x[f + i] / Dg[f + i] : x[R[i - c]];
    __syncthreads();
    MFS_STAMP(1);
    if (r > 0) {                                                               // (a root has no rows below its columns: nothing to subtract)
        double acc[CPW];
#pragma unroll
        for (int q = 0; q < CPW; ++q) acc[q] = 0.0;
        for (int a0 = 0; a0 < r; a0 += 64) {
            const int a = a0 + lane;
            const double va = a < r ? v[c + a] : 0.0;
            double pv[CPW];
            if (a0 == 0) {
#pragma unroll
                for (int q = 0; q < CPW; ++q) pv[q] = pvf[q];
            } else {
#pragma unroll
                for (int q = 0; q < CPW; ++q) { const int k = wave + NW * q; pv[q] = (k < c && a < r) ? P[(c + a) + (size_t)k * m] : 0.0; }
            }
#pragma unroll
            for (int q = 0; q < CPW; ++q) acc[q] += pv[q] * va;
        }
#pragma unroll
        for (int q = 0; q < CPW; ++q) {
            const int k = wave + NW * q;
            const double t = calipso::wave_sum_l63(acc[q]);     // (16 sums per wavefront: by __shfl_down they were 3.8 of a node's 8 us, bench/mf_solve_trace.py)
            if (lane == 63 && k < c) v[k] -= t;
        }
    }
    __syncthreads();
    MFS_STAMP(2);
    if (wave == 0) {
        double zk = lane < c ? v[lane] : 0.0;
#pragma unroll
        for (int q = 0; q < 32; ++q) { const int i = c - 1 - q; if (i >= 1) zk = fma(-pl0[q], mf_readlane_d(zk, i), zk); }
#pragma unroll
        for (int q = 0; q < 32; ++q) { const int i = c - 33 - q; if (i >= 1) zk = fma(-pl1[q], mf_readlane_d(zk, i), zk); }
        if (lane < c) x[f + lane] = zk;
    }
    MFS_STAMP(3); MFS_STAMP(4);
}
template <int MF_THREADS, bool GP>
__global__ __launch_bounds__(MF_THREADS) void k_mf_backward(const MfDev d, const MfSlots sl, int first, int n, int nrhs, double* __restrict__ X) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const MfNode nd = d.nrec[first + blockIdx.x];
#ifdef CALIPSO_LDL_TRACE
    MFS_BEGIN(1)
    mf_backward_node<MF_THREADS>(d, nd, (size_t)blockIdx.y, (size_t)(sl.use ? sl.slot[blockIdx.y / nrhs] : (int)(blockIdx.y / nrhs)), n, X, sm, mfs_on, mfs_tr);
#else
    mf_backward_node<MF_THREADS>(d, nd, (size_t)blockIdx.y, (size_t)(sl.use ? sl.slot[blockIdx.y / nrhs] : (int)(blockIdx.y / nrhs)), n, X, sm);
#endif
}

#include "sparse_wide.hpp"

int g_wide_fronts = 1;         // calipso_hip_debug_wide_fronts: 0 = the one-workgroup kernel for the global-memory fronts too (plans made afterwards)
static int g_mf_items = 1;      // extend-add items for the LDS fronts (calipso_hip_debug_mf_items)
// launch helpers: the thread count of a level is fixed by the analyse phase (MfSeg::threads)
#define MF_LAUNCH(KERNEL, G, GRID, LDS, STREAM, ...)                                                                              \
    do {                                                                                                                          \
        if ((G).global) hipLaunchKernelGGL((KERNEL<512, true>), GRID, dim3(512), LDS, STREAM, __VA_ARGS__);                       \
        else if ((G).threads == 512) hipLaunchKernelGGL((KERNEL<512, false>), GRID, dim3(512), LDS, STREAM, __VA_ARGS__);         \
        else hipLaunchKernelGGL((KERNEL<256, false>), GRID, dim3(256), LDS, STREAM, __VA_ARGS__);                                \
    } while (0)


// the sweeps of a solve: 256 threads whatever the front (their 175-184 registers allow two wavefronts per SIMD: TWO workgroups of 256 per compute unit instead of one
// of 512 — a level of a batch has more fronts than compute units, and the node's work is a few microseconds; the bits do not depend on the thread count)
#define MF_LAUNCH_SOLVE(KERNEL, G, GRID, LDS, STREAM, ...)                                                                        \
    do {                                                                                                                          \
        if ((G).global) hipLaunchKernelGGL((KERNEL<512, true>), GRID, dim3(512), LDS, STREAM, __VA_ARGS__);                       \
        else hipLaunchKernelGGL((KERNEL<256, false>), GRID, dim3(256), LDS, STREAM, __VA_ARGS__);                                \
    } while (0)

}  // namespace

struct calipso_hip_sparse {
    SparsePlan plan;                             // everything the analyse phase made (sparse_plan.hpp): the host's copy of every table on the device
    int n = 0, device = 0;
    bool lds_acc = true;
    bool mf = false;                             // multifrontal numeric phase (plan.mf: nested-dissection orders whose fronts fit)
    MfDev md{};                                  // md and d hold COPIES of the pointers below: refresh_views() after anything grew
    SpDev d{};
    int batch = 1, selected = 0;                 // matrices of this pattern factored together / the one get_factor reads
    std::vector<long long> inertia_all;          // batch x 3
    std::vector<void*> dev;                      // every device allocation (device_memory.hpp): freed with the handle
    std::vector<void*>& device_allocations() { return dev; }
    hipStream_t device_stream() const { return stream; }
    int device_error(const std::string& text) { err = text; return CALIPSO_ERR_HIP; }
    Grown<double> Aval, Lx, D, panel, upd, fpool, wscr;      // what holds VALUES, for `batch` matrices, instance-major (alloc_values)
    Grown<long long> inertia_dev;                // batch x 3: k_reference_inertia's
    Grown<double> rhs, x, uvec;                  // a solve's right-hand sides, the permuted vectors and the update vectors of the sweeps (sparse_reserve_solve)
    Grown<double> wpart;                         // partial products of the backward sweep: (column of the solve, node of the level, row block, 64)
    const int* d_perm = nullptr;
    int work_slots = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = true;      // false once a solver handle lent its own stream (sparse_borrow_stream): a stream per plan would only crowd the hardware queues
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipGraphExec_t graph_factor = nullptr;
    bool graph_tried = false, factored = false;
    i64 inertia[3] = {0, 0, 0};
    double ms_factor = 0.0, ms_solve = 0.0;
    std::string err;
};

static thread_local std::string g_sparse_err;
#define PK(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) { (s ? s->err : g_sparse_err) = std::string(#call) + ": " + hipGetErrorString(e__); return CALIPSO_ERR_HIP; } } while (0)

namespace {

// the copies that the kernels' records hold of the handle's buffers: the one place that takes them, after anything was made or grew
void refresh_views(calipso_hip_sparse* s) {
    s->d.Aval = s->md.Aval = s->Aval.p; s->d.D = s->md.D = s->D.p; s->d.Lx = s->Lx.p;
    s->md.panel = s->panel.p; s->md.upd = s->upd.p; s->md.fpool = s->fpool.p; s->md.wscr = s->wscr.p; s->md.uvec = s->uvec.p;
}
// everything that holds VALUES, made anew for `batch` matrices of the analysed pattern (the stream is idle): what a smaller batch no longer needs is given back, and
// everything starts as zeros, filled on the plan's stream: of these only Aval is read before it is written (entries a structured handle never writes are structural zeros)
int alloc_values(calipso_hip_sparse* s, int batch) {
    const size_t B = (size_t)batch;
    const MfPlan* M = s->mf ? &*s->plan.mf : nullptr;
    const std::pair<Grown<double>*, size_t> each[7] = {{&s->Aval, std::max<size_t>((size_t)s->plan.nnzA, 1)}, {&s->D, (size_t)s->n}, {&s->Lx, M ? 0 : std::max<size_t>((size_t)s->plan.L.nnzL, 1)},
        {&s->panel, M ? std::max<size_t>((size_t)M->panel_total, 1) : 0}, {&s->upd, M ? std::max<size_t>((size_t)M->upd_total, 1) : 0}, {&s->fpool, M ? (size_t)M->pool_total : 0},
        {&s->wscr, M ? (size_t)M->wide_count * WF_SCR : 0}};
    for (const auto& [b, per_matrix] : each) {
        device_release(s, *b);
        if (const int rc = device_grown(s, *b, B * per_matrix)) return rc;
    }
    device_release(s, s->inertia_dev);
    if (const int rc = device_grown(s, s->inertia_dev, 3 * B)) return rc;
    if (M) { s->md.sPanel = M->panel_total; s->md.sUpd = M->upd_total; s->md.sPool = M->pool_total; }
    s->md.sA = s->plan.nnzA; s->md.sD = s->n;
    refresh_views(s);
    s->batch = batch; s->selected = 0; s->factored = false;
    s->inertia_all.assign(3 * B, 0);
    return CALIPSO_OK;
}
// the numeric factorisation of nz matrices (storage slots sl) on stream st: a launch per level of the tree (fronts beyond the LDS: three, sparse_wide.hpp)
void mf_enqueue_factor(calipso_hip_sparse* s, hipStream_t st, const MfSlots& sl, unsigned nz) {
    for (const MfSeg& g : s->plan.mf->levels) {
        if (g.wide.on) mf_wide_factor(st, s->md, sl, g.wide, g.first, g.count, nz);
        else MF_LAUNCH(k_mf_factor, g, dim3((unsigned)g.count, nz), g.lds_factor, st, s->md, sl, g.first, g.ypan);
    }
}
// both sweeps of a solve for ny = instances x nrhs columns of X (already permuted)
void mf_enqueue_solve(calipso_hip_sparse* s, hipStream_t st, const MfSlots& sl, unsigned ny, int nrhs, double* X) {
    const MfPlan& M = *s->plan.mf;
    const bool wide_ok = s->wpart.p && (size_t)ny * (size_t)M.wide_count * (size_t)M.wide_blocks * 64 <= s->wpart.cap;
    for (const MfSeg& g : M.levels) {
        if (g.wide.solve && wide_ok) mf_wide_forward(st, s->md, sl, g.wide, g.first, g.count, ny, s->n, nrhs, M.usum, X);
        else MF_LAUNCH_SOLVE(k_mf_forward, g, dim3((unsigned)g.count, ny), g.lds_solve, st, s->md, sl, g.first, s->n, nrhs, M.usum, X);
    }
    for (auto g = M.levels.rbegin(); g != M.levels.rend(); ++g) {
        if (g->wide.solve && wide_ok) mf_wide_backward(st, s->md, sl, g->wide, g->first, g->count, ny, s->n, nrhs, X, s->wpart.p, M.wide_blocks);
        else MF_LAUNCH_SOLVE(k_mf_backward, (*g), dim3((unsigned)g->count, ny), g->lds_solve, st, s->md, sl, g->first, s->n, nrhs, X);
    }
}

void enqueue_factor(calipso_hip_sparse* s) {
    if (s->mf) { mf_enqueue_factor(s, s->stream, MfSlots{}, (unsigned)s->batch); return; }
    const size_t lds = s->lds_acc ? sizeof(double) * (size_t)s->n : 0;
    for (int z = 0; z < s->batch; ++z) {                    // the column method takes the matrices of a batch one after the other
        SpDev d = s->d;
        d.Aval += (size_t)z * (size_t)s->plan.nnzA; d.Lx += (size_t)z * (size_t)s->plan.L.nnzL; d.D += (size_t)z * (size_t)s->n;
        for (const Segment& g : s->plan.cols.plan) {
            const int grid = g.chain ? 1 : std::min(g.count, s->work_slots);
            if (s->lds_acc) hipLaunchKernelGGL(k_sp_factor<true>, dim3(grid), dim3(SP_THREADS), lds, s->stream, d, g.first, g.count);
            else hipLaunchKernelGGL(k_sp_factor<false>, dim3(grid), dim3(SP_THREADS), 0, s->stream, d, g.first, g.count);
        }
    }
}

}  // namespace


// ---- hooks for the Newton handle (ldl.hip): the Schur complement S of a stage-structured problem through the multifrontal path -----------------
// S lives densely (column-major, leading dimension NP) in every instance's slab; `src` holds, for each entry of the analysed pattern, its offset
// row + col * NP.  Everything is enqueued on the CALLER's stream; nothing synchronises.
namespace {
__global__ void k_gather_dense(calipso::Batch bt, const double* __restrict__ S, const long long* __restrict__ src, long long nnz, double* __restrict__ Aval) {
    calipso::inst_shift(bt, S);
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nnz) Aval[(size_t)bt.slot[blockIdx.z] * (size_t)nnz + (size_t)q] = S[src[q]];
}
__global__ void k_permute_in_slab(calipso::Batch bt, const double* __restrict__ x, const int* __restrict__ perm, int n, double* __restrict__ dx) {
    calipso::inst_shift(bt, x);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dx[(size_t)blockIdx.z * n + i] = x[perm[i]];
}
__global__ void k_permute_out_slab(calipso::Batch bt, const double* __restrict__ dx, const int* __restrict__ perm, int n, double* __restrict__ x) {
    calipso::inst_shift(bt, x);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[perm[i]] = dx[(size_t)blockIdx.z * n + i];
}
// the p columns of X (leading dimension ld) of ONE instance: blockIdx.y = column
__global__ void k_permute_in_cols(const double* __restrict__ X, long long ld, const int* __restrict__ perm, int n, double* __restrict__ dx) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dx[(size_t)blockIdx.y * n + i] = X[(size_t)blockIdx.y * ld + perm[i]];
}
__global__ void k_permute_out_cols(const double* __restrict__ dx, const int* __restrict__ perm, int n, double* __restrict__ X, long long ld) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) X[(size_t)blockIdx.y * ld + perm[i]] = dx[(size_t)blockIdx.y * n + i];
}
// compute_inertia! (linear_solver.jl:33-44) of the S block: signs of its n pivots added to the handle's counters (icount[3..5] = positive, non-positive, zero)
__global__ __launch_bounds__(256) void k_count_signs(calipso::Batch bt, const double* __restrict__ D, int n, int* __restrict__ icount) {
    calipso::inst_shift_i(bt, icount);
    __shared__ int sh[3][4];
    const double* Dz = D + (size_t)bt.slot[blockIdx.z] * n;
    int pos = 0, nonpos = 0, zero = 0;
    for (int i = threadIdx.x; i < n; i += 256) { const double v = Dz[i]; pos += v > 0.0; nonpos += !(v > 0.0); zero += v == 0.0; }
    pos = calipso::wave_sum_i(pos); nonpos = calipso::wave_sum_i(nonpos); zero = calipso::wave_sum_i(zero);
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = pos; sh[1][threadIdx.x >> 6] = nonpos; sh[2][threadIdx.x >> 6] = zero; }
    __syncthreads();
    if (threadIdx.x == 0) {
        icount[3] += sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
        icount[4] += sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
        icount[5] += sh[2][0] + sh[2][1] + sh[2][2] + sh[2][3];
    }
}
// compute_inertia! as calipso_hip_sparse_factorize reports it, on the device: the up-looking factorisation stops at the first exact zero pivot in elimination order,
// the rest of D counts as zeros and inertia[0] = -1 (qdldl.jl:444,456,579).  One workgroup per matrix of `sl` (a whole batch: slot = blockIdx.z); out[3 * slot ..]:
// integers, so no order of summation shows.  It only reads D: both numeric phases.  Neither pass over D leaves early: a thread's loads do not wait for one another
constexpr int IN_THREADS = 1024, IN_WAVES = IN_THREADS / 64;
__global__ __launch_bounds__(IN_THREADS) void k_reference_inertia(const MfSlots sl, const double* __restrict__ D, int n, long long* __restrict__ out) {
    __shared__ int sh[3][IN_WAVES];
    const int slot = sl.use ? sl.slot[blockIdx.z] : (int)blockIdx.z, wave = threadIdx.x >> 6;
    const double* Dz = D + (size_t)slot * n;
    int first = n;
    for (int i = threadIdx.x; i < n; i += IN_THREADS) first = min(first, Dz[i] == 0.0 ? i : n);
    for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o));
    if ((threadIdx.x & 63) == 0) sh[0][wave] = first;
    __syncthreads();
    for (int w = 0; w < IN_WAVES; ++w) first = min(first, sh[0][w]);
    int pos = 0, nonpos = 0;
    for (int i = threadIdx.x; i < first; i += IN_THREADS) { const double v = Dz[i]; pos += v > 0.0; nonpos += v <= 0.0; }
    pos = calipso::wave_sum_i(pos); nonpos = calipso::wave_sum_i(nonpos);
    if ((threadIdx.x & 63) == 0) { sh[1][wave] = pos; sh[2][wave] = nonpos; }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long p = 0, q = 0, z = 0;
        for (int w = 0; w < IN_WAVES; ++w) { p += sh[1][w]; q += sh[2][w]; }
        if (first < n) { z = n - first; q += n - first; p = -1; }
        out[3 * (size_t)slot] = p; out[3 * (size_t)slot + 1] = q; out[3 * (size_t)slot + 2] = z;
    }
}
// the storage slots of the matrices of `bt` as the kernels take them — or false: not 1 .. batch matrices, a slot outside 0 .. batch - 1
bool slots_of(const calipso_hip_sparse* sp, const calipso::Batch& bt, MfSlots* sl) {
    if (bt.n < 1 || bt.n > sp->batch || bt.n > calipso::MAX_BATCH) return false;
    *sl = MfSlots{};
    sl->use = 1;
    for (int k = 0; k < bt.n; ++k) { if (bt.slot[k] < 0 || bt.slot[k] >= sp->batch) return false; sl->slot[k] = bt.slot[k]; }
    return true;
}
}  // namespace

namespace calipso {
bool sparse_is_multifrontal(const calipso_hip_sparse* sp) { return sp && sp->mf; }
// a plan owned by a solver handle is only ever driven on that handle's stream: give the plan's own stream back
void sparse_borrow_stream(calipso_hip_sparse* sp, hipStream_t st) {
    if (!sp) return;
    if (sp->owns_stream && sp->stream) { (void)hipStreamSynchronize(sp->stream); (void)hipStreamDestroy(sp->stream); }
    sp->stream = st; sp->owns_stream = false;
}
int sparse_batch(const calipso_hip_sparse* sp) { return sp ? sp->batch : 0; }
// the stream every call of the plan enqueues on: a handle that owns a plan (sparse_kkt.hip) orders its own kernels with it
hipStream_t sparse_stream(const calipso_hip_sparse* sp) { return sp ? sp->stream : nullptr; }
void sparse_values(calipso_hip_sparse* sp, double** values, long long* stride) { *values = sp ? sp->Aval.p : nullptr; *stride = sp ? (long long)sp->plan.nnzA : 0; }
// gather the pattern's entries from the dense S of every instance of `bt`, factor, add the pivot signs to the instances' counters
// values_in_place: the caller has written the pattern's entries into sparse_values() itself (structured handles: blocks.hip) — no gather
int sparse_factor_from_dense(calipso_hip_sparse* sp, hipStream_t st, const Batch& bt, const double* S, const long long* src, int* icount, bool values_in_place) {
    MfSlots sl;
    if (!sp || !sp->mf || !slots_of(sp, bt, &sl)) return CALIPSO_ERR_ARGUMENT;
    const unsigned nz = (unsigned)bt.n;
    if (!values_in_place) hipLaunchKernelGGL(k_gather_dense, dim3((unsigned)((sp->plan.nnzA + 255) / 256), 1, nz), dim3(256), 0, st, bt, S, src, (long long)sp->plan.nnzA, sp->Aval.p);
    mf_enqueue_factor(sp, st, sl, nz);
    if (icount) hipLaunchKernelGGL(k_count_signs, dim3(1, 1, nz), dim3(256), 0, st, bt, sp->D.p, sp->n, icount);      // (NULL: the caller counts by sparse_inertia_enqueue)
    sp->factored = true;
    return CALIPSO_OK;
}
// the reference's inertia of the factors of the matrices of `bt` into out[3 * slot ..] (device, batch x 3), in stream order: what calipso_hip_sparse_factorize returns
int sparse_inertia_enqueue(calipso_hip_sparse* sp, hipStream_t st, const Batch& bt, long long* out) {
    MfSlots sl;
    if (!sp || !sp->mf || !out || !slots_of(sp, bt, &sl)) return CALIPSO_ERR_ARGUMENT;
    hipLaunchKernelGGL(k_reference_inertia, dim3(1, 1, (unsigned)bt.n), dim3(IN_THREADS), 0, st, sl, sp->D.p, sp->n, out);
    return CALIPSO_OK;
}
// x <- S^-1 x for the first n entries of every instance's x (a slab buffer)
int sparse_solve_inplace(calipso_hip_sparse* sp, hipStream_t st, const Batch& bt, double* x) {
    MfSlots sl;
    if (!sp || !sp->mf || !slots_of(sp, bt, &sl)) return CALIPSO_ERR_ARGUMENT;
    const unsigned nz = (unsigned)bt.n, gx = (unsigned)((sp->n + 255) / 256);
    hipLaunchKernelGGL(k_permute_in_slab, dim3(gx, 1, nz), dim3(256), 0, st, bt, x, sp->d_perm, sp->n, sp->x.p);
    mf_enqueue_solve(sp, st, sl, nz, 1, sp->x.p);
    hipLaunchKernelGGL(k_permute_out_slab, dim3(gx, 1, nz), dim3(256), 0, st, bt, sp->x.p, sp->d_perm, sp->n, x);
    return CALIPSO_OK;
}
// X (ld x p, column-major, in the slab of the single instance `slot`) <- S^-1 X: all p right-hand sides through the tree in the same launches
int sparse_solve_inplace_multi(calipso_hip_sparse* s, hipStream_t st, int slot, double* X, long long ld, int p) {
    if (!s || !s->mf || slot < 0 || slot >= s->batch || p < 1 || p > 65535) return CALIPSO_ERR_ARGUMENT;
    const int rc = sparse_reserve_solve(s, p);
    if (rc != CALIPSO_OK) return rc;
    MfSlots sl{};
    sl.use = 1;
    // every column of the launch belongs to the same factor: with nrhs = p the kernels take slot[blockIdx.y / p] = slot[0]
    sl.slot[0] = slot;
    const unsigned gx = (unsigned)((s->n + 255) / 256), ny = (unsigned)p;
    hipLaunchKernelGGL(k_permute_in_cols, dim3(gx, ny), dim3(256), 0, st, X, ld, s->d_perm, s->n, s->x.p);
    mf_enqueue_solve(s, st, sl, ny, p, s->x.p);
    hipLaunchKernelGGL(k_permute_out_cols, dim3(gx, ny), dim3(256), 0, st, s->x.p, s->d_perm, s->n, X, ld);
    return CALIPSO_OK;
}
// buffers for solves of `cols` columns in all (instances x right-hand sides): afterwards a solve of that many allocates nothing
int sparse_reserve_solve(calipso_hip_sparse* s, int cols) {
    PK(hipSetDevice(s->device));
    const size_t C = (size_t)cols;
    const MfPlan* M = s->mf ? &*s->plan.mf : nullptr;
    int rc;
    if ((rc = device_grown(s, s->rhs, (size_t)s->n * C)) || (rc = device_grown(s, s->x, (size_t)s->n * C)) ||
        (rc = device_grown(s, s->uvec, M ? (size_t)std::max<long long>(M->usum, 1) * C : 0)) ||
        (rc = device_grown(s, s->wpart, M ? C * (size_t)M->wide_count * (size_t)M->wide_blocks * 64 : 0))) return rc;
    refresh_views(s);
    return CALIPSO_OK;
}
void sparse_work(const calipso_hip_sparse* sp, double out[3]) { out[0] = (double)sp->plan.R.flops; out[1] = (double)sp->plan.L.nnzL; out[2] = (double)sp->n; }
void sparse_describe(const calipso_hip_sparse* sp, int64_t out[4]) { out[0] = sp->plan.levels(); out[1] = sp->mf ? sp->plan.mf->max_front : 0; out[2] = sp->plan.A.nnzU; out[3] = sp->mf ? 2 : (sp->lds_acc ? 1 : 0); }
}  // namespace calipso

// (tests / A-B timing) how plans made AFTERWARDS treat fronts beyond the LDS: 1 = many workgroups per front (default), 0 = one; returns the old value
// (tests / A-B timing) whether plans made AFTERWARDS carry the extend-add items of the LDS fronts (1, default) or assemble child by child, row by row (0); returns the old value
extern "C" int32_t calipso_hip_debug_mf_items(int32_t on) { const int was = g_mf_items; if (on >= 0) g_mf_items = on != 0; return was; }
extern "C" int32_t calipso_hip_debug_wide_fronts(int32_t on) { const int was = g_wide_fronts; if (on >= 0) g_wide_fronts = on != 0; return was; }
#ifdef CALIPSO_LDL_TRACE
extern "C" int32_t calipso_hip_debug_mf_trace(long long* out, int32_t reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_mf_trace), sizeof(long long) * 64 * 12) != hipSuccess) return -1;
    int n = 0;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_mf_trace_n), sizeof(int)) != hipSuccess) return -1;
    if (reset) { const int z = 0; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_mf_trace_n), &z, sizeof(int)); }
    return n;
}
extern "C" int32_t calipso_hip_debug_mfs_trace(long long* out, int32_t reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_mfs_trace), sizeof(long long) * 128 * 8) != hipSuccess) return -1;
    int n = 0;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_mfs_trace_n), sizeof(int)) != hipSuccess) return -1;
    if (reset) { const int z = 0; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_mfs_trace_n), &z, sizeof(int)); }
    return n;
}
#endif

extern "C" {

const char* calipso_hip_sparse_last_error(calipso_hip_sparse* s) { return s ? s->err.c_str() : g_sparse_err.c_str(); }

int32_t calipso_hip_sparse_destroy(calipso_hip_sparse* s) {
    if (!s) return CALIPSO_OK;
    (void)hipSetDevice(s->device);
    if (s->stream && s->owns_stream) (void)hipStreamSynchronize(s->stream);
    if (s->graph_factor) (void)hipGraphExecDestroy(s->graph_factor);
    for (void* p : s->dev) if (p) (void)hipFree(p);
    if (s->e0) (void)hipEventDestroy(s->e0);
    if (s->e1) (void)hipEventDestroy(s->e1);
    if (s->stream && s->owns_stream) (void)hipStreamDestroy(s->stream);
    delete s;
    return CALIPSO_OK;
}

// QDLDL(A; perm) analyse phase (qdldl.jl:134-188): order, P A P', etree, pattern of L — plus the level schedule of the device factorisation.
// colptr / rowval: Julia SparseMatrixCSC pattern (1-based); only the upper triangle is read (triu!, linear_solver.jl:23).
// method: 0 natural, 1 RCM, 2 minimum degree, 4 nested dissection, 3 = `perm` (1-based, perm[k] = vertex eliminated k-th).
static int32_t sparse_create_impl(int64_t n, const int64_t* colptr, const int64_t* rowval, int32_t method, const int64_t* perm, int32_t device,
                                  calipso_hip_sparse** out);
int32_t calipso_hip_sparse_create(int64_t n, const int64_t* colptr, const int64_t* rowval, int32_t method, const int64_t* perm, int32_t device,
                                  calipso_hip_sparse** out) {
    if (!out) return CALIPSO_ERR_ARGUMENT;
    *out = nullptr;
    const int32_t rc = sparse_create_impl(n, colptr, rowval, method, perm, device, out);
    if (rc != CALIPSO_OK && *out) {             // a failure after the handle was made (stream, uploads, allocations): no half-built handle leaves here
        g_sparse_err = (*out)->err;
        (void)calipso_hip_sparse_destroy(*out);
        *out = nullptr;
    }
    return rc;
}
static int32_t sparse_create_impl(int64_t n, const int64_t* colptr, const int64_t* rowval, int32_t method, const int64_t* perm, int32_t device,
                                  calipso_hip_sparse** out) {
    calipso_hip_sparse* s = nullptr;
    if (n < 1 || n > 0x3fffffff || !colptr || method < 0 || method > 5 || (method == 3 && !perm)) {
        g_sparse_err = "calipso_hip_sparse_create: bad arguments"; return CALIPSO_ERR_ARGUMENT;
    }
    if (!calipso::csc_pattern_ok(n, colptr, rowval)) { g_sparse_err = "colptr must be 1-based (Julia SparseMatrixCSC) and non-decreasing, rowval in 1..n, nnz < 2^31"; return CALIPSO_ERR_ARGUMENT; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_sparse_err = "no HIP device available (libcalipso_hip has no CPU path)"; return CALIPSO_ERR_HIP; }
    if (device < 0 || device >= ndev) { g_sparse_err = "device ordinal out of range"; return CALIPSO_ERR_ARGUMENT; }
    // ---- order
    std::vector<i64> p((size_t)n);
    Pieces pieces;                                  // nested dissection: (first position, count) of every leaf piece / separator
    if (method == 3) {
        std::copy(perm, perm + n, p.begin());       // (analyse refuses what is not a permutation of 1:n)
    } else if (method >= 4) {
        const int rc = calipso::nested_dissection_pieces(n, colptr, rowval, p.data(), pieces);
        if (rc < 0) { g_sparse_err = "nested dissection failed"; return rc; }
    } else {
        const int rc = calipso_hip_ordering(n, colptr, rowval, method, p.data());
        if (rc < 0) { g_sparse_err = "calipso_hip_ordering failed"; return rc; }
    }
    if (method != 4) pieces.clear();                // the multifrontal numeric phase is method 4's; 5 keeps the dissection's order for the column method
    // ---- the analysis: every table of both numeric phases, on the host (sparse_plan.hpp)
    Limits lim = LIMITS;
    lim.wide_fronts = g_wide_fronts; lim.mf_items = g_mf_items;
    SparsePlan plan = analyse(n, colptr, rowval, std::move(p), pieces, lim);
    if (plan.status) { g_sparse_err = plan.message; return plan.status; }
    // ---- the handle and its device side
    s = new calipso_hip_sparse();
    *out = s;
    s->plan = std::move(plan);
    const SparsePlan& P = s->plan;
    s->n = (int)n; s->device = device; s->mf = P.mf.has_value();
    s->lds_acc = n <= SP_LDS_MAX_N;
    PK(hipSetDevice(device));
    PK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    PK(hipEventCreate(&s->e0)); PK(hipEventCreate(&s->e1));
    s->d.n = (int)n;
    int rc;
    std::vector<int> hperm((size_t)n);
    for (i64 k = 0; k < n; ++k) hperm[(size_t)k] = (int)(P.perm[(size_t)k] - 1);
    if ((rc = device_upload(s, P.cols.order, &s->d.order)) || (rc = device_upload(s, P.A.Alp, &s->d.Alp)) || (rc = device_upload(s, P.A.Ali, &s->d.Ali)) || (rc = device_upload(s, P.A.Asrc, &s->d.Asrc)) ||
        (rc = device_upload(s, P.L.Lp, &s->d.Lp)) || (rc = device_upload(s, P.L.Li, &s->d.Li)) || (rc = device_upload(s, P.R.Rp, &s->d.Rp)) || (rc = device_upload(s, P.R.Rk, &s->d.Rk)) ||
        (rc = device_upload(s, P.R.Rpos, &s->d.Rpos)) || (rc = device_upload(s, P.R.Rend, &s->d.Rend)) || (rc = device_upload(s, hperm, &s->d_perm))) return rc;
    if ((rc = alloc_values(s, 1))) return rc;
    if (s->mf) {
        const MfPlan& M = *P.mf;
        MfDev& md = s->md;
        md.nnodes = M.nnodes;
        if ((rc = device_upload(s, M.order, &md.order)) || (rc = device_upload(s, M.first, &md.nfirst)) || (rc = device_upload(s, M.cols, &md.ncols)) || (rc = device_upload(s, M.rows, &md.nrows)) ||
            (rc = device_upload(s, M.rowptr, &md.rowptr)) || (rc = device_upload(s, M.rowsv, &md.rows)) || (rc = device_upload(s, M.rel, &md.rel)) || (rc = device_upload(s, M.childptr, &md.childptr)) ||
            (rc = device_upload(s, M.children, &md.children)) || (rc = device_upload(s, M.panel_off, &md.panel_off)) || (rc = device_upload(s, M.upd_off, &md.upd_off)) ||
            (rc = device_upload(s, M.u_off, &md.u_off)) || (rc = device_upload(s, M.Aloc, &md.Aloc)) || (rc = device_upload(s, M.foff, &md.foff))) return rc;
        md.xit = nullptr;
        if ((rc = device_upload(s, M.nrec, &md.nrec)) || (rc = device_upload(s, M.crec, &md.crec)) || (!M.xit.empty() && (rc = device_upload(s, M.xit, &md.xit)))) return rc;
        if (M.wide_count && ((rc = device_upload(s, M.wptrE, &md.wptrE)) || (rc = device_upload(s, M.wptrC, &md.wptrC)) || (rc = device_upload(s, M.wEcol, &md.wEcol)) ||
                             (rc = device_upload(s, M.wEsrc, &md.wEsrc)) || (rc = device_upload(s, M.wC, &md.wC)))) return rc;
        for (const MfSeg& g : M.levels) if (g.wide.on && !mf_wide_prepare(&s->err)) return CALIPSO_ERR_HIP;
        md.Alp = s->d.Alp; md.Asrc = s->d.Asrc;
        for (const void* fn : {(const void*)k_mf_factor<256, false>, (const void*)k_mf_factor<512, false>, (const void*)k_mf_forward<256, false>,
                               (const void*)k_mf_forward<512, false>, (const void*)k_mf_backward<256, false>, (const void*)k_mf_backward<512, false>})
            PK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LIMITS.lds_budget));     // (k_mf_factor also holds 1 KiB of static LDS)
    }
    s->work_slots = std::min(P.cols.widest, 2048);
    if (s->lds_acc) {
        PK(hipFuncSetAttribute((const void*)k_sp_factor<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * SP_LDS_MAX_N)));
    } else {
        s->work_slots = std::min(s->work_slots, 512);
        if ((rc = device_fixed(s, &s->d.work, (size_t)s->work_slots * (size_t)n))) return rc;
    }
    return CALIPSO_OK;
}

// info = [n, nnz(triu A), nnz(L), levels of the elimination tree, launches per factorisation, widest level, multiply-adds per factorisation,
//         1 if the column accumulator lives in LDS]
int32_t calipso_hip_sparse_info(calipso_hip_sparse* s, int64_t info[8]) {
    if (!s || !info) return CALIPSO_ERR_ARGUMENT;
    const SparsePlan& P = s->plan;
    info[0] = s->n; info[1] = P.A.nnzU; info[2] = P.L.nnzL; info[3] = P.levels(); info[4] = s->mf ? (i64)P.mf->levels.size() : (i64)P.cols.plan.size(); info[5] = P.widest(); info[6] = P.R.flops; info[7] = s->mf ? 2 : (s->lds_acc ? 1 : 0);
    return CALIPSO_OK;
}

// Number of matrices (same pattern, different values) the following calls treat together: nzval = batch x nnz, inertia = batch x 3,
// b / x = batch x (n x nrhs).  The multifrontal path factors the whole batch in the same launches (one workgroup per front and matrix);
// the column method takes them one after the other.  Invalidates the current factorisation.
int32_t calipso_hip_sparse_set_batch(calipso_hip_sparse* s, int64_t batch) {
    if (!s || batch < 1 || batch > 65535) return CALIPSO_ERR_ARGUMENT;
    PK(hipSetDevice(s->device));
    PK(hipStreamSynchronize(s->stream));
    if (s->graph_factor) { (void)hipGraphExecDestroy(s->graph_factor); s->graph_factor = nullptr; }
    s->graph_tried = false;
    return alloc_values(s, (int)batch);
}
// which matrix of the batch calipso_hip_sparse_get_factor reads (default 0)
int32_t calipso_hip_sparse_select(calipso_hip_sparse* s, int64_t instance) {
    if (!s || instance < 0 || instance >= s->batch) return CALIPSO_ERR_ARGUMENT;
    s->selected = (int)instance;
    return CALIPSO_OK;
}

// QDLDL_factor! + compute_inertia! (qdldl.jl:400-589, linear_solver.jl:19-44) for new values on the analysed pattern.
// nzval: batch x nnz(A) values in the caller's CSC order (host).  inertia: batch x 3 (may be NULL).  Returns CALIPSO_WARN_ZERO_PIVOT if any
// matrix met an exact zero pivot (its inertia[0] = -1).
static int32_t sparse_factorize(calipso_hip_sparse* s, const double* nzval, int64_t* inertia, hipMemcpyKind kind) {
    if (!s || (!nzval && s->plan.nnzA > 0)) return CALIPSO_ERR_ARGUMENT;
    PK(hipSetDevice(s->device));
    const size_t B = (size_t)s->batch;
    if (s->plan.nnzA) PK(hipMemcpyAsync(s->Aval.p, nzval, sizeof(double) * B * (size_t)s->plan.nnzA, kind, s->stream));
    PK(hipEventRecord(s->e0, s->stream));
    if (!s->graph_tried) {          // the level schedule is a fixed launch sequence with fixed arguments: captured once, replayed afterwards
        s->graph_tried = true;
        hipGraph_t g = nullptr;
        if (hipStreamBeginCapture(s->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            enqueue_factor(s);
            if (hipStreamEndCapture(s->stream, &g) == hipSuccess && g) {
                if (hipGraphInstantiate(&s->graph_factor, g, nullptr, nullptr, 0) != hipSuccess) s->graph_factor = nullptr;
                (void)hipGraphDestroy(g);
            }
        }
        (void)hipGetLastError();
    }
    if (s->graph_factor) PK(hipGraphLaunch(s->graph_factor, s->stream));
    else enqueue_factor(s);
    PK(hipEventRecord(s->e1, s->stream));
    hipLaunchKernelGGL(k_reference_inertia, dim3(1, 1, (unsigned)B), dim3(IN_THREADS), 0, s->stream, MfSlots{}, s->D.p, s->n, s->inertia_dev.p);      // compute_inertia! as the reference sees it
    PK(hipMemcpyAsync(s->inertia_all.data(), s->inertia_dev.p, sizeof(long long) * 3 * B, hipMemcpyDeviceToHost, s->stream));
    PK(hipStreamSynchronize(s->stream));
    PK(hipGetLastError());
    float ms = 0.f; PK(hipEventElapsedTime(&ms, s->e0, s->e1)); s->ms_factor = ms;
    int rc = CALIPSO_OK;
    for (size_t z = 0; z < B; ++z) if (s->inertia_all[3 * z + 2] > 0) rc = CALIPSO_WARN_ZERO_PIVOT;
    s->factored = true;
    if (inertia) std::copy(s->inertia_all.begin(), s->inertia_all.end(), inertia);
    return rc;
}
int32_t calipso_hip_sparse_factorize(calipso_hip_sparse* s, const double* nzval, int64_t* inertia) { return sparse_factorize(s, nzval, inertia, hipMemcpyHostToDevice); }
// the same with the values already resident on the handle's device (d_nzval: device pointer, batch x nnz)
int32_t calipso_hip_sparse_factorize_device(calipso_hip_sparse* s, const double* d_nzval, int64_t* inertia) { return sparse_factorize(s, d_nzval, inertia, hipMemcpyDeviceToDevice); }

// solve!(F, b) (qdldl.jl:330-351) for nrhs right-hand sides per matrix: b, x = batch x (column-major n x nrhs) host arrays (may alias)
static int32_t sparse_solve(calipso_hip_sparse* s, int64_t nrhs, const double* b, double* x, hipMemcpyKind kin, hipMemcpyKind kout) {
    if (!s || nrhs < 0 || (nrhs > 0 && (!b || !x)) || nrhs * (int64_t)(s ? s->batch : 1) > 65535) return CALIPSO_ERR_ARGUMENT;
    if (!s->factored) { s->err = "calipso_hip_sparse_solve: factorize first"; return CALIPSO_ERR_ARGUMENT; }
    if (nrhs == 0) return CALIPSO_OK;
    PK(hipSetDevice(s->device));
    const size_t cols = (size_t)nrhs * (size_t)s->batch;
    const size_t need = (size_t)s->n * cols;
    if (const int rrc = calipso::sparse_reserve_solve(s, (int)cols)) return rrc;
    PK(hipMemcpyAsync(s->rhs.p, b, sizeof(double) * need, kin, s->stream));
    PK(hipEventRecord(s->e0, s->stream));
    const unsigned gx = (unsigned)((s->n + 255) / 256), ny = (unsigned)cols;
    hipLaunchKernelGGL(k_permute_in_cols, dim3(gx, ny), dim3(256), 0, s->stream, s->rhs.p, (long long)s->n, s->d_perm, s->n, s->x.p);          // permute!(x, perm)  qdldl.jl:333
    if (s->mf) {
        mf_enqueue_solve(s, s->stream, MfSlots{}, ny, (int)nrhs, s->x.p);
    } else {
        for (int z = 0; z < s->batch; ++z) {
            SpDev d = s->d;
            d.Lx += (size_t)z * (size_t)s->plan.L.nnzL; d.D += (size_t)z * (size_t)s->n;
            double* xz = s->x.p + (size_t)z * (size_t)nrhs * (size_t)s->n;
            for (const Segment& g : s->plan.cols.plan)
                hipLaunchKernelGGL(k_sp_forward, dim3(g.chain ? 1 : (unsigned)std::min(g.count, 4096), (unsigned)nrhs), dim3(64), 0, s->stream, d, g.first, g.count, xz);
            for (auto g = s->plan.cols.plan.rbegin(); g != s->plan.cols.plan.rend(); ++g)
                hipLaunchKernelGGL(k_sp_backward, dim3(g->chain ? 1 : (unsigned)std::min(g->count, 4096), (unsigned)nrhs), dim3(64), 0, s->stream, d, g->first, g->count, xz);
        }
    }
    hipLaunchKernelGGL(k_permute_out_cols, dim3(gx, ny), dim3(256), 0, s->stream, s->x.p, s->d_perm, s->n, s->rhs.p, (long long)s->n);         // ipermute!(x, perm) qdldl.jl:349
    PK(hipEventRecord(s->e1, s->stream));
    PK(hipMemcpyAsync(x, s->rhs.p, sizeof(double) * need, kout, s->stream));
    PK(hipStreamSynchronize(s->stream));
    PK(hipGetLastError());
    float ms = 0.f; PK(hipEventElapsedTime(&ms, s->e0, s->e1)); s->ms_solve = ms;
    return CALIPSO_OK;
}
int32_t calipso_hip_sparse_solve(calipso_hip_sparse* s, int64_t nrhs, const double* b, double* x) { return sparse_solve(s, nrhs, b, x, hipMemcpyHostToDevice, hipMemcpyDeviceToHost); }
// the same with right-hand sides and solutions resident on the handle's device (device pointers; may alias)
int32_t calipso_hip_sparse_solve_device(calipso_hip_sparse* s, int64_t nrhs, const double* d_b, double* d_x) { return sparse_solve(s, nrhs, d_b, d_x, hipMemcpyDeviceToDevice, hipMemcpyDeviceToDevice); }

// the factor for inspection: perm[n] (1-based), Lp[n+1], Li[nnz(L)] (1-based, strictly lower, rows ascending — F.L of qdldl.jl:160-166 without the
// unit diagonal), Lx[nnz(L)], D[n]; any output may be NULL
int32_t calipso_hip_sparse_get_factor(calipso_hip_sparse* s, int64_t* perm, int64_t* Lp, int64_t* Li, double* Lx, double* D) {
    if (!s) return CALIPSO_ERR_ARGUMENT;
    if ((Lx || D) && !s->factored) { s->err = "calipso_hip_sparse_get_factor: factorize first"; return CALIPSO_ERR_ARGUMENT; }
    PK(hipSetDevice(s->device));
    const std::vector<int>&hLp = s->plan.L.Lp, &hLi = s->plan.L.Li;
    const size_t nnzL = (size_t)s->plan.L.nnzL;
    if (perm) std::copy(s->plan.perm.begin(), s->plan.perm.end(), perm);
    if (Lp) for (size_t k = 0; k < hLp.size(); ++k) Lp[k] = (i64)hLp[k] + 1;
    if (Li) for (size_t k = 0; k < hLi.size(); ++k) Li[k] = (i64)hLi[k] + 1;
    if (Lx && nnzL && s->mf) {
        // multifrontal storage: dense m x c panels per node; pick the entries of the exact pattern out of them
        const MfPlan& M = *s->plan.mf;
        std::vector<double> panel((size_t)M.panel_total);
        PK(hipMemcpyAsync(panel.data(), s->panel.p + (size_t)s->selected * (size_t)M.panel_total, sizeof(double) * panel.size(), hipMemcpyDeviceToHost, s->stream));
        PK(hipStreamSynchronize(s->stream));
        for (int t = 0; t < M.nnodes; ++t) {
            const int f = M.first[(size_t)t], c = M.cols[(size_t)t], m = c + M.rows[(size_t)t];
            const int* Rb = M.rowsv.data() + M.rowptr[(size_t)t]; const int* Re = Rb + M.rows[(size_t)t];
            const double* Pn = panel.data() + M.panel_off[(size_t)t];
            for (int j = f; j < f + c; ++j)
                for (int q = hLp[(size_t)j]; q < hLp[(size_t)j + 1]; ++q) {
                    const int i = hLi[(size_t)q];
                    const int lr = i < f + c ? i - f : c + (int)(std::lower_bound(Rb, Re, i) - Rb);
                    Lx[q] = Pn[(size_t)lr + (size_t)(j - f) * m];
                }
        }
    } else
    if (Lx && nnzL) PK(hipMemcpyAsync(Lx, s->Lx.p + (size_t)s->selected * nnzL, sizeof(double) * nnzL, hipMemcpyDeviceToHost, s->stream));
    if (D) PK(hipMemcpyAsync(D, s->D.p + (size_t)s->selected * (size_t)s->n, sizeof(double) * (size_t)s->n, hipMemcpyDeviceToHost, s->stream));
    PK(hipStreamSynchronize(s->stream));
    return CALIPSO_OK;
}

// ms[0] = device time of the last factorisation (all level launches), ms[1] = of the last solve call; HIP events on the handle's stream
int32_t calipso_hip_sparse_timing(calipso_hip_sparse* s, double ms[2]) {
    if (!s || !ms) return CALIPSO_ERR_ARGUMENT;
    ms[0] = s->ms_factor; ms[1] = s->ms_solve;
    return CALIPSO_OK;
}

}  // extern "C"
