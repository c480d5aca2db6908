// sparse_plan.hpp — the analyse phase of the sparse LDL^T (sparse.hip) as plain host C++: no HIP header, so tests/sparse_plan_host/main.cpp can build
// every table on the CPU under the sanitizers.  From a pattern, an order and the pieces of a nested dissection: P A P' as a lower CSC with its gather
// map, the elimination tree, the pattern of L and its row view, the level plan of the column method, and the whole multifrontal plan (supernodes,
// row sets, relative indices, front offsets, the wide-front row tables, node / child records, extend-add items).  These tables hold every address
// k_mf_factor, the sweeps and sparse_wide.hpp load and store through; sparse.hip uploads them as they are.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <optional>
#include <string>
#include <utility>
#include <vector>

namespace calipso {
typedef int64_t i64;      // (as in calipso_options.hpp)
namespace sparse_plan {

// ---- what the kernels read (layouts fixed: the device code indexes these records) ----------------------------------------------------------------
// One record per node in LAUNCH order and one per (node, child): what a workgroup needs to find its front comes with ONE load each instead of a chain of
// dependent table look-ups (order -> nfirst / ncols / nrows -> childptr -> children -> upd_off / rowptr ...: 0.7 us per hop on a cold launch).
struct MfNode { int s, f, c, r; int rowptr, chfirst, nch, alp0; int alp1, pad0, pad1, pad2; long long panel_off, upd_off, u_off, foff; int xa0, xa1; };
// pad0: first row record of a front factored by many workgroups (sparse_wide.hpp; -1: none), pad1: launch position of the parent (-1: a root), pad2: the level's ypan
struct MfChild { int rc, rowptr; long long upd_off, u_off; int pos, pad; };   // pos: the child's launch position
// one entry of a child's update matrix on its way into the parent's LDS front (MfNode::xa0 .. xa1, children in ascending order, a child's lower triangle row by row):
// usrc = its offset in the instance's update pool, tq = its place in the parent's packed front | the child's ordinal << 16
struct MfXItem { unsigned usrc, tq; };
struct MfRowItem { long long uoff; int relptr, a, uo, pad; };   // row a of a child's update matrix (offset in the update pool), the child's relative indices, the row's entry of the child's vector (solves)
struct MfWide { int on = 0; int m = 0, r = 0, nch = 0; int solve = 0; };   // what a level's launches must cover (maxima over its nodes); solve: the sweeps of this level by many workgroups too
struct MfSeg { int first, count; size_t lds_factor, lds_solve; int threads; bool global; int ypan; MfWide wide; };   // ypan: room for the 64 x py exchange rows of the in-register panels
struct Segment { int first, count; bool chain; };
static_assert(sizeof(MfNode) == 88 && sizeof(MfChild) == 32 && sizeof(MfXItem) == 8 && sizeof(MfRowItem) == 24, "records the kernels load whole");
static_assert(sizeof(MfWide) == 20 && sizeof(MfSeg) == 56 && sizeof(Segment) == 12, "launch descriptors");

// ---- the limits: one definition of each (sparse.hip and sparse_wide.hpp take their constants from a default-constructed Limits) -------------------
struct Limits {
    int max_front = 196;                        // (m (m + 1) / 2 + 2 m) doubles <= 160 KiB: the front's lower triangle, packed, + the pivot-column buffers
    int max_front_wide = 8192;                  // fronts factored and solved by many workgroups (sparse_wide.hpp); beyond: the column method
    int max_front_global = 4095;                // the ONE-workgroup kernels on fronts in global memory (wide_fronts = 0: the A/B reference of sparse_wide.hpp): same algorithm
                                                // as in LDS, every access a memory access (a 1500-row front is ~2 ms); 4095 is where the 24-bit index arithmetic of the packed triangle ends
    int big = 96;                               // threads per front: 256 for small fronts (several workgroups share a CU), 512 for fronts of more than `big` rows
    int py = 18;                                // row stride of the exchange rows of an in-register panel (pivot16.hpp)
    size_t lds_budget = 160 * 1024 - 2048;      // dynamic LDS of a front's workgroup (k_mf_factor also holds 1 KiB of static LDS)
    int lds_max_n = 19400;                      // column method: 155 200 B of the CU's 160 KiB LDS for the accumulator (4 KiB of record stage beside it)
    int wide_solve_m = 2048, wide_solve_nch = 4;// the sweeps of a level by many workgroups too: fronts beyond this many rows (measured cross-over: ~2200), or nodes with more children
    int wf_solve_rows = 1024;                   // rows of L21 per workgroup of the backward sweep's partial products (sparse_wide.hpp)
    long long max_pool = 1ll << 31;             // update matrices + panels per matrix, in doubles (16 GiB): the column method beyond
    size_t max_item_bytes = (size_t)512 << 20;  // the extend-add items: not built beyond 512 MiB ...
    int max_item_children = 65535;              // ... or when a node has more children than the 16 bits of an item's ordinal hold (the row-wise loop then)
    int wide_fronts = 1;                        // fronts beyond the LDS by many workgroups (1) or by one (0)
    int mf_items = 1;                           // extend-add items for the LDS fronts (1) or the assembly child by child, row by row (0)
};

constexpr int REFUSED_ARGUMENT = -4;            // CALIPSO_ERR_ARGUMENT (sparse.hip asserts the value)
struct Refusal { int status = 0; std::string message; };
typedef std::vector<std::pair<int, int>> Pieces;   // nested dissection: (first position, count) of every leaf piece / separator

// ---- the column tables ---------------------------------------------------------------------------------------------------------------------------
struct LowerCsc { std::vector<int> Alp, Ali, Asrc; i64 nnzU = 0; };                       // P A P' lower (diagonal included, rows ascending), Asrc = index into the caller's nzval
struct LPattern { std::vector<int> Lp, Li; i64 nnzL = 0; };                               // strictly lower pattern of L, rows ascending
struct RowView { std::vector<int> Rp, Rk, Rpos, Rend; i64 flops = 0; };                   // for row j the columns k < j with L(j,k) != 0 (ascending), the slot of L(j,k), the end of column k
struct ColumnLevels { std::vector<int> order; std::vector<Segment> plan; int height = 0, widest = 0; };   // columns sorted by (level, index), a launch per level (chains merged)

// P A P' as a lower CSC (rows ascending), with the gather map from the caller's nzval; lowrow = row view of the strictly lower part: columns i < j of row j
inline LowerCsc permuted_lower_csc(i64 n, const i64* colptr, const i64* rowval, const std::vector<int>& ip, std::vector<std::vector<int>>& lowrow, Refusal& no) {
    LowerCsc A;
    std::vector<std::vector<std::pair<int, int>>> col((size_t)n);       // (row, source index)
    for (i64 c = 0; c < n; ++c)
        for (i64 q = colptr[c] - 1; q < colptr[c + 1] - 1; ++q) {
            const i64 r = rowval[q] - 1;
            if (r < 0 || r >= n) { no = {REFUSED_ARGUMENT, "row index out of range"}; return A; }
            if (r > c) continue;
            const int pr = ip[(size_t)r], pc = ip[(size_t)c];
            col[(size_t)std::min(pr, pc)].push_back({std::max(pr, pc), (int)q});
            ++A.nnzU;
        }
    A.Alp.assign((size_t)n + 1, 0);
    A.Ali.reserve((size_t)A.nnzU); A.Asrc.reserve((size_t)A.nnzU);
    lowrow.assign((size_t)n, {});
    for (int j = 0; j < (int)n; ++j) {
        auto& cj = col[(size_t)j];
        std::sort(cj.begin(), cj.end());
        for (size_t a = 1; a < cj.size(); ++a) if (cj[a].first == cj[a - 1].first) { no = {REFUSED_ARGUMENT, "duplicate entry in the CSC pattern"}; return A; }
        for (auto& e : cj) { A.Ali.push_back(e.first); A.Asrc.push_back(e.second); if (e.first > j) lowrow[(size_t)e.first].push_back(j); }
        A.Alp[(size_t)j + 1] = (int)A.Ali.size();
    }
    // QDLDL_etree! refuses a matrix with an empty column of the upper triangle (qdldl.jl:366-371): column j of triu(P A P') = row j of the lower part + diagonal
    for (int j = 0; j < (int)n; ++j) {
        const bool diag = A.Alp[(size_t)j] < A.Alp[(size_t)j + 1] && A.Ali[(size_t)A.Alp[(size_t)j]] == j;
        if (!diag && lowrow[(size_t)j].empty()) { no = {REFUSED_ARGUMENT, "empty column in triu(A): QDLDL_etree! fails on this matrix (qdldl.jl:366-371)"}; return A; }
    }
    return A;
}

// elimination tree (Liu, path compression); -1 = root
inline std::vector<int> elimination_tree(i64 n, const std::vector<std::vector<int>>& lowrow) {
    std::vector<int> parent((size_t)n, -1), anc((size_t)n, -1);
    for (int j = 0; j < (int)n; ++j)
        for (int i0 : lowrow[(size_t)j]) {
            int i = i0;
            while (i != -1 && i < j) { const int nxt = anc[(size_t)i]; anc[(size_t)i] = j; if (nxt == -1) parent[(size_t)i] = j; i = nxt; }
        }
    return parent;
}

// pattern of L: struct(L_j) = struct(A_j below the diagonal) U (struct(L_c) \ {j}) over the children c of j
inline LPattern pattern_of_L(i64 n, const LowerCsc& A, const std::vector<int>& parent, Refusal& no) {
    LPattern L;
    std::vector<std::vector<int>> children((size_t)n);
    for (int j = 0; j < (int)n; ++j) if (parent[(size_t)j] >= 0) children[(size_t)parent[(size_t)j]].push_back(j);
    std::vector<std::vector<int>> Lcol((size_t)n);
    std::vector<int> mark((size_t)n, -1);
    for (int j = 0; j < (int)n; ++j) {
        std::vector<int>& lj = Lcol[(size_t)j];
        mark[(size_t)j] = j;
        for (int q = A.Alp[(size_t)j]; q < A.Alp[(size_t)j + 1]; ++q) { const int r = A.Ali[(size_t)q]; if (r > j && mark[(size_t)r] != j) { mark[(size_t)r] = j; lj.push_back(r); } }
        for (int c : children[(size_t)j]) for (int r : Lcol[(size_t)c]) if (r != j && mark[(size_t)r] != j) { mark[(size_t)r] = j; lj.push_back(r); }
        std::sort(lj.begin(), lj.end());
        L.nnzL += (i64)lj.size();
        if (L.nnzL > 0x7fffffff) { no = {REFUSED_ARGUMENT, "nnz(L) exceeds 2^31 - 1"}; return L; }
    }
    L.Lp.assign((size_t)n + 1, 0); L.Li.reserve((size_t)L.nnzL);
    for (int j = 0; j < (int)n; ++j) { L.Li.insert(L.Li.end(), Lcol[(size_t)j].begin(), Lcol[(size_t)j].end()); L.Lp[(size_t)j + 1] = (int)L.Li.size(); }
    return L;
}

inline RowView row_view(i64 n, const LPattern& L) {
    RowView R;
    R.Rp.assign((size_t)n + 1, 0);
    for (int v : L.Li) R.Rp[(size_t)v + 1] += 1;
    for (int j = 0; j < (int)n; ++j) R.Rp[(size_t)j + 1] += R.Rp[(size_t)j];
    R.Rk.resize((size_t)L.nnzL); R.Rpos.resize((size_t)L.nnzL); R.Rend.resize((size_t)L.nnzL);
    std::vector<int> nextr(R.Rp.begin(), R.Rp.end() - 1);
    for (int k = 0; k < (int)n; ++k)
        for (int q = L.Lp[(size_t)k]; q < L.Lp[(size_t)k + 1]; ++q) {
            const int at = nextr[(size_t)L.Li[(size_t)q]]++;
            R.Rk[(size_t)at] = k; R.Rpos[(size_t)at] = q; R.Rend[(size_t)at] = L.Lp[(size_t)k + 1];
            R.flops += (i64)(L.Lp[(size_t)k + 1] - q);
        }
    return R;
}

// levels of the tree (level(j) = 1 + max level of j's children) and the launch plan of the column method
inline ColumnLevels column_levels(i64 n, const std::vector<int>& parent) {
    ColumnLevels C;
    std::vector<int> level((size_t)n, 0);
    for (int j = 0; j < (int)n; ++j) {          // children have smaller indices: one ascending pass
        if (parent[(size_t)j] >= 0) level[(size_t)parent[(size_t)j]] = std::max(level[(size_t)parent[(size_t)j]], level[(size_t)j] + 1);
        C.height = std::max(C.height, level[(size_t)j] + 1);
    }
    C.order.resize((size_t)n);
    std::iota(C.order.begin(), C.order.end(), 0);
    std::stable_sort(C.order.begin(), C.order.end(), [&](int a, int b) { return level[(size_t)a] < level[(size_t)b]; });
    for (int a = 0; a < (int)n;) {
        int b = a;
        while (b < (int)n && level[(size_t)C.order[(size_t)b]] == level[(size_t)C.order[(size_t)a]]) ++b;
        const int cnt = b - a;
        C.widest = std::max(C.widest, cnt);
        if (cnt == 1 && !C.plan.empty() && C.plan.back().chain) C.plan.back().count += 1;        // extend the chain of single-column levels
        else C.plan.push_back({a, cnt, cnt == 1});
        a = b;
    }
    return C;
}

// ---- the multifrontal plan -----------------------------------------------------------------------------------------------------------------------
// The pieces of the dissection as SUPERNODES: node t owns the contiguous columns [first, first + cols) and the rows R_t below them.
struct MfPlan {
    int nnodes = 0, max_front = 0, widest = 0;           // widest: most nodes of one level
    int width = 0; bool last_resort = false;             // the route: the chunk width accepted, or the last resort (fronts beyond Limits::max_front in global memory)
    std::vector<int> first, cols, rows, parent;          // per node: first column, c, r, parent node (-1: a root)
    std::vector<int> rowptr, rowsv;                      // R_t (global, permuted row indices), ascending
    std::vector<int> rel;                                // aligned with rowsv: local index of R_t[k] in the PARENT's front
    std::vector<int> childptr, children, order;          // children ascending; nodes sorted by level
    std::vector<int> Aloc;                               // per entry of the permuted lower CSC: offset inside its node's packed front (row (row + 1) / 2 + column)
    std::vector<long long> panel_off, upd_off, u_off;
    std::vector<long long> foff;                         // offset of a global-memory front in the pool (levels reuse the pool)
    std::vector<MfSeg> levels;                           // a launch per level of the node tree
    long long panel_total = 0, upd_total = 0, usum = 0, pool_total = 0;
    std::vector<int> wbase, wptrE, wptrC, wEcol, wEsrc;  // fronts factored by many workgroups (sparse_wide.hpp): per row its entries of A and its child rows
    std::vector<MfRowItem> wC;
    int wide_count = 0;                                  // most such fronts of one level
    int wide_blocks = 1;                                 // most row blocks of such a front in the backward sweep
    std::vector<MfNode> nrec;                            // [launch position]
    std::vector<MfChild> crec;                           // [chfirst + q]
    std::vector<MfXItem> xit;                            // extend-add items of the LDS fronts (empty: none)
};

// One attempt, from nothing: the pieces cut into chunks of <= width columns; a complete plan, or nothing when a front exceeds front_limit (or the
// update matrices and panels exceed max_pool, or the pieces do not cover the columns).
inline std::optional<MfPlan> multifrontal_attempt(i64 n, const LowerCsc& A, const LPattern& L, const Pieces& base_pieces, int width, int front_limit, const Limits& lim) {
    MfPlan M;
    const std::vector<int>&Alp = A.Alp, &Ali = A.Ali, &Asrc = A.Asrc;
    Pieces pieces;
    for (const auto& bp : base_pieces) for (int o = 0; o < bp.second; o += width) pieces.push_back({bp.first + o, std::min(width, bp.second - o)});
    const int NN = M.nnodes = (int)pieces.size();
    std::vector<int> node_of((size_t)n, -1);
    for (int t = 0; t < NN; ++t) for (int q = 0; q < pieces[(size_t)t].second; ++q) node_of[(size_t)(pieces[(size_t)t].first + q)] = t;
    for (int j = 0; j < (int)n; ++j) if (node_of[(size_t)j] < 0) return std::nullopt;
    std::vector<std::vector<int>> R((size_t)NN);
    M.parent.assign((size_t)NN, -1);
    std::vector<int> stamp((size_t)n, -1);
    for (int t = 0; t < NN; ++t) {
        // rows below the node reached from any of its columns, plus what the children passed up (already in R[t])
        const int f = pieces[(size_t)t].first, c = pieces[(size_t)t].second, last = f + c - 1;
        std::vector<int>& rt = R[(size_t)t];
        for (int v : rt) stamp[(size_t)v] = t;
        for (int j = f; j <= last; ++j) for (int q = L.Lp[(size_t)j]; q < L.Lp[(size_t)j + 1]; ++q) { const int i = L.Li[(size_t)q]; if (i > last && stamp[(size_t)i] != t) { stamp[(size_t)i] = t; rt.push_back(i); } }
        std::sort(rt.begin(), rt.end());
        M.max_front = std::max(M.max_front, c + (int)rt.size());
        if (!rt.empty()) {
            const int par = node_of[(size_t)rt[0]];
            M.parent[(size_t)t] = par;
            const int pl = pieces[(size_t)par].first + pieces[(size_t)par].second - 1;
            std::vector<int>& rp = R[(size_t)par];                  // closure: what the parent does not own it must carry on
            for (int v : rt) if (v > pl) rp.push_back(v);
            std::sort(rp.begin(), rp.end()); rp.erase(std::unique(rp.begin(), rp.end()), rp.end());
        }
    }
    if (M.max_front > front_limit) return std::nullopt;             // a front that does not fit: next chunk width / global fronts / column method
    M.first.resize((size_t)NN); M.cols.resize((size_t)NN); M.rows.resize((size_t)NN); M.rowptr.assign((size_t)NN + 1, 0);
    M.panel_off.resize((size_t)NN); M.upd_off.resize((size_t)NN); M.u_off.resize((size_t)NN);
    for (int t = 0; t < NN; ++t) {
        const int c = pieces[(size_t)t].second, r = (int)R[(size_t)t].size();
        M.first[(size_t)t] = pieces[(size_t)t].first; M.cols[(size_t)t] = c; M.rows[(size_t)t] = r;
        M.rowptr[(size_t)t + 1] = M.rowptr[(size_t)t] + r;
        M.panel_off[(size_t)t] = M.panel_total; M.panel_total += (long long)(c + r) * c;
        M.upd_off[(size_t)t] = M.upd_total; M.upd_total += (long long)r * r;
        M.u_off[(size_t)t] = M.usum; M.usum += r;
        M.rowsv.insert(M.rowsv.end(), R[(size_t)t].begin(), R[(size_t)t].end());
    }
    if (M.upd_total + M.panel_total > lim.max_pool) return std::nullopt;
    // relative indices into the parent's front, children lists, levels
    M.rel.assign(M.rowsv.size(), 0);
    std::vector<std::vector<int>> kids((size_t)NN);
    std::vector<int> lev((size_t)NN, 0);
    for (int t = 0; t < NN; ++t) {
        const int par = M.parent[(size_t)t];
        if (par < 0) continue;
        kids[(size_t)par].push_back(t);
        lev[(size_t)par] = std::max(lev[(size_t)par], lev[(size_t)t] + 1);      // children precede parents in position order
        const int pf = M.first[(size_t)par], pc = M.cols[(size_t)par];
        const std::vector<int>& rp = R[(size_t)par];
        for (int k = 0; k < M.rows[(size_t)t]; ++k) {
            const int v = R[(size_t)t][(size_t)k];
            M.rel[(size_t)M.rowptr[(size_t)t] + (size_t)k] = v < pf + pc ? v - pf : pc + (int)(std::lower_bound(rp.begin(), rp.end(), v) - rp.begin());
        }
    }
    M.childptr.assign((size_t)NN + 1, 0);
    for (int t = 0; t < NN; ++t) { M.childptr[(size_t)t + 1] = M.childptr[(size_t)t] + (int)kids[(size_t)t].size(); M.children.insert(M.children.end(), kids[(size_t)t].begin(), kids[(size_t)t].end()); }
    // where each entry of the permuted lower CSC lands in its node's front
    M.Aloc.assign(Ali.size(), 0);
    for (int j = 0; j < (int)n; ++j) {
        const int t = node_of[(size_t)j], f = M.first[(size_t)t], c = M.cols[(size_t)t];
        const std::vector<int>& rt = R[(size_t)t];
        for (int q = Alp[(size_t)j]; q < Alp[(size_t)j + 1]; ++q) {
            const int i = Ali[(size_t)q];
            const int lr = i < f + c ? i - f : c + (int)(std::lower_bound(rt.begin(), rt.end(), i) - rt.begin());
            M.Aloc[(size_t)q] = lr * (lr + 1) / 2 + (j - f);          // packed lower triangle (k_mf_factor: tri)
        }
    }
    M.order.resize((size_t)NN);
    M.foff.assign((size_t)NN, 0);
    M.wbase.assign((size_t)NN, -1);
    std::iota(M.order.begin(), M.order.end(), 0);
    std::stable_sort(M.order.begin(), M.order.end(), [&](int a, int b) { return lev[(size_t)a] < lev[(size_t)b]; });
    for (int a = 0; a < NN;) {
        int b = a; size_t lf = 0, ls = 0, mmax = 0;
        while (b < NN && lev[(size_t)M.order[(size_t)b]] == lev[(size_t)M.order[(size_t)a]]) {
            const int t = M.order[(size_t)b]; const size_t m = (size_t)(M.cols[(size_t)t] + M.rows[(size_t)t]);
            lf = std::max(lf, sizeof(double) * (m * (m + 1) / 2 + 2 * m)); ls = std::max(ls, sizeof(double) * 5 * m);   // the vector + four slices of partial sums per row
            mmax = std::max(mmax, m);
            ++b;
        }
        const bool glob = mmax > (size_t)lim.max_front;
        if (glob) {                                               // the level's fronts in the (reused) global pool; the solves keep only v in LDS
            long long off = 0;
            for (int q = a; q < b; ++q) { const int t = M.order[(size_t)q]; const long long mm = M.cols[(size_t)t] + M.rows[(size_t)t]; M.foff[(size_t)t] = off; off += mm * (mm + 1) / 2; }
            M.pool_total = std::max(M.pool_total, off);
            lf = 0;
        }
        int ypan = 0;                                             // full 16-column panels of fronts with >= 32 rows go through registers (pivot16.hpp) when the LDS has room for the exchange rows
        if (!glob && mmax >= 32 && lf + sizeof(double) * 64 * lim.py <= lim.lds_budget) { ypan = 1; lf += sizeof(double) * 64 * lim.py; }
        MfWide wide;                                              // fronts beyond the LDS: many workgroups per front (sparse_wide.hpp)
        if (glob && lim.wide_fronts) {
            wide.on = 1;
            M.wide_count = std::max(M.wide_count, b - a);
            for (int q = a; q < b; ++q) {
                const int t = M.order[(size_t)q], f = M.first[(size_t)t], c = M.cols[(size_t)t], r = M.rows[(size_t)t], mm = c + r;
                wide.m = std::max(wide.m, mm); wide.r = std::max(wide.r, r); wide.nch = std::max(wide.nch, (int)kids[(size_t)t].size());
                // per row of the front: its entries of A (any order: distinct targets) and the child rows that land in it, children ascending
                const int base = (int)M.wptrE.size();
                M.wbase[(size_t)t] = base;
                std::vector<int> cntE((size_t)mm + 1, 0), cntC((size_t)mm + 1, 0);
                const std::vector<int>& rt = R[(size_t)t];
                auto local = [&](int i) { return i < f + c ? i - f : c + (int)(std::lower_bound(rt.begin(), rt.end(), i) - rt.begin()); };
                for (int j = f; j < f + c; ++j) for (int e = Alp[(size_t)j]; e < Alp[(size_t)j + 1]; ++e) ++cntE[(size_t)local(Ali[(size_t)e]) + 1];
                for (int ch : kids[(size_t)t]) for (int k = 0; k < M.rows[(size_t)ch]; ++k) ++cntC[(size_t)M.rel[(size_t)M.rowptr[(size_t)ch] + (size_t)k] + 1];
                const int e0 = (int)M.wEcol.size(), c0 = (int)M.wC.size();
                for (int i = 0; i < mm; ++i) { cntE[(size_t)i + 1] += cntE[(size_t)i]; cntC[(size_t)i + 1] += cntC[(size_t)i]; }
                for (int i = 0; i <= mm; ++i) { M.wptrE.push_back(e0 + cntE[(size_t)i]); M.wptrC.push_back(c0 + cntC[(size_t)i]); }
                M.wEcol.resize((size_t)e0 + (size_t)cntE[(size_t)mm]); M.wEsrc.resize(M.wEcol.size()); M.wC.resize((size_t)c0 + (size_t)cntC[(size_t)mm]);
                std::vector<int> atE(cntE.begin(), cntE.end() - 1), atC(cntC.begin(), cntC.end() - 1);
                for (int j = f; j < f + c; ++j) for (int e = Alp[(size_t)j]; e < Alp[(size_t)j + 1]; ++e) {
                    const int at = e0 + atE[(size_t)local(Ali[(size_t)e])]++;
                    M.wEcol[(size_t)at] = j - f; M.wEsrc[(size_t)at] = Asrc[(size_t)e];
                }
                for (int ch : kids[(size_t)t]) for (int k = 0; k < M.rows[(size_t)ch]; ++k) {       // kids are ascending: so is every row's item list
                    const int at = c0 + atC[(size_t)M.rel[(size_t)M.rowptr[(size_t)ch] + (size_t)k]]++;
                    M.wC[(size_t)at] = {M.upd_off[(size_t)ch] + (long long)k * M.rows[(size_t)ch], M.rowptr[(size_t)ch], k, (int)(M.u_off[(size_t)ch] + k), 0};
                }
            }
        }
        wide.solve = wide.on && (wide.m > lim.wide_solve_m || wide.nch > lim.wide_solve_nch);
        if (wide.solve) M.wide_blocks = std::max(M.wide_blocks, (wide.r + lim.wf_solve_rows - 1) / lim.wf_solve_rows);
        M.levels.push_back({a, b - a, lf, ls, mmax > (size_t)lim.big ? 512 : 256, glob, ypan, wide});
        M.widest = std::max(M.widest, b - a);
        a = b;
    }
    // the node and child records
    M.nrec.resize((size_t)NN);
    std::vector<int> pos_of((size_t)NN, 0), ypan_of((size_t)NN, 0);
    for (int pos = 0; pos < NN; ++pos) pos_of[(size_t)M.order[(size_t)pos]] = pos;
    for (const MfSeg& g : M.levels) for (int q = 0; q < g.count; ++q) ypan_of[(size_t)(g.first + q)] = g.ypan;
    for (int pos = 0; pos < NN; ++pos) {
        const int t = M.order[(size_t)pos];
        MfNode& nd = M.nrec[(size_t)pos];
        nd.s = t; nd.f = M.first[(size_t)t]; nd.c = M.cols[(size_t)t]; nd.r = M.rows[(size_t)t];
        nd.rowptr = M.rowptr[(size_t)t]; nd.chfirst = (int)M.crec.size(); nd.nch = M.childptr[(size_t)t + 1] - M.childptr[(size_t)t];
        nd.alp0 = (int)Alp[(size_t)nd.f]; nd.alp1 = (int)Alp[(size_t)(nd.f + nd.c)]; nd.pad0 = M.wbase[(size_t)t];
        nd.pad1 = M.parent[(size_t)t] >= 0 ? pos_of[(size_t)M.parent[(size_t)t]] : -1; nd.pad2 = ypan_of[(size_t)pos];
        nd.panel_off = M.panel_off[(size_t)t]; nd.upd_off = M.upd_off[(size_t)t]; nd.u_off = M.u_off[(size_t)t]; nd.foff = M.foff[(size_t)t];
        for (int q = M.childptr[(size_t)t]; q < M.childptr[(size_t)t + 1]; ++q) {
            const int ch = M.children[(size_t)q];
            M.crec.push_back({M.rows[(size_t)ch], M.rowptr[(size_t)ch], M.upd_off[(size_t)ch], M.u_off[(size_t)ch], pos_of[(size_t)ch], 0});
        }
    }
    // extend-add items of the fronts that live in LDS (k_mf_factor's assembly): per node the entries of its children's update matrices, children ascending, a
    // child's lower triangle row by row; not built when a node has more than max_item_children children or the table would exceed max_item_bytes (the row-wise loop then)
    std::vector<char> lds_front((size_t)NN, 0);
    for (const MfSeg& g : M.levels) for (int q = 0; q < g.count; ++q) lds_front[(size_t)(g.first + q)] = !g.global;
    size_t total = 0; bool ok = true;
    for (int pos = 0; pos < NN && ok; ++pos) {
        if (!lds_front[(size_t)pos]) continue;
        const int t = M.order[(size_t)pos];
        if (M.childptr[(size_t)t + 1] - M.childptr[(size_t)t] > lim.max_item_children) ok = false;
        for (int q = M.childptr[(size_t)t]; q < M.childptr[(size_t)t + 1]; ++q) { const size_t rch = (size_t)M.rows[(size_t)M.children[(size_t)q]]; total += rch * (rch + 1) / 2; }
    }
    if (ok && lim.mf_items && total <= lim.max_item_bytes / sizeof(MfXItem)) {
        M.xit.reserve(total + 1);
        for (int pos = 0; pos < NN; ++pos) {
            MfNode& nd = M.nrec[(size_t)pos];
            nd.xa0 = nd.xa1 = -1;
            if (!lds_front[(size_t)pos]) continue;
            const int t = M.order[(size_t)pos];
            nd.xa0 = (int)M.xit.size();
            for (int q = M.childptr[(size_t)t]; q < M.childptr[(size_t)t + 1]; ++q) {
                const int ch = M.children[(size_t)q], rch = M.rows[(size_t)ch];
                const int* rel = M.rel.data() + M.rowptr[(size_t)ch];
                const unsigned ord = (unsigned)(q - M.childptr[(size_t)t]);
                for (int a = 0; a < rch; ++a) for (int b = 0; b <= a; ++b)
                    M.xit.push_back({(unsigned)(M.upd_off[(size_t)ch] + (long long)a * rch + b), (unsigned)(rel[a] * (rel[a] + 1) / 2 + rel[b]) | (ord << 16)});
            }
            nd.xa1 = (int)M.xit.size();
        }
        if (M.xit.empty()) M.xit.push_back({0u, 0u});
    } else for (MfNode& nd : M.nrec) nd.xa0 = nd.xa1 = -1;
    return M;
}

// A piece the level structure could not split (a clique-like stage block) or a wide separator is cut into a chain of chunks of <= w columns;
// w is lowered until every front (chunk + its rows below) fits one CU's LDS — e.g. 56 for stages of 56 variables, where chunks that straddle
// two stages would carry both stages' neighbours.  Last resort: chunks of 64 columns with the oversized fronts in global memory.
inline std::optional<MfPlan> multifrontal_plan(i64 n, const LowerCsc& A, const LPattern& L, const Pieces& base_pieces, const Limits& lim) {
    if (base_pieces.empty()) return std::nullopt;
    for (int width : {64, 56, 48, 40, 32, 24, 16})
        if (auto M = multifrontal_attempt(n, A, L, base_pieces, width, lim.max_front, lim)) { M->width = width; return M; }
    auto M = multifrontal_attempt(n, A, L, base_pieces, 64, lim.wide_fronts ? lim.max_front_wide : lim.max_front_global, lim);
    if (M) { M->width = 64; M->last_resort = true; }
    return M;
}

// ---- the whole analysis --------------------------------------------------------------------------------------------------------------------------
struct SparsePlan {
    int status = 0; std::string message;         // a refusal: nothing else is filled
    i64 n = 0, nnzA = 0;
    std::vector<i64> perm;                       // 1-based, perm[k] = vertex eliminated k-th
    LowerCsc A;
    std::vector<int> parent;
    LPattern L;
    RowView R;
    ColumnLevels cols;
    std::optional<MfPlan> mf;                    // the multifrontal numeric phase (a dissection whose fronts fit); the column method otherwise
    int levels() const { return mf ? (int)mf->levels.size() : cols.height; }
    int widest() const { return mf ? mf->widest : cols.widest; }
};

// colptr / rowval: a checked 1-based CSC pattern (ordering.hpp: csc_pattern_ok) of which the upper triangle is read; p: the order (1-based), chosen
// by the caller; pieces: those of the nested dissection that made p (empty: no multifrontal plan)
inline SparsePlan analyse(i64 n, const i64* colptr, const i64* rowval, std::vector<i64> p, const Pieces& pieces, const Limits& lim) {
    SparsePlan S;
    auto refuse = [](Refusal no) { SparsePlan r; r.status = no.status; r.message = std::move(no.message); return r; };
    std::vector<int> ip((size_t)n, -1);
    if ((i64)p.size() != n) return refuse({REFUSED_ARGUMENT, "perm is not a permutation of 1:n"});
    for (i64 k = 0; k < n; ++k) {
        const i64 v = p[(size_t)k];
        if (v < 1 || v > n || ip[(size_t)v - 1] >= 0) return refuse({REFUSED_ARGUMENT, "perm is not a permutation of 1:n"});
        ip[(size_t)v - 1] = (int)k;
    }
    Refusal no;
    std::vector<std::vector<int>> lowrow;
    S.n = n; S.nnzA = colptr[n] - 1;
    S.A = permuted_lower_csc(n, colptr, rowval, ip, lowrow, no);
    if (no.status) return refuse(std::move(no));
    S.parent = elimination_tree(n, lowrow);
    S.L = pattern_of_L(n, S.A, S.parent, no);
    if (no.status) return refuse(std::move(no));
    S.R = row_view(n, S.L);
    S.cols = column_levels(n, S.parent);
    S.mf = multifrontal_plan(n, S.A, S.L, pieces, lim);
    S.perm = std::move(p);
    return S;
}

}  // namespace sparse_plan
}  // namespace calipso
