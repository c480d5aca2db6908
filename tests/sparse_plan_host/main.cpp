// The analyse phase of the sparse LDL^T on the CPU: plans one case (a text file written by tests/test_sparse_plan_cpu.py: pattern, method or perm,
// optional pieces, limits) with calipso.jl_amd/csrc/sparse_plan.hpp — the order and the dissection pieces from ordering.hpp — and checks every table by
// brute force: the column tables against a dense boolean symbolic elimination, every address table of the multifrontal plan by a round trip to global
// indices.  Prints the route the plan took, then "sparse plan ok"; a refusal is printed with its status and text.  Built by the host compiler under
// the address and undefined-behaviour sanitizers; no HIP.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <set>
#include <string>
#include <tuple>

#include "../../calipso.jl_amd/csrc/ordering.hpp"
#include "../../calipso.jl_amd/csrc/sparse_plan.hpp"

using namespace calipso::sparse_plan;
using calipso::i64;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); std::exit(1); } } while (0)

static long long tri(long long i) { return i * (i + 1) / 2; }

struct Case {
    i64 n = 0; int method = 0;
    std::vector<i64> colptr, rowval, perm;
    Pieces pieces;
    Limits lim;
};

static Case read_case(const char* path) {
    std::ifstream in(path);
    CHECK(in.good());
    Case c; std::string key;
    auto list = [&](std::vector<i64>& v) { size_t k; in >> k; v.resize(k); for (auto& x : v) in >> x; };
    while (in >> key) {
        if (key == "n") in >> c.n;
        else if (key == "method") in >> c.method;
        else if (key == "colptr") list(c.colptr);
        else if (key == "rowval") list(c.rowval);
        else if (key == "perm") list(c.perm);
        else if (key == "pieces") { std::vector<i64> v; list(v); for (size_t k = 0; k + 1 < v.size(); k += 2) c.pieces.push_back({(int)v[k], (int)v[k + 1]}); }
        else if (key == "limit") {
            std::string name; long long v; in >> name >> v;
            if (name == "max_front") c.lim.max_front = (int)v; else if (name == "max_front_wide") c.lim.max_front_wide = (int)v;
            else if (name == "max_front_global") c.lim.max_front_global = (int)v; else if (name == "big") c.lim.big = (int)v;
            else if (name == "wide_solve_m") c.lim.wide_solve_m = (int)v; else if (name == "wide_solve_nch") c.lim.wide_solve_nch = (int)v;
            else if (name == "wf_solve_rows") c.lim.wf_solve_rows = (int)v; else if (name == "max_pool") c.lim.max_pool = v;
            else if (name == "max_item_bytes") c.lim.max_item_bytes = (size_t)v; else if (name == "max_item_children") c.lim.max_item_children = (int)v;
            else if (name == "wide_fronts") c.lim.wide_fronts = (int)v; else if (name == "mf_items") c.lim.mf_items = (int)v;
            else CHECK(!"unknown limit");
        } else CHECK(!"unknown key");
    }
    CHECK(c.n >= 1 && (i64)c.colptr.size() == c.n + 1);
    return c;
}

// ---- the column tables against a dense boolean symbolic elimination of P A P' --------------------------------------------------------------------
static void check_columns(const Case& c, const SparsePlan& S) {
    const int n = (int)c.n;
    CHECK((i64)S.perm.size() == c.n);
    std::vector<int> ip((size_t)n, -1);
    for (int k = 0; k < n; ++k) { const i64 v = S.perm[(size_t)k]; CHECK(v >= 1 && v <= n && ip[(size_t)v - 1] < 0); ip[(size_t)v - 1] = k; }
    std::vector<std::vector<char>> F((size_t)n, std::vector<char>((size_t)n, 0));
    std::vector<std::pair<int, int>> at((size_t)c.rowval.size(), {-1, -1});                 // per entry of the caller's pattern: (row, column) of P A P' lower
    i64 nnzU = 0;
    for (int col = 0; col < n; ++col)
        for (i64 q = c.colptr[(size_t)col] - 1; q < c.colptr[(size_t)col + 1] - 1; ++q) {
            const int r = (int)c.rowval[(size_t)q] - 1;
            if (r > col) continue;
            const int pr = ip[(size_t)r], pc = ip[(size_t)col];
            at[(size_t)q] = {std::max(pr, pc), std::min(pr, pc)};
            F[(size_t)std::max(pr, pc)][(size_t)std::min(pr, pc)] = 1; ++nnzU;
        }
    // the lower CSC and its gather map
    const LowerCsc& A = S.A;
    CHECK(A.nnzU == nnzU && (int)A.Alp.size() == n + 1 && A.Alp[0] == 0 && (i64)A.Ali.size() == nnzU && A.Asrc.size() == A.Ali.size() && S.nnzA == (i64)c.rowval.size());
    std::vector<char> used(c.rowval.size(), 0);
    for (int j = 0; j < n; ++j) {
        CHECK(A.Alp[(size_t)j] <= A.Alp[(size_t)j + 1]);
        for (int q = A.Alp[(size_t)j]; q < A.Alp[(size_t)j + 1]; ++q) {
            CHECK(A.Ali[(size_t)q] >= j && A.Ali[(size_t)q] < n && (q == A.Alp[(size_t)j] || A.Ali[(size_t)q] > A.Ali[(size_t)q - 1]));
            const int src = A.Asrc[(size_t)q];
            CHECK(src >= 0 && src < (int)c.rowval.size() && !used[(size_t)src] && at[(size_t)src] == std::make_pair(A.Ali[(size_t)q], j));
            used[(size_t)src] = 1;
        }
    }
    CHECK(A.Alp[(size_t)n] == (int)nnzU);
    // symbolic elimination
    for (int k = 0; k < n; ++k) {
        std::vector<int> rows;
        for (int i = k + 1; i < n; ++i) if (F[(size_t)i][(size_t)k]) rows.push_back(i);
        for (size_t a = 0; a < rows.size(); ++a) for (size_t b = 0; b <= a; ++b) F[(size_t)rows[a]][(size_t)rows[b]] = 1;
    }
    const LPattern& L = S.L;
    CHECK((int)L.Lp.size() == n + 1 && L.Lp[0] == 0);
    i64 flops = 0;
    for (int k = 0; k < n; ++k) {
        std::vector<int> rows;
        for (int i = k + 1; i < n; ++i) if (F[(size_t)i][(size_t)k]) rows.push_back(i);
        CHECK(L.Lp[(size_t)k + 1] - L.Lp[(size_t)k] == (int)rows.size() && L.Lp[(size_t)k + 1] <= (int)L.Li.size());
        for (size_t a = 0; a < rows.size(); ++a) CHECK(L.Li[(size_t)L.Lp[(size_t)k] + a] == rows[a]);
        CHECK(S.parent[(size_t)k] == (rows.empty() ? -1 : rows[0]));
        for (int q = L.Lp[(size_t)k]; q < L.Lp[(size_t)k + 1]; ++q) flops += L.Lp[(size_t)k + 1] - q;
    }
    CHECK(L.nnzL == (i64)L.Li.size() && L.Lp[(size_t)n] == (int)L.nnzL);
    // the row view indexes exactly the entries of each row
    const RowView& R = S.R;
    CHECK((int)R.Rp.size() == n + 1 && R.Rp[0] == 0 && R.Rp[(size_t)n] == (int)L.nnzL && R.flops == flops);
    CHECK(R.Rk.size() == L.Li.size() && R.Rpos.size() == L.Li.size() && R.Rend.size() == L.Li.size());
    for (int j = 0; j < n; ++j) {
        int expect = 0;
        for (int k = 0; k < j; ++k) expect += F[(size_t)j][(size_t)k];
        CHECK(R.Rp[(size_t)j + 1] - R.Rp[(size_t)j] == expect);
        for (int q = R.Rp[(size_t)j]; q < R.Rp[(size_t)j + 1]; ++q) {
            const int k = R.Rk[(size_t)q], pos = R.Rpos[(size_t)q];
            CHECK(k >= 0 && k < j && (q == R.Rp[(size_t)j] || k > R.Rk[(size_t)q - 1]));
            CHECK(pos >= L.Lp[(size_t)k] && pos < L.Lp[(size_t)k + 1] && L.Li[(size_t)pos] == j && R.Rend[(size_t)q] == L.Lp[(size_t)k + 1]);
        }
    }
    // the segments partition `order`; every column's level is above all of its children's
    const ColumnLevels& C = S.cols;
    CHECK((int)C.order.size() == n);
    std::vector<int> level((size_t)n, -1);
    int at_pos = 0, lev = 0, widest = 0;
    for (const Segment& g : C.plan) {
        CHECK(g.first == at_pos && g.count >= 1 && g.first + g.count <= n && (!g.chain || g.count >= 1));
        for (int q = 0; q < g.count; ++q) {
            const int j = C.order[(size_t)(g.first + q)];
            CHECK(j >= 0 && j < n && level[(size_t)j] < 0);
            level[(size_t)j] = g.chain ? lev + q : lev;                                    // a chain walks single-column levels one after the other
        }
        widest = std::max(widest, g.chain ? 1 : g.count);
        CHECK(g.chain || g.count > 1);
        lev += g.chain ? g.count : 1;
        at_pos += g.count;
    }
    CHECK(at_pos == n && C.height == lev && C.widest == widest);
    for (int j = 0; j < n; ++j) if (S.parent[(size_t)j] >= 0) CHECK(level[(size_t)S.parent[(size_t)j]] > level[(size_t)j]);
}

// ---- the multifrontal plan -----------------------------------------------------------------------------------------------------------------------
static void check_multifrontal(const Case& c, const SparsePlan& S) {
    const MfPlan& M = *S.mf;
    const Limits& lim = c.lim;
    const int n = (int)c.n, NN = M.nnodes;
    const LowerCsc& A = S.A; const LPattern& L = S.L;
    CHECK(NN >= 1 && (int)M.first.size() == NN && (int)M.cols.size() == NN && (int)M.rows.size() == NN && (int)M.parent.size() == NN && (int)M.rowptr.size() == NN + 1);
    // the pieces cover every column exactly once
    std::vector<int> node_of((size_t)n, -1);
    for (int t = 0; t < NN; ++t) {
        CHECK(M.cols[(size_t)t] >= 1 && M.first[(size_t)t] >= 0 && M.first[(size_t)t] + M.cols[(size_t)t] <= n && M.cols[(size_t)t] <= 64);
        for (int q = 0; q < M.cols[(size_t)t]; ++q) { CHECK(node_of[(size_t)(M.first[(size_t)t] + q)] < 0); node_of[(size_t)(M.first[(size_t)t] + q)] = t; }
    }
    for (int j = 0; j < n; ++j) CHECK(node_of[(size_t)j] >= 0);
    auto rows_of = [&](int t) { return M.rowsv.data() + M.rowptr[(size_t)t]; };
    auto global = [&](int t, int l) { CHECK(l >= 0 && l < M.cols[(size_t)t] + M.rows[(size_t)t]); return l < M.cols[(size_t)t] ? M.first[(size_t)t] + l : rows_of(t)[l - M.cols[(size_t)t]]; };
    // rows of a node = the union of Li over its columns beyond its last column; the parent owns the first of them.  (Equality needs the columns of a node
    // to hang together in the elimination tree, as the pieces of every case here do; a node that merges independent subtrees hands the rows of both to
    // its parent, a superset of that union.)
    int max_front = 0;
    long long panel = 0, upd = 0, usum = 0;
    CHECK(M.rowptr[0] == 0 && (int)M.rowsv.size() == M.rowptr[(size_t)NN] && M.rel.size() == M.rowsv.size());
    for (int t = 0; t < NN; ++t) {
        const int f = M.first[(size_t)t], cc = M.cols[(size_t)t], last = f + cc - 1;
        std::set<int> u;
        for (int j = f; j <= last; ++j) for (int q = L.Lp[(size_t)j]; q < L.Lp[(size_t)j + 1]; ++q) if (L.Li[(size_t)q] > last) u.insert(L.Li[(size_t)q]);
        CHECK(M.rows[(size_t)t] == (int)u.size() && M.rowptr[(size_t)t + 1] == M.rowptr[(size_t)t] + M.rows[(size_t)t]);
        int k = 0;
        for (int v : u) CHECK(rows_of(t)[k++] == v);
        CHECK(M.parent[(size_t)t] == (u.empty() ? -1 : node_of[(size_t)*u.begin()]));
        max_front = std::max(max_front, cc + (int)u.size());
        // offsets: disjoint, in node order, ending at the totals
        CHECK(M.panel_off[(size_t)t] == panel && M.upd_off[(size_t)t] == upd && M.u_off[(size_t)t] == usum);
        panel += (long long)(cc + M.rows[(size_t)t]) * cc; upd += (long long)M.rows[(size_t)t] * M.rows[(size_t)t]; usum += M.rows[(size_t)t];
    }
    CHECK(M.max_front == max_front && M.panel_total == panel && M.upd_total == upd && M.usum == usum && upd + panel <= lim.max_pool);
    CHECK(max_front <= (M.last_resort ? (lim.wide_fronts ? lim.max_front_wide : lim.max_front_global) : lim.max_front));
    // children lists
    CHECK((int)M.childptr.size() == NN + 1 && M.childptr[0] == 0 && (int)M.children.size() == M.childptr[(size_t)NN]);
    for (int t = 0; t < NN; ++t) {
        std::vector<int> kids;
        for (int ch = 0; ch < NN; ++ch) if (M.parent[(size_t)ch] == t) kids.push_back(ch);
        CHECK(M.childptr[(size_t)t + 1] - M.childptr[(size_t)t] == (int)kids.size());
        for (size_t q = 0; q < kids.size(); ++q) CHECK(M.children[(size_t)M.childptr[(size_t)t] + q] == kids[q]);
    }
    // launch order: the levels partition it, children on lower levels than their parents
    CHECK((int)M.order.size() == NN);
    std::vector<int> pos_of((size_t)NN, -1), lev_of((size_t)NN, -1);
    int at_pos = 0, widest = 0, wide_count = 0, wide_blocks = 1;
    for (size_t g = 0; g < M.levels.size(); ++g) {
        const MfSeg& s = M.levels[g];
        CHECK(s.first == at_pos && s.count >= 1 && s.first + s.count <= NN);
        int mmax = 0, rmax = 0, chmax = 0;
        for (int q = 0; q < s.count; ++q) {
            const int t = M.order[(size_t)(s.first + q)];
            CHECK(t >= 0 && t < NN && pos_of[(size_t)t] < 0);
            pos_of[(size_t)t] = s.first + q; lev_of[(size_t)t] = (int)g;
            mmax = std::max(mmax, M.cols[(size_t)t] + M.rows[(size_t)t]); rmax = std::max(rmax, M.rows[(size_t)t]);
            chmax = std::max(chmax, M.childptr[(size_t)t + 1] - M.childptr[(size_t)t]);
        }
        CHECK(s.global == (mmax > lim.max_front) && s.threads == (mmax > lim.big ? 512 : 256) && s.lds_solve == sizeof(double) * 5 * (size_t)mmax);
        const size_t front = sizeof(double) * (size_t)(tri(mmax) + 2 * mmax), exch = sizeof(double) * 64 * (size_t)lim.py;
        if (s.global) CHECK(s.lds_factor == 0 && s.ypan == 0);
        else CHECK(s.ypan == (mmax >= 32 && front + exch <= lim.lds_budget) && s.lds_factor == front + (s.ypan ? exch : 0));
        CHECK(s.wide.on == (s.global && lim.wide_fronts));
        if (s.wide.on) {
            CHECK(s.wide.m == mmax && s.wide.r == rmax && s.wide.nch == chmax && s.wide.solve == (mmax > lim.wide_solve_m || chmax > lim.wide_solve_nch));
            wide_count = std::max(wide_count, s.count);
            if (s.wide.solve) wide_blocks = std::max(wide_blocks, (rmax + lim.wf_solve_rows - 1) / lim.wf_solve_rows);
        } else CHECK(s.wide.m == 0 && s.wide.r == 0 && s.wide.nch == 0 && s.wide.solve == 0);
        // the level's fronts in the pool: disjoint, inside it
        if (s.global) {
            std::vector<std::pair<long long, long long>> iv;
            for (int q = 0; q < s.count; ++q) { const int t = M.order[(size_t)(s.first + q)]; iv.push_back({M.foff[(size_t)t], M.foff[(size_t)t] + tri(M.cols[(size_t)t] + M.rows[(size_t)t])}); }
            std::sort(iv.begin(), iv.end());
            for (size_t q = 0; q < iv.size(); ++q) CHECK(iv[q].first >= 0 && iv[q].second <= M.pool_total && (q == 0 || iv[q].first >= iv[q - 1].second));
        }
        widest = std::max(widest, s.count);
        at_pos += s.count;
    }
    CHECK(at_pos == NN && M.widest == widest && M.wide_count == wide_count && M.wide_blocks == wide_blocks && (int)M.foff.size() == NN && (int)M.wbase.size() == NN);
    for (int t = 0; t < NN; ++t) if (M.parent[(size_t)t] >= 0) CHECK(lev_of[(size_t)M.parent[(size_t)t]] > lev_of[(size_t)t] && pos_of[(size_t)M.parent[(size_t)t]] > pos_of[(size_t)t]);
    // rel: the child's rows inside the parent's front
    for (int t = 0; t < NN; ++t) {
        const int par = M.parent[(size_t)t];
        const int* rel = M.rel.data() + M.rowptr[(size_t)t];
        for (int k = 0; k < M.rows[(size_t)t]; ++k) {
            CHECK(par >= 0 && global(par, rel[k]) == rows_of(t)[k] && (k == 0 || rel[k] > rel[k - 1]));
        }
    }
    // Aloc: every entry of A inside its node's packed front
    CHECK(M.Aloc.size() == A.Ali.size());
    for (int j = 0; j < n; ++j) {
        const int t = node_of[(size_t)j];
        for (int q = A.Alp[(size_t)j]; q < A.Alp[(size_t)j + 1]; ++q) {
            int lr = 0;
            while (tri(lr + 1) <= M.Aloc[(size_t)q]) ++lr;
            const int lc = M.Aloc[(size_t)q] - (int)tri(lr);
            CHECK(M.Aloc[(size_t)q] >= 0 && lc == j - M.first[(size_t)t] && lc <= lr && global(t, lr) == A.Ali[(size_t)q]);
        }
    }
    // node and child records, field by field
    CHECK((int)M.nrec.size() == NN && (int)M.crec.size() == (int)M.children.size());
    bool any_items = false;
    int xat = 0;
    for (int pos = 0; pos < NN; ++pos) {
        const MfNode& nd = M.nrec[(size_t)pos];
        const int t = M.order[(size_t)pos];
        const MfSeg& s = M.levels[(size_t)lev_of[(size_t)t]];
        CHECK(nd.s == t && nd.f == M.first[(size_t)t] && nd.c == M.cols[(size_t)t] && nd.r == M.rows[(size_t)t] && nd.rowptr == M.rowptr[(size_t)t]);
        CHECK(nd.nch == M.childptr[(size_t)t + 1] - M.childptr[(size_t)t] && nd.chfirst >= 0 && nd.chfirst + nd.nch <= (int)M.crec.size());
        CHECK(nd.alp0 == A.Alp[(size_t)nd.f] && nd.alp1 == A.Alp[(size_t)(nd.f + nd.c)] && nd.pad0 == M.wbase[(size_t)t] && nd.pad2 == s.ypan);
        CHECK(nd.pad1 == (M.parent[(size_t)t] >= 0 ? pos_of[(size_t)M.parent[(size_t)t]] : -1));
        CHECK(nd.panel_off == M.panel_off[(size_t)t] && nd.upd_off == M.upd_off[(size_t)t] && nd.u_off == M.u_off[(size_t)t] && nd.foff == M.foff[(size_t)t]);
        CHECK((nd.pad0 >= 0) == (s.wide.on != 0));
        for (int q = 0; q < nd.nch; ++q) {
            const MfChild& cr = M.crec[(size_t)(nd.chfirst + q)];
            const int ch = M.children[(size_t)M.childptr[(size_t)t] + (size_t)q];
            CHECK(cr.rc == M.rows[(size_t)ch] && cr.rowptr == M.rowptr[(size_t)ch] && cr.upd_off == M.upd_off[(size_t)ch] && cr.u_off == M.u_off[(size_t)ch] && cr.pos == pos_of[(size_t)ch] && cr.pad == 0);
        }
        // extend-add items: children ascending, a child's lower triangle row by row; source inside the child's slot, target = the pair of parent rows rel gives
        if (nd.xa0 < 0) { CHECK(nd.xa0 == -1 && nd.xa1 == -1); continue; }
        CHECK(!s.global && lim.mf_items && nd.xa0 == xat && nd.xa1 >= nd.xa0 && nd.xa1 <= (int)M.xit.size());
        any_items = true;
        long long expect = 0;
        for (int q = 0; q < nd.nch; ++q) expect += tri(M.rows[(size_t)M.children[(size_t)M.childptr[(size_t)t] + (size_t)q]]);
        CHECK(nd.xa1 - nd.xa0 == expect);
        std::tuple<int, int, int> before{-1, -1, -1};
        for (int e = nd.xa0; e < nd.xa1; ++e) {
            const MfXItem& it = M.xit[(size_t)e];
            const int ord = (int)(it.tq >> 16), place = (int)(it.tq & 0xffffu);
            CHECK(ord < nd.nch);
            const int ch = M.children[(size_t)M.childptr[(size_t)t] + (size_t)ord], rch = M.rows[(size_t)ch];
            const long long off = (long long)it.usrc - M.upd_off[(size_t)ch];
            CHECK(off >= 0 && off < (long long)rch * rch && (long long)it.usrc < M.upd_total);
            const int a = (int)(off / rch), b = (int)(off % rch);
            CHECK(b <= a);
            int lr = 0;
            while (tri(lr + 1) <= place) ++lr;
            const int* rel = M.rel.data() + M.rowptr[(size_t)ch];
            CHECK(lr == rel[a] && place - (int)tri(lr) == rel[b] && lr < nd.c + nd.r && global(t, lr) == rows_of(ch)[a] && global(t, rel[b]) == rows_of(ch)[b]);
            CHECK(std::make_tuple(ord, a, b) > before);
            before = std::make_tuple(ord, a, b);
        }
        xat = nd.xa1;
    }
    if (any_items) CHECK((int)M.xit.size() == std::max(xat, 1));                            // (an empty table is one dummy item: the upload is never empty)
    else CHECK(M.xit.empty() || (lim.mf_items && M.xit.size() == 1));
    // wide rows: per row of a front factored by many workgroups exactly its entries of A and the child rows that land in it, children ascending
    if (!M.wide_count) CHECK(M.wptrE.empty() && M.wptrC.empty() && M.wEcol.empty() && M.wEsrc.empty() && M.wC.empty());
    CHECK(M.wptrE.size() == M.wptrC.size() && M.wEcol.size() == M.wEsrc.size());
    size_t seenE = 0, seenC = 0, seen_rows = 0;
    for (int pos = 0; pos < NN; ++pos) {                     // (the row tables were filled in launch order)
        const int t = M.order[(size_t)pos], base = M.wbase[(size_t)t];
        if (base < 0) continue;
        const int f = M.first[(size_t)t], cc = M.cols[(size_t)t], mm = cc + M.rows[(size_t)t];
        CHECK((size_t)base == seen_rows && (size_t)base + (size_t)mm + 1 <= M.wptrE.size());
        seen_rows += (size_t)mm + 1;
        for (int i = 0; i < mm; ++i) {
            const int e0 = M.wptrE[(size_t)(base + i)], e1 = M.wptrE[(size_t)(base + i + 1)], c0 = M.wptrC[(size_t)(base + i)], c1 = M.wptrC[(size_t)(base + i + 1)];
            CHECK((size_t)e0 == seenE && e1 >= e0 && (size_t)e1 <= M.wEcol.size() && (size_t)c0 == seenC && c1 >= c0 && (size_t)c1 <= M.wC.size());
            std::set<std::pair<int, int>> want, got;
            for (int j = f; j < f + cc; ++j) for (int e = A.Alp[(size_t)j]; e < A.Alp[(size_t)j + 1]; ++e) if (A.Ali[(size_t)e] == global(t, i)) want.insert({j - f, A.Asrc[(size_t)e]});
            for (int e = e0; e < e1; ++e) got.insert({M.wEcol[(size_t)e], M.wEsrc[(size_t)e]});
            CHECK(want == got && (int)got.size() == e1 - e0);
            int at = c0;
            for (int q = M.childptr[(size_t)t]; q < M.childptr[(size_t)t + 1]; ++q) {
                const int ch = M.children[(size_t)q], rch = M.rows[(size_t)ch];
                for (int k = 0; k < rch; ++k) {
                    if (global(t, M.rel[(size_t)M.rowptr[(size_t)ch] + (size_t)k]) != global(t, i)) continue;
                    CHECK(at < c1);
                    const MfRowItem& it = M.wC[(size_t)at++];
                    CHECK(it.uoff == M.upd_off[(size_t)ch] + (long long)k * rch && it.relptr == M.rowptr[(size_t)ch] && it.a == k && it.uo == (int)(M.u_off[(size_t)ch] + k) && it.pad == 0);
                    CHECK(it.uoff + k < M.upd_total);
                }
            }
            CHECK(at == c1);
            seenE = (size_t)e1; seenC = (size_t)c1;
        }
    }
    CHECK(seen_rows == M.wptrE.size() && seenE == M.wEcol.size() && seenC == M.wC.size());
}

int main(int argc, char** argv) {
    CHECK(argc == 2);
    const Case c = read_case(argv[1]);
    const i64 n = c.n;
    std::vector<i64> p((size_t)n);
    Pieces pieces = c.pieces;
    namespace ord = calipso::ordering;
    if (c.method == 3) p = c.perm;
    else if (c.method == 0) std::iota(p.begin(), p.end(), (i64)1);
    else {
        CHECK(ord::csc_pattern_ok(n, c.colptr.data(), c.rowval.data()));
        const auto adj = ord::adjacency(n, c.colptr.data(), c.rowval.data());
        p = c.method == 1 ? ord::rcm(adj) : c.method == 2 ? ord::minimum_degree(adj) : ord::nested_dissection(adj, c.method == 4 ? &pieces : nullptr);
    }
    const SparsePlan S = analyse(n, c.colptr.data(), c.rowval.data(), p, pieces, c.lim);
    if (S.status) {
        CHECK(!S.mf && S.perm.empty() && S.A.Ali.empty() && S.L.Li.empty());
        std::printf("refused %d %s\n", S.status, S.message.c_str());
        return 0;
    }
    check_columns(c, S);
    if (S.mf) {
        check_multifrontal(c, S);
        const MfPlan& M = *S.mf;
        int lds = 0, glob = 0, wide = 0, by_m = 0, by_nch = 0, items = 0;
        for (const MfSeg& g : M.levels) {
            lds += !g.global; glob += g.global; wide += g.wide.on;
            by_m += g.wide.on && g.wide.m > c.lim.wide_solve_m; by_nch += g.wide.on && g.wide.nch > c.lim.wide_solve_nch;
        }
        for (const MfNode& nd : M.nrec) items += nd.xa0 >= 0;
        std::printf("route multifrontal width=%d last_resort=%d max_front=%d nodes=%d lds_levels=%d global_levels=%d wide_levels=%d solve_by_m=%d solve_by_nch=%d wide_blocks=%d item_nodes=%d items=%zu pool=%lld\n",
                    M.width, (int)M.last_resort, M.max_front, M.nnodes, lds, glob, wide, by_m, by_nch, M.wide_blocks, items, M.xit.size(), M.pool_total);
    } else std::printf("route columns levels=%d widest=%d launches=%zu\n", S.cols.height, S.cols.widest, S.cols.plan.size());
    std::printf("sparse plan ok\n");
    return 0;
}
