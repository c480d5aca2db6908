// The workspace layout of a p-column pass (calipso.jl_amd/csrc/column_layout.hpp) over small dimension tuples, forward / transposed x rounds on / off x with and
// without grad_theta columns: every region has the size its kernels index, lies inside the total, overlaps no other region but for the two stated aliases, and the
// total is what the solver reserved before there was a layout function (the formulas below are written out from those allocations, not taken from the header).
// Stand-alone: only the pure header is included; tests/test_column_layout_cpu.py builds this with the host compiler and runs it.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../calipso.jl_amd/csrc/column_layout.hpp"

using namespace calipso;

static int failures = 0;
static long cases = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; if (failures < 20) std::printf("FAILED %s:%d: %s  [%s]\n", __FILE__, __LINE__, #cond, where); } } while (0)

struct Named { const char* name; ColumnRegion r; size_t want; };

static bool overlap(const ColumnRegion& a, const ColumnRegion& b) { return a.len && b.len && a.off < b.off + b.len && b.off < a.off + a.len; }
static bool pair_is(const Named& a, const Named& b, const char* x, const char* y) {
    return (!std::strcmp(a.name, x) && !std::strcmp(b.name, y)) || (!std::strcmp(a.name, y) && !std::strcmp(b.name, x));
}

static void check_one(size_t nx, size_t ne, size_t nc, size_t np, size_t NP, size_t p, bool transposed, bool rounds, bool with_theta, size_t nparts) {
    char where[160];
    std::snprintf(where, sizeof where, "nx %zu ne %zu nc %zu np %zu NP %zu p %zu transposed %d rounds %d theta %d nparts %zu", nx, ne, nc, np, NP, p, (int)transposed, (int)rounds,
                  (int)with_theta, nparts);
    const size_t m = ne + nc, n = nx + m, N = nx + 2 * ne + 3 * nc;      // the condensed system, a Point (point.jl:13-22)
    const size_t extra = with_theta ? np * p : 0;
    const ColumnLayout L = column_layout(n, N, NP, m, p, transposed, rounds, nparts, extra);
    ++cases;
    // what each region must hold (0: the pass does not have it)
    const size_t Np = N * p;
    const std::vector<Named> regions = {
        {"rsym", L.rsym, transposed ? 0 : n * p}, {"dsym", L.dsym, transposed ? 0 : n * p}, {"xbuf", L.xbuf, NP * p}, {"u", L.u, NP * p}, {"z", L.z, NP * p},
        {"t1", L.t1, m * p}, {"t2", L.t2, m * p}, {"X", L.X, (transposed || rounds) ? Np : 0}, {"V", L.V, transposed ? Np : 0},
        {"E", L.E, rounds ? Np : 0}, {"C", L.C, rounds ? Np : 0}, {"Xsave", L.Xsave, rounds ? Np : 0}, {"part", L.part, rounds ? nparts * p : 0},
        {"norms", L.norms, rounds ? p : 0}, {"hx", L.hx, rounds ? NP * p : 0}, {"zx", L.zx, rounds ? m * p : 0}, {"grad_theta", L.grad_theta, transposed ? extra : 0}};
    for (const Named& a : regions) {
        CHECK(a.r.len == a.want);
        CHECK(a.r.off + a.r.len <= L.total);
    }
    // The solves keep every region but hx and zx live at once (a correction solve reads E and writes C while X, Xsave, V and grad_theta's place wait); the rounds'
    // residual writes hx and zx while X, V, E, C, Xsave, part and norms are live.  So: no two regions overlap, except the two aliases onto workspace that is free
    // between two solves
    for (size_t i = 0; i < regions.size(); ++i)
        for (size_t j = i + 1; j < regions.size(); ++j) {
            const Named &a = regions[i], &b = regions[j];
            if (pair_is(a, b, "hx", "u") || pair_is(a, b, "zx", "t2")) continue;      // the ONLY permitted aliases
            if (overlap(a.r, b.r)) { ++failures; std::printf("FAILED: %s overlaps %s  [%s]\n", a.name, b.name, where); }
        }
    // the totals reserved before the layout function existed
    size_t want;
    if (!transposed) {
        want = (n + 3 * NP + 2 * m) * p + n * p;                          // the pipeline buffer + the dsym scratch, once two allocations
        if (rounds) want += 4 * Np + (nparts + 1) * p;                    // X, E, C, Xsave, partial norms, column norms
    } else {
        want = (3 * NP + 2 * m) * p + 2 * Np + extra;                     // the transposed pipeline, V, lambda, grad_theta
        if (rounds) want += 3 * Np + (nparts + 1) * p;                    // E, C, Xsave, partial norms, column norms
    }
    CHECK(L.total == want);
    // the rounds only append: a pass without them finds its regions where a pass with them left them (the buffer is kept between calls)
    if (rounds) {
        const ColumnLayout U = column_layout(n, N, NP, m, p, transposed, false, nparts, extra);
        CHECK(U.xbuf.off == L.xbuf.off && U.u.off == L.u.off && U.z.off == L.z.off && U.t1.off == L.t1.off && U.t2.off == L.t2.off);
        CHECK(U.rsym.off == L.rsym.off && U.dsym.off == L.dsym.off && U.V.off == L.V.off && U.grad_theta.off == L.grad_theta.off);
        CHECK(U.total <= L.total);
    }
}

int main() {
    const size_t nxs[] = {1, 3, 128, 130}, nes[] = {0, 2, 5}, ncs[] = {0, 1, 4}, ps[] = {1, 2, 7}, nps[] = {1, 3};
    for (size_t nx : nxs) for (size_t ne : nes) for (size_t nc : ncs) for (size_t p : ps) for (size_t np : nps) {
        const size_t NP = (nx + 127) / 128 * 128;                         // nx padded to the Schur tile: NP > nx but for nx = 128
        const size_t nparts = (ne + nc + 255) / 256;                      // 0 without constraints
        for (int t = 0; t < 2; ++t) for (int r = 0; r < 2; ++r) for (int g = 0; g < 2; ++g) {
            check_one(nx, ne, nc, np, NP, p, t != 0, r != 0, g != 0, nparts);
            check_one(nx, ne, nc, np, NP, p, t != 0, r != 0, g != 0, nparts + 2);      // more than one partial norm per column
        }
    }
    if (failures) { std::printf("%d failures in %ld cases\n", failures, cases); return 1; }
    std::printf("column layout ok (%ld cases)\n", cases);
    return 0;
}
