// The host pieces of solve! on the sparse handle (calipso.jl_amd/csrc/sparse_solve.hpp) on the CPU: only that header and step_decisions.hpp, the plain host
// compiler, the address and undefined-behaviour sanitizers.  tests/test_sparse_solve_host_cpu.py builds and runs it.
//   main filter <capacity> <file>    replays the file's operations (a theta merit: augment, c theta merit: check, r: reset) through sparse_solve::Filter and prints
//                                    every check's verdict and, at the end, the kept pairs
//   main layout                      sweeps (nx, ne, nc, small cones, wide cones) and checks the item space and the workspace layout: no two partials share an
//                                    address, every address lies inside the workspace, sections begin at multiples of 64, the grid respects its cap
//   main checks                      prints what the argument checks say about a fixed list of calls
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../calipso.jl_amd/csrc/sparse_solve.hpp"
#include "../../calipso.jl_amd/csrc/step_decisions.hpp"

using namespace calipso::sparse_solve;
using calipso::i64;

static int run_filter(i64 capacity, const char* path) {
    Filter f(capacity);
    std::ifstream in(path);
    if (!in) { std::printf("cannot read %s\n", path); return 2; }
    std::string op;
    while (in >> op) {
        if (op == "r") { f.reset(); continue; }
        double th = 0.0, m = 0.0;
        in >> th >> m;
        if (op == "a") f.augment(th, m);
        else if (op == "c") std::printf("check %d\n", f.accepts(th, m) ? 1 : 0);
        else { std::printf("unknown operation %s\n", op.c_str()); return 2; }
    }
    std::printf("index %lld capacity %lld\n", (long long)f.index, (long long)f.capacity());
    for (i64 i = 0; i < f.index; ++i) std::printf("pair %.17g %.17g\n", f.theta[(size_t)i], f.merit[(size_t)i]);
    for (i64 i = f.index; i < f.capacity(); ++i)
        if (f.theta[(size_t)i] != 1.0e8 || f.merit[(size_t)i] != 1.0e8) { std::printf("slot %lld beyond the index is not empty\n", (long long)i); return 1; }
    return 0;
}

static bool check_layout(i64 nx, i64 ne, i64 nc, i64 n_small, i64 n_wide) {
    const Layout l = layout(nx, ne, nc, n_small, n_wide);
    const auto bad = [&](const char* what) { std::printf("layout(%lld, %lld, %lld, %lld, %lld): %s\n", (long long)nx, (long long)ne, (long long)nc, (long long)n_small, (long long)n_wide, what); return false; };
    if (l.rows != nx + ne + nc || l.small0 < l.rows || l.small0 % WAVE || l.wide0 < l.small0 + n_small || l.wide0 % WAVE || l.items != l.wide0 + WAVE * n_wide || l.items % WAVE)
        return bad("the item sections");
    if (l.grid < 1 || l.grid > GRID_CAP) return bad("the grid");
    if ((i64)l.grid * THREADS < l.items && l.grid != GRID_CAP) return bad("a grid below its cap that does not cover the items");
    std::vector<char> used((size_t)l.doubles, 0);
    const auto take = [&](i64 a) { if (a < 0 || a >= l.doubles || used[(size_t)a]) return false; used[(size_t)a] = 1; return true; };
    for (int b = 0; b < l.grid; ++b) {
        for (int q = 0; q < PP_COUNT; ++q) if (!take(l.prologue(q, b))) return bad("a prologue partial");
        for (int q = 0; q < CP_COUNT; ++q) if (!take(l.candidate(q, b))) return bad("a candidate partial");
        for (int q = 0; q < AP_COUNT; ++q) if (!take(l.accept(q, b))) return bad("an accept partial");
    }
    for (char u : used) if (!u) return bad("a hole in the workspace");
    std::vector<char> words((size_t)l.mask_ints, 0);
    for (int b = 0; b < l.grid; ++b)
        for (int m = 0; m < PUB_MASK_INTS; ++m) {
            const i64 a = l.mask(m, b);
            if (a < 0 || a >= l.mask_ints || words[(size_t)a]) return bad("a mask word");
            words[(size_t)a] = 1;
        }
    return true;
}

static int run_layout() {
    const i64 sizes[] = {0, 1, 255, 256, 257, (i64)GRID_CAP * THREADS + 1000};      // the last: above the grid cap
    const i64 cones[] = {0, 1, 255, 256, 257, 3000};                                // 3000 wavefront cones: above the cap too
    long long cases = 0, capped = 0;
    for (i64 nx : sizes) for (i64 ne : sizes) for (i64 nc : sizes) for (i64 n_soc : cones)
        for (int split = 0; split < 3; ++split) {
            const i64 n_small = split == 0 ? n_soc : (split == 1 ? 0 : n_soc / 2), n_wide = n_soc - n_small;
            if (!check_layout(nx, ne, nc, n_small, n_wide)) return 1;
            cases += 1;
            if (layout(nx, ne, nc, n_small, n_wide).grid == GRID_CAP) capped += 1;
        }
    static_assert(PUB_BYTES <= sizeof(double) * PUB_ALLOC_DOUBLES && PUB_CONE_SEARCH_FAILED < PUB_DOUBLES && PUB_MASK_INTS == 2 * calipso::CONE_MASK_WORDS, "the published block");
    std::printf("layout ok cases=%lld capped=%lld\n", cases, capped);
    return 0;
}

static int run_checks() {
    double x = 0.0;
    const auto show = [](const std::string& t) { std::printf("%s\n", t.empty() ? "ok" : t.c_str()); };
    show(check_named_vector("get", "solution", &x, 56, 12, 4, 12, false));
    show(check_named_vector("get", "solution", &x, 55, 12, 4, 12, false));
    show(check_named_vector("get", "no_such_vector", &x, 1, 12, 4, 12, false));
    show(check_named_vector("get", "dual", nullptr, 4, 12, 4, 12, false));
    show(check_named_vector("get", "dual", nullptr, 0, 12, 0, 12, false));
    show(check_named_vector("set", "residual", &x, 56, 12, 4, 12, true));
    show(check_named_vector("set", "dual", &x, 4, 12, 4, 12, true));
    show(check_keep_trace(0));
    show(check_keep_trace(1));
    show(check_keep_trace(TRACE_ROWS_MAX + 1));
    show(check_trace(nullptr, 3));
    show(check_trace(nullptr, 0));
    show(check_step_sizes("candidate", 0.5, 1.0));
    show(check_step_sizes("candidate", 0.0, 1.0));
    show(check_step_sizes("candidate", 0.5, 2.0));
    for (int v = 0; v < V_COUNT; ++v) std::printf("%s %lld\n", vector_name(v), (long long)vector_length(v, 12, 4, 12));
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "filter" && argc == 4) return run_filter(std::atoll(argv[2]), argv[3]);
    if (mode == "layout") return run_layout();
    if (mode == "checks") return run_checks();
    std::printf("usage: main filter <capacity> <file> | layout | checks\n");
    return 2;
}
