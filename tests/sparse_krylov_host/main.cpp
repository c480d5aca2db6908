// The host half of the sparse handle's `H \ residual` fallback (calipso.jl_amd/csrc/sparse_krylov.hpp) on the CPU: this program includes only that header, is built
// with the plain host compiler under the address and undefined-behaviour sanitizers and run by tests/test_sparse_krylov_host_cpu.py.  It drives the header's Cycle
// exactly as sparse_kkt.hip does — right-preconditioned GMRES, classical Gram-Schmidt applied twice, V and Z kept — with dense host arithmetic in the kernels' place.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "../../calipso.jl_amd/csrc/sparse_krylov.hpp"

using namespace calipso::sparse_krylov;
typedef std::vector<double> Vec;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

static const double EPS = std::numeric_limits<double>::epsilon();

struct Dense {
    int n;
    Vec a;                                                  // row-major
    double& at(int i, int j) { return a[(size_t)i * n + j]; }
    double at(int i, int j) const { return a[(size_t)i * n + j]; }
    Vec mul(const Vec& x) const { Vec y(n, 0.0); for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) y[i] += at(i, j) * x[j]; return y; }
    double frobenius() const { double s = 0.0; for (double v : a) s += v * v; return std::sqrt(s); }
};
static double norm2(const Vec& v) { double s = 0.0; for (double x : v) s += x * x; return std::sqrt(s); }
static double norm_inf(const Vec& v) { double s = 0.0; for (double x : v) s = std::fmax(s, std::fabs(x)); return s; }

// a diagonally dominant, non-symmetric test matrix and the solution it is asked for: known without any other solver
static Dense matrix(int n) {
    Dense A{n, Vec((size_t)n * n)};
    for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) A.at(i, j) = i == j ? 4.0 + 0.25 * i : (0.5 + 0.125 * ((3 * i + 5 * j) % 7)) / (1.0 + std::abs(i - j)) * (j > i ? -1.0 : 1.0);
    return A;
}
static Vec solution(int n) { Vec x(n); for (int i = 0; i < n; ++i) x[i] = (i % 2 ? -1.0 : 1.0) * (1.0 + 0.5 * i); return x; }
// A^-1 by Gauss-Jordan with partial pivoting
static Dense inverse(Dense A) {
    const int n = A.n;
    Dense I{n, Vec((size_t)n * n, 0.0)};
    for (int i = 0; i < n; ++i) I.at(i, i) = 1.0;
    for (int c = 0; c < n; ++c) {
        int p = c;
        for (int r = c + 1; r < n; ++r) if (std::fabs(A.at(r, c)) > std::fabs(A.at(p, c))) p = r;
        for (int j = 0; j < n; ++j) { std::swap(A.at(c, j), A.at(p, j)); std::swap(I.at(c, j), I.at(p, j)); }
        const double d = A.at(c, c);
        for (int j = 0; j < n; ++j) { A.at(c, j) /= d; I.at(c, j) /= d; }
        for (int r = 0; r < n; ++r) if (r != c) { const double f = A.at(r, c); for (int j = 0; j < n; ++j) { A.at(r, j) -= f * A.at(c, j); I.at(r, j) -= f * I.at(c, j); } }
    }
    return I;
}

struct Outcome { int iterations = 0, cycles = 0; bool converged = false, finite = true; double true_norm = 0.0, worst_estimate_gap = 0.0; Vec x; };

// what gmres() of sparse_kkt.hip does, on dense host data; also measures, at every column, |estimate - |b - A x_j|_2| against the rounding of forming that residual
static Outcome gmres(const Dense& A, const Dense& M, const Vec& b, int restart, int max_cycles, double tolerance) {
    const int n = A.n;
    Outcome out;
    out.x.assign(n, 0.0);
    Vec r0 = b;
    for (;;) {
        std::vector<Vec> V, Z;
        const double beta = norm2(r0);
        Cycle cycle;
        cycle.begin(restart, beta);
        ColumnVerdict verdict = beta == 0.0 ? COLUMN_BREAKDOWN : COLUMN_CONTINUE;
        if (beta > 0.0) { Vec v0(n); for (int i = 0; i < n; ++i) v0[i] = r0[i] / beta; V.push_back(v0); }
        for (int j = 0; verdict == COLUMN_CONTINUE; ++j) {
            Z.push_back(M.mul(V[j]));
            Vec w = A.mul(Z[j]);
            double h[RESTART_MAX + 1];
            for (int q = 0; q <= j; ++q) h[q] = 0.0;
            for (int pass = 0; pass < 2; ++pass) {
                double c[RESTART_MAX + 1];
                for (int q = 0; q <= j; ++q) { c[q] = 0.0; for (int i = 0; i < n; ++i) c[q] += V[q][i] * w[i]; }
                for (int q = 0; q <= j; ++q) { for (int i = 0; i < n; ++i) w[i] -= V[q][i] * c[q]; h[q] += c[q]; }
            }
            const double hnext = norm2(w);
            Vec next(n);
            for (int i = 0; i < n; ++i) next[i] = hnext > 0.0 ? w[i] / hnext : 0.0;
            V.push_back(next);
            verdict = cycle.push(h, hnext, tolerance);
            out.iterations += 1;
            if (verdict == COLUMN_NONFINITE) break;
            // the estimate against the true residual of the x this column would give
            double y[RESTART_MAX];
            CHECK(cycle.solve(y));
            Vec x = out.x;
            for (int q = 0; q < cycle.j; ++q) for (int i = 0; i < n; ++i) x[i] += Z[q][i] * y[q];
            Vec Ax = A.mul(x), r(n);
            for (int i = 0; i < n; ++i) r[i] = b[i] - Ax[i];
            const double rounding = 64.0 * EPS * (norm2(b) + A.frobenius() * norm2(x));
            out.worst_estimate_gap = std::fmax(out.worst_estimate_gap, std::fabs(cycle.estimate() - norm2(r)) / rounding);
        }
        double y[RESTART_MAX];
        if (verdict == COLUMN_NONFINITE || !cycle.solve(y)) { out.finite = false; return out; }
        for (int q = 0; q < cycle.j; ++q) for (int i = 0; i < n; ++i) out.x[i] += Z[q][i] * y[q];
        out.cycles += 1;
        Vec Ax = A.mul(out.x);
        for (int i = 0; i < n; ++i) r0[i] = b[i] - Ax[i];
        out.true_norm = norm_inf(r0);
        const CycleVerdict next = after_cycle(out.true_norm, tolerance, out.cycles, max_cycles);
        if (next == CYCLE_NONFINITE) { out.finite = false; return out; }
        if (next == CYCLE_CONVERGED) { out.converged = true; return out; }
        if (next == CYCLE_UNCONVERGED) return out;
    }
}

static double error_of(const Vec& x, const Vec& want) { double e = 0.0; for (size_t i = 0; i < x.size(); ++i) e = std::fmax(e, std::fabs(x[i] - want[i])); return e / norm_inf(want); }

static int run_gmres() {
    const double tolerance = 1e-10;
    for (int n : {1, 2, 5, 12, 30}) {
        const Dense A = matrix(n), Ainv = inverse(A);
        const Vec want = solution(n), b = A.mul(want);
        // an exact preconditioner: A M = I, one iteration
        Outcome e = gmres(A, Ainv, b, 16, 4, tolerance);
        CHECK(e.finite && e.converged && e.iterations == 1 && e.cycles == 1 && e.true_norm <= tolerance && error_of(e.x, want) <= 1e-12 && e.worst_estimate_gap <= 1.0);
        // a perturbed one: M = A^-1 (I + E), |E| about 0.3 — no longer the inverse, as the condensed solve with its symmetrised cone blocks
        Dense M = Ainv;
        Dense E{n, Vec((size_t)n * n)};
        for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) E.at(i, j) = (i == j ? 1.0 : 0.0) + 0.3 * std::sin(1.0 + 3.0 * i + 7.0 * j) / std::sqrt((double)n);
        for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) { double s = 0.0; for (int k = 0; k < n; ++k) s += Ainv.at(i, k) * E.at(k, j); M.at(i, j) = s; }
        Outcome p = gmres(A, M, b, 16, 4, tolerance);
        CHECK(p.finite && p.converged && p.true_norm <= tolerance && error_of(p.x, want) <= 1e-9 && p.worst_estimate_gap <= 1.0);
        CHECK(p.iterations <= std::min(n, 16) * p.cycles && (n == 1 || p.iterations > 1));
        // restarts: two columns a cycle
        Outcome r = gmres(A, M, b, 2, 16, tolerance);
        CHECK(r.finite && r.converged && r.true_norm <= tolerance && error_of(r.x, want) <= 1e-9 && r.worst_estimate_gap <= 1.0 && r.iterations <= 2 * r.cycles);
        if (n >= 5) CHECK(r.cycles >= 2);
        // the caps: one cycle of two columns does not get there on the larger systems, and says so with a finite step
        Outcome c = gmres(A, M, b, 2, 1, tolerance);
        CHECK(c.finite && c.cycles == 1 && c.iterations <= 2);
        if (n >= 5) CHECK(!c.converged && c.true_norm > tolerance && std::isfinite(norm_inf(c.x)));
        std::printf("n %d exact %d/%d perturbed %d/%d restart2 %d/%d capped %d gap %.3f %.3f %.3f ok\n", n, e.iterations, e.cycles, p.iterations, p.cycles, r.iterations, r.cycles,
                    c.converged ? 1 : 0, e.worst_estimate_gap, p.worst_estimate_gap, r.worst_estimate_gap);
    }
    std::printf("gmres ok\n");
    return 0;
}

static int run_edges() {
    // an exact breakdown: A = M = I, b = 2 e1 — w - V h is zero exactly; the cycle ends with the exact answer
    {
        Dense I{3, Vec(9, 0.0)};
        for (int i = 0; i < 3; ++i) I.at(i, i) = 1.0;
        Outcome o = gmres(I, I, Vec{2.0, 0.0, 0.0}, 16, 4, 0.0);
        CHECK(o.finite && o.converged && o.iterations == 1 && o.cycles == 1 && o.x[0] == 2.0 && o.x[1] == 0.0 && o.true_norm == 0.0);
        Cycle c; c.begin(4, 2.0);
        const double h[1] = {1.0};
        CHECK(c.push(h, 0.0, 0.0) == COLUMN_BREAKDOWN && c.j == 1 && c.estimate() == 0.0);
        // a zero right-hand side: nothing to do, converged without a column
        Outcome z = gmres(I, I, Vec{0.0, 0.0, 0.0}, 16, 4, 1e-10);
        CHECK(z.finite && z.converged && z.iterations == 0 && z.cycles == 1 && norm_inf(z.x) == 0.0);
    }
    // the column cap: `restart` columns fill a cycle, a further one is refused unchanged
    {
        Cycle c; c.begin(2, 1.0);
        const double h0[1] = {0.5}, h1[2] = {0.25, 0.5};
        CHECK(c.push(h0, 0.5, 1e-30) == COLUMN_CONTINUE && c.j == 1);
        CHECK(c.push(h1, 0.5, 1e-30) == COLUMN_FULL && c.j == 2);
        const double before = c.estimate();
        const double h2[3] = {1.0, 1.0, 1.0};
        CHECK(c.push(h2, 1.0, 1e-30) == COLUMN_FULL && c.j == 2 && c.estimate() == before);
        double y[RESTART_MAX];
        CHECK(c.solve(y) && std::isfinite(y[0]) && std::isfinite(y[1]));
        Cycle full; full.begin(RESTART_MAX, 1.0);
        double h[RESTART_MAX + 1];
        for (int j = 0; j < RESTART_MAX; ++j) { for (int i = 0; i <= j; ++i) h[i] = i == j ? 1.0 : 0.125; CHECK(full.push(h, 0.5, 0.0) == (j + 1 < RESTART_MAX ? COLUMN_CONTINUE : COLUMN_FULL)); }
        CHECK(full.j == RESTART_MAX && full.push(h, 0.5, 0.0) == COLUMN_FULL && full.solve(y));
        // convergence ends a cycle early; a smaller estimate every column
        Cycle e; e.begin(8, 1.0);
        const double g0[1] = {1.0};
        CHECK(e.push(g0, 1e-3, 1e-2) == COLUMN_CONVERGED && e.estimate() <= 1e-2 && e.estimate() > 0.0);
    }
    // what is not finite ends the fallback, and so does a projected problem that is singular
    {
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        const double good[2] = {1.0, 0.5}, bad_nan[2] = {1.0, nan}, bad_inf[1] = {inf}, zero[1] = {0.0};
        Cycle c; c.begin(4, 1.0);
        CHECK(c.push(bad_inf, 1.0, 1e-10) == COLUMN_NONFINITE && c.j == 0);
        CHECK(c.push(good, nan, 1e-10) == COLUMN_NONFINITE && c.push(good, inf, 1e-10) == COLUMN_NONFINITE && c.j == 0);
        CHECK(c.push(zero, 0.0, 1e-10) == COLUMN_NONFINITE && c.j == 0);
        CHECK(c.push(good, 0.5, 1e-10) == COLUMN_CONTINUE && c.push(bad_nan, 0.5, 1e-10) == COLUMN_NONFINITE && c.j == 1);
        Cycle b; b.begin(4, nan);
        CHECK(b.push(good, 0.5, 1e-10) == COLUMN_NONFINITE);
        CHECK(after_cycle(nan, 1e-10, 1, 4) == CYCLE_NONFINITE && after_cycle(inf, 1e-10, 1, 4) == CYCLE_NONFINITE);
    }
    // between cycles
    CHECK(after_cycle(1e-10, 1e-10, 1, 4) == CYCLE_CONVERGED && after_cycle(0.0, 0.0, 4, 4) == CYCLE_CONVERGED);
    CHECK(after_cycle(2e-10, 1e-10, 1, 4) == CYCLE_RESTART && after_cycle(2e-10, 1e-10, 3, 4) == CYCLE_RESTART);
    CHECK(after_cycle(2e-10, 1e-10, 4, 4) == CYCLE_UNCONVERGED && after_cycle(2e-10, 1e-10, 1, 1) == CYCLE_UNCONVERGED);
    // the report's counters
    {
        FallbackReport r;
        r.begin_solve();
        r.v[FI_ITERATIONS] = 7; r.v[FI_CONVERGED] = 1; r.count_in_solve();
        r.begin_call();
        r.v[FI_ITERATIONS] = 3; r.v[FI_CONVERGED] = 0; r.count_in_solve();
        CHECK(r.v[FI_SOLVE_FALLBACKS] == 2 && r.v[FI_SOLVE_ITERATIONS] == 10 && r.v[FI_SOLVE_MOST_ITERATIONS] == 7 && r.v[FI_SOLVE_UNCONVERGED] == 1);
        r.begin_call();
        CHECK(r.v[FI_TAKEN] == 0 && r.v[FI_ITERATIONS] == 0 && !r.step_taken && r.v[FI_SOLVE_FALLBACKS] == 2);
        r.begin_solve();
        CHECK(r.v[FI_SOLVE_FALLBACKS] == 0 && r.v[FI_SOLVE_MOST_ITERATIONS] == 0);
    }
    std::printf("edges ok\n");
    return 0;
}

static int run_layout() {
    int cases = 0;
    for (i64 N : {1, 21, 255, 256, 257, 1314, 65536, 65537, 106480, 3000000})
        for (i64 restart = 1; restart <= RESTART_MAX; ++restart) {
            const Layout l = layout(N, restart);
            CHECK(l.grid >= 1 && l.grid <= GRID_CAP && (l.grid * THREADS >= N || l.grid == GRID_CAP) && (l.grid - 1) * THREADS < N);
            // V, Z, the dots' partials, the norm's partials, the coefficients: in this order, end to start, nothing beyond `doubles`
            const i64 begin[5] = {l.off_V, l.off_Z, l.off_dots, l.off_norm, l.off_coef};
            const i64 size[5] = {(restart + 1) * N, restart * N, (i64)RESTART_MAX * l.grid, l.grid, COEF_DOUBLES};
            CHECK(begin[0] == 0);
            for (int k = 0; k < 5; ++k) CHECK(begin[k] + size[k] == (k < 4 ? begin[k + 1] : l.doubles));
            CHECK(l.vector_doubles() == (2 * restart + 1) * N && l.off_dots == l.vector_doubles());
            // what the kernels index: vector `restart` of V, vector restart - 1 of Z, partial (RESTART_MAX - 1, grid - 1), the coefficient slots
            CHECK(l.off_V + restart * N + N <= l.off_Z && l.off_Z + (restart - 1) * N + N <= l.off_dots && l.off_dots + (RESTART_MAX - 1) * l.grid + l.grid <= l.off_norm);
            CHECK(COEF_NORM >= RESTART_MAX && COEF_BETA > COEF_NORM && COEF_BETA < COEF_DOUBLES);
            ++cases;
        }
    std::printf("layout ok cases=%d\n", cases);
    return 0;
}

static int run_options() {
    KrylovOptions o;
    std::printf("defaults %d %d %d\n", o.fallback, o.restart, o.max_cycles);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    struct Try { const char* name; double value; };
    const Try tries[] = {{"krylov_fallback", 1}, {"krylov_fallback", 0}, {"krylov_fallback", 2}, {"krylov_fallback", -1}, {"krylov_fallback", 0.5}, {"krylov_fallback", nan},
                         {"krylov_restart", 1}, {"krylov_restart", 32}, {"krylov_restart", 0}, {"krylov_restart", 33}, {"krylov_restart", 2.5},
                         {"krylov_max_cycles", 1}, {"krylov_max_cycles", 16}, {"krylov_max_cycles", 0}, {"krylov_max_cycles", 17}, {"krylov_max_cycles", nan},
                         {"krylov_tolerance", 1}, {"iterative_refinement_tolerance", 1e-8}};
    for (const Try& t : tries) {
        std::string why;
        const int rc = set_option(o, t.name, t.value, &why);
        std::printf("%s %g -> %d [%d %d %d]%s%s\n", t.name, t.value, rc, o.fallback, o.restart, o.max_cycles, why.empty() ? "" : " ", why.c_str());
    }
    CHECK(set_option(o, "krylov_restart", 0.0, nullptr) == -1 && o.restart == 32);      // (a refusal without a text wanted)
    return 0;
}

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "gmres") return run_gmres();
    if (what == "edges") return run_edges();
    if (what == "layout") return run_layout();
    if (what == "options") return run_options();
    std::printf("usage: %s gmres | edges | layout | options\n", argv[0]);
    return 2;
}
