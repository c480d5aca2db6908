// sparse_krylov.hpp — the host half of the `H \ residual` fallback of the sparse handle (search_direction.jl:22 for calipso_hip_sparse_kkt_*): restarted
// right-preconditioned GMRES on the unreduced H with the condensed solve as preconditioner.  Here: the options and their checks, the workspace layout, the
// Hessenberg least-squares problem of one cycle (Givens rotations, the residual estimate, the back-substitution for y), and the verdicts between cycles.
// Plain host C++, no HIP: sparse_kkt.hip drives the kernels of sparse_krylov.hip through it, tests/sparse_krylov_host/main.cpp runs it on the CPU.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

namespace calipso {
namespace sparse_krylov {

typedef int64_t i64;

constexpr int RESTART_MAX = 32;            // the dots kernel keeps one accumulator per basis vector in registers: a compile-time bound
constexpr int CYCLES_MAX = 16;
constexpr int THREADS = 256;               // (= KT of sparse_kkt_handle.hpp)
constexpr int GRID_CAP = 256;              // workgroups of a vector kernel; rows beyond THREADS * GRID_CAP are taken in stride order
// what comes back per iteration, in ONE read-back: the summed coefficients of both Gram-Schmidt passes, |w|_2, and the cycle's |r0|_2
constexpr int COEF_NORM = RESTART_MAX, COEF_BETA = RESTART_MAX + 1, COEF_DOUBLES = RESTART_MAX + 2;

struct KrylovOptions {
    int fallback = 0;                      // krylov_fallback: search_direction goes on to GMRES where iterative refinement fails
    int restart = 16;                      // krylov_restart: 1 .. RESTART_MAX
    int max_cycles = 4;                    // krylov_max_cycles: 1 .. CYCLES_MAX
};

// 1 taken, 0 not one of these options, -1 refused (*why says why)
inline int set_option(KrylovOptions& o, const char* name, double value, std::string* why) {
    const auto integer_in = [&](double lo, double hi) {
        if (value == value && value >= lo && value <= hi && value == std::floor(value)) return true;
        if (why) *why = std::string(name) + ": an integer in " + std::to_string((int)lo) + " .. " + std::to_string((int)hi) + ", not " + std::to_string(value);
        return false;
    };
    if (!std::strcmp(name, "krylov_fallback")) { if (!integer_in(0, 1)) return -1; o.fallback = (int)value; return 1; }
    if (!std::strcmp(name, "krylov_restart")) { if (!integer_in(1, RESTART_MAX)) return -1; o.restart = (int)value; return 1; }
    if (!std::strcmp(name, "krylov_max_cycles")) { if (!integer_in(1, CYCLES_MAX)) return -1; o.max_cycles = (int)value; return 1; }
    return 0;
}

// the workspace, in doubles: V (restart + 1 vectors of N), Z = M V (restart vectors), the partials of the dots (one per (vector, workgroup)) and of |w|^2 (one
// per workgroup), the coefficient block
struct Layout {
    i64 N = 0, restart = 0, grid = 1;
    i64 off_V = 0, off_Z = 0, off_dots = 0, off_norm = 0, off_coef = 0, doubles = 0;
    i64 vector_doubles() const { return (2 * restart + 1) * N; }
};
inline i64 grid_of(i64 N) { const i64 g = (N + THREADS - 1) / THREADS; return g < 1 ? 1 : (g > GRID_CAP ? GRID_CAP : g); }
inline Layout layout(i64 N, i64 restart) {
    Layout l;
    l.N = N; l.restart = restart; l.grid = grid_of(N);
    l.off_V = 0;
    l.off_Z = l.off_V + (restart + 1) * N;
    l.off_dots = l.off_Z + restart * N;
    l.off_norm = l.off_dots + (i64)RESTART_MAX * l.grid;
    l.off_coef = l.off_norm + l.grid;
    l.doubles = l.off_coef + COEF_DOUBLES;
    return l;
}

enum ColumnVerdict {
    COLUMN_CONTINUE = 0,                   // another iteration of this cycle
    COLUMN_CONVERGED,                      // the estimate is at or below the tolerance: the cycle ends
    COLUMN_FULL,                           // j = restart: the cycle ends
    COLUMN_BREAKDOWN,                      // |w| = 0 exactly: the Krylov space is exhausted, the cycle ends (the estimate is then 0 too)
    COLUMN_NONFINITE                       // a coefficient or a norm is not finite, or the projected problem is singular: the fallback ends, nothing is taken
};

// one cycle's least-squares problem  min | beta e1 - Hbar y |  kept as the triangular factor of Hbar under Givens rotations
struct Cycle {
    int restart = 0, j = 0;                // j columns pushed
    double R[RESTART_MAX][RESTART_MAX];    // R[row][column], upper triangular
    double cs[RESTART_MAX], sn[RESTART_MAX], g[RESTART_MAX + 1];

    void begin(int restart_, double beta) { restart = restart_; j = 0; g[0] = beta; }
    // |g_j|: the 2-norm of the residual of the best x in the space so far, which bounds its infinity norm
    double estimate() const { return std::fabs(g[j]); }
    // column j of the Hessenberg matrix: h[0 .. j] (the Gram-Schmidt coefficients) and hnext = |w|_2
    ColumnVerdict push(const double* h, double hnext, double tolerance) {
        if (j >= restart || j >= RESTART_MAX) return COLUMN_FULL;
        if (!std::isfinite(hnext) || !std::isfinite(g[j])) return COLUMN_NONFINITE;
        for (int i = 0; i <= j; ++i) if (!std::isfinite(h[i])) return COLUMN_NONFINITE;
        double col[RESTART_MAX + 1];
        for (int i = 0; i <= j; ++i) col[i] = h[i];
        for (int i = 0; i < j; ++i) {      // the rotations so far
            const double a = col[i], b = col[i + 1];
            col[i] = cs[i] * a + sn[i] * b;
            col[i + 1] = -sn[i] * a + cs[i] * b;
        }
        const double r = std::hypot(col[j], hnext);
        if (!(r > 0.0) || !std::isfinite(r)) return COLUMN_NONFINITE;      // a zero column: H Z is singular on this space
        cs[j] = col[j] / r; sn[j] = hnext / r;
        col[j] = r;
        for (int i = 0; i <= j; ++i) R[i][j] = col[i];
        g[j + 1] = -sn[j] * g[j];
        g[j] = cs[j] * g[j];
        ++j;
        if (hnext == 0.0) return COLUMN_BREAKDOWN;
        if (estimate() <= tolerance) return COLUMN_CONVERGED;
        return j >= restart ? COLUMN_FULL : COLUMN_CONTINUE;
    }
    // y (j entries) by back-substitution; false where a pivot is zero or y is not finite
    bool solve(double* y) const {
        for (int i = j - 1; i >= 0; --i) {
            double a = g[i];
            for (int k = i + 1; k < j; ++k) a -= R[i][k] * y[k];
            if (R[i][i] == 0.0) return false;
            y[i] = a / R[i][i];
            if (!std::isfinite(y[i])) return false;
        }
        return true;
    }
};

enum CycleVerdict {
    CYCLE_CONVERGED = 0,                   // the TRUE |R - H step|_inf is at or below the tolerance
    CYCLE_RESTART,                         // restart from that residual
    CYCLE_UNCONVERGED,                     // no cycles remain: the step is left in place, reported as unconverged
    CYCLE_NONFINITE                        // the true norm is not finite: nothing is taken
};
inline CycleVerdict after_cycle(double true_norm_inf, double tolerance, int cycles_done, int max_cycles) {
    if (!std::isfinite(true_norm_inf)) return CYCLE_NONFINITE;
    if (true_norm_inf <= tolerance) return CYCLE_CONVERGED;
    if (cycles_done >= max_cycles) return CYCLE_UNCONVERGED;
    return CYCLE_RESTART;
}

// what calipso_hip_sparse_kkt_fallback_info reports
enum { FI_TAKEN = 0, FI_ITERATIONS, FI_CYCLES, FI_NORM, FI_CONVERGED, FI_DEVICE_MS, FI_LAUNCHES, FI_SOLVE_FALLBACKS, FI_SOLVE_ITERATIONS, FI_SOLVE_MOST_ITERATIONS,
       FI_SOLVE_UNCONVERGED, FI_WORKSPACE_BYTES, FI_COUNT };

struct FallbackReport {
    double v[FI_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool step_taken = false;               // the GMRES step replaced the refined one (finite throughout)
    void begin_call() { for (int i = FI_TAKEN; i <= FI_LAUNCHES; ++i) v[i] = 0.0; step_taken = false; }
    void begin_solve() { for (int i = FI_SOLVE_FALLBACKS; i <= FI_SOLVE_UNCONVERGED; ++i) v[i] = 0.0; }
    void count_in_solve() {
        v[FI_SOLVE_FALLBACKS] += 1.0; v[FI_SOLVE_ITERATIONS] += v[FI_ITERATIONS];
        if (v[FI_ITERATIONS] > v[FI_SOLVE_MOST_ITERATIONS]) v[FI_SOLVE_MOST_ITERATIONS] = v[FI_ITERATIONS];
        if (v[FI_CONVERGED] == 0.0) v[FI_SOLVE_UNCONVERGED] += 1.0;
    }
};

}  // namespace sparse_krylov
}  // namespace calipso
