// column_layout.hpp — where everything lives in the workspace of a p-column pass through the current factors (columns.hip): differentiate!, its correction rounds and
// its reverse mode.  The ONE copy of it: columns.hip sizes its reserve with `total` and takes every pointer from the same regions, so the two cannot disagree.  Plain
// C++ like step_decisions.hpp and sensitivity_columns.hpp (integers in, offsets out; no HIP, no handle): tests/column_layout runs it on the CPU.
#pragma once
#include <cstddef>

namespace calipso {

struct ColumnRegion { size_t off = 0, len = 0; };      // in doubles from the start of the workspace; len = 0: the pass does not have it
struct ColumnLayout {
    ColumnRegion rsym, dsym;      // n  x p  forward only: the condensed right-hand sides, the condensed steps k_recover leaves behind
    ColumnRegion xbuf;            // NP x p  the zero-padded x-block: b_x -> dx (transposed: [V_x; 0] -> xb)
    ColumnRegion u, z;            // NP x p  the substitution scratches of S^-1
    ColumnRegion t1, t2;          // m  x p  the seed of the condensed middle, Omega b_m (transposed: g), and what it leaves, [gx; hx] dx
    ColumnRegion V;               // N  x p  transposed only: the cotangents (forward: the handle's jacobian_parameters)
    ColumnRegion X;               // N  x p  the iterate: lambda (forward: only with the rounds — an unrefined pass writes solution_sensitivity directly)
    ColumnRegion grad_theta;      // `extra` transposed only: np x p
    ColumnRegion E, C, Xsave;     // N  x p  the rounds: residual, correction, the iterate a forced round may go back to
    ColumnRegion part, norms;     // nparts x p partial norms, p column norms
    // the products of the rounds' residual, Lxx X_x + [gx; hx]' X_yz (NP x p) and [gx; hx] X_x (m x p).  ALIASES: they land on the substitution scratch u and on the
    // second m x p block t2, which are free between two solves (the middle writes both before it reads them)
    ColumnRegion hx, zx;
    size_t total = 0;
};

inline ColumnLayout column_layout(size_t n, size_t N, size_t NP, size_t m, size_t p, bool transposed, bool with_rounds, size_t nparts, size_t extra) {
    ColumnLayout L;
    auto take = [&L](ColumnRegion& r, size_t len) { r.off = L.total; r.len = len; L.total += len; };
    if (!transposed) take(L.rsym, n * p);
    take(L.xbuf, NP * p); take(L.u, NP * p); take(L.z, NP * p); take(L.t1, m * p); take(L.t2, m * p);
    if (!transposed) take(L.dsym, n * p);
    if (transposed) { take(L.V, N * p); take(L.X, N * p); take(L.grad_theta, extra); }
    if (with_rounds) {      // (appended: a pass without them finds everything else where a pass with them left it)
        if (!transposed) take(L.X, N * p);
        take(L.E, N * p); take(L.C, N * p); take(L.Xsave, N * p); take(L.part, nparts * p); take(L.norms, p);
        L.hx = L.u; L.zx = L.t2;
    }
    return L;
}

}  // namespace calipso
