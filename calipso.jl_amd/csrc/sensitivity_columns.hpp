// sensitivity_columns.hpp — the bookkeeping of differentiate! with "opt.differentiate_refinement": which parameter columns still take correction rounds, how many
// each has taken, and when the whole loop ends.  The ONE copy of it (columns.hip: refine_columns calls it, for differentiate! and for its reverse mode); plain C++ like step_decisions.hpp (no HIP, no
// handle, no device): tests/sensitivity_columns runs it on the CPU.  Every column is the loop of iterative_refinement.jl:14-44 on its own: its own round count and
// first norm, the verdict of step_decisions.hpp: refine_next on the norms the device reports.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "step_decisions.hpp"

namespace calipso {

struct SensitivityColumns {
    std::vector<int> active;       // != 0: the column takes the next correction round (the device's mask: k_accumulate_masked); a column that has stopped stays 0.
                                   // 2: the round is one that only min_iterative_refinement asks for — the column already meets the tolerance —, so its iterate is saved first
    std::vector<int> restore;      // 1: the forced round just taken raised the column's norm: the saved iterate goes back (k_restore_masked) and the column stops
    std::vector<int> failed;       // 1: it stopped without meeting the stopping test (refine_next: REFINE_FAILED); differentiate! has no fallback: it keeps its last iterate
    std::vector<int> it;           // rounds it has taken (a hopeless column reports the reference's count: refine_next)
    std::vector<double> norm0;     // ||E(:, j)||_inf of the unrefined column
    std::vector<double> norm;      // the last norm it was judged on
    int n_active = 0, n_restore = 0;
    bool first = true;             // the next norms are those of the unrefined columns

    void begin(int p) {
        const size_t n = (size_t)std::max(0, p);
        active.assign(n, 1); restore.assign(n, 0); failed.assign(n, 0); it.assign(n, 0); norm0.assign(n, 0.0); norm.assign(n, 0.0);
        n_active = (int)n; n_restore = 0; first = true;
    }
    int columns() const { return (int)active.size(); }
    // norms[j] = ||R_theta(:, j) - H X(:, j)||_inf for the current X (NaN reported as +inf): of the unrefined columns on the first call, afterwards behind a round that
    // the active columns took.  The norms of stopped columns are not looked at (nothing touches those columns any more).  Returns how many columns take another round.
    // A column within the tolerance whose round only min_iterative_refinement asks for has nothing to gain but rounding noise: such a round is kept only if it does not
    // raise the column's norm.  If it does, the column goes back to the iterate it had (restore), keeps that norm and stops — a further round would start from the same
    // iterate and end the same way.  The option therefore never leaves a column that met the stopping test with a larger residual than the unrefined solve had.
    int judge(const Options& o, const double* norms) {
        n_active = 0; n_restore = 0;
        for (size_t j = 0; j < active.size(); ++j) {
            restore[j] = 0;
            if (!active[j]) continue;
            if (first) norm0[j] = norms[j];
            else {
                it[j] += 1;
                if (active[j] == 2 && !(norms[j] <= norm[j])) { restore[j] = 1; n_restore += 1; active[j] = 0; continue; }
            }
            norm[j] = norms[j];
            const RefineVerdict v = refine_next(o, norm[j], norm0[j], &it[j]);
            if (v == REFINE_ROUND) { n_active += 1; active[j] = norm[j] <= o.iterative_refinement_tolerance ? 2 : 1; continue; }
            active[j] = 0;
            if (v == REFINE_FAILED) failed[j] = 1;
        }
        first = false;
        return n_active;
    }
    bool finished() const { return n_active == 0; }      // the loop ends exactly when no column is active
    // the report of calipso_hip_differentiate_info: [columns, rounds (largest over the columns), columns that did not meet the stopping test, largest final norm]
    void report(double out[4]) const {
        int rounds = 0, nfail = 0;
        double worst = 0.0;
        for (size_t j = 0; j < active.size(); ++j) {
            rounds = std::max(rounds, it[j]); nfail += failed[j];
            worst = (norm[j] != norm[j]) ? HUGE_VAL : std::max(worst, norm[j]);
        }
        out[0] = (double)active.size(); out[1] = (double)rounds; out[2] = (double)nfail; out[3] = worst;
    }
};

}  // namespace calipso
