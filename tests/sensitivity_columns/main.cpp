// The column bookkeeping of differentiate!'s correction rounds (calipso.jl_amd/csrc/sensitivity_columns.hpp) against cases worked out by hand from the loop of
// iterative_refinement.jl:14-51, which every column runs on its own (step_decisions.hpp: refine_next).  Stand-alone: only the two pure headers are included;
// tests/test_sensitivity_columns_cpu.py builds this with the host compiler and runs it.  The driver below is the loop of columns.hip: refine_columns without the
// device: judge the norms of the unrefined columns, then one judge() behind every round, until no column is active.
#include <cstdio>
#include <limits>
#include <vector>

#include "../../calipso.jl_amd/csrc/sensitivity_columns.hpp"
#include "../../calipso.jl_amd/csrc/step_decisions.hpp"

using namespace calipso;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)
static const double INF = std::numeric_limits<double>::infinity();
static const double NaN = std::numeric_limits<double>::quiet_NaN();

static Options options(i64 min_rounds, i64 max_rounds, double tol) {
    Options o;
    o.min_iterative_refinement = min_rounds; o.max_iterative_refinement = max_rounds; o.iterative_refinement_tolerance = tol;
    return o;
}
// script[k]: the norms the device reports at the k-th read-back (k = 0: the unrefined columns).  Returns the rounds run; masks[k] = the active mask after read-back k
static int drive(SensitivityColumns& c, const Options& o, int p, const std::vector<std::vector<double>>& script, std::vector<std::vector<int>>* masks = nullptr) {
    c.begin(p);
    int rounds = 0;
    for (size_t k = 0; k < script.size(); ++k) {
        std::vector<int> before = c.active;
        const int n = c.judge(o, script[k].data());
        if (masks) masks->push_back(c.active);
        int count = 0;
        for (size_t j = 0; j < c.active.size(); ++j) {
            count += c.active[j] != 0;
            CHECK(!(c.active[j] && !before[j]));          // a stopped column is never marked active again
        }
        CHECK(n == count && c.n_active == count);
        CHECK(c.finished() == (count == 0));              // the loop ends exactly when no column is active
        if (c.finished()) { CHECK(k + 1 == script.size()); return rounds; }      // ... and not before the script says so
        rounds += 1;
    }
    CHECK(c.finished());      // the script ran out before the loop ended
    return rounds;
}

// three columns that stop after 0, 1 and 3 rounds (min = 0, max = 10, tolerance 0.5)
static void test_columns_stop_one_by_one() {
    const Options o = options(0, 10, 0.5);
    SensitivityColumns c;
    std::vector<std::vector<int>> masks;
    // the norms a stopped column goes on reporting must not matter: 99 (far above the tolerance), 0, NaN
    const int rounds = drive(c, o, 3, {{0.25, 4.0, 8.0}, {99.0, 0.25, 2.0}, {0.0, NaN, 1.0}, {INF, 0.0, 0.5}}, &masks);
    CHECK(rounds == 3);
    CHECK(masks.size() == 4);
    CHECK((masks[0] == std::vector<int>{0, 1, 1}) && (masks[1] == std::vector<int>{0, 0, 1}) && (masks[2] == std::vector<int>{0, 0, 1}) && (masks[3] == std::vector<int>{0, 0, 0}));
    CHECK(c.it[0] == 0 && c.it[1] == 1 && c.it[2] == 3);
    CHECK(c.failed[0] == 0 && c.failed[1] == 0 && c.failed[2] == 0);
    CHECK(c.norm0[0] == 0.25 && c.norm0[1] == 4.0 && c.norm0[2] == 8.0);
    CHECK(c.norm[0] == 0.25 && c.norm[1] == 0.25 && c.norm[2] == 0.5);       // the norm each column was last judged on
    double out[4];
    c.report(out);
    CHECK(out[0] == 3.0 && out[1] == 3.0 && out[2] == 0.0 && out[3] == 0.5);
}

// min_iterative_refinement holds a column that already meets the tolerance for its first round (iterative_refinement.jl:14-16: `iteration >= min`)
static void test_minimum_rounds() {
    const Options o = options(1, 10, 0.5);
    SensitivityColumns c;
    CHECK(drive(c, o, 2, {{0.0, 0.125}, {0.0, 0.125}}) == 1);
    CHECK(c.it[0] == 1 && c.it[1] == 1 && c.failed[0] == 0 && c.failed[1] == 0);
}

// ... and such a forced round (mask value 2: the iterate is saved first) is kept only if it does not raise the column's norm.  Column 0: 0.25 -> 0.375, still within
// the tolerance but worse: it goes back to the iterate it had, keeps the norm 0.25, has taken its round, is not failed.  Column 1: 0.25 -> 0.125, kept.  Column 2:
// 0.125 -> 0.125, kept.  Column 3 is outside the tolerance (mask value 1, nothing saved): 4 -> 8 is kept as the reference keeps it, and the column goes on
static void test_forced_round_that_makes_it_worse() {
    const Options o = options(1, 10, 0.5);
    SensitivityColumns c;
    std::vector<std::vector<int>> masks;
    CHECK(drive(c, o, 4, {{0.25, 0.25, 0.125, 4.0}, {0.375, 0.125, 0.125, 8.0}, {0.0, 0.0, 0.0, 0.5}}, &masks) == 2);
    CHECK((masks[0] == std::vector<int>{2, 2, 2, 1}) && (masks[1] == std::vector<int>{0, 0, 0, 1}));
    CHECK(c.it[0] == 1 && c.it[1] == 1 && c.it[2] == 1 && c.it[3] == 2);
    CHECK(c.norm[0] == 0.25 && c.norm[1] == 0.125 && c.norm[2] == 0.125 && c.norm[3] == 0.5);
    CHECK(c.failed[0] == 0 && c.failed[1] == 0 && c.failed[2] == 0 && c.failed[3] == 0);
    // the restore mask is that of the LAST judge only: column 0 was flagged behind round 1, nothing behind round 2
    CHECK(c.n_restore == 0 && c.restore[0] == 0);
    c.begin(2);
    const double first[2] = {0.25, 0.25}, second[2] = {std::numeric_limits<double>::quiet_NaN(), 0.25};
    CHECK(c.judge(o, first) == 2 && c.n_restore == 0);
    CHECK(c.judge(o, second) == 0 && c.n_restore == 1 && c.restore[0] == 1 && c.restore[1] == 0);      // a NaN is worse than anything
    CHECK(c.norm[0] == 0.25 && c.failed[0] == 0 && c.finished());
}

// a column whose norm is NaN from the start (the device reports +inf, vectors.hip: rabs; a NaN that reached the host counts the same): it takes the minimum number of
// rounds (2), stops there, is counted as failed and reports the reference's round count max + 1 = 6 (step_decisions.hpp: refine_next, the documented deviation).
// Its neighbour never meets the tolerance: it = 0..5 run a round, at it = 6 the loop is exhausted with norm <= norm0: done, not failed
static void test_nan_column() {
    for (const double bad : {INF, NaN}) {
        const Options o = options(2, 5, 0.5);
        SensitivityColumns c;
        std::vector<std::vector<int>> masks;
        const int rounds = drive(c, o, 2, {{bad, 1.0}, {bad, 1.0}, {bad, 1.0}, {7.0, 1.0}, {7.0, 1.0}, {7.0, 1.0}, {7.0, 1.0}}, &masks);
        CHECK(rounds == 6);
        CHECK((masks[0] == std::vector<int>{1, 1}) && (masks[1] == std::vector<int>{1, 1}) && (masks[2] == std::vector<int>{0, 1}));
        CHECK(c.it[0] == 6 && c.failed[0] == 1);
        CHECK(c.it[1] == 6 && c.failed[1] == 0);
        double out[4];
        c.report(out);
        CHECK(out[0] == 2.0 && out[1] == 6.0 && out[2] == 1.0 && out[3] == INF);      // (a NaN norm reports +inf)
    }
}

// max_iterative_refinement exhausted (max = 1, tolerance 0: the test is never met): the reference's loop runs it = 0, 1 — two rounds — and then fails exactly when the
// final norm exceeds the first (iterative_refinement.jl:45-51)
static void test_exhausted() {
    const Options o = options(0, 1, 0.0);
    SensitivityColumns c;
    CHECK(drive(c, o, 3, {{4.0, 4.0, 4.0}, {8.0, 2.0, 9.0}, {16.0, 1.0, 4.0}}) == 2);
    CHECK(c.it[0] == 2 && c.it[1] == 2 && c.it[2] == 2);
    CHECK(c.failed[0] == 1 && c.failed[1] == 0 && c.failed[2] == 0);                   // 16 > 4: failed; 1 <= 4 and 4 <= 4: done
    double out[4];
    c.report(out);
    CHECK(out[0] == 3.0 && out[1] == 2.0 && out[2] == 1.0 && out[3] == 16.0);
}

static void test_one_and_no_column() {
    const Options o = options(1, 10, 0.5);
    {
        SensitivityColumns c;
        CHECK(drive(c, o, 1, {{3.0}, {0.75}, {0.5}}) == 2);
        CHECK(c.columns() == 1 && c.it[0] == 2 && c.failed[0] == 0 && c.norm0[0] == 3.0 && c.norm[0] == 0.5);
        // the same object again: begin() forgets the last call
        CHECK(drive(c, o, 1, {{0.25}, {0.25}}) == 1);
        CHECK(c.it[0] == 1 && c.norm0[0] == 0.25);
    }
    {
        SensitivityColumns c;
        c.begin(0);
        CHECK(c.columns() == 0 && c.finished());          // no column: the loop has ended before it began
        CHECK(c.judge(o, nullptr) == 0 && c.finished());
        double out[4] = {1, 1, 1, 1};
        c.report(out);
        CHECK(out[0] == 0.0 && out[1] == 0.0 && out[2] == 0.0 && out[3] == 0.0);
    }
}

int main() {
    test_columns_stop_one_by_one();
    test_minimum_rounds();
    test_forced_round_that_makes_it_worse();
    test_nan_column();
    test_exhausted();
    test_one_and_no_column();
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("sensitivity columns ok\n");
    return 0;
}
