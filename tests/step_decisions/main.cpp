// The host's Newton-step decisions (calipso.jl_amd/csrc/step_decisions.hpp) against values worked out by hand from the reference's formulas (the file:line citations
// are those of the header).  Stand-alone: only the pure header is included; tests/test_step_decisions_cpu.py builds this with the host compiler and runs it.
// The numbers are dyadic (sums of a few powers of two) wherever a product or a power is expected, so every expected value below is exact and compared bit for bit.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../calipso.jl_amd/csrc/step_decisions.hpp"

using namespace calipso;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)
static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }
static const double INF = std::numeric_limits<double>::infinity();

// ---- inertia_correction! inertia.jl:30-80 ---------------------------------------------------------------------------------------------------------------------
// what a driver does with ic_begin / ic_after: factorise (here: take the next scripted inertia), ask, repeat
struct Walk { IcVerdict verdict; int nfact; std::vector<double> ep, ed; };      // ep / ed: the regularisation each factorisation ran with
static Walk walk(const Options& o, Scalars& sc, int nx, int m, const std::vector<std::vector<int64_t>>& script) {
    Walk w{IC_AGAIN, 0, {}, {}};
    ic_begin(o, sc);
    for (size_t k = 0; k < script.size(); ++k) {
        w.ep.push_back(sc.ep); w.ed.push_back(sc.ed); w.nfact += 1;
        w.verdict = ic_after(o, sc, script[k].data(), nx, m, k == 0);
        if (w.verdict != IC_AGAIN) break;
    }
    return w;
}
static void test_inertia_walk() {
    Options o;
    o.primal_regularization_initial = 0.0009765625; o.dual_regularization_initial = 0.001953125;       // 2^-10, 2^-9
    o.min_regularization = 9.5367431640625e-07;                                                        // 2^-20
    o.scaling_regularization_last = 0.5; o.scaling_regularization = 8.0; o.scaling_regularization_initial = 100.0;
    o.dual_regularization = 0.5; o.dual_regularization_exponent = 0.25; o.max_regularization = 64.0;
    const int nx = 5, m = 3;
    const std::vector<int64_t> ok = {5, 3, 0}, bad = {4, 4, 0}, bad_zero = {-1, 3, 1};                  // (a zero pivot reports posDCount = -1)
    {   // IC-1 succeeds: one factorisation with the initial regularisation, eps_last untouched
        Scalars sc; sc.kappa = 0.0625; sc.ep_last = 0.25; sc.ep = 7.0; sc.ed = 7.0;
        const Walk w = walk(o, sc, nx, m, {ok, bad, bad});
        CHECK(w.verdict == IC_DONE && w.nfact == 1);
        CHECK(same(sc.ep, 0.0009765625) && same(sc.ed, 0.001953125) && same(sc.ep_last, 0.25));
    }
    {   // bad x 3, then ok, eps_last = 0.25 > 0: IC-3 max(2^-20, 0.5 * 0.25) = 0.125, IC-5 takes scaling_regularization: 1, 8; eps_last <- 8
        Scalars sc; sc.kappa = 0.0625; sc.ep_last = 0.25;
        const Walk w = walk(o, sc, nx, m, {bad, bad, bad, ok, bad});
        CHECK(w.verdict == IC_DONE && w.nfact == 4);
        CHECK(w.ep.size() == 4 && same(w.ep[0], 0.0009765625) && same(w.ep[1], 0.125) && same(w.ep[2], 1.0) && same(w.ep[3], 8.0));
        for (double ed : w.ed) CHECK(same(ed, 0.001953125));                                            // no zero eigenvalue reported: IC-2 does not fire
        CHECK(same(sc.ep, 8.0) && same(sc.ep_last, 8.0) && same(sc.ed, 0.001953125));
    }
    {   // the same with eps_last = 0: IC-3 (quirk B-1: always the max) gives max(2^-20, 0.5 * 0) = 2^-20, IC-5 takes scaling_regularization_initial: x100, x100
        Scalars sc; sc.kappa = 0.0625; sc.ep_last = 0.0;
        const Walk w = walk(o, sc, nx, m, {bad, bad, bad, ok});
        CHECK(w.verdict == IC_DONE && w.nfact == 4);
        CHECK(same(w.ep[1], 9.5367431640625e-07) && same(w.ep[2], 100.0 * 9.5367431640625e-07) && same(w.ep[3], 100.0 * (100.0 * 9.5367431640625e-07)));
        CHECK(same(w.ep[2], 9.5367431640625e-05) && same(w.ep[3], 0.0095367431640625));                // 100 / 2^20, 10000 / 2^20
        CHECK(same(sc.ep_last, 0.0095367431640625));                                                    // (IC-5 looked at the OLD eps_last = 0 throughout)
    }
    {   // a zero eigenvalue at IC-1: IC-2 sets ed = 0.5 * 0.0625^0.25 = 0.5 * 0.5; it stays for the later factorisations
        Scalars sc; sc.kappa = 0.0625; sc.ep_last = 0.25;
        const Walk w = walk(o, sc, nx, m, {bad_zero, bad, ok});
        CHECK(w.verdict == IC_DONE && w.nfact == 3);
        CHECK(same(w.ed[0], 0.001953125) && same(w.ed[1], 0.25) && same(w.ed[2], 0.25) && same(sc.ed, 0.25));
        CHECK(same(w.ep[1], 0.125) && same(w.ep[2], 1.0) && same(sc.ep, 1.0) && same(sc.ep_last, 1.0));      // (IC-5 after the second: 8 * 0.125)
    }
    {   // a zero eigenvalue only LATER does not touch ed (IC-2 stands before the loop)
        Scalars sc; sc.kappa = 0.0625; sc.ep_last = 0.25;
        const Walk w = walk(o, sc, nx, m, {bad, bad_zero, ok});
        CHECK(w.verdict == IC_DONE && same(sc.ed, 0.001953125));
    }
    {   // never ok: 2^-10, 0.125, 1, 8, 64 — after the 4th factorisation ep = 64 is NOT > max_regularization = 64 (again), after the 5th 512 is: failed, eps_last kept
        Scalars sc; sc.kappa = 0.0625; sc.ep_last = 0.25;
        const Walk w = walk(o, sc, nx, m, std::vector<std::vector<int64_t>>(9, bad));
        CHECK(w.verdict == IC_FAILED && w.nfact == 5);
        CHECK(w.ep.size() == 5 && same(w.ep[3], 8.0) && same(w.ep[4], 64.0) && same(sc.ep, 512.0) && same(sc.ep_last, 0.25));
    }
    CHECK(inertia_ok(ok.data(), nx, m) && !inertia_ok(bad.data(), nx, m) && !inertia_ok(bad_zero.data(), nx, m));
    { const int64_t z[3] = {5, 3, 1}; CHECK(!inertia_ok(z, nx, m)); }
}

// ---- iterative_refinement! iterative_refinement.jl:14-51 -----------------------------------------------------------------------------------------------------
// a driver's loop: norms[k] is the residual norm after k rounds; returns the verdict, *rounds the count reported
static RefineVerdict refine(const Options& o, const std::vector<double>& norms, int* rounds, int* ran) {
    int it = 0; *ran = 0;
    for (;;) {
        const RefineVerdict v = refine_next(o, norms[(size_t)*ran], norms[0], &it);
        if (v != REFINE_ROUND) { *rounds = it; return v; }
        *ran += 1; it += 1;
    }
}
static void test_refine_next() {
    Options o; o.iterative_refinement_tolerance = 0.5; o.max_iterative_refinement = 2; o.min_iterative_refinement = 0;
    int rounds = -1, ran = -1;
    CHECK(refine(o, {0.5, 9, 9, 9}, &rounds, &ran) == REFINE_DONE && rounds == 0 && ran == 0);          // tolerance met at round 0, no minimum
    o.min_iterative_refinement = 1;
    CHECK(refine(o, {0.5, 0.25, 9, 9}, &rounds, &ran) == REFINE_DONE && rounds == 1 && ran == 1);       // ... one round is the minimum
    CHECK(refine(o, {4, 3, 2, 4, 0}, &rounds, &ran) == REFINE_DONE && rounds == 3 && ran == 3);         // exhausted (iteration = 0, 1, 2 ran), 4 <= 4: ok
    CHECK(refine(o, {4, 3, 2, 4.5, 0}, &rounds, &ran) == REFINE_FAILED && rounds == 3 && ran == 3);     // exhausted, 4.5 > 4: failed
    CHECK(refine(o, {4, 3, 0.5, 0}, &rounds, &ran) == REFINE_DONE && rounds == 2 && ran == 2);          // tolerance met in the last admitted iteration
    o.min_iterative_refinement = 0;
    CHECK(refine(o, {INF, 0, 0, 0}, &rounds, &ran) == REFINE_FAILED && rounds == 3 && ran == 0);        // +inf at round 0: failed at once, max + 1 rounds reported
    o.min_iterative_refinement = 1;
    CHECK(refine(o, {INF, INF, 0, 0}, &rounds, &ran) == REFINE_FAILED && rounds == 3 && ran == 1);      // ... once the minimum number of rounds is done
    CHECK(refine(o, {4, INF, 0, 0}, &rounds, &ran) == REFINE_FAILED && rounds == 3 && ran == 1);        // +inf later (inf <= 4 is false all the same)
    CHECK(refine(o, {INF, 0.25, 0, 0}, &rounds, &ran) == REFINE_DONE && rounds == 1 && ran == 1);       // a round below the minimum may still repair it
    o.max_iterative_refinement = -1; o.min_iterative_refinement = 0;                                    // the loop body never runs: norm <= norm_initial decides
    CHECK(refine(o, {4}, &rounds, &ran) == REFINE_DONE && rounds == 0 && ran == 0);
    CHECK(refine(o, {INF}, &rounds, &ran) == REFINE_FAILED && rounds == 0 && ran == 0);                 // (the single driver's rule: a non-finite norm never passes)
}

// ---- optimality_error.jl:8-9, solve.jl:130-135 ----------------------------------------------------------------------------------------------------------------
static void test_step_norms() {
    double hs[18] = {0};
    hs[8] = 4.0; hs[9] = 3.0; hs[10] = 1.0; hs[11] = 2.0; hs[12] = 2.5; hs[13] = 1.0e6; hs[14] = 1.0e6; hs[15] = 1.0e6;
    {   // no constraints: both scalings are 1 whatever the dual sums hold
        const StepNorms n = step_norms(hs, 8, 0, 0);
        CHECK(same(n.residual_violation, 0.5) && same(n.optimality, 3.0) && same(n.slack_violation, 2.0));
    }
    hs[13] = 100.0; hs[14] = 0.0;
    {   // nc = 0, (100 + 0) / 2 = 50 < 100: sd = 100 / 100
        const StepNorms n = step_norms(hs, 8, 2, 0);
        CHECK(same(n.optimality, 3.0) && same(n.slack_violation, 2.0));
    }
    hs[13] = 300.0; hs[14] = 100.0;
    {   // (300 + 100) / 2 = 200 > 100: sd = 2, the Lagrangian gradient counts 1.5; comp / 1 = 2.5 is now the largest (nc = 0: hs[15] not looked at)
        const StepNorms n = step_norms(hs, 8, 2, 0);
        CHECK(same(n.optimality, 2.5));
    }
    hs[15] = 200.0;
    {   // ne + nc = 1 + 4: 400 / 5 = 80 < 100: sd = 1; 200 / 4 = 50 < 100: sc = 1
        const StepNorms n = step_norms(hs, 16, 1, 4);
        CHECK(same(n.residual_violation, 0.25) && same(n.optimality, 3.0));
    }
    hs[15] = 1600.0; hs[12] = 16.0;
    {   // 1600 / 4 = 400 > 100: sc = 4, comp counts 16 / 4 = 4 > 3
        const StepNorms n = step_norms(hs, 16, 1, 4);
        CHECK(same(n.optimality, 4.0));
    }
    hs[10] = 5.0; hs[11] = 6.0;
    { const StepNorms n = step_norms(hs, 16, 1, 4); CHECK(same(n.optimality, 6.0) && same(n.slack_violation, 6.0)); }
    hs[10] = 7.0;
    { const StepNorms n = step_norms(hs, 16, 1, 4); CHECK(same(n.optimality, 7.0) && same(n.slack_violation, 7.0)); }
}

// ---- solve.jl:138-143 and :165 --------------------------------------------------------------------------------------------------------------------------------
static void test_exit_kind() {
    Options o;
    o.residual_tolerance = 0.5; o.slack_tolerance = 0.5; o.equality_tolerance = 0.5; o.complementarity_tolerance = 0.5;
    o.central_path_update_tolerance = 10.0; o.optimality_tolerance = 1.0;
    const double far = 100.0;                                                                           // an optimality error no inner exit takes
    CHECK(exit_kind(o, 0.5, {0.25, far, 0.25}, 0.5, 0.5, true) == 1);                                   // (< for the two norms, <= for the two violations)
    CHECK(exit_kind(o, 0.5, {0.5, far, 0.25}, 0.5, 0.5, true) == 0);                                    // each conjunct failing alone
    CHECK(exit_kind(o, 0.5, {0.25, far, 0.5}, 0.5, 0.5, true) == 0);
    CHECK(exit_kind(o, 0.5, {0.25, far, 0.25}, 0.75, 0.5, true) == 0);
    CHECK(exit_kind(o, 0.5, {0.25, far, 0.25}, 0.5, 0.75, true) == 0);
    CHECK(exit_kind(o, 0.5, {0.25, far, 0.25}, 0.5, 0.5, false) == 0);                                  // a benchmark step never converges outwards
    CHECK(exit_kind(o, 0.5, {0.25, 0.0, 0.25}, 0.5, 0.5, false) == 2);
    CHECK(exit_kind(o, 0.5, {0.25, 0.0, 0.25}, 0.5, 0.5, true) == 1);                                   // the outer test stands first
    CHECK(same(inner_exit_threshold(o, 0.5), 5.0) && same(inner_exit_threshold(o, 0.0625), 1.0));       // max(10 * 0.5, 1), max(10 * 0.0625, 1)
    CHECK(exit_kind(o, 0.5, {9, 5.0, 9}, 0, 0, true) == 2 && exit_kind(o, 0.5, {9, 5.5, 9}, 0, 0, true) == 0);
    CHECK(exit_kind(o, 0.0625, {9, 1.0, 9}, 0, 0, true) == 2 && exit_kind(o, 0.0625, {9, 1.5, 9}, 0, 0, true) == 0);
}

// ---- solve.jl:190-221 -----------------------------------------------------------------------------------------------------------------------------------------
static void masks_with_first_clear(int* mask, int k) {      // bits 0..k-1 set (violation), bit k clear, the rest as it falls
    for (int w = 0; w < CONE_MASK_WORDS; ++w) mask[w] = 0;
    for (int b = 0; b < k; ++b) mask[b >> 5] |= (int)(1u << (b & 31));
}
static void test_cone_step_sizes() {
    Options o; o.max_cone_line_search = 40;
    int ms[CONE_MASK_WORDS], mt[CONE_MASK_WORDS];
    for (double sls : {0.5, 0.7}) {
        o.scaling_line_search = sls;
        const int firsts[5] = {0, 31, 32, 40, 7};
        for (int a = 0; a < 5; ++a) {
            const int ks = firsts[a], kt = firsts[(a + 1) % 5];
            masks_with_first_clear(ms, ks); masks_with_first_clear(mt, kt);
            double as = -1.0, at = -1.0;
            CHECK(cone_step_sizes(ms, mt, o, &as, &at));
            double es = 1.0, et = 1.0;                                                                  // cone_step_size = scaling_line_search * cone_step_size, k times
            for (int k = 0; k < ks; ++k) es = sls * es;
            for (int k = 0; k < kt; ++k) et = sls * et;
            CHECK(same(as, es) && same(at, et));
            if (sls == 0.5) CHECK(same(as, std::ldexp(1.0, -ks)) && same(at, std::ldexp(1.0, -kt)));    // 2^-k
        }
        // trials 0..40 all violated: failure, whichever of the two — and whatever stands beyond max_cone_line_search (bit 41 is clear)
        double as = -1.0, at = -1.0;
        masks_with_first_clear(ms, 41); masks_with_first_clear(mt, 3);
        CHECK(!cone_step_sizes(ms, mt, o, &as, &at) && !cone_step_sizes(mt, ms, o, &as, &at));
        CHECK(same(as, -1.0) && same(at, -1.0));
    }
    masks_with_first_clear(ms, 32);
    CHECK(ms[0] == -1 && ms[1] == 0 && first_feasible_trial(ms, 40) == 32 && first_feasible_trial(ms, 32) == 32 && first_feasible_trial(ms, 31) == -1);
    masks_with_first_clear(ms, CONE_MASK_TRIALS);                                                       // every bit of every word set
    CHECK(first_feasible_trial(ms, 831) == -1 && first_feasible_trial(ms, 5000) == -1);                 // (never past the mask words)
}

// ---- solve.jl:254-302, line_search.jl, filter.jl:81-89 ---------------------------------------------------------------------------------------------------------
static void test_line_search() {
    // merit_exponent 2, violation_exponent 1, Armijo 0.5, both progress tolerances 0.5: with M = 12, theta = 8, d = -4, step 1
    //   switching: 1 * 4^2 > 8;  Armijo: Mh - 12 - 10 mach * 12 <= 0.5 * 1 * -4, i.e. Mh <= 10 (+ 120 mach);
    //   sufficient progress: thetah - 10 mach * 8 <= 4  or  Mh - 10 mach * 12 <= 12 - 4 = 8
    // the filter holds the one pair (6, 10): it takes a candidate with thetah < 6 or Mh < 10
    struct Row { double slack_tolerance, mach, theta, M, thetah, Mh, dd, step; bool filter; bool accepts, augments; };
    const Row rows[] = {
        {10, 0,      8, 12, 7, 10,    -4,  1, true,  false, false},   // the filter rejects (7 >= 6 and 10 >= 10) what switching + Armijo (10 <= 10) would take
        {10, 0,      8, 12, 7, 10,    -4,  1, false, true,  false},   // ... an empty filter does not
        {10, 0,      8, 12, 5, 9,     -4,  1, true,  true,  false},   // switching + Armijo accept (no sufficient progress: 5 > 4, 9 > 8)
        {10, 0,      8, 12, 3, 11,    -4,  1, true,  true,  true},    // switching holds, Armijo fails (11 > 10): sufficient progress (3 <= 4) accepts; filter augmented
        {10, 0,      8, 12, 5, 11,    -4,  1, true,  false, true},    // ... and neither: back-track
        {4,  0,      8, 12, 5, 9,     -4,  1, true,  false, false},   // theta > slack_tolerance: row 3 is left to sufficient progress, which it has not
        {4,  0,      8, 12, 4, 9,     -4,  1, true,  true,  false},   // ... which it has (4 <= 4)
        {10, 0,      8, 12, 5, 9,     0.5, 1, true,  false, true},    // d >= 0: no switching
        {10, 0,      8, 12, 5, 9,     -2,  1, true,  false, true},    // 1 * 2^2 > 8 fails: no switching
        {10, 0,      8, 12, 5, 9,     -4,  0.5, true, false, true},   // step 0.5: 0.5 * 16 > 8 fails
        {10, 0.0625, 8, 12, 5, 17.5,  -4,  1, true,  true,  false},   // the machine-tolerance term: 17.5 - 12 - 0.625 * 12 = -2 <= -2
        {10, 0.0625, 8, 12, 9.5, 17.75, -4, 1, false, false, true},   // Armijo fails by 0.25; progress: 9.5 - 5 > 4 and 17.75 - 7.5 > 8
        {10, 0.0625, 8, 12, 9, 17.75, -4,  1, false, true,  true},    // ... 9 - 0.625 * 8 = 4 <= 4
    };
    const double ft[1] = {6.0}, fm[1] = {10.0};
    CHECK(filter_accepts(ft, fm, 1, 5.0, 10.0) && filter_accepts(ft, fm, 1, 6.0, 9.0) && !filter_accepts(ft, fm, 1, 6.0, 10.0) && filter_accepts(ft, fm, 0, 6.0, 10.0));
    int r = 0;
    for (const Row& w : rows) {
        Options o;
        o.merit_exponent = 2.0; o.violation_exponent = 1.0; o.armijo_tolerance = 0.5; o.violation_tolerance = 0.5; o.merit_tolerance = 0.5;
        o.slack_tolerance = w.slack_tolerance; o.machine_tolerance = w.mach;
        const bool fok = filter_accepts(ft, fm, w.filter ? 1 : 0, w.thetah, w.Mh);
        const bool acc = line_search_accepts(o, fok, w.theta, w.M, w.thetah, w.Mh, w.dd, w.step);
        const bool aug = filter_needs_augment(o, w.theta, w.M, w.Mh, w.dd, w.step);
        if (acc != w.accepts || aug != w.augments) std::printf("line-search row %d: accepts %d (expected %d), augments %d (expected %d)\n", r, acc, w.accepts, aug, w.augments);
        CHECK(acc == w.accepts && aug == w.augments);
        ++r;
    }
}

// ---- initialize.jl:38-48, solve.jl:356-365 ---------------------------------------------------------------------------------------------------------------------
static void test_scalars() {
    Options o;
    o.central_path_scaling = 0.5; o.central_path_exponent = 2.0; o.residual_tolerance = 1.25;           // kappa >= 1.25 / 10 = 0.125
    o.penalty_scaling = 10.0; o.max_penalty = 1000.0;
    Scalars sc;
    sc.kappa = 4.0; central_path_update(o, sc);        CHECK(same(sc.kappa, 2.0) && same(sc.tau, 0.99));             // min(0.5 * 4, 4^2) = 2: the scaling; 1 - 2 < 0.99
    sc.kappa = 0.375; central_path_update(o, sc);      CHECK(same(sc.kappa, 0.140625) && same(sc.tau, 0.99));        // min(0.1875, 0.375^2): the power; 0.859375 < 0.99
    sc.kappa = 0.25; central_path_update(o, sc);       CHECK(same(sc.kappa, 0.125) && same(sc.tau, 0.99));           // min(0.125, 0.0625) = 0.0625 < 0.125: clamped
    o.residual_tolerance = 0.0;
    sc.kappa = 0.0625; central_path_update(o, sc);     CHECK(same(sc.kappa, 0.00390625) && same(sc.tau, 0.99609375)); // 2^-8; tau = 1 - kappa > 0.99
    sc.rho = 2.0; sc.kappa = 0.25; penalty_update(o, sc);     CHECK(same(sc.rho, 20.0));                // max(10 * 2, 1 / 0.25 = 4)
    sc.rho = 2.0; sc.kappa = 0.03125; penalty_update(o, sc);  CHECK(same(sc.rho, 32.0));                // max(20, 32)
    o.max_penalty = 16.0;
    sc.rho = 2.0; sc.kappa = 0.25; penalty_update(o, sc);     CHECK(same(sc.rho, 16.0));                // clamped
    CHECK(same(sc.kappa, 0.25));                                                                        // (the penalty update leaves kappa alone)
    o.central_path_initial = 1.0; o.penalty_initial = 3.0;
    { Scalars s0; s0.ep = 5.0; s0.ep_last = 6.0; s0.ed = 7.0; initial_scalars(o, s0);
      CHECK(same(s0.kappa, 1.0) && same(s0.tau, 0.99) && same(s0.rho, 3.0) && same(s0.ep, 5.0) && same(s0.ep_last, 6.0) && same(s0.ed, 7.0)); }
    o.central_path_initial = 0.0078125;
    { Scalars s0; initial_scalars(o, s0); CHECK(same(s0.kappa, 0.0078125) && same(s0.tau, 0.9921875)); }
    Scalars now, saved;
    now.kappa = 1; now.tau = 2; now.rho = 3; now.ep = 4; now.ep_last = 5; now.ed = 6;
    saved.kappa = 7; saved.tau = 8; saved.rho = 9; saved.ep = 10; saved.ep_last = 11; saved.ed = 12;
    restore_scalars_keeping_regularization(now, saved);
    CHECK(now.kappa == 7 && now.tau == 8 && now.rho == 9 && now.ep == 4 && now.ep_last == 11 && now.ed == 6);
}

int main() {
    test_inertia_walk();
    test_refine_next();
    test_step_norms();
    test_exit_kind();
    test_cone_step_sizes();
    test_line_search();
    test_scalars();
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("step decisions ok\n");
    return 0;
}
