// The host bookkeeping of solve! for groups of sparse conic QPs (calipso.jl_amd/csrc/sparse_solve_group.hpp) on the CPU: only that header and what it includes, the
// plain host compiler, the address and undefined-behaviour sanitizers.  tests/test_sparse_solve_group_host_cpu.py builds and runs it.
//   main layout            sweeps (members, nx, ne, nc, cones) and checks the member-major slab of the solve's arrays: no two pieces share an address, every piece lies
//                          inside the slab, the pieces cover it, member m's piece begins m strides after member 0's, the mask words fit their piece
//   main checks            prints what the argument checks say about a fixed list of calls
//   main recorded <file>   drives the lockstep as sparse_solve_group.hip's solve() does on what the ORACLE read step by step (tests/golden/sparse_solve_group_small.txt):
//                          published blocks, masks, candidates, and per search_direction! the inertias and norms, which go through the search_direction lockstep of
//                          sparse_kkt_group.hpp begun for the stepping subset (see run_recorded)
//   main replay <file>     drives the lockstep as sparse_solve_group.hip's solve() does, with read-backs made from per-member schedules.  The file:
//                          "N ne nc members continue_after_refinement_failure", then per member "events" and that many events in the order the member meets them:
//                          "O" (its prologue says inner convergence: an outer update), "X" (its prologue says solved), "S trials status factorizations rounds" (a
//                          step: what its search_direction returns, and how many line-search trials its candidate needs).  Published blocks are built so that the
//                          decisions of step_decisions.hpp come out as the event says.  Prints per member its status, counts and scalars, then the report.  A member
//                          that is live with no event left, or ends with events unread (other than by a refinement failure), fails the run
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "../../calipso.jl_amd/csrc/sparse_solve_group.hpp"

using namespace calipso::sparse_solve_group;
using calipso::i64;
namespace ssv = calipso::sparse_solve;

static bool check_layout(long long members, long long nx, long long ne, long long nc, long long n_small, long long n_wide) {
    const ssv::Layout one = ssv::layout(nx, ne, nc, n_small, n_wide);
    const Layout l = layout(members, nx, ne, nc, one);
    const auto bad = [&](const char* what) { std::printf("layout(%lld, %lld, %lld, %lld, %lld, %lld): %s\n", members, nx, ne, nc, n_small, n_wide, what); return false; };
    const long long N = nx + 2 * ne + 3 * nc, n = nx + ne + nc;
    const long long want[A_COUNT] = {N, ne, n, nc, nc, nc, ne, nc, ne, nc, nx, nx, ne, nc, one.doubles, (one.mask_ints + 1) / 2, PUB_STRIDE, DS_STRIDE, 1};
    if (2 * l.stride[A_WSM] < one.mask_ints) return bad("the mask words do not fit their piece");
    if (PUB_STRIDE * (long long)sizeof(double) < (long long)ssv::PUB_BYTES) return bad("a published block does not fit its piece");
    struct Piece { long long begin, end; };
    std::vector<Piece> pieces;
    for (int a = 0; a < A_COUNT; ++a) {
        if (l.stride[a] != want[a]) return bad("a stride is not the array's own length");
        for (long long m = 0; m < members; ++m) {
            const long long at = l.at((Array)a, m);
            if (at != l.offset[a] + m * l.stride[a]) return bad("a member's piece is not m strides after member 0's");
            if (at < 0 || at + l.stride[a] > l.doubles) return bad("a piece leaves the slab");
            if (l.stride[a] > 0) pieces.push_back(Piece{at, at + l.stride[a]});
        }
    }
    std::sort(pieces.begin(), pieces.end(), [](const Piece& x, const Piece& y) { return x.begin < y.begin; });
    long long at = 0;
    for (const Piece& p : pieces) { if (p.begin != at) return bad(p.begin < at ? "two pieces overlap" : "a gap between two pieces"); at = p.end; }
    if (at != l.doubles) return bad("the pieces do not cover the slab");
    return true;
}

static int run_layout() {
    long long cases = 0, largest = 0;
    for (long long members : {1, 2, 3, 8, 127, 128})
        for (long long nx : {1, 7, 36, 1000, 100000})
            for (long long ne : {0, 1, 24, 60000})
                for (long long nc : {0, 1, 9, 280, 40000})
                    for (long long cones : {0, 1, 3}) {
                        const long long n_small = nc >= 3 * cones ? cones : 0, n_wide = nc >= 20 ? cones / 2 : 0;
                        if (!check_layout(members, nx, ne, nc, n_small, n_wide)) return 1;
                        ++cases;
                        largest = std::max(largest, layout(members, nx, ne, nc, ssv::layout(nx, ne, nc, n_small, n_wide)).doubles);
                    }
    std::printf("layout ok cases=%lld largest=%lld\n", cases, largest);
    return 0;
}

static void say(const std::string& s) { std::printf("%s\n", s.empty() ? "ok" : s.c_str()); }

static int run_checks() {
    const double x = 0.0;
    const char* attach = "calipso_hip_sparse_kkt_group_qp_attach";
    say(check_attach(attach, 3, 2, 1, &x, &x, &x));
    say(check_attach(attach, 3, 0, 0, &x, nullptr, nullptr));
    say(check_attach(attach, 3, 2, 1, nullptr, &x, &x));
    say(check_attach(attach, 3, 2, 1, &x, nullptr, &x));
    say(check_attach(attach, 3, 2, 1, &x, &x, nullptr));
    say(check_initialize("calipso_hip_sparse_kkt_group_initialize", 3, &x));
    say(check_initialize("calipso_hip_sparse_kkt_group_initialize", 3, nullptr));
    const char* solve = "calipso_hip_sparse_kkt_group_solve";
    const bool all[3] = {true, true, true}, no_gx[3] = {true, false, true};
    const long long nnz[3] = {5, 4, 3}, no_equalities[3] = {5, 0, 3};
    say(check_ready(solve, all, nnz, true, true, true));
    say(check_ready(solve, no_gx, no_equalities, true, true, true));
    say(check_ready(solve, no_gx, nnz, true, true, true));
    say(check_ready(solve, all, nnz, false, true, true));
    say(check_ready(solve, all, nnz, true, false, true));
    say(check_ready("calipso_hip_sparse_kkt_group_initialize", all, nnz, true, false, false));
    say(check_solve(solve, nullptr));
    say(check_keep_trace("calipso_hip_sparse_kkt_group_keep_trace", 1));
    say(check_keep_trace("calipso_hip_sparse_kkt_group_keep_trace", 0));
    say(check_trace("calipso_hip_sparse_kkt_group_trace", nullptr, 2));
    say(check_trace("calipso_hip_sparse_kkt_group_trace", &x, -1));
    const char* get = "calipso_hip_sparse_kkt_group_get";
    say(check_named_vector(get, "solution", &x, 3 + 2 * 2 + 3 * 1, 3, 2, 1));
    say(check_named_vector(get, "dual", &x, 3, 3, 2, 1));
    say(check_named_vector(get, "differentiate_slacks", &x, 2, 3, 2, 1));
    say(check_named_vector(get, nullptr, &x, 2, 3, 2, 1));
    say(calipso::sparse_kkt_group::check_member(get, 4, 4));
    return 0;
}

struct Event { char kind; int trials, status, factorizations, rounds; };

static int run_replay(const char* path) {
    std::ifstream in(path);
    long long N, ne, nc; int members, cont;
    if (!(in >> N >> ne >> nc >> members >> cont)) { std::printf("replay: bad header\n"); return 1; }
    std::vector<std::vector<Event>> events((size_t)members);
    for (auto& ev : events) {
        int count; in >> count;
        for (int i = 0; i < count; ++i) {
            Event e{'?', 0, 0, 0, 0};
            in >> e.kind;
            if (e.kind == 'S') in >> e.trials >> e.status >> e.factorizations >> e.rounds;
            ev.push_back(e);
        }
    }
    if (!in) { std::printf("replay: bad file\n"); return 1; }
    std::vector<size_t> next((size_t)members, 0);
    std::vector<double> pub((size_t)members * (size_t)PUB_STRIDE, 0.0);
    Lockstep ls(members);
    calipso::Options opt;
    ls.begin(opt, cont != 0, N, ne, nc);
    const auto block = [&](int k) { return pub.data() + (size_t)k * (size_t)PUB_STRIDE; };
    const auto fail = [](int k, const char* what) { std::printf("replay: member %d: %s\n", k, what); return 1; };
    // the prologue the member's next event asks for: 'S' a large optimality error, 'O' none but a residual violation, 'X' nothing left
    const auto prologue = [&](int k) {
        double* p = block(k);
        for (int i = 8; i < 16; ++i) p[i] = 0.0;
        p[ssv::PUB_G_INF] = 0.0; p[ssv::PUB_PRODUCT_INF] = 0.0;
        if (next[(size_t)k] >= events[(size_t)k].size()) return false;
        const char kind = events[(size_t)k][next[(size_t)k]].kind;
        if (kind != 'X') p[ssv::PUB_RES_1] = 1.0e3 * (double)N;
        if (kind == 'S') p[ssv::PUB_RES_N_INF] = 1.0e6;
        p[ssv::PUB_MERIT] = 1.0; p[ssv::PUB_THETA] = 1.0;
        return true;
    };
    for (int k = 0; k < members; ++k) if (!prologue(k)) return fail(k, "no event at the start");
    ls.after_start(pub.data());
    std::vector<double> reg(3 * (size_t)members, 0.0), info(4 * (size_t)members, 0.0);
    std::vector<int32_t> status((size_t)members, 0);
    while (ls.any_live()) {
        ++ls.ticks;
        for (;;) {
            const std::vector<int> live = ls.in_phase(LIVE);
            const std::vector<int> who = ls.classify(pub.data());
            for (int k : live) {                                           // the classification is the event's
                const Event& e = events[(size_t)k][next[(size_t)k]];
                const Phase want = e.kind == 'S' ? STEPPING : e.kind == 'O' ? NEEDS_OUTER : ENDED;
                if (ls.m[(size_t)k].phase != want) return fail(k, "classified against its event");
                if (e.kind != 'S') ++next[(size_t)k];
            }
            if (who.empty()) break;
            const std::vector<int> with_prologue = ls.outer_begin(who);
            for (int k : with_prologue) if (!prologue(k)) return fail(k, "live with no event left");
            ls.outer_after(who, with_prologue);
        }
        const std::vector<int> stepping = ls.stepping();
        if (stepping.empty()) continue;
        ls.regularization_in(stepping, reg.data());
        for (int k : stepping) {
            const Event& e = events[(size_t)k][next[(size_t)k]];
            status[(size_t)k] = e.status; info[4 * (size_t)k] = e.factorizations; info[4 * (size_t)k + 1] = e.rounds;
            reg[3 * (size_t)k] = 1.0e-7; reg[3 * (size_t)k + 1] = 1.0 / (double)(1 + ls.m[(size_t)k].accepted); reg[3 * (size_t)k + 2] = 1.0e-7;
        }
        const std::vector<int> on = ls.after_search_direction(stepping, status.data(), info.data(), reg.data());
        if (on.empty()) continue;
        for (int k : on) {                                                 // clear masks: both step sizes 1; a candidate that is rejected while trials remain
            double* p = block(k);
            std::fill(p + ssv::PUB_DOUBLES, p + PUB_STRIDE, 0.0);
            p[ssv::PUB_STEP_S] = 1.0; p[ssv::PUB_STEP_T] = 1.0; p[ssv::PUB_DD] = -1.0;
            const bool reject = events[(size_t)k][next[(size_t)k]].trials > 0;
            p[ssv::PUB_CAND_THETA] = reject ? 2.0 : 0.0; p[ssv::PUB_CAND_MERIT] = reject ? 2.0 : 0.0;
        }
        ls.after_first_candidate(on, pub.data());
        for (;;) {
            const std::vector<int> who = ls.rejecting();
            if (who.empty()) break;
            for (int k : who) {
                const bool reject = ls.m[(size_t)k].line_search + 1 < events[(size_t)k][next[(size_t)k]].trials;
                block(k)[ssv::PUB_CAND_THETA] = reject ? 2.0 : 0.0; block(k)[ssv::PUB_CAND_MERIT] = reject ? 2.0 : 0.0;
            }
            ls.after_trial(who, pub.data());
        }
        const std::vector<int> who = ls.accepting();
        for (int k : who) {
            if (ls.m[(size_t)k].line_search != events[(size_t)k][next[(size_t)k]].trials) return fail(k, "took other line-search trials than its event says");
            ++next[(size_t)k];
            if (!prologue(k)) return fail(k, "live with no event left");
        }
        ls.after_accept(who, pub.data());
    }
    for (int k = 0; k < members; ++k) {
        const Member& q = ls.m[(size_t)k];
        if (q.status != STATUS_REFINEMENT && next[(size_t)k] != events[(size_t)k].size()) return fail(k, "ended with events unread");
        double out[INFO_DOUBLES];
        ls.info(k, 0.0, 0.0, 0.0, out);
        std::printf("member %d status %d total_iterations %lld outer %lld accepted %lld factorizations %lld max_rounds %lld refinement_failures %lld worst %d waits %lld trials %lld kappa %.17g rho %.17g ep_last %.17g\n",
                    k, q.status, (long long)q.total_iterations, (long long)q.outer, (long long)q.accepted, (long long)q.factorizations, (long long)q.max_rounds,
                    (long long)q.refinement_failures, q.worst, (long long)q.waits, (long long)q.trials, out[9], out[10], out[11]);
    }
    std::printf("report ticks %lld outer_rounds %lld trial_rounds %lld host_waits %lld worst %d\n", (long long)ls.ticks, (long long)ls.outer_rounds, (long long)ls.trial_rounds,
                (long long)ls.host_waits, ls.worst_status());
    return 0;
}

// ---- the lockstep on what the ORACLE read, step by step (tests/golden/sparse_solve_group_small.txt, recorded by sparse_solve_group_cases.record_solve) -------------
// The file: "N ne nc nx members continue", then per member "records" and that many records in the order the member consumes them:
//   P / A  16 doubles of the published block, |g|_inf, |s o t|_inf     a prologue at the start or behind an outer update / behind an accepted iterate
//   S      inertias norms, then that many inertia triples and norms      what its search_direction! reads: fed to the search_direction lockstep (sparse_kkt_group.hpp)
//   C      26 + 26 mask words, a_s a_t merit violation dd                the cone search and the first candidate
//   T      merit violation                                              a line-search trial
// A member that asks for a record of another kind than the next one, or ends with records unread, fails the run.
struct Record { char kind = '?'; std::vector<double> d; std::vector<long long> n; };

static int run_recorded(const char* path) {
    std::ifstream in(path);
    long long N, ne, nc, nx; int members, cont;
    if (!(in >> N >> ne >> nc >> nx >> members >> cont)) { std::printf("recorded: bad header\n"); return 1; }
    std::vector<std::vector<Record>> recs((size_t)members);
    for (auto& list : recs) {
        int count; in >> count;
        for (int i = 0; i < count; ++i) {
            Record r;
            in >> r.kind;
            size_t doubles = 0, ints = 0;
            if (r.kind == 'P' || r.kind == 'A') doubles = 18;
            else if (r.kind == 'C') { ints = 2 * calipso::CONE_MASK_WORDS; doubles = 5; }
            else if (r.kind == 'T') doubles = 2;
            else if (r.kind == 'S') { long long ni, nn; in >> ni >> nn; ints = 3 * (size_t)ni; doubles = (size_t)nn; }
            else { std::printf("recorded: unknown record %c\n", r.kind); return 1; }
            r.n.resize(ints); r.d.resize(doubles);
            for (long long& v : r.n) in >> v;
            for (double& v : r.d) in >> v;
            list.push_back(r);
        }
    }
    if (!in) { std::printf("recorded: bad file\n"); return 1; }
    std::vector<size_t> next((size_t)members, 0);
    std::vector<double> pub((size_t)members * (size_t)PUB_STRIDE, 0.0);
    const auto block = [&](int k) { return pub.data() + (size_t)k * (size_t)PUB_STRIDE; };
    bool failed = false;
    const auto take = [&](int k, char kind) -> const Record* {
        if (next[(size_t)k] >= recs[(size_t)k].size() || recs[(size_t)k][next[(size_t)k]].kind != kind) {
            std::printf("recorded: member %d asks for a record %c, the recording holds %s\n", k, kind,
                        next[(size_t)k] < recs[(size_t)k].size() ? std::string(1, recs[(size_t)k][next[(size_t)k]].kind).c_str() : "none");
            failed = true;
            return nullptr;
        }
        return &recs[(size_t)k][next[(size_t)k]++];
    };
    const auto prologue = [&](int k, char kind) {
        const Record* r = take(k, kind);
        if (!r) return;
        std::copy(r->d.begin(), r->d.begin() + 16, block(k));
        block(k)[ssv::PUB_G_INF] = r->d[16]; block(k)[ssv::PUB_PRODUCT_INF] = r->d[17];
    };
    Lockstep ls(members);
    calipso::sparse_kkt_group::Lockstep kl(members);
    calipso::Options opt;
    kl.opt = opt;
    ls.begin(opt, cont != 0, N, ne, nc);
    for (int k = 0; k < members; ++k) prologue(k, 'P');
    if (failed) return 1;
    ls.after_start(pub.data());
    std::vector<double> reg(3 * (size_t)members, 0.0), info(4 * (size_t)members, 0.0), norm((size_t)members, 0.0);
    std::vector<int32_t> status((size_t)members, 0);
    std::vector<int64_t> inertia(3 * (size_t)members, 0);
    long long sd_waits = 0;
    while (ls.any_live()) {
        ++ls.ticks;
        for (;;) {
            const std::vector<int> who = ls.classify(pub.data());
            if (who.empty()) break;
            const std::vector<int> with_prologue = ls.outer_begin(who);
            for (int k : with_prologue) prologue(k, 'P');
            if (failed) return 1;
            ls.outer_after(who, with_prologue);
        }
        const std::vector<int> stepping = ls.stepping();
        if (stepping.empty()) continue;
        // search_direction! of the stepping members through ITS lockstep, on the recorded inertias and norms
        std::vector<const Record*> sd((size_t)members, nullptr);
        std::vector<size_t> at_inertia((size_t)members, 0), at_norm((size_t)members, 0);
        for (int k : stepping) { sd[(size_t)k] = take(k, 'S'); kl.m[(size_t)k].sc = ls.m[(size_t)k].sc; }
        if (failed) return 1;
        ls.regularization_in(stepping, reg.data());
        kl.begin(reg.data(), stepping);
        for (;;) {
            const std::vector<int> walking = kl.walking();
            if (walking.empty()) break;
            for (int k : walking) {
                if (3 * at_inertia[(size_t)k] + 3 > sd[(size_t)k]->n.size()) { std::printf("recorded: member %d factors more often than the oracle\n", k); return 1; }
                for (int i = 0; i < 3; ++i) inertia[3 * (size_t)k + i] = sd[(size_t)k]->n[3 * at_inertia[(size_t)k] + i];
                ++at_inertia[(size_t)k];
            }
            kl.after_factorizations(walking, inertia.data(), nx, ne + nc);
            ++sd_waits;
        }
        kl.after_solve();
        std::vector<int> refining = kl.refining();
        for (bool first = true; !refining.empty(); first = false) {
            for (int k : refining) {
                if (at_norm[(size_t)k] >= sd[(size_t)k]->d.size()) { std::printf("recorded: member %d refines more often than the oracle\n", k); return 1; }
                norm[(size_t)k] = sd[(size_t)k]->d[at_norm[(size_t)k]++];
            }
            refining = kl.after_norms(refining, norm.data(), first);
            ++sd_waits;
        }
        ++sd_waits;                                                        // (the call's closing wait)
        for (int k : stepping)
            if (3 * at_inertia[(size_t)k] != sd[(size_t)k]->n.size() || at_norm[(size_t)k] != sd[(size_t)k]->d.size()) { std::printf("recorded: member %d left a read-back of its search_direction unread\n", k); return 1; }
        kl.outputs(reg.data(), info.data(), status.data(), stepping);
        const std::vector<int> on = ls.after_search_direction(stepping, status.data(), info.data(), reg.data());
        if (on.empty()) continue;
        for (int k : on) {
            const Record* r = take(k, 'C');
            if (!r) return 1;
            int* masks = reinterpret_cast<int*>(block(k) + ssv::PUB_DOUBLES);
            for (size_t i = 0; i < r->n.size(); ++i) masks[i] = (int)(uint32_t)r->n[i];
            block(k)[ssv::PUB_STEP_S] = r->d[0]; block(k)[ssv::PUB_STEP_T] = r->d[1]; block(k)[ssv::PUB_CAND_MERIT] = r->d[2]; block(k)[ssv::PUB_CAND_THETA] = r->d[3];
            block(k)[ssv::PUB_DD] = r->d[4];
        }
        ls.after_first_candidate(on, pub.data());
        for (;;) {
            const std::vector<int> who = ls.rejecting();
            if (who.empty()) break;
            for (int k : who) {
                const Record* r = take(k, 'T');
                if (!r) return 1;
                block(k)[ssv::PUB_CAND_MERIT] = r->d[0]; block(k)[ssv::PUB_CAND_THETA] = r->d[1];
            }
            ls.after_trial(who, pub.data());
        }
        const std::vector<int> who = ls.accepting();
        for (int k : who) prologue(k, 'A');
        if (failed) return 1;
        ls.after_accept(who, pub.data());
    }
    for (int k = 0; k < members; ++k) {
        const Member& q = ls.m[(size_t)k];
        if (next[(size_t)k] != recs[(size_t)k].size()) { std::printf("recorded: member %d ended with records unread\n", k); return 1; }
        std::printf("member %d status %d total_iterations %lld outer %lld accepted %lld factorizations %lld max_rounds %lld refinement_failures %lld worst %d waits %lld trials %lld kappa %.17g rho %.17g ep_last %.17g\n",
                    k, q.status, (long long)q.total_iterations, (long long)q.outer, (long long)q.accepted, (long long)q.factorizations, (long long)q.max_rounds,
                    (long long)q.refinement_failures, q.worst, (long long)q.waits, (long long)q.trials, q.sc.kappa, q.sc.rho, q.sc.ep_last);
    }
    std::printf("report ticks %lld outer_rounds %lld trial_rounds %lld host_waits %lld search_direction_waits %lld worst %d\n", (long long)ls.ticks, (long long)ls.outer_rounds,
                (long long)ls.trial_rounds, (long long)ls.host_waits, sd_waits, ls.worst_status());
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "layout") return run_layout();
    if (mode == "checks") return run_checks();
    if (mode == "replay" && argc > 2) return run_replay(argv[2]);
    if (mode == "recorded" && argc > 2) return run_recorded(argv[2]);
    std::printf("usage: main layout | checks | replay <file> | recorded <file>\n");
    return 2;
}
