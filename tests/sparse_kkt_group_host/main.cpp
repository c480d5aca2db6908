// The host bookkeeping of search_direction! for groups of sparse problems (calipso.jl_amd/csrc/sparse_kkt_group.hpp) on the CPU: only that header and
// step_decisions.hpp, the plain host compiler, the address and undefined-behaviour sanitizers.  tests/test_sparse_kkt_group_host_cpu.py builds and runs it.
//   main layout            sweeps (members, nnz of Lxx, gx, hx, nx, ne, nc) and checks the member-major slabs: no two pieces share an address, every piece lies
//                          inside the slab, the pieces cover it, member m's piece of an array begins m strides after member 0's
//   main checks            prints what the argument checks say about a fixed list of calls
//   main replay <file>     replays the lockstep on recorded read-backs.  The file: "nx m members max_regularization", then per member
//                          "kappa ep_last inertias norms" followed by that many inertia triples (one per factorisation, in order) and norms (one per H v pass, in
//                          order).  Prints the set of members of every factorisation round, of the solve, of every norm pass and every correction round, then per
//                          member its status, counts and regularisation, and the report.  A member that asks for a read-back the file does not hold, or leaves one
//                          unread, fails the run: the recorded sequences are exactly what the lockstep must consume
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "../../calipso.jl_amd/csrc/sparse_kkt_group.hpp"
#include "../../calipso.jl_amd/csrc/step_decisions.hpp"

using namespace calipso::sparse_kkt_group;
using calipso::i64;

static bool check_layout(long long members, long long nnzL, long long nnzg, long long nnzh, long long nx, long long ne, long long nc) {
    const long long N = nx + 2 * ne + 3 * nc, n = nx + ne + nc;
    const Layout l = layout(members, nnzL, nnzg, nnzh, N, n);
    const auto bad = [&](const char* what) { std::printf("layout(%lld, %lld, %lld, %lld, %lld, %lld): %s\n", members, nnzL, nnzg, nnzh, N, n, what); return false; };
    const long long want[A_COUNT] = {nnzL, nnzg, nnzh, N, 1, N, N, N, N, n, 1};
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
    for (const Piece& p : pieces) { if (p.begin != at) return bad(p.begin < at ? "two pieces overlap" : "a hole in the slab"); at = p.end; }
    if (at != l.doubles) return bad("the pieces do not cover the slab");
    return true;
}

static int run_layout() {
    long long cases = 0, largest = 0;
    for (long long members : {1, 2, 3, 7, 64, 128})
        for (long long nx : {1, 6, 12, 100000})
            for (long long ne : {0, 1, 4})
                for (long long nc : {0, 2, 12, 66})
                    for (long long fill : {0, 1, 3})
                        for (long long nnzh : {0LL, nc * fill}) {
                            if (!check_layout(members, nx * fill + (fill ? 1 : 0), ne * fill, nnzh, nx, ne, nc)) return 1;
                            ++cases;
                            largest = std::max(largest, layout(members, nx * fill + (fill ? 1 : 0), ne * fill, nnzh, nx + 2 * ne + 3 * nc, nx + ne + nc).doubles);
                        }
    std::printf("layout ok cases=%lld largest=%lld\n", cases, largest);
    return 0;
}

static void say(const std::string& text) { std::printf("%s\n", text.empty() ? "ok" : text.c_str()); }

static int run_checks() {
    static const char* const create = "calipso_hip_sparse_kkt_group_create";
    static const char* const option = "calipso_hip_sparse_kkt_group_set_option";
    double x = 0.0;
    say(check_members(create, 1)); say(check_members(create, 128)); say(check_members(create, 0)); say(check_members(create, 129)); say(check_members(create, -3));
    say(check_numeric_phase(create, 2)); say(check_numeric_phase(create, 1)); say(check_numeric_phase(create, 0));
    say(check_member("calipso_hip_sparse_kkt_group_get_matrix", 0, 6)); say(check_member("calipso_hip_sparse_kkt_group_get_matrix", 6, 6)); say(check_member("calipso_hip_sparse_kkt_group_get_matrix", -1, 6));
    say(check_option(option, "krylov_fallback", 0.0)); say(check_option(option, "krylov_fallback", 1.0)); say(check_option(option, "krylov_restart", 8.0));
    say(check_option(option, "max_regularization", 1e3));
    say(check_required("calipso_hip_sparse_kkt_group_factorize", "ep", &x)); say(check_required("calipso_hip_sparse_kkt_group_factorize", "ep", nullptr));
    return 0;
}

static void print_set(const char* what, const std::vector<int>& members) {
    std::printf("%s", what);
    for (int k : members) std::printf(" %d", k);
    std::printf("\n");
}

static int run_replay(const char* path) {
    std::ifstream in(path);
    if (!in) { std::printf("cannot read %s\n", path); return 2; }
    long long nx = 0, m_rows = 0, members = 0;
    double max_regularization = 0.0;
    in >> nx >> m_rows >> members >> max_regularization;
    if (!in || !check_members("replay", members).empty()) { std::printf("bad header\n"); return 2; }
    Lockstep ls((int)members);
    ls.opt.max_regularization = max_regularization;
    std::vector<std::vector<int64_t>> inertias((size_t)members);
    std::vector<std::vector<double>> norms((size_t)members);
    std::vector<size_t> next_inertia((size_t)members, 0), next_norm((size_t)members, 0);
    std::vector<double> regularization(3 * (size_t)members, 0.0);
    for (long long k = 0; k < members; ++k) {
        double kappa = 0.0, ep_last = 0.0; long long ni = 0, nn = 0;
        in >> kappa >> ep_last >> ni >> nn;
        ls.m[(size_t)k].sc.kappa = kappa; regularization[3 * (size_t)k + 1] = ep_last;
        inertias[(size_t)k].resize(3 * (size_t)ni); norms[(size_t)k].resize((size_t)nn);
        for (int64_t& v : inertias[(size_t)k]) { long long t = 0; in >> t; v = t; }
        for (double& v : norms[(size_t)k]) in >> v;
        if (!in) { std::printf("bad member %lld\n", k); return 2; }
    }
    ls.begin(regularization.data());
    std::vector<int64_t> inertia(3 * (size_t)members, 0);
    for (;;) {
        const std::vector<int> walking = ls.walking();
        if (walking.empty()) break;
        print_set("factor", walking);
        for (int k : walking) {
            if (3 * next_inertia[(size_t)k] + 3 > inertias[(size_t)k].size()) { std::printf("member %d asks for a factorisation that was not recorded\n", k); return 1; }
            std::copy(inertias[(size_t)k].begin() + 3 * (long)next_inertia[(size_t)k], inertias[(size_t)k].begin() + 3 * (long)next_inertia[(size_t)k] + 3, inertia.begin() + 3 * k);
            ++next_inertia[(size_t)k];
        }
        ls.after_factorizations(walking, inertia.data(), nx, m_rows);
    }
    print_set("solve", ls.passed());
    ls.after_solve();
    std::vector<double> norm((size_t)members, 0.0);
    std::vector<int> refining = ls.refining();
    for (bool first = true; !refining.empty(); first = false) {
        print_set("norms", refining);
        for (int k : refining) {
            if (next_norm[(size_t)k] >= norms[(size_t)k].size()) { std::printf("member %d asks for a norm that was not recorded\n", k); return 1; }
            norm[(size_t)k] = norms[(size_t)k][next_norm[(size_t)k]++];
        }
        refining = ls.after_norms(refining, norm.data(), first);
        if (!refining.empty()) print_set("round", refining);
    }
    std::vector<double> info(4 * (size_t)members, 0.0);
    std::vector<int32_t> status((size_t)members, 0);
    ls.outputs(regularization.data(), info.data(), status.data());
    for (long long k = 0; k < members; ++k) {
        if (3 * next_inertia[(size_t)k] != inertias[(size_t)k].size() || (status[(size_t)k] != STATUS_INERTIA && next_norm[(size_t)k] != norms[(size_t)k].size())) {
            std::printf("member %lld left recorded read-backs unread\n", k); return 1;
        }
        std::printf("member %lld status %d factorizations %d rounds %d ep %.17g ep_last %.17g ed %.17g\n", k, (int)status[(size_t)k], (int)info[4 * (size_t)k], (int)info[4 * (size_t)k + 1],
                    regularization[3 * (size_t)k], regularization[3 * (size_t)k + 1], regularization[3 * (size_t)k + 2]);
    }
    std::printf("report factor_rounds %d refine_rounds %d last_factor_active %d last_refine_active %d worst %d\n", ls.factor_rounds, ls.refine_rounds, ls.last_factor_active,
                ls.last_refine_active, ls.worst());
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "layout") return run_layout();
    if (mode == "checks") return run_checks();
    if (mode == "replay" && argc > 2) return run_replay(argv[2]);
    std::printf("usage: main layout | checks | replay <file>\n");
    return 2;
}
