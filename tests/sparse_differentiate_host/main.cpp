// The shared pieces of differentiate! on the sparse handle (calipso.jl_amd/csrc/sparse_differentiate.hpp) on the CPU: only that header and sparse_kkt.hpp, the plain
// host compiler, the address and undefined-behaviour sanitizers.  tests/test_sparse_differentiate_host_cpu.py builds and runs it.
//   main maps      for an equality row, a nonnegative row and second-order cones of dimension 2, 3, 5 and 70 at random interior s, t with ep = 0.12, ed = 0.21, rho = 52:
//                  the dense matrices of the forward pre and post functions and of the transposed ones, built from unit vectors; each transposed matrix must equal
//                  the transpose within 64 eps (largest entry).  Prints one line per case with the worst deviation in units of eps * largest entry
//   main layout    sweeps (N, n, k, rounds) and checks the workspace layout: regions inside the workspace, no overlap, no hole
//   main checks    prints what the argument checks say about a fixed list of calls
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "../../calipso.jl_amd/csrc/sparse_differentiate.hpp"
#include "../../calipso.jl_amd/csrc/sparse_kkt.hpp"

using namespace calipso::sparse_differentiate;

namespace {

// SplitMix64: the same points on every machine
struct Rng {
    uint64_t x;
    double uniform() {
        x += 0x9E3779B97F4A7C15ull;
        uint64_t z = x;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
        return (double)(z >> 11) * (1.0 / 9007199254740992.0);
    }
};

typedef std::vector<double> Vec;
struct Mat {
    int rows, cols; Vec a;
    Mat(int r, int c) : rows(r), cols(c), a((size_t)r * (size_t)c, 0.0) {}
    double& at(int i, int j) { return a[(size_t)i + (size_t)j * (size_t)rows]; }
    double at(int i, int j) const { return a[(size_t)i + (size_t)j * (size_t)rows]; }
};

// the worst |A(i, j) - B(j, i)| in units of eps * (largest entry of either); < 0: the shapes do not match
double transpose_gap(const Mat& A, const Mat& B) {
    if (A.rows != B.cols || A.cols != B.rows) return -1.0;
    double big = 0.0, gap = 0.0;
    for (int i = 0; i < A.rows; ++i)
        for (int j = 0; j < A.cols; ++j) {
            big = std::fmax(big, std::fmax(std::fabs(A.at(i, j)), std::fabs(B.at(j, i))));
            gap = std::fmax(gap, std::fabs(A.at(i, j) - B.at(j, i)));
        }
    if (!(big > 0.0)) return -1.0;                      // a map that is identically zero checks nothing
    return gap / (std::numeric_limits<double>::epsilon() * big);
}

const MapScalars SC{0.12, 0.21, 52.0};
constexpr double BOUND = 64.0;

bool report(const char* name, int dm, const double gaps[3]) {
    bool ok = true;
    for (int i = 0; i < 3; ++i) ok = ok && gaps[i] >= 0.0 && gaps[i] <= BOUND;
    std::printf("%s %d pre' %.3g post'(solution) %.3g post'(residual) %.3g %s\n", name, dm, gaps[0], gaps[1], gaps[2], ok ? "ok" : "FAILED");
    return ok;
}

// A cone block of dimension dm (dm = 1 with soc = false: a nonnegative row).  The forward maps as matrices:
//   Fc (dm x 3 dm)      rsym_c from (r_s, r_z, r_t)                       forward pre
//   Ec (3 dm x dm)      (Ds, dz, Dt) from the symmetric solution dz       forward post, residual zero
//   Dc (2 dm x 2 dm)    (Ds, Dt) from (r_s, r_t)                          forward post, solution zero
// and the transposed ones: pre g from (v_s, v_z, v_t) must be Ec', post (l_s, l_z, l_t) from h must be Fc', post (l_s, l_t) from (v_s, v_t) must be Dc'
bool cone_case(bool soc, int dm, Rng& rng) {
    Vec s((size_t)dm), t((size_t)dm);
    if (soc) {       // interior: the first entry above the norm of the tail
        double ns = 0.0, nt = 0.0;
        for (int i = 1; i < dm; ++i) { s[(size_t)i] = rng.uniform() - 0.5; t[(size_t)i] = rng.uniform() - 0.5; ns += s[(size_t)i] * s[(size_t)i]; nt += t[(size_t)i] * t[(size_t)i]; }
        s[0] = std::sqrt(ns) + 0.5 + rng.uniform(); t[0] = std::sqrt(nt) + 0.5 + rng.uniform();
    } else { s[0] = 0.5 + rng.uniform(); t[0] = 0.5 + rng.uniform(); }
    const Vec zero((size_t)dm, 0.0);
    const auto unit = [&](int j) { Vec e((size_t)dm, 0.0); e[(size_t)j] = 1.0; return e; };
    Mat Fc(dm, 3 * dm), Ec(3 * dm, dm), Dc(2 * dm, 2 * dm), Tpre(dm, 3 * dm), Tpost_h(3 * dm, dm), Tpost_v(2 * dm, 2 * dm);
    Vec o1((size_t)dm), o2((size_t)dm), o3((size_t)dm), o4((size_t)dm);
    for (int part = 0; part < 3; ++part)
        for (int j = 0; j < dm; ++j) {
            const Vec e = unit(j);
            const Vec &a = part == 0 ? e : zero, &b = part == 1 ? e : zero, &c = part == 2 ? e : zero;      // (s, z, t) parts
            if (soc) { soc_forward_pre(SC, dm, s.data(), t.data(), a.data(), b.data(), c.data(), o1.data()); soc_transposed_pre(SC, dm, s.data(), t.data(), a.data(), b.data(), c.data(), o2.data(), o3.data(), o4.data()); }
            else { o1[0] = nonnegative_forward_pre(SC, s[0], t[0], a[0], b[0], c[0]); o2[0] = nonnegative_transposed_pre(SC, s[0], t[0], a[0], b[0], c[0]); }
            for (int i = 0; i < dm; ++i) { Fc.at(i, part * dm + j) = o1[(size_t)i]; Tpre.at(i, part * dm + j) = o2[(size_t)i]; }
        }
    for (int j = 0; j < dm; ++j) {       // the dependence on the symmetric solution / on h
        const Vec e = unit(j);
        if (soc) soc_forward_post(SC, dm, s.data(), t.data(), e.data(), zero.data(), zero.data(), o1.data(), o2.data());
        else nonnegative_forward_post(SC, s[0], t[0], e[0], 0.0, 0.0, &o1[0], &o2[0]);
        for (int i = 0; i < dm; ++i) { Ec.at(i, j) = o1[(size_t)i]; Ec.at(dm + i, j) = e[(size_t)i]; Ec.at(2 * dm + i, j) = o2[(size_t)i]; }
        if (soc) soc_transposed_post(SC, dm, s.data(), t.data(), e.data(), zero.data(), zero.data(), o1.data(), o2.data());
        else nonnegative_transposed_post(SC, s[0], t[0], e[0], 0.0, 0.0, &o1[0], &o2[0]);
        for (int i = 0; i < dm; ++i) { Tpost_h.at(i, j) = o1[(size_t)i]; Tpost_h.at(dm + i, j) = e[(size_t)i]; Tpost_h.at(2 * dm + i, j) = o2[(size_t)i]; }
    }
    for (int part = 0; part < 2; ++part)       // the direct dependence on the residual / on v: (s, t) parts
        for (int j = 0; j < dm; ++j) {
            const Vec e = unit(j);
            const Vec &a = part == 0 ? e : zero, &c = part == 1 ? e : zero;
            if (soc) soc_forward_post(SC, dm, s.data(), t.data(), zero.data(), a.data(), c.data(), o1.data(), o2.data());
            else nonnegative_forward_post(SC, s[0], t[0], 0.0, a[0], c[0], &o1[0], &o2[0]);
            for (int i = 0; i < dm; ++i) { Dc.at(i, part * dm + j) = o1[(size_t)i]; Dc.at(dm + i, part * dm + j) = o2[(size_t)i]; }
            if (soc) soc_transposed_post(SC, dm, s.data(), t.data(), zero.data(), a.data(), c.data(), o1.data(), o2.data());
            else nonnegative_transposed_post(SC, s[0], t[0], 0.0, a[0], c[0], &o1[0], &o2[0]);
            for (int i = 0; i < dm; ++i) { Tpost_v.at(i, part * dm + j) = o1[(size_t)i]; Tpost_v.at(dm + i, part * dm + j) = o2[(size_t)i]; }
        }
    const double gaps[3] = {transpose_gap(Tpre, Ec), transpose_gap(Tpost_h, Fc), transpose_gap(Tpost_v, Dc)};
    return report(soc ? "second_order" : "nonnegative", dm, gaps);
}

// an equality row: rsym_e from (r_r, r_y); (Dr, dy) from dy; Dr from r_r — and their transposes
bool equality_case() {
    Mat F(1, 2), E(2, 1), D(1, 1), Tpre(1, 2), Tpost_h(2, 1), Tpost_v(1, 1);
    F.at(0, 0) = equality_forward_pre(SC, 1.0, 0.0); F.at(0, 1) = equality_forward_pre(SC, 0.0, 1.0);
    Tpre.at(0, 0) = equality_transposed_pre(SC, 1.0, 0.0); Tpre.at(0, 1) = equality_transposed_pre(SC, 0.0, 1.0);
    E.at(0, 0) = equality_forward_post(SC, 1.0, 0.0); E.at(1, 0) = 1.0;
    Tpost_h.at(0, 0) = equality_transposed_post(SC, 1.0, 0.0); Tpost_h.at(1, 0) = 1.0;
    D.at(0, 0) = equality_forward_post(SC, 0.0, 1.0);
    Tpost_v.at(0, 0) = equality_transposed_post(SC, 0.0, 1.0);
    const double gaps[3] = {transpose_gap(Tpre, E), transpose_gap(Tpost_h, F), transpose_gap(Tpost_v, D)};
    return report("equality", 1, gaps);
}

int run_maps() {
    Rng rng{20240611ull};
    bool ok = equality_case();
    ok = cone_case(false, 1, rng) && ok;
    for (int dm : {2, 3, 5, 70}) ok = cone_case(true, dm, rng) && ok;
    std::printf(ok ? "maps ok\n" : "maps FAILED\n");
    return ok ? 0 : 1;
}

bool check_layout(size_t N, size_t n, size_t k, bool rounds) {
    const Layout l = layout(N, n, k, rounds);
    const auto bad = [&](const char* what) { std::printf("layout(%zu, %zu, %zu, %d): %s\n", N, n, k, (int)rounds, what); return false; };
    const Region* regions[8] = {&l.V, &l.X, &l.rsym, &l.dsym, &l.E, &l.C, &l.Xsave, &l.norms};
    const size_t want[8] = {N * k, N * k, n * k, n * k, rounds ? N * k : 0, rounds ? N * k : 0, rounds ? N * k : 0, rounds ? k : 0};
    std::vector<char> used(l.doubles, 0);
    for (int r = 0; r < 8; ++r) {
        if (regions[r]->len != want[r]) return bad("a region's length");
        if (regions[r]->off + regions[r]->len > l.doubles) return bad("a region beyond the workspace");
        for (size_t i = 0; i < regions[r]->len; ++i) { char& u = used[regions[r]->off + i]; if (u) return bad("two regions overlap"); u = 1; }
    }
    for (char u : used) if (!u) return bad("a hole in the workspace");
    if (l.ints != (rounds ? 2 * k : 0)) return bad("the column masks");
    return true;
}
int run_layout() {
    long cases = 0;
    for (size_t nx : {1, 6, 70})
        for (size_t ne : {0, 1, 5})
            for (size_t nc : {0, 2, 66})
                for (size_t k : {1, 2, 3, 64, 65, 257})
                    for (int rounds = 0; rounds < 2; ++rounds) { if (!check_layout(nx + 2 * ne + 3 * nc, nx + ne + nc, k, rounds != 0)) return 1; ++cases; }
    std::printf("layout ok cases=%ld\n", cases);
    return 0;
}

int run_checks() {
    const auto say = [](const std::string& t) { std::printf("%s\n", t.empty() ? "ok" : t.c_str()); };
    double x = 0.0;
    say(check_columns("differentiate", 1));
    say(check_columns("differentiate", 65535));
    say(check_columns("differentiate", 0));
    say(check_columns("differentiate", -3));
    say(check_columns("differentiate", 65536));
    say(check_array("solve_columns", "B", &x));
    say(check_array("solve_columns", "B", nullptr));
    say(check_gradients("differentiate_adjoint", false, false, false));
    say(check_gradients("differentiate_adjoint", true, true, true));
    say(check_gradients("differentiate_adjoint", true, false, true));
    say(check_gradients("differentiate_adjoint", true, true, false));
    std::printf("option %d %d %d %d %d\n", (int)refinement_option(0.0), (int)refinement_option(1.0), (int)refinement_option(2.0), (int)refinement_option(-1.0), (int)refinement_option(0.5));
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "maps") return run_maps();
    if (what == "layout") return run_layout();
    if (what == "checks") return run_checks();
    std::printf("usage: main maps | layout | checks\n");
    return 2;
}
