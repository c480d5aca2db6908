// A generated evaluator (calipso.jl_amd/codegen.py: Problem.evaluator_source()) on the CPU: a mock of the batch kernel's context with the members the generated
// code may use and nothing else, every hook called for each thread id in turn.  Built by tests/test_codegen_cpu.py with the plain host compiler (no HIP include
// path) under the address and undefined-behaviour sanitizers, with -DEVALUATOR_FILE="..." -DEVALUATOR=Type -DNX= -DNE= -DNC= -DNP=.  Every array has exactly the
// size the kernel gives it, so an index of a static table that is out of range is caught.  Reads points (w then theta, one number per line) from argv[1] and prints
//     <array> <threads> <point> <values ...>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <limits>
#include <vector>

#define __device__

struct Dm {
    int nx, ne, nc, m, N, ldz;
    int oy() const { return nx + ne + nc; }
    int oz() const { return nx + ne + nc + ne; }
};

template <int NT> struct Ctx {
    static constexpr int threads = NT;
    int tid;
    Dm d;
    const double* theta;
    double *fx, *Z, *Hw;
    double* total;                                     // c.sum across the sequential "threads": the sum so far
    template <int K> void sum(double (&v)[K]) {
        for (int k = 0; k < K; ++k) { total[k] += v[k]; v[k] = total[k]; }
    }
};

#include EVALUATOR_FILE

static void print(const char* name, int threads, int point, const std::vector<double>& v) {
    printf("%s %d %d", name, threads, point);
    for (double x : v) printf(" %.17g", x);
    printf("\n");
}

template <int NT> static void run(int point, const std::vector<double>& w, const std::vector<double>& theta) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    Dm d{NX, NE, NC, NE + NC, NX + 2 * NE + 3 * NC, ((NE + NC + 2) | 1)};
    std::vector<double> out(d.m, nan), fx(d.nx, nan), Z((size_t)d.ldz * d.nx, nan), Hw((size_t)d.nx * d.nx, nan), J((size_t)d.N * NP, 0.0);
    double total[1] = {0.0};
    Ctx<NT> c{0, d, theta.data(), fx.data(), Z.data(), Hw.data(), total};
    double f = nan;
    for (c.tid = 0; c.tid < NT; ++c.tid) f = EVALUATOR::objective(c, w.data());
    print("objective", NT, point, {f});
    for (c.tid = 0; c.tid < NT; ++c.tid) EVALUATOR::constraints(c, w.data(), out.data());
    print("constraints", NT, point, out);
    for (c.tid = 0; c.tid < NT; ++c.tid) EVALUATOR::derivatives(c, w.data());
    print("fx", NT, point, fx);
    std::vector<double> Zd((size_t)d.m * d.nx);        // without the padding rows of the leading dimension (which nobody may have written: still NaN)
    for (int col = 0; col < d.nx; ++col)
        for (int r = 0; r < d.ldz; ++r) {
            if (r < d.m) Zd[r + (size_t)col * d.m] = Z[r + (size_t)col * d.ldz];
            else if (Z[r + (size_t)col * d.ldz] == Z[r + (size_t)col * d.ldz]) { printf("padding of Z written\n"); exit(1); }
        }
    print("Z", NT, point, Zd);
    print("Hw", NT, point, Hw);
#if NP > 0
    for (c.tid = 0; c.tid < NT; ++c.tid) EVALUATOR::jacobian_parameters(c, w.data(), J.data());
#endif
    print("J", NT, point, J);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* fh = fopen(argv[1], "r");
    if (!fh) return 2;
    const int N = NX + 2 * NE + 3 * NC;
    for (int point = 0;; ++point) {
        std::vector<double> w(N), theta(NP);
        bool ok = true;
        for (double& v : w) ok = ok && fscanf(fh, "%lf", &v) == 1;
        for (double& v : theta) ok = ok && fscanf(fh, "%lf", &v) == 1;
        if (!ok) break;
        run<1>(point, w, theta);
        run<64>(point, w, theta);
        run<256>(point, w, theta);
    }
    fclose(fh);
    printf("done\n");
    return 0;
}
