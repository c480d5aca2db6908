// The per-template device functions of calipso.jl_amd/trajectory.py on the host (tests/test_trajectory_codegen_cpu.py): __device__ defined away, the generated file
// included, every instance of every template called with all flags through <name>_template.  The destinations are mocked: the vector fields are plain arrays; the
// address table of a template is the identity into a buffer of its own (entry e of instance s at e * n + s), so that every direct entry comes back where the test can
// name it.  Input (text): nx ne nc np NT, the point x, y, z, theta, then per template: n nv m nth nd nq and its tables vi, ri, pi.  Output: one line per array.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#define __device__
#include TEMPLATES_FILE

static void dump(const char* name, int k, const std::vector<double>& v) {
    printf("%s %d", name, k);
    for (double e : v) printf(" %.17g", e);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* fh = fopen(argv[1], "r");
    if (!fh) return 2;
    int nx, ne, nc, np, nt;
    if (fscanf(fh, "%d %d %d %d %d", &nx, &ne, &nc, &np, &nt) != 5) return 3;
    auto reals = [&](int n) { std::vector<double> v(n); for (double& e : v) if (fscanf(fh, "%lf", &e) != 1) exit(3); return v; };
    auto ints = [&](int n) { std::vector<int> v(n); for (int& e : v) if (fscanf(fh, "%d", &e) != 1) exit(3); return v; };
    const std::vector<double> x = reals(nx), y = reals(ne), z = reals(nc), th = reals(np);
    const double NaN = NAN;
    std::vector<double> fx(nx, NaN), g(ne, NaN), h(nc, NaN);
    for (int k = 0; k < nt; ++k) {
        const std::vector<int> shape = ints(6);
        const int n = shape[0], nv = shape[1], m = shape[2], nth = shape[3], nd = shape[4], nq = shape[5];
        const std::vector<int> vi = ints(nv * n), ri = ints(m * n), pi = ints(nth * n);
        std::vector<int> ad(nd * n);
        for (int e = 0; e < nd * n; ++e) ad[e] = e;
        std::vector<double> direct(nd * n, NaN), part(nq * n, NaN);
        double* base[12] = {fx.data(), g.data(), h.data(), direct.data(), direct.data(), direct.data(), direct.data(), nullptr, nullptr, nullptr, nullptr, nullptr};
        for (int s = 0; s < n + 3; ++s)          // (three lanes past the last instance: they must do nothing)
            NAME_TEMPLATE(k, 0xffffu, s, n, x.data(), y.data(), z.data(), th.data(), vi.data(), ri.data(), pi.data(), ad.data(), base, part.data());
        dump("direct", k, direct);
        dump("part", k, part);
    }
    dump("fx", 0, fx);
    dump("g", 0, g);
    dump("h", 0, h);
    printf("done\n");
    return 0;
}
