// The host tables of a trajectory evaluator (include/calipso_trajectory_tables.hpp) without a GPU (tests/test_trajectory_codegen_cpu.py): the blob's checks, the address
// table of a route and its fill chunks, under the address and undefined-behaviour sanitizers.  Input (text): NT, the six shape arrays (kind, nv, m, nth, nd, nq), the
// number of words and the blob of TrajectoryProblem.tables(), then the layout: "dense LD", or "block NJ NH TOTAL" and NJ Jacobian + NH Hessian block descriptors
// "row0 nrows col0 ncols offset ld" (offset into one storage of TOTAL doubles, in place of the device pointer).  Output: "refused" when the blob is, else "rc N" and,
// for rc = 0, one line per table of the route.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "calipso_trajectory_tables.hpp"

using namespace calipso::trajectory;

static void dump(const char* name, int k, const std::vector<int32_t>& words, int at, size_t count) {
    printf("%s %d", name, k);
    for (size_t e = 0; e < count; ++e) printf(" %d", words.at((size_t)at + e));
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* fh = fopen(argv[1], "r");
    if (!fh) return 2;
    auto ints = [&](size_t n) { std::vector<int> v(n); for (int& e : v) if (fscanf(fh, "%d", &e) != 1) exit(3); return v; };
    const int nt = ints(1)[0];
    const std::vector<int> kind = ints(nt), nv = ints(nt), m = ints(nt), nth = ints(nt), nd = ints(nt), nq = ints(nt);
    const Shape sh{nt, kind.data(), nv.data(), m.data(), nth.data(), nd.data(), nq.data()};
    const int words = ints(1)[0];
    const std::vector<int> blob = ints((size_t)words);          // (exactly `words` of them on the heap: the sanitizer sees a read past the end)
    Tables u;
    if (!parse_tables(sh, blob.data(), words, u)) { printf("refused\ndone\n"); return 0; }
    char layout[16];
    if (fscanf(fh, "%15s", layout) != 1) return 3;
    RouteTable r;
    int rc;
    if (!strcmp(layout, "dense")) {
        rc = dense_route(sh, u, ints(1)[0], r);
    } else {
        const std::vector<int> count = ints(3);
        std::vector<double> storage((size_t)count[2]);
        std::vector<calipso_device_block> blocks((size_t)(count[0] + count[1]));
        for (calipso_device_block& b : blocks) {
            const std::vector<int> d = ints(6);
            b.row0 = d[0]; b.nrows = d[1]; b.col0 = d[2]; b.ncols = d[3]; b.values = storage.data() + d[4]; b.ld = d[5];
        }
        calipso_device_block_data out;
        memset(&out, 0, sizeof(out));
        out.nx = u.nx; out.np = u.np; out.ne = u.ne; out.nc = u.nc;
        out.n_jacobian_blocks = count[0]; out.jacobian_blocks = blocks.data();
        out.n_hessian_blocks = count[1]; out.hessian_blocks = blocks.data() + count[0];
        double* base = nullptr;
        rc = block_route(sh, u, &out, r, &base);
        if (rc == 0 && base != storage.data()) return 4;         // (the test's first block starts the storage)
    }
    printf("rc %d\n", rc);
    if (rc == 0) {
        for (int k = 0; k < nt; ++k) {
            const size_t n = (size_t)u.n[k];
            dump("vi", k, r.words, r.vi[k], nv[k] * n); dump("ri", k, r.words, r.ri[k], m[k] * n); dump("pi", k, r.words, r.pi[k], nth[k] * n);
            dump("ad", k, r.words, r.ad[k], nd[k] * n);
        }
        dump("g_addr", 0, r.words, r.g_addr, (size_t)u.G); dump("g_field", 0, r.words, r.g_field, (size_t)u.G);
        dump("g_slots", 0, r.words, r.g_slots, (size_t)u.G * u.W); dump("obj_slots", 0, r.words, r.obj_slots, (size_t)u.n_obj);
        for (int c = 0; c < N_FILL; ++c) {                       // per category: offset length offset length ...
            printf("fill %d", c);
            for (int e = r.fill_first[c]; e < r.fill_first[c] + r.fill_count[c]; ++e) printf(" %d %d", r.words.at((size_t)(r.c_off + e)), r.words.at((size_t)(r.c_len + e)));
            printf("\n");
        }
        printf("words 0 %zu\n", r.words.size());
    }
    printf("done\n");
    return 0;
}
