// The sparse route of a trajectory evaluator's host tables WITH the stored parameter patterns of a sparse handle (include/calipso_trajectory_tables.hpp: SparseLayout,
// sparse_route) without a GPU (tests/test_trajectory_sparse_parameter_route_cpu.py), under the address and undefined-behaviour sanitizers.  Input (text): as
// sparse_route_main.cpp — NT, the six shape arrays, the blob, the sizes "nx np ne nc", the three stored patterns Lxx, gx, hx — then "1" and the three parameter
// patterns Lp, gp, hp, each as "nnz", np + 1 column pointers and nnz row indices, 1-based; or "0": the parameter pointers stay NULL.  Output: as sparse_route_main.cpp.
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
    const std::vector<int> blob = ints((size_t)words);
    Tables u;
    if (!parse_tables(sh, blob.data(), words, u)) { printf("refused\ndone\n"); return 0; }
    const std::vector<int> sizes = ints(4);
    std::vector<int64_t> colptr[6], rowval[6];                  // (exactly as long as the pattern says: the sanitizer sees a read past the end)
    auto pattern = [&](int k, int cols) {
        const int nnz = ints(1)[0];
        for (int e : ints((size_t)cols + 1)) colptr[k].push_back(e);
        for (int e : ints((size_t)nnz)) rowval[k].push_back(e);
    };
    for (int k = 0; k < 3; ++k) pattern(k, sizes[0]);
    const int with = ints(1)[0];
    for (int k = 3; k < 6 && with; ++k) pattern(k, sizes[1]);
    calipso_device_sparse_data out;
    memset(&out, 0, sizeof(out));
    out.nx = sizes[0]; out.np = sizes[1]; out.ne = sizes[2]; out.nc = sizes[3];
    out.Lxx_colptr = colptr[0].data(); out.Lxx_rowval = rowval[0].data(); out.nnz_Lxx = (int64_t)rowval[0].size();
    out.gx_colptr = colptr[1].data(); out.gx_rowval = rowval[1].data(); out.nnz_gx = (int64_t)rowval[1].size();
    out.hx_colptr = colptr[2].data(); out.hx_rowval = rowval[2].data(); out.nnz_hx = (int64_t)rowval[2].size();
    if (with) {
        out.Lp_colptr = colptr[3].data(); out.Lp_rowval = rowval[3].data(); out.nnz_Lp = (int64_t)rowval[3].size();
        out.gp_colptr = colptr[4].data(); out.gp_rowval = rowval[4].data(); out.nnz_gp = (int64_t)rowval[4].size();
        out.hp_colptr = colptr[5].data(); out.hp_rowval = rowval[5].data(); out.nnz_hp = (int64_t)rowval[5].size();
    }
    RouteTable r;
    const int rc = sparse_route(sh, u, &out, r);
    printf("rc %d\n", rc);
    if (rc == 0) {
        for (int k = 0; k < nt; ++k) {
            const size_t n = (size_t)u.n[k];
            dump("vi", k, r.words, r.vi[k], nv[k] * n); dump("ri", k, r.words, r.ri[k], m[k] * n); dump("pi", k, r.words, r.pi[k], nth[k] * n);
            dump("ad", k, r.words, r.ad[k], nd[k] * n);
        }
        dump("g_addr", 0, r.words, r.g_addr, (size_t)u.G); dump("g_field", 0, r.words, r.g_field, (size_t)u.G);
        for (int c = 0; c < N_FILL; ++c) {                       // per category: offset length offset length ...
            printf("fill %d", c);
            for (int e = r.fill_first[c]; e < r.fill_first[c] + r.fill_count[c]; ++e) printf(" %d %d", r.words.at((size_t)(r.c_off + e)), r.words.at((size_t)(r.c_len + e)));
            printf("\n");
        }
    }
    printf("done\n");
    return 0;
}
