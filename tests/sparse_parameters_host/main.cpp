// The host side of the parameter Jacobians on the sparse handle (calipso.jl_amd/csrc/sparse_parameters.hpp) without a GPU (tests/test_sparse_parameters_host_cpu.py),
// under the address and undefined-behaviour sanitizers: the checks of the three stored patterns and of a column selection, the split into short and long columns and
// the launch geometry.  Output: one line per check ("ok" or the refusal's text), then the split and the geometry of a pattern with the column lengths
// 0, 1, 2, 63, 64, 65, 300, then "done".
#include <cstdio>
#include <string>
#include <vector>

#include "../../calipso.jl_amd/csrc/sparse_parameters.hpp"

using namespace calipso::sparse_parameters;

static void show(const std::string& s) { std::printf("%s\n", s.empty() ? "ok" : s.c_str()); }

// a CSC pattern (1-based) whose column j holds the rows 1 .. lengths[j]; the arrays are exactly as long as the pattern says
struct Csc {
    std::vector<int64_t> colptr, rowval;
    explicit Csc(const std::vector<int>& lengths) {
        colptr.push_back(1);
        for (int len : lengths) {
            for (int r = 1; r <= len; ++r) rowval.push_back(r);
            colptr.push_back(colptr.back() + len);
        }
    }
};

int main() {
    const char* entry = "set_parameter_patterns";
    const int64_t np = 7, rows[3] = {300, 5, 4};
    const Csc L({0, 1, 2, 63, 64, 65, 300}), g({0, 0, 5, 0, 0, 0, 0}), h({0, 0, 1, 0, 0, 0, 4});
    const Patterns good{{L.colptr.data(), g.colptr.data(), h.colptr.data()}, {L.rowval.data(), g.rowval.data(), h.rowval.data()}};
    show(check_patterns(entry, np, rows, good));                                                                            // 0
    show(check_patterns(entry, 0, rows, good));                                                                             // 1: no parameters
    { Patterns p = good; p.colptr[1] = nullptr; show(check_patterns(entry, np, rows, p)); }                                 // 2
    { Csc bad = g; bad.colptr[0] = 0; Patterns p = good; p.colptr[1] = bad.colptr.data(); show(check_patterns(entry, np, rows, p)); }      // 3: not 1-based
    { Csc bad = g; bad.colptr[4] = 1; Patterns p = good; p.colptr[1] = bad.colptr.data(); show(check_patterns(entry, np, rows, p)); }      // 4: a decrease
    { Csc bad = h; bad.colptr[3] = 9; Patterns p = good; p.colptr[2] = bad.colptr.data(); show(check_patterns(entry, np, rows, p)); }      // 5: past nnz + 1
    { Csc bad = L; std::swap(bad.rowval[1], bad.rowval[2]); Patterns p = good; p.rowval[0] = bad.rowval.data(); show(check_patterns(entry, np, rows, p)); }   // 6: unsorted rows
    { Csc bad = L; bad.rowval[2] = bad.rowval[1]; Patterns p = good; p.rowval[0] = bad.rowval.data(); show(check_patterns(entry, np, rows, p)); }              // 7: a duplicate
    { Csc bad = h; bad.rowval.back() = 5; Patterns p = good; p.rowval[2] = bad.rowval.data(); show(check_patterns(entry, np, rows, p)); }                      // 8: a row out of range
    { Csc bad = g; bad.rowval[0] = 0; Patterns p = good; p.rowval[1] = bad.rowval.data(); show(check_patterns(entry, np, rows, p)); }                          // 9: row 0
    { Patterns p = good; p.rowval[0] = nullptr; show(check_patterns(entry, np, rows, p)); }                                 // 10
    { const Csc e({0, 0, 0, 0, 0, 0, 0}); Patterns p = good; p.colptr[1] = e.colptr.data(); p.rowval[1] = nullptr; show(check_patterns(entry, np, rows, p)); }   // 11: an empty array, no rows: ok

    const char* fwd = "differentiate_parameters";
    const int64_t all[3] = {1, 7, 7}, zero[2] = {3, 0}, beyond[2] = {8, 1};
    show(check_selection(fwd, np, 3, all));                                                                                 // 12: a repeated and a last index
    show(check_selection(fwd, np, 7, nullptr));                                                                             // 13
    show(check_selection(fwd, np, 6, nullptr));                                                                             // 14: NULL with k != np
    show(check_selection(fwd, np, 2, zero));                                                                                // 15: index 0
    show(check_selection(fwd, np, 2, beyond));                                                                              // 16: index np + 1
    show(check_selection(fwd, np, 0, all));                                                                                 // 17
    show(check_selection(fwd, np, COLUMNS_MAX + 1, nullptr));                                                               // 18

    const Split s = split_columns(np, good);
    std::printf("split %d longest %lld long", SPLIT_LENGTH, (long long)s.longest);
    for (int32_t j : s.long_columns) std::printf(" %d", j);
    std::printf("\n");
    for (int64_t len : {0, 1, SPLIT_LENGTH - 1, SPLIT_LENGTH, SPLIT_LENGTH + 1}) std::printf("is_long %lld %d\n", (long long)len, is_long(len) ? 1 : 0);
    for (int64_t n : {1, 63, 64, 65, 1000}) {
        for (int64_t nl : {0, 3}) {
            const Geometry geo = geometry(n, nl);
            std::printf("geometry %lld %lld: long0 %lld items %lld blocks %u\n", (long long)n, (long long)nl, (long long)geo.long0, (long long)geo.items, geo.blocks);
        }
    }
    for (int64_t longest : {0, 1, 256, 257, 300}) std::printf("scatter %lld %u\n", (long long)longest, scatter_blocks(longest));
    for (int m = 0; m < 3; ++m) std::printf("name %s %d\n", array_name(m), array_by_name(array_name(m)));
    std::printf("name %d %d\n", array_by_name("lagrangian_hessian"), array_by_name(nullptr));
    std::printf("done\n");
    return 0;
}
