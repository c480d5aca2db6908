// ordering.hip — the ordering / symbolic service of the LinearSolver seam: integer work on the host, as in the reference.
//
// The reference factors  P K P' = L D L'  with P = amd(K) from the third-party AMD.jl (qdldl.jl:135), builds the permuted upper-triangular
// matrix and the entry map AtoPAPt (permute_symmetric, qdldl.jl:642-742), the elimination tree and the column counts of L
// (QDLDL_etree!, qdldl.jl:358-395).  Here:
//   calipso_hip_ordering         an elimination order for a sparse symmetric pattern: reverse Cuthill-McKee (minimises the bandwidth — what the
//                                device LDL^T of ldl.hip exploits: everything outside the band is skipped) or minimum degree on the quotient
//                                graph (the fill-reducing order class of AMD; AMD.jl's exact permutation is not reproducible and no reference
//                                test pins it).
//   calipso_hip_symbolic         P A P' (upper triangle, CSC, entries in the reference's placement order), AtoPAPt, etree, column counts — integer
//                                results, bit-exact against the oracle's restatement for the same permutation (tests/test_oracle_qdldl.py,
//                                tests/test_abi_cpu.py::test_symbolic_matches_the_oracle).  Pure host functions: no device needed.
//   calipso_hip_ldl_analyze_csc  chooses / installs the order of a calipso_hip_ldl_* handle; the following factorisations scatter P K P' and, when the
//                                permuted matrix is banded, run the band-limited device factorisation and triangular solves.
// All indices 1-based Int64 (Julia's), as everywhere in this ABI.
#include <algorithm>
#include <vector>

#include "internal.hpp"
#include "ordering.hpp"      // the graph routines: plain host C++

using calipso::i64;
using namespace calipso::ordering;

namespace calipso {
// nested dissection with its pieces (leaf pieces <= 48 vertices and separators, each contiguous in the order): the supernodes of the multifrontal
// factorisation of sparse.hip.  perm: 1-based, n entries; pieces: (first position 0-based, count)
int nested_dissection_pieces(i64 n, const i64* colptr, const i64* rowval, i64* perm, std::vector<std::pair<int, int>>& pieces) {
    if (n < 0 || !colptr || !perm || (!rowval && colptr[n] > 1)) return CALIPSO_ERR_ARGUMENT;
    pieces.clear();
    const std::vector<i64> p = nested_dissection(adjacency(n, colptr, rowval), &pieces);
    std::copy(p.begin(), p.end(), perm);
    return CALIPSO_OK;
}
// one gate for every entry point that walks a caller's CSC pattern: colptr[0] == 1, non-decreasing, fewer than 2^31 entries, 1 <= rowval <= n
bool csc_pattern_ok(i64 n, const i64* colptr, const i64* rowval) { return ordering::csc_pattern_ok(n, colptr, rowval); }
}  // namespace calipso

extern "C" {

// method 0: natural (1..n), 1: reverse Cuthill-McKee, 2: minimum degree, 4: nested dissection (3 is "the caller's order" in the analyse calls).  Pattern: CSC, 1-based, any triangle(s).  perm[k] = the vertex eliminated k-th.
int32_t calipso_hip_ordering(int64_t n, const int64_t* colptr, const int64_t* rowval, int32_t method, int64_t* perm) {
    if (n < 0 || !colptr || !perm || method < 0 || method > 4 || method == 3 || !calipso::csc_pattern_ok(n, colptr, rowval)) return CALIPSO_ERR_ARGUMENT;
    if (method == 0) { for (i64 k = 0; k < n; ++k) perm[k] = k + 1; return CALIPSO_OK; }
    const auto adj = adjacency(n, colptr, rowval);
    const std::vector<i64> p = method == 1 ? rcm(adj) : method == 2 ? minimum_degree(adj) : nested_dissection(adj);
    std::copy(p.begin(), p.end(), perm);
    return CALIPSO_OK;
}

// Symbolic phase for the upper triangle of A under `perm` (NULL = natural): Pp[n+1], Pi[nnz(triu A)], AtoPAPt[nnz A] (0 for entries below the
// diagonal), etree[n] (-1 = root), Lnz[n]; any output may be NULL.  Returns sum(Lnz) = nnz(L), -1 in QDLDL_etree!'s failure cases, or a negative
// status < -1.  info (may be NULL): [0] half bandwidth of P A P', [1] nnz(triu A).
int64_t calipso_hip_symbolic(int64_t n, const int64_t* colptr, const int64_t* rowval, const int64_t* perm, int64_t* Pp, int64_t* Pi, int64_t* AtoPAPt,
                             int64_t* etree, int64_t* Lnz, int64_t info[2]) {
    if (n < 1 || !calipso::csc_pattern_ok(n, colptr, rowval)) return CALIPSO_ERR_ARGUMENT;
    std::vector<i64> iperm((size_t)n);
    if (perm) { if (!is_permutation(n, perm)) return CALIPSO_ERR_ARGUMENT; for (i64 k = 0; k < n; ++k) iperm[(size_t)perm[k] - 1] = k + 1; }   // invperm (qdldl.jl:143)
    else for (i64 k = 0; k < n; ++k) iperm[(size_t)k] = k + 1;
    std::vector<i64> pp, pi, map, parent, lnz;
    permute_upper(n, colptr, rowval, iperm.data(), pp, pi, map);
    const i64 total = etree_counts(n, pp, pi, parent, lnz);
    i64 hb = 0;
    for (i64 j = 0; j < n; ++j) for (i64 p = pp[(size_t)j] - 1; p < pp[(size_t)j + 1] - 1; ++p) hb = std::max(hb, j + 1 - pi[(size_t)p]);
    if (Pp) std::copy(pp.begin(), pp.end(), Pp);
    if (Pi) std::copy(pi.begin(), pi.end(), Pi);
    if (AtoPAPt) std::copy(map.begin(), map.end(), AtoPAPt);
    if (etree) for (i64 k = 0; k < n; ++k) etree[k] = parent[(size_t)k] < 0 ? -1 : parent[(size_t)k] + 1;
    if (Lnz) std::copy(lnz.begin(), lnz.end(), Lnz);
    if (info) { info[0] = hb; info[1] = (i64)pi.size(); }
    return total;
}

}  // extern "C"
