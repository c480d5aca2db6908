// sparse_differentiate.hpp — what the sparse handle shares between device and host: the per-row and per-cone arithmetic of the condensed solve's four maps — the ONLY
// copy: the map kernels of sparse_kkt.hip, which every Newton step's solve and every column of differentiate! go through, call these functions — and, for
// differentiate! (sparse_differentiate.hip), the workspace layout of a k-column pass and the argument checks of the entries.  No HIP include: the hipcc-only qualifiers sit
// behind CALIPSO_HD, so tests/sparse_differentiate_host/main.cpp builds the maps' dense matrices on the CPU under the sanitizers.
//
// The condensed solve of search_direction_symmetric! (search_direction.jl:25-104) is  step = M residual,  M = E K^-1 F + D:
//   F  residual_symmetric! (residual.jl:53-101)            rsym_x = r_x,  rsym_e = r_y + r_r / (rho + ep),  rsym_c = r_z + W (Cbar r_s + r_t)
//   E  the recovery's dependence on the symmetric solution  dx, dy, dz as they are,  Dr = dy / (rho + ep),  Ds = W Cbar dz,  Dt = -Cbar^-1 Ct Ds
//   D  ... and on the residual itself                       Dr = r_r / (rho + ep),  Ds = W (r_t + Cbar r_s),  Dt = Cbar^-1 (r_t - Ct Ds)
// with Ct = arrow(t), Cbar = arrow(s) - ed I, W = (Ct + Cbar ep)^-1 (for a nonnegative row the three are scalars).  Every block is symmetric and K is factored from
// one triangle, so the transposed map is  lambda = M' v = F' K^-1 E' v + D' v:
//   pre   g = E' v          g_x = v_x,  g_e = v_y + v_r / (rho + ep),  g_c = v_z + Cbar W a       with  p = Cbar^-1 v_t,  a = v_s - Ct p
//   post  F' h + D' v       l_x = h_x,  l_y = h_e,  l_z = h_c,  l_r = (h_e + v_r) / (rho + ep),  l_s = Cbar W (h_c + a),  l_t = W (h_c + a) + p
// A second-order cone of any dimension is one thread's: O(dimension) through the closed-form arrow inverse, its temporaries in the caller's output entries.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#define CALIPSO_HD __host__ __device__ __forceinline__
#else
#define CALIPSO_HD inline
#endif

namespace calipso {
namespace sparse_kkt {

// second_order_matrix_inverse's vector form (cones/second_order.jl:50-65) for u = first row of Cs + Cbar_t P, on the fly: U(k), X(k) give the entries, put(k, value)
// takes entry k of the UNSCALED result times 1 / u[0] in the reference's order
template <typename FU, typename FX, typename FP>
CALIPSO_HD void arrow_inverse(int dm, FU U, FX X, FP put) {
    const double u0 = U(0);
    double uu = 0.0, d0 = 0.0;
    for (int k = 1; k < dm; ++k) { const double uk = U(k); uu += uk * uk; d0 += (uk / u0) * X(k); }
    const double alpha = -1.0 / (u0 * u0) * uu;
    const double beta = 1.0 / (1.0 + alpha);
    const double x0_1 = X(0) - d0;
    double d1 = 0.0;
    for (int k = 1; k < dm; ++k) { const double us = U(k) / u0; const double o = X(k) - beta * (us * x0_1); d1 += us * o; put(k, 1.0 / u0 * o); }
    put(0, 1.0 / u0 * (X(0) - d1));
}

}  // namespace sparse_kkt

namespace sparse_differentiate {

using sparse_kkt::arrow_inverse;

// what the maps read besides the slacks: the regularisation of the last assemble and the penalty
struct MapScalars { double ep, ed, rho; };

// ---- equality rows ---------------------------------------------------------------------------------------------------------------------------------------------
CALIPSO_HD double equality_forward_pre(const MapScalars& c, double r_r, double r_y) { return r_y + r_r / (c.rho + c.ep); }                       // residual.jl:62-66
CALIPSO_HD double equality_forward_post(const MapScalars& c, double dy, double r_r) { return (r_r + dy) / (c.rho + c.ep); }                      // Dr  search_direction.jl:62-66
CALIPSO_HD double equality_transposed_pre(const MapScalars& c, double v_r, double v_y) { return v_y + v_r / (c.rho + c.ep); }
CALIPSO_HD double equality_transposed_post(const MapScalars& c, double h_e, double v_r) { return (h_e + v_r) / (c.rho + c.ep); }                  // l_r

// ---- nonnegative rows (s, t: the slack and its dual) -------------------------------------------------------------------------------------------------------------
CALIPSO_HD double nonnegative_forward_pre(const MapScalars& c, double s, double t, double r_s, double r_z, double r_t) {
    const double Sb = s - c.ed;
    return r_z + (r_t + Sb * r_s) / (t + Sb * c.ep);
}
CALIPSO_HD void nonnegative_forward_post(const MapScalars& c, double s, double t, double dz, double r_s, double r_t, double* Ds, double* Dt) {
    const double Sb = s - c.ed;
    const double ds = (r_t + Sb * (r_s + dz)) / (t + Sb * c.ep);
    *Ds = ds;
    *Dt = (r_t - t * ds) / Sb;
}
CALIPSO_HD double nonnegative_transposed_pre(const MapScalars& c, double s, double t, double v_s, double v_z, double v_t) {
    const double Sb = s - c.ed;
    const double p = v_t / Sb, a = v_s - t * p;
    return v_z + Sb * a / (t + Sb * c.ep);
}
CALIPSO_HD void nonnegative_transposed_post(const MapScalars& c, double s, double t, double h, double v_s, double v_t, double* l_s, double* l_t) {
    const double Sb = s - c.ed;
    const double p = v_t / Sb, a = v_s - t * p;
    const double y = (h + a) / (t + Sb * c.ep);
    *l_s = Sb * y;
    *l_t = y + p;
}

// ---- second-order cones: s, t and every vector are the cone's dm entries ---------------------------------------------------------------------------------------
// rsym = r_z + W (Cbar r_s + r_t)
CALIPSO_HD void soc_forward_pre(const MapScalars& c, int dm, const double* s, const double* t, const double* r_s, const double* r_z, const double* r_t, double* out) {
    const double S0 = s[0] - c.ed, ep = c.ep;
    double v0 = 0.0;
    for (int b = 0; b < dm; ++b) v0 += (b == 0 ? S0 : s[b]) * r_s[b];
    v0 += r_t[0];
    arrow_inverse(dm,
                  [&](int b) { return t[b] + (b == 0 ? S0 : s[b]) * ep; },
                  [&](int a) { return a == 0 ? v0 : (s[a] * r_s[0] + S0 * r_s[a]) + r_t[a]; },
                  [&](int a, double v) { out[a] = r_z[a] + v; });
}
// Ds = W (r_t + Cbar (r_s + dz)),  Dt = Cbar^-1 (r_t - Ct Ds)      (Ds is read back)
CALIPSO_HD void soc_forward_post(const MapScalars& c, int dm, const double* s, const double* t, const double* dz, const double* r_s, const double* r_t, double* Ds, double* Dt) {
    const double S0 = s[0] - c.ed, ep = c.ep;
    double v0 = 0.0;
    for (int b = 0; b < dm; ++b) v0 += (b == 0 ? S0 : s[b]) * (r_s[b] + dz[b]);
    v0 = r_t[0] + v0;
    arrow_inverse(dm,
                  [&](int b) { return t[b] + (b == 0 ? S0 : s[b]) * ep; },
                  [&](int a) { return a == 0 ? v0 : r_t[a] + (s[a] * (r_s[0] + dz[0]) + S0 * (r_s[a] + dz[a])); },
                  [&](int a, double v) { Ds[a] = v; });
    double c0 = 0.0;
    for (int b = 0; b < dm; ++b) c0 += t[b] * Ds[b];
    c0 = r_t[0] - c0;
    arrow_inverse(dm,
                  [&](int b) { return b == 0 ? S0 : s[b]; },
                  [&](int a) { return a == 0 ? c0 : r_t[a] - (t[a] * Ds[0] + t[0] * Ds[a]); },
                  [&](int a, double v) { Dt[a] = v; });
}
// p = Cbar^-1 v_t into `p`, then y = W (h + v_s - Ct p) into `y` (h may be NULL: zero).  p and y: dm entries each, distinct from every input
CALIPSO_HD void soc_transposed_core(const MapScalars& c, int dm, const double* s, const double* t, const double* h, const double* v_s, const double* v_t, double* p, double* y) {
    const double S0 = s[0] - c.ed, ep = c.ep;
    arrow_inverse(dm,
                  [&](int b) { return b == 0 ? S0 : s[b]; },
                  [&](int a) { return v_t[a]; },
                  [&](int a, double v) { p[a] = v; });
    double a0 = 0.0;
    for (int b = 0; b < dm; ++b) a0 += t[b] * p[b];
    a0 = (h ? h[0] : 0.0) + (v_s[0] - a0);
    arrow_inverse(dm,
                  [&](int b) { return t[b] + (b == 0 ? S0 : s[b]) * ep; },
                  [&](int a) { return a == 0 ? a0 : (h ? h[a] : 0.0) + (v_s[a] - (t[a] * p[0] + t[0] * p[a])); },
                  [&](int a, double v) { y[a] = v; });
}
// g = v_z + Cbar W a;  p, y: scratch (the kernels pass the cone's entries of l_t and l_s, which the post map writes later)
CALIPSO_HD void soc_transposed_pre(const MapScalars& c, int dm, const double* s, const double* t, const double* v_s, const double* v_z, const double* v_t, double* g, double* p, double* y) {
    soc_transposed_core(c, dm, s, t, nullptr, v_s, v_t, p, y);
    const double S0 = s[0] - c.ed;
    double g0 = 0.0;
    for (int b = 0; b < dm; ++b) g0 += (b == 0 ? S0 : s[b]) * y[b];
    g[0] = v_z[0] + g0;
    for (int a = 1; a < dm; ++a) g[a] = v_z[a] + (s[a] * y[0] + S0 * y[a]);
}
// l_s = Cbar W (h + a),  l_t = W (h + a) + p;  both outputs serve as the scratch of the core first
CALIPSO_HD void soc_transposed_post(const MapScalars& c, int dm, const double* s, const double* t, const double* h, const double* v_s, const double* v_t, double* l_s, double* l_t) {
    soc_transposed_core(c, dm, s, t, h, v_s, v_t, l_t, l_s);
    const double S0 = s[0] - c.ed;
    double l0 = 0.0;
    for (int b = 0; b < dm; ++b) { l0 += (b == 0 ? S0 : s[b]) * l_s[b]; l_t[b] = l_s[b] + l_t[b]; }
    const double y0 = l_s[0];
    for (int a = 1; a < dm; ++a) l_s[a] = s[a] * y0 + S0 * l_s[a];
    l_s[0] = l0;
}

// ---- the workspace of a k-column pass: doubles first, then the column masks of the correction rounds ---------------------------------------------------------------
struct Region { size_t off = 0, len = 0; };
struct Layout {
    Region V, X, rsym, dsym, E, C, Xsave, norms;      // V: the caller's columns (N x k), X: the map's (N x k), rsym / dsym: n x k; E, C, Xsave, norms: the rounds'
    size_t doubles = 0, ints = 0;                     // ints: active (k), restore (k)
};
inline Layout layout(size_t N, size_t n, size_t k, bool rounds) {
    Layout l;
    size_t at = 0;
    const auto take = [&](Region& r, size_t len) { r.off = at; r.len = len; at += len; };
    take(l.V, N * k); take(l.X, N * k); take(l.rsym, n * k); take(l.dsym, n * k);
    if (rounds) { take(l.E, N * k); take(l.C, N * k); take(l.Xsave, N * k); take(l.norms, k); }
    l.doubles = at; l.ints = rounds ? 2 * k : 0;
    return l;
}

// ---- argument checks: an empty string, or the refusal's text (the entry returns CALIPSO_ERR_ARGUMENT with it) ---------------------------------------------------
constexpr int64_t COLUMNS_MAX = 65535;      // the multi-column solve's grid limit (blockIdx.y carries the column)
inline std::string check_columns(const char* entry, int64_t k) {
    if (k < 1) return std::string(entry) + ": k: at least one column, not " + std::to_string(k);
    if (k > COLUMNS_MAX) return std::string(entry) + ": k: at most " + std::to_string(COLUMNS_MAX) + " columns in one call (the multi-column solve's grid limit), not " + std::to_string(k);
    return "";
}
inline std::string check_array(const char* entry, const char* name, const void* p) {
    if (!p) return std::string(entry) + ": " + name + " is NULL";
    return "";
}
// grad: data gradients need the QP's vectors and a point to evaluate the closed forms at
inline std::string check_gradients(const char* entry, bool wanted, bool qp_attached, bool point_resident) {
    if (!wanted) return "";
    if (!qp_attached) return std::string(entry) + ": grad: no QP attached (calipso_hip_sparse_kkt_qp_attach first)";
    if (!point_resident) return std::string(entry) + ": grad: no point resident (calipso_hip_sparse_kkt_initialize, or set_values with w, first)";
    return "";
}
inline bool refinement_option(double value) { return value == 0.0 || value == 1.0; }

}  // namespace sparse_differentiate
}  // namespace calipso
