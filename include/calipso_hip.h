/*
 * calipso_hip.h — C ABI of libcalipso_hip.so: the MI355X (gfx950) implementation of CALIPSO's
 * per-iteration Newton/KKT hot path.
 *
 * The reference (thowell/CALIPSO.jl v0.1.1) is pure Julia and has no FFI; the seams this ABI replaces are
 * Julia functions and types (paths relative to src/solver/ of the reference):
 *   - exported API            Solver / initialize! / solve!            CALIPSO.jl:48-50, solver.jl:46-173,
 *                                                                      initialize.jl:9-13, solve.jl:8-377
 *   - linear-solver seam      LDLSolver, factorize!, compute_inertia!, linear_solve!   linear_solver.jl:1-60
 *   - per-function seams      cone!, residual!, residual_jacobian_variables(_symmetric)!, residual_symmetric!,
 *                             search_direction(_symmetric)!, iterative_refinement!, inertia_correction!,
 *                             cone_violation, merit, merit_gradient!, constraint_violation!, optimality_error,
 *                             differentiate!      (one entry point each, cited below)
 * INTEGRATION.md shows the Julia `ccall` binding for every entry point.
 *
 * Conventions
 *   - plain C: pointers + sizes, no C++/torch types; every function returns an int32 status.
 *   - all floating point is IEEE fp64; all indices are Int64 and 1-BASED (Julia's), matrices column-major.
 *   - the caller owns every host buffer; the opaque handle owns device memory, one HIP stream and its events (and, created on first use, a second
 *     stream that only ever carries the finish of a factorisation beside its pivot chain and is joined into the first before the call that
 *     queued it returns: everything a caller orders or synchronises against is the first stream).
 *   - one handle = one problem shape (nx, np, ne, nc + cone layout); a handle is used by one host thread at a time;
 *     distinct handles are independent (as distinct `Solver`s are in the reference).
 *   - host arrays are named by the reference's own field names ("equality_jacobian_variables", "solution", ...).
 *   - nothing here falls back to the CPU: without a usable HIP device every call fails with CALIPSO_ERR_HIP.
 */
#ifndef CALIPSO_HIP_H
#define CALIPSO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct calipso_hip_solver calipso_hip_solver;

/* status codes: negative = the reference's error() cases, positive = its @warn cases */
enum {
    CALIPSO_OK = 0,
    CALIPSO_ERR_INERTIA = -1,      /* error("inertia correction failure")  inertia.jl:72 */
    CALIPSO_ERR_CONE_SEARCH = -2,  /* error("cone search failure")         solve.jl:210,220 */
    CALIPSO_ERR_CALLBACK = -3,     /* the evaluation callback returned non-zero */
    CALIPSO_ERR_ARGUMENT = -4,     /* unknown field name, wrong length, null pointer */
    CALIPSO_ERR_HIP = -5,          /* HIP runtime error / no device; text in calipso_hip_last_error */
    CALIPSO_ERR_LAYOUT = -6,       /* cone index sets violate the layout the reference relies on (cones/cone.jl:27-59 vs residual.jl:46-48) */
    CALIPSO_WARN_ZERO_PIVOT = 1,   /* @warn "Zero entry in D (matrix is not quasidefinite)" qdldl.jl:309-311 */
    CALIPSO_WARN_REFINEMENT = 2,   /* @warn "iterative refinement failure" iterative_refinement.jl:50 */
    CALIPSO_WARN_LINE_SEARCH = 3   /* @warn "residual line search failure" solve.jl:301 */
};

/* evaluate! keyword flags (evaluate.jl:1-23), one bit each */
enum {
    CALIPSO_EVAL_OBJECTIVE = 1u << 0,
    CALIPSO_EVAL_OBJECTIVE_GRADIENT = 1u << 1,
    CALIPSO_EVAL_OBJECTIVE_HESSIAN = 1u << 2,
    CALIPSO_EVAL_EQUALITY = 1u << 3,
    CALIPSO_EVAL_EQUALITY_JACOBIAN = 1u << 4,
    CALIPSO_EVAL_EQUALITY_DUAL_GRADIENT = 1u << 5,
    CALIPSO_EVAL_EQUALITY_DUAL_HESSIAN = 1u << 6,
    CALIPSO_EVAL_CONE = 1u << 7,
    CALIPSO_EVAL_CONE_JACOBIAN = 1u << 8,
    CALIPSO_EVAL_CONE_DUAL_GRADIENT = 1u << 9,
    CALIPSO_EVAL_CONE_DUAL_HESSIAN = 1u << 10,
    CALIPSO_EVAL_OBJECTIVE_JACOBIAN_PARAMETERS = 1u << 11,
    CALIPSO_EVAL_EQUALITY_JACOBIAN_PARAMETERS = 1u << 12,
    CALIPSO_EVAL_EQUALITY_DUAL_JACOBIAN_PARAMETERS = 1u << 13,
    CALIPSO_EVAL_CONE_JACOBIAN_PARAMETERS = 1u << 14,
    CALIPSO_EVAL_CONE_DUAL_JACOBIAN_PARAMETERS = 1u << 15
};

/* cone! keyword flags (cones/cone.jl:71-77) */
enum {
    CALIPSO_CONE_BARRIER = 1 << 0,
    CALIPSO_CONE_BARRIER_GRADIENT = 1 << 1,
    CALIPSO_CONE_PRODUCT = 1 << 2,
    CALIPSO_CONE_JACOBIAN = 1 << 3, /* arrow/diagonal Jacobians are implicit in (s, t) on the device; kept for API parity */
    CALIPSO_CONE_TARGET = 1 << 4
};

/* User-evaluation callback: the stand-in for the generated functions evaluate! calls (evaluate.jl:37-121).
 * Called on the host with the point's x, y, z and the parameters; it must evaluate the flagged quantities and hand
 * them to the handle with calipso_hip_set_field (the three Hessian terms as ONE summed "lagrangian_hessian").
 * Return 0 on success. */
typedef int32_t (*calipso_eval_fn)(void* user, uint32_t flags, const double* x, const double* y, const double* z,
                                   const double* theta);

/* DEVICE-side user evaluation: the same contract as calipso_eval_fn, but every pointer is a DEVICE pointer into the
 * handle's own memory and the function only ENQUEUES work (HIP kernels, hipMemcpyAsync, hipBLAS ...) on the given stream — it must not
 * synchronise.  x, y, z point into the current / candidate point, theta to the parameters; `out` names where each flagged ProblemData
 * field has to be written (fields that do not exist for the shape are NULL).  With such an evaluator a whole solve! — including the
 * up to 25 backtracking re-evaluations of the residual line search, solve.jl:254-302 — runs without the point ever visiting the host
 * and without a block upload.  Return 0 on success. */
typedef struct calipso_device_problem_data {
    double* objective;                        /* [1] */
    double* objective_gradient_variables;     /* [nx] */
    double* equality_constraint;              /* [ne] */
    double* cone_constraint;                  /* [nc] */
    double* equality_dual_jacobian_variables; /* [nx]  (g'y)_x */
    double* cone_dual_jacobian_variables;     /* [nx]  (h'z)_x */
    double* lagrangian_hessian;               /* [nx*nx] column-major: objective Hessian + (g'y)_xx + (h'z)_xx summed (the latter two iff
                                                 options.constraint_tensor, residual_jacobian_variables.jl:10-16) */
    double* equality_jacobian_variables;      /* ne x nx column-major with leading dimension jacobian_ld */
    double* cone_jacobian_variables;          /* nc x nx column-major with leading dimension jacobian_ld */
    int64_t jacobian_ld;                      /* = ne + nc: the two Jacobians are stacked in one matrix on the device */
    double* lagrangian_gradient_parameters;   /* [nx*np] objective + equality-dual + cone-dual terms summed (residual_jacobian_parameters.jl:8-14) */
    double* equality_jacobian_parameters;     /* [ne*np] */
    double* cone_jacobian_parameters;         /* [nc*np] */
    int64_t nx, np, ne, nc;
} calipso_device_problem_data;
typedef int32_t (*calipso_device_eval_fn)(void* user, uint32_t flags, const double* x, const double* y, const double* z, const double* theta,
                                          const calipso_device_problem_data* out, void* hip_stream);

/* The same for a STRUCTURED handle (calipso_hip_create_structured), without the dense interchange arrays: the generated functions of evaluate! (evaluate.jl:37-121)
 * write the non-zeros of the Jacobians and of the Hessian where the sparsity lists say (methods.*_sparsity, src/trajectory_optimization/sparsity.jl:28-129) — here
 * straight into the handle's packed blocks.  A block = rows [row0, row0 + nrows) x columns [col0, col0 + ncols) (0-based; rows numbered in the stacked matrix
 * [equality; cone]: cone row k is row ne + k), values column-major with leading dimension ld, a DEVICE pointer into the handle's own storage.  Hessian blocks are the
 * diagonal blocks of the Lagrangian Hessian (row0 = col0, nrows = ncols).  The descriptor arrays exist twice: on the host (`*_blocks`) and on the device
 * (`*_blocks_device`, for kernels that walk them).  An evaluator asked for a Jacobian / the Hessian writes EVERY entry of every block of it (zeros included);
 * nothing outside the blocks exists, so nothing can be written there.  The vector fields are those of calipso_device_problem_data.  With such an evaluator a
 * structured handle never allocates the nx^2 + (ne + nc) nx doubles of dense scratch that calipso_device_eval_fn costs it. */
typedef struct calipso_device_block { int64_t row0, nrows, col0, ncols; double* values; int64_t ld; } calipso_device_block;
typedef struct calipso_device_block_data {
    double* objective; double* objective_gradient_variables; double* equality_constraint; double* cone_constraint;
    double* equality_dual_jacobian_variables; double* cone_dual_jacobian_variables;
    double* lagrangian_gradient_parameters; double* equality_jacobian_parameters; double* cone_jacobian_parameters;
    int64_t nx, np, ne, nc;
    int64_t n_jacobian_blocks; const calipso_device_block* jacobian_blocks; const calipso_device_block* jacobian_blocks_device;
    int64_t n_hessian_blocks; const calipso_device_block* hessian_blocks; const calipso_device_block* hessian_blocks_device;
} calipso_device_block_data;
typedef int32_t (*calipso_device_block_eval_fn)(void* user, uint32_t flags, const double* x, const double* y, const double* z, const double* theta,
                                                const calipso_device_block_data* out, void* hip_stream);

/* The same for a SPARSE handle (calipso_hip_sparse_kkt_set_evaluator): the three matrices are the handle's own resident non-zero arrays on the patterns given to
 * calipso_hip_sparse_kkt_create, in the caller's non-zero order — the next assemble reads what the evaluator wrote, nothing is copied.  An evaluator asked for a
 * Jacobian / the Hessian writes EVERY stored non-zero of it (zeros included).  lagrangian_hessian holds both triangles and receives the sum of the terms whose bits are
 * set: fxx (OBJECTIVE_HESSIAN) + (y'g)xx (EQUALITY_DUAL_HESSIAN) + (z'h)xx (CONE_DUAL_HESSIAN).  (g'y)x and (h'z)x are never asked for: the handle forms them from its
 * column views on the fresh Jacobian values.  The six pattern arrays are HOST copies (1-based, as given to create), for an evaluator that builds its own address table
 * on the first call.  The evaluator enqueues on hip_stream and returns without waiting; 0, or a code the handle reports.
 * The parameter Jacobians: without calipso_hip_sparse_kkt_set_parameter_patterns the last fields are NULL / 0 and no parameter-Jacobian bit is ever set.  With it the
 * three parameter arrays are the handle's resident values on the three stored CSC patterns with np columns (HOST copies of the patterns, 1-based, as given), and the
 * evaluator may be called with the five parameter bits: it writes EVERY stored non-zero of an array it is asked for; lagrangian_gradient_parameters receives the sum
 * of the terms whose bits are set: f_x,theta (OBJECTIVE_JACOBIAN_PARAMETERS) + (y'g)_x,theta (EQUALITY_DUAL_...) + (z'h)_x,theta (CONE_DUAL_...)
 * (residual_jacobian_parameters.jl:8-14). */
typedef struct calipso_device_sparse_data {
    double* objective;                       /* [1]  */
    double* objective_gradient_variables;    /* [nx] */
    double* equality_constraint;             /* [ne] */
    double* cone_constraint;                 /* [nc] */
    double* lagrangian_hessian;              /* nzval on the handle's Lxx pattern (both triangles): fxx + (y'g)xx + (z'h)xx, the terms whose bits are set */
    double* equality_jacobian_variables;     /* nzval on the gx pattern */
    double* cone_jacobian_variables;         /* nzval on the hx pattern */
    const int64_t *Lxx_colptr, *Lxx_rowval, *gx_colptr, *gx_rowval, *hx_colptr, *hx_rowval;   /* HOST copies, 1-based, as given to create */
    int64_t nx, np, ne, nc, nnz_Lxx, nnz_gx, nnz_hx;
    double* lagrangian_gradient_parameters;  /* nzval on the Lp pattern (nx rows, np columns); NULL without parameter patterns, as everything below */
    double* equality_jacobian_parameters;    /* nzval on the gp pattern (ne rows) */
    double* cone_jacobian_parameters;        /* nzval on the hp pattern (nc rows) */
    const int64_t *Lp_colptr, *Lp_rowval, *gp_colptr, *gp_rowval, *hp_colptr, *hp_rowval;     /* HOST copies, 1-based, as given to set_parameter_patterns */
    int64_t nnz_Lp, nnz_gp, nnz_hp;
} calipso_device_sparse_data;
typedef int32_t (*calipso_device_sparse_eval_fn)(void* user, uint32_t flags, const double* x, const double* y, const double* z, const double* theta,
                                                 const calipso_device_sparse_data* out, void* hip_stream);

/* callback_inner(custom, solver) / callback_outer(custom, solver)  (solver.jl:183,193; called at solve.jl:350,371) */
typedef void (*calipso_callback_fn)(void* user, calipso_hip_solver* solver);

/* ---- life cycle ------------------------------------------------------------------------------------------------ */
/* Solver(methods, nx, np, ne, nc; nonnegative_indices, second_order_indices)   solver.jl:46-150, indices.jl:20-63.
 * nonneg_idx: n_nonneg cone-local indices (1-based); soc_ptr: n_soc+1 zero-based offsets into soc_idx (1-based,
 * first entry of each cone is its head).  The sets must be [1..q] followed by contiguous SOC blocks in order
 * (the only layout for which the reference is self-consistent), else CALIPSO_ERR_LAYOUT.
 * LIMIT: a second-order cone may have at most 1024 entries (csrc/soc_wide.hip: one wavefront per cone, up to sixteen entries per lane; the reference has none,
 * cones/second_order.jl:1-69 — its largest is 12): wider cones are refused with CALIPSO_ERR_ARGUMENT and a message in calipso_hip_last_error(NULL). */
int32_t calipso_hip_create(int64_t nx, int64_t np, int64_t ne, int64_t nc, int64_t n_nonneg, const int64_t* nonneg_idx,
                           int64_t n_soc, const int64_t* soc_ptr, const int64_t* soc_idx, int32_t device,
                           calipso_hip_solver** out);
/* Solver(...) for a stage-structured problem whose sparsity is known up front — as the reference's are (methods.*_sparsity, src/trajectory_optimization/
 * sparsity.jl:28-129): constraint row k of [equality; cone] touches columns row_first[k]..row_last[k] (1-based, inclusive; first > last: an empty row; the
 * rows of a second-order cone share the union of their ranges), the Lagrangian Hessian is block diagonal with blocks starting at hessian_block_start[0] = 1 <
 * hessian_block_start[1] < ... .  The handle holds ONLY the blocks (packed contiguously, both orientations), the tiles of the Schur complement that the
 * blocks couple, and the multifrontal factor of the Schur complement: O(stages x block^2) device memory — none of the dense nx^2 / (ne + nc) nx / NP^2 buffers of
 * calipso_hip_create exist.  Uploads: calipso_hip_set_field with the dense host arrays of ProblemData (packed on the host; a non-zero outside the declared
 * structure is an error), calipso_hip_set_sparsity + calipso_hip_scatter_field / _hessian (straight into the blocks), calipso_hip_qp_attach.  Everything
 * else of this header works as on a dense handle — calipso_hip_differentiate included (differentiate.jl:1-61: the products with [gx; hx] block by block for all
 * parameter columns at once, the solves through the fronts for all columns together) and device evaluators (they write the dense ProblemData layout: on such a
 * handle into dense scratch arrays — nx^2 + (ne + nc) nx doubles, allocated on the first evaluation — whose entries go into the blocks behind the evaluator; a
 * non-zero outside the declared structure is an error) — except: no calipso_hip_analyze_structure / clear_structure / set_stage_parallel(off) /
 * set_stage_blocks(off) (the structure is fixed); members of a group must share one structure.  The Hessian must have at least two diagonal blocks (dynamics whose y'f Hessian couples x_t with
 * x_{t+1}, e.g. implicit integrators, declare one block and are refused: use calipso_hip_create + calipso_hip_analyze_structure for those). */
int32_t calipso_hip_create_structured(int64_t nx, int64_t np, int64_t ne, int64_t nc, int64_t n_nonneg, const int64_t* nonneg_idx, int64_t n_soc,
                                      const int64_t* soc_ptr, const int64_t* soc_idx, int32_t device, const int64_t* row_first, const int64_t* row_last,
                                      int64_t n_hessian_blocks, const int64_t* hessian_block_start, calipso_hip_solver** out);
int32_t calipso_hip_destroy(calipso_hip_solver*);
const char* calipso_hip_last_error(calipso_hip_solver*); /* never NULL */
const char* calipso_hip_version(void);
int32_t calipso_hip_device_count(void);

/* ---- data movement (host <-> handle), by the reference's field names ----------------------------------------- */
/* ProblemData (problem_data.jl:2-31): "objective"[1] "objective_gradient_variables"[nx] "equality_constraint"[ne]
 *   "equality_jacobian_variables"[ne*nx] "equality_dual_jacobian_variables"[nx] "cone_constraint"[nc]
 *   "cone_jacobian_variables"[nc*nx] "cone_dual_jacobian_variables"[nx] "lagrangian_hessian"[nx*nx]
 *   ( = objective_jacobian_variables_variables + equality_dual_..._variables + cone_dual_..._variables,
 *     residual_jacobian_variables.jl:10-16 )  "cone_product"[nc] "cone_target"[nc] "barrier"[1] "barrier_gradient"[nc]
 *   "jacobian_parameters"[N*np] ( = dR/dtheta, residual_jacobian_parameters.jl:1-40 )
 * Points / SolverData (point.jl, solver_data.jl): "solution"[N] "candidate"[N] "residual"[N] "residual_error"[N]
 *   "step"[N] "step_correction"[N] "residual_symmetric"[n] "step_symmetric"[n] "merit_gradient"[n]
 *   "jacobian_variables_symmetric"[n*n] (dense K, after calipso_hip_residual_jacobian_variables_symmetric)
 *   "solution_sensitivity"[N*np] "parameters"[np] "dual"[ne]
 * Scalars (solver.jl:81-127): "central_path" "fraction_to_boundary" "penalty" "primal_regularization"
 *   "primal_regularization_last" "dual_regularization";  options (options.jl:6-59): "opt.<field>" (as double).  One option has no counterpart in
 *   the reference: "opt.solve_block" (512, 1024 or 2048, default 1024) — the widest diagonal block of the factor of S whose inverse is assembled for the
 *   triangular solves.  It changes the summation order of the solves (not the factor): 1024 suits one system (fewer dependent launches), 512 suits
 *   a group (one merge level less; its solves are bandwidth-bound); 2048 is there for larger systems (at nx = 2432 its extra merge level costs 0.15 ms
 *   and saves 0.07).  Set it on every member of a group (the first member's value governs the group's launches).  And "opt.solve_wform" (0 or 1,
 *   default 1): the solves (linear_solve!, linear_solver.jl:52-60) multiply with the stacked blocks [Tinv_b; W_b], W_b = L[below, b] Tinv_b formed once per
 *   factorisation, so that a solve is two dependent launches per solve block instead of four — and ONE for the last block, which has nothing below it and goes
 *   through the symmetric inverse Tinv' D^-1 Tinv of its Schur complement; same factor, different summation order.  One system wants it; a group
 *   (bandwidth-bound solves) does not need the extra products.  The members of a group must agree on it. */
int32_t calipso_hip_set_field(calipso_hip_solver*, const char* name, const double* data, int64_t len);
int32_t calipso_hip_get_field(calipso_hip_solver*, const char* name, double* data, int64_t len);
/* The scatter of evaluate! on the device (evaluate.jl:37-121): register `methods.<field>_sparsity` once — `count` (row, col)
 * pairs, 1-based, in cache order, duplicates allowed — then hand over only the value caches of an evaluation: O(nnz) over PCIe instead of the
 * dense blocks.  Semantics of the reference: plain assignment in list order, so the LAST writer of a repeated entry wins (the trajectory layer
 * repeats entries across stages); the three Hessian matrices are assigned separately and summed into "lagrangian_hessian"
 * (residual_jacobian_variables.jl:10-16).  Fields: "objective_jacobian_variables_variables", "equality_dual_jacobian_variables_variables",
 * "cone_dual_jacobian_variables_variables" (calipso_hip_scatter_hessian; a NULL part is "not re-evaluated in this call": as in evaluate.jl:37-42
 * it keeps the values of its last scatter — zeros if it never had one; count = 0 in calipso_hip_set_sparsity drops a part),
 * "equality_jacobian_variables", "cone_jacobian_variables" (calipso_hip_scatter_field). */
int32_t calipso_hip_set_sparsity(calipso_hip_solver*, const char* field, int64_t count, const int64_t* rows, const int64_t* cols);
int32_t calipso_hip_scatter_field(calipso_hip_solver*, const char* field, const double* values, int64_t count);
int32_t calipso_hip_scatter_hessian(calipso_hip_solver*, const double* objective_values, int64_t n_objective, const double* equality_dual_values,
                                    int64_t n_equality_dual, const double* cone_dual_values, int64_t n_cone_dual);
/* Indices (indices.jl:1-63) as the handle computed them, 1-based; returns the length or a negative status */
int64_t calipso_hip_get_index(calipso_hip_solver*, const char* name, int64_t* out, int64_t cap);

/* ---- the hot path, one entry point per reference function ---------------------------------------------------- */
/* cone!(problem, methods, idx, point; barrier, barrier_gradient, product, jacobian, target)  cones/cone.jl:71-106
 * which: 0 = solution, 1 = candidate */
int32_t calipso_hip_cone(calipso_hip_solver*, int32_t which, int32_t flags);
/* residual!(data, problem, idx, solution, kappa, rho, lambda)  residual.jl:1-51 */
int32_t calipso_hip_residual(calipso_hip_solver*);
/* the reductions solve! takes of the residual and iterate (solve.jl:130-135, optimality_error.jl:1-27):
 * out[0]=||R||_p/N (p = opt.residual_norm) out[1]=optimality_error out[2]=max(||R_y||inf,||R_z||inf)
 * out[3]=||equality_constraint||inf out[4]=||cone_product||inf */
int32_t calipso_hip_violations(calipso_hip_solver*, double out[5]);
/* residual_jacobian_variables! + residual_jacobian_variables_symmetric!  (residual_jacobian_variables.jl:1-167)
 * materialised as the dense n x n K for inspection ("jacobian_variables_symmetric"); the factorisation below works
 * from the blocks and never needs this. */
int32_t calipso_hip_residual_jacobian_variables_symmetric(calipso_hip_solver*);
/* out = H * v with the unreduced Jacobian H (never materialised): mul! of iterative_refinement.jl:9,39; v, out host[N] */
int32_t calipso_hip_jacobian_variables_mul(calipso_hip_solver*, const double* v, double* out);
/* factorize!(linear_solver, K) + compute_inertia!(linear_solver)   linear_solver.jl:19-44, qdldl.jl:269-317,400-589
 * LDL^T of P K P' in the constraint-first order [z | y | x]; inertia = (positive, negative, zero).
 * Returns CALIPSO_WARN_ZERO_PIVOT if an exact zero pivot was met (positive is then -1, as qdldl.jl:456,579). */
int32_t calipso_hip_factorize(calipso_hip_solver*, int64_t inertia[3]);
/* inertia_correction!(solver)   inertia.jl:30-80  (IC-1..IC-6 incl. the reference's quirks); n_factorizations may be NULL */
int32_t calipso_hip_inertia_correction(calipso_hip_solver*, int64_t* n_factorizations);
/* residual_symmetric!  residual.jl:53-101; which: 0 residual, 1 residual_error */
int32_t calipso_hip_residual_symmetric(calipso_hip_solver*, int32_t which);
/* linear_solve!(solver, x, K, b; fact=false): step_symmetric = K \ residual_symmetric with the current factors
 * (linear_solver.jl:52-60, qdldl.jl:330-351).  The reference's hidden re-factorisation (fact=true) is NOT replicated:
 * the matrix is unchanged between calipso_hip_factorize and the solves, so the factors are reused. */
int32_t calipso_hip_linear_solve(calipso_hip_solver*);
/* search_direction_symmetric!  search_direction.jl:25-104; which: 0 (step <- residual), 1 (step_correction <- residual_error) */
int32_t calipso_hip_search_direction_symmetric(calipso_hip_solver*, int32_t which);
/* iterative_refinement!(step, solver)  iterative_refinement.jl:1-52; returns CALIPSO_WARN_REFINEMENT on failure.
 * rounds / final_norm may be NULL */
int32_t calipso_hip_iterative_refinement(calipso_hip_solver*, int32_t* rounds, double* final_norm);
/* search_direction!(solver)  search_direction.jl:1-23 = inertia correction + condensed solve + refinement (+ pivoted
 * dense fallback on the unreduced system when refinement fails, replacing `H \ R` of :113) */
int32_t calipso_hip_search_direction(calipso_hip_solver*);
/* search_direction_nonsymmetric!(step, H, residual, ...)  search_direction.jl:106-119 (`step .= H \ residual`): partially pivoted
 * dense LU of the unreduced N x N matrix (assembled on the device on demand).  "step" <- H^-1 "residual".  Exception path. */
int32_t calipso_hip_search_direction_nonsymmetric(calipso_hip_solver*);
/* cone fraction-to-boundary search  solve.jl:190-221 with cone_violation (cones/cone.jl:62-68): writes candidate s, t
 * and returns the two step sizes (opt.scaling_line_search^k, k = number of shrinkings).  CALIPSO_ERR_CONE_SEARCH once k would exceed
 * opt.max_cone_line_search (<= 831). */
int32_t calipso_hip_cone_search(calipso_hip_solver*, double* step_size, double* step_size_cone_slack_dual);
/* cone_violation(xhat, x, tau, ...)  cones/cone.jl:62-68 on host vectors of length nc; *violated = 0/1 */
int32_t calipso_hip_cone_violation(calipso_hip_solver*, const double* xhat, const double* x, double tau, int32_t* violated);
/* candidate x, r (and s when with_cone_slack) = solution - step_size * step   solve.jl:224-229, 268-276 */
int32_t calipso_hip_candidate(calipso_hip_solver*, double step_size, int32_t with_cone_slack);
/* merit(f, r, Phi, kappa, lambda, rho)  merit.jl:2-15 on point `which` (uses "objective" and "barrier") */
int32_t calipso_hip_merit(calipso_hip_solver*, int32_t which, double* M);
/* merit_gradient!  merit.jl:17-31 (solution point) */
int32_t calipso_hip_merit_gradient(calipso_hip_solver*);
/* constraint_violation!(c, g, r, h, s, idx; norm_type)  constraint_violation.jl:1-13 on point `which` */
int32_t calipso_hip_constraint_violation(calipso_hip_solver*, int32_t which, double* theta);
/* d = dot(merit_gradient, step.primals) used by switching_condition / armijo (line_search.jl:3,16) */
int32_t calipso_hip_merit_directional(calipso_hip_solver*, double* d);
/* accept the candidate: x,r,s <- candidate; y,z -= step_size*step; t <- candidate t   solve.jl:309-326 */
int32_t calipso_hip_accept(calipso_hip_solver*, double step_size);

/* ---- drivers ----------------------------------------------------------------------------------------------------- */
/* initialize!(solver, guess)  initialize.jl:9-13 */
int32_t calipso_hip_initialize(calipso_hip_solver*, const double* guess);
/* solve!(solver)  solve.jl:8-377: returns 1 (true), 0 (false) or a negative status.  eval may be NULL when a device
 * evaluator is attached (calipso_hip_qp_attach). */
int32_t calipso_hip_solve(calipso_hip_solver*, calipso_eval_fn eval, void* user);
/* differentiate!(solver)  differentiate.jl:1-61: dR/dtheta assembled on the device, one factorisation, then one condensed
 * solve + recovery per parameter column (as differentiate.jl:29-58, without its per-column re-factorisation).
 * Default: the columns are the UNREFINED condensed solve.  The reference's QDLDL works on the (nx + ne + nc) symmetric matrix; the constraint-first condensation onto
 * nx loses digits at a solution (penalty 1e7, central path 1e-7), so the columns agree with the reference only as far as the record in INTEGRATION.md (next to quirk
 * B-12) shows: 5e-10 .. 2e-9 relative to max(1, |S|) at the solutions measured there, already below 1e-8 — the option below is insurance, it brings
 * |H S + dR/dtheta| from 1e-10 .. 1e-9 down to 1e-16.
 * Option "opt.differentiate_refinement" = 1 (calipso_hip_set_field; a handle-level value like "opt.solve_block", not an option of the reference; default 0, other values
 * CALIPSO_ERR_ARGUMENT): the correction rounds of iterative_refinement.jl:14-44 on all columns together — E = dR/dtheta - H X with the unreduced, matrix-free H
 * (residual_jacobian_variables.jl:1-108), per-column infinity norms, the correction through the same factors, X(:, j) += correction(:, j) for the columns that have not
 * met the stopping test of iterative_refinement.jl:14-16 (the handle's iterative_refinement_tolerance, min_ / max_iterative_refinement; iterative_refinement = 0: no
 * rounds; a column already within the tolerance keeps the round min_iterative_refinement asks for only if it does not raise the column's norm, so the option never
 * leaves such a column with a larger residual than the unrefined solve had).  A column that exhausts its rounds with a larger error than it started with keeps its last iterate (differentiate! has no H \ residual fallback) and is counted.
 * Exception: on a handle whose layout has any second-order cone the option is inert, the columns are the unrefined solve bit for bit — that IS the reference's answer
 * there (its triu-symmetrised cone blocks, quirk B-3; refining would move away from it), and calipso_hip_differentiate_info reports 0 rounds. */
int32_t calipso_hip_differentiate(calipso_hip_solver*, calipso_eval_fn eval, void* user);
/* report of the last calipso_hip_differentiate (also the one at the end of calipso_hip_solve, solve.jl:144-146 with options.differentiate): [columns, correction rounds
 * run (largest over the columns; iterative_refinement.jl:14-44), columns that did not meet the stopping test (:45-51), largest final column norm
 * ||dR/dtheta(:, j) - H X(:, j)||_inf].  Zeros when no refinement ran; out[0] = columns is still filled in. */
int32_t calipso_hip_differentiate_info(calipso_hip_solver*, double out[4]);
/* differentiate! in REVERSE mode on a Solver handle (dense, stage-structured or stage-parallel): differentiate.jl:1-61 and residual_jacobian_parameters.jl:1-40,
 * transposed.  One factorisation with the regularisation the handle holds, as calipso_hip_differentiate; then for k cotangent columns v = dLoss/dw at once the
 * transposed map lambda = M' v of the map M that calipso_hip_differentiate applies to a column: the condensed solve of differentiate.jl:29-58 stage by stage in reverse
 * order (search_direction.jl:38-101 and residual.jl:53-101 transposed; the products with [gx; hx] and the solve with the factor of S are their own transposes, S being
 * factored from one triangle).  One condensed solve per cotangent instead of one per parameter column.  The fields are those of the last search direction (quirk
 * B-12), as for calipso_hip_differentiate: grad_theta = S' v for the S = dw/dtheta that calipso_hip_differentiate would return on the same handle state.
 * Host arrays:
 *   cotangent   N x k, column-major, required
 *   adjoint     N x k = lambda = M' v, or NULL
 *   grad_theta  np x k = -R_theta' lambda = S' v, or NULL (the parameter Jacobians are evaluated as by calipso_hip_differentiate: `eval`, or the device evaluator)
 *   grad_qp     NULL, or six pointers in the order P, q, A, b, G, h (NULLs skipped) on a handle with calipso_hip_qp_attach: per cotangent column the gradient with
 *               respect to that array of the QP, each k x size with the matrices column-major as calipso_hip_qp_attach takes them:
 *               P: -c (lambda_x x' + x lambda_x'); q: -lambda_x; A: -(lambda_y x' + y lambda_x'); b: lambda_y; G: lambda_z x' + z lambda_x'; h: -lambda_z
 *               with x, y, z of the resident point and c the objective scale
 * "opt.differentiate_refinement" = 1 with iterative_refinement = 1: the correction rounds of calipso_hip_differentiate on all cotangent columns, against H' (E = v - H'
 * lambda; the same per-column stopping and restoring decisions).  Inert on a handle with any second-order cone, as for calipso_hip_differentiate (quirk B-3): the result is the
 * unrefined transposed map bit for bit.
 * The call keeps its own workspace (grown on demand, kept, counted in the device bytes of calipso_hip_kernel_times); it leaves solution_sensitivity and the workspace
 * of calipso_hip_differentiate alone.  CALIPSO_ERR_ARGUMENT with calipso_hip_last_error naming the argument: a NULL handle, k < 1 (or above 65535), a NULL cotangent,
 * grad_theta with np = 0, grad_qp on a handle without an attached QP.  A compact structured handle whose block products are not available is refused with the message of
 * calipso_hip_differentiate. */
int32_t calipso_hip_differentiate_adjoint(calipso_hip_solver*, calipso_eval_fn eval, void* user, int64_t k,
                                          const double* cotangent,   /* N x k, column-major, required */
                                          double* adjoint,           /* N x k = lambda = M' v, or NULL */
                                          double* grad_theta,        /* np x k = -R_theta' lambda = S' v, or NULL */
                                          double* const* grad_qp);   /* NULL, or six pointers P, q, A, b, G, h (NULLs skipped), each k x size, column-major matrices */
/* as calipso_hip_differentiate_info, for the last reverse call: [cotangent columns, correction rounds run (largest over the columns), columns that did not meet the
 * stopping test, largest final column norm ||v - H' lambda||_inf]; zeros when no round ran, out[0] is still filled in */
int32_t calipso_hip_differentiate_adjoint_info(calipso_hip_solver*, double out[4]);
/* HIP-event times of the last reverse call in ms (a deliberate addition for callers that budget the call, and for bench/differentiate_adjoint.py): [0] from its entry to
 * its last kernel (evaluation of the parameter Jacobians — a host callback included, when grad_theta is asked for —, factorisation, transposed solve, rounds, gradient
 * kernels), [1] the copies of the results to the host arrays, [2] of [0] the QP data-gradient kernels alone, between events of their own (0 without grad_qp) */
int32_t calipso_hip_differentiate_adjoint_times(calipso_hip_solver*, double out[3]);
/* install a device-side evaluator (NULL removes it): calipso_hip_solve / calipso_hip_differentiate / the group drivers then call it instead
 * of the host callback (their `eval` argument may be NULL), and calipso_hip_device_evaluate runs it on point `which` (0 solution, 1 candidate) */
int32_t calipso_hip_set_device_evaluator(calipso_hip_solver*, calipso_device_eval_fn fn, void* user);
/* structured handles only (CALIPSO_ERR_ARGUMENT otherwise): the evaluator writes the packed blocks (calipso_device_block_data above); replaces an evaluator set by
 * calipso_hip_set_device_evaluator.  evaluate.jl:37-121 */
int32_t calipso_hip_set_device_block_evaluator(calipso_hip_solver*, calipso_device_block_eval_fn fn, void* user);
int32_t calipso_hip_device_evaluate(calipso_hip_solver*, int32_t which, uint32_t flags);
/* install the per-inner-iteration / per-outer-update callbacks (NULL disables; options.callback_inner/outer) */
int32_t calipso_hip_set_callbacks(calipso_hip_solver*, calipso_callback_fn inner, calipso_callback_fn outer, void* user);
/* statistics of the last solve: [total_iterations, outer, factorizations, refinement_failures, max_refinement_rounds,
 * fallbacks, last_refinement_rounds, newton_steps] */
int32_t calipso_hip_stats(calipso_hip_solver*, int64_t out[8]);

/* ---- device-resident conic QP evaluator (synthetic benchmark inputs) ------------------------------- */
/* min c*x'Px + q'x  s.t. Ax - b = 0, h - Gx in K.  Host arrays are copied once; afterwards evaluate! runs as device
 * mat-vecs and no host callback is needed (eval = NULL).  P must be symmetric.
 * The equality Jacobian gx = A of such a handle stays what this call installed, and every first factorisation of an inertia correction uses the same initial
 * regularisation: a dense handle stepped alone (padded nx >= 1024, ne > 0) therefore keeps the equality products gx' (omega_y gx) of the Schur complement in a buffer of
 * its own (padded nx squared doubles) and its later factorisations start from them, until the penalty changes, gx is written (this call, calipso_hip_set_field /
 * calipso_hip_scatter_field of equality_jacobian_variables, a device evaluator) or the regularisation differs (the retries of an inertia correction go without).
 * The factor is the same to the bit either way.  "opt.schur_cache" = 0 (calipso_hip_set_field) turns it off; calipso_hip_schur_cache_info counts.  (bench.py's
 * roofline.achieved counts the algorithmic flops of a step: with hits the device executes fewer than it is credited with.) */
int32_t calipso_hip_qp_attach(calipso_hip_solver*, const double* P, const double* q, const double* A, const double* b,
                              const double* G, const double* h, double objective_scale);
/* evaluate!(...; flags) with the attached evaluator on point `which` */
int32_t calipso_hip_qp_evaluate(calipso_hip_solver*, int32_t which, uint32_t flags);
/* One inner Newton iteration of solve! (solve.jl:98-353) at the current iterate with fixed kappa/rho, device evaluator
 * attached; if `advance` is 0 the iterate is restored afterwards (benchmark mode: every step does identical work).
 * info[0]=step_size info[1]=step_size_t info[2]=refinement rounds info[3]=factorizations info[4]=M_candidate info[5]=theta_candidate */
int32_t calipso_hip_newton_step(calipso_hip_solver*, int32_t advance, double info[6]);
/* `count` such steps in one call — the loop a caller would write around calipso_hip_newton_step (solve.jl:107-377 runs its iterations without leaving the
 * solver either): info = count x 6 doubles (may be NULL), status = count return codes; stops at the first failing step (its code is returned).  The stream is
 * synchronised and the phase timers are read after the LAST step only. */
int32_t calipso_hip_newton_steps(calipso_hip_solver*, int32_t count, int32_t advance, double* info, int32_t* status);
/* ---- groups: several handles of one shape stepped in lockstep through the same kernel launches ------------------------------
 * The reference has no batching: distinct `Solver`s are simply independent; BASELINE config C4 runs many of them
 * per GPU.  A group covers up to 128 handles created with identical dimensions and cone layout on one device; every launch of a
 * group step carries all members (the instance is a grid dimension), so the latency-bound parts of the step cost the same for
 * the whole group as for one handle.  Per member the arithmetic is exactly that of calipso_hip_newton_step.  Members stay
 * usable through the single-handle entry points between group calls (not concurrently with them). */
typedef struct calipso_hip_group calipso_hip_group;
int32_t calipso_hip_group_create(calipso_hip_solver** handles, int32_t count, calipso_hip_group** out);
int32_t calipso_hip_group_destroy(calipso_hip_group*);
/* calipso_hip_newton_step for every member: info = count x 6 doubles (row per member, fields as above), status = count codes */
int32_t calipso_hip_group_newton_step(calipso_hip_group*, int32_t advance, double* info, int32_t* status);
/* solve!(solver) (solve.jl:8-377) for every member in lockstep: result[i] = 1 converged, 0 iteration caps reached, < 0 the
 * member's error code.  Per member identical to calipso_hip_solve.  Members with a device evaluator are evaluated inside the
 * group's launches; the others through their host callback (calipso_hip_group_set_evaluators: one calipso_eval_fn / user pointer
 * per member, NULL where a device evaluator is attached), one member after the other. */
int32_t calipso_hip_group_set_evaluators(calipso_hip_group*, const calipso_eval_fn* evals, void* const* users);
int32_t calipso_hip_group_solve(calipso_hip_group*, int32_t* result);
/* differentiate! in REVERSE mode for every member through the same launches (differentiate.jl:1-61 and residual_jacobian_parameters.jl:1-40, transposed): per member exactly
 * what calipso_hip_differentiate_adjoint gives with "opt.differentiate_refinement" = 0.  ONE factorisation over all members, each with the regularisation it holds
 * (differentiate.jl:13-20; the fields are those of the last search direction, quirk B-12), then the condensed solve of differentiate.jl:29-58 transposed
 * (search_direction.jl:38-101 and residual.jl:53-101 in reverse order; the first-row quirk of the second-order dt recovery, second_order.jl:63-65, is kept) for all members
 * and all k columns in the same launches: the products and the block triangular solves are batched fp64 MFMA GEMMs with the member in a grid dimension — every k, k = 1
 * included.  Every cone layout the single-handle entry admits.  Host arrays, member-major (member i's share at i x the share's size):
 *   cotangent   count x (N x k), column-major per member, required
 *   adjoint     count x (N x k) = lambda_i = M_i' v_i, or NULL
 *   grad_theta  count x (np x k) = -R_theta' lambda_i = S_i' v_i, or NULL.  The parameter Jacobians (differentiate.jl:3) are evaluated as calipso_hip_group_solve evaluates:
 *               device evaluators inside the group's launches, host callbacks of calipso_hip_group_set_evaluators one member after the other
 *   grad_qp     NULL, or six pointers P, q, A, b, G, h (NULLs skipped), every member with calipso_hip_qp_attach: each count x (k x size), the closed forms of
 *               calipso_hip_differentiate_adjoint with the member's point and objective scale (the gradient of P symmetric to the bit)
 *   status      count codes, required: what calipso_hip_differentiate_adjoint would return for that member alone.  The group's factorisation has no failure of one member
 *               that the single-handle entry would report (a zero pivot is none there either: the values are then not finite); a launch the runtime refuses fails the call
 *   ms          NULL, or the HIP-event time in ms from the entry's first enqueue to its last kernel
 * Returns as calipso_hip_group_newton_step: CALIPSO_OK, or the error of the call as a whole.  Afterwards calipso_hip_differentiate_adjoint_info of every member reads
 * [k, 0, 0, 0].  The workspace (count x the columns of one handle's reverse call, and the staging of the gradients) belongs to the group: grown on demand, kept, freed by
 * calipso_hip_group_destroy.  The members' own workspaces, solution_sensitivity and points are left alone (their factors are overwritten, as by any factorisation).
 * CALIPSO_ERR_ARGUMENT, calipso_hip_last_error of the first member naming the cause, the group and its members usable afterwards: k < 1 (or above 65535), a NULL cotangent
 * or status, grad_theta with np = 0, grad_qp with a member that has no attached QP, a member with "opt.differentiate_refinement" = 1 (the correction rounds have no group
 * form), a member with an analysed structure (calipso_hip_analyze_structure, stage blocks, stage-parallel, structured handles: dense treatment only), a dead group. */
int32_t calipso_hip_group_differentiate_adjoint(calipso_hip_group*, int64_t k,
                                                const double* cotangent,   /* count x (N x k), member-major, column-major per member; required */
                                                double* adjoint,           /* count x (N x k) = lambda_i = M_i' v_i, or NULL */
                                                double* grad_theta,        /* count x (np x k) = -R_theta' lambda = S_i' v_i, or NULL */
                                                double* const* grad_qp,    /* NULL, or six pointers P, q, A, b, G, h (NULLs skipped), each count x (k x size), matrices column-major */
                                                int32_t* status,           /* count: what calipso_hip_differentiate_adjoint would return for that member alone */
                                                double* ms);               /* NULL, or the HIP-event time from the entry's first enqueue to its last kernel */
/* differentiate! in FORWARD mode for every member through the same launches (differentiate.jl:1-61): per member exactly what calipso_hip_differentiate gives on that
 * handle alone with "opt.differentiate_refinement" = 0.  The parameter Jacobians (differentiate.jl:3) are evaluated as calipso_hip_group_solve evaluates (device evaluators
 * inside the group's launches, host callbacks of calipso_hip_group_set_evaluators one member after the other), ONE factorisation over all members, each with the
 * regularisation it holds (differentiate.jl:13-20, quirk B-12), dR/dtheta of all members in one launch (:23, residual_jacobian_parameters.jl:1-40), then the condensed
 * solve of :29-58 (residual.jl:53-101, search_direction.jl:38-101) for all members' np columns in the same launches — the products and the block triangular solves as
 * batched fp64 MFMA GEMMs with the member in a grid dimension — and sensitivity = -step (:54-56).  Every cone layout the single-handle entry admits.
 *   sensitivity count x (N x np) host doubles, member-major, column-major per member, or NULL.  Either way every member's own solution_sensitivity and
 *               jacobian_parameters hold its result afterwards (calipso_hip_get "solution_sensitivity" reads what it reads after calipso_hip_differentiate)
 *   status      count codes, required: what calipso_hip_differentiate would return for that member alone (a launch the runtime refuses fails the call)
 *   tile        columns of the batched products per workgroup: 0 = the library's choice by np, 16 or 64 force a form.  The two forms give the same bits
 *   ms          NULL, or two HIP-event times in ms: [0] from the entry's first enqueue to its last kernel, [1] of that the column pass alone, from dR/dtheta formed to
 *               the last kernel (without the host callbacks and the factorisation)
 * Afterwards calipso_hip_differentiate_info of every member reads [np, 0, 0, 0].  The workspace (count x the columns of one handle's forward call) belongs to the group:
 * grown on demand, kept, freed by calipso_hip_group_destroy; the group's reverse workspace and the members' own are left alone.
 * CALIPSO_ERR_ARGUMENT, calipso_hip_last_error of the first member naming the cause, the group and its members usable afterwards: a dead or NULL group, a NULL status,
 * a tile other than 0, 16, 64, np = 0, a member with "opt.differentiate_refinement" = 1 (the correction rounds have no group form), a member with an analysed structure
 * (calipso_hip_analyze_structure, stage blocks, stage-parallel, structured handles: dense treatment only), a member with neither a device evaluator nor a callback. */
int32_t calipso_hip_group_differentiate(calipso_hip_group*,
                                        double* sensitivity,   /* count x (N x np), member-major, column-major per member, or NULL */
                                        int32_t* status,       /* count: what calipso_hip_differentiate would return for that member alone */
                                        int32_t tile,          /* 0, 16 or 64 columns per workgroup of the batched products */
                                        double ms[2]);         /* NULL, or [whole call, column pass] in ms */

/* ---- stage-banded structure -------------------------------------------------------------------------------
 * Trajectory-optimisation problems order their variables stage by stage (src/trajectory_optimization/indices.jl:41-180), which
 * makes the Schur complement onto x banded.  calipso_hip_analyze_structure reads the non-zero pattern of the blocks the handle
 * currently holds (lagrangian_hessian, equality / cone Jacobians) and from then on the factorisation and the triangular solves
 * skip everything outside the band (the reference obtains the same saving from its sparse LDL^T, qdldl.jl:400-589).  Results are
 * bit-identical to the dense treatment.  Re-run it (or calipso_hip_clear_structure) if the pattern of the blocks changes.
 * out[0] = half bandwidth of S, out[1] = 64-row blocks per panel inside the band (0: dense treatment kept),
 * out[2], out[3] = average number of equality / cone rows a 16-column group visits.  out may be NULL. */
int32_t calipso_hip_analyze_structure(calipso_hip_solver*, int64_t out[4]);
int32_t calipso_hip_clear_structure(calipso_hip_solver*);
/* Stage-parallel factorisation of the Schur complement (the reference gets its parallel-free equivalent from AMD + sparse QDLDL,
 * qdldl.jl:134-188,400-589): after calipso_hip_analyze_structure, S is factored by the multifrontal sparse LDL^T over a nested dissection of its
 * skyline pattern (for a trajectory problem: log2(stages) launches instead of the chain of nx pivots) and solved over the same tree.  `batch` >= the
 * largest group this handle will lead (1 for a handle stepped alone).  Same inertia as the blocked factorisation; values agree to rounding.
 * info (may be NULL) = [tree levels, rows of the largest front, nnz(triu) of the pattern of S, 2].  on = 0 switches back.  Fails (and keeps the
 * blocked factorisation) when a front would exceed one CU's LDS (196 rows). */
int32_t calipso_hip_set_stage_parallel(calipso_hip_solver*, int32_t on, int32_t batch, int64_t info[4]);
/* Stage blocks (after calipso_hip_analyze_structure; SURVEY.md 8(f1): the reference keeps stage-structured problems sparse end to end,
 * src/trajectory_optimization/sparsity.jl:28-129, src/solver/evaluate.jl:37-121): the runs of constraint rows with one column range and the diagonal
 * blocks of the Lagrangian Hessian are packed contiguously and the mat-vecs of the Newton step and the Schur-complement kernel work on the packed
 * blocks (one workgroup per block / per pair of column segments) instead of the dense-layout kernels.  The dense buffers stay the interchange format of
 * the uploads; a pack kernel follows every upload on the handle's stream.  Results agree with the dense treatment to rounding (not bitwise).  on = 0
 * switches back.  Refused when the structure has fewer than two Hessian blocks.  Members of a group must agree (all on with one structure, or all off).
 * info (may be NULL) = [Z blocks, Hessian blocks, column segments, packed doubles per instance]. */
int32_t calipso_hip_set_stage_blocks(calipso_hip_solver*, int32_t on, int64_t info[4]);

/* ---- LinearSolver seam (src/solver/linear_solver.jl:1-60) ----------------------------------------------------------------------
 * A stand-alone device LDL^T for ANY sparse symmetric quasi-definite matrix the caller assembled itself, so that the reference's own
 * search_direction! / iterative_refinement! / differentiate! / inertia_correction! (which hand `data.jacobian_variables_symmetric`
 * to `solver.linear_solver`) run unmodified on the GPU factorisation: `HIPLDLSolver <: LinearSolver` in julia/CalipsoHIP.jl.
 *   calipso_hip_ldl_create         = ldl_solver(A)                               linear_solver.jl:46-50  (destroy: calipso_hip_destroy)
 *   calipso_hip_ldl_factorize_csc  = factorize!(s, A; update) + compute_inertia! linear_solver.jl:19-44, qdldl.jl:134-188,269-317
 *   calipso_hip_ldl_inertia        = compute_inertia!(s) of the last factorisation
 *   calipso_hip_ldl_solve          = linear_solve!(s, x, A, b; fact=false)       linear_solver.jl:52-60,82-99, qdldl.jl:330-351
 * A is Julia's SparseMatrixCSC: colptr[n+1], rowval[nnz] 1-based Int64, nzval[nnz]; only triu(A) is read (linear_solver.jl:23);
 * no pivoting; inertia = (#D>0, #D<=0, #D==0), positive = -1 and CALIPSO_WARN_ZERO_PIVOT on an exact zero pivot (qdldl.jl:456,579).
 * b, x: column-major n x nrhs host arrays (may alias). */
int32_t calipso_hip_ldl_create(int64_t n, int32_t device, calipso_hip_solver** out);
int32_t calipso_hip_ldl_factorize_csc(calipso_hip_solver*, int64_t n, const int64_t* colptr, const int64_t* rowval, const double* nzval,
                                      int64_t inertia[3]);
int32_t calipso_hip_ldl_inertia(calipso_hip_solver*, int64_t inertia[3]);
/* Ordering / symbolic service (qdldl.jl:134-188,358-395,642-742).  Host-side integer work, 1-based Int64 like the reference.
 *   calipso_hip_ordering: elimination order of a sparse symmetric pattern (CSC, any triangle(s)): method 0 natural, 1 reverse Cuthill-McKee
 *     (minimum bandwidth: what the dense device factorisation exploits), 4 nested dissection (level-structure separators: minimum tree height, what
 *     the sparse device factorisation exploits), 2 minimum degree on the quotient graph (AMD's order class; AMD.jl's exact
 *     output, qdldl.jl:135, is third-party and unpinned).  perm[k] = vertex eliminated k-th.
 *   calipso_hip_symbolic: permute_symmetric + QDLDL_etree! for triu(A) under perm (NULL = natural): Pp[n+1], Pi[nnz triu], AtoPAPt[nnz A] (0 below
 *     the diagonal), etree[n] (-1 = root), Lnz[n]; returns nnz(L) (-1 in the reference's failure cases); info = [half bandwidth of PAP', nnz triu].
 *     Bit-exact against the oracle's restatement for the same perm.  Outputs may be NULL.
 *   calipso_hip_ldl_analyze_csc: installs the order on a calipso_hip_ldl_create handle (method 3 = the caller's perm); the following
 *     calipso_hip_ldl_factorize_csc calls factor P A P' and, if it is banded, only inside the band; calipso_hip_ldl_solve permutes the right-hand
 *     sides (qdldl.jl:330-351).  info = [half bandwidth, band blocks used (0 = dense treatment), nnz(L) symbolic, nnz triu]. */
int32_t calipso_hip_ordering(int64_t n, const int64_t* colptr, const int64_t* rowval, int32_t method, int64_t* perm);
int64_t calipso_hip_symbolic(int64_t n, const int64_t* colptr, const int64_t* rowval, const int64_t* perm, int64_t* Pp, int64_t* Pi, int64_t* AtoPAPt,
                             int64_t* etree, int64_t* Lnz, int64_t info[2]);
int32_t calipso_hip_ldl_analyze_csc(calipso_hip_solver*, int64_t n, const int64_t* colptr, const int64_t* rowval, int32_t method, int64_t* perm,
                                    int64_t info[4]);
int32_t calipso_hip_ldl_solve(calipso_hip_solver*, int64_t n, int64_t nrhs, const double* b, double* x);

/* ---- sparse LDL^T on the device (src/solver/qdldl.jl:134-188 analyse, :400-589 factor, :330-351,592-640 solve) --------
 * The LinearSolver seam WITHOUT dense n x n storage: memory O(nnz(L)).  The analyse phase (host) orders the matrix (method 0 natural, 1 RCM,
 * 2 minimum degree, 4 nested dissection, 3 = the caller's 1-based `perm`), builds P A P', the elimination tree, the pattern of L and the LEVEL
 * schedule; the numeric phase is a left-looking factorisation by tree levels (one launch per level, one workgroup per column, single-column levels
 * merged into chains) and level-scheduled triangular solves.  With a nested-dissection order the stages of a trajectory problem
 * (trajectory_optimization/sparsity.jl:28-129) are eliminated in parallel: the number of levels is the sequential depth.  No pivoting; inertia and
 * zero-pivot behaviour as calipso_hip_ldl_factorize_csc.  L and D agree with QDLDL's to rounding (the summation order differs).
 *   calipso_hip_sparse_create      = QDLDL analyse of qdldl(A; perm)          qdldl.jl:134-188, 358-395, 642-742  (pattern only: colptr, rowval 1-based)
 *   calipso_hip_sparse_factorize   = QDLDL_factor! + compute_inertia!         qdldl.jl:400-589, linear_solver.jl:19-44  (nzval in the pattern's order, host)
 *   calipso_hip_sparse_solve       = solve!(F, b) for nrhs columns            qdldl.jl:330-351
 *   calipso_hip_sparse_get_factor  = F.perm, F.L (strictly lower, 1-based CSC), F.D   qdldl.jl:160-166
 *   calipso_hip_sparse_info        info[8] = n, nnz(triu A), nnz(L), tree levels, launches per factorisation, widest level, multiply-adds,
 *                                  numeric phase (0 columns / global accumulator, 1 columns / LDS accumulator, 2 multifrontal)
 *   calipso_hip_sparse_timing      ms[2] = device time of the last factorisation / solve (HIP events on the handle's stream)
 *   calipso_hip_sparse_set_batch   `batch` matrices of the analysed pattern per call (BASELINE config C4: many independent problems of one structure):
 *                                  nzval = batch x nnz, inertia = batch x 3, b / x = batch x (n x nrhs); the multifrontal path factors them in the
 *                                  same launches.  calipso_hip_sparse_select picks the matrix calipso_hip_sparse_get_factor reads.
 * Numeric phase: with method 4 (nested dissection) the factorisation is MULTIFRONTAL over the dissection tree — the pieces of the dissection (cut into
 * chains of <= 64 columns) are the supernodes, each front is assembled and partially factored by one workgroup, in its LDS when the front has <= 196
 * rows, in global memory up to 1024 rows; one launch per tree level (~log2 T launches for a T-stage problem).  Larger fronts, every other order
 * and method 5 (nested-dissection order, column method) take the left-looking column method. */
typedef struct calipso_hip_sparse calipso_hip_sparse;
int32_t calipso_hip_sparse_create(int64_t n, const int64_t* colptr, const int64_t* rowval, int32_t method, const int64_t* perm, int32_t device,
                                  calipso_hip_sparse** out);
int32_t calipso_hip_sparse_destroy(calipso_hip_sparse*);
const char* calipso_hip_sparse_last_error(calipso_hip_sparse*);
int32_t calipso_hip_sparse_info(calipso_hip_sparse*, int64_t info[8]);
int32_t calipso_hip_sparse_set_batch(calipso_hip_sparse*, int64_t batch);
int32_t calipso_hip_sparse_select(calipso_hip_sparse*, int64_t instance);
int32_t calipso_hip_sparse_factorize(calipso_hip_sparse*, const double* nzval, int64_t* inertia);
int32_t calipso_hip_sparse_solve(calipso_hip_sparse*, int64_t nrhs, const double* b, double* x);
/* the same with values / right-hand sides / solutions already resident on the handle's device (device pointers) */
int32_t calipso_hip_sparse_factorize_device(calipso_hip_sparse*, const double* d_nzval, int64_t* inertia);
int32_t calipso_hip_sparse_solve_device(calipso_hip_sparse*, int64_t nrhs, const double* d_b, double* d_x);
int32_t calipso_hip_sparse_get_factor(calipso_hip_sparse*, int64_t* perm, int64_t* Lp, int64_t* Li, double* Lx, double* D);
int32_t calipso_hip_sparse_timing(calipso_hip_sparse*, double ms[2]);

/* ---- search_direction! on sparse problem data resident on the device (csrc/sparse_kkt.hip; analysis: csrc/sparse_kkt.hpp) ---------------------------
 * The linear-algebra half of a sparse solve!: search_direction! (src/solver/search_direction.jl:1-23) for a problem whose Lagrangian Hessian and Jacobians
 * are SPARSE and stay on the device — no nx x nx or (ne + nc) x nx array exists anywhere.  Sparse non-zeros, a point w (layout of point.jl:13-22,
 * N = nx + 2 ne + 3 nc) and a residual go in; the step, the regularisation it ended with and the work it took come out.  One system per handle.
 * Patterns are Julia SparseMatrixCSC patterns (1-based Int64, rows ascending and duplicate-free within a column; else CALIPSO_ERR_ARGUMENT and a text):
 * Lxx (nx x nx: the full Lagrangian Hessian, BOTH triangles, as the reference holds it), gx (ne x nx), hx (nc x nx).  Cone layout as
 * calipso_hip_smallnewton_set_cones: n_nonnegative rows, then n_soc contiguous second-order cones of dims[j] >= 2 — of ANY dimension: the blocks are formed
 * column by column through the closed form of second_order_matrix_inverse (cones/second_order.jl:50-65), O(dimension) per column.
 *   create          the pattern of triu(K) of jacobian_variables_symmetric (solver.jl:88-122 obtains it from a warm-up assembly) + qdldl(K; perm) analyse
 *                   (qdldl.jl:134-188) through calipso_hip_sparse_create: method / perm as there.  Without a HIP device: CALIPSO_ERR_HIP, "no HIP device".
 *   info            info[8] = n, nnz(triu K), nnz(L), tree levels, numeric phase (as calipso_hip_sparse_info), launches of one assemble, largest cone dimension, N
 *   pattern         colptr[n + 1], rowval[nnz(triu K)] of triu(K), 1-based, in the order idx.variables, idx.symmetric_equality, idx.symmetric_cone (indices.jl:20-63)
 *   set_option      the regularisation and refinement options of options.jl:6-59 by name (include/calipso_options.hpp: set_search_direction_option), and
 *                   "central_path": the solver's scalar that IC-2 reads (inertia.jl:44)
 *   set_values      nzval of Lxx, gx, hx in the patterns' order, the point w (N), the penalty rho (1): host arrays, or (_device) device pointers on the handle's
 *                   device — a host or foreign pointer there is CALIPSO_ERR_ARGUMENT naming the argument.  NULL keeps what is resident.
 *   factorize       residual_jacobian_variables! + residual_jacobian_variables_symmetric! (residual_jacobian_variables.jl:1-167) at the given (ep, ed), on the
 *                   device and without forming H, then factorize! + compute_inertia! (linear_solver.jl:19-44); CALIPSO_WARN_ZERO_PIVOT as calipso_hip_sparse_factorize
 *   get_matrix      K.nzval of the last assemble (jacobian_variables_symmetric, upper triangle)
 *   mul             out = H v for the unreduced N x N matrix at the regularisation of the last assemble (mul!(e, H, v), iterative_refinement.jl:9,39)
 *   solve_symmetric search_direction_symmetric! (search_direction.jl:25-104): residual_symmetric! (residual.jl:53-101), linear_solve! with the current
 *                   factorisation, the recovery of the r-, s- and t-parts (search_direction.jl:59-101)
 *   search_direction  search_direction! whole: inertia_correction! (inertia.jl:30-80; every retry one assemble + one factorisation), search_direction_symmetric!,
 *                   iterative_refinement! (iterative_refinement.jl:1-52; a round reads back one double).  regularization = [ep, ep_last, ed], in and out:
 *                   ep_last is what the caller carries from call to call (primal_regularization_last).  info = [factorisations, refinement rounds,
 *                   |residual - H step|_inf at exit, GMRES iterations of the fallback].  (_device: residual and step are device pointers.)  Returns CALIPSO_OK,
 *                   CALIPSO_ERR_INERTIA, CALIPSO_ERR_ARGUMENT, CALIPSO_ERR_HIP, or CALIPSO_WARN_REFINEMENT: where the reference's refinement fails it goes on to
 *                   `H \ residual` (search_direction.jl:22).  By default there is NO such fallback here: the call returns the warning with the last refined step in
 *                   place, and the handle stays usable.  With the option krylov_fallback = 1 the call goes on to solve_nonsymmetric below and still returns the
 *                   warning, as the dense handle does; a fallback that met a non-finite number leaves the last refined step in place, exactly as without the option.
 *   solve_nonsymmetric  search_direction_nonsymmetric! for this handle, `H \ residual` without a pivoted LU (csrc/sparse_krylov.hip, host logic csrc/sparse_krylov.hpp):
 *                   restarted right-preconditioned GMRES on the unreduced H at the regularisation of the last assemble, preconditioned by solve_symmetric with the
 *                   CURRENT factorisation, started from zero, whatever krylov_fallback says.  V and Z = M V are kept, so a cycle ends with x += Z y; classical
 *                   Gram-Schmidt applied twice, two launches per pass whatever the iteration; one read-back per iteration.  A cycle ends when the estimate |g_j+1|
 *                   (a 2-norm, which bounds the infinity norm) is at or below iterative_refinement_tolerance, at krylov_restart columns, or on an exact breakdown;
 *                   then the TRUE |residual - H step|_inf decides: stop, restart from that residual, or — after krylov_max_cycles — leave the step in place
 *                   unconverged (the reference does not inspect its LU's answer either).  Sums are reduced in a fixed order: a call repeats bit for bit.  Returns
 *                   CALIPSO_OK converged, CALIPSO_WARN_REFINEMENT unconverged (not finite: a zero step); refusals as solve_symmetric.  (_device: device pointers.)
 *   fallback_info   out[12]: of the last search_direction / solve_nonsymmetric [0] fallback taken, [1] GMRES iterations, [2] cycles, [3] the final true
 *                   |residual - H step|_inf, [4] converged, [5] device ms (HIP events), [6] launches of the fallback's own kernels; accumulated over the last solve
 *                   [7] fallbacks, [8] their iterations, [9] most iterations of one, [10] unconverged ones; [11] bytes of the workspace ((2 restart + 1) N doubles
 *                   and partials, reserved on the first fallback and kept)
 *   set_option      additionally krylov_fallback (0 / 1, default 0), krylov_restart (1 .. 32, default 16), krylov_max_cycles (1 .. 16, default 4); any other value is
 *                   CALIPSO_ERR_ARGUMENT
 *   timing          ms[8] of the last search_direction, HIP events on the handle's stream: [assembles, factorisations, first solve, refinement solves,
 *                   H v + norm of all rounds, wall-clock of the call, 0, 0]; the last two slots belong to the differentiate entries below: of the last
 *                   solve_columns / differentiate / differentiate_adjoint, [6] its first pre + multi-column solve + post, [7] its correction rounds with their
 *                   read-backs (their assemble and factorisation are added to [0] and [1]) */
typedef struct calipso_hip_sparse_kkt calipso_hip_sparse_kkt;
int32_t calipso_hip_sparse_kkt_create(int64_t nx, int64_t ne, int64_t nc, int64_t n_nonnegative, int64_t n_soc, const int64_t* dims, const int64_t* Lxx_colptr,
                                      const int64_t* Lxx_rowval, const int64_t* gx_colptr, const int64_t* gx_rowval, const int64_t* hx_colptr, const int64_t* hx_rowval,
                                      int32_t method, const int64_t* perm, int32_t device, calipso_hip_sparse_kkt** out);
int32_t calipso_hip_sparse_kkt_destroy(calipso_hip_sparse_kkt*);
const char* calipso_hip_sparse_kkt_last_error(calipso_hip_sparse_kkt*);
int32_t calipso_hip_sparse_kkt_info(calipso_hip_sparse_kkt*, int64_t info[8]);
int32_t calipso_hip_sparse_kkt_pattern(calipso_hip_sparse_kkt*, int64_t* colptr, int64_t* rowval);
int32_t calipso_hip_sparse_kkt_set_option(calipso_hip_sparse_kkt*, const char* name, double value);
int32_t calipso_hip_sparse_kkt_set_values(calipso_hip_sparse_kkt*, const double* Lxx, const double* gx, const double* hx, const double* w, const double* penalty);
int32_t calipso_hip_sparse_kkt_set_values_device(calipso_hip_sparse_kkt*, const double* Lxx, const double* gx, const double* hx, const double* w, const double* penalty);
int32_t calipso_hip_sparse_kkt_factorize(calipso_hip_sparse_kkt*, double ep, double ed, int64_t inertia[3]);
int32_t calipso_hip_sparse_kkt_get_matrix(calipso_hip_sparse_kkt*, double* nzval);
int32_t calipso_hip_sparse_kkt_mul(calipso_hip_sparse_kkt*, const double* v, double* out);
int32_t calipso_hip_sparse_kkt_solve_symmetric(calipso_hip_sparse_kkt*, const double* residual, double* step);
int32_t calipso_hip_sparse_kkt_search_direction(calipso_hip_sparse_kkt*, const double* residual, double* step, double regularization[3], double info[4]);
int32_t calipso_hip_sparse_kkt_search_direction_device(calipso_hip_sparse_kkt*, const double* residual, double* step, double regularization[3], double info[4]);
int32_t calipso_hip_sparse_kkt_timing(calipso_hip_sparse_kkt*, double ms[8]);
int32_t calipso_hip_sparse_kkt_solve_nonsymmetric(calipso_hip_sparse_kkt*, const double* residual, double* step);
int32_t calipso_hip_sparse_kkt_solve_nonsymmetric_device(calipso_hip_sparse_kkt*, const double* residual, double* step);
int32_t calipso_hip_sparse_kkt_fallback_info(calipso_hip_sparse_kkt*, double out[12]);

/* ---- search_direction! on sparse data, for GROUPS of same-pattern problems in lockstep (csrc/sparse_kkt_group.hip; host bookkeeping: csrc/sparse_kkt_group.hpp) ----
 * `members` problems (1 .. 128) that share the patterns of Lxx, gx, hx and the cone layout — sampling MPC, a parameter sweep, a minibatch — stepped through the
 * SAME launches: one analysis, one device copy of its tables, one multifrontal plan with calipso_hip_sparse_set_batch(members); per member its own non-zeros,
 * point, penalty, kappa and work vectors.  Every array below is members x count, member-major (member m's piece at m * count).  Member m's results are, bit for
 * bit, those of a calipso_hip_sparse_kkt on the same data, whatever the group's size and the member's place in it: the kernels call the single handle's arithmetic
 * (csrc/sparse_kkt_kernels.hpp) after shifting their pointers, the member on blockIdx.z through the list of active members.  The host waits of a call are those of
 * its slowest member, not the sum, and its launches do not depend on the number of members.
 *   create          the arguments of calipso_hip_sparse_kkt_create and `members`; anything but 1 .. 128 is CALIPSO_ERR_ARGUMENT naming the argument.  A group needs
 *                   the multifrontal numeric phase (info[4] == 2: method 4); the column method factors a batch one matrix after the other, so on such a plan
 *                   create refuses with a text that names the numeric phase.  Without a HIP device: CALIPSO_ERR_HIP, "no HIP device".
 *   info            info[9] = the eight values of calipso_hip_sparse_kkt_info, then members
 *   pattern         as calipso_hip_sparse_kkt_pattern: triu(K) is the same for every member
 *   set_option      the regularisation and refinement options (options.jl:6-59) by name, shared by the group; "central_path" sets every member's kappa (IC-2,
 *                   inertia.jl:44).  krylov_fallback = 1 is CALIPSO_ERR_ARGUMENT, "not built for groups": there is no `H \ residual` (search_direction.jl:22) in a
 *                   group, a member whose refinement fails gets status 2 and its last refined step — what the single handle does by default.
 *   set_values      as calipso_hip_sparse_kkt_set_values with members x count arrays; penalty and central_path take `members` values (rho and kappa are per
 *                   member).  NULL keeps what is resident.  (_device: device pointers, except central_path, which the host reads.)
 *   factorize       residual_jacobian_variables_symmetric! (residual_jacobian_variables.jl:1-167) + factorize! + compute_inertia! (linear_solver.jl:19-44) of every
 *                   member at ITS (ep[m], ed[m]): one assemble launch into the plan's own value storage, one batched factorisation; inertia = members x 3
 *   get_matrix      K.nzval of `member`'s last assemble
 *   mul             out = H v per member (mul!(e, H, v), iterative_refinement.jl:9,39), each at the regularisation of its last assemble; v, out = members x N
 *   solve_symmetric search_direction_symmetric! (search_direction.jl:25-104) per member with the current factors; residual, step = members x N
 *   search_direction  search_direction! (search_direction.jl:1-23) of every member in lockstep: inertia_correction! (inertia.jl:30-80) round by round over the
 *                   members still walking — one assemble, one batched factorisation, ONE read-back of all their inertias, the verdict per member on that member's
 *                   own scalars; one pre launch, one batched solve, one post launch for all that passed; iterative_refinement! (iterative_refinement.jl:1-52) as
 *                   one fused H v / norm pass over the active members, ONE read-back of the norms, the verdict per member, the correction solve and add for
 *                   those that go on.  regularization (members x 3, in and out), info (members x 4; [3] is 0: no fallback) and status (members) mean per member
 *                   what the single entry's outputs and return value mean.  A member whose inertia correction fails gets CALIPSO_ERR_INERTIA in status, its
 *                   regularisation is where the walk stopped, its step is untouched, and the other members go on.  Returns the worst member status — 0, 2
 *                   (CALIPSO_WARN_REFINEMENT) or CALIPSO_ERR_INERTIA — or CALIPSO_ERR_ARGUMENT / CALIPSO_ERR_HIP, which fail the call.  report[8] = lockstep
 *                   factorisation rounds, lockstep refinement rounds, host waits, kernel launches (this file's, and per batched factorisation / solve one per
 *                   level of the plan's schedule — fronts beyond the LDS take more — and the two permutations), device ms, wall ms, members active in the last
 *                   factorisation round, members active in the last refinement round.  (_device: residual and step are device pointers.)
 *   timing          ms[8] of the last search_direction, HIP events on the plan's stream: [inertia correction, first solve, refinement, 0, 0, wall-clock, the
 *                   three together, 0] */
typedef struct calipso_hip_sparse_kkt_group calipso_hip_sparse_kkt_group;
int32_t calipso_hip_sparse_kkt_group_create(int64_t nx, int64_t ne, int64_t nc, int64_t n_nonnegative, int64_t n_soc, const int64_t* dims, const int64_t* Lxx_colptr,
                                            const int64_t* Lxx_rowval, const int64_t* gx_colptr, const int64_t* gx_rowval, const int64_t* hx_colptr, const int64_t* hx_rowval,
                                            int32_t method, const int64_t* perm, int32_t device, int64_t members, calipso_hip_sparse_kkt_group** out);
int32_t calipso_hip_sparse_kkt_group_destroy(calipso_hip_sparse_kkt_group*);
const char* calipso_hip_sparse_kkt_group_last_error(calipso_hip_sparse_kkt_group*);
int32_t calipso_hip_sparse_kkt_group_info(calipso_hip_sparse_kkt_group*, int64_t info[9]);
int32_t calipso_hip_sparse_kkt_group_pattern(calipso_hip_sparse_kkt_group*, int64_t* colptr, int64_t* rowval);
int32_t calipso_hip_sparse_kkt_group_set_option(calipso_hip_sparse_kkt_group*, const char* name, double value);
int32_t calipso_hip_sparse_kkt_group_set_values(calipso_hip_sparse_kkt_group*, const double* Lxx, const double* gx, const double* hx, const double* w, const double* penalty,
                                                const double* central_path);
int32_t calipso_hip_sparse_kkt_group_set_values_device(calipso_hip_sparse_kkt_group*, const double* Lxx, const double* gx, const double* hx, const double* w, const double* penalty,
                                                       const double* central_path);
int32_t calipso_hip_sparse_kkt_group_factorize(calipso_hip_sparse_kkt_group*, const double* ep, const double* ed, int64_t* inertia);
int32_t calipso_hip_sparse_kkt_group_get_matrix(calipso_hip_sparse_kkt_group*, int64_t member, double* nzval);
int32_t calipso_hip_sparse_kkt_group_mul(calipso_hip_sparse_kkt_group*, const double* v, double* out);
int32_t calipso_hip_sparse_kkt_group_solve_symmetric(calipso_hip_sparse_kkt_group*, const double* residual, double* step);
int32_t calipso_hip_sparse_kkt_group_search_direction(calipso_hip_sparse_kkt_group*, const double* residual, double* step, double* regularization, double* info,
                                                      int32_t* status, double report[8]);
int32_t calipso_hip_sparse_kkt_group_search_direction_device(calipso_hip_sparse_kkt_group*, const double* residual, double* step, double* regularization, double* info,
                                                             int32_t* status, double report[8]);
int32_t calipso_hip_sparse_kkt_group_timing(calipso_hip_sparse_kkt_group*, double ms[8]);

/* ---- solve! on sparse data, for GROUPS of same-pattern conic QPs in lockstep (csrc/sparse_solve_group.hip; host bookkeeping: csrc/sparse_solve_group.hpp) ----------
 * A whole solve! (src/solver/solve.jl:8-377) of the sparse conic QP of calipso_hip_sparse_kkt_qp_attach for every member of a group, device-resident.  Member m's
 * status, counts, scalars, trace and point are, bit for bit, those of calipso_hip_sparse_kkt_solve on the same data with the same options: the kernels call the
 * single handle's arithmetic (csrc/sparse_solve_kernels.hpp) on the single handle's grid after shifting their pointers by the member's strides.  The members'
 * kappa, tau, rho and step sizes live in a member-major device array that one stream-ordered copy fills at the head of every read-back group.
 *   qp_attach       q (members x nx), b (members x ne), hvec (members x nc), member-major, and one objective constant per member (NULL: zeros; a HOST array on both
 *                   routes).  A NULL array of a non-empty block is CALIPSO_ERR_ARGUMENT naming it.  (_device: q, b, hvec are device pointers.)
 *   initialize      initialize! (initialize.jl:9-48) of every member: x0 = members x nx
 *   solve           one tick: every live member is classified from its published prologue (solved members leave with status 1); the members that need an outer
 *                   update get it in one batch with ONE read-back, and are classified again (a member at its outer cap ends with status 0); the others take one
 *                   group search_direction restricted to them; a member whose inertia correction fails ends with CALIPSO_ERR_INERTIA, one whose refinement fails
 *                   with -102 at its last accepted iterate — or, with continue_after_refinement_failure = 1, takes its last refined step; cone masks and the first
 *                   candidate with ONE read-back (a cone search failure ends that member with CALIPSO_ERR_CONE_SEARCH); while any member's filter or line search
 *                   rejects, a further candidate for the rejecting members at their own step sizes, ONE read-back per round; accept, trace row and the next
 *                   prologue with ONE read-back.  A member that has ended is never launched again: its point is its last accepted iterate.  status (members),
 *                   info (members x 16, per member the layout of calipso_hip_sparse_kkt_solve's info; the three times are the group's).  Returns the worst
 *                   (smallest) member status.  report[16] = the eight of search_direction summed over the ticks, then ticks, outer-update rounds, line-search
 *                   trial rounds, host waits (all), launches (all), vector-half device ms, search_direction device ms, wall ms.
 *   get             a resident vector of `member` by the names of calipso_hip_sparse_kkt_get (the twelve vectors of the solver)
 *   solution_device the members' points on the device: members x N
 *   keep_trace      keep the first `rows` accepted iterates of every member;  trace: those of `member` (returns the rows written; *accepted: all it accepted)
 *   set_option      additionally every option solve! reads (include/calipso_options.hpp: set_solve_option, warmstart among them), penalty (every member's resident
 *                   scalar), fraction_to_boundary and continue_after_refinement_failure: shared by the group.  As on the single handle, solve starts every member's
 *                   kappa, tau and rho from the OPTIONS (initialize.jl:38-48: central_path_initial, penalty_initial), so central_path, fraction_to_boundary and
 *                   penalty act on search_direction and the building blocks only, not on solve.  After solve the members' K and factors are of mixed age (they
 *                   left at different ticks): the group holds no current factorisation, factorize or search_direction make one. */
int32_t calipso_hip_sparse_kkt_group_qp_attach(calipso_hip_sparse_kkt_group*, const double* q, const double* b, const double* hvec, const double* objective_constants);
int32_t calipso_hip_sparse_kkt_group_qp_attach_device(calipso_hip_sparse_kkt_group*, const double* q, const double* b, const double* hvec, const double* objective_constants);
int32_t calipso_hip_sparse_kkt_group_initialize(calipso_hip_sparse_kkt_group*, const double* x0);
int32_t calipso_hip_sparse_kkt_group_initialize_device(calipso_hip_sparse_kkt_group*, const double* x0);
int32_t calipso_hip_sparse_kkt_group_solve(calipso_hip_sparse_kkt_group*, int32_t* status, double* info, double report[16]);
int32_t calipso_hip_sparse_kkt_group_get(calipso_hip_sparse_kkt_group*, const char* name, int64_t member, double* out, int64_t len);
int32_t calipso_hip_sparse_kkt_group_solution_device(calipso_hip_sparse_kkt_group*, double** p);
int32_t calipso_hip_sparse_kkt_group_keep_trace(calipso_hip_sparse_kkt_group*, int64_t rows);
int32_t calipso_hip_sparse_kkt_group_trace(calipso_hip_sparse_kkt_group*, int64_t member, double* out, int64_t cap_rows, int64_t* accepted);

/* ---- solve! on sparse problem data resident on the device (csrc/sparse_solve.hip; host pieces: csrc/sparse_solve.hpp) --------------------------------------
 * The vector half of a sparse solve! on the same handle, and the whole solve! (src/solver/solve.jl:8-377) for the problem class that needs no user code, the
 * sparse conic QP   min c x'Px + q'x  s.t.  Ax - b = 0,  h - Gx in K   in the handle's terms: Lxx = c (P + P'), gx = A, hx = -G (set_values), and three more
 * resident vectors q (nx), b (ne), hvec (nc).  evaluate! (evaluate.jl:37-121) is then a gather over the views the handle holds: f = 1/2 x'Lxx x + q'x + constant,
 * fx = Lxx x + q, g = gx x - b, h = hx x + hvec, gx'y, hx'z; Hessian and Jacobians are constant and the dual Hessians zero.  Every vector stays on the device
 * from initialize! to the converged point; sums are reduced in a fixed order, so a solve repeats bit for bit.
 *   qp_attach       q, b, hvec and the objective's constant: host arrays, or (_device) device pointers, checked as in set_values_device.  NULL keeps what is resident.
 *   initialize      initialize!(solver, x0) (initialize.jl:9-48): x <- x0, r <- g(x0), s, t <- the cones' interior points, y, z <- 0.  (_device: x0 on the device.)
 *   solve           solve! whole.  Without the option warmstart it repeats initialize_slacks! / initialize_duals! from the resident x, as calipso_hip_solve does.  The
 *                   decisions are those of csrc/step_decisions.hpp; the linear algebra is search_direction above, on resident vectors; primal_regularization_last
 *                   starts at 0 in every solve.  Returns 1 solved, 0 iteration caps, CALIPSO_ERR_INERTIA, CALIPSO_ERR_CONE_SEARCH, CALIPSO_ERR_ARGUMENT (nothing
 *                   attached, no point), CALIPSO_ERR_HIP — and -100 - CALIPSO_WARN_REFINEMENT where the refinement fails and the reference goes on to `H \ residual`
 *                   (search_direction.jl:22): by default the handle has no such fallback, the point is the last accepted iterate and the handle stays usable.  With
 *                   the option continue_after_refinement_failure = 1 the step search_direction left (the last refined one) is taken, the event counted, and the solve
 *                   goes on.  With the option krylov_fallback = 1 search_direction takes the GMRES fallback above; its step, converged or unconverged but finite, is
 *                   taken, the event counted in the refinement failures and the worst warning as before, and the solve goes on (fallback_info counts them).
 *                   info[16] = total_iterations, outer iterations, accepted iterates, factorisations, most refinement rounds of a step, refinement failures, worst
 *                   warning (CALIPSO_WARN_LINE_SEARCH as calipso_hip_solve reports it), host waits outside search_direction, line-search trials beyond the first
 *                   candidates, central_path and penalty at exit, primal_regularization_last, device ms of the vector half, device ms inside search_direction,
 *                   wall ms, the status.  Host waits: accept is read back together with the next step's prologue, the cone-search masks with the first candidate,
 *                   every further trial once, the prologue behind an outer update once: 2 accepted + outer + trials.
 *   step_prologue   solve.jl:100-135, 170-172 at the solution (which = 0): evaluate!, cone!(barrier, barrier_gradient, product, target), merit and merit_gradient
 *                   (merit.jl:2-31), residual! (residual.jl:1-51), constraint_violation!, the norms of optimality_error.jl:1-27 — central_path as set_option gave it,
 *                   the penalty and the dual as resident.  scalars[16] = f, barrier, merit, constraint violation, residual violation, optimality error, slack
 *                   violation, 0, then |residual|_1, |residual[1:n]|_inf, |residual_y|_inf, |residual_z|_inf, |residual_t|_inf, |y|_1, |z|_1, |t|_1
 *   cone_search     solve.jl:190-221 on the resident step with fraction_to_boundary and max_cone_line_search: a[2] = the step sizes of the cone slacks and of
 *                   their duals, or CALIPSO_ERR_CONE_SEARCH
 *   candidate       solve.jl:206-250: x^, r^, s^ with a_s, t^ with a_t; out[3] = merit and constraint violation at the candidate, merit_gradient . step.primals
 *   accept          solve.jl:309-333 with step size a: violations[2] = |g|_inf, |s o t|_inf
 *   outer_update    solve.jl:362-364: dual <- dual + penalty r
 *   get / set       the resident vectors by their reference names: solution, candidate, dual, residual, merit_gradient, step, cone_product, cone_target,
 *                   barrier_gradient, equality_constraint, cone_constraint, objective_gradient_variables; set takes solution, dual and step (tests, warm starts)
 *   solution_device the resident point (N doubles on the handle's device), synchronised
 *   keep_trace / trace   solution.all after each accepted iterate of a solve, at most `rows` of them kept on the device; trace returns the rows copied (at most
 *                   cap_rows) and, in *accepted, the accepted iterates of the last solve
 *   set_option      additionally every option solve! reads (include/calipso_options.hpp: set_solve_option), fraction_to_boundary, penalty (the resident scalar),
 *                   warmstart, continue_after_refinement_failure */
int32_t calipso_hip_sparse_kkt_qp_attach(calipso_hip_sparse_kkt*, const double* q, const double* b, const double* hvec, double objective_constant);
int32_t calipso_hip_sparse_kkt_qp_attach_device(calipso_hip_sparse_kkt*, const double* q, const double* b, const double* hvec, double objective_constant);
int32_t calipso_hip_sparse_kkt_initialize(calipso_hip_sparse_kkt*, const double* x0);
int32_t calipso_hip_sparse_kkt_initialize_device(calipso_hip_sparse_kkt*, const double* x0);
int32_t calipso_hip_sparse_kkt_solve(calipso_hip_sparse_kkt*, double info[16]);
int32_t calipso_hip_sparse_kkt_step_prologue(calipso_hip_sparse_kkt*, int32_t which, double scalars[16]);
int32_t calipso_hip_sparse_kkt_cone_search(calipso_hip_sparse_kkt*, double a[2]);
int32_t calipso_hip_sparse_kkt_candidate(calipso_hip_sparse_kkt*, double a_s, double a_t, double out[3]);
int32_t calipso_hip_sparse_kkt_accept(calipso_hip_sparse_kkt*, double a, double violations[2]);
int32_t calipso_hip_sparse_kkt_outer_update(calipso_hip_sparse_kkt*);
int32_t calipso_hip_sparse_kkt_get(calipso_hip_sparse_kkt*, const char* name, double* out, int64_t len);
int32_t calipso_hip_sparse_kkt_set(calipso_hip_sparse_kkt*, const char* name, const double* in, int64_t len);
int32_t calipso_hip_sparse_kkt_solution_device(calipso_hip_sparse_kkt*, double** p);
int32_t calipso_hip_sparse_kkt_keep_trace(calipso_hip_sparse_kkt*, int64_t rows);
int32_t calipso_hip_sparse_kkt_trace(calipso_hip_sparse_kkt*, double* out, int64_t cap_rows, int64_t* accepted);

/* ---- solve! on sparse data with an evaluator: the same entries for NONLINEAR problems (csrc/sparse_solve.hip) ----------------------------------------------------
 * With a calipso_device_sparse_eval_fn the kernels above read what the evaluator wrote instead of gathering the QP: fx, g, h and the objective (a device scalar) at the
 * solution, the objective, g, h at a candidate.  gx'y and hx'z are still gathered from the handle's column views; residual, merit, norms and the cones are unchanged.
 * Every evaluator call is an enqueue on the handle's stream: the host waits of solve stay 2 accepted + outer + trials.  With a deterministic evaluator a solve
 * repeats bit for bit.
 *   set_evaluator   fn with its user pointer and the number of parameters np.  Replaces qp_attach, and qp_attach replaces it: a handle holds one problem class.
 *                   fn = NULL removes it.  Lxx, gx, hx need no set_values then: the evaluator writes them.  theta starts as zeros.
 *   set_parameters  theta (np doubles; _device: a device pointer, checked as in set_values_device), resident on the handle
 *   evaluate        the evaluator at the solution (which = 0: into objective, objective_gradient_variables, equality_constraint, cone_constraint) or at the candidate
 *                   (which = 1: x from the candidate, y and z the solution's; the objective and the constraints go to the candidate's own buffers, the gradient and
 *                   the matrices to the only ones there are).  Synchronised.  flags: CALIPSO_EVAL_* without the dual gradients and without any parameter-Jacobian
 *                   bit — those return CALIPSO_ERR_ARGUMENT naming the bit.  An evaluation that writes a matrix invalidates the assembled K and its factor.
 *   get             additionally objective (1 double: the evaluator's at the solution), lagrangian_hessian, equality_jacobian_variables and
 *                   cone_jacobian_variables (the three resident non-zero arrays, on either problem class)
 *   An evaluator's non-zero return r becomes CALIPSO_ERR_ARGUMENT (r = 1) or CALIPSO_ERR_HIP (others) with r in last_error; the handle stays usable.
 *   Where the calls are made: one with every variable-side bit (objective, gradient, constraints, both Jacobians, the Hessian terms — the dual ones iff the option
 *                   constraint_tensor — at the resident y, z) in front of every prologue, standing in for solve.jl:100-135 and :175-185; OBJECTIVE | EQUALITY | CONE at
 *                   every candidate, between the kernel that forms the point and the one that reduces merit and violation; EQUALITY in front of initialize and of
 *                   the accept that starts a solve.
 *   Which point the matrices belong to: after solve returns, the resident Hessian and Jacobians are those of the RETURNED point (the last prologue's evaluation), with
 *                   its y, z — not, as in the reference, those of the last search direction one iterate earlier.  differentiate / differentiate_adjoint therefore
 *                   assemble with the matrices of the returned point and the slacks of quirk B-12 (above); on a QP the matrices are constant and nothing differs.
 *                   The parameter Jacobians of differentiate_parameters / differentiate_adjoint_parameters are evaluated at the same resident point and theta.
 *   set_parameter_patterns  the stored patterns of dR/dtheta's three non-zero blocks (residual_jacobian_parameters.jl:1-40), CSC with np columns, 1-based, rows ascending
 *                   and duplicate-free within a column: Lp = lagrangian_gradient_parameters (nx rows), gp = equality_jacobian_parameters (ne rows), hp =
 *                   cone_jacobian_parameters (nc rows).  Needs an evaluator with np > 0; a pattern that breaks the rule is CALIPSO_ERR_ARGUMENT naming the array.  The
 *                   handle keeps three resident value arrays and device copies of the patterns — no array of size N x np, nx x np, ne x np or nc x np is ever
 *                   allocated.  set_evaluator and qp_attach drop the patterns; a handle without them behaves as it did before they existed.  A later call takes the
 *                   device arrays of an earlier one again where they are large enough; a refused call leaves the patterns there were.
 *   evaluate_parameters  the evaluator with the five parameter bits at the resident x, y, z, theta into the three arrays.  Synchronised.  (evaluate keeps refusing those bits.)
 *   get             additionally lagrangian_gradient_parameters, equality_jacobian_parameters, cone_jacobian_parameters (the resident values on their patterns) */
int32_t calipso_hip_sparse_kkt_set_evaluator(calipso_hip_sparse_kkt*, calipso_device_sparse_eval_fn fn, void* user, int64_t np);
int32_t calipso_hip_sparse_kkt_set_parameters(calipso_hip_sparse_kkt*, const double* theta);
int32_t calipso_hip_sparse_kkt_set_parameters_device(calipso_hip_sparse_kkt*, const double* theta);
int32_t calipso_hip_sparse_kkt_evaluate(calipso_hip_sparse_kkt*, int32_t which, uint32_t flags);
int32_t calipso_hip_sparse_kkt_set_parameter_patterns(calipso_hip_sparse_kkt*, const int64_t* Lp_colptr, const int64_t* Lp_rowval, const int64_t* gp_colptr,
                                                      const int64_t* gp_rowval, const int64_t* hp_colptr, const int64_t* hp_rowval);
int32_t calipso_hip_sparse_kkt_evaluate_parameters(calipso_hip_sparse_kkt*);

/* ---- differentiate! on sparse problem data resident on the device (csrc/sparse_differentiate.hip; host and shared pieces: csrc/sparse_differentiate.hpp) -------
 * differentiate! (src/solver/differentiate.jl:1-61) in both directions on the same handle, for k columns in the launches of one: the condensed solve of
 * search_direction_symmetric! (search_direction.jl:25-104) is the linear map  step = M residual  (residual_symmetric!, K^-1 with K read from one triangle, the
 * recovery of Dr, Ds, Dt), and a "pre" launch, ONE multi-column sparse LDL^T solve and a "post" launch apply M or M' to all columns.  H is the unreduced N x N matrix
 * calipso_hip_sparse_kkt_mul applies; both are taken at the regularisation of the last assemble.  Every sum is a gather in a fixed order: a call repeats bit for bit.
 * Arrays are column-major, N x k; the _device forms take device pointers of the handle's device, checked as in set_values_device.
 *   solve_columns        X = M B (transposed = 0) or M' B with the CURRENT factorisation, as solve_symmetric (search_direction.jl:25-104); no refinement
 *   differentiate        differentiate.jl:13-58 for the caller's dR/dtheta (N x k; the handle has no theta of its own): one assemble + factorisation at the (ep, ed)
 *                        the handle holds, then sensitivity = -M jacobian_parameters (:54-56)
 *   differentiate_adjoint  the same factorisation, then adjoint = lambda = M' cotangent (differentiate.jl:29-58 transposed), and the gradients of a loss with
 *                        dLoss/dw = cotangent with respect to the QP's data: grad = NULL, or six pointers Lxx, q, gx, b, hx, hvec (NULLs skipped), each k x size with
 *                        the matrices ON THEIR STORED PATTERNS in the caller's non-zero order (sizes nnz(Lxx), nx, nnz(gx), ne, nnz(hx), nc).  With x, y, z of the
 *                        resident point and l_x, l_y, l_z the parts of lambda:  Lxx(i, c): -l_x[i] x[c];  q: -l_x;  gx(e, c): -(l_y[e] x[c] + y[e] l_x[c]);  b: +l_y;
 *                        hx(m, c): -(l_z[m] x[c] + z[m] l_x[c]);  hvec: -l_z — one launch, one thread per (stored non-zero, column); no nx x nx array exists anywhere.
 *                        adjoint may be NULL.
 *   differentiate_parameters  differentiate with the EVALUATOR's dR/dtheta (set_parameter_patterns): columns = k 1-based parameter indices (a HOST array in both forms;
 *                        repeats allowed), or NULL for all parameters, and then k = np.  The evaluator is asked for the five parameter bits on the handle's stream; a clear
 *                        and one launch write the N x k block of the selected columns straight into the pass's workspace (x rows from Lx,theta, y rows from g,theta, z rows
 *                        from h,theta, one writer per address); from there on it IS differentiate, so the result is bit for bit what differentiate returns for the same
 *                        block handed in by the caller.  No N x np array exists.
 *   differentiate_adjoint_parameters  differentiate_adjoint with grad = NULL, then grad_theta (np x k, column-major) = -R_theta' lambda:  grad_theta(j, c) =
 *                        -(sum_i Lx,theta(i, j) l_x[i, c] + sum_e g,theta(e, j) l_y[e, c] + sum_m h,theta(m, j) l_z[m, c]), a gather over the three stored columns in stored
 *                        order: one thread per (parameter, cotangent column) for a column of fewer than 64 non-zeros, one wavefront with a fixed-order cross-lane sum
 *                        for a longer one (the split length, csrc/sparse_parameters.hpp: SPLIT_LENGTH, is UNMEASURED).  No floating-point atomics: a call repeats bit for
 *                        bit.  adjoint may be NULL; differentiate_adjoint_times[2] is this kernel's time.
 *                        Both evaluate the parameter Jacobians at the resident point and theta — the point of the resident Hessian and Jacobians (the deviation from
 *                        quirk B-12 described with set_evaluator above); info, times and bytes count these calls as they count the two above.
 *   Option differentiate_refinement = 1 (set_option; default 0, other values CALIPSO_ERR_ARGUMENT): the correction rounds of iterative_refinement.jl:14-44 on all
 *                        columns, forward against H, reverse against H', with the per-column decisions of csrc/sensitivity_columns.hpp; one read-back of k norms per
 *                        round.  On a handle with any second-order cone the option is inert (quirk B-3, as calipso_hip_differentiate): the columns are the unrefined
 *                        map bit for bit and 0 rounds are reported.
 *   The slacks of the cone blocks (quirk B-12): the reference's differentiate! calls no cone!, it works on the cone product Jacobians where the last search direction
 *                        left them, one iterate before the point solve! returns.  calipso_hip_sparse_kkt_solve keeps the s, t its last search_direction was assembled
 *                        at (2 nc doubles, a device-to-device copy on the handle's stream) and the two differentiate entries assemble with those; after set_values
 *                        with w, set("solution") or initialize they are the resident point's own.  get("differentiate_slacks") returns them (2 nc: s, then t).  x, y, z
 *                        of the gradient formulas are always the resident point's.
 *   differentiate_info / differentiate_adjoint_info   [columns, correction rounds (largest over the columns), columns that did not meet the stopping test, largest final
 *                        column norm], as calipso_hip_differentiate_info; differentiate_adjoint_times: HIP-event ms of the last reverse call, [0] entry to last kernel,
 *                        [1] the copies of the results, [2] of [0] the gradient kernel alone, as calipso_hip_differentiate_adjoint_times
 * CALIPSO_ERR_ARGUMENT with calipso_hip_sparse_kkt_last_error naming the argument, the handle usable afterwards: a NULL handle, k < 1, k > 65535 (the multi-column
 * solve's grid limit), a missing array, grad without an attached QP or without a resident point, no values resident (solve_columns: no factorisation); the _parameters
 * entries: no parameter patterns set, a column index outside 1 .. np, columns = NULL with k != np, a NULL sensitivity / grad_theta. */
int32_t calipso_hip_sparse_kkt_solve_columns(calipso_hip_sparse_kkt*, int64_t k, int32_t transposed, const double* B, double* X);
int32_t calipso_hip_sparse_kkt_solve_columns_device(calipso_hip_sparse_kkt*, int64_t k, int32_t transposed, const double* B, double* X);
int32_t calipso_hip_sparse_kkt_differentiate(calipso_hip_sparse_kkt*, int64_t k, const double* jacobian_parameters, double* sensitivity);
int32_t calipso_hip_sparse_kkt_differentiate_device(calipso_hip_sparse_kkt*, int64_t k, const double* jacobian_parameters, double* sensitivity);
int32_t calipso_hip_sparse_kkt_differentiate_adjoint(calipso_hip_sparse_kkt*, int64_t k, const double* cotangent, double* adjoint, double* const* grad);
int32_t calipso_hip_sparse_kkt_differentiate_adjoint_device(calipso_hip_sparse_kkt*, int64_t k, const double* cotangent, double* adjoint, double* const* grad);
int32_t calipso_hip_sparse_kkt_differentiate_parameters(calipso_hip_sparse_kkt*, int64_t k, const int64_t* columns, double* sensitivity);
int32_t calipso_hip_sparse_kkt_differentiate_parameters_device(calipso_hip_sparse_kkt*, int64_t k, const int64_t* columns, double* sensitivity);
int32_t calipso_hip_sparse_kkt_differentiate_adjoint_parameters(calipso_hip_sparse_kkt*, int64_t k, const double* cotangent, double* adjoint, double* grad_theta);
int32_t calipso_hip_sparse_kkt_differentiate_adjoint_parameters_device(calipso_hip_sparse_kkt*, int64_t k, const double* cotangent, double* adjoint, double* grad_theta);
int32_t calipso_hip_sparse_kkt_differentiate_info(calipso_hip_sparse_kkt*, double out[4]);
int32_t calipso_hip_sparse_kkt_differentiate_adjoint_info(calipso_hip_sparse_kkt*, double out[4]);
int32_t calipso_hip_sparse_kkt_differentiate_adjoint_times(calipso_hip_sparse_kkt*, double out[3]);
/* the device bytes the three entries above hold for their columns (the N x k and n x k blocks, the rounds' blocks and masks, the staging of a host call's gradients, the
 * N doubles of the point with the kept slacks): grown on demand, never shrunk, kept — a call that repeats its shapes allocates nothing.  The multi-column LDL^T solve's
 * own right-hand-side buffers (2 n k doubles and its update vectors) belong to the calipso_hip_sparse handle and are not counted */
int32_t calipso_hip_sparse_kkt_differentiate_bytes(calipso_hip_sparse_kkt*, int64_t* out);

/* ---- batched small systems (BASELINE config C5): LDS-resident LDL^T + multi-right-hand-side solve, one workgroup per
 * instance, one launch for the whole batch.  The sensitivity solves of the reference's MPC auto-tuning loop
 * (examples/autotuning/cartpole.jl:179-227 -> differentiate.jl:29-58: n = 89, 102 parameter columns per step) for thousands of
 * independent steps at once; semantics of the LinearSolver seam above (only triu(K) read, no pivoting, natural order).
 *   create(n <= 128, nrhs, batch, device)   set(K[batch][n*n], B[batch][n*nrhs]) column-major host arrays (NULL = keep what is resident)
 *   solve(&ms)   one launch, inputs resident; ms = its HIP-event duration   get(X[batch][n*nrhs], inertia[batch][3]) -> number of
 *   instances with an exact zero pivot (inertia as compute_inertia!, linear_solver.jl:33-44) or a negative status */
typedef struct calipso_hip_small calipso_hip_small;
int32_t calipso_hip_small_create(int64_t n, int64_t nrhs, int64_t batch, int32_t device, calipso_hip_small** out);
int32_t calipso_hip_small_destroy(calipso_hip_small*);
const char* calipso_hip_small_last_error(calipso_hip_small*);
int32_t calipso_hip_small_set(calipso_hip_small*, const double* K, const double* B);
int32_t calipso_hip_small_solve(calipso_hip_small*, double* ms);
int32_t calipso_hip_small_get(calipso_hip_small*, double* X, int64_t* inertia);

/* ---- solve! for a batch of SMALL conic problems, the whole Newton iteration in one kernel (csrc/smallnewton.hip) ------------------------------
 * Solver / initialize! / solve! (src/solver/solver.jl:46-150, initialize.jl:9-48, solve.jl:8-377) for `batch` independent problems of ONE shape that are too small
 * for the general path to be anything but launch latency (the MPC problems of examples/autotuning/cartpole.jl:179-227: n = 89): one workgroup per instance, problem
 * data ([A; -G], q, [-b; h]; the Hessian block stays in L2), iterates and the factor in the compute unit's LDS, every decision of solve.jl:98-368 (exit tests, inertia_correction!, iterative_refinement!, cone search,
 * filter line search, outer updates) on the device, ONE launch per call.  Evaluator: the QP of calipso_hip_qp_attach (min c x'Px + q'x s.t. Ax = b, h - Gx >= 0), or a
 * device evaluator of the caller's (set_evaluator below: nonlinear f, g, h with parameters theta), with nonnegative and second-order cones (dimension <= 16; wider: the general path); residual_norm = constraint_norm = 1.  Points have the layout of point.jl:13-22 (N = nx + 2 ne + 3 nc).  Limits: nx <= 128 and the
 * instance must fit 160 KB of LDS (n up to ~200), else CALIPSO_ERR_ARGUMENT at create: the general path (calipso_hip_create + groups) takes those.
 * Admitted: 1 <= nx <= 128, ne, nc >= 0, cones of dimension 2 .. 16, any footprint up to 160 KB (e.g. (nx, ne, nc) = (128, 63, 0); tests/test_gpu_smallnewton_edges.py
 * finds the last admitted shape from the refusal itself and holds the kernel to the oracle there).
 * Quirk B-13, a DELIBERATE DEPARTURE of this kernel: with ne = nc = 0 the reference's constraint_violation! returns norm(c) / length(c) = 0.0 / 0 = NaN
 * (constraint_violation.jl:13); no comparison of the residual line search holds with it (solve.jl:257-259, line_search.jl:11-12), every iteration halves its step
 * max_residual_line_search = 25 times, moves by 2^-25 of the Newton step, and solve! returns false after max_outer_iterations x max_residual_iterations iterations far
 * from the minimiser.  The oracle and the general path (calipso_hip_solve) keep that behaviour.  This kernel takes the violation of an empty constraint set as 0, so an
 * unconstrained problem takes full Newton steps and converges (status 1; a convex QP: to -(2cP)^-1 q within the tolerances).  Both behaviours are pinned:
 * tests/test_oracle_solve.py (the crawl) and tests/test_gpu_smallnewton_edges.py (the kernel against the closed form, the general path against the oracle).
 *   create(nx, ne, nc, batch, device)        set_option(name, value): options.jl:6-59 by name; plus "threads" = threads per instance (0: chosen by the LDS footprint so that
 *                                            a compute unit holds as many instances as fit; 64, 128 or 256 force a build of the kernel); "lu_fallback" = 0 (default) or 1:
 *                                            where iterative refinement fails, take the reference's `H \ residual` (search_direction.jl:22) inside the kernel — a partially
 *                                            pivoted LU of the unreduced N x N matrix — and go on; costs batch x N^2 doubles of device memory, held while the option is 1
 *   set_qp(P, q, A, b, G, h, c, shared)      column-major host arrays, batch-major (instance k at k * size) or ONE problem for all (shared != 0)
 *   set_state(w, lambda, scalars)            points (batch x N; initialize!: x in the first nx entries), lambda (batch x ne), [central_path, fraction_to_boundary, penalty] (batch x 3)
 *   solve(result, ms)                        solve! of every instance: 1 converged, 0 iteration caps, CALIPSO_ERR_INERTIA / CALIPSO_ERR_CONE_SEARCH (the reference's error()s),
 *                                            -100 - CALIPSO_WARN_REFINEMENT where the reference would fall back to `H \ residual` (search_direction.jl:22: left to the general path;
 *                                            lu_fallback = 0 only), -100 - CALIPSO_WARN_ZERO_PIVOT where that fallback met an exactly singular H (lu_fallback = 1)
 *   steps(count, advance, info, status, ms)  `count` passes of the inner loop body (solve.jl:98-353) from the resident state = calipso_hip_newton_steps for the batch
 *   get_state(w, lambda, scalars, counters)  scalars batch x 6 [central_path, fraction_to_boundary, penalty, primal_regularization, primal_regularization_last, dual_regularization],
 *                                            counters batch x 8 [total_iterations, outer, factorizations, refinement failures, max / last refinement rounds, Newton steps, accepted iterates]
 *   trace(rows, NULL) keeps the first `rows` accepted iterates of every instance (solution.all after solve.jl:309-326); trace(rows, out) reads them (batch x rows x N) */
typedef struct calipso_hip_smallnewton calipso_hip_smallnewton;
int32_t calipso_hip_smallnewton_create(int64_t nx, int64_t ne, int64_t nc, int64_t batch, int32_t device, calipso_hip_smallnewton** out);
int32_t calipso_hip_smallnewton_destroy(calipso_hip_smallnewton*);
const char* calipso_hip_smallnewton_last_error(calipso_hip_smallnewton*);
int32_t calipso_hip_smallnewton_set_option(calipso_hip_smallnewton*, const char* name, double value);
/* cone layout (indices.jl:45-63): the first n_nonnegative cone entries nonnegative (default: all nc), then n_soc second-order cones of dims[j] (2 .. 16) entries each, contiguous */
int32_t calipso_hip_smallnewton_set_cones(calipso_hip_smallnewton*, int64_t n_nonnegative, int64_t n_soc, const int64_t* dims);
int32_t calipso_hip_smallnewton_set_qp(calipso_hip_smallnewton*, const double* P, const double* q, const double* A, const double* b, const double* G, const double* h,
                                       double objective_scale, int32_t shared);
int32_t calipso_hip_smallnewton_set_state(calipso_hip_smallnewton*, const double* w, const double* lambda, const double* scalars);
int32_t calipso_hip_smallnewton_get_state(calipso_hip_smallnewton*, double* w, double* lambda, double* scalars, int64_t* counters);
int32_t calipso_hip_smallnewton_trace(calipso_hip_smallnewton*, int32_t rows, double* out);
int32_t calipso_hip_smallnewton_solve(calipso_hip_smallnewton*, int32_t* result, double* ms);
int32_t calipso_hip_smallnewton_steps(calipso_hip_smallnewton*, int32_t count, int32_t advance, double* info, int32_t* status, double* ms);
/* differentiate!(solver)  differentiate.jl:1-61 for every instance in ONE launch, at the resident points (after calipso_hip_smallnewton_solve): the condensed matrix
 * with the regularisation solve! left is factored once (:13-20), then search_direction_symmetric! per column of dR/dtheta (:29-52) and sensitivity = -1.0 * the
 * result (:55-57).  jacobian_parameters (residual_jacobian_parameters.jl:1-40: the caller's model; constant for the parametric QPs of an MPC loop,
 * examples/autotuning/cartpole.jl:179-227): batch x (N x p) doubles on the host, column-major per instance — or ONE N x p matrix for all instances (shared != 0) —,
 * N = nx + 2 ne + 3 nc in the order of point.jl; sensitivity: batch x (N x p).  Batches without second-order cones refine every column (iterative_refinement.jl:1-52:
 * the condensed solve is five digits short of the reference's QDLDL at a solution); with second-order cones the unrefined solve IS the reference's result (quirk B-3).
 * The cone Jacobians are those of the last search direction, as the reference's fields are (quirk B-12).  status[k] = 0, or 1 when the inertia of the factorisation is not (nx, ne + nc, 0) (the reference does not look). */
int32_t calipso_hip_smallnewton_differentiate(calipso_hip_smallnewton*, int64_t p, int32_t shared, const double* jacobian_parameters, double* sensitivity, int32_t* status, double* ms);
/* Nonlinear problems: a DEVICE EVALUATOR compiled into the caller's own HIP library against include/calipso_smallnewton.hpp (HIP C++; INTEGRATION.md "Writing an
 * evaluator for the batched kernel").  The evaluator is a C++ type whose workgroup-cooperative hooks give f and [g; h] at a point (evaluate!, solve.jl:78,231,278), fx,
 * [gx; hx] and the Lagrangian Hessian fxx + (y'g)xx + (z'h)xx at the solution (solve.jl:100,175; differentiate.jl:3) and, optionally, dR/dtheta
 * (residual_jacobian_parameters.jl:1-40).  CALIPSO_SMALLNEWTON_EVALUATOR(Type, symbol) instantiates every build of the kernels for that type in the caller's code
 * object and emits  extern "C" int32_t symbol(const calipso_smallnewton_launch*): the library asks it for its ABI version, sizeof(Args), SN_JB and whether it
 * provides dR/dtheta, has it grant the LDS, and has it launch the right build on the handle's stream (as a calipso_device_eval_fn enqueues on the stream it is given).
 *   set_evaluator(fn, n_parameters)          checks the handshake (a mismatch: CALIPSO_ERR_ARGUMENT and a message), allocates the per-instance Hessians (batch x nx^2
 *                                            doubles: the message states the bytes when that fails); replaces set_qp, as set_qp replaces it; solve / steps /
 *                                            differentiate need one of the two.  The cone layout, options and state calls are the same for both.
 *   set_parameters(theta, shared)            theta: batch x n_parameters (row k for instance k) or ONE n_parameters vector for all (shared != 0); required before a
 *                                            launch when n_parameters > 0
 *   differentiate_parameters(sens, status, ms)  differentiate! with dR/dtheta from the evaluator at the resident points (p = n_parameters): sensitivity batch x (N x p)
 *                                            as calipso_hip_smallnewton_differentiate, which keeps taking a caller-given dR/dtheta under an evaluator too
 *   differentiate! takes [gx; hx] and the Hessian where the last search direction evaluated them (the iterate before the final one, as the cone Jacobians:
 *   quirk B-12) and dR/dtheta at the solution, as the reference does.  calipso_hip_debug_smallnewton_describe answers for the evaluator's build of the kernel (its entry's occupancy query). */
#define CALIPSO_SMALLNEWTON_ABI 1
enum { CALIPSO_SMALLNEWTON_QUERY = 0, CALIPSO_SMALLNEWTON_GRANT_LDS = 1, CALIPSO_SMALLNEWTON_OCCUPANCY = 2, CALIPSO_SMALLNEWTON_LAUNCH = 3 };
typedef struct calipso_smallnewton_launch {
    int32_t op;                 /* CALIPSO_SMALLNEWTON_QUERY / _GRANT_LDS / _OCCUPANCY / _LAUNCH */
    int32_t abi;                /* CALIPSO_SMALLNEWTON_ABI of the library that asks */
    int64_t* out;               /* QUERY: out[5] = {ABI, sizeof(Args), SN_JB, 1 if dR/dtheta is provided, 1 if the reverse mode is built} (the library pre-zeroes five
                                   entries: an entry built before the reverse mode leaves out[4] = 0); OCCUPANCY: out[0] = instances a compute unit holds */
    const void* args;           /* LAUNCH: the kernels' argument block (calipso::sn::Args) */
    int64_t args_bytes;         /* its size, sizeof(Args) of the library */
    int32_t mode;               /* 0 solve!, 1 Newton steps, 2 differentiate!, 3 its reverse mode (args: calipso::sn::AdjArgs, which begins with Args) */
    int32_t threads;            /* threads per instance: 64, 128 or 256 */
    int32_t soc, lu;            /* second-order cones in the layout; the lu_fallback build */
    int32_t eval_rtheta;        /* differentiate!: dR/dtheta from the evaluator */
    int32_t reserved;
    int64_t grid;               /* instances = workgroups */
    int64_t lds_bytes;          /* dynamic LDS per workgroup (GRANT_LDS: the size to grant) */
    void* stream;               /* hipStream_t to launch on */
} calipso_smallnewton_launch;
typedef int32_t (*calipso_smallnewton_kernels_fn)(const calipso_smallnewton_launch*);
int32_t calipso_hip_smallnewton_set_evaluator(calipso_hip_smallnewton*, calipso_smallnewton_kernels_fn fn, int64_t n_parameters);
int32_t calipso_hip_smallnewton_set_parameters(calipso_hip_smallnewton*, const double* theta, int32_t shared);
int32_t calipso_hip_smallnewton_differentiate_parameters(calipso_hip_smallnewton*, double* sensitivity, int32_t* status, double* ms);
/* differentiate! in REVERSE mode (differentiate.jl:1-61 and residual_jacobian_parameters.jl:1-40, transposed) for every instance in ONE launch, at the resident
 * points: the factorisation of differentiate above, then for each of k cotangent columns v = dLoss/dw the transposed map lambda = M' v of the map M that
 * differentiate applies to a column (search_direction_symmetric! stage by stage in reverse order; batches without second-order cones refine against H' as the
 * forward columns refine against H, with the same options; with second-order cones neither refines, quirk B-3), then the contractions with dR/dtheta in the same
 * launch: grad = -R_theta' lambda = S' v for the S = dw/dtheta that differentiate would return — one solve per cotangent instead of one per parameter.  The cone
 * Jacobians, [gx; hx] and the Hessian are those of the last search direction (quirk B-12), as for differentiate.
 *   cotangent   batch x (N x k), column-major per instance (required)
 *   adjoint     batch x (N x k) = lambda (NULL: not returned)
 *   grad_theta  batch x (n_parameters x k): -R_theta' lambda with the evaluator's dR/dtheta at the resident points (NULL: skipped; needs an evaluator that provides it)
 *   grad_qp     batch x (nqp x k), nqp = nx^2 + nx + ne nx + ne + nc nx + nc: the built-in QP's data gradients in set_qp's column-major block order P, q, A, b, G, h
 *               (P's gradient symmetric, P taken symmetric) per instance even for shared data — summing is the caller's (NULL: skipped; the QP only)
 *   status[k] as differentiate.  CALIPSO_ERR_ARGUMENT with last_error for k < 1, no cotangent, no problem data, grad_theta without an evaluator providing dR/dtheta
 *   (or with no parameters), grad_qp under an evaluator, and an evaluator entry that does not report the reverse mode (QUERY's out[4] stays 0: built before it) */
int32_t calipso_hip_smallnewton_differentiate_adjoint(calipso_hip_smallnewton*, int64_t k, const double* cotangent, double* adjoint, double* grad_theta, double* grad_qp,
                                                      int32_t* status, double* ms);
/* DEVICE-RESIDENT, STREAM-ORDERED twins of the data entries above (csrc/smallnewton_io.hip; INTEGRATION.md "The batch kernel on device tensors").  Every pointer
 * is DEVICE memory on the handle's device; the work is enqueued on the handle's stream; NO entry waits for the device, none reports `ms`, and nothing is read back:
 * the results are valid in stream order.  Each entry checks, before it enqueues anything, that every non-NULL pointer is device memory of the handle's device
 * (hipPointerGetAttributes): a host or foreign pointer is CALIPSO_ERR_ARGUMENT with a message naming the argument.  The host entries above keep working on the
 * same handle, on whatever stream it has, and still wait for their own work.  The launches are those of solve / differentiate_adjoint: k_smallnewton and
 * k_smallnewton_adj, unchanged; small kernels pack and unpack around them.  Buffers grow on demand and are kept: a call that repeats its shapes allocates nothing
 * (hipFree waits for the whole device).  One HIP runtime per process: with PyTorch, `import torch` first.
 *   set_stream(hip_stream, borrow)           borrow != 0: all later work of the handle goes to the caller's hipStream_t (torch.cuda.current_stream().cuda_stream;
 *                                            NULL = the legacy default stream, which is torch's default stream); borrow == 0: back to the handle's own stream.  The
 *                                            new stream first waits ON THE DEVICE for what the old one holds (an event recorded on the old stream).  A borrowed
 *                                            stream is not owned and is never destroyed by the handle: the caller must take the handle off it — set_stream(NULL, 0)
 *                                            or set_stream(another, 1) — BEFORE destroying it; the handle touches the old stream once more in that call (and
 *                                            destroy waits for the stream it holds).  The evaluator's entry already launches on the stream it is handed.
 *   set_qp_device(P, q, A, b, G, h, c, shared_mask, row_major)
 *                                            bit i of shared_mask: array i of P, q, A, b, G, h is ONE array for all instances, else batch-major; row_major != 0:
 *                                            matrices (rows, cols) row-major, as torch lays them out, else column-major as set_qp.  The pack kernel that set_qp
 *                                            goes through as well writes Lxx = (2c) P, Z = [A; -G] (ld m, column-major), bh = [-b; h]: the same bits from both
 *                                            entries.  P and q are stored once when shared; Z once only when A and G are both shared or absent, bh likewise
 *                                            for b and h — otherwise the shared half is repeated into per-instance storage.  Replaces an evaluator as set_qp does
 *                                            (that one case frees the evaluator's buffers and waits).
 *   initialize_device(x0)                    initialize!: x0 (batch x nx; NULL: zeros) into the first nx entries of every point, zeros behind
 *   set_state_device(w, lambda, scalars)     the layouts of set_state; one kernel copies w and lambda and scatters the three scalars into their slots
 *   set_parameters_device(theta, shared)     theta copied device to device into the handle's buffer (kept while the size repeats)
 *   solve_device()                           the launch of solve: no events, no wait; the statuses stay on the device
 *   get_solution_device(x, y, z, w, status)  one kernel gathers x (batch x nx), y (batch x ne), z (batch x nc) out of the points, optionally the points (batch x N)
 *                                            and the int32 status of the handle's last SOLVE (host or device; kept apart from the status a differentiate leaves); NULLs skipped
 *   differentiate_adjoint_device(k, cot_w, cot_x, cot_y, cot_z, adjoint, grad_theta, grad_qp, reduce_mask, row_major, status)
 *                                            the launch of differentiate_adjoint.  The cotangent is cot_w, batch x (N x k), which the kernel reads where it lies — or,
 *                                            with cot_w NULL, the parts cot_x / cot_y / cot_z (batch x (nx | ne | nc) x k, column-major per instance, each may be
 *                                            NULL), scattered into the N-layout with zeros elsewhere.  adjoint (batch x (N x k)) and grad_theta (batch x
 *                                            (n_parameters x k)) are written by the launch straight into the caller's buffers.  grad_qp: NULL or SIX pointers in the
 *                                            order P, q, A, b, G, h (NULLs skipped).  Without bit i of reduce_mask array i's gradient comes per instance, batch x k x
 *                                            size_i (a matrix row-major when row_major != 0, else column-major); with bit i it is SUMMED OVER THE BATCH on the
 *                                            device, k x size_i.  The sum is deterministic and free of atomics: the batch is cut into chunks of 64 instances
 *                                            (whatever the grid or the device), a chunk is added in instance order, the chunks in chunk order.  Every gradient
 *                                            (grad_qp and grad_theta) of an instance whose last solve status is not 1 is NaN, before any sum.  status (batch, int32)
 *                                            as differentiate_adjoint.  The refusals of differentiate_adjoint apply, with its messages.
 *   For tests (exported, not declared, like calipso_hip_debug_smallnewton_describe): calipso_hip_debug_smallnewton_buffers(s, int64_t out[8]) = the device
 *   addresses of Lxx, q, Z, bh and their element strides per instance (0: stored once) — a repeated set_qp_device must leave all eight as they were. */
int32_t calipso_hip_smallnewton_set_stream(calipso_hip_smallnewton*, void* hip_stream, int32_t borrow);
int32_t calipso_hip_smallnewton_set_qp_device(calipso_hip_smallnewton*, const double* P, const double* q, const double* A, const double* b, const double* G, const double* h,
                                              double objective_scale, int32_t shared_mask, int32_t row_major);
int32_t calipso_hip_smallnewton_initialize_device(calipso_hip_smallnewton*, const double* x0);
int32_t calipso_hip_smallnewton_set_state_device(calipso_hip_smallnewton*, const double* w, const double* lambda, const double* scalars);
int32_t calipso_hip_smallnewton_set_parameters_device(calipso_hip_smallnewton*, const double* theta, int32_t shared);
int32_t calipso_hip_smallnewton_solve_device(calipso_hip_smallnewton*);
int32_t calipso_hip_smallnewton_get_solution_device(calipso_hip_smallnewton*, double* x, double* y, double* z, double* w, int32_t* status);
int32_t calipso_hip_smallnewton_differentiate_adjoint_device(calipso_hip_smallnewton*, int64_t k, const double* cot_w, const double* cot_x, const double* cot_y, const double* cot_z,
                                                             double* adjoint, double* grad_theta, double* const* grad_qp, int32_t reduce_mask, int32_t row_major, int32_t* status);

/* ---- multi-GPU exchange of the batched path: RCCL over xGMI, one process per GPU ---------------------------------
 * Problem instances are sharded block-contiguously over ranks and never interact (the reference's `Solver`s are independent); the
 * only exchange is after a batch round: all-gather of per-problem status rows, all-reduce of counters.  RCCL is dlopen'ed on first
 * use.  calipso_hip_comm_unique_id = ncclGetUniqueId (one rank), calipso_hip_comm_init = ncclCommInitRank (all ranks, same id). */
typedef struct calipso_hip_comm calipso_hip_comm;
int32_t calipso_hip_comm_unique_id(uint8_t id[128]);
int32_t calipso_hip_comm_init(int32_t rank, int32_t nranks, const uint8_t id[128], int32_t device, calipso_hip_comm** out);
int32_t calipso_hip_comm_destroy(calipso_hip_comm*);
/* out[0] = ncclCommCount, out[1] = ncclCommUserRank of the live communicator (what RCCL itself reports: the self-check of a multi-GPU run) */
int32_t calipso_hip_comm_size(calipso_hip_comm*, int32_t out[2]);
const char* calipso_hip_comm_last_error(calipso_hip_comm*);
/* rows: n_rows x 4 int32 of this rank (row counts may differ between ranks); all_rows: capacity cap_rows rows, filled in global
 * problem-id order; counts_out[nranks] (may be NULL) = rows per rank.  Returns the total row count or a negative status. */
int64_t calipso_hip_comm_gather_status(calipso_hip_comm*, const int32_t* rows, int64_t n_rows, int32_t* all_rows, int64_t cap_rows,
                                       int64_t* counts_out);
int32_t calipso_hip_comm_allreduce_sum(calipso_hip_comm*, double* values, int64_t count);

/* measured fp64 matrix-core ceiling (TFLOP/s) of `device`: back-to-back independent v_mfma_f64_16x16x4_f64, 8 wavefronts per SIMD
 * (a few milliseconds).  bench.py reports it as roofline.peak_measured next to the datasheet peak. */
int32_t calipso_hip_mfma_f64_peak(int32_t device, double* tflops);

/* timing of the last calipso_hip_newton_step / factorisation, in milliseconds, from HIP events on the handle's stream:
 * [0] evaluate + cone + residual + reductions   [1] cone pivots + Omega*hx   [2] search_direction! total (factor + solves + refinement)
 * [3] LDL^T of the Schur complement   [5] cone search + line search + accept   [6] whole step
 * [7] the Schur-complement MFMA kernel (k_schur), last launch   [8] number of factorisations timed so far */
int32_t calipso_hip_phase_times(calipso_hip_solver*, double out[9]);
/* per-kernel figures of the last factorisation and the handle's layout (bench.py: the live launch durations behind `roofline`):
 * [0] ms of the panel-step launches of the LDL^T of the Schur complement (k_ldl_diag + k_ldl_step: the pivot chain, one launch per 64
 *     pivots; HIP events around exactly these launches; the rest of [3] above is the parallel finish: factor columns + block inverses)
 * [1] number of those launches   [2] NP = padded order of the Schur complement   [3] bytes of the handle's device slab + the dense scratch a structured handle
 *     allocates for a calipso_device_eval_fn (none with a calipso_device_block_eval_fn)
 * [4] ms of ONE launch of the refinement residual's mat-vec kernel (k_gemv_t2_and_n: [gx; hx]' times two vectors and Lxx times one, the first residual of the
 *     last calipso_hip_newton_step; 0 when the handle takes another path) and [5] the bytes it reads, 8 (m nx + nx^2)
 * [6] 1 when the last factorisation took the left-looking schedule of one dense system (csrc/lfac.hip: the products of the Schur complement as slices of the panel
 *     launches — [0] / [1] then cover k_lfac's launches, Schur complement included, and phase [7] of calipso_hip_phase_times is ~0)   [7] bytes of that schedule's
 *     buffers outside the slab (Z = A M of every panel, the factor columns, the launch plan) */
int32_t calipso_hip_kernel_times(calipso_hip_solver*, double out[8]);
/* work of one Newton step on a handle that exploits its stage structure (src/trajectory_optimization/sparsity.jl:28-129 is where the reference's structure
 * comes from): [0] flops of the Schur complement by segment pairs (k_schur_blocks)   [1] doubles of the packed blocks of [gx; hx] and Lxx (both orientations)
 * [2] segment pairs   [3] flops of one multifrontal LDL^T of S   [4] nnz(L) of its fronts   [5] order of S   [6] 1 for a structured handle   [7] reserved */
int32_t calipso_hip_structure_work(calipso_hip_solver*, double out[8]);
/* which schedule the handle's Newton steps took: [0] steps so far whose prologue (gradients, barrier, merit + gradient, residual, norms: solve.jl:100-135) ran on
 * the handle's second stream beside the factorisation instead of in front of it (a single handle that queues the step ahead; CALIPSO_HIP_PROLOGUE_AHEAD=0: never)
 * [1] where the last step's went: 0 main stream, 1 forked at the start of the step, 2 handed over while the pivot chain runs   [2] factorisations queued ahead of an exit
 * test that held after all (their traces were undone)   [3] reserved */
int32_t calipso_hip_schedule_info(calipso_hip_solver*, double out[4]);
/* The cache of the Schur complement's equality products (calipso_hip_qp_attach): factorisations so far that [0] stored the products (capture), [1] started from the
 * stored ones (hit), [2] could have used the cache and went without (bypass: another regularisation than the initial one)   [3] bytes of the buffer.  All zero on a
 * handle without the cache ("opt.schur_cache" = 0, no attached QP, ne = 0, a member stepped by its group, padded nx < 1024, structured handles). */
int32_t calipso_hip_schur_cache_info(calipso_hip_solver*, double out[4]);
int32_t calipso_hip_synchronize(calipso_hip_solver*);
/* Independent Solvers stepped from different host threads (solver.jl:46-150: the reference's Solvers are independent objects; batch.py: lanes) overlap on the GPU only
 * if the runtime put their streams behind different hardware dispatchers — which depends on the order in which the process created its streams and cannot be queried.
 * calipso_hip_streams_concurrent MEASURES it (a kernel of many more workgroups than the chip holds on one stream, a one-workgroup kernel on the other, both ways):
 * out[1], out[2] = the short kernel's time behind a's / b's long kernel (us), out[3] = the long kernel's duration (us) — and chains of 48 short kernels on both streams at
 * once against one chain alone (out[4], out[5], us: two streams of the highest priority class pass the first test and still run their chains one after the other);
 * out[0] = 1 if the streams run side by side by both tests, else 0.  calipso_hip_rebind_stream gives the handle a NEW stream (the old one is drained and destroyed; priority_class
 * 0, 1, 2 = the classes calipso_hip_create deals out by creation order, -1 = keep): the runtime binds it to the least used hardware queue of the class.  The Python
 * mirror's BatchSolver (and the Julia module's lanes) probe the leaders of their lanes at creation and rebind until every pair runs side by side. */
int32_t calipso_hip_streams_concurrent(calipso_hip_solver* a, calipso_hip_solver* b, double out[6]);
int32_t calipso_hip_rebind_stream(calipso_hip_solver*, int32_t priority_class);

/* SplitMix64 uniform stream of SURVEY.md 8(d): seed = 0xCA11B50000000000 + 4096*problem_id + stream_id,
 * u = (next() >> 11) * 2^-53, out[i] = lo + (hi-lo)*u.  Pure host function. */
int32_t calipso_hip_splitmix_uniform(uint64_t problem_id, uint64_t stream_id, double lo, double hi, int64_t count, double* out);

#ifdef __cplusplus
}
#endif
#endif
