# CalipsoHIP.jl — Julia host layer over libcalipso_hip.so (include/calipso_hip.h).
#
# Keeps the reference's surface for the Newton/KKT hot path (CALIPSO.jl v0.1.1):
#     Solver(...)  ->  HIPSolver(solver::CALIPSO.Solver)      wraps an ordinary CALIPSO.Solver (its codegen'd methods,
#                                                            ProblemData, Indices, Options are reused unchanged)
#     initialize!(hs, x0)            src/solver/initialize.jl:9-13
#     solve!(hs)::Bool               src/solver/solve.jl:8-377   — the whole loop runs in the library; Julia only evaluates the
#                                                                  user functions (evaluate!) when the library calls back
#     HIPLDLSolver <: LinearSolver   src/solver/linear_solver.jl:1-60 seam: factorize!(s, A), compute_inertia!(s), linear_solve!(s, x, A, b) on
#                                    the device for the sparse K the reference assembles itself (calipso_hip_ldl_*)
#
# NOTE: Julia is not installed in the build container of this repository, so this file has not been executed there; it is the
# binding a maintainer adds (see INTEGRATION.md).  The same C ABI is exercised end-to-end by the Python ctypes mirror
# (calipso.jl_amd/__init__.py) in tests/.
module CalipsoHIP

using CALIPSO
import Libdl
using LinearAlgebra
using SparseArrays

const lib = get(ENV, "CALIPSO_HIP_LIB", joinpath(@__DIR__, "..", "libcalipso_hip.so"))

# evaluate! flags (include/calipso_hip.h)
const EVAL_OBJECTIVE = UInt32(1) << 0
const EVAL_OBJECTIVE_GRADIENT = UInt32(1) << 1
const EVAL_OBJECTIVE_HESSIAN = UInt32(1) << 2
const EVAL_EQUALITY = UInt32(1) << 3
const EVAL_EQUALITY_JACOBIAN = UInt32(1) << 4
const EVAL_EQUALITY_DUAL_GRADIENT = UInt32(1) << 5
const EVAL_EQUALITY_DUAL_HESSIAN = UInt32(1) << 6
const EVAL_CONE = UInt32(1) << 7
const EVAL_CONE_JACOBIAN = UInt32(1) << 8
const EVAL_CONE_DUAL_GRADIENT = UInt32(1) << 9
const EVAL_CONE_DUAL_HESSIAN = UInt32(1) << 10
const EVAL_OBJECTIVE_JACOBIAN_PARAMETERS = UInt32(1) << 11
const EVAL_EQUALITY_JACOBIAN_PARAMETERS = UInt32(1) << 12
const EVAL_EQUALITY_DUAL_JACOBIAN_PARAMETERS = UInt32(1) << 13
const EVAL_CONE_JACOBIAN_PARAMETERS = UInt32(1) << 14
const EVAL_CONE_DUAL_JACOBIAN_PARAMETERS = UInt32(1) << 15

struct HIPError <: Exception
    code::Int32
    msg::String
end

mutable struct HIPSolver
    handle::Ptr{Cvoid}
    solver::CALIPSO.Solver          # the reference Solver: methods, problem (ProblemData), indices, options, parameters
    eval_cfunction::Base.CFunction  # keeps the @cfunction alive
end

last_error(h) = unsafe_string(ccall((:calipso_hip_last_error, lib), Cstring, (Ptr{Cvoid},), h))

function check(h, rc::Integer, what)
    rc == -1 && error("inertia correction failure")    # same text as src/solver/inertia.jl:72
    rc == -2 && error("cone search failure")           # src/solver/solve.jl:210,220
    rc < 0 && throw(HIPError(Int32(rc), "$what: $(last_error(h))"))
    rc == 1 && @warn "Zero entry in D (matrix is not quasidefinite)"     # src/solver/qdldl.jl:309-311
    rc == 2 && @warn "iterative refinement failure"                       # src/solver/iterative_refinement.jl:50
    return rc
end

set_field!(h, name::String, v::AbstractArray{Float64}) =
    check(h, ccall((:calipso_hip_set_field, lib), Int32, (Ptr{Cvoid}, Cstring, Ptr{Float64}, Int64), h, name, v, length(v)), "set_field($name)")
set_field!(h, name::String, v::Real) = set_field!(h, name, [Float64(v)])
function get_field(h, name::String, len::Integer)
    out = zeros(len)
    check(h, ccall((:calipso_hip_get_field, lib), Int32, (Ptr{Cvoid}, Cstring, Ptr{Float64}, Int64), h, name, out, len), "get_field($name)")
    return out
end

"""
    HIPSolver(solver::CALIPSO.Solver; device=0)

Create the device handle for an existing reference `Solver` (src/solver/solver.jl:46-150).  Index sets are passed 1-based,
exactly as `solver.indices` holds them.
"""
# structure = (row_first, row_last, hessian_block_start) (1-based Int vectors) makes a STRUCTURED handle (calipso_hip_create_structured): only the stage
# blocks of the problem live on the device.  `declared_structure(solver)` reads it off the methods' sparsity lists.
function HIPSolver(solver::CALIPSO.Solver; device::Integer=0, structure=nothing)
    d = solver.dimensions
    idx = solver.indices
    nn = Vector{Int64}(idx.cone_nonnegative)
    soc = idx.cone_second_order
    ptr = Int64[0]
    flat = Int64[]
    for c in soc
        append!(flat, c)
        push!(ptr, length(flat))
    end
    href = Ref{Ptr{Cvoid}}(C_NULL)
    rc = if structure === nothing
        ccall((:calipso_hip_create, lib), Int32,
            (Int64, Int64, Int64, Int64, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Int64}, Int32, Ptr{Ptr{Cvoid}}),
            d.variables, d.parameters, d.equality_dual, d.cone_dual, length(nn), nn, length(soc), ptr, flat, device, href)
    else
        rf, rl, hb = Vector{Int64}(structure[1]), Vector{Int64}(structure[2]), Vector{Int64}(structure[3])
        ccall((:calipso_hip_create_structured, lib), Int32,
            (Int64, Int64, Int64, Int64, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Int64}, Int32, Ptr{Int64}, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Ptr{Cvoid}}),
            d.variables, d.parameters, d.equality_dual, d.cone_dual, length(nn), nn, length(soc), ptr, flat, device, rf, rl, length(hb), hb, href)
    end
    if rc != 0 && structure !== nothing
        # the declared structure has nothing for the block path to exploit (one Hessian block: e.g. dynamics whose y'f Hessian couples x_t with x_{t+1}, src/
        # trajectory_optimization/dynamics.jl:245-259): a dense handle instead, whose banded / stage-parallel treatment calipso_hip_analyze_structure can still turn on
        @warn "calipso_hip_create_structured refused the declared structure ($(last_error(C_NULL))); falling back to a dense handle"
        rc = ccall((:calipso_hip_create, lib), Int32,
            (Int64, Int64, Int64, Int64, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Int64}, Int32, Ptr{Ptr{Cvoid}}),
            d.variables, d.parameters, d.equality_dual, d.cone_dual, length(nn), nn, length(soc), ptr, flat, device, href)
    end
    rc != 0 && throw(HIPError(rc, "calipso_hip_create: $(last_error(href[]))"))
    hs = HIPSolver(href[], solver, @cfunction($(evaluate_callback), Int32, (Ptr{Cvoid}, UInt32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64})))
    finalizer(x -> ccall((:calipso_hip_destroy, lib), Int32, (Ptr{Cvoid},), x.handle), hs)
    # options (src/solver/options.jl:6-59) -> handle
    for f in fieldnames(typeof(solver.options))
        v = getfield(solver.options, f)
        v isa Real && f != :linear_solver && ccall((:calipso_hip_set_field, lib), Int32, (Ptr{Cvoid}, Cstring, Ptr{Float64}, Int64), hs.handle, "opt.$f", [Float64(v)], 1)
    end
    length(solver.parameters) > 0 && set_field!(hs.handle, "parameters", solver.parameters)
    return hs
end

# The structure of a solver whose methods carry sparsity lists (src/solver/methods.jl; every trajectory problem): per row of [equality; cone] the extrema of
# the columns in the Jacobian lists, and the diagonal blocks of the three Hessian lists (a new block starts where no listed entry couples to an earlier column).
function declared_structure(solver::CALIPSO.Solver)
    d = solver.dimensions; m = solver.methods
    ne, nc, nx = d.equality_dual, d.cone_dual, d.variables
    rf = fill(1, ne + nc); rl = fill(0, ne + nc); seen = falses(ne + nc)
    for (off, list) in ((0, m.equality_jacobian_variables_sparsity), (ne, m.cone_jacobian_variables_sparsity)), (i, j) in list
        k = off + i
        rf[k] = seen[k] ? min(rf[k], j) : j; rl[k] = seen[k] ? max(rl[k], j) : j; seen[k] = true
    end
    reach = collect(1:nx)
    for list in (m.objective_jacobian_variables_variables_sparsity, m.equality_dual_jacobian_variables_variables_sparsity, m.cone_dual_jacobian_variables_variables_sparsity), (i, j) in list
        lo, hi = minmax(i, j); reach[lo] = max(reach[lo], hi)
    end
    starts = Int64[1]; r = 0
    for j in 1:nx
        j > starts[end] && r < j && push!(starts, j)
        r = max(r, reach[j])
    end
    return (rf, rl, starts)
end

const ACTIVE = Ref{Union{Nothing,HIPSolver}}(nothing)   # fallback for callers that pass user = C_NULL to the C drivers

# evaluate!(problem, methods, idx, point, parameters; <flags>)  (src/solver/evaluate.jl:1-124) at the point the library hands
# over, then upload of the flagged ProblemData fields (the three Hessian terms as one summed "lagrangian_hessian",
# src/solver/residual_jacobian_variables.jl:10-16).
function evaluate_callback(user::Ptr{Cvoid}, flags::UInt32, px::Ptr{Float64}, py::Ptr{Float64}, pz::Ptr{Float64}, pth::Ptr{Float64})::Int32
    # No exception may unwind through the @cfunction frame into C: everything, including the lookup of the solver, is inside `try`.
    try
        # `user` = pointer_from_objref(hs) as passed to calipso_hip_solve / calipso_hip_group_set_evaluators (the caller keeps `hs`
        # rooted with GC.@preserve for the duration of the ccall); ACTIVE[] serves callers that passed C_NULL
        hs = user != C_NULL ? (unsafe_pointer_to_objref(user)::HIPSolver) : (ACTIVE[]::HIPSolver)
        s = hs.solver
        d = s.dimensions
        pt = s.candidate                      # scratch Point the generated functions read from
        pt.variables .= unsafe_wrap(Array, px, d.variables)
        d.equality_dual > 0 && (pt.equality_dual .= unsafe_wrap(Array, py, d.equality_dual))
        d.cone_dual > 0 && (pt.cone_dual .= unsafe_wrap(Array, pz, d.cone_dual))
        has(f) = (flags & f) != 0
        CALIPSO.evaluate!(s.problem, s.methods, s.indices, pt, s.parameters;
            objective=has(EVAL_OBJECTIVE), objective_gradient_variables=has(EVAL_OBJECTIVE_GRADIENT),
            objective_jacobian_variables_variables=has(EVAL_OBJECTIVE_HESSIAN),
            equality_constraint=has(EVAL_EQUALITY), equality_jacobian_variables=has(EVAL_EQUALITY_JACOBIAN),
            equality_dual_jacobian_variables=has(EVAL_EQUALITY_DUAL_GRADIENT),
            equality_dual_jacobian_variables_variables=has(EVAL_EQUALITY_DUAL_HESSIAN),
            cone_constraint=has(EVAL_CONE), cone_jacobian_variables=has(EVAL_CONE_JACOBIAN),
            cone_dual_jacobian_variables=has(EVAL_CONE_DUAL_GRADIENT),
            cone_dual_jacobian_variables_variables=has(EVAL_CONE_DUAL_HESSIAN),
            objective_jacobian_variables_parameters=has(EVAL_OBJECTIVE_JACOBIAN_PARAMETERS),
            equality_jacobian_parameters=has(EVAL_EQUALITY_JACOBIAN_PARAMETERS),
            equality_dual_jacobian_variables_parameters=has(EVAL_EQUALITY_DUAL_JACOBIAN_PARAMETERS),
            cone_jacobian_parameters=has(EVAL_CONE_JACOBIAN_PARAMETERS),
            cone_dual_jacobian_variables_parameters=has(EVAL_CONE_DUAL_JACOBIAN_PARAMETERS))
        p = s.problem
        h = hs.handle
        has(EVAL_OBJECTIVE) && set_field!(h, "objective", p.objective)
        has(EVAL_OBJECTIVE_GRADIENT) && set_field!(h, "objective_gradient_variables", p.objective_gradient_variables)
        has(EVAL_EQUALITY) && d.equality_dual > 0 && set_field!(h, "equality_constraint", p.equality_constraint)
        has(EVAL_EQUALITY_JACOBIAN) && d.equality_dual > 0 && set_field!(h, "equality_jacobian_variables", p.equality_jacobian_variables)
        has(EVAL_EQUALITY_DUAL_GRADIENT) && set_field!(h, "equality_dual_jacobian_variables", p.equality_dual_jacobian_variables)
        has(EVAL_CONE) && d.cone_dual > 0 && set_field!(h, "cone_constraint", p.cone_constraint)
        has(EVAL_CONE_JACOBIAN) && d.cone_dual > 0 && set_field!(h, "cone_jacobian_variables", p.cone_jacobian_variables)
        has(EVAL_CONE_DUAL_GRADIENT) && set_field!(h, "cone_dual_jacobian_variables", p.cone_dual_jacobian_variables)
        if has(EVAL_OBJECTIVE_HESSIAN)
            L = copy(p.objective_jacobian_variables_variables)
            if s.options.constraint_tensor
                L .+= p.equality_dual_jacobian_variables_variables
                L .+= p.cone_dual_jacobian_variables_variables
            end
            set_field!(h, "lagrangian_hessian", L)
        end
        if has(EVAL_OBJECTIVE_JACOBIAN_PARAMETERS) && d.parameters > 0
            G = p.objective_jacobian_variables_parameters + p.equality_dual_jacobian_variables_parameters + p.cone_dual_jacobian_variables_parameters
            set_field!(h, "lagrangian_gradient_parameters", G)
            d.equality_dual > 0 && set_field!(h, "equality_jacobian_parameters", p.equality_jacobian_parameters)
            d.cone_dual > 0 && set_field!(h, "cone_jacobian_parameters", p.cone_jacobian_parameters)
        end
        return Int32(0)
    catch err
        @error "evaluate! callback failed" err
        return Int32(1)
    end
end

"initialize!(solver, guess)  src/solver/initialize.jl:9-13"
function CALIPSO.initialize!(hs::HIPSolver, guess)
    g = Vector{Float64}(guess)
    hs.solver.solution.variables .= g
    check(hs.handle, ccall((:calipso_hip_initialize, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}), hs.handle, g), "initialize!")
    return
end

"""device-side evaluation (src/solver/evaluate.jl:37-121 as kernels on the solver's stream): `fn` = address of a `calipso_device_eval_fn` (dense ProblemData layout) or,
with `blocks = true` on a handle made with `structure = ...`, of a `calipso_device_block_eval_fn` that writes the handle's packed blocks (no dense scratch);
`user` is handed to it unchanged.  solve! then never calls back into Julia for an evaluation."""
function set_device_evaluator!(hs::HIPSolver, fn::Ptr{Cvoid}, user::Ptr{Cvoid} = C_NULL; blocks::Bool = false)
    rc = blocks ? ccall((:calipso_hip_set_device_block_evaluator, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), hs.handle, fn, user) :
                  ccall((:calipso_hip_set_device_evaluator, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), hs.handle, fn, user)
    check(hs.handle, rc, "set_device_evaluator!")
    return
end

"""correction rounds on every column of `differentiate!` (iterative_refinement.jl:14-44 per column; `"opt.differentiate_refinement"`, not an option of the reference —
the default is the unrefined condensed solve; inert on a layout with second-order cones, where the unrefined solve is the reference's answer)"""
set_differentiate_refinement!(hs::HIPSolver, on::Bool = true) = set_field!(hs.handle, "opt.differentiate_refinement", on ? 1.0 : 0.0)

"report of the last `differentiate!` of the handle: (columns, rounds = largest over the columns, failed_columns, final_norm); zeros when no correction round ran"
function differentiate_info(hs::HIPSolver)
    out = zeros(Float64, 4)
    check(hs.handle, ccall((:calipso_hip_differentiate_info, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}), hs.handle, out), "differentiate_info")
    return (columns = Int(out[1]), rounds = Int(out[2]), failed_columns = Int(out[3]), final_norm = out[4])
end

"""differentiate! in reverse mode on the handle (calipso_hip_differentiate_adjoint; differentiate.jl:1-61 and residual_jacobian_parameters.jl:1-40, transposed): for the
cotangent columns `cotangent` (N or N x k, dLoss/dw at the resident point) the adjoint `lambda = M' v` of the map `differentiate!` applies to a column and
`grad_theta = S' v` for the `S = dw/dtheta` that `differentiate!` would return — one condensed solve per cotangent instead of one per parameter.  `qp`: names out of
"PqAbGh" on a handle with an attached QP: the gradients with respect to those arrays (matrices rows x nx x k).  Returns a NamedTuple (adjoint, theta, qp::Dict).
`set_differentiate_refinement!` turns the correction rounds (against H') on; `differentiate_adjoint_info` reports them."""
function differentiate_adjoint!(hs::HIPSolver, cotangent::AbstractVecOrMat{Float64}; adjoint::Bool = true, theta::Bool = hs.solver.dimensions.parameters > 0, qp::AbstractString = "")
    d = hs.solver.dimensions
    V = Matrix{Float64}(reshape(cotangent, size(cotangent, 1), :))
    size(V, 1) == d.total || throw(ArgumentError("cotangent must be N or N x k"))
    k = size(V, 2)
    nx, ne, nc = d.variables, d.equality_dual, d.cone_dual
    sizes = Dict('P' => (nx, nx), 'q' => (nx,), 'A' => (ne, nx), 'b' => (ne,), 'G' => (nc, nx), 'h' => (nc,))
    all(c -> haskey(sizes, c), qp) || throw(ArgumentError("qp must be made of names out of PqAbGh"))
    adj = adjoint ? zeros(Float64, d.total, k) : nothing
    gth = theta ? zeros(Float64, max(d.parameters, 1), k) : nothing
    gq = Dict{Char,Array{Float64}}(c => zeros(Float64, sizes[c]..., k) for c in qp)
    ptrs = Ptr{Float64}[haskey(gq, c) ? pointer(gq[c]) : Ptr{Float64}(C_NULL) for c in "PqAbGh"]
    opt(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    rc = GC.@preserve hs V adj gth gq ptrs ccall((:calipso_hip_differentiate_adjoint, lib), Int32,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Ptr{Float64}}),
        hs.handle, hs.eval_cfunction, pointer_from_objref(hs), k, V, opt(adj), opt(gth), isempty(qp) ? Ptr{Ptr{Float64}}(C_NULL) : pointer(ptrs))
    check(hs.handle, rc, "differentiate_adjoint!")
    return (adjoint = adj, theta = theta ? gth[1:d.parameters, :] : nothing, qp = gq)
end

"report of the last `differentiate_adjoint!` of the handle, as `differentiate_info`: (columns, rounds, failed_columns, final_norm)"
function differentiate_adjoint_info(hs::HIPSolver)
    out = zeros(Float64, 4)
    check(hs.handle, ccall((:calipso_hip_differentiate_adjoint_info, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}), hs.handle, out), "differentiate_adjoint_info")
    return (columns = Int(out[1]), rounds = Int(out[2]), failed_columns = Int(out[3]), final_norm = out[4])
end

"HIP-event times of the last `differentiate_adjoint!` in ms: (device = entry to last kernel, copy = results to the host, gradients = of device, the QP data-gradient kernels alone)"
function differentiate_adjoint_times(hs::HIPSolver)
    out = zeros(Float64, 3)
    check(hs.handle, ccall((:calipso_hip_differentiate_adjoint_times, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}), hs.handle, out), "differentiate_adjoint_times")
    return (device = out[1], copy = out[2], gradients = out[3])
end

"solve!(solver)::Bool  src/solver/solve.jl:8-377 — results are copied back into the wrapped Solver's fields"
function CALIPSO.solve!(hs::HIPSolver)
    rc = GC.@preserve hs ccall((:calipso_hip_solve, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), hs.handle, hs.eval_cfunction, pointer_from_objref(hs))
    check(hs.handle, rc, "solve!")
    copy_back!(hs)
    return rc == 1
end

"copy the results of the device handle into the wrapped reference Solver's own fields (what tests and examples read)"
function copy_back!(hs::HIPSolver)
    s = hs.solver
    d = s.dimensions
    s.solution.all .= get_field(hs.handle, "solution", d.total)
    s.data.residual.all .= get_field(hs.handle, "residual", d.total)
    s.data.step.all .= get_field(hs.handle, "step", d.total)
    d.cone_dual > 0 && (s.problem.cone_product .= get_field(hs.handle, "cone_product", d.cone_dual))
    for (name, ref) in (("central_path", s.central_path), ("penalty", s.penalty), ("fraction_to_boundary", s.fraction_to_boundary),
                        ("primal_regularization", s.primal_regularization), ("dual_regularization", s.dual_regularization),
                        ("primal_regularization_last", s.primal_regularization_last))
        ref[1] = get_field(hs.handle, name, 1)[1]
    end
    d.equality_dual > 0 && (s.dual .= get_field(hs.handle, "dual", d.equality_dual))
    if s.options.differentiate && d.parameters > 0
        s.data.solution_sensitivity .= reshape(get_field(hs.handle, "solution_sensitivity", d.total * d.parameters), d.total, d.parameters)
    end
    return
end

# ---- linear-solver seam (src/solver/linear_solver.jl:1-60) -------------------------------------------------------------------
"""
    HIPLDLSolver(A::SparseMatrixCSC) / hip_ldl_solver(A)

Drop-in for `LDLSolver` (linear_solver.jl:3-17,46-50): a device LDL^T for the sparse symmetric quasi-definite matrix the
reference assembles itself.  `factorize!(s, A)` ships A's CSC arrays (colptr / rowval / nzval, 1-based as Julia stores them; only
triu(A) is read, linear_solver.jl:23) to the device and factors there; `compute_inertia!` / `linear_solve!` have the reference's
signatures and semantics, so the reference's own `search_direction!` (search_direction.jl:1-23), `iterative_refinement!`
(iterative_refinement.jl:20-26), `inertia_correction!` (inertia.jl:17-28) and `differentiate!` (differentiate.jl:19-46) run
unmodified with `solver.linear_solver = hip_ldl_solver(solver.data.jacobian_variables_symmetric)`.
(One-line change in the reference for that assignment: the field is declared `linear_solver::LDLSolver{T,Int}` in
solver.jl:14 — widen it to `linear_solver::LinearSolver`.)
"""
mutable struct HIPLDLSolver <: CALIPSO.LinearSolver
    handle::Ptr{Cvoid}
    n::Int
    inertia::CALIPSO.Inertia
end

function HIPLDLSolver(n::Integer; device::Integer=0)
    href = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:calipso_hip_ldl_create, lib), Int32, (Int64, Int32, Ptr{Ptr{Cvoid}}), n, device, href)
    rc != 0 && throw(HIPError(rc, "calipso_hip_ldl_create: $(last_error(href[]))"))
    s = HIPLDLSolver(href[], n, CALIPSO.Inertia(0, 0, 0))
    finalizer(x -> ccall((:calipso_hip_destroy, lib), Int32, (Ptr{Cvoid},), x.handle), s)
    return s
end

"ldl_solver(A)  linear_solver.jl:46-50 (factors once at construction, as `qdldl(A)` does there)"
function hip_ldl_solver(A::SparseMatrixCSC{Float64,Int}; device::Integer=0)
    s = HIPLDLSolver(size(A, 1); device=device)
    CALIPSO.factorize!(s, A)
    return s
end
hip_ldl_solver(A::Matrix{Float64}; kw...) = hip_ldl_solver(sparse(A); kw...)

"factorize!(s, A; update)  linear_solver.jl:19-31.  `update` only selects between value update and symbolic re-analysis in QDLDL; the dense device factorisation has no symbolic phase, so both take the same path.  Like the reference with update=true, only triu(A) matters (A itself is not mutated here)."
function CALIPSO.factorize!(s::HIPLDLSolver, A::SparseMatrixCSC{Float64,Int}; update=false)
    out = zeros(Int64, 3)
    rc = ccall((:calipso_hip_ldl_factorize_csc, lib), Int32, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}),
               s.handle, s.n, A.colptr, A.rowval, A.nzval, out)
    rc < 0 && throw(HIPError(rc, "factorize!: $(last_error(s.handle))"))
    rc == 1 && @warn "Zero entry in D (matrix is not quasidefinite)"     # qdldl.jl:309-311
    s.inertia.positive, s.inertia.negative, s.inertia.zero = out
    return nothing
end

"compute_inertia!(s)  linear_solver.jl:33-44"
function CALIPSO.compute_inertia!(s::HIPLDLSolver)
    out = zeros(Int64, 3)
    check(s.handle, ccall((:calipso_hip_ldl_inertia, lib), Int32, (Ptr{Cvoid}, Ptr{Int64}), s.handle, out), "compute_inertia!")
    s.inertia.positive, s.inertia.negative, s.inertia.zero = out
    return nothing
end

"linear_solve!(s, x, A, b; fact, update)  linear_solver.jl:52-60"
function CALIPSO.linear_solve!(s::HIPLDLSolver, x::Vector{Float64}, A::SparseMatrixCSC{Float64,Int}, b::Vector{Float64}; fact=true, update=true)
    fact && CALIPSO.factorize!(s, A; update=update)
    check(s.handle, ccall((:calipso_hip_ldl_solve, lib), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Ptr{Float64}), s.handle, s.n, 1, b, x), "linear_solve!")
    return
end

"linear_solve!(s, X, A, B; fact, update) for matrices  linear_solver.jl:82-99: all columns through one factorisation"
function CALIPSO.linear_solve!(s::HIPLDLSolver, x::Matrix{Float64}, A::SparseMatrixCSC{Float64,Int}, b::Matrix{Float64}; fact=true, update=true)
    fact && CALIPSO.factorize!(s, A; update=update)
    check(s.handle, ccall((:calipso_hip_ldl_solve, lib), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Ptr{Float64}), s.handle, s.n, size(b, 2), b, x), "linear_solve!")
    return
end

# ---- sparse variant: qdldl(A; perm) on the device without dense storage (csrc/sparse.hip) ---------------------------------------------------
"""
    HIPSparseLDLSolver(A::SparseMatrixCSC; method=:nested_dissection, perm=nothing) / hip_sparse_ldl_solver(A)

`LDLSolver` (linear_solver.jl:1-60) with the analyse phase of `qdldl(A; perm)` (qdldl.jl:134-188) at construction and the numeric
factorisation / triangular solves level-scheduled on the device; memory O(nnz(L)).  The pattern of `A` is fixed at construction
(as `update=true` assumes in linear_solver.jl:24-27); `factorize!` sends only `A.nzval`.
"""
mutable struct HIPSparseLDLSolver <: CALIPSO.LinearSolver
    handle::Ptr{Cvoid}
    n::Int
    nnz::Int
    inertia::CALIPSO.Inertia
end
const SPARSE_METHODS = Dict(:natural => 0, :rcm => 1, :minimum_degree => 2, :nested_dissection => 4, :nested_dissection_columns => 5)
sparse_last_error(h) = unsafe_string(ccall((:calipso_hip_sparse_last_error, lib), Cstring, (Ptr{Cvoid},), h))

function HIPSparseLDLSolver(A::SparseMatrixCSC{Float64,Int}; method::Symbol=:nested_dissection, perm::Union{Nothing,Vector{Int}}=nothing, device::Integer=0)
    href = Ref{Ptr{Cvoid}}(C_NULL)
    m = perm === nothing ? SPARSE_METHODS[method] : 3
    rc = ccall((:calipso_hip_sparse_create, lib), Int32, (Int64, Ptr{Int64}, Ptr{Int64}, Int32, Ptr{Int64}, Int32, Ptr{Ptr{Cvoid}}),
               size(A, 1), A.colptr, A.rowval, m, perm === nothing ? C_NULL : perm, device, href)
    if rc != 0
        msg = sparse_last_error(href[])
        href[] != C_NULL && ccall((:calipso_hip_sparse_destroy, lib), Int32, (Ptr{Cvoid},), href[])
        throw(HIPError(rc, "calipso_hip_sparse_create: $msg"))
    end
    s = HIPSparseLDLSolver(href[], size(A, 1), nnz(A), CALIPSO.Inertia(0, 0, 0))
    finalizer(x -> ccall((:calipso_hip_sparse_destroy, lib), Int32, (Ptr{Cvoid},), x.handle), s)
    return s
end
function hip_sparse_ldl_solver(A::SparseMatrixCSC{Float64,Int}; kw...)
    s = HIPSparseLDLSolver(A; kw...)
    CALIPSO.factorize!(s, A)
    return s
end

function CALIPSO.factorize!(s::HIPSparseLDLSolver, A::SparseMatrixCSC{Float64,Int}; update=false)
    nnz(A) == s.nnz || throw(HIPError(-1, "factorize!: the pattern of A differs from the analysed one (build a new HIPSparseLDLSolver)"))
    out = zeros(Int64, 3)
    rc = ccall((:calipso_hip_sparse_factorize, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int64}), s.handle, A.nzval, out)
    rc < 0 && throw(HIPError(rc, "factorize!: $(sparse_last_error(s.handle))"))
    rc == 1 && @warn "Zero entry in D (matrix is not quasidefinite)"     # qdldl.jl:309-311
    s.inertia.positive, s.inertia.negative, s.inertia.zero = out
    return nothing
end
CALIPSO.compute_inertia!(s::HIPSparseLDLSolver) = nothing      # (set by factorize!, as the values of linear_solver.jl:33-44 only change there)
function CALIPSO.linear_solve!(s::HIPSparseLDLSolver, x::VecOrMat{Float64}, A::SparseMatrixCSC{Float64,Int}, b::VecOrMat{Float64}; fact=true, update=true)
    fact && CALIPSO.factorize!(s, A; update=update)
    rc = ccall((:calipso_hip_sparse_solve, lib), Int32, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}), s.handle, size(b, 2), b, x)
    rc < 0 && throw(HIPError(rc, "linear_solve!: $(sparse_last_error(s.handle))"))
    return
end

# ---- search_direction! on sparse problem data resident on the device (csrc/sparse_kkt.hip): ccall wrappers, no logic ---------------------------------
"""
    SparseKKT(Lxx, gx, hx; n_nonnegative, second_order_dims, method=:nested_dissection, perm=nothing)

search_direction! (search_direction.jl:1-23) for a problem whose Lagrangian Hessian `Lxx` (both triangles) and Jacobians `gx`, `hx` are sparse and stay on the
device: `set_values!`, then `sparse_search_direction!(kkt, residual, step, regularization)` with `regularization = [εp, εp_last, εd]`, in and out.  Returns
`(status, info)`: status 2 = the refinement failed and `step` is the last refined step (there is no `H \\ residual` fallback).
"""
mutable struct SparseKKT
    handle::Ptr{Cvoid}
    N::Int
    nnz_upper::Int
end
kkt_last_error(h) = unsafe_string(ccall((:calipso_hip_sparse_kkt_last_error, lib), Cstring, (Ptr{Cvoid},), h))
kkt_check(rc, k, what) = rc < 0 ? throw(HIPError(rc, "$what: $(kkt_last_error(k.handle))")) : rc

function SparseKKT(Lxx::SparseMatrixCSC{Float64,Int}, gx::SparseMatrixCSC{Float64,Int}, hx::SparseMatrixCSC{Float64,Int}; n_nonnegative::Integer,
                   second_order_dims::Vector{Int}=Int[], method::Symbol=:nested_dissection, perm::Union{Nothing,Vector{Int}}=nothing, device::Integer=0)
    href = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:calipso_hip_sparse_kkt_create, lib), Int32,
               (Int64, Int64, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int32, Ptr{Int64}, Int32, Ptr{Ptr{Cvoid}}),
               size(Lxx, 1), size(gx, 1), size(hx, 1), n_nonnegative, length(second_order_dims), second_order_dims, Lxx.colptr, Lxx.rowval, gx.colptr, gx.rowval,
               hx.colptr, hx.rowval, perm === nothing ? SPARSE_METHODS[method] : 3, perm === nothing ? C_NULL : perm, device, href)
    rc != 0 && throw(HIPError(rc, "calipso_hip_sparse_kkt_create: $(kkt_last_error(C_NULL))"))
    info = zeros(Int64, 8)
    ccall((:calipso_hip_sparse_kkt_info, lib), Int32, (Ptr{Cvoid}, Ptr{Int64}), href[], info)
    k = SparseKKT(href[], info[8], info[2])
    finalizer(x -> ccall((:calipso_hip_sparse_kkt_destroy, lib), Int32, (Ptr{Cvoid},), x.handle), k)
    return k
end
kkt_info(k::SparseKKT) = (info = zeros(Int64, 8); kkt_check(ccall((:calipso_hip_sparse_kkt_info, lib), Int32, (Ptr{Cvoid}, Ptr{Int64}), k.handle, info), k, "info"); info)
kkt_pattern(k::SparseKKT, colptr::Vector{Int64}, rowval::Vector{Int64}) =
    kkt_check(ccall((:calipso_hip_sparse_kkt_pattern, lib), Int32, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), k.handle, colptr, rowval), k, "pattern")
set_option!(k::SparseKKT, name::AbstractString, value::Real) =
    kkt_check(ccall((:calipso_hip_sparse_kkt_set_option, lib), Int32, (Ptr{Cvoid}, Cstring, Float64), k.handle, name, value), k, "set_option!($name)")
kkt_ptr(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
# host arrays (nothing keeps what is resident); penalty: a one-element vector
set_values!(k::SparseKKT; Lxx=nothing, gx=nothing, hx=nothing, w=nothing, penalty=nothing) = GC.@preserve Lxx gx hx w penalty kkt_check(
    ccall((:calipso_hip_sparse_kkt_set_values, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
          k.handle, kkt_ptr(Lxx), kkt_ptr(gx), kkt_ptr(hx), kkt_ptr(w), kkt_ptr(penalty)), k, "set_values!")
# device pointers on the handle's device (C_NULL keeps what is resident)
set_values_device!(k::SparseKKT; Lxx=C_NULL, gx=C_NULL, hx=C_NULL, w=C_NULL, penalty=C_NULL) = kkt_check(
    ccall((:calipso_hip_sparse_kkt_set_values_device, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), k.handle, Lxx, gx, hx, w, penalty),
    k, "set_values_device!")
function kkt_factorize!(k::SparseKKT, ep::Real, ed::Real)
    out = zeros(Int64, 3)
    rc = kkt_check(ccall((:calipso_hip_sparse_kkt_factorize, lib), Int32, (Ptr{Cvoid}, Float64, Float64, Ptr{Int64}), k.handle, ep, ed, out), k, "factorize")
    return rc, out
end
kkt_matrix!(k::SparseKKT, nzval::Vector{Float64}) = kkt_check(ccall((:calipso_hip_sparse_kkt_get_matrix, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}), k.handle, nzval), k, "get_matrix")
kkt_mul!(k::SparseKKT, out::Vector{Float64}, v::Vector{Float64}) =
    kkt_check(ccall((:calipso_hip_sparse_kkt_mul, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), k.handle, v, out), k, "mul")
solve_symmetric!(k::SparseKKT, step::Vector{Float64}, residual::Vector{Float64}) =
    kkt_check(ccall((:calipso_hip_sparse_kkt_solve_symmetric, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), k.handle, residual, step), k, "solve_symmetric")
function sparse_search_direction!(k::SparseKKT, residual::Vector{Float64}, step::Vector{Float64}, regularization::Vector{Float64})
    info = zeros(4)
    rc = kkt_check(ccall((:calipso_hip_sparse_kkt_search_direction, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                         k.handle, residual, step, regularization, info), k, "search_direction!")
    return rc, info
end
function sparse_search_direction_device!(k::SparseKKT, residual::Ptr{Cvoid}, step::Ptr{Cvoid}, regularization::Vector{Float64})
    info = zeros(4)
    rc = kkt_check(ccall((:calipso_hip_sparse_kkt_search_direction_device, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}),
                         k.handle, residual, step, regularization, info), k, "search_direction_device!")
    return rc, info
end
# search_direction_nonsymmetric! for this handle: `H \ residual` by preconditioned GMRES with the current factorisation (csrc/sparse_krylov.hip)
solve_nonsymmetric!(k::SparseKKT, step::Vector{Float64}, residual::Vector{Float64}) =
    kkt_check(ccall((:calipso_hip_sparse_kkt_solve_nonsymmetric, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), k.handle, residual, step), k, "solve_nonsymmetric")
solve_nonsymmetric_device!(k::SparseKKT, step::Ptr{Cvoid}, residual::Ptr{Cvoid}) =
    kkt_check(ccall((:calipso_hip_sparse_kkt_solve_nonsymmetric_device, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), k.handle, residual, step), k, "solve_nonsymmetric_device")
kkt_fallback_info(k::SparseKKT) = (out = zeros(12); kkt_check(ccall((:calipso_hip_sparse_kkt_fallback_info, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}), k.handle, out), k, "fallback_info"); out)
kkt_timing(k::SparseKKT) = (ms = zeros(8); kkt_check(ccall((:calipso_hip_sparse_kkt_timing, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}), k.handle, ms), k, "timing"); ms)

# ---- search_direction! on sparse data for groups of same-pattern problems in lockstep (csrc/sparse_kkt_group.hip): ccall wrappers, no logic ----------------------
"""
    SparseKKTGroup(Lxx, gx, hx, members; n_nonnegative, second_order_dims, method=:nested_dissection, perm=nothing)

`members` (1 .. 128) problems of one pattern through the same launches: one analysis, one multifrontal plan.  Every array is member-major (`members` pieces of
one length).  `group_search_direction!(g, residual, step, regularization)` returns `(worst, info, status, report)`; member m's results are bit for bit those of a
`SparseKKT` on the same data.  No `H \\ residual` fallback: a member whose refinement fails gets status 2 and its last refined step.
"""
mutable struct SparseKKTGroup
    handle::Ptr{Cvoid}
    N::Int
    nnz_upper::Int
    members::Int
end
group_last_error(h) = unsafe_string(ccall((:calipso_hip_sparse_kkt_group_last_error, lib), Cstring, (Ptr{Cvoid},), h))
group_check(rc, g, what) = rc < 0 ? throw(HIPError(rc, "$what: $(group_last_error(g.handle))")) : rc
function SparseKKTGroup(Lxx::SparseMatrixCSC{Float64,Int}, gx::SparseMatrixCSC{Float64,Int}, hx::SparseMatrixCSC{Float64,Int}, members::Integer; n_nonnegative::Integer,
                        second_order_dims::Vector{Int}=Int[], method::Symbol=:nested_dissection, perm::Union{Nothing,Vector{Int}}=nothing, device::Integer=0)
    href = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:calipso_hip_sparse_kkt_group_create, lib), Int32,
               (Int64, Int64, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Int32, Ptr{Int64}, Int32, Int64, Ptr{Ptr{Cvoid}}),
               size(Lxx, 1), size(gx, 1), size(hx, 1), n_nonnegative, length(second_order_dims), second_order_dims, Lxx.colptr, Lxx.rowval, gx.colptr, gx.rowval,
               hx.colptr, hx.rowval, perm === nothing ? SPARSE_METHODS[method] : 3, perm === nothing ? C_NULL : perm, device, members, href)
    rc != 0 && throw(HIPError(rc, "calipso_hip_sparse_kkt_group_create: $(group_last_error(C_NULL))"))
    info = zeros(Int64, 9)
    ccall((:calipso_hip_sparse_kkt_group_info, lib), Int32, (Ptr{Cvoid}, Ptr{Int64}), href[], info)
    g = SparseKKTGroup(href[], info[8], info[2], info[9])
    finalizer(x -> ccall((:calipso_hip_sparse_kkt_group_destroy, lib), Int32, (Ptr{Cvoid},), x.handle), g)
    return g
end
group_info(g::SparseKKTGroup) = (info = zeros(Int64, 9); group_check(ccall((:calipso_hip_sparse_kkt_group_info, lib), Int32, (Ptr{Cvoid}, Ptr{Int64}), g.handle, info), g, "info"); info)
group_pattern(g::SparseKKTGroup, colptr::Vector{Int64}, rowval::Vector{Int64}) =
    group_check(ccall((:calipso_hip_sparse_kkt_group_pattern, lib), Int32, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), g.handle, colptr, rowval), g, "pattern")
set_option!(g::SparseKKTGroup, name::AbstractString, value::Real) =
    group_check(ccall((:calipso_hip_sparse_kkt_group_set_option, lib), Int32, (Ptr{Cvoid}, Cstring, Float64), g.handle, name, value), g, "set_option!($name)")
# host arrays, members x count each (nothing keeps what is resident); penalty and central_path: `members` values
set_values!(g::SparseKKTGroup; Lxx=nothing, gx=nothing, hx=nothing, w=nothing, penalty=nothing, central_path=nothing) = GC.@preserve Lxx gx hx w penalty central_path group_check(
    ccall((:calipso_hip_sparse_kkt_group_set_values, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
          g.handle, kkt_ptr(Lxx), kkt_ptr(gx), kkt_ptr(hx), kkt_ptr(w), kkt_ptr(penalty), kkt_ptr(central_path)), g, "set_values!")
# device pointers on the group's device (C_NULL keeps what is resident); central_path stays a host vector
set_values_device!(g::SparseKKTGroup; Lxx=C_NULL, gx=C_NULL, hx=C_NULL, w=C_NULL, penalty=C_NULL, central_path=nothing) = GC.@preserve central_path group_check(
    ccall((:calipso_hip_sparse_kkt_group_set_values_device, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}),
          g.handle, Lxx, gx, hx, w, penalty, kkt_ptr(central_path)), g, "set_values_device!")
function group_factorize!(g::SparseKKTGroup, ep::Vector{Float64}, ed::Vector{Float64})
    out = zeros(Int64, 3 * g.members)
    rc = group_check(ccall((:calipso_hip_sparse_kkt_group_factorize, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}), g.handle, ep, ed, out), g, "factorize")
    return rc, out
end
group_matrix!(g::SparseKKTGroup, member::Integer, nzval::Vector{Float64}) =      # member: 0-based, as the C entry takes it
    group_check(ccall((:calipso_hip_sparse_kkt_group_get_matrix, lib), Int32, (Ptr{Cvoid}, Int64, Ptr{Float64}), g.handle, member, nzval), g, "get_matrix")
group_mul!(g::SparseKKTGroup, out::Vector{Float64}, v::Vector{Float64}) =
    group_check(ccall((:calipso_hip_sparse_kkt_group_mul, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), g.handle, v, out), g, "mul")
solve_symmetric!(g::SparseKKTGroup, step::Vector{Float64}, residual::Vector{Float64}) =
    group_check(ccall((:calipso_hip_sparse_kkt_group_solve_symmetric, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), g.handle, residual, step), g, "solve_symmetric")
# returns the worst member status (0, 2 or -1 = a member's inertia correction failed: see status), info (4 per member), status (per member), report (8)
function group_search_direction!(g::SparseKKTGroup, residual::Vector{Float64}, step::Vector{Float64}, regularization::Vector{Float64})
    info, status, report = zeros(4 * g.members), zeros(Int32, g.members), zeros(8)
    rc = ccall((:calipso_hip_sparse_kkt_group_search_direction, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}),
               g.handle, residual, step, regularization, info, status, report)
    rc != -1 && group_check(rc, g, "search_direction!")
    return rc, info, status, report
end
function group_search_direction_device!(g::SparseKKTGroup, residual::Ptr{Cvoid}, step::Ptr{Cvoid}, regularization::Vector{Float64})
    info, status, report = zeros(4 * g.members), zeros(Int32, g.members), zeros(8)
    rc = ccall((:calipso_hip_sparse_kkt_group_search_direction_device, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}),
               g.handle, residual, step, regularization, info, status, report)
    rc != -1 && group_check(rc, g, "search_direction_device!")
    return rc, info, status, report
end
group_timing(g::SparseKKTGroup) = (ms = zeros(8); group_check(ccall((:calipso_hip_sparse_kkt_group_timing, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}), g.handle, ms), g, "timing"); ms)

# ---- solve! of every member of a group in lockstep (csrc/sparse_solve_group.hip): ccall wrappers, no logic.  Arrays are members x count, member-major; `member` is
# 0-based, as the C entries take it.  Member m's results are bit for bit those of sparse_solve! on a SparseKKT with the same data and options
qp_attach!(g::SparseKKTGroup, q::Vector{Float64}, b::Vector{Float64}, h::Vector{Float64}; objective_constants=nothing) = GC.@preserve objective_constants group_check(
    ccall((:calipso_hip_sparse_kkt_group_qp_attach, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), g.handle, q, b, h, kkt_ptr(objective_constants)),
    g, "qp_attach!")
qp_attach_device!(g::SparseKKTGroup, q::Ptr{Cvoid}, b::Ptr{Cvoid}, h::Ptr{Cvoid}; objective_constants=nothing) = GC.@preserve objective_constants group_check(
    ccall((:calipso_hip_sparse_kkt_group_qp_attach_device, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}), g.handle, q, b, h, kkt_ptr(objective_constants)),
    g, "qp_attach_device!")
group_initialize!(g::SparseKKTGroup, x0::Vector{Float64}) = group_check(ccall((:calipso_hip_sparse_kkt_group_initialize, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}), g.handle, x0), g, "initialize!")
group_initialize_device!(g::SparseKKTGroup, x0::Ptr{Cvoid}) =
    group_check(ccall((:calipso_hip_sparse_kkt_group_initialize_device, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), g.handle, x0), g, "initialize_device!")
# returns the worst member status (a member's own error status does not throw: see status), status (per member), info (16 per member), report (16)
function group_solve!(g::SparseKKTGroup)
    status, info, report = zeros(Int32, g.members), zeros(16 * g.members), zeros(16)
    rc = ccall((:calipso_hip_sparse_kkt_group_solve, lib), Int32, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}), g.handle, status, info, report)
    rc < 0 && !(rc in status) && group_check(rc, g, "solve!")
    return rc, status, info, report
end
group_get!(g::SparseKKTGroup, name::AbstractString, member::Integer, out::Vector{Float64}) =
    group_check(ccall((:calipso_hip_sparse_kkt_group_get, lib), Int32, (Ptr{Cvoid}, Cstring, Int64, Ptr{Float64}, Int64), g.handle, name, member, out, length(out)), g, "get($name)")
function group_solution_device(g::SparseKKTGroup)
    p = Ref{Ptr{Float64}}(C_NULL)
    group_check(ccall((:calipso_hip_sparse_kkt_group_solution_device, lib), Int32, (Ptr{Cvoid}, Ptr{Ptr{Float64}}), g.handle, p), g, "solution_device")
    return p[]
end
group_keep_trace!(g::SparseKKTGroup, rows::Integer) = group_check(ccall((:calipso_hip_sparse_kkt_group_keep_trace, lib), Int32, (Ptr{Cvoid}, Int64), g.handle, rows), g, "keep_trace!")
function group_trace!(g::SparseKKTGroup, member::Integer, out::Matrix{Float64})      # out: N x cap_rows (column r = accepted iterate r); returns (rows written, accepted in all)
    accepted = Ref{Int64}(0)
    rows = group_check(ccall((:calipso_hip_sparse_kkt_group_trace, lib), Int32, (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Ptr{Int64}), g.handle, member, out, size(out, 2), accepted), g, "trace")
    return rows, accepted[]
end

# ---- solve! on the same handle (csrc/sparse_solve.hip): the sparse conic QP min c x'Px + q'x  s.t.  Ax - b = 0,  h - Gx in K  with Lxx = c (P + P'), gx = A, hx = -G ----
# host vectors (nothing keeps what is resident)
qp_attach!(k::SparseKKT; q=nothing, b=nothing, h=nothing, objective_constant::Real=0.0) = GC.@preserve q b h kkt_check(
    ccall((:calipso_hip_sparse_kkt_qp_attach, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64), k.handle, kkt_ptr(q), kkt_ptr(b), kkt_ptr(h),
          objective_constant), k, "qp_attach!")
# initialize!(solver, x0)  initialize.jl:9-48
sparse_initialize!(k::SparseKKT, x0::Vector{Float64}) = kkt_check(ccall((:calipso_hip_sparse_kkt_initialize, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}), k.handle, x0), k, "initialize!")
"""
    sparse_solve!(kkt) -> (status, info)

solve! (solve.jl:8-377) with every vector resident on the device.  status 1 solved, 0 iteration caps, -102 a refinement failure without the option
`continue_after_refinement_failure` (the point is the last accepted iterate); the reference's error()s throw.  `info` as calipso_hip_sparse_kkt_solve documents it.
"""
function sparse_solve!(k::SparseKKT)
    info = zeros(16)
    rc = ccall((:calipso_hip_sparse_kkt_solve, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}), k.handle, info)
    rc == -102 || kkt_check(rc, k, "solve!")
    return rc, info
end
function sparse_get(k::SparseKKT, name::AbstractString, len::Integer)
    out = zeros(len)
    kkt_check(ccall((:calipso_hip_sparse_kkt_get, lib), Int32, (Ptr{Cvoid}, Cstring, Ptr{Float64}, Int64), k.handle, name, out, len), k, "get($name)")
    return out
end
sparse_set!(k::SparseKKT, name::AbstractString, v::Vector{Float64}) =
    kkt_check(ccall((:calipso_hip_sparse_kkt_set, lib), Int32, (Ptr{Cvoid}, Cstring, Ptr{Float64}, Int64), k.handle, name, v, length(v)), k, "set($name)")

# ---- solve! on sparse data with an evaluator: nonlinear problems on the same handle (ccall wrappers, no logic; not executed here either) ---------------------------
# fn: a calipso_device_sparse_eval_fn from a shared library (dlsym), user: its object; replaces qp_attach!, and qp_attach! replaces it; fn = C_NULL removes it
sparse_set_evaluator!(k::SparseKKT, fn::Ptr{Cvoid}, user::Ptr{Cvoid}=C_NULL; num_parameters::Integer=0) =
    kkt_check(ccall((:calipso_hip_sparse_kkt_set_evaluator, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64), k.handle, fn, user, num_parameters), k, "set_evaluator!")
sparse_set_parameters!(k::SparseKKT, theta::Vector{Float64}) =
    kkt_check(ccall((:calipso_hip_sparse_kkt_set_parameters, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}), k.handle, theta), k, "set_parameters!")
sparse_set_parameters_device!(k::SparseKKT, theta::Ptr{Cvoid}) =
    kkt_check(ccall((:calipso_hip_sparse_kkt_set_parameters_device, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), k.handle, theta), k, "set_parameters_device!")
# the evaluator at the solution (which = 0) or at the candidate (1); flags: CALIPSO_EVAL_* without dual gradients and parameter Jacobians
sparse_evaluate!(k::SparseKKT, flags::Integer; which::Integer=0) =
    kkt_check(ccall((:calipso_hip_sparse_kkt_evaluate, lib), Int32, (Ptr{Cvoid}, Int32, UInt32), k.handle, which, flags), k, "evaluate!")
# the stored patterns of dR/dtheta's three blocks (1-based CSC, num_parameters columns): the Lagrangian's theta-gradient (nx rows), g,theta (ne rows), h,theta (nc rows)
sparse_set_parameter_patterns!(k::SparseKKT, Lp_colptr::Vector{Int64}, Lp_rowval::Vector{Int64}, gp_colptr::Vector{Int64}, gp_rowval::Vector{Int64}, hp_colptr::Vector{Int64}, hp_rowval::Vector{Int64}) =
    kkt_check(ccall((:calipso_hip_sparse_kkt_set_parameter_patterns, lib), Int32, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}), k.handle,
                    Lp_colptr, Lp_rowval, gp_colptr, gp_rowval, hp_colptr, hp_rowval), k, "set_parameter_patterns!")
# the evaluator's five parameter bits at the resident point and theta into the three resident arrays (sparse_get: lagrangian_gradient_parameters, ...)
sparse_evaluate_parameters!(k::SparseKKT) = kkt_check(ccall((:calipso_hip_sparse_kkt_evaluate_parameters, lib), Int32, (Ptr{Cvoid},), k.handle), k, "evaluate_parameters!")

# ---- differentiate! on the same handle (csrc/sparse_differentiate.hip): ccall wrappers, no logic; not executed here either (see the note at the top) -----------
# X = M B (transposed: M' B) through the current factorisation; B, X: N x k
sparse_solve_columns!(k::SparseKKT, X::Matrix{Float64}, B::Matrix{Float64}; transposed::Bool=false) = kkt_check(
    ccall((:calipso_hip_sparse_kkt_solve_columns, lib), Int32, (Ptr{Cvoid}, Int64, Int32, Ptr{Float64}, Ptr{Float64}), k.handle, size(B, 2), transposed ? 1 : 0, B, X), k, "solve_columns!")
# differentiate! (differentiate.jl:13-58) for the caller's dR/dtheta (N x k): sensitivity = -M jacobian_parameters
sparse_differentiate!(k::SparseKKT, sensitivity::Matrix{Float64}, jacobian_parameters::Matrix{Float64}) = kkt_check(
    ccall((:calipso_hip_sparse_kkt_differentiate, lib), Int32, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}), k.handle, size(jacobian_parameters, 2), jacobian_parameters, sensitivity), k, "differentiate!")
# reverse mode: adjoint = M' cotangent (N x k, or nothing); grad: six arrays Lxx, q, gx, b, hx, hvec (size x k each, or nothing), the matrices on their stored patterns
function sparse_differentiate_adjoint!(k::SparseKKT, cotangent::Matrix{Float64}; adjoint=nothing, grad=nothing)
    ptrs = grad === nothing ? C_NULL : Ptr{Float64}[kkt_ptr(g) for g in grad]
    GC.@preserve adjoint grad ptrs kkt_check(
        ccall((:calipso_hip_sparse_kkt_differentiate_adjoint, lib), Int32, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Ptr{Float64}}), k.handle, size(cotangent, 2), cotangent,
              kkt_ptr(adjoint), ptrs), k, "differentiate_adjoint!")
end
# the same two with the EVALUATOR's dR/dtheta on its stored patterns (sparse_set_parameter_patterns!): columns = 1-based parameter indices, nothing = all of them;
# grad_theta: num_parameters x k
sparse_differentiate_parameters!(k::SparseKKT, sensitivity::Matrix{Float64}; columns::Union{Nothing,Vector{Int64}}=nothing) = GC.@preserve columns kkt_check(
    ccall((:calipso_hip_sparse_kkt_differentiate_parameters, lib), Int32, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}), k.handle, size(sensitivity, 2),
          columns === nothing ? C_NULL : pointer(columns), sensitivity), k, "differentiate_parameters!")
sparse_differentiate_adjoint_parameters!(k::SparseKKT, grad_theta::Matrix{Float64}, cotangent::Matrix{Float64}; adjoint=nothing) = GC.@preserve adjoint kkt_check(
    ccall((:calipso_hip_sparse_kkt_differentiate_adjoint_parameters, lib), Int32, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), k.handle, size(cotangent, 2), cotangent,
          kkt_ptr(adjoint), grad_theta), k, "differentiate_adjoint_parameters!")
sparse_differentiate_parameters_device!(k::SparseKKT, sensitivity::Ptr{Cvoid}, ncols::Integer; columns::Union{Nothing,Vector{Int64}}=nothing) = GC.@preserve columns kkt_check(
    ccall((:calipso_hip_sparse_kkt_differentiate_parameters_device, lib), Int32, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Cvoid}), k.handle, ncols,
          columns === nothing ? C_NULL : pointer(columns), sensitivity), k, "differentiate_parameters_device!")
sparse_differentiate_adjoint_parameters_device!(k::SparseKKT, grad_theta::Ptr{Cvoid}, cotangent::Ptr{Cvoid}, ncols::Integer; adjoint::Ptr{Cvoid}=C_NULL) = kkt_check(
    ccall((:calipso_hip_sparse_kkt_differentiate_adjoint_parameters_device, lib), Int32, (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), k.handle, ncols, cotangent, adjoint,
          grad_theta), k, "differentiate_adjoint_parameters_device!")
sparse_differentiate_info(k::SparseKKT) = (out = zeros(4); kkt_check(ccall((:calipso_hip_sparse_kkt_differentiate_info, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}), k.handle, out), k, "differentiate_info"); out)
sparse_differentiate_adjoint_info(k::SparseKKT) = (out = zeros(4); kkt_check(ccall((:calipso_hip_sparse_kkt_differentiate_adjoint_info, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}), k.handle, out), k, "differentiate_adjoint_info"); out)
sparse_differentiate_adjoint_times(k::SparseKKT) = (out = zeros(3); kkt_check(ccall((:calipso_hip_sparse_kkt_differentiate_adjoint_times, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}), k.handle, out), k, "differentiate_adjoint_times"); out)
sparse_differentiate_bytes(k::SparseKKT) = (out = zeros(Int64, 1); kkt_check(ccall((:calipso_hip_sparse_kkt_differentiate_bytes, lib), Int32, (Ptr{Cvoid}, Ptr{Int64}), k.handle, out), k, "differentiate_bytes"); out[1])
# the device forms: device pointers of the handle's device
sparse_solve_columns_device!(k::SparseKKT, X::Ptr{Cvoid}, B::Ptr{Cvoid}, ncols::Integer; transposed::Bool=false) = kkt_check(
    ccall((:calipso_hip_sparse_kkt_solve_columns_device, lib), Int32, (Ptr{Cvoid}, Int64, Int32, Ptr{Cvoid}, Ptr{Cvoid}), k.handle, ncols, transposed ? 1 : 0, B, X), k, "solve_columns_device!")
sparse_differentiate_device!(k::SparseKKT, sensitivity::Ptr{Cvoid}, jacobian_parameters::Ptr{Cvoid}, ncols::Integer) = kkt_check(
    ccall((:calipso_hip_sparse_kkt_differentiate_device, lib), Int32, (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}), k.handle, ncols, jacobian_parameters, sensitivity), k, "differentiate_device!")
sparse_differentiate_adjoint_device!(k::SparseKKT, cotangent::Ptr{Cvoid}, ncols::Integer; adjoint::Ptr{Cvoid}=C_NULL, grad::Union{Nothing,Vector{Ptr{Cvoid}}}=nothing) = GC.@preserve grad kkt_check(
    ccall((:calipso_hip_sparse_kkt_differentiate_adjoint_device, lib), Int32, (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}), k.handle, ncols, cotangent, adjoint,
          grad === nothing ? C_NULL : grad), k, "differentiate_adjoint_device!")

# The handle-resident variant: the KKT blocks are already on the device (uploaded by the evaluation callback or by set_field!), the
# condensed matrix is never formed on the host.  factorize! = calipso_hip_factorize on those blocks with the handle's kappa / rho /
# regularisation scalars (which the caller syncs with sync_scalars!); `A` is accepted for signature parity only.
mutable struct HIPKKTSolver <: CALIPSO.LinearSolver
    hs::HIPSolver
    inertia::CALIPSO.Inertia
end
HIPKKTSolver(hs::HIPSolver) = HIPKKTSolver(hs, CALIPSO.Inertia(0, 0, 0))

"push the reference Solver's iterate and scalars (solver.jl:81-127) to the handle before factorize!/linear_solve! in HIPKKTSolver mode"
function sync_scalars!(hs::HIPSolver)
    s = hs.solver
    set_field!(hs.handle, "solution", s.solution.all)
    for (name, ref) in (("central_path", s.central_path), ("penalty", s.penalty), ("fraction_to_boundary", s.fraction_to_boundary),
                        ("primal_regularization", s.primal_regularization), ("dual_regularization", s.dual_regularization))
        set_field!(hs.handle, name, ref[1])
    end
    return
end

function CALIPSO.factorize!(s::HIPKKTSolver, A=nothing; update=true)
    sync_scalars!(s.hs)
    out = zeros(Int64, 3)
    check(s.hs.handle, ccall((:calipso_hip_factorize, lib), Int32, (Ptr{Cvoid}, Ptr{Int64}), s.hs.handle, out), "factorize!")
    s.inertia.positive, s.inertia.negative, s.inertia.zero = out
    return nothing
end
CALIPSO.compute_inertia!(s::HIPKKTSolver) = nothing      # filled by factorize! (one device pass counts the pivot signs)

function CALIPSO.linear_solve!(s::HIPKKTSolver, x::Vector{Float64}, A, b::Vector{Float64}; fact=true, update=true)
    fact && CALIPSO.factorize!(s, A; update=update)
    set_field!(s.hs.handle, "residual_symmetric", b)
    check(s.hs.handle, ccall((:calipso_hip_linear_solve, lib), Int32, (Ptr{Cvoid},), s.hs.handle), "linear_solve!")
    x .= get_field(s.hs.handle, "step_symmetric", length(b))
    return
end

# ---- search_direction_nonsymmetric! (src/solver/search_direction.jl:106-119): step = H \ residual on the device ---------------
function search_direction_nonsymmetric!(hs::HIPSolver)
    check(hs.handle, ccall((:calipso_hip_search_direction_nonsymmetric, lib), Int32, (Ptr{Cvoid},), hs.handle), "search_direction_nonsymmetric!")
    return
end

# ---- stage-banded structure: what the reference gets from its sparsity pattern (src/trajectory_optimization/sparsity.jl) ---------
"Analyse the non-zero pattern of the blocks currently on the device; afterwards the factorisation and the solves skip everything outside the band of the Schur complement. Returns (half_bandwidth, band_blocks, equality_rows_per_group, cone_rows_per_group)."
function analyze_structure!(hs::HIPSolver)
    out = zeros(Int64, 4)
    check(hs.handle, ccall((:calipso_hip_analyze_structure, lib), Int32, (Ptr{Cvoid}, Ptr{Int64}), hs.handle, out), "analyze_structure!")
    return Tuple(out)
end
clear_structure!(hs::HIPSolver) = check(hs.handle, ccall((:calipso_hip_clear_structure, lib), Int32, (Ptr{Cvoid},), hs.handle), "clear_structure!")
# calipso_hip_set_stage_blocks (after analyze_structure!): packed blocks of [gx; hx] / the Lagrangian Hessian, block mat-vecs, Schur complement by
# segment pairs (csrc/blocks.hip).  Returns (z_blocks, hessian_blocks, segments, packed_doubles).
function set_stage_blocks!(hs::HIPSolver, on::Bool=true)
    out = zeros(Int64, 4)
    check(hs.handle, ccall((:calipso_hip_set_stage_blocks, lib), Int32, (Ptr{Cvoid}, Int32, Ptr{Int64}), hs.handle, on ? 1 : 0, out), "set_stage_blocks!")
    return (z_blocks = out[1], hessian_blocks = out[2], segments = out[3], packed_doubles = out[4])
end

# calipso_hip_kernel_times: [1] ms of the panel-step launches of the last LDL^T of S, [2] their number, [3] NP, [4] bytes of the device slab
function kernel_times(hs::HIPSolver)
    out = zeros(Float64, 8)
    ccall((:calipso_hip_kernel_times, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}), hs.handle, out)
    return out
end

# calipso_hip_schedule_info: [1] Newton steps so far whose prologue ran on the second stream beside the factorisation, [2] where the last step's went (0 main stream,
# 1 forked at the start of the step, 2 handed over while the pivot chain runs), [3] factorisations queued ahead of an exit test that held after all
function schedule_info(hs::HIPSolver)
    out = zeros(Float64, 4)
    ccall((:calipso_hip_schedule_info, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}), hs.handle, out)
    return out
end

# calipso_hip_schur_cache_info: factorisations of a handle with an attached QP that [1] stored the Schur complement's equality products, [2] started from the stored
# ones, [3] could have used them and went without; [4] bytes of the buffer (all zero: the handle has no such cache)
function schur_cache_info(hs::HIPSolver)
    out = zeros(Float64, 4)
    ccall((:calipso_hip_schur_cache_info, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}), hs.handle, out)
    return out
end

"After `analyze_structure!`: factor the Schur complement by the multifrontal sparse LDL' over a nested dissection of its pattern (log2(stages) launches instead of the chain of nx pivots); `batch` >= the largest group this solver leads. Returns (tree levels, largest front, nnz of the pattern, 2)."
function set_stage_parallel!(hs::HIPSolver, on::Bool=true; batch::Integer=1)
    out = zeros(Int64, 4)
    check(hs.handle, ccall((:calipso_hip_set_stage_parallel, lib), Int32, (Ptr{Cvoid}, Int32, Int32, Ptr{Int64}), hs.handle, on ? 1 : 0, batch, out), "set_stage_parallel!")
    return Tuple(out)
end

# ---- groups: many same-shape solvers stepped through the same kernel launches (BASELINE config C4) ------------------------------
"Up to 16 `HIPSolver`s of one shape on one device; `newton_step!` advances every member by one inner iteration of solve!."
mutable struct HIPGroup
    handle::Ptr{Cvoid}
    members::Vector{HIPSolver}
end
function HIPGroup(members::Vector{HIPSolver})
    hs = Ptr{Cvoid}[m.handle for m in members]
    g = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:calipso_hip_group_create, lib), Int32, (Ptr{Ptr{Cvoid}}, Int32, Ptr{Ptr{Cvoid}}), hs, length(hs), g)
    rc == 0 || error("calipso_hip_group_create failed ($rc)")
    grp = HIPGroup(g[], members)
    finalizer(x -> ccall((:calipso_hip_group_destroy, lib), Int32, (Ptr{Cvoid},), x.handle), grp)
    return grp
end
"Do the HIP streams of two handles run side by side?  (calipso_hip_streams_concurrent: measured — a long kernel on one, a short one on the other, both ways)"
function streams_concurrent(a::HIPSolver, b::HIPSolver)
    out = zeros(Float64, 6)
    rc = ccall((:calipso_hip_streams_concurrent, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}), a.handle, b.handle, out)
    rc == 0 || error("calipso_hip_streams_concurrent failed ($rc)")
    return out[1] == 1.0, out[2], out[3], out[4], out[5], out[6]
end
"A new HIP stream (another hardware queue) for the handle: calipso_hip_rebind_stream; priority_class 0, 1, 2 or -1 (keep)."
function rebind_stream!(s::HIPSolver, priority_class::Integer=-1)
    rc = ccall((:calipso_hip_rebind_stream, lib), Int32, (Ptr{Cvoid}, Int32), s.handle, priority_class)
    rc == 0 || error("calipso_hip_rebind_stream failed ($rc)")
    return s
end
"""
Handles (or the first members of groups) that are stepped at the same time from different tasks: probe every pair and give the later one of a colliding pair a new
stream until all run side by side (what `BatchSolver.spread_streams` of the Python mirror does at creation).  Returns the number of streams replaced.
"""
function spread_streams!(leaders::Vector{HIPSolver}; max_rebinds::Integer=12)
    rebinds = 0
    for attempt in 0:max_rebinds
        bad = [(i, j) for j in 1:length(leaders) for i in 1:j-1 if !streams_concurrent(leaders[i], leaders[j])[1]]
        (isempty(bad) || attempt == max_rebinds) && break
        rebind_stream!(leaders[bad[1][2]], (rebinds + bad[1][2]) % 3)
        rebinds += 1
    end
    return rebinds
end
"One inner Newton iteration (solve.jl:98-353) for every member (device evaluator attached); returns (info 6 x B, status B)."
function newton_step!(g::HIPGroup; advance::Bool=true)
    B = length(g.members)
    info = zeros(Float64, 6, B); status = zeros(Int32, B)
    rc = ccall((:calipso_hip_group_newton_step, lib), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Int32}), g.handle, advance ? 1 : 0, info, status)
    rc < 0 && error("calipso_hip_group_newton_step failed ($rc)")
    return info, status
end

"solve! (solve.jl:8-377) of every member in lockstep; members are evaluated through `evaluate_callback` (their own CALIPSO.evaluate!), which finds its solver through the per-member `user` pointer.  Returns the per-member results (1 converged, 0 caps reached, < 0 error code)."
function CALIPSO.solve!(g::HIPGroup)
    members = g.members
    res = zeros(Int32, length(members))
    cb = @cfunction(evaluate_callback, Int32, (Ptr{Cvoid}, UInt32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}))
    evals = fill(cb, length(members))
    GC.@preserve members begin
        users = Ptr{Cvoid}[pointer_from_objref(m) for m in members]
        rc = ccall((:calipso_hip_group_set_evaluators, lib), Int32, (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}), g.handle, evals, users)
        rc < 0 && error("calipso_hip_group_set_evaluators failed ($rc)")
        rc = ccall((:calipso_hip_group_solve, lib), Int32, (Ptr{Cvoid}, Ptr{Int32}), g.handle, res)
        rc < 0 && error("calipso_hip_group_solve failed ($rc): $(last_error(members[1].handle))")
    end
    for (m, r) in zip(members, res)
        r >= 0 && copy_back!(m)
    end
    return res
end

"""differentiate! in reverse mode for every member of the group through the same launches (calipso_hip_group_differentiate_adjoint): `cotangent` N x k x B (dLoss/dw of
every member at its resident point).  Per member what `differentiate_adjoint!` gives on the handle alone without correction rounds: `adjoint` N x k x B, `theta`
np x k x B (the parameter Jacobians through `evaluate_callback`, as `solve!` of the group evaluates), `qp`: names out of "PqAbGh" on members with an attached QP
(matrices rows x nx x k x B).  Returns a NamedTuple (adjoint, theta, qp::Dict, status, ms)."""
function differentiate_adjoint!(g::HIPGroup, cotangent::AbstractArray{Float64,3}; adjoint::Bool = true, theta::Bool = g.members[1].solver.dimensions.parameters > 0, qp::AbstractString = "")
    members = g.members
    d = members[1].solver.dimensions
    B = length(members)
    (size(cotangent, 1) == d.total && size(cotangent, 3) == B) || throw(ArgumentError("cotangent must be N x k x members"))
    V = Array{Float64,3}(cotangent)
    k = size(V, 2)
    nx, ne, nc = d.variables, d.equality_dual, d.cone_dual
    sizes = Dict('P' => (nx, nx), 'q' => (nx,), 'A' => (ne, nx), 'b' => (ne,), 'G' => (nc, nx), 'h' => (nc,))
    all(c -> haskey(sizes, c), qp) || throw(ArgumentError("qp must be made of names out of PqAbGh"))
    adj = adjoint ? zeros(Float64, d.total, k, B) : nothing
    gth = theta ? zeros(Float64, max(d.parameters, 1), k, B) : nothing
    gq = Dict{Char,Array{Float64}}(c => zeros(Float64, sizes[c]..., k, B) for c in qp)
    ptrs = Ptr{Float64}[haskey(gq, c) ? pointer(gq[c]) : Ptr{Float64}(C_NULL) for c in "PqAbGh"]
    opt(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    status = zeros(Int32, B); ms = Ref{Float64}(0.0)
    cb = @cfunction(evaluate_callback, Int32, (Ptr{Cvoid}, UInt32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}))
    evals = fill(cb, B)
    GC.@preserve members V adj gth gq ptrs begin
        users = Ptr{Cvoid}[pointer_from_objref(m) for m in members]
        rc = ccall((:calipso_hip_group_set_evaluators, lib), Int32, (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}), g.handle, evals, users)
        rc < 0 && error("calipso_hip_group_set_evaluators failed ($rc)")
        rc = ccall((:calipso_hip_group_differentiate_adjoint, lib), Int32,
            (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Ptr{Float64}}, Ptr{Int32}, Ptr{Float64}),
            g.handle, k, V, opt(adj), opt(gth), isempty(qp) ? Ptr{Ptr{Float64}}(C_NULL) : pointer(ptrs), status, ms)
        rc < 0 && error("calipso_hip_group_differentiate_adjoint failed ($rc): $(last_error(members[1].handle))")
    end
    return (adjoint = adj, theta = theta ? gth[1:d.parameters, :, :] : nothing, qp = gq, status = status, ms = ms[])
end

"""differentiate! for every member of the group through the same launches (calipso_hip_group_differentiate; differentiate.jl:1-61): per member what `differentiate!` gives
on the handle alone without correction rounds (the parameter Jacobians through `evaluate_callback`, as `solve!` of the group evaluates).  `tile`: columns per workgroup
of the batched products, 0 = the library's choice, 16 or 64 (the same bits either way).  Every member's `solver.data.solution_sensitivity` is filled.  Returns a
NamedTuple (sensitivity N x np x B, status, ms = (whole call, column pass))."""
function CALIPSO.differentiate!(g::HIPGroup; tile::Integer = 0)
    members = g.members
    d = members[1].solver.dimensions
    B = length(members)
    sens = zeros(Float64, d.total, d.parameters, B)
    status = zeros(Int32, B); ms = zeros(Float64, 2)
    cb = @cfunction(evaluate_callback, Int32, (Ptr{Cvoid}, UInt32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}))
    evals = fill(cb, B)
    GC.@preserve members sens begin
        users = Ptr{Cvoid}[pointer_from_objref(m) for m in members]
        rc = ccall((:calipso_hip_group_set_evaluators, lib), Int32, (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}), g.handle, evals, users)
        rc < 0 && error("calipso_hip_group_set_evaluators failed ($rc)")
        rc = ccall((:calipso_hip_group_differentiate, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int32}, Int32, Ptr{Float64}), g.handle, sens, status, tile, ms)
        rc < 0 && error("calipso_hip_group_differentiate failed ($rc): $(last_error(members[1].handle))")
    end
    for (i, m) in enumerate(members)
        m.solver.data.solution_sensitivity .= sens[:, :, i]
    end
    return (sensitivity = sens, status = status, ms = (ms[1], ms[2]))
end

# ---- solve! for a batch of small QPs in one kernel launch (include/calipso_hip.h: calipso_hip_smallnewton_*; csrc/smallnewton.hip) ----------------
"`batch` independent QPs (min c x'Px + q'x s.t. Ax = b, h - Gx >= 0) of one shape: `HIPSmallNewton(nx, ne, nc, batch)`, `set_qp!` (or `set_evaluator!` + `set_parameters!` for a nonlinear problem with a device evaluator), `initialize!`, `solve!`, `differentiate!` — every instance's whole solve! in ONE launch."
mutable struct HIPSmallNewton
    handle::Ptr{Cvoid}
    nx::Int; ne::Int; nc::Int; batch::Int
    np::Int                     # parameters of the device evaluator (set_evaluator!), 0 for a QP
end
function HIPSmallNewton(nx::Integer, ne::Integer, nc::Integer, batch::Integer; device::Integer=0)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:calipso_hip_smallnewton_create, lib), Int32, (Int64, Int64, Int64, Int64, Int32, Ptr{Ptr{Cvoid}}), nx, ne, nc, batch, device, h)
    rc == 0 || error("calipso_hip_smallnewton_create failed ($rc): " * unsafe_string(ccall((:calipso_hip_smallnewton_last_error, lib), Cstring, (Ptr{Cvoid},), h[])))
    s = HIPSmallNewton(h[], nx, ne, nc, batch, 0)
    finalizer(x -> ccall((:calipso_hip_smallnewton_destroy, lib), Int32, (Ptr{Cvoid},), x.handle), s)
    return s
end
sn_check(s::HIPSmallNewton, rc, what) = rc < 0 ? error("$what failed ($rc): " * unsafe_string(ccall((:calipso_hip_smallnewton_last_error, lib), Cstring, (Ptr{Cvoid},), s.handle))) : rc
"options.jl:6-59 by name (Symbol or String), plus `threads` (0, 64, 128, 256) and `lu_fallback` (0 or 1: `H \\ residual` in the kernel where iterative refinement fails, batch x N^2 doubles of device memory)"
function set_option!(s::HIPSmallNewton, name, value::Real)
    sn_check(s, ccall((:calipso_hip_smallnewton_set_option, lib), Int32, (Ptr{Cvoid}, Cstring, Float64), s.handle, String(name), Float64(value)), "calipso_hip_smallnewton_set_option($name)")
    return s
end
"cone layout: the first `n_nonnegative` cone entries nonnegative, then second-order cones of the given dimensions (contiguous; 2 .. 16 entries each)"
function set_cones!(s::HIPSmallNewton, n_nonnegative::Integer, dims::Vector{Int64}=Int64[])
    sn_check(s, ccall((:calipso_hip_smallnewton_set_cones, lib), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}), s.handle, n_nonnegative, length(dims), isempty(dims) ? C_NULL : dims), "calipso_hip_smallnewton_set_cones")
end
"column-major arrays of ONE problem (shared = true) or stacked along a trailing batch dimension: P (nx, nx[, batch]), A (ne, nx[, batch]), G (nc, nx[, batch])"
function set_qp!(s::HIPSmallNewton, P, q, A, b, G, h; objective_scale::Float64=0.5, shared::Bool=ndims(P) == 2)
    f(a) = isempty(a) ? zeros(1) : collect(Float64, vec(a))
    sn_check(s, ccall((:calipso_hip_smallnewton_set_qp, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Int32),
                      s.handle, f(P), f(q), f(A), f(b), f(G), f(h), objective_scale, shared ? 1 : 0), "calipso_hip_smallnewton_set_qp")
    s.np = 0
end
"initialize!(solver, guess) for every instance: x0 is nx x batch"
function CALIPSO.initialize!(s::HIPSmallNewton, x0::AbstractMatrix)
    N = s.nx + 2 * s.ne + 3 * s.nc
    w = zeros(N, s.batch); w[1:s.nx, :] .= x0
    sn_check(s, ccall((:calipso_hip_smallnewton_set_state, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), s.handle, w, C_NULL, C_NULL), "calipso_hip_smallnewton_set_state")
end
"solve!(solver) for every instance in one launch: (result per instance, launch milliseconds)"
function CALIPSO.solve!(s::HIPSmallNewton)
    res = zeros(Int32, s.batch); ms = Ref{Float64}(0.0)
    sn_check(s, ccall((:calipso_hip_smallnewton_solve, lib), Int32, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Float64}), s.handle, res, ms), "calipso_hip_smallnewton_solve")
    return res, ms[]
end
"differentiate!(solver) for every instance in one launch (differentiate.jl:1-61): jacobian_parameters is N x p x batch (dR/dtheta per instance) or N x p (one matrix for all); returns (sensitivity N x p x batch, status, ms)"
function CALIPSO.differentiate!(s::HIPSmallNewton, jacobian_parameters::AbstractArray{Float64})
    N = s.nx + 2 * s.ne + 3 * s.nc
    shared = ndims(jacobian_parameters) == 2
    size(jacobian_parameters, 1) == N && (shared || size(jacobian_parameters, 3) == s.batch) || error("jacobian_parameters must be N x p x batch or N x p")
    p = size(jacobian_parameters, 2)
    J = Array{Float64}(jacobian_parameters); sens = zeros(N, p, s.batch); st = zeros(Int32, s.batch); ms = Ref{Float64}(0.0)
    sn_check(s, ccall((:calipso_hip_smallnewton_differentiate, lib), Int32, (Ptr{Cvoid}, Int64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}), s.handle, p, shared ? 1 : 0, J, sens, st, ms), "calipso_hip_smallnewton_differentiate")
    return sens, st, ms[]
end
"differentiate!(solver) with dR/dtheta from the device evaluator at the resident points (p = n_parameters): (sensitivity N x p x batch, status, ms)"
function CALIPSO.differentiate!(s::HIPSmallNewton)
    N = s.nx + 2 * s.ne + 3 * s.nc
    sens = zeros(N, max(s.np, 1), s.batch); st = zeros(Int32, s.batch); ms = Ref{Float64}(0.0)
    sn_check(s, ccall((:calipso_hip_smallnewton_differentiate_parameters, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}), s.handle, sens, st, ms), "calipso_hip_smallnewton_differentiate_parameters")
    return sens, st, ms[]
end
"""differentiate! in reverse mode for every instance in one launch (calipso_hip_smallnewton_differentiate_adjoint): cotangent N x k x batch (dLoss/dw per
instance; an N x batch matrix is k = 1); returns (adjoint N x k x batch = M'v or nothing, grad_theta n_parameters x k x batch = -R_theta' lambda with the
evaluator's dR/dtheta or nothing, grad_qp nqp x k x batch — P, q, A, b, G, h in set_qp!'s column-major block order — or nothing, status, ms)"""
function differentiate_adjoint!(s::HIPSmallNewton, cotangent::AbstractArray{Float64}; adjoint::Bool=true, theta::Bool=s.np > 0, qp::Bool=s.np == 0)
    N = s.nx + 2 * s.ne + 3 * s.nc
    V = ndims(cotangent) == 2 ? reshape(Array{Float64}(cotangent), N, 1, s.batch) : Array{Float64}(cotangent)
    size(V, 1) == N && size(V, 3) == s.batch || error("cotangent must be N x k x batch or N x batch")
    k = size(V, 2)
    nqp = s.nx * s.nx + s.nx + s.ne * s.nx + s.ne + s.nc * s.nx + s.nc
    adj = adjoint ? zeros(N, k, s.batch) : nothing
    gth = theta ? zeros(max(s.np, 1), k, s.batch) : nothing
    gqp = qp ? zeros(nqp, k, s.batch) : nothing
    st = zeros(Int32, s.batch); ms = Ref{Float64}(0.0)
    ptr(a) = a === nothing ? Ptr{Float64}(C_NULL) : pointer(a)
    GC.@preserve V adj gth gqp sn_check(s, ccall((:calipso_hip_smallnewton_differentiate_adjoint, lib), Int32,
        (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}), s.handle, k, V, ptr(adj), ptr(gth), ptr(gqp), st, ms),
        "calipso_hip_smallnewton_differentiate_adjoint")
    return adj, gth, gqp, st, ms[]
end
"""a device evaluator instead of the QP: `symbol` is the entry CALIPSO_SMALLNEWTON_EVALUATOR (include/calipso_smallnewton.hpp) emitted into the HIP shared library at
`library` (INTEGRATION.md, "Writing an evaluator for the batched kernel"); n_parameters = length of theta per instance"""
function set_evaluator!(s::HIPSmallNewton, library::AbstractString, symbol::Symbol, n_parameters::Integer)
    fn = Libdl.dlsym(Libdl.dlopen(library), symbol)
    sn_check(s, ccall((:calipso_hip_smallnewton_set_evaluator, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), s.handle, fn, n_parameters), "calipso_hip_smallnewton_set_evaluator($symbol)")
    s.np = Int(n_parameters)
end
"theta: n_parameters x batch (column k for instance k) or one n_parameters vector for all"
function set_parameters!(s::HIPSmallNewton, theta::AbstractVecOrMat)
    shared = ndims(theta) == 1
    size(theta, 1) == s.np && (shared || size(theta, 2) == s.batch) || error("theta must be n_parameters x batch or n_parameters")
    sn_check(s, ccall((:calipso_hip_smallnewton_set_parameters, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int32), s.handle, Array{Float64}(theta), shared ? 1 : 0), "calipso_hip_smallnewton_set_parameters")
end
"solution.all of every instance (N x batch)"
function solution(s::HIPSmallNewton)
    N = s.nx + 2 * s.ne + 3 * s.nc
    w = zeros(N, s.batch)
    sn_check(s, ccall((:calipso_hip_smallnewton_get_state, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}), s.handle, w, C_NULL, C_NULL, C_NULL), "calipso_hip_smallnewton_get_state")
    return w
end

# ---- the device-resident, stream-ordered entries of the batch kernel (include/calipso_hip.h: calipso_hip_smallnewton_*_device; csrc/smallnewton_io.hip) ----
# Every array argument is a DEVICE pointer on the handle's device (e.g. `Ptr{Float64}(UInt(pointer(a)))` of an AMDGPU.jl ROCArray; column-major Julia arrays:
# row_major = false); the work is enqueued on the handle's stream and nothing waits for it.  C_NULL skips an optional argument.
const DevPtr = Ptr{Float64}
"all later work of the handle on the caller's hipStream_t (`stream`: a pointer; C_NULL = the legacy default stream), or `nothing`: back to the handle's own stream"
function set_stream!(s::HIPSmallNewton, stream::Union{Nothing,Ptr{Cvoid}})
    sn_check(s, ccall((:calipso_hip_smallnewton_set_stream, lib), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32), s.handle, stream === nothing ? C_NULL : stream, stream === nothing ? 0 : 1), "calipso_hip_smallnewton_set_stream")
end
"set_qp! from device arrays; bit i of shared_mask: array i of P, q, A, b, G, h is one array for all instances"
function set_qp_device!(s::HIPSmallNewton, P::DevPtr, q::DevPtr, A::DevPtr, b::DevPtr, G::DevPtr, h::DevPtr; objective_scale::Float64=0.5, shared_mask::Integer=0, row_major::Bool=false)
    sn_check(s, ccall((:calipso_hip_smallnewton_set_qp_device, lib), Int32, (Ptr{Cvoid}, DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, Float64, Int32, Int32),
                      s.handle, P, q, A, b, G, h, objective_scale, shared_mask, row_major ? 1 : 0), "calipso_hip_smallnewton_set_qp_device")
    s.np = 0
    return s
end
"initialize! with the guesses on the device (nx x batch), or zeros (C_NULL)"
initialize_device!(s::HIPSmallNewton, x0::DevPtr=DevPtr(C_NULL)) =
    sn_check(s, ccall((:calipso_hip_smallnewton_initialize_device, lib), Int32, (Ptr{Cvoid}, DevPtr), s.handle, x0), "calipso_hip_smallnewton_initialize_device")
"points (N x batch), lambda (ne x batch), [central_path, fraction_to_boundary, penalty] (3 x batch) from the device; C_NULL leaves what is resident"
set_state_device!(s::HIPSmallNewton, w::DevPtr, lambda::DevPtr=DevPtr(C_NULL), scalars::DevPtr=DevPtr(C_NULL)) =
    sn_check(s, ccall((:calipso_hip_smallnewton_set_state_device, lib), Int32, (Ptr{Cvoid}, DevPtr, DevPtr, DevPtr), s.handle, w, lambda, scalars), "calipso_hip_smallnewton_set_state_device")
"theta on the device: n_parameters x batch, or one n_parameters vector for all (shared)"
set_parameters_device!(s::HIPSmallNewton, theta::DevPtr; shared::Bool=false) =
    sn_check(s, ccall((:calipso_hip_smallnewton_set_parameters_device, lib), Int32, (Ptr{Cvoid}, DevPtr, Int32), s.handle, theta, shared ? 1 : 0), "calipso_hip_smallnewton_set_parameters_device")
"solve! of every instance, enqueued: nothing is read back (solution_device!)"
solve_device!(s::HIPSmallNewton) = sn_check(s, ccall((:calipso_hip_smallnewton_solve_device, lib), Int32, (Ptr{Cvoid},), s.handle), "calipso_hip_smallnewton_solve_device")
"x (nx x batch), y (ne x batch), z (nc x batch), w (N x batch) and the Int32 status of the last solve (batch) into device arrays; C_NULL skips one"
solution_device!(s::HIPSmallNewton; x::DevPtr=DevPtr(C_NULL), y::DevPtr=DevPtr(C_NULL), z::DevPtr=DevPtr(C_NULL), w::DevPtr=DevPtr(C_NULL), status::Ptr{Int32}=Ptr{Int32}(C_NULL)) =
    sn_check(s, ccall((:calipso_hip_smallnewton_get_solution_device, lib), Int32, (Ptr{Cvoid}, DevPtr, DevPtr, DevPtr, DevPtr, Ptr{Int32}), s.handle, x, y, z, w, status), "calipso_hip_smallnewton_get_solution_device")
"""differentiate_adjoint! on the device: k cotangent columns as `cot_w` (N x k x batch) or as the parts `cot_x`, `cot_y`, `cot_z`; `adjoint` (N x k x batch) and
`grad_theta` (n_parameters x k x batch) are written by the launch; `grad_qp`: six device pointers (P, q, A, b, G, h; C_NULL skips one), per instance (size x k x batch)
or, with bit i of `reduce_mask`, summed over the batch on the device (size x k).  Gradients of instances whose solve status is not 1 are NaN."""
function differentiate_adjoint_device!(s::HIPSmallNewton, k::Integer; cot_w::DevPtr=DevPtr(C_NULL), cot_x::DevPtr=DevPtr(C_NULL), cot_y::DevPtr=DevPtr(C_NULL), cot_z::DevPtr=DevPtr(C_NULL),
                                       adjoint::DevPtr=DevPtr(C_NULL), grad_theta::DevPtr=DevPtr(C_NULL), grad_qp::Union{Nothing,Vector{DevPtr}}=nothing, reduce_mask::Integer=0,
                                       row_major::Bool=false, status::Ptr{Int32}=Ptr{Int32}(C_NULL))
    grad_qp === nothing || length(grad_qp) == 6 || error("grad_qp: six device pointers (P, q, A, b, G, h)")
    gq = grad_qp === nothing ? Ptr{DevPtr}(C_NULL) : pointer(grad_qp)
    GC.@preserve grad_qp sn_check(s, ccall((:calipso_hip_smallnewton_differentiate_adjoint_device, lib), Int32,
        (Ptr{Cvoid}, Int64, DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, DevPtr, Ptr{DevPtr}, Int32, Int32, Ptr{Int32}),
        s.handle, k, cot_w, cot_x, cot_y, cot_z, adjoint, grad_theta, gq, reduce_mask, row_major ? 1 : 0, status), "calipso_hip_smallnewton_differentiate_adjoint_device")
end

# ---- multi-GPU exchange (include/calipso_hip.h: calipso_hip_comm_*): RCCL over xGMI, one process per GPU -------------------------
"RCCL communicator: `id = comm_unique_id()` on one rank, distributed by the launcher (file / MPI / Distributed.jl), then `HIPComm(rank, nranks, id; device)` on every rank."
mutable struct HIPComm
    handle::Ptr{Cvoid}
    rank::Int
    nranks::Int
end
function comm_unique_id()
    id = zeros(UInt8, 128)
    rc = ccall((:calipso_hip_comm_unique_id, lib), Int32, (Ptr{UInt8},), id)
    rc == 0 || error("calipso_hip_comm_unique_id failed ($rc)")
    return id
end
function HIPComm(rank::Integer, nranks::Integer, id::Vector{UInt8}; device::Integer=0)
    c = Ref{Ptr{Cvoid}}(C_NULL)
    rc = ccall((:calipso_hip_comm_init, lib), Int32, (Int32, Int32, Ptr{UInt8}, Int32, Ptr{Ptr{Cvoid}}), rank, nranks, id, device, c)
    rc == 0 || error("calipso_hip_comm_init failed ($rc)")
    comm = HIPComm(c[], rank, nranks)
    finalizer(x -> ccall((:calipso_hip_comm_destroy, lib), Int32, (Ptr{Cvoid},), x.handle), comm)
    return comm
end
"(ranks, own rank) as the live communicator reports them (ncclCommCount / ncclCommUserRank)"
function comm_size(c::HIPComm)
    out = zeros(Int32, 2)
    rc = ccall((:calipso_hip_comm_size, lib), Int32, (Ptr{Cvoid}, Ptr{Int32}), c.handle, out)
    rc == 0 || error("calipso_hip_comm_size failed ($rc)")
    return Int(out[1]), Int(out[2])
end
"all-gather of the per-problem status rows (4 x k Int32 per rank, k may differ) in global problem-id order; `capacity` = total rows"
function gather_status(c::HIPComm, rows::Matrix{Int32}, capacity::Integer)
    out = zeros(Int32, 4, capacity); counts = zeros(Int64, c.nranks)
    n = ccall((:calipso_hip_comm_gather_status, lib), Int64, (Ptr{Cvoid}, Ptr{Int32}, Int64, Ptr{Int32}, Int64, Ptr{Int64}), c.handle, rows, size(rows, 2), out, capacity, counts)
    n < 0 && error("calipso_hip_comm_gather_status failed ($n)")
    return out[:, 1:n], counts
end
function allreduce_sum!(c::HIPComm, v::Vector{Float64})
    rc = ccall((:calipso_hip_comm_allreduce_sum, lib), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64), c.handle, v, length(v))
    rc == 0 || error("calipso_hip_comm_allreduce_sum failed ($rc)")
    return v
end

export SparseKKT, set_values!, set_values_device!, kkt_info, kkt_pattern, kkt_factorize!, kkt_matrix!, kkt_mul!, solve_symmetric!, sparse_search_direction!, sparse_search_direction_device!, kkt_timing, qp_attach!, sparse_initialize!, sparse_solve!, sparse_get, sparse_set!
export SparseKKTGroup, group_info, group_pattern, group_factorize!, group_matrix!, group_mul!, group_search_direction!, group_search_direction_device!, group_timing
export sparse_solve_columns!, sparse_differentiate!,sparse_differentiate_adjoint!, sparse_differentiate_info, sparse_differentiate_adjoint_info, sparse_differentiate_adjoint_times, sparse_differentiate_bytes, sparse_solve_columns_device!, sparse_differentiate_device!, sparse_differentiate_adjoint_device!
export HIPSolver, streams_concurrent, rebind_stream!, spread_streams!, HIPLDLSolver, HIPSparseLDLSolver, hip_sparse_ldl_solver, HIPKKTSolver, hip_ldl_solver, HIPGroup, HIPSmallNewton, set_option!, set_cones!, set_qp!, set_evaluator!, set_parameters!, differentiate_adjoint!, solution, set_stream!, set_qp_device!, initialize_device!, set_state_device!, set_parameters_device!, solve_device!, solution_device!, differentiate_adjoint_device!, HIPComm, comm_unique_id, comm_size, gather_status, allreduce_sum!, newton_step!,
       search_direction_nonsymmetric!, analyze_structure!, clear_structure!, set_stage_parallel!, set_stage_blocks!, declared_structure, kernel_times, sync_scalars!, copy_back!

end # module
