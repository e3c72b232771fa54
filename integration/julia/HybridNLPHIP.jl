# HybridNLPHIP.jl -- the reference-side binding: a drop-in MOI.AbstractNLPEvaluator that forwards the
# callbacks of /root/reference/src/moi.jl:1-33 to libqln_hip.so (C ABI: include/qln_evaluator.h).
#
# NOT EXECUTED in this pipeline (no Julia on either box) -- kept free of arithmetic so that review by
# reading is credible: every evaluator method is one ccall.  Usage inside the reference's notebook, after
# `include("nlp.jl")`, `include("moi.jl")` etc.:
#     nlp = HybridNLPHIP(model, obj, init_mode, k_trans, N, xinit, xterm)
#     Z_sol, solver = solve(Z0, nlp, c_tol=1e-3, tol=1e-3)    # dispatches to the method at the END OF THIS FILE
# The reference's own `solve` is typed `solve(x0, prob::HybridNLP; ...)` (src/moi.jl:46) and HybridNLP is a concrete
# struct (src/nlp.jl:13), so it cannot take this type; this file therefore adds a second METHOD of the same generic
# function `solve` for HybridNLPHIP (same keywords, same Ipopt options, same bounds) -- src/moi.jl itself is not edited.
# tests/test_julia_binding.py holds every ccall and struct of this file to include/qln_evaluator.h (symbol, argument
# count, pointer / integer / double class of every argument, field order and width of the three structs).
using LinearAlgebra        # diag
using MathOptInterface
const MOI = MathOptInterface
const LIBQLN = get(ENV, "QLN_LIB", joinpath(@__DIR__, "..", "..", "quadruped_landing_amd", "csrc", "libqln_hip.so"))

struct QlnModel; g::Cdouble; mb::Cdouble; mf::Cdouble; lb::Cdouble; l1::Cdouble; l2::Cdouble; end
struct QlnBatchDesc
    B::Int32; N::Int32; model::QlnModel
    k_trans::Ptr{Int32}; init_mode::Ptr{Int32}; x0::Ptr{Cdouble}; xf::Ptr{Cdouble}; cost::Ptr{Cdouble}
    cost_batch::Int32; z_stride::Int64; align::Int32
    jac_format::Int32      # 0 = dense 15x20 step blocks, 1 = structural non-zeros only (QLN_JAC_FORMAT_*)
end

qln_check(rc) = rc == 0 || error("libqln_hip: " * unsafe_string(ccall((:qln_last_error, LIBQLN), Cstring, ())))

mutable struct HybridNLPHIP <: MOI.AbstractNLPEvaluator
    handle::Ptr{Cvoid}
    N::Int; k_trans::Int; init_mode::Int
    lb::Vector{Float64}; ub::Vector{Float64}      # fields solve() reads (src/moi.jl:69)
    n_nlp::Int; m_nlp::Int
    use_sparse_jacobian::Bool
    exact_hessian::Bool                           # offer :Hess (the reference offers none: Ipopt falls back to L-BFGS)
    matrix_free::Bool                             # offer :JacVec and :HessVec (products, nothing stored)
end

# HybridNLP(model, obj, init_mode, k_trans, N, x0, xf) -- src/nlp.jl:34-37.  `obj` is the reference's
# Vector{QuadraticCost}; it is flattened to the 41-double records [Q(15) R(5) q(15) r(5) c].
function HybridNLPHIP(model, obj, init_mode, k_trans, N, x0, xf; use_sparse_jacobian=false, device=0, exact_hessian=false,
                      matrix_free=false)
    # a sparse solve wants only the entries that can be non-zero; the dense callback needs neither format in particular
    jac_format = use_sparse_jacobian ? 1 : 0
    cost = vcat([[diag(o.Q); diag(o.R); o.q; o.r; o.c] for o in obj]...)
    kt = Int32[k_trans]; im = Int32[init_mode]; x0v = collect(Float64, x0); xfv = collect(Float64, xf)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve cost kt im x0v xfv begin
        d = Ref(QlnBatchDesc(1, N, QlnModel(model.g, model.mb, model.mf, model.lb, model.l1, model.l2),
                             pointer(kt), pointer(im), pointer(x0v), pointer(xfv), pointer(cost), 1, 0, 0, jac_format))
        qln_check(ccall((:qln_create, LIBQLN), Cint, (Ref{QlnBatchDesc}, Cint, Ref{Ptr{Cvoid}}), d, device, h))
    end
    m = Ref{Int32}(0); nnz = Ref{Int32}(0)
    qln_check(ccall((:qln_problem_dims, LIBQLN), Cint, (Ptr{Cvoid}, Int32, Ref{Int32}, Ref{Int32}), h[], 0, m, nnz))
    lb = zeros(m[]); ub = zeros(m[])
    qln_check(ccall((:qln_constraint_bounds, LIBQLN), Cint, (Ptr{Cvoid}, Int32, Ptr{Cdouble}, Ptr{Cdouble}), h[], 0, lb, ub))
    nlp = HybridNLPHIP(h[], N, k_trans, init_mode, lb, ub, 20N - 5, m[], use_sparse_jacobian, exact_hessian, matrix_free)
    finalizer(p -> ccall((:qln_destroy, LIBQLN), Cint, (Ptr{Cvoid},), p.handle), nlp)
end

num_primals(nlp::HybridNLPHIP) = nlp.n_nlp      # src/nlp.jl:86
num_duals(nlp::HybridNLPHIP) = nlp.m_nlp        # src/nlp.jl:87

function MOI.eval_objective(prob::HybridNLPHIP, x)                      # src/moi.jl:1-3
    f = Ref{Cdouble}(0.0)
    qln_check(ccall((:qln_eval_objective_host, LIBQLN), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ref{Cdouble}), prob.handle, x, f))
    return f[]
end
function MOI.eval_objective_gradient(prob::HybridNLPHIP, grad_f, x)     # src/moi.jl:5-8
    qln_check(ccall((:qln_eval_objective_gradient_host, LIBQLN), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), prob.handle, x, grad_f))
    return nothing
end
function MOI.eval_constraint(prob::HybridNLPHIP, g, x)                  # src/moi.jl:10-13
    qln_check(ccall((:qln_eval_constraint_host, LIBQLN), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), prob.handle, x, g))
    return nothing
end
function MOI.eval_constraint_jacobian(prob::HybridNLPHIP, vec, x)       # src/moi.jl:15-24
    if prob.use_sparse_jacobian   # vec has one slot per entry of jacobian_structure (block-COO order)
        qln_check(ccall((:qln_eval_constraint_jacobian_host, LIBQLN), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}), prob.handle, x, vec))
    else                          # dense column-major m_nlp x n_nlp; only jac_c!'s write-set is assigned
        qln_check(ccall((:qln_eval_constraint_jacobian_dense_host, LIBQLN), Cint, (Ptr{Cvoid}, Int32, Ptr{Cdouble}, Ptr{Cdouble}), prob.handle, 0, x, vec))
    end
    return nothing
end
# src/moi.jl:26-28 offers [:Grad, :Jac]; with exact_hessian=true :Hess too, and Ipopt stops forcing L-BFGS by itself
# and with matrix_free=true :JacVec, :HessVec after them
function MOI.features_available(prob::HybridNLPHIP)
    feats = prob.exact_hessian ? [:Grad, :Jac, :Hess] : [:Grad, :Jac]
    return prob.matrix_free ? vcat(feats, [:JacVec, :HessVec]) : feats
end
MOI.initialize(prob::HybridNLPHIP, features) = nothing                  # src/moi.jl:30
function MOI.jacobian_structure(nlp::HybridNLPHIP)                      # src/moi.jl:31-33
    if !nlp.use_sparse_jacobian
        return vec(Tuple.(CartesianIndices(zeros(num_duals(nlp), num_primals(nlp)))))
    end
    nnz = Ref{Int32}(0)
    qln_check(ccall((:qln_problem_dims, LIBQLN), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}, Ref{Int32}), nlp.handle, 0, C_NULL, nnz))
    rows = zeros(Int32, nnz[]); cols = zeros(Int32, nnz[])
    qln_check(ccall((:qln_jacobian_structure, LIBQLN), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int32}), nlp.handle, 0, rows, cols))
    return [(Int(r) + 1, Int(c) + 1) for (r, c) in zip(rows, cols)]     # the ABI is 0-based
end

# The Hessian of the Lagrangian, sigma d2 eval_f + sum_i mu_i d2 c_i, as the lower triangle of a block-diagonal pattern
# (55 entries per step block, 15 for x_N).  Its objective part is the Hessian of eval_f, the function -- not the Jacobian
# of grad_f!, which has no d(h l)/dh (quirk Q2) and is not symmetric.
function MOI.hessian_lagrangian_structure(nlp::HybridNLPHIP)
    nnz = 55 * (nlp.N - 1) + 15
    rows = zeros(Int32, nnz); cols = zeros(Int32, nnz)
    qln_check(ccall((:qln_hessian_structure, LIBQLN), Cint, (Int32, Ptr{Int32}, Ptr{Int32}), nlp.N, rows, cols))
    return [(Int(r) + 1, Int(c) + 1) for (r, c) in zip(rows, cols)]     # the ABI is 0-based
end
function MOI.eval_hessian_lagrangian(prob::HybridNLPHIP, H, x, sigma, mu)
    s = Ref{Cdouble}(sigma)
    qln_check(ccall((:qln_eval_hessian_lagrangian_host, LIBQLN), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ref{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, x, s, mu, H))
    return nothing
end

# Matrix-free products (:JacVec, :HessVec): the Jacobian and the Hessian of the Lagrangian are re-derived per knot on the
# GPU and contracted there, never stored.  y = J(x) w (m_nlp), y = J(x)' w (n_nlp), h = (sigma d2 f + sum mu_i d2 c_i) v.
function MOI.eval_constraint_jacobian_product(prob::HybridNLPHIP, y, x, w)
    qln_check(ccall((:qln_eval_constraint_jvp_host, LIBQLN), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, x, w, y))
    return nothing
end
function MOI.eval_constraint_jacobian_transpose_product(prob::HybridNLPHIP, y, x, w)
    qln_check(ccall((:qln_eval_constraint_vjp_host, LIBQLN), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, x, w, y))
    return nothing
end
function MOI.eval_hessian_lagrangian_product(prob::HybridNLPHIP, h, x, v, sigma, mu)
    s = Ref{Cdouble}(sigma)
    qln_check(ccall((:qln_eval_hessian_lagrangian_product_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ref{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}), prob.handle, x, s, mu, v, h))
    return nothing
end

# ---- beyond the evaluator: the same NLP solved on the GPU in place of `solve(Z0, nlp)` (src/moi.jl:46-103) -------------
# qln_solve_host: augmented-Lagrangian iLQR, one wavefront per problem (DESIGN.md 4.6); objective, constraint bounds and the
# variable bounds of solve() (quirk Q6 included) are the reference's.  Field order = include/qln_evaluator.h.
struct QlnSolveOptions
    max_outer::Int32; max_inner::Int32
    tol_violation::Cdouble; inner_tol::Cdouble
    rho0::Cdouble; rho_factor::Cdouble; rho_max::Cdouble
    h_min::Cdouble; h_max::Cdouble; theta_min::Cdouble; theta_max::Cdouble
    q6_bounds::Int32; exact_h_gradient::Int32
    h_prox::Cdouble
    rescue_outer::Int32
end

function solve_hip(x0, prob::HybridNLPHIP; c_tol=1.0e-6)
    opt = Ref{QlnSolveOptions}()
    qln_check(ccall((:qln_solve_default_options, LIBQLN), Cint, (Ref{QlnSolveOptions},), opt))
    o = opt[]
    opt[] = QlnSolveOptions(o.max_outer, o.max_inner, c_tol, o.inner_tol, o.rho0, o.rho_factor, o.rho_max, o.h_min, o.h_max,
                            o.theta_min, o.theta_max, o.q6_bounds, o.exact_h_gradient, o.h_prox, o.rescue_outer)
    Z = collect(Float64, x0)             # in: initial guess (its controls are used); out: the solution
    info = zeros(16)                     # {outer, iLQR iterations, f, violation, rho, status, ...}
    qln_check(ccall((:qln_solve_host, LIBQLN), Cint, (Ptr{Cvoid}, Ptr{Cdouble}, Ref{QlnSolveOptions}, Ptr{Cdouble}),
                    prob.handle, Z, opt, info))
    return Z, info
end

# ---- is a trajectory optimal?  Least-squares multipliers and the KKT residual (include/qln_evaluator.h, DESIGN.md 4.15) ----
# At any Z (qln_solve's, Ipopt's, a file's): lam over the active set (every equality row, clearance rows with c_i <= act_tol,
# variables within bound_tol of a bound of solve() held fixed), MOI's convention L = f + lam'c.  Returns (lam, lag, info):
# lag = g + J'lam is the dual infeasibility on the free variables and z_L - z_U on the fixed ones, info the 16-entry report
# (info[1] iterations, info[5] max |lag| over the free variables, info[8] / info[9] the wrong-sign counts; 1-based here).
# g = nothing: the reference's grad_f!, what Ipopt sees (no d(h l)/dh, quirk Q2); pass the exact gradient to measure that.
function estimate_multipliers(prob::HybridNLPHIP, Z; g=nothing, act_tol=1.0e-6, bound_tol=1.0e-8, row_scaling::Bool=true,
                              max_iters=20000, rel_tol=1.0e-8)
    x = collect(Float64, Z)
    c = zeros(num_duals(prob)); MOI.eval_constraint(prob, c, x)
    grad = zeros(num_primals(prob))
    g === nothing ? MOI.eval_objective_gradient(prob, grad, x) : copyto!(grad, g)
    lam = zeros(num_duals(prob)); lag = zeros(num_primals(prob)); info = zeros(16)
    qln_check(ccall((:qln_estimate_multipliers_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{QlnSolveOptions}, Cdouble, Cdouble, Int32, Int32,
                     Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, x, c, grad, C_NULL, act_tol, bound_tol, Int32(row_scaling), Int32(max_iters), rel_tol, lam, lag, info))
    return lam, lag, info
end

# ---- TVLQR tracking along solved trajectories (include/qln_evaluator.h, DESIGN.md 4.11) -----------------------------------
# Zref: the problem's reference in the layout of Z; Q, Qf: 15 diagonal weights, R: 4 (the forces).  Returns K as a
# (15, 4, N-1) array (K[:, m, k] = row m of knot k's gain) and P as (120, N) packed lower triangles (or nothing).
function tracking_lqr(prob::HybridNLPHIP, Zref::Vector{Float64}, Q::Vector{Float64}, R::Vector{Float64}, Qf::Vector{Float64};
                      with_cost_to_go::Bool=true)
    N = prob.N
    K = zeros(15, 4, N - 1)
    P = with_cost_to_go ? zeros(120, N) : nothing
    qln_check(ccall((:qln_tracking_lqr_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, Q, R, Qf, K, P === nothing ? C_NULL : P))
    return K, P
end
# closed-loop roll-out (K = nothing: open loop) from x0 (15 values, nothing: the problem's own x0); returns Zout
function tracking_rollout(prob::HybridNLPHIP, Zref::Vector{Float64}; K=nothing, x0=nothing)
    Zout = zeros(length(Zref))
    qln_check(ccall((:qln_tracking_rollout_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, K === nothing ? C_NULL : K, x0 === nothing ? C_NULL : x0, Zout))
    return Zout
end
# reverse sweep of tracking_rollout at the trajectory Zout: the cotangent Zbar (layout of Z, weighting Zout's states and applied
# controls) -> (Zref_bar, K_bar, x0_bar); K = nothing is the shooting gradient (K_bar = nothing).  include/qln_evaluator.h
function tracking_rollout_vjp(prob::HybridNLPHIP, Zref::Vector{Float64}, Zout::Vector{Float64}, Zbar::Vector{Float64}; K=nothing)
    Zref_bar = zeros(length(Zref))
    K_bar = K === nothing ? nothing : zeros(size(K))
    x0_bar = zeros(15)
    qln_check(ccall((:qln_tracking_rollout_vjp_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, K === nothing ? C_NULL : K, Zout, Zbar, Zref_bar, K_bar === nothing ? C_NULL : K_bar,
                    x0_bar))
    return Zref_bar, K_bar, x0_bar
end
# forward sweep of tracking_rollout at the trajectory Zout: the tangents Zref_dot (layout of Z), K_dot (size of K, needs K) and
# x0_dot (15 values) -- each nothing for zero, at least one given -- -> Zout_dot, the tangent of Zout's states and applied
# controls.  The adjoint of tracking_rollout_vjp.  include/qln_evaluator.h, DESIGN.md 4.14
function tracking_rollout_jvp(prob::HybridNLPHIP, Zref::Vector{Float64}, Zout::Vector{Float64}; K=nothing, Zref_dot=nothing,
                              K_dot=nothing, x0_dot=nothing)
    Zout_dot = zeros(length(Zref))
    qln_check(ccall((:qln_tracking_rollout_jvp_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, K === nothing ? C_NULL : K, Zout, Zref_dot === nothing ? C_NULL : Zref_dot,
                    K_dot === nothing ? C_NULL : K_dot, x0_dot === nothing ? C_NULL : x0_dot, Zout_dot))
    return Zout_dot
end
# The roll-out and its two sweeps with a PLANT model of the problem's own (include/qln_evaluator.h, DESIGN.md 4.16): model is
# (g, mb, mf, lb), four values, or nothing (the handle's model); the gains and the reference stay what they are.
# tracking_rollout_model_jvp takes a fourth tangent model_dot (four values), tracking_rollout_model_vjp returns a fourth
# cotangent model_bar (four values).
function tracking_rollout_model(prob::HybridNLPHIP, Zref::Vector{Float64}; K=nothing, x0=nothing, model=nothing)
    Zout = zeros(length(Zref))
    qln_check(ccall((:qln_tracking_rollout_model_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, K === nothing ? C_NULL : K, x0 === nothing ? C_NULL : x0,
                    model === nothing ? C_NULL : model, Zout))
    return Zout
end
function tracking_rollout_model_jvp(prob::HybridNLPHIP, Zref::Vector{Float64}, Zout::Vector{Float64}; K=nothing, model=nothing,
                                    Zref_dot=nothing, K_dot=nothing, x0_dot=nothing, model_dot=nothing)
    Zout_dot = zeros(length(Zref))
    qln_check(ccall((:qln_tracking_rollout_model_jvp_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, K === nothing ? C_NULL : K, Zout, model === nothing ? C_NULL : model,
                    Zref_dot === nothing ? C_NULL : Zref_dot, K_dot === nothing ? C_NULL : K_dot,
                    x0_dot === nothing ? C_NULL : x0_dot, model_dot === nothing ? C_NULL : model_dot, Zout_dot))
    return Zout_dot
end
function tracking_rollout_model_vjp(prob::HybridNLPHIP, Zref::Vector{Float64}, Zout::Vector{Float64}, Zbar::Vector{Float64};
                                    K=nothing, model=nothing)
    Zref_bar = zeros(length(Zref))
    K_bar = K === nothing ? nothing : zeros(size(K))
    x0_bar = zeros(15)
    model_bar = zeros(4)
    qln_check(ccall((:qln_tracking_rollout_model_vjp_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, K === nothing ? C_NULL : K, Zout, model === nothing ? C_NULL : model, Zbar, Zref_bar,
                    K_bar === nothing ? C_NULL : K_bar, x0_bar, model_bar))
    return Zref_bar, K_bar, x0_bar, model_bar
end
# The roll-out with guard-triggered touchdown (include/qln_evaluator.h, DESIGN.md 4.17): contact begins when the free foot
# reaches the ground, not at the problem's k_trans, which is not read.  Returns (Zout, events); events holds 8 values: the
# 0-based knot whose step contains the touchdown (-1: none), tau, the clock at touchdown, the foot's x, its (vx, vy) before the
# jump map, the smallest vertical force under a standing foot, 0.  Zout is not a trajectory of the knot schedule: its
# derivatives are tracking_rollout_guarded_jvp / _vjp below, gains and covariances along it tracking_lqr_guarded and
# tracking_covariance_guarded; the other jvp / vjp / lqr / covariance calls do not apply to it.
function tracking_rollout_guarded(prob::HybridNLPHIP, Zref::Vector{Float64}; K=nothing, x0=nothing, model=nothing)
    Zout = zeros(length(Zref))
    events = zeros(8)
    qln_check(ccall((:qln_tracking_rollout_guarded_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, K === nothing ? C_NULL : K, x0 === nothing ? C_NULL : x0,
                    model === nothing ? C_NULL : model, Zout, events))
    return Zout, events
end
# The sweeps through the guard-triggered touchdown (include/qln_evaluator.h, DESIGN.md 4.18): the derivative of
# tracking_rollout_guarded at the (Zout, events) it returned, at fixed touchdown knot, with the derivative of the touchdown
# time.  Tangents and cotangents are tracking_rollout_model_jvp's / _vjp's; the forward sweep also returns event_dot (8 values:
# d tau in entry 2, the touchdown clock's tangent in entry 3, 1-based, zeros elsewhere).
function tracking_rollout_guarded_jvp(prob::HybridNLPHIP, Zref::Vector{Float64}, Zout::Vector{Float64}, events::Vector{Float64};
                                      K=nothing, model=nothing, Zref_dot=nothing, K_dot=nothing, x0_dot=nothing,
                                      model_dot=nothing)
    Zout_dot = zeros(length(Zref))
    event_dot = zeros(8)
    qln_check(ccall((:qln_tracking_rollout_guarded_jvp_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, K === nothing ? C_NULL : K, Zout, model === nothing ? C_NULL : model, events,
                    Zref_dot === nothing ? C_NULL : Zref_dot, K_dot === nothing ? C_NULL : K_dot,
                    x0_dot === nothing ? C_NULL : x0_dot, model_dot === nothing ? C_NULL : model_dot, Zout_dot, event_dot))
    return Zout_dot, event_dot
end
function tracking_rollout_guarded_vjp(prob::HybridNLPHIP, Zref::Vector{Float64}, Zout::Vector{Float64}, events::Vector{Float64},
                                      Zbar::Vector{Float64}; K=nothing, model=nothing)
    Zref_bar = zeros(length(Zref))
    K_bar = K === nothing ? nothing : zeros(size(K))
    x0_bar = zeros(15)
    model_bar = zeros(4)
    qln_check(ccall((:qln_tracking_rollout_guarded_vjp_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, K === nothing ? C_NULL : K, Zout, model === nothing ? C_NULL : model, events, Zbar,
                    Zref_bar, K_bar === nothing ? C_NULL : K_bar, x0_bar, model_bar))
    return Zref_bar, K_bar, x0_bar, model_bar
end
# covariance of the roll-out's states along the trajectory Zout (for the nominal case: the reference itself):
# Sigma_0 = Sigma0, Sigma_{k+1} = (A_k - B_k K_k) Sigma_k (A_k - B_k K_k)' + diag(W); K = nothing is the open loop.
# Sigma0: a 15x15 matrix (its lower triangle is read); W: 15 variances or nothing (zeros).  Returns Sigma as (120, N) packed
# lower triangles (row i >= j at i(i+1)/2 + j, 0-based) and marg as (8, N): the clearance row's variance, the four force
# variances, the two foot-height variances and the trace, per knot.  include/qln_evaluator.h, DESIGN.md 4.13
function tracking_covariance(prob::HybridNLPHIP, Zout::Vector{Float64}, Sigma0::Matrix{Float64}; K=nothing, W=nothing)
    N = prob.N
    packed = Float64[Sigma0[i, j] for i in 1:15 for j in 1:i]
    Sigma = zeros(120, N)
    marg = zeros(8, N)
    qln_check(ccall((:qln_tracking_covariance_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zout, K === nothing ? C_NULL : K, packed, Int32(1), W === nothing ? C_NULL : W, Sigma, marg))
    return Sigma, marg
end
# Gains and covariances through the guard-triggered touchdown (include/qln_evaluator.h, DESIGN.md 4.19), on the blocks of the
# sweeps above: Ztraj / Zout and events are what tracking_rollout_guarded returned.  tracking_lqr_guarded returns (K, P) as
# tracking_lqr; tracking_covariance_guarded returns (Sigma, marg, event_var) with event_var = (variance of tau, variance of the
# touchdown clock), zeros without a touchdown.
function tracking_lqr_guarded(prob::HybridNLPHIP, Ztraj::Vector{Float64}, events::Vector{Float64}, Q::Vector{Float64},
                              R::Vector{Float64}, Qf::Vector{Float64}; model=nothing, with_cost_to_go::Bool=true)
    N = prob.N
    K = zeros(15, 4, N - 1)
    P = with_cost_to_go ? zeros(120, N) : nothing
    qln_check(ccall((:qln_tracking_lqr_guarded_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}),
                    prob.handle, Ztraj, model === nothing ? C_NULL : model, events, Q, R, Qf, K, P === nothing ? C_NULL : P))
    return K, P
end
function tracking_covariance_guarded(prob::HybridNLPHIP, Zout::Vector{Float64}, events::Vector{Float64}, Sigma0::Matrix{Float64};
                                     K=nothing, W=nothing, model=nothing)
    N = prob.N
    packed = Float64[Sigma0[i, j] for i in 1:15 for j in 1:i]
    Sigma = zeros(120, N)
    marg = zeros(8, N)
    event_var = zeros(2)
    qln_check(ccall((:qln_tracking_covariance_guarded_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zout, K === nothing ? C_NULL : K, model === nothing ? C_NULL : model, events, packed, Int32(1),
                    W === nothing ? C_NULL : W, Sigma, marg, event_var))
    return Sigma, marg, event_var
end
# The Kalman filter and the LQG covariance along Zout (include/qln_evaluator.h, DESIGN.md 4.21): tracking_covariance for a
# controller that feeds back the estimate built from the measurements y_k = H dx_k + v_k.  H: a (ny, 15) matrix, 1 <= ny <= 8;
# V: ny measurement variances (> 0); Sigma0, W as tracking_covariance.  Returns (L, Pest, Sigma, marg): the filter gains as
# (ny, 15, N) (column-major: L[r, i, k] is entry (i, r) of L_k), the error covariances P^+_k and the true state's covariances
# X_k as (120, N) packed lower triangles, marg as (8, N) with the applied-force variances diag(K M K').  K = nothing is the
# filter alone: Sigma and marg are nothing.  tracking_kalman_guarded is the same through the guard-triggered touchdown at the
# (Zout, events) of tracking_rollout_guarded, and also returns event_var (nothing without K).
function tracking_kalman(prob::HybridNLPHIP, Zout::Vector{Float64}, H::Matrix{Float64}, V::Vector{Float64},
                         Sigma0::Matrix{Float64}; K=nothing, W=nothing)
    N = prob.N
    ny = size(H, 1)
    (1 <= ny <= 8 && size(H, 2) == 15 && length(V) == ny) || error("H: (ny, 15) with 1 <= ny <= 8, V: ny variances")
    Hrow = Matrix{Float64}(transpose(H))  # row-major [ny][15]
    packed = Float64[Sigma0[i, j] for i in 1:15 for j in 1:i]
    L = zeros(ny, 15, N)
    Pest = zeros(120, N)
    Sigma = K === nothing ? nothing : zeros(120, N)
    marg = K === nothing ? nothing : zeros(8, N)
    qln_check(ccall((:qln_tracking_kalman_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zout, K === nothing ? C_NULL : K, Hrow, Int32(ny), V, packed, Int32(1),
                    W === nothing ? C_NULL : W, L, Pest, Sigma === nothing ? C_NULL : Sigma, marg === nothing ? C_NULL : marg))
    return L, Pest, Sigma, marg
end
function tracking_kalman_guarded(prob::HybridNLPHIP, Zout::Vector{Float64}, events::Vector{Float64}, H::Matrix{Float64},
                                 V::Vector{Float64}, Sigma0::Matrix{Float64}; K=nothing, W=nothing, model=nothing)
    N = prob.N
    ny = size(H, 1)
    (1 <= ny <= 8 && size(H, 2) == 15 && length(V) == ny) || error("H: (ny, 15) with 1 <= ny <= 8, V: ny variances")
    Hrow = Matrix{Float64}(transpose(H))
    packed = Float64[Sigma0[i, j] for i in 1:15 for j in 1:i]
    L = zeros(ny, 15, N)
    Pest = zeros(120, N)
    Sigma = K === nothing ? nothing : zeros(120, N)
    marg = K === nothing ? nothing : zeros(8, N)
    event_var = K === nothing ? nothing : zeros(2)
    qln_check(ccall((:qln_tracking_kalman_guarded_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble},
                     Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zout, K === nothing ? C_NULL : K, model === nothing ? C_NULL : model, events, Hrow, Int32(ny), V,
                    packed, Int32(1), W === nothing ? C_NULL : W, L, Pest, Sigma === nothing ? C_NULL : Sigma,
                    marg === nothing ? C_NULL : marg, event_var === nothing ? C_NULL : event_var))
    return L, Pest, Sigma, marg, event_var
end
# The forward sweep through the design of the filter (include/qln_evaluator.h, DESIGN.md 4.28): how L_k, P^+_k and log det S_k of
# tracking_kalman move along a direction of the noise (Sigma0_dot a 15 x 15 symmetric matrix of either sign, W_dot 15 values,
# V_dot ny values; nothing for zero, at least one), at the gains L (ny, 15, N) that call returned for the same (Zout, H, V) --
# which the sweep cannot check.  Returns (L_dot (ny, 15, N), Pest_dot (120, N) packed, logdet_dot (N)).
# tracking_kalman_guarded_jvp is the same through the guard-triggered touchdown at (Zout, events, model).
function tracking_kalman_jvp(prob::HybridNLPHIP, Zout::Vector{Float64}, L::Array{Float64,3}, H::Matrix{Float64},
                             V::Vector{Float64}; Sigma0_dot=nothing, W_dot=nothing, V_dot=nothing)
    N = prob.N
    ny = size(H, 1)
    (1 <= ny <= 8 && size(H, 2) == 15 && length(V) == ny && size(L) == (ny, 15, N)) ||
        error("H: (ny, 15) with 1 <= ny <= 8, V: ny variances, L: (ny, 15, N)")
    (V_dot === nothing || length(V_dot) == ny) || error("V_dot: ny values")
    Hrow = Matrix{Float64}(transpose(H))  # row-major [ny][15]
    packed = Sigma0_dot === nothing ? nothing : Float64[Sigma0_dot[i, j] for i in 1:15 for j in 1:i]
    L_dot = zeros(ny, 15, N)
    Pest_dot = zeros(120, N)
    logdet_dot = zeros(N)
    qln_check(ccall((:qln_kalman_design_jvp_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zout, L, Hrow, Int32(ny), V, packed === nothing ? C_NULL : packed, Int32(1),
                    W_dot === nothing ? C_NULL : W_dot, V_dot === nothing ? C_NULL : V_dot, L_dot, Pest_dot, logdet_dot))
    return L_dot, Pest_dot, logdet_dot
end
function tracking_kalman_guarded_jvp(prob::HybridNLPHIP, Zout::Vector{Float64}, events::Vector{Float64}, L::Array{Float64,3},
                                     H::Matrix{Float64}, V::Vector{Float64}; Sigma0_dot=nothing, W_dot=nothing, V_dot=nothing,
                                     model=nothing)
    N = prob.N
    ny = size(H, 1)
    (1 <= ny <= 8 && size(H, 2) == 15 && length(V) == ny && size(L) == (ny, 15, N)) ||
        error("H: (ny, 15) with 1 <= ny <= 8, V: ny variances, L: (ny, 15, N)")
    (V_dot === nothing || length(V_dot) == ny) || error("V_dot: ny values")
    Hrow = Matrix{Float64}(transpose(H))
    packed = Sigma0_dot === nothing ? nothing : Float64[Sigma0_dot[i, j] for i in 1:15 for j in 1:i]
    L_dot = zeros(ny, 15, N)
    Pest_dot = zeros(120, N)
    logdet_dot = zeros(N)
    qln_check(ccall((:qln_kalman_design_guarded_jvp_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble},
                     Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zout, model === nothing ? C_NULL : model, events, L, Hrow, Int32(ny), V,
                    packed === nothing ? C_NULL : packed, Int32(1), W_dot === nothing ? C_NULL : W_dot,
                    V_dot === nothing ? C_NULL : V_dot, L_dot, Pest_dot, logdet_dot))
    return L_dot, Pest_dot, logdet_dot
end
# The reverse sweep through the design of the filter (include/qln_evaluator.h, DESIGN.md 4.29): the transpose of
# tracking_kalman_jvp's map between the arrays as stored, at the same gains L (ny, 15, N).  The cotangents L_bar (ny, 15, N),
# Pest_bar (120, N) packed and logdet_bar (N), of any sign; nothing for zero, at least one.  Returns (Sigma0_bar (120) packed --
# an off-diagonal entry is the cotangent of both of its sides --, W_bar (15), V_bar (ny)); with them
# sum(L_bar .* L_dot) + sum(Pest_bar .* Pest_dot) + sum(logdet_bar .* logdet_dot) equals the three products with the packed
# Sigma0_dot, W_dot and V_dot.  tracking_kalman_guarded_vjp is the same through the guard-triggered touchdown.
function tracking_kalman_vjp(prob::HybridNLPHIP, Zout::Vector{Float64}, L::Array{Float64,3}, H::Matrix{Float64},
                             V::Vector{Float64}; L_bar=nothing, Pest_bar=nothing, logdet_bar=nothing)
    N = prob.N
    ny = size(H, 1)
    (1 <= ny <= 8 && size(H, 2) == 15 && length(V) == ny && size(L) == (ny, 15, N)) ||
        error("H: (ny, 15) with 1 <= ny <= 8, V: ny variances, L: (ny, 15, N)")
    ((L_bar === nothing || size(L_bar) == (ny, 15, N)) && (Pest_bar === nothing || size(Pest_bar) == (120, N)) &&
     (logdet_bar === nothing || length(logdet_bar) == N)) || error("L_bar: (ny, 15, N), Pest_bar: (120, N), logdet_bar: N values")
    Hrow = Matrix{Float64}(transpose(H))  # row-major [ny][15]
    Sigma0_bar = zeros(120)
    W_bar = zeros(15)
    V_bar = zeros(ny)
    qln_check(ccall((:qln_noise_design_vjp_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zout, L, Hrow, Int32(ny), V, L_bar === nothing ? C_NULL : L_bar,
                    Pest_bar === nothing ? C_NULL : Pest_bar, logdet_bar === nothing ? C_NULL : logdet_bar, Sigma0_bar, W_bar, V_bar))
    return Sigma0_bar, W_bar, V_bar
end
function tracking_kalman_guarded_vjp(prob::HybridNLPHIP, Zout::Vector{Float64}, events::Vector{Float64}, L::Array{Float64,3},
                                     H::Matrix{Float64}, V::Vector{Float64}; L_bar=nothing, Pest_bar=nothing, logdet_bar=nothing,
                                     model=nothing)
    N = prob.N
    ny = size(H, 1)
    (1 <= ny <= 8 && size(H, 2) == 15 && length(V) == ny && size(L) == (ny, 15, N)) ||
        error("H: (ny, 15) with 1 <= ny <= 8, V: ny variances, L: (ny, 15, N)")
    ((L_bar === nothing || size(L_bar) == (ny, 15, N)) && (Pest_bar === nothing || size(Pest_bar) == (120, N)) &&
     (logdet_bar === nothing || length(logdet_bar) == N)) || error("L_bar: (ny, 15, N), Pest_bar: (120, N), logdet_bar: N values")
    Hrow = Matrix{Float64}(transpose(H))
    Sigma0_bar = zeros(120)
    W_bar = zeros(15)
    V_bar = zeros(ny)
    qln_check(ccall((:qln_noise_design_guarded_vjp_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zout, model === nothing ? C_NULL : model, events, L, Hrow, Int32(ny), V,
                    L_bar === nothing ? C_NULL : L_bar, Pest_bar === nothing ? C_NULL : Pest_bar,
                    logdet_bar === nothing ? C_NULL : logdet_bar, Sigma0_bar, W_bar, V_bar))
    return Sigma0_bar, W_bar, V_bar
end
# Fixed-interval smoothing of a flown landing (include/qln_evaluator.h, DESIGN.md 4.25): the state at every knot given all N
# measurements, by the modified Bryson-Frazier sweep, which inverts nothing.  Ztraj: the trajectory the filter was designed
# along; L (ny, 15, N) and Pest (120, N) as tracking_kalman returns them for the same (Ztraj, H, V); Xhat (15, N) and innov
# (ny, N): the record of tracking_rollout_estimated.  Returns (Xs, Ps): the smoothed states as (15, N) and their error
# covariances as (120, N) packed lower triangles; at knot N, Xs = Xhat and Ps = Pest.  The call does not check that L and Pest
# belong together.  landing_smoother_guarded is the same through the guard-triggered touchdown at (Ztraj, events, model).
function landing_smoother(prob::HybridNLPHIP, Ztraj::Vector{Float64}, L::Array{Float64,3}, Pest::Matrix{Float64},
                          H::Matrix{Float64}, V::Vector{Float64}, Xhat::Matrix{Float64}, innov::Matrix{Float64})
    N = prob.N
    ny = size(H, 1)
    (1 <= ny <= 8 && size(H, 2) == 15 && length(V) == ny && size(L) == (ny, 15, N) && size(Pest) == (120, N) &&
     size(Xhat) == (15, N) && size(innov) == (ny, N)) || error("H: (ny, 15), V: ny, L: (ny, 15, N), Pest: (120, N), Xhat: (15, N), innov: (ny, N)")
    Hrow = Matrix{Float64}(transpose(H))  # row-major [ny][15]
    Xs = zeros(15, N)
    Ps = zeros(120, N)
    qln_check(ccall((:qln_landing_smoother_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Ztraj, L, Pest, Hrow, Int32(ny), V, Xhat, innov, Xs, Ps))
    return Xs, Ps
end
function landing_smoother_guarded(prob::HybridNLPHIP, Ztraj::Vector{Float64}, events::Vector{Float64}, L::Array{Float64,3},
                                  Pest::Matrix{Float64}, H::Matrix{Float64}, V::Vector{Float64}, Xhat::Matrix{Float64},
                                  innov::Matrix{Float64}; model=nothing)
    N = prob.N
    ny = size(H, 1)
    (1 <= ny <= 8 && size(H, 2) == 15 && length(V) == ny && size(L) == (ny, 15, N) && size(Pest) == (120, N) &&
     size(Xhat) == (15, N) && size(innov) == (ny, N)) || error("H: (ny, 15), V: ny, L: (ny, 15, N), Pest: (120, N), Xhat: (15, N), innov: (ny, N)")
    Hrow = Matrix{Float64}(transpose(H))
    Xs = zeros(15, N)
    Ps = zeros(120, N)
    qln_check(ccall((:qln_landing_smoother_guarded_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32,
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Ztraj, model === nothing ? C_NULL : model, events, L, Pest, Hrow, Int32(ny), V, Xhat, innov, Xs, Ps))
    return Xs, Ps
end
# The estimate-feedback roll-out (include/qln_evaluator.h, DESIGN.md 4.22): the plant and the estimator flown together, the
# forces fed back from the estimate xhat_k|k that the filter gains L of tracking_kalman build from y_k = H dx_k + v_k.  L: (ny, 15,
# N) as tracking_kalman returns it; H: (ny, 15); vnoise: (ny, N) and wnoise: (15, N-1) samples drawn by the caller, nothing for
# none; x0, xhat0: 15 values or nothing (the problem's x0, the reference's first knot).  Returns (Zout, Xhat, innov): the true
# states and applied controls, the estimates as (15, N) and the innovations as (ny, N).  tracking_rollout_estimated_guarded lets
# the plant and the estimator each land by their own guard and also returns (events, events_hat), their touchdown records.
function tracking_rollout_estimated(prob::HybridNLPHIP, Zref::Vector{Float64}, L::Array{Float64,3}, H::Matrix{Float64};
                                    K=nothing, vnoise=nothing, wnoise=nothing, x0=nothing, xhat0=nothing, model=nothing)
    N = prob.N
    ny = size(H, 1)
    (1 <= ny <= 8 && size(H, 2) == 15 && size(L) == (ny, 15, N)) || error("H: (ny, 15) with 1 <= ny <= 8, L: (ny, 15, N)")
    Hrow = Matrix{Float64}(transpose(H))  # row-major [ny][15]
    Zout = zeros(length(Zref))
    Xhat = zeros(15, N)
    innov = zeros(ny, N)
    qln_check(ccall((:qln_tracking_rollout_estimated_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, K === nothing ? C_NULL : K, L, Hrow, Int32(ny), vnoise === nothing ? C_NULL : vnoise,
                    wnoise === nothing ? C_NULL : wnoise, x0 === nothing ? C_NULL : x0, xhat0 === nothing ? C_NULL : xhat0,
                    model === nothing ? C_NULL : model, Zout, Xhat, innov))
    return Zout, Xhat, innov
end
function tracking_rollout_estimated_guarded(prob::HybridNLPHIP, Zref::Vector{Float64}, L::Array{Float64,3}, H::Matrix{Float64};
                                            K=nothing, vnoise=nothing, wnoise=nothing, x0=nothing, xhat0=nothing, model=nothing)
    N = prob.N
    ny = size(H, 1)
    (1 <= ny <= 8 && size(H, 2) == 15 && size(L) == (ny, 15, N)) || error("H: (ny, 15) with 1 <= ny <= 8, L: (ny, 15, N)")
    Hrow = Matrix{Float64}(transpose(H))
    Zout = zeros(length(Zref))
    Xhat = zeros(15, N)
    innov = zeros(ny, N)
    events = zeros(8)
    events_hat = zeros(8)
    qln_check(ccall((:qln_tracking_rollout_estimated_guarded_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}),
                    prob.handle, Zref, K === nothing ? C_NULL : K, L, Hrow, Int32(ny), vnoise === nothing ? C_NULL : vnoise,
                    wnoise === nothing ? C_NULL : wnoise, x0 === nothing ? C_NULL : x0, xhat0 === nothing ? C_NULL : xhat0,
                    model === nothing ? C_NULL : model, Zout, Xhat, innov, events, events_hat))
    return Zout, Xhat, innov, events, events_hat
end
# The filter on recorded data (include/qln_evaluator.h, DESIGN.md 4.26): the estimator of tracking_rollout_estimated run on a
# record.  Zref: the reference (only its state slots are read); Zrec: the recorded trajectory, of which only the control slots
# are read, the four applied forces and h_k of every knot; L: (ny, 15, N) as tracking_kalman returns it; H: (ny, 15); Y: (ny, N),
# the readings less H x_ref,k (what the roll-out forms as y_k); V: the ny measurement variances the gains were designed for, or
# nothing for no score; xhat0: 15 values or nothing (the reference's first knot).  Returns (Xhat, innov, score, loglik): the
# estimates as (15, N), the innovations as (ny, N), score (2, N) = (nis_k, log det S_k) and the Gaussian log-likelihood, the last
# two nothing without V.  The call cannot check that L belongs to V.  landing_filter_guarded lets the estimator land by its own
# guard and also returns events_hat, its touchdown record.  model: the record's own (g, mb, mf, lb), or nothing for the handle's
# (DESIGN.md 4.27; with nothing the call has the bits of the entry without a model).
function landing_filter(prob::HybridNLPHIP, Zref::Vector{Float64}, Zrec::Vector{Float64}, L::Array{Float64,3}, H::Matrix{Float64},
                        Y::Matrix{Float64}; V=nothing, xhat0=nothing, model=nothing)
    N = prob.N
    ny = size(H, 1)
    (1 <= ny <= 8 && size(H, 2) == 15 && size(L) == (ny, 15, N) && size(Y) == (ny, N) && (V === nothing || length(V) == ny)) ||
        error("H: (ny, 15) with 1 <= ny <= 8, L: (ny, 15, N), Y: (ny, N), V: ny")
    Hrow = Matrix{Float64}(transpose(H))  # row-major [ny][15]
    Xhat = zeros(15, N)
    innov = zeros(ny, N)
    score = V === nothing ? nothing : zeros(2, N)
    loglik = V === nothing ? nothing : zeros(1)
    qln_check(ccall((:qln_landing_filter_model_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, Zrec, L, Hrow, Int32(ny), model === nothing ? C_NULL : model, V === nothing ? C_NULL : V, Y,
                    xhat0 === nothing ? C_NULL : xhat0, Xhat, innov, score === nothing ? C_NULL : score,
                    loglik === nothing ? C_NULL : loglik))
    return Xhat, innov, score, loglik === nothing ? nothing : loglik[1]
end
function landing_filter_guarded(prob::HybridNLPHIP, Zref::Vector{Float64}, Zrec::Vector{Float64}, L::Array{Float64,3},
                                H::Matrix{Float64}, Y::Matrix{Float64}; V=nothing, xhat0=nothing, model=nothing)
    N = prob.N
    ny = size(H, 1)
    (1 <= ny <= 8 && size(H, 2) == 15 && size(L) == (ny, 15, N) && size(Y) == (ny, N) && (V === nothing || length(V) == ny)) ||
        error("H: (ny, 15) with 1 <= ny <= 8, L: (ny, 15, N), Y: (ny, N), V: ny")
    Hrow = Matrix{Float64}(transpose(H))
    Xhat = zeros(15, N)
    innov = zeros(ny, N)
    score = V === nothing ? nothing : zeros(2, N)
    loglik = V === nothing ? nothing : zeros(1)
    events_hat = zeros(8)
    qln_check(ccall((:qln_landing_filter_guarded_model_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, Zrec, L, Hrow, Int32(ny), model === nothing ? C_NULL : model, V === nothing ? C_NULL : V, Y,
                    xhat0 === nothing ? C_NULL : xhat0, Xhat, innov, score === nothing ? C_NULL : score,
                    loglik === nothing ? C_NULL : loglik, events_hat))
    return Xhat, innov, score, loglik === nothing ? nothing : loglik[1], events_hat
end
# The sweeps through the filter (include/qln_evaluator.h, DESIGN.md 4.27), host forms: the derivative of landing_filter /
# landing_filter_guarded at the record and the (Xhat, innov[, events_hat]) it returned, with respect to Y, the control slots of
# Zrec, L, xhat0 and model, AT FIXED GAINS in the score: V given asks for nis_dot (N) and loglik_dot (the exact derivative of
# loglik at fixed gains) and excludes L_dot / L_bar, which need V = nothing.  Forward: tangents as keywords, nothing for zero;
# returns (Xhat_dot (15, N), innov_dot (ny, N), nis_dot, loglik_dot), the last two nothing without V, and guarded also
# event_hat_dot.  Reverse: cotangents as keywords (Xhat_bar (15, N), innov_bar (ny, N), and with V nis_bar (N) and loglik_bar);
# returns (Y_bar (ny, N), Zrec_bar, L_bar or nothing with V, xhat0_bar (15), model_bar (4)).
function _filter_sweep_rows(prob::HybridNLPHIP, L::Array{Float64,3}, H::Matrix{Float64}, V)
    ny = size(H, 1)
    (1 <= ny <= 8 && size(H, 2) == 15 && size(L) == (ny, 15, prob.N) && (V === nothing || length(V) == ny)) ||
        error("H: (ny, 15) with 1 <= ny <= 8, L: (ny, 15, N), V: ny")
    return ny, Matrix{Float64}(transpose(H))  # row-major [ny][15]
end
function landing_filter_jvp(prob::HybridNLPHIP, Zref::Vector{Float64}, Zrec::Vector{Float64}, L::Array{Float64,3},
                            H::Matrix{Float64}, Xhat::Matrix{Float64}, innov::Matrix{Float64}; V=nothing, model=nothing,
                            Y_dot=nothing, Zrec_dot=nothing, L_dot=nothing, xhat0_dot=nothing, model_dot=nothing)
    ny, Hrow = _filter_sweep_rows(prob, L, H, V)
    Xhat_dot = zeros(15, prob.N)
    innov_dot = zeros(ny, prob.N)
    nis_dot = V === nothing ? nothing : zeros(prob.N)
    loglik_dot = V === nothing ? nothing : zeros(1)
    qln_check(ccall((:qln_landing_filter_jvp_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, Zrec, L, Hrow, Int32(ny), model === nothing ? C_NULL : model, V === nothing ? C_NULL : V, Xhat,
                    innov, Y_dot === nothing ? C_NULL : Y_dot, Zrec_dot === nothing ? C_NULL : Zrec_dot,
                    L_dot === nothing ? C_NULL : L_dot, xhat0_dot === nothing ? C_NULL : xhat0_dot,
                    model_dot === nothing ? C_NULL : model_dot, Xhat_dot, innov_dot, nis_dot === nothing ? C_NULL : nis_dot,
                    loglik_dot === nothing ? C_NULL : loglik_dot))
    return Xhat_dot, innov_dot, nis_dot, loglik_dot === nothing ? nothing : loglik_dot[1]
end
function landing_filter_guarded_jvp(prob::HybridNLPHIP, Zref::Vector{Float64}, Zrec::Vector{Float64}, L::Array{Float64,3},
                                    H::Matrix{Float64}, Xhat::Matrix{Float64}, innov::Matrix{Float64}, events_hat::Vector{Float64};
                                    V=nothing, model=nothing, Y_dot=nothing, Zrec_dot=nothing, L_dot=nothing, xhat0_dot=nothing,
                                    model_dot=nothing)
    ny, Hrow = _filter_sweep_rows(prob, L, H, V)
    Xhat_dot = zeros(15, prob.N)
    innov_dot = zeros(ny, prob.N)
    nis_dot = V === nothing ? nothing : zeros(prob.N)
    loglik_dot = V === nothing ? nothing : zeros(1)
    event_hat_dot = zeros(8)
    qln_check(ccall((:qln_landing_filter_guarded_jvp_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, Zrec, L, Hrow, Int32(ny), model === nothing ? C_NULL : model, V === nothing ? C_NULL : V, Xhat,
                    innov, events_hat, Y_dot === nothing ? C_NULL : Y_dot, Zrec_dot === nothing ? C_NULL : Zrec_dot,
                    L_dot === nothing ? C_NULL : L_dot, xhat0_dot === nothing ? C_NULL : xhat0_dot,
                    model_dot === nothing ? C_NULL : model_dot, Xhat_dot, innov_dot, nis_dot === nothing ? C_NULL : nis_dot,
                    loglik_dot === nothing ? C_NULL : loglik_dot, event_hat_dot))
    return Xhat_dot, innov_dot, nis_dot, loglik_dot === nothing ? nothing : loglik_dot[1], event_hat_dot
end
function landing_filter_vjp(prob::HybridNLPHIP, Zref::Vector{Float64}, Zrec::Vector{Float64}, L::Array{Float64,3},
                            H::Matrix{Float64}, Xhat::Matrix{Float64}, innov::Matrix{Float64}; V=nothing, model=nothing,
                            Xhat_bar=nothing, innov_bar=nothing, nis_bar=nothing, loglik_bar=nothing)
    ny, Hrow = _filter_sweep_rows(prob, L, H, V)
    Y_bar = zeros(ny, prob.N)
    Zrec_bar = zeros(length(Zrec))
    L_bar = V === nothing ? zeros(ny, 15, prob.N) : nothing
    xhat0_bar = zeros(15)
    model_bar = zeros(4)
    qln_check(ccall((:qln_landing_filter_vjp_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, Zrec, L, Hrow, Int32(ny), model === nothing ? C_NULL : model, V === nothing ? C_NULL : V, Xhat,
                    innov, Xhat_bar === nothing ? C_NULL : Xhat_bar, innov_bar === nothing ? C_NULL : innov_bar,
                    nis_bar === nothing ? C_NULL : nis_bar, loglik_bar === nothing ? C_NULL : Float64[loglik_bar], Y_bar, Zrec_bar,
                    L_bar === nothing ? C_NULL : L_bar, xhat0_bar, model_bar))
    return Y_bar, Zrec_bar, L_bar, xhat0_bar, model_bar
end
function landing_filter_guarded_vjp(prob::HybridNLPHIP, Zref::Vector{Float64}, Zrec::Vector{Float64}, L::Array{Float64,3},
                                    H::Matrix{Float64}, Xhat::Matrix{Float64}, innov::Matrix{Float64}, events_hat::Vector{Float64};
                                    V=nothing, model=nothing, Xhat_bar=nothing, innov_bar=nothing, nis_bar=nothing,
                                    loglik_bar=nothing)
    ny, Hrow = _filter_sweep_rows(prob, L, H, V)
    Y_bar = zeros(ny, prob.N)
    Zrec_bar = zeros(length(Zrec))
    L_bar = V === nothing ? zeros(ny, 15, prob.N) : nothing
    xhat0_bar = zeros(15)
    model_bar = zeros(4)
    qln_check(ccall((:qln_landing_filter_guarded_vjp_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, Zrec, L, Hrow, Int32(ny), model === nothing ? C_NULL : model, V === nothing ? C_NULL : V, Xhat,
                    innov, events_hat, Xhat_bar === nothing ? C_NULL : Xhat_bar, innov_bar === nothing ? C_NULL : innov_bar,
                    nis_bar === nothing ? C_NULL : nis_bar, loglik_bar === nothing ? C_NULL : Float64[loglik_bar], Y_bar, Zrec_bar,
                    L_bar === nothing ? C_NULL : L_bar, xhat0_bar, model_bar))
    return Y_bar, Zrec_bar, L_bar, xhat0_bar, model_bar
end
# The sweeps through the estimate-feedback roll-out (include/qln_evaluator.h, DESIGN.md 4.23): the derivative of
# tracking_rollout_estimated / _guarded at the (Zout, Xhat, innov[, events, events_hat]) it returned, with respect to Zref, K, L,
# x0, xhat0 and model, at FIXED noise samples and fixed H.  Forward: tangents as keywords, nothing for zero -- except xhat0_dot,
# whose nothing is the roll-out's xhat0 = nothing (the estimate starts on the reference, its tangent is Zref_dot's first knot);
# returns (Zout_dot, Xhat_dot (15, N), innov_dot (ny, N)) and guarded also (event_dot, event_hat_dot).  Reverse: cotangents Zbar
# and, as keywords, Xhat_bar (15, N) and innov_bar (ny, N); returns (Zref_bar, K_bar, L_bar, x0_bar, xhat0_bar, model_bar), with
# with_xhat0 = false xhat0_bar is nothing and its value is added to Zref_bar's first knot.
_opt(x) = x === nothing ? C_NULL : x
function _estimated_rows(prob::HybridNLPHIP, L::Array{Float64,3}, H::Matrix{Float64})
    ny = size(H, 1)
    (1 <= ny <= 8 && size(H, 2) == 15 && size(L) == (ny, 15, prob.N)) || error("H: (ny, 15) with 1 <= ny <= 8, L: (ny, 15, N)")
    return ny, Matrix{Float64}(transpose(H))  # row-major [ny][15]
end
function tracking_rollout_estimated_jvp(prob::HybridNLPHIP, Zref::Vector{Float64}, L::Array{Float64,3}, H::Matrix{Float64},
                                        Zout::Vector{Float64}, Xhat::Matrix{Float64}, innov::Matrix{Float64}; K=nothing,
                                        model=nothing, Zref_dot=nothing, K_dot=nothing, L_dot=nothing, x0_dot=nothing,
                                        xhat0_dot=nothing, model_dot=nothing)
    ny, Hrow = _estimated_rows(prob, L, H)
    Zout_dot = zeros(length(Zref))
    Xhat_dot = zeros(15, prob.N)
    innov_dot = zeros(ny, prob.N)
    qln_check(ccall((:qln_tracking_rollout_estimated_jvp_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, _opt(K), L, Hrow, Int32(ny), _opt(model), Zout, Xhat, innov, _opt(Zref_dot), _opt(K_dot),
                    _opt(L_dot), _opt(x0_dot), _opt(xhat0_dot), _opt(model_dot), Zout_dot, Xhat_dot, innov_dot))
    return Zout_dot, Xhat_dot, innov_dot
end
function tracking_rollout_estimated_guarded_jvp(prob::HybridNLPHIP, Zref::Vector{Float64}, L::Array{Float64,3}, H::Matrix{Float64},
                                                Zout::Vector{Float64}, Xhat::Matrix{Float64}, innov::Matrix{Float64},
                                                events::Vector{Float64}, events_hat::Vector{Float64}; K=nothing, model=nothing,
                                                Zref_dot=nothing, K_dot=nothing, L_dot=nothing, x0_dot=nothing,
                                                xhat0_dot=nothing, model_dot=nothing)
    ny, Hrow = _estimated_rows(prob, L, H)
    Zout_dot = zeros(length(Zref))
    Xhat_dot = zeros(15, prob.N)
    innov_dot = zeros(ny, prob.N)
    event_dot = zeros(8)
    event_hat_dot = zeros(8)
    qln_check(ccall((:qln_tracking_rollout_estimated_guarded_jvp_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}),
                    prob.handle, Zref, _opt(K), L, Hrow, Int32(ny), _opt(model), Zout, Xhat, innov, events, events_hat,
                    _opt(Zref_dot), _opt(K_dot), _opt(L_dot), _opt(x0_dot), _opt(xhat0_dot), _opt(model_dot), Zout_dot, Xhat_dot,
                    innov_dot, event_dot, event_hat_dot))
    return Zout_dot, Xhat_dot, innov_dot, event_dot, event_hat_dot
end
function tracking_rollout_estimated_vjp(prob::HybridNLPHIP, Zref::Vector{Float64}, L::Array{Float64,3}, H::Matrix{Float64},
                                        Zout::Vector{Float64}, Xhat::Matrix{Float64}, innov::Matrix{Float64},
                                        Zbar::Vector{Float64}; K=nothing, model=nothing, Xhat_bar=nothing, innov_bar=nothing,
                                        with_xhat0::Bool=true)
    ny, Hrow = _estimated_rows(prob, L, H)
    Zref_bar = zeros(length(Zref))
    K_bar = K === nothing ? nothing : zeros(size(K))
    L_bar = zeros(ny, 15, prob.N)
    x0_bar = zeros(15)
    xhat0_bar = with_xhat0 ? zeros(15) : nothing
    model_bar = zeros(4)
    qln_check(ccall((:qln_tracking_rollout_estimated_vjp_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, _opt(K), L, Hrow, Int32(ny), _opt(model), Zout, Xhat, innov, Zbar, _opt(Xhat_bar),
                    _opt(innov_bar), Zref_bar, _opt(K_bar), L_bar, x0_bar, _opt(xhat0_bar), model_bar))
    return Zref_bar, K_bar, L_bar, x0_bar, xhat0_bar, model_bar
end
function tracking_rollout_estimated_guarded_vjp(prob::HybridNLPHIP, Zref::Vector{Float64}, L::Array{Float64,3}, H::Matrix{Float64},
                                                Zout::Vector{Float64}, Xhat::Matrix{Float64}, innov::Matrix{Float64},
                                                events::Vector{Float64}, events_hat::Vector{Float64}, Zbar::Vector{Float64};
                                                K=nothing, model=nothing, Xhat_bar=nothing, innov_bar=nothing,
                                                with_xhat0::Bool=true)
    ny, Hrow = _estimated_rows(prob, L, H)
    Zref_bar = zeros(length(Zref))
    K_bar = K === nothing ? nothing : zeros(size(K))
    L_bar = zeros(ny, 15, prob.N)
    x0_bar = zeros(15)
    xhat0_bar = with_xhat0 ? zeros(15) : nothing
    model_bar = zeros(4)
    qln_check(ccall((:qln_tracking_rollout_estimated_guarded_vjp_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, _opt(K), L, Hrow, Int32(ny), _opt(model), Zout, Xhat, innov, events, events_hat, Zbar,
                    _opt(Xhat_bar), _opt(innov_bar), Zref_bar, _opt(K_bar), L_bar, x0_bar, _opt(xhat0_bar), model_bar))
    return Zref_bar, K_bar, L_bar, x0_bar, xhat0_bar, model_bar
end
# Contact-aware force limits (include/qln_evaluator.h, DESIGN.md 4.20).  limits holds 8 values, {lo, hi} of F_x and of F_y for a
# free foot, then for a standing one (+-Inf: no limit).  tracking_rollout_limited is tracking_rollout_model (guarded = false) or
# tracking_rollout_guarded (guarded = true) with the applied forces clamped, and returns (Zout, events, sat): events is nothing
# when not guarded, sat holds one saturation code per knot, sum_m s_m 4^m with s_m = 1 at the lower and 2 at the upper limit
# (unpack_saturation).  The sweeps and the gains at that active set take sat, and events for the guarded blocks (nothing: the
# knot schedule's); a channel that rode a limit has no tangent, a zero row in K_bar and a zero row in the designed K.
function tracking_rollout_limited(prob::HybridNLPHIP, Zref::Vector{Float64}, limits::Vector{Float64}; K=nothing, x0=nothing,
                                  model=nothing, guarded::Bool=false)
    length(limits) == 8 || error("limits: 8 values expected")
    Zout = zeros(length(Zref))
    events = guarded ? zeros(8) : nothing
    sat = zeros(prob.N - 1)
    qln_check(ccall((:qln_tracking_rollout_limited_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, K === nothing ? C_NULL : K, x0 === nothing ? C_NULL : x0,
                    model === nothing ? C_NULL : model, limits, Int32(guarded ? 1 : 0), Zout,
                    events === nothing ? C_NULL : events, sat))
    return Zout, events, sat
end
function tracking_rollout_limited_jvp(prob::HybridNLPHIP, Zref::Vector{Float64}, Zout::Vector{Float64}, sat::Vector{Float64};
                                      events=nothing, K=nothing, model=nothing, Zref_dot=nothing, K_dot=nothing, x0_dot=nothing,
                                      model_dot=nothing)
    Zout_dot = zeros(length(Zref))
    event_dot = events === nothing ? nothing : zeros(8)
    qln_check(ccall((:qln_tracking_rollout_limited_jvp_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, K === nothing ? C_NULL : K, Zout, model === nothing ? C_NULL : model,
                    events === nothing ? C_NULL : events, sat, Zref_dot === nothing ? C_NULL : Zref_dot,
                    K_dot === nothing ? C_NULL : K_dot, x0_dot === nothing ? C_NULL : x0_dot,
                    model_dot === nothing ? C_NULL : model_dot, Zout_dot, event_dot === nothing ? C_NULL : event_dot))
    return Zout_dot, event_dot
end
function tracking_rollout_limited_vjp(prob::HybridNLPHIP, Zref::Vector{Float64}, Zout::Vector{Float64}, sat::Vector{Float64},
                                      Zbar::Vector{Float64}; events=nothing, K=nothing, model=nothing)
    Zref_bar = zeros(length(Zref))
    K_bar = K === nothing ? nothing : zeros(size(K))
    x0_bar = zeros(15)
    model_bar = zeros(4)
    qln_check(ccall((:qln_tracking_rollout_limited_vjp_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, K === nothing ? C_NULL : K, Zout, model === nothing ? C_NULL : model,
                    events === nothing ? C_NULL : events, sat, Zbar, Zref_bar, K_bar === nothing ? C_NULL : K_bar, x0_bar,
                    model_bar))
    return Zref_bar, K_bar, x0_bar, model_bar
end
# events = nothing: tracking_lqr's blocks (model must then be nothing); else tracking_lqr_guarded's
function tracking_lqr_limited(prob::HybridNLPHIP, Ztraj::Vector{Float64}, sat::Vector{Float64}, Q::Vector{Float64},
                              R::Vector{Float64}, Qf::Vector{Float64}; events=nothing, model=nothing,
                              with_cost_to_go::Bool=true)
    N = prob.N
    K = zeros(15, 4, N - 1)
    P = with_cost_to_go ? zeros(120, N) : nothing
    qln_check(ccall((:qln_tracking_lqr_limited_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Ztraj, model === nothing ? C_NULL : model, events === nothing ? C_NULL : events, sat, Q, R, Qf,
                    K, P === nothing ? C_NULL : P))
    return K, P
end
# saturation codes (N-1) -> (4, N-1) digits per channel (F1x, F1y, F2x, F2y): 0 free, 1 at the lower limit, 2 at the upper
unpack_saturation(sat::Vector{Float64}) = [(Int(sat[k]) >> (2 * (m - 1))) & 3 for m in 1:4, k in 1:length(sat)]
# gains K (15, 4, N-1) designed elsewhere, with the rows of the channels that rode a limit set to zero
function mask_gains(K::Array{Float64,3}, sat::Vector{Float64})
    s = unpack_saturation(sat)
    return [s[m, k] == 0 ? K[j, m, k] : 0.0 for j in 1:size(K, 1), m in 1:4, k in 1:length(sat)]
end
# Force limits in the estimate-feedback roll-out (include/qln_evaluator.h, DESIGN.md 4.24): tracking_rollout_estimated (guarded =
# false) or tracking_rollout_estimated_guarded (guarded = true) with the forces fed back from the estimate clamped to limits by the
# PLANT's contact mode, before the plant, the estimator or Zout read them.  Returns (Zout, Xhat, innov, events, events_hat, sat):
# the records nothing when not guarded, sat as tracking_rollout_limited returns it.  The sweeps at that active set take sat after
# the trajectory, and both records for the guarded blocks (both nothing: the knot schedule's); the rest is the estimated sweeps'.
function tracking_rollout_estimated_limited(prob::HybridNLPHIP, Zref::Vector{Float64}, limits::Vector{Float64},
                                            L::Array{Float64,3}, H::Matrix{Float64}; K=nothing, vnoise=nothing, wnoise=nothing,
                                            x0=nothing, xhat0=nothing, model=nothing, guarded::Bool=false)
    length(limits) == 8 || error("limits: 8 values expected")
    ny, Hrow = _estimated_rows(prob, L, H)
    Zout = zeros(length(Zref))
    Xhat = zeros(15, prob.N)
    innov = zeros(ny, prob.N)
    events = guarded ? zeros(8) : nothing
    events_hat = guarded ? zeros(8) : nothing
    sat = zeros(prob.N - 1)
    qln_check(ccall((:qln_tracking_rollout_estimated_limited_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, _opt(K), L, Hrow, Int32(ny), _opt(vnoise), _opt(wnoise), _opt(x0), _opt(xhat0), _opt(model),
                    limits, Int32(guarded ? 1 : 0), Zout, Xhat, innov, _opt(events), _opt(events_hat), sat))
    return Zout, Xhat, innov, events, events_hat, sat
end
function tracking_rollout_estimated_limited_jvp(prob::HybridNLPHIP, Zref::Vector{Float64}, L::Array{Float64,3}, H::Matrix{Float64},
                                                Zout::Vector{Float64}, Xhat::Matrix{Float64}, innov::Matrix{Float64},
                                                sat::Vector{Float64}; events=nothing, events_hat=nothing, K=nothing, model=nothing,
                                                Zref_dot=nothing, K_dot=nothing, L_dot=nothing, x0_dot=nothing,
                                                xhat0_dot=nothing, model_dot=nothing)
    ny, Hrow = _estimated_rows(prob, L, H)
    (events === nothing) == (events_hat === nothing) || error("events and events_hat: both or neither")
    Zout_dot = zeros(length(Zref))
    Xhat_dot = zeros(15, prob.N)
    innov_dot = zeros(ny, prob.N)
    event_dot = events === nothing ? nothing : zeros(8)
    event_hat_dot = events === nothing ? nothing : zeros(8)
    qln_check(ccall((:qln_tracking_rollout_estimated_limited_jvp_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, _opt(K), L, Hrow, Int32(ny), _opt(model), Zout, Xhat, innov, _opt(events), _opt(events_hat),
                    sat, _opt(Zref_dot), _opt(K_dot), _opt(L_dot), _opt(x0_dot), _opt(xhat0_dot), _opt(model_dot), Zout_dot,
                    Xhat_dot, innov_dot, _opt(event_dot), _opt(event_hat_dot)))
    return Zout_dot, Xhat_dot, innov_dot, event_dot, event_hat_dot
end
function tracking_rollout_estimated_limited_vjp(prob::HybridNLPHIP, Zref::Vector{Float64}, L::Array{Float64,3}, H::Matrix{Float64},
                                                Zout::Vector{Float64}, Xhat::Matrix{Float64}, innov::Matrix{Float64},
                                                sat::Vector{Float64}, Zbar::Vector{Float64}; events=nothing, events_hat=nothing,
                                                K=nothing, model=nothing, Xhat_bar=nothing, innov_bar=nothing,
                                                with_xhat0::Bool=true)
    ny, Hrow = _estimated_rows(prob, L, H)
    (events === nothing) == (events_hat === nothing) || error("events and events_hat: both or neither")
    Zref_bar = zeros(length(Zref))
    K_bar = K === nothing ? nothing : zeros(size(K))
    L_bar = zeros(ny, 15, prob.N)
    x0_bar = zeros(15)
    xhat0_bar = with_xhat0 ? zeros(15) : nothing
    model_bar = zeros(4)
    qln_check(ccall((:qln_tracking_rollout_estimated_limited_vjp_host, LIBQLN), Cint,
                    (Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int32, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.handle, Zref, _opt(K), L, Hrow, Int32(ny), _opt(model), Zout, Xhat, innov, _opt(events), _opt(events_hat),
                    sat, Zbar, _opt(Xhat_bar), _opt(innov_bar), Zref_bar, _opt(K_bar), L_bar, x0_bar, _opt(xhat0_bar), model_bar))
    return Zref_bar, K_bar, L_bar, x0_bar, xhat0_bar, model_bar
end

# ---- the reference's Ipopt solve, for this evaluator type: a method of `solve` (src/moi.jl:46-103) ------------------------
# Same generic function, same keyword arguments and defaults, same five things handed to Ipopt.  What differs from the
# HybridNLP method, on purpose:
#   * the variable bounds come from the library (qln_variable_bounds: theta, h and the two lower bounds of quirk Q6 at the
#     reference's own indices 22+20(k-1), 24+20(k-1)) instead of being restated here;
#   * the evaluator Ipopt calls back is `prob` itself.  The reference's MOI.eval_constraint_jacobian passes the GLOBAL
#     `nlp` to jac_c! (src/moi.jl:22) and jac_c! reads the GLOBAL `lb` (src/constraints.jl:270,272) -- quirk Q4: both are
#     sidestepped, the veneer's callbacks use their argument's handle, whose model carries lb.
# Requires `using Ipopt` in the session, as the reference's notebook has (MathOptInterface 0.9: MOI.SingleVariable).
function solve(x0, prob::HybridNLPHIP; tol=1.0e-6, c_tol=1.0e-6, max_iter=2000)
    n_nlp = num_primals(prob)
    length(x0) == n_nlp || error("solve: x0 has $(length(x0)) entries, the problem has $n_nlp variables")
    x_l = Vector{Float64}(undef, n_nlp); x_u = Vector{Float64}(undef, n_nlp)
    qln_check(ccall((:qln_variable_bounds, LIBQLN), Cint, (Int32, Ptr{QlnSolveOptions}, Ptr{Cdouble}, Ptr{Cdouble}),
                    prob.N, C_NULL, x_l, x_u))
    block = MOI.NLPBlockData(MOI.NLPBoundsPair.(prob.lb, prob.ub), prob, true)       # true: has an objective
    solver = Ipopt.Optimizer()
    for (name, value) in ("max_iter" => max_iter, "tol" => tol, "constr_viol_tol" => c_tol)
        solver.options[name] = value
    end
    x = MOI.add_variables(solver, n_nlp)
    for (xi, lo, hi, start) in zip(x, x_l, x_u, x0)
        v = MOI.SingleVariable(xi)
        MOI.add_constraint(solver, v, MOI.LessThan(hi))        # +-Inf bounds included, as the reference adds them
        MOI.add_constraint(solver, v, MOI.GreaterThan(lo))
        MOI.set(solver, MOI.VariablePrimalStart(), xi, start)
    end
    MOI.set(solver, MOI.NLPBlock(), block)
    MOI.set(solver, MOI.ObjectiveSense(), MOI.MIN_SENSE)
    MOI.optimize!(solver)
    return MOI.get(solver, MOI.VariablePrimal(), x), solver
end
