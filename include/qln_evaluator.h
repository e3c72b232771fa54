/*
 * qln_evaluator.h -- C ABI of the MI355X-native batched NLP evaluator for the
 * hybrid planar-quadruped landing problem.
 *
 * This is the drop-in boundary for the reference's evaluator path
 *   src/moi.jl:1-33          (MOI.eval_objective / eval_objective_gradient /
 *                             eval_constraint / eval_constraint_jacobian /
 *                             jacobian_structure on HybridNLP)
 *   src/costs.jl:6-34        (eval_f, grad_f!)
 *   src/constraints.jl:145-158, 212-291   (eval_c!, jac_c!)
 *   src/nlp.jl:13-87         (HybridNLP index maps, bounds, sizes)
 * generalised from ONE problem to a batch of B independent landing problems.
 * Plain pointers and sizes only; every entry point returns an int status
 * (QLN_OK == 0, negative = error) and never throws or exits.  The Julia `ccall`
 * veneer a maintainer would add is integration/julia/HybridNLPHIP.jl; the Python
 * ctypes mirror used by the tests is quadruped_landing_amd/_lib.py.
 *
 * Threading: a handle is not thread-safe; distinct handles are independent.  Batched (device-pointer)
 * calls are asynchronous and ordered on the handle's stream; MOI-mode (host-pointer) calls return
 * after the results are in the caller's buffers.  The library never frees, reallocates or keeps caller
 * buffers; it owns only its handle (descriptor copies and, for MOI mode, lazily allocated staging) and what the
 * caller explicitly asks it to allocate with qln_vals_alloc_placed.
 *
 * Host forms (the qln_*_host entry points, MOI mode included) take HOST pointers in the layouts of their device form
 * and are synchronous.  The mode is chosen once, in qln_create: a batch with (z_total + c_total + j_total) * 8 bytes
 * <= 8 MiB is evaluated on pinned host buffers mapped into the device's address space (the kernels read and write them
 * directly: one launch, one synchronisation), a larger one is staged through device memory.
 * qln_eval_hessian_lagrangian_host and qln_solve_host are always staged.  The handle allocates each buffer on first
 * use, zero-filled, and keeps it until qln_destroy.  Four arguments are in-out and copied in whole, so that their
 * entries from n_nlp to z_stride come back as the caller's buffer held them: Zout of qln_tracking_rollout_host (and of
 * qln_tracking_rollout_guarded_host), Zref_bar of qln_tracking_rollout_vjp_host, Zout_dot of qln_tracking_rollout_jvp_host (each also in its _model_ form,
 * qln_tracking_rollout_model_host and its two sweeps) and Z of qln_solve_host.  The
 * padding of every other result (past n_nlp in the layout of Z, between the problems of c, vals and hvals) comes back as
 * zeros.
 *
 * Layouts (all FP64, all offsets/strides in doubles):
 *   Z     problem b at Z + b*z_stride, length n_nlp = 20N-5,
 *         [x_1 u_1 x_2 u_2 ... x_{N-1} u_{N-1} x_N]           (src/nlp.jl:38-39,94-102)
 *   c     problem b at c + c_off[b], length m_nlp(b) = 18N - k_trans(b) + 16, in the
 *         reference's cinds order (src/nlp.jl:48-63): init 15 | term 14 | dyn 15(N-1) |
 *         contact-init N | contact-other N-k_trans+1 | final-control 1 | clearance N
 *   vals  problem b at vals + j_off[b], length nnz(b); block-COO of the reference's
 *         jac_c! write-set, state-dependent entries first:
 *           [ (N-1) step blocks, 15x20 column-major each            src/constraints.jl:186-198 ]
 *           [ N clearance d/dtheta entries                          src/constraints.jl:269-273 ]
 *           [ I(15) 15x15 col-major | I(15)[1:14,:] 14x15           src/constraints.jl:228-229 ]
 *           [ 15(N-1) diagonal -1 of the -I(n) blocks               src/constraints.jl:200     ]
 *           [ contact-init N ones | contact-other N-k_trans+1 ones  src/constraints.jl:235-256 ]
 *           [ final-control 2 ones | clearance d/dyb N ones         src/constraints.jl:259-265 ]
 *         The first 300(N-1)+N values depend on Z; the rest are constants and are
 *         written only when QLN_JAC_WRITE_CONSTANTS is set (or once by
 *         qln_jacobian_init_constants).
 *         With jac_format = QLN_JAC_FORMAT_STRUCTURAL only the first section differs: a step block holds
 *         just the entries that can be non-zero in the knot's contact mode, in column-major order of
 *         that pattern -- 71 values in contact modes 1/2, 56 at the transition knot k_trans-1 (the jump
 *         mask zeroes rows 5, 7, 11-15, src/planar_quadruped.jl:262-263), 57 in mode 3 -- so the section
 *         has 71*n1 + 56*nj + 57*n3 values (n1 = knots before the transition knot, nj = 0/1, n3 = knots
 *         from k_trans on).  Entries left out are exactly 0.0 in the reference's ForwardDiff Jacobian for
 *         every Z; qln_jacobian_structure lists the entries that remain.
 *   grad  same layout as Z.        f: one double per problem.
 */
#ifndef QLN_EVALUATOR_H
#define QLN_EVALUATOR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QLN_NX 15          /* state dim   (src/planar_quadruped.jl:25) */
#define QLN_NU 5           /* control dim (src/planar_quadruped.jl:26) */
#define QLN_NZ 20
#define QLN_COST_STRIDE 41 /* Q[15] R[5] q[15] r[5] c  (src/quadratic_cost.jl:16-22) */

#define QLN_OK 0
#define QLN_ERR_INVALID_ARGUMENT (-1)
#define QLN_ERR_HIP (-2)
#define QLN_ERR_NO_DEVICE (-3)
#define QLN_ERR_UNSUPPORTED (-4)

/* flags for the Jacobian entry points */
#define QLN_JAC_WRITE_CONSTANTS 1u

/* qln_batch_desc.jac_format: layout of the step-block section of vals (see "Layouts") */
#define QLN_JAC_FORMAT_DENSE_BLOCKS 0 /* one dense 15x20 block per dynamics knot: the reference's unit of work */
#define QLN_JAC_FORMAT_STRUCTURAL 1   /* only the structurally non-zero entries of every block */

typedef struct qln_handle qln_handle;

/* PlanarQuadruped (src/planar_quadruped.jl:11-20) */
typedef struct qln_model {
    double g, mb, mf, lb, l1, l2;
} qln_model;

/* A batch of B landing problems with a common horizon N.  All pointers are HOST
 * pointers; qln_create copies them to the device.  Mirrors the arguments of
 * HybridNLP(model, obj, init_mode, k_trans, N, x0, xf) (src/nlp.jl:34-37). */
typedef struct qln_batch_desc {
    int32_t B;                /* problems */
    int32_t N;                /* knot points per problem (>= 2) */
    qln_model model;
    const int32_t* k_trans;   /* [B], 1-based start index of mode 3, 1 <= k_trans <= N+1 */
    const int32_t* init_mode; /* [B], 1 or 2 */
    const double* x0;         /* [B][15] */
    const double* xf;         /* [B][15] */
    const double* cost;       /* [cost_batch][N][41] per-knot diagonal QuadraticCost (obj vector); NULL = none yet:
                                 build it on the device with qln_set_lqr_cost before evaluating f / grad */
    int32_t cost_batch;       /* 1 = one table shared by all problems, or B */
    int64_t z_stride;         /* doubles between consecutive problems in Z/grad; 0 -> n_nlp (dense) */
    int32_t align;            /* c_off/j_off are rounded up to a multiple of this many doubles;
                                 0 -> 16 (128 B).  j_off is always kept even. */
    int32_t jac_format;       /* QLN_JAC_FORMAT_* */
} qln_batch_desc;

typedef struct qln_dims {
    int32_t B, N;
    int32_t n_nlp;        /* 20N-5                           (src/nlp.jl:86) */
    int32_t m_nlp_max;    /* max_b 18N - k_trans(b) + 16     (src/nlp.jl:87) */
    int32_t nnz_max;      /* max_b nnz(b) */
    int32_t nnz_dynamic;  /* state-dependent values at the head of a problem's vals segment: 300(N-1)+N with dense
                             blocks; the largest per-problem count of the batch in the structural format */
    int64_t z_stride;
    int64_t z_total;      /* doubles to allocate for Z / grad */
    int64_t c_total;      /* doubles to allocate for c */
    int64_t j_total;      /* doubles to allocate for vals */
} qln_dims;

const char* qln_last_error(void);        /* thread-local message of the last failing call */
/* for the companion libraries of this ABI (qln_multi.h): records `msg` in the same slot and returns `code` */
int qln_set_last_error(int code, const char* msg);
const char* qln_version(void);

/* Lifetime.  `device` is a HIP device ordinal. */
int qln_create(const qln_batch_desc* desc, int device, qln_handle** out);
int qln_destroy(qln_handle* h);
/* What qln_create will lay out for `desc`, without a device: the sizes and the per-problem offsets (exclusive scans of
 * m_nlp(b) / nnz(b) rounded up to desc->align; src/nlp.jl:48-87 per problem).  Host arithmetic only -- the same code
 * qln_create runs first; desc->x0 / xf / cost are not read.  c_off, j_off: [B] or NULL. */
int qln_layout(const qln_batch_desc* desc, qln_dims* dims, int64_t* c_off, int64_t* j_off);
/* All launches go to `hip_stream` (a hipStream_t; NULL = the default stream). */
int qln_set_stream(qln_handle* h, void* hip_stream);
int qln_synchronize(qln_handle* h);

/* Sizes and index maps (num_primals/num_duals/cinds/lb/ub of src/nlp.jl:48-87). */
int qln_get_dims(const qln_handle* h, qln_dims* out);
int qln_get_offsets(const qln_handle* h, int64_t* c_off /*[B]*/, int64_t* j_off /*[B]*/);
int qln_problem_dims(const qln_handle* h, int32_t b, int32_t* m_nlp, int32_t* nnz);
/* number of state-dependent values at the head of problem b's vals segment (step blocks + N clearance entries) */
int qln_problem_nnz_dynamic(const qln_handle* h, int32_t b, int32_t* nnz_dynamic);
int qln_constraint_index_ranges(const qln_handle* h, int32_t b, int32_t cinds[14]); /* 1-based [start,end] x 7 */
int qln_constraint_bounds(const qln_handle* h, int32_t b, double* lb, double* ub);
/* 0-based (row, col) of every entry of problem b's vals segment (MOI.jacobian_structure, src/moi.jl:31-33,
 * restricted to the jac_c! write-set). */
int qln_jacobian_structure(const qln_handle* h, int32_t b, int32_t* rows, int32_t* cols);

/* Batched, device-pointer, stream-ordered (asynchronous) evaluation. */
int qln_eval_objective(qln_handle* h, const double* Z, double* f);                 /* src/costs.jl:6-16  */
int qln_eval_objective_gradient(qln_handle* h, const double* Z, double* grad);     /* src/costs.jl:23-34 */
int qln_eval_constraint(qln_handle* h, const double* Z, double* c);                /* src/constraints.jl:145-158 */
int qln_eval_constraint_jacobian(qln_handle* h, const double* Z, double* vals, uint32_t flags); /* :212-291 */
/* The fused hot path: eval_c! and jac_c! of every knot of every problem in one launch. */
int qln_eval_constraint_and_jacobian(qln_handle* h, const double* Z, double* c, double* vals, uint32_t flags);
/* Everything an NLP iteration asks of the evaluator from ONE read of Z: f = eval_f, grad = grad_f!, c = eval_c!,
 * vals = jac_c! (src/costs.jl:6-34, src/constraints.jl:145-158, 212-291) in a single launch -- the wave that has a
 * problem's slice of Z in LDS for the constraint rows also forms the objective terms and the gradient from it.  Same
 * layouts and the same bits as the separate entry points.  Needs a cost table. */
int qln_eval_all(qln_handle* h, const double* Z, double* f, double* grad, double* c, double* vals, uint32_t flags);
/* The pair a line search -- or Ipopt's filter at a trial point, which calls eval_f and eval_g at the same x (src/moi.jl:1-3,
 * 10-13; 1696 + 1696 of the reference run's 4222 callbacks, src/main.ipynb:717-722) -- asks for: f = eval_f and c = eval_c!
 * from ONE read of Z in one launch, no derivatives.  Same layouts and the same bits as qln_eval_objective and
 * qln_eval_constraint.  Needs a cost table. */
int qln_eval_objective_and_constraint(qln_handle* h, const double* Z, double* f, double* c);
int qln_jacobian_init_constants(qln_handle* h, double* vals);
/* Products with the constraint Jacobian of jac_c! (src/constraints.jl:212-291) at Z, for the caller side of the path
 * (solver iterations on the GPU).  The Jacobian is not read from memory: every step block is re-derived
 * from Z in registers, so no vals buffer is involved and the result is the same for either jac_format.
 *   qln_eval_constraint_jvp:  y = J(Z) v      v: layout of Z (z_stride), y: layout of c (c_off)
 *   qln_eval_constraint_vjp:  g = J(Z)^T lam  lam: layout of c, g: layout of Z (entries past n_nlp are not touched)
 * Device pointers, stream-ordered. */
int qln_eval_constraint_jvp(qln_handle* h, const double* Z, const double* v, double* y);
int qln_eval_constraint_vjp(qln_handle* h, const double* Z, const double* lam, double* g);
/* The Hessian of the Lagrangian -- the second-order callback of an MOI.AbstractNLPEvaluator (:Hess), which the reference
 * does not offer (src/moi.jl:26-28 declares [:Grad, :Jac], so Ipopt runs L-BFGS).  For problem b, with a scalar sigma_b
 * and multipliers mu in the layout of c:
 *
 *   H_b = sigma_b d2 eval_f(Z) + sum_i mu_i d2 c_i(Z),  returned as the lower triangle (row >= col) in a fixed sparse pattern.
 *
 * H_b is block-diagonal over knots (dynamics row block k is linear in x_{k+1}; the objective is a sum over knots of
 * h_k l_k(x_k, u_k); clearance row k involves only theta_k; the initial, terminal, contact and final-control rows are linear).
 *   Step block k = 1..N-1, variables z_k = Z[20(k-1) .. 20(k-1)+19] = (x_k[0..14], F1x, F1y, F2x, F2y, h_k):
 *     H_k = sigma d2(h_k l_k) + d2(mu_dyn,k . M_k rk4_mode(k)(x_k, u_k)) + mu_clr,k c''(theta_k) e2 e2'
 *     M_k = the jump mask JUMP_DIAG (quirk Q1) at the transition knot k_trans-1, the identity elsewhere: multipliers on
 *     masked rows contribute nothing.
 *   Objective part (u_k[4] = h_k; Q, R, q, r of the knot's 41-double cost record): h Q_i on the x diagonal, h R_i on the
 *     force diagonal (i < 4), Q_i x_i + q_i in (h, x_i), R_i u_i + r_i in (h, F_i), 2(R_4 h + r_4) + h R_4 in (h, h).
 *     This is the Hessian of eval_f, the FUNCTION -- not the Jacobian of grad_f!: quirk Q2 drops d(h l)/dh from the
 *     gradient, and the Jacobian of that gradient is not symmetric.
 *   Terminal block: the diagonal of x_N, sigma Qf_i, plus the clearance term at i = 2.
 *   Clearance c = y_b - (lb/2)|sin theta|: its second derivative is taken on the branch quirk Q3's Jacobian takes --
 *     +(lb/2) sin theta for theta > 0, -(lb/2) sin theta otherwise: the derivative of the entry jac_c! writes.
 *   Only the dynamics rows and the clearance rows of mu are read; the other rows are linear and never read.
 * The step's second derivatives are few (the polynomial step of qln_kernels.hip: no force x force and no theta-coupled
 * term survives), so a step block has 55 lower-triangle entries whatever the mode: 34 of mu . M rk4 and the objective's
 * diagonal and h row.
 * Layout: problem b at hvals + b*h_stride, h_stride = nnz = 55(N-1)+15 rounded up to desc.align (N is shared and the
 * pattern depends neither on k_trans nor on the mode, so the layout is uniform).  Inside a segment the N-1 step blocks come
 * first, with global indices (20(k-1)+r, 20(k-1)+c) and their 55 values in column-major order of the pattern, then the 15
 * terminal diagonal values.  An entry that is structurally zero in a knot's mode is an exact zero.  A buffer of
 * (B-1)*h_stride + nnz doubles holds the batch (no padding behind the last problem). */
#define QLN_HESS_STEP_NNZ 55
#define QLN_HESS_TERM_NNZ 15
/* device-free: nnz of one problem and the stride between problems for `desc` (desc->N and desc->align are read) */
int qln_hessian_layout(const qln_batch_desc* desc, int32_t* nnz, int64_t* h_stride);
/* device-free: 0-based (row, col), row >= col, of the nnz entries of a segment, in the order of the values */
int qln_hessian_structure(int32_t N, int32_t* rows, int32_t* cols);
/* device pointers, stream-ordered; sigma: [B] or NULL (= 1.0 for every problem); mu: layout of c.  Needs a cost table. */
int qln_eval_hessian_lagrangian(qln_handle* h, const double* Z, const double* sigma, const double* mu, double* hvals);
/* The Hessian-vector product of the Lagrangian -- the matrix-free second-order callback of an MOI.AbstractNLPEvaluator
 * (:HessVec, eval_hessian_lagrangian_product), which Newton-CG, trust-region Steihaug and matrix-free SQP ask for.  For
 * problem b, with v and y in the layout of Z (z_stride), a scalar sigma_b and multipliers mu in the layout of c:
 *
 *   y_b = (sigma_b d2 eval_f(Z_b) + sum_i mu_i d2 c_i(Z_b)) v_b
 *
 * The operator is the one qln_eval_hessian_lagrangian returns, with the same conventions: the objective part is the
 * Hessian of eval_f, the FUNCTION (quirk Q2), the jump mask (quirk Q1) zeroes the multipliers of the transition knot's
 * masked rows, the clearance curvature takes quirk Q3's branch, and only the dynamics and clearance rows of mu are read.
 * Nothing is stored: each knot's 55 step-block values are formed in registers and contracted with v there.
 *   Step block k acts on z_k = Z[20(k-1) .. 20(k-1)+19] (y's entries of the same range); the terminal block is the
 *   15-entry diagonal on x_N = Z[20(N-1) .. 20(N-1)+14].
 * Every entry of y below n_nlp is written (an exact zero where H's row is empty for this v); entries from n_nlp to
 * z_stride are never written, and the entries of Z and v there are never read.
 * Device pointers, stream-ordered; sigma: [B] or NULL (= 1.0 for every problem).  Needs a cost table. */
int qln_eval_hessian_lagrangian_product(qln_handle* h, const double* Z, const double* sigma, const double* mu,
                                        const double* v, double* y);
/* One Gauss-Newton step on the constraint violation for every problem of the batch (the solver
 * iteration on the GPU, consuming the Jacobian where it is produced).  For problem b
 *     dZ_b = D x,  x = the minimum-norm minimiser of || A D x + rho ||_2   (subject to ||x|| <= radius[b] if given),
 * rho_i = c_i on the equality rows, min(c_i, 0) on the clearance rows (bounds of src/nlp.jl:66-69), A = jac_c(Z) without
 * the rows of satisfied clearance constraints, D = diag(col_scale) (NULL = identity; a zero holds a variable fixed).
 * Computed by at most max_iters CGLS iterations, stopped early once ||(AD)'(A dZ + rho)|| <= rel_tol * ||(AD)' rho|| or
 * when the iterate leaves the trust radius (it is then cut at the boundary, Steihaug-Toint).  One wavefront per
 * problem with every vector in LDS; the Jacobian is re-derived from Z inside the products and never stored.
 * c = eval_c!(Z) as written by qln_eval_constraint.  radius: [B] or NULL; col_scale: [n_nlp] or NULL (shared by all
 * problems).  info (may be NULL): QLN_GN_INFO_STRIDE doubles per problem {iterations done, ||(AD)' rho||^2,
 * ||(AD)'(A dZ + rho)||^2, ||A dZ + rho||^2 (the linear model's prediction), ||rho||^2, 1 if cut at the radius,
 * ||x||, 0}.  dZ has the layout of Z.  QLN_ERR_UNSUPPORTED if a problem does not fit the 160 KB of LDS of a CU
 * (N > 149).  Device pointers, stream-ordered. */
#define QLN_GN_INFO_STRIDE 8
int qln_gauss_newton_step(qln_handle* h, const double* Z, const double* c, double* dZ, int32_t max_iters, double rel_tol,
                          const double* radius /*[B] or NULL*/, const double* col_scale /*[n_nlp] or NULL*/,
                          double* info /*[B][QLN_GN_INFO_STRIDE] or NULL*/);
/* Batched solve of the reference NLP on the GPU -- the caller of this evaluator in the reference, solve() of
 * src/moi.jl:46-103 (objective eval_f, constraints eval_c! with the bounds of src/nlp.jl:66-69, the variable bounds
 * of src/moi.jl:51-67 incl. quirk Q6), for every problem of the batch at once, one wavefront per problem.
 * Method (quadruped_landing_amd/csrc/qln_ilqr_kernels.hip): augmented-Lagrangian iLQR -- the states are eliminated by
 * rolling the controls out from x0 with the evaluator's own RK4 step, a Newton-type step is a Riccati sweep over the
 * knots in LDS (the step blocks are the evaluator's closed form), terminal / final-control rows, clearance rows and
 * the state bounds carry multipliers + penalty, the bounds on the step length h are kept inside the sweep.
 * Z (device, layout of Z): in = initial guess, of which the CONTROLS u_k are used (h clamped to its bounds; the
 * states are rolled out from x0); out = the solution: its dynamics / initial-condition rows are zero to the last bit
 * by construction, the remaining rows to options->tol_violation when status = 0.
 * info (device, may be NULL): QLN_SOLVE_INFO_STRIDE doubles per problem {outer iterations, iLQR iterations, objective
 * f of the returned Z (the bits qln_eval_objective gives for it), violation of the returned Z (what
 * qln_constraint_violation gives for its eval_c!, and solve()'s bounds on theta and quirk Q6's on the knots after the
 * first), final penalty rho, status (0 = converged to tol_violation, 1 = iteration limit, 2 = no descent at the largest
 * penalty: an inner loop took twelve failed steps on end, which max_inner < 12 rules out before the rescue phase),
 * augmented cost, last accepted step length, sum of h, LM mu at exit, five phase timers, 1 if the rescue phase
 * ran}.  f and the violation are measured on the trajectory that is handed back (the RK4 roll-out); status is the solver's
 * stop test on its own closed-form roll-out of the same controls, which differs from it by rounding (1e-15 per step): with
 * status = 0 the reported violation can exceed tol_violation by that much.  max_outer = 0 and rescue_outer = 0 make the
 * call a roll-out-and-report of the given controls (status 1).
 * The reference holds nothing to compare the iterates with (it hands its callbacks to Ipopt); the result is judged by
 * this evaluator: qln_eval_constraint + qln_constraint_violation and qln_eval_objective on the returned Z.  The iterates
 * themselves are held to a numpy restatement of the method run in double and in 80-bit extended precision
 * (tests/ilqr_ref.py, tests/test_gpu_ilqr_iterates.py): controls, counts, step lengths, mu and rho of single and of twelve
 * iterations, of runs to convergence, of steps without descent, a stalled inner loop and the rescue phase.  The sweep differentiates the step the roll-out takes: the clock x[14] is kept through the jump, so a cost
 * with a weight on it is handled consistently.
 * Needs a cost table.  QLN_ERR_UNSUPPORTED if a problem does not fit the LDS of a CU (N > ~650).  Stream-ordered.
 * The first call on a handle allocates the solver's device scratch, 494 N doubles per problem (158 KB at N = 40: step
 * entries, feedback laws, the sixteen trial trajectories, multipliers), kept until qln_destroy -- a 10-GB hipMalloc at
 * B = 65 536 that took between a few ms and 2 s on this pool's boxes: make one throw-away call before timing. */
typedef struct qln_solve_options {
    int32_t max_outer;        /* multiplier updates                                   default 80   */
    int32_t max_inner;        /* iLQR iterations per multiplier update (inexact inner solves pay)   default 6 */
    double tol_violation;     /* stop when the violation is <= this                   default 1e-6 (solve()'s c_tol) */
    double inner_tol;         /* inner loop ends when the cost decrease is below inner_tol (1 + |J|)   default 1e-7 */
    double rho0, rho_factor, rho_max;  /* penalty schedule                            default 3, 5, 1e8 */
    double h_min, h_max;      /* bounds on the step length (src/moi.jl:58-61)         default 0.001, 0.02 */
    double theta_min, theta_max;       /* bounds on the body angle (src/moi.jl:54-56) default -pi/2, pi/2 */
    int32_t q6_bounds;        /* the lower bounds of quirk Q6 (yb_{k+1}, x1_{k+1} >= 0, src/moi.jl:64-65)  default 1 */
    int32_t exact_h_gradient; /* 0: objective gradient as the reference's grad_f!, which has no d(h l)/dh (quirk Q2) --
                                 the stage weights h_k are frozen within an iteration; 1: the exact gradient (couples the
                                 step lengths to the cost: use tighter inner solves, max_inner ~30)             default 0 */
    double h_prox;            /* proximal weight on the step lengths in the Newton system (it vanishes at a fixed point):
                                 with the reference's gradient the objective does not see h, the h_k are fixed by the
                                 constraints alone and wander along flat directions without it          default 1e4 */
    int32_t rescue_outer;     /* a problem still above the tolerance after max_outer updates gets this many more, with
                                 accurate inner solves (60 iterations) from a penalty of at most 1e6; info[15] = 1
                                 where that phase ran                                                     default 20 */
} qln_solve_options;
#define QLN_SOLVE_INFO_STRIDE 16
int qln_solve_default_options(qln_solve_options* opt);
/* The variable bounds solve() hands to Ipopt (src/moi.jl:51-67), for a caller that keeps Ipopt: x_l / x_u are host
 * arrays of n_nlp = 20N-5 doubles, -inf / +inf where the reference sets none.  theta in [theta_min, theta_max] at every
 * knot, h in [h_min, h_max] at every dynamics knot, and -- with q6_bounds != 0, the default -- the two lower bounds of
 * src/moi.jl:64-65 exactly where the reference puts them: 1-based 22+20(k-1) and 24+20(k-1), i.e. yb_{k+1} >= 0 and
 * x1_{k+1} >= 0 (quirk Q6; the source comment says "F", the Ipopt header of the shipped run counts 120 such variables,
 * src/main.ipynb:222).  opt = NULL: the defaults, which are the reference's literals.  Needs no handle and no GPU. */
int qln_variable_bounds(int32_t N, const qln_solve_options* opt /* NULL = defaults */, double* x_l, double* x_u);
int qln_solve(qln_handle* h, double* Z, const qln_solve_options* opt /* NULL = defaults */, double* info);
/* the same as a host form (see "Host forms" above: Z copied in, solved on the GPU, copied back) -- what the Julia veneer
 * calls in place of `solve(Z0, nlp)`.  info (host, may be NULL): [B][QLN_SOLVE_INFO_STRIDE]. */
int qln_solve_host(qln_handle* h, double* Z, const qln_solve_options* opt, double* info);
/* Least-squares estimate of the Lagrange multipliers of every problem at ANY point Z, and its KKT residual: what says
 * whether a trajectory -- qln_solve's, Ipopt's, a file's -- is a stationary point and not only a feasible one, and what
 * a caller that keeps Ipopt hands it as the dual start.  Convention: MOI's and Ipopt's, the one
 * qln_eval_hessian_lagrangian uses: L = f + lam' c, stationarity reads grad f + J' lam - z_L + z_U = 0.  For problem b
 *   active rows   every equality row; clearance row i (the last N rows of c) iff !(c_i > act_tol), so a NaN is active.
 *                 A = jac_c(Z) restricted to them.
 *   fixed         with bound_tol >= 0, variable j iff Z_j <= l_j + bound_tol or Z_j >= u_j - bound_tol, (l, u) exactly
 *                 what qln_variable_bounds(N, bounds) returns (theta, h, and quirk Q6's entries when q6_bounds != 0; only
 *                 h_min, h_max, theta_min, theta_max and q6_bounds of `bounds` are read).  bound_tol < 0: none is fixed.
 *                 D = diag(free), entries 0 or 1.
 *   row scaling   row_scaling != 0: w_i = the 2-norm of row i of A D (1 where that is 0); row_scaling == 0: w = 1.
 *                 T = (A D)' W^-1, an n x m operator.
 *   solve         min_y || T y + D g ||_2 by CGLS started at 0 (r = -D g, s = T' r, p = s, gamma = s.s; then q = T p,
 *                 alpha = gamma / q.q, y += alpha p, r -= alpha q, s = T' r, beta = gamma_new / gamma, p = s + beta p),
 *                 stopped at max_iters or once gamma <= rel_tol^2 gamma_0.  Started at 0 the iterates converge to the
 *                 minimum-norm y although T is rank deficient (at a solved landing the stacked Jacobian is: most h on a
 *                 bound, x1 on quirk Q6's); the residual is unique either way.  Row scaling cuts the iteration count
 *                 several times over and is what a caller wants unless it compares iterates.
 *   lam           = W^-1 y, in the layout of c; an exact 0 on the inactive rows.
 *   lag           = g + A' lam, in the layout of Z (may be NULL): the dual infeasibility on the free columns, the bound
 *                 multipliers z_L - z_U on the fixed ones.  Formed by one more transposed product with D = I, not from the
 *                 recurrence's r.  Every entry below n_nlp is written, entries from n_nlp to z_stride never.
 *   info          (may be NULL) QLN_MULT_INFO_STRIDE doubles per problem, the counts exact integers: {0 iterations done,
 *                 1 ||D g||^2, 2 gamma at exit, 3 ||r||^2 of the recurrence, 4 max |lag_j| over the free columns, 5 active
 *                 clearance rows, 6 fixed variables, 7 active clearance rows with lam_i > 0 (the wrong sign for c_i >= 0:
 *                 reported, not projected), 8 fixed variables whose lag_j contradicts their bound (< 0 at a lower, > 0 at
 *                 an upper; never counted when both bounds are within bound_tol), 9 max |lam_i c_i| over the active
 *                 clearance rows, 10 max |lam_i|, 11 max |g_j| over the free columns, 12-15 zero}.  The four maxima (4,
 *                 9, 10, 11) ignore a NaN entry (fmax from 0); the sums 1, 2 and 3 carry it, so they are what tells a
 *                 non-finite g or Z.
 * g is the caller's, in the layout of Z, so no cost table is needed.  qln_eval_objective_gradient gives the reference's
 * grad_f!, which is what Ipopt sees; by quirk Q2 it has no d(h l)/dh, so with it the h-columns of lag measure
 * stationarity against that field and not against the gradient of eval_f.  A caller may pass the exact gradient instead.
 * c = eval_c!(Z) as written by qln_eval_constraint; only its clearance rows are read.
 * One wavefront per problem with every vector in LDS, the Jacobian re-derived from Z inside the products and never
 * stored, as in qln_gauss_newton_step: (4 n_nlp + 4 m_nlp + N) doubles per problem with m_nlp taken at k_trans = 1,
 * QLN_ERR_UNSUPPORTED if that does not fit the 160 KB of LDS of a CU (the bound follows from the count; with today's
 * layout 153 N + 40 doubles, so N > 133).  QLN_ERR_INVALID_ARGUMENT, without touching a GPU, for a NULL h, Z, c, g or
 * lam, max_iters < 0, a negative or non-finite act_tol or rel_tol, a non-finite bound_tol, or bounds with min > max.
 * Device pointers, stream-ordered. */
#define QLN_MULT_INFO_STRIDE 16
int qln_estimate_multipliers(qln_handle* h, const double* Z, const double* c, const double* g,
                             const qln_solve_options* bounds /* NULL = defaults; only the bound fields are read */,
                             double act_tol, double bound_tol, int32_t row_scaling, int32_t max_iters, double rel_tol,
                             double* lam, double* lag /* may be NULL */, double* info /* [B][QLN_MULT_INFO_STRIDE] or NULL */);
/* the same as a host form (see "Host forms" above): Z, c, g copied in, lam and -- where asked for -- lag and info copied
 * back, through the one staging path; the padding of lam and lag comes back as zeros. */
int qln_estimate_multipliers_host(qln_handle* h, const double* Z, const double* c, const double* g,
                                  const qln_solve_options* bounds, double act_tol, double bound_tol, int32_t row_scaling,
                                  int32_t max_iters, double rel_tol, double* lam, double* lag, double* info);
/* OPT-IN EXTENSION WITHOUT A REFERENCE ORACLE.  The leg-length ("kinematic") constraint group exists in the reference
 * only as commented-out code (src/constraints.jl:115-138 values, :276-288 Jacobian, src/nlp.jl:60,70 index range and
 * bounds): the reference never computes it, so nothing can be compared with it, and it is NOT part of c / vals above.
 *   d[b][2k]   = |pb_k - p1_k|,  d[b][2k+1] = |pb_k - p2_k|      k = 0..N-1   (as the commented source defines them)
 *   bounds     0 <= d <= l1 + l2 + lb/2                                        (qln_kinematic_bounds)
 *   jac[b][2k+i][4] = d(row)/d(xb, yb, x_foot, y_foot) = (+e, -e) with e = (pb - p_foot)/|pb - p_foot|: the
 *   mathematically correct Jacobian, in the columns 20k + {0, 1, 3, 4} (foot 1) / 20k + {0, 1, 5, 6} (foot 2) of Z --
 *   the commented Jacobian indexes x[7:8] / x[9:10], which are not the feet, and is not reproduced.
 * Checked against an independent numpy statement of the formula and its complex-step derivative only
 * (tests/test_gpu_kinematic.py).  d: [B][2N] doubles, jac (may be NULL): [B][2N][4].  Device pointers, stream-ordered. */
int qln_eval_kinematic_constraint(qln_handle* h, const double* Z, double* d, double* jac);
int qln_kinematic_bounds(const qln_handle* h, double* lower, double* upper); /* the two scalars */
/* OPT-IN EXTENSION WITHOUT A REFERENCE ORACLE.  The reference has no friction constraint at all (its NLP lets the ground
 * pull on a foot); the path's stated scope names one, so it is offered as a group of its own, NOT part of c / vals above:
 * the friction pyramid |F_x| <= mu F_y of every foot that stands on the ground during dynamics knot k = 0..N-2, as two
 * linear rows per foot
 *   d[b][4k + 0] = mu F1y_k - F1x_k,  d[b][4k + 1] = mu F1y_k + F1x_k,  d[b][4k + 2], [4k + 3]: the same for foot 2,
 *   bounds 0 <= d < +inf (the two rows of a foot add up to 2 mu F_y >= 0: the ground only pushes).
 * Which feet stand is the mode schedule of the dynamics rows (src/constraints.jl:23-37): before the transition knot only
 * the foot of init_mode, from it on both; the rows of a foot in flight are 0 with zero derivatives (its force entries
 * drive the leg, src/planar_quadruped.jl:36-79).
 *   jac[b][4k + i][2] = d(row)/d(F_x, F_y) of that foot = (-1, mu) / (+1, mu), in the columns 20k + 15 + {0, 1} (foot 1) /
 *   20k + 15 + {2, 3} (foot 2) of Z.
 * Checked against a numpy statement of the same formula (tests/test_gpu_kinematic.py).  d: [B][4(N-1)] doubles, jac (may be
 * NULL): [B][4(N-1)][2].  Device pointers, stream-ordered. */
int qln_eval_friction_cone(qln_handle* h, const double* Z, double mu, double* d, double* jac);
/* viol[b] = largest violation of problem b's constraint bounds (src/nlp.jl:66-69) by c: max |c_i| over the equality
 * rows, max(0, -c_i) over the clearance rows -- the "Constraint violation" Ipopt prints for the reference's solve
 * (src/main.ipynb:712).  Device pointers; c as written by qln_eval_constraint. */
int qln_constraint_violation(qln_handle* h, const double* c, double* viol /*[B]*/);
/* The step before the path: the notebook's initial guess Z0 = packZ(nlp, Xguess, Uref)
 * (src/main.ipynb:181-198, src/nlp.jl:94-102, src/ref_traj.jl:19-34) for every problem of the batch, written
 * on the device in the handle's Z layout.  Needs k_trans >= 2 for every problem (the notebook divides by
 * k_trans - 1). */
int qln_initial_guess(qln_handle* h, double* Z);
/* The synthetic workload of SURVEY.md 8d generated on the device (8f-3): per-problem random drop states
 *   theta0 ~ U(theta_deg) degrees, y2_0 ~ U(y2), vby0 = -sqrt(two_g * H) with H ~ U(drop_height), omega0 ~ U(omega),
 * written into x0_template's entries 3, 7, 9, 10 (1-based; the notebook's xinit, src/main.ipynb:114-124) and mirrored for
 * init_mode 2.  The uniform draws are those of numpy.random.default_rng(seed) (PCG64) consumed in the host recipe's
 * order -- theta0[B], y2_0[B], H[B], omega0[B] starting `stream_offset` draws into the stream -- bit for bit: pcg_state /
 * pcg_inc are numpy.random.PCG64(seed).state's 128-bit `state` and `inc` as {high, low} words.  Replaces the x0 the
 * handle was created with. */
typedef struct qln_drop_state_sampler {
    uint64_t pcg_state[2], pcg_inc[2];
    int64_t stream_offset;
    double x0_template[15];
    double theta_deg[2], y2[2], drop_height[2], omega[2];  /* {low, high} */
    double two_g;                                          /* 2 * 9.81 in the recipe */
} qln_drop_state_sampler;
int qln_sample_drop_states(qln_handle* h, const qln_drop_state_sampler* s);
/* The ragged workload's per-problem descriptors drawn on the device (k_trans ~ U{2..N-1},
 * init_mode ~ U{1,2}; 8f-3): numpy.random.Generator.integers(low, high, size = count) on the PCG64 stream -- Lemire's
 * multiply-shift on 32-bit draws, the low half of a 64-bit output first -- starting `draw_offset` 32-BIT draws into the
 * stream.  out: HOST array [count] (the draws are made on `device` and copied back: they are the descriptors qln_create is
 * given).  numpy REJECTS a draw with probability < (high - low) / 2^32 and redraws, which shifts every later position of
 * the stream by one: *rejected returns how many draws of this call numpy would have rejected, and unless it is 0 the
 * output -- and every stream position behind this call, e.g. a qln_drop_state_sampler.stream_offset computed from the
 * draw count -- is NOT numpy's: fall back to the host generator for that seed.  (Two such calls of count B each consume
 * exactly B 64-bit outputs: the drop states then start at stream_offset = B.  A range of ONE value consumes no draw at
 * all, as in numpy.)  Needs no handle. */
int qln_sample_bounded_integers(int device, const uint64_t pcg_state[2], const uint64_t pcg_inc[2], int64_t draw_offset, int32_t low,
                                int32_t high /* exclusive */, int64_t count, int32_t* out, int64_t* rejected);
/* Time-varying LQR tracking (TVLQR) along a batch of reference trajectories, and the closed-loop roll-out under its gains.
 * For problem b the reference is its slice of Zref (layout of Z, z_stride): x_ref,k, k = 1..N, and
 * u_ref,k = (F1x, F1y, F2x, F2y, h_k), k = 1..N-1.  Deviations dx_k = x_k - x_ref,k.  Only the four forces are fed back,
 * du_k = -K_k dx_k; the step length h_k stays at the reference's value (the contact schedule is indexed by knot, as in
 * the NLP).
 *   A_k = d x_{k+1} / d x_k (15x15) and B_k = d x_{k+1} / d F_k (15x4) at (x_ref,k, u_ref,k), of the map the roll-out
 *   applies: the knot's RK4 step followed, at the transition knot k_trans-1, by the jump map.  That is the evaluator's dense
 *   step block, columns 0..18, with one deliberate exception: quirk Q1's mask zeroes row 14 (the clock) at the jump knot,
 *   but the jump map keeps x[14], so A_k's row 14 there is the true derivative (1 on the diagonal).  This changes only
 *   P[14][14] at knots 1..k_trans-1 and never K: the clock feeds no other state and no force feeds the clock.
 *   Weights are shared by the batch and diagonal: Q (15), R (4), Qf (15), not scaled by h_k; R_i > 0, Q_i >= 0,
 *   Qf_i >= 0, all finite (else QLN_ERR_INVALID_ARGUMENT).
 *   J = sum_{k=1}^{N-1} (dx_k' Q dx_k + du_k' R du_k) + dx_N' Qf dx_N   (no 1/2 factors)
 *   P_N = Qf;  Quu = R + B'P_{k+1}B,  Qux = B'P_{k+1}A,  K_k = Quu^-1 Qux,  P_k = Q + A'P_{k+1}A - Qux'K_k, formed on the
 *   lower triangle (P_k is exactly symmetric).  dx_1' P_1 dx_1 is the optimal cost of the linearised problem.
 * Every N >= 2 and every k_trans in [1, N+1] is supported (the sweep keeps one knot at a time: no limit on N). */
#define QLN_TRACK_NU 4       /* fed-back controls: the four contact forces */
#define QLN_TRACK_P_NNZ 120  /* packed lower triangle of a 15x15 cost-to-go */
/* K: [B][N-1][4][15] row-major; P (may be NULL: not written): [B][N][120], row i >= j at i(i+1)/2 + j.
 * Zref, K, P: device pointers, stream-ordered.  Qdiag / Rdiag / Qfdiag: HOST arrays, passed by value in the kernel
 * arguments (no upload).  Needs no cost table. */
int qln_tracking_lqr(qln_handle* h, const double* Zref, const double* Qdiag, const double* Rdiag, const double* Qfdiag,
                     double* K, double* P);
/* Closed-loop roll-out of the nonlinear hybrid system under the handle's mode schedule:
 *   x_1 = x0[b] (NULL: the handle's x0), F_k = F_ref,k - K_k (x_k - x_ref,k), h_k = h_ref,k,
 *   x_{k+1} = the evaluator's RK4 step + jump map (bit for bit the step qln_solve's roll-out takes).
 * Zout gets the states and the applied controls (h included) in the layout of Z; it can be handed to qln_eval_constraint /
 * qln_eval_objective / qln_constraint_violation.  Entries from n_nlp to z_stride are never written.  K == NULL is the
 * open-loop roll-out of Zref's controls.  Zout must not overlap Zref.  x0: device [B][15] or NULL.  Stream-ordered. */
int qln_tracking_rollout(qln_handle* h, const double* Zref, const double* K, const double* x0, double* Zout);
/* the same as host forms (see "Host forms" above; Zout is in-out) */
int qln_tracking_lqr_host(qln_handle* h, const double* Zref, const double* Qdiag, const double* Rdiag, const double* Qfdiag,
                          double* K, double* P);
int qln_tracking_rollout_host(qln_handle* h, const double* Zref, const double* K, const double* x0, double* Zout);
/* Reverse-mode derivative (vector-Jacobian product) of qln_tracking_rollout.  Knots are 0-based here, k = 0..N-2 (knot k
 * is the header's k+1 above).  The forward map is exactly qln_tracking_rollout's:
 *   u_k = (F_ref,k - K_k (x_k - x_ref,k), h_ref,k),  x_{k+1} = Phi_k(x_k, u_k),  x_0 = x0[b] or the handle's x0,
 * where Phi_k is the RK4 step followed, at k+1 == k_trans-1, by the jump map.  Given a cotangent Zbar in the layout of Z,
 * which weights the states and the APPLIED controls (h included) that Zout holds, the reverse sweep is
 *   lam_{N-1} = Zbar[x_{N-1}]
 *   for k = N-2 .. 0:
 *     [A_k B_k] = d Phi_k / d(x_k, u_k) at Zout's (x_k, u_k)        (15 x 20, the h column included)
 *     ubar_k     = Zbar[u_k] + B_k' lam_{k+1}                         (5)
 *     Fref_bar_k = ubar_k[0:4],  href_bar_k = ubar_k[4]
 *     xref_bar_k = K_k' ubar_k[0:4]                                   (0 if K == NULL)
 *     Kbar_k     = -ubar_k[0:4] (x_k - x_ref,k)'                      (4 x 15)
 *     lam_k      = Zbar[x_k] + A_k' lam_{k+1} - K_k' ubar_k[0:4]
 *   x0_bar = lam_0
 * A_k, B_k are the true derivative of what the roll-out applies: the evaluator's closed-form step block, except that at
 * the jump knot, where quirk Q1's mask zeroes the clock row, the jump map keeps it -- row 14 there is 1 at x[14] and 1 at
 * h, as in qln_tracking_lqr (rows 4, 6 and 10-13 are zero).  The linearisation points are Zout's: the roll-out is not
 * re-run, and nothing checks that Zout is the roll-out of (Zref, K, x0).  The result is the derivative at the trajectory
 * Zout holds.  With K == NULL it is the reduced gradient of single shooting (controls -> trajectory).
 * Outputs (each may be NULL: not written; overwritten, not accumulated; none may overlap an input or another output):
 *   Zref_bar: layout of Z.  Every entry below n_nlp is written -- x_ref slots of knots 0..N-2, F_ref and h_ref slots, and
 *             exact zeros in the x_ref,N-1 slots, which the roll-out never reads; entries from n_nlp to z_stride never.
 *   K_bar:    [B][N-1][4][15], the layout of K.  QLN_ERR_INVALID_ARGUMENT if K == NULL and K_bar != NULL.
 *   x0_bar:   [B][15].
 * Zref is read for K_bar only (the states x_ref,k); it must still be non-NULL.  Every N >= 2, k_trans in [1, N+1] and
 * init_mode, as the forward call.  Device pointers, stream-ordered; needs no cost table. */
int qln_tracking_rollout_vjp(qln_handle* h, const double* Zref, const double* K, const double* Zout, const double* Zbar,
                             double* Zref_bar, double* K_bar, double* x0_bar);
/* the same as a host form (see "Host forms" above; Zref_bar is in-out) */
int qln_tracking_rollout_vjp_host(qln_handle* h, const double* Zref, const double* K, const double* Zout, const double* Zbar,
                                  double* Zref_bar, double* K_bar, double* x0_bar);
/* Forward-mode derivative (Jacobian-vector product) of qln_tracking_rollout: the tangent of Zout along a direction
 * (Zref_dot, K_dot, x0_dot) of the inputs, at the trajectory Zout holds.  Knots are 0-based, k = 0..N-2, and the forward map,
 * Phi_k and the blocks are those of qln_tracking_rollout_vjp: [A_k B_k] = d Phi_k / d(x_k, u_k) at Zout's (x_k, u_k) is the
 * evaluator's closed-form 15 x 20 step block, the h column included, and at the jump knot row 14 is the jump map's (1 at
 * x[14] and 1 at h), not quirk Q1's masked zero.  The linearisation points are Zout's: the roll-out is not re-run, and
 * nothing checks that Zout is the roll-out of (Zref, K, x0).  The sweep is
 *   dx_0 = x0_dot[b]                                                  (zeros if x0_dot == NULL)
 *   for k = 0 .. N-2:
 *     e_k  = x_k - x_ref,k                                            (Zout's x_k, Zref's x_ref,k)
 *     dF_k = Fref_dot_k - K_k (dx_k - xref_dot_k) - Kdot_k e_k        (4)
 *     dh_k = href_dot_k
 *     Zout_dot[u_k] = (dF_k, dh_k)
 *     dx_{k+1} = A_k dx_k + B_k (dF_k, dh_k)
 *   Zout_dot[x_k] = dx_k,  k = 0..N-1
 * where every term with K, K_dot, Zref_dot or x0_dot equal to NULL is an exact zero, and xref_dot_{N-1} is never read.  It
 * is the exact adjoint of qln_tracking_rollout_vjp: <Zbar, Zout_dot> = <Zref_bar, Zref_dot> + <K_bar, K_dot> + <x0_bar, x0_dot>.
 * Tangents (each may be NULL; all three NULL is QLN_ERR_INVALID_ARGUMENT):
 *   Zref_dot: layout of Z (entries from n_nlp to z_stride are not read).
 *   K_dot:    [B][N-1][4][15], the layout of K.  QLN_ERR_INVALID_ARGUMENT if K == NULL and K_dot != NULL.
 *   x0_dot:   [B][15].
 * Zout_dot: layout of Z.  Every entry below n_nlp is written; entries from n_nlp to z_stride never.  It must overlap no
 * input.  Zref is read for K_dot only (the states x_ref,k); it must still be non-NULL.  Every N >= 2, k_trans in [1, N+1]
 * and init_mode, as the forward call.  Device pointers, stream-ordered; needs no cost table. */
int qln_tracking_rollout_jvp(qln_handle* h, const double* Zref, const double* K, const double* Zout, const double* Zref_dot,
                             const double* K_dot, const double* x0_dot, double* Zout_dot);
/* the same as a host form (see "Host forms" above; Zout_dot is in-out) */
int qln_tracking_rollout_jvp_host(qln_handle* h, const double* Zref, const double* K, const double* Zout,
                                  const double* Zref_dot, const double* K_dot, const double* x0_dot, double* Zout_dot);
/* The closed-loop roll-out with a per-problem PLANT model, and its two sweeps.  The gains, the references and the mode
 * schedule are the handle's; what differs per problem is the model the dynamics read while rolling out:
 *   theta_b = model[b] = (g, mb, mf, lb), in this order (QLN_MODEL_NP doubles); Ib = mb * (lb * lb) / 12 per problem, formed as
 *   for the handle's model.  l1 and l2 enter only the kinematic rows and are not part of it.
 *   x_{k+1} = Phi_k(x_k, u_k; theta_b),  u_k = (F_ref,k - K_k (x_k - x_ref,k), h_ref,k)     (knots 0-based, k = 0..N-2)
 * Everything else -- layouts, NULL conventions of K and x0, overlap rules, what is written -- is qln_tracking_rollout's and
 * its sweeps', which these calls reduce to: with model == NULL (the handle's model for every problem), or with model[b]
 * equal to the handle's four values, qln_tracking_rollout_model's Zout is bit for bit qln_tracking_rollout's.
 * qln_tracking_lqr and qln_tracking_covariance keep the handle's model: the design model does not follow the plant.
 *   model: device, [B][QLN_MODEL_NP], or NULL.  The device forms do not validate it; a NaN in model[b] stays in problem b's
 *          outputs.  The host forms refuse a non-finite entry and mb, mf or lb <= 0 with QLN_ERR_INVALID_ARGUMENT.
 * Forward sweep (qln_tracking_rollout_model_jvp): qln_tracking_rollout_jvp's recursion with the model's tangent,
 *   dx_{k+1} = A_k dx_k + B_k (dF_k, dh_k) + G_k model_dot[b],   G_k = d Phi_k / d theta (15 x 4) at Zout's (x_k, u_k) and theta_b;
 *   A_k and B_k are formed at theta_b too, and dF_k is unchanged (the gains do not depend on the plant).  Rows 4, 6 and
 *   10-13 of G_k are zero at the jump knot, as A_k's; row 14 (the clock) always.  All four tangents NULL is
 *   QLN_ERR_INVALID_ARGUMENT; a NULL tangent equals a zero tensor in every value.  model_dot: device [B][QLN_MODEL_NP] or NULL.
 * Reverse sweep (qln_tracking_rollout_model_vjp): qln_tracking_rollout_vjp's recursion at theta_b, and
 *   model_bar[b] = sum_k G_k' lam_{k+1}       ([B][QLN_MODEL_NP] or NULL: not written; overwritten, not accumulated)
 *   It is the exact adjoint of the forward sweep:
 *   <Zbar, Zout_dot> = <Zref_bar, Zref_dot> + <K_bar, K_dot> + <x0_bar, x0_dot> + <model_bar, model_dot>.
 * Device pointers, stream-ordered; needs no cost table. */
#define QLN_MODEL_NP 4 /* g, mb, mf, lb: what the dynamics read */
int qln_tracking_rollout_model(qln_handle* h, const double* Zref, const double* K, const double* x0, const double* model,
                               double* Zout);
int qln_tracking_rollout_model_jvp(qln_handle* h, const double* Zref, const double* K, const double* Zout, const double* model,
                                   const double* Zref_dot, const double* K_dot, const double* x0_dot, const double* model_dot,
                                   double* Zout_dot);
int qln_tracking_rollout_model_vjp(qln_handle* h, const double* Zref, const double* K, const double* Zout, const double* model,
                                   const double* Zbar, double* Zref_bar, double* K_bar, double* x0_bar, double* model_bar);
/* the same as host forms (see "Host forms" above; Zout, Zout_dot and Zref_bar are in-out as in the forms without a model) */
int qln_tracking_rollout_model_host(qln_handle* h, const double* Zref, const double* K, const double* x0, const double* model,
                                    double* Zout);
int qln_tracking_rollout_model_jvp_host(qln_handle* h, const double* Zref, const double* K, const double* Zout,
                                        const double* model, const double* Zref_dot, const double* K_dot, const double* x0_dot,
                                        const double* model_dot, double* Zout_dot);
int qln_tracking_rollout_model_vjp_host(qln_handle* h, const double* Zref, const double* K, const double* Zout,
                                        const double* model, const double* Zbar, double* Zref_bar, double* K_bar, double* x0_bar,
                                        double* model_bar);
/* The closed-loop roll-out with GUARD-TRIGGERED touchdown: contact begins when the free foot reaches the ground, not at a
 * knot index.  qln_tracking_rollout switches mode at the handle's k_trans whatever the state is, which is the NLP's
 * schedule; a drop that is not the planned one (higher, or with another foot mass) lands earlier or later than that, and
 * this call simulates it.  Zref, K, x0, model and Zout mean what they mean for qln_tracking_rollout_model: K == NULL is the
 * open-loop roll-out, x0 == NULL the handle's x0, model == NULL the handle's model for every problem; Zout must not overlap
 * Zref, and entries from n_nlp to z_stride are never written.  Knots are 0-based, k = 0..N-2.
 *   F_k = F_ref,k - K_k (x_k - x_ref,k), h_k = h_ref,k, the product formed as in qln_tracking_rollout.  Gains and reference
 *   stay indexed by knot, that is by time: they are the controller under test.
 * Read from the handle: N, each problem's init_mode, x0 and the model.  k_trans is NOT read.
 * Mode schedule: problem b starts in mode init_mode (one foot stands, the other is free); after touchdown it is in mode 3
 * for the rest of the roll-out.  There is no lift-off.
 * Guard, at a knot k that starts in a single-stance mode: y, v are the free foot's height and vertical velocity (mode 1:
 * x[6], x[13]; mode 2: x[4], x[11]), a = -F_y / mf + g with that foot's applied vertical force (mode 1: u[3]; mode 2: u[1]),
 * h = u[4].  With the forces held the height over the step is y + v t + a t^2 / 2 exactly, and the first tau in [0, h] at which
 * it is <= 0 is
 *     if (y <= 0)                         tau = 0
 *     else  disc = v*v - 2*a*y;  den = -v + sqrt(disc)
 *           if (disc >= 0 && den > 0) { tau = 2*y/den;  touchdown iff tau <= h }   else none
 *   The comparisons are written so that a NaN never triggers a touchdown.  The one expression is the smaller positive root
 *   for every sign of a and v, in its cancellation-free form (a == 0: -y/v).  sqrt and the division are correctly rounded.
 * The touchdown step is composite, the applied forces held: (1) an RK4 step of length tau in the flight mode, (2) the jump
 * map of the knot-scheduled roll-out (y1 = y2 = 0, all four foot velocities 0), (3) an RK4 step of length h - tau in mode 3,
 * (4) the clock advances by h: x_{k+1}[14] = x_k[14] + h.  Zout's x_{k+1} is the state after the whole composite step, Zout's
 * u_k is (F_k, h_k) as always.  A step without touchdown is bit for bit the knot-scheduled roll-out's step of that mode.
 * event (may be NULL: not written; Zout is the same), QLN_TOUCHDOWN_INFO_STRIDE doubles per problem:
 *   0     the 0-based knot k whose step contains the touchdown, an exact integer; -1 if there is none, and then entries
 *         1-5 are 0
 *   1     tau
 *   2     the clock at touchdown, x_k[14] + tau
 *   3     the free foot's x at touchdown
 *   4, 5  its velocity (vx, vy) just before the jump map
 *   6     the smallest applied vertical force over all knots and over the feet standing at the knot's start (fmin from
 *         +inf); negative: the ground pulled
 *   7     0
 * Two consequences.  A guarded Zout is NOT a trajectory of the handle's knot schedule: its derivatives are
 * qln_tracking_rollout_guarded_jvp / _vjp below, gains along it are qln_tracking_lqr_guarded's and covariances along it
 * qln_tracking_covariance_guarded's, all of which take the event record; qln_tracking_rollout_jvp / _vjp, their _model_
 * forms, qln_tracking_lqr and qln_tracking_covariance "at the trajectory Zout" do not apply to it, and its dynamics rows under
 * qln_eval_constraint are non-zero at the touchdown knot.  And under sampled feedback the closed-loop map is DISCONTINUOUS in the initial state
 * where the touchdown moves from the end of one step to the start of the next: the control of that knot is computed from
 * the pre-impact state in one case and from the post-impact state in the other.  Open loop (K == NULL) it is continuous.
 * Derivatives through the event, the saltation term included, are qln_tracking_rollout_guarded_jvp / _vjp: they read the knot
 * and tau from the record.
 * Device pointers, stream-ordered; needs no cost table.  The device form does not validate model; the host form refuses a
 * non-finite entry and mb, mf or lb <= 0.  A NULL h, Zref or Zout, or an overlap, is QLN_ERR_INVALID_ARGUMENT. */
#define QLN_TOUCHDOWN_INFO_STRIDE 8
int qln_tracking_rollout_guarded(qln_handle* h, const double* Zref, const double* K, const double* x0,
                                 const double* model /* [B][QLN_MODEL_NP] (g, mb, mf, lb) or NULL = the handle's */,
                                 double* Zout, double* event /* [B][QLN_TOUCHDOWN_INFO_STRIDE] or NULL */);
/* the same as a host form (see "Host forms" above; Zout is in-out) */
int qln_tracking_rollout_guarded_host(qln_handle* h, const double* Zref, const double* K, const double* x0, const double* model,
                                      double* Zout, double* event);
/* Forward and reverse sweeps THROUGH the guard-triggered touchdown: the derivative of qln_tracking_rollout_guarded at the
 * trajectory Zout holds, at FIXED touchdown knot.  Knots are 0-based, k = 0..N-2.  The arguments are those of
 * qln_tracking_rollout_model_jvp / _vjp plus
 *   event: device, [B][QLN_TOUCHDOWN_INFO_STRIDE], the record the guarded roll-out wrote.  Required.  Only entries 0 (the knot
 *          k*) and 1 (tau) are read; k* < 0 or beyond N-2 means no touchdown.
 * k_trans is not read.  As with the other sweeps nothing is re-run, and nothing checks that Zout / event are the roll-out of
 * the inputs.  m is the problem's init_mode, theta_b its model (model == NULL: the handle's).
 * Block per knot, at Zout's (x_k, u_k) and theta_b:
 *   k < k*, or no touchdown:  [A_k B_k G_k] of mode m, no jump;
 *   k > k*:                    the same in mode 3;
 *   k == k*: the composite step.  The forces F = u_k[0:4] are held and h = u_k[4]; y, v, F_y are the free foot's, selected as
 *     by the guard above, a = -F_y / mf + g.
 *       x- = RK4_m(x_k, F; tau), recomputed as the forward call forms it; w = x-[iv], the foot's vertical velocity before the
 *            jump map;
 *       dtau = -(dy + tau dv + (tau^2 / 2) da) / w,   da = -dF_y / mf + (F_y / mf^2) dmf + dg;
 *              dtau = 0 where the guard's first branch was taken (x_k[iy] <= 0, tau = 0);
 *       dx- = A_m dx_k + B_m dF + b_m dtau + G_m dtheta    (mode m's block at step length tau; b is the block's h column)
 *       dx+ = dx- with entries 4, 6, 10-13 set to zero      (the jump map)
 *       dx_{k+1} = A_3 dx+ + B_3 dF + b_3 (dh - dtau) + G_3 dtheta    (the mode-3 block at (x+, F, h - tau))
 *     The clock rows of the two legs add up to dx_k[14] + dh by themselves.
 * Forward sweep (qln_tracking_rollout_guarded_jvp): qln_tracking_rollout_model_jvp's recursion on these blocks; tangents,
 *   NULL rules, Zout_dot and overlap rules are the same.  One optional output more,
 *   event_dot: [B][QLN_TOUCHDOWN_INFO_STRIDE] or NULL (not written).  Entry 1 is dtau, entry 2 is dx_{k*}[14] + dtau, the
 *              tangent of the touchdown clock; every other entry is 0, and the whole record is 0 without a touchdown.
 * Reverse sweep (qln_tracking_rollout_guarded_vjp): qln_tracking_rollout_model_vjp's recursion; at k* the exact transpose of
 *   the sequence above.  Through the mode-3 leg lam+ = A_3' lam, ubar_F += B_3' lam, hbar += b_3' lam, taubar = -b_3' lam,
 *   model_bar += G_3' lam; through the jump map the six entries of lam+ are zeroed; through the flight leg the same with
 *   taubar += b_m' lam-.  taubar is then distributed by dtau's coefficients onto lam_k[iy] and lam_k[iv], onto the free foot's
 *   ubar_F_y -- before that ubar enters K_k' ubar, K_bar and Zref_bar -- and onto model_bar[g] and model_bar[mf].  It is the
 *   exact adjoint of the forward sweep on (Zref, K, x0, model) -> Zout:
 *   <Zbar, Zout_dot> = <Zref_bar, Zref_dot> + <K_bar, K_dot> + <x0_bar, x0_dot> + <model_bar, model_dot>.
 *   event_dot has no cotangent.
 * Limits.  The result is the derivative at fixed touchdown knot: where the knot changes the closed-loop map is discontinuous
 * (above) and no derivative exists.  It scales with 1 / |w|: a grazing touchdown has no useful derivative.
 * Errors: a NULL event is QLN_ERR_INVALID_ARGUMENT; the other NULL combinations are the _model_ sweeps'.  The device forms
 * do not validate event; the host forms refuse a knot that is not an integer in [-1, N-2] and a tau that is not finite or is
 * negative.  event and event_dot take part in the overlap rule.  Device pointers, stream-ordered; needs no cost table. */
int qln_tracking_rollout_guarded_jvp(qln_handle* h, const double* Zref, const double* K, const double* Zout, const double* model,
                                     const double* event, const double* Zref_dot, const double* K_dot, const double* x0_dot,
                                     const double* model_dot, double* Zout_dot, double* event_dot);
int qln_tracking_rollout_guarded_vjp(qln_handle* h, const double* Zref, const double* K, const double* Zout, const double* model,
                                     const double* event, const double* Zbar, double* Zref_bar, double* K_bar, double* x0_bar,
                                     double* model_bar);
/* the same as host forms (see "Host forms" above; Zout_dot and Zref_bar are in-out as in the _model_ forms) */
int qln_tracking_rollout_guarded_jvp_host(qln_handle* h, const double* Zref, const double* K, const double* Zout,
                                          const double* model, const double* event, const double* Zref_dot, const double* K_dot,
                                          const double* x0_dot, const double* model_dot, double* Zout_dot, double* event_dot);
int qln_tracking_rollout_guarded_vjp_host(qln_handle* h, const double* Zref, const double* K, const double* Zout,
                                          const double* model, const double* event, const double* Zbar, double* Zref_bar,
                                          double* K_bar, double* x0_bar, double* model_bar);
/* TVLQR gains THROUGH the guard-triggered touchdown: qln_tracking_lqr's recursion, weights, outputs, packing and exact symmetry
 * of P, on the blocks of qln_tracking_rollout_guarded_jvp at Ztraj's (x_k, u_k) -- the saltation-matrix TVLQR of a hybrid system.
 *   Ztraj: device, layout of Z: the trajectory to linearise along, as a rule the Zout of a guarded roll-out of the plan;
 *   model: device, [B][QLN_MODEL_NP] or NULL = the handle's;
 *   event: device, [B][QLN_TOUCHDOWN_INFO_STRIDE], the record that roll-out wrote.  Required.  Only entries 0 (the knot k*) and
 *          1 (tau) are read; k* < 0 or beyond N-2 means no touchdown.  k_trans is not read, and nothing is re-run.
 * [A_k B_k] is mode init_mode's block for k < k* (or without a touchdown) and mode 3's for k > k*, neither with a jump.  At
 * k* it is the composite step's, with dh = 0 and in the notation of the sweeps above (t_x: dtau's coefficients -1/w at iy and
 * -tau/w at iv; t_F: (tau^2 / 2) / (mf w) at the free foot's F_y; all zero where tau = 0 came from the guard's first branch):
 *   A* v + B* f = A_3 J (A_m v + B_m f + b_m s) + B_3 f - b_3 s,   s = t_x . v + t_F . f
 * Usage: roll the plan out guarded for (Zg, event), design gains along Zg with event, track perturbed drops against
 * Zref = Zg with those gains, guarded.  For every drop that lands in the same knot they are the first-order optimal gains; a
 * drop that lands in another knot is outside what a derivative at fixed knot says.
 * A batch without a touchdown and with model == NULL (or the handle's model passed) gives qln_tracking_lqr's bits for a handle
 * with k_trans = N + 1.  Errors: a NULL h, Ztraj, K or event, weights as for qln_tracking_lqr, an output that overlaps an
 * input or the other output: QLN_ERR_INVALID_ARGUMENT.  The device form does not validate model or event; the host form does,
 * as the guarded sweeps' host forms do.  Device pointers, stream-ordered; needs no cost table. */
int qln_tracking_lqr_guarded(qln_handle* h, const double* Ztraj, const double* model /* [B][QLN_MODEL_NP] or NULL */,
                             const double* event /* [B][QLN_TOUCHDOWN_INFO_STRIDE], required */, const double* Qdiag,
                             const double* Rdiag, const double* Qfdiag, double* K, double* P /* or NULL */);
/* the same as a host form (see "Host forms" above; the weights are host arrays in both) */
int qln_tracking_lqr_guarded_host(qln_handle* h, const double* Ztraj, const double* model, const double* event,
                                  const double* Qdiag, const double* Rdiag, const double* Qfdiag, double* K, double* P);
/* CONTACT-AWARE FORCE LIMITS in the closed-loop roll-out, its sweeps and gains: a foot can only push, and a leg has a force
 * limit.  The calls above apply F_k = F_ref,k - K_k (x_k - x_ref,k) as computed, whatever its sign and size; these clamp it.
 * All of it is opt-in: every call above keeps its bits.  Knots are 0-based, k = 0..N-2.
 * Limits.  lim: a HOST array of QLN_FORCE_LIMITS_N = 8 doubles, passed by value in the kernel arguments as Qdiag is:
 *     {free_x_lo, free_x_hi, free_y_lo, free_y_hi, stand_x_lo, stand_x_hi, stand_y_lo, stand_y_hi}
 *   A foot is "standing" or "free" by the contact mode at the START of knot k: in mode 1 foot 1 stands and foot 2 is free, in
 *   mode 2 the reverse, in mode 3 both stand.  Knot-scheduled calls (guarded == 0) take the mode from the handle's schedule, the
 *   mode qln_tracking_rollout's step uses for that knot (the jump knot is still in init_mode).  Guarded calls take the
 *   problem's current mode; in the touchdown knot the landing foot counts as free for the whole step, because the forces are
 *   held -- the convention of the event record's entry 6.  +-inf is allowed and means no limit on that side; a NaN, or lo > hi,
 *   is QLN_ERR_INVALID_ARGUMENT.  The limits are the same for every problem.
 * Clamp.  For channel m (F1x, F1y, F2x, F2y) of F = F_ref,k - K_k e_k, formed exactly as in qln_tracking_rollout (with
 *   K == NULL the reference's forces are clamped), and {lo, hi} the channel's pair for its foot's contact state:
 *     s_m = F < lo ? 1 : (F > hi ? 2 : 0),     F_applied = s_m == 1 ? lo : s_m == 2 ? hi : F
 *   A NaN fails both comparisons and passes through with s_m = 0; F == lo exactly is s_m = 0.  h_k is never clamped.  Zout's
 *   u_k, the guard's a, the step and the event record's entry 6 all use the applied forces (so entry 6 >= stand_y_lo).  With
 *   all eight limits infinite the result is bit for bit qln_tracking_rollout_model's (guarded == 0) or _guarded's.
 * Saturation record.  sat: [B][N-1] doubles; knot k holds the exact integer sum_m s_m 4^m (0..170).  An output of the roll-out
 *   (may be NULL: not written, Zout is the same); a REQUIRED input of the sweeps and of the gain design, as event is of the
 *   guarded ones.  It takes part in the overlap rules.  The device forms do not validate it (a value that is no code in
 *   [0, 170] masks nothing); the host forms refuse a value that is not an integer code with every s_m in {0, 1, 2}.
 * qln_tracking_rollout_limited: guarded == 0 is qln_tracking_rollout_model on the handle's schedule, and event must be NULL;
 *   guarded != 0 is qln_tracking_rollout_guarded (event may be NULL).  model == NULL is the handle's model.  The NULL and
 *   overlap rules are those forms', plus sat.
 * Derivative at FIXED ACTIVE SET (qln_tracking_rollout_limited_jvp / _vjp).  A channel with s_m != 0 is a constant, so its
 *   dF_k[m] is zero.  event == NULL selects the blocks of qln_tracking_rollout_model_jvp / _vjp (then event_dot must be NULL),
 *   a non-NULL event those of qln_tracking_rollout_guarded_jvp / _vjp; the other arguments, NULL rules and outputs are theirs.
 *   Forward:  dF_k = mask_k .* (Fref_dot_k - K_k (dx_k - xref_dot_k) - Kdot_k e_k), mask_k[m] = (s_m == 0); everything
 *     downstream, dtau's dF_y at the touchdown knot and Zout_dot's u_k included, uses the masked dF_k.
 *   Reverse:  ubar_k[0:4] is masked after the touchdown knot's taubar has been distributed onto it and before it enters
 *     K_k' ubar, K_bar and Zref_bar: the saturated channels' F_ref_bar and rows of K_bar are exact zeros, and Zbar[u_k][m] of a
 *     saturated channel goes nowhere.
 *   The h column is untouched.  The two sweeps are exact adjoints, with the duality identity of the guarded sweeps.
 *   Limits of the statement: where the active set changes the closed-loop map has a kink and the result is a one-sided
 *   derivative at best (of the side the record describes); the fixed touchdown knot carries the caveat it always did.
 * Gains at fixed active set (qln_tracking_lqr_limited).  The recursion, weights, packing and exact symmetry of P of
 *   qln_tracking_lqr (event == NULL; model must then be NULL, that design has no plant model) or qln_tracking_lqr_guarded
 *   (event given), with the columns of B_k of the saturated channels set to zero.  At the touchdown knot the mask sits at the
 *   composite operator's force input (f in A* v + B* f), so the rank-one dtau term loses the channel too.  The saturated rows
 *   of K_k are then exact 0.0 (Quu decouples to R_m on them), and P_k is the cost-to-go of feedback on the free channels only.
 *   With sat all zero it is the existing call bit for bit.
 * Covariance needs nothing new: with those zero rows of K, A_k - B_k K_k is already the closed loop of the clamped system, so
 *   qln_tracking_covariance / _guarded apply as they are.  Gains designed elsewhere get the zero rows from the bindings'
 *   mask_gains(K, sat).
 * Errors: a NaN limit or lo > hi, a NULL lim, event with guarded == 0, a NULL sat in a sweep or the design, model without event
 *   in the design, event_dot without event: QLN_ERR_INVALID_ARGUMENT, besides those of the forms they extend.  Device pointers,
 *   stream-ordered; needs no cost table. */
#define QLN_FORCE_LIMITS_N 8
int qln_tracking_rollout_limited(qln_handle* h, const double* Zref, const double* K, const double* x0, const double* model,
                                 const double* lim /* host, [QLN_FORCE_LIMITS_N] */, int32_t guarded, double* Zout,
                                 double* event /* [B][QLN_TOUCHDOWN_INFO_STRIDE] or NULL; NULL if guarded == 0 */,
                                 double* sat /* [B][N-1] or NULL */);
int qln_tracking_rollout_limited_jvp(qln_handle* h, const double* Zref, const double* K, const double* Zout, const double* model,
                                     const double* event /* or NULL: the knot schedule */, const double* sat /* required */,
                                     const double* Zref_dot, const double* K_dot, const double* x0_dot, const double* model_dot,
                                     double* Zout_dot, double* event_dot);
int qln_tracking_rollout_limited_vjp(qln_handle* h, const double* Zref, const double* K, const double* Zout, const double* model,
                                     const double* event /* or NULL: the knot schedule */, const double* sat /* required */,
                                     const double* Zbar, double* Zref_bar, double* K_bar, double* x0_bar, double* model_bar);
int qln_tracking_lqr_limited(qln_handle* h, const double* Ztraj, const double* model, const double* event /* or NULL */,
                             const double* sat /* required */, const double* Qdiag, const double* Rdiag, const double* Qfdiag,
                             double* K, double* P /* or NULL */);
/* the same as host forms (see "Host forms" above; Zout, Zout_dot and Zref_bar are in-out as in the forms they extend; lim and
 * the weights are host arrays in both) */
int qln_tracking_rollout_limited_host(qln_handle* h, const double* Zref, const double* K, const double* x0, const double* model,
                                      const double* lim, int32_t guarded, double* Zout, double* event, double* sat);
int qln_tracking_rollout_limited_jvp_host(qln_handle* h, const double* Zref, const double* K, const double* Zout,
                                          const double* model, const double* event, const double* sat, const double* Zref_dot,
                                          const double* K_dot, const double* x0_dot, const double* model_dot, double* Zout_dot,
                                          double* event_dot);
int qln_tracking_rollout_limited_vjp_host(qln_handle* h, const double* Zref, const double* K, const double* Zout,
                                          const double* model, const double* event, const double* sat, const double* Zbar,
                                          double* Zref_bar, double* K_bar, double* x0_bar, double* model_bar);
int qln_tracking_lqr_limited_host(qln_handle* h, const double* Ztraj, const double* model, const double* event, const double* sat,
                                  const double* Qdiag, const double* Rdiag, const double* Qfdiag, double* K, double* P);
/* Covariance propagation through the closed-loop roll-out: the linear-Gaussian forward sweep along the trajectory Zout
 * holds.  Knots are 0-based, k = 0..N-2, as in qln_tracking_rollout_vjp.
 *   A_k (15x15), B_k (15x4) = d Phi_k / d(x_k, F_k) at Zout's (x_k, u_k): exactly the blocks qln_tracking_rollout_vjp uses --
 *   the evaluator's closed-form step block, except that at the jump knot row 14 is the jump map's (1 at x[14]).  The h
 *   column is not used: step lengths are not perturbed.  Nothing checks that Zout is a roll-out; for the nominal case pass
 *   the reference itself.
 *   Sigma_0 = Sigma0,  Sigma_{k+1} = Acl_k Sigma_k Acl_k' + diag(W),  Acl_k = A_k - B_k K_k  (K == NULL: Acl_k = A_k, open loop)
 *   W is added after every step, the jump knot included.  Every Sigma_k is formed on its lower triangle and is exactly
 *   symmetric; positive semi-definiteness is not enforced.
 * Inputs:
 *   Sigma0: device, [sigma0_batch][120], packed lower triangle, row i >= j at i(i+1)/2 + j (the layout of P);
 *           sigma0_batch is 1 (shared by every problem) or B, else QLN_ERR_INVALID_ARGUMENT (as cost_batch).
 *   Wdiag:  a HOST array of 15 entries, passed by value in the kernel arguments; every entry finite and >= 0, else
 *           QLN_ERR_INVALID_ARGUMENT; NULL means zeros.
 *   K:      device, [B][N-1][4][15], or NULL.
 * Outputs (at least one non-NULL, else QLN_ERR_INVALID_ARGUMENT; overwritten, not accumulated; which of them is asked for
 * does not change the other's bits; none may overlap an input or the other):
 *   Sigma: [B][N][120] packed.
 *   marg:  [B][N][QLN_TRACK_MARG_STRIDE], per knot
 *     [0]    the variance of the clearance row, a' Sigma_k a with a = e_yb + c'(theta_k) e_theta, c' the derivative entry
 *            jac_c! writes (quirk Q3's branch at theta == 0);
 *     [1..4] the variances of the four applied forces, diag(K_k Sigma_k K_k'): exact zeros when K == NULL and at knot N-1;
 *     [5],[6] Sigma_k[4][4] and Sigma_k[6][6], the two foot heights;
 *     [7]    trace Sigma_k.
 * Every N >= 2, every k_trans in [1, N+1] and both init_modes, as the other tracking calls.  Device pointers,
 * stream-ordered; needs no cost table. */
#define QLN_TRACK_MARG_STRIDE 8
int qln_tracking_covariance(qln_handle* h, const double* Zout, const double* K, const double* Sigma0, int32_t sigma0_batch,
                            const double* Wdiag, double* Sigma, double* marg);
/* the same as a host form (see "Host forms" above; Wdiag is a host array in both; nothing is in-out) */
int qln_tracking_covariance_host(qln_handle* h, const double* Zout, const double* K, const double* Sigma0,
                                 int32_t sigma0_batch, const double* Wdiag, double* Sigma, double* marg);
/* Covariance propagation THROUGH the guard-triggered touchdown: qln_tracking_covariance's recursion, inputs, outputs and
 * marginals on the blocks of qln_tracking_lqr_guarded at a guarded roll-out's (Zout, event), at FIXED touchdown knot:
 *   Sigma_{k+1} = Acl_k Sigma_k Acl_k' + diag(W),  Acl_k = A_k - B_k K_k,  Acl_{k*} = A* - B* K_{k*}.
 * model and event as for qln_tracking_lqr_guarded (event required).  One optional output more,
 *   event_var: [B][2] or NULL (not written).  [0] is the variance of tau, c' Sigma_{k*} c with c = t_x - K_{k*}' t_F (c = t_x
 *              when K == NULL); [1] is the variance of the touchdown clock x_{k*}[14] + tau, the same with c + e_14.  Both are
 *              0 without a touchdown, and where tau = 0 came from the guard's first branch [0] is 0.
 * At least one of Sigma, marg and event_var must be non-NULL; which of them is asked for does not change the others' bits,
 * and none may overlap an input or another output.  A batch without a touchdown and with model == NULL (or the handle's model
 * passed) gives qln_tracking_covariance's bits for a handle with k_trans = N + 1.  First order, as the sweeps: the variance of
 * a touchdown that can move to another knot is not described.  The device form does not validate model or event; the host
 * form does.  Device pointers, stream-ordered; needs no cost table. */
int qln_tracking_covariance_guarded(qln_handle* h, const double* Zout, const double* K, const double* model, const double* event,
                                    const double* Sigma0, int32_t sigma0_batch, const double* Wdiag, double* Sigma, double* marg,
                                    double* event_var /* [B][2] or NULL */);
int qln_tracking_covariance_guarded_host(qln_handle* h, const double* Zout, const double* K, const double* model,
                                         const double* event, const double* Sigma0, int32_t sigma0_batch, const double* Wdiag,
                                         double* Sigma, double* marg, double* event_var);
/* Kalman filter gains and the LQG covariance along a tracked landing: qln_tracking_covariance with the controller fed an
 * ESTIMATE, F_k = F_ref,k - K_k xhat_k|k, built from ny noisy measurements per knot, y_k = H dx_k + v_k, k = 0..N-1.
 *   A_k, B_k: exactly the blocks of qln_tracking_covariance at Zout's (x_k, u_k) -- the evaluator's closed-form block, row 14
 *   restored at the jump knot, no h column.
 *   P^-_0 = Sigma0,  M^-_0 = 0, and for k = 0 .. N-1
 *     S_k   = H P^-_k H' + diag(V)                    (ny x ny, solved by L D L' without pivoting)
 *     L_k   = P^-_k H' S_k^-1                         (15 x ny, the filter gain: xhat+ = xhat- + L_k (y_k - H xhat-))
 *     P^+_k = (I - L_k H) P^-_k (I - L_k H)' + L_k diag(V) L_k'          (Joseph form; the error's covariance)
 *     M_k   = M^-_k + (P^-_k - P^+_k)                 (the covariance of the estimate xhat_k|k)
 *     X_k   = M_k + P^+_k                             (the covariance of the true state; estimate and error are orthogonal)
 *     P^-_{k+1} = A_k P^+_k A_k' + diag(W)            (open loop: the error does not see the gains)
 *     M^-_{k+1} = Acl_k M_k Acl_k',  Acl_k = A_k - B_k K_k
 *   Every matrix is formed on its lower triangle and is exactly symmetric; positive semi-definiteness is not enforced.
 * Inputs:
 *   H:      device, [ny][15] row-major, shared by every problem and every knot; 1 <= ny <= QLN_TRACK_NY_MAX.  The kernel always
 *           works on QLN_TRACK_NY_MAX rows: the rows behind ny are zero rows with variance 1, which changes no value, so a
 *           call gives the bits of the same call with those rows written out.
 *   Vdiag:  a HOST array of ny measurement variances, every entry finite and > 0.
 *   Sigma0, sigma0_batch, Wdiag: as for qln_tracking_covariance.
 *   K:      device, [B][N-1][4][15], or NULL: the filter alone, which returns Lgain and Pest only (Sigma and marg must be
 *           NULL then).  Gains of qln_tracking_lqr_limited or masked ones are taken as they are: their zero rows already make
 *           A - B K the clamped loop.
 * Outputs (each optional, at least one non-NULL; overwritten; which of them is asked for does not change the others' bits, and
 * the filter alone gives the bits Lgain and Pest have with K; none may overlap an input or another output):
 *   Lgain: [B][N][15][ny], the gains L_k.
 *   Pest:  [B][N][120] packed, P^+_k.
 *   Sigma: [B][N][120] packed, X_k.
 *   marg:  [B][N][QLN_TRACK_MARG_STRIDE] on X_k: [0] the clearance row's variance, [5], [6] X_k[4][4] and X_k[6][6], [7] the
 *          trace; [1..4] the variances of the four APPLIED forces, diag(K_k M_k K_k') -- the forces feed back the estimate --
 *          exact zeros at knot N-1.
 * Refused with QLN_ERR_INVALID_ARGUMENT: ny outside 1..QLN_TRACK_NY_MAX, a V entry not finite or not > 0, a W entry not
 * finite or negative, H == NULL, sigma0_batch not 1 or B, no output, Sigma or marg (or event_var) with K == NULL, overlaps.
 * The device forms do not validate device data; the host forms also refuse a non-finite H.  Device pointers, stream-ordered;
 * needs no cost table. */
#define QLN_TRACK_NY_MAX 8
int qln_tracking_kalman(qln_handle* h, const double* Zout, const double* K /* or NULL */, const double* H, int32_t ny,
                        const double* Vdiag, const double* Sigma0, int32_t sigma0_batch, const double* Wdiag /* or NULL */,
                        double* Lgain, double* Pest, double* Sigma, double* marg);
int qln_tracking_kalman_host(qln_handle* h, const double* Zout, const double* K, const double* H, int32_t ny, const double* Vdiag,
                             const double* Sigma0, int32_t sigma0_batch, const double* Wdiag, double* Lgain, double* Pest,
                             double* Sigma, double* marg);
/* The same THROUGH the guard-triggered touchdown, on the blocks of qln_tracking_covariance_guarded at a guarded roll-out's
 * (Zout, event), at fixed touchdown knot k*: the knot's two applications are the composite operator's, A* for P and
 * A* - B* K_{k*} for M.  model and event as for qln_tracking_covariance_guarded (event required).  One optional output more,
 *   event_var: [B][2] or NULL (not written; needs K).  With t_x, t_F the coefficients of d tau and c = t_x - K_{k*}' t_F,
 *              [0] = c' M_{k*} c + t_x' P^+_{k*} t_x, the variance of tau; [1] the same with c + e_14 and t_x + e_14, the
 *              variance of the touchdown clock.  The zero conventions are qln_tracking_covariance_guarded's.
 * A batch without a touchdown and with model == NULL (or the handle's model passed) gives qln_tracking_kalman's bits for a
 * handle with k_trans = N + 1.  The device form does not validate model or event; the host form does. */
int qln_tracking_kalman_guarded(qln_handle* h, const double* Zout, const double* K, const double* model, const double* event,
                                const double* H, int32_t ny, const double* Vdiag, const double* Sigma0, int32_t sigma0_batch,
                                const double* Wdiag, double* Lgain, double* Pest, double* Sigma, double* marg,
                                double* event_var /* [B][2] or NULL */);
int qln_tracking_kalman_guarded_host(qln_handle* h, const double* Zout, const double* K, const double* model, const double* event,
                                     const double* H, int32_t ny, const double* Vdiag, const double* Sigma0, int32_t sigma0_batch,
                                     const double* Wdiag, double* Lgain, double* Pest, double* Sigma, double* marg,
                                     double* event_var);
/* The ESTIMATE-FEEDBACK roll-out: the nonlinear hybrid plant and the estimator rolled out together in one launch, the loop
 * qln_tracking_kalman designs and predicts.  The roll-outs above feed back the true state; this one feeds back xhat_k|k, built
 * from ny noisy measurements per knot with the filter gains L_k.  The library draws nothing: the measurement and process noise
 * are samples the caller supplies, so the call is deterministic.  Knots are 0-based.
 * Zref, K, x0, model, Zout and event mean what they mean for qln_tracking_rollout_model / _guarded.  x_0 = x0[b] (NULL: the
 * handle's x0), xhat^-_0 = xhat0[b] (NULL: x_ref,0 -- the estimate starts on the nominal, the design's M^-_0 = 0), and for
 * k = 0 .. N-1
 *     y_k      = H (x_k - x_ref,k) + v_k                     v_k = vnoise[b][k]  (NULL: zeros)
 *     innov_k  = y_k - H (xhat^-_k - x_ref,k)
 *     xhat_k   = xhat^-_k + L_k innov_k                      L_k = Lgain[b][k], [15][ny]
 *     if k == N-1: stop
 *     F_k      = F_ref,k - K_k (xhat_k - x_ref,k),  h_k = h_ref,k          (K == NULL: F_k = F_ref,k)
 *     x_{k+1}  = Phi_k(x_k, u_k; model[b]) + w_k             w_k = wnoise[b][k]  (NULL: none)
 *     xhat^-_{k+1} = Phi_k(xhat_k, u_k; the handle's model)
 *   Every product is formed as qln_tracking_rollout forms K dx: the first product, then fused multiply-adds in index order;
 *   L_k innov_k is accumulated onto xhat^-_k column by column.
 * Knot-scheduled form (qln_tracking_rollout_estimated): Phi_k is the step of qln_tracking_rollout_model, for the plant and for
 *   the estimator alike.
 * Guarded form (qln_tracking_rollout_estimated_guarded): Phi_k is the guarded step of qln_tracking_rollout_guarded, taken twice.
 *   The plant and the estimator each carry their own contact mode, their own guard decision and tau and their own touchdown
 *   record: the estimator lands when its ESTIMATED foot reaches the ground, and the handle's k_trans is not read.  This is the
 *   loop the saltation term of qln_tracking_kalman_guarded describes; a contact switch shared with the plant would be a
 *   different filter.
 * Noise: w_k is added as given, after the whole (composite) step, clock row included.
 * Estimator model: always the handle's -- the design model does not follow the plant, as for qln_tracking_lqr.
 * Inputs (device pointers):
 *   Lgain:  [B][N][15][ny], the layout qln_tracking_kalman writes.  Required.
 *   H:      [ny][15] row-major, shared by every problem and knot; 1 <= ny <= QLN_TRACK_NY_MAX.  Required.  A call with ny rows
 *           gives, in Zout and Xhat, the bits of the call with QLN_TRACK_NY_MAX rows whose further H rows and L columns are zero.
 *   vnoise: [B][N][ny] or NULL.   wnoise: [B][N-1][15] or NULL.   xhat0: [B][15] or NULL.
 * Outputs (overwritten; which optional ones are asked for does not change the others' bits; none may overlap an input or
 * another output):
 *   Zout:      required; the TRUE states and the applied controls in the layout of Z; entries past n_nlp are never written.
 *   Xhat:      [B][N][15] or NULL; xhat_k|k.
 *   innov:     [B][N][ny] or NULL.
 *   event:     guarded only, [B][QLN_TOUCHDOWN_INFO_STRIDE] or NULL: the plant's record.
 *   event_hat: guarded only, the same shape or NULL: the estimator's record, its entry 6 taken over the same applied forces by the
 *              estimator's own standing feet.
 * Reductions: with Lgain = 0, xhat0 == NULL and Zref a qln_tracking_rollout_model / _guarded roll-out (K == NULL) under the
 * handle's model, the estimate stays on Zref and Zout is bit for bit qln_tracking_rollout_model(Zref, NULL, x0, model),
 * respectively _guarded and its event record, whatever K is.
 * Refused with QLN_ERR_INVALID_ARGUMENT: a NULL h, Zref, Zout, Lgain or H; ny outside 1..QLN_TRACK_NY_MAX; an overlap.  The
 * device forms do not validate device data; the host forms also refuse a non-finite H, and a model as
 * qln_tracking_rollout_guarded_host does.  Force limits in this loop are qln_tracking_rollout_estimated_limited
 * below; these two calls apply the forces as computed.  Their derivatives are qln_tracking_rollout_estimated_jvp / _vjp below.
 * Device pointers, stream-ordered; needs no cost table. */
int qln_tracking_rollout_estimated(qln_handle* h, const double* Zref, const double* K /* or NULL */, const double* Lgain,
                                   const double* H, int32_t ny, const double* vnoise, const double* wnoise, const double* x0,
                                   const double* xhat0, const double* model, double* Zout, double* Xhat, double* innov);
int qln_tracking_rollout_estimated_guarded(qln_handle* h, const double* Zref, const double* K, const double* Lgain, const double* H,
                                           int32_t ny, const double* vnoise, const double* wnoise, const double* x0,
                                           const double* xhat0, const double* model, double* Zout, double* Xhat, double* innov,
                                           double* event, double* event_hat);
/* the same as host forms (see "Host forms" above; Zout is in-out) */
int qln_tracking_rollout_estimated_host(qln_handle* h, const double* Zref, const double* K, const double* Lgain, const double* H,
                                        int32_t ny, const double* vnoise, const double* wnoise, const double* x0,
                                        const double* xhat0, const double* model, double* Zout, double* Xhat, double* innov);
int qln_tracking_rollout_estimated_guarded_host(qln_handle* h, const double* Zref, const double* K, const double* Lgain,
                                                const double* H, int32_t ny, const double* vnoise, const double* wnoise,
                                                const double* x0, const double* xhat0, const double* model, double* Zout,
                                                double* Xhat, double* innov, double* event, double* event_hat);
/* Forward and reverse sweeps THROUGH the estimate-feedback roll-out: the derivative of qln_tracking_rollout_estimated / _guarded
 * with respect to (Zref, K, Lgain, x0, xhat0, model) at the trajectory (Zout, Xhat, innov) it produced.  vnoise, wnoise and H are
 * HELD FIXED -- the pathwise derivative at fixed noise samples -- and get no tangent and no cotangent.  Knots are 0-based.
 * Inputs of both sweeps (device pointers):
 *   Zref, K (or NULL), Lgain, H, ny, model (or NULL): the roll-out's.
 *   Zout, Xhat: the trajectory it wrote.  Both required.
 *   innov:      the innovations it wrote.  Required exactly when a tangent or cotangent of Lgain is asked for (Lgain_dot,
 *               Lgain_bar); otherwise it may be NULL and is not read.
 *   event, event_hat (guarded forms): the plant's and the estimator's records.  Both required.  Only entries 0 (the knot) and 1
 *               (tau) are read, as in qln_tracking_rollout_guarded_jvp.
 * Nothing is re-run, and nothing checks that the trajectory is the roll-out of the inputs.  The handle's k_trans is read by the
 * knot-scheduled forms only.
 * Blocks.  [A^p_k B^p_k G^p_k] is the plant's block at Zout's (x_k, u_k) and model[b]; [A^e_k B^e_k] is the estimator's at
 * (Xhat_k, Zout's u_k) and the handle's model, which has no tangent.  Knot-scheduled forms: both are the blocks of
 * qln_tracking_rollout_model_jvp.  Guarded forms: each chain takes the blocks of qln_tracking_rollout_guarded_jvp at its OWN
 * touchdown knot and tau -- the plant's from event, the estimator's from event_hat -- and the composite step with its own dtau at
 * that knot; the estimator's dtau depends on dxh and dF, not on dx, and the two chains may land in different knots.
 * Forward sweep (qln_tracking_rollout_estimated_jvp / _guarded_jvp).  Tangents Zref_dot, K_dot, Lgain_dot, x0_dot, xhat0_dot,
 * model_dot, each optional (NULL: zero, except xhat0_dot below; all NULL is refused; K_dot needs K):
 *     dx_0 = x0_dot,   dxm_0 = xhat0_dot       (xhat0_dot == NULL: dxm_0 = x_ref_dot,0, the forward call's xhat0 == NULL case)
 *     for k = 0 .. N-1:
 *       dinnov_k = H (dx_k - dxm_k)
 *       dxh_k    = dxm_k + L_k dinnov_k + Lgain_dot_k innov_k
 *       if k == N-1: stop
 *       dF_k = dF_ref,k - K_k (dxh_k - dx_ref,k) - K_dot_k (xhat_k - x_ref,k),   dh_k = dh_ref,k
 *       dx_{k+1}  = A^p_k dx_k  + B^p_k (dF_k, dh_k) + G^p_k model_dot
 *       dxm_{k+1} = A^e_k dxh_k + B^e_k (dF_k, dh_k)
 *   Outputs (overwritten; which optional ones are asked for does not change the others' bits):
 *     Zout_dot: required, layout of Z: dx_k and (dF_k, dh_k); entries past n_nlp are never written.
 *     Xhat_dot: [B][N][15] or NULL: dxh_k.     innov_dot: [B][N][ny] or NULL: dinnov_k.
 *     event_dot, event_hat_dot (guarded): [B][QLN_TOUCHDOWN_INFO_STRIDE] or NULL, with the entries
 *               qln_tracking_rollout_guarded_jvp defines, for the plant's and for the estimator's touchdown.
 * Reverse sweep (qln_tracking_rollout_estimated_vjp / _guarded_vjp).  Cotangents Zbar (required, layout of Z), Xhat_bar
 * [B][N][15] and innov_bar [B][N][ny] (NULL: zero).  The exact transpose of the recursion above, k = N-1 .. 0, with lam and lamm
 * the cotangents of dx and dxm (zero behind the last knot):
 *     k < N-1:  ubar = Zbar[u_k] + B^p' lam + B^e' lamm,   ax = A^p' lam,   model_bar += G^p' lam,
 *               xhb = Xhat_bar_k + A^e' lamm - K_k' ubar[0:4]                  (k == N-1: ax = 0, xhb = Xhat_bar_k)
 *     ib = innov_bar_k + L_k' xhb,    lam = Zbar[x_k] + ax + H' ib,    lamm = xhb - H' ib
 *   Outputs, each optional (K_bar needs K):
 *     Zref_bar:  layout of Z: K_k' ubar[0:4] in the x slots (zero at knot N-1), ubar in the u slots;
 *     K_bar:     -ubar[0:4] (xhat_k - x_ref,k)';      Lgain_bar: [B][N][15][ny], xhb innov_k';
 *     x0_bar:    lam after knot 0;                     model_bar: [B][QLN_MODEL_NP];
 *     xhat0_bar: [B][15], lamm after knot 0.  If it is NULL that cotangent is ADDED to Zref_bar's x_0 slot -- the forward call
 *                with xhat0 == NULL, whose xhat^-_0 is x_ref,0; if it is non-NULL it is written there and not added.
 *   In each of the two modes
 *     <Zbar, Zout_dot> + <Xhat_bar, Xhat_dot> + <innov_bar, innov_dot> = <Zref_bar, Zref_dot> + <K_bar, K_dot>
 *         + <Lgain_bar, Lgain_dot> + <x0_bar, x0_dot> + <xhat0_bar, xhat0_dot> + <model_bar, model_dot>.
 * Reductions: with Lgain = 0, Lgain_dot == NULL, xhat0_dot == NULL, Zref_dot == NULL and Xhat on Zref the estimator's chain is
 * zero, and Zout_dot is bit for bit qln_tracking_rollout_model_jvp's (K == NULL) on (x0_dot, model_dot), respectively
 * _guarded_jvp's with its event_dot; the reverse sweep's x0_bar and model_bar are those sweeps'.  A call with ny rows gives the
 * bits of the call with QLN_TRACK_NY_MAX rows whose further H rows and columns of L, Lgain_dot and innov are zero.
 * Refused with QLN_ERR_INVALID_ARGUMENT: a NULL h, Zref, Lgain, H, Zout, Xhat, Zout_dot or Zbar; ny outside
 * 1..QLN_TRACK_NY_MAX; a NULL event or event_hat (guarded); Lgain_dot or Lgain_bar without innov; K_dot or K_bar without K; no
 * tangent at all; an output that overlaps an input or another output.  The device forms do not validate device data; the host
 * forms also refuse a non-finite H, a model and event records as qln_tracking_rollout_guarded_jvp_host does.
 * Device pointers, stream-ordered; needs no cost table. */
int qln_tracking_rollout_estimated_jvp(qln_handle* h, const double* Zref, const double* K, const double* Lgain, const double* H,
                                       int32_t ny, const double* model, const double* Zout, const double* Xhat,
                                       const double* innov, const double* Zref_dot, const double* K_dot, const double* Lgain_dot,
                                       const double* x0_dot, const double* xhat0_dot, const double* model_dot, double* Zout_dot,
                                       double* Xhat_dot, double* innov_dot);
int qln_tracking_rollout_estimated_vjp(qln_handle* h, const double* Zref, const double* K, const double* Lgain, const double* H,
                                       int32_t ny, const double* model, const double* Zout, const double* Xhat,
                                       const double* innov, const double* Zbar, const double* Xhat_bar, const double* innov_bar,
                                       double* Zref_bar, double* K_bar, double* Lgain_bar, double* x0_bar, double* xhat0_bar,
                                       double* model_bar);
int qln_tracking_rollout_estimated_guarded_jvp(qln_handle* h, const double* Zref, const double* K, const double* Lgain,
                                               const double* H, int32_t ny, const double* model, const double* Zout,
                                               const double* Xhat, const double* innov, const double* event,
                                               const double* event_hat, const double* Zref_dot, const double* K_dot,
                                               const double* Lgain_dot, const double* x0_dot, const double* xhat0_dot,
                                               const double* model_dot, double* Zout_dot, double* Xhat_dot, double* innov_dot,
                                               double* event_dot, double* event_hat_dot);
int qln_tracking_rollout_estimated_guarded_vjp(qln_handle* h, const double* Zref, const double* K, const double* Lgain,
                                               const double* H, int32_t ny, const double* model, const double* Zout,
                                               const double* Xhat, const double* innov, const double* event,
                                               const double* event_hat, const double* Zbar, const double* Xhat_bar,
                                               const double* innov_bar, double* Zref_bar, double* K_bar, double* Lgain_bar,
                                               double* x0_bar, double* xhat0_bar, double* model_bar);
/* the same as host forms (see "Host forms" above; Zout_dot and Zref_bar are in-out as in the _model_ forms) */
int qln_tracking_rollout_estimated_jvp_host(qln_handle* h, const double* Zref, const double* K, const double* Lgain,
                                            const double* H, int32_t ny, const double* model, const double* Zout,
                                            const double* Xhat, const double* innov, const double* Zref_dot, const double* K_dot,
                                            const double* Lgain_dot, const double* x0_dot, const double* xhat0_dot,
                                            const double* model_dot, double* Zout_dot, double* Xhat_dot, double* innov_dot);
int qln_tracking_rollout_estimated_vjp_host(qln_handle* h, const double* Zref, const double* K, const double* Lgain,
                                            const double* H, int32_t ny, const double* model, const double* Zout,
                                            const double* Xhat, const double* innov, const double* Zbar, const double* Xhat_bar,
                                            const double* innov_bar, double* Zref_bar, double* K_bar, double* Lgain_bar,
                                            double* x0_bar, double* xhat0_bar, double* model_bar);
int qln_tracking_rollout_estimated_guarded_jvp_host(qln_handle* h, const double* Zref, const double* K, const double* Lgain,
                                                    const double* H, int32_t ny, const double* model, const double* Zout,
                                                    const double* Xhat, const double* innov, const double* event,
                                                    const double* event_hat, const double* Zref_dot, const double* K_dot,
                                                    const double* Lgain_dot, const double* x0_dot, const double* xhat0_dot,
                                                    const double* model_dot, double* Zout_dot, double* Xhat_dot,
                                                    double* innov_dot, double* event_dot, double* event_hat_dot);
int qln_tracking_rollout_estimated_guarded_vjp_host(qln_handle* h, const double* Zref, const double* K, const double* Lgain,
                                                    const double* H, int32_t ny, const double* model, const double* Zout,
                                                    const double* Xhat, const double* innov, const double* event,
                                                    const double* event_hat, const double* Zbar, const double* Xhat_bar,
                                                    const double* innov_bar, double* Zref_bar, double* K_bar, double* Lgain_bar,
                                                    double* x0_bar, double* xhat0_bar, double* model_bar);
/* CONTACT-AWARE FORCE LIMITS in the estimate-feedback roll-out and its sweeps: the loop of qln_tracking_rollout_estimated /
 * _guarded with the clamp of qln_tracking_rollout_limited.  The forces are fed back from a noisy estimate, so this is the loop
 * in which they chatter against stand_y_lo and the caps.  All of it is opt-in: every call above keeps its bits.  Knots are
 * 0-based, k = 0..N-2.
 * The loop (qln_tracking_rollout_estimated_limited).  qln_tracking_rollout_estimated (guarded == 0; event and event_hat must be
 *   NULL) or qln_tracking_rollout_estimated_guarded (guarded != 0) statement for statement, with one added step: after
 *   F_k = F_ref,k - K_k (xhat_k - x_ref,k) has been formed and before Zout's u_k is stored, the four forces go through the clamp
 *   of qln_tracking_rollout_limited.  lim (a HOST array of QLN_FORCE_LIMITS_N doubles), the codes s_m and the record
 *   sat[b][k] = sum_m s_m 4^m ([B][N-1], may be NULL: not written, the other outputs are the same) are the same as there: a NaN
 *   passes through with s_m = 0, F == lo exactly is s_m = 0, h_k is never clamped, and with K == NULL the reference's forces are
 *   clamped.
 * Whose contact mode picks the limits: the PLANT's.  Knot-scheduled: the handle's schedule (the jump knot is still in
 *   init_mode).  Guarded: the plant's current mode at the start of the knot, the landing foot counting as free for its whole
 *   touchdown knot -- exactly qln_tracking_rollout_limited's rule.  The limits are the plant's saturation, a fact about the
 *   ground and the actuator, not a decision of the controller; the estimator's believed mode picks nothing.
 * Where the applied forces go.  There is one set of applied forces, used everywhere: Zout's u_k, the plant's guard and step, the
 *   estimator's guard and step (the estimator is told what was applied, as it is above), and entry 6 of both event records.
 *   The plant's entry 6 is therefore >= stand_y_lo.  The estimator's need not be: it may believe a foot stands that does not,
 *   and that foot's force was clamped as a free one's.
 * Sweeps at FIXED ACTIVE SET (qln_tracking_rollout_estimated_limited_jvp / _vjp).  sat is a REQUIRED input, and takes part in
 *   the overlap rules.  event and event_hat both NULL select the blocks of qln_tracking_rollout_estimated_jvp / _vjp (then
 *   event_dot and event_hat_dot must be NULL), both given those of the _guarded_ forms; the other arguments, NULL rules and
 *   outputs are theirs.
 *   Forward:  the recursion of qln_tracking_rollout_estimated_jvp with dF_k multiplied by mask_k[m] = (s_m == 0) before
 *     anything reads it: Zout_dot's u_k, both chains' B applications, and both chains' dtau at their own touchdown knots.
 *   Reverse:  ubar_k[0:4] is masked after B^p' lam, B^e' lamm and both chains' taubar have been added onto it, and before
 *     K_k' ubar, K_bar and Zref_bar read it: the saturated channels' rows of K_bar and force slots of Zref_bar are exact zeros.
 *     Lgain_bar needs no mask.
 *   The two sweeps are exact adjoints: the duality identity of the estimated sweeps holds as it stands.  The one-sided-derivative
 *   caveat of qln_tracking_rollout_limited_jvp carries over: where the active set changes the map has a kink.
 * Exact reductions.
 *   1. All eight limits infinite: Zout, Xhat, innov, event and event_hat are the bits of qln_tracking_rollout_estimated /
 *      _guarded, and sat is all zeros.
 *   2. sat all zero in a sweep: every output has the bits of qln_tracking_rollout_estimated_jvp / _vjp, or of the _guarded_ forms.
 *   3. K == NULL and wnoise == NULL: Zout, event and sat are the bits of qln_tracking_rollout_limited(Zref, NULL, x0, model, lim,
 *      guarded, ...), whatever Lgain, H, vnoise and xhat0 are: the estimate does not reach the plant.
 *   4. Knot-scheduled form only: Lgain = 0, xhat0 == NULL, wnoise == NULL and Zref the output of
 *      qln_tracking_rollout_limited(.., K = NULL, .., lim, 0) under the handle's model: the estimate stays on Zref, so Zout and sat
 *      are the bits of qln_tracking_rollout_limited(Zref, NULL, x0, model, lim, 0) whatever K is.  In the guarded form this does
 *      not hold: a plant that lands in another knot than the nominal picks other limits.
 *   5. A call with ny rows equals the call with QLN_TRACK_NY_MAX rows and zero rows and columns, and every subset of optional
 *      outputs has the bits of the full call.
 * Errors: those of the two families, plus a NaN limit or lo > hi, a NULL lim, event or event_hat non-NULL with guarded == 0,
 *   exactly one of event / event_hat in a sweep, event_dot / event_hat_dot without records, a NULL sat in a sweep:
 *   QLN_ERR_INVALID_ARGUMENT.  The device forms do not validate sat; the host forms validate its codes as
 *   qln_tracking_rollout_limited_jvp_host does.  Device pointers, stream-ordered; needs no cost table. */
int qln_tracking_rollout_estimated_limited(qln_handle* h, const double* Zref, const double* K /* or NULL */, const double* Lgain,
                                           const double* H, int32_t ny, const double* vnoise, const double* wnoise,
                                           const double* x0, const double* xhat0, const double* model,
                                           const double* lim /* host, [QLN_FORCE_LIMITS_N] */, int32_t guarded, double* Zout,
                                           double* Xhat, double* innov, double* event /* NULL if guarded == 0 */,
                                           double* event_hat /* NULL if guarded == 0 */, double* sat /* [B][N-1] or NULL */);
int qln_tracking_rollout_estimated_limited_jvp(qln_handle* h, const double* Zref, const double* K, const double* Lgain,
                                               const double* H, int32_t ny, const double* model, const double* Zout,
                                               const double* Xhat, const double* innov,
                                               const double* event /* both NULL: the knot schedule; both given: guarded */,
                                               const double* event_hat, const double* sat /* required */,
                                               const double* Zref_dot, const double* K_dot, const double* Lgain_dot,
                                               const double* x0_dot, const double* xhat0_dot, const double* model_dot,
                                               double* Zout_dot, double* Xhat_dot, double* innov_dot, double* event_dot,
                                               double* event_hat_dot);
int qln_tracking_rollout_estimated_limited_vjp(qln_handle* h, const double* Zref, const double* K, const double* Lgain,
                                               const double* H, int32_t ny, const double* model, const double* Zout,
                                               const double* Xhat, const double* innov, const double* event,
                                               const double* event_hat, const double* sat /* required */, const double* Zbar,
                                               const double* Xhat_bar, const double* innov_bar, double* Zref_bar, double* K_bar,
                                               double* Lgain_bar, double* x0_bar, double* xhat0_bar, double* model_bar);
/* the same as host forms (see "Host forms" above; Zout, Zout_dot and Zref_bar are in-out as in the forms they extend; lim is a
 * host array in both) */
int qln_tracking_rollout_estimated_limited_host(qln_handle* h, const double* Zref, const double* K, const double* Lgain,
                                                const double* H, int32_t ny, const double* vnoise, const double* wnoise,
                                                const double* x0, const double* xhat0, const double* model, const double* lim,
                                                int32_t guarded, double* Zout, double* Xhat, double* innov, double* event,
                                                double* event_hat, double* sat);
int qln_tracking_rollout_estimated_limited_jvp_host(qln_handle* h, const double* Zref, const double* K, const double* Lgain,
                                                    const double* H, int32_t ny, const double* model, const double* Zout,
                                                    const double* Xhat, const double* innov, const double* event,
                                                    const double* event_hat, const double* sat, const double* Zref_dot,
                                                    const double* K_dot, const double* Lgain_dot, const double* x0_dot,
                                                    const double* xhat0_dot, const double* model_dot, double* Zout_dot,
                                                    double* Xhat_dot, double* innov_dot, double* event_dot,
                                                    double* event_hat_dot);
int qln_tracking_rollout_estimated_limited_vjp_host(qln_handle* h, const double* Zref, const double* K, const double* Lgain,
                                                    const double* H, int32_t ny, const double* model, const double* Zout,
                                                    const double* Xhat, const double* innov, const double* event,
                                                    const double* event_hat, const double* sat, const double* Zbar,
                                                    const double* Xhat_bar, const double* innov_bar, double* Zref_bar,
                                                    double* K_bar, double* Lgain_bar, double* x0_bar, double* xhat0_bar,
                                                    double* model_bar);
/* Fixed-interval SMOOTHING of a flown landing: the state at every knot given all N measurements, where the filter's Xhat_k uses
 * the measurements up to knot k only.  The modified Bryson-Frazier sweep, backward over the record a roll-out of the
 * estimate-feedback loop left (qln_tracking_rollout_estimated*), on the filter qln_tracking_kalman designed.  It inverts
 * nothing: the Rauch-Tung-Striebel form needs (P^-_{k+1})^-1, which is singular in ordinary use here (a clock slot with zero
 * initial and process variance).
 * Knots are 0-based.  A_k are exactly the blocks of qln_tracking_kalman at Ztraj's (x_k, u_k); guarded, the blocks of
 * qln_tracking_kalman_guarded at (Ztraj, model, event), with the touchdown knot's composite A*.  L_k = Lgain[b][k] and
 * P^+_k = Pest[b][k] are that call's outputs.  q_{N-1} = 0, Theta_{N-1} = 0, and for k = N-1 .. 0
 *     Xs_k     = Xhat_k + P^+_k q_k
 *     Ps_k     = P^+_k - P^+_k Theta_k P^+_k                 (lower triangle only: exactly symmetric)
 *     C_k      = I - L_k H
 *     e_k      = innov_k - H (L_k innov_k)                   (the post-fit residual)
 *     r_k      = H' (e_k ./ V) + C_k' q_k
 *     Lambda_k = H' diag(1/V) H C_k + C_k' Theta_k C_k       (lower triangle only)
 *     q_{k-1}  = A_{k-1}' r_k,   Theta_{k-1} = A_{k-1}' Lambda_k A_{k-1}
 * This is the Bryson-Frazier smoother rewritten with S^-1 = V^-1 (I - H L) and (I - L H) P^- = P^+, two identities that hold for
 * the optimal gains of qln_tracking_kalman at the same (Ztraj, H, V, Sigma0, W).  So the call needs neither Sigma0, W nor K, no
 * ny x ny factorisation and no 15 x 15 inverse -- and it does NOT check that Lgain and Pest belong together: with other gains it
 * returns the recursion's values, which are then not a smoother's.  First order at a fixed touchdown knot, as every sweep here.
 * Xs is in absolute coordinates (Xhat is), so no reference is read.
 * Inputs (all required but model): Ztraj [B] x z_stride, the trajectory the filter was designed along; Lgain [B][N][15][ny] and
 *   Pest [B][N][120] packed, qln_tracking_kalman's; H [ny][15] and Vdiag (a HOST array, ny entries, finite and > 0) as for that
 *   call, eight rows always, the rows behind ny being zero rows with V = 1 and zero columns of L, so a call gives the bits of the
 *   same call with those written out; Xhat [B][N][15] and innov [B][N][ny], the roll-out's record.
 * Outputs (each optional, at least one non-NULL; overwritten; which is asked for does not change the other's bits; none may
 * overlap an input or the other output):
 *   Xs: [B][N][15], the smoothed states.   Ps: [B][N][120] packed, their error covariances.
 * At knot N-1, Xs = Xhat and Ps = Pest bit for bit.
 * Refused with QLN_ERR_INVALID_ARGUMENT: ny outside 1..QLN_TRACK_NY_MAX, no output, a NULL event in the guarded form, a NULL
 * input, a V entry not finite or not > 0, overlaps -- the checks that need no handle before the null handle, in the family's
 * order.  The device forms do not validate device data; the host forms also refuse a non-finite H and validate model and event
 * as qln_tracking_kalman_guarded_host does.  A guarded batch without a touchdown and with model == NULL gives
 * qln_landing_smoother's bits for a handle with k_trans = N + 1.  Device pointers, stream-ordered; needs no cost table. */
int qln_landing_smoother(qln_handle* h, const double* Ztraj, const double* Lgain, const double* Pest, const double* H, int32_t ny,
                         const double* Vdiag /* host, ny entries, finite and > 0 */, const double* Xhat, const double* innov,
                         double* Xs /* [B][N][15] or NULL */, double* Ps /* [B][N][120] packed, or NULL */);
int qln_landing_smoother_host(qln_handle* h, const double* Ztraj, const double* Lgain, const double* Pest, const double* H,
                              int32_t ny, const double* Vdiag, const double* Xhat, const double* innov, double* Xs, double* Ps);
int qln_landing_smoother_guarded(qln_handle* h, const double* Ztraj, const double* model /* or NULL */,
                                 const double* event /* required */, const double* Lgain, const double* Pest, const double* H,
                                 int32_t ny, const double* Vdiag, const double* Xhat, const double* innov, double* Xs, double* Ps);
int qln_landing_smoother_guarded_host(qln_handle* h, const double* Ztraj, const double* model, const double* event,
                                      const double* Lgain, const double* Pest, const double* H, int32_t ny, const double* Vdiag,
                                      const double* Xhat, const double* innov, double* Xs, double* Ps);
/* The forward sweep through the DESIGN of the filter: how the gains, the error covariances and log det S_k of
 * qln_tracking_kalman* move when V, W or Sigma0 move -- the first question of noise identification and of a sensitivity study of
 * the estimator, and with qln_landing_filter_jvp the total derivative of the likelihood through the gains' design.  (The entries
 * stand outside the qln_tracking_ prefix, as the smoother's and the filter's do.)  It runs at what the design returned, the
 * gains L_k = Lgain[b][k], and re-runs nothing: neither P^-, Sigma0, W nor a factorisation is read.  At the optimal gain the
 * Joseph form is stationary in L (S L' = H P^- cancels the dL term), so with dotted quantities as tangents, for k = 0 .. N-1:
 *     Pd^-_0     = Sigma0_dot
 *     Gd         = H Pd^-_k                                        (ny x 15)
 *     Sd_k       = Gd H' + diag(V_dot)                             (ny x ny, symmetric)
 *     Sinv_k     = diag(1/V) (I - H L_k)                           (the smoother's identity; symmetric for optimal gains)
 *     Ld_k       = (Pd^-_k H' - L_k Sd_k) Sinv_k                   (15 x ny)
 *     logdet_dot_k = sum_ab Sinv_k[a][b] Sd_k[a][b]                (= d log det S_k)
 *     Pd^+_k     = (I - L_k H) Pd^-_k (I - L_k H)' + L_k diag(V_dot) L_k'
 *     Pd^-_{k+1} = A_k Pd^+_k A_k' + diag(W_dot)
 * A_k are exactly the open-loop blocks of qln_tracking_kalman at Zout's (x_k, u_k); guarded, those of
 * qln_tracking_kalman_guarded at (Zout, model, event), with the touchdown knot's composite A*.  First order at a fixed touchdown
 * knot, as every sweep here.  Nothing is divided or factored, and Sigma0_dot may be indefinite.
 * TWO CAVEATS.  The call cannot check that Lgain is optimal for (Zout, H, V, Sigma0, W): with other gains it returns the
 * recursion's values, which are then no derivative.  And I - H L_k loses |H P^- H'| / V digits (S^-1 = V^-1 (I - H L) with H L
 * near I when the prior dominates the sensor), the loss qln_landing_filter's score has; it reaches Ld and logdet_dot, not Pd^+.
 * Inputs: Zout [B] x z_stride; Lgain [B][N][15][ny]; H [ny][15] and Vdiag (a HOST array, ny entries, finite and > 0) as for the
 *   design, eight rows always, the rows behind ny being zero rows with V = 1, V_dot = 0 and zero columns of L, so a call gives the
 *   bits of the same call with those written out.  The direction, each optional (NULL: zero), at least one: Sigma0_dot
 *   [sigma0_batch][120] packed (sigma0_batch 1 or B; not read when Sigma0_dot is NULL), Wdiag_dot (HOST, 15) and Vdiag_dot
 *   (HOST, ny), finite, of either sign.
 * Outputs (each optional, at least one non-NULL; overwritten; which are asked for changes no other output's bits; none may
 * overlap an input or another output): Lgain_dot [B][N][15][ny]; Pest_dot [B][N][120] packed; logdet_dot [B][N].
 * With Lgain = 0 and Vdiag_dot = NULL, Pest_dot is qln_tracking_covariance*'s Sigma (K = NULL) at Sigma0 = Sigma0_dot,
 * W = Wdiag_dot, bit for bit.
 * Refused with QLN_ERR_INVALID_ARGUMENT, the checks that need no handle before the null handle, in this order: ny outside
 * 1..QLN_TRACK_NY_MAX, no output, a NULL event in the guarded form, a NULL H or Vdiag, a V entry not finite or not > 0, all three
 * tangents NULL, a non-finite entry of Wdiag_dot or Vdiag_dot, a NULL Lgain, sigma0_batch < 1 with Sigma0_dot; behind the handle
 * sigma0_batch not 1 or B with Sigma0_dot, a NULL Zout, and an output that overlaps an input or another output.  The device
 * forms do not validate device data; the host forms also refuse a non-finite H and validate model and event as
 * qln_tracking_kalman_guarded_host does.  A guarded batch without a touchdown and with model == NULL gives
 * qln_kalman_design_jvp's bits for a handle with k_trans = N + 1.  Device pointers, stream-ordered; needs no cost table. */
int qln_kalman_design_jvp(qln_handle* h, const double* Zout, const double* Lgain, const double* H, int32_t ny,
                          const double* Vdiag /* host, ny entries, finite and > 0 */, const double* Sigma0_dot /* or NULL */,
                          int32_t sigma0_batch, const double* Wdiag_dot /* host, or NULL */,
                          const double* Vdiag_dot /* host, or NULL */, double* Lgain_dot, double* Pest_dot, double* logdet_dot);
int qln_kalman_design_jvp_host(qln_handle* h, const double* Zout, const double* Lgain, const double* H, int32_t ny,
                               const double* Vdiag, const double* Sigma0_dot, int32_t sigma0_batch, const double* Wdiag_dot,
                               const double* Vdiag_dot, double* Lgain_dot, double* Pest_dot, double* logdet_dot);
int qln_kalman_design_guarded_jvp(qln_handle* h, const double* Zout, const double* model /* or NULL */,
                                  const double* event /* required */, const double* Lgain, const double* H, int32_t ny,
                                  const double* Vdiag, const double* Sigma0_dot, int32_t sigma0_batch, const double* Wdiag_dot,
                                  const double* Vdiag_dot, double* Lgain_dot, double* Pest_dot, double* logdet_dot);
int qln_kalman_design_guarded_jvp_host(qln_handle* h, const double* Zout, const double* model, const double* event,
                                       const double* Lgain, const double* H, int32_t ny, const double* Vdiag,
                                       const double* Sigma0_dot, int32_t sigma0_batch, const double* Wdiag_dot,
                                       const double* Vdiag_dot, double* Lgain_dot, double* Pest_dot, double* logdet_dot);
/* The REVERSE sweep through the design of the filter: the transpose of qln_kalman_design_jvp*'s linear map, so that one design,
 * one filter and two reverse sweeps give the whole gradient of a likelihood with respect to the noise (with
 * qln_landing_filter_vjp), where forward mode takes one sweep per parameter.  Per problem that map takes (Sigma0_dot[120],
 * Wdiag_dot[15], Vdiag_dot[ny]) to (Lgain_dot[N][15][ny], Pest_dot[N][120], logdet_dot[N]); its coefficients depend on Zout
 * (through A_k), Lgain, H and V only.  This call is its transpose BETWEEN THE ARRAYS AS STORED: cotangents (Lgain_bar, Pest_bar,
 * logdet_bar) in, (Sigma0_bar, Wdiag_bar, Vdiag_bar) out, PER PROBLEM -- the forward call shares Wdiag_dot and Vdiag_dot over the
 * batch, the transpose does not sum over it (the caller does, if it wants that), so nothing is accumulated across problems and
 * the results are deterministic.  For every direction and every cotangent, over the stored arrays and with no weights,
 *     <Lgain_bar, Lgain_dot> + <Pest_bar, Pest_dot> + <logdet_bar, logdet_dot> = <Sigma0_bar, Sigma0_dot> + <Wdiag_bar, Wdiag_dot>
 *                                                                               + <Vdiag_bar, Vdiag_dot>.
 * The packed convention that makes it so: a packed off-diagonal entry stands for both (i, j) and (j, i); Pest_bar[p] enters the
 * full symmetric cotangent as Pest_bar[p] / 2 on each side (the diagonal as it is), and Sigma0_bar[p] = Lambda_0(i, j) +
 * Lambda_0(j, i) off the diagonal, Lambda_0(i, i) on it.  With C = I - L_k H, Sinv = diag(1/V) (I - H L_k), sym(X) = (X + X') / 2
 * and Lambda the full symmetric cotangent of Pd^-_{k+1} (zero behind the last knot), for k = N-1 .. 0:
 *     Wdiag_bar += diag(Lambda);   Pi = A_k' Lambda A_k + sym(Pest_bar_k)          (k = N-1: Pi = sym(Pest_bar_k))
 *     Vdiag_bar += diag(L_k' Pi L_k)
 *     Tb         = Lgain_bar_k Sinv'             row j: (lb_j - (lb_j L_k') H') ./ V         (15 x ny)
 *     Sb         = -L_k' Tb + logdet_bar_k Sinv                                               (ny x ny)
 *     Vdiag_bar += diag(Sb)
 *     Lambda     = C' Pi C + H' sym(Sb) H + sym(Tb H)
 * and Sigma0_bar = pack(Lambda_0).  A_k are the forward sweep's blocks; guarded, the touchdown knot's composite A*, applied
 * transposed as qln_landing_smoother_guarded applies it.  Nothing is divided or factored, and the cotangents may have any sign.
 * THE FORWARD CALL'S TWO CAVEATS hold here: with gains that are not optimal for (Zout, H, V, Sigma0, W) the result is the
 * transpose of a map that is no derivative; and I - H L_k loses |H P^- H'| / V digits, a loss that here reaches every output
 * that Lgain_bar or logdet_bar feeds.
 * Inputs: Zout, Lgain, H, ny and Vdiag as for qln_kalman_design_jvp (Zout's last knot and padding are not read), eight rows
 *   always, the rows behind ny being zero rows with V = 1 and zero columns of L and Lgain_bar, so a call gives the bits of the
 *   same call with those written out.  The cotangents, each optional (NULL: zero, not read, the bits of explicit zeros), at least
 *   one: Lgain_bar [B][N][15][ny], Pest_bar [B][N][120] packed, logdet_bar [B][N].
 * Outputs (each optional, at least one non-NULL; overwritten; which are asked for changes no other output's bits; none may
 * overlap an input or another output; device arrays in the device forms): Sigma0_bar [B][120] packed; Wdiag_bar [B][15];
 * Vdiag_bar [B][ny].
 * Refused with QLN_ERR_INVALID_ARGUMENT, the checks that need no handle before the null handle, in this order: ny outside
 * 1..QLN_TRACK_NY_MAX, no output, a NULL event in the guarded form, a NULL H or Vdiag, a V entry not finite or not > 0, all three
 * cotangents NULL, a NULL Lgain; behind the handle a NULL Zout, and an output that overlaps an input or another output.  The
 * device forms do not validate device data; the host forms also refuse a non-finite H and validate model and event as
 * qln_tracking_kalman_guarded_host does.  A guarded batch without a touchdown and with model == NULL gives
 * qln_noise_design_vjp's bits for a handle with k_trans = N + 1.  Device pointers, stream-ordered; needs no cost table.
 * (The entries stand outside the qln_tracking_, qln_landing_ and qln_kalman_ prefixes, whose sets are closed.) */
int qln_noise_design_vjp(qln_handle* h, const double* Zout, const double* Lgain, const double* H, int32_t ny,
                         const double* Vdiag /* host, ny entries, finite and > 0 */, const double* Lgain_bar /* or NULL */,
                         const double* Pest_bar /* or NULL */, const double* logdet_bar /* or NULL */,
                         double* Sigma0_bar /* [B][120] or NULL */, double* Wdiag_bar /* [B][15] or NULL */,
                         double* Vdiag_bar /* [B][ny] or NULL */);
int qln_noise_design_vjp_host(qln_handle* h, const double* Zout, const double* Lgain, const double* H, int32_t ny,
                              const double* Vdiag, const double* Lgain_bar, const double* Pest_bar, const double* logdet_bar,
                              double* Sigma0_bar, double* Wdiag_bar, double* Vdiag_bar);
int qln_noise_design_guarded_vjp(qln_handle* h, const double* Zout, const double* model /* or NULL */,
                                 const double* event /* required */, const double* Lgain, const double* H, int32_t ny,
                                 const double* Vdiag, const double* Lgain_bar, const double* Pest_bar, const double* logdet_bar,
                                 double* Sigma0_bar, double* Wdiag_bar, double* Vdiag_bar);
int qln_noise_design_guarded_vjp_host(qln_handle* h, const double* Zout, const double* model, const double* event,
                                      const double* Lgain, const double* H, int32_t ny, const double* Vdiag,
                                      const double* Lgain_bar, const double* Pest_bar, const double* logdet_bar,
                                      double* Sigma0_bar, double* Wdiag_bar, double* Vdiag_bar);
/* The FILTER on recorded data, and the score of that data under it: the estimator of qln_tracking_rollout_estimated* as a call
 * of its own, for a landing that was flown elsewhere -- sensor readings and the forces that were applied -- where that call
 * produces Xhat and innov only together with a plant it integrates itself.  Its outputs feed qln_landing_smoother*, and loglik
 * says how consistent the filter (its gains, its V) is with the data.
 * Knots are 0-based.  For k = 0 .. N-1, with xhat^-_0 = xhat0[b] (NULL: x_ref,0):
 *     innov_k = Y[b][k] - H (xhat^-_k - x_ref,k)          yh exactly as the roll-out forms it
 *     xhat_k  = xhat^-_k + L_k innov_k                    column by column onto each entry, as there
 *     e_k     = innov_k - H (L_k innov_k)                 (the post-fit residual; L_k innov_k formed apart from xhat)
 *     nis_k   = sum_r innov_k[r] e_k[r] / V[r]            (the normalised innovation squared, innov' S^-1 innov)
 *     G_k     = lower triangle of diag(1/V) (I - H L_k)   (= S_k^-1 for the optimal gains)
 *     ldS_k   = - sum_i log d_i,  d the pivots of the L D L' of G_k without pivoting      (= log det S_k)
 *     if k < N-1:  u_k = the five control slots of Zrec at knot k;  xhat^-_{k+1} = Phi_k(xhat_k, u_k; the handle's model)
 *     loglik[b] = -1/2 sum_k (nis_k + ldS_k + ny log 2 pi)
 * Phi_k is the estimator's step of the estimate-feedback roll-out: knot-scheduled, by the handle's k_trans and init_mode; guarded,
 * the guarded step with the estimator's own mode, guard and touchdown record, written to event_hat (entry 6 means what it means
 * in the flight: the least vertical force asked of a foot the ESTIMATOR believed standing).  A replay of a flight -- Y its
 * measurements, Zrec its Zout -- returns that flight's Xhat, innov and event_hat; bit for bit where Y holds the flight's bits.
 * The score comes from the gains alone, through S^-1 = V^-1 (I - H L), which holds for the optimal gains of qln_tracking_kalman*
 * at the same (H, V): no P^-, no Sigma0 and no W is read, and nothing is inverted but the eight pivots.  The call CANNOT check
 * that Lgain belongs to V: with other gains score and loglik are the recursion's values, not a likelihood, and a pivot d_i that
 * is not > 0 gives NaN in ldS_k and loglik.
 * Inputs: Zref [B] x z_stride, of which ONLY THE STATE SLOTS are read (x_ref,k); Zrec [B] x z_stride, of which ONLY THE CONTROL
 *   SLOTS are read: the four applied forces and h_k, laid out as in Z -- the forces after any clamp, so one call replays limited
 *   and unlimited flights alike; its state slots are not read, so a user with real data fills nothing else.  Lgain
 *   [B][N][15][ny] and H [ny][15] as for qln_tracking_rollout_estimated.  Y [B][N][ny]: the measurement in the form the roll-out
 *   forms it, the reading minus H x_ref,k.  xhat0 [B][15] or NULL.  Vdiag: a HOST array, ny entries, required only when score or
 *   loglik is asked for, then finite and > 0.  The kernel works on eight rows always, the rows behind ny being zero rows of H,
 *   zero columns of L and V = 1, which add exact zeros (log 1), so a call gives the bits of the same call with those written out
 *   -- in Xhat, innov's ny columns, score and event_hat; loglik counts its measurements, so the written-out call's is lower by
 *   (8 - ny) N log(2 pi) / 2, the density of the added readings.
 * Outputs (each optional, at least one non-NULL; overwritten; which are asked for does not change the others' bits; none may
 * overlap an input or another output):
 *   Xhat [B][N][15]; innov [B][N][ny]; score [B][N][2] = {nis_k, ldS_k}; loglik [B]; event_hat [B][QLN_TOUCHDOWN_INFO_STRIDE]
 *   (guarded only).
 * Refused with QLN_ERR_INVALID_ARGUMENT, the checks that need no handle before the null handle, in the family's order: ny outside
 * 1..QLN_TRACK_NY_MAX, no output, a NULL Vdiag with score or loglik, a V entry not finite or not > 0 (then), a NULL H, Lgain or
 * Y; behind the handle a NULL Zref, a NULL Zrec, overlaps.  The device forms do not validate device data; the host forms also
 * refuse a non-finite H.  Device pointers, stream-ordered; needs no cost table. */
int qln_landing_filter(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H, int32_t ny,
                       const double* Vdiag /* host, ny entries, or NULL without score and loglik */, const double* Y,
                       const double* xhat0 /* or NULL */, double* Xhat, double* innov, double* score, double* loglik);
int qln_landing_filter_host(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H, int32_t ny,
                            const double* Vdiag, const double* Y, const double* xhat0, double* Xhat, double* innov, double* score,
                            double* loglik);
int qln_landing_filter_guarded(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H,
                               int32_t ny, const double* Vdiag, const double* Y, const double* xhat0, double* Xhat, double* innov,
                               double* score, double* loglik, double* event_hat /* [B][QLN_TOUCHDOWN_INFO_STRIDE] or NULL */);
int qln_landing_filter_guarded_host(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H,
                                    int32_t ny, const double* Vdiag, const double* Y, const double* xhat0, double* Xhat,
                                    double* innov, double* score, double* loglik, double* event_hat);
/* The filter at a MODEL OF EACH RECORD'S OWN: the calls above with model [B][QLN_MODEL_NP] = {g, mb, mf, lb} per problem behind
 * ny, in the family's order; Phi_k is taken at model[b] where the calls above take the handle's model.  model == NULL is the
 * handle's four values, and with NULL or with rows that hold those values every output has the bits of the call above.  The host
 * forms also refuse a model entry that is not finite, or a mass or the body length that is not positive.  Everything else --
 * inputs, outputs, refusals -- as above. */
int qln_landing_filter_model(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H, int32_t ny,
                             const double* model /* [B][QLN_MODEL_NP] or NULL */, const double* Vdiag, const double* Y,
                             const double* xhat0, double* Xhat, double* innov, double* score, double* loglik);
int qln_landing_filter_model_host(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H,
                                  int32_t ny, const double* model, const double* Vdiag, const double* Y, const double* xhat0,
                                  double* Xhat, double* innov, double* score, double* loglik);
int qln_landing_filter_guarded_model(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H,
                                     int32_t ny, const double* model, const double* Vdiag, const double* Y, const double* xhat0,
                                     double* Xhat, double* innov, double* score, double* loglik, double* event_hat);
int qln_landing_filter_guarded_model_host(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain,
                                          const double* H, int32_t ny, const double* model, const double* Vdiag, const double* Y,
                                          const double* xhat0, double* Xhat, double* innov, double* score, double* loglik,
                                          double* event_hat);
/* The SWEEPS THROUGH THE FILTER: the forward (tangent) and the reverse (cotangent) sweep of qln_landing_filter_model* and of its
 * score, at the record and at the trajectory the filter produced.  Nothing is re-run.
 * Evaluation point (both sweeps): Zref; Zrec, of which only the control slots are read; Lgain, H, ny; model or NULL; Xhat, the
 * filter's output; innov, its other output, REQUIRED EXACTLY WHEN a tangent or cotangent of Lgain or a score term is asked for;
 * Vdiag, a HOST array of ny entries, required exactly when a score term is asked for, then finite and > 0; the guarded forms
 * also take event_hat, the filter's record, of which only entries 0 (the knot) and 1 (tau) are read.  Zref gets no tangent and
 * is not read: Y already is the reading minus H x_ref, so x_ref cancels out of every derivative; it keeps its place in the
 * family's order and must not be NULL.
 * Forward sweep.  Tangents, each optional (NULL: zero), at least one: Y_dot [B][N][ny]; Zrec_dot in the layout of Z, of which
 * only the control slots are read (dF_k, dh_k); Lgain_dot [B][N][15][ny]; xhat0_dot [B][15] (NULL means zero: x_ref,0 is an
 * input without a tangent here); model_dot [B][QLN_MODEL_NP].
 *     dxm_0 = xhat0_dot
 *     for k = 0 .. N-1:
 *       dinnov_k  = Y_dot_k - H dxm_k
 *       dxh_k     = dxm_k + L_k dinnov_k + Lgain_dot_k innov_k
 *       de_k      = dinnov_k - H (L_k dinnov_k)
 *       nis_dot_k = sum_r (dinnov_k[r] e_k[r] + innov_k[r] de_k[r]) / V[r]            (e_k as in qln_landing_filter)
 *       if k < N-1:  dxm_{k+1} = A^e_k dxh_k + B^e_k (dF_k, dh_k) + G^e_k model_dot
 *     loglik_dot[b] = -1/2 sum_k nis_dot_k
 * [A^e B^e G^e] is the block of qln_tracking_rollout_model_jvp at (Xhat_k, Zrec's u_k, model[b]); guarded, the blocks of
 * qln_tracking_rollout_guarded_jvp at the estimator's own touchdown knot and tau from event_hat: at that knot the composite
 * step, whose d tau depends on dxh, dF and model_dot.
 * Outputs (each optional, at least one; overwritten; which are asked for does not change the others' bits): Xhat_dot
 * [B][N][15]; innov_dot [B][N][ny]; nis_dot [B][N]; loglik_dot [B]; guarded: event_hat_dot [B][QLN_TOUCHDOWN_INFO_STRIDE] with
 * the entries qln_tracking_rollout_guarded_jvp defines (1: d tau, 2: the touchdown clock's tangent, the rest zeros).
 * FIXED GAINS.  log det S_k depends on Lgain alone, and its derivative is not offered: nis_dot or loglik_dot together with
 * Lgain_dot is refused, and loglik_dot is the EXACT derivative of loglik AT FIXED GAINS (the prediction-error gradient).  The
 * gains of qln_tracking_kalman* themselves depend on the model: a caller to whom the total derivative matters redesigns them
 * between outer iterations.  For the total derivative along (Sigma0_dot, W_dot, V_dot), qln_kalman_design_jvp gives the
 * Lgain_dot to pass here (without a score term) and the derivative of log det S_k.
 * Reverse sweep, the exact transpose.  Cotangents, each optional (NULL: zero), at least one: Xhat_bar [B][N][15]; innov_bar
 * [B][N][ny]; nis_bar [B][N]; loglik_bar [B].  With nb_k = nis_bar_k - loglik_bar / 2 and lamm, the cotangent of dxm_{k+1}, zero
 * behind the last knot, for k = N-1 .. 0:
 *     k < N-1:  ubar_k = B^e' lamm;  xhb = Xhat_bar_k + A^e' lamm;  model_bar += G^e' lamm          (k = N-1: xhb = Xhat_bar_k)
 *     ib   = innov_bar_k + L_k' xhb + nb_k (G_k + G_k') innov_k,    G_k = diag(1/V) (I - H L_k), the FULL matrix
 *     lamm = xhb - H' ib
 * Outputs (each optional, at least one): Y_bar [B][N][ny] = ib; Zrec_bar in the layout of Z: ubar_k in the control slots, exact
 * zeros in the state slots, entries past n_nlp never written; Lgain_bar [B][N][15][ny] = xhb innov_k', refused together with
 * nis_bar or loglik_bar for the reason above; xhat0_bar [B][15] = lamm after knot 0; model_bar [B][QLN_MODEL_NP].
 * Reductions: nis_dot_k and ib are sums over the sensor rows in row order, each row's H-product a sum over a row of sixteen
 * lanes in a fixed tree; model_bar is summed over the knots per state and then over the states.  The loops over the sensor rows
 * run to QLN_TRACK_NY_MAX under r < ny, the rows behind ny taking V = 1, so a call with ny rows gives the bits of the call with
 * eight rows and zeros written out.
 * <Xhat_bar, Xhat_dot> + <innov_bar, innov_dot> + <nis_bar, nis_dot> + <loglik_bar, loglik_dot> = <Y_bar, Y_dot> + <Zrec_bar,
 * Zrec_dot> + <Lgain_bar, Lgain_dot> + <xhat0_bar, xhat0_dot> + <model_bar, model_dot> holds in both modes.
 * Refused with QLN_ERR_INVALID_ARGUMENT, the checks that need no handle before the null handle, in the family's order: ny outside
 * 1..QLN_TRACK_NY_MAX, no tangent (no cotangent), no output, Lgain_dot (Lgain_bar) together with a score term, a NULL Vdiag
 * with a score term, a V entry not finite or not > 0 (then), a NULL innov where it is required, a NULL event_hat (guarded), a
 * NULL H or Lgain; behind the handle a NULL Zref, Zrec or Xhat, and an output that overlaps an input or another output.  The
 * device forms do not validate device data; the host forms also refuse a non-finite H, a model as above and an event_hat whose
 * knot is not an integer in [-1, N-2] or whose tau is not finite and >= 0.  Device pointers, stream-ordered; needs no cost
 * table. */
int qln_landing_filter_jvp(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H, int32_t ny,
                           const double* model /* or NULL */, const double* Vdiag /* host, or NULL without a score term */,
                           const double* Xhat, const double* innov /* or NULL */, const double* Y_dot, const double* Zrec_dot,
                           const double* Lgain_dot, const double* xhat0_dot, const double* model_dot, double* Xhat_dot,
                           double* innov_dot, double* nis_dot, double* loglik_dot);
int qln_landing_filter_jvp_host(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H,
                                int32_t ny, const double* model, const double* Vdiag, const double* Xhat, const double* innov,
                                const double* Y_dot, const double* Zrec_dot, const double* Lgain_dot, const double* xhat0_dot,
                                const double* model_dot, double* Xhat_dot, double* innov_dot, double* nis_dot, double* loglik_dot);
int qln_landing_filter_guarded_jvp(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H,
                                   int32_t ny, const double* model, const double* Vdiag, const double* Xhat, const double* innov,
                                   const double* event_hat /* required */, const double* Y_dot, const double* Zrec_dot,
                                   const double* Lgain_dot, const double* xhat0_dot, const double* model_dot, double* Xhat_dot,
                                   double* innov_dot, double* nis_dot, double* loglik_dot, double* event_hat_dot);
int qln_landing_filter_guarded_jvp_host(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H,
                                        int32_t ny, const double* model, const double* Vdiag, const double* Xhat,
                                        const double* innov, const double* event_hat, const double* Y_dot, const double* Zrec_dot,
                                        const double* Lgain_dot, const double* xhat0_dot, const double* model_dot,
                                        double* Xhat_dot, double* innov_dot, double* nis_dot, double* loglik_dot,
                                        double* event_hat_dot);
int qln_landing_filter_vjp(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H, int32_t ny,
                           const double* model, const double* Vdiag, const double* Xhat, const double* innov,
                           const double* Xhat_bar, const double* innov_bar, const double* nis_bar, const double* loglik_bar,
                           double* Y_bar, double* Zrec_bar, double* Lgain_bar, double* xhat0_bar, double* model_bar);
int qln_landing_filter_vjp_host(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H,
                                int32_t ny, const double* model, const double* Vdiag, const double* Xhat, const double* innov,
                                const double* Xhat_bar, const double* innov_bar, const double* nis_bar, const double* loglik_bar,
                                double* Y_bar, double* Zrec_bar, double* Lgain_bar, double* xhat0_bar, double* model_bar);
int qln_landing_filter_guarded_vjp(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H,
                                   int32_t ny, const double* model, const double* Vdiag, const double* Xhat, const double* innov,
                                   const double* event_hat /* required */, const double* Xhat_bar, const double* innov_bar,
                                   const double* nis_bar, const double* loglik_bar, double* Y_bar, double* Zrec_bar,
                                   double* Lgain_bar, double* xhat0_bar, double* model_bar);
int qln_landing_filter_guarded_vjp_host(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H,
                                        int32_t ny, const double* model, const double* Vdiag, const double* Xhat,
                                        const double* innov, const double* event_hat, const double* Xhat_bar,
                                        const double* innov_bar, const double* nis_bar, const double* loglik_bar, double* Y_bar,
                                        double* Zrec_bar, double* Lgain_bar, double* xhat0_bar, double* model_bar);
/* Z <- Z + N(0, sigma^2) on every entry, step lengths h then clipped to [h_min, h_max] (redraw_h = 0) or redrawn
 * U(h_min, h_max) (redraw_h != 0) -- the evaluation point of SURVEY.md 8d from qln_initial_guess's Z0.  The normal
 * draws are Box-Muller on the sampler's stream from `stream_offset`: the recipe's distribution, not numpy's numbers. */
int qln_perturb_point(qln_handle* h, const qln_drop_state_sampler* s, double* Z, double sigma, double h_min, double h_max,
                      int redraw_h);
/* the handle's current boundary states, copied to host arrays ([B][15] each; either may be NULL) */
int qln_get_boundary_states(qln_handle* h, double* x0, double* xf);
/* The notebook's objective built on the device: obj[k] = LQRCost(Q, R, Xref[k], Uref[k]), k < N, and
 * obj[N] = LQRCost(Qf, R*0, Xref[N], Uref[1]) (src/main.ipynb:158-161, src/quadratic_cost.jl:33-42) with Xref/Uref of
 * reference_trajectory(model, N, k_trans, xf, init_mode, dt) (src/ref_traj.jl:6-39).  Q, Qf: 15 diagonal entries,
 * R: 5.  per_problem != 0 builds one table per problem (k_trans / init_mode / xf may differ), else one shared table
 * from problem 0.  Replaces any previous cost table of the handle. */
int qln_set_lqr_cost(qln_handle* h, const double* Qdiag, const double* Rdiag, const double* Qfdiag, double dt,
                     int per_problem);
/* Copies the handle's cost table ([cost_batch][N][41]) to a host buffer; cost_batch is returned through *cost_batch. */
int qln_get_cost(qln_handle* h, double* cost_host, int32_t* cost_batch);

/* MOI mode: the host forms of the evaluator (see "Host forms" above) */
int qln_eval_objective_host(qln_handle* h, const double* Z, double* f);
int qln_eval_objective_gradient_host(qln_handle* h, const double* Z, double* grad);
int qln_eval_constraint_host(qln_handle* h, const double* Z, double* c);
int qln_eval_constraint_jacobian_host(qln_handle* h, const double* Z, double* vals);
/* MOI mode of qln_eval_hessian_lagrangian (:Hess) */
int qln_eval_hessian_lagrangian_host(qln_handle* h, const double* Z, const double* sigma, const double* mu, double* hvals);
/* MOI mode of qln_eval_hessian_lagrangian_product (:HessVec) and of qln_eval_constraint_jvp / _vjp (:JacVec,
 * eval_constraint_jacobian_product / _transpose_product) */
int qln_eval_hessian_lagrangian_product_host(qln_handle* h, const double* Z, const double* sigma, const double* mu,
                                             const double* v, double* y);
int qln_eval_constraint_jvp_host(qln_handle* h, const double* Z, const double* v, double* y);
int qln_eval_constraint_vjp_host(qln_handle* h, const double* Z, const double* lam, double* g);
/* Reference-compatible dense Jacobian of ONE problem (src/moi.jl:15-24): `jac` is a host,
 * column-major m_nlp x n_nlp buffer; exactly the jac_c! write-set is assigned (explicit zeros of
 * the identity blocks included), every other entry is left untouched.  `b` selects the problem. */
int qln_eval_constraint_jacobian_dense_host(qln_handle* h, int32_t b, const double* Z, double* jac);

/* Placement-aware allocation of the Jacobian buffer (optional; every entry point also accepts plain hipMalloc memory).
 * On MI355X the store bandwidth a buffer sustains depends on where it lies physically: device memory behaves as
 * 32-GiB regions, and the evaluator's eight write fronts (one per XCD, the first four in the first half of vals) run
 * ~20 % faster when the two halves of the buffer lie in different regions (DESIGN.md section 5,
 * profiles/r01_placement_regions.txt).  This call builds such a buffer with the HIP virtual-memory API: it maps
 * j_total doubles + 64 GiB of physical memory (less if less is free) in 256-MiB chunks behind one virtual range,
 * times the fused launch on windows of that range, keeps the fastest window and returns every chunk outside it to the
 * driver.  Buffers under 1 GiB are mapped as they come.  Z as for qln_eval_constraint_and_jacobian; c: the constraint
 * buffer the timed launches write -- it is OVERWRITTEN -- or NULL to have the call use a scratch buffer of its own.
 * *vals is at least 2-MiB aligned and holds j_total doubles; constants are not written.  ms_best (may be NULL): launch
 * time on the window kept.  QLN_ERR_HIP if the memory or the virtual-memory API is not available; nothing stays
 * allocated or mapped after a failure.
 * Release with qln_vals_free_placed (qln_destroy releases what is left).  Both wait for the whole DEVICE to go idle
 * before unmapping -- the buffer is plain memory to its users, so work on any stream may still be touching it -- and
 * report a failing unmap / release instead of hiding it.  The physical memory goes back to the driver; the virtual
 * range stays reserved for the life of the process, because on ROCm 7.2 an address that has been unmapped keeps
 * serving accesses through its old translations if it is ever mapped again (bench/vmm_va_reuse.cpp,
 * profiles/r02_vmm_va_reuse.txt): ~70 GiB of address space per call, of 128 TiB. */
int qln_vals_alloc_placed(qln_handle* h, const double* Z, double* c, double** vals, float* ms_best);
/* The same with the transient memory the scan may map beyond j_total doubles chosen by the caller (qln_vals_alloc_placed
 * = 64 GiB: two region lengths, so the slab contains two region boundaries and the scan has two chances of a clean
 * straddling window).  32 GiB gives one boundary, 0 maps the buffer as it comes (no scan: a plain allocation's luck).
 * Measured consequence: profiles/r03_placement_budget.txt.  The virtual range reserved (and retired, see below) is
 * j_total * 8 + transient_bytes. */
int qln_vals_alloc_placed_budget(qln_handle* h, const double* Z, double* c, int64_t transient_bytes, double** vals, float* ms_best);
/* Address space retired by placed allocations in this process so far (their virtual ranges are never returned, see
 * above) and the cap at which qln_vals_alloc_placed refuses with QLN_ERR_UNSUPPORTED and a message that says so (64 TiB of
 * the 128 TiB: ~900 default-size calls).  Either pointer may be NULL.  Needs no handle. */
int qln_vals_placed_address_space(int64_t* retired_bytes, int64_t* cap_bytes);
int qln_vals_free_placed(qln_handle* h, double* vals);
/* What the placement scan of a buffer returned by qln_vals_alloc_placed did (each out pointer may be NULL). */
int qln_vals_placed_info(const qln_handle* h, const double* vals, int64_t* chunk_bytes, int64_t* chunks_scanned,
                         int64_t* window_first_chunk);

/* Measurement helper for bench.py: runs `warmup` + `iters` launches of the fused hot path on the
 * handle's stream and returns each timed launch's duration from HIP events (milliseconds). */
int qln_time_constraint_and_jacobian(qln_handle* h, const double* Z, double* c, double* vals, uint32_t flags,
                                     int32_t warmup, int32_t iters, float* ms_each /*[iters]*/);
/* The same launches back to back with nothing between them: ONE pair of HIP events around all `iters` launches;
 * *ms_total = elapsed ms of the whole run (the launches may overlap at their edges: the next one's first workgroups start while
 * the previous one's last drain).  Average launch time = *ms_total / iters. */
int qln_time_constraint_and_jacobian_total(qln_handle* h, const double* Z, double* c, double* vals, uint32_t flags,
                                           int32_t warmup, int32_t iters, float* ms_total);

#ifdef __cplusplus
}
#endif
#endif
