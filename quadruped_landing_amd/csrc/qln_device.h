// qln_device.h -- launch interface between the C-ABI host layer (qln_api.cpp) and
// the gfx950 kernels (qln_kernels.hip).  Internal; the public boundary is
// include/qln_evaluator.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/qln_evaluator.h"

namespace qln {

// Per-problem descriptor, one 32-byte record per problem so that a wave fetches everything it needs to
// start with ONE scalar load (k_trans / init_mode of HybridNLP, src/nlp.jl:17-19, and the output offsets).
struct alignas(32) ProblemDesc {
    int32_t k_trans;    // 1-based start index of mode 3
    int32_t init_mode;  // 1 or 2
    int64_t c_off;      // offset of the problem's constraint vector in c
    int64_t j_off;      // offset of the problem's Jacobian values in vals (even)
    int64_t reserved;
};

// Device-resident description of a batch (mirrors HybridNLP, src/nlp.jl:13-33, per problem).
struct BatchParams {
    int32_t B;
    int32_t N;
    double g, mb, mf, lb;      // PlanarQuadruped, src/planar_quadruped.jl:11-20
    const ProblemDesc* desc;   // [B]
    const double* bnd;         // [B][30]: x0 (15) then xf (15) of each problem
    const double* cost;        // [cost_batch][N][41]
    int32_t cost_batch;
    int64_t z_stride;
    int32_t jac_format;        // QLN_JAC_FORMAT_*: layout of the step-block section of vals
    int32_t kt_max;            // largest k_trans of the batch (host-side sizing of the structural format's LDS tile)
};

// The model constants the kernels compute with (PlanarQuadruped, src/planar_quadruped.jl:11-20)
struct Model {
    double g, mb, mf, lb;
    double Ib;  // mb * lb^2 / 12, src/planar_quadruped.jl:41
    __host__ __device__ __forceinline__ explicit Model(const BatchParams& P)
        : g(P.g), mb(P.mb), mf(P.mf), lb(P.lb), Ib(mb * (lb * lb) / 12) {}
    // one problem's own model: th = (g, mb, mf, lb), QLN_MODEL_NP doubles (the plant of qln_tracking_rollout_model)
    __host__ __device__ __forceinline__ explicit Model(const double* th)
        : g(th[0]), mb(th[1]), mf(th[2]), lb(th[3]), Ib(mb * (lb * lb) / 12) {}
};

// ---------------------------------------------------------------------------------------------
// Structural non-zeros of the 15x20 step Jacobian d(x+)/d[x;u] (contact*_jacobian,
// src/planar_quadruped.jl:225-248, times the jump mask of :262-263 at the transition knot).
// A knot falls into one of five categories; the pattern of each is fixed:
//   0  contact mode 1 (foot 1 pinned, foot 2 free)   71 entries
//   1  contact mode 2 (foot 2 pinned, foot 1 free)   71
//   2  mode 3 (both feet pinned)                      57
//   3  mode 1 followed by the jump map                56   (rows 5, 7, 11-15 masked; quirk Q1)
//   4  mode 2 followed by the jump map                56
// In QLN_JAC_FORMAT_STRUCTURAL the values of a block are stored in column-major order of its pattern.
// ---------------------------------------------------------------------------------------------
constexpr int kStepCategories = 5;

__host__ __device__ constexpr bool step_entry_present(int cat, int row, int col) {
    const bool f1 = (cat == 1 || cat == 4);  // foot 1 free
    const bool f2 = (cat == 0 || cat == 3);  // foot 2 free
    const bool keep = cat < 3;               // not masked by the jump
    switch (row) {
        case 0: return col == 0 || col == 7 || col == 15 || col == 17 || col == 19;
        case 1: return col == 1 || col == 8 || col == 16 || col == 18 || col == 19;
        case 2:   // theta: every position, velocity, force and h
        case 9:   // omega: the same without theta itself
            if (col == 14) return false;
            if (col == 2) return row == 2;
            if (col == 10 || col == 11) return f1;
            if (col == 12 || col == 13) return f2;
            return true;
        case 3: return col == 3 || (f1 && (col == 10 || col == 15 || col == 19));
        case 4: return keep && (col == 4 || (f1 && (col == 11 || col == 16 || col == 19)));
        case 5: return col == 5 || (f2 && (col == 12 || col == 17 || col == 19));
        case 6: return keep && (col == 6 || (f2 && (col == 13 || col == 18 || col == 19)));
        case 7: return col == 7 || col == 15 || col == 17 || col == 19;
        case 8: return col == 8 || col == 16 || col == 18 || col == 19;
        case 10: return keep && (col == 10 || (f1 && (col == 15 || col == 19)));
        case 11: return keep && (col == 11 || (f1 && (col == 16 || col == 19)));
        case 12: return keep && (col == 12 || (f2 && (col == 17 || col == 19)));
        case 13: return keep && (col == 13 || (f2 && (col == 18 || col == 19)));
        case 14: return keep && (col == 14 || col == 19);
        default: return false;
    }
}

// position of (row, col) inside the category's value list (column-major over the pattern)
__host__ __device__ constexpr int step_entry_pos(int cat, int row, int col) {
    int n = 0;
    for (int c = 0; c <= col; ++c)
        for (int r = 0; r < 15; ++r) {
            if (c == col && r == row) return n;
            if (step_entry_present(cat, r, c)) ++n;
        }
    return n;
}

__host__ __device__ constexpr int step_nnz(int cat) { return step_entry_pos(cat, 15, 19); }

// union of the five patterns (85 entries) and the position of an entry inside it (column-major)
constexpr int kStepUnion = 85;
__host__ __device__ constexpr bool step_union_present(int row, int col) {
    return step_entry_present(0, row, col) || step_entry_present(1, row, col);
}
__host__ __device__ constexpr int step_union_pos(int row, int col) {
    int n = 0;
    for (int c = 0; c <= col; ++c)
        for (int r = 0; r < 15; ++r) {
            if (c == col && r == row) return n;
            if (step_union_present(r, c)) ++n;
        }
    return n;
}
static_assert(step_union_pos(15, 19) == kStepUnion, "the union of the patterns has 85 entries");
static_assert(step_nnz(0) == 71 && step_nnz(1) == 71 && step_nnz(2) == 57 && step_nnz(3) == 56 && step_nnz(4) == 56,
              "structural non-zero counts of SURVEY.md 8.0");

// Category of dynamics knot K (1-based, 1..N-1) under the mode schedule of src/constraints.jl:23-37.
__host__ __device__ constexpr int step_category(int K, int k_trans, int init_mode) {
    return (K == k_trans - 1) ? (init_mode == 1 ? 3 : 4) : (K < k_trans - 1) ? (init_mode == 1 ? 0 : 1) : 2;
}

// The same schedule as the flags the dynamics read: which foot is free during knot K's step (mode 1 = foot 2 free,
// mode 2 = foot 1 free, mode 3 = both pinned) and whether the jump map (src/planar_quadruped.jl:250-263) follows it.
// The second argument is the jump knot k_trans - 1, subtracted by the caller: hipcc simplifies a function before it
// inlines it, and with the subtraction in here it rewrites `K <= k_trans - 1` to `K < k_trans` on its own, where the
// kernels fold it together with K = lane + 1 -- different integer code, and with it different register tables in the
// large kernels (profiles/step_block_refactor_resource_usage.txt).
struct KnotMode {
    bool f1free, f2free, jump;
    bool pinned;  // mode 3.  Not derived from the other two where it is used (the structural emission): `mode == 3` is the
                  // compare the evaluator has always made, and !(f1free || f2free) is two more in 14 of its instantiations
};
__host__ __device__ __forceinline__ constexpr KnotMode knot_mode(int K, int k_jump, int im) {
    const int mode = (K <= k_jump) ? im : 3;
    return {mode == 2, mode == 1, K == k_jump, mode == 3};
}
constexpr bool knot_mode_matches_category() {
    bool seen[kStepCategories] = {false, false, false, false, false};
    for (int im = 1; im <= 2; ++im)
        for (int kt = 1; kt <= 6; ++kt)
            for (int K = 1; K <= kt + 2; ++K) {
                const int cat = step_category(K, kt, im);
                const KnotMode m = knot_mode(K, kt - 1, im);
                seen[cat] = true;
                if (m.f1free != (cat == 1 || cat == 4) || m.f2free != (cat == 0 || cat == 3) || m.jump != (cat >= 3) ||
                    m.pinned != (cat == 2))
                    return false;
            }
    return seen[0] && seen[1] && seen[2] && seen[3] && seen[4];
}
static_assert(knot_mode_matches_category(), "knot_mode and step_category state the same schedule, in all five categories");

// Offset (doubles) of 0-based knot k's block inside the step-block section of a problem, structural format:
// contact knots first (71 each), then the jump knot (56), then mode 3 (57 each).  step_block_offset(N-1) is the
// section's length.
__host__ __device__ constexpr int step_block_offset(int k, int N, int k_trans) {
    const int nc = (k_trans - 2 < 0) ? 0 : (k_trans - 2 > N - 1 ? N - 1 : k_trans - 2);  // knots before the jump
    const int nj = (k_trans >= 2 && k_trans <= N) ? 1 : 0;
    return (k <= nc) ? 71 * k : 71 * nc + 56 * nj + 57 * (k - nc - nj);
}

// ---------------------------------------------------------------------------------------------
// Where the rows of one problem's constraint vector c are, and where the sections of its vals segment are (the "Layouts"
// comment of include/qln_evaluator.h is the public statement).  These two functions are the only statement of either in
// the library: the kernels, the size and structure queries of qln_api.cpp and the launch code take every row offset,
// every section offset and every count from them.  Both structs are returned and passed by value: one whose address is
// taken lives in scratch memory (carve() in qln_ilqr_kernels.hip).
// ---------------------------------------------------------------------------------------------

// Rows of c, 0-based (cinds of src/nlp.jl:48-63): initial state (15), terminal state (14), dynamics (15 per step),
// contact-init (N), contact-other (N - k_trans + 1), final control (1), clearance (N; the only inequality rows).
struct RowLayout {
    int o_init, o_term, o_dyn, o_ci, o_co, o_fc, o_bp, m;
};
__host__ __device__ __forceinline__ constexpr RowLayout row_layout(int N, int k_trans) {
    RowLayout r{};
    r.o_init = 0;
    r.o_term = r.o_init + 15;
    r.o_dyn = r.o_term + 14;
    r.o_ci = r.o_dyn + 15 * (N - 1);
    r.o_co = r.o_ci + N;
    r.o_fc = r.o_co + (N - k_trans + 1);
    r.o_bp = r.o_fc + 1;
    r.m = r.o_bp + N;
    return r;
}

// Sections of vals, in the write order of jac_c! (src/constraints.jl:186-274): the step blocks [0, dyn) -- 300 values per
// step, or the patterns' values in QLN_JAC_FORMAT_STRUCTURAL --, the N clearance d/dtheta entries at o_clear (with the
// step blocks the values that depend on Z: nnz_dynamic = o_const), then the constants from o_const on: I(15) of the
// initial rows (225 values), the 15 x 14 block of the terminal rows (210), the diagonal -1 of -I(n) (15 per step), the
// contact-init ones (N), the contact-other ones (N - k_trans + 1), the two final-control entries, the clearance d/dy ones (N).
struct ValsLayout {
    int dyn, o_clear, o_const, o_init, o_term, o_next, o_ci, o_co, o_fc, o_by, nnz;
};
__host__ __device__ __forceinline__ constexpr ValsLayout vals_layout(int N, int k_trans, int jac_format) {
    ValsLayout v{};
    v.dyn = (jac_format == QLN_JAC_FORMAT_STRUCTURAL) ? step_block_offset(N - 1, N, k_trans) : 300 * (N - 1);
    v.o_clear = v.dyn;
    v.o_const = v.o_clear + N;
    // The constants, counted from o_const first and in this order of summation: hipcc simplifies this function before it
    // inlines it, and with the sections summed one after the other from `dyn` on, the count of constants reaches the kernels
    // in another shape than the `i < c_ci` test of jac_const_value() -- different integer code in every instantiation that
    // writes the Jacobian (profiles/row_layout_refactor_resource_usage.txt).
    const int c_next = 15 * 15 + 15 * 14;
    const int c_ci = c_next + 15 * (N - 1);
    const int n_const = c_ci + 3 * N - k_trans + 3;
    v.o_init = v.o_const;
    v.o_term = v.o_const + 15 * 15;
    v.o_next = v.o_const + c_next;
    v.o_ci = v.o_const + c_ci;
    v.o_co = v.o_ci + N;
    v.o_fc = v.o_co + (N - k_trans + 1);
    v.o_by = v.o_fc + 2;
    v.nnz = v.o_const + n_const;
    return v;
}
// Value of constant i, counted from o_const: column-major I(15), the column-major 15 x 14 block of I(15)'s first 14 rows,
// then -1 up to o_ci and +1 behind it.
__host__ __device__ __forceinline__ constexpr double jac_const_value(const ValsLayout& L, int i) {
    const int n_init = L.o_term - L.o_const, n_term = L.o_next - L.o_const;
    if (i < n_init) return (i % 15 == i / 15) ? 1.0 : 0.0;
    if (i < n_term) return ((i - n_init) % 14 == (i - n_init) / 14) ? 1.0 : 0.0;
    if (i < L.o_ci - L.o_const) return -1.0;
    return 1.0;
}

constexpr bool layouts_match_reference() {
    for (int N : {2, 12, 40, 61, 80, 130})
        for (int kt : {1, 2, N - 1, N, N + 1}) {
            const RowLayout r = row_layout(N, kt);
            if (r.o_init != 0 || r.o_term - r.o_init != 15 || r.o_dyn - r.o_term != 14 || r.o_ci - r.o_dyn != 15 * (N - 1) ||
                r.o_co - r.o_ci != N || r.o_fc - r.o_co != N - kt + 1 || r.o_bp - r.o_fc != 1 || r.m - r.o_bp != N ||
                r.m != 18 * N - kt + 16)
                return false;
            for (int fmt : {QLN_JAC_FORMAT_DENSE_BLOCKS, QLN_JAC_FORMAT_STRUCTURAL}) {
                const ValsLayout v = vals_layout(N, kt, fmt);
                const int dyn = (fmt == QLN_JAC_FORMAT_STRUCTURAL) ? step_block_offset(N - 1, N, kt) : 300 * (N - 1);
                if (v.dyn != dyn || v.o_clear != v.dyn || v.o_const - v.o_clear != N || v.o_init != v.o_const ||
                    v.o_term - v.o_init != 225 || v.o_next - v.o_term != 210 || v.o_ci - v.o_next != 15 * (N - 1) ||
                    v.o_co - v.o_ci != N || v.o_fc - v.o_co != N - kt + 1 || v.o_by - v.o_fc != 2 || v.nnz - v.o_by != N ||
                    v.nnz != dyn + 435 + 15 * (N - 1) + 4 * N - kt + 3)
                    return false;
                // first and last constant of each kind: the two identity blocks (column-major), the -1 of -I(n), the ones
                const int c_ci = v.o_ci - v.o_const, n_const = v.nnz - v.o_const;
                if (jac_const_value(v, 0) != 1.0 || jac_const_value(v, 1) != 0.0 || jac_const_value(v, 224) != 1.0 ||
                    jac_const_value(v, 225) != 1.0 || jac_const_value(v, 226) != 0.0 || jac_const_value(v, 225 + 13 * 14 + 13) != 1.0 ||
                    jac_const_value(v, 434) != 0.0 || jac_const_value(v, 435) != -1.0 || jac_const_value(v, c_ci - 1) != -1.0 ||
                    jac_const_value(v, c_ci) != 1.0 || jac_const_value(v, n_const - 1) != 1.0)
                    return false;
            }
        }
    return true;
}
static_assert(layouts_match_reference(), "group lengths of cinds (src/nlp.jl:48-63) and section lengths of jac_c!'s write order");
constexpr bool notebook_ranges_match() {  // N = 61, k_trans = 21: the 1-based ranges of the notebook's problem (src/main.ipynb)
    const RowLayout r = row_layout(61, 21);
    return r.o_init == 0 && r.o_term == 15 && r.o_dyn == 29 && r.o_ci == 929 && r.o_co == 990 && r.o_fc == 1031 && r.o_bp == 1032 &&
           r.m == 1093;
}
static_assert(notebook_ranges_match(), "(1,15) (16,29) (30,929) (930,990) (991,1031) (1032,1032) (1033,1093)");

// internal launch flag (bit 0 is QLN_JAC_WRITE_CONSTANTS): prefer latency over throughput for a small batch
constexpr uint32_t kLaunchSplit = 2u;
// L2 prefetch for a later workgroup of the XCD (k_constraint_jacobian): distance in problems in bits 8..28 of the flags (0 = off),
// what is prefetched in bits 29..31 (default: the slice of Z only)
constexpr uint32_t kDensePrefetchAhead = 64;
constexpr uint32_t kPrefetchNoZ = 1u << 29, kPrefetchBnd = 1u << 30, kPrefetchDesc = 1u << 31;

// Fused eval_c! + jac_c! over problems [b_begin, b_begin + nb).  c or vals may be null.
hipError_t launch_constraint_jacobian(const BatchParams& p, int32_t b_begin, int32_t nb, const double* Z, double* c,
                                      double* vals, uint32_t flags, hipStream_t stream);
hipError_t launch_eval_all(const BatchParams& p, const double* Z, double* f, double* grad, double* c, double* vals, uint32_t flags,
                           hipStream_t stream);
hipError_t launch_objective_and_constraint(const BatchParams& p, const double* Z, double* f, double* c, hipStream_t stream);
hipError_t launch_kinematic_rows(const BatchParams& p, const double* Z, double* d, double* jac_vals, hipStream_t stream);
hipError_t launch_friction_rows(const BatchParams& p, const double* Z, double mu, double* d, double* jac_vals, hipStream_t stream);
hipError_t launch_jacobian_constants(const BatchParams& p, double* vals, hipStream_t stream);
hipError_t launch_objective(const BatchParams& p, const double* Z, double* f, hipStream_t stream);
hipError_t launch_objective_gradient(const BatchParams& p, const double* Z, double* grad, hipStream_t stream);
hipError_t launch_initial_guess(const BatchParams& p, double* Z, hipStream_t stream);
hipError_t launch_constraint_violation(const BatchParams& p, const double* c, double* viol, hipStream_t stream);
// y = J(Z) v and g = J(Z)^T lam with the constraint Jacobian re-derived in registers (qln_solver_kernels.hip)
hipError_t launch_constraint_jvp(const BatchParams& p, const double* Z, const double* v, double* y, hipStream_t stream);
hipError_t launch_constraint_vjp(const BatchParams& p, const double* Z, const double* lam, double* g, hipStream_t stream);
// H = sigma d2 f + sum mu_i d2 c_i, the 55 + 15 values per knot of qln_hessian.h's pattern (qln_hessian_kernels.hip)
hipError_t launch_hessian_lagrangian(const BatchParams& p, const double* Z, const double* sigma, const double* mu, double* hvals,
                                     int64_t h_stride, hipStream_t stream);
// y = H v with the same H, contracted in registers (qln_hessian_kernels.hip); v and y in the layout of Z
hipError_t launch_hessian_lagrangian_product(const BatchParams& p, const double* Z, const double* sigma, const double* mu,
                                             const double* v, double* y, hipStream_t stream);
// TVLQR gains (and cost-to-go, P may be null) along the reference trajectories Zref (qln_tracking_kernels.hip).  Qd / Rd / Qfd
// are host arrays.  event (null: the handle's knot schedule and model): the guarded roll-out's records, whose knot and tau the
// sweep through the touchdown reads (qln_tracking_lqr_guarded), with model [B][QLN_MODEL_NP] (null: the handle's).
// sat [B][N-1] (null: none): the limited roll-out's saturation codes, whose channels' columns of B_k are zero
// (qln_tracking_lqr_limited); the sweeps below take it the same way, and the roll-out writes it (null: not written) when lim, a
// host array of QLN_FORCE_LIMITS_N doubles, is given (qln_tracking_rollout_limited).
hipError_t launch_tracking_lqr(const BatchParams& p, const double* Qd, const double* Rd, const double* Qfd, const double* Zref,
                               const double* model, const double* event, const double* sat, double* K, double* P,
                               hipStream_t stream);
// The roll-out from x0 (null: the handle's x0) and its two sweeps at Zout's trajectory, with a per-problem plant: model
// [B][QLN_MODEL_NP] = (g, mb, mf, lb) per problem (null: the handle's), its tangent model_dot and cotangent model_bar in the same
// layout.  Reverse: cotangent Zbar -> Zref_bar, K_bar, x0_bar, model_bar (each may be null).  Forward: tangents Zref_dot, K_dot,
// x0_dot, model_dot (each may be null: zero) -> Zout_dot in the layout of Z.  K_bar and K_dot need K and read Zref's states.
// With nothing of the model passed the kernels run without their kModel flag (qln_tracking_kernels.hip).
// guarded: touchdown by the free foot's height instead of the knot schedule; event [B][QLN_TOUCHDOWN_INFO_STRIDE] or null
hipError_t launch_tracking_rollout(const BatchParams& p, const double* Zref, const double* K, const double* x0,
                                   const double* model, double* Zout, bool guarded, double* event, const double* lim,
                                   double* sat, hipStream_t stream);
// event (null: the knot-scheduled sweeps): the guarded roll-out's records, whose knot and tau the sweeps through the
// touchdown read (qln_tracking_rollout_guarded_vjp / _jvp); event_dot [B][QLN_TOUCHDOWN_INFO_STRIDE] or null, with event only.
hipError_t launch_tracking_rollout_vjp(const BatchParams& p, const double* Zref, const double* K, const double* Zout,
                                       const double* model, const double* event, const double* sat, const double* Zbar,
                                       double* Zref_bar, double* K_bar, double* x0_bar, double* model_bar, hipStream_t stream);
hipError_t launch_tracking_rollout_jvp(const BatchParams& p, const double* Zref, const double* K, const double* Zout,
                                       const double* model, const double* event, const double* sat, const double* Zref_dot,
                                       const double* K_dot, const double* x0_dot, const double* model_dot, double* Zout_dot,
                                       double* event_dot, hipStream_t stream);
// Sigma_{k+1} = (A_k - B_k K_k) Sigma_k (A_k - B_k K_k)' + diag(Wd) along Zout (K null: open loop); Sigma0 [sigma0_batch][120],
// Wd a host array (null: zeros); Sigma [B][N][120] and marg [B][N][8], either may be null (qln_tracking_kernels.hip).
// event and model as for launch_tracking_lqr (qln_tracking_covariance_guarded); event_var [B][2] or null, with event only.
hipError_t launch_tracking_covariance(const BatchParams& p, const double* Zout, const double* K, const double* model,
                                      const double* event, const double* Sigma0, int sigma0_batch, const double* Wd,
                                      double* Sigma, double* marg, double* event_var, hipStream_t stream);
// The Kalman filter and the LQG covariance along Zout (qln_tracking_kalman / _guarded): H [ny][15] on the device, Vd (ny) and Wd
// (15 or null) host arrays; Lgain [B][N][15][ny], Pest, Sigma [B][N][120], marg [B][N][8], event_var [B][2], each may be null;
// K null: the filter alone (Lgain and Pest only).  model and event as for launch_tracking_covariance.
hipError_t launch_tracking_kalman(const BatchParams& p, const double* Zout, const double* K, const double* model,
                                  const double* event, const double* H, int ny, const double* Vd, const double* Sigma0,
                                  int sigma0_batch, const double* Wd, double* Lgain, double* Pest, double* Sigma, double* marg,
                                  double* event_var, hipStream_t stream);
// The forward sweep through the Kalman design (qln_kalman_design_jvp / _guarded) at the gains it returned: Lgain
// [B][N][15][ny] and H [ny][15] on the device, Vd (ny) a host array; the direction: Sigma0_dot [sigma0_batch][120] on the device or
// null, Wd_dot (15) and Vd_dot (ny) host arrays or null (zeros); Lgain_dot [B][N][15][ny], Pest_dot [B][N][120] and logdet_dot
// [B][N], each may be null, not all.  event selects the guarded blocks, and model is read with it only.
hipError_t launch_tracking_kalman_jvp(const BatchParams& p, const double* Zout, const double* model, const double* event,
                                      const double* Lgain, const double* H, int ny, const double* Vd, const double* Sigma0_dot,
                                      int sigma0_batch, const double* Wd_dot, const double* Vd_dot, double* Lgain_dot,
                                      double* Pest_dot, double* logdet_dot, hipStream_t stream);
// The reverse sweep through the Kalman design (qln_noise_design_vjp / _guarded_vjp), the transpose of the forward
// sweep's map at the same gains: Lgain [B][N][15][ny] and H [ny][15] on the device, Vd (ny) a host array; the cotangents Lgain_bar
// [B][N][15][ny], Pest_bar [B][N][120] and logdet_bar [B][N] on the device, each may be null (zeros), not all; Sigma0_bar [B][120],
// Wdiag_bar [B][15] and Vdiag_bar [B][ny] on the device, each may be null, not all.  event selects the guarded blocks, and model
// is read with it only.
hipError_t launch_tracking_kalman_vjp(const BatchParams& p, const double* Zout, const double* model, const double* event,
                                      const double* Lgain, const double* H, int ny, const double* Vd, const double* Lgain_bar,
                                      const double* Pest_bar, const double* logdet_bar, double* Sigma0_bar, double* Wdiag_bar,
                                      double* Vdiag_bar, hipStream_t stream);
// The fixed-interval smoother of a flown landing (qln_landing_smoother / _guarded): Lgain [B][N][15][ny], Pest [B][N][120],
// H [ny][15], Xhat [B][N][15] and innov [B][N][ny] on the device, Vd (ny) a host array; Xs [B][N][15] and Ps [B][N][120], either
// may be null.  event selects the guarded blocks, and model is read with it only.
hipError_t launch_landing_smoother(const BatchParams& p, const double* Ztraj, const double* model, const double* event,
                                   const double* Lgain, const double* Pest, const double* H, int ny, const double* Vd,
                                   const double* Xhat, const double* innov, double* Xs, double* Ps, hipStream_t stream);
// The filter on recorded data (qln_landing_filter / _guarded): Zref (state slots read), Zrec (control slots read), Lgain
// [B][N][15][ny], H [ny][15] and Y [B][N][ny] on the device, Vd (ny) a host array read only when score or loglik is asked for;
// xhat0 [B][15] may be null; model [B][QLN_MODEL_NP] (null: the handle's) is the model of each record's own
// (qln_landing_filter_model); Xhat [B][N][15], innov [B][N][ny], score [B][N][2], loglik [B] and event_hat
// [B][QLN_TOUCHDOWN_INFO_STRIDE] (guarded only) may each be null, not all.
hipError_t launch_landing_filter(const BatchParams& p, const double* Zref, const double* Zrec, const double* Lgain, const double* H,
                                 int ny, const double* Vd, const double* Y, const double* xhat0, const double* model, double* Xhat,
                                 double* innov, double* score, double* loglik, bool guarded, double* event_hat,
                                 hipStream_t stream);
// The sweeps through the filter (qln_landing_filter_jvp / _vjp) at the record and the trajectory the filter
// produced: Zrec (control slots read), Lgain, H, model (null: the handle's), Xhat; innov with a tangent or cotangent of Lgain or
// a score term; event_hat (entries 0 and 1 read) selects the guarded blocks.  iv: 1 / V of the score terms (host; V = 1 behind ny).
struct FilterSweepIn {
    const double *Zrec, *Lgain, *H;
    int ny;
    const double *model, *Xhat, *innov, *event_hat;
    double iv[QLN_TRACK_NY_MAX];
};
// the tangents (null: zero) and the forward sweep's outputs (each may be null, not all)
struct FilterJvpArgs {
    const double *Y_dot, *Zrec_dot, *Lgain_dot, *xhat0_dot, *model_dot;
    double *Xhat_dot, *innov_dot, *nis_dot, *loglik_dot, *event_hat_dot;
};
// the cotangents (null: zero) and the reverse sweep's outputs (each may be null, not all)
struct FilterVjpArgs {
    const double *Xhat_bar, *innov_bar, *nis_bar, *loglik_bar;
    double *Y_bar, *Zrec_bar, *Lgain_bar, *xhat0_bar, *model_bar;
};
hipError_t launch_landing_filter_jvp(const BatchParams& p, const FilterSweepIn& in, const FilterJvpArgs& a, hipStream_t stream);
hipError_t launch_landing_filter_vjp(const BatchParams& p, const FilterSweepIn& in, const FilterVjpArgs& a, hipStream_t stream);
// The roll-out of the plant and the estimator side by side (qln_tracking_rollout_estimated / _guarded): Lgain [B][N][15][ny] and
// H [ny][15] on the device; vnoise [B][N][ny], wnoise [B][N-1][15], x0, xhat0 [B][15], model and K may be null; Xhat [B][N][15],
// innov [B][N][ny] may be null; event and event_hat [B][QLN_TOUCHDOWN_INFO_STRIDE] or null, with guarded only.
// lim (null: none), a host array of QLN_FORCE_LIMITS_N doubles: the applied forces are clamped by the plant's contact mode
// (qln_tracking_rollout_estimated_limited), and sat [B][N-1] (null: not written; with lim only) gets the saturation codes.
hipError_t launch_tracking_rollout_estimated(const BatchParams& p, const double* Zref, const double* K, const double* Lgain,
                                             const double* H, int ny, const double* vnoise, const double* wnoise,
                                             const double* x0, const double* xhat0, const double* model, double* Zout,
                                             double* Xhat, double* innov, bool guarded, double* event, double* event_hat,
                                             const double* lim, double* sat, hipStream_t stream);
// The sweeps through the estimate-feedback roll-out (qln_tracking_rollout_estimated_jvp / _vjp, qln_tracking_kernels.hip).  What
// both read: the roll-out's inputs and the trajectory it produced; event and event_hat (both or neither) select the guarded
// blocks.  innov is read only with a tangent or cotangent of Lgain.
struct EstimatedSweepIn {
    const double *Zref, *K, *Lgain, *H;
    int ny;
    const double *model, *Zout, *Xhat, *innov, *event, *event_hat;
};
// the tangents (null: zero; xhat0_dot null: x_ref_dot,0) and the forward sweep's outputs (all but Zout_dot may be null)
struct EstimatedJvpArgs {
    const double *Zref_dot, *K_dot, *Lgain_dot, *x0_dot, *xhat0_dot, *model_dot;
    double *Zout_dot, *Xhat_dot, *innov_dot, *event_dot, *event_hat_dot;
};
// the cotangents (Xhat_bar, innov_bar null: zero) and the reverse sweep's outputs (each may be null; xhat0_bar null: the
// cotangent of xhat^-_0 is added to Zref_bar's x_0 slot)
struct EstimatedVjpArgs {
    const double *Zbar, *Xhat_bar, *innov_bar;
    double *Zref_bar, *K_bar, *Lgain_bar, *x0_bar, *xhat0_bar, *model_bar;
};
// sat [B][N-1] (null: none): the limited roll-out's saturation codes, which select the sweeps at that active set
// (qln_tracking_rollout_estimated_limited_jvp / _vjp)
hipError_t launch_tracking_rollout_estimated_jvp(const BatchParams& p, const EstimatedSweepIn& in, const EstimatedJvpArgs& a,
                                                 const double* sat, hipStream_t stream);
hipError_t launch_tracking_rollout_estimated_vjp(const BatchParams& p, const EstimatedSweepIn& in, const EstimatedVjpArgs& a,
                                                 const double* sat, hipStream_t stream);
// batched Gauss-Newton step on the constraint violation, CGLS per problem in LDS (qln_solver_kernels.hip)
size_t gauss_newton_lds_bytes(int32_t N);
hipError_t launch_gauss_newton_step(const BatchParams& p, const double* Z, const double* c, double* dZ, int max_iters,
                                    double rel_tol, const double* radius, const double* col_scale, double* info,
                                    hipStream_t stream);
// least-squares multiplier estimate and KKT report, CGLS per problem in LDS (qln_solver_kernels.hip)
struct MultiplierParams {
    double th_lo, th_hi, h_lo, h_hi;  // bounds on theta (every knot) and h (every dynamics knot), src/moi.jl:54-61
    int q6;                           // quirk Q6's lower bounds 0 on yb_{k+1}, x1_{k+1} (src/moi.jl:64-65)
    double act_tol, bound_tol;        // bound_tol < 0: no variable is fixed
    int row_scaling, max_iters;
    double rel_tol;
};
size_t multiplier_lds_bytes(int32_t N);
hipError_t launch_estimate_multipliers(const BatchParams& p, const MultiplierParams& mp, const double* Z, const double* c,
                                       const double* g, double* lam, double* lag, double* info, hipStream_t stream);
// device-side generator of the synthetic workload (qln_sampler_kernels.hip)
struct DropStateSampler {
    unsigned long long state_hi, state_lo, inc_hi, inc_lo;  // numpy.random.PCG64(seed).state
    long long stream_offset;                                // draws of the stream consumed before this call
    double x0_template[15];
    double lo[4], range[4];                                 // theta0 [deg], y2_0, drop height H, omega0: low and high - low
    double deg2rad, two_g;
};
hipError_t launch_sample_drop_states(const BatchParams& p, const DropStateSampler& s, double* bnd, hipStream_t stream);
hipError_t launch_bounded_integers(const DropStateSampler& s, uint32_t range, int32_t low, int64_t count, int32_t* out,
                                   unsigned long long* rejected, hipStream_t stream);
hipError_t launch_perturb_point(const BatchParams& p, const DropStateSampler& s, double* Z, double sigma, double h_lo, double h_hi,
                                int redraw_h, hipStream_t stream);
// batched augmented-Lagrangian iLQR solve of the reference NLP (qln_ilqr_kernels.hip)
struct SolveParams {
    int32_t max_outer, max_inner;
    double tol, inner_tol;
    double rho0, rho_factor, rho_max;
    double mu0, mu_min, mu_max;
    double h_lo, h_hi, th_lo, th_hi;
    double h_prox;  // proximal weight on the step lengths in Quu: without the d(h l)/dh term (quirk Q2) the objective does
                    // not see h at all, the h_k are then fixed by the constraints alone and wander along flat directions
    int32_t q6, exact_h;
    int32_t rescue_outer;  // extra multiplier updates with accurate inner solves for problems the schedule did not finish
};
size_t ilqr_lds_bytes(int32_t N);
size_t ilqr_scratch_doubles(int32_t B, int32_t N);
hipError_t launch_al_ilqr(const BatchParams& p, const SolveParams& s, double* Z, double* info, double* scratch,
                          hipStream_t stream);
hipError_t launch_lqr_cost(const BatchParams& p, const double* qrqf, double dt, double* cost, int cost_batch,
                           hipStream_t stream);

}  // namespace qln
