// qln_tracking_kernels.hip -- time-varying LQR tracking along a batch of reference trajectories (qln_tracking_lqr) and the
// closed-loop roll-out of the nonlinear hybrid system under the gains (qln_tracking_rollout).  Semantics: the comment
// above the declarations in include/qln_evaluator.h.
//
// k_tracking_lqr: the backward Riccati sweep is serial in the knots, so the parallelism is across problems and inside a
// knot's 15x15 products.  One problem per row of sixteen lanes, four problems per wave; lane j < 15 keeps row j of
// P_{k+1} (= column j) in registers, lane 15 shadows lane 14 and stores nothing.  A_k, B_k are the evaluator's closed
// form (step_block / for_each_step_entry), formed for the knot by every lane of the row alike from the reference's
// (x_k, u_k): what a lane needs at compile-time positions (every column of A for T = P A, every column of B for
// S = P B and B'S) is in registers, what it needs at its own runtime position (column j of A for A'T, column j of Qux)
// comes from a per-row LDS table in the compact four-entries-per-column form of the solver's sweep (a_slot of
// qln_row16.h): A(c,c), A(2,c), A(9,c) and the position <- velocity coupling A(c-7,c).
// Per knot, three LDS hand-offs inside the wave (no s_barrier, wave_lds_sync):
//   1. T row j = P row j . A (60 FMAs, structure known at compile time), S row j = P row j . B (24) -> LDS;
//   2. Qxx row j = A'T (rows 2, 9, j-7 of T from LDS), Quu = R + B'S (every lane, all of S from LDS), Qux column j;
//      Quu = L D L' (every lane alike), K column j = Quu^-1 Qux column j -> the K tile in LDS;
//   3. P_k row j, entries c <= j, = Q + Qxx - Qux'K -> the packed lower-triangle tile; every lane reads its full row back
//      from the tile, so P is exactly symmetric, and the K and P tiles leave as coalesced stores (sixteen lanes, 128 B).
// Every kernel here that needs the roll-out's A_k, B_k takes them from for_each_rollout_entry (qln_kernel_common.h): the
// evaluator's block with the jump map's clock row.  The mapping, the DPP moves and the knot's load / store are qln_row16.h's.
//
// k_tracking_rollout: one lane per problem, the solver's step_forward (qln_kernel_common.h) on the fed-back forces.  With
// the flag kGuard (qln_tracking_rollout_guarded) the contact mode is the lane's own state instead of the
// handle's knot schedule: touchdown happens in the step in which the free foot reaches the ground, located in closed form.
//
// k_tracking_rollout_vjp: the reverse sweep of the roll-out.  One problem per row of sixteen lanes, as
// k_tracking_lqr; lane j < 15 owns lam[j], column j of A_k, row j of B_k and of the h column, and column j of K and K_bar;
// lane 15 holds lam = 0 and only stores a u slot.  Nothing goes through LDS:
//   (A'lam)[j] needs lam at rows j, 2, 9 and j-7 -- two DPP row broadcasts and one row shift;
//   B'lam and the h column are row sums (four DPP steps each).  Rows 2 and 9 (theta, omega) are dense in B and h, but
//   bilinear in (positions, forces): their share of B'lam is folded into the row sums as lane j's x_j times a sign pattern
//   (d tau / d x_j d F_m), so no lane forms a whole row;
//   K_k'ubar and K_bar = -ubar dx' are four FMAs / four products per lane on column j, stored coalesced.
// The knot's slices (x_k, u_k, Zbar, x_ref and K column j) are loaded one knot ahead.
//
// k_tracking_covariance: the forward sweep Sigma_{k+1} = Acl_k Sigma_k Acl_k' + diag(W), Acl_k = A_k - B_k K_k (DESIGN.md
// 4.13).  The mapping of k_tracking_lqr: one problem per row of sixteen lanes, lane j < 15 keeps column j of Sigma_k
// (= row j) in registers, and every lane forms the knot's StepBlock alike.  No dense Acl: a lane applies Acl to a vector v as
// A v - B (K v) -- the visitor's entries of A (four per column) and of B (24) at compile-time positions, K read row by row
// from a per-row LDS tile -- and the knot is two such applications with a transpose between them, Sigma' = Acl (Acl Sigma)':
//   1. V column j = Acl Sigma column j -> row j of the padded image (stride 17) in LDS; g = K Sigma column j on the way,
//      whose row sums against K column j are the force variances (diag of M = G K');
//   2. lane j reads row j of V back (consecutive addresses) and forms column j of Sigma' = Acl V row j' + W_j e_j, stored
//      as row j of the image.  From there on only the image's lower triangle is read -- by the lanes for their next column,
//      by the marginals and by the packed tile's coalesced stores -- so every Sigma_k is exactly symmetric.
// Expanded, that is A Sigma A' - (A G')B' - B (G A') + B M B' with G = K Sigma and M = G K', grouped so that nothing but
// K v crosses lanes.  Zout's knot (two coalesced loads, handed out through LDS) and the K tile are loaded one knot ahead;
// the clearance row's cosine is taken for sixteen knots at a time, one per lane.
// The image is stated in qln_image15.h, for this sweep and k_tracking_kalman (k_landing_smoother takes the stride and sym_at
// from it and keeps its own knot, for its launch time): its stride and triangle
// (sym_at, Image15), the packed, K and gain tiles in and out (tile_fill / tile_store), the dense chains on broadcast reads with
// their rows-in-flight fence (chain_rows), the knot's two applications with the transpose between them (congruence) and the
// marginals (marginals_store).  Here stay the kernels' LDS layouts, the operators (cov_apply, cov_apply_touchdown,
// block_apply_t) and what reads a guarded record: guard_event, touchdown_block_at, touchdown_time_forms.
//
// k_tracking_rollout_jvp: the forward (tangent) sweep of the roll-out, the adjoint of the reverse sweep in
// its mapping: one problem per row of sixteen lanes, lane j < 15 owns dx[j], row j of [A_k B_k] and column j of K and Kdot;
// nothing goes through LDS.  Every lane forms the knot's StepBlock (Zout's knot: two coalesced loads, handed round by DPP
// row broadcasts) and picks its row's entries from the visitor; (A dx)[j] is the diagonal, the coupling A(j, j+7) through a
// row shift, and for the dense rows 2 and 9 two row sums; K (dx - xref_dot) + Kdot e is four more.
//
// The roll-out and its two sweeps also exist with a per-problem plant (qln_tracking_rollout_model and its _jvp / _vjp, DESIGN.md
// 4.16): the same three kernels with the flag kModel, which read the problem's (g, mb, mf, lb) instead of the handle's and add
// the term of G_k = d Phi_k / d model (ModelBlock / for_each_model_entry of qln_kernel_common.h) in the mapping they have.
//
// The two sweeps also exist through the guarded roll-out's touchdown (qln_tracking_rollout_guarded_jvp / _vjp): the
// flag kGuard, on the kModel path only.  The modes come from the problem's touchdown knot in the event record, and that knot
// takes the composite step's derivative: the row / column of [A B G] applied twice (jvp_apply_row, vjp_apply_column), at
// (x_k, tau) in the flight mode and at (x+, h - tau) in mode 3, the jump map's zeros between them and the derivative of tau,
// which scales with one over the foot's vertical velocity at the touchdown.
//
// The Riccati and the covariance sweep exist through that touchdown too (qln_tracking_lqr_guarded, qln_tracking_covariance_guarded,
// DESIGN.md 4.19): the flags kModel and kGuard on k_tracking_lqr and k_tracking_covariance.  Their lanes hold whole 15-vectors,
// so the touchdown knot's composite block is applied to them as an operator, stated once (TouchdownBlock, touchdown_apply,
// touchdown_apply_t): forward in the covariance sweep, transposed in the Riccati sweep.
//
// The roll-out, its two sweeps and the Riccati sweep also exist with contact-aware force limits (qln_tracking_rollout_limited and
// its _jvp / _vjp, qln_tracking_lqr_limited): the flag kLimit.  The roll-out clamps the applied forces by the
// foot's contact state and records the channels that rode a limit; the sweeps and the Riccati sweep read that record and treat
// those channels as constants (no tangent, no cotangent, a zero column of B_k).
//
// k_tracking_kalman: the Kalman filter along Zout and the covariance of the loop that feeds back its estimate
// (qln_tracking_kalman / _guarded), in k_tracking_covariance's mapping and on its blocks, operator and
// applications (cov_apply, cov_apply_touchdown): per knot a measurement update of the error covariance P -- H P by chains on
// broadcast LDS reads, S = H P H' + V by row sums, an 8 x 8 L D L' in every lane, the Joseph form through the image -- and two
// predictions, P's open loop and the estimate covariance M's closed loop, each a congruence step in an image of its own.
//
// k_tracking_rollout_estimated: the loop that filter designs, flown (qln_tracking_rollout_estimated / _guarded):
// the plant and the estimator rolled out side by side in k_tracking_rollout's mapping, one lane per problem, on its step and its
// guarded step, the forces fed back from the estimate and the noise read from the caller's samples.
//
// k_tracking_rollout_estimated_jvp / _vjp: the forward and reverse sweeps through that loop at fixed noise samples
// (qln_tracking_rollout_estimated_jvp / _vjp and their _guarded forms), on the row-of-sixteen mapping of the
// roll-out's own sweeps: a problem's two chains, the plant's along Zout and the estimator's along Xhat, each through
// jvp_apply_row / vjp_apply_column, coupled by the measurement update (H from LDS, row j of L_k and column j of K_k per lane).
//
// These three also exist with the flag kLimit (qln_tracking_rollout_estimated_limited and its _jvp / _vjp): the
// forces fed back from the estimate are clamped by the PLANT's contact state before the plant, the estimator or Zout read them,
// and the two sweeps treat the channels of that record as constants in both chains.
//
// k_landing_smoother: the fixed-interval smoother of a flown landing (qln_landing_smoother / _guarded), the
// estimator's backward pass: the modified Bryson-Frazier sweep on the filter's gains and covariances, in k_tracking_kalman's
// mapping and tiles, with the blocks and the touchdown operator applied transposed as the Riccati sweep applies them.
//
// k_tracking_kalman_jvp: the forward sweep through k_tracking_kalman's design (qln_kalman_design_jvp / _guarded_jvp, DESIGN.md
// 4.28): the tangents of the gains, of P^+ and of log det S_k along (Sigma0_dot, W_dot, V_dot), at the gains alone, in that
// kernel's mapping, on its blocks and on k_tracking_covariance's open-loop knot.
//
// k_tracking_kalman_vjp: the reverse sweep through that design (qln_noise_design_vjp / _guarded_vjp): the transpose
// of k_tracking_kalman_jvp's map between the arrays as stored, cotangents of the gains, of P^+ and of log det S_k in, those of
// (Sigma0, W, V) per problem out, in the same mapping, on the smoother's transposed applications (block_apply_t, touchdown_apply_t).
//
// k_landing_filter: the estimator on recorded data (qln_landing_filter / _guarded): the estimator's half of
// k_tracking_rollout_estimated, measurements and applied forces read where that kernel forms them, and with kScore the
// normalised innovation squared, log det S_k and the log-likelihood from the gains alone.  kModel: at a model of each record's own.
//
// k_landing_filter_jvp / k_landing_filter_vjp: the sweeps through that filter and its score at fixed gains
// (qln_landing_filter_jvp / _vjp): the estimator's half of k_tracking_rollout_estimated_jvp / _vjp in their row
// mapping and on their step functions, with a model tangent on that half.
#include "qln_image15.h"

#include <utility>

namespace qln {
namespace {

// per-row LDS image (doubles): compact A table [16][4] | T [15][16] | S [15][4] | K tile [4][15] | packed P [120]; the
// sections behind T are placed in the kernel (the guarded sweep's T has a row stride of kLTGuard)
constexpr int kLAC = 0, kLT = 64, kLTGuard = 17;

// bit s of a_slots(c): slot s of column c can be non-zero in some mode; bit r of b_rows_mask(m): B(r, m) can be
__host__ __device__ constexpr unsigned a_slots(int c) {
    unsigned m = 0;
    for (int r = 0; r < 15; ++r)
        if (step_union_present(r, c)) m |= 1u << a_slot(r, c);
    return m;
}
__host__ __device__ constexpr unsigned b_rows_mask(int m) {
    unsigned s = 0;
    for (int r = 0; r < 15; ++r)
        if (step_union_present(r, 15 + m)) s |= 1u << r;
    return s;
}

// The model a problem's roll-out and sweeps compute with: the handle's, or (kModel, model given) the problem's own four
// doubles, Ib formed as Model's constructor forms it.  Chosen scalar by scalar and constructed once: a Model selected between
// two whole structs was laid out in scratch memory (profiles/rollout_model_resource_usage.txt).
template <bool kModel>
__device__ __forceinline__ Model plant_model(const BatchParams& P, const double* __restrict__ model, int b) {
    double th[QLN_MODEL_NP] = {P.g, P.mb, P.mf, P.lb};
    if constexpr (kModel) {
        if (model) {
#pragma unroll
            for (int p = 0; p < QLN_MODEL_NP; ++p) th[p] = model[(int64_t)QLN_MODEL_NP * b + p];
        }
    }
    return Model(th);
}

// The contact mode of knot k in a guarded roll-out whose touchdown knot is ks (< 0: none): the problem's init_mode up to and
// including ks (the flight leg of the touchdown knot), mode 3 behind it.  No knot carries the jump in its block: the sweeps
// apply the jump map between the two legs of the touchdown knot themselves.
__device__ __forceinline__ KnotMode guard_mode(int k, int ks, int im) {
    const int mode = (ks < 0 || k <= ks) ? im : 3;
    return {mode == 2, mode == 1, false, mode == 3};
}
// a problem's touchdown knot from its event record: anything that is not a knot of the roll-out means none
__device__ __forceinline__ int guard_knot(double knot, int N) { return (knot >= 0.0 && knot <= (double)(N - 2)) ? (int)knot : -1; }

// The composite step of a guarded roll-out's touchdown knot as a linear operator, for the lanes that hold a
// whole 15-vector: the Riccati and the covariance sweep through the touchdown (qln_tracking_lqr_guarded,
// qln_tracking_covariance_guarded).  In the notation of k_tracking_rollout_jvp: [A_m B_m b_m] is the flight mode's block at
// (x_k, F, tau), [A_3 B_3 b_3] the mode-3 block at (x+, F, h - tau), J zeroes the entries the jump map zeroes, and
// d tau = t_x . dx + t_F . dF has three coefficients: on the free foot's height and vertical velocity and on its F_y (all zero
// where the guard's first branch was taken, tau = 0).  Step lengths are not perturbed (dh = 0).  [A* B*] is not sparse in the
// four-slots-per-column pattern; it is two sparse blocks, six zeros and a rank-one term, and is applied as such.
struct TouchdownBlock {
    double x[14], xp[14];  // x_k and x+ = J x-, without their clocks
    double F1x, F1y, F2x, F2y;
    double tau, rest;      // the two legs' lengths: tau and h - tau
    KnotMode md;           // the flight leg's mode
    double ty, tv, tF;     // d tau's coefficients on dx[iy], dx[iv] and the free foot's dF_y
};

// x- and x+ are recomputed with step_mode exactly as the roll-out and its sweeps form them; xk's clock feeds nothing.
__device__ __forceinline__ TouchdownBlock touchdown_block(const Model& M, const KnotMode md, double tau, const double (&xk)[15],
                                                          const double (&u)[5]) {
    TouchdownBlock T;
    double xm[15];
    step_mode(M, md, tau, xk, u, xm);
    const double y = md.f2free ? xk[6] : xk[4], w = md.f2free ? xm[13] : xm[11];
    jump_map(xm);
#pragma unroll
    for (int i = 0; i < 14; ++i) {
        T.x[i] = xk[i];
        T.xp[i] = xm[i];
    }
    T.F1x = u[0], T.F1y = u[1], T.F2x = u[2], T.F2y = u[3];
    T.tau = tau, T.rest = u[4] - tau;
    T.md = md;
    // d tau = -(dy + tau dv + tau^2/2 da) / w with da = -dF_y / mf, w the foot's vertical velocity in x-
    const double iw = (y <= 0.0) ? 0.0 : -1.0 / w;
    T.ty = iw;
    T.tv = tau * iw;
    T.tF = -(0.5 * tau * tau) * iw / M.mf;
    return T;
}
// touchdown_block on a knot's twenty entries (x_k, u_k) in LDS
__device__ __forceinline__ TouchdownBlock touchdown_block_at(const double* z, const Model& M, const KnotMode md, double tau) {
    double xk[15];
#pragma unroll
    for (int i = 0; i < 14; ++i) xk[i] = z[i];
    xk[14] = 0.0;  // the clock feeds nothing
    const double u5[5] = {z[15], z[16], z[17], z[18], z[19]};
    return touchdown_block(M, md, tau, xk, u5);
}
// a problem's touchdown knot and tau from its event record; without kGuard nothing is read and there is no such knot
struct GuardEvent {
    int ks;
    double tau;
};
template <bool kGuard>
__device__ __forceinline__ GuardEvent guard_event(const double* __restrict__ event, int bc, int N) {
    if constexpr (kGuard) return {guard_knot(event[(int64_t)QLN_TOUCHDOWN_INFO_STRIDE * bc], N), event[(int64_t)QLN_TOUCHDOWN_INFO_STRIDE * bc + 1]};
    else return {-1, 0.0};
}
// The two legs' blocks are formed where an application uses them, one after the other, from the leg's length passed through
// an empty asm: what stays live between a knot's applications is the TouchdownBlock, not two StepBlocks of fifty values.
__device__ __forceinline__ StepBlock touchdown_flight_block(const TouchdownBlock& T, const Model& M) {
    double h = T.tau;
    asm volatile("" : "+v"(h));
    return step_block(T.x, T.F1x, T.F1y, T.F2x, T.F2y, h, T.md, M);
}
__device__ __forceinline__ StepBlock touchdown_stance_block(const TouchdownBlock& T, const Model& M) {
    double h = T.rest;
    asm volatile("" : "+v"(h));
    return step_block(T.xp, T.F1x, T.F1y, T.F2x, T.F2y, h, KnotMode{false, false, false, true}, M);
}

// out = A* v + B* f = A_3 J (A_m v + B_m f + b_m s) + B_3 f - b_3 s,  s = t_x . v + t_F . f   (kHasF false: f = 0)
template <bool kHasF>
__device__ __forceinline__ void touchdown_apply(const TouchdownBlock& T, const Model& M, const double (&v)[15],
                                                const double (&f)[4], double (&out)[15]) {
    const bool f2 = T.md.f2free;  // mode 1: foot 2 is the free one
    double s = fma(T.ty, f2 ? v[6] : v[4], T.tv * (f2 ? v[13] : v[11]));
    if constexpr (kHasF) s = fma(T.tF, f2 ? f[3] : f[1], s);
    double w[15];
#pragma unroll
    for (int i = 0; i < 15; ++i) w[i] = out[i] = 0.0;
    for_each_rollout_entry(touchdown_flight_block(T, M), [&](auto r, auto c, double val) {
        if constexpr (c < 15) w[r] = fma(val, v[c], w[r]);
        else if constexpr (c == 19) w[r] = fma(val, s, w[r]);
        else if constexpr (kHasF) w[r] = fma(val, f[c - 15], w[r]);
    });
    jump_map(w);
    for_each_rollout_entry(touchdown_stance_block(T, M), [&](auto r, auto c, double val) {
        if constexpr (c < 15) out[r] = fma(val, w[c], out[r]);
        else if constexpr (c == 19) out[r] = fma(-val, s, out[r]);
        else if constexpr (kHasF) out[r] = fma(val, f[c - 15], out[r]);
    });
}

// The transposed operator on a vector p:  q = A_3'p,  r = J q,  sigma = b_m . r - b_3 . p,
//   ax = A*'p = A_m'r + sigma t_x,   bf = B*'p = B_m'r + B_3'p + sigma t_F
// sigma is what the saltation term hangs on, and as two dot products it cancels: the body moves through the touchdown, so
// b_m and b_3 agree in its rows and r is close to p there.  A_3 has a unit diagonal (mode 3, no jump), so with
// dq = (A_3' - I) p and q = p + dq the same number is  sum over the rows J keeps of (b_m - b_3) q + b_3 dq,  less b_3 p over
// the rows it zeroes: small terms, formed from differences.  The Riccati sweep subtracts Qux'K from Qxx with a factor of
// about 70 between them and the result (R is small); summed the plain way, sigma's rounding left 1e-13 in P where the numpy
// recursion leaves 1e-14.
__device__ __forceinline__ void touchdown_apply_t(const TouchdownBlock& T, const Model& M, const double (&p)[15],
                                                  double (&ax)[15], double (&bf)[4]) {
    const bool f2 = T.md.f2free;
    double q[15], dq[15], b3[15], sigma = 0.0;
#pragma unroll
    for (int i = 0; i < 15; ++i) dq[i] = ax[i] = 0.0;
#pragma unroll
    for (int m = 0; m < 4; ++m) bf[m] = 0.0;
    for_each_rollout_entry(touchdown_stance_block(T, M), [&](auto r, auto c, double val) {
        if constexpr (c < 15) {
            if constexpr (r != c) dq[c] = fma(val, p[r], dq[c]);  // the diagonal is 1.0
        } else if constexpr (c == 19) {
            b3[r] = val;
        } else {
            bf[c - 15] = fma(val, p[r], bf[c - 15]);
        }
    });
#pragma unroll
    for (int i = 0; i < 15; ++i) q[i] = p[i] + dq[i];
    jump_map(q);
    for_each_rollout_entry(touchdown_flight_block(T, M), [&](auto r, auto c, double val) {
        if constexpr (c < 15) {
            ax[c] = fma(val, q[r], ax[c]);
        } else if constexpr (c == 19) {
            constexpr bool zeroed = r == 4 || r == 6 || (r >= 10 && r <= 13);  // the rows of jump_map
            if constexpr (zeroed) sigma = fma(-b3[r], p[r], sigma);
            else sigma = fma(val - b3[r], q[r], fma(b3[r], dq[r], sigma));
        } else {
            bf[c - 15] = fma(val, q[r], bf[c - 15]);
        }
    });
    const double sy = sigma * T.ty, sv = sigma * T.tv, sF = sigma * T.tF;
    ax[4] += f2 ? 0.0 : sy;
    ax[6] += f2 ? sy : 0.0;
    ax[11] += f2 ? 0.0 : sv;
    ax[13] += f2 ? sv : 0.0;
    bf[1] += f2 ? 0.0 : sF;
    bf[3] += f2 ? sF : 0.0;
}

struct TrackWeights {
    double Q[15], R[4], Qf[15];
};

// The contact-aware force limits (qln_tracking_rollout_limited): {lo, hi} of F_x and F_y for a free foot, then
// for a standing one, passed by value in the kernel arguments.
struct ForceLimits {
    double v[QLN_FORCE_LIMITS_N];
};

// Channel m's clamp: s = 1 below lo, 2 above hi, else 0 (a NaN fails both comparisons and passes through); returns 4^m s, the
// channel's digit of the knot's saturation code.  The limits are selected by the foot's contact state, never indexed: a
// private array indexed at run time is laid out in scratch memory.
template <int m>
__device__ __forceinline__ double clamp_channel(const ForceLimits& lim, bool stand, double& F) {
    constexpr int ax = 2 * (m & 1);  // F_x or F_y
    const double lo = stand ? lim.v[4 + ax] : lim.v[ax], hi = stand ? lim.v[5 + ax] : lim.v[1 + ax];
    const bool below = F < lo, above = F > hi;
    F = below ? lo : above ? hi : F;
    return below ? (double)(1 << (2 * m)) : above ? (double)(2 << (2 * m)) : 0.0;
}
// the applied forces of a knot within the limits; stand1, stand2: the foot stands at the knot's start.  Returns the code.
__device__ __forceinline__ double clamp_forces(const ForceLimits& lim, bool stand1, bool stand2, double (&u)[5]) {
    double code = clamp_channel<0>(lim, stand1, u[0]);
    code += clamp_channel<1>(lim, stand1, u[1]);
    code += clamp_channel<2>(lim, stand2, u[2]);
    code += clamp_channel<3>(lim, stand2, u[3]);
    return code;
}
// A knot's saturation code as the sweeps read it: bit m says channel m rode a limit (digit s_m != 0).  Anything that is not a
// code (the device forms do not validate sat) is no channel at all.
__device__ __forceinline__ unsigned limit_mask(double code) {
    const unsigned c = (code >= 0.0 && code <= 170.0) ? (unsigned)code : 0u;
    return ((c | (c >> 1)) & 0x55u);
}
__device__ __forceinline__ bool limited(unsigned mask, int m) { return (mask >> (2 * m)) & 1u; }
// v[m] = 0 on the channels of the mask: a clamped force is a constant (selected, so that nothing non-finite survives)
__device__ __forceinline__ void limit_zero4(unsigned mask, double (&v)[4]) {
#pragma unroll
    for (int m = 0; m < 4; ++m) v[m] = limited(mask, m) ? 0.0 : v[m];
}

// The knot's block is formed in every lane's registers; forming it once per row into LDS tables was measured slower
// (profiles/tracking_variants.txt).
// kGuard (qln_tracking_lqr_guarded, with kModel): the blocks of the guarded sweeps at Zref's (x_k, u_k).  The model is the
// problem's (plant_model), the modes are guard_mode's of the problem's touchdown knot ks, read with tau from event, and every
// knot but ks is the statement below.  At ks the knot runs on the transposed composite operator (touchdown_apply_t), three
// kinds of application per lane: (T row j, S row j) = (A*'p_j, B*'p_j) -> LDS; lane j reads column j of T back and applies the
// operator again, which gives column j of Qxx = A*'T (row j, by symmetry) and column j of Qux = B*'T; B*' on the four columns
// of S gives Quu, the same in every lane.  The factorisation, the K column, P_k's row and the stores are the same code for
// every knot; the rows of a wave reach their ks in different iterations, and only the operator applications diverge.  T's
// image has a row stride of kLTGuard here, so that neither the lanes' row writes nor their column reads share a bank.
// kLimit (qln_tracking_lqr_limited): the columns of B_k of the channels that rode a limit at knot k (sat, the
// limited roll-out's record, decoded once per knot) are zero.  On the block's tables that is S = P B's and Quu's; on the composite
// operator it is B*'p's entries, the mask at the operator's force input, so the rank-one d tau term loses the channel too.
// Quu then decouples to R_m on those channels and their rows of K are exact zeros.
template <bool kWantP, bool kModel, bool kGuard, bool kLimit = false>
__global__ __launch_bounds__(kWave) void k_tracking_lqr(BatchParams P, TrackWeights W, const double* __restrict__ Zref,
                                                        double* __restrict__ Kout, double* __restrict__ Pout,
                                                        const double* __restrict__ model, const double* __restrict__ event,
                                                        const double* __restrict__ sat) {
    static_assert(kModel || !kGuard, "the guarded sweep runs on the kModel path");
    // T's row stride, and the sections behind it
    constexpr int kTS = kGuard ? kLTGuard : 16, kLS = kLT + (kGuard ? 16 * 16 : 15 * 16), kLK = kLS + 60, kLP = kLK + 60,
                  kLRow = kLP + QLN_TRACK_P_NNZ;
    static_assert(kLRow % 2 == 0 && kLS % 2 == 0 && kLK % 2 == 0 && kLP % 2 == 0 && 15 * kTS <= kLS - kLT, "16-byte aligned sections");
    __shared__ double lds[kRows * kLRow];
    const Row16 r16 = row16_of(P);  // lane 15 shadows row 14 and stores nothing
    const int ln = r16.ln, j = r16.j, b = r16.b, bc = r16.bc, kt = r16.kt, im = r16.im, N = P.N;
    const bool own = r16.own, valid = r16.valid;
    const Model Mp = plant_model<kModel>(P, model, bc);
    const Model& M = kGuard ? Mp : r16.M;
    const GuardEvent ev = guard_event<kGuard>(event, bc, N);
    [[maybe_unused]] const int ks = ev.ks;
    [[maybe_unused]] const double tau = ev.tau;
    double* __restrict__ L = lds + r16.row * kLRow;
    const double* __restrict__ Zb = Zref + (int64_t)bc * P.z_stride;
    const int jp = a_coupling(j), jq = jp < 0 ? 0 : jp;

    // the compact A table: slots no entry fills stay 0.0
    for (int i = ln; i < 64; i += 16) L[kLAC + i] = 0.0;
    // P_N = Qf
    double p[15];
#pragma unroll
    for (int c = 0; c < 15; ++c) p[c] = (c == j) ? W.Qf[c] : 0.0;
    if (kWantP) {
#pragma unroll
        for (int c = 0; c < 15; ++c)
            if (own && c <= j) L[kLP + j * (j + 1) / 2 + c] = p[c];
        wave_lds_sync();
        if (valid) {
            double* __restrict__ Pb = Pout + ((int64_t)b * N + (N - 1)) * QLN_TRACK_P_NNZ;
            for (int i = ln; i < QLN_TRACK_P_NNZ; i += 16) Pb[i] = L[kLP + i];
        }
    }
    // the reference's (x_k, F_k, h_k) of the knot: requested one knot ahead
    double zn[19];
#pragma unroll
    for (int i = 0; i < 19; ++i) zn[i] = Zb[20 * (N - 2) + (i < 14 ? i : i + 1)];

    for (int k = N - 2; k >= 0; --k) {
        double x[14];
#pragma unroll
        for (int i = 0; i < 14; ++i) x[i] = zn[i];
        const double F1x = zn[14], F1y = zn[15], F2x = zn[16], F2y = zn[17], h = zn[18];
        if (k > 0) {
#pragma unroll
            for (int i = 0; i < 19; ++i) zn[i] = Zb[20 * (k - 1) + (i < 14 ? i : i + 1)];
        }
        KnotMode md;
        if constexpr (kGuard) md = guard_mode(k, ks, im);
        else md = knot_mode(k + 1, kt - 1, im);
        const bool td = kGuard && k == ks;  // the touchdown knot: the composite operator instead of the block's tables
        [[maybe_unused]] unsigned lmask = 0u;
        if constexpr (kLimit) lmask = limit_mask(sat[(int64_t)bc * (N - 1) + k]);
        [[maybe_unused]] TouchdownBlock tb;
        double Ac[15][4], Bm[15][4];
        double t[15], sr[4];
        if (td) {
            double xk[15];
#pragma unroll
            for (int i = 0; i < 14; ++i) xk[i] = x[i];
            xk[14] = 0.0;  // the clock feeds nothing
            const double u5[5] = {F1x, F1y, F2x, F2y, h};
            tb = touchdown_block(M, md, tau, xk, u5);
            touchdown_apply_t(tb, M, p, t, sr);
            if constexpr (kLimit) limit_zero4(lmask, sr);
        } else {
#pragma unroll
            for (int c = 0; c < 15; ++c)
#pragma unroll
                for (int s = 0; s < 4; ++s) Ac[c][s] = Bm[c][s] = 0.0;
            const StepBlock blk = step_block(x, F1x, F1y, F2x, F2y, h, md, M);
            for_each_rollout_entry(blk, [&](auto r, auto c, double val) {
                if constexpr (c < 15) Ac[c][a_slot(r, c)] = val;
                else if constexpr (c < 19) Bm[r][c - 15] = val;
            });
            // ---- 1. the knot's A table; T row j = P row j . A, S row j = P row j . B ----
            if (ln == 0) {
#pragma unroll
                for (int c = 0; c < 15; ++c)
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        if ((a_slots(c) >> s) & 1u) L[kLAC + 4 * c + s] = Ac[c][s];
            }
#pragma unroll
            for (int c = 0; c < 15; ++c) {
                const unsigned sl = a_slots(c);
                double acc = p[c] * Ac[c][0];
                if ((sl >> 1) & 1u) acc = fma(p[2], Ac[c][1], acc);
                if ((sl >> 2) & 1u) acc = fma(p[9], Ac[c][2], acc);
                if ((sl >> 3) & 1u) acc = fma(p[a_coupling(c) < 0 ? 0 : a_coupling(c)], Ac[c][3], acc);
                t[c] = acc;
            }
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                double acc = 0.0;
                bool first = true;
#pragma unroll
                for (int r = 0; r < 15; ++r)
                    if ((b_rows_mask(m) >> r) & 1u) {
                        acc = first ? p[r] * Bm[r][m] : fma(p[r], Bm[r][m], acc);
                        first = false;
                    }
                sr[m] = acc;
            }
            // the masked columns of B, where they show: S = P B here, Quu's rows and columns below (Qux reads S alone)
            if constexpr (kLimit) limit_zero4(lmask, sr);
        }
        if (own) {
#pragma unroll
            for (int c = 0; c < 15; ++c) L[kLT + kTS * j + c] = t[c];
#pragma unroll
            for (int m = 0; m < 4; ++m) L[kLS + 4 * j + m] = sr[m];
        }
        wave_lds_sync();
        // ---- 2. Qxx row j = A'T, Quu = R + B'S, Qux column j = S'A column j; K column j ----
        double qx[15], qu[4], q[4][4];
        if (td) {
            // column j of T, then A*' and B*' on it: column j of Qxx (its row j, by symmetry) and of Qux
            double tc[15];
#pragma unroll
            for (int i = 0; i < 15; ++i) tc[i] = L[kLT + kTS * i + j];
            touchdown_apply_t(tb, M, tc, qx, qu);
            if constexpr (kLimit) limit_zero4(lmask, qu);
            // Quu = R + B*'S, column by column
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                double sc[15], ax[15], bs[4];
#pragma unroll
                for (int i = 0; i < 15; ++i) sc[i] = L[kLS + 4 * i + m];
                touchdown_apply_t(tb, M, sc, ax, bs);
                if constexpr (kLimit) limit_zero4(lmask, bs);
#pragma unroll
                for (int n = m; n < 4; ++n) {
                    const double acc = (m == n) ? W.R[m] + bs[n] : bs[n];
                    q[n][m] = acc;
                    q[m][n] = acc;
                }
            }
        } else {
            const double a0 = L[kLAC + 4 * j], a2 = L[kLAC + 4 * j + 1], a9 = L[kLAC + 4 * j + 2], ac = L[kLAC + 4 * j + 3];
#pragma unroll
            for (int c = 0; c < 15; ++c) {
                double acc = a0 * t[c];
                acc = fma(a2, L[kLT + kTS * 2 + c], acc);
                acc = fma(a9, L[kLT + kTS * 9 + c], acc);
                acc = fma(ac, L[kLT + kTS * jq + c], acc);
                qx[c] = acc;
            }
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                double acc = a0 * sr[m];
                acc = fma(a2, L[kLS + 4 * 2 + m], acc);
                acc = fma(a9, L[kLS + 4 * 9 + m], acc);
                acc = fma(ac, L[kLS + 4 * jq + m], acc);
                qu[m] = acc;
            }
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int m = 0; m <= n; ++m) {
                    double acc = (m == n) ? W.R[m] : 0.0;
#pragma unroll
                    for (int r = 0; r < 15; ++r)
                        if ((b_rows_mask(n) >> r) & 1u) acc = fma(L[kLS + 4 * r + m], Bm[r][n], acc);
                    if constexpr (kLimit) {
                        if (m != n) acc = (limited(lmask, n) || limited(lmask, m)) ? 0.0 : acc;
                        else acc = limited(lmask, n) ? W.R[n] : acc;
                    }
                    q[n][m] = acc;
                    q[m][n] = acc;
                }
        }
        // Quu = L D L' (the same bits in every lane), then K column j = Quu^-1 Qux column j
        double l[4][4], d[4], dinv[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            double dc = q[c][c];
#pragma unroll
            for (int m = 0; m < c; ++m) dc = fma(-l[c][m] * d[m], l[c][m], dc);
            d[c] = dc;
            dinv[c] = 1.0 / dc;
#pragma unroll
            for (int r = c + 1; r < 4; ++r) {
                double v = q[r][c];
#pragma unroll
                for (int m = 0; m < c; ++m) v = fma(-l[r][m] * d[m], l[c][m], v);
                l[r][c] = v * dinv[c];
            }
        }
        double kc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double v = qu[i];
#pragma unroll
            for (int m = 0; m < i; ++m) v = fma(-l[i][m], kc[m], v);
            kc[i] = v;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) kc[i] *= dinv[i];
#pragma unroll
        for (int i = 3; i >= 0; --i) {
#pragma unroll
            for (int m = i + 1; m < 4; ++m) kc[i] = fma(-l[m][i], kc[m], kc[i]);
        }
        if (own) {
#pragma unroll
            for (int m = 0; m < 4; ++m) L[kLK + 15 * m + j] = kc[m];
        }
        wave_lds_sync();
        // ---- 3. P_k row j on the lower triangle: Q + Qxx - Qux'K ----
#pragma unroll
        for (int c = 0; c < 15; ++c) {
            double acc = qx[c];
#pragma unroll
            for (int m = 0; m < 4; ++m) acc = fma(-qu[m], L[kLK + 15 * m + c], acc);
            if (c == j) acc = acc + W.Q[c];
            if (own && c <= j) L[kLP + j * (j + 1) / 2 + c] = acc;
        }
        wave_lds_sync();
#pragma unroll
        for (int c = 0; c < 15; ++c) p[c] = L[kLP + ((c <= j) ? j * (j + 1) / 2 + c : c * (c + 1) / 2 + j)];
        if (valid) {
            double* __restrict__ Kb = Kout + ((int64_t)b * (N - 1) + k) * (QLN_TRACK_NU * QLN_NX);
            for (int i = ln; i < QLN_TRACK_NU * QLN_NX; i += 16) Kb[i] = L[kLK + i];
            if (kWantP) {
                double* __restrict__ Pb = Pout + ((int64_t)b * N + k) * QLN_TRACK_P_NNZ;
                for (int i = ln; i < QLN_TRACK_P_NNZ; i += 16) Pb[i] = L[kLP + i];
            }
        }
        // the tiles are read above before the next knot's phase 2 / 3 writes them (two hand-offs later)
    }
}

// what the guarded roll-out reports of a problem's touchdown (entries 0..6 of its event record, include/qln_evaluator.h)
struct Touchdown {
    double knot, tau, clock, px, vx, vy, fmin;
};

// One knot of the guarded roll-out, started in `mode` (1, 2: one foot free; 3: both standing; updated).  The free foot's
// height under held forces is y + v t + a t^2 / 2, a = -F_y / mf + g; its first root in [0, h] is taken in the
// cancellation-free form 2 y / (-v + sqrt(v^2 - 2 a y)), and every comparison is false on a NaN.  Without a touchdown the
// step is step_forward's of the flight mode (the same bits); with one it is RK4 over tau in the flight mode, the jump map,
// RK4 over h - tau in mode 3, the forces held, and the clock advanced by h.  y, v and F_y are selected, never indexed: a
// private array indexed at run time is laid out in scratch memory.
__device__ __forceinline__ void guarded_step(const Model& M, int k, int& mode, const double (&x)[15], const double (&u)[5],
                                             double (&xn)[15], Touchdown& td) {
    const double h = u[4];
    const bool m1 = mode == 1, m3 = mode == 3;
    // the feet standing at the knot's start: foot 1 in mode 1, foot 2 in mode 2, both in mode 3
    td.fmin = fmin(td.fmin, m3 ? fmin(u[1], u[3]) : m1 ? u[1] : u[3]);
    bool hit = false;
    double tau = 0.0;
    if (!m3) {
        const double y = m1 ? x[6] : x[4], v = m1 ? x[13] : x[11], Fy = m1 ? u[3] : u[1];
        const double a = -Fy / M.mf + M.g;
        if (y <= 0.0) {
            hit = true;
        } else {
            const double disc = v * v - 2 * a * y;
            const double den = -v + sqrt(disc);
            if (disc >= 0.0 && den > 0.0) {
                tau = 2 * y / den;
                hit = tau <= h;
            }
        }
    }
    const KnotMode md = {mode == 2, m1, false, m3};
    step_mode(M, md, hit ? tau : h, x, u, xn);
    if (hit) {
        td.knot = (double)k;
        td.tau = tau;
        td.clock = x[14] + tau;
        td.px = m1 ? xn[5] : xn[3];
        td.vx = m1 ? xn[12] : xn[10];
        td.vy = m1 ? xn[13] : xn[11];
        double xm[15];
#pragma unroll
        for (int i = 0; i < 15; ++i) xm[i] = xn[i];
        jump_map(xm);
        step_mode(M, KnotMode{false, false, false, true}, h - tau, xm, u, xn);
        xn[14] = x[14] + h;
        mode = 3;
    }
}

// x_1 = x0[b] (or the handle's x0), F_k = F_ref,k - K_k (x_k - x_ref,k), h_k = h_ref,k, x_{k+1} = step_forward.
// kModel: the plant of problem b is model[b] = (g, mb, mf, lb) instead of the handle's model (qln_tracking_rollout_model);
// the same step_forward on it, so equal models give equal bits.
// kGuard (qln_tracking_rollout_guarded): the handle's k_trans is not read.  The problem stays in init_mode until its free
// foot reaches the ground; the knot in which it does takes the composite step of guarded_step, and every later knot is in
// mode 3.  event (null: not written) gets the problem's QLN_TOUCHDOWN_INFO_STRIDE doubles after the last knot.
// kLimit (qln_tracking_rollout_limited, DESIGN.md 4.20, with kModel): the forces are clamped to lim before they are stored,
// before the guard and before the step, with the limits of a standing or of a free foot by the contact mode at the knot's
// start (the lane's mode, or the knot schedule's); sat (null: not written) gets the knot's code sum_m s_m 4^m.
template <bool kModel, bool kGuard, bool kLimit = false>
__global__ __launch_bounds__(kWave) void k_tracking_rollout(BatchParams P, const double* __restrict__ Zref,
                                                            const double* __restrict__ Kg, const double* __restrict__ x0,
                                                            double* __restrict__ Zout, const double* __restrict__ model,
                                                            double* __restrict__ event, ForceLimits lim,
                                                            double* __restrict__ sat) {
    static_assert(kModel || !kLimit, "the limited roll-out runs on the kModel path");
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= P.B) return;
    const ProblemDesc pd = P.desc[b];
    const int N = P.N, kt = pd.k_trans, im = pd.init_mode;
    const Model M = plant_model<kModel>(P, model, b);
    const double* __restrict__ Zr = Zref + (int64_t)b * P.z_stride;
    double* __restrict__ Zo = Zout + (int64_t)b * P.z_stride;
    const double* __restrict__ xs = x0 ? x0 + (int64_t)b * 15 : P.bnd + (int64_t)b * 30;
    double x[15], u[5], xn[15];
#pragma unroll
    for (int i = 0; i < 15; ++i) {
        x[i] = xs[i];
        Zo[i] = x[i];
    }
    int mode = im;
    Touchdown td = {-1.0, 0.0, 0.0, 0.0, 0.0, 0.0, __builtin_inf()};
    for (int k = 0; k < N - 1; ++k) {
#pragma unroll
        for (int i = 0; i < 5; ++i) u[i] = Zr[20 * k + 15 + i];
        if (Kg) {
            const double* __restrict__ Kk = Kg + ((int64_t)b * (N - 1) + k) * (QLN_TRACK_NU * QLN_NX);
            double dx[15];
#pragma unroll
            for (int i = 0; i < 15; ++i) dx[i] = x[i] - Zr[20 * k + i];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                double du = Kk[15 * m] * dx[0];
#pragma unroll
                for (int i = 1; i < 15; ++i) du = fma(Kk[15 * m + i], dx[i], du);
                u[m] = u[m] - du;
            }
        }
        if constexpr (kLimit) {
            bool stand1, stand2;
            if constexpr (kGuard) {
                stand1 = mode != 2, stand2 = mode != 1;
            } else {
                const KnotMode md = knot_mode(k + 1, kt - 1, im);
                stand1 = !md.f1free, stand2 = !md.f2free;
            }
            const double code = clamp_forces(lim, stand1, stand2, u);
            if (sat) sat[(int64_t)b * (N - 1) + k] = code;
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) Zo[20 * k + 15 + i] = u[i];
        if constexpr (kGuard) guarded_step(M, k, mode, x, u, xn, td);
        else step_forward(M, k, kt, im, x, u, xn);
#pragma unroll
        for (int i = 0; i < 15; ++i) {
            x[i] = xn[i];
            Zo[20 * (k + 1) + i] = xn[i];
        }
    }
    if constexpr (kGuard) {
        if (event) {
            double* __restrict__ ev = event + (int64_t)QLN_TOUCHDOWN_INFO_STRIDE * b;
            ev[0] = td.knot;
            ev[1] = td.tau;
            ev[2] = td.clock;
            ev[3] = td.px;
            ev[4] = td.vx;
            ev[5] = td.vy;
            ev[6] = td.fmin;
            ev[7] = 0.0;
        }
    }
}

// The estimate-feedback roll-out (qln_tracking_rollout_estimated / _guarded, include/qln_evaluator.h), in
// k_tracking_rollout's mapping: one lane per problem, which carries the plant's state x and the estimate xhat side by side.
// H is uniform over the batch: the block copies its ny rows to LDS once, and every later read of it is a broadcast read at an
// address the whole wave shares.
// Per knot: the innovation of ny sensor rows and the update xhat += L_k innov in loops over QLN_TRACK_NY_MAX rows, so that x,
// xhat and innov stay at compile-time positions; L_k is read row by row, ny consecutive doubles per lane, with a scheduling
// barrier every three rows -- read column by column a wave's lines of L_k do not fit the L1 and were fetched once per sensor
// row, and with all 120 loads in flight at once the kernel spilled -- then the forces fed back from xhat, then the
// same step twice: the plant's on (x, model[b]) and the estimator's on (xhat, the handle's model).  Products are formed as
// k_tracking_rollout forms K dx: the first product, then fma in index order.
// kGuard: both steps are guarded_step, each on a contact mode and a Touchdown record of its own.
// kLimit (qln_tracking_rollout_estimated_limited): the forces fed back from the estimate are clamped to lim
// before they are stored and before either system's guard and step, as k_tracking_rollout<.., kLimit> clamps them, with the
// limits of a standing or of a free foot by the PLANT's contact mode at the knot's start (its lane's mode, or the knot
// schedule's): the limits are the plant's saturation, whatever the estimator believes.  sat (null: not written) gets the code.
template <bool kGuard, bool kLimit = false>
__global__ __launch_bounds__(kWave) void k_tracking_rollout_estimated(
    BatchParams P, const double* __restrict__ Hg, int ny, const double* __restrict__ Zref, const double* __restrict__ Kg,
    const double* __restrict__ Lg, const double* __restrict__ vnoise, const double* __restrict__ wnoise,
    const double* __restrict__ x0, const double* __restrict__ xhat0, const double* __restrict__ model,
    double* __restrict__ Zout, double* __restrict__ Xhat, double* __restrict__ innov_out, double* __restrict__ event,
    double* __restrict__ event_hat, ForceLimits lim, double* __restrict__ sat) {
    constexpr int NY = QLN_TRACK_NY_MAX;
    __shared__ double Hs[NY * 15];
    for (int i = threadIdx.x; i < 15 * ny; i += kWave) Hs[i] = Hg[i];
    __syncthreads();
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= P.B) return;
    const ProblemDesc pd = P.desc[b];
    const int N = P.N, kt = pd.k_trans, im = pd.init_mode;
    const Model M = plant_model<true>(P, model, b);     // the plant's
    const Model Mh = plant_model<true>(P, nullptr, b);  // the estimator's: always the handle's
    const double* __restrict__ Zr = Zref + (int64_t)b * P.z_stride;
    double* __restrict__ Zo = Zout + (int64_t)b * P.z_stride;
    const double* __restrict__ xs = x0 ? x0 + (int64_t)b * 15 : P.bnd + (int64_t)b * 30;
    const double* __restrict__ hs = xhat0 ? xhat0 + (int64_t)b * 15 : Zr;
    const double* __restrict__ Lb = Lg + (int64_t)b * N * (15 * ny);
    const double* __restrict__ vb = vnoise ? vnoise + (int64_t)b * N * ny : nullptr;
    const double* __restrict__ wb = wnoise ? wnoise + (int64_t)b * (N - 1) * 15 : nullptr;
    double x[15], xhat[15], u[5], xn[15];
#pragma unroll
    for (int i = 0; i < 15; ++i) {
        x[i] = xs[i];
        xhat[i] = hs[i];
        Zo[i] = x[i];
    }
    [[maybe_unused]] int mode = im, mode_hat = im;
    [[maybe_unused]] Touchdown td = {-1.0, 0.0, 0.0, 0.0, 0.0, 0.0, __builtin_inf()}, tdh = td;
    for (int k = 0; k < N; ++k) {
        // innov_k = (H (x_k - x_ref,k) + v_k) - H (xhat^-_k - x_ref,k); the rows behind ny are zeros
        double innov[NY];
        {
            double d[15], e[15];
#pragma unroll
            for (int i = 0; i < 15; ++i) {
                const double xr = Zr[20 * k + i];
                d[i] = x[i] - xr;
                e[i] = xhat[i] - xr;
            }
#pragma unroll
            for (int r = 0; r < NY; ++r) {
                innov[r] = 0.0;
                if (r < ny) {
                    double y = Hs[15 * r] * d[0], yh = Hs[15 * r] * e[0];
#pragma unroll
                    for (int i = 1; i < 15; ++i) {
                        y = fma(Hs[15 * r + i], d[i], y);
                        yh = fma(Hs[15 * r + i], e[i], yh);
                    }
                    if (vb) y = y + vb[(int64_t)ny * k + r];
                    innov[r] = y - yh;
                    if (innov_out) innov_out[((int64_t)b * N + k) * ny + r] = innov[r];
                }
            }
        }
        // xhat_k = xhat^-_k + L_k innov_k, accumulated column by column onto each entry.  Row i of L_k is ny consecutive doubles,
        // which the lane reads as whole cache lines; a column behind ny reads the row's last entry against a zero innovation,
        // which adds an exact zero, so the loop has no branch.  Three rows' loads are in flight at a time.
        {
            // the row's address is carried in the lane and hidden from the optimiser after each step: folded into 120 uniform
            // offsets ny * i + min(r, ny - 1) it took more scalar registers than there are
            const double* Li = Lb + (int64_t)k * (15 * ny);
#pragma unroll
            for (int i = 0; i < 15; ++i) {
#pragma unroll
                for (int r = 0; r < NY; ++r) xhat[i] = fma(Li[min(r, ny - 1)], innov[r], xhat[i]);
                Li += ny;
                asm volatile("" : "+v"(Li));
                if (i % 3 == 2) __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (Xhat) {
            double* __restrict__ Xk = Xhat + ((int64_t)b * N + k) * 15;
#pragma unroll
            for (int i = 0; i < 15; ++i) Xk[i] = xhat[i];
        }
        if (k == N - 1) break;
#pragma unroll
        for (int i = 0; i < 5; ++i) u[i] = Zr[20 * k + 15 + i];
        if (Kg) {
            const double* __restrict__ Kk = Kg + ((int64_t)b * (N - 1) + k) * (QLN_TRACK_NU * QLN_NX);
            double dx[15];
#pragma unroll
            for (int i = 0; i < 15; ++i) dx[i] = xhat[i] - Zr[20 * k + i];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                double du = Kk[15 * m] * dx[0];
#pragma unroll
                for (int i = 1; i < 15; ++i) du = fma(Kk[15 * m + i], dx[i], du);
                u[m] = u[m] - du;
            }
        }
        if constexpr (kLimit) {
            bool stand1, stand2;
            if constexpr (kGuard) {
                stand1 = mode != 2, stand2 = mode != 1;
            } else {
                const KnotMode md = knot_mode(k + 1, kt - 1, im);
                stand1 = !md.f1free, stand2 = !md.f2free;
            }
            const double code = clamp_forces(lim, stand1, stand2, u);
            if (sat) sat[(int64_t)b * (N - 1) + k] = code;
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) Zo[20 * k + 15 + i] = u[i];
        // the plant's step, then the process noise on the whole state
        if constexpr (kGuard) guarded_step(M, k, mode, x, u, xn, td);
        else step_forward(M, k, kt, im, x, u, xn);
#pragma unroll
        for (int i = 0; i < 15; ++i) {
            x[i] = wb ? xn[i] + wb[(int64_t)15 * k + i] : xn[i];
            Zo[20 * (k + 1) + i] = x[i];
        }
        // the estimator's prediction: the same step on the estimate, at the handle's model
        if constexpr (kGuard) guarded_step(Mh, k, mode_hat, xhat, u, xn, tdh);
        else step_forward(Mh, k, kt, im, xhat, u, xn);
#pragma unroll
        for (int i = 0; i < 15; ++i) xhat[i] = xn[i];
    }
    if constexpr (kGuard) {
        auto put = [&](double* __restrict__ out, const Touchdown& t) {
            if (!out) return;
            double* __restrict__ ev = out + (int64_t)QLN_TOUCHDOWN_INFO_STRIDE * b;
            ev[0] = t.knot;
            ev[1] = t.tau;
            ev[2] = t.clock;
            ev[3] = t.px;
            ev[4] = t.vx;
            ev[5] = t.vy;
            ev[6] = t.fmin;
            ev[7] = 0.0;
        };
        put(event, td);
        put(event_hat, tdh);
    }
}

// lanes 0 .. n-1 of a row, in every lane of it
template <int... I>
__device__ __forceinline__ void row_bcast_first(double v, double (&out)[sizeof...(I)], std::integer_sequence<int, I...>) {
    ((out[I] = row_bcast<I>(v)), ...);
}

// One knot's inputs, as lane j of a row reads them: its own x_j, Zbar x_j, x_ref,j and K column j, and the knot's applied
// controls and their cotangents (the same five values in every lane of the row).
struct VjpKnot {
    double x, zb, xr, u[5], ub[5], kc[4];
};

template <bool kHasK>
__device__ __forceinline__ void vjp_load(VjpKnot& s, const double* __restrict__ Zo, const double* __restrict__ Zb,
                                         const double* __restrict__ Zr, const double* __restrict__ Kk, int k, int j) {
    s.x = Zo[20 * k + j];
    s.zb = Zb[20 * k + j];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        s.u[i] = Zo[20 * k + 15 + i];
        s.ub[i] = Zb[20 * k + 15 + i];
    }
    s.xr = Zr ? Zr[20 * k + j] : 0.0;
    if constexpr (kHasK) {
#pragma unroll
        for (int m = 0; m < 4; ++m) s.kc[m] = Kk[15 * m + j];
    }
}

// entry j of a state held in registers, chosen by compares: an array indexed at run time is laid out in scratch memory
// (profiles/rollout_guarded_sweeps_resource_usage.txt)
__device__ __forceinline__ double pick15(const double (&v)[15], int j) {
    double o = v[0];
#pragma unroll
    for (int i = 1; i < 15; ++i) {
        double t = v[i];
        asm volatile("" : "+v"(t));  // opaque: left visible, the chain of selects is turned back into v[j]
        o = (j == i) ? t : o;
    }
    return o;
}

// lane j's constant pattern in the reverse sweep, its scalars: what column j of A, row j of B and h_j are built from (the
// kernel forms them, with the row's two sign patterns e[4] and sg[4], before its loop)
struct VjpLane {
    int j;
    bool pos;        // position row (h^2/2 in B) or velocity / clock row (h)
    int foot;        // the foot the row belongs to (0: body, theta or clock)
    bool jrow;       // a row the jump map zeroes
    bool cpl, kcpl;  // A(j-7, j) = h (times the foot's flag): velocity -> position; ... into a row the jump map zeroes
    double inv, gy;  // B row j = hpow * inv * e, h_j = hfac * (sum_m e[m] F_m * inv + gy) (the clock: 1)
    double g, iIb;
};

// Column j of [A B G]' applied to lam, for one step of length h in mode md at the state whose entry j is xj: returns
// (A'lam)[j], ub = ub0 + (B'lam, the h column's product), and (kModel, want_mbar) adds lane j's share of G'lam to mbar.  The
// knot of the guarded reverse sweep, which its touchdown knot calls twice, once per leg; the statement is the knot-scheduled
// sweep's own, kept there in place (see the kernel).
template <bool kModel>
__device__ __forceinline__ double vjp_apply_column(const VjpLane& c, const double (&e)[4], const double (&sg)[4], double xj,
                                                   double F0, double F1, double F2, double F3, double h, const KnotMode& md,
                                                   const Model& M, double lam, bool want_mbar, double (&mbar)[QLN_MODEL_NP],
                                                   const double (&ub0)[5], double (&ub)[5]) {
    const int j = c.j;
    const bool pos = c.pos;
    const double g = c.g, iIb = c.iIb;
    const double m1 = md.f1free ? 1.0 : 0.0, m2 = md.f2free ? 1.0 : 0.0;
    const double keep = md.jump ? 0.0 : 1.0;
    const double h2 = h * h;
    const double Aw = h * iIb, At = 0.5 * h2 * iIb, Bt = h2 * h * iIb * (1.0 / 6.0), Ct = h2 * h2 * iIb * (1.0 / 24.0);
    const double ga1 = g * (1.0 - m1), ga2 = g * (1.0 - m2);
    const double taua = ga1 * F0 + ga2 * F2;
    // the lane's masks for this knot
    const double fm = c.foot == 1 ? m1 : c.foot == 2 ? m2 : 1.0;  // the row's foot is free
    const double km = c.jrow ? keep : 1.0;
    const double rmask = fm * km;                           // row j of B and of the h column
    const double fmv = pos ? 1.0 : fm;                      // w = m foot velocity - body velocity
    const double cmask = c.cpl ? fm * (c.kcpl ? keep : 1.0) : 0.0;
    if constexpr (kModel) {
        if (want_mbar) {
            double xk[14];
            row_bcast_first(xj, xk, std::make_integer_sequence<int, 14>{});
            const ModelBlock mblk = model_block(xk, F0, F1, F2, F3, h, md, M);
            for_each_model_entry(mblk, [&](auto r, auto q, double val) { mbar[q] = (j == r) ? fma(val, lam, mbar[q]) : mbar[q]; });
        }
    }
    // cross-lane lam: rows 2 and 9 (row broadcasts) and j-7 (row shift)
    const double lam2 = dpp_f64<0x152>(lam), lam9 = dpp_f64<0x159>(lam), lamc = row_shr7(lam);
    // ---- A'lam, column j: diagonal, rows 2 and 9 (h-power times d tau / d x_j), row j-7 ----
    const double sF = ((sg[0] * F0 + sg[1] * F1) + sg[2] * F2) + sg[3] * F3;
    const double phi = fmv * sF;
    const double alam = fma(h * cmask, lamc, fma((pos ? Aw : At) * phi, lam9, fma((pos ? At : Bt) * phi, lam2, km * lam)));
    // ---- the lane's shares of B'lam and of the h column ----
    const double Lr = rmask * lam;
    const double Fs = ((e[0] * F0 + e[1] * F1) + e[2] * F2) + e[3] * F3;
    const double bco = (pos ? 0.5 * h2 : h) * c.inv * Lr;
    const double al = At * lam2 + Aw * lam9, be = Bt * lam2 + At * lam9, gm = Ct * lam2 + Bt * lam9;
    const double xs = fmv * xj;
    const double tco = (pos ? al : be) * xs;                // rows 2 and 9 of B, through d tau / d F_m
    double red[5];
#pragma unroll
    for (int m = 0; m < 4; ++m) red[m] = fma(e[m], bco, sg[m] * tco);
    const double hco = pos ? fma(Aw, lam2, iIb * lam9) : al;  // rows 2 and 9 of the h column, through tau
    red[4] = fma(cmask * xj, lamc, fma(hco * xs, sF, (pos ? h : 1.0) * fma(Fs, c.inv, c.gy) * Lr));
#pragma unroll
    for (int m = 0; m < 5; ++m) ub[m] = ub0[m] + row_sum16(red[m]);
    ub[0] = fma(gm, ga1, ub[0]);
    ub[2] = fma(gm, ga2, ub[2]);
    ub[4] = fma(be, taua, ub[4]);
    return alam;
}

// The reverse sweep of k_tracking_rollout (include/qln_evaluator.h): lam_{N-1} = Zbar[x_{N-1}], then per knot k = N-2..0
//   ubar = Zbar[u_k] + B_k'lam_{k+1},  lam_k = Zbar[x_k] + A_k'lam_{k+1} - K_k'ubar[0:4],
// with xref_bar_k = K_k'ubar[0:4], Kbar_k = -ubar[0:4] (x_k - x_ref,k)'.  A_k, B_k and the h column are the derivative of
// step_forward at Zout's (x_k, u_k): the evaluator's closed form, with the jump knot's clock row kept (1 at x[14] and at h).
// Zr is read only for Kbar (may be null otherwise).
// kModel (qln_tracking_rollout_model_vjp): the blocks are formed at problem b's own model (model, null: the handle's), and
// model_bar[b] = sum_k G_k'lam_{k+1} with G_k = d Phi_k / d (g, mb, mf, lb) of qln_kernel_common.h: every lane forms the knot's
// ModelBlock (Zout's states handed round by DPP row broadcasts), lane j accumulates G_k[j][p] lam_{k+1}[j] over the knots,
// and the four row sums are taken once, after the loop.
// kGuard (qln_tracking_rollout_guarded_vjp, with kModel): the modes are guard_mode's of the problem's touchdown knot ks, read
// with tau from event.  At ks the transpose of the composite step: vjp_apply_column through the mode-3 leg at (x+, h - tau),
// the jump map's zeros, vjp_apply_column through the flight leg at (x_k, tau); what the two h columns leave for tau goes, by
// d tau's coefficients, onto lam[iy], lam[iv], the free foot's ubar_F_y and the model's g and mf.  x- and x+ are recomputed by
// every lane of the row with step_mode, as the roll-out forms them.
// kLimit (qln_tracking_rollout_limited_vjp, DESIGN.md 4.20, with kModel): a channel that rode a limit at knot k (sat, the limited
// roll-out's record) was a constant, so its ubar is zeroed -- after the touchdown knot's taubar has been distributed onto it,
// before it enters K_k'ubar, K_bar and Zref_bar.
template <bool kHasK, bool kModel, bool kGuard, bool kLimit = false>
__global__ __launch_bounds__(kWave) void k_tracking_rollout_vjp(BatchParams P, const double* __restrict__ Zref,
                                                                const double* __restrict__ Kg, const double* __restrict__ Zout,
                                                                const double* __restrict__ Zbar, double* __restrict__ Zref_bar,
                                                                double* __restrict__ Kbar, double* __restrict__ x0_bar,
                                                                const double* __restrict__ model,
                                                                double* __restrict__ model_bar,
                                                                const double* __restrict__ event,
                                                                const double* __restrict__ sat) {
    static_assert(kModel || !kGuard, "the guarded sweep runs on the kModel path");
    static_assert(kModel || !kLimit, "the limited sweep runs on the kModel path");
    const Row16 r16 = row16_of(P);  // lane 15 reads lane 14's slots and contributes nothing
    const int j = r16.j, b = r16.b, bc = r16.bc, kt = r16.kt, im = r16.im, N = P.N;
    const bool own = r16.own, valid = r16.valid;
    const Model M = plant_model<kModel>(P, model, bc);
    const double g = M.g, imb = 1.0 / M.mb, imf = 1.0 / M.mf;
    const double iIb = 12.0 / (M.mb * (M.lb * M.lb));
    const double* __restrict__ Zo = Zout + (int64_t)bc * P.z_stride;
    const double* __restrict__ Zb = Zbar + (int64_t)bc * P.z_stride;
    const double* __restrict__ Zr = Kbar ? Zref + (int64_t)bc * P.z_stride : nullptr;
    const double* __restrict__ Kb = kHasK ? Kg + (int64_t)bc * (N - 1) * (QLN_TRACK_NU * QLN_NX) : nullptr;
    const GuardEvent ev = guard_event<kGuard>(event, bc, N);
    [[maybe_unused]] const int ks = ev.ks;
    [[maybe_unused]] const double tau = ev.tau;

    // ---- lane j's constant pattern: what column j of A, row j of B and h_j are built from ----
    const bool pos = j < 7;                 // position row (h^2/2 in B) or velocity / clock row (h)
    const int p = pos ? j : j - 7;          // the position index the row belongs to (7: the clock)
    const int foot = (p == 3 || p == 4) ? 1 : (p == 5 || p == 6) ? 2 : 0;
    const bool jrow = j == 4 || j == 6 || (j >= 10 && j <= 13);  // rows the jump map zeroes
    const bool cpl = j >= 7 && j <= 13;     // A(j-7, j) = h (times the foot's flag): velocity -> position
    const bool kcpl = j == 11 || j == 13;   // ... into a row the jump map zeroes
    // e[m]: the force columns of B's row j (body rows: F_p and F_{p+2} through 1/mb; foot rows: their foot's F_{p-3});
    // sg[m]: d^2 tau / d x_p d F_m of the torque tau = r1x F1y - r1y F1x + r2x F2y - r2y F2x (r = foot - body position)
    double e[4], sg[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        e[m] = ((p <= 1 && (m == p || m == p + 2)) || (foot && m == p - 3)) ? 1.0 : 0.0;
        sg[m] = 0.0;
    }
    if (p == 0) sg[1] = sg[3] = -1.0;
    if (p == 1) sg[0] = sg[2] = 1.0;
    if (p == 3) sg[1] = 1.0;
    if (p == 4) sg[0] = -1.0;
    if (p == 5) sg[3] = 1.0;
    if (p == 6) sg[2] = -1.0;
    // B row j = hpow * inv * e, h_j = hfac * (sum_m e[m] F_m * inv + gy) (the clock: 1)
    const double inv = (p <= 1) ? imb : foot ? -imf : 0.0;
    const double gy = (p == 1 || p == 4 || p == 6) ? g : (j == 14) ? 1.0 : 0.0;
    [[maybe_unused]] const VjpLane lc = {j, pos, foot, jrow, cpl, kcpl, inv, gy, g, iIb};

    double mbar[QLN_MODEL_NP] = {0.0, 0.0, 0.0, 0.0};  // lane j's share of model_bar
    double lam = own ? Zb[20 * (N - 1) + j] : 0.0;
    if (valid && Zref_bar && own) Zref_bar[(int64_t)b * P.z_stride + 20 * (N - 1) + j] = 0.0;  // x_ref,N-1: never read
    VjpKnot cur, nxt;
    vjp_load<kHasK>(nxt, Zo, Zb, Zr, Kb + (kHasK ? (int64_t)(N - 2) * 60 : 0), N - 2, j);
    // the knot's saturation code, loaded with the knot's slices (the same value in every lane of the row)
    [[maybe_unused]] const double* __restrict__ Sb = kLimit ? sat + (int64_t)bc * (N - 1) : nullptr;
    [[maybe_unused]] double satc = 0.0, satn = 0.0;
    if constexpr (kLimit) satn = Sb[N - 2];
    for (int k = N - 2; k >= 0; --k) {
        cur = nxt;
        if (k > 0) vjp_load<kHasK>(nxt, Zo, Zb, Zr, Kb + (kHasK ? (int64_t)(k - 1) * 60 : 0), k - 1, j);
        if constexpr (kLimit) {
            satc = satn;
            if (k > 0) satn = Sb[k - 1];
        }
        KnotMode md;
        if constexpr (kGuard) md = guard_mode(k, ks, im);
        else md = knot_mode(k + 1, kt - 1, im);
        const double F0 = cur.u[0], F1 = cur.u[1], F2 = cur.u[2], F3 = cur.u[3], h = cur.u[4];
        double ub[5];
        double alam;
        if constexpr (kGuard) {
            const bool td = k == ks;
            double lamA = lam, hA = h, hb3 = 0.0, w = 1.0, y = 0.0;
            double ubA[5] = {cur.ub[0], cur.ub[1], cur.ub[2], cur.ub[3], cur.ub[4]};
            if (td) {
                double xk[15], xm[15];
                row_bcast_first(cur.x, xk, std::make_integer_sequence<int, 15>{});
                const double u5[5] = {F0, F1, F2, F3, h};
                step_mode(M, md, tau, xk, u5, xm);
                y = md.f2free ? xk[6] : xk[4];
                w = md.f2free ? xm[13] : xm[11];
                jump_map(xm);
                // the mode-3 leg at (x+, F, h - tau)
                ubA[4] = 0.0;
                double ub3[5];
                const double a3 = vjp_apply_column<kModel>(lc, e, sg, pick15(xm, j), F0, F1, F2, F3, h - tau,
                                                           KnotMode{false, false, false, true}, M, lam, model_bar != nullptr, mbar, ubA,
                                                           ub3);
#pragma unroll
                for (int m = 0; m < 4; ++m) ubA[m] = ub3[m];
                hb3 = ub3[4];
                lamA = (own && !lc.jrow) ? a3 : 0.0;  // the jump map
                hA = tau;
            }
            alam = vjp_apply_column<kModel>(lc, e, sg, cur.x, F0, F1, F2, F3, hA, md, M, lamA, model_bar != nullptr, mbar, ubA, ub);
            if (td) {
                // tau's cotangent, and d tau = -(dy + tau dv + tau^2/2 da) / w with da = -dF_y / mf + F_y / mf^2 dmf + dg
                const double taubar = ub[4] - hb3;
                ub[4] = cur.ub[4] + hb3;
                const bool f2 = md.f2free;
                const double cw = (y <= 0.0) ? 0.0 : -taubar / w, ca = cw * (0.5 * tau * tau);
                const int iy = f2 ? 6 : 4, iv = f2 ? 13 : 11;
                alam = (j == iy) ? alam + cw : (j == iv) ? fma(cw, tau, alam) : alam;
                const double Fy = f2 ? F3 : F1, cf = -ca / M.mf;
                ub[1] = f2 ? ub[1] : ub[1] + cf;
                ub[3] = f2 ? ub[3] + cf : ub[3];
                if (r16.ln == 0) {
                    mbar[0] += ca;
                    mbar[2] = fma(ca, Fy / (M.mf * M.mf), mbar[2]);
                }
            }
        } else {
            // The knot-scheduled sweeps keep their own statement of the knot, the one vjp_apply_column restates: routed through
            // the function, all four of them were allocated 2 to 6 VGPRs differently
            // (profiles/rollout_guarded_sweeps_resource_usage.txt).  A guarded sweep of a batch that never lands is bit for bit
            // the _model_ sweep (tests/test_gpu_rollout_guarded_sweeps.py), which holds the two statements to each other.
            const double m1 = md.f1free ? 1.0 : 0.0, m2 = md.f2free ? 1.0 : 0.0;
            const double keep = md.jump ? 0.0 : 1.0;
            const double h2 = h * h;
            const double Aw = h * iIb, At = 0.5 * h2 * iIb, Bt = h2 * h * iIb * (1.0 / 6.0), Ct = h2 * h2 * iIb * (1.0 / 24.0);
            const double ga1 = g * (1.0 - m1), ga2 = g * (1.0 - m2);
            const double taua = ga1 * F0 + ga2 * F2;
            // the lane's masks for this knot
            const double fm = foot == 1 ? m1 : foot == 2 ? m2 : 1.0;  // the row's foot is free
            const double km = jrow ? keep : 1.0;
            const double rmask = fm * km;                           // row j of B and of the h column
            const double fmv = pos ? 1.0 : fm;                      // w = m foot velocity - body velocity
            const double cmask = cpl ? fm * (kcpl ? keep : 1.0) : 0.0;
            if constexpr (kModel) {
                if (model_bar) {
                    double xk[14];
                    row_bcast_first(cur.x, xk, std::make_integer_sequence<int, 14>{});
                    const ModelBlock mblk = model_block(xk, F0, F1, F2, F3, h, md, M);
                    for_each_model_entry(mblk, [&](auto r, auto q, double val) { mbar[q] = (j == r) ? fma(val, lam, mbar[q]) : mbar[q]; });
                }
            }
            // cross-lane lam: rows 2 and 9 (row broadcasts) and j-7 (row shift)
            const double lam2 = dpp_f64<0x152>(lam), lam9 = dpp_f64<0x159>(lam), lamc = row_shr7(lam);
            // ---- A'lam, column j: diagonal, rows 2 and 9 (h-power times d tau / d x_j), row j-7 ----
            const double sF = ((sg[0] * F0 + sg[1] * F1) + sg[2] * F2) + sg[3] * F3;
            const double phi = fmv * sF;
            alam = fma(h * cmask, lamc, fma((pos ? Aw : At) * phi, lam9, fma((pos ? At : Bt) * phi, lam2, km * lam)));
            // ---- the lane's shares of B'lam and of the h column ----
            const double Lr = rmask * lam;
            const double Fs = ((e[0] * F0 + e[1] * F1) + e[2] * F2) + e[3] * F3;
            const double bco = (pos ? 0.5 * h2 : h) * inv * Lr;
            const double al = At * lam2 + Aw * lam9, be = Bt * lam2 + At * lam9, gm = Ct * lam2 + Bt * lam9;
            const double xs = fmv * cur.x;
            const double tco = (pos ? al : be) * xs;                // rows 2 and 9 of B, through d tau / d F_m
            double red[5];
#pragma unroll
            for (int m = 0; m < 4; ++m) red[m] = fma(e[m], bco, sg[m] * tco);
            const double hco = pos ? fma(Aw, lam2, iIb * lam9) : al;  // rows 2 and 9 of the h column, through tau
            red[4] = fma(cmask * cur.x, lamc, fma(hco * xs, sF, (pos ? h : 1.0) * fma(Fs, inv, gy) * Lr));
#pragma unroll
            for (int m = 0; m < 5; ++m) ub[m] = cur.ub[m] + row_sum16(red[m]);
            ub[0] = fma(gm, ga1, ub[0]);
            ub[2] = fma(gm, ga2, ub[2]);
            ub[4] = fma(be, taua, ub[4]);
        }
        if constexpr (kLimit) {
            const unsigned lmask = limit_mask(satc);
#pragma unroll
            for (int m = 0; m < 4; ++m) ub[m] = limited(lmask, m) ? 0.0 : ub[m];
        }
        // ---- K'ubar, lam_k, and the outputs of the knot ----
        double kub = 0.0;
        if constexpr (kHasK) kub = ((cur.kc[0] * ub[0] + cur.kc[1] * ub[1]) + cur.kc[2] * ub[2]) + cur.kc[3] * ub[3];
        lam = own ? (cur.zb + alam) - kub : 0.0;
        if (valid) {
            if (Zref_bar) knot_store(Zref_bar + (int64_t)b * P.z_stride + 20 * k, r16, kub, ub);
            if (kHasK && Kbar && own) {
                double* __restrict__ o = Kbar + ((int64_t)b * (N - 1) + k) * (QLN_TRACK_NU * QLN_NX);
                const double dx = cur.x - cur.xr;
#pragma unroll
                for (int m = 0; m < 4; ++m) o[15 * m + j] = -ub[m] * dx;
            }
        }
    }
    if (valid && x0_bar && own) x0_bar[(int64_t)b * QLN_NX + j] = lam;
    if constexpr (kModel) {
        if (model_bar) {
            double out = 0.0;
#pragma unroll
            for (int q = 0; q < QLN_MODEL_NP; ++q) {
                const double sq = row_sum16(mbar[q]);
                out = (r16.ln == q) ? sq : out;
            }
            if (valid && r16.ln < QLN_MODEL_NP) model_bar[(int64_t)b * QLN_MODEL_NP + r16.ln] = out;
        }
    }
}


// ---- k_tracking_covariance ----
// per-row LDS image (doubles): Sigma / V image [15][17] (one region: V lives there between the two applications) | K [4][16] |
// the knot's 20 entries of Zout | the clearance derivatives of sixteen knots.  The image, its tiles, the chains and the
// congruence step of this kernel, k_tracking_kalman and k_landing_smoother: qln_image15.h.
constexpr int kCImg = 0, kCK = 256, kCZ = kCK + 4 * 16, kCD = kCZ + 20, kCRow = kCD + 16;
static_assert(kImgSize <= kCK - kCImg && kCK % 2 == 0 && kCZ % 2 == 0 && kCD % 2 == 0 && kCRow % 2 == 0,
              "the image fits; 16-byte aligned sections");

struct CovNoise {
    double w[15];
};

// g = K v on the K tile (rows of sixteen); zeros without K
template <bool kHasK>
__device__ __forceinline__ void k_times(const double* Kl, const double (&v)[15], double (&g)[4]) {
    if constexpr (kHasK) {
        chain_rows([&](int m, int c) { return Kl[16 * m + c]; }, v, g);
    } else {
#pragma unroll
        for (int m = 0; m < 4; ++m) g[m] = 0.0;
    }
}

// out = Acl v = A v - B (K v); g = K v (4).  The block's entries are formed where they are used (the weight x force
// products of rows 2 and 9 included): what stays live between the knot's two applications is the StepBlock, not 70 entries.
template <bool kHasK>
__device__ __forceinline__ void cov_apply(const StepBlock& blk, const double* Kl, const double (&v)[15],
                                          double (&out)[15], double (&g)[4]) {
#pragma unroll
    for (int i = 0; i < 15; ++i) out[i] = 0.0;
    k_times<kHasK>(Kl, v, g);
    // the h-weights pass through an empty asm, as in the evaluator's tile loop: the 25 weight x force products are then
    // formed here, in each application, instead of living in 50 registers across both
    StepBlock bk = blk;
    asm volatile("" : "+v"(bk.wAt), "+v"(bk.wBt), "+v"(bk.wAw));
    for_each_rollout_entry(bk, [&](auto r, auto c, double val) {
        if constexpr (c < 15) out[r] = fma(val, v[c], out[r]);
        else if constexpr (kHasK && c < 19) out[r] = fma(-val, g[c - 15], out[r]);
    });
}

// out = Acl* v = A* v - B* (K v) at the touchdown knot of a guarded roll-out: cov_apply with the composite operator
// (touchdown_apply) in the block's place, f = -K v; g = K v (4)
template <bool kHasK>
__device__ __forceinline__ void cov_apply_touchdown(const TouchdownBlock& tb, const Model& M, const double* Kl, const double (&v)[15],
                                                    double (&out)[15], double (&g)[4]) {
    double f[4];
    k_times<kHasK>(Kl, v, g);
#pragma unroll
    for (int m = 0; m < 4; ++m) f[m] = -g[m];
    touchdown_apply<kHasK>(tb, M, v, f, out);
}

// The touchdown time's row against a symmetric matrix X, as lane j sees it.  r = t_x, with kWithK r = t_x - K' t_F on the free
// foot's force row of the K tile Kl; x(i): entry i of X's column j.  q = r' X r and q14 = (r + e_14)' X (r + e_14), the variances
// of tau and of the touchdown clock: lane j's share is r_j (r . x) and (r_j + [j == 14]) (r . x + x_14), and the row sums are
// the quadratic forms.  kSelect14: e_14 joins r_j by a select (the covariance sweep) instead of an added 0.0 or 1.0 (the Kalman
// sweep); the two differ in the sign of a zero, and each sweep keeps its bits.
template <bool kWithK, bool kSelect14, class Col>
__device__ __forceinline__ void touchdown_time_forms(const TouchdownBlock& tb, const KnotMode md, const double* Kl, Col x, int j,
                                                     bool own, double& q, double& q14) {
    const int iy = md.f2free ? 6 : 4, iv = md.f2free ? 13 : 11;
    [[maybe_unused]] const double* Kf = Kl + 16 * (md.f2free ? 3 : 1);
    double sc = 0.0, rj = 0.0, x14 = 0.0;
#pragma unroll
    for (int i = 0; i < 15; ++i) {
        double ri = (i == 4 || i == 6) ? ((i == iy) ? tb.ty : 0.0) : (i == 11 || i == 13) ? ((i == iv) ? tb.tv : 0.0) : 0.0;
        if constexpr (kWithK) ri = fma(-Kf[i], tb.tF, ri);
        const double xi = x(i);
        sc = fma(xi, ri, sc);
        rj = (i == j) ? ri : rj;
        x14 = xi;
    }
    q = row_sum16(own ? rj * sc : 0.0);
    const double r14 = kSelect14 ? (j == 14 ? rj + 1.0 : rj) : rj + ((j == 14) ? 1.0 : 0.0);
    q14 = row_sum16(own ? r14 * (sc + x14) : 0.0);
}

// Sigma_0 = Sigma0[b] (or the shared one), Sigma_{k+1} = Acl_k Sigma_k Acl_k' + diag(W) at Zout's knots; Sig gets every
// Sigma_k packed, mg the eight marginals of every knot (include/qln_evaluator.h).  Either may be null; which one is does
// not change the arithmetic of the other.
// kGuard (qln_tracking_covariance_guarded, with kModel): the blocks of the guarded sweeps at Zout's (x_k, u_k) -- the
// problem's model (plant_model), guard_mode's modes of the touchdown knot ks read with tau from event, and at ks the knot's
// two applications are the composite operator's (cov_apply_touchdown), Acl* = A* - B* K.  ev_var (null: not written) gets the
// variance of tau, c' Sigma_ks c with c = t_x - K_ks' t_F, and of the touchdown clock, the same with c + e_14
// (touchdown_time_forms).  Both are 0 without a touchdown.
template <bool kHasK, bool kModel, bool kGuard>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_tracking_covariance(BatchParams P, CovNoise Wn, const double* __restrict__ Zout,
                                                               const double* __restrict__ Kg, const double* __restrict__ Sigma0,
                                                               int sigma0_batch, double* __restrict__ Sig,
                                                               double* __restrict__ mg, const double* __restrict__ model,
                                                               const double* __restrict__ event, double* __restrict__ ev_var) {
    static_assert(kModel || !kGuard, "the guarded sweep runs on the kModel path");
    __shared__ double lds[kRows * kCRow];
    const Row16 r16 = row16_of(P);  // lane 15 shadows column 14 and writes nothing to the image
    const int ln = r16.ln, j = r16.j, bc = r16.bc, kt = r16.kt, im = r16.im, N = P.N;
    const bool own = r16.own, valid = r16.valid;
    const Model Mp = plant_model<kModel>(P, model, bc);
    const Model& M = kGuard ? Mp : r16.M;
    const GuardEvent ev = guard_event<kGuard>(event, bc, N);
    [[maybe_unused]] double var_tau = 0.0, var_clock = 0.0;
    double* L = lds + r16.row * kCRow;
    const Image15 Sg{L + kCImg, j, own};
    const double* __restrict__ Zb = Zout + (int64_t)bc * P.z_stride;
    const double* __restrict__ Kb = kHasK ? Kg + (int64_t)bc * (N - 1) * (QLN_TRACK_NU * QLN_NX) : nullptr;
    double* __restrict__ Sb = Sig ? Sig + (int64_t)bc * N * QLN_TRACK_P_NNZ : nullptr;
    double* __restrict__ Mb = mg ? mg + (int64_t)bc * N * QLN_TRACK_MARG_STRIDE : nullptr;

    int po[8], ko[4];
    packed_offsets(ln, po);
    k_offsets(ln, kCK, ko);
    double wj = 0.0;
#pragma unroll
    for (int i = 0; i < 15; ++i) wj = (i == j) ? Wn.w[i] : wj;

    // Sigma_0: the packed tile into the image's lower triangle
    const TileLane tl{ln, ln};  // this sweep has the scalar registers for hoisted tail masks (TileLane)
    {
        const double* __restrict__ S0 = Sigma0 + (int64_t)(sigma0_batch == 1 ? 0 : bc) * QLN_TRACK_P_NNZ;
        tile_fill(Sg.a, po, QLN_TRACK_P_NNZ, tl, [&](int t) { return S0[ln + 16 * t]; });
    }
    wave_lds_sync();
    double s[15];  // the lane's column of Sigma_k, carried from knot to knot
    Sg.column(s);

    // the clearance row's derivative entry needs a cosine: lane ln takes knot k0 + ln, once every sixteen knots
    auto clearance_derivatives = [&](int k0) {
        L[kCD + ln] = clearance_dtheta(Zb[20 * min(k0 + ln, N - 1) + 2], M.lb);
    };
    // Sigma_k and its marginals leave from the image's lower triangle; fv: the knot's force variances
    auto emit = [&](int k, const double (&fv)[4]) {
        const auto sat = [&](int o) { return Sg.a[o]; };
        if (Sb && valid) tile_store(Sb + (int64_t)k * QLN_TRACK_P_NNZ, po, QLN_TRACK_P_NNZ, tl, sat);
        if (Mb) marginals_store(Mb + (int64_t)k * QLN_TRACK_MARG_STRIDE, L[kCD + (k & 15)], fv, sat, Sg, valid, tl);
    };

    // Zout's knot (20 entries: lane ln takes ln and ln + 16) and the knot's K entries: requested one knot ahead
    double zn[2], kn[4];
    knot_load(Zb, ln, zn[0], zn[1]);
    if constexpr (kHasK) k_request(Kb, ln, kn);

    for (int k = 0; k < N - 1; ++k) {
        if (Mb && (k & 15) == 0) clearance_derivatives(k);
        L[kCZ + ln] = zn[0];
        if (ln < 4) L[kCZ + 16 + ln] = zn[1];
        if constexpr (kHasK) tile_fill(L, ko, QLN_TRACK_NU * QLN_NX, tl, [&](int t) { return kn[t]; });
        if (k + 1 < N - 1) {
            knot_load(Zb + 20 * (k + 1), ln, zn[0], zn[1]);
            if constexpr (kHasK) k_request(Kb + (int64_t)(k + 1) * (QLN_TRACK_NU * QLN_NX), ln, kn);
        }
        wave_lds_sync();  // the knot and the K tile are in place
        KnotMode md;
        if constexpr (kGuard) md = guard_mode(k, ev.ks, im);
        else md = knot_mode(k + 1, kt - 1, im);
        const bool td = kGuard && k == ev.ks;  // the touchdown knot: the composite operator in the block's place
        [[maybe_unused]] TouchdownBlock tb;
        StepBlock blk;
        if (td) {
            tb = touchdown_block_at(L + kCZ, M, md, ev.tau);
            if (ev_var) touchdown_time_forms<kHasK, true>(tb, md, L + kCK, [&](int i) { return s[i]; }, j, own, var_tau, var_clock);
        } else {
            blk = step_block(L + kCZ, md, M);
        }
        // Sigma_{k+1} = Acl Sigma_k Acl' + diag(W).  Behind the first application g = K Sigma column j, whose row sums against
        // K column j are the force variances (diag of M = G K'), and Sigma_k leaves.
        double g[4];
        congruence_from(
            Sg, s,
            [&](const double (&v)[15], double (&out)[15]) {
                if (td) cov_apply_touchdown<kHasK>(tb, M, L + kCK, v, out, g);
                else cov_apply<kHasK>(blk, L + kCK, v, out, g);
            },
            [&] {
                double fv[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    fv[m] = 0.0;
                    if constexpr (kHasK) {
                        if (Mb) fv[m] = row_sum16(own ? L[kCK + 16 * m + j] * g[m] : 0.0);
                    }
                }
                emit(k, fv);
            },
            wj);
        wave_lds_sync();  // Sigma_{k+1} is in place; the K tile and the knot may be rewritten
        Sg.column(s);
    }
    if (Mb && ((N - 1) & 15) == 0) {
        clearance_derivatives(N - 1);
        wave_lds_sync();
    }
    const double fv0[4] = {0.0, 0.0, 0.0, 0.0};
    emit(N - 1, fv0);
    if constexpr (kGuard) {
        if (ev_var && valid && ln < 2) ev_var[(int64_t)2 * bc + ln] = (ln == 0) ? var_tau : var_clock;
    }
}


// ---- k_tracking_kalman ----
// per-row LDS image (doubles): the P image [15][17] | the M image [15][17] | K [4][16] | the knot's 20 entries of Zout | the
// clearance derivatives of sixteen knots | the H tile [8][16], V in its column 15 | the L tile [15][8]
constexpr int kKP = 0, kKM = 256, kKK = 512, kKZ = kKK + 4 * 16, kKD = kKZ + 20, kKH = kKD + 16,
              kKL = kKH + QLN_TRACK_NY_MAX * 16, kKRow = kKL + 15 * QLN_TRACK_NY_MAX;
static_assert(kImgSize <= kKM - kKP && kImgSize <= kKK - kKM && kKZ % 2 == 0 && kKD % 2 == 0 && kKH % 2 == 0 && kKL % 2 == 0 &&
                  kKRow % 2 == 0,
              "the images fit; 16-byte aligned sections");

// the process variances and the measurement variances; the rows behind ny carry V = 1
struct KalmanNoise {
    double w[15], v[QLN_TRACK_NY_MAX];
};

// The Kalman filter and the LQG covariance along Zout (include/qln_evaluator.h): per knot the measurement update
// of the error covariance P (gain L_k, Joseph form), the estimate's covariance M_k = M^-_k + (P^-_k - P^+_k), and the two
// predictions P^-_{k+1} = A P^+ A' + diag(W) (cov_apply<false>) and M^-_{k+1} = Acl M Acl' (cov_apply<true>), on the blocks, the
// modes and the touchdown operator of k_tracking_covariance and in its mapping: one problem per row of sixteen lanes, lane j
// owns column j.  P and M each live in a padded image of their own, and the two recursions run one after the other within the
// knot through the images, so that neither holds the other's column in registers.  The update:
//   1. lane j forms G[:, j] = H P^-[:, j] (eight chains on broadcast reads of the H tile, one row in flight at a time);
//   2. S = G H' + diag(V): 36 row sums, the same bits in every lane, factored L D L' (no pivoting) by every lane alike;
//   3. lane j solves S x = G[:, j]: x is row j of the gain L = P^- H' S^-1, which goes to the L tile;
//   4. column j of (I - L H) P^- -> row j of the image; lane j reads row j of that back and forms column j of
//      P^+ = (I - L H) [.]' + L diag(V) L' as v - L (H v - V .* x), stored as row j of the image.  From there on only the lower
//      triangle is read, as in k_tracking_covariance.
// The kernel is compiled for eight measurement rows: the rows r >= ny of the H tile are zero rows and carry V = 1.  That
// changes no value -- S is block diagonal with an identity behind ny, those columns of L are exact zeros, and x + 0.0 * y == x
// for the finite y here -- and the call with ny rows gives the bits of the call with the zero rows written out.
// X_k = M_k + P^+_k is never stored in LDS: the packed tile and the marginals add the two images' entries where they leave.
// Without K (kHasK false) the call is the filter alone: no M image, Lgain and Pest only, and their bits are the same.
template <bool kHasK, bool kModel, bool kGuard>
__global__ __launch_bounds__(kWave) void k_tracking_kalman(BatchParams P, KalmanNoise Nz, const double* __restrict__ Zout,
                                                           const double* __restrict__ Kg, const double* __restrict__ Hg, int ny,
                                                           const double* __restrict__ Sigma0, int sigma0_batch,
                                                           double* __restrict__ Lg, double* __restrict__ Pe,
                                                           double* __restrict__ Sig, double* __restrict__ mg,
                                                           const double* __restrict__ model, const double* __restrict__ event,
                                                           double* __restrict__ ev_var) {
    static_assert(kModel || !kGuard, "the guarded sweep runs on the kModel path");
    constexpr int NY = QLN_TRACK_NY_MAX;
    __shared__ double lds[kRows * kKRow];
    const Row16 r16 = row16_of(P);  // lane 15 shadows column 14 and writes nothing to the images
    const int ln = r16.ln, j = r16.j, bc = r16.bc, kt = r16.kt, im = r16.im, N = P.N;
    const bool own = r16.own, valid = r16.valid;
    const Model Mp = plant_model<kModel>(P, model, bc);
    const Model& M = kGuard ? Mp : r16.M;
    const GuardEvent ev = guard_event<kGuard>(event, bc, N);
    [[maybe_unused]] double var_tau = 0.0, var_clock = 0.0;
    double* L = lds + r16.row * kKRow;
    const Image15 Pm{L + kKP, j, own}, Mm{L + kKM, j, own};
    const double* __restrict__ Zb = Zout + (int64_t)bc * P.z_stride;
    const double* __restrict__ Kb = kHasK ? Kg + (int64_t)bc * (N - 1) * (QLN_TRACK_NU * QLN_NX) : nullptr;
    double* __restrict__ Lb = Lg ? Lg + (int64_t)bc * N * (QLN_NX * ny) : nullptr;
    double* __restrict__ Pb = Pe ? Pe + (int64_t)bc * N * QLN_TRACK_P_NNZ : nullptr;
    double* __restrict__ Sb = (kHasK && Sig) ? Sig + (int64_t)bc * N * QLN_TRACK_P_NNZ : nullptr;
    double* __restrict__ Mb = (kHasK && mg) ? mg + (int64_t)bc * N * QLN_TRACK_MARG_STRIDE : nullptr;

    int po[8], ko[4], lo[8];
    packed_offsets(ln, po);
    k_offsets(ln, kKK, ko);
    gain_offsets(ln, ny, kKL, lo);
    double wj = 0.0;
#pragma unroll
    for (int i = 0; i < 15; ++i) wj = (i == j) ? Nz.w[i] : wj;
    const auto Hrow = [&](int r, int c) { return L[kKH + 16 * r + c]; };  // H(r, c); V_r in column 15
    const auto Lrow = [&](int i, int r) { return L[kKL + NY * i + r]; };  // the gain's L(i, r)

    // P^-_0 = Sigma0: the packed tile into the image's lower triangle; M^-_0 = 0; the H tile, zero rows behind ny
    {
        const double* __restrict__ S0 = Sigma0 + (int64_t)(sigma0_batch == 1 ? 0 : bc) * QLN_TRACK_P_NNZ;
        tile_fill(Pm.a, po, QLN_TRACK_P_NNZ, tile_lane(ln), [&](int t) { return S0[ln + 16 * t]; });
        if constexpr (kHasK) {
#pragma unroll
            for (int t = 0; t < 16; ++t) L[kKM + ln + 16 * t] = 0.0;
        }
#pragma unroll
        for (int r = 0; r < NY; ++r) L[kKH + 16 * r + ln] = own ? ((r < ny) ? Hg[15 * r + ln] : 0.0) : Nz.v[r];  // column 15: V
    }
    wave_lds_sync();

    auto clearance_derivatives = [&](int k0) {
        L[kKD + ln] = clearance_dtheta(Zb[20 * min(k0 + ln, N - 1) + 2], M.lb);
    };
    // the entry at offset o of P^+_k and of X_k = M_k + P^+_k (the filter alone: of P^+_k)
    const auto pat = [&](int o) { return Pm.a[o]; };
    const auto xat = [&](int o) {
        if constexpr (kHasK) return Mm.a[o] + Pm.a[o];
        else return Pm.a[o];
    };
    // the knot's outputs leave from the L tile and the images' lower triangles; fv: the knot's force variances
    auto emit = [&](int k, const double (&fv)[4]) {
        const TileLane tl = tile_lane(ln);
        if (Lb && valid) tile_store(Lb + (int64_t)k * (QLN_NX * ny), lo, QLN_NX * ny, tl, [&](int o) { return L[o]; });
        if (Pb && valid) tile_store(Pb + (int64_t)k * QLN_TRACK_P_NNZ, po, QLN_TRACK_P_NNZ, tl, pat);
        if constexpr (kHasK) {
            if (Sb && valid) tile_store(Sb + (int64_t)k * QLN_TRACK_P_NNZ, po, QLN_TRACK_P_NNZ, tl, xat);
            if (Mb) marginals_store(Mb + (int64_t)k * QLN_TRACK_MARG_STRIDE, L[kKD + (k & 15)], fv, xat, Pm, valid, tl);
        }
    };

    // Zout's knot and the knot's K entries: requested one knot ahead, as in k_tracking_covariance
    double zn[2] = {0.0, 0.0}, kn[4];
    if (N > 1) knot_load(Zb, ln, zn[0], zn[1]);
    if constexpr (kHasK) k_request(Kb, ln, kn);

    for (int k = 0; k < N; ++k) {
        const bool last = k == N - 1;  // the last knot has an update and no step
        if (Mb && (k & 15) == 0) clearance_derivatives(k);
        if (!last) {
            L[kKZ + ln] = zn[0];
            if (ln < 4) L[kKZ + 16 + ln] = zn[1];
            if constexpr (kHasK) tile_fill(L, ko, QLN_TRACK_NU * QLN_NX, tile_lane(ln), [&](int t) { return kn[t]; });
            if (k + 1 < N - 1) {
                knot_load(Zb + 20 * (k + 1), ln, zn[0], zn[1]);
                if constexpr (kHasK) k_request(Kb + (int64_t)(k + 1) * (QLN_TRACK_NU * QLN_NX), ln, kn);
            }
        }
        wave_lds_sync();  // the knot and the K tile are in place

        // ---- the measurement update: L_k, P^+_k and M_k ----
        double p[15], x[NY];
        Pm.column(p);
        {
            double G[NY];
            chain_rows(Hrow, p, G);
            double S[NY][NY], dd[NY], dinv[NY];  // the lower triangle; below the diagonal it becomes the unit factor
            double hj[NY];                         // column j of H
#pragma unroll
            for (int r = 0; r < NY; ++r) hj[r] = Hrow(r, j);
#pragma unroll
            for (int a = 0; a < NY; ++a) {
#pragma unroll
                for (int b = 0; b <= a; ++b) S[a][b] = row_sum16(own ? G[a] * hj[b] : 0.0);
                S[a][a] += Hrow(a, 15);
            }
#pragma unroll
            for (int c = 0; c < NY; ++c) {
                double w[NY], d = S[c][c];  // w: row c of the factor times D
#pragma unroll
                for (int q = 0; q < c; ++q) {
                    w[q] = S[c][q] * dd[q];
                    d = fma(-S[c][q], w[q], d);
                }
                dd[c] = d;
                dinv[c] = 1.0 / d;
#pragma unroll
                for (int i = c + 1; i < NY; ++i) {
                    double t = S[i][c];
#pragma unroll
                    for (int q = 0; q < c; ++q) t = fma(-S[i][q], w[q], t);
                    S[i][c] = t * dinv[c];
                }
            }
            // S x = G[:, j]: forward, the diagonal, backward
#pragma unroll
            for (int i = 0; i < NY; ++i) {
                double t = G[i];
#pragma unroll
                for (int q = 0; q < i; ++q) t = fma(-S[i][q], x[q], t);
                x[i] = t;
            }
#pragma unroll
            for (int i = 0; i < NY; ++i) x[i] *= dinv[i];
#pragma unroll
            for (int i = NY - 2; i >= 0; --i) {
#pragma unroll
                for (int q = i + 1; q < NY; ++q) x[i] = fma(-S[q][i], x[q], x[i]);
            }
            if (own) {
#pragma unroll
                for (int r = 0; r < NY; ++r) L[kKL + NY * j + r] = x[r];
            }
            wave_lds_sync();  // the L tile is in place, and every lane holds its column of P^-
            double u[15];
            chain_rows_sub(Lrow, G, p, u);  // column j of (I - L H) P^- -> row j of the image
            Pm.store_row(u);
        }
        wave_lds_sync();
        {
            double vt[15], t[NY], out[15];
            Pm.transposed(vt);
            chain_rows(Hrow, vt, t);
#pragma unroll
            for (int r = 0; r < NY; ++r) t[r] = fma(-Hrow(r, 15), x[r], t[r]);  // H v - V .* (row j of L): the Joseph form's two terms share L
            chain_rows_sub(Lrow, t, vt, out);
            wave_lds_sync();  // every lane holds its row: P^+ may overwrite the image
            Pm.store_row(out);
        }
        wave_lds_sync();
        // only the lower triangle of P^+_k is read from here on; M_k = M^-_k + (P^-_k - P^+_k), entry by entry
        if constexpr (kHasK) {
            double m[15];
#pragma unroll
            for (int c = 0; c < 15; ++c) m[c] = Mm.a[Mm.sym(c)] + (p[c] - Pm.a[Pm.sym(c)]);
            wave_lds_sync();  // M^- has been read
            Mm.store_row(m);
            wave_lds_sync();
        }
        const double fv0[4] = {0.0, 0.0, 0.0, 0.0};
        if (last) {
            emit(k, fv0);
            break;
        }

        KnotMode md;
        if constexpr (kGuard) md = guard_mode(k, ev.ks, im);
        else md = knot_mode(k + 1, kt - 1, im);
        // The two predictions of the knot, M's first (its K m gives the force variances, so the knot's outputs leave behind its
        // first application).  apply(hasK, v, out, g): out = (A - B K) v or A v on the knot's operator.  The knot's body exists
        // once per operator -- the step block's and the touchdown knot's -- so that neither form's values stay live across the
        // other's applications; the hand-offs through LDS stay inside a row, whose sixteen lanes take the same form.
        auto predict = [&](auto apply) {
            double g[4];
            if constexpr (kHasK) {
                congruence(
                    Mm, [&](const double (&v)[15], double (&out)[15]) { apply(std::true_type{}, v, out, g); },
                    [&] {
                        double fv[4] = {0.0, 0.0, 0.0, 0.0};
                        if (Mb) {
#pragma unroll
                            for (int q = 0; q < 4; ++q) fv[q] = row_sum16(own ? L[kKK + 16 * q + j] * g[q] : 0.0);
                        }
                        emit(k, fv);
                    });
            } else {
                emit(k, fv0);
            }
            // P^-_{k+1} = A P^+_k A' + diag(W): k_tracking_covariance's open-loop knot
            congruence(Pm, [&](const double (&v)[15], double (&out)[15]) { apply(std::false_type{}, v, out, g); }, [] {}, wj);
        };
        if (kGuard && k == ev.ks) {  // the touchdown knot: the composite operator in the block's place
            const TouchdownBlock tb = touchdown_block_at(L + kKZ, M, md, ev.tau);
            // the variances of tau and of the touchdown clock: c' M c + t_x' P^+ t_x with c = t_x - K' t_F, then with e_14 added
            // to both; lane j takes column j of M against c and of P^+ against t_x (touchdown_time_forms)
            if constexpr (kHasK) {
                if (ev_var) {
                    int je = j;  // an opaque copy, as a tile's lane: the fifteen masks i == j are formed here, not ahead of the loop
                    asm volatile("" : "+v"(je));
                    double qm, qm14, qp, qp14;
                    touchdown_time_forms<true, false>(tb, md, L + kKK, [&](int i) { return Mm.a[Mm.sym(i)]; }, je, own, qm, qm14);
                    touchdown_time_forms<false, false>(tb, md, L + kKK, [&](int i) { return Pm.a[Pm.sym(i)]; }, je, own, qp, qp14);
                    var_tau = qm + qp;
                    var_clock = qm14 + qp14;
                }
            }
            predict([&](auto hasK, const double (&v)[15], double (&out)[15], double (&g)[4]) {
                cov_apply_touchdown<decltype(hasK)::value>(tb, M, L + kKK, v, out, g);
            });
        } else {
            const StepBlock blk = step_block(L + kKZ, md, M);
            predict([&](auto hasK, const double (&v)[15], double (&out)[15], double (&g)[4]) {
                cov_apply<decltype(hasK)::value>(blk, L + kKK, v, out, g);
            });
        }
        wave_lds_sync();  // both images hold the priors of knot k + 1; the K tile and the knot may be rewritten
    }
    if constexpr (kGuard) {
        if (kHasK && ev_var && valid && ln < 2) ev_var[(int64_t)2 * bc + ln] = (ln == 0) ? var_tau : var_clock;
    }
}


// ---- k_tracking_kalman_jvp ----
// per-row LDS image (doubles): the Pd image [15][17] | the knot's 20 entries of Zout | the H tile [8][16], 1/V in its column 15 |
// two L tiles [15][8] (the knot's, and the next knot's while it is staged) | the Ld tile [15][8]
constexpr int kJTile = 15 * QLN_TRACK_NY_MAX;
constexpr int kJP = 0, kJZ = 256, kJH = kJZ + 20, kJL = kJH + QLN_TRACK_NY_MAX * 16, kJLd = kJL + 2 * kJTile, kJRow = kJLd + kJTile;
static_assert(kImgSize <= kJZ - kJP && kJZ % 2 == 0 && kJH % 2 == 0 && kJL % 2 == 0 && kJLd % 2 == 0 && kJRow % 2 == 0,
              "the image fits; 16-byte aligned sections");

// the tangents of the process and the measurement variances, and 1 / V; the rows behind ny carry 1 / V = 1 and V_dot = 0
struct KalmanNoiseDot {
    double wd[15], iv[QLN_TRACK_NY_MAX], vd[QLN_TRACK_NY_MAX];
};

// The forward sweep through k_tracking_kalman's design (include/qln_evaluator.h): how the gains L_k, the error
// covariances P^+_k and log det S_k move along (Sigma0_dot, W_dot, V_dot), at the gains the design returned and nothing else of
// it -- at the optimal gain the Joseph form is stationary in L, so P^+'s tangent carries no L_dot term.  In k_tracking_kalman's
// mapping, one problem per row of sixteen lanes, lane j owns column j, and one padded image holds Pd.  Per knot:
//   1. lane j forms Gd[:, j] = H Pd^-[:, j] and at once the first pass of the Joseph form, column j of (I - L H) Pd^-, so that
//      its column of Pd^- is dead before the rest;
//   2. Sd = Gd H' + diag(V_dot): 36 row sums, the same bits in every lane, each consumed where it is formed -- its share of
//      tr(V^-1 Sd) and of row j of L Sd -- so that Sd is never held;
//   3. d log det S = tr(Sinv Sd) = tr(V^-1 Sd) - tr(V^-1 H L Sd) with Sinv = diag(1/V) (I - H L): lane j's share of the second
//      trace is sum_a H(a, j) / V_a (L Sd)(j, a), one more row sum.  Row j of Ld = T Sinv, T = Pd^- H' - L Sd: with
//      tv = T(j, :) ./ V it is tv - (tv H) L, two dense chains on broadcast reads of the two tiles, and leaves through the Ld
//      tile.  No entry of H L is formed;
//   4. Pd^+ = (I - L H) [.]' + L diag(V_dot) L': k_tracking_kalman's second pass with V_dot where V stands;
//   5. Pd^-_{k+1} = A Pd^+ A' + diag(W_dot): k_tracking_covariance's open-loop knot (the touchdown knot: the composite operator).
// L_{k+1} is requested at the top of knot k and staged into the other L tile behind the update, so that its eight entries per lane
// are not held across the prediction, where the step block peaks.  Compiled for eight measurement rows as k_tracking_kalman: zero
// rows of H and zero columns of L behind ny change no value.  Nothing here divides or factors, and Pd may be indefinite.
template <bool kModel, bool kGuard>
__device__ __forceinline__ void kalman_jvp_sweep(const BatchParams& P, const KalmanNoiseDot& Nz, const double* __restrict__ Zout,
                                                 const double* __restrict__ Lg, const double* __restrict__ Hg, int ny,
                                                 const double* __restrict__ Sigma0d, int sigma0_batch, double* __restrict__ Ldg,
                                                 double* __restrict__ Pdg, double* __restrict__ ldg,
                                                 const double* __restrict__ model, const double* __restrict__ event) {
    static_assert(kModel || !kGuard, "the guarded sweep runs on the kModel path");
    constexpr int NY = QLN_TRACK_NY_MAX;
    __shared__ double lds[kRows * kJRow];
    const Row16 r16 = row16_of(P);  // lane 15 shadows column 14 and writes nothing to the image
    const int ln = r16.ln, j = r16.j, bc = r16.bc, kt = r16.kt, im = r16.im, N = P.N;
    const bool own = r16.own, valid = r16.valid;
    const Model Mp = plant_model<kModel>(P, model, bc);
    const Model& M = kGuard ? Mp : r16.M;
    const GuardEvent ev = guard_event<kGuard>(event, bc, N);
    double* L = lds + r16.row * kJRow;
    const Image15 Pm{L + kJP, j, own};
    const int gn = QLN_NX * ny;  // a knot's gain entries
    const double* __restrict__ Zb = Zout + (int64_t)bc * P.z_stride;
    const double* __restrict__ Lb = Lg + (int64_t)bc * N * gn;
    double* __restrict__ Ldb = Ldg ? Ldg + (int64_t)bc * N * gn : nullptr;
    double* __restrict__ Pdb = Pdg ? Pdg + (int64_t)bc * N * QLN_TRACK_P_NNZ : nullptr;
    double* __restrict__ ldb = ldg ? ldg + (int64_t)bc * N : nullptr;

    int po[8], lo[8];
    packed_offsets(ln, po);
    gain_offsets(ln, ny, kJL, lo);
    double wj = 0.0;
#pragma unroll
    for (int i = 0; i < 15; ++i) wj = (i == j) ? Nz.wd[i] : wj;
    const auto Hrow = [&](int r, int c) { return L[kJH + 16 * r + c]; };  // H(r, c); 1 / V_r in column 15

    // Pd^-_0 = Sigma0_dot (null: zero); the three gain tiles zero, so the columns behind ny stay zero; the H tile, zero rows behind ny
    {
        if (Sigma0d) {
            const double* __restrict__ S0 = Sigma0d + (int64_t)(sigma0_batch == 1 ? 0 : bc) * QLN_TRACK_P_NNZ;
            tile_fill(Pm.a, po, QLN_TRACK_P_NNZ, tile_lane(ln), [&](int t) { return S0[ln + 16 * t]; });
        } else {
#pragma unroll
            for (int t = 0; t < 16; ++t) L[kJP + ln + 16 * t] = 0.0;
        }
#pragma unroll
        for (int t = 0; t < (3 * kJTile + 15) / 16; ++t)
            if (ln + 16 * t < 3 * kJTile) L[kJL + ln + 16 * t] = 0.0;
#pragma unroll
        for (int r = 0; r < NY; ++r) L[kJH + 16 * r + ln] = own ? ((r < ny) ? Hg[15 * r + ln] : 0.0) : Nz.iv[r];
    }
    wave_lds_sync();

    // a knot's gain entries ln + 16 t, requested one knot ahead like the knot itself, and staged into tile k & 1
    auto gain_request = [&](int k, double (&lq)[8]) {
        const double* __restrict__ Lk = Lb + (int64_t)k * gn;
#pragma unroll
        for (int t = 0; t < 8; ++t) lq[t] = Lk[min(ln + 16 * t, gn - 1)];
    };
    double zn[2] = {0.0, 0.0}, lq[8];
    if (N > 1) knot_load(Zb, ln, zn[0], zn[1]);
    gain_request(0, lq);
    tile_fill(L, lo, gn, tile_lane(ln), [&](int t) { return lq[t]; });

    for (int k = 0; k < N; ++k) {
        const double* Lt = L + kJL + kJTile * (k & 1);
        const auto Lrow = [&](int i, int r) { return Lt[NY * i + r]; };  // the gain's L(i, r)
        const bool last = k == N - 1;  // the last knot has an update and no step
        if (!last) {
            L[kJZ + ln] = zn[0];
            if (ln < 4) L[kJZ + 16 + ln] = zn[1];
            if (k + 1 < N - 1) knot_load(Zb + 20 * (k + 1), ln, zn[0], zn[1]);
        }
        if (!last) gain_request(k + 1, lq);
        wave_lds_sync();  // the knot and the L tile are in place

        // ---- the update's tangent: Ld_k, d log det S_k and Pd^+_k ----
        double Gd[NY], ldot;
        {
            double p[15], u[15];
            Pm.column(p);
            chain_rows(Hrow, p, Gd);
            chain_rows_sub(Lrow, Gd, p, u);  // column j of (I - L H) Pd^- -> row j of the image
            wave_lds_sync();                 // every lane holds its column of Pd^-
            Pm.store_row(u);
        }
        {
            double hj[NY], lj[NY], LS[NY], tv[NY], ld[NY];
#pragma unroll
            for (int r = 0; r < NY; ++r) {
                hj[r] = Hrow(r, j);
                lj[r] = Lrow(j, r);  // row j of L
            }
            double tr = 0.0;
#pragma unroll
            for (int r = 0; r < NY; ++r) LS[r] = 0.0;
            // Sd's lower triangle, entry by entry: what it adds to tr(V^-1 Sd) and to row j of L Sd (Sd is symmetric)
#pragma unroll
            for (int a = 0; a < NY; ++a) {
#pragma unroll
                for (int b = 0; b < a; ++b) {
                    const double sd = row_sum16(own ? Gd[a] * hj[b] : 0.0);
                    LS[b] = fma(lj[a], sd, LS[b]);
                    LS[a] = fma(lj[b], sd, LS[a]);
                }
                const double sd = row_sum16(own ? Gd[a] * hj[a] : 0.0) + Nz.vd[a];
                tr = fma(Hrow(a, 15), sd, tr);
                LS[a] = fma(lj[a], sd, LS[a]);
            }
            // the second trace's share of lane j, and tv = T(j, :) ./ V
            double c = 0.0;
#pragma unroll
            for (int a = 0; a < NY; ++a) {
                const double iva = Hrow(a, 15);
                c = fma(hj[a] * iva, LS[a], c);
                tv[a] = (Gd[a] - LS[a]) * iva;
            }
            ldot = tr - row_sum16(own ? c : 0.0);
            double w[15];
            chain_rows([&](int i, int a) { return Hrow(a, i); }, tv, w);          // tv H
            chain_rows_sub([&](int b, int i) { return Lrow(i, b); }, w, tv, ld);  // tv - (tv H) L
            if (own) {
#pragma unroll
                for (int r = 0; r < NY; ++r) L[kJLd + NY * j + r] = ld[r];
            }
        }
        wave_lds_sync();
        {
            double vt[15], t[NY], out[15];
            Pm.transposed(vt);
            chain_rows(Hrow, vt, t);
#pragma unroll
            for (int r = 0; r < NY; ++r) t[r] = fma(-Nz.vd[r], Lrow(j, r), t[r]);  // H v - V_dot .* (row j of L)
            chain_rows_sub(Lrow, t, vt, out);
            wave_lds_sync();  // every lane holds its row: Pd^+ may overwrite the image
            Pm.store_row(out);
        }
        // L_{k+1} has had the update to arrive: into the other tile, which knot k - 1 read last
        if (!last) tile_fill(L + kJTile * ((k + 1) & 1), lo, gn, tile_lane(ln), [&](int t) { return lq[t]; });
        wave_lds_sync();
        // only the lower triangle of Pd^+_k is read from here on; the knot's outputs leave from it and from the Ld tile
        {
            const TileLane tl = tile_lane(ln);
            if (Ldb && valid) tile_store(Ldb + (int64_t)k * gn, lo, gn, tl, [&](int o) { return L[o + (kJLd - kJL)]; });
            if (Pdb && valid) tile_store(Pdb + (int64_t)k * QLN_TRACK_P_NNZ, po, QLN_TRACK_P_NNZ, tl, [&](int o) { return Pm.a[o]; });
            if (ldb && valid && ln == 0) ldb[k] = ldot;
        }
        if (last) break;

        // Pd^-_{k+1} = A Pd^+_k A' + diag(W_dot): k_tracking_covariance's open-loop knot on this image
        KnotMode md;
        if constexpr (kGuard) md = guard_mode(k, ev.ks, im);
        else md = knot_mode(k + 1, kt - 1, im);
        double g[4];
        if (kGuard && k == ev.ks) {  // the touchdown knot: the composite operator in the block's place
            const TouchdownBlock tb = touchdown_block_at(L + kJZ, M, md, ev.tau);
            congruence(
                Pm, [&](const double (&v)[15], double (&out)[15]) { cov_apply_touchdown<false>(tb, M, nullptr, v, out, g); }, [] {},
                wj);
        } else {
            const StepBlock blk = step_block(L + kJZ, md, M);
            congruence(
                Pm, [&](const double (&v)[15], double (&out)[15]) { cov_apply<false>(blk, nullptr, v, out, g); }, [] {}, wj);
        }
        wave_lds_sync();  // the image holds the prior's tangent of knot k + 1; the L tile and the knot may be rewritten
    }
}

// The knot-scheduled form is asked for two waves per SIMD, which it fits without spills (its step block is the light one); the
// guarded form stays at one, as k_tracking_kalman's: profiles/tracking_kalman_jvp_resource_usage.txt.
template <bool kModel, bool kGuard>
__global__ __launch_bounds__(kWave) void k_tracking_kalman_jvp(BatchParams P, KalmanNoiseDot Nz, const double* __restrict__ Zout,
                                                               const double* __restrict__ Lg, const double* __restrict__ Hg, int ny,
                                                               const double* __restrict__ Sigma0d, int sigma0_batch,
                                                               double* __restrict__ Ldg, double* __restrict__ Pdg,
                                                               double* __restrict__ ldg, const double* __restrict__ model,
                                                               const double* __restrict__ event) {
    kalman_jvp_sweep<kModel, kGuard>(P, Nz, Zout, Lg, Hg, ny, Sigma0d, sigma0_batch, Ldg, Pdg, ldg, model, event);
}
template <>
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_tracking_kalman_jvp<false, false>(
    BatchParams P, KalmanNoiseDot Nz, const double* __restrict__ Zout, const double* __restrict__ Lg, const double* __restrict__ Hg,
    int ny, const double* __restrict__ Sigma0d, int sigma0_batch, double* __restrict__ Ldg, double* __restrict__ Pdg,
    double* __restrict__ ldg, const double* __restrict__ model, const double* __restrict__ event) {
    kalman_jvp_sweep<false, false>(P, Nz, Zout, Lg, Hg, ny, Sigma0d, sigma0_batch, Ldg, Pdg, ldg, model, event);
}


// ---- k_landing_smoother ----
// per-row LDS image (doubles): the P^+ image [15][17] (Ps_k leaves from it) | the Theta image [15][17] | the L tile [15][8] | the
// H tile [8][16], 1/V in its column 15 | the knot's 20 entries of Ztraj | q [16] | r [16] | the knot's innovations [8].
// This kernel keeps its own statement of the knot, on qln_image15.h's stride and sym_at alone: on the shared accessors, tiles,
// chains and congruence step its guarded form launched 0.3 % slower (profiles/sym_image_timing.txt), and any of the shared offset
// tables, guard_event or touchdown_block_at changes its device assembly, which as it stands is the one it had before that header.
constexpr int kSStr = kImgStr, kSP = 0, kSTh = 256, kSL = 512, kSH = kSL + 15 * QLN_TRACK_NY_MAX, kSZ = kSH + QLN_TRACK_NY_MAX * 16,
              kSQ = kSZ + 20, kSR = kSQ + 16, kSI = kSR + 16, kSRow = kSI + QLN_TRACK_NY_MAX;
static_assert(15 * kSStr <= kSTh - kSP && 15 * kSStr <= kSL - kSTh && kSH % 2 == 0 && kSZ % 2 == 0 && kSQ % 2 == 0 && kSR % 2 == 0 &&
                  kSI % 2 == 0 && kSRow % 2 == 0 && kSRow <= kKRow,
              "the images fit; 16-byte aligned sections; within the Kalman kernel's budget");

// the reciprocals of the measurement variances; the rows behind ny carry 1
struct SmootherNoise {
    double iv[QLN_TRACK_NY_MAX];
};

// out = A_k' v on the knot's block: cov_apply's open-loop application with rows and columns exchanged
__device__ __forceinline__ void block_apply_t(const StepBlock& blk, const double (&v)[15], double (&out)[15]) {
#pragma unroll
    for (int i = 0; i < 15; ++i) out[i] = 0.0;
    StepBlock bk = blk;
    asm volatile("" : "+v"(bk.wAt), "+v"(bk.wBt), "+v"(bk.wAw));  // as in cov_apply: the products are formed per application
    for_each_rollout_entry(bk, [&](auto r, auto c, double val) {
        if constexpr (c < 15) out[c] = fma(val, v[r], out[c]);
    });
}

// The fixed-interval smoother of a flown landing (include/qln_evaluator.h): the modified Bryson-Frazier sweep,
// backward from knot N-1 on the filter's own gains L_k and covariances P^+_k, which inverts nothing.  The mapping of
// k_tracking_kalman and of the Riccati sweep: one problem per row of sixteen lanes, lane j owns column j of P^+_k, of Theta and
// of every product; the blocks A_k, the modes and the touchdown knot's operator are those sweeps', applied transposed
// (block_apply_t, touchdown_apply_t).  Per knot k = N-1 .. 0:
//   1. P^+_k, L_k, innov_k and Ztraj's knot k-1 (loaded one knot ahead) go to LDS; lane j reads its column p of P^+_k;
//   2. Xs_k[j] = Xhat_k[j] + p . q (q: fifteen broadcast reads);  Ps_k column j = p - P^+ (Theta p): two dense chains on
//      broadcast reads of the images' lower triangles, written into the P image's lower triangle, which leaves packed;
//   3. r_k[j] = q_j + H[:, j] . ((innov - H (L innov)) ./ V - L'q): lane j's row of L against innov, sixteen row sums;
//      Lambda_k column j = Theta c + H' (V^-1 (H c) - L' (Theta c)),  c = column j of I - L H: chains on broadcast reads of
//      the L tile, the Theta image and the H tile; its entries on and below the diagonal replace the Theta image's;
//   4. q_{k-1} = A' r (every lane alike, lane 0 writes it) and Theta_{k-1} = A' Lambda A by two transposed applications with a
//      transpose through the image between them, as the covariance sweep's knot.  The body of 4 exists once per operator form.
// The kernel is compiled for eight measurement rows, as k_tracking_kalman: zero rows of H with 1/V = 1 and zero columns of L
// behind ny.  The vector recursion (q, r, Xs) and the matrix recursion (Theta, Lambda, Ps) share no value: each runs only when
// its output is asked for, and neither changes the other's bits.
template <bool kGuard>
__global__ __launch_bounds__(kWave) void k_landing_smoother(BatchParams P, SmootherNoise Nz, const double* __restrict__ Ztraj,
                                                            const double* __restrict__ Lg, const double* __restrict__ Pe,
                                                            const double* __restrict__ Hg, int ny, const double* __restrict__ Xhat,
                                                            const double* __restrict__ innov, double* __restrict__ Xs,
                                                            double* __restrict__ Ps, const double* __restrict__ model,
                                                            const double* __restrict__ event) {
    constexpr int NY = QLN_TRACK_NY_MAX;
    // rows of a dense chain whose broadcast reads are in flight together, held apart by an empty asm as K's rows in cov_apply.
    // One wave per SIMD runs here, so a knot waits on LDS latency row by row; with three rows in flight the compiler hoisted
    // the reads of whole chains and both instantiations went to scratch (152 and 92 bytes per lane), so it stays at one.
    constexpr int kFlight = 1;
    __shared__ double lds[kRows * kSRow];
    const Row16 r16 = row16_of(P);  // lane 15 shadows column 14 and writes nothing to the images
    const int ln = r16.ln, j = r16.j, bc = r16.bc, kt = r16.kt, im = r16.im, N = P.N;
    const bool own = r16.own, valid = r16.valid;
    const Model Mp = plant_model<kGuard>(P, model, bc);
    const Model& M = kGuard ? Mp : r16.M;
    [[maybe_unused]] int ks = -1;
    [[maybe_unused]] double tau = 0.0;
    if constexpr (kGuard) {
        ks = guard_knot(event[(int64_t)QLN_TOUCHDOWN_INFO_STRIDE * bc], N);
        tau = event[(int64_t)QLN_TOUCHDOWN_INFO_STRIDE * bc + 1];
    }
    double* L = lds + r16.row * kSRow;
    const bool wantX = Xs != nullptr, wantP = Ps != nullptr;
    const double* __restrict__ Zb = Ztraj + (int64_t)bc * P.z_stride;
    const double* __restrict__ Lb = Lg + (int64_t)bc * N * (QLN_NX * ny);
    const double* __restrict__ Pb = Pe + (int64_t)bc * N * QLN_TRACK_P_NNZ;
    const double* __restrict__ Xb = Xhat + (int64_t)bc * N * QLN_NX;
    const double* __restrict__ Ib = innov + (int64_t)bc * N * ny;
    double* __restrict__ Xo = wantX ? Xs + (int64_t)bc * N * QLN_NX : nullptr;
    double* __restrict__ Po = wantP ? Ps + (int64_t)bc * N * QLN_TRACK_P_NNZ : nullptr;

    // where the packed entries ln + 16 t lie in an image's lower triangle (relative to the image) and the entries of a knot's
    // [15][ny] gain in the L tile (rows of eight), as in k_tracking_kalman
    int po[8], lo[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int i = min(ln + 16 * t, QLN_TRACK_P_NNZ - 1);
        int r = 0;
#pragma unroll
        for (int q = 1; q < 15; ++q) r += (i >= q * (q + 1) / 2) ? 1 : 0;
        po[t] = kSStr * r + (i - r * (r + 1) / 2);
        const int g = min(ln + 16 * t, QLN_NX * ny - 1), gr = g / ny;
        lo[t] = kSL + NY * gr + (g - ny * gr);
    }
    const int rowj = kSStr * j, colj = j;
    auto sym = [&](int c) { return (c <= j) ? rowj + c : colj + kSStr * c; };  // relative to the image

    // q_{N-1} = 0, Theta_{N-1} = 0; the H tile, zero rows behind ny; the L tile's columns and the innovations behind ny stay 0.0
    {
#pragma unroll
        for (int t = 0; t < 16; ++t) L[kSTh + ln + 16 * t] = 0.0;
#pragma unroll
        for (int t = 0; t < 8; ++t)
            if (ln + 16 * t < 15 * NY) L[kSL + ln + 16 * t] = 0.0;
#pragma unroll
        for (int r = 0; r < NY; ++r) L[kSH + 16 * r + ln] = own ? ((r < ny) ? Hg[15 * r + ln] : 0.0) : Nz.iv[r];  // column 15: 1/V
        L[kSQ + ln] = 0.0;
        L[kSR + ln] = 0.0;
        if (ln < NY) L[kSI + ln] = 0.0;
    }

    // the knot's inputs, requested one knot ahead: P^+_k and L_k (entries ln + 16 t), Xhat_k[j], innov_k[ln] and Ztraj's knot k-1
    double pn[8], gn[8], xn = 0.0, in = 0.0, zn[2] = {0.0, 0.0};
    auto request = [&](int k) {
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            pn[t] = Pb[(int64_t)k * QLN_TRACK_P_NNZ + min(ln + 16 * t, QLN_TRACK_P_NNZ - 1)];
            gn[t] = Lb[(int64_t)k * (QLN_NX * ny) + min(ln + 16 * t, QLN_NX * ny - 1)];
        }
        if (wantX) {
            xn = Xb[(int64_t)k * QLN_NX + j];
            in = Ib[(int64_t)k * ny + min(ln, ny - 1)];
        }
        if (k > 0) knot_load(Zb + 20 * (k - 1), ln, zn[0], zn[1]);
    };
    request(N - 1);
    wave_lds_sync();

    for (int k = N - 1; k >= 0; --k) {
        // ---- 1. the knot's inputs into LDS ----
        {
            int le = ln;  // an opaque copy, as in k_tracking_kalman's emit: the tails' lane masks are formed here
            asm volatile("" : "+v"(le));
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                if (le + 16 * t < QLN_TRACK_P_NNZ) L[kSP + po[t]] = pn[t];
                if (le + 16 * t < QLN_NX * ny) L[lo[t]] = gn[t];
            }
            if (wantX && le < ny) L[kSI + ln] = in;
            if (k > 0) {
                L[kSZ + ln] = zn[0];
                if (le < 4) L[kSZ + 16 + ln] = zn[1];
            }
        }
        const double xh = xn;
        if (k > 0) request(k - 1);
        wave_lds_sync();  // the knot's tiles are in place

        // ---- 2. Xs_k and Ps_k ----
        {
            double p[15];
#pragma unroll
            for (int c = 0; c < 15; ++c) p[c] = L[kSP + sym(c)];
            if (wantX) {
                double acc = p[0] * L[kSQ];
#pragma unroll
                for (int c = 1; c < 15; ++c) acc = fma(p[c], L[kSQ + c], acc);
                if (valid && own) Xo[(int64_t)k * QLN_NX + j] = xh + acc;
            }
            if (wantP) {
                double u[15], ps[15];
#pragma unroll
                for (int i = 0; i < 15; ++i) {
                    double acc = L[kSTh + sym_at(i, 0)] * p[0];
#pragma unroll
                    for (int c = 1; c < 15; ++c) acc = fma(L[kSTh + sym_at(i, c)], p[c], acc);
                    if (i % kFlight == kFlight - 1) asm volatile("" : "+v"(acc) : : "memory");  // kFlight rows in flight at a time
                    u[i] = acc;
                }
#pragma unroll
                for (int i = 0; i < 15; ++i) {
                    double acc = L[kSP + sym_at(i, 0)] * u[0];
#pragma unroll
                    for (int c = 1; c < 15; ++c) acc = fma(L[kSP + sym_at(i, c)], u[c], acc);
                    if (i % kFlight == kFlight - 1) asm volatile("" : "+v"(acc) : : "memory");
                    ps[i] = p[i] - acc;
                }
                wave_lds_sync();  // every lane has read P^+_k: Ps_k may overwrite the image
                if (own) {  // column j on and below the diagonal: the lower triangle of the stated expression
#pragma unroll
                    for (int i = 0; i < 15; ++i)
                        if (i >= j) L[kSP + kSStr * i + j] = ps[i];
                }
                wave_lds_sync();
                if (valid) {
                    int le = ln;
                    asm volatile("" : "+v"(le));
                    double* __restrict__ o = Po + (int64_t)k * QLN_TRACK_P_NNZ;
#pragma unroll
                    for (int t = 0; t < 8; ++t)
                        if (le + 16 * t < QLN_TRACK_P_NNZ) o[ln + 16 * t] = L[kSP + po[t]];
                }
            }
        }
        if (k == 0) break;

        // ---- 3. r_k and Lambda_k ----
        {
            double x[NY], hj[NY];  // row j of L_k, column j of H
#pragma unroll
            for (int r = 0; r < NY; ++r) {
                x[r] = L[kSL + NY * j + r];
                hj[r] = L[kSH + 16 * r + j];
            }
            if (wantX) {
                double y = x[0] * L[kSI];  // (L innov)[j]
#pragma unroll
                for (int r = 1; r < NY; ++r) y = fma(x[r], L[kSI + r], y);
                const double qj = L[kSQ + j];
                double rj = qj;
#pragma unroll
                for (int r = 0; r < NY; ++r) {
                    const double e = L[kSI + r] - row_sum16(own ? hj[r] * y : 0.0);  // the post-fit residual
                    const double lq = row_sum16(own ? x[r] * qj : 0.0);             // (L'q)[r]
                    rj = fma(hj[r], fma(e, L[kSH + 16 * r + 15], -lq), rj);
                }
                if (own) L[kSR + j] = rj;
            }
            if (wantP) {
                double cj[15], u[15], w[NY];
                int je = j;  // an opaque copy: the fifteen masks i == j are formed here, not ahead of the loop
                asm volatile("" : "+v"(je));
#pragma unroll
                for (int i = 0; i < 15; ++i) {
                    double acc = (i == je) ? 1.0 : 0.0;
#pragma unroll
                    for (int r = 0; r < NY; ++r) acc = fma(-L[kSL + NY * i + r], hj[r], acc);
                    if (i % kFlight == kFlight - 1) asm volatile("" : "+v"(acc) : : "memory");
                    cj[i] = acc;
                }
#pragma unroll
                for (int i = 0; i < 15; ++i) {
                    double acc = L[kSTh + sym_at(i, 0)] * cj[0];
#pragma unroll
                    for (int c = 1; c < 15; ++c) acc = fma(L[kSTh + sym_at(i, c)], cj[c], acc);
                    if (i % kFlight == kFlight - 1) asm volatile("" : "+v"(acc) : : "memory");
                    u[i] = acc;
                }
#pragma unroll
                for (int r = 0; r < NY; ++r) {
                    double hc = L[kSH + 16 * r] * cj[0], lu = L[kSL + r] * u[0];
#pragma unroll
                    for (int c = 1; c < 15; ++c) {
                        hc = fma(L[kSH + 16 * r + c], cj[c], hc);
                        lu = fma(L[kSL + NY * c + r], u[c], lu);
                    }
                    asm volatile("" : "+v"(hc), "+v"(lu) : : "memory");
                    w[r] = fma(hc, L[kSH + 16 * r + 15], -lu);
                }
#pragma unroll
                for (int i = 0; i < 15; ++i) {
                    double acc = u[i];
#pragma unroll
                    for (int r = 0; r < NY; ++r) acc = fma(L[kSH + 16 * r + i], w[r], acc);
                    if (i % kFlight == kFlight - 1) asm volatile("" : "+v"(acc) : : "memory");
                    u[i] = acc;
                }
                wave_lds_sync();  // every lane has read Theta_k: Lambda_k may overwrite the image
                // Column j on and below the diagonal, not the whole column as a row: H' V^-1 H C is symmetric only up to the
                // rounding of H C, which 1 / V magnifies, and the entry (i, j), i >= j, of the stated expression is column j's
                if (own) {
#pragma unroll
                    for (int i = 0; i < 15; ++i)
                        if (i >= j) L[kSTh + kSStr * i + j] = u[i];
                }
            }
        }
        wave_lds_sync();  // r_k and Lambda_k are in place

        // ---- 4. q_{k-1} = A_{k-1}' r_k, Theta_{k-1} = A_{k-1}' Lambda_k A_{k-1} ----
        // apply_t(v, out): out = A' v on the knot's operator.  The body exists once per operator -- the step block's and the
        // touchdown knot's -- so that neither form's values stay live across the other's applications (as k_tracking_kalman).
        auto back = [&](auto apply_t) {
            double v[15], out[15];
            if (wantX) {
#pragma unroll
                for (int c = 0; c < 15; ++c) v[c] = L[kSR + c];
                apply_t(v, out);
                if (ln == 0) {
#pragma unroll
                    for (int c = 0; c < 15; ++c) L[kSQ + c] = out[c];
                }
            }
            if (wantP) {
                // only the lower triangle of Lambda_k is read: it is exactly symmetric
#pragma unroll
                for (int c = 0; c < 15; ++c) v[c] = L[kSTh + sym(c)];
                apply_t(v, out);  // column j of A' Lambda
                wave_lds_sync();  // the image has been read
                if (own) {
#pragma unroll
                    for (int i = 0; i < 15; ++i) L[kSTh + kSStr * j + i] = out[i];
                }
                wave_lds_sync();
#pragma unroll
                for (int c = 0; c < 15; ++c) v[c] = L[kSTh + kSStr * c + j];  // row j of A' Lambda = column j of Lambda A
                apply_t(v, out);
                wave_lds_sync();
                if (own) {
#pragma unroll
                    for (int i = 0; i < 15; ++i) L[kSTh + kSStr * j + i] = out[i];
                }
            }
        };
        KnotMode md;
        if constexpr (kGuard) md = guard_mode(k - 1, ks, im);
        else md = knot_mode(k, kt - 1, im);
        if (kGuard && k - 1 == ks) {  // the touchdown knot: the composite operator, transposed, in the block's place
            double xk[15];
#pragma unroll
            for (int i = 0; i < 14; ++i) xk[i] = L[kSZ + i];
            xk[14] = 0.0;  // the clock feeds nothing
            const double u5[5] = {L[kSZ + 15], L[kSZ + 16], L[kSZ + 17], L[kSZ + 18], L[kSZ + 19]};
            const TouchdownBlock tb = touchdown_block(M, md, tau, xk, u5);
            back([&](const double (&v)[15], double (&out)[15]) {
                double bf[4];
                touchdown_apply_t(tb, M, v, out, bf);
            });
        } else {
            const StepBlock blk = step_block(L + kSZ, md, M);
            back([&](const double (&v)[15], double (&out)[15]) { block_apply_t(blk, v, out); });
        }
        wave_lds_sync();  // q_{k-1} and Theta_{k-1} are in place; the tiles and the knot may be rewritten
    }
}


// ---- k_tracking_kalman_vjp ----
// per-row LDS image (doubles): the Lambda image [15][17] | the knot's 20 entries of Zout | the H tile [8][16], 1/V in its column 15 |
// the L tile [15][8] | the Lgain_bar tile [15][8], which becomes the Tb tile in place
constexpr int kVP = 0, kVZ = 256, kVH = kVZ + 20, kVL = kVH + QLN_TRACK_NY_MAX * 16, kVB = kVL + kJTile, kVRow = kVB + kJTile;
static_assert(kImgSize <= kVZ - kVP && kVZ % 2 == 0 && kVH % 2 == 0 && kVL % 2 == 0 && kVB % 2 == 0 && kVRow % 2 == 0 &&
                  kVRow <= kKRow,
              "the image fits; 16-byte aligned sections; within the Kalman kernel's budget");

// The reverse sweep through k_tracking_kalman's design (include/qln_evaluator.h): the transpose of
// k_tracking_kalman_jvp's linear map between the arrays as stored, cotangents (Lgain_bar, Pest_bar, logdet_bar) in, (Sigma0_bar,
// Wdiag_bar, Vdiag_bar) per problem out.  That kernel's mapping, one problem per row of sixteen lanes, lane j owns column j, and
// one padded image holds Lambda, the full symmetric cotangent of Pd^-_{k+1} (zero behind the last knot); its backbone is the
// smoother's: A' Lambda A by two transposed applications (block_apply_t, touchdown_apply_t) and C' . C with C = I - L H.  Per
// knot k = N-1 .. 0, with Sinv = diag(1/V) (I - H L):
//   1. (k < N-1) Wbar_j += Lambda(j, j);  Pi = A_k' Lambda A_k: the congruence step, transposed;
//   2. Pi += sym(Pest_bar_k): a packed off-diagonal entry stands for two, so half of it goes to the image's lower triangle, which
//      is the one that is read;
//   3. row j of Tb = Lgain_bar_k Sinv': (lb - (lb L') H') ./ V, two dense chains on broadcast reads of the two tiles, no entry of
//      H L formed; it replaces row j of the Lgain_bar tile;
//   4. sym(Sb), Sb = -L' Tb + logdet_bar_k Sinv: 36 row sums, the same bits in every lane, each consumed where it is formed --
//      its share of y = sym(Sb) H[:, j] and, on the diagonal, of Vbar -- so that Sb is never held;
//   5. C' Pi C by two applications of v - H' (L' v) with a transpose through the image between them; the first one's L' Pi[:, j]
//      is row j of Pi L, whose row sums against row j of L are diag(L' Pi L), the rest of Vbar;
//   6. column j of H' sym(Sb) H + sym(Tb H) = H' (y + Tb(j, :)' / 2) + Tb H[:, j] / 2 is added before the column is stored as
//      row j: Lambda_k.
// Sigma0_bar leaves from Lambda_0's lower triangle, the off-diagonal entries doubled.  Wbar (lane j's entry) and Vbar stay in
// registers across the knots.  L_k, Lgain_bar_k, Pest_bar_k and logdet_bar_k are requested one knot ahead, behind the knot's step
// block, and Zout's knot at the top of the knot before.  A NULL cotangent is a zero that is not read and takes the path of a
// given one, so its bits are those of explicit zeros.  Compiled for eight measurement rows as k_tracking_kalman: zero rows of H,
// zero columns of L and Lgain_bar and 1/V = 1 behind ny change no value.  Nothing here divides or factors.
template <bool kModel, bool kGuard>
__global__ __launch_bounds__(kWave) void k_tracking_kalman_vjp(BatchParams P, SmootherNoise Nz, const double* __restrict__ Zout,
                                                               const double* __restrict__ Lg, const double* __restrict__ Hg, int ny,
                                                               const double* __restrict__ Lbg, const double* __restrict__ Pbg,
                                                               const double* __restrict__ ldbg, double* __restrict__ S0b,
                                                               double* __restrict__ Wbg, double* __restrict__ Vbg,
                                                               const double* __restrict__ model, const double* __restrict__ event) {
    static_assert(kModel || !kGuard, "the guarded sweep runs on the kModel path");
    constexpr int NY = QLN_TRACK_NY_MAX;
    __shared__ double lds[kRows * kVRow];
    const Row16 r16 = row16_of(P);  // lane 15 shadows column 14 and writes nothing to the image
    const int ln = r16.ln, j = r16.j, bc = r16.bc, kt = r16.kt, im = r16.im, N = P.N;
    const bool own = r16.own, valid = r16.valid;
    const Model Mp = plant_model<kModel>(P, model, bc);
    const Model& M = kGuard ? Mp : r16.M;
    const GuardEvent ev = guard_event<kGuard>(event, bc, N);
    double* L = lds + r16.row * kVRow;
    const Image15 Lm{L + kVP, j, own};
    const int gn = QLN_NX * ny;  // a knot's gain entries
    const double* __restrict__ Zb = Zout + (int64_t)bc * P.z_stride;
    const double* __restrict__ Lb = Lg + (int64_t)bc * N * gn;
    const double* __restrict__ Bb = Lbg ? Lbg + (int64_t)bc * N * gn : nullptr;
    const double* __restrict__ Pb = Pbg ? Pbg + (int64_t)bc * N * QLN_TRACK_P_NNZ : nullptr;
    const double* __restrict__ lb = ldbg ? ldbg + (int64_t)bc * N : nullptr;

    int po[8], lo[8];
    packed_offsets(ln, po);
    gain_offsets(ln, ny, kVL, lo);
    const auto Hrow = [&](int r, int c) { return L[kVH + 16 * r + c]; };  // H(r, c); 1 / V_r in column 15
    const auto Lrow = [&](int i, int r) { return L[kVL + NY * i + r]; };  // the gain's L(i, r)
    const auto Brow = [&](int i, int r) { return L[kVB + NY * i + r]; };  // Lgain_bar(i, r), then Tb(i, r)

    // Lambda = 0 behind the last knot; the two gain tiles zero, so the columns behind ny stay zero; the H tile, zero rows behind ny
    {
#pragma unroll
        for (int t = 0; t < 16; ++t) L[kVP + ln + 16 * t] = 0.0;
#pragma unroll
        for (int t = 0; t < (2 * kJTile + 15) / 16; ++t)
            if (ln + 16 * t < 2 * kJTile) L[kVL + ln + 16 * t] = 0.0;
#pragma unroll
        for (int r = 0; r < NY; ++r) L[kVH + 16 * r + ln] = own ? ((r < ny) ? Hg[15 * r + ln] : 0.0) : Nz.iv[r];
    }

    // a knot's entries ln + 16 t of L, Lgain_bar and Pest_bar and its logdet_bar, requested one knot ahead
    double zn[2] = {0.0, 0.0}, lq[8], bq[8], pq[8], ldn;
    auto request = [&](int k) {
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int g = min(ln + 16 * t, gn - 1);
            lq[t] = Lb[(int64_t)k * gn + g];
            bq[t] = Bb ? Bb[(int64_t)k * gn + g] : 0.0;
            pq[t] = Pb ? Pb[(int64_t)k * QLN_TRACK_P_NNZ + min(ln + 16 * t, QLN_TRACK_P_NNZ - 1)] : 0.0;
        }
        ldn = lb ? lb[k] : 0.0;
    };
    request(N - 1);
    wave_lds_sync();

    double wbar = 0.0, vbar[NY];
#pragma unroll
    for (int r = 0; r < NY; ++r) vbar[r] = 0.0;

    for (int k = N - 1; k >= 0; --k) {
        const bool last = k == N - 1;  // the last knot has an update and no step
        tile_fill(L, lo, gn, tile_lane(ln), [&](int t) { return lq[t]; });
        tile_fill(L + (kVB - kVL), lo, gn, tile_lane(ln), [&](int t) { return bq[t]; });
        if (!last) {
            L[kVZ + ln] = zn[0];
            if (ln < 4) L[kVZ + 16 + ln] = zn[1];
        }
        if (k > 0) knot_load(Zb + 20 * (k - 1), ln, zn[0], zn[1]);
        wave_lds_sync();  // the knot and the two tiles are in place

        // ---- 1. Wbar and Pi = A_k' Lambda A_k ----
        if (!last) {
            wbar += Lm.a[(kImgStr + 1) * j];
            KnotMode md;
            if constexpr (kGuard) md = guard_mode(k, ev.ks, im);
            else md = knot_mode(k + 1, kt - 1, im);
            if (kGuard && k == ev.ks) {  // the touchdown knot: the composite operator, transposed, in the block's place
                const TouchdownBlock tb = touchdown_block_at(L + kVZ, M, md, ev.tau);
                congruence(
                    Lm,
                    [&](const double (&v)[15], double (&out)[15]) {
                        double bf[4];
                        touchdown_apply_t(tb, M, v, out, bf);
                    },
                    [] {});
            } else {
                const StepBlock blk = step_block(L + kVZ, md, M);
                congruence(Lm, [&](const double (&v)[15], double (&out)[15]) { block_apply_t(blk, v, out); }, [] {});
            }
            wave_lds_sync();
        }
        // ---- 2. Pi += sym(Pest_bar_k), into the lower triangle; a diagonal entry lies at a multiple of kImgStr + 1 ----
        {
            const TileLane tl = tile_lane(ln);
#pragma unroll
            for (int t = 0; t < 8; ++t)
                if (tl.le + 16 * t < QLN_TRACK_P_NNZ) {
                    const double half = (po[t] % (kImgStr + 1) == 0) ? 1.0 : 0.5;
                    Lm.a[po[t]] = fma(half, pq[t], Lm.a[po[t]]);
                }
        }
        const double ldb = ldn;
        if (k > 0) request(k - 1);
        wave_lds_sync();

        // ---- 3. and 4. Tb's row j, sym(Sb) and what hangs on it ----
        double hj[NY], lj[NY], tb[NY], y[NY];
#pragma unroll
        for (int r = 0; r < NY; ++r) {
            hj[r] = Hrow(r, j);
            lj[r] = Lrow(j, r);  // row j of L
            y[r] = 0.0;
        }
        {
            double lbj[NY], w[15];
#pragma unroll
            for (int r = 0; r < NY; ++r) lbj[r] = Brow(j, r);
            chain_rows(Lrow, lbj, w);                                             // lb L'
            chain_rows_sub([&](int a, int i) { return Hrow(a, i); }, w, lbj, tb);  // lb - (lb L') H'
            double q[NY];  // Tb(j, :) + logdet_bar H(:, j)' ./ V: the row sums of L(j, a) q[b] are (L' Tb + logdet_bar (H L)' / V)(a, b)
#pragma unroll
            for (int r = 0; r < NY; ++r) {
                tb[r] *= Hrow(r, 15);
                q[r] = fma(ldb * Hrow(r, 15), hj[r], tb[r]);
            }
            if (own) {
#pragma unroll
                for (int r = 0; r < NY; ++r) L[kVB + NY * j + r] = tb[r];
            }
#pragma unroll
            for (int a = 0; a < NY; ++a) {
#pragma unroll
                for (int b = 0; b < a; ++b) {
                    const double s = row_sum16(own ? -0.5 * fma(lj[a], q[b], lj[b] * q[a]) : 0.0);
                    y[a] = fma(s, hj[b], y[a]);
                    y[b] = fma(s, hj[a], y[b]);
                }
                const double s = fma(ldb, Hrow(a, 15), row_sum16(own ? -(lj[a] * q[a]) : 0.0));
                vbar[a] += s;
                y[a] = fma(s, hj[a], y[a]);
            }
        }
        // ---- 5. C' Pi C, and 6. the sources ----
        const auto Lt = [&](int a, int c) { return Lrow(c, a); };  // L'
        const auto Ht = [&](int i, int a) { return Hrow(a, i); };  // H'
        {
            double p[15], u[15], t[NY];
            Lm.column(p);
            chain_rows(Lt, p, t);  // row j of Pi L
#pragma unroll
            for (int a = 0; a < NY; ++a) vbar[a] += row_sum16(own ? lj[a] * t[a] : 0.0);
            chain_rows_sub(Ht, t, p, u);  // column j of C' Pi -> row j of the image
            wave_lds_sync();              // every lane holds its column of Pi; the Tb tile is in place
            Lm.store_row(u);
        }
        wave_lds_sync();
        {
            double vt[15], t[NY], out[15], z[NY], s1[15], s2[15];
            Lm.transposed(vt);
            chain_rows(Lt, vt, t);
            chain_rows_sub(Ht, t, vt, out);  // column j of C' Pi C
#pragma unroll
            for (int a = 0; a < NY; ++a) z[a] = fma(0.5, tb[a], y[a]);
            chain_rows(Ht, z, s1);    // H' (y + Tb(j, :)' / 2)
            chain_rows(Brow, hj, s2);  // Tb H[:, j]
#pragma unroll
            for (int i = 0; i < 15; ++i) out[i] += fma(0.5, s2[i], s1[i]);
            wave_lds_sync();  // every lane holds its row: Lambda_k may overwrite the image
            Lm.store_row(out);
        }
        wave_lds_sync();  // only the lower triangle of Lambda_k is read from here on; the tiles and the knot may be rewritten
    }

    if (S0b && valid)
        tile_store(S0b + (int64_t)bc * QLN_TRACK_P_NNZ, po, QLN_TRACK_P_NNZ, tile_lane(ln),
                   [&](int o) { return (o % (kImgStr + 1) == 0) ? Lm.a[o] : 2.0 * Lm.a[o]; });
    if (Wbg && valid && own) Wbg[(int64_t)bc * QLN_NX + j] = wbar;
    if (Vbg && valid) {
        double v = vbar[0];
#pragma unroll
        for (int q = 1; q < NY; ++q) v = (ln == q) ? vbar[q] : v;
        if (ln < ny) Vbg[(int64_t)bc * ny + ln] = v;
    }
}


// ---- k_tracking_rollout_jvp ----
// One knot's inputs, as lane ln of a row loads them.  z0 / zd0: entry ln of the knot's twenty in Zout / Zref_dot (lane
// j < 15: x_j, lane 15: F1x); z1 / zd1: entry 16 + (ln & 3) (F1y, F2x, F2y, h in lanes 0-3).  xr: x_ref,j; kc, kd: column j
// of K_k and of Kdot_k.
struct JvpKnot {
    double z0, z1, zd0, zd1, xr, kc[4], kd[4];
};

template <bool kHasK, bool kHasKd, bool kHasZd>
__device__ __forceinline__ void jvp_load(JvpKnot& s, const double* __restrict__ Zo, const double* __restrict__ Zd,
                                         const double* __restrict__ Zr, const double* __restrict__ Kk,
                                         const double* __restrict__ Kdk, int k, int ln, int j) {
    knot_load(Zo + 20 * k, ln, s.z0, s.z1);
    if constexpr (kHasZd) knot_load(Zd + 20 * k, ln, s.zd0, s.zd1);
    if constexpr (kHasK) {
#pragma unroll
        for (int m = 0; m < 4; ++m) s.kc[m] = Kk[60 * (int64_t)k + 15 * m + j];
    }
    if constexpr (kHasKd) {
        s.xr = Zr[20 * k + j];
#pragma unroll
        for (int m = 0; m < 4; ++m) s.kd[m] = Kdk[60 * (int64_t)k + 15 * m + j];
    }
}

// Row j of [A B G] applied to the knot's tangents, for one step of length h in mode md at the state x: returns
// (A dx + B (dF, dh) + G md4)[j].  blk is step_block() of the same arguments, formed by every lane of the row alike; the lane
// picks its row's entries from the visitor (rows 2 and 9 of A: at the lane's column, summed over the row).  kWantB: the force columns exist (some dF can be non-zero);
// kWantH: the h column is formed, and applied where use_h says.  The tangent sweep's knot; the touchdown knot of the guarded
// sweep calls it twice, once per leg.
template <bool kWantB, bool kWantH, bool kModel>
__device__ __forceinline__ double jvp_apply_row(int j, bool own, const StepBlock& blk, const double (&x)[14], double F1x,
                                                double F1y, double F2x, double F2y, double h, const KnotMode md, const Model& M,
                                                double dx, const double (&dF)[4], double dh, bool use_h, bool want_model,
                                                const double (&md4)[QLN_MODEL_NP]) {
    // ---- row j of [A B]: the visitor's entries at the lane's row (rows 2 and 9 of A: at the lane's column) ----
    double a2 = 0.0, a9 = 0.0, dg = 0.0, cp = 0.0, bj[4] = {0.0, 0.0, 0.0, 0.0}, hj = 0.0;
    for_each_rollout_entry(blk, [&](auto r, auto c, double val) {
        if constexpr (c < 15) {
            if constexpr (r == 2) a2 = (j == c) ? val : a2;
            else if constexpr (r == 9) a9 = (j == c) ? val : a9;
            else if constexpr (r == c) dg = (j == r) ? val : dg;
            else cp = (j == r) ? val : cp;  // r == c - 7 (a_structure_ok)
        } else if constexpr (c < 19) {
            if constexpr (kWantB) bj[c - 15] = (j == r) ? val : bj[c - 15];
        } else if constexpr (kWantH) {
            hj = (j == r) ? val : hj;
        }
    });
    const double dxc = row_shl7(dx);  // dx[j+7], 0 past the row's end
    const double s2 = row_sum16(own ? a2 * dx : 0.0), s9 = row_sum16(own ? a9 * dx : 0.0);
    double acc = (j == 2) ? s2 : (j == 9) ? s9 : fma(cp, dxc, dg * dx);
    if constexpr (kWantB) {
#pragma unroll
        for (int m = 0; m < 4; ++m) acc = fma(bj[m], dF[m], acc);
    }
    if constexpr (kWantH) {
        if (use_h) acc = fma(hj, dh, acc);
    }
    if constexpr (kModel) {
        if (want_model) {
            const ModelBlock mblk = model_block(x, F1x, F1y, F2x, F2y, h, md, M);
            double gj[QLN_MODEL_NP] = {0.0, 0.0, 0.0, 0.0};
            for_each_model_entry(mblk, [&](auto r, auto q, double val) { gj[q] = (j == r) ? val : gj[q]; });
#pragma unroll
            for (int q = 0; q < QLN_MODEL_NP; ++q) acc = fma(gj[q], md4[q], acc);
        }
    }
    return acc;
}

// The forward (tangent) sweep of k_tracking_rollout (include/qln_evaluator.h): dx_0 = x0_dot, then per knot k = 0..N-2
//   dF_k = Fref_dot_k - K_k (dx_k - xref_dot_k) - Kdot_k (x_k - x_ref,k),  dh_k = href_dot_k,
//   dx_{k+1} = A_k dx_k + B_k (dF_k, dh_k),
// with the blocks of the reverse sweep: the evaluator's closed form at Zout's (x_k, u_k), the jump knot's clock row kept.
// One problem per row of sixteen lanes; lane j < 15 owns dx[j], row j of [A_k B_k] and column j of K_k and Kdot_k, lane 15
// holds dx = 0 and only stores a u slot.  Every lane of the row forms the knot's StepBlock alike -- Zout's knot arrives as two
// coalesced loads and is handed round by DPP row broadcasts -- and picks its row's entries from the visitor: the diagonal
// and the velocity coupling A(j, j+7) (dx[j+7] by a row shift), B row j, and the h column's entry.  Rows 2 and 9 of A are
// dense: lane c contributes A(2, c) dx_c and A(9, c) dx_c to two row sums; K (dx - xref_dot) + Kdot e is four more.
// Template flags say which inputs exist: nothing that is absent is read (Zref only with Kdot).
// kModel (qln_tracking_rollout_model_jvp): [A_k B_k] at problem b's own model (model, null: the handle's), and the model's
// tangent enters as + G_k model_dot[b], lane j picking row j of G_k from for_each_model_entry (model_dot null: no term).
// kGuard (qln_tracking_rollout_guarded_jvp, with kModel): the modes are guard_mode's of the problem's touchdown knot ks, read
// with tau from event.  At ks the composite step: d tau from dy, dv, dF_y (row broadcasts of dx; dF is in every lane) and the
// model's tangent over w, the foot's vertical velocity in x- = step_mode(x_k; tau), which every lane of the row recomputes;
// jvp_apply_row through the flight leg at (x_k, tau) with d tau in the place of dh, the jump map's zeros, jvp_apply_row
// through the mode-3 leg at (x+, h - tau) with dh - d tau.  event_dot (null: not written) gets d tau and the clock's tangent.
// kLimit (qln_tracking_rollout_limited_jvp, DESIGN.md 4.20, with kModel): a channel that rode a limit at knot k (sat, the limited
// roll-out's record) was a constant: its dF is zero, for everything downstream, the touchdown knot's d tau included.
template <bool kHasK, bool kHasKd, bool kHasZd, bool kModel, bool kGuard, bool kLimit = false>
__global__ __launch_bounds__(kWave) void k_tracking_rollout_jvp(BatchParams P, const double* __restrict__ Zref,
                                                                const double* __restrict__ Kg, const double* __restrict__ Zout,
                                                                const double* __restrict__ Zref_dot,
                                                                const double* __restrict__ Kdot,
                                                                const double* __restrict__ x0_dot,
                                                                double* __restrict__ Zout_dot,
                                                                const double* __restrict__ model,
                                                                const double* __restrict__ model_dot,
                                                                const double* __restrict__ event,
                                                                double* __restrict__ event_dot,
                                                                const double* __restrict__ sat) {
    static_assert(kHasK || !kHasKd, "Kdot needs K");
    static_assert(kModel || !kLimit, "the limited sweep runs on the kModel path");
    static_assert(kModel || !kGuard, "the guarded sweep runs on the kModel path");
    const Row16 r16 = row16_of(P);  // lane 15 reads lane 14's slots and contributes nothing
    const int ln = r16.ln, j = r16.j, bc = r16.bc, kt = r16.kt, im = r16.im, N = P.N;
    const bool own = r16.own, valid = r16.valid;
    const Model M = plant_model<kModel>(P, model, bc);
    const int64_t zo = (int64_t)bc * P.z_stride, ko = (int64_t)bc * (N - 1) * (QLN_TRACK_NU * QLN_NX);
    const double* __restrict__ Zo = Zout + zo;
    const double* __restrict__ Zd = kHasZd ? Zref_dot + zo : nullptr;
    const double* __restrict__ Zr = kHasKd ? Zref + zo : nullptr;
    const double* __restrict__ Kb = kHasK ? Kg + ko : nullptr;
    const double* __restrict__ Kdb = kHasKd ? Kdot + ko : nullptr;
    double* __restrict__ Od = Zout_dot + zo;
    [[maybe_unused]] int ks = -1;
    [[maybe_unused]] double tau = 0.0, e_tau = 0.0, e_clock = 0.0;
    if constexpr (kGuard) {
        ks = guard_knot(event[(int64_t)QLN_TOUCHDOWN_INFO_STRIDE * bc], N);
        tau = event[(int64_t)QLN_TOUCHDOWN_INFO_STRIDE * bc + 1];
    }

    double md4[QLN_MODEL_NP] = {0.0, 0.0, 0.0, 0.0};
    if constexpr (kModel) {
        if (model_dot) {
#pragma unroll
            for (int q = 0; q < QLN_MODEL_NP; ++q) md4[q] = model_dot[(int64_t)bc * QLN_MODEL_NP + q];
        }
    }
    double dx = (own && x0_dot) ? x0_dot[(int64_t)bc * QLN_NX + j] : 0.0;
    JvpKnot cur, nxt;
    jvp_load<kHasK, kHasKd, kHasZd>(nxt, Zo, Zd, Zr, Kb, Kdb, 0, ln, j);
    // the knot's saturation code, loaded with the knot's slices (the same value in every lane of the row)
    [[maybe_unused]] const double* __restrict__ Sb = kLimit ? sat + (int64_t)bc * (N - 1) : nullptr;
    [[maybe_unused]] double satc = 0.0, satn = 0.0;
    if constexpr (kLimit) satn = Sb[0];
    for (int k = 0; k < N - 1; ++k) {
        cur = nxt;
        if (k + 1 < N - 1) jvp_load<kHasK, kHasKd, kHasZd>(nxt, Zo, Zd, Zr, Kb, Kdb, k + 1, ln, j);
        if constexpr (kLimit) {
            satc = satn;
            if (k + 1 < N - 1) satn = Sb[k + 1];
        }
        // ---- the knot's state and controls, in every lane ----
        double x[14];
        row_bcast_first(cur.z0, x, std::make_integer_sequence<int, 14>{});
        const double F1x = row_bcast<15>(cur.z0), F1y = row_bcast<0>(cur.z1), F2x = row_bcast<1>(cur.z1),
                     F2y = row_bcast<2>(cur.z1), h = row_bcast<3>(cur.z1);
        KnotMode md;
        if constexpr (kGuard) md = guard_mode(k, ks, im);
        else md = knot_mode(k + 1, kt - 1, im);
        // the knot's block, in every lane; the guarded sweep forms its blocks where it applies them, at each leg's step length
        StepBlock blk;
        if constexpr (!kGuard) blk = step_block(x, F1x, F1y, F2x, F2y, h, md, M);
        // ---- the applied controls' tangent: dF = Fref_dot - K (dx - xref_dot) - Kdot e, dh = href_dot ----
        double dF[4], dh = 0.0, xrd = 0.0;
#pragma unroll
        for (int m = 0; m < 4; ++m) dF[m] = 0.0;
        if constexpr (kHasZd) {
            xrd = cur.zd0;
            dF[0] = row_bcast<15>(cur.zd0);
            dF[1] = row_bcast<0>(cur.zd1);
            dF[2] = row_bcast<1>(cur.zd1);
            dF[3] = row_bcast<2>(cur.zd1);
            dh = row_bcast<3>(cur.zd1);
        }
        if constexpr (kHasK) {
            const double d = dx - xrd;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                double t = cur.kc[m] * d;
                if constexpr (kHasKd) t = fma(cur.kd[m], cur.z0 - cur.xr, t);
                dF[m] = dF[m] - row_sum16(own ? t : 0.0);
            }
        }
        if constexpr (kLimit) limit_zero4(limit_mask(satc), dF);
        // ---- row j of [A B G] on the knot's tangents ----
        double acc;
        if constexpr (kGuard) {
            const bool td = k == ks;
            double hA = h, dhA = dh, dtau = 0.0;
            double xm[15];
            if (td) {
                const bool f2 = md.f2free;  // mode 1: foot 2 is the free one
                double xk[15];
#pragma unroll
                for (int i = 0; i < 14; ++i) xk[i] = x[i];
                xk[14] = 0.0;  // the clock feeds nothing
                const double u5[5] = {F1x, F1y, F2x, F2y, h};
                step_mode(M, md, tau, xk, u5, xm);
                const double y = f2 ? x[6] : x[4], Fy = f2 ? F2y : F1y, w = f2 ? xm[13] : xm[11];
                const double dy4 = row_bcast<4>(dx), dy6 = row_bcast<6>(dx), dv11 = row_bcast<11>(dx), dv13 = row_bcast<13>(dx);
                const double dy = f2 ? dy6 : dy4, dv = f2 ? dv13 : dv11, dFy = f2 ? dF[3] : dF[1];
                const double da = (-dFy / M.mf + (Fy / (M.mf * M.mf)) * md4[2]) + md4[0];
                dtau = (y <= 0.0) ? 0.0 : -((dy + tau * dv) + (0.5 * tau * tau) * da) / w;
                e_tau = dtau;
                e_clock = row_bcast<14>(dx) + dtau;
                hA = tau;
                dhA = dtau;
            }
            blk = step_block(x, F1x, F1y, F2x, F2y, hA, md, M);
            acc = jvp_apply_row<kHasK || kHasZd, true, kModel>(j, own, blk, x, F1x, F1y, F2x, F2y, hA, md, M, dx, dF, dhA,
                                                               kHasZd || td, model_dot != nullptr, md4);
            if (td) {
                const bool jrow = j == 4 || j == 6 || (j >= 10 && j <= 13);
                const double dxm = (own && !jrow) ? acc : 0.0;  // the jump map
                jump_map(xm);
                double xp[14];
#pragma unroll
                for (int i = 0; i < 14; ++i) xp[i] = xm[i];
                const KnotMode m3 = {false, false, false, true};
                blk = step_block(xp, F1x, F1y, F2x, F2y, h - tau, m3, M);
                acc = jvp_apply_row<kHasK || kHasZd, true, kModel>(j, own, blk, xp, F1x, F1y, F2x, F2y, h - tau, m3, M, dxm, dF,
                                                                   dh - dtau, true, model_dot != nullptr, md4);
            }
        } else {
            acc = jvp_apply_row<kHasK || kHasZd, kHasZd, kModel>(j, own, blk, x, F1x, F1y, F2x, F2y, h, md, M, dx, dF, dh, true,
                                                                 model_dot != nullptr, md4);
        }
        // ---- the knot's twenty entries of Zout_dot: dx_k and (dF_k, dh_k) ----
        // (dF, dh) become one array only here: held as one through the knot it costs up to 8 VGPRs
        // (profiles/row16_refactor_resource_usage.txt)
        if (valid) knot_store(Od + 20 * k, r16, dx, {dF[0], dF[1], dF[2], dF[3], dh});
        dx = own ? acc : 0.0;
    }
    if (valid && own) Od[20 * (N - 1) + j] = dx;
    if constexpr (kGuard) {
        // the record's tangent: d tau and the touchdown clock's, zeros elsewhere and without a touchdown
        if (event_dot && valid && ln < QLN_TOUCHDOWN_INFO_STRIDE)
            event_dot[(int64_t)QLN_TOUCHDOWN_INFO_STRIDE * bc + ln] = (ln == 1) ? e_tau : (ln == 2) ? e_clock : 0.0;
    }
}

// ---- k_tracking_rollout_estimated_jvp / _vjp ----
// The sweeps through the estimate-feedback roll-out (qln_tracking_rollout_estimated_jvp / _vjp and their _guarded forms,
// include/qln_evaluator.h), in the mapping of k_tracking_rollout_jvp / _vjp: one problem per row of sixteen
// lanes.  A problem carries two chains, the plant's along Zout and the estimator's along Xhat, so lane j < 15 owns two
// entries -- dx[j] and dxm[j] forward, lam[j] and lamm[j] in reverse -- and each knot applies two blocks: the plant's at
// (x_k, u_k, model[b]) and the estimator's at (xhat_k, u_k, the handle's model), both through the siblings' jvp_apply_row /
// vjp_apply_column, so that a chain of this sweep and the sibling sweep on the same trajectory give the same bits.
// The measurement update couples the chains.  H is uniform over the batch and staged once per block in LDS; lane j reads
// column j of it (conflict-free: consecutive lanes, consecutive words) and H (dx - dxm) is ny row sums.  Lane j reads row j
// of L_k (ny consecutive doubles: the row's fifteen lanes cover the tile's 15 ny doubles as whole lines) and column j of K_k;
// the sweeps take no RK4 step outside a touchdown knot, so nothing here is duplicated across the row's lanes but the blocks,
// as in the siblings.  Loops over the sensor rows run to QLN_TRACK_NY_MAX under a uniform r < ny, so every value sits at a
// compile-time position and a call with ny rows gives the bits of one with zero rows and columns behind them.
// Every slice of a knot is loaded one knot ahead (EstimatedJvpKnot / EstimatedVjpKnot), what is uniform over the row -- the
// controls, the innovations and their cotangents -- as one entry per lane, handed round by DPP row broadcasts when it is used;
// loaded where they are used the kernels took 1.9 (forward; 2.9 guarded) and 1.7 to 1.8 times as long.  The two
// chains' steps are kept apart by scheduling barriers: interleaved, two blocks' temporaries are live at once.

// knot_load of Zout's knot for the two sweeps.  kLimit: lane 4's second entry, which repeats u_1 and which nobody reads, is
// the knot's saturation code instead (code: its address), read back by row_bcast<4>: the same number of loads and of
// registers as without the flag.  Carried as a value of its own, loaded beside the slices, the forward sweep took 15 to 20 %
// longer than its sibling.
template <bool kLimit>
__device__ __forceinline__ void estimated_knot_load(const double* __restrict__ zk, const double* __restrict__ code, int ln, double& e0,
                                                    double& e1) {
    if constexpr (kLimit) {
        e0 = zk[ln];
        const double* q = (ln == 4) ? code : zk + 16 + (ln & 3);
        e1 = *q;
    } else {
        knot_load(zk, ln, e0, e1);
    }
}

// One chain's knot of the forward sweep: row j of [A B G] on (dx, dF, dh, md4).  kGuard: the guarded sweep's statement of the
// knot (k_tracking_rollout_jvp), td saying that this is the chain's touchdown knot, with d tau and the clock's tangent left
// in e_tau / e_clock there.
template <bool kGuard, bool kModel>
__device__ __forceinline__ double estimated_jvp_step(int j, bool own, const double (&x)[14], double F1x, double F1y, double F2x,
                                                     double F2y, double h, const KnotMode md, bool td, double tau, const Model& M,
                                                     double dx, const double (&dF)[4], double dh, bool want_model,
                                                     const double (&md4)[QLN_MODEL_NP], double& e_tau, double& e_clock) {
    if constexpr (!kGuard) {
        const StepBlock blk = step_block(x, F1x, F1y, F2x, F2y, h, md, M);
        return jvp_apply_row<true, true, kModel>(j, own, blk, x, F1x, F1y, F2x, F2y, h, md, M, dx, dF, dh, true, want_model, md4);
    } else {
        double hA = h, dhA = dh, dtau = 0.0;
        double xm[15];
        if (td) {
            const bool f2 = md.f2free;  // mode 1: foot 2 is the free one
            double xk[15];
#pragma unroll
            for (int i = 0; i < 14; ++i) xk[i] = x[i];
            xk[14] = 0.0;  // the clock feeds nothing
            const double u5[5] = {F1x, F1y, F2x, F2y, h};
            step_mode(M, md, tau, xk, u5, xm);
            const double y = f2 ? x[6] : x[4], Fy = f2 ? F2y : F1y, w = f2 ? xm[13] : xm[11];
            const double dy4 = row_bcast<4>(dx), dy6 = row_bcast<6>(dx), dv11 = row_bcast<11>(dx), dv13 = row_bcast<13>(dx);
            const double dy = f2 ? dy6 : dy4, dv = f2 ? dv13 : dv11, dFy = f2 ? dF[3] : dF[1];
            const double da = (-dFy / M.mf + (Fy / (M.mf * M.mf)) * md4[2]) + md4[0];
            dtau = (y <= 0.0) ? 0.0 : -((dy + tau * dv) + (0.5 * tau * tau) * da) / w;
            e_tau = dtau;
            e_clock = row_bcast<14>(dx) + dtau;
            hA = tau;
            dhA = dtau;
        }
        StepBlock blk = step_block(x, F1x, F1y, F2x, F2y, hA, md, M);
        double acc = jvp_apply_row<true, true, kModel>(j, own, blk, x, F1x, F1y, F2x, F2y, hA, md, M, dx, dF, dhA, true, want_model,
                                                       md4);
        if (td) {
            const bool jrow = j == 4 || j == 6 || (j >= 10 && j <= 13);
            const double dxj = (own && !jrow) ? acc : 0.0;  // the jump map
            jump_map(xm);
            double xp[14];
#pragma unroll
            for (int i = 0; i < 14; ++i) xp[i] = xm[i];
            const KnotMode m3 = {false, false, false, true};
            blk = step_block(xp, F1x, F1y, F2x, F2y, h - tau, m3, M);
            acc = jvp_apply_row<true, true, kModel>(j, own, blk, xp, F1x, F1y, F2x, F2y, h - tau, m3, M, dxj, dF, dh - dtau, true,
                                                    want_model, md4);
        }
        return acc;
    }
}

// One knot's inputs of the forward sweep, as lane ln of a row loads them: row j of L_k and of Ldot_k, and ivl: entry ln of innov_k
// (lanes behind ny repeat the last; handed round by DPP row broadcasts), for every knot;
// z0 / z1 / zd0 / zd1 as in JvpKnot, xh: xhat_k[j], xr: x_ref,j, kc, kd: column j of K_k and of Kdot_k (the knots with a step).
struct EstimatedJvpKnot {
    double l[QLN_TRACK_NY_MAX], ld[QLN_TRACK_NY_MAX], ivl;
    double z0, z1, xh, zd0, zd1, xr, kc[4], kd[4];
};

// The forward sweep (include/qln_evaluator.h): dx_0 = x0_dot, dxm_0 = xhat0_dot (null: x_ref_dot,0), then per knot
//   dinnov = H (dx - dxm),  dxh = dxm + L_k dinnov + Ldot_k innov_k                                  (k = 0 .. N-1)
//   dF = Fref_dot - K_k (dxh - xref_dot) - Kdot_k (xhat_k - x_ref,k),  dh = href_dot                 (k < N-1)
//   dx' = A^p dx + B^p (dF, dh) + G^p model_dot,   dxm' = A^e dxh + B^e (dF, dh)
// kHasK: K is given (K_dot is a run-time argument of that path); kHasLd: Lgain_dot is, and innov with it.
// kLimit (qln_tracking_rollout_estimated_limited_jvp): a channel that rode a limit at knot k (sat, the limited
// roll-out's record) was a constant: its dF is zero before anything reads it -- Zout_dot's u_k, both chains' B and both chains'
// d tau at their own touchdown knots.  The knot's code is loaded one knot ahead in a slot of the knot's slices
// (estimated_knot_load).
template <bool kGuard, bool kHasK, bool kHasLd, bool kLimit = false>
__global__ __launch_bounds__(kWave) void k_tracking_rollout_estimated_jvp(BatchParams P, EstimatedSweepIn in, EstimatedJvpArgs a,
                                                                          const double* __restrict__ sat) {
    constexpr int NY = QLN_TRACK_NY_MAX;
    __shared__ double Hs[NY * 15];
    const int ny = in.ny;
    for (int i = threadIdx.x; i < 15 * ny; i += kWave) Hs[i] = in.H[i];
    __syncthreads();
    const Row16 r16 = row16_of(P);  // lane 15 reads lane 14's slots and contributes nothing
    const int ln = r16.ln, j = r16.j, bc = r16.bc, kt = r16.kt, im = r16.im, N = P.N;
    const bool own = r16.own, valid = r16.valid;
    const Model M = plant_model<true>(P, in.model, bc);   // the plant's
    const Model Mh = plant_model<true>(P, nullptr, bc);   // the estimator's: always the handle's
    const int64_t zo = (int64_t)bc * P.z_stride, ko = (int64_t)bc * (N - 1) * (QLN_TRACK_NU * QLN_NX);
    const int64_t xo = (int64_t)bc * N * QLN_NX, go = xo * ny, io = (int64_t)bc * N * ny;
    const double* __restrict__ Zo = in.Zout + zo;
    const double* __restrict__ Xh = in.Xhat + xo;
    const double* __restrict__ Zd = a.Zref_dot ? a.Zref_dot + zo : nullptr;
    const double* __restrict__ Zr = a.K_dot ? in.Zref + zo : nullptr;
    const double* __restrict__ Kb = kHasK ? in.K + ko : nullptr;
    const double* __restrict__ Kdb = (kHasK && a.K_dot) ? a.K_dot + ko : nullptr;
    const double* __restrict__ Lb = in.Lgain + go + (int64_t)j * ny;
    const double* __restrict__ Ldb = kHasLd ? a.Lgain_dot + go + (int64_t)j * ny : nullptr;
    const double* __restrict__ Ib = kHasLd ? in.innov + io : nullptr;
    double* __restrict__ Od = a.Zout_dot + zo;
    [[maybe_unused]] int ks = -1, ksh = -1;
    [[maybe_unused]] double tau = 0.0, tauh = 0.0;
    double e_tau = 0.0, e_clock = 0.0, eh_tau = 0.0, eh_clock = 0.0;
    if constexpr (kGuard) {
        ks = guard_knot(in.event[(int64_t)QLN_TOUCHDOWN_INFO_STRIDE * bc], N);
        tau = in.event[(int64_t)QLN_TOUCHDOWN_INFO_STRIDE * bc + 1];
        ksh = guard_knot(in.event_hat[(int64_t)QLN_TOUCHDOWN_INFO_STRIDE * bc], N);
        tauh = in.event_hat[(int64_t)QLN_TOUCHDOWN_INFO_STRIDE * bc + 1];
    }
    double md4[QLN_MODEL_NP] = {0.0, 0.0, 0.0, 0.0};
    const double zero4[QLN_MODEL_NP] = {0.0, 0.0, 0.0, 0.0};  // the estimator's model has no tangent
    if (a.model_dot) {
#pragma unroll
        for (int q = 0; q < QLN_MODEL_NP; ++q) md4[q] = a.model_dot[(int64_t)bc * QLN_MODEL_NP + q];
    }
    double* __restrict__ Xd = a.Xhat_dot ? a.Xhat_dot + xo : nullptr;
    double* __restrict__ Ido = a.innov_dot ? a.innov_dot + io : nullptr;
    double dx = (own && a.x0_dot) ? a.x0_dot[(int64_t)bc * QLN_NX + j] : 0.0;
    double dxm = !own ? 0.0 : a.xhat0_dot ? a.xhat0_dot[(int64_t)bc * QLN_NX + j] : Zd ? Zd[j] : 0.0;
    [[maybe_unused]] const double* __restrict__ Sb = kLimit ? sat + (int64_t)bc * (N - 1) : nullptr;
    // the knot's slices are loaded one knot ahead: the gains' rows for every knot, the rest for the knots that take a step
    auto load = [&](EstimatedJvpKnot& s, int k) {
        const double* __restrict__ Lk = Lb + (int64_t)k * (15 * ny);
#pragma unroll
        for (int r = 0; r < NY; ++r) s.l[r] = r < ny ? Lk[r] : 0.0;
        if constexpr (kHasLd) {
            const double* __restrict__ Ldk = Ldb + (int64_t)k * (15 * ny);
            const double* __restrict__ ik = Ib + (int64_t)k * ny;
#pragma unroll
            for (int r = 0; r < NY; ++r) s.ld[r] = r < ny ? Ldk[r] : 0.0;
            s.ivl = ik[min(ln, ny - 1)];
        }
        if (k == N - 1) return;
        estimated_knot_load<kLimit>(Zo + 20 * k, kLimit ? Sb + k : nullptr, ln, s.z0, s.z1);
        s.xh = Xh[(int64_t)k * QLN_NX + j];
        if (Zd) knot_load(Zd + 20 * k, ln, s.zd0, s.zd1);
        if constexpr (kHasK) {
#pragma unroll
            for (int m = 0; m < 4; ++m) s.kc[m] = Kb[60 * (int64_t)k + 15 * m + j];
            if (Kdb) {
                s.xr = Zr[20 * k + j];
#pragma unroll
                for (int m = 0; m < 4; ++m) s.kd[m] = Kdb[60 * (int64_t)k + 15 * m + j];
            }
        }
    };
    EstimatedJvpKnot cur = {}, nxt = {};
    load(nxt, 0);
    for (int k = 0; k < N; ++k) {
        cur = nxt;
        if (k + 1 < N) load(nxt, k + 1);
        // ---- the measurement update's tangent ----
        const double dd = dx - dxm;
        double din[NY];
#pragma unroll
        for (int r = 0; r < NY; ++r) {
            din[r] = 0.0;
            if (r < ny) din[r] = row_sum16(own ? Hs[15 * r + j] * dd : 0.0);
        }
        double dxh = dxm;
#pragma unroll
        for (int r = 0; r < NY; ++r)
            if (r < ny) dxh = fma(cur.l[r], din[r], dxh);
        if constexpr (kHasLd) {
            double iv[NY];
            row_bcast_first(cur.ivl, iv, std::make_integer_sequence<int, NY>{});
#pragma unroll
            for (int r = 0; r < NY; ++r)
                if (r < ny) dxh = fma(cur.ld[r], iv[r], dxh);
        }
        dxh = own ? dxh : 0.0;
        if (valid) {
            if (Xd && own) Xd[(int64_t)k * QLN_NX + j] = dxh;
            if (Ido && ln < ny) {
                double o = din[0];
#pragma unroll
                for (int r = 1; r < NY; ++r) o = (ln == r) ? din[r] : o;
                Ido[(int64_t)k * ny + ln] = o;
            }
        }
        if (k == N - 1) break;
        // ---- the knot's states and controls, in every lane ----
        const double z0 = cur.z0, z1 = cur.z1, xhj = cur.xh;
        double x[14], xe[14];
        row_bcast_first(z0, x, std::make_integer_sequence<int, 14>{});
        const double F1x = row_bcast<15>(z0), F1y = row_bcast<0>(z1), F2x = row_bcast<1>(z1), F2y = row_bcast<2>(z1),
                     h = row_bcast<3>(z1);
        // ---- the applied controls' tangent ----
        double dF[4] = {0.0, 0.0, 0.0, 0.0}, dh = 0.0, xrd = 0.0;
        if (Zd) {
            xrd = cur.zd0;
            dF[0] = row_bcast<15>(cur.zd0);
            dF[1] = row_bcast<0>(cur.zd1);
            dF[2] = row_bcast<1>(cur.zd1);
            dF[3] = row_bcast<2>(cur.zd1);
            dh = row_bcast<3>(cur.zd1);
        }
        if constexpr (kHasK) {
            const double d = dxh - xrd;
            const double e = Kdb ? xhj - cur.xr : 0.0;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                double t = cur.kc[m] * d;
                if (Kdb) t = fma(cur.kd[m], e, t);
                dF[m] = dF[m] - row_sum16(own ? t : 0.0);
            }
        }
        if constexpr (kLimit) limit_zero4(limit_mask(row_bcast<4>(z1)), dF);
        // ---- the two chains' steps, one after the other: two blocks live at once do not fit the registers ----
        KnotMode md, mdh;
        if constexpr (kGuard) {
            md = guard_mode(k, ks, im);
            mdh = guard_mode(k, ksh, im);
        } else {
            md = mdh = knot_mode(k + 1, kt - 1, im);
        }
        const double accp = estimated_jvp_step<kGuard, true>(j, own, x, F1x, F1y, F2x, F2y, h, md, k == ks, tau, M, dx, dF, dh,
                                                             a.model_dot != nullptr, md4, e_tau, e_clock);
        __builtin_amdgcn_sched_barrier(0);
        row_bcast_first(xhj, xe, std::make_integer_sequence<int, 14>{});
        const double acce = estimated_jvp_step<kGuard, false>(j, own, xe, F1x, F1y, F2x, F2y, h, mdh, k == ksh, tauh, Mh, dxh, dF, dh,
                                                              false, zero4, eh_tau, eh_clock);
        __builtin_amdgcn_sched_barrier(0);
        if (valid) knot_store(Od + 20 * k, r16, dx, {dF[0], dF[1], dF[2], dF[3], dh});
        dx = own ? accp : 0.0;
        dxm = own ? acce : 0.0;
    }
    if (valid && own) Od[20 * (N - 1) + j] = dx;
    if constexpr (kGuard) {
        if (valid && ln < QLN_TOUCHDOWN_INFO_STRIDE) {
            if (a.event_dot) a.event_dot[(int64_t)QLN_TOUCHDOWN_INFO_STRIDE * bc + ln] = (ln == 1) ? e_tau : (ln == 2) ? e_clock : 0.0;
            if (a.event_hat_dot)
                a.event_hat_dot[(int64_t)QLN_TOUCHDOWN_INFO_STRIDE * bc + ln] = (ln == 1) ? eh_tau : (ln == 2) ? eh_clock : 0.0;
        }
    }
}

// One knot's inputs of the reverse sweep, as lane ln of a row loads them: row j of L_k, ivl / ibl: entry ln of innov_k and of
// innov_bar_k, xhb: Xhat_bar_k[j] and zb0: Zbar's entry ln of the knot (every knot); z0 / z1 and zb0 / zb1 as in JvpKnot, of Zout
// and of Zbar, xh: xhat_k[j], xr: x_ref,j, kc: column j of K_k (the knots with a step).
struct EstimatedVjpKnot {
    double l[QLN_TRACK_NY_MAX], ivl, ibl, xhb;
    double z0, z1, zb0, zb1, xh, xr, kc[4];
};

// One chain's knot of the reverse sweep: column j of [A B G]' on lam; returns (A'lam)[j], ub = ub0 + (B'lam, the h column's
// product), and (kModel) adds to mbar.  kGuard: the guarded reverse sweep's statement of the knot (k_tracking_rollout_vjp),
// td saying that this is the chain's touchdown knot; the estimator's chain (kModel false) has no model cotangent to hand
// tau's to.
template <bool kGuard, bool kModel>
__device__ __forceinline__ double estimated_vjp_step(const VjpLane& lc, const double (&e)[4], const double (&sg)[4], int ln, bool own,
                                                     double xj, double F0, double F1, double F2, double F3, double h,
                                                     const KnotMode& md, bool td, double tau, const Model& M, double lam,
                                                     bool want_mbar, double (&mbar)[QLN_MODEL_NP], const double (&ub0)[5],
                                                     double (&ub)[5]) {
    if constexpr (!kGuard) {
        return vjp_apply_column<kModel>(lc, e, sg, xj, F0, F1, F2, F3, h, md, M, lam, want_mbar, mbar, ub0, ub);
    } else {
        const int j = lc.j;
        double lamA = lam, hA = h, hb3 = 0.0, w = 1.0, y = 0.0;
        double ubA[5] = {ub0[0], ub0[1], ub0[2], ub0[3], ub0[4]};
        if (td) {
            double xk[15], xm[15];
            row_bcast_first(xj, xk, std::make_integer_sequence<int, 15>{});
            const double u5[5] = {F0, F1, F2, F3, h};
            step_mode(M, md, tau, xk, u5, xm);
            y = md.f2free ? xk[6] : xk[4];
            w = md.f2free ? xm[13] : xm[11];
            jump_map(xm);
            // the mode-3 leg at (x+, F, h - tau)
            ubA[4] = 0.0;
            double ub3[5];
            const double a3 = vjp_apply_column<kModel>(lc, e, sg, pick15(xm, j), F0, F1, F2, F3, h - tau,
                                                       KnotMode{false, false, false, true}, M, lam, want_mbar, mbar, ubA, ub3);
#pragma unroll
            for (int m = 0; m < 4; ++m) ubA[m] = ub3[m];
            hb3 = ub3[4];
            lamA = (own && !lc.jrow) ? a3 : 0.0;  // the jump map
            hA = tau;
        }
        double alam = vjp_apply_column<kModel>(lc, e, sg, xj, F0, F1, F2, F3, hA, md, M, lamA, want_mbar, mbar, ubA, ub);
        if (td) {
            // tau's cotangent, and d tau = -(dy + tau dv + tau^2/2 da) / w with da = -dF_y / mf + F_y / mf^2 dmf + dg
            const double taubar = ub[4] - hb3;
            ub[4] = ub0[4] + hb3;
            const bool f2 = md.f2free;
            const double cw = (y <= 0.0) ? 0.0 : -taubar / w, ca = cw * (0.5 * tau * tau);
            const int iy = f2 ? 6 : 4, iv = f2 ? 13 : 11;
            alam = (j == iy) ? alam + cw : (j == iv) ? fma(cw, tau, alam) : alam;
            const double Fy = f2 ? F3 : F1, cf = -ca / M.mf;
            ub[1] = f2 ? ub[1] : ub[1] + cf;
            ub[3] = f2 ? ub[3] + cf : ub[3];
            if constexpr (kModel) {
                if (ln == 0) {
                    mbar[0] += ca;
                    mbar[2] = fma(ca, Fy / (M.mf * M.mf), mbar[2]);
                }
            }
        }
        return alam;
    }
}

// lane j's constant pattern at the model M (k_tracking_rollout_vjp forms the same before its loop)
__device__ __forceinline__ VjpLane vjp_lane(int j, const Model& M) {
    const bool pos = j < 7;
    const int p = pos ? j : j - 7;
    const int foot = (p == 3 || p == 4) ? 1 : (p == 5 || p == 6) ? 2 : 0;
    const bool jrow = j == 4 || j == 6 || (j >= 10 && j <= 13);
    const bool cpl = j >= 7 && j <= 13;
    const bool kcpl = j == 11 || j == 13;
    const double g = M.g, imb = 1.0 / M.mb, imf = 1.0 / M.mf;
    const double iIb = 12.0 / (M.mb * (M.lb * M.lb));
    const double inv = (p <= 1) ? imb : foot ? -imf : 0.0;
    const double gy = (p == 1 || p == 4 || p == 6) ? g : (j == 14) ? 1.0 : 0.0;
    return {j, pos, foot, jrow, cpl, kcpl, inv, gy, g, iIb};
}

// The reverse sweep (include/qln_evaluator.h), the exact transpose of the forward one: lam (of dx) and lamm (of dxm) start at
// zero behind the last knot, and per knot k = N-1 .. 0
//   k < N-1:  ubar = Zbar[u_k] + B^p'lam + B^e'lamm,  ax = A^p'lam,  model_bar += G^p'lam,
//             xhb = Xhat_bar_k + A^e'lamm - K_k'ubar[0:4]                                   (k = N-1: ax = 0, xhb = Xhat_bar_k)
//   ib = innov_bar_k + L_k'xhb,   Lbar_k = xhb innov_k',   lam = Zbar[x_k] + ax + H'ib,   lamm = xhb - H'ib
// with Zref_bar[x_k] = K_k'ubar[0:4], Zref_bar[u_k] = ubar, Kbar_k = -ubar[0:4] (xhat_k - x_ref,k)'.  The plant's chain is applied
// first, onto Zbar[u_k], as k_tracking_rollout_vjp applies it; the estimator's adds to it.
// kHasK: K is given; kHasLb: Lgain_bar is asked for, and innov given with it.
// kLimit (qln_tracking_rollout_estimated_limited_vjp): ubar[0:4] of a channel that rode a limit at knot k (sat)
// is zero after both chains' B' and taubar have been added onto it and before K_k'ubar, K_bar and Zref_bar read it, so that the
// sweep is the exact transpose of the limited forward one.  The knot's code is loaded one knot ahead in a slot of the knot's
// slices (estimated_knot_load).
template <bool kGuard, bool kHasK, bool kHasLb, bool kLimit = false>
__global__ __launch_bounds__(kWave) void k_tracking_rollout_estimated_vjp(BatchParams P, EstimatedSweepIn in, EstimatedVjpArgs a,
                                                                          const double* __restrict__ sat) {
    constexpr int NY = QLN_TRACK_NY_MAX;
    __shared__ double Hs[NY * 15];
    const int ny = in.ny;
    for (int i = threadIdx.x; i < 15 * ny; i += kWave) Hs[i] = in.H[i];
    __syncthreads();
    const Row16 r16 = row16_of(P);  // lane 15 reads lane 14's slots and contributes nothing
    const int ln = r16.ln, j = r16.j, b = r16.b, bc = r16.bc, kt = r16.kt, im = r16.im, N = P.N;
    const bool own = r16.own, valid = r16.valid;
    const Model M = plant_model<true>(P, in.model, bc);
    const Model Mh = plant_model<true>(P, nullptr, bc);
    const int64_t zo = (int64_t)bc * P.z_stride, ko = (int64_t)bc * (N - 1) * (QLN_TRACK_NU * QLN_NX);
    const int64_t xo = (int64_t)bc * N * QLN_NX, go = xo * ny, io = (int64_t)bc * N * ny;
    const double* __restrict__ Zo = in.Zout + zo;
    const double* __restrict__ Zb = a.Zbar + zo;
    const double* __restrict__ Xh = in.Xhat + xo;
    const double* __restrict__ Zr = a.K_bar ? in.Zref + zo : nullptr;
    const double* __restrict__ Kb = kHasK ? in.K + ko : nullptr;
    const double* __restrict__ Lb = in.Lgain + go + (int64_t)j * ny;
    const double* __restrict__ Ib = kHasLb ? in.innov + io : nullptr;
    [[maybe_unused]] int ks = -1, ksh = -1;
    [[maybe_unused]] double tau = 0.0, tauh = 0.0;
    if constexpr (kGuard) {
        ks = guard_knot(in.event[(int64_t)QLN_TOUCHDOWN_INFO_STRIDE * bc], N);
        tau = in.event[(int64_t)QLN_TOUCHDOWN_INFO_STRIDE * bc + 1];
        ksh = guard_knot(in.event_hat[(int64_t)QLN_TOUCHDOWN_INFO_STRIDE * bc], N);
        tauh = in.event_hat[(int64_t)QLN_TOUCHDOWN_INFO_STRIDE * bc + 1];
    }
    // ---- lane j's constant pattern, at each chain's model; the sign patterns are the models' alike ----
    const VjpLane lc = vjp_lane(j, M), lch = vjp_lane(j, Mh);
    const int p = lc.pos ? j : j - 7;
    double e[4], sg[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        e[m] = ((p <= 1 && (m == p || m == p + 2)) || (lc.foot && m == p - 3)) ? 1.0 : 0.0;
        sg[m] = 0.0;
    }
    if (p == 0) sg[1] = sg[3] = -1.0;
    if (p == 1) sg[0] = sg[2] = 1.0;
    if (p == 3) sg[1] = 1.0;
    if (p == 4) sg[0] = -1.0;
    if (p == 5) sg[3] = 1.0;
    if (p == 6) sg[2] = -1.0;

    double mbar[QLN_MODEL_NP] = {0.0, 0.0, 0.0, 0.0};   // lane j's share of model_bar
    double none[QLN_MODEL_NP] = {0.0, 0.0, 0.0, 0.0};   // the estimator's model has no cotangent
    double lam = 0.0, lamm = 0.0;
    // the knot's slices are loaded one knot ahead: the gains' row and the cotangents for every knot, the rest for the knots that
    // take a step
    const double* __restrict__ Xhb = a.Xhat_bar ? a.Xhat_bar + xo : nullptr;
    const double* __restrict__ Ibb = a.innov_bar ? a.innov_bar + io : nullptr;
    [[maybe_unused]] const double* __restrict__ Sb = kLimit ? sat + (int64_t)bc * (N - 1) : nullptr;
    auto load = [&](EstimatedVjpKnot& s, int k) {
        const double* __restrict__ Lk = Lb + (int64_t)k * (15 * ny);
#pragma unroll
        for (int r = 0; r < NY; ++r) s.l[r] = r < ny ? Lk[r] : 0.0;
        if constexpr (kHasLb) s.ivl = Ib[(int64_t)k * ny + min(ln, ny - 1)];
        if (Ibb) s.ibl = Ibb[(int64_t)k * ny + min(ln, ny - 1)];
        if (Xhb) s.xhb = Xhb[(int64_t)k * QLN_NX + j];
        if (k == N - 1) {
            s.zb0 = Zb[20 * k + j];  // the last knot has no controls
            return;
        }
        estimated_knot_load<kLimit>(Zo + 20 * k, kLimit ? Sb + k : nullptr, ln, s.z0, s.z1);
        knot_load(Zb + 20 * k, ln, s.zb0, s.zb1);
        s.xh = Xh[(int64_t)k * QLN_NX + j];
        if constexpr (kHasK) {
#pragma unroll
            for (int m = 0; m < 4; ++m) s.kc[m] = Kb[60 * (int64_t)k + 15 * m + j];
        }
        if (Zr) s.xr = Zr[20 * k + j];
    };
    EstimatedVjpKnot cur = {}, nxt = {};
    load(nxt, N - 1);
    for (int k = N - 1; k >= 0; --k) {
        cur = nxt;
        if (k > 0) load(nxt, k - 1);
        double xhb = (own && Xhb) ? cur.xhb : 0.0;
        double ax = 0.0, kub = 0.0;
        double ub[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (k < N - 1) {
            const double xj = own ? cur.z0 : row_bcast<14>(cur.z0), xhj = cur.xh;
            const double u[5] = {row_bcast<15>(cur.z0), row_bcast<0>(cur.z1), row_bcast<1>(cur.z1), row_bcast<2>(cur.z1),
                                 row_bcast<3>(cur.z1)};
            const double ubz[5] = {row_bcast<15>(cur.zb0), row_bcast<0>(cur.zb1), row_bcast<1>(cur.zb1), row_bcast<2>(cur.zb1),
                                   row_bcast<3>(cur.zb1)};
            double ubp[5];
            KnotMode md, mdh;
            if constexpr (kGuard) {
                md = guard_mode(k, ks, im);
                mdh = guard_mode(k, ksh, im);
            } else {
                md = mdh = knot_mode(k + 1, kt - 1, im);
            }
            ax = estimated_vjp_step<kGuard, true>(lc, e, sg, ln, own, xj, u[0], u[1], u[2], u[3], u[4], md, k == ks, tau, M, lam,
                                                  a.model_bar != nullptr, mbar, ubz, ubp);
            __builtin_amdgcn_sched_barrier(0);  // one chain after the other: two knots' temporaries at once do not fit
            const double axh = estimated_vjp_step<kGuard, false>(lch, e, sg, ln, own, xhj, u[0], u[1], u[2], u[3], u[4], mdh, k == ksh,
                                                                 tauh, Mh, lamm, false, none, ubp, ub);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (kLimit) {
                const unsigned lmask = limit_mask(row_bcast<4>(cur.z1));
#pragma unroll
                for (int m = 0; m < 4; ++m) ub[m] = limited(lmask, m) ? 0.0 : ub[m];
            }
            if constexpr (kHasK) kub = ((cur.kc[0] * ub[0] + cur.kc[1] * ub[1]) + cur.kc[2] * ub[2]) + cur.kc[3] * ub[3];
            xhb = own ? (xhb + axh) - kub : 0.0;
            if (kHasK && a.K_bar && valid && own) {
                double* __restrict__ o = a.K_bar + ((int64_t)b * (N - 1) + k) * (QLN_TRACK_NU * QLN_NX);
                const double dxr = xhj - cur.xr;
#pragma unroll
                for (int m = 0; m < 4; ++m) o[15 * m + j] = -ub[m] * dxr;
            }
        }
        // ---- the measurement update, transposed ----
        [[maybe_unused]] double iv[NY], ibr[NY];
        if constexpr (kHasLb) row_bcast_first(cur.ivl, iv, std::make_integer_sequence<int, NY>{});
        if (Ibb) row_bcast_first(cur.ibl, ibr, std::make_integer_sequence<int, NY>{});
        double hib = 0.0;
#pragma unroll
        for (int r = 0; r < NY; ++r) {
            if (r < ny) {
                double ib = row_sum16(own ? cur.l[r] * xhb : 0.0);
                if (Ibb) ib = ibr[r] + ib;
                hib = fma(Hs[15 * r + j], ib, hib);
                if constexpr (kHasLb) {
                    if (valid && own) a.Lgain_bar[((int64_t)b * N + k) * (15 * ny) + (int64_t)j * ny + r] = xhb * iv[r];
                }
            }
        }
        const double zbx = own ? cur.zb0 : 0.0;
        lam = own ? (zbx + ax) + hib : 0.0;
        lamm = own ? xhb - hib : 0.0;
        if (valid && a.Zref_bar) {
            double* __restrict__ zk = a.Zref_bar + (int64_t)b * P.z_stride + 20 * k;
            const double x0slot = (k == 0 && !a.xhat0_bar) ? kub + lamm : kub;  // xhat0 == NULL: xhat^-_0 is x_ref,0
            if (k < N - 1) knot_store(zk, r16, x0slot, ub);
            else if (own) zk[j] = x0slot;
        }
    }
    if (valid && own) {
        if (a.x0_bar) a.x0_bar[(int64_t)b * QLN_NX + j] = lam;
        if (a.xhat0_bar) a.xhat0_bar[(int64_t)b * QLN_NX + j] = lamm;
    }
    if (a.model_bar) {
        double out = 0.0;
#pragma unroll
        for (int q = 0; q < QLN_MODEL_NP; ++q) {
            const double sq = row_sum16(mbar[q]);
            out = (ln == q) ? sq : out;
        }
        if (valid && ln < QLN_MODEL_NP) a.model_bar[(int64_t)b * QLN_MODEL_NP + ln] = out;
    }
}

// ---- k_landing_filter ----
// entry (r, c), c <= r, of a packed lower triangle of QLN_TRACK_NY_MAX rows
__host__ __device__ constexpr int filter_tri(int r, int c) { return r * (r + 1) / 2 + c; }
constexpr int kFilterTri = filter_tri(QLN_TRACK_NY_MAX - 1, QLN_TRACK_NY_MAX - 1) + 1;  // 36

// The filter on recorded data (qln_landing_filter / _guarded, include/qln_evaluator.h): the estimator's half of
// k_tracking_rollout_estimated in that kernel's mapping, one lane per problem, with the measurement read from Y and the applied
// forces from Zrec where that kernel forms both from a plant it integrates.  H goes to LDS once per block, all eight rows, the
// rows behind ny as zeros.  yh, the update xhat += L_k innov and the estimator's step are that kernel's expressions in that
// kernel's order, and L_k is read row by row for its reason, so a replay of a flight returns the flight's bits.
// kGuard: the step is guarded_step on the estimator's own contact mode and Touchdown record, written to event_hat.
// kScore: nis_k, log det S_k and the log-likelihood from the gains alone, S_k^-1 = V^-1 (I - H L_k).  Under the same pass
// over L_k's rows the lane accumulates g = L_k innov_k (apart from xhat, whose size would swamp it) and the lower triangle of
// H L_k; then e_k = innov_k - H g, nis_k = sum_r innov_k[r] e_k[r] / V[r], and the L D L' of the lower triangle of
// diag(1/V) (I - H L_k) without pivoting, right-looking and in place, whose pivots give log det S_k = - sum log d_i (NaN where
// a pivot is not > 0).  The rows behind ny have a zero row of H and V = 1: pivot 1, log 1 = 0, and zeros everywhere else.
// kModel (qln_landing_filter_model / _guarded_model): the step is taken at the record's own model, model[b].  Its
// four doubles are read at the step, every knot, behind a hidden address: held over the knots, a lane's own Model would sit
// beside the score's accumulators, which leave no register free.  A null model there is the handle's four values.
template <bool kGuard, bool kScore, bool kModel = false>
__global__ __launch_bounds__(kWave) void k_landing_filter(BatchParams P, SmootherNoise Nz, const double* __restrict__ Hg, int ny,
                                                          const double* __restrict__ Zref, const double* __restrict__ Zrec,
                                                          const double* __restrict__ Lg, const double* __restrict__ Yg,
                                                          const double* __restrict__ xhat0, double* __restrict__ Xhat,
                                                          double* __restrict__ innov_out, double* __restrict__ score,
                                                          double* __restrict__ loglik, double* __restrict__ event_hat,
                                                          const double* __restrict__ model) {
    constexpr int NY = QLN_TRACK_NY_MAX;
    __shared__ double Hs[NY * 15];
    for (int i = threadIdx.x; i < NY * 15; i += kWave) Hs[i] = i < 15 * ny ? Hg[i] : 0.0;
    // 1 / V beside it: held in scalar registers over the knots, the eight took more of them than there are
    [[maybe_unused]] __shared__ double Vs[NY];
    if constexpr (kScore) {
#pragma unroll
        for (int r = 0; r < NY; ++r)
            if ((int)threadIdx.x == r) Vs[r] = Nz.iv[r];
    }
    __syncthreads();
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= P.B) return;
    const ProblemDesc pd = P.desc[b];
    const int N = P.N, kt = pd.k_trans, im = pd.init_mode;
    [[maybe_unused]] const Model Mh = plant_model<true>(P, nullptr, b);  // the estimator's: the handle's without kModel
    const double* __restrict__ Zr = Zref + (int64_t)b * P.z_stride;
    const double* __restrict__ Zc = Zrec + (int64_t)b * P.z_stride;
    const double* __restrict__ hs = xhat0 ? xhat0 + (int64_t)b * 15 : Zr;
    const double* __restrict__ Lb = Lg + (int64_t)b * N * (15 * ny);
    const double* __restrict__ yb = Yg + (int64_t)b * N * ny;
    double xhat[15], u[5], xn[15];
#pragma unroll
    for (int i = 0; i < 15; ++i) xhat[i] = hs[i];
    [[maybe_unused]] int mode_hat = im;
    [[maybe_unused]] Touchdown tdh = {-1.0, 0.0, 0.0, 0.0, 0.0, 0.0, __builtin_inf()};
    [[maybe_unused]] double ll = 0.0;
    for (int k = 0; k < N; ++k) {
        // innov_k = Y_k - H (xhat^-_k - x_ref,k); the rows behind ny are zeros
        double innov[NY];
        {
            double e[15];
#pragma unroll
            for (int i = 0; i < 15; ++i) e[i] = xhat[i] - Zr[20 * k + i];
#pragma unroll
            for (int r = 0; r < NY; ++r) {
                innov[r] = 0.0;
                if (r < ny) {
                    double yh = Hs[15 * r] * e[0];
#pragma unroll
                    for (int i = 1; i < 15; ++i) yh = fma(Hs[15 * r + i], e[i], yh);
                    innov[r] = yb[(int64_t)ny * k + r] - yh;
                    if (innov_out) innov_out[((int64_t)b * N + k) * ny + r] = innov[r];
                }
            }
        }
        // xhat_k = xhat^-_k + L_k innov_k as k_tracking_rollout_estimated forms it: row i of L_k is ny consecutive doubles, a
        // column behind ny reads the row's last entry against a zero innovation (or a zero row of H), three rows in flight
        [[maybe_unused]] double g[15], hl[kFilterTri];
        if constexpr (kScore) {
#pragma unroll
            for (int t = 0; t < kFilterTri; ++t) hl[t] = 0.0;
        }
        {
            const double* Li = Lb + (int64_t)k * (15 * ny);
#pragma unroll
            for (int i = 0; i < 15; ++i) {
                if constexpr (kScore) {
                    double lr[NY];
#pragma unroll
                    for (int r = 0; r < NY; ++r) lr[r] = Li[min(r, ny - 1)];
#pragma unroll
                    for (int r = 0; r < NY; ++r) xhat[i] = fma(lr[r], innov[r], xhat[i]);
                    double gi = lr[0] * innov[0];
#pragma unroll
                    for (int r = 1; r < NY; ++r) gi = fma(lr[r], innov[r], gi);
                    g[i] = gi;
                    // column i of H at an offset hidden from the optimiser: H does not change over the knots, and 120 reads at
                    // known addresses may be hoisted out of the knot loop into registers this kernel does not have
                    int hi = i;
                    asm volatile("" : "+v"(hi));
#pragma unroll
                    for (int r = 0; r < NY; ++r) {
                        const double hr = Hs[15 * r + hi];
#pragma unroll
                        for (int c = 0; c <= r; ++c) hl[filter_tri(r, c)] = fma(hr, lr[c], hl[filter_tri(r, c)]);
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < NY; ++r) xhat[i] = fma(Li[min(r, ny - 1)], innov[r], xhat[i]);
                }
                Li += ny;
                asm volatile("" : "+v"(Li));
                if constexpr (kScore) {
                    // the sums are formed where the rows are read: left to the optimiser they sank below the branches that
                    // follow, to their first use, and L_k's 120 entries stayed live until there, which spilled
                    asm volatile("" : "+v"(g[i]));
                    if (i % 3 == 2) {
#pragma unroll
                        for (int t = 0; t < kFilterTri; ++t) asm volatile("" : "+v"(hl[t]));
                    }
                }
                if (i % 3 == 2) __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (Xhat) {
            double* __restrict__ Xk = Xhat + ((int64_t)b * N + k) * 15;
#pragma unroll
            for (int i = 0; i < 15; ++i) Xk[i] = xhat[i];
        }
        if constexpr (kScore) {
            double nis = 0.0;
#pragma unroll
            for (int r = 0; r < NY; ++r) {
                int hr = 15 * r;  // hidden for the same reason
                asm volatile("" : "+v"(hr));
                double hg = Hs[hr] * g[0];
#pragma unroll
                for (int i = 1; i < 15; ++i) hg = fma(Hs[hr + i], g[i], hg);
                nis = nis + innov[r] * (innov[r] - hg) * Vs[hr - 14 * r];
            }
            // formed here, for the same reason: the eight logarithms below branch
            asm volatile("" : "+v"(nis));
            // G = the lower triangle of diag(1/V) (I - H L_k), then its L D L' in place: column j's pivot, the column scaled, and
            // the trailing triangle less the column's outer product
#pragma unroll
            for (int r = 0; r < NY; ++r) {
                int vr = r;  // hidden as H's offsets are
                asm volatile("" : "+v"(vr));
                const double ivr = Vs[vr];
#pragma unroll
                for (int c = 0; c <= r; ++c) hl[filter_tri(r, c)] = ivr * ((r == c ? 1.0 : 0.0) - hl[filter_tri(r, c)]);
            }
            double lds = 0.0;
#pragma unroll
            for (int j = 0; j < NY; ++j) {
                const double dj = hl[filter_tri(j, j)];
                lds = lds + (dj > 0.0 ? log(dj) : __builtin_nan(""));
                const double inv = 1.0 / dj;
#pragma unroll
                for (int i = j + 1; i < NY; ++i) {
                    const double lij = hl[filter_tri(i, j)] * inv;
#pragma unroll
                    for (int c = j + 1; c <= i; ++c) hl[filter_tri(i, c)] = hl[filter_tri(i, c)] - lij * hl[filter_tri(c, j)];
                }
            }
            lds = -lds;
            if (score) {
                double* __restrict__ sk = score + ((int64_t)b * N + k) * 2;
                sk[0] = nis;
                sk[1] = lds;
            }
            ll = ll + ((nis + lds) + (double)ny * 1.8378770664093454836);  // log 2 pi
        }
        if (k == N - 1) break;
        // the applied forces and the step length are the record's
#pragma unroll
        for (int i = 0; i < 5; ++i) u[i] = Zc[20 * k + 15 + i];
        if constexpr (kModel) {
            const double* mp = model;
            asm volatile("" : "+v"(mp));
            const Model Mb = plant_model<true>(P, mp, b);
            if constexpr (kGuard) guarded_step(Mb, k, mode_hat, xhat, u, xn, tdh);
            else step_forward(Mb, k, kt, im, xhat, u, xn);
        } else {
            if constexpr (kGuard) guarded_step(Mh, k, mode_hat, xhat, u, xn, tdh);
            else step_forward(Mh, k, kt, im, xhat, u, xn);
        }
#pragma unroll
        for (int i = 0; i < 15; ++i) xhat[i] = xn[i];
    }
    if constexpr (kScore) {
        if (loglik) loglik[b] = -0.5 * ll;
    }
    if constexpr (kGuard) {
        if (event_hat) {
            double* __restrict__ ev = event_hat + (int64_t)QLN_TOUCHDOWN_INFO_STRIDE * b;
            ev[0] = tdh.knot;
            ev[1] = tdh.tau;
            ev[2] = tdh.clock;
            ev[3] = tdh.px;
            ev[4] = tdh.vx;
            ev[5] = tdh.vy;
            ev[6] = tdh.fmin;
            ev[7] = 0.0;
        }
    }
}

// ---- k_landing_filter_jvp / k_landing_filter_vjp ----
// The sweeps through the filter (qln_landing_filter_jvp / _vjp, include/qln_evaluator.h): the estimator's half
// of k_tracking_rollout_estimated_jvp / _vjp in their mapping -- one problem per row of sixteen lanes, lane j holding dxm[j] /
// lamm[j], H staged once per block, row j of L_k, every knot slice loaded one knot ahead, what is uniform over the row handed
// round by DPP row broadcasts -- with the model's tangent on that half: the block is estimated_jvp_step<kGuard, true> /
// estimated_vjp_step<kGuard, true> at (Xhat_k, Zrec's u_k, model[b]).  With no tangent but xhat0's and Lgain's the estimator's
// chain of the siblings is repeated expression for expression, so a replay of a flight returns their bits.
// kScore: the tangent and the cotangent of nis_k.  In this mapping g = L_k innov_k and L_k dinnov_k are one fma chain per lane,
// and H g, H (L_k dinnov_k) and L_k' (H' w) are ny row sums each: nothing is factorised.  V enters as 1 / V, 1 behind ny.

// One knot's inputs of the forward sweep, as lane ln of a row loads them: row j of L_k and of Ldot_k, ivl / ydl: entry ln of
// innov_k and of Y_dot_k (lanes behind ny repeat the last), for every knot; z0 / z1 and zd0 / zd1: Zrec's and Zrec_dot's knot as
// knot_load takes it (only the control slots are used), xh: xhat_k[j], for the knots with a step.
struct FilterJvpKnot {
    double l[QLN_TRACK_NY_MAX], ld[QLN_TRACK_NY_MAX], ivl, ydl;
    double z0, z1, xh, zd0, zd1;
};

template <bool kGuard, bool kHasLd, bool kScore>
__global__ __launch_bounds__(kWave) void k_landing_filter_jvp(BatchParams P, FilterSweepIn in, FilterJvpArgs a) {
    static_assert(!(kHasLd && kScore), "the score's tangent is taken at fixed gains");
    constexpr int NY = QLN_TRACK_NY_MAX;
    constexpr bool kInnov = kHasLd || kScore;
    __shared__ double Hs[NY * 15];
    const int ny = in.ny;
    for (int i = threadIdx.x; i < 15 * ny; i += kWave) Hs[i] = in.H[i];
    // 1 / V beside it, read at a hidden offset (k_landing_filter): held in scalar registers over the knots the eight took sixteen
    [[maybe_unused]] __shared__ double Vs[NY];
    if constexpr (kScore) {
#pragma unroll
        for (int r = 0; r < NY; ++r)
            if ((int)threadIdx.x == r) Vs[r] = in.iv[r];
    }
    __syncthreads();
    const Row16 r16 = row16_of(P);  // lane 15 reads lane 14's slots and contributes nothing
    const int ln = r16.ln, j = r16.j, bc = r16.bc, kt = r16.kt, im = r16.im, N = P.N;
    const bool own = r16.own, valid = r16.valid;
    const Model M = plant_model<true>(P, in.model, bc);
    const int64_t zo = (int64_t)bc * P.z_stride, xo = (int64_t)bc * N * QLN_NX, go = xo * ny, io = (int64_t)bc * N * ny;
    const double* __restrict__ Zc = in.Zrec + zo;
    const double* __restrict__ Xh = in.Xhat + xo;
    const double* __restrict__ Zd = a.Zrec_dot ? a.Zrec_dot + zo : nullptr;
    const double* __restrict__ Yd = a.Y_dot ? a.Y_dot + io : nullptr;
    const double* __restrict__ Lb = in.Lgain + go + (int64_t)j * ny;
    const double* __restrict__ Ldb = kHasLd ? a.Lgain_dot + go + (int64_t)j * ny : nullptr;
    const double* __restrict__ Ib = kInnov ? in.innov + io : nullptr;
    [[maybe_unused]] int ksh = -1;
    [[maybe_unused]] double tauh = 0.0;
    double eh_tau = 0.0, eh_clock = 0.0;
    if constexpr (kGuard) {
        ksh = guard_knot(in.event_hat[(int64_t)QLN_TOUCHDOWN_INFO_STRIDE * bc], N);
        tauh = in.event_hat[(int64_t)QLN_TOUCHDOWN_INFO_STRIDE * bc + 1];
    }
    double md4[QLN_MODEL_NP] = {0.0, 0.0, 0.0, 0.0};
    if (a.model_dot) {
#pragma unroll
        for (int q = 0; q < QLN_MODEL_NP; ++q) md4[q] = a.model_dot[(int64_t)bc * QLN_MODEL_NP + q];
    }
    double* __restrict__ Xd = a.Xhat_dot ? a.Xhat_dot + xo : nullptr;
    double* __restrict__ Ido = a.innov_dot ? a.innov_dot + io : nullptr;
    double dxm = (own && a.xhat0_dot) ? a.xhat0_dot[(int64_t)bc * QLN_NX + j] : 0.0;
    [[maybe_unused]] double lld = 0.0;
    auto load = [&](FilterJvpKnot& s, int k) {
        const double* __restrict__ Lk = Lb + (int64_t)k * (15 * ny);
#pragma unroll
        for (int r = 0; r < NY; ++r) s.l[r] = r < ny ? Lk[r] : 0.0;
        if constexpr (kHasLd) {
            const double* __restrict__ Ldk = Ldb + (int64_t)k * (15 * ny);
#pragma unroll
            for (int r = 0; r < NY; ++r) s.ld[r] = r < ny ? Ldk[r] : 0.0;
        }
        if constexpr (kInnov) s.ivl = Ib[(int64_t)k * ny + min(ln, ny - 1)];
        if (Yd) s.ydl = Yd[(int64_t)k * ny + min(ln, ny - 1)];
        if (k == N - 1) return;
        knot_load(Zc + 20 * k, ln, s.z0, s.z1);
        s.xh = Xh[(int64_t)k * QLN_NX + j];
        if (Zd) knot_load(Zd + 20 * k, ln, s.zd0, s.zd1);
    };
    FilterJvpKnot cur = {}, nxt = {};
    load(nxt, 0);
    for (int k = 0; k < N; ++k) {
        // the row count behind a hidden value, once per knot: the eight tests r < ny, held over the step, cost scalar registers
        int nyk = ny;
        asm volatile("" : "+s"(nyk));
        cur = nxt;
        if (k + 1 < N) load(nxt, k + 1);
        // ---- the measurement update's tangent: dinnov = Y_dot - H dxm, formed as the siblings form H (dx - dxm) at dx = 0 ----
        const double dd = 0.0 - dxm;
        double din[NY];
        [[maybe_unused]] double yd[NY], iv[NY];
        if (Yd) row_bcast_first(cur.ydl, yd, std::make_integer_sequence<int, NY>{});
        if constexpr (kInnov) row_bcast_first(cur.ivl, iv, std::make_integer_sequence<int, NY>{});
#pragma unroll
        for (int r = 0; r < NY; ++r) {
            din[r] = 0.0;
            if (r < nyk) {
                din[r] = row_sum16(own ? Hs[15 * r + j] * dd : 0.0);
                if (Yd) din[r] = yd[r] + din[r];
            }
        }
        double dxh = dxm;
#pragma unroll
        for (int r = 0; r < NY; ++r)
            if (r < nyk) dxh = fma(cur.l[r], din[r], dxh);
        if constexpr (kHasLd) {
#pragma unroll
            for (int r = 0; r < NY; ++r)
                if (r < nyk) dxh = fma(cur.ld[r], iv[r], dxh);
        }
        dxh = own ? dxh : 0.0;
        if constexpr (kScore) {
            // e = innov - H (L innov), de = dinnov - H (L dinnov), nis_dot = sum_r (dinnov[r] e[r] + innov[r] de[r]) / V[r]
            double g = 0.0, gd = 0.0;
#pragma unroll
            for (int r = 0; r < NY; ++r)
                if (r < nyk) {
                    g = fma(cur.l[r], iv[r], g);
                    gd = fma(cur.l[r], din[r], gd);
                }
            double nd = 0.0;
            int vo = 0;
            asm volatile("" : "+v"(vo));
#pragma unroll
            for (int r = 0; r < NY; ++r)
                if (r < nyk) {
                    const double e = iv[r] - row_sum16(own ? Hs[15 * r + j] * g : 0.0);
                    const double de = din[r] - row_sum16(own ? Hs[15 * r + j] * gd : 0.0);
                    nd = fma(fma(din[r], e, iv[r] * de), Vs[vo + r], nd);
                }
            lld = lld + nd;
            if (valid && ln == 0 && a.nis_dot) a.nis_dot[(int64_t)bc * N + k] = nd;
        }
        if (valid) {
            if (Xd && own) Xd[(int64_t)k * QLN_NX + j] = dxh;
            if (Ido && ln < ny) {
                int lk = ln;  // hidden, as the lane's index is below
                asm volatile("" : "+v"(lk));
                double o = din[0];
#pragma unroll
                for (int r = 1; r < NY; ++r) o = (lk == r) ? din[r] : o;
                Ido[(int64_t)k * ny + ln] = o;
            }
        }
        if (k == N - 1) break;
        // ---- the estimate and the record's controls, in every lane; the controls' tangent ----
        const double z0 = cur.z0, z1 = cur.z1;
        double xe[14];
        row_bcast_first(cur.xh, xe, std::make_integer_sequence<int, 14>{});
        const double F1x = row_bcast<15>(z0), F1y = row_bcast<0>(z1), F2x = row_bcast<1>(z1), F2y = row_bcast<2>(z1),
                     h = row_bcast<3>(z1);
        double dF[4] = {0.0, 0.0, 0.0, 0.0}, dh = 0.0;
        if (Zd) {
            dF[0] = row_bcast<15>(cur.zd0);
            dF[1] = row_bcast<0>(cur.zd1);
            dF[2] = row_bcast<1>(cur.zd1);
            dF[3] = row_bcast<2>(cur.zd1);
            dh = row_bcast<3>(cur.zd1);
        }
        KnotMode mdh;
        if constexpr (kGuard) mdh = guard_mode(k, ksh, im);
        else mdh = knot_mode(k + 1, kt - 1, im);
        // the lane's index behind a hidden value: the block's entries are picked by comparisons with it, and held over the knots
        // as lane masks those comparisons took more scalar registers than there are
        int jk = j;
        asm volatile("" : "+v"(jk));
        const double acce = estimated_jvp_step<kGuard, true>(jk, own, xe, F1x, F1y, F2x, F2y, h, mdh, k == ksh, tauh, M, dxh, dF, dh,
                                                             a.model_dot != nullptr, md4, eh_tau, eh_clock);
        __builtin_amdgcn_sched_barrier(0);
        dxm = own ? acce : 0.0;
    }
    if constexpr (kScore) {
        if (valid && ln == 0 && a.loglik_dot) a.loglik_dot[bc] = -0.5 * lld;
    }
    if constexpr (kGuard) {
        if (valid && ln < QLN_TOUCHDOWN_INFO_STRIDE && a.event_hat_dot)
            a.event_hat_dot[(int64_t)QLN_TOUCHDOWN_INFO_STRIDE * bc + ln] = (ln == 1) ? eh_tau : (ln == 2) ? eh_clock : 0.0;
    }
}

// One knot's inputs of the reverse sweep, as lane ln of a row loads them: row j of L_k, ivl / ibl: entry ln of innov_k and of
// innov_bar_k, xhb: Xhat_bar_k[j], nb: nis_bar_k (every knot); z0 / z1: Zrec's knot, xh: xhat_k[j] (the knots with a step).
struct FilterVjpKnot {
    double l[QLN_TRACK_NY_MAX], ivl, ibl, xhb, nb;
    double z0, z1, xh;
};

// The exact transpose of the forward sweep: lamm, the cotangent of dxm_{k+1}, starts at zero behind the last knot, and per knot
//   k < N-1:  ubar = B^e'lamm,  xhb = Xhat_bar_k + A^e'lamm,  model_bar += G^e'lamm                (k = N-1: xhb = Xhat_bar_k)
//   ib = innov_bar_k + L_k'xhb + nb_k (G_k + G_k') innov_k,   Lbar_k = xhb innov_k',   lamm = xhb - H'ib
// with nb_k = nis_bar_k - loglik_bar / 2 and G_k = diag(1/V) (I - H L_k), the full matrix:
//   ((G + G') innov)[r] = (e[r] / V[r] + w[r]) - (L_k' H' w)[r],   e = innov - H (L_k innov),  w = innov / V.
// kHasLb: Lgain_bar is asked for.
template <bool kGuard, bool kHasLb, bool kScore>
__global__ __launch_bounds__(kWave) void k_landing_filter_vjp(BatchParams P, FilterSweepIn in, FilterVjpArgs a) {
    static_assert(!(kHasLb && kScore), "the score's cotangent is taken at fixed gains");
    constexpr int NY = QLN_TRACK_NY_MAX;
    constexpr bool kInnov = kHasLb || kScore;
    __shared__ double Hs[NY * 15];
    const int ny = in.ny;
    for (int i = threadIdx.x; i < 15 * ny; i += kWave) Hs[i] = in.H[i];
    // 1 / V beside it, read at a hidden offset (k_landing_filter): held in scalar registers over the knots the eight took sixteen
    [[maybe_unused]] __shared__ double Vs[NY];
    if constexpr (kScore) {
#pragma unroll
        for (int r = 0; r < NY; ++r)
            if ((int)threadIdx.x == r) Vs[r] = in.iv[r];
    }
    __syncthreads();
    const Row16 r16 = row16_of(P);  // lane 15 reads lane 14's slots and contributes nothing
    // A row past the batch's end leaves here, behind the barrier: every cross-lane move below stays inside a row of sixteen, so
    // the rows that remain lose no source lane, and the flag need not be held over the knots.
    if (!r16.valid) return;
    const int ln = r16.ln, j = r16.j, bc = r16.bc, kt = r16.kt, im = r16.im, N = P.N;
    const bool own = r16.own;
    constexpr bool valid = true;
    const Model M = plant_model<true>(P, in.model, bc);
    const int64_t zo = (int64_t)bc * P.z_stride, xo = (int64_t)bc * N * QLN_NX, go = xo * ny, io = (int64_t)bc * N * ny;
    const double* __restrict__ Zc = in.Zrec + zo;
    const double* __restrict__ Xh = in.Xhat + xo;
    const double* __restrict__ Lb = in.Lgain + go + (int64_t)j * ny;
    const double* __restrict__ Ib = kInnov ? in.innov + io : nullptr;
    [[maybe_unused]] int ksh = -1;
    [[maybe_unused]] double tauh = 0.0;
    if constexpr (kGuard) {
        ksh = guard_knot(in.event_hat[(int64_t)QLN_TOUCHDOWN_INFO_STRIDE * bc], N);
        tauh = in.event_hat[(int64_t)QLN_TOUCHDOWN_INFO_STRIDE * bc + 1];
    }
    // ---- lane j's constant pattern (k_tracking_rollout_estimated_vjp forms the same) ----
    const VjpLane lc = vjp_lane(j, M);
    const int p = lc.pos ? j : j - 7;
    double e[4], sg[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        e[m] = ((p <= 1 && (m == p || m == p + 2)) || (lc.foot && m == p - 3)) ? 1.0 : 0.0;
        sg[m] = 0.0;
    }
    if (p == 0) sg[1] = sg[3] = -1.0;
    if (p == 1) sg[0] = sg[2] = 1.0;
    if (p == 3) sg[1] = 1.0;
    if (p == 4) sg[0] = -1.0;
    if (p == 5) sg[3] = 1.0;
    if (p == 6) sg[2] = -1.0;

    double mbar[QLN_MODEL_NP] = {0.0, 0.0, 0.0, 0.0};  // lane j's share of model_bar
    const double zero5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    double lamm = 0.0;
    const double* __restrict__ Xhb = a.Xhat_bar ? a.Xhat_bar + xo : nullptr;
    const double* __restrict__ Ibb = a.innov_bar ? a.innov_bar + io : nullptr;
    [[maybe_unused]] const double* __restrict__ Nbb = (kScore && a.nis_bar) ? a.nis_bar + (int64_t)bc * N : nullptr;
    [[maybe_unused]] const double llb = (kScore && a.loglik_bar) ? a.loglik_bar[bc] : 0.0;
    double* __restrict__ Zrb = a.Zrec_bar ? a.Zrec_bar + zo : nullptr;
    double* __restrict__ Ybp = a.Y_bar ? a.Y_bar + io : nullptr;
    [[maybe_unused]] double* __restrict__ Lgb = kHasLb ? a.Lgain_bar + go + (int64_t)j * ny : nullptr;
    auto load = [&](FilterVjpKnot& s, int k) {
        const double* __restrict__ Lk = Lb + (int64_t)k * (15 * ny);
#pragma unroll
        for (int r = 0; r < NY; ++r) s.l[r] = r < ny ? Lk[r] : 0.0;
        if constexpr (kInnov) s.ivl = Ib[(int64_t)k * ny + min(ln, ny - 1)];
        if (Ibb) s.ibl = Ibb[(int64_t)k * ny + min(ln, ny - 1)];
        if (Xhb) s.xhb = Xhb[(int64_t)k * QLN_NX + j];
        if constexpr (kScore) s.nb = Nbb ? Nbb[k] : 0.0;
        if (k == N - 1) return;
        knot_load(Zc + 20 * k, ln, s.z0, s.z1);
        s.xh = Xh[(int64_t)k * QLN_NX + j];
    };
    FilterVjpKnot cur = {}, nxt = {};
    load(nxt, N - 1);
    for (int k = N - 1; k >= 0; --k) {
        int nyk = ny, lnk = ln;  // hidden once per knot, as in the forward sweep; the lane's place in the row with it
        asm volatile("" : "+s"(nyk));
        asm volatile("" : "+v"(lnk));
        const bool ownk = lnk < 15;
        cur = nxt;
        if (k > 0) load(nxt, k - 1);
        double xhb = (ownk && Xhb) ? cur.xhb : 0.0;
        if (k < N - 1) {
            const double u[5] = {row_bcast<15>(cur.z0), row_bcast<0>(cur.z1), row_bcast<1>(cur.z1), row_bcast<2>(cur.z1),
                                 row_bcast<3>(cur.z1)};
            KnotMode mdh;
            if constexpr (kGuard) mdh = guard_mode(k, ksh, im);
            else mdh = knot_mode(k + 1, kt - 1, im);
            double ub[5];
            // the lane's index and flags behind a hidden value, for the reason given in the forward sweep
            int jk = j;
            asm volatile("" : "+v"(jk));
            VjpLane lk = lc;
            lk.j = jk;
            lk.pos = jk < 7;
            lk.jrow = jk == 4 || jk == 6 || (jk >= 10 && jk <= 13);
            lk.cpl = jk >= 7 && jk <= 13;
            lk.kcpl = jk == 11 || jk == 13;
            const int pk = lk.pos ? jk : jk - 7;
            lk.foot = (pk == 3 || pk == 4) ? 1 : (pk == 5 || pk == 6) ? 2 : 0;
            const double axh = estimated_vjp_step<kGuard, true>(lk, e, sg, lnk, ownk, cur.xh, u[0], u[1], u[2], u[3], u[4], mdh, k == ksh,
                                                                tauh, M, lamm, a.model_bar != nullptr, mbar, zero5, ub);
            __builtin_amdgcn_sched_barrier(0);
            xhb = ownk ? xhb + axh : 0.0;
            if (valid && Zrb) knot_store(Zrb + 20 * k, r16, 0.0, ub);
        } else if (valid && Zrb && ownk) {
            Zrb[20 * k + j] = 0.0;  // the last knot has no controls
        }
        // ---- the measurement update, transposed ----
        [[maybe_unused]] double iv[NY], ibr[NY];
        if constexpr (kInnov) row_bcast_first(cur.ivl, iv, std::make_integer_sequence<int, NY>{});
        if (Ibb) row_bcast_first(cur.ibl, ibr, std::make_integer_sequence<int, NY>{});
        [[maybe_unused]] double g = 0.0, hw = 0.0, nbk = 0.0, w[NY];
        if constexpr (kScore) {
            nbk = cur.nb - 0.5 * llb;
            int vo = 0;
            asm volatile("" : "+v"(vo));
#pragma unroll
            for (int r = 0; r < NY; ++r) {
                w[r] = 0.0;
                if (r < nyk) {
                    w[r] = Vs[vo + r];
                    g = fma(cur.l[r], iv[r], g);
                    hw = fma(Hs[15 * r + j], iv[r] * w[r], hw);
                }
            }
        }
        double hib = 0.0, ibo = 0.0;
#pragma unroll
        for (int r = 0; r < NY; ++r) {
            if (r < nyk) {
                double ib = row_sum16(ownk ? cur.l[r] * xhb : 0.0);
                if (Ibb) ib = ibr[r] + ib;
                if constexpr (kScore) {
                    const double er = iv[r] - row_sum16(ownk ? Hs[15 * r + j] * g : 0.0);
                    const double lthw = row_sum16(ownk ? cur.l[r] * hw : 0.0);
                    ib = fma(nbk, fma(er, w[r], iv[r] * w[r]) - lthw, ib);
                }
                hib = fma(Hs[15 * r + j], ib, hib);
                ibo = (lnk == r) ? ib : ibo;
                if constexpr (kHasLb) {
                    if (valid && ownk) Lgb[(int64_t)k * (15 * ny) + r] = xhb * iv[r];
                }
            }
        }
        if (valid && Ybp && lnk < nyk) Ybp[(int64_t)k * ny + ln] = ibo;
        lamm = ownk ? xhb - hib : 0.0;
    }
    if (valid && own && a.xhat0_bar) a.xhat0_bar[(int64_t)bc * QLN_NX + j] = lamm;
    if (a.model_bar) {
        double out = 0.0;
#pragma unroll
        for (int q = 0; q < QLN_MODEL_NP; ++q) {
            const double sq = row_sum16(mbar[q]);
            out = (ln == q) ? sq : out;
        }
        if (valid && ln < QLN_MODEL_NP) a.model_bar[(int64_t)bc * QLN_MODEL_NP + ln] = out;
    }
}

}  // namespace

// event (the guarded roll-out's records) sends the Riccati and the covariance sweep to their kGuard instantiations, which exist
// on the kModel path only, as the roll-out's sweeps': a null model there is the handle's four values.  Without event, model is
// not read.
// sat (the limited roll-out's saturation record) sends it to the kLimit instantiations: the guarded pair with event, the
// knot-scheduled pair without.
hipError_t launch_tracking_lqr(const BatchParams& p, const double* Qd, const double* Rd, const double* Qfd, const double* Zref,
                               const double* model, const double* event, const double* sat, double* K, double* P,
                               hipStream_t stream) {
    TrackWeights w;
    for (int i = 0; i < 15; ++i) {
        w.Q[i] = Qd[i];
        w.Qf[i] = Qfd[i];
    }
    for (int i = 0; i < 4; ++i) w.R[i] = Rd[i];
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(row16_grid(p.B)), dim3(kWave), 0, stream, p, w, Zref, K, P, model, event, sat);
    };
    if (sat && event)
        P ? go(k_tracking_lqr<true, true, true, true>) : go(k_tracking_lqr<false, true, true, true>);
    else if (sat)
        P ? go(k_tracking_lqr<true, false, false, true>) : go(k_tracking_lqr<false, false, false, true>);
    else if (event)
        P ? go(k_tracking_lqr<true, true, true>) : go(k_tracking_lqr<false, true, true>);
    else
        P ? go(k_tracking_lqr<true, false, false>) : go(k_tracking_lqr<false, false, false>);
    return hipGetLastError();
}

// The roll-out and its two sweeps.  kModel is on only where something of the model is passed: the forms at the handle's model
// pass null and run the instantiation without the flag.
hipError_t launch_tracking_rollout(const BatchParams& p, const double* Zref, const double* K, const double* x0,
                                   const double* model, double* Zout, bool guarded, double* event, const double* lim,
                                   double* sat, hipStream_t stream) {
    ForceLimits fl{};
    if (lim)
        for (int i = 0; i < QLN_FORCE_LIMITS_N; ++i) fl.v[i] = lim[i];
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((p.B + kWave - 1) / kWave), dim3(kWave), 0, stream, p, Zref, K, x0, Zout, model, event, fl,
                           sat);
    };
    // lim (host, QLN_FORCE_LIMITS_N doubles): the limited roll-out, on the kModel path whether a model is given or not
    if (lim)
        guarded ? go(k_tracking_rollout<true, true, true>) : go(k_tracking_rollout<true, false, true>);
    else if (guarded)
        model ? go(k_tracking_rollout<true, true>) : go(k_tracking_rollout<false, true>);
    else
        model ? go(k_tracking_rollout<true, false>) : go(k_tracking_rollout<false, false>);
    return hipGetLastError();
}

// event (the guarded roll-out's records) sends the two sweeps to their kGuard instantiations, which exist on the kModel path
// only: a null model there is the handle's four values.  2 of the reverse sweep (K or not) and 6 of the tangent sweep (the six
// combinations of K, K_dot and Zref_dot that exist without the flag).
hipError_t launch_tracking_rollout_vjp(const BatchParams& p, const double* Zref, const double* K, const double* Zout,
                                       const double* model, const double* event, const double* sat, const double* Zbar,
                                       double* Zref_bar, double* K_bar, double* x0_bar, double* model_bar, hipStream_t stream) {
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(row16_grid(p.B)), dim3(kWave), 0, stream, p, Zref, K, Zout, Zbar, Zref_bar, K_bar, x0_bar,
                           model, model_bar, event, sat);
    };
    // sat (the limited roll-out's saturation record): the kLimit instantiations, on the kModel path
    if (sat && event)
        K ? go(k_tracking_rollout_vjp<true, true, true, true>) : go(k_tracking_rollout_vjp<false, true, true, true>);
    else if (sat)
        K ? go(k_tracking_rollout_vjp<true, true, false, true>) : go(k_tracking_rollout_vjp<false, true, false, true>);
    else if (event)
        K ? go(k_tracking_rollout_vjp<true, true, true>) : go(k_tracking_rollout_vjp<false, true, true>);
    else if (model || model_bar)
        K ? go(k_tracking_rollout_vjp<true, true, false>) : go(k_tracking_rollout_vjp<false, true, false>);
    else
        K ? go(k_tracking_rollout_vjp<true, false, false>) : go(k_tracking_rollout_vjp<false, false, false>);
    return hipGetLastError();
}

hipError_t launch_tracking_rollout_jvp(const BatchParams& p, const double* Zref, const double* K, const double* Zout,
                                       const double* model, const double* event, const double* sat, const double* Zref_dot,
                                       const double* K_dot, const double* x0_dot, const double* model_dot, double* Zout_dot,
                                       double* event_dot, hipStream_t stream) {
    if (K_dot && !K) return hipErrorInvalidValue;
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(row16_grid(p.B)), dim3(kWave), 0, stream, p, Zref, K, Zout, Zref_dot, K_dot, x0_dot,
                           Zout_dot, model, model_dot, event, event_dot, sat);
    };
    // kHasK, kHasKd, kHasZd as compile-time flags, then kModel and kGuard (and kLimit where sat is given)
    auto pick = [&](auto hasK, auto hasKd, auto hasZd) {
        if (sat && event)
            go(k_tracking_rollout_jvp<hasK(), hasKd(), hasZd(), true, true, true>);
        else if (sat)
            go(k_tracking_rollout_jvp<hasK(), hasKd(), hasZd(), true, false, true>);
        else if (event)
            go(k_tracking_rollout_jvp<hasK(), hasKd(), hasZd(), true, true>);
        else if (model || model_dot)
            go(k_tracking_rollout_jvp<hasK(), hasKd(), hasZd(), true, false>);
        else
            go(k_tracking_rollout_jvp<hasK(), hasKd(), hasZd(), false, false>);
    };
    constexpr std::true_type yes{};
    constexpr std::false_type no{};
    if (K_dot)
        Zref_dot ? pick(yes, yes, yes) : pick(yes, yes, no);
    else if (K)
        Zref_dot ? pick(yes, no, yes) : pick(yes, no, no);
    else
        Zref_dot ? pick(no, no, yes) : pick(no, no, no);
    return hipGetLastError();
}

hipError_t launch_tracking_covariance(const BatchParams& p, const double* Zout, const double* K, const double* model,
                                      const double* event, const double* Sigma0, int sigma0_batch, const double* Wd,
                                      double* Sigma, double* marg, double* event_var, hipStream_t stream) {
    if (event_var && !event) return hipErrorInvalidValue;
    CovNoise w;
    for (int i = 0; i < 15; ++i) w.w[i] = Wd ? Wd[i] : 0.0;
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(row16_grid(p.B)), dim3(kWave), 0, stream, p, w, Zout, K, Sigma0, sigma0_batch, Sigma, marg,
                           model, event, event_var);
    };
    if (event)
        K ? go(k_tracking_covariance<true, true, true>) : go(k_tracking_covariance<false, true, true>);
    else
        K ? go(k_tracking_covariance<true, false, false>) : go(k_tracking_covariance<false, false, false>);
    return hipGetLastError();
}

// The four instantiations of k_tracking_kalman: K or the filter alone, event or the knot schedule (as launch_tracking_covariance).
hipError_t launch_tracking_kalman(const BatchParams& p, const double* Zout, const double* K, const double* model,
                                  const double* event, const double* H, int ny, const double* Vd, const double* Sigma0,
                                  int sigma0_batch, const double* Wd, double* Lgain, double* Pest, double* Sigma, double* marg,
                                  double* event_var, hipStream_t stream) {
    if (event_var && !event) return hipErrorInvalidValue;
    if (!K && (Sigma || marg || event_var)) return hipErrorInvalidValue;
    if (ny < 1 || ny > QLN_TRACK_NY_MAX || !H || !Vd) return hipErrorInvalidValue;
    KalmanNoise nz;
    for (int i = 0; i < 15; ++i) nz.w[i] = Wd ? Wd[i] : 0.0;
    for (int r = 0; r < QLN_TRACK_NY_MAX; ++r) nz.v[r] = r < ny ? Vd[r] : 1.0;
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(row16_grid(p.B)), dim3(kWave), 0, stream, p, nz, Zout, K, H, ny, Sigma0, sigma0_batch, Lgain,
                           Pest, Sigma, marg, model, event, event_var);
    };
    if (event)
        K ? go(k_tracking_kalman<true, true, true>) : go(k_tracking_kalman<false, true, true>);
    else
        K ? go(k_tracking_kalman<true, false, false>) : go(k_tracking_kalman<false, false, false>);
    return hipGetLastError();
}

// The two instantiations of k_tracking_kalman_jvp: event or the knot schedule (model is read with event only, as above).
hipError_t launch_tracking_kalman_jvp(const BatchParams& p, const double* Zout, const double* model, const double* event,
                                      const double* Lgain, const double* H, int ny, const double* Vd, const double* Sigma0_dot,
                                      int sigma0_batch, const double* Wd_dot, const double* Vd_dot, double* Lgain_dot,
                                      double* Pest_dot, double* logdet_dot, hipStream_t stream) {
    if (ny < 1 || ny > QLN_TRACK_NY_MAX || !Zout || !Lgain || !H || !Vd) return hipErrorInvalidValue;
    if (!Lgain_dot && !Pest_dot && !logdet_dot) return hipErrorInvalidValue;
    KalmanNoiseDot nz;
    for (int i = 0; i < 15; ++i) nz.wd[i] = Wd_dot ? Wd_dot[i] : 0.0;
    for (int r = 0; r < QLN_TRACK_NY_MAX; ++r) {
        nz.iv[r] = r < ny ? 1.0 / Vd[r] : 1.0;
        nz.vd[r] = (r < ny && Vd_dot) ? Vd_dot[r] : 0.0;
    }
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(row16_grid(p.B)), dim3(kWave), 0, stream, p, nz, Zout, Lgain, H, ny, Sigma0_dot, sigma0_batch,
                           Lgain_dot, Pest_dot, logdet_dot, model, event);
    };
    if (event) go(k_tracking_kalman_jvp<true, true>);
    else go(k_tracking_kalman_jvp<false, false>);
    return hipGetLastError();
}

// The two instantiations of k_tracking_kalman_vjp: event or the knot schedule (model is read with event only, as above).
hipError_t launch_tracking_kalman_vjp(const BatchParams& p, const double* Zout, const double* model, const double* event,
                                      const double* Lgain, const double* H, int ny, const double* Vd, const double* Lgain_bar,
                                      const double* Pest_bar, const double* logdet_bar, double* Sigma0_bar, double* Wdiag_bar,
                                      double* Vdiag_bar, hipStream_t stream) {
    if (ny < 1 || ny > QLN_TRACK_NY_MAX || !Zout || !Lgain || !H || !Vd) return hipErrorInvalidValue;
    if (!Lgain_bar && !Pest_bar && !logdet_bar) return hipErrorInvalidValue;
    if (!Sigma0_bar && !Wdiag_bar && !Vdiag_bar) return hipErrorInvalidValue;
    SmootherNoise nz;
    for (int r = 0; r < QLN_TRACK_NY_MAX; ++r) nz.iv[r] = r < ny ? 1.0 / Vd[r] : 1.0;
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(row16_grid(p.B)), dim3(kWave), 0, stream, p, nz, Zout, Lgain, H, ny, Lgain_bar, Pest_bar,
                           logdet_bar, Sigma0_bar, Wdiag_bar, Vdiag_bar, model, event);
    };
    if (event) go(k_tracking_kalman_vjp<true, true>);
    else go(k_tracking_kalman_vjp<false, false>);
    return hipGetLastError();
}

// The two instantiations of k_landing_smoother: event or the knot schedule (model is read with event only, as above).
hipError_t launch_landing_smoother(const BatchParams& p, const double* Ztraj, const double* model, const double* event,
                                   const double* Lgain, const double* Pest, const double* H, int ny, const double* Vd,
                                   const double* Xhat, const double* innov, double* Xs, double* Ps, hipStream_t stream) {
    if (ny < 1 || ny > QLN_TRACK_NY_MAX || !H || !Vd || !Ztraj || !Lgain || !Pest || !Xhat || !innov) return hipErrorInvalidValue;
    if (!Xs && !Ps) return hipErrorInvalidValue;
    SmootherNoise nz;
    for (int r = 0; r < QLN_TRACK_NY_MAX; ++r) nz.iv[r] = r < ny ? 1.0 / Vd[r] : 1.0;
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(row16_grid(p.B)), dim3(kWave), 0, stream, p, nz, Ztraj, Lgain, Pest, H, ny, Xhat, innov, Xs,
                           Ps, model, event);
    };
    event ? go(k_landing_smoother<true>) : go(k_landing_smoother<false>);
    return hipGetLastError();
}

// The eight instantiations of k_landing_filter: the knot schedule or the guard, the score (score or loglik asked for, which
// needs Vd) or not, and the record's own model (model given) or the handle's.
hipError_t launch_landing_filter(const BatchParams& p, const double* Zref, const double* Zrec, const double* Lgain, const double* H,
                                 int ny, const double* Vd, const double* Y, const double* xhat0, const double* model, double* Xhat,
                                 double* innov, double* score, double* loglik, bool guarded, double* event_hat,
                                 hipStream_t stream) {
    if (ny < 1 || ny > QLN_TRACK_NY_MAX || !H || !Lgain || !Y || !Zref || !Zrec) return hipErrorInvalidValue;
    if (!guarded && event_hat) return hipErrorInvalidValue;
    if (!Xhat && !innov && !score && !loglik && !event_hat) return hipErrorInvalidValue;
    const bool scored = score || loglik;
    if (scored && !Vd) return hipErrorInvalidValue;
    SmootherNoise nz;
    for (int r = 0; r < QLN_TRACK_NY_MAX; ++r) nz.iv[r] = (scored && r < ny) ? 1.0 / Vd[r] : 1.0;
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((p.B + kWave - 1) / kWave), dim3(kWave), 0, stream, p, nz, H, ny, Zref, Zrec, Lgain, Y, xhat0,
                           Xhat, innov, score, loglik, event_hat, model);
    };
    if (model) {
        if (scored)
            guarded ? go(k_landing_filter<true, true, true>) : go(k_landing_filter<false, true, true>);
        else
            guarded ? go(k_landing_filter<true, false, true>) : go(k_landing_filter<false, false, true>);
    } else if (scored)
        guarded ? go(k_landing_filter<true, true>) : go(k_landing_filter<false, true>);
    else
        guarded ? go(k_landing_filter<true, false>) : go(k_landing_filter<false, false>);
    return hipGetLastError();
}

// The sweeps through the filter: six instantiations each -- the knot schedule or the guard (event_hat given), and a tangent /
// cotangent of Lgain, a score term, or neither (the first two exclude each other: the score is differentiated at fixed gains).
static bool filter_sweep_in_ok(const FilterSweepIn& in, bool want_innov) {
    return in.ny >= 1 && in.ny <= QLN_TRACK_NY_MAX && in.Zrec && in.Lgain && in.H && in.Xhat && (!want_innov || in.innov);
}

hipError_t launch_landing_filter_jvp(const BatchParams& p, const FilterSweepIn& in, const FilterJvpArgs& a, hipStream_t stream) {
    const bool score = a.nis_dot || a.loglik_dot;
    if (!filter_sweep_in_ok(in, a.Lgain_dot || score) || (a.Lgain_dot && score)) return hipErrorInvalidValue;
    if (!a.Y_dot && !a.Zrec_dot && !a.Lgain_dot && !a.xhat0_dot && !a.model_dot) return hipErrorInvalidValue;
    if (!a.Xhat_dot && !a.innov_dot && !score && !a.event_hat_dot) return hipErrorInvalidValue;
    if (!in.event_hat && a.event_hat_dot) return hipErrorInvalidValue;
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(row16_grid(p.B)), dim3(kWave), 0, stream, p, in, a); };
    auto pick = [&](auto guard) {
        if (a.Lgain_dot) go(k_landing_filter_jvp<guard(), true, false>);
        else if (score) go(k_landing_filter_jvp<guard(), false, true>);
        else go(k_landing_filter_jvp<guard(), false, false>);
    };
    in.event_hat ? pick(std::true_type{}) : pick(std::false_type{});
    return hipGetLastError();
}

hipError_t launch_landing_filter_vjp(const BatchParams& p, const FilterSweepIn& in, const FilterVjpArgs& a, hipStream_t stream) {
    const bool score = a.nis_bar || a.loglik_bar;
    if (!filter_sweep_in_ok(in, a.Lgain_bar || score) || (a.Lgain_bar && score)) return hipErrorInvalidValue;
    if (!a.Xhat_bar && !a.innov_bar && !score) return hipErrorInvalidValue;
    if (!a.Y_bar && !a.Zrec_bar && !a.Lgain_bar && !a.xhat0_bar && !a.model_bar) return hipErrorInvalidValue;
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(row16_grid(p.B)), dim3(kWave), 0, stream, p, in, a); };
    auto pick = [&](auto guard) {
        if (a.Lgain_bar) go(k_landing_filter_vjp<guard(), true, false>);
        else if (score) go(k_landing_filter_vjp<guard(), false, true>);
        else go(k_landing_filter_vjp<guard(), false, false>);
    };
    in.event_hat ? pick(std::true_type{}) : pick(std::false_type{});
    return hipGetLastError();
}

// The four instantiations of k_tracking_rollout_estimated: the knot schedule or the guard, and lim (host, QLN_FORCE_LIMITS_N
// doubles; null: none) sends it to the kLimit pair, which writes sat (null: not written).
hipError_t launch_tracking_rollout_estimated(const BatchParams& p, const double* Zref, const double* K, const double* Lgain,
                                             const double* H, int ny, const double* vnoise, const double* wnoise,
                                             const double* x0, const double* xhat0, const double* model, double* Zout,
                                             double* Xhat, double* innov, bool guarded, double* event, double* event_hat,
                                             const double* lim, double* sat, hipStream_t stream) {
    if (ny < 1 || ny > QLN_TRACK_NY_MAX || !H || !Lgain) return hipErrorInvalidValue;
    if (!guarded && (event || event_hat)) return hipErrorInvalidValue;
    if (sat && !lim) return hipErrorInvalidValue;
    ForceLimits fl{};
    if (lim)
        for (int i = 0; i < QLN_FORCE_LIMITS_N; ++i) fl.v[i] = lim[i];
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((p.B + kWave - 1) / kWave), dim3(kWave), 0, stream, p, H, ny, Zref, K, Lgain, vnoise,
                           wnoise, x0, xhat0, model, Zout, Xhat, innov, event, event_hat, fl, sat);
    };
    if (lim)
        guarded ? go(k_tracking_rollout_estimated<true, true>) : go(k_tracking_rollout_estimated<false, true>);
    else
        guarded ? go(k_tracking_rollout_estimated<true>) : go(k_tracking_rollout_estimated<false>);
    return hipGetLastError();
}

// The sweeps through it: eight instantiations each -- the knot schedule or the guard (both event records given), K or not,
// and a tangent / cotangent of Lgain or not; every other optional argument is a run-time one.  sat (the limited roll-out's
// saturation record; null: none) sends them to the eight kLimit instantiations.  It is the kernels' last argument, behind the
// two structs, so that the instantiations without the flag read their arguments where they always did.
static bool estimated_sweep_in_ok(const EstimatedSweepIn& in) {
    return in.ny >= 1 && in.ny <= QLN_TRACK_NY_MAX && in.Zref && in.Lgain && in.H && in.Zout && in.Xhat &&
           (in.event != nullptr) == (in.event_hat != nullptr);
}

hipError_t launch_tracking_rollout_estimated_jvp(const BatchParams& p, const EstimatedSweepIn& in, const EstimatedJvpArgs& a,
                                                 const double* sat, hipStream_t stream) {
    if (!estimated_sweep_in_ok(in) || !a.Zout_dot) return hipErrorInvalidValue;
    if ((a.K_dot && !in.K) || (a.Lgain_dot && !in.innov)) return hipErrorInvalidValue;
    if (!in.event && (a.event_dot || a.event_hat_dot)) return hipErrorInvalidValue;
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(row16_grid(p.B)), dim3(kWave), 0, stream, p, in, a, sat); };
    auto pick = [&](auto guard, auto hasK) {
        if (sat)
            a.Lgain_dot ? go(k_tracking_rollout_estimated_jvp<guard(), hasK(), true, true>)
                        : go(k_tracking_rollout_estimated_jvp<guard(), hasK(), false, true>);
        else
            a.Lgain_dot ? go(k_tracking_rollout_estimated_jvp<guard(), hasK(), true>)
                        : go(k_tracking_rollout_estimated_jvp<guard(), hasK(), false>);
    };
    constexpr std::true_type yes{};
    constexpr std::false_type no{};
    if (in.event)
        in.K ? pick(yes, yes) : pick(yes, no);
    else
        in.K ? pick(no, yes) : pick(no, no);
    return hipGetLastError();
}

hipError_t launch_tracking_rollout_estimated_vjp(const BatchParams& p, const EstimatedSweepIn& in, const EstimatedVjpArgs& a,
                                                 const double* sat, hipStream_t stream) {
    if (!estimated_sweep_in_ok(in) || !a.Zbar) return hipErrorInvalidValue;
    if ((a.K_bar && !in.K) || (a.Lgain_bar && !in.innov)) return hipErrorInvalidValue;
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(row16_grid(p.B)), dim3(kWave), 0, stream, p, in, a, sat); };
    auto pick = [&](auto guard, auto hasK) {
        if (sat)
            a.Lgain_bar ? go(k_tracking_rollout_estimated_vjp<guard(), hasK(), true, true>)
                        : go(k_tracking_rollout_estimated_vjp<guard(), hasK(), false, true>);
        else
            a.Lgain_bar ? go(k_tracking_rollout_estimated_vjp<guard(), hasK(), true>)
                        : go(k_tracking_rollout_estimated_vjp<guard(), hasK(), false>);
    };
    constexpr std::true_type yes{};
    constexpr std::false_type no{};
    if (in.event)
        in.K ? pick(yes, yes) : pick(yes, no);
    else
        in.K ? pick(no, yes) : pick(no, no);
    return hipGetLastError();
}

}  // namespace qln
