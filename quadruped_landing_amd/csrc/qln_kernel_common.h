// qln_kernel_common.h -- device code shared by the gfx950 kernel files.  Internal.
//   * wave / dispatch helpers (xcd_contiguous_index, wave_lds_sync, wave_sum, wave_max);
//   * the value path: dynamics, rk4_step, step_mode / step_forward (one knot of a roll-out), literal restatements of the reference
//     that round like it;
//   * clearance_dtheta, the one derivative entry of the clearance rows (the J v / J' lam products and the covariance
//     sweep's clearance marginal read it);
//   * the 15 x 20 step Jacobian in closed form, the one statement of it that the evaluator (qln_kernels.hip), J v / J' lam
//     and the Gauss-Newton step (qln_solver_kernels.hip), the iLQR solve (qln_ilqr_kernels.hip) and the TVLQR sweep
//     (qln_tracking_kernels.hip) share: StepBlock + step_block() form a knot's base quantities from explicit arguments
//     (states, forces, h, KnotMode, Model), for_each_step_entry() visits the 85 entries of the union pattern with row and
//     col as compile-time constants, for_each_rollout_entry() the same with the roll-out's clock row.  A static_assert
//     holds the visit order to step_union_pos();
//   * the 15 x 4 derivative of a roll-out's knot with respect to the model (g, mb, mf, lb), in closed form from the same
//     base quantities: ModelBlock + model_block() and for_each_model_entry() over its 24 entries (the roll-out's tangent
//     and reverse sweeps with a per-problem plant, qln_tracking_kernels.hip).
// The functions here are compiled under the floating-point contraction mode in force where this header is INCLUDED.
// qln_solver_kernels.hip sets contract(fast) above the include so that its step blocks fuse; the same then holds for
// EVERYTHING in this header in that file: a value-path helper (rk4_step, step_forward) called from there would fuse too
// and no longer round like the reference.  None is called there today.
#pragma once

#include "qln_device.h"

#include <type_traits>

namespace qln {
namespace {

constexpr int kWave = 64;
constexpr int kBlk = 300;  // 15 x 20 doubles per step block

// Workgroups are observed to be dealt round-robin over the 8 XCDs (blocks b and b+8 share one;
// MI355X_MICROARCH.md "Workgroup dispatch").  Giving each XCD a CONTIGUOUS range of problems makes
// every XCD's L2/TLB see one sequential write front instead of every 8th 100-KB region: a pure
// fill of the evaluator's store shape goes from ~5.8 to ~6.8 TB/s with this map alone
// (profiles/r01_store_ceiling.txt).  Placement is a speed matter only: any dispatch order computes
// the same results.
__device__ __forceinline__ int xcd_contiguous_index(int block, int n) {
    const int per_xcd = (n + 7) >> 3;
    return (block & 7) * per_xcd + (block >> 3);  // may be >= n for the last blocks: caller checks
}
__host__ inline unsigned xcd_grid(int n) { return 8u * (unsigned)((n + 7) / 8); }

// Every workgroup of the hot kernel is ONE wavefront, so cross-lane hand-offs through LDS need no
// s_barrier: the LDS executes a wave's DS instructions in issue order.  What is needed is that the
// compiler keeps that order; a wavefront-scope fence plus the (instruction-less) wave barrier do
// that.  Unlike __syncthreads() this does not drain vmcnt, so the global store stream of one
// sub-tile keeps flowing while the next one is assembled.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// sum over the wave's 64 lanes, the same bits in every lane
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}
// max over the wave's 64 lanes, the same bits in every lane (fmax: a NaN loses)
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, kWave));
    return v;
}

// ---------------------------------------------------------------------------------------------
// Value path (shared by the evaluator and by the solver's rollout, which must round identically): literal restatement of contact{1,2,3}_dynamics (src/planar_quadruped.jl:36-185).
// f1free/f2free select the mode: mode 1 = foot 2 free, mode 2 = foot 1 free, mode 3 = none.
// ---------------------------------------------------------------------------------------------
struct StepConst {
    double abx, aby;    // body acceleration
    double a1x, a1y;    // foot 1 acceleration (0 if pinned)
    double a2x, a2y;    // foot 2 acceleration (0 if pinned)
};

__device__ __forceinline__ void dynamics(const double (&s)[14], const double (&u)[5], const StepConst& k, bool f1free,
                                         bool f2free, double Ib, double (&f)[14]) {
    const double F1x = u[0], F1y = u[1], F2x = u[2], F2y = u[3];
    // tauF = -F1x*(p1[2]-pb[2]) + F1y*(p1[1]-pb[1]) - F2x*(p2[2]-pb[2]) + F2y*(p2[1]-pb[1])
    const double tauF = -F1x * (s[4] - s[1]) + F1y * (s[3] - s[0]) - F2x * (s[6] - s[1]) + F2y * (s[5] - s[0]);
    f[0] = s[7];
    f[1] = s[8];
    f[2] = s[9];
    f[3] = f1free ? s[10] : 0.0;
    f[4] = f1free ? s[11] : 0.0;
    f[5] = f2free ? s[12] : 0.0;
    f[6] = f2free ? s[13] : 0.0;
    f[7] = k.abx;
    f[8] = k.aby;
    f[9] = tauF / Ib;
    f[10] = k.a1x;
    f[11] = k.a1y;
    f[12] = k.a2x;
    f[13] = k.a2y;
}

// contact*_dynamics_rk4 (src/planar_quadruped.jl:189-221) over a step of length h, which need not be u[4]: the guarded
// roll-out splits a knot's step at the touchdown and holds the forces over both parts
__device__ __forceinline__ void rk4_step(const double (&x)[15], const double (&u)[5], double h, const StepConst& k, bool f1free,
                                         bool f2free, double Ib, double (&xn)[15]) {
    const double hh = 0.5 * h;
    double s0[14], s[14], f1[14], f2[14], f3[14], f4[14];
#pragma unroll
    for (int i = 0; i < 14; ++i) s0[i] = x[i];
    dynamics(s0, u, k, f1free, f2free, Ib, f1);
#pragma unroll
    for (int i = 0; i < 14; ++i) s[i] = s0[i] + hh * f1[i];
    dynamics(s, u, k, f1free, f2free, Ib, f2);
#pragma unroll
    for (int i = 0; i < 14; ++i) s[i] = s0[i] + hh * f2[i];
    dynamics(s, u, k, f1free, f2free, Ib, f3);
#pragma unroll
    for (int i = 0; i < 14; ++i) s[i] = s0[i] + h * f3[i];
    dynamics(s, u, k, f1free, f2free, Ib, f4);
    const double h6 = h / 6.0;
#pragma unroll
    for (int i = 0; i < 14; ++i) xn[i] = s0[i] + h6 * (((f1[i] + 2 * f2[i]) + 2 * f3[i]) + f4[i]);
    xn[14] = x[14] + h;
}
__device__ __forceinline__ void rk4_step(const double (&x)[15], const double (&u)[5], const StepConst& k, bool f1free,
                                         bool f2free, double Ib, double (&xn)[15]) {
    rk4_step(x, u, u[4], k, f1free, f2free, Ib, xn);
}

// the jump map of a touchdown (src/constraints.jl:19-38): both feet on the ground and at rest; the clock is kept
__device__ __forceinline__ void jump_map(double (&xn)[15]) {
    xn[4] = 0.0;
    xn[6] = 0.0;
    xn[10] = xn[11] = xn[12] = xn[13] = 0.0;
}

// The RK4 step of length h in the contact mode md with the forces u[0..3] held, then md's jump map: step_forward's body with
// the mode and the step length as arguments (the guarded roll-out takes the parts of a touchdown step with it).
__device__ __forceinline__ void step_mode(const Model& M, const KnotMode md, double h, const double (&x)[15],
                                          const double (&u)[5], double (&xn)[15]) {
    StepConst sc;
    sc.abx = (u[0] + u[2]) / M.mb;
    sc.aby = (u[1] + u[3]) / M.mb + M.g;
    sc.a1x = md.f1free ? (-u[0] / M.mf) : 0.0;
    sc.a1y = md.f1free ? (-u[1] / M.mf + M.g) : 0.0;
    sc.a2x = md.f2free ? (-u[2] / M.mf) : 0.0;
    sc.a2y = md.f2free ? (-u[3] / M.mf + M.g) : 0.0;
    rk4_step(x, u, h, sc, md.f1free, md.f2free, M.Ib, xn);
    if (md.jump) jump_map(xn);
}

// one dynamics knot of a roll-out (qln_solve's and qln_tracking_rollout's): the evaluator's RK4 step + jump map (src/constraints.jl:19-38)
__device__ __forceinline__ void step_forward(const Model& M, int k, int kt, int im, const double (&x)[15], const double (&u)[5],
                                             double (&xn)[15]) {
    step_mode(M, knot_mode(k + 1, kt - 1, im), u[4], x, u, xn);
}

// d(clearance_k)/d(theta_k), src/constraints.jl:269-273 (theta == 0 takes the + branch, quirk Q3)
__device__ __forceinline__ double clearance_dtheta(double th, double lb) {
    const double cth = cos(th);
    return (th > 0) ? (-lb / 2 * cth) : (lb / 2 * cth);
}

// ---------------------------------------------------------------------------------------------
// The 15 x 20 step Jacobian in closed form (derivation in qln_kernels.hip's header): the one statement every kernel
// family forms its blocks from.  step_block() computes the base quantities of a knot, for_each_step_entry() hands out
// the 85 entries of the union pattern built from them.
// ---------------------------------------------------------------------------------------------
// What the 85 entries read.  Column 19 (hc[]), the eight force-column entries of the theta/omega rows and a dozen
// scalars are values; the 30 (weight x force) products of the theta/omega rows are formed where an entry is used,
// from wAt / wBt / wAw (one multiply each).  Those three are the h-weights At, Bt, Aw; they are members like the rest,
// and not const, because the evaluator's dense tile loop passes them through an empty asm to keep the products inside
// the loop.
struct StepBlock {
    double F1x, F1y, F2x, F2y, h;
    double keep;  // 0 at the jump knot (quirk Q1), else 1
    double sFx, sFy, mF1x, mF1y, mF2x, mF2y;
    double hmb, h2mb;
    double t15, t16, t17, t18, o15, o16, o17, o18;
    double s_m1h, s_m1h2, s_k1h, s_k1h2, s_m2h, s_m2h2, s_k2h, s_k2h2, s_k1f, s_k2f;
    double hc[15];
    double wAt, wBt, wAw;
};

// x: the knot's state without the clock; F1x .. F2y, h: its control
__device__ __forceinline__ StepBlock step_block(const double (&x)[14], double F1x, double F1y, double F2x, double F2y, double h,
                                                KnotMode md, const Model& M) {
    const double g = M.g, mb = M.mb, mf = M.mf, Ib = M.Ib;
    const double m1 = md.f1free ? 1.0 : 0.0, m2 = md.f2free ? 1.0 : 0.0;
    const double keep = md.jump ? 0.0 : 1.0;
    const double km1 = keep * m1, km2 = keep * m2;
    const double abx = (F1x + F2x) / mb, aby = (F1y + F2y) / mb + g;
    const double a1x = m1 * (-F1x / mf), a1y = m1 * (-F1y / mf + g);
    const double a2x = m2 * (-F2x / mf), a2y = m2 * (-F2y / mf + g);
    const double h2 = h * h, h3 = h2 * h, h4 = h2 * h2;
    const double iIb = 1.0 / Ib;
    const double Aw = h * iIb;
    const double At = 0.5 * h2 * iIb;
    const double Bt = h3 * iIb * (1.0 / 6.0);
    const double Ct = h4 * iIb * (1.0 / 24.0);
    const double sFx = F1x + F2x, sFy = F1y + F2y;
    const double r1x = x[3] - x[0], r1y = x[4] - x[1], r2x = x[5] - x[0], r2y = x[6] - x[1];
    const double w1x = m1 * x[10] - x[7], w1y = m1 * x[11] - x[8];
    const double w2x = m2 * x[12] - x[7], w2y = m2 * x[13] - x[8];
    const double tau0 = r1x * F1y - r1y * F1x + r2x * F2y - r2y * F2x;
    const double tauv = w1x * F1y - w1y * F1x + w2x * F2y - w2y * F2x;
    const double ga1 = g * (1.0 - m1), ga2 = g * (1.0 - m2);
    const double taua = ga1 * F1x + ga2 * F2x;
    const double hmb = h / mb, h2mb = 0.5 * h2 / mb, hmf = h / mf, h2mf = 0.5 * h2 / mf;
    StepBlock b;
    b.F1x = F1x, b.F1y = F1y, b.F2x = F2x, b.F2y = F2y, b.h = h;
    b.keep = keep;
    b.sFx = sFx, b.sFy = sFy;
    b.hmb = hmb, b.h2mb = h2mb;
    b.hc[0] = x[7] + h * abx;
    b.hc[1] = x[8] + h * aby;
    b.hc[2] = x[9] + (Aw * tau0 + At * tauv + Bt * taua);
    b.hc[3] = m1 * (x[10] + h * a1x);
    b.hc[4] = km1 * (x[11] + h * a1y);
    b.hc[5] = m2 * (x[12] + h * a2x);
    b.hc[6] = km2 * (x[13] + h * a2y);
    b.hc[7] = abx;
    b.hc[8] = aby;
    b.hc[9] = iIb * (tau0 + h * tauv + 0.5 * h2 * taua);
    b.hc[10] = keep * a1x;
    b.hc[11] = keep * a1y;
    b.hc[12] = keep * a2x;
    b.hc[13] = keep * a2y;
    b.hc[14] = keep;
    b.t15 = -At * r1y - Bt * w1y + Ct * ga1, b.t16 = At * r1x + Bt * w1x;
    b.t17 = -At * r2y - Bt * w2y + Ct * ga2, b.t18 = At * r2x + Bt * w2x;
    b.o15 = -Aw * r1y - At * w1y + Bt * ga1, b.o16 = Aw * r1x + At * w1x;
    b.o17 = -Aw * r2y - At * w2y + Bt * ga2, b.o18 = Aw * r2x + At * w2x;
    b.mF1x = m1 * F1x, b.mF1y = m1 * F1y, b.mF2x = m2 * F2x, b.mF2y = m2 * F2y;
    b.s_m1h = m1 * h, b.s_m1h2 = -m1 * h2mf, b.s_k1h = km1 * h, b.s_k1h2 = -km1 * h2mf;
    b.s_m2h = m2 * h, b.s_m2h2 = -m2 * h2mf, b.s_k2h = km2 * h, b.s_k2h2 = -km2 * h2mf;
    b.s_k1f = -km1 * hmf, b.s_k2f = -km2 * hmf;
    b.wAt = At, b.wBt = Bt, b.wAw = Aw;
    return b;
}
// the knot as it lies in Z: x_k at zk[0..14], u_k = (F1x, F1y, F2x, F2y, h) behind it
__device__ __forceinline__ StepBlock step_block(const double* zk, KnotMode md, const Model& M) {
    double x[14];
#pragma unroll
    for (int i = 0; i < 14; ++i) x[i] = zk[i];
    return step_block(x, zk[15], zk[16], zk[17], zk[18], zk[19], md, M);
}

// The one list of the 85 entries of the union pattern, E(row, col, value) over a StepBlock b: column 19 (d/dh,
// dense), row 2 (theta) and row 9 (omega), rows 0-1 (body position), rows 3-6 (foot positions; the y rows are masked
// at the jump), rows 7-8 (body velocity), rows 10-13 (foot velocities) and row 14 (clock), masked at the jump (quirk
// Q1).  In column-major order of (row, col) -- the order of the values inside a block in both formats; the structural
// format's emission and step_union_pos() rely on it, and the static_assert below holds the list to it.  Private to
// this header: the two visitors below are the interface.
#define QLN_STEP_ENTRY_LIST(E)                                                                                    \
    /* columns 0-6: positions */                                                                                  \
    E(0, 0, 1.0) E(2, 0, -b.wAt * b.sFy) E(9, 0, -b.wAw * b.sFy)                                                  \
    E(1, 1, 1.0) E(2, 1, b.wAt * b.sFx) E(9, 1, b.wAw * b.sFx)                                                    \
    E(2, 2, 1.0)                                                                                                  \
    E(2, 3, b.wAt * b.F1y) E(3, 3, 1.0) E(9, 3, b.wAw * b.F1y)                                                    \
    E(2, 4, -b.wAt * b.F1x) E(4, 4, b.keep) E(9, 4, -b.wAw * b.F1x)                                               \
    E(2, 5, b.wAt * b.F2y) E(5, 5, 1.0) E(9, 5, b.wAw * b.F2y)                                                    \
    E(2, 6, -b.wAt * b.F2x) E(6, 6, b.keep) E(9, 6, -b.wAw * b.F2x)                                               \
    /* columns 7-14: velocities and the clock */                                                                  \
    E(0, 7, b.h) E(2, 7, -b.wBt * b.sFy) E(7, 7, 1.0) E(9, 7, -b.wAt * b.sFy)                                     \
    E(1, 8, b.h) E(2, 8, b.wBt * b.sFx) E(8, 8, 1.0) E(9, 8, b.wAt * b.sFx)                                       \
    E(2, 9, b.h) E(9, 9, 1.0)                                                                                     \
    E(2, 10, b.wBt * b.mF1y) E(3, 10, b.s_m1h) E(9, 10, b.wAt * b.mF1y) E(10, 10, b.keep)                         \
    E(2, 11, -b.wBt * b.mF1x) E(4, 11, b.s_k1h) E(9, 11, -b.wAt * b.mF1x) E(11, 11, b.keep)                       \
    E(2, 12, b.wBt * b.mF2y) E(5, 12, b.s_m2h) E(9, 12, b.wAt * b.mF2y) E(12, 12, b.keep)                         \
    E(2, 13, -b.wBt * b.mF2x) E(6, 13, b.s_k2h) E(9, 13, -b.wAt * b.mF2x) E(13, 13, b.keep)                       \
    E(14, 14, b.keep)                                                                                             \
    /* columns 15-18: forces */                                                                                   \
    E(0, 15, b.h2mb) E(2, 15, b.t15) E(3, 15, b.s_m1h2) E(7, 15, b.hmb) E(9, 15, b.o15) E(10, 15, b.s_k1f)        \
    E(1, 16, b.h2mb) E(2, 16, b.t16) E(4, 16, b.s_k1h2) E(8, 16, b.hmb) E(9, 16, b.o16) E(11, 16, b.s_k1f)        \
    E(0, 17, b.h2mb) E(2, 17, b.t17) E(5, 17, b.s_m2h2) E(7, 17, b.hmb) E(9, 17, b.o17) E(12, 17, b.s_k2f)        \
    E(1, 18, b.h2mb) E(2, 18, b.t18) E(6, 18, b.s_k2h2) E(8, 18, b.hmb) E(9, 18, b.o18) E(13, 18, b.s_k2f)        \
    /* column 19: the step length h */                                                                            \
    E(0, 19, b.hc[0]) E(1, 19, b.hc[1]) E(2, 19, b.hc[2]) E(3, 19, b.hc[3]) E(4, 19, b.hc[4])                     \
    E(5, 19, b.hc[5]) E(6, 19, b.hc[6]) E(7, 19, b.hc[7]) E(8, 19, b.hc[8]) E(9, 19, b.hc[9])                     \
    E(10, 19, b.hc[10]) E(11, 19, b.hc[11]) E(12, 19, b.hc[12]) E(13, 19, b.hc[13]) E(14, 19, b.hc[14])

template <int I>
using Idx = std::integral_constant<int, I>;  // row and col reach a visitor as constants: usable in if constexpr

// f(row, col, value) for the 85 entries of b, in column-major order
template <typename F>
__device__ __forceinline__ void for_each_step_entry(const StepBlock& b, F&& f) {
#define QLN_E(row, col, val) [[clang::always_inline]] f(Idx<row>{}, Idx<col>{}, (val));
    QLN_STEP_ENTRY_LIST(QLN_E)
#undef QLN_E
}
// The block of a ROLL-OUT's knot (the TVLQR sweep, the covariance and tangent sweeps of qln_tracking_kernels.hip): the
// same entries with row 14 replaced by 1.0.  Row 14 is the clock, t+ = t + h: 1 at x[14] and at h.  The evaluator's
// block carries the reference's jump mask there, which zeroes the row at the jump knot (quirk Q1: keep = 0); the
// roll-out's step_forward applies the jump map itself, which keeps the clock, so the derivative of what the roll-out
// computes has the 1 at every knot.  Nothing else differs between the two blocks.
template <typename F>
__device__ __forceinline__ void for_each_rollout_entry(const StepBlock& b, F&& f) {
#define QLN_E(row, col, val) [[clang::always_inline]] f(Idx<row>{}, Idx<col>{}, (row == 14) ? 1.0 : (val));
    QLN_STEP_ENTRY_LIST(QLN_E)
#undef QLN_E
}
// f(row, col) for the same entries in the same order, for whoever holds the values elsewhere (or wants none)
template <typename F>
__host__ __device__ __forceinline__ constexpr void for_each_step_entry(F&& f) {
#define QLN_E(row, col, val) [[clang::always_inline]] f(Idx<row>{}, Idx<col>{});
    QLN_STEP_ENTRY_LIST(QLN_E)
#undef QLN_E
}
#undef QLN_STEP_ENTRY_LIST

constexpr bool step_entries_in_union_order() {
    int n = 0;
    bool ok = true;
    for_each_step_entry([&](auto row, auto col) {
        ok = ok && step_union_present(row, col) && step_union_pos(row, col) == n;
        ++n;
    });
    return ok && n == kStepUnion;
}
static_assert(step_entries_in_union_order(), "the entries are visited at positions 0 .. 84 of step_union_pos, each once");

// ---------------------------------------------------------------------------------------------
// G = d x+ / d theta, theta = (g, mb, mf, lb) (QLN_MODEL_NP): the 15 x 4 derivative of a roll-out's knot -- RK4 step and jump
// map -- with respect to the model its dynamics read, in closed form from the base quantities of step_block() above.  The
// step is polynomial in h: body and feet move under the constant accelerations ab = sF / mb + g e_y and a_i = m_i (-F_i / mf
// + g e_y), and only theta and omega see the state, through tau / Ib with tau(t) = tau0 + t tauv + t^2/2 taua:
//   theta+ = theta + h omega + dth,  dth = At tau0 + Bt tauv + Ct taua,     omega+ = omega + dom,  dom = Aw tau0 + At tauv + Bt taua.
// Which entries can be non-zero, from that derivation (24 of the 60):
//   column g:  the y rows -- 1, 8 (body), 4, 11 and 6, 13 (a free foot; zero at the jump) -- and rows 2, 9 through taua = g dga;
//   column mb: rows 0, 1, 7, 8 through ab, and rows 2, 9 through Ib alone (d (1/Ib) / d mb = -1 / (Ib mb));
//   column mf: the rows of a free foot, 3 .. 6 and 10 .. 13 (4, 6, 10 .. 13 zero at the jump);
//   column lb: rows 2, 9 through Ib alone (d (1/Ib) / d lb = -2 / (Ib lb)).
// mf does not reach theta / omega, and mb reaches them through Ib only: the accelerations enter tau as
// sum_i (a_i - ab) x F_i, where F_i x F_i / mf and sF x sF / mb vanish identically.  A numerical derivative of the RK4 stages
// leaves rounding (~1e-17) in those four places; the pattern here is the algebraic one.  Row 14, the clock, reads no model.
// ---------------------------------------------------------------------------------------------
struct ModelBlock {
    double h, h2h;                              // h and h^2/2: column g of the body's y rows
    double k1, k2;                              // keep * m1, keep * m2: the y rows and velocities of a free foot
    double g2, g9;                              // column g of theta, omega: Ct dga, Bt dga
    double b0, b1, b7, b8;                      // column mb of the body rows
    double dth, dom, nimb, nilb2;               // rows 2, 9 of columns mb and lb: dth, dom times -1/mb and -2/lb
    double f3, f4, f5, f6, f10, f11, f12, f13;  // column mf
};

// the arguments of step_block(): the block is G at the same knot
__device__ __forceinline__ ModelBlock model_block(const double (&x)[14], double F1x, double F1y, double F2x, double F2y, double h,
                                                  KnotMode md, const Model& M) {
    const double g = M.g, mb = M.mb, mf = M.mf, Ib = M.Ib;
    const double m1 = md.f1free ? 1.0 : 0.0, m2 = md.f2free ? 1.0 : 0.0;
    const double keep = md.jump ? 0.0 : 1.0;
    const double km1 = keep * m1, km2 = keep * m2;
    const double h2 = h * h, h3 = h2 * h, h4 = h2 * h2;
    const double iIb = 1.0 / Ib;
    const double Aw = h * iIb;
    const double At = 0.5 * h2 * iIb;
    const double Bt = h3 * iIb * (1.0 / 6.0);
    const double Ct = h4 * iIb * (1.0 / 24.0);
    const double sFx = F1x + F2x, sFy = F1y + F2y;
    const double r1x = x[3] - x[0], r1y = x[4] - x[1], r2x = x[5] - x[0], r2y = x[6] - x[1];
    const double w1x = m1 * x[10] - x[7], w1y = m1 * x[11] - x[8];
    const double w2x = m2 * x[12] - x[7], w2y = m2 * x[13] - x[8];
    const double tau0 = r1x * F1y - r1y * F1x + r2x * F2y - r2y * F2x;
    const double tauv = w1x * F1y - w1y * F1x + w2x * F2y - w2y * F2x;
    const double dga = (1.0 - m1) * F1x + (1.0 - m2) * F2x;  // d taua / d g
    const double taua = g * dga;
    const double h2h = 0.5 * h2;
    const double imb = 1.0 / mb, imb2 = imb * imb, imf2 = 1.0 / (mf * mf);
    const double ph = h2h * imf2, vh = h * imf2;  // d (h^2/2 a_i) / d mf and d (h a_i) / d mf per unit of F_i
    ModelBlock b;
    b.h = h, b.h2h = h2h;
    b.k1 = km1, b.k2 = km2;
    b.g2 = Ct * dga, b.g9 = Bt * dga;
    b.b0 = -(h2h * imb2) * sFx, b.b1 = -(h2h * imb2) * sFy, b.b7 = -(h * imb2) * sFx, b.b8 = -(h * imb2) * sFy;
    b.dth = At * tau0 + Bt * tauv + Ct * taua;
    b.dom = Aw * tau0 + At * tauv + Bt * taua;
    b.nimb = -imb, b.nilb2 = -2.0 / M.lb;
    b.f3 = m1 * ph * F1x, b.f4 = km1 * ph * F1y, b.f5 = m2 * ph * F2x, b.f6 = km2 * ph * F2y;
    b.f10 = km1 * vh * F1x, b.f11 = km1 * vh * F1y, b.f12 = km2 * vh * F2x, b.f13 = km2 * vh * F2y;
    return b;
}

// The one list of G's 24 entries, E(row, param, value) over a ModelBlock b, column-major like the step block's.
#define QLN_MODEL_ENTRY_LIST(E)                                                                                    \
    /* g */                                                                                                        \
    E(1, 0, b.h2h) E(2, 0, b.g2) E(4, 0, b.k1 * b.h2h) E(6, 0, b.k2 * b.h2h)                                       \
    E(8, 0, b.h) E(9, 0, b.g9) E(11, 0, b.k1 * b.h) E(13, 0, b.k2 * b.h)                                           \
    /* mb */                                                                                                       \
    E(0, 1, b.b0) E(1, 1, b.b1) E(2, 1, b.dth * b.nimb) E(7, 1, b.b7) E(8, 1, b.b8) E(9, 1, b.dom * b.nimb)        \
    /* mf */                                                                                                       \
    E(3, 2, b.f3) E(4, 2, b.f4) E(5, 2, b.f5) E(6, 2, b.f6) E(10, 2, b.f10) E(11, 2, b.f11) E(12, 2, b.f12)        \
    E(13, 2, b.f13)                                                                                                \
    /* lb */                                                                                                       \
    E(2, 3, b.dth * b.nilb2) E(9, 3, b.dom * b.nilb2)

constexpr int kModelNnz = 24;
// f(row, param, value) for the 24 entries of b, row and param as compile-time constants
template <typename F>
__device__ __forceinline__ void for_each_model_entry(const ModelBlock& b, F&& f) {
#define QLN_E(row, col, val) [[clang::always_inline]] f(Idx<row>{}, Idx<col>{}, (val));
    QLN_MODEL_ENTRY_LIST(QLN_E)
#undef QLN_E
}
// f(row, param) for the same entries in the same order
template <typename F>
__host__ __device__ __forceinline__ constexpr void for_each_model_entry(F&& f) {
#define QLN_E(row, col, val) [[clang::always_inline]] f(Idx<row>{}, Idx<col>{});
    QLN_MODEL_ENTRY_LIST(QLN_E)
#undef QLN_E
}
#undef QLN_MODEL_ENTRY_LIST

// The pattern the derivation gives, stated a second time as a rule, and the list held to it: every entry once, in
// column-major order, none in the clock's row.
__host__ __device__ constexpr bool model_entry_present(int row, int p) {
    const bool tw = row == 2 || row == 9;
    switch (p) {
        case 0: return tw || row == 1 || row == 8 || row == 4 || row == 11 || row == 6 || row == 13;
        case 1: return tw || row == 0 || row == 1 || row == 7 || row == 8;
        case 2: return (row >= 3 && row <= 6) || (row >= 10 && row <= 13);
        case 3: return tw;
        default: return false;
    }
}
constexpr bool model_entries_in_order() {
    int n = 0, last = -1;
    bool ok = true;
    for_each_model_entry([&](auto row, auto p) {
        const int at = 15 * p + row;
        ok = ok && model_entry_present(row, p) && at > last && p < QLN_MODEL_NP;
        last = at;
        ++n;
    });
    int present = 0;
    for (int p = 0; p < QLN_MODEL_NP; ++p)
        for (int r = 0; r < 15; ++r) present += model_entry_present(r, p) ? 1 : 0;
    return ok && n == kModelNnz && present == kModelNnz;
}
static_assert(model_entries_in_order(), "G's 24 entries, each once, in column-major order");

}  // namespace
}  // namespace qln
