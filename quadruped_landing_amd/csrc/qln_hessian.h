// qln_hessian.h -- the Hessian of the Lagrangian of one dynamics knot in closed form (qln_hessian_kernels.hip) and its
// fixed sparse pattern (qln_api.cpp's qln_hessian_structure).  Internal; the contract is in include/qln_evaluator.h.
//
// Variables of step block k: z = (x_k[0..14], F1x, F1y, F2x, F2y, h) = columns 0..19.  The step is the polynomial of
// qln_kernels.hip's header (p+ = p + h v + h^2/2 a, v+ = v + h a, theta+ / omega+ through tau0, tauv, taua):
//   * tau0 is bilinear in the relative positions (x0, x1, x3..x6) and the forces, tauv in the relative velocities
//     (x7, x8, x10..x13) and the forces, taua = g (1 - m1) F1x + g (1 - m2) F2x is linear in the forces -- the r x F
//     products of the accelerations cancel, so no force x force and no theta-coupled second derivative survives;
//   * every other row is linear in x and in the forces for a fixed h.
// So mu . M rk4 has second derivatives only in (force, state) pairs of tau0 / tauv (16 entries) and in the h row (18):
// 34 lower-triangle entries.  The objective h l(x, u) adds the 19 diagonal entries of x and the forces and (h, theta),
// (h, clock): 55.  Row >= col, column-major over the pattern -- the order of the values inside a block.
#pragma once

#include <hip/hip_runtime.h>

#include "qln_device.h"

namespace qln {

constexpr int kHessStep = 55;   // QLN_HESS_STEP_NNZ
constexpr int kHessTerm = 15;   // QLN_HESS_TERM_NNZ

// (row, col) of the 55 entries of a step block, column-major
__host__ __device__ constexpr bool hess_entry_present(int row, int col) {
    if (row < col || row > 19 || col < 0) return false;
    if (row == col || row == 19) return true;  // the diagonal of x and the forces, (h, h), and the whole h row
    switch (col) {                             // (force, state) pairs of tau0 (positions) and tauv (velocities)
        case 0: case 7: return row == 16 || row == 18;
        case 1: case 8: return row == 15 || row == 17;
        case 3: case 10: return row == 16;
        case 4: case 11: return row == 15;
        case 5: case 12: return row == 18;
        case 6: case 13: return row == 17;
        default: return false;
    }
}
__host__ __device__ constexpr int hess_entry_pos(int row, int col) {
    int n = 0;
    for (int c = 0; c <= col; ++c)
        for (int r = 0; r < 20; ++r) {
            if (c == col && r == row) return n;
            if (hess_entry_present(r, c)) ++n;
        }
    return n;
}
static_assert(hess_entry_pos(20, 19) == kHessStep, "the step-block pattern has 55 entries");

// Clearance curvature of a knot: derivative of quirk Q3's jac_c! entry
__host__ __device__ __forceinline__ double clearance_curvature(double th, double lb) {
    const double s_th = sin(th);
    return (th > 0) ? (0.5 * lb) * s_th : -((0.5 * lb) * s_th);
}

// The 55 values of step block k of H = sigma d2(h l) + d2(mu_dyn . M rk4) + mu_clr c''(theta) e2 e2', column-major.
//   z:    x_k[0..14], F1x, F1y, F2x, F2y, h
//   rec:  Q[15] R[5] q[15] r[5] of the knot's cost record (its constant is not needed)
//   lam:  the knot's 15 dynamics multipliers with the jump mask already applied (masked rows = 0)
//   md:   the knot's contact mode (its jump flag is not read: the mask is in lam);  M: the model constants
//   mu_c: the clearance multiplier of the knot; sig: sigma
// The clearance term is the derivative of the entry jac_c! writes (quirk Q3): (lb/2) sin(theta) for theta > 0,
// -(lb/2) sin(theta) otherwise.
template <typename Z, typename R, typename L, typename O>
__host__ __device__ __forceinline__ void hessian_step_block(const Z& z, const R& rec, const L& lam, KnotMode md, const Model& M,
                                                            double mu_c, double sig, O&& out) {
    const double g = M.g, mb = M.mb, mf = M.mf, lb = M.lb;
    const double F1x = z[15], F1y = z[16], F2x = z[17], F2y = z[18], h = z[19];
    const double m1 = md.f1free ? 1.0 : 0.0, m2 = md.f2free ? 1.0 : 0.0;
    const double iIb = 1.0 / M.Ib;
    const double h2 = h * h;
    const double Aw = h * iIb, At = 0.5 * h2 * iIb, Bt = h2 * h * iIb * (1.0 / 6.0);
    const double sFx = F1x + F2x, sFy = F1y + F2y;
    const double r1x = z[3] - z[0], r1y = z[4] - z[1], r2x = z[5] - z[0], r2y = z[6] - z[1];
    const double w1x = m1 * z[10] - z[7], w1y = m1 * z[11] - z[8];
    const double w2x = m2 * z[12] - z[7], w2y = m2 * z[13] - z[8];
    const double tau0 = r1x * F1y - r1y * F1x + r2x * F2y - r2y * F2x;
    const double tauv = w1x * F1y - w1y * F1x + w2x * F2y - w2y * F2x;
    const double ga1 = g * (1.0 - m1), ga2 = g * (1.0 - m2);
    const double taua = ga1 * F1x + ga2 * F2x;
    const double abx = sFx / mb, aby = sFy / mb + g;
    const double a1x = m1 * (-F1x / mf), a1y = m1 * (-F1y / mf + g);
    const double a2x = m2 * (-F2x / mf), a2y = m2 * (-F2y / mf + g);
    const double imb = 1.0 / mb, imf = 1.0 / mf, hmb = h * imb, hmf = h * imf;
    const double l0 = lam[0], l1 = lam[1], l2 = lam[2], l3 = lam[3], l4 = lam[4], l5 = lam[5], l6 = lam[6];
    const double l7 = lam[7], l8 = lam[8], l9 = lam[9], l10 = lam[10], l11 = lam[11], l12 = lam[12], l13 = lam[13];
    // multipliers of the theta / omega rows times the h-weights of tau0 / tauv in those rows and their h-derivatives
    const double cT0 = l2 * At + l9 * Aw;   // d2/(dF dr):  theta+ carries h^2/2 tau0, omega+ h tau0
    const double cTv = l2 * Bt + l9 * At;   // d2/(dF dw):  h^3/6 tauv, h^2/2 tauv
    const double dT0 = l2 * Aw + l9 * iIb;  // d2/(dh dr)
    const double dTv = cT0;                 // d2/(dh dw)
    // objective sigma h l(x, u): l = 1/2 x'Qx + q'x + 1/2 u'Ru + r'u + c with u[4] = h
    const double sh = sig * h;
    const double clr = clearance_curvature(z[2], lb);
#define QH_D(i) (sh * rec[i])                                // (x_i, x_i)
#define QH_X(i) (sig * (rec[i] * z[i] + rec[20 + i]))         // (h, x_i)
#define QH_U(j) (sig * (rec[15 + j] * z[15 + j] + rec[35 + j]))  // (h, F_j)
    out(0, QH_D(0));
    out(1, -cT0);
    out(2, -cT0);
    out(3, QH_X(0) - dT0 * sFy);
    out(4, QH_D(1));
    out(5, cT0);
    out(6, cT0);
    out(7, QH_X(1) + dT0 * sFx);
    out(8, QH_D(2) + mu_c * clr);
    out(9, QH_X(2));
    out(10, QH_D(3));
    out(11, cT0);
    out(12, QH_X(3) + dT0 * F1y);
    out(13, QH_D(4));
    out(14, -cT0);
    out(15, QH_X(4) - dT0 * F1x);
    out(16, QH_D(5));
    out(17, cT0);
    out(18, QH_X(5) + dT0 * F2y);
    out(19, QH_D(6));
    out(20, -cT0);
    out(21, QH_X(6) - dT0 * F2x);
    out(22, QH_D(7));
    out(23, -cTv);
    out(24, -cTv);
    out(25, QH_X(7) + (l0 - dTv * sFy));
    out(26, QH_D(8));
    out(27, cTv);
    out(28, cTv);
    out(29, QH_X(8) + (l1 + dTv * sFx));
    out(30, QH_D(9));
    out(31, QH_X(9) + l2);
    out(32, QH_D(10));
    out(33, m1 * cTv);
    out(34, QH_X(10) + m1 * (l3 + dTv * F1y));
    out(35, QH_D(11));
    out(36, -(m1 * cTv));
    out(37, QH_X(11) + m1 * (l4 - dTv * F1x));
    out(38, QH_D(12));
    out(39, m2 * cTv);
    out(40, QH_X(12) + m2 * (l5 + dTv * F2y));
    out(41, QH_D(13));
    out(42, -(m2 * cTv));
    out(43, QH_X(13) + m2 * (l6 - dTv * F2x));
    out(44, QH_D(14));
    out(45, QH_X(14));
    // (h, F): body position / velocity rows, the free foot's position / velocity rows, theta and omega
    const double bx = l0 * hmb + l7 * imb, by = l1 * hmb + l8 * imb;
    out(46, sh * rec[15]);
    out(47, QH_U(0) + (bx - m1 * (l3 * hmf + l10 * imf)) + (l2 * (-Aw * r1y - At * w1y + Bt * ga1) +
                                                             l9 * iIb * (-r1y - h * w1y + 0.5 * h2 * ga1)));
    out(48, sh * rec[16]);
    out(49, QH_U(1) + (by - m1 * (l4 * hmf + l11 * imf)) + (l2 * (Aw * r1x + At * w1x) + l9 * iIb * (r1x + h * w1x)));
    out(50, sh * rec[17]);
    out(51, QH_U(2) + (bx - m2 * (l5 * hmf + l12 * imf)) + (l2 * (-Aw * r2y - At * w2y + Bt * ga2) +
                                                             l9 * iIb * (-r2y - h * w2y + 0.5 * h2 * ga2)));
    out(52, sh * rec[18]);
    out(53, QH_U(3) + (by - m2 * (l6 * hmf + l13 * imf)) + (l2 * (Aw * r2x + At * w2x) + l9 * iIb * (r2x + h * w2x)));
    // (h, h): 2 dl/dh + h d2l/dh2 of the objective; the h-curvature of every row of the step
    const double hh_obj = sig * (2.0 * (rec[19] * h + rec[39]) + h * rec[19]);
    const double hh_dyn = (l0 * abx + l1 * aby) + (l3 * a1x + l4 * a1y + l5 * a2x + l6 * a2y) +
                          l2 * (iIb * (tau0 + h * tauv + 0.5 * h2 * taua)) + l9 * (iIb * (tauv + h * taua));
    out(54, hh_obj + hh_dyn);
#undef QH_D
#undef QH_X
#undef QH_U
}

}  // namespace qln
