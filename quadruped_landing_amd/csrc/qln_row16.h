// qln_row16.h -- what the kernels on the row-of-sixteen mapping share (qln_tracking_kernels.hip: the TVLQR sweep, the
// roll-out's reverse and tangent sweeps, the covariance sweep; qln_ilqr_kernels.hip: the solve's Riccati sweep and
// roll-out lanes).  Internal; included by those two files only.
//   * DPP moves inside a row of sixteen lanes: dpp_f64, the named row shifts, quad_sum / row_sum16, row_bcast;
//   * the compact four-slots-per-column form of A = d x+/d x: a_slot, a_coupling, checked against the union pattern;
//   * the mapping itself -- one problem per row, four problems per wave: Row16 / row16_of;
//   * a knot's twenty doubles across a row: knot_load / knot_store.
// What the sweeps with a symmetric 15 x 15 matrix per row in LDS add to this (the covariance sweep, the Kalman sweep) -- the
// image, its tiles, the dense chains, the congruence step, the marginals -- is qln_image15.h, on top of this file.
#pragma once

#include "qln_kernel_common.h"

namespace qln {
namespace {

constexpr int kRows = kWave / 16;  // problems per wave

// v from the lane the DPP control names, as two 32-bit moves.  bound_ctrl is set: a lane whose source lies outside the
// row (the shifts) reads 0.0, and where every lane has a source no old value has to be prepared.
template <int kCtrl>
__device__ __forceinline__ double dpp_f64(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), kCtrl, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), kCtrl, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double row_shr7(double v) { return dpp_f64<0x117>(v); }  // v of lane ln - 7 (0.0 for ln < 7)
__device__ __forceinline__ double row_shl7(double v) { return dpp_f64<0x107>(v); }  // v of lane ln + 7 (0.0 for ln > 8)
// sums over the four lanes of a quad / the sixteen of a row (all active), the same bits in every lane: each step adds a
// commuted pair
__device__ __forceinline__ double quad_sum(double v) {
    v += dpp_f64<0xB1>(v);  // quad_perm [1, 0, 3, 2]
    v += dpp_f64<0x4E>(v);  // quad_perm [2, 3, 0, 1]
    return v;
}
__device__ __forceinline__ double row_sum16(double v) {
    v = quad_sum(v);
    v += dpp_f64<0x141>(v);  // row_half_mirror
    v += dpp_f64<0x140>(v);  // row_mirror
    return v;
}
// lane I of each row of sixteen lanes, in every lane of that row (DPP row_newbcast: one v_mov_b64_dpp, no LDS, no wait).
// The source lane must be enabled.  bound_ctrl as in dpp_f64: every lane has a source, so no old value is prepared.
template <int I>
__device__ __forceinline__ double row_bcast(double v) {
    static_assert(I >= 0 && I < 16, "a lane of the row");
    return __builtin_amdgcn_update_dpp(0.0, v, 0x150 + I, 0xf, 0xf, true);
}

// A = d x+/d x has at most four entries per column c: the diagonal, rows 2 (theta) and 9 (omega), and for the velocity
// columns c in {7, 8, 10 .. 13} the coupling A(c-7, c) (a position picks up h times its velocity).  A column's four
// slots are {A(c,c), A(2,c), A(9,c), A(c-7,c)}; by symmetry of the rule a row r's coupling is A(r, r+7).
__host__ __device__ constexpr int a_slot(int row, int col) { return row == col ? 0 : row == 2 ? 1 : row == 9 ? 2 : 3; }
__host__ __device__ constexpr int a_coupling(int c) { return (c == 7 || c == 8 || (c >= 10 && c <= 13)) ? c - 7 : -1; }
constexpr bool a_structure_ok() {
    for (int c = 0; c < 15; ++c)
        for (int r = 0; r < 15; ++r)
            if (step_union_present(r, c) && !(r == c || r == 2 || r == 9 || r == a_coupling(c))) return false;
    return true;
}
static_assert(a_structure_ok(), "A has four entries per column: diagonal, rows 2 and 9, and row c-7");

// One problem per row of sixteen lanes.  Lane ln < 15 owns index j = ln of the problem's fifteen states (a row or a
// column of a 15 x 15 matrix, an entry of a vector); lane 15 shadows j = 14 and contributes / stores nothing of its
// own.  Waves take problems in XCD-contiguous order; the rows past the batch's end work on the last problem (bc) and
// store nothing (valid).
struct Row16 {
    int ln, row;  // lane inside the row, row inside the wave
    int j;
    bool own;     // ln < 15
    int b, bc;    // the row's problem, and the same clamped to the batch
    bool valid;   // b < B
    int kt, im;   // the problem's k_trans and init_mode
    Model M;
};
__device__ __forceinline__ Row16 row16_of(const BatchParams& P) {
    const int lane = threadIdx.x;
    const int ln = lane & 15, row = lane >> 4;
    const bool own = ln < 15;
    const int wave = xcd_contiguous_index(blockIdx.x, (P.B + kRows - 1) / kRows);
    const int b = wave * kRows + row;
    const bool valid = b < P.B;
    const int bc = valid ? b : P.B - 1;
    const ProblemDesc pd = P.desc[bc];
    return {ln, row, own ? ln : 14, own, b, bc, valid, pd.k_trans, pd.init_mode, Model(P)};
}
__host__ inline unsigned row16_grid(int B) { return xcd_grid((B + kRows - 1) / kRows); }

// A knot's twenty doubles (x_k, u_k) across a row.  In: two coalesced loads, lane ln takes entry ln (lane j < 15: x_j,
// lane 15: u_0) and entry 16 + (ln & 3) (u_1 .. u_4 in lanes 0-3, repeated in the others).  Out: lane j < 15 stores its
// xj, and the five values of u (the same in every lane of the row) leave from lane 15 and lanes 0-3.
__device__ __forceinline__ void knot_load(const double* __restrict__ zk, int ln, double& e0, double& e1) {
    e0 = zk[ln];
    e1 = zk[16 + (ln & 3)];
}
__device__ __forceinline__ void knot_store(double* __restrict__ zk, const Row16& r, double xj, const double (&u)[5]) {
    zk[r.ln] = r.own ? xj : u[0];
    if (r.ln < 4) zk[16 + r.ln] = r.ln == 0 ? u[1] : r.ln == 1 ? u[2] : r.ln == 2 ? u[3] : u[4];
}

}  // namespace
}  // namespace qln
