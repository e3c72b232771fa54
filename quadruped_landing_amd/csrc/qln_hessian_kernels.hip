// qln_hessian_kernels.hip -- gfx950 kernels of the Hessian of the Lagrangian:
//
//   k_hessian_lagrangian          H_b = sigma_b d2 eval_f(Z) + sum_i mu_i d2 c_i(Z)   lower triangle, fixed pattern
//                                 (qln_hessian.h; qln_eval_hessian_lagrangian)
//   k_hessian_lagrangian_product  y_b = H_b v_b, H never stored (qln_eval_hessian_lagrangian_product)
//
// The Hessian is block-diagonal over knots: dynamics row block k is linear in x_{k+1}, the objective is a sum of
// h_k l_k(x_k, u_k), clearance row k sees theta_k only, and the other constraint groups are linear.  So a step block
// needs the knot's 20 entries of Z, its 15 dynamics multipliers, its clearance multiplier, sigma and its cost record --
// the mapping of the evaluator: one 64-lane wavefront (= one workgroup) per problem, lane = dynamics knot, chunks of up to
// 64 knots.  The 55 values of a block are formed in registers in closed form (hessian_step_block of qln_hessian.h, from
// the knot's KnotMode and the Model of qln_device.h like the first-order step_block; ~120 flops), put into an LDS tile in the
// order of the output segment and drained as 16-byte-per-lane stores.
//
// Reads: the chunk's slice of Z and its dynamics multipliers are staged in LDS with coalesced 8-byte loads, all issued
// before the first wait.  Cost records: with a shared table and one chunk (N <= 65) the waves are persistent and lane k
// keeps knot k's record in registers for every problem it handles (the design of k_objective_shared); otherwise the
// chunk's records are staged in LDS with the slice (coalesced, one request per 512 B).
//
// The objective part is the Hessian of eval_f, the function.  It is NOT the Jacobian of grad_f!: quirk Q2 drops
// d(h l)/dh from the gradient, and the Jacobian of that gradient is not symmetric.
#include "qln_kernel_common.h"
#include "qln_hessian.h"

// Nothing here has to round like the reference (the parity tests hold it to 1e-8), so a*b+c may fuse.
#pragma clang fp contract(fast)

namespace qln {
namespace {

constexpr int kCostRec = QLN_COST_STRIDE;             // Q[15] R[5] q[15] r[5] c
constexpr int kHC = 64;                                 // dynamics knots per chunk
constexpr int kHZ = 20 * kHC;                           // doubles of Z a chunk stages (x_k, u_k of its knots)
constexpr int kHMu = 15 * kHC;                          // dynamics multipliers of a chunk
constexpr int kHRec = kCostRec * kHC;                   // cost records of a chunk
constexpr int kHTile = kHessStep * kHC + kHessTerm + 1; // the chunk's output (+ the terminal block, + one for parity)
constexpr int kZIters = kHZ / kWave, kMuIters = kHMu / kWave, kRecIters = kHRec / kWave;
static_assert(kHZ % kWave == 0 && kHMu % kWave == 0 && kHRec % kWave == 0, "whole staging rounds");
constexpr int kHMuOff = kHZ, kHRecOff = kHZ + kHMu;
constexpr int lds_doubles(bool rec_regs) {
    return rec_regs ? (kHTile > kHRecOff ? kHTile : kHRecOff) : (kHTile > kHRecOff + kHRec ? kHTile : kHRecOff + kHRec);
}

// JUMP_DIAG (src/planar_quadruped.jl:262-263): rows 4, 6, 10..14 (0-based) of the transition knot are masked
__device__ __forceinline__ bool jump_masked(int i) { return i == 4 || i == 6 || i >= 10; }

// One wave per problem of [its share of the batch]: problems are dealt XCD-contiguously -- workgroup w lies on XCD w & 7
// and takes the problems x * per_xcd + (w >> 3) + j * (gridDim.x >> 3) of that XCD's range -- so every XCD writes one
// forward-moving front.  gridDim.x is a multiple of 8.  REC_REGS: a shared cost table and N - 1 <= 64.
template <bool REC_REGS>
__global__ __launch_bounds__(kWave) void k_hessian_lagrangian(BatchParams P, const double* __restrict__ Z,
                                                              const double* __restrict__ S, const double* __restrict__ MU,
                                                              double* __restrict__ H, int64_t h_stride) {
    __shared__ __attribute__((aligned(16))) double s_lds[lds_doubles(REC_REGS)];
    double* const s_z = s_lds;
    double* const s_mu = s_lds + kHMuOff;
    double* const s_rec = s_lds + kHRecOff;
    double* const s_t = s_lds;  // output tile: aliases the staged inputs once every lane holds its own in registers
    const int lane = threadIdx.x;
    const int N = P.N;
    const Model M(P);
    const int per_xcd = (P.B + 7) >> 3, slots = gridDim.x >> 3;
    const int xcd = blockIdx.x & 7;

    double rrec[kCostRec - 1];  // REC_REGS: lane k's Q R q r (the constant is not needed)
    if constexpr (REC_REGS) {
        const double* __restrict__ rec = P.cost + kCostRec * min(lane, N - 2);
#pragma unroll
        for (int i = 0; i < kCostRec - 1; ++i) rrec[i] = rec[i];
    }

    for (int j = blockIdx.x >> 3; j < per_xcd; j += slots) {
        const int b = xcd * per_xcd + j;
        if (b >= P.B) break;  // wave-uniform
        const ProblemDesc pd = P.desc[b];
        const int kt = pd.k_trans, im = pd.init_mode;
        const double* __restrict__ Zb = Z + (int64_t)b * P.z_stride;
        const double* __restrict__ Mb = MU + pd.c_off;
        const double* __restrict__ Cb = P.cost + (P.cost_batch == 1 ? 0 : (int64_t)b * N * kCostRec);
        const RowLayout R = row_layout(N, kt);
        const double sig = S ? S[b] : 1.0;
        double* __restrict__ Hb = H + (int64_t)b * h_stride;

        for (int kc0 = 0; kc0 < N - 1; kc0 += kHC) {
            const int nk = min(kHC, N - 1 - kc0);
            const bool last_chunk = (kc0 + nk == N - 1);
            double mu_c, mu_cn, th_n, qf;
            {
                // every request of the chunk before the first wait; clamped indices instead of predicates
                double zr[kZIters], mr[kMuIters];
                const int nz = 20 * nk, nm = 15 * nk;
#pragma unroll
                for (int it = 0; it < kZIters; ++it) zr[it] = Zb[20 * kc0 + min(it * kWave + lane, nz - 1)];
#pragma unroll
                for (int it = 0; it < kMuIters; ++it) mr[it] = Mb[R.o_dyn + 15 * kc0 + min(it * kWave + lane, nm - 1)];
                mu_c = Mb[R.o_bp + kc0 + min(lane, nk - 1)];
                mu_cn = Mb[R.o_bp + N - 1];
                th_n = Zb[20 * (N - 1) + 2];
                qf = Cb[kCostRec * (N - 1) + min(lane, 14)];
                if constexpr (!REC_REGS) {
                    double rr[kRecIters];
                    const int nr = kCostRec * nk;
#pragma unroll
                    for (int it = 0; it < kRecIters; ++it) rr[it] = Cb[kCostRec * kc0 + min(it * kWave + lane, nr - 1)];
                    wave_lds_sync();  // the previous chunk's tile has been drained
#pragma unroll
                    for (int it = 0; it < kRecIters; ++it) s_rec[it * kWave + lane] = rr[it];
                } else {
                    wave_lds_sync();
                }
#pragma unroll
                for (int it = 0; it < kZIters; ++it) s_z[it * kWave + lane] = zr[it];
#pragma unroll
                for (int it = 0; it < kMuIters; ++it) s_mu[it * kWave + lane] = mr[it];
                wave_lds_sync();
            }
            const bool valid = lane < nk;
            const int kl = valid ? lane : 0;
            const int K = kc0 + kl + 1;  // 1-based dynamics knot
            const KnotMode md = knot_mode(K, kt - 1, im);
            double z[20], lam[15], rec[kCostRec - 1];
#pragma unroll
            for (int i = 0; i < 20; ++i) z[i] = s_z[20 * kl + i];
#pragma unroll
            for (int i = 0; i < 15; ++i) lam[i] = (md.jump && jump_masked(i)) ? 0.0 : s_mu[15 * kl + i];
#pragma unroll
            for (int i = 0; i < kCostRec - 1; ++i) rec[i] = REC_REGS ? rrec[i] : s_rec[kCostRec * kl + i];
            wave_lds_sync();  // every lane holds its inputs: the tile may overwrite the staged slice

            // the segment's 16-byte pieces: the tile's image starts at the parity of its global address
            double* __restrict__ G = Hb + kHessStep * kc0;
            const int par = (int)((reinterpret_cast<uintptr_t>(G) >> 3) & 1);
            double* const t = s_t + par;
            if (valid) {
                hessian_step_block(z, rec, lam, md, M, mu_c, sig,
                                   [&](int e, double v) { t[kHessStep * lane + e] = v; });
            }
            const int n = kHessStep * nk + (last_chunk ? kHessTerm : 0);
            if (last_chunk && lane < kHessTerm) {
                // terminal block: sigma Qf on the diagonal of x_N, the clearance curvature of x_N's row at theta
                double v = sig * qf;
                if (lane == 2) v = v + mu_cn * clearance_curvature(th_n, M.lb);
                t[kHessStep * nk + lane] = v;
            }
            wave_lds_sync();
            if (lane == 0) {
                if (par) G[0] = t[0];
                if ((par + n) & 1) G[n - 1] = t[n - 1];
            }
            const int q1 = (par + n) >> 1;  // pieces [par, q1) are whole
            double2* __restrict__ dst = reinterpret_cast<double2*>(G - par);
            const double2* src = reinterpret_cast<const double2*>(s_t);
            for (int q = par + lane; q < q1; q += kWave) dst[q] = src[q];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// y = H v without storing H (qln_eval_hessian_lagrangian_product)
// ---------------------------------------------------------------------------------------------
// The mapping, the staging and the record handling of k_hessian_lagrangian; the chunk's slice of v is staged in LDS next
// to Z's, and each of a block's 55 values is contracted with v where it is formed: y[r] += H_rc v[c], and y[c] += H_rc v[r]
// off the diagonal.  (r, c) of entry e come from a constexpr table, so once hessian_step_block is inlined and unrolled
// every index is a constant and y[20] stays in registers.  The blocks do not overlap (block k owns z_k's 20 entries, the
// terminal block x_N's 15), so the chunk's slice of y is complete in the lanes and leaves through an LDS tile as coalesced
// 8-byte stores (k_constraint_vjp's s_g).
struct HessEntryTable {
    int r[kHessStep], c[kHessStep];
};
constexpr HessEntryTable hess_entry_table() {
    HessEntryTable t{};
    int n = 0;
    for (int c = 0; c < 20; ++c)
        for (int r = c; r < 20; ++r)
            if (hess_entry_present(r, c)) {
                t.r[n] = r;
                t.c[n] = c;
                ++n;
            }
    return t;
}
constexpr HessEntryTable kHessEntry = hess_entry_table();
static_assert(kHessEntry.r[kHessStep - 1] == 19 && kHessEntry.c[kHessStep - 1] == 19, "(h, h) closes the pattern");

constexpr int kPVOff = kHZ + kHMu, kPRecOff = kPVOff + kHZ;  // v's slice behind the multipliers, then the records
constexpr int kPTile = 20 * kHC + 15;                        // the chunk's slice of y (+ x_N's 15 in the last chunk)
static_assert(kPTile <= kPVOff, "the output slice fits in the bytes of the staged Z and multipliers");
constexpr int product_lds_doubles(bool rec_regs) { return rec_regs ? kPRecOff : kPRecOff + kHRec; }

template <bool REC_REGS>
__global__ __launch_bounds__(kWave) void k_hessian_lagrangian_product(BatchParams P, const double* __restrict__ Z,
                                                                      const double* __restrict__ S,
                                                                      const double* __restrict__ MU,
                                                                      const double* __restrict__ V, double* __restrict__ Y) {
    __shared__ __attribute__((aligned(16))) double s_lds[product_lds_doubles(REC_REGS)];
    double* const s_z = s_lds;
    double* const s_mu = s_lds + kHMuOff;
    double* const s_v = s_lds + kPVOff;
    double* const s_rec = s_lds + kPRecOff;
    double* const s_t = s_lds;  // output slice: written once every lane is done with the staged slices
    const int lane = threadIdx.x;
    const int N = P.N;
    const Model M(P);
    const int per_xcd = (P.B + 7) >> 3, slots = gridDim.x >> 3;
    const int xcd = blockIdx.x & 7;

    double rrec[kCostRec - 1];  // REC_REGS: lane k's Q R q r (the constant is not needed)
    if constexpr (REC_REGS) {
        const double* __restrict__ rec = P.cost + kCostRec * min(lane, N - 2);
#pragma unroll
        for (int i = 0; i < kCostRec - 1; ++i) rrec[i] = rec[i];
    }

    for (int j = blockIdx.x >> 3; j < per_xcd; j += slots) {
        const int b = xcd * per_xcd + j;
        if (b >= P.B) break;  // wave-uniform
        const ProblemDesc pd = P.desc[b];
        const int kt = pd.k_trans, im = pd.init_mode;
        const double* __restrict__ Zb = Z + (int64_t)b * P.z_stride;
        const double* __restrict__ Vb = V + (int64_t)b * P.z_stride;
        const double* __restrict__ Mb = MU + pd.c_off;
        const double* __restrict__ Cb = P.cost + (P.cost_batch == 1 ? 0 : (int64_t)b * N * kCostRec);
        const RowLayout R = row_layout(N, kt);
        const double sig = S ? S[b] : 1.0;
        double* __restrict__ Yb = Y + (int64_t)b * P.z_stride;

        for (int kc0 = 0; kc0 < N - 1; kc0 += kHC) {
            const int nk = min(kHC, N - 1 - kc0);
            const bool last_chunk = (kc0 + nk == N - 1);
            double mu_c, mu_cn, th_n, qf, v_n;
            {
                // every request of the chunk before the first wait; clamped indices instead of predicates
                double zr[kZIters], vr[kZIters], mr[kMuIters];
                const int nz = 20 * nk, nm = 15 * nk;
#pragma unroll
                for (int it = 0; it < kZIters; ++it) zr[it] = Zb[20 * kc0 + min(it * kWave + lane, nz - 1)];
#pragma unroll
                for (int it = 0; it < kZIters; ++it) vr[it] = Vb[20 * kc0 + min(it * kWave + lane, nz - 1)];
#pragma unroll
                for (int it = 0; it < kMuIters; ++it) mr[it] = Mb[R.o_dyn + 15 * kc0 + min(it * kWave + lane, nm - 1)];
                mu_c = Mb[R.o_bp + kc0 + min(lane, nk - 1)];
                mu_cn = Mb[R.o_bp + N - 1];
                th_n = Zb[20 * (N - 1) + 2];
                qf = Cb[kCostRec * (N - 1) + min(lane, 14)];
                v_n = Vb[20 * (N - 1) + min(lane, 14)];
                if constexpr (!REC_REGS) {
                    double rr[kRecIters];
                    const int nr = kCostRec * nk;
#pragma unroll
                    for (int it = 0; it < kRecIters; ++it) rr[it] = Cb[kCostRec * kc0 + min(it * kWave + lane, nr - 1)];
                    wave_lds_sync();  // the previous chunk's slice of y has been drained
#pragma unroll
                    for (int it = 0; it < kRecIters; ++it) s_rec[it * kWave + lane] = rr[it];
                } else {
                    wave_lds_sync();
                }
#pragma unroll
                for (int it = 0; it < kZIters; ++it) s_z[it * kWave + lane] = zr[it];
#pragma unroll
                for (int it = 0; it < kZIters; ++it) s_v[it * kWave + lane] = vr[it];
#pragma unroll
                for (int it = 0; it < kMuIters; ++it) s_mu[it * kWave + lane] = mr[it];
                wave_lds_sync();
            }
            const bool valid = lane < nk;
            const int kl = valid ? lane : 0;
            const int K = kc0 + kl + 1;  // 1-based dynamics knot
            const KnotMode md = knot_mode(K, kt - 1, im);
            double z[20], lam[15], rec[kCostRec - 1], y[20];
#pragma unroll
            for (int i = 0; i < 20; ++i) z[i] = s_z[20 * kl + i];
#pragma unroll
            for (int i = 0; i < 15; ++i) lam[i] = (md.jump && jump_masked(i)) ? 0.0 : s_mu[15 * kl + i];
#pragma unroll
            for (int i = 0; i < kCostRec - 1; ++i) rec[i] = REC_REGS ? rrec[i] : s_rec[kCostRec * kl + i];
#pragma unroll
            for (int i = 0; i < 20; ++i) y[i] = 0.0;
            const double* const vk = s_v + 20 * kl;
            if (valid) {
                hessian_step_block(z, rec, lam, md, M, mu_c, sig, [&](int e, double h) {
                    const int r = kHessEntry.r[e], c = kHessEntry.c[e];
                    y[r] += h * vk[c];
                    if (r != c) y[c] += h * vk[r];
                });
            }
            double y_n = 0.0;
            if (last_chunk && lane < kHessTerm) {
                // terminal block: the diagonal of k_hessian_lagrangian's last 15 values times x_N's slice of v
                double h = sig * qf;
                if (lane == 2) h = h + mu_cn * clearance_curvature(th_n, M.lb);
                y_n = h * v_n;
            }
            wave_lds_sync();  // every lane is done with the staged slices: their bytes now take the result
            if (valid) {
#pragma unroll
                for (int i = 0; i < 20; ++i) s_t[20 * lane + i] = y[i];
            }
            if (last_chunk && lane < kHessTerm) s_t[20 * nk + lane] = y_n;
            wave_lds_sync();
            const int n = 20 * nk + (last_chunk ? kHessTerm : 0);
            for (int i = lane; i < n; i += kWave) Yb[20 * kc0 + i] = s_t[i];
        }
    }
}

}  // namespace

hipError_t launch_hessian_lagrangian(const BatchParams& p, const double* Z, const double* sigma, const double* mu, double* hvals,
                                     int64_t h_stride, hipStream_t stream) {
    const bool rec_regs = (p.cost_batch == 1 && p.N - 1 <= kHC);
    if (rec_regs) {
        // persistent: the record is loaded once per wave; four waves per CU over the 256 CUs
        const unsigned grid = std::min(xcd_grid(p.B), 8u * 128u);
        hipLaunchKernelGGL(k_hessian_lagrangian<true>, dim3(grid), dim3(kWave), 0, stream, p, Z, sigma, mu, hvals, h_stride);
    } else {
        hipLaunchKernelGGL(k_hessian_lagrangian<false>, dim3(xcd_grid(p.B)), dim3(kWave), 0, stream, p, Z, sigma, mu, hvals,
                           h_stride);
    }
    return hipGetLastError();
}

hipError_t launch_hessian_lagrangian_product(const BatchParams& p, const double* Z, const double* sigma, const double* mu,
                                             const double* v, double* y, hipStream_t stream) {
    // the grids of k_hessian_lagrangian
    if (p.cost_batch == 1 && p.N - 1 <= kHC) {
        const unsigned grid = std::min(xcd_grid(p.B), 8u * 128u);
        hipLaunchKernelGGL(k_hessian_lagrangian_product<true>, dim3(grid), dim3(kWave), 0, stream, p, Z, sigma, mu, v, y);
    } else {
        hipLaunchKernelGGL(k_hessian_lagrangian_product<false>, dim3(xcd_grid(p.B)), dim3(kWave), 0, stream, p, Z, sigma, mu, v,
                           y);
    }
    return hipGetLastError();
}

}  // namespace qln
