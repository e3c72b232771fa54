// qln_launch_plan.h -- which instantiation of k_constraint_jacobian<T, KC, W, WITH_C, WITH_J, NNZ, SPLIT, STREAM, WITH_F>
// (qln_kernels.hip) serves a request, and with what grid, dynamic LDS and L2 prefetch.  Host-only integer arithmetic on
// (nb, N, format, outputs), the only statement of these rules (DESIGN.md section 4.1 has the measurements behind them): no HIP
// call, no environment, so tests/test_launch_plan_host.py checks it without a GPU.  Internal.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "qln_device.h"

namespace qln {

// Sizes the kernel and the LDS sizing below share (doubles): the staged slice of Z of a chunk of KC knots, the even offset
// of the residual stage behind it, and one wave-row of the unpredicated staging writes (= kWave).
constexpr int chunk_z_slice(int KC) { return KC * 20 + 15; }
constexpr int chunk_c_stage(int KC) { return (chunk_z_slice(KC) + 1) & ~1; }
constexpr int kStageRow = 64;

struct LaunchRequest {
    int32_t nb = 0, N = 0, jac_format = QLN_JAC_FORMAT_DENSE_BLOCKS;
    int32_t kt_max = 0;                                     // largest k_trans of the batch
    bool c = false, vals = false, f = false, grad = false;  // f + vals: qln_eval_all (grad rides along, chooses nothing); f + c: a line search
    bool prefer_latency = false;                            // kLaunchSplit: a small batch whose caller waits for the result
    // the knob builds' environment (make tuning / prefetchknob): QLN_VARIANT, QLN_PREFETCH_AHEAD (problems) and _MASK (1 = slice
    // of Z, 2 = boundary vectors, 4 = descriptor; < 0: the plan's own), QLN_PAD_LDS (unused LDS of the c + J launch: fewer waves)
    int variant = 0, prefetch_ahead = -1, prefetch_mask = -1;
    unsigned pad_lds = 0;
};

struct LaunchPlan {
    int T, KC, W;
    bool with_c, with_j, nnz, split, stream, with_f;
    int workgroups;                          // before xcd_grid
    unsigned lds_bytes;                      // dynamic LDS
    uint32_t prefetch_ahead, prefetch_what;  // problems ahead on the XCD (0 = off); kPrefetchNoZ | kPrefetchBnd | kPrefetchDesc
};

// Tile, chunk size and register budget of a launch, and whether it is one workgroup per chunk
struct PlanShape {
    int T, KC, W;
    bool nnz = false, split = false;
    int prefetch_knots = 0;  // prefetch kDensePrefetchAhead problems ahead when c is written and N - 1 <= this; 0: never
    bool by_rows = false;    // a launch of c alone: the rows of c decide the streaming, not the Jacobian's bytes
};

// 40-knot chunks where they make no more passes than 64-knot chunks would (N <= 41, 66 <= N <= 81, ...)
inline bool chunks_of_40(int N) { return (N - 1 + 39) / 40 == (N - 1 + 63) / 64; }

// Dynamic LDS of the structural-format instantiations (bytes): the longest run of vals a sub-tile of `sub` knots can be
// in this batch -- a chunk's run grows with k_trans (71 values per knot before the transition, 57 after), so the batch's
// largest k_trans bounds it -- plus the parity slot, and never less than what aliases the tile: the staged slice of Z
// (written unpredicated in whole wave-rows), the residual stage and, for qln_eval_all, the objective terms.
inline size_t nnz_lds_bytes(int N, int kt_max, int KC, int sub, bool with_f) {
    const int kt = std::min(std::max(kt_max, 1), N + 1);
    int longest = 0;
    for (int kc0 = 0; kc0 < N - 1; kc0 += KC) {
        const int nk = std::min(KC, N - 1 - kc0);
        for (int t0 = 0; t0 < nk; t0 += sub) {
            const int nkt = std::min(sub, nk - t0);
            // x of the run's knots lie before the transition knot at the batch's largest k_trans (71 values each), and no
            // problem of the batch has more of them; every other knot has at most 57: 57 nkt + 14 x bounds every problem's run
            const int x = std::min(nkt, std::max(0, std::min(kt - 2, N - 1) - (kc0 + t0)));
            longest = std::max(longest, step_nnz(2) * nkt + (step_nnz(0) - step_nnz(2)) * x);
        }
    }
    const int rows = (chunk_z_slice(KC) + kStageRow - 1) / kStageRow;
    const int need = std::max({chunk_c_stage(KC) + KC * 15 + (with_f ? kStageRow : 0), rows * kStageRow, longest + 2});
    return (size_t)((need + 1) & ~1) * sizeof(double);
}

#ifdef QLN_TUNING
// Tuning build only (make tuning -> libqln_hip_tuning.so): the shapes QLN_VARIANT selects for A/B runs, and when each
// applies -- always, to a call without vals, to a dense handle, to a structural handle with vals.  Otherwise: the product's.
enum VariantWhen { kAlways, kNoVals, kDense, kStructuralVals };
constexpr struct { int id; VariantWhen when; PlanShape shape; } kVariants[] = {
    // dense tile / register budget; 4-6 with the shipping prefetch; 7-10 40-knot chunks (13 staging registers instead of 21)
    {1, kAlways, {8, 64, 2}}, {2, kAlways, {12, 64, 1}}, {3, kAlways, {16, 64, 1}},
    {4, kAlways, {12, 64, 1, false, false, 64}}, {5, kAlways, {12, 64, 2, false, false, 64}}, {6, kAlways, {10, 64, 2, false, false, 64}},
    {7, kAlways, {12, 40, 2, false, false, 40}}, {8, kAlways, {8, 40, 2, false, false, 40}},
    {9, kAlways, {16, 40, 2, false, false, 40}}, {10, kAlways, {10, 40, 2, false, false, 40}},
    // structural format: chunk size / sub-tiles (16, 17, 19) / register budget
    {11, kStructuralVals, {0, 32, 2, true}}, {12, kStructuralVals, {0, 40, 2, true}}, {13, kStructuralVals, {0, 32, 1, true}},
    {14, kStructuralVals, {0, 64, 1, true}}, {15, kStructuralVals, {0, 64, 2, true}}, {16, kStructuralVals, {20, 40, 3, true}},
    {17, kStructuralVals, {20, 40, 2, true}}, {18, kStructuralVals, {0, 40, 2, true}}, {19, kStructuralVals, {14, 40, 3, true}},
    // small-batch launches: one workgroup per chunk
    {21, kDense, {16, 16, 1, false, true}}, {22, kDense, {8, 8, 2, false, true}}, {23, kDense, {10, 10, 2, false, true}},
    {24, kStructuralVals, {0, 16, 2, true, true}}, {25, kStructuralVals, {0, 8, 2, true, true}},
    // constraint-only launch: chunk size / tile (= LDS) / register budget
    {31, kNoVals, {5, 40, 2, false, false, 0, true}}, {32, kNoVals, {5, 40, 3, false, false, 0, true}}, {33, kNoVals, {5, 40, 4, false, false, 0, true}},
    {34, kNoVals, {8, 64, 3, false, false, 0, true}}, {35, kNoVals, {8, 64, 4, false, false, 0, true}},
    {36, kNoVals, {4, 32, 3, false, false, 0, true}}, {37, kNoVals, {4, 32, 4, false, false, 0, true}},
};
#endif

inline PlanShape plan_shape(const LaunchRequest& r) {
    const bool structural = r.jac_format == QLN_JAC_FORMAT_STRUCTURAL;
    // Latency-bound callers (the host-pointer MOI mode: one problem or a handful) get one workgroup per 16-knot chunk instead
    // of per problem: the launch is then as long as one chunk.  It pays below ~256 problems only.  c alone: the dense kernel.
    if (r.prefer_latency && !r.f && r.nb <= 256 && r.N > 17)
        return (r.vals && structural) ? PlanShape{0, 16, 2, true, true} : PlanShape{16, 16, 1, false, true};
    // qln_eval_all: the structural format always in 40-knot chunks; dense one-chunk problems prefetch
    if (r.f && r.vals) return structural ? PlanShape{0, 40, 1, true} : PlanShape{16, 64, 1, false, false, 64};
#ifdef QLN_TUNING
    for (const auto& v : kVariants)
        if (v.id == r.variant && !r.f &&
            (v.when == kAlways || (v.when == kNoVals && !r.vals) || (v.when == kDense && !structural) ||
             (v.when == kStructuralVals && structural && r.vals)))
            return v.shape;
#endif
    // c alone, or f + c: no tile to fill, the LDS holds only the staged slice and the residual stage; two waves per SIMD
    if (!r.vals) return chunks_of_40(r.N) ? PlanShape{5, 40, 2, false, false, 0, true} : PlanShape{8, 64, 2, false, false, 0, true};
    // structural c / J: 64-knot chunks where they cover the horizon in fewer passes (N - 1 = 41 .. 64, 81 .. 128, ...)
    if (structural) return chunks_of_40(r.N) ? PlanShape{0, 40, 1, true} : PlanShape{0, 64, 1, true};
    // dense c / J: a 12-block tile, one wave per SIMD; one-chunk problems prefetch the slice of Z of a later workgroup into L2
    return PlanShape{12, 64, 1, false, false, 64};
}

inline LaunchPlan plan_launch(const LaunchRequest& r) {
    const PlanShape s = plan_shape(r);
    LaunchPlan pl{};
    pl.T = s.T, pl.KC = s.KC, pl.W = s.W;
    pl.with_c = r.c, pl.with_j = r.vals, pl.nnz = s.nnz, pl.split = s.split, pl.with_f = r.f;
    pl.workgroups = s.split ? r.nb * ((r.N - 2) / s.KC + 1) : r.nb;
    // outputs larger than the caches are streamed (non-temporal stores); row_layout at k_trans = 0: more rows than any problem has
    const int64_t bytes = s.by_rows ? (int64_t)row_layout(r.N, 0).m * 8 : (int64_t)(r.N - 1) * (s.nnz ? step_nnz(0) : 300) * 8;
    pl.stream = r.nb * bytes > ((int64_t)512 << 20);
    pl.lds_bytes = (s.nnz ? (unsigned)nnz_lds_bytes(r.N, r.kt_max, s.KC, s.T > 0 ? s.T : s.KC, r.f) : 0u) +
                   ((r.c && r.vals && !r.f) ? r.pad_lds : 0u);
    if (s.split || (r.f && !r.vals)) return pl;  // neither prefetches, knob or not
    // with the objective riding along, the later problem's boundary vectors and descriptor too (without it they cost what the slice gains)
    if (s.prefetch_knots && r.c && r.N - 1 <= s.prefetch_knots) {
        pl.prefetch_ahead = kDensePrefetchAhead;
        pl.prefetch_what = r.f ? kPrefetchBnd | kPrefetchDesc : 0u;
    }
    if (r.prefetch_ahead >= 0) pl.prefetch_ahead = (uint32_t)r.prefetch_ahead;
    const int m = r.prefetch_mask;
    if (m >= 0) pl.prefetch_what = ((m & 1) ? 0u : kPrefetchNoZ) | ((m & 2) ? kPrefetchBnd : 0u) | ((m & 4) ? kPrefetchDesc : 0u);
    return pl;
}

// The kernel's flags word: bit 0 QLN_JAC_WRITE_CONSTANTS, bits 8..28 the prefetch distance, bits 29..31 what is prefetched
inline uint32_t kernel_flags(const LaunchPlan& pl, bool write_constants) {
    return (write_constants ? (uint32_t)QLN_JAC_WRITE_CONSTANTS : 0u) | (pl.prefetch_ahead << 8) | pl.prefetch_what;
}

}  // namespace qln
