// qln_image15.h -- what the sweeps that keep symmetric 15 x 15 matrices in LDS share (qln_tracking_kernels.hip: the covariance
// sweep and the Kalman sweep; the smoother takes the stride and sym_at and states its knot itself, see there).
// Internal; included by that file only.  On qln_row16.h's mapping, one problem per row of sixteen lanes, lane j owns column j:
//   * the image: a matrix in the row's LDS with row stride kImgStr, of which only the lower triangle is ever read as the
//     matrix -- sym_at, Image15 and its column / row / transposed accessors;
//   * packed tiles in and out, coalesced: the offset tables of the packed lower triangle, of a knot's K and of its gain, the
//     lane of a tile (TileLane) and tile_fill / tile_store / k_request;
//   * dense chains on broadcast LDS reads (chain_rows, chain_rows_sub) with the rows-in-flight fence;
//   * the congruence step X <- Op X Op' (+ diag w) through the image;
//   * the eight marginals of a knot over an entry accessor.
// Every rule of these kernels is stated here once: which triangle is read, where a wave_lds_sync stands between a read and a
// write of the image, why a tail's lane mask comes from an opaque copy, why one row of a tile is in flight at a time.
#pragma once

#include "qln_row16.h"

#include <type_traits>

namespace qln {
namespace {

// Row stride of an image: 17 is odd, so a lane's row (consecutive addresses) and its column (stride 17) both spread over the banks.
constexpr int kImgStr = 17;
constexpr int kImgSize = 15 * kImgStr;

// entry (i, c) of a symmetric image, read from its lower triangle
__host__ __device__ constexpr int sym_at(int i, int c) { return (i >= c) ? kImgStr * i + c : kImgStr * c + i; }

// One image as lane j of its row sees it.  A write of the image stands between two wave_lds_sync: one behind the last read of
// what it overwrites, one in front of the first read of what it wrote (the congruence step below shows the pattern).
struct Image15 {
    double* a;  // the image's entry (0, 0) in the row's LDS
    int j;      // the lane's column; lane 15 shadows column 14
    bool own;   // ... and writes nothing to the image

    // entry c of column j, from the lower triangle: (max(c, j), min(c, j))
    __device__ __forceinline__ int sym(int c) const { return (c <= j) ? kImgStr * j + c : j + kImgStr * c; }
    __device__ __forceinline__ void column(double (&v)[15]) const {
#pragma unroll
        for (int c = 0; c < 15; ++c) v[c] = a[sym(c)];
    }
    // the lane's column stored as row j: consecutive addresses, and nothing symmetrises -- the reader decides what it reads
    __device__ __forceinline__ void store_row(const double (&v)[15]) const {
        if (own) {
#pragma unroll
            for (int i = 0; i < 15; ++i) a[kImgStr * j + i] = v[i];
        }
    }
    // column j of what the lanes stored as rows: row j of the product, transposed
    __device__ __forceinline__ void transposed(double (&v)[15]) const {
#pragma unroll
        for (int c = 0; c < 15; ++c) v[c] = a[kImgStr * c + j];
    }
    __device__ __forceinline__ void add_diagonal(double w) const {
        if (own) a[(kImgStr + 1) * j] = a[(kImgStr + 1) * j] + w;
    }
};

// Where the entries ln + 16 t of a packed tile lie: the packed lower triangle in an image (relative to the image), a knot's K
// [4][15] in a tile with rows of sixteen and a knot's gain [15][ny] in a tile with rows of QLN_TRACK_NY_MAX (both from base).
// The tails' entries are clamped to the tile's last; tile_fill and tile_store do not touch them.
__device__ __forceinline__ void packed_offsets(int ln, int (&po)[8]) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int i = min(ln + 16 * t, QLN_TRACK_P_NNZ - 1);
        int r = 0;
#pragma unroll
        for (int q = 1; q < 15; ++q) r += (i >= q * (q + 1) / 2) ? 1 : 0;
        po[t] = kImgStr * r + (i - r * (r + 1) / 2);
    }
}
__device__ __forceinline__ void k_offsets(int ln, int base, int (&ko)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int i = min(ln + 16 * t, QLN_TRACK_NU * QLN_NX - 1);
        const int m = i / 15;
        ko[t] = base + 16 * m + (i - 15 * m);
    }
}
__device__ __forceinline__ void gain_offsets(int ln, int ny, int base, int (&lo)[8]) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int g = min(ln + 16 * t, QLN_NX * ny - 1), gr = g / ny;
        lo[t] = base + QLN_TRACK_NY_MAX * gr + (g - ny * gr);
    }
}

// A lane of a tile: ln addresses, le forms the tails' predicates.  tile_lane makes le an opaque copy of ln: formed from ln itself
// the predicates are hoisted out of the knot loop, and the sixteen lane masks stay in scalar registers through every knot and
// push other scalars out (the Kalman sweep and the smoother).  The covariance sweep has those registers and passes {ln, ln}: the
// opaque form's compares in every knot cost it 4 % of a launch (profiles/sym_image_timing.txt).  How a new sweep decides: read
// its TotalSGPRs and SGPR spills in the compiler's resource report with {ln, ln}.  Sixteen masks are 32 scalar registers; a
// kernel that reports spills, or sits at the 106 it can have, takes tile_lane, one with that much room takes {ln, ln}.
struct TileLane {
    int ln, le;
};
__device__ __forceinline__ TileLane tile_lane(int ln) {
    int le = ln;
    asm volatile("" : "+v"(le));
    return {ln, le};
}
// entries ln + 16 t < count of a tile: into LDS at off[t] from src(t), and out of LDS (entry(off[t])) to o, coalesced
template <int T, class Src>
__device__ __forceinline__ void tile_fill(double* L, const int (&off)[T], int count, TileLane tl, Src src) {
#pragma unroll
    for (int t = 0; t < T; ++t)
        if (tl.le + 16 * t < count) L[off[t]] = src(t);
}
template <int T, class Entry>
__device__ __forceinline__ void tile_store(double* __restrict__ o, const int (&off)[T], int count, TileLane tl, Entry entry) {
#pragma unroll
    for (int t = 0; t < T; ++t)
        if (tl.le + 16 * t < count) o[tl.ln + 16 * t] = entry(off[t]);
}
// a knot's K entries ln + 16 t, requested (one knot ahead of the tile_fill that stages them)
__device__ __forceinline__ void k_request(const double* __restrict__ Kk, int ln, double (&kn)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) kn[t] = Kk[min(ln + 16 * t, QLN_TRACK_NU * QLN_NX - 1)];
}

// Dense chains on broadcast LDS reads: out[r] = sum_c e(r, c) v[c], a product first and fma from there on, c ascending.
// kFlight rows' reads are in flight together: an empty asm holds a row's sum in front of the next rows' reads.  Left to itself
// the compiler issues every row's reads first (K's four rows: 120 registers).  One wave per SIMD runs in these kernels, so a
// knot waits on LDS latency row by row; with three rows in flight the compiler hoisted the reads of whole chains and both
// instantiations of the smoother went to scratch (152 and 92 bytes per lane), so the default stays at one.
template <int kFlight = 1, int R, int C, class Entry>
__device__ __forceinline__ void chain_rows(Entry e, const double (&v)[C], double (&out)[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        double acc = e(r, 0) * v[0];
#pragma unroll
        for (int c = 1; c < C; ++c) acc = fma(e(r, c), v[c], acc);
        if (r % kFlight == kFlight - 1) asm volatile("" : "+v"(acc) : : "memory");
        out[r] = acc;
    }
}
// out[r] = from[r] - sum_c e(r, c) v[c]: fma(-e, v, .) onto the vector's entry, c ascending
template <int kFlight = 1, int R, int C, class Entry>
__device__ __forceinline__ void chain_rows_sub(Entry e, const double (&v)[C], const double (&from)[R], double (&out)[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        double acc = from[r];
#pragma unroll
        for (int c = 0; c < C; ++c) acc = fma(-e(r, c), v[c], acc);
        if (r % kFlight == kFlight - 1) asm volatile("" : "+v"(acc) : : "memory");
        out[r] = acc;
    }
}

// The congruence step X <- Op X Op' (+ diag w e_j e_j' per lane): two applications with a transpose through the image between
// them, X' = Op (Op X)'.  apply(v, out): out = Op v.  between() runs behind the first application while X is still in the
// image -- the outputs that leave there.  Afterwards only X's lower triangle may be read: it is then exactly symmetric.  The
// caller puts a wave_lds_sync between this and its next read of the image.  congruence_from: the lane already holds its column
// of X (the covariance sweep carries it from knot to knot).
struct NoDiagonal {};
template <class Apply, class Between, class Diag = NoDiagonal>
__device__ __forceinline__ void congruence_from(const Image15& X, const double (&col)[15], Apply apply, Between between, Diag w = {}) {
    double v[15], out[15];
    apply(col, out);  // column j of Op X
    between();
    wave_lds_sync();  // the image has been read: Op X may overwrite it
    X.store_row(out);
    wave_lds_sync();
    X.transposed(v);  // row j of Op X = column j of X Op'
    apply(v, out);
    wave_lds_sync();  // every lane holds its row of Op X
    X.store_row(out);
    if constexpr (!std::is_same<Diag, NoDiagonal>::value) X.add_diagonal(w);
}
template <class Apply, class Between, class Diag = NoDiagonal>
__device__ __forceinline__ void congruence(const Image15& X, Apply apply, Between between, Diag w = {}) {
    double col[15];
    X.column(col);
    congruence_from(X, col, apply, between, w);
}

// A knot's eight marginals (include/qln_evaluator.h) from the entries x(offset) of a symmetric image's lower triangle: the
// clearance row's variance with the row's derivative dth, the four force variances fv, two diagonal entries and the trace.
// img: an image of the lane (its column and whether it owns one); valid: the row's problem lies inside the batch.
template <class Entry>
__device__ __forceinline__ void marginals_store(double* __restrict__ mk, double dth, const double (&fv)[4], Entry x, const Image15& img,
                                                bool valid, TileLane tl) {
    const int j = img.j, ln = tl.ln, le = tl.le;
    const bool own = img.own;
    const double s11 = x(sym_at(1, 1)), s21 = x(sym_at(2, 1)), s22 = x(sym_at(2, 2));
    double mv[QLN_TRACK_MARG_STRIDE];
    mv[0] = fma(dth, fma(dth, s22, 2.0 * s21), s11);  // a' X a, a = e_yb + dth e_theta
#pragma unroll
    for (int m = 0; m < 4; ++m) mv[1 + m] = fv[m];
    mv[5] = x(sym_at(4, 4));
    mv[6] = x(sym_at(6, 6));
    const double dj = x((kImgStr + 1) * j);
    mv[7] = row_sum16(own ? dj : 0.0);
    double v = mv[0];
#pragma unroll
    for (int q = 1; q < QLN_TRACK_MARG_STRIDE; ++q) v = (le == q) ? mv[q] : v;
    if (valid && le < QLN_TRACK_MARG_STRIDE) mk[ln] = v;
}

}  // namespace
}  // namespace qln
