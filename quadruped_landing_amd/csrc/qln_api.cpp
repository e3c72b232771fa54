// qln_api.cpp -- the C ABI of include/qln_evaluator.h on top of the gfx950 kernels.
//
// Owns: the handle (device copies of the problem descriptors, offset tables, lazily allocated
// staging for the host-pointer MOI mode).  Never owns or reallocates caller buffers, never throws
// across the boundary, never calls exit (SURVEY.md 8b "Errors"/"Ownership").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "../../include/qln_evaluator.h"
#include "qln_device.h"
#include "qln_hessian.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define QLN_HIP(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(QLN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                \
    } while (0)

int64_t round_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// Lagrangian Hessian: 55 values per step block, 15 for the terminal diagonal; segments h_stride apart
int32_t hessian_nnz(int32_t N) { return QLN_HESS_STEP_NNZ * (N - 1) + QLN_HESS_TERM_NNZ; }
int64_t hessian_stride(int32_t N, int32_t align) { return round_up(hessian_nnz(N), align ? align : 16); }

// Whether a placed buffer's virtual range is handed back (hipMemAddressFree) when the buffer is released.
// It is NOT: on this stack (ROCm 7.2 user space, the pool's host driver) a virtual address that has been unmapped
// with hipMemUnmap keeps serving GPU accesses through the translations of its previous mapping, with every call
// returning hipSuccess -- so an address that was ever unmapped must never be mapped again, neither in place nor
// after hipMemAddressFree + hipMemAddressReserve (which hands the same addresses out again).  Reproduced without
// this library or torch by bench/vmm_va_reuse.cpp (profiles/r02_vmm_va_reuse.txt):
//   reserve R; map chunks A; fill through R; hipMemUnmap(R); map chunks B at R; fill through R
//     -> every word of A (still alive, inspected through a second mapping) carries B's pattern;
//   ... hipMemUnmap(R); hipMemAddressFree(R); hipMemAddressReserve -> R again; map B; fill; read back
//     -> ~0.7 % of the words read back wrong, and A (alive) has been written into.
// That is what round 1 saw as "writes through stale translations"; it is not a missing synchronisation (the device was
// idle at every unmap in that sequence, and is here).  Keeping a released buffer's range reserved costs address space
// only (~70 GiB of 128 TiB per qln_vals_alloc_placed call); the physical memory is returned.
constexpr bool kReturnVirtualRange = false;
// ... so every placed allocation retires its virtual range for the life of the process.  The ranges are counted, reported
// (qln_vals_placed_address_space) and capped well inside the 128 TiB of user address space: a process that places buffers in
// a loop gets a clear refusal after ~900 default-size calls instead of a failing hipMemAddressReserve somewhere else.
constexpr uint64_t kVaCapBytes = (uint64_t)64 << 40;  // 64 TiB: half the address space stays for everything else
std::atomic<uint64_t> g_va_retired{0};

// sizes of src/nlp.jl:48-87, from the two layouts of qln_device.h
int32_t m_nlp_of(int32_t N, int32_t kt) { return qln::row_layout(N, kt).m; }
int32_t nnz_dyn_of(int32_t N, int32_t kt, int32_t fmt) { return qln::vals_layout(N, kt, fmt).o_const; }
int32_t nnz_of(int32_t N, int32_t kt, int32_t fmt) { return qln::vals_layout(N, kt, fmt).nnz; }

int64_t tracking_k_total(const qln_dims& D) { return (int64_t)D.B * (D.N - 1) * QLN_TRACK_NU * QLN_NX; }
int64_t tracking_p_total(const qln_dims& D) { return (int64_t)D.B * D.N * QLN_TRACK_P_NNZ; }
int64_t tracking_marg_total(const qln_dims& D) { return (int64_t)D.B * D.N * QLN_TRACK_MARG_STRIDE; }
int64_t tracking_sat_total(const qln_dims& D) { return (int64_t)D.B * (D.N - 1); }
int64_t tracking_gain_total(const qln_dims& D, int ny) { return (int64_t)D.B * D.N * QLN_NX * ny; }
int64_t tracking_meas_total(const qln_dims& D, int ny) { return (int64_t)D.B * D.N * ny; }

// The buffers of the host forms (qln_*_host), one per role.  A role's size follows from the role and the handle's layout
// (host_role_size): no form can allocate a buffer that another finds too small.  An in-out argument is copied in whole,
// padding included, so its role returns no out-only result: that padding would reach the next caller.
enum HostRole {
    kZ,      // in: the point Z / Zref (in-out of qln_solve_host)           layout of Z
    kV,      // in: a direction v, the vjp's Zout                           layout of Z
    kZbar,   // in: the vjp's cotangent Zbar                                layout of Z
    kZio,    // in-out: the roll-out's Zout, the vjp's Zref_bar, the jvp's Zout_dot  layout of Z
    kZdot,   // in: the jvp's tangent Zref_dot                              layout of Z
    kZout,   // out: H v, J' lam (padding zero)                             layout of Z
    kGrad,   // out: grad f                                                 layout of Z
    kC,      // out: c, J v (padding zero)                                  layout of c
    kMu,     // in: the multipliers mu / lam                                layout of c
    kVals,   // out: the Jacobian values                                    layout of vals
    kF,      // out: f                                                      [B]
    kSigma,  // in: sigma                                                   [B]
    kHvals,  // out: the Hessian values                                     (B-1) h_stride + nnz
    kK,      // out of the LQR, in to the roll-out and its vjp: the gains   [B][N-1][4][15]
    kKbar,   // out: the gains' cotangent                                   layout of K
    kKdot,   // in: the jvp's tangent K_dot                                 layout of K
    kP,      // out: the cost-to-go                                         [B][N][120]
    kX0,     // in: the roll-out's x0; out: the vjp's x0_bar, the design vjp's Wdiag_bar  [B][15]
    kCov0,   // in: the covariance sweep's Sigma0 (1 or B tiles used); out: the design vjp's Sigma0_bar  [B][120]
    kCov,    // out: the covariances                                        layout of P
    kMarg,   // out: the marginals                                          [B][N][8]
    kMultInfo,  // out: the multiplier estimate's report                    [B][16]
    kModel,  // in: the per-problem plant models                            [B][4]
    kModelD, // in: the model jvp's model_dot; out: the model vjp's model_bar  [B][4]
    kEvent,  // out: the guarded roll-out's touchdown records; in: the same for its sweeps  [B][8]
    kEventD, // out: the guarded jvp's event_dot                            [B][8]
    kEventVar,  // out: the guarded covariance sweep's event_var            [B][2]
    kSat,    // out: the limited roll-out's saturation codes; in: the same for its sweeps and gains  [B][N-1]
    kH,      // in: the Kalman filter's measurement matrix (ny rows used)   [8][15]
    kLgain,  // out: the filter gains ([B][N][15][ny] used)                 [B][N][15][8]
    kPest,   // out: the error covariances P^+; in: the design vjp's Pest_bar  layout of P
    kXhat0,  // in: the estimated roll-out's xhat0                          [B][15]
    kVnoise, // in: its measurement noise ([B][N][ny] used)                 [B][N][8]
    kWnoise, // in: its process noise                                       [B][N-1][15]
    kXhat,   // out: its estimates xhat_k|k                                 [B][N][15]
    kInnov,  // out: its innovations ([B][N][ny] used)                      [B][N][8]
    kEventHat,  // out: the estimator's touchdown records; in: the same for the sweeps  [B][8]
    kLgainD, // in: the estimated jvp's Lgain_dot; out: the vjp's Lgain_bar  layout of Lgain
    kXhatD,  // out: the estimated jvp's Xhat_dot; in: the vjp's Xhat_bar   [B][N][15]
    kInnovD, // out: the estimated jvp's innov_dot; in: the vjp's innov_bar  [B][N][8]
    kEventHatD,  // out: the estimated guarded jvp's event_hat_dot          [B][8]
    kXs,     // out: the smoother's states                                  [B][N][15]
    kPs,     // out: the smoother's covariances                             layout of P
    kZrec,   // in: the filter's recorded trajectory (control slots read)    layout of Z
    kY,      // in: the filter's measurements ([B][N][ny] used)             [B][N][8]
    kScore,  // out: the filter's {nis_k, log det S_k}                      [B][N][2]
    kLoglik, // out: the filter's log-likelihood; out / in: its sweeps' loglik_dot / loglik_bar  [B]
    kNisD,   // out: the filter jvp's nis_dot, the design jvp's logdet_dot; in: the vjps' nis_bar and logdet_bar  [B][N]
    kVbar,   // out: the design vjp's Vdiag_bar ([B][ny] used)              [B][8]
    kHostRoles
};

}  // namespace

struct qln_handle {
    int device = 0;
    qln_model model{};
    hipStream_t stream = nullptr;
    qln::BatchParams p{};
    qln_dims dims{};
    std::vector<int32_t> k_trans, init_mode;
    std::vector<int64_t> c_off, j_off;
    // device storage owned by the handle
    qln::ProblemDesc* d_desc = nullptr;
    double* d_bnd = nullptr;
    double* d_cost = nullptr;
    int64_t h_stride = 0;  // doubles between consecutive problems' Hessian segments (qln_hessian_layout)
    // the host forms' buffers by HostRole, allocated on first use and kept until qln_destroy: device memory (staged), or
    // -- zero_copy, small batches -- pinned host memory mapped into the device's address space, which the kernels read
    // and write directly, so that a callback is one launch and one synchronisation
    double* staged[kHostRoles] = {};
    struct Mapped {
        double* host = nullptr;
        double* dev = nullptr;
    };
    Mapped mapped[kHostRoles];
    bool zero_copy = false;
    std::vector<double> h_vals_one;  // one problem's Jacobian values, staged for the dense scatter
    // dense MOI scatter: per problem, where each value of the vals segment goes in the column-major matrix, and the
    // write-set's explicit zeros (built on first use)
    struct DenseMap {
        std::vector<int64_t> at, zeros;
    };
    std::vector<DenseMap> dense_map;
    // buffers handed out by qln_vals_alloc_placed
    struct Placed {
        char* va = nullptr;        // reserved virtual range
        size_t va_size = 0;        // bytes reserved at va
        size_t chunk = 0;
        size_t first = 0;          // first chunk still mapped
        size_t scanned = 0;        // chunks the placement scan looked at
        std::vector<hipMemGenericAllocationHandle_t> chunks;  // the mapped ones, in order
        double* vals = nullptr;
    };
    std::vector<Placed> placed;
    // scratch of qln_solve (step blocks of every knot), allocated on first use
    double* solve_scratch = nullptr;
    size_t solve_scratch_n = 0;
};

namespace {

template <class T>
int upload(T** dst, const T* src, size_t n) {
    QLN_HIP(hipMalloc(reinterpret_cast<void**>(dst), std::max<size_t>(n, 1) * sizeof(T)));
    if (n) QLN_HIP(hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
    return QLN_OK;
}

int64_t host_role_size(const qln_handle* h, HostRole r) {
    const qln_dims& D = h->dims;
    switch (r) {
        case kZ: case kV: case kZbar: case kZio: case kZdot: case kZout: case kGrad: case kZrec: return D.z_total;
        case kC: case kMu: return D.c_total;
        case kVals: return D.j_total;
        case kF: case kSigma: case kLoglik: return D.B;
        case kHvals: return (int64_t)(D.B - 1) * h->h_stride + hessian_nnz(D.N);  // no padding behind the last problem
        case kK: case kKbar: case kKdot: return tracking_k_total(D);
        case kP: case kCov: case kPest: case kPs: return tracking_p_total(D);
        case kCov0: return (int64_t)D.B * QLN_TRACK_P_NNZ;
        case kMarg: return tracking_marg_total(D);
        case kX0: case kXhat0: return (int64_t)D.B * QLN_NX;
        case kMultInfo: return (int64_t)D.B * QLN_MULT_INFO_STRIDE;
        case kModel: case kModelD: return (int64_t)D.B * QLN_MODEL_NP;
        case kEvent: case kEventD: case kEventHat: case kEventHatD: return (int64_t)D.B * QLN_TOUCHDOWN_INFO_STRIDE;
        case kEventVar: return (int64_t)D.B * 2;
        case kSat: return tracking_sat_total(D);
        case kH: return (int64_t)QLN_TRACK_NY_MAX * QLN_NX;
        case kLgain: case kLgainD: return tracking_gain_total(D, QLN_TRACK_NY_MAX);
        case kVnoise: case kInnov: case kInnovD: case kY: return tracking_meas_total(D, QLN_TRACK_NY_MAX);
        case kScore: return (int64_t)D.B * D.N * 2;
        case kNisD: return (int64_t)D.B * D.N;
        case kVbar: return (int64_t)D.B * QLN_TRACK_NY_MAX;
        case kWnoise: return (int64_t)D.B * (D.N - 1) * QLN_NX;
        case kXhat: case kXhatD: case kXs: return (int64_t)D.B * D.N * QLN_NX;
        case kHostRoles: break;
    }
    return 0;
}

// The role's buffer, mapped or in device memory, allocated on first use and zero-filled: the padding the kernels never
// write comes back as zeros, not stale memory.
int acquire(qln_handle* h, HostRole r, bool mapped) {
    const size_t bytes = std::max<int64_t>(host_role_size(h, r), 1) * sizeof(double);
    if (!mapped) {
        double*& buf = h->staged[r];
        if (buf) return QLN_OK;
        QLN_HIP(hipMalloc(reinterpret_cast<void**>(&buf), bytes));
        QLN_HIP(hipMemset(buf, 0, bytes));
        return QLN_OK;
    }
    qln_handle::Mapped& m = h->mapped[r];
    if (m.host) return QLN_OK;
    void* hp = nullptr;
    QLN_HIP(hipHostMalloc(&hp, bytes, hipHostMallocMapped));
    std::memset(hp, 0, bytes);
    void* dp = nullptr;
    if (hipError_t e = hipHostGetDevicePointer(&dp, hp, 0); e != hipSuccess) {
        (void)hipHostFree(hp);
        return fail(QLN_ERR_HIP, std::string("hipHostGetDevicePointer: ") + hipGetErrorString(e));
    }
    m.host = static_cast<double*>(hp);
    m.dev = static_cast<double*>(dp);
    return QLN_OK;
}

// One argument of an entry point, declared once for both memory forms: `n` doubles at `at` in its role's buffer (n < 0: the
// whole buffer).  Its direction is which of src and dst is given: in, out, or both.  Neither given: an optional argument the
// caller left NULL -- no buffer, no copy, it overlaps nothing, and the launch sees NULL.  view (out only): set to where the
// results can be read, the mapped buffer itself (then nothing is copied to dst) or dst.  ruled: the overlap rule looks at it.
// staged: the host form stages it; where it does not, the launch sees NULL in the host form and lets another buffer stand in.
struct HostArg {
    HostRole role;
    const double* src;
    double* dst;
    int64_t n, at;
    const double** view;
    bool ruled = true, staged = true;
    HostArg sized(int64_t count) const { HostArg a = *this; a.n = count; return a; }
    HostArg ruled_if(bool on) const { HostArg a = *this; a.ruled = on; return a; }
    HostArg staged_if(bool on) const { HostArg a = *this; a.staged = on; return a; }
    bool passed() const { return src || dst; }
};
using HostArgs = std::initializer_list<HostArg>;
HostArg copy_in(HostRole r, const double* p) { return {r, p, nullptr, -1, 0, nullptr}; }
HostArg copy_out(HostRole r, double* p) { return {r, nullptr, p, -1, 0, nullptr}; }
HostArg copy_inout(HostRole r, double* p) { return {r, p, p, -1, 0, nullptr}; }

int64_t host_arg_size(const qln_handle* h, const HostArg& a) { return a.n < 0 ? host_role_size(h, a.role) : a.n; }

// The one staging path of the host forms.  Mapped (h->zero_copy, unless the form passes may_map = false) or staged, it
// acquires every passed argument's buffer, copies the inputs in, calls launch(d, mapped) with d[role] the device-visible
// buffer of each passed argument (NULL for the rest), copies the outputs back and synchronises the stream once.
template <class Launch>
int host_call(qln_handle* h, HostArgs args, Launch&& launch, bool may_map = true) {
    const bool mapped = may_map && h->zero_copy;
    auto bytes = [&](const HostArg& a) { return host_arg_size(h, a) * sizeof(double); };
    double* d[kHostRoles] = {};
    for (const HostArg& a : args)
        if (a.passed() && a.staged) {
            if (int rc = acquire(h, a.role, mapped)) return rc;
            d[a.role] = mapped ? h->mapped[a.role].dev : h->staged[a.role];
        }
    for (const HostArg& a : args) {
        if (!a.src || !a.staged) continue;
        if (mapped) std::memcpy(h->mapped[a.role].host + a.at, a.src, bytes(a));
        else QLN_HIP(hipMemcpyAsync(d[a.role] + a.at, a.src, bytes(a), hipMemcpyHostToDevice, h->stream));
    }
    QLN_HIP(launch(d, mapped));
    if (!mapped)
        for (const HostArg& a : args)
            if (a.dst) QLN_HIP(hipMemcpyAsync(a.dst, d[a.role] + a.at, bytes(a), hipMemcpyDeviceToHost, h->stream));
    QLN_HIP(hipStreamSynchronize(h->stream));
    for (const HostArg& a : args) {
        if (!a.dst) continue;
        const double* v = mapped ? h->mapped[a.role].host + a.at : a.dst;
        if (a.view) *a.view = v;
        else if (mapped) std::memcpy(a.dst, v, bytes(a));
    }
    return QLN_OK;
}

int check_handle(const qln_handle* h) {
    if (!h) return fail(QLN_ERR_INVALID_ARGUMENT, "null handle");
    return QLN_OK;
}

int bind_device(const qln_handle* h) {
    QLN_HIP(hipSetDevice(h->device));
    return QLN_OK;
}

// The two memory forms of an entry point: the caller's pointers are device memory, or host memory (qln_*_host).
enum MemForm { kDeviceMem, kHostMem };

// Runs one operation on its argument table.  Host form: host_call.  Device form: d[role] is the caller's own pointer of
// every passed argument, staged by the host form or not, then the one launch -- no copy and no synchronisation.
template <class Launch>
int run_call(qln_handle* h, MemForm mem, HostArgs args, Launch&& launch) {
    if (int rc = bind_device(h)) return rc;
    if (mem == kHostMem) return host_call(h, args, launch);
    double* d[kHostRoles] = {};
    for (const HostArg& a : args)
        if (a.passed()) d[a.role] = a.dst ? a.dst : const_cast<double*>(a.src);
    QLN_HIP(launch(d, false));
    return QLN_OK;
}

}  // namespace

extern "C" {

const char* qln_last_error(void) { return g_err.c_str(); }
int qln_set_last_error(int code, const char* msg) { return fail(code, msg ? msg : ""); }
const char* qln_version(void) { return "quadruped_landing_amd 0.1 (gfx950)"; }

// Argument checks and the layout of a batch (sizes, per-problem offsets): everything qln_create decides before it touches
// a device.  c_off / j_off: [B] or null.
static int layout_of(const qln_batch_desc* d, const char* who, bool need_states, qln_dims* D, int64_t* c_off, int64_t* j_off) {
    const std::string w = std::string(who) + ": ";
    if (d->B < 1) return fail(QLN_ERR_INVALID_ARGUMENT, w + "B must be >= 1");
    if (d->N < 2) return fail(QLN_ERR_INVALID_ARGUMENT, w + "N must be >= 2");
    if (d->N > 50000000 / 20) return fail(QLN_ERR_INVALID_ARGUMENT, w + "N too large for 32-bit indices");
    if (!d->k_trans || !d->init_mode || (need_states && (!d->x0 || !d->xf)))
        return fail(QLN_ERR_INVALID_ARGUMENT, w + "null descriptor array");
    if (d->cost_batch != 1 && d->cost_batch != d->B)
        return fail(QLN_ERR_INVALID_ARGUMENT, w + "cost_batch must be 1 or B");
    const int32_t n_nlp = 20 * d->N - 5;
    const int64_t z_stride = d->z_stride ? d->z_stride : n_nlp;
    if (z_stride < n_nlp) return fail(QLN_ERR_INVALID_ARGUMENT, w + "z_stride < n_nlp");
    const int64_t align = d->align ? d->align : 16;
    if (align < 1) return fail(QLN_ERR_INVALID_ARGUMENT, w + "align must be >= 1");
    const int32_t fmt = d->jac_format;
    if (fmt != QLN_JAC_FORMAT_DENSE_BLOCKS && fmt != QLN_JAC_FORMAT_STRUCTURAL)
        return fail(QLN_ERR_INVALID_ARGUMENT, w + "unknown jac_format");
    for (int32_t b = 0; b < d->B; ++b) {
        if (d->k_trans[b] < 1 || d->k_trans[b] > d->N + 1)
            return fail(QLN_ERR_INVALID_ARGUMENT, w + "k_trans out of range [1, N+1] at problem " + std::to_string(b));
        if (d->init_mode[b] != 1 && d->init_mode[b] != 2)
            return fail(QLN_ERR_INVALID_ARGUMENT, w + "init_mode must be 1 or 2 at problem " + std::to_string(b));
    }
    const int64_t jalign = (align % 2) ? align * 2 : align;  // keep j_off even: 16-byte stores
    int64_t co = 0, jo = 0;
    int32_t m_max = 0, nnz_max = 0, dyn_max = 0;
    for (int32_t b = 0; b < d->B; ++b) {
        const int32_t m = m_nlp_of(d->N, d->k_trans[b]), nz = nnz_of(d->N, d->k_trans[b], fmt);
        dyn_max = std::max(dyn_max, nnz_dyn_of(d->N, d->k_trans[b], fmt));
        co = round_up(co, align);
        jo = round_up(jo, jalign);
        if (c_off) c_off[b] = co;
        if (j_off) j_off[b] = jo;
        co += m;   // no padding behind the last problem: for B == 1 the totals are exactly m_nlp / nnz,
        jo += nz;  // so Ipopt-owned buffers of the reference's sizes can be passed as they are
        m_max = std::max(m_max, m);
        nnz_max = std::max(nnz_max, nz);
    }
    D->B = d->B;
    D->N = d->N;
    D->n_nlp = n_nlp;
    D->m_nlp_max = m_max;
    D->nnz_max = nnz_max;
    D->nnz_dynamic = dyn_max;
    D->z_stride = z_stride;
    D->z_total = z_stride * (int64_t)d->B;
    D->c_total = co;
    D->j_total = jo;
    return QLN_OK;
}

int qln_layout(const qln_batch_desc* d, qln_dims* dims, int64_t* c_off, int64_t* j_off) {
    if (!d || !dims) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_layout: null argument");
    return layout_of(d, "qln_layout", false, dims, c_off, j_off);
}

int qln_create(const qln_batch_desc* d, int device, qln_handle** out) {
    if (!d || !out) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_create: null argument");
    *out = nullptr;
    qln_dims lay{};
    std::vector<int64_t> c_off((size_t)std::max(d->B, 0)), j_off((size_t)std::max(d->B, 0));
    if (int rc = layout_of(d, "qln_create", true, &lay, c_off.data(), j_off.data())) return rc;
    const int64_t z_stride = lay.z_stride;
    const int32_t fmt = d->jac_format;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(QLN_ERR_NO_DEVICE, "qln_create: no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_create: bad device ordinal");

    qln_handle* h = new (std::nothrow) qln_handle();
    if (!h) return fail(QLN_ERR_HIP, "qln_create: out of host memory");
    h->device = device;
    h->model = d->model;
    h->k_trans.assign(d->k_trans, d->k_trans + d->B);
    h->init_mode.assign(d->init_mode, d->init_mode + d->B);
    h->c_off = std::move(c_off);
    h->j_off = std::move(j_off);
    h->dims = lay;
    qln_dims& D = h->dims;
    h->h_stride = hessian_stride(d->N, d->align);

    int rc = QLN_OK;
    auto bail = [&](int code) {
        qln_destroy(h);
        return code;
    };
    if (hipSetDevice(device) != hipSuccess) return bail(fail(QLN_ERR_HIP, "hipSetDevice failed"));
    {
        // one 32-byte descriptor record and one 30-double boundary record per problem
        std::vector<qln::ProblemDesc> desc((size_t)d->B);
        std::vector<double> bnd((size_t)d->B * 30);
        for (int32_t b = 0; b < d->B; ++b) {
            desc[b].k_trans = d->k_trans[b];
            desc[b].init_mode = d->init_mode[b];
            desc[b].c_off = h->c_off[b];
            desc[b].j_off = h->j_off[b];
            desc[b].reserved = 0;
            std::memcpy(&bnd[(size_t)b * 30], d->x0 + (size_t)b * 15, 15 * sizeof(double));
            std::memcpy(&bnd[(size_t)b * 30 + 15], d->xf + (size_t)b * 15, 15 * sizeof(double));
        }
        if ((rc = upload(&h->d_desc, desc.data(), desc.size()))) return bail(rc);
        if ((rc = upload(&h->d_bnd, bnd.data(), bnd.size()))) return bail(rc);
    }
    if (d->cost && (rc = upload(&h->d_cost, d->cost, (size_t)d->cost_batch * d->N * QLN_COST_STRIDE))) return bail(rc);

    qln::BatchParams& P = h->p;
    P.B = d->B;
    P.N = d->N;
    P.g = d->model.g;
    P.mb = d->model.mb;
    P.mf = d->model.mf;
    P.lb = d->model.lb;
    P.desc = h->d_desc;
    P.bnd = h->d_bnd;
    P.cost = h->d_cost;
    P.cost_batch = d->cost_batch;
    P.z_stride = z_stride;
    P.jac_format = fmt;
    P.kt_max = *std::max_element(d->k_trans, d->k_trans + d->B);
    // host-pointer (MOI) mode: up to 8 MB per callback the kernels work on mapped host memory directly (one launch, no
    // copies: 19-21 us against 32 us for the notebook's problem, profiles/r01_moi_latency.txt); larger batches are
    // staged through device memory
    h->zero_copy = (D.z_total + D.c_total + D.j_total) * (int64_t)sizeof(double) <= ((int64_t)8 << 20);
    *out = h;
    return QLN_OK;
}

// Gives a placed buffer back: unmap every chunk still mapped, release the physical handles, free the virtual range.
// The caller has synchronised the DEVICE (not just the handle's stream: the buffer was handed out as plain memory, so
// work on any stream -- torch's current one, a stream set later with qln_set_stream -- may have touched it).  Every
// return code is looked at; the first failure is reported through qln_last_error and the rest is still attempted.
static int release_placed(qln_handle::Placed& p) {
    hipError_t first = hipSuccess;
    const char* what = nullptr;
    auto note = [&](hipError_t e, const char* w) {
        if (e != hipSuccess && first == hipSuccess) {
            first = e;
            what = w;
        }
    };
    for (size_t i = 0; i < p.chunks.size(); ++i) {
        note(hipMemUnmap(p.va + (p.first + i) * p.chunk, p.chunk), "hipMemUnmap");
        note(hipMemRelease(p.chunks[i]), "hipMemRelease");
    }
    p.chunks.clear();
    if (p.va && kReturnVirtualRange) note(hipMemAddressFree(p.va, p.va_size), "hipMemAddressFree");
    p.va = nullptr;
    if (first != hipSuccess) return fail(QLN_ERR_HIP, std::string("releasing a placed buffer: ") + what + ": " + hipGetErrorString(first));
    return QLN_OK;
}

int qln_destroy(qln_handle* h) {
    if (!h) return QLN_OK;
    (void)hipSetDevice(h->device);
    int rc = QLN_OK;
    if (!h->placed.empty()) {
        // nothing on any stream may still be reading or writing memory about to be unmapped
        if (hipError_t e = hipDeviceSynchronize(); e != hipSuccess)
            rc = fail(QLN_ERR_HIP, std::string("qln_destroy: hipDeviceSynchronize: ") + hipGetErrorString(e));
        for (auto& p : h->placed)
            if (int r = release_placed(p); r != QLN_OK && rc == QLN_OK) rc = r;
    }
    for (const qln_handle::Mapped& m : h->mapped)
        if (m.host) (void)hipHostFree(m.host);
    for (double* b : h->staged)
        if (b) (void)hipFree(b);
    void* bufs[] = {h->d_desc, h->d_bnd, h->d_cost, h->solve_scratch};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    delete h;
    return rc;
}

int qln_set_stream(qln_handle* h, void* hip_stream) {
    if (int rc = check_handle(h)) return rc;
    h->stream = reinterpret_cast<hipStream_t>(hip_stream);
    return QLN_OK;
}

int qln_synchronize(qln_handle* h) {
    if (int rc = check_handle(h)) return rc;
    if (int rc = bind_device(h)) return rc;
    QLN_HIP(hipStreamSynchronize(h->stream));
    return QLN_OK;
}

int qln_get_dims(const qln_handle* h, qln_dims* out) {
    if (int rc = check_handle(h)) return rc;
    if (!out) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_get_dims: null out");
    *out = h->dims;
    return QLN_OK;
}

int qln_get_offsets(const qln_handle* h, int64_t* c_off, int64_t* j_off) {
    if (int rc = check_handle(h)) return rc;
    if (c_off) std::copy(h->c_off.begin(), h->c_off.end(), c_off);
    if (j_off) std::copy(h->j_off.begin(), h->j_off.end(), j_off);
    return QLN_OK;
}

static int check_problem(const qln_handle* h, int32_t b) {
    if (int rc = check_handle(h)) return rc;
    if (b < 0 || b >= h->dims.B) return fail(QLN_ERR_INVALID_ARGUMENT, "problem index out of range");
    return QLN_OK;
}

int qln_problem_dims(const qln_handle* h, int32_t b, int32_t* m_nlp, int32_t* nnz) {
    if (int rc = check_problem(h, b)) return rc;
    if (m_nlp) *m_nlp = m_nlp_of(h->dims.N, h->k_trans[b]);
    if (nnz) *nnz = nnz_of(h->dims.N, h->k_trans[b], h->p.jac_format);
    return QLN_OK;
}

int qln_problem_nnz_dynamic(const qln_handle* h, int32_t b, int32_t* nnz_dynamic) {
    if (int rc = check_problem(h, b)) return rc;
    if (!nnz_dynamic) return fail(QLN_ERR_INVALID_ARGUMENT, "null nnz_dynamic");
    *nnz_dynamic = nnz_dyn_of(h->dims.N, h->k_trans[b], h->p.jac_format);
    return QLN_OK;
}

int qln_constraint_index_ranges(const qln_handle* h, int32_t b, int32_t cinds[14]) {
    if (int rc = check_problem(h, b)) return rc;
    if (!cinds) return fail(QLN_ERR_INVALID_ARGUMENT, "null cinds");
    // 1-based inclusive ranges of the seven groups: a group ends where the next one starts
    const qln::RowLayout R = qln::row_layout(h->dims.N, h->k_trans[b]);
    const int32_t start[8] = {R.o_init, R.o_term, R.o_dyn, R.o_ci, R.o_co, R.o_fc, R.o_bp, R.m};
    for (int i = 0; i < 7; ++i) {
        cinds[2 * i] = start[i] + 1;
        cinds[2 * i + 1] = start[i + 1];
    }
    return QLN_OK;
}

int qln_constraint_bounds(const qln_handle* h, int32_t b, double* lb, double* ub) {
    // src/nlp.jl:66-69: lb = ub = 0 except ub[c_body_pos_inds] = Inf
    if (int rc = check_problem(h, b)) return rc;
    if (!lb || !ub) return fail(QLN_ERR_INVALID_ARGUMENT, "null bounds");
    const qln::RowLayout R = qln::row_layout(h->dims.N, h->k_trans[b]);
    for (int32_t i = 0; i < R.m; ++i) {
        lb[i] = 0.0;
        ub[i] = 0.0;
    }
    for (int32_t i = R.o_bp; i < R.m; ++i) ub[i] = std::numeric_limits<double>::infinity();
    return QLN_OK;
}

int qln_jacobian_structure(const qln_handle* h, int32_t b, int32_t* rows, int32_t* cols) {
    if (int rc = check_problem(h, b)) return rc;
    if (!rows || !cols) return fail(QLN_ERR_INVALID_ARGUMENT, "null rows/cols");
    const int32_t N = h->dims.N, kt = h->k_trans[b], im = h->init_mode[b];
    const qln::RowLayout R = qln::row_layout(N, kt);
    const qln::ValsLayout L = qln::vals_layout(N, kt, h->p.jac_format);
    const int32_t y_init = (im == 1) ? 4 : 6, y_other = (im == 1) ? 6 : 4;
    int64_t e = 0;
    auto put = [&](int32_t r, int32_t c) {
        rows[e] = r;
        cols[e] = c;
        ++e;
    };
    // each section must start where vals_layout, which the kernels write by, says it does; one that does not is this
    // function's bug, and is reported instead of handed out as a structure that disagrees with the values
    bool in_place = true;
    auto at = [&](int32_t section_start) { in_place = in_place && e == section_start; };
    const bool structural = (h->p.jac_format == QLN_JAC_FORMAT_STRUCTURAL);
    for (int32_t k = 0; k < N - 1; ++k) {  // D[ci, [xi[k]; ui[k]]], src/constraints.jl:186-198
        const int cat = qln::step_category(k + 1, kt, im);
        for (int32_t c = 0; c < 20; ++c)
            for (int32_t r = 0; r < 15; ++r)
                if (!structural || qln::step_entry_present(cat, r, c)) put(R.o_dyn + 15 * k + r, 20 * k + c);
    }
    at(L.o_clear);
    for (int32_t k = 0; k < N; ++k) put(R.o_bp + k, 20 * k + 2);       // :269-273
    at(L.o_init);
    for (int32_t c = 0; c < 15; ++c)                                    // :228
        for (int32_t r = 0; r < 15; ++r) put(R.o_init + r, c);
    at(L.o_term);
    for (int32_t c = 0; c < 15; ++c)                                    // :229
        for (int32_t r = 0; r < 14; ++r) put(R.o_term + r, 20 * (N - 1) + c);
    at(L.o_next);
    for (int32_t k = 0; k < N - 1; ++k)                                 // :200 (diagonal of -I(n))
        for (int32_t r = 0; r < 15; ++r) put(R.o_dyn + 15 * k + r, 20 * (k + 1) + r);
    at(L.o_ci);
    for (int32_t k = 0; k < N; ++k) put(R.o_ci + k, 20 * k + y_init);   // :235-243
    at(L.o_co);
    for (int32_t K = kt; K <= N; ++K) put(R.o_co + (K - kt), 20 * (K - 1) + y_other);  // :246-256
    at(L.o_fc);
    put(R.o_fc, 20 * (N - 2) + 16);                                     // :259
    put(R.o_fc, 20 * (N - 2) + 18);                                     // :260
    at(L.o_by);
    for (int32_t k = 0; k < N; ++k) put(R.o_bp + k, 20 * k + 1);        // :266
    at(L.nnz);
    if (!in_place) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_jacobian_structure: the sections written do not match vals_layout");
    return QLN_OK;
}

// ------------------------------------------------------------------ device-pointer mode

static int check_cost(const qln_handle* h) {
    if (!h->p.cost) return fail(QLN_ERR_INVALID_ARGUMENT, "no cost table: pass desc.cost or call qln_set_lqr_cost first");
    return QLN_OK;
}

int qln_set_lqr_cost(qln_handle* h, const double* Qdiag, const double* Rdiag, const double* Qfdiag, double dt,
                     int per_problem) {
    if (int rc = check_handle(h)) return rc;
    if (!Qdiag || !Rdiag || !Qfdiag) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_set_lqr_cost: null weights");
    if (int rc = bind_device(h)) return rc;
    const int32_t cb = per_problem ? h->dims.B : 1;
    double w[35];
    std::memcpy(w, Qdiag, 15 * sizeof(double));
    std::memcpy(w + 15, Rdiag, 5 * sizeof(double));
    std::memcpy(w + 20, Qfdiag, 15 * sizeof(double));
    double* d_w = nullptr;
    double* d_cost = nullptr;
    QLN_HIP(hipMalloc(reinterpret_cast<void**>(&d_w), sizeof(w)));
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d_cost), (size_t)cb * h->dims.N * QLN_COST_STRIDE * sizeof(double));
    if (e == hipSuccess) e = hipMemcpyAsync(d_w, w, sizeof(w), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = qln::launch_lqr_cost(h->p, d_w, dt, d_cost, cb, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(d_w);
    if (e != hipSuccess) {
        if (d_cost) (void)hipFree(d_cost);
        return fail(QLN_ERR_HIP, std::string("qln_set_lqr_cost: ") + hipGetErrorString(e));
    }
    if (h->d_cost) (void)hipFree(h->d_cost);
    h->d_cost = d_cost;
    h->p.cost = d_cost;
    h->p.cost_batch = cb;
    return QLN_OK;
}

int qln_get_cost(qln_handle* h, double* cost_host, int32_t* cost_batch) {
    if (int rc = check_handle(h)) return rc;
    if (int rc = check_cost(h)) return rc;
    if (cost_batch) *cost_batch = h->p.cost_batch;
    if (!cost_host) return QLN_OK;
    if (int rc = bind_device(h)) return rc;
    QLN_HIP(hipMemcpy(cost_host, h->p.cost, (size_t)h->p.cost_batch * h->dims.N * QLN_COST_STRIDE * sizeof(double),
                      hipMemcpyDeviceToHost));
    return QLN_OK;
}

int qln_eval_objective(qln_handle* h, const double* Z, double* f) {
    if (int rc = check_handle(h)) return rc;
    if (int rc = check_cost(h)) return rc;
    if (!Z || !f) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_eval_objective: null pointer");
    if (int rc = bind_device(h)) return rc;
    QLN_HIP(qln::launch_objective(h->p, Z, f, h->stream));
    return QLN_OK;
}

int qln_eval_objective_gradient(qln_handle* h, const double* Z, double* grad) {
    if (int rc = check_handle(h)) return rc;
    if (int rc = check_cost(h)) return rc;
    if (!Z || !grad) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_eval_objective_gradient: null pointer");
    if (int rc = bind_device(h)) return rc;
    QLN_HIP(qln::launch_objective_gradient(h->p, Z, grad, h->stream));
    return QLN_OK;
}

int qln_eval_constraint(qln_handle* h, const double* Z, double* c) {
    if (int rc = check_handle(h)) return rc;
    if (!Z || !c) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_eval_constraint: null pointer");
    if (int rc = bind_device(h)) return rc;
    QLN_HIP(qln::launch_constraint_jacobian(h->p, 0, h->p.B, Z, c, nullptr, 0, h->stream));
    return QLN_OK;
}

static int check_vals(const double* vals) {
    if (!vals) return fail(QLN_ERR_INVALID_ARGUMENT, "null vals");
    if (reinterpret_cast<uintptr_t>(vals) % 16) return fail(QLN_ERR_INVALID_ARGUMENT, "vals must be 16-byte aligned");
    return QLN_OK;
}

int qln_eval_constraint_jacobian(qln_handle* h, const double* Z, double* vals, uint32_t flags) {
    if (int rc = check_handle(h)) return rc;
    if (!Z) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_eval_constraint_jacobian: null Z");
    if (int rc = check_vals(vals)) return rc;
    if (int rc = bind_device(h)) return rc;
    QLN_HIP(qln::launch_constraint_jacobian(h->p, 0, h->p.B, Z, nullptr, vals, flags & QLN_JAC_WRITE_CONSTANTS, h->stream));
    return QLN_OK;
}

int qln_eval_constraint_and_jacobian(qln_handle* h, const double* Z, double* c, double* vals, uint32_t flags) {
    if (int rc = check_handle(h)) return rc;
    if (!Z || !c) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_eval_constraint_and_jacobian: null pointer");
    if (int rc = check_vals(vals)) return rc;
    if (int rc = bind_device(h)) return rc;
    QLN_HIP(qln::launch_constraint_jacobian(h->p, 0, h->p.B, Z, c, vals, flags & QLN_JAC_WRITE_CONSTANTS, h->stream));
    return QLN_OK;
}

int qln_eval_all(qln_handle* h, const double* Z, double* f, double* grad, double* c, double* vals, uint32_t flags) {
    if (int rc = check_handle(h)) return rc;
    if (int rc = check_cost(h)) return rc;
    if (!Z || !f || !grad || !c) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_eval_all: null pointer");
    if (int rc = check_vals(vals)) return rc;
    if (int rc = bind_device(h)) return rc;
    QLN_HIP(qln::launch_eval_all(h->p, Z, f, grad, c, vals, flags & QLN_JAC_WRITE_CONSTANTS, h->stream));
    return QLN_OK;
}

int qln_eval_objective_and_constraint(qln_handle* h, const double* Z, double* f, double* c) {
    if (int rc = check_handle(h)) return rc;
    if (int rc = check_cost(h)) return rc;
    if (!Z || !f || !c) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_eval_objective_and_constraint: null pointer");
    if (int rc = bind_device(h)) return rc;
    QLN_HIP(qln::launch_objective_and_constraint(h->p, Z, f, c, h->stream));
    return QLN_OK;
}

int qln_jacobian_init_constants(qln_handle* h, double* vals) {
    if (int rc = check_handle(h)) return rc;
    if (int rc = check_vals(vals)) return rc;
    if (int rc = bind_device(h)) return rc;
    QLN_HIP(qln::launch_jacobian_constants(h->p, vals, h->stream));
    return QLN_OK;
}

int qln_eval_kinematic_constraint(qln_handle* h, const double* Z, double* d, double* jac) {
    if (int rc = check_handle(h)) return rc;
    if (!Z || !d) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_eval_kinematic_constraint: null pointer");
    if (int rc = bind_device(h)) return rc;
    QLN_HIP(qln::launch_kinematic_rows(h->p, Z, d, jac, h->stream));
    return QLN_OK;
}

int qln_kinematic_bounds(const qln_handle* h, double* lower, double* upper) {
    if (int rc = check_handle(h)) return rc;
    if (!lower || !upper) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_kinematic_bounds: null pointer");
    *lower = 0.0;
    *upper = h->model.l1 + h->model.l2 + h->model.lb / 2;  // src/nlp.jl:70 (commented out there)
    return QLN_OK;
}

int qln_eval_friction_cone(qln_handle* h, const double* Z, double mu, double* d, double* jac) {
    if (int rc = check_handle(h)) return rc;
    if (!Z || !d) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_eval_friction_cone: null pointer");
    if (!(mu > 0.0) || !std::isfinite(mu)) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_eval_friction_cone: mu must be positive and finite");
    if (int rc = bind_device(h)) return rc;
    QLN_HIP(qln::launch_friction_rows(h->p, Z, mu, d, jac, h->stream));
    return QLN_OK;
}

int qln_constraint_violation(qln_handle* h, const double* c, double* viol) {
    if (int rc = check_handle(h)) return rc;
    if (!c || !viol) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_constraint_violation: null pointer");
    if (int rc = bind_device(h)) return rc;
    QLN_HIP(qln::launch_constraint_violation(h->p, c, viol, h->stream));
    return QLN_OK;
}

int qln_eval_constraint_jvp(qln_handle* h, const double* Z, const double* v, double* y) {
    if (int rc = check_handle(h)) return rc;
    if (!Z || !v || !y) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_eval_constraint_jvp: null pointer");
    if (int rc = bind_device(h)) return rc;
    QLN_HIP(qln::launch_constraint_jvp(h->p, Z, v, y, h->stream));
    return QLN_OK;
}

int qln_eval_constraint_vjp(qln_handle* h, const double* Z, const double* lam, double* g) {
    if (int rc = check_handle(h)) return rc;
    if (!Z || !lam || !g) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_eval_constraint_vjp: null pointer");
    if (int rc = bind_device(h)) return rc;
    QLN_HIP(qln::launch_constraint_vjp(h->p, Z, lam, g, h->stream));
    return QLN_OK;
}

int qln_gauss_newton_step(qln_handle* h, const double* Z, const double* c, double* dZ, int32_t max_iters, double rel_tol,
                          const double* radius, const double* col_scale, double* info) {
    if (int rc = check_handle(h)) return rc;
    if (!Z || !c || !dZ) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_gauss_newton_step: null pointer");
    if (max_iters < 0 || !(rel_tol >= 0.0)) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_gauss_newton_step: bad max_iters / rel_tol");
    if (qln::gauss_newton_lds_bytes(h->dims.N) > 160 * 1024)
        return fail(QLN_ERR_UNSUPPORTED, "qln_gauss_newton_step: N = " + std::to_string(h->dims.N) +
                                             " does not fit one problem in the 160 KB of LDS of a CU (N <= 149)");
    if (int rc = bind_device(h)) return rc;
    QLN_HIP(qln::launch_gauss_newton_step(h->p, Z, c, dZ, max_iters, rel_tol, radius, col_scale, info, h->stream));
    return QLN_OK;
}

int qln_solve_default_options(qln_solve_options* o) {
    if (!o) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_solve_default_options: null");
    // Inexact inner solves: a few iLQR iterations per multiplier update, a gentle penalty growth.  Measured on 16 384
    // random N = 40 problems (profiles/r02_solve_sweep_options.txt): 60 inner iterations and rho x10 from 1 take a median
    // of 214 iterations; 8 inner iterations and rho x5 from 10 solve the same 16 384 with a median of 75 (max 144).
    o->max_outer = 80;
    o->max_inner = 6;
    o->tol_violation = 1e-6;
    o->inner_tol = 1e-7;
    o->rho0 = 3.0;
    o->rho_factor = 5.0;
    o->rho_max = 1e8;
    o->h_min = 0.001;   // src/moi.jl:59-60
    o->h_max = 0.02;
    o->theta_min = -M_PI / 2;  // src/moi.jl:55-56
    o->theta_max = M_PI / 2;
    o->q6_bounds = 1;
    o->exact_h_gradient = 0;
    o->h_prox = 1e4;
    o->rescue_outer = 20;
    return QLN_OK;
}

int qln_variable_bounds(int32_t N, const qln_solve_options* opt, double* x_l, double* x_u) {
    if (N < 2) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_variable_bounds: N must be >= 2");
    if (!x_l || !x_u) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_variable_bounds: null output");
    qln_solve_options o;
    qln_solve_default_options(&o);
    if (opt) o = *opt;
    const int64_t n_nlp = 20 * (int64_t)N - 5;
    for (int64_t i = 0; i < n_nlp; ++i) {
        x_l[i] = -HUGE_VAL;
        x_u[i] = HUGE_VAL;
    }
    for (int32_t k = 0; k < N; ++k) {  // 0-based knot; the reference's indices are 1-based, k = 1..N
        x_l[20 * k + 2] = o.theta_min;  // src/moi.jl:55-56
        x_u[20 * k + 2] = o.theta_max;
        if (k < N - 1) {
            x_l[20 * k + 19] = o.h_min;  // src/moi.jl:59-60
            x_u[20 * k + 19] = o.h_max;
            if (o.q6_bounds) {           // src/moi.jl:64-65: 22+20(k-1), 24+20(k-1) 1-based = yb_{k+1}, x1_{k+1} (quirk Q6)
                x_l[20 * k + 21] = 0.0;
                x_l[20 * k + 23] = 0.0;
            }
        }
    }
    return QLN_OK;
}

int qln_solve(qln_handle* h, double* Z, const qln_solve_options* opt, double* info) {
    if (int rc = check_handle(h)) return rc;
    if (int rc = check_cost(h)) return rc;
    if (!Z) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_solve: null Z");
    qln_solve_options o;
    qln_solve_default_options(&o);
    if (opt) o = *opt;
    if (o.max_outer < 0 || o.max_inner < 1 || !(o.tol_violation > 0) || !(o.rho0 > 0) || !(o.rho_factor > 1) || !(o.rho_max >= o.rho0) ||
        !(o.h_min > 0) || !(o.h_max >= o.h_min) || !(o.theta_max > o.theta_min) || !(o.inner_tol >= 0) ||
        !(o.h_prox >= 0) || o.rescue_outer < 0)
        return fail(QLN_ERR_INVALID_ARGUMENT, "qln_solve: bad options");
    if (qln::ilqr_lds_bytes(h->dims.N) > 160 * 1024)
        return fail(QLN_ERR_UNSUPPORTED, "qln_solve: N = " + std::to_string(h->dims.N) + " does not fit one problem in the 160 KB of LDS of a CU");
    if (int rc = bind_device(h)) return rc;
    const size_t need = qln::ilqr_scratch_doubles(h->dims.B, h->dims.N);
    if (h->solve_scratch_n < need) {
        if (h->solve_scratch) {
            QLN_HIP(hipStreamSynchronize(h->stream));
            QLN_HIP(hipFree(h->solve_scratch));
            h->solve_scratch = nullptr;
            h->solve_scratch_n = 0;
        }
        QLN_HIP(hipMalloc(reinterpret_cast<void**>(&h->solve_scratch), need * sizeof(double)));
        h->solve_scratch_n = need;
    }
    qln::SolveParams sp;
    sp.max_outer = o.max_outer;
    sp.max_inner = o.max_inner;
    sp.tol = o.tol_violation;
    sp.inner_tol = o.inner_tol;
    sp.rho0 = o.rho0;
    sp.rho_factor = o.rho_factor;
    sp.rho_max = o.rho_max;
    sp.mu0 = 1e-6;
    sp.mu_min = 1e-8;
    sp.mu_max = 1e6;
    sp.h_lo = o.h_min;
    sp.h_hi = o.h_max;
    sp.th_lo = o.theta_min;
    sp.th_hi = o.theta_max;
    sp.h_prox = o.h_prox;
    sp.q6 = o.q6_bounds;
    sp.exact_h = o.exact_h_gradient;
    sp.rescue_outer = o.rescue_outer;
    QLN_HIP(qln::launch_al_ilqr(h->p, sp, Z, info, h->solve_scratch, h->stream));
    return QLN_OK;
}

// Everything qln_estimate_multipliers decides before it touches a device.
static int check_multiplier_args(const qln_handle* h, const double* Z, const double* c, const double* g,
                                 const qln_solve_options* bounds, double act_tol, double bound_tol, int32_t row_scaling,
                                 int32_t max_iters, double rel_tol, const double* lam, const char* who, qln::MultiplierParams* mp) {
    const std::string w = std::string(who) + ": ";
    if (int rc = check_handle(h)) return rc;
    if (!Z || !c || !g || !lam) return fail(QLN_ERR_INVALID_ARGUMENT, w + "null pointer");
    if (max_iters < 0) return fail(QLN_ERR_INVALID_ARGUMENT, w + "max_iters < 0");
    if (!(std::isfinite(act_tol) && act_tol >= 0.0 && std::isfinite(rel_tol) && rel_tol >= 0.0))
        return fail(QLN_ERR_INVALID_ARGUMENT, w + "act_tol and rel_tol must be finite and >= 0");
    if (!std::isfinite(bound_tol)) return fail(QLN_ERR_INVALID_ARGUMENT, w + "bound_tol must be finite");
    qln_solve_options o;
    qln_solve_default_options(&o);
    if (bounds) o = *bounds;
    if (!(o.h_max >= o.h_min) || !(o.theta_max >= o.theta_min)) return fail(QLN_ERR_INVALID_ARGUMENT, w + "bounds with min > max");
    if (qln::multiplier_lds_bytes(h->dims.N) > 160 * 1024)
        return fail(QLN_ERR_UNSUPPORTED, w + "N = " + std::to_string(h->dims.N) +
                                             " does not fit one problem in the 160 KB of LDS of a CU");
    mp->th_lo = o.theta_min, mp->th_hi = o.theta_max, mp->h_lo = o.h_min, mp->h_hi = o.h_max, mp->q6 = o.q6_bounds;
    mp->act_tol = act_tol, mp->bound_tol = bound_tol, mp->row_scaling = row_scaling, mp->max_iters = max_iters;
    mp->rel_tol = rel_tol;
    return QLN_OK;
}

int qln_estimate_multipliers(qln_handle* h, const double* Z, const double* c, const double* g, const qln_solve_options* bounds,
                             double act_tol, double bound_tol, int32_t row_scaling, int32_t max_iters, double rel_tol,
                             double* lam, double* lag, double* info) {
    qln::MultiplierParams mp;
    if (int rc = check_multiplier_args(h, Z, c, g, bounds, act_tol, bound_tol, row_scaling, max_iters, rel_tol, lam,
                                       "qln_estimate_multipliers", &mp))
        return rc;
    if (int rc = bind_device(h)) return rc;
    QLN_HIP(qln::launch_estimate_multipliers(h->p, mp, Z, c, g, lam, lag, info, h->stream));
    return QLN_OK;
}

// Staged only: a mapped path would keep the second read of g on the host link with no measurement behind it.
int qln_estimate_multipliers_host(qln_handle* h, const double* Z, const double* c, const double* g,
                                  const qln_solve_options* bounds, double act_tol, double bound_tol, int32_t row_scaling,
                                  int32_t max_iters, double rel_tol, double* lam, double* lag, double* info) {
    qln::MultiplierParams mp;
    if (int rc = check_multiplier_args(h, Z, c, g, bounds, act_tol, bound_tol, row_scaling, max_iters, rel_tol, lam,
                                       "qln_estimate_multipliers_host", &mp))
        return rc;
    if (int rc = bind_device(h)) return rc;
    return host_call(h, {copy_in(kZ, Z), copy_in(kMu, c), copy_in(kV, g), copy_out(kC, lam), copy_out(kZout, lag),
                         copy_out(kMultInfo, info)},
                     [&](double* const* d, bool) {
                         return qln::launch_estimate_multipliers(h->p, mp, d[kZ], d[kMu], d[kV], d[kC], d[kZout], d[kMultInfo],
                                                                 h->stream);
                     },
                     false);
}

static qln::DropStateSampler sampler_of(const qln_drop_state_sampler* s) {
    qln::DropStateSampler d;
    d.state_hi = s->pcg_state[0], d.state_lo = s->pcg_state[1];
    d.inc_hi = s->pcg_inc[0], d.inc_lo = s->pcg_inc[1];
    d.stream_offset = s->stream_offset;
    std::memcpy(d.x0_template, s->x0_template, sizeof d.x0_template);
    const double* r[4] = {s->theta_deg, s->y2, s->drop_height, s->omega};
    for (int a = 0; a < 4; ++a) {
        d.lo[a] = r[a][0];
        d.range[a] = r[a][1] - r[a][0];  // numpy: low + (high - low) * u
    }
    d.deg2rad = M_PI / 180.0;  // numpy.deg2rad: x * (pi / 180)
    d.two_g = s->two_g;
    return d;
}

int qln_sample_drop_states(qln_handle* h, const qln_drop_state_sampler* s) {
    if (int rc = check_handle(h)) return rc;
    if (!s) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_sample_drop_states: null sampler");
    if (s->stream_offset < 0) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_sample_drop_states: negative stream_offset");
    if (int rc = bind_device(h)) return rc;
    QLN_HIP(qln::launch_sample_drop_states(h->p, sampler_of(s), h->d_bnd, h->stream));
    return QLN_OK;
}

int qln_sample_bounded_integers(int device, const uint64_t pcg_state[2], const uint64_t pcg_inc[2], int64_t draw_offset, int32_t low,
                                int32_t high, int64_t count, int32_t* out, int64_t* rejected) {
    if (!pcg_state || !pcg_inc || !out || !rejected) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_sample_bounded_integers: null pointer");
    if (draw_offset < 0 || count < 0 || high <= low) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_sample_bounded_integers: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(QLN_ERR_NO_DEVICE, "qln_sample_bounded_integers: no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_sample_bounded_integers: bad device ordinal");
    *rejected = 0;
    if (count == 0) return QLN_OK;
    if ((int64_t)high - low == 1) {  // one possible value: numpy fills it in without touching the stream
        for (int64_t i = 0; i < count; ++i) out[i] = low;
        return QLN_OK;
    }
    QLN_HIP(hipSetDevice(device));
    qln::DropStateSampler d{};
    d.state_hi = pcg_state[0], d.state_lo = pcg_state[1];
    d.inc_hi = pcg_inc[0], d.inc_lo = pcg_inc[1];
    d.stream_offset = draw_offset;
    int32_t* d_out = nullptr;
    unsigned long long* d_rej = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d_out), (size_t)count * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_rej), sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(d_rej, 0, sizeof(unsigned long long));
    if (e == hipSuccess) e = qln::launch_bounded_integers(d, (uint32_t)((int64_t)high - low), low, count, d_out, d_rej, nullptr);
    unsigned long long rej = 0;
    if (e == hipSuccess) e = hipMemcpy(out, d_out, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(&rej, d_rej, sizeof rej, hipMemcpyDeviceToHost);
    if (d_out) (void)hipFree(d_out);
    if (d_rej) (void)hipFree(d_rej);
    if (e != hipSuccess) return fail(QLN_ERR_HIP, std::string("qln_sample_bounded_integers: ") + hipGetErrorString(e));
    *rejected = (int64_t)rej;
    return QLN_OK;
}

int qln_perturb_point(qln_handle* h, const qln_drop_state_sampler* s, double* Z, double sigma, double h_min, double h_max,
                      int redraw_h) {
    if (int rc = check_handle(h)) return rc;
    if (!s || !Z) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_perturb_point: null pointer");
    if (s->stream_offset < 0 || !(sigma >= 0) || !(h_max >= h_min)) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_perturb_point: bad argument");
    if (int rc = bind_device(h)) return rc;
    QLN_HIP(qln::launch_perturb_point(h->p, sampler_of(s), Z, sigma, h_min, h_max, redraw_h, h->stream));
    return QLN_OK;
}

int qln_get_boundary_states(qln_handle* h, double* x0, double* xf) {
    if (int rc = check_handle(h)) return rc;
    if (int rc = bind_device(h)) return rc;
    std::vector<double> bnd((size_t)h->dims.B * 30);
    QLN_HIP(hipStreamSynchronize(h->stream));
    QLN_HIP(hipMemcpy(bnd.data(), h->d_bnd, bnd.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int32_t b = 0; b < h->dims.B; ++b) {
        if (x0) std::memcpy(x0 + (size_t)b * 15, &bnd[(size_t)b * 30], 15 * sizeof(double));
        if (xf) std::memcpy(xf + (size_t)b * 15, &bnd[(size_t)b * 30 + 15], 15 * sizeof(double));
    }
    return QLN_OK;
}

int qln_solve_host(qln_handle* h, double* Z, const qln_solve_options* opt, double* info) {
    if (int rc = check_handle(h)) return rc;
    if (!Z) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_solve_host: null Z");
    if (int rc = bind_device(h)) return rc;
    if (int rc = acquire(h, kZ, false)) return rc;
    double* dZ = h->staged[kZ];
    double* d_info = nullptr;
    const size_t ninfo = (size_t)h->dims.B * QLN_SOLVE_INFO_STRIDE;
    if (info) QLN_HIP(hipMalloc(reinterpret_cast<void**>(&d_info), ninfo * sizeof(double)));
    int rc = QLN_OK;
    hipError_t e = hipMemcpyAsync(dZ, Z, h->dims.z_total * sizeof(double), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) rc = qln_solve(h, dZ, opt, d_info);
    if (e == hipSuccess && rc == QLN_OK) e = hipMemcpyAsync(Z, dZ, h->dims.z_total * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && rc == QLN_OK && info) e = hipMemcpyAsync(info, d_info, ninfo * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && rc == QLN_OK) e = hipStreamSynchronize(h->stream);
    if (d_info) (void)hipFree(d_info);
    if (rc != QLN_OK) return rc;
    if (e != hipSuccess) return fail(QLN_ERR_HIP, std::string("qln_solve_host: ") + hipGetErrorString(e));
    return QLN_OK;
}

int qln_initial_guess(qln_handle* h, double* Z) {
    if (int rc = check_handle(h)) return rc;
    if (!Z) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_initial_guess: null Z");
    for (int32_t b = 0; b < h->dims.B; ++b)
        if (h->k_trans[b] < 2)
            return fail(QLN_ERR_UNSUPPORTED, "qln_initial_guess: k_trans < 2 at problem " + std::to_string(b) +
                                                 " (the notebook's rule divides by k_trans - 1)");
    if (int rc = bind_device(h)) return rc;
    QLN_HIP(qln::launch_initial_guess(h->p, Z, h->stream));
    return QLN_OK;
}

// ------------------------------------------------------------------ Lagrangian Hessian

int qln_hessian_layout(const qln_batch_desc* d, int32_t* nnz, int64_t* h_stride) {
    if (!d || !nnz || !h_stride) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_hessian_layout: null argument");
    if (d->N < 2) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_hessian_layout: N must be >= 2");
    if (d->N > 50000000 / 20) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_hessian_layout: N too large for 32-bit indices");
    if (d->align < 0) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_hessian_layout: align must be >= 1");
    *nnz = hessian_nnz(d->N);
    *h_stride = hessian_stride(d->N, d->align);
    return QLN_OK;
}

int qln_hessian_structure(int32_t N, int32_t* rows, int32_t* cols) {
    if (N < 2) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_hessian_structure: N must be >= 2");
    if (N > 50000000 / 20) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_hessian_structure: N too large for 32-bit indices");
    if (!rows || !cols) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_hessian_structure: null pointer");
    int32_t rb[QLN_HESS_STEP_NNZ], cb[QLN_HESS_STEP_NNZ];
    int n = 0;
    for (int c = 0; c < 20; ++c)
        for (int r = c; r < 20; ++r)
            if (qln::hess_entry_present(r, c)) {
                rb[n] = r;
                cb[n] = c;
                ++n;
            }
    int64_t at = 0;
    for (int32_t k = 0; k < N - 1; ++k)
        for (int e = 0; e < QLN_HESS_STEP_NNZ; ++e, ++at) {
            rows[at] = 20 * k + rb[e];
            cols[at] = 20 * k + cb[e];
        }
    for (int i = 0; i < QLN_HESS_TERM_NNZ; ++i, ++at) rows[at] = cols[at] = 20 * (N - 1) + i;
    return QLN_OK;
}

static int check_hessian_args(const qln_handle* h, const double* Z, const double* mu, const double* hvals, const char* who) {
    if (int rc = check_handle(h)) return rc;
    if (int rc = check_cost(h)) return rc;
    if (!Z || !mu || !hvals) return fail(QLN_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
    if (reinterpret_cast<uintptr_t>(hvals) % 8) return fail(QLN_ERR_INVALID_ARGUMENT, std::string(who) + ": hvals must be 8-byte aligned");
    return QLN_OK;
}

int qln_eval_hessian_lagrangian(qln_handle* h, const double* Z, const double* sigma, const double* mu, double* hvals) {
    if (int rc = check_hessian_args(h, Z, mu, hvals, "qln_eval_hessian_lagrangian")) return rc;
    if (int rc = bind_device(h)) return rc;
    QLN_HIP(qln::launch_hessian_lagrangian(h->p, Z, sigma, mu, hvals, h->h_stride, h->stream));
    return QLN_OK;
}

static int check_hessian_product_args(const qln_handle* h, const double* Z, const double* mu, const double* v, const double* y,
                                      const char* who) {
    if (int rc = check_handle(h)) return rc;
    if (int rc = check_cost(h)) return rc;
    if (!Z || !mu || !v || !y) return fail(QLN_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
    return QLN_OK;
}

int qln_eval_hessian_lagrangian_product(qln_handle* h, const double* Z, const double* sigma, const double* mu, const double* v,
                                        double* y) {
    if (int rc = check_hessian_product_args(h, Z, mu, v, y, "qln_eval_hessian_lagrangian_product")) return rc;
    if (int rc = bind_device(h)) return rc;
    QLN_HIP(qln::launch_hessian_lagrangian_product(h->p, Z, sigma, mu, v, y, h->stream));
    return QLN_OK;
}

// ------------------------------------------------------------------ TVLQR tracking (qln_tracking_kernels.hip)

static int check_tracking_weights(const double* Q, const double* R, const double* Qf, const std::string& w) {
    if (!Q || !R || !Qf) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null weights");
    for (int i = 0; i < QLN_NX; ++i)
        if (!(std::isfinite(Q[i]) && Q[i] >= 0.0 && std::isfinite(Qf[i]) && Qf[i] >= 0.0))
            return fail(QLN_ERR_INVALID_ARGUMENT, w + ": Q and Qf must be finite and >= 0 (entry " + std::to_string(i) + ")");
    for (int i = 0; i < QLN_TRACK_NU; ++i)
        if (!(std::isfinite(R[i]) && R[i] > 0.0))
            return fail(QLN_ERR_INVALID_ARGUMENT, w + ": R must be finite and > 0 (entry " + std::to_string(i) + ")");
    return QLN_OK;
}

// The one overlap rule of the entry points, read from a call's argument table: no output -- an argument with a destination --
// may overlap an input or another output, each over its declared extent.  An argument left NULL, or declared outside the
// rule, overlaps nothing.
static int check_no_overlap(const qln_handle* h, HostArgs args, const std::string& w) {
    auto overlap = [&](const HostArg& a, const HostArg& b) {
        if (!a.ruled || !b.ruled || !a.passed() || !b.passed()) return false;
        const uintptr_t x = reinterpret_cast<uintptr_t>(a.dst ? a.dst : a.src);
        const uintptr_t y = reinterpret_cast<uintptr_t>(b.dst ? b.dst : b.src);
        return x < y + (uintptr_t)host_arg_size(h, b) * sizeof(double) && y < x + (uintptr_t)host_arg_size(h, a) * sizeof(double);
    };
    for (const HostArg& o : args) {
        if (!o.dst) continue;
        for (const HostArg& i : args)
            if (!i.dst && overlap(o, i)) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": an output overlaps an input");
        for (const HostArg& q : args)
            if (q.dst && &q != &o && overlap(o, q)) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": two outputs overlap");
    }
    return QLN_OK;
}

// host forms only: every entry finite, and mb, mf, lb > 0 (the device forms do not look at the values)
static int check_host_models(const qln_handle* h, const double* model, const char* who) {
    if (!model) return QLN_OK;
    for (int64_t b = 0; b < h->dims.B; ++b) {
        const double* th = model + b * QLN_MODEL_NP;
        for (int p = 0; p < QLN_MODEL_NP; ++p)
            if (!std::isfinite(th[p]) || (p > 0 && !(th[p] > 0.0)))
                return fail(QLN_ERR_INVALID_ARGUMENT, std::string(who) + ": model[" + std::to_string(b) + "][" + std::to_string(p) +
                                                          "] is not finite, or a mass or the body length is not positive");
    }
    return QLN_OK;
}

// host forms only: the knot an integer in [-1, N-2], tau finite and >= 0 (the device forms do not look at the values)
static int check_host_events(const qln_handle* h, const double* event, const char* who) {
    if (!event) return QLN_OK;
    for (int64_t b = 0; b < h->dims.B; ++b) {
        const double knot = event[b * QLN_TOUCHDOWN_INFO_STRIDE], tau = event[b * QLN_TOUCHDOWN_INFO_STRIDE + 1];
        if (!(knot >= -1.0 && knot <= (double)(h->dims.N - 2)) || knot != std::floor(knot))
            return fail(QLN_ERR_INVALID_ARGUMENT, std::string(who) + ": event[" + std::to_string(b) +
                                                      "][0] is not a knot of the roll-out (an integer in [-1, N-2])");
        if (!std::isfinite(tau) || tau < 0.0)
            return fail(QLN_ERR_INVALID_ARGUMENT,
                        std::string(who) + ": event[" + std::to_string(b) + "][1] (tau) is not finite or is negative");
    }
    return QLN_OK;
}

// host forms only: every entry of sat an integer code sum_m s_m 4^m with every digit s_m in {0, 1, 2} (the device forms do not
// look at the values)
static int check_host_sat(const qln_handle* h, const double* sat, const char* who) {
    if (!sat) return QLN_OK;
    const int64_t n1 = h->dims.N - 1;
    for (int64_t i = 0; i < tracking_sat_total(h->dims); ++i) {
        const double c = sat[i];
        bool ok = c >= 0.0 && c <= 170.0 && c == std::floor(c);
        for (int m = 0, v = ok ? (int)c : 0; ok && m < QLN_TRACK_NU; ++m, v >>= 2) ok = (v & 3) != 3;
        if (!ok)
            return fail(QLN_ERR_INVALID_ARGUMENT, std::string(who) + ": sat[" + std::to_string(i / n1) + "][" + std::to_string(i % n1) +
                                                      "] is not a saturation code (an integer with every base-4 digit in {0, 1, 2})");
    }
    return QLN_OK;
}

// host forms only: the ny rows of the measurement matrix finite (the device forms do not look at the values)
static int check_host_meas(const double* H, int32_t ny, const char* who) {
    for (int i = 0; i < ny * QLN_NX; ++i)
        if (!std::isfinite(H[i]))
            return fail(QLN_ERR_INVALID_ARGUMENT, std::string(who) + ": H is not finite (entry " + std::to_string(i) + ")");
    return QLN_OK;
}

// NaN, or lo > hi, in one of the four {lo, hi} pairs of the force limits (+-inf: no limit on that side)
static int check_force_limits(const double* lim, const char* who) {
    if (!lim) return fail(QLN_ERR_INVALID_ARGUMENT, std::string(who) + ": null lim");
    for (int i = 0; i < QLN_FORCE_LIMITS_N; i += 2)
        if (std::isnan(lim[i]) || std::isnan(lim[i + 1]) || lim[i] > lim[i + 1])
            return fail(QLN_ERR_INVALID_ARGUMENT, std::string(who) + ": lim[" + std::to_string(i) + "], lim[" + std::to_string(i + 1) +
                                                      "] is not a {lo, hi} pair (a NaN, or lo > hi)");
    return QLN_OK;
}

// host forms only: the values of every input that is a measurement matrix, a model, an event record or a saturation record,
// in the order of the table -- so a table's order is the precedence between two bad values.  An output or an in-out of these
// roles (the roll-outs' records) is no input; an input outside the overlap rule is still looked at.  H has ny rows: its
// declared extent over QLN_NX.
static int check_host_values(const qln_handle* h, HostArgs args, const char* who) {
    for (const HostArg& a : args) {
        if (!a.src || a.dst) continue;
        int rc = QLN_OK;
        if (a.role == kH) rc = check_host_meas(a.src, (int32_t)(host_arg_size(h, a) / QLN_NX), who);
        else if (a.role == kModel) rc = check_host_models(h, a.src, who);
        else if (a.role == kEvent || a.role == kEventHat) rc = check_host_events(h, a.src, who);
        else if (a.role == kSat) rc = check_host_sat(h, a.src, who);
        if (rc) return rc;
    }
    return QLN_OK;
}

// What every operation does after its own check: the overlap rule, in the host form the value checks, then the launch --
// all three read the one argument table.
extern "C++" {
template <class Launch>
static int run_tracking_call(qln_handle* h, MemForm mem, HostArgs args, const char* who, Launch&& launch) {
    if (int rc = check_no_overlap(h, args, who)) return rc;
    if (mem == kHostMem)
        if (int rc = check_host_values(h, args, who)) return rc;
    return run_call(h, mem, args, launch);
}
}

// The refusals that several operations share, each stated once; an operation's check calls them in the order its refusals
// have always had.
static int check_tracking_wdiag(const double* Wdiag, const std::string& w) {
    if (Wdiag)
        for (int i = 0; i < QLN_NX; ++i)
            if (!(std::isfinite(Wdiag[i]) && Wdiag[i] >= 0.0))
                return fail(QLN_ERR_INVALID_ARGUMENT, w + ": Wdiag must be finite and >= 0 (entry " + std::to_string(i) + ")");
    return QLN_OK;
}

static int check_tracking_ny(int32_t ny, const std::string& w) {
    if (ny < 1 || ny > QLN_TRACK_NY_MAX)
        return fail(QLN_ERR_INVALID_ARGUMENT, w + ": ny must be in [1, " + std::to_string(QLN_TRACK_NY_MAX) + "]");
    return QLN_OK;
}

static int check_tracking_vdiag(const double* Vdiag, int32_t ny, const std::string& w) {
    for (int i = 0; i < ny; ++i)
        if (!(std::isfinite(Vdiag[i]) && Vdiag[i] > 0.0))
            return fail(QLN_ERR_INVALID_ARGUMENT, w + ": Vdiag must be finite and > 0 (entry " + std::to_string(i) + ")");
    return QLN_OK;
}

// in two steps: at least 1 before the handle is looked at (h null), then 1 or the handle's B
static int check_sigma0_batch(int32_t sigma0_batch, const qln_handle* h, const std::string& w) {
    if (h ? sigma0_batch != 1 && sigma0_batch != h->dims.B : sigma0_batch < 1)
        return fail(QLN_ERR_INVALID_ARGUMENT, w + ": sigma0_batch must be 1 or B");
    return QLN_OK;
}

static int check_guard_event(bool guarded, const double* event, const std::string& w) {
    if (guarded && !event) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null event (the guarded roll-out's records)");
    return QLN_OK;
}

static int check_limited_sat(bool limited, const double* sat, const std::string& w) {
    if (limited && !sat) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null sat (the limited roll-out's saturation record)");
    return QLN_OK;
}

static int check_some_output(bool some, const std::string& w) {
    if (!some) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": every output is NULL (nothing to compute)");
    return QLN_OK;
}

// Every operation below is one argument struct, its builders, one check and one body for both memory forms.  The struct has a
// named field per argument.  A builder per prototype shape returns it value-initialised, so an optional the shape leaves out
// is null, and a small modifier adds what a guarded, a limited or a model form adds, with the flags that follow from it; an
// entry point is one call of the body on what they build, and the two memory forms of a pair differ in nothing but the form
// and the name.  (The sweeps of the filter and of the estimate-feedback roll-out also take the launch's own argument struct,
// qln::...JvpArgs / ...VjpArgs, which an entry point fills in the order of its prototype.)  The check holds what needs no
// device, in the order the refusals have always had.  The body declares the argument table once -- role, pointer, direction,
// extent, whether the overlap rule looks at it, whether the host form stages it -- and hands it to the runner: the rule, the
// host form's look at the values of H, a model, an event record and a saturation record, the staging and the launch all read
// that table (run_tracking_call).

// The Riccati sweep (k_tracking_lqr).  The entry point on the handle's knot schedule passes no model and no event, and the
// launch then takes the kernel without its kGuard flag.
// guarded: the sweep through the guard-triggered touchdown, which needs the roll-out's event records
// limited: the design at the limited roll-out's active set, which needs its saturation record sat; event then selects the
// guarded blocks, and without it the knot schedule's, which have no plant model
struct LqrCall {
    const double *Zref, *model, *event, *sat, *Q, *R, *Qf;
    double *K, *P;
    bool guarded, limited;
};

static int check_tracking_lqr_args(const qln_handle* h, const LqrCall& a, const char* who) {
    // the limited form's checks need no handle and come first
    if (int rc = check_limited_sat(a.limited, a.sat, who)) return rc;
    if (a.limited && !a.event && a.model)
        return fail(QLN_ERR_INVALID_ARGUMENT,
                    std::string(who) + ": model without event (the knot-scheduled design has no plant model)");
    if (int rc = check_handle(h)) return rc;
    if (!a.Zref || !a.K) return fail(QLN_ERR_INVALID_ARGUMENT, std::string(who) + ": null Zref or K");
    if (int rc = check_tracking_weights(a.Q, a.R, a.Qf, who)) return rc;
    return check_guard_event(!a.limited && a.guarded, a.event, who);
}

static int tracking_lqr(qln_handle* h, MemForm mem, const LqrCall& a, const char* who) {
    if (int rc = check_tracking_lqr_args(h, a, who)) return rc;
    // the sweep on the handle's knot schedule has never had an overlap rule
    const bool ruled = a.limited || a.guarded;
    const HostArgs args = {copy_in(kZ, a.Zref).ruled_if(ruled), copy_in(kModel, a.model).ruled_if(ruled),
                           copy_in(kEvent, a.event).ruled_if(ruled), copy_in(kSat, a.sat).ruled_if(ruled),
                           copy_out(kK, a.K).ruled_if(ruled), copy_out(kP, a.P).ruled_if(ruled)};
    return run_tracking_call(h, mem, args, who, [&](double* const* d, bool) {
        return qln::launch_tracking_lqr(h->p, a.Q, a.R, a.Qf, d[kZ], d[kModel], d[kEvent], d[kSat], d[kK], d[kP], h->stream);
    });
}

static LqrCall lqr_call(const double* Zref, const double* Q, const double* R, const double* Qf, double* K, double* P) {
    LqrCall a{};
    a.Zref = Zref; a.Q = Q; a.R = R; a.Qf = Qf; a.K = K; a.P = P;
    return a;
}
static LqrCall at_events(LqrCall a, const double* model, const double* event) {
    a.guarded = true; a.model = model; a.event = event;
    return a;
}
static LqrCall at_active_set(LqrCall a, const double* sat) {
    a.limited = true; a.sat = sat; a.guarded = a.event != nullptr;
    return a;
}

int qln_tracking_lqr(qln_handle* h, const double* Zref, const double* Qdiag, const double* Rdiag, const double* Qfdiag,
                     double* K, double* P) {
    return tracking_lqr(h, kDeviceMem, lqr_call(Zref, Qdiag, Rdiag, Qfdiag, K, P), "qln_tracking_lqr");
}
int qln_tracking_lqr_host(qln_handle* h, const double* Zref, const double* Qdiag, const double* Rdiag, const double* Qfdiag,
                          double* K, double* P) {
    return tracking_lqr(h, kHostMem, lqr_call(Zref, Qdiag, Rdiag, Qfdiag, K, P), "qln_tracking_lqr_host");
}
int qln_tracking_lqr_guarded(qln_handle* h, const double* Ztraj, const double* model, const double* event, const double* Qdiag,
                             const double* Rdiag, const double* Qfdiag, double* K, double* P) {
    return tracking_lqr(h, kDeviceMem, at_events(lqr_call(Ztraj, Qdiag, Rdiag, Qfdiag, K, P), model, event),
                        "qln_tracking_lqr_guarded");
}
int qln_tracking_lqr_guarded_host(qln_handle* h, const double* Ztraj, const double* model, const double* event,
                                  const double* Qdiag, const double* Rdiag, const double* Qfdiag, double* K, double* P) {
    return tracking_lqr(h, kHostMem, at_events(lqr_call(Ztraj, Qdiag, Rdiag, Qfdiag, K, P), model, event),
                        "qln_tracking_lqr_guarded_host");
}
// the design at the limited roll-out's active set: event selects the guarded blocks
int qln_tracking_lqr_limited(qln_handle* h, const double* Ztraj, const double* model, const double* event, const double* sat,
                             const double* Qdiag, const double* Rdiag, const double* Qfdiag, double* K, double* P) {
    return tracking_lqr(h, kDeviceMem, at_active_set(at_events(lqr_call(Ztraj, Qdiag, Rdiag, Qfdiag, K, P), model, event), sat),
                        "qln_tracking_lqr_limited");
}
int qln_tracking_lqr_limited_host(qln_handle* h, const double* Ztraj, const double* model, const double* event, const double* sat,
                                  const double* Qdiag, const double* Rdiag, const double* Qfdiag, double* K, double* P) {
    return tracking_lqr(h, kHostMem, at_active_set(at_events(lqr_call(Ztraj, Qdiag, Rdiag, Qfdiag, K, P), model, event), sat),
                        "qln_tracking_lqr_limited_host");
}

// The roll-out (k_tracking_rollout), with the per-problem plant as an optional argument: the entry points without a model
// leave it null, and the launch then takes the kernel without its kModel flag.
// guarded: the touchdown by the free foot's height, with its event records (may be null)
// limited: the roll-out within the force limits lim, with its saturation record sat (may be null)
struct RolloutCall {
    const double *Zref, *K, *x0, *model, *lim;
    double *Zout, *event, *sat;
    bool guarded, limited;
};

static int check_tracking_rollout_args(const qln_handle* h, const RolloutCall& a, const char* who) {
    if (a.limited) {
        if (int rc = check_force_limits(a.lim, who)) return rc;
        if (!a.guarded && a.event)
            return fail(QLN_ERR_INVALID_ARGUMENT, std::string(who) + ": event with guarded == 0 (the knot schedule has no record)");
    }
    if (int rc = check_handle(h)) return rc;
    if (!a.Zref || !a.Zout) return fail(QLN_ERR_INVALID_ARGUMENT, std::string(who) + ": null Zref or Zout");
    return QLN_OK;
}

static int tracking_rollout(qln_handle* h, MemForm mem, const RolloutCall& a, const char* who) {
    if (int rc = check_tracking_rollout_args(h, a, who)) return rc;
    // the overlap rule does not look at K, x0 and model
    const HostArgs args = {copy_in(kZ, a.Zref), copy_inout(kZio, a.Zout), copy_in(kK, a.K).ruled_if(false),
                           copy_in(kX0, a.x0).ruled_if(false), copy_in(kModel, a.model).ruled_if(false),
                           copy_out(kEvent, a.event), copy_out(kSat, a.sat)};
    return run_tracking_call(h, mem, args, who, [&](double* const* d, bool) {
        return qln::launch_tracking_rollout(h->p, d[kZ], d[kK], d[kX0], d[kModel], d[kZio], a.guarded, d[kEvent],
                                            a.limited ? a.lim : nullptr, d[kSat], h->stream);
    });
}

static RolloutCall rollout_call(const double* Zref, const double* K, const double* x0, const double* model, double* Zout) {
    RolloutCall a{};
    a.Zref = Zref; a.K = K; a.x0 = x0; a.model = model; a.Zout = Zout;
    return a;
}
static RolloutCall with_touchdown(RolloutCall a, double* event) {
    a.guarded = true; a.event = event;
    return a;
}
static RolloutCall within_limits(RolloutCall a, const double* lim, int32_t guarded, double* event, double* sat) {
    a.limited = true; a.lim = lim; a.sat = sat; a.guarded = guarded != 0; a.event = event;
    return a;
}

int qln_tracking_rollout(qln_handle* h, const double* Zref, const double* K, const double* x0, double* Zout) {
    return tracking_rollout(h, kDeviceMem, rollout_call(Zref, K, x0, nullptr, Zout), "qln_tracking_rollout");
}
int qln_tracking_rollout_host(qln_handle* h, const double* Zref, const double* K, const double* x0, double* Zout) {
    return tracking_rollout(h, kHostMem, rollout_call(Zref, K, x0, nullptr, Zout), "qln_tracking_rollout_host");
}
int qln_tracking_rollout_model(qln_handle* h, const double* Zref, const double* K, const double* x0, const double* model,
                               double* Zout) {
    return tracking_rollout(h, kDeviceMem, rollout_call(Zref, K, x0, model, Zout), "qln_tracking_rollout_model");
}
int qln_tracking_rollout_model_host(qln_handle* h, const double* Zref, const double* K, const double* x0, const double* model,
                                    double* Zout) {
    return tracking_rollout(h, kHostMem, rollout_call(Zref, K, x0, model, Zout), "qln_tracking_rollout_model_host");
}
int qln_tracking_rollout_guarded(qln_handle* h, const double* Zref, const double* K, const double* x0, const double* model,
                                 double* Zout, double* event) {
    return tracking_rollout(h, kDeviceMem, with_touchdown(rollout_call(Zref, K, x0, model, Zout), event),
                            "qln_tracking_rollout_guarded");
}
int qln_tracking_rollout_guarded_host(qln_handle* h, const double* Zref, const double* K, const double* x0, const double* model,
                                      double* Zout, double* event) {
    return tracking_rollout(h, kHostMem, with_touchdown(rollout_call(Zref, K, x0, model, Zout), event),
                            "qln_tracking_rollout_guarded_host");
}
// the roll-out within contact-aware force limits: the knot-scheduled or the guarded one, with its saturation record
int qln_tracking_rollout_limited(qln_handle* h, const double* Zref, const double* K, const double* x0, const double* model,
                                 const double* lim, int32_t guarded, double* Zout, double* event, double* sat) {
    return tracking_rollout(h, kDeviceMem, within_limits(rollout_call(Zref, K, x0, model, Zout), lim, guarded, event, sat),
                            "qln_tracking_rollout_limited");
}
int qln_tracking_rollout_limited_host(qln_handle* h, const double* Zref, const double* K, const double* x0, const double* model,
                                      const double* lim, int32_t guarded, double* Zout, double* event, double* sat) {
    return tracking_rollout(h, kHostMem, within_limits(rollout_call(Zref, K, x0, model, Zout), lim, guarded, event, sat),
                            "qln_tracking_rollout_limited_host");
}

// Its reverse sweep (k_tracking_rollout_vjp).  model_bar goes with model, as in the roll-out.
// guarded: the sweep through the guard-triggered touchdown, which needs the roll-out's event records
// limited: the sweep at the limited roll-out's active set, which needs its saturation record sat (checked first: it needs no
// handle); event then selects the guarded blocks
struct RolloutVjpCall {
    const double *Zref, *K, *Zout, *model, *event, *sat, *Zbar;
    double *Zref_bar, *K_bar, *x0_bar, *model_bar;
    bool guarded, limited;
};

static int check_tracking_vjp_args(const qln_handle* h, const RolloutVjpCall& a, const char* who) {
    const std::string w(who);
    if (int rc = check_limited_sat(a.limited, a.sat, w)) return rc;
    if (int rc = check_handle(h)) return rc;
    if (!a.Zref || !a.Zout || !a.Zbar) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null Zref, Zout or Zbar");
    if (int rc = check_guard_event(a.guarded, a.event, w)) return rc;
    if (a.K_bar && !a.K) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": K_bar needs K (K == NULL has no gains to differentiate)");
    return QLN_OK;
}

static int tracking_rollout_vjp(qln_handle* h, MemForm mem, const RolloutVjpCall& a, const char* who) {
    if (int rc = check_tracking_vjp_args(h, a, who)) return rc;
    // the host form stages Zref only when K_bar asks for it (the kernel reads it for nothing else); otherwise Zout's buffer
    // stands in
    const HostArgs args = {copy_in(kV, a.Zout), copy_in(kZbar, a.Zbar), copy_in(kZ, a.Zref).staged_if(a.K_bar != nullptr),
                           copy_in(kK, a.K), copy_in(kModel, a.model), copy_in(kEvent, a.event), copy_in(kSat, a.sat),
                           copy_inout(kZio, a.Zref_bar), copy_out(kKbar, a.K_bar), copy_out(kX0, a.x0_bar),
                           copy_out(kModelD, a.model_bar)};
    return run_tracking_call(h, mem, args, who, [&](double* const* d, bool) {
        return qln::launch_tracking_rollout_vjp(h->p, d[kZ] ? d[kZ] : d[kV], d[kK], d[kV], d[kModel], d[kEvent], d[kSat],
                                                d[kZbar], d[kZio], d[kKbar], d[kX0], d[kModelD], h->stream);
    });
}

static RolloutVjpCall rollout_vjp_call(const double* Zref, const double* K, const double* Zout, const double* Zbar,
                                       double* Zref_bar, double* K_bar, double* x0_bar) {
    RolloutVjpCall a{};
    a.Zref = Zref; a.K = K; a.Zout = Zout; a.Zbar = Zbar; a.Zref_bar = Zref_bar; a.K_bar = K_bar; a.x0_bar = x0_bar;
    return a;
}
static RolloutVjpCall with_model(RolloutVjpCall a, const double* model, double* model_bar) {
    a.model = model; a.model_bar = model_bar;
    return a;
}
static RolloutVjpCall at_events(RolloutVjpCall a, const double* event) {
    a.guarded = true; a.event = event;
    return a;
}
static RolloutVjpCall at_active_set(RolloutVjpCall a, const double* sat) {
    a.limited = true; a.sat = sat; a.guarded = a.event != nullptr;
    return a;
}

int qln_tracking_rollout_vjp(qln_handle* h, const double* Zref, const double* K, const double* Zout, const double* Zbar,
                             double* Zref_bar, double* K_bar, double* x0_bar) {
    return tracking_rollout_vjp(h, kDeviceMem, rollout_vjp_call(Zref, K, Zout, Zbar, Zref_bar, K_bar, x0_bar),
                                "qln_tracking_rollout_vjp");
}
int qln_tracking_rollout_vjp_host(qln_handle* h, const double* Zref, const double* K, const double* Zout, const double* Zbar,
                                  double* Zref_bar, double* K_bar, double* x0_bar) {
    return tracking_rollout_vjp(h, kHostMem, rollout_vjp_call(Zref, K, Zout, Zbar, Zref_bar, K_bar, x0_bar),
                                "qln_tracking_rollout_vjp_host");
}
int qln_tracking_rollout_model_vjp(qln_handle* h, const double* Zref, const double* K, const double* Zout, const double* model,
                                   const double* Zbar, double* Zref_bar, double* K_bar, double* x0_bar, double* model_bar) {
    return tracking_rollout_vjp(h, kDeviceMem,
                                with_model(rollout_vjp_call(Zref, K, Zout, Zbar, Zref_bar, K_bar, x0_bar), model, model_bar),
                                "qln_tracking_rollout_model_vjp");
}
int qln_tracking_rollout_model_vjp_host(qln_handle* h, const double* Zref, const double* K, const double* Zout,
                                        const double* model, const double* Zbar, double* Zref_bar, double* K_bar, double* x0_bar,
                                        double* model_bar) {
    return tracking_rollout_vjp(h, kHostMem,
                                with_model(rollout_vjp_call(Zref, K, Zout, Zbar, Zref_bar, K_bar, x0_bar), model, model_bar),
                                "qln_tracking_rollout_model_vjp_host");
}
int qln_tracking_rollout_guarded_vjp(qln_handle* h, const double* Zref, const double* K, const double* Zout, const double* model,
                                     const double* event, const double* Zbar, double* Zref_bar, double* K_bar, double* x0_bar,
                                     double* model_bar) {
    return tracking_rollout_vjp(h, kDeviceMem,
                                at_events(with_model(rollout_vjp_call(Zref, K, Zout, Zbar, Zref_bar, K_bar, x0_bar), model,
                                                     model_bar), event), "qln_tracking_rollout_guarded_vjp");
}
int qln_tracking_rollout_guarded_vjp_host(qln_handle* h, const double* Zref, const double* K, const double* Zout,
                                          const double* model, const double* event, const double* Zbar, double* Zref_bar,
                                          double* K_bar, double* x0_bar, double* model_bar) {
    return tracking_rollout_vjp(h, kHostMem,
                                at_events(with_model(rollout_vjp_call(Zref, K, Zout, Zbar, Zref_bar, K_bar, x0_bar), model,
                                                     model_bar), event), "qln_tracking_rollout_guarded_vjp_host");
}
int qln_tracking_rollout_limited_vjp(qln_handle* h, const double* Zref, const double* K, const double* Zout, const double* model,
                                     const double* event, const double* sat, const double* Zbar, double* Zref_bar, double* K_bar,
                                     double* x0_bar, double* model_bar) {
    return tracking_rollout_vjp(h, kDeviceMem,
                                at_active_set(at_events(with_model(rollout_vjp_call(Zref, K, Zout, Zbar, Zref_bar, K_bar, x0_bar),
                                                                   model, model_bar), event), sat),
                                "qln_tracking_rollout_limited_vjp");
}
int qln_tracking_rollout_limited_vjp_host(qln_handle* h, const double* Zref, const double* K, const double* Zout,
                                          const double* model, const double* event, const double* sat, const double* Zbar,
                                          double* Zref_bar, double* K_bar, double* x0_bar, double* model_bar) {
    return tracking_rollout_vjp(h, kHostMem,
                                at_active_set(at_events(with_model(rollout_vjp_call(Zref, K, Zout, Zbar, Zref_bar, K_bar, x0_bar),
                                                                   model, model_bar), event), sat),
                                "qln_tracking_rollout_limited_vjp_host");
}

// Its forward sweep (k_tracking_rollout_jvp).  The checks that need no handle come first.  guarded and limited as in the
// reverse sweep; event_dot goes with event.
struct RolloutJvpCall {
    const double *Zref, *K, *Zout, *model, *event, *sat, *Zref_dot, *K_dot, *x0_dot, *model_dot;
    double *Zout_dot, *event_dot;
    bool guarded, limited;
};

static int check_tracking_jvp_args(const qln_handle* h, const RolloutJvpCall& a, const char* who) {
    const std::string w(who);
    if (int rc = check_limited_sat(a.limited, a.sat, w)) return rc;
    if (a.limited && !a.event && a.event_dot)
        return fail(QLN_ERR_INVALID_ARGUMENT, w + ": event_dot without event (the knot-scheduled sweep has no record)");
    if (int rc = check_guard_event(a.guarded, a.event, w)) return rc;
    if (!a.Zref_dot && !a.K_dot && !a.x0_dot && !a.model_dot)
        return fail(QLN_ERR_INVALID_ARGUMENT, w + ": every tangent is NULL (no direction)");
    if (a.K_dot && !a.K) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": K_dot needs K (K == NULL has no gains to perturb)");
    if (!a.Zref || !a.Zout || !a.Zout_dot) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null Zref, Zout or Zout_dot");
    return check_handle(h);
}

static int tracking_rollout_jvp(qln_handle* h, MemForm mem, const RolloutJvpCall& a, const char* who) {
    if (int rc = check_tracking_jvp_args(h, a, who)) return rc;
    // the host form stages Zref only when K_dot is given (the kernel reads it for nothing else); otherwise Zout's buffer
    // stands in
    const HostArgs args = {copy_in(kV, a.Zout), copy_in(kZ, a.Zref).staged_if(a.K_dot != nullptr), copy_in(kK, a.K),
                           copy_in(kModel, a.model), copy_in(kEvent, a.event), copy_in(kSat, a.sat), copy_in(kZdot, a.Zref_dot),
                           copy_in(kKdot, a.K_dot), copy_in(kX0, a.x0_dot), copy_in(kModelD, a.model_dot),
                           copy_inout(kZio, a.Zout_dot), copy_out(kEventD, a.event_dot)};
    return run_tracking_call(h, mem, args, who, [&](double* const* d, bool) {
        return qln::launch_tracking_rollout_jvp(h->p, d[kZ] ? d[kZ] : d[kV], d[kK], d[kV], d[kModel], d[kEvent], d[kSat],
                                                d[kZdot], d[kKdot], d[kX0], d[kModelD], d[kZio], d[kEventD], h->stream);
    });
}

static RolloutJvpCall rollout_jvp_call(const double* Zref, const double* K, const double* Zout, const double* Zref_dot,
                                       const double* K_dot, const double* x0_dot, double* Zout_dot) {
    RolloutJvpCall a{};
    a.Zref = Zref; a.K = K; a.Zout = Zout; a.Zref_dot = Zref_dot; a.K_dot = K_dot; a.x0_dot = x0_dot; a.Zout_dot = Zout_dot;
    return a;
}
static RolloutJvpCall with_model(RolloutJvpCall a, const double* model, const double* model_dot) {
    a.model = model; a.model_dot = model_dot;
    return a;
}
static RolloutJvpCall at_events(RolloutJvpCall a, const double* event, double* event_dot) {
    a.guarded = true; a.event = event; a.event_dot = event_dot;
    return a;
}
static RolloutJvpCall at_active_set(RolloutJvpCall a, const double* sat) {
    a.limited = true; a.sat = sat; a.guarded = a.event != nullptr;
    return a;
}

int qln_tracking_rollout_jvp(qln_handle* h, const double* Zref, const double* K, const double* Zout, const double* Zref_dot,
                             const double* K_dot, const double* x0_dot, double* Zout_dot) {
    return tracking_rollout_jvp(h, kDeviceMem, rollout_jvp_call(Zref, K, Zout, Zref_dot, K_dot, x0_dot, Zout_dot),
                                "qln_tracking_rollout_jvp");
}
int qln_tracking_rollout_jvp_host(qln_handle* h, const double* Zref, const double* K, const double* Zout,
                                  const double* Zref_dot, const double* K_dot, const double* x0_dot, double* Zout_dot) {
    return tracking_rollout_jvp(h, kHostMem, rollout_jvp_call(Zref, K, Zout, Zref_dot, K_dot, x0_dot, Zout_dot),
                                "qln_tracking_rollout_jvp_host");
}
int qln_tracking_rollout_model_jvp(qln_handle* h, const double* Zref, const double* K, const double* Zout, const double* model,
                                   const double* Zref_dot, const double* K_dot, const double* x0_dot, const double* model_dot,
                                   double* Zout_dot) {
    return tracking_rollout_jvp(h, kDeviceMem,
                                with_model(rollout_jvp_call(Zref, K, Zout, Zref_dot, K_dot, x0_dot, Zout_dot), model, model_dot),
                                "qln_tracking_rollout_model_jvp");
}
int qln_tracking_rollout_model_jvp_host(qln_handle* h, const double* Zref, const double* K, const double* Zout,
                                        const double* model, const double* Zref_dot, const double* K_dot, const double* x0_dot,
                                        const double* model_dot, double* Zout_dot) {
    return tracking_rollout_jvp(h, kHostMem,
                                with_model(rollout_jvp_call(Zref, K, Zout, Zref_dot, K_dot, x0_dot, Zout_dot), model, model_dot),
                                "qln_tracking_rollout_model_jvp_host");
}
int qln_tracking_rollout_guarded_jvp(qln_handle* h, const double* Zref, const double* K, const double* Zout, const double* model,
                                     const double* event, const double* Zref_dot, const double* K_dot, const double* x0_dot,
                                     const double* model_dot, double* Zout_dot, double* event_dot) {
    return tracking_rollout_jvp(h, kDeviceMem,
                                at_events(with_model(rollout_jvp_call(Zref, K, Zout, Zref_dot, K_dot, x0_dot, Zout_dot), model,
                                                     model_dot), event, event_dot), "qln_tracking_rollout_guarded_jvp");
}
int qln_tracking_rollout_guarded_jvp_host(qln_handle* h, const double* Zref, const double* K, const double* Zout,
                                          const double* model, const double* event, const double* Zref_dot, const double* K_dot,
                                          const double* x0_dot, const double* model_dot, double* Zout_dot, double* event_dot) {
    return tracking_rollout_jvp(h, kHostMem,
                                at_events(with_model(rollout_jvp_call(Zref, K, Zout, Zref_dot, K_dot, x0_dot, Zout_dot), model,
                                                     model_dot), event, event_dot), "qln_tracking_rollout_guarded_jvp_host");
}
int qln_tracking_rollout_limited_jvp(qln_handle* h, const double* Zref, const double* K, const double* Zout, const double* model,
                                     const double* event, const double* sat, const double* Zref_dot, const double* K_dot,
                                     const double* x0_dot, const double* model_dot, double* Zout_dot, double* event_dot) {
    return tracking_rollout_jvp(h, kDeviceMem,
                                at_active_set(at_events(with_model(rollout_jvp_call(Zref, K, Zout, Zref_dot, K_dot, x0_dot,
                                                                                    Zout_dot), model, model_dot), event, event_dot),
                                              sat), "qln_tracking_rollout_limited_jvp");
}
int qln_tracking_rollout_limited_jvp_host(qln_handle* h, const double* Zref, const double* K, const double* Zout,
                                          const double* model, const double* event, const double* sat, const double* Zref_dot,
                                          const double* K_dot, const double* x0_dot, const double* model_dot, double* Zout_dot,
                                          double* event_dot) {
    return tracking_rollout_jvp(h, kHostMem,
                                at_active_set(at_events(with_model(rollout_jvp_call(Zref, K, Zout, Zref_dot, K_dot, x0_dot,
                                                                                    Zout_dot), model, model_dot), event, event_dot),
                                              sat), "qln_tracking_rollout_limited_jvp_host");
}

// The covariance sweep (k_tracking_covariance).  The checks that need no handle come first.
// guarded: the sweep through the guard-triggered touchdown, which needs the roll-out's event records and may return event_var
struct CovarianceCall {
    const double *Zout, *K, *model, *event, *Sigma0;
    int32_t sigma0_batch;
    const double* Wdiag;
    double *Sigma, *marg, *event_var;
    bool guarded;
};

static int check_tracking_covariance_args(const qln_handle* h, const CovarianceCall& a, const char* who) {
    const std::string w(who);
    if (!a.Sigma && !a.marg && !a.event_var)
        return fail(QLN_ERR_INVALID_ARGUMENT, a.guarded ? w + ": Sigma, marg and event_var are all NULL (nothing to compute)"
                                                        : w + ": Sigma and marg are both NULL (nothing to compute)");
    if (int rc = check_guard_event(a.guarded, a.event, w)) return rc;
    if (int rc = check_tracking_wdiag(a.Wdiag, w)) return rc;
    if (int rc = check_sigma0_batch(a.sigma0_batch, nullptr, w)) return rc;
    if (int rc = check_handle(h)) return rc;
    if (int rc = check_sigma0_batch(a.sigma0_batch, h, w)) return rc;
    if (!a.Zout || !a.Sigma0) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null Zout or Sigma0");
    return QLN_OK;
}

static int tracking_covariance(qln_handle* h, MemForm mem, const CovarianceCall& a, const char* who) {
    if (int rc = check_tracking_covariance_args(h, a, who)) return rc;
    // Sigma0: the tiles the call reads, of the role's B
    const HostArgs args = {copy_in(kV, a.Zout), copy_in(kK, a.K), copy_in(kModel, a.model), copy_in(kEvent, a.event),
                           copy_in(kCov0, a.Sigma0).sized((int64_t)a.sigma0_batch * QLN_TRACK_P_NNZ), copy_out(kCov, a.Sigma),
                           copy_out(kMarg, a.marg), copy_out(kEventVar, a.event_var)};
    return run_tracking_call(h, mem, args, who, [&](double* const* d, bool) {
        return qln::launch_tracking_covariance(h->p, d[kV], d[kK], d[kModel], d[kEvent], d[kCov0], a.sigma0_batch, a.Wdiag,
                                               d[kCov], d[kMarg], d[kEventVar], h->stream);
    });
}

static CovarianceCall covariance_call(const double* Zout, const double* K, const double* Sigma0, int32_t sigma0_batch,
                                      const double* Wdiag, double* Sigma, double* marg) {
    CovarianceCall a{};
    a.Zout = Zout; a.K = K; a.Sigma0 = Sigma0; a.sigma0_batch = sigma0_batch; a.Wdiag = Wdiag; a.Sigma = Sigma; a.marg = marg;
    return a;
}
static CovarianceCall at_events(CovarianceCall a, const double* model, const double* event, double* event_var) {
    a.guarded = true; a.model = model; a.event = event; a.event_var = event_var;
    return a;
}

int qln_tracking_covariance(qln_handle* h, const double* Zout, const double* K, const double* Sigma0, int32_t sigma0_batch,
                            const double* Wdiag, double* Sigma, double* marg) {
    return tracking_covariance(h, kDeviceMem, covariance_call(Zout, K, Sigma0, sigma0_batch, Wdiag, Sigma, marg),
                               "qln_tracking_covariance");
}
int qln_tracking_covariance_host(qln_handle* h, const double* Zout, const double* K, const double* Sigma0,
                                 int32_t sigma0_batch, const double* Wdiag, double* Sigma, double* marg) {
    return tracking_covariance(h, kHostMem, covariance_call(Zout, K, Sigma0, sigma0_batch, Wdiag, Sigma, marg),
                               "qln_tracking_covariance_host");
}
int qln_tracking_covariance_guarded(qln_handle* h, const double* Zout, const double* K, const double* model, const double* event,
                                    const double* Sigma0, int32_t sigma0_batch, const double* Wdiag, double* Sigma, double* marg,
                                    double* event_var) {
    return tracking_covariance(h, kDeviceMem,
                               at_events(covariance_call(Zout, K, Sigma0, sigma0_batch, Wdiag, Sigma, marg), model, event,
                                         event_var), "qln_tracking_covariance_guarded");
}
int qln_tracking_covariance_guarded_host(qln_handle* h, const double* Zout, const double* K, const double* model,
                                         const double* event, const double* Sigma0, int32_t sigma0_batch, const double* Wdiag,
                                         double* Sigma, double* marg, double* event_var) {
    return tracking_covariance(h, kHostMem,
                               at_events(covariance_call(Zout, K, Sigma0, sigma0_batch, Wdiag, Sigma, marg), model, event,
                                         event_var), "qln_tracking_covariance_guarded_host");
}

// The Kalman filter and the LQG covariance (k_tracking_kalman).  The checks that need no handle come first.
// guarded: through the guard-triggered touchdown, which needs the roll-out's event records and may return event_var
struct KalmanCall {
    const double *Zout, *K, *model, *event, *H;
    int32_t ny;
    const double *Vdiag, *Sigma0;
    int32_t sigma0_batch;
    const double* Wdiag;
    double *Lgain, *Pest, *Sigma, *marg, *event_var;
    bool guarded;
};

static int check_tracking_kalman_args(const qln_handle* h, const KalmanCall& a, const char* who) {
    const std::string w(who);
    if (int rc = check_tracking_ny(a.ny, w)) return rc;
    if (int rc = check_some_output(a.Lgain || a.Pest || a.Sigma || a.marg || a.event_var, w)) return rc;
    if (!a.K && (a.Sigma || a.marg || a.event_var))
        return fail(QLN_ERR_INVALID_ARGUMENT, w + ": Sigma, marg and event_var need K (K == NULL is the filter alone: Lgain and Pest)");
    if (int rc = check_guard_event(a.guarded, a.event, w)) return rc;
    if (!a.H || !a.Vdiag) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null H or Vdiag");
    if (int rc = check_tracking_vdiag(a.Vdiag, a.ny, w)) return rc;
    if (int rc = check_tracking_wdiag(a.Wdiag, w)) return rc;
    if (int rc = check_sigma0_batch(a.sigma0_batch, nullptr, w)) return rc;
    if (int rc = check_handle(h)) return rc;
    if (int rc = check_sigma0_batch(a.sigma0_batch, h, w)) return rc;
    if (!a.Zout || !a.Sigma0) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null Zout or Sigma0");
    return QLN_OK;
}

static int tracking_kalman(qln_handle* h, MemForm mem, const KalmanCall& a, const char* who) {
    if (int rc = check_tracking_kalman_args(h, a, who)) return rc;
    // the rows the call reads and the gains it writes, of the roles' eight; the tiles it reads, of the role's B
    const HostArgs args = {copy_in(kV, a.Zout), copy_in(kK, a.K), copy_in(kH, a.H).sized((int64_t)a.ny * QLN_NX),
                           copy_in(kModel, a.model), copy_in(kEvent, a.event),
                           copy_in(kCov0, a.Sigma0).sized((int64_t)a.sigma0_batch * QLN_TRACK_P_NNZ),
                           copy_out(kLgain, a.Lgain).sized(tracking_gain_total(h->dims, a.ny)), copy_out(kPest, a.Pest),
                           copy_out(kCov, a.Sigma), copy_out(kMarg, a.marg), copy_out(kEventVar, a.event_var)};
    return run_tracking_call(h, mem, args, who, [&](double* const* d, bool) {
        return qln::launch_tracking_kalman(h->p, d[kV], d[kK], d[kModel], d[kEvent], d[kH], a.ny, a.Vdiag, d[kCov0],
                                           a.sigma0_batch, a.Wdiag, d[kLgain], d[kPest], d[kCov], d[kMarg], d[kEventVar],
                                           h->stream);
    });
}

static KalmanCall kalman_call(const double* Zout, const double* K, const double* H, int32_t ny, const double* Vdiag,
                              const double* Sigma0, int32_t sigma0_batch, const double* Wdiag, double* Lgain, double* Pest,
                              double* Sigma, double* marg) {
    KalmanCall a{};
    a.Zout = Zout; a.K = K; a.H = H; a.ny = ny; a.Vdiag = Vdiag; a.Sigma0 = Sigma0; a.sigma0_batch = sigma0_batch;
    a.Wdiag = Wdiag; a.Lgain = Lgain; a.Pest = Pest; a.Sigma = Sigma; a.marg = marg;
    return a;
}
static KalmanCall at_events(KalmanCall a, const double* model, const double* event, double* event_var) {
    a.guarded = true; a.model = model; a.event = event; a.event_var = event_var;
    return a;
}

int qln_tracking_kalman(qln_handle* h, const double* Zout, const double* K, const double* H, int32_t ny, const double* Vdiag,
                        const double* Sigma0, int32_t sigma0_batch, const double* Wdiag, double* Lgain, double* Pest,
                        double* Sigma, double* marg) {
    return tracking_kalman(h, kDeviceMem, kalman_call(Zout, K, H, ny, Vdiag, Sigma0, sigma0_batch, Wdiag, Lgain, Pest, Sigma, marg),
                           "qln_tracking_kalman");
}
int qln_tracking_kalman_host(qln_handle* h, const double* Zout, const double* K, const double* H, int32_t ny, const double* Vdiag,
                             const double* Sigma0, int32_t sigma0_batch, const double* Wdiag, double* Lgain, double* Pest,
                             double* Sigma, double* marg) {
    return tracking_kalman(h, kHostMem, kalman_call(Zout, K, H, ny, Vdiag, Sigma0, sigma0_batch, Wdiag, Lgain, Pest, Sigma, marg),
                           "qln_tracking_kalman_host");
}
int qln_tracking_kalman_guarded(qln_handle* h, const double* Zout, const double* K, const double* model, const double* event,
                                const double* H, int32_t ny, const double* Vdiag, const double* Sigma0, int32_t sigma0_batch,
                                const double* Wdiag, double* Lgain, double* Pest, double* Sigma, double* marg, double* event_var) {
    return tracking_kalman(h, kDeviceMem,
                           at_events(kalman_call(Zout, K, H, ny, Vdiag, Sigma0, sigma0_batch, Wdiag, Lgain, Pest, Sigma, marg),
                                     model, event, event_var), "qln_tracking_kalman_guarded");
}
int qln_tracking_kalman_guarded_host(qln_handle* h, const double* Zout, const double* K, const double* model, const double* event,
                                     const double* H, int32_t ny, const double* Vdiag, const double* Sigma0, int32_t sigma0_batch,
                                     const double* Wdiag, double* Lgain, double* Pest, double* Sigma, double* marg,
                                     double* event_var) {
    return tracking_kalman(h, kHostMem,
                           at_events(kalman_call(Zout, K, H, ny, Vdiag, Sigma0, sigma0_batch, Wdiag, Lgain, Pest, Sigma, marg),
                                     model, event, event_var), "qln_tracking_kalman_guarded_host");
}

// The forward sweep through the Kalman design (k_tracking_kalman_jvp).  The checks that need no handle come first.
// guarded: through the guard-triggered touchdown, which needs the roll-out's event records
struct KalmanJvpCall {
    const double *Zout, *model, *event, *Lgain, *H;
    int32_t ny;
    const double *Vdiag, *Sigma0_dot;
    int32_t sigma0_batch;
    const double *Wdiag_dot, *Vdiag_dot;
    double *Lgain_dot, *Pest_dot, *logdet_dot;
    bool guarded;
};

static int check_kalman_design_jvp_args(const qln_handle* h, const KalmanJvpCall& a, const char* who) {
    const std::string w(who);
    if (int rc = check_tracking_ny(a.ny, w)) return rc;
    if (int rc = check_some_output(a.Lgain_dot || a.Pest_dot || a.logdet_dot, w)) return rc;
    if (int rc = check_guard_event(a.guarded, a.event, w)) return rc;
    if (!a.H || !a.Vdiag) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null H or Vdiag");
    if (int rc = check_tracking_vdiag(a.Vdiag, a.ny, w)) return rc;
    if (!a.Sigma0_dot && !a.Wdiag_dot && !a.Vdiag_dot)
        return fail(QLN_ERR_INVALID_ARGUMENT, w + ": Sigma0_dot, Wdiag_dot and Vdiag_dot are all NULL (no direction)");
    if (a.Wdiag_dot)
        for (int i = 0; i < QLN_NX; ++i)
            if (!std::isfinite(a.Wdiag_dot[i]))
                return fail(QLN_ERR_INVALID_ARGUMENT, w + ": Wdiag_dot must be finite (entry " + std::to_string(i) + ")");
    if (a.Vdiag_dot)
        for (int i = 0; i < a.ny; ++i)
            if (!std::isfinite(a.Vdiag_dot[i]))
                return fail(QLN_ERR_INVALID_ARGUMENT, w + ": Vdiag_dot must be finite (entry " + std::to_string(i) + ")");
    if (!a.Lgain) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null Lgain");
    if (a.Sigma0_dot)
        if (int rc = check_sigma0_batch(a.sigma0_batch, nullptr, w)) return rc;
    if (int rc = check_handle(h)) return rc;
    if (a.Sigma0_dot)
        if (int rc = check_sigma0_batch(a.sigma0_batch, h, w)) return rc;
    if (!a.Zout) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null Zout");
    return QLN_OK;
}

static int kalman_design_jvp(qln_handle* h, MemForm mem, const KalmanJvpCall& a, const char* who) {
    if (int rc = check_kalman_design_jvp_args(h, a, who)) return rc;
    // the rows and gains of the call's ny, of the roles' eight; the tiles it reads, of the role's B
    const int64_t ng = tracking_gain_total(h->dims, a.ny);
    const int32_t nb = a.Sigma0_dot ? a.sigma0_batch : 1;
    const HostArgs args = {copy_in(kV, a.Zout), copy_in(kH, a.H).sized((int64_t)a.ny * QLN_NX), copy_in(kModel, a.model),
                           copy_in(kEvent, a.event), copy_in(kLgain, a.Lgain).sized(ng),
                           copy_in(kCov0, a.Sigma0_dot).sized((int64_t)nb * QLN_TRACK_P_NNZ),
                           copy_out(kLgainD, a.Lgain_dot).sized(ng), copy_out(kPest, a.Pest_dot), copy_out(kNisD, a.logdet_dot)};
    return run_tracking_call(h, mem, args, who, [&](double* const* d, bool) {
        return qln::launch_tracking_kalman_jvp(h->p, d[kV], d[kModel], d[kEvent], d[kLgain], d[kH], a.ny, a.Vdiag, d[kCov0], nb,
                                               a.Wdiag_dot, a.Vdiag_dot, d[kLgainD], d[kPest], d[kNisD], h->stream);
    });
}

static KalmanJvpCall kalman_jvp_call(const double* Zout, const double* Lgain, const double* H, int32_t ny, const double* Vdiag,
                                     const double* Sigma0_dot, int32_t sigma0_batch, const double* Wdiag_dot,
                                     const double* Vdiag_dot, double* Lgain_dot, double* Pest_dot, double* logdet_dot) {
    KalmanJvpCall a{};
    a.Zout = Zout; a.Lgain = Lgain; a.H = H; a.ny = ny; a.Vdiag = Vdiag; a.Sigma0_dot = Sigma0_dot; a.sigma0_batch = sigma0_batch;
    a.Wdiag_dot = Wdiag_dot; a.Vdiag_dot = Vdiag_dot; a.Lgain_dot = Lgain_dot; a.Pest_dot = Pest_dot; a.logdet_dot = logdet_dot;
    return a;
}
static KalmanJvpCall at_events(KalmanJvpCall a, const double* model, const double* event) {
    a.guarded = true; a.model = model; a.event = event;
    return a;
}

int qln_kalman_design_jvp(qln_handle* h, const double* Zout, const double* Lgain, const double* H, int32_t ny, const double* Vdiag,
                          const double* Sigma0_dot, int32_t sigma0_batch, const double* Wdiag_dot, const double* Vdiag_dot,
                          double* Lgain_dot, double* Pest_dot, double* logdet_dot) {
    return kalman_design_jvp(h, kDeviceMem,
                             kalman_jvp_call(Zout, Lgain, H, ny, Vdiag, Sigma0_dot, sigma0_batch, Wdiag_dot, Vdiag_dot, Lgain_dot,
                                             Pest_dot, logdet_dot), "qln_kalman_design_jvp");
}
int qln_kalman_design_jvp_host(qln_handle* h, const double* Zout, const double* Lgain, const double* H, int32_t ny,
                               const double* Vdiag, const double* Sigma0_dot, int32_t sigma0_batch, const double* Wdiag_dot,
                               const double* Vdiag_dot, double* Lgain_dot, double* Pest_dot, double* logdet_dot) {
    return kalman_design_jvp(h, kHostMem,
                             kalman_jvp_call(Zout, Lgain, H, ny, Vdiag, Sigma0_dot, sigma0_batch, Wdiag_dot, Vdiag_dot, Lgain_dot,
                                             Pest_dot, logdet_dot), "qln_kalman_design_jvp_host");
}
int qln_kalman_design_guarded_jvp(qln_handle* h, const double* Zout, const double* model, const double* event, const double* Lgain,
                                  const double* H, int32_t ny, const double* Vdiag, const double* Sigma0_dot, int32_t sigma0_batch,
                                  const double* Wdiag_dot, const double* Vdiag_dot, double* Lgain_dot, double* Pest_dot,
                                  double* logdet_dot) {
    return kalman_design_jvp(h, kDeviceMem,
                             at_events(kalman_jvp_call(Zout, Lgain, H, ny, Vdiag, Sigma0_dot, sigma0_batch, Wdiag_dot, Vdiag_dot,
                                                       Lgain_dot, Pest_dot, logdet_dot), model, event),
                             "qln_kalman_design_guarded_jvp");
}
int qln_kalman_design_guarded_jvp_host(qln_handle* h, const double* Zout, const double* model, const double* event,
                                       const double* Lgain, const double* H, int32_t ny, const double* Vdiag,
                                       const double* Sigma0_dot, int32_t sigma0_batch, const double* Wdiag_dot,
                                       const double* Vdiag_dot, double* Lgain_dot, double* Pest_dot, double* logdet_dot) {
    return kalman_design_jvp(h, kHostMem,
                             at_events(kalman_jvp_call(Zout, Lgain, H, ny, Vdiag, Sigma0_dot, sigma0_batch, Wdiag_dot, Vdiag_dot,
                                                       Lgain_dot, Pest_dot, logdet_dot), model, event),
                             "qln_kalman_design_guarded_jvp_host");
}

// The reverse sweep through the Kalman design (k_tracking_kalman_vjp).  The checks that need no handle come first.
// guarded: through the guard-triggered touchdown, which needs the roll-out's event records
struct KalmanVjpCall {
    const double *Zout, *model, *event, *Lgain, *H;
    int32_t ny;
    const double *Vdiag, *Lgain_bar, *Pest_bar, *logdet_bar;
    double *Sigma0_bar, *Wdiag_bar, *Vdiag_bar;
    bool guarded;
};

static int check_noise_design_vjp_args(const qln_handle* h, const KalmanVjpCall& a, const char* who) {
    const std::string w(who);
    if (int rc = check_tracking_ny(a.ny, w)) return rc;
    if (int rc = check_some_output(a.Sigma0_bar || a.Wdiag_bar || a.Vdiag_bar, w)) return rc;
    if (int rc = check_guard_event(a.guarded, a.event, w)) return rc;
    if (!a.H || !a.Vdiag) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null H or Vdiag");
    if (int rc = check_tracking_vdiag(a.Vdiag, a.ny, w)) return rc;
    if (!a.Lgain_bar && !a.Pest_bar && !a.logdet_bar)
        return fail(QLN_ERR_INVALID_ARGUMENT, w + ": Lgain_bar, Pest_bar and logdet_bar are all NULL (no cotangent)");
    if (!a.Lgain) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null Lgain");
    if (int rc = check_handle(h)) return rc;
    if (!a.Zout) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null Zout");
    return QLN_OK;
}

static int noise_design_vjp(qln_handle* h, MemForm mem, const KalmanVjpCall& a, const char* who) {
    if (int rc = check_noise_design_vjp_args(h, a, who)) return rc;
    // the rows, gains and variances of the call's ny, of the roles' eight
    const int64_t ng = tracking_gain_total(h->dims, a.ny);
    const HostArgs args = {copy_in(kV, a.Zout), copy_in(kH, a.H).sized((int64_t)a.ny * QLN_NX), copy_in(kModel, a.model),
                           copy_in(kEvent, a.event), copy_in(kLgain, a.Lgain).sized(ng), copy_in(kLgainD, a.Lgain_bar).sized(ng),
                           copy_in(kPest, a.Pest_bar), copy_in(kNisD, a.logdet_bar), copy_out(kCov0, a.Sigma0_bar),
                           copy_out(kX0, a.Wdiag_bar), copy_out(kVbar, a.Vdiag_bar).sized((int64_t)h->dims.B * a.ny)};
    return run_tracking_call(h, mem, args, who, [&](double* const* d, bool) {
        return qln::launch_tracking_kalman_vjp(h->p, d[kV], d[kModel], d[kEvent], d[kLgain], d[kH], a.ny, a.Vdiag, d[kLgainD],
                                               d[kPest], d[kNisD], d[kCov0], d[kX0], d[kVbar], h->stream);
    });
}

static KalmanVjpCall kalman_vjp_call(const double* Zout, const double* Lgain, const double* H, int32_t ny, const double* Vdiag,
                                     const double* Lgain_bar, const double* Pest_bar, const double* logdet_bar, double* Sigma0_bar,
                                     double* Wdiag_bar, double* Vdiag_bar) {
    KalmanVjpCall a{};
    a.Zout = Zout; a.Lgain = Lgain; a.H = H; a.ny = ny; a.Vdiag = Vdiag; a.Lgain_bar = Lgain_bar; a.Pest_bar = Pest_bar;
    a.logdet_bar = logdet_bar; a.Sigma0_bar = Sigma0_bar; a.Wdiag_bar = Wdiag_bar; a.Vdiag_bar = Vdiag_bar;
    return a;
}
static KalmanVjpCall at_events(KalmanVjpCall a, const double* model, const double* event) {
    a.guarded = true; a.model = model; a.event = event;
    return a;
}

int qln_noise_design_vjp(qln_handle* h, const double* Zout, const double* Lgain, const double* H, int32_t ny, const double* Vdiag,
                         const double* Lgain_bar, const double* Pest_bar, const double* logdet_bar, double* Sigma0_bar,
                         double* Wdiag_bar, double* Vdiag_bar) {
    return noise_design_vjp(h, kDeviceMem,
                            kalman_vjp_call(Zout, Lgain, H, ny, Vdiag, Lgain_bar, Pest_bar, logdet_bar, Sigma0_bar, Wdiag_bar,
                                            Vdiag_bar), "qln_noise_design_vjp");
}
int qln_noise_design_vjp_host(qln_handle* h, const double* Zout, const double* Lgain, const double* H, int32_t ny,
                              const double* Vdiag, const double* Lgain_bar, const double* Pest_bar, const double* logdet_bar,
                              double* Sigma0_bar, double* Wdiag_bar, double* Vdiag_bar) {
    return noise_design_vjp(h, kHostMem,
                            kalman_vjp_call(Zout, Lgain, H, ny, Vdiag, Lgain_bar, Pest_bar, logdet_bar, Sigma0_bar, Wdiag_bar,
                                            Vdiag_bar), "qln_noise_design_vjp_host");
}
int qln_noise_design_guarded_vjp(qln_handle* h, const double* Zout, const double* model, const double* event, const double* Lgain,
                                 const double* H, int32_t ny, const double* Vdiag, const double* Lgain_bar, const double* Pest_bar,
                                 const double* logdet_bar, double* Sigma0_bar, double* Wdiag_bar, double* Vdiag_bar) {
    return noise_design_vjp(h, kDeviceMem,
                            at_events(kalman_vjp_call(Zout, Lgain, H, ny, Vdiag, Lgain_bar, Pest_bar, logdet_bar, Sigma0_bar,
                                                      Wdiag_bar, Vdiag_bar), model, event), "qln_noise_design_guarded_vjp");
}
int qln_noise_design_guarded_vjp_host(qln_handle* h, const double* Zout, const double* model, const double* event,
                                      const double* Lgain, const double* H, int32_t ny, const double* Vdiag,
                                      const double* Lgain_bar, const double* Pest_bar, const double* logdet_bar,
                                      double* Sigma0_bar, double* Wdiag_bar, double* Vdiag_bar) {
    return noise_design_vjp(h, kHostMem,
                            at_events(kalman_vjp_call(Zout, Lgain, H, ny, Vdiag, Lgain_bar, Pest_bar, logdet_bar, Sigma0_bar,
                                                      Wdiag_bar, Vdiag_bar), model, event), "qln_noise_design_guarded_vjp_host");
}

// The fixed-interval smoother (k_landing_smoother).  The checks that need no handle come first.
// guarded: through the guard-triggered touchdown, which needs the roll-out's event records
struct SmootherCall {
    const double *Ztraj, *model, *event, *Lgain, *Pest, *H;
    int32_t ny;
    const double *Vdiag, *Xhat, *innov;
    double *Xs, *Ps;
    bool guarded;
};

static int check_landing_smoother_args(const qln_handle* h, const SmootherCall& a, const char* who) {
    const std::string w(who);
    if (int rc = check_tracking_ny(a.ny, w)) return rc;
    if (!a.Xs && !a.Ps) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": Xs and Ps are both NULL (nothing to compute)");
    if (int rc = check_guard_event(a.guarded, a.event, w)) return rc;
    if (!a.H || !a.Vdiag) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null H or Vdiag");
    if (int rc = check_tracking_vdiag(a.Vdiag, a.ny, w)) return rc;
    if (!a.Lgain || !a.Pest) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null Lgain or Pest");
    if (!a.Xhat || !a.innov) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null Xhat or innov");
    if (int rc = check_handle(h)) return rc;
    if (!a.Ztraj) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null Ztraj");
    return QLN_OK;
}

static int landing_smoother(qln_handle* h, MemForm mem, const SmootherCall& a, const char* who) {
    if (int rc = check_landing_smoother_args(h, a, who)) return rc;
    // the rows, gains and innovations of the call's ny, of the roles' eight
    const HostArgs args = {copy_in(kV, a.Ztraj), copy_in(kH, a.H).sized((int64_t)a.ny * QLN_NX), copy_in(kModel, a.model),
                           copy_in(kEvent, a.event), copy_in(kLgain, a.Lgain).sized(tracking_gain_total(h->dims, a.ny)),
                           copy_in(kPest, a.Pest), copy_in(kXhat, a.Xhat),
                           copy_in(kInnov, a.innov).sized(tracking_meas_total(h->dims, a.ny)), copy_out(kXs, a.Xs),
                           copy_out(kPs, a.Ps)};
    return run_tracking_call(h, mem, args, who, [&](double* const* d, bool) {
        return qln::launch_landing_smoother(h->p, d[kV], d[kModel], d[kEvent], d[kLgain], d[kPest], d[kH], a.ny, a.Vdiag,
                                            d[kXhat], d[kInnov], d[kXs], d[kPs], h->stream);
    });
}

static SmootherCall smoother_call(const double* Ztraj, const double* Lgain, const double* Pest, const double* H, int32_t ny,
                                  const double* Vdiag, const double* Xhat, const double* innov, double* Xs, double* Ps) {
    SmootherCall a{};
    a.Ztraj = Ztraj; a.Lgain = Lgain; a.Pest = Pest; a.H = H; a.ny = ny; a.Vdiag = Vdiag; a.Xhat = Xhat; a.innov = innov;
    a.Xs = Xs; a.Ps = Ps;
    return a;
}
static SmootherCall at_events(SmootherCall a, const double* model, const double* event) {
    a.guarded = true; a.model = model; a.event = event;
    return a;
}

int qln_landing_smoother(qln_handle* h, const double* Ztraj, const double* Lgain, const double* Pest, const double* H, int32_t ny,
                         const double* Vdiag, const double* Xhat, const double* innov, double* Xs, double* Ps) {
    return landing_smoother(h, kDeviceMem, smoother_call(Ztraj, Lgain, Pest, H, ny, Vdiag, Xhat, innov, Xs, Ps),
                            "qln_landing_smoother");
}
int qln_landing_smoother_host(qln_handle* h, const double* Ztraj, const double* Lgain, const double* Pest, const double* H,
                              int32_t ny, const double* Vdiag, const double* Xhat, const double* innov, double* Xs, double* Ps) {
    return landing_smoother(h, kHostMem, smoother_call(Ztraj, Lgain, Pest, H, ny, Vdiag, Xhat, innov, Xs, Ps),
                            "qln_landing_smoother_host");
}
int qln_landing_smoother_guarded(qln_handle* h, const double* Ztraj, const double* model, const double* event, const double* Lgain,
                                 const double* Pest, const double* H, int32_t ny, const double* Vdiag, const double* Xhat,
                                 const double* innov, double* Xs, double* Ps) {
    return landing_smoother(h, kDeviceMem,
                            at_events(smoother_call(Ztraj, Lgain, Pest, H, ny, Vdiag, Xhat, innov, Xs, Ps), model, event),
                            "qln_landing_smoother_guarded");
}
int qln_landing_smoother_guarded_host(qln_handle* h, const double* Ztraj, const double* model, const double* event,
                                      const double* Lgain, const double* Pest, const double* H, int32_t ny, const double* Vdiag,
                                      const double* Xhat, const double* innov, double* Xs, double* Ps) {
    return landing_smoother(h, kHostMem,
                            at_events(smoother_call(Ztraj, Lgain, Pest, H, ny, Vdiag, Xhat, innov, Xs, Ps), model, event),
                            "qln_landing_smoother_guarded_host");
}

// The filter on recorded data (k_landing_filter).  The checks that need no handle come first.
// guarded: the estimator lands by its own guard, with its event record (may be null)
// model: the model of each record's own (qln_landing_filter_model; null: the handle's)
struct FilterCall {
    const double *Zref, *Zrec, *Lgain, *H;
    int32_t ny;
    const double *model, *Vdiag, *Y, *xhat0;
    double *Xhat, *innov, *score, *loglik, *event_hat;
    bool guarded;
};

static int check_landing_filter_args(const qln_handle* h, const FilterCall& a, const char* who) {
    const std::string w(who);
    if (int rc = check_tracking_ny(a.ny, w)) return rc;
    if (int rc = check_some_output(a.Xhat || a.innov || a.score || a.loglik || a.event_hat, w)) return rc;
    if (a.score || a.loglik) {
        if (!a.Vdiag) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null Vdiag with score or loglik");
        if (int rc = check_tracking_vdiag(a.Vdiag, a.ny, w)) return rc;
    }
    if (!a.H || !a.Lgain || !a.Y) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null H, Lgain or Y");
    if (int rc = check_handle(h)) return rc;
    if (!a.Zref) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null Zref");
    if (!a.Zrec) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null Zrec");
    return QLN_OK;
}

static int landing_filter(qln_handle* h, MemForm mem, const FilterCall& a, const char* who) {
    if (int rc = check_landing_filter_args(h, a, who)) return rc;
    // the rows, gains, measurements and innovations of the call's ny, of the roles' eight
    const int64_t ng = tracking_gain_total(h->dims, a.ny), nm = tracking_meas_total(h->dims, a.ny);
    const HostArgs args = {copy_in(kZ, a.Zref), copy_in(kZrec, a.Zrec), copy_in(kLgain, a.Lgain).sized(ng),
                           copy_in(kH, a.H).sized((int64_t)a.ny * QLN_NX), copy_in(kModel, a.model), copy_in(kY, a.Y).sized(nm),
                           copy_in(kXhat0, a.xhat0), copy_out(kXhat, a.Xhat), copy_out(kInnov, a.innov).sized(nm),
                           copy_out(kScore, a.score), copy_out(kLoglik, a.loglik), copy_out(kEventHat, a.event_hat)};
    return run_tracking_call(h, mem, args, who, [&](double* const* d, bool) {
        return qln::launch_landing_filter(h->p, d[kZ], d[kZrec], d[kLgain], d[kH], a.ny, a.Vdiag, d[kY], d[kXhat0], d[kModel],
                                          d[kXhat], d[kInnov], d[kScore], d[kLoglik], a.guarded, d[kEventHat], h->stream);
    });
}

static FilterCall filter_call(const double* Zref, const double* Zrec, const double* Lgain, const double* H, int32_t ny,
                              const double* Vdiag, const double* Y, const double* xhat0, double* Xhat, double* innov, double* score,
                              double* loglik, bool guarded, double* event_hat) {
    FilterCall a{};
    a.Zref = Zref; a.Zrec = Zrec; a.Lgain = Lgain; a.H = H; a.ny = ny; a.Vdiag = Vdiag; a.Y = Y; a.xhat0 = xhat0;
    a.Xhat = Xhat; a.innov = innov; a.score = score; a.loglik = loglik; a.guarded = guarded; a.event_hat = event_hat;
    return a;
}

int qln_landing_filter(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H, int32_t ny,
                       const double* Vdiag, const double* Y, const double* xhat0, double* Xhat, double* innov, double* score,
                       double* loglik) {
    return landing_filter(h, kDeviceMem,
                          filter_call(Zref, Zrec, Lgain, H, ny, Vdiag, Y, xhat0, Xhat, innov, score, loglik, false, nullptr),
                          "qln_landing_filter");
}
int qln_landing_filter_host(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H, int32_t ny,
                            const double* Vdiag, const double* Y, const double* xhat0, double* Xhat, double* innov, double* score,
                            double* loglik) {
    return landing_filter(h, kHostMem,
                          filter_call(Zref, Zrec, Lgain, H, ny, Vdiag, Y, xhat0, Xhat, innov, score, loglik, false, nullptr),
                          "qln_landing_filter_host");
}
int qln_landing_filter_guarded(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H,
                               int32_t ny, const double* Vdiag, const double* Y, const double* xhat0, double* Xhat, double* innov,
                               double* score, double* loglik, double* event_hat) {
    return landing_filter(h, kDeviceMem,
                          filter_call(Zref, Zrec, Lgain, H, ny, Vdiag, Y, xhat0, Xhat, innov, score, loglik, true, event_hat),
                          "qln_landing_filter_guarded");
}
int qln_landing_filter_guarded_host(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H,
                                    int32_t ny, const double* Vdiag, const double* Y, const double* xhat0, double* Xhat,
                                    double* innov, double* score, double* loglik, double* event_hat) {
    return landing_filter(h, kHostMem,
                          filter_call(Zref, Zrec, Lgain, H, ny, Vdiag, Y, xhat0, Xhat, innov, score, loglik, true, event_hat),
                          "qln_landing_filter_guarded_host");
}
// the filter at a model of each record's own: the same path with model [B][QLN_MODEL_NP] (null: the handle's)
static FilterCall with_model(FilterCall a, const double* model) {
    a.model = model;
    return a;
}
int qln_landing_filter_model(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H, int32_t ny,
                             const double* model, const double* Vdiag, const double* Y, const double* xhat0, double* Xhat,
                             double* innov, double* score, double* loglik) {
    return landing_filter(h, kDeviceMem,
                          with_model(filter_call(Zref, Zrec, Lgain, H, ny, Vdiag, Y, xhat0, Xhat, innov, score, loglik, false,
                                                 nullptr), model), "qln_landing_filter_model");
}
int qln_landing_filter_model_host(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H,
                                  int32_t ny, const double* model, const double* Vdiag, const double* Y, const double* xhat0,
                                  double* Xhat, double* innov, double* score, double* loglik) {
    return landing_filter(h, kHostMem,
                          with_model(filter_call(Zref, Zrec, Lgain, H, ny, Vdiag, Y, xhat0, Xhat, innov, score, loglik, false,
                                                 nullptr), model), "qln_landing_filter_model_host");
}
int qln_landing_filter_guarded_model(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H,
                                     int32_t ny, const double* model, const double* Vdiag, const double* Y, const double* xhat0,
                                     double* Xhat, double* innov, double* score, double* loglik, double* event_hat) {
    return landing_filter(h, kDeviceMem,
                          with_model(filter_call(Zref, Zrec, Lgain, H, ny, Vdiag, Y, xhat0, Xhat, innov, score, loglik, true,
                                                 event_hat), model), "qln_landing_filter_guarded_model");
}
int qln_landing_filter_guarded_model_host(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain,
                                          const double* H, int32_t ny, const double* model, const double* Vdiag, const double* Y,
                                          const double* xhat0, double* Xhat, double* innov, double* score, double* loglik,
                                          double* event_hat) {
    return landing_filter(h, kHostMem,
                          with_model(filter_call(Zref, Zrec, Lgain, H, ny, Vdiag, Y, xhat0, Xhat, innov, score, loglik, true,
                                                 event_hat), model), "qln_landing_filter_guarded_model_host");
}

// The sweeps through the filter (k_landing_filter_jvp / _vjp).  What both share: the record and the trajectory the filter
// produced.  The checks that need no handle come first.  guarded: the sweeps through the estimator's own touchdown, which need
// its record event_hat.
struct FilterTraj {
    const double *Zref, *Zrec, *Lgain, *H;
    int32_t ny;
    const double *model, *Vdiag, *Xhat, *innov, *event_hat;
    bool guarded;
};

// want_gain: a tangent or cotangent of Lgain is asked for; want_score: one of nis or loglik.  They exclude each other (log det S_k
// depends on the gains, and its derivative is not offered), and either needs innov; the score also needs Vdiag.
static int check_filter_sweep_args(const qln_handle* h, const FilterTraj& t, bool want_gain, bool want_score, bool forward,
                                   const std::string& w) {
    if (want_gain && want_score)
        return fail(QLN_ERR_INVALID_ARGUMENT,
                    w + (forward ? ": Lgain_dot with nis_dot or loglik_dot (the score is differentiated at fixed gains)"
                                 : ": Lgain_bar with nis_bar or loglik_bar (the score is differentiated at fixed gains)"));
    if (want_score) {
        if (!t.Vdiag) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null Vdiag with a score term");
        if (int rc = check_tracking_vdiag(t.Vdiag, t.ny, w)) return rc;
    }
    if ((want_gain || want_score) && !t.innov)
        return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null innov (Lgain's tangent or cotangent and the score terms need the innovations)");
    if (t.guarded && !t.event_hat) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null event_hat (the guarded filter's record)");
    if (!t.H || !t.Lgain) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null H or Lgain");
    if (int rc = check_handle(h)) return rc;
    if (!t.Zref || !t.Zrec || !t.Xhat) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null Zref, Zrec or Xhat");
    return QLN_OK;
}

static qln::FilterSweepIn filter_sweep_in(double* const* d, const FilterTraj& t, bool want_score) {
    qln::FilterSweepIn in = {d[kZrec], d[kLgain], d[kH], t.ny, d[kModel], d[kXhat], d[kInnov], d[kEventHat], {}};
    for (int r = 0; r < QLN_TRACK_NY_MAX; ++r) in.iv[r] = (want_score && r < t.ny) ? 1.0 / t.Vdiag[r] : 1.0;
    return in;
}

// Zref is not read (it has no tangent, and Y already is the reading minus H x_ref): it is checked, ruled and never staged.
// innov is staged, and ruled, only where it is read.
static int landing_filter_jvp(qln_handle* h, MemForm mem, const FilterTraj& t, const qln::FilterJvpArgs& a, const char* who) {
    const std::string w(who);
    if (int rc = check_tracking_ny(t.ny, w)) return rc;
    if (!a.Y_dot && !a.Zrec_dot && !a.Lgain_dot && !a.xhat0_dot && !a.model_dot)
        return fail(QLN_ERR_INVALID_ARGUMENT, w + ": every tangent is NULL (no direction)");
    if (int rc = check_some_output(a.Xhat_dot || a.innov_dot || a.nis_dot || a.loglik_dot || a.event_hat_dot, w)) return rc;
    const bool want_gain = a.Lgain_dot != nullptr, want_score = a.nis_dot || a.loglik_dot;
    if (int rc = check_filter_sweep_args(h, t, want_gain, want_score, true, w)) return rc;
    const int64_t ng = tracking_gain_total(h->dims, t.ny), nm = tracking_meas_total(h->dims, t.ny);
    const bool want_innov = want_gain || want_score;
    const HostArgs args = {copy_in(kZ, t.Zref).staged_if(false), copy_in(kZrec, t.Zrec), copy_in(kLgain, t.Lgain).sized(ng),
                           copy_in(kH, t.H).sized((int64_t)t.ny * QLN_NX), copy_in(kModel, t.model), copy_in(kXhat, t.Xhat),
                           copy_in(kInnov, t.innov).sized(nm).ruled_if(want_innov).staged_if(want_innov),
                           copy_in(kEventHat, t.event_hat), copy_in(kY, a.Y_dot).sized(nm), copy_in(kZdot, a.Zrec_dot),
                           copy_in(kLgainD, a.Lgain_dot).sized(ng), copy_in(kXhat0, a.xhat0_dot), copy_in(kModelD, a.model_dot),
                           copy_out(kXhatD, a.Xhat_dot), copy_out(kInnovD, a.innov_dot).sized(nm), copy_out(kNisD, a.nis_dot),
                           copy_out(kLoglik, a.loglik_dot), copy_out(kEventHatD, a.event_hat_dot)};
    return run_tracking_call(h, mem, args, who, [&](double* const* d, bool) {
        const qln::FilterJvpArgs da = {d[kY], d[kZdot], d[kLgainD], d[kXhat0], d[kModelD], d[kXhatD], d[kInnovD], d[kNisD],
                                       d[kLoglik], d[kEventHatD]};
        return qln::launch_landing_filter_jvp(h->p, filter_sweep_in(d, t, want_score), da, h->stream);
    });
}

// Zrec_bar is in-out: the kernel never writes behind n_nlp, and that padding is the caller's.
static int landing_filter_vjp(qln_handle* h, MemForm mem, const FilterTraj& t, const qln::FilterVjpArgs& a, const char* who) {
    const std::string w(who);
    if (int rc = check_tracking_ny(t.ny, w)) return rc;
    if (!a.Xhat_bar && !a.innov_bar && !a.nis_bar && !a.loglik_bar)
        return fail(QLN_ERR_INVALID_ARGUMENT, w + ": every cotangent is NULL (nothing to pull back)");
    if (int rc = check_some_output(a.Y_bar || a.Zrec_bar || a.Lgain_bar || a.xhat0_bar || a.model_bar, w)) return rc;
    const bool want_gain = a.Lgain_bar != nullptr, want_score = a.nis_bar || a.loglik_bar;
    if (int rc = check_filter_sweep_args(h, t, want_gain, want_score, false, w)) return rc;
    const int64_t ng = tracking_gain_total(h->dims, t.ny), nm = tracking_meas_total(h->dims, t.ny);
    const bool want_innov = want_gain || want_score;
    const HostArgs args = {copy_in(kZ, t.Zref).staged_if(false), copy_in(kZrec, t.Zrec), copy_in(kLgain, t.Lgain).sized(ng),
                           copy_in(kH, t.H).sized((int64_t)t.ny * QLN_NX), copy_in(kModel, t.model), copy_in(kXhat, t.Xhat),
                           copy_in(kInnov, t.innov).sized(nm).ruled_if(want_innov).staged_if(want_innov),
                           copy_in(kEventHat, t.event_hat), copy_in(kXhatD, a.Xhat_bar), copy_in(kInnovD, a.innov_bar).sized(nm),
                           copy_in(kNisD, a.nis_bar), copy_in(kLoglik, a.loglik_bar), copy_out(kY, a.Y_bar).sized(nm),
                           copy_inout(kZio, a.Zrec_bar), copy_out(kLgainD, a.Lgain_bar).sized(ng), copy_out(kXhat0, a.xhat0_bar),
                           copy_out(kModelD, a.model_bar)};
    return run_tracking_call(h, mem, args, who, [&](double* const* d, bool) {
        const qln::FilterVjpArgs da = {d[kXhatD], d[kInnovD], d[kNisD], d[kLoglik], d[kY], d[kZio], d[kLgainD], d[kXhat0],
                                       d[kModelD]};
        return qln::launch_landing_filter_vjp(h->p, filter_sweep_in(d, t, want_score), da, h->stream);
    });
}

static FilterTraj filter_traj(const double* Zref, const double* Zrec, const double* Lgain, const double* H, int32_t ny,
                              const double* model, const double* Vdiag, const double* Xhat, const double* innov, bool guarded,
                              const double* event_hat) {
    FilterTraj t{};
    t.Zref = Zref; t.Zrec = Zrec; t.Lgain = Lgain; t.H = H; t.ny = ny; t.model = model; t.Vdiag = Vdiag; t.Xhat = Xhat;
    t.innov = innov; t.guarded = guarded; t.event_hat = event_hat;
    return t;
}

int qln_landing_filter_jvp(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H, int32_t ny,
                           const double* model, const double* Vdiag, const double* Xhat, const double* innov, const double* Y_dot,
                           const double* Zrec_dot, const double* Lgain_dot, const double* xhat0_dot, const double* model_dot,
                           double* Xhat_dot, double* innov_dot, double* nis_dot, double* loglik_dot) {
    return landing_filter_jvp(h, kDeviceMem, filter_traj(Zref, Zrec, Lgain, H, ny, model, Vdiag, Xhat, innov, false, nullptr),
                              qln::FilterJvpArgs{Y_dot, Zrec_dot, Lgain_dot, xhat0_dot, model_dot, Xhat_dot, innov_dot, nis_dot,
                                                 loglik_dot, nullptr}, "qln_landing_filter_jvp");
}
int qln_landing_filter_jvp_host(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H,
                                int32_t ny, const double* model, const double* Vdiag, const double* Xhat, const double* innov,
                                const double* Y_dot, const double* Zrec_dot, const double* Lgain_dot, const double* xhat0_dot,
                                const double* model_dot, double* Xhat_dot, double* innov_dot, double* nis_dot, double* loglik_dot) {
    return landing_filter_jvp(h, kHostMem, filter_traj(Zref, Zrec, Lgain, H, ny, model, Vdiag, Xhat, innov, false, nullptr),
                              qln::FilterJvpArgs{Y_dot, Zrec_dot, Lgain_dot, xhat0_dot, model_dot, Xhat_dot, innov_dot, nis_dot,
                                                 loglik_dot, nullptr}, "qln_landing_filter_jvp_host");
}
int qln_landing_filter_guarded_jvp(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H,
                                   int32_t ny, const double* model, const double* Vdiag, const double* Xhat, const double* innov,
                                   const double* event_hat, const double* Y_dot, const double* Zrec_dot, const double* Lgain_dot,
                                   const double* xhat0_dot, const double* model_dot, double* Xhat_dot, double* innov_dot,
                                   double* nis_dot, double* loglik_dot, double* event_hat_dot) {
    return landing_filter_jvp(h, kDeviceMem, filter_traj(Zref, Zrec, Lgain, H, ny, model, Vdiag, Xhat, innov, true, event_hat),
                              qln::FilterJvpArgs{Y_dot, Zrec_dot, Lgain_dot, xhat0_dot, model_dot, Xhat_dot, innov_dot, nis_dot,
                                                 loglik_dot, event_hat_dot}, "qln_landing_filter_guarded_jvp");
}
int qln_landing_filter_guarded_jvp_host(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H,
                                        int32_t ny, const double* model, const double* Vdiag, const double* Xhat,
                                        const double* innov, const double* event_hat, const double* Y_dot, const double* Zrec_dot,
                                        const double* Lgain_dot, const double* xhat0_dot, const double* model_dot,
                                        double* Xhat_dot, double* innov_dot, double* nis_dot, double* loglik_dot,
                                        double* event_hat_dot) {
    return landing_filter_jvp(h, kHostMem, filter_traj(Zref, Zrec, Lgain, H, ny, model, Vdiag, Xhat, innov, true, event_hat),
                              qln::FilterJvpArgs{Y_dot, Zrec_dot, Lgain_dot, xhat0_dot, model_dot, Xhat_dot, innov_dot, nis_dot,
                                                 loglik_dot, event_hat_dot}, "qln_landing_filter_guarded_jvp_host");
}
int qln_landing_filter_vjp(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H, int32_t ny,
                           const double* model, const double* Vdiag, const double* Xhat, const double* innov,
                           const double* Xhat_bar, const double* innov_bar, const double* nis_bar, const double* loglik_bar,
                           double* Y_bar, double* Zrec_bar, double* Lgain_bar, double* xhat0_bar, double* model_bar) {
    return landing_filter_vjp(h, kDeviceMem, filter_traj(Zref, Zrec, Lgain, H, ny, model, Vdiag, Xhat, innov, false, nullptr),
                              qln::FilterVjpArgs{Xhat_bar, innov_bar, nis_bar, loglik_bar, Y_bar, Zrec_bar, Lgain_bar, xhat0_bar,
                                                 model_bar}, "qln_landing_filter_vjp");
}
int qln_landing_filter_vjp_host(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H,
                                int32_t ny, const double* model, const double* Vdiag, const double* Xhat, const double* innov,
                                const double* Xhat_bar, const double* innov_bar, const double* nis_bar, const double* loglik_bar,
                                double* Y_bar, double* Zrec_bar, double* Lgain_bar, double* xhat0_bar, double* model_bar) {
    return landing_filter_vjp(h, kHostMem, filter_traj(Zref, Zrec, Lgain, H, ny, model, Vdiag, Xhat, innov, false, nullptr),
                              qln::FilterVjpArgs{Xhat_bar, innov_bar, nis_bar, loglik_bar, Y_bar, Zrec_bar, Lgain_bar, xhat0_bar,
                                                 model_bar}, "qln_landing_filter_vjp_host");
}
int qln_landing_filter_guarded_vjp(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H,
                                   int32_t ny, const double* model, const double* Vdiag, const double* Xhat, const double* innov,
                                   const double* event_hat, const double* Xhat_bar, const double* innov_bar, const double* nis_bar,
                                   const double* loglik_bar, double* Y_bar, double* Zrec_bar, double* Lgain_bar, double* xhat0_bar,
                                   double* model_bar) {
    return landing_filter_vjp(h, kDeviceMem, filter_traj(Zref, Zrec, Lgain, H, ny, model, Vdiag, Xhat, innov, true, event_hat),
                              qln::FilterVjpArgs{Xhat_bar, innov_bar, nis_bar, loglik_bar, Y_bar, Zrec_bar, Lgain_bar, xhat0_bar,
                                                 model_bar}, "qln_landing_filter_guarded_vjp");
}
int qln_landing_filter_guarded_vjp_host(qln_handle* h, const double* Zref, const double* Zrec, const double* Lgain, const double* H,
                                        int32_t ny, const double* model, const double* Vdiag, const double* Xhat,
                                        const double* innov, const double* event_hat, const double* Xhat_bar,
                                        const double* innov_bar, const double* nis_bar, const double* loglik_bar, double* Y_bar,
                                        double* Zrec_bar, double* Lgain_bar, double* xhat0_bar, double* model_bar) {
    return landing_filter_vjp(h, kHostMem, filter_traj(Zref, Zrec, Lgain, H, ny, model, Vdiag, Xhat, innov, true, event_hat),
                              qln::FilterVjpArgs{Xhat_bar, innov_bar, nis_bar, loglik_bar, Y_bar, Zrec_bar, Lgain_bar, xhat0_bar,
                                                 model_bar}, "qln_landing_filter_guarded_vjp_host");
}

// The estimate-feedback roll-out (k_tracking_rollout_estimated).  The checks that need no handle come first.
// guarded: both the plant and the estimator land by their own guards, each with an event record (may be null)
// limited: the loop within the force limits lim, with its saturation record sat (may be null)
struct EstimatedCall {
    const double *Zref, *K, *Lgain, *H;
    int32_t ny;
    const double *vnoise, *wnoise, *x0, *xhat0, *model, *lim;
    double *Zout, *Xhat, *innov, *event, *event_hat, *sat;
    bool guarded, limited;
};

static int check_tracking_estimated_args(const qln_handle* h, const EstimatedCall& a, const char* who) {
    const std::string w(who);
    if (a.limited) {
        if (int rc = check_force_limits(a.lim, who)) return rc;
        if (!a.guarded && (a.event || a.event_hat))
            return fail(QLN_ERR_INVALID_ARGUMENT, w + ": event or event_hat with guarded == 0 (the knot schedule has no record)");
    }
    if (int rc = check_tracking_ny(a.ny, w)) return rc;
    if (!a.Lgain || !a.H) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null Lgain or H");
    if (int rc = check_handle(h)) return rc;
    if (!a.Zref || !a.Zout) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null Zref or Zout");
    return QLN_OK;
}

static int tracking_rollout_estimated(qln_handle* h, MemForm mem, const EstimatedCall& a, const char* who) {
    if (int rc = check_tracking_estimated_args(h, a, who)) return rc;
    // the rows, gains, samples and innovations of the call's ny, of the roles' eight
    const int64_t ng = tracking_gain_total(h->dims, a.ny), nm = tracking_meas_total(h->dims, a.ny);
    const HostArgs args = {copy_in(kZ, a.Zref), copy_inout(kZio, a.Zout), copy_in(kK, a.K), copy_in(kLgain, a.Lgain).sized(ng),
                           copy_in(kH, a.H).sized((int64_t)a.ny * QLN_NX), copy_in(kVnoise, a.vnoise).sized(nm),
                           copy_in(kWnoise, a.wnoise), copy_in(kX0, a.x0), copy_in(kXhat0, a.xhat0), copy_in(kModel, a.model),
                           copy_out(kXhat, a.Xhat), copy_out(kInnov, a.innov).sized(nm), copy_out(kEvent, a.event),
                           copy_out(kEventHat, a.event_hat), copy_out(kSat, a.sat)};
    return run_tracking_call(h, mem, args, who, [&](double* const* d, bool) {
        return qln::launch_tracking_rollout_estimated(h->p, d[kZ], d[kK], d[kLgain], d[kH], a.ny, d[kVnoise], d[kWnoise], d[kX0],
                                                      d[kXhat0], d[kModel], d[kZio], d[kXhat], d[kInnov], a.guarded, d[kEvent],
                                                      d[kEventHat], a.limited ? a.lim : nullptr, d[kSat], h->stream);
    });
}

static EstimatedCall estimated_call(const double* Zref, const double* K, const double* Lgain, const double* H, int32_t ny,
                                    const double* vnoise, const double* wnoise, const double* x0, const double* xhat0,
                                    const double* model, double* Zout, double* Xhat, double* innov) {
    EstimatedCall a{};
    a.Zref = Zref; a.K = K; a.Lgain = Lgain; a.H = H; a.ny = ny; a.vnoise = vnoise; a.wnoise = wnoise;
    a.x0 = x0; a.xhat0 = xhat0; a.model = model; a.Zout = Zout; a.Xhat = Xhat; a.innov = innov;
    return a;
}
static EstimatedCall with_touchdown(EstimatedCall a, double* event, double* event_hat) {
    a.guarded = true; a.event = event; a.event_hat = event_hat;
    return a;
}
static EstimatedCall within_limits(EstimatedCall a, const double* lim, int32_t guarded, double* event, double* event_hat,
                                   double* sat) {
    a.limited = true; a.lim = lim; a.sat = sat; a.guarded = guarded != 0; a.event = event; a.event_hat = event_hat;
    return a;
}

int qln_tracking_rollout_estimated(qln_handle* h, const double* Zref, const double* K, const double* Lgain, const double* H,
                                   int32_t ny, const double* vnoise, const double* wnoise, const double* x0, const double* xhat0,
                                   const double* model, double* Zout, double* Xhat, double* innov) {
    return tracking_rollout_estimated(h, kDeviceMem,
                                      estimated_call(Zref, K, Lgain, H, ny, vnoise, wnoise, x0, xhat0, model, Zout, Xhat, innov),
                                      "qln_tracking_rollout_estimated");
}
int qln_tracking_rollout_estimated_host(qln_handle* h, const double* Zref, const double* K, const double* Lgain, const double* H,
                                        int32_t ny, const double* vnoise, const double* wnoise, const double* x0,
                                        const double* xhat0, const double* model, double* Zout, double* Xhat, double* innov) {
    return tracking_rollout_estimated(h, kHostMem,
                                      estimated_call(Zref, K, Lgain, H, ny, vnoise, wnoise, x0, xhat0, model, Zout, Xhat, innov),
                                      "qln_tracking_rollout_estimated_host");
}
int qln_tracking_rollout_estimated_guarded(qln_handle* h, const double* Zref, const double* K, const double* Lgain, const double* H,
                                           int32_t ny, const double* vnoise, const double* wnoise, const double* x0,
                                           const double* xhat0, const double* model, double* Zout, double* Xhat, double* innov,
                                           double* event, double* event_hat) {
    return tracking_rollout_estimated(h, kDeviceMem,
                                      with_touchdown(estimated_call(Zref, K, Lgain, H, ny, vnoise, wnoise, x0, xhat0, model, Zout,
                                                                    Xhat, innov), event, event_hat),
                                      "qln_tracking_rollout_estimated_guarded");
}
int qln_tracking_rollout_estimated_guarded_host(qln_handle* h, const double* Zref, const double* K, const double* Lgain,
                                                const double* H, int32_t ny, const double* vnoise, const double* wnoise,
                                                const double* x0, const double* xhat0, const double* model, double* Zout,
                                                double* Xhat, double* innov, double* event, double* event_hat) {
    return tracking_rollout_estimated(h, kHostMem,
                                      with_touchdown(estimated_call(Zref, K, Lgain, H, ny, vnoise, wnoise, x0, xhat0, model, Zout,
                                                                    Xhat, innov), event, event_hat),
                                      "qln_tracking_rollout_estimated_guarded_host");
}
// the loop within contact-aware force limits: the knot-scheduled or the guarded one, with its saturation record
int qln_tracking_rollout_estimated_limited(qln_handle* h, const double* Zref, const double* K, const double* Lgain, const double* H,
                                           int32_t ny, const double* vnoise, const double* wnoise, const double* x0,
                                           const double* xhat0, const double* model, const double* lim, int32_t guarded,
                                           double* Zout, double* Xhat, double* innov, double* event, double* event_hat,
                                           double* sat) {
    return tracking_rollout_estimated(h, kDeviceMem,
                                      within_limits(estimated_call(Zref, K, Lgain, H, ny, vnoise, wnoise, x0, xhat0, model, Zout,
                                                                   Xhat, innov), lim, guarded, event, event_hat, sat),
                                      "qln_tracking_rollout_estimated_limited");
}
int qln_tracking_rollout_estimated_limited_host(qln_handle* h, const double* Zref, const double* K, const double* Lgain,
                                                const double* H, int32_t ny, const double* vnoise, const double* wnoise,
                                                const double* x0, const double* xhat0, const double* model, const double* lim,
                                                int32_t guarded, double* Zout, double* Xhat, double* innov, double* event,
                                                double* event_hat, double* sat) {
    return tracking_rollout_estimated(h, kHostMem,
                                      within_limits(estimated_call(Zref, K, Lgain, H, ny, vnoise, wnoise, x0, xhat0, model, Zout,
                                                                   Xhat, innov), lim, guarded, event, event_hat, sat),
                                      "qln_tracking_rollout_estimated_limited_host");
}

// The sweeps through the estimate-feedback roll-out (k_tracking_rollout_estimated_jvp / _vjp).  What both sweeps share: the
// roll-out's inputs and the trajectory it produced.  The checks that need no handle come first.
// guarded: the sweeps through the two guard-triggered touchdowns, which need both of the roll-out's event records
// sat: the limited roll-out's saturation record, required by the sweeps at its active set (limited), whose event and event_hat
// -- both or neither -- select the guarded or the knot-scheduled blocks
struct EstimatedTraj {
    const double *Zref, *K, *Lgain, *H;
    int32_t ny;
    const double *model, *Zout, *Xhat, *innov, *event, *event_hat, *sat;
    bool guarded, limited;
};

// want_gain: a tangent or cotangent of Lgain is asked for, which needs innov
static int check_tracking_estimated_sweep_args(const qln_handle* h, const EstimatedTraj& t, bool want_gain,
                                               const std::string& w) {
    if (int rc = check_tracking_ny(t.ny, w)) return rc;
    if (!t.Lgain || !t.H) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null Lgain or H");
    if (int rc = check_limited_sat(t.limited, t.sat, w)) return rc;
    if (t.limited && (t.event != nullptr) != (t.event_hat != nullptr))
        return fail(QLN_ERR_INVALID_ARGUMENT, w + ": exactly one of event and event_hat (both: the guarded blocks, neither: the "
                                                  "knot-scheduled ones)");
    if (t.guarded && (!t.event || !t.event_hat))
        return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null event or event_hat (the guarded roll-out's two records)");
    if (want_gain && !t.innov)
        return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null innov (the tangent or cotangent of Lgain needs the innovations)");
    if (!t.Zref || !t.Zout || !t.Xhat) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null Zref, Zout or Xhat");
    return check_handle(h);
}

static int check_tracking_estimated_jvp_args(const qln_handle* h, const EstimatedTraj& t, const qln::EstimatedJvpArgs& a,
                                             const char* who) {
    const std::string w(who);
    if (!a.Zref_dot && !a.K_dot && !a.Lgain_dot && !a.x0_dot && !a.xhat0_dot && !a.model_dot)
        return fail(QLN_ERR_INVALID_ARGUMENT, w + ": every tangent is NULL (no direction)");
    if (a.K_dot && !t.K) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": K_dot needs K (K == NULL has no gains to perturb)");
    if (!a.Zout_dot) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null Zout_dot");
    if (t.limited && !t.event && !t.event_hat && (a.event_dot || a.event_hat_dot))
        return fail(QLN_ERR_INVALID_ARGUMENT, w + ": event_dot or event_hat_dot without event and event_hat (the knot-scheduled "
                                                  "sweep has no record)");
    return check_tracking_estimated_sweep_args(h, t, a.Lgain_dot != nullptr, w);
}

static int check_tracking_estimated_vjp_args(const qln_handle* h, const EstimatedTraj& t, const qln::EstimatedVjpArgs& a,
                                             const char* who) {
    const std::string w(who);
    if (a.K_bar && !t.K) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": K_bar needs K (K == NULL has no gains to differentiate)");
    if (!a.Zbar) return fail(QLN_ERR_INVALID_ARGUMENT, w + ": null Zbar");
    return check_tracking_estimated_sweep_args(h, t, a.Lgain_bar != nullptr, w);
}

// the trajectory as the launch reads it: Zout's buffer stands in for a Zref the host form did not stage
static qln::EstimatedSweepIn estimated_sweep_in(double* const* d, int32_t ny) {
    return {d[kZ] ? d[kZ] : d[kV], d[kK], d[kLgain], d[kH], ny, d[kModel], d[kV], d[kXhat], d[kInnov], d[kEvent], d[kEventHat]};
}

// The host form stages Zref only when K_dot is given (the kernel reads it for nothing else), and innov only with Lgain_dot,
// which is also when the overlap rule looks at innov.  Lgain, H, innov and their tangents have the extent of the call's ny.
// The saturation record stands before the event records: the host form has always looked at its values first.
static int tracking_estimated_jvp(qln_handle* h, MemForm mem, const EstimatedTraj& t, const qln::EstimatedJvpArgs& a,
                                  const char* who) {
    if (int rc = check_tracking_estimated_jvp_args(h, t, a, who)) return rc;
    const int64_t ng = tracking_gain_total(h->dims, t.ny), nm = tracking_meas_total(h->dims, t.ny);
    const bool want_gain = a.Lgain_dot != nullptr;
    const HostArgs args = {copy_in(kV, t.Zout), copy_in(kZ, t.Zref).staged_if(a.K_dot != nullptr), copy_in(kK, t.K),
                           copy_in(kLgain, t.Lgain).sized(ng), copy_in(kH, t.H).sized((int64_t)t.ny * QLN_NX),
                           copy_in(kModel, t.model), copy_in(kXhat, t.Xhat),
                           copy_in(kInnov, t.innov).sized(nm).ruled_if(want_gain).staged_if(want_gain),
                           copy_in(kSat, t.sat), copy_in(kEvent, t.event), copy_in(kEventHat, t.event_hat),
                           copy_in(kZdot, a.Zref_dot), copy_in(kKdot, a.K_dot), copy_in(kLgainD, a.Lgain_dot).sized(ng),
                           copy_in(kX0, a.x0_dot), copy_in(kXhat0, a.xhat0_dot), copy_in(kModelD, a.model_dot),
                           copy_inout(kZio, a.Zout_dot), copy_out(kXhatD, a.Xhat_dot), copy_out(kInnovD, a.innov_dot).sized(nm),
                           copy_out(kEventD, a.event_dot), copy_out(kEventHatD, a.event_hat_dot)};
    return run_tracking_call(h, mem, args, who, [&](double* const* d, bool) {
        const qln::EstimatedJvpArgs da = {d[kZdot], d[kKdot], d[kLgainD], d[kX0], d[kXhat0], d[kModelD], d[kZio], d[kXhatD],
                                          d[kInnovD], d[kEventD], d[kEventHatD]};
        return qln::launch_tracking_rollout_estimated_jvp(h->p, estimated_sweep_in(d, t.ny), da, d[kSat], h->stream);
    });
}

// Zref with K_bar and innov with Lgain_bar, as in the forward sweep.
static int tracking_estimated_vjp(qln_handle* h, MemForm mem, const EstimatedTraj& t, const qln::EstimatedVjpArgs& a,
                                  const char* who) {
    if (int rc = check_tracking_estimated_vjp_args(h, t, a, who)) return rc;
    const int64_t ng = tracking_gain_total(h->dims, t.ny), nm = tracking_meas_total(h->dims, t.ny);
    const bool want_gain = a.Lgain_bar != nullptr;
    const HostArgs args = {copy_in(kV, t.Zout), copy_in(kZ, t.Zref).staged_if(a.K_bar != nullptr), copy_in(kK, t.K),
                           copy_in(kLgain, t.Lgain).sized(ng), copy_in(kH, t.H).sized((int64_t)t.ny * QLN_NX),
                           copy_in(kModel, t.model), copy_in(kXhat, t.Xhat),
                           copy_in(kInnov, t.innov).sized(nm).ruled_if(want_gain).staged_if(want_gain),
                           copy_in(kSat, t.sat), copy_in(kEvent, t.event), copy_in(kEventHat, t.event_hat),
                           copy_in(kZbar, a.Zbar), copy_in(kXhatD, a.Xhat_bar), copy_in(kInnovD, a.innov_bar).sized(nm),
                           copy_inout(kZio, a.Zref_bar), copy_out(kKbar, a.K_bar), copy_out(kLgainD, a.Lgain_bar).sized(ng),
                           copy_out(kX0, a.x0_bar), copy_out(kXhat0, a.xhat0_bar), copy_out(kModelD, a.model_bar)};
    return run_tracking_call(h, mem, args, who, [&](double* const* d, bool) {
        const qln::EstimatedVjpArgs da = {d[kZbar], d[kXhatD], d[kInnovD], d[kZio], d[kKbar], d[kLgainD], d[kX0], d[kXhat0],
                                          d[kModelD]};
        return qln::launch_tracking_rollout_estimated_vjp(h->p, estimated_sweep_in(d, t.ny), da, d[kSat], h->stream);
    });
}

static EstimatedTraj estimated_traj(const double* Zref, const double* K, const double* Lgain, const double* H, int32_t ny,
                                    const double* model, const double* Zout, const double* Xhat, const double* innov) {
    EstimatedTraj t{};
    t.Zref = Zref; t.K = K; t.Lgain = Lgain; t.H = H; t.ny = ny; t.model = model; t.Zout = Zout; t.Xhat = Xhat; t.innov = innov;
    return t;
}
static EstimatedTraj at_events(EstimatedTraj t, const double* event, const double* event_hat) {
    t.guarded = true; t.event = event; t.event_hat = event_hat;
    return t;
}
// event and event_hat -- both or neither -- then select the guarded or the knot-scheduled blocks
static EstimatedTraj at_active_set(EstimatedTraj t, const double* sat) {
    t.limited = true; t.sat = sat; t.guarded = t.event && t.event_hat;
    return t;
}

int qln_tracking_rollout_estimated_jvp(qln_handle* h, const double* Zref, const double* K, const double* Lgain, const double* H,
                                       int32_t ny, const double* model, const double* Zout, const double* Xhat,
                                       const double* innov, const double* Zref_dot, const double* K_dot, const double* Lgain_dot,
                                       const double* x0_dot, const double* xhat0_dot, const double* model_dot, double* Zout_dot,
                                       double* Xhat_dot, double* innov_dot) {
    return tracking_estimated_jvp(h, kDeviceMem, estimated_traj(Zref, K, Lgain, H, ny, model, Zout, Xhat, innov),
                                  qln::EstimatedJvpArgs{Zref_dot, K_dot, Lgain_dot, x0_dot, xhat0_dot, model_dot, Zout_dot,
                                                        Xhat_dot, innov_dot, nullptr, nullptr},
                                  "qln_tracking_rollout_estimated_jvp");
}
int qln_tracking_rollout_estimated_jvp_host(qln_handle* h, const double* Zref, const double* K, const double* Lgain,
                                            const double* H, int32_t ny, const double* model, const double* Zout,
                                            const double* Xhat, const double* innov, const double* Zref_dot, const double* K_dot,
                                            const double* Lgain_dot, const double* x0_dot, const double* xhat0_dot,
                                            const double* model_dot, double* Zout_dot, double* Xhat_dot, double* innov_dot) {
    return tracking_estimated_jvp(h, kHostMem, estimated_traj(Zref, K, Lgain, H, ny, model, Zout, Xhat, innov),
                                  qln::EstimatedJvpArgs{Zref_dot, K_dot, Lgain_dot, x0_dot, xhat0_dot, model_dot, Zout_dot,
                                                        Xhat_dot, innov_dot, nullptr, nullptr},
                                  "qln_tracking_rollout_estimated_jvp_host");
}
int qln_tracking_rollout_estimated_guarded_jvp(qln_handle* h, const double* Zref, const double* K, const double* Lgain,
                                               const double* H, int32_t ny, const double* model, const double* Zout,
                                               const double* Xhat, const double* innov, const double* event,
                                               const double* event_hat, const double* Zref_dot, const double* K_dot,
                                               const double* Lgain_dot, const double* x0_dot, const double* xhat0_dot,
                                               const double* model_dot, double* Zout_dot, double* Xhat_dot, double* innov_dot,
                                               double* event_dot, double* event_hat_dot) {
    return tracking_estimated_jvp(h, kDeviceMem,
                                  at_events(estimated_traj(Zref, K, Lgain, H, ny, model, Zout, Xhat, innov), event, event_hat),
                                  qln::EstimatedJvpArgs{Zref_dot, K_dot, Lgain_dot, x0_dot, xhat0_dot, model_dot, Zout_dot,
                                                        Xhat_dot, innov_dot, event_dot, event_hat_dot},
                                  "qln_tracking_rollout_estimated_guarded_jvp");
}
int qln_tracking_rollout_estimated_guarded_jvp_host(qln_handle* h, const double* Zref, const double* K, const double* Lgain,
                                                    const double* H, int32_t ny, const double* model, const double* Zout,
                                                    const double* Xhat, const double* innov, const double* event,
                                                    const double* event_hat, const double* Zref_dot, const double* K_dot,
                                                    const double* Lgain_dot, const double* x0_dot, const double* xhat0_dot,
                                                    const double* model_dot, double* Zout_dot, double* Xhat_dot,
                                                    double* innov_dot, double* event_dot, double* event_hat_dot) {
    return tracking_estimated_jvp(h, kHostMem,
                                  at_events(estimated_traj(Zref, K, Lgain, H, ny, model, Zout, Xhat, innov), event, event_hat),
                                  qln::EstimatedJvpArgs{Zref_dot, K_dot, Lgain_dot, x0_dot, xhat0_dot, model_dot, Zout_dot,
                                                        Xhat_dot, innov_dot, event_dot, event_hat_dot},
                                  "qln_tracking_rollout_estimated_guarded_jvp_host");
}
int qln_tracking_rollout_estimated_vjp(qln_handle* h, const double* Zref, const double* K, const double* Lgain, const double* H,
                                       int32_t ny, const double* model, const double* Zout, const double* Xhat,
                                       const double* innov, const double* Zbar, const double* Xhat_bar, const double* innov_bar,
                                       double* Zref_bar, double* K_bar, double* Lgain_bar, double* x0_bar, double* xhat0_bar,
                                       double* model_bar) {
    return tracking_estimated_vjp(h, kDeviceMem, estimated_traj(Zref, K, Lgain, H, ny, model, Zout, Xhat, innov),
                                  qln::EstimatedVjpArgs{Zbar, Xhat_bar, innov_bar, Zref_bar, K_bar, Lgain_bar, x0_bar, xhat0_bar,
                                                        model_bar}, "qln_tracking_rollout_estimated_vjp");
}
int qln_tracking_rollout_estimated_vjp_host(qln_handle* h, const double* Zref, const double* K, const double* Lgain,
                                            const double* H, int32_t ny, const double* model, const double* Zout,
                                            const double* Xhat, const double* innov, const double* Zbar, const double* Xhat_bar,
                                            const double* innov_bar, double* Zref_bar, double* K_bar, double* Lgain_bar,
                                            double* x0_bar, double* xhat0_bar, double* model_bar) {
    return tracking_estimated_vjp(h, kHostMem, estimated_traj(Zref, K, Lgain, H, ny, model, Zout, Xhat, innov),
                                  qln::EstimatedVjpArgs{Zbar, Xhat_bar, innov_bar, Zref_bar, K_bar, Lgain_bar, x0_bar, xhat0_bar,
                                                        model_bar}, "qln_tracking_rollout_estimated_vjp_host");
}
int qln_tracking_rollout_estimated_guarded_vjp(qln_handle* h, const double* Zref, const double* K, const double* Lgain,
                                               const double* H, int32_t ny, const double* model, const double* Zout,
                                               const double* Xhat, const double* innov, const double* event,
                                               const double* event_hat, const double* Zbar, const double* Xhat_bar,
                                               const double* innov_bar, double* Zref_bar, double* K_bar, double* Lgain_bar,
                                               double* x0_bar, double* xhat0_bar, double* model_bar) {
    return tracking_estimated_vjp(h, kDeviceMem,
                                  at_events(estimated_traj(Zref, K, Lgain, H, ny, model, Zout, Xhat, innov), event, event_hat),
                                  qln::EstimatedVjpArgs{Zbar, Xhat_bar, innov_bar, Zref_bar, K_bar, Lgain_bar, x0_bar, xhat0_bar,
                                                        model_bar}, "qln_tracking_rollout_estimated_guarded_vjp");
}
int qln_tracking_rollout_estimated_guarded_vjp_host(qln_handle* h, const double* Zref, const double* K, const double* Lgain,
                                                    const double* H, int32_t ny, const double* model, const double* Zout,
                                                    const double* Xhat, const double* innov, const double* event,
                                                    const double* event_hat, const double* Zbar, const double* Xhat_bar,
                                                    const double* innov_bar, double* Zref_bar, double* K_bar, double* Lgain_bar,
                                                    double* x0_bar, double* xhat0_bar, double* model_bar) {
    return tracking_estimated_vjp(h, kHostMem,
                                  at_events(estimated_traj(Zref, K, Lgain, H, ny, model, Zout, Xhat, innov), event, event_hat),
                                  qln::EstimatedVjpArgs{Zbar, Xhat_bar, innov_bar, Zref_bar, K_bar, Lgain_bar, x0_bar, xhat0_bar,
                                                        model_bar}, "qln_tracking_rollout_estimated_guarded_vjp_host");
}

// the sweeps at the limited loop's active set: the same path with its saturation record; event and event_hat select the guarded
// blocks
int qln_tracking_rollout_estimated_limited_jvp(qln_handle* h, const double* Zref, const double* K, const double* Lgain,
                                               const double* H, int32_t ny, const double* model, const double* Zout,
                                               const double* Xhat, const double* innov, const double* event,
                                               const double* event_hat, const double* sat, const double* Zref_dot,
                                               const double* K_dot, const double* Lgain_dot, const double* x0_dot,
                                               const double* xhat0_dot, const double* model_dot, double* Zout_dot,
                                               double* Xhat_dot, double* innov_dot, double* event_dot, double* event_hat_dot) {
    return tracking_estimated_jvp(h, kDeviceMem,
                                  at_active_set(at_events(estimated_traj(Zref, K, Lgain, H, ny, model, Zout, Xhat, innov), event,
                                                          event_hat), sat),
                                  qln::EstimatedJvpArgs{Zref_dot, K_dot, Lgain_dot, x0_dot, xhat0_dot, model_dot, Zout_dot,
                                                        Xhat_dot, innov_dot, event_dot, event_hat_dot},
                                  "qln_tracking_rollout_estimated_limited_jvp");
}
int qln_tracking_rollout_estimated_limited_jvp_host(qln_handle* h, const double* Zref, const double* K, const double* Lgain,
                                                    const double* H, int32_t ny, const double* model, const double* Zout,
                                                    const double* Xhat, const double* innov, const double* event,
                                                    const double* event_hat, const double* sat, const double* Zref_dot,
                                                    const double* K_dot, const double* Lgain_dot, const double* x0_dot,
                                                    const double* xhat0_dot, const double* model_dot, double* Zout_dot,
                                                    double* Xhat_dot, double* innov_dot, double* event_dot,
                                                    double* event_hat_dot) {
    return tracking_estimated_jvp(h, kHostMem,
                                  at_active_set(at_events(estimated_traj(Zref, K, Lgain, H, ny, model, Zout, Xhat, innov), event,
                                                          event_hat), sat),
                                  qln::EstimatedJvpArgs{Zref_dot, K_dot, Lgain_dot, x0_dot, xhat0_dot, model_dot, Zout_dot,
                                                        Xhat_dot, innov_dot, event_dot, event_hat_dot},
                                  "qln_tracking_rollout_estimated_limited_jvp_host");
}
int qln_tracking_rollout_estimated_limited_vjp(qln_handle* h, const double* Zref, const double* K, const double* Lgain,
                                               const double* H, int32_t ny, const double* model, const double* Zout,
                                               const double* Xhat, const double* innov, const double* event,
                                               const double* event_hat, const double* sat, const double* Zbar,
                                               const double* Xhat_bar, const double* innov_bar, double* Zref_bar, double* K_bar,
                                               double* Lgain_bar, double* x0_bar, double* xhat0_bar, double* model_bar) {
    return tracking_estimated_vjp(h, kDeviceMem,
                                  at_active_set(at_events(estimated_traj(Zref, K, Lgain, H, ny, model, Zout, Xhat, innov), event,
                                                          event_hat), sat),
                                  qln::EstimatedVjpArgs{Zbar, Xhat_bar, innov_bar, Zref_bar, K_bar, Lgain_bar, x0_bar, xhat0_bar,
                                                        model_bar}, "qln_tracking_rollout_estimated_limited_vjp");
}
int qln_tracking_rollout_estimated_limited_vjp_host(qln_handle* h, const double* Zref, const double* K, const double* Lgain,
                                                    const double* H, int32_t ny, const double* model, const double* Zout,
                                                    const double* Xhat, const double* innov, const double* event,
                                                    const double* event_hat, const double* sat, const double* Zbar,
                                                    const double* Xhat_bar, const double* innov_bar, double* Zref_bar,
                                                    double* K_bar, double* Lgain_bar, double* x0_bar, double* xhat0_bar,
                                                    double* model_bar) {
    return tracking_estimated_vjp(h, kHostMem,
                                  at_active_set(at_events(estimated_traj(Zref, K, Lgain, H, ny, model, Zout, Xhat, innov), event,
                                                          event_hat), sat),
                                  qln::EstimatedVjpArgs{Zbar, Xhat_bar, innov_bar, Zref_bar, K_bar, Lgain_bar, x0_bar, xhat0_bar,
                                                        model_bar}, "qln_tracking_rollout_estimated_limited_vjp_host");
}

// ------------------------------------------------------------------ host-pointer (MOI) mode

int qln_eval_objective_host(qln_handle* h, const double* Z, double* f) {
    if (int rc = check_handle(h)) return rc;
    if (int rc = check_cost(h)) return rc;
    if (!Z || !f) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_eval_objective_host: null pointer");
    if (int rc = bind_device(h)) return rc;
    return host_call(h, {copy_in(kZ, Z), copy_out(kF, f)},
                     [&](double* const* d, bool) { return qln::launch_objective(h->p, d[kZ], d[kF], h->stream); });
}

int qln_eval_objective_gradient_host(qln_handle* h, const double* Z, double* grad) {
    if (int rc = check_handle(h)) return rc;
    if (int rc = check_cost(h)) return rc;
    if (!Z || !grad) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_eval_objective_gradient_host: null pointer");
    if (int rc = bind_device(h)) return rc;
    return host_call(h, {copy_in(kZ, Z), copy_out(kGrad, grad)}, [&](double* const* d, bool mapped) {
        const hipError_t e = mapped ? hipSuccess : hipMemsetAsync(d[kGrad], 0, h->dims.z_total * sizeof(double), h->stream);
        return e != hipSuccess ? e : qln::launch_objective_gradient(h->p, d[kZ], d[kGrad], h->stream);
    });
}

int qln_eval_constraint_host(qln_handle* h, const double* Z, double* c) {
    if (int rc = check_handle(h)) return rc;
    if (!Z || !c) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_eval_constraint_host: null pointer");
    if (int rc = bind_device(h)) return rc;
    return host_call(h, {copy_in(kZ, Z), copy_out(kC, c)}, [&](double* const* d, bool mapped) {
        return qln::launch_constraint_jacobian(h->p, 0, h->p.B, d[kZ], d[kC], nullptr, mapped ? qln::kLaunchSplit : 0u, h->stream);
    });
}

int qln_eval_constraint_jacobian_host(qln_handle* h, const double* Z, double* vals) {
    if (int rc = check_handle(h)) return rc;
    if (!Z || !vals) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_eval_constraint_jacobian_host: null pointer");
    if (int rc = bind_device(h)) return rc;
    return host_call(h, {copy_in(kZ, Z), copy_out(kVals, vals)}, [&](double* const* d, bool mapped) {
        return qln::launch_constraint_jacobian(h->p, 0, h->p.B, d[kZ], nullptr, d[kVals],
                                               QLN_JAC_WRITE_CONSTANTS | (mapped ? qln::kLaunchSplit : 0u), h->stream);
    });
}

// Staged only: a mapped path would change its latency with no measurement behind it.
int qln_eval_hessian_lagrangian_host(qln_handle* h, const double* Z, const double* sigma, const double* mu, double* hvals) {
    if (int rc = check_hessian_args(h, Z, mu, hvals, "qln_eval_hessian_lagrangian_host")) return rc;
    if (int rc = bind_device(h)) return rc;
    return host_call(h, {copy_in(kZ, Z), copy_in(kMu, mu), copy_out(kHvals, hvals), copy_in(kSigma, sigma)},
                     [&](double* const* d, bool) {
                         return qln::launch_hessian_lagrangian(h->p, d[kZ], d[kSigma], d[kMu], d[kHvals], h->h_stride,
                                                               h->stream);
                     },
                     false);
}

int qln_eval_hessian_lagrangian_product_host(qln_handle* h, const double* Z, const double* sigma, const double* mu,
                                             const double* v, double* y) {
    if (int rc = check_hessian_product_args(h, Z, mu, v, y, "qln_eval_hessian_lagrangian_product_host")) return rc;
    if (int rc = bind_device(h)) return rc;
    return host_call(h, {copy_in(kZ, Z), copy_in(kV, v), copy_in(kMu, mu), copy_out(kZout, y), copy_in(kSigma, sigma)},
                     [&](double* const* d, bool) {
                         return qln::launch_hessian_lagrangian_product(h->p, d[kZ], d[kSigma], d[kMu], d[kV], d[kZout],
                                                                       h->stream);
                     });
}

int qln_eval_constraint_jvp_host(qln_handle* h, const double* Z, const double* v, double* y) {
    if (int rc = check_handle(h)) return rc;
    if (!Z || !v || !y) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_eval_constraint_jvp_host: null pointer");
    if (int rc = bind_device(h)) return rc;
    return host_call(h, {copy_in(kZ, Z), copy_in(kV, v), copy_out(kC, y)}, [&](double* const* d, bool) {
        return qln::launch_constraint_jvp(h->p, d[kZ], d[kV], d[kC], h->stream);
    });
}

int qln_eval_constraint_vjp_host(qln_handle* h, const double* Z, const double* lam, double* g) {
    if (int rc = check_handle(h)) return rc;
    if (!Z || !lam || !g) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_eval_constraint_vjp_host: null pointer");
    if (int rc = bind_device(h)) return rc;
    return host_call(h, {copy_in(kZ, Z), copy_in(kMu, lam), copy_out(kZout, g)}, [&](double* const* d, bool) {
        return qln::launch_constraint_vjp(h->p, d[kZ], d[kMu], d[kZout], h->stream);
    });
}

int qln_eval_constraint_jacobian_dense_host(qln_handle* h, int32_t b, const double* Z, double* jac) {
    // MOI.eval_constraint_jacobian with use_sparse_jacobian=false (src/moi.jl:15-24): the values are
    // computed on the GPU; the host only scatters them into the caller's column-major matrix,
    // touching exactly the write-set of jac_c! (src/constraints.jl:219-274).
    if (int rc = check_problem(h, b)) return rc;
    if (!Z || !jac) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_eval_constraint_jacobian_dense_host: null pointer");
    if (int rc = bind_device(h)) return rc;
    const int32_t N = h->dims.N, kt = h->k_trans[b];
    const int32_t nnz = nnz_of(N, kt, h->p.jac_format);
    const int64_t m = m_nlp_of(N, kt);
    // only problem b's n_nlp entries of Z go in; its nnz values are scattered from mapped memory, or staged back first
    h->h_vals_one.resize(nnz);
    const double* v = nullptr;
    if (int rc = host_call(h,
                           {{kZ, Z, nullptr, h->dims.n_nlp, (int64_t)b * h->dims.z_stride, nullptr},
                            {kVals, nullptr, h->h_vals_one.data(), nnz, h->j_off[b], &v}},
                           [&](double* const* d, bool mapped) {
                               return qln::launch_constraint_jacobian(h->p, b, 1, d[kZ], nullptr, d[kVals],
                                                                      QLN_JAC_WRITE_CONSTANTS | (mapped ? qln::kLaunchSplit : 0u),
                                                                      h->stream);
                           }))
        return rc;
    if (h->dense_map.empty()) h->dense_map.resize((size_t)h->dims.B);
    qln_handle::DenseMap& dm = h->dense_map[(size_t)b];
    if (dm.at.empty()) {
        std::vector<int32_t> rows(nnz), cols(nnz);
        if (int rc = qln_jacobian_structure(h, b, rows.data(), cols.data())) return rc;
        dm.at.resize(nnz);
        for (int32_t e = 0; e < nnz; ++e) dm.at[e] = rows[e] + m * (int64_t)cols[e];
        // D[ci, xi[k+1]] .= -I(n) assigns the whole 15x15 block (explicit zeros off the diagonal)
        const int32_t o_dyn = qln::row_layout(N, kt).o_dyn;
        for (int32_t k = 0; k < N - 1; ++k)
            for (int32_t c = 0; c < 15; ++c)
                for (int32_t r = 0; r < 15; ++r)
                    if (r != c) dm.zeros.push_back((o_dyn + 15 * k + r) + m * (int64_t)(20 * (k + 1) + c));
        if (h->p.jac_format == QLN_JAC_FORMAT_STRUCTURAL)
            // D[ci, [xi[k]; ui[k]]] .= J assigns the whole 15x20 block: the entries the structural format leaves out are 0
            for (int32_t k = 0; k < N - 1; ++k)
                for (int32_t c = 0; c < 20; ++c)
                    for (int32_t r = 0; r < 15; ++r) dm.zeros.push_back((o_dyn + 15 * k + r) + m * (int64_t)(20 * k + c));
    }
    for (int64_t i : dm.zeros) jac[i] = 0.0;
    for (int32_t e = 0; e < nnz; ++e) jac[dm.at[e]] = v[e];
    return QLN_OK;
}

// ------------------------------------------------------------------ placement-aware allocation

static int time_fused(qln_handle* h, const double* Z, double* c, double* vals, int warmup, int iters, float* best) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
        if (e0) (void)hipEventDestroy(e0);
        return fail(QLN_ERR_HIP, "hipEventCreate failed");
    }
    int rc = QLN_OK;
    *best = 1e30f;
    for (int i = 0; i < warmup + iters && rc == QLN_OK; ++i) {
        (void)hipEventRecord(e0, h->stream);
        if (qln::launch_constraint_jacobian(h->p, 0, h->p.B, Z, c, vals, 0, h->stream) != hipSuccess) rc = fail(QLN_ERR_HIP, "launch failed");
        (void)hipEventRecord(e1, h->stream);
        if (rc == QLN_OK && hipEventSynchronize(e1) != hipSuccess) rc = fail(QLN_ERR_HIP, "hipEventSynchronize failed");
        float ms = 0.f;
        if (rc == QLN_OK && hipEventElapsedTime(&ms, e0, e1) != hipSuccess) rc = fail(QLN_ERR_HIP, "hipEventElapsedTime failed");
        if (rc == QLN_OK && i >= warmup) *best = std::min(*best, ms);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return rc;
}

int qln_vals_alloc_placed(qln_handle* h, const double* Z, double* c, double** vals, float* ms_best) {
    return qln_vals_alloc_placed_budget(h, Z, c, (int64_t)64 << 30, vals, ms_best);
}

int qln_vals_placed_address_space(int64_t* retired_bytes, int64_t* cap_bytes) {
    if (retired_bytes) *retired_bytes = (int64_t)g_va_retired.load();
    if (cap_bytes) *cap_bytes = (int64_t)kVaCapBytes;
    return QLN_OK;
}

int qln_vals_alloc_placed_budget(qln_handle* h, const double* Z, double* c, int64_t transient_bytes, double** vals, float* ms_best) {
    if (int rc = check_handle(h)) return rc;
    if (!Z || !vals) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_vals_alloc_placed: null pointer");
    if (transient_bytes < 0) return fail(QLN_ERR_INVALID_ARGUMENT, "qln_vals_alloc_placed: negative transient budget");
    *vals = nullptr;
    if (int rc = bind_device(h)) return rc;
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = h->device;
    size_t gran = 0;
    QLN_HIP(hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended));
    // Physical chunks of 256 MiB: launch times are the same from 2 MiB to 1 GiB (profiles/r01_vmm_placement.txt), and a
    // finer chunk makes the window scan finer.  (Round 1 recorded "chunks of 2 GiB and more raise a GPU memory access
    // fault": that program had unmapped, freed and re-reserved the same range a dozen times before it got to that size,
    // i.e. it ran into the address-reuse defect described at kReturnVirtualRange.  On a fresh range 2-GiB chunks are
    // fine: bench/vmm_big_chunk.cpp, profiles/r02_vmm_big_chunk.txt.)
    const size_t chunk = round_up((int64_t)256 << 20, (int64_t)gran);
    const size_t bytes = (size_t)h->dims.j_total * 8;
    const size_t need = (bytes + chunk - 1) / chunk;                     // chunks under vals
    const size_t region = ((size_t)32 << 30) / chunk;                    // period of the speed classes, in chunks
    const bool small = bytes < ((size_t)1 << 30);                        // nothing to gain: one plain mapping
    size_t free_b = 0, total_b = 0;
    QLN_HIP(hipMemGetInfo(&free_b, &total_b));
    const size_t budget = free_b / 10 * 9 / chunk;                       // chunks this call may hold at once
    if (budget < need + 1) return fail(QLN_ERR_HIP, "qln_vals_alloc_placed: not enough free device memory");

    // Everything this call holds until it has succeeded.  abandon() is the one way out on failure: synchronise the
    // device, unmap what is mapped, release every handle, hand the range back, free the scratch constraint buffer.
    std::vector<hipMemGenericAllocationHandle_t> slab;   // consecutive physical chunks (consecutive allocations are
    std::vector<char> mapped;                            // consecutive in device memory as far as launch times can tell)
    char* va = nullptr;
    size_t va_size = 0;
    double* scratch_c = nullptr;
    auto abandon = [&](int code) {
        (void)hipDeviceSynchronize();
        for (size_t i = 0; i < slab.size(); ++i) {
            if (i < mapped.size() && mapped[i]) (void)hipMemUnmap(va + i * chunk, chunk);
            if (slab[i]) (void)hipMemRelease(slab[i]);
        }
        if (va && kReturnVirtualRange) (void)hipMemAddressFree(va, va_size);
        if (scratch_c) (void)hipFree(scratch_c);
        return code;
    };
    auto fail_hip = [&](const char* what, hipError_t e) {
        return abandon(fail(QLN_ERR_HIP, std::string("qln_vals_alloc_placed: ") + what + ": " + hipGetErrorString(e)));
    };

    // the timed launches write a constraint vector: the caller's c if one is given (it is overwritten), else a scratch
    if (!c) {
        if (hipError_t e = hipMalloc(reinterpret_cast<void**>(&scratch_c), (size_t)h->dims.c_total * 8); e != hipSuccess)
            return fail_hip("hipMalloc(scratch c)", e);
        c = scratch_c;
    }
    // two region lengths beyond the buffer: the slab then contains two boundaries, i.e. two chances of a clean
    // straddling window
    // (a caller with less memory to spare passes a smaller transient budget: one region length gives one boundary)
    (void)region;
    const size_t extra = ((size_t)transient_bytes + chunk - 1) / chunk;
    size_t nslab = small ? need : std::min(budget, need + extra + 1);
    if (g_va_retired.load() + (uint64_t)nslab * chunk > kVaCapBytes)
        return abandon(fail(QLN_ERR_UNSUPPORTED,
                            "qln_vals_alloc_placed: this process has retired " + std::to_string(g_va_retired.load() >> 30) +
                                " GiB of virtual address space in placed allocations (ranges are never returned: an unmapped address "
                                "must not be mapped again on this stack); the cap is " + std::to_string(kVaCapBytes >> 30) +
                                " GiB -- reuse placed buffers instead of re-allocating them, or use plain hipMalloc memory"));
    for (size_t i = 0; i < nslab; ++i) {
        hipMemGenericAllocationHandle_t hd;
        const hipError_t e = hipMemCreate(&hd, chunk, &prop, 0);
        if (e != hipSuccess) {
            if (slab.size() >= need + 1) break;  // less than planned, still usable
            return fail_hip("hipMemCreate", e);
        }
        slab.push_back(hd);
    }
    nslab = slab.size();
    mapped.assign(nslab, 0);
    va_size = nslab * chunk;
    {
        void* p = nullptr;
        if (hipError_t e = hipMemAddressReserve(&p, va_size, 0, nullptr, 0); e != hipSuccess) return fail_hip("hipMemAddressReserve", e);
        va = static_cast<char*>(p);
        if (!kReturnVirtualRange) g_va_retired.fetch_add((uint64_t)va_size);  // whatever happens next, this range is spent
    }
    for (size_t i = 0; i < nslab; ++i) {
        if (hipError_t e = hipMemMap(va + i * chunk, chunk, 0, slab[i], 0); e != hipSuccess) return fail_hip("hipMemMap", e);
        mapped[i] = 1;
    }
    {
        hipMemAccessDesc ad = {};
        ad.location = prop.location;
        ad.flags = hipMemAccessFlagsProtReadWrite;
        if (hipError_t e = hipMemSetAccess(va, va_size, &ad, 1); e != hipSuccess) return fail_hip("hipMemSetAccess", e);
    }

    // The slab as it lies, the fused launch timed on its windows: the best one straddles a region boundary (XCDs 0-3
    // write one region, XCDs 4-7 the next).  Giving every XCD's range a region of its own (ranges 16 GiB apart) was
    // tried as a second layout: 1.10 ms against 1.08-1.10 ms for the best window, so it is not built.
    size_t best_off = 0;  // chunks
    float best = 1e30f;
    {
        auto probe = [&](size_t off) {
            float ms = 0.f;
            const int rc = time_fused(h, Z, c, reinterpret_cast<double*>(va + off * chunk), 1, 2, &ms);
            if (rc == QLN_OK && ms < best) {
                best = ms;
                best_off = off;
            }
            return rc;
        };
        int rc = QLN_OK;
        if (small) {
            rc = probe(0);
        } else {
            for (size_t off = 0; off + need <= nslab && rc == QLN_OK; off += 4) rc = probe(off);  // 1-GiB steps
            const size_t centre = best_off;
            for (int k = -3; k <= 3 && rc == QLN_OK; ++k) {
                const int64_t off = (int64_t)centre + k;
                if (k != 0 && off >= 0 && (size_t)off + need <= nslab) rc = probe((size_t)off);
            }
        }
        if (rc != QLN_OK) return abandon(rc);
    }
    // Every chunk outside the window goes back to the driver; the window keeps its addresses.  time_fused waited for
    // each of its launches, but nothing is assumed: the device is idle before the first unmap.
    if (hipError_t e = hipDeviceSynchronize(); e != hipSuccess) return fail_hip("hipDeviceSynchronize", e);
    for (size_t i = 0; i < nslab; ++i) {
        if (i >= best_off && i < best_off + need) continue;
        if (hipError_t e = hipMemUnmap(va + i * chunk, chunk); e != hipSuccess) return fail_hip("hipMemUnmap", e);
        mapped[i] = 0;
    }
    for (size_t i = 0; i < nslab; ++i) {
        if (i >= best_off && i < best_off + need) continue;
        const hipError_t e = hipMemRelease(slab[i]);
        slab[i] = nullptr;  // released (or lost): abandon() must not release it again
        if (e != hipSuccess) return fail_hip("hipMemRelease", e);
    }
    if (scratch_c) {
        const hipError_t e = hipFree(scratch_c);
        scratch_c = nullptr;
        if (e != hipSuccess) return fail_hip("hipFree(scratch c)", e);
    }
    qln_handle::Placed P;
    P.chunk = chunk;
    P.va = va;
    P.va_size = va_size;
    P.first = best_off;
    P.chunks.assign(slab.begin() + (long)best_off, slab.begin() + (long)(best_off + need));
    P.vals = reinterpret_cast<double*>(va + best_off * chunk);
    P.scanned = nslab;
    h->placed.push_back(P);
    *vals = P.vals;
    if (ms_best) *ms_best = best;
    return QLN_OK;
}

int qln_vals_placed_info(const qln_handle* h, const double* vals, int64_t* chunk_bytes, int64_t* chunks_scanned,
                         int64_t* window_first_chunk) {
    if (int rc = check_handle(h)) return rc;
    for (const auto& p : h->placed)
        if (p.vals == vals) {
            if (chunk_bytes) *chunk_bytes = (int64_t)p.chunk;
            if (chunks_scanned) *chunks_scanned = (int64_t)p.scanned;
            if (window_first_chunk) *window_first_chunk = (int64_t)p.first;
            return QLN_OK;
        }
    return fail(QLN_ERR_INVALID_ARGUMENT, "qln_vals_placed_info: not a buffer of this handle");
}

int qln_vals_free_placed(qln_handle* h, double* vals) {
    if (int rc = check_handle(h)) return rc;
    if (int rc = bind_device(h)) return rc;
    for (size_t i = 0; i < h->placed.size(); ++i)
        if (h->placed[i].vals == vals) {
            // the whole device, not the handle's stream: the buffer was handed out as plain memory and any stream may
            // have work on it (torch's current stream; a stream set with qln_set_stream after the last launch)
            QLN_HIP(hipDeviceSynchronize());
            const int rc = release_placed(h->placed[i]);
            h->placed.erase(h->placed.begin() + (long)i);
            return rc;
        }
    return fail(QLN_ERR_INVALID_ARGUMENT, "qln_vals_free_placed: not a buffer of this handle");
}

// ------------------------------------------------------------------ measurement

int qln_time_constraint_and_jacobian(qln_handle* h, const double* Z, double* c, double* vals, uint32_t flags, int32_t warmup,
                                     int32_t iters, float* ms_each) {
    if (int rc = check_handle(h)) return rc;
    if (!Z || !c || !ms_each || iters < 1 || warmup < 0)
        return fail(QLN_ERR_INVALID_ARGUMENT, "qln_time_constraint_and_jacobian: bad argument");
    if (int rc = check_vals(vals)) return rc;
    if (int rc = bind_device(h)) return rc;
    flags &= QLN_JAC_WRITE_CONSTANTS;
    std::vector<hipEvent_t> ev(2 * (size_t)iters, nullptr);
    int rc = QLN_OK;
    for (auto& e : ev)
        if (rc == QLN_OK && hipEventCreate(&e) != hipSuccess) rc = fail(QLN_ERR_HIP, "hipEventCreate failed");
    for (int32_t i = 0; i < warmup && rc == QLN_OK; ++i)
        if (qln::launch_constraint_jacobian(h->p, 0, h->p.B, Z, c, vals, flags, h->stream) != hipSuccess)
            rc = fail(QLN_ERR_HIP, "warmup launch failed");
    for (int32_t i = 0; i < iters && rc == QLN_OK; ++i) {
        (void)hipEventRecord(ev[2 * i], h->stream);
        if (qln::launch_constraint_jacobian(h->p, 0, h->p.B, Z, c, vals, flags, h->stream) != hipSuccess)
            rc = fail(QLN_ERR_HIP, "timed launch failed");
        (void)hipEventRecord(ev[2 * i + 1], h->stream);
    }
    if (rc == QLN_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(QLN_ERR_HIP, "stream synchronize failed");
    for (int32_t i = 0; i < iters && rc == QLN_OK; ++i)
        if (hipEventElapsedTime(&ms_each[i], ev[2 * i], ev[2 * i + 1]) != hipSuccess)
            rc = fail(QLN_ERR_HIP, "hipEventElapsedTime failed");
    for (auto& e : ev)
        if (e) (void)hipEventDestroy(e);
    return rc;
}

int qln_time_constraint_and_jacobian_total(qln_handle* h, const double* Z, double* c, double* vals, uint32_t flags, int32_t warmup,
                                           int32_t iters, float* ms_total) {
    if (int rc = check_handle(h)) return rc;
    if (!Z || !c || !ms_total || iters < 1 || warmup < 0)
        return fail(QLN_ERR_INVALID_ARGUMENT, "qln_time_constraint_and_jacobian_total: bad argument");
    if (int rc = check_vals(vals)) return rc;
    if (int rc = bind_device(h)) return rc;
    flags &= QLN_JAC_WRITE_CONSTANTS;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = QLN_OK;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) rc = fail(QLN_ERR_HIP, "hipEventCreate failed");
    for (int32_t i = 0; i < warmup && rc == QLN_OK; ++i)
        if (qln::launch_constraint_jacobian(h->p, 0, h->p.B, Z, c, vals, flags, h->stream) != hipSuccess)
            rc = fail(QLN_ERR_HIP, "warmup launch failed");
    if (rc == QLN_OK) (void)hipEventRecord(e0, h->stream);
    for (int32_t i = 0; i < iters && rc == QLN_OK; ++i)
        if (qln::launch_constraint_jacobian(h->p, 0, h->p.B, Z, c, vals, flags, h->stream) != hipSuccess)
            rc = fail(QLN_ERR_HIP, "timed launch failed");
    if (rc == QLN_OK) (void)hipEventRecord(e1, h->stream);
    if (rc == QLN_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(QLN_ERR_HIP, "stream synchronize failed");
    if (rc == QLN_OK && hipEventElapsedTime(ms_total, e0, e1) != hipSuccess) rc = fail(QLN_ERR_HIP, "hipEventElapsedTime failed");
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return rc;
}

}  // extern "C"
