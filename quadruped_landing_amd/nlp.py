"""HybridNLP: the landing NLP (mirror of src/nlp.jl:13-114) generalised to a batch of B
independent problems, evaluated by the gfx950 kernels through the C ABI.

The index maps (xinds/uinds/cinds), bounds and sizes are host logic and are pure
numpy; every evaluation (eval_f, grad_f, eval_c, jac_c) is a kernel launch behind
include/qln_evaluator.h -- there is no CPU implementation of the arithmetic here.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from .planar_quadruped import PlanarQuadruped

n, m = 15, 5


# ----------------------------------------------------------------------------- index maps


def num_primals(N: int) -> int:
    """src/nlp.jl:86"""
    return n * N + m * (N - 1)


def num_duals(N: int, k_trans: int) -> int:
    """src/nlp.jl:87 (= cinds[end][end])"""
    return cinds(N, k_trans)[-1][-1]


def xinds(N: int):
    """src/nlp.jl:38, 1-based like the reference."""
    return [np.arange(1, n + 1) + (k - 1) * (n + m) for k in range(1, N + 1)]


def uinds(N: int):
    """src/nlp.jl:39, 1-based."""
    return [np.arange(n + 1, n + m + 1) + (k - 1) * (n + m) for k in range(1, N)]


def cinds(N: int, k_trans: int):
    """src/nlp.jl:48-63: seven 1-based inclusive (start, end) ranges."""
    out, e = [], 0
    for ln in (n, n - 1, (N - 1) * n, N, N - k_trans + 1, 1, N):
        out.append((e + 1, e + ln))
        e += ln
    return out


def constraint_bounds(N: int, k_trans: int):
    """src/nlp.jl:66-69"""
    ci = cinds(N, k_trans)
    m_nlp = ci[-1][-1]
    lb, ub = np.zeros(m_nlp), np.zeros(m_nlp)
    ub[ci[6][0] - 1 : ci[6][1]] = np.inf
    return lb, ub


def packZ(N: int, X, U):
    """src/nlp.jl:94-102.  X: (...,N,15), U: (...,N-1,5) -> Z (...,20N-5)."""
    X = np.asarray(X, dtype=np.float64)
    U = np.asarray(U, dtype=np.float64)
    Z = np.zeros(X.shape[:-2] + (num_primals(N),))
    body = Z[..., : 20 * (N - 1)].reshape(X.shape[:-2] + (N - 1, 20))
    body[..., :15] = X[..., : N - 1, :]
    body[..., 15:] = U
    Z[..., 20 * (N - 1) :] = X[..., N - 1, :]
    return Z


def unpackZ(N: int, Z):
    """src/nlp.jl:110-114"""
    Z = np.asarray(Z)
    body = Z[..., : 20 * (N - 1)].reshape(Z.shape[:-1] + (N - 1, 20))
    X = np.concatenate([body[..., :15], Z[..., None, 20 * (N - 1) :]], axis=-2)
    return X, body[..., 15:]


# ----------------------------------------------------------------------------- evaluator


def hessian_structure(N: int):
    """0-based (rows, cols), row >= col, of the Lagrangian Hessian of one problem with N knots (qln_hessian_structure):
    N-1 step blocks of 55 entries, column-major inside a block, then the 15 terminal diagonal entries.  No device."""
    n = _lib.HESS_STEP_NNZ * (int(N) - 1) + _lib.HESS_TERM_NNZ
    rows, cols = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    _lib.check(_lib.lib().qln_hessian_structure(int(N), rows.ctypes.data_as(ip), cols.ctypes.data_as(ip)))
    return rows, cols


def tracking_weights(Q, R, Qf):
    """The diagonal TVLQR weights as contiguous float64 arrays (15, 4, 15); a scalar broadcasts."""
    Q = np.ascontiguousarray(np.broadcast_to(np.asarray(Q, dtype=np.float64), (n,)))
    R = np.ascontiguousarray(np.broadcast_to(np.asarray(R, dtype=np.float64), (_lib.TRACK_NU,)))
    Qf = np.ascontiguousarray(np.broadcast_to(np.asarray(Qf, dtype=np.float64), (n,)))
    return Q, R, Qf


def tracking_k_shape(B: int, N: int):
    """Shape of the gains of qln_tracking_lqr: (B, N-1, 4, 15), row-major."""
    return (B, N - 1, _lib.TRACK_NU, n)


def tracking_p_shape(B: int, N: int):
    """Shape of the packed cost-to-go of qln_tracking_lqr: (B, N, 120), row i >= j at i(i+1)/2 + j."""
    return (B, N, _lib.TRACK_P_NNZ)


def unpack_cost_to_go(P):
    """(..., 120) packed lower triangles -> (..., 15, 15) symmetric numpy matrices."""
    P = P.detach().cpu().numpy() if hasattr(P, "detach") else np.asarray(P)
    r, c = np.tril_indices(n)  # row-major over the lower triangle: (i, j) at i(i+1)/2 + j
    out = np.zeros(P.shape[:-1] + (n, n))
    out[..., r, c] = P
    out[..., c, r] = P
    return out


def unpack_covariance(Sigma):
    """(..., 120) packed lower triangles of qln_tracking_covariance -> (..., 15, 15) symmetric numpy matrices (the layout
    of the cost-to-go)."""
    return unpack_cost_to_go(Sigma)


def pack_covariance(Sigma):
    """(..., 15, 15) matrices -> (..., 120) packed lower triangles, row i >= j at i(i+1)/2 + j (the lower triangle is what
    is kept)."""
    Sigma = np.asarray(Sigma, dtype=np.float64)
    r, c = np.tril_indices(n)
    return np.ascontiguousarray(Sigma[..., r, c])


def tracking_sigma0(Sigma0, B: int):
    """The initial covariance of qln_tracking_covariance in any of its forms -> (packed (sigma0_batch, 120), sigma0_batch):
    a 15-vector of variances, a 15x15 matrix, (B, 15, 15), or already packed (120,), (1, 120) or (B, 120)."""
    S = np.asarray(Sigma0, dtype=np.float64)
    if S.shape == (n,):
        S = np.diag(S)
    if S.shape[-2:] == (n, n) and S.ndim in (2, 3):
        S = pack_covariance(S)
    if S.ndim == 1:
        S = S[None]
    if S.ndim != 2 or S.shape[1] != _lib.TRACK_P_NNZ or S.shape[0] not in (1, B):
        raise ValueError(f"Sigma0 of shape {np.shape(Sigma0)}: expected (15,), (15, 15), ({B}, 15, 15), (120,), (1, 120) or "
                         f"({B}, 120)")
    return np.ascontiguousarray(S), int(S.shape[0])


def tracking_noise(W):
    """The diagonal process noise as a contiguous (15,) array, or None (zeros); a scalar broadcasts."""
    if W is None:
        return None
    return np.ascontiguousarray(np.broadcast_to(np.asarray(W, dtype=np.float64), (n,)))


def measurement_model(H, V):
    """The measurement model y = H dx + v of qln_tracking_kalman as contiguous float64 arrays (H (ny, 15), V (ny,)): H a
    matrix of 1 to 8 rows of 15 (a 15-vector is one row), V the ny measurement variances (a scalar broadcasts).  A
    non-finite H, or a V entry that is not finite and > 0, is refused."""
    H = np.asarray(H, dtype=np.float64)
    if H.ndim == 1:
        H = H[None]
    if H.ndim != 2 or H.shape[1] != n or not 1 <= H.shape[0] <= _lib.TRACK_NY_MAX:
        raise ValueError(f"H of shape {H.shape}: expected (ny, 15) with 1 <= ny <= {_lib.TRACK_NY_MAX}")
    if np.ndim(V) > 1 or (np.ndim(V) == 1 and np.shape(V)[0] != H.shape[0]):
        raise ValueError(f"V of shape {np.shape(V)}: expected a scalar or ({H.shape[0]},)")
    V = np.ascontiguousarray(np.broadcast_to(np.asarray(V, dtype=np.float64), (H.shape[0],)))
    if not np.isfinite(H).all():
        raise ValueError("H is not finite")
    if not (np.isfinite(V) & (V > 0)).all():
        raise ValueError("V: every measurement variance must be finite and > 0")
    return np.ascontiguousarray(H), V


def landing_measurements(Zout, Zref, H, vnoise=None, B=None):
    """Y (B, N, ny) in the form qln_landing_filter reads it and the estimate-feedback roll-out forms it: H (x_k - x_ref,k) + v_k,
    from a flown or recorded state trajectory Zout and the reference Zref (both in the layout of Z: B problems, a stride of at
    least n_nlp each; flat buffers need B, HybridNLP.landing_measurements passes it), H (ny, 15) and vnoise (B, N, ny) or None.
    Tensors in, a tensor out (on Zout's device); numpy in, numpy out.  The products are torch's or numpy's, not the kernel's:
    equal to the roll-out's y_k up to rounding, not bit for bit."""
    torch_in = hasattr(Zout, "detach")
    H = np.asarray(H.detach().cpu().numpy() if hasattr(H, "detach") else H, dtype=np.float64)
    if H.ndim == 1:
        H = H[None]
    if H.ndim != 2 or H.shape[1] != n:
        raise ValueError(f"H of shape {H.shape}: expected (ny, 15)")
    if B is None:
        if Zout.ndim != 2:
            raise ValueError("a flat Zout needs B, the number of problems")
        B = Zout.shape[0]
    zo, zr = Zout.reshape(B, -1), Zref.reshape(B, -1)
    N = (min(zo.shape[1], zr.shape[1]) + 5) // 20
    if torch_in:
        T = _torch()
        Ht = T.from_numpy(np.ascontiguousarray(H)).to(zo.device)
        idx = (20 * T.arange(N, device=zo.device)[:, None] + T.arange(n, device=zo.device)[None, :]).reshape(-1)
        y = (zo[:, idx] - zr.to(zo.device)[:, idx]).reshape(B, N, n) @ Ht.T
        return (y if vnoise is None else y + vnoise.reshape(B, N, -1)).contiguous()
    idx = 20 * np.arange(N)[:, None] + np.arange(n)[None, :]
    y = (np.asarray(zo)[:, idx] - np.asarray(zr)[:, idx]) @ H.T
    return y if vnoise is None else y + np.asarray(vnoise).reshape(B, N, -1)


def tracking_l_shape(B: int, N: int, ny: int):
    """Shape of the filter gains of qln_tracking_kalman: (B, N, 15, ny), row-major."""
    return (B, N, n, ny)


def force_limits(limits):
    """The eight force limits {free_x_lo, free_x_hi, free_y_lo, free_y_hi, stand_x_lo, stand_x_hi, stand_y_lo, stand_y_hi} as
    the contiguous float64 array the limited calls pass; +-inf means no limit on that side.  A NaN, or lo > hi, is refused."""
    lim = np.ascontiguousarray(np.asarray(limits, dtype=np.float64).reshape(-1))
    if lim.size != _lib.FORCE_LIMITS_N:
        raise ValueError(f"limits has {lim.size} entries, expected {_lib.FORCE_LIMITS_N}")
    if np.isnan(lim).any() or (lim[0::2] > lim[1::2]).any():
        raise ValueError("limits: a NaN, or a lower limit above its upper limit")
    return lim


def unpack_saturation(sat):
    """Saturation codes (B, N-1) (numpy or a tensor) -> int8 (B, N-1, 4): per channel (F1x, F1y, F2x, F2y) 0 for a free
    force, 1 for one held at its lower limit, 2 at its upper limit."""
    c = (sat.detach().cpu().numpy() if hasattr(sat, "detach") else np.asarray(sat)).astype(np.int64)
    return ((c[..., None] >> np.array([0, 2, 4, 6])) & 3).astype(np.int8)


def mask_gains(K, sat):
    """Gains K (B, N-1, 4, 15) designed elsewhere, with the rows of the channels that rode a limit (sat, the limited
    roll-out's record) set to zero: A - B K is then the closed loop of the clamped system, for the covariance calls.  numpy
    in, numpy out; tensors in, a tensor out."""
    free = unpack_saturation(sat) == 0
    if hasattr(K, "detach"):
        T = _torch()
        return T.where(T.from_numpy(free).to(K.device).reshape(K.shape[:-1] + (1,)), K, T.zeros((), dtype=K.dtype, device=K.device))
    return np.where(free[..., None], np.asarray(K), 0.0)


def _torch():
    import torch

    return torch


def _host_ptr(a):
    """The address of a host array for the C ABI, None (NULL) for an optional argument left out."""
    return None if a is None else a.ctypes.data


class _DeviceForm:
    """The device memory form of the tracking and landing operations of HybridNLP, and with _HostForm everything in which the
    two forms of an operation differ: how an input is checked, how an output is allocated, whether H is staged on the device,
    the address an array is passed by, the entry point's suffix and the sibling calls a message names.  Here: inputs are
    contiguous float64 CUDA tensors on the handle's device holding at least the elements the operation reads (TypeError /
    ValueError of HybridNLP._check), outputs are fresh tensors or the caller's, checked like inputs."""

    suffix = ""
    MEASUREMENTS = " (landing_measurements)"
    TRAJ = "Lgain and Xhat are required: the filter gains and the estimates tracking_rollout_estimated returned"
    INNOV = "innov is required with a tangent or cotangent of Lgain (with_innovations=True in the roll-out)"
    RECORDS = "events and events_hat are required: the two records tracking_rollout_estimated returned"

    def __init__(self, nlp):
        self.nlp, self.check = nlp, nlp._check

    def fn(self, name):
        return getattr(_lib.lib(), name)

    @staticmethod
    def ptr(t):
        return None if t is None else t.data_ptr()

    def arr(self, t, size, name):
        self.check(t, size, name)
        return t

    def opt(self, t, size, name):
        if t is not None:
            self.check(t, size, name)
        return t

    loose = opt  # the filter's sweeps: the host form differs

    def Z(self, t, name):
        return self.arr(t, self.nlp.dims.z_total, name)

    def Z_opt(self, t, name):
        return self.opt(t, self.nlp.dims.z_total, name)

    def K(self, t, name="K"):
        return self.opt(t, self.nlp.B * (self.nlp.N - 1) * _lib.TRACK_NU * n, name)

    def x0(self, t, name="x0"):
        return self.opt(t, self.nlp.B * n, name)

    def model(self, t, name="model"):
        return self.opt(t, self.nlp.B * _lib.MODEL_NP, name)

    def events(self, t):
        if t is None:
            raise ValueError("events is required: the record tracking_rollout_guarded returned with Zout")
        return self.arr(t, self.nlp.B * _lib.TOUCHDOWN_INFO_STRIDE, "events")

    def events_hat(self, t):
        return self.arr(t, self.nlp.B * _lib.TOUCHDOWN_INFO_STRIDE, "events_hat")

    def sat(self, t):
        if t is None:
            raise ValueError("sat is required: the saturation record tracking_rollout_limited returned with Zout")
        return self.arr(t, self.nlp.B * (self.nlp.N - 1), "sat")

    def H(self, Hh):
        return _torch().from_numpy(Hh).to(self.nlp._dev())

    def sigma0(self, Sigma0):
        """Sigma0 in any form of tracking_sigma0, or a CUDA tensor of 1 or B packed tiles -> (device tensor, sigma0_batch)."""
        T = _torch()
        if Sigma0 is None:
            raise ValueError("Sigma0 is required")
        if isinstance(Sigma0, T.Tensor) and Sigma0.is_cuda:
            nb = Sigma0.numel() // _lib.TRACK_P_NNZ
            if Sigma0.numel() != nb * _lib.TRACK_P_NNZ or nb not in (1, self.nlp.B):
                raise ValueError("a device Sigma0 must hold 1 or B packed tiles of 120")
            s0 = Sigma0
        else:
            host, nb = tracking_sigma0(Sigma0, self.nlp.B)
            s0 = T.from_numpy(host).to(self.nlp._dev())
        self.check(s0, nb * _lib.TRACK_P_NNZ, "Sigma0")
        return s0, nb

    def zeros(self, shape, want=True):
        T = _torch()
        return T.zeros(shape, dtype=T.float64, device=self.nlp._dev()) if want else None

    def empty(self, shape, want=True):
        T = _torch()
        return T.empty(shape, dtype=T.float64, device=self.nlp._dev()) if want else None

    def out(self, t, shape, name, empty=False):
        """The caller's buffer, or a fresh one (empty: one the operation writes whole), checked"""
        if t is None:
            t = self.empty(shape) if empty else self.zeros(shape)
        self.check(t, math.prod(shape), name)
        return t


class _HostForm:
    """The host memory form (synchronous): inputs are anything numpy reads, flattened to contiguous float64 of exactly the
    expected size (ValueError), a Z given as (B, n_nlp) rows is padded to the handle's z_stride, x0 and its like broadcast to
    (B, 15); outputs are fresh zeroed arrays, never the caller's; H is used in place; the entry point is the _host one."""

    suffix = "_host"
    MEASUREMENTS = ""
    TRAJ = "Lgain and Xhat are required: what tracking_rollout_estimated_host took and returned"
    INNOV = "innov is required with a tangent or cotangent of Lgain"
    RECORDS = "events and events_hat are required: the two records the roll-out returned"

    def __init__(self, nlp):
        self.nlp = nlp

    def fn(self, name):
        return getattr(_lib.lib(), name + "_host")

    ptr = staticmethod(_host_ptr)

    @staticmethod
    def arr(a, size, name):
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
        if a.size != size:
            raise ValueError(f"{name} has {a.size} entries, expected {size}")
        return a

    def opt(self, a, size, name):
        return None if a is None else self.arr(a, size, name)

    @staticmethod
    def loose(a, size, name):
        if a is None:
            return None
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
        if a.size < size:
            raise ValueError(f"{name} has {a.size} entries, expected {size}")
        return a

    def Z(self, a, name):
        return self.nlp._host_Z(a, name)

    def Z_opt(self, a, name):
        return None if a is None else self.nlp._host_Z(a, name)

    def K(self, a, name="K"):
        return self.nlp._host_K(a)

    def x0(self, a, name="x0"):
        if a is None:
            return None
        return np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (self.nlp.B, n)))

    def model(self, a, name="model"):
        return self.opt(a, self.nlp.B * _lib.MODEL_NP, name)

    def events(self, a):
        if a is None:
            raise ValueError("events is required: the record tracking_rollout_guarded_host returned with Zout")
        return self.arr(a, self.nlp.B * _lib.TOUCHDOWN_INFO_STRIDE, "events")

    events_hat = events

    def sat(self, a):
        if a is None:
            raise ValueError("sat is required: the saturation record tracking_rollout_limited_host returned with Zout")
        return self.arr(a, self.nlp.B * (self.nlp.N - 1), "sat")

    @staticmethod
    def H(Hh):
        return Hh

    def sigma0(self, Sigma0):
        if Sigma0 is None:
            raise ValueError("Sigma0 is required")
        return tracking_sigma0(Sigma0, self.nlp.B)

    @staticmethod
    def zeros(shape, want=True):
        return np.zeros(shape) if want else None

    empty = zeros

    @staticmethod
    def out(a, shape, name, empty=False):
        return np.zeros(shape)


# layout of the step-block section of vals (include/qln_evaluator.h, QLN_JAC_FORMAT_*)
JAC_FORMATS = {"dense_blocks": _lib.QLN_JAC_FORMAT_DENSE_BLOCKS, "structural": _lib.QLN_JAC_FORMAT_STRUCTURAL}


class _PlacedBuffer:
    """Owner of a buffer obtained from qln_vals_alloc_placed, exposed to torch through __cuda_array_interface__
    (the tensor made from it keeps this object alive; the buffer goes back to the driver when both are gone)."""

    def __init__(self, nlp, ptr: int, numel: int):
        self._nlp, self._ptr = nlp, ptr
        self.__cuda_array_interface__ = {"shape": (numel,), "typestr": "<f8", "data": (ptr, False), "version": 2}

    def __del__(self):
        h = getattr(self._nlp, "_h", None)
        if h and self._ptr:
            # qln_vals_free_placed waits for the whole device (the tensor may have been used on any stream) and
            # reports a failing unmap / release; a destructor cannot raise, so a failure becomes a warning
            try:
                rc = _lib.lib().qln_vals_free_placed(h, self._ptr)
                if rc != _lib.QLN_OK:
                    import warnings

                    warnings.warn(f"qln_vals_free_placed failed ({rc}): {_lib.lib().qln_last_error().decode()}")
            except Exception:
                pass
            self._ptr = 0


class HybridNLP:
    """Batch of B landing problems with a common horizon N on one GPU.

    Constructor arguments follow HybridNLP(model, obj, init_mode, k_trans, N, x0, xf)
    (src/nlp.jl:34-37); `obj` is the 41-double cost table of quadratic_cost.lqr_objective,
    either (N,41) shared by all problems or (B,N,41).  Scalars broadcast over the batch.
    """

    def __init__(self, model: PlanarQuadruped, obj, init_mode, k_trans, N: int, x0, xf, *,
                 device: int = 0, z_stride: int = 0, align: int = 16, stream=None, jac_format: str = "dense_blocks",
                 exact_hessian: bool = False, matrix_free: bool = False):
        self.model = model
        # opt-in: offer the exact Lagrangian Hessian (moi.features_available then lists "Hess")
        self.exact_hessian = bool(exact_hessian)
        # opt-in: offer the Jacobian and Hessian-of-the-Lagrangian products (moi.features_available: "JacVec", "HessVec")
        self.matrix_free = bool(matrix_free)
        if jac_format not in JAC_FORMATS:
            raise ValueError(f"jac_format must be one of {sorted(JAC_FORMATS)}")
        self.jac_format = jac_format
        self.N = int(N)
        x0 = np.asarray(x0, dtype=np.float64)
        B = x0.shape[0] if x0.ndim == 2 else 1
        self.B = B
        self.x0 = np.ascontiguousarray(np.broadcast_to(x0, (B, n)))
        self.xf = np.ascontiguousarray(np.broadcast_to(np.asarray(xf, dtype=np.float64), (B, n)))
        self.k_trans = np.ascontiguousarray(np.broadcast_to(np.asarray(k_trans, dtype=np.int32), (B,)))
        self.init_mode = np.ascontiguousarray(np.broadcast_to(np.asarray(init_mode, dtype=np.int32), (B,)))
        if obj is None:  # no cost yet: build it on the device with set_lqr_cost()
            self.cost_batch = 1
        else:
            obj = np.ascontiguousarray(obj, dtype=np.float64)
            if obj.shape == (self.N, _lib.COST_STRIDE):
                self.cost_batch = 1
            elif obj.shape == (B, self.N, _lib.COST_STRIDE):
                self.cost_batch = B
            else:
                raise ValueError(f"obj must have shape (N,41) or (B,N,41), got {obj.shape}")
        self.obj = obj
        self.device = int(device)

        L = _lib.lib()
        d = _lib.QlnBatchDesc()
        d.B, d.N = B, self.N
        d.model = _lib.QlnModel(model.g, model.mb, model.mf, model.lb, model.l1, model.l2)
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        d.k_trans = self.k_trans.ctypes.data_as(ip)
        d.init_mode = self.init_mode.ctypes.data_as(ip)
        d.x0, d.xf = self.x0.ctypes.data_as(dp), self.xf.ctypes.data_as(dp)
        d.cost = self.obj.ctypes.data_as(dp) if self.obj is not None else None
        d.cost_batch, d.z_stride, d.align = self.cost_batch, int(z_stride), int(align)
        d.jac_format = JAC_FORMATS[jac_format]
        h = C.c_void_p()
        _lib.check(L.qln_create(C.byref(d), self.device, C.byref(h)))
        self._h = h
        dims = _lib.QlnDims()
        _lib.check(L.qln_get_dims(self._h, C.byref(dims)))
        self.dims = dims
        self.n_nlp, self.z_stride = dims.n_nlp, dims.z_stride
        self.nnz_dynamic = dims.nnz_dynamic
        self.c_off = np.zeros(B, dtype=np.int64)
        self.j_off = np.zeros(B, dtype=np.int64)
        lp = C.POINTER(C.c_int64)
        _lib.check(L.qln_get_offsets(self._h, self.c_off.ctypes.data_as(lp), self.j_off.ctypes.data_as(lp)))
        hn, hs = C.c_int32(), C.c_int64()
        _lib.check(L.qln_hessian_layout(C.byref(d), C.byref(hn), C.byref(hs)))
        self.h_nnz, self.h_stride = hn.value, hs.value
        self.h_total = (B - 1) * self.h_stride + self.h_nnz  # no padding behind the last problem
        if stream is not None:
            self.set_stream(stream)

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().qln_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream):
        """`stream`: a torch.cuda.Stream or a raw hipStream_t address."""
        ptr = getattr(stream, "cuda_stream", stream)
        _lib.check(_lib.lib().qln_set_stream(self._h, C.c_void_p(int(ptr))))

    def synchronize(self):
        _lib.check(_lib.lib().qln_synchronize(self._h))

    # -- sizes / index maps (src/nlp.jl:85-87) ------------------------------------------------
    def num_primals(self) -> int:
        return self.n_nlp

    def num_duals(self, b: int = 0) -> int:
        mm, _ = self.problem_dims(b)
        return mm

    def size(self):
        return (n, m, self.N)

    def problem_dims(self, b: int = 0):
        mm, nz = C.c_int32(), C.c_int32()
        _lib.check(_lib.lib().qln_problem_dims(self._h, b, C.byref(mm), C.byref(nz)))
        return mm.value, nz.value

    def problem_nnz_dynamic(self, b: int = 0) -> int:
        """State-dependent values at the head of problem b's vals segment (step blocks + N clearance entries)."""
        nd = C.c_int32()
        _lib.check(_lib.lib().qln_problem_nnz_dynamic(self._h, b, C.byref(nd)))
        return nd.value

    def cinds(self, b: int = 0):
        out = (C.c_int32 * 14)()
        _lib.check(_lib.lib().qln_constraint_index_ranges(self._h, b, out))
        return [(out[2 * i], out[2 * i + 1]) for i in range(7)]

    def bounds(self, b: int = 0):
        """(lb, ub) of problem b, src/nlp.jl:66-69."""
        mm, _ = self.problem_dims(b)
        lb, ub = np.empty(mm), np.empty(mm)
        _lib.check(_lib.lib().qln_constraint_bounds(self._h, b, lb.ctypes.data, ub.ctypes.data))
        return lb, ub

    def jacobian_structure(self, b: int = 0):
        """0-based (rows, cols) of problem b's block-COO values."""
        _, nz = self.problem_dims(b)
        rows, cols = np.zeros(nz, dtype=np.int32), np.zeros(nz, dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        _lib.check(_lib.lib().qln_jacobian_structure(self._h, b, rows.ctypes.data_as(ip), cols.ctypes.data_as(ip)))
        return rows, cols

    # -- device buffers -------------------------------------------------------------------------
    def _dev(self):
        return _torch().device("cuda", self.device)

    def new_Z(self):
        return _torch().zeros(self.dims.z_total, dtype=_torch().float64, device=self._dev())

    def new_c(self):
        return _torch().zeros(self.dims.c_total, dtype=_torch().float64, device=self._dev())

    def new_vals(self):
        return _torch().zeros(self.dims.j_total, dtype=_torch().float64, device=self._dev())

    def placed_info(self, vals):
        """(chunk_bytes, chunks_scanned, window_first_chunk) of a buffer made by new_vals_regions."""
        a, b, c_ = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().qln_vals_placed_info(self._h, vals.data_ptr(), C.byref(a), C.byref(b), C.byref(c_)))
        return a.value, b.value, c_.value

    @staticmethod
    def placed_address_space():
        """(bytes of virtual address space retired by placed allocations in this process, the cap at which the library refuses)"""
        a, b = C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().qln_vals_placed_address_space(C.byref(a), C.byref(b)))
        return a.value, b.value

    def new_vals_regions(self, Z, c=None, transient_gib: float = 64.0):
        """The Jacobian buffer placed across two 32-GiB regions of device memory (qln_vals_alloc_placed: HIP
        virtual-memory API, the fused launch timed on windows of a j_total + `transient_gib` range, the fastest window kept
        and everything else released).  Returns (vals, ms) -- ms = launch time on the window kept.  Raises QlnError if the
        device has not got the memory free or the virtual-memory API fails."""
        t = _torch()
        self._check(Z, self.dims.z_total, "Z")
        if c is not None:  # overwritten by the timed launches; None = the library uses a scratch buffer of its own
            self._check(c, self.dims.c_total, "c")
        ptr, ms = C.c_void_p(), C.c_float()
        _lib.check(_lib.lib().qln_vals_alloc_placed_budget(self._h, Z.data_ptr(), None if c is None else c.data_ptr(),
                                                           int(transient_gib * 2**30), C.byref(ptr), C.byref(ms)))
        vals = t.as_tensor(_PlacedBuffer(self, ptr.value, int(self.dims.j_total)), device=self._dev())
        return vals, float(ms.value)

    def new_vals_placed(self, Z, c, trials: int = 4, launches: int = 3, spread: bool = True, regions: bool = True):
        """Setup-time placement choice for the (large, long-lived) Jacobian buffer.

        Where a multi-GB buffer lies physically changes the store bandwidth the hot kernel sustains by ~20 % on
        MI355X: device memory behaves as 32-GiB regions, and the kernel's eight write fronts (the first four in the
        first half of the buffer) run fastest when the two halves lie in different regions (DESIGN.md section 5,
        profiles/r01_placement_windows.txt).  With `regions` the buffer is built that way (new_vals_regions).
        If that is not possible (too little free memory), or `regions` is off, `trials` plain allocations are
        timed instead -- held simultaneously and, with `spread`, ~32 GiB apart so that they sample different
        regions -- and the fastest is kept.  Returns (vals, [ms]) -- one time per candidate tried.
        """
        t = _torch()
        if regions:
            try:
                vals, ms = self.new_vals_regions(Z, c)
                return vals, [ms]
            except _lib.QlnError:
                pass
        trials = max(1, int(trials))
        nbytes = 8 * int(self.dims.j_total)
        spacer_bytes = 0
        if spread and trials > 1:
            free, _ = t.cuda.mem_get_info(self._dev())
            # one candidate + one spacer per trial, about 32 GiB apart, within 85 % of what is free now
            spacer_bytes = max(0, min(32 * 2**30 - nbytes, int(0.85 * free) // trials - nbytes))
        cands, times, spacers = [], [], []
        for i in range(trials):
            v = self.new_vals()
            self.init_jacobian_constants(v)
            ms = self.time_c_and_jac(Z, c, v, warmup=1, iters=max(1, int(launches)))
            cands.append(v)
            times.append(float(np.median(ms)))
            if spacer_bytes >= 2**20 and i + 1 < trials:
                spacers.append(t.empty(spacer_bytes, dtype=t.uint8, device=self._dev()))
        best = int(np.argmin(times))
        vals = cands[best]
        cands.clear()
        spacers.clear()
        del v
        t.cuda.empty_cache()
        return vals, times

    def new_f(self):
        return _torch().zeros(self.B, dtype=_torch().float64, device=self._dev())

    def upload_Z(self, Z_host):
        """Z_host: (B, n_nlp) -> device buffer in the handle's z_stride layout."""
        t = _torch()
        Z_host = np.asarray(Z_host, dtype=np.float64).reshape(self.B, self.n_nlp)
        buf = np.zeros((self.B, self.z_stride))
        buf[:, : self.n_nlp] = Z_host
        return t.from_numpy(buf.reshape(-1)).to(self._dev())

    def _check(self, t, total, name):
        T = _torch()
        if not (isinstance(t, T.Tensor) and t.is_cuda and t.dtype == T.float64 and t.is_contiguous()):
            raise TypeError(f"{name} must be a contiguous float64 CUDA tensor")
        if t.device.index != self.device:
            raise ValueError(f"{name} is on cuda:{t.device.index}, handle is on cuda:{self.device}")
        if t.numel() < total:
            raise ValueError(f"{name} has {t.numel()} elements, need {total}")
        return C.c_void_p(t.data_ptr())

    # -- evaluation (device tensors, stream-ordered) ----------------------------------------------
    def eval_f(self, Z, out=None):
        """src/costs.jl:6-16 for every problem -> (B,) tensor."""
        out = self.new_f() if out is None else out
        _lib.check(_lib.lib().qln_eval_objective(self._h, self._check(Z, self.dims.z_total, "Z"), self._check(out, self.B, "f")))
        return out

    def grad_f(self, Z, out=None):
        """src/costs.jl:23-34 -> tensor laid out like Z."""
        out = self.new_Z() if out is None else out
        _lib.check(_lib.lib().qln_eval_objective_gradient(
            self._h, self._check(Z, self.dims.z_total, "Z"), self._check(out, self.dims.z_total, "grad")))
        return out

    def eval_c(self, Z, out=None):
        """src/constraints.jl:145-158 -> c buffer (problem b at c_off[b])."""
        out = self.new_c() if out is None else out
        _lib.check(_lib.lib().qln_eval_constraint(
            self._h, self._check(Z, self.dims.z_total, "Z"), self._check(out, self.dims.c_total, "c")))
        return out

    def jac_c(self, Z, out=None, write_constants: bool = True):
        """src/constraints.jl:212-291 -> block-COO values (problem b at j_off[b])."""
        out = self.new_vals() if out is None else out
        flags = _lib.QLN_JAC_WRITE_CONSTANTS if write_constants else 0
        _lib.check(_lib.lib().qln_eval_constraint_jacobian(
            self._h, self._check(Z, self.dims.z_total, "Z"), self._check(out, self.dims.j_total, "vals"), flags))
        return out

    def eval_c_and_jac(self, Z, c=None, vals=None, write_constants: bool = True):
        """The fused hot path: eval_c! + jac_c! in one launch."""
        c = self.new_c() if c is None else c
        vals = self.new_vals() if vals is None else vals
        flags = _lib.QLN_JAC_WRITE_CONSTANTS if write_constants else 0
        _lib.check(_lib.lib().qln_eval_constraint_and_jacobian(
            self._h, self._check(Z, self.dims.z_total, "Z"), self._check(c, self.dims.c_total, "c"),
            self._check(vals, self.dims.j_total, "vals"), flags))
        return c, vals

    def eval_all(self, Z, f=None, grad=None, c=None, vals=None, write_constants: bool = True):
        """f, grad_f, c and the Jacobian values from one read of Z, in one launch (qln_eval_all)."""
        f = self.new_f() if f is None else f
        grad = self.new_Z() if grad is None else grad
        c = self.new_c() if c is None else c
        vals = self.new_vals() if vals is None else vals
        flags = _lib.QLN_JAC_WRITE_CONSTANTS if write_constants else 0
        _lib.check(_lib.lib().qln_eval_all(
            self._h, self._check(Z, self.dims.z_total, "Z"), self._check(f, self.B, "f"),
            self._check(grad, self.dims.z_total, "grad"), self._check(c, self.dims.c_total, "c"),
            self._check(vals, self.dims.j_total, "vals"), flags))
        return f, grad, c, vals

    def eval_f_and_c(self, Z, f=None, c=None):
        """f and c from one read of Z in one launch (qln_eval_objective_and_constraint): what a line search asks for."""
        f = self.new_f() if f is None else f
        c = self.new_c() if c is None else c
        _lib.check(_lib.lib().qln_eval_objective_and_constraint(
            self._h, self._check(Z, self.dims.z_total, "Z"), self._check(f, self.B, "f"), self._check(c, self.dims.c_total, "c")))
        return f, c

    def init_jacobian_constants(self, vals):
        _lib.check(_lib.lib().qln_jacobian_init_constants(self._h, self._check(vals, self.dims.j_total, "vals")))
        return vals

    def jac_vec(self, Z, v, out=None):
        """y = jac_c(Z) @ v for every problem (v in Z's layout, y in c's); the Jacobian is re-derived in registers."""
        self._check(Z, self.dims.z_total, "Z")
        self._check(v, self.dims.z_total, "v")
        out = self.new_c() if out is None else out
        self._check(out, self.dims.c_total, "out")
        _lib.check(_lib.lib().qln_eval_constraint_jvp(self._h, Z.data_ptr(), v.data_ptr(), out.data_ptr()))
        return out

    def jac_t_vec(self, Z, lam, out=None):
        """g = jac_c(Z)' @ lam for every problem (lam in c's layout, g in Z's)."""
        self._check(Z, self.dims.z_total, "Z")
        self._check(lam, self.dims.c_total, "lam")
        out = self.new_Z() if out is None else out
        self._check(out, self.dims.z_total, "out")
        _lib.check(_lib.lib().qln_eval_constraint_vjp(self._h, Z.data_ptr(), lam.data_ptr(), out.data_ptr()))
        return out

    # -- Lagrangian Hessian ---------------------------------------------------------------------
    def hessian_structure(self):
        """0-based (rows, cols), row >= col, of one problem's Hessian segment in the order of its values."""
        return hessian_structure(self.N)

    def new_hvals(self):
        return _torch().zeros(self.h_total, dtype=_torch().float64, device=self._dev())

    def hess_lag(self, Z, sigma, mu, out=None):
        """Lower triangle of sigma_b d2 f + sum_i mu_i d2 c_i for every problem (problem b at b * h_stride).  Z, mu (layout
        of c) and out are device tensors; sigma a (B,) device tensor or None (1.0 for every problem)."""
        out = self.new_hvals() if out is None else out
        sp = None if sigma is None else self._check(sigma, self.B, "sigma")
        _lib.check(_lib.lib().qln_eval_hessian_lagrangian(
            self._h, self._check(Z, self.dims.z_total, "Z"), sp, self._check(mu, self.dims.c_total, "mu"),
            self._check(out, self.h_total, "hvals")))
        return out

    def hess_lag_host(self, Z, sigma, mu):
        """The same with host arrays (MOI mode): returns an (h_total,) numpy array."""
        Z, mu, sigma = self._host_Z(Z), self._host_c(mu, "mu"), self._host_sigma(sigma)
        out = np.zeros(self.h_total)
        _lib.check(_lib.lib().qln_eval_hessian_lagrangian_host(self._h, Z.ctypes.data, _host_ptr(sigma), mu.ctypes.data,
                                                               out.ctypes.data))
        return out

    def hess_lag_vec(self, Z, sigma, mu, v, out=None):
        """y = (sigma_b d2 f + sum_i mu_i d2 c_i) v for every problem, the Hessian never stored.  Z, v and out in Z's layout,
        mu in c's, all device tensors; sigma a (B,) device tensor or None (1.0 for every problem).  out's entries past
        n_nlp are not written."""
        out = self.new_Z() if out is None else out
        sp = None if sigma is None else self._check(sigma, self.B, "sigma")
        _lib.check(_lib.lib().qln_eval_hessian_lagrangian_product(
            self._h, self._check(Z, self.dims.z_total, "Z"), sp, self._check(mu, self.dims.c_total, "mu"),
            self._check(v, self.dims.z_total, "v"), self._check(out, self.dims.z_total, "out")))
        return out

    def hess_lag_vec_host(self, Z, sigma, mu, v):
        """The same with host arrays (MOI mode): returns a (z_total,) numpy array (zeros past n_nlp)."""
        Z, v, mu, sigma = self._host_Z(Z), self._host_Z(v, "v"), self._host_c(mu, "mu"), self._host_sigma(sigma)
        out = np.zeros(self.dims.z_total)
        _lib.check(_lib.lib().qln_eval_hessian_lagrangian_product_host(
            self._h, Z.ctypes.data, _host_ptr(sigma), mu.ctypes.data, v.ctypes.data, out.ctypes.data))
        return out

    # -- TVLQR tracking along reference trajectories ---------------------------------------------
    # Every operation from here to differentiable_estimated_rollout is stated once, as an _op_ method that takes the memory
    # form (_DeviceForm / _HostForm) and the variant's extras as optional arguments and picks the entry point from what is
    # present; the public methods are the wrappers that name the form (DESIGN.md "One body per operation").
    def _op_lqr(self, f, kind, Ztraj, Q, R, Qf, name="Ztraj", events=None, sat=None, model=None, K=None, P=None,
                with_cost_to_go=True):
        """kind: "" (at the handle's schedule), "_guarded" (events required) or "_limited" (sat required, events optional)"""
        Qh, Rh, Qfh = tracking_weights(Q, R, Qf)
        Ztraj = f.Z(Ztraj, name)
        extra = ()
        if kind:
            sat = f.sat(sat) if kind == "_limited" else None
            events = f.events(events) if kind == "_guarded" or events is not None else None
            model = f.model(model)
            extra = (f.ptr(model), f.ptr(events)) + ((f.ptr(sat),) if kind == "_limited" else ())
        K = f.out(K, tracking_k_shape(self.B, self.N), "K", empty=True)
        P = f.out(P, tracking_p_shape(self.B, self.N), "P", empty=True) if with_cost_to_go else None
        _lib.check(f.fn("qln_tracking_lqr" + kind)(self._h, f.ptr(Ztraj), *extra, Qh.ctypes.data, Rh.ctypes.data, Qfh.ctypes.data,
                                                   f.ptr(K), f.ptr(P)))
        return K, P

    def tracking_lqr(self, Zref, Q, R, Qf, K=None, P=None, with_cost_to_go=True):
        """Time-varying LQR gains along the references Zref (device tensor, layout of Z): returns (K, P) with
        K (B, N-1, 4, 15) and P (B, N, 120) packed lower triangles (None without with_cost_to_go).  Only the four forces
        are fed back, du_k = -K_k (x_k - x_ref,k); Q (15), R (4), Qf (15) are diagonal weights (qln_evaluator.h)."""
        return self._op_lqr(_DeviceForm(self), "", Zref, Q, R, Qf, "Zref", K=K, P=P, with_cost_to_go=with_cost_to_go)

    def tracking_lqr_host(self, Zref, Q, R, Qf, with_cost_to_go=True):
        """The same with host arrays (synchronous): returns numpy (K, P)."""
        return self._op_lqr(_HostForm(self), "", Zref, Q, R, Qf, "Zref", with_cost_to_go=with_cost_to_go)

    # -- the closed-loop roll-out and its two sweeps ------------------------------------------------
    # kind picks the entry point: "" (the handle's model), "_model" (a per-problem plant), "_guarded" (touchdown by the guard,
    # with the event record) or "_limited" (clamped forces: limits, the guarded flag and the saturation record).
    def _vjp_want(self, K, want, names):
        want = names if want is None else tuple(want)
        bad = set(want) - set(names)
        if bad:
            raise ValueError(f"want: unknown outputs {sorted(bad)} ({', '.join(names)})")
        if want == names and K is None:
            want = tuple(w for w in names if w != "K")  # the default asks for K_bar only where there are gains
        return want

    def _op_rollout(self, f, kind, Zref, K, x0, model=None, out=None, limits=None, guarded=False, with_events=True,
                    with_sat=True):
        limited = kind == "_limited"
        lim = force_limits(limits) if limited else None
        Zref = f.Z(Zref, "Zref")
        out = f.out(out, (self.dims.z_total,), "out")
        K, x0 = f.K(K), f.x0(x0)
        args = [self._h, f.ptr(Zref), f.ptr(K), f.ptr(x0)]
        if kind:
            model = f.model(model)
            args.append(f.ptr(model))
        if limited:
            args += [lim.ctypes.data, int(bool(guarded))]
        args.append(f.ptr(out))
        ev = sat = None
        if kind in ("_guarded", "_limited"):
            ev = f.zeros((self.B, _lib.TOUCHDOWN_INFO_STRIDE), with_events and (guarded or not limited))
            args.append(f.ptr(ev))
        if limited:
            sat = f.zeros((self.B, self.N - 1), with_sat)
            args.append(f.ptr(sat))
        _lib.check(f.fn("qln_tracking_rollout" + kind)(*args))
        return (out, ev, sat) if limited else (out, ev) if kind == "_guarded" else out

    def _op_rollout_vjp(self, f, kind, Zref, Zout, Zbar, K, model, want, events=None, sat=None):
        """Returns (Zref_bar, K_bar, x0_bar, model_bar); model_bar is None for kind ""."""
        want = self._vjp_want(K, want, ("Zref", "K", "x0", "model") if kind else ("Zref", "K", "x0"))
        Zref, Zout, Zbar = f.Z(Zref, "Zref"), f.Z(Zout, "Zout"), f.Z(Zbar, "Zbar")
        sat = f.sat(sat) if kind == "_limited" else None
        events = f.events(events) if kind == "_guarded" or events is not None else None
        K, model = f.K(K), f.model(model)
        zb = f.zeros((self.dims.z_total,), "Zref" in want)
        kb = f.zeros(tracking_k_shape(self.B, self.N), "K" in want)
        xb = f.zeros((self.B, n), "x0" in want)
        mb = f.zeros((self.B, _lib.MODEL_NP), "model" in want)
        args = [self._h, f.ptr(Zref), f.ptr(K), f.ptr(Zout)]
        if kind:
            args.append(f.ptr(model))
        if kind in ("_guarded", "_limited"):
            args.append(f.ptr(events))
        if kind == "_limited":
            args.append(f.ptr(sat))
        args += [f.ptr(Zbar), f.ptr(zb), f.ptr(kb), f.ptr(xb)]
        if kind:
            args.append(f.ptr(mb))
        _lib.check(f.fn("qln_tracking_rollout" + kind + "_vjp")(*args))
        return zb, kb, xb, mb

    def _op_rollout_jvp(self, f, kind, Zref, Zout, K, model, Zref_dot, K_dot, x0_dot, model_dot, out, events=None, sat=None,
                        with_event_dot=True):
        Zref, Zout = f.Z(Zref, "Zref"), f.Z(Zout, "Zout")
        sat = f.sat(sat) if kind == "_limited" else None
        events = f.events(events) if kind == "_guarded" or events is not None else None
        K, model = f.K(K), f.model(model)
        Zref_dot, K_dot, x0_dot = f.Z_opt(Zref_dot, "Zref_dot"), f.K(K_dot, "K_dot"), f.x0(x0_dot, "x0_dot")
        model_dot = f.model(model_dot, "model_dot")
        out = f.out(out, (self.dims.z_total,), "out")
        args = [self._h, f.ptr(Zref), f.ptr(K), f.ptr(Zout)]
        if kind:
            args.append(f.ptr(model))
        if kind in ("_guarded", "_limited"):
            args.append(f.ptr(events))
        if kind == "_limited":
            args.append(f.ptr(sat))
        args += [f.ptr(Zref_dot), f.ptr(K_dot), f.ptr(x0_dot)]
        if kind:
            args.append(f.ptr(model_dot))
        args.append(f.ptr(out))
        if kind in ("", "_model"):
            _lib.check(f.fn("qln_tracking_rollout" + kind + "_jvp")(*args))
            return out
        ed = f.zeros((self.B, _lib.TOUCHDOWN_INFO_STRIDE), with_event_dot and events is not None)
        _lib.check(f.fn("qln_tracking_rollout" + kind + "_jvp")(*args, f.ptr(ed)))
        return out, ed

    # the names quadruped_landing_amd/rollout_grad.py calls: the device form, m the per-problem plant
    def _rollout(self, m, Zref, K, x0, model, out):
        return self._op_rollout(_DeviceForm(self), "_model" if m else "", Zref, K, x0, model, out)

    def _rollout_vjp(self, m, Zref, Zout, Zbar, K, model, want):
        return self._op_rollout_vjp(_DeviceForm(self), "_model" if m else "", Zref, Zout, Zbar, K, model, want)

    def _rollout_jvp(self, m, Zref, Zout, K, model, Zref_dot, K_dot, x0_dot, model_dot, out):
        return self._op_rollout_jvp(_DeviceForm(self), "_model" if m else "", Zref, Zout, K, model, Zref_dot, K_dot, x0_dot,
                                    model_dot, out)

    def tracking_rollout(self, Zref, K=None, x0=None, out=None):
        """Closed-loop roll-out of the hybrid dynamics from x0 ((B, 15) device tensor, None: the handle's x0) with
        F_k = F_ref,k - K_k (x_k - x_ref,k) and h_k = h_ref,k; K None is the open-loop roll-out.  Returns Zout in the
        layout of Z (entries past n_nlp are not written).  out must not overlap Zref."""
        return self._op_rollout(_DeviceForm(self), "", Zref, K, x0, out=out)

    def tracking_rollout_host(self, Zref, K=None, x0=None):
        """The same with host arrays (synchronous): returns a (z_total,) numpy array (zeros past n_nlp)."""
        return self._op_rollout(_HostForm(self), "", Zref, K, x0)

    # -- reverse-mode derivative of the closed-loop roll-out ---------------------------------------
    def tracking_rollout_vjp(self, Zref, Zout, Zbar, K=None, want=None):
        """Reverse sweep of tracking_rollout at the trajectory Zout (device tensors, layout of Z): the cotangent Zbar of
        (Zout's states and applied controls) -> (Zref_bar, K_bar, x0_bar), each None unless named in want (default: all
        three, K_bar only when K is given).  Zref_bar is laid out like Z (zeros past n_nlp on a fresh buffer), K_bar like K
        (B, N-1, 4, 15), x0_bar (B, 15).  Stream-ordered; semantics in include/qln_evaluator.h."""
        return self._op_rollout_vjp(_DeviceForm(self), "", Zref, Zout, Zbar, K, None, want)[:3]

    def tracking_rollout_vjp_host(self, Zref, Zout, Zbar, K=None, want=None):
        """The same with host arrays (synchronous): numpy (Zref_bar (z_total,), K_bar (B, N-1, 4, 15), x0_bar (B, 15))."""
        return self._op_rollout_vjp(_HostForm(self), "", Zref, Zout, Zbar, K, None, want)[:3]

    # -- forward-mode derivative of the closed-loop roll-out ---------------------------------------
    def tracking_rollout_jvp(self, Zref, Zout, K=None, Zref_dot=None, K_dot=None, x0_dot=None, out=None):
        """Forward sweep of tracking_rollout at the trajectory Zout (device tensors): the tangents Zref_dot (layout of Z),
        K_dot (B, N-1, 4, 15) and x0_dot (B, 15) -- each None for zero, at least one given, K_dot only with K -- to the
        tangent Zout_dot of Zout's states and applied controls, in the layout of Z (zeros past n_nlp on a fresh buffer; out
        must overlap no input).  Stream-ordered; semantics in include/qln_evaluator.h."""
        return self._op_rollout_jvp(_DeviceForm(self), "", Zref, Zout, K, None, Zref_dot, K_dot, x0_dot, None, out)

    def tracking_rollout_jvp_host(self, Zref, Zout, K=None, Zref_dot=None, K_dot=None, x0_dot=None):
        """The same with host arrays (synchronous): returns a (z_total,) numpy array (zeros past n_nlp)."""
        return self._op_rollout_jvp(_HostForm(self), "", Zref, Zout, K, None, Zref_dot, K_dot, x0_dot, None, None)

    # -- the roll-out and its sweeps with a per-problem plant model --------------------------------
    def plant_models(self, models=None):
        """(B, 4) float64 device tensor of per-problem plant models (g, mb, mf, lb): a PlanarQuadruped tiled over the batch
        (None: the handle's own model), or a sequence of B of them."""
        from .planar_quadruped import plant_models

        return _torch().from_numpy(plant_models(self.model if models is None else models, self.B)).to(self._dev())

    def tracking_rollout_model(self, Zref, K=None, x0=None, model=None, out=None):
        """tracking_rollout with a per-problem PLANT: model is a (B, 4) float64 device tensor of (g, mb, mf, lb) rows
        (plant_models; None: the handle's model, then bit for bit tracking_rollout).  The gains and the references stay
        what they are: only the dynamics that are rolled out read the problem's model (qln_evaluator.h)."""
        return self._op_rollout(_DeviceForm(self), "_model", Zref, K, x0, model, out)

    def tracking_rollout_model_host(self, Zref, K=None, x0=None, model=None):
        """The same with host arrays (synchronous): returns a (z_total,) numpy array (zeros past n_nlp).  A non-finite
        model entry, or mb, mf or lb <= 0, is refused."""
        return self._op_rollout(_HostForm(self), "_model", Zref, K, x0, model)

    def tracking_rollout_model_vjp(self, Zref, Zout, Zbar, K=None, model=None, want=None):
        """Reverse sweep of tracking_rollout_model at the trajectory Zout: tracking_rollout_vjp with the blocks at each
        problem's model, and a fourth output model_bar (B, 4), the cotangent of `model`.  Returns (Zref_bar, K_bar, x0_bar,
        model_bar), each None unless named in want (default: all, K_bar only when K is given)."""
        return self._op_rollout_vjp(_DeviceForm(self), "_model", Zref, Zout, Zbar, K, model, want)

    def tracking_rollout_model_vjp_host(self, Zref, Zout, Zbar, K=None, model=None, want=None):
        """The same with host arrays (synchronous): numpy (Zref_bar, K_bar, x0_bar, model_bar (B, 4))."""
        return self._op_rollout_vjp(_HostForm(self), "_model", Zref, Zout, Zbar, K, model, want)

    def tracking_rollout_model_jvp(self, Zref, Zout, K=None, model=None, Zref_dot=None, K_dot=None, x0_dot=None,
                                   model_dot=None, out=None):
        """Forward sweep of tracking_rollout_model at the trajectory Zout: tracking_rollout_jvp with the blocks at each
        problem's model and a fourth tangent model_dot (B, 4) -- each tangent None for zero, at least one given."""
        return self._op_rollout_jvp(_DeviceForm(self), "_model", Zref, Zout, K, model, Zref_dot, K_dot, x0_dot, model_dot, out)

    def tracking_rollout_model_jvp_host(self, Zref, Zout, K=None, model=None, Zref_dot=None, K_dot=None, x0_dot=None,
                                        model_dot=None):
        """The same with host arrays (synchronous): returns a (z_total,) numpy array (zeros past n_nlp)."""
        return self._op_rollout_jvp(_HostForm(self), "_model", Zref, Zout, K, model, Zref_dot, K_dot, x0_dot, model_dot, None)

    # -- the roll-out with guard-triggered touchdown -------------------------------------------------
    def tracking_rollout_guarded(self, Zref, K=None, x0=None, model=None, out=None, with_events=True):
        """tracking_rollout_model with touchdown when the free foot reaches the ground instead of at the handle's k_trans
        (which is not read): the event is located inside its step in closed form, the step is split there, and the problem
        is in mode 3 from then on.  Returns (Zout, events): events is a (B, 8) float64 device tensor of {knot (-1: none),
        tau, clock at touchdown, the foot's x, its (vx, vy) before the jump map, the smallest standing-foot vertical force,
        0}, None without with_events.  Zout is not a trajectory of the handle's schedule: its derivatives are
        tracking_rollout_guarded_jvp / _vjp, which take the events; the other jvp / vjp / covariance calls do not apply to it
        (qln_evaluator.h)."""
        return self._op_rollout(_DeviceForm(self), "_guarded", Zref, K, x0, model, out, with_events=with_events)

    def tracking_rollout_guarded_host(self, Zref, K=None, x0=None, model=None, with_events=True):
        """The same with host arrays (synchronous): returns numpy (Zout (z_total,), zeros past n_nlp, events (B, 8) or None).
        A non-finite model entry, or mb, mf or lb <= 0, is refused."""
        return self._op_rollout(_HostForm(self), "_guarded", Zref, K, x0, model, with_events=with_events)

    # -- forward and reverse sweeps through the guard-triggered touchdown ----------------------------
    def tracking_rollout_guarded_jvp(self, Zref, Zout, events, K=None, model=None, Zref_dot=None, K_dot=None, x0_dot=None,
                                     model_dot=None, out=None, with_event_dot=True):
        """Forward sweep of tracking_rollout_guarded at the trajectory (Zout, events) it returned, at fixed touchdown knot:
        tracking_rollout_model_jvp's tangents and rules, with the composite touchdown step and the derivative of tau
        (qln_evaluator.h).  Returns (Zout_dot, event_dot): event_dot is a (B, 8) device tensor holding d tau in entry 1 and
        the touchdown clock's tangent in entry 2, zeros elsewhere and for a problem that does not land; None without
        with_event_dot."""
        return self._op_rollout_jvp(_DeviceForm(self), "_guarded", Zref, Zout, K, model, Zref_dot, K_dot, x0_dot, model_dot, out,
                                    events, with_event_dot=with_event_dot)

    def tracking_rollout_guarded_jvp_host(self, Zref, Zout, events, K=None, model=None, Zref_dot=None, K_dot=None, x0_dot=None,
                                          model_dot=None, with_event_dot=True):
        """The same with host arrays (synchronous): numpy (Zout_dot (z_total,), event_dot (B, 8) or None).  A knot that is
        not an integer in [-1, N-2], or a tau that is not finite or is negative, is refused."""
        return self._op_rollout_jvp(_HostForm(self), "_guarded", Zref, Zout, K, model, Zref_dot, K_dot, x0_dot, model_dot, None,
                                    events, with_event_dot=with_event_dot)

    def tracking_rollout_guarded_vjp(self, Zref, Zout, events, Zbar, K=None, model=None, want=None):
        """Reverse sweep of tracking_rollout_guarded at the trajectory (Zout, events) it returned, the exact adjoint of
        tracking_rollout_guarded_jvp: tracking_rollout_model_vjp's cotangents and rules.  Returns (Zref_bar, K_bar, x0_bar,
        model_bar), each None unless named in want (default: all, K_bar only when K is given)."""
        return self._op_rollout_vjp(_DeviceForm(self), "_guarded", Zref, Zout, Zbar, K, model, want, events)

    def tracking_rollout_guarded_vjp_host(self, Zref, Zout, events, Zbar, K=None, model=None, want=None):
        """The same with host arrays (synchronous): numpy (Zref_bar, K_bar, x0_bar, model_bar (B, 4))."""
        return self._op_rollout_vjp(_HostForm(self), "_guarded", Zref, Zout, Zbar, K, model, want, events)

    # -- covariance propagation through the closed-loop roll-out -----------------------------------
    def _op_covariance(self, f, guarded, Zout, K, Sigma0, W, with_sigma, with_marginals, Sigma=None, marg=None, events=None,
                       model=None, with_event_var=True):
        Zout = f.Z(Zout, "Zout")
        events = f.events(events) if guarded else None
        K = f.K(K)
        model = f.model(model) if guarded else None
        s0, nb = f.sigma0(Sigma0)
        Wh = tracking_noise(W)
        S = f.out(Sigma, tracking_p_shape(self.B, self.N), "Sigma", empty=True) if with_sigma else None
        mg = f.out(marg, (self.B, self.N, _lib.TRACK_MARG_STRIDE), "marg", empty=True) if with_marginals else None
        if not guarded:
            _lib.check(f.fn("qln_tracking_covariance")(self._h, f.ptr(Zout), f.ptr(K), f.ptr(s0), nb, _host_ptr(Wh), f.ptr(S),
                                                       f.ptr(mg)))
            return S, mg
        ev = f.zeros((self.B, 2), with_event_var)
        _lib.check(f.fn("qln_tracking_covariance_guarded")(self._h, f.ptr(Zout), f.ptr(K), f.ptr(model), f.ptr(events), f.ptr(s0),
                                                           nb, _host_ptr(Wh), f.ptr(S), f.ptr(mg), f.ptr(ev)))
        return S, mg, ev

    def tracking_covariance(self, Zout, K=None, Sigma0=None, W=None, with_sigma=True, with_marginals=True, Sigma=None,
                            marg=None):
        """Sigma_{k+1} = (A_k - B_k K_k) Sigma_k (A_k - B_k K_k)' + diag(W) along the trajectory Zout (device tensor, layout
        of Z; for the nominal case the reference itself), K None for the open loop.  Sigma0: a 15-vector of variances, a
        15x15 matrix, (B, 15, 15), or packed (numpy or a CUDA tensor of packed tiles).  Returns (Sigma, marg): Sigma
        (B, N, 120) packed lower triangles (unpack_covariance), marg (B, N, 8) = clearance variance, four force variances,
        the two foot-height variances, trace; each None unless asked for (Sigma / marg: buffers to write into instead of
        fresh ones).  Stream-ordered (qln_evaluator.h)."""
        return self._op_covariance(_DeviceForm(self), False, Zout, K, Sigma0, W, with_sigma, with_marginals, Sigma, marg)

    def tracking_covariance_host(self, Zout, K=None, Sigma0=None, W=None, with_sigma=True, with_marginals=True):
        """The same with host arrays (synchronous): numpy (Sigma (B, N, 120), marg (B, N, 8))."""
        return self._op_covariance(_HostForm(self), False, Zout, K, Sigma0, W, with_sigma, with_marginals)

    # -- gains and covariances through the guard-triggered touchdown --------------------------------
    def tracking_lqr_guarded(self, Ztraj, events, Q, R, Qf, model=None, K=None, P=None, with_cost_to_go=True):
        """tracking_lqr through the guarded touchdown: gains along Ztraj, as a rule the Zout tracking_rollout_guarded returned
        for the plan, with its events (B, 8), on the blocks of tracking_rollout_guarded_jvp -- the composite step with the
        derivative of tau at the touchdown knot (qln_evaluator.h).  model: (B, 4) device tensor or None (the handle's).
        Returns (K, P) as tracking_lqr."""
        return self._op_lqr(_DeviceForm(self), "_guarded", Ztraj, Q, R, Qf, events=events, model=model, K=K, P=P,
                            with_cost_to_go=with_cost_to_go)

    def tracking_lqr_guarded_host(self, Ztraj, events, Q, R, Qf, model=None, with_cost_to_go=True):
        """The same with host arrays (synchronous): returns numpy (K, P).  The events' and the models' values are checked as
        by the guarded sweeps' host forms."""
        return self._op_lqr(_HostForm(self), "_guarded", Ztraj, Q, R, Qf, events=events, model=model,
                            with_cost_to_go=with_cost_to_go)

    def tracking_covariance_guarded(self, Zout, events, K=None, Sigma0=None, W=None, model=None, with_sigma=True,
                                    with_marginals=True, with_event_var=True, Sigma=None, marg=None):
        """tracking_covariance through the guarded touchdown, at the (Zout, events) tracking_rollout_guarded returned, at fixed
        touchdown knot.  Returns (Sigma, marg, event_var): the first two as tracking_covariance, event_var a (B, 2) device
        tensor with the variance of tau and of the touchdown clock (zeros for a problem that does not land); each None
        unless asked for."""
        return self._op_covariance(_DeviceForm(self), True, Zout, K, Sigma0, W, with_sigma, with_marginals, Sigma, marg, events,
                                   model, with_event_var)

    def tracking_covariance_guarded_host(self, Zout, events, K=None, Sigma0=None, W=None, model=None, with_sigma=True,
                                         with_marginals=True, with_event_var=True):
        """The same with host arrays (synchronous): numpy (Sigma (B, N, 120), marg (B, N, 8), event_var (B, 2))."""
        return self._op_covariance(_HostForm(self), True, Zout, K, Sigma0, W, with_sigma, with_marginals, events=events,
                                   model=model, with_event_var=with_event_var)

    # -- the Kalman filter and the LQG covariance: the controller feeds back an estimate -------------
    def _op_kalman(self, f, guarded, Zout, events, K, H, V, Sigma0, W, model, with_gains, with_pest, with_sigma, with_marginals,
                   with_event_var):
        """with_sigma, with_marginals and with_event_var: None for "where there are gains" """
        Hh, Vh = measurement_model(H, V)
        ny = Hh.shape[0]
        with_sigma, with_marginals, with_event_var = ((K is not None) if w is None else w
                                                      for w in (with_sigma, with_marginals, with_event_var))
        Zout, K = f.Z(Zout, "Zout"), f.K(K)
        s0, nb = f.sigma0(Sigma0)
        Wh = tracking_noise(W)
        Hd = f.H(Hh)
        Lg = f.empty(tracking_l_shape(self.B, self.N, ny), with_gains)
        Pe = f.empty(tracking_p_shape(self.B, self.N), with_pest)
        S = f.empty(tracking_p_shape(self.B, self.N), with_sigma)
        mg = f.empty((self.B, self.N, _lib.TRACK_MARG_STRIDE), with_marginals)
        tail = (f.ptr(Hd), ny, Vh.ctypes.data, f.ptr(s0), nb, _host_ptr(Wh), f.ptr(Lg), f.ptr(Pe), f.ptr(S), f.ptr(mg))
        if not guarded:
            _lib.check(f.fn("qln_tracking_kalman")(self._h, f.ptr(Zout), f.ptr(K), *tail))
            return Lg, Pe, S, mg
        events, model = f.events(events), f.model(model)
        ev = f.zeros((self.B, 2), with_event_var)
        _lib.check(f.fn("qln_tracking_kalman_guarded")(self._h, f.ptr(Zout), f.ptr(K), f.ptr(model), f.ptr(events), *tail,
                                                       f.ptr(ev)))
        return Lg, Pe, S, mg, ev

    def tracking_kalman(self, Zout, H, V, K=None, Sigma0=None, W=None, with_gains=True, with_pest=True, with_sigma=None,
                        with_marginals=None):
        """The Kalman filter and the LQG covariance along Zout: tracking_covariance for a controller that feeds back the
        estimate xhat_k|k built from the measurements y_k = H dx_k + v_k, var v = V (measurement_model), at every knot
        (qln_evaluator.h).  Returns (L, Pest, Sigma, marg): the filter gains (B, N, 15, ny), the error covariances P^+_k and the
        true state's covariances X_k = M_k + P^+_k as packed (B, N, 120) tiles (unpack_covariance), and marg (B, N, 8) as
        tracking_covariance's on X_k, with the applied-force variances diag(K M K'); each None unless asked for.  K None is the
        filter alone: L and Pest only (with_sigma / with_marginals default to K being given).  Stream-ordered."""
        return self._op_kalman(_DeviceForm(self), False, Zout, None, K, H, V, Sigma0, W, None, with_gains, with_pest, with_sigma,
                               with_marginals, False)

    def tracking_kalman_host(self, Zout, H, V, K=None, Sigma0=None, W=None, with_gains=True, with_pest=True, with_sigma=None,
                             with_marginals=None):
        """The same with host arrays (synchronous): numpy (L, Pest, Sigma, marg)."""
        return self._op_kalman(_HostForm(self), False, Zout, None, K, H, V, Sigma0, W, None, with_gains, with_pest, with_sigma,
                               with_marginals, False)

    def tracking_kalman_guarded(self, Zout, events, H, V, K=None, Sigma0=None, W=None, model=None, with_gains=True,
                                with_pest=True, with_sigma=None, with_marginals=None, with_event_var=None):
        """tracking_kalman through the guarded touchdown, at the (Zout, events) tracking_rollout_guarded returned, at fixed
        touchdown knot.  Returns (L, Pest, Sigma, marg, event_var): the first four as tracking_kalman, event_var a (B, 2)
        device tensor with the variance of tau and of the touchdown clock under estimate feedback (zeros for a problem that
        does not land); each None unless asked for."""
        return self._op_kalman(_DeviceForm(self), True, Zout, events, K, H, V, Sigma0, W, model, with_gains, with_pest, with_sigma,
                               with_marginals, with_event_var)

    def tracking_kalman_guarded_host(self, Zout, events, H, V, K=None, Sigma0=None, W=None, model=None, with_gains=True,
                                     with_pest=True, with_sigma=None, with_marginals=None, with_event_var=None):
        """The same with host arrays (synchronous): numpy (L, Pest, Sigma, marg, event_var)."""
        return self._op_kalman(_HostForm(self), True, Zout, events, K, H, V, Sigma0, W, model, with_gains, with_pest, with_sigma,
                               with_marginals, with_event_var)

    # -- the forward sweep through the filter's design ---------------------------------------------------
    KALMAN_JVP_OUT = ("Lgain", "Pest", "logdet")

    def _op_kalman_jvp(self, f, guarded, Zout, events, Lgain, H, V, Sigma0_dot, W_dot, V_dot, model, want):
        """One path for the four forms.  Returns a dict of the outputs asked for (want None: all three)."""
        Hh, Vh = measurement_model(H, V)
        ny = Hh.shape[0]
        want = self.KALMAN_JVP_OUT if want is None else tuple(want)
        bad = set(want) - set(self.KALMAN_JVP_OUT)
        if bad:
            raise ValueError(f"want: unknown outputs {sorted(bad)} ({', '.join(self.KALMAN_JVP_OUT)})")
        if Lgain is None:
            raise ValueError(f"Lgain is required: the gains tracking_kalman{f.suffix} returned for (Zout, H, V)")
        if Sigma0_dot is None and W_dot is None and V_dot is None:
            raise ValueError("a direction is required: at least one of Sigma0_dot, W_dot and V_dot")
        Wd = tracking_noise(W_dot)
        Vd = None
        if V_dot is not None:
            if np.ndim(V_dot) > 1 or (np.ndim(V_dot) == 1 and np.shape(V_dot)[0] != ny):
                raise ValueError(f"V_dot of shape {np.shape(V_dot)}: expected a scalar or ({ny},)")
            Vd = np.ascontiguousarray(np.broadcast_to(np.asarray(V_dot, dtype=np.float64), (ny,)))
        for name, a in (("W_dot", Wd), ("V_dot", Vd)):
            if a is not None and not np.isfinite(a).all():
                raise ValueError(f"{name} is not finite")
        Zout = f.Z(Zout, "Zout")
        Lgain = f.arr(Lgain, self.B * self.N * n * ny, "Lgain")
        s0, nb = (None, 1) if Sigma0_dot is None else f.sigma0(Sigma0_dot)
        Hd = f.H(Hh)
        B, N = self.B, self.N
        shapes = dict(Lgain=tracking_l_shape(B, N, ny), Pest=tracking_p_shape(B, N), logdet=(B, N))
        res = {k: f.empty(shapes[k]) for k in self.KALMAN_JVP_OUT if k in want}
        extra = ()
        if guarded:
            events, model = f.events(events), f.model(model)
            extra = (f.ptr(model), f.ptr(events))
        _lib.check(f.fn("qln_kalman_design" + ("_guarded" if guarded else "") + "_jvp")(
            self._h, f.ptr(Zout), *extra, f.ptr(Lgain), f.ptr(Hd), ny, Vh.ctypes.data, f.ptr(s0), nb, _host_ptr(Wd), _host_ptr(Vd),
            *(f.ptr(res.get(k)) for k in self.KALMAN_JVP_OUT)))
        return res

    def tracking_kalman_jvp(self, Zout, Lgain, H, V, Sigma0_dot=None, W_dot=None, V_dot=None, events=None, model=None,
                            guarded=False, want=None):
        """Forward sweep through the design of tracking_kalman (guarded: of tracking_kalman_guarded, at events and model): how
        the gains, the error covariances P^+_k and log det S_k move along a direction (Sigma0_dot in any form Sigma0 takes and of
        either sign, W_dot a scalar or (15,), V_dot a scalar or (ny,); each optional, at least one), at the gains Lgain the design
        returned for (Zout, H, V) -- which the call cannot check (qln_kalman_design_jvp).  want: the outputs by name, of Lgain
        (B, N, 15, ny), Pest (B, N, 120) packed and logdet (B, N); default all.  Returns a dict of device tensors; which are asked
        for changes no other's bits.  Stream-ordered."""
        return self._op_kalman_jvp(_DeviceForm(self), guarded, Zout, events, Lgain, H, V, Sigma0_dot, W_dot, V_dot, model, want)

    def tracking_kalman_jvp_host(self, Zout, Lgain, H, V, Sigma0_dot=None, W_dot=None, V_dot=None, events=None, model=None,
                                 guarded=False, want=None):
        """The same with host arrays (synchronous): a dict of numpy arrays."""
        return self._op_kalman_jvp(_HostForm(self), guarded, Zout, events, Lgain, H, V, Sigma0_dot, W_dot, V_dot, model, want)

    def landing_loglik_jvp(self, Zout, Zref, Zrec, Lgain, H, V, Xhat, innov, Sigma0_dot=None, W_dot=None, V_dot=None, events=None,
                           model=None, guarded_design=False, events_hat=None, guarded=False, filter_model=None):
        """The TOTAL derivative of landing_filter's log-likelihood along a direction (Sigma0_dot, W_dot, V_dot) of the design's
        noise, through the gains' design: tracking_kalman_jvp along the design's trajectory Zout (guarded_design: with events and
        model), landing_filter_jvp of the record (Zref, Zrec, Xhat, innov; guarded: with events_hat; filter_model: the records'
        own models) with that Lgain_dot and no score term, and on the device
            nis_dot_k  = innov' Sinv innov_dot + innov_dot' Sinv innov + innov' Sinv_dot innov,   Sinv = diag(1/V) (I - H L),
            Sinv_dot   = -diag(V_dot / V^2) (I - H L) - diag(1/V) H Lgain_dot,
            loglik_dot = -1/2 sum_k (nis_dot_k + logdet_dot_k).
        Device tensors in; returns (loglik_dot (B,), nis_dot (B, N), logdet_dot (B, N))."""
        T = _torch()
        Hh, Vh = measurement_model(H, V)
        ny = Hh.shape[0]
        d = self.tracking_kalman_jvp(Zout, Lgain, H, V, Sigma0_dot, W_dot, V_dot, events, model, guarded_design,
                                     want=("Lgain", "logdet"))
        s = self.landing_filter_jvp(Zref, Zrec, Lgain, H, Xhat, innov=innov, model=filter_model, events_hat=events_hat,
                                    guarded=guarded, Lgain_dot=d["Lgain"], want=("innov",))
        dev = self._dev()
        Ht, Vt = T.from_numpy(np.array(Hh)).to(dev), T.from_numpy(np.array(Vh)).to(dev)
        Vd = T.zeros(ny, dtype=T.float64, device=dev) if V_dot is None else T.from_numpy(
            np.array(np.broadcast_to(np.asarray(V_dot, dtype=np.float64), (ny,)))).to(dev)
        L, Ld = Lgain.reshape(self.B, self.N, n, ny), d["Lgain"]
        iv, ivd = innov.reshape(self.B, self.N, ny), s["innov"]
        G = T.eye(ny, dtype=T.float64, device=dev) - T.einsum("ri,bkis->bkrs", Ht, L)  # I - H L
        Sinv = G / Vt[:, None]
        Sinv_dot = -(Vd / (Vt * Vt))[:, None] * G - T.einsum("ri,bkis->bkrs", Ht, Ld) / Vt[:, None]
        nis_dot = (T.einsum("bkr,bkrs,bks->bk", iv, Sinv, ivd) + T.einsum("bkr,bkrs,bks->bk", ivd, Sinv, iv)
                   + T.einsum("bkr,bkrs,bks->bk", iv, Sinv_dot, iv))
        return -0.5 * (nis_dot + d["logdet"]).sum(dim=1), nis_dot, d["logdet"]

    # -- the reverse sweep through the filter's design ---------------------------------------------------
    KALMAN_VJP_OUT = ("Sigma0", "W", "V")

    def _op_kalman_vjp(self, f, guarded, Zout, events, Lgain, H, V, Lgain_bar, Pest_bar, logdet_bar, model, want, reduce):
        """One path for the four forms.  Returns a dict of the outputs asked for (want None: all three)."""
        Hh, Vh = measurement_model(H, V)
        ny = Hh.shape[0]
        want = self.KALMAN_VJP_OUT if want is None else tuple(want)
        bad = set(want) - set(self.KALMAN_VJP_OUT)
        if bad:
            raise ValueError(f"want: unknown outputs {sorted(bad)} ({', '.join(self.KALMAN_VJP_OUT)})")
        if not want:
            raise ValueError(f"want: at least one of {', '.join(self.KALMAN_VJP_OUT)}")
        if Lgain is None:
            raise ValueError(f"Lgain is required: the gains tracking_kalman{f.suffix} returned for (Zout, H, V)")
        if Lgain_bar is None and Pest_bar is None and logdet_bar is None:
            raise ValueError("a cotangent is required: at least one of Lgain_bar, Pest_bar and logdet_bar")
        B, N = self.B, self.N
        Zout = f.Z(Zout, "Zout")
        Lgain = f.arr(Lgain, B * N * n * ny, "Lgain")
        Lb = f.opt(Lgain_bar, B * N * n * ny, "Lgain_bar")
        Pb = f.opt(Pest_bar, B * N * _lib.TRACK_P_NNZ, "Pest_bar")
        lb = f.opt(logdet_bar, B * N, "logdet_bar")
        Hd = f.H(Hh)
        shapes = dict(Sigma0=(B, _lib.TRACK_P_NNZ), W=(B, n), V=(B, ny))
        res = {k: f.empty(shapes[k]) for k in self.KALMAN_VJP_OUT if k in want}
        extra = ()
        if guarded:
            events, model = f.events(events), f.model(model)
            extra = (f.ptr(model), f.ptr(events))
        _lib.check(f.fn("qln_noise_design" + ("_guarded" if guarded else "") + "_vjp")(
            self._h, f.ptr(Zout), *extra, f.ptr(Lgain), f.ptr(Hd), ny, Vh.ctypes.data, f.ptr(Lb), f.ptr(Pb), f.ptr(lb),
            *(f.ptr(res.get(k)) for k in self.KALMAN_VJP_OUT)))
        if reduce:
            for k in ("W", "V"):
                if k in res:
                    res[k] = res[k].sum(0)
        return res

    def tracking_kalman_vjp(self, Zout, Lgain, H, V, Lgain_bar=None, Pest_bar=None, logdet_bar=None, events=None, model=None,
                            guarded=False, want=None, reduce=False):
        """Reverse sweep through the design of tracking_kalman (guarded: of tracking_kalman_guarded, at events and model): the
        transpose of tracking_kalman_jvp's map between the arrays as stored (qln_noise_design_vjp), at the gains Lgain the design
        returned for (Zout, H, V).  The cotangents Lgain_bar (B, N, 15, ny), Pest_bar (B, N, 120) packed and logdet_bar (B, N), of
        any sign, each optional (None: zero), at least one.  want: the outputs by name, of Sigma0 (B, 120) packed, W (B, 15) and V
        (B, ny), per problem; default all.  reduce: W and V summed over the batch, (15,) and (ny,), as tracking_kalman_jvp shares
        W_dot and V_dot over it.  With the packed convention of the header, <cotangents, tracking_kalman_jvp's outputs> =
        <these, its direction> over the stored arrays.  Returns a dict of device tensors; which are asked for changes no other's
        bits.  Stream-ordered."""
        return self._op_kalman_vjp(_DeviceForm(self), guarded, Zout, events, Lgain, H, V, Lgain_bar, Pest_bar, logdet_bar, model,
                                   want, reduce)

    def tracking_kalman_vjp_host(self, Zout, Lgain, H, V, Lgain_bar=None, Pest_bar=None, logdet_bar=None, events=None, model=None,
                                 guarded=False, want=None, reduce=False):
        """The same with host arrays (synchronous): a dict of numpy arrays."""
        return self._op_kalman_vjp(_HostForm(self), guarded, Zout, events, Lgain, H, V, Lgain_bar, Pest_bar, logdet_bar, model,
                                   want, reduce)

    def landing_loglik_grad(self, Zout, Zref, Zrec, Lgain, H, V, Xhat, innov, events=None, model=None, guarded_design=False,
                            events_hat=None, guarded=False, filter_model=None):
        """The gradient of each record's landing_filter log-likelihood with respect to the design's noise (Sigma0, W, V), through
        the gains' design, in one filter sweep and one design sweep, both reverse -- landing_loglik_jvp's arguments without the
        direction, and its value along any direction is the inner product with this:
            innov_bar_k  = -1/2 (Sinv + Sinv') innov_k,   Sinv = diag(1/V) (I - H L_k)     -> landing_filter_vjp, asking for Lgain
            Lgain_bar_k += 1/2 H' (innov_k ./ V) innov_k'                                   (nis reads L_k itself)
            tracking_kalman_vjp(Lgain_bar, logdet_bar = -1/2)                               -> Sigma0, W, V per record
            V[a]        += 1/2 sum_k innov_k[a] ((I - H L_k) innov_k)[a] / V_a^2            (nis reads V itself)
        Device tensors in; returns a dict of device tensors Sigma0 (B, 120) packed (an off-diagonal entry is the derivative along
        both of its sides), W (B, 15) and V (B, ny), per record."""
        T = _torch()
        Hh, Vh = measurement_model(H, V)
        ny = Hh.shape[0]
        dev = self._dev()
        Ht, Vt = T.from_numpy(np.array(Hh)).to(dev), T.from_numpy(np.array(Vh)).to(dev)
        L, iv = Lgain.reshape(self.B, self.N, n, ny), innov.reshape(self.B, self.N, ny)
        G = T.eye(ny, dtype=T.float64, device=dev) - T.einsum("ri,bkis->bkrs", Ht, L)  # I - H L
        Sinv = G / Vt[:, None]
        innov_bar = -0.5 * T.einsum("bkrs,bks->bkr", Sinv + Sinv.transpose(-1, -2), iv).contiguous()
        s = self.landing_filter_vjp(Zref, Zrec, Lgain, H, Xhat, innov=innov, model=filter_model, events_hat=events_hat,
                                    guarded=guarded, innov_bar=innov_bar, want=("Lgain",))
        Lb = (s["Lgain"].reshape(self.B, self.N, n, ny) + 0.5 * T.einsum("ri,bkr,bks->bkis", Ht, iv / Vt, iv)).contiguous()
        lb = T.full((self.B, self.N), -0.5, dtype=T.float64, device=dev)
        g = self.tracking_kalman_vjp(Zout, Lgain, H, V, Lb, None, lb, events, model, guarded_design)
        g["V"] = g["V"] + 0.5 * (iv * T.einsum("bkrs,bks->bkr", G, iv)).sum(dim=1) / (Vt * Vt)
        return g

    # -- the fixed-interval smoother: the estimator's backward pass ------------------------------------
    def _op_smoother(self, f, guarded, Ztraj, events, Lgain, Pest, H, V, Xhat, innov, model, with_states, with_cov):
        Hh, Vh = measurement_model(H, V)
        ny = Hh.shape[0]
        for name, t in (("Lgain", Lgain), ("Pest", Pest), ("Xhat", Xhat), ("innov", innov)):
            if t is None:
                raise ValueError(f"{name} is required: tracking_kalman{f.suffix}'s gains and covariances, the estimated roll-out's "
                                 "record")
        Ztraj = f.Z(Ztraj, "Ztraj")
        Lgain = f.arr(Lgain, self.B * self.N * n * ny, "Lgain")
        Pest = f.arr(Pest, self.B * self.N * _lib.TRACK_P_NNZ, "Pest")
        Xhat = f.arr(Xhat, self.B * self.N * n, "Xhat")
        innov = f.arr(innov, self.B * self.N * ny, "innov")
        Hd = f.H(Hh)
        Xs = f.empty((self.B, self.N, n), with_states)
        Ps = f.empty(tracking_p_shape(self.B, self.N), with_cov)
        extra = ()
        if guarded:
            events, model = f.events(events), f.model(model)
            extra = (f.ptr(model), f.ptr(events))
        _lib.check(f.fn("qln_landing_smoother" + ("_guarded" if guarded else ""))(
            self._h, f.ptr(Ztraj), *extra, f.ptr(Lgain), f.ptr(Pest), f.ptr(Hd), ny, Vh.ctypes.data, f.ptr(Xhat), f.ptr(innov),
            f.ptr(Xs), f.ptr(Ps)))
        return Xs, Ps

    def landing_smoother(self, Ztraj, Lgain, Pest, H, V, Xhat, innov, with_states=True, with_cov=True):
        """Fixed-interval smoothing of a flown landing: the state at every knot given all N measurements (the filter's Xhat_k
        uses those up to knot k).  The Bryson-Frazier sweep, backward over the record (Xhat, innov) of
        tracking_rollout_estimated, on the gains Lgain (B, N, 15, ny) and covariances Pest (B, N, 120) tracking_kalman
        returned for the same (Ztraj, H, V); it inverts nothing, so singular priors (a noiseless clock slot) are fine, and it
        does not check that Lgain and Pest belong together (qln_evaluator.h).  Device tensors in; returns (Xs (B, N, 15), Ps
        (B, N, 120) packed), device tensors, each None unless asked for; which is asked for does not change the other's
        bits.  At knot N-1, Xs = Xhat and Ps = Pest.  Stream-ordered."""
        return self._op_smoother(_DeviceForm(self), False, Ztraj, None, Lgain, Pest, H, V, Xhat, innov, None, with_states, with_cov)

    def landing_smoother_host(self, Ztraj, Lgain, Pest, H, V, Xhat, innov, with_states=True, with_cov=True):
        """The same with host arrays (synchronous): numpy (Xs, Ps)."""
        return self._op_smoother(_HostForm(self), False, Ztraj, None, Lgain, Pest, H, V, Xhat, innov, None, with_states, with_cov)

    def landing_smoother_guarded(self, Ztraj, events, Lgain, Pest, H, V, Xhat, innov, model=None, with_states=True,
                                 with_cov=True):
        """landing_smoother through the guarded touchdown, on the blocks of tracking_kalman_guarded at (Ztraj, events, model),
        at fixed touchdown knot: the touchdown knot's composite operator is applied transposed."""
        return self._op_smoother(_DeviceForm(self), True, Ztraj, events, Lgain, Pest, H, V, Xhat, innov, model, with_states,
                                 with_cov)

    def landing_smoother_guarded_host(self, Ztraj, events, Lgain, Pest, H, V, Xhat, innov, model=None, with_states=True,
                                      with_cov=True):
        """The same with host arrays (synchronous): numpy (Xs, Ps)."""
        return self._op_smoother(_HostForm(self), True, Ztraj, events, Lgain, Pest, H, V, Xhat, innov, model, with_states, with_cov)

    # -- the filter on recorded data, and the score of the data under it -------------------------------
    def _op_filter(self, f, guarded, Zref, Zrec, Lgain, H, Y, V, xhat0, with_estimate, with_innovations, with_score, with_events,
                   model=None):
        score = (V is not None) if with_score is None else with_score
        if score and V is None:
            raise ValueError("V is required with with_score: the measurement variances the gains were designed for")
        Hh, Vh = measurement_model(H, V) if score else (self._measurement_rows(H), None)
        ny = Hh.shape[0]
        for name, t in (("Lgain", Lgain), ("Y", Y)):
            if t is None:
                raise ValueError(f"{name} is required: tracking_kalman{f.suffix}'s gains, the recorded measurements"
                                 + f.MEASUREMENTS)
        Zref, Zrec = f.Z(Zref, "Zref"), f.Z(Zrec, "Zrec")
        Lgain = f.arr(Lgain, self.B * self.N * n * ny, "Lgain")
        Y = f.arr(Y, self.B * self.N * ny, "Y")
        xhat0 = f.x0(xhat0, "xhat0")
        Hd = f.H(Hh)
        Xh, iv = f.zeros((self.B, self.N, n), with_estimate), f.zeros((self.B, self.N, ny), with_innovations)
        sc, ll = f.zeros((self.B, self.N, 2), score), f.zeros((self.B,), score)
        # model None: the existing entries; a model of each record's own: the _model entries, model behind ny
        model = f.model(model)
        mp = () if model is None else (f.ptr(model),)
        sfx = "" if model is None else "_model"
        args = (self._h, f.ptr(Zref), f.ptr(Zrec), f.ptr(Lgain), f.ptr(Hd), ny, *mp, _host_ptr(Vh), f.ptr(Y), f.ptr(xhat0),
                f.ptr(Xh), f.ptr(iv), f.ptr(sc), f.ptr(ll))
        if not guarded:
            _lib.check(f.fn("qln_landing_filter" + sfx)(*args))
            return Xh, iv, sc, ll
        eh = f.zeros((self.B, _lib.TOUCHDOWN_INFO_STRIDE), with_events)
        _lib.check(f.fn("qln_landing_filter_guarded" + sfx)(*args, f.ptr(eh)))
        return Xh, iv, sc, ll, eh

    def landing_measurements(self, Zout, Zref, H, vnoise=None):
        """landing_measurements for this handle's layout: Zout and Zref as the handle's calls take and return them."""
        if vnoise is not None:
            vnoise = vnoise.reshape(self.B, self.N, -1)
        if hasattr(Zout, "detach"):
            zo, zr = (z.reshape(self.B, -1)[:, :self.n_nlp] for z in (Zout, Zref))
        else:
            zo, zr = (np.asarray(z).reshape(self.B, -1)[:, :self.n_nlp] for z in (Zout, Zref))
        return landing_measurements(zo, zr, H, vnoise)

    def landing_filter(self, Zref, Zrec, Lgain, H, Y, V=None, xhat0=None, with_estimate=True, with_innovations=True,
                       with_score=None, model=None):
        """The estimator of tracking_rollout_estimated run on a RECORD: measurements Y (B, N, ny) in the roll-out's form (the
        reading minus H x_ref,k: landing_measurements) and the forces that were applied, the control slots of Zrec -- its state
        slots are not read, and of Zref only the state slots are.  Lgain (B, N, 15, ny) are tracking_kalman's gains, xhat0
        (B, 15) the initial estimate (None: the reference's first knot); the prediction is the handle's model on the knot
        schedule.  With V (the variances the gains were designed for; with_score, default: V given) it also scores the record:
        score (B, N, 2) = {nis_k, log det S_k} and loglik (B,), the Gaussian log-likelihood, from the gains alone -- which the
        call cannot check belong to V (qln_evaluator.h).  Device tensors in; returns (Xhat, innov, score, loglik), each None
        unless asked for; which are asked for does not change the others' bits.  A replay of a flight returns its Xhat and
        innov.  model (B, 4) = {g, mb, mf, lb} per record sends the prediction to a model of each record's own
        (qln_landing_filter_model); None is the handle's, and the existing entry.  Stream-ordered."""
        return self._op_filter(_DeviceForm(self), False, Zref, Zrec, Lgain, H, Y, V, xhat0, with_estimate, with_innovations,
                               with_score, False, model)

    def landing_filter_host(self, Zref, Zrec, Lgain, H, Y, V=None, xhat0=None, with_estimate=True, with_innovations=True,
                            with_score=None, model=None):
        """The same with host arrays (synchronous): numpy (Xhat, innov, score, loglik).  A non-finite H is refused."""
        return self._op_filter(_HostForm(self), False, Zref, Zrec, Lgain, H, Y, V, xhat0, with_estimate, with_innovations,
                               with_score, False, model)

    def landing_filter_guarded(self, Zref, Zrec, Lgain, H, Y, V=None, xhat0=None, with_estimate=True, with_innovations=True,
                               with_score=None, with_events=True, model=None):
        """landing_filter with the estimator landing by its own guard, as in tracking_rollout_estimated(guarded=True): returns
        (Xhat, innov, score, loglik, events_hat), events_hat (B, 8) the estimator's touchdown records."""
        return self._op_filter(_DeviceForm(self), True, Zref, Zrec, Lgain, H, Y, V, xhat0, with_estimate, with_innovations,
                               with_score, with_events, model)

    def landing_filter_guarded_host(self, Zref, Zrec, Lgain, H, Y, V=None, xhat0=None, with_estimate=True,
                                    with_innovations=True, with_score=None, with_events=True, model=None):
        """The same with host arrays (synchronous): numpy (Xhat, innov, score, loglik, events_hat)."""
        return self._op_filter(_HostForm(self), True, Zref, Zrec, Lgain, H, Y, V, xhat0, with_estimate, with_innovations,
                               with_score, with_events, model)

    # -- the sweeps through the filter: tangents and cotangents of Xhat, innov, nis and loglik ----------
    FILTER_JVP_OUT = ("Xhat", "innov", "nis", "loglik", "event_hat")
    FILTER_VJP_OUT = ("Y", "Zrec", "Lgain", "xhat0", "model")

    def _op_filter_sweep(self, f, forward, guarded, Zref, Zrec, Lgain, H, Xhat, innov, V, model, events_hat, given, want):
        """One path for the four forms.  given: the tangents (forward) or cotangents by name, None for absent; want: the outputs
        by name.  Returns a dict of the outputs asked for.  The inputs are checked by the form's loose rule: a Z is not padded."""
        if guarded and events_hat is None:
            raise ValueError("events_hat is required: the record landing_filter_guarded returned")
        Hh, Vh = measurement_model(H, V) if V is not None else (self._measurement_rows(H), None)
        ny = Hh.shape[0]
        B, N = self.B, self.N
        sizes = dict(Xhat=B * N * n, innov=B * N * ny, nis=B * N, loglik=B, event_hat=B * _lib.TOUCHDOWN_INFO_STRIDE,
                     Y=B * N * ny, Zrec=self.dims.z_total, Lgain=B * N * n * ny, xhat0=B * n, model=B * _lib.MODEL_NP)
        shapes = dict(Xhat=(B, N, n), innov=(B, N, ny), nis=(B, N), loglik=(B,), event_hat=(B, _lib.TOUCHDOWN_INFO_STRIDE),
                      Y=(B, N, ny), Zrec=(self.dims.z_total,), Lgain=(B, N, n, ny), xhat0=(B, n), model=(B, _lib.MODEL_NP))
        outs = self.FILTER_JVP_OUT if forward else self.FILTER_VJP_OUT
        bad = set(want) - set(outs)
        if bad or (not guarded and "event_hat" in want):
            raise ValueError(f"want: unknown outputs {sorted(bad)} ({', '.join(outs)}; event_hat with guarded only)")
        Hd = f.H(Hh)
        for name, a in (("Zref", Zref), ("Zrec", Zrec), ("Lgain", Lgain), ("Xhat", Xhat)):
            if a is None:
                raise ValueError(f"{name} is required: the record and the trajectory landing_filter produced")
        keep = [f.loose(Zref, self.dims.z_total, "Zref"), f.loose(Zrec, self.dims.z_total, "Zrec"),
                f.loose(Lgain, sizes["Lgain"], "Lgain"), f.loose(model, sizes["model"], "model"),
                f.loose(Xhat, sizes["Xhat"], "Xhat"), f.loose(innov, sizes["innov"], "innov")]
        ev = f.loose(events_hat, sizes["event_hat"], "events_hat") if guarded else None
        gnames = ("Y", "Zrec", "Lgain", "xhat0", "model") if forward else ("Xhat", "innov", "nis", "loglik")
        gin = [f.loose(given.get(k), sizes[k], k + ("_dot" if forward else "_bar")) for k in gnames]
        res = {k: f.zeros(shapes[k]) for k in outs if k in want}
        args = [self._h, f.ptr(keep[0]), f.ptr(keep[1]), f.ptr(keep[2]), f.ptr(Hd), ny, f.ptr(keep[3]), _host_ptr(Vh),
                f.ptr(keep[4]), f.ptr(keep[5])]
        if guarded:
            args.append(f.ptr(ev))
        args += [f.ptr(g) for g in gin]
        args += [f.ptr(res.get(k)) for k in outs if guarded or k != "event_hat"]
        _lib.check(f.fn("qln_landing_filter" + ("_guarded" if guarded else "") + ("_jvp" if forward else "_vjp"))(*args))
        return res

    def _filter_jvp_want(self, want, V, Lgain_dot, guarded):
        if want is not None:
            return tuple(want)
        score = V is not None and Lgain_dot is None
        return ("Xhat", "innov") + (("nis", "loglik") if score else ()) + (("event_hat",) if guarded else ())

    def landing_filter_jvp(self, Zref, Zrec, Lgain, H, Xhat, innov=None, V=None, model=None, events_hat=None, guarded=False,
                           Y_dot=None, Zrec_dot=None, Lgain_dot=None, xhat0_dot=None, model_dot=None, want=None):
        """Forward sweep of landing_filter(model=...) at the record and the trajectory it produced (qln_landing_filter_jvp;
        guarded: through the estimator's own touchdown, at the knot and tau of events_hat).  Tangents (each optional, at least
        one): Y_dot (B, N, ny), Zrec_dot in the layout of Z (control slots read), Lgain_dot, xhat0_dot (B, 15), model_dot (B, 4).
        want: the outputs by name, of Xhat, innov, nis, loglik and (guarded) event_hat; default Xhat and innov, the score's
        two when V is given and Lgain_dot is not, and event_hat when guarded.  loglik's tangent is the exact derivative AT FIXED
        GAINS, so a score term together with Lgain_dot is refused; innov is needed with Lgain_dot or a score term.  The total
        derivative through the gains' design is landing_loglik_jvp.  Returns a dict of device tensors.  Stream-ordered."""
        given = dict(Y=Y_dot, Zrec=Zrec_dot, Lgain=Lgain_dot, xhat0=xhat0_dot, model=model_dot)
        return self._op_filter_sweep(_DeviceForm(self), True, guarded, Zref, Zrec, Lgain, H, Xhat, innov, V, model, events_hat,
                                     given, self._filter_jvp_want(want, V, Lgain_dot, guarded))

    def landing_filter_jvp_host(self, Zref, Zrec, Lgain, H, Xhat, innov=None, V=None, model=None, events_hat=None, guarded=False,
                                Y_dot=None, Zrec_dot=None, Lgain_dot=None, xhat0_dot=None, model_dot=None, want=None):
        """The same with host arrays (synchronous): a dict of numpy arrays."""
        given = dict(Y=Y_dot, Zrec=Zrec_dot, Lgain=Lgain_dot, xhat0=xhat0_dot, model=model_dot)
        return self._op_filter_sweep(_HostForm(self), True, guarded, Zref, Zrec, Lgain, H, Xhat, innov, V, model, events_hat, given,
                                     self._filter_jvp_want(want, V, Lgain_dot, guarded))

    def _filter_vjp_want(self, want, innov, nis_bar, loglik_bar):
        if want is not None:
            return tuple(want)
        gain = innov is not None and nis_bar is None and loglik_bar is None
        return ("Y", "Zrec") + (("Lgain",) if gain else ()) + ("xhat0", "model")

    def landing_filter_vjp(self, Zref, Zrec, Lgain, H, Xhat, innov=None, V=None, model=None, events_hat=None, guarded=False,
                           Xhat_bar=None, innov_bar=None, nis_bar=None, loglik_bar=None, want=None):
        """Reverse sweep, the exact transpose of landing_filter_jvp (qln_landing_filter_vjp).  Cotangents (each optional, at
        least one): Xhat_bar (B, N, 15), innov_bar (B, N, ny), nis_bar (B, N), loglik_bar (B,).  want: the outputs by name, of
        Y, Zrec (layout of Z: the controls' cotangents, exact zeros in the state slots), Lgain, xhat0 and model; default all
        that the call can give (Lgain only with innov and without a score cotangent: the score is differentiated at fixed
        gains).  With loglik_bar = 1 the outputs are the gradient of the log-likelihood.  Returns a dict of device tensors."""
        given = dict(Xhat=Xhat_bar, innov=innov_bar, nis=nis_bar, loglik=loglik_bar)
        return self._op_filter_sweep(_DeviceForm(self), False, guarded, Zref, Zrec, Lgain, H, Xhat, innov, V, model, events_hat,
                                     given, self._filter_vjp_want(want, innov, nis_bar, loglik_bar))

    def landing_filter_vjp_host(self, Zref, Zrec, Lgain, H, Xhat, innov=None, V=None, model=None, events_hat=None, guarded=False,
                                Xhat_bar=None, innov_bar=None, nis_bar=None, loglik_bar=None, want=None):
        """The same with host arrays (synchronous): a dict of numpy arrays."""
        given = dict(Xhat=Xhat_bar, innov=innov_bar, nis=nis_bar, loglik=loglik_bar)
        return self._op_filter_sweep(_HostForm(self), False, guarded, Zref, Zrec, Lgain, H, Xhat, innov, V, model, events_hat,
                                     given, self._filter_vjp_want(want, innov, nis_bar, loglik_bar))

    # -- the estimate-feedback roll-out: the plant and the estimator flown together -------------------
    @staticmethod
    def _measurement_rows(H):
        H = np.asarray(H.detach().cpu().numpy() if hasattr(H, "detach") else H, dtype=np.float64)
        if H.ndim == 1:
            H = H[None]
        if H.ndim != 2 or H.shape[1] != n or not 1 <= H.shape[0] <= _lib.TRACK_NY_MAX:
            raise ValueError(f"H of shape {H.shape}: expected (ny, 15) with 1 <= ny <= {_lib.TRACK_NY_MAX}")
        return np.ascontiguousarray(H)

    def _op_estimated(self, f, limited, Zref, limits, K, Lgain, H, vnoise, wnoise, x0, xhat0, model, guarded, out, with_estimate,
                      with_innovations, with_events, with_sat=True):
        """Returns (Zout, Xhat, innov), guarded also (events, events_hat), limited all of them and sat."""
        lim = force_limits(limits) if limited else None
        Hh = self._measurement_rows(H)
        ny = Hh.shape[0]
        Hd = f.H(Hh)
        Zref = f.Z(Zref, "Zref")
        out = f.out(out, (self.dims.z_total,), "out")
        K = f.K(K)
        if Lgain is None:
            raise ValueError(f"Lgain is required: the filter gains tracking_kalman{f.suffix} returned")
        Lgain = f.arr(Lgain, self.B * self.N * n * ny, "Lgain")
        vnoise = f.opt(vnoise, self.B * self.N * ny, "vnoise")
        wnoise = f.opt(wnoise, self.B * (self.N - 1) * n, "wnoise")
        x0, xhat0, model = f.x0(x0), f.x0(xhat0, "xhat0"), f.model(model)
        Xh = f.zeros((self.B, self.N, n), with_estimate)
        iv = f.zeros((self.B, self.N, ny), with_innovations)
        args = [self._h, f.ptr(Zref), f.ptr(K), f.ptr(Lgain), f.ptr(Hd), ny, f.ptr(vnoise), f.ptr(wnoise), f.ptr(x0), f.ptr(xhat0),
                f.ptr(model)]
        if limited:
            args += [lim.ctypes.data, int(bool(guarded))]
        args += [f.ptr(out), f.ptr(Xh), f.ptr(iv)]
        if not (guarded or limited):
            _lib.check(f.fn("qln_tracking_rollout_estimated")(*args))
            return out, Xh, iv
        ev = f.zeros((self.B, _lib.TOUCHDOWN_INFO_STRIDE), guarded and with_events)
        eh = f.zeros((self.B, _lib.TOUCHDOWN_INFO_STRIDE), guarded and with_events)
        if not limited:
            _lib.check(f.fn("qln_tracking_rollout_estimated_guarded")(*args, f.ptr(ev), f.ptr(eh)))
            return out, Xh, iv, ev, eh
        sat = f.zeros((self.B, self.N - 1), with_sat)
        _lib.check(f.fn("qln_tracking_rollout_estimated_limited")(*args, f.ptr(ev), f.ptr(eh), f.ptr(sat)))
        return out, Xh, iv, ev, eh, sat

    def tracking_rollout_estimated(self, Zref, K, Lgain, H, vnoise=None, wnoise=None, x0=None, xhat0=None, model=None,
                                   guarded=False, out=None, with_estimate=True, with_innovations=False, with_events=True):
        """The closed loop that feeds back an ESTIMATE, flown on the nonlinear hybrid plant: tracking_rollout_model (guarded
        False) or tracking_rollout_guarded (guarded True) with F_k = F_ref,k - K_k (xhat_k|k - x_ref,k), the estimate updated
        at every knot from y_k = H (x_k - x_ref,k) + v_k with the filter gains Lgain (B, N, 15, ny) of tracking_kalman and
        predicted with the handle's model; guarded, the estimator lands by its own estimated foot (qln_evaluator.h).  The
        noise is the caller's: vnoise (B, N, ny) and wnoise (B, N-1, 15) device tensors of samples, None for none; xhat0
        (B, 15), None: the reference's first knot.  Returns (Zout, Xhat, innov), and guarded also (events, events_hat), the
        plant's and the estimator's touchdown records: Xhat (B, N, 15), innov (B, N, ny), each None unless asked for."""
        return self._op_estimated(_DeviceForm(self), False, Zref, None, K, Lgain, H, vnoise, wnoise, x0, xhat0, model, guarded, out,
                                  with_estimate, with_innovations, with_events)

    def tracking_rollout_estimated_host(self, Zref, K, Lgain, H, vnoise=None, wnoise=None, x0=None, xhat0=None, model=None,
                                        guarded=False, with_estimate=True, with_innovations=False, with_events=True):
        """The same with host arrays (synchronous): numpy (Zout (z_total,), zeros past n_nlp, Xhat, innov) and guarded also
        (events, events_hat).  A non-finite H or model entry, or mb, mf or lb <= 0, is refused."""
        return self._op_estimated(_HostForm(self), False, Zref, None, K, Lgain, H, vnoise, wnoise, x0, xhat0, model, guarded, None,
                                  with_estimate, with_innovations, with_events)

    # -- forward and reverse sweeps through the estimate-feedback roll-out ----------------------------
    def _op_estimated_traj(self, f, limited, Zref, K, Lgain, H, Zout, Xhat, sat, innov, model, guarded, events, events_hat,
                           want_gain):
        """The arguments both sweeps share, checked: (guarded, ny, the C arguments up to innov / event_hat / sat, what must stay
        alive).  limited: the sweeps at fixed active set, where both records or neither select the blocks, then sat."""
        if limited:
            if (events is None) != (events_hat is None):
                raise ValueError("events and events_hat: both (the guarded blocks) or neither (the knot-scheduled ones)")
            guarded = events is not None
        Hh = self._measurement_rows(H)
        ny = Hh.shape[0]
        Hd = f.H(Hh)
        Zref, K = f.Z(Zref, "Zref"), f.K(K)
        if Lgain is None or Xhat is None:
            raise ValueError(f.TRAJ)
        Lgain = f.arr(Lgain, self.B * self.N * n * ny, "Lgain")
        model = f.model(model)
        Zout = f.Z(Zout, "Zout")
        Xhat = f.arr(Xhat, self.B * self.N * n, "Xhat")
        if want_gain and innov is None:
            raise ValueError(f.INNOV)
        innov = f.opt(innov if want_gain else None, self.B * self.N * ny, "innov")
        keep = [Zref, K, Lgain, Hd, model, Zout, Xhat, innov]
        if guarded:
            if events is None or events_hat is None:
                raise ValueError(f.RECORDS)
            keep += [f.events(events), f.events_hat(events_hat)]
        elif limited:
            keep += [None, None]
        if limited:
            keep.append(f.sat(sat))
        args = [self._h] + [f.ptr(a) for a in keep]
        args.insert(5, ny)
        return guarded, ny, args, keep

    def _op_estimated_jvp(self, f, limited, Zref, K, Lgain, H, Zout, Xhat, sat, innov, model, guarded, events, events_hat,
                          Zref_dot, K_dot, Lgain_dot, x0_dot, xhat0_dot, model_dot, out, with_estimate, with_innovations,
                          with_event_dot):
        guarded, ny, args, keep = self._op_estimated_traj(f, limited, Zref, K, Lgain, H, Zout, Xhat, sat, innov, model, guarded,
                                                          events, events_hat, Lgain_dot is not None)
        keep += [f.Z_opt(Zref_dot, "Zref_dot"), f.K(K_dot, "K_dot"), f.opt(Lgain_dot, self.B * self.N * n * ny, "Lgain_dot"),
                 f.x0(x0_dot, "x0_dot"), f.x0(xhat0_dot, "xhat0_dot"), f.model(model_dot, "model_dot")]
        out = f.out(out, (self.dims.z_total,), "out")
        Xd, ivd = f.zeros((self.B, self.N, n), with_estimate), f.zeros((self.B, self.N, ny), with_innovations)
        args += [f.ptr(a) for a in keep[-6:]] + [f.ptr(out), f.ptr(Xd), f.ptr(ivd)]
        if not (guarded or limited):
            _lib.check(f.fn("qln_tracking_rollout_estimated_jvp")(*args))
            return out, Xd, ivd
        ed = f.zeros((self.B, _lib.TOUCHDOWN_INFO_STRIDE), guarded and with_event_dot)
        ehd = f.zeros((self.B, _lib.TOUCHDOWN_INFO_STRIDE), guarded and with_event_dot)
        _lib.check(f.fn("qln_tracking_rollout_estimated" + ("_limited" if limited else "_guarded") + "_jvp")(
            *args, f.ptr(ed), f.ptr(ehd)))
        return out, Xd, ivd, ed, ehd

    ESTIMATED_VJP_OUTPUTS = ("Zref", "K", "Lgain", "x0", "xhat0", "model")

    def _op_estimated_vjp(self, f, limited, Zref, K, Lgain, H, Zout, Xhat, sat, Zbar, innov, model, guarded, events, events_hat,
                          Xhat_bar, innov_bar, want):
        default = want is None
        want = self._vjp_want(K, want, self.ESTIMATED_VJP_OUTPUTS)
        if default and innov is None:
            want = tuple(w for w in want if w != "Lgain")
        guarded, ny, args, keep = self._op_estimated_traj(f, limited, Zref, K, Lgain, H, Zout, Xhat, sat, innov, model, guarded,
                                                          events, events_hat, "Lgain" in want)
        keep += [f.Z(Zbar, "Zbar"), f.opt(Xhat_bar, self.B * self.N * n, "Xhat_bar"),
                 f.opt(innov_bar, self.B * self.N * ny, "innov_bar")]
        shapes = ((self.dims.z_total,), tracking_k_shape(self.B, self.N), (self.B, self.N, n, ny), (self.B, n), (self.B, n),
                  (self.B, _lib.MODEL_NP))
        outs = tuple(f.zeros(shape, name in want) for name, shape in zip(self.ESTIMATED_VJP_OUTPUTS, shapes))
        kind = "_limited" if limited else "_guarded" if guarded else ""
        _lib.check(f.fn("qln_tracking_rollout_estimated" + kind + "_vjp")(*args, *(f.ptr(a) for a in keep[-3:]),
                                                                        *(f.ptr(o) for o in outs)))
        return outs

    def tracking_rollout_estimated_jvp(self, Zref, K, Lgain, H, Zout, Xhat, innov=None, model=None, guarded=False, events=None,
                                       events_hat=None, Zref_dot=None, K_dot=None, Lgain_dot=None, x0_dot=None, xhat0_dot=None,
                                       model_dot=None, out=None, with_estimate=True, with_innovations=True, with_event_dot=True):
        """Forward sweep of tracking_rollout_estimated at the trajectory (Zout, Xhat, innov[, events, events_hat]) it returned,
        at fixed noise samples and fixed H: tangents of Zref, K, Lgain, x0, xhat0 and model, each None for zero -- except
        xhat0_dot, whose None is the forward call's xhat0 = None (the estimate starts on the reference, so its tangent is
        Zref_dot's first knot).  innov is needed only with Lgain_dot.  Returns (Zout_dot, Xhat_dot, innov_dot), and guarded
        also (event_dot, event_hat_dot), each optional one None unless asked for (qln_evaluator.h)."""
        return self._op_estimated_jvp(_DeviceForm(self), False, Zref, K, Lgain, H, Zout, Xhat, None, innov, model, guarded, events,
                                      events_hat, Zref_dot, K_dot, Lgain_dot, x0_dot, xhat0_dot, model_dot, out, with_estimate,
                                      with_innovations, with_event_dot)

    def tracking_rollout_estimated_vjp(self, Zref, K, Lgain, H, Zout, Xhat, Zbar, innov=None, model=None, guarded=False,
                                       events=None, events_hat=None, Xhat_bar=None, innov_bar=None, want=None):
        """Reverse sweep of tracking_rollout_estimated, the exact adjoint of tracking_rollout_estimated_jvp: cotangents Zbar
        (layout of Z), Xhat_bar (B, N, 15) and innov_bar (B, N, ny), the last two None for zero.  Returns (Zref_bar, K_bar,
        Lgain_bar, x0_bar, xhat0_bar, model_bar), each None unless named in want (default: all, K_bar only when K is given,
        Lgain_bar only when innov is).  Without "xhat0" in want the cotangent of the initial estimate is added to Zref_bar's
        first knot: the forward call's xhat0 = None."""
        return self._op_estimated_vjp(_DeviceForm(self), False, Zref, K, Lgain, H, Zout, Xhat, None, Zbar, innov, model, guarded,
                                      events, events_hat, Xhat_bar, innov_bar, want)

    def tracking_rollout_estimated_jvp_host(self, Zref, K, Lgain, H, Zout, Xhat, innov=None, model=None, guarded=False,
                                            events=None, events_hat=None, Zref_dot=None, K_dot=None, Lgain_dot=None, x0_dot=None,
                                            xhat0_dot=None, model_dot=None, with_estimate=True, with_innovations=True,
                                            with_event_dot=True):
        """The same with host arrays (synchronous): numpy (Zout_dot (z_total,), Xhat_dot, innov_dot) and guarded also
        (event_dot, event_hat_dot).  A non-finite H, a model or an event record that the guarded sweeps' host forms refuse,
        is refused."""
        return self._op_estimated_jvp(_HostForm(self), False, Zref, K, Lgain, H, Zout, Xhat, None, innov, model, guarded, events,
                                      events_hat, Zref_dot, K_dot, Lgain_dot, x0_dot, xhat0_dot, model_dot, None, with_estimate,
                                      with_innovations, with_event_dot)

    def tracking_rollout_estimated_vjp_host(self, Zref, K, Lgain, H, Zout, Xhat, Zbar, innov=None, model=None, guarded=False,
                                            events=None, events_hat=None, Xhat_bar=None, innov_bar=None, want=None):
        """The same with host arrays (synchronous): numpy (Zref_bar, K_bar, Lgain_bar, x0_bar, xhat0_bar, model_bar)."""
        return self._op_estimated_vjp(_HostForm(self), False, Zref, K, Lgain, H, Zout, Xhat, None, Zbar, innov, model, guarded,
                                      events, events_hat, Xhat_bar, innov_bar, want)

    # -- contact-aware force limits: the roll-out, its sweeps and the gains at fixed active set ------
    def tracking_rollout_limited(self, Zref, limits, K=None, x0=None, model=None, guarded=False, out=None, with_events=True,
                                 with_sat=True):
        """tracking_rollout_model (guarded False: the handle's knot schedule) or tracking_rollout_guarded (guarded True) with
        the applied forces clamped to `limits`, eight numbers {free_x_lo, free_x_hi, free_y_lo, free_y_hi, stand_x_lo,
        stand_x_hi, stand_y_lo, stand_y_hi} (force_limits; +-inf: no limit): a foot takes the standing pair where it stands at
        the knot's start and the free pair otherwise.  Returns (Zout, events, sat): events as tracking_rollout_guarded (None
        when not guarded or without with_events), sat a (B, N-1) float64 device tensor of saturation codes sum_m s_m 4^m with
        s_m = 1 at the lower and 2 at the upper limit (unpack_saturation; None without with_sat).  The derivatives at this
        active set are tracking_rollout_limited_jvp / _vjp and the gains tracking_lqr_limited's, which take sat
        (qln_evaluator.h)."""
        return self._op_rollout(_DeviceForm(self), "_limited", Zref, K, x0, model, out, limits, guarded, with_events, with_sat)

    def tracking_rollout_limited_host(self, Zref, limits, K=None, x0=None, model=None, guarded=False, with_events=True,
                                      with_sat=True):
        """The same with host arrays (synchronous): numpy (Zout (z_total,), events (B, 8) or None, sat (B, N-1) or None)."""
        return self._op_rollout(_HostForm(self), "_limited", Zref, K, x0, model, None, limits, guarded, with_events, with_sat)

    def tracking_rollout_limited_jvp(self, Zref, Zout, sat, events=None, K=None, model=None, Zref_dot=None, K_dot=None,
                                     x0_dot=None, model_dot=None, out=None, with_event_dot=True):
        """Forward sweep of tracking_rollout_limited at the (Zout, events, sat) it returned, at fixed active set and fixed
        touchdown knot: the tangent of a force that rode a limit is zero.  events None: the knot-scheduled blocks
        (tracking_rollout_model_jvp's), else the guarded ones.  Returns (Zout_dot, event_dot), event_dot None without events
        or with_event_dot."""
        return self._op_rollout_jvp(_DeviceForm(self), "_limited", Zref, Zout, K, model, Zref_dot, K_dot, x0_dot, model_dot, out,
                                    events, sat, with_event_dot)

    def tracking_rollout_limited_jvp_host(self, Zref, Zout, sat, events=None, K=None, model=None, Zref_dot=None, K_dot=None,
                                          x0_dot=None, model_dot=None, with_event_dot=True):
        """The same with host arrays (synchronous): numpy (Zout_dot (z_total,), event_dot (B, 8) or None).  A sat entry that is
        not a saturation code is refused."""
        return self._op_rollout_jvp(_HostForm(self), "_limited", Zref, Zout, K, model, Zref_dot, K_dot, x0_dot, model_dot, None,
                                    events, sat, with_event_dot)

    def tracking_rollout_limited_vjp(self, Zref, Zout, sat, Zbar, events=None, K=None, model=None, want=None):
        """Reverse sweep of tracking_rollout_limited at the (Zout, events, sat) it returned, the exact adjoint of
        tracking_rollout_limited_jvp: the rows of K_bar and the force entries of Zref_bar of a channel that rode a limit are
        exact zeros.  Returns (Zref_bar, K_bar, x0_bar, model_bar), each None unless named in want (default: all, K_bar only
        when K is given)."""
        return self._op_rollout_vjp(_DeviceForm(self), "_limited", Zref, Zout, Zbar, K, model, want, events, sat)

    def tracking_rollout_limited_vjp_host(self, Zref, Zout, sat, Zbar, events=None, K=None, model=None, want=None):
        """The same with host arrays (synchronous): numpy (Zref_bar, K_bar, x0_bar, model_bar (B, 4))."""
        return self._op_rollout_vjp(_HostForm(self), "_limited", Zref, Zout, Zbar, K, model, want, events, sat)

    def tracking_lqr_limited(self, Ztraj, sat, Q, R, Qf, events=None, model=None, K=None, P=None, with_cost_to_go=True):
        """tracking_lqr (events None; model must then be None) or tracking_lqr_guarded (events given) at the active set of a
        limited roll-out: the columns of B_k of the channels that rode a limit at knot k (sat) are zero, so their rows of K_k
        are exact zeros and P is the cost-to-go of feedback on the free channels only.  Returns (K, P) as tracking_lqr."""
        return self._op_lqr(_DeviceForm(self), "_limited", Ztraj, Q, R, Qf, events=events, sat=sat, model=model, K=K, P=P,
                            with_cost_to_go=with_cost_to_go)

    def tracking_lqr_limited_host(self, Ztraj, sat, Q, R, Qf, events=None, model=None, with_cost_to_go=True):
        """The same with host arrays (synchronous): returns numpy (K, P)."""
        return self._op_lqr(_HostForm(self), "_limited", Ztraj, Q, R, Qf, events=events, sat=sat, model=model,
                            with_cost_to_go=with_cost_to_go)

    # -- contact-aware force limits in the estimate-feedback roll-out and its sweeps -------------------
    def tracking_rollout_estimated_limited(self, Zref, limits, K, Lgain, H, vnoise=None, wnoise=None, x0=None, xhat0=None,
                                           model=None, guarded=False, out=None, with_estimate=True, with_innovations=False,
                                           with_events=True, with_sat=True):
        """tracking_rollout_estimated with the forces fed back from the estimate clamped to `limits` (force_limits) before
        anything reads them: Zout's controls, the plant's guard and step, the estimator's guard and step.  A foot takes the
        standing pair where the PLANT's foot stands at the knot's start -- by the handle's knot schedule, or guarded by the
        plant's own contact mode -- whatever the estimator believes (qln_evaluator.h).  Returns (Zout, Xhat, innov, events,
        events_hat, sat): events and events_hat None when not guarded or without with_events, sat the (B, N-1) saturation
        record of tracking_rollout_limited (None without with_sat), which the sweeps at this active set take."""
        return self._op_estimated(_DeviceForm(self), True, Zref, limits, K, Lgain, H, vnoise, wnoise, x0, xhat0, model, guarded,
                                  out, with_estimate, with_innovations, with_events, with_sat)

    def tracking_rollout_estimated_limited_host(self, Zref, limits, K, Lgain, H, vnoise=None, wnoise=None, x0=None, xhat0=None,
                                                model=None, guarded=False, with_estimate=True, with_innovations=False,
                                                with_events=True, with_sat=True):
        """The same with host arrays (synchronous): numpy (Zout (z_total,), Xhat, innov, events, events_hat, sat)."""
        return self._op_estimated(_HostForm(self), True, Zref, limits, K, Lgain, H, vnoise, wnoise, x0, xhat0, model, guarded, None,
                                  with_estimate, with_innovations, with_events, with_sat)

    def tracking_rollout_estimated_limited_jvp(self, Zref, K, Lgain, H, Zout, Xhat, sat, innov=None, model=None, events=None,
                                               events_hat=None, Zref_dot=None, K_dot=None, Lgain_dot=None, x0_dot=None,
                                               xhat0_dot=None, model_dot=None, out=None, with_estimate=True,
                                               with_innovations=True, with_event_dot=True):
        """Forward sweep of tracking_rollout_estimated_limited at the trajectory and the sat it returned, at fixed active set:
        tracking_rollout_estimated_jvp with the tangent of every force that rode a limit zero, for everything that reads it.
        events and events_hat both None: the knot-scheduled blocks, both given: the guarded ones.  Returns (Zout_dot, Xhat_dot,
        innov_dot, event_dot, event_hat_dot), the last two None without records or with_event_dot."""
        return self._op_estimated_jvp(_DeviceForm(self), True, Zref, K, Lgain, H, Zout, Xhat, sat, innov, model, False, events,
                                      events_hat, Zref_dot, K_dot, Lgain_dot, x0_dot, xhat0_dot, model_dot, out, with_estimate,
                                      with_innovations, with_event_dot)

    def tracking_rollout_estimated_limited_vjp(self, Zref, K, Lgain, H, Zout, Xhat, sat, Zbar, innov=None, model=None, events=None,
                                               events_hat=None, Xhat_bar=None, innov_bar=None, want=None):
        """Reverse sweep of tracking_rollout_estimated_limited, the exact adjoint of tracking_rollout_estimated_limited_jvp: the
        rows of K_bar and the force entries of Zref_bar of a channel that rode a limit are exact zeros.  Arguments and returns
        as tracking_rollout_estimated_vjp, with sat and with the records selecting the blocks."""
        return self._op_estimated_vjp(_DeviceForm(self), True, Zref, K, Lgain, H, Zout, Xhat, sat, Zbar, innov, model, False,
                                      events, events_hat, Xhat_bar, innov_bar, want)

    def tracking_rollout_estimated_limited_jvp_host(self, Zref, K, Lgain, H, Zout, Xhat, sat, innov=None, model=None, events=None,
                                                    events_hat=None, Zref_dot=None, K_dot=None, Lgain_dot=None, x0_dot=None,
                                                    xhat0_dot=None, model_dot=None, with_estimate=True, with_innovations=True,
                                                    with_event_dot=True):
        """The same with host arrays (synchronous): numpy (Zout_dot (z_total,), Xhat_dot, innov_dot, event_dot, event_hat_dot).
        A sat entry that is not a saturation code is refused."""
        return self._op_estimated_jvp(_HostForm(self), True, Zref, K, Lgain, H, Zout, Xhat, sat, innov, model, False, events,
                                      events_hat, Zref_dot, K_dot, Lgain_dot, x0_dot, xhat0_dot, model_dot, None, with_estimate,
                                      with_innovations, with_event_dot)

    def tracking_rollout_estimated_limited_vjp_host(self, Zref, K, Lgain, H, Zout, Xhat, sat, Zbar, innov=None, model=None,
                                                    events=None, events_hat=None, Xhat_bar=None, innov_bar=None, want=None):
        """The same with host arrays (synchronous): numpy (Zref_bar, K_bar, Lgain_bar, x0_bar, xhat0_bar, model_bar)."""
        return self._op_estimated_vjp(_HostForm(self), True, Zref, K, Lgain, H, Zout, Xhat, sat, Zbar, innov, model, False, events,
                                      events_hat, Xhat_bar, innov_bar, want)

    def differentiable_rollout(self, Zref, K=None, x0=None, model=None, guarded=False, limits=None):
        """tracking_rollout as a torch autograd op: returns Zout, differentiable in Zref, K and x0 (each a float64 CUDA
        tensor or None).  The backward pass is one qln_tracking_rollout_vjp launch at the Zout the forward produced, a
        forward-mode tangent (torch.autograd.forward_ad, torch.func.jvp) one qln_tracking_rollout_jvp launch.
        With model, a (B, 4) tensor of per-problem plant models (plant_models), it is tracking_rollout_model, differentiable
        in model too, through the _model_ forms of the two sweeps.
        With guarded it is tracking_rollout_guarded and returns (Zout, events): Zout is differentiable in Zref, K, x0 and
        model (None: the handle's, no gradient) through the sweeps through the touchdown, at fixed touchdown knot; events,
        the (B, 8) record, is not differentiable.
        With limits (eight numbers, force_limits) it is tracking_rollout_limited, with or without guarded, and returns
        (Zout, sat) or (Zout, events, sat): Zout is differentiable in the same four inputs through the sweeps at fixed
        active set; sat, the (B, N-1) saturation record, is not differentiable."""
        from .rollout_grad import GuardedRolloutFunction, LimitedRolloutFunction, ModelRolloutFunction, RolloutFunction

        if limits is not None:
            return LimitedRolloutFunction.apply(self, Zref, K, x0, model, force_limits(limits), bool(guarded))
        if guarded:
            return GuardedRolloutFunction.apply(self, Zref, K, x0, model)
        if model is None:
            return RolloutFunction.apply(self, Zref, K, x0)
        return ModelRolloutFunction.apply(self, Zref, K, x0, model)

    def differentiable_landing_filter(self, Zref, Lgain, H, Vdiag=None, guarded=False):
        """The filter on recorded data as a torch autograd op: returns f with f(Y, Zrec, xhat0=None, model=None) ->
        (Xhat, innov) or, with Vdiag, (Xhat, innov, loglik); guarded, the estimator's event record follows, non-differentiable.
        Reverse mode is landing_filter_vjp and forward mode (torch.autograd.forward_ad) landing_filter_jvp, bit for bit, at the
        trajectory the forward produced.  Y, Zrec (its control slots), xhat0 and model are differentiable; Lgain -- pass a tensor
        that requires grad -- only when Vdiag is None, that is without the loglik output: the likelihood is differentiated AT
        FIXED GAINS (log det S_k depends on the gains; qln_evaluator.h), and with Vdiag a gradient or tangent of Lgain raises."""
        from .rollout_grad import LandingFilterFunction

        def f(Y, Zrec, xhat0=None, model=None):
            return LandingFilterFunction.apply(self, Y, Zrec, xhat0, model, Lgain, Zref, H, Vdiag, bool(guarded))

        return f

    def differentiable_estimated_rollout(self, Zref, K, Lgain, H, vnoise=None, wnoise=None, x0=None, xhat0=None, model=None,
                                         guarded=False, limits=None):
        """tracking_rollout_estimated as a torch autograd op: returns (Zout, Xhat, innov), and guarded also (events,
        events_hat).  Zout, Xhat and innov are differentiable in Zref, K, Lgain, x0, xhat0 and model (each a float64 CUDA
        tensor; K, x0, xhat0 and model may be None) at FIXED noise samples: the backward pass is one
        qln_tracking_rollout_estimated_vjp launch at the trajectory the forward produced, a forward-mode tangent
        (torch.autograd.forward_ad, torch.func.jvp) one qln_tracking_rollout_estimated_jvp launch; guarded, both go through
        the plant's and the estimator's touchdowns at fixed knots.  H, vnoise, wnoise and the event records are not
        differentiable.  With xhat0 None the estimate starts on Zref's first knot and Zref carries its gradient.
        With limits (eight numbers, force_limits) it is tracking_rollout_estimated_limited and returns sat, the (B, N-1)
        saturation record, as one more, last output, not differentiable; both autograd modes then run the sweeps at that
        active set (tracking_rollout_estimated_limited_vjp / _jvp)."""
        from .rollout_grad import EstimatedLimitedRolloutFunction, EstimatedRolloutFunction

        if limits is not None:
            return EstimatedLimitedRolloutFunction.apply(self, Zref, K, Lgain, x0, xhat0, model, H, vnoise, wnoise,
                                                         force_limits(limits), bool(guarded))
        return EstimatedRolloutFunction.apply(self, Zref, K, Lgain, x0, xhat0, model, H, vnoise, wnoise, bool(guarded))

    def split_hvals(self, hvals):
        """(h_total,) values -> (step blocks (B, N-1, 55), terminal diagonals (B, 15)) as numpy arrays."""
        h = hvals.detach().cpu().numpy() if hasattr(hvals, "detach") else np.asarray(hvals)
        h = h.reshape(-1)
        seg = np.stack([h[b * self.h_stride: b * self.h_stride + self.h_nnz] for b in range(self.B)])
        steps = seg[:, : _lib.HESS_STEP_NNZ * (self.N - 1)].reshape(self.B, self.N - 1, _lib.HESS_STEP_NNZ)
        return steps, seg[:, _lib.HESS_STEP_NNZ * (self.N - 1):]

    def gauss_newton_step(self, Z, c, out=None, max_iters: int = 200, rel_tol: float = 1e-10, radius=None,
                          col_scale=None, info=None):
        """dZ = D x, x the minimum-norm least-squares step on the constraint violation of every problem (CGLS in LDS,
        one wave per problem); `c` = eval_c(Z).  Optional device tensors: `radius` (B,) trust radius on |x|,
        `col_scale` (n_nlp,) diagonal of D (0 = variable held fixed), `info` (B, 8): {iterations, |(AD)'rho|^2,
        |(AD)'(A dZ + rho)|^2, |A dZ + rho|^2, |rho|^2, cut at the radius, |x|, 0}."""
        self._check(Z, self.dims.z_total, "Z")
        self._check(c, self.dims.c_total, "c")
        out = self.new_Z() if out is None else out
        self._check(out, self.dims.z_total, "out")
        ptr = lambda t, total, name: None if t is None else self._check(t, total, name)
        _lib.check(_lib.lib().qln_gauss_newton_step(self._h, Z.data_ptr(), c.data_ptr(), out.data_ptr(), int(max_iters),
                                                    float(rel_tol), ptr(radius, self.B, "radius"),
                                                    ptr(col_scale, self.n_nlp, "col_scale"),
                                                    ptr(info, _lib.GN_INFO_STRIDE * self.B, "info")))
        return out

    def _bound_options(self, bounds):
        """qln_solve_options at their defaults with the given bound fields set (h_min, h_max, theta_min, theta_max, q6_bounds)."""
        opt = _lib.QlnSolveOptions()
        _lib.check(_lib.lib().qln_solve_default_options(C.byref(opt)))
        for k, v in bounds.items():
            if k not in ("h_min", "h_max", "theta_min", "theta_max", "q6_bounds"):
                raise TypeError(f"unknown bound option {k!r}")
            setattr(opt, k, v)
        return opt

    def estimate_multipliers(self, Z, c=None, g=None, *, act_tol: float = 1e-6, bound_tol: float = 1e-8, row_scaling: bool = True,
                             max_iters: int = 20000, rel_tol: float = 1e-8, lam=None, lag=None, info=None, **bounds):
        """Least-squares Lagrange multipliers of every problem at Z and the KKT residual (qln_estimate_multipliers; CGLS in
        LDS, one wave per problem).  `c` = eval_c(Z) and `g` = grad_f(Z) when not given (a caller may pass another
        gradient, e.g. the exact one: by quirk Q2 grad_f has no d(h l)/dh).  Convention L = f + lam'c.  `bounds`: h_min,
        h_max, theta_min, theta_max, q6_bounds of qln_solve_options.  Returns (lam, lag, info): lam in the layout of c (0
        on inactive clearance rows), lag = g + A'lam in the layout of Z (dual infeasibility on the free columns, z_L - z_U
        on the fixed ones), info a (B, 16) tensor {iterations, |Dg|^2, gamma, |r|^2, max |lag| free, active clearance rows,
        fixed variables, wrong-sign clearance multipliers, wrong-sign bound multipliers, max |lam_i c_i|, max |lam|,
        max |g| free, 0...}.  `lag=False` / `info=False`: not computed (None is returned in its place)."""
        t = _torch()
        self._check(Z, self.dims.z_total, "Z")
        c = self.eval_c(Z) if c is None else c
        g = self.grad_f(Z) if g is None else g
        lam = self.new_c() if lam is None else lam
        lag = self.new_Z() if lag is None else lag
        if info is None:
            info = t.zeros(self.B * _lib.MULT_INFO_STRIDE, dtype=t.float64, device=self._dev())
        ptr = lambda a, total, name: None if a is False else self._check(a, total, name)
        opt = self._bound_options(bounds)
        _lib.check(_lib.lib().qln_estimate_multipliers(
            self._h, Z.data_ptr(), self._check(c, self.dims.c_total, "c"), self._check(g, self.dims.z_total, "g"), C.byref(opt),
            float(act_tol), float(bound_tol), int(bool(row_scaling)), int(max_iters), float(rel_tol),
            self._check(lam, self.dims.c_total, "lam"), ptr(lag, self.dims.z_total, "lag"),
            ptr(info, self.B * _lib.MULT_INFO_STRIDE, "info")))
        return (lam, None if lag is False else lag,
                None if info is False else info.view(-1)[: self.B * _lib.MULT_INFO_STRIDE].view(self.B, _lib.MULT_INFO_STRIDE))

    def solve(self, Z, info=None, **options):
        """Batched solve of the reference NLP (solve(), src/moi.jl:46-103) on the GPU, in place on `Z` (device tensor,
        layout of Z; the controls of the guess are used, the states are rolled out from x0).  `options`: fields of
        qln_solve_options (max_outer, max_inner, tol_violation, rho0, ..., q6_bounds, exact_h_gradient).
        Returns (Z, info) with info a (B, 16) tensor: outer iterations, iLQR iterations, f, violation, rho, status, ..."""
        t = _torch()
        self._check(Z, self.dims.z_total, "Z")
        if info is None:
            info = t.zeros(self.B * _lib.SOLVE_INFO_STRIDE, dtype=t.float64, device=self._dev())
        self._check(info, self.B * _lib.SOLVE_INFO_STRIDE, "info")
        opt = _lib.QlnSolveOptions()
        _lib.check(_lib.lib().qln_solve_default_options(C.byref(opt)))
        for k, v in options.items():
            if not hasattr(opt, k):
                raise TypeError(f"unknown solve option {k!r}")
            setattr(opt, k, v)
        _lib.check(_lib.lib().qln_solve(self._h, Z.data_ptr(), C.byref(opt), info.data_ptr()))
        return Z, info.view(self.B, _lib.SOLVE_INFO_STRIDE)

    def kinematic_constraint(self, Z, with_jacobian: bool = True):
        """OPT-IN, nothing in the reference to compare with: the leg-length rows the reference has only as commented-out code
        (src/constraints.jl:115-138).  Returns (d (B, 2N), jac (B, 2N, 4) or None, (lower, upper))."""
        t = _torch()
        self._check(Z, self.dims.z_total, "Z")
        d = t.empty(self.B * 2 * self.N, dtype=t.float64, device=self._dev())
        jac = t.empty(self.B * 8 * self.N, dtype=t.float64, device=self._dev()) if with_jacobian else None
        _lib.check(_lib.lib().qln_eval_kinematic_constraint(self._h, Z.data_ptr(), d.data_ptr(),
                                                            jac.data_ptr() if jac is not None else None))
        lo, up = C.c_double(), C.c_double()
        _lib.check(_lib.lib().qln_kinematic_bounds(self._h, C.byref(lo), C.byref(up)))
        return d.view(self.B, 2 * self.N), (jac.view(self.B, 2 * self.N, 4) if jac is not None else None), (lo.value, up.value)

    def friction_cone(self, Z, mu: float, with_jacobian: bool = True):
        """OPT-IN, nothing in the reference to compare with (it has no friction constraint): the friction pyramid
        |F_x| <= mu F_y of the feet that stand on the ground at each dynamics knot, two linear rows per foot, bounds
        0 <= d < inf.  Returns (d (B, N-1, 4), jac (B, N-1, 4, 2) or None); see qln_eval_friction_cone."""
        t = _torch()
        self._check(Z, self.dims.z_total, "Z")
        n = self.B * (self.N - 1)
        d = t.empty(4 * n, dtype=t.float64, device=self._dev())
        jac = t.empty(8 * n, dtype=t.float64, device=self._dev()) if with_jacobian else None
        _lib.check(_lib.lib().qln_eval_friction_cone(self._h, Z.data_ptr(), float(mu), d.data_ptr(),
                                                     jac.data_ptr() if jac is not None else None))
        return d.view(self.B, self.N - 1, 4), (jac.view(self.B, self.N - 1, 4, 2) if jac is not None else None)

    def constraint_violation(self, c, out=None):
        """Per-problem constraint violation as Ipopt reports it (src/main.ipynb:712) -> (B,) tensor."""
        out = self.new_f() if out is None else out
        _lib.check(_lib.lib().qln_constraint_violation(self._h, self._check(c, self.dims.c_total, "c"),
                                                       self._check(out, self.B, "viol")))
        return out

    def initial_guess(self, out=None):
        """Z0 of the notebook's initial-guess rule (src/main.ipynb:181-198) for every problem, on the device."""
        out = self.new_Z() if out is None else out
        _lib.check(_lib.lib().qln_initial_guess(self._h, self._check(out, self.dims.z_total, "Z")))
        return out

    def sample_drop_states(self, sampler):
        """Redraw x0 of every problem on the device (qln_sample_drop_states; `sampler` from
        problem_gen.drop_state_sampler): bit-identical to problem_gen.make_batch's host draws.  Updates self.x0."""
        _lib.check(_lib.lib().qln_sample_drop_states(self._h, C.byref(sampler)))
        self.x0, _ = self.boundary_states()
        return self.x0

    def perturb_point(self, Z, sampler, sigma: float = 0.05, h_min: float = 0.001, h_max: float = 0.02, redraw_h: bool = False):
        """Z += N(0, sigma^2), h clipped (or redrawn uniformly): the evaluation point of SURVEY.md 8d, on the device."""
        _lib.check(_lib.lib().qln_perturb_point(self._h, C.byref(sampler), self._check(Z, self.dims.z_total, "Z"), float(sigma),
                                                float(h_min), float(h_max), int(redraw_h)))
        return Z

    def boundary_states(self):
        """(x0, xf) as the handle holds them now, (B, 15) each."""
        x0, xf = np.zeros((self.B, n)), np.zeros((self.B, n))
        _lib.check(_lib.lib().qln_get_boundary_states(self._h, x0.ctypes.data, xf.ctypes.data))
        return x0, xf

    def set_lqr_cost(self, Q, R, Qf, dt: float, per_problem: bool = False):
        """The notebook's objective (src/main.ipynb:158-161) built on the device from the handle's own k_trans /
        init_mode / xf; Q, Qf: 15 diagonal entries, R: 5."""
        Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(15)
        R = np.ascontiguousarray(R, dtype=np.float64).reshape(5)
        Qf = np.ascontiguousarray(Qf, dtype=np.float64).reshape(15)
        _lib.check(_lib.lib().qln_set_lqr_cost(self._h, Q.ctypes.data, R.ctypes.data, Qf.ctypes.data, float(dt),
                                               1 if per_problem else 0))
        self.cost_batch = self.B if per_problem else 1

    def get_cost(self):
        cb = C.c_int32()
        _lib.check(_lib.lib().qln_get_cost(self._h, None, C.byref(cb)))
        out = np.zeros((cb.value, self.N, _lib.COST_STRIDE))
        _lib.check(_lib.lib().qln_get_cost(self._h, out.ctypes.data, C.byref(cb)))
        return out[0] if cb.value == 1 else out

    def time_c_and_jac(self, Z, c, vals, warmup: int, iters: int, write_constants: bool = False):
        """HIP-event duration (ms) of each of `iters` launches of the fused hot path."""
        ms = (C.c_float * iters)()
        flags = _lib.QLN_JAC_WRITE_CONSTANTS if write_constants else 0
        _lib.check(_lib.lib().qln_time_constraint_and_jacobian(
            self._h, self._check(Z, self.dims.z_total, "Z"), self._check(c, self.dims.c_total, "c"),
            self._check(vals, self.dims.j_total, "vals"), flags, warmup, iters, ms))
        return np.array(ms[:], dtype=np.float64)

    def time_c_and_jac_total(self, Z, c, vals, warmup: int, iters: int, write_constants: bool = False) -> float:
        """Elapsed ms of `iters` launches of the fused hot path issued back to back, one pair of HIP events around all of them."""
        ms = C.c_float()
        flags = _lib.QLN_JAC_WRITE_CONSTANTS if write_constants else 0
        _lib.check(_lib.lib().qln_time_constraint_and_jacobian_total(
            self._h, self._check(Z, self.dims.z_total, "Z"), self._check(c, self.dims.c_total, "c"),
            self._check(vals, self.dims.j_total, "vals"), flags, warmup, iters, C.byref(ms)))
        return float(ms.value)

    # -- host-pointer (MOI) mode ------------------------------------------------------------------
    def _host_Z(self, Z, name="Z"):
        Z = np.asarray(Z, dtype=np.float64)
        if Z.size == self.B * self.n_nlp and self.z_stride != self.n_nlp:
            buf = np.zeros((self.B, self.z_stride))
            buf[:, : self.n_nlp] = Z.reshape(self.B, self.n_nlp)
            Z = buf
        Z = np.ascontiguousarray(Z.reshape(-1))
        if Z.size != self.dims.z_total:
            raise ValueError(f"{name} has {Z.size} entries, expected {self.dims.z_total}")
        return Z

    def _host_c(self, c, name):
        c = np.ascontiguousarray(np.asarray(c, dtype=np.float64).reshape(-1))
        if c.size != self.dims.c_total:
            raise ValueError(f"{name} has {c.size} entries, expected {self.dims.c_total}")
        return c

    def _host_sigma(self, sigma):
        """sigma broadcast to (B,), or None (1.0 for every problem)."""
        if sigma is None:
            return None
        return np.ascontiguousarray(np.broadcast_to(np.asarray(sigma, dtype=np.float64), (self.B,)))

    def _host_K(self, K):
        """Gains flattened, or None (the open-loop roll-out)."""
        if K is None:
            return None
        K = np.ascontiguousarray(np.asarray(K, dtype=np.float64).reshape(-1))
        nk = self.B * (self.N - 1) * _lib.TRACK_NU * n
        if K.size != nk:
            raise ValueError(f"K has {K.size} entries, expected {nk}")
        return K

    def eval_f_host(self, Z):
        Z = self._host_Z(Z)
        f = np.zeros(self.B)
        _lib.check(_lib.lib().qln_eval_objective_host(self._h, Z.ctypes.data, f.ctypes.data))
        return f

    def grad_f_host(self, Z):
        Z = self._host_Z(Z)
        g = np.zeros(self.dims.z_total)
        _lib.check(_lib.lib().qln_eval_objective_gradient_host(self._h, Z.ctypes.data, g.ctypes.data))
        return g

    def eval_c_host(self, Z):
        Z = self._host_Z(Z)
        c = np.zeros(self.dims.c_total)
        _lib.check(_lib.lib().qln_eval_constraint_host(self._h, Z.ctypes.data, c.ctypes.data))
        return c

    def jac_c_host(self, Z):
        Z = self._host_Z(Z)
        v = np.zeros(self.dims.j_total)
        _lib.check(_lib.lib().qln_eval_constraint_jacobian_host(self._h, Z.ctypes.data, v.ctypes.data))
        return v

    def jac_vec_host(self, Z, v):
        """jac_vec with host arrays (MOI mode): returns a (c_total,) numpy array."""
        Z, v = self._host_Z(Z), self._host_Z(v, "v")
        y = np.zeros(self.dims.c_total)
        _lib.check(_lib.lib().qln_eval_constraint_jvp_host(self._h, Z.ctypes.data, v.ctypes.data, y.ctypes.data))
        return y

    def jac_t_vec_host(self, Z, lam):
        """jac_t_vec with host arrays (MOI mode): returns a (z_total,) numpy array (zeros past n_nlp)."""
        Z, lam = self._host_Z(Z), self._host_c(lam, "lam")
        g = np.zeros(self.dims.z_total)
        _lib.check(_lib.lib().qln_eval_constraint_vjp_host(self._h, Z.ctypes.data, lam.ctypes.data, g.ctypes.data))
        return g

    def estimate_multipliers_host(self, Z, c=None, g=None, *, act_tol: float = 1e-6, bound_tol: float = 1e-8,
                                  row_scaling: bool = True, max_iters: int = 20000, rel_tol: float = 1e-8, want_lag: bool = True,
                                  want_info: bool = True, **bounds):
        """estimate_multipliers with host arrays (MOI mode): returns numpy (lam (c_total,), lag (z_total,) or None,
        info (B, 16) or None)."""
        Z = self._host_Z(Z)
        c = self.eval_c_host(Z) if c is None else self._host_c(c, "c")
        g = self.grad_f_host(Z) if g is None else self._host_Z(g, "g")
        lam = np.zeros(self.dims.c_total)
        lag = np.zeros(self.dims.z_total) if want_lag else None
        info = np.zeros((self.B, _lib.MULT_INFO_STRIDE)) if want_info else None
        opt = self._bound_options(bounds)
        _lib.check(_lib.lib().qln_estimate_multipliers_host(
            self._h, Z.ctypes.data, c.ctypes.data, g.ctypes.data, C.byref(opt), float(act_tol), float(bound_tol),
            int(bool(row_scaling)), int(max_iters), float(rel_tol), lam.ctypes.data, _host_ptr(lag), _host_ptr(info)))
        return lam, lag, info

    def jac_c_dense_host(self, Z_b, jac, b: int = 0):
        """Reference-compatible dense Jacobian of problem b: `jac` is a Fortran-ordered
        (m_nlp, n_nlp) float64 array; only the jac_c! write-set is assigned."""
        Z_b = np.ascontiguousarray(Z_b, dtype=np.float64)
        mm, _ = self.problem_dims(b)
        if Z_b.size != self.n_nlp:
            raise ValueError("Z_b must hold one problem's n_nlp entries")
        if not (jac.dtype == np.float64 and jac.flags.f_contiguous and jac.shape == (mm, self.n_nlp)):
            raise ValueError("jac must be a Fortran-ordered float64 (m_nlp, n_nlp) array")
        _lib.check(_lib.lib().qln_eval_constraint_jacobian_dense_host(self._h, b, Z_b.ctypes.data, jac.ctypes.data))
        return jac

    # -- views ------------------------------------------------------------------------------------
    def split_c(self, c_host, b: int = 0):
        mm, _ = self.problem_dims(b)
        return np.asarray(c_host)[self.c_off[b] : self.c_off[b] + mm]

    def split_vals(self, vals_host, b: int = 0):
        _, nz = self.problem_dims(b)
        return np.asarray(vals_host)[self.j_off[b] : self.j_off[b] + nz]


# ----------------------------------------------------------------------------- caller-side pieces of solve()


def variable_bounds(N: int):
    """Variable bounds exactly as `solve()` sets them (src/moi.jl:51-67), 0-based arrays (x_l, x_u).

    Reproduces the reference's quirk Q6 on purpose: its "lower bound of F" lines index
    `22+20(k-1)` and `24+20(k-1)` (1-based), which are yb_{k+1} and x1_{k+1}, not F1y/F2y (17, 19);
    the Ipopt header of the shipped run confirms it ("variables with only lower bounds: 120",
    src/main.ipynb:222).  Pass quirk_Q6=False to bound the forces instead.
    """
    return _variable_bounds(N, True)


def _variable_bounds(N: int, quirk_Q6: bool):
    n_nlp = num_primals(N)
    x_l, x_u = np.full(n_nlp, -np.inf), np.full(n_nlp, np.inf)
    for k in range(1, N + 1):
        x_l[3 + 20 * (k - 1) - 1] = -np.pi / 2  # theta >= -pi/2
        x_u[3 + 20 * (k - 1) - 1] = np.pi / 2
        if k < N:
            x_l[20 + 20 * (k - 1) - 1] = 0.001  # dt
            x_u[20 + 20 * (k - 1) - 1] = 0.02
            if quirk_Q6:
                x_l[22 + 20 * (k - 1) - 1] = 0.0
                x_l[24 + 20 * (k - 1) - 1] = 0.0
            else:
                x_l[17 + 20 * (k - 1) - 1] = 0.0
                x_l[19 + 20 * (k - 1) - 1] = 0.0
    return x_l, x_u


def variable_bounds_forces(N: int):
    """The bounds the comment in src/moi.jl:63 describes (F1y, F2y >= 0) -- not what the reference does."""
    return _variable_bounds(N, False)


def split_bound_multipliers(lag, Z, x_l=None, x_u=None, *, bound_tol: float = 1e-8):
    """(z_L, z_U) of Ipopt's convention (grad f + J'lam - z_L + z_U = 0) from the fixed columns of `lag` = g + A'lam as
    estimate_multipliers returns it: lag_j = z_L_j - z_U_j where Z_j is within bound_tol of a bound, so z_L = max(lag, 0)
    at a lower bound and z_U = max(-lag, 0) at an upper one; both are >= 0 where the sign is right and 0 where it is not
    (info[8] counts those) and on every free column.  `lag`, `Z`: (..., n_nlp) arrays of the same shape; x_l, x_u default to
    variable_bounds(N)."""
    lag, Z = np.asarray(lag, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    if x_l is None or x_u is None:
        x_l, x_u = variable_bounds((Z.shape[-1] + 5) // 20)
    with np.errstate(invalid="ignore"):
        at_l, at_u = Z <= x_l + bound_tol, Z >= x_u - bound_tol
    if bound_tol < 0:
        at_l, at_u = np.zeros_like(at_l), np.zeros_like(at_u)
    z_L = np.where(at_l & ~at_u, np.maximum(lag, 0.0), 0.0)
    z_U = np.where(at_u & ~at_l, np.maximum(-lag, 0.0), 0.0)
    return z_L, z_U


def ipopt_initial_point(Z0, x_l, x_u, *, bound_push: float = 1e-2, bound_frac: float = 1e-2,
                        bound_relax_factor: float = 1e-8, constr_viol_tol: float = 1e-6):
    """The point at which Ipopt 3.13 evaluates iteration 0 when `solve()` (src/moi.jl:46-103) hands it `Z0` and the
    variable bounds: Ipopt first relaxes every finite bound by min(constr_viol_tol, bound_relax_factor*max(1,|b|))
    and then pushes the starting point inside the relaxed bounds by bound_push / bound_frac (Ipopt options of the
    same names at their defaults; `solve()` sets constr_viol_tol = c_tol = 1e-6).  With `variable_bounds(N)` -- quirk
    Q6 included -- this reproduces the iteration-0 objective the notebook printed, 1.8380701e+00
    (src/main.ipynb:232): known answer KA6."""
    x = np.array(Z0, dtype=np.float64, copy=True)
    x_l, x_u = np.asarray(x_l, dtype=np.float64), np.asarray(x_u, dtype=np.float64)
    has_l, has_u = np.isfinite(x_l), np.isfinite(x_u)
    with np.errstate(invalid="ignore"):
        lo = np.where(has_l, x_l - np.minimum(constr_viol_tol, bound_relax_factor * np.maximum(1.0, np.abs(x_l))), x_l)
        up = np.where(has_u, x_u + np.minimum(constr_viol_tol, bound_relax_factor * np.maximum(1.0, np.abs(x_u))), x_u)
        p_l = bound_push * np.maximum(1.0, np.abs(lo))
        p_u = bound_push * np.maximum(1.0, np.abs(up))
        both = has_l & has_u
        frac = bound_frac * (up - lo)
        p_l = np.where(both, np.minimum(p_l, frac), p_l)
        p_u = np.where(both, np.minimum(p_u, frac), p_u)
        x = np.where(has_l, np.maximum(x, lo + p_l), x)
        x = np.where(has_u, np.minimum(x, up - p_u), x)
    return x
