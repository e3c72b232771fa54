"""What tests/test_gpu_binding_calls.py records: every public method of the tracking and landing section of HybridNLP, in both
memory forms, driven while a recorder sits in front of _lib.lib().  A trace entry is one line: the C calls a method made -- the
symbol and every argument, by position, as an integer, null, in:<name> (a buffer the caller passed, or the staged copy of one,
found by content), out:<position> (a buffer the method returned), or host:/dev:<values> (a constant the binding staged; the
arguments that are host arrays in both forms, H and Sigma0 always say in which memory what the C call reads lives) -- and
the structure of what it returned, or the exception it raised.  Only public methods and _lib.lib() are touched, so the same module records at
any commit.  Not a test module."""
import ctypes as C
import hashlib
import inspect
import os

import numpy as np

from quadruped_landing_amd import _lib
from tests import rollout_estimated_cases as EC
from tests import rollout_guarded_cases as GC
from tests import tracking_abi as TA
from tests import tracking_cases as TC

GOLDEN = os.path.join(TA.ROOT, "tests", "golden", "binding_calls.json")
PARAMS = TA.parameter_names(("tracking", "landing"))
B, N = 3, 5
# n_nlp = 95: with z_stride 96 the host forms pad a Z given as (B, n_nlp) rows; by default z_stride == n_nlp
HANDLES = {"padded": {"z_stride": 96}, "unpadded": {}}
STAGED = set(TA.HOST_ONLY) | {"H", "Sigma0"}  # arguments that are no buffers of the memory form: where their copy lives is said


def doubles(p, B, N, ny, nb, z_total):
    """doubles behind the parameter p of a call with ny measurement rows and nb initial covariances"""
    if p in ("Qdiag", "Qfdiag", "Wdiag"):
        return 15
    if p in ("Rdiag", "Vdiag", "lim", "H"):
        return {"Rdiag": 4, "Vdiag": ny, "lim": 8, "H": 15 * ny}[p]
    if p.startswith("Z"):
        return z_total
    if p.startswith("K"):
        return B * (N - 1) * 60
    if p.startswith(("x0", "xhat0")):
        return B * 15
    if p.startswith("model"):
        return B * 4
    if p == "event_var":
        return B * 2
    if p.startswith("event"):
        return B * 8
    if p == "sat":
        return B * (N - 1)
    if p in ("P", "Pest", "Sigma", "Ps"):
        return B * N * 120
    if p == "Sigma0":
        return nb * 120
    if p.startswith("Lgain"):
        return B * N * 15 * ny
    if p == "wnoise":
        return B * (N - 1) * 15
    if p.startswith("Xhat") or p == "Xs":
        return B * N * 15
    if p == "marg":
        return B * N * 8
    if p == "score":
        return B * N * 2
    if p.startswith("nis"):
        return B * N
    if p.startswith("loglik"):
        return B
    if p == "vnoise" or p.startswith(("innov", "Y")):
        return B * N * ny
    raise KeyError(p)


class _Raw:
    """size doubles of device memory at addr, for torch.as_tensor"""

    def __init__(self, addr, size):
        self.__cuda_array_interface__ = {"shape": (size,), "typestr": "<f8", "data": (addr, False), "version": 2}


def _read(addr, size, on_host, device):
    if on_host:
        return np.array((C.c_double * size).from_address(addr))
    import torch

    return torch.as_tensor(_Raw(addr, size), device=torch.device("cuda", device)).cpu().numpy().copy()


def _is_array(a):
    return isinstance(a, np.ndarray) or hasattr(a, "data_ptr")


def _host(a):
    return np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float64).reshape(-1)


def _values(v):
    if v.size <= 16:
        return ",".join(repr(float(x)) for x in v)
    return f"{v.size}#{hashlib.sha1(np.ascontiguousarray(v).tobytes()).hexdigest()[:12]}"


def structure(res):
    """t[3,5,15] a tensor, n[288] an array, - for None; a tuple in (), a dict in {}"""
    def one(o):
        if o is None:
            return "-"
        dtype = str(o.dtype).replace("torch.", "")
        return ("n" if isinstance(o, np.ndarray) else "t") + str(list(o.shape)).replace(" ", "") + ("" if dtype == "float64" else dtype)

    if isinstance(res, dict):
        return "{" + ", ".join(f"{k}: {one(v)}" for k, v in res.items()) + "}"
    if isinstance(res, (tuple, list)):
        return "(" + ", ".join(one(o) for o in res) + ")"
    return one(res)


class Recorder:
    """Stands where _lib.lib() stood: the tracking and landing symbols are noted, with the content of every buffer at the time
    of the call, then called; dry, a call is noted and answered QLN_OK without being made (a refusal case whose buffers are
    short must not reach the device if the binding fails to refuse it)."""

    def __init__(self, real):
        self.real, self.calls, self.dry, self.nlp, self.host = real, [], False, None, False

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name not in PARAMS:
            return fn

        def wrapped(*args):
            self.calls.append((name, None if self.dry else self._snapshot(name, args[1:])))
            return _lib.QLN_OK if self.dry else fn(*args)

        return wrapped

    def _snapshot(self, name, args):
        names, types = PARAMS[name], _lib.SIGNATURES[name][1][1:]
        assert len(names) == len(types) == len(args), name
        ints = {p: int(v) for p, t, v in zip(names, types, args) if t is C.c_int32}
        out = []
        for p, t, v in zip(names, types, args):
            addr = getattr(v, "value", v)
            if t is C.c_int32:
                out.append(int(v))
            elif not addr:
                out.append(None)
            else:
                on_host = self.host or p in TA.HOST_ONLY
                size = doubles(p, self.nlp.B, self.nlp.N, ints.get("ny", 0), ints.get("sigma0_batch", 0), self.nlp.dims.z_total)
                out.append((int(addr), on_host, _read(int(addr), size, on_host, self.nlp.device), p in STAGED))
        return out


class Driver:
    """Calls the methods of one handle in one memory form and keeps the trace."""

    def __init__(self, nlp, host, rec, brief=False):
        self.nlp, self.host, self.rec, self.brief, self.trace, self.base = nlp, host, rec, brief, {}, {}

    # -- inputs in this form ---------------------------------------------------------------------------------------------
    def arr(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if self.host:
            return a
        import torch

        return torch.from_numpy(a).to(torch.device("cuda", self.nlp.device))

    def Z(self, a):
        """(B, n_nlp) rows: unpadded for the host form, which pads them; in the handle's layout on the device"""
        a = np.ascontiguousarray(a, dtype=np.float64)
        return a if self.host else self.nlp.upload_Z(a)

    def Zfull(self, a):
        """the same rows in the handle's layout in both forms: the filter's sweeps do not pad"""
        a = np.ascontiguousarray(a, dtype=np.float64)
        if not self.host:
            return self.nlp.upload_Z(a)
        pad = np.zeros((self.nlp.B, self.nlp.z_stride))
        pad[:, :self.nlp.n_nlp] = a
        return pad.reshape(-1)

    def dev(self, **kw):
        """arguments only the device forms take: buffers to write into, each given by its shape"""
        return {} if self.host else {k: self.arr(np.zeros(shape)) for k, shape in kw.items()}

    # -- one call --------------------------------------------------------------------------------------------------------
    def run(self, method, case, base=False, dry=False, **kw):
        """One call, kept as "method | case": "symbol(arguments by position); ... -> returns" or "... !! the exception".  base:
        the call the refusals start from, and all that a brief driver keeps."""
        name = method + ("_host" if self.host else "")
        if base:
            self.base[method] = dict(kw)
        self.rec.calls, self.rec.dry, self.rec.nlp, self.rec.host = [], dry, self.nlp, self.host
        res = None
        try:
            res = getattr(self.nlp, name)(**kw)
            end = " -> " + structure(res)
        except Exception as e:  # noqa: BLE001 -- the refusal is what is recorded
            end = f" !! {type(e).__name__}: {e}"
        if base or not self.brief:
            key = f"{name} | {case}"
            assert key not in self.trace, key
            self.trace[key] = "; ".join(self._describe(sym, snap, kw, res) for sym, snap in self.rec.calls) + end
        return res

    def _describe(self, sym, snap, kw, res):
        if snap is None:
            return sym + "(not made)"
        outs = res.items() if isinstance(res, dict) else enumerate(res if isinstance(res, (tuple, list)) else (res,))
        outs = [(k, o) for k, o in outs if o is not None]
        ins = [(k, a) for k, a in kw.items() if _is_array(a)]
        content = []
        for k, a in ins:
            h = _host(a)
            content.append((k, h))
            if h.size == self.nlp.B * self.nlp.n_nlp and self.nlp.z_stride != self.nlp.n_nlp:
                pad = np.zeros((self.nlp.B, self.nlp.z_stride))
                pad[:, :self.nlp.n_nlp] = h.reshape(self.nlp.B, self.nlp.n_nlp)
                content.append((k, pad.reshape(-1)))
        args = []
        for a in snap:
            if a is None or isinstance(a, int):
                args.append("null" if a is None else str(a))
                continue
            addr, on_host, data, staged = a
            hit = [f"out:{k}" for k, o in outs if TA.address(o) == addr] + [f"in:{k}" for k, i in ins if TA.address(i) == addr]
            hit += [f"in:{k}" for k, h in content if h.size == data.size and np.array_equal(h, data)]
            where = "host:" if on_host else "dev:"
            args.append((where if staged else "") + hit[0] if hit else where + _values(data))
        return f"{sym}({', '.join(args)})"


def handle(kind):
    """(the handle, the host inputs of its case): tests/rollout_guarded_cases.py's, on which the first problems land and the
    last one does not"""
    batch, Zref, K, x0, th = GC.case(N, 1, B, True, True)
    nlp = TC.nlp(batch, model=TC.SECOND_MODEL, **HANDLES[kind])
    assert (nlp.z_stride != nlp.n_nlp) == (kind == "padded"), (kind, nlp.z_stride, nlp.n_nlp)
    return nlp, (Zref, K, x0, th)


def drive(d, case):
    """Every method of the section in d's form, and one call each at ny = 1 and ny = 8."""
    nlp, (Zr, Kh, x0h, th) = d.nlp, case
    rng = np.random.default_rng(5)
    rnd = lambda *s, scale=1.0: d.arr(scale * rng.normal(size=s))  # noqa: E731
    rZ = lambda scale=1.0: d.Z(scale * rng.normal(size=(B, nlp.n_nlp)))  # noqa: E731
    Zref, K, x0, model = d.Z(Zr), d.arr(Kh), d.arr(x0h), d.arr(th)
    Q, R, Qf = TC.QW, TC.R, TC.QFW
    W = np.array([1e-8] * 14 + [0.0])
    ny = 2
    H, V = EC.sensors()[:ny], 1e-6 * (1.0 + np.arange(ny))
    S0 = np.full(15, 1e-6)
    lim = np.array([-0.5, 0.5, -0.5, 0.5, -20.0, 20.0, -5.0, 40.0])
    zt = nlp.dims.z_total
    kshape, pshape, eshape = (B, N - 1, 4, 15), (B, N, 120), (B, 8)

    Zout = d.run("tracking_rollout", "all", base=True, Zref=Zref, K=K, x0=x0, **d.dev(out=(zt,)))
    # -- the Kalman gains, the estimate-feedback roll-out, the smoother and the filter: the methods that take H ----------------
    d.run("tracking_kalman", "defaults", Zout=Zout, H=H, V=V, Sigma0=S0)
    d.run("tracking_kalman", "ny = 1", Zout=Zout, H=EC.sensors()[:1], V=1e-6, K=K, Sigma0=S0)
    d.run("tracking_kalman", "ny = 8", Zout=Zout, H=EC.sensors(), V=1e-6 * (1.0 + np.arange(8)), K=K, Sigma0=S0, W=W)
    Lg, Pe, _, _ = d.run("tracking_kalman", "all", base=True, Zout=Zout, H=H, V=V, K=K, Sigma0=S0, W=W)
    est = dict(Zref=Zref, K=K, Lgain=Lg, H=H)
    noise = dict(vnoise=rnd(B, N, ny, scale=1e-3), wnoise=rnd(B, N - 1, 15, scale=1e-4), x0=x0,
                 xhat0=d.arr(x0h + 1e-3), model=model)
    d.run("tracking_rollout_estimated", "defaults", **est)
    Ze, Xh, iv = d.run("tracking_rollout_estimated", "all", base=True, **est, **noise, with_innovations=True, **d.dev(out=(zt,)))
    Zeg, Xhg, ivg, evp, evh = d.run("tracking_rollout_estimated", "guarded", **est, **noise, guarded=True, with_innovations=True)
    d.run("landing_smoother", "defaults", base=True, Ztraj=Ze, Lgain=Lg, Pest=Pe, H=H, V=V, Xhat=Xh, innov=iv)
    d.run("landing_smoother_guarded", "all", base=True, Ztraj=Zeg, events=evp, Lgain=Lg, Pest=Pe, H=H, V=V, Xhat=Xhg, innov=ivg,
          model=model)
    Y = nlp.landing_measurements(Ze, Zref, H)
    Y = d.arr(_host(Y).reshape(B, N, ny))
    fil = dict(Zref=Zref, Zrec=Ze, Lgain=Lg, H=H, Y=Y)
    Xf, ivf, _, _ = d.run("landing_filter", "defaults", **fil)
    d.run("landing_filter", "V", **fil, V=V)
    d.run("landing_filter", "all", base=True, **fil, V=V, xhat0=noise["xhat0"], model=model)
    Xfg, ivfg, _, _, ehf = d.run("landing_filter_guarded", "all", base=True, **fil, V=V, xhat0=noise["xhat0"], model=model)
    swp = dict(Zref=d.Zfull(Zr), Zrec=Ze, Lgain=Lg, H=H, Xhat=Xf)
    d.run("landing_filter_jvp", "defaults", **swp, Y_dot=rnd(B, N, ny))
    d.run("landing_filter_vjp", "defaults", **swp, Xhat_bar=rnd(B, N, 15))
    d.run("landing_filter_jvp", "Zref in rows of n_nlp", **dict(swp, Zref=Zref), Y_dot=rnd(B, N, ny))
    dots = dict(Y_dot=rnd(B, N, ny), Zrec_dot=d.Zfull(rng.normal(size=(B, nlp.n_nlp))), Lgain_dot=rnd(B, N, 15, ny, scale=1e-2), xhat0_dot=rnd(B, 15),
                model_dot=rnd(B, 4, scale=1e-2))
    bars = dict(Xhat_bar=rnd(B, N, 15), innov_bar=rnd(B, N, ny), nis_bar=rnd(B, N), loglik_bar=rnd(B))
    d.run("landing_filter_jvp", "all", base=True, **swp, innov=ivf, V=V, model=model, **dots)
    d.run("landing_filter_jvp", "score", **swp, innov=ivf, V=V, Y_dot=dots["Y_dot"])
    d.run("landing_filter_jvp", "want", **swp, innov=ivf, V=V, Y_dot=dots["Y_dot"], want=("loglik",))
    swg = dict(swp, Xhat=Xfg, innov=ivfg, V=V, model=model, events_hat=ehf, guarded=True)
    d.run("landing_filter_jvp", "guarded", **swg, Y_dot=dots["Y_dot"], model_dot=dots["model_dot"])
    d.run("landing_filter_jvp", "guarded want", **swg, Y_dot=dots["Y_dot"], want=("event_hat", "Xhat"))
    d.run("landing_filter_vjp", "all", base=True, **swp, innov=ivf, V=V, model=model, **bars)
    d.run("landing_filter_vjp", "gain", **swp, innov=ivf, Xhat_bar=bars["Xhat_bar"], innov_bar=bars["innov_bar"])
    d.run("landing_filter_vjp", "want", **swp, innov=ivf, V=V, loglik_bar=bars["loglik_bar"], want=("Y", "model"))
    d.run("landing_filter_vjp", "guarded", **swg, Xhat_bar=bars["Xhat_bar"], loglik_bar=bars["loglik_bar"])
    for flag in ("with_estimate", "with_innovations", "with_score"):
        d.run("landing_filter", f"{flag} off", **fil, V=V, **{flag: False})
        d.run("landing_filter_guarded", f"{flag} off", **fil, V=V, **{flag: False})
    d.run("landing_filter_guarded", "defaults", **fil)
    d.run("landing_filter_guarded", "with_events off", **fil, with_events=False)
    for flag in ("with_states", "with_cov"):
        d.run("landing_smoother", f"{flag} off", **d.base["landing_smoother"], **{flag: False})
        d.run("landing_smoother_guarded", f"{flag} off", **d.base["landing_smoother_guarded"], **{flag: False})
    for flag in ("with_gains", "with_pest", "with_sigma", "with_marginals"):
        d.run("tracking_kalman", f"{flag} off", **d.base["tracking_kalman"], **{flag: False})
    d.run("tracking_rollout_estimated", "with_estimate off", **est, with_estimate=False)
    for flag in ("with_estimate", "with_events"):
        d.run("tracking_rollout_estimated", f"guarded {flag} off", **est, guarded=True, **{flag: False})

    # -- the gains ---------------------------------------------------------------------------------------------------------
    d.run("tracking_lqr", "defaults", Zref=Zref, Q=Q, R=R, Qf=Qf)
    d.run("tracking_lqr", "all", base=True, Zref=Zref, Q=Q, R=R, Qf=Qf, **d.dev(K=kshape, P=pshape))
    d.run("tracking_lqr", "with_cost_to_go off", Zref=Zref, Q=10.0, R=1e-2, Qf=30.0, with_cost_to_go=False)
    # -- the roll-out and its sweeps, plain and with a plant model ---------------------------------------------------------------
    d.run("tracking_rollout", "defaults", Zref=Zref)
    d.run("tracking_rollout_model", "defaults", Zref=Zref)
    Zm = d.run("tracking_rollout_model", "all", base=True, Zref=Zref, K=K, x0=x0, model=model, **d.dev(out=(zt,)))
    Zbar = rZ()
    tan = dict(Zref_dot=rZ(), K_dot=rnd(*kshape, scale=1e-2), x0_dot=rnd(B, 15))
    md = rnd(B, 4, scale=1e-2)
    d.run("tracking_rollout_vjp", "defaults", Zref=Zref, Zout=Zout, Zbar=Zbar)
    d.run("tracking_rollout_vjp", "all", base=True, Zref=Zref, Zout=Zout, Zbar=Zbar, K=K)
    d.run("tracking_rollout_vjp", "want", Zref=Zref, Zout=Zout, Zbar=Zbar, K=K, want=("x0",))
    d.run("tracking_rollout_model_vjp", "defaults", Zref=Zref, Zout=Zm, Zbar=Zbar)
    d.run("tracking_rollout_model_vjp", "all", base=True, Zref=Zref, Zout=Zm, Zbar=Zbar, K=K, model=model)
    d.run("tracking_rollout_model_vjp", "want", Zref=Zref, Zout=Zm, Zbar=Zbar, K=K, model=model, want=("model", "Zref"))
    d.run("tracking_rollout_jvp", "one tangent", Zref=Zref, Zout=Zout, x0_dot=tan["x0_dot"])
    d.run("tracking_rollout_jvp", "all", base=True, Zref=Zref, Zout=Zout, K=K, **tan, **d.dev(out=(zt,)))
    d.run("tracking_rollout_model_jvp", "one tangent", Zref=Zref, Zout=Zm, model_dot=md)
    d.run("tracking_rollout_model_jvp", "all", base=True, Zref=Zref, Zout=Zm, K=K, model=model, **tan, model_dot=md,
          **d.dev(out=(zt,)))
    # -- through the guarded touchdown ---------------------------------------------------------------------------------------
    d.run("tracking_rollout_guarded", "defaults", Zref=Zref)
    Zg, ev = d.run("tracking_rollout_guarded", "all", base=True, Zref=Zref, K=K, x0=x0, model=model, **d.dev(out=(zt,)))
    d.run("tracking_rollout_guarded", "with_events off", Zref=Zref, K=K, x0=x0, model=model, with_events=False)
    gd = dict(Zref=Zref, Zout=Zg, events=ev)
    d.run("tracking_rollout_guarded_jvp", "one tangent", **gd, Zref_dot=tan["Zref_dot"])
    d.run("tracking_rollout_guarded_jvp", "all", base=True, **gd, K=K, model=model, **tan, model_dot=md, **d.dev(out=(zt,)))
    d.run("tracking_rollout_guarded_jvp", "with_event_dot off", **gd, K=K, model=model, **tan, with_event_dot=False)
    d.run("tracking_rollout_guarded_vjp", "defaults", **gd, Zbar=Zbar)
    d.run("tracking_rollout_guarded_vjp", "all", base=True, **gd, Zbar=Zbar, K=K, model=model)
    d.run("tracking_rollout_guarded_vjp", "want", **gd, Zbar=Zbar, K=K, model=model, want=("K",))
    d.run("tracking_lqr_guarded", "defaults", Ztraj=Zg, events=ev, Q=Q, R=R, Qf=Qf)
    d.run("tracking_lqr_guarded", "all", base=True, Ztraj=Zg, events=ev, Q=Q, R=R, Qf=Qf, model=model,
          **d.dev(K=kshape, P=pshape))
    d.run("tracking_lqr_guarded", "with_cost_to_go off", Ztraj=Zg, events=ev, Q=Q, R=R, Qf=Qf, with_cost_to_go=False)
    # -- the covariances -------------------------------------------------------------------------------------------------------
    d.run("tracking_covariance", "defaults", Zout=Zout, Sigma0=S0)
    d.run("tracking_covariance", "all", base=True, Zout=Zout, K=K, Sigma0=np.tile(np.diag(S0), (B, 1, 1)), W=W,
          **d.dev(Sigma=pshape, marg=(B, N, 8)))
    if not d.host:
        from quadruped_landing_amd import nlp as NL

        d.run("tracking_covariance", "device Sigma0", Zout=Zout, K=K, Sigma0=d.arr(NL.pack_covariance(np.diag(S0))[None]))
    cg = dict(Zout=Zg, events=ev, K=K, Sigma0=S0, W=W, model=model)
    d.run("tracking_covariance_guarded", "defaults", Zout=Zg, events=ev, Sigma0=S0)
    d.run("tracking_covariance_guarded", "all", base=True, **cg, **d.dev(Sigma=pshape, marg=(B, N, 8)))
    for flag in ("with_sigma", "with_marginals"):
        d.run("tracking_covariance", f"{flag} off", Zout=Zout, K=K, Sigma0=S0, **{flag: False})
    for flag in ("with_sigma", "with_marginals", "with_event_var"):
        d.run("tracking_covariance_guarded", f"{flag} off", **cg, **{flag: False})
    kg = dict(Zout=Zg, events=ev, H=H, V=V, Sigma0=S0)
    d.run("tracking_kalman_guarded", "defaults", **kg)
    d.run("tracking_kalman_guarded", "all", base=True, **kg, K=K, W=W, model=model)
    for flag in ("with_gains", "with_pest", "with_sigma", "with_marginals", "with_event_var"):
        d.run("tracking_kalman_guarded", f"{flag} off", **kg, K=K, **{flag: False})
    # -- the sweeps through the estimate-feedback roll-out ---------------------------------------------------------------------
    et = dict(Zref=Zref, K=K, Lgain=Lg, H=H, Zout=Ze, Xhat=Xh)
    eg = dict(et, Zout=Zeg, Xhat=Xhg, innov=ivg, model=model, events=evp, events_hat=evh)
    edots = dict(tan, Lgain_dot=rnd(B, N, 15, ny, scale=1e-2), xhat0_dot=rnd(B, 15), model_dot=md)
    ebars = dict(Xhat_bar=rnd(B, N, 15), innov_bar=rnd(B, N, ny))
    d.run("tracking_rollout_estimated_jvp", "one tangent", **et, Zref_dot=tan["Zref_dot"])
    d.run("tracking_rollout_estimated_jvp", "all", base=True, **et, innov=iv, model=model, **edots, **d.dev(out=(zt,)))
    d.run("tracking_rollout_estimated_jvp", "guarded", **eg, guarded=True, **edots)
    for flag in ("with_estimate", "with_innovations", "with_event_dot"):
        d.run("tracking_rollout_estimated_jvp", f"guarded {flag} off", **eg, guarded=True, **tan, **{flag: False})
    for flag in ("with_estimate", "with_innovations"):
        d.run("tracking_rollout_estimated_jvp", f"{flag} off", **et, **tan, **{flag: False})
    d.run("tracking_rollout_estimated_vjp", "defaults", **et, Zbar=Zbar)
    d.run("tracking_rollout_estimated_vjp", "all", base=True, **et, Zbar=Zbar, innov=iv, model=model, **ebars)
    d.run("tracking_rollout_estimated_vjp", "guarded", **eg, guarded=True, Zbar=Zbar, **ebars)
    d.run("tracking_rollout_estimated_vjp", "want", **et, Zbar=Zbar, innov=iv, want=("Lgain", "xhat0"))
    # -- contact-aware force limits ----------------------------------------------------------------------------------------------
    d.run("tracking_rollout_limited", "defaults", Zref=Zref, limits=lim)
    Zl, _, sat = d.run("tracking_rollout_limited", "all", base=True, Zref=Zref, limits=lim, K=K, x0=x0, model=model,
                       **d.dev(out=(zt,)))
    Zlg, evl, satg = d.run("tracking_rollout_limited", "guarded", Zref=Zref, limits=lim, K=K, x0=x0, model=model, guarded=True)
    for flag in ("with_events", "with_sat"):
        d.run("tracking_rollout_limited", f"guarded {flag} off", Zref=Zref, limits=lim, K=K, guarded=True, **{flag: False})
    d.run("tracking_rollout_limited", "with_sat off", Zref=Zref, limits=lim, K=K, with_sat=False)
    ld = dict(Zref=Zref, Zout=Zl, sat=sat)
    lg = dict(Zref=Zref, Zout=Zlg, sat=satg, events=evl, K=K, model=model)
    d.run("tracking_rollout_limited_jvp", "one tangent", **ld, Zref_dot=tan["Zref_dot"])
    d.run("tracking_rollout_limited_jvp", "all", base=True, **lg, **tan, model_dot=md, **d.dev(out=(zt,)))
    d.run("tracking_rollout_limited_jvp", "with_event_dot off", **lg, **tan, with_event_dot=False)
    d.run("tracking_rollout_limited_vjp", "defaults", **ld, Zbar=Zbar)
    d.run("tracking_rollout_limited_vjp", "all", base=True, **lg, Zbar=Zbar)
    d.run("tracking_rollout_limited_vjp", "want", **lg, Zbar=Zbar, want=("Zref", "x0"))
    d.run("tracking_lqr_limited", "defaults", Ztraj=Zl, sat=sat, Q=Q, R=R, Qf=Qf)
    d.run("tracking_lqr_limited", "all", base=True, Ztraj=Zlg, sat=satg, Q=Q, R=R, Qf=Qf, events=evl, model=model,
          **d.dev(K=kshape, P=pshape))
    d.run("tracking_lqr_limited", "with_cost_to_go off", Ztraj=Zl, sat=sat, Q=Q, R=R, Qf=Qf, with_cost_to_go=False)
    el = dict(Zref=Zref, limits=lim, K=K, Lgain=Lg, H=H)
    d.run("tracking_rollout_estimated_limited", "defaults", **el)
    Zel, Xhl, ivl, _, _, satl = d.run("tracking_rollout_estimated_limited", "all", base=True, **el, **noise, with_innovations=True,
                                      **d.dev(out=(zt,)))
    Zelg, Xhlg, ivlg, evpl, evhl, satlg = d.run("tracking_rollout_estimated_limited", "guarded", **el, **noise, guarded=True,
                                                with_innovations=True)
    for flag in ("with_estimate", "with_events", "with_sat"):
        d.run("tracking_rollout_estimated_limited", f"guarded {flag} off", **el, guarded=True, **{flag: False})
    for flag in ("with_estimate", "with_sat"):
        d.run("tracking_rollout_estimated_limited", f"{flag} off", **el, **{flag: False})
    lt = dict(Zref=Zref, K=K, Lgain=Lg, H=H, Zout=Zel, Xhat=Xhl, sat=satl)
    ltg = dict(lt, Zout=Zelg, Xhat=Xhlg, sat=satlg, innov=ivlg, model=model, events=evpl, events_hat=evhl)
    d.run("tracking_rollout_estimated_limited_jvp", "one tangent", **lt, Zref_dot=tan["Zref_dot"])
    d.run("tracking_rollout_estimated_limited_jvp", "all", base=True, **ltg, **edots, **d.dev(out=(zt,)))
    for flag in ("with_estimate", "with_innovations", "with_event_dot"):
        d.run("tracking_rollout_estimated_limited_jvp", f"{flag} off", **ltg, **tan, **{flag: False})
    for flag in ("with_estimate", "with_innovations"):
        d.run("tracking_rollout_estimated_limited_jvp", f"{flag} off, scheduled", **lt, **tan, **{flag: False})
    d.run("tracking_rollout_estimated_limited_vjp", "defaults", **lt, Zbar=Zbar)
    d.run("tracking_rollout_estimated_limited_vjp", "all", base=True, **ltg, Zbar=Zbar, **ebars)
    d.run("tracking_rollout_estimated_limited_vjp", "want", **lt, Zbar=Zbar, innov=ivl, want=("K", "Lgain"))

    # -- the rules across arguments that the binding enforces itself -----------------------------------------------------------
    d.run("landing_filter", "rule: with_score without V", **fil, with_score=True)
    d.run("landing_filter_jvp", "rule: guarded without events_hat", **swp, guarded=True, Y_dot=dots["Y_dot"])
    d.run("tracking_rollout_estimated_limited_jvp", "rule: events without events_hat", **lt, events=evpl,
          Zref_dot=tan["Zref_dot"])
    d.run("tracking_rollout_estimated_jvp", "rule: guarded without events_hat", **et, guarded=True, events=evp,
          Zref_dot=tan["Zref_dot"])
    d.run("tracking_rollout_estimated_jvp", "rule: Lgain_dot without innov", **et, Lgain_dot=edots["Lgain_dot"])
    d.run("tracking_rollout_estimated_vjp", "rule: Lgain wanted without innov", **et, Zbar=Zbar, want=("Lgain",))
    d.run("landing_filter_jvp", "rule: Lgain_dot without innov", **swp, Lgain_dot=dots["Lgain_dot"])
    d.run("landing_filter_jvp", "rule: event_hat wanted, not guarded", **swp, Y_dot=dots["Y_dot"], want=("Xhat", "event_hat"))
    for method, kw in (("tracking_rollout_vjp", dict(Zref=Zref, Zout=Zout, Zbar=Zbar)),
                       ("tracking_rollout_guarded_vjp", dict(gd, Zbar=Zbar)), ("tracking_rollout_limited_vjp", dict(ld, Zbar=Zbar)),
                       ("tracking_rollout_estimated_vjp", dict(et, Zbar=Zbar)),
                       ("landing_filter_jvp", dict(swp, Y_dot=dots["Y_dot"])),
                       ("landing_filter_vjp", dict(swp, Xhat_bar=bars["Xhat_bar"]))):
        d.run(method, "rule: unknown want", **kw, want=("Zref", "bogus"))


def refusals(d):
    """For every method that drive() gave a base call: every required argument None; one array argument one element short
    (not made if the binding lets it pass); and in the device form one tensor as the host array of its values (likewise).
    Which argument: the next one from method to method, so that every role has its turn."""
    for i, (method, kw) in enumerate(d.base.items()):
        sig = inspect.signature(getattr(d.nlp, method + ("_host" if d.host else "")))
        required = [p.name for p in sig.parameters.values() if p.default is p.empty]
        d.run(method, "refuse: required None", **{**kw, **{r: None for r in required}})
        arrays = [k for k, a in kw.items() if _is_array(a)]
        k = arrays[i % len(arrays)]
        d.run(method, f"refuse: {k} short", dry=True, **{**kw, k: kw[k].reshape(-1)[:-1]})
        tensors = [k for k, a in kw.items() if hasattr(a, "data_ptr")]
        if tensors:
            k = tensors[i % len(tensors)]
            d.run(method, f"refuse: {k} a host array", dry=True, **{**kw, k: kw[k].detach().cpu().numpy()})


def record():
    """The whole trace: {handle: {form: {"method | case": what it did}}}.  The padded handle runs everything; the unpadded one
    differs from it only in what becomes of a Z, so it keeps one call of every method, the one with every argument."""
    real = _lib.lib()
    rec = Recorder(real)
    lib_before, _lib.lib = _lib.lib, lambda: rec
    out = {}
    try:
        for kind in HANDLES:
            nlp, case = handle(kind)
            out[kind] = {}
            for form in ("device", "host"):
                d = Driver(nlp, form == "host", rec, brief=kind != "padded")
                drive(d, case)
                if kind == "padded":
                    refusals(d)
                out[kind][form] = d.trace
            nlp.synchronize()
            nlp.close()
    finally:
        _lib.lib = lib_before
    return out
