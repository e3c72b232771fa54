"""The host forms of the tracking family whose other tests stay in mapped memory, at a size that is staged through device
memory: B = 64, N = 40 on a padded layout (Z_STRIDE below).  Every output of a host form is the device form's,
bit for bit, on the same inputs; the device forms are held to the numpy yardsticks by their own modules, so none is needed
here.  The inputs are the case modules': tests/rollout_guarded_cases.py's guarded case with gains and per-problem models,
tests/rollout_limited_ref.py's limits, tests/rollout_estimated_cases.py's draws and tests/tracking_cases.py's weights.

The host-form tests of those modules run one case each against a yardstick at the yardstick's size, so these are cases of
a module of their own rather than further parameters of them; one handle and one set of inputs serve all of them."""
import functools

import numpy as np
import pytest

from quadruped_landing_amd import _lib
from quadruped_landing_amd import nlp as NL
from tests import rollout_estimated_cases as EC
from tests import rollout_guarded_cases as GC
from tests import rollout_limited_ref as LR
from tests import tracking_abi as TA
from tests import tracking_cases as TC
from tests import tracking_cov_ref as CR

pytestmark = pytest.mark.gpu

B, N, NY = 64, 40, 3
# With the default layout this batch is 8 * (50 880 + 47 090 + 824 309) = 7.4 MB and stays in mapped memory (the B = 64 of
# tests/test_gpu_hessian_product.py is staged because its N is 61).  Padding every problem's Z to 3 000 doubles takes it to
# 8.5 MB, past the switch at 8 MiB, with the same B and N; the padding must come back untouched as well.
Z_STRIDE = 3000


@functools.lru_cache(maxsize=None)
def _case():
    """The handle and the inputs every test shares; nothing here is changed afterwards."""
    batch, Zref, K, x0, th = GC.case(N, 1, B, True, True)
    nlp = TC.nlp(batch, TC.SECOND_MODEL, z_stride=Z_STRIDE)
    d = nlp.dims
    assert 8 * (d.z_total + d.c_total + d.j_total) > 8 << 20  # past the switch from mapped to staged buffers
    rng = np.random.default_rng(64)

    def like_Z(scale=1.0):
        z = np.zeros((B, nlp.z_stride))
        z[:, :nlp.n_nlp] = scale * rng.normal(size=(B, nlp.n_nlp))
        return z.reshape(-1)

    Z = np.zeros((B, nlp.z_stride))
    Z[:, :nlp.n_nlp] = Zref
    e = EC.draws(64, B, N, NY)
    ins = dict(Zref=Z.reshape(-1), K=K, x0=x0, model=th, lim=LR.TEST_LIMITS, guarded=1, ny=NY, sigma0_batch=B,
               Qdiag=TC.QW, Rdiag=TC.R, Qfdiag=TC.QFW, Wdiag=rng.uniform(0.0, 1e-2, size=15), Vdiag=rng.uniform(1e-6, 1e-4, size=8),
               Sigma0=NL.pack_covariance(1e-6 * CR.random_psd(rng, shape=(B,))), Lgain=e["Lgain"], H=e["H"], vnoise=e["vnoise"],
               wnoise=e["wnoise"], xhat0=x0 + e["dxhat0"],
               # tangents and cotangents
               Zref_dot=like_Z(), K_dot=rng.normal(size=K.shape), x0_dot=rng.normal(size=x0.shape), model_dot=th * rng.normal(size=th.shape),
               Lgain_dot=rng.normal(size=e["Lgain"].shape), xhat0_dot=rng.normal(size=x0.shape), Zbar=like_Z(),
               Xhat_bar=rng.normal(size=(B, N, 15)), innov_bar=rng.normal(size=(B, N, NY)))
    return nlp, ins


def _both(name, outs, **more):
    """Runs the device form and the host form of one entry point on the shared inputs (and `more`), asserts that every output
    agrees bit for bit, and returns the outputs by parameter name."""
    import torch

    nlp, ins = _case()
    ins = {**ins, **more}
    dev, host = {}, {}
    for p in TA.PARAMS[name]:
        if p in outs:
            n = TA.size(p, B, N, nlp.dims.z_total)
            dev[p], host[p] = torch.zeros(n, dtype=torch.float64, device="cuda"), np.zeros(n)
        elif ins[p] is None or TA.is_int(name, p):
            dev[p] = host[p] = ins[p]
        else:
            host[p] = np.ascontiguousarray(ins[p], dtype=np.float64).reshape(-1)
            dev[p] = host[p] if p in TA.HOST_ONLY else torch.from_numpy(host[p]).cuda()
    L = _lib.lib()
    assert TA.call(nlp._h, name, dev) == _lib.QLN_OK, L.qln_last_error()
    torch.cuda.synchronize()
    assert TA.call(nlp._h, name + "_host", host) == _lib.QLN_OK, L.qln_last_error()
    got = {p: dev[p].cpu().numpy() for p in outs}
    for p in outs:
        assert got[p].any(), (name, p)
        assert np.array_equal(got[p].view(np.int64), host[p].view(np.int64)), (name, p)
    return got


@functools.lru_cache(maxsize=None)
def _guarded():
    return _both("qln_tracking_rollout_guarded", ("Zout", "event"))


@functools.lru_cache(maxsize=None)
def _limited():
    return _both("qln_tracking_rollout_limited", ("Zout", "event", "sat"))


@functools.lru_cache(maxsize=None)
def _estimated(guarded):
    if guarded:
        return _both("qln_tracking_rollout_estimated_guarded", ("Zout", "Xhat", "innov", "event", "event_hat"))
    return _both("qln_tracking_rollout_estimated", ("Zout", "Xhat", "innov"))


def test_guarded_rollout_and_its_sweeps():
    r = _guarded()
    _both("qln_tracking_rollout_guarded_jvp", ("Zout_dot", "event_dot"), **r)
    _both("qln_tracking_rollout_guarded_vjp", ("Zref_bar", "K_bar", "x0_bar", "model_bar"), **r)


def test_guarded_gains_and_covariance():
    r = _guarded()
    _both("qln_tracking_lqr_guarded", ("K", "P"), Ztraj=r["Zout"], event=r["event"])
    _both("qln_tracking_covariance_guarded", ("Sigma", "marg", "event_var"), **r)


def test_limited_rollout_its_sweeps_and_gains():
    r = _limited()
    assert (r["sat"] != 0).any(), "no force rode a limit"
    _both("qln_tracking_rollout_limited_jvp", ("Zout_dot", "event_dot"), **r)
    _both("qln_tracking_rollout_limited_vjp", ("Zref_bar", "K_bar", "x0_bar", "model_bar"), **r)
    _both("qln_tracking_lqr_limited", ("K", "P"), Ztraj=r["Zout"], event=r["event"], sat=r["sat"])


@pytest.mark.parametrize("guarded", [False, True])
def test_estimated_sweeps(guarded):
    r = _estimated(guarded)
    g = "_guarded" if guarded else ""
    events = ("event_dot", "event_hat_dot") if guarded else ()
    _both(f"qln_tracking_rollout_estimated{g}_jvp", ("Zout_dot", "Xhat_dot", "innov_dot") + events, **r)
    _both(f"qln_tracking_rollout_estimated{g}_vjp", ("Zref_bar", "K_bar", "Lgain_bar", "x0_bar", "xhat0_bar", "model_bar"), **r)
