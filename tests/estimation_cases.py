"""What the GPU tests of the estimation family share -- the Kalman design and its two sweeps, the smoother, the filter and its
sweeps, the estimate-feedback roll-out, its sweeps and its limited forms: the time limit of a GPU step, the host-to-device
helper, the draw of a measurement model, the family's shapes, the design at a roll-out on the knot schedule and through the
guarded touchdown, the float64 / longdouble pair of a yardstick, and the plumbing of the estimate-feedback sweeps.  One
statement, so that every test module of the family sees the same inputs; a module keeps its own lru_cache'd _run on top, which
asks the GPU for its own operation and builds its own yardstick.  Not a test module: torch is imported inside the functions
that need it."""
import faulthandler
import itertools
import types

import numpy as np
import pytest

from tests import rollout_guarded_cases as GC
from tests import rollout_guarded_sweep_ref as SR
from tests import tracking_cases as TC
from tests import tracking_cov_ref as CR


def time_limit(seconds):
    """The autouse fixture of a GPU test module, `_time_limit = time_limit(600)`: every test there is a GPU step with a time limit
    of its own, and a hang ends the process with a traceback."""
    @pytest.fixture(autouse=True)
    def _time_limit():
        faulthandler.dump_traceback_later(seconds, exit=True)
        yield
        faulthandler.cancel_dump_traceback_later()

    return _time_limit


def dev(a):
    """A host array (float64 already: nothing is converted) on the device; None stays None."""
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def measurement(rng, ny, V=None):
    """H = normal / sqrt(15), V in [0.5, 2] (or the given value in every row)"""
    return rng.normal(size=(ny, 15)) / np.sqrt(15.0), rng.uniform(0.5, 2.0, size=ny) if V is None else np.full(ny, V)


def vec_rel(got, ref):
    """knot_rel on vectors (..., N, 15)"""
    return CR.knot_rel(np.asarray(got)[..., None], np.asarray(ref)[..., None])


def in_both_precisions(f, *arrays, **kw):
    """(f on the float64 arrays as they are, f on their longdouble copies); an argument that is None stays None.  The caller sets
    its own distance measure on the pair."""
    return f(*arrays, **kw), f(*(None if a is None else np.asarray(a).astype(np.longdouble) for a in arrays), **kw)


# ---- the shapes -------------------------------------------------------------------------------------------------------------
def design_shapes():
    """(kind, B, N, k_trans, init_mode, ny): N = 2 (one step, two updates), 3, and 17, 33 across the sixteen-knot chunk of the
    clearance cosines; k_trans in {1, 2, N, N + 1}, both init_modes; B = 3 (a partly filled wave) and 5 (a second wave with one
    row); ny takes turns over 8, 3, 1.  A module appends its own columns by the tuple's index."""
    out = []
    for i, (N, kt, im) in enumerate(itertools.product((2, 3, 17, 33), ("1", "2", "N", "N+1"), (1, 2))):
        k_trans = {"1": 1, "2": 2, "N": N, "N+1": N + 1}[kt]
        out.append(("shape", 3 if i % 2 else 5, N, k_trans, im, (8, 3, 1)[i % 3]))
    return out


RAGGED = [("ragged", 9, 17, 6, 1, 8), ("ragged", 6, 33, 12, 2, 3)]
GUARDED_SHAPES = [("shape", N, im, B) for (N, im, B) in GC.SHAPES]  # (kind, N, init_mode, B)
GUARDED_RAGGED = ("ragged", 12, 0, 70)  # GC.ragged_case


# ---- the design at a roll-out -------------------------------------------------------------------------------------------------
def scheduled_design(kind, B, N, k_trans, im, ny, sensor_seed, V=None, **handle_kw):
    """One knot-scheduled case up to its measurement model: the handle (handle_kw: TC.nlp's), random gains K, the roll-out Zout
    under them, a Sigma0 per problem and W (TC.cov_setup), H and V drawn by a generator seeded sensor_seed past the case's seed
    and left open as rng, and the evaluator's dense blocks at Zout: blocks(b, zo[b]) (N-1, 15, 20) and A (B, N-1, 15, 15)."""
    seed = 100 * N + 10 * k_trans + im
    batch = TC.batch(B, N, k_trans, im, seed=seed, ragged=kind == "ragged")
    nlp, K, Zout, S0, W = TC.cov_setup(batch, seed, True, **handle_kw)
    rng = np.random.default_rng(seed + sensor_seed)
    H, V = measurement(rng, ny, V)
    blocks, zo = TC.evaluator_blocks(nlp, Zout), TC.rows(nlp, Zout)
    A = np.stack([blocks(b, zo[b])[:, :, :15] for b in range(B)])
    return types.SimpleNamespace(nlp=nlp, seed=seed, K=K, Zout=Zout, S0=S0, W=W, H=H, V=V, rng=rng, blocks=blocks, zo=zo, A=A)


def guarded_design(kind, N, im, B, with_gains, with_models, ny=None, sensor_seed=43):
    """One case through the guarded touchdown up to its measurement model: GC.case (GC.ragged_case for kind 'ragged', which has
    gains and models of its own), the handle at TC.SECOND_MODEL, the guarded roll-out Zout with its events, and a Sigma0 per
    problem, W, H and V drawn in this order by a generator seeded sensor_seed past GC.seed_of and left open as rng; ny takes
    turns with N + B unless given.  F, T are the complex-step blocks of the composite step at Zout (SR.blocks)."""
    if kind == "ragged":
        batch, Zref, K, x0, th = GC.ragged_case()
        ims, with_models = np.asarray(batch.init_mode), True
    else:
        batch, Zref, K, x0, th = GC.case(N, im, B, with_gains, with_models)
        ims = im
    nlp = TC.nlp(batch, TC.SECOND_MODEL)
    dK, model = dev(K), dev(th) if with_models else None
    Zout, ev = nlp.tracking_rollout_guarded(nlp.upload_Z(Zref), dK, dev(x0), model)
    zo, evh = TC.rows(nlp, Zout), ev.cpu().numpy()
    seed = GC.seed_of(N, im, with_gains, with_models)
    rng = np.random.default_rng(seed + sensor_seed)
    ny = (8, 3, 1)[(N + B) % 3] if ny is None else ny
    S0, W = CR.random_psd(rng, shape=(B,)), rng.uniform(0.0, 1e-2, size=15)
    H, V = measurement(rng, ny)
    F, T = SR.blocks(N, ims, zo, th, evh)
    return types.SimpleNamespace(nlp=nlp, seed=seed, K=K, dK=dK, th=th, model=model, Zout=Zout, ev=ev, evh=evh, zo=zo, S0=S0, W=W,
                                 H=H, V=V, rng=rng, F=F, T=T)


# ---- the plumbing of the estimate-feedback sweeps ---------------------------------------------------------------------------
JVP_OUT = ("Zout_dot", "Xhat_dot", "innov_dot", "event_dot", "event_hat_dot")
VJP_OUT = ("Zref_bar", "K_bar", "Lgain_bar", "x0_bar", "xhat0_bar", "model_bar")


def upload(nlp, dirs):
    """Host tangents or cotangents on the device, the trajectory-shaped ones at the handle's stride"""
    return {k: (nlp.upload_Z(v) if k in ("Zref_dot", "Zbar") else dev(v)) for k, v in dirs.items()}


def present(inp, dirs, lgain=True):
    """The tangents that exist for these inputs: K_dot only with K; xhat0_dot exactly when xhat0 is given (None is the xhat0 =
    None case, whose tangent is Zref_dot's); Lgain_dot unless left out."""
    keep = lambda k: not ((k == "K_dot" and inp["K"] is None) or (k == "xhat0_dot" and inp["xhat0"] is None) or  # noqa: E731
                          (k == "Lgain_dot" and not lgain))
    return {k: v for k, v in dirs.items() if keep(k)}


def want(h, wx, lgain=True):
    """The reverse sweep's outputs that exist for these inputs, as present() names the tangents"""
    return tuple(w for w in ("Zref", "K", "Lgain", "x0", "xhat0", "model")
                 if not ((w == "K" and h["K"] is None) or (w == "xhat0" and not wx) or (w == "Lgain" and not lgain)))


def host(nlp, names, outs):
    """A sweep's outputs that are not None under their names, on the host; the trajectory-shaped ones as (B, n_nlp)"""
    return {n: (TC.rows(nlp, o) if n in ("Zout_dot", "Zref_bar") else o.cpu().numpy()) for n, o in zip(names, outs) if o is not None}
