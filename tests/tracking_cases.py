"""What the tests of the tracking family share -- the gains, the closed-loop roll-out, its two sweeps with and without a
per-problem plant model, and the covariance sweep, on the CPU and on the GPU: the shapes and host cases, the weights, the
second robot model, and the helpers that build a batch, a handle, the inputs and tangents of a call and the step blocks the
numpy yardsticks run on.  One statement, so that every test module of the family sees the same inputs.  Not a test module:
torch and the library are imported inside the functions that need them."""
import numpy as np

from quadruped_landing_amd.planar_quadruped import PlanarQuadruped
from tests import rollout_ref as RR
from tests import tracking_cov_ref as CR
from tests import tracking_ref as TR

Q = np.array([10.0] * 14 + [0.0])
R = np.array([1e-3, 1e-2, 1e-3, 1e-2])
QW = np.array([10.0] * 14 + [0.7])
QFW = np.array([30.0] * 14 + [2.0])

# Without the coincidences of PlanarQuadruped()'s defaults (1/mb == mf, lb*lb == lb/2 == l1 == l2: tests/test_model_host.py)
SECOND_MODEL = PlanarQuadruped(g=-9.1, mb=8.7, mf=0.13, lb=0.46, l1=0.27, l2=0.22)
SECOND = np.array(SECOND_MODEL.plant_parameters())  # (g, mb, mf, lb), a row of a per-problem plant model

SHAPES = [  # (B, N, k_trans, init_mode): tests/test_gpu_hessian.py's list
    (3, 2, 1, 1), (3, 2, 2, 2), (3, 2, 3, 1), (5, 3, 2, 1), (5, 3, 3, 2), (5, 3, 4, 1),
    (9, 40, 14, 1), (9, 40, 1, 2), (9, 40, 39, 1), (9, 40, 40, 2), (9, 40, 41, 1),
    (17, 61, 21, 1), (17, 61, 60, 2), (10, 65, 64, 1), (10, 65, 65, 2), (10, 65, 2, 1),
    (11, 80, 66, 2), (11, 80, 10, 1), (4, 200, 130, 1), (4, 200, 201, 2),
]

CASES = [(2, 1, 1), (2, 2, 2), (2, 3, 1), (3, 2, 1), (5, 3, 2), (6, 4, 1), (6, 7, 2), (8, 5, 1)]  # (N, k_trans, init_mode)


def problem(N, k_trans, init_mode, seed):
    """One host problem of CASES: a reference, gains, x0 near the reference's x_0 and a random cotangent."""
    from quadruped_landing_amd import problem_gen as PG

    b = PG.make_batch(1, N, min(max(k_trans, 2), N - 1) if N > 2 else 2, init_mode, seed=seed)
    rng = np.random.default_rng(seed)
    Zref = b.Z[0].astype(np.float64)
    x0 = Zref[:15] + 1e-2 * rng.normal(size=15)
    K = 0.05 * rng.normal(size=(N - 1, 4, 15))
    Zbar = rng.normal(size=20 * N - 5)
    return Zref, K, x0, Zbar


def batch(B, N, k_trans, init_mode, seed=0, ragged=False):
    from quadruped_landing_amd import problem_gen as PG

    kt_build = min(max(int(k_trans), 2), N - 1) if N > 2 else 2
    b = PG.make_batch(B, N, kt_build, init_mode, seed=seed, ragged=ragged)
    if not ragged:
        b.k_trans[:] = k_trans
    return b


def nlp(batch, model=None, **kw):
    """A handle on the batch; its (design) model is the batch's unless one is given."""
    from quadruped_landing_amd import HybridNLP

    return HybridNLP(batch.model if model is None else model, batch.obj, batch.init_mode, batch.k_trans, batch.N, batch.x0,
                     batch.xf, **kw)


def dense_blocks(nlp, Z):
    import torch

    vals = nlp.jac_c(Z).cpu().numpy()
    N = nlp.N
    out = np.zeros((nlp.B, N - 1, 15, 20))
    for b in range(nlp.B):
        seg = vals[nlp.j_off[b]: nlp.j_off[b] + 300 * (N - 1)]
        out[b] = seg.reshape(N - 1, 20, 15).transpose(0, 2, 1)
    torch.cuda.synchronize()
    return out


def gains(nlp, seed, scale=0.05):
    import torch

    rng = np.random.default_rng(seed)
    return torch.from_numpy(scale * rng.normal(size=(nlp.B, nlp.N - 1, 4, 15))).cuda()


def inputs(nlp, batch, seed, with_gains, model=None):
    """A reference, gains (or None), x0 near the reference's x_0, the GPU roll-out (under the per-problem models, if given)
    and a random cotangent."""
    import torch

    rng = np.random.default_rng(seed)
    Zref = nlp.upload_Z(batch.Z)
    K = gains(nlp, seed + 1) if with_gains else None
    x0 = torch.from_numpy(batch.Z[:, :15] + 1e-2 * rng.normal(size=(nlp.B, 15))).cuda()
    Zout = nlp.tracking_rollout(Zref, K, x0) if model is None else nlp.tracking_rollout_model(Zref, K, x0, model)
    Zbar = nlp.upload_Z(rng.normal(size=(nlp.B, nlp.n_nlp)))
    return Zref, K, x0, Zout, Zbar


def tangents(nlp, seed, with_gains, scale=(1.0, 1.0, 1.0, 1.0), model=None):
    """Random tangents of Zref (zero past n_nlp), K (None without gains) and x0, as device tensors; with per-problem models,
    a fourth of the models, relative to each parameter's size."""
    import torch

    rng = np.random.default_rng(seed)
    zd = nlp.upload_Z(scale[0] * rng.normal(size=(nlp.B, nlp.n_nlp)))
    kd = torch.from_numpy(scale[1] * rng.normal(size=(nlp.B, nlp.N - 1, 4, 15))).cuda() if with_gains else None
    xd = torch.from_numpy(scale[2] * rng.normal(size=(nlp.B, 15))).cuda()
    if model is None:
        return zd, kd, xd
    return zd, kd, xd, model * torch.from_numpy(scale[3] * rng.normal(size=(nlp.B, 4))).cuda()


def rows(nlp, t):
    """The first n_nlp entries of every problem, on the host: (B, n_nlp)."""
    return t.view(nlp.B, -1)[:, :nlp.n_nlp].cpu().numpy()


def to_np(t):
    return None if t is None else t.cpu().numpy()


def evaluator_blocks(nlp, Zout):
    dense = dense_blocks(nlp, Zout)
    return lambda b, zo: RR.evaluator_blocks(dense[b], int(nlp.k_trans[b]))


def cs_blocks(nlp):
    return lambda b, zo: RR.complex_step_blocks(nlp.N, int(nlp.k_trans[b]), int(nlp.init_mode[b]), zo)


def vjp_per_problem(nlp, Zref, K, Zout, Zbar, zb, kb, xb, blocks):
    """worst per-problem relative norm of (Zref_bar, K_bar, x0_bar) against the numpy sweep on blocks(b, Zout_b)"""
    zr, zo, zbar, zg = rows(nlp, Zref), rows(nlp, Zout), rows(nlp, Zbar), rows(nlp, zb)
    Kh, kg, xg = to_np(K), to_np(kb), to_np(xb)
    worst = 0.0
    for b in range(nlp.B):
        r_z, r_k, r_x, _ = RR.sweep_vjp(blocks(b, zo[b]), zr[b], None if Kh is None else Kh[b], zo[b], zbar[b])
        e = [RR.rel(zg[b], r_z), RR.rel(xg[b], r_x)] + ([] if kg is None else [RR.rel(kg[b], r_k)])
        worst = max(worst, *e)
    return worst


def jvp_per_problem(nlp, Zref, K, Zout, zd, kd, xd, got, blocks):
    """worst per-problem relative norm of Zout_dot against the numpy sweep on blocks(b, Zout_b)"""
    zr, zo, g = rows(nlp, Zref), rows(nlp, Zout), rows(nlp, got)
    zdh = None if zd is None else rows(nlp, zd)
    Kh, kdh, xdh = to_np(K), to_np(kd), to_np(xd)
    worst = 0.0
    for b in range(nlp.B):
        ref = RR.sweep_jvp(blocks(b, zo[b]), zr[b], None if Kh is None else Kh[b], zo[b], None if zdh is None else zdh[b],
                           None if kdh is None else kdh[b], None if xdh is None else xdh[b])
        worst = max(worst, RR.rel(g[b], ref))
    return worst


def ref_gains(nlp, Z, Qw, Rw, Qfw, restore_clock=True):
    blocks = dense_blocks(nlp, Z)
    A = np.zeros((nlp.B, nlp.N - 1, 15, 15))
    Bm = np.zeros((nlp.B, nlp.N - 1, 15, 4))
    for b in range(nlp.B):
        A[b], Bm[b] = TR.blocks_from_dense(blocks[b], int(nlp.k_trans[b]), restore_clock)
    K, P = TR.riccati(A, Bm, Qw, Rw, Qfw)
    return A, Bm, K, P


def check_gains_against_numpy(batch, bar=1e-10, weights=None, **kw):
    """weights: (Qdiag, Rdiag, Qfdiag) in place of (QW, R, QFW)"""
    from quadruped_landing_amd import nlp as NL

    Qw, Rw, Qfw = (QW, R, QFW) if weights is None else weights
    h = nlp(batch, **kw)
    Z = h.upload_Z(batch.Z)
    K, P = h.tracking_lqr(Z, Qw, Rw, Qfw)
    _, _, Kr, Pr = ref_gains(h, Z, Qw, Rw, Qfw)
    Kg = K.cpu().numpy()
    Pg = NL.unpack_cost_to_go(P)
    ek, ep = CR.knot_rel(Kg, Kr), CR.knot_rel(Pg, Pr)
    assert ek <= bar and ep <= bar, (ek, ep)
    assert np.array_equal(Pg, np.swapaxes(Pg, -1, -2))
    return ek, ep


def cov_setup(batch, seed, with_gains, **kw):
    """A handle, a roll-out Zout near the batch's Z under random gains (or open loop), per-problem random Sigma0 and W."""
    h = nlp(batch, **kw)
    _, K, _, Zout, _ = inputs(h, batch, seed, with_gains)
    rng = np.random.default_rng(seed + 100)
    S0 = CR.random_psd(rng, shape=(h.B,))
    W = rng.uniform(0.0, 1e-2, size=15)
    return h, K, Zout, S0, W


def cov_reference(nlp, K, Zout, S0, W, blocks):
    """numpy (Sigma (B, N, 15, 15), marg (B, N, 8)) on blocks(b, zo) (N-1, 15, 20) per problem"""
    zo = rows(nlp, Zout)
    Kh = to_np(K)
    N = nlp.N
    Sr = np.zeros((nlp.B, N, 15, 15))
    mr = np.zeros((nlp.B, N, 8))
    for b in range(nlp.B):
        F = blocks(b, zo[b])
        Sr[b] = CR.propagate(F[:, :, :15], F[:, :, 15:19], None if Kh is None else Kh[b], S0[b] if S0.ndim == 3 else S0, W)
        theta = zo[b][2 + 20 * np.arange(N)]
        mr[b] = CR.marginals(Sr[b], None if Kh is None else Kh[b], theta, nlp.model.lb)
    return Sr, mr


def cov_errors(nlp, K, Zout, S0, W, blocks):
    from quadruped_landing_amd import nlp as NL

    S, mg = nlp.tracking_covariance(Zout, K, S0, W)
    Sg, mgg = NL.unpack_covariance(S), mg.cpu().numpy()
    assert np.array_equal(Sg, np.swapaxes(Sg, -1, -2))
    Sr, mr = cov_reference(nlp, K, Zout, S0, W, blocks)
    if K is None:
        assert not mgg[:, :, 1:5].any()
    assert not mgg[:, -1, 1:5].any()
    return CR.knot_rel(Sg, Sr), CR.entry_rel(mgg, mr)
