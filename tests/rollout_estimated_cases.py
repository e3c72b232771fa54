"""What the CPU and the GPU tests of the estimate-feedback roll-out (qln_tracking_rollout_estimated / _guarded) share: the
random inputs of a case, the Monte Carlo experiment's settings, draws and statistics, so that the seeds checked on the CPU are
the ones the GPU runs.  Not a test module."""
import os

import numpy as np

from tests import tracking_cases as TC
from tests import tracking_cov_ref as CR

NYS = (1, 3, 8)


def draws(seed, B, N, ny, scale_l=0.01, scale_v=1e-3, scale_w=1e-4):
    """Random inputs of one comparison: Lgain (B, N, 15, ny) and H (ny, 15) -- draws, not designed gains, so that a misindexed
    tile cannot hide behind structure -- and vnoise (B, N, ny), wnoise (B, N-1, 15), xhat0 offsets (B, 15).  The scales keep the
    random loop bounded over 60 knots (the body's pitch is unstable open loop, e^15 over 0.6 s): at 0.05 / 1e-2 / 1e-3 the
    estimate of an N = 61 case overflows, at these every state stays below 1e3 and the float64 yardstick is within 3e-14 of its
    longdouble restatement, while a filter gain still moves the estimate by 1e-5 of its size, five orders above the bar."""
    rng = np.random.default_rng(seed)
    return dict(Lgain=scale_l * rng.normal(size=(B, N, 15, ny)), H=rng.normal(size=(ny, 15)) / np.sqrt(15.0),
                vnoise=scale_v * rng.normal(size=(B, N, ny)), wnoise=scale_w * rng.normal(size=(B, N - 1, 15)),
                dxhat0=1e-2 * rng.normal(size=(B, 15)))


# ---- the Monte Carlo experiment ------------------------------------------------------------------------------------------
MC_S = 4096
MC_DIRECTIONS = 32
MC_HEIGHT = 0.02          # the guarded experiment drops the free foot this much higher than planned
MC_W = np.array([1e-10] * 14 + [0.0])
# (sensor sd, process noise or None, seed)
MC_SETTINGS = [(1e-3, MC_W, 2024), (1e-4, None, 2025), (1e-2, MC_W, 2026)]


def band(S=MC_S):
    """A variance estimated from S normal samples has relative standard deviation sqrt(2 / (S - 1)): five of them."""
    return 5.0 * np.sqrt(2.0 / (S - 1))


def sensors():
    """The eight rows of examples/estimate_landing.py: body pose x[0..2], gyro x[9], the feet relative to the body."""
    H = np.zeros((8, 15))
    for r, i in enumerate((0, 1, 2, 9)):
        H[r, i] = 1.0
    for r, (foot, body) in enumerate(((3, 0), (4, 1), (5, 0), (6, 1)), start=4):
        H[r, foot], H[r, body] = 1.0, -1.0
    return H


def notebook():
    """The notebook problem at the reference's own solution tests/golden/data_6.csv: (batch of one with Z the file's)."""
    from quadruped_landing_amd import problem_gen as PG

    nb = PG.notebook_problem()
    nb.Z = np.loadtxt(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data_6.csv"))[None, :]
    return nb


def mc_draws(seed, N, sd, W, S=MC_S):
    """Sigma_0 = 1e-8 (G G'/15 + 0.1 I) as tests/test_gpu_tracking_cov.py's experiment, and the samples: dx0 (S, 15) ~ N(0,
    Sigma_0), vnoise (S, N, 8) of standard deviation sd, wnoise (S, N-1, 15) of variance W (None: none), and the directions
    (32, 15) and (32, 8) the covariances are probed along."""
    rng = np.random.default_rng(seed)
    S0 = 1e-8 * (CR.random_psd(rng) + 0.1 * np.eye(15))
    dx0 = rng.normal(size=(S, 15)) @ np.linalg.cholesky(S0).T
    v = sd * rng.normal(size=(S, N, 8))
    w = None if W is None else np.sqrt(W) * rng.normal(size=(S, N - 1, 15))
    return S0, dx0, v, w, rng.normal(size=(MC_DIRECTIONS, 15)), rng.normal(size=(MC_DIRECTIONS, 8))


def mc_worst(zout, xhat, innov, znom, X, Pp, Sk, Wx, Wy):
    """The worst |ratio - 1| over all knots and directions, of the sample variance over the predicted one, for the true state
    (zout - znom against X_k), the estimation error (zout - xhat against P^+_k) and the innovation (against S_k).  zout (S, n),
    xhat (S, N, 15), innov (S, N, ny), znom (n,); X, Pp (N, 15, 15), Sk (N, ny, ny)."""
    S, N = xhat.shape[0], xhat.shape[1]
    z = np.concatenate([zout, np.zeros((S, 5))], axis=1).reshape(S, N, 20)[:, :, :15]
    zn = np.concatenate([znom, np.zeros(5)]).reshape(N, 20)[:, :15]
    worst = {}
    for name, smp, cov, D in (("X", z - zn, X, Wx), ("P+", z - xhat, Pp, Wx), ("S", innov, Sk, Wy)):
        proj = np.einsum("skd,wd->skw", smp, D)                      # (S, N, 32)
        var = proj.var(axis=0, ddof=1)                               # (N, 32)
        pred = np.einsum("wd,kde,we->kw", D, cov, D)
        worst[name] = float(np.abs(var / pred - 1.0).max())
    return worst


def innovation_covariances(Pm, H, V):
    """S_k = H P^-_k H' + diag(V), (N, ny, ny)."""
    return np.einsum("rd,kde,se->krs", H, Pm, H) + np.diag(V)


def handle_pair(nb, S):
    """(a handle on the one notebook problem, a handle on S copies of it)"""
    rep = lambda a: np.repeat(np.asarray(a), S, axis=0)  # noqa: E731
    from quadruped_landing_amd import HybridNLP

    one = HybridNLP(nb.model, nb.obj, nb.init_mode, nb.k_trans, nb.N, nb.x0, nb.xf)
    many = HybridNLP(nb.model, nb.obj, rep(nb.init_mode), rep(nb.k_trans), nb.N, rep(nb.x0), rep(nb.xf))
    return one, many


Q, R = TC.Q, TC.R
