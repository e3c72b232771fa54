"""numpy yardstick of qln_tracking_rollout_jvp (include/qln_evaluator.h): the forward (tangent) sweep of the closed-loop
roll-out on dense 15x20 step blocks -- the blocks of tests/rollout_vjp_ref.py (evaluator_blocks or complex_step_blocks) --
and the same derivative by complex step of the whole numpy roll-out."""
import numpy as np

from tests import rollout_vjp_ref as RV

NX, NU = 15, 4


def sweep(F, Zref, K, Zout, Zref_dot=None, K_dot=None, x0_dot=None):
    """The header's forward sweep on blocks F (N-1, 15, 20) for one problem (vectors of length n_nlp, K and K_dot
    (N-1, 4, 15), x0_dot (15,); a tangent that is None is zero): returns Zout_dot (n_nlp,)."""
    n1 = len(F)
    N = n1 + 1
    Zref, Zout = np.asarray(Zref, dtype=np.float64), np.asarray(Zout, dtype=np.float64)
    zd = np.zeros(20 * N - 5) if Zref_dot is None else np.asarray(Zref_dot, dtype=np.float64)
    out = np.zeros(20 * N - 5)
    dx = np.zeros(NX) if x0_dot is None else np.array(x0_dot, dtype=np.float64)
    for k in range(n1):
        du = zd[20 * k + 15: 20 * k + 20].copy()
        if K is not None:
            du[:4] -= K[k] @ (dx - zd[20 * k: 20 * k + 15])
            if K_dot is not None:
                du[:4] -= K_dot[k] @ (Zout[20 * k: 20 * k + 15] - Zref[20 * k: 20 * k + 15])
        out[20 * k: 20 * k + 15] = dx
        out[20 * k + 15: 20 * k + 20] = du
        dx = F[k, :, :15] @ dx + F[k, :, 15:] @ du
    out[20 * n1:] = dx
    return out


def sweep_batch(F, Zref, K, Zout, Zref_dot, K_dot, x0_dot):
    """sweep vectorised over a batch: F (B, N-1, 15, 20), Z-like (B, n_nlp), K and K_dot (B, N-1, 4, 15), x0_dot (B, 15);
    all three tangents given."""
    nb, n1 = F.shape[:2]
    out = np.zeros_like(Zout)
    dx = x0_dot.copy()
    for k in range(n1):
        xs, us = slice(20 * k, 20 * k + 15), slice(20 * k + 15, 20 * k + 20)
        du = Zref_dot[:, us].copy()
        du[:, :4] -= np.einsum("bmj,bj->bm", K[:, k], dx - Zref_dot[:, xs])
        du[:, :4] -= np.einsum("bmj,bj->bm", K_dot[:, k], Zout[:, xs] - Zref[:, xs])
        out[:, xs] = dx
        out[:, us] = du
        dx = np.einsum("bij,bj->bi", F[:, k, :, :15], dx) + np.einsum("bij,bj->bi", F[:, k, :, 15:], du)
    out[:, 20 * n1:] = dx
    return out


def jvp_complex_step(N, k_trans, init_mode, Zref, K, x0, Zref_dot=None, K_dot=None, x0_dot=None, eps=1e-30):
    """d/dt rollout(Zref + t Zref_dot, K + t K_dot, x0 + t x0_dot) at t = 0 by complex step: one complex roll-out."""
    zr = np.asarray(Zref, dtype=np.complex128)
    xx = np.asarray(x0, dtype=np.complex128)
    kk = None if K is None else np.asarray(K, dtype=np.complex128)
    if Zref_dot is not None:
        zr = zr + 1j * eps * np.asarray(Zref_dot)
    if K_dot is not None:
        kk = kk + 1j * eps * np.asarray(K_dot)
    if x0_dot is not None:
        xx = xx + 1j * eps * np.asarray(x0_dot)
    return RV.rollout(N, k_trans, init_mode, zr, kk, xx).imag / eps
