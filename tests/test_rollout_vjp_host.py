"""CPU checks of the roll-out's reverse sweep: the numpy yardstick against complex-step differentiation of a whole numpy
closed-loop roll-out, the restored jump-knot clock row of the evaluator's blocks, argument validation that needs no device
and the ctypes table."""
import numpy as np
import pytest

from tests import rollout_vjp_ref as RV
from tests import tracking_ref as TR

CASES = [(2, 1, 1), (2, 2, 2), (2, 3, 1), (3, 2, 1), (5, 3, 2), (6, 4, 1), (6, 7, 2), (8, 5, 1)]


def _problem(N, k_trans, init_mode, seed):
    from quadruped_landing_amd import problem_gen as PG

    b = PG.make_batch(1, N, min(max(k_trans, 2), N - 1) if N > 2 else 2, init_mode, seed=seed)
    rng = np.random.default_rng(seed)
    Zref = b.Z[0].astype(np.float64)
    x0 = Zref[:15] + 1e-2 * rng.normal(size=15)
    K = 0.05 * rng.normal(size=(N - 1, 4, 15))
    Zbar = rng.normal(size=20 * N - 5)
    return Zref, K, x0, Zbar


@pytest.mark.parametrize("N,k_trans,init_mode", CASES)
@pytest.mark.parametrize("with_gains", [False, True])
def test_sweep_matches_complex_step_of_the_whole_rollout(N, k_trans, init_mode, with_gains):
    Zref, K, x0, Zbar = _problem(N, k_trans, init_mode, seed=10 * N + k_trans)
    K = K if with_gains else None
    Zout = RV.rollout(N, k_trans, init_mode, Zref, K, x0)
    F = RV.complex_step_blocks(N, k_trans, init_mode, Zout)
    zb, kb, xb = RV.sweep(F, Zref, K, Zout, Zbar)
    zc, kc, xc = RV.vjp_complex_step(N, k_trans, init_mode, Zref, K, x0, Zbar)
    assert RV.rel(zb, zc) <= 1e-12 and RV.rel(xb, xc) <= 1e-12, (RV.rel(zb, zc), RV.rel(xb, xc))
    assert np.all(zb[20 * (N - 1):] == 0.0) and np.all(zc[20 * (N - 1):] == 0.0)
    if with_gains:
        assert RV.rel(kb, kc) <= 1e-12, RV.rel(kb, kc)
    else:
        assert kb is None and np.all(zb[[20 * k + i for k in range(N - 1) for i in range(15)]] == 0.0)


@pytest.mark.parametrize("N,k_trans,init_mode", [(6, 4, 1), (8, 5, 2), (8, 2, 1)])
def test_restored_evaluator_blocks_are_the_true_step_derivative(N, k_trans, init_mode):
    from oracle import oracle as O

    Zref, K, x0, _ = _problem(N, k_trans, init_mode, seed=N)
    Zout = RV.rollout(N, k_trans, init_mode, Zref, K, x0)
    masked = np.zeros((N - 1, 15, 20))
    for k in range(N - 1):
        mode = init_mode if k + 1 <= k_trans - 1 else 3
        J = O.contact_jacobian(mode, Zout[20 * k: 20 * k + 15], Zout[20 * k + 15: 20 * k + 20], None)
        if k + 1 == k_trans - 1:
            J = J.copy()
            J[list(TR.JUMP_ROWS) + [14], :] = 0.0  # the evaluator's jump block, quirk Q1 included
        masked[k] = J
    kj = k_trans - 2
    assert masked[kj, 14, 14] == 0.0 and masked[kj, 14, 19] == 0.0
    F = RV.evaluator_blocks(masked, k_trans)
    C = RV.complex_step_blocks(N, k_trans, init_mode, Zout)
    assert np.abs(F - C).max() <= 1e-10 * max(1.0, np.abs(C).max())
    assert F[kj, 14, 14] == 1.0 and F[kj, 14, 19] == 1.0 and not F[kj, 14, :14].any()


def test_entry_points_reject_bad_arguments_without_a_device():
    from quadruped_landing_amd import _lib

    L = _lib.lib()
    z = np.zeros(100)
    k = np.zeros(60)
    for fn in (L.qln_tracking_rollout_vjp, L.qln_tracking_rollout_vjp_host):
        assert fn(None, z.ctypes.data, k.ctypes.data, z.ctypes.data, z.ctypes.data, None, None, None) == \
            _lib.QLN_ERR_INVALID_ARGUMENT
        assert fn(None, z.ctypes.data, None, z.ctypes.data, z.ctypes.data, None, k.ctypes.data, None) == \
            _lib.QLN_ERR_INVALID_ARGUMENT


def test_ctypes_table():
    import ctypes as C

    from quadruped_landing_amd import _lib

    for name in ("qln_tracking_rollout_vjp", "qln_tracking_rollout_vjp_host"):
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == 8
        assert getattr(_lib.lib(), name).argtypes == args
