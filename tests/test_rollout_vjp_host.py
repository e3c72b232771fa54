"""CPU checks of the roll-out's reverse sweep: the numpy yardstick against complex-step differentiation of a whole numpy
closed-loop roll-out, the restored jump-knot clock row of the evaluator's blocks, argument validation that needs no device
and the ctypes table."""
import numpy as np
import pytest

from tests import rollout_ref as RR
from tests import tracking_cases as TC
from tests import tracking_ref as TR
from tests.tracking_cases import CASES


@pytest.mark.parametrize("N,k_trans,init_mode", CASES)
@pytest.mark.parametrize("with_gains", [False, True])
def test_sweep_matches_complex_step_of_the_whole_rollout(N, k_trans, init_mode, with_gains):
    Zref, K, x0, Zbar = TC.problem(N, k_trans, init_mode, seed=10 * N + k_trans)
    K = K if with_gains else None
    Zout = RR.rollout(N, k_trans, init_mode, Zref, K, x0)
    F = RR.complex_step_blocks(N, k_trans, init_mode, Zout)
    zb, kb, xb, _ = RR.sweep_vjp(F, Zref, K, Zout, Zbar)
    zc, kc, xc = RR.vjp_complex_step(N, k_trans, init_mode, Zref, K, x0, Zbar)
    assert RR.rel(zb, zc) <= 1e-12 and RR.rel(xb, xc) <= 1e-12, (RR.rel(zb, zc), RR.rel(xb, xc))
    assert np.all(zb[20 * (N - 1):] == 0.0) and np.all(zc[20 * (N - 1):] == 0.0)
    if with_gains:
        assert RR.rel(kb, kc) <= 1e-12, RR.rel(kb, kc)
    else:
        assert kb is None and np.all(zb[[20 * k + i for k in range(N - 1) for i in range(15)]] == 0.0)


@pytest.mark.parametrize("N,k_trans,init_mode", [(6, 4, 1), (8, 5, 2), (8, 2, 1)])
def test_restored_evaluator_blocks_are_the_true_step_derivative(N, k_trans, init_mode):
    from oracle import oracle as O

    Zref, K, x0, _ = TC.problem(N, k_trans, init_mode, seed=N)
    Zout = RR.rollout(N, k_trans, init_mode, Zref, K, x0)
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
    F = RR.evaluator_blocks(masked, k_trans)
    C = RR.complex_step_blocks(N, k_trans, init_mode, Zout)
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
