"""CPU checks of the TVLQR tracking layer: the numpy Riccati against a dense KKT solve on oracle step blocks, argument
validation that needs no device, and the layouts of K and P."""
import ctypes as C

import numpy as np
import pytest

from tests import tracking_ref as TR

Q = np.array([10.0] * 14 + [0.5])
R = np.array([1e-3, 1e-2, 1e-3, 1e-2])
QF = np.array([20.0] * 14 + [1.0])


def _reference(N, k_trans, init_mode, seed):
    from quadruped_landing_amd import problem_gen as PG

    b = PG.make_batch(1, N, k_trans, init_mode, seed=seed)
    return b.Z[0]


@pytest.mark.parametrize("N,k_trans,init_mode", [(6, 3, 1), (12, 8, 2), (12, 11, 1)])
def test_riccati_matches_dense_kkt_for_every_unit_dx1(N, k_trans, init_mode):
    Z = _reference(N, k_trans, init_mode, seed=N)
    A, B = TR.oracle_blocks(N, k_trans, init_mode, Z)
    assert A[k_trans - 2, 14, 14] == 1.0 and np.all(A[k_trans - 2, 4] == 0.0)
    K, P = TR.riccati(A, B, Q, R, QF)
    for i in range(15):
        dx1 = np.zeros(15)
        dx1[i] = 1.0
        du, dx, J = TR.kkt(A, B, Q, R, QF, dx1)
        np.testing.assert_allclose(-K[0] @ dx1, du[0], rtol=1e-9, atol=1e-9 * max(1.0, np.abs(du).max()))
        du_cl, dx_cl = TR.closed_loop(A, B, K, dx1)
        np.testing.assert_allclose(du_cl, du, rtol=1e-8, atol=1e-9 * max(1.0, np.abs(du).max()))
        Jp = dx1 @ P[0] @ dx1
        assert abs(Jp - J) <= 1e-10 * abs(J), (i, Jp, J)
        assert abs(TR.lq_cost(dx_cl, du_cl, Q, R, QF) - J) <= 1e-9 * abs(J)


def test_entry_points_reject_a_null_handle_without_a_device():
    from quadruped_landing_amd import _lib

    L = _lib.lib()
    w = np.ones(15)
    r = np.ones(4)
    z = np.zeros(100)
    assert L.qln_tracking_lqr(None, z.ctypes.data, w.ctypes.data, r.ctypes.data, w.ctypes.data, z.ctypes.data, None) == \
        _lib.QLN_ERR_INVALID_ARGUMENT
    assert L.qln_tracking_rollout(None, z.ctypes.data, None, None, z.ctypes.data) == _lib.QLN_ERR_INVALID_ARGUMENT
    assert L.qln_tracking_lqr_host(None, z.ctypes.data, w.ctypes.data, r.ctypes.data, w.ctypes.data, z.ctypes.data,
                                   None) == _lib.QLN_ERR_INVALID_ARGUMENT
    assert L.qln_tracking_rollout_host(None, z.ctypes.data, None, None, z.ctypes.data) == _lib.QLN_ERR_INVALID_ARGUMENT


def test_weights_broadcast_and_shapes():
    from quadruped_landing_amd import nlp

    Qh, Rh, Qfh = nlp.tracking_weights(1.0, [1, 2, 3, 4], np.arange(15))
    assert Qh.shape == (15,) and Rh.shape == (4,) and Qfh.shape == (15,) and Rh.dtype == np.float64
    with pytest.raises(ValueError):
        nlp.tracking_weights(np.ones(14), 1.0, 1.0)
    assert nlp.tracking_k_shape(7, 40) == (7, 39, 4, 15)
    assert nlp.tracking_p_shape(7, 40) == (7, 40, 120)


def test_packed_cost_to_go_layout():
    from quadruped_landing_amd import nlp

    rng = np.random.default_rng(0)
    M = rng.normal(size=(3, 2, 15, 15))
    M = M + np.swapaxes(M, -1, -2)
    packed = np.zeros((3, 2, 120))
    for i in range(15):
        for j in range(i + 1):
            packed[..., i * (i + 1) // 2 + j] = M[..., i, j]
    np.testing.assert_array_equal(nlp.unpack_cost_to_go(packed), M)
