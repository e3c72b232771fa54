"""The multiplier estimate without a GPU: the numpy restatement (tests/multiplier_ref.py) that the GPU tests hold the
kernel to is itself held to numpy.linalg.lstsq on the oracle's Jacobian; its bounds are the library's
qln_variable_bounds; the C entry points validate their arguments without a device.

N = 2 and N = 3 are not compared with lstsq at convergence: there lstsq resolves singular directions that CGLS has not
reached at rel_tol = 1e-9 (the two differ by the whole residual, 5e-6, measured with this restatement); those sizes are
covered by the iterate tests on the GPU.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from quadruped_landing_amd import _lib, problem_gen as PG, split_bound_multipliers, variable_bounds
from tests import multiplier_ref as MR
from tests.helpers import oracle_model

CASES = [(12, 5), (17, 6)]


def _problems(N, kt, B=2):
    batch = PG.make_batch(B, N, kt, 1, seed=N)
    for b in range(B):
        o = O.OracleNLP(N, kt, 1, batch.x0[b], batch.xf[b], batch.obj, oracle_model(batch.model))
        Z = batch.Z[b]
        yield Z, o.eval_c(Z), o.grad_f(Z), MR.oracle_jacobian(o, Z)


@pytest.mark.parametrize("N,kt", CASES)
@pytest.mark.parametrize("row_scaling", [False, True])
def test_converged_restatement_agrees_with_lstsq(N, kt, row_scaling):
    for Z, c, g, J in _problems(N, kt):
        A, free, w, T = MR.operator(J, Z, c, N, row_scaling=row_scaling)
        assert (free == 0).sum() > 0  # make_batch clips h to its bounds: the fixed-variable branch is met
        lam, lag, info = MR.estimate(J, Z, c, g, N, row_scaling=row_scaling, max_iters=50000, rel_tol=1e-9)
        assert info[0] < 50000
        y_ls, res_ls = MR.lstsq_residual(T, free * g)
        res = free * lag  # the residual vector T y + D g, formed from lam and not from the recurrence
        gmax = np.abs(g).max()
        err = np.abs(res - res_ls).max()
        print(f"N={N} scaling={row_scaling}: {int(info[0])} iterations, |res - res_lstsq| = {err:.3e}, max|g| = {gmax:.3e}")
        assert err <= 1e-6 * gmax
        assert abs(info[4] - np.abs(res).max()) == 0.0
        if not row_scaling:
            lerr = np.abs(lam - y_ls).max() / np.abs(y_ls).max()
            print(f"   lam rel err {lerr:.3e}")
            assert lerr <= 1e-5


@pytest.mark.parametrize("N", [2, 3, 12])
def test_restatement_bounds_are_the_librarys(N):
    L = _lib.lib()
    n = 20 * N - 5
    xl, xu = np.zeros(n), np.zeros(n)
    _lib.check(L.qln_variable_bounds(N, None, xl.ctypes.data, xu.ctypes.data))
    wl, wu = MR.bounds(N)
    assert np.array_equal(xl, wl) and np.array_equal(xu, wu)
    assert np.array_equal(wl, variable_bounds(N)[0]) and np.array_equal(wu, variable_bounds(N)[1])
    opt = _lib.QlnSolveOptions()
    _lib.check(L.qln_solve_default_options(C.byref(opt)))
    opt.q6_bounds, opt.h_min, opt.h_max, opt.theta_min, opt.theta_max = 0, 0.002, 0.05, -1.0, 1.25
    _lib.check(L.qln_variable_bounds(N, C.byref(opt), xl.ctypes.data, xu.ctypes.data))
    wl, wu = MR.bounds(N, h_min=0.002, h_max=0.05, theta_min=-1.0, theta_max=1.25, q6_bounds=False)
    assert np.array_equal(xl, wl) and np.array_equal(xu, wu)


def test_info_counts_of_the_restatement_on_a_hand_made_active_set():
    """Three clearance rows made active by hand (one through a NaN): the counts, and the exact zeros of lam elsewhere."""
    N = 12
    for Z, c, g, J in _problems(N, 5, B=1):
        c = c.copy()
        c[-N:] = 1.0
        c[-3:] = [0.0, -0.1, np.nan]  # three active clearance rows, the NaN one included
        lam, lag, info = MR.estimate(J, Z, c, g, N, max_iters=3, rel_tol=0.0)
        assert info[0] == 3 and info[5] == 3
        assert np.all(lam[-N:-3] == 0.0)
        x_l, x_u = variable_bounds(N)
        fixed = (Z <= x_l + 1e-8) | (Z >= x_u - 1e-8)
        assert info[6] == fixed.sum() > 0
        _, _, info_none = MR.estimate(J, Z, c, g, N, max_iters=3, rel_tol=0.0, bound_tol=-1.0)
        assert info_none[6] == 0 and info_none[8] == 0


def test_split_bound_multipliers():
    N = 3
    x_l, x_u = variable_bounds(N)
    Z = np.zeros(20 * N - 5)
    Z[19] = 0.001   # h_1 on its lower bound
    Z[39] = 0.02    # h_2 on its upper bound
    Z[2] = 0.3      # theta free
    Z[21] = 0.5     # yb_2 off quirk Q6's bound; x1_2 = Z[23] = 0 on it
    Z[41] = Z[43] = 0.5
    lag = np.arange(1.0, Z.size + 1)
    lag[39] = -7.0
    lag[23] = -2.0  # the wrong sign at a lower bound
    zL, zU = split_bound_multipliers(lag, Z)
    assert zL[19] == 20.0 and zU[19] == 0.0
    assert zU[39] == 7.0 and zL[39] == 0.0
    assert zL[23] == 0.0 and zU[23] == 0.0
    assert zL[2] == 0.0 and zL[21] == 0.0
    assert np.all(zL >= 0) and np.all(zU >= 0)
    assert np.count_nonzero(zL) + np.count_nonzero(zU) == 2
    zL, zU = split_bound_multipliers(lag, Z, bound_tol=-1.0)
    assert not zL.any() and not zU.any()
    # batched input
    zL, zU = split_bound_multipliers(np.stack([lag, lag]), np.stack([Z, Z]))
    assert zL.shape == (2, Z.size) and zL[1, 19] == 20.0


@pytest.mark.parametrize("name", ["qln_estimate_multipliers", "qln_estimate_multipliers_host"])
def test_argument_validation_with_a_null_handle(name):
    L = _lib.lib()
    a = np.zeros(64)
    p = a.ctypes.data
    fn = getattr(L, name)
    assert fn(None, p, p, p, None, 1e-6, 1e-8, 1, 10, 1e-8, p, p, p) == _lib.QLN_ERR_INVALID_ARGUMENT
    assert b"null handle" in L.qln_last_error()
    assert _lib.MULT_INFO_STRIDE == MR.INFO_STRIDE == 16
