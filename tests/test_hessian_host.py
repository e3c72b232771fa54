"""The Lagrangian Hessian without a GPU: its layout and structure (qln_hessian_layout / qln_hessian_structure), the exact
step-block pattern against a symbolic expansion of oracle/np_oracle.py, argument validation, and the MOI surface."""
import ctypes as C

import numpy as np
import pytest

from quadruped_landing_amd import _lib, moi
from quadruped_landing_amd.nlp import hessian_structure
from tests import hessian_sym as HS

NS = (2, 3, 40, 61, 65, 200)


def _layout(N, align):
    d = _lib.QlnBatchDesc()
    d.B, d.N, d.align = 3, N, align
    nnz, stride = C.c_int32(), C.c_int64()
    rc = _lib.lib().qln_hessian_layout(C.byref(d), C.byref(nnz), C.byref(stride))
    return rc, nnz.value, stride.value


@pytest.mark.parametrize("N", NS)
def test_structure_is_block_diagonal_lower_and_column_major(N):
    rows, cols = hessian_structure(N)
    assert rows.size == 55 * (N - 1) + 15
    assert np.all(rows >= cols) and rows.min() >= 0 and rows.max() < 20 * N - 5
    assert len(set(zip(rows.tolist(), cols.tolist()))) == rows.size  # no duplicates
    steps_r = rows[: 55 * (N - 1)].reshape(N - 1, 55)
    steps_c = cols[: 55 * (N - 1)].reshape(N - 1, 55)
    base = 20 * np.arange(N - 1)[:, None]
    # every block is the same local pattern shifted to its knot: block-diagonal
    assert np.array_equal(steps_r - base, np.broadcast_to(steps_r[0], steps_r.shape))
    assert np.array_equal(steps_c - base, np.broadcast_to(steps_c[0], steps_c.shape))
    r0, c0 = steps_r[0], steps_c[0]
    assert r0.max() < 20 and c0.max() < 20
    assert list(zip(c0.tolist(), r0.tolist())) == sorted(zip(c0.tolist(), r0.tolist()))  # column-major
    term = 20 * (N - 1) + np.arange(15)
    assert np.array_equal(rows[55 * (N - 1):], term) and np.array_equal(cols[55 * (N - 1):], term)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("align", [0, 1, 2, 3, 16, 32])
def test_layout_honours_align(N, align):
    rc, nnz, stride = _layout(N, align)
    assert rc == _lib.QLN_OK
    assert nnz == 55 * (N - 1) + 15
    a = align or 16
    assert stride >= nnz and stride % a == 0 and stride - nnz < a


def test_step_pattern_is_exactly_the_symbolic_union():
    """sigma h stagecost + mu . M rk4 (+ the clearance curvature at (theta, theta)), expanded for modes 1/2/3 with and
    without the jump mask: the union of the entries that are not identically zero IS the library's 55-entry pattern."""
    rows, cols = hessian_structure(2)
    lib_block = list(zip(rows[:55].tolist(), cols[:55].tolist()))
    assert lib_block == HS.step_pattern()
    assert len(lib_block) == _lib.HESS_STEP_NNZ == 55
    # the dynamics part alone: 34 entries, no force x force and no theta-coupled term
    dyn = set()
    for mode, jump in HS.CASES:
        for (r, c), e in HS.lagrangian_hessian(mode, jump).items():
            if e.subs(HS.SIGMA, 0) != 0:
                dyn.add((r, c))
    assert len(dyn) == 34
    assert not any(15 <= r < 19 and 15 <= c < 19 for r, c in dyn)
    assert not any(2 in (r, c) for r, c in dyn)


def test_argument_validation_needs_no_gpu():
    L = _lib.lib()
    rows = np.zeros(100, dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    assert L.qln_hessian_structure(1, rows.ctypes.data_as(ip), rows.ctypes.data_as(ip)) == _lib.QLN_ERR_INVALID_ARGUMENT
    assert b"N must be >= 2" in L.qln_last_error()
    assert L.qln_hessian_structure(2, None, rows.ctypes.data_as(ip)) == _lib.QLN_ERR_INVALID_ARGUMENT
    assert b"null" in L.qln_last_error()
    nnz, stride = C.c_int32(), C.c_int64()
    assert L.qln_hessian_layout(None, C.byref(nnz), C.byref(stride)) == _lib.QLN_ERR_INVALID_ARGUMENT
    rc, _, _ = _layout(1, 16)
    assert rc == _lib.QLN_ERR_INVALID_ARGUMENT
    d = _lib.QlnBatchDesc()
    d.B, d.N = 1, 5
    assert L.qln_hessian_layout(C.byref(d), None, C.byref(stride)) == _lib.QLN_ERR_INVALID_ARGUMENT
    buf = np.zeros(1000)
    for fn in (L.qln_eval_hessian_lagrangian, L.qln_eval_hessian_lagrangian_host):
        assert fn(None, buf.ctypes.data, None, buf.ctypes.data, buf.ctypes.data) == _lib.QLN_ERR_INVALID_ARGUMENT
        assert b"null handle" in L.qln_last_error()


def test_no_gpu_means_no_hessian_either():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    import quadruped_landing_amd as Q
    from quadruped_landing_amd import problem_gen as PG

    b = PG.make_batch(2, 5, 3, 1)
    with pytest.raises(_lib.QlnError):
        Q.HybridNLP(b.model, b.obj, b.init_mode, b.k_trans, b.N, b.x0, b.xf, exact_hessian=True)


class _Prob:
    """What moi.py reads of a HybridNLP for the structure, without a device."""

    def __init__(self, N, exact_hessian):
        self.N, self.exact_hessian = N, exact_hessian

    def hessian_structure(self):
        return hessian_structure(self.N)


def test_moi_offers_hess_only_on_opt_in():
    assert moi.features_available(None) == ["Grad", "Jac"]
    assert moi.features_available(_Prob(40, False)) == ["Grad", "Jac"]
    assert moi.features_available(_Prob(40, True)) == ["Grad", "Jac", "Hess"]
    for name in ("hessian_lagrangian_structure", "eval_hessian_lagrangian"):
        assert callable(getattr(moi, name))


@pytest.mark.parametrize("N", (2, 40, 61))
def test_moi_structure_is_one_based_and_matches_the_c_structure(N):
    st = moi.hessian_lagrangian_structure(_Prob(N, True))
    rows, cols = hessian_structure(N)
    assert st == list(zip((rows + 1).tolist(), (cols + 1).tolist()))
    assert min(min(p) for p in st) == 1 and max(max(p) for p in st) == 20 * N - 5
    assert all(r >= c for r, c in st)
