"""CPU checks of the roll-out's forward (tangent) sweep: the numpy yardstick is the exact adjoint of the reverse sweep's
yardstick and matches complex-step differentiation of a whole numpy closed-loop roll-out; argument validation of the C
entry points that needs no device, and the ctypes table."""
import numpy as np
import pytest

from tests import rollout_ref as RR
from tests import tracking_cases as TC
from tests.tracking_cases import CASES, SHAPES

# (N, k_trans): the notebook problem's shape and a few of the tracking shapes
ADJOINT_SHAPES = [(61, 21)] + [(N, kt) for _, N, kt, _ in (SHAPES[0], SHAPES[4], SHAPES[6], SHAPES[12], SHAPES[18])]


@pytest.mark.parametrize("N,k_trans", ADJOINT_SHAPES)
@pytest.mark.parametrize("with_gains", [False, True])
def test_sweep_is_the_adjoint_of_the_reverse_sweep(N, k_trans, with_gains):
    """<Zbar, J d> = <J' Zbar, d> on random blocks, trajectories and directions: neither side needs an oracle."""
    rng = np.random.default_rng(100 * N + k_trans)
    n = 20 * N - 5
    F = RR.evaluator_blocks(rng.normal(size=(N - 1, 15, 20)) / 4.0, k_trans)
    Zref, Zout, Zbar, zd = (rng.normal(size=n) for _ in range(4))
    K = 0.05 * rng.normal(size=(N - 1, 4, 15)) if with_gains else None
    kd = rng.normal(size=(N - 1, 4, 15)) if with_gains else None
    xd = rng.normal(size=15)
    zb, kb, xb, _ = RR.sweep_vjp(F, Zref, K, Zout, Zbar)
    out = RR.sweep_jvp(F, Zref, K, Zout, zd, kd, xd)
    lhs = float(Zbar @ out)
    rhs = float(zb @ zd + xb @ xd + (0.0 if kb is None else kb.reshape(-1) @ kd.reshape(-1)))
    assert abs(lhs - rhs) <= 1e-12 * (abs(lhs) + abs(rhs)), (lhs, rhs)


@pytest.mark.parametrize("N,k_trans,init_mode", CASES)
@pytest.mark.parametrize("with_gains", [False, True])
def test_sweep_matches_complex_step_of_the_whole_rollout(N, k_trans, init_mode, with_gains):
    Zref, K, x0, _ = TC.problem(N, k_trans, init_mode, seed=10 * N + k_trans)
    K = K if with_gains else None
    rng = np.random.default_rng(7 * N + k_trans)
    zd = rng.normal(size=20 * N - 5)
    kd = rng.normal(size=(N - 1, 4, 15)) if with_gains else None
    xd = rng.normal(size=15)
    Zout = RR.rollout(N, k_trans, init_mode, Zref, K, x0)
    F = RR.complex_step_blocks(N, k_trans, init_mode, Zout)
    for dots in ((zd, kd, xd), (None, None, xd), (zd, None, None)) + (((None, kd, None),) if with_gains else ()):
        got = RR.sweep_jvp(F, Zref, K, Zout, *dots)
        ref = RR.jvp_complex_step(N, k_trans, init_mode, Zref, K, x0, None, *dots)
        assert RR.rel(got, ref) <= 1e-8, RR.rel(got, ref)
    # xref_dot_{N-1} is never read
    zd2 = zd.copy()
    zd2[20 * (N - 1):] += 1.0
    assert np.array_equal(RR.sweep_jvp(F, Zref, K, Zout, zd2, kd, xd), RR.sweep_jvp(F, Zref, K, Zout, zd, kd, xd))


def test_entry_points_reject_bad_arguments_without_a_device():
    """Each refusal with the code the reverse sweep gives for its analogue (QLN_ERR_INVALID_ARGUMENT)."""
    from quadruped_landing_amd import _lib

    L = _lib.lib()
    z, o = np.zeros(100), np.zeros(100)
    k, kd = np.zeros(60), np.zeros(60)
    x = np.zeros(15)
    p = lambda a: a.ctypes.data  # noqa: E731
    for fn in (L.qln_tracking_rollout_jvp, L.qln_tracking_rollout_jvp_host):
        # all three tangents NULL
        assert fn(None, p(z), p(k), p(z), None, None, None, p(o)) == _lib.QLN_ERR_INVALID_ARGUMENT
        # K_dot without K
        assert fn(None, p(z), None, p(z), None, p(kd), None, p(o)) == _lib.QLN_ERR_INVALID_ARGUMENT
        # a NULL Zout_dot, a NULL handle
        assert fn(None, p(z), p(k), p(z), p(z), None, p(x), None) == _lib.QLN_ERR_INVALID_ARGUMENT
        assert fn(None, p(z), p(k), p(z), p(z), p(kd), p(x), p(o)) == _lib.QLN_ERR_INVALID_ARGUMENT
    # the reverse sweep's analogues give the same code
    assert L.qln_tracking_rollout_vjp(None, p(z), None, p(z), p(z), None, p(k), None) == _lib.QLN_ERR_INVALID_ARGUMENT


def test_ctypes_table():
    import ctypes as C
    import os
    import re

    from quadruped_landing_amd import _lib

    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "qln_evaluator.h")).read()
    for name in ("qln_tracking_rollout_jvp", "qln_tracking_rollout_jvp_host"):
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == 8
        assert getattr(_lib.lib(), name).argtypes == args
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert proto, name
        params = [q.strip() for q in proto.group(1).split(",")]
        assert len(params) == 8 and params[0].startswith("qln_handle*")
        assert all(q.startswith("const double*") for q in params[1:7]) and params[7].startswith("double*")
        assert params[7].endswith("Zout_dot")
