"""The matrix-free products without a GPU: the four new entry points (qln_eval_hessian_lagrangian_product and its _host
form, qln_eval_constraint_jvp_host / _vjp_host) are declared, bound and exported, validate their arguments, and the MOI
surface offers "JacVec" and "HessVec" only on opt-in."""
import os
import re

import numpy as np

from quadruped_landing_amd import _lib, moi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("qln_eval_hessian_lagrangian_product", "qln_eval_hessian_lagrangian_product_host",
       "qln_eval_constraint_jvp_host", "qln_eval_constraint_vjp_host")


def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "qln_evaluator.h")).read()
    L = _lib.lib()
    for name in NEW:
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(L, name) is not None
    assert len(_lib.SIGNATURES["qln_eval_hessian_lagrangian_product"][1]) == 6
    assert len(_lib.SIGNATURES["qln_eval_hessian_lagrangian_product_host"][1]) == 6
    assert len(_lib.SIGNATURES["qln_eval_constraint_jvp_host"][1]) == 4
    assert len(_lib.SIGNATURES["qln_eval_constraint_vjp_host"][1]) == 4


def test_argument_validation_needs_no_gpu():
    L = _lib.lib()
    buf = np.zeros(1000)
    p = buf.ctypes.data
    for fn in (L.qln_eval_hessian_lagrangian_product, L.qln_eval_hessian_lagrangian_product_host):
        assert fn(None, p, None, p, p, p) == _lib.QLN_ERR_INVALID_ARGUMENT
        assert b"null handle" in L.qln_last_error()
    for fn in (L.qln_eval_constraint_jvp_host, L.qln_eval_constraint_vjp_host):
        assert fn(None, p, p, p) == _lib.QLN_ERR_INVALID_ARGUMENT
        assert b"null handle" in L.qln_last_error()


class _Prob:
    """What moi.features_available reads of a HybridNLP, without a device."""

    def __init__(self, exact_hessian=False, matrix_free=False):
        self.exact_hessian, self.matrix_free = exact_hessian, matrix_free


def test_moi_offers_jacvec_and_hessvec_only_on_opt_in_after_the_existing_entries():
    assert moi.features_available(None) == ["Grad", "Jac"]
    assert moi.features_available(_Prob()) == ["Grad", "Jac"]
    assert moi.features_available(_Prob(exact_hessian=True)) == ["Grad", "Jac", "Hess"]
    assert moi.features_available(_Prob(matrix_free=True)) == ["Grad", "Jac", "JacVec", "HessVec"]
    assert moi.features_available(_Prob(True, True)) == ["Grad", "Jac", "Hess", "JacVec", "HessVec"]
    for name in ("eval_constraint_jacobian_product", "eval_constraint_jacobian_transpose_product",
                 "eval_hessian_lagrangian_product"):
        assert callable(getattr(moi, name))


def test_hybrid_nlp_takes_the_matrix_free_keyword():
    import inspect

    from quadruped_landing_amd import HybridNLP

    p = inspect.signature(HybridNLP.__init__).parameters["matrix_free"]
    assert p.kind == p.KEYWORD_ONLY and p.default is False
    for name in ("hess_lag_vec", "hess_lag_vec_host", "jac_vec_host", "jac_t_vec_host"):
        assert callable(getattr(HybridNLP, name))


def test_julia_file_defines_the_three_product_methods():
    src = open(os.path.join(ROOT, "integration", "julia", "HybridNLPHIP.jl")).read()
    for meth in ("eval_constraint_jacobian_product", "eval_constraint_jacobian_transpose_product",
                 "eval_hessian_lagrangian_product"):
        assert re.search(rf"function\s+MOI\.{meth}\s*\(\s*\w+::HybridNLPHIP", src), meth
    assert re.search(r"HybridNLPHIP\([^)]*;[^)]*matrix_free\s*=\s*false", src, flags=re.S)
    assert ":JacVec, :HessVec" in src
    for sym in ("qln_eval_constraint_jvp_host", "qln_eval_constraint_vjp_host", "qln_eval_hessian_lagrangian_product_host"):
        assert f"(:{sym}, LIBQLN)" in src, sym
