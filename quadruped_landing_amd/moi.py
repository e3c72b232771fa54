"""MOI.AbstractNLPEvaluator callback surface (mirror of src/moi.jl:1-33).

Same method names and argument order as the reference's MOI methods on HybridNLP; `prob` is a
quadruped_landing_amd.nlp.HybridNLP.  Host arrays in, host arrays filled in place -- the shape
Ipopt's callbacks have (src/moi.jl:1-24) -- with the arithmetic done by the HIP kernels.
The Julia veneer with the identical surface is integration/julia/HybridNLPHIP.jl.
"""
from __future__ import annotations

import numpy as np


def eval_objective(prob, x):
    """MOI.eval_objective, src/moi.jl:1-3.  Scalar for B == 1, else (B,) array."""
    f = prob.eval_f_host(x)
    return float(f[0]) if prob.B == 1 else f


def eval_objective_gradient(prob, grad_f, x):
    """MOI.eval_objective_gradient, src/moi.jl:5-8 (in place)."""
    g = prob.grad_f_host(x)
    np.asarray(grad_f).reshape(-1)[:] = g.reshape(prob.B, prob.z_stride)[:, : prob.n_nlp].reshape(-1) \
        if np.asarray(grad_f).size == prob.B * prob.n_nlp else g
    return None


def eval_constraint(prob, g, x):
    """MOI.eval_constraint, src/moi.jl:10-13 (in place)."""
    c = prob.eval_c_host(x)
    out = np.asarray(g).reshape(-1)
    if prob.B == 1:
        out[:] = c[: out.size]
    else:
        out[:] = c
    return None


def eval_constraint_jacobian(prob, vec, x, b: int = 0):
    """MOI.eval_constraint_jacobian, src/moi.jl:15-24: `vec` is a flat length m_nlp*n_nlp buffer,
    reshaped column-major (m_nlp, n_nlp); only the jac_c! write-set is assigned."""
    m_nlp, n_nlp = prob.num_duals(b), prob.num_primals()
    jac = np.asarray(vec).reshape((m_nlp, n_nlp), order="F")
    if not np.shares_memory(jac, vec):
        raise ValueError("vec must be a contiguous float64 buffer")
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if x.size == n_nlp:                     # problem b's own decision vector
        xb = x
    elif x.size == prob.B * prob.z_stride:  # the whole batch in the handle's layout: take problem b's slice
        xb = x.reshape(prob.B, prob.z_stride)[b, :n_nlp]
    elif x.size == prob.B * n_nlp:
        xb = x.reshape(prob.B, n_nlp)[b]
    else:
        raise ValueError(f"x has {x.size} entries; expected n_nlp = {n_nlp} or the whole batch")
    prob.jac_c_dense_host(xb, jac, b)
    return None


def _fill_z(prob, out, z):
    """Copy a result in the handle's Z layout into `out`: one problem's n_nlp entries per problem if that is its size,
    the whole layout otherwise."""
    out = np.asarray(out).reshape(-1)
    if out.size == prob.B * prob.n_nlp:
        out[:] = z.reshape(prob.B, prob.z_stride)[:, : prob.n_nlp].reshape(-1)
    elif out.size == z.size:
        out[:] = z
    else:
        raise ValueError(f"output has {out.size} entries; expected {prob.B * prob.n_nlp} or {z.size}")


def _fill_c(prob, out, c):
    out = np.asarray(out).reshape(-1)
    if out.size != c.size:
        raise ValueError(f"output has {out.size} entries; expected {c.size}")
    out[:] = c


def eval_constraint_jacobian_product(prob, y, x, w):
    """MOI.eval_constraint_jacobian_product (in place): y = J(x) w.  For B == 1 x and w are n_nlp vectors and y the m_nlp
    constraint rows; for a batch x and w hold every problem (n_nlp each or the handle's Z layout) and y is in the layout
    of c.  The Jacobian is re-derived on the GPU, never stored."""
    _fill_c(prob, y, prob.jac_vec_host(x, w))
    return None


def eval_constraint_jacobian_transpose_product(prob, y, x, w):
    """MOI.eval_constraint_jacobian_transpose_product (in place): y = J(x)' w, w in the layout of c (m_nlp for B == 1),
    y like x."""
    _fill_z(prob, y, prob.jac_t_vec_host(x, w))
    return None


def eval_hessian_lagrangian_product(prob, h, x, v, sigma, mu):
    """MOI.eval_hessian_lagrangian_product (in place): h = (sigma d2 f(x) + sum_i mu[i] d2 c_i(x)) v, the operator
    eval_hessian_lagrangian returns, never stored.  x, v and h: n_nlp vectors for B == 1, or every problem (n_nlp each or
    the handle's Z layout); mu in the layout of c; sigma a scalar or a (B,) array."""
    _fill_z(prob, h, prob.hess_lag_vec_host(x, np.broadcast_to(np.asarray(sigma, dtype=np.float64), (prob.B,)), mu, v))
    return None


def features_available(prob):
    """src/moi.jl:26-28; "Hess" only for a problem built with exact_hessian=True (the reference offers none), and
    "JacVec", "HessVec" after them only for one built with matrix_free=True."""
    feats = ["Grad", "Jac", "Hess"] if getattr(prob, "exact_hessian", False) else ["Grad", "Jac"]
    if getattr(prob, "matrix_free", False):
        feats += ["JacVec", "HessVec"]
    return feats


def initialize(prob, features):
    """src/moi.jl:30"""
    return None


def jacobian_structure(prob, b: int = 0):
    """src/moi.jl:31-33: all (row, col) pairs of the dense m_nlp x n_nlp matrix, row index fastest,
    1-based like the reference."""
    m_nlp, n_nlp = prob.num_duals(b), prob.num_primals()
    cols, rows = np.divmod(np.arange(m_nlp * n_nlp), m_nlp)
    return list(zip((rows + 1).tolist(), (cols + 1).tolist()))


def sparse_jacobian_structure(prob, b: int = 0):
    """The write-set of jac_c! as 1-based (row, col) pairs in the order of the block-COO values --
    what `use_sparse_jacobian=true` (src/nlp.jl:35,75-76) was meant to hand to Ipopt."""
    rows, cols = prob.jacobian_structure(b)
    return list(zip((rows + 1).tolist(), (cols + 1).tolist()))


def hessian_lagrangian_structure(prob):
    """MOI.hessian_lagrangian_structure: 1-based (row, col) pairs, row >= col, of one problem's Lagrangian Hessian in the
    order eval_hessian_lagrangian fills them (block-diagonal over knots, 55 per step block, 15 for x_N)."""
    rows, cols = prob.hessian_structure()
    return list(zip((rows + 1).tolist(), (cols + 1).tolist()))


def eval_hessian_lagrangian(prob, H, x, sigma, mu):
    """MOI.eval_hessian_lagrangian (in place): H[j] = value of entry j of hessian_lagrangian_structure for
    sigma * d2 f(x) + sum_i mu[i] d2 c_i(x).  For a batch, x / mu / H hold every problem (mu in the layout of c, H problem b
    at b * h_stride) and sigma may be a scalar or a (B,) array."""
    out = np.asarray(H).reshape(-1)
    vals = prob.hess_lag_host(x, np.broadcast_to(np.asarray(sigma, dtype=np.float64), (prob.B,)), mu)
    if out.size < vals.size:
        raise ValueError(f"H has {out.size} entries, expected {vals.size}")
    out[: vals.size] = vals
    return None
