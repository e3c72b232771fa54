"""numpy restatement of qln_estimate_multipliers (include/qln_evaluator.h): the active set, the free mask from
variable_bounds, the row norms w, the CGLS recurrence on T = (A D)' W^-1 started at 0, and the info fields -- on a dense
or scipy-sparse Jacobian of ONE problem, built from the oracle (forward-mode duals), never from the library under test.
"""
import numpy as np

from quadruped_landing_amd.nlp import _variable_bounds

INFO_STRIDE = 16


def oracle_jacobian(onlp, Z):
    """The oracle's jac_c of one OracleNLP problem at Z as a scipy CSR matrix (m_nlp, n_nlp)."""
    import scipy.sparse as sp

    rows, cols = onlp.jac_structure()
    return sp.coo_matrix((onlp.jac_c_coo(Z), (rows, cols)), shape=(onlp.m_nlp, onlp.n_nlp)).tocsr()


def batch_jacobian(nlp, ref, b):
    """Problem b's Jacobian from oracle_batch's values in the product handle's layout, as _system of
    tests/test_gpu_gauss_newton.py builds it."""
    import scipy.sparse as sp

    m, nnz = nlp.problem_dims(b)
    rows, cols = nlp.jacobian_structure(b)
    vals = ref["vals"][nlp.j_off[b]: nlp.j_off[b] + nnz]
    return sp.coo_matrix((vals, (rows, cols)), shape=(m, nlp.n_nlp)).tocsr()


def bounds(N, h_min=0.001, h_max=0.02, theta_min=-np.pi / 2, theta_max=np.pi / 2, q6_bounds=True):
    """(x_l, x_u) of qln_variable_bounds(N, opt): variable_bounds(N) with the option scalars in place of the literals."""
    x_l, x_u = _variable_bounds(N, True)
    if not q6_bounds:
        k = 20 * np.arange(1, N)
        x_l[k + 1] = x_l[k + 3] = -np.inf
    x_l[2::20], x_u[2::20] = theta_min, theta_max
    x_l[19::20], x_u[19::20] = h_min, h_max
    return x_l, x_u


def active_rows(c, N, act_tol):
    """every equality row; clearance row i (the last N of c) iff !(c_i > act_tol): a NaN is active"""
    m = c.size
    with np.errstate(invalid="ignore"):
        return (np.arange(m) < m - N) | ~(c > act_tol)


def sides(Z, x_l, x_u, bound_tol):
    """(at the lower bound, at the upper bound) to bound_tol; bound_tol < 0: no variable is fixed"""
    if bound_tol < 0:
        return np.zeros(Z.size, bool), np.zeros(Z.size, bool)
    with np.errstate(invalid="ignore"):
        return Z <= x_l + bound_tol, Z >= x_u - bound_tol


def operator(J, Z, c, N, *, act_tol=1e-6, bound_tol=1e-8, row_scaling=True, **bnd):
    """(A, free, w, T): A = the active rows of J (the others zeroed, so lam keeps the layout of c), free the 0/1 mask,
    w the norms of the rows of A D (1 where 0, and 1 everywhere without row scaling), T = (A D)' W^-1."""
    import scipy.sparse as sp

    act = active_rows(c, N, act_tol)
    at_l, at_u = sides(Z, *bounds(N, **bnd), bound_tol)
    free = (~(at_l | at_u)).astype(float)
    A = sp.diags(act.astype(float)) @ sp.csr_matrix(J)
    AD = (A @ sp.diags(free)).tocsr()
    w = np.ones(A.shape[0])
    if row_scaling:
        w = np.sqrt(np.asarray(AD.multiply(AD).sum(axis=1)).ravel())
        w[w == 0] = 1.0
    T = (sp.diags(1.0 / w) @ AD).T.tocsr()
    return A, free, w, T


def cgls(T, rhs, max_iters, rel_tol):
    """min_y || T y - rhs ||_2 from 0, exactly the recurrence of the header.  Returns (y, r, gamma, iterations)."""
    y = np.zeros(T.shape[1])
    r = rhs.copy()
    s = T.T @ r
    p = s.copy()
    gamma = gamma0 = s @ s
    it = 0
    while it < max_iters and gamma > rel_tol * rel_tol * gamma0:
        q = T @ p
        qq = q @ q
        if not qq > 0:
            break
        alpha = gamma / qq
        y += alpha * p
        r -= alpha * q
        s = T.T @ r
        gnew = s @ s
        p = s + (gnew / gamma) * p
        gamma = gnew
        it += 1
    return y, r, gamma, it


def _max_abs(v):
    """the library's maxima are fmax reductions from 0: a NaN entry is ignored, an empty set gives 0"""
    return float(np.fmax.reduce(np.abs(v), initial=0.0))


def estimate(J, Z, c, g, N, *, act_tol=1e-6, bound_tol=1e-8, row_scaling=True, max_iters=20000, rel_tol=1e-8, **bnd):
    """(lam, lag, info) of one problem as the library defines them."""
    A, free, w, T = operator(J, Z, c, N, act_tol=act_tol, bound_tol=bound_tol, row_scaling=row_scaling, **bnd)
    Dg = free * g
    y, r, gamma, it = cgls(T, -Dg, max_iters, rel_tol)
    lam = y / w
    act = active_rows(c, N, act_tol)
    lam[~act] = 0.0
    lag = g + A.T @ lam
    at_l, at_u = sides(Z, *bounds(N, **bnd), bound_tol)
    fr = free > 0
    clear = np.arange(c.size) >= c.size - N
    ac = act & clear
    info = np.zeros(INFO_STRIDE)
    info[0] = it
    info[1] = Dg @ Dg
    info[2] = gamma
    info[3] = r @ r
    info[4] = _max_abs(lag[fr])
    info[5] = ac.sum()
    info[6] = (~fr).sum()
    info[7] = (lam[ac] > 0).sum()
    info[8] = ((at_l & ~at_u & (lag < 0)) | (at_u & ~at_l & (lag > 0))).sum()
    info[9] = _max_abs(lam[ac] * c[ac])
    info[10] = _max_abs(lam)
    info[11] = _max_abs(g[fr])
    return lam, lag, info


def lstsq_residual(T, Dg):
    """(y, residual vector T y + D g) of numpy.linalg.lstsq's minimum-norm solution, rcond = 1e-12"""
    Td = T.toarray()
    y, *_ = np.linalg.lstsq(Td, -Dg, rcond=1e-12)
    return y, Td @ y + Dg
