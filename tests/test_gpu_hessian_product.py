"""GPU parity of the Hessian-vector product of the Lagrangian (qln_eval_hessian_lagrangian_product / _host,
moi.eval_hessian_lagrangian_product) and of the MOI Jacobian products (qln_eval_constraint_jvp_host / _vjp_host).

References: the stored Hessian of qln_eval_hessian_lagrangian at the same (Z, sigma, mu), expanded to the symmetric
matrix and multiplied by v on the host, and the symbolic oracle of tests/hessian_sym.py the same way.  Bars are per row
of y: |dy_i| <= tol * sum_j |H_ij| |v_j|, the rounding a reordered sum of the row's products can show.
"""
import os

import numpy as np
import pytest

from quadruped_landing_amd import moi
from tests import hessian_sym as HS
from tests.test_gpu_hessian import SHAPES, _batch, _inputs, _nlp

pytestmark = pytest.mark.gpu

RTOL_STORED = 1e-13
RTOL_ORACLE = 1e-8


def _selectors():
    """R[e, r] = 1 where entry e of a step block lies in row r, Cs[e, c] likewise for its column; off[e]: r != c."""
    from quadruped_landing_amd.nlp import hessian_structure

    rows, cols = hessian_structure(2)
    r, c = rows[:55], cols[:55]
    R, Cs = np.zeros((55, 20)), np.zeros((55, 20))
    R[np.arange(55), r] = 1.0
    Cs[np.arange(55), c] = 1.0
    return R, Cs, (r != c).astype(np.float64)


def _expand(segs, v, N):
    """(H v) of the symmetric matrices of P problems at once: segs (P, nnz) lower-triangle segments (step blocks of 55,
    then the 15 terminal diagonal values), v (P, >= n_nlp) -> (P, n_nlp)."""
    R, Cs, off = _selectors()
    P, K = segs.shape[0], N - 1
    s = segs[:, : 55 * K].reshape(P, K, 55)
    vb = v[:, : 20 * K].reshape(P, K, 20)
    y = np.zeros((P, 20 * N - 5))
    y[:, : 20 * K] = ((s * (vb @ Cs.T)) @ R + (s * off * (vb @ R.T)) @ Cs).reshape(P, 20 * K)
    y[:, 20 * K:] = segs[:, 55 * K:] * v[:, 20 * K: 20 * K + 15]
    return y


def _segments(nlp, h, ix=None):
    ix = range(nlp.B) if ix is None else ix
    return np.stack([h[b * nlp.h_stride: b * nlp.h_stride + nlp.h_nnz] for b in ix])


def _vec(nlp, seed, pad=np.nan):
    """(B, z_stride) random direction, the step-length entries on their own scale; `pad` past n_nlp."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(nlp.B, nlp.z_stride))
    v[:, 19 + 20 * np.arange(nlp.N - 1)] *= 1e-2
    v[:, nlp.n_nlp:] = pad
    return v


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()


def _hv(nlp, Z, sig_d, mu_d, v, fill=np.nan):
    """y of every problem as (B, z_stride), out pre-filled with `fill`."""
    import torch

    out = torch.full((nlp.dims.z_total,), fill, dtype=torch.float64, device="cuda")
    nlp.hess_lag_vec(Z, sig_d, mu_d, _dev(v), out)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(nlp.B, nlp.z_stride)


def _stored(nlp, Z, sig_d, mu_d):
    import torch

    out = torch.zeros(nlp.h_total, dtype=torch.float64, device="cuda")
    nlp.hess_lag(Z, sig_d, mu_d, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _Z_nan_padded(nlp, batch):
    buf = np.full((nlp.B, nlp.z_stride), np.nan)
    buf[:, : nlp.n_nlp] = batch.Z
    return _dev(buf)


def _row_err(y, ref, scale):
    """max over rows of |y - ref| / scale (0 where they agree exactly)."""
    d = np.abs(y - ref)
    return float(np.max(np.where(d == 0, 0.0, d / np.maximum(scale, 1e-300)), initial=0.0))


def _check(batch, seed=0, **kw):
    nlp = _nlp(batch, **kw)
    n = nlp.n_nlp
    Z = _Z_nan_padded(nlp, batch)
    sigma, mu, sig_d, mu_d = _inputs(nlp, seed)
    v = _vec(nlp, seed + 1)
    y = _hv(nlp, Z, sig_d, mu_d, v)
    # padding past n_nlp is never written; NaN in the padding of Z and v never reaches the written part
    assert np.all(np.isnan(y[:, n:])) and np.all(np.isfinite(y[:, :n]))
    segs = _segments(nlp, _stored(nlp, Z, sig_d, mu_d))
    scale = _expand(np.abs(segs), np.abs(v), batch.N)
    err = _row_err(y[:, :n], _expand(segs, v, batch.N), scale)
    assert err <= RTOL_STORED, err
    ref = HS.batch_hvals(batch.N, batch.k_trans, batch.init_mode, batch.Z, mu, nlp.c_off, sigma, batch.obj)
    oscale = _expand(np.abs(ref), np.abs(v), batch.N)
    # the oracle's own row norm, floored at 1e-12 x the problem's largest (its bar on the stored values)
    oscale = np.maximum(oscale, 1e-12 * oscale.max(axis=1, keepdims=True))
    oerr = _row_err(y[:, :n], _expand(ref, v, batch.N), oscale)
    assert oerr <= RTOL_ORACLE, oerr
    return nlp


@pytest.mark.parametrize("B,N,k_trans,init_mode", SHAPES)
def test_against_stored_hessian_and_oracle_over_shapes(B, N, k_trans, init_mode):
    _check(_batch(B, N, k_trans, init_mode, seed=N + k_trans))


@pytest.mark.parametrize("N", [40, 80])
def test_ragged_with_per_problem_costs(N):
    _check(_batch(37, N, 0, 0, seed=N, ragged=True))


@pytest.mark.parametrize("N,kw", [(40, dict(z_stride=832, align=3)), (65, dict(z_stride=1296, align=1)),
                                  (80, dict(z_stride=1601, align=32)), (61, dict(align=2, z_stride=1300))])
def test_padded_strides_and_alignments_with_per_problem_cost(N, kw):
    nlp = _check(_batch(13, N, 21, 2, seed=3, per_problem_cost=True), **kw)
    assert nlp.z_stride == kw["z_stride"] > nlp.n_nlp


@pytest.mark.parametrize("B,N,ragged", [(65536, 40, False), (65536, 80, True)])
def test_full_size_every_problem(B, N, ragged):
    """BASELINE.json configs[2] (65 536 x N = 40, shared table: the persistent waves) and the ragged N = 80 configuration
    (per-problem tables, two chunks): every problem against the stored-Hessian product; then, oracle-free on a sample,
    with sigma = 0 H v = the central difference of qln_eval_constraint_vjp along v."""
    import torch
    from quadruped_landing_amd import problem_gen as PG

    batch = PG.make_batch(B, N, 14, 1, seed=11, ragged=ragged)
    nlp = _nlp(batch)
    n = nlp.n_nlp
    Z = nlp.upload_Z(batch.Z)
    sigma, mu, sig_d, mu_d = _inputs(nlp, 5)
    v = _vec(nlp, 6, pad=0.0)
    y = _hv(nlp, Z, sig_d, mu_d, v)
    h = _stored(nlp, Z, sig_d, mu_d)
    worst = 0.0
    step = 2048
    for p0 in range(0, B, step):
        ix = np.arange(p0, min(B, p0 + step))
        segs = _segments(nlp, h, ix)
        scale = _expand(np.abs(segs), np.abs(v[ix]), N)
        worst = max(worst, _row_err(y[ix, :n], _expand(segs, v[ix], N), scale))
    print(f"\nfull size B={B} N={N} ragged={ragged}: worst row error against the stored-Hessian product {worst:.3e}")
    assert worst <= RTOL_STORED
    del h

    # oracle-free: sigma = 0, H v against (J(Z + e v)' mu - J(Z - e v)' mu) / 2e
    rng = np.random.default_rng(9)
    y0 = _hv(nlp, Z, torch.zeros(B, dtype=torch.float64, device="cuda"), mu_d, v)
    h0 = _stored(nlp, Z, torch.zeros(B, dtype=torch.float64, device="cuda"), mu_d)
    eps = 1e-6
    vd = _dev(v)
    gp = nlp.jac_t_vec(Z + eps * vd, mu_d).cpu().numpy().reshape(B, nlp.z_stride)
    gm = nlp.jac_t_vec(Z - eps * vd, mu_d).cpu().numpy().reshape(B, nlp.z_stride)
    ix = rng.choice(B, size=64, replace=False)
    segs = _segments(nlp, h0, ix)
    fd = (gp[ix, :n] - gm[ix, :n]) / (2 * eps)
    # truncation is O(eps^2); rounding of the difference ~1e-16 |g| / eps = 1e-10 |g|
    tol = 1e-6 * _expand(np.abs(segs), np.abs(v[ix]), N) + 1e-8 * np.abs(gp[ix, :n]).max(axis=1, keepdims=True)
    fd_err = float(np.max(np.abs(y0[ix, :n] - fd) / tol))
    print(f"oracle-free: worst |Hv - central difference| / tol over 64 problems {fd_err:.3e}")
    assert fd_err <= 1.0


def _algebra_setup(seed=8, N=70, kt=20):
    batch = _batch(9, N, kt, 1, seed=seed)
    nlp = _nlp(batch)
    Z = nlp.upload_Z(batch.Z)
    return batch, nlp, Z


def test_symmetry_and_linearity_in_v():
    batch, nlp, Z = _algebra_setup()
    n, N = nlp.n_nlp, batch.N
    sigma, mu, sig_d, mu_d = _inputs(nlp, 2)
    u, v = _vec(nlp, 3, pad=0.0), _vec(nlp, 4, pad=0.0)
    Hu, Hv = _hv(nlp, Z, sig_d, mu_d, u)[:, :n], _hv(nlp, Z, sig_d, mu_d, v)[:, :n]
    absH = np.abs(_segments(nlp, _stored(nlp, Z, sig_d, mu_d)))
    # symmetry: u.(Hv) = v.(Hu), relative to sum_ij |u_i| |H_ij| |v_j|
    s = np.sum(np.abs(u[:, :n]) * _expand(absH, np.abs(v), N), axis=1)
    assert np.all(np.abs(np.sum(u[:, :n] * Hv, axis=1) - np.sum(v[:, :n] * Hu, axis=1)) <= 1e-13 * s)
    # linearity in v
    a, b = 0.75, -2.5
    Hw = _hv(nlp, Z, sig_d, mu_d, a * u + b * v)[:, :n]
    scale = abs(a) * _expand(absH, np.abs(u), N) + abs(b) * _expand(absH, np.abs(v), N)
    assert np.all(np.abs(Hw - (a * Hu + b * Hv)) <= 1e-13 * scale)


def test_linearity_in_sigma_and_mu():
    import torch

    batch, nlp, Z = _algebra_setup(seed=5, N=40, kt=14)
    n, N = nlp.n_nlp, batch.N
    sigma, mu, sig_d, mu_d = _inputs(nlp, 3)
    v = _vec(nlp, 7, pad=0.0)
    ones = torch.ones(nlp.B, dtype=torch.float64, device="cuda")
    zs, zm = torch.zeros_like(ones), torch.zeros_like(mu_d)
    full = _hv(nlp, Z, sig_d, mu_d, v)[:, :n]
    obj = _hv(nlp, Z, ones, zm, v)[:, :n]
    con = _hv(nlp, Z, zs, mu_d, v)[:, :n]
    absO = np.abs(_segments(nlp, _stored(nlp, Z, ones, zm)))
    absC = np.abs(_segments(nlp, _stored(nlp, Z, zs, mu_d)))
    scale = _expand(np.abs(sigma)[:, None] * absO + absC, np.abs(v), N)
    assert np.all(np.abs(full - (sigma[:, None] * obj + con)) <= 1e-13 * scale)
    # mu: H(mu1 + mu2) v = H(mu1) v + H(mu2) v
    mu2 = np.random.default_rng(11).normal(size=mu.size)
    c2 = _hv(nlp, Z, zs, _dev(mu2), v)[:, :n]
    c12 = _hv(nlp, Z, zs, _dev(mu + mu2), v)[:, :n]
    absC2 = np.abs(_segments(nlp, _stored(nlp, Z, zs, _dev(mu2))))
    assert np.all(np.abs(c12 - (con + c2)) <= 1e-13 * _expand(absC + absC2, np.abs(v), N))
    # sigma = None means 1.0 for every problem
    assert np.array_equal(_hv(nlp, Z, None, zm, v)[:, :n], obj)


def test_zero_inputs_give_exact_zeros_and_ignored_multipliers_are_never_read():
    import torch

    batch, nlp, Z = _algebra_setup(seed=4)
    n, N = nlp.n_nlp, batch.N
    sigma, mu, sig_d, mu_d = _inputs(nlp, 2)
    v = _vec(nlp, 1, pad=0.0)
    y0 = _hv(nlp, Z, sig_d, mu_d, np.zeros_like(v))
    assert np.all(y0[:, :n] == 0.0)
    zs = torch.zeros(nlp.B, dtype=torch.float64, device="cuda")
    assert np.all(_hv(nlp, Z, zs, torch.zeros_like(mu_d), v)[:, :n] == 0.0)
    y1 = _hv(nlp, Z, sig_d, mu_d, v)
    mu2 = mu.copy()
    for b in range(nlp.B):
        kt = int(batch.k_trans[b])
        m = 18 * N - kt + 16
        lin = np.r_[0:29, 29 + 15 * (N - 1): m - N]  # initial, terminal, contact, final-control rows
        mu2[nlp.c_off[b] + lin] = 1e3 * np.arange(1, lin.size + 1)
        jrow = nlp.c_off[b] + 29 + 15 * (kt - 2)
        mu2[jrow + np.array([4, 6, 10, 11, 12, 13, 14])] = -7.0e5
    y2 = _hv(nlp, Z, sig_d, _dev(mu2), v)
    assert np.array_equal(y1[:, :n].view(np.uint64), y2[:, :n].view(np.uint64))


def test_clearance_curvature_takes_quirk_Q3s_branch():
    """theta = +-0 and +-1e-300 on the first knot, the jump knot, a knot of the second chunk and the terminal knot;
    sigma = 0, mu on the clearance rows only, v = 1: y at theta_k is +(lb/2) sin(theta) mu for theta > 0 and
    -(lb/2) sin(theta) mu otherwise (within 1 ulp), a zero at theta = +-0; every other entry is zero."""
    import torch

    N, kt = 80, 10
    batch = _batch(4, N, kt, 1, seed=6)
    knots = [1, kt - 1, 70, N]  # 1-based
    thetas = [0.0, -0.0, 1e-300, -1e-300]
    for b in range(4):
        for k in knots:
            batch.Z[b, 20 * (k - 1) + 2] = thetas[b]
    nlp = _nlp(batch)
    n = nlp.n_nlp
    Z = nlp.upload_Z(batch.Z)
    rng = np.random.default_rng(1)
    mu = np.zeros(nlp.dims.c_total)
    muc = rng.uniform(0.5, 2.0, size=(4, N))
    for b in range(4):
        o = nlp.c_off[b] + 17 * N - kt + 16
        mu[o: o + N] = muc[b]
    v = np.ones((4, nlp.z_stride))
    y = _hv(nlp, Z, torch.zeros(4, dtype=torch.float64, device="cuda"), _dev(mu), v)[:, :n]
    lb = batch.model.lb
    for b in range(4):
        th = thetas[b]
        for k in knots:
            got = y[b, 20 * (k - 1) + 2]
            exp = ((lb / 2) * np.sin(th) if th > 0 else -((lb / 2) * np.sin(th))) * muc[b, k - 1]
            if th == 0:
                assert got == 0.0
            else:
                assert abs(got - exp) <= np.spacing(abs(exp)), (b, k, got, exp)
                assert np.sign(got) == np.sign(exp) == 1.0
        mask = np.ones(n, dtype=bool)
        mask[20 * np.arange(N) + 2] = False
        assert np.all(y[b, mask] == 0.0)


@pytest.mark.parametrize("z_stride", [0, 20 * 61 + 3])
@pytest.mark.parametrize("B", [7, 64])
def test_host_forms_give_the_device_bits(B, z_stride):
    """B = 7 runs on mapped host memory (zero copy), B = 64 is staged through device memory.  With a padded z_stride, a
    roll-out's in-out Zout full of NaN goes through the handle first: none of it may reach the padding of a result."""
    import torch

    from quadruped_landing_amd import _lib

    batch = _batch(B, 61, 21, 1, seed=12)
    nlp = _nlp(batch, matrix_free=True, exact_hessian=True, z_stride=z_stride)
    n = nlp.n_nlp
    zout = np.full(nlp.dims.z_total, np.nan)
    _lib.check(_lib.lib().qln_tracking_rollout_host(nlp._h, nlp._host_Z(batch.Z).ctypes.data, None, None, zout.ctypes.data))
    assert np.all(np.isnan(zout.reshape(B, nlp.z_stride)[:, n:]))  # in-out: the padding comes back as it went in
    Z = nlp.upload_Z(batch.Z)
    sigma, mu, sig_d, mu_d = _inputs(nlp, 4)
    v = _vec(nlp, 5, pad=0.0)
    yd = _hv(nlp, Z, sig_d, mu_d, v, fill=0.0).reshape(-1)
    yh = nlp.hess_lag_vec_host(batch.Z, sigma, mu, v)
    assert np.array_equal(yd.view(np.uint64), yh.view(np.uint64))
    yh1 = nlp.hess_lag_vec_host(batch.Z, None, mu, v[:, :n])  # n_nlp per problem, sigma = 1
    yd1 = _hv(nlp, Z, None, mu_d, v, fill=0.0).reshape(-1)
    assert np.array_equal(yd1.view(np.uint64), yh1.view(np.uint64))
    jd = nlp.jac_vec(Z, _dev(v)).cpu().numpy()
    assert np.array_equal(jd.view(np.uint64), nlp.jac_vec_host(batch.Z, v).view(np.uint64))
    gd = torch.zeros(nlp.dims.z_total, dtype=torch.float64, device="cuda")
    gd = nlp.jac_t_vec(Z, mu_d, gd).cpu().numpy()
    assert np.array_equal(gd.view(np.uint64), nlp.jac_t_vec_host(batch.Z, mu).view(np.uint64))
    assert moi.features_available(nlp) == ["Grad", "Jac", "Hess", "JacVec", "HessVec"]


def test_argument_validation_with_a_handle():
    from quadruped_landing_amd import HybridNLP, _lib

    batch = _batch(2, 5, 3, 1)
    nlp = _nlp(batch)
    L = _lib.lib()
    buf = np.zeros(nlp.dims.z_total + nlp.dims.c_total)
    p = buf.ctypes.data
    for fn in (L.qln_eval_hessian_lagrangian_product, L.qln_eval_hessian_lagrangian_product_host):
        for args in ((None, None, p, p, p), (p, None, None, p, p), (p, None, p, None, p), (p, None, p, p, None)):
            assert fn(nlp._h, *args) == _lib.QLN_ERR_INVALID_ARGUMENT
            assert b"null pointer" in L.qln_last_error()
    for fn in (L.qln_eval_constraint_jvp_host, L.qln_eval_constraint_vjp_host):
        for args in ((None, p, p), (p, None, p), (p, p, None)):
            assert fn(nlp._h, *args) == _lib.QLN_ERR_INVALID_ARGUMENT
            assert b"null pointer" in L.qln_last_error()
    # the Hessian product needs a cost table
    nc = HybridNLP(batch.model, None, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf)
    for fn in (L.qln_eval_hessian_lagrangian_product, L.qln_eval_hessian_lagrangian_product_host):
        assert fn(nc._h, p, None, p, p, p) == _lib.QLN_ERR_INVALID_ARGUMENT
        assert b"no cost table" in L.qln_last_error()


def test_moi_products_on_the_notebook_problem(golden_dir):
    """At data_6.csv: moi.eval_constraint_jacobian_product and its transpose equal the dense moi.eval_constraint_jacobian
    matrix times w; moi.eval_hessian_lagrangian_product equals the expanded moi.eval_hessian_lagrangian times v."""
    from quadruped_landing_amd import problem_gen as PG

    nb = PG.notebook_problem()
    one = _nlp(nb, matrix_free=True, exact_hessian=True)
    assert moi.features_available(one) == ["Grad", "Jac", "Hess", "JacVec", "HessVec"]
    N, n = nb.N, one.n_nlp
    m = one.num_duals(0)
    x = np.loadtxt(os.path.join(golden_dir, "data_6.csv"))
    rng = np.random.default_rng(0)
    w, lam, v, mu1 = rng.normal(size=n), rng.normal(size=m), rng.normal(size=n), rng.normal(size=m)

    jac = np.zeros(m * n)
    moi.eval_constraint_jacobian(one, jac, x)
    J = jac.reshape((m, n), order="F")
    y = np.full(m, np.nan)
    moi.eval_constraint_jacobian_product(one, y, x, w)
    assert np.all(np.abs(y - J @ w) <= 1e-12 * (np.abs(J) @ np.abs(w)) + 1e-300)
    g = np.full(n, np.nan)
    moi.eval_constraint_jacobian_transpose_product(one, g, x, lam)
    assert np.all(np.abs(g - J.T @ lam) <= 1e-12 * (np.abs(J.T) @ np.abs(lam)) + 1e-300)

    st = moi.hessian_lagrangian_structure(one)
    H = np.full(len(st), np.nan)
    moi.eval_hessian_lagrangian(one, H, x, 0.75, mu1)
    dense = np.zeros((n, n))
    for (r, c), val in zip(st, H):
        dense[r - 1, c - 1] += val
        if r != c:
            dense[c - 1, r - 1] += val
    hv = np.full(n, np.nan)
    moi.eval_hessian_lagrangian_product(one, hv, x, v, 0.75, mu1)
    assert np.all(np.abs(hv - dense @ v) <= 1e-13 * (np.abs(dense) @ np.abs(v)))
    # sigma as a (B,) array
    hv2 = np.full(n, np.nan)
    moi.eval_hessian_lagrangian_product(one, hv2, x, v, np.array([0.75]), mu1)
    assert np.array_equal(hv, hv2)

