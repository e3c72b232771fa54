"""GPU parity of qln_estimate_multipliers: least-squares Lagrange multipliers over the active set and the KKT report.

The reference has no such estimate (Ipopt keeps its duals to itself), so what pins the kernel is
  * the same CGLS recurrence in numpy (tests/multiplier_ref.py) on the ORACLE's Jacobian, iterate for iterate over the
    first three iterations, to 1e-8 of the result's size -- what the project holds the two LDS products to in
    test_gpu_gauss_newton.py; later Krylov iterates amplify the ~1e-11 relative difference between the closed-form and
    the forward-mode Jacobian (perturbing numpy's own matrix by 4e-11 relative moved three iterates by <= 2.6e-10);
  * planted multipliers recovered through the separate k_constraint_vjp, no oracle involved;
  * the converged estimate at a GPU-solved landing against numpy.linalg.lstsq's residual;
  * masks, locality of a NaN, the host form, the LDS bound, randomised shapes, and the example.
"""
import dataclasses

import numpy as np
import pytest

from tests import multiplier_ref as MR
from tests.helpers import oracle_batch

pytestmark = pytest.mark.gpu

S = MR.INFO_STRIDE


def _nlp(batch, **kw):
    from quadruped_landing_amd import HybridNLP

    return HybridNLP(batch.model, batch.obj, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf, **kw)


def _meet_every_branch(batch):
    """make_batch's noisy point with several clearance rows active in problem 0, theta on +-pi/2 and h on both bounds."""
    N = batch.N
    batch.Z[0, 1:20 * min(N, 4):20] = -0.3          # yb below the ground at the first knots of problem 0
    batch.Z[-1, 2] = np.pi / 2
    batch.Z[-1, 22] = -np.pi / 2
    batch.Z[0, 19] = 0.001
    if N > 2:
        batch.Z[0, 39] = 0.02
        batch.Z[-1, 39] = 0.001
    return batch


def _run(nlp, batch, **kw):
    """(Z, c, g, lam, lag, info) as host arrays, c and g evaluated by the library at batch.Z"""
    import torch

    Z = nlp.upload_Z(batch.Z)
    c, g = nlp.eval_c(Z), nlp.grad_f(Z)
    lam, lag, info = nlp.estimate_multipliers(Z, c, g, **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (Z, c, g, lam, lag)) + (info.cpu().numpy(),)


def _against_restatement(nlp, batch, out, problems=None, tol=1e-8, **kw):
    Z, c, g, lam, lag, info = out
    ref = oracle_batch(batch, nlp)
    n = nlp.n_nlp
    for b in range(batch.B) if problems is None else problems:
        m = nlp.problem_dims(b)[0]
        cs, zs = slice(nlp.c_off[b], nlp.c_off[b] + m), slice(b * nlp.z_stride, b * nlp.z_stride + n)
        J = MR.batch_jacobian(nlp, ref, b)
        lam_r, lag_r, info_r = MR.estimate(J, Z[zs], c[cs], g[zs], batch.N, **kw)
        el = np.abs(lam[cs] - lam_r).max() / np.abs(lam_r).max()
        eg = np.abs(lag[zs] - lag_r).max() / np.abs(lag_r).max()
        print(f"N={batch.N} problem {b}: {int(info[b, 0])} iterations, active clearance {int(info[b, 5])}, fixed "
              f"{int(info[b, 6])}, wrong signs {int(info[b, 7])}/{int(info[b, 8])}, lam rel err {el:.3e}, lag rel err {eg:.3e}")
        assert el <= tol and eg <= tol
        for k in (0, 5, 6, 7, 8):
            assert info[b, k] == info_r[k], (b, k, info[b, k], info_r[k])
        assert abs(info[b, 1] - info_r[1]) <= 1e-9 * info_r[1]
        assert np.all(info[b, 12:] == 0.0)
        yield b, lam[cs], lag[zs], info[b], info_r, (lag_r, c[cs][-batch.N:])


@pytest.mark.parametrize("row_scaling", [False, True])
@pytest.mark.parametrize("B,N,ragged", [(3, 40, False), (5, 17, True), (2, 80, True), (2, 3, False), (2, 2, False), (2, 64, True),
                                        (2, 65, True)])
def test_iterates_follow_the_numpy_restatement_on_the_oracle_jacobian(B, N, ragged, row_scaling):
    from quadruped_landing_amd import problem_gen as PG

    batch = _meet_every_branch(PG.make_batch(B, N, max(2, N // 3), 1, seed=N, ragged=ragged))
    nlp = _nlp(batch)
    kw = dict(max_iters=3, rel_tol=0.0, row_scaling=row_scaling)
    seen = list(_against_restatement(nlp, batch, _run(nlp, batch, **kw), **kw))
    assert seen[0][3][5] >= 2                                   # several clearance rows active in problem 0
    assert all(x[3][6] >= 2 for x in (seen[0], seen[-1]))       # theta / h on their bounds
    for _, lam, lag, info, info_r, (lag_r, c_clear) in seen:
        # the rest of the report, with what the 1e-8 on lam and lag leaves of each field
        assert abs(info[4] - info_r[4]) <= 1e-8 * np.abs(lag_r).max()
        assert abs(info[10] - info_r[10]) <= 1e-8 * info_r[10]
        assert abs(info[9] - info_r[9]) <= 1e-8 * info_r[10] * np.abs(c_clear).max()
        assert info[11] == info_r[11]
        # and the recurrence's own scalars to what test_gpu_gauss_newton.py grants the same two
        assert abs(info[3] - info_r[3]) <= 1e-6 * info_r[3] + 1e-300
        assert abs(info[2] - info_r[2]) <= 1e-4 * info_r[2] + 1e-300


def test_planted_multipliers_are_recovered_through_the_separate_vjp_kernel():
    import torch
    from quadruped_landing_amd import problem_gen as PG

    batch = PG.make_batch(3, 12, 5, 1, seed=21)
    batch.Z[1, 1:100:20] = -0.3  # some clearance rows active in problem 1
    nlp = _nlp(batch)
    Z = nlp.upload_Z(batch.Z)
    c = nlp.eval_c(Z)
    ch = c.cpu().numpy()
    rng = np.random.default_rng(5)
    lam_star = rng.normal(size=ch.size)
    for b in range(batch.B):
        m = nlp.problem_dims(b)[0]
        clear = slice(nlp.c_off[b] + m - batch.N, nlp.c_off[b] + m)
        lam_star[clear] = np.where(ch[clear] > 1e-6, 0.0, lam_star[clear])
    assert np.count_nonzero(lam_star == 0.0) > 0
    lam_star = torch.from_numpy(lam_star).cuda()
    Jt_star = nlp.jac_t_vec(Z, lam_star)
    g = -Jt_star
    lam, lag, info = nlp.estimate_multipliers(Z, c, g, bound_tol=-1.0, max_iters=20000, rel_tol=1e-11)
    Jt = nlp.jac_t_vec(Z, lam)
    torch.cuda.synchronize()
    info = info.cpu().numpy()
    Jt, Jt_star = Jt.cpu().numpy().reshape(batch.B, -1), Jt_star.cpu().numpy().reshape(batch.B, -1)
    for b in range(batch.B):
        err = np.abs(Jt[b] - Jt_star[b]).max() / np.abs(Jt_star[b]).max()
        print(f"problem {b}: {int(info[b, 0])} iterations, max|lag| {info[b, 4]:.3e}, max|g| {info[b, 11]:.3e}, J'lam rel err {err:.3e}")
        assert info[b, 6] == 0 and info[b, 0] < 20000
        assert info[b, 4] <= 1e-8 * info[b, 11]
        assert err <= 1e-8


def test_converged_estimate_at_a_solved_landing_against_lstsq():
    import torch
    from quadruped_landing_amd import problem_gen as PG

    batch = PG.make_batch(3, 12, 5, 1, seed=3, noise=0.0)
    nlp = _nlp(batch)
    Z0 = nlp.initial_guess()
    Zroll, _ = nlp.solve(Z0.clone(), max_outer=0, rescue_outer=0)  # the roll-out of the initial guess
    Z, sinfo = nlp.solve(Z0.clone())
    max_iters = 20000
    c, g = nlp.eval_c(Z), nlp.grad_f(Z)
    lam, lag, info = nlp.estimate_multipliers(Z, c, g, max_iters=max_iters, rel_tol=1e-9)
    full = g + nlp.jac_t_vec(Z, lam)
    _, _, info_roll = nlp.estimate_multipliers(Zroll, max_iters=max_iters, rel_tol=1e-9)
    torch.cuda.synchronize()
    assert np.all(sinfo.cpu().numpy()[:, 5] == 0)
    Zh, ch, gh, lagh, fullh = (t.cpu().numpy() for t in (Z, c, g, lag, full))
    info, info_roll = info.cpu().numpy(), info_roll.cpu().numpy()
    solved = dataclasses.replace(batch, Z=Zh.reshape(batch.B, -1)[:, : nlp.n_nlp].copy())
    ref = oracle_batch(solved, nlp)
    n = nlp.n_nlp
    for b in range(batch.B):
        m = nlp.problem_dims(b)[0]
        cs, zs = slice(nlp.c_off[b], nlp.c_off[b] + m), slice(b * nlp.z_stride, b * nlp.z_stride + n)
        A, free, w, T = MR.operator(MR.batch_jacobian(nlp, ref, b), Zh[zs], ch[cs], batch.N)
        _, res_ls = MR.lstsq_residual(T, free * gh[zs])
        fr = free > 0
        gmax = np.abs(gh[zs]).max()
        err = np.abs(lagh[zs][fr] - res_ls[fr]).max()
        print(f"problem {b}: {int(info[b, 0])} iterations; dual infeasibility max|lag_free| = {info[b, 4]:.3e} at the solved "
              f"point, {info_roll[b, 4]:.3e} at the roll-out of the initial guess; |lag_free| {np.linalg.norm(lagh[zs][fr]):.6e} "
              f"vs lstsq {np.linalg.norm(res_ls):.6e}; |lag - res_lstsq| = {err:.3e}, max|g| = {gmax:.3e}; fixed "
              f"{int(info[b, 6])}, active clearance {int(info[b, 5])}, wrong signs {int(info[b, 7])}/{int(info[b, 8])}")
        assert info[b, 0] < max_iters
        assert np.linalg.norm(lagh[zs][fr]) <= np.linalg.norm(res_ls) * (1 + 1e-6) + 1e-9
        assert err <= 1e-6 * gmax
        assert np.abs(lagh[zs] - fullh[zs]).max() <= 1e-8 * max(1.0, np.abs(fullh[zs]).max())
        assert info[b, 4] == np.abs(lagh[zs][fr]).max()


def test_masks_locality_of_a_nan_and_no_fixed_variables():
    from quadruped_landing_amd import problem_gen as PG

    batch = PG.make_batch(4, 10, 4, 1, seed=6)
    batch.Z[1, 1::20] = -0.5   # problem 1: body below the ground at every knot -> all clearance rows active
    batch.Z[2, 1::20] = 5.0    # problem 2: far above -> none active
    batch.Z[3, 7] = np.nan     # problem 3: a NaN in the state
    nlp = _nlp(batch)
    kw = dict(max_iters=3, rel_tol=0.0)
    out = _run(nlp, batch, **kw)
    N = batch.N
    x_l, x_u = MR.bounds(N)
    for b, lam, lag, info, *_ in _against_restatement(nlp, batch, out, problems=(0, 1, 2), **kw):
        assert np.all(np.isfinite(lam)) and np.all(np.isfinite(lag))
        c = out[1][nlp.c_off[b]: nlp.c_off[b] + lam.size]
        inactive = c[-N:] > 1e-6
        assert np.all(lam[-N:][inactive] == 0.0) and info[5] == N - inactive.sum()
        fixed = (batch.Z[b] <= x_l + 1e-8) | (batch.Z[b] >= x_u - 1e-8)
        assert fixed.sum() == info[6] > 0
        assert info[4] == np.abs(lag[~fixed]).max()  # the fixed columns are left out ...
        assert np.abs(lag[fixed]).max() > 0          # ... although they hold the bound multipliers
    info = out[5]
    assert info[1, 5] == N and info[2, 5] == 0
    out_free = _run(nlp, batch, bound_tol=-1.0, **kw)
    assert np.all(out_free[5][:3, 6] == 0) and np.all(out_free[5][:3, 8] == 0)
    list(_against_restatement(nlp, batch, out_free, problems=(0, 1, 2), bound_tol=-1.0, **kw))


def test_host_form_is_the_device_form_bit_for_bit():
    from quadruped_landing_amd import problem_gen as PG

    batch = _meet_every_branch(PG.make_batch(3, 17, 6, 1, seed=9))
    nlp = _nlp(batch, z_stride=20 * 17 - 5 + 3)
    kw = dict(max_iters=5, rel_tol=0.0)
    Z, c, g, lam, lag, info = _run(nlp, batch, **kw)
    lam_h, lag_h, info_h = nlp.estimate_multipliers_host(Z, c, g, **kw)
    assert lam_h.tobytes() == lam.tobytes() and lag_h.tobytes() == lag.tobytes() and info_h.tobytes() == info.tobytes()
    lam_only, none_lag, none_info = nlp.estimate_multipliers_host(Z, c, g, want_lag=False, want_info=False, **kw)
    assert none_lag is None and none_info is None and lam_only.tobytes() == lam.tobytes()
    lam_i, none_lag, info_i = nlp.estimate_multipliers_host(Z, c, g, want_lag=False, **kw)
    assert lam_i.tobytes() == lam.tobytes() and info_i.tobytes() == info.tobytes()
    # c and g default to the library's own eval_c and grad_f
    lam_d, lag_d, _ = nlp.estimate_multipliers_host(Z, **kw)
    assert np.abs(lam_d - lam).max() <= 1e-12 * np.abs(lam).max() and np.abs(lag_d - lag).max() <= 1e-12 * np.abs(lag).max()
    # the device form without lag and info
    import torch

    Zd = nlp.upload_Z(batch.Z)
    lam_dev, no_lag, no_info = nlp.estimate_multipliers(Zd, lag=False, info=False, **kw)
    torch.cuda.synchronize()
    assert no_lag is None and no_info is None and lam_dev.cpu().numpy().tobytes() == lam.tobytes()
    # the padding behind n_nlp is never written
    assert np.all(lag.reshape(batch.B, -1)[:, nlp.n_nlp:] == 0.0)


def test_argument_checks_with_a_handle():
    from quadruped_landing_amd import problem_gen as PG
    from quadruped_landing_amd._lib import QLN_ERR_INVALID_ARGUMENT, QlnError

    batch = PG.make_batch(2, 5, 3, 1, seed=0)
    nlp = _nlp(batch)
    Z = nlp.upload_Z(batch.Z)
    for bad in (dict(max_iters=-1), dict(act_tol=-1.0), dict(act_tol=np.nan), dict(rel_tol=-1e-3), dict(rel_tol=np.inf),
                dict(bound_tol=np.nan), dict(bound_tol=np.inf), dict(h_min=0.03), dict(theta_min=2.0)):
        with pytest.raises(QlnError) as e:
            nlp.estimate_multipliers(Z, **bad)
        assert e.value.code == QLN_ERR_INVALID_ARGUMENT, bad
    with pytest.raises(TypeError):
        nlp.estimate_multipliers(Z, max_outer=3)  # not a bound field


def test_problems_too_large_for_lds_are_refused():
    import torch
    from quadruped_landing_amd import num_duals, problem_gen as PG
    from quadruped_landing_amd._lib import QLN_ERR_UNSUPPORTED, QlnError

    def fits(N):  # the documented count: z, dsc, r, q of n_nlp; y, p, s, w of m_nlp at k_trans = 1; the mask
        return 8 * (4 * (20 * N - 5) + 4 * num_duals(N, 1) + N) <= 160 * 1024

    N = max(n for n in range(2, 400) if fits(n))
    assert fits(N) and not fits(N + 1) and 100 < N < 149
    batch = PG.make_batch(2, N, 50, 1, seed=0)
    nlp = _nlp(batch)
    lam, lag, info = nlp.estimate_multipliers(nlp.upload_Z(batch.Z), max_iters=3, rel_tol=0.0)
    torch.cuda.synchronize()
    assert torch.isfinite(lam).all() and torch.isfinite(lag.view(2, -1)[:, : nlp.n_nlp]).all() and torch.isfinite(info).all()
    assert np.all(info.cpu().numpy()[:, 0] == 3)
    batch = PG.make_batch(1, N + 1, 50, 1, seed=0)
    nlp = _nlp(batch)
    with pytest.raises(QlnError) as e:
        nlp.estimate_multipliers(nlp.upload_Z(batch.Z))
    assert e.value.code == QLN_ERR_UNSUPPORTED and "LDS" in str(e.value)


def test_multipliers_random_shapes_property():
    """Randomised shapes (hypothesis): both code paths of the kernel (step blocks cached in registers for N <= 64,
    re-derived for larger N), ragged k_trans / init_mode, strides and alignments, both scaling modes."""
    from hypothesis import given, settings, strategies as st
    from quadruped_landing_amd import problem_gen as PG

    @settings(max_examples=int(__import__("os").environ.get("QLN_FUZZ_EXAMPLES", 12)), deadline=None)
    @given(B=st.integers(1, 6), N=st.integers(2, 100), pad=st.integers(0, 5), align=st.sampled_from([1, 2, 16]),
           scaled=st.booleans(), seed=st.integers(0, 10**6))
    def check(B, N, pad, align, scaled, seed):
        batch = PG.make_batch(B, N, seed=seed, ragged=True) if N > 3 else PG.make_batch(B, N, 2, 1 + seed % 2, seed=seed)
        _meet_every_branch(batch)
        nlp = _nlp(batch, z_stride=(20 * N - 5 + pad) if pad else 0, align=align)
        kw = dict(max_iters=2, rel_tol=0.0, row_scaling=scaled)
        list(_against_restatement(nlp, batch, _run(nlp, batch, **kw), **kw))

    check()


def test_the_example_runs_on_a_small_batch():
    from examples.certify_landings import certify, report

    sinfo, info = certify(8)
    text = report(sinfo, info)
    print(text)
    assert info.shape == (8, S) and "dual infeasibility" in text and "CGLS iterations" in text
    assert np.all(np.isfinite(info)) and np.all(info[:, 0] > 0)


def test_the_example_certifies_the_notebook_problem_and_a_trajectory_file():
    """the --notebook form at B = 1: the GPU-solved notebook problem, then the reference's own data_6.csv read through
    trajectory_io.load_trajectory; a few iterations suffice to run the path"""
    import os

    from examples.certify_landings import certify_notebook, report_notebook

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data_6.csv")
    rows = certify_notebook(path, max_iters=50)
    text = report_notebook(rows)
    print(text)
    assert len(rows) == 2 and rows[1][0] == path
    for _, viol, i in rows:
        assert i.shape == (S,) and np.isfinite(i).all() and np.isfinite(viol) and i[0] <= 50
    assert rows[1][1] < 2e-6  # the file is the point of the reference's run, which reported a violation of 1.493e-6
    assert text.count("CGLS iterations") == 2
