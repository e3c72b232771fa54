"""Every kernel that reads a cost table, held to a table without coincidences.

qln_batch_desc.cost is [cost_batch][N][41], one record Q[15] R[5] q[15] r[5] c per knot; every kernel that reads it indexes
the record by knot, by entry and, when cost_batch == B, by problem.  Every other GPU test runs the notebook's table, under
which fourteen of the fifteen Q are equal, R[0] == R[2], R[1] == R[3], the clock and step-length slots are zero, every stage
record of a phase is the same 41 doubles, Qf == Q and the terminal record's control slots are zero: a kernel that exchanges
two entries, reads a neighbouring knot's record, another problem's table or a stage record at the terminal knot passes all
of them.  tests/cost_cases.py's tables have none of these coincidences (tests/test_cost_cases_host.py, which also holds the
yardsticks used here to each other under such tables), and this file repeats the default-table comparisons with them, each
at the standard its default-table counterpart applies (named where it is applied): bit for bit against the C oracle for f
and grad, RTOL = 1e-8 with _block_rel_err for the Hessian, the bars of tests/test_gpu_hessian_product.py for the product,
ilqr_cases.tolerances for the solver's iterates.  The tracking designs get the same treatment for their diagonal weights."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from oracle import oracle as O
from tests import cost_cases as CC
from tests import hessian_sym as HS
from tests import ilqr_cases as IC
from tests import tracking_cases as TC
from tests import tracking_cov_ref as CR
from tests.helpers import oracle_batch, oracle_model, rel_err

pytestmark = pytest.mark.gpu

TABLES = [False, True]
TABLE_IDS = ["shared", "per-problem"]


def _nlp(batch, **kw):
    from quadruped_landing_amd import HybridNLP

    return HybridNLP(batch.model, batch.obj, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf, **kw)


def _evaluator_batch(B, N, ragged, per_problem, seed):
    """a batch under an evaluator's table (both signs); per-problem runs have uniform k_trans and init_mode, so that only
    the table tells the problems apart"""
    from quadruped_landing_amd import problem_gen as PG

    batch = PG.make_batch(B, N, seed=seed, ragged=True) if ragged else CC.uniform_batch(B, N, seed=seed)
    if per_problem:
        batch.k_trans[:] = batch.k_trans[0]
        batch.init_mode[:] = batch.init_mode[0]
    return CC.with_generic_cost(batch, seed + 1, per_problem, convex=False)


def _rows(nlp, t):
    return t.cpu().numpy().reshape(nlp.B, -1)[:, : nlp.n_nlp]


def _same_bits_as_the_oracle(label, batch, nlp, f, g, nthreads=4):
    """f (B,) and grad (B, n_nlp) of every problem bit for bit the C oracle's (test_value_path_rounds_like_the_reference)"""
    ref = oracle_batch(batch, nlp, want_c=False, want_j=False, want_f=True, want_grad=True, nthreads=nthreads)
    rg = ref["grad"].reshape(batch.B, -1)[:, : nlp.n_nlp]
    ef, eg = rel_err(f, ref["f"]), rel_err(g, rg, floor=1e-300)
    print(f"{label}: f rel err {ef:.3e}, grad rel err {eg:.3e} (bit for bit asked)")
    bad_f = np.nonzero(f != ref["f"])[0]
    assert bad_f.size == 0, (label, "f differs in problems", bad_f[:8].tolist(), ef)
    bad = np.argwhere(g != rg)
    assert bad.size == 0, (label, "grad differs at (problem, knot, entry)", [(int(b), int(j) // 20, int(j) % 20) for b, j in bad[:8]], eg)
    assert np.all(rg[:, 19::20] != 0)  # R_h h + r_h: the step-length slots are read
    return ref


# ---- eval_f, grad_f: the unshared kernels --------------------------------------------------------------------------------
OBJECTIVE_SHAPES = [(4, 2, False, 0), (5, 3, False, 0), (9, 41, False, 0), (9, 41, False, 3), (5, 64, False, 0), (3, 65, False, 0),
                    (7, 130, True, 0)]  # (B, N, ragged, z_pad)


@pytest.mark.parametrize("per_problem", TABLES, ids=TABLE_IDS)
@pytest.mark.parametrize("B,N,ragged,z_pad", OBJECTIVE_SHAPES)
def test_objective_and_gradient_are_the_oracles_bits(B, N, ragged, z_pad, per_problem):
    """k_objective / k_objective_gradient (B < 4096): every problem, every entry"""
    import torch

    batch = _evaluator_batch(B, N, ragged, per_problem, seed=B + N)
    nlp = _nlp(batch, z_stride=(20 * N - 5 + z_pad) if z_pad else 0)
    assert nlp.get_cost().shape == batch.obj.shape
    Z = nlp.upload_Z(batch.Z)
    f, g = nlp.eval_f(Z), nlp.grad_f(Z)
    torch.cuda.synchronize()
    _same_bits_as_the_oracle(f"eval_f/grad_f {B}x{N} pad={z_pad} per_problem={per_problem}", batch, nlp, f.cpu().numpy(), _rows(nlp, g))


# ---- eval_f, grad_f: the shared-table kernels ----------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 7, 33, 64])  # 1, 2, 6 and 10 slice loads
def test_shared_table_kernels_are_the_oracles_bits(N):
    """k_objective_shared (lane = knot, the knot's record in registers) and k_objective_gradient_shared (the table in LDS),
    cost_batch == 1 and B >= 4096: every problem against the oracle, as
    test_shared_cost_table_kernels_at_their_size_limits does."""
    import torch

    B = 4096 + 3
    batch = _evaluator_batch(B, N, False, False, seed=N)
    nlp = _nlp(batch)
    Z = nlp.upload_Z(batch.Z)
    f, g = nlp.eval_f(Z), nlp.grad_f(Z)
    torch.cuda.synchronize()
    _same_bits_as_the_oracle(f"shared-table kernels {B}x{N}", batch, nlp, f.cpu().numpy(), _rows(nlp, g), nthreads=8)


# ---- eval_all and eval_f_and_c -------------------------------------------------------------------------------------------
FUSED_SHAPES = [(4, 2, False), (9, 41, False), (5, 64, False), (3, 65, False), (6, 66, True), (5000, 40, False)]  # one per chunking


@pytest.mark.parametrize("per_problem", TABLES, ids=TABLE_IDS)
@pytest.mark.parametrize("B,N,ragged", FUSED_SHAPES)
def test_fused_launches_give_the_bits_of_the_separate_entry_points_and_of_the_oracle(B, N, ragged, per_problem):
    """qln_eval_all and qln_eval_objective_and_constraint: f and grad are the separate entry points' bits
    (test_eval_all_gives_the_bits_of_the_separate_entry_points,
    test_objective_and_constraint_in_one_launch_give_the_bits_of_the_separate_entry_points) and the oracle's."""
    import torch

    batch = _evaluator_batch(B, N, ragged, per_problem, seed=B + N + 1)
    nlp = _nlp(batch)
    Z = nlp.upload_Z(batch.Z)
    nan = float("nan")
    mk = lambda n: torch.full((n,), nan, dtype=torch.float64, device="cuda")  # noqa: E731
    f, g, c, v = nlp.eval_all(Z, mk(B), mk(nlp.dims.z_total), mk(nlp.dims.c_total), mk(nlp.dims.j_total))
    f3, c3 = nlp.eval_f_and_c(Z, mk(B), mk(nlp.dims.c_total))
    f1, g1 = nlp.eval_f(Z), nlp.grad_f(Z, mk(nlp.dims.z_total))
    c1, v1 = nlp.eval_c_and_jac(Z, mk(nlp.dims.c_total), mk(nlp.dims.j_total))
    torch.cuda.synchronize()
    eq = lambda a, b: torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))  # noqa: E731
    label = f"fused launches {B}x{N} ragged={ragged} per_problem={per_problem}"
    _same_bits_as_the_oracle(label + " (eval_all)", batch, nlp, f.cpu().numpy(), _rows(nlp, g), nthreads=8)
    _same_bits_as_the_oracle(label + " (separate)", batch, nlp, f1.cpu().numpy(), _rows(nlp, g1), nthreads=8)
    assert np.array_equal(f3.cpu().numpy(), f.cpu().numpy()), "eval_f_and_c's objective differs"
    assert eq(f, f1) and eq(g, g1) and eq(c, c1) and eq(c3, c1) and eq(v, v1) and not torch.isnan(f).any()


# ---- Hessian and Hessian-vector product ----------------------------------------------------------------------------------
HESSIAN_SHAPES = [(3, 2, 2, 2), (5, 3, 3, 2), (9, 40, 14, 1), (10, 65, 64, 1), (11, 80, 66, 2)]  # N - 1 <= 64: records in registers


@pytest.mark.parametrize("per_problem", TABLES, ids=TABLE_IDS)
@pytest.mark.parametrize("B,N,k_trans,init_mode", HESSIAN_SHAPES)
def test_hessian_and_its_product_against_hessian_sym(B, N, k_trans, init_mode, per_problem):
    """tests/test_gpu_hessian.py's _check (RTOL = 1e-8 with _block_rel_err; sigma = 0, -1.5, 1 and random values) and
    tests/test_gpu_hessian_product.py's _check (1e-13 against the stored Hessian, 1e-8 against the oracle per row).  By
    name: the objective's (h, h) entries sigma (3 R_h h + 2 r_h) -- zero under the notebook's table -- are non-zero in the
    reference and agree."""
    import torch
    from tests.test_gpu_hessian import RTOL, _batch, _inputs, _run, _segments
    from tests.test_gpu_hessian import _check as check_values
    from tests.test_gpu_hessian_product import _check as check_product

    batch = CC.with_generic_cost(_batch(B, N, k_trans, init_mode, seed=N + k_trans), N + 3, per_problem, convex=False)
    nlp, got, err = check_values(batch, seed=4)
    check_product(batch, seed=5)
    sigma, mu, sig_d, mu_d = _inputs(nlp, 4)
    assert sigma[0] == 0.0 and sigma[1] == -1.5 and sigma[2] == 1.0 and len(set(sigma.tolist())) == B
    hh = 55 * np.arange(N - 1) + HS.step_pattern().index((19, 19))
    ref = HS.batch_hvals(N, batch.k_trans, batch.init_mode, batch.Z, mu, nlp.c_off, sigma, batch.obj)
    ehh = rel_err(got[:, hh], ref[:, hh])
    # the objective's part alone: mu = 0
    obj = _segments(nlp, _run(nlp, nlp.upload_Z(batch.Z), sig_d, torch.zeros_like(mu_d)))
    cost = np.broadcast_to(batch.obj, (B, N, 41))
    want = sigma[:, None] * (3 * cost[:, :-1, 19] * batch.Z[:, 19::20] + 2 * cost[:, :-1, 39])
    assert np.all(want[1:] != 0) and not want[0].any() and np.all(ref[:, hh] != 0)
    eobj = rel_err(obj[1:, hh], want[1:])
    print(f"Hessian {B}x{N} kt={k_trans} per_problem={per_problem}: worst relative error {err:.3e}; (h, h) entries {ehh:.3e}, "
          f"their objective part {eobj:.3e}")
    assert ehh <= RTOL and eobj <= RTOL and not obj[0, hh].any()


# ---- the solver's iterates -----------------------------------------------------------------------------------------------
ONE_ITERATION = [("N12-kt5", False), ("N17-ragged", True), ("N65", True), ("N2", True), ("kt-extremes", True)]


@pytest.mark.parametrize("exact_h", [0, 1])
@pytest.mark.parametrize("name,per_problem", ONE_ITERATION)
def test_one_iteration_under_a_convex_generic_table(name, per_problem, exact_h):
    """stage_ell_row, stage_eval and the sweep of qln_ilqr_kernels.hip: tests/test_gpu_ilqr_iterates.py's _hold"""
    from tests.test_gpu_ilqr_iterates import _hold, _solve_gpu

    batch = CC.solver_case(name, per_problem)
    o = dataclasses.replace(IC.ONE, exact_h_gradient=exact_h)
    _hold(f"generic table, one iteration {name} exact_h={exact_h}", batch, o, _solve_gpu(batch, o))


MULTI_IDS, MULTI = CC.multi_iteration_cases()


@pytest.mark.parametrize("name,per_problem,o", MULTI, ids=MULTI_IDS)
def test_many_iterations_under_a_convex_generic_table(name, per_problem, o):
    """The trial costs of the line search (stage_ell_row: the record across sixteen lanes, entries picked by DPP lane
    immediates) show in decisions only -- the cost the call reports is another read of the record -- and one iteration from
    the guess takes the full step whatever they are.  Twelve and twenty-four iterations of N17-ragged (both init_modes) have
    decisions that a wrong lane flips (tests/test_cost_cases_host.py measures which).  The yardstick alone leaves out 0
    problems of each of these cases, and none of their tolerances rests on a lucky float64 run
    (cost_cases.multi_iteration_cases)."""
    from tests.test_gpu_ilqr_iterates import _hold, _solve_gpu

    batch = CC.solver_case(name, per_problem)
    _hold(f"generic table, {o.max_outer * o.max_inner} iterations {name} exact_h={o.exact_h_gradient}", batch, o, _solve_gpu(batch, o),
          multi=True)


def test_one_iteration_under_the_second_model_and_a_convex_generic_table():
    from tests.test_gpu_ilqr_iterates import _hold, _solve_gpu

    batch = CC.solver_case("N12-kt5", True, IC.SECOND_MODEL)
    _hold("generic table, second model, one iteration N12-kt5", batch, IC.ONE, _solve_gpu(batch, IC.ONE), model=IC.SECOND_MODEL)


@pytest.mark.parametrize("per_problem", TABLES, ids=TABLE_IDS)
def test_objective_a_full_solve_reports_is_the_oracles_at_the_returned_point(per_problem):
    """info[2] of qln_solve (k_solve_report's own read of the table) against the C oracle's eval_f at the returned Z, at
    tests/test_gpu_solve.py's bar for that entry, 1e-9 |f|; the evaluator's eval_f there bit for bit."""
    import torch

    batch = CC.solver_case("N12-kt5", per_problem)
    nlp = _nlp(batch)
    Z, info = nlp.solve(nlp.upload_Z(batch.Z))
    torch.cuda.synchronize()
    inf, Zh = info.cpu().numpy(), _rows(nlp, Z)
    fe = nlp.eval_f(Z).cpu().numpy()
    assert np.all(np.isfinite(Zh))
    for b in range(batch.B):
        cost = batch.obj[b] if per_problem else batch.obj
        f = O.OracleNLP(batch.N, int(batch.k_trans[b]), int(batch.init_mode[b]), batch.x0[b], batch.xf[b], cost,
                        oracle_model(batch.model)).eval_f(Zh[b])
        print(f"full solve b={b} per_problem={per_problem}: status {inf[b, 5]:.0f}, iLQR iterations {inf[b, 1]:.0f}, reported f "
              f"{inf[b, 2]:.12e}, oracle {f:.12e}, relative distance {abs(inf[b, 2] - f) / abs(f):.2e}")
        assert abs(inf[b, 2] - f) <= 1e-9 * abs(f)
        assert fe[b] == f


# ---- sharding ------------------------------------------------------------------------------------------------------------
def test_three_shards_read_their_own_part_of_a_per_problem_table():
    """qln_multi_create_on_one_device, 3 shards of B = 37: f (gathered) and grad (qln_eval_objective_gradient on every
    shard's handle and Z) are the single handle's bits -- shard_desc's cost_begin."""
    import torch
    from quadruped_landing_amd import _lib, multi

    batch = _evaluator_batch(37, 25, False, True, seed=12)
    nlp = _nlp(batch)
    Z1 = nlp.upload_Z(batch.Z)
    f1, g1 = nlp.eval_f(Z1), nlp.grad_f(Z1)
    torch.cuda.synchronize()
    f1, g1 = f1.cpu().numpy(), _rows(nlp, g1)
    _same_bits_as_the_oracle("single handle 37x25", batch, nlp, f1, g1)
    m = multi.MultiNLP(batch.model, batch.obj, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf, devices=[0, 0, 0],
                       one_device=True)
    try:
        m.set_Z(batch.Z)
        m.eval_f()
        m.gather(multi.GATHER_F)
        f, _, _ = m.gathered(viol=False)
        assert np.array_equal(f, f1)
        end = 0
        for r in range(3):
            s = m.shard(r)
            assert s["begin"] == end
            end = s["end"]
            nb = s["end"] - s["begin"]
            dims = _lib.QlnDims()
            _lib.check(_lib.lib().qln_get_dims(s["handle"], C.byref(dims)))
            assert dims.B == nb
            g = torch.full((dims.z_total,), float("nan"), dtype=torch.float64, device="cuda")
            m.synchronize()
            torch.cuda.synchronize()
            _lib.check(_lib.lib().qln_eval_objective_gradient(s["handle"], C.c_void_p(s["Z"]), C.c_void_p(g.data_ptr())))
            m.synchronize()
            torch.cuda.synchronize()
            assert np.array_equal(g.cpu().numpy().reshape(nb, -1)[:, : nlp.n_nlp], g1[s["begin"]: s["end"]]), r
        assert end == 37
    finally:
        m.close()


# ---- host forms and the round trip ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_problem", TABLES, ids=TABLE_IDS)
def test_host_forms_give_the_device_forms_bits_and_the_table_comes_back(per_problem):
    import torch
    from tests.test_gpu_hessian import _inputs, _run

    batch = _evaluator_batch(7, 41, False, per_problem, seed=23)
    nlp = _nlp(batch, exact_hessian=True)
    got = nlp.get_cost()
    assert got.shape == batch.obj.shape and np.array_equal(got.view(np.uint64), batch.obj.view(np.uint64))
    Z = nlp.upload_Z(batch.Z)
    f, g = nlp.eval_f(Z), nlp.grad_f(Z)
    sigma, mu, sig_d, mu_d = _inputs(nlp, 6)
    hd = _run(nlp, Z, sig_d, mu_d, fill=0.0)
    torch.cuda.synchronize()
    assert np.array_equal(nlp.eval_f_host(batch.Z), f.cpu().numpy())
    assert np.array_equal(nlp.grad_f_host(batch.Z).reshape(batch.B, -1)[:, : nlp.n_nlp], _rows(nlp, g))
    hh = nlp.hess_lag_host(batch.Z, sigma, mu)
    assert np.array_equal(hd.view(np.uint64), hh.view(np.uint64))
    _same_bits_as_the_oracle(f"host forms 7x41 per_problem={per_problem}", batch, nlp, f.cpu().numpy(), _rows(nlp, g))


# ---- qln_set_lqr_cost ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_problem", TABLES, ids=TABLE_IDS)
def test_lqr_cost_built_on_device_from_distinct_weights_is_bitwise_the_host_builder(per_problem):
    """test_lqr_cost_built_on_device_is_bitwise_the_host_builder with fifteen distinct Q, five distinct R (R[4] != 0) and a
    Qf that is no multiple of Q"""
    from quadruped_landing_amd import HybridNLP, problem_gen as PG
    from quadruped_landing_amd.quadratic_cost import lqr_objective
    from quadruped_landing_amd.ref_traj import reference_trajectory

    w = CC.DISTINCT_WEIGHTS["lqr_cost"]
    batch = PG.make_batch(96, 33, 11, 2, seed=21, ragged=per_problem)
    nlp = HybridNLP(batch.model, None, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf)
    Z = nlp.upload_Z(batch.Z)
    nlp.set_lqr_cost(w["Q"], w["R"], w["Qf"], CC.DT, per_problem=per_problem)
    Xref, Uref = reference_trajectory(batch.model, batch.N, batch.k_trans, batch.xf, batch.init_mode, CC.DT)
    want = lqr_objective(w["Q"], w["R"], w["Qf"], Xref, Uref) if per_problem else lqr_objective(w["Q"], w["R"], w["Qf"], Xref[0], Uref[0])
    got = nlp.get_cost()
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, ("records differ at", bad[:8].tolist(), rel_err(got, want, floor=1e-300))
    assert np.all(want[..., :-1, 19] == 700.0) and np.all(want[..., :-1, 39] != 0) and not want[..., -1, 15:20].any()
    ref = HybridNLP(batch.model, want, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf)
    assert np.array_equal(nlp.eval_f(Z).cpu().numpy(), ref.eval_f(Z).cpu().numpy())
    assert np.array_equal(nlp.grad_f(Z).cpu().numpy(), ref.grad_f(Z).cpu().numpy())


# ---- the tracking designs' diagonal weights ------------------------------------------------------------------------------
def _tracking_weights():
    w = CC.DISTINCT_WEIGHTS["tracking"]
    return w["Q"], w["R"], w["Qf"]


@pytest.mark.parametrize("B,N,k_trans,init_mode", [(3, 2, 2, 2), (9, 40, 14, 1), (10, 65, 64, 1), (11, 80, 66, 2)])
def test_tracking_gains_under_distinct_weights(B, N, k_trans, init_mode):
    """qln_tracking_lqr: tracking_cases.check_gains_against_numpy at its bar, 1e-10"""
    ek, ep = TC.check_gains_against_numpy(TC.batch(B, N, k_trans, init_mode, seed=N + k_trans), weights=_tracking_weights())
    print(f"tracking_lqr {B}x{N} kt={k_trans}, distinct weights: K {ek:.2e} P {ep:.2e}; bar 1e-10")


def _distinct(monkeypatch):
    """the weights the guarded and limited cases of the tracking family read from tracking_cases, replaced for this test"""
    Qw, Rw, Qfw = _tracking_weights()
    monkeypatch.setattr(TC, "QW", Qw)
    monkeypatch.setattr(TC, "R", Rw)
    monkeypatch.setattr(TC, "QFW", Qfw)


@pytest.mark.parametrize("N,im,B", [(2, 1, 24), (40, 1, 9)])
def test_guarded_tracking_gains_under_distinct_weights(N, im, B, monkeypatch):
    """qln_tracking_lqr_guarded: test_gains_and_covariances_match_the_yardstick's comparison of K and P at its smallest and its
    N = 40 shape (1e-10, or 100 times the yardstick's own float64-to-longdouble distance where that is more)"""
    from tests.test_gpu_tracking_guarded import BAR, _run

    _distinct(monkeypatch)
    nlp, d, h, g, dist = _run.__wrapped__("shape", N, im, B, True)  # not the cached run of the default weights
    errs = (CR.knot_rel(g["Kh"], h["Kr"]), CR.knot_rel(g["Ph"], h["Pr"]))
    bars = [max(BAR, 100 * x) for x in dist[:2]]
    print(f"guarded N={N} B={B}, distinct weights: K {errs[0]:.2e}, P {errs[1]:.2e}; yardstick to longdouble {max(dist[:2]):.2e}; "
          f"bars {max(bars):.2e}")
    assert all(e <= b for e, b in zip(errs, bars)), (errs, bars)
    assert np.array_equal(g["Ph"], np.swapaxes(g["Ph"], -1, -2)) and (h["ev"][:, 0] >= 0).any()


@pytest.mark.parametrize("N,im,B", [(2, 1, 24), (40, 1, 9)])
def test_limited_tracking_gains_under_distinct_weights(N, im, B, monkeypatch):
    """qln_tracking_lqr_limited: test_limited_gains_match_the_riccati_recursion_on_masked_blocks' comparison at its smallest and
    its N = 40 shape, the same bars"""
    from quadruped_landing_amd import nlp as NL
    from tests import rollout_limited_ref as LR
    from tests.test_gpu_rollout_limited import BAR, _run

    _distinct(monkeypatch)
    nlp, d, h, _ = _run.__wrapped__("shape", N, im, B)
    Kg, Pg = nlp.tracking_lqr_limited(d["Zout"], d["sat"], TC.QW, TC.R, TC.QFW, d["ev"], d["model"])
    Kh, Ph = Kg.cpu().numpy(), NL.unpack_cost_to_go(Pg)
    errs = (CR.knot_rel(Kh, h["Kr"]), CR.knot_rel(Ph, h["Pr"]))
    bars = [max(BAR, 100 * x) for x in h["gdist"]]
    print(f"limited N={N} B={B}, distinct weights: K {errs[0]:.2e}, P {errs[1]:.2e}; yardstick to longdouble {max(h['gdist']):.2e}; "
          f"bars {bars}")
    assert all(e <= b for e, b in zip(errs, bars))
    held = ~LR.free_channels(h["sat"])
    assert held.any() and (Kh[held] == 0.0).all() and np.array_equal(Ph, np.swapaxes(Ph, -1, -2))
