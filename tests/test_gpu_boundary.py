"""Every reader of x0 and xf, held to boundary states without coincidences.

qln_batch_desc.x0 / .xf become the [B][30] table BatchParams::bnd.  Its device-side readers: k_constraint_jacobian in every
instantiation that writes c (the hot launch: c, c + J, f + c and eval_all, both formats, every chunking the launch plan
picks), k_initial_guess, k_lqr_cost, k_al_ilqr and k_exact_rollout, the tracking roll-outs when x0 == NULL,
k_sample_drop_states (which writes the x0 half), qln_get_boundary_states, and the shard slicing of qln_multi.cpp.  Every
other GPU test runs the generator's states, under which xf is the same fifteen doubles for every problem, twelve of them
zero, xf[5] == 2 xf[0], and x0[j] == xf[j] in eight slots: a kernel that reads problem 0's xf, a neighbour's, the other half
in an equal slot, two zero slots exchanged, or drops the velocity half passes all of them.  tests/boundary_cases.py's states
have none of these coincidences (tests/test_boundary_cases_host.py, which also shows each such reading to move the
yardsticks by 1e-6 or more in every problem), and this file repeats the default-state comparisons with them, each at the
standard of its default-state counterpart, named where it is applied."""
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import boundary_cases as BC
from tests import cost_cases as CC
from tests import ilqr_cases as IC
from tests import tracking_cases as TC
from tests.helpers import build_c_host, oracle_batch, oracle_model, rel_err, write_problem_file

pytestmark = pytest.mark.gpu

RTOL = 1e-8  # tests/test_gpu_parity.py's, for the clearance rows (the device's sin and libm's differ in the last bit)
FORMATS = ["dense_blocks", "structural"]


def _nlp(batch, **kw):
    from quadruped_landing_amd import HybridNLP

    return HybridNLP(batch.model, batch.obj, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf, **kw)


def _rows(nlp, t):
    return t.cpu().numpy().reshape(nlp.B, -1)[:, : nlp.n_nlp]


def _nan(n):
    import torch

    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


def _same(a, b):
    """bit for bit, NaN padding included"""
    import torch

    return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)) and torch.equal(torch.isnan(a), torch.isnan(b))


def _equality_rows(nlp, batch):
    """mask over the handle's c: every row but the N clearance rows that close each problem's segment"""
    from quadruped_landing_amd import nlp as NL

    mask = np.zeros(nlp.dims.c_total, dtype=bool)
    for b in range(batch.B):
        m = NL.num_duals(batch.N, int(batch.k_trans[b]))
        mask[nlp.c_off[b]: nlp.c_off[b] + m - batch.N] = True
    return mask


def _c_is_the_oracles(label, nlp, batch, ref, eq, c, c_plain):
    """tests/test_gpu_parity.py::test_value_path_rounds_like_the_reference: the equality rows -- the fifteen initial and the
    fourteen terminal rows, the readers of bnd, among them -- are the C oracle's bits; the clearance rows, which read no
    boundary state, are within RTOL of the oracle (sin) and the bits of a handle with the default states at the same Z; the
    padding stays NaN."""
    c = c.cpu().numpy()
    assert np.array_equal(np.isnan(c), np.isnan(ref["c"])), label
    bad = np.nonzero(eq & (c != ref["c"]))[0]
    assert bad.size == 0, (label, "equality rows differ at", bad[:8].tolist(), rel_err(c[eq], ref["c"][eq], floor=1e-300))
    ine = ~eq & ~np.isnan(c)
    assert rel_err(c[ine], ref["c"][ine], floor=1.0) <= RTOL, label
    assert np.array_equal(c[ine], c_plain[ine]), label
    return int(np.count_nonzero(c[ine] != ref["c"][ine]))


# ---- the hot launch -------------------------------------------------------------------------------------------------------
def _evaluators(B, N, ragged, kw, fmt, streamed=False):
    import torch

    batch = BC.evaluator_batch(B, N, ragged, seed=B + N)
    plain = BC.evaluator_batch(B, N, ragged, seed=B + N, generic=False)
    nlp, nlp0 = _nlp(batch, jac_format=fmt, **kw), _nlp(plain, jac_format=fmt, **kw)
    d = nlp.dims
    Z = nlp.upload_Z(batch.Z)
    c0, v0 = nlp0.eval_c_and_jac(Z, _nan(d.c_total), _nan(d.j_total))
    c2, v2 = nlp.eval_c_and_jac(Z, _nan(d.c_total), _nan(d.j_total))
    f4, g4, c4, v4 = nlp.eval_all(Z, _nan(B), _nan(d.z_total), _nan(d.c_total), _nan(d.j_total))
    cs = {"eval_c_and_jac": c2, "eval_all": c4}
    if not streamed:
        cs["eval_c"] = nlp.eval_c(Z, _nan(d.c_total))
        f3, c3 = nlp.eval_f_and_c(Z, _nan(B), _nan(d.c_total))
        cs["eval_f_and_c"] = c3
    torch.cuda.synchronize()
    label = f"{B}x{N} ragged={ragged} {fmt} {kw}"
    ref = oracle_batch(batch, nlp, want_c=True, want_j=False, want_f=True, want_grad=True, nthreads=8)
    eq = _equality_rows(nlp, batch)
    c_plain = c0.cpu().numpy()
    assert not np.array_equal(c_plain[eq], ref["c"][eq])  # the two handles do differ
    last = [_c_is_the_oracles(f"{label} {name}", nlp, batch, ref, eq, c, c_plain) for name, c in cs.items()]
    # f and grad: tests/test_gpu_cost.py::_same_bits_as_the_oracle (they read no boundary state, but ride in the launches that do)
    fs = [f4] + ([] if streamed else [f3])
    for f in fs:
        assert np.array_equal(f.cpu().numpy(), ref["f"]), label
    assert np.array_equal(_rows(nlp, g4), ref["grad"].reshape(B, -1)[:, : nlp.n_nlp]), label
    # the Jacobian's values do not depend on bnd: the bits of the handle with the default states
    assert _same(v2, v0) and _same(v4, v0), label
    print(f"{label}: c of {len(cs)} entry points bit for bit the oracle's in {int(eq.sum())} equality rows; clearance rows that differ "
          f"from libm's in the last bits: {last}")


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("B,N,ragged,kw", BC.EVALUATOR_SHAPES, ids=BC.EVALUATOR_IDS)
def test_every_launch_that_writes_c_reads_its_own_boundary_states(B, N, ragged, kw, fmt):
    """k_constraint_jacobian through eval_c, eval_c_and_jac, eval_f_and_c and eval_all, outputs pre-filled with NaN: one
    shape per launch plan (tests/test_boundary_cases_host.py enumerates which), one with a padded z_stride and align = 7"""
    _evaluators(B, N, ragged, kw, fmt)


def test_streamed_launches_read_their_own_boundary_states():
    """the non-temporal instantiations of the dense c + J and eval_all launches (outputs past 512 MiB)"""
    B, N, ragged, kw = BC.STREAMED_SHAPE
    _evaluators(B, N, ragged, kw, "dense_blocks", streamed=True)


# ---- the initial guess ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 12, 80])
@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
def test_initial_guess_ramps_to_each_problems_own_xf(ragged, N):
    """tests/test_gpu_parity.py::test_initial_guess_on_device_is_bitwise_the_notebook_rule with a per-problem xf: k_trans at 2
    and at N in every batch (N = 2 has no ragged draw: uniform both times)"""
    from quadruped_landing_amd import problem_gen as PG
    from quadruped_landing_amd.ref_traj import reference_trajectory

    B = 70
    batch = BC.evaluator_batch(B, N, ragged and N > 2, seed=N, noise=0.0)
    batch.k_trans[0::3] = 2
    batch.k_trans[1::3] = N
    if ragged:
        batch.init_mode[:] = 1 + np.arange(B) % 2
    _, Uref = reference_trajectory(batch.model, N, batch.k_trans, batch.xf, batch.init_mode, BC.DT)
    want = PG.initial_guess(N, batch.k_trans, batch.x0, batch.xf, Uref)
    nlp = _nlp(batch, z_stride=20 * N + 3)
    got = nlp.initial_guess().cpu().numpy().reshape(B, 20 * N + 3)[:, : nlp.n_nlp]
    bad = np.argwhere(got != want)
    assert bad.size == 0, ("differs at (problem, entry)", bad[:8].tolist())
    after = batch.k_trans < N  # the knots behind the transition hold xf[0:14]; the ramp starts at x0
    assert np.all(want[after, -15:-1] == batch.xf[after, :14]) and np.all(want[:, :15] == batch.x0)


def test_initial_guess_of_the_notebook_problem_with_a_generic_xf():
    from quadruped_landing_amd import problem_gen as PG

    nb = BC.generic_boundary(PG.notebook_problem())
    nlp = _nlp(nb)
    _, Uref = O.reference_trajectory(61, 21, nb.xf[0], 1, BC.DT, oracle_model(nb.model))
    assert np.array_equal(nlp.initial_guess().cpu().numpy(), O.notebook_initial_guess(61, 21, nb.x0[0], nb.xf[0], Uref))


# ---- qln_set_lqr_cost -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_problem", [False, True], ids=["shared", "per-problem"])
def test_lqr_cost_built_on_device_tracks_each_problems_own_xf(per_problem):
    """tests/test_gpu_cost.py::test_lqr_cost_built_on_device_from_distinct_weights_is_bitwise_the_host_builder with a
    per-problem xterm: the per-problem table is the host builder's on each problem's xf, the shared one problem 0's"""
    from quadruped_landing_amd.quadratic_cost import lqr_objective
    from quadruped_landing_amd.ref_traj import reference_trajectory

    w = CC.DISTINCT_WEIGHTS["lqr_cost"]
    batch = BC.evaluator_batch(96, 33, per_problem, seed=21)
    batch.obj = None
    nlp = _nlp(batch)
    Z = nlp.upload_Z(batch.Z)
    nlp.set_lqr_cost(w["Q"], w["R"], w["Qf"], BC.DT, per_problem=per_problem)
    Xref, Uref = reference_trajectory(batch.model, batch.N, batch.k_trans, batch.xf, batch.init_mode, BC.DT)
    want = lqr_objective(w["Q"], w["R"], w["Qf"], Xref, Uref) if per_problem else lqr_objective(w["Q"], w["R"], w["Qf"], Xref[0], Uref[0])
    got = nlp.get_cost()
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, ("records differ at", bad[:8].tolist(), rel_err(got, want, floor=1e-300))
    if per_problem:
        assert len({t[-1].tobytes() for t in want}) == batch.B  # a terminal record per xf
    batch.obj = want
    ref = _nlp(batch)
    assert np.array_equal(ref.get_cost(), want)
    assert np.array_equal(nlp.eval_f(Z).cpu().numpy(), ref.eval_f(Z).cpu().numpy())
    assert np.array_equal(nlp.grad_f(Z).cpu().numpy(), ref.grad_f(Z).cpu().numpy())


# ---- the solver -----------------------------------------------------------------------------------------------------------
SOLVER_CASES = BC.solver_cases()


@pytest.mark.parametrize("case", list(SOLVER_CASES))
def test_solver_iterates_under_generic_boundary_states(case):
    """tests/test_gpu_ilqr_iterates.py's _hold -- controls, counts, step lengths, mu and rho against tests/ilqr_ref.py in
    longdouble, bounds from ilqr_cases.tolerances -- on the cases tests/test_boundary_cases_host.py qualified: no problem
    is left out"""
    from tests.test_gpu_ilqr_iterates import _hold, _solve_gpu

    name, o, model, cost = SOLVER_CASES[case]
    batch = BC.solver_batch(name, model, cost)
    ratio = _hold(f"generic states {case}", batch, o, _solve_gpu(batch, o), model=model, multi=o is IC.TWELVE, may_leave_out=False)
    print(f"generic states {case}: worst distance {ratio:.2f} times the float64-to-longdouble distance (bound {IC.TOL_MARGIN:g})")


def test_violation_a_full_solve_reports_measures_the_terminal_rows_against_each_problems_own_xf():
    """info[3] of qln_solve (k_exact_rollout's own read of xf) after a full solve: it holds the terminal-state error
    max |x_N[0:14] - xf[b, 0:14]| recomputed on the host from the returned Z, and is the evaluator's violation at
    tests/test_gpu_solve.py's bar for that entry (>= qln_constraint_violation, <= max(that, the bounds) (1 + 1e-12)).
    Generic states make a problem infeasible in the slots no control reaches (the standing foot), so the terminal rows ARE
    the largest in some problems: there the entry is the terminal error to the same bar."""
    import torch
    from tests.test_gpu_solve import _judge

    batch = BC.solver_batch("N12-kt5", None, "kept")
    nlp = _nlp(batch)
    Z, info = nlp.solve(nlp.upload_Z(batch.Z))
    torch.cuda.synchronize()
    inf = info.cpu().numpy()
    viol, f, bviol, c, Zh = _judge(nlp, Z)
    assert np.all(np.isfinite(Zh)) and np.array_equal(inf[:, 2], f)
    term = np.max(np.abs(Zh[:, -15:-1] - batch.xf[:, :14]), axis=1)
    assert np.all(inf[:, 3] >= viol) and np.all(inf[:, 3] <= np.maximum(viol, bviol) * (1 + 1e-12) + 1e-300)
    assert np.all(inf[:, 3] >= term)
    for b in range(batch.B):
        o = O.OracleNLP(batch.N, int(batch.k_trans[b]), int(batch.init_mode[b]), batch.x0[b], batch.xf[b], batch.obj, oracle_model(batch.model))
        seg = nlp.split_c(c, b)
        assert np.array_equal(seg[:29], o.eval_c(Zh[b])[:29]) and not seg[:15].any()
        assert np.max(np.abs(seg[15:29])) == term[b]
    dominant = term >= np.maximum(viol, bviol)
    print(f"full solve under generic states: status {inf[:, 5].astype(int).tolist()}, reported violation {inf[:, 3]}, terminal "
          f"error {term}; the terminal rows are the largest in {int(dominant.sum())} of {batch.B} problems")
    assert dominant.any() and np.all(inf[dominant, 3] <= term[dominant] * (1 + 1e-12))


# ---- roll-outs from the handle's own x0 -----------------------------------------------------------------------------------
LIMITS = [-3.0, 3.0, -3.0, 30.0, -20.0, 20.0, 0.0, 40.0]


def _tuple_equal(a, b):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None and not np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True):
            return False
    return True


@pytest.mark.parametrize("N", [2, 12])
def test_rollouts_without_x0_start_from_each_problems_own_x0(N):
    """x0 = None against the same call with the handle's x0 passed as a device tensor, bit for bit: B = 70 (two blocks of
    64 lanes), closed loop.  No yardstick is involved: every problem is compared."""
    import torch

    B = 70
    batch = BC.evaluator_batch(B, N, N > 2, seed=N + 1)
    nlp = _nlp(batch)
    rng = np.random.default_rng(N)
    Zref, K = nlp.upload_Z(batch.Z), TC.gains(nlp, N)
    x0 = torch.from_numpy(batch.x0.copy()).cuda()
    model = torch.from_numpy(np.tile(TC.SECOND, (B, 1))).cuda()
    Lg = torch.from_numpy(0.05 * rng.normal(size=(B, N, 15, 3))).cuda()
    H = rng.normal(size=(3, 15))
    xhat0 = torch.from_numpy(batch.x0 + 0.01 * rng.normal(size=(B, 15))).cuda()
    calls = {
        "tracking_rollout": lambda x: nlp.tracking_rollout(Zref, K, x),
        "tracking_rollout_model": lambda x: nlp.tracking_rollout_model(Zref, K, x, model),
        "tracking_rollout_guarded": lambda x: nlp.tracking_rollout_guarded(Zref, K, x, model),
        "tracking_rollout_limited": lambda x: nlp.tracking_rollout_limited(Zref, LIMITS, K, x, model),
        "tracking_rollout_limited (guarded)": lambda x: nlp.tracking_rollout_limited(Zref, LIMITS, K, x, model, guarded=True),
    }
    for guarded in (False, True):
        for xh in (xhat0, None):
            calls[f"tracking_rollout_estimated guarded={guarded} xhat0={'given' if xh is not None else 'None'}"] = (
                lambda x, g=guarded, xh=xh: nlp.tracking_rollout_estimated(Zref, K, Lg, H, None, None, x, xh, model, guarded=g,
                                                                           with_innovations=True))
    for name, call in calls.items():
        own, given = call(None), call(x0)
        torch.cuda.synchronize()
        assert _tuple_equal(own, given), name
        Zout = _rows(nlp, own[0] if isinstance(own, tuple) else own)
        assert np.array_equal(Zout[:, :15], batch.x0), name  # the first knot is the problem's own x0, every slot
    # and the neighbour's x0 gives another roll-out in every problem: the comparison above can tell
    other = nlp.tracking_rollout(Zref, K, torch.roll(x0, 1, dims=0))
    assert np.all(np.any(_rows(nlp, other) != _rows(nlp, nlp.tracking_rollout(Zref, K)), axis=1))


# ---- the sampler and the read-back ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("im", [1, 2])
def test_sampler_redraws_x0_and_leaves_each_problems_xf_alone(im):
    """tests/test_gpu_sampler.py::test_device_drop_states_are_bit_identical_to_the_host_generator on a handle whose xf
    differs per problem: B = 300 (two blocks of 256 threads)"""
    from quadruped_landing_amd import problem_gen as PG

    B, seed = 300, 17
    host = PG.make_batch(B, 12, 5, im, seed=seed, build_obj=False)
    batch = BC.generic_boundary(PG.make_batch(B, 12, 5, im, seed=seed, build_obj=False))
    nlp = _nlp(batch)
    x0, xf = nlp.boundary_states()
    assert np.array_equal(x0, batch.x0) and np.array_equal(xf, batch.xf)
    drawn = nlp.sample_drop_states(PG.drop_state_sampler(seed, host.model))
    assert np.array_equal(drawn, host.x0)
    x0, xf = nlp.boundary_states()
    assert np.array_equal(x0, host.x0) and np.array_equal(xf.view(np.uint64), batch.xf.view(np.uint64))


# ---- shards ---------------------------------------------------------------------------------------------------------------
def test_three_shards_read_their_own_part_of_the_boundary_table():
    """qln_multi_create_on_one_device, 3 shards of B = 37, on the pattern of
    test_three_shards_read_their_own_part_of_a_per_problem_table: c and f (gathered), the initial guess and one solver
    iteration of every shard are the single handle's bits -- shard_desc's x0 / xf slices"""
    import torch
    from quadruped_landing_amd import multi

    batch = BC.with_cost(BC.evaluator_batch(37, 25, False, seed=37 + 25, noise=0.0), "rebuilt")
    nlp = _nlp(batch)
    Z1 = nlp.upload_Z(batch.Z)
    c1, f1 = nlp.eval_c(Z1).cpu().numpy(), nlp.eval_f(Z1).cpu().numpy()
    g1 = _rows(nlp, nlp.initial_guess())
    o = IC.ONE.gpu_kwargs()
    Zs, info1 = nlp.solve(nlp.upload_Z(batch.Z), **o)
    torch.cuda.synchronize()
    Zs, info1 = _rows(nlp, Zs), info1.cpu().numpy()
    ref = oracle_batch(batch, nlp, want_j=False, want_f=True)
    eq = _equality_rows(nlp, batch)
    assert np.array_equal(c1[eq], ref["c"][eq]) and np.array_equal(f1, ref["f"])  # the single handle is the oracle's
    m = multi.MultiNLP(batch.model, batch.obj, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf, devices=[0, 0, 0],
                       one_device=True)
    try:
        def shard_rows(name_):
            m.synchronize()
            torch.cuda.synchronize()
            parts, end = [], 0
            for r in range(3):
                s = m.shard(r)
                assert s["begin"] == end and s["end"] > s["begin"]
                end = s["end"]
                parts.append(m.shard_tensor(r, name_).cpu().numpy().reshape(s["end"] - s["begin"], -1)[:, : nlp.n_nlp])
            assert end == 37 and len({len(p) for p in parts}) > 1  # unequal shards
            return np.concatenate(parts)

        m.set_Z(batch.Z)
        m.eval_c_and_jac(with_jacobian=False)
        m.eval_f()
        m.gather(multi.GATHER_F | multi.GATHER_C)
        f, _, c = m.gathered(viol=False, c=True)
        assert np.array_equal(f, f1)
        for b in range(batch.B):
            mm = nlp.problem_dims(b)[0]
            assert np.array_equal(c[m.c_off[b]: m.c_off[b] + mm], c1[nlp.c_off[b]: nlp.c_off[b] + mm]), b
        info = m.solve(**o)
        assert np.array_equal(info[:, :10], info1[:, :10])
        assert np.array_equal(shard_rows("Z"), Zs)
        m.initial_guess()
        assert np.array_equal(shard_rows("Z"), g1)
    finally:
        m.close()


# ---- host forms -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", BC.HOST_FORM_SHAPES)
def test_host_forms_give_the_device_forms_bits(B, N):
    """eval_c_host (N = 41: one workgroup per 16-knot chunk, the plan of a caller that waits) and qln_solve_host against
    eval_c and qln_solve; c's equality rows the oracle's"""
    import torch
    from quadruped_landing_amd import _lib

    batch = BC.evaluator_batch(B, N, False, seed=B + N, noise=0.0)
    nlp = _nlp(batch)
    Z = nlp.upload_Z(batch.Z)
    c = nlp.eval_c(Z, _nan(nlp.dims.c_total)).cpu().numpy()
    ch = nlp.eval_c_host(batch.Z)
    ok = ~np.isnan(c)
    assert np.array_equal(ch[ok], c[ok])
    ref = oracle_batch(batch, nlp, want_j=False)
    eq = _equality_rows(nlp, batch)
    assert np.array_equal(ch[eq], ref["c"][eq])
    Zs, info = nlp.solve(nlp.upload_Z(batch.Z))
    torch.cuda.synchronize()
    Zh = nlp._host_Z(batch.Z).copy()
    ih = np.zeros((B, _lib.SOLVE_INFO_STRIDE))
    _lib.check(_lib.lib().qln_solve_host(nlp._h, Zh.ctypes.data, None, ih.ctypes.data))
    assert np.array_equal(Zh.reshape(B, -1)[:, : nlp.n_nlp], _rows(nlp, Zs))
    assert np.array_equal(ih[:, :10], info.cpu().numpy()[:, :10])


def test_c_host_reads_the_files_own_xf(tmp_path):
    """tests/host_c/moi_host.c (its problem file carries x0[15] and xf[15]) at one generic problem, at a point whose
    dynamics rows are zero -- the trajectory one solver iteration returns -- so that the largest equality residual it prints
    is a terminal row's: that figure and f are the oracle's to the last digit"""
    import torch

    batch = BC.solver_batch("N12-kt5", None, "kept")
    nlp = _nlp(batch)
    Z, _ = nlp.solve(nlp.upload_Z(batch.Z), **IC.ONE.gpu_kwargs())
    torch.cuda.synchronize()
    Zh = _rows(nlp, Z)
    b = 3
    one = BC.evaluator_batch(1, 12, False, seed=0)
    one.k_trans[:], one.init_mode[:] = batch.k_trans[b], batch.init_mode[b]
    one.x0, one.xf, one.obj = batch.x0[b: b + 1], batch.xf[b: b + 1], batch.obj
    o = O.OracleNLP(12, int(one.k_trans[0]), int(one.init_mode[0]), one.x0[0], one.xf[0], one.obj, oracle_model(one.model))
    c = o.eval_c(Zh[b])
    neq = c.size - 12
    worst = int(np.argmax(np.abs(c[:neq])))
    assert 15 <= worst < 29, worst  # a terminal row
    pf = tmp_path / "problem.txt"
    write_problem_file(pf, one, Zh[b])
    out = subprocess.run([build_c_host(tmp_path), str(pf)], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0
    kv = dict(line.split("=", 1) for line in out.stdout.splitlines() if "=" in line)
    assert kv["totals_match"] == "1" and kv["guards_intact"] == "1"
    assert float(kv["max_abs_c_eq"]) == np.max(np.abs(c[:neq])) == abs(Zh[b, -15 + worst - 15] - one.xf[0, worst - 15])
    assert float(kv["f"]) == o.eval_f(Zh[b])
