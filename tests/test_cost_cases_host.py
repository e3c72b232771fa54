"""tests/cost_cases.py without a GPU: that its tables and weights have none of the notebook table's coincidences, and that
the yardsticks tests/test_gpu_cost.py leans on -- the C oracle, oracle/np_oracle.py, tests/hessian_sym.py, tests/ilqr_ref.py
-- agree with each other, and with evidence of their own, under such a table.

The notebook's table, lqr_objective(Q_DIAG, R_DIAG, Q_DIAG, Xref, Uref): fourteen equal Q, R[0] == R[2], R[1] == R[3], zeros
in the clock and step-length slots, one record per phase, Qf == Q, zeros in the terminal record's control slots.  A kernel
that exchanges two entries of a record, reads a neighbouring knot's record or a stage record at the terminal knot computes
the right bits under it; the last test here states that as an exact zero."""
import itertools

import numpy as np
import pytest

from oracle import np_oracle as NP
from oracle import oracle as O
from quadruped_landing_amd import problem_gen as PG
from quadruped_landing_amd.planar_quadruped import PlanarQuadruped
from tests import cost_cases as CC
from tests import ilqr_cases as IC
from tests import ilqr_ref as IR
from tests.helpers import oracle_model
from tests.tracking_cases import SECOND_MODEL


# ---- no coincidences -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("convex", [False, True])
@pytest.mark.parametrize("per_problem", [False, True])
def test_generic_tables_have_no_coincidences(per_problem, convex):
    batch = CC.uniform_batch(5, 9, 4, 1, seed=1)
    tab = CC.generic_cost(batch, 3, per_problem, convex)
    assert tab.shape == ((5, 9, 41) if per_problem else (9, 41)) and tab.flags.c_contiguous and np.all(np.isfinite(tab))
    rec = tab.reshape(-1, 41)
    for r in rec:
        assert len(set(r.tolist())) == 41 and not (r == 0).any()      # within a record: no two entries equal, none zero
    assert len({r.tobytes() for r in rec}) == len(rec)                # no two records equal ...
    drawn = np.ones(41, dtype=bool)
    drawn[15:20] = drawn[35:40] = False                               # (the terminal records share their sentinels)
    for a, b in itertools.combinations(range(len(rec)), 2):
        assert not np.any(rec[a, drawn] == rec[b, drawn]), (a, b)     # ... in no drawn slot
    t = tab.reshape(-1, 9, 41)
    assert np.all(t[:, 8, None, :15] != t[:, :8, :15])                # the terminal Q is no stage knot's
    s = CC.terminal_sentinels()
    assert np.array_equal(t[:, 8, 15:20], np.broadcast_to(s[:5], (len(t), 5)))
    assert np.array_equal(t[:, 8, 35:40], np.broadcast_to(s[5:], (len(t), 5)))
    assert len(set(np.abs(s).tolist())) == 10 and np.abs(s).min() >= 1e6 and (s > 0).any() and (s < 0).any()
    if convex:
        assert np.all(t[:, :, :15] > 0) and np.all(t[:, :8, 15:20] > 0)
    else:
        assert (t[:, :, :20] < 0).any() and (t[:, :, :20] > 0).any()
    # the same arguments give the same table, another seed another one
    assert np.array_equal(tab, CC.generic_cost(batch, 3, per_problem, convex))
    assert not np.any(tab[..., :8, :] == CC.generic_cost(batch, 4, per_problem, convex)[..., :8, :])


def test_the_notebook_table_has_every_one_of_them():
    """what generic_cost is there to avoid, stated on make_batch's own table"""
    tab = PG.make_batch(2, 9, 4, 1, seed=1).obj
    assert tab.shape == (9, 41)
    assert len(set(tab[0, :14].tolist())) == 1 and tab[0, 15] == tab[0, 17] and tab[0, 16] == tab[0, 18]
    assert not tab[:, [14, 19, 34, 39]].any()
    assert len({r.tobytes() for r in tab[:8]}) == 2                   # one record per phase
    assert np.array_equal(tab[8, :15], tab[0, :15]) and not tab[8, 15:20].any() and not tab[8, 35:40].any()


@pytest.mark.parametrize("name", ["tracking", "lqr_cost"])
def test_distinct_weights_are_distinct_and_near_the_weights_they_replace(name):
    w, old = CC.DISTINCT_WEIGHTS[name], CC.REPLACED[name]
    assert w["Q"].shape == w["Qf"].shape == (15,) and w["R"].shape == old["R"].shape
    allw = np.concatenate([w["Q"], w["R"], w["Qf"]])
    assert len(set(allw.tolist())) == allw.size and np.all(allw > 0)
    for k in ("Q", "R", "Qf"):
        had = old[k] != 0
        ratio = w[k][had] / old[k][had]
        assert np.all(ratio <= 3.0) and np.all(ratio >= 1 / 3.0), k
    assert w["Q"][14] != 0 and w["Qf"][14] != 0
    if name == "lqr_cost":
        assert w["R"].size == 5 and w["R"][4] != 0


# ---- the C oracle and the numpy oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("convex", [False, True])
@pytest.mark.parametrize("model", [None, SECOND_MODEL], ids=["default-model", "second-model"])
def test_c_oracle_objective_and_gradient_agree_with_the_numpy_oracle(model, convex):
    """eval_f at tests/test_oracle_property.py's standard, 1e-10 max(1, |f|).  np_oracle has no gradient: grad_f! is held, at
    the same standard per entry, to complex-step derivatives of np_oracle.eval_f; on the step-length rows minus the knot's
    stage cost, which grad_f! leaves out (quirk Q2).  The terminal record's control slots are not read."""
    m = model or PlanarQuadruped()
    batch = CC.with_generic_cost(PG.make_batch(3, 12, 5, 1, seed=9, model=m), 11, True, convex)
    N, n = batch.N, 20 * batch.N - 5
    for b in range(batch.B):
        cost, Z = batch.obj[b], batch.Z[b]
        o = O.OracleNLP(N, 5, 1, batch.x0[b], batch.xf[b], cost, oracle_model(m))
        f, g = o.eval_f(Z), o.grad_f(Z)
        fn = NP.eval_f(N, cost, Z)
        assert abs(f - fn) <= 1e-10 * max(1.0, abs(fn))
        d = np.zeros(n)
        for j in range(n):
            Zc = Z.astype(complex)
            Zc[j] += 1e-30j
            d[j] = NP.eval_f(N, cost, Zc).imag / 1e-30
        for k in range(N - 1):
            d[20 * k + 19] -= NP.stagecost(cost[k], Z[20 * k: 20 * k + 15], Z[20 * k + 15: 20 * k + 20])
        assert np.max(np.abs(g - d)) <= 1e-10 * max(1.0, np.max(np.abs(d)))
        assert np.all(g[19::20] != 0)  # R_h h + r_h: zero under the notebook table
        other = cost.copy()
        other[N - 1, 15:20], other[N - 1, 35:40] = 3.0, -7.0
        o2 = O.OracleNLP(N, 5, 1, batch.x0[b], batch.xf[b], other, oracle_model(m))
        assert o2.eval_f(Z) == f and np.array_equal(o2.grad_f(Z), g)


# ---- the Hessian's yardstick ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("convex", [False, True])
@pytest.mark.parametrize("model", [None, SECOND_MODEL], ids=["default-model", "second-model"])
def test_hessian_sym_against_differences_of_the_oracle_under_a_generic_table(model, convex):
    """tests/test_model_host.py's comparison, whose (h, h) entries are second differences of the oracle's eval_f: they are
    sigma (3 R_h h + 2 r_h), non-zero here."""
    from tests import hessian_sym as HS
    from tests.test_model_host import _hessian_sym_against_differences

    with IC.np_model(model):
        batch, mu, sigma, H, tol = _hessian_sym_against_differences(model or PlanarQuadruped(), 5, convex=convex)
        H0 = HS.problem_hvals(batch.N, 3, 1, batch.Z[0], 0 * mu, sigma, batch.obj)  # the objective's part alone
    hh = 55 * np.arange(batch.N - 1) + HS.step_pattern().index((19, 19))
    cost, h = batch.obj, batch.Z[0, 19::20]
    want = sigma * (3 * cost[:-1, 19] * h + 2 * cost[:-1, 39])
    assert np.all(want != 0) and np.sum(np.abs(want) > 1000 * tol[hh]) >= 3  # the comparison above can tell them from zero
    assert np.max(np.abs(H0[hh] - want)) <= 1e-14 * np.max(np.abs(want))


# ---- the solver's yardstick ----------------------------------------------------------------------------------------------
def _case():
    batch = CC.solver_case("N12-kt5", per_problem=True)
    return batch, *IC.problems(batch)


@pytest.mark.parametrize("exact_h", [0, 1])
@pytest.mark.parametrize("multipliers", [False, True])
def test_slope_of_the_line_search_cost_under_a_generic_table(multipliers, exact_h):
    """test_slope_of_the_line_search_cost_is_the_sweeps_d_dot_Qu of tests/test_ilqr_ref_host.py, its bound unchanged"""
    import dataclasses

    from tests.test_ilqr_ref_host import SLOPE_RTOL, WIDE, _multipliers, _slope

    _, P, U0 = _case()
    o = IR.Options(exact_h_gradient=exact_h, theta_min=-0.3 if multipliers else IR.Options.theta_min, **WIDE)
    for b in range(2):
        lam, leq = _multipliers(P[b], U0[b], dataclasses.replace(o, exact_h_gradient=0)) if multipliers else (None, None)
        pred, fd, corr = _slope(P[b], U0[b], o, lam, leq)
        print(f"generic table b={b} multipliers={multipliers} exact_h={exact_h}: d.Qu = {pred:.12e}, difference quotient "
              f"{fd:.12e}, relative distance {abs(pred - fd) / abs(pred):.2e}, Richardson correction {corr / abs(pred):.2e}")
        assert pred < 0
        assert abs(pred - fd) <= SLOPE_RTOL * abs(pred) + corr


def test_sweep_is_the_dense_kkt_solution_under_a_generic_table():
    from tests.test_ilqr_ref_host import _sweep_against_dense_kkt

    _, P, U0 = _case()
    _sweep_against_dense_kkt("generic table N12-kt5 b=0", P[0], U0[0])


MULTI_IDS, MULTI = CC.multi_iteration_cases()


STABLE = 0.25  # the share of a case's tolerance that float64 runs from one-ulp neighbours of the guess may use


@pytest.mark.parametrize("name,per_problem,o", MULTI, ids=MULTI_IDS)
def test_many_iteration_cases_are_unambiguous_and_their_tolerance_is_no_lucky_sample(name, per_problem, o):
    """The multi-iteration cases of tests/test_gpu_cost.py (cost_cases.multi_iteration_cases states the rule): float64 and
    longdouble agree in every decision with margins above 1e-9, so the GPU test leaves no problem out on the yardstick's
    account; and two float64 runs whose guess is moved by one ulp per entry take the same decisions and stay within STABLE
    of the tolerance the kernel gets from the unmoved run."""
    batch = CC.solver_case(name, per_problem)
    P, U0 = IC.problems(batch)
    left_out, spread, share = 0, 0.0, 0.0
    for b in range(batch.B):
        r64, r80 = IC.reference_pair(P[b], U0[b], o, keep_trials=False)
        left_out += IC.ambiguous(r64, r80)
        tol_u, tol_j, eu, _ = IC.tolerances(r64, r80, o)
        spread = max(spread, eu)
        rng = np.random.default_rng(b)
        for _ in range(2):
            r = IR.solve(P[b], U0[b] * (1 + 2.0**-52 * rng.integers(-1, 2, size=U0[b].shape)), o, keep_trials=False)
            assert r.decisions() == r80.decisions()
            share = max(share, IR.control_error(r.U, r80.U, o.h_max) / tol_u, IR.relative_error(r.J, r80.J) / tol_j)
    print(f"generic table {name} x{o.max_outer * o.max_inner} exact_h={o.exact_h_gradient}: float64 spread {spread:.2e}, ambiguous "
          f"{left_out} of {batch.B}; one-ulp neighbours use {share:.3f} of the tolerance (bound {STABLE})")
    assert left_out == 0 and share <= STABLE


def _solve_with_merit_table(monkeypatch, p, U0, o, swap):
    """the yardstick with entries swap[0] and swap[1] of every record exchanged in the trial costs of the line search ALONE"""
    import dataclasses

    orig = IR.trial_costs

    def trial_costs(q, *a, **kw):
        tab = q.cost.copy()
        tab[:, list(swap)] = q.cost[:, list(swap)[::-1]]
        return orig(dataclasses.replace(q, cost=tab), *a, **kw)

    with monkeypatch.context() as m:
        m.setattr(IR, "trial_costs", trial_costs)
        return IR.solve(p, U0, o, keep_trials=False)


@pytest.mark.parametrize("swap", [(0, 1), (3, 4), (6, 7), (10, 11), (12, 13), (26, 27)], ids=str)
def test_twelve_ragged_iterations_see_a_fault_in_the_trial_merit_alone(swap, monkeypatch):
    """The kernel forms the line search's trial costs from a record spread over sixteen lanes (stage_ell_row); the cost it
    reports comes from another read of the record.  A wrong lane there changes nothing but decisions: which step length
    wins, whether a step is accepted.  One iteration from the guess does not see it (the full step wins by a wide margin);
    twelve iterations of N17-ragged do, in some problem, for every exchange of neighbouring entries of Q and q -- both
    init_modes are needed: the standing foot's states are constant zeros.  Measured for every pair (i, i + 1), i < 13, of Q:
    between 1 and 8 of the 8 problems change a decision or move by more than 1e-9; six pairs are asserted here."""
    batch = CC.solver_case("N17-ragged", True)
    P, U0 = IC.problems(batch)
    seen = 0
    for b in range(batch.B):
        base = IR.solve(P[b], U0[b], IC.TWELVE, keep_trials=False)
        r = _solve_with_merit_table(monkeypatch, P[b], U0[b], IC.TWELVE, swap)
        seen += r.decisions() != base.decisions() or IR.control_error(r.U, base.U, IC.TWELVE.h_max) > 1e-9
        one = _solve_with_merit_table(monkeypatch, P[b], U0[b], IC.ONE, swap)
        assert one.decisions() == IR.solve(P[b], U0[b], IC.ONE, keep_trials=False).decisions()
    print(f"merit-only exchange {swap}: seen by {seen} of {batch.B} problems in twelve iterations, by none in one")
    assert seen >= 1


def _faults(cost):
    """three ways of reading a table wrongly, as tables"""
    N = cost.shape[-2]
    no_h = cost.copy()
    no_h[..., : N - 1, 19] = no_h[..., : N - 1, 39] = 0.0           # the step-length slots R[4], r[4] never read
    swapped = cost.copy()
    swapped[..., [1, 8]] = cost[..., [8, 1]]                          # two entries of Q exchanged
    shifted = cost.copy()
    shifted[..., : N - 1, :] = np.roll(cost[..., : N - 1, :], -1, axis=-2)  # knot k reads knot k + 1's stage record
    return {"R[4], r[4] zeroed": no_h, "Q[1] <-> Q[8]": swapped, "stage records shifted by one knot": shifted}


TEETH = 1e-5  # four orders above the tolerance the kernel is held to (100 x a float64 spread <= 1.6e-12)


@pytest.mark.parametrize("name,per_problem", [("N12-kt5", False), ("N17-ragged", True), ("N65", True)])
def test_generic_table_has_teeth_and_the_notebook_table_has_none(name, per_problem):
    """Each fault moves the yardstick's first iteration, in every problem, by more than TEETH in the measure the kernel is
    held in.  Under make_batch's table the same exchange of Q[1] and Q[8] moves it by exactly 0.  (Q[3] <-> Q[10] would
    move nothing under either table: the standing foot's states, which the controls cannot reach.)"""
    batch = CC.solver_case(name, per_problem)
    P, U0 = IC.problems(batch)
    base = [IR.solve(P[b], U0[b], IC.ONE) for b in range(batch.B)]
    for what, tab in _faults(batch.obj).items():
        moved = [IR.control_error(IR.solve(IR.Problem.of_batch(batch, b, cost=tab), U0[b], IC.ONE).U, base[b].U, IC.ONE.h_max)
                 for b in range(batch.B)]
        print(f"generic table {name}: {what} moves the first iteration by {min(moved):.2e} .. {max(moved):.2e}")
        assert min(moved) > TEETH, (what, moved)
    plain = IC.shape(name)
    P0, V0 = IC.problems(plain)
    tab = _faults(plain.obj)["Q[1] <-> Q[8]"]
    for b in range(plain.B):
        a, c = IR.solve(P0[b], V0[b], IC.ONE), IR.solve(IR.Problem.of_batch(plain, b, cost=tab), V0[b], IC.ONE)
        assert IR.control_error(c.U, a.U, IC.ONE.h_max) == 0.0 and np.array_equal(c.U, a.U)
