"""tests/boundary_cases.py without a GPU: the coincidences of the generator's boundary states, stated on the generator;
that the generic states have none of them; that every wrong reading in MUTATIONS moves the yardsticks' c by exactly 0 under
the default states and by 1e-6 or more, in every problem, under the generic ones; that the yardsticks
tests/test_gpu_boundary.py leans on -- the C oracle, oracle/np_oracle.py, problem_gen.initial_guess, lqr_objective,
tests/ilqr_ref.py -- agree with each other and qualify under such states; and which launch plans of the hot kernel the
shapes of the GPU module reach."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import np_oracle as NP
from oracle import oracle as O
from quadruped_landing_amd import problem_gen as PG
from quadruped_landing_amd.quadratic_cost import lqr_objective
from quadruped_landing_amd.ref_traj import reference_trajectory
from tests import boundary_cases as BC
from tests import cost_cases as CC
from tests import ilqr_cases as IC
from tests import ilqr_ref as IR
from tests.helpers import oracle_model

TEETH = 1e-6  # the least a wrong reading moves c, in every problem it can show in: bit for bit comparisons see 1e-16


# ---- the coincidences, on the generator -----------------------------------------------------------------------------------
def _default_batches():
    return [PG.make_batch(9, 12, 5, 1, seed=3), PG.make_batch(9, 12, 5, 2, seed=3), PG.make_batch(16, 12, seed=3, ragged=True),
            PG.notebook_problem()]


def test_the_generators_boundary_states_have_every_coincidence():
    """what generic_boundary is there to avoid; whoever changes the generator meets it here"""
    for batch in _default_batches():
        xf, x0, im = batch.xf, batch.x0, batch.init_mode
        assert np.array_equal(xf, np.tile(PG.terminal_state(batch.model), (batch.B, 1)))  # one xf for every problem
        zero = [j for j in range(15) if j not in BC.XF_NONZERO]
        assert len(zero) == 12 and not xf[:, zero].any() and np.all(xf[:, BC.XF_NONZERO] != 0)
        assert np.array_equal(xf[:, 5], 2 * xf[:, 0])                                     # bit for bit
        assert not xf[:, 7:15].any()                                                      # velocities and clock
        one, two = im == 1, im == 2
        assert np.all(x0[one][:, BC.X0_IS_XF_MODE1] == xf[one][:, BC.X0_IS_XF_MODE1])
        assert np.all(x0[two][:, BC.X0_IS_XF_MODE2] == xf[two][:, BC.X0_IS_XF_MODE2])
        assert not x0[one][:, BC.X0_ZERO_MODE1].any()
        assert np.all(x0[one][:, BC.X0_SHARED_MODE1] == x0[one][:1, BC.X0_SHARED_MODE1]) if one.any() else True
        assert x0[:, BC.SWAP_SLOT].tolist() == xf[:, BC.SWAP_SLOT].tolist() == [0.0] * batch.B
        assert not xf[:, list(BC.ZERO_PAIR)].any()
    b1 = _default_batches()[0]
    free = [j for j in range(15) if j not in BC.X0_SHARED_MODE1]
    assert free == [2, 6, 8, 9] and all(len(set(b1.x0[:, j].tolist())) == b1.B for j in free)


@pytest.mark.parametrize("ragged", [False, True])
def test_generic_states_have_none_of_them(ragged):
    batch = BC.evaluator_batch(70, 12, ragged, seed=1)
    x0, xf = batch.x0, batch.xf
    assert x0.shape == xf.shape == (70, 15) and x0.flags.c_contiguous and xf.flags.c_contiguous
    both = np.concatenate([x0, xf], axis=1).reshape(-1)
    assert np.all(np.isfinite(both)) and np.all(both != 0) and len(set(both.tolist())) == 30 * 70
    assert np.all(x0 != xf) and np.all(xf[:, 5] != 2 * xf[:, 0])
    plain = BC.evaluator_batch(70, 12, ragged, seed=1, generic=False)
    assert np.array_equal(plain.Z, batch.Z) and np.array_equal(plain.k_trans, batch.k_trans)  # the guess stays
    assert np.max(np.abs(x0 - plain.x0)) < 6 * BC.SCALE and np.max(np.abs(xf - plain.xf)) < 6 * BC.SCALE
    again = BC.evaluator_batch(70, 12, ragged, seed=1)
    assert np.array_equal(again.x0, x0) and np.array_equal(again.xf, xf)
    other = BC.generic_boundary(BC.evaluator_batch(70, 12, ragged, seed=1, generic=False), BC.SEED + 1)
    assert not np.any(other.xf == xf) and not np.any(other.x0 == x0)
    # the rebuilt cost is a table per problem, no two alike
    tab = BC.rebuilt_cost(batch)
    assert tab.shape == (70, 12, 41) and len({t.tobytes() for t in tab}) == 70


# ---- the mutations --------------------------------------------------------------------------------------------------------
def _mutation_batches():
    """(label, generic batch, default-state twin) of every shape tests/test_gpu_boundary.py compares c at"""
    out = []
    for (B, N, ragged, _), label in zip(BC.EVALUATOR_SHAPES + [BC.STREAMED_SHAPE], BC.EVALUATOR_IDS + ["streamed"]):
        out.append((label, BC.evaluator_batch(B, N, ragged, seed=B + N), BC.evaluator_batch(B, N, ragged, seed=B + N, generic=False)))
    for B, N in BC.HOST_FORM_SHAPES + [(37, 25)]:
        out.append((f"{B}x{N}", BC.evaluator_batch(B, N, False, seed=B + N), BC.evaluator_batch(B, N, False, seed=B + N, generic=False)))
    for name in ("N12-kt5", "N17-ragged", "N65", "N2", "kt-extremes"):
        out.append((name, BC.solver_batch(name, None, "kept"), IC.shape(name)))
    return out


def test_every_mutation_moves_c_under_generic_states_and_by_exactly_zero_under_the_default_ones():
    """C oracle, every shape: per problem max |c(mutated) - c(true)|.  The minimum over problems and shapes of each
    mutation is what DESIGN.md section 3 quotes."""
    worst = {name: np.inf for name in BC.MUTATIONS}
    for label, generic, plain in _mutation_batches():
        cg, cp = BC.oracle_c(generic), BC.oracle_c(plain)
        for name in BC.MUTATIONS:
            d0 = BC.mutation_effect(plain, name, cp)
            assert d0.max() == 0.0, (label, name, d0.max())
            d = BC.mutation_effect(generic, name, cg)
            worst[name] = min(worst[name], d.min())
            assert d.min() >= TEETH, (label, name, d.min(), int(d.argmin()))
    for name, w in worst.items():
        print(f"mutation '{name}': 0 under the default states; least per-problem max |delta c| under the generic ones {w:.2e}")


@pytest.mark.parametrize("ragged", [False, True])
def test_mutations_through_the_numpy_oracle(ragged):
    """the same statement by oracle/np_oracle.py, and its agreement with the C oracle at generic states at
    tests/test_oracle_property.py's bar, 1e-12 max(1, |c|)"""
    generic, plain = BC.evaluator_batch(6, 12, ragged, seed=4), BC.evaluator_batch(6, 12, ragged, seed=4, generic=False)

    def c_np(batch, x0, xf):
        return [NP.eval_c(batch.N, int(batch.k_trans[b]), int(batch.init_mode[b]), x0[b], xf[b], batch.Z[b]) for b in range(batch.B)]

    cg, cp = c_np(generic, generic.x0, generic.xf), c_np(plain, plain.x0, plain.xf)
    for a, b in zip(BC.oracle_c(generic), cg):
        assert a.shape == b.shape and np.max(np.abs(a - b)) <= 1e-12 * max(1.0, np.max(np.abs(b)))
    for name, (fn, blind) in BC.MUTATIONS.items():
        d0 = [np.max(np.abs(a - b)) for a, b in zip(c_np(plain, *fn(plain.x0, plain.xf)), cp)]
        assert max(d0) == 0.0, name
        d = np.delete([np.max(np.abs(a - b)) for a, b in zip(c_np(generic, *fn(generic.x0, generic.xf)), cg)], list(blind))
        assert d.min() >= TEETH, (name, d.min())


# ---- the host builders with a per-problem xf -----------------------------------------------------------------------------
@pytest.mark.parametrize("ragged", [False, True])
def test_initial_guess_and_lqr_objective_take_a_per_problem_xf(ragged):
    """problem_gen.initial_guess, reference_trajectory and lqr_objective on xf of shape (B, 15), against the oracle's
    one-problem restatements (notebook_initial_guess, reference_trajectory, lqr_cost_table) problem by problem, bit for bit"""
    batch = BC.evaluator_batch(7, 12, ragged, seed=8, noise=0.0)
    w = CC.DISTINCT_WEIGHTS["lqr_cost"]
    Xref, Uref = reference_trajectory(batch.model, batch.N, batch.k_trans, batch.xf, batch.init_mode, BC.DT)
    Z0 = PG.initial_guess(batch.N, batch.k_trans, batch.x0, batch.xf, Uref)
    tab = lqr_objective(w["Q"], w["R"], w["Qf"], Xref, Uref)
    assert Z0.shape == (7, 20 * 12 - 5) and tab.shape == (7, 12, 41)
    m = oracle_model(batch.model)
    for b in range(batch.B):
        kt, im = int(batch.k_trans[b]), int(batch.init_mode[b])
        Xo, Uo = O.reference_trajectory(batch.N, kt, batch.xf[b], im, BC.DT, m)
        assert np.array_equal(Xo, Xref[b]) and np.array_equal(Uo, Uref[b])
        assert np.array_equal(Z0[b], O.notebook_initial_guess(batch.N, kt, batch.x0[b], batch.xf[b], Uo)), b
        assert np.array_equal(tab[b], O.lqr_cost_table(w["Q"], w["R"], w["Qf"], Xo, Uo)), b
    assert np.array_equal(BC.rebuilt_cost(batch), lqr_objective(PG.Q_DIAG, PG.R_DIAG, PG.Q_DIAG, Xref, Uref))


# ---- the solver cases -----------------------------------------------------------------------------------------------------
STABLE = 0.25  # tests/test_cost_cases_host.py's: the share of a tolerance that one-ulp neighbours of the guess may use
SOLVER_CASES = BC.solver_cases()


@pytest.mark.parametrize("case", list(SOLVER_CASES))
def test_solver_cases_are_unambiguous_and_their_tolerance_is_no_lucky_sample(case):
    """cost_cases.multi_iteration_cases' rule for every solver run of tests/test_gpu_boundary.py: float64 and longdouble
    agree in every decision with margins above 1e-9 in every problem (none is left out), and float64 runs whose guess is
    moved by one ulp per entry take the same decisions and stay within STABLE of the tolerance the kernel gets."""
    name, o, model, cost = SOLVER_CASES[case]
    batch = BC.solver_batch(name, model, cost)
    left_out, spread, share = 0, 0.0, 0.0
    with IC.np_model(model):
        P, U0 = IC.problems(batch)
        for b in range(batch.B):
            r64, r80 = IC.reference_pair(P[b], U0[b], o, keep_trials=False)
            left_out += IC.ambiguous(r64, r80)
            tol_u, tol_j, eu, _ = IC.tolerances(r64, r80, o)
            spread = max(spread, eu)
            rng = np.random.default_rng(b)
            for _ in range(2):
                r = IR.solve(P[b], U0[b] * (1 + 2.0**-52 * rng.integers(-1, 2, size=U0[b].shape)), o, keep_trials=False)
                assert r.decisions() == r80.decisions(), (case, b)
                share = max(share, IR.control_error(r.U, r80.U, o.h_max) / tol_u, IR.relative_error(r.J, r80.J) / tol_j)
    print(f"generic states {case}: float64 spread {spread:.2e}, ambiguous {left_out} of {batch.B}; one-ulp neighbours use "
          f"{share:.3f} of the tolerance (bound {STABLE})")
    assert left_out == 0 and share <= STABLE


@pytest.mark.parametrize("name", ["N12-kt5", "N17-ragged", "N65", "N2", "kt-extremes"])
def test_solver_yardstick_sees_every_mutation(name):
    """the first iteration of tests/ilqr_ref.py moves by more than cost_cases' TEETH = 1e-5 (four orders above the tolerance)
    in some problem for every mutation the solver can see -- it reads xf[0:14] in the terminal rows and x0 at the first
    knot -- and by exactly 0 under the default states"""
    generic, plain = BC.solver_batch(name, None, "kept"), IC.shape(name)
    for label, (fn, blind) in BC.MUTATIONS.items():
        for batch, want_zero in ((plain, True), (generic, False)):
            x0, xf = fn(batch.x0, batch.xf)
            moved = []
            for b in range(batch.B):
                if b in blind:
                    continue
                p = IR.Problem.of_batch(batch, b)
                u0 = IR.controls_of(batch.Z[b], batch.N)
                q = IR.Problem(p.N, p.k_trans, p.init_mode, x0[b], xf[b], p.cost)
                moved.append(IR.control_error(IR.solve(q, u0, IC.ONE).U, IR.solve(p, u0, IC.ONE).U, IC.ONE.h_max))
            if want_zero:
                assert max(moved) == 0.0, (name, label)
            else:
                print(f"generic states {name}: '{label}' moves the first iteration by {min(moved):.2e} .. {max(moved):.2e}")
                assert max(moved) > 1e-5, (name, label, moved)


# ---- the launch plans the evaluator shapes reach --------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = {"c": (1, 0, 0, 0), "cJ": (1, 1, 0, 0), "fc": (1, 0, 1, 0), "all": (1, 1, 1, 1)}  # the WITH_C requests of the API

# Instantiations with non-temporal stores that no shape here reaches: outputs past 512 MiB.  c alone and f + c stream by
# their rows (29 300 problems of N = 130, 600 MB of Z); the structural format at 71 values a knot (24 238 problems of
# N = 40).  They differ from their STREAM = 0 twins, which are covered, in the store instructions alone.
NOT_REACHED = {"<5,40,2,1,0,0,0,1,0>", "<8,64,2,1,0,0,0,1,0>", "<5,40,2,1,0,0,0,1,1>", "<8,64,2,1,0,0,0,1,1>",
               "<0,40,1,1,1,1,0,1,0>", "<0,64,1,1,1,1,0,1,0>", "<0,40,1,1,1,1,0,1,1>"}


def _plans(tmp_path, requests):
    """the template arguments plan_launch() answers each (nb, N, format, kt_max, outputs, prefer_latency) with"""
    from tests.test_launch_plan_host import HIPCC

    exe = str(tmp_path / "launch_plan_print")
    if not os.path.exists(exe):
        subprocess.run([HIPCC, "-O1", "-std=c++17", "--offload-host-only", "--offload-arch=gfx950", "-o", exe,
                        os.path.join(ROOT, "tests", "launch_plan_print.cpp")], check=True)
    text = "".join(f"{nb} {N} {fmt} {kt} {' '.join(map(str, OUTPUTS[out]))} {lat} 0 -1 -1 0\n" for nb, N, fmt, kt, out, lat in requests)
    got = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(got) == len(requests)
    return [re.match(r"<[\d,]+>", l).group(0) for l in got]


def test_evaluator_shapes_reach_every_plan_of_a_launch_that_writes_c(tmp_path):
    """Every instantiation of k_constraint_jacobian with WITH_C that plan_launch() can answer a request of the API with --
    swept over nb, N, both formats, the four output sets, and the latency preference where the API sets it (eval_c_host
    alone asks for c with it) -- is reached by a shape of tests/test_gpu_boundary.py, but for NOT_REACHED."""
    sweep = [(nb, N, fmt, min(14, N), out, 0) for nb in (1, 4, 256, 257, 5000, 5736, 7400, 25000, 100000) for N in range(2, 140)
             for fmt in (0, 1) for out in OUTPUTS]
    sweep += [(nb, N, fmt, min(14, N), "c", 1) for nb in (1, 256, 257) for N in range(2, 140) for fmt in (0, 1)]
    possible = set(_plans(tmp_path, sweep))
    mine = []
    for B, N, ragged, _ in BC.EVALUATOR_SHAPES:
        kt = int(BC.evaluator_batch(B, N, ragged, seed=B + N, generic=False).k_trans.max()) if B < 100 else 14
        mine += [(B, N, fmt, kt, out, 0) for fmt in (0, 1) for out in OUTPUTS]
    B, N, _, _ = BC.STREAMED_SHAPE
    mine += [(B, N, 0, 14, out, 0) for out in ("cJ", "all")]
    mine += [(B, N, 0, 5, "c", 1) for B, N in BC.HOST_FORM_SHAPES]
    reached = set(_plans(tmp_path, mine))
    print(f"{len(possible)} plans write c; the shapes reach {len(reached)}: {sorted(reached)}")
    assert reached <= possible and NOT_REACHED <= possible and not (NOT_REACHED & reached)
    assert possible - reached == NOT_REACHED, sorted(possible - reached - NOT_REACHED)
