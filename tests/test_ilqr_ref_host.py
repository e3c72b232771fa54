"""tests/ilqr_ref.py, the numpy yardstick of qln_solve's iterates, held to evidence of its own (no GPU): the slope of its
line-search cost, a dense KKT solve of the sweep's linear-quadratic problem, the teeth of the clock-weight case, the
agreement of its float64 and longdouble runs in every discrete decision, and -- for the control-flow cases of
tests/ilqr_cases.py -- that every case and prefix is unambiguous, reaches the branches it names, and that the rescue phase does
what the header says of it."""
import dataclasses
import os

import numpy as np
import pytest

from tests import ilqr_cases as IC
from tests import ilqr_ref as IR

LD = np.longdouble
WIDE = dict(h_min=-1.0, h_max=1.0)  # (the restatement alone takes a negative bound) no clamp of h acts: the slope identity and the KKT problem have no box


def test_longdouble_is_the_80_bit_type():
    IR.require_extended_precision()


def _linearise(p, U0, o, lam=None, leq=None, clock_row="rollout", mu=IR.MU0):
    """the sweep of one iteration at the guess, in longdouble"""
    U = np.array(U0, dtype=LD)
    U[:, 4] = np.clip(U[:, 4], LD(o.h_min), LD(o.h_max))
    X = IR.rollout(p, U, LD)
    lam = np.zeros((p.N, 6), dtype=LD) if lam is None else lam
    leq = np.zeros(15, dtype=LD) if leq is None else leq
    rho = LD(o.rho0)
    tm = IR.stage_terms(p, o, X, U, lam, leq, rho, U[:, 4], LD)
    gz, Hzz = IR.stage_derivatives(p, o, X, U, leq, rho, tm, LD)
    blocks = IR.step_blocks(p, X, U, LD, clock_row)
    sw = IR.backward(p, o, U, gz, Hzz, blocks, mu, LD)
    assert sw.ok
    return X, U, lam, leq, rho, tm, gz, Hzz, blocks, sw


def _slope(p, U0, o, lam=None, leq=None, clock_row="rollout"):
    """(sum_k d_k . Qu_k, central difference of the line-search cost at alpha = 0 with its own error estimate)"""
    X, U, lam, leq, rho, tm, gz, Hzz, blocks, sw = _linearise(p, U0, o, lam, leq, clock_row)
    assert not sw.clamped.any()
    pred = np.sum(sw.d * sw.Qu)

    def cd(delta):
        J = IR.trial_costs(p, o, X, U, sw, [LD(delta), LD(-delta)], lam, leq, rho, LD)[0]
        return (J[0] - J[1]) / (2 * LD(delta))

    c1, c2 = cd(2e-5), cd(1e-5)
    fd = c2 + (c2 - c1) / 3  # Richardson: the central difference's error is even in delta
    return float(pred), float(fd), float(abs(c2 - c1))


# The central difference at delta = 1e-5, extrapolated once: what is left is the delta^4 term and the rounding of the cost,
# eps_longdouble |J| / delta = 1e-14 |J|; |J| and the slope are of the same order (a Newton step removes most of the cost).
# The bound is 1e-9 of the slope plus the extrapolation's own correction, which measures the truncation.
SLOPE_RTOL = 1e-9


def _multipliers(p, U0, o):
    """non-zero multipliers: those of two outer iterations of the method itself"""
    r = IR.solve(p, U0, dataclasses.replace(o, max_outer=2, max_inner=2), LD)
    assert np.any(r.leq[:14] != 0) and r.leq[14] != 0
    return r.lam, r.leq


@pytest.mark.parametrize("exact_h", [0, 1])
@pytest.mark.parametrize("multipliers", [False, True])
@pytest.mark.parametrize("case", ["N12-kt5", "N17-ragged", "clock"])
def test_slope_of_the_line_search_cost_is_the_sweeps_d_dot_Qu(case, multipliers, exact_h):
    batch = IC.clock_case() if case == "clock" else IC.shape(case)
    P, U0 = IC.problems(batch)
    o = IR.Options(exact_h_gradient=exact_h, theta_min=-0.3 if multipliers else IR.Options.theta_min, **WIDE)
    for b in range(2):
        lam, leq = _multipliers(P[b], U0[b], dataclasses.replace(o, exact_h_gradient=0)) if multipliers else (None, None)
        assert not multipliers or np.any(lam != 0)  # (theta_min = -0.3 is violated from the drop state on)
        pred, fd, corr = _slope(P[b], U0[b], o, lam, leq)
        print(f"{case} b={b} multipliers={multipliers} exact_h={exact_h}: d.Qu = {pred:.12e}, difference quotient {fd:.12e}, "
              f"relative distance {abs(pred - fd) / abs(pred):.2e}, Richardson correction {corr / abs(pred):.2e}")
        assert pred < 0
        assert abs(pred - fd) <= SLOPE_RTOL * abs(pred) + corr


def _lu_solve(M, rhs):
    """dense solve by Gaussian elimination with partial pivoting in the dtype of M, refined once; returns the solution and
    the size of the refinement's correction, which estimates the first solution's error"""
    n = len(M)
    A = M.copy()
    perm = np.arange(n)
    for j in range(n):
        piv = j + int(np.argmax(np.abs(A[j:, j])))
        if piv != j:
            A[[j, piv]] = A[[piv, j]]
            perm[[j, piv]] = perm[[piv, j]]
        A[j + 1:, j] /= A[j, j]
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j, j + 1:])

    def solve(b):
        y = b[perm].copy()
        for i in range(n):
            y[i] -= A[i, :i] @ y[:i]
        for i in range(n - 1, -1, -1):
            y[i] = (y[i] - A[i, i + 1:] @ y[i + 1:]) / A[i, i]
        return y

    x = solve(rhs)
    dx = solve(rhs - M @ x)
    return x + dx, dx


@pytest.mark.parametrize("case,b", [("N12-kt5", 0), ("N17-ragged", 1), ("clock", 0), ("N2", 0)])
def test_sweep_is_the_dense_kkt_solution_of_its_quadratic_problem(case, b):
    """With no clamp acting, du_k = d_k + K_k dx_k rolled through dx_{k+1} = A_k dx_k + B_k du_k from dx_1 = 0 minimises
    sum_k (g_k' dz_k + dz_k' H_k dz_k / 2) with mu and h_prox on the control blocks: the same du as one dense solve of the KKT
    system over all dx, du and the multipliers of the linearised dynamics (tests/tracking_ref.kkt's pattern).
    Tolerance: the correction of one step of iterative refinement of the dense solve estimates that solve's error (the
    conditioning of the problem times the rounding of longdouble); the sweep is the same problem solved in the same
    arithmetic by other means, so it is held to 100 times that estimate."""
    batch = IC.clock_case() if case == "clock" else IC.shape(case)
    P, U0 = IC.problems(batch)
    _sweep_against_dense_kkt(f"{case} b={b}", P[b], U0[b])


def _sweep_against_dense_kkt(label, p, U0):
    """the comparison of test_sweep_is_the_dense_kkt_solution_of_its_quadratic_problem on one problem"""
    o = IR.Options(**WIDE)
    lam, leq = _multipliers(p, U0, o)
    X, U, lam, leq, rho, tm, gz, Hzz, blocks, sw = _linearise(p, U0, o, lam, leq)
    assert not sw.clamped.any()
    N = p.N
    nx, nu = 15 * N, 5 * (N - 1)
    nv = nx + nu
    H, g = np.zeros((nv, nv), dtype=LD), np.zeros(nv, dtype=LD)
    reg = LD(IR.MU0) * np.eye(5, dtype=LD)
    reg[4, 4] += LD(o.h_prox)
    for k in range(N):
        xs = slice(15 * k, 15 * k + 15)
        H[xs, xs], g[xs] = Hzz[k, :15, :15], gz[k, :15]
        if k < N - 1:
            us = slice(nx + 5 * k, nx + 5 * k + 5)
            H[us, us], g[us] = Hzz[k, 15:, 15:] + reg, gz[k, 15:]
            H[us, xs], H[xs, us] = Hzz[k, 15:, :15], Hzz[k, :15, 15:]
    C = np.zeros((nx, nv), dtype=LD)
    C[:15, :15] = np.eye(15)
    for k in range(N - 1):
        r = slice(15 * (k + 1), 15 * (k + 2))
        C[r, 15 * k: 15 * k + 15] = blocks[k][:, :15]
        C[r, 15 * (k + 1): 15 * (k + 2)] = -np.eye(15)
        C[r, nx + 5 * k: nx + 5 * k + 5] = blocks[k][:, 15:]
    M = np.block([[H, C.T], [C, np.zeros((nx, nx), dtype=LD)]])
    sol, corr = _lu_solve(M, np.concatenate([-g, np.zeros(nx, dtype=LD)]))
    du_kkt = sol[nx:nv].reshape(N - 1, 5)
    du_err = np.abs(corr[nx:nv]).reshape(N - 1, 5)
    dx = np.zeros(15, dtype=LD)
    du = np.zeros((N - 1, 5), dtype=LD)
    for k in range(N - 1):
        du[k] = sw.d[k] + sw.K[k] @ dx
        dx = blocks[k][:, :15] @ dx + blocks[k][:, 15:] @ du[k]
    e = IR.control_error(U + du, U + du_kkt, 0.02)
    tol = 100 * IR.control_error(U + du_kkt + du_err, U + du_kkt, 0.02)
    print(f"{label}: sweep against dense KKT e = {e:.2e}, refinement correction x 100 = {tol:.2e}, step size "
          f"{IR.control_error(U + du_kkt, U, 0.02):.2e}")
    assert tol < 1e-9  # the estimate itself is small: the dense solve is a usable yardstick
    assert e <= tol


def test_clock_weight_case_has_teeth():
    """The case test_gpu_ilqr_iterates.py uses for the clock row can see it: with the jump knot's clock row masked (the
    evaluator's block), the sweep no longer differentiates the cost the line search evaluates -- the slope identity fails --
    and the first iteration's controls move by more than 1000 times the tolerance the kernel is held to."""
    batch = IC.clock_case()
    P, U0 = IC.problems(batch)
    wide = IR.Options(**WIDE)
    for b in range(batch.B):
        pred, fd, corr = _slope(P[b], U0[b], wide, clock_row="masked")
        bound = SLOPE_RTOL * abs(pred) + corr
        r64, r80 = IC.reference_pair(P[b], U0[b], IC.ONE)
        masked = IR.solve(P[b], U0[b], IC.ONE, LD, clock_row="masked")
        tol_u = IC.tolerances(r64, r80, IC.ONE)[0]
        a = r80.iterations[0].a_star
        moved = IR.control_error(masked.iterations[0].U_try[a], r80.U, IC.ONE.h_max)
        print(f"clock b={b}: masked slope off by {abs(pred - fd) / abs(pred):.2e} (bound {bound / abs(pred):.2e}); first-iteration "
              f"controls moved by {moved:.2e} = {moved / tol_u:.1e} x the tolerance {tol_u:.1e}")
        assert a >= 0
        assert abs(pred - fd) > bound
        assert moved > 1000 * tol_u


@pytest.mark.parametrize("case,model", [("N12-kt5", None), ("N17-ragged", None), ("N12-kt5", IC.SECOND_MODEL)],
                         ids=["N12-kt5", "N17-ragged", "N12-kt5-second-model"])
def test_float64_and_longdouble_agree_in_every_decision_of_twelve_iterations(case, model):
    """The multi-iteration cases of the GPU test: the two precisions take the same step lengths, accept and reject alike and
    end with the same mu, rho, counts and status, and no decision of the longdouble run is closer than 1e-9: none of the
    problems is ambiguous, so the GPU test leaves none out on the yardstick's account."""
    batch = IC.shape(case, model)
    with IC.np_model(model):
        P, U0 = IC.problems(batch)
        left_out = 0
        for b in range(batch.B):
            r64, r80 = IC.reference_pair(P[b], U0[b], IC.TWELVE, keep_trials=False)
            kind = min(r80.margins, key=lambda m: m[2])
            print(f"{case} b={b}: outer {r80.outer} iters {r80.iters} status {r80.status} rho {r80.rho:g} alpha {r80.alpha:g}; spread "
                  f"e(U) = {IR.control_error(r64.U, r80.U, 0.02):.2e}, J {IR.relative_error(r64.J, r80.J):.2e}; smallest margin "
                  f"{kind[2]:.2e} ({kind[1]}, iteration {kind[0]})")
            assert r80.iters == 12 or r80.status == 0 or any(i.inner_break for i in r80.iterations)
            left_out += IC.ambiguous(r64, r80)
        assert left_out == 0


# ---- the control flow: stop tests, failure paths, the rescue phase ------------------------------------------------------
def _join(pair):
    """a longdouble stored as (hi, lo) float64"""
    return pair[0].astype(LD) + pair[1].astype(LD)


def test_without_a_rescue_the_restatement_is_unchanged_to_the_bit():
    """tests/golden/ilqr_ref_bits.npz was written by the restatement as it stood before it had a rescue phase
    (tests/golden/make_ilqr_ref_bits.py): controls, multipliers and report of the ONE and TWELVE cases in both precisions.
    rescue_outer defaults to 0, and with 0 nothing of those runs has moved by a bit."""
    from tests.golden import make_ilqr_ref_bits as G

    assert IR.Options().rescue_outer == 0 and IC.ONE.rescue_outer == 0 and IC.TWELVE.rescue_outer == 0
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ilqr_ref_bits.npz")) as gold:
        n = 0
        for name, which in G.CASES:
            now = G.record(name, which)
            n += len(now)
            for key, value in now.items():
                assert value.dtype == gold[key].dtype and np.array_equal(value, gold[key], equal_nan=True), key
            b = f"{name}/{which}/0"
            assert np.array_equal(_join(now[b + "/U80"]), _join(gold[b + "/U80"]))  # (the split is exact: see G.split)
        assert n == len(gold.files)


def _branch_table(rows):
    width = max(len(name) for name, _ in rows)
    print(" " * width + "  " + " ".join(f"{i:>3d}" for i in range(len(IC.BRANCHES))))
    for name, count in rows:
        print(f"{name:<{width}}  " + " ".join(f"{count[k]:>3d}" if count[k] else "  ." for k in IC.BRANCHES))
    for i, k in enumerate(IC.BRANCHES):
        print(f"  {i:>2d} = {k}")


def _sum_branches(runs):
    total = dict.fromkeys(IC.BRANCHES, 0)
    for r, o in runs:
        for k, v in IC.branches(r, o).items():
            total[k] += int(v)
    return total


def test_the_twelve_iteration_cases_reach_none_of_the_control_flow_branches():
    """Why the control-flow cases exist: max_outer = 4, max_inner = 3 over the 28 problems of five shapes accepts 336 steps,
    clamps, grows or keeps the penalty and ends at status 1 -- and takes none of the branches of IC.BRANCHES."""
    rows = []
    for name in ["N12-kt5", "N17-ragged", "N3", "N2", "kt-extremes"]:
        batch = IC.shape(name)
        P, U0 = IC.problems(batch)
        runs = [(IR.solve(P[b], U0[b], IC.TWELVE, keep_trials=False), IC.TWELVE) for b in range(batch.B)]
        assert all(r.status == 1 and r.iters == 12 and all(i.a_star >= 0 for i in r.iterations) for r, _ in runs)
        rows.append((f"twelve iterations {name} ({batch.B} problems)", _sum_branches(runs)))
    _branch_table(rows)
    assert all(v == 0 for _, count in rows for v in count.values())


@pytest.mark.parametrize("case", IC.FLOW_CASES, ids=lambda c: c.name)
def test_control_flow_case_is_unambiguous_and_reaches_its_branches(case):
    """Every problem of the case, at the case's own schedule and at every prefix of it: float64 and longdouble agree in every
    decision and no margin of the longdouble run is below AMBIGUOUS -- none may be left out (the cases were picked one by
    one) -- float64 runs from controls moved by an ulp take the same decisions and stay within the tolerance the kernel is
    held to (the float64 spread that sets it is representative), and at its own schedule every problem takes every branch
    the case is there for."""
    worst, margin, perturbed = 0.0, np.inf, 0.0
    schedules = IC.flow_schedules(case)
    for o in schedules:
        for b in case.problems:
            r64, r80 = IC.flow_reference(case.batch, b, o)
            assert r64.decisions() == r80.decisions(), (case.name, b, o)
            assert r80.min_margin() >= IC.AMBIGUOUS, (case.name, b, o, r80.min_margin())
            assert not IC.ambiguous(r64, r80)
            worst, margin = max(worst, IR.control_error(r64.U, r80.U, o.h_max)), min(margin, r80.min_margin())
            same, ratio_u, ratio_j = IC.flow_perturbed(case.batch, b, o)
            assert same and ratio_u <= 1 and ratio_j <= 1, (case.name, b, o, same, ratio_u, ratio_j)
            perturbed = max(perturbed, ratio_u, ratio_j)
    for b in case.problems:
        r64, r80 = IC.flow_reference(case.batch, b, case.options)
        count = IC.branches(r64, case.options)
        print(f"{case.name} b={b}: outer {r64.outer} iters {r64.iters} status {r64.status} rho {r64.rho:g} mu {r64.mu:.3g} rescued "
              f"{int(r64.rescued)}; " + ", ".join(f"{k} {v}" for k, v in count.items() if v))
        assert all(count[k] > 0 for k in case.reaches), (case.name, b, count)
        same = {k: v for k, v in IC.branches(r80, case.options).items() if k != "non-finite trial"}  # (longdouble's range is wider)
        assert same == {k: v for k, v in count.items() if k != "non-finite trial"}
    print(f"{case.name}: {len(schedules)} schedules x {len(case.problems)} problems, largest float64 spread e(U) = {worst:.2e} "
          f"(tolerance {max(IC.TOL_MARGIN * worst, IC.TOL_FLOOR):.1e}), smallest margin {margin:.2e}; float64 runs moved by an ulp use "
          f"at most {perturbed:.3f} of the tolerance")


def test_every_control_flow_branch_is_reached_by_some_case():
    rows = []
    for case in IC.FLOW_CASES:
        rows.append((case.name, _sum_branches([(IC.flow_reference(case.batch, b, case.options)[0], case.options) for b in case.problems])))
    _branch_table(rows)
    reached = {k for _, count in rows for k in IC.BRANCHES if count[k]}
    assert reached == set(IC.BRANCHES) - set(IC.NOT_FOUND)
    named = {k for case in IC.FLOW_CASES for k in case.reaches}
    assert named == reached


# A failed pivot and a stalled inner loop were looked for in 1 344 float64 runs: the 28 problems of N12-kt5, N17-ragged,
# kt-extremes, N3 and N2 under rho0 = rho_max in {1e6, 1e8, 1e12} x h_prox in {0, 1e4} x exact_h_gradient x theta in +-pi/2 /
# +-0.3 x h in [0.001, 0.02] / [0.006, 0.014], max_outer = 2, max_inner = 30; every hit was then run in both precisions.
#   stalled   23 runs reach mu_max = 1e6 (the largest mu seen), one of them unambiguous: the "stalled, status 2 N12" case.
#   pivot     none at 1e6 or 1e8; at 1e12, 181 runs have one (N12-kt5 40, N17-ragged 99, kt-extremes 41, N3 1) and in all 181
#             the two precisions take different decisions.  Cut to the shortest schedule that contains the first failure and
#             two more iterations (the 152 runs of the three larger shapes whose first failure lies in the first multiplier
#             update), all 152 still differ.  That is the nature of the branch: Quu = Huu + B'PB + mu I is positive definite
#             in exact arithmetic (a Gauss-Newton Hessian), a pivot fails through rounding alone, and what rounding decides
#             the two precisions decide differently.  The path stays held by the invariants of tests/test_gpu_solve.py only
#             (DESIGN.md 4.6).
FLOW_SEARCH = dict(runs=1344, stalled=23, stalled_unambiguous=1, failed_pivot=181, failed_pivot_unambiguous=0,
                   failed_pivot_prefixes=152, failed_pivot_prefixes_unambiguous=0, largest_mu=1e6)


def test_failed_pivot_is_recorded_as_not_found():
    assert IC.NOT_FOUND == ["failed pivot"] and FLOW_SEARCH["failed_pivot_unambiguous"] == FLOW_SEARCH["failed_pivot_prefixes_unambiguous"] == 0
    print(f"the search for a failed pivot and a stalled inner loop: {FLOW_SEARCH}")
    # the search's one reproducible sample: the pivot fails in float64 in the first inner loop and the precisions disagree
    batch = IC.shape("N17-ragged")
    P, U0 = IC.problems(batch)
    o = IR.Options(rho0=1e12, rho_max=1e12, h_min=0.006, h_max=0.014, max_outer=1, max_inner=4)
    r64, r80 = IC.reference_pair(P[4], U0[4], o, keep_trials=False)
    assert IC.branches(r64, o)["failed pivot"] > 0 and r64.decisions() != r80.decisions()


def _rescue_cases():
    return [c for c in IC.FLOW_CASES if c.options.rescue_outer > 0]


@pytest.mark.parametrize("case", _rescue_cases(), ids=lambda c: c.name)
def test_rescue_phase_of_the_restatement(case):
    """The rescue phase against what the header says of it: the updates before it are those of the run without it; where it
    starts the penalty is min(rho, 1e6) and, the previous violation forgotten, the first update does not grow it; an inner
    loop of it may run to 60 iterations and no further; and a run that converges before max_outer never enters it."""
    o = case.options
    for b in case.problems:
        for T, (with_, without) in zip("fl", zip(IC.flow_reference(case.batch, b, o),
                                                  IC.flow_reference(case.batch, b, dataclasses.replace(o, rescue_outer=0)))):
            assert with_.rescued and not without.rescued
            n = len(without.iterations)
            assert [dataclasses.astuple(i)[:4] + (i.a_star,) for i in with_.iterations[:n]] == [dataclasses.astuple(i)[:4] + (i.a_star,) for i in without.iterations]
            assert with_.decisions()[0][:n] == without.decisions()[0] and with_.outer_decisions[:o.max_outer] == without.outer_decisions
            assert not any(i.rescue for i in with_.iterations[:n]) and all(i.rescue for i in with_.iterations[n:])
            before, after = with_.rho_at_rescue
            assert before == without.rho and after == min(before, 1e6) and with_.iterations[n].rho == after
            first = with_.outer_decisions[o.max_outer]
            assert first[2] and not first[1] and (first[0] or first[5] == after)  # in the rescue; no growth; rho as it was cut
            per_outer = np.bincount([i.outer for i in with_.iterations], minlength=with_.outer)
            assert per_outer[:o.max_outer].max(initial=0) <= o.max_inner and per_outer[o.max_outer:].max() <= IR.RESCUE_INNER
            assert with_.outer <= o.max_outer + o.rescue_outer


def test_a_run_that_converges_in_time_is_not_rescued():
    case = IC.flow_case("converges N12 seed 16")
    b = case.problems[0]
    P, U0 = IC.problems(IC.flow_batch(case.batch))
    plain = IC.flow_reference(case.batch, b, case.options)[0]
    r = IR.solve(P[b], U0[b], dataclasses.replace(case.options, rescue_outer=20), keep_trials=False)
    assert plain.status == 0 and not r.rescued and r.decisions() == plain.decisions() and np.array_equal(r.U, plain.U)
