"""tests/ilqr_ref.py, the numpy yardstick of qln_solve's iterates, held to evidence of its own (no GPU): the slope of its
line-search cost, a dense KKT solve of the sweep's linear-quadratic problem, the teeth of the clock-weight case, and the
agreement of its float64 and longdouble runs in every discrete decision."""
import dataclasses

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
