"""Cost tables and weights without coincidences, shared by tests/test_cost_cases_host.py (on the CPU) and
tests/test_gpu_cost.py (on the GPU).  Not a test module.

qln_batch_desc.cost is [cost_batch][N][41], one record Q[15] R[5] q[15] r[5] c per knot.  The table make_batch builds --
lqr_objective(Q_DIAG, R_DIAG, Q_DIAG, Xref, Uref), the notebook's -- cannot tell a kernel that indexes the record rightly
from many that do not: fourteen of the fifteen Q are the same 10.0, R[0] == R[2] and R[1] == R[3], the clock and step-length
slots Q[14], q[14], R[4], r[4] are zero, every stage record of a phase is the same 41 doubles, Qf == Q, the terminal
record's control slots hold R * 0, and c is what LQRCost derives from the other forty.  generic_cost draws every record of
every knot (and of every problem) independently; DISTINCT_WEIGHTS does the same for the diagonal weights of the tracking
designs and of qln_set_lqr_cost."""
import numpy as np

from quadruped_landing_amd import problem_gen as PG
from quadruped_landing_amd.ref_traj import reference_trajectory

DT = 0.009
SENTINEL = 1e6  # the terminal record's ten control slots: +-SENTINEL (j + 1), never read by the reference


def terminal_sentinels():
    """the values of slots 15..19 (R) and 35..39 (r) of a terminal record: distinct, large, finite, of both signs.
    Finite on purpose: a kernel that multiplies such a slot by a zero mask is not wrong by the oracle."""
    return np.array([(-1.0) ** j * SENTINEL * (j + 1) for j in range(10)])


def generic_cost(batch, seed, per_problem, convex):
    """(N, 41), or (B, N, 41) with per_problem: every record drawn on its own.

    convex=True (for the solver: a positive definite stage cost around the reference trajectory):
        Q_k[i] = 10 U(0.3, 3) for all fifteen entries, the clock included; R_k[0..3] = R_DIAG U(0.3, 3); R_k[4] = U(300, 3000);
        q = -Q (Xref_k + 0.05 N(0, 1)); r = -R (Uref_k + N(0, 1)) with a step-length reference ~ U(0.005, 0.015); c ~ N(0, 1).
    convex=False (for the evaluators): all 41 entries ~ N(0, 1), so both signs appear.
    The terminal record is a draw of its own like every other; its ten control slots hold terminal_sentinels()."""
    N, B = batch.N, batch.B
    rng = np.random.default_rng(seed)
    lead = (B,) if per_problem else ()
    if convex:
        Xref, Uref = reference_trajectory(batch.model, N, batch.k_trans, batch.xf, batch.init_mode, DT)
        if not per_problem:
            Xref, Uref = Xref[0], Uref[0]
        Uref = np.concatenate([Uref, Uref[..., -1:, :]], axis=-2)  # a row for the terminal record, overwritten below
        tab = np.empty(lead + (N, 41))
        Q = 10.0 * rng.uniform(0.3, 3.0, size=lead + (N, 15))
        R = np.empty(lead + (N, 5))
        R[..., :4] = PG.R_DIAG[:4] * rng.uniform(0.3, 3.0, size=lead + (N, 4))
        R[..., 4] = rng.uniform(300.0, 3000.0, size=lead + (N,))
        uref = Uref + rng.normal(size=lead + (N, 5))
        uref[..., 4] = rng.uniform(0.005, 0.015, size=lead + (N,))
        tab[..., 0:15] = Q
        tab[..., 15:20] = R
        tab[..., 20:35] = -Q * (Xref + 0.05 * rng.normal(size=lead + (N, 15)))
        tab[..., 35:40] = -R * uref
        tab[..., 40] = rng.normal(size=lead + (N,))
    else:
        tab = rng.normal(size=lead + (N, 41))
    s = terminal_sentinels()
    tab[..., N - 1, 15:20] = s[:5]
    tab[..., N - 1, 35:40] = s[5:]
    return np.ascontiguousarray(tab)


def with_generic_cost(batch, seed, per_problem, convex):
    """the batch itself, its table replaced"""
    batch.obj = generic_cost(batch, seed, per_problem, convex)
    return batch


SOLVER_SEED = 5  # the draw tests/test_cost_cases_host.py holds the solver's yardstick to


def twenty_four():
    """max_outer = 6, max_inner = 4: late iterations, whose descent test J_try < J_cur a bias of the trial merit alone flips"""
    from tests import ilqr_ref as IR

    return IR.Options(max_outer=6, max_inner=4)


def multi_iteration_cases():
    """(ids, [(shape, per_problem, options)]): the many-iteration runs the GPU is held to.  A case qualifies if the yardstick
    leaves out none of its problems as ambiguous and if its tolerance -- 100 times ONE float64 run's distance from the
    longdouble run -- is not founded on a lucky sample: float64 runs whose guess is moved by one ulp stay within a quarter
    of it (tests/test_cost_cases_host.py holds both; the runs here use at most 0.11).  Twenty-four iterations of N12-kt5
    with per-problem tables do not qualify: problem 0's float64 run lands 6.6e-14 (controls) and 2.6e-15 (cost) from the
    longdouble run, its one-ulp neighbours 1.5e-12 and up to 2.5e-12, three to ten times the tolerance on the cost.  (The kernel at that
    problem: controls 3.5e-12, 53 times the lucky spread and under the bound; cost 1.9e-12 against a tolerance of 2.6e-13 --
    among the float64 neighbours, and what first showed that this tolerance rests on luck.)"""
    import dataclasses

    from tests import ilqr_cases as IC

    cases = {"N12-kt5-shared-x12": ("N12-kt5", False, IC.TWELVE), "N17-ragged-x12": ("N17-ragged", True, IC.TWELVE),
             "N17-ragged-x12-exact-h": ("N17-ragged", True, dataclasses.replace(IC.TWELVE, exact_h_gradient=1)),
             "N17-ragged-x24": ("N17-ragged", True, twenty_four())}
    return list(cases), list(cases.values())


def solver_case(name, per_problem, model=None):
    """ilqr_cases.shape(name) under a convex generic table"""
    from tests import ilqr_cases as IC

    return with_generic_cost(IC.shape(name, model), SOLVER_SEED, per_problem, True)


def uniform_batch(B, N, k_trans=None, init_mode=1, seed=0, **kw):
    """uniform k_trans and init_mode: in a per-problem run only the table tells the problems apart"""
    kt = (2 if N <= 3 else min(14, N - 1)) if k_trans is None else k_trans
    return PG.make_batch(B, N, kt, init_mode, seed=seed, **kw)


# Diagonal weights, pairwise distinct within a set, none zero; each within a factor 3 of the weight it replaces, so that the
# conditioning of the comparisons that use them is that of the weights they replace:
#   "tracking":  tracking_cases.QW = [10] * 14 + [0.7], R = [1e-3, 1e-2, 1e-3, 1e-2], QFW = [30] * 14 + [2.0]
#   "lqr_cost":  Q = Q_DIAG with Q[14] = 0.7, R = R_DIAG, Qf = 3 Q_DIAG of test_lqr_cost_built_on_device_is_bitwise_the_host_builder;
#                R[4] and Qf[14] are zero there and have no factor to keep
_SPREAD = np.array([0.41, 0.55, 0.68, 0.83, 0.97, 1.13, 1.31, 1.52, 1.77, 2.05, 2.38, 2.71, 0.47, 0.74])
DISTINCT_WEIGHTS = {
    "tracking": dict(Q=np.concatenate([10.0 * _SPREAD, [0.9]]), R=np.array([6e-4, 1.7e-2, 2.1e-3, 4.5e-3]),
                     Qf=np.concatenate([30.0 * _SPREAD[::-1] * 1.07, [2.6]])),
    "lqr_cost": dict(Q=np.concatenate([10.0 * _SPREAD[::-1], [0.5]]), R=np.array([1.9e-3, 6.1e-3, 4.3e-4, 2.3e-2, 700.0]),
                     Qf=np.concatenate([30.0 * _SPREAD * 0.93, [1.9]])),
}
REPLACED = {
    "tracking": dict(Q=np.array([10.0] * 14 + [0.7]), R=np.array([1e-3, 1e-2, 1e-3, 1e-2]), Qf=np.array([30.0] * 14 + [2.0])),
    "lqr_cost": dict(Q=np.array([10.0] * 14 + [0.7]), R=PG.R_DIAG, Qf=3.0 * PG.Q_DIAG),
}
