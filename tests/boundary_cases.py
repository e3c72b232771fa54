"""Boundary states without coincidences, shared by tests/test_boundary_cases_host.py (on the CPU) and
tests/test_gpu_boundary.py (on the GPU).  Not a test module.

qln_batch_desc.x0 / .xf become the [B][30] table BatchParams::bnd, x0 (15) then xf (15) of each problem; every kernel that
reads it indexes it by problem, by half and by slot.  The states make_batch and notebook_problem() build cannot tell a
kernel that does so rightly from many that do not: xf is the same fifteen doubles for every problem, twelve of them 0.0
(only slots 0, 1 and 5 are not), xf[5] == 2 xf[0] bit for bit, every velocity and the clock are zero; x0 of init_mode 1
differs between problems in slots 2, 6, 8 and 9 only; and in eight of the fifteen slots x0[j] == xf[j] in every problem
(six under init_mode 2).  generic_boundary draws every slot of both states of every problem on its own; MUTATIONS are the
wrong readings such coincidences hide, as inputs for a yardstick."""
import numpy as np

from quadruped_landing_amd import nlp as NL
from quadruped_landing_amd import problem_gen as PG
from quadruped_landing_amd.quadratic_cost import lqr_objective
from quadruped_landing_amd.ref_traj import reference_trajectory

DT = 0.009
SCALE = 0.05  # of the size of make_batch's own noise on Z: the solver's yardstick stays as well conditioned as it is there
SEED = 6      # the draw tests/test_boundary_cases_host.py holds to "no coincidence" and "every mutation shows" at every shape

# the coincidences of the default states, by slot (tests/test_boundary_cases_host.py asserts each on the generator)
XF_NONZERO = [0, 1, 5]
X0_SHARED_MODE1 = [0, 1, 3, 4, 5, 7, 10, 11, 12, 13, 14]  # identical across the problems of an init_mode 1 batch
X0_ZERO_MODE1 = [3, 4, 7, 10, 11, 12, 14]
X0_IS_XF_MODE1 = [3, 4, 5, 7, 10, 11, 12, 14]
X0_IS_XF_MODE2 = [6, 7, 10, 12, 13, 14]


def generic_boundary(batch, seed=SEED):
    """the batch itself with x0[b] = make_batch's x0[b] + SCALE N(0, 1) and xf[b] = terminal_state(model) + SCALE N(0, 1), all
    fifteen slots of every problem drawn on their own (velocities and clock of xf included).  batch.Z stays: it is a guess."""
    rng = np.random.default_rng(seed)
    B = batch.B
    batch.x0 = np.ascontiguousarray(batch.x0 + SCALE * rng.normal(size=(B, 15)))
    batch.xf = np.ascontiguousarray(PG.terminal_state(batch.model) + SCALE * rng.normal(size=(B, 15)))
    return batch


def rebuilt_cost(batch, Q=PG.Q_DIAG, R=PG.R_DIAG, Qf=PG.Q_DIAG):
    """(B, N, 41): the notebook's cost around the reference trajectory to each problem's OWN xf (what qln_set_lqr_cost builds
    per problem)"""
    Xref, Uref = reference_trajectory(batch.model, batch.N, batch.k_trans, batch.xf, batch.init_mode, DT)
    return lqr_objective(Q, R, Qf, Xref, Uref)


def with_cost(batch, which):
    """'kept': batch.obj as generated (around the default xf); 'rebuilt': rebuilt_cost(batch)"""
    if which == "rebuilt":
        batch.obj = rebuilt_cost(batch)
    elif which != "kept":
        raise KeyError(which)
    return batch


def evaluator_batch(B, N, ragged, seed, generic=True, **kw):
    """make_batch's batch (uniform k_trans = min(14, N - 1), init_mode 1, or ragged) under generic states, or -- generic=False --
    its twin under the default ones, same Z"""
    kt = 2 if N <= 3 else min(14, N - 1)
    batch = PG.make_batch(B, N, seed=seed, ragged=True, **kw) if ragged else PG.make_batch(B, N, kt, 1, seed=seed, **kw)
    return generic_boundary(batch, SEED) if generic else batch


# ---- the shapes both modules use ------------------------------------------------------------------------------------------
# (B, N, ragged, handle options): the launch plans these reach are enumerated by tests/test_boundary_cases_host.py
EVALUATOR_SHAPES = [(4, 2, False, {}), (5, 3, False, {}), (9, 41, False, {}), (5, 64, False, {}), (3, 65, False, {}),
                    (6, 66, True, {}), (7, 130, True, {}), (5000, 40, False, {}), (9, 40, False, dict(z_stride=803, align=7))]
EVALUATOR_IDS = [f"{B}x{N}" + ("-ragged" if r else "") + ("-padded" if kw else "") for B, N, r, kw in EVALUATOR_SHAPES]
STREAMED_SHAPE = (5736, 40, False, {})  # dense blocks only: 93 600 B of Jacobian per problem, the first size past 512 MiB
HOST_FORM_SHAPES = [(5, 41), (5, 12)]   # eval_c_host: one workgroup per 16-knot chunk (N > 17, B <= 256), and per problem


def solver_cases():
    """id -> (shape name, options, model, cost): the solver runs; tests/test_boundary_cases_host.py qualifies each"""
    import dataclasses

    from tests import ilqr_cases as IC

    cases = {}
    for name in ("N12-kt5", "N17-ragged", "N65", "N2", "kt-extremes"):
        for exact_h in (0, 1):
            cases[f"one-{name}-exact_h{exact_h}"] = (name, dataclasses.replace(IC.ONE, exact_h_gradient=exact_h), None, "kept")
    for name in ("N12-kt5", "N17-ragged"):
        cases[f"twelve-{name}"] = (name, IC.TWELVE, None, "kept")
    cases["one-N12-kt5-second-model"] = ("N12-kt5", IC.ONE, IC.SECOND_MODEL, "kept")
    cases["one-N12-kt5-second-model-generic-table"] = ("N12-kt5", IC.ONE, IC.SECOND_MODEL, "generic")  # all three at once
    cases["one-N17-ragged-rebuilt-table"] = ("N17-ragged", IC.ONE, None, "rebuilt")
    return cases


def solver_batch(name, model, cost):
    """the batch of a solver case: cost 'kept', 'rebuilt' (around each problem's own xf) or 'generic' (cost_cases' convex
    per-problem table: model, table and boundary states without coincidences at once)"""
    from tests import cost_cases as CC
    from tests import ilqr_cases as IC

    batch = generic_boundary(IC.shape(name, model), SEED)
    return CC.with_generic_cost(batch, CC.SOLVER_SEED, True, True) if cost == "generic" else with_cost(batch, cost)


# ---- wrong readings of the table, as inputs -------------------------------------------------------------------------------
SWAP_SLOT = 7     # x0[7] == xf[7] == 0 under both init_modes
ZERO_PAIR = (8, 9)  # two of xf's twelve zeros (c reads xf[0:14])


def _next_problem(x0, xf):
    return x0, np.roll(xf, -1, axis=0)


def _problem_zero(x0, xf):
    return x0, np.tile(xf[:1], (len(xf), 1))


def _swap_halves(x0, xf):
    a, b = x0.copy(), xf.copy()
    a[:, SWAP_SLOT], b[:, SWAP_SLOT] = xf[:, SWAP_SLOT], x0[:, SWAP_SLOT]
    return a, b


def _swap_zeros(x0, xf):
    b = xf.copy()
    b[:, list(ZERO_PAIR)] = xf[:, list(ZERO_PAIR)[::-1]]
    return x0, b


def _drop_velocities(x0, xf):
    b = xf.copy()
    b[:, 7:15] = 0.0
    return x0, b


def _twice_slot_zero(x0, xf):
    b = xf.copy()
    b[:, 5] = 2 * xf[:, 0]
    return x0, b


# name -> ((x0, xf) -> (x0, xf) as a kernel with that fault would see them, problems the fault cannot show in)
MUTATIONS = {
    "xf of problem b + 1 mod B": (_next_problem, ()),
    "xf of problem 0": (_problem_zero, (0,)),
    f"x0[{SWAP_SLOT}] <-> xf[{SWAP_SLOT}]": (_swap_halves, ()),
    f"xf[{ZERO_PAIR[0]}] <-> xf[{ZERO_PAIR[1]}]": (_swap_zeros, ()),
    "xf[7:15] zeroed": (_drop_velocities, ()),
    "xf[5] := 2 xf[0]": (_twice_slot_zero, ()),
}


def c_layout(batch):
    """(c_off (B,), c_total) of an unpadded host layout"""
    m = np.array([NL.num_duals(batch.N, int(k)) for k in batch.k_trans], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(m)])
    return off[:-1].copy(), int(off[-1])


def oracle_c(batch, x0=None, xf=None, nthreads=4):
    """c of every problem from the C oracle, as a list of per-problem rows; x0 / xf in place of the batch's"""
    from oracle import oracle as O
    from tests.helpers import oracle_model

    c_off, c_total = c_layout(batch)
    n = 20 * batch.N - 5
    out = O.batch_eval(batch.N, oracle_model(batch.model), batch.k_trans, batch.init_mode, batch.x0 if x0 is None else x0,
                       batch.xf if xf is None else xf, batch.obj, np.ascontiguousarray(batch.Z).reshape(-1), n, c_off,
                       np.zeros(batch.B, dtype=np.int64), c_total, 0, True, False, False, False, nthreads)
    ends = np.append(c_off[1:], c_total)
    return [out["c"][a:e] for a, e in zip(c_off, ends)]


def mutation_effect(batch, name, c_true=None):
    """per-problem max |c(mutated inputs) - c(true inputs)| from the C oracle, the problems the fault cannot show in left out"""
    fn, blind = MUTATIONS[name]
    c_true = oracle_c(batch) if c_true is None else c_true
    x0, xf = fn(batch.x0, batch.xf)
    c_mut = oracle_c(batch, x0, xf)
    d = np.array([np.max(np.abs(a - b)) for a, b in zip(c_mut, c_true)])
    return np.delete(d, list(blind))
