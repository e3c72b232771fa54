"""What the CPU and the GPU tests of the guarded roll-out (qln_tracking_rollout_guarded) share: the shapes, and one builder
of a case's host inputs, so that the seeds checked on the CPU are the ones the GPU runs.  Not a test module."""
import copy

import numpy as np

from tests import rollout_ref as RR
from tests import tracking_cases as TC

# (N, init_mode, B): one knot, two, several and the full sizes, both feet.  One lane per problem and 64 lanes per block: these
# are one block each, and ragged_case below runs two.
SHAPES = [(2, 1, 24), (2, 2, 24), (3, 1, 24), (5, 2, 32), (8, 1, 48), (40, 1, 9), (40, 2, 9), (61, 1, 17)]
MARGIN = 1e-9      # a problem closer than this to one of the guard's boundaries is left out of a comparison
LEFT_OUT = 0.01    # ... and at most this share of a test's problems may be


def free_foot(init_mode):
    """Indices of the free foot's (y, vy) in the state: mode 1 frees foot 2, mode 2 foot 1."""
    return (6, 13) if init_mode == 1 else (4, 11)


def seed_of(N, init_mode, with_gains, with_models):
    return 1000 * N + 100 * init_mode + 10 * int(with_gains) + int(with_models)


def case(N, init_mode, B, with_gains, with_models, seed=None):
    """Host inputs of one case: (batch, Zref (B, n_nlp), K (B, N-1, 4, 15) or None, x0 (B, 15), th (B, 4)).  The reference
    is problem_gen's; x0 lies near its first knot.  For N <= 8 the free foot starts at y ~ U(0, 0.02 (N-1)) with v = -1,
    which spreads the touchdowns over every knot; for N >= 40 the generator's own drop heights do.  The last problem's
    reference pulls its free foot up, so that it never lands.  th is the handle's model (TC.SECOND) for every problem, or
    models drawn around it."""
    seed = seed_of(N, init_mode, with_gains, with_models) if seed is None else seed
    batch = TC.batch(B, N, 14 if N >= 40 else 2, init_mode, seed=seed)
    rng = np.random.default_rng(seed + 7)
    Zref = np.ascontiguousarray(batch.Z, dtype=np.float64)
    x0 = Zref[:, :15] + 1e-2 * rng.normal(size=(B, 15))
    iy, iv = free_foot(init_mode)
    if N <= 8:
        x0[:, iy] = rng.uniform(0.0, 0.02 * (N - 1), size=B)
        x0[:, iv] = -1.0
    # one problem without a touchdown in every batch: its reference pulls the free foot up (F_y = -2 N on 0.13 kg against
    # g = -9.1 m/s^2 is 6 m/s^2 upwards) from rest at 0.3 m
    Zref[B - 1, 15 + (3 if init_mode == 1 else 1)::20] = -2.0
    x0[B - 1, iy], x0[B - 1, iv] = 0.3, 0.0
    K = 0.05 * rng.normal(size=(B, N - 1, 4, 15)) if with_gains else None
    th = RR.draw_models(B, seed + 2, TC.SECOND) if with_models else np.tile(TC.SECOND, (B, 1))
    return batch, Zref, K, x0, th


def with_k_trans(batch, k_trans):
    """A copy of the batch whose handle switches mode at k_trans (the guarded call does not read it)."""
    b = copy.copy(batch)
    b.k_trans = np.full(batch.B, k_trans, dtype=np.int32)
    return b


CONTINUITY = [(40, 14), (12, 2)]  # (N, the k_trans the reference is generated with)
CONTINUITY_B = 2001


def continuity_case(N, kt_build, B=CONTINUITY_B):
    """Open loop, one reference for every problem; the free foot's start height runs linearly over [0.02, 0.12] with
    v = -1.  Returns (batch, Zref (B, n_nlp), x0 (B, 15), th (B, 4))."""
    one = TC.batch(1, N, kt_build, 1, seed=N)
    batch = TC.batch(B, N, kt_build, 1, seed=N)
    Zref = np.ascontiguousarray(np.tile(one.Z[0].astype(np.float64), (B, 1)))
    x0 = Zref[:, :15].copy()
    x0[:, 6] = np.linspace(0.02, 0.12, B)
    x0[:, 13] = -1.0
    return batch, Zref, x0, np.tile(TC.SECOND, (B, 1))


def continuity_ratio(knots, xN):
    """(number of changes of the touchdown knot along the sweep, largest neighbour difference of x_N at a change over the
    largest elsewhere)."""
    d = np.linalg.norm(np.diff(xN, axis=0), axis=1)
    change = np.diff(knots) != 0
    return int(change.sum()), float(d[change].max() / d[~change].max())


def tau_zero_case(N=5, init_mode=1):
    """Open loop, three problems whose free foot starts at y = 0.0, -0.0 and -1e-3: touchdown at tau = 0 of knot 0."""
    batch = TC.batch(3, N, 2, init_mode, seed=11 + init_mode)
    Zref = np.ascontiguousarray(batch.Z, dtype=np.float64)
    x0 = Zref[:, :15].copy()
    iy, iv = free_foot(init_mode)
    x0[:, iy] = [0.0, -0.0, -1e-3]
    x0[:, iv] = -1.0
    return batch, Zref, x0, np.tile(TC.SECOND, (3, 1))


def ragged_case(B=70, N=12, seed=3, **kw):
    """More than one block of 64 lanes, per-problem init_mode, k_trans and step lengths, gains and models."""
    batch = TC.batch(B, N, 5, 1, seed=seed, ragged=True)
    rng = np.random.default_rng(seed + 7)
    Zref = np.ascontiguousarray(batch.Z, dtype=np.float64)
    x0 = Zref[:, :15] + 1e-2 * rng.normal(size=(B, 15))
    for b in range(B):
        iy, iv = free_foot(int(batch.init_mode[b]))
        x0[b, iy], x0[b, iv] = rng.uniform(0.0, 0.2), -1.0
    K = 0.05 * rng.normal(size=(B, N - 1, 4, 15))
    return batch, Zref, K, x0, RR.draw_models(B, seed + 2, TC.SECOND)
