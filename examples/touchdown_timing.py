"""When does the foot really land?  Solve the notebook's problem (N = 61, k_trans = 21) with qln_solve, compute TVLQR gains,
and drop 1 024 robots whose free foot starts up to 2 cm higher or lower than planned and whose feet are up to 10 % lighter
or heavier than the design model's.  The knot-scheduled roll-out puts every one of them on the ground at the planned knot,
wherever the foot is; the guarded roll-out (qln_tracking_rollout_guarded) lets the foot land when it reaches the ground
and reports when and how hard.  Prints the distribution of actual minus planned touchdown time, the impact speed, the
smallest force under a standing foot, and the terminal error of both roll-outs.
   python examples/touchdown_timing.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from quadruped_landing_amd import HybridNLP, problem_gen as PG  # noqa: E402

S = 1024
Q = np.array([10.0] * 14 + [0.0])
R = np.array([1e-3, 1e-2, 1e-3, 1e-2])
HEIGHT, FOOT_MASS = 0.02, 0.10  # +- 2 cm of free-foot start height, +- 10 % of foot mass


def quantiles(v):
    return "min {:+.4e}  5 % {:+.4e}  median {:+.4e}  95 % {:+.4e}  max {:+.4e}".format(
        v.min(), *np.percentile(v, [5, 50, 95]), v.max())


def main():
    nb = PG.notebook_problem()
    N, n, kt = nb.N, 20 * nb.N - 5, int(nb.k_trans[0])
    one = HybridNLP(nb.model, nb.obj, nb.init_mode, nb.k_trans, N, nb.x0, nb.xf)
    Zs = one.upload_Z(nb.Z)
    _, info = one.solve(Zs)
    zref = Zs.cpu().numpy().reshape(-1)[:n]
    print(f"solve: status {int(info[0, 5])}, violation {float(info[0, 3]):.2e}, objective {float(info[0, 2]):.4f}")
    planned = zref[20 * (kt - 1) + 14]  # the clock of the first knot after the jump map
    print(f"planned touchdown: end of knot {kt - 2} (0-based), clock {planned:.4f} s")

    rng = np.random.default_rng(0)
    x0 = np.tile(nb.x0.reshape(1, 15), (S, 1))
    x0[:, 6] += rng.uniform(-HEIGHT, HEIGHT, size=S)  # init_mode 1: foot 2 is the free one
    nlp = HybridNLP(nb.model, nb.obj, np.full(S, nb.init_mode[0]), np.full(S, kt), N, x0, np.tile(nb.xf.reshape(1, 15), (S, 1)))
    model = nlp.plant_models()
    model[:, 2] *= torch.from_numpy(1.0 + rng.uniform(-FOOT_MASS, FOOT_MASS, size=S)).cuda()
    Zref = nlp.upload_Z(np.tile(zref, (S, 1)))
    K, _ = nlp.tracking_lqr(Zref, Q, R, Q, with_cost_to_go=False)
    x0d = torch.from_numpy(x0).cuda()

    Zg, events = nlp.tracking_rollout_guarded(Zref, K, x0d, model)
    Zk = nlp.tracking_rollout_model(Zref, K, x0d, model)
    torch.cuda.synchronize()
    ev = events.cpu().numpy()
    landed = ev[:, 0] >= 0
    print(f"{S} drops, free foot +-{100 * HEIGHT:.0f} cm, foot mass +-{100 * FOOT_MASS:.0f} %: {int(landed.sum())} land, "
          f"{int((~landed).sum())} never reach the ground within the horizon")
    if landed.any():
        e = ev[landed]
        knots = e[:, 0].astype(int)
        print(f"touchdown knot: {knots.min()} .. {knots.max()} (planned {kt - 2}); "
              f"{int((knots != kt - 2).sum())} of {len(knots)} land in another knot than planned")
        print(f"actual - planned touchdown clock [s]: {quantiles(e[:, 2] - planned)}")
        print(f"impact speed |v_y| [m/s]:             {quantiles(np.abs(e[:, 5]))}")
        print(f"impact speed |v_x| [m/s]:             {quantiles(np.abs(e[:, 4]))}")
    print(f"smallest standing-foot F_y [N]:       {quantiles(ev[:, 6])}")
    print(f"  the ground pulls (F_y < 0) in {int((ev[:, 6] < 0).sum())} of {S} drops")
    xref = zref[20 * (N - 1): 20 * (N - 1) + 14]
    print(f"{'':28s} {'median |x_N - x_ref,N|':>24s} {'max':>12s}")
    for name, Z in (("guarded touchdown", Zg), ("touchdown at the planned knot", Zk)):
        xN = Z.view(S, -1)[:, 20 * (N - 1): 20 * (N - 1) + 14].cpu().numpy()
        err = np.linalg.norm(xN - xref, axis=1)
        print(f"{name:28s} {np.median(err):24.3e} {np.max(err):12.3e}")
    # what the knot schedule hides: where the free foot is when the planned knot puts it on the ground
    yk = Zk.view(S, -1)[:, 20 * (kt - 2) + 6].cpu().numpy()
    print(f"knot-scheduled roll-out: free foot's height at the start of the planned touchdown knot [m]: {quantiles(yk)}")


if __name__ == "__main__":
    main()
