"""How well does one derivative predict where and when the foot lands?  Solve the notebook's problem (N = 61, k_trans = 21)
with qln_solve, compute TVLQR gains, and take ONE nominal guarded roll-out (qln_tracking_rollout_guarded) and ONE forward
sweep through its touchdown (qln_tracking_rollout_guarded_jvp) per drop: 1 024 drops whose free foot starts up to 2 cm
higher or lower than planned and whose feet are up to 10 % lighter or heavier than the design model's, as in
examples/touchdown_timing.py.  Each drop's perturbation is its own direction (x0_dot, model_dot) at the nominal point, so
nominal + tangent is the first-order prediction of its touchdown clock and of x_N; the actual guarded roll-outs of the
perturbed drops say how good it is.  For contrast, the same prediction from the knot-scheduled sweep
(qln_tracking_rollout_model_jvp at the knot-scheduled roll-out), which cannot move the touchdown at all.
   python examples/touchdown_sensitivity.py"""
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
    return "median {:.3e}  95 % {:.3e}  max {:.3e}".format(*np.percentile(v, [50, 95]), v.max())


def main():
    nb = PG.notebook_problem()
    N, n, kt = nb.N, 20 * nb.N - 5, int(nb.k_trans[0])
    one = HybridNLP(nb.model, nb.obj, nb.init_mode, nb.k_trans, N, nb.x0, nb.xf)
    Zs = one.upload_Z(nb.Z)
    _, info = one.solve(Zs)
    zref = Zs.cpu().numpy().reshape(-1)[:n]
    print(f"solve: status {int(info[0, 5])}, violation {float(info[0, 3]):.2e}, objective {float(info[0, 2]):.4f}")

    rng = np.random.default_rng(0)
    dy = rng.uniform(-HEIGHT, HEIGHT, size=S)
    dmf = rng.uniform(-FOOT_MASS, FOOT_MASS, size=S)
    x0 = np.tile(nb.x0.reshape(1, 15), (S, 1))  # the nominal drop, S times: every problem gets its own direction
    nlp = HybridNLP(nb.model, nb.obj, np.full(S, nb.init_mode[0]), np.full(S, kt), N, x0, np.tile(nb.xf.reshape(1, 15), (S, 1)))
    model = nlp.plant_models()
    Zref = nlp.upload_Z(np.tile(zref, (S, 1)))
    K, _ = nlp.tracking_lqr(Zref, Q, R, Q, with_cost_to_go=False)
    x0d = torch.from_numpy(x0).cuda()
    x0_dot = torch.zeros_like(x0d)
    x0_dot[:, 6] = torch.from_numpy(dy).cuda()  # init_mode 1: foot 2 is the free one
    model_dot = torch.zeros_like(model)
    model_dot[:, 2] = model[:, 2] * torch.from_numpy(dmf).cuda()

    # one nominal guarded roll-out and one sweep through its touchdown
    Zn, ev_n = nlp.tracking_rollout_guarded(Zref, K, x0d, model)
    Zd, ev_d = nlp.tracking_rollout_guarded_jvp(Zref, Zn, ev_n, K, model, x0_dot=x0_dot, model_dot=model_dot)
    # the same from the knot-scheduled roll-out and its sweep
    Zk = nlp.tracking_rollout_model(Zref, K, x0d, model)
    Zkd = nlp.tracking_rollout_model_jvp(Zref, Zk, K, model, x0_dot=x0_dot, model_dot=model_dot)
    # what really happens
    Za, ev_a = nlp.tracking_rollout_guarded(Zref, K, x0d + x0_dot, model + model_dot)
    torch.cuda.synchronize()

    xN = lambda Z: Z.view(S, -1)[:, 20 * (N - 1): 20 * (N - 1) + 14].cpu().numpy()  # noqa: E731
    en, ed, ea = ev_n.cpu().numpy(), ev_d.cpu().numpy(), ev_a.cpu().numpy()
    same = ea[:, 0] == en[:, 0]
    print(f"nominal drop: touchdown in knot {int(en[0, 0])} at tau = {en[0, 1]:.4e} s, clock {en[0, 2]:.4f} s "
          f"(planned: end of knot {kt - 2}, clock {zref[20 * (kt - 1) + 14]:.4f} s)")
    print(f"{S} drops, free foot +-{100 * HEIGHT:.0f} cm, foot mass +-{100 * FOOT_MASS:.0f} %: {int(same.sum())} land in the "
          f"nominal knot, {int((~same).sum())} in another one (no derivative reaches those: the knot is fixed)")
    move = np.abs(ea[:, 2] - en[:, 2])
    print(f"actual shift of the touchdown clock [s]:              {quantiles(move)}")
    for name, keep in (("drops landing in the nominal knot", same), ("all drops", np.ones(S, dtype=bool))):
        print(f"-- {name} ({int(keep.sum())})")
        err_t = np.abs(en[keep, 2] + ed[keep, 2] - ea[keep, 2])
        print(f"touchdown clock, nominal + event_dot, error [s]:      {quantiles(err_t)}")
        print(f"touchdown clock, knot schedule (no shift), error [s]: {quantiles(move[keep])}")
        act = xN(Za)[keep]
        for label, pred in (("guarded roll-out + guarded sweep", xN(Zn) + xN(Zd)), ("knot-scheduled roll-out + its sweep", xN(Zk) + xN(Zkd)),
                            ("guarded roll-out alone (zeroth order)", xN(Zn))):
            print(f"|x_N predicted - x_N actual|, {label:38s} {quantiles(np.linalg.norm(pred[keep] - act, axis=1))}")


if __name__ == "__main__":
    main()
