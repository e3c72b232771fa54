"""Design the tracking controller ON the touchdown.  The experiment of examples/touchdown_timing.py -- the notebook's problem
(N = 61, k_trans = 21) solved with qln_solve, 1 024 drops whose free foot starts up to 2 cm higher or lower than planned and
whose feet are up to 10 % lighter or heavier -- rolled out with the guarded touchdown under two designs:
  (a) the plan as reference with time-indexed TVLQR gains (qln_tracking_lqr), which puts the jump at the planned knot;
  (b) the guarded roll-out of the plan, Zg, as reference with gains from qln_tracking_lqr_guarded along (Zg, events): the
      saltation-matrix TVLQR at the knot where the nominal drop really lands.
Prints the terminal error of both, the share of drops that keep the nominal touchdown knot (for those (b)'s gains are the
first-order optimal ones), and the touchdown clock's standard deviation as qln_tracking_covariance_guarded's event_var
predicts it from the drops' covariance, beside the sample's.
   python examples/track_touchdown.py"""
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


def main():
    nb = PG.notebook_problem()
    N, n, kt = nb.N, 20 * nb.N - 5, int(nb.k_trans[0])
    one = HybridNLP(nb.model, nb.obj, nb.init_mode, nb.k_trans, N, nb.x0, nb.xf)
    Zs = one.upload_Z(nb.Z)
    _, info = one.solve(Zs)
    zref = Zs.cpu().numpy().reshape(-1)[:n]
    print(f"solve: status {int(info[0, 5])}, violation {float(info[0, 3]):.2e}, objective {float(info[0, 2]):.4f}")

    rng = np.random.default_rng(0)
    x0 = np.tile(nb.x0.reshape(1, 15), (S, 1))
    x0[:, 6] += rng.uniform(-HEIGHT, HEIGHT, size=S)  # init_mode 1: foot 2 is the free one
    nlp = HybridNLP(nb.model, nb.obj, np.full(S, nb.init_mode[0]), np.full(S, kt), N, x0, np.tile(nb.xf.reshape(1, 15), (S, 1)))
    nominal = nlp.plant_models()
    model = nominal.clone()
    model[:, 2] *= torch.from_numpy(1.0 + rng.uniform(-FOOT_MASS, FOOT_MASS, size=S)).cuda()
    Zplan = nlp.upload_Z(np.tile(zref, (S, 1)))
    x0d = torch.from_numpy(x0).cuda()
    x0n = torch.from_numpy(np.tile(nb.x0.reshape(1, 15), (S, 1))).cuda()

    # (a) the plan and its time-indexed gains
    Ka, _ = nlp.tracking_lqr(Zplan, Q, R, Q, with_cost_to_go=False)
    Za, eva = nlp.tracking_rollout_guarded(Zplan, Ka, x0d, model)
    # (b) the nominal drop rolled out guarded (open loop, the design model), gains along it through its touchdown
    Zg, evg = nlp.tracking_rollout_guarded(Zplan, None, x0n, nominal)
    Kb, _ = nlp.tracking_lqr_guarded(Zg, evg, Q, R, Q, nominal, with_cost_to_go=False)
    Zb, evb = nlp.tracking_rollout_guarded(Zg, Kb, x0d, model)
    torch.cuda.synchronize()
    nom = evg[0].cpu().numpy()
    print(f"planned touchdown: end of knot {kt - 2} (0-based); the nominal drop, rolled out guarded, lands in knot {int(nom[0])} at "
          f"tau = {nom[1]:.4e} s, clock {nom[2]:.4f} s")

    print(f"{'guarded roll-out of ' + str(S) + ' drops under':50s} {'median |x_N - x_ref,N|':>24s} {'max':>12s} {'keep the knot':>14s}")
    for name, Z, ev, ref in (("(a) plan + time-indexed TVLQR gains", Za, eva, Zplan), ("(b) Zg + gains of qln_tracking_lqr_guarded", Zb, evb, Zg)):
        xN = Z.view(S, -1)[:, 20 * (N - 1): 20 * (N - 1) + 14].cpu().numpy()
        xr = ref.view(S, -1)[:, 20 * (N - 1): 20 * (N - 1) + 14].cpu().numpy()
        err = np.linalg.norm(xN - xr, axis=1)
        keep = float((ev[:, 0] == evg[:, 0]).double().mean())
        print(f"{name:50s} {np.median(err):24.3e} {np.max(err):12.3e} {100 * keep:13.1f}%")
    same = (evb[:, 0] == evg[:, 0]).cpu().numpy()
    xN = Zb.view(S, -1)[:, 20 * (N - 1): 20 * (N - 1) + 14].cpu().numpy()
    xr = Zg.view(S, -1)[:, 20 * (N - 1): 20 * (N - 1) + 14].cpu().numpy()
    err = np.linalg.norm(xN - xr, axis=1)
    if same.any() and (~same).any():
        print(f"(b) by touchdown knot: median {np.median(err[same]):.3e} over the {int(same.sum())} drops that keep the nominal knot, "
              f"{np.median(err[~same]):.3e} over the {int((~same).sum())} that do not")

    # how uncertain is the moment of touchdown?  The drops' covariance: the foot height is uniform on +-HEIGHT (the foot mass is
    # a model perturbation, which a state covariance does not carry)
    var0 = np.zeros(15)
    var0[6] = HEIGHT ** 2 / 3.0
    for name, Zt, evt, K in (("open loop", Zg, evg, None), ("under (b)'s gains", Zg, evg, Kb)):
        _, _, var = nlp.tracking_covariance_guarded(Zt, evt, K, var0, None, nominal, with_sigma=False, with_marginals=False)
        print(f"touchdown clock, {name}: predicted standard deviation {float(var[0, 1].sqrt()):.4e} s (tau: {float(var[0, 0].sqrt()):.4e} s)")
    clock = evb[:, 2].cpu().numpy()
    print(f"touchdown clock, sample of (b): standard deviation {clock.std():.4e} s over all drops, {clock[same].std():.4e} s over those "
          f"that keep the knot (foot mass +-{100 * FOOT_MASS:.0f} % included)")


if __name__ == "__main__":
    main()
