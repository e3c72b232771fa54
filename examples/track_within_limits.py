"""Track the landing with feet that can only push and legs that have a force limit.  The experiment of
examples/touchdown_timing.py -- the notebook's problem (N = 61, k_trans = 21) solved with qln_solve, 1 024 drops whose free
foot starts up to 2 cm higher or lower than planned and whose feet are up to 10 % lighter or heavier -- rolled out guarded
under contact-aware force limits (qln_tracking_rollout_limited): a standing foot's vertical force stays in [0, cap], a free
foot's forces in +-cap, the two caps at 90 % of the largest forces of the nominal drop, so that its peaks ride them.  Two designs:
  (a) the guarded roll-out of the plan as reference with qln_tracking_lqr_guarded's gains, which do not know about the limits;
  (b) the LIMITED roll-out of the plan as reference with qln_tracking_lqr_limited's gains along it, designed at its active set.
Prints, for both, the terminal error, the touchdown clock's spread, the share of saturated (knot, channel) pairs and the
smallest force under a standing foot (the event record's entry 6), and the same for (a)'s controller without the limits.
   python examples/track_within_limits.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from quadruped_landing_amd import HybridNLP, problem_gen as PG  # noqa: E402
from quadruped_landing_amd.nlp import unpack_saturation  # noqa: E402

S = 1024
Q = np.array([10.0] * 14 + [0.0])
R = np.array([1e-3, 1e-2, 1e-3, 1e-2])
HEIGHT, FOOT_MASS = 0.02, 0.10  # +- 2 cm of free-foot start height, +- 10 % of foot mass
CAP = 0.90                      # the caps: this much of the nominal drop's largest force of the kind


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

    # the nominal drop rolled out guarded (open loop, the design model), and the limits from its forces
    Zg, evg = nlp.tracking_rollout_guarded(Zplan, None, x0n, nominal)
    F = np.concatenate([Zg.view(S, -1)[0, :n].cpu().numpy(), np.zeros(5)]).reshape(N, 20)[: N - 1, 15:19]
    ks = int(evg[0, 0])
    stand_y = np.concatenate([F[:, 1], F[ks + 1:, 3]])
    free = F[: ks + 1, 2:4]
    cap_y, cap_free = CAP * float(stand_y.max()), CAP * float(np.abs(free).max())
    inf = np.inf
    lim = np.array([-cap_free, cap_free, -cap_free, cap_free, -inf, inf, 0.0, cap_y])
    print(f"the nominal drop lands in knot {ks}; its standing feet push with {stand_y.min():.3f} .. {stand_y.max():.3f} N, its free foot "
          f"is driven with up to {np.abs(free).max():.3f} N")
    print(f"limits: standing F_y in [0, {cap_y:.3f}] N, free-foot forces in +-{cap_free:.3f} N, standing F_x unlimited")

    # (a) gains through the touchdown that do not know about the limits; (b) the limited nominal and gains at its active set
    Ka, _ = nlp.tracking_lqr_guarded(Zg, evg, Q, R, Q, nominal, with_cost_to_go=False)
    Zn, evn, satn = nlp.tracking_rollout_limited(Zplan, lim, None, x0n, nominal, guarded=True)
    Kb, _ = nlp.tracking_lqr_limited(Zn, satn, Q, R, Q, evn, nominal, with_cost_to_go=False)
    print(f"the limited nominal: {int((unpack_saturation(satn[0]) != 0).sum())} of {4 * (N - 1)} (knot, channel) pairs ride a limit, "
          f"touchdown in knot {int(evn[0, 0])}")

    Z0, ev0 = nlp.tracking_rollout_guarded(Zg, Ka, x0d, model)
    Za, eva, sata = nlp.tracking_rollout_limited(Zg, lim, Ka, x0d, model, guarded=True)
    Zb, evb, satb = nlp.tracking_rollout_limited(Zn, lim, Kb, x0d, model, guarded=True)
    torch.cuda.synchronize()

    head = f"{'guarded roll-out of ' + str(S) + ' drops under':58s} {'median |x_N - x_ref,N|':>24s} {'max':>12s} {'clock std [s]':>14s} " \
           f"{'saturated':>10s} {'min standing F_y [N]':>22s}"
    print(head)
    rows = (("(a) without limits: Zg + gains of qln_tracking_lqr_guarded", Z0, ev0, None, Zg),
            ("(a) within limits:  Zg + gains of qln_tracking_lqr_guarded", Za, eva, sata, Zg),
            ("(b) within limits:  Zn + gains of qln_tracking_lqr_limited", Zb, evb, satb, Zn))
    for name, Z, ev, sat, ref in rows:
        xN = Z.view(S, -1)[:, 20 * (N - 1): 20 * (N - 1) + 14].cpu().numpy()
        xr = ref.view(S, -1)[:, 20 * (N - 1): 20 * (N - 1) + 14].cpu().numpy()
        err = np.linalg.norm(xN - xr, axis=1)
        e = ev.cpu().numpy()
        clock = e[e[:, 0] >= 0, 2]
        share = "-" if sat is None else f"{100 * float((unpack_saturation(sat) != 0).mean()):.2f}%"
        print(f"{name:58s} {np.median(err):24.3e} {np.max(err):12.3e} {clock.std():14.4e} {share:>10s} {e[:, 6].min():22.4e}")
    print("(b)'s reference forces already lie on the caps where the nominal rides them, and its gains' rows are zero there: such a "
          "force equals its limit and counts as free")
    for name, ev in (("(a) within limits", eva), ("(b) within limits", evb)):
        assert float(ev[:, 6].min()) >= lim[6], name  # the ground no longer pulls
    print(f"the ground pulls (F_y < 0 under a standing foot) in {int((ev0[:, 6] < 0).sum())} of {S} drops without limits, in "
          f"{int((eva[:, 6] < 0).sum())} and {int((evb[:, 6] < 0).sum())} within them")


if __name__ == "__main__":
    main()
