"""What did a landing do, once it has been flown?  The 1 024 drops and the two sensor grades of
examples/fly_estimated_landing.py -- the notebook's problem solved with qln_solve, the free foot up to 2 cm higher or lower than
planned, each drop flown guarded with estimate feedback under drawn noise -- are SMOOTHED: qln_landing_smoother_guarded runs
backward over each flight's record (Xhat, innov) on the gains and covariances qln_tracking_kalman_guarded designed, and returns
the state at every knot given all N measurements, where the filter's estimate at knot k had seen k + 1 of them.  Against the
true flown states it prints
  * the root-mean-square error of the filtered and of the smoothed estimate, per group of knots;
  * the error of the smoothed drop state in the standard deviations the call predicts for it (Ps at knot 0; 1 if that holds);
  * the error of the moment of touchdown read off the filtered and off the smoothed state of the touchdown knot.
   python examples/smooth_landing.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from estimate_landing import HEIGHT, NOISE, Q, R, S, W, sensors  # noqa: E402
from quadruped_landing_amd import HybridNLP, nlp as NL, problem_gen as PG  # noqa: E402


def touchdown_time(x, Fy, h, g, mf):
    """The guard's closed form (include/qln_evaluator.h): the first root in [0, h] of the free foot's height y + v t + a t^2 / 2
    under the held force, a = -F_y / mf + g, from a state's y = x[6] and v = x[13] (init_mode 1: foot 2 is the free one)."""
    y, v = x[:, 6], x[:, 13]
    a = -Fy / mf + g
    with np.errstate(invalid="ignore", divide="ignore"):
        tau = 2 * y / (-v + np.sqrt(v * v - 2 * a * y))
    return np.clip(np.where(y <= 0, 0.0, tau), 0.0, h)


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
    Zref = nlp.upload_Z(np.tile(zref, (S, 1)))
    K, _ = nlp.tracking_lqr(Zref, Q, R, Q, with_cost_to_go=False)
    sd0 = 1e-3 * np.maximum(np.abs(x0), 0.1)  # 0.1 % of each drop-state entry (floor 1e-4 absolute); the clock is known
    sd0[:, 14] = 0.0
    S0 = np.zeros((S, 120))
    S0[:, [i * (i + 3) // 2 for i in range(15)]] = sd0 * sd0
    H = sensors()
    gen = torch.Generator(device="cuda").manual_seed(0)
    randn = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=gen)  # noqa: E731
    rows = np.arange(S)

    # the drop's nominal: the guarded roll-out under state feedback, as examples/fly_estimated_landing.py
    Zg, events = nlp.tracking_rollout_guarded(Zref, K, torch.from_numpy(x0).cuda())
    ev = events.cpu().numpy()
    groups = [("knot 0 (the drop)", [0]), ("knots 1 .. N/3", range(1, N // 3)), ("knots N/3 .. 2N/3", range(N // 3, 2 * N // 3)),
              ("knots 2N/3 .. N-2", range(2 * N // 3, N - 1)), ("knot N-1", [N - 1])]
    print(f"{S} drops, N = {N}; rms error against the flown states, all 15 entries, filtered -> smoothed")
    for sd in NOISE:
        L, Pe, _, _, _ = nlp.tracking_kalman_guarded(Zg, events, H, sd * sd, None, S0, W)
        xs = torch.from_numpy(x0).cuda() + randn(S, 15) * torch.from_numpy(sd0).cuda()
        v, w = sd * randn(S, N, 8), randn(S, N - 1, 15) * torch.from_numpy(np.sqrt(W)).cuda()
        Zo, Xhat, innov, evp, _ = nlp.tracking_rollout_estimated(Zg, K, L, H, v, w, xs, guarded=True, with_innovations=True)
        Xs, Ps = nlp.landing_smoother_guarded(Zg, events, L, Pe, H, sd * sd, Xhat, innov)
        torch.cuda.synchronize()
        zo = np.concatenate([Zo.view(S, -1)[:, :n].cpu().numpy(), np.zeros((S, 5))], axis=1).reshape(S, N, 20)
        xt, xh, xsm, evp = zo[:, :, :15], Xhat.cpu().numpy(), Xs.cpu().numpy(), evp.cpu().numpy()
        print(f"sensor sd {sd:.0e}:")
        for name, ks in groups:
            ks = list(ks)
            ef, es = np.sqrt(np.mean((xt - xh)[:, ks] ** 2)), np.sqrt(np.mean((xt - xsm)[:, ks] ** 2))
            print(f"  {name:20s} {ef:10.3e} -> {es:10.3e}   ({es / ef:.3f})")
        # the drop state in predicted standard deviations: the clock is known exactly and is left out
        sd_s = np.sqrt(np.diagonal(NL.unpack_covariance(Ps)[:, 0], axis1=-2, axis2=-1))[:, :14]
        sd_f = np.sqrt(np.diagonal(NL.unpack_covariance(Pe)[:, 0], axis1=-2, axis2=-1))[:, :14]
        print(f"  drop state: rms of (flown - smoothed) / predicted sd {np.sqrt(np.mean(((xt - xsm)[:, 0, :14] / sd_s) ** 2)):.3f}; "
              f"median predicted sd, smoothed over filtered {np.median(sd_s / sd_f):.3f}")
        # the moment of touchdown, from the state estimate of the plant's touchdown knot and the force the flight applied there
        land = (evp[:, 0] >= 0) & (evp[:, 0] == ev[:, 0])
        k = evp[land, 0].astype(int)
        r = rows[land]
        Fy, h = zo[r, k, 18], zo[r, k, 19]
        t_f = touchdown_time(xh[r, k], Fy, h, nb.model.g, nb.model.mf)
        t_s = touchdown_time(xsm[r, k], Fy, h, nb.model.g, nb.model.mf)
        rf, rs = np.sqrt(np.mean((t_f - evp[land, 1]) ** 2)), np.sqrt(np.mean((t_s - evp[land, 1]) ** 2))
        print(f"  moment of touchdown ({int(land.sum())} drops landing in their nominal's knot): rms error {rf:.3e} s filtered -> "
              f"{rs:.3e} s smoothed   ({rs / rf:.3f})")


if __name__ == "__main__":
    main()
