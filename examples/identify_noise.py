"""Which sensor variance do recorded landings speak for?  The 1 024 drops of examples/fly_estimated_landing.py (feet as planned,
the first sensor grade) are flown once, guarded, with estimate feedback.  Then the flight is forgotten but for what a logger
would keep: the measurements Y and the forces that were applied, the control slots of Zout.  For each scale s on a grid the filter
is redesigned for the sensor variance s V (qln_tracking_kalman_guarded), the records are replayed through it
(qln_landing_filter_guarded) and the Gaussian log-likelihoods are summed.  The curve peaks where the filter's V is the one the
sensors had; there the normalised innovation squared averages ny = 8 a knot.  Last, the replay's record (Xhat, innov) goes to
qln_landing_smoother_guarded, as a flight's own record would.
   python examples/identify_noise.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from estimate_landing import HEIGHT, NOISE, Q, R, S, W, sensors  # noqa: E402
from quadruped_landing_amd import HybridNLP, problem_gen as PG  # noqa: E402

SCALES = (0.25, 0.5, 0.7, 1.0, 1.4, 2.0, 4.0)


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
    sd0 = 1e-3 * np.maximum(np.abs(x0), 0.1)
    sd0[:, 14] = 0.0
    S0 = np.zeros((S, 120))
    S0[:, [i * (i + 3) // 2 for i in range(15)]] = sd0 * sd0
    H, sd = sensors(), NOISE[0]
    V = sd * sd
    gen = torch.Generator(device="cuda").manual_seed(0)
    randn = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=gen)  # noqa: E731

    # the flights: each drop's nominal, the filter for the sensors' own V, the loop flown under drawn noise
    Zg, events = nlp.tracking_rollout_guarded(Zref, K, torch.from_numpy(x0).cuda(), None)
    design = lambda v: nlp.tracking_kalman_guarded(Zg, events, H, v, K, S0, W, None, with_sigma=False, with_marginals=False,  # noqa: E731
                                                   with_event_var=False)[:2]
    L, _ = design(V)
    xs = torch.from_numpy(x0).cuda() + randn(S, 15) * torch.from_numpy(sd0).cuda()
    v, w = sd * randn(S, N, 8), randn(S, N - 1, 15) * torch.from_numpy(np.sqrt(W)).cuda()
    Zo, Xf, _, _, evf = nlp.tracking_rollout_estimated(Zg, K, L, H, v, w, xs, None, None, guarded=True)

    # what a logger keeps: the readings (less H x_ref, the form the filter takes them in) and the applied forces
    Y = nlp.landing_measurements(Zo, Zg, H, v)
    Zrec = torch.full_like(Zo, float("nan"))          # the states of the record are not read ...
    ctrl = (20 * torch.arange(N - 1, device="cuda")[:, None] + 15 + torch.arange(5, device="cuda")[None, :]).reshape(-1)
    Zrec.view(S, -1)[:, ctrl] = Zo.view(S, -1)[:, ctrl]  # ... only the four forces and h_k of every knot

    print(f"{S} recorded landings, N = {N}, ny = 8, sensor sd {sd:.0e} (V = {V:.0e}); filter redesigned for s V, records replayed")
    print(f"{'s':>6s} {'sum loglik':>16s} {'per landing':>12s} {'mean nis per knot':>18s}")
    curve = {}
    for s in SCALES:
        Ls, Ps = design(s * V)
        Xh, iv, sc, ll, evh = nlp.landing_filter_guarded(Zg, Zrec, Ls, H, Y, s * V)
        curve[s] = float(ll.sum())
        print(f"{s:6.2f} {curve[s]:16.3f} {curve[s] / S:12.3f} {float(sc[..., 0].mean()):18.3f}")
        if s == 1.0:
            rec = (Ls, Ps, Xh, iv, sc)
            worst = float((Xh - Xf).abs().max())
            knots = int((evh[:, 0] != evf[:, 0]).sum())
    best = max(curve, key=curve.get)
    Ls, Ps, Xh, iv, sc = rec
    nis = sc[..., 0].mean(dim=0).cpu().numpy()
    print(f"maximiser on the grid: s = {best:.2f}")
    print(f"at s = 1: mean nis per knot in [{nis.min():.3f}, {nis.max():.3f}] (ny = 8; five standard deviations of a mean of {S}: "
          f"+-{5 * np.sqrt(2 * 8 / S):.3f}); replayed Xhat within {worst:.1e} of the flight's, {knots} estimators land in another knot")

    # the replay's record is a record: the smoother takes it
    Xs, _ = nlp.landing_smoother_guarded(Zg, events, Ls, Ps, H, V, Xh, iv, None, with_cov=False)
    z = torch.cat([Zo.view(S, -1)[:, :n], torch.zeros(S, 5, dtype=torch.float64, device="cuda")], dim=1).view(S, N, 20)[:, :, :15]
    rms = lambda e: float(torch.sqrt((e[:, :-1, :14] ** 2).mean()))  # noqa: E731
    print(f"smoother on the replay's record: rms of flown - Xs over rms of flown - Xhat, knots 0..N-2: {rms(z - Xs) / rms(z - Xh):.3f}")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
