"""Does a noisy landing do what the Kalman layer predicts?  The 1 024 drops and the two sensor grades of
examples/estimate_landing.py -- the notebook's problem solved with qln_solve, the free foot up to 2 cm higher or lower than
planned, the feet up to 10 % lighter or heavier, each drop rolled out with the guarded touchdown under TVLQR gains -- are FLOWN
with estimate feedback: qln_tracking_rollout_estimated_guarded rolls each drop's plant and a Kalman filter out together along
the drop's own nominal, with a drop state drawn from the 0.1 % covariance, sensor noise and process noise drawn by torch.randn.
Beside each figure qln_tracking_kalman_guarded predicts -- the standard deviation of the touchdown clock (event_var), of the
vertical force at the drop's tightest force margin, of the clearance at its tightest clearance margin -- it prints the sampled
one: the root mean square, over the drops, of the flown deviation from the nominal, in predicted standard deviations (1 if the
prediction holds), and how many drops landed in another knot than their nominal.  Each grade is flown twice: with the feet as
planned, where the filter's model is the plant's, and with the drawn foot masses, where it is not -- the filter always predicts
with the handle's model, and the prediction knows nothing of that error.
   python examples/fly_estimated_landing.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from estimate_landing import FOOT_MASS, HEIGHT, NOISE, Q, R, S, W, sensors  # noqa: E402
from quadruped_landing_amd import HybridNLP, problem_gen as PG  # noqa: E402


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
    drawn = nlp.plant_models()
    drawn[:, 2] *= torch.from_numpy(1.0 + rng.uniform(-FOOT_MASS, FOOT_MASS, size=S)).cuda()
    Zref = nlp.upload_Z(np.tile(zref, (S, 1)))
    K, _ = nlp.tracking_lqr(Zref, Q, R, Q, with_cost_to_go=False)
    sd0 = 1e-3 * np.maximum(np.abs(x0), 0.1)  # 0.1 % of each drop-state entry (floor 1e-4 absolute); the clock is known
    sd0[:, 14] = 0.0
    S0 = np.zeros((S, 120))
    S0[:, [i * (i + 3) // 2 for i in range(15)]] = sd0 * sd0
    H, lb = sensors(), nb.model.lb
    knots, rows = 20 * np.arange(N), np.arange(S)
    gen = torch.Generator(device="cuda").manual_seed(0)
    randn = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=gen)  # noqa: E731
    clearance = lambda z: z[:, knots + 1] - lb / 2 * np.abs(np.sin(z[:, knots + 2]))  # noqa: E731

    print(f"{S} drops; sampled = rms over the drops of (flown - nominal) / predicted sd")
    print(f"{'':44s} {'touchdown clock':>28s} {'F_y at tightest margin':>28s} {'clearance at tightest':>28s} {'other knot':>11s}")
    print(f"{'':44s} {'pred. median sd [s]':>19s} {'sampled':>8s} {'pred. min margin [sd]':>19s} {'sampled':>6s} "
          f"{'pred. max var [m^2]':>19s} {'sampled':>8s} {'plant':>5s} {'est.':>5s}")
    for feet, model in (("as planned", None), (f"+-{100 * FOOT_MASS:.0f} %", drawn)):
        # the drop's nominal: the guarded roll-out under state feedback, as examples/estimate_landing.py
        Zg, events = nlp.tracking_rollout_guarded(Zref, K, torch.from_numpy(x0).cuda(), model)
        z, ev = Zg.view(S, -1)[:, :n].cpu().numpy(), events.cpu().numpy()
        for sd in NOISE:
            L, _, _, mg, var = nlp.tracking_kalman_guarded(Zg, events, H, sd * sd, K, S0, W, model, with_pest=False, with_sigma=False)
            mg, var = mg.cpu().numpy(), var.cpu().numpy()
            # the flight: the drop state, the sensor noise and the process noise are drawn here, the library draws nothing
            xs = torch.from_numpy(x0).cuda() + randn(S, 15) * torch.from_numpy(sd0).cuda()
            v, w = sd * randn(S, N, 8), randn(S, N - 1, 15) * torch.from_numpy(np.sqrt(W)).cuda()
            Zo, _, _, evp, evh = nlp.tracking_rollout_estimated(Zg, K, L, H, v, w, xs, None, model, guarded=True)
            zo, evp, evh = Zo.view(S, -1)[:, :n].cpu().numpy(), evp.cpu().numpy(), evh.cpu().numpy()
            same = (ev[:, 0] >= 0) & (evp[:, 0] == ev[:, 0])
            rms = lambda d, s: float(np.sqrt(np.mean((d / s) ** 2)))  # noqa: E731
            clock = rms((evp[same, 2] - ev[same, 2]), np.sqrt(var[same, 1]))
            # the vertical force (foot 1: u[1], foot 2: u[3]) at the knot and foot of the drop's tightest predicted margin
            fy = np.stack([z[:, knots[:-1] + 16], z[:, knots[:-1] + 18]], axis=-1).reshape(S, -1)
            fo = np.stack([zo[:, knots[:-1] + 16], zo[:, knots[:-1] + 18]], axis=-1).reshape(S, -1)
            sf = np.sqrt(mg[:, :-1, [2, 4]]).reshape(S, -1)
            with np.errstate(divide="ignore", invalid="ignore"):
                margin = np.where(sf > 0, np.abs(fy) / sf, np.inf)
            at = margin.argmin(axis=1)
            force = rms((fo - fy)[rows, at], sf[rows, at])
            # the clearance at the knot of the drop's tightest predicted clearance margin
            c, co = clearance(z), clearance(zo)
            with np.errstate(divide="ignore", invalid="ignore"):
                cm = np.where(mg[:, :, 0] > 0, c / np.sqrt(mg[:, :, 0]), np.inf)
            ck = cm.argmin(axis=1)
            clear = rms((co - c)[rows, ck], np.sqrt(mg[rows, ck, 0]))
            print(f"feet {feet:10s} sensor sd {sd:.0e} {'':15s} {np.median(np.sqrt(var[same, 1])):19.3e} {clock:8.3f} "
                  f"{margin[rows, at].min():19.2f} {force:6.3f}   {mg[rows, ck, 0].max():19.3e} {clear:8.3f} "
                  f"{int((evp[:, 0] != ev[:, 0]).sum()):5d} {int((evh[:, 0] != evp[:, 0]).sum()):5d}")
    torch.cuda.synchronize()
    print("other knot: drops whose plant lands in another knot than its nominal (left out of the clock's figure), and whose "
          "estimator lands in another knot than its plant")


if __name__ == "__main__":
    main()
