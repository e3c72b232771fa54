"""The sensor variance of examples/identify_noise.py found by its gradient instead of a grid.  The same 1 024 recorded landings;
the summed log-likelihood is maximised over a = log of the scale of V by secant steps on its derivative, then over (a, b), b = log
of the scale of W, by quasi-Newton (BFGS) steps on its gradient.  The derivative is HybridNLP.landing_loglik_jvp: the TOTAL
derivative through the gains' design (qln_kalman_design_guarded_jvp, qln_landing_filter_guarded_jvp and three einsums), along
V_dot = V (d V / d a) and W_dot = W (d W / d b).  Every step designs the filter once, replays the records once and takes one sweep
per unknown; the grid of examples/identify_noise.py designs the filter once per point.
   python examples/identify_noise_gradient.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from estimate_landing import HEIGHT, NOISE, Q, R, S, W, sensors  # noqa: E402
from identify_noise import SCALES  # noqa: E402
from quadruped_landing_amd import HybridNLP, problem_gen as PG  # noqa: E402

STEP_MAX = 1.0   # a step in the log-scales is at most this long
TOL = 1e-4       # ... and the search stops below this


def main():
    nb = PG.notebook_problem()
    N, n, kt = nb.N, 20 * nb.N - 5, int(nb.k_trans[0])
    one = HybridNLP(nb.model, nb.obj, nb.init_mode, nb.k_trans, N, nb.x0, nb.xf)
    Zs = one.upload_Z(nb.Z)
    _, info = one.solve(Zs)
    zref = Zs.cpu().numpy().reshape(-1)[:n]
    print(f"solve: status {int(info[0, 5])}, violation {float(info[0, 3]):.2e}, objective {float(info[0, 2]):.4f}")

    # the flights and their records, exactly as examples/identify_noise.py draws them
    rng = np.random.default_rng(0)
    x0 = np.tile(nb.x0.reshape(1, 15), (S, 1))
    x0[:, 6] += rng.uniform(-HEIGHT, HEIGHT, size=S)
    nlp = HybridNLP(nb.model, nb.obj, np.full(S, nb.init_mode[0]), np.full(S, kt), N, x0, np.tile(nb.xf.reshape(1, 15), (S, 1)))
    Zref = nlp.upload_Z(np.tile(zref, (S, 1)))
    K, _ = nlp.tracking_lqr(Zref, Q, R, Q, with_cost_to_go=False)
    sd0 = 1e-3 * np.maximum(np.abs(x0), 0.1)
    sd0[:, 14] = 0.0
    S0 = np.zeros((S, 120))
    S0[:, [i * (i + 3) // 2 for i in range(15)]] = sd0 * sd0
    H, sd = sensors(), NOISE[0]
    V = np.full(8, sd * sd)
    gen = torch.Generator(device="cuda").manual_seed(0)
    randn = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=gen)  # noqa: E731
    Zg, events = nlp.tracking_rollout_guarded(Zref, K, torch.from_numpy(x0).cuda(), None)
    counts = {"designs": 0}

    def design(v, w):
        counts["designs"] += 1
        return nlp.tracking_kalman_guarded(Zg, events, H, v, None, S0, w, None)[0]

    L = design(V, W)
    xs = torch.from_numpy(x0).cuda() + randn(S, 15) * torch.from_numpy(sd0).cuda()
    v, w = sd * randn(S, N, 8), randn(S, N - 1, 15) * torch.from_numpy(np.sqrt(W)).cuda()
    Zo, _, _, _, _ = nlp.tracking_rollout_estimated(Zg, K, L, H, v, w, xs, None, None, guarded=True)
    Y = nlp.landing_measurements(Zo, Zg, H, v)
    Zrec = torch.full_like(Zo, float("nan"))
    ctrl = (20 * torch.arange(N - 1, device="cuda")[:, None] + 15 + torch.arange(5, device="cuda")[None, :]).reshape(-1)
    Zrec.view(S, -1)[:, ctrl] = Zo.view(S, -1)[:, ctrl]

    def score(a, b, unknowns):
        """(sum loglik, its gradient in the unknowns) at V e^a, W e^b: one design, one replay, one sweep per unknown"""
        va, wb = np.exp(a) * V, np.exp(b) * W
        Ls = design(va, wb)
        Xh, iv, _, ll, evh = nlp.landing_filter_guarded(Zg, Zrec, Ls, H, Y, va)
        g = []
        for u in unknowns:
            d = dict(V_dot=va) if u == "a" else dict(W_dot=wb)
            ld, _, _ = nlp.landing_loglik_jvp(Zg, Zg, Zrec, Ls, H, va, Xh, iv, events=events, guarded_design=True, events_hat=evh,
                                              guarded=True, **d)
            g.append(float(ld.sum()))
        return float(ll.sum()), np.array(g)

    print(f"{S} recorded landings, N = {N}, ny = 8, sensor sd {sd:.0e}; V e^a and W e^b, a = b = 0 is what the flights had")
    # -- the grid of examples/identify_noise.py, for the comparison --------------------------------------------------------
    counts["designs"] = 0
    grid = {s: score(np.log(s), 0.0, ())[0] for s in SCALES}
    best = max(grid, key=grid.get)
    print(f"grid of {len(SCALES)} scales: maximiser s = {best:.2f} (sum loglik {grid[best]:.3f}), {counts['designs']} designs")

    # -- one unknown: secant steps on d loglik / d a ----------------------------------------------------------------------
    counts["designs"] = 0
    a0 = float(np.log(SCALES[0]))
    f0, g0 = score(a0, 0.0, "a")
    a1 = a0 + 0.5 * np.sign(g0[0])
    print(f"{'step':>4s} {'scale of V':>11s} {'sum loglik':>16s} {'d / d a':>13s}")
    print(f"{0:4d} {np.exp(a0):11.5f} {f0:16.3f} {g0[0]:13.3f}")
    for it in range(1, 20):
        f1, g1 = score(a1, 0.0, "a")
        print(f"{it:4d} {np.exp(a1):11.5f} {f1:16.3f} {g1[0]:13.3f}")
        step = -g1[0] * (a1 - a0) / (g1[0] - g0[0])
        step = float(np.clip(step, -STEP_MAX, STEP_MAX))
        a0, g0, a1 = a1, g1, a1 + step
        if abs(step) < TOL:
            break
    a_star = a1
    print(f"secant on the gradient: scale of V = {np.exp(a_star):.4f} after {counts['designs']} designs "
          f"(the grid: {best:.2f} after {len(SCALES)})")

    # -- two unknowns: BFGS steps on the gradient in (a, b), from the grid's corner -----------------------------------------
    counts["designs"] = 0
    x = np.array([np.log(SCALES[0]), np.log(4.0)])
    f, g = score(x[0], x[1], "ab")
    Binv = np.eye(2) / max(np.abs(g).max(), 1.0)  # the first step is a clipped gradient step
    print(f"{'step':>4s} {'scale of V':>11s} {'scale of W':>11s} {'sum loglik':>16s} {'d / d a':>13s} {'d / d b':>13s}")
    print(f"{0:4d} {np.exp(x[0]):11.5f} {np.exp(x[1]):11.5f} {f:16.3f} {g[0]:13.3f} {g[1]:13.3f}")
    for it in range(1, 25):
        p = Binv @ g  # ascent on loglik
        if np.linalg.norm(p) > STEP_MAX:
            p *= STEP_MAX / np.linalg.norm(p)
        xn = x + p
        fn, gn = score(xn[0], xn[1], "ab")
        print(f"{it:4d} {np.exp(xn[0]):11.5f} {np.exp(xn[1]):11.5f} {fn:16.3f} {gn[0]:13.3f} {gn[1]:13.3f}")
        s_, y_ = xn - x, -(gn - g)  # BFGS on -loglik
        if s_ @ y_ > 1e-12:
            rho = 1.0 / (s_ @ y_)
            E = np.eye(2) - rho * np.outer(s_, y_)
            Binv = E @ Binv @ E.T + rho * np.outer(s_, s_)
        x, f, g = xn, fn, gn
        if np.linalg.norm(p) < TOL:
            break
    print(f"BFGS on the gradient: scale of V = {np.exp(x[0]):.4f}, scale of W = {np.exp(x[1]):.4f}, sum loglik {f:.3f}, "
          f"after {counts['designs']} designs")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
