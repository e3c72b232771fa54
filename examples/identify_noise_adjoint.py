"""Every diagonal entry of the process and the sensor noise of examples/identify_noise.py found at once, by the adjoint.  The same
1 024 recorded landings; the summed log-likelihood is maximised over the 15 + ny logarithms of the scales of W's and V's entries
by quasi-Newton (BFGS) steps with backtracking.  The gradient is HybridNLP.landing_loglik_grad: one design, one replay of the
records and two reverse sweeps (qln_landing_filter_guarded_vjp, qln_noise_design_guarded_vjp) give all 15 + ny entries, where
forward mode (examples/identify_noise_gradient.py, which therefore fits two scales) takes one design sweep per entry.
   python examples/identify_noise_adjoint.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from estimate_landing import HEIGHT, NOISE, Q, R, S, W, sensors  # noqa: E402
from quadruped_landing_amd import HybridNLP, problem_gen as PG  # noqa: E402

STEP_MAX = 1.0   # a step in the log-scales is at most this long
TOL = 1e-3       # ... and the search stops below this
STEPS = 60
START = 4.0      # every scale starts this factor away from what the flights had, V above and W below


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
    ny = H.shape[0]
    V = np.full(ny, sd * sd)
    Wv = np.broadcast_to(np.asarray(W, dtype=np.float64), (15,)).copy()
    gen = torch.Generator(device="cuda").manual_seed(0)
    randn = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=gen)  # noqa: E731
    Zg, events = nlp.tracking_rollout_guarded(Zref, K, torch.from_numpy(x0).cuda(), None)
    counts = {"designs": 0, "gradients": 0}

    def design(v, w):
        counts["designs"] += 1
        return nlp.tracking_kalman_guarded(Zg, events, H, v, None, S0, w, None)[0]

    L = design(V, Wv)
    xs = torch.from_numpy(x0).cuda() + randn(S, 15) * torch.from_numpy(sd0).cuda()
    v, w = sd * randn(S, N, ny), randn(S, N - 1, 15) * torch.from_numpy(np.sqrt(Wv)).cuda()
    Zo, _, _, _, _ = nlp.tracking_rollout_estimated(Zg, K, L, H, v, w, xs, None, None, guarded=True)
    Y = nlp.landing_measurements(Zo, Zg, H, v)
    Zrec = torch.full_like(Zo, float("nan"))
    ctrl = (20 * torch.arange(N - 1, device="cuda")[:, None] + 15 + torch.arange(5, device="cuda")[None, :]).reshape(-1)
    Zrec.view(S, -1)[:, ctrl] = Zo.view(S, -1)[:, ctrl]

    def value(x):
        """(sum loglik, what its gradient needs) at W e^x[:15], V e^x[15:]: one design and one replay of the records"""
        wb, va = np.exp(x[:15]) * Wv, np.exp(x[15:]) * V
        Ls = design(va, wb)
        Xh, iv, _, ll, evh = nlp.landing_filter_guarded(Zg, Zrec, Ls, H, Y, va)
        return float(ll.sum()), (wb, va, Ls, Xh, iv, evh)

    def gradient(at):
        """the gradient in the 15 + ny log-scales at value()'s point: the two reverse sweeps"""
        wb, va, Ls, Xh, iv, evh = at
        counts["gradients"] += 1
        g = nlp.landing_loglik_grad(Zg, Zg, Zrec, Ls, H, va, Xh, iv, events=events, guarded_design=True, events_hat=evh,
                                    guarded=True)
        return np.concatenate([g["W"].sum(0).cpu().numpy() * wb, g["V"].sum(0).cpu().numpy() * va])

    m = 15 + ny
    print(f"{S} recorded landings, N = {N}, ny = {ny}, sensor sd {sd:.0e}; {m} unknowns: the log-scales of W's 15 and V's {ny} "
          "entries, all 0 is what the flights had")
    counts["designs"] = 0
    f_true, _ = value(np.zeros(m))
    counts["designs"] = 0
    x = np.concatenate([np.full(15, -np.log(START)), np.full(ny, np.log(START))])
    f, at = value(x)
    g = gradient(at)
    Binv = np.eye(m) / max(np.abs(g).max(), 1.0)  # the first step is a clipped gradient step
    print(f"{'step':>4s} {'sum loglik':>16s} {'|gradient|':>12s} {'|step|':>9s} {'scales of V: min':>17s} {'max':>8s} "
          f"{'scales of W: min':>17s} {'max':>8s}")
    row = lambda it, f, g, p, x: print(f"{it:4d} {f:16.3f} {np.linalg.norm(g):12.3f} {p:9.4f} {np.exp(x[15:].min()):17.4f} "  # noqa: E731
                                       f"{np.exp(x[15:].max()):8.4f} {np.exp(x[:15].min()):17.4f} {np.exp(x[:15].max()):8.4f}")
    row(0, f, g, 0.0, x)
    for it in range(1, STEPS + 1):
        p = Binv @ g  # ascent on loglik
        if not np.isfinite(p).all() or p @ g <= 0.0:
            p, Binv = g / max(np.abs(g).max(), 1.0), np.eye(m) / max(np.abs(g).max(), 1.0)
        if np.linalg.norm(p) > STEP_MAX:
            p *= STEP_MAX / np.linalg.norm(p)
        for _ in range(8):  # backtracking on the value alone: a design and a replay per trial, no sweep
            fn, at = value(x + p)
            if np.isfinite(fn) and fn >= f:
                break
            p = 0.5 * p
        else:
            fn, at = value(x + p)
        xn, gn = x + p, gradient(at)
        row(it, fn, gn, float(np.linalg.norm(p)), xn)
        s_, y_ = xn - x, -(gn - g)  # BFGS on -loglik
        if s_ @ y_ > 1e-12:
            rho = 1.0 / (s_ @ y_)
            E = np.eye(m) - rho * np.outer(s_, y_)
            Binv = E @ Binv @ E.T + rho * np.outer(s_, s_)
        x, f, g = xn, fn, gn
        if np.linalg.norm(p) < TOL:
            break
    names = [f"W[{i}]" for i in range(15)] + [f"V[{i}]" for i in range(ny)]
    print("scales found (1 is what the flights had; an entry the records say little about stays where the search left it):")
    for i in range(0, m, 6):
        print("   " + "  ".join(f"{names[q]} {np.exp(x[q]):8.4f}" for q in range(i, min(i + 6, m))))
    print(f"sum loglik {f:.3f} at the scales found, {f_true:.3f} at the scales the flights had")
    print(f"{counts['gradients']} gradients of {m} entries and {counts['designs']} designs; each gradient is one reverse design sweep, "
          f"where forward mode takes {m} forward sweeps: {counts['gradients']} against {m * counts['gradients']} design sweeps")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
