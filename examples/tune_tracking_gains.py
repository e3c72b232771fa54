"""Tune TVLQR tracking gains through the closed-loop roll-out's gradient: solve the notebook's problem (N = 61,
k_trans = 21) with qln_solve, compute TVLQR gains, then run Adam on the gains (and, with --forces, on the feed-forward
forces) over a training batch of perturbed drop states, differentiating the nonlinear hybrid roll-out with
HybridNLP.differentiable_rollout.  The loss is the tracking cost written in torch on Zout (not eval_f, whose gradient
follows quirk Q2).  Prints held-out medians of the terminal error, the constraint violation and the objective for the
open loop, TVLQR and the tuned gains.
   python examples/tune_tracking_gains.py [--scale 0.05] [--steps 40] [--forces]
--scale is the drop-state perturbation, relative to |x0| with a floor of 0.1 (the tracking example uses 0.001)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from quadruped_landing_amd import HybridNLP, problem_gen as PG  # noqa: E402

S = 512  # drop states per batch (training and held-out)
Q = np.array([10.0] * 14 + [0.0])
R = np.array([1e-3, 1e-2, 1e-3, 1e-2])


def drop_states(x0, scale, seed):
    rng = np.random.default_rng(seed)
    x = np.tile(x0.reshape(1, 15), (S, 1))
    x[:, :14] += rng.normal(0.0, scale, size=(S, 14)) * np.maximum(np.abs(x[:, :14]), 0.1)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=0.05)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--forces", action="store_true", help="tune the feed-forward forces too")
    a = ap.parse_args()
    nb = PG.notebook_problem()
    N, n = nb.N, 20 * nb.N - 5
    one = HybridNLP(nb.model, nb.obj, nb.init_mode, nb.k_trans, N, nb.x0, nb.xf)
    Zs = one.upload_Z(nb.Z)
    one.solve(Zs)
    zref = Zs.cpu().numpy().reshape(-1)[:n]
    xtr, xte = drop_states(nb.x0, a.scale, 1), drop_states(nb.x0, a.scale, 2)
    nlp = HybridNLP(nb.model, nb.obj, np.full(S, nb.init_mode[0]), np.full(S, nb.k_trans[0]), N, xte,
                    np.tile(nb.xf.reshape(1, 15), (S, 1)))
    Zref = nlp.upload_Z(np.tile(zref, (S, 1)))
    K0, _ = nlp.tracking_lqr(Zref, Q, R, Q, with_cost_to_go=False)
    K0 = K0[0].clone()  # the same reference for every sample: one set of gains
    dev = Zref.device
    xi = torch.tensor([20 * k + i for k in range(N) for i in range(15)], device=dev)
    fi = torch.tensor([20 * k + 15 + m for k in range(N - 1) for m in range(4)], device=dev)
    wx, wf = torch.tensor(np.tile(Q, N), device=dev), torch.tensor(np.tile(R, N - 1), device=dev)
    zr = torch.from_numpy(zref).to(dev)

    def cost(Zo):  # tracking cost of every sample, in torch on the roll-out
        z = Zo.view(S, -1)
        return ((z[:, xi] - zr[xi]) ** 2 * wx).sum(1) + ((z[:, fi] - zr[fi]) ** 2 * wf).sum(1)

    sK = float(K0.abs().mean())
    theta = torch.zeros_like(K0, requires_grad=True)
    dF = torch.zeros(len(fi), dtype=torch.float64, device=dev, requires_grad=a.forces)
    opt = torch.optim.Adam([theta] + ([dF] if a.forces else []), lr=a.lr)

    def build(th, df):
        Kb = (K0 + sK * th).expand(S, *K0.shape).contiguous()
        Zr = Zref.view(S, -1).clone()
        Zr[:, fi] = Zr[:, fi] + df
        return Zr.reshape(-1), Kb

    x_tr = torch.from_numpy(xtr).to(dev)
    for step in range(a.steps):
        opt.zero_grad()
        Zr, Kb = build(theta, dF)
        loss = cost(nlp.differentiable_rollout(Zr, Kb, x_tr)).mean()
        loss.backward()
        opt.step()
        if step % 10 == 0 or step == a.steps - 1:
            print(f"step {step:3d}: training loss {loss.item():.5e}")
    x_te = torch.from_numpy(xte).to(dev)
    rows = []
    with torch.no_grad():
        Zr_t, K_t = build(theta, dF)
        for name, Zr, gains in (("open loop", Zref, None), ("TVLQR", Zref, K0.expand(S, *K0.shape).contiguous()),
                                ("tuned", Zr_t, K_t)):
            Zo = nlp.tracking_rollout(Zr, gains, x_te)
            viol = nlp.constraint_violation(nlp.eval_c(Zo)).cpu().numpy()
            f = nlp.eval_f(Zo).cpu().numpy()
            xN = Zo.view(S, -1)[:, 20 * (N - 1): 20 * (N - 1) + 14].cpu().numpy()
            err = np.linalg.norm(xN - zref[20 * (N - 1): 20 * (N - 1) + 14], axis=1)
            rows.append((name, np.median(err), np.median(viol), np.median(f), float(cost(Zo).median())))
    print(f"held-out: {S} drop states perturbed by {100 * a.scale:g} % (relative, floor 0.1); {a.steps} Adam steps on K"
          + (" and the feed-forward forces" if a.forces else ""))
    print(f"{'':10s} {'median |x_N - x_ref,N|':>24s} {'median violation':>17s} {'median objective':>17s} {'median cost':>12s}")
    for name, e, v, f, c in rows:
        print(f"{name:10s} {e:24.3e} {v:17.3e} {f:17.4f} {c:12.4e}")


if __name__ == "__main__":
    main()
