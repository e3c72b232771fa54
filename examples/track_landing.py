"""Closed-loop tracking of a solved landing: solve the notebook's problem (N = 61, k_trans = 21) with qln_solve, compute
TVLQR gains with the notebook's weights, roll 1 024 perturbed drop states out open and closed loop, and compare the
terminal-state error, the constraint violation and the objective of both.
   python examples/track_landing.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from quadruped_landing_amd import HybridNLP, problem_gen as PG  # noqa: E402

S = 1024
Q = np.array([10.0] * 14 + [0.0])
R = np.array([1e-3, 1e-2, 1e-3, 1e-2])


def main():
    nb = PG.notebook_problem()
    N, n = nb.N, 20 * nb.N - 5
    one = HybridNLP(nb.model, nb.obj, nb.init_mode, nb.k_trans, N, nb.x0, nb.xf)
    Zs = one.upload_Z(nb.Z)
    _, info = one.solve(Zs)
    zref = Zs.cpu().numpy().reshape(-1)[:n]
    print(f"solve: status {int(info[0, 5])}, violation {float(info[0, 3]):.2e}, objective {float(info[0, 2]):.4f}")
    # S copies of the reference: one problem per sample, the same mode schedule
    rng = np.random.default_rng(0)
    x0 = np.tile(nb.x0.reshape(1, 15), (S, 1))
    x0[:, :14] += rng.normal(0.0, 1e-3, size=(S, 14)) * np.maximum(np.abs(x0[:, :14]), 0.1)
    nlp = HybridNLP(nb.model, nb.obj, np.full(S, nb.init_mode[0]), np.full(S, nb.k_trans[0]), N, x0,
                    np.tile(nb.xf.reshape(1, 15), (S, 1)))
    Zref = nlp.upload_Z(np.tile(zref, (S, 1)))
    K, _ = nlp.tracking_lqr(Zref, Q, R, Q, with_cost_to_go=False)
    x0d = torch.from_numpy(x0).cuda()
    rows = []
    for name, gains in (("open loop", None), ("closed loop", K)):
        Zo = nlp.tracking_rollout(Zref, gains, x0d)
        c = nlp.eval_c(Zo)
        viol = nlp.constraint_violation(c).cpu().numpy()
        f = nlp.eval_f(Zo).cpu().numpy()
        xN = Zo.view(S, -1)[:, 20 * (N - 1): 20 * (N - 1) + 14].cpu().numpy()
        err = np.linalg.norm(xN - zref[20 * (N - 1): 20 * (N - 1) + 14], axis=1)
        rows.append((name, np.median(err), np.max(err), np.median(viol), np.median(f)))
    print(f"{S} drop states perturbed by 0.1 % (relative, floor 1e-4 absolute)")
    print(f"{'':12s} {'median |x_N - x_ref,N|':>24s} {'max':>10s} {'median violation':>17s} {'median objective':>17s}")
    for name, med, mx, v, f in rows:
        print(f"{name:12s} {med:24.3e} {mx:10.3e} {v:17.3e} {f:17.4f}")
    verdict = "reduces" if rows[1][1] < rows[0][1] else "does not reduce"
    print(f"the closed loop {verdict} the median terminal error")


if __name__ == "__main__":
    main()
