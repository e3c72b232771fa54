"""How optimal are the landings qln_solve returns?  Solve a batch of random N = 40 landings on the GPU (status 0 says
"feasible to tol_violation" and nothing more), estimate the Lagrange multipliers of every one by least squares over its
active set (qln_estimate_multipliers), and print what the KKT report says: the dual infeasibility max |grad f + J'lam|
over the free columns relative to max(1, max |grad f|), the CGLS iterations it took, and how many multipliers came out
with the wrong sign (clearance rows with lam > 0, bound multipliers against their bound).

    python examples/certify_landings.py [B]
    python examples/certify_landings.py --notebook [trajectory.csv]

The second form does the same for the notebook problem (N = 61, k_trans = 21) solved from its initial guess and, given a
trajectory in the reference's file format (one float per line, e.g. the reference's own data_6.csv), for that point too.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quadruped_landing_amd import HybridNLP, problem_gen as PG  # noqa: E402
from quadruped_landing_amd.trajectory_io import load_trajectory  # noqa: E402

QUANTILES = (0.0, 0.25, 0.5, 0.75, 0.95, 1.0)


def certify(B=1024, N=40, k_trans=14, seed=1, **estimate_options):
    """Returns (solve info (B, 16), multiplier info (B, 16)) as numpy arrays."""
    batch = PG.make_batch(B, N, k_trans, 1, seed=seed, noise=0.0)
    nlp = HybridNLP(batch.model, batch.obj, batch.init_mode, batch.k_trans, batch.N, batch.x0, batch.xf)
    Z, sinfo = nlp.solve(nlp.initial_guess())
    lam, lag, info = nlp.estimate_multipliers(Z, **estimate_options)
    torch.cuda.synchronize()
    return sinfo.cpu().numpy(), info.cpu().numpy()


def report(sinfo, info):
    rel = info[:, 4] / np.maximum(1.0, info[:, 11])
    rows = (("dual infeasibility / max(1, |g|)", rel, "{:10.3e}"), ("CGLS iterations", info[:, 0], "{:10.0f}"),
            ("clearance rows with lam > 0", info[:, 7], "{:10.0f}"), ("bound multipliers of the wrong sign", info[:, 8], "{:10.0f}"),
            ("active clearance rows", info[:, 5], "{:10.0f}"), ("fixed variables", info[:, 6], "{:10.0f}"))
    lines = [f"{info.shape[0]} landings, {int((sinfo[:, 5] == 0).sum())} with status 0; max violation {sinfo[:, 3].max():.2e}",
             f"{'quantile':36s}" + "".join(f"{q:10.2f}" for q in QUANTILES)]
    for name, v, fmt in rows:
        lines.append(f"{name:36s}" + "".join(fmt.format(x) for x in np.quantile(v, QUANTILES)))
    lines.append(f"landings with a wrong-sign clearance multiplier: {int((info[:, 7] > 0).sum())}, "
                 f"with a wrong-sign bound multiplier: {int((info[:, 8] > 0).sum())}")
    return "\n".join(lines)


def certify_notebook(trajectory=None, **estimate_options):
    """[(label, info row)] for the notebook problem solved on the GPU and, if given, for the trajectory file's point."""
    nb = PG.notebook_problem()
    nlp = HybridNLP(nb.model, nb.obj, nb.init_mode, nb.k_trans, nb.N, nb.x0, nb.xf)
    Z, _ = nlp.solve(nlp.initial_guess())
    points = [("qln_solve from the notebook's initial guess", Z)]
    if trajectory is not None:
        points.append((trajectory, nlp.upload_Z(load_trajectory(trajectory, nb.N)[None, :])))
    out = []
    for label, Zp in points:
        viol = float(nlp.constraint_violation(nlp.eval_c(Zp))[0])
        _, _, info = nlp.estimate_multipliers(Zp, **estimate_options)
        torch.cuda.synchronize()
        out.append((label, viol, info.cpu().numpy()[0]))
    return out


def report_notebook(rows):
    lines = []
    for label, viol, i in rows:
        lines.append(f"{label}: violation {viol:.3e}; dual infeasibility max |grad f + J'lam| = {i[4]:.3e} over the free "
                     f"variables (max |grad f| there {i[11]:.3e}), {i[0]:.0f} CGLS iterations; {i[5]:.0f} active clearance "
                     f"rows, {i[6]:.0f} fixed variables; wrong signs: {i[7]:.0f} clearance, {i[8]:.0f} bound; "
                     f"max |lam_i c_i| {i[9]:.3e}, max |lam| {i[10]:.3e}")
    return "\n".join(lines)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--notebook":
        print(report_notebook(certify_notebook(sys.argv[2] if len(sys.argv) > 2 else None)))
    else:
        print(report(*certify(int(sys.argv[1]) if len(sys.argv) > 1 else 1024)))
