"""How much drop-state error can each landing take?  Solve 1 024 random landings (N = 40) with qln_solve, compute TVLQR
gains, propagate a 0.1 % drop-state covariance through every closed loop in one qln_tracking_covariance launch, and print
per landing the smallest clearance margin and the smallest vertical-force margin over the knots, in standard deviations.
Then compare one landing's Sigma_N with the sample covariance of 1 024 perturbed roll-outs of that landing.
   python examples/landing_uncertainty.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from quadruped_landing_amd import HybridNLP, nlp as NL, problem_gen as PG  # noqa: E402

B = S = 1024
N = 40
Q = np.array([10.0] * 14 + [0.0])
R = np.array([1e-3, 1e-2, 1e-3, 1e-2])


def drop_state_variances(x0):
    """0.1 % of each drop-state entry (floor 1e-4 absolute); the clock is known."""
    sd = 1e-3 * np.maximum(np.abs(x0), 0.1)
    sd[:, 14] = 0.0
    return sd * sd


def main():
    batch = PG.make_batch(B, N, 14, 1, seed=0)
    nlp = HybridNLP(batch.model, batch.obj, batch.init_mode, batch.k_trans, N, batch.x0, batch.xf)
    Zs = nlp.upload_Z(batch.Z)
    _, info = nlp.solve(Zs)
    print(f"solved {int((info[:, 5] == 0).sum())} of {B} landings")
    K, _ = nlp.tracking_lqr(Zs, Q, R, Q, with_cost_to_go=False)
    var0 = drop_state_variances(batch.x0)
    S0 = np.zeros((B, 120))
    S0[:, [i * (i + 3) // 2 for i in range(15)]] = var0  # the diagonal of the packed lower triangle
    Sigma, marg = nlp.tracking_covariance(Zs, K, S0)
    torch.cuda.synchronize()
    z = Zs.view(B, -1)[:, : nlp.n_nlp].cpu().numpy()
    mg = marg.cpu().numpy()
    knots = 20 * np.arange(N)
    clearance = z[:, knots + 1] - batch.model.lb / 2 * np.abs(np.sin(z[:, knots + 2]))
    with np.errstate(divide="ignore", invalid="ignore"):
        m_clear = np.where(mg[:, :, 0] > 0, clearance / np.sqrt(mg[:, :, 0]), np.inf).min(axis=1)
        fy = np.stack([z[:, knots[:-1] + 16], z[:, knots[:-1] + 18]], axis=-1)  # F1y, F2y of every dynamics knot
        sd_fy = np.sqrt(mg[:, :-1, [2, 4]])
        m_force = np.where(sd_fy > 0, np.abs(fy) / sd_fy, np.inf).min(axis=(1, 2))
    print(f"{'landing':>8s} {'min clearance margin [sd]':>27s} {'min F_y margin [sd]':>21s}")
    for b in range(B):
        print(f"{b:8d} {m_clear[b]:27.2f} {m_force[b]:21.2f}")
    print(f"over the batch: clearance margin min {m_clear.min():.2f} / median {np.median(m_clear):.2f} sd, "
          f"F_y margin min {m_force.min():.2f} / median {np.median(m_force):.2f} sd")

    # one landing against the sample covariance of S perturbed roll-outs of it
    b = 0
    rep = lambda a: np.repeat(np.asarray(a)[b:b + 1], S, axis=0)  # noqa: E731
    many = HybridNLP(batch.model, batch.obj if batch.obj.ndim == 2 else batch.obj[b], rep(batch.init_mode), rep(batch.k_trans),
                     N, rep(batch.x0), rep(batch.xf))
    rng = np.random.default_rng(1)
    x0 = z[b, :15] + rng.normal(size=(S, 15)) * np.sqrt(var0[b])
    Zo = many.tracking_rollout(many.upload_Z(np.tile(z[b], (S, 1))), K[b:b + 1].expand(S, -1, -1, -1).contiguous(),
                               torch.from_numpy(x0).cuda())
    xN = Zo.view(S, -1)[:, 20 * (N - 1): 20 * (N - 1) + 15].cpu().numpy()
    SN = NL.unpack_covariance(Sigma)[b, -1]
    CN = np.cov(xN, rowvar=False)
    sd_lin, sd_mc = np.sqrt(np.diag(SN)), np.sqrt(np.diag(CN))
    print(f"landing {b}: terminal standard deviations, propagated against {S} roll-outs")
    for i in range(14):
        print(f"  x[{i:2d}]  {sd_lin[i]:10.3e}  {sd_mc[i]:10.3e}")
    print(f"  |Sigma_N - sample covariance| / |Sigma_N| = {np.linalg.norm(SN - CN) / np.linalg.norm(SN):.3f} "
          f"(sampling error of {S} draws: ~{np.sqrt(2.0 / (S - 1)):.3f} per variance)")


if __name__ == "__main__":
    main()
