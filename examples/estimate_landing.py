"""What do the landing margins cost when the controller has to estimate the state?  The 1 024 drops of
examples/touchdown_timing.py -- the notebook's problem (N = 61, k_trans = 21) solved with qln_solve, the free foot up to 2 cm
higher or lower than planned, the feet up to 10 % lighter or heavier -- rolled out with the guarded touchdown under
time-indexed TVLQR gains.  Along every drop's own trajectory a 0.1 % drop-state covariance is propagated through the touchdown
twice: under state feedback (qln_tracking_covariance_guarded: the controller reads the true state) and under estimate feedback
(qln_tracking_kalman_guarded: it reads a Kalman filter's estimate), with eight sensor rows -- body pose x[0..2], gyro x[9], and
the two feet relative to the body -- at two noise levels.  Prints the clearance margin, the vertical-force margin and the
touchdown clock's standard deviation, in standard deviations of the linear-Gaussian prediction.
   python examples/estimate_landing.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from quadruped_landing_amd import HybridNLP, problem_gen as PG  # noqa: E402

S = 1024
Q = np.array([10.0] * 14 + [0.0])
R = np.array([1e-3, 1e-2, 1e-3, 1e-2])
HEIGHT, FOOT_MASS = 0.02, 0.10  # +- 2 cm of free-foot start height, +- 10 % of foot mass
W = np.array([1e-10] * 14 + [0.0])  # process noise per step; the clock is known
NOISE = (1e-3, 1e-2)  # sensor standard deviations [m, rad, rad/s]


def sensors():
    """Eight rows: body pose x[0..2], gyro x[9], feet relative to the body x[3]-x[0], x[4]-x[1], x[5]-x[0], x[6]-x[1]."""
    H = np.zeros((8, 15))
    for r, i in enumerate((0, 1, 2, 9)):
        H[r, i] = 1.0
    for r, (foot, body) in enumerate(((3, 0), (4, 1), (5, 0), (6, 1)), start=4):
        H[r, foot], H[r, body] = 1.0, -1.0
    return H


def margins(z, marg, var, lb, N):
    """(clearance margin, F_y margin, touchdown-clock sd) per drop from the marginals of a sweep"""
    knots = 20 * np.arange(N)
    clearance = z[:, knots + 1] - lb / 2 * np.abs(np.sin(z[:, knots + 2]))
    with np.errstate(divide="ignore", invalid="ignore"):
        m_clear = np.where(marg[:, :, 0] > 0, clearance / np.sqrt(marg[:, :, 0]), np.inf).min(axis=1)
        fy = np.stack([z[:, knots[:-1] + 16], z[:, knots[:-1] + 18]], axis=-1)
        sd_fy = np.sqrt(marg[:, :-1, [2, 4]])
        m_force = np.where(sd_fy > 0, np.abs(fy) / sd_fy, np.inf).min(axis=(1, 2))
    return m_clear, m_force, np.sqrt(var[:, 1])


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
    model = nlp.plant_models()
    model[:, 2] *= torch.from_numpy(1.0 + rng.uniform(-FOOT_MASS, FOOT_MASS, size=S)).cuda()
    Zref = nlp.upload_Z(np.tile(zref, (S, 1)))
    K, _ = nlp.tracking_lqr(Zref, Q, R, Q, with_cost_to_go=False)
    Zg, events = nlp.tracking_rollout_guarded(Zref, K, torch.from_numpy(x0).cuda(), model)
    landed = (events[:, 0] >= 0).cpu().numpy()
    print(f"{S} drops, {int(landed.sum())} land within the horizon")

    sd0 = 1e-3 * np.maximum(np.abs(x0), 0.1)  # 0.1 % of each drop-state entry (floor 1e-4 absolute); the clock is known
    sd0[:, 14] = 0.0
    S0 = np.zeros((S, 120))
    S0[:, [i * (i + 3) // 2 for i in range(15)]] = sd0 * sd0
    z = Zg.view(S, -1)[:, :n].cpu().numpy()
    lb = nb.model.lb

    rows = []
    _, mg, var = nlp.tracking_covariance_guarded(Zg, events, K, S0, W, model, with_sigma=False)
    rows.append(("state feedback", margins(z, mg.cpu().numpy(), var.cpu().numpy(), lb, N)))
    H = sensors()
    for sd in NOISE:
        _, Pest, _, mg, var = nlp.tracking_kalman_guarded(Zg, events, H, sd * sd, K, S0, W, model, with_gains=False)
        rows.append((f"estimate feedback, sensor sd {sd:.0e}", margins(z, mg.cpu().numpy(), var.cpu().numpy(), lb, N)))
    torch.cuda.synchronize()
    print(f"{'':36s} {'clearance margin [sd]':>24s} {'F_y margin [sd]':>24s} {'touchdown clock sd [s]':>26s}")
    print(f"{'':36s} {'min':>11s} {'median':>12s} {'min':>11s} {'median':>12s} {'median':>13s} {'max':>12s}")
    for name, (mc, mf, ck) in rows:
        ck = ck[landed]
        print(f"{name:36s} {mc.min():11.2f} {np.median(mc):12.2f} {mf.min():11.2f} {np.median(mf):12.2f} "
              f"{np.median(ck):13.3e} {ck.max():12.3e}")
    tr = Pest.cpu().numpy()[:, :, [i * (i + 3) // 2 for i in range(15)]].sum(axis=2)
    print(f"estimate feedback, sensor sd {NOISE[-1]:.0e}: trace of the error covariance P+ at knot 0 / {N - 1}, median over the "
          f"drops: {np.median(tr[:, 0]):.3e} / {np.median(tr[:, -1]):.3e}")


if __name__ == "__main__":
    main()
