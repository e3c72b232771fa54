"""Which robot made this landing -- from its sensors alone?  The 1 024 guarded drops of examples/fly_estimated_landing.py (the
notebook's problem solved with qln_solve, the free foot up to 2 cm higher or lower than planned, a drop state drawn from the
0.1 % covariance) are flown with estimate feedback by PLANTS whose body and foot masses are off by up to 10 % per drop, under
sensor noise of 1e-3.  Of each flight only the RECORD is kept: the eight sensor readings per knot and the forces that were
applied.  The two masses of each record are then recovered by maximising the record's log-likelihood under the filter
(qln_landing_filter_guarded_model) with the filter's new derivatives only: per outer iteration the Kalman gains are redesigned at
the current masses (qln_tracking_kalman_guarded), the filter is run on the record, and one Gauss-Newton step is taken per
record on the tangents of the innovations in the two mass directions (qln_landing_filter_guarded_jvp, two launches for the whole
batch), whose loglik_dot is the exact gradient at fixed gains and whose innov_dot gives the Gauss-Newton matrix
sum_k J_k' S_k^-1 J_k with S_k^-1 = V^-1 (I - H L_k).  Printed: the relative mass errors before and after, and beside them those
of examples/identify_model.py's fit on the same drops and the same drawn masses with FULL noise-free state trajectories.
   python examples/identify_model_from_sensors.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from estimate_landing import HEIGHT, NOISE, Q, R, S, W, sensors  # noqa: E402
from identify_model import gauss_newton  # noqa: E402
from quadruped_landing_amd import HybridNLP, problem_gen as PG  # noqa: E402

MASS = 0.10  # body and foot mass off by up to this share, per drop
OUTER = 6


def quantiles(err):
    return " ".join(f"{v:10.2e}" for v in np.quantile(err, [0.5, 0.9, 0.99, 1.0]))


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
    nominal = nlp.plant_models()
    truth = nominal.clone()
    truth[:, 1:3] *= torch.from_numpy(1.0 + MASS * rng.uniform(-1.0, 1.0, size=(S, 2))).cuda()
    Zref = nlp.upload_Z(np.tile(zref, (S, 1)))
    K, _ = nlp.tracking_lqr(Zref, Q, R, Q, with_cost_to_go=False)
    X0 = torch.from_numpy(x0).cuda()
    sd0 = 1e-3 * np.maximum(np.abs(x0), 0.1)
    sd0[:, 14] = 0.0
    S0 = np.zeros((S, 120))
    S0[:, [i * (i + 3) // 2 for i in range(15)]] = sd0 * sd0
    H, sd = sensors(), NOISE[0]
    V = np.full(H.shape[0], sd * sd)
    gen = torch.Generator(device="cuda").manual_seed(0)
    randn = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=gen)  # noqa: E731

    def gains(th):
        """the Kalman gains along the drop's nominal at the masses th"""
        Zg, events = nlp.tracking_rollout_guarded(Zref, K, X0, th)
        return nlp.tracking_kalman_guarded(Zg, events, H, V, K, S0, W, th, with_pest=False, with_sigma=False, with_marginals=False,
                                           with_event_var=False)[0]

    # the flights: each drop's plant has its own masses; the estimator in the loop knows the handle's only
    Zg, _ = nlp.tracking_rollout_guarded(Zref, K, X0, None)
    xs = X0 + randn(S, 15) * torch.from_numpy(sd0).cuda()
    v, w = sd * randn(S, N, 8), randn(S, N - 1, 15) * torch.from_numpy(np.sqrt(W)).cuda()
    Zo, _, _, _, _ = nlp.tracking_rollout_estimated(Zg, K, gains(nominal), H, v, w, xs, None, truth, guarded=True)
    # the record: the readings (less H x_ref, the reference being the drop's nominal) and the applied forces, nothing else
    Y = nlp.landing_measurements(Zo, Zg, H, v)
    ctrl = (20 * torch.arange(N - 1, device="cuda")[:, None] + 15 + torch.arange(5, device="cuda")[None, :]).reshape(-1)
    Zrec = torch.zeros_like(Zo)
    Zrec.view(S, -1)[:, ctrl] = Zo.view(S, -1)[:, ctrl]
    del Zo, xs, w

    Ht, iV = torch.from_numpy(H).cuda(), torch.from_numpy(1.0 / V).cuda()
    eye = torch.eye(H.shape[0], dtype=torch.float64, device="cuda")
    th, scale = nominal.clone(), nominal.abs()
    err = lambda t: np.abs((t[:, 1:3] / truth[:, 1:3]).cpu().numpy() - 1.0)  # noqa: E731
    before = err(th)
    print(f"{S} records of {N} knots x {H.shape[0]} sensors at sd {sd:.0e}; body and foot mass off by up to {100 * MASS:.0f} %")
    print(f"  {'outer':>5s} {'median loglik':>14s} {'median |mb err|':>16s} {'median |mf err|':>16s}")
    for it in range(OUTER + 1):
        L = gains(th)  # redesigned at the current masses: the sweeps differentiate at fixed gains
        Xhat, innov, _, loglik, eh = nlp.landing_filter_guarded(Zg, Zrec, L, H, Y, V, None, model=th)
        e = err(th)
        print(f"  {it:5d} {float(loglik.median()):14.2f} {np.median(e[:, 0]):16.3e} {np.median(e[:, 1]):16.3e}")
        if it == OUTER:
            break
        J, g = [], []
        for p in (1, 2):
            d = torch.zeros_like(th)
            d[:, p] = scale[:, p]
            t = nlp.landing_filter_jvp(Zg, Zrec, L, H, Xhat, innov, V, th, eh, True, model_dot=d, want=("innov", "loglik"))
            J.append(t["innov"])
            g.append(t["loglik"])
        J, g = torch.stack(J, dim=-1), torch.stack(g, dim=-1)  # (S, N, ny, 2), (S, 2)
        G = iV[:, None] * (eye - torch.einsum("ri,snij->snrj", Ht, L))  # S_k^-1 = V^-1 (I - H L_k)
        G = 0.5 * (G + G.transpose(-1, -2))
        A = torch.einsum("snrp,snrc,sncq->spq", J, G, J)
        step = torch.linalg.solve(A, g[:, :, None])[:, :, 0]
        th = th.clone()
        th[:, 1:3] += scale[:, 1:3] * step
    after = err(th)
    # the same drops and the same drawn masses with full states: examples/identify_model.py's fit of noise-free trajectories
    target = nlp.tracking_rollout_model(Zref, K, X0, truth)
    full = err(gauss_newton(nlp, Zref, K, X0, target, nominal))
    torch.cuda.synchronize()
    print(f"  relative mass error {'':24s} {'median':>10s} {'90 %':>10s} {'99 %':>10s} {'max':>10s}")
    for i, name in enumerate(("mb", "mf")):
        print(f"  {name}: before (the handle's model)        {quantiles(before[:, i])}")
        print(f"  {name}: from sensor records, {OUTER} outer its  {quantiles(after[:, i])}")
        print(f"  {name}: from full noise-free states       {quantiles(full[:, i])}")


if __name__ == "__main__":
    main()
