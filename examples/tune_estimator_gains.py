"""Tune the feedback gains K and the filter gains L on sampled landings of plants the design does not know.  The 1 024 drops and
the sensors of examples/fly_estimated_landing.py, with the feet up to 10 % lighter or heavier than the filter's model: there
the flown deviations reach several predicted standard deviations, because the Riccati and the Kalman design are optimal only
for the linearised, correctly modelled loop.  Here Adam descends on K and L through HybridNLP.differentiable_estimated_rollout
-- qln_tracking_rollout_estimated_guarded forward, qln_tracking_rollout_estimated_guarded_vjp backward -- over one FIXED set of
noise samples (drop-state errors, sensor noise, process noise): the pathwise gradient at fixed samples and fixed touchdown
knots.  The loss is the mean over the drops of the squared terminal deviation from the drop's nominal plus the squared
estimation error summed over the knots, each state weighted alike.  It prints the loss before and after, on the training
samples and on a held-out set of samples drawn afterwards.
   python examples/tune_estimator_gains.py [steps]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from estimate_landing import FOOT_MASS, HEIGHT, NOISE, Q, R, S, W, sensors  # noqa: E402
from quadruped_landing_amd import HybridNLP, problem_gen as PG  # noqa: E402

STEPS = 100
LR = 1e-2  # Adam's step, relative: in units of each gain array's mean magnitude


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else STEPS
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
    model[:, 2] *= torch.from_numpy(1.0 + rng.uniform(-FOOT_MASS, FOOT_MASS, size=S)).cuda()  # the feet the filter does not know
    Zref = nlp.upload_Z(np.tile(zref, (S, 1)))
    K0, _ = nlp.tracking_lqr(Zref, Q, R, Q, with_cost_to_go=False)
    sd0 = 1e-3 * np.maximum(np.abs(x0), 0.1)
    sd0[:, 14] = 0.0
    S0 = np.zeros((S, 120))
    S0[:, [i * (i + 3) // 2 for i in range(15)]] = sd0 * sd0
    H, sd = sensors(), NOISE[0]
    x0d, sd0d = torch.from_numpy(x0).cuda(), torch.from_numpy(sd0).cuda()
    # the drops' nominals and the designed filter, as examples/fly_estimated_landing.py: the design sees the handle's feet
    Zg, events = nlp.tracking_rollout_guarded(Zref, K0, x0d, model)
    L0, *_ = nlp.tracking_kalman_guarded(Zg, events, H, sd * sd, K0, S0, W, model, with_pest=False, with_sigma=False)
    nominal = Zg.view(S, -1)[:, :n]

    gen = torch.Generator(device="cuda").manual_seed(0)
    randn = lambda *s: torch.randn(*s, dtype=torch.float64, device="cuda", generator=gen)  # noqa: E731
    draw = lambda: (x0d + randn(S, 15) * sd0d, sd * randn(S, N, 8),  # noqa: E731
                    randn(S, N - 1, 15) * torch.from_numpy(np.sqrt(W)).cuda())
    train, held_out = draw(), draw()

    def loss_of(K, L, samples):
        xs, v, w = samples
        Zo, Xhat, _, evp, evh = nlp.differentiable_estimated_rollout(Zg, K, L, H, v, w, xs, None, model, guarded=True)
        z = torch.cat([Zo.view(S, -1)[:, :n], Zo.new_zeros((S, 5))], dim=1).view(S, N, 20)[:, :, :14]
        terminal = ((z[:, -1] - nominal[:, n - 15: n - 1]) ** 2).sum(dim=1).mean()
        estimate = ((z - Xhat[:, :, :14]) ** 2).sum(dim=(1, 2)).mean()
        return terminal + estimate, float(terminal.detach()), float(estimate.detach()), evp, evh

    def report(tag, K, L):
        for name, smp in (("training", train), ("held-out", held_out)):
            with torch.no_grad():
                total, t, e, evp, evh = loss_of(K, L, smp)
            print(f"{tag:7s} {name:9s} loss {float(total):.6e} = terminal {t:.6e} + estimation {e:.6e}; "
                  f"{int((evp[:, 0] != events[:, 0]).sum())} plants and {int((evh[:, 0] != evp[:, 0]).sum())} estimators in another knot")

    scale = lambda t: float(t.abs().mean())  # noqa: E731
    print(f"{S} drops, feet +-{100 * FOOT_MASS:.0f} %, sensor sd {sd:.0e}; Adam, {steps} steps of {LR:g} of each array's mean "
          f"magnitude on K ({K0.numel()} entries, mean |K| {scale(K0):.3e}) and L ({L0.numel()} entries, mean |L| {scale(L0):.3e})")
    report("before", K0, L0)
    K, L = K0.clone().requires_grad_(True), L0.clone().requires_grad_(True)
    opt = torch.optim.Adam([{"params": [K], "lr": LR * scale(K0)}, {"params": [L], "lr": LR * scale(L0)}])
    for step in range(steps):
        opt.zero_grad()
        total, t, e, _, _ = loss_of(K, L, train)
        total.backward()
        if step % 20 == 0:
            print(f"  step {step:3d}: training loss {float(total.detach()):.6e}; |grad K| {float(K.grad.norm()):.3e}, |grad L| "
                  f"{float(L.grad.norm()):.3e}")
        opt.step()
    report("after", K.detach(), L.detach())
    torch.cuda.synchronize()
    print("the gradient is the pathwise one at fixed samples and fixed touchdown knots: a drop that changes its knot during the "
          "descent is outside what it says")


if __name__ == "__main__":
    main()
