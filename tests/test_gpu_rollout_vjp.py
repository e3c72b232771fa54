"""GPU checks of qln_tracking_rollout_vjp / HybridNLP.differentiable_rollout: the numpy reverse sweep on the evaluator's
own blocks and on complex-step blocks over the tracking shapes and at full size, the adjoint identity against central
differences of the GPU roll-out, torch gradcheck, the anchor 2 P_0 dx_0 of the TVLQR cost-to-go, and the call's contract."""
import numpy as np
import pytest

from tests import rollout_ref as RR
from tests import tracking_cases as TC
from tests.tracking_cases import SHAPES, Q, R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,N,k_trans,init_mode", SHAPES)
@pytest.mark.parametrize("with_gains", [False, True])
def test_matches_numpy_sweep_over_shapes(B, N, k_trans, init_mode, with_gains):
    batch = TC.batch(B, N, k_trans, init_mode, seed=N + k_trans)
    nlp = TC.nlp(batch)
    Zref, K, x0, Zout, Zbar = TC.inputs(nlp, batch, N + 3 * k_trans, with_gains)
    zb, kb, xb = nlp.tracking_rollout_vjp(Zref, Zout, Zbar, K)
    ev = TC.vjp_per_problem(nlp, Zref, K, Zout, Zbar, zb, kb, xb, TC.evaluator_blocks(nlp, Zout))
    cs = TC.vjp_per_problem(nlp, Zref, K, Zout, Zbar, zb, kb, xb, TC.cs_blocks(nlp))
    print(f"B={B} N={N} k_trans={k_trans} mode={init_mode} K={with_gains}: evaluator blocks {ev:.2e}, complex step {cs:.2e}")
    assert ev <= 1e-12 and cs <= 1e-8, (ev, cs)


@pytest.mark.parametrize("with_gains", [False, True])
def test_ragged_batch_and_padded_layout(with_gains):
    for batch, kw in ((TC.batch(37, 12, 5, 1, seed=3, ragged=True), {}),
                      (TC.batch(13, 12, 7, 2, seed=4), {"z_stride": 20 * 12 + 3, "align": 7})):
        nlp = TC.nlp(batch, **kw)
        Zref, K, x0, Zout, Zbar = TC.inputs(nlp, batch, 5, with_gains)
        zb, kb, xb = nlp.tracking_rollout_vjp(Zref, Zout, Zbar, K)
        assert TC.vjp_per_problem(nlp, Zref, K, Zout, Zbar, zb, kb, xb, TC.evaluator_blocks(nlp, Zout)) <= 1e-12


@pytest.mark.parametrize("B,N,ragged", [(65536, 40, False), (65536, 80, True)])
def test_full_size_every_problem(B, N, ragged):
    from quadruped_landing_amd import problem_gen as PG

    full = PG.make_batch(B, N, 14, 1, seed=2, ragged=ragged)
    worst = 0.0
    chunk = 4096
    for s in range(0, B, chunk):
        sub = PG.LandingBatch(full.model, N, full.k_trans[s:s + chunk], full.init_mode[s:s + chunk], full.x0[s:s + chunk],
                              full.xf[s:s + chunk], full.obj if full.obj.ndim == 2 else full.obj[s:s + chunk],
                              full.Z[s:s + chunk])
        nlp = TC.nlp(sub)
        Zref, K, x0, Zout, Zbar = TC.inputs(nlp, sub, s, True)
        zb, kb, xb = nlp.tracking_rollout_vjp(Zref, Zout, Zbar, K)
        dense = TC.dense_blocks(nlp, Zout)
        n = nlp.n_nlp
        f = lambda t: t.view(nlp.B, -1)[:, :n].cpu().numpy()  # noqa: E731
        zr, zo, zbar, zg = f(Zref), f(Zout), f(Zbar), f(zb)
        Kh, kg, xg = K.cpu().numpy(), kb.cpu().numpy(), xb.cpu().numpy()
        # the sweep vectorised over the chunk
        nb = nlp.B
        F = dense.copy()
        kj = nlp.k_trans.astype(int) - 2
        for b in np.nonzero((kj >= 0) & (kj < N - 1))[0]:
            F[b] = RR.evaluator_blocks(dense[b], nlp.k_trans[b])
        lam = zbar[:, 20 * (N - 1): 20 * (N - 1) + 15]
        r_z = np.zeros_like(zg)
        r_k = np.zeros_like(kg)
        for k in range(N - 2, -1, -1):
            ubar = zbar[:, 20 * k + 15: 20 * k + 20] + np.einsum("bij,bi->bj", F[:, k, :, 15:], lam)
            kub = np.einsum("bmj,bm->bj", Kh[:, k], ubar[:, :4])
            r_z[:, 20 * k + 15: 20 * k + 20] = ubar
            r_z[:, 20 * k: 20 * k + 15] = kub
            r_k[:, k] = -ubar[:, :4, None] * (zo[:, 20 * k: 20 * k + 15] - zr[:, 20 * k: 20 * k + 15])[:, None, :]
            lam = zbar[:, 20 * k: 20 * k + 15] + np.einsum("bij,bi->bj", F[:, k, :, :15], lam) - kub
        for got, ref in ((zg, r_z), (kg.reshape(nb, -1), r_k.reshape(nb, -1)), (xg, lam)):
            e = np.linalg.norm(got - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-300)
            worst = max(worst, float(e.max()))
        del nlp
    print(f"full size B={B} N={N} ragged={ragged}: worst per-problem rel err {worst:.2e}")
    assert worst <= 1e-12, worst


def test_adjoint_identity_against_central_differences():
    import torch

    batch = TC.batch(8, 40, 14, 1, seed=21)
    nlp = TC.nlp(batch)
    Zref, K, x0, Zout, Zbar = TC.inputs(nlp, batch, 21, True)
    zb, kb, xb = nlp.tracking_rollout_vjp(Zref, Zout, Zbar, K)
    rng = np.random.default_rng(22)
    n = nlp.n_nlp
    pad = torch.zeros(nlp.B, nlp.z_stride, dtype=torch.float64)
    for _ in range(3):
        dz = pad.clone()
        dz[:, :n] = torch.from_numpy(rng.normal(size=(nlp.B, n)))
        dz = dz.reshape(-1).cuda()
        dk = torch.from_numpy(rng.normal(size=K.shape)).cuda()
        dx = torch.from_numpy(rng.normal(size=(nlp.B, 15))).cuda()
        # scale each direction to a comparable effect
        dz, dk, dx = 1e-3 * dz, 1e-2 * dk, 1e-3 * dx
        eps = 1e-4
        plus = nlp.tracking_rollout(Zref + eps * dz, K + eps * dk, x0 + eps * dx)
        minus = nlp.tracking_rollout(Zref - eps * dz, K - eps * dk, x0 - eps * dx)
        lhs = float(torch.dot((plus - minus).view(-1), Zbar.view(-1))) / (2 * eps)
        rhs = float(torch.dot(dz, zb) + torch.dot(dk.view(-1), kb.view(-1)) + torch.dot(dx.view(-1), xb.view(-1)))
        assert abs(lhs - rhs) <= 1e-6 * abs(rhs), (lhs, rhs)


def test_autograd_gradcheck():
    import torch

    batch = TC.batch(2, 6, 4, 1, seed=31)
    nlp = TC.nlp(batch)
    Zref = nlp.upload_Z(batch.Z).requires_grad_(True)
    K = TC.gains(nlp, 32, scale=0.02).requires_grad_(True)
    x0 = torch.from_numpy(batch.Z[:, :15].copy()).cuda().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda z, k, x: nlp.differentiable_rollout(z, k, x), (Zref, K, x0), eps=1e-6,
                                    atol=1e-7, rtol=1e-6)
    # None inputs and inputs that need no gradient get None
    z2 = Zref.detach().clone().requires_grad_(True)
    out = nlp.differentiable_rollout(z2, None, None)
    out.sum().backward()
    assert z2.grad is not None and torch.isfinite(z2.grad).all()
    k2 = K.detach().clone().requires_grad_(True)
    nlp.differentiable_rollout(Zref.detach(), k2, x0.detach()).pow(2).sum().backward()
    assert k2.grad is not None and k2.grad.shape == K.shape


def test_x0_bar_is_twice_P0_dx0_on_the_tvlqr_closed_loop():
    import torch

    from quadruped_landing_amd import HybridNLP, nlp as NL, problem_gen as PG

    nb = PG.notebook_problem()
    nlp = HybridNLP(nb.model, nb.obj, nb.init_mode, nb.k_trans, nb.N, nb.x0, nb.xf)
    Zs = nlp.upload_Z(nb.Z)
    nlp.solve(Zs)
    K, P = nlp.tracking_lqr(Zs, Q, R, Q)
    P0 = NL.unpack_cost_to_go(P)[0, 0]
    N, n = nlp.N, nlp.n_nlp
    zr = Zs.cpu().numpy()[:n]
    xi = np.array([20 * k + i for k in range(N) for i in range(15)])
    fi = np.array([20 * k + 15 + m for k in range(N - 1) for m in range(4)])
    wx = np.tile(Q, N)
    wf = np.tile(R, N - 1)
    rng = np.random.default_rng(41)
    d = rng.normal(size=15)
    d[14] = 0.0
    d /= np.linalg.norm(d)
    errs = []
    for eps in (1e-3, 1e-4):
        x0 = torch.from_numpy((zr[:15] + eps * d)[None]).cuda()
        zo = nlp.tracking_rollout(Zs, K, x0).cpu().numpy()
        zbar = np.zeros(nlp.z_stride)
        zbar[xi] = 2 * wx * (zo[xi] - zr[xi])
        zbar[fi] = 2 * wf * (zo[fi] - zr[fi])
        _, _, xb = nlp.tracking_rollout_vjp(Zs, torch.from_numpy(zo).cuda(), torch.from_numpy(zbar).cuda(), K)
        ref = 2 * P0 @ (eps * d)
        errs.append(np.linalg.norm(xb.cpu().numpy()[0] - ref) / np.linalg.norm(ref))
    ratio = errs[0] / errs[1]
    print(f"anchor: rel err {errs[0]:.2e} (eps 1e-3), {errs[1]:.2e} (eps 1e-4), ratio {ratio:.1f}")
    assert errs[1] < 1e-2 and 5.0 <= ratio <= 20.0, (errs, ratio)


@pytest.mark.parametrize("B", [5, 1024])  # mapped pinned buffers (small batch) and staged device copies
def test_contract_sentinels_linearity_refusal_and_host_forms(B):
    import torch

    from quadruped_landing_amd import _lib

    N = 12
    batch = TC.batch(B, N, 5, 2, seed=51)
    nlp = TC.nlp(batch, z_stride=20 * N + 3)
    Zref, K, x0, Zout, Zbar = TC.inputs(nlp, batch, 51, True)
    zb, kb, xb = nlp.tracking_rollout_vjp(Zref, Zout, Zbar, K)
    L = _lib.lib()
    n, zs = nlp.n_nlp, nlp.z_stride
    # sentinels: slots past n_nlp untouched; each output alone (the others NULL) equals the all-outputs call bit for bit
    for which in range(3):
        s_z = torch.full((B * zs,), 7.0, dtype=torch.float64, device="cuda")
        s_k = torch.full(K.shape, 7.0, dtype=torch.float64, device="cuda")
        s_x = torch.full((B, 15), 7.0, dtype=torch.float64, device="cuda")
        outs = [s_z, s_k, s_x]
        ptrs = [o.data_ptr() if i == which else None for i, o in enumerate(outs)]
        _lib.check(L.qln_tracking_rollout_vjp(nlp._h, Zref.data_ptr(), K.data_ptr(), Zout.data_ptr(), Zbar.data_ptr(), *ptrs))
        torch.cuda.synchronize()
        for i, (o, ref) in enumerate(zip(outs, (zb, kb, xb))):
            if i != which:
                assert (o == 7.0).all()
            elif i == 0:
                v = o.view(B, zs)
                assert (v[:, n:] == 7.0).all() and torch.equal(v[:, :n], zb.view(B, zs)[:, :n])
            else:
                assert torch.equal(o, ref)
    # linearity in Zbar
    Zbar2 = nlp.upload_Z(np.random.default_rng(52).normal(size=(B, n)))
    z2, k2, x2 = nlp.tracking_rollout_vjp(Zref, Zout, Zbar2, K)
    z3, k3, x3 = nlp.tracking_rollout_vjp(Zref, Zout, 2.0 * Zbar - 3.0 * Zbar2, K)
    for a, b_, c in ((zb, z2, z3), (kb, k2, k3), (xb, x2, x3)):
        ref = 2.0 * a - 3.0 * b_
        assert float((c - ref).norm() / ref.norm()) <= 1e-13
    # K == NULL with K_bar is refused; NULL K gives zero x_ref slots
    with pytest.raises(_lib.QlnError):
        nlp.tracking_rollout_vjp(Zref, Zout, Zbar, None, want=("K",))
    with pytest.raises(_lib.QlnError):
        nlp.tracking_rollout_vjp_host(Zref.cpu().numpy(), Zout.cpu().numpy(), Zbar.cpu().numpy(), None, want=("K",))
    with pytest.raises(_lib.QlnError):  # an output that overlaps an input
        _lib.check(L.qln_tracking_rollout_vjp(nlp._h, Zref.data_ptr(), K.data_ptr(), Zout.data_ptr(), Zbar.data_ptr(),
                                              Zbar.data_ptr(), None, None))
    z0, k0, _ = nlp.tracking_rollout_vjp(Zref, Zout, Zbar)
    assert k0 is None
    xs = np.array([20 * k + i for k in range(N) for i in range(15)])
    assert (z0.view(B, zs)[:, xs] == 0.0).all()
    # host forms equal the device forms bit for bit (twice: the second call reuses the handle's buffers)
    h = [t.cpu().numpy() for t in (Zref, K, Zout, Zbar)]
    for _ in range(2):
        hz, hk, hx = nlp.tracking_rollout_vjp_host(h[0], h[2], h[3], h[1])
        assert np.array_equal(hz, zb.cpu().numpy()) and np.array_equal(hk, kb.cpu().numpy())
        assert np.array_equal(hx, xb.cpu().numpy())
    hz0, hk0, hx0 = nlp.tracking_rollout_vjp_host(h[0], h[2], h[3])
    assert hk0 is None and np.array_equal(hz0, z0.cpu().numpy())
