"""Every family of the launch plan (csrc/qln_launch_plan.h) once on the GPU at its smallest shape, against the oracle with the
tolerance of tests/test_gpu_parity.py: the device-pointer entry points at the horizons where the plan changes shape (17 | 18
the split's limit, 41 | 42 and 65 | 66 the chunk rule, 65 | 66 the dense prefetch, 82 the third 40-knot chunk), both formats,
and the host-pointer forms that ask for one workgroup per chunk -- granted for B = 1, 2, refused for B = 257.

The oracle writes dense blocks; a structural handle's values are compared with the oracle's entries at the (row, col)
positions its own qln_jacobian_structure lists."""
import numpy as np
import pytest

from tests.helpers import oracle_batch, rel_err
from tests.test_gpu_parity import RTOL

pytestmark = pytest.mark.gpu

FORMATS = ("dense_blocks", "structural")


class _Case:
    """a ragged batch, a handle in the format under test and the oracle's results (in the layout of a dense-block handle)"""

    def __init__(self, B, N, fmt):
        from quadruped_landing_amd import HybridNLP, problem_gen as PG

        self.batch = b = PG.make_batch(B, N, seed=100 * B + N, ragged=True)
        mk = lambda f: HybridNLP(b.model, b.obj, b.init_mode, b.k_trans, b.N, b.x0, b.xf, jac_format=f)
        self.dense = mk("dense_blocks")
        self.nlp = self.dense if fmt == "dense_blocks" else mk(fmt)
        self.ref = oracle_batch(b, self.dense, want_f=True, want_grad=True)
        self.B, self.n = B, self.nlp.n_nlp

    def vals_ref(self, b):
        want = self.dense.split_vals(self.ref["vals"], b)
        if self.nlp is self.dense:
            return want
        rd, cd = self.dense.jacobian_structure(b)
        rs, cs = self.nlp.jacobian_structure(b)
        kd, ks = rd.astype(np.int64) * self.n + cd, rs.astype(np.int64) * self.n + cs
        order = np.argsort(kd, kind="stable")
        at = np.searchsorted(kd[order], ks)
        assert np.array_equal(kd[order][at], ks)  # every structural position is one of the dense blocks' positions
        return want[order[at]]

    def check(self, c=None, vals=None, f=None, grad=None):
        close = lambda got, want, floor: rel_err(got, want, floor=floor) <= RTOL and not np.isnan(np.asarray(got)).any()
        for b in range(self.B):
            if c is not None:
                assert close(self.nlp.split_c(c, b), self.nlp.split_c(self.ref["c"], b), 1.0), ("c", b)
            if vals is not None:
                assert close(self.nlp.split_vals(vals, b), self.vals_ref(b), 1e-300), ("vals", b)
        if f is not None:
            assert close(f, self.ref["f"], 0.0), "f"
        if grad is not None:
            assert close(np.asarray(grad).reshape(self.B, -1)[:, : self.n], self.ref["grad"].reshape(self.B, -1)[:, : self.n], 1e-300), "grad"


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("N", [17, 18, 41, 42, 65, 66, 82])
def test_device_pointer_entry_points(N, fmt):
    import torch

    B = 3
    case = _Case(B, N, fmt)
    nlp = case.nlp
    Z = nlp.upload_Z(case.batch.Z)
    mk = lambda n: torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    zt, ct, jt = nlp.dims.z_total, nlp.dims.c_total, nlp.dims.j_total
    c0, v0 = nlp.eval_c_and_jac(Z, mk(ct), mk(jt))
    c1 = nlp.eval_c(Z, mk(ct))
    v1 = nlp.jac_c(Z, mk(jt))
    f2, g2, c2, v2 = nlp.eval_all(Z, mk(B), mk(zt), mk(ct), mk(jt))
    f3, c3 = nlp.eval_f_and_c(Z, mk(B), mk(ct))
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy()
    case.check(c=host(c0), vals=host(v0))
    case.check(c=host(c1), vals=host(v1))
    case.check(c=host(c2), vals=host(v2), f=host(f2), grad=host(g2))
    case.check(c=host(c3), f=host(f3))
    # what no problem owns stays as it was found
    assert np.array_equal(np.isnan(host(c0)), np.isnan(case.ref["c"])) and np.array_equal(np.isnan(host(c0)), np.isnan(host(c3)))
    assert np.array_equal(np.isnan(host(v0)), np.isnan(host(v1))) and np.array_equal(np.isnan(host(v0)), np.isnan(host(v2)))


@pytest.mark.parametrize("B,fmt", [(1, "dense_blocks"), (1, "structural"), (2, "dense_blocks"), (2, "structural"), (257, "structural")])
def test_host_pointer_forms(B, fmt):
    """N = 18: B = 1, 2 run one workgroup per 16-knot chunk (eval_c_host on a structural handle through the dense kernel);
    B = 257 (structural: about 5.4 MB, still mapped host memory) asks for it and is refused."""
    case = _Case(B, 18, fmt)
    nlp, Z = case.nlp, case.batch.Z
    assert 8 * (nlp.dims.z_total + nlp.dims.c_total + nlp.dims.j_total) <= 8 << 20  # mapped, so the split is asked for
    case.check(c=nlp.eval_c_host(Z), vals=nlp.jac_c_host(Z), f=nlp.eval_f_host(Z), grad=nlp.grad_f_host(Z))
