"""Host side of the boundary (no GPU): index maps, bounds, packZ/unpackZ, cost/reference-trajectory setup
and the synthetic generator, each against the oracle's restatement of the same reference code."""
import numpy as np
import pytest

import quadruped_landing_amd as Q
from quadruped_landing_amd import nlp as NLP
from quadruped_landing_amd import problem_gen as PG
from oracle import oracle as O


@pytest.mark.parametrize("N,kt", [(61, 21), (40, 14), (2, 2), (80, 79), (80, 2), (12, 13), (12, 1)])
def test_index_maps_match_oracle(N, kt):
    o = O.OracleNLP(N, kt, 1, np.zeros(15), np.zeros(15), np.zeros((N, 41)))
    assert NLP.num_primals(N) == o.n_nlp == 20 * N - 5
    assert NLP.num_duals(N, kt) == o.m_nlp == 18 * N - kt + 16
    assert NLP.cinds(N, kt) == o.cinds()
    lb, ub = NLP.constraint_bounds(N, kt)
    lo, uo = o.bounds()
    assert np.array_equal(lb, lo) and np.array_equal(ub, uo)


@pytest.mark.parametrize("init_mode", [1, 2])
@pytest.mark.parametrize("jac_format", ["dense_blocks", "structural"])
@pytest.mark.parametrize("N,kt", [(61, 21), (40, 14), (2, 2), (80, 79), (80, 2), (12, 13), (12, 1)])
def test_library_layout_sizes_match_oracle(N, kt, jac_format, init_mode):
    """qln_layout is device-free: the sizes it derives from the library's row and vals layouts (row_layout / vals_layout of
    csrc/qln_device.h) for one problem are the oracle's -- m_nlp; in dense blocks nnz and 300 (N-1) + N; in the structural
    format the non-zero step-block values of jac_c_coo at a generic point plus N, and that plus the oracle's constant tail."""
    import ctypes as C

    from quadruped_landing_amd import _lib

    rng = np.random.default_rng(7)
    o = O.OracleNLP(N, kt, init_mode, rng.normal(size=15), rng.normal(size=15), np.zeros((N, 41)))
    Z = rng.normal(size=o.n_nlp)
    Z[19::20] = 0.01
    dense_dyn = 300 * (N - 1)
    tail = o.nnz - dense_dyn - N
    if jac_format == "dense_blocks":
        fmt, want_dyn = _lib.QLN_JAC_FORMAT_DENSE_BLOCKS, dense_dyn + N
    else:
        fmt, want_dyn = _lib.QLN_JAC_FORMAT_STRUCTURAL, int(np.count_nonzero(o.jac_c_coo(Z)[:dense_dyn])) + N
    d = _lib.QlnBatchDesc()
    d.B, d.N = 1, N
    k, m = np.array([kt], dtype=np.int32), np.array([init_mode], dtype=np.int32)
    d.k_trans = k.ctypes.data_as(C.POINTER(C.c_int32))
    d.init_mode = m.ctypes.data_as(C.POINTER(C.c_int32))
    d.cost_batch, d.z_stride, d.align, d.jac_format = 1, 0, 16, fmt
    dims = _lib.QlnDims()
    i64 = C.POINTER(C.c_int64)
    co, jo = np.full(1, -1, dtype=np.int64), np.full(1, -1, dtype=np.int64)
    assert _lib.lib().qln_layout(C.byref(d), C.byref(dims), co.ctypes.data_as(i64), jo.ctypes.data_as(i64)) == _lib.QLN_OK
    assert (dims.m_nlp_max, dims.c_total) == (o.m_nlp, o.m_nlp)
    assert dims.nnz_dynamic == want_dyn
    assert (dims.nnz_max, dims.j_total) == (want_dyn + tail, want_dyn + tail)
    assert (co[0], jo[0]) == (0, 0)


def test_xinds_uinds_are_the_references():
    # src/nlp.jl:38-39: xinds[k] = (k-1)*20 + (1:15), uinds[k] = (k-1)*20 + (16:20)
    xi, ui = NLP.xinds(61), NLP.uinds(61)
    assert len(xi) == 61 and len(ui) == 60
    assert xi[0].tolist() == list(range(1, 16)) and ui[0].tolist() == list(range(16, 21))
    assert xi[60].tolist() == list(range(1201, 1216)) and ui[59][-1] == 1200


def test_pack_unpack_roundtrip():
    rng = np.random.default_rng(0)
    X, U = rng.normal(size=(3, 7, 15)), rng.normal(size=(3, 6, 5))
    Z = NLP.packZ(7, X, U)
    assert Z.shape == (3, 135)
    X2, U2 = NLP.unpackZ(7, Z)
    assert np.array_equal(X, X2) and np.array_equal(U, U2)
    assert np.array_equal(Z[1, 20:35], X[1, 1]) and np.array_equal(Z[1, 35:40], U[1, 1])


@pytest.mark.parametrize("init_mode", [1, 2])
def test_reference_trajectory_and_lqr_cost_bitwise(init_mode):
    model = Q.PlanarQuadruped()
    xterm = PG.terminal_state(model)
    Xr, Ur = Q.reference_trajectory(model, 61, 21, xterm, init_mode, 0.009)
    Xo, Uo = O.reference_trajectory(61, 21, xterm, init_mode, 0.009)
    assert np.array_equal(Ur, Uo)
    assert np.array_equal(Xr[:, :14], Xo[:, :14]) and np.max(np.abs(Xr[:, 14] - Xo[:, 14])) <= 1e-15
    tab = Q.lqr_objective(PG.Q_DIAG, PG.R_DIAG, PG.Q_DIAG, Xr, Ur)
    assert np.array_equal(tab, O.lqr_cost_table(PG.Q_DIAG, PG.R_DIAG, PG.Q_DIAG, Xo, Uo))
    assert Ur[0, 1 if init_mode == 1 else 3] == 98.10000000000001


def test_notebook_problem_matches_oracle_setup():
    nb = PG.notebook_problem()
    nlp, xinit, xterm, Xref, Uref = O.notebook_problem()
    assert np.array_equal(nb.x0[0], xinit) and np.array_equal(nb.xf[0], xterm)
    assert np.array_equal(nb.obj, nlp.cost)
    assert np.array_equal(nb.Z[0], O.notebook_initial_guess(61, 21, xinit, xterm, Uref))


def test_generator_is_deterministic_and_in_range():
    a = PG.make_batch(64, 40, 14, 1, seed=0)
    b = PG.make_batch(64, 40, 14, 1, seed=0)
    assert np.array_equal(a.Z, b.Z) and np.array_equal(a.x0, b.x0)
    assert not np.array_equal(a.Z, PG.make_batch(64, 40, 14, 1, seed=1).Z)
    h = a.Z[:, 19::20]
    assert h.shape == (64, 39) and h.min() >= 0.001 and h.max() <= 0.02
    th = np.rad2deg(a.x0[:, 2])
    assert th.min() >= -40 and th.max() <= -10
    r = PG.make_batch(256, 80, seed=3, ragged=True)
    assert r.k_trans.min() >= 2 and r.k_trans.max() <= 79 and set(np.unique(r.init_mode)) == {1, 2}
    assert r.obj.shape == (256, 80, 41)


def test_moi_surface_names():
    from quadruped_landing_amd import moi

    # the seven MOI methods of src/moi.jl:1-33
    for name in ("eval_objective", "eval_objective_gradient", "eval_constraint", "eval_constraint_jacobian",
                 "features_available", "initialize", "jacobian_structure"):
        assert callable(getattr(moi, name))
    assert moi.features_available(None) == ["Grad", "Jac"] and moi.initialize(None, ["Grad"]) is None


def test_variable_bounds_reproduce_solve_including_quirk_Q6():
    # src/main.ipynb:221-223: 1215 variables, 120 with only lower bounds, 121 with lower and upper bounds
    x_l, x_u = Q.variable_bounds(61)
    lower_only = np.isfinite(x_l) & ~np.isfinite(x_u)
    both = np.isfinite(x_l) & np.isfinite(x_u)
    assert x_l.size == 1215 and lower_only.sum() == 120 and both.sum() == 121
    assert not (~np.isfinite(x_l) & np.isfinite(x_u)).any()
    # theta in [-pi/2, pi/2] at every knot, dt in [0.001, 0.02]
    assert x_l[2] == -np.pi / 2 and x_u[1202] == np.pi / 2 and x_l[19] == 0.001 and x_u[1199 - 20 + 20] == 0.02
    # Q6: the zero lower bounds sit on yb_{k+1}, x1_{k+1} (0-based 21, 23), not on F1y, F2y (16, 18)
    assert x_l[21] == 0.0 and x_l[23] == 0.0 and x_l[16] == -np.inf and x_l[18] == -np.inf
    fl, _ = NLP.variable_bounds_forces(61)
    assert fl[16] == 0.0 and fl[18] == 0.0 and fl[21] == -np.inf


def test_trajectory_io_roundtrip(tmp_path, golden_dir):
    import os
    from quadruped_landing_amd import trajectory_io as TIO

    Z = TIO.load_trajectory(os.path.join(golden_dir, "data_6.csv"))
    assert Z.size == 1215
    p = tmp_path / "z.csv"
    TIO.save_trajectory(str(p), Z)
    assert np.array_equal(TIO.load_trajectory(str(p), 61), Z)  # bit-exact round trip
    tab = TIO.as_plot_table(Z)
    assert tab.shape == (60, 20) and tab[0, 2] == Z[2] and tab[59, 15] == Z[59 * 20 + 15]
    X, U = TIO.states_controls(Z)
    assert X.shape == (61, 15) and U.shape == (60, 5)
    with pytest.raises(ValueError):
        TIO.load_trajectory(str(p), 40)


def test_bench_strict_nnz_counts_match_oracle_structure():
    # bench.py's "strict" roofline figure counts the structurally non-zero entries of each step block:
    # check its three constants against the oracle's forward-mode Jacobian at a generic point
    import bench

    rng = np.random.default_rng(5)
    x, u = rng.normal(size=15), np.append(rng.normal(size=4), 0.01)
    nnz = {m: int(np.count_nonzero(O.contact_jacobian(m, x, u))) for m in (1, 2, 3)}
    assert nnz == {1: bench.NNZ_CONTACT, 2: bench.NNZ_CONTACT, 3: bench.NNZ_FLIGHT}
    mask = np.array([1, 1, 1, 1, 0, 1, 0, 1, 1, 1, 0, 0, 0, 0, 0])  # src/planar_quadruped.jl:262-263 (Q1)
    for m in (1, 2):
        assert int(np.count_nonzero(mask[:, None] * O.contact_jacobian(m, x, u))) == bench.NNZ_JUMP
    # whole problem, against the block-COO values of a full evaluation
    N, kt = 12, 5
    prob = O.OracleNLP(N, kt, 1, rng.normal(size=15), rng.normal(size=15), np.zeros((N, 41)))
    Z = rng.normal(size=prob.n_nlp)
    Z[19::20] = 0.01
    vals = prob.jac_c_coo(Z)
    dyn_nnz = int(np.count_nonzero(vals[: 300 * (N - 1)]))
    assert int(bench.strict_bytes(N, kt)) == 8 * (20 * N - 5) + 8 * prob.m_nlp + 8 * (dyn_nnz + N)


def test_ipopt_initial_point_pushes_exactly_the_bounded_variables_inside():
    """nlp.ipopt_initial_point (the point of Ipopt's iteration 0, KA6): variables without bounds are untouched, bounded
    ones end strictly inside their relaxed bounds, a point already far inside is untouched, and the push distances are
    Ipopt's (bound_push relative to max(1, |bound|), capped by bound_frac of the range when both bounds exist)."""
    import numpy as np
    from quadruped_landing_amd import nlp as NL

    N = 9
    xl, xu = NL.variable_bounds(N)
    Z = np.zeros(NL.num_primals(N))
    Z[19::20] = 0.001            # time steps on their lower bound
    Z[2::20] = 2.0               # theta beyond its upper bound pi/2
    Zp = NL.ipopt_initial_point(Z, xl, xu)
    free = ~np.isfinite(xl) & ~np.isfinite(xu)
    assert np.array_equal(Zp[free], Z[free])
    both = np.isfinite(xl) & np.isfinite(xu)
    assert np.all(Zp[both] > xl[both] - 1e-8) and np.all(Zp[both] < xu[both] + 1e-8)
    h = Zp[19::20]
    assert np.allclose(h, 0.001 - 1e-8 + 0.01 * (0.019 + 2e-8), rtol=0, atol=1e-15)   # bound_frac of the (relaxed) range
    th = Zp[2::20]
    up = np.pi / 2 + 1e-8 * (np.pi / 2)   # relaxed by bound_relax_factor * max(1, |bound|)
    assert np.allclose(th, up - 0.01 * up, rtol=0, atol=1e-15)  # bound_push * |bound| = 0.0157 < bound_frac * range
    lower_only = np.isfinite(xl) & ~np.isfinite(xu)
    assert np.allclose(Zp[lower_only], -1e-8 + 0.01, rtol=0, atol=1e-15)   # yb_{k+1}, x1_{k+1} >= 0 (quirk Q6), pushed to 0.01
    inside = Z.copy()
    inside[19::20] = 0.01
    inside[2::20] = 0.3
    inside[lower_only] = 0.5
    assert np.array_equal(NL.ipopt_initial_point(inside, xl, xu), inside)


def test_drop_state_sampler_carries_numpys_pcg64_state():
    import numpy as np
    from quadruped_landing_amd import problem_gen as PG

    s = PG.drop_state_sampler(7, stream_offset=12)
    st = np.random.PCG64(7).state["state"]
    assert (int(s.pcg_state[0]) << 64) | int(s.pcg_state[1]) == st["state"]
    assert (int(s.pcg_inc[0]) << 64) | int(s.pcg_inc[1]) == st["inc"]
    assert s.stream_offset == 12 and s.two_g == 2 * 9.81
    assert list(s.x0_template) == list(PG.notebook_initial_state(PG.PlanarQuadruped()))
    assert (s.theta_deg[0], s.theta_deg[1]) == PG.THETA0_DEG and (s.omega[0], s.omega[1]) == PG.OMEGA0


def test_ragged_descriptors_are_make_batchs_and_a_rejected_draw_is_detected():
    """config 4's k_trans / init_mode: numpy's Generator.integers is Lemire's multiply-shift on the 32-bit halves
    of the PCG64 outputs, low half first, with a rejection step of probability (2^32 mod range) / 2^32 per draw (22 / 2^32 for
    U{2..79}, never for U{1,2}).  Without a rejection the two calls consume exactly B 64-bit outputs and the drop states follow at
    stream position B -- what the device-side generator relies on; with one, every later position shifts and the workload must be
    generated on the host.  Pinned here: (i) an emulation of that algorithm on PCG64's raw outputs reproduces numpy's integers
    and the stream position behind them (so qln_sample_bounded_integers' kernel, which is the same arithmetic, has a CPU
    witness); (ii) ragged_descriptors returns make_batch's descriptors; (iii) seeds 6076 and 6979 -- found by scanning -- reject
    one draw at B = 65 536, N = 80, and are reported as such."""
    from quadruped_landing_amd import problem_gen as PG

    def emulate(seed, low, high, count, draw_offset):
        raw = np.random.PCG64(seed).random_raw((draw_offset + count + 1) // 2 + 1)
        halves = np.empty(2 * raw.size, dtype=np.uint64)
        halves[0::2], halves[1::2] = raw & np.uint64(0xFFFFFFFF), raw >> np.uint64(32)
        u = halves[draw_offset: draw_offset + count]
        r = np.uint64(high - low)
        m = u * r
        thr = (0xFFFFFFFF - (high - low - 1)) % (high - low)
        return (low + (m >> np.uint64(32))).astype(np.int32), int(((m & np.uint64(0xFFFFFFFF)) < thr).sum())

    for seed, B, N in [(0, 1001, 80), (7, 4096, 80), (3, 333, 12), (11, 2, 3), (12, 5, 3)]:
        kt, im, off = PG.ragged_descriptors(seed, B, N)
        host = PG.make_batch(B, N, seed=seed, ragged=True, build_obj=False)
        draws_kt = 0 if N == 3 else B   # a range of one value (N = 3: k_trans = 2) consumes nothing
        assert off == (draws_kt + B + 1) // 2 and np.array_equal(kt, host.k_trans) and np.array_equal(im, host.init_mode)
        ekt, r1 = emulate(seed, 2, N, B, 0) if draws_kt else (np.full(B, 2, dtype=np.int32), 0)
        eim, r2 = emulate(seed, 1, 3, B, draws_kt)
        assert r1 == 0 and r2 == 0 and np.array_equal(ekt, kt) and np.array_equal(eim, im)
        # the drop states follow at that 64-bit position: theta0 of make_batch is the uniform drawn there
        g = np.random.Generator(np.random.PCG64(seed).advance(off))
        assert np.array_equal(np.deg2rad(g.uniform(*PG.THETA0_DEG, size=B)), host.x0[:, 2])
    for seed in (6076, 6979):
        assert PG.ragged_descriptors(seed, 65536, 80)[2] is None
        assert emulate(seed, 2, 80, 65536, 0)[1] == 1
    assert PG.ragged_descriptors(6075, 65536, 80)[2] == 65536
