"""Do two builds of libqln_hip.so give the same bits in the three sweeps that keep symmetric 15 x 15 images in LDS --
qln_tracking_covariance, qln_tracking_kalman, qln_landing_smoother and their _guarded forms (csrc/qln_image15.h)?
   python bench/tracking_image_bits_ab.py <other libqln_hip.so> [<this libqln_hip.so>]
starts one fresh child per library, one after the other and each under a time limit of its own, stops at the first child that
does not exit 0, and compares every pair of dumped arrays as uint64 views (NaN sentinels compare equal): one line per array,
"values, how many differ", and a verdict.  Exit status 0 only if no value differs.
   QLN_LIB_PATH=<libqln_hip.so> python bench/tracking_image_bits_ab.py --child <directory>
is the child: it runs the calls below on fixed seeds with the library QLN_LIB_PATH names and writes every output array into
the directory, then prints which kernel instantiations its calls reach (all ten must be).  That list is derived from the
arguments of the calls as the launch wrappers at the end of csrc/qln_tracking_kernels.hip dispatch them today -- K given or not,
the guarded entry point or the plain one -- not observed in the library: after a change of that dispatch, read it again.

Shapes: the smallest at which these kernels can go wrong.  B = 5 (two waves, the second with three rows past the batch's end)
at N = 2, 3, 16, 17, 33, 40 -- one step; the clearance derivatives' sixteen-knot blocks with a partial last block and, at 17
and 33, the (N - 1) & 15 == 0 tail; the tests' own size -- and B = 70 at N = 17: ragged k_trans and step lengths, both
init_modes (the handle takes 1 and 2; mode 3 is what a problem is in after its touchdown), z_stride = 20 N + 3.
Calls: covariance with K and K == NULL, sigma0_batch 1 and B, Sigma and marg both and each alone, guarded with and without
ev_var; Kalman at ny = 1, 3, 8 with K and as the filter alone, the full set of outputs and each alone, guarded with and without
ev_var; the smoother on those Kalman outputs at ny = 1, 3, 8, both outputs and each alone.  Both batches run every one of these.
Host forms: one per entry point (every output, Kalman and the smoother at ny = 3), at N = 3 and at N = 17 of both batches.
The guarded record is the guarded roll-out's of the same library, and the child refuses to go on unless the batch holds a
problem that touches down in the first step (ks = 0), one in the last (ks = N - 2) and one that never lands (ks = -1)."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NS = (2, 3, 16, 17, 33, 40)
CHILD_LIMIT = 300  # seconds; a child takes a few
REACHED = set()


def free_foot(im):
    return (6, 13) if im == 1 else (4, 11)


def dev(a):
    import torch

    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return None if t is None else (t if isinstance(t, np.ndarray) else t.cpu().numpy())


def guarded_batch(B, N, seed, ragged, model, **kw):
    """A handle and the inputs of a guarded roll-out whose record holds ks = 0 (problem 0), ks = N - 2 (problem 1: its free
    foot's start height is searched with the roll-out itself) and ks = -1 (the last problem: its reference pulls the foot up)."""
    from quadruped_landing_amd import HybridNLP, problem_gen as PG

    def handle(b, **k):
        return HybridNLP(model, b.obj, b.init_mode, b.k_trans, b.N, b.x0, b.xf, **k)

    kt = min(max(N // 3, 2), N - 1) if N > 2 else 2
    im0 = 1 + seed % 2
    batch = PG.make_batch(B, N, kt, im0, seed=seed, ragged=ragged, model=model)
    rng = np.random.default_rng(seed + 7)
    Zref = np.ascontiguousarray(batch.Z, dtype=np.float64)
    K = 0.05 * rng.normal(size=(B, N - 1, 4, 15))
    th = np.array(model.plant_parameters()) * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, size=(B, 4)))
    x0 = Zref[:, :15] + 1e-2 * rng.normal(size=(B, 15))
    span = float(Zref[1, 19::20].sum())
    for b in range(B):
        iy, iv = free_foot(int(batch.init_mode[b]))
        x0[b, iy], x0[b, iv] = rng.uniform(0.0, span), -1.0
    iy, iv = free_foot(int(batch.init_mode[0]))
    x0[0, iy] = 1e-4  # at v = -1 m/s the foot is down within the first step (h >= 1e-3 s)
    iy, iv = free_foot(int(batch.init_mode[B - 1]))
    Zref[B - 1, 15 + (3 if batch.init_mode[B - 1] == 1 else 1)::20] = -2.0
    x0[B - 1, iy], x0[B - 1, iv] = 0.3, 0.0
    # Problem 1 falls freely: no reference force on its free foot (the reference's support force behind its k_trans would drive
    # the foot down there) and a tenth of the gains.  Its start height: 1024 copies of the problem over a ladder of heights up to
    # one and a half times the free fall over the whole span, the first that lands in the last step.
    P = 1024
    Zref[1, 15 + (3 if batch.init_mode[1] == 1 else 1)::20] = 0.0
    K[1] *= 0.1
    probe = PG.make_batch(P, N, kt, int(batch.init_mode[1]), seed=seed, model=model)
    hp = handle(probe)
    iy, iv = free_foot(int(batch.init_mode[1]))
    xp = np.tile(x0[1], (P, 1))
    xp[:, iy] = np.linspace(1e-4, 1.5 * (span + 0.5 * abs(model.g) * span * span), P)
    _, evp = hp.tracking_rollout_guarded(hp.upload_Z(np.tile(Zref[1], (P, 1))), dev(np.tile(K[1], (P, 1, 1, 1))), dev(xp),
                                         dev(np.tile(th[1], (P, 1))))
    hit = np.flatnonzero(evp.cpu().numpy()[:, 0] == N - 2)
    if not len(hit):
        raise SystemExit(f"B={B} N={N}: no start height of the ladder lands in the last step")
    x0[1, iy] = xp[hit[0], iy]
    del hp
    nlp = handle(batch, **kw)
    Zr, dK, dx, dm = nlp.upload_Z(Zref), dev(K), dev(x0), dev(th)
    Zout, ev = nlp.tracking_rollout_guarded(Zr, dK, dx, dm)
    ks = ev.cpu().numpy()[:, 0]
    if not (ks[0] == 0 and ks[1] == N - 2 and ks[B - 1] == -1):
        raise SystemExit(f"B={B} N={N}: the record's touchdown knots {ks[0]}, {ks[1]}, {ks[B - 1]} are not 0, N - 2, -1")
    return nlp, dict(K=K, th=th, dK=dK, dm=dm, Zout=Zout, ev=ev, Zplain=nlp.tracking_rollout(Zr, dK, dx))


def child(outdir):
    import torch

    from quadruped_landing_amd import _lib
    from quadruped_landing_amd.planar_quadruped import PlanarQuadruped

    model = PlanarQuadruped(g=-9.1, mb=8.7, mf=0.13, lb=0.46, l1=0.27, l2=0.22)
    count = [0]

    def dump(name, arrays, names):
        for a, n in zip(arrays, names):
            if a is not None:
                np.save(os.path.join(outdir, f"{name}_{n}.npy"), host(a))
                count[0] += 1

    def inst(kernel, *flags):
        REACHED.add(f"{kernel}<{', '.join('true' if f else 'false' for f in flags)}>")

    for B, N, ragged in [(5, n, False) for n in NS] + [(70, 17, True)]:
        kw = dict(z_stride=20 * N + 3, align=1) if ragged else {}
        nlp, g = guarded_batch(B, N, 1000 * N + B, ragged, model, **kw)
        rng = np.random.default_rng(N + B)
        A = rng.normal(size=(B, 15, 15))
        S0 = A @ np.swapaxes(A, 1, 2) / 15.0
        W = rng.uniform(0.0, 1e-2, size=15)
        zp, zg, ev, dK, dm = g["Zplain"], g["Zout"], g["ev"], g["dK"], g["dm"]
        tag = f"B{B}_N{N}"
        with_host = N in (3, 17)
        # ---- covariance ----
        for kn, k_ in (("K", dK), ("open", None)):
            for sn, s0 in (("sB", S0), ("s1", S0[0])):
                for fl in ((True, True), (True, False), (False, True)):
                    f = "".join(str(int(v)) for v in fl)
                    dump(f"{tag}_cov_{kn}_{sn}_{f}", nlp.tracking_covariance(zp, k_, s0, W, *fl), ("S", "marg"))
                    inst("k_tracking_covariance", k_ is not None, False, False)
                    for wv in (True, False):
                        dump(f"{tag}_covg_{kn}_{sn}_{f}_v{int(wv)}", nlp.tracking_covariance_guarded(zg, ev, k_, s0, W, dm, *fl, wv),
                             ("S", "marg", "var"))
                        inst("k_tracking_covariance", k_ is not None, True, True)
        if with_host:
            dump(f"{tag}_cov_host", nlp.tracking_covariance_host(host(zp), g["K"], S0, W), ("S", "marg"))
            dump(f"{tag}_covg_host", nlp.tracking_covariance_guarded_host(host(zg), host(ev), g["K"], S0, W, g["th"]), ("S", "marg", "var"))
        # ---- Kalman, and the smoother on its outputs ----
        for ny in (1, 3, 8):
            H, V = rng.normal(size=(ny, 15)) / np.sqrt(15.0), rng.uniform(0.5, 2.0, size=ny)
            Xhat, innov = dev(rng.normal(size=(B, N, 15))), dev(rng.normal(size=(B, N, ny)))
            kal = nlp.tracking_kalman(zp, H, V, dK, S0, W)
            kalg = nlp.tracking_kalman_guarded(zg, ev, H, V, dK, S0, W, dm)
            dump(f"{tag}_kal_ny{ny}_all", kal, ("L", "Pe", "S", "marg"))
            dump(f"{tag}_kalg_ny{ny}_all", kalg, ("L", "Pe", "S", "marg", "var"))
            inst("k_tracking_kalman", True, False, False)
            inst("k_tracking_kalman", True, True, True)
            for i in range(4):
                fl = [q == i for q in range(4)]
                dump(f"{tag}_kal_ny{ny}_only{i}", nlp.tracking_kalman(zp, H, V, dK, S0[0], W, *fl), ("L", "Pe", "S", "marg"))
            for i in range(5):
                fl = [q == i for q in range(5)]
                dump(f"{tag}_kalg_ny{ny}_only{i}", nlp.tracking_kalman_guarded(zg, ev, H, V, dK, S0[0], W, dm, *fl),
                     ("L", "Pe", "S", "marg", "var"))
            dump(f"{tag}_kalg_ny{ny}_nov", nlp.tracking_kalman_guarded(zg, ev, H, V, dK, S0, W, dm, with_event_var=False),
                 ("L", "Pe", "S", "marg", "var"))
            for fl in ((True, True), (True, False), (False, True)):  # the filter alone
                f = "".join(str(int(v)) for v in fl)
                dump(f"{tag}_fil_ny{ny}_{f}", nlp.tracking_kalman(zp, H, V, None, S0, W, *fl), ("L", "Pe", "S", "marg"))
                dump(f"{tag}_filg_ny{ny}_{f}", nlp.tracking_kalman_guarded(zg, ev, H, V, None, S0, W, dm, *fl), ("L", "Pe", "S", "marg", "var"))
                inst("k_tracking_kalman", False, False, False)
                inst("k_tracking_kalman", False, True, True)
                dump(f"{tag}_smo_ny{ny}_{f}", nlp.landing_smoother(zp, kal[0], kal[1], H, V, Xhat, innov, *fl), ("Xs", "Ps"))
                dump(f"{tag}_smog_ny{ny}_{f}", nlp.landing_smoother_guarded(zg, ev, kalg[0], kalg[1], H, V, Xhat, innov, dm, *fl), ("Xs", "Ps"))
                inst("k_landing_smoother", False)
                inst("k_landing_smoother", True)
            if with_host and ny == 3:
                dump(f"{tag}_kal_host", nlp.tracking_kalman_host(host(zp), H, V, g["K"], S0, W), ("L", "Pe", "S", "marg"))
                dump(f"{tag}_kalg_host", nlp.tracking_kalman_guarded_host(host(zg), host(ev), H, V, g["K"], S0, W, g["th"]),
                     ("L", "Pe", "S", "marg", "var"))
                a = (host(kal[0]), host(kal[1]), H, V, host(Xhat), host(innov))
                dump(f"{tag}_smo_host", nlp.landing_smoother_host(host(zp), *a), ("Xs", "Ps"))
                a = (host(kalg[0]), host(kalg[1]), H, V, host(Xhat), host(innov), g["th"])
                dump(f"{tag}_smog_host", nlp.landing_smoother_guarded_host(host(zg), host(ev), *a), ("Xs", "Ps"))
        torch.cuda.synchronize()
        del nlp, g
    print(f"{os.path.basename(os.path.dirname(_lib.LIB_PATH)) or '.'}/{os.path.basename(_lib.LIB_PATH)}: {count[0]} arrays; reached "
          f"{len(REACHED)} instantiations: " + "; ".join(sorted(REACHED)))
    if len(REACHED) != 10:
        raise SystemExit("not all ten instantiations were reached")


def parent(libs):
    dirs = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, lib in enumerate(libs):  # one child at a time has the GPU open
            d = os.path.join(tmp, str(i))
            os.mkdir(d)
            dirs.append(d)
            env = dict(os.environ, QLN_LIB_PATH=os.path.abspath(lib))
            try:
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", d], env=env, timeout=CHILD_LIMIT).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(f"child for {lib} ended with status {rc}: nothing more is started")
                return 2
        names = sorted(os.listdir(dirs[0]))
        if names != sorted(os.listdir(dirs[1])):
            print("the two children wrote different sets of arrays")
            return 2
        bad = values = 0
        for n in names:
            a, b = (np.load(os.path.join(d, n)) for d in dirs)
            if a.shape != b.shape:
                print(f"{n:48s} shapes {a.shape} and {b.shape}")
                bad += 1
                continue
            diff = int((np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64)).sum())
            print(f"{n:48s} {a.size:9d} values, {diff:10d} differ")
            values += a.size
            bad += diff > 0
        rel = [os.path.relpath(os.path.abspath(lib), ROOT) for lib in libs]
        print(f"VERDICT {rel[0]} vs {rel[1]}: {len(names)} arrays, {values} values, {bad} arrays with differences")
        return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2])
    elif len(sys.argv) > 1:
        here = os.path.join(ROOT, "quadruped_landing_amd", "csrc", "libqln_hip.so")
        sys.exit(parent([sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else here]))
    else:
        sys.exit(__doc__)
