"""numpy yardstick of qln_tracking_covariance (include/qln_evaluator.h): the covariance recursion of the closed-loop
roll-out on given step blocks, the packed lower-triangle layout, and the eight marginals of a knot.  dtype-generic: the
arrays keep the dtype they come in with (float64, or longdouble to measure the recursion's own rounding)."""
import numpy as np

NX, NU, NNZ, MARG = 15, 4, 120, 8


def _tril():
    return np.tril_indices(NX)  # row-major over the lower triangle: (i, j) at i(i+1)/2 + j


def pack(S):
    """(..., 15, 15) -> (..., 120): the lower triangle, row i >= j at i(i+1)/2 + j."""
    r, c = _tril()
    return np.ascontiguousarray(np.asarray(S)[..., r, c])


def unpack(P):
    """(..., 120) -> (..., 15, 15) symmetric."""
    P = np.asarray(P)
    r, c = _tril()
    out = np.zeros(P.shape[:-1] + (NX, NX), dtype=P.dtype)
    out[..., r, c] = P
    out[..., c, r] = P
    return out


def closed_loop_blocks(A, B, K):
    """Acl_k = A_k - B_k K_k (K None: A_k), (N-1, 15, 15)."""
    A = np.asarray(A)
    return A.copy() if K is None else A - np.asarray(B) @ np.asarray(K)


def propagate(A, B, K, Sigma0, W=None):
    """Sigma_0 = Sigma0, Sigma_{k+1} = Acl_k Sigma_k Acl_k' + diag(W), each formed on its lower triangle (exactly
    symmetric).  A (..., N-1, 15, 15), B (..., N-1, 15, 4), K (..., N-1, 4, 15) or None, Sigma0 (..., 15, 15) or (15, 15),
    W (15,) or None -> (..., N, 15, 15)."""
    Acl = closed_loop_blocks(A, B, K)
    dt = np.result_type(Acl.dtype, np.asarray(Sigma0).dtype)
    lead, n1 = Acl.shape[:-3], Acl.shape[-3]
    S = np.broadcast_to(unpack(pack(np.asarray(Sigma0, dtype=dt))), lead + (NX, NX))
    Wm = np.zeros((NX, NX), dtype=dt) if W is None else np.diag(np.asarray(W, dtype=dt))
    out = np.zeros(lead + (n1 + 1, NX, NX), dtype=dt)
    out[..., 0, :, :] = S
    for k in range(n1):
        a = Acl[..., k, :, :]
        S = unpack(pack(a @ S @ np.swapaxes(a, -1, -2) + Wm))
        out[..., k + 1, :, :] = S
    return out


def explicit(A, B, K, Sigma0, W=None):
    """The same covariances from explicit transition products: Sigma_k = Phi_k Sigma0 Phi_k' + sum_{j<k} Phi_{k,j} W Phi_{k,j}'
    with Phi_k = Acl_{k-1} .. Acl_0 and Phi_{k,j} = Acl_{k-1} .. Acl_{j+1}."""
    Acl = closed_loop_blocks(A, B, K)
    N = len(Acl) + 1
    S0 = np.asarray(Sigma0, dtype=Acl.dtype)
    Wm = np.zeros((NX, NX), dtype=Acl.dtype) if W is None else np.diag(np.asarray(W, dtype=Acl.dtype))
    out = np.zeros((N, NX, NX), dtype=Acl.dtype)

    def phi(k, j):  # Acl_{k-1} .. Acl_{j+1}
        P = np.eye(NX, dtype=Acl.dtype)
        for i in range(j + 1, k):
            P = Acl[i] @ P
        return P

    for k in range(N):
        Pk = phi(k, -1)
        S = Pk @ S0 @ Pk.T
        for j in range(k):
            Pj = phi(k, j)
            S = S + Pj @ Wm @ Pj.T
        out[k] = S
    return out


def clearance_dtheta(theta, lb):
    """The derivative entry jac_c! writes for the clearance row (theta == 0 takes the + branch, quirk Q3)."""
    theta = np.asarray(theta)
    return np.where(theta > 0, -lb / 2 * np.cos(theta), lb / 2 * np.cos(theta))


def marginals(Sigma, K, theta, lb):
    """Sigma (..., N, 15, 15), K (..., N-1, 4, 15) or None, theta (..., N) -> (..., N, 8): the clearance row's variance
    a' Sigma a with a = e_yb + c'(theta) e_theta, the four force variances diag(K Sigma K') (zeros without K and at the
    last knot), Sigma[4][4], Sigma[6][6] and the trace."""
    Sigma = np.asarray(Sigma)
    N = Sigma.shape[-3]
    out = np.zeros(Sigma.shape[:-2] + (MARG,), dtype=Sigma.dtype)
    a = np.zeros(Sigma.shape[:-2] + (NX,), dtype=Sigma.dtype)
    a[..., 1] = 1.0
    a[..., 2] = clearance_dtheta(theta, lb)
    out[..., 0] = np.einsum("...i,...ij,...j->...", a, Sigma, a)
    if K is not None:
        K = np.asarray(K)
        out[..., : N - 1, 1:5] = np.einsum("...mi,...ij,...mj->...m", K, Sigma[..., : N - 1, :, :], K)
    out[..., 5] = Sigma[..., 4, 4]
    out[..., 6] = Sigma[..., 6, 6]
    out[..., 7] = np.trace(Sigma, axis1=-2, axis2=-1)
    return out


def knot_rel(got, ref):
    """Worst per-knot relative Frobenius error over (..., N, 15, 15) (exact zeros compare as zero)."""
    got, ref = np.asarray(got), np.asarray(ref)
    num = np.linalg.norm((got - ref).reshape(got.shape[:-2] + (-1,)).astype(np.float64), axis=-1)
    den = np.linalg.norm(ref.reshape(ref.shape[:-2] + (-1,)).astype(np.float64), axis=-1)
    return float(np.max(np.where(num == 0.0, 0.0, num / np.maximum(den, 1e-300))))


def entry_rel(got, ref):
    """Worst entry-wise error relative to max(|ref|, 1e-300) (exact zeros compare as zero)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    d = np.abs(got - ref)
    return float(np.max(np.where(d == 0.0, 0.0, d / np.maximum(np.abs(ref), 1e-300))))


def random_psd(rng, scale=1.0, shape=()):
    """Random positive semi-definite 15x15 matrices G G' * scale."""
    G = rng.normal(size=shape + (NX, NX))
    return scale * (G @ np.swapaxes(G, -1, -2)) / NX
