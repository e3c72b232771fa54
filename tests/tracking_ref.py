"""numpy yardstick of the TVLQR tracking entry points (include/qln_evaluator.h, qln_tracking_lqr): the Riccati recursion
on given step blocks, a dense KKT solve of the same linear-quadratic problem, and step blocks from the CPU oracle."""
import numpy as np

NX, NU = 15, 4
JUMP_ROWS = (4, 6, 10, 11, 12, 13)  # rows the jump map zeroes (0-based); it keeps row 14, the clock


def riccati(A, B, Q, R, Qf):
    """A (..., N-1, 15, 15), B (..., N-1, 15, 4) -> K (..., N-1, 4, 15), P (..., N, 15, 15) of the header's recursion."""
    A, B = np.asarray(A), np.asarray(B)
    n1 = A.shape[-3]
    Pk = np.broadcast_to(np.diag(Qf), A.shape[:-3] + (NX, NX)).copy()
    K = np.zeros(A.shape[:-3] + (n1, NU, NX))
    P = np.zeros(A.shape[:-3] + (n1 + 1, NX, NX))
    P[..., n1, :, :] = Pk
    for k in range(n1 - 1, -1, -1):
        a, b = A[..., k, :, :], B[..., k, :, :]
        bT = np.swapaxes(b, -1, -2)
        quu = np.diag(R) + bT @ Pk @ b
        qux = bT @ Pk @ a
        kk = np.linalg.solve(quu, qux)
        Pk = np.diag(Q) + np.swapaxes(a, -1, -2) @ Pk @ a - np.swapaxes(qux, -1, -2) @ kk
        Pk = 0.5 * (Pk + np.swapaxes(Pk, -1, -2))
        K[..., k, :, :] = kk
        P[..., k, :, :] = Pk
    return K, P


def kkt(A, B, Q, R, Qf, dx1):
    """The linearised tracking problem as one equality-constrained QP: min J over (dx_1..dx_N, du_1..du_{N-1}) with dx_1
    fixed and dx_{k+1} = A_k dx_k + B_k du_k.  Returns (du (N-1, 4), dx (N, 15), J)."""
    n1 = len(A)
    N = n1 + 1
    nv = NX * N + NU * n1
    H = np.zeros((nv, nv))
    for k in range(N):
        w = Qf if k == N - 1 else Q
        H[NX * k: NX * (k + 1), NX * k: NX * (k + 1)] = 2 * np.diag(w)
    for k in range(n1):
        o = NX * N + NU * k
        H[o: o + NU, o: o + NU] = 2 * np.diag(R)
    C = np.zeros((NX * N, nv))
    d = np.zeros(NX * N)
    C[:NX, :NX] = np.eye(NX)
    d[:NX] = dx1
    for k in range(n1):
        r = NX * (k + 1)
        C[r: r + NX, NX * k: NX * (k + 1)] = A[k]
        C[r: r + NX, NX * (k + 1): NX * (k + 2)] = -np.eye(NX)
        C[r: r + NX, NX * N + NU * k: NX * N + NU * (k + 1)] = B[k]
    M = np.block([[H, C.T], [C, np.zeros((C.shape[0], C.shape[0]))]])
    sol = np.linalg.solve(M, np.concatenate([np.zeros(nv), d]))
    v = sol[:nv]
    dx = v[: NX * N].reshape(N, NX)
    du = v[NX * N:].reshape(n1, NU)
    return du, dx, 0.5 * v @ H @ v


def closed_loop(A, B, K, dx1):
    """dx_{k+1} = (A_k - B_k K_k) dx_k: (du (N-1, 4), dx (N, 15))."""
    dx = [np.asarray(dx1, dtype=float)]
    du = []
    for k in range(len(A)):
        u = -K[k] @ dx[-1]
        du.append(u)
        dx.append(A[k] @ dx[-1] + B[k] @ u)
    return np.array(du), np.array(dx)


def lq_cost(dx, du, Q, R, Qf):
    return float(np.sum(dx[:-1] ** 2 * Q) + np.sum(du ** 2 * R) + np.sum(dx[-1] ** 2 * Qf))


def blocks_from_dense(blocks, k_trans, restore_clock=True):
    """Evaluator step blocks (N-1, 15, 20) -> A (N-1, 15, 15), B (N-1, 15, 4); row 14 of the jump knot restored."""
    A = np.array(blocks[:, :, :15])
    B = np.array(blocks[:, :, 15:19])
    kj = k_trans - 2  # 0-based jump knot
    if restore_clock and 0 <= kj < len(A):
        A[kj, 14, 14] = 1.0
    return A, B


def oracle_blocks(N, k_trans, init_mode, Z, model=None, restore_clock=True):
    """Step blocks of the CPU oracle (contact_jacobian times the jump mask) at the knots of Z (n_nlp,)."""
    from oracle import oracle as O

    blocks = np.zeros((N - 1, NX, 20))
    for k in range(N - 1):
        K = k + 1
        mode = init_mode if K <= k_trans - 1 else 3
        x, u = Z[20 * k: 20 * k + 15], Z[20 * k + 15: 20 * k + 20]
        J = O.contact_jacobian(mode, x, u, model)
        if K == k_trans - 1:
            J = J.copy()
            J[list(JUMP_ROWS) + [14], :] = 0.0
        blocks[k] = J
    return blocks_from_dense(blocks, k_trans, restore_clock)
