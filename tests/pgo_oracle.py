"""numpy restatement of K27, pose-graph optimisation (include/mi355x_match.h): the edge residual
e = (Log R_d, t_d), its exact first-order lines, the cost with K25's Huber term, the undamped system, and Levenberg-Marquardt
in two independent forms:
  (a) refine(..., dense=False): the stated algorithm -- block-Jacobi preconditioned conjugate gradients, exactly
      `pcg_iterations` trips per step;
  (b) refine(..., dense=True): the same loop with np.linalg.solve on the dense damped system of the live nodes.
float64 by default.  dtype=np.float32 forms the per-edge lines, the node sums and the PCG vectors in float32 as the kernel
does (dot products, the pose state and its update stay float64): its distance from the float64 run is what the GPU
tolerances of tests/test_gpu_pgo.py are set from.  One graph per call; every per-edge quantity is vectorised over the edges."""
import numpy as np

F32, F64 = np.float32, np.float64
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX, LAMBDA_STEP = 1e-4, 1e-9, 1e6, 10.0
PIVOT_RATIO = 1e-6
LOG_SMALL, LOG_NEAR_PI, JL_SERIES = 1e-4, -0.9, 0.0625


def hat(v):
    v = np.asarray(v)
    z = np.zeros_like(v[..., 0])
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, -v[..., 0]], -1),
                     np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def exp_so3(w):
    """Rodrigues, float64, one vector"""
    w = np.asarray(w, F64)
    th = np.linalg.norm(w)
    K = hat(w)
    if th < 1e-8:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def log_so3(R):
    """(..., 3, 3) -> (..., 3), the header's "Log", in R's dtype"""
    R = np.asarray(R)
    dt = R.dtype.type
    v = dt(0.5) * np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    s2 = (v * v).sum(-1)
    s = np.sqrt(s2)
    c = dt(0.5) * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - dt(1))
    theta = np.arctan2(s, c)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(s < dt(LOG_SMALL), dt(1) + s2 / dt(6), theta / s)
        phi = k[..., None] * v
        near = c < dt(LOG_NEAR_PI)
        if np.any(near):
            diag = np.stack([R[..., 0, 0], R[..., 1, 1], R[..., 2, 2]], -1)
            m = np.argmax(diag, -1)
            d = dt(1) - c
            am = np.sqrt(np.maximum((np.take_along_axis(diag, m[..., None], -1)[..., 0] - c) / d, dt(0)))
            sym = R + np.swapaxes(R, -1, -2)
            row = np.take_along_axis(sym, m[..., None, None].repeat(3, -1), -2)[..., 0, :]
            a = row / (dt(2) * d * am)[..., None]
            a = np.where(np.arange(3) == m[..., None], am[..., None], a)
            sg = np.where((a * v).sum(-1) < 0, -theta, theta)
            phi = np.where(near[..., None], sg[..., None] * a, phi)
    return phi.astype(R.dtype)


def jl_inv(phi):
    """(..., 3) -> (..., 3, 3): the inverse left Jacobian of SO(3), in phi's dtype"""
    phi = np.asarray(phi)
    dt = phi.dtype.type
    th2 = (phi * phi).sum(-1)
    h = dt(0.5) * np.sqrt(th2)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(th2 < dt(JL_SERIES), dt(1 / 12) + th2 / dt(720) + th2 * th2 / dt(30240), (dt(1) - h * np.cos(h) / np.sin(h)) / th2)
    eye = np.eye(3, dtype=phi.dtype)
    sq = phi[..., :, None] * phi[..., None, :] - th2[..., None, None] * eye
    return (eye - dt(0.5) * hat(phi) + k[..., None, None] * sq).astype(phi.dtype)


def active(N, ei, zr, zt, info, valid):
    ei = np.asarray(ei)
    i, j = ei[:, 0], ei[:, 1]
    fin = np.isfinite(zr).all((1, 2)) & np.isfinite(zt).all(1) & np.isfinite(info).all((1, 2))
    return (np.asarray(valid) != 0) & (i != j) & (i >= 0) & (i < N) & (j >= 0) & (j < N) & fin


def omega(info):
    up = np.triu(np.asarray(info))
    return up + np.swapaxes(np.triu(np.asarray(info), 1), -1, -2)


def residual(Ri, ti, Rj, tj, zr, zt):
    """e (E, 6), R_p (E, 3, 3), u = R_d t_z (E, 3) for stacked edges, in the inputs' dtype"""
    Rp = Rj @ np.swapaxes(Ri, -1, -2)
    Rd = Rp @ np.swapaxes(zr, -1, -2)
    u = (Rd @ zt[..., None])[..., 0]
    td = tj - (Rp @ ti[..., None])[..., 0] - u
    return np.concatenate([log_so3(Rd), td], -1), Rp, u


def lines(e, Rp, u):
    """J_i, J_j (E, 6, 6)"""
    E = e.shape[0]
    jl = jl_inv(e[:, :3])
    Ji, Jj = np.zeros((E, 6, 6), e.dtype), np.zeros((E, 6, 6), e.dtype)
    Jj[:, :3, :3] = jl
    Jj[:, 3:, :3] = -hat(e[:, 3:])
    Jj[:, 3:, 3:] = np.eye(3, dtype=e.dtype)
    Ji[:, :3, :3] = -(jl @ Rp)
    Ji[:, 3:, :3] = -(hat(u) @ Rp)
    Ji[:, 3:, 3:] = -Rp
    return Ji, Jj


def _edges(R, t, ei, zr, zt, info, act, dtype):
    """the active edges' (index array, i, j, e, R_p, u, Omega) at the poses rounded to dtype"""
    k = np.flatnonzero(act)
    i, j = np.asarray(ei)[k, 0], np.asarray(ei)[k, 1]
    Rd, td = np.asarray(R, F64).astype(dtype), np.asarray(t, F64).astype(dtype)
    e, Rp, u = residual(Rd[i], td[i], Rd[j], td[j], np.asarray(zr)[k].astype(dtype), np.asarray(zt)[k].astype(dtype))
    return k, i, j, e, Rp, u, omega(np.asarray(info)[k]).astype(dtype)


def _rho(chi2, huber):
    dt = chi2.dtype.type
    with np.errstate(invalid="ignore"):
        chi = np.sqrt(chi2)
        out = (huber > 0) & (chi > dt(huber))
        rho = np.where(out, dt(2 * huber) * chi - dt(huber) * dt(huber), chi2)
        w = np.where(out, dt(huber) / np.where(out, chi, dt(1)), dt(1))
    bad = ~np.isfinite(chi2)
    return np.where(bad, dt(0), w).astype(chi2.dtype), np.where(bad, dt(np.inf), rho).astype(chi2.dtype)


def cost(R, t, ei, zr, zt, info, valid, huber=0.0, dtype=F64):
    """-> (chi2 (E,), cost float, active (E,) bool)"""
    act = active(len(R), ei, zr, zt, info, valid)
    k, i, j, e, _, _, O = _edges(R, t, ei, zr, zt, info, act, dtype)
    chi2 = np.einsum("ea,eab,eb->e", e, O, e).astype(dtype)
    _, rho = _rho(chi2, huber)
    out = np.zeros(len(act), dtype)
    out[k] = np.where(np.isfinite(chi2), chi2, np.inf)
    return out, float(rho.astype(F64).sum()), act


def linearise(R, t, ei, zr, zt, info, valid, fixed, huber=0.0, dtype=F64):
    """the undamped system at (R, t): dict(diag (N, 6, 6), off (E, 6, 6), g (N, 6), cost, live (N,), act (E,), ei)"""
    N, E = len(R), len(ei)
    fixed = np.asarray(fixed) != 0
    act = active(N, ei, zr, zt, info, valid)
    k, i, j, e, Rp, u, O = _edges(R, t, ei, zr, zt, info, act, dtype)
    chi2 = np.einsum("ea,eab,eb->e", e, O, e).astype(dtype)
    w, rho = _rho(chi2, huber)
    good = np.isfinite(chi2)
    Ji, Jj = lines(e, Rp, u)
    oe = np.einsum("eab,eb->ea", O, e)
    wz = np.where(good, w, 0)[:, None, None].astype(dtype)
    with np.errstate(invalid="ignore"):
        Hii = np.where(good[:, None, None], wz * (np.swapaxes(Ji, 1, 2) @ O @ Ji), 0).astype(dtype)
        Hjj = np.where(good[:, None, None], wz * (np.swapaxes(Jj, 1, 2) @ O @ Jj), 0).astype(dtype)
        Hij = np.where(good[:, None, None], wz * (np.swapaxes(Ji, 1, 2) @ O @ Jj), 0).astype(dtype)
        gi = np.where(good[:, None], wz[:, 0] * np.einsum("eba,eb->ea", Ji, oe), 0).astype(dtype)
        gj = np.where(good[:, None], wz[:, 0] * np.einsum("eba,eb->ea", Jj, oe), 0).astype(dtype)
    live = np.zeros(N, bool)
    live[i] = True
    live[j] = True
    live &= ~fixed
    diag, g = np.zeros((N, 6, 6), dtype), np.zeros((N, 6), dtype)
    # np.add.at adds in the order given: every node meets its edges in ascending edge index
    order = np.argsort(np.concatenate([2 * k, 2 * k + 1]), kind="stable")
    nodes, blocks, grads = np.concatenate([i, j])[order], np.concatenate([Hii, Hjj])[order], np.concatenate([gi, gj])[order]
    np.add.at(diag, nodes, blocks)
    np.add.at(g, nodes, grads)
    diag[~live] = 0
    g[~live] = 0
    off = np.zeros((E, 6, 6), dtype)
    off[k] = np.where((fixed[i] | fixed[j])[:, None, None], 0, Hij)
    return dict(diag=diag, off=off, g=g, cost=float(rho.astype(F64).sum()), live=live, act=act, ei=np.asarray(ei), chi2=chi2)


def _factor(M):
    """LDL^T of one 6x6 block under K18's pivot rule, float64 -> (L, d) or None"""
    dmax = np.diag(M).max()
    if not dmax > 0:
        return None
    L, d = np.eye(6), np.zeros(6)
    A = M.copy()
    for c in range(6):
        d[c] = A[c, c]
        if not (d[c] > PIVOT_RATIO * dmax) or not np.isfinite(d[c]):
            return None
        L[c + 1:, c] = A[c, c + 1:] / d[c]
        A[c + 1:, c + 1:] -= np.outer(L[c + 1:, c], L[c + 1:, c]) * d[c]
    return L, d


def block_solve(D, lam, r, dtype=F64):
    """z = (D + lam diag D)^-1 r through the factors rounded to dtype, or None where the block fails the pivot rule"""
    M = np.asarray(D, F64).copy()
    M[np.diag_indices(6)] += F64(dtype(lam)) * np.diag(M)
    f = _factor(M)
    if f is None:
        return None
    L, d = f[0].astype(dtype), f[1].astype(dtype)
    y = np.asarray(r, dtype).copy()
    for i in range(6):
        y[i + 1:] -= L[i + 1:, i] * y[i]
    z = y / d
    for i in range(5, -1, -1):
        z[:i] -= L[i, :i] * z[i]
    return z


def _apply(lin, lam, p, dtype):
    """(H + lam diag H) p for p (N, 6), rows of nodes that are not live left 0"""
    lamf = dtype(lam)
    out = np.einsum("nab,nb->na", lin["diag"], p) + lamf * np.einsum("naa,na->na", lin["diag"], p)
    k = np.flatnonzero(lin["act"])
    i, j = lin["ei"][k, 0], lin["ei"][k, 1]
    np.add.at(out, i, np.einsum("eab,eb->ea", lin["off"][k], p[j]))
    np.add.at(out, j, np.einsum("eba,eb->ea", lin["off"][k], p[i]))
    return out.astype(dtype)


def pcg_step(lin, lam, trips, dtype=F64):
    """the header's "Solve": dx (N, 6) after exactly `trips` trips, and the mask of frozen nodes"""
    N = len(lin["diag"])
    lamf = dtype(lam)
    on = lin["live"].copy()
    Minv = np.zeros((N, 6, 6), dtype)
    for n in np.flatnonzero(on):
        cols = [block_solve(lin["diag"][n], lamf, c, dtype) for c in np.eye(6, dtype=dtype)]
        if cols[0] is None:
            on[n] = False
        else:
            Minv[n] = np.stack(cols, 1)
    mask = on[:, None]
    prec = lambda r: np.einsum("nab,nb->na", Minv, r).astype(dtype)
    dot = lambda a, b: float((a.astype(F64) * b.astype(F64)).sum())
    x = np.zeros((N, 6), dtype)
    r = np.where(mask, -lin["g"], 0).astype(dtype)
    z = prec(r)
    p = z.copy()
    rz = dot(r, z)
    dead = False
    for _ in range(trips):
        q = np.where(mask, _apply(lin, lamf, p, dtype), 0).astype(dtype)
        pap = dot(p, q)
        dead = dead or not (pap > 0) or not np.isfinite(pap) or rz == 0
        alpha = dtype(0 if dead else rz / pap)
        x = (x + alpha * p).astype(dtype)
        r = (r - alpha * q).astype(dtype)
        z = prec(r)
        rz_new = dot(r, z)
        if not dead:
            p = (z + dtype(rz_new / rz) * p).astype(dtype)
            rz = rz_new
    return x, lin["live"] & ~on


def dense_matrix(lin, lam=0.0):
    """the damped system of the live nodes as a dense (6n, 6n) float64 matrix, its gradient and the live nodes' indices"""
    nodes = np.flatnonzero(lin["live"])
    pos = {int(n): a for a, n in enumerate(nodes)}
    H, g = np.zeros((6 * len(nodes), 6 * len(nodes))), np.zeros(6 * len(nodes))
    for a, n in enumerate(nodes):
        H[6 * a:6 * a + 6, 6 * a:6 * a + 6] = lin["diag"][n]
        g[6 * a:6 * a + 6] = lin["g"][n]
    for e in np.flatnonzero(lin["act"]):
        i, j = (int(v) for v in lin["ei"][e])
        if i in pos and j in pos:
            H[6 * pos[i]:6 * pos[i] + 6, 6 * pos[j]:6 * pos[j] + 6] += lin["off"][e]
            H[6 * pos[j]:6 * pos[j] + 6, 6 * pos[i]:6 * pos[i] + 6] += lin["off"][e].T
    return H + lam * np.diag(np.diag(H)), g, nodes


def dense_step(lin, lam):
    H, g, nodes = dense_matrix(lin, lam)
    dx = np.zeros((len(lin["diag"]), 6))
    dx[nodes] = np.linalg.solve(H, -g).reshape(-1, 6)
    return dx, np.zeros(len(dx), bool)


def update(R, t, dx):
    """K18's update of float64 poses: R <- Exp(w) R, t <- Exp(w) t + tau"""
    R2, t2 = R.copy(), t.copy()
    for n in np.flatnonzero(np.any(dx != 0, 1)):
        E = exp_so3(dx[n, :3])
        R2[n], t2[n] = E @ R[n], E @ t[n] + dx[n, 3:]
    return R2, t2


def refine(R0, t0, ei, zr, zt, info, valid, fixed, iterations=10, pcg_iterations=64, huber=0.0, dtype=F64, dense=False):
    """K25's loop on the pose graph -> dict(R, t float32; R64, t64; chi2; cost0, cost; accepted; info; ok; costs)"""
    R, t = np.asarray(R0, F64).copy(), np.asarray(t0, F64).copy()
    a = (ei, zr, zt, info, valid)
    _, c0, act = cost(R, t, *a, huber, dtype)
    fx = np.asarray(fixed) != 0
    lin = linearise(R, t, *a, fixed, huber, dtype)
    refused = not np.isfinite(c0) or not act.any() or not fx.any() or not lin["live"].any()
    if refused:
        c = 0.0 if not act.any() else np.inf
        return dict(R=np.asarray(R0, F32), t=np.asarray(t0, F32), R64=R, t64=t, chi2=np.zeros(len(ei), F32), cost0=c, cost=c, accepted=0,
                    info=np.zeros((len(R), 6, 6), F32), ok=False, costs=[c])
    lam, c, accepted, costs = LAMBDA0, c0, 0, [c0]
    for _ in range(iterations):
        dx, _ = dense_step(lin, lam) if dense else pcg_step(lin, lam, pcg_iterations, dtype)
        Rc, tc = update(R, t, dx.astype(F64))
        _, cc, _ = cost(Rc, tc, *a, huber, dtype)
        if np.isfinite(cc) and cc < c:
            R, t, c, accepted = Rc, tc, cc, accepted + 1
            lin = linearise(R, t, *a, fixed, huber, dtype)
            lam = max(lam / LAMBDA_STEP, LAMBDA_MIN)
        else:
            lam = min(lam * LAMBDA_STEP, LAMBDA_MAX)
        costs.append(c)
    chi2, _, _ = cost(R, t, *a, 0.0, dtype)
    return dict(R=R.astype(F32), t=t.astype(F32), R64=R, t64=t, chi2=chi2, cost0=c0, cost=c, accepted=accepted, info=lin["diag"], ok=True,
                costs=costs)


def rotation_angle_deg(Ra, Rb):
    """the angle of Ra Rb^T by atan2(sin, cos): arccos of the trace alone turns a rounding error d of float32 matrices into
    an angle of sqrt(d)"""
    M = np.asarray(Ra, F64) @ np.asarray(Rb, F64).T
    s = 0.5 * np.linalg.norm([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    return float(np.degrees(np.arctan2(s, (np.trace(M) - 1) / 2)))
