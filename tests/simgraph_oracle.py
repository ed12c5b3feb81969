"""numpy restatement of K31, Sim(3) pose-graph optimisation (include/mi355x_match_simgraph.h): the edge residual
e = (Log R_d, t_d, log s_d), its exact first-order 7x7 lines, the cost with K25's Huber term, the undamped system, the update
and Levenberg-Marquardt in two independent forms:
  (a) refine(..., dense=False): the stated algorithm -- block-Jacobi preconditioned conjugate gradients, exactly
      `pcg_iterations` trips per step;
  (b) refine(..., dense=True): the same loop with np.linalg.solve on the dense damped system of the live nodes.
float64 by default.  dtype=np.float32 forms the per-edge lines, the node sums and the PCG vectors in float32 as the kernel
does (dot products, the state and its update stay float64): its distance from the float64 run is what the GPU tolerances of
tests/test_gpu_simgraph.py are set from.  Also the map correction (correct) in float64, in the header's order, rounded once.
One graph per call; every per-edge quantity is vectorised over the edges.  Log, J_l^-1, Exp and the Huber term are
tests/pgo_oracle.py's: K31 takes them from K27 as they are."""
import numpy as np

from pgo_oracle import (LAMBDA0, LAMBDA_MAX, LAMBDA_MIN, LAMBDA_STEP, PIVOT_RATIO, _rho, exp_so3, hat, jl_inv, log_so3,  # noqa: F401
                        rotation_angle_deg)

F32, F64 = np.float32, np.float64
D = 7


def active(N, ei, zs, zr, zt, info, valid):
    ei = np.asarray(ei)
    i, j = ei[:, 0], ei[:, 1]
    zs = np.asarray(zs)
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(zs) & (zs > 0) & np.isfinite(zr).all((1, 2)) & np.isfinite(zt).all(1) & np.isfinite(info).all((1, 2))
    return (np.asarray(valid) != 0) & (i != j) & (i >= 0) & (i < N) & (j >= 0) & (j < N) & fin


def omega(info):
    up = np.triu(np.asarray(info))
    return up + np.swapaxes(np.triu(np.asarray(info), 1), -1, -2)


def residual(si, Ri, ti, sj, Rj, tj, zs, zr, zt):
    """e (E, 7), R_p (E, 3, 3), u = s_d R_d t_z (E, 3), s_p (E,) for stacked edges, in the inputs' dtype"""
    with np.errstate(divide="ignore", invalid="ignore"):
        Rp = Rj @ np.swapaxes(Ri, -1, -2)
        Rd = Rp @ np.swapaxes(zr, -1, -2)
        sp = sj / si
        sd = sp / zs
        u = sd[..., None] * (Rd @ zt[..., None])[..., 0]
        td = tj - sp[..., None] * (Rp @ ti[..., None])[..., 0] - u
        ls = np.log(sd)
    return np.concatenate([log_so3(Rd), td, ls[..., None]], -1).astype(Rp.dtype), Rp, u, sp


def lines(e, Rp, u, sp):
    """J_i, J_j (E, 7, 7)"""
    E = e.shape[0]
    jl = jl_inv(e[:, :3])
    Ji, Jj = np.zeros((E, D, D), e.dtype), np.zeros((E, D, D), e.dtype)
    Jj[:, :3, :3] = jl
    Jj[:, 3:6, :3] = -hat(e[:, 3:6])
    Jj[:, 3:6, 3:6] = np.eye(3, dtype=e.dtype)
    Jj[:, 3:6, 6] = e[:, 3:6]
    Jj[:, 6, 6] = 1
    Ji[:, :3, :3] = -(jl @ Rp)
    Ji[:, 3:6, :3] = -(hat(u) @ Rp)
    Ji[:, 3:6, 3:6] = -sp[:, None, None] * Rp
    Ji[:, 3:6, 6] = u
    Ji[:, 6, 6] = -1
    return Ji, Jj


def _edges(s, R, t, ei, zs, zr, zt, info, act, dtype):
    """the active edges' (index array, i, j, e, R_p, u, s_p, Omega) at the state rounded to dtype"""
    k = np.flatnonzero(act)
    i, j = np.asarray(ei)[k, 0], np.asarray(ei)[k, 1]
    sd, Rd, td = np.asarray(s, F64).astype(dtype), np.asarray(R, F64).astype(dtype), np.asarray(t, F64).astype(dtype)
    e, Rp, u, sp = residual(sd[i], Rd[i], td[i], sd[j], Rd[j], td[j], np.asarray(zs)[k].astype(dtype), np.asarray(zr)[k].astype(dtype),
                            np.asarray(zt)[k].astype(dtype))
    return k, i, j, e, Rp, u, sp, omega(np.asarray(info)[k]).astype(dtype)


def _chi2(e, O, dtype):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.einsum("ea,eab,eb->e", e, O, e).astype(dtype)


def cost(s, R, t, ei, zs, zr, zt, info, valid, huber=0.0, dtype=F64):
    """-> (chi2 (E,), cost float, active (E,) bool)"""
    act = active(len(R), ei, zs, zr, zt, info, valid)
    k, i, j, e, _, _, _, O = _edges(s, R, t, ei, zs, zr, zt, info, act, dtype)
    chi2 = _chi2(e, O, dtype)
    _, rho = _rho(chi2, huber)
    out = np.zeros(len(act), dtype)
    out[k] = np.where(np.isfinite(chi2), chi2, np.inf)
    return out, float(rho.astype(F64).sum()), act


def linearise(s, R, t, ei, zs, zr, zt, info, valid, fixed, huber=0.0, dtype=F64):
    """the undamped system at (s, R, t): dict(diag (N, 7, 7), off (E, 7, 7), g (N, 7), cost, live (N,), act (E,), ei)"""
    N, E = len(R), len(ei)
    fixed = np.asarray(fixed) != 0
    act = active(N, ei, zs, zr, zt, info, valid)
    k, i, j, e, Rp, u, sp, O = _edges(s, R, t, ei, zs, zr, zt, info, act, dtype)
    chi2 = _chi2(e, O, dtype)
    w, rho = _rho(chi2, huber)
    good = np.isfinite(chi2)
    with np.errstate(invalid="ignore", over="ignore"):
        Ji, Jj = lines(e, Rp, u, sp)
        oe = np.einsum("eab,eb->ea", O, e)
        wz = np.where(good, w, 0)[:, None, None].astype(dtype)
        Hii = np.where(good[:, None, None], wz * (np.swapaxes(Ji, 1, 2) @ O @ Ji), 0).astype(dtype)
        Hjj = np.where(good[:, None, None], wz * (np.swapaxes(Jj, 1, 2) @ O @ Jj), 0).astype(dtype)
        Hij = np.where(good[:, None, None], wz * (np.swapaxes(Ji, 1, 2) @ O @ Jj), 0).astype(dtype)
        gi = np.where(good[:, None], wz[:, 0] * np.einsum("eba,eb->ea", Ji, oe), 0).astype(dtype)
        gj = np.where(good[:, None], wz[:, 0] * np.einsum("eba,eb->ea", Jj, oe), 0).astype(dtype)
    live = np.zeros(N, bool)
    live[i] = True
    live[j] = True
    live &= ~fixed
    diag, g = np.zeros((N, D, D), dtype), np.zeros((N, D), dtype)
    # np.add.at adds in the order given: every node meets its edges in ascending edge index
    order = np.argsort(np.concatenate([2 * k, 2 * k + 1]), kind="stable")
    nodes, blocks, grads = np.concatenate([i, j])[order], np.concatenate([Hii, Hjj])[order], np.concatenate([gi, gj])[order]
    np.add.at(diag, nodes, blocks)
    np.add.at(g, nodes, grads)
    diag[~live] = 0
    g[~live] = 0
    off = np.zeros((E, D, D), dtype)
    off[k] = np.where((fixed[i] | fixed[j])[:, None, None], 0, Hij)
    return dict(diag=diag, off=off, g=g, cost=float(rho.astype(F64).sum()), live=live, act=act, ei=np.asarray(ei), chi2=chi2)


def _factor(M):
    """LDL^T of one 7x7 block under K18's pivot rule, float64 -> (L, d) or None"""
    dmax = np.diag(M).max()
    if not dmax > 0:
        return None
    L, d = np.eye(D), np.zeros(D)
    A = M.copy()
    for c in range(D):
        d[c] = A[c, c]
        if not (d[c] > PIVOT_RATIO * dmax) or not np.isfinite(d[c]):
            return None
        L[c + 1:, c] = A[c, c + 1:] / d[c]
        A[c + 1:, c + 1:] -= np.outer(L[c + 1:, c], L[c + 1:, c]) * d[c]
    return L, d


def block_solve(Dn, lam, r, dtype=F64):
    """z = (D + lam diag D)^-1 r through the factors rounded to dtype, or None where the block fails the pivot rule"""
    M = np.asarray(Dn, F64).copy()
    M[np.diag_indices(D)] += F64(dtype(lam)) * np.diag(M)
    f = _factor(M)
    if f is None:
        return None
    L, d = f[0].astype(dtype), f[1].astype(dtype)
    y = np.asarray(r, dtype).copy()
    for i in range(D):
        y[i + 1:] -= L[i + 1:, i] * y[i]
    z = y / d
    for i in range(D - 1, -1, -1):
        z[:i] -= L[i, :i] * z[i]
    return z


def _apply(lin, lam, p, dtype):
    """(H + lam diag H) p for p (N, 7), rows of nodes that are not live left 0"""
    lamf = dtype(lam)
    out = np.einsum("nab,nb->na", lin["diag"], p) + lamf * np.einsum("naa,na->na", lin["diag"], p)
    k = np.flatnonzero(lin["act"])
    i, j = lin["ei"][k, 0], lin["ei"][k, 1]
    np.add.at(out, i, np.einsum("eab,eb->ea", lin["off"][k], p[j]))
    np.add.at(out, j, np.einsum("eba,eb->ea", lin["off"][k], p[i]))
    return out.astype(dtype)


def pcg_step(lin, lam, trips, dtype=F64):
    """the header's "Solve": dx (N, 7) after exactly `trips` trips, and the mask of frozen nodes"""
    N = len(lin["diag"])
    lamf = dtype(lam)
    on = lin["live"].copy()
    Minv = np.zeros((N, D, D), dtype)
    for n in np.flatnonzero(on):
        cols = [block_solve(lin["diag"][n], lamf, c, dtype) for c in np.eye(D, dtype=dtype)]
        if cols[0] is None:
            on[n] = False
        else:
            Minv[n] = np.stack(cols, 1)
    mask = on[:, None]
    prec = lambda r: np.einsum("nab,nb->na", Minv, r).astype(dtype)
    dot = lambda a, b: float((a.astype(F64) * b.astype(F64)).sum())
    x = np.zeros((N, D), dtype)
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
    """the damped system of the live nodes as a dense (7n, 7n) float64 matrix, its gradient and the live nodes' indices"""
    nodes = np.flatnonzero(lin["live"])
    pos = {int(n): a for a, n in enumerate(nodes)}
    H, g = np.zeros((D * len(nodes), D * len(nodes))), np.zeros(D * len(nodes))
    for a, n in enumerate(nodes):
        H[D * a:D * a + D, D * a:D * a + D] = lin["diag"][n]
        g[D * a:D * a + D] = lin["g"][n]
    for e in np.flatnonzero(lin["act"]):
        i, j = (int(v) for v in lin["ei"][e])
        if i in pos and j in pos:
            H[D * pos[i]:D * pos[i] + D, D * pos[j]:D * pos[j] + D] += lin["off"][e]
            H[D * pos[j]:D * pos[j] + D, D * pos[i]:D * pos[i] + D] += lin["off"][e].T
    return H + lam * np.diag(np.diag(H)), g, nodes


def dense_step(lin, lam):
    H, g, nodes = dense_matrix(lin, lam)
    dx = np.zeros((len(lin["diag"]), D))
    dx[nodes] = np.linalg.solve(H, -g).reshape(-1, D)
    return dx, np.zeros(len(dx), bool)


def update(s, R, t, dx):
    """the header's update of a float64 state: R <- Exp(w) R, s <- exp(sigma) s, t <- exp(sigma) Exp(w) t + tau"""
    s2, R2, t2 = s.copy(), R.copy(), t.copy()
    for n in np.flatnonzero(np.any(dx != 0, 1)):
        E, k = exp_so3(dx[n, :3]), np.exp(dx[n, 6])
        s2[n], R2[n], t2[n] = k * s[n], E @ R[n], k * (E @ t[n]) + dx[n, 3:6]
    return s2, R2, t2


def refine(s0, R0, t0, ei, zs, zr, zt, info, valid, fixed, iterations=10, pcg_iterations=64, huber=0.0, dtype=F64, dense=False):
    """K25's loop on the Sim(3) graph -> dict(s, R, t float32; s64, R64, t64; chi2; cost0, cost; accepted; info; ok; costs)"""
    s, R, t = np.asarray(s0, F64).copy(), np.asarray(R0, F64).copy(), np.asarray(t0, F64).copy()
    a = (ei, zs, zr, zt, info, valid)
    _, c0, act = cost(s, R, t, *a, huber, dtype)
    fx = np.asarray(fixed) != 0
    lin = linearise(s, R, t, *a, fixed, huber, dtype)
    refused = not np.isfinite(c0) or not act.any() or not fx.any() or not lin["live"].any()
    if refused:
        c = 0.0 if not act.any() else np.inf
        return dict(s=np.asarray(s0, F32), R=np.asarray(R0, F32), t=np.asarray(t0, F32), s64=s, R64=R, t64=t, chi2=np.zeros(len(ei), F32),
                    cost0=c, cost=c, accepted=0, info=np.zeros((len(R), D, D), F32), ok=False, costs=[c])
    lam, c, accepted, costs = LAMBDA0, c0, 0, [c0]
    for _ in range(iterations):
        dx, _ = dense_step(lin, lam) if dense else pcg_step(lin, lam, pcg_iterations, dtype)
        sc, Rc, tc = update(s, R, t, dx.astype(F64))
        _, cc, _ = cost(sc, Rc, tc, *a, huber, dtype)
        if np.isfinite(cc) and cc < c:
            s, R, t, c, accepted = sc, Rc, tc, cc, accepted + 1
            lin = linearise(s, R, t, *a, fixed, huber, dtype)
            lam = max(lam / LAMBDA_STEP, LAMBDA_MIN)
        else:
            lam = min(lam * LAMBDA_STEP, LAMBDA_MAX)
        costs.append(c)
    chi2, _, _ = cost(s, R, t, *a, 0.0, dtype)
    return dict(s=s.astype(F32), R=R.astype(F32), t=t.astype(F32), s64=s, R64=R, t64=t, chi2=chi2, cost0=c0, cost=c, accepted=accepted,
                info=lin["diag"], ok=True, costs=costs)


def correct(r_old, t_old, s, r, t, points, ref):
    """mi_simgraph_correct for one graph: float32 arrays in, float64 arithmetic in the header's order, rounded once ->
    (r_out (N, 3, 3), t_out (N, 3), points_out (L, 3)) float32"""
    r_old, t_old, s, r, t, points = (np.asarray(a, F32).astype(F64) for a in (r_old, t_old, s, r, t, points))
    ref = np.asarray(ref)
    N = len(s)
    with np.errstate(divide="ignore", invalid="ignore"):
        t_out = (t / s[:, None]).astype(F32) if N else np.zeros((0, 3), F32)
        out = points.copy()
        ok = (ref >= 0) & (ref < N)
        k = ref[ok]
        X = points[ok]
        Ro, Rn = r_old[k], r[k]
        y = ((Ro[:, :, 0] * X[:, None, 0] + Ro[:, :, 1] * X[:, None, 1]) + Ro[:, :, 2] * X[:, None, 2]) + t_old[k]
        d = y - t[k]
        out[ok] = ((Rn[:, 0, :] * d[:, None, 0] + Rn[:, 1, :] * d[:, None, 1]) + Rn[:, 2, :] * d[:, None, 2]) / s[k][:, None]
    return r.astype(F32), t_out, out.astype(F32)


def camera_centres(s, R, t):
    """the camera centres -R^T t / s of a state, float64"""
    s, R, t = np.asarray(s, F64), np.asarray(R, F64), np.asarray(t, F64)
    return -np.einsum("nba,nb->na", R, t) / s[:, None]
