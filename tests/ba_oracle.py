"""Numpy restatement of K25, windowed bundle adjustment (include/mi355x_match.h, "windowed bundle adjustment"), for ONE
window.  Every function takes `dt`: with numpy.float64 it is the oracle the kernels are tested against; with numpy.float32
the per-observation work (the lines, a landmark's V, h and inverse, Y, the products that enter S, the point step) is done
in the kernel's number format and in the kernel's operation order, vectorised over the landmarks -- the sums ACROSS
landmarks are numpy's pairwise float32 sums where the kernel has lanes-strided partial sums, which is the difference the
GPU tolerances leave room for (tests/test_ba_host.py measures it).  The reduced system is solved in float64 either way.

Shapes: R (F, 3, 3), t (F, 3), X (L, 3), obs (F, L, 2) normalised (u, v), vis (F, L)."""
import numpy as np

LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = 1e-4, 1e-9, 1e6
PIVOT_RATIO = 1e-6
SMALL_ANGLE = 1e-8


def active(vis):
    return (np.asarray(vis) != 0).sum(axis=0) >= 2


def frame_lines(R, t, X, uv, huber, dt):
    """The lines of every landmark in one frame (csrc/ba_math.h: ba_line), in the kernel's operation order: dict of ok (L,),
    ju, jv (L, 6), xu, xv (L, 3), ru, rv, e2, w, rho (L,).  Where ok is False the lines are zero and rho = e2 = +inf."""
    R, t, X, uv = (np.asarray(a, dt) for a in (R, t, X, uv))
    hub = dt(huber)
    one = dt(1)
    with np.errstate(all="ignore"):
        x = ((R[0, 0] * X[:, 0] + R[0, 1] * X[:, 1]) + R[0, 2] * X[:, 2]) + t[0]
        y = ((R[1, 0] * X[:, 0] + R[1, 1] * X[:, 1]) + R[1, 2] * X[:, 2]) + t[1]
        z = ((R[2, 0] * X[:, 0] + R[2, 1] * X[:, 1]) + R[2, 2] * X[:, 2]) + t[2]
        xn, yn, iz = x / z, y / z, one / z
        zero = np.zeros_like(x)
        ju = np.stack([-(xn * yn), one + xn * xn, -yn, iz, zero, -(xn * iz)], axis=1)
        jv = np.stack([-(one + yn * yn), xn * yn, xn, zero, iz, -(yn * iz)], axis=1)
        ru, rv = xn - uv[:, 0], yn - uv[:, 1]
        front = z > 0
        ju, jv = np.where(front[:, None], ju, 0).astype(dt), np.where(front[:, None], jv, 0).astype(dt)
        ru, rv = np.where(front, ru, 0).astype(dt), np.where(front, rv, 0).astype(dt)
        xu = ju[:, 3:4] * R[0][None, :] + ju[:, 5:6] * R[2][None, :]
        xv = jv[:, 4:5] * R[1][None, :] + jv[:, 5:6] * R[2][None, :]
        e2 = ru * ru + rv * rv
        ok = front & (e2 < np.inf)
        e = np.sqrt(e2)
        far = (hub > 0) & (e > hub)
        w = np.where(far, hub / e, one).astype(dt)
        rho = np.where(far, (dt(2) * hub) * e - hub * hub, e2).astype(dt)
    inf = dt(np.inf)
    k6, k3 = ok[:, None], ok[:, None]
    return dict(ok=ok, ju=np.where(k6, ju, 0).astype(dt), jv=np.where(k6, jv, 0).astype(dt), xu=np.where(k3, xu, 0).astype(dt),
                xv=np.where(k3, xv, 0).astype(dt), ru=np.where(ok, ru, 0).astype(dt), rv=np.where(ok, rv, 0).astype(dt),
                e2=np.where(ok, e2, inf).astype(dt), w=np.where(ok, w, 0).astype(dt), rho=np.where(ok, rho, inf).astype(dt))


def cost(R, t, X, obs, vis, huber, dt=np.float64):
    """-> (e2 (F, L): 0 where not seen or inactive, cost, active (L,))"""
    vis = np.asarray(vis) != 0
    act = active(vis)
    F, L = vis.shape
    e2 = np.zeros((F, L), dt)
    per = np.zeros(L, dt)                                  # a landmark's own sum, over its frames in index order
    for f in range(F):
        ln = frame_lines(R[f], t[f], X, np.where(vis[f][:, None], obs[f], 0), huber, dt)
        use = vis[f] & act
        e2[f] = np.where(use, ln["e2"], 0)
        with np.errstate(invalid="ignore"):
            per = (per + np.where(use, ln["rho"], 0)).astype(dt)
    return e2, float(np.sum(per, dtype=dt)), act


def inv3(V6, lam, dt):
    """csrc/ba_math.h: ba_inv3 for V (L, 6) = (00 01 02 11 12 22) -> (Vi (L, 6), usable (L,))"""
    lam = dt(lam)
    with np.errstate(all="ignore"):
        m = [V6[:, 0] + lam * V6[:, 0], V6[:, 1], V6[:, 2], V6[:, 3] + lam * V6[:, 3], V6[:, 4], V6[:, 5] + lam * V6[:, 5]]
        c = [m[3] * m[5] - m[4] * m[4], m[2] * m[4] - m[1] * m[5], m[1] * m[4] - m[2] * m[3], m[0] * m[5] - m[2] * m[2],
             m[1] * m[2] - m[0] * m[4], m[0] * m[3] - m[1] * m[1]]
        det = (m[0] * c[0] + m[1] * c[1]) + m[2] * c[2]
        p1, p2 = c[5] / m[0], det / c[5]
        dmax = np.maximum(np.maximum(m[0], m[3]), m[5])
        pmin = np.where(p1 > m[0], m[0], p1)
        pmin = np.where(p2 < pmin, p2, pmin)
        ok = (dmax > 0) & (pmin > dt(PIVOT_RATIO) * dmax)
        vi = np.stack([ck / det for ck in c], axis=1).astype(dt)
        ok = ok & np.all(np.abs(vi) < np.inf, axis=1)
    return np.where(ok[:, None], vi, 0).astype(dt), ok


def _sym3(v6):
    return np.stack([np.stack([v6[:, 0], v6[:, 1], v6[:, 2]], 1), np.stack([v6[:, 1], v6[:, 3], v6[:, 4]], 1),
                     np.stack([v6[:, 2], v6[:, 4], v6[:, 5]], 1)], 1)


def _cross(ln):
    """W (L, 6, 3) = (w J_u[i]) X_u[c] + (w J_v[i]) X_v[c]"""
    a, b = ln["w"][:, None] * ln["ju"], ln["w"][:, None] * ln["jv"]
    return a[:, :, None] * ln["xu"][:, None, :] + b[:, :, None] * ln["xv"][:, None, :]


def _dot3(A, B):
    """(L, 6, 6): (A_i0 B_j0 + A_i1 B_j1) + A_i2 B_j2"""
    return (A[:, :, None, 0] * B[:, None, :, 0] + A[:, :, None, 1] * B[:, None, :, 1]) + A[:, :, None, 2] * B[:, None, :, 2]


def linearise(R, t, X, obs, vis, num_fixed, huber, lam=0.0, dt=np.float64):
    """One linearisation at damping lam: dict of the explicit blocks U (F, 6, 6), g (F, 6) (zero for fixed frames), V (L, 3, 3)
    (undamped), h (L, 3), W (F, L, 6, 3) (zero for fixed frames), Vi (L, 3, 3) (damped inverse, zero when frozen or inactive),
    active, and the reduced system S (n, n), b (n) in float64, n = 6 (F - num_fixed); `lines`: the per-frame lines with
    the entries that add nothing masked out."""
    vis = np.asarray(vis) != 0
    F, L = vis.shape
    act = active(vis)
    lines = []
    V6, h = np.zeros((L, 6), dt), np.zeros((L, 3), dt)
    pairs3 = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    for f in range(F):
        ln = frame_lines(R[f], t[f], X, np.where(vis[f][:, None], obs[f], 0), huber, dt)
        use = vis[f] & act & ln["ok"]
        for k in ("ju", "jv", "xu", "xv"):
            ln[k] = np.where(use[:, None], ln[k], 0).astype(dt)
        for k in ("ru", "rv", "w"):
            ln[k] = np.where(use, ln[k], 0).astype(dt)
        ln["use"] = use
        lines.append(ln)
        wu, wv = ln["w"][:, None] * ln["xu"], ln["w"][:, None] * ln["xv"]
        for k, (i, j) in enumerate(pairs3):
            V6[:, k] = (V6[:, k] + wu[:, i] * ln["xu"][:, j]) + wv[:, i] * ln["xv"][:, j]
        for i in range(3):
            h[:, i] = (h[:, i] + wu[:, i] * ln["ru"]) + wv[:, i] * ln["rv"]
    vi6, usable = inv3(V6, lam, dt)
    vi6 = np.where(act[:, None], vi6, 0).astype(dt)
    Vi = _sym3(vi6)
    nfree = F - num_fixed
    n = 6 * nfree
    U, g, W = np.zeros((F, 6, 6)), np.zeros((F, 6)), np.zeros((F, L, 6, 3), dt)
    S, b = np.zeros((n, n)), np.zeros(n)
    Y = {}
    for f in range(num_fixed, F):
        ln = lines[f]
        W[f] = _cross(ln)
        Y[f] = ((W[f][:, :, 0, None] * Vi[:, None, 0, :] + W[f][:, :, 1, None] * Vi[:, None, 1, :]) + W[f][:, :, 2, None] * Vi[:, None, 2, :]).astype(dt)
        wu, wv = ln["w"][:, None] * ln["ju"], ln["w"][:, None] * ln["jv"]
        Ul = wu[:, :, None] * ln["ju"][:, None, :] + wv[:, :, None] * ln["jv"][:, None, :]      # (L, 6, 6); the kernel adds the two terms one after the other
        gl = wu * ln["ru"][:, None] + wv * ln["rv"][:, None]
        U[f] = np.sum(Ul, axis=0, dtype=dt)
        g[f] = np.sum(gl, axis=0, dtype=dt)
        Q = np.sum(_dot3(Y[f], W[f]), axis=0, dtype=dt).astype(np.float64)
        q = np.sum((Y[f][:, :, 0] * h[:, None, 0] + Y[f][:, :, 1] * h[:, None, 1]) + Y[f][:, :, 2] * h[:, None, 2], axis=0, dtype=dt).astype(np.float64)
        p = 6 * (f - num_fixed)
        Ud = U[f] + lam * np.diag(np.diag(U[f]))
        Q = np.triu(Q) + np.triu(Q, 1).T                  # the kernel forms i <= j only
        S[p:p + 6, p:p + 6] = Ud - Q
        b[p:p + 6] = g[f] - q
    for f in range(num_fixed, F):
        for f2 in range(f + 1, F):
            Q = np.sum(_dot3(Y[f], W[f2]), axis=0, dtype=dt).astype(np.float64)
            p, p2 = 6 * (f - num_fixed), 6 * (f2 - num_fixed)
            S[p:p + 6, p2:p2 + 6] = -Q
            S[p2:p2 + 6, p:p + 6] = -Q.T
    return dict(U=U, g=g, V=_sym3(V6), h=h, W=W, Vi=Vi, vi6=vi6, frozen=act & ~usable, active=act, S=S, b=b, lines=lines)


def ldlt_solve(S, b):
    """S x = -b by the header's LDL^T (column by column, every element updated in the order of j), float64 -> (x, usable).
    The bits of csrc/ba_math.h: ba_ldlt_solve."""
    a = np.array(S, np.float64)
    x = np.array(b, np.float64)
    n = len(x)
    if n == 0:
        return x, True
    dmax = np.max(np.diag(a))
    if not dmax > 0:
        return np.zeros(n), False
    for j in range(n):
        d = a[j, j]
        if not (d > PIVOT_RATIO * dmax) or not d < np.inf:
            return np.zeros(n), False
        lj = a[j, j + 1:] / d
        a[j, j + 1:] = lj
        a[j + 1:, j + 1:] -= (lj[:, None] * lj[None, :]) * d         # only the upper triangle is read later
    x = -x
    for i in range(n):
        x[i + 1:] = x[i + 1:] - a[i, i + 1:] * x[i]
    x = x / np.diag(a)
    for i in range(n - 1, -1, -1):
        x[:i] = x[:i] - a[:i, i] * x[i]
    return x, bool(np.all(np.abs(x) < np.inf))


def exp_so3(w):
    w = np.asarray(w, np.float64)
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = np.sqrt(th2)
    a, bb = 1.0, 0.0
    if th >= SMALL_ANGLE:
        a, bb = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    kx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + a * kx + bb * (kx @ kx)


def step(lin, R64, t64, X, num_fixed, dt=np.float64):
    """The Schur step of a linearisation: (usable, candidate R64, t64 (float64 poses), candidate X (dt), dp, dX)"""
    dp, usable = ldlt_solve(lin["S"], lin["b"])
    F = R64.shape[0]
    if not usable:
        return False, R64, t64, X, dp, np.zeros_like(X)
    Rc, tc = R64.copy(), t64.copy()
    s = lin["h"].astype(dt).copy()
    dpf = dp.astype(dt)
    for f in range(num_fixed, F):
        d = dp[6 * (f - num_fixed):6 * (f - num_fixed) + 6]
        E = exp_so3(d[:3])
        Rc[f], tc[f] = E @ R64[f], E @ t64[f] + d[3:]
        ln, df = lin["lines"][f], dpf[6 * (f - num_fixed):6 * (f - num_fixed) + 6]
        su, sv = ln["ju"][:, 0] * df[0], ln["jv"][:, 0] * df[0]
        for i in range(1, 6):
            su, sv = su + ln["ju"][:, i] * df[i], sv + ln["jv"][:, i] * df[i]
        for a in range(3):
            s[:, a] = (s[:, a] + (ln["w"] * ln["xu"][:, a]) * su) + (ln["w"] * ln["xv"][:, a]) * sv
    Vi = lin["Vi"]
    dX = -((Vi[:, :, 0] * s[:, None, 0] + Vi[:, :, 1] * s[:, None, 1]) + Vi[:, :, 2] * s[:, None, 2])
    return True, Rc, tc, (np.asarray(X, dt) + dX.astype(dt)).astype(dt), dp, dX


def refine(R, t, X, obs, vis, num_fixed, iterations, huber, dt=np.float64):
    """The LM loop -> dict(R, t, X (float32, as the kernel returns them), point_ok, cost0, cost, accepted, info, ok)"""
    f32 = np.float32
    R64, t64 = np.asarray(R, np.float64).copy(), np.asarray(t, np.float64).copy()
    Xs = np.asarray(X, dt).copy()
    act = active(vis)

    def at(Ra, ta):                                      # the pose the lines are formed at: rounded to float32
        return (Ra.astype(f32), ta.astype(f32))

    _, c0, _ = cost(*at(R64, t64), Xs, obs, vis, huber, dt)
    F = R64.shape[0]
    if not np.isfinite(c0) or not act.any():
        c0 = 0.0 if not act.any() else np.inf
        return dict(R=np.asarray(R, f32), t=np.asarray(t, f32), X=np.asarray(X, f32), point_ok=np.zeros(len(act), bool), cost0=c0, cost=c0,
                    accepted=0, info=np.zeros((6 * F, 6 * F)), ok=False, costs=[c0])
    lam, cur, accepted, costs = LAMBDA0, c0, 0, [c0]
    for _ in range(iterations):
        lin = linearise(*at(R64, t64), Xs, obs, vis, num_fixed, huber, lam, dt)
        usable, Rc, tc, Xc, _, _ = step(lin, R64, t64, Xs, num_fixed, dt)
        c = np.inf
        if usable:
            _, c, _ = cost(*at(Rc, tc), Xc, obs, vis, huber, dt)
        if usable and np.isfinite(c) and c < cur:
            R64, t64, Xs, cur, accepted = Rc, tc, Xc, c, accepted + 1
            lam = max(lam / 10.0, LAMBDA_MIN)
        else:
            lam = min(lam * 10.0, LAMBDA_MAX)
        costs.append(cur)
    lin = linearise(*at(R64, t64), Xs, obs, vis, num_fixed, huber, 0.0, dt)
    return dict(R=R64.astype(f32), t=t64.astype(f32), X=Xs.astype(f32), point_ok=act.copy(), cost0=c0, cost=cur, accepted=accepted,
                info=full_system(lin["S"], F, num_fixed), ok=True, costs=costs, R64=R64, t64=t64, X64=Xs)


def full_system(S, F, num_fixed):
    out = np.zeros((6 * F, 6 * F))
    out[6 * num_fixed:, 6 * num_fixed:] = S
    return out


def full_rhs(b, F, num_fixed):
    out = np.zeros(6 * F)
    out[6 * num_fixed:] = b
    return out


def normalise(keypoints_yx, K):
    """pixel (y, x) -> normalised (u, v), float32, for a camera matrix without skew"""
    kp = np.asarray(keypoints_yx, np.float64)
    return np.stack([(kp[..., 1] - K[0, 2]) / K[0, 0], (kp[..., 0] - K[1, 2]) / K[1, 1]], axis=-1).astype(np.float32)


def gauge_align(R, t, X, X_ref, act):
    """With one fixed frame the scale of a window about camera 0 is free.  -> (t, X) scaled about camera 0's centre so that
    the active points' mean distance from it equals X_ref's; rotations are unaffected."""
    R, t, X = (np.asarray(a, np.float64) for a in (R, t, X))
    c0 = -R[0].T @ t[0]
    s = np.linalg.norm(X_ref[act] - c0, axis=1).sum() / np.linalg.norm(X[act] - c0, axis=1).sum()
    Xs = X.copy()
    Xs[act] = c0 + s * (X[act] - c0)
    ts = np.stack([-R[f] @ (c0 + s * (-R[f].T @ t[f] - c0)) for f in range(R.shape[0])])
    return ts, Xs


def rotation_angle_deg(Ra, Rb):
    """the angle of Ra^T Rb from its skew part and its trace (an arccos of the trace alone loses half the digits near 0)"""
    M = np.asarray(Ra, np.float64).T @ np.asarray(Rb, np.float64)
    sk = 0.5 * np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    return float(np.degrees(np.arctan2(np.linalg.norm(sk), (np.trace(M) - 1.0) / 2.0)))
