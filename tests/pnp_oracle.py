"""numpy restatement of the K23 absolute-pose algorithm (include/mi355x_match.h, "absolute pose"), in two parts.

THE ORACLE (float64, `dtype` selects float32 for the score and the refit's rows): the counter-based sampler (pose_oracle's
hash, 4 slots), the header's degeneracy tests, a P3P minimal solver that is NOT the header's -- Grunert's substitution
u = l2 / l1, v = l3 / l1, v eliminated linearly between the two ratio equations, the quartic in u formed by numpy's
polynomial arithmetic and solved by numpy.roots (companion-matrix eigenvalues), five Newton steps on the three
law-of-cosines equations, Horn's alignment through numpy.linalg.eigh (rigid_oracle) -- the header's disambiguation by the
fourth row, its reprojection MSAC score, its Gauss-Newton refit and its local-optimisation schedule.

THE RESTATEMENT (`*_f32`): csrc/pnp_math.h and what it calls of csrc/rigid_math.h, operation by operation on numpy.float32
scalars (numpy.float64 where the C++ says double).  tests/native/pnp_host.cpp, the same header compiled for the host, must
return its bits; its deviation from the oracle is what the host and GPU tests take their tolerances from.

Host only; shared by tests/test_pnp_host.py and tests/test_gpu_pnp*.py."""
import numpy as np

import pose_oracle as PO
import rigid_oracle as RO

F = np.float32
D = np.float64
INF32 = F(np.inf)
DEG = F(1e-6)                    # RG_DEGENERATE
JACOBI_SWEEPS = 6                # RG_JACOBI_SWEEPS
CUBIC_NEWTON = 24                # PNP_CUBIC_NEWTON
POLISH = 2                       # PNP_POLISH
GN_ITERS = 3                     # PNP_GN_ITERS
PIVOT_RATIO = 1e-6               # ICP_PIVOT_RATIO
SMALL_ANGLE = 1e-8               # ICP_SMALL_ANGLE


def sample_ranks(seed, b, h, nv):
    """the 4 distinct ranks (among the valid rows, index order) of hypothesis h of pair b: slots 0 .. 2 solve, slot 3 picks"""
    return PO.sample_ranks(seed, b, h, nv, 4)


# ---- the restatement of csrc/rigid_math.h and csrc/pnp_math.h on float32 scalars ---------------------------------------------
def _v(x):
    return [F(t) for t in np.asarray(x, F).ravel()]


def rg_degenerate3_f32(p0, p1, p2):
    e1 = [p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]]
    e2 = [p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]]
    cx, cy, cz = e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]
    cc = (cx * cx + cy * cy) + cz * cz
    n1 = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2]
    n2 = (e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2]
    return not (cc > DEG * n1 * n2)


def rg_jacobi_f32(a, n):
    """rg_jacobi<n> in place on the list of lists a; returns v"""
    v = [[F(1) if r == c else F(0) for c in range(n)] for r in range(n)]
    for _ in range(JACOBI_SWEEPS):
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = a[p][q]
                if apq != F(0):
                    theta = (a[q][q] - a[p][p]) / (F(2) * apq)
                    t = (F(1) if theta >= F(0) else F(-1)) / (abs(theta) + np.sqrt(F(1) + theta * theta))
                    c = F(1) / np.sqrt(F(1) + t * t)
                    s = c * t
                    for k in range(n):
                        akp, akq = a[k][p], a[k][q]
                        a[k][p] = c * akp - s * akq
                        a[k][q] = s * akp + c * akq
                    for k in range(n):
                        apk, aqk = a[p][k], a[q][k]
                        a[p][k] = c * apk - s * aqk
                        a[q][k] = s * apk + c * aqk
                    a[p][q] = F(0)
                    a[q][p] = F(0)
                    for k in range(n):
                        vkp, vkq = v[k][p], v[k][q]
                        v[k][p] = c * vkp - s * vkq
                        v[k][q] = s * vkp + c * vkq
    return v


def rg_rotation_from_scatter_f32(s):
    n = [[F(0)] * 4 for _ in range(4)]
    n[0][0] = (s[0][0] + s[1][1]) + s[2][2]
    n[0][1] = s[1][2] - s[2][1]
    n[0][2] = s[2][0] - s[0][2]
    n[0][3] = s[0][1] - s[1][0]
    n[1][1] = (s[0][0] - s[1][1]) - s[2][2]
    n[1][2] = s[0][1] + s[1][0]
    n[1][3] = s[2][0] + s[0][2]
    n[2][2] = (s[1][1] - s[0][0]) - s[2][2]
    n[2][3] = s[1][2] + s[2][1]
    n[3][3] = (s[2][2] - s[0][0]) - s[1][1]
    for p in range(1, 4):
        for q in range(p):
            n[p][q] = n[q][p]
    n0 = [list(r) for r in n]
    v = rg_jacobi_f32(n, 4)
    m, best = 0, n[0][0]
    qq = [v[0][0], v[1][0], v[2][0], v[3][0]]
    for c in range(1, 4):
        if n[c][c] > best:
            best, m = n[c][c], c
            qq = [v[0][c], v[1][c], v[2][c], v[3][c]]
    qv = [D(x) for x in qq]
    w = [(((D(n0[k][0]) * qv[0] + D(n0[k][1]) * qv[1]) + D(n0[k][2]) * qv[2]) + D(n0[k][3]) * qv[3]) - D(best) * qv[k]
         for k in range(4)]
    d = [F(0)] * 4
    for j in range(4):
        dot = ((D(v[0][j]) * w[0] + D(v[1][j]) * w[1]) + D(v[2][j]) * w[2]) + D(v[3][j]) * w[3]
        den = best - n[j][j]
        coef = F(dot) / den if (j != m and den > F(0)) else F(0)
        for k in range(4):
            d[k] = d[k] + coef * v[k][j]
    q0, qx, qy, qz = qq[0] + d[0], qq[1] + d[1], qq[2] + d[2], qq[3] + d[3]
    nn = np.sqrt(((q0 * q0 + qx * qx) + qy * qy) + qz * qz)
    sg = F(-1) if q0 < F(0) else F(1)
    q0, qx, qy, qz = sg * q0 / nn, sg * qx / nn, sg * qy / nn, sg * qz / nn
    two = F(2)
    return [((q0 * q0 + qx * qx) - qy * qy) - qz * qz, two * (qx * qy - q0 * qz), two * (qx * qz + q0 * qy),
            two * (qy * qx + q0 * qz), ((q0 * q0 - qx * qx) + qy * qy) - qz * qz, two * (qy * qz - q0 * qx),
            two * (qz * qx - q0 * qy), two * (qz * qy + q0 * qx), ((q0 * q0 - qx * qx) - qy * qy) + qz * qz]


def rg_solve_minimal_f32(a, b):
    """rg_solve_minimal on rows a[k], b[k] (lists of 3 float32); None or the 12 values"""
    if rg_degenerate3_f32(a[0], a[1], a[2]) or rg_degenerate3_f32(b[0], b[1], b[2]):
        return None
    three = F(3)
    ca = [((a[0][j] + a[1][j]) + a[2][j]) / three for j in range(3)]
    cb = [((b[0][j] + b[1][j]) + b[2][j]) / three for j in range(3)]
    s = [[((a[0][i] - ca[i]) * (b[0][j] - cb[j]) + (a[1][i] - ca[i]) * (b[1][j] - cb[j])) + (a[2][i] - ca[i]) * (b[2][j] - cb[j])
          for j in range(3)] for i in range(3)]
    rt = rg_rotation_from_scatter_f32(s) + [F(0)] * 3
    chk = F(0)
    for j in range(3):
        rt[9 + j] = cb[j] - ((rt[3 * j] * ca[0] + rt[3 * j + 1] * ca[1]) + rt[3 * j + 2] * ca[2])
        chk = chk + (((abs(rt[3 * j]) + abs(rt[3 * j + 1])) + abs(rt[3 * j + 2])) + abs(rt[9 + j]))
    return rt if chk < INF32 else None


def _cof(m):
    return [m[3] * m[5] - m[4] * m[4], m[2] * m[4] - m[1] * m[5], m[1] * m[4] - m[2] * m[3], m[0] * m[5] - m[2] * m[2],
            m[1] * m[2] - m[0] * m[4], m[0] * m[3] - m[1] * m[1]]


def _sdot(c, b):
    return ((c[0] * b[0] + c[3] * b[3]) + c[5] * b[5]) + F(2) * ((c[1] * b[1] + c[2] * b[2]) + c[4] * b[4])


def pnp_setup_f32(X, uv):
    """pnp_setup: X three lists of 3 float32, uv three lists of 2; None or the dict of PnpSetup's fields"""
    if rg_degenerate3_f32(X[0], X[1], X[2]):
        return None
    one, two, three = F(1), F(2), F(3)
    f = []
    for k in range(3):
        nn = np.sqrt((uv[k][0] * uv[k][0] + uv[k][1] * uv[k][1]) + one)
        f.append([uv[k][0] / nn, uv[k][1] / nn, one / nn])
    if rg_degenerate3_f32(f[0], f[1], f[2]):
        return None

    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

    def dist2(a, b):
        d0, d1, d2 = a[0] - b[0], a[1] - b[1], a[2] - b[2]
        return (d0 * d0 + d1 * d1) + d2 * d2
    c12, c13, c23 = dot(f[0], f[1]), dot(f[0], f[2]), dot(f[1], f[2])
    a12, a13, a23 = dist2(X[0], X[1]), dist2(X[0], X[2]), dist2(X[1], X[2])
    d1 = [a23, -(a23 * c12), F(0), a23 - a12, a12 * c23, -a12]
    d2 = [a23, F(0), -(a23 * c13), -a13, a13 * c23, a23 - a13]
    k1, k2 = _cof(d1), _cof(d2)
    c0 = (d1[0] * k1[0] + d1[1] * k1[1]) + d1[2] * k1[2]
    c3 = (d2[0] * k2[0] + d2[1] * k2[1]) + d2[2] * k2[2]
    c1, c2 = _sdot(k1, d2), _sdot(k2, d1)
    b, c, d = c2 / c3, c1 / c3, c0 / c3
    bb = b * b - three * c
    if bb >= F(0):
        v = np.sqrt(bb)
        t1 = (-b - v) / three
        f1 = ((t1 + b) * t1 + c) * t1 + d
        if f1 > F(0):
            g = t1 - np.sqrt(-f1 / (three * t1 + b))
        else:
            t2 = (-b + v) / three
            f2 = ((t2 + b) * t2 + c) * t2 + d
            g = t2 + np.sqrt(-f2 / (three * t2 + b))
    else:
        g = -b / three
    for _ in range(CUBIC_NEWTON):
        fv, fp = ((g + b) * g + c) * g + d, (three * g + two * b) * g + c
        if fp != F(0):
            g = g - fv / fp
    a = [[F(0)] * 3 for _ in range(3)]
    a[0][0] = d1[0] + g * d2[0]
    a[0][1] = d1[1] + g * d2[1]
    a[0][2] = d1[2] + g * d2[2]
    a[1][1] = d1[3] + g * d2[3]
    a[1][2] = d1[4] + g * d2[4]
    a[2][2] = d1[5] + g * d2[5]
    a[1][0], a[2][0], a[2][1] = a[0][1], a[0][2], a[1][2]
    e = rg_jacobi_f32(a, 3)
    l0, l1, l2 = a[0][0], a[1][1], a[2][2]
    iz, lo = 0, abs(l0)
    if abs(l1) < lo:
        iz, lo = 1, abs(l1)
    if abs(l2) < lo:
        iz = 2
    lp, lq = (l1 if iz == 0 else l0), (l1 if iz == 2 else l2)
    ep = [e[k][1] if iz == 0 else e[k][0] for k in range(3)]
    eq = [e[k][1] if iz == 2 else e[k][2] for k in range(3)]
    if not (lp * lq < F(0)):
        return None
    swap = lp < F(0)
    sp, sq = np.sqrt(lq if swap else lp), np.sqrt(-lp if swap else -lq)
    return dict(f=f, c12=c12, c13=c13, c23=c23, a12=a12, a13=a13, a23=a23, g=g,
                np=[sp * (eq[k] if swap else ep[k]) for k in range(3)], nq=[sq * (ep[k] if swap else eq[k]) for k in range(3)])


def pnp_candidate_f32(X, S, c, polish=POLISH):
    """pnp_candidate: None or (depths [3], rt [12]); `polish` other than PNP_POLISH only for the constant's justification"""
    two, half = F(2), F(-0.5)
    a12, a13, a23, c12, c13, c23 = S["a12"], S["a13"], S["a23"], S["c12"], S["c13"], S["c23"]
    sg = F(-1) if (c & 2) else F(1)
    n0, n1, n2 = S["np"][0] + sg * S["nq"][0], S["np"][1] + sg * S["nq"][1], S["np"][2] + sg * S["nq"][2]
    w0, w1 = -n1 / n0, -n2 / n0
    qa = ((a13 - a12) * w1 * w1 + two * a12 * c13 * w1) - a12
    qb = (two * a12 * c13 * w0 - two * a13 * c12 * w1) - two * w0 * w1 * (a12 - a13)
    qc = ((a13 - a12) * w0 * w0 - two * a13 * c12 * w0) + a13
    disc = qb * qb - F(4) * qa * qc
    if not (disc >= F(0)):
        return None
    sd = np.sqrt(disc)
    qq = half * (qb + (sd if qb >= F(0) else -sd))
    tau = qc / qq if (c & 1) else qq / qa
    if not (tau > F(0)):
        return None
    l2 = np.sqrt(a23 / (tau * (tau - two * c23) + F(1)))
    l3 = tau * l2
    l1 = w0 * l2 + w1 * l3

    def usable():
        return (l1 > F(0) and l2 > F(0) and l3 > F(0)) and (l1 < INF32 and l2 < INF32 and l3 < INF32)
    if not usable():
        return None
    for _ in range(polish):
        r0 = ((l1 * l1 + l2 * l2) - two * c12 * l1 * l2) - a12
        r1 = ((l1 * l1 + l3 * l3) - two * c13 * l1 * l3) - a13
        r2 = ((l2 * l2 + l3 * l3) - two * c23 * l2 * l3) - a23
        j00, j01 = two * (l1 - c12 * l2), two * (l2 - c12 * l1)
        j10, j12 = two * (l1 - c13 * l3), two * (l3 - c13 * l1)
        j21, j22 = two * (l2 - c23 * l3), two * (l3 - c23 * l2)
        det = -(j00 * j12 * j21) - j01 * j10 * j22
        if det != F(0):
            n1_ = l1 - ((-(j12 * j21) * r0 - j01 * j22 * r1) + j01 * j12 * r2) / det
            n2_ = l2 - ((-(j10 * j22) * r0 + j00 * j22 * r1) - j00 * j12 * r2) / det
            n3_ = l3 - ((j10 * j21 * r0 - j00 * j21 * r1) - j01 * j10 * r2) / det
            l1, l2, l3 = n1_, n2_, n3_
    if not usable():
        return None
    l = [l1, l2, l3]
    rt = rg_solve_minimal_f32(X, [[l[k] * S["f"][k][j] for j in range(3)] for k in range(3)])
    return None if rt is None else (l, rt)


def pnp_dist2_f32(rt, X, uv):
    x = ((rt[0] * X[0] + rt[1] * X[1]) + rt[2] * X[2]) + rt[9]
    y = ((rt[3] * X[0] + rt[4] * X[1]) + rt[5] * X[2]) + rt[10]
    z = ((rt[6] * X[0] + rt[7] * X[1]) + rt[8] * X[2]) + rt[11]
    du, dv = x / z - uv[0], y / z - uv[1]
    d2 = du * du + dv * dv
    return d2 if (z > F(0) and d2 < INF32) else INF32


def pnp_solve_minimal_f32(X4, uv4, polish=POLISH):
    """pnp_solve_minimal on a 4-sample (arrays (4, 3), (4, 2)): (chosen rt or None, [(c, depths, rt, d2 on row 3)])"""
    with np.errstate(all="ignore"):
        X, uv = [_v(r) for r in np.asarray(X4)], [_v(r) for r in np.asarray(uv4)]
        S = pnp_setup_f32(X[:3], uv[:3])
        if S is None:
            return None, []
        cands, best, chosen = [], INF32, None
        for c in range(4):
            m = pnp_candidate_f32(X[:3], S, c, polish)
            if m is None:
                continue
            d2 = pnp_dist2_f32(m[1], X[3], uv[3])
            cands.append((c, m[0], m[1], d2))
            if chosen is None or d2 < best:
                best, chosen = d2, m[1]
        return chosen, cands


def pnp_lines_f32(rt, X, uv):
    """pnp_lines: (ok, ju [6], jv [6], ru, rv)"""
    with np.errstate(all="ignore"):
        rt, X, uv = _v(rt), _v(X), _v(uv)
        x = ((rt[0] * X[0] + rt[1] * X[1]) + rt[2] * X[2]) + rt[9]
        y = ((rt[3] * X[0] + rt[4] * X[1]) + rt[5] * X[2]) + rt[10]
        z = ((rt[6] * X[0] + rt[7] * X[1]) + rt[8] * X[2]) + rt[11]
        if not z > F(0):
            return False, [F(0)] * 6, [F(0)] * 6, F(0), F(0)
        xn, yn, iz, one = x / z, y / z, F(1) / z, F(1)
        return (True, [-(xn * yn), one + xn * xn, -yn, iz, F(0), -(xn * iz)], [-(one + yn * yn), xn * yn, xn, F(0), iz, -(yn * iz)],
                xn - uv[0], yn - uv[1])


# ---- the oracle --------------------------------------------------------------------------------------------------------------
def bearings(uv, dtype=D):
    h = np.concatenate([np.asarray(uv, dtype), np.ones((len(uv), 1), dtype)], axis=1)
    return h / np.sqrt((h * h).sum(axis=1, keepdims=True))


def _lawcos(l, c, a):
    r = np.array([l[0] ** 2 + l[1] ** 2 - 2 * c[0] * l[0] * l[1] - a[0], l[0] ** 2 + l[2] ** 2 - 2 * c[1] * l[0] * l[2] - a[1],
                  l[1] ** 2 + l[2] ** 2 - 2 * c[2] * l[1] * l[2] - a[2]])
    J = 2 * np.array([[l[0] - c[0] * l[1], l[1] - c[0] * l[0], 0], [l[0] - c[1] * l[2], 0, l[2] - c[1] * l[0]],
                      [0, l[1] - c[2] * l[2], l[2] - c[2] * l[1]]])
    return r, J


def p3p_depths(X, f):
    """every depth triple (l1, l2, l3), all positive, with |l_i f_i - l_j f_j| = |X_i - X_j|: Grunert's quartic"""
    X, f = np.asarray(X, D), np.asarray(f, D)
    c = (float(f[0] @ f[1]), float(f[0] @ f[2]), float(f[1] @ f[2]))                # Python floats: poly1d's operators
    a = (float(((X[0] - X[1]) ** 2).sum()), float(((X[0] - X[2]) ** 2).sum()), float(((X[1] - X[2]) ** 2).sum()))
    P = np.poly1d
    u = P([1.0, 0.0])
    A = P([1.0, -2 * c[0], 1.0])
    num = -((a[1] - a[2]) * A + a[0] * u * u - a[0])          # v = num / den from the difference of the two ratio equations
    den = P([-2 * a[0] * c[2], 2 * a[0] * c[1]])
    quartic = a[1] * A * den * den - a[0] * (den * den + num * num - 2 * c[1] * num * den)
    out = []
    with np.errstate(all="ignore"):
        for r in np.atleast_1d(quartic.roots):
            if abs(r.imag) > 1e-4 * (1 + abs(r.real)) or not r.real > 0:
                continue
            uu = r.real
            vv = num(uu) / den(uu)
            l1 = np.sqrt(a[0] / A(uu))
            l = np.array([l1, uu * l1, vv * l1])
            if not np.isfinite(l).all():
                continue
            for _ in range(5):
                res, J = _lawcos(l, c, a)
                try:
                    l = l - np.linalg.solve(J, res)
                except np.linalg.LinAlgError:
                    break
            res, _ = _lawcos(l, c, a)
            if not (np.isfinite(l).all() and (l > 0).all() and np.abs(res).max() < 1e-9 * max(a)):
                continue
            if any(np.abs(l - o).max() < 1e-7 * np.abs(l).max() for o in out):
                continue
            out.append(l)
    return out


def dist2(R, t, X, uv):
    """the header's reprojection d^2 per row in R's dtype; +inf for z <= 0 or a non-finite value"""
    dt = R.dtype.type
    with np.errstate(all="ignore"):
        p = X.astype(R.dtype) @ R.T + t
        du, dv = p[:, 0] / p[:, 2] - uv[:, 0].astype(R.dtype), p[:, 1] / p[:, 2] - uv[:, 1].astype(R.dtype)
        d2 = (du * du + dv * dv).astype(R.dtype)
    return np.where((p[:, 2] > 0) & np.isfinite(d2), d2, dt(np.inf)).astype(R.dtype)


def solve_minimal(X4, uv4):
    """the float64 oracle on a 4-sample: (R, t) or None, and every candidate [(depths, R, t)]"""
    X, uv = np.asarray(X4, D), np.asarray(uv4, D)
    f = bearings(uv[:3])
    if RO.degenerate3(X[:3]) or RO.degenerate3(f):
        return None, []
    cands, best, chosen = [], np.inf, None
    for l in p3p_depths(X[:3], f):
        m = RO.solve_minimal(X[:3], l[:, None] * f, D)
        if m is None:
            continue
        cands.append((l, m[0], m[1]))
        d2 = dist2(m[0], m[1], X[3:4], uv[3:4])[0]
        if chosen is None or d2 < best:
            best, chosen = d2, m
    return chosen, cands


def score(R, t, X, uv, thr):
    d2 = dist2(R, t, X, uv)
    t2 = R.dtype.type(thr) * R.dtype.type(thr)
    return R.dtype.type(np.minimum(d2, t2).sum(dtype=R.dtype)), int((d2 <= t2).sum()), d2


def hypotheses(X, uv, valid, num_hyp, thr, seed, b=0, dtype=D):
    """one pair: (rt_h (H, 12), cost (H,), count (H,), ranks (H, 4)).  dtype float64: the oracle; float32: the restatement
    of the kernel's solver and a float32 score"""
    sel = np.arange(len(X)) if valid is None else np.flatnonzero(valid)
    q3, q2 = X[sel].astype(dtype), uv[sel].astype(dtype)
    nv = len(sel)
    rt_h = np.zeros((num_hyp, 12), dtype)
    cost = np.full(num_hyp, np.inf, dtype)
    count = np.zeros(num_hyp, np.int32)
    ranks = np.zeros((num_hyp, 4), np.int64)
    if nv < 4:
        return rt_h, cost, count, ranks
    for h in range(num_hyp):
        ranks[h] = sample_ranks(seed, b, h, nv)
        if dtype == D:
            m, _ = solve_minimal(q3[ranks[h]], q2[ranks[h]])
            rt = None if m is None else np.concatenate([m[0].ravel(), m[1]])
        else:
            rt, _ = pnp_solve_minimal_f32(q3[ranks[h]], q2[ranks[h]])
            rt = None if rt is None else np.array(rt, F)
        if rt is None:
            continue
        c, k, _ = score(rt[:9].reshape(3, 3), rt[9:], q3, q2, thr)
        if np.isfinite(c):
            rt_h[h], cost[h], count[h] = rt, c, k
    return rt_h, cost, count, ranks


def _ldl_solve(A, b):
    """icp_solve: A x = -b by LDL^T without pivoting; None when a pivot is not above PIVOT_RATIO max diag(A)"""
    n = 6
    L, dg = np.eye(n), np.zeros(n)
    dmax = A.diagonal().max()
    if not (np.isfinite(A).all() and np.isfinite(b).all() and dmax > 0):
        return None
    for j in range(n):
        d = A[j, j] - (L[j, :j] ** 2 * dg[:j]).sum()
        dg[j] = d
        if not d > PIVOT_RATIO * dmax:
            return None
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j] * dg[:j]).sum()) / d
    y = np.linalg.solve(L, -b)
    x = np.linalg.solve(L.T, y / dg)
    return x if np.isfinite(x).all() else None


def _exp(w):
    th = np.sqrt(w @ w)
    kx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < SMALL_ANGLE:
        return np.eye(3) + kx
    return np.eye(3) + np.sin(th) / th * kx + (1 - np.cos(th)) / (th * th) * (kx @ kx)


def linearise(R, t, X, uv, dtype=D):
    """(A (6, 6), b (6,), sum r^2, rows used) of the reprojection system at (R, t) over the rows X, uv, summed in dtype"""
    Rd, td = R.astype(dtype), t.astype(dtype)
    with np.errstate(all="ignore"):
        p = X.astype(dtype) @ Rd.T + td
        use = p[:, 2] > 0
        p, q = p[use], uv[use].astype(dtype)
        xn, yn, iz = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2], dtype(1) / p[:, 2]
        z0 = np.zeros_like(xn)
        ju = np.stack([-(xn * yn), 1 + xn * xn, -yn, iz, z0, -(xn * iz)], axis=1).astype(dtype)
        jv = np.stack([-(1 + yn * yn), xn * yn, xn, z0, iz, -(yn * iz)], axis=1).astype(dtype)
        ru, rv = xn - q[:, 0], yn - q[:, 1]
        A = ((ju[:, :, None] * ju[:, None, :]).sum(axis=0, dtype=dtype) + (jv[:, :, None] * jv[:, None, :]).sum(axis=0, dtype=dtype))
        bb = (ju * ru[:, None]).sum(axis=0, dtype=dtype) + (jv * rv[:, None]).sum(axis=0, dtype=dtype)
        rr = (ru * ru).sum(dtype=dtype) + (rv * rv).sum(dtype=dtype)
    return A.astype(D), bb.astype(D), float(rr), int(use.sum())


def refit(X, uv, mask, R0, t0, dtype=D, iters=GN_ITERS):
    """mi_pnp_refit, one pair: (R, t, info (6, 6), ok).  The rows and sums in `dtype`, the solve and the pose in float64;
    iters + 1 linearisations, every one of which must be usable; the last one's A is info and its step is not applied"""
    sel = np.flatnonzero(mask)
    Xs, us = X[sel], uv[sel]
    R, t = np.asarray(R0, D).copy(), np.asarray(t0, D).copy()
    fail = (np.asarray(R0, dtype), np.asarray(t0, dtype), np.zeros((6, 6), dtype), False)
    for it in range(iters + 1):
        A, b, _, m = linearise(R.astype(dtype), t.astype(dtype), Xs, us, dtype)
        x = _ldl_solve(A, b) if m >= 4 else None
        if x is None:
            return fail
        if it == iters:
            return R.astype(dtype), t.astype(dtype), A.astype(dtype), True
        E = _exp(x[:3])
        R, t = E @ R, E @ t + x[3:]


def ransac(X, uv, valid, num_hyp, thr, rounds, seed, b=0, dtype=D):
    """mi_pnp_ransac, one pair: (R, t, inlier (n,) bool, best_h, count, rmse, info, ok); costs inside the refinement as
    (valid rows beyond the threshold) thr^2 + the inliers' sum of d^2 in float64, the header's rule"""
    n = len(X)
    vmask = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    rt_h, cost, _, _ = hypotheses(X, uv, valid, num_hyp, thr, seed, b, dtype)
    best_h = int(np.argmin(cost)) if np.isfinite(cost).any() else 0
    fail = (np.eye(3, dtype=dtype), np.zeros(3, dtype), np.zeros(n, bool), best_h, 0, dtype(0), np.zeros((6, 6), dtype), False)
    if not np.isfinite(cost[best_h]):
        return fail
    q3, q2 = np.where(vmask[:, None], X, 0).astype(dtype), np.where(vmask[:, None], uv, 0).astype(dtype)
    R, t = rt_h[best_h, :9].reshape(3, 3), rt_h[best_h, 9:]
    t2 = dtype(thr) * dtype(thr)

    def step_cost(Rc, tc):
        d2 = dist2(Rc, tc, q3[vmask], q2[vmask])
        inl = d2 <= t2
        return float(int((~inl).sum())) * float(t2) + float(d2[inl].sum(dtype=dtype))
    cur = step_cost(R, t)
    for r in range(rounds):
        kr = dtype(1.0 + 0.5 * (rounds - 1 - r))
        d2 = dist2(R, t, q3, q2)
        R2, tt2, _, ok = refit(q3, q2, vmask & (d2 <= (kr * dtype(thr)) * (kr * dtype(thr))), R, t, dtype)
        if not ok:
            continue
        c2 = step_cost(R2, tt2)
        if c2 < cur:
            R, t, cur = R2, tt2, c2
    d2 = dist2(R, t, q3, q2)
    inlier = vmask & (d2 <= t2)
    cnt = int(inlier.sum())
    if cnt < 4:
        return fail
    info = linearise(R, t, q3[inlier], q2[inlier], dtype)[0].astype(dtype)
    return R, t, inlier, best_h, cnt, dtype(np.sqrt(d2[inlier].sum(dtype=dtype) / dtype(cnt))), info, True


# ---- the scenes the host and GPU tests share --------------------------------------------------------------------------------
THR_PX = 2.0                     # AbsolutePoseEstimator's default ransac_threshold


def scenes(seeds, n, outliers, noise_px):
    """a batch of synth_rgbd_pair scenes as 3-D to 2-D problems: frame 1 lifted through its depth by mi_lift_keypoints'
    float32 arithmetic -> pts3 (B, n, 3) float32; frame 2's pixels normalised -> pts2 (B, n, 2) float32 (x, y); the lists of
    R and t with X2 = R X1 + t; the planted inlier masks (B, n); the threshold THR_PX in normalised units.  Frame 1's depth
    carries no noise, its pixels and frame 2's N(0, noise_px^2)."""
    from onnx_image_processing_amd.synth import rgbd_camera, synth_rgbd_pair
    K = rgbd_camera()
    ki = np.linalg.inv(K).astype(F)
    p3, p2, Rs, ts, inl = [], [], [], [], []
    for seed in seeds:
        k1, k2, d1, _, R, t, m = synth_rgbd_pair(seed, n, outliers, noise_px, 0.0)
        x1, v1 = RO.lift_f32(k1, d1, ki, 1.0, RO.MIN_DEPTH, RO.MAX_DEPTH)
        assert v1.all()
        p3.append(x1)
        p2.append(normalise_f32(k2, ki))
        Rs.append(R)
        ts.append(t)
        inl.append(m)
    return np.stack(p3), np.stack(p2), Rs, ts, np.stack(inl), THR_PX / ((K[0, 0] + K[1, 1]) / 2)


def normalise_f32(kp_yx, k_inv):
    """mi_normalise_keypoints in its float32 arithmetic: pixel (y, x) -> normalised (x, y)"""
    kp, ki = np.asarray(kp_yx, F), np.asarray(k_inv, F).ravel()
    y, x = kp[..., 0], kp[..., 1]
    return np.stack([(x * ki[0] + y * ki[1]) + ki[2], (x * ki[3] + y * ki[4]) + ki[5]], axis=-1).astype(F)


def has_all_inlier_sample(seed, b, num_hyp, valid, inlier):
    """some hypothesis h < num_hyp of pair b draws its 4 rows among the planted inliers"""
    sel = np.flatnonzero(valid)
    return any(inlier[sel[sample_ranks(seed, b, h, len(sel))]].all() for h in range(num_hyp))
