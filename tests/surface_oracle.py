"""numpy restatement of K20, TSDF surface extraction (include/mi355x_match.h, "TSDF surface extraction"): marching tetrahedra
over the Kuhn split of every cell of a K19 volume -> vertices, normals, triangles and the counts.

`extract` takes `dtype` as tsdf_oracle.py's functions do: np.float64 is the oracle; np.float32 is the header's arithmetic
operation by operation (numpy fuses nothing), i.e. the kernels' bits.  The triangle table is generated here from the header's
orientation rule; csrc/surface_math.h generates its own and tests/test_surface_host.py compares the two entry for entry.

A volume is tsdf_oracle's pair (tsdf, weight) of (nz, ny, nx) arrays, a grid its (origin (3,), voxel_size, truncation)."""
import functools

import numpy as np

import tsdf_oracle as TO

F32, F64 = np.float32, np.float64
TETS = ((0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7))
EDGE_POS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))          # a tetrahedron's edges as pairs of path positions


def corner(m):
    """the offset (dx, dy, dz) of corner m"""
    return np.array([m & 1, (m >> 1) & 1, (m >> 2) & 1])


def _oriented(t, case, tri):
    """tri: three edges (pairs of path positions) -> the same with the last two swapped unless the normal of the midpoints'
    triangle points from the inside corners' mean towards the outside corners' mean"""
    pts = np.array([corner(m) for m in TETS[t]], F64)
    inside = np.array([(case >> s) & 1 for s in range(4)], bool)
    v = [(pts[a] + pts[b]) / 2 for a, b in tri]
    n = np.cross(v[1] - v[0], v[2] - v[0])
    d = pts[~inside].mean(0) - pts[inside].mean(0)
    assert abs(n @ d) > 1e-9
    return tuple(tri) if n @ d > 0 else (tri[0], tri[2], tri[1])


@functools.lru_cache(maxsize=None)
def triangle_table():
    """table[t][case] = a tuple of 0, 1 or 2 triangles, each three edges, each edge a pair (a, b) of path positions, a < b"""
    def edge(a, b):
        return (min(a, b), max(a, b))
    table = []
    for t in range(6):
        row = []
        for case in range(16):
            ins = [s for s in range(4) if (case >> s) & 1]
            out = [s for s in range(4) if not (case >> s) & 1]
            if len(ins) in (1, 3):
                s = ins[0] if len(ins) == 1 else out[0]
                others = out if len(ins) == 1 else ins
                tris = [tuple(edge(s, u) for u in others)]
            elif len(ins) == 2:
                (A, B), (C, D) = ins, out
                tris = [(edge(A, C), edge(A, D), edge(B, D)), (edge(A, C), edge(B, D), edge(B, C))]
            else:
                tris = []
            row.append(tuple(_oriented(t, case, tri) for tri in tris))
        table.append(tuple(row))
    return tuple(table)


def packed_table():
    """the table in csrc/surface_math.h's encoding, (6, 16) uint32: the count in bits 0-1, then 3 bits per vertex (an index
    into EDGE_POS), triangle n's vertex v at bit 2 + 3 (3 n + v)"""
    out = np.zeros((6, 16), np.uint32)
    for t, row in enumerate(triangle_table()):
        for case, tris in enumerate(row):
            e = len(tris)
            for n, tri in enumerate(tris):
                for v, pair in enumerate(tri):
                    e |= EDGE_POS.index(pair) << (2 + 3 * (3 * n + v))
            out[t, case] = e
    return out


def classify(volume, min_weight=1.0):
    """-> (observed, inside), bool (nz, ny, nx).  min_weight is rounded to float32 as the C ABI receives it; the weights of the
    tests are small integers, exact in both types"""
    tsdf, weight = volume
    obs = weight >= weight.dtype.type(F32(min_weight))
    with np.errstate(invalid="ignore"):
        return obs, obs & ~(tsdf > 0)


def edge_masks(obs, ins):
    """exists (nz, ny, nx, 8) bool: [..., e] iff the edge of class e owned by the voxel carries a vertex ([..., 0] is never set)"""
    nz, ny, nx = obs.shape
    exists = np.zeros((nz, ny, nx, 8), bool)
    for e in range(1, 8):
        dx, dy, dz = corner(e)
        p = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        q = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        exists[p + (e,)] = obs[p] & obs[q] & (ins[p] ^ ins[q])
    return exists


def extract(volume, grid, min_weight=1.0, dtype=F64, normals=True):
    """-> dict(vertices (V, 3), normals (V, 3), normal_ok (V,) bool, triangles (T, 3) int32, counts (V, T), owner (V, 4) int =
    (i, j, k, e) of every vertex, alpha (V,))"""
    T = dtype
    tsdf, weight = (x.astype(T) for x in volume)
    nz, ny, nx = tsdf.shape
    origin, vs, _ = grid
    vs_t = T(F32(vs))
    obs, ins = classify((tsdf, weight), min_weight)
    exists = edge_masks(obs, ins)
    # ---- vertices: ids in the order (owner's linear index, class) = C order of `exists`
    vid = np.full(exists.shape, -1, np.int64)
    vid[exists] = np.arange(int(exists.sum()))
    k, j, i, e = np.nonzero(exists)
    dx, dy, dz = e & 1, (e >> 1) & 1, (e >> 2) & 1
    f_p, f_q = tsdf[k, j, i], tsdf[k + dz, j + dy, i + dx]
    with np.errstate(invalid="ignore", divide="ignore"):
        a = (f_p / (f_p - f_q)).astype(T)
    cen = TO.centres((nx, ny, nz), grid, T)
    pos, g = [], []
    for idx, d, c in ((i, dx, cen[0]), (j, dy, cen[1]), (k, dz, cen[2])):
        pos.append(np.where(d == 1, c[idx] + a * vs_t, c[idx]).astype(T))
        g.append(np.where(d == 1, idx.astype(T) + a, idx.astype(T)).astype(T))
    vertices, g = np.stack(pos, -1).reshape(-1, 3), np.stack(g, -1).reshape(-1, 3)
    nrm, nok = np.zeros_like(vertices), np.zeros(len(vertices), bool)
    if normals and len(vertices):
        grad, nok = [], np.ones(len(vertices), bool)
        for ax in range(3):
            hi, lo = g.copy(), g.copy()
            hi[:, ax] = g[:, ax] + T(1)
            lo[:, ax] = g[:, ax] - T(1)
            fh, okh = TO.sample((tsdf, weight), hi, T)
            fl, okl = TO.sample((tsdf, weight), lo, T)
            nok &= okh & okl
            grad.append(fh - fl)
        with np.errstate(invalid="ignore", over="ignore"):
            length = np.sqrt((grad[0] * grad[0] + grad[1] * grad[1]) + grad[2] * grad[2]).astype(T)
            nok &= (length > 0) & np.isfinite(length)
        with np.errstate(invalid="ignore", divide="ignore"):
            nrm = np.where(nok[:, None], np.stack(grad, -1) / length[:, None], T(0)).astype(T)
    # ---- triangles
    table = triangle_table()
    cz, cy, cx = nz - 1, ny - 1, nx - 1

    def at(arr, m):
        ox, oy, oz = corner(m)
        return arr[oz:oz + cz, oy:oy + cy, ox:ox + cx]
    cell_lin = np.arange(cz * cy * cx).reshape(cz, cy, cx)
    keys, tris = [], []
    for t, path in enumerate(TETS):
        ok = at(obs, path[0]) & at(obs, path[1]) & at(obs, path[2]) & at(obs, path[3])
        case = sum(at(ins, path[s]).astype(np.int64) << s for s in range(4))
        for c in range(1, 15):
            sel = ok & (case == c)
            if not sel.any():
                continue
            ck, cj, ci = np.nonzero(sel)
            for n, tri in enumerate(table[t][c]):
                ids = []
                for sa, sb in tri:
                    p, q = path[sa], path[sb]
                    ox, oy, oz = corner(p)
                    ids.append(vid[ck + oz, cj + oy, ci + ox, q - p])
                tris.append(np.stack(ids, -1))
                keys.append((cell_lin[ck, cj, ci] * 6 + t) * 2 + n)
    if tris:
        keys, tris = np.concatenate(keys), np.concatenate(tris)
        triangles = tris[np.argsort(keys, kind="stable")]
    else:
        triangles = np.zeros((0, 3), np.int64)
    assert (triangles >= 0).all()
    return dict(vertices=vertices, normals=nrm, normal_ok=nok, triangles=triangles.astype(np.int32),
                counts=(len(vertices), len(triangles)), owner=np.stack([i, j, k, e], -1), alpha=a)


def sphere_volume(n=20, centre=(9.3, 9.7, 10.1), radius=6.2, dtype=F64):
    """clip((|x - c| - r) / 3, -1, 1) at the voxel indices of an n^3 grid, weight 1 everywhere -> (tsdf, weight)"""
    z, y, x = np.meshgrid(*(np.arange(n, dtype=F64),) * 3, indexing="ij")
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
    return np.clip((d - radius) / 3.0, -1.0, 1.0).astype(dtype), np.ones((n, n, n), dtype)


PLANE_GRID = (np.array([-1.3, 0.4, 2.0], F32), 0.07, 0.28)


def plane_volume(dtype=F64):
    """a 130 x 3 x 3 volume (nx, ny, nz) holding a slanted plane that crosses every x, so that every 64-voxel chunk of a row
    owns vertices (two carries per row), at the smallest ny, nz that have cells; a few voxels unobserved -> (tsdf, weight)"""
    z, y, x = np.meshgrid(np.arange(3, dtype=F64), np.arange(3, dtype=F64), np.arange(130, dtype=F64), indexing="ij")
    tsdf = np.clip((0.011 * x + 1.0 * y + 0.7 * z - 1.9) / 2.0, -1.0, 1.0).astype(F32)
    weight = np.ones((3, 3, 130), F32)
    weight[1, 1, 40:45] = 0
    weight[:, :, 100] = 0
    weight[0, 2, 63:66] = 0
    return tsdf.astype(dtype), weight.astype(dtype)


UNIT_GRID =(np.array([-0.5, -0.5, -0.5], F32), 1.0, 3.0)      # voxel centres at the integers: world = grid coordinates


def mesh_topology(vertices, triangles):
    """-> dict(closed: every directed edge once and its reverse once, euler: V - E + F, used: every vertex in a triangle,
    degenerate: triangles of zero area)"""
    tri = np.asarray(triangles, np.int64)
    de = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    code = de[:, 0] * (len(vertices) + 1) + de[:, 1]
    rev = de[:, 1] * (len(vertices) + 1) + de[:, 0]
    uniq, cnt = np.unique(code, return_counts=True)
    closed = bool((cnt == 1).all()) and np.array_equal(uniq, np.unique(rev)) and not (de[:, 0] == de[:, 1]).any()
    und = np.unique(np.sort(de, axis=1), axis=0)
    v = np.asarray(vertices, F64)
    area2 = np.linalg.norm(np.cross(v[tri[:, 1]] - v[tri[:, 0]], v[tri[:, 2]] - v[tri[:, 0]]), axis=1)
    return dict(closed=closed, euler=len(vertices) - len(und) + len(tri), used=len(np.unique(tri)) == len(vertices),
                degenerate=int((area2 == 0).sum()))
