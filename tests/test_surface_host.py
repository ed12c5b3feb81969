"""K20 TSDF surface extraction without a GPU: the numpy oracle's own sanity (tests/surface_oracle.py), the kernels' arithmetic
and compile-time triangle table (csrc/surface_math.h) compiled as plain C++ in tests/native/surface_host.cpp, the host-side
argument checks of `mi_tsdf_surface` (MI_E_* before any launch), the workspace size and the Python layer's refusals.

Bounds.  The table is compared entry for entry; a, the vertex and the normal are float32 in the header's order, which the
oracle's float32 run reproduces operation by operation: compared bit for bit.
The oracle's own sanity (float64): on the analytic sphere clip((|x - c| - r) / 3, -1, 1) over 20^3 voxels, c = (9.3, 9.7, 10.1),
r = 6.2, the mesh has 2168 vertices and 4332 triangles, is closed, consistently oriented outwards, of Euler characteristic 2,
uses every vertex, and its vertices lie within 6.0128e-2 voxel of the sphere (linear interpolation of a distance clipped at
3 voxels).  With c = (10, 10, 10), r = 6, which puts nodes at exactly 0: 2042 vertices, 4080 triangles, 420 of them of zero
area, still closed and of Euler characteristic 2.  On the fused rooms the float32 and float64 runs give the counts of COUNTS
and identical triangles: a condition on the scenes, not a tolerance."""
import ctypes

import numpy as np
import pytest
import torch

import surface_oracle as SO
import tsdf_oracle as TO
from helpers import host_program, run_host, run_records
from onnx_image_processing_amd import _native as N

NULL, SHAPE, PARAM, CAPACITY, ALIGN = -1, -2, -3, -4, -5
F32, F64 = np.float32, np.float64
NAN, INF = float("nan"), float("inf")
SPHERE_DISTANCE = 6.0128e-2                                          # voxels, float64 oracle against the analytic sphere
COUNTS = {("room", (37, 53)): (9232, 17732), ("room", (48, 64)): (9716, 18708), ("odd", (37, 53)): (6659, 12744),
          ("odd", (48, 64)): (6876, 13192), ("tiny", (37, 53)): (9, 8), ("tiny", (48, 64)): (9, 8)}
SPECS = {"room": TO.ROOM, "odd": TO.ODD, "tiny": TO.TINY}


# ---- the oracle's own sanity --------------------------------------------------------------------------------------------------------

def test_oracle_table_follows_the_rule():
    table = SO.triangle_table()
    assert len(table) == 6 and all(len(row) == 16 for row in table)
    for t, row in enumerate(table):
        assert row[0] == () and row[15] == ()
        for case, tris in enumerate(row):
            n_in = bin(case).count("1")
            assert len(tris) == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[n_in]
            for tri in tris:                                          # every edge joins an inside and an outside position
                assert len(set(tri)) == 3 and all(((case >> a) & 1) != ((case >> b) & 1) and a < b for a, b in tri)
            assert sorted(map(sorted, tris)) == sorted(map(sorted, table[t][15 - case]))       # the complement: the same edges
    packed = SO.packed_table()
    assert packed.shape == (6, 16) and (packed[:, [0, 15]] == 0).all() and ((packed & 3) == [[0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0]]).all()


def _outward(mesh, centre):
    v, t = mesh["vertices"].astype(F64), mesh["triangles"]
    n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    return (n * (v[t].mean(1) - np.asarray(centre, F64))).sum(1)


def test_oracle_sphere_is_a_closed_outward_manifold():
    c, r = (9.3, 9.7, 10.1), 6.2
    mesh = SO.extract(SO.sphere_volume(20, c, r), SO.UNIT_GRID)
    topo = SO.mesh_topology(mesh["vertices"], mesh["triangles"])
    dist = float(np.abs(np.linalg.norm(mesh["vertices"] - np.array(c), axis=1) - r).max())
    print(f"sphere: counts {mesh['counts']}, {topo}, vertices within {dist:.4e} voxel of the sphere")
    assert mesh["counts"] == (2168, 4332)
    assert topo == dict(closed=True, euler=2, used=True, degenerate=0)
    assert (_outward(mesh, c) > 0).all()
    assert dist <= SPHERE_DISTANCE * 1.001
    assert mesh["normal_ok"].all() and np.abs(np.linalg.norm(mesh["normals"], axis=1) - 1).max() < 1e-12
    assert ((mesh["normals"] * (mesh["vertices"] - np.array(c))).sum(1) > 0).all()              # towards the positive side
    assert (mesh["alpha"] >= 0).all() and (mesh["alpha"] <= 1).all()
    # the float32 run: the same topology
    m32 = SO.extract(SO.sphere_volume(20, c, r, F32), SO.UNIT_GRID, dtype=F32)
    assert m32["vertices"].dtype == F32 and np.array_equal(m32["triangles"], mesh["triangles"])


def test_oracle_sphere_with_nodes_at_zero_stays_closed():
    c, r = (10.0, 10.0, 10.0), 6.0
    vol = SO.sphere_volume(20, c, r)
    assert (vol[0] == 0).sum() > 0
    mesh = SO.extract(vol, SO.UNIT_GRID)
    topo = SO.mesh_topology(mesh["vertices"], mesh["triangles"])
    print(f"sphere through nodes: counts {mesh['counts']}, {topo}")
    assert mesh["counts"] == (2042, 4080)
    assert topo == dict(closed=True, euler=2, used=True, degenerate=420)
    assert (_outward(mesh, c) >= 0).all()
    assert set(np.unique(mesh["alpha"][(mesh["alpha"] == 0) | (mesh["alpha"] == 1)])) == {0.0, 1.0}


@pytest.mark.parametrize("h,w", [(37, 53), (48, 64)])
@pytest.mark.parametrize("name", ["room", "odd", "tiny"])
def test_oracle_float32_and_float64_agree_on_the_fused_rooms(name, h, w):
    _, grid = TO.grid_of(SPECS[name])
    m64 = SO.extract(TO.fused_room(h, w, SPECS[name], F64), grid)
    m32 = SO.extract(TO.fused_room(h, w, SPECS[name], F32), grid, dtype=F32)
    print(f"{name} {h} x {w}: counts {m64['counts']}, vertex {np.abs(m32['vertices'] - m64['vertices']).max():.4e}, normal "
          f"{np.abs(m32['normals'] - m64['normals']).max():.4e}, normals on {m64['normal_ok'].mean():.3f} of the vertices")
    assert m64["counts"] == m32["counts"] == COUNTS[name, (h, w)]
    assert np.array_equal(m64["triangles"], m32["triangles"]) and np.array_equal(m64["owner"], m32["owner"])
    assert np.array_equal(m64["normal_ok"], m32["normal_ok"]) and m64["normal_ok"].any() == (name != "tiny")
    assert len(np.unique(m64["triangles"])) <= m64["counts"][0] and m64["triangles"].max() < m64["counts"][0]
    # a larger min_weight observes less
    m2 = SO.extract(TO.fused_room(h, w, SPECS[name], F64), grid, min_weight=2.0)
    assert m2["counts"][0] < m64["counts"][0] or name == "tiny"


# ---- the kernels' arithmetic on the host ----------------------------------------------------------------------------------------

# tests/native/surface_host.cpp around csrc/surface_math.h, compiled as plain C++ (no HIP)
surface_host = host_program("surface_host.cpp", hip=False)


def test_native_table_is_the_oracles(surface_host):
    rows = np.array(run_host(surface_host, "table"), np.int64)
    assert rows.shape == (96, 3) and np.array_equal(rows[:, 0], np.repeat(np.arange(6), 16)) and np.array_equal(rows[:, 1], np.tile(np.arange(16), 6))
    assert np.array_equal(rows[:, 2].reshape(6, 16), SO.packed_table().astype(np.int64))


def test_native_bits_and_cells_are_the_oracles(surface_host):
    recs = [[t, w, mw] for t in (-1.0, -0.0, 0.0, 1e-30, 1.0, NAN) for w in (0.0, 0.5, 1.0, 2.0, NAN) for mw in (0.5, 1.0, 2.0)]
    out = np.array(run_records(surface_host, "bits", recs))[:, 0]
    for (t, w, mw), got in zip(recs, out):
        obs = w >= mw
        assert got == (1 if obs else 0) + (2 if obs and not t > 0 else 0), (t, w, mw)
    # every (observed, inside) pair of a cell's eight corners, inside implying observed
    pairs = [(o, n) for o in range(256) for n in range(256) if n & ~o == 0]
    out = np.array(run_records(surface_host, "cell", pairs)).astype(np.int64)
    table = SO.triangle_table()
    for (o, n), got in zip(pairs, out):
        edges = sum(1 << e for e in range(1, 8) if (o & 1) and (o >> e) & 1 and ((n & 1) != ((n >> e) & 1)))
        cases = [sum(((n >> m) & 1) << s for s, m in enumerate(path)) for path in SO.TETS]
        tris = sum(len(table[t][cases[t]]) for t, path in enumerate(SO.TETS) if all((o >> m) & 1 for m in path))
        assert got.tolist() == [edges, tris, *cases], (o, n)


def test_native_vertex_and_normal_are_the_float32_oracles(surface_host, tmp_path):
    h, w = 37, 53
    for name in ("odd", "tiny", "sphere"):
        if name == "sphere":
            vol, grid = SO.sphere_volume(20, (10.0, 10.0, 10.0), 6.0, F32), SO.UNIT_GRID              # nodes at exactly 0
        else:
            vol, grid = TO.fused_room(h, w, SPECS[name], F32), TO.grid_of(SPECS[name])[1]
        nz, ny, nx = vol[0].shape
        path = str(tmp_path / "volume.bin")
        np.stack(vol, axis=-1).astype(F32).tofile(path)
        mesh = SO.extract(vol, grid, dtype=F32)
        assert mesh["counts"][0] > 0
        out = np.array(run_records(surface_host, ["vertex", path, str(nx), str(ny), str(nz)], [[*o, *grid[0], grid[1]] for o in mesh["owner"]]))
        assert np.array_equal(out[:, 0].astype(F32).view(np.uint32), mesh["alpha"].view(np.uint32))
        assert np.array_equal(out[:, 1:4].astype(F32).view(np.uint32), mesh["vertices"].view(np.uint32))
        assert np.array_equal(out[:, 4].astype(bool), mesh["normal_ok"])
        assert np.array_equal(out[:, 5:8].astype(F32).view(np.uint32), mesh["normals"].view(np.uint32))
        assert mesh["normal_ok"].any() == (name != "tiny")


# ---- argument checks ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    return N.load()


p_keepalive = []


@pytest.fixture(scope="module")
def p():
    buf = ctypes.create_string_buffer(1 << 16)
    p_keepalive.append(buf)
    return (ctypes.addressof(buf) + 255) & ~255          # 256-byte aligned fake "device" pointer: never dereferenced by a refused call


def test_surface_argument_checks(lib, p):
    f = lib.mi_tsdf_surface
    big = 1 << 40

    def call(**kw):
        a = dict(vol=p, batch=2, nz=56, ny=44, nx=72, o=(-2.25, -1.75, 0.5), vs=0.0625, mw=1.0, mv=1000, mt=2000, v=p, n=p, t=p, c=p,
                 ws=p, wb=big)
        a.update(kw)
        return f(a["vol"], a["batch"], a["nz"], a["ny"], a["nx"], *a["o"], a["vs"], a["mw"], a["mv"], a["mt"], a["v"], a["n"], a["t"],
                 a["c"], a["ws"], a["wb"], None)
    # NULL
    assert call(vol=None) == NULL and call(c=None) == NULL and call(ws=None) == NULL
    assert call(v=None) == NULL and call(t=None) == NULL and call(v=None, mv=0, t=None) == NULL
    # K19's volume checks, ids that fit int32, capacities that fit
    assert call(batch=0) == SHAPE and call(nz=1) == SHAPE and call(ny=1) == SHAPE and call(nx=1) == SHAPE and call(nx=-3) == SHAPE
    assert call(batch=2, nz=1024, ny=1024, nx=1024) == SHAPE and call(batch=8, nz=512, ny=512, nx=1024) == SHAPE
    assert call(batch=65535, nz=32, ny=32, nx=33) == SHAPE and call(batch=65536, nz=2, ny=2, nx=2) == PARAM
    assert call(batch=1, nz=512, ny=512, nx=683) == SHAPE                             # 12 * voxels >= 2^31: ids leave int32
    assert call(batch=1, nz=512, ny=512, nx=682, wb=0) == CAPACITY                    # the largest that fits: refused for the workspace only
    assert call(batch=3, mv=1 << 30) == SHAPE and call(batch=3, mt=1 << 30) == SHAPE and call(batch=2, mv=1 << 30) == SHAPE
    # parameters
    for kw in (dict(mw=0.0), dict(mw=-1.0), dict(mw=NAN), dict(mw=INF), dict(o=(NAN, 0.0, 0.0)), dict(o=(0.0, INF, 0.0)),
               dict(o=(0.0, 0.0, -INF)), dict(vs=0.0), dict(vs=-1.0), dict(vs=NAN), dict(vs=INF), dict(mv=-1), dict(mt=-1)):
        assert call(**kw) == PARAM, kw
    # alignment
    for kw in (dict(vol=p + 8), dict(v=p + 8), dict(n=p + 4), dict(t=p + 2), dict(c=p + 1), dict(ws=p + 8)):
        assert call(**kw) == ALIGN, kw
    # the workspace
    need = lib.mi_tsdf_surface_workspace_bytes(2, 56, 44, 72)
    assert call(wb=need - 1) == CAPACITY and call(wb=0) == CAPACITY
    assert call(wb=0, v=None, n=None, t=None, mv=0, mt=0) == CAPACITY                  # the sizing pass needs it as well


def test_workspace_size_grows_with_the_volume(lib):
    ws = lib.mi_tsdf_surface_workspace_bytes
    assert ws(1, 2, 2, 2) > 0 and ws(1, 2, 2, 2) % 16 == 0
    assert ws(1, 56, 44, 72) >= 56 * 44 * 72 and ws(2, 56, 44, 72) == 2 * ws(1, 56, 44, 72)
    assert ws(1, 56, 44, 72) < ws(1, 57, 44, 72) < ws(1, 57, 45, 72) < ws(1, 57, 45, 73)
    assert ws(1, 256, 256, 256) < 1.1 * 256 ** 3                                       # a byte per voxel and a little per row
    assert ws(0, 8, 8, 8) == 0 and ws(1, 1, 8, 8) == 0 and ws(1, 512, 512, 683) == 0 and ws(1, 512, 512, 682) > 0


def test_module_argument_errors():
    from onnx_image_processing_amd import ops
    from onnx_image_processing_amd.pytorch_model.geometry import TsdfVolume
    from onnx_image_processing_amd.synth import rgbd_camera
    m = TsdfVolume(torch.from_numpy(rgbd_camera(48, 64)), (8, 8, 8), 0.1, (0.0, 0.0, 0.0))
    for call in (m.extract_surface, lambda: m.extract_surface(100, 200), m.extract_points, lambda: m.extract_points(50)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    vol = torch.zeros(1, 4, 4, 4, 2)
    for call in (lambda: ops.tsdf_surface(vol, (0, 0, 0), 0.1, 10, 10), lambda: ops.tsdf_surface_counts(vol)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    assert callable(ops.tsdf_surface) and callable(ops.tsdf_surface_counts)
    assert "voxel_downsample_batch" in TsdfVolume.extract_points.__doc__
