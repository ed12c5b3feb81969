"""K20 TSDF surface extraction on the GPU against tests/surface_oracle.py (the numpy restatement of include/mi355x_match.h,
"TSDF surface extraction").

Every volume is the float32 oracle's (tests/tsdf_oracle.py; tests/test_gpu_tsdf.py proves the GPU integration equal to it),
uploaded.  Counts and triangles are integers: compared exactly.  Vertices and normals are compared bit for bit with the oracle
run in float32, which is the header's arithmetic, and with the float64 oracle within the deviation of the SAME oracle run in
float32 from its float64 run, measured on the CPU on the very volumes the test uses, times 4 (the margin of
tests/test_gpu_tsdf.py).  Nothing here was taken from the kernels.  Largest deviation of a vertex / normal component:
    ROOM (37, 53) 6.1060e-6 / 5.0155e-6 (the same with min_weight 2), ODD (37, 53) 2.8704e-6 / 4.3737e-6,
    TINY (37, 53) 1.9712e-7 / no normals, the 130 x 3 x 3 plane 6.9663e-7 / no normals (no +- one voxel in 3 voxels),
    the 20^3 sphere 9.0385e-7 / 2.7098e-7
-> TOL = 4 times these.  The float32 oracle has the float64 oracle's counts, triangles and normal validity on all of them.
Runs unchanged under MI_POISON_EMPTY=1 (conftest.py): every output and the workspace come from torch.empty."""
import functools

import numpy as np
import pytest
import torch

import surface_oracle as SO
import tsdf_oracle as TO
from gpu_common import DEV, GPU, bits
from onnx_image_processing_amd import _native as N
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.pytorch_model.geometry import TsdfVolume
from onnx_image_processing_amd.synth import rgbd_camera

pytestmark = GPU
F32, F64 = np.float32, np.float64
H, W = 37, 53
SPECS = {"room": TO.ROOM, "odd": TO.ODD, "tiny": TO.TINY}
COUNTS = {"room": (9232, 17732), "odd": (6659, 12744), "tiny": (9, 8), "plane": (1504, 2447), "sphere": (2168, 4332)}
TOL = {"room": (2.4424e-5, 2.0062e-5), "odd": (1.1482e-5, 1.7495e-5), "tiny": (7.8848e-7, 0.0), "plane": (2.7866e-6, 0.0),
       "sphere": (3.6154e-6, 1.0840e-6)}
SPHERE = ((9.3, 9.7, 10.1), 6.2)


@functools.lru_cache(maxsize=None)
def scene(name):
    """(volume float32 (tsdf, weight), volume float64, grid) of a named test volume"""
    if name == "plane":
        return SO.plane_volume(F32), SO.plane_volume(F64), SO.PLANE_GRID
    if name == "sphere":
        v = SO.sphere_volume(20, *SPHERE, F32)
        return v, tuple(x.astype(F64) for x in v), SO.UNIT_GRID
    return TO.fused_room(H, W, SPECS[name], F32), TO.fused_room(H, W, SPECS[name], F64), TO.grid_of(SPECS[name])[1]


@functools.lru_cache(maxsize=None)
def oracle(name, min_weight=1.0, dtype=F32):
    v32, v64, grid = scene(name)
    return SO.extract(v32 if dtype == F32 else v64, grid, min_weight=min_weight, dtype=dtype)


@functools.lru_cache(maxsize=None)
def uploaded(name):
    """(1, nz, ny, nx, 2) on the GPU; never written to"""
    return torch.from_numpy(np.stack(scene(name)[0], axis=-1).astype(F32))[None].to(DEV)


def extract(name, mv, mt, min_weight=1.0, **kw):
    grid = scene(name)[2]
    return ops.tsdf_surface(uploaded(name), grid[0].tolist(), grid[1], mv, mt, min_weight, **kw)


def check_against_the_oracles(name, got, min_weight=1.0):
    """got: ops.tsdf_surface's outputs for ONE volume with capacities at or above the totals"""
    vertex, normal, tris, counts = (x[0].cpu().numpy() for x in got)
    m32, m64 = oracle(name, min_weight, F32), oracle(name, min_weight, F64)
    nv, nt = m32["counts"]
    assert m64["counts"] == (nv, nt) and np.array_equal(m64["triangles"], m32["triangles"]) and np.array_equal(m64["normal_ok"], m32["normal_ok"])
    print(f"{name} (min_weight {min_weight}): counts {counts.tolist()} against {(nv, nt)}")
    assert counts.tolist() == [nv, nt]
    assert np.array_equal(tris[:nt], m32["triangles"])
    v, n = vertex[:nv], normal[:nv]
    assert (v[:, 3] == 1).all() and np.array_equal(n[:, 3] != 0, m32["normal_ok"]) and set(np.unique(n[:, 3])) <= {0.0, 1.0}
    dv = float(np.abs(v[:, :3] - m64["vertices"]).max()) if nv else 0.0
    dn = float(np.abs(n[:, :3] - m64["normals"]).max()) if nv else 0.0
    same = np.array_equal(bits(v[:, :3]), bits(m32["vertices"])) and np.array_equal(bits(n[:, :3]), bits(m32["normals"]))
    tol_v, tol_n = TOL[name]
    print(f"  vertex {dv:.3e} (tolerance {tol_v:.2e}), normal {dn:.3e} (tolerance {tol_n:.2e}), float32 oracle's bits: {same}")
    assert np.abs(m32["vertices"] - m64["vertices"]).max() <= tol_v / 4 * 1.001 and np.abs(m32["normals"] - m64["normals"]).max() <= tol_n / 4 * 1.001
    assert dv <= tol_v and dn <= tol_n
    assert same
    # the tails
    assert not vertex[nv:].any() and not normal[nv:].any() and (tris[nt:] == -1).all()
    return vertex, normal, tris


# ---- 1. the meshes -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["room", "odd", "tiny", "plane"])
def test_mesh_is_the_oracles(name):
    nv, nt = COUNTS[name]
    assert oracle(name)["counts"] == (nv, nt)
    got = extract(name, nv + 37, nt + 11)                         # capacities above the totals: the tails are checked too
    assert got[0].shape == (1, nv + 37, 4) and got[1].shape == (1, nv + 37, 4) and got[2].shape == (1, nt + 11, 3) and got[3].shape == (1, 2)
    assert got[2].dtype == torch.int32 and got[3].dtype == torch.int32
    check_against_the_oracles(name, got)
    if name == "plane":                                           # every 64-voxel chunk of the rows owns vertices
        assert (np.bincount(oracle(name)["owner"][:, 0] // 64, minlength=3) > 0).all()
    exact = extract(name, nv, nt)                                 # exactly the totals: no tail
    assert all(torch.equal(bits(a[:, :n]), bits(b)) for a, b, n in zip(got[:3], exact[:3], (nv, nv, nt))) and torch.equal(got[3], exact[3])


def test_min_weight_2_is_the_oracle_run_with_it():
    m = oracle("room", 2.0)
    assert m["counts"] == (8389, 16048) and m["counts"] != COUNTS["room"]
    check_against_the_oracles("room", extract("room", 8400, 16100, 2.0), 2.0)


def test_sphere_is_a_closed_outward_manifold():
    nv, nt = COUNTS["sphere"]
    vertex, normal, tris = check_against_the_oracles("sphere", extract("sphere", nv, nt))
    topo = SO.mesh_topology(vertex[:, :3], tris)
    assert topo == dict(closed=True, euler=2, used=True, degenerate=0)
    v = vertex[:, :3].astype(F64)
    n = np.cross(v[tris[:, 1]] - v[tris[:, 0]], v[tris[:, 2]] - v[tris[:, 0]])
    assert ((n * (v[tris].mean(1) - np.array(SPHERE[0]))).sum(1) > 0).all()
    assert ((normal[:, :3] * (v - np.array(SPHERE[0]))).sum(1) > 0).all() and np.abs(np.linalg.norm(normal[:, :3], axis=1) - 1).max() < 1e-6


# ---- 2. capacities, tails, sizing ------------------------------------------------------------------------------------------------

def raw_call(volume, grid, mv, mt, guard, min_weight=1.0):
    """`mi_tsdf_surface` on outputs that sit inside larger sentinel-filled buffers, `guard` rows on either side"""
    b, nz, ny, nx = (int(x) for x in volume.shape[:4])
    vertex = torch.full((b * mv + 2 * guard, 4), 7.0, dtype=torch.float32, device=DEV)
    normal = torch.full((b * mv + 2 * guard, 4), 7.0, dtype=torch.float32, device=DEV)
    tris = torch.full((b * mt + 2 * guard, 3), 7, dtype=torch.int32, device=DEV)
    counts = torch.full((b + 2, 2), 7, dtype=torch.int32, device=DEV)
    wbytes = int(N.load().mi_tsdf_surface_workspace_bytes(b, nz, ny, nx))
    work = torch.empty((wbytes // 8,), dtype=torch.int64, device=DEV)
    N.call("mi_tsdf_surface", volume.data_ptr(), b, nz, ny, nx, *grid[0].tolist(), grid[1], min_weight, mv, mt,
           vertex[guard:].data_ptr(), normal[guard:].data_ptr(), tris[guard:].data_ptr(), counts[1:].data_ptr(), work.data_ptr(), wbytes,
           N.stream_ptr())
    for buf, n in ((vertex, b * mv), (normal, b * mv), (tris, b * mt)):
        assert bool((buf[:guard] == 7).all()) and bool((buf[guard + n:] == 7).all())
    assert bool((counts[0] == 7).all()) and bool((counts[b + 1] == 7).all())
    return (vertex[guard:guard + b * mv].view(b, mv, 4), normal[guard:guard + b * mv].view(b, mv, 4), tris[guard:guard + b * mt].view(b, mt, 3),
            counts[1:b + 1])


def test_capacities_below_the_totals_keep_the_true_counts_and_the_first_rows():
    nv, nt = COUNTS["room"]
    grid = scene("room")[2]
    full = extract("room", nv, nt)
    for mv, mt in ((1000, 777), (1, nt), (nv, 1), (64, 0), (0, 5), (0, 0)):      # (0, 0) with outputs given: still only the counts
        vertex, normal, tris, counts = raw_call(uploaded("room"), grid, mv, mt, 16)
        assert counts.tolist() == [[nv, nt]], (mv, mt)
        assert torch.equal(bits(vertex), bits(full[0][:, :mv])) and torch.equal(bits(normal), bits(full[1][:, :mv])), (mv, mt)
        assert torch.equal(tris, full[2][:, :mt]), (mv, mt)                    # the true ids, also those past max_vertices
        assert mt != nt or int(tris.max()) >= mv
    vertex, normal, tris, counts = extract("room", 1000, 777)
    assert counts.tolist() == [[nv, nt]] and torch.equal(bits(vertex), bits(full[0][:, :1000])) and torch.equal(tris, full[2][:, :777])


def test_capacities_above_the_totals_write_the_tails():
    nv, nt = COUNTS["odd"]
    grid = scene("odd")[2]
    full = extract("odd", nv, nt)
    for mv, mt in ((nv + 1, nt + 1), (nv + 70001, nt + 300), (nv + 5, nt + 40003)):       # the tail's workgroups stride over it
        vertex, normal, tris, counts = raw_call(uploaded("odd"), grid, mv, mt, 16)
        assert counts.tolist() == [[nv, nt]]
        assert torch.equal(bits(vertex[:, :nv]), bits(full[0])) and torch.equal(bits(normal[:, :nv]), bits(full[1])) and torch.equal(tris[:, :nt], full[2])
        assert not bool(vertex[:, nv:].any()) and not bool(normal[:, nv:].any()) and bool((tris[:, nt:] == -1).all())


@pytest.mark.parametrize("name", ["room", "tiny"])
def test_a_reset_volume_is_all_tail(name):
    nx, ny, nz = SPECS[name][0]
    grid = scene(name)[2]
    vol = ops.tsdf_reset(torch.empty((2, nz, ny, nx, 2), dtype=torch.float32, device=DEV))
    vertex, normal, tris, counts = ops.tsdf_surface(vol, grid[0].tolist(), grid[1], 300, 500)
    assert counts.tolist() == [[0, 0], [0, 0]]
    assert not bool(vertex.any()) and not bool(normal.any()) and bool((tris == -1).all())   # NaN (a poisoned byte left) would be True
    vertex, normal, tris, counts = ops.tsdf_surface(vol, grid[0].tolist(), grid[1], 300, 500, normals=False, triangles=False)
    assert normal is None and tris is None and counts.tolist() == [[0, 0], [0, 0]] and not bool(vertex.any())
    assert ops.tsdf_surface_counts(vol).tolist() == [[0, 0], [0, 0]]
    # observed and inside everywhere: no crossing either
    vol[..., 0], vol[..., 1] = -0.5, 3.0
    assert ops.tsdf_surface_counts(vol).tolist() == [[0, 0], [0, 0]]


def test_sizing_pass_equals_the_counts_of_the_full_call():
    for name in ("room", "odd", "tiny", "plane", "sphere"):
        for mw in (1.0, 2.0):
            sizing = ops.tsdf_surface_counts(uploaded(name), mw)
            assert sizing.shape == (1, 2) and sizing.dtype == torch.int32
            assert sizing.tolist() == [list(oracle(name, mw)["counts"])], (name, mw)
            assert torch.equal(sizing, extract(name, 10, 10, mw)[3]) and torch.equal(sizing, extract(name, 0, 0, mw)[3])


# ---- 3. batches, reproducibility, graphs ------------------------------------------------------------------------------------------

def three_volumes():
    """three different volumes of ROOM's shape: the four views, the same seen from weight 2, and one with a block unobserved
    (the oracle finds 5914 vertices and 10985 triangles in it)"""
    room = uploaded("room")
    thin = room.clone()
    thin[..., 1] = torch.where(room[..., 1] >= 2, room[..., 1], torch.zeros_like(room[..., 1]))
    cut = room.clone()
    cut[:, 20:40, 10:30, 15:50, 1] = 0
    return [room, thin, cut]


def test_batch_is_the_single_calls_and_runs_repeat():
    vols = three_volumes()
    grid = scene("room")[2]
    singles = [ops.tsdf_surface(v, grid[0].tolist(), grid[1], 9500, 18000) for v in vols]
    assert len({tuple(s[3][0].tolist()) for s in singles}) == 3                            # three different meshes
    assert singles[1][3].tolist() == [list(oracle("room", 2.0)["counts"])] and singles[2][3].tolist() == [[5914, 10985]]
    batch = ops.tsdf_surface(torch.cat(vols), grid[0].tolist(), grid[1], 9500, 18000)
    for b, s in enumerate(singles):
        assert all(torch.equal(bits(x[b]), bits(y[0])) for x, y in zip(batch, s)), b
    again = ops.tsdf_surface(torch.cat(vols), grid[0].tolist(), grid[1], 9500, 18000)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(batch, again))
    assert torch.equal(ops.tsdf_surface_counts(torch.cat(vols)), batch[3])


def module(vols, **kw):
    spec = TO.ROOM
    m = TsdfVolume(torch.from_numpy(rgbd_camera(H, W)), spec[0], spec[2], spec[1], truncation=spec[3], batch=len(vols), size=(H, W), **kw).to(DEV)
    m.volume.copy_(torch.cat(vols))
    return m


def test_extract_surface_replays_from_a_captured_graph_to_the_eager_bits():
    vols = three_volumes()
    orders = [(0, 1, 2), (2, 0, 1), (1, 1, 0)]
    m = module(vols)
    eager = []
    for o in orders:
        m.volume.copy_(torch.cat([vols[i] for i in o]))
        eager.append([x.clone() for x in m.extract_surface(9500, 18000)])
    m.volume.copy_(torch.cat(vols))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.extract_surface(9500, 18000)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m.extract_surface(9500, 18000)
    for i in (1, 2, 0):
        m.volume.copy_(torch.cat([vols[j] for j in orders[i]]))
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(out, eager[i])), i


# ---- 4. the module ---------------------------------------------------------------------------------------------------------------

def test_extract_surface_without_capacities_returns_exactly_sized_arrays():
    vols = three_volumes()
    m = module(vols[:1])
    nv, nt = COUNTS["room"]
    vertex, normal, tris, counts = m.extract_surface()
    assert vertex.shape == (1, nv, 4) and normal.shape == (1, nv, 4) and tris.shape == (1, nt, 3) and counts.tolist() == [[nv, nt]]
    ref = extract("room", nv, nt)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip((vertex, normal, tris, counts), ref))
    # a batch: sized by its largest volume, the others' tails filled
    m3 = module(vols)
    v3, n3, t3, c3 = m3.extract_surface()
    assert v3.shape[1] == int(c3[:, 0].max()) and t3.shape[1] == int(c3[:, 1].max()) and c3[0].tolist() == [nv, nt]
    for b in range(3):
        assert not bool(v3[b, int(c3[b, 0]):].any()) and bool((t3[b, int(c3[b, 1]):] == -1).all())
        assert int(t3[b, :int(c3[b, 1])].min()) >= 0 and int(t3[b, :int(c3[b, 1])].max()) < int(c3[b, 0])
    # one capacity given: the other comes from the sizing pass
    v, n, t, c = m.extract_surface(max_vertices=100)
    assert v.shape == (1, 100, 4) and t.shape == (1, nt, 3) and torch.equal(t, tris) and torch.equal(bits(v), bits(vertex[:, :100]))
    # min_weight reaches the kernel
    assert m.extract_surface(min_weight=2.0)[3].tolist() == [list(oracle("room", 2.0)["counts"])]


def test_extract_points_is_the_vertex_part():
    m = module(three_volumes())
    vertex, normal, _, counts = m.extract_surface()
    points, pnormal, pcounts = m.extract_points()
    assert torch.equal(bits(points), bits(vertex)) and torch.equal(bits(pnormal), bits(normal)) and torch.equal(pcounts, counts)
    points, pnormal, pcounts = m.extract_points(500)
    assert points.shape == (3, 500, 4) and torch.equal(bits(points), bits(vertex[:, :500])) and torch.equal(bits(pnormal), bits(normal[:, :500]))
    assert torch.equal(pcounts, counts)                             # the triangle totals are still counted
    # the cloud feeds voxel_downsample_batch as the docstring says
    clouds = [vertex[b, :int(counts[b, 0]), :3].contiguous() for b in range(3)]
    down, mask = ops.voxel_downsample_batch(clouds, 0.25)[:2]
    assert down.shape[0] == sum(int(c) for c in counts[:, 0]) and 0 < int(mask.sum()) < down.shape[0]
