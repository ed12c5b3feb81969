"""K12 voxel downsampling on the MI355X: reference parity on every fixture case, the fp64 oracle at scale, batching,
determinism, leaf forms and hipGraph capture.  Also run under MI_POISON_EMPTY=1 (conftest.py): a workspace assumed
zero or a row left unwritten then fails here.

Parity: mask, M and the voxel order equal the reference's exactly; each mean g is within 2 float32 ulps of the largest
|x| of its voxel's column of the fp64 mean e, and no further from the reference's mean r than r is from e plus that."""
import numpy as np
import pytest
import torch

from test_voxel_host import golden_cases, voxel_oracle
from gpu_common import DEV, gpu
from onnx_image_processing_amd import ops
from onnx_image_processing_amd.synth import synth_depth_cloud

pytestmark = pytest.mark.gpu


def _model():
    from pytorch_model.pointcloud.voxel_downsampling import VoxelDownsampling
    return VoxelDownsampling()


def check_against_oracle(pts, leaf, out, mask, ref_out=None, ref_mask=None, what=""):
    out = out.cpu().numpy() if isinstance(out, torch.Tensor) else out
    mask = mask.cpu().numpy() if isinstance(mask, torch.Tensor) else mask
    keys, means, counts = voxel_oracle(pts, leaf)
    m = keys.size
    n = pts.shape[0]
    assert out.shape == pts.shape and out.dtype == np.float32 and mask.shape == (n,) and mask.dtype == bool, what
    if ref_mask is not None:
        assert np.array_equal(mask, ref_mask), what
    assert int(mask.sum()) == m and mask[:m].all(), what
    assert (out[m:] == 0).all() and not np.signbit(out[m:]).any(), what
    if m == 0:
        return
    # per voxel and column: the largest |x| (the scale of the 2-ulp bound)
    with np.errstate(over="ignore", invalid="ignore"):
        c = np.floor(pts[:, :3] / np.float32(leaf)).astype(np.int64)
        c = c - c.min(0)
        mx = c.max(0)
        key = c[:, 0] * (mx[1] + 1) * (mx[2] + 1) + c[:, 1] * (mx[2] + 1) + c[:, 2]
    inv = np.searchsorted(keys, key)
    amax = np.zeros((m, pts.shape[1]), np.float32)
    np.maximum.at(amax, inv, np.abs(pts))
    bound = 2.0 * np.spacing(amax).astype(np.float64)
    g = out[:m].astype(np.float64)
    assert np.isfinite(g).all(), f"{what}: {int((~np.isfinite(g)).any(1).sum())} means not finite"
    err = np.abs(g - means)
    bad = err > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} means off, worst {err.max():.3e} (row {np.argmax(err.max(1))})"
    if ref_out is not None:
        r = ref_out[:m].astype(np.float64)
        assert (np.abs(g - r) <= np.abs(r - means) + bound).all(), what


def test_every_fixture_case():
    model = _model()
    for name, (pts, leaf, ref_out, ref_mask) in golden_cases().items():
        out, mask = model(gpu(pts), torch.tensor(leaf, device=DEV))
        torch.cuda.synchronize()
        check_against_oracle(pts, leaf, out, mask, ref_out, ref_mask, name)


def test_generic_column_counts():
    """D outside the fast instances {3, 4, 6}: the generic instance (columns in rounds of four)."""
    rng = np.random.default_rng(5)
    model = _model()
    for d in (3, 4, 5, 6, 7, 11):
        pts = (rng.standard_normal((20_000, d)) * 2 + 1).astype(np.float32)
        out, mask = model(gpu(pts), 0.25)
        check_against_oracle(pts, np.float32(0.25), out, mask, what=f"d={d}")


def test_sixteen_depth_frames_in_one_batch():
    clouds = [synth_depth_cloud(100 + i) for i in range(16)]
    out, mask, counts, offs = ops.voxel_downsample_batch([gpu(c) for c in clouds], 0.02)
    out, mask, counts = out.cpu().numpy(), mask.cpu().numpy(), counts.cpu().numpy()
    o = offs.cpu().numpy()
    assert o[-1] == 16 * 480 * 640
    for b, c in enumerate(clouds):
        sl = slice(o[b], o[b + 1])
        check_against_oracle(c, np.float32(0.02), out[sl], mask[sl], what=f"frame {b}")
        assert counts[b] == mask[sl].sum()


def test_four_million_points_where_the_reference_is_inaccurate():
    pts = (3 * np.random.default_rng(7).standard_normal((4_000_000, 3)) + 10).astype(np.float32)
    out, mask = _model()(gpu(pts), torch.tensor(0.05, device=DEV))
    check_against_oracle(pts, np.float32(0.05), out, mask, what="4M")


def test_one_voxel_of_a_million_points():
    """Every point in one voxel: the spanning-voxel fix-up over ~3900 tile pieces, not one thread over 1M points."""
    pts = np.random.default_rng(8).uniform(0.001, 0.049, (1_000_000, 3)).astype(np.float32)
    out, mask = _model()(gpu(pts), 0.05)
    check_against_oracle(pts, np.float32(0.05), out, mask, what="one voxel")
    assert int(mask.sum()) == 1


def test_batch_equals_single_calls_bit_for_bit():
    rng = np.random.default_rng(9)
    clouds = [synth_depth_cloud(5, 120, 160), np.zeros((0, 3), np.float32), (rng.standard_normal((777, 3))).astype(np.float32),
              np.zeros((0, 3), np.float32), np.tile(np.float32([[1, 2, 3]]), (3000, 1)), synth_depth_cloud(6, 60, 80)]
    leaves = [0.02, 0.05, 0.1, 0.05, 0.05, 0.03]
    out, mask, counts, offs = ops.voxel_downsample_batch([gpu(c) for c in clouds], leaves)
    o = offs.cpu().numpy()
    model = _model()
    for b, (c, lf) in enumerate(zip(clouds, leaves)):
        so, sm = model(gpu(c), lf)
        assert torch.equal(out[o[b]:o[b + 1]], so) and torch.equal(mask[o[b]:o[b + 1]], sm), b
        assert int(counts[b]) == int(sm.sum())
    # packed points + device offsets: the same call
    out2, mask2, counts2, _ = ops.voxel_downsample_batch(torch.cat([gpu(c) for c in clouds]), gpu(np.float32(leaves)),
                                                         offsets=offs)
    assert torch.equal(out, out2) and torch.equal(mask, mask2) and torch.equal(counts, counts2)


def test_many_clouds_use_two_cloud_digits():
    """300 clouds: the cloud id takes two radix digits."""
    rng = np.random.default_rng(10)
    clouds = [(rng.standard_normal((int(rng.integers(0, 60)), 3))).astype(np.float32) for _ in range(300)]
    out, mask, counts, offs = ops.voxel_downsample_batch([gpu(c) for c in clouds], 0.5)
    out, mask, o = out.cpu().numpy(), mask.cpu().numpy(), offs.cpu().numpy()
    for b, c in enumerate(clouds):
        check_against_oracle(c, np.float32(0.5), out[o[b]:o[b + 1]], mask[o[b]:o[b + 1]], what=f"cloud {b}")


def test_two_calls_are_bitwise_equal():
    clouds = [gpu(synth_depth_cloud(200 + i)) for i in range(4)]
    a = ops.voxel_downsample_batch(clouds, 0.02)
    b = ops.voxel_downsample_batch(clouds, 0.02)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_leaf_forms_agree():
    pts = gpu(synth_depth_cloud(21, 240, 320))
    model = _model()
    outs = [model(pts, lf) for lf in (torch.tensor(0.02, device=DEV), torch.tensor(0.02), 0.02,
                                      torch.tensor([0.02], device=DEV))]
    for o, m in outs[1:]:
        assert torch.equal(o, outs[0][0]) and torch.equal(m, outs[0][1])


def test_empty_input_is_the_reference_clone():
    pts = torch.zeros(0, 5, device=DEV)
    out, mask = _model()(pts, 0.1)
    assert out.shape == (0, 5) and mask.shape == (0,) and mask.dtype == torch.bool


def test_non_float32_and_narrow_inputs_raise():
    with pytest.raises(RuntimeError, match="float32"):
        _model()(torch.zeros(10, 3, dtype=torch.float64, device=DEV), 0.1)
    with pytest.raises(RuntimeError, match="3 columns"):
        _model()(torch.zeros(10, 2, device=DEV), 0.1)


def test_graph_capture_replays_bit_identically():
    from onnx_image_processing_amd.graph import GraphedModule
    model = _model()
    p1 = gpu(synth_depth_cloud(31, 240, 320))
    p2 = gpu(synth_depth_cloud(32, 240, 320))
    leaf = torch.tensor(0.02, device=DEV)
    g = GraphedModule(model, p1, leaf)
    o, m = g(p1, leaf)
    e_o, e_m = model(p1, leaf)
    assert torch.equal(o, e_o) and torch.equal(m, e_m)
    leaf2 = torch.tensor(0.05, device=DEV)
    o, m = g(p2, leaf2)
    e_o, e_m = model(p2, leaf2)
    assert torch.equal(o, e_o) and torch.equal(m, e_m)
    check_against_oracle(p2.cpu().numpy(), np.float32(0.05), o, m, what="graph replay")


# voxel sizes (in points, one voxel per unit cell along x) whose voxels cross 256-row tiles and end ON a tile edge with
# further voxels after them, or end inside a tile: the fix-up must take exactly the tiles that hold the voxel's rows
EDGE_LAYOUTS = [[512, 100], [300, 300], [256, 256, 1], [1, 255, 512, 3], [768, 5], [255, 1, 256, 256, 7],
                [10, 502, 512, 1], [513, 511, 256, 2]]


def _edge_cloud(sizes, seed):
    rng = np.random.default_rng(seed)
    pts = [np.stack([v + rng.uniform(0.1, 0.9, n), rng.uniform(0.1, 0.9, n), rng.uniform(0.1, 0.9, n)], 1)
           for v, n in enumerate(sizes)]
    p = np.concatenate(pts).astype(np.float32)
    return p[rng.permutation(p.shape[0])]


def _call_with_workspace(pts: torch.Tensor, leaf: float, fill: int):
    """mi_voxel_downsample with a workspace pre-filled with `fill` bytes (the ABI takes a workspace of any content)."""
    from onnx_image_processing_amd import _native as N
    n, d = pts.shape
    offs = torch.tensor([0, n], dtype=torch.int64, device=DEV)
    lf = torch.tensor([leaf], dtype=torch.float32, device=DEV)
    wbytes = N.load().mi_voxel_downsample_workspace_bytes(1, n, d)
    work = torch.full((wbytes,), fill, dtype=torch.uint8, device=DEV)
    out = torch.zeros((n, d), dtype=torch.float32, device=DEV)
    mask = torch.zeros((n,), dtype=torch.bool, device=DEV)
    counts = torch.zeros((1,), dtype=torch.int64, device=DEV)
    N.call("mi_voxel_downsample", pts.data_ptr(), offs.data_ptr(), 1, n, d, lf.data_ptr(), out.data_ptr(), mask.data_ptr(),
           counts.data_ptr(), work.data_ptr(), wbytes, N.stream_ptr())
    return out, mask, counts


def test_voxels_ending_on_tile_edges():
    model = _model()
    for k, sizes in enumerate(EDGE_LAYOUTS):
        pts = _edge_cloud(sizes, 40 + k)
        out, mask = model(gpu(pts), 1.0)
        check_against_oracle(pts, np.float32(1.0), out, mask, what=f"sizes {sizes}")
        dirty = [_call_with_workspace(gpu(pts), 1.0, fill) for fill in (0x00, 0x5A, 0xFF)]
        for o, m, c in dirty:
            assert torch.equal(o, out) and torch.equal(m, mask) and int(c[0]) == len(sizes), f"sizes {sizes}"


def test_depth_frames_at_coarse_leaves():
    """Dense clouds at leaf 0.1-0.2: many voxels of hundreds of points, some ending on tile edges mid-cloud."""
    clouds = [synth_depth_cloud(60 + i) for i in range(3)]
    for leaf in (0.1, 0.2):
        out, mask, counts, offs = ops.voxel_downsample_batch([gpu(c) for c in clouds], leaf)
        out, mask, o = out.cpu().numpy(), mask.cpu().numpy(), offs.cpu().numpy()
        for b, c in enumerate(clouds):
            check_against_oracle(c, np.float32(leaf), out[o[b]:o[b + 1]], mask[o[b]:o[b + 1]], what=f"leaf {leaf} frame {b}")
