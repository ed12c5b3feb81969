"""GPU runtime behaviour of the library -- everything that is not "this kernel computes the reference's numbers":
hipGraph capture / replay (forked and unforked), host threads and streams, the Sinkhorn stream-schedule tuner, loud
failure modes (timed-out solver, dirty ticket counters), the one-call C ABI (`mi_match_pairs`) from Python and from a
C host without Python, and bench.py's N-rank control flow on real RCCL with one rank.  Run with `-m gpu` on an MI355X."""
import os

import numpy as np
import pytest
import torch

from gpu_common import DEV, ROOT, _images, _status_word, gpu, mods  # noqa: F401  (mods: the module fixture)
from helpers import (ALLOW, bad_tables, bits_mismatch, cfg_of, check_match_sets, load_golden, match_dict, p_close, permute_p,  # noqa: F401
                     tie_canonical_perm, unpack_bits)
from onnx_image_processing_amd.synth import synth_batch, synth_image  # noqa: F401
from oracle import numpy_oracle as O  # noqa: F401

pytestmark = pytest.mark.gpu


def test_sinkhorn_stream_schedules_agree(mods):
    """mi_sinkhorn_dots for >= 64 pairs picks the streams of its two half-batches itself (caller + helper, two helpers,
    or unsplit -- whichever the first calls on a caller stream measured fastest; csrc/sinkhorn_dots.hip ForkJoin).  The
    schedules are the same arithmetic: duals and P of every fixed schedule (debug library, key 11) and of the self-tuned
    default -- through its trial calls and after its decision, on the default stream and on a second stream -- are
    identical."""
    from onnx_image_processing_amd import _native as N, ops
    rng = np.random.default_rng(77)
    b1 = rng.integers(0, 2 ** 32, size=(70, 300, 16), dtype=np.uint64).astype(np.uint32)
    b2 = rng.integers(0, 2 ** 32, size=(70, 280, 16), dtype=np.uint64).astype(np.uint32)
    b2[:, :100] = b1[:, :100]
    t1, t2 = gpu(b1.view(np.int32)), gpu(b2.view(np.int32))
    run = lambda: [t.clone() for t in ops.sinkhorn_bits(t1, t2, True, 0.05, 1.0, 12, return_duals=True)]
    with N.debug_library() as lib:
        want = None
        for sched in (0, 1, 2):
            assert lib.mi_debug_set(11, sched) == 0
            got = run()
            want = want or got
            for x, y in zip(got, want):
                assert torch.equal(x, y), sched
        assert lib.mi_debug_set(11, -1) == 0
        assert lib.mi_debug_set(11, 3) != 0
    other = torch.cuda.Stream()
    shape = (70, 300, 280, 12)
    for stream in (torch.cuda.current_stream(), other):
        with torch.cuda.stream(stream):
            ops.set_sinkhorn_schedule(ops.MI_SCHEDULE_UNDECIDED)  # forget whatever earlier tests left on this stream
            assert ops.sinkhorn_schedule(*shape) == ops.MI_SCHEDULE_UNDECIDED
            for call in range(12):                               # nine trial calls, then the decided schedule
                for x, y in zip(run(), want):
                    assert torch.equal(x, y), call
                stream.synchronize()
            decided = ops.sinkhorn_schedule(*shape)              # product ABI: the decision is visible ...
            assert decided in (0, 1, 2), decided
            assert ops.sinkhorn_schedule(64, 300, 280, 12) == ops.MI_SCHEDULE_UNDECIDED     # ... per shape
            for pin in (2, 1, 0):                                # ... and can be pinned
                ops.set_sinkhorn_schedule(pin)
                assert ops.sinkhorn_schedule(*shape) == pin and ops.sinkhorn_schedule(64, 300, 280, 12) == pin
                for x, y in zip(run(), want):
                    assert torch.equal(x, y), pin
            ops.set_sinkhorn_schedule(ops.MI_SCHEDULE_UNDECIDED)
            with pytest.raises(RuntimeError):
                ops.set_sinkhorn_schedule(3)
    # MI_SOLVER_NO_FORK: everything on the caller's stream, same duals
    ops.set_solver_flags(ops.MI_SOLVER_NO_FORK)
    try:
        for x, y in zip(run(), want):
            assert torch.equal(x, y)
        ops.set_solver_flags(ops.MI_SOLVER_NO_FORK | ops.MI_SOLVER_MULTI_LAUNCH)
        for x, y in zip(run(), want):
            assert torch.equal(x, y)
    finally:
        ops.set_solver_flags(ops.MI_SOLVER_DEFAULT)
    with pytest.raises(ValueError):
        ops.set_solver_flags(4)


@pytest.mark.parametrize("batch,n,m,bits,eps", [(64, 512, 512, 256, 0.05), (40, 300, 277, 512, 0.05), (33, 700, 1024, 256, 0.1),
                                               (3, 130, 900, 992, 0.05), (64, 512, 512, 256, 0.03), (9, 512, 512, 512, 0.2)])
def test_sinkhorn_row_kernel_reading_the_dots_as_fp16_denormals(mods, batch, n, m, bits, eps):
    """With fewer than 1024 descriptor bits every dot product is < 1024, and the uint16 read as an fp16 is the denormal
    dot * 2^-24: mi_sinkhorn_dots' row kernel (MI_SOLVER_DOTS_BELOW_1024, which ops.sinkhorn_bits and mi_match_pairs set
    by themselves) multiplies it in one v_fma_mix_f32 instead of converting first and carries the 2^24 in the row factor.
    Exact scalings around the same roundings: duals and P are identical with it (default) and without (debug key 15 =
    0) -- one and two 512-column chunks, ragged extents, the largest value the flag admits (992 set bits against
    themselves), zero dots, both row kernels (eps = 0.03 takes the row-maximum one)."""
    from onnx_image_processing_amd import _native as N, ops
    rng = np.random.default_rng(n + m)
    w = bits // 32
    b1 = rng.integers(0, 2 ** 32, size=(batch, n, w), dtype=np.uint64).astype(np.uint32)
    b2 = rng.integers(0, 2 ** 32, size=(batch, m, w), dtype=np.uint64).astype(np.uint32)
    k = min(n, m) // 3
    b2[:, :k] = b1[:, :k]
    b1[:, 0], b2[:, 0] = 0xFFFFFFFF, 0xFFFFFFFF          # dot product = bits
    b1[:, 1] = 0
    b2[:, 2] = ~b1[:, 2]                                  # dot product 0 against a non-empty descriptor
    t1, t2 = gpu(b1.view(np.int32)), gpu(b2.view(np.int32))
    run = lambda: [t.clone() for t in ops.sinkhorn_bits(t1, t2, True, eps, 1.0, 10, return_duals=True)]
    got = run()
    assert all(bool(torch.isfinite(t).all()) for t in got[1:])
    with N.debug_library() as lib:
        assert lib.mi_debug_set(15, 0) == 0
        want = run()
        assert lib.mi_debug_set(15, 2) != 0
    for x, y in zip(got, want):
        assert torch.equal(x, y)


@pytest.mark.parametrize("batch,n,m,bits", [(33, 700, 1024, 256), (3, 130, 900, 512), (64, 1024, 1024, 512), (2, 1000, 513, 256)])
def test_sinkhorn_wide_rows_split_over_wave_pairs(mods, batch, n, m, bits):
    """512 < m <= 1024: the bounded-shift row kernel gives the two 512-column chunks of a row to two waves (the one-chunk
    code per wave, the half sums of a row meeting in LDS) instead of holding both chunks in one wave.  The sums associate
    differently, nothing else: duals and P agree with the two-chunk kernel (debug key 16 = 0) to rounding, and with the
    fp64 oracle to the usual bound; ragged extents, rows past n in the last band, m = 513 (the right half nearly empty)."""
    from onnx_image_processing_amd import _native as N, ops
    rng = np.random.default_rng(n + m)
    w = bits // 32
    b1 = rng.integers(0, 2 ** 32, size=(batch, n, w), dtype=np.uint64).astype(np.uint32)
    b2 = rng.integers(0, 2 ** 32, size=(batch, m, w), dtype=np.uint64).astype(np.uint32)
    k = min(n, m) // 3
    b2[:, m - k:] = b1[:, :k]                              # the matches sit in the right half
    b1[:, 1] = 0
    t1, t2 = gpu(b1.view(np.int32)), gpu(b2.view(np.int32))
    run = lambda: [t.clone() for t in ops.sinkhorn_bits(t1, t2, True, 0.05, 1.0, 10, return_duals=True)]
    got = run()
    with N.debug_library() as lib:
        assert lib.mi_debug_set(16, 0) == 0
        want = run()
        assert lib.mi_debug_set(16, 2) != 0
    assert all(bool(torch.isfinite(t).all()) for t in got[1:])
    assert float((got[0][:, :n, :m] - want[0][:, :n, :m]).abs().max()) < 3e-5                # P (entries <= 1; an ulp of a dual of magnitude 40 is 4e-6)
    assert float(((got[0] - want[0]).abs() / want[0].clamp_min(1.0)).max()) < 1e-5            # dustbin row / column: up to ~n
    for x, y in zip(got[1:], want[1:]):                                       # duals
        assert float((x - y).abs().max()) < 5e-4
    unpack = lambda b: np.unpackbits(np.ascontiguousarray(b).view(np.uint8), axis=-1, bitorder="little").astype(np.float64)
    d1, d2 = unpack(b1[:1]), unpack(b2[:1])
    d1 /= np.maximum(np.linalg.norm(d1, axis=-1, keepdims=True), 1e-12)
    d2 /= np.maximum(np.linalg.norm(d2, axis=-1, keepdims=True), 1e-12)
    ref = O.sinkhorn_match(d1, d2, 10, 0.05, 1.0, dtype=np.float64)
    assert float(np.abs(got[0][:1, :n, :m].cpu().numpy() - ref[:, :n, :m]).max()) < 1e-4


@pytest.mark.parametrize("batch,n,m", [(3, 512, 512), (2, 300, 277), (2, 33, 1000), (2, 1024, 1024), (1, 5, 3), (9, 130, 512)])
def test_sinkhorn_dots_p_kernel_with_loads_up_front(mods, batch, n, m):
    """The P output of mi_sinkhorn_dots and of mi_sinkhorn: four rows per wave with every load issued before the first use (default) against
    the one-row-per-wave loop (debug key 18 = 0): the same expressions on the same operands, P identical bit for bit --
    core, dustbin row, dustbin column, ragged extents, one and two 512-column chunks, rows past n in the last wave."""
    from onnx_image_processing_amd import _native as N, ops
    rng = np.random.default_rng(batch + n + m)
    b1 = rng.integers(0, 2 ** 32, size=(batch, n, 8), dtype=np.uint64).astype(np.uint32)
    b2 = rng.integers(0, 2 ** 32, size=(batch, m, 8), dtype=np.uint64).astype(np.uint32)
    k = min(n, m) // 3
    b2[:, :k] = b1[:, :k]
    t1, t2 = gpu(b1.view(np.int32)), gpu(b2.view(np.int32))
    def run():
        out = [ops.sinkhorn_bits(t1, t2, True, 0.05, 1.0, 6).clone()]
        z, pitch = ops.cost_logscores_bits(t1, t2, True, 0.05)          # the fp32-Z form's P kernel (mi_sinkhorn)
        out.append(ops.sinkhorn(z, m, pitch, -1.0 / 0.05, 6).clone())
        return out
    got = run()
    with N.debug_library() as lib:
        assert lib.mi_debug_set(18, 0) == 0
        want = run()
        assert lib.mi_debug_set(18, 2) != 0
    for x, y in zip(got, want):
        assert x.shape == (batch, n + 1, m + 1) and bool(torch.isfinite(x).all())
        assert torch.equal(x, y)


@pytest.mark.parametrize("batch,n,m", [(3, 512, 512), (2, 300, 277), (2, 33, 1000), (2, 1024, 1024), (1, 5, 3), (5, 130, 512)])
def test_mnn_extract_in_one_pass_over_p(mods, batch, n, m):
    """mi_mnn_extract on a materialised P: row and column winners in ONE pass (a band of 32 rows per workgroup, loads up
    front, the columns' winners merged across workgroups by a 64-bit atomic maximum) against the row kernel + column
    kernel pair (debug key 19 = 0).  Winners are exact maxima of (score, index) keys: every output identical -- with
    exact ties (duplicated rows and columns), all-zero rows, ragged extents and two 512-column chunks."""
    from onnx_image_processing_amd import _native as N, ops
    rng = np.random.default_rng(batch * 1000 + n + m)
    pm = rng.random((batch, n + 1, m + 1), dtype=np.float32) ** 8
    pm[:, : min(n, m), : min(n, m)] += np.eye(min(n, m), dtype=np.float32)[None] * (rng.random((batch, min(n, m), 1), dtype=np.float32) > 0.5)
    if n > 4 and m > 4:
        pm[:, 3] = pm[:, 2]                      # exact ties between rows ...
        pm[:, :, 4] = pm[:, :, 1]                # ... and between columns
        pm[:, 1, :] = 0.0                        # an all-zero row
    pt = gpu(pm)
    k1 = gpu(rng.integers(0, 400, (batch, n, 2)).astype(np.float32))
    k2 = gpu(rng.integers(0, 400, (batch, m, 2)).astype(np.float32))
    run = lambda: [t.clone() for t in ops.mnn_extract(pt, k1, k2, 50, 0.05, return_indices=True)]
    got = run()
    with N.debug_library() as lib:
        assert lib.mi_debug_set(19, 0) == 0
        want = run()
        assert lib.mi_debug_set(19, 2) != 0
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    assert int(got[3].sum()) > 0


@pytest.mark.parametrize("n,m", [(300, 280), (520, 700)])
def test_fp32_sinkhorn_stream_schedules_agree(mods, n, m):
    """mi_sinkhorn (fp32 log-scores: float descriptors, the reference's default configuration) for >= 64 pairs runs as
    two half batches on two streams too since round 4, scheduled by the same per-stream tuner under a shape key of its
    own: duals and P of every fixed schedule (debug key 11), of the tuner's trial calls and of its decision are identical,
    the decision of the packed solver for the same (batch, n, m, iterations) is a different entry, a pin applies to
    both solvers, and a replayed capture of the call (unsplit: its stream's tuner has not decided) gives the same P."""
    from onnx_image_processing_amd import _native as N, ops
    from onnx_image_processing_amd.graph import GraphedModule
    rng = np.random.default_rng(n + m)
    d1 = rng.standard_normal((70, n, 64)).astype(np.float32)
    d2 = rng.standard_normal((70, m, 64)).astype(np.float32)
    d2[:, :100] = d1[:, :100] + 0.05 * rng.standard_normal((70, 100, 64)).astype(np.float32)
    d1 /= np.linalg.norm(d1, axis=-1, keepdims=True)
    d2 /= np.linalg.norm(d2, axis=-1, keepdims=True)
    z, pitch = ops.cost_logscores_f32(gpu(d1), gpu(d2), 0, 0.1)
    iters = 9
    run = lambda: [t.clone() for t in ops.sinkhorn(z, m, pitch, -10.0, iters, return_duals=True)]
    with N.debug_library() as lib:
        want = None
        for sched in (2, 0, 1):
            assert lib.mi_debug_set(11, sched) == 0
            got = run()
            want = want or got
            for x, y in zip(got, want):
                assert torch.equal(x, y), sched
        assert lib.mi_debug_set(11, -1) == 0
    assert bool(torch.isfinite(want[0]).all()) and float(want[0][:, :-1, :-1].max()) > 0.3
    ops.set_sinkhorn_schedule(ops.MI_SCHEDULE_UNDECIDED)
    for call in range(12):                                       # nine trial calls, then the decided schedule
        for x, y in zip(run(), want):
            assert torch.equal(x, y), call
        torch.cuda.synchronize()
    assert ops.sinkhorn_schedule(70, n, m, iters + (1 << 20)) in (0, 1, 2)        # this solver's own shape key ...
    assert ops.sinkhorn_schedule(70, n, m, iters) == ops.MI_SCHEDULE_UNDECIDED    # ... not the packed solver's
    for pin in (2, 1, 0):
        ops.set_sinkhorn_schedule(pin)
        for x, y in zip(run(), want):
            assert torch.equal(x, y), pin
    ops.set_sinkhorn_schedule(ops.MI_SCHEDULE_UNDECIDED)
    # a capture on a stream whose tuner has not decided records the unsplit schedule (nothing is tried inside a capture)
    graphed = GraphedModule(lambda zz: ops.sinkhorn(zz, m, pitch, -10.0, iters), z)
    for _ in range(2):
        assert torch.equal(graphed(z), want[0])
    assert torch.isfinite(want[0]).all()


def test_cpu_tensor_is_refused(mods):
    with pytest.raises(RuntimeError):
        mods["ShiTomasiScore"](3)(torch.zeros(1, 1, 16, 16))


def test_hipgraph_replay_equals_eager(mods):
    """graph.GraphedModule: the whole wrapper forward captured into one hipGraph replays bit-identically."""
    from onnx_image_processing_amd.graph import GraphedModule
    g = load_golden("small_hamming_96x128_k48")
    cfg = cfg_of(g)
    a, b = _images(g)
    model = mods["MatchExtractionWrapper"](mods["ShiTomasiSparseBADSinkhornMatcher"](max_keypoints=int(g["k"]), **cfg),
                                           max_matches=40, match_threshold=0.1).to(DEV)
    eager = [t.clone() for t in model(gpu(a), gpu(b))]
    graphed = GraphedModule(model, gpu(a), gpu(b))
    for _ in range(3):
        out = graphed(gpu(a), gpu(b))
        for x, y in zip(out, eager):
            assert torch.equal(x, y)
    swapped = [t.clone() for t in graphed(gpu(b), gpu(a))]                       # new inputs through the same graph
    for x, y in zip(swapped, model(gpu(b), gpu(a))):
        assert torch.equal(x, y)
    with pytest.raises(RuntimeError):
        graphed(gpu(a[:, :, :50]), gpu(b))


def test_hipgraph_replay_survives_device_synchronisation(mods):
    """The one-pair-per-call host (the VO loop) synchronises after every replay and launches other work in between.
    A hipMemsetAsync captured into the graph (the library's former way of clearing the Sinkhorn hand-off area and K1's
    ticket counters) zeroed correctly on the first replay only on this stack -- later replays filled the range with a
    recycled argument block, so the solver's status word came back non-zero and every match invalid (round 3; the
    clears are kernels now, csrc/common.h mi_zero_async).  Module path and the one-call path, one pair and a batch
    large enough for K1's ticket schedule."""
    from onnx_image_processing_amd.graph import GraphedModule
    g = load_golden("small_hamming_96x128_k48")
    cfg = cfg_of(g)
    a, b = _images(g)
    model = mods["MatchExtractionWrapper"](mods["ShiTomasiSparseBADSinkhornMatcher"](max_keypoints=int(g["k"]), **cfg),
                                           max_matches=40, match_threshold=0.1).to(DEV)
    noise = torch.empty(1 << 16, dtype=torch.int32, device=DEV)
    for single in (False, True):
        fwd = model.forward_single_call if single else model
        ga, gb = gpu(a), gpu(b)
        eager = [t.clone() for t in fwd(ga, gb)]
        assert int(eager[3].sum()) > 10
        graphed = GraphedModule(fwd, ga, gb)
        for it in range(4):
            out = graphed(ga, gb)
            torch.cuda.synchronize()                                 # the host waits for every call ...
            for x, y in zip(out, eager):
                assert torch.equal(x, y), (single, it)
            noise.fill_(0x55555555 + it)                             # ... and launches something else before the next
            torch.cuda.synchronize()
    # the other models a per-frame host would replay: the visual-odometry model and the AKAZE matcher
    from onnx_image_processing_amd.pytorch_model.feature_detection import (AKAZESparseBADSinkhornMatcher,
                                                                           ShiTomasiAngleSparseBADSinkhornWithEssentialMatrix)
    a1, b1 = synth_batch(9000, 1, 240, 320)
    cam = torch.tensor([[300.0, 0.0, 160.0], [0.0, 300.0, 120.0], [0.0, 0.0, 1.0]])
    vo = ShiTomasiAngleSparseBADSinkhornWithEssentialMatrix(K=cam, max_keypoints=128, block_size=5, num_pairs=512, binarize=True,
                                                            soft_binarize=False, sinkhorn_iterations=10, epsilon=0.05,
                                                            nms_radius=3).to(DEV)
    ak = mods["MatchExtractionWrapper"](AKAZESparseBADSinkhornMatcher(max_keypoints=128, num_pairs=256, binarize=False,
                                                                       sinkhorn_iterations=10, epsilon=0.05, nms_radius=3),
                                        max_matches=40, match_threshold=0.1).to(DEV)
    for m in (vo, ak):
        x1, x2 = gpu(a1), gpu(b1)
        eager = [t.clone() for t in m(x1, x2)]
        graphed = GraphedModule(m, x1, x2)
        for it in range(3):
            out = graphed(x1, x2)
            torch.cuda.synchronize()
            for x, y in zip(out, eager):
                assert torch.equal(x, y), (type(m).__name__, it)
            noise.fill_(it)
            torch.cuda.synchronize()
    # a batch whose corner response takes the ticket schedule (more than two tiles per resident workgroup)
    a2, b2 = synth_batch(9100, 40, 480, 640)
    m2 = mods["MatchExtractionWrapper"](mods["ShiTomasiSparseBADSinkhornMatcher"](max_keypoints=128, **cfg),
                                        max_matches=40, match_threshold=0.1).to(DEV)
    g1, g2 = gpu(a2), gpu(b2)
    eager = [t.clone() for t in m2(g1, g2)]
    graphed = GraphedModule(m2, g1, g2)
    for it in range(3):
        out = graphed(g1, g2)
        torch.cuda.synchronize()
        for x, y in zip(out, eager):
            assert torch.equal(x, y), it
        noise.fill_(it)
        torch.cuda.synchronize()


def test_host_threads_on_their_own_streams(mods):
    """Four host threads, each with its own stream and its own model instance, run one-pair forwards (ctypes releases the
    GIL: the C entry points really run concurrently -- the helper-stream registry, the occupancy cache, the BAD plan
    cache and the single-launch Sinkhorn's workgroups of four calls sharing the device) and every result equals the
    single-threaded one."""
    import threading
    g = load_golden("small_hamming_96x128_k48")
    cfg = cfg_of(g)
    a, b = _images(g)
    make = lambda: mods["MatchExtractionWrapper"](mods["ShiTomasiSparseBADSinkhornMatcher"](max_keypoints=int(g["k"]), **cfg),
                                                  max_matches=40, match_threshold=0.1).to(DEV)
    want = [t.clone() for t in make()(gpu(a), gpu(b))]
    torch.cuda.synchronize()
    errors = []

    def worker(tid):
        try:
            model = make()
            stream = torch.cuda.Stream()
            x, y = gpu(a), gpu(b)
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                for it in range(40):
                    out = model(x, y) if (it + tid) % 2 else model.forward_single_call(x, y)
                    stream.synchronize()
                    for o, w in zip(out, want):
                        if not torch.equal(o, w):
                            errors.append((tid, it))
                            return
        except Exception as e:                                   # noqa: BLE001 -- reported by the assertion below
            errors.append((tid, repr(e)))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def _wrapper_96(mods, k=48):
    cfg = dict(block_size=3, num_pairs=256, binarize=True, soft_binarize=False, sinkhorn_iterations=10, epsilon=0.1,
               nms_radius=2)
    return mods["MatchExtractionWrapper"](mods["ShiTomasiSparseBADSinkhornMatcher"](max_keypoints=k, **cfg),
                                          max_matches=40, match_threshold=0.1).to(DEV)


@pytest.mark.parametrize("form", ["pinned_fork", "undecided", "no_fork_flag"])
def test_hipgraph_replay_through_the_forked_streams(mods, form):
    """64 pairs per call: mi_sinkhorn_dots can run the two half-batches on its helper stream (fork/join by events).
    pinned_fork: the capture stream's schedule is pinned to {caller, helper}: the capture has to follow that fork and
    the replay has to equal the eager result.  undecided: a capture taken before the tuner has
    decided records the UNSPLIT schedule -- no cross-stream branch in the graph.  no_fork_flag:
    MI_SOLVER_NO_FORK rules the fork out even where a forking schedule is pinned."""
    from onnx_image_processing_amd import ops
    from onnx_image_processing_amd.graph import GraphedModule
    if form == "pinned_fork" and os.environ.get("GPU_MAX_HW_QUEUES") == "1":
        # ROCm 7.2's hipGraphLaunch segfaults (hip::Graph::UpdateStreams <- hip::GraphExec::Run) on ANY captured graph with
        # a cross-stream branch when the device has one hardware queue -- four torch kernels suffice
        # (tools/graph_fork_probe.py torch; DESIGN.md "forked graphs").  The other two forms are the product's way out.
        pytest.skip("runtime bug: hipGraphLaunch of a forked capture with GPU_MAX_HW_QUEUES=1")
    a, b = synth_batch(8800, 64, 96, 128)
    model = _wrapper_96(mods)
    eager = [t.clone() for t in model(gpu(a), gpu(b))]
    assert int(eager[3].sum()) > 64 * 10

    def before_capture():                              # runs on the capture stream, after the warm-up calls
        if form == "undecided":
            ops.set_sinkhorn_schedule(ops.MI_SCHEDULE_UNDECIDED)
        else:
            ops.set_sinkhorn_schedule(ops.MI_SCHEDULE_CALLER_HELPER)

    if form == "no_fork_flag":
        ops.set_solver_flags(ops.MI_SOLVER_NO_FORK)
    try:
        graphed = GraphedModule(model, gpu(a), gpu(b), before_capture=before_capture, debug=True)
    finally:
        ops.set_solver_flags(ops.MI_SOLVER_DEFAULT)
    from onnx_image_processing_amd.graph import graph_topology
    topo = graph_topology(graphed.graph)
    if os.environ.get("MI_REPORT"):
        print(f"[graph topology, {form}] {topo}")
    assert topo["nodes"] >= 30 and topo["edges"] >= topo["nodes"] - 1      # (unsplit: 30 nodes since both images share the front end's launches)
    assert (topo["forks"] > 0) == (form == "pinned_fork") and (topo["joins"] > 0) == (form == "pinned_fork"), (form, topo)
    for _ in range(2):
        for x, y in zip(graphed(gpu(a), gpu(b)), eager):
            assert torch.equal(x, y)
    swapped = [t.clone() for t in graphed(gpu(b), gpu(a))]
    for x, y in zip(swapped, model(gpu(b), gpu(a))):
        assert torch.equal(x, y)


def _preallocated_sinkhorn_call(seed=1, batch=64, n=96, m=96, iterations=10):
    """(call, duals): call() enqueues mi_sinkhorn_dots for `batch` pairs on torch's current stream using buffers
    allocated HERE -- no allocation inside, so it can run while another thread holds a capture open (torch.cuda.graph
    empties the allocator's cache on entry; a fresh hipMalloc under a global-mode capture is refused)."""
    from onnx_image_processing_amd import _native as N, ops
    rng = np.random.default_rng(seed)
    b1 = gpu(rng.integers(0, 2 ** 31, size=(batch, n, 8)).astype(np.int32))
    b2 = gpu(rng.integers(0, 2 ** 31, size=(batch, m, 8)).astype(np.int32))
    _, u0, v0, (dots, ri, ci, pitch, (work, _)) = ops.sinkhorn_bits(b1, b2, True, 0.05, 1.0, iterations, want_p=False,
                                                                   return_state=True)
    want = (u0.clone(), v0.clone())
    u, v = torch.empty_like(u0), torch.empty_like(v0)
    wbytes = work.numel() * 8

    def call():
        N.call("mi_sinkhorn_dots", dots.data_ptr(), ri.data_ptr(), ci.data_ptr(), batch, n, m, pitch, 0.05, 1.0, 1.0,
               iterations, u.data_ptr(), v.data_ptr(), None, work.data_ptr(), wbytes, ops._solver_flags, N.stream_ptr())
        return u, v

    return call, want, (batch, n, m, iterations)


def test_tuner_trials_while_another_thread_captures(mods):
    """Thread A is inside a torch.cuda.graph capture (GLOBAL capture mode, torch's default) while thread B makes the
    first calls of a shape on its own stream -- the calls whose hipEventRecord / hipEventQuery the schedule tuner issues
    on B's thread.  Under another thread's global-mode capture hipEventQuery is refused AND INVALIDATES that capture
    (tools/capture_mode_probe.py: hipEventQuery INVALIDATED, with hipThreadExchangeStreamCaptureMode(relaxed) SURVIVED);
    the library makes them in relaxed mode (csrc/sinkhorn_dots.hip, RelaxedCaptureMode): both threads must succeed, A's
    replay and B's duals must equal the eager ones (VERDICT r3 next #3c).  B calls the C ABI on preallocated buffers:
    torch's own allocator may not hipMalloc while A captures."""
    import threading
    from onnx_image_processing_amd import ops
    from onnx_image_processing_amd.graph import GraphedModule
    model = _wrapper_96(mods)
    a, b = synth_batch(8850, 64, 96, 128)
    ga, gb = gpu(a), gpu(b)
    want = [t.clone() for t in model(ga, gb)]
    sb = torch.cuda.Stream()
    sb.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(sb):
        call, want_duals, shape = _preallocated_sinkhorn_call()
        call()                                                     # creates B's helper streams
        sb.synchronize()
        ops.set_sinkhorn_schedule(ops.MI_SCHEDULE_UNDECIDED)       # the tuner's first calls will happen during A's capture
        assert ops.sinkhorn_schedule(*shape) == ops.MI_SCHEDULE_UNDECIDED
    torch.cuda.synchronize()
    in_capture, b_done, errors, box = threading.Event(), threading.Event(), [], {}

    def thread_b():
        try:
            in_capture.wait(60)
            with torch.cuda.stream(sb):
                for _ in range(12):                                # nine trial calls (event records + queries), then more
                    box["duals"] = call()
                box["during"] = ops.sinkhorn_schedule(*shape)      # harvests with hipEventQuery, still inside A's capture
        except Exception as e:      # noqa: BLE001
            errors.append(e)
        finally:
            b_done.set()

    def hold_capture_open():                                       # called on A's capture stream, inside the capture
        in_capture.set()
        b_done.wait(120)

    t = threading.Thread(target=thread_b)
    t.start()
    try:
        graphed = GraphedModule(model, ga, gb, inside_capture=hold_capture_open)
    finally:
        in_capture.set()
        t.join(180)
    assert not errors, errors
    sb.synchronize()
    with torch.cuda.stream(sb):
        for _ in range(2):                                         # harvest what is left: the window closes
            call()
            sb.synchronize()
        assert ops.sinkhorn_schedule(*shape) in (0, 1, 2)
        ops.set_sinkhorn_schedule(ops.MI_SCHEDULE_UNDECIDED)
    for x, y in zip(box["duals"], want_duals):
        assert torch.equal(x, y)
    for x, y in zip(graphed(ga, gb), want):
        assert torch.equal(x, y)


def test_two_host_threads_on_two_streams(mods):
    """Two host threads, each on its own torch stream, 64 pairs per call (the forked Sinkhorn schedule): every
    caller stream owns its helper streams and events, so the threads cannot cross each other's fork/join
    (ADVICE r1 medium).  Results must equal the single-threaded ones, call after call."""
    import threading
    from onnx_image_processing_amd import _native as N
    model = _wrapper_96(mods)
    data = [synth_batch(8900 + 100 * t, 64, 96, 128) for t in range(2)]
    inputs = [(gpu(a), gpu(b)) for a, b in data]
    want = [[t.clone() for t in model(*inp)] for inp in inputs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(2)]
    errors = []

    def worker(t):
        try:
            with torch.cuda.stream(streams[t]):
                for _ in range(12):
                    got = model(*inputs[t])
                    streams[t].synchronize()
                    for x, y in zip(got, want[t]):
                        if not torch.equal(x, y):
                            raise AssertionError(f"thread {t}: result differs from the single-threaded run")
        except Exception as e:      # noqa: BLE001
            errors.append(e)

    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    threads = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for s in streams:               # the helper streams can be handed back (and are re-created on demand)
        N.call("mi_release_stream_resources", s.cuda_stream)
    with torch.cuda.stream(streams[0]):
        got = model(*inputs[0])
    streams[0].synchronize()
    for x, y in zip(got, want[0]):
        assert torch.equal(x, y)


def test_corner_ticket_schedule_equals_static(mods):
    """mi_corner_response_balanced on a batch large enough for the ticket schedule (> 2 tiles per persistent workgroup):
    the score map is the static schedule's (mi_corner_response / _u8) bit for bit, the counter block is left zero, and
    a second call on the same block gives the same map; rows of the oracle spot-checked."""
    from onnx_image_processing_amd import _native as N, ops
    n, h, w = 120, 480, 640                                      # 9,000 tiles of 128 x 32 on 1,024 workgroups
    base = np.stack([synth_image(900 + i, h, w) for i in range(6)])[:, None]
    img8 = gpu(np.tile(base, (n // 6, 1, 1, 1)))
    ctr = torch.zeros(ops.TILE_COUNTER_BYTES // 4, dtype=torch.int32, device=DEV)
    for x, u8, static in ((img8.float(), 0, "mi_corner_response"), (img8, 1, "mi_corner_response_u8")):
        want = torch.empty((n, 1, h, w), dtype=torch.float32, device=DEV)
        N.call(static, x.data_ptr(), n, h, w, 3, want.data_ptr(), N.stream_ptr())
        for _ in range(6):                                       # repeated: the hand-off of a ticket between waves is timing dependent
            got = torch.full((n, 1, h, w), -1.0, dtype=torch.float32, device=DEV)
            N.call("mi_corner_response_balanced", x.data_ptr(), u8, n, h, w, 3, got.data_ptr(), ctr.data_ptr(), N.stream_ptr())
            assert torch.equal(got, want)
            assert int(ctr.abs().sum()) == 0
    assert np.array_equal(want[:6].cpu().numpy(), O.shi_tomasi_score(base.astype(np.float32), 3))
    # the bench's own batch (448 frames, where round 2's fault appeared): ONE extra launch per pixel type
    n = 448
    img8 = gpu(np.tile(base, (n // 6 + 1, 1, 1, 1))[:n])
    for x, u8, static in ((img8.float(), 0, "mi_corner_response"), (img8, 1, "mi_corner_response_u8")):
        want = torch.empty((n, 1, h, w), dtype=torch.float32, device=DEV)
        N.call(static, x.data_ptr(), n, h, w, 3, want.data_ptr(), N.stream_ptr())
        got = torch.full((n, 1, h, w), -1.0, dtype=torch.float32, device=DEV)
        N.call("mi_corner_response_balanced", x.data_ptr(), u8, n, h, w, 3, got.data_ptr(), ctr.data_ptr(), N.stream_ptr())
        assert torch.equal(got, want)
        del want, got


@pytest.mark.parametrize("bs", [5, 7])
def test_corner_blocks_5_and_7_streaming_kernel_equals_tile_kernel(mods, bs):
    """Blocks 5 and 7 run the streaming LDS-DMA kernel since round 4 (same stencil as the register-staged tile kernel,
    debug key 1 = 1): identical score maps on shapes with partial tiles, on a batch small enough for the static tile
    schedule and on one large enough for tickets (repeated: the ticket hand-off is timing dependent), counter left zero."""
    from onnx_image_processing_amd import _native as N, ops
    for n, h, w, reps in ((3, 100, 200, 1), (1, 37, 64, 1), (150, 240, 384, 4)):
        base = np.stack([synth_image(950 + i, h, w) for i in range(3)])[:, None].astype(np.float32)
        x = gpu(np.tile(base, ((n + 2) // 3, 1, 1, 1))[:n])
        with N.debug_library() as lib:
            lib.mi_debug_set(1, 1)
            want = ops.corner_response(x, bs)
        ctr = torch.zeros(ops.TILE_COUNTER_BYTES // 4, dtype=torch.int32, device=DEV)
        for _ in range(reps):
            got = torch.full((n, 1, h, w), -1.0, dtype=torch.float32, device=DEV)
            N.call("mi_corner_response_balanced", x.data_ptr(), 0, n, h, w, bs, got.data_ptr(), ctr.data_ptr(), N.stream_ptr())
            assert torch.equal(got, want), (n, h, w)
            assert int(ctr.abs().sum()) == 0
        got = torch.empty((n, 1, h, w), dtype=torch.float32, device=DEV)
        N.call("mi_corner_response", x.data_ptr(), n, h, w, bs, got.data_ptr(), N.stream_ptr())       # no counter: static
        assert torch.equal(got, want)


def test_corner_dirty_tile_counter_is_harmless(mods):
    """A counter block left dirty (a launch that died between its first draw and the last workgroup's reset) must not
    make later calls skip tiles: the launcher clears the block on the stream ahead of the kernel.
    Garbage of three kinds -- mid-range tickets, huge tickets, a wrong `done` count -- still gives the static map."""
    from onnx_image_processing_amd import _native as N, ops
    n, h, w = 120, 480, 640
    base = np.stack([synth_image(910 + i, h, w) for i in range(6)])[:, None]
    img8 = gpu(np.tile(base, (n // 6, 1, 1, 1)))
    words = ops.TILE_COUNTER_BYTES // 4
    for x, u8, static in ((img8.float(), 0, "mi_corner_response"), (img8, 1, "mi_corner_response_u8")):
        want = torch.empty((n, 1, h, w), dtype=torch.float32, device=DEV)
        N.call(static, x.data_ptr(), n, h, w, 3, want.data_ptr(), N.stream_ptr())
        for fill in (37, 0x7FFFFFF0, -1):
            ctr = torch.full((words,), fill, dtype=torch.int32, device=DEV)
            got = torch.full((n, 1, h, w), -1.0, dtype=torch.float32, device=DEV)
            N.call("mi_corner_response_balanced", x.data_ptr(), u8, n, h, w, 3, got.data_ptr(), ctr.data_ptr(), N.stream_ptr())
            assert torch.equal(got, want), fill
            assert int(ctr.abs().sum()) == 0
    # the module path allocates its block per call (uninitialised memory): same map
    assert torch.equal(ops.corner_response(img8, 3), want)


def _poison_setup(batch=2, n=96, m=80):
    from onnx_image_processing_amd import ops
    rng = np.random.default_rng(4242)
    b1 = rng.integers(0, 2 ** 32, size=(batch, n, 8), dtype=np.uint64).astype(np.uint32)
    b2 = rng.integers(0, 2 ** 32, size=(batch, m, 8), dtype=np.uint64).astype(np.uint32)
    b2[:, :40] = b1[:, :40]
    k1 = gpu(rng.integers(0, 200, size=(batch, n, 2)).astype(np.float32))
    k2 = gpu(rng.integers(0, 200, size=(batch, m, 2)).astype(np.float32))
    p, u, v, state = ops.sinkhorn_bits(gpu(b1.view(np.int32)), gpu(b2.view(np.int32)), True, 0.05, 1.0, 10,
                                       return_state=True, want_p=False)
    return u, v, state, k1, k2, m


def test_timed_out_solver_is_loud_not_garbage(mods):
    """What a hand-off time-out of the single-launch Sinkhorn leaves behind (status word != 0, NaN duals) must come out
    as "no matches", never as plausible wrong ones and never as an out-of-bounds read:
    (a) a healthy call: status word 0, matches found; (b) the status word alone forces valid = 0 for every match of
    the call; (c) NaN duals alone (no status word handed over) give no winner anywhere: valid = 0, indices -1;
    (d) a NaN row inside an otherwise healthy P through mi_mnn_extract loses only that row."""
    from onnx_image_processing_amd import ops
    u, v, state, k1, k2, m = _poison_setup()
    assert _status_word(state) == 0
    good = ops.mnn_from_duals_dots(state, m, 0.05, u, v, k1, k2, 30, 0.1, return_indices=True)
    assert int(good[3].sum()) >= 2 * 20
    work, addr = state[4]
    word = work.view(torch.int32)[(addr - work.data_ptr()) // 4:(addr - work.data_ptr()) // 4 + 1]
    word.fill_(1)                                                # (b)
    mk1, mk2, sc, valid, ij = ops.mnn_from_duals_dots(state, m, 0.05, u, v, k1, k2, 30, 0.1, return_indices=True)
    assert int(valid.sum()) == 0 and bool((ij == -1).all()) and bool((sc <= 0).all())
    word.fill_(0)
    again = ops.mnn_from_duals_dots(state, m, 0.05, u, v, k1, k2, 30, 0.1, return_indices=True)
    for x, y in zip(again, good):
        assert torch.equal(x, y)
    un, vn = u.clone(), v.clone()                                # (c): pair 0 poisoned, pair 1 healthy
    un[0].fill_(float("nan"))
    vn[0].fill_(float("nan"))
    mk1, mk2, sc, valid, ij = ops.mnn_from_duals_dots(state[:4], m, 0.05, un, vn, k1, k2, 30, 0.1, return_indices=True)
    assert int(valid[0].sum()) == 0 and bool((ij[0] == -1).all())
    assert torch.equal(valid[1], good[3][1]) and torch.equal(ij[1], good[4][1]) and torch.equal(sc[1], good[2][1])


def test_small_call_on_one_stream_while_another_stream_runs_the_batched_step(mods):
    """The header's contract: calls on different streams may run concurrently.  A one-pair and an eight-pair call (the
    single-launch Sinkhorn, whose bands hand column sums to each other inside the launch) are issued on stream A while
    stream B is busy with 448-pair steps; A's results must be the single-stream results and its solver status 0
    (VERDICT r2 next #2).  One process, one run."""
    from onnx_image_processing_amd import ops
    from onnx_image_processing_amd.synth import synth_batch_u8
    cfg = dict(block_size=3, num_pairs=512, binarize=True, soft_binarize=False, sinkhorn_iterations=20, epsilon=0.05,
               nms_radius=5)
    model = mods["MatchExtractionWrapper"](mods["ShiTomasiSparseBADSinkhornMatcher"](max_keypoints=512, **cfg),
                                           max_matches=100, match_threshold=0.1).to(DEV)
    a8, b8 = synth_batch_u8(2000, 448, 480, 640)
    big1, big2 = gpu(a8), gpu(b8)
    small = [(big1[:1].clone(), big2[:1].clone()), (big1[8:16].clone(), big2[8:16].clone())]
    want_small = [[t.clone() for t in model.forward_single_call(x, y)] for x, y in small]
    want_mod = [[t.clone() for t in model(x, y)] for x, y in small]
    want_big = [t.clone() for t in model(big1, big2)]
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    got_small, got_mod = [], []
    with torch.cuda.stream(sb):
        for _ in range(6):
            got_big = model(big1, big2)
    with torch.cuda.stream(sa):
        for _ in range(3):
            for x, y in small:
                got_small.append(model.forward_single_call(x, y))
                got_mod.append(model(x, y))
        bits = [gpu(np.random.default_rng(3).integers(0, 2 ** 32, size=(8, 512, 16), dtype=np.uint64).astype(np.uint32).view(np.int32))] * 2
        state = ops.sinkhorn_bits(*bits, True, 0.05, 1.0, 20, return_state=True, want_p=False)[3]
    with torch.cuda.stream(sb):
        for _ in range(2):
            got_big = model(big1, big2)
    torch.cuda.synchronize()
    for i, (g, gm) in enumerate(zip(got_small, got_mod)):
        for x, y in zip(g, want_small[i % 2]):
            assert torch.equal(x, y)
        for x, y in zip(gm, want_mod[i % 2]):
            assert torch.equal(x, y)
    for x, y in zip(got_big, want_big):
        assert torch.equal(x, y)
    assert _status_word(state) == 0


@pytest.mark.parametrize("shape,k,normalize", [((3, 480, 640), 512, True), ((2, 120, 160), 96, True),
                                               ((1, 97, 132), 64, False), ((2, 240, 320), 256, True),
                                               ((40, 120, 160), 96, True), ((36, 480, 640), 512, True)])
def test_match_pairs_single_call_equals_module_path(mods, shape, k, normalize):
    """mi_match_pairs (one call, caller-provided workspace) against MatchExtractionWrapper.forward, which issues
    the same entry points one by one: keypoints, matches, scores and validity identical bit for bit.  Up to 32 pairs
    both images of every pair share one launch per stage; the last two cases take the other branch (one image side
    per launch, the 36 x 640x480 one with K1's ticket counters carved out of the workspace)."""
    n, h, w = shape
    a, b = synth_batch(4000 + h, n, h, w)
    model = mods["MatchExtractionWrapper"](
        mods["ShiTomasiSparseBADSinkhornMatcher"](max_keypoints=k, num_pairs=512, binarize=True, soft_binarize=False,
                                                  sinkhorn_iterations=20, epsilon=0.05 if normalize else 8.0,
                                                  unused_score=1.0 if normalize else 40.0,
                                                  normalize_descriptors=normalize),
        max_matches=100 if k >= 100 else k, match_threshold=0.1).to(DEV)
    ref = model(gpu(a), gpu(b))
    kp1, kp2, _ = model.feature_matcher(gpu(a), gpu(b))
    got = model.forward_single_call(gpu(a), gpu(b), want_keypoints=True)
    assert torch.equal(got[0], kp1) and torch.equal(got[1], kp2)
    for x, y in zip(got[2:], ref):
        assert torch.equal(x, y)
    assert int(ref[3].sum()) > 0
    if h * w >= 480 * 640 or n >= 33:                           # uint8 frames through mi_match_pairs_u8, both branches
        got8 = model.forward_single_call(gpu(a.astype(np.uint8)), gpu(b.astype(np.uint8)), want_keypoints=True)
        for x, y in zip(got8, got):
            assert torch.equal(x, y)


def test_match_pairs_argument_checks(mods):
    import ctypes
    from onnx_image_processing_amd import _native as N, ops
    m = mods["SparseBAD"](512, binarize=True, soft_binarize=False).to(DEV)
    prm = N.MatchParams(3, 5, 2000, 0.0, 7, 512, m.pair_geom.data_ptr(), m.pair_thr.data_ptr(), None, 1, 0.05, 1.0, 20, 100, 0.1)
    assert N.load().mi_match_pairs_workspace_bytes(1, 480, 640, ctypes.byref(prm)) == 0        # K > 1024
    prm.max_keypoints = 512
    need = N.load().mi_match_pairs_workspace_bytes(2, 480, 640, ctypes.byref(prm))
    assert need > 2 * 480 * 640 * 4
    img = torch.zeros(2, 1, 480, 640, device=DEV)
    small = torch.empty(1024, dtype=torch.int64, device=DEV)
    out = torch.empty(2 * 512 * 2, device=DEV)
    rc = N.load().mi_match_pairs(img.data_ptr(), img.data_ptr(), 2, 480, 640, ctypes.byref(prm), out.data_ptr(), out.data_ptr(),
                                 out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), None, small.data_ptr(),
                                 small.numel() * 8, None)
    assert rc == -4                                                                      # MI_E_CAPACITY
    with pytest.raises(RuntimeError):
        mods["MatchExtractionWrapper"](mods["ShiTomasiSparseBADSinkhornMatcher"](max_keypoints=64)).to(DEV) \
            .forward_single_call(img, img)                                               # soft descriptors: not covered


def _run_bench(extra_args, forced: bool):
    """bench.py as the driver runs it (a fresh process, stdout = the JSON line); forced: MI_BENCH_FORCE_DIST=1."""
    import json
    import socket
    import subprocess
    import sys
    with socket.socket() as sck:
        sck.bind(("127.0.0.1", 0))
        port = sck.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MI_BENCH_FORCE_DIST"):
        env.pop(k, None)
    if forced:
        env["MI_BENCH_FORCE_DIST"] = "1"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--cpu-pairs", "0", "--no-extras", "--no-side", *extra_args]
    run = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), run.stdout[:500]     # RCCL's version banner goes to stderr
    return json.loads(lines[0])


def test_bench_with_a_forced_rccl_group_of_one():
    """bench.py itself with MI_BENCH_FORCE_DIST=1: the N-rank control flow of the script (process group joined after the
    pre-warm, barriers, the pipelined gather of every step's records, the per-rank facts) on real RCCL with one rank.
    stdout must hold exactly the JSON line and the line must say what it ran on.  (The RATE against a run without a
    group is tests/test_gpu_perf.py, `-m gpu_perf`: a busy box must not fail the correctness suite.)"""
    line = _run_bench(["--steps", "30", "--warmup", "5"], forced=True)
    assert line["backend"] == "nccl" and line["ranks_seen"] == 1 and line["n_gpus"] == 1
    assert line["config"]["result_gather"].startswith("FORCED group of one rank")
    assert line["config"]["mean_valid_matches_per_pair"] > 50
    assert line["sinkhorn_schedule"] in (0, 1, 2)                # the tuner decided during the untimed steps


def test_bench_vo_stream_form_with_a_forced_rccl_group_of_one():
    """`bench.py --workload vo --stream` (BASELINE configs[4] as sample/visual_odometry.py:520-545 runs it: ONE pair per
    call per rank, hipGraph replay, host synchronised after every call, the 100 matches + E gathered to rank 0 per call,
    pipelined by one call) on real RCCL with one rank: every call's record arrives, E is finite, the line reports per-rank
    calls per second and what the per-call gather costs."""
    line = _run_bench(["--workload", "vo", "--stream", "--steps", "60", "--warmup", "10", "--full"], forced=True)
    assert line["backend"] == "nccl" and line["ranks_seen"] == 1 and "STREAM form" in line["config"]["workload"]
    assert line["config"]["pairs_per_gpu_per_step"] == 1 and line["config"]["finite_essential_matrices"] == 1
    assert line["config"]["mean_valid_matches_per_pair"] > 50
    st = line["stream"]
    assert len(st["calls_per_sec_per_rank"]) == 1 and st["calls_per_sec_per_rank"][0] > 500
    assert st["record_bytes_per_call"] == 102 * 6 * 4 and st["ms_per_call_without_gather_rank0"] > 0
    assert abs(line["value"] - 1e3 / st["ms_per_call_with_gather"]) < 1e-6 * line["value"]


def test_plain_bench_run_times_exactly_its_steps_and_dumps_the_last_step(tmp_path):
    """A plain run (no --full) is the headline only: set-up, warm-up, EXACTLY --steps timed steps, the last timed step's
    outputs under --dump-outputs, the line -- no per-kernel table, extras, CPU baseline or side workloads.  The dumped
    arrays are the wrapper's outputs for the seeded pairs (every match inside the frame, scores in (0, 1]), and a
    --workload run honours an explicit --steps 500 too (it used to turn 500 into its own default of 50)."""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    out = tmp_path / "dump"
    line = _run_bench(["--steps", "7", "--warmup", "2", "--dump-outputs", str(out)], forced=False)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line
    assert line["steps"] == 7 and line["warmup"] == 2 and line["dtype"] == "f32" and line["higher_is_better"] is True
    assert line["value"] == pytest.approx(448 / (line["ms_per_step"] * 1e-3))
    assert not {"kernels", "roofline", "roofline_other", "u8_ingest", "latency", "cpu_baseline", "side_workloads"} & set(line)
    got = {p.stem: np.load(p) for p in out.glob("*.npy")}
    assert set(got) == {"matched_keypoints0", "matched_keypoints1", "match_scores", "match_valid"}
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["matched_keypoints0"].shape == (448, 100, 2) and got["match_valid"].shape == (448, 100)
    v = got["match_valid"] > 0.5
    assert got["match_valid"].sum() / 448 == pytest.approx(line["config"]["mean_valid_matches_per_pair"])
    assert v.sum() > 448 * 50 and (got["match_scores"][v] > 0).all() and (got["match_scores"][v] <= 1).all()
    for key in ("matched_keypoints0", "matched_keypoints1"):
        yx = got[key][v]                               # keypoints are (y, x)
        assert (yx >= 0).all() and (yx[:, 0] < 480).all() and (yx[:, 1] < 640).all()
    okw = {k: v for k, v in bench.CFG.items() if k not in ("num_pairs", "sampling_mode")}
    box, thr = bad_tables(512)
    for i in (0, 447):                                 # first and last pair: the records are in pair order
        a, b = synth_batch(1000 + i, 1, 480, 640)
        k1, k2, p = O.match_pair(a, b, box, thr, 512, **okw)
        mk1, mk2, sc, valid, _ = O.mnn_extract(p, k1, k2, **bench.MNN)
        want = {(*map(float, mk1[0, j]), *map(float, mk2[0, j])): float(sc[0, j]) for j in np.nonzero(valid[0])[0]}
        g = {(*map(float, got["matched_keypoints0"][i, j]), *map(float, got["matched_keypoints1"][i, j])):
             float(got["match_scores"][i, j]) for j in np.nonzero(v[i])[0]}
        assert bench.compare_match_sets(g, want, bench.MNN["max_matches"]) < 2, i
    side = _run_bench(["--workload", "c4", "--pairs-per-gpu", "8", "--steps", "500", "--warmup", "1",
                       "--dump-outputs", str(tmp_path / "c4")], forced=False)
    assert side["steps"] == 500 and "kernels" not in side and "roofline" not in side
    assert np.load(tmp_path / "c4" / "match_valid.npy").shape == (8, 100)


def test_rccl_process_group_of_one_runs_the_gather_path(tmp_path):
    """The N > 1 code of bench.py -- init_process_group(backend "nccl" = RCCL), gather of match records, max-over-ranks
    reduction, per-rank facts, barriers, teardown -- on real hardware.  A one-GPU box cannot host two RCCL ranks, so the
    group has ONE rank (distributed.init(force=True)): every collective call, tensor placement and argument the N-rank run
    makes is exercised, only the peer traffic is missing (that half is covered by the world-2 gloo tests).  Runs in a
    fresh child process (its own rendezvous port and process group)."""
    import socket
    import subprocess
    import sys as _sys
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    code = """
import os, sys, json
sys.path.insert(0, %r)
import torch, torch.distributed as dist
import bench
from onnx_image_processing_amd import distributed as D
rank, world, local = D.init(force=True)
assert dist.is_initialized() and dist.get_backend() == "nccl" and dist.get_world_size() == 1
dev = torch.device("cuda", local)
rec = torch.rand(5, 100, 6, device=dev)
out = D.gather_records(rec, dst=0, total=5)
assert out is not None and torch.equal(out, rec)
out2 = D.gather_records(rec, dst=0, collective="all_gather")
assert torch.equal(out2, rec)
assert D.barrier_max_ms(12.5, dev) == 12.5
calls = []
gather = bench.PipelinedGather(total=5)                       # the bench's own form: one gather in flight
def step():
    calls.append(1)
    return gather(rec * len(calls))
elapsed, per_step, last, own = bench.run_timed(step, steps=3, warmup=1, world=2, device=dev, sync=torch.cuda.synchronize,
                                               drain=gather.drain)
facts = bench.world_facts(own, 3, dev)
assert len(per_step) == 3 and torch.equal(last, rec * 4)
dist.barrier()
dist.destroy_process_group()
print(json.dumps(facts))
""" % ROOT
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    r = subprocess.run([_sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    import json as _json
    facts = _json.loads(r.stdout.strip().splitlines()[-1])
    assert facts["ranks_seen"] == 1 and facts["backend"] == "nccl" and len(facts["ms_per_step_per_rank"]) == 1


def test_c_host_without_python_or_torch_gets_the_same_matches(mods, tmp_path):
    """tests/native/host_match_pairs.c -- plain C, hipMalloc'd buffers, the library through dlopen, a workspace full of
    garbage -- run as a child process on the frames and pair table the Python modules get: keypoints, matches, scores and
    validity equal MatchExtractionWrapper's bit for bit (2 pairs: the merged launches and the single-launch Sinkhorn; 40
    pairs: one image side per launch, ticket-scheduled K1, the forked Sinkhorn halves are not reached below 64)."""
    import subprocess
    import sys as _sys
    sys_path_tests = os.path.join(ROOT, "tests")
    if sys_path_tests not in _sys.path:
        _sys.path.insert(0, sys_path_tests)
    from test_host_and_abi import _build_c_host
    from onnx_image_processing_amd import _native as N
    from onnx_image_processing_amd.synth import synth_batch_u8
    exe = _build_c_host(tmp_path)
    cfg = dict(block_size=3, num_pairs=512, binarize=True, soft_binarize=False, sinkhorn_iterations=20, epsilon=0.05,
               nms_radius=5)
    K, Mx = 512, 100
    model = mods["MatchExtractionWrapper"](mods["ShiTomasiSparseBADSinkhornMatcher"](max_keypoints=K, **cfg),
                                           max_matches=Mx, match_threshold=0.1).to(DEV)
    geom = model.feature_matcher.descriptor.pair_geom.cpu().numpy().astype(np.uint32)
    thr = model.feature_matcher.descriptor.pair_thr.cpu().numpy().astype(np.float32)
    for batch in (2, 40):
        a8, b8 = synth_batch_u8(5100, batch, 480, 640)
        fin, fout = str(tmp_path / f"in{batch}.bin"), str(tmp_path / f"out{batch}.bin")
        with open(fin, "wb") as f:
            f.write(np.array([batch, 480, 640, K, 512, Mx], np.int32).tobytes())
            f.write(a8.tobytes()); f.write(b8.tobytes()); f.write(geom.tobytes()); f.write(thr.tobytes())
        r = subprocess.run([exe, N.LIB_PATH, fin, fout], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        raw = open(fout, "rb").read()
        nk, nm, ns = batch * K * 2, batch * Mx * 2, batch * Mx
        fl = np.frombuffer(raw, np.float32, 2 * nk + 2 * nm + ns)
        valid = np.frombuffer(raw, np.uint8, ns, offset=4 * (2 * nk + 2 * nm + ns))
        rcs = np.frombuffer(raw, np.int32, 2, offset=4 * (2 * nk + 2 * nm + ns) + ns)
        assert rcs.tolist() == [0, 0]
        want = [t.cpu().numpy() for t in model.forward_single_call(gpu(a8), gpu(b8), want_keypoints=True)]
        got = (fl[:nk].reshape(batch, K, 2), fl[nk:2 * nk].reshape(batch, K, 2), fl[2 * nk:2 * nk + nm].reshape(batch, Mx, 2),
               fl[2 * nk + nm:2 * nk + 2 * nm].reshape(batch, Mx, 2), fl[2 * nk + 2 * nm:].reshape(batch, Mx),
               valid.reshape(batch, Mx).astype(bool))
        for x, y in zip(got, want):
            assert np.array_equal(x, y), batch
        assert int(valid.sum()) == batch * Mx
