"""Rate comparisons on a real MI355X: `-m gpu_perf`, on a box nothing else is using.  Not part of `-m gpu` -- a noisy
neighbour must not fail the correctness suite."""
from gpu_common import GPU_PERF
from test_gpu_runtime import _run_bench

# selected by `-m gpu_perf`; a `-m "not gpu"` run on a machine without a GPU (the CPU suite) skips it
pytestmark = GPU_PERF


def test_forced_rccl_group_costs_less_than_seven_percent():
    """Joining the process group BEFORE the first step used to cost the Sinkhorn its stream overlap (175 k instead of
    200 k pairs/s per rank, round 3); bench.py joins after a pre-warm and mi_sinkhorn_dots tunes its stream schedule:
    with a forced RCCL group of one rank and a gather every step the rate stays within 7 % of a run without a group."""
    forced = _run_bench(["--steps", "60", "--warmup", "5"], forced=True)
    plain = _run_bench(["--steps", "60", "--warmup", "5"], forced=False)
    assert forced["value"] > 0.93 * plain["value"], (forced["value"], plain["value"])
