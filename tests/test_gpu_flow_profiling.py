"""GPU: the per-launch timer of the flow bands (EngineBase::timed / timed_gemm around every launch, read back with kernel_stats()).  Profiling
only records events around the launches and copies debug stages aside, so it must not change a byte of a call's outputs; every record lands in a
row with a name (the kernel's symbol or its family's) and with accumulate the rows of two identical calls count every launch twice."""
import numpy as np
import pytest

from prisma_amd import engine, synth

pytestmark = pytest.mark.gpu


def make(band):
    if band == "flow_raft":
        return engine.FlowRaft(synth.raft_weights(seed=4321), device=0)
    return engine.FlowGMFlow(synth.gmflow_weights(seed=2468), device=0)


@pytest.mark.parametrize("band", ["flow_raft", "flow_gmflow"])
def test_profiling_changes_no_byte_and_names_every_launch(band):
    frames = synth.frame_pair_sequence(3, 131, 181, seed=33)      # a ragged 17 x 23 grid (flow_gmflow: padded to 18 x 24)
    net = make(band)
    call = lambda: net.infer_sequence(frames, scale=1.0, iters=2, backward=True)
    plain = call()
    net.set_profiling(timing=True, debug_stages=True)
    timed = call()
    assert len(plain) == len(timed)
    for a, b in zip(plain, timed):
        assert np.array_equal(a, b)
    one = net.kernel_stats()
    assert one
    for row in one:
        assert row["name"] and row["launches"] >= 1, row
    net.set_profiling(timing=True, debug_stages=True, accumulate=True)
    call()
    call()
    two = net.kernel_stats()
    assert [(r["name"], r["launches"]) for r in two] == [(r["name"], 2 * r["launches"]) for r in one]
    net.close()
