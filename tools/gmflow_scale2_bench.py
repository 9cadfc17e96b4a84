"""flow_gmflow one-scale against the two-scale refinement model on one box in one process: ms per pair (both directions, 1080p clip at
--scale 0.75), the arena of the plan (pb_flow_arena_bytes) and the engine's kernel statistics by family, for one-scale default, one-scale
(4, 1) and two-scale (4, 1), in the protocol of tools/gmflow_local_bench.py:
python tools/gmflow_scale2_bench.py      (AB_PAIRS pairs per call, default 2; AB_REPS timed calls, default 5)"""
import os, sys, json, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from prisma_amd import engine, synth
P, REPS, H, W = int(os.environ.get("AB_PAIRS", "2")), int(os.environ.get("AB_REPS", "5")), 1080, 1920
frames = torch.from_numpy(synth.frame_pair_sequence(P + 1, H, W, seed=150)).cuda()
sh, sw = engine.flow_out_size(H, W, 0.75)
rgb = torch.empty((P, 2, sh, sw, 3), dtype=torch.uint8, device="cuda")
mx = torch.zeros((P, 2), dtype=torch.float32, device="cuda")
for scales, corr, prop in ((1, -1, -1), (1, 4, 1), (2, 4, 1)):
    net = engine.FlowGMFlow(synth.gmflow_weights(seed=2468, num_scales=scales))
    assert net.num_scales == scales
    call = lambda: net.infer_sequence_dev(frames.data_ptr(), P + 1, H, W, 0.75, 1, True, 0, rgb.data_ptr(), mx.data_ptr())
    net.set_matching(corr, prop)
    net.set_profiling(timing=False)
    call(); net.sync()
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call(); net.sync()
        times.append((time.perf_counter() - t0) * 1e3 / P)
    net.set_profiling(timing=True, accumulate=True)
    for _ in range(2):
        call(); net.sync()
    out = {s["name"]: round(s["ms"] / 2 / P, 3) for s in net.kernel_stats()}
    times.sort()
    print(f"scales {scales} corr {corr:2d} prop {prop:2d}  ms/pair median {times[len(times) // 2]:.2f} min {times[0]:.2f} max {times[-1]:.2f}  "
          f"arena {net.arena_bytes() / 2 ** 30:.2f} GiB ({P} pairs)  kernel ms/pair", json.dumps(out), flush=True)
    net.close()
