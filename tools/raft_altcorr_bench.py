"""flow_raft with and without --alternate_corr on one box in one visit: ms per pair, the engine's kernel statistics and the arena size.
  (a) 8 pairs at 1080p x 0.75, both directions, 12 iterations: one warmed-up context switched default / alternate / default / alternate;
      per mode the median of the timed calls of both visits, kernel ms per pair from pb_get_kernel_stats, arena_bytes
  (b) alternate only: 2 pairs at 2160 x 3840, scale 1.0, both directions, 12 iterations: ms per pair and arena_bytes.  (The default path is
      not run there: its volume is 45 254 246 400 bytes per pair-direction, arithmetic on tests/raft_ref.geometry.)
python tools/raft_altcorr_bench.py            runs each step as a child process under its own time limit and stops at the first that fails
python tools/raft_altcorr_bench.py --step a   one step in this process
AB_REPS timed calls per visit (default 5), AB_TIMEOUT_A / AB_TIMEOUT_B seconds (default 240 / 300)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = int(os.environ.get("AB_REPS", "5"))
ITERS = 12


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def run_step(step):
    import torch
    from prisma_amd import engine, synth
    pairs, H, W, scale = (8, 1080, 1920, 0.75) if step == "a" else (2, 2160, 3840, 1.0)
    frames = torch.from_numpy(synth.frame_pair_sequence(pairs + 1, H, W, seed=150)).cuda()
    sh, sw = engine.flow_out_size(H, W, scale)
    rgb = torch.empty((pairs, 2, sh, sw, 3), dtype=torch.uint8, device="cuda")
    mx = torch.zeros((pairs, 2), dtype=torch.float32, device="cuda")
    net = engine.FlowRaft(synth.raft_weights(seed=4321))
    call = lambda: net.infer_sequence_dev(frames.data_ptr(), pairs + 1, H, W, scale, ITERS, True, 0, rgb.data_ptr(), mx.data_ptr())
    modes = (False, True, False, True) if step == "a" else (True,)
    times, stats, arena = {}, {}, {}
    for alt in modes:
        net.set_alternate_corr(alt)
        net.set_profiling(timing=False)
        call(); net.sync()                                   # re-plans the arena, warms the mode up
        call(); net.sync()
        for _ in range(REPS):
            t0 = time.perf_counter()
            call(); net.sync()
            times.setdefault(alt, []).append((time.perf_counter() - t0) * 1e3 / pairs)
        arena[alt] = net.arena_bytes()
        net.set_profiling(timing=True, accumulate=True)      # per-launch events: a run of its own, not part of the timed calls
        for _ in range(2):
            call(); net.sync()
        stats[alt] = {s["name"]: round(s["ms"] / 2 / pairs, 3) for s in net.kernel_stats()}
    for alt in sorted(times):
        t = times[alt]
        print(json.dumps({"step": step, "frame": [H, W], "scale": scale, "pairs": pairs, "iters": ITERS, "alternate_corr": alt,
                          "ms_per_pair_median": round(median(t), 3), "ms_per_pair_min": round(min(t), 3), "ms_per_pair_max": round(max(t), 3),
                          "timed_calls": len(t), "arena_bytes": arena[alt], "kernel_ms_per_pair": stats[alt]}), flush=True)
    net.close()


def main():
    if "--step" in sys.argv:
        run_step(sys.argv[sys.argv.index("--step") + 1])
        return 0
    for step, limit in (("a", os.environ.get("AB_TIMEOUT_A", "240")), ("b", os.environ.get("AB_TIMEOUT_B", "300"))):
        rc = subprocess.run(["timeout", "-k", "10", limit, sys.executable, os.path.abspath(__file__), "--step", step]).returncode
        if rc:
            print("step %s ended with status %d: stopping" % (step, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
