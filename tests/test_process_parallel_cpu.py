"""CPU: process.py --jobs / --gpus (bands of one input side by side, video bands under torch.distributed.run).  `process.ROOT`
points at a temporary tree whose bands/ holds the real rgba.py and fake GPU bands: each fake notes when it started and ended in a
side folder, sleeps, adds the entries its real script adds to metadata.json through the real bands.common.meta, and exits as an
environment variable says.  Nothing here touches a GPU."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import process  # noqa: E402

FAKES = ("mask_mmdet", "depth_anything", "flow_gmflow", "flow_raft")
FAKE = '''
import copy, os, resource, signal, sys, time
sys.path.insert(0, os.environ["FAKE_REAL_ROOT"])
from bands.common import meta                           # the real one
NAME = os.path.basename(__file__)[:-3]
BAND = "mask" if NAME == "mask_mmdet" else NAME
side = os.environ["FAKE_SIDE"]
open(os.path.join(side, NAME + ".start"), "w").write(repr(time.monotonic()))
how = os.environ.get("FAKE_EXIT_" + NAME, "0")
if how == "abort":
    resource.setrlimit(resource.RLIMIT_CORE, (0, 0))
    os.kill(os.getpid(), signal.SIGABRT)
argv = sys.argv[1:]
folder = argv[argv.index("-i") + 1]
subpath = argv[argv.index("--subpath") + 1] if "--subpath" in argv else ""
data = meta.load_metadata(folder)
loaded = copy.deepcopy(data)
rgba = meta.get_url(folder, data, "rgba")
video = meta.is_video(rgba)
ext = rgba.rsplit(".", 1)[1]
if NAME.startswith("flow"):
    meta.get_target(rgba, data, band=BAND)
    if "--mask" in argv:
        meta.get_target(rgba, data, band=BAND + "_mask")
else:
    meta.get_target(rgba, data, band=BAND, force_extension="png")
time.sleep(0.5)
if NAME == "mask_mmdet":
    data["bands"][BAND] = {"url": BAND + "." + (ext if video else "png"), "ids": ["person", "cat"]}
elif NAME == "depth_anything":
    if video:
        if subpath:
            data["bands"][BAND]["folder"] = subpath
        data["bands"][BAND]["values"] = {"min": {"type": "float", "url": BAND + "_min.csv"}, "max": {"type": "float", "url": BAND + "_max.csv"}}
    else:
        data["bands"][BAND]["values"] = {"min": {"value": 0.25, "type": "float"}, "max": {"value": 80.5, "type": "float"}}
else:
    data["bands"][BAND] = {"url": BAND + "." + ext, "values": {"dist": {"type": "float", "url": BAND + ".csv"}}}
    if subpath:
        data["bands"][BAND]["folder"] = subpath
    if "--backwards" in argv:
        data["bands"][BAND + "_bwd"] = {"url": BAND + "_bwd." + ext}
        if subpath:
            data["bands"][BAND + "_bwd"]["folder"] = subpath + "_bwd"
    if "--mask" in argv:
        data["bands"][BAND + "_mask"] = {"url": BAND + "_mask." + ext}
        if "--backwards" in argv:
            data["bands"][BAND + "_mask_bwd"] = {"url": BAND + "_mask_bwd." + ext}
meta.merge_metadata(folder, data, loaded)
print("fake %s wrote its entries" % NAME)
print("fake %s says so on stderr too" % NAME, file=sys.stderr)
open(os.path.join(side, NAME + ".end"), "w").write(repr(time.monotonic()))
sys.exit(int(how))
'''


@pytest.fixture
def tree(tmp_path, monkeypatch):
    """The temporary ROOT; returns (side folder, clip path, png path)."""
    root = tmp_path / "root"
    (root / "bands").mkdir(parents=True)
    shutil.copy(os.path.join(ROOT, "bands", "rgba.py"), root / "bands" / "rgba.py")
    os.symlink(os.path.join(ROOT, "bands", "common"), root / "bands" / "common")        # rgba.py imports common.* beside itself
    for name in FAKES:
        (root / "bands" / (name + ".py")).write_text(FAKE)
    side = tmp_path / "side"
    side.mkdir()
    monkeypatch.setattr(process, "ROOT", str(root))
    monkeypatch.setenv("FAKE_REAL_ROOT", ROOT)
    monkeypatch.setenv("FAKE_SIDE", str(side))
    monkeypatch.setenv("PRISMA_OVERWRITE", "1")
    monkeypatch.delenv("PRISMA_GPUS", raising=False)
    for name in FAKES:
        monkeypatch.delenv("FAKE_EXIT_" + name, raising=False)
    clip = tmp_path / "clip.npy"
    np.save(clip, np.random.default_rng(0).integers(0, 256, (3, 48, 64, 3), dtype=np.uint8))
    from PIL import Image
    png = tmp_path / "still.png"
    Image.fromarray(np.random.default_rng(1).integers(0, 256, (48, 64, 3), dtype=np.uint8)).save(png)
    return side, clip, png


def _intervals(side):
    out = {}
    for f in os.listdir(side):
        name, kind = f.rsplit(".", 1)
        out.setdefault(name, {})[kind] = float(open(os.path.join(side, f)).read())
    return out


def _clear(side):
    for f in os.listdir(side):
        os.unlink(os.path.join(side, f))


def _overlap(a, b):
    return a["start"] < b["end"] and b["start"] < a["end"]


def test_plan_width():
    assert [process.plan_width(j, g) for j, g in ((1, 1), (3, 1), (3, 8), (3, 16), (3, 32))] == [1, 3, 2, 1, 1]


def test_jobs_overlap_and_the_folder_equals_the_serial_runs(tree, tmp_path):
    side, clip, _ = tree
    process.main(["-i", str(clip), "--output", str(tmp_path / "par"), "--jobs", "3"])
    par = _intervals(side)
    assert sorted(par) == ["depth_anything", "flow_gmflow", "mask_mmdet"]
    names = sorted(par)
    for i in range(3):
        for j in range(i + 1, 3):
            assert _overlap(par[names[i]], par[names[j]]), (names[i], names[j], par)
    assert [os.path.basename(c[1]) for c in process.COMMANDS] == ["rgba.py", "mask_mmdet.py", "depth_anything.py", "flow_gmflow.py"]
    assert process.RESULTS == [("rgba", 0), ("mask_mmdet", 0), ("depth_anything", 0), ("flow_gmflow", 0)]
    _clear(side)
    process.main(["-i", str(clip), "--output", str(tmp_path / "ser"), "--jobs", "1"])
    ser = _intervals(side)
    for i in range(3):
        for j in range(i + 1, 3):
            assert not _overlap(ser[names[i]], ser[names[j]]), (names[i], names[j], ser)
    assert open(tmp_path / "par" / "metadata.json", "rb").read() == open(tmp_path / "ser" / "metadata.json", "rb").read()
    assert sorted(os.listdir(tmp_path / "par")) == sorted(os.listdir(tmp_path / "ser"))       # no log files in the PRISMA folder


@pytest.mark.parametrize("what", ["video", "video_rgbd", "still"])
def test_metadata_is_byte_identical_to_the_serial_runs(tree, tmp_path, what):
    _, clip, png = tree
    argv = {"video": ["-i", str(clip), "-f", "all", "-b", "-m", "-e", "2"],
            "video_rgbd": ["-i", str(clip), "-f", "all", "-b", "-m", "--rgbd", "right"],
            "still": ["-i", str(png), "-e", "1"]}[what]
    process.main(argv + ["--output", str(tmp_path / "ser")])
    process.main(argv + ["--output", str(tmp_path / "par"), "--jobs", "3"])
    ser = open(tmp_path / "ser" / "metadata.json", "rb").read()
    assert open(tmp_path / "par" / "metadata.json", "rb").read() == ser
    bands = json.loads(ser)["bands"]
    if what == "video":
        assert list(bands) == ["rgba", "mask", "depth_anything", "depth",
                               "flow_gmflow", "flow_gmflow_mask", "flow_gmflow_bwd", "flow_gmflow_mask_bwd",
                               "flow_raft", "flow_raft_mask", "flow_raft_bwd", "flow_raft_mask_bwd",
                               "flow", "flow_bwd", "flow_mask", "flow_mask_bwd"]
    bands = json.load(open(tmp_path / "par" / "metadata.json"))["bands"]
    if what == "video_rgbd":                     # the measured half keeps the `depth` name (process.py, reference :243)
        assert bands["depth"] == {"url": "depth.npy"}
    else:
        assert bands["depth"] == bands["depth_anything"] and "values" in bands["depth"]
    if what != "still":
        for suffix in ("", "_bwd", "_mask", "_mask_bwd"):
            assert bands["flow" + suffix] == bands["flow_gmflow" + suffix] and bands["flow" + suffix]["url"] == "flow_gmflow" + suffix + ".npy"
    else:
        assert "flow" not in bands


def test_a_second_run_over_the_same_folder_keeps_the_serial_order(tree, tmp_path):
    """Keys the folder already holds stay where they are in a serial run, so they do in a parallel one."""
    _, clip, _ = tree
    for out, jobs in (("ser", "1"), ("par", "3")):
        process.main(["-i", str(clip), "-f", "flow_raft", "--output", str(tmp_path / out), "--jobs", "3"])     # the same first run for both
        process.main(["-i", str(clip), "-f", "all", "-b", "--output", str(tmp_path / out), "--jobs", jobs])
    assert open(tmp_path / "par" / "metadata.json", "rb").read() == open(tmp_path / "ser" / "metadata.json", "rb").read()


def test_gpus_puts_video_bands_under_torch_distributed_run(tree, tmp_path, monkeypatch):
    _, clip, png = tree
    real = subprocess.run

    def fake(cmd, **kw):
        return real(cmd, **kw) if os.path.basename(cmd[1]) == "rgba.py" else subprocess.CompletedProcess(cmd, 0)
    monkeypatch.setattr(process.subprocess, "run", fake)
    process.main(["-i", str(clip), "-f", "all", "-b", "--output", str(tmp_path / "one")])
    plain = [list(c) for c in process.COMMANDS]
    bands = os.path.join(process.ROOT, "bands")
    assert plain[1] == [sys.executable, os.path.join(bands, "mask_mmdet.py"), "-i", str(tmp_path / "one"), "--sdf", "--subpath", "mask"]
    process.main(["-i", str(clip), "-f", "all", "-b", "--output", str(tmp_path / "one"), "--gpus", "1"])
    assert process.COMMANDS == plain                                               # --gpus 1 is today's argv
    process.main(["-i", str(clip), "-f", "all", "-b", "--output", str(tmp_path / "one"), "--gpus", "2"])
    assert process.COMMANDS[0] == plain[0]                                         # rgba: always plain
    ports = []
    for cmd, old in zip(process.COMMANDS[1:], plain[1:]):
        assert cmd[:8] == [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                           "--master-port"]
        ports.append(int(cmd[8]))
        assert cmd[9:] == old[1:]                                                  # the band's own arguments are unchanged
    assert len(ports) == 4 and len(set(ports)) == 4 and all(1024 <= p < 65536 for p in ports)
    monkeypatch.setenv("PRISMA_GPUS", "2")                                         # the default of --gpus
    process.main(["-i", str(clip), "--output", str(tmp_path / "one")])
    assert [c[2] for c in process.COMMANDS[1:]] == ["torch.distributed.run"] * 3
    process.main(["-i", str(png), "--output", str(tmp_path / "two"), "--gpus", "2"])                 # a still image never shards
    assert [c[1] for c in process.COMMANDS] == [os.path.join(bands, b + ".py") for b in ("rgba", "mask_mmdet", "depth_anything")]
    assert process.build_command("flow_raft", "f", gpus=1) == process.build_command("flow_raft", "f")
    assert process.build_command("rgba", "f", gpus=8) == process.build_command("rgba", "f")


def test_a_failing_band_is_recorded_and_the_others_finish(tree, tmp_path, monkeypatch, capsys):
    side, clip, _ = tree
    monkeypatch.setenv("FAKE_EXIT_depth_anything", "3")
    with pytest.raises(SystemExit) as e:
        process.main(["-i", str(clip), "-f", "all", "--output", str(tmp_path / "out"), "--jobs", "3"])
    assert e.value.code == 1
    assert "1 band(s) FAILED: depth_anything (exit 3)" in capsys.readouterr().err
    assert process.RESULTS == [("rgba", 0), ("mask_mmdet", 0), ("depth_anything", 3), ("flow_gmflow", 0), ("flow_raft", 0)]
    times = _intervals(side)
    assert all("end" in times[name] for name in FAKES)
    bands = json.load(open(tmp_path / "out" / "metadata.json"))["bands"]
    assert bands["flow"] == bands["flow_gmflow"] and "flow_raft" in bands and "mask" in bands


def test_a_band_killed_by_a_signal_stops_further_starts(tree, tmp_path, monkeypatch, capsys):
    side, clip, _ = tree
    monkeypatch.setenv("FAKE_EXIT_mask_mmdet", "abort")
    with pytest.raises(SystemExit) as e:
        process.main(["-i", str(clip), "-f", "all", "--output", str(tmp_path / "out"), "--jobs", "2"])
    assert e.value.code == 1
    err = capsys.readouterr().err
    assert "mask_mmdet (exit -6)" in err and "FAILED" in err
    times = _intervals(side)
    assert sorted(times) == ["depth_anything", "mask_mmdet"]                       # the flow bands were never started
    assert "end" in times["depth_anything"] and "end" not in times["mask_mmdet"]   # the one already running finished
    assert process.RESULTS == [("rgba", 0), ("mask_mmdet", -6), ("depth_anything", 0)]
    assert [os.path.basename(c[1]) for c in process.COMMANDS] == ["rgba.py", "mask_mmdet.py", "depth_anything.py"]


def test_keyboard_interrupt_terminates_the_children(tree, tmp_path, monkeypatch):
    _, clip, _ = tree
    started = []
    popen = subprocess.Popen

    def recording(*a, **kw):
        started.append(popen(*a, **kw))
        return started[-1]

    class Interrupted(process.queue.Queue):
        def get(self, *a, **kw):
            raise KeyboardInterrupt
    monkeypatch.setattr(process.subprocess, "Popen", recording)
    monkeypatch.setattr(process.queue, "Queue", Interrupted)
    with pytest.raises(KeyboardInterrupt):
        process.main(["-i", str(clip), "--output", str(tmp_path / "out"), "--jobs", "3"])
    assert len(started) == 4 and started[0].returncode == 0                       # rgba, through subprocess.run
    assert [p.poll() for p in started[1:]] == [-15] * 3                            # the three bands: SIGTERM, and waited for


def test_child_output_is_relayed_with_the_bands_prefix(tree, tmp_path, capfd):
    _, clip, _ = tree
    process.main(["-i", str(clip), "--output", str(tmp_path / "out"), "--jobs", "3"])
    out, err = capfd.readouterr()
    for name in ("mask_mmdet", "depth_anything", "flow_gmflow"):
        assert "[%s] fake %s wrote its entries\n" % (name, name) in out
        assert "[%s] fake %s says so on stderr too\n" % (name, name) in err
    assert not [line for line in out.splitlines() if line.startswith("fake ")]     # nothing reaches the terminal unprefixed
