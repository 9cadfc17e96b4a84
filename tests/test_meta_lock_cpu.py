"""CPU: metadata.json under concurrent writers (bands/common/meta.py update_metadata / merge_metadata).  Bands of one clip may run
side by side (process.py --jobs); each ends by merging only what it changed into the file, under a lock, through a rename."""
import copy
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bands.common import meta  # noqa: E402

WRITER = """
import sys
sys.path.insert(0, %r)
from bands.common import meta
folder, who = sys.argv[1], sys.argv[2]
for i in range(25):
    def add(data, key="band_%%s_%%02d" %% (who, i)):
        data["bands"][key] = {"url": key + ".npy"}
    meta.update_metadata(folder, add)
""" % ROOT


def _folder(tmp_path, data=None):
    folder = tmp_path / "clip"
    folder.mkdir()
    (folder / "metadata.json").write_text(json.dumps(data or {"bands": {"rgba": {"url": "rgba.npy"}}}, indent=4))
    return str(folder)


def test_eight_processes_lose_no_update(tmp_path):
    folder = _folder(tmp_path)
    procs = [subprocess.Popen([sys.executable, "-c", WRITER, folder, str(w)]) for w in range(8)]
    assert [p.wait(timeout=120) for p in procs] == [0] * 8
    bands = json.load(open(os.path.join(folder, "metadata.json")))["bands"]            # parses: never torn
    assert set(bands) == {"rgba"} | {"band_%d_%02d" % (w, i) for w in range(8) for i in range(25)}
    assert len(bands) == 201
    assert sorted(os.listdir(folder)) == ["metadata.json", "metadata.json.lock"]      # no temporary file left; the lock file stays


def test_merge_with_a_stale_copy_keeps_the_other_writers_changes(tmp_path):
    folder = _folder(tmp_path, {"bands": {"rgba": {"url": "rgba.npy"}}, "fps": 24.0, "width": 64})
    a = meta.load_metadata(folder)                      # A loads
    a_loaded = copy.deepcopy(a)
    b = meta.load_metadata(folder)                      # B adds band x and changes fps, and is done first
    b_loaded = copy.deepcopy(b)
    meta.add_band(b, "x", url="x.npy")
    b["fps"] = 30.0
    meta.merge_metadata(folder, b, b_loaded)
    meta.add_band(a, "y", url="y.npy")                  # A adds band y and merges its stale copy
    meta.merge_metadata(folder, a, a_loaded)
    out = meta.load_metadata(folder)
    assert out == {"bands": {"rgba": {"url": "rgba.npy"}, "x": {"url": "x.npy"}, "y": {"url": "y.npy"}}, "fps": 30.0, "width": 64}
    assert list(out["bands"]) == ["rgba", "x", "y"]


def test_a_replaced_entry_drops_the_old_entrys_keys(tmp_path):
    """mask_mmdet replaces its whole entry at the end, which drops the `folder` key an earlier run (or get_target) left."""
    folder = _folder(tmp_path, {"bands": {"rgba": {"url": "rgba.npy"}, "mask": {"url": "mask.npy", "folder": "mask", "ids": ["old"]}}})
    data = meta.load_metadata(folder)
    loaded = copy.deepcopy(data)
    meta.update_metadata(folder, lambda d: d["bands"].__setitem__("other", {"url": "other.npy"}))      # someone else, meanwhile
    data["bands"]["mask"] = {"url": "mask.npy", "ids": ["person"]}
    meta.merge_metadata(folder, data, loaded)
    out = meta.load_metadata(folder)
    assert out["bands"]["mask"] == {"url": "mask.npy", "ids": ["person"]}
    assert out["bands"]["other"] == {"url": "other.npy"} and out["bands"]["rgba"] == {"url": "rgba.npy"}


def test_an_untouched_key_keeps_the_files_value(tmp_path):
    folder = _folder(tmp_path, {"bands": {"rgba": {"url": "rgba.npy"}, "depth": {"url": "a.npy"}}, "fps": 24.0})
    data = meta.load_metadata(folder)
    loaded = copy.deepcopy(data)

    def other(d):
        d["bands"]["depth"] = {"url": "b.npy"}
        d["fps"] = 12.0
    meta.update_metadata(folder, other)
    data["frames"] = 3
    meta.merge_metadata(folder, data, loaded)
    out = meta.load_metadata(folder)
    assert out["bands"]["depth"] == {"url": "b.npy"} and out["fps"] == 12.0 and out["frames"] == 3


def test_a_band_alone_writes_the_bytes_of_write_metadata(tmp_path):
    start = {"bands": {"rgba": {"url": "rgba.npy"}, "mask": {"url": "mask.npy", "folder": "mask"}}, "width": 64, "height": 48,
             "fps": 24.0, "focal_length": 55.42562584220407, "principal_point": [32.0, 24.0]}
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    one, two = _folder(tmp_path / "a", start), _folder(tmp_path / "b", start)
    for folder, merge in ((one, False), (two, True)):
        data = meta.load_metadata(folder)
        loaded = copy.deepcopy(data)
        meta.get_target(os.path.join(folder, "rgba.npy"), data, band="flow_raft")            # what a flow band does to its copy
        meta.get_target(os.path.join(folder, "rgba.npy"), data, band="flow_raft_mask")
        data["bands"]["flow_raft"] = {"url": "flow_raft.npy", "values": {"dist": {"type": "float", "url": "flow_raft.csv"}}, "folder": "f"}
        data["bands"]["flow_raft_bwd"] = {"url": "flow_raft_bwd.npy"}
        data["bands"]["mask"] = {"url": "mask.npy", "ids": ["person"]}
        data["frames"] = 3
        if merge:
            meta.merge_metadata(folder, data, loaded)
        else:
            meta.write_metadata(folder, data)
    a, b = open(os.path.join(one, "metadata.json"), "rb").read(), open(os.path.join(two, "metadata.json"), "rb").read()
    assert a == b and b"\n    " in a                                  # indent=4, same keys in the same order
    assert list(json.loads(b)["bands"]) == ["rgba", "mask", "flow_raft", "flow_raft_mask", "flow_raft_bwd"]


def test_set_default_band_goes_through_the_lock(tmp_path):
    folder = _folder(tmp_path, {"bands": {"rgba": {"url": "rgba.npy"}, "depth_anything": {"url": "depth_anything.npy"}}})
    meta.set_default_band(folder, "depth", "depth_anything")
    meta.set_default_band(folder, "flow", "flow_gmflow")               # no such band: nothing changes
    out = meta.load_metadata(folder)
    assert out["bands"]["depth"] == out["bands"]["depth_anything"] and "flow" not in out["bands"]
    assert os.path.exists(os.path.join(folder, "metadata.json.lock"))
