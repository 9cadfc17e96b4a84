"""prisma folder contract: <folder>/metadata.json + one file per band.

Re-statement of the behaviour of /root/reference/bands/common/meta.py (load_metadata :27-32,
create_metadata :35-58, is_video :65-67, get_target :70-93, get_url :96-104, add_band :109-121,
write_metadata :124-134, set_default_band :137-146, get_record3d_data :148-156) - same function names,
arguments and JSON layout, so files written by either implementation are interchangeable.
"""
import collections
import copy
import fcntl
import json
import os
import stat
import tempfile

META_FILE = "metadata.json"
LOCK_SUFFIX = ".lock"     # <folder>/metadata.json.lock: flock()ed by update_metadata, never deleted (unlinking a lock file races)


def get_metadata_path(path):
    if os.path.isfile(path):
        return path if path.endswith(".json") else get_metadata_path(os.path.dirname(path))
    if os.path.isdir(path):
        return os.path.join(path, META_FILE)
    return None


def load_metadata(path):
    mp = get_metadata_path(path)
    if mp and os.path.exists(mp):
        with open(mp) as f:
            return json.load(f)
    return None


def create_metadata(path):
    folder = os.path.dirname(path) if os.path.isfile(path) else path
    os.makedirs(folder, exist_ok=True)
    mp = os.path.join(folder, META_FILE)
    if not os.path.exists(mp):
        with open(mp, "w") as f:
            f.write(json.dumps({"bands": {}}, indent=4))
    return load_metadata(mp)


VIDEO_OUT_EXTS = ("avi", "mjpeg")          # Motion JPEG containers the bands write (common/io.py VideoWriter)
VIDEO_OUT_CHROMAS = {"444": 444, "420": 420, "mono": 400}
VideoOut = collections.namedtuple("VideoOut", "ext quality chroma")


def video_out():
    """PRISMA_VIDEO_OUT (process.py --video_out): the container every derived video band is written in instead of the clip's own.  `avi` or
    `mjpeg`, then optionally `,q=NN` (JPEG quality 1 .. 100, default 90) and one of `,444` `,420` `,mono` (default 444: the bands carry data in
    their colours).  -> VideoOut(ext, quality, chroma 444 | 420 | 400), None when unset or empty; anything else is refused."""
    v = os.environ.get("PRISMA_VIDEO_OUT", "")
    if not v:
        return None
    ext, *opts = v.split(",")
    bad = RuntimeError("PRISMA_VIDEO_OUT=%s: `avi` or `mjpeg`, then optionally `,q=NN` (1 .. 100) and one of `,444` `,420` `,mono`" % v)
    if ext not in VIDEO_OUT_EXTS:
        raise bad
    quality, chroma = None, None
    for o in opts:
        if o.startswith("q=") and quality is None and o[2:].isdigit() and 1 <= int(o[2:]) <= 100:
            quality = int(o[2:])
        elif o in VIDEO_OUT_CHROMAS and chroma is None:
            chroma = VIDEO_OUT_CHROMAS[o]
        else:
            raise bad
    return VideoOut(ext, 90 if quality is None else quality, 444 if chroma is None else chroma)


def band_video_ext(path):
    """the extension of a video band derived from the clip `path`: PRISMA_VIDEO_OUT's when set, else the clip's own"""
    vo = video_out()
    return vo.ext if vo is not None and is_video(path) else os.path.basename(path).rsplit(".", 1)[1]


def is_video(path):
    # the reference tests the suffix only (:65-67); .npy frame stacks are this repo's offline stand-in, .y4m the container that needs no library,
    # .avi / .mjpeg the Motion JPEG files of PRISMA_VIDEO_OUT
    return path.endswith((".mp4", ".npy", ".y4m", ".avi", ".mjpeg"))


def add_band(metadata, band, url="", folder=""):
    b = metadata.setdefault("bands", {}).setdefault(band, {})
    if url != "":
        b["url"] = url
    if folder != "":
        b["folder"] = folder


def get_target(path, metadata, band="rgba", target="", force_extension=None):
    folder = target if os.path.isdir(target) else os.path.dirname(path)
    # rgba keeps the clip's container: the other bands read it
    ext = os.path.basename(path).rsplit(".", 1)[1] if band == "rgba" else band_video_ext(path)
    if force_extension and (not is_video(path) or force_extension == "csv"):
        ext = force_extension
    name = band + "." + ext
    if target == "" or os.path.isdir(target):
        target = os.path.join(folder, name)
    if metadata:
        add_band(metadata, band, url=name)
    return target


def get_url(path, metadata, band):
    if os.path.isdir(path) and metadata:
        url = metadata.get("bands", {}).get(band, {}).get("url")
        if url:
            return os.path.join(path, url)
    return path


def write_metadata(path, metadata):
    if metadata is None:
        return
    mp = get_metadata_path(path)
    if mp and os.path.exists(mp):
        with open(mp, "w") as f:
            f.write(json.dumps(metadata, indent=4))


def update_metadata(path, fn):
    """Read-modify-write of metadata.json that is safe against other processes doing the same: an exclusive flock on
    `metadata.json.lock`, the file re-read under it, `fn(data)` applied (it changes `data` in place or returns the new dict; False means
    "nothing to write"), the result written to a temporary name in the same folder and renamed over metadata.json - a reader never sees a torn file.
    Returns what was written; None (and nothing written) where there is no metadata.json, as write_metadata."""
    mp = get_metadata_path(path)
    if not (mp and os.path.exists(mp)):
        return None
    with open(mp + LOCK_SUFFIX, "a") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            with open(mp) as f:
                data = json.load(f)
            out = fn(data)
            if out is False:
                return data
            if out is None:
                out = data
            fd, tmp = tempfile.mkstemp(prefix=META_FILE + ".", suffix=".tmp", dir=os.path.dirname(mp))
            try:
                with os.fdopen(fd, "w") as f:
                    f.write(json.dumps(out, indent=4))
                os.chmod(tmp, stat.S_IMODE(os.stat(mp).st_mode))      # mkstemp's 0600 would change who can read the folder's metadata
                os.replace(tmp, mp)
            except BaseException:
                if os.path.exists(tmp):
                    os.unlink(tmp)
                raise
            return out
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def merge_metadata(path, data, loaded):
    """A band's last metadata write when other bands may be writing the same folder.  `loaded` is a deep copy of what the band read
    at start, `data` its copy now; under the lock only what the band changed goes into the current file: every top-level key that
    differs, and every key of `bands` that was added or changed - a changed entry replaces the file's as a whole (mask_mmdet
    relies on that to drop its `folder` key).  A key the band did not touch keeps the file's current value.  A band running alone
    writes the bytes write_metadata(path, data) would."""
    if data is None:
        return
    loaded = loaded or {}
    missing = object()

    def apply(cur):
        for k, v in data.items():
            if k == "bands" and isinstance(v, dict) and isinstance(cur.get("bands"), dict):
                old = loaded.get("bands") if isinstance(loaded.get("bands"), dict) else {}
                for b, entry in v.items():
                    if old.get(b, missing) != entry:
                        cur["bands"][b] = copy.deepcopy(entry)
                for b in old:
                    if b not in v:
                        cur["bands"].pop(b, None)
            elif loaded.get(k, missing) != v:
                cur[k] = copy.deepcopy(v)
        for k in loaded:
            if k not in data:
                cur.pop(k, None)
    update_metadata(path, apply)


def set_default_band(path, band, band_default):
    def alias(data):
        if band_default not in data.get("bands", {}):
            return False
        data["bands"][band] = data["bands"][band_default]
    update_metadata(path, alias)


def get_record3d_data(path):
    """Record3D's capture data of a video, {"intrinsicMatrix": [9 numbers, column major], "rangeOfEncodedDepth": [min, max]} (:148-156).
    The reference reads the container's `movie_more` tag through pymediainfo.  Looked up here in this order: a sidecar
    `<path without extension>.record3d.json` holding that tag's JSON (the offline stand-in, as .npy stacks are for .mp4), then pymediainfo
    when it imports; otherwise an error that names both."""
    sidecar = path.rsplit(".", 1)[0] + ".record3d.json"
    if os.path.exists(sidecar):
        with open(sidecar) as f:
            info = json.load(f)
    else:
        try:
            from pymediainfo import MediaInfo
        except ImportError as e:
            raise RuntimeError("Record3D data of %s: no sidecar %s and pymediainfo (the reference's reader of the video's `movie_more` tag) is "
                               "not installed" % (path, sidecar)) from e
        info = json.loads(json.loads(MediaInfo.parse(path).to_json())["tracks"][0]["movie_more"])
    if len(info.get("intrinsicMatrix", ())) != 9 or len(info.get("rangeOfEncodedDepth", ())) != 2:
        raise RuntimeError("Record3D data of %s: needs intrinsicMatrix (9 numbers) and rangeOfEncodedDepth (min, max)" % path)
    return info
