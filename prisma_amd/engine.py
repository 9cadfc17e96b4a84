"""Python host side of the bands engine: thin, typed wrappers over the C ABI.

`DepthAnything` mirrors what bands/depth_anything.py builds in init_model() and calls in
infer() (reference lines 48-76, 100-143); all arithmetic runs in libprisma_bands.so on the GPU.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _lib
from ._lib import I420, YuvFormat, check
from .synth import DEPTH_CFGS, MASK_CFGS, DepthCfg, MaskCfg


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


# one vertex of the reference's point cloud (bands/common/geom.py:32-33 npy_types): 15 packed bytes
VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])


def device_count() -> int:
    return _lib.load().pb_device_count()


def net_size(H: int, W: int) -> Tuple[int, int]:
    """(net_h, net_w) of the network input for an HxW frame (transform.py:100-166)."""
    nh, nw = C.c_int(), C.c_int()
    check(_lib.load().pb_depth_net_size(H, W, C.byref(nh), C.byref(nw)))
    return nh.value, nw.value


def i420_bytes(H: int, W: int) -> int:
    """bytes of one I420 frame (a .y4m's): H W of Y, then ceil(H / 2) ceil(W / 2) each of Cb and Cr (pb_i420_bytes, needs no GPU)"""
    return int(_lib.load().pb_i420_bytes(int(H), int(W)))


def yuv_bytes(fmt: YuvFormat, H: int, W: int) -> int:
    """bytes of one planar YUV frame of layout `fmt` (a .y4m's; pb_yuv_bytes, needs no GPU): H W samples of Y, then for 4:2:0 / 4:2:2 / 4:4:4 the
    subsampled Cb and Cr planes, a sample one byte at 8 bit and two above; 0 for a format the library does not have"""
    return int(_lib.load().pb_yuv_bytes(C.byref(YuvFormat(*fmt).c()), int(H), int(W)))


def yuv_coeffs(fmt: YuvFormat) -> Tuple[int, ...]:
    """(cy, crv, cgu, cgv, cbu, yoff, coff) of the library's integer conversion of layout `fmt` (pb_yuv_coeffs, needs no GPU)"""
    out = (C.c_int32 * 7)()
    check(_lib.load().pb_yuv_coeffs(C.byref(YuvFormat(*fmt).c()), out))
    return tuple(out)


def yuv_fwd_coeffs(fmt: YuvFormat) -> Tuple[int, ...]:
    """(yr, yg, yb, ur, ug, h, vg, vb, F, yoff, coff, 2^d - 1) of the library's integer RGB -> YUV conversion to layout `fmt` (pb_yuv_fwd_coeffs,
    needs no GPU)"""
    out = (C.c_int32 * 12)()
    check(_lib.load().pb_yuv_fwd_coeffs(C.byref(YuvFormat(*fmt).c()), out))
    return tuple(int(v) for v in out)


JPEG_CHROMAS = (444, 420, 400)


def jpeg_format(chroma: int) -> YuvFormat:
    """the layout of the planes a JPEG of `chroma` is made of: JFIF's colour space"""
    return YuvFormat(int(chroma), 8, True, "bt601")


def jpeg_bound(chroma: int, quality: int, H: int, W: int) -> int:
    """worst-case bytes of one JPEG frame (pb_jpeg_bound, needs no GPU); 0 for a chroma / quality / size the encoder does not have"""
    return int(_lib.load().pb_jpeg_bound(C.byref(_lib.pb_jpeg_cfg(int(chroma), int(quality))), int(H), int(W)))


class JpegOverflow(_lib.PrismaBandsError):
    """jpeg_encode: the caller's buffer is too small.  .needed: the bytes that would do; .offsets: where every frame would lie - the frames that
    end within the capacity are in the buffer."""

    def __init__(self, msg, needed, offsets):
        super().__init__(msg)
        self.needed, self.offsets = needed, offsets


FORMATS = ("rgb", "i420")       # what `frames` / the encoded `rgb` results of a band context are: [..., H, W, 3] or [..., i420_bytes(H, W)] uint8


RGBD_SIDES = ("left", "right", "top", "bottom")      # where the depth is: pb_rgbd_boxes' side 0 .. 3


def _rgbd_side(side) -> int:
    if isinstance(side, str):
        if side not in RGBD_SIDES:
            raise ValueError("side %r: one of %s" % (side, ", ".join(RGBD_SIDES)))
        return RGBD_SIDES.index(side)
    return int(side)


def rgbd_boxes(H: int, W: int, side) -> Tuple[Tuple[int, int, int, int], Tuple[int, int, int, int]]:
    """(rgb_box, depth_box) of an H x W side-by-side RGB-D frame as half-open (y0, y1, x0, x1); `side` (a name of RGBD_SIDES or its index)
    is where the depth is (bands/rgba.py:29-40, 58-59; pb_rgbd_boxes, needs no GPU)"""
    rb, db = (C.c_int * 4)(), (C.c_int * 4)()
    check(_lib.load().pb_rgbd_boxes(H, W, _rgbd_side(side), rb, db))
    return tuple(rb), tuple(db)


def run_concurrently(jobs):
    """Drive several band contexts at once: jobs = [(ctx, enqueue), ...] where `enqueue()` calls one of ctx's asynchronous device-pointer
    entry points (`infer_dev`, `infer_sequence_dev`, `infer_batch_dev`).  Every job is enqueued on its own ctx stream from this thread
    (an enqueue returns in a few milliseconds; the GPU then shares its CUs between the streams), then each ctx is waited for in order.
    Returns the seconds from the first enqueue to each ctx's completion.  Results are the bytes of running the jobs one after the other:
    contexts share no buffers (tests/test_gpu_edges.py::test_bands_run_concurrently_equal_sequential).  This replaces the reference's
    strictly sequential band order (process.py:205-290) where the bands of one video are independent."""
    import time
    t0 = time.perf_counter()
    started = []
    try:
        for ctx, enqueue in jobs:
            started.append(ctx)
            enqueue()
    except BaseException:
        for ctx in started:                 # an enqueue failed: nothing may stay in flight on the contexts that did start
            try:
                ctx.sync()
            except Exception:               # noqa: BLE001 - the first error is the one to report
                pass
        raise
    done = []
    for ctx, _ in jobs:
        ctx.sync()
        done.append(time.perf_counter() - t0)
    return done


class _Ctx:
    def __init__(self):
        self.lib = _lib.load()
        self.ctx = C.c_void_p()
        self._host = {}                 # host_empty(): address -> (weak reference to the array, bytes)
        self._formats = ["rgb", "rgb"]  # frame_format, rgb_format
        self._rgb_full = False

    def close(self):
        """pb_destroy: waits for the submissions still outstanding, then frees everything the context owns - the host_empty() arrays
        included.  They die with the context: an array still referenced afterwards points at freed memory, so it is made read-only
        here and must not be touched again (host_free() the arrays, or drop them, before close() where that matters)."""
        if self.ctx:
            for ref, _ in getattr(self, "_host", {}).values():
                arr = ref()
                if arr is not None:
                    arr.flags.writeable = False
            self._host = {}
            self.lib.pb_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # RCCL all-gather of per-frame scalars through the C ABI (pb_comm_*, pb_gather_scalars)
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        check(_lib.load().pb_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, comm_id: bytes, rank: int, world: int):
        assert len(comm_id) == 128
        check(self.lib.pb_comm_init(self.ctx, C.create_string_buffer(comm_id, 128), rank, world))
        self._comm_world = world

    def gather_scalars(self, local: np.ndarray) -> np.ndarray:
        """float32 [n_local, ...] of this rank -> [world, n_local, ...] on every rank (same n_local everywhere)."""
        local = _f32(local)
        out = np.empty((self._comm_world,) + local.shape, np.float32)
        check(self.lib.pb_gather_scalars(self.ctx, _ptr(local), local.size, _ptr(out)))
        return out

    # device memory helpers (frames resident in HBM for bench / pipelines)
    def dev_alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        check(self.lib.pb_dev_alloc(self.ctx, C.byref(p), nbytes))
        return p.value

    def dev_free(self, ptr: int):
        check(self.lib.pb_dev_free(self.ctx, C.c_void_p(ptr)))

    def h2d(self, ptr: int, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        check(self.lib.pb_memcpy_h2d(self.ctx, C.c_void_p(ptr), _ptr(arr), arr.nbytes))

    def d2h(self, arr: np.ndarray, ptr: int):
        assert arr.flags.c_contiguous
        check(self.lib.pb_memcpy_d2h(self.ctx, _ptr(arr), C.c_void_p(ptr), arr.nbytes))

    # page-locked host memory owned by the context (pb_host_alloc): what submit_* demands and the blocking calls address without staging
    def host_empty(self, shape, dtype) -> np.ndarray:
        """An uninitialised C-contiguous array of `shape` / `dtype` over a page-locked block of the context (the band loops' rings; no
        torch pin_memory needed).  host_free(arr) releases it; close() releases whatever is left - the array does not own its memory and
        dies with the context (see close)."""
        import weakref
        shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
        dt = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dt.itemsize
        p = C.c_void_p()
        check(self.lib.pb_host_alloc(self.ctx, C.byref(p), nbytes))
        arr = np.frombuffer((C.c_ubyte * max(nbytes, 1)).from_address(p.value), np.uint8, nbytes).view(dt).reshape(shape)
        self._host[p.value] = (weakref.ref(arr), nbytes)
        return arr

    def host_free(self, arr: np.ndarray):
        """Releases a host_empty() array (pb_host_free; anything else is refused with PB_ERR_ARG).  No submission may still use it, and
        the array - with every view of it - must not be touched afterwards."""
        ptr = arr.ctypes.data
        check(self.lib.pb_host_free(self.ctx, C.c_void_p(ptr)))
        getattr(self, "_host", {}).pop(ptr, None)

    def host_bytes(self) -> int:
        """bytes of the host_empty() blocks the context holds"""
        return sum(n for _, n in getattr(self, "_host", {}).values())

    def sync(self):
        check(self.lib.pb_sync(self.ctx))

    def wait(self):
        """Blocks until the OLDEST submit_* call of this context not yet waited for has its results in the caller's (page-locked) arrays
        and returns what that call returned (pb_wait)."""
        check(self.lib.pb_wait(self.ctx))
        return self._inflight.pop(0)[0] if getattr(self, "_inflight", None) else None

    def _hold(self, result, *arrays):
        # the arrays of a submission must outlive it: keep references until wait() hands the results back
        if not hasattr(self, "_inflight"):
            self._inflight = []
        self._inflight.append((result, arrays))

    def encode_still(self, depth: np.ndarray, flip: bool = True, encode_range: bool = True):
        """write_depth(heatmap=True) of one float32 depth map on the GPU (bands/common/io.py:138-172): -> (rgb u8 [H,W,3], min, max)."""
        depth = _f32(depth)
        H, W = depth.shape
        rgb = np.empty((H, W, 3), np.uint8)
        lo, hi = C.c_float(), C.c_float()
        check(self.lib.pb_depth_encode_still(self.ctx, _ptr(depth), H, W, int(flip), int(encode_range), _ptr(rgb), C.byref(lo), C.byref(hi)))
        return rgb, lo.value, hi.value

    def point_cloud(self, depth: np.ndarray, rgb: np.ndarray, flip: bool = True, u0: Optional[float] = None, v0: Optional[float] = None,
                    fx: float = 1000.0, fy: float = 1000.0) -> np.ndarray:
        """write_pcl's vertices on the GPU (bands/common/io.py:201-211, bands/common/geom.py:5-47; pb_depth_point_cloud): depth [H, W] or
        [n, H, W] float32 and rgb [..., H, W, 3] uint8 -> the PLY's vertex records, a structured array of depth's shape viewed over the
        returned bytes.  u0 / v0 default to the reference's W / 2 and H / 2."""
        depth = _f32(depth)
        rgb = np.ascontiguousarray(rgb, np.uint8)
        assert depth.ndim in (2, 3) and rgb.shape == depth.shape + (3,), (depth.shape, rgb.shape)
        H, W = depth.shape[-2:]
        n = depth.shape[0] if depth.ndim == 3 else 1
        raw = np.empty(depth.shape + (VERTEX_DTYPE.itemsize,), np.uint8)
        check(self.lib.pb_depth_point_cloud(self.ctx, _ptr(depth), _ptr(rgb), n, H, W, int(flip), W / 2 if u0 is None else u0,
                                            H / 2 if v0 is None else v0, fx, fy, _ptr(raw)))
        return raw.view(VERTEX_DTYPE).reshape(depth.shape)

    def point_cloud_dev(self, depth_ptr: int, rgb_ptr: int, n: int, H: int, W: int, out_ptr: int, flip: bool = True,
                        u0: Optional[float] = None, v0: Optional[float] = None, fx: float = 1000.0, fy: float = 1000.0):
        """the same on device pointers (dev_alloc), enqueued on the ctx stream (pb_depth_point_cloud_dev): sync() waits; out_ptr takes
        n * H * W * 15 bytes"""
        check(self.lib.pb_depth_point_cloud_dev(self.ctx, C.c_void_p(depth_ptr), C.c_void_p(rgb_ptr), n, H, W, int(flip),
                                                W / 2 if u0 is None else u0, H / 2 if v0 is None else v0, fx, fy, C.c_void_p(out_ptr)))

    def rgbd_depth(self, frames: np.ndarray, side, want_heat: bool = False, want_rgb: bool = True, out_rgb: Optional[np.ndarray] = None,
                   out_heat: Optional[np.ndarray] = None):
        """`--encoding_depth hue` of the depth half of side-by-side RGB-D frames [n, H, W, 3] uint8 (bands/rgba.py:58-63; pb_rgbd_depth):
        -> the heat-encoded half [n, Hd, Wd, 3] uint8, or with want_heat (that, heat [n, Hd, Wd] float32: the decoded value in [0, 1]);
        want_rgb=False: heat alone.  out_rgb / out_heat: the caller's own (page-locked) arrays."""
        frames = np.ascontiguousarray(frames, np.uint8)
        assert frames.ndim == 4 and frames.shape[-1] == 3, frames.shape
        n, H, W = frames.shape[:3]
        _, db = rgbd_boxes(H, W, side)
        shape = (n, db[1] - db[0], db[3] - db[2])
        rgb = (np.empty(shape + (3,), np.uint8) if out_rgb is None else out_rgb) if want_rgb else None
        heat = (np.empty(shape, np.float32) if out_heat is None else out_heat) if want_heat else None
        assert rgb is None or (rgb.shape == shape + (3,) and rgb.dtype == np.uint8 and rgb.flags.c_contiguous)
        assert heat is None or (heat.shape == shape and heat.dtype == np.float32 and heat.flags.c_contiguous)
        check(self.lib.pb_rgbd_depth(self.ctx, _ptr(frames), n, H, W, _rgbd_side(side), _ptr(rgb), _ptr(heat)))
        return (rgb, heat) if want_heat and want_rgb else (heat if want_heat else rgb)

    def rgbd_depth_dev(self, frames_ptr: int, n: int, H: int, W: int, side, depth_ptr: int = 0, heat_ptr: int = 0):
        """the same on device pointers (dev_alloc), enqueued on the ctx stream (pb_rgbd_depth_dev): sync() waits; depth_ptr takes
        n * Hd * Wd * 3 bytes (no alignment needed), heat_ptr n * Hd * Wd floats; 0 = not wanted"""
        check(self.lib.pb_rgbd_depth_dev(self.ctx, C.c_void_p(frames_ptr), n, H, W, _rgbd_side(side), C.c_void_p(depth_ptr or None),
                                         C.c_void_p(heat_ptr or None)))

    # I420 <-> RGB (pb_i420_to_rgb / pb_rgb_to_i420: 8 bit, BT.601 limited range, exact integers; tests/yuv_ref.py restates them)
    def i420_to_rgb(self, yuv: np.ndarray, H: int, W: int, out: Optional[np.ndarray] = None) -> np.ndarray:
        """I420 frames uint8 [n, i420_bytes(H, W)] (or one frame [i420_bytes]) -> RGB uint8 [n, H, W, 3] ([H, W, 3]); `out`: the caller's own
        (page-locked) array"""
        yuv = np.ascontiguousarray(yuv, np.uint8)
        fb = i420_bytes(H, W)
        assert yuv.ndim in (1, 2) and yuv.shape[-1] == fb, (yuv.shape, fb)
        shape = yuv.shape[:-1] + (H, W, 3)
        rgb = np.empty(shape, np.uint8) if out is None else out
        assert rgb.shape == shape and rgb.dtype == np.uint8 and rgb.flags.c_contiguous
        check(self.lib.pb_i420_to_rgb(self.ctx, _ptr(yuv), yuv.size // fb, H, W, _ptr(rgb)))
        return rgb

    def rgb_to_i420(self, rgb: np.ndarray, out: Optional[np.ndarray] = None) -> np.ndarray:
        """RGB uint8 [n, H, W, 3] (or one frame [H, W, 3]) -> I420 frames uint8 [n, i420_bytes(H, W)] ([i420_bytes]); `out`: the caller's own
        (page-locked) array"""
        rgb = np.ascontiguousarray(rgb, np.uint8)
        assert rgb.ndim in (3, 4) and rgb.shape[-1] == 3, rgb.shape
        H, W = rgb.shape[-3:-1]
        shape = rgb.shape[:-3] + (i420_bytes(H, W),)
        yuv = np.empty(shape, np.uint8) if out is None else out
        assert yuv.shape == shape and yuv.dtype == np.uint8 and yuv.flags.c_contiguous
        check(self.lib.pb_rgb_to_i420(self.ctx, _ptr(rgb), rgb.size // (H * W * 3), H, W, _ptr(yuv)))
        return yuv

    # any planar .y4m layout -> RGB (pb_yuv_to_rgb: exact integers, tests/yuv_fmt_ref.py restates them)
    def yuv_to_rgb(self, fmt: YuvFormat, yuv: np.ndarray, H: int, W: int, out: Optional[np.ndarray] = None) -> np.ndarray:
        """frames of layout `fmt`, uint8 [n, yuv_bytes(fmt, H, W)] (or one frame [yuv_bytes]; a 16-bit sample is two bytes, little-endian) -> RGB
        uint8 [n, H, W, 3] ([H, W, 3]); `out`: the caller's own (page-locked) array"""
        fmt = YuvFormat(*fmt)
        yuv = np.ascontiguousarray(yuv, np.uint8)
        fb = yuv_bytes(fmt, H, W)
        if fb <= 0:
            raise ValueError("no such YUV format: %r" % (fmt,))
        assert yuv.ndim in (1, 2) and yuv.shape[-1] == fb, (yuv.shape, fb)
        shape = yuv.shape[:-1] + (H, W, 3)
        rgb = np.empty(shape, np.uint8) if out is None else out
        assert rgb.shape == shape and rgb.dtype == np.uint8 and rgb.flags.c_contiguous
        check(self.lib.pb_yuv_to_rgb(self.ctx, C.byref(fmt.c()), _ptr(yuv), yuv.size // fb, H, W, _ptr(rgb)))
        return rgb

    def yuv_to_rgb_dev(self, fmt: YuvFormat, yuv_ptr: int, n: int, H: int, W: int, rgb_ptr: int):
        """the same on device pointers (dev_alloc), enqueued on the ctx stream (pb_yuv_to_rgb_dev): sync() waits"""
        check(self.lib.pb_yuv_to_rgb_dev(self.ctx, C.byref(YuvFormat(*fmt).c()), C.c_void_p(yuv_ptr), n, H, W, C.c_void_p(rgb_ptr)))

    # RGB -> any planar .y4m layout (pb_rgb_to_yuv: exact integers, tests/yuv_out_ref.py restates them)
    def rgb_to_yuv(self, fmt: YuvFormat, rgb: np.ndarray, out: Optional[np.ndarray] = None) -> np.ndarray:
        """RGB uint8 [n, H, W, 3] (or one frame [H, W, 3]) -> frames of layout `fmt`, uint8 [n, yuv_bytes(fmt, H, W)] ([yuv_bytes]; a 16-bit
        sample is two bytes, little-endian); `out`: the caller's own (page-locked) array"""
        fmt = YuvFormat(*fmt)
        rgb = np.ascontiguousarray(rgb, np.uint8)
        assert rgb.ndim in (3, 4) and rgb.shape[-1] == 3, rgb.shape
        H, W = rgb.shape[-3:-1]
        fb = yuv_bytes(fmt, H, W)
        if fb <= 0:
            raise ValueError("no such YUV format: %r" % (fmt,))
        shape = rgb.shape[:-3] + (fb,)
        yuv = np.empty(shape, np.uint8) if out is None else out
        assert yuv.shape == shape and yuv.dtype == np.uint8 and yuv.flags.c_contiguous
        check(self.lib.pb_rgb_to_yuv(self.ctx, C.byref(fmt.c()), _ptr(rgb), rgb.size // (H * W * 3), H, W, _ptr(yuv)))
        return yuv

    def rgb_to_yuv_dev(self, fmt: YuvFormat, rgb_ptr: int, n: int, H: int, W: int, yuv_ptr: int):
        """the same on device pointers (dev_alloc), enqueued on the ctx stream (pb_rgb_to_yuv_dev): sync() waits"""
        check(self.lib.pb_rgb_to_yuv_dev(self.ctx, C.byref(YuvFormat(*fmt).c()), C.c_void_p(rgb_ptr), n, H, W, C.c_void_p(yuv_ptr)))

    # planar full-range BT.601 YUV -> baseline JPEG frames (pb_jpeg_encode: exact integers, tests/jpeg_ref.py restates them)
    def jpeg_encode(self, planes: np.ndarray, H: int, W: int, chroma: int = 444, quality: int = 90, out: Optional[np.ndarray] = None,
                    capacity: Optional[int] = None):
        """frames of layout jpeg_format(chroma), uint8 [n, yuv_bytes] (or one frame [yuv_bytes]) -> (out, offsets): frame i is
        out[offsets[i]:offsets[i + 1]], a complete .jpg; offsets int64 [n + 1].  `out`: the caller's own (page-locked) uint8 array, of which
        `capacity` bytes (default: all) may be written - too small raises JpegOverflow.  Without `out` the buffer is sized here and grown once
        if the frames need more."""
        planes = np.ascontiguousarray(planes, np.uint8)
        fb = yuv_bytes(jpeg_format(chroma), H, W)
        if fb <= 0 or jpeg_bound(chroma, quality, H, W) <= 0:
            raise ValueError("no such JPEG: chroma %r (one of %r), quality %r (1 .. 100), %r x %r" % (chroma, JPEG_CHROMAS, quality, H, W))
        assert planes.ndim in (1, 2) and planes.shape[-1] == fb, (planes.shape, fb)
        n = planes.size // fb
        cfg = _lib.pb_jpeg_cfg(int(chroma), int(quality))
        offsets = np.zeros(n + 1, np.int64)
        own = out is None
        if own:
            out = np.empty(int(capacity) if capacity is not None else n * (fb // 2 + 1024), np.uint8)
        assert out.dtype == np.uint8 and out.ndim == 1 and out.flags.c_contiguous
        cap = out.size if capacity is None else int(capacity)
        assert 0 <= cap <= out.size
        rc = self.lib.pb_jpeg_encode(self.ctx, C.byref(cfg), _ptr(planes), n, int(H), int(W), _ptr(out), cap, _ptr(offsets))
        if rc < 0 and int(offsets[n]) > cap:
            if not own:
                raise JpegOverflow(self.lib.pb_last_error().decode(), int(offsets[n]), offsets)
            out = np.empty(int(offsets[n]), np.uint8)
            rc = self.lib.pb_jpeg_encode(self.ctx, C.byref(cfg), _ptr(planes), n, int(H), int(W), _ptr(out), out.size, _ptr(offsets))
        check(rc)
        return out, offsets

    def jpeg_encode_dev(self, planes_ptr: int, n: int, H: int, W: int, chroma: int, quality: int, out_ptr: int, capacity: int, offsets_ptr: int):
        """the same on device pointers (dev_alloc), enqueued on the ctx stream (pb_jpeg_encode_dev): sync() waits; offsets_ptr takes n + 1 int64,
        of which the last is the bytes needed - more than `capacity` means the frames past it were not written"""
        check(self.lib.pb_jpeg_encode_dev(self.ctx, C.byref(_lib.pb_jpeg_cfg(int(chroma), int(quality))), C.c_void_p(planes_ptr), n, int(H), int(W),
                                          C.c_void_p(out_ptr), int(capacity), C.c_void_p(offsets_ptr)))

    def i420_to_rgb_dev(self, yuv_ptr: int, n: int, H: int, W: int, rgb_ptr: int):
        """the same on device pointers (dev_alloc), enqueued on the ctx stream (pb_i420_to_rgb_dev): sync() waits"""
        check(self.lib.pb_i420_to_rgb_dev(self.ctx, C.c_void_p(yuv_ptr), n, H, W, C.c_void_p(rgb_ptr)))

    def rgb_to_i420_dev(self, rgb_ptr: int, n: int, H: int, W: int, yuv_ptr: int):
        check(self.lib.pb_rgb_to_i420_dev(self.ctx, C.c_void_p(rgb_ptr), n, H, W, C.c_void_p(yuv_ptr)))

    # bilinear RGB resize (pb_rgb_resize: 8 bit, exact integers, half-pixel centres; tests/resize_ref.py restates it)
    def rgb_resize(self, rgb: np.ndarray, H: int, W: int, i420: bool = False, out: Optional[np.ndarray] = None) -> np.ndarray:
        """RGB uint8 [n, sh, sw, 3] (or one frame [sh, sw, 3]) -> RGB uint8 [n, H, W, 3] ([H, W, 3]), or with i420 I420 frames
        [n, i420_bytes(H, W)] ([i420_bytes]) - the bytes of rgb_to_i420 on the resized frames; `out`: the caller's own (page-locked) array"""
        rgb = np.ascontiguousarray(rgb, np.uint8)
        assert rgb.ndim in (3, 4) and rgb.shape[-1] == 3, rgb.shape
        sh, sw = rgb.shape[-3:-1]
        H, W = int(H), int(W)
        shape = rgb.shape[:-3] + ((i420_bytes(H, W),) if i420 else (H, W, 3))
        res = np.empty(shape, np.uint8) if out is None else out
        assert res.shape == shape and res.dtype == np.uint8 and res.flags.c_contiguous
        check(self.lib.pb_rgb_resize(self.ctx, _ptr(rgb), rgb.size // (sh * sw * 3), sh, sw, H, W, _ptr(res), int(bool(i420))))
        return res

    def rgb_resize_dev(self, rgb_ptr: int, n: int, sh: int, sw: int, H: int, W: int, out_ptr: int, i420: bool = False):
        """the same on device pointers (dev_alloc), enqueued on the ctx stream (pb_rgb_resize_dev): sync() waits"""
        check(self.lib.pb_rgb_resize_dev(self.ctx, C.c_void_p(rgb_ptr), n, sh, sw, H, W, C.c_void_p(out_ptr), int(bool(i420))))

    # what the band's host-pointer and submit calls take as `frames` and give as their encoded `rgb` (the mask band: its id images):
    # "rgb" (the default) or "i420" - pb_set_option "frames_i420" / "rgb_out_i420".  With frame_format = "i420" those calls take
    # [n, i420_bytes(H, W)] arrays and need `size=(H, W)`; with rgb_format = "i420" their rgb arrays are [..., i420_bytes(h, w)] of the output size.
    # frame_format also takes a YuvFormat (pb_set_frame_format): the calls then take [n, yuv_bytes(fmt, H, W)] arrays of that layout's planes.
    # rgb_format does too (pb_set_out_format): their rgb arrays are then [..., yuv_bytes(fmt, h, w)] of the output size.
    @property
    def frame_format(self):
        return self._formats[0]

    @frame_format.setter
    def frame_format(self, fmt):
        if isinstance(fmt, str):
            self._set_format(0, "frames_i420", fmt)
            return
        fmt = YuvFormat(*fmt)
        check(self.lib.pb_set_frame_format(self.ctx, C.byref(fmt.c())))       # a refusal leaves the context and this attribute as they were
        self._formats[0] = fmt

    @property
    def rgb_format(self):
        return self._formats[1]

    @rgb_format.setter
    def rgb_format(self, fmt):
        if isinstance(fmt, str):
            self._set_format(1, "rgb_out_i420", fmt)
            return
        fmt = YuvFormat(*fmt)
        check(self.lib.pb_set_out_format(self.ctx, C.byref(fmt.c())))       # a refusal leaves the context and this attribute as they were
        self._formats[1] = fmt

    # flow bands: their `rgb` results have the clip's H x W instead of the band's sh x sw (pb_set_option "rgb_out_full": resized on the GPU, what
    # a video of the clip's size holds); flow, masks and max displacements stay at sh x sw
    @property
    def rgb_full(self) -> bool:
        return self._rgb_full

    @rgb_full.setter
    def rgb_full(self, on: bool):
        self.set_option("rgb_out_full", int(bool(on)))
        self._rgb_full = bool(on)

    def _set_format(self, which: int, key: str, fmt: str):
        if fmt not in FORMATS:
            raise ValueError("format %r: one of %s" % (fmt, ", ".join(FORMATS)))
        self.set_option(key, FORMATS.index(fmt))
        self._formats[which] = fmt

    def _frames_in(self, frames: np.ndarray, size) -> Tuple[int, int, int]:
        """(n, H, W) of a call's `frames` in the context's frame_format, shape checked"""
        if self.frame_format != "rgb":
            fmt = I420 if self.frame_format == "i420" else self.frame_format
            assert size is not None, "frame_format %r: the call needs size=(H, W)" % (self.frame_format,)
            H, W = int(size[0]), int(size[1])
            assert frames.ndim == 2 and frames.dtype == np.uint8 and frames.shape[1] == yuv_bytes(fmt, H, W), (frames.shape, fmt, H, W)
            return frames.shape[0], H, W
        n, H, W, ch = frames.shape
        assert ch == 3 and (size is None or tuple(size) == (H, W))
        return n, H, W

    def rgb_shape(self, h: int, w: int) -> tuple:
        """trailing shape of one encoded result frame in the context's rgb_format"""
        if self.rgb_format == "rgb":
            return (h, w, 3)
        return (i420_bytes(h, w),) if self.rgb_format == "i420" else (yuv_bytes(self.rgb_format, h, w),)

    def _flow_rgb_shape(self, H: int, W: int, sh: int, sw: int) -> tuple:
        """trailing shape of one encoded frame of a flow call: the band's sh x sw, or with rgb_full the clip's H x W"""
        return self.rgb_shape(H, W) if self.rgb_full else self.rgb_shape(sh, sw)

    def set_option(self, key: str, value: int):
        check(self.lib.pb_set_option(self.ctx, key.encode(), int(value)))


    def set_profiling(self, timing: bool = True, debug_stages: bool = False, accumulate: bool = False):
        """per-launch HIP-event timing (read with kernel_stats), debug stage snapshots, and `accumulate`: keep the records of
        earlier infer calls so that a timed loop can be queried once after it ends"""
        check(self.lib.pb_set_profiling(self.ctx, (1 if timing else 0) | (2 if debug_stages else 0) | (4 if accumulate else 0)))

    # debug stages of the last call (pb_*_get_stage): the band classes name their symbol, the default capacity in floats and whether
    # trailing 1-dims of shape_out are dropped
    _stage_sym: Optional[str] = None
    _stage_cap = 1 << 26
    _stage_squeeze = True

    def stage(self, name: str, cap: Optional[int] = None) -> np.ndarray:
        cap = self._stage_cap if cap is None else cap
        out = np.empty(cap, np.float32)
        shape = (C.c_int64 * 4)()
        n = check(getattr(self.lib, self._stage_sym)(self.ctx, name.encode(), _ptr(out), cap, shape))
        dims = [int(s) for s in shape]
        while self._stage_squeeze and len(dims) > 1 and dims[-1] == 1:
            dims.pop()
        return out[:n].reshape(dims).copy()

    def kernel_stats(self) -> List[dict]:
        arr = (_lib.pb_kernel_stat * 64)()
        n = check(self.lib.pb_get_kernel_stats(self.ctx, arr, 64))
        return [dict(name=arr[i].name.decode(), ms=arr[i].ms, flops=arr[i].flops, exec_flops=arr[i].exec_flops, bytes=arr[i].bytes,
                     launches=arr[i].launches) for i in range(n)]


_SPLIT_INFO = ("pw", "pa", "mx3", "mx2", "sa", "sw", "tapin", "K", "cw", "Cseg", "ldo", "lo8", "lo8_pa")


def _split_info(info, M: int) -> dict:
    d = dict(zip(_SPLIT_INFO, list(info)))
    d["M"] = M
    return d


def _epi_info(info) -> dict:
    return dict(zip(("pw", "pa", "mx2", "sw", "K", "nk16", "mx3", "splitk"), list(info)))


def raft_geometry(h8: int, w8: int) -> List[dict]:
    """the flow_raft band's pyramid plan over an h8 x w8 feature grid (csrc corr_pyramid_geometry; needs no GPU): per level h, w, the tiled
    layout's padded wp / hp and the volume's row stride ld"""
    geo = (C.c_int * 20)()
    check(_lib.load().pb_op_raft_geometry(h8, w8, geo))
    return [dict(h=geo[l * 5], w=geo[l * 5 + 1], wp=geo[l * 5 + 2], hp=geo[l * 5 + 3], ld=geo[l * 5 + 4]) for l in range(4)]


FLOW_GEO = ("sh", "sw", "Hp", "Wp", "padl", "padt", "h8", "w8", "P")


def flow_geometry(H: int, W: int, scale: float, factor: int = 8) -> dict:
    """the flow bands' plan of an H x W frame (csrc flow_chunk.h flow_geometry; needs no GPU): the scaled size, its padding to a multiple of
    `factor` (8 RAFT, 16 GMFlow, 32 two-scale GMFlow) and the 1/8 grid"""
    geo = (C.c_int * 9)()
    check(_lib.load().pb_op_flow_geometry(H, W, C.c_float(scale), factor, geo))
    return dict(zip(FLOW_GEO, geo))


def flow_taps(src: int, dst: int, scale: float):
    """one axis of the flow bands' 8-bit cubic resize table, as the engines upload it (needs no GPU) -> (idx [dst, 4], co [dst, 4] int32)"""
    idx, co = np.empty((dst, 4), np.int32), np.empty((dst, 4), np.int32)
    check(_lib.load().pb_op_flow_taps(src, dst, C.c_float(scale), _ptr(idx), _ptr(co)))
    return idx, co


def corr_layout_index(layout: int, P: int, pld: int) -> np.ndarray:
    """[P, pld] int64: where entry c of source row p sits in a level of flow_raft's correlation volume, layout 0 row-major / 1 source-blocked
    (csrc/corr_layout.h, the function the kernels compile; needs no GPU)"""
    out = np.empty((P, pld), np.int64)
    check(_lib.load().pb_op_corr_layout_index(layout, P, pld, _ptr(out)))
    return out


def gm_geometry(h8: int, w8: int, splits: int = 2) -> dict:
    """the flow_gmflow band's window geometry of an h8 x w8 token grid (csrc gm_geometry): P, window wh x ww = Lw tokens, V^T row strides;
    splits = 8: the two-scale model's 1/4 grid"""
    P, wh, ww = h8 * w8, h8 // splits, w8 // splits
    return dict(h8=h8, w8=w8, P=P, wh=wh, ww=ww, Lw=wh * ww, ldv=-(-(wh * ww) // 32) * 32, ldvP=-(-P // 32) * 32, ns=splits)


def gm_tables(h8: int, w8: int):
    """the two host tables GmflowEngine::prepare_g uploads (csrc sine_positions / shift_regions; needs no GPU): pos [P, 128] float32 and the
    shifted-window region ids [4, Lw] int8 in window order"""
    pos = np.empty((h8 * w8, 128), np.float32)
    reg = np.empty((4, (h8 // 2) * (w8 // 2)), np.int8)
    check(_lib.load().pb_op_gm_tables(h8, w8, _ptr(pos), _ptr(reg)))
    return pos, reg


def gm_tables_n(h: int, w: int, splits: int):
    """gm_tables for a grid cut into splits x splits windows (2 or 8; pb_op_gm_tables_n): pos [P, 128], region ids [splits^2, Lw]"""
    pos = np.empty((h * w, 128), np.float32)
    reg = np.empty((splits * splits, (h // splits) * (w // splits)), np.int8)
    check(_lib.load().pb_op_gm_tables_n(h, w, splits, _ptr(pos), _ptr(reg)))
    return pos, reg


class Ops(_Ctx):
    """Single-kernel entry points (pb_op_*) used by the parity tests."""

    def __init__(self, device: int = 0):
        super().__init__()
        check(self.lib.pb_create(C.byref(self.ctx), device, b"ops", None, 0, None, 0))

    def gemm(self, A, W, bias=None, act: int = 0, tile: int = 0) -> np.ndarray:
        A, W = _f32(A), _f32(W)
        M, K = A.shape
        N = W.shape[0]
        out = np.empty((M, N), np.float32)
        b = None if bias is None else _f32(bias)
        check(self.lib.pb_op_gemm(self.ctx, _ptr(A), _ptr(W), _ptr(b), _ptr(out), M, N, K, act, tile))
        return out

    def corr_volume(self, A, W, ldo: int = 0, guard_rows: int = 32) -> np.ndarray:
        """the flow band's all-pairs correlation kernel alone: [M + guard_rows, ldo] floats, NaN wherever the kernel must not write."""
        A, W = _f32(A), _f32(W)
        M, N = A.shape[0], W.shape[0]
        ldo = ldo or N
        out = np.empty((M + guard_rows, ldo), np.float32)
        check(self.lib.pb_op_corr_volume(self.ctx, _ptr(A), M, _ptr(W), N, ldo, guard_rows, _ptr(out)))
        return out

    def corr_volume_blocked(self, A, W, ldo: int = 0, guard_halfs: int = 4096) -> np.ndarray:
        """the same kernel storing the source-blocked layout (csrc/corr_layout.h): the raw fp16 buffer, round_up(M, 8) * ldo + guard_halfs
        entries, 0x7e7e (a NaN) wherever the kernel did not write."""
        A, W = _f32(A), _f32(W)
        M, N = A.shape[0], W.shape[0]
        ldo = ldo or N
        out = np.empty(-(-M // 8) * 8 * ldo + guard_halfs, np.float16)
        check(self.lib.pb_op_corr_volume_blocked(self.ctx, _ptr(A), M, _ptr(W), N, ldo, guard_halfs, _ptr(out)))
        return out

    def gemm_bench(self, M: int, N: int, K: int, tile: int = 0, epi: int = 0, iters: int = 20) -> float:
        """mean milliseconds per launch on device-resident random data."""
        ms = C.c_double()
        check(self.lib.pb_op_gemm_bench(self.ctx, M, N, K, tile, epi, iters, C.byref(ms)))
        return ms.value

    def attention_bench(self, B: int, heads: int, N: int, variant: int = 0, iters: int = 10) -> float:
        """mean milliseconds per launch of the fused attention kernel on device-resident random Q, K, V."""
        ms = C.c_double()
        check(self.lib.pb_op_attention_bench(self.ctx, B, heads, N, variant, iters, C.byref(ms)))
        return ms.value

    def layernorm(self, x, g, b) -> np.ndarray:
        x, g, b = _f32(x), _f32(g), _f32(b)
        out = np.empty_like(x)
        check(self.lib.pb_op_layernorm(self.ctx, _ptr(x), _ptr(g), _ptr(b), _ptr(out), x.shape[0], x.shape[1]))
        return out

    def attention128(self, q, k, v, region=None) -> np.ndarray:
        """softmax(q k^T / sqrt(128) + mask) v for q, k, v [B, L, 128] (one head); region [B, L] int8: keys of another region get -100"""
        q, k, v = _f32(q), _f32(k), _f32(v)
        B, L, D = q.shape
        assert D == 128 and k.shape == q.shape and v.shape == q.shape
        out = np.empty_like(q)
        rg = None if region is None else np.ascontiguousarray(region, np.int8)
        check(self.lib.pb_op_attention128(self.ctx, _ptr(q), _ptr(k), _ptr(v), _ptr(rg), _ptr(out), B, L))
        return out

    def attention128_split(self, q, k, v, region=None, kxor: int = 0) -> np.ndarray:
        """the same in the flow_gmflow band's split precision; v [B, L, 128 or 32]; region [nreg, L] int8; keys / values of b are those of b ^ kxor"""
        q, k, v = _f32(q), _f32(k), _f32(v)
        B, L, D = q.shape
        vc = v.shape[2]
        assert D == 128 and k.shape == q.shape and v.shape[:2] == (B, L) and vc in (32, 128)
        out = np.empty((B, L, vc), np.float32)
        rg = None if region is None else np.ascontiguousarray(region, np.int8)
        check(self.lib.pb_op_attention128_split(self.ctx, _ptr(q), _ptr(k), _ptr(v), _ptr(rg), 0 if rg is None else rg.shape[0], _ptr(out),
                                                B, L, vc, kxor))
        return out

    def attention(self, q, k, v) -> np.ndarray:
        q, k, v = _f32(q), _f32(k), _f32(v)
        B, Hh, N, d = q.shape
        assert d == 64
        out = np.empty_like(q)
        check(self.lib.pb_op_attention(self.ctx, _ptr(q), _ptr(k), _ptr(v), _ptr(out), B, Hh, N))
        return out

    def conv2d(self, x, w, bias=None, stride=1, pad=None, relu_in=False, relu_out=False) -> np.ndarray:
        x, w = _f32(x), _f32(w)
        B, Ci, H, W = x.shape
        Co, _, ks, _ = w.shape
        pad = ks // 2 if pad is None else pad
        OH, OW = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
        out = np.empty((B, Co, OH, OW), np.float32)
        b = None if bias is None else _f32(bias)
        check(self.lib.pb_op_conv2d(self.ctx, _ptr(x), _ptr(w), _ptr(b), _ptr(out), B, Ci, H, W, Co, ks, stride, pad,
                                    int(relu_in), int(relu_out)))
        return out

    def conv2d_split(self, x, w, bias, skip=None, stride: int = 1, layout: int = 2, sa: int = 1, tapin: int = 0, tile: int = 0,
                     split_out: bool = True, act: int = 0, pre_relu: bool = False, ci_off: int = 0, guard_rows: int = 64):
        """one convolution through the engines' split-precision packing and launch code (pb_op_conv2d_split).  x NHWC [B, H, W, Ci]
        (mx2: [B, H, W, Ctot] of which channels [ci_off, ci_off + Ci) are read); w [Co, Ci, kh, kw].  Returns (raw output buffer as uint8
        [rows, ldo * 2], info dict, kernel symbol)."""
        x, w, bias = _f32(x), _f32(w), _f32(bias)
        B, H, W, Cx = x.shape
        Co, Ci, kh, kw = w.shape
        OH, OW = (H + 2 * (kh // 2) - kh) // stride + 1, (W + 2 * (kw // 2) - kw) // stride + 1
        M = B * OH * OW
        sk = None if skip is None else _f32(skip)
        assert sk is None or sk.shape == (M, Co)
        ldo = (2 if split_out else 1) * (-(-Co // 64) * 64)
        rows = -(-M // 256) * 256 + guard_rows
        out = np.empty((rows, ldo * 2), np.uint8)
        info = (C.c_int * 13)()
        kname = C.create_string_buffer(128)
        check(self.lib.pb_op_conv2d_split(self.ctx, _ptr(x), _ptr(w), _ptr(bias), _ptr(sk), B, H, W, Ci, Cx, ci_off, Co, kh, kw, stride, layout,
                                          sa, tapin, tile, int(split_out), act, int(pre_relu), rows, _ptr(out), info, kname, 128))
        return out, _split_info(info, M), kname.value.decode()

    def dense_split(self, A, w, bias, skip=None, layout: int = 2, sa: int = 1, tile: int = 0, split_out: bool = True, act: int = 0,
                    guard_rows: int = 64):
        """one dense layer A [M, K] x w [N, K]^T through the same packing and launch code (pb_op_dense_split); returns as conv2d_split"""
        A, w, bias = _f32(A), _f32(w), _f32(bias)
        M, K = A.shape
        N = w.shape[0]
        sk = None if skip is None else _f32(skip)
        assert sk is None or sk.shape == (M, N)
        ldo = (2 if split_out else 1) * (-(-N // 64) * 64)
        rows = -(-M // 256) * 256 + guard_rows
        out = np.empty((rows, ldo * 2), np.uint8)
        info = (C.c_int * 13)()
        kname = C.create_string_buffer(128)
        check(self.lib.pb_op_dense_split(self.ctx, _ptr(A), _ptr(w), _ptr(bias), _ptr(sk), M, K, N, layout, sa, tile, int(split_out), act, rows,
                                         _ptr(out), info, kname, 128))
        return out, _split_info(info, M), kname.value.decode()

    # ---- the GEMM's fused ViT epilogues one by one (pb_op_gemm_resid / _qkv / _patch; tests/test_gpu_epilogue_ops.py) ----
    def gemm_resid(self, A, w, bias, gamma, X, layout: int = 0, tile: int = 1, ldr: int = 0, guard_rows: int = 8):
        """X [M, N] (fp32) += A [M, K] (gamma . w)^T + gamma . bias as DepthEngine's proj / fc2 run it (LayerScale folded on the host).
        Returns (raw residual stream as uint8 [M + guard_rows, ldr * 4], info dict, kernel symbol)."""
        A, w, bias, gamma, X = _f32(A), _f32(w), _f32(bias), _f32(gamma), _f32(X)
        M, K = A.shape
        N = w.shape[0]
        ldr = ldr or N
        assert w.shape == (N, K) and bias.shape == (N,) and gamma.shape == (N,) and X.shape == (M, N)
        out = np.empty((M + guard_rows, ldr * 4), np.uint8)
        info = (C.c_int * 8)()
        kname = C.create_string_buffer(128)
        check(self.lib.pb_op_gemm_resid(self.ctx, _ptr(A), _ptr(w), _ptr(bias), _ptr(gamma), _ptr(X), M, N, K, ldr, layout, tile, guard_rows, _ptr(out),
                                        info, kname, 128))
        return out, _epi_info(info), kname.value.decode()

    def gemm_qkv(self, A, w, bias, B: int, ntp: int, layout: int = 0, tile: int = 1, guard_rows: int = 8):
        """A [B ntp, D] x w [3 D, D]^T + bias through the qkv epilogue.  Returns (q, k as uint8 [B heads ntp + guard_rows, 128], vt as uint8
        [B heads 64 + guard_rows, ntp * 2], info dict, kernel symbol)."""
        A, w, bias = _f32(A), _f32(w), _f32(bias)
        M, D = A.shape
        heads = D // 64
        assert M == B * ntp and w.shape == (3 * D, D) and bias.shape == (3 * D,)
        q = np.empty((B * heads * ntp + guard_rows, 128), np.uint8)
        k = np.empty_like(q)
        vt = np.empty((B * heads * 64 + guard_rows, ntp * 2), np.uint8)
        info = (C.c_int * 8)()
        kname = C.create_string_buffer(128)
        check(self.lib.pb_op_gemm_qkv(self.ctx, _ptr(A), _ptr(w), _ptr(bias), B, ntp, D, layout, tile, guard_rows, _ptr(q), _ptr(k), _ptr(vt), info,
                                      kname, 128))
        return q, k, vt, _epi_info(info), kname.value.decode()

    def gemm_patch(self, A, w, bias, pos, B: int, ntp: int, layout: int = 0, guard_rows: int = 8):
        """A [B P, 588] x w [D, 588]^T + bias + pos [1 + P, D] into rows b ntp + 1 + patch of the fp32 residual stream.  Returns (raw stream as
        uint8 [B ntp + guard_rows, D * 4], info dict, kernel symbol)."""
        A, w, bias, pos = _f32(A), _f32(w), _f32(bias), _f32(pos)
        D = w.shape[0]
        P = A.shape[0] // B
        assert A.shape == (B * P, 588) and w.shape == (D, 588) and bias.shape == (D,) and pos.shape == (1 + P, D)
        out = np.empty((B * ntp + guard_rows, D * 4), np.uint8)
        info = (C.c_int * 8)()
        kname = C.create_string_buffer(128)
        check(self.lib.pb_op_gemm_patch(self.ctx, _ptr(A), _ptr(w), _ptr(bias), _ptr(pos), B, P, ntp, D, layout, guard_rows, _ptr(out), info, kname, 128))
        return out, _epi_info(info), kname.value.decode()

    def raft_gru(self, which: str, x, w, bias, h32, z=None, add1=None, add2=None, layout: int = 0, tile: int = 1, guard_rows: int = 8):
        """SepConvGRU's fused epilogues (pb_op_raft_gru_zr / _q).  x [n, H, W, 384], w [256 | 128, gc, kh, kw], h32 [rows, 128]; "q" also takes z
        [rows, 256].  Returns for "zr": (zrb uint8 [rows + guard, 512], rh uint8 [rows + guard, ld * 2], info, kernel); for "q": (out uint8
        [rows + guard, ld * 2], h32 uint8 [rows + guard, 512] with its guard rows preset to 0xFF, info, kernel); ld = 576 for mx2 (3) else 384."""
        x, w, bias = _f32(x), _f32(w), _f32(bias)
        n, H, W, _ = x.shape
        N, gc, kh, kw = w.shape
        rows, ld = n * H * W, 576 if layout == 3 else 384
        assert x.shape[3] == 384 and N == (256 if which == "zr" else 128) and bias.shape == (N,)
        hb = np.full((rows + guard_rows, 128), np.nan, np.float32)
        hb.view(np.uint8)[:] = 0xFF
        hb[:rows] = _f32(h32)
        a1 = None if add1 is None else _f32(add1)
        a2 = None if add2 is None else _f32(add2)
        assert all(a is None or a.shape == (rows, N) for a in (a1, a2))
        info = (C.c_int * 8)()
        kname = C.create_string_buffer(128)
        if which == "zr":
            zrb = np.empty((rows + guard_rows, 512), np.uint8)
            rh = np.empty((rows + guard_rows, ld * 2), np.uint8)
            check(self.lib.pb_op_raft_gru_zr(self.ctx, _ptr(x), _ptr(w), _ptr(bias), _ptr(a1), _ptr(a2), _ptr(hb), n, H, W, gc, kh, kw, layout, tile,
                                             guard_rows, _ptr(zrb), _ptr(rh), info, kname, 128))
            return zrb, rh, _epi_info(info), kname.value.decode()
        zz = _f32(z)
        assert zz.shape == (rows, 256)
        out = np.empty((rows + guard_rows, ld * 2), np.uint8)
        check(self.lib.pb_op_raft_gru_q(self.ctx, _ptr(x), _ptr(w), _ptr(bias), _ptr(a1), _ptr(a2), _ptr(zz), _ptr(hb), n, H, W, gc, kh, kw, layout, tile,
                                        guard_rows, _ptr(out), info, kname, 128))
        return out, hb.view(np.uint8).reshape(rows + guard_rows, 512), _epi_info(info), kname.value.decode()

    def conv_pixshuf(self, x, w, bias, layout: int = 0, act: int = 0, guard_rows: int = 8):
        """the convolution form of the pixel shuffle (RAFT's stem): x [B, H, W, 64], w [256, 64, 3, 3], bias [64], s = 2.  Returns (raw output as
        uint8 [B 2H 2W + guard_rows, ldo * 2], info dict, kernel symbol)."""
        x, w, bias = _f32(x), _f32(w), _f32(bias)
        B, H, W, Cc = x.shape
        assert Cc == 64 and w.shape == (256, 64, 3, 3) and bias.shape == (64,)
        out = np.empty((B * H * W * 4 + guard_rows, (2 if layout else 1) * 128), np.uint8)
        info = (C.c_int * 8)()
        kname = C.create_string_buffer(128)
        check(self.lib.pb_op_conv_pixshuf(self.ctx, _ptr(x), _ptr(w), _ptr(bias), B, H, W, layout, act, guard_rows, _ptr(out), info, kname, 128))
        return out, _epi_info(info), kname.value.decode()

    def gemm_fc1(self, A, w, bias, tile: int = 1, guard_rows: int = 8):
        """gelu(A [M, K] w [N, K]^T + bias) as the split ViT's fc1 runs it: fp16 weights on the MX build of the kernel, an e4m3 copy of the
        stored fp16 behind it.  Returns (raw rows as uint8 [M + guard_rows, 3 N], info dict, kernel symbol)."""
        A, w, bias = _f32(A), _f32(w), _f32(bias)
        M, K = A.shape
        N = w.shape[0]
        assert w.shape == (N, K) and bias.shape == (N,)
        out = np.empty((M + guard_rows, 3 * N), np.uint8)
        info = (C.c_int * 8)()
        kname = C.create_string_buffer(128)
        check(self.lib.pb_op_gemm_fc1(self.ctx, _ptr(A), _ptr(w), _ptr(bias), M, K, N, tile, guard_rows, _ptr(out), info, kname, 128))
        return out, _epi_info(info), kname.value.decode()

    def gemm_pixshuf(self, x, wt, bias, s: int, layout: int = 0, tile: int = 1, guard_rows: int = 8):
        """a transposed convolution (kernel == stride == s) as a 1 x 1 GEMM with the pixel-shuffle epilogue (EPI_PIXSHUF).  x [B, h, w, C], wt
        [C, C, s, s], bias [C]; layout 0 fp16, 1 split16 ([hi | lo]), 2 mx3 ([hi | hi8 | lo8]) for the input map and the output.  Returns (raw
        output as uint8 [B h s w s + guard_rows, ldo * 2], info dict, kernel symbol)."""
        x, wt, bias = _f32(x), _f32(wt), _f32(bias)
        B, h, w, Cc = x.shape
        assert wt.shape == (Cc, Cc, s, s) and bias.shape == (Cc,)
        ldo = (2 if layout else 1) * (-(-Cc // 64) * 64)
        out = np.empty((B * h * s * w * s + guard_rows, ldo * 2), np.uint8)
        info = (C.c_int * 8)()
        kname = C.create_string_buffer(128)
        check(self.lib.pb_op_gemm_pixshuf(self.ctx, _ptr(x), _ptr(wt), _ptr(bias), B, h, w, Cc, s, layout, tile, guard_rows, _ptr(out), info, kname, 128))
        return out, _epi_info(info), kname.value.decode()

    def conv_head(self, x, w, bias, w2, b2: float, layout: int = 0, guard_rows: int = 8):
        """the DPT head's fused output_conv2 (EPI_HEAD): x NHWC [B, H, W, C], w [32, C, 3, 3] -> relu(relu(conv + bias) . w2 + b2), one float per
        pixel.  layout 0 fp16, 1 split16 (map [hi | lo]), 2 mx3.  Returns (float32 [B H W + guard_rows] raw, info dict, kernel symbol)."""
        x, w, bias, w2 = _f32(x), _f32(w), _f32(bias), _f32(w2)
        B, H, W, Cc = x.shape
        assert w.shape == (32, Cc, 3, 3) and bias.shape == (32,) and w2.shape == (32,)
        out = np.empty(B * H * W + guard_rows, np.float32)
        info = (C.c_int * 8)()
        kname = C.create_string_buffer(128)
        check(self.lib.pb_op_conv_head(self.ctx, _ptr(x), _ptr(w), _ptr(bias), _ptr(w2), float(b2), B, H, W, Cc, layout, guard_rows, _ptr(out), info,
                                       kname, 128))
        return out, _epi_info(info), kname.value.decode()

    # ---- the flow_raft band's kernels one by one (pb_op_raft_*; tests/test_gpu_raft_ops.py) ----
    def raft_lookup(self, fmap1, fmap2, flow, o8: bool = False, guard_rows: int = 8, want_levels: bool = False):
        """pooling, tiling, the all-pairs volumes and the 9 x 9 x 4 lookup as RaftEngine::infer launches them.  fmap1 [n, P, 256], fmap2
        [n, h8, w8, 256], flow [n P, 2] -> (raw rows as uint8 [n P + guard_rows, ldo * 2], [levels [n P, h_l, w_l]] or None)"""
        fmap1, fmap2, flow = _f32(fmap1), _f32(fmap2), _f32(flow)
        n, h8, w8, _ = fmap2.shape
        rows = n * h8 * w8
        assert fmap1.shape == (n, h8 * w8, 256) and fmap2.shape[3] == 256 and flow.shape == (rows, 2)
        ldo = 576 if o8 else 384
        out = np.empty((rows + guard_rows, ldo * 2), np.uint8)
        geo = raft_geometry(h8, w8)
        lv = np.empty(sum(rows * g["h"] * g["w"] for g in geo), np.float32) if want_levels else None
        check(self.lib.pb_op_raft_lookup(self.ctx, _ptr(fmap1), _ptr(fmap2), _ptr(flow), n, h8, w8, int(o8), guard_rows, _ptr(out), _ptr(lv)))
        levels = None
        if want_levels:
            levels, o = [], 0
            for g in geo:
                k = rows * g["h"] * g["w"]
                levels.append(lv[o:o + k].reshape(rows, g["h"], g["w"]))
                o += k
        return out, levels

    def raft_lookup_otf(self, fmap1, fmap2, flow, o8: bool = False, guard_rows: int = 8) -> np.ndarray:
        """--alternate_corr: pooling and the 9 x 9 x 4 lookup straight from the feature maps (corr_otf.hip) as RaftEngine::infer launches them
        with set_alternate_corr(True).  Arguments and raw rows as raft_lookup; there is no volume, so no levels."""
        fmap1, fmap2, flow = _f32(fmap1), _f32(fmap2), _f32(flow)
        n, h8, w8, _ = fmap2.shape
        rows = n * h8 * w8
        assert fmap1.shape == (n, h8 * w8, 256) and fmap2.shape[3] == 256 and flow.shape == (rows, 2)
        out = np.empty((rows + guard_rows, (576 if o8 else 384) * 2), np.uint8)
        check(self.lib.pb_op_raft_lookup_otf(self.ctx, _ptr(fmap1), _ptr(fmap2), _ptr(flow), n, h8, w8, int(o8), guard_rows, _ptr(out)))
        return out

    def raft_convf1(self, flow, w, bias, passes: int = 2, o8: bool = True, gemm_path: bool = False, guard_rows: int = 8) -> np.ndarray:
        """flow [n, h8, w8, 2], w [128, 2, 7, 7] -> raw rows uint8 [n h8 w8 + guard_rows, ldo * 2] (ldo 192 with the e4m3 copy at byte 256, else 128)"""
        flow, w, bias = _f32(flow), _f32(w), _f32(bias)
        n, h8, w8, _ = flow.shape
        assert w.shape == (128, 2, 7, 7) and bias.shape == (128,) and flow.shape[3] == 2
        out = np.empty((n * h8 * w8 + guard_rows, (192 if o8 else 128) * 2), np.uint8)
        check(self.lib.pb_op_raft_convf1(self.ctx, _ptr(flow), _ptr(w), _ptr(bias), n, h8, w8, passes, int(o8), int(gemm_path), guard_rows, _ptr(out)))
        return out

    def raft_flow_head2(self, x, w, bias, flow, split: bool = True, guard_rows: int = 8) -> np.ndarray:
        """x [n, H, W, 256], w [2, 256, 3, 3], flow [n H W, 2] -> flow + conv (float32 [n H W + guard_rows, 2], guard rows NaN)"""
        x, w, bias, flow = _f32(x), _f32(w), _f32(bias), _f32(flow)
        n, H, W, _ = x.shape
        assert x.shape[3] == 256 and w.shape == (2, 256, 3, 3) and flow.shape == (n * H * W, 2)
        buf = np.empty((n * H * W + guard_rows, 2), np.float32)
        buf[:n * H * W] = flow
        check(self.lib.pb_op_raft_flow_head2(self.ctx, _ptr(x), _ptr(w), _ptr(bias), _ptr(buf), n, H, W, int(split), guard_rows))
        return buf

    def raft_upsample(self, flow, mask, h8: int, w8: int, pad_l: int, pad_t: int, sh: int, sw: int, guard: int = 64):
        """flow [n, h8 w8, 2], mask [n h8 w8, 576] -> (up [n, sh, sw, 2], guard floats behind it, maxd [n])"""
        flow, mask = _f32(flow), _f32(mask)
        n = flow.shape[0]
        assert flow.shape == (n, h8 * w8, 2) and mask.shape == (n * h8 * w8, 576)
        buf = np.empty(n * sh * sw * 2 + guard, np.float32)
        mx = np.empty(n, np.float32)
        check(self.lib.pb_op_raft_upsample(self.ctx, _ptr(flow), _ptr(mask), n, h8, w8, pad_l, pad_t, sh, sw, guard, _ptr(buf), _ptr(mx)))
        return buf[:n * sh * sw * 2].reshape(n, sh, sw, 2), buf[n * sh * sw * 2:], mx

    def raft_instnorm(self, a, b=None, layout: int = 0, stats_lo: bool = True, normalise_b: bool = False, inplace: bool = False,
                      guard_rows: int = 8):
        """a (and b) [B, HW, C] -> (stats [B, C, 2] = {mean, rstd}, raw out uint8 [B HW + guard_rows, ld * 2]); layout 0 [C], 1 [hi | lo],
        2 [hi | hi8 | lo8]"""
        a = _f32(a)
        B, HW, Cc = a.shape
        bb = None if b is None else _f32(b)
        assert bb is None or bb.shape == a.shape
        ld = 2 * Cc if layout else Cc
        st = np.empty((B, Cc, 2), np.float32)
        out = np.empty((B * HW + guard_rows, ld * 2), np.uint8)
        check(self.lib.pb_op_raft_instnorm(self.ctx, _ptr(a), _ptr(bb), B, HW, Cc, layout, int(stats_lo), 0 if bb is None else (2 if normalise_b else 1),
                                           int(inplace), guard_rows, _ptr(st), _ptr(out)))
        return st, out

    def raft_state(self, ctx_rows, flow, ld: int = 576, inp_off: int = 256, guard_rows: int = 8):
        """init_state + put_flow -> (h32 [rows + guard, 128], hx raw, hx2 raw uint8 [rows + guard, ld * 2], flow after init [rows + guard, 2])"""
        ctx_rows, flow = _f32(ctx_rows), _f32(flow)
        rows = ctx_rows.shape[0]
        assert ctx_rows.shape == (rows, 256) and flow.shape == (rows, 2)
        h32 = np.empty((rows + guard_rows, 128), np.float32)
        hx = np.empty((rows + guard_rows, ld * 2), np.uint8)
        hx2 = np.empty_like(hx)
        f0 = np.empty((rows + guard_rows, 2), np.float32)
        check(self.lib.pb_op_raft_state(self.ctx, _ptr(ctx_rows), _ptr(flow), rows, ld, inp_off, guard_rows, _ptr(h32), _ptr(hx), _ptr(hx2), _ptr(f0)))
        return h32, hx, hx2, f0

    # ---- the flow bands' frame prep and flow tail (pb_op_flow_*; tests/test_gpu_flow_io_ops.py) ----
    def flow_prep(self, frames, scale: float, factor: int, layout: int, norm_mode: int, inference_size=None, guard_rows: int = 8, guard: int = 64):
        """frames uint8 [n, H, W, 3] through one launch of the prep kernel -> (geo dict (flow_geometry; Hp, Wp the inference size when given),
        raw uint8 [n Hp/4 Wp/4 + guard_rows, 128 (layout 0) | 256] one 4 x 4 block per row, scaled uint8 [n, sh, sw, 3], the guard bytes behind
        it, lo8_pa)"""
        frames = np.ascontiguousarray(frames, np.uint8)
        n, H, W, _ = frames.shape
        geo = flow_geometry(H, W, scale, factor)
        ih, iw = inference_size if inference_size else (0, 0)
        if inference_size:
            geo.update(Hp=ih, Wp=iw, padl=0, padt=0, h8=ih // 8, w8=iw // 8, P=(ih // 8) * (iw // 8))
        rows = n * (geo["Hp"] // 4) * (geo["Wp"] // 4)
        raw = np.empty((rows + guard_rows, 256 if layout else 128), np.uint8)
        sc = np.empty(n * geo["sh"] * geo["sw"] * 3 + guard, np.uint8)
        pa = C.c_int(-1)
        check(self.lib.pb_op_flow_prep(self.ctx, _ptr(frames), n, H, W, C.c_float(scale), factor, layout, norm_mode, ih, iw, guard_rows, guard,
                                       _ptr(raw), _ptr(sc), C.byref(pa)))
        cut = n * geo["sh"] * geo["sw"] * 3
        return geo, raw, sc[:cut].reshape(n, geo["sh"], geo["sw"], 3), sc[cut:], pa.value

    def flow_resize_back(self, flow, sh: int, sw: int, guard: int = 64):
        """flow [n, ih, iw, 2] -> (out [n, sh, sw, 2], guard floats behind it, maxd [n])"""
        flow = _f32(flow)
        n, ih, iw, _ = flow.shape
        buf = np.empty(n * sh * sw * 2 + guard, np.float32)
        mx = np.empty(n, np.float32)
        check(self.lib.pb_op_flow_resize_back(self.ctx, _ptr(flow), n, ih, iw, sh, sw, guard, _ptr(buf), _ptr(mx)))
        return buf[:n * sh * sw * 2].reshape(n, sh, sw, 2), buf[n * sh * sw * 2:], mx

    def flow_encode(self, flow, maxd, guard: int = 64):
        """flow [n, sh, sw, 2], maxd [n] -> (rgb uint8 [n, sh, sw, 3], guard bytes behind it, max_out [n])"""
        flow, maxd = _f32(flow), _f32(maxd)
        n, sh, sw, _ = flow.shape
        assert maxd.shape == (n,)
        buf = np.empty(n * sh * sw * 3 + guard, np.uint8)
        mx = np.empty(n, np.float32)
        check(self.lib.pb_op_flow_encode(self.ctx, _ptr(flow), _ptr(maxd), n, sh, sw, guard, _ptr(buf), _ptr(mx)))
        return buf[:n * sh * sw * 3].reshape(n, sh, sw, 3), buf[n * sh * sw * 3:], mx

    def flow_fwdbwd_mask(self, flows, alpha_1: float = 0.05, alpha_2: float = 0.5) -> np.ndarray:
        """pb_flow_fwdbwd_mask on an ops context: flows [n, 2, sh, sw, 2] -> bool [n, 2, sh, sw]"""
        return _fwdbwd_mask(self, flows, alpha_1, alpha_2)

    # ---- the flow_gmflow band's kernels one by one (pb_op_gm_*, pb_op_attention128_cfg; tests/test_gpu_gmflow_ops.py) ----
    # raw buffers come back as uint8 [rows + guard_rows, bytes per row]: 0xFF wherever the kernel did not write
    def gm_tokens(self, feat, pos, guard_rows: int = 8):
        """feat [NP + 1, P, 128], pos [P, 128] -> (X float32 [2 NP P + guard, 128], Xs raw [.., 512])"""
        feat, pos = _f32(feat), _f32(pos)
        F, P, _ = feat.shape
        assert feat.shape[2] == 128 and pos.shape == (P, 128) and F >= 2
        R = (F - 1) * 2 * P
        X = np.empty((R + guard_rows, 128), np.float32)
        Xs = np.empty((R + guard_rows, 512), np.uint8)
        check(self.lib.pb_op_gm_tokens(self.ctx, _ptr(feat), _ptr(pos), F - 1, P, guard_rows, _ptr(X), _ptr(Xs)))
        return X, Xs

    # ---- the two-scale model's forms (tests/test_gpu_gmflow_scale2_ops.py) ----
    def gm_tokens_warped(self, feat, warped, pos, dirs: int, guard_rows: int = 8):
        """feat [B / dirs + 1, P, 128], warped [B, P, 128], pos [P, 128] -> (X float32 [2 B P + guard, 128], Xs raw [.., 512]): image 2 b is
        frame b // dirs + b % dirs plus pos, image 2 b + 1 is warped[b] plus pos"""
        feat, warped, pos = _f32(feat), _f32(warped), _f32(pos)
        B, P, _ = warped.shape
        assert feat.shape == (B // dirs + 1, P, 128) and pos.shape == (P, 128) and B % dirs == 0
        X = np.empty((2 * B * P + guard_rows, 128), np.float32)
        Xs = np.empty((2 * B * P + guard_rows, 512), np.uint8)
        check(self.lib.pb_op_gm_tokens_warped(self.ctx, _ptr(feat), _ptr(warped), _ptr(pos), B, dirs, P, guard_rows, _ptr(X), _ptr(Xs)))
        return X, Xs

    def gm_warp(self, flow8, feat4, h8: int, w8: int, dirs: int, guard_rows: int = 8):
        """flow8 [B, h8 w8, 2], feat4 [B / dirs + 1, 4 h8 w8, 128] -> raw (flow_up [4 B h8 w8 + guard, 2], warped [4 B h8 w8 + guard, 128])"""
        flow8, feat4 = _f32(flow8), _f32(feat4)
        B, P8 = flow8.shape[0], h8 * w8
        assert flow8.shape == (B, P8, 2) and feat4.shape == (B // dirs + 1, 4 * P8, 128) and B % dirs == 0
        up = np.empty((4 * B * P8 + guard_rows, 2), np.float32)
        wp = np.empty((4 * B * P8 + guard_rows, 128), np.float32)
        check(self.lib.pb_op_gm_warp(self.ctx, _ptr(flow8), _ptr(feat4), B, dirs, h8, w8, guard_rows, _ptr(up), _ptr(wp)))
        return up, wp

    def gm_upsample(self, flow, mask, h: int, w: int, factor: int, pad_l: int, pad_t: int, sh: int, sw: int, guard: int = 16):
        """flow [n, h w, 2], mask [n, h w, 9 factor^2] -> (raw up float32 [n sh sw 2 + guard], max displacement [n]); factor 8 or 4"""
        flow, mask = _f32(flow), _f32(mask)
        n = flow.shape[0]
        assert flow.shape == (n, h * w, 2) and mask.shape == (n, h * w, 9 * factor * factor)
        up = np.empty(n * sh * sw * 2 + guard, np.float32)
        mx = np.empty(n, np.float32)
        check(self.lib.pb_op_gm_upsample(self.ctx, _ptr(flow), _ptr(mask), n, h, w, factor, pad_l, pad_t, sh, sw, guard, _ptr(up), _ptr(mx)))
        return up, mx

    def gm_pack_n(self, src, h: int, w: int, splits: int, jobs, shifted: bool, guard_rows: int = 8):
        """gm_pack over splits x splits windows: per job raw [splits^2 images Lw + guard, 512] or [splits^2 images 256 + guard, 2 ldv]"""
        src = _f32(src)
        g = gm_geometry(h, w, splits)
        images, ld, nw = src.shape[0] // g["P"], src.shape[1], splits * splits
        assert src.shape[0] == images * g["P"] and 1 <= len(jobs) <= 5
        outs = [np.empty((images * nw * 256 + guard_rows, g["ldv"] * 2) if vt else (images * nw * g["Lw"] + guard_rows, 512), np.uint8) for _, vt in jobs]
        cols = (C.c_int * 5)(*[c for c, _ in jobs])
        kinds = (C.c_int * 5)(*[int(vt) for _, vt in jobs])
        ptrs = (C.c_void_p * 5)(*[o.ctypes.data for o in outs])
        check(self.lib.pb_op_gm_pack_n(self.ctx, _ptr(src), images, h, w, splits, ld, len(jobs), cols, kinds, int(shifted), guard_rows, ptrs))
        return outs

    def gm_ln_n(self, M, gamma, beta, X, h: int, w: int, splits: int, windowed: bool, shifted: bool, mode: int, guard_rows: int = 8):
        """gm_ln over splits x splits windows"""
        M, gamma, beta, X = _f32(M), _f32(gamma), _f32(beta), _f32(X)
        rows, xrows = M.shape[0], X.shape[0]
        Xb = np.empty((xrows + guard_rows, 128), np.float32)
        Xb.view(np.uint8)[...] = 0xFF
        Xb[:xrows] = X
        out = np.empty((xrows + guard_rows, 1024 if mode else 512), np.uint8)
        check(self.lib.pb_op_gm_ln_n(self.ctx, _ptr(M), _ptr(gamma), _ptr(beta), _ptr(Xb), rows, xrows, h, w, splits, int(windowed), int(shifted), mode,
                                     guard_rows, _ptr(out)))
        return Xb, out

    def gm_window_block_n(self, Y, X, gamma, beta, h: int, w: int, splits: int, shifted: bool, cross: bool, split: int = 1,
                          pv_single: bool = False) -> np.ndarray:
        """gm_window_block over splits x splits windows; pv_single False: P and V split, the attention a two-scale context launches (True: the
        one-scale model's, gm_window_block's)"""
        Y, X, gamma, beta = _f32(Y), _f32(X).copy(), _f32(gamma), _f32(beta)
        images = X.shape[0] // (h * w)
        assert X.shape == (images * h * w, 128) and Y.shape == (X.shape[0], 384)
        check(self.lib.pb_op_gm_window_block_n(self.ctx, _ptr(Y), _ptr(X), _ptr(gamma), _ptr(beta), images, h, w, splits, int(shifted), int(cross), split,
                                               int(pv_single)))
        return X

    def gm_split_rows(self, src, Cc: int, guard_rows: int = 8) -> np.ndarray:
        """src [rows, ld >= Cc] -> raw [rows + guard, 4 Cc] ([hi | lo] halfs)"""
        src = _f32(src)
        rows, ld = src.shape
        out = np.empty((rows + guard_rows, 4 * Cc), np.uint8)
        check(self.lib.pb_op_gm_split_rows(self.ctx, _ptr(src), rows, ld, Cc, guard_rows, _ptr(out)))
        return out

    def gm_grid_vt(self, h8: int, w8: int, guard_rows: int = 8) -> np.ndarray:
        out = np.empty((64 + guard_rows, gm_geometry(h8, w8)["ldvP"] * 2), np.uint8)
        check(self.lib.pb_op_gm_grid_vt(self.ctx, h8, w8, guard_rows, _ptr(out)))
        return out

    def gm_pack(self, src, h8: int, w8: int, jobs, shifted: bool, guard_rows: int = 8):
        """src [images P, ld]; jobs [(first column, is_vt)] (at most 5) -> per job raw [4 images Lw + guard, 512] or [4 images 256 + guard, 2 ldv]"""
        src = _f32(src)
        g = gm_geometry(h8, w8)
        images, ld = src.shape[0] // g["P"], src.shape[1]
        assert src.shape[0] == images * g["P"] and 1 <= len(jobs) <= 5
        outs = [np.empty((images * 4 * 256 + guard_rows, g["ldv"] * 2) if vt else (images * 4 * g["Lw"] + guard_rows, 512), np.uint8) for _, vt in jobs]
        cols = (C.c_int * 5)(*[c for c, _ in jobs])
        kinds = (C.c_int * 5)(*[int(vt) for _, vt in jobs])
        ptrs = (C.c_void_p * 5)(*[o.ctypes.data for o in outs])
        check(self.lib.pb_op_gm_pack(self.ctx, _ptr(src), images, h8, w8, ld, len(jobs), cols, kinds, int(shifted), guard_rows, ptrs))
        return outs

    def gm_ln(self, M, gamma, beta, X, h8: int, w8: int, windowed: bool, shifted: bool, mode: int, guard_rows: int = 8):
        """M [rows, 128]; X [xrows, 128] -> (X afterwards float32 [xrows + guard, 128] with the guard rows as preset, raw out [xrows + guard,
        512 or 1024]); rows <= xrows (windowed: X is whole images)"""
        M, gamma, beta, X = _f32(M), _f32(gamma), _f32(beta), _f32(X)
        rows, xrows = M.shape[0], X.shape[0]
        Xb = np.empty((xrows + guard_rows, 128), np.float32)
        Xb.view(np.uint8)[...] = 0xFF
        Xb[:xrows] = X
        out = np.empty((xrows + guard_rows, 1024 if mode else 512), np.uint8)
        check(self.lib.pb_op_gm_ln(self.ctx, _ptr(M), _ptr(gamma), _ptr(beta), _ptr(Xb), rows, xrows, h8, w8, int(windowed), int(shifted), mode,
                                   guard_rows, _ptr(out)))
        return Xb, out

    def gm_match_flow(self, O, h8: int, w8: int, guard_rows: int = 8):
        """O [B, P, 32] -> (flow float32 [B P + guard, 2], vt raw [64 B + guard, 2 ldvP])"""
        O = _f32(O)
        B, P, _ = O.shape
        assert O.shape[1:] == (h8 * w8, 32)
        flow = np.empty((B * P + guard_rows, 2), np.float32)
        vt = np.empty((64 * B + guard_rows, gm_geometry(h8, w8)["ldvP"] * 2), np.uint8)
        check(self.lib.pb_op_gm_match_flow(self.ctx, _ptr(O), B, h8, w8, guard_rows, _ptr(flow), _ptr(vt)))
        return flow, vt

    def gm_upsampler_in(self, O, X, img_step: int, guard_rows: int = 8):
        """O [B, P, 32], X [images, P, 128] -> (flow float32 [B P + guard, 2], map raw [B P + guard, 768])"""
        O, X = _f32(O), _f32(X)
        B, P, _ = O.shape
        assert X.shape[1:] == (P, 128)
        flow = np.empty((B * P + guard_rows, 2), np.float32)
        mp = np.empty((B * P + guard_rows, 768), np.uint8)
        check(self.lib.pb_op_gm_upsampler_in(self.ctx, _ptr(O), _ptr(X), B, X.shape[0], P, img_step, guard_rows, _ptr(flow), _ptr(mp)))
        return flow, mp

    def attention128_cfg(self, q, k, v, region=None, split: int = 1, pv_single: int = 0, v_shared: bool = False, kxor: int = 0, ldq: int = 256,
                         strided: int = 0, fill: float = 0.0) -> np.ndarray:
        """attention128.hip's general form (pb_op_attention128_cfg): q, k [B, L, 128], v [1 if v_shared else B, L, 32 or 128] -> [B, L, vcols]"""
        q, v = _f32(q), _f32(v)
        k = None if k is None else _f32(k)
        B, L, _ = q.shape
        vc = v.shape[2]
        assert q.shape[2] == 128 and (k is None or k.shape == q.shape) and v.shape[:2] == (1 if v_shared else B, L)
        rg = None if region is None else np.ascontiguousarray(region, np.int8)
        out = np.empty((B, L, vc), np.float32)
        check(self.lib.pb_op_attention128_cfg(self.ctx, _ptr(q), _ptr(k), _ptr(v), _ptr(rg), 0 if rg is None else rg.shape[0], _ptr(out), B, L,
                                              split, pv_single, vc, int(v_shared), kxor, ldq, strided, fill))
        return out

    def gm_window_block(self, Y, X, gamma, beta, h8: int, w8: int, shifted: bool, cross: bool, split: int = 1) -> np.ndarray:
        """Y [images P, 384] = q | k | v, X [images P, 128] -> X + LayerNorm(window attention), float32 [images P, 128]"""
        Y, X, gamma, beta = _f32(Y), _f32(X).copy(), _f32(gamma), _f32(beta)
        images = X.shape[0] // (h8 * w8)
        assert X.shape == (images * h8 * w8, 128) and Y.shape == (X.shape[0], 384)
        check(self.lib.pb_op_gm_window_block(self.ctx, _ptr(Y), _ptr(X), _ptr(gamma), _ptr(beta), images, h8, w8, int(shifted), int(cross), split))
        return X

    def gm_match(self, tokens, h8: int, w8: int, dirs: int, split: int = 1) -> np.ndarray:
        """tokens [2 NP, P, 128] -> matched flow [NP dirs, P, 2]"""
        tokens = _f32(tokens)
        NP = tokens.shape[0] // 2
        assert tokens.shape == (2 * NP, h8 * w8, 128)
        flow = np.empty((NP * dirs, h8 * w8, 2), np.float32)
        check(self.lib.pb_op_gm_match(self.ctx, _ptr(tokens), NP, h8, w8, dirs, split, _ptr(flow)))
        return flow

    def gm_propagate(self, q, k, flow_in, X, h8: int, w8: int, dirs: int, split: int = 1, guard_rows: int = 8):
        """q, k, X [2 NP, P, 128], flow_in [NP dirs, P, 2] -> (the fp32 flow match_flow made of flow_in + coordinate, propagated flow, both
        [NP dirs, P, 2]; upsampler map raw [NP dirs P + guard, 768])"""
        q, k, flow_in, X = _f32(q), _f32(k), _f32(flow_in), _f32(X)
        NP, P = q.shape[0] // 2, h8 * w8
        B = NP * dirs
        assert q.shape == (2 * NP, P, 128) and k.shape == q.shape and X.shape == q.shape and flow_in.shape == (B, P, 2)
        fm, fp = np.empty((B, P, 2), np.float32), np.empty((B, P, 2), np.float32)
        mp = np.empty((B * P + guard_rows, 768), np.uint8)
        check(self.lib.pb_op_gm_propagate(self.ctx, _ptr(q), _ptr(k), _ptr(flow_in), _ptr(X), NP, h8, w8, dirs, split, guard_rows, _ptr(fm), _ptr(fp),
                                          _ptr(mp)))
        return fm, fp, mp

    def gm_local_match(self, tokens, h8: int, w8: int, dirs: int, radius: int, guard_rows: int = 8) -> np.ndarray:
        """tokens [2 NP, P, 128] -> raw flow [NP dirs P + guard, 2] of the local matching over (2 radius + 1)^2 target tokens"""
        tokens = _f32(tokens)
        NP = tokens.shape[0] // 2
        assert tokens.shape == (2 * NP, h8 * w8, 128)
        flow = np.empty((NP * dirs * h8 * w8 + guard_rows, 2), np.float32)
        check(self.lib.pb_op_gm_local_match(self.ctx, _ptr(tokens), NP, h8, w8, dirs, radius, guard_rows, _ptr(flow)))
        return flow

    def gm_local_propagate(self, q, k, flow_in, h8: int, w8: int, img_step: int, radius: int, guard_rows: int = 8) -> np.ndarray:
        """q, k [B img_step, P, 128], flow_in [B, P, 2] -> raw [B P + guard, 32]: the local-window propagation owns columns 0, 1"""
        q, k, flow_in = _f32(q), _f32(k), _f32(flow_in)
        B, P = flow_in.shape[0], h8 * w8
        assert q.shape == (B * img_step, P, 128) and k.shape == q.shape and flow_in.shape == (B, P, 2)
        out = np.empty((B * P + guard_rows, 32), np.float32)
        check(self.lib.pb_op_gm_local_propagate(self.ctx, _ptr(q), _ptr(k), _ptr(flow_in), B, h8, w8, img_step, radius, guard_rows, _ptr(out)))
        return out

    # ---- the mask_mmdet band's kernels one by one (pb_op_mask_*; tests/test_gpu_mask_ops.py) ----
    # maps come back raw: uint8 [rows + guard_rows, bytes per row], 0xFF wherever the kernel did not write.  split: [hi | lo] rows
    @staticmethod
    def _i32(a) -> np.ndarray:
        return np.ascontiguousarray(a, dtype=np.int32)

    def mask_prep(self, frames, nh: int, nw: int, Hp: int, Wp: int, xt, yt, split: bool, guard_rows: int = 8):
        """frames uint8 [n, H, W, 3], xt [nw, 4], yt [nh, 4] -> (raw [n Hp/4 Wp/4 + guard, 128 (1 + split)], chw float32 [3 n Hp Wp + guard])"""
        frames = np.ascontiguousarray(frames, np.uint8)
        n, H, W, _ = frames.shape
        xt, yt = self._i32(xt), self._i32(yt)
        assert xt.shape == (nw, 4) and yt.shape == (nh, 4) and frames.shape[3] == 3
        out = np.empty((n * (Hp // 4) * (Wp // 4) + guard_rows, 128 * (1 + int(split))), np.uint8)
        chw = np.empty(3 * n * Hp * Wp + guard_rows, np.float32)
        check(self.lib.pb_op_mask_prep(self.ctx, _ptr(frames), n, H, W, nh, nw, Hp, Wp, _ptr(xt), _ptr(yt), int(split), guard_rows, _ptr(out), _ptr(chw)))
        return out, chw

    def mask_maxpool(self, x, split: bool, guard_rows: int = 8) -> np.ndarray:
        """x [n, H, W, C] -> raw [n OH OW + guard, 2 C (1 + split)]"""
        x = _f32(x)
        n, H, W, Cc = x.shape
        out = np.empty((n * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) + guard_rows, 2 * Cc * (1 + int(split))), np.uint8)
        check(self.lib.pb_op_mask_maxpool(self.ctx, _ptr(x), n, H, W, Cc, int(split), guard_rows, _ptr(out)))
        return out

    def mask_nearest_add(self, dst, src, split: bool, guard_rows: int = 8) -> np.ndarray:
        """dst [n, h, w, C] += src [n, sh, sw, C] -> raw [n h w + guard, 2 C (1 + split)]"""
        dst, src = _f32(dst), _f32(src)
        n, h, w, Cc = dst.shape
        assert src.shape[0] == n and src.shape[3] == Cc
        out = np.empty((n * h * w + guard_rows, 2 * Cc * (1 + int(split))), np.uint8)
        check(self.lib.pb_op_mask_nearest_add(self.ctx, _ptr(dst), _ptr(src), n, h, w, src.shape[1], src.shape[2], Cc, int(split), guard_rows, _ptr(out)))
        return out

    def mask_subsample2(self, x, split: bool, guard_rows: int = 8) -> np.ndarray:
        x = _f32(x)
        n, H, W, Cc = x.shape
        out = np.empty((n * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) + guard_rows, 2 * Cc * (1 + int(split))), np.uint8)
        check(self.lib.pb_op_mask_subsample2(self.ctx, _ptr(x), n, H, W, Cc, int(split), guard_rows, _ptr(out)))
        return out

    def mask_coord_concat(self, x, ldi: int, split: bool, guard_rows: int = 8) -> np.ndarray:
        """x [n, h, w, C] in rows of ldi halfs -> raw [n h w + guard, 2 (C + 64) (1 + split)]"""
        x = _f32(x)
        n, h, w, Cc = x.shape
        out = np.empty((n * h * w + guard_rows, 2 * (Cc + 64) * (1 + int(split))), np.uint8)
        check(self.lib.pb_op_mask_coord_concat(self.ctx, _ptr(x), n, h, w, Cc, ldi, int(split), guard_rows, _ptr(out)))
        return out

    def mask_bilinear(self, x, OH: int, OW: int, ldi: int, ldo: int, split: bool, y0=None, guard_rows: int = 8) -> np.ndarray:
        """x [n, H, W, C] (rows of ldi halfs) -> raw [n OH OW + guard, 2 ldo]; y0 [n, OH, OW, C]: accumulate into it"""
        x = _f32(x)
        n, H, W, Cc = x.shape
        y0 = None if y0 is None else _f32(y0)
        assert y0 is None or y0.shape == (n, OH, OW, Cc)
        out = np.empty((n * OH * OW + guard_rows, 2 * ldo), np.uint8)
        check(self.lib.pb_op_mask_bilinear(self.ctx, _ptr(x), _ptr(y0), n, H, W, OH, OW, Cc, ldi, ldo, int(split), guard_rows, _ptr(out)))
        return out

    def mask_gn_relu(self, x, gamma, beta, layout: int, guard_rows: int = 8):
        """x [n, HW, C]; layout 0 fp16 -> fp16, 1 split -> split, 2 split -> [hi | hi | lo] -> (raw [n HW + guard, 2 ldo], aff [n, C, 2])"""
        x, gamma, beta = _f32(x), _f32(gamma), _f32(beta)
        n, HW, Cc = x.shape
        assert gamma.shape == (Cc,) and beta.shape == (Cc,)
        out = np.empty((n * HW + guard_rows, 2 * Cc * (1, 2, 3)[layout]), np.uint8)
        aff = np.empty((n, Cc, 2), np.float32)
        check(self.lib.pb_op_mask_gn_relu(self.ctx, _ptr(x), _ptr(gamma), _ptr(beta), n, HW, Cc, layout, guard_rows, _ptr(out), _ptr(aff)))
        return out, aff

    def mask_cls_points_nms(self, logit, pts_total: int, off: int, guard_rows: int = 8) -> np.ndarray:
        """logit [n, g, g, C] -> raw float32 [n pts_total + guard, C] (0xFF bytes = NaN outside this level's rows)"""
        logit = _f32(logit)
        n, g, _, Cc = logit.shape
        out = np.empty((n * pts_total + guard_rows, Cc), np.float32)
        check(self.lib.pb_op_mask_cls_points_nms(self.ctx, _ptr(logit), n, pts_total, off, g, Cc, guard_rows, _ptr(out)))
        return out

    def mask_gather_rows(self, src, idx, rows_pad: int, split: bool, guard_rows: int = 8) -> np.ndarray:
        src, idx = _f32(src), self._i32(idx)
        out = np.empty((rows_pad + guard_rows, 2 * src.shape[1] * (1 + int(split))), np.uint8)
        check(self.lib.pb_op_mask_gather_rows(self.ctx, _ptr(src), src.shape[0], _ptr(idx), len(idx), rows_pad, src.shape[1], int(split), guard_rows, _ptr(out)))
        return out

    def mask_stats(self, logit, HW: int, thr: float, guard_rows: int = 1) -> np.ndarray:
        """logit [rows, ld] -> raw float32 [rows + guard, 2] = (area, soft sum)"""
        logit = _f32(logit)
        out = np.empty((logit.shape[0] + guard_rows, 2), np.float32)
        check(self.lib.pb_op_mask_stats(self.ctx, _ptr(logit), logit.shape[0], HW, logit.shape[1], thr, guard_rows, _ptr(out)))
        return out

    def mask_intersections(self, logit, idx, HW: int, thr: float, inter_rows: int, guard_rows: int = 2):
        """-> (bits uint64 [n + guard, HW / 64], inter raw float32 [inter_rows, 512])"""
        logit, idx = _f32(logit), self._i32(idx)
        bits = np.empty((len(idx) + guard_rows, HW // 64), np.uint64)
        inter = np.empty((inter_rows, 512), np.float32)
        check(self.lib.pb_op_mask_intersections(self.ctx, _ptr(logit), logit.shape[0], logit.shape[1], _ptr(idx), len(idx), HW, thr, guard_rows, _ptr(bits),
                                                inter_rows, _ptr(inter)))
        return bits, inter

    def mask_matrix_nms(self, inter, area, label, score, sigma: float, guard: int = 4):
        """inter [n, 512] (upper triangle read) -> (comp, decayed scores), raw float32 [n + guard] each"""
        inter, area, score, label = _f32(inter), _f32(area), _f32(score), self._i32(label)
        n = len(area)
        assert inter.shape == (n, 512)
        comp, out = np.empty(n + guard, np.float32), np.empty(n + guard, np.float32)
        check(self.lib.pb_op_mask_matrix_nms(self.ctx, _ptr(inter), _ptr(area), _ptr(label), _ptr(score), n, sigma, guard, _ptr(comp), _ptr(out)))
        return comp, out

    def mask_sigmoid_rows(self, logit, idx, HW: int, guard_rows: int = 1) -> np.ndarray:
        logit, idx = _f32(logit), self._i32(idx)
        out = np.empty((len(idx) + guard_rows, HW), np.float32)
        check(self.lib.pb_op_mask_sigmoid_rows(self.ctx, _ptr(logit), logit.shape[0], logit.shape[1], _ptr(idx), len(idx), HW, guard_rows, _ptr(out)))
        return out

    def mask_dynconv(self, kernels, idx, row_off: int, feat, split: bool, guard_rows: int = 2) -> np.ndarray:
        """kernels [rows, 256], idx [row_off + M], feat [HW4, 256] -> raw float32 [M + guard, HW4]: row m = <kernels[idx[row_off + m]], feat>"""
        kernels, feat, idx = _f32(kernels), _f32(feat), self._i32(idx)
        M = len(idx) - row_off
        out = np.empty((M + guard_rows, feat.shape[0]), np.float32)
        check(self.lib.pb_op_mask_dynconv(self.ctx, _ptr(kernels), kernels.shape[0], _ptr(idx), row_off, M, _ptr(feat), feat.shape[0], int(split),
                                          guard_rows, _ptr(out)))
        return out

    def mask_band_accumulate(self, sig, use, h: int, w: int, H: int, W: int, thr: float, guard: int = 64):
        """sig [k, fh, fw], use [k] -> (out raw uint8 [3 H W + guard], inst raw uint8 [k H W + guard])"""
        sig, use = _f32(sig), np.ascontiguousarray(use, np.uint8)
        k, fh, fw = sig.shape
        out = np.empty(3 * H * W + guard, np.uint8)
        inst = np.empty(k * H * W + guard, np.uint8)
        check(self.lib.pb_op_mask_band_accumulate(self.ctx, _ptr(sig), _ptr(use), k, fh, fw, h, w, H, W, thr, guard, _ptr(out), _ptr(inst)))
        return out, inst

    # ---- the depth bands' kernels one by one (pb_op_depth_*, pb_op_zoe_*; tests/test_gpu_depth_ops.py) ----
    # raw buffers as above: 0xFF wherever the kernel did not write, guard rows / elements behind the last row
    def depth_layernorm(self, x, g, b, ntok: int, drop_cls: bool, ldy: int, lo_off: int = 0, o8_off: int = 0, o8_scale: float = 1.0,
                        lo8: bool = False, guard_rows: int = 8):
        """x [B, ntp, D] -> (raw uint8 [rows + guard, 2 ldy], the engine's lo8 scale exponent); rows = B ntp, or B (ntok - 1) with drop_cls"""
        x, g, b = _f32(x), _f32(g), _f32(b)
        B, ntp, D = x.shape
        rows = B * (ntok - 1) if drop_cls else B * ntp
        out = np.empty((rows + guard_rows, 2 * ldy), np.uint8)
        pa = C.c_int(-1)
        check(self.lib.pb_op_depth_layernorm(self.ctx, _ptr(x), _ptr(g), _ptr(b), B, ntp, ntok, D, int(drop_cls), ldy, lo_off, o8_off, o8_scale,
                                             int(lo8), guard_rows, _ptr(out), C.byref(pa)))
        return out, pa.value

    def depth_attention(self, q, k, v, variant: int, ldo: int, o8_off: int = 0, o8_scale: float = 1.0, guard_rows: int = 8) -> np.ndarray:
        """q, k, v [B, heads, N, 64] -> raw uint8 [B ntp + guard, 2 ldo]; variant 1: the 8-wave kernel, 2: the 4-wave kernel"""
        q, k, v = _f32(q), _f32(k), _f32(v)
        B, Hh, N, d = q.shape
        assert d == 64 and k.shape == q.shape and v.shape == q.shape
        ntp = -(-N // 16) * 16
        out = np.empty((B * ntp + guard_rows, 2 * ldo), np.uint8)
        check(self.lib.pb_op_depth_attention(self.ctx, _ptr(q), _ptr(k), _ptr(v), B, Hh, N, variant, ldo, o8_off, o8_scale, guard_rows, _ptr(out)))
        return out

    def depth_preprocess(self, frames, metric: bool = False, guard_rows: int = 8):
        """frames uint8 [n, H, W, 3] -> (chw float32 [n, 3, nh, nw], raw uint8 [round_up(n P, 256) + guard, 1280]: the im2col rows of 640 halfs);
        one launch with both outputs, the relative band's cubic table or (metric) the align-corners table to 392 x 518"""
        frames = np.ascontiguousarray(frames, np.uint8)
        n, H, W, c = frames.shape
        assert c == 3
        nh, nw = (392, 518) if metric else net_size(H, W)
        rows = -(-(n * (nh // 14) * (nw // 14)) // 256) * 256 + guard_rows
        chw = np.empty((n, 3, nh, nw), np.float32)
        raw = np.empty((rows, 1280), np.uint8)
        check(self.lib.pb_op_depth_preprocess(self.ctx, _ptr(frames), n, H, W, int(metric), nh, nw, guard_rows, _ptr(chw), _ptr(raw)))
        return chw, raw

    def depth_cls_rows(self, cls, pos, B: int, ntp: int, guard_rows: int = 2) -> np.ndarray:
        """-> raw float32 [B ntp + guard, D]: the residual stream, preset, after cls_rows"""
        cls, pos = _f32(cls), _f32(pos)
        out = np.empty((B * ntp + guard_rows, cls.shape[0]), np.float32)
        check(self.lib.pb_op_depth_cls_rows(self.ctx, _ptr(cls), _ptr(pos), B, ntp, cls.shape[0], guard_rows, _ptr(out)))
        return out

    def depth_dpt_tail(self, z, bias, w2, b2: float, OH: int, OW: int, layout: int, ldz: int, guard: int = 64):
        """z [B, H, W, 288] -> (raw float32 [B OH OW + guard], the engine's lo8 scale exponent); layout 0 [hi], 1 [hi | lo], 2 [hi | hi8 | lo8]"""
        z, bias, w2 = _f32(z), _f32(bias), _f32(w2)
        B, H, W, Cc = z.shape
        assert Cc == 288 and bias.shape == (32,) and w2.shape == (32,)
        out = np.empty(B * OH * OW + guard, np.float32)
        pa = C.c_int(-1)
        check(self.lib.pb_op_depth_dpt_tail(self.ctx, _ptr(z), _ptr(bias), _ptr(w2), b2, B, H, W, OH, OW, layout, ldz, guard, _ptr(out), C.byref(pa)))
        return out, pa.value

    def depth_resize_minmax(self, net, H: int, W: int, guard: int = 64):
        """net [B, nh, nw] -> (raw float32 [B H W + guard], mnmx float32 [B, 2])"""
        net = _f32(net)
        B, nh, nw = net.shape
        out = np.empty(B * H * W + guard, np.float32)
        mm = np.empty((B, 2), np.float32)
        check(self.lib.pb_op_depth_resize_minmax(self.ctx, _ptr(net), B, nh, nw, H, W, guard, _ptr(out), _ptr(mm)))
        return out, mm

    def zoe_softplus(self, buf, rows: int, cols: int) -> np.ndarray:
        """buf float32 [rows + guard, ld], whole: columns [0, cols) of rows [0, rows) are replaced by their softplus"""
        buf = _f32(buf).copy()
        check(self.lib.pb_op_zoe_softplus(self.ctx, _ptr(buf), rows, cols, buf.shape[1], buf.shape[0] - rows))
        return buf

    def zoe_dot32_relu(self, act, ld: int, w2, b2: float, guard: int = 8) -> np.ndarray:
        act, w2 = _f32(act), _f32(w2)
        out = np.empty(act.shape[0] + guard, np.float32)
        check(self.lib.pb_op_zoe_dot32_relu(self.ctx, _ptr(act), ld, _ptr(w2), b2, act.shape[0], guard, _ptr(out)))
        return out

    def zoe_bilerp_add(self, a, src, lda: int, lds: int, ldo: int, guard_rows: int = 8) -> np.ndarray:
        """a [n, H, W, C] + bilinear(src [n, h, w, C], align_corners) -> raw uint8 [n H W + guard, 2 ldo]"""
        a, src = _f32(a), _f32(src)
        n, H, W, Cc = a.shape
        out = np.empty((n * H * W + guard_rows, 2 * ldo), np.uint8)
        check(self.lib.pb_op_zoe_bilerp_add(self.ctx, _ptr(a), _ptr(src), n, src.shape[1], src.shape[2], H, W, Cc, lda, lds, ldo, guard_rows, _ptr(out)))
        return out

    def zoe_attractor(self, A, nA: int, bprev, H: int, W: int, alpha: float, guard_rows: int = 2) -> np.ndarray:
        """A [n H W, ldA], bprev [n, h, w, 64] -> raw float32 [n H W + guard, 64]"""
        A, bprev = _f32(A), _f32(bprev)
        n, h, w, _ = bprev.shape
        out = np.empty((n * H * W + guard_rows, 64), np.float32)
        check(self.lib.pb_op_zoe_attractor(self.ctx, _ptr(A), A.shape[1], nA, _ptr(bprev), n, h, w, H, W, alpha, guard_rows, _ptr(out)))
        return out

    def zoe_cat(self, act, ld_act: int, rel, emb, ld_emb: int, H: int, W: int, guard_rows: int = 4) -> np.ndarray:
        """act [n H W, 32], rel [n H W], emb [n, h, w, 128] -> raw uint8 [n H W + guard, 384]"""
        act, rel, emb = _f32(act), _f32(rel), _f32(emb)
        n, h, w, _ = emb.shape
        out = np.empty((n * H * W + guard_rows, 384), np.uint8)
        check(self.lib.pb_op_zoe_cat(self.ctx, _ptr(act), ld_act, _ptr(rel), _ptr(emb), ld_emb, n, h, w, H, W, guard_rows, _ptr(out)))
        return out

    def zoe_logbinom_depth(self, pt, bins, H: int, W: int, min_temp: float = 0.0212, max_temp: float = 50.0, guard: int = 8) -> np.ndarray:
        """pt [n H W, ld_pt], bins [n, h, w, 64] -> raw float32 [n H W + guard]"""
        pt, bins = _f32(pt), _f32(bins)
        n, h, w, _ = bins.shape
        out = np.empty(n * H * W + guard, np.float32)
        check(self.lib.pb_op_zoe_logbinom_depth(self.ctx, _ptr(pt), pt.shape[1], _ptr(bins), n, h, w, H, W, min_temp, max_temp, guard, _ptr(out)))
        return out

    def zoe_pil_resize(self, x, H: int, W: int, guard: int = 8) -> np.ndarray:
        """x [n, h, w] -> raw float32 [n H W + guard]: Pillow's bicubic resize of float32 maps"""
        x = _f32(x)
        n, h, w = x.shape
        out = np.empty(n * H * W + guard, np.float32)
        check(self.lib.pb_op_zoe_pil_resize(self.ctx, _ptr(x), n, h, w, H, W, guard, _ptr(out)))
        return out

    def bilinear(self, x, OH: int, OW: int, align_corners: bool) -> np.ndarray:
        x = _f32(x)
        B, Cc, H, W = x.shape
        out = np.empty((B, Cc, OH, OW), np.float32)
        check(self.lib.pb_op_bilinear(self.ctx, _ptr(x), _ptr(out), B, Cc, H, W, OH, OW, int(align_corners)))
        return out

    def preprocess(self, frame: np.ndarray) -> np.ndarray:
        frame = np.ascontiguousarray(frame, np.uint8)
        H, W = frame.shape[:2]
        nh, nw = net_size(H, W)
        out = np.empty((3, nh, nw), np.float32)
        check(self.lib.pb_op_preprocess(self.ctx, _ptr(frame), H, W, _ptr(out), nh, nw))
        return out

    def encode_depth(self, depth, flip: bool = True):
        depth = _f32(depth)
        if depth.ndim == 2:
            depth = depth[None]
        n, H, W = depth.shape
        rgb = np.empty((n, H, W, 3), np.uint8)
        mn, mx = np.empty(n, np.float32), np.empty(n, np.float32)
        check(self.lib.pb_op_encode_depth(self.ctx, _ptr(depth), n, H, W, int(flip), _ptr(rgb), _ptr(mn), _ptr(mx)))
        return rgb, mn, mx


class DepthAnything(_Ctx):
    """Depth-Anything (DINOv2 ViT + DPT) band on one GPU.

    weights: reference state_dict naming -> float32 ndarray (bands/d_anything/dpt.py:139-171).
    """
    _stage_sym = "pb_depth_get_stage"

    def __init__(self, weights: Dict[str, np.ndarray], cfg: DepthCfg | str = "vitl", device: int = 0,
                 max_batch: int = 1, metric: bool = False, precision: Optional[int] = None):
        super().__init__()
        self.cfg = DEPTH_CFGS[cfg] if isinstance(cfg, str) else cfg
        self.metric = bool(metric)
        self.precision = _lib.default_precision() if precision is None else int(precision)
        if self.metric:      # ZoeDepth state dict: the core's tensors sit under `core.core.`
            weights = {(k[len("core.core."):] if k.startswith("core.core.") else k): v for k, v in weights.items()}
        c = _lib.pb_depth_cfg(self.cfg.embed_dim, self.cfg.depth, self.cfg.heads, self.cfg.features,
                              (C.c_int32 * 4)(*self.cfg.out_channels), self.cfg.pos_grid, max_batch, int(self.metric),
                              self.precision)
        keep: List[np.ndarray] = []
        arr = (_lib.pb_tensor * len(weights))()
        for i, (name, w) in enumerate(weights.items()):
            w = _f32(w)
            keep.append(w)
            arr[i].name = name.encode()
            arr[i].dtype = 0
            arr[i].ndim = w.ndim
            for j, s in enumerate(w.shape):
                arr[i].shape[j] = s
            arr[i].data = w.ctypes.data
        check(self.lib.pb_create(C.byref(self.ctx), device, b"depth_anything", arr, len(weights), C.byref(c),
                                 C.sizeof(c)))
        self.max_batch = max_batch

    def infer_batch(self, frames: np.ndarray, want_depth: bool = True, want_rgb: bool = True, flip: bool = True,
                    out_depth: Optional[np.ndarray] = None, out_rgb: Optional[np.ndarray] = None, size=None):
        """frames uint8 [n,H,W,3] RGB -> (depth f32 [n,H,W] | None, rgb u8 [n,H,W,3] | None, min [n], max [n]).
        out_depth / out_rgb: caller-owned result arrays (e.g. views of page-locked memory, which the library's copy engines then
        write directly - no staging copy).  frame_format / rgb_format "i420": frames [n, i420_bytes(H, W)] with size=(H, W) / rgb of that shape."""
        frames = np.ascontiguousarray(frames, np.uint8)
        n, H, W = self._frames_in(frames, size)
        depth = (out_depth if out_depth is not None else np.empty((n, H, W), np.float32)) if want_depth else None
        rgb = (out_rgb if out_rgb is not None else np.empty((n,) + self.rgb_shape(H, W), np.uint8)) if want_rgb else None
        assert depth is None or (depth.dtype == np.float32 and depth.shape == (n, H, W) and depth.flags.c_contiguous)
        assert rgb is None or (rgb.dtype == np.uint8 and rgb.shape == (n,) + self.rgb_shape(H, W) and rgb.flags.c_contiguous)
        mn, mx = np.empty(n, np.float32), np.empty(n, np.float32)
        check(self.lib.pb_depth_infer_batch(self.ctx, _ptr(frames), n, H, W, _ptr(depth), _ptr(rgb), _ptr(mn),
                                            _ptr(mx), int(flip)))
        return depth, rgb, mn, mx

    def submit_batch(self, frames: np.ndarray, out_rgb: Optional[np.ndarray] = None, out_depth: Optional[np.ndarray] = None,
                     out_min: Optional[np.ndarray] = None, out_max: Optional[np.ndarray] = None, flip: bool = True, size=None):
        """Asynchronous infer_batch (pb_depth_submit_batch): every array - `frames` and each given output - must be a C-contiguous view of
        PAGE-LOCKED memory (`host_empty()`, or torch `pin_memory()` + `.numpy()`); returns after the enqueue, `wait()` returns (depth, rgb, min, max) once they are
        filled.  Up to two submissions may be in flight per context: the second one's uploads run under the first one's kernels."""
        n, H, W = self._frames_in(frames, size)
        assert frames.dtype == np.uint8 and frames.flags.c_contiguous
        for a, dt, shp in ((out_rgb, np.uint8, (n,) + self.rgb_shape(H, W)), (out_depth, np.float32, (n, H, W)), (out_min, np.float32, (n,)), (out_max, np.float32, (n,))):
            assert a is None or (a.dtype == dt and a.shape == shp and a.flags.c_contiguous)
        check(self.lib.pb_depth_submit_batch(self.ctx, _ptr(frames), n, H, W, _ptr(out_depth), _ptr(out_rgb), _ptr(out_min), _ptr(out_max), int(flip)))
        self._hold((out_depth, out_rgb, out_min, out_max), frames, out_depth, out_rgb, out_min, out_max)

    def infer(self, img: np.ndarray, normalize: bool = False) -> np.ndarray:
        """bands/depth_anything.py:100-143 `infer(img, normalize)` for the relative model."""
        d = self.infer_batch(img[None], want_depth=True, want_rgb=False)[0][0]
        if normalize:
            lo, hi = d.min(), d.max()
            if hi - lo > np.finfo("float").eps:
                d = (d - lo) / (hi - lo)
        return d

    def infer_dev(self, frames_ptr: int, n: int, H: int, W: int, depth_ptr: int = 0, rgb_ptr: int = 0,
                  min_ptr: int = 0, max_ptr: int = 0, flip: bool = True):
        """All pointers are device addresses; asynchronous on the ctx stream (call sync())."""
        v = lambda p: C.c_void_p(p) if p else None
        check(self.lib.pb_depth_infer_batch_dev(self.ctx, v(frames_ptr), n, H, W, v(depth_ptr), v(rgb_ptr),
                                                v(min_ptr), v(max_ptr), int(flip)))


def _fwdbwd_mask(ctx: "_Ctx", flows, alpha_1: float, alpha_2: float) -> np.ndarray:
    """pb_flow_fwdbwd_mask on any context (it needs a device and a stream, no band): flows f32 [n, 2, sh, sw, 2] -> bool [n, 2, sh, sw]"""
    flows = np.ascontiguousarray(flows, np.float32)
    n, d, sh, sw, two = flows.shape
    assert d == 2 and two == 2
    mask = np.empty((n, 2, sh, sw), np.uint8)
    check(ctx.lib.pb_flow_fwdbwd_mask(ctx.ctx, _ptr(flows), n, sh, sw, C.c_float(alpha_1), C.c_float(alpha_2), _ptr(mask)))
    return mask.view(np.bool_)


def flow_out_size(H: int, W: int, scale: float) -> Tuple[int, int]:
    sh, sw = C.c_int(), C.c_int()
    check(_lib.load().pb_flow_out_size(H, W, C.c_float(scale), C.byref(sh), C.byref(sw)))
    return sh.value, sw.value


class FlowRaft(_Ctx):
    """RAFT optical-flow band on one GPU (bands/flow_raft.py:38-66 init_model / infer).

    weights: reference checkpoint naming without the `module.` prefix (fnet.*, cnet.*, update_block.*).
    """
    _stage_sym = "pb_flow_get_stage"

    BAND = b"flow_raft"

    def __init__(self, weights: Dict[str, np.ndarray], device: int = 0, precision: Optional[int] = None):
        super().__init__()
        self.precision = _lib.default_precision() if precision is None else int(precision)
        fc = _lib.pb_flow_cfg(self.precision)
        keep = {k: _f32(v) for k, v in weights.items() if np.asarray(v).dtype.kind == "f"}
        arr = (_lib.pb_tensor * len(keep))()
        for i, (name, w) in enumerate(keep.items()):
            arr[i].name = name.encode()
            arr[i].dtype = 0
            arr[i].ndim = w.ndim
            for j, s in enumerate(w.shape):
                arr[i].shape[j] = s
            arr[i].data = w.ctypes.data
        check(self.lib.pb_create(C.byref(self.ctx), device, self.BAND, arr, len(keep), C.byref(fc), C.sizeof(fc)))

    def infer_sequence(self, frames: np.ndarray, scale: float = 0.75, iters: int = 12, backward: bool = False,
                       want_flow: bool = True, want_rgb: bool = True, out_flow: Optional[np.ndarray] = None,
                       out_rgb: Optional[np.ndarray] = None, size=None):
        """frames uint8 [F,H,W,3] -> (flow f32 [F-1,dirs,sh,sw,2] | None, rgb u8 [F-1,dirs,sh,sw,3] | None, maxdisp [F-1,dirs]).
        out_flow / out_rgb: caller-owned result arrays (page-locked ones are written by the copy engines directly).
        frame_format / rgb_format "i420": frames [F, i420_bytes(H, W)] with size=(H, W) / rgb [F-1, dirs, i420_bytes(sh, sw)].
        rgb_full: the rgb frames have the clip's size - [F-1, dirs, H, W, 3] / [F-1, dirs, i420_bytes(H, W)] (also of the three calls below)."""
        frames = np.ascontiguousarray(frames, np.uint8)
        F, H, W = self._frames_in(frames, size)
        assert F >= 2
        sh, sw = flow_out_size(H, W, scale)
        d = 2 if backward else 1
        rshape = (F - 1, d) + self._flow_rgb_shape(H, W, sh, sw)
        flow = (out_flow if out_flow is not None else np.empty((F - 1, d, sh, sw, 2), np.float32)) if want_flow else None
        rgb = (out_rgb if out_rgb is not None else np.empty(rshape, np.uint8)) if want_rgb else None
        assert flow is None or (flow.dtype == np.float32 and flow.shape == (F - 1, d, sh, sw, 2) and flow.flags.c_contiguous)
        assert rgb is None or (rgb.dtype == np.uint8 and rgb.shape == rshape and rgb.flags.c_contiguous)
        mx = np.empty((F - 1, d), np.float32)
        check(self.lib.pb_flow_infer_sequence(self.ctx, _ptr(frames), F, H, W, C.c_float(scale), iters, int(backward),
                                              _ptr(flow), _ptr(rgb), _ptr(mx)))
        return flow, rgb, mx

    def submit_sequence(self, frames: np.ndarray, scale: float = 0.75, iters: int = 12, backward: bool = False,
                        out_flow: Optional[np.ndarray] = None, out_rgb: Optional[np.ndarray] = None, out_max: Optional[np.ndarray] = None, size=None):
        """Asynchronous infer_sequence (pb_flow_submit_sequence): page-locked arrays only (see DepthAnything.submit_batch); `wait()` returns
        (flow, rgb, maxdisp)."""
        F, H, W = self._frames_in(frames, size)
        assert F >= 2 and frames.dtype == np.uint8 and frames.flags.c_contiguous
        sh, sw = flow_out_size(H, W, scale)
        d = 2 if backward else 1
        for a, dt, shp in ((out_flow, np.float32, (F - 1, d, sh, sw, 2)), (out_rgb, np.uint8, (F - 1, d) + self._flow_rgb_shape(H, W, sh, sw)), (out_max, np.float32, (F - 1, d))):
            assert a is None or (a.dtype == dt and a.shape == shp and a.flags.c_contiguous)
        check(self.lib.pb_flow_submit_sequence(self.ctx, _ptr(frames), F, H, W, C.c_float(scale), iters, int(backward), _ptr(out_flow), _ptr(out_rgb), _ptr(out_max)))
        self._hold((out_flow, out_rgb, out_max), frames, out_flow, out_rgb, out_max)

    def infer_sequence_masks(self, frames: np.ndarray, scale: float = 0.75, iters: int = 12, alpha_1: float = 0.05,
                             alpha_2: float = 0.5, want_flow: bool = True, want_rgb: bool = True, out_flow: Optional[np.ndarray] = None,
                             out_rgb: Optional[np.ndarray] = None, out_mask: Optional[np.ndarray] = None, size=None):
        """Both directions plus the forward/backward consistency masks (bands/flow_raft.py:58-64):
        -> (flow | None, rgb | None, maxdisp [F-1,2], mask bool [F-1,2,sh,sw]).  The same chunked three-stage pipeline as infer_sequence;
        out_flow / out_rgb / out_mask (uint8): caller-owned result arrays, page-locked ones are written by the copy engines directly."""
        frames = np.ascontiguousarray(frames, np.uint8)
        F, H, W = self._frames_in(frames, size)
        assert F >= 2
        sh, sw = flow_out_size(H, W, scale)
        rshape = (F - 1, 2) + self._flow_rgb_shape(H, W, sh, sw)
        flow = (out_flow if out_flow is not None else np.empty((F - 1, 2, sh, sw, 2), np.float32)) if want_flow else None
        rgb = (out_rgb if out_rgb is not None else np.empty(rshape, np.uint8)) if want_rgb else None
        mx = np.empty((F - 1, 2), np.float32)
        mask = out_mask if out_mask is not None else np.empty((F - 1, 2, sh, sw), np.uint8)
        assert flow is None or (flow.dtype == np.float32 and flow.shape == (F - 1, 2, sh, sw, 2) and flow.flags.c_contiguous)
        assert rgb is None or (rgb.dtype == np.uint8 and rgb.shape == rshape and rgb.flags.c_contiguous)
        assert mask.dtype == np.uint8 and mask.shape == (F - 1, 2, sh, sw) and mask.flags.c_contiguous
        check(self.lib.pb_flow_infer_sequence_masks(self.ctx, _ptr(frames), F, H, W, C.c_float(scale), iters,
                                                    C.c_float(alpha_1), C.c_float(alpha_2), _ptr(flow), _ptr(rgb), _ptr(mx),
                                                    _ptr(mask)))
        return flow, rgb, mx, mask.view(np.bool_)

    def submit_sequence_masks(self, frames: np.ndarray, scale: float = 0.75, iters: int = 12, alpha_1: float = 0.05, alpha_2: float = 0.5,
                              out_flow: Optional[np.ndarray] = None, out_rgb: Optional[np.ndarray] = None, out_max: Optional[np.ndarray] = None,
                              out_mask: Optional[np.ndarray] = None, size=None):
        """Asynchronous infer_sequence_masks (pb_flow_submit_sequence_masks): page-locked arrays only (see DepthAnything.submit_batch;
        host_empty() gives them); out_mask (uint8 [F-1, 2, sh, sw]) is required.  `wait()` returns (flow, rgb, maxdisp, mask.view(bool))."""
        F, H, W = self._frames_in(frames, size)
        assert F >= 2 and frames.dtype == np.uint8 and frames.flags.c_contiguous
        assert out_mask is not None, "submit_sequence_masks: out_mask is required"
        sh, sw = flow_out_size(H, W, scale)
        for a, dt, shp in ((out_flow, np.float32, (F - 1, 2, sh, sw, 2)), (out_rgb, np.uint8, (F - 1, 2) + self._flow_rgb_shape(H, W, sh, sw)), (out_max, np.float32, (F - 1, 2)),
                           (out_mask, np.uint8, (F - 1, 2, sh, sw))):
            assert a is None or (a.dtype == dt and a.shape == shp and a.flags.c_contiguous)
        check(self.lib.pb_flow_submit_sequence_masks(self.ctx, _ptr(frames), F, H, W, C.c_float(scale), iters, C.c_float(alpha_1), C.c_float(alpha_2),
                                                     _ptr(out_flow), _ptr(out_rgb), _ptr(out_max), _ptr(out_mask)))
        self._hold((out_flow, out_rgb, out_max, out_mask.view(np.bool_)), frames, out_flow, out_rgb, out_max, out_mask)

    def fwdbwd_mask(self, flows: np.ndarray, alpha_1: float = 0.05, alpha_2: float = 0.5) -> np.ndarray:
        """flows f32 [n,2,sh,sw,2] (forward, backward) -> bool [n,2,sh,sw] (bands/common/flow.py:28-40)."""
        return _fwdbwd_mask(self, flows, alpha_1, alpha_2)

    def infer_sequence_dev(self, frames_ptr: int, F: int, H: int, W: int, scale: float, iters: int, backward: bool,
                           flow_ptr: int = 0, rgb_ptr: int = 0, max_ptr: int = 0):
        v = lambda p: C.c_void_p(p) if p else None
        check(self.lib.pb_flow_infer_sequence_dev(self.ctx, v(frames_ptr), F, H, W, C.c_float(scale), iters, int(backward),
                                                  v(flow_ptr), v(rgb_ptr), v(max_ptr)))

    def set_alternate_corr(self, on: bool = True):
        """--alternate_corr of the band (reference raft.py:103-106, corr.py:63-91): every lookup computes its window entries from the feature
        maps and no all-pairs correlation volume is allocated or computed.  Takes effect with the next call.  flow_raft only."""
        check(self.lib.pb_flow_set_alternate_corr(self.ctx, int(bool(on))))

    def arena_bytes(self) -> int:
        """bytes of the arena the current plan (the last call's size, pair count and mode) committed; 0 before the first call"""
        return int(check(self.lib.pb_flow_arena_bytes(self.ctx)))


class FlowGMFlow(FlowRaft):
    """GMFlow optical-flow band on one GPU (bands/flow_gmflow.py:42-118 init_model / infer; the model at the band's default flags, or - when
    the weights are a two-scale state dict - GMFlow's refinement model, see num_scales).

    weights: reference checkpoint naming (backbone.*, transformer.layers.N.*, feature_flow_attn.*, upsampler.*).  Same calls as FlowRaft
    (`iters` is ignored: GMFlow is not iterative; frames are padded to multiples of 16, of 32 with two scales).  stage(): "feat", "block0",
    "tfeat" as [frames, tokens, 128], "flow_match", "flow_prop" as [pairs * dirs, tokens, 2] (with two scales: the coarse scale's; the fine
    scale's are "feat4", "flow_up", "warp", "block0_4", "tfeat4", "flow_match4", "flow_prop4" on the 1/4 grid; there the coarse "tfeat" and
    "block0" exist only after a call under set_profiling(debug_stages=True))."""
    BAND = b"flow_gmflow"

    @property
    def num_scales(self) -> int:
        """1: the band's default model; 2: the refinement model (num_scales 2, upsample_factor 4, padding_factor 32, attn_splits_list 2 8) -
        decided by the weights (backbone.trident_conv.weight and an upsampler.2.weight of 144 rows)"""
        return int(check(self.lib.pb_flow_num_scales(self.ctx)))

    def set_inference_size(self, size=None):
        """--inference_size H W of the band (reference flow_gmflow.py:76-100): run the network on a bilinear (align_corners) resize of the
        scaled frame to (H, W), multiples of 16, and resize the flow back; None / (0, 0) = off (pad to /16, the default)."""
        h, w = (0, 0) if not size else (int(size[0]), int(size[1]))
        check(self.lib.pb_flow_set_inference_size(self.ctx, h, w))

    def set_matching(self, corr_radius: int = -1, prop_radius: int = -1):
        """--corr_radius_list R / --prop_radius_list r of the band (reference gmflow.py:128-157): -1 = global (the default); R in 1 .. 4 =
        local matching over (2 R + 1)^2 target tokens; r in 1 .. 2 = local-window propagation.  With a matching radius the backward flow is
        the forward flow of the swapped pair (the reference's pred_bidir_flow raises there).
        With two scales (num_scales == 2) these are the FINE scale's radii, the reference's --corr_radius_list -1 R --prop_radius_list -1 r:
        R in 1 .. 4, r in 1 .. 2, default (4, 1); -1 is refused (nothing global is built on the 1/4 grid) and the context stays as it was.
        The coarse scale is always global."""
        check(self.lib.pb_flow_set_matching(self.ctx, int(corr_radius), int(prop_radius)))


def _mask_cfg(cfg: MaskCfg, max_batch: int, precision: int = 0) -> "_lib.pb_mask_cfg":
    return _lib.pb_mask_cfg((C.c_int32 * 4)(*cfg.blocks), cfg.scale_long, cfg.scale_short, cfg.num_classes, cfg.feat_channels,
                            cfg.stacked_convs, (C.c_int32 * 5)(*cfg.num_grids), (C.c_int32 * 5)(*cfg.strides),
                            cfg.mask_feat_channels, cfg.mask_out_channels, cfg.nms_pre, cfg.max_per_img, cfg.score_thr,
                            cfg.mask_thr, cfg.filter_thr, cfg.sigma, max_batch, precision)


def mask_net_size(cfg: MaskCfg | str, H: int, W: int) -> Tuple[int, int, int, int]:
    """(nh, nw, Hp, Wp): keep-ratio rescale to (scale_long, scale_short), then pad to a multiple of 32."""
    cfg = MASK_CFGS[cfg] if isinstance(cfg, str) else cfg
    c = _mask_cfg(cfg, 1)
    v = [C.c_int() for _ in range(4)]
    check(_lib.load().pb_mask_net_size(C.byref(c), H, W, *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


SDF_NTAB = 4130     # squared distances 0 .. 4128 are the ones getSDF's remap does not saturate on either side; entry 4129 = saturated


def sdf_tables(n_tab: int = SDF_NTAB):
    """(tab_out, tab_in): the byte `masks[..., 1] = sdf * 255 -> astype(uint8)` of the reference's getSDF (bands/mask_mmdet.py:64-69,
    150-152) for a pixel outside / inside the mask whose squared Euclidean distance to the other side is i - evaluated with the
    reference's own float64 numpy expression, so the device only has to deliver the exact integer i."""
    d = np.sqrt(np.arange(n_tab, dtype=np.float64))
    d[-1] = 1.0e6                                            # "at least this far": saturated on both sides
    tabs = []
    for sdf in (d, -d):
        v = (sdf + 127.0) / 255.0
        v = (v - 0.25) * 2.0
        g = (1.0 - np.clip(v, 0.0, 1.0)) * 255
        tabs.append(np.ascontiguousarray(g.astype(np.uint8)))
    return tabs[0], tabs[1]


class MaskMMDet(_Ctx):
    """SOLOv2 instance-mask band on one GPU (bands/mask_mmdet.py:36-39 init_model, :131-154 per-frame body).

    weights: mmdet state_dict naming (backbone.*, neck.*, mask_head.*) -> float32 ndarray.
    """
    _stage_sym = "pb_mask_get_stage"
    _stage_cap = 1 << 27
    _stage_squeeze = False      # always 4-D

    def __init__(self, weights: Dict[str, np.ndarray], cfg: MaskCfg | str = "r101", device: int = 0, max_batch: int = 4,
                 precision: Optional[int] = None):
        super().__init__()
        self.cfg = MASK_CFGS[cfg] if isinstance(cfg, str) else cfg
        self.precision = _lib.default_precision() if precision is None else int(precision)
        c = _mask_cfg(self.cfg, max_batch, self.precision)
        keep = {k: _f32(v) for k, v in weights.items() if np.asarray(v).dtype.kind == "f"}
        arr = (_lib.pb_tensor * len(keep))()
        for i, (name, w) in enumerate(keep.items()):
            arr[i].name = name.encode()
            arr[i].dtype = 0
            arr[i].ndim = w.ndim
            for j, s in enumerate(w.shape):
                arr[i].shape[j] = s
            arr[i].data = w.ctypes.data
        check(self.lib.pb_create(C.byref(self.ctx), device, b"mask_mmdet", arr, len(keep), C.byref(c), C.sizeof(c)))
        self._hw = None

    def infer_batch(self, frames: np.ndarray, confidence: float = 0.5, keep_classes=None, out: Optional[np.ndarray] = None, size=None) -> np.ndarray:
        """frames uint8 [n,H,W,3] RGB -> uint8 [n,H,W,3] accumulated masks of the kept classes.  Calls of more than max_batch frames are
        pipelined (chunk i's id images return while chunk i + 1 runs); `out`: a caller-owned result array (a page-locked one is written by
        the copy engine directly).  frame_format / rgb_format "i420": frames [n, i420_bytes(H, W)] with size=(H, W) / id images of that shape."""
        frames = np.ascontiguousarray(frames, np.uint8)
        n, H, W = self._frames_in(frames, size)
        if out is None:
            out = np.empty((n,) + self.rgb_shape(H, W), np.uint8)
        assert out.dtype == np.uint8 and out.shape == (n,) + self.rgb_shape(H, W) and out.flags.c_contiguous
        ids = None if keep_classes is None else np.ascontiguousarray(keep_classes, np.int32)
        check(self.lib.pb_mask_infer_batch(self.ctx, _ptr(frames), n, H, W, C.c_float(confidence), _ptr(ids),
                                           0 if ids is None else len(ids), _ptr(out)))
        self._hw = (H, W)
        return out

    def set_sdf(self, on: bool = True):
        """--sdf of the band (reference mask_mmdet.py:64-69,150-152): every following infer_batch* writes the clamped signed distance
        field of the id image into its green channel, on the device.  The byte is tabulated here with the reference's float64
        expression (sdf_tables) and looked up by the exact squared distance the library computes."""
        if not on:
            check(self.lib.pb_mask_set_sdf(self.ctx, None, None, 0))
            return
        to, ti = sdf_tables()
        check(self.lib.pb_mask_set_sdf(self.ctx, _ptr(to), _ptr(ti), len(to)))

    def sdf_green(self, masks: np.ndarray) -> np.ndarray:
        """id images uint8 [n,H,W,3] -> the same with the SDF in the green channel (needs set_sdf)."""
        out = np.ascontiguousarray(masks, np.uint8).copy()
        n, H, W, ch = out.shape
        assert ch == 3
        check(self.lib.pb_mask_sdf_green(self.ctx, _ptr(out), n, H, W))
        return out

    def infer_batch_dev(self, frames_ptr: int, n: int, H: int, W: int, confidence: float, keep_classes, out_ptr: int):
        ids = None if keep_classes is None else np.ascontiguousarray(keep_classes, np.int32)
        check(self.lib.pb_mask_infer_batch_dev(self.ctx, C.c_void_p(frames_ptr), n, H, W, C.c_float(confidence), _ptr(ids),
                                               0 if ids is None else len(ids), C.c_void_p(out_ptr)))
        self._hw = (H, W)

    def instances(self, frame: int, with_masks: bool = False):
        """(scores, labels, masks bool [k,H,W] | None, candidate_count) of frame `frame` of the last call."""
        cap = self.cfg.max_per_img
        sc, lb, cand = np.empty(cap, np.float32), np.empty(cap, np.int32), C.c_int32()
        masks = None
        if with_masks:
            H, W = self._hw
            masks = np.empty((cap, H, W), np.uint8)
        k = check(self.lib.pb_mask_get_instances(self.ctx, frame, cap, _ptr(sc), _ptr(lb), _ptr(masks), C.byref(cand)))
        return sc[:k].copy(), lb[:k].copy(), (masks[:k].view(np.bool_) if with_masks else None), cand.value
