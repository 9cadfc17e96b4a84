"""Frame sources / sinks of the band scripts (host side, stays Python like the reference).

Re-states the file behaviour of /root/reference/bands/common/io.py: open_rgb (:78-83),
check_overwrite (:35-41), VideoWriter (:246-305, libx264 crf 15 yuv420p), write_depth (:138-172),
write_ply (the file half of write_pcl :201-211; its arithmetic runs on the GPU, pb_depth_point_cloud).
decord / PyAV / OpenCV are optional here (absent in the build image): .mp4 needs them, .npy
frame stacks ([n,H,W,3] uint8) and .png work everywhere.

.y4m (YUV4MPEG2) is the video container that needs no library: one text header line, then `FRAME\n` + the raw I420 planes per frame.
It streams in both directions, ffmpeg / mpv / every encoder read and write it (`ffmpeg -i in.mp4 in.y4m` before a run,
`ffmpeg -i depth_anything.y4m -crf 15 depth_anything.mp4` after it), and its frames are what the engines take and give with the
"frames_i420" / "rgb_out_i420" options (include/prisma_bands.h) - half the bytes of RGB through PCIe and the page-locked rings.

A clip is read in whatever planar layout it has (Y4M_TAGS: 4:2:0, 4:2:2, 4:4:4 or mono, 8 to 16 bit, limited or full range) - `ffmpeg -i in.mov
in.y4m` does not convert pixel formats - and its planes go to the engine as they are (pb_set_frame_format).  A header does not name the matrix:
PRISMA_Y4M_MATRIX=bt601 (the default) | bt709 does; it is not guessed from the frame size.  Chroma siting is not acted on, interlaced clips,
4:1:1 and alpha layouts are refused, and so is XCOLORRANGE=FULL in a header without a `C` tag (a header that names no layout is 8-bit 4:2:0, limited).  The colour arithmetic is common/yuv.py's.

What is written is 8 bit, 4:2:0, limited range, BT.601 unless PRISMA_Y4M_OUT (process.py --y4m_out) names another layout: a `C` tag of Y4M_TAGS,
optionally followed by `,full` and / or `,bt709` (C444p12,full  Cmono,full  C422p10,bt709), or `source` for the layout of the input clip.  The
band videos carry data in their colours - depth as a hue ramp, flow as direction and length, masks as grey - and 8-bit 4:2:0 averages and
quantises it.  Properties of the two rules, checked over all 2^24 colours (tests/test_yuv_out_ref_cpu.py): a 4:4:4 video of 12, 14 or 16 bits, in
either range and matrix, returns every RGB byte the band produced - C444p12,full is the lossless choice, 6 bytes per pixel; at 10 bits up to
2.2 % of the colours come back off by 1, at 8 bits 75 - 84 % by up to 2; a grey value through Cmono,full comes back exactly - the choice for the
mask videos, one byte per pixel.  A header has no tag for the matrix: a file written with `,bt709` is read back with PRISMA_Y4M_MATRIX=bt709.

.avi / .mjpeg (Motion JPEG) is the compressed container that needs no library either: every frame a complete baseline .jpg, encoded on the GPU
(pb_jpeg_encode; there is no host encoder), an AVI 1.0 file around them or nothing at all.  PRISMA_VIDEO_OUT (process.py --video_out; common/meta.py
video_out) makes every derived band video one: `avi` or `mjpeg`, then `,q=NN` and one of `,444` `,420` `,mono`.  The frames are planes of JFIF's
colour space - 8 bit, full range, BT.601 (jpeg_format) - which the engines deliver like a .y4m layout (planar_out).  Read back with Pillow.
"""
import os
from fractions import Fraction

import numpy as np

from .meta import VIDEO_OUT_EXTS, video_out
from .resize import resize_rgb
from .yuv import I420, Format, i420_bytes, rgb_to_yuv, yuv_bytes, yuv_to_rgb

Y4M_MAGIC = b"YUV4MPEG2"
Y4M_CHROMA = ("C420", "C420jpeg", "C420mpeg2", "C420paldv")      # 8-bit 4:2:0; the siting they name is not acted on (nearest / block mean)
Y4M_DEPTHS = (9, 10, 12, 14, 16)
# every `C` tag a clip may carry -> (chroma layout, bits per sample)
Y4M_TAGS = dict([(t, (420, 8)) for t in Y4M_CHROMA] + [("C422", (422, 8)), ("C444", (444, 8)), ("Cmono", (400, 8))]
                + [("C%dp%d" % (c, d), (c, d)) for c in (420, 422, 444) for d in Y4M_DEPTHS] + [("Cmono%d" % d, (400, d)) for d in Y4M_DEPTHS])
Y4M_MATRICES = ("bt601", "bt709")


def y4m_matrix():
    """the matrix .y4m clips are decoded with: PRISMA_Y4M_MATRIX, "bt601" when unset (a header does not carry it)"""
    m = os.environ.get("PRISMA_Y4M_MATRIX", "") or "bt601"
    if m not in Y4M_MATRICES:
        raise RuntimeError("PRISMA_Y4M_MATRIX=%s: one of %s" % (m, ", ".join(Y4M_MATRICES)))
    return m


def y4m_out(source=None):
    """the layout .y4m videos are written in: PRISMA_Y4M_OUT, I420 (8 bit, 4:2:0, limited, BT.601) when unset or empty.  `TAG[,full][,bt709]`
    with TAG one of Y4M_TAGS, or `source`: the layout of the input clip (`source`: its common/yuv.py Format, None when the clip is no .y4m - then
    I420) with PRISMA_Y4M_MATRIX's matrix.  A matrix comes from this variable only: PRISMA_Y4M_MATRIX alone changes nothing that is written."""
    v = os.environ.get("PRISMA_Y4M_OUT", "")
    if not v:
        return I420
    if v == "source":
        return I420 if source is None else Format(int(source[0]), int(source[1]), bool(source[2]), y4m_matrix())
    tag, *opts = v.split(",")
    if tag not in Y4M_TAGS:
        raise RuntimeError("PRISMA_Y4M_OUT=%s: %s is not a layout that is written: `source`, or one of %s, then `,full` and / or `,bt709`"
                           % (v, tag or "(nothing)", ", ".join(Y4M_TAGS)))
    if len(set(opts)) != len(opts) or any(o not in ("full", "bt709") for o in opts):
        raise RuntimeError("PRISMA_Y4M_OUT=%s: after the layout come `,full` and / or `,bt709`, each at most once" % v)
    return Format(Y4M_TAGS[tag][0], Y4M_TAGS[tag][1], "full" in opts, "bt709" if "bt709" in opts else "bt601")


def y4m_tag(fmt):
    """the `C` tag of a layout: what ffmpeg writes for it (C420jpeg for 8-bit 4:2:0, as this writer always has)"""
    chroma, depth = int(fmt[0]), int(fmt[1])
    if (chroma, depth) not in Y4M_TAGS.values():
        raise ValueError("no .y4m tag for %r" % (tuple(fmt),))
    if chroma == 400:
        return "Cmono" if depth == 8 else "Cmono%d" % depth
    if depth == 8:
        return "C420jpeg" if chroma == 420 else "C%d" % chroma
    return "C%dp%d" % (chroma, depth)


def create_folder(path):
    os.makedirs(path, exist_ok=True)


def check_overwrite(path, assume_yes=None):
    """Reference asks interactively (io.py:35-41); PRISMA_OVERWRITE=1 or a non-tty answers yes."""
    if not path or not os.path.exists(path):
        return
    if assume_yes is None:
        assume_yes = os.environ.get("PRISMA_OVERWRITE", "") == "1" or not os.isatty(0)
    if not assume_yes and input(f"File {path} already exists. Overwrite? [y/N] ").lower() != "y":
        raise SystemExit(0)


def open_rgb(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def write_rgb(path, rgb_u8):
    from PIL import Image
    Image.fromarray(rgb_u8).save(path)


def get_image_size(path):
    """(width, height) of an image file (io.py:57-60)."""
    from PIL import Image
    with Image.open(path) as im:
        return im.size[0], im.size[1]


def get_video_data(path):
    """(width, height, fps, total_frames) of a video (io.py:63-67)."""
    v = FrameReader(path)
    if v.i420:                   # from the header and the file size: no frame is decoded
        return v.width, v.height, v.fps, len(v)
    f0 = v[0]
    return f0.shape[1], f0.shape[0], v.fps, len(v)


def is_y4m(path):
    return bool(path) and path.endswith(".y4m")


def is_mjpeg(path):
    """a Motion JPEG file of this writer: an AVI of JPEG frames, or their bare concatenation"""
    return bool(path) and path.endswith(tuple("." + e for e in VIDEO_OUT_EXTS))


def is_planar(path):
    """the file's frames are planes a VideoWriter takes as they are (write_planes) and an engine delivers (rgb_format): .y4m, .avi, .mjpeg"""
    return is_y4m(path) or is_mjpeg(path)


JPEG_CHROMAS = (444, 420, 400)


def jpeg_format(chroma=444):
    """the layout of the planes a JPEG frame is made of - JFIF's colour space: 8 bit, full range, BT.601"""
    return Format(int(chroma), 8, True, "bt601")


def planar_out(path, source=None):
    """the layout of the frames written to `path`: PRISMA_Y4M_OUT's for a .y4m (y4m_out), the JPEG planes of PRISMA_VIDEO_OUT's subsampling (4:4:4
    when it names none) for an .avi / .mjpeg, None for every other file"""
    if is_y4m(path):
        return y4m_out(source)
    if is_mjpeg(path):
        vo = video_out()
        return jpeg_format(vo.chroma if vo else 444)
    return None


def y4m_header(width, height, rate, fmt=None):
    """the header line VideoWriter writes; `rate` a Fraction, `fmt` the layout (None: 8-bit 4:2:0, limited)"""
    fmt = I420 if fmt is None else fmt
    return ("YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 %s XCOLORRANGE=%s\n" % (width, height, rate.numerator, rate.denominator, y4m_tag(fmt),
                                                                      "FULL" if fmt[2] else "LIMITED")).encode("ascii")


def as_rate(rate):
    """A frame rate as an exact Fraction: a Fraction stays (a .y4m source's num:den), a float becomes the nearest ratio a header can carry."""
    return rate if isinstance(rate, Fraction) else Fraction(rate).limit_denominator(1001000)


class Y4MFile:
    """The container side of a .y4m: header, frame index, raw planes.  .width / .height / .rate (Fraction) / .format (common/yuv.py Format: the
    layout of the `C` tag - 4:2:0, 8 bit without one -, the range of XCOLORRANGE, the matrix of PRISMA_Y4M_MATRIX) / .frame_bytes / len();
    read_i420(i, out) copies a frame's planes as they are in the file, whatever the layout."""

    def __init__(self, path):
        self.path = path
        self._fd = os.open(path, os.O_RDONLY)
        size = os.fstat(self._fd).st_size
        head = os.pread(self._fd, 4096, 0)
        end = head.find(b"\n")
        if not head.startswith(Y4M_MAGIC + b" ") or end < 0:
            raise RuntimeError("%s: not a YUV4MPEG2 file (no `YUV4MPEG2 ...` header line)" % path)
        self.width = self.height = 0
        self.rate = Fraction(24)
        layout, full, ctag, xtag = (420, 8), False, None, None
        matrix = y4m_matrix()
        try:
            for tok in head[:end].decode("ascii").split()[1:]:
                k, v = tok[0], tok[1:]
                if k == "W":
                    self.width = int(v)
                elif k == "H":
                    self.height = int(v)
                elif k == "F":
                    num, den = v.split(":")
                    self.rate = Fraction(int(num), int(den))
                elif k == "I" and tok != "Ip":
                    raise RuntimeError("%s: %s: interlaced material is not supported (progressive `Ip` only)" % (path, tok))
                elif k == "C":
                    if tok not in Y4M_TAGS:
                        raise RuntimeError("%s: %s: not a layout this reader has (%s)" % (path, tok, ", ".join(Y4M_TAGS)))
                    layout, ctag = Y4M_TAGS[tok], tok
                elif k == "X" and tok.upper().startswith("XCOLORRANGE="):
                    if tok.upper() not in ("XCOLORRANGE=LIMITED", "XCOLORRANGE=FULL"):
                        raise RuntimeError("%s: %s: XCOLORRANGE is LIMITED or FULL" % (path, tok))
                    full, xtag = tok.upper() == "XCOLORRANGE=FULL", tok
        except (ValueError, ZeroDivisionError) as e:
            raise RuntimeError("%s: malformed YUV4MPEG2 header %r" % (path, head[:end])) from e
        if self.width < 1 or self.height < 1:
            raise RuntimeError("%s: the YUV4MPEG2 header carries no W / H" % path)
        if full and ctag is None:
            # XCOLORRANGE is ffmpeg's extension, and ffmpeg always writes the `C` tag next to it: a header that names no layout is the plain
            # 8-bit 4:2:0 stream of the format's first writers, which this reader has always taken as limited range and refused otherwise
            raise RuntimeError("%s: %s without a `C` tag: a header that names no layout is read as 8-bit 4:2:0, limited range only; full range is "
                               "read from a clip whose header names its layout (%s)" % (path, xtag, ", ".join(Y4M_TAGS)))
        self.format = Format(layout[0], layout[1], full, matrix)
        self.frame_bytes = fb = yuv_bytes(self.format, self.height, self.width)
        first = end + 1
        try:
            self._index(first, size, fb)
        except RuntimeError as e:
            # the commonest cause of frames that do not fit their `C` tag: a tool relabelled the header and left 8-bit 4:2:0 planes behind it
            plain = i420_bytes(self.height, self.width)
            n, rest = divmod(size - first, 6 + plain)
            if fb != plain and n and rest == 0 and all(os.pread(self._fd, 6, first + i * (6 + plain)) == b"FRAME\n" for i in range(n)):
                raise RuntimeError("%s: %s: the header says frames of %d bytes, the file holds %d frames of %d bytes each - the size of 8-bit 4:2:0 "
                                   "frames (%s)" % (path, ctag, fb, n, plain, e)) from e
            raise

    def _index(self, first, size, fb):
        path = self.path
        # every frame line the bare `FRAME\n`: frame i is found by arithmetic (each supposed line is looked at once); otherwise one scan
        n, rest = divmod(size - first, 6 + fb)
        if rest == 0 and all(os.pread(self._fd, 6, first + i * (6 + fb)) == b"FRAME\n" for i in range(n)):
            self._first, self._offsets, self._n = first + 6, None, n
            return
        self._offsets, pos = [], first
        while pos < size:
            line = os.pread(self._fd, 4096, pos)
            nl = line.find(b"\n")
            if not line.startswith(b"FRAME") or nl < 0 or line[5:6] not in (b"\n", b" "):
                raise RuntimeError("%s: frame %d: no FRAME line at byte %d" % (path, len(self._offsets), pos))
            if pos + nl + 1 + fb > size:
                raise RuntimeError("%s: frame %d is truncated: %d of %d bytes" % (path, len(self._offsets), size - pos - nl - 1, fb))
            self._offsets.append(pos + nl + 1)
            pos += nl + 1 + fb
        self._n = len(self._offsets)

    def __len__(self):
        return self._n

    def read_i420(self, i, out):
        """The three planes of frame i into `out`, a writable C-contiguous uint8 buffer of frame_bytes bytes (a page-locked ring slot's
        row as well as a plain array).  pread: safe from the decode thread while another thread reads another frame."""
        if not 0 <= i < self._n:
            raise IndexError("%s: frame %d of %d" % (self.path, i, self._n))
        view = memoryview(out).cast("B")
        if len(view) != self.frame_bytes:
            raise ValueError("%s: read_i420 needs %d bytes, got %d" % (self.path, self.frame_bytes, len(view)))
        off = self._first + i * (6 + self.frame_bytes) if self._offsets is None else self._offsets[i]
        got = 0
        while got < self.frame_bytes:
            k = os.preadv(self._fd, [view[got:]], off + got)
            if k <= 0:
                raise RuntimeError("%s: frame %d is truncated" % (self.path, i))
            got += k
        return out

    def close(self):
        if self._fd is not None:
            os.close(self._fd)
            self._fd = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001
            pass


AVI_MAX = 2 ** 31 - 1       # an AVI 1.0 file is one RIFF chunk; readers take its 32-bit sizes and offsets as signed
AVI_MOVI = 220              # where the `movi` fourcc lies in a file of this writer: idx1 offsets count from it


def _avi_header(width, height, rate, frames=0, max_frame=0, movi_bytes=0, riff_bytes=0):
    """the 224 bytes in front of the first frame chunk: RIFF AVI, LIST hdrl (avih, LIST strl (strh vids / MJPG, strf BITMAPINFOHEADER)), LIST movi"""
    import struct
    usec = (1000000 * rate.denominator + rate.numerator // 2) // rate.numerator
    per_sec = (max_frame * rate.numerator + rate.denominator - 1) // rate.denominator
    avih = struct.pack("<14I", usec, min(per_sec, 2 ** 32 - 1), 0, 0x10, frames, 0, 1, max_frame, width, height, 0, 0, 0, 0)
    strh = struct.pack("<4s4sIHHIIIIIIII4h", b"vids", b"MJPG", 0, 0, 0, 0, rate.denominator, rate.numerator, 0, frames, max_frame, 0xFFFFFFFF, 0,
                       0, 0, width, height)
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
    chunk = lambda tag, body: tag + struct.pack("<I", len(body)) + body      # noqa: E731
    strl = b"strl" + chunk(b"strh", strh) + chunk(b"strf", strf)
    hdrl = b"hdrl" + chunk(b"avih", avih) + chunk(b"LIST", strl)
    head = b"RIFF" + struct.pack("<I", riff_bytes) + b"AVI " + chunk(b"LIST", hdrl) + b"LIST" + struct.pack("<I", 4 + movi_bytes) + b"movi"
    assert len(head) == AVI_MOVI + 4
    return head


class GpuJpegEncoder:
    """The encoder a Motion JPEG VideoWriter makes for itself: a GPU context of its own (the band's is busy, and the writer runs on the sink
    thread), pb_jpeg_encode on page-locked buffers.  encoder(planes [n, frame bytes] uint8, H, W, chroma, quality) -> the n frames' bytes, views
    that hold until the next call.  There is no host fallback: without a GPU the context cannot be made."""

    def __init__(self, device=0):
        from prisma_amd import engine
        self._engine, self._ctx, self._out = engine, engine.Ops(device=device), None

    def host_empty(self, shape, dtype):
        return self._ctx.host_empty(shape, dtype)

    def _room(self, nbytes):
        if self._out is None or self._out.size < nbytes:
            if self._out is not None:
                self._ctx.host_free(self._out)
            self._out = self._ctx.host_empty(int(nbytes), np.uint8)
        return self._out

    def __call__(self, planes, H, W, chroma, quality):
        n = len(planes)
        out = self._room(max(1 << 16, planes.size // 2))      # frames are a fraction of their planes; grown to what they need when they are not
        try:
            out, offs = self._ctx.jpeg_encode(planes, H, W, chroma, quality, out=out)
        except self._engine.JpegOverflow as e:
            out, offs = self._ctx.jpeg_encode(planes, H, W, chroma, quality, out=self._room(e.needed + e.needed // 4))
        return [out[offs[i]:offs[i + 1]] for i in range(n)]

    def close(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = self._out = None


def _jpeg_end(buf, pos):
    """the position behind the EOI of the JPEG frame that starts at buf[pos] (SOI): its segments walked by their lengths, its entropy-coded data
    scanned for a marker that is neither a stuffed 0xFF nor RSTm - SOI / EOI byte pairs inside a segment's payload are not looked at"""
    if buf[pos:pos + 2] != b"\xff\xd8":
        raise RuntimeError("no JPEG frame (SOI) at byte %d" % pos)
    pos += 2
    while True:
        if pos + 2 > len(buf) or buf[pos] != 0xFF:
            raise RuntimeError("broken JPEG frame: no marker at byte %d" % pos)
        m = buf[pos + 1]
        if m == 0xD9:
            return pos + 2
        if pos + 4 > len(buf):
            raise RuntimeError("broken JPEG frame: it ends inside the segment at byte %d" % pos)
        pos += 2 + int.from_bytes(buf[pos + 2:pos + 4], "big")
        if m != 0xDA:
            continue
        while True:                     # entropy-coded data
            pos = buf.find(b"\xff", pos)
            if pos < 0 or pos + 1 >= len(buf):
                raise RuntimeError("broken JPEG frame: the entropy-coded data does not end")
            if buf[pos + 1] == 0x00 or 0xD0 <= buf[pos + 1] <= 0xD7:
                pos += 2
                continue
            break                       # a marker: EOI, or another segment (a further scan)


class MjpegFile:
    """The container side of an .avi (AVI 1.0 with an `MJPG` video stream and an idx1 index - what VideoWriter writes; anything else is refused by
    name) or a bare .mjpeg stream: .width / .height / .rate (Fraction; None for a bare stream, which carries none) / len() / frame(i) -> the
    JPEG's bytes."""

    def __init__(self, path):
        import mmap
        import struct
        self.path, self.rate = path, None
        self._f = open(path, "rb")
        self._buf = mmap.mmap(self._f.fileno(), 0, access=mmap.ACCESS_READ) if os.fstat(self._f.fileno()).st_size else b""
        buf = self._buf
        self._spans = []
        if path.endswith(".avi"):
            if buf[:4] != b"RIFF" or buf[8:12] != b"AVI ":
                raise RuntimeError("%s: not an AVI file (no `RIFF ... AVI ` header)" % path)
            chunks, movi = {}, None

            def walk(lo, hi):
                nonlocal movi
                while lo + 8 <= hi:
                    tag, size = bytes(buf[lo:lo + 4]), struct.unpack("<I", buf[lo + 4:lo + 8])[0]
                    if tag == b"LIST":
                        kind = bytes(buf[lo + 8:lo + 12])
                        if kind == b"movi":
                            movi = lo + 8
                        else:
                            walk(lo + 12, lo + 8 + size)
                    else:
                        chunks.setdefault(tag, (lo + 8, size))
                    lo += 8 + size + (size & 1)
            walk(12, len(buf))
            if b"RIFF" in chunks or b"indx" in chunks:
                raise RuntimeError("%s: an OpenDML AVI (AVIX / indx) - this reader has AVI 1.0 with an idx1 index only" % path)
            if movi is None or b"strh" not in chunks or b"strf" not in chunks or b"idx1" not in chunks:
                raise RuntimeError("%s: an AVI without a movi list, a stream header or an idx1 index - this reader has AVI 1.0 MJPG files with idx1 only" % path)
            sh, sf = chunks[b"strh"][0], chunks[b"strf"][0]
            kind, codec = bytes(buf[sh:sh + 4]), bytes(buf[sf + 16:sf + 20])
            if kind != b"vids" or codec.upper() != b"MJPG":
                raise RuntimeError("%s: the first stream is %r / %r - this reader decodes Motion JPEG (`vids` / `MJPG`) only" % (path, kind, codec))
            scale, rate = struct.unpack("<II", buf[sh + 20:sh + 28])
            self.rate = Fraction(rate, scale) if rate and scale else None
            self.width, self.height = struct.unpack("<ii", buf[sf + 4:sf + 12])
            at, size = chunks[b"idx1"]
            for k in range(size // 16):
                tag, _flags, off, ln = struct.unpack("<4sIII", buf[at + 16 * k:at + 16 * k + 16])
                if tag != b"00dc":
                    continue
                if bytes(buf[movi + off:movi + off + 4]) != b"00dc" or struct.unpack("<I", buf[movi + off + 4:movi + off + 8])[0] != ln:
                    raise RuntimeError("%s: idx1 entry %d does not point at a `00dc` chunk of its size (offsets count from the movi list)" % (path, k))
                self._spans.append((movi + off + 8, ln))
        else:
            pos = 0
            while pos < len(buf):
                try:
                    end = _jpeg_end(buf, pos)
                except RuntimeError as e:
                    raise RuntimeError("%s: frame %d: %s" % (path, len(self._spans), e)) from e
                self._spans.append((pos, end - pos))
                pos = end
            if self._spans:
                from PIL import Image
                import io as _io
                with Image.open(_io.BytesIO(self.frame(0))) as im:
                    self.width, self.height = im.size
            else:
                self.width = self.height = 0

    def __len__(self):
        return len(self._spans)

    def frame(self, i):
        at, ln = self._spans[i]
        return bytes(self._buf[at:at + ln])

    def decode(self, i):
        """frame i as uint8 [H, W, 3] RGB: Pillow's decode of the frame's bytes"""
        import io as _io
        from PIL import Image
        with Image.open(_io.BytesIO(self.frame(i))) as im:
            return np.asarray(im.convert("RGB"))

    def close(self):
        if self._f is not None:
            if self._buf:
                self._buf.close()
            self._f.close()
            self._f = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001
            pass


class FrameReader:
    """len() / [i] -> uint8 HxWx3 RGB; fps.  decord for .mp4 (reference), numpy memmap for .npy, Y4MFile for .y4m, MjpegFile for .avi /
    .mjpeg (Motion JPEG as VideoWriter writes it, decoded with Pillow on the host).
    .rate is what a VideoWriter of the band's output takes: the exact Fraction of a .y4m source, else fps.
    .i420: the source holds planar YUV frames (.y4m) - then .width / .height are known without a decode, .format is their layout (common/yuv.py
    Format; I420 for the usual clip) and .frame_bytes their size, read_i420(i, out) copies frame i's planes as they are into the caller's
    buffer of frame_bytes bytes, and [i] converts them on the host (common/yuv.py), whatever the layout."""

    def __init__(self, path):
        self.fps = 24.0
        self.i420 = False
        if is_y4m(path):
            self._y4m = Y4MFile(path)
            self.i420, self.width, self.height = True, self._y4m.width, self._y4m.height
            self.format, self.frame_bytes = self._y4m.format, self._y4m.frame_bytes
            self.fps = self._y4m.rate.numerator / self._y4m.rate.denominator
            self.read_i420 = self._y4m.read_i420
            self._n = len(self._y4m)
            self._get = lambda i: yuv_to_rgb(self.format, self._y4m.read_i420(i, np.empty(self.frame_bytes, np.uint8)), self.height, self.width)
        elif is_mjpeg(path):
            self._mj = MjpegFile(path)
            self._n, self._get = len(self._mj), self._mj.decode
            if self._mj.rate is not None:
                self.fps = self._mj.rate.numerator / self._mj.rate.denominator
        elif path.endswith(".npy"):
            self._a = np.load(path, mmap_mode="r")
            assert self._a.ndim == 4 and self._a.shape[-1] == 3 and self._a.dtype == np.uint8
            self._get = lambda i: np.asarray(self._a[i])
            self._n = self._a.shape[0]
        else:
            try:
                import decord
            except ImportError as e:
                raise RuntimeError("reading .mp4 needs decord (reference dependency); use a .npy frame stack here") from e
            self._v = decord.VideoReader(path)
            self.fps = self._v.get_avg_fps()
            self._get = lambda i: self._v[i].asnumpy()
            self._n = len(self._v)

    @property
    def rate(self):
        mj = getattr(self, "_mj", None)
        if mj is not None and mj.rate is not None:
            return mj.rate
        return self._y4m.rate if self.i420 else self.fps

    def __len__(self):
        return self._n

    def __getitem__(self, i):
        return self._get(i)


class VideoWriter:
    """write(uint8 HxWx3) / close().  .mp4 -> PyAV libx264 crf 15 (io.py:246-305); .npy -> frame stack; .y4m -> planar YUV frames of
    layout `fmt` (common/yuv.py Format; None: I420) appended to the file as they come (nothing is kept in memory), the header written with the
    first frame and that frame's own size (no rescale, as the .npy writer), write_planes(planes, h, w) for frames that already are in that
    layout (the engines' rgb_format results; write_i420 is the same for an I420 writer).
    rescale=True (a .y4m writer's; the flow bands pass it, whose frames are `--scale` times the clip's): the video has the width and height
    the writer was opened with, as the reference's has (io.py:297 rescales every frame to them).  write() resizes a frame of another size
    on the host (common/resize.py: bilinear with two taps, where PyAV's reformat runs swscale's), write_i420 takes frames of that size only.

    .avi / .mjpeg -> Motion JPEG: baseline JPEG frames of `quality` (None: PRISMA_VIDEO_OUT's, 90 without one) made of planes of layout `fmt`
    (None: planar_out's - 4:4:4 unless PRISMA_VIDEO_OUT says otherwise; always 8 bit, full range, BT.601: JFIF's colour space), which write_planes
    takes as a .y4m writer does and write() converts to; rescale as above.  Frames are gathered `group` at a time and encoded in one call of
    `encoder(planes [n, bytes], H, W, chroma, quality) -> n byte strings` - by default a GpuJpegEncoder on `device`, made with the first frame;
    there is no host fallback (tests pass tests/jpeg_ref.py's).  .avi is AVI 1.0: RIFF AVI, hdrl (avih, one strl: vids / MJPG, dwRate / dwScale the
    exact rate, BITMAPINFOHEADER), movi of `00dc` chunks padded to even, idx1; frames are appended as they come, 16 index bytes per frame are kept
    and the counts and sizes patched into the headers by close().  The file is one RIFF: a frame that would take it past 2 GiB raises (OpenDML is
    not written); the frames of its group that were not yet written are dropped with it, and close() still leaves a valid file of what fits.  .mjpeg is the bare concatenation of the frames, of any length (`ffmpeg -framerate R -i x.mjpeg`)."""

    def __init__(self, width, height, frame_rate, filename, rescale=False, fmt=None, quality=None, encoder=None, group=8, device=0):
        self.filename, self._frames, self._av, self._y4m, self._mj = filename, None, None, None, None
        self.i420 = is_y4m(filename)
        if is_mjpeg(filename):
            vo = video_out()
            self.format = planar_out(filename) if fmt is None else Format(*fmt)
            self.quality = int(quality if quality is not None else (vo.quality if vo else 90))
            if self.format != jpeg_format(self.format[0]) or self.format[0] not in JPEG_CHROMAS or not 1 <= self.quality <= 100:
                raise ValueError("%s: a JPEG frame is made of 8-bit full-range BT.601 planes, 4:4:4, 4:2:0 or mono, at quality 1 .. 100 - not %r at %r"
                                 % (filename, tuple(self.format), self.quality))
            self._rate, self._size, self._rescale = as_rate(frame_rate), (int(height), int(width)) if rescale else None, bool(rescale)
            self._encoder, self._own_encoder, self._device, self._group, self._held, self._buf = encoder, False, device, max(1, int(group)), 0, None
            self._avi, self._index, self._count, self._max_frame = filename.endswith(".avi"), bytearray(), 0, 0
            self._mj = open(filename, "wb")
            return
        self.format = I420 if fmt is None else Format(*fmt)
        yuv_bytes(self.format, 1, 1)        # an unknown layout is refused here
        if self.i420:
            # rescale: the size is the writer's, not the first frame's
            self._rate, self._size, self._rescale, self._started = as_rate(frame_rate), (int(height), int(width)) if rescale else None, bool(rescale), False
            self._y4m = open(filename, "wb")
        elif filename.endswith(".npy"):
            self._frames = []
        else:
            try:
                import av
            except ImportError as e:
                raise RuntimeError("writing .mp4 needs PyAV (reference dependency); write a .npy stack here") from e
            # reference io.py:262-289: sides clamped to 3840 keeping the aspect, made even; rate as '%.2f' (29.97 stays 29.97, so the
            # band videos stay frame-aligned with rgba.mp4); libx264 crf 15, frame threading AUTO
            max_size = 3840
            if width > max_size or height > max_size:
                aspect = height / width
                width, height = (max_size, round(max_size * aspect)) if aspect < 1 else (round(max_size / aspect), max_size)
            self._av = av.open(filename, mode="w")
            self._st = self._av.add_stream("libx264", rate="%.2f" % frame_rate, options={"crf": "15"})
            self._w, self._h = 2 * round(width / 2), 2 * round(height / 2)
            self._st.width, self._st.height, self._st.pix_fmt = self._w, self._h, "yuv420p"
            self._st.thread_type = "AUTO"

    def write_i420(self, yuv, height, width):
        """one I420 frame (uint8, i420_bytes(height, width) bytes: Y, Cb, Cr planes) of a .y4m whose layout is I420"""
        if self._y4m is None:
            raise RuntimeError("%s: write_i420 is a .y4m writer's" % self.filename)
        if self.format != I420:
            raise RuntimeError("%s: write_i420 on a writer of %r (write_planes takes its frames)" % (self.filename, tuple(self.format)))
        self.write_planes(yuv, height, width)

    def write_planes(self, yuv, height, width):
        """one frame of the writer's layout (uint8, yuv_bytes(format, height, width) bytes: the Y plane, then Cb and Cr if the layout has them)"""
        if self._mj is not None:
            return self._mj_planes(yuv, height, width)
        if self._y4m is None:
            raise RuntimeError("%s: write_planes is a .y4m writer's" % self.filename)
        if self._size is None:
            self._size = (height, width)
        if not self._started:       # the header goes out with the first frame
            self._started = True
            self._y4m.write(y4m_header(self._size[1], self._size[0], self._rate, self.format))
        yuv = np.ascontiguousarray(yuv, np.uint8).reshape(-1)
        if (height, width) != self._size or yuv.size != yuv_bytes(self.format, height, width):
            raise ValueError("%s: a %d x %d frame of %d bytes in a %d x %d video" % ((self.filename, height, width, yuv.size) + self._size))
        self._y4m.write(b"FRAME\n")
        self._y4m.write(memoryview(yuv))
        self._y4m.flush()

    # ---- Motion JPEG ----
    def _tell(self):
        return self._mj.tell()

    def _mj_planes(self, yuv, height, width):
        if self._size is None:
            self._size = (height, width)
        fb = yuv_bytes(self.format, height, width)
        yuv = np.asarray(yuv, np.uint8).reshape(-1)
        if (height, width) != self._size or yuv.size != fb:
            raise ValueError("%s: a %d x %d frame of %d bytes in a %d x %d video" % ((self.filename, height, width, yuv.size) + self._size))
        if self._buf is None:           # the first frame: the encoder (a GPU context of the writer's own) and the group's buffer, page-locked if it can be
            if self._encoder is None:
                self._encoder, self._own_encoder = GpuJpegEncoder(self._device), True
            alloc = getattr(self._encoder, "host_empty", np.empty)
            self._buf = alloc((self._group, fb), np.uint8)
            if self._avi:
                self._mj.write(_avi_header(width, height, self._rate))
        self._buf[self._held] = yuv
        self._held += 1
        if self._held == self._group:
            self._mj_flush()

    def _mj_flush(self):
        if not self._held:
            return
        h, w = self._size
        frames = self._encoder(self._buf[:self._held], h, w, self.format[0], self.quality)
        self._held = 0
        for f in frames:
            f = memoryview(f).cast("B")
            n = len(f)
            if self._avi:
                at = self._tell()
                # the chunk, its pad byte, the index with this frame's entry: what the file would end as
                if at + 8 + n + (n & 1) + 8 + len(self._index) + 16 > AVI_MAX:
                    raise RuntimeError("%s: frame %d would take the file past 2 GiB, the limit of an AVI 1.0 file (one RIFF chunk; OpenDML is not "
                                       "written): write `.mjpeg` (PRISMA_VIDEO_OUT=mjpeg: a bare stream of any length) or lower the quality (,q=NN)"
                                       % (self.filename, self._count))
                self._index += b"00dc" + (0x10).to_bytes(4, "little") + (at - AVI_MOVI).to_bytes(4, "little") + n.to_bytes(4, "little")
                self._mj.write(b"00dc" + n.to_bytes(4, "little"))
            self._mj.write(f)
            if self._avi and n & 1:
                self._mj.write(b"\0")
            self._count += 1
            self._max_frame = max(self._max_frame, n)
        self._mj.flush()

    def _mj_close(self):
        try:
            self._mj_flush()
            if self._avi:
                if self._buf is None:       # no frame was written: an empty video of the writer's size, if it has one
                    h, w = self._size or (0, 0)
                    self._mj.write(_avi_header(w, h, self._rate))
                end = self._tell()
                self._mj.write(b"idx1" + len(self._index).to_bytes(4, "little") + bytes(self._index))
                total = self._tell()
                h, w = self._size or (0, 0)
                self._mj.seek(0)
                self._mj.write(_avi_header(w, h, self._rate, self._count, self._max_frame, end - (AVI_MOVI + 4), total - 8))
        finally:
            self._mj.close()
            if self._own_encoder:
                self._encoder.close()

    def write(self, rgb):
        if self._y4m is not None or self._mj is not None:
            if self._rescale and tuple(rgb.shape[:2]) != self._size:
                rgb = resize_rgb(rgb, *self._size)
            self.write_planes(rgb_to_yuv(self.format, np.asarray(rgb, np.uint8)), rgb.shape[0], rgb.shape[1])
            return
        if self._frames is not None:
            self._frames.append(np.array(rgb))      # a copy, always: the caller's frame may be a view of a ring slot that a later chunk overwrites
            return
        import av
        frame = av.VideoFrame.from_ndarray(np.ascontiguousarray(rgb, np.uint8), format="rgb24")
        for pkt in self._st.encode(frame.reformat(width=self._w, height=self._h)):     # io.py:297: frames may be scaled
            self._av.mux(pkt)

    def close(self):
        if self._mj is not None:
            self._mj_close()
            return
        if self._y4m is not None:
            self._y4m.close()
            return
        if self._frames is not None:
            np.save(self.filename, np.stack(self._frames) if self._frames else np.zeros((0, 0, 0, 3), np.uint8))
            return
        for pkt in self._st.encode():
            self._av.mux(pkt)
        self._av.close()


def _sobel_mag_u8(img_u8):
    """cv2.Sobel(img, CV_64F, 1, 0, ksize=1) / (0, 1): central differences, reflect-101 border.
    PARITY UNPINNED (third-party opencv-python absent); call site encode.py:81-95."""
    a = img_u8.astype(np.float64)
    p = np.pad(a, 1, mode="reflect")
    gx = p[1:-1, 2:] - p[1:-1, :-2]
    gy = p[2:, 1:-1] - p[:-2, 1:-1]
    return np.sqrt(gx * gx + gy * gy)


def float_to_rgb(value, min_value=0.0, max_value=1.0, base=256):
    """encode.py:141-146: 24-bit fixed point of a scalar in three channels."""
    L = np.clip((value - min_value) / (max_value - min_value), 0.0, 1.0) * (base ** 3 - 1)
    return (np.floor(L % base) / (base - 1), np.floor(L / base) % base / (base - 1),
            np.floor(L / (base * base)) % base / (base - 1))


def write_depth(path, depth, heat_rgb_fn, normalize=True, flip=False, heatmap=True, encode_range=True):
    """Still-image encode (io.py:138-172): heat ramp, Sobel edge in the saturation, min/max packed in
    pixels (0,0) and (0,1).  heat_rgb_fn(float64 HxW in 0..1) -> float64 HxWx3 (the band's ramp)."""
    dmin, dmax = depth.min(), depth.max()
    if normalize:
        depth = (depth - dmin) / (dmax - dmin)
    if flip:
        depth = 1.0 - depth
    if not heatmap:
        from PIL import Image
        Image.fromarray((depth * 65535).astype("uint16")).save(path)
        return
    mag = _sobel_mag_u8((depth * 255).astype(np.uint8))
    edge = mag * (255.0 / mag.max()) / 255.0 if mag.max() > 0 else mag
    rgb = heat_rgb_fn(depth.astype(np.float64))
    sat = (1.0 - edge)[..., None]
    rgb = rgb * sat + (1.0 - sat)
    if encode_range:
        rgb[0, 0] = float_to_rgb(dmin, 0.0, 1000.0)
        rgb[0, 1] = float_to_rgb(dmax, 0.0, 1000.0)
    write_rgb(path, (rgb * 255).astype(np.uint8))


def write_ply(path, vertices):
    """Binary PLY of one `vertex` element (geom.py:27-47 save_point_cloud): the header plyfile writes for the structured dtype
    (x, y, z '<f4'; red, green, blue 'u1'), then the packed 15-byte records.  PARITY UNPINNED (third-party plyfile absent): the header
    is restated from the PLY format, not compared with a file the real package wrote."""
    vertices = np.ascontiguousarray(vertices).reshape(-1)
    names = {"<f4": "float", "|u1": "uchar"}
    props = ["property %s %s" % (names[vertices.dtype[n].str], n) for n in vertices.dtype.names]
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % vertices.size] + props + ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(vertices.tobytes())


def write_flo(path, flow):
    """Middlebury .flo (io.py:175-197): float32 magic 202021.25, int32 width, int32 height, float32 HxWx2."""
    flow = np.ascontiguousarray(flow, np.float32)
    with open(path, "wb") as f:
        np.array([202021.25], np.float32).tofile(f)
        np.array([flow.shape[1], flow.shape[0]], np.int32).tofile(f)
        flow.tofile(f)


def encode_flow(flow, mask):
    """encode.py:105-110: 8.8 fixed point around 2^15 in uint16, validity in the third channel."""
    q = np.float32(2 ** 15) + flow.astype(np.float32) * np.float32(2 ** 8)
    ok = mask.astype(bool) & (q.max(axis=-1) < (2 ** 16 - 1)) & (0 < q.min(axis=-1))
    return np.concatenate([q.astype(np.uint16), ok[..., None].astype(np.uint16) * (2 ** 16 - 1)], axis=-1)


def write_png16(path, img_u16):
    """16-bit RGB PNG, channel order as given (PIL cannot write this mode; cv2 is absent)."""
    import struct
    import zlib
    a = np.ascontiguousarray(img_u16, np.uint16)
    h, w, c = a.shape
    assert c == 3
    raw = np.concatenate([np.zeros((h, 1), np.uint8), a.astype(">u2").view(np.uint8).reshape(h, w * 6)], axis=1).tobytes()

    def chunk(tag, payload):
        return struct.pack(">I", len(payload)) + tag + payload + struct.pack(">I", zlib.crc32(tag + payload) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def write_flow_png(path, flow, mask):
    """cv2.imwrite(path, encode_flow(flow, mask)) (common/flow.py:96-99): OpenCV stores the array as B, G, R, so
    the file's R channel is the validity mask, G is v and B is u."""
    write_png16(path, encode_flow(flow, mask)[..., ::-1])
