"""The band scripts' chunk loop, once (SURVEY 8 e, 8 f-4): decode of chunk i+1 and the encode / file writes of chunk i-1 overlap the engine's
work on chunk i (common/pipe.py), every rank works through its contiguous shard, rank 0 muxes the output as the chunks finish and only the
per-unit scalars go through a collective (prisma_amd/shard.py).  `chunks` is the decode side alone (rgba's split uses it without a GPU);
`run_sharded` is the whole loop of depth_anything, mask_mmdet and the two flow bands.

The engine call comes in two forms.  `step` is one blocking call per chunk on arrays the loop stacks (pageable: the library stages every
copy, in series with the kernels).  `stream=Stream(...)` is the streamed schedule: the decode thread writes the frames straight into a
ring of page-locked slots, the main thread submits chunk k + 1 before it waits for chunk k (the library's submit_* / wait, two submissions
in flight: one's copies run under the other's kernels), and the results land in a second ring whose slots the sink thread gives back when
the chunk has been written.  Both forms hand the same bytes to `write_chunk` and `dump`.

A source of planar YUV frames (a .y4m: FrameReader.i420) is read without a conversion: `i420=True` makes a frame its packed planes, in whatever
layout the clip has (FrameReader.format, .frame_bytes) - read_i420 straight into the stacked array or the ring slot - for an engine whose
frame_format is that layout (frame_formats)."""
import collections
import os
import queue
import sys
import threading
import time

import numpy as np

from .pipe import AsyncSink, prefetch

# slots of the streamed loop's two rings: decode may run this many chunks ahead of the engine, the sink this many behind it (two of each are in
# flight in the engine).  A slot is one chunk (+ halo) of frames / one chunk of every result array: DESIGN.md section 6 has the footprint.
RING_IN, RING_OUT = 4, 4
MAX_IN_FLIGHT = 2       # submissions outstanding per context: the library's limit (include/prisma_bands.h, pb_wait)
last_stream = {}        # what the last streamed loop of this process did: submissions, slots, ring_bytes (tools/band_loop_bench.py reads it)


def ring_slots():
    """(input slots, output slots): RING_IN / RING_OUT, or PRISMA_RING_SLOTS = "n" | "in,out" (tests: slot reuse within a few chunks).  Never
    fewer than the submissions in flight, each of which holds one slot of either ring."""
    v = os.environ.get("PRISMA_RING_SLOTS", "")
    if not v:
        return RING_IN, RING_OUT
    p = [int(x) for x in v.split(",")]
    return max(MAX_IN_FLIGHT, p[0]), max(MAX_IN_FLIGHT, p[-1])


def stream_enabled(min_chunks, n_chunks):
    """Which loop a band runs.  PRISMA_STREAM=1 / 0: the streamed / the blocking one, whatever the clip.  Unset: streamed when this rank's shard
    has at least `min_chunks` chunks (0: never) - page-locking and releasing the rings costs a fixed 0.2 - 0.4 s that a shard has to be long
    enough to win back; a band's `min_chunks` is the shortest clip its streamed loop was measured not slower on (EXPERIMENTS.md 6.19)."""
    v = os.environ.get("PRISMA_STREAM", "")
    if v != "":
        return v != "0"
    return bool(min_chunks) and n_chunks >= min_chunks


class Stream:
    """What a band gives run_sharded(stream=...) for the streamed schedule.

    host                       .host_empty(shape, dtype) / .host_free(array): page-locked memory (an engine context: pb_host_alloc), and .wait()
    frame                      (shape, dtype) of one decoded frame
    results                    {name: (shape of one unit, dtype)}: one array per result the band asked for, the per-unit scalars included
    submit(start, frames, res) main thread: enqueue the engine call.  frames = the leading m (+ halo) frames of an input slot, res = {name:
                               the leading m units of that array of an output slot} - contiguous page-locked views also for a short last chunk.
                               A band whose engine call is blocking (mask) makes that call here and passes wait = a no-op.
    collect(start, res)        main thread, after the wait: -> (video_chunk, dump_payload, scalar_rows) as `step` returns them, views of res
    wait()                     blocks until the OLDEST submission has its results in `res` (default: host.wait)

    Nothing a band keeps past the return of write_chunk / dump may be a view of `res`: the slot is overwritten by a later chunk."""

    def __init__(self, host, frame, results, submit, collect, wait=None, i420=False):
        self.host, self.frame, self.results, self.submit, self.collect = host, frame, dict(results), submit, collect
        self.i420 = i420            # frame = ((src.frame_bytes,), uint8): the decode thread fills a slot's rows with src.read_i420
        self.wait = wait if wait is not None else host.wait


def frame_formats(model, yin, yout, h, w, layout=None, out_layout=None):
    """Tells a band's engine what the loop will hand it (`yin`: the source is a .y4m, its frames are planes of `layout`, the reader's .format -
    I420 without one) and wants back (`yout`: the output is a .y4m, its frames planes of `out_layout`, io.y4m_out()'s - I420 without one -, or an
    .avi / .mjpeg, whose JPEG frames are made of the planes io.planar_out() names):
    engine.frame_format / rgb_format.  -> the extra keyword arguments of the
    engine's calls: the frame size, which plane arrays do not carry.  With neither, nothing is touched and nothing is passed: the calls are what
    they were before .y4m."""
    if not (yin or yout) and getattr(model, "frame_format", "rgb") == "rgb" and getattr(model, "rgb_format", "rgb") == "rgb":
        return {}
    named = lambda f: "i420" if f is None or tuple(f) == (420, 8, False, "bt601") else tuple(f)      # noqa: E731
    model.frame_format, model.rgb_format = named(layout) if yin else "rgb", named(out_layout) if yout else "rgb"
    return {"size": (h, w)} if yin or yout else {}


def i420_bytes(h, w):
    return h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)


def chunks(src, first, last, chunk, halo=0, i420=False):
    """(start, frames) for start in range(first, last, chunk): frames = src[start : min(last, start + chunk) + halo] as one array, read up to two
    chunks ahead on one worker thread.  halo = 1 for pairs: chunk k's last frame is chunk k+1's first.  i420: [frames, src.frame_bytes] planes."""
    def load_i420(s):
        a = np.empty((min(last, s + chunk) + halo - s, getattr(src, "frame_bytes", None) or i420_bytes(src.height, src.width)), np.uint8)
        for j in range(len(a)):
            src.read_i420(s + j, a[j])
        return a
    load = lambda s: np.stack([src[i] for i in range(s, min(last, s + chunk) + halo)])      # noqa: E731
    return prefetch(load_i420 if i420 else load, range(first, last, chunk))


def _run_streamed(src, first, last, chunk, halo, st, emit, n_scalars):
    """The streamed schedule over this rank's units [first, last): -> the scalar rows (copies).  On every exit, error or not: the decode thread
    has stopped, every outstanding submission has been waited for (the copy engines write ring memory), the sink is closed, and only then
    are the rings freed; the first exception is the one raised."""
    n_in, n_out = ring_slots()
    fshape, fdtype = st.frame
    starts = list(range(first, last, chunk))
    cap = min(chunk, max(0, last - first))  # units of a slot: a shard shorter than a chunk holds no more than itself
    rings, free_in, free_out, ready = [], queue.Queue(), queue.Queue(), queue.Queue()
    in_flight = collections.deque()         # (start, input slot, output slot, m) of the submissions not yet waited for, oldest first
    stop = threading.Event()
    sink = AsyncSink(depth=n_out)           # the output ring is the back-pressure: a job in this queue holds a slot
    rows, err, n_sub, decoder = [], None, 0, None
    made, t_alloc = {"in": 0, "out": 0}, [0.0, 0.0]        # slots allocated so far; seconds spent page-locking them on the decode / the main thread

    def alloc(shape, dtype, who):
        t0 = time.perf_counter()
        a = st.host.host_empty(shape, dtype)
        t_alloc[who] += time.perf_counter() - t0
        rings.append(a)
        return a

    # A slot is page-locked when it is first needed, by the thread that needs it (an input slot by the decode thread, an output slot by the
    # main thread): locking pages costs about a quarter of a second per GB, which up front is exposed and this way runs under the engine's
    # work on the chunks before - all but the first slot of each ring - and a short clip never locks slots it does not get to use.
    def fresh(q, kind, make):
        try:
            return q.get_nowait()
        except queue.Empty:
            if made[kind] < (n_in if kind == "in" else n_out):
                made[kind] += 1
                return make()
        return None

    def new_in():
        return alloc((cap + halo,) + tuple(fshape), fdtype, 0)

    def new_out():
        return {k: alloc((cap,) + tuple(shp), dt, 1) for k, (shp, dt) in st.results.items()}

    def decode():                           # decode thread: frame by frame straight into a free slot, no np.stack
        try:
            for s in starts:
                slot = fresh(free_in, "in", new_in)
                while slot is None:         # blocks while no slot is free
                    if stop.is_set():
                        return
                    try:
                        slot = free_in.get(timeout=0.05)
                    except queue.Empty:
                        pass
                m = min(last, s + chunk) - s
                for j in range(m + halo):
                    if st.i420:
                        src.read_i420(s + j, slot[j])
                    else:
                        slot[j] = src[s + j]
                ready.put((s, slot, m, None))
        except BaseException as e:          # noqa: BLE001 - handed to the main thread
            ready.put((None, None, 0, e))

    def take(q):                            # a blocking get that notices a failed sink (its skipped jobs never give their slots back)
        while True:
            try:
                return q.get(timeout=0.05)
            except queue.Empty:
                if sink.failed:
                    sink.close()

    def written(s, oslot, video, payload):  # sink thread: the slot is free again only when emit has returned
        try:
            emit(s, video, payload)
        finally:
            free_out.put(oslot)

    def retire():                           # the oldest submission: wait, release its input slot, hand its results to the sink
        s, islot, oslot, m = in_flight.popleft()      # (a wait that fails has consumed the submission all the same)
        st.wait()
        free_in.put(islot)
        video, payload, scalars = st.collect(s, {k: v[:m] for k, v in oslot.items()})
        if n_scalars:
            rows.append(np.array(scalars, np.float32).reshape(m, n_scalars))       # a copy: `scalars` may be a view of the slot
        sink.submit(written, s, oslot, video, payload)

    try:
        decoder = threading.Thread(target=decode, name="band-decode", daemon=True)
        decoder.start()
        for _ in starts:
            if len(in_flight) == MAX_IN_FLIGHT:     # chunk k - 1 is waited for only now: chunk k went in before
                retire()
            oslot = fresh(free_out, "out", new_out)      # (a new one is locked while the decode thread fills the chunk's frames)
            s, islot, m, e = take(ready)
            if e is not None:
                raise e
            if oslot is None:
                oslot = take(free_out)
            st.submit(s, islot[:m + halo], {k: v[:m] for k, v in oslot.items()})       # (one that fails has drained what it enqueued)
            in_flight.append((s, islot, oslot, m))
            n_sub += 1
        while in_flight:
            retire()
    except BaseException as e:              # noqa: BLE001 - re-raised below, after the clean-up
        err = e
    stop.set()
    if decoder is not None:
        decoder.join()                      # it may be in the middle of a slot
    for _ in range(len(in_flight)):         # nothing may still be in flight when ring memory goes away
        try:
            st.wait()
        except BaseException as e:          # noqa: BLE001
            err = err or e
    try:
        sink.close()
    except BaseException as e:              # noqa: BLE001
        err = err or e
    held, t0 = sum(a.nbytes for a in rings), time.perf_counter()
    for a in rings:
        try:
            st.host.host_free(a)
        except BaseException as e:          # noqa: BLE001
            err = err or e
    if err is not None:
        raise err
    last_stream.update(submissions=n_sub, slots=(n_in, n_out), used=(made["in"], made["out"]), ring_bytes=held, lock_s=tuple(t_alloc),
                       free_s=time.perf_counter() - t0)
    if os.environ.get("PRISMA_STREAM_LOG", "") not in ("", "0"):      # opt-in: the one line that says which loop ran
        print("[loop] streamed: %d submissions, rings %d in / %d out, %d bytes page-locked" % (n_sub, n_in, n_out, held), file=sys.stderr)
    return rows


def run_sharded(rk, src, n_units, chunk, halo, out_path, est_bytes, step, write_chunk, dump=None, n_scalars=0, ctx=None, stream=None, i420=False):
    """This rank's shard of `n_units` units (frames; pairs with halo = 1) of `src`, `chunk` units per engine call.

    step(start, frames) -> (video_chunk, dump_payload, scalar_rows)   main thread: the engine call.  video_chunk is {name: array}, what
                                                                       travels to rank 0; scalar_rows is [units, n_scalars] (None with n_scalars = 0)
    write_chunk(start, video_chunk)                                    rank 0 only, chunks in unit order: from the sink thread for its own
                                                                       chunks, from the relay's drain for the other ranks'
    dump(start, dump_payload)                                          every rank, sink thread: the per-unit files
    stream                                                             a Stream: the streamed schedule instead of `step` (which is then unused)
    i420                                                               the blocking loop's frames are src's I420 planes (chunks(i420=True))

    `out_path` and `est_bytes` (what the other ranks may park in the spool) are shard.Relay's; `ctx` is rk.gather's.  n_scalars is an argument
    because a rank with an empty shard has to know whether to join the gather.  Returns the float32 [n_units, n_scalars] rows of every rank in
    unit order on rank 0, None on the other ranks and without scalars."""
    from prisma_amd import shard      # here, not at the top: rgba takes `chunks` from this module and runs without the package
    first, last = rk.frames(n_units)
    relay = shard.Relay(rk, out_path, est_bytes=est_bytes)
    rows = []

    def emit(s, video, payload):      # sink thread, chunk after chunk in order
        if rk.main:
            write_chunk(s, video)
        else:
            relay.put(s, video)
        if dump:
            dump(s, payload)

    if stream is not None:
        rows = _run_streamed(src, first, last, chunk, halo, stream, emit, n_scalars)
        rows = np.concatenate(rows) if rows else []
    else:
        sink = AsyncSink(depth=2)
        for s, frames in chunks(src, first, last, chunk, halo, i420=i420):
            video, payload, scalars = step(s, frames)
            sink.submit(emit, s, video, payload)
            if n_scalars:
                rows += list(scalars)
        sink.close()
    rows = np.asarray(rows, np.float32).reshape(-1, n_scalars) if n_scalars else None
    if rk.world > 1:
        # scalars first (every rank gets here when its own compute is done), then rank 0 muxes the other ranks' chunks while they
        # wait on a file signal in relay.close() - no collective is pending during the mux
        # (with a bounded spool, PRISMA_SPOOL_MAX_CHUNKS, the drain has to run DURING the gather: Relay.drain_begin)
        if rk.main:
            relay.drain_begin(n_units, chunk, write_chunk)
        if n_scalars:
            rows = rk.gather(rows, n_units, ctx=ctx)
        if rk.main:
            relay.drain_end()
    relay.close()
    return rows if rk.main else None
