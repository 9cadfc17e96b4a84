"""The band scripts' chunk loop, once (SURVEY 8 e, 8 f-4): decode of chunk i+1 and the encode / file writes of chunk i-1 overlap the engine's
work on chunk i (common/pipe.py), every rank works through its contiguous shard, rank 0 muxes the output as the chunks finish and only the
per-unit scalars go through a collective (prisma_amd/shard.py).  `chunks` is the decode side alone (rgba's split uses it without a GPU);
`run_sharded` is the whole loop of depth_anything, mask_mmdet and the two flow bands.  The engine call is one argument, `step`: the streamed
entry points (submit_* / wait on page-locked rings) replace the blocking calls here, in one place."""
import numpy as np

from .pipe import AsyncSink, prefetch


def chunks(src, first, last, chunk, halo=0):
    """(start, frames) for start in range(first, last, chunk): frames = src[start : min(last, start + chunk) + halo] as one array, read up to two
    chunks ahead on one worker thread.  halo = 1 for pairs: chunk k's last frame is chunk k+1's first."""
    load = lambda s: np.stack([src[i] for i in range(s, min(last, s + chunk) + halo)])      # noqa: E731
    return prefetch(load, range(first, last, chunk))


def run_sharded(rk, src, n_units, chunk, halo, out_path, est_bytes, step, write_chunk, dump=None, n_scalars=0, ctx=None):
    """This rank's shard of `n_units` units (frames; pairs with halo = 1) of `src`, `chunk` units per engine call.

    step(start, frames) -> (video_chunk, dump_payload, scalar_rows)   main thread: the engine call.  video_chunk is {name: array}, what
                                                                       travels to rank 0; scalar_rows is [units, n_scalars] (None with n_scalars = 0)
    write_chunk(start, video_chunk)                                    rank 0 only, chunks in unit order: from the sink thread for its own
                                                                       chunks, from the relay's drain for the other ranks'
    dump(start, dump_payload)                                          every rank, sink thread: the per-unit files

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

    sink = AsyncSink(depth=2)
    for s, frames in chunks(src, first, last, chunk, halo):
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
