"""The C ABI's additions for the streamed band loops: pb_flow_submit_sequence_masks, pb_host_alloc, pb_host_free.  CPU: the prototypes parse and
the ctypes signatures carry the header's argument counts.  GPU: page-locked blocks owned by a context (engine._Ctx.host_empty / host_free)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from prisma_amd import _lib

NEW = {"pb_flow_submit_sequence_masks": 13, "pb_host_alloc": 3, "pb_host_free": 2}


def _prototypes():
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "prisma_bands.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    return {m.group(2): (m.group(1).strip(), [a.strip() for a in m.group(3).split(",")])
            for m in re.finditer(r"\b((?:const\s+)?[A-Za-z_0-9]+\s*\*?)\s*\b(pb_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)}


def test_new_prototypes_parse_and_match_the_binding():
    protos = _prototypes()
    for name, nargs in NEW.items():
        ret, args = protos[name]
        assert ret == "int" and len(args) == nargs, (name, ret, args)
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is C.c_int and len(argtypes) == nargs
    # the asynchronous form takes exactly what its blocking twin takes
    assert [a.split()[:-1] for a in protos["pb_flow_submit_sequence_masks"][1]] == [a.split()[:-1] for a in protos["pb_flow_infer_sequence_masks"][1]]
    assert _lib.SYMBOLS["pb_flow_submit_sequence_masks"][1] == _lib.SYMBOLS["pb_flow_infer_sequence_masks"][1]
    assert "pb_mask_submit_batch" not in protos and "pb_mask_submit_batch" not in _lib.SYMBOLS         # on purpose: see the header
    assert _lib.ABI_VERSION == 3


def test_every_binding_has_the_headers_argument_count():
    protos = _prototypes()
    for name, (_, argtypes) in _lib.SYMBOLS.items():
        args = protos[name][1]
        n = 0 if args in ([""], ["void"]) else len(args)
        assert n == len(argtypes), (name, args, argtypes)


@pytest.fixture(scope="module")
def depth():
    from prisma_amd import engine, synth
    net = engine.DepthAnything(synth.depth_anything_weights("vits", seed=1234), "vits", device=0, max_batch=2)
    yield net
    net.close()


@pytest.mark.gpu
def test_host_blocks_are_page_locked_and_round_trip(depth):
    from prisma_amd import synth
    frames = synth.frames(2, 96, 128, seed=3)
    ref_depth, ref_rgb, ref_mn, ref_mx = depth.infer_batch(frames)
    with pytest.raises(RuntimeError, match="page-locked"):                     # pageable memory is what submit refuses ...
        depth.submit_batch(frames, out_rgb=np.empty((2, 96, 128, 3), np.uint8))
    fr = depth.host_empty(frames.shape, np.uint8)
    out = {"rgb": depth.host_empty((2, 96, 128, 3), np.uint8), "depth": depth.host_empty((2, 96, 128), np.float32),
           "mn": depth.host_empty(2, np.float32), "mx": depth.host_empty((2,), np.float32)}
    assert fr.flags.c_contiguous and fr.flags.writeable and fr.shape == frames.shape and fr.dtype == np.uint8
    assert depth.host_bytes() == fr.nbytes + sum(a.nbytes for a in out.values())
    fr[...] = frames
    assert np.array_equal(fr, frames)                                          # contents round-trip
    depth.submit_batch(fr, out_rgb=out["rgb"], out_depth=out["depth"], out_min=out["mn"], out_max=out["mx"])      # ... and these are accepted
    d, rgb, mn, mx = depth.wait()
    assert d is out["depth"] and np.array_equal(d, ref_depth) and np.array_equal(rgb, ref_rgb)
    assert np.array_equal(mn, ref_mn) and np.array_equal(mx, ref_mx)
    for a in [fr] + list(out.values()):
        depth.host_free(a)
    assert depth.host_bytes() == 0


@pytest.mark.gpu
def test_foreign_pointer_is_refused(depth):
    from prisma_amd import engine
    mine = depth.host_empty(64, np.uint8)
    with pytest.raises(RuntimeError) as ei:
        depth.host_free(np.empty(64, np.uint8))                                # not a block of any context
    assert "not a block" in str(ei.value)
    assert depth.lib.pb_host_free(depth.ctx, C.c_void_p(np.empty(8, np.uint8).ctypes.data)) == -1      # PB_ERR_ARG
    other = engine.Ops(device=0)
    try:
        assert other.lib.pb_host_free(other.ctx, C.c_void_p(mine.ctypes.data)) == -1                   # another context's block
        assert depth.lib.pb_host_free(depth.ctx, C.c_void_p(mine.ctypes.data + 8)) == -1               # the middle of one's own
    finally:
        other.close()
    mine[...] = 7                                                              # still alive after the refusals
    depth.host_free(mine)
    with pytest.raises(RuntimeError):
        depth.host_free(mine)                                                  # twice: the context no longer owns it


@pytest.mark.gpu
def test_close_with_live_blocks_and_a_submission_in_flight():
    from prisma_amd import engine, synth
    net = engine.DepthAnything(synth.depth_anything_weights("vits", seed=1234), "vits", device=0, max_batch=2)
    fr = net.host_empty((2, 96, 128, 3), np.uint8)
    rgb = net.host_empty((2, 96, 128, 3), np.uint8)
    spare = net.host_empty((3, 5), np.float32)
    fr[...] = synth.frames(2, 96, 128, seed=3)
    net.submit_batch(fr, out_rgb=rgb)
    net.close()                                                                # waits for the submission, then frees the three blocks
    assert not net.ctx and net.host_bytes() == 0 and not spare.flags.writeable and not fr.flags.writeable
    net.close()                                                                # idempotent
