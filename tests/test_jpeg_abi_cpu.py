"""CPU: the JPEG entry points are in the header, the binding and the built library, pb_jpeg_cfg is struct 7 of an ABI that is still version 3, and
pb_jpeg_bound - which needs no GPU - is no smaller than what the rule (tests/jpeg_ref.py) produces on its worst input here."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as entry  # noqa: E402
import jpeg_ref as J  # noqa: E402
import yuv_out_ref as O  # noqa: E402
from prisma_amd import _lib  # noqa: E402

NAMES = ("pb_jpeg_bound", "pb_jpeg_encode", "pb_jpeg_encode_dev")


@pytest.fixture(scope="module")
def lib():
    entry.build()
    return _lib.load()


def test_entry_points_everywhere(lib):
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "prisma_bands.h")).read()
    declared = set(re.findall(r"\b(pb_[a-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "typedef struct pb_jpeg_cfg" in hdr
    assert lib.pb_abi_version() == 3 == _lib.ABI_VERSION
    assert lib.pb_struct_size(7) == C.sizeof(_lib.pb_jpeg_cfg) == 8 and lib.pb_struct_size(8) == -1
    from prisma_amd import engine
    assert callable(engine._Ctx.jpeg_encode) and callable(engine._Ctx.jpeg_encode_dev) and callable(engine.jpeg_bound)


def test_bound_refusals(lib):
    from prisma_amd import engine
    assert lib.pb_jpeg_bound(None, 8, 8) == 0
    for chroma, q, h, w in ((422, 90, 8, 8), (444, 0, 8, 8), (444, 101, 8, 8), (444, 90, 0, 8), (444, 90, 8, 65536), (0, 90, 8, 8)):
        assert engine.jpeg_bound(chroma, q, h, w) == 0
    assert engine.jpeg_bound(400, 1, 1, 1) > 0 and engine.jpeg_bound(420, 100, 65535, 16) > 0


@pytest.mark.parametrize("chroma", J.CHROMAS)
def test_bound_holds_on_noise_at_quality_100(chroma):
    from prisma_amd import engine
    for (H, W) in ((83, 101), (17, 33), (1, 1), (8, 8)):
        rgb = np.random.default_rng(H * 1000 + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
        n = len(J.encode(O.rgb_to_yuv((chroma, 8, True, "bt601"), rgb), H, W, chroma, 100))
        assert engine.jpeg_bound(chroma, 100, H, W) >= n
    # and it is what the header says: the header segments, 2 x 208 bytes per block, the markers
    rows, cols = J.mcu_grid(chroma, 83, 101)
    blocks = rows * cols * {444: 3, 420: 6, 400: 1}[chroma]
    assert engine.jpeg_bound(chroma, 100, 83, 101) == len(J.header(83, 101, chroma, 100)) + 416 * blocks + 2 * (rows - 1) + 2
