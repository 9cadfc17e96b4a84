"""CPU: the host images of the packed GEMM weights (prisma_amd/csrc/pack_layout.h - the very text every band engine packs its weights with)
built with the host clang++ of ROCm (no offload; g++ 11 has no _Float16) and held byte for byte against a numpy restatement made of
tests/split_ref.py's f16 / e4m3_bytes / weight_pw: the fp16, split-fp16 (sa with and without sw), mx2 and mx3 rows per tap, the slice-major
K order, the packed metadata, and pb_f32_to_e4m3 on every fp16 bit pattern."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import split_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "pack_layout.h"
int main(int argc, char **argv) {
    if (argv[1][0] == 'e') {            // e: the e4m3 byte of every fp16 bit pattern widened to float
        for (unsigned b = 0; b < 65536; ++b) {
            const unsigned short u = (unsigned short)b;
            f16 h;
            memcpy(&h, &u, 2);
            putchar(pb_f32_to_e4m3((float)h));
        }
        return 0;
    }
    // p N K Kpad taps sa sw mx mx2 tapin <file of N x K float32>: the metadata on stderr, the row bytes on stdout
    int a[9];
    for (int i = 0; i < 9; ++i) a[i] = atoi(argv[2 + i]);
    std::vector<float> w((size_t)a[0] * a[1]);
    FILE *f = fopen(argv[11], "rb");
    if (!f || fread(w.data(), 4, w.size(), f) != w.size()) return 2;
    fclose(f);
    PackSpec s;
    s.sa = a[4]; s.sw = a[5]; s.mx = a[6]; s.mx2 = a[7]; s.tapin = a[8];
    PackedW o;
    const std::vector<f16> rows = pack_rows(w.data(), a[0], a[1], a[2], a[3], s, o);
    fprintf(stderr, "%zu %d %d %d %d %d %d %d %d %d %d %d %d\n", rows.size(), o.N, o.K, o.Kreal, o.sa, o.sw, o.Cseg, o.mx2, o.mx3, o.mx_pw, o.nk16,
            o.tapin, o.taps);
    fwrite(rows.data(), 2, rows.size(), stdout);
    return 0;
}
"""

META = ("halfs", "N", "K", "Kreal", "sa", "sw", "Cseg", "mx2", "mx3", "mx_pw", "nk16", "tapin", "taps")


def _clangxx():
    roots = [os.environ.get("ROCM_PATH"), os.environ.get("ROCM_HOME"), "/opt/rocm"]
    hipcc = shutil.which("hipcc")
    if hipcc:
        roots.append(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))))
    for r in roots:
        p = r and os.path.join(r, "llvm", "bin", "clang++")
        if p and os.path.exists(p):
            return p
    raise RuntimeError("the host clang++ of ROCm (<rocm>/llvm/bin/clang++) was not found")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("pack_layout")
    src = d / "pack.cpp"
    src.write_text(SRC)
    out = d / "pack"
    subprocess.run([_clangxx(), "-O1", "-std=c++17", "-I", os.path.join(ROOT, "prisma_amd", "csrc"), str(src), "-o", str(out)], check=True)
    return str(out)


def run_pack(exe, tmp_path, w, Kpad, taps, sa, sw, mx, mx2, tapin):
    N, K = w.shape
    path = tmp_path / "w.f32"
    np.ascontiguousarray(w, np.float32).tofile(path)
    p = subprocess.run([exe, "p"] + [str(v) for v in (N, K, Kpad, taps, sa, sw, mx, mx2, tapin)] + [str(path)], capture_output=True, check=True)
    meta = dict(zip(META, map(int, p.stderr.split())))
    return np.frombuffer(p.stdout, np.uint8), meta


def want_rows(w, Kpad, taps, layout, sa, sw, tapin):
    """numpy restatement: per tap [w_hi | w_hi (sa) | w_lo (sw)] (f16 / split16), [w_hi | w_lo8] (mx2), [w_hi | w_lo8 | w_hi8] (mx3) with
    w_lo8 = e4m3((w - w_hi) 2^pw), w_hi8 = e4m3(w_hi 2^(pw - 12)); rows padded to a multiple of 256, every tap to Kpad / taps channels;
    slice-major: the (taps x S) grid of 128-byte blocks of every row transposed"""
    N, K = w.shape
    Cin, Cp, Np = K // taps, Kpad // taps, -(-N // 256) * 256
    w = np.asarray(w, np.float32).reshape(N, taps, Cin)
    hi = R.f16(w)
    res = w - hi                                          # exact in fp32
    pw = R.weight_pw(w, layout == R.MX3) if layout in (R.MX2, R.MX3) else 0

    def halfs(x):                                         # [N, taps, Cin] float32 -> bytes [N, taps, 2 Cp]
        o = np.zeros((N, taps, Cp), np.float16)
        o[:, :, :Cin] = x.astype(np.float16)
        return o.view(np.uint8)

    def fp8(x, p):                                        # -> bytes [N, taps, Cp]
        o = np.zeros((N, taps, Cp), np.uint8)
        o[:, :, :Cin] = R.e4m3_bytes(np.ldexp(x, p).astype(np.float32))
        return o

    if layout == R.MX3:
        segs = [halfs(hi), fp8(res, pw), fp8(hi, pw - 12)]
    elif layout == R.MX2:
        segs = [halfs(hi), fp8(res, pw)]
    else:
        segs = [halfs(hi)] + ([halfs(hi)] if sa else []) + ([halfs(res)] if sw else [])
    rows = np.concatenate(segs, axis=2).reshape(N, -1)    # [N, taps x bytes per tap]
    if tapin:
        rows = rows.reshape(N, taps, -1, 128).transpose(0, 2, 1, 3).reshape(N, -1)
    full = np.zeros((Np, rows.shape[1]), np.uint8)
    full[:N] = rows
    segw = {R.MX3: 2.0, R.MX2: 1.5}.get(layout, 1 + sa + sw)
    meta = dict(halfs=full.size // 2, N=N, K=int(taps * segw * Cp), Kreal=K, sa=0 if layout == R.MX2 else sa, sw=sw, Cseg=Cp, mx2=int(layout == R.MX2),
                mx3=int(layout == R.MX3), mx_pw=pw, nk16=Cp // 64 if layout in (R.MX2, R.MX3) else 0, tapin=tapin, taps=taps)
    return full.reshape(-1), meta


# layout -> (sa, sw, mx, mx2) of the PackSpec
SPECS = {"f16": (R.F16, 0, 0, 0, 0), "split16": (R.SPLIT16, 1, 1, 0, 0), "split16_sw": (R.SPLIT16, 0, 1, 0, 0), "split16_sa_only": (R.SPLIT16, 1, 0, 0, 0),
         "mx2": (R.MX2, 0, 1, 1, 1), "mx3": (R.MX3, 1, 1, 1, 0)}


def check(exe, tmp_path, w, Kpad, taps, name, tapin):
    layout, sa, sw, mx, mx2 = SPECS[name]
    got, gmeta = run_pack(exe, tmp_path, w, Kpad, taps, sa, sw, mx, mx2, tapin)
    want, wmeta = want_rows(w, Kpad, taps, layout, sa, sw, int(bool(tapin and taps > 1)))
    assert gmeta == wmeta
    assert got.size == want.size
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:4]}"
    return gmeta


# channels per tap: 64 (a multiple of the K tile), 24 -> 64 and 96 -> 128 (padded); mx2 needs 128 per tap, so 64 runs as 64 -> 128 there
@pytest.mark.parametrize("tapin", [0, 1])
@pytest.mark.parametrize("Cin,Cp", [(64, 64), (24, 64), (96, 128)])
@pytest.mark.parametrize("N", [8, 40])
@pytest.mark.parametrize("taps", [1, 9])
@pytest.mark.parametrize("name", list(SPECS))
def test_rows_and_metadata_equal_the_restatement(exe, tmp_path, name, taps, N, Cin, Cp, tapin):
    if name == "mx2":
        Cp = 128
    g = np.random.default_rng(1000 * taps + 10 * N + Cin + tapin)
    w = (g.standard_normal((N, taps * Cin)) * (taps * Cin) ** -0.5).astype(np.float32)
    check(exe, tmp_path, w, taps * Cp, taps, name, tapin)


@pytest.mark.parametrize("name", ["mx2", "mx3"])
def test_all_zero_weight_keeps_pw_zero(exe, tmp_path, name):
    meta = check(exe, tmp_path, np.zeros((8, 9 * 128), np.float32), 9 * 128, 9, name, 0)
    assert meta["mx_pw"] == 0
    # ... and so does a weight that is exactly fp16 (no residual): only mx3's cap by max |w| can move it
    w = R.f16(np.random.default_rng(5).standard_normal((8, 128)))
    meta = check(exe, tmp_path, w, 128, 1, name, 0)
    assert meta["mx_pw"] == (0 if name == "mx2" else min(0, 20 - R._exp(float(np.abs(w).max()))))


@pytest.mark.parametrize("name", ["mx2", "mx3"])
def test_e4m3_subnormal_residuals_and_saturating_hi8(exe, tmp_path, name):
    """one large residual sets pw; the other residuals are 2^-10 .. 2^-16 of it and land in e4m3's subnormal range (below 2^-6 after the scale) or
    at zero; and weights beyond 448 / 2^(pw - 12) (mx3 caps pw so that max |w| 2^(pw - 12) < 256 - so the cap itself is under test: without it
    hi8 would clamp)"""
    g = np.random.default_rng(77)
    w = R.f16(g.standard_normal((8, 128))).astype(np.float32)
    w[0, 0] = np.float32(1.0 + 2.0 ** -12)                       # residual 2^-12: pw = 8 - (-11) = 19, capped by max |w| for mx3
    w[1:, :] += (g.integers(-7, 8, size=(7, 128)) * 2.0 ** -22).astype(np.float32)      # residuals of a few 2^-22: < 2^-6 after 2^19
    w[2, 5] = np.float32(300.0 + 2.0 ** -5)                      # |w| 2^(19 - 12) = 38400 > 448: the cap (mx3) / nothing stored of w_hi (mx2)
    meta = check(exe, tmp_path, w, 128, 1, name, 0)
    pw = R.weight_pw(w, name == "mx3")
    assert meta["mx_pw"] == pw
    lo8 = R.e4m3_bytes(np.ldexp(w - R.f16(w), pw).astype(np.float32))
    assert ((lo8 & 0x78) == 0).any() and ((lo8 & 0x7F) != 0).any()           # subnormal codes are among the residual bytes
    if name == "mx3":
        assert pw == 20 - R._exp(float(np.abs(w).max())) and np.abs(np.ldexp(R.f16(w), pw - 12)).max() < 256


def test_f32_to_e4m3_on_every_fp16_pattern(exe):
    got = np.frombuffer(subprocess.run([exe, "e"], capture_output=True, check=True).stdout, np.uint8)
    x = np.arange(65536, dtype=np.uint16).view(np.float16).astype(np.float32)
    want = R.e4m3_bytes(x).copy()
    nan = np.isnan(x)
    want[nan] = 0x7F                                      # (np.clip passes NaN through; torch encodes it as 0x7F / 0xFF: the sign is dropped)
    assert got.size == 65536
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(hex(int(b)), hex(int(got[b])), hex(int(want[b]))) for b in bad[:8]]
    assert got[np.float16(448).view(np.uint16)] == 0x7E and got[np.float16(-60000).view(np.uint16)] == 0xFE and (got[nan] == 0x7F).all()
