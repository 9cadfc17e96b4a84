// Host-compilable pieces of the flow engines (no HIP types, so tests/test_flow_chunk_cpu.py builds them with the host compiler and checks them
// against brute-force loops): the padded geometry of a call, and how many frame pairs a host-pointer flow call sends to FlowEngine::infer at
// once (abi.hip flow_host_pipeline).
#pragma once
#include <math.h>
#include <stdint.h>

// --scale as the reference computes with it.  The C ABI carries the scale as a float, the reference hands Python's double to
// cv2.resize(fx = fy = scale): for a dyadic scale (0.75, 0.5, 1) the two are one number, for 0.6 or 0.7 the widened float is 2.4e-8 off, which
// moves the scaled size at some clip sizes (H x 0.7 on a half-even tie) and 8-bit tap coefficients at many.  Returned: the double of the
// shortest decimal m x 10^-k (m of 1 .. 9 digits) that rounds back to the float - the literal the caller typed, for anything of up to 7
// significant digits (a longer literal gets the shortest decimal of its float, not itself); a dyadic scale is returned unchanged.  Sizes
// (flow_geometry) and tap tables (flow_engine.hip) are computed from this value.  Plain arithmetic, no text and so no locale: m < 2^53 and
// 10^|k| <= 10^22 are exact doubles, so the one division (or product) that forms m x 10^-k is correctly rounded - the double strtod would give.
// Outside 1e-13 .. 1e13 (and for NaN) the widened float is returned.
static inline double flow_scale_exact(float scale) {
    const double v = (double)scale;
    if (!(v >= 1e-13 && v <= 1e13)) return v;
    const int e10 = (int)floor(log10(v));
    for (int digits = 1; digits <= 9; ++digits) {
        const int k = digits - 1 - e10;                  // decimal places: |k| <= 22
        double p = 1.0;
        for (int i = 0; i < (k < 0 ? -k : k); ++i) p *= 10.0;
        const double m = nearbyint(k >= 0 ? v * p : v / p);
        const double d = k >= 0 ? m / p : m * p;
        if ((float)d == scale) return d;
    }
    return v;
}

// The sizes a flow call works on: the scaled frame sh x sw (cv2.resize(fx = fy = scale): round-half-even of the product), padded as
// InputPadder('sintel', padding_factor = factor) pads it (bands/common/flow.py:43-55: up to the next multiple of `factor`, the smaller half of the
// padding on the left / top) to Hp x Wp, and the 1/8 grid h8 x w8 of P tokens.  factor: 8 (RAFT), 16 (GMFlow), 32 (two-scale GMFlow).
struct FlowGeometry { int sh, sw, Hp, Wp, padl, padt, h8, w8, P; };
static inline FlowGeometry flow_geometry(int H, int W, float scale, int factor) {
    FlowGeometry g;
    const double s = flow_scale_exact(scale);
    g.sh = (int)nearbyint((double)H * s);
    g.sw = (int)nearbyint((double)W * s);
    const int ph = (((g.sh / factor) + 1) * factor - g.sh) % factor, pw = (((g.sw / factor) + 1) * factor - g.sw) % factor;
    g.padl = pw / 2; g.padt = ph / 2;
    g.Hp = g.sh + ph; g.Wp = g.sw + pw;
    g.h8 = g.Hp / 8; g.w8 = g.Wp / 8; g.P = g.h8 * g.w8;
    return g;
}

// The hoisted GRU share (raft_engine.hip) addresses its lo plane as an `int` offset of rows * Lhx halfs, rows = pairs * dirs * P update-block
// rows of a call: infer() refuses a call with rows * Lhx >= 2^31.  Returns the largest cp <= wanted with cp * dirs * P * Lhx < 2^31, or 0 when
// not even one pair fits (the engine then refuses the call with its own message).  P: pixels of the 1/8 grid, Lhx: halfs per row of hx_.
static inline int flow_chunk_pairs(int wanted, int dirs, int64_t P, int64_t Lhx) {
    if (wanted <= 0 || dirs <= 0 || P <= 0 || Lhx <= 0) return 0;
    const int64_t per_pair = (int64_t)dirs * P * Lhx;
    const int64_t fit = ((INT64_C(1) << 31) - 1) / per_pair;      // cp * per_pair <= 2^31 - 1
    return (int)(fit < wanted ? fit : wanted);
}
