// Host-compilable pieces of the flow engines (no HIP types, so tests/test_flow_chunk_cpu.py builds them with the host compiler and checks them
// against brute-force loops): the padded geometry of a call, and how many frame pairs a host-pointer flow call sends to FlowEngine::infer at
// once (abi.hip flow_host_pipeline).
#pragma once
#include <math.h>
#include <stdint.h>

// The sizes a flow call works on: the scaled frame sh x sw (cv2.resize(fx = fy = scale): round-half-even of the product), padded as
// InputPadder('sintel', padding_factor = factor) pads it (bands/common/flow.py:43-55: up to the next multiple of `factor`, the smaller half of the
// padding on the left / top) to Hp x Wp, and the 1/8 grid h8 x w8 of P tokens.  factor: 8 (RAFT), 16 (GMFlow), 32 (two-scale GMFlow).
struct FlowGeometry { int sh, sw, Hp, Wp, padl, padt, h8, w8, P; };
static inline FlowGeometry flow_geometry(int H, int W, float scale, int factor) {
    FlowGeometry g;
    g.sh = (int)nearbyint((double)H * scale);
    g.sw = (int)nearbyint((double)W * scale);
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
