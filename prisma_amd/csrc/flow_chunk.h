// How many frame pairs a host-pointer flow call sends to RaftEngine::infer at once (abi.hip flow_host_pipeline).  Host-compilable: no HIP
// types, so tests/test_flow_chunk_cpu.py builds it with the host compiler and checks it against a brute-force loop.
#pragma once
#include <stdint.h>

// The hoisted GRU share (raft_engine.hip) addresses its lo plane as an `int` offset of rows * Lhx halfs, rows = pairs * dirs * P update-block
// rows of a call: infer() refuses a call with rows * Lhx >= 2^31.  Returns the largest cp <= wanted with cp * dirs * P * Lhx < 2^31, or 0 when
// not even one pair fits (the engine then refuses the call with its own message).  P: pixels of the 1/8 grid, Lhx: halfs per row of hx_.
static inline int flow_chunk_pairs(int wanted, int dirs, int64_t P, int64_t Lhx) {
    if (wanted <= 0 || dirs <= 0 || P <= 0 || Lhx <= 0) return 0;
    const int64_t per_pair = (int64_t)dirs * P * Lhx;
    const int64_t fit = ((INT64_C(1) << 31) - 1) / per_pair;      // cp * per_pair <= 2^31 - 1
    return (int)(fit < wanted ? fit : wanted);
}
