// Where an entry of the flow_raft band's correlation volume sits, as plain C++ so that the same text runs in the kernels (volume.hip stores,
// raft_kernels.hip corr_lookup_blocked_kernel loads), in the host code that de-blocks a level and - compiled by g++ - in
// tests/test_corr_layout_cpu.py.  Test infrastructure includes this file; it includes nothing.
//
// One level of one pair-direction holds P source rows of `pld` entries (halfs), pld a multiple of 64: T = pld / 64 target tiles of 8 x 8
// (corr_tile_kernel), entry e = (y & 7) * 8 + (x & 7) of tile j = (y >> 3) * (wp >> 3) + (x >> 3).
//   CORR_ROWMAJOR  [p][j][e]                      a source row is pld contiguous halfs
//   CORR_BLOCKED   [p >> 3][j][p & 7][e]          the eight rows' copies of a target tile are 1 KB contiguous; P is rounded up to 8 rows
// Neighbouring source pixels look up nearly the same target tiles (flow is coherent), so the blocked lookup reads 1 KB runs where the
// row-major one reads 128-byte lines pld * 2 bytes apart.
#pragma once
#if defined(__HIPCC__)
#define PB_CL __device__ __host__ __forceinline__
#else
#define PB_CL inline
#endif

enum { CORR_ROWMAJOR = 0, CORR_BLOCKED = 1 };

// source rows a pair-direction's level is carved for: a block of 8 never straddles two pair-directions
PB_CL long long corr_layout_rows(int layout, int P) { return layout == CORR_BLOCKED ? ((long long)P + 7) / 8 * 8 : P; }

// first half of the 8 rows x 64 entries that block (p >> 3) keeps of tile j
PB_CL long long corr_blocked_tile(int pblk, int j, int T) { return ((long long)pblk * T + j) * 512; }

// offset in halfs of entry c (= j * 64 + e) of source row p inside its pair-direction's level
PB_CL long long corr_layout_index(int layout, int p, int c, int pld) {
    if (layout != CORR_BLOCKED) return (long long)p * pld + c;
    return corr_blocked_tile(p >> 3, c >> 6, pld >> 6) + (p & 7) * 64 + (c & 63);
}
