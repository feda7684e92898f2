// svs_index.hpp - the integer index arithmetic of the kernels: which tile a workgroup owns, where a block's pixels
// live, and where its payload bits sit in the stream.  Plain C++ (host and device): csrc/svs_device.hpp calls it with
// blockIdx / gridDim, csrc/svs_capi.hip fills the divisors, tests/hostemu exports every function to the CPU tier
// (tests/test_index_arithmetic_cpu.py holds each against Python integers).  The payload readers that go with it
// (payload_window, payload_qword, window32) stand in svs_block.hpp.
#pragma once
#include <stdint.h>

#include "svs_order.hpp"

#ifndef SVS_HD
#if defined(__HIPCC__)
#define SVS_HD __host__ __device__ __forceinline__
#else
#define SVS_HD inline
#endif
#endif

namespace svs {

// ---------------------------------------------------------------------------------------
// geometry shared by all kernels; division by W/8 and by blocks-per-frame is done with
// host-computed multipliers (exact for dividends < 2^31)
// ---------------------------------------------------------------------------------------
struct FastDiv {
    uint32_t mul;
    uint32_t shift;  // 31..62
    uint32_t div;
    uint32_t pad;
};

struct Geometry {
    FastDiv by_wb;          // divide by blocks per block-row
    FastDiv by_bpf;         // divide by blocks per frame
    uint32_t total_blocks;  // n_frames * blocks per frame   (< 2^31)
    uint32_t n_ac;          // 1..63
    uint32_t xcd_chunk;     // tile_id() chunk (0 = identity)
    uint32_t pad;           // embed launches: the rule (svs_block.hpp rule_word): 0, 1 = SVS_NEAREST, else SVS_MINMOVE and the bits of h
    int64_t row_pitch;
    int64_t frame_pitch;
};

// host side (1 <= d < 2^31): q = (n * mul) >> shift is exact for n < 2^31:  shift = 31 + ceil(log2 d),
// mul = ceil(2^shift / d) <= 2^31
inline FastDiv make_div(uint32_t d) {
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;
    FastDiv r;
    r.shift = 31 + l;
    r.mul = (uint32_t)(((1ull << r.shift) + d - 1) / d);
    r.div = d;
    r.pad = 0;
    return r;
}

SVS_HD uint32_t fast_div(uint32_t n, const FastDiv &d) {
    return (uint32_t)(((uint64_t)n * d.mul) >> d.shift);
}

// byte offset of the top-left pixel of global block `gblock` (frames in order, raster inside); col_bytes = bytes of one
// block's row (8 gray, 24 interleaved BGR)
SVS_HD int64_t block_offset_at(uint32_t gblock, const FastDiv &by_wb, const FastDiv &by_bpf, int64_t row_pitch,
                               int64_t frame_pitch, uint32_t col_bytes) {
    const uint32_t frame = fast_div(gblock, by_bpf);
    const uint32_t in_frame = gblock - frame * by_bpf.div;
    const uint32_t brow = fast_div(in_frame, by_wb);
    const uint32_t bcol = in_frame - brow * by_wb.div;
    return (int64_t)frame * frame_pitch + (int64_t)(brow * 8u) * row_pitch + (int64_t)(bcol * col_bytes);
}

SVS_HD int64_t block_offset(uint32_t gblock, const Geometry &g) {
    return block_offset_at(gblock, g.by_wb, g.by_bpf, g.row_pitch, g.frame_pitch, 8u);
}

SVS_HD int64_t block_offset_bgr(uint32_t gblock, const Geometry &g, int64_t row_pitch, int64_t frame_pitch) {
    return block_offset_at(gblock, g.by_wb, g.by_bpf, row_pitch, frame_pitch, 24u);
}

// The part of a run of `count` consecutive global blocks that starts at block `first` which lies in frame f, as positions
// [*begin, *end) within the run (empty: *begin == *end).  bpf = blocks per frame; (f + 1) * bpf and first + count stay below
// 2^32 (a call has fewer than 2^31 blocks, a grid at most one workgroup more).  The frames a run touches are
// fast_div(first, by_bpf) .. fast_div(first + count - 1, by_bpf), the division block_offset performs; walking them with this
// function cuts the run into its per-frame runs (the histogram tail of the soft side, svs_device.hpp hist_soft_run).
SVS_HD void frame_run(uint32_t first, uint32_t count, uint32_t f, uint32_t bpf, uint32_t *begin, uint32_t *end) {
    const uint32_t lo = f * bpf, hi = lo + bpf, last = first + count;
    // both frame edges clamped into [first, last]: a frame before or behind the run gives an empty part at that end
    const uint32_t b = lo < first ? first : (lo > last ? last : lo), e = hi < first ? first : (hi > last ? last : hi);
    *begin = b - first;
    *end = e - first;
}

constexpr uint32_t kEighth = 0xFFFFFFFFu;   // tile_of() chunk: one contiguous eighth of the grid per XCD-group

// Workgroup -> tile mapping.  Workgroups are dealt round-robin over the 8 XCDs (i % 8 names the
// group that shares an XCD and its L2).  With chunk C > 0, the workgroups of one XCD take C consecutive
// tiles at a time: tiles [g*8C + x*C, g*8C + (x+1)*C) go to XCD-group x in round g, so each XCD streams
// runs of C adjacent tiles.  C = 0 is the identity; C = kEighth gives every XCD-group one contiguous eighth of the grid.
// Placement only affects speed, never results: for every grid the map is a permutation of [0, grid).
SVS_HD uint32_t tile_of(uint32_t i, uint32_t grid, uint32_t chunk) {
    if (chunk == 0) return i;
    if (chunk == kEighth) {  // one contiguous eighth of the grid per XCD-group (bijective for any grid)
        const uint32_t n = grid, q = n / 8u, r = n % 8u, x = i % 8u;
        return (x < r ? x * (q + 1u) : r * (q + 1u) + (x - r) * q) + i / 8u;
    }
    const uint32_t span = 8u * chunk;
    const uint32_t full = (grid / span) * span;  // tiles covered by whole rounds
    if (i >= full) return i;
    const uint32_t x = i % 8u, j = i / 8u;
    return (j / chunk) * span + x * chunk + (j % chunk);
}

// first stream bit of global block gblock in raster order
SVS_HD uint64_t stream_first_raster(uint32_t gblock, uint32_t n) { return (uint64_t)gblock * n; }

// first stream bit of the slot of global block gblock under the keyed order (svs_order.hpp), and of its right neighbour
// gblock + 1 (same frame: the two-block layout needs an even number of blocks per block row) in *second
SVS_HD uint64_t stream_first_keyed(uint32_t gblock, uint32_t n, const FastDiv &by_bpf, const BlockOrderArgs &o,
                                   uint64_t *second = nullptr) {
    const uint32_t f = fast_div(gblock, by_bpf);
    const uint32_t i = gblock - f * by_bpf.div;
    const RoundKeys rk = round_keys(o, o.first_frame + f);
    const uint64_t frame0 = (uint64_t)f * by_bpf.div;
    if (second) *second = (frame0 + block_to_slot(i + 1u, o, rk)) * n;
    return (frame0 + block_to_slot(i, o, rk)) * n;
}

}  // namespace svs
