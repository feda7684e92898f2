// svs_device.hpp - gfx950 kernels of the fused block-DCT / QIM frame operator.
// Per-block arithmetic lives in svs_block.hpp; this file maps blocks to lanes, moves bytes
// between HBM and registers, and packs the extracted bit stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "svs_block.hpp"
#include "svs_colour.hpp"
#include "svs_index.hpp"
#include "svs_order.hpp"
#include "svs_readback.hpp"

namespace svs {

// FastDiv, Geometry, fast_div, block_offset, block_offset_bgr: svs_index.hpp (plain C++, the CPU tier tests it)

#ifndef SVS_WG
#define SVS_WG 256  // threads per workgroup of the embed / extract kernels
#endif

// Workgroup -> tile mapping (svs_index.hpp, tile_of): chunk = 0 is the identity, C > 0 runs of C tiles per XCD-group,
// kEighth one contiguous eighth of the grid per XCD-group.  Placement only affects speed, never results.
__device__ __forceinline__ uint32_t tile_id(uint32_t chunk) { return tile_of(blockIdx.x, gridDim.x, chunk); }

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Frames are streamed exactly once: non-temporal loads/stores keep them from displacing each other
// in L2 / Infinity Cache (measured on MI355X: embed +5 %, extract +11 %, profiles/history/r01_ab_variants.txt)
#define SVS_LD(p) __builtin_nontemporal_load(p)
#define SVS_ST(v, p) __builtin_nontemporal_store(v, p)

// Lanes own one block (8-byte row accesses) or, in the one-row embed kernel, two horizontally adjacent blocks A|B (BPL = 2:
// one 16-byte access per row).  Rows travel as native 2- / 4-dword vectors; the per-block arithmetic
// works on plain scalar arrays filled from them (this exact shape is what hipcc scalarises fully -
// structs of rows updated in place ended up in LDS).
template <int BPL>
struct RowVec;
template <>
struct RowVec<1> { typedef u32x2 type; };
template <>
struct RowVec<2> { typedef u32x4 type; };

template <int BPL>
__device__ __forceinline__ void load_rows(const uint8_t *src, int64_t row_pitch, typename RowVec<BPL>::type (&v)[8]) {
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = SVS_LD(reinterpret_cast<const typename RowVec<BPL>::type *>(src + r * row_pitch));
}

template <int BPL>
__device__ __forceinline__ void store_rows(uint8_t *dst, int64_t row_pitch, const typename RowVec<BPL>::type (&v)[8]) {
    // write-through (sc1) stores: the line is not kept in the XCD's L2 (measured against non-temporal stores,
    // profiles/history/r01_ab_quant_exact.txt: one-shot copy 6.74 vs 6.55 TB/s; embed +1.5 % at n = 3, +9.5 % at n = 10).  The data registers must not be reused before
    // the store has read them: s_nop 1 inside the string (cdna_hip_programming.md section 5.7 item 1).
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        if constexpr (BPL == 1)
            asm volatile("global_store_dwordx2 %0, %1, off sc1\n\ts_nop 1" ::"v"(dst + r * row_pitch), "v"(v[r]) : "memory");
        else
            asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(dst + r * row_pitch), "v"(v[r]) : "memory");
    }
}

// Tail of the extract kernels: a wavefront's 64*BPL consecutive blocks produce exactly n*BPL aligned
// 64-bit words of the packed stream.  The wave assembles them in a private LDS array of big-endian dwords
// (stream bit p of the wave's chunk = bit 31 - p%32 of dword p/32): every lane ORs its n-bit string in at bit
// offset lane*BPL*n (ds_or_b32 on at most three dwords), then lanes w < 2*BPL*n byte-swap one dword each and store
// it.  SVS_WAVE_BITS_DWORDS = dwords per wave incl. slack for the unconditional second / third OR.
#define SVS_WAVE_BITS_DWORDS(BPL) (2 * (BPL) * 63 + 4)

__device__ __forceinline__ void wave_lds_fence() {  // wave-private LDS: pins the compiler's order, no workgroup barrier
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int U>
__device__ __forceinline__ void or_bit_string(uint32_t *mine, uint32_t bit_at, uint32_t hi, uint32_t lo) {
    // hi:lo = up to 8U-1 bits, MSB-first from bit 63; lands at stream bit `bit_at` of the wave's chunk
    const uint32_t d = bit_at >> 5, o = bit_at & 31u;
    atomicOr(&mine[d], hi >> o);
    atomicOr(&mine[d + 1], __builtin_amdgcn_alignbit(hi, lo, o));           // ({hi,lo} >> o) & 0xffffffff
    if constexpr (U > 4) atomicOr(&mine[d + 2], __builtin_amdgcn_alignbit(lo, 0u, o));  // o + n > 64 needs n > 32
}

template <int U, int BPL>
__device__ __forceinline__ void emit_wave_bits(uint32_t *mine, uint32_t lane, uint64_t wave_first_block, uint32_t n,
                                               uint32_t hi_a, uint32_t lo_a, uint32_t hi_b, uint32_t lo_b,
                                               uint8_t *__restrict__ out, uint64_t out_bytes) {
    const uint32_t words = 2u * BPL * n;  // 64*BPL*n bits
    for (uint32_t w = lane; w < words + 4u; w += 64u) mine[w] = 0u;
    wave_lds_fence();
    or_bit_string<U>(mine, lane * BPL * n, hi_a, lo_a);
    if constexpr (BPL == 2) or_bit_string<U>(mine, (lane * BPL + 1u) * n, hi_b, lo_b);
    wave_lds_fence();
    const uint64_t wave_byte0 = wave_first_block * n / 8u;  // multiple of 8 bytes
    for (uint32_t w = lane; w < words; w += 64u) {
        const uint32_t word = __builtin_bswap32(mine[w]);  // first stream bit -> MSB of the first byte in memory
        const uint64_t at = wave_byte0 + 4ull * w;
        if (at + 4 <= out_bytes) {
            *reinterpret_cast<uint32_t *>(out + at) = word;
        } else {
            for (uint32_t j = 0; j < 4 && at + j < out_bytes; ++j) out[at + j] = (uint8_t)(word >> (8 * j));
        }
    }
}

// ---------------------------------------------------------------------------------------
// Keyed block order (svs_order.hpp).  A KEYED instantiation takes one BlockOrderArgs after its last parameter (the parameter
// pack `Order`, one element exactly when KEYED); the unkeyed ones take none, so their parameter lists and their code are
// what they were before the order existed.  Pixels still move in raster order - every lane loads and stores its own
// block(s), coalesced - and only a block's place in the payload stream changes: block i of call frame f takes stream bits
// (f N + sigma_t^-1(i)) n .. + n - 1, t = first_frame + f.  Payload reads become one scattered 8-byte read per block.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ BlockOrderArgs order_arg() { return BlockOrderArgs{}; }
__device__ __forceinline__ BlockOrderArgs order_arg(const BlockOrderArgs &o) { return o; }

// s_b of global block gblock (svs_block.hpp): per lane - a wave may straddle two frames
__device__ __forceinline__ uint32_t dither_seed_of(uint32_t gblock, const Geometry &g, const DitherArgs &d) {
    const uint32_t f = fast_div(gblock, g.by_bpf);
    return dither_block_seed(d.seed, d.first_frame + f, gblock - f * g.by_bpf.div);
}

// first stream bit of global block gblock (KEYED: of its slot), and of its right neighbour gblock + 1 (same frame: the
// two-block layout needs an even number of blocks per block row) in *second
template <bool KEYED>
__device__ __forceinline__ uint64_t stream_first(uint32_t gblock, uint32_t n, const Geometry &g, const BlockOrderArgs &o,
                                                 uint64_t *second = nullptr) {
    if constexpr (!KEYED) return stream_first_raster(gblock, n);
    else return stream_first_keyed(gblock, n, g.by_bpf, o, second);
}

// KEYED extraction: a block's n bits (hi:lo, MSB first from bit 63) ORed into the packed output at stream bit `pos` with
// 32-bit global atomics (the call has cleared the output first).  Only dwords that receive a 1 bit are touched; a 1 bit lies
// below the call's capacity, and what the OR adds to the last, partial dword past it is 0.
template <int U>
__device__ __forceinline__ void or_bits_global(uint8_t *out, uint64_t pos, uint32_t hi, uint32_t lo) {
    uint32_t *w = reinterpret_cast<uint32_t *>(out) + (pos >> 5);
    const uint32_t o = (uint32_t)(pos & 31u);
    const uint32_t x0 = hi >> o, x1 = __builtin_amdgcn_alignbit(hi, lo, o);
    if (x0) atomicOr(&w[0], __builtin_bswap32(x0));   // stream bit p -> bit 7 - p % 8 of byte p / 8
    if (x1) atomicOr(&w[1], __builtin_bswap32(x1));
    if constexpr (U > 4) {                               // o + n > 64 needs n > 32
        const uint32_t x2 = __builtin_amdgcn_alignbit(lo, 0u, o);
        if (x2) atomicOr(&w[2], __builtin_bswap32(x2));
    }
}

// A worklist entry: one block for the eight-lane exact replay.  8-byte aligned because row1_deposit / row1_collect move its rows
// as 8-byte LDS accesses.
struct alignas(8) GuardEntry {
    uint32_t px[16];   // rows as (low dword, high dword) pairs: the original pixels in, the exact stego pixels out
    uint32_t hi, lo;   // payload window of the block
    uint32_t nb;       // bits the block takes
    uint32_t pad;
};
static_assert(sizeof(GuardEntry) == 80 && sizeof(GuardEntry) % 8 == 0, "80-byte entries, rows 8-byte aligned");
#define SVS_GUARD_TILE 72   // floats per block of the transposition tile: element (i, j) at 9 i + j; 72 = 8 (mod 64) keeps the
                            // eight groups of a wave on different LDS banks in both directions

// ---------------------------------------------------------------------------------------
// Exact replays, EIGHT LANES PER BLOCK: the blocks that a kernel's fast arithmetic cannot decide are redone with pocketfft's
// arithmetic (svs::pf, the same operation sequence per line as the lane-per-block forms of svs_block.hpp / svs_readback.hpp).
// Lane r of a group of eight transforms column r, then row r, of its block; the lines meet in the group's transposition tile t,
// element (i, j) at S i + j (S = 9: SVS_GUARD_TILE, embed / extract; S = 8: read-back's 64-float tiles).
// ---------------------------------------------------------------------------------------
// forward: the block's pixel column r, then coefficient row r -> c[v] = D[r][v]
template <int S>
__device__ __forceinline__ void forward8(const uint32_t *px, float *t, uint32_t r, float (&c)[8]) {
    float a[8], b[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) a[y] = (float)((px[2 * y + (r >> 2)] >> (8u * (r & 3u))) & 0xffu);
    pf::dct2_8(a, b);                       // b[u] = V[u][r]
#pragma unroll
    for (int u = 0; u < 8; ++u) t[S * u + r] = b[u];
    wave_lds_fence();
#pragma unroll
    for (int x = 0; x < 8; ++x) a[x] = t[S * r + x];   // V[r][x]
    wave_lds_fence();
    pf::dct2_8(a, c);
}

// inverse: coefficient column r (c[u] = D[u][r]), vertical first (config_and_setup.py:168), then pixel row r -> p[x] = P[r][x]
template <int S>
__device__ __forceinline__ void inverse8(const float (&c)[8], float *t, uint32_t r, float (&p)[8]) {
    float a[8], b[8];
    pf::dct3_8(c, b);                       // b[y] = column r of the vertical inverse
#pragma unroll
    for (int y = 0; y < 8; ++y) t[S * y + r] = b[y];
    wave_lds_fence();
#pragma unroll
    for (int x = 0; x < 8; ++x) a[x] = t[S * r + x];
    pf::dct3_8(a, p);
}

// this lane's rank among the lanes of `mask` (the lanes below it whose bit is set)
__device__ __forceinline__ uint32_t wave_rank(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// The wave-private worklist of the replays (ballot + mbcnt: no atomics, no barrier).  mine[j]: this lane's block j (one or two
// blocks per lane) is to be redone.  The entries are numbered block 0's in lane order, then block 1's, and go in rounds of CAP:
//   deposit(j, e)      the owner of block j fills entry e (0 .. CAP - 1) of the round
//   replay(e, grp, r)  lanes 8 grp .. 8 grp + 7 redo entry e, lane r = lane & 7 - eight entries per pass
//   collect(j, e)      the owner takes block j's result back
// Returns the number of entries - 0, wave-uniform, after the ballot alone when no lane has one.
template <int CAP, int B, class Deposit, class Replay, class Collect>
__device__ __forceinline__ uint32_t wave_worklist(const bool (&mine)[B], uint32_t lane, Deposit &&deposit, Replay &&replay,
                                                  Collect &&collect) {
    static_assert(B == 1 || B == 2, "one or two blocks per lane");
    uint64_t mask[B], any = 0;
    uint32_t rank[B], total = 0;
#pragma unroll
    for (int j = 0; j < B; ++j) { mask[j] = __ballot(mine[j]); any |= mask[j]; }
    if (any == 0) return 0;                 // wave-uniform
#pragma unroll
    for (int j = 0; j < B; ++j) { rank[j] = total + wave_rank(mask[j]); total += (uint32_t)__popcll(mask[j]); }
    const uint32_t grp = lane >> 3, r = lane & 7u;
    for (uint32_t base = 0; base < total; base += (uint32_t)CAP) {   // wave-uniform
        bool in[B];
#pragma unroll
        for (int j = 0; j < B; ++j) in[j] = mine[j] && rank[j] >= base && rank[j] < base + (uint32_t)CAP;
#pragma unroll
        for (int j = 0; j < B; ++j)
            if (in[j]) deposit(j, rank[j] - base);
        wave_lds_fence();
        const uint32_t todo = min(total - base, (uint32_t)CAP);
        for (uint32_t at = 0; at < todo; at += 8u)
            if (at + grp < todo) replay(at + grp, grp, r);
        wave_lds_fence();
#pragma unroll
        for (int j = 0; j < B; ++j)
            if (in[j]) collect(j, rank[j] - base);
        if constexpr (CAP < 64) wave_lds_fence();   // the next round overwrites the entries
    }
    return total;
}

// FAST extraction, second path: a block with a quantiser input inside the per-block tie margin (svs_block.hpp SVS_TIE2_*)
// gets the pocketfft-identical forward transform on eight lanes; lane r then takes coefficient column r and quantises its
// coefficients k = 8 u + r of the rows u the payload uses; the bits are ORed into the entry.  About 200 instructions per pass
// of 8 blocks, against 580 for every wave that had such a lane when the whole block was redone by its own lane (round 2).
template <int QM>
__device__ __forceinline__ void extract_replay8(GuardEntry *e, float *t, uint32_t r, uint32_t n, const QimParams &qp) {
    float b[8];
    forward8<9>(e->px, t, r, b);            // b[v] = D[r][v]
#pragma unroll
    for (int v = 0; v < 8; ++v) t[9 * r + v] = b[v];
    wave_lds_fence();
    uint32_t hi = 0, lo = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const uint32_t k = 8u * u + r;
        if (k >= 1u && k <= n) {            // no lane of the wave enters for rows the payload does not use
            const uint32_t bit = (uint32_t)quant_index<QM>(t[9 * u + r], qp) & 1u;
            const uint32_t i = k - 1u;
            if (i < 32u) hi |= bit << (31u - i);
            else lo |= bit << (63u - i);
        }
    }
    if (hi) atomicOr(&e->hi, hi);
    if (lo) atomicOr(&e->lo, lo);
}

// the wave's tie blocks through the worklist (CAP entries per round); on return hi/lo of those blocks hold the reference's bits
template <int QM, int CAP>
__device__ __forceinline__ void extract_phase2(GuardEntry *entries, float *tile, uint32_t lane, uint32_t n, const QimParams &qp,
                                               bool tie, const uint32_t (&ax)[8], const uint32_t (&ay)[8], uint32_t &hi, uint32_t &lo) {
    wave_worklist<CAP>(
        {tie}, lane,
        [&](int, uint32_t i) {
            GuardEntry *e = &entries[i];
#pragma unroll
            for (int r = 0; r < 8; ++r) { e->px[2 * r] = ax[r]; e->px[2 * r + 1] = ay[r]; }
            e->hi = 0; e->lo = 0;
        },
        [&](uint32_t i, uint32_t grp, uint32_t r) { extract_replay8<QM>(&entries[i], tile + grp * SVS_GUARD_TILE, r, n, qp); },
        [&](int, uint32_t i) { hi = entries[i].hi; lo = entries[i].lo; });
}

// ---------------------------------------------------------------------------------------
// EXTRACT: one lane = one block; a wavefront's 64 blocks produce exactly n
// aligned 64-bit words of the packed stream (stream bit = global block * n + i), assembled through
// a wave-private LDS byte array and written with plain dword stores - no atomics, no pre-zeroed
// output.  HBM traffic per block: 64 B read + n bits written.
// ---------------------------------------------------------------------------------------
#define SVS_EXTRACT_CAP 16   // worklist entries per wave and round of the extract kernels
// BPL (blocks per lane) is always 1 here and in the other non-row1 kernels; it stays in their template parameter lists so that
// the kernel symbols match the ones the traces under profiles/ name.
template <int U, int QM, int BPL, int NFIX = 0, bool KEYED = false, class... Order>
__global__ __launch_bounds__(SVS_WG) void extract_kernel(const uint8_t *__restrict__ gray, const Geometry g,
                                                      const QimParams qp, uint8_t *__restrict__ out,
                                                      const uint64_t out_bytes, const Order... order) {
    static_assert(BPL == 1, "one block per lane");
    static_assert(sizeof...(Order) == (KEYED ? 1u : 0u), "KEYED instantiations take one BlockOrderArgs");
    __shared__ uint32_t flags[SVS_WG / 64][SVS_WAVE_BITS_DWORDS(1)];
    __shared__ GuardEntry entries[SVS_WG / 64][SVS_EXTRACT_CAP];
    __shared__ float tiles[SVS_WG / 64][8 * SVS_GUARD_TILE];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t tile = tile_id(g.xcd_chunk);
    const uint32_t gblock = tile * (uint32_t)SVS_WG + threadIdx.x;
    const uint32_t n = g.n_ac;

    // the block's bits, MSB first: bit i at position 63-i of hi:lo
    uint32_t hi = 0, lo = 0;
    uint32_t ax[8], ay[8];
    bool tie = false;
    float off = 0.0f;
    if (gblock < g.total_blocks) {
        u32x2 v[8];
        load_rows<1>(gray + block_offset(gblock, g), g.row_pitch, v);
#pragma unroll
        for (int r = 0; r < 8; ++r) { ax[r] = v[r].x; ay[r] = v[r].y; }
        tie = extract_block_cheap<U, QM, NFIX>(ax, ay, n, qp, hi, lo, off);      // -> candidate
    }
    // Step two only in waves with a candidate (svs_block.hpp): pocketfft's own flat index 4 and the per-block tie margin.
    // Stego frames at delta >= 8 have none: one ballot.  (Round 3 computed both for every block: +3..7 % on stego frames.)
    if (__ballot(tie) != 0) {
        if (gblock < g.total_blocks) tie = extract_block_settle<QM>(ax, ay, n, qp, hi, off);
    }
    // A quantiser input within the per-block error bound of a rounding tie (svs_block.hpp, SVS_TIE2_*): those blocks get the
    // pocketfft-identical transform from eight lanes each (wave-private worklist).  Never taken on stego frames at delta >= 8.
    extract_phase2<QM, SVS_EXTRACT_CAP>(&entries[wave][0], &tiles[wave][0], lane, n, qp, tie, ax, ay, hi, lo);
    if constexpr (KEYED) {
        if (gblock < g.total_blocks) or_bits_global<U>(out, stream_first<true>(gblock, n, g, order_arg(order...)), hi, lo);
    } else {
        emit_wave_bits<U, 1>(&flags[wave][0], lane, (uint64_t)tile * (uint32_t)SVS_WG + wave * 64u, n, hi, lo, 0u, 0u, out, out_bytes);
    }
}

// ---------------------------------------------------------------------------------------
// EXACT-mode kernels (pocketfft-identical arithmetic, svs_block.hpp "EXACT mode"): one block per lane.
// The embed kernel transforms all 64 coefficients both ways (about 2 700 VALU instructions per block),
// so it is VALU-bound at roughly 40 % of the fast kernel's rate; it exists for bit-identical output.
// ---------------------------------------------------------------------------------------
// Register-allocated for 2 waves per SIMD: +1..3 % over 3; 4 spills 52 B and is 8 % slower.
template <int QM, int U = 8, bool KEYED = false, class... Order>  // U: coefficient rows the quantiser loop covers (flat indices 1..n lie in rows < U)
__global__ __launch_bounds__(SVS_WG, 2) void embed_exact_kernel(const uint8_t *gray,  // may alias stego
                                                          uint8_t *stego, const Geometry g,
                                                          const QimParams qp,
                                                          const uint32_t *__restrict__ bits,
                                                          const uint64_t bit_offset, const uint64_t n_bits,
                                                          const uint32_t n_words, const CoeffTable sel,
                                                          const DitherArgs dith, const ChannelArgs chan,
                                                          const StepArgs steps, const Order... order) {
    static_assert(sizeof...(Order) == (KEYED ? 1u : 0u), "KEYED instantiations take one BlockOrderArgs");
    // The requantisation channel (svs_requantise_dev; chan.on): a wave-uniform branch around everything else, compiled into ONE
    // instantiation - the unkeyed eight-row QM_DOUBLE one, which otherwise serves only calls whose delta is no float32 value
    // (the channel's division is the float32 one whatever QM says).  Every other instantiation ignores `chan`.  The same
    // round trip as the body below - load eight rows, forward, touch coefficients, inverse, store - without a payload window,
    // a budget or an early copy: every block is requantised, and the store rounds (requantise_block_exact).  A lane loads its
    // rows before it stores them, so in place works as for the embed.
    if constexpr (QM == QM_DOUBLE && U == 8 && !KEYED) {
        if (chan.on) {
            const uint32_t gblock = tile_id(g.xcd_chunk) * (uint32_t)SVS_WG + threadIdx.x;
            if (gblock >= g.total_blocks) return;
            const int64_t off = block_offset(gblock, g);
            typename RowVec<1>::type v[8];
            load_rows<1>(gray + off, g.row_pitch, v);
            uint32_t ax[8], ay[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) { ax[r] = v[r].x; ay[r] = v[r].y; }
            requantise_block_exact(ax, ay, chan);
#pragma unroll
            for (int r = 0; r < 8; ++r) { v[r].x = ax[r]; v[r].y = ay[r]; }
            store_rows<1>(stego + off, g.row_pitch, v);
            return;
        }
    }
    // SVS_NEAREST, SVS_MINMOVE: ONE wave-uniform branch around the whole body, the rule a compile-time constant on every side
    // (QimRule; under SVS_MINMOVE its half_cell is the launch's, the kind is the constant: rule_from_word with a word > 1).
    // A `return` inside the body leaves the body, and nothing follows the calls.
    // A coefficient selection (sel.count != 0; the U = 8 instantiations only - svs_route.hpp plans no other for one) is a
    // second such branch: `table` is a compile-time NULL on the side without one, which is the body as it was.
    // A keyed dither (dith.on; the U = 8 instantiations only - svs_route.hpp plans no other for one) is a third: `dithered` is a
    // compile-time false on every side that was there before, which keeps its code; the dithered side has its own three copies.
    // Per-coefficient steps (steps.on; svs_stepped_embed_dev) are a fourth, compiled into the two eight-row QM_DOUBLE
    // instantiations alone, which otherwise serve only calls whose delta is no float32 value (the stepped arithmetic is the
    // float32 one whatever QM says; svs_route.hpp plans no other instantiation for a stepped call).  `stepped` is a compile-time
    // false on every side that was there before.  The stepped side reads its table from the dither's copy, on or off, as the
    // dithered side does: the call's selection or the prefix table of n_ac.
    // A matrix call (steps.matrix(); svs_matrix_embed_dev) is one more side of the stepped side, behind it: the same loads, stream
    // position, budget and store with g.n_ac = k stream bits a block and a table of 2^k - 1 slots; embed_block_matrix in the place
    // of embed_block_stepped.  It keeps a wave-private tile of 64 count floats in dynamic LDS - the values of the flipped forms;
    // twice that with the pair search, for its costs -, which only this launch requests (svs_capi.hip matrix_lds_bytes); a lane
    // reads and writes its own column alone, so nothing is fenced.
    const auto body = [&](const QimRule qp, const CoeffTable *table, auto dithered, auto stepped, auto matrix) __attribute__((always_inline)) {
        const uint32_t gblock = tile_id(g.xcd_chunk) * (uint32_t)SVS_WG + threadIdx.x;
        if (gblock >= g.total_blocks) return;
        const int64_t off = block_offset(gblock, g);
        typename RowVec<1>::type v[8];
        load_rows<1>(gray + off, g.row_pitch, v);
        const uint32_t n = g.n_ac;  // 0 = round-trip every block without touching a coefficient
        const uint64_t first = stream_first<KEYED>(gblock, n, g, order_arg(order...));
        if (first >= n_bits) {
            if (stego != gray) store_rows<1>(stego + off, g.row_pitch, v);
            return;
        }
        uint32_t ax[8], ay[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) { ax[r] = v[r].x; ay[r] = v[r].y; }
        uint32_t hi, lo;
        payload_window(bits, n_words, bit_offset + first, hi, lo);
        if constexpr (decltype(stepped)::value) {
            uint32_t s_b = 0u;
            if constexpr (decltype(dithered)::value) s_b = dither_seed_of(gblock, g, dith);
            if constexpr (decltype(matrix)::value) {
                extern __shared__ float matrix_tile[];
                const uint32_t per_wave = 64u * table->count * ((steps.matrix() & 8u) ? 2u : 1u);   // svs_capi.hip matrix_lds_bytes
                float *tile = matrix_tile + (threadIdx.x >> 6) * per_wave + (threadIdx.x & 63u);
                embed_block_matrix<decltype(dithered)::value>(ax, ay, block_budget(first, n_bits, n), hi, qp.kind, *table, steps,
                                                              steps.matrix(), s_b, tile, 64u);
            } else
                embed_block_stepped<decltype(dithered)::value>(ax, ay, block_budget(first, n_bits, n), hi, lo, qp.kind, *table, steps, s_b);
        } else if constexpr (decltype(dithered)::value)
            embed_block_exact<U, QM, true>(ax, ay, n, block_budget(first, n_bits, n), hi, lo, qp, false, table,
                                           dither_seed_of(gblock, g, dith));
        else
            embed_block_exact<U, QM>(ax, ay, n, block_budget(first, n_bits, n), hi, lo, qp, false, table);
#pragma unroll
        for (int r = 0; r < 8; ++r) { v[r].x = ax[r]; v[r].y = ay[r]; }
        store_rows<1>(stego + off, g.row_pitch, v);
    };
    constexpr std::false_type plain{};
    if constexpr (QM == QM_DOUBLE && U == 8) {
        if (steps.on) {    // wave-uniform
            constexpr std::true_type stepped{};
            if (steps.matrix()) {   // wave-uniform; behind the side that was there first, which returns
                constexpr std::true_type matrix{};
                if (dith.on) {
                    constexpr std::true_type dithered{};
                    if (g.pad > 1u) body(QimRule(qp, (uint32_t)RULE_MINMOVE), &dith.sel, dithered, stepped, matrix);
                    else if (g.pad) body(QimRule(qp, 1u), &dith.sel, dithered, stepped, matrix);
                    else body(QimRule(qp, 0u), &dith.sel, dithered, stepped, matrix);
                    return;
                }
                if (g.pad > 1u) body(QimRule(qp, (uint32_t)RULE_MINMOVE), &dith.sel, plain, stepped, matrix);
                else if (g.pad) body(QimRule(qp, 1u), &dith.sel, plain, stepped, matrix);
                else body(QimRule(qp, 0u), &dith.sel, plain, stepped, matrix);
                return;
            }
            if (dith.on) {
                constexpr std::true_type dithered{};
                if (g.pad > 1u) body(QimRule(qp, (uint32_t)RULE_MINMOVE), &dith.sel, dithered, stepped, plain);
                else if (g.pad) body(QimRule(qp, 1u), &dith.sel, dithered, stepped, plain);
                else body(QimRule(qp, 0u), &dith.sel, dithered, stepped, plain);
                return;
            }
            if (g.pad > 1u) body(QimRule(qp, (uint32_t)RULE_MINMOVE), &dith.sel, plain, stepped, plain);
            else if (g.pad) body(QimRule(qp, 1u), &dith.sel, plain, stepped, plain);
            else body(QimRule(qp, 0u), &dith.sel, plain, stepped, plain);
            return;
        }
    }
    if constexpr (U == 8) {
        if (dith.on) {     // wave-uniform; `sel` is the call's selection or the prefix table of n_ac: one selected loop serves both
            constexpr std::true_type dithered{};
            if (g.pad > 1u) body(rule_from_word(qp, g.pad), &dith.sel, dithered, plain, plain);
            else if (g.pad) body(QimRule(qp, 1u), &dith.sel, dithered, plain, plain);
            else body(QimRule(qp, 0u), &dith.sel, dithered, plain, plain);
            return;
        }
        if (sel.count) {   // Geometry::n_ac == sel.count: the stream ranges and the block budget are those of n_ac slots
            if (g.pad > 1u) body(rule_from_word(qp, g.pad), &sel, plain, plain, plain);
            else if (g.pad) body(QimRule(qp, 1u), &sel, plain, plain, plain);
            else body(QimRule(qp, 0u), &sel, plain, plain, plain);
            return;
        }
    }
    if (g.pad > 1u) body(rule_from_word(qp, g.pad), nullptr, plain, plain, plain);
    else if (g.pad) body(QimRule(qp, 1u), nullptr, plain, plain, plain);
    else body(QimRule(qp, 0u), nullptr, plain, plain, plain);
}

// ---------------------------------------------------------------------------------------
// EMBED, streaming kernel (launched for two coefficient rows, n = 8..15, since round 6 - one row: embed_row1_kernel below; flags
// 0 and SVS_EXACT_GUARDED, include/svsdct.h): one lane = one block, grid = ceil(total_blocks / SVS_WG) workgroups of SVS_WG.
// HBM traffic per block: 64 B read + 64 B written + n payload bits read - nothing else, whatever the content.
//   phase 1  lane = block: the cheap arithmetic (svs_block.hpp) - embed_block_guarded (n <= 7) / _guarded2 (n = 8..15):
//            pocketfft-identical payload coefficients, sparse inverse, rigorous per-block error bound - the result is the
//            reference's, bit for bit.  Returns "undecided" for the blocks whose truncation the reference's own float32
//            noise decides.  (n >= 16 does not come here: every mode runs embed_exact_kernel.)
//   phase 2  the wave's undecided blocks are compacted into a wave-private LDS worklist (ballot + mbcnt: no atomics, no
//            barrier) and redone with the pocketfft-identical arithmetic by EIGHT LANES PER BLOCK: lane r of a group
//            transforms column r, then row r, of its block - the four 1-D passes of the reference (vertical / horizontal
//            forward, vertical / horizontal inverse, config_and_setup.py:135,168) with a transposition through a
//            wave-private LDS tile in between.  Every value comes from the same svs::pf operation sequence as in
//            embed_block_exact, so the bits are the same; what changes is the shape: about 40 VGPRs and 300-450
//            instructions per pass of 8 blocks instead of 140 VGPRs and 2 100 per pass of 64 - affordable inside the
//            streaming kernel.  More than SVS_GUARD_CAP undecided blocks in a wave (flat content) take further rounds.
//   phase 3  every lane stores its rows (its own result, or the one it collected from the worklist): the wave's stores
//            cover whole 512-byte row segments - no partial lines, no second launch, no scratch buffer in HBM.
// `gray` and `stego` may be the same buffer (in-place embedding, include/svsdct.h), so neither is __restrict__: every
// lane loads its own rows before it stores them and touches nobody else's.
// ---------------------------------------------------------------------------------------
#define SVS_GUARD_CAP 32    // worklist entries per wave and round (80 B each) of the one-row (rigorous guard) embed kernel

// QIM on flat indices k = 8 u + r in 1..n (config_and_setup.py:139-158): one coefficient per lane and row, so a wave
// runs n / 8 + 1 quantiser sequences, each on all the lanes that have a coefficient.  RULE: qim_target (svs_block.hpp); k is
// the lane's own here, so the band of SVS_MINMOVE comes from a read of the margin table
template <int QM, int UROWS, int RULE>
__device__ __forceinline__ void qim_replay8(float (&a)[8], uint32_t hi, uint32_t lo, uint32_t nb, uint32_t r, uint32_t n,
                                            const QimRule &qp) {
#pragma unroll
    for (int u = 0; u < UROWS; ++u) {
        const uint32_t k = 8u * u + r;
        if (k >= 1u && k <= n) {
            const int i = (int)k - 1;
            const int bit = (int)window_bit(hi, lo, i);
            const float c = a[u];
            const float cn = qim_target<QM, RULE>(c, bit, qp, qim_band<RULE>(qp, k));
            a[u] = ((uint32_t)i < nb) ? cn : c;
        }
    }
}

// px: the block's 16 row dwords (low, high per row) in LDS - original pixels in, exact stego pixels out
// UROWS: coefficient rows that can hold payload (n <= 8 UROWS - 1); the quantiser loop covers only those
template <int QM, int UROWS = 8>
__device__ __forceinline__ void guard_replay8(uint32_t *px, uint32_t hi, uint32_t lo, uint32_t nb, float *t, uint32_t r, uint32_t n,
                                              const QimRule &qp) {
    float a[8], b[8];
    forward8<9>(px, t, r, b);   // b[v] = D[r][v]: coefficient row r
    // to coefficient COLUMNS (what the vertical inverse wants): lane r takes D[u][r], u = 0..7
#pragma unroll
    for (int v = 0; v < 8; ++v) t[9 * r + v] = b[v];
    wave_lds_fence();
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] = t[9 * u + r];
    wave_lds_fence();
    if (qp.kind == (uint32_t)RULE_MINMOVE) qim_replay8<QM, UROWS, RULE_MINMOVE>(a, hi, lo, nb, r, n, qp);
    else if (qp.kind == (uint32_t)RULE_NEAREST) qim_replay8<QM, UROWS, RULE_NEAREST>(a, hi, lo, nb, r, n, qp);
    else qim_replay8<QM, UROWS, RULE_REFERENCE>(a, hi, lo, nb, r, n, qp);
    inverse8<9>(a, t, r, b);   // pixel row r
    uint32_t lo4, hi4;
    store_row_trunc(b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], lo4, hi4);   // np.uint8(np.clip(.)) (:171)
    px[2 * r] = lo4;
    px[2 * r + 1] = hi4;
}

// phase 1 for one block whose rows are ax/ay, in place: stego pixels out - unless the block is undecided, then its original
// pixels are left untouched (svs_block.hpp decides before it writes).  -> undecided
template <int U, int QM, int NFIX = 0>
__device__ __forceinline__ bool guard_phase1(uint32_t (&ax)[8], uint32_t (&ay)[8], uint32_t n, uint64_t first,
                                             const QimRule &qp, const uint32_t *__restrict__ bits,
                                             uint64_t bit_offset, uint64_t n_bits, uint32_t n_words,
                                             uint32_t *keep_hi = nullptr) {
    const uint32_t hi = window32(payload_qword(bits, n_words, bit_offset + first), (uint32_t)((bit_offset + first) & 31u)), lo = 0;
    if (keep_hi) *keep_hi = hi;
    const uint32_t nb = block_budget(first, n_bits, n);
    static_assert(U <= 2, "n <= 15: with more coefficient rows every mode runs the lane-per-block pocketfft kernel");
    if constexpr (U == 1) return embed_block_guarded<QM>(ax, ay, n, nb, hi, lo, qp);          // n <= 7: rigorous, 8 tests
    else return embed_block_guarded2<QM, NFIX>(ax, ay, n, nb, hi, lo, qp);                    // n = 8..15: rigorous, 64 tests
}
// what phase 2 needs to rebuild a block's payload window (kept out of the lanes' registers on the common path)
struct GuardPayload {
    const uint32_t *bits;
    uint64_t bit_offset, n_bits;
    uint32_t n_words;
};

// phase 2: the wave's undecided blocks (their rows still hold the ORIGINAL pixels; `first` is the lane's first stream bit)
// through the worklist `entries` (CAP entries) and the transposition tile `tile` (8 * SVS_GUARD_TILE floats), both private to
// the wave.  On return the rows of undecided blocks hold the exact stego pixels.  Returns the number of blocks redone.
template <int QM, int CAP = SVS_GUARD_CAP, bool KEPT = false, int UROWS = 2>
__device__ __forceinline__ uint32_t guard_phase2(GuardEntry *entries, float *tile, uint32_t lane, uint32_t n,
                                                 const QimRule &qp, const GuardPayload &pl,
                                                 bool und, uint64_t first, uint32_t (&ax)[8], uint32_t (&ay)[8],
                                                 uint32_t hi_kept = 0) {
    return wave_worklist<CAP>(
        {und}, lane,
        [&](int, uint32_t i) {
            GuardEntry *e = &entries[i];
#pragma unroll
            for (int r = 0; r < 8; ++r) { e->px[2 * r] = ax[r]; e->px[2 * r + 1] = ay[r]; }
            uint32_t hi, lo;
            if constexpr (KEPT) { hi = hi_kept; lo = 0; }   // n <= 15: the window's first word, still in a register from phase 1
            else payload_window(pl.bits, pl.n_words, pl.bit_offset + first, hi, lo);
            e->hi = hi; e->lo = lo; e->nb = block_budget(first, pl.n_bits, n);
        },
        [&](uint32_t i, uint32_t grp, uint32_t r) {
            GuardEntry *e = &entries[i];
            guard_replay8<QM, UROWS>(e->px, e->hi, e->lo, e->nb, tile + grp * SVS_GUARD_TILE, r, n, qp);
        },
        [&](int, uint32_t i) {
            const GuardEntry *e = &entries[i];
#pragma unroll
            for (int r = 0; r < 8; ++r) { ax[r] = e->px[2 * r]; ay[r] = e->px[2 * r + 1]; }
        });
}

// phase 2 over PARKED rows (round 4; the two-row kernel): every lane has written its block's original rows to its slot of a
// wave-private LDS array before phase 1 (slot = lane, SVS_SLOT_DWORDS apart), so phase 1 works in place and an undecided block
// needs no deposit: the worklist is a list of {slot, budget, payload window} words, the exact replay reads and writes the
// slots, and the owners of undecided blocks read theirs back.  One round: the worklist holds all 64 lanes if it must.
#define SVS_SLOT_DWORDS 18   // 16 row dwords + 2: 8-byte aligned, and 16 consecutive lanes hit 16 different even banks
template <int QM>
__device__ __forceinline__ uint32_t guard_phase2_slots(uint32_t *slots, u32x2 *meta, float *tile, uint32_t lane, uint32_t n,
                                                       const QimRule &qp, bool und, uint32_t nb, uint32_t hi,
                                                       uint32_t (&ax)[8], uint32_t (&ay)[8]) {
    return wave_worklist<64>(
        {und}, lane,
        [&](int, uint32_t i) { u32x2 m; m.x = lane | (nb << 8); m.y = hi; meta[i] = m; },
        [&](uint32_t i, uint32_t grp, uint32_t r) {
            const u32x2 m = meta[i];
            guard_replay8<QM, 2>(slots + (m.x & 0xffu) * SVS_SLOT_DWORDS, m.y, 0u, m.x >> 8, tile + grp * SVS_GUARD_TILE, r, n, qp);
        },
        [&](int, uint32_t) {
            const u32x2 *mine = reinterpret_cast<const u32x2 *>(slots + lane * SVS_SLOT_DWORDS);
#pragma unroll
            for (int r = 0; r < 8; ++r) { const u32x2 v = mine[r]; ax[r] = v.x; ay[r] = v.y; }
        });
}

// Register targets (waves per SIMD) of the embed kernels: natural allocation.  (One row: 96 VGPRs, 5 waves; spills in the
// replay cost 1.90 vs 1.71 ms.  Two rows: 103 VGPRs, 4 waves; a target of 5 waves spills 68 B and costs 3.26 vs 2.74 ms
// per 600 x 4K, 6 waves 4.30 ms - profiles/r04_ab_two_row.txt.)
// Lanes past the end of the batch shadow its last block(s): they load and compute like everybody else, and never store.
template <int BPL>
__device__ __forceinline__ uint32_t shadow_block(uint32_t gblock, const Geometry &g, bool &live) {
    live = gblock < g.total_blocks;
    return live ? gblock : g.total_blocks - (uint32_t)BPL;   // the host launches with total_blocks >= BPL (a multiple of BPL)
}
// Two rows, except for power-of-two delta: original rows parked in LDS and phase 1 in place (guard_phase2_slots: 68 instead
// of 103 VGPRs, 5 instead of 4 waves per SIMD, 29.7 KB of LDS per workgroup).  The kernel is bound by vector issue either
// way, and which form the compiler schedules better depends on the quantiser: general delta (QM_F32, the GUI's default 20)
// 2.62 vs 2.78 ms per 600 x 4K at n = 10 and 2.82 vs 2.93 at n = 15 in favour of the parked form, power-of-two delta 2.74 vs
// 2.65 against it - both orders of a 15-round A/B (profiles/r04_ab_two_row.txt).
// The experiments library (-DSVS_EXPERIMENTS) counts the blocks a launch redid exactly into a device counter (measurement
// hook svs_guard_counter_set); the product kernels have no such parameter and the product library no such state.
#if defined(SVS_EXPERIMENTS)
#define SVS_REPLAY_COUNTER_PARAM , unsigned long long *__restrict__ replay_counter
#else
#define SVS_REPLAY_COUNTER_PARAM
#endif
template <int U, int QM, int BPL, int NFIX = 0, bool KEYED = false, class... Order>   // NFIX: compile-time n (two rows only; svs_capi.hip instantiates the GUI's default 10)
__global__ __launch_bounds__(SVS_WG) void embed_kernel(const uint8_t *gray, uint8_t *stego, const Geometry g, const QimParams qp,
                                                    const uint32_t *__restrict__ bits, const uint64_t bit_offset,
                                                    const uint64_t n_bits, const uint32_t n_words SVS_REPLAY_COUNTER_PARAM,
                                                    const Order... order) {
    static_assert(sizeof...(Order) == (KEYED ? 1u : 0u), "KEYED instantiations take one BlockOrderArgs");
    static_assert(U == 2, "n = 8..15 (svs_capi.hip: one coefficient row runs embed_row1_kernel, more rows embed_exact_kernel in every mode)");
    static_assert(BPL == 1, "one block per lane (see extract_kernel)");
    constexpr bool PARKED = QM != QM_POW2;
    // PARKED: per wave 64 slots of original rows + the worklist words; otherwise the worklist entries carry the rows
    __shared__ __attribute__((aligned(16))) uint32_t park[PARKED ? SVS_WG / 64 : 1][PARKED ? 64 * SVS_SLOT_DWORDS : 2];
    __shared__ u32x2 meta[PARKED ? SVS_WG / 64 : 1][PARKED ? 64 : 1];
    __shared__ GuardEntry entries[PARKED ? 1 : SVS_WG / 64][PARKED ? 1 : SVS_GUARD_CAP];
    __shared__ float tiles[SVS_WG / 64][8 * SVS_GUARD_TILE];
    // SVS_NEAREST, SVS_MINMOVE: ONE wave-uniform branch around the whole body, the rule a compile-time constant on every side
    // (QimRule).  A `return` inside the body leaves the body, and nothing follows the calls.
    const auto body = [&](const QimRule qp) __attribute__((always_inline)) {
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        // (Round 5 tried block-row aligned tiles - a workgroup reads and writes ONE contiguous stretch, eight full pixel rows, at
        // the price of idle lanes - to bring the launch from the rate of a copy with this access pattern to that of a linear copy:
        // 1.73 vs 1.64 ms per 600 x 4K at n = 3, 3.15 vs 2.63 at n = 10, slower on every placement: profiles/r05_ab_row_tiles.txt.)
        // Shadow lanes keep the row registers defined on one path only (round 6: no zero-initialised copies at the joins).
        bool live;
        const uint32_t gblock = shadow_block<1>(tile_id(g.xcd_chunk) * (uint32_t)SVS_WG + threadIdx.x, g, live);
        const uint32_t n = g.n_ac;
        bool und = false, write = false;
        // n <= 15: the payload window of a block is its first word - kept in a register from phase 1, because re-reading it for
        // the worklist is a global load in the life of every wave that replays
        uint32_t hi = 0, nb = 0;
        u32x2 v[8];
        uint32_t ax[8], ay[8];
        const int64_t off = block_offset(gblock, g);
        load_rows<1>(gray + off, g.row_pitch, v);
#pragma unroll
        for (int r = 0; r < 8; ++r) { ax[r] = v[r].x; ay[r] = v[r].y; }
        uint64_t first_keyed = 0;   // KEYED: the slot's first stream bit, computed once
        if constexpr (KEYED) first_keyed = stream_first<true>(gblock, n, g, order_arg(order...));
        if (live) {
            const uint64_t first = KEYED ? first_keyed : (uint64_t)gblock * n;  // stream index of this lane's first bit
            write = stego != gray;                         // past the budget: byte-identical copy (the reference's loops `break`, :130,:132)
            if (first < n_bits) {
                write = true;
                if constexpr (PARKED) {
                    // park the original rows (the exact replay reads them there), then phase 1 in place
                    u32x2 *slot = reinterpret_cast<u32x2 *>(&park[wave][lane * SVS_SLOT_DWORDS]);
#pragma unroll
                    for (int r = 0; r < 8; ++r) slot[r] = v[r];
                    hi = window32(payload_qword(bits, n_words, bit_offset + first), (uint32_t)((bit_offset + first) & 31u));
                    nb = block_budget(first, n_bits, n);
                    und = embed_block_guarded2<QM, NFIX, true>(ax, ay, n, nb, hi, 0u, qp);
                } else {
                    und = guard_phase1<U, QM, NFIX>(ax, ay, n, first, qp, bits, bit_offset, n_bits, n_words, &hi);
                }
            }
        }
        uint32_t redone;
        if constexpr (PARKED) {
            redone = guard_phase2_slots<QM>(&park[wave][0], &meta[wave][0], &tiles[wave][0], lane, n, qp, und, nb, hi, ax, ay);
        } else {
            const GuardPayload pl{bits, bit_offset, n_bits, n_words};
            const uint64_t first = KEYED ? first_keyed : (uint64_t)gblock * n;
            redone = guard_phase2<QM, SVS_GUARD_CAP, true>(&entries[wave][0], &tiles[wave][0], lane, n, qp, pl, und, first, ax, ay, hi);
        }
#if defined(SVS_EXPERIMENTS)
        if (replay_counter != nullptr && redone != 0 && lane == 0) atomicAdd(replay_counter, (unsigned long long)redone);
#else
        (void)redone;
#endif
        if (write) {
#pragma unroll
            for (int r = 0; r < 8; ++r) { v[r].x = ax[r]; v[r].y = ay[r]; }
            store_rows<1>(stego + off, g.row_pitch, v);
        }
    };
    if (g.pad > 1u) body(rule_from_word(qp, g.pad));
    else if (g.pad) body(QimRule(qp, 1u));
    else body(QimRule(qp, 0u));
}

// ---------------------------------------------------------------------------------------
// EMBED, one coefficient row (n <= 7), round 6: the streaming kernel above with the rows kept in ONE representation from
// the load to the store and the cheap result applied in the integer domain (svs_block.hpp, guard_decide_int).
//   * every lane loads (lanes past the end of the batch shadow its last block(s) and never store), so the row registers
//     are defined on one path only: no copies at the joins (round 5: 173 static v_mov_b32, 61 of them on every wave's path);
//   * a decided block costs 16 v_add_u32 instead of 192 conversion / add / saturating-conversion instructions; a WAVE in
//     which some block could clip at 0 / 255 (a wave-uniform ballot) takes a packed 16-bit saturating add for all its
//     lanes - same bytes, 10 instructions per row dword;
//   * the worklist deposit / collection moves rows as the 8-byte pairs they are held in.
// Phases 2 and 3 as in embed_kernel.  gray and stego may alias.
// ---------------------------------------------------------------------------------------
// Rows stay in the load / store vectors: block A = components x, y of v[r], block B (two blocks per lane) = z, w.
template <int BPL>
__device__ __forceinline__ void row1_block(const typename RowVec<BPL>::type (&v)[8], int which, uint32_t (&rx)[8], uint32_t (&ry)[8]) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        if constexpr (BPL == 2) { rx[r] = which ? v[r].z : v[r].x; ry[r] = which ? v[r].w : v[r].y; }
        else { rx[r] = v[r].x; ry[r] = v[r].y; }
    }
}
// worklist deposit / collection of one block's rows as the 8-byte halves of the row vectors they live in (volatile: the
// load / store vectoriser would otherwise pair rows into 16-byte LDS accesses and gather their operands with v_mov)
typedef __attribute__((address_space(3))) volatile u32x2 lds_v64;
template <int BPL>
__device__ __forceinline__ void row1_deposit(GuardEntry *e, const typename RowVec<BPL>::type (&v)[8], int which) {
    lds_v64 *px = (lds_v64 *)(e->px);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        u32x2 t;
        if constexpr (BPL == 2) { if (which) { t.x = v[r].z; t.y = v[r].w; } else { t.x = v[r].x; t.y = v[r].y; } }
        else { t.x = v[r].x; t.y = v[r].y; }
        px[r] = t;
    }
}
template <int BPL>
__device__ __forceinline__ void row1_collect(const GuardEntry *e, typename RowVec<BPL>::type (&v)[8], int which) {
    const lds_v64 *px = (const lds_v64 *)(e->px);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const u32x2 t = px[r];
        if constexpr (BPL == 2) { if (which) { v[r].z = t.x; v[r].w = t.y; } else { v[r].x = t.x; v[r].y = t.y; } }
        else { v[r].x = t.x; v[r].y = t.y; }
    }
}

// phase 2 of the one-row kernel: guard_phase2 on the row vectors, one or two blocks per lane (the payload windows are kept
// from phase 1)
template <int QM, int BPL, int CAP, bool KEYED = false>   // KEYED: block B's first stream bit is first_b, not first_a + n
__device__ __forceinline__ uint32_t row1_phase2(GuardEntry *entries, float *tile, uint32_t lane, uint32_t n, const QimRule &qp,
                                                uint64_t n_bits, bool und_a, bool und_b, uint64_t first_a, uint64_t first_b, uint32_t hi_a,
                                                uint32_t hi_b, typename RowVec<BPL>::type (&v)[8]) {
    bool und[BPL];
    und[0] = und_a;
    if constexpr (BPL == 2) und[1] = und_b;
    return wave_worklist<CAP>(
        und, lane,
        [&](int j, uint32_t i) {
            GuardEntry *e = &entries[i];
            row1_deposit<BPL>(e, v, j);
            e->hi = j ? hi_b : hi_a; e->lo = 0u;
            e->nb = block_budget(j ? (KEYED ? first_b : first_a + n) : first_a, n_bits, n);
        },
        [&](uint32_t i, uint32_t grp, uint32_t r) {
            GuardEntry *e = &entries[i];
            guard_replay8<QM, 1>(e->px, e->hi, e->lo, e->nb, tile + grp * SVS_GUARD_TILE, r, n, qp);
        },
        [&](int j, uint32_t i) { row1_collect<BPL>(&entries[i], v, j); });
}

// what the lanes of a launch share (kernel arguments, in SGPRs)
struct Row1Args {
    const uint8_t *gray;
    uint8_t *stego;
    const uint32_t *bits;
    uint64_t bit_offset, n_bits;
    uint32_t n_words;
};

// The stream positions of a lane's block(s): unkeyed, block B follows block A in the stream and both windows come from A's
// payload qword; keyed, each block has its own slot and its own qword.  A keyed block past the budget is left as it is
// (the reference's loops `break` before its slot) - it never reaches the arithmetic.
struct Row1Slots {
    uint64_t first_a, first_b;
    uint64_t q_b;
};

// phases 1-3 for the rows `v` of global block(s) gb (already loaded from gray + off): decide / apply, exact replay of the
// wave's undecided blocks, store.
template <int QM, int BPL, bool KEYED = false>
__device__ __forceinline__ uint32_t row1_process(typename RowVec<BPL>::type (&v)[8], uint32_t gb, bool live, int64_t off, uint64_t q,
                                                 const Geometry &g, const QimRule &qp, const Row1Args &a, GuardEntry *entries,
                                                 float *tile, uint32_t lane, const Row1Slots &ks = Row1Slots{}) {
    const uint32_t n = g.n_ac;
    const uint64_t first = KEYED ? ks.first_a : (uint64_t)gb * n;   // stream index of this lane's first bit
    const uint64_t first_b = ks.first_b;   // KEYED only (unkeyed: first + n, formed where it is used)
    const bool has_a = !KEYED || first < a.n_bits, has_b = BPL == 2 && (!KEYED || first_b < a.n_bits);
    bool und_a = false, und_b = false, clip = false;
    uint32_t hi_a = 0, hi_b = 0;
    ColumnDeltas ca = {0u, 0u, 0u, 0u}, cb = {0u, 0u, 0u, 0u};
    if (live && (KEYED ? (has_a || has_b) : first < a.n_bits)) {
        const uint32_t sh = (uint32_t)((a.bit_offset + first) & 31u);
        hi_a = window32(q, sh);
        uint32_t flags = 0;
        if (has_a) {
            uint32_t rx[8], ry[8];
            row1_block<BPL>(v, 0, rx, ry);
            flags = guard_decide_int<QM>(rx, ry, n, block_budget(first, a.n_bits, n), hi_a, qp, ca);
            und_a = (flags & SVS_ROW1_UNDECIDED) != 0;
            if (und_a) { ca.e_lo = 0u; ca.o_lo = 0u; ca.e_hi = 0u; ca.o_hi = 0u; }   // keeps its original pixels for the replay
        }
        clip = flags == SVS_ROW1_MAY_CLIP;
        if constexpr (BPL == 2) {
            SVS_SCHED_FENCE();   // one block at a time
            hi_b = KEYED ? window32(ks.q_b, (uint32_t)((a.bit_offset + first_b) & 31u)) : window32(q, sh + n);
        }
        if (BPL == 2 && has_b) {
            uint32_t rx[8], ry[8];
            row1_block<BPL>(v, 1, rx, ry);
            // a budget of 0 (only the lane the payload ends in can see it) leaves block B as it is: all its deltas are 0
            flags = guard_decide_int<QM>(rx, ry, n, block_budget(KEYED ? first_b : first + n, a.n_bits, n), hi_b, qp, cb);
            und_b = (flags & SVS_ROW1_UNDECIDED) != 0;
            if (und_b) { cb.e_lo = 0u; cb.o_lo = 0u; cb.e_hi = 0u; cb.o_hi = 0u; }
            clip = clip || flags == SVS_ROW1_MAY_CLIP;
        }
    }
    SVS_SCHED_FENCE();
    // The stores (every lane: the deltas of a lane without payload are 0).  Wave-uniform: when some block of the wave could
    // clip at 0 / 255, all of them take the saturating form - same bytes where nothing clips.
    const bool clip_wave = __ballot(clip) != 0;
    {
        const uint32_t keep = clip_wave ? 0u : 0xffffffffu;
        const uint32_t a0 = packed_addend(ca.e_lo, ca.o_lo) & keep, a1 = packed_addend(ca.e_hi, ca.o_hi) & keep;
        const uint32_t b0 = packed_addend(cb.e_lo, cb.o_lo) & keep, b1 = packed_addend(cb.e_hi, cb.o_hi) & keep;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            v[r].x += a0; v[r].y += a1;
            if constexpr (BPL == 2) { v[r].z += b0; v[r].w += b1; }
        }
    }
    if (clip_wave) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            v[r].x = add_clip_dword(v[r].x, ca.e_lo, ca.o_lo);
            v[r].y = add_clip_dword(v[r].y, ca.e_hi, ca.o_hi);
            if constexpr (BPL == 2) {
                v[r].z = add_clip_dword(v[r].z, cb.e_lo, cb.o_lo);
                v[r].w = add_clip_dword(v[r].w, cb.e_hi, cb.o_hi);
            }
            SVS_SCHED_FENCE();   // row by row: scheduled for latency, this rare path would set the kernel's register count
        }
    }
    const uint32_t redone = row1_phase2<QM, BPL, SVS_GUARD_CAP, KEYED>(entries, tile, lane, n, qp, a.n_bits, und_a, und_b, first,
                                                                       first_b, hi_a, hi_b, v);
    // past the budget: byte-identical copy (the reference's loops `break`, :130,:132)
    if (live && (a.stego != a.gray || (KEYED ? has_a || has_b : first < a.n_bits))) store_rows<BPL>(a.stego + off, g.row_pitch, v);
    return redone;
}

// static LDS of embed_row1_kernel: each wave's worklist and transposition tile.  The host sizes the kernel's occupancy cap on
// it (svs_capi.hip, lds_pad_for).
typedef GuardEntry Row1Entries[SVS_WG / 64][SVS_GUARD_CAP];
typedef float Row1Tiles[SVS_WG / 64][8 * SVS_GUARD_TILE];
constexpr uint32_t kRow1StaticLds = sizeof(Row1Entries) + sizeof(Row1Tiles);

template <int QM, int BPL, bool KEYED = false, class... Order>
__global__ __launch_bounds__(SVS_WG) void embed_row1_kernel(const uint8_t *gray, uint8_t *stego, const Geometry g,
                                                          const QimParams qp, const uint32_t *__restrict__ bits,
                                                          const uint64_t bit_offset, const uint64_t n_bits,
                                                          const uint32_t n_words SVS_REPLAY_COUNTER_PARAM, const Order... order) {
    static_assert(sizeof...(Order) == (KEYED ? 1u : 0u), "KEYED instantiations take one BlockOrderArgs");
    __shared__ Row1Entries entries;
    __shared__ Row1Tiles tiles;
    // SVS_NEAREST, SVS_MINMOVE: ONE wave-uniform branch around the whole body, the rule a compile-time constant on every side
    // (QimRule).  A `return` inside the body leaves the body, and nothing follows the calls.
    const auto body = [&](const QimRule qp) __attribute__((always_inline)) {
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        bool live;
        const uint32_t gb = shadow_block<BPL>((tile_id(g.xcd_chunk) * (uint32_t)SVS_WG + threadIdx.x) * BPL, g, live);
        const int64_t off = block_offset(gb, g);
        typename RowVec<BPL>::type v[8];
        load_rows<BPL>(gray + off, g.row_pitch, v);
        const Row1Args a{gray, stego, bits, bit_offset, n_bits, n_words};
        const uint32_t n = g.n_ac;
        uint64_t q = 0;
        uint32_t redone;
        if constexpr (KEYED) {   // two blocks per lane: two qword reads, one per slot
            Row1Slots ks{0, 0, 0};
            ks.first_a = stream_first<true>(gb, n, g, order_arg(order...), BPL == 2 ? &ks.first_b : nullptr);
            if (live && ks.first_a < n_bits) q = payload_qword(bits, n_words, bit_offset + ks.first_a);
            if (BPL == 2 && live && ks.first_b < n_bits) ks.q_b = payload_qword(bits, n_words, bit_offset + ks.first_b);
            redone = row1_process<QM, BPL, true>(v, gb, live, off, q, g, qp, a, &entries[wave][0], &tiles[wave][0], lane, ks);
        } else {
            if (live && (uint64_t)gb * n < n_bits) q = payload_qword(bits, n_words, bit_offset + (uint64_t)gb * n);
            redone = row1_process<QM, BPL>(v, gb, live, off, q, g, qp, a, &entries[wave][0], &tiles[wave][0], lane);
        }
#if defined(SVS_EXPERIMENTS)
        if (replay_counter != nullptr && redone != 0 && lane == 0) atomicAdd(replay_counter, (unsigned long long)redone);
#else
        (void)redone;
#endif
    };
    if (g.pad > 1u) body(rule_from_word(qp, g.pad));
    else if (g.pad) body(QimRule(qp, 1u));
    else body(QimRule(qp, 0u));
}

// (Round 6 also ran this kernel as a PERSISTENT, software-pipelined loop - few workgroups per CU, each loading the rows of its
// next tile before it computes on the current one, so that the bytes in flight stay low and constant: correct, and slower on
// every placement, 1.77 - 1.95 ms per 600 x 4K against 1.58 - 1.62, even with the arithmetic skipped: profiles/r06_stream_pipeline.txt.
// What the one-shot launch has and the loop has not is the hardware's own pacing: a workgroup starts when another one ends.)

// Tail of the soft side of extract_exact_kernel: a wave's tile holds the n bytes of each of its `blocks` live blocks, block j
// (lane j) at byte j n.  Without an order they are one run of blocks * n bytes of the output at `run0` (a multiple of
// 64: the output is dword aligned), copied as dwords with a byte tail; with one, block j owns the n bytes at its own
// first_j, copied bytewise - byte t of the tile belongs to block t / n ((t * recip) >> 20, SoftArgs) and goes to
// first_j + t % n.  Every byte of the output has one writer; nothing at or past out_bytes (the call's capacity) is written.
template <bool KEYED>
__device__ __forceinline__ void copy_soft_run(const uint8_t *tile, uint32_t lane, uint32_t n, uint32_t blocks, uint64_t run0,
                                              uint64_t first, uint32_t recip, uint8_t *__restrict__ out, uint64_t out_bytes) {
    const uint32_t bytes = blocks * n;
    if constexpr (!KEYED) {
        const uint32_t *words = reinterpret_cast<const uint32_t *>(tile);
        for (uint32_t w = lane; 4u * w < bytes; w += 64u) {
            const uint64_t at = run0 + 4ull * w;
            if (4u * w + 4u <= bytes && at + 4u <= out_bytes) {
                *reinterpret_cast<uint32_t *>(out + at) = words[w];
            } else {
                for (uint32_t j = 4u * w; j < bytes && run0 + j < out_bytes; ++j) out[run0 + j] = tile[j];
            }
        }
    } else {
        const uint32_t f_lo = (uint32_t)first, f_hi = (uint32_t)(first >> 32);
        for (uint32_t t0 = 0; t0 < bytes; t0 += 64u) {   // wave-uniform trip count: the shuffles run with every lane on
            const uint32_t t = t0 + lane;
            const uint32_t j = min((t * recip) >> 20, 63u);
            const uint64_t at = (((uint64_t)(uint32_t)__shfl((int)f_hi, (int)j) << 32) | (uint32_t)__shfl((int)f_lo, (int)j)) + (t - j * n);
            if (t < bytes && at < out_bytes) out[at] = tile[t];
        }
    }
}

// The vote tail of the soft side (SoftArgs::vote; svs_soft_vote*): the tile as copy_soft_run finds it, but no byte is written -
// byte t, call-local stream bit i (run0 + t without an order, first_j + t % n with one), adds vote_of(byte, i < head) to
// tally[(base + i) mod period] with a global int32 atomic whose result nobody reads.  Integer sums: the order of the adds
// does not matter.  The residue of the run's (the block's) first byte is taken once in 64 bits (vote_residue); from there a
// byte is one conditional subtract away.  Where one wave would hit an entry many times it sums first: without an order and
// period < the run's bytes, lane j walks the tile bytes of residues j, j + 64, .. (stride period) and issues one add each;
// with an order and period <= 64, lane j < period sums residue j over every block.  The tile is wave-private: no barrier
// beyond the caller's wave_lds_fence.  Nothing outside the tally's out_bytes = 4 period bytes is touched.
template <bool KEYED>
__device__ __forceinline__ void vote_soft_run(const uint8_t *tile, uint32_t lane, uint32_t n, uint32_t blocks, uint64_t run0,
                                              uint64_t first, const SoftArgs &sa, int32_t *__restrict__ tally, uint64_t out_bytes) {
    const uint32_t bytes = blocks * n;
    const uint64_t period = sa.period;
    if (bytes == 0u) return;   // wave-uniform
    if constexpr (!KEYED) {
        const uint64_t r0 = vote_residue(run0, sa);   // wave-uniform
        if (period < bytes) {                         // wave-uniform; period < 64 n <= 4032
            const uint32_t p = (uint32_t)period, r = (uint32_t)r0;
            for (uint32_t j = lane; j < p; j += 64u) {
                int32_t sum = 0;
                for (uint32_t t = j >= r ? j - r : j + p - r; t < bytes; t += p) sum += vote_of(tile[t], run0 + t < sa.head);
                if (4ull * j + 4u <= out_bytes) (void)atomicAdd(tally + j, sum);
            }
        } else {
            for (uint32_t t = lane; t < bytes; t += 64u) {
                uint64_t j = r0 + t;                  // t < bytes <= period
                if (j >= period) j -= period;
                if (4u * j + 4u <= out_bytes) (void)atomicAdd(tally + j, vote_of(tile[t], run0 + t < sa.head));
            }
        }
    } else {
        // per lane, of its own block: the residue of the first byte and how many of its leading bytes lie in copy 0
        const uint64_t res = vote_residue(first, sa);
        const uint32_t r_lo = (uint32_t)res, r_hi = (uint32_t)(res >> 32);
        const uint32_t lead = first < sa.head ? (sa.head - first < n ? (uint32_t)(sa.head - first) : n) : 0u;
        if (period <= 64u) {                          // wave-uniform
            const uint32_t p = (uint32_t)period;
            int32_t sum = 0;
            for (uint32_t j = 0; j < blocks; ++j) {   // wave-uniform trip count: the shuffles run with every lane on
                const uint32_t r = (uint32_t)__shfl((int)r_lo, (int)j), lead_j = (uint32_t)__shfl((int)lead, (int)j);
                // lanes at or past the period sum bytes of the tile too and drop the sum
                for (uint32_t s = lane >= r ? lane - r : lane + p - r; s < n; s += p) sum += vote_of(tile[j * n + s], s < lead_j);
            }
            if (lane < p && 4u * lane + 4u <= out_bytes) (void)atomicAdd(tally + lane, sum);
        } else {
            for (uint32_t t0 = 0; t0 < bytes; t0 += 64u) {   // wave-uniform trip count, as copy_soft_run
                const uint32_t t = t0 + lane;
                const uint32_t j = min((t * sa.recip) >> 20, 63u), s = t - j * n;
                uint64_t at = (((uint64_t)(uint32_t)__shfl((int)r_hi, (int)j) << 32) | (uint32_t)__shfl((int)r_lo, (int)j)) + s;
                const uint32_t lead_j = (uint32_t)__shfl((int)lead, (int)j);
                if (at >= period) at -= period;       // s < n <= 63 < period
                if (t < bytes && 4u * at + 4u <= out_bytes) (void)atomicAdd(tally + at, vote_of(tile[t], s < lead_j));
            }
        }
    }
}

// The histogram tail of the soft side (SoftArgs::hist; svs_soft_histogram*; the instantiations without an order only): the tiles
// as copy_soft_run finds them, but no byte is written - each is counted into hist[frame * 256 + byte], a row of 256 uint32 per
// frame.  The workgroup shares ONE table of 256 LDS counters (`table`: behind the tiles, requested by this launch only) and
// walks the frames its SVS_WG blocks touch - fast_div by blocks per frame, as block_offset: one frame at 4K, 256 at one block a
// frame - with a workgroup-uniform trip count.  Per frame: every wave adds the bytes of its own part of the frame (frame_run,
// svs_index.hpp) with one LDS atomic each - the tile is wave-private, the table is not: barriers -, then thread v flushes
// entry v with ONE global atomic whose result nobody reads, skipped where the entry is 0, and clears it for the next frame.
// (Counting the bytes equal to the first pending lane's by a ballot before the atomics, to spare the LDS the serialised adds to
// a hot entry, measured slower on noise and on stego alike, and a table per wave - fences instead of barriers, four times the
// flushes - 25 to 31 % slower on noise at n <= 10: profiles/soft_histogram_variants.txt.)  Integer counting: the order of the
// adds does not matter.  Nothing outside the out_bytes = 1024 n_frames bytes of `hist` is touched.
__device__ __forceinline__ void hist_soft_run(const uint8_t *tile, uint32_t *table, uint32_t lane, uint32_t n, uint32_t blocks,
                                              uint32_t wave_first, uint32_t wg_first, const Geometry &g,
                                              uint32_t *__restrict__ hist, uint64_t out_bytes) {
    static_assert(SVS_WG == (int)kHistBins, "thread v of the workgroup owns entry v of the table");
    const uint32_t wg_blocks = wg_first < g.total_blocks ? min((uint32_t)SVS_WG, g.total_blocks - wg_first) : 0u;
    if (wg_blocks == 0u) return;   // workgroup-uniform: no barrier is left waiting
    const uint32_t bpf = g.by_bpf.div;
    const uint32_t f_first = fast_div(wg_first, g.by_bpf), f_last = fast_div(wg_first + wg_blocks - 1u, g.by_bpf);
    table[threadIdx.x] = 0u;
    for (uint32_t f = f_first; f <= f_last; ++f) {   // workgroup-uniform
        __syncthreads();                             // the table is clear
        uint32_t begin, end;
        frame_run(wave_first, blocks, f, bpf, &begin, &end);
        const uint32_t t_end = end * n;
        for (uint32_t t = begin * n + lane; t < t_end; t += 64u) (void)atomicAdd(&table[tile[t]], 1u);
        __syncthreads();                             // every wave's counts of frame f are in
        const uint32_t c = table[threadIdx.x];
        table[threadIdx.x] = 0u;
        const uint64_t at = (uint64_t)f * kHistBins + threadIdx.x;
        if (c != 0u && 4u * at + 4u <= out_bytes) (void)atomicAdd(hist + at, c);
    }
}

// The eight-row instantiations are register-allocated for the six waves per SIMD they ran at before the dithered side joined
// them (75 - 80 VGPRs; each side fits on its own, left alone the allocator takes 81 - 85 for the pair); a minimum of 1 is the
// default of the others.
template <int U, int QM, int BPL = 1, bool KEYED = false, class... Order>   // BPL: see extract_kernel
__global__ __launch_bounds__(SVS_WG, U == 8 ? 6 : 1) void extract_exact_kernel(const uint8_t *__restrict__ gray, const Geometry g,
                                                            const QimParams qp, uint8_t *__restrict__ out,
                                                            const uint64_t out_bytes, const CoeffTable sel,
                                                            const DitherArgs dith, const SoftArgs soft, const StepArgs steps,
                                                            const Order... order) {
    static_assert(BPL == 1, "one block per lane");
    static_assert(sizeof...(Order) == (KEYED ? 1u : 0u), "KEYED instantiations take one BlockOrderArgs");
    __shared__ uint32_t flags[SVS_WG / 64][SVS_WAVE_BITS_DWORDS(1)];
    // A soft call (soft.on; the U = 8 instantiations only - svs_route.hpp plans no other for one) is a third side behind the
    // same kind of branch: one byte per payload coefficient instead of one bit (svs_block.hpp, SoftArgs).  It takes its wave
    // tiles from dynamic LDS, which only the soft launch requests (soft_lds_bytes), and touches neither `flags` nor `sel`.
    // Per-coefficient steps under a soft call (soft.on && steps.on; svs_stepped_soft_*) are the same side with the stepped byte in
    // the bytes' places (svs_block.hpp extract_block_stepped_soft), compiled into the two QM_POW2 instantiations that hold the
    // stepped side (below) behind ONE wave-uniform branch around the whole side, tails included: as an alternative beside
    // extract_block_soft that shares the loads and the tails it spilled 75 VGPRs (profiles/stepped_soft_resources.txt).
    if constexpr (U == 8) {
        const auto soft_side = [&](auto stepped) __attribute__((always_inline)) {
            extern __shared__ uint32_t soft_tiles[];
            // the wave index as a scalar: with it in a vector register the keyed instantiations, at their bound of 80, spilled
            // the thread index across the block body once the vote tail joined (profiles/soft_vote_resources.txt)
            const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
            const uint32_t n = g.n_ac;   // == dith.sel.count
            const uint32_t wave_first = tile_id(g.xcd_chunk) * (uint32_t)SVS_WG + wave * 64u;
            const uint32_t gblock = wave_first + lane;
            uint8_t *tile = reinterpret_cast<uint8_t *>(soft_tiles) + wave * 64u * n;   // 64 n bytes: dword aligned
            const bool live = gblock < g.total_blocks;
            uint64_t first = 0;
            if (live) {
                u32x2 v[8];
                load_rows<1>(gray + block_offset(gblock, g), g.row_pitch, v);
                uint32_t ax[8], ay[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) { ax[r] = v[r].x; ay[r] = v[r].y; }
                uint8_t *mine = tile + lane * n;
                const uint32_t s_b = dith.on ? dither_seed_of(gblock, g, dith) : 0u;
                const auto put = [&](uint32_t s, uint32_t byte) { mine[s] = (uint8_t)byte; };
                if constexpr (decltype(stepped)::value) extract_block_stepped_soft(ax, ay, dith.sel, steps, dith.on != 0u, s_b, put);
                else extract_block_soft<QM>(ax, ay, dith.sel, qp, soft, dith.on != 0u, s_b, put);
                if constexpr (KEYED) first = stream_first<true>(gblock, n, g, order_arg(order...));
            }
            wave_lds_fence();
            const uint32_t blocks = wave_first < g.total_blocks ? min(64u, g.total_blocks - wave_first) : 0u;
            if constexpr (!KEYED) {
                if (soft.hist) {   // wave-uniform: `out` is the rows of a histogram call, out_bytes their 1024 n_frames bytes
                    hist_soft_run(tile, soft_tiles + (SVS_WG / 64) * 16u * n, lane, n, blocks, wave_first, wave_first - wave * 64u, g,
                                  reinterpret_cast<uint32_t *>(out), out_bytes);
                    return;
                }
            }
            if (soft.vote)     // wave-uniform: `out` is the tally of a vote call, out_bytes its 4 period bytes
                vote_soft_run<KEYED>(tile, lane, n, blocks, (uint64_t)wave_first * n, first, soft, reinterpret_cast<int32_t *>(out),
                                     out_bytes);
            else
                copy_soft_run<KEYED>(tile, lane, n, blocks, (uint64_t)wave_first * n, first, soft.recip, out, out_bytes);
        };
        if (soft.on) {     // wave-uniform
            if constexpr (QM == QM_POW2) {
                // the side that was there first comes first: with the stepped one ahead of it the keyed instantiation spilled
                // two registers on the side that was there before (profiles/stepped_soft_resources.txt)
                if (!steps.on) {   // wave-uniform
                    soft_side(std::false_type{});
                    return;
                }
                soft_side(std::true_type{});
                return;
            }
            soft_side(std::false_type{});
            return;
        }
    }
    // A keyed dither (dith.on; the U = 8 instantiations only - svs_route.hpp plans no other for one): ONE wave-uniform branch
    // around the whole body, as in embed_exact_kernel; `dithered` is a compile-time false on the side that was there before.
    // (The dithered forms as two more alternatives beside the selection's branch, sharing the loads and the tail, took 136
    // instead of 77 VGPRs and three waves per SIMD from the calls without a dither.)
    // Per-coefficient steps (steps.on; svs_stepped_extract_dev) are one more such side, compiled into the two eight-row QM_POW2
    // instantiations alone (svs_route.hpp plans no other for a stepped call; the GUI's delta = 20 runs the QM_F32 ones).  Its
    // table is `sel`, never empty: the call's selection or the prefix table of n_ac.
    const auto body = [&](auto dithered, auto stepped) __attribute__((always_inline)) {
        constexpr bool DITH = decltype(dithered)::value;
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        const uint32_t tile = tile_id(g.xcd_chunk);
        const uint32_t gblock = tile * (uint32_t)SVS_WG + threadIdx.x;
        const uint32_t n = g.n_ac;
        uint32_t hi = 0, lo = 0;
        if (gblock < g.total_blocks) {
            u32x2 v[8];
            load_rows<1>(gray + block_offset(gblock, g), g.row_pitch, v);
            uint32_t ax[8], ay[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) { ax[r] = v[r].x; ay[r] = v[r].y; }
            // a coefficient selection (U = 8 only; n == sel.count): one wave-uniform branch around the block's arithmetic
            bool selected = false;
            if constexpr (U == 8) selected = sel.count != 0;
            if constexpr (decltype(stepped)::value) {
                uint32_t s_b = 0u;
                if constexpr (DITH) s_b = dither_seed_of(gblock, g, dith);
                extract_block_stepped<DITH>(ax, ay, sel, steps, hi, lo, s_b);
                // a matrix call (svs_matrix_extract_dev): the block's n = g.n_ac stream bits are the syndrome of its parities
                if (steps.matrix()) matrix_fold(hi, lo);   // wave-uniform
            } else if constexpr (DITH) {
                // the prefix form and the selected form, as on the side without a dither
                const uint32_t s_b = dither_seed_of(gblock, g, dith);
                if (selected) extract_block_exact_selected<QM, true>(ax, ay, sel, qp, hi, lo, s_b);
                else extract_block_exact<U, QM, true>(ax, ay, n, qp, hi, lo, s_b);
            } else {
                if (selected) extract_block_exact_selected<QM>(ax, ay, sel, qp, hi, lo);
                else extract_block_exact<U, QM>(ax, ay, n, qp, hi, lo);
            }
            if constexpr (KEYED) or_bits_global<U>(out, stream_first<true>(gblock, n, g, order_arg(order...)), hi, lo);
        }
        if constexpr (!KEYED)
            emit_wave_bits<U, 1>(&flags[wave][0], lane, (uint64_t)tile * (uint32_t)SVS_WG + wave * 64u, n, hi, lo, 0u, 0u, out, out_bytes);
    };
    if constexpr (U == 8 && QM == QM_POW2) {
        if (steps.on) {    // wave-uniform
            if (dith.on) body(std::true_type{}, std::true_type{});
            else body(std::false_type{}, std::true_type{});
            return;
        }
    }
    if constexpr (U == 8) {
        if (dith.on) {     // wave-uniform
            body(std::true_type{}, std::false_type{});
            return;
        }
    }
    body(std::false_type{}, std::false_type{});
}

// ---------------------------------------------------------------------------------------
// Interleaved BGR rows (the colour plumbing further down, and the colour form of the read-back pass)
// ---------------------------------------------------------------------------------------
struct ColourParams {
    int64_t in_row_pitch, in_frame_pitch;    // BGR input
    int64_t out_row_pitch, out_frame_pitch;  // BGR output
    uint32_t wb, wg, wr, shift;              // (B*wb + G*wg + R*wr + 2^(shift-1)) >> shift
};

// block_offset_bgr(gblock, g, row_pitch, frame_pitch): svs_index.hpp

// One block row of interleaved BGR = 24 bytes at an 8-byte aligned address: three 8-byte accesses.  (A 16-byte +
// an 8-byte access is no faster for loads and 1.7x SLOWER for stores - the 16-byte half is misaligned half the time.)
__device__ __forceinline__ void load_bgr_row(const uint8_t *p, u32x2 &q0, u32x2 &q1, u32x2 &q2) {
    const u32x2 *row = reinterpret_cast<const u32x2 *>(p);
    q0 = SVS_LD(row); q1 = SVS_LD(row + 1); q2 = SVS_LD(row + 2);
}
__device__ __forceinline__ void store_bgr_row(uint8_t *p, const u32x2 &q0, const u32x2 &q1, const u32x2 &q2) {
    u32x2 *row = reinterpret_cast<u32x2 *>(p);
    SVS_ST(q0, row); SVS_ST(q1, row + 1); SVS_ST(q2, row + 2);
}

// 8 interleaved BGR pixels (6 dwords) -> 8 gray bytes (2 dwords)
__device__ __forceinline__ void bgr8_to_gray(const u32x2 &q0, const u32x2 &q1, const u32x2 &q2, const ColourParams &c,
                                             uint32_t &lo4, uint32_t &hi4) {
    const uint32_t w[6] = {q0.x, q0.y, q1.x, q1.y, q2.x, q2.y};
    const uint32_t half = 1u << (c.shift - 1);
    uint32_t px[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int b0 = 3 * j, b1 = 3 * j + 1, b2 = 3 * j + 2;
        const uint32_t B = (w[b0 >> 2] >> (8 * (b0 & 3))) & 0xffu, G = (w[b1 >> 2] >> (8 * (b1 & 3))) & 0xffu,
                       R = (w[b2 >> 2] >> (8 * (b2 & 3))) & 0xffu;
        // B, G, R < 2^8 and the weights <= 2^16: 24-bit multiplies (full rate) are exact
        px[j] = (__umul24(B, c.wb) + __umul24(G, c.wg) + __umul24(R, c.wr) + half) >> c.shift;
    }
    lo4 = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
    hi4 = px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24);
}

// ---------------------------------------------------------------------------------------
// READ-BACK pass (SVS_READBACK, include/svsdct.h): launched on the call's stream after the embed kernel, in place on the
// stego planes.
//   check   one lane per block, each block read once: lanes whose block carries payload bits (the block's slot with a keyed
//           order, as the ordered embed kernels map it) read it back with the exact extraction arithmetic against the same
//           payload words the embed used (svs_readback.hpp readback_block_ok: extract_exact_kernel's forward transform on
//           the payload rows).  A block that reads back is not written.  Waves without a failing block end after a ballot.
//   repair  the wave's failing blocks are compacted into a wave-private LDS worklist (ballot + mbcnt: their rows and
//           payload window, SVS_RB_CAP per round); the whole wave then repairs them eight lanes per block (search8: lane r
//           transforms column r and row r, the block's lines meet in an LDS tile) - eight blocks at a time.  Owners of repaired blocks read
//           the accepted rows back and store them; an unrepaired block is not written (the reference's bytes stay).
// Counts: one 64-bit atomic per wave and kind into counts[0] (repaired) / counts[1] (left unrepaired), NULL for none.
// ---------------------------------------------------------------------------------------
#define SVS_RB_SLOT 16   // dwords of a worklist entry's rows: row y = (dword 2y, dword 2y + 1)
#define SVS_RB_CAP 32    // worklist entries per wave and round (18 KB of LDS per workgroup in all: eight workgroups per CU)

__device__ __forceinline__ uint32_t group8_or(uint32_t v) {
    v |= (uint32_t)__shfl_xor((int)v, 1, 64);
    v |= (uint32_t)__shfl_xor((int)v, 2, 64);
    return v | (uint32_t)__shfl_xor((int)v, 4, 64);
}
__device__ __forceinline__ float group8_min(float v) {
    v = fminf(v, __shfl_xor(v, 1, 64));
    v = fminf(v, __shfl_xor(v, 2, 64));
    return fminf(v, __shfl_xor(v, 4, 64));
}
__device__ __forceinline__ float group8_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 1, 64));
    v = fmaxf(v, __shfl_xor(v, 2, 64));
    return fmaxf(v, __shfl_xor(v, 4, 64));
}

// svs_readback.hpp search_block on eight lanes (r = 0..7) of one worklist entry: px = its rows in LDS (in: the reference's
// stego; out: the last iterate), t = the group's 64-float tile.  The same operations on the same values, so the same bytes;
// true (in all eight lanes) when an iterate was accepted.  The one copy of the loop on the device: `rows` is what a form of
// the pass differs in, lane r's coefficient row of each (svs_readback.hpp's row functions) -
//   targets(c, T)               the row's targets from the block's coefficients
//   correction(T, c, scale, d)  its over-relaxed correction
//   rejects(c)                  non-zero while the row keeps these coefficients from being accepted: the lane's own verdict,
//                               ORed over the group here
// - a small value type (PlainRows, KeyedRows, SteppedRows below), everything inlined.
template <class Rows>
__device__ __forceinline__ bool search8(uint32_t *px, float *t, uint32_t r, const Rows &rows) {
    float c[8], T[8];
    forward8<8>(px, t, r, c);
    rows.targets(c, T);
#pragma unroll 1
    for (int it = 0; it < SVS_READBACK_ITERS; ++it) {
        const float scale = 1.0f + 0.5f * (float)it;
        float d[8], col[8], row[8], y[8];
        rows.correction(T, c, scale, d);
#pragma unroll
        for (int x = 0; x < 8; ++x) t[8 * r + x] = d[x];            // coefficient row r
        wave_lds_fence();
#pragma unroll
        for (int u = 0; u < 8; ++u) col[u] = t[8 * u + r];          // coefficient column r
        wave_lds_fence();
        inverse8<8>(col, t, r, row);                                 // row r of P
        wave_lds_fence();
        float mn = 1e30f, mx = -1e30f;
        repair_add_row(px[2 * r], px[2 * r + 1], row, y, mn, mx);
        const float s = repair_shift(group8_min(mn), group8_max(mx));
        uint32_t lo4, hi4;
        repair_store_row(y, s, lo4, hi4);
        px[2 * r] = lo4;
        px[2 * r + 1] = hi4;
        wave_lds_fence();
        forward8<8>(px, t, r, c);
        if (group8_or(rows.rejects(c)) == 0) return true;
    }
    return false;
}

// does the worklist entry px read back?  Eight lanes: the forward transform and acceptance test of search8, so the verdict is
// readback_block_ok's (the exact read-back) for every number of coefficient rows
template <class Rows>
__device__ __forceinline__ bool reads_back8(const uint32_t *px, float *t, uint32_t r, const Rows &rows) {
    float c[8];
    forward8<8>(px, t, r, c);
    return !group8_or(rows.rejects(c));
}

// an entry that is checked on eight lanes before it is searched: left alone when it reads back, else settled as 1 = repaired or
// 2 = could not be repaired (settle: readback_worklist's)
template <class Rows, class Settle>
__device__ __forceinline__ void check_and_search8(uint32_t *px, float *t, uint32_t r, const Rows &rows, Settle &&settle) {
    if (reads_back8(px, t, r, rows)) return;   // uniform over the entry's eight lanes
    wave_lds_fence();
    settle(search8(px, t, r, rows) ? 1u : 2u);
}

// the gray and the colour form: flat indices 1 .. nb under the call's quantiser
template <int QM>
struct PlainRows {
    uint32_t r, nb, hi, lo;
    const QimParams &qp;
    __device__ __forceinline__ void targets(const float (&c)[8], float (&T)[8]) const { repair_targets_row<QM>(c, (int)r, nb, hi, lo, qp, T); }
    __device__ __forceinline__ void correction(const float (&T)[8], const float (&c)[8], float scale, float (&d)[8]) const {
        repair_correction_row(T, c, (int)r, nb, scale, d);
    }
    __device__ __forceinline__ uint32_t rejects(const float (&c)[8]) const { return row_misses<QM>(c, (int)r, nb, hi, lo, qp) ? 1u : 0u; }
};

// The wave's worklist, every form: wslots / wmeta / wtiles = the wave's part of readback_kernel's three LDS arrays, `wanted` =
// this lane's block enters the worklist, as number `rank` of the wave's `total`.  Rounds of SVS_RB_CAP entries, each in passes
// of eight entries on eight lanes each:
//   deposit(e, m)          the owner fills its entry: e = its SVS_RB_SLOT dwords of rows, m = its meta - x / y = the payload
//                          window, z = nb, w = s_b (0 without a dither)
//   examine(px, t, r, m, settle)   lanes 8 grp .. 8 grp + 7, r = lane & 7, on the entry's rows px with the group's tile t.  An
//                          entry it leaves as it is keeps status 0; one it searched it settles, in all eight lanes, with
//                          settle(1) = px holds the accepted block or settle(2) = searched in vain, kept in the entry as z = nb |
//                          status << 8 - written there, inside the branch that searched, not behind examine
//   store(e)               the owner of an entry with status 1 writes its rows out (wtiles is free between the passes)
// Returns the lane's status (0 for a lane without an entry).
template <class Deposit, class Examine, class Store>
__device__ __forceinline__ uint32_t readback_worklist(uint32_t *wslots, u32x4 *wmeta, float *wtiles, const bool wanted,
                                                      const uint32_t rank, const uint32_t total, Deposit &&deposit,
                                                      Examine &&examine, Store &&store) {
    const uint32_t lane = threadIdx.x & 63u, grp = lane >> 3, r = lane & 7u;
    uint32_t status = 0;
#pragma unroll 1
    for (uint32_t base = 0; base < total; base += SVS_RB_CAP) {   // wave-uniform: rounds of SVS_RB_CAP entries (at most two)
        const bool mine = wanted && rank >= base && rank < base + SVS_RB_CAP;
        if (mine) {
            u32x4 m;
            deposit(wslots + (rank - base) * SVS_RB_SLOT, m);
            wmeta[rank - base] = m;
        }
        wave_lds_fence();
        const uint32_t count = total - base < SVS_RB_CAP ? total - base : SVS_RB_CAP;
#pragma unroll 1
        for (uint32_t at = 0; at < count; at += 8u) {   // wave-uniform: eight entries at a time (at most four passes)
            const uint32_t idx = at + grp;
            if (idx < count) {
                const u32x4 m = wmeta[idx];
                examine(wslots + idx * SVS_RB_SLOT, wtiles + 64 * grp, r, m, [&](uint32_t found) {
                    if (r == 0) wmeta[idx].z = m.z | found << 8;
                });
            }
            wave_lds_fence();
        }
        if (mine) {
            status = wmeta[rank - base].z >> 8;
            if (status == 1) store(wslots + (rank - base) * SVS_RB_SLOT);
        }
        wave_lds_fence();
    }
    return status;
}

// one 64-bit atomic per wave and kind: counts[at] += the wave's lanes with status 1, counts[at + 1] += those with status 2
__device__ __forceinline__ void add_counts(unsigned long long *counts, uint32_t at, uint32_t status) {
    const uint64_t rep = __ballot(status == 1), left = __ballot(status == 2);
    if (counts && (threadIdx.x & 63u) == 0) {
        if (rep) atomicAdd(&counts[at], (unsigned long long)__popcll(rep));
        if (left) atomicAdd(&counts[at + 1], (unsigned long long)__popcll(left));
    }
}

// an entry's meta as its owner deposits it: the payload window that starts at stream bit `at`, nb and s_b
__device__ __forceinline__ u32x4 entry_meta(const uint32_t *__restrict__ bits, uint32_t n_words, uint64_t at, uint32_t nb, uint32_t s_b) {
    u32x4 m; m.z = nb; m.w = s_b;
    uint32_t hi, lo;
    payload_window(bits, n_words, at, hi, lo);
    m.x = hi; m.y = lo;
    return m;
}

// a gray block's rows into its entry, and an accepted entry's rows back over the block
__device__ __forceinline__ void deposit_rows(const uint8_t *src, int64_t row_pitch, uint32_t *e) {
    u32x2 v[8];
    load_rows<1>(src, row_pitch, v);
#pragma unroll
    for (int y = 0; y < 8; ++y) { e[2 * y] = v[y].x; e[2 * y + 1] = v[y].y; }
}
__device__ __forceinline__ void store_entry_rows(const uint32_t *e, uint8_t *dst, int64_t row_pitch) {
    u32x2 v[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) { v[y].x = e[2 * y]; v[y].y = e[2 * y + 1]; }
    store_rows<1>(dst, row_pitch, v);
}

// The colour form (svs_embed_bgr_readback_dev): the same pass in place on the fused colour embed's interleaved BGR output
// (c: its pitches in out_*, the call's weights).  Check and repair work on gray(BGR), the call's fixed-point gray, so they
// are the gray pass's; only the way a block's rows come in and leave differs.  A body of its own behind the kernel's
// wave-uniform `form` argument - no instantiation of its own, and the gray body stays as it was.  Raster order
// only: the colour calls have no keyed order.
//   check   every block that carries payload is deposited in the worklist - its gray rows computed from its 24-byte rows -
//           and read back on eight lanes (reads_back8)
//   repair  the failing entries, as in the gray form
//   store   keep_colour_pixel(P, t') for the pixels whose gray the repair changed, P = the pixel in the buffer, t' = the
//           repaired gray - the other pixels keep their bytes.  After the plain embed P = (g, g, g) and the result is
//           (t', t', t'); after the keep-colour embed it is the cover's colour shifted: one store serves both.
#define SVS_RB_GRAY 0u
#define SVS_RB_BGR 1u
static_assert(64 * 6 <= 8 * 64, "one 24-byte row per lane fits the wave's tiles");

// gray rows of one block from its BGR rows into a worklist entry, a row at a time
__device__ __forceinline__ void deposit_bgr_as_gray(const uint8_t *src, int64_t row_pitch, const ColourParams &c, uint32_t *e) {
#pragma unroll 1
    for (int y = 0; y < 8; ++y) {
        u32x2 q0, q1, q2;
        load_bgr_row(src + (int64_t)y * row_pitch, q0, q1, q2);
        uint32_t lo4, hi4;
        bgr8_to_gray(q0, q1, q2, c, lo4, hi4);
        e[2 * y] = lo4;
        e[2 * y + 1] = hi4;
    }
}

// A repaired block leaves in its colours, a row at a time: the pixels whose gray the repair changed are redone with the exact
// rule (svs_colour.hpp), one at a time through the lane's 24 bytes of LDS (`row`); a row without such a pixel is not written.
__device__ __forceinline__ void store_entry_as_bgr(const uint32_t *e, uint8_t *dst, int64_t row_pitch, const ColourParams &c,
                                                   u32x2 *row) {
#pragma unroll 1
    for (int y = 0; y < 8; ++y) {
        uint8_t *p = dst + (int64_t)y * row_pitch;
        u32x2 q0, q1, q2;
        load_bgr_row(p, q0, q1, q2);
        uint32_t glo, ghi;
        bgr8_to_gray(q0, q1, q2, c, glo, ghi);
        const uint32_t tlo = e[2 * y], thi = e[2 * y + 1];
        const uint32_t xlo = glo ^ tlo, xhi = ghi ^ thi;
        if ((xlo | xhi) == 0u) continue;
        uint32_t todo = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            todo |= ((xlo >> (8 * j)) & 0xffu) ? 1u << j : 0u;
            todo |= ((xhi >> (8 * j)) & 0xffu) ? 1u << (4 + j) : 0u;
        }
        row[0] = q0; row[1] = q1; row[2] = q2;
        uint8_t *pb = reinterpret_cast<uint8_t *>(row);
        while (todo != 0u) {
            const uint32_t i = (uint32_t)__builtin_ctz(todo);
            todo &= todo - 1u;
            uint32_t B = pb[3 * i], G = pb[3 * i + 1], R = pb[3 * i + 2];
            const uint32_t t = ((i < 4 ? tlo : thi) >> (8u * (i & 3u))) & 0xffu;
            keep_colour_pixel(B, G, R, t, c.wb, c.wg, c.wr, c.shift);
            pb[3 * i] = (uint8_t)B; pb[3 * i + 1] = (uint8_t)G; pb[3 * i + 2] = (uint8_t)R;
        }
        store_bgr_row(p, row[0], row[1], row[2]);
    }
}

// Every block that carries payload goes through the worklist and is CHECKED on eight lanes too (reads_back8): the
// lane-per-block check of the gray form, fed from BGR, took up to 132 VGPRs with eight coefficient rows - a wave per SIMD of
// the gray form's - while this body stays within the search's registers; the arithmetic per block is the same sixteen 8-point
// transforms, spread over eight lanes.
template <int QM>
__device__ __forceinline__ void readback_colour(uint32_t *wslots, u32x4 *wmeta, float *wtiles, uint8_t *bgr, const Geometry &g,
                                                const QimParams &qp, const uint32_t *__restrict__ bits, const uint64_t bit_offset,
                                                const uint64_t n_bits, const uint32_t n_words, unsigned long long *counts,
                                                const ColourParams &c) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gblock = tile_id(g.xcd_chunk) * (uint32_t)SVS_WG + threadIdx.x;
    const uint32_t n = g.n_ac;
    uint32_t nb = 0;
    uint64_t first = 0;
    if (gblock < g.total_blocks) {
        first = (uint64_t)gblock * n;
        nb = block_budget(first, n_bits, n);
    }
    const uint64_t mask = __ballot(nb > 0);
    if (mask == 0) return;               // wave-uniform
    const uint32_t total = (uint32_t)__popcll(mask);
    const uint32_t rank = wave_rank(mask);
    int64_t off = 0;
    if (nb > 0) off = block_offset_bgr(gblock, g, c.out_row_pitch, c.out_frame_pitch);
    const uint32_t status = readback_worklist(
        wslots, wmeta, wtiles, nb > 0, rank, total,
        [&](uint32_t *e, u32x4 &m) {
            deposit_bgr_as_gray(bgr + off, c.out_row_pitch, c, e);
            m = entry_meta(bits, n_words, bit_offset + first, nb, 0u);
        },
        [&](uint32_t *px, float *t, uint32_t r, const u32x4 &m, auto settle) {
            check_and_search8(px, t, r, PlainRows<QM>{r, m.z, m.x, m.y, qp}, settle);
        },
        [&](const uint32_t *e) {   // 24 bytes of the tiles per lane
            store_entry_as_bgr(e, bgr + off, c.out_row_pitch, c, reinterpret_cast<u32x2 *>(wtiles) + 3 * lane);
        });
    add_counts(counts, 0u, status);
}

// The keyed form (svs_embed_dithered_readback_dev): the gray pass under a coefficient SELECTION and a keyed DITHER
// (svs_readback.hpp, the keyed forms).  kd.sel = the call's inverse table or the prefix table of n_ac (never empty here), kd.on
// = the dither's switch, a kernel argument and so wave-uniform.  Every block that carries payload goes into the worklist - its
// rows, payload window, nb and s_b - is checked on eight lanes and searched on eight lanes when it fails; the owner stores an
// accepted block, every other block is never written.
//   table   lane r of a group handles flat indices 8r .. 8r + 7 and needs words 2r and 2r + 1 of the inverse table: selected
//           into two registers once (fourteen v_cndmask), never indexed - a per-lane index into a kernel argument is scratch
//   dither  s_b is that of the block's PHYSICAL position (dither_seed_of), per owner lane - a wave can straddle two frames -
//           and travels in the entry; the eight lanes each derive the d of their coefficient row from it once per entry
//   window  that of the block's SLOT: stream_first<true> under an order, gblock * n in raster order (`raster`, wave-uniform)
#define SVS_RB_SEL 4u      // form = SVS_RB_SEL + the call's QuantMode (+ SVS_RB_RASTER: no block order)
#define SVS_RB_RASTER 8u

__device__ __forceinline__ RowSlots row_slots_of_lane(const CoeffTable &t, uint32_t r) {
    RowSlots rs{t.w[0], t.w[1]};
#pragma unroll
    for (int u = 1; u < 8; ++u) {
        rs.w0 = r == (uint32_t)u ? t.w[2 * u] : rs.w0;
        rs.w1 = r == (uint32_t)u ? t.w[2 * u + 1] : rs.w1;
    }
    return rs;
}

template <int QM>
struct KeyedRows {
    const RowSlots &rs;
    uint32_t nb, hi, lo;
    const QimParams &qp;
    bool dith;
    const float (&dv)[8];   // the row's d, all 0 without a dither
    __device__ __forceinline__ void targets(const float (&c)[8], float (&T)[8]) const { keyed_targets_row<QM>(c, rs, nb, hi, lo, qp, dith, dv, T); }
    __device__ __forceinline__ void correction(const float (&T)[8], const float (&c)[8], float scale, float (&d)[8]) const {
        keyed_correction_row(T, c, rs, nb, scale, d);
    }
    __device__ __forceinline__ uint32_t rejects(const float (&c)[8]) const { return keyed_row_misses<QM>(c, rs, nb, hi, lo, qp, dith, dv) ? 1u : 0u; }
};

template <int QM>
__device__ __forceinline__ void readback_keyed(uint32_t *wslots, u32x4 *wmeta, float *wtiles, uint8_t *stego, const Geometry &g,
                                               const QimParams &qp, const uint32_t *__restrict__ bits, const uint64_t bit_offset,
                                               const uint64_t n_bits, const uint32_t n_words, unsigned long long *counts,
                                               const DitherArgs &kd, const bool raster, const BlockOrderArgs &ord) {
    const uint32_t gblock = tile_id(g.xcd_chunk) * (uint32_t)SVS_WG + threadIdx.x;
    const uint32_t n = g.n_ac;
    const bool dith = kd.on != 0u;
    uint32_t nb = 0;
    uint64_t first = 0;
    if (gblock < g.total_blocks) {
        first = raster ? stream_first_raster(gblock, n) : stream_first<true>(gblock, n, g, ord);
        nb = block_budget(first, n_bits, n);
    }
    const uint64_t mask = __ballot(nb > 0);
    if (mask == 0) return;               // wave-uniform
    const uint32_t total = (uint32_t)__popcll(mask);
    const uint32_t rank = wave_rank(mask);
    const RowSlots rs = row_slots_of_lane(kd.sel, threadIdx.x & 7u);
    int64_t off = 0;
    if (nb > 0) off = block_offset(gblock, g);
    const uint32_t status = readback_worklist(
        wslots, wmeta, wtiles, nb > 0, rank, total,
        [&](uint32_t *e, u32x4 &m) {
            deposit_rows(stego + off, g.row_pitch, e);
            m = entry_meta(bits, n_words, bit_offset + first, nb, dith ? dither_seed_of(gblock, g, kd) : 0u);
        },
        [&](uint32_t *px, float *t, uint32_t r, const u32x4 &m, auto settle) {
            float dv[8];
            if (dith) keyed_dither_row(m.w, r, qp.delta_f, dv);
            else {
#pragma unroll
                for (int v = 0; v < 8; ++v) dv[v] = 0.0f;
            }
            check_and_search8(px, t, r, KeyedRows<QM>{rs, m.z, m.x, m.y, qp, dith, dv}, settle);
        },
        [&](const uint32_t *e) { store_entry_rows(e, stego + off, g.row_pitch); });
    add_counts(counts, 0u, status);
}

// The stepped form (svs_stepped_embed_readback_dev): readback_keyed with a step per coefficient (svs_readback.hpp, the stepped
// forms), behind form = SVS_RB_STEP (+ SVS_RB_RASTER).  kd as in the keyed form - its table is never empty -, `steps` the call's
// table, by value.  What differs:
//   steps   lane r of a group needs the steps of flat indices 8r .. 8r + 7, dwords 4r .. 4r + 3 of the table: selected into four
//           registers once (twenty-eight v_cndmask, as row_slots_of_lane selects the inverse table), kept packed and converted
//           where a step is used
//   dither  d is recomputed from the entry's s_b where it is used (svs_readback.hpp), not held in eight registers
// No QimParams is read: the body has no quantiser mode, so it is one body, not three.
#define SVS_RB_STEP 16u

__device__ __forceinline__ RowSteps row_steps_of_lane(const StepArgs &t, uint32_t r) {
    RowSteps st{{t.w[0], t.w[1], t.w[2], t.w[3]}};
#pragma unroll
    for (int u = 1; u < 8; ++u) {
#pragma unroll
        for (int j = 0; j < 4; ++j) st.w[j] = r == (uint32_t)u ? t.w[4 * u + j] : st.w[j];
    }
    return st;
}

// gate (wave-uniform) = 0: the read-back's verdict, bit 0 = the row misses a bit; 1..127: the margin pass's
// (strengthen_block_stepped), SVS_MARGIN_MISS | SVS_MARGIN_WEAK - both as two bits from one row function.
struct SteppedRows {
    const RowSlots &rs;
    const RowSteps &st;
    uint32_t r, nb, hi, lo;
    bool dith;
    uint32_t s_b, gate;
    __device__ __forceinline__ void targets(const float (&c)[8], float (&T)[8]) const { stepped_targets_row(c, rs, st, r, nb, hi, lo, dith, s_b, T); }
    __device__ __forceinline__ void correction(const float (&T)[8], const float (&c)[8], float scale, float (&d)[8]) const {
        keyed_correction_row(T, c, rs, nb, scale, d);
    }
    __device__ __forceinline__ uint32_t rejects(const float (&c)[8]) const {
        // s_b is hidden from the compiler HERE, once per iterate, so that d is recomputed: left to itself it computes the row's
        // eight d ahead of the loop and holds them beside the eight float steps (133 VGPRs instead of 127)
        uint32_t sb = s_b;
        asm volatile("" : "+v"(sb));
        return __builtin_expect(gate != 0u, 0) ? stepped_row_verdict(c, rs, st, r, nb, hi, lo, dith, sb, (float)gate)
                                               : stepped_row_misses(c, rs, st, r, nb, hi, lo, dith, sb) ? 1u : 0u;
    }
};

// GATED false: the read-back - the gate is the constant 0 and every branch on it folds away.  GATED true: the
// margin pass (svs_stepped_embed_readback_margin_dev's second launch; readback_kernel takes it when `steps` carries a gate), the
// same body with the gate read from `steps` and a wave-uniform branch at the check, at the search's acceptance and at the counts.
// Two bodies, so that the read-back's keeps its code; and the gated one branches at run time instead of being a third compiled
// form, because that is what fits: with the gate known to be non-zero the compiler's margin-only body takes 131 VGPRs, with the
// branches kept - the gate hidden from it below - the kernel stays at 128 (profiles/readback_margin_resources.txt).
template <bool GATED>
__device__ __forceinline__ void readback_stepped(uint32_t *wslots, u32x4 *wmeta, float *wtiles, uint8_t *stego, const Geometry &g,
                                                 const uint32_t *__restrict__ bits, const uint64_t bit_offset, const uint64_t n_bits,
                                                 const uint32_t n_words, unsigned long long *counts, const DitherArgs &kd,
                                                 const StepArgs &steps, const bool raster, const BlockOrderArgs &ord) {
    const uint32_t gblock = tile_id(g.xcd_chunk) * (uint32_t)SVS_WG + threadIdx.x;
    const uint32_t n = g.n_ac;
    const bool dith = kd.on != 0u;
    uint32_t gate = 0u;   // wave-uniform, a scalar; 0: the read-back, > 0: the margin pass
    if constexpr (GATED) {
        gate = steps.margin_gate();
        asm volatile("" : "+s"(gate));   // hidden: the caller has tested it, and known non-zero it folds the branches (above)
    }
    uint32_t nb = 0;
    uint64_t first = 0;
    if (gblock < g.total_blocks) {
        first = raster ? stream_first_raster(gblock, n) : stream_first<true>(gblock, n, g, ord);
        nb = block_budget(first, n_bits, n);
    }
    const uint64_t mask = __ballot(nb > 0);
    if (mask == 0) return;               // wave-uniform
    const uint32_t total = (uint32_t)__popcll(mask);
    const uint32_t rank = wave_rank(mask);
    const RowSlots rs = row_slots_of_lane(kd.sel, threadIdx.x & 7u);
    const RowSteps st = row_steps_of_lane(steps, threadIdx.x & 7u);
    int64_t off = 0;
    if (nb > 0) off = block_offset(gblock, g);
    const uint32_t status = readback_worklist(
        wslots, wmeta, wtiles, nb > 0, rank, total,
        [&](uint32_t *e, u32x4 &m) {
            deposit_rows(stego + off, g.row_pitch, e);
            m = entry_meta(bits, n_words, bit_offset + first, nb, dith ? dither_seed_of(gblock, g, kd) : 0u);
        },
        [&](uint32_t *px, float *t, uint32_t r, const u32x4 &m, auto settle) {
            const SteppedRows rows{rs, st, r, m.z, m.x, m.y, dith, m.w, gate};
            float c[8];
            forward8<8>(px, t, r, c);
            // searched (uniform over the eight lanes): the read-back, a block that misses a bit; the margin pass, a block that
            // decodes and has a weak coefficient - one that misses a bit is the read-back's unrepaired block and is left.  (The
            // row functions called here, not rows.rejects: the check needs no hidden s_b.)
            bool search;
            if (__builtin_expect(gate != 0u, 0))
                search = group8_or(stepped_row_verdict(c, rs, st, r, m.z, m.x, m.y, dith, m.w, (float)gate)) == SVS_MARGIN_WEAK;
            else search = group8_or(stepped_row_misses(c, rs, st, r, m.z, m.x, m.y, dith, m.w) ? 1u : 0u) != 0;
            if (!search) return;
            wave_lds_fence();
            settle(search8(px, t, r, rows) ? 1u : 2u);
        },
        [&](const uint32_t *e) { store_entry_rows(e, stego + off, g.row_pitch); });
    add_counts(counts, gate != 0u ? 2u : 0u, status);   // svs_margin_counts: {repaired, unrepaired, strengthened, weak}
}

// form = SVS_RB_GRAY: `stego` = the gray planes of g, c unused.  form = SVS_RB_BGR + the call's QuantMode: `stego` = the BGR
// output, readback_colour - in ONE instantiation only.  The colour body depends on the quantiser mode alone (not on U, and it
// has no order), so all three of its forms live in the instantiation whose gray body leaves the most registers free,
// readback_kernel<8, QM_POW2, true, BlockOrderArgs>, and every colour call launches that one: the other seventeen
// are the gray pass's code as it was.  (The colour body next to the gray one cost every instantiation that held both 2 - 9
// VGPRs, and the eight-row ones with a step that is no power of two a wave per SIMD.)
// form = SVS_RB_SEL + the call's QuantMode (+ SVS_RB_RASTER): the keyed form, readback_keyed, `stego` = the gray planes, kd its
// table and dither.  Its three bodies live in that same instantiation for the same reason: they depend on the quantiser mode
// alone - all eight coefficient rows always, and raster order is a wave-uniform switch in front of the order the KEYED
// instantiation takes - and the eight-row keyed instantiations of the two other modes sit at exactly 128 VGPRs, where any body
// beside the gray one costs a wave per SIMD (profiles/keyed_readback_resources.txt).
// form = SVS_RB_STEP (+ SVS_RB_RASTER): the stepped form, readback_stepped, `stego` = the gray planes, kd its table and dither,
// `steps` the call's per-coefficient steps.  One body - it reads no QimParams - in that same instantiation, behind the sides that
// were there first; the other seventeen carry `steps` unused, as they carry kd (profiles/stepped_readback_resources.txt).
#define SVS_RB_HOSTS_COLOUR(U, QM, KEYED) ((U) == 8 && (QM) == QM_POW2 && (KEYED))
template <int U, int QM, bool KEYED = false, class... Order>
__global__ __launch_bounds__(SVS_WG) void readback_kernel(uint8_t *stego, const Geometry g, const QimParams qp,
                                                         const uint32_t *__restrict__ bits, const uint64_t bit_offset,
                                                         const uint64_t n_bits, const uint32_t n_words,
                                                         unsigned long long *counts, const ColourParams c, const uint32_t form,
                                                         const DitherArgs kd, const StepArgs steps, const Order... order) {
    static_assert(sizeof...(Order) == (KEYED ? 1u : 0u), "KEYED instantiations take one BlockOrderArgs");
    __shared__ uint32_t slots[SVS_WG / 64][SVS_RB_CAP * SVS_RB_SLOT];
    __shared__ u32x4 meta[SVS_WG / 64][SVS_RB_CAP];
    __shared__ float tiles[SVS_WG / 64][8 * 64];
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t *ws = &slots[wave][0];
    u32x4 *wm = &meta[wave][0];
    float *wt = &tiles[wave][0];
    if constexpr (SVS_RB_HOSTS_COLOUR(U, QM, KEYED)) {
        if (form != SVS_RB_GRAY) {   // a kernel argument: wave-uniform; form - SVS_RB_BGR = the call's quantiser mode
            if (form >= SVS_RB_SEL) {    // the keyed form; (form & 3) = the call's quantiser mode
                const bool raster = (form & SVS_RB_RASTER) != 0u;
                if (form >= SVS_RB_STEP) {   // the stepped form: after the sides that were there first; no quantiser mode
                    // wave-uniform: a gate in `steps` makes the launch the margin pass
                    if (steps.margin_gate() != 0u)
                        readback_stepped<true>(ws, wm, wt, stego, g, bits, bit_offset, n_bits, n_words, counts, kd, steps, raster, order...);
                    else
                        readback_stepped<false>(ws, wm, wt, stego, g, bits, bit_offset, n_bits, n_words, counts, kd, steps, raster, order...);
                    return;
                }
                const uint32_t qm = form & 3u;
                if (qm == QM_F32) readback_keyed<QM_F32>(ws, wm, wt, stego, g, qp, bits, bit_offset, n_bits, n_words, counts, kd, raster, order...);
                else if (qm == QM_DOUBLE) readback_keyed<QM_DOUBLE>(ws, wm, wt, stego, g, qp, bits, bit_offset, n_bits, n_words, counts, kd, raster, order...);
                else readback_keyed<QM_POW2>(ws, wm, wt, stego, g, qp, bits, bit_offset, n_bits, n_words, counts, kd, raster, order...);
                return;
            }
            if (form == SVS_RB_BGR + QM_F32) readback_colour<QM_F32>(ws, wm, wt, stego, g, qp, bits, bit_offset, n_bits, n_words, counts, c);
            else if (form == SVS_RB_BGR + QM_DOUBLE) readback_colour<QM_DOUBLE>(ws, wm, wt, stego, g, qp, bits, bit_offset, n_bits, n_words, counts, c);
            else readback_colour<QM_POW2>(ws, wm, wt, stego, g, qp, bits, bit_offset, n_bits, n_words, counts, c);
            return;
        }
    }
    // The gray form: one lane per block checks it with the lane-per-block arithmetic (readback_block_ok<U, QM>), and only the
    // failing blocks enter the worklist, where they are searched without another check.
    const uint32_t gblock = tile_id(g.xcd_chunk) * (uint32_t)SVS_WG + threadIdx.x;
    const uint32_t n = g.n_ac;
    uint32_t nb = 0;
    uint64_t first = 0;
    if (gblock < g.total_blocks) {
        first = stream_first<KEYED>(gblock, n, g, order_arg(order...));
        nb = block_budget(first, n_bits, n);
    }
    if (__ballot(nb > 0) == 0) return;   // wave-uniform
    bool bad = false;
    int64_t off = 0;
    uint32_t hi = 0, lo = 0;
    if (nb > 0) {
        off = block_offset(gblock, g);
        u32x2 v[8];
        load_rows<1>(stego + off, g.row_pitch, v);
        uint32_t ax[8], ay[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) { ax[r] = v[r].x; ay[r] = v[r].y; }
        payload_window(bits, n_words, bit_offset + first, hi, lo);
        bad = !readback_block_ok<U, QM>(ax, ay, nb, hi, lo, qp);
    }
    const uint64_t mask = __ballot(bad);
    if (mask == 0) return;               // wave-uniform: content without failures
    const uint32_t status = readback_worklist(
        ws, wm, wt, bad, wave_rank(mask), (uint32_t)__popcll(mask),
        [&](uint32_t *e, u32x4 &m) {   // the rows are read again (the block's own bytes, still unwritten): no registers held across rounds
            deposit_rows(stego + off, g.row_pitch, e);
            m.x = hi; m.y = lo; m.z = nb; m.w = 0u;
        },
        [&](uint32_t *px, float *t, uint32_t r, const u32x4 &m, auto settle) {
            settle(search8(px, t, r, PlainRows<QM>{r, m.z, m.x, m.y, qp}) ? 1u : 2u);
        },
        [&](const uint32_t *e) { store_entry_rows(e, stego + off, g.row_pitch); });
    add_counts(counts, 0u, status);
}

// ---------------------------------------------------------------------------------------
// measurement helpers
// ---------------------------------------------------------------------------------------
// lowbias32: svs_order.hpp
// 8 pixels per thread per step; same hash as svsdct/synth.py
__global__ __launch_bounds__(256) void fill_synthetic_kernel(uint8_t *__restrict__ frames, int32_t n_frames,
                                                             int32_t height, int32_t width, int64_t row_pitch,
                                                             int64_t frame_pitch, uint32_t seed,
                                                             uint32_t first_frame, uint32_t lo, uint32_t span) {
    const uint32_t groups_per_row = (uint32_t)width / 8u;
    const uint64_t total = (uint64_t)n_frames * height * groups_per_row;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t xg = (uint32_t)(t % groups_per_row);
        const uint64_t r = t / groups_per_row;
        const uint32_t y = (uint32_t)(r % (uint32_t)height), f = (uint32_t)(r / (uint32_t)height);
        const uint32_t base = seed + (f + first_frame) * 0x9E3779B1u + y * 0x85EBCA6Bu;
        uint32_t px[2] = {0, 0};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t x = xg * 8u + j;
            const uint32_t v = lo + lowbias32(base + x * 0xC2B2AE35u) % span;
            px[j >> 2] |= v << (8 * (j & 3));
        }
        u32x2 r8;
        r8.x = px[0];
        r8.y = px[1];
        *reinterpret_cast<u32x2 *>(frames + (int64_t)f * frame_pitch + (int64_t)y * row_pitch + xg * 8u) = r8;
    }
}

__global__ __launch_bounds__(256) void fill_bits_kernel(uint32_t *__restrict__ words, uint64_t n_words,
                                                        uint64_t n_bits, uint32_t seed, uint64_t first_bit) {
    const uint32_t s = seed * 0x632BE5ABu;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_words;
         w += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t be = 0;  // big-endian view: stream bit 32w+j at bit 31-j
        for (uint32_t j = 0; j < 32; ++j) {
            const uint64_t i = 32ull * w + j;
            if (i < n_bits) be |= (lowbias32(s + (uint32_t)(first_bit + i)) >> 31) << (31 - j);
        }
        words[w] = __builtin_bswap32(be);
    }
}

// ---------------------------------------------------------------------------------------
// The reference operator's payload types are Python strings of '0' / '1' characters (bit_payload_segment in, the joined
// string out: config_and_setup.py:106-109,124-126,173-174).  The host-pointer entry points svs_embed_str / svs_extract_str
// take / return exactly that; the conversion to and from the packed stream runs here, on the device, at the price of moving
// one byte per bit over the link (1.3 MB for a 4K frame at n = 10: 25 us) instead of three host passes over it.
// 32 characters -> one packed dword: the bit is the low bit of the character ('0' = 0x30, '1' = 0x31); four of them times
// 0x08040201 leave the nibble c0 c1 c2 c3 in bits 27..24 of the product (no carries: every cross term lands below bit 19).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ascii_to_packed_kernel(const uint8_t *__restrict__ ascii, uint64_t n_chars,
                                                              uint32_t *__restrict__ words, uint64_t n_words) {
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t base = 32ull * w;
        uint32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (base + 32 <= n_chars) {
            const u32x4 a = *reinterpret_cast<const u32x4 *>(ascii + base), b = *reinterpret_cast<const u32x4 *>(ascii + base + 16);
            d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
        } else {
            for (uint32_t j = 0; j < 32 && base + j < n_chars; ++j) d[j >> 2] |= (uint32_t)ascii[base + j] << (8 * (j & 3));
        }
        uint32_t be = 0;   // stream bit 32 w + j at bit 31 - j
#pragma unroll
        for (int j = 0; j < 8; ++j) be |= ((((d[j] & 0x01010101u) * 0x08040201u) >> 24) & 0xfu) << (28 - 4 * j);
        words[w] = __builtin_bswap32(be);
    }
}

// one packed byte -> its eight characters, MSB first
__global__ __launch_bounds__(256) void packed_to_ascii_kernel(const uint8_t *__restrict__ packed, uint64_t n_bytes,
                                                              u32x2 *__restrict__ ascii8) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_bytes; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t v = packed[i];
        u32x2 o;
        o.x = 0x30303030u | ((v >> 7) & 1u) | (((v >> 6) & 1u) << 8) | (((v >> 5) & 1u) << 16) | (((v >> 4) & 1u) << 24);
        o.y = 0x30303030u | ((v >> 3) & 1u) | (((v >> 2) & 1u) << 8) | (((v >> 1) & 1u) << 16) | ((v & 1u) << 24);
        ascii8[i] = o;
    }
}

// per-frame sum of squared differences; blockIdx.y = frame, 8 pixels per thread per step,
// partial sums reduced in-wave, one 64-bit atomic per wave
__global__ __launch_bounds__(256) void frame_sse_kernel(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b,
                                                        int32_t height, int32_t width, int64_t row_pitch,
                                                        int64_t frame_pitch, unsigned long long *__restrict__ sse) {
    const uint32_t f = blockIdx.y;
    const uint32_t groups_per_row = (uint32_t)width / 8u;
    const uint64_t total = (uint64_t)height * groups_per_row;
    unsigned long long acc = 0;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total;
         t += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t xg = (uint32_t)(t % groups_per_row), y = (uint32_t)(t / groups_per_row);
        const int64_t off = (int64_t)f * frame_pitch + (int64_t)y * row_pitch + xg * 8u;
        const u32x2 va = *reinterpret_cast<const u32x2 *>(a + off);
        const u32x2 vb = *reinterpret_cast<const u32x2 *>(b + off);
        const uint32_t wa[2] = {va.x, va.y}, wb[2] = {vb.x, vb.y};
        uint32_t s = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int d = (int)((wa[j >> 2] >> (8 * (j & 3))) & 0xff) - (int)((wb[j >> 2] >> (8 * (j & 3))) & 0xff);
            s += (uint32_t)(d * d);
        }
        acc += s;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63u) == 0 && acc) atomicAdd(&sse[f], acc);
}

__global__ __launch_bounds__(256) void bit_errors_kernel(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b,
                                                         uint64_t n_bits, unsigned long long *__restrict__ count) {
    const uint64_t n_bytes = (n_bits + 7) / 8;
    unsigned long long acc = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_bytes;
         i += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t x = (uint32_t)(a[i] ^ b[i]);
        if (i == n_bytes - 1 && (n_bits & 7u)) x &= 0xFFu << (8 - (n_bits & 7u));
        acc += __popc(x);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63u) == 0 && acc) atomicAdd(count, acc);
}

// ---------------------------------------------------------------------------------------
// Colour plumbing around the operator: interleaved 8-bit BGR -> gray
// (cv2.COLOR_BGR2GRAY, config_and_setup.py:112) and gray -> BGR (cv2.COLOR_GRAY2BGR, embed_process.py:126).
// OpenCV's 8-bit BGR2GRAY is fixed point: (B*wb + G*wg + R*wr + 2^(shift-1)) >> shift; the weights are passed
// in because they differ between OpenCV generations (15-bit 3735/19235/9798 today, 14-bit 1868/9617/4899 in
// older builds) and cv2 is not available to pin either.  4 pixels per thread: 12 bytes in, one dword out.
// ---------------------------------------------------------------------------------------
// (kernels: bgr_to_gray_kernel / gray_to_bgr_kernel below, after the wave-cooperative row helpers they share with the
// fused colour path)
// ---------------------------------------------------------------------------------------
// Fused colour path ("fused read of 3 B/px"): the frames that carry payload go
// BGR -> gray -> embed -> BGR in ONE pass - 3 B/pixel read, 3 B/pixel written (+1 for the optional gray
// reference the operator returns) instead of the 10 B/pixel of convert / embed / convert.  One lane = one
// block = 8 rows x 24 bytes; stego pixels are written as B = G = R = gray (cv2.COLOR_GRAY2BGR).  Every block
// of these frames is converted; blocks past the payload budget carry their gray value unchanged.
// ---------------------------------------------------------------------------------------
// (ColourParams, block_offset_bgr, load_bgr_row / store_bgr_row and bgr8_to_gray stand above the read-back pass, which uses them)
// 8 gray bytes -> 8 interleaved BGR pixels with B = G = R: six byte permutes (v_perm_b32 selects bytes 0-3 from
// its second operand, 4-7 from its first)
__device__ __forceinline__ void gray8_to_bgr(uint32_t lo4, uint32_t hi4, u32x2 &q0, u32x2 &q1, u32x2 &q2) {
    q0.x = __builtin_amdgcn_perm(0u, lo4, 0x01000000u);  // a a a b
    q0.y = __builtin_amdgcn_perm(0u, lo4, 0x02020101u);  // b b c c
    q1.x = __builtin_amdgcn_perm(0u, lo4, 0x03030302u);  // c d d d
    q1.y = __builtin_amdgcn_perm(0u, hi4, 0x01000000u);
    q2.x = __builtin_amdgcn_perm(0u, hi4, 0x02020101u);
    q2.y = __builtin_amdgcn_perm(0u, hi4, 0x03030302u);
}

// A wave's 64 blocks are 64 x 24 = 1536 consecutive bytes per pixel row (except where the run of blocks wraps to the
// next block row / frame): seen as 192 units of 8 bytes, unit u = bytes [8*(u%3), +8) of the row of block u/3.
struct WaveUnits {
    uint32_t owner[3], part[3];  // of unit lane + 64 j
    bool live[3];
};
__device__ __forceinline__ WaveUnits wave_units(uint32_t lane, uint32_t wave_first, uint32_t total_blocks) {
    WaveUnits w;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const uint32_t u = lane + 64u * j;
        w.owner[j] = (u * 171u) >> 9;  // u / 3 for u < 192
        w.part[j] = u - 3u * w.owner[j];
        w.live[j] = wave_first + w.owner[j] < total_blocks;
    }
    return w;
}

// Cooperative load of the wave's BGR rows: every load instruction covers 512
// contiguous bytes; the rows pass through a wave-private, double-buffered LDS row (2 x 192 units) from which each lane
// picks its own 24 bytes and converts them to gray.  +6 % in extract_bgr_kernel over lanes loading their own rows at a
// 24-byte stride (profiles/history/r01_aux_kernel_rates.txt).
__device__ __forceinline__ void wave_load_gray(const uint8_t *__restrict__ bgr, const Geometry &g, const ColourParams &c,
                                               const WaveUnits &wu, uint32_t wave_first, uint32_t lane, u32x2 *rowbuf,
                                               uint32_t (&ax)[8], uint32_t (&ay)[8]) {
    u32x2 raw[8][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const uint8_t *src = bgr + block_offset_bgr(wave_first + wu.owner[j], g, c.in_row_pitch, c.in_frame_pitch) +
                             8u * wu.part[j];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            u32x2 v; v.x = 0u; v.y = 0u;
            if (wu.live[j]) v = SVS_LD(reinterpret_cast<const u32x2 *>(src + r * c.in_row_pitch));
            raw[r][j] = v;
        }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        u32x2 *buf = rowbuf + (r & 1) * 192;
#pragma unroll
        for (int j = 0; j < 3; ++j) buf[lane + 64 * j] = raw[r][j];
        wave_lds_fence();  // also separates the reads of row r-1 from the writes of row r+1 into the same buffer
        bgr8_to_gray(buf[3 * lane], buf[3 * lane + 1], buf[3 * lane + 2], c, ax[r], ay[r]);
    }
    wave_lds_fence();
}

// Same, HALF rows at a time (two rounds of 4 rows): half the registers in flight, for kernels that are short of them
__device__ __forceinline__ void wave_load_gray_halves(const uint8_t *bgr, const Geometry &g,
                                                      const ColourParams &c, uint32_t wave_first, uint32_t lane,
                                                      u32x2 *rowbuf, uint32_t (&ax)[8], uint32_t (&ay)[8]) {
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
        const WaveUnits wu = wave_units(lane, wave_first, g.total_blocks);
        u32x2 raw[4][3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint8_t *src = bgr + block_offset_bgr(wave_first + wu.owner[j], g, c.in_row_pitch, c.in_frame_pitch) +
                                 8u * wu.part[j] + (int64_t)(4 * half) * c.in_row_pitch;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                u32x2 v; v.x = 0u; v.y = 0u;
                if (wu.live[j]) v = SVS_LD(reinterpret_cast<const u32x2 *>(src + r * c.in_row_pitch));
                raw[r][j] = v;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            u32x2 *buf = rowbuf + (r & 1) * 192;
#pragma unroll
            for (int j = 0; j < 3; ++j) buf[lane + 64 * j] = raw[r][j];
            wave_lds_fence();
            uint32_t gx, gy;
            bgr8_to_gray(buf[3 * lane], buf[3 * lane + 1], buf[3 * lane + 2], c, gx, gy);
            if (half == 0) { ax[r] = gx; ay[r] = gy; } else { ax[4 + r] = gx; ay[4 + r] = gy; }
        }
        wave_lds_fence();
    }
}

// Gray rows of a wave's 64 blocks -> interleaved BGR with B = G = R, through the wave-private tile `mine` (8 rows x 64
// lanes of 8 gray bytes): every store instruction covers 512 contiguous bytes.
__device__ __forceinline__ void wave_store_gray_as_bgr(u32x2 *mine, uint32_t lane, uint32_t gblock, bool live,
                                                       const uint32_t (&ax)[8], const uint32_t (&ay)[8],
                                                       uint8_t *bgr_out, const Geometry &g,
                                                       const ColourParams &c) {
    if (live) {
#pragma unroll
        for (int r = 0; r < 8; ++r) { u32x2 v; v.x = ax[r]; v.y = ay[r]; mine[r * 64 + lane] = v; }
    }
    wave_lds_fence();  // wave-private tile: LDS operations of one wave execute in order; this pins the compiler's order
    const uint32_t wave_first = gblock - lane;
    const WaveUnits wu = wave_units(lane, wave_first, g.total_blocks);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const uint32_t owner = wu.owner[j], part = wu.part[j];
        if (!wu.live[j]) continue;
        // gray pixels feeding the unit's two dwords (v_perm_b32: selector bytes 0-3 pick from the low gray dword,
        // 4-7 from the high one): part 0 = p0 p0 p0 p1 | p1 p1 p2 p2, part 1 = p2 p3 p3 p3 | p4 p4 p4 p5,
        // part 2 = p5 p5 p6 p6 | p6 p7 p7 p7
        const uint32_t sel0 = part == 0 ? 0x01000000u : part == 1 ? 0x03030302u : 0x06060505u;
        const uint32_t sel1 = part == 0 ? 0x02020101u : part == 1 ? 0x05040404u : 0x07070706u;
        uint8_t *dst = bgr_out + block_offset_bgr(wave_first + owner, g, c.out_row_pitch, c.out_frame_pitch) + 8u * part;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const u32x2 v = mine[r * 64 + owner];
            u32x2 q;
            q.x = __builtin_amdgcn_perm(v.y, v.x, sel0);
            q.y = __builtin_amdgcn_perm(v.y, v.x, sel1);
            asm volatile("global_store_dwordx2 %0, %1, off sc1\n\ts_nop 1" ::"v"(dst + r * c.out_row_pitch), "v"(q) : "memory");
        }
    }
}

// SVS_KEEP_COLOUR: the stego rows leave as the COVER's pixels shifted to the stego gray (svs_colour.hpp) instead of
// B = G = R.  The wave re-reads the cover four rows at a time (the same 512-byte cooperative loads as wave_load_gray_halves,
// units [0, 192) of the wave's 4 KB region); each lane takes its 24 bytes, adds d = stego - cover gray to B, G and R as
// packed 16-bit lanes and parks the result at units [192, 384); only in a wave where some lane's sum left [0, 255] do the
// pixels with a clipped channel get the exact rule, byte by byte through LDS.  The wave then stores the row as 512-byte
// runs.  Every row is loaded before it is stored and a wave touches only its own blocks: bgr_in == bgr_out is safe.
__device__ __forceinline__ void wave_store_keep_colour(u32x2 *region, uint32_t lane, uint32_t gblock,
                                                       const uint32_t (&ax)[8], const uint32_t (&ay)[8],
                                                       const uint8_t *bgr_in, uint8_t *bgr_out, const Geometry &g,
                                                       const ColourParams &c) {
    typedef int16_t i16x2 __attribute__((ext_vector_type(2)));
    const auto pk_sub = [](uint32_t a, uint32_t b) {
        return __builtin_bit_cast(uint32_t, __builtin_bit_cast(i16x2, a) - __builtin_bit_cast(i16x2, b));
    };
    u32x2 *cover = region, *shifted = region + 192;
    const uint32_t wave_first = gblock - lane;
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
        const WaveUnits wu = wave_units(lane, wave_first, g.total_blocks);
        u32x2 raw[4][3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint8_t *src = bgr_in + block_offset_bgr(wave_first + wu.owner[j], g, c.in_row_pitch, c.in_frame_pitch) +
                                 8u * wu.part[j] + (int64_t)(4 * half) * c.in_row_pitch;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                u32x2 v; v.x = 0u; v.y = 0u;
                if (wu.live[j]) v = SVS_LD(reinterpret_cast<const u32x2 *>(src + r * c.in_row_pitch));
                raw[r][j] = v;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int j = 0; j < 3; ++j) cover[lane + 64 * j] = raw[r][j];
            wave_lds_fence();
            const u32x2 q0 = cover[3 * lane], q1 = cover[3 * lane + 1], q2 = cover[3 * lane + 2];
            const uint32_t tlo = half == 0 ? ax[r] : ax[4 + r], thi = half == 0 ? ay[r] : ay[4 + r];
            uint32_t glo, ghi;
            bgr8_to_gray(q0, q1, q2, c, glo, ghi);
            // d of pixels (0,1) (2,3) (4,5) (6,7) as 16-bit lanes, then of the twelve channel pairs of the 24 bytes
            // B0G0 R0B1 G1R1 B2G2 R2B3 G3R3 B4G4 R4B5 G5R5 B6G6 R6B7 G7R7
            const uint32_t d01 = pk_sub(__builtin_amdgcn_perm(0u, tlo, 0x0c010c00u), __builtin_amdgcn_perm(0u, glo, 0x0c010c00u));
            const uint32_t d23 = pk_sub(__builtin_amdgcn_perm(0u, tlo, 0x0c030c02u), __builtin_amdgcn_perm(0u, glo, 0x0c030c02u));
            const uint32_t d45 = pk_sub(__builtin_amdgcn_perm(0u, thi, 0x0c010c00u), __builtin_amdgcn_perm(0u, ghi, 0x0c010c00u));
            const uint32_t d67 = pk_sub(__builtin_amdgcn_perm(0u, thi, 0x0c030c02u), __builtin_amdgcn_perm(0u, ghi, 0x0c030c02u));
            const uint32_t lo = 0x01000100u, hi = 0x03020302u;   // (a, a) and (b, b) of a lane pair (a, b)
            const uint32_t dd[12] = {__builtin_amdgcn_perm(0u, d01, lo), d01, __builtin_amdgcn_perm(0u, d01, hi),
                                     __builtin_amdgcn_perm(0u, d23, lo), d23, __builtin_amdgcn_perm(0u, d23, hi),
                                     __builtin_amdgcn_perm(0u, d45, lo), d45, __builtin_amdgcn_perm(0u, d45, hi),
                                     __builtin_amdgcn_perm(0u, d67, lo), d67, __builtin_amdgcn_perm(0u, d67, hi)};
            const uint32_t w[6] = {q0.x, q0.y, q1.x, q1.y, q2.x, q2.y};
            uint32_t s[12], any = 0u;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                s[2 * k] = pk_add_i16(__builtin_amdgcn_perm(0u, w[k], 0x0c010c00u), dd[2 * k]);
                s[2 * k + 1] = pk_add_i16(__builtin_amdgcn_perm(0u, w[k], 0x0c030c02u), dd[2 * k + 1]);
                any |= s[2 * k] | s[2 * k + 1];
            }
            u32x2 o0, o1, o2;   // low bytes of the 16-bit lanes
            o0.x = __builtin_amdgcn_perm(s[1], s[0], 0x06040200u); o0.y = __builtin_amdgcn_perm(s[3], s[2], 0x06040200u);
            o1.x = __builtin_amdgcn_perm(s[5], s[4], 0x06040200u); o1.y = __builtin_amdgcn_perm(s[7], s[6], 0x06040200u);
            o2.x = __builtin_amdgcn_perm(s[9], s[8], 0x06040200u); o2.y = __builtin_amdgcn_perm(s[11], s[10], 0x06040200u);
            shifted[3 * lane] = o0; shifted[3 * lane + 1] = o1; shifted[3 * lane + 2] = o2;
            const bool clipped = (any & 0xff00ff00u) != 0u;   // some lane < 0 (0xffxx) or > 255 (0x01xx)
            if (__ballot(clipped) != 0ull) {
                // the pixels with a clipped channel (byte 2m + h of the row belongs to pixel (2m + h) / 3), redone one at a
                // time: the wave loops as often as its busiest lane has clipped pixels, not eight times
                uint32_t todo = 0u;
#pragma unroll
                for (int m = 0; m < 12; ++m) {
                    todo |= (s[m] & 0x0000ff00u) ? 1u << ((2 * m) / 3) : 0u;
                    todo |= (s[m] & 0xff000000u) ? 1u << ((2 * m + 1) / 3) : 0u;
                }
                const uint8_t *cb = reinterpret_cast<const uint8_t *>(cover + 3 * lane);
                uint8_t *ob = reinterpret_cast<uint8_t *>(shifted + 3 * lane);
                while (todo != 0u) {
                    const uint32_t p = (uint32_t)__builtin_ctz(todo);
                    todo &= todo - 1u;
                    uint32_t B = cb[3 * p], G = cb[3 * p + 1], R = cb[3 * p + 2];
                    const uint32_t t = ((p < 4 ? tlo : thi) >> (8u * (p & 3u))) & 0xffu;
                    keep_colour_pixel(B, G, R, t, c.wb, c.wg, c.wr, c.shift);
                    ob[3 * p] = (uint8_t)B; ob[3 * p + 1] = (uint8_t)G; ob[3 * p + 2] = (uint8_t)R;
                }
            }
            wave_lds_fence();
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (!wu.live[j]) continue;
                const uint32_t owner = wu.owner[j], part = wu.part[j];
                uint8_t *dst = bgr_out + block_offset_bgr(wave_first + owner, g, c.out_row_pitch, c.out_frame_pitch) + 8u * part +
                               (int64_t)(4 * half + r) * c.out_row_pitch;
                const u32x2 v = shifted[lane + 64 * j];
                asm volatile("global_store_dwordx2 %0, %1, off sc1\n\ts_nop 1" ::"v"(dst), "v"(v) : "memory");
            }
            wave_lds_fence();   // the next row's writes into the region come after these reads
        }
    }
}

// Stand-alone conversions (svs_bgr_to_gray_dev / svs_gray_to_bgr_dev), block-structured like the operator so that they
// share its coalesced row movers: 8x8 blocks, one lane per block.
__global__ __launch_bounds__(SVS_WG) void bgr_to_gray_kernel(const uint8_t *__restrict__ bgr, uint8_t *__restrict__ gray,
                                                             const Geometry g, const ColourParams c) {
    __shared__ __attribute__((aligned(16))) u32x2 rows[SVS_WG / 64][2 * 192];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t gblock = tile_id(g.xcd_chunk) * (uint32_t)SVS_WG + threadIdx.x;
    const WaveUnits wu = wave_units(lane, gblock - lane, g.total_blocks);
    uint32_t ax[8], ay[8];
    wave_load_gray(bgr, g, c, wu, gblock - lane, lane, &rows[wave][0], ax, ay);
    if (gblock < g.total_blocks) {
        typename RowVec<1>::type v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) { v[r].x = ax[r]; v[r].y = ay[r]; }
        store_rows<1>(gray + block_offset(gblock, g), g.row_pitch, v);
    }
}

__global__ __launch_bounds__(SVS_WG) void gray_to_bgr_kernel(const uint8_t *__restrict__ gray, uint8_t *__restrict__ bgr,
                                                             const Geometry g, const ColourParams c) {
    __shared__ __attribute__((aligned(16))) u32x2 tile[SVS_WG / 64][8][64];
    const uint32_t gblock = tile_id(g.xcd_chunk) * (uint32_t)SVS_WG + threadIdx.x;
    const bool live = gblock < g.total_blocks;
    uint32_t ax[8], ay[8];
    if (live) {
        typename RowVec<1>::type v[8];
        load_rows<1>(gray + block_offset(gblock, g), g.row_pitch, v);
#pragma unroll
        for (int r = 0; r < 8; ++r) { ax[r] = v[r].x; ay[r] = v[r].y; }
    }
    wave_store_gray_as_bgr(&tile[threadIdx.x >> 6][0][0], threadIdx.x & 63u, gblock, live, ax, ay, bgr, g, c);
}

// Stego rows leave through a wave-private LDS tile: each lane parks its 8 stego gray
// bytes per row, then the wave writes the BGR row as 192 consecutive 8-byte units - unit u = bytes [8*(u%3), +8) of the
// 24-byte row of the wave's block u/3 - so every store instruction covers 512 contiguous bytes instead of 8 bytes in
// every 24.
// KEEP (SVS_KEEP_COLOUR): the cover's colours shifted to the stego gray, wave_store_keep_colour; otherwise B = G = R.
template <int U, int QM, bool EXACT, bool KEEP>
__global__ __launch_bounds__(SVS_WG) void embed_bgr_kernel(const uint8_t *bgr_in,   // may alias bgr_out
                                                        uint8_t *bgr_out, uint8_t *__restrict__ gray_ref,
                                                        const Geometry g, const ColourParams c, const QimParams qp_arg,
                                                        const uint32_t *__restrict__ bits, const uint64_t bit_offset,
                                                        const uint64_t n_bits, const uint32_t n_words) {
    // one wave-private 4 KB region per wave: row staging of the cooperative load, then (streaming arithmetic) the worklist and transposition
    // tile of the exact replay (guard_phase2 with 16 entries per round), then the stego tile of the cooperative store
    __shared__ __attribute__((aligned(16))) u32x2 lds_tile[SVS_WG / 64][8][64];
    static_assert(16 * sizeof(GuardEntry) + 8 * SVS_GUARD_TILE * sizeof(float) <= 8 * 64 * sizeof(u32x2), "wave region too small");
    // SVS_NEAREST, SVS_MINMOVE: the rule stays a run-time value here and the bodies test it once per block (two compares of a
    // wave-uniform word).  Two copies of the whole body, as in the gray kernels, take the allocation of the larger one: 124 ->
    // 132 and 167 -> 169 VGPRs, a wave per SIMD less.  The same holds for a single branch around the body with only the
    // SVS_MINMOVE side a constant: the keep-colour forms go 124 -> 132 and 168 -> 169 VGPRs, 4 -> 3 and 3 -> 2 waves.  With the
    // run-time rule no form loses a wave (the plain one-row form grows from 82 to 93 VGPRs, the limit of 5 waves is 96) and the
    // flag-clear time is inside the spread of the build before the flag: profiles/minmove_resources.txt, minmove_rates.txt.
    const QimRule rule = rule_from_word(qp_arg, g.pad);
    const QimRule &qp = rule;
    const uint32_t tile = tile_id(g.xcd_chunk);
    const uint32_t gblock = tile * (uint32_t)SVS_WG + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool live = gblock < g.total_blocks;
    uint32_t ax[8], ay[8];
    // cooperative load, four rows at a time: +5..7 % over per-lane loads at a 24-byte stride with the streaming arithmetic (62 -> 78 VGPRs),
    // neutral in EXACT mode; all eight rows at once cost 100+ VGPRs and gained 1 % (profiles/history/r01_aux_kernel_rates.txt)
    wave_load_gray_halves(bgr_in, g, c, gblock - lane, lane, &lds_tile[wave][0][0], ax, ay);
    bool und = false;
    constexpr bool KEPT = !EXACT && U <= 2;   // see embed_kernel
    uint32_t hi_kept = 0;
    if (live) {
        if (gray_ref != nullptr) {  // the operator's first return value: the gray frame before embedding
            uint8_t *ref = gray_ref + block_offset(gblock, g);
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                u32x2 v; v.x = ax[r]; v.y = ay[r];
                SVS_ST(v, reinterpret_cast<u32x2 *>(ref + r * g.row_pitch));
            }
        }
        const uint32_t n = g.n_ac;
        const uint64_t first = (uint64_t)gblock * n;
        if (first < n_bits) {
            if constexpr (EXACT) {
                uint32_t hi, lo;
                payload_window(bits, n_words, bit_offset + first, hi, lo);
                embed_block_exact<8, QM>(ax, ay, n, block_budget(first, n_bits, n), hi, lo, qp);
            } else {
                und = guard_phase1<U, QM>(ax, ay, n, first, qp, bits, bit_offset, n_bits, n_words, KEPT ? &hi_kept : nullptr);
            }
        }
    }
    if constexpr (!EXACT) {   // undecided blocks: exact replay inside the wave (see embed_kernel)
        GuardEntry *entries = reinterpret_cast<GuardEntry *>(&lds_tile[wave][0][0]);
        float *t = reinterpret_cast<float *>(entries + 16);
        const GuardPayload pl{bits, bit_offset, n_bits, n_words};
        guard_phase2<QM, 16, KEPT>(entries, t, lane, g.n_ac, qp, pl, und, (uint64_t)gblock * g.n_ac, ax, ay, hi_kept);
    }
    if constexpr (KEEP)
        wave_store_keep_colour(&lds_tile[wave][0][0], lane, gblock, ax, ay, bgr_in, bgr_out, g, c);
    else
        wave_store_gray_as_bgr(&lds_tile[wave][0][0], lane, gblock, live, ax, ay, bgr_out, g, c);
}

// extract straight from interleaved BGR frames (gray computed on the fly).  One coefficient row: pocketfft-identical forward;
// two and more rows (round 4): the two-step FAST extraction of extract_kernel - FMA-factored forward, wave ballot of near-tie
// candidates, pocketfft coefficient 4 + per-block margin, 8-lane exact replay of tie blocks - instead of the pocketfft forward
// of every row for every block (0.88 ms per 200 x 4K BGR frames at n = 10 against an HBM floor of 0.75).
// FASTX = false keeps the pocketfft forward (delta below SVS_FAST_EXTRACT_DELTA_MIN).
template <int U, int QM, bool FASTX = (U >= 2)>
__global__ __launch_bounds__(SVS_WG) void extract_bgr_kernel(const uint8_t *__restrict__ bgr, const Geometry g,
                                                          const ColourParams c, const QimParams qp,
                                                          uint8_t *__restrict__ out, const uint64_t out_bytes) {
    __shared__ uint32_t flags[SVS_WG / 64][SVS_WAVE_BITS_DWORDS(1)];
    __shared__ __attribute__((aligned(16))) u32x2 rows[SVS_WG / 64][2 * 192];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t tile = tile_id(g.xcd_chunk);
    const uint32_t gblock = tile * (uint32_t)SVS_WG + threadIdx.x;
    const uint32_t n = g.n_ac;
    uint32_t hi = 0, lo = 0;
    uint32_t ax[8], ay[8];
    const WaveUnits wu = wave_units(lane, gblock - lane, g.total_blocks);
    wave_load_gray(bgr, g, c, wu, gblock - lane, lane, &rows[wave][0], ax, ay);
    if constexpr (FASTX) {
        __shared__ GuardEntry entries[SVS_WG / 64][SVS_EXTRACT_CAP];
        __shared__ float tiles[SVS_WG / 64][8 * SVS_GUARD_TILE];
        bool tie = false;
        float off = 0.0f;
        if (gblock < g.total_blocks) tie = extract_block_cheap<U, QM>(ax, ay, n, qp, hi, lo, off);    // -> candidate
        if (__ballot(tie) != 0) {
            if (gblock < g.total_blocks) tie = extract_block_settle<QM>(ax, ay, n, qp, hi, off);
        }
        extract_phase2<QM, SVS_EXTRACT_CAP>(&entries[wave][0], &tiles[wave][0], lane, n, qp, tie, ax, ay, hi, lo);
    } else {
        if (gblock < g.total_blocks) extract_block_exact<U, QM>(ax, ay, n, qp, hi, lo);
    }
    emit_wave_bits<U, 1>(&flags[wave][0], lane, (uint64_t)tile * (uint32_t)SVS_WG + wave * 64u, n, hi, lo, 0u, 0u, out,
                         out_bytes);
}

// ---------------------------------------------------------------------------------------
// SSIM evaluator: mean structural similarity of two gray frames as
// skimage.metrics.structural_similarity computes it with its defaults for 2-D uint8 input (what the
// reference's evaluation.calc_ssim calls, evaluation.py:21-26): 7x7 uniform window, K1 = 0.01, K2 = 0.03,
// sample covariance (NP/(NP-1)), float64 arithmetic, mean over the map cropped by 3 pixels per side.
// Window sums are exact integers here (skimage's running float sums differ from them by rounding only).
// One workgroup = 256 output columns x SSIM_BAND output rows; a thread walks down its column keeping the
// last 7 horizontal window sums of the five moments in registers.
// ---------------------------------------------------------------------------------------
#define SVS_SSIM_BAND 126  // output rows per workgroup (a multiple of 7 keeps the row groups aligned)
__global__ __launch_bounds__(256) void ssim_partial_kernel(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b,
                                                           int32_t height, int32_t width, int64_t row_pitch,
                                                           int64_t frame_pitch, const double *__restrict__ data_range,
                                                           double *__restrict__ partial) {
    __shared__ __attribute__((aligned(8))) uint8_t ra[7][256 + 8], rb[7][256 + 8];  // 7 input rows at a time
    __shared__ double red[4];
    const int out_w = width - 6, out_h = height - 6;
    const int x0 = blockIdx.x * 256, y0 = blockIdx.y * SVS_SSIM_BAND, f = blockIdx.z;
    const int t = threadIdx.x;
    const uint8_t *pa = a + (int64_t)f * frame_pitch, *pb = b + (int64_t)f * frame_pitch;
    const double R = data_range[f];
    // C1 and C2 scaled by 49^2 and 49 * 48, the denominators of the means and the sample (co)variances: see below
    const double C1 = 2401.0 * ((0.01 * R) * (0.01 * R)), C2 = 2352.0 * ((0.03 * R) * (0.03 * R));
    // ring of the last 7 horizontal 7-sums of the five moments; slot = input row % 7, so with rows handled in groups
    // of 7 every slot index below is a compile-time constant
    uint32_t ha[7], hb[7], haa[7], hbb[7], hab[7];
    uint32_t va = 0, vb = 0, vaa = 0, vbb = 0, vab = 0;
#pragma unroll
    for (int i = 0; i < 7; ++i) ha[i] = hb[i] = haa[i] = hbb[i] = hab[i] = 0;
    double acc = 0.0;
    const int rows = min(SVS_SSIM_BAND, out_h - y0) + 6;  // input rows this band touches
    const bool col_ok = x0 + t < out_w;
    for (int r0 = 0; r0 < rows; r0 += 7) {
        __syncthreads();
        // stage 7 rows x 264 columns of both frames with 8-byte loads (x0 and the row pitch are multiples of 8, the
        // width is a multiple of 8, so a chunk is either wholly inside the frame or wholly outside)
        for (int i = t; i < 7 * 33; i += 256) {
            const int j = i / 33, c8 = i - j * 33;
            const int x = x0 + 8 * c8, y = y0 + r0 + j;
            u32x2 qa = {0u, 0u}, qb = {0u, 0u};
            if (x < width && y < height && r0 + j < rows) {
                qa = *reinterpret_cast<const u32x2 *>(pa + (int64_t)y * row_pitch + x);
                qb = *reinterpret_cast<const u32x2 *>(pb + (int64_t)y * row_pitch + x);
            }
            *reinterpret_cast<u32x2 *>(&ra[j][8 * c8]) = qa;
            *reinterpret_cast<u32x2 *>(&rb[j][8 * c8]) = qb;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            uint32_t sa = 0, sb = 0, saa = 0, sbb = 0, sab = 0;
#pragma unroll
            for (int d = 0; d < 7; ++d) {
                const uint32_t u = ra[j][t + d], v = rb[j][t + d];
                sa += u; sb += v;
                saa += __umul24(u, u); sbb += __umul24(v, v); sab += __umul24(u, v);  // full-rate 24-bit multiplies
            }
            va += sa - ha[j]; vb += sb - hb[j]; vaa += saa - haa[j]; vbb += sbb - hbb[j]; vab += sab - hab[j];
            ha[j] = sa; hb[j] = sb; haa[j] = saa; hbb[j] = sbb; hab[j] = sab;
            const int r = r0 + j;
            if (r >= 6 && r < rows && col_ok) {
                // skimage's four terms, those of the means (sum / 49) scaled by 49^2 and those of the sample (co)variances
                // by 49 * 48: apart from C1, C2 they are exact integers below 2^29 - 2 sum(x) sum(y), sum(x)^2 + sum(y)^2,
                // and the numerators 49 sum(xy) - sum(x) sum(y) (>= 0 for the variances: Cauchy-Schwarz).  A flat window's
                // variance is exactly 0, so with a data range of 0 (C1 = C2 = 0) a window flat in both frames gives
                // skimage's 0 / 0 = NaN.
                const uint32_t nx = 49u * vaa - va * va, ny = 49u * vbb - vb * vb;
                const int32_t nxy = (int32_t)(49u * vab - va * vb);
                const double A1 = (double)(2u * va * vb) + C1, B1 = (double)(va * va + vb * vb) + C1;
                const double A2 = (double)(2 * nxy) + C2, B2 = (double)(nx + ny) + C2;
                acc += (A1 * A2) / (B1 * B2);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    __syncthreads();
    if ((t & 63) == 0) red[t >> 6] = acc;
    __syncthreads();
    if (t == 0)
        partial[((int64_t)f * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// fixed-order sum of a frame's partials -> mean SSIM (deterministic: no atomics)
__global__ void ssim_finish_kernel(const double *__restrict__ partial, int32_t per_frame, double count,
                                   double *__restrict__ ssim) {
    const int f = blockIdx.x;
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < per_frame; ++i) s += partial[(int64_t)f * per_frame + i];
        ssim[f] = s / count;
    }
}

// per-frame max - min of a plane (the data_range quirk of evaluation.calc_ssim, evaluation.py:26), in two steps:
// workgroups of SVS_RANGE_ROWS rows fold their bytes into lohi[frame] = {min, max} with integer atomics (exact and
// order-independent), then one thread per frame turns the pair into the double the SSIM kernel reads.
#define SVS_RANGE_ROWS 16
__global__ __launch_bounds__(256) void frame_minmax_kernel(const uint8_t *__restrict__ a, int32_t height, int32_t width,
                                                           int64_t row_pitch, int64_t frame_pitch,
                                                           uint32_t *__restrict__ lohi) {
    const int f = blockIdx.y, y0 = blockIdx.x * SVS_RANGE_ROWS;
    const int w8 = width / 8;  // width is a multiple of 8, rows are 8-byte aligned
    uint32_t lo = 0x00ff00ffu, hi = 0u;  // two 16-bit lanes each
    for (int y = y0; y < min(y0 + SVS_RANGE_ROWS, height); ++y) {
        const u32x2 *row = reinterpret_cast<const u32x2 *>(a + (int64_t)f * frame_pitch + (int64_t)y * row_pitch);
        for (int c = threadIdx.x; c < w8; c += 256) {
            const u32x2 v = SVS_LD(row + c);
            const uint32_t e0 = v.x & 0x00ff00ffu, o0 = (v.x >> 8) & 0x00ff00ffu;
            const uint32_t e1 = v.y & 0x00ff00ffu, o1 = (v.y >> 8) & 0x00ff00ffu;
            // packed 16-bit min / max (v_pk_min_u16 / v_pk_max_u16): four bytes per pair of instructions
            typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
            auto pk = [](uint32_t x) { return __builtin_bit_cast(u16x2, x); };
            u16x2 l = __builtin_elementwise_min(__builtin_elementwise_min(pk(e0), pk(o0)),
                                                __builtin_elementwise_min(pk(e1), pk(o1)));
            u16x2 h = __builtin_elementwise_max(__builtin_elementwise_max(pk(e0), pk(o0)),
                                                __builtin_elementwise_max(pk(e1), pk(o1)));
            lo = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(pk(lo), l));
            hi = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(pk(hi), h));
        }
    }
    uint32_t mn = min(lo & 0xffffu, lo >> 16), mx = max(hi & 0xffffu, hi >> 16);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = min(mn, (uint32_t)__shfl_down(mn, o, 64));
        mx = max(mx, (uint32_t)__shfl_down(mx, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&lohi[2 * f], mn);
        atomicMax(&lohi[2 * f + 1], mx);
    }
}

__global__ void frame_range_finish_kernel(const uint32_t *__restrict__ lohi, int32_t n_frames, double *__restrict__ range) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < n_frames) range[f] = (double)lohi[2 * f + 1] - (double)lohi[2 * f];
}

#if defined(SVS_EXPERIMENTS)   // measurement kernels behind the experiments library's svs_ref_* / svs_probe_* hooks
// 8-byte-per-lane copy (what the one-block-per-lane kernels issue): non-temporal load, write-through or non-temporal store
template <int SC1>
__global__ __launch_bounds__(256) void copy8_kernel(const u32x2 *__restrict__ src, u32x2 *__restrict__ dst, uint64_t n8) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n8) {
        const u32x2 v = __builtin_nontemporal_load(src + i);
        if constexpr (SC1) asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(dst + i), "v"(v) : "memory");
        else __builtin_nontemporal_store(v, dst + i);
    }
}

// mixed widths: which side of a copy is sensitive to the 8-byte access width?  SPLIT_LOAD: lane-strided 8-byte loads
// (lane i reads elements i and i + 64 of its wave's 1 KB) + one 16-byte store after a swap through LDS is not needed for
// the probe: the two halves are simply stored where they belong with the other width.
template <int WIDE_LOAD>
__global__ __launch_bounds__(256) void copy_mixed_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint64_t bytes) {
    // each wave moves 1 KB: either 64 x 16-byte loads + 2 x (64 x 8-byte) stores, or 2 x (64 x 8-byte) loads + 64 x 16-byte stores
    const uint64_t wave_base = ((uint64_t)blockIdx.x * 256u + (threadIdx.x & ~63u)) * 16u;
    const uint32_t lane = threadIdx.x & 63u;
    if (wave_base + 1024 > bytes) return;
    __shared__ __attribute__((aligned(16))) u32x4 buf[4][64];
    u32x4 *mine = buf[threadIdx.x >> 6];
    if constexpr (WIDE_LOAD) {
        mine[lane] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(src + wave_base) + lane);
        wave_lds_fence();
        const u32x2 *as8 = reinterpret_cast<const u32x2 *>(mine);
        const u32x2 a = as8[lane], b = as8[lane + 64];
        u32x2 *out = reinterpret_cast<u32x2 *>(dst + wave_base);
        asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(out + lane), "v"(a) : "memory");
        asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(out + lane + 64), "v"(b) : "memory");
    } else {
        const u32x2 *in = reinterpret_cast<const u32x2 *>(src + wave_base);
        u32x2 *as8 = reinterpret_cast<u32x2 *>(mine);
        as8[lane] = __builtin_nontemporal_load(in + lane);
        as8[lane + 64] = __builtin_nontemporal_load(in + lane + 64);
        wave_lds_fence();
        const u32x4 v = mine[lane];
        asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(reinterpret_cast<u32x4 *>(dst + wave_base) + lane), "v"(v) : "memory");
    }
}

// ---- reference streams for tools/ab_bench.py: what plain copies / reads reach on the same box ----
// mode 0: one 16-byte element per thread, non-temporal;  mode 1: grid-stride, 4 x 16 B in flight per
// thread, non-temporal;  mode 2: as 1 with default cache policy
template <int MODE>
__global__ __launch_bounds__(256) void copy_kernel(const u32x4 *__restrict__ src, u32x4 *__restrict__ dst, uint64_t n16) {
    if constexpr (MODE >= 3) {
        // cache-policy experiments on the one-shot copy: 3 = nt load + sc1 (write-through) store, 4 = nt load + sc0 sc1 nt
        // store, 5 = sc1 load + sc1 store
        const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
        if (i < n16) {
            u32x4 v;
            if constexpr (MODE == 5) asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(src + i) : "memory");
            else v = __builtin_nontemporal_load(src + i);
            if constexpr (MODE == 4) asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1 nt" ::"v"(dst + i), "v"(v) : "memory");
            else asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(dst + i), "v"(v) : "memory");
        }
    } else if constexpr (MODE == 0) {
        const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
        if (i < n16) __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
    } else {
        const uint64_t stride = (uint64_t)gridDim.x * 256u;
        uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
        for (; i + 3 * stride < n16; i += 4 * stride) {
            u32x4 a, b, c, d;
            if constexpr (MODE == 1) {
                a = __builtin_nontemporal_load(src + i); b = __builtin_nontemporal_load(src + i + stride);
                c = __builtin_nontemporal_load(src + i + 2 * stride); d = __builtin_nontemporal_load(src + i + 3 * stride);
                __builtin_nontemporal_store(a, dst + i); __builtin_nontemporal_store(b, dst + i + stride);
                __builtin_nontemporal_store(c, dst + i + 2 * stride); __builtin_nontemporal_store(d, dst + i + 3 * stride);
            } else {
                a = src[i]; b = src[i + stride]; c = src[i + 2 * stride]; d = src[i + 3 * stride];
                dst[i] = a; dst[i + stride] = b; dst[i + 2 * stride] = c; dst[i + 3 * stride] = d;
            }
        }
        for (; i < n16; i += stride) dst[i] = src[i];
    }
}

// read-only stream: xor-reduce, one dword written per workgroup (keeps the loads alive)
__global__ __launch_bounds__(256) void read_kernel(const u32x4 *__restrict__ src, uint32_t *__restrict__ sink, uint64_t n16) {
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    u32x4 acc = {0, 0, 0, 0};
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n16; i += stride)
        acc ^= __builtin_nontemporal_load(src + i);
    const uint32_t v = acc.x ^ acc.y ^ acc.z ^ acc.w;
    if (v == 0x12345678u) sink[blockIdx.x] = v;
}

// probe used by tests/test_gpu_primitives.py: what v_cvt_pk_u8_f32 does with a value
__global__ void probe_cvt_pk_u8_kernel(const float *__restrict__ in, uint32_t *__restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = __builtin_amdgcn_cvt_pk_u8_f32(in[i], 0, 0u);
}
#endif  // SVS_EXPERIMENTS

}  // namespace svs
