// svs_enc.hpp - what ONE LANE of the device encoders does (include/svsenc.h), in a form that compiles for the device
// (csrc/svs_enc.hip: a wave runs the lanes side by side) and for the host (tests/hostemu/enc_emu.cpp steps lane after lane).
// Three parts: the convolutional encoder of include/svsfec.h as word arithmetic - a window of the info stream, the xor network
// of a generator, the interleave of rates 2 and 3 and the compaction of a punctured period -, the Reed-Solomon encoder of
// include/svsrs.h as the walk of one codeword with svs_rs.hpp's own lfsr_step, and the source position of a tiled bit stream.
// A Reader is anything with `uint32_t operator()(uint64_t i) const`, byte i of a packed stream; no function here asks it for a
// byte behind the stream's last.  Integers only; every step and bit index is 64 bits wide (n_info reaches 2^40, a tiled stream
// 2^43 bits).
#pragma once

#include "svs_fec.hpp"
#include "svs_rs.hpp"

#if defined(__HIPCC__)
#define SVS_ENC_HD __host__ __device__ inline
#else
#define SVS_ENC_HD inline
#endif

namespace svsenc {

// the reader of a stream that lies in memory
struct Bytes {
    const uint8_t *p;
    SVS_ENC_HD uint32_t operator()(uint64_t i) const { return p[i]; }
};

// ---- packed bits, MSB first ---------------------------------------------------------------------------------------------------
// `count` <= 32 bits of a stream of n_bits from bit `pos` on, the first in bit 31, zeros behind them and zeros for every bit
// at or behind n_bits.  Reads the bytes that hold the bits asked for and are inside the stream, no others.
template <typename Reader>
SVS_ENC_HD uint32_t bits_at(const Reader &rd, uint64_t n_bits, uint64_t pos, int count) {
    if (count <= 0 || pos >= n_bits) return 0u;
    if ((uint64_t)count > n_bits - pos) count = (int)(n_bits - pos);
    const uint64_t first = pos >> 3, last = (pos + (uint64_t)count - 1) >> 3;        // at most five bytes
    uint64_t v = 0;
    for (int i = 0; i < 5; ++i) v = (v << 8) | (first + (uint64_t)i <= last ? (uint64_t)rd(first + (uint64_t)i) : 0u);
    const uint32_t word = (uint32_t)(v >> (8 - (int)(pos & 7)));                       // bit 39 - (pos & 7) of v is bit `pos`
    return word & (0xFFFFFFFFu << (32 - count));
}

// ---- the convolutional encoder -------------------------------------------------------------------------------------------------
// The window of step t0: bit 63 - i is x[t0 - 6 + i], i = 0 .. 8 NB - 8 and further where the bytes reach, x = 0 outside
// [0, n_info).  NB <= 8 bytes are read at most: enough for (8 NB - 13) steps at any bit phase.
template <int NB, typename Reader>
SVS_ENC_HD uint64_t info_window(const Reader &rd, uint64_t n_info, uint64_t t0) {
    static_assert(NB >= 1 && NB <= 8, "a window is at most eight bytes");
    // bit t0 - 6 may lie before the stream: count bytes from one byte before it, so that nothing is negative
    const uint64_t lead = t0 + 2;                                 // the place of x[t0 - 6] in the stream moved up by a byte
    const uint64_t v0 = lead >> 3, n_bytes = (n_info + 7) >> 3;
    uint64_t w = 0;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const uint64_t at = v0 + (uint64_t)i;                     // byte at - 1 of the stream
        const uint64_t b = at >= 1 && at - 1 < n_bytes ? (uint64_t)rd(at - 1) : 0u;
        w |= b << (56 - 8 * i);
    }
    w <<= (int)(lead & 7);
    // the bits at and behind n_info are no payload: the pad bits of the last byte are not read as zeros by anybody else
    const uint64_t from = v0 * 8 + (lead & 7);                    // = t0 + 2: bit 63 is stream bit `from` - 8
    if (n_info + 8 <= from) return 0;
    const uint64_t valid = n_info + 8 - from;                     // bits of the window before n_info
    return valid >= 64 ? w : w & ~(~0ull >> valid);
}

// out_j of the steps t0 + s from the window of t0: bit 63 - s.  x[t - d] of step t0 + s is bit 63 - s of w << (6 - d); the taps
// d of generator j are the set bits 6 - d of svsfec::generator(j) (reg = (x << 6) | s holds x[t - d] in bit 6 - d)
SVS_ENC_HD uint64_t mother_bits(uint64_t w, int j) {
    const uint32_t g = svsfec::generator(j);
    uint64_t out = 0;
    for (int d = 0; d <= 6; ++d)
        if ((g >> (6 - d)) & 1u) out ^= w << (6 - d);
    return out;
}

// the low 16 bits of v, bit i moved to bit 2 i
SVS_ENC_HD uint32_t spread16(uint32_t v) {
    v &= 0xFFFFu;
    v = (v | (v << 8)) & 0x00FF00FFu;
    v = (v | (v << 4)) & 0x0F0F0F0Fu;
    v = (v | (v << 2)) & 0x33333333u;
    v = (v | (v << 1)) & 0x55555555u;
    return v;
}

// the low 21 bits of v, bit i moved to bit 3 i
SVS_ENC_HD uint64_t spread21(uint64_t v) {
    v &= 0x1FFFFFull;
    v = (v | (v << 32)) & 0x001F00000000FFFFull;
    v = (v | (v << 16)) & 0x001F0000FF0000FFull;
    v = (v | (v << 8)) & 0x100F00F00F00F00Full;
    v = (v | (v << 4)) & 0x10C30C30C30C30C3ull;
    v = (v | (v << 2)) & 0x1249249249249249ull;
    return v;
}

// up to 96 sent bits, MSB first: bit i of the run is bit 31 - i % 32 of word i / 32
struct Sent {
    uint32_t word[3];
    int n;
    SVS_ENC_HD void push(uint32_t bits, int count) {             // `count` <= 32 bits, the first in bit count - 1
        if (count == 0) return;
        const int at = n >> 5, used = n & 31, room = 32 - used;
        if (count <= room) {
            word[at] |= bits << (room - count);
        } else {
            word[at] |= bits >> (count - room);
            word[at + 1] |= bits << (32 - (count - room));
        }
        n += count;
    }
};

// The unit of a lane: `steps` trellis steps that send `dwords` whole dwords, taken in chunks of `chunk` steps - a multiple of
// the period that one window of at most eight bytes serves
template <int CODE>
struct FecUnit;
template <> struct FecUnit<2> { static constexpr int steps = 16, chunk = 16, dwords = 1; };
template <> struct FecUnit<34> { static constexpr int steps = 24, chunk = 24, dwords = 1; };
template <> struct FecUnit<78> { static constexpr int steps = 28, chunk = 28, dwords = 1; };
template <> struct FecUnit<3> { static constexpr int steps = 32, chunk = 32, dwords = 3; };
template <> struct FecUnit<23> { static constexpr int steps = 64, chunk = 32, dwords = 3; };
template <> struct FecUnit<56> { static constexpr int steps = 80, chunk = 40, dwords = 3; };

// the sent bits of `count` whole periods of a punctured code from the mother bits o0, o1 (bit 63 - s: step s of the chunk)
template <int CODE>
SVS_ENC_HD void compact(uint64_t o0, uint64_t o1, int count, Sent *sent) {
    constexpr svsfec::Puncture pc = svsfec::puncture(CODE);
#pragma unroll
    for (int q = 0; q < count; ++q) {
        uint32_t kept = 0;
#pragma unroll
        for (int i = 0; i < pc.period; ++i) {
            const int s = q * pc.period + i;
            if (svsfec::punct_kept(pc, i, 0)) kept = (kept << 1) | (uint32_t)((o0 >> (63 - s)) & 1u);
            if (svsfec::punct_kept(pc, i, 1)) kept = (kept << 1) | (uint32_t)((o1 >> (63 - s)) & 1u);
        }
        sent->push(kept, pc.kept);
    }
}

// Unit u of the coded stream of n_info bits: the steps [u steps, (u + 1) steps) -> out[0 .. dwords), the first sent bit of the
// unit in bit 31 of out[0].  A step at or behind n_info + 6 sees nothing but zeros and sends zeros: the pad bits are 0 unasked.
template <int CODE, typename Reader>
SVS_ENC_HD void fec_unit(const Reader &rd, uint64_t n_info, uint64_t u, uint32_t *out) {
    using U = FecUnit<CODE>;
    constexpr int NB = (7 + 6 + U::chunk + 7) / 8;
    Sent sent{{0u, 0u, 0u}, 0};
#pragma unroll
    for (int c = 0; c < U::steps / U::chunk; ++c) {
        const uint64_t w = info_window<NB>(rd, n_info, u * (uint64_t)U::steps + (uint64_t)(c * U::chunk));
        const uint64_t o0 = mother_bits(w, 0), o1 = mother_bits(w, 1);
        if constexpr (CODE == 2) {
            sent.push((spread16((uint32_t)(o0 >> 48)) << 1) | spread16((uint32_t)(o1 >> 48)), 32);
        } else if constexpr (CODE == 3) {
            // 21 steps fill 63 bits, the other 11 the 33 behind them
            const uint64_t o2 = mother_bits(w, 2);
            const uint64_t head = spread21(o0 >> 43) << 3 | spread21(o1 >> 43) << 2 | spread21(o2 >> 43) << 1;
            const uint64_t rest = spread21((o0 >> 32) & 0x7FFu) << 33 | spread21((o1 >> 32) & 0x7FFu) << 32 | spread21((o2 >> 32) & 0x7FFu) << 31;
            sent.word[0] = (uint32_t)(head >> 32);
            sent.word[1] = (uint32_t)head | (uint32_t)(rest >> 63);
            sent.word[2] = (uint32_t)(rest >> 31);
        } else {
            compact<CODE>(o0, o1, U::chunk / svsfec::puncture(CODE).period, &sent);
        }
    }
#pragma unroll
    for (int i = 0; i < U::dwords; ++i) out[i] = sent.word[i];
}

// the sent bits a unit holds, and the units of a stream of n_coded sent bits
template <int CODE>
SVS_ENC_HD uint64_t fec_units(uint64_t n_coded) {
    return (n_coded + 32u * FecUnit<CODE>::dwords - 1) / (32u * FecUnit<CODE>::dwords);
}

// ---- the Reed-Solomon encoder: codeword c of a stream of k data bytes over C codewords, rows = k / C, extra = k % C ---------------
// Walks the data bytes data[c], data[c + C], .. with the LFSR (w: the remainder, 0 at the start; table: svsrs::LfsrTable's rows),
// eight rows at a time with every load ahead of the first step; the codewords c < extra take one more byte behind the loop.
// kCopy: each byte is also stored at the same offset of `copy` - the data part of an out-of-place stream.
template <bool kCopy>
SVS_ENC_HD void rs_walk(const uint8_t *data, uint8_t *copy, uint64_t C, uint32_t rows, uint64_t extra, uint64_t c, const uint32_t *table,
                        uint32_t *w) {
    uint64_t at = c;
    uint32_t i = 0;
    for (; i + 8 <= rows; i += 8, at += 8 * C) {
        uint32_t b[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) b[j] = data[at + (uint64_t)j * C];
        if (kCopy) {
#pragma unroll
            for (int j = 0; j < 8; ++j) copy[at + (uint64_t)j * C] = (uint8_t)b[j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) svsrs::lfsr_step(w, b[j], table);
    }
    for (; i < rows; ++i, at += C) {
        const uint32_t b = data[at];
        if (kCopy) copy[at] = (uint8_t)b;
        svsrs::lfsr_step(w, b, table);
    }
    if (c < extra) {                                             // at = rows * C + c, below k
        const uint32_t b = data[at];
        if (kCopy) copy[at] = (uint8_t)b;
        svsrs::lfsr_step(w, b, table);
    }
}
// parity byte j of the remainder, and where it goes: neighbouring codewords store neighbouring bytes
SVS_ENC_HD uint8_t rs_parity_byte(const uint32_t *w, int j) { return (uint8_t)(w[j >> 2] >> (8 * (j & 3))); }
SVS_ENC_HD uint64_t rs_parity_offset(uint64_t k, uint64_t C, uint64_t c, int j) { return k + (uint64_t)j * C + c; }

// ---- the tile: output bit i is input bit i mod period ------------------------------------------------------------------------------
// the residue of output dword d's first bit
SVS_ENC_HD uint64_t tile_residue(uint64_t d, uint64_t period) { return (d * 32u) % period; }
// Output dword d (the bits 32 d .. 32 d + 31, the first in bit 31) of n_out bits from its residue r: runs of the source from
// r to the period's end, then from 0 again - a dword spans several copies when the period is short.  Bits at and behind n_out
// are 0.
template <typename Reader>
SVS_ENC_HD uint32_t tile_dword(const Reader &rd, uint64_t period, uint64_t r, uint64_t d, uint64_t n_out) {
    uint32_t out = 0;
    int have = 0;
    while (have < 32) {
        const uint64_t left = period - r;
        const int run = left < (uint64_t)(32 - have) ? (int)left : 32 - have;
        out |= bits_at(rd, period, r, run) >> have;
        have += run;
        r += (uint64_t)run;
        if (r == period) r = 0;
    }
    const uint64_t first = d * 32u;
    if (n_out <= first) return 0u;
    return n_out - first >= 32 ? out : out & (0xFFFFFFFFu << (32 - (int)(n_out - first)));
}

}  // namespace svsenc
