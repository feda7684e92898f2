// enc_emu.cpp - test-only host build of csrc/svs_enc.hpp: the three device calls of include/svsenc.h as the kernels of
// csrc/svs_enc.hip walk them - one "lane" after the other, a unit of the coded stream, a codeword or an output dword each - with
// every value coming from the header's functions; and the same word functions on a synthetic stream (byte i is a hash of i), so
// that positions no buffer reaches - output bits near 2^32, 2^40 and 2^43 - can be asked for.
// tests/enc_lib.py compiles it with g++ into a shared library; with -DENC_EMU_MAIN it is a stand-alone program that
// tests/test_enc_cpu.py builds with -fsanitize=address,undefined and runs once.
#include "svs_enc.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

using namespace svsenc;

constexpr svsrs::Field kField = svsrs::make_field();
constexpr svsrs::Generator kGenerator = svsrs::make_generator(kField);
constexpr svsrs::LfsrTable kLfsr = svsrs::make_lfsr(kField, kGenerator);

// the synthetic stream: byte i
struct Hashed {
    uint32_t operator()(uint64_t i) const { return (uint32_t)(((i + 1) * 0x9E3779B97F4A7C15ull) >> 56); }
};

uint64_t coded_bits(uint64_t n_info, int rate) {
    const uint64_t n = n_info + svsfec::kTail;
    const svsfec::Puncture pc = svsfec::puncture(rate);
    return pc.period ? svsfec::sent_before(pc, n) : (uint64_t)rate * n;
}

// csrc/svs_enc.hip's store_dword
void store_dword(uint8_t *out, uint64_t at, uint64_t bytes, uint32_t word) {
    for (int b = 0; b < 4; ++b)
        if (at + (uint64_t)b < bytes) out[at + (uint64_t)b] = (uint8_t)(word >> (24 - 8 * b));
}

template <int CODE, typename Reader>
void encode_units(const Reader &rd, uint64_t n_info, uint8_t *out) {
    const uint64_t n_coded = coded_bits(n_info, CODE), bytes = (n_coded + 7) / 8, units = fec_units<CODE>(n_coded);
    for (uint64_t u = 0; u < units; ++u) {
        uint32_t word[3] = {0, 0, 0};
        fec_unit<CODE>(rd, n_info, u, word);
        for (int i = 0; i < FecUnit<CODE>::dwords; ++i) store_dword(out, (u * FecUnit<CODE>::dwords + (uint64_t)i) * 4u, bytes, word[i]);
    }
}

template <typename Reader>
int unit_of(const Reader &rd, uint64_t n_info, int rate, uint64_t u, uint32_t *out) {
    switch (rate) {
        case 2: fec_unit<2>(rd, n_info, u, out); return FecUnit<2>::dwords;
        case 3: fec_unit<3>(rd, n_info, u, out); return FecUnit<3>::dwords;
        case 23: fec_unit<23>(rd, n_info, u, out); return FecUnit<23>::dwords;
        case 34: fec_unit<34>(rd, n_info, u, out); return FecUnit<34>::dwords;
        case 56: fec_unit<56>(rd, n_info, u, out); return FecUnit<56>::dwords;
        case 78: fec_unit<78>(rd, n_info, u, out); return FecUnit<78>::dwords;
    }
    return -1;
}

}  // namespace

extern "C" {

// svs_fec_encode_dev: ceil(n_coded / 8) bytes to `out`
int enc_emu_fec_encode(const uint8_t *info, uint64_t n_info, int rate, uint8_t *out) {
    const Bytes rd{info};
    switch (rate) {
        case 2: encode_units<2>(rd, n_info, out); break;
        case 3: encode_units<3>(rd, n_info, out); break;
        case 23: encode_units<23>(rd, n_info, out); break;
        case 34: encode_units<34>(rd, n_info, out); break;
        case 56: encode_units<56>(rd, n_info, out); break;
        case 78: encode_units<78>(rd, n_info, out); break;
        default: return -1;
    }
    return 0;
}

// unit u of the coded stream of the first n_info bits of the synthetic stream -> out[0 .. 3); returns the unit's dwords
int enc_emu_fec_unit_hashed(uint64_t n_info, int rate, uint64_t u, uint32_t *out) { return unit_of(Hashed{}, n_info, rate, u, out); }
int enc_emu_unit_steps(int rate) {
    return rate == 2 ? FecUnit<2>::steps : rate == 3 ? FecUnit<3>::steps : rate == 23 ? FecUnit<23>::steps : rate == 34 ? FecUnit<34>::steps
           : rate == 56 ? FecUnit<56>::steps : rate == 78 ? FecUnit<78>::steps : -1;
}
uint32_t enc_emu_hashed_byte(uint64_t i) { return Hashed{}(i); }

// svs_rs_encode_dev: out == data encodes in place
int enc_emu_rs_encode(const uint8_t *data, uint64_t k, uint8_t *out) {
    if (k == 0) return 0;
    const uint64_t C = svsrs::codewords(k), extra = k % C;
    const uint32_t rows = (uint32_t)(k / C);
    for (uint64_t c = 0; c < C; ++c) {
        uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (out == data) rs_walk<false>(data, out, C, rows, extra, c, &kLfsr.row[0][0], w);
        else rs_walk<true>(data, out, C, rows, extra, c, &kLfsr.row[0][0], w);
        for (int j = 0; j < svsrs::kParity; ++j) out[rs_parity_offset(k, C, c, j)] = rs_parity_byte(w, j);
    }
    return 0;
}

// svs_bits_tile_dev: ceil(n_out / 8) bytes to `out`
int enc_emu_tile(const uint8_t *in, uint64_t period, uint8_t *out, uint64_t n_out) {
    if (period == 0) return -1;
    const uint64_t bytes = (n_out + 7) / 8, dwords = (n_out + 31) / 32;
    for (uint64_t d = 0; d < dwords; ++d) store_dword(out, d * 4u, bytes, tile_dword(Bytes{in}, period, tile_residue(d, period), d, n_out));
    return 0;
}

// output dword d of the synthetic stream's first `period` bits tiled to n_out bits
uint32_t enc_emu_tile_dword_hashed(uint64_t period, uint64_t d, uint64_t n_out) {
    return tile_dword(Hashed{}, period, tile_residue(d, period), d, n_out);
}

}  // extern "C"

#ifdef ENC_EMU_MAIN
namespace {

uint32_t bit_of(const std::vector<uint8_t> &p, uint64_t i) { return (p[i >> 3] >> (7 - (i & 7))) & 1u; }

// include/svsfec.h's encoder, one bit at a time
std::vector<uint8_t> serial_fec(const std::vector<uint8_t> &info, uint64_t n_info, int rate) {
    const svsfec::Puncture pc = svsfec::puncture(rate);
    std::vector<uint8_t> out((coded_bits(n_info, rate) + 7) / 8, 0);
    uint32_t s = 0;
    uint64_t at = 0;
    for (uint64_t t = 0; t < n_info + svsfec::kTail; ++t) {
        const uint32_t x = t < n_info ? bit_of(info, t) : 0u;
        for (int j = 0; j < (pc.period ? 2 : rate); ++j) {
            if (pc.period && !svsfec::punct_kept(pc, (int)(t % (uint64_t)pc.period), j)) continue;
            out[at >> 3] |= (uint8_t)(svsfec::output_bit(s, x, j) << (7 - (at & 7)));
            ++at;
        }
        s = svsfec::next_state(s, x);
    }
    return out;
}

}  // namespace

int main() {
    uint32_t seed = 12345;
    const auto next = [&]() { return (uint8_t)((seed = seed * 1664525u + 1013904223u) >> 24); };
    const int rates[6] = {2, 3, 23, 34, 56, 78};
    // exact-size heap buffers: a byte read or written behind one is the sanitizer's to find
    for (uint64_t n_info : {1ull, 2ull, 7ull, 8ull, 9ull, 25ull, 31ull, 32ull, 33ull, 58ull, 506ull, 1019ull, 5123ull}) {
        std::vector<uint8_t> info((n_info + 7) / 8);
        for (auto &b : info) b = next();                             // the pad bits of the last byte are not zeros
        for (int rate : rates) {
            const std::vector<uint8_t> want = serial_fec(info, n_info, rate);
            std::vector<uint8_t> got(want.size(), 0xEE);
            if (enc_emu_fec_encode(info.data(), n_info, rate, got.data()) != 0 || got != want) {
                std::printf("fec: n_info %llu rate %d differs\n", (unsigned long long)n_info, rate);
                return 1;
            }
        }
    }
    for (uint64_t k : {1ull, 222ull, 223ull, 224ull, 225ull, 447ull, 5000ull}) {
        std::vector<uint8_t> data(k);
        for (auto &b : data) b = next();
        const uint64_t C = svsrs::codewords(k), total = svsrs::coded_bytes(k);
        std::vector<uint8_t> want(total), got(total, 0xEE), in_place(total, 0xEE);
        for (uint64_t i = 0; i < k; ++i) want[i] = in_place[i] = data[i];
        for (uint64_t c = 0; c < C; ++c) {                           // svs_rs_encode's loop
            uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (uint64_t i = c; i < k; i += C) svsrs::lfsr_step(w, data[i], &kLfsr.row[0][0]);
            for (int j = 0; j < svsrs::kParity; ++j) want[k + (uint64_t)j * C + c] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
        }
        enc_emu_rs_encode(data.data(), k, got.data());
        enc_emu_rs_encode(in_place.data(), k, in_place.data());
        if (got != want || in_place != want) {
            std::printf("rs: k %llu differs\n", (unsigned long long)k);
            return 1;
        }
    }
    for (uint64_t period : {1ull, 7ull, 14ull, 31ull, 32ull, 33ull, 4794ull}) {
        std::vector<uint8_t> in((period + 7) / 8);
        for (auto &b : in) b = next();
        for (uint64_t n_out : {period - 1, period, period + 1, 3 * period + 5}) {
            if (n_out == 0) continue;
            std::vector<uint8_t> want((n_out + 7) / 8, 0), got(want.size(), 0xEE);
            for (uint64_t i = 0; i < n_out; ++i) want[i >> 3] |= (uint8_t)(bit_of(in, i % period) << (7 - (i & 7)));
            if (enc_emu_tile(in.data(), period, got.data(), n_out) != 0 || got != want) {
                std::printf("tile: period %llu n_out %llu differs\n", (unsigned long long)period, (unsigned long long)n_out);
                return 1;
            }
        }
    }
    uint32_t word[3];
    for (int rate : rates)
        for (uint64_t u : {(1ull << 32) / 96, (1ull << 40) / 32, (1ull << 41) / 32}) enc_emu_fec_unit_hashed(1ull << 40, rate, u, word);
    enc_emu_tile_dword_hashed((1ull << 43) - 11, (1ull << 38) - 1, 1ull << 43);
    std::printf("enc emu ok\n");
    return 0;
}
#endif
