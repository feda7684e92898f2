// rs_emu.cpp - test-only host build of csrc/svs_rs.hpp: the decoder of include/svsrs.h and include/svsrse.h as the kernel of
// csrc/svs_rs_decode.hpp walks it - the LFSR over a codeword's bytes with the optional mask beside them, a list of at most 32
// erased bytes, and for a dirty codeword 64 "lanes" stepped one after the other through the syndromes, the erasure locator,
// Berlekamp-Massey, the root search and Forney - with every per-lane value coming from the header's functions.  Without a mask
// it is svs_rs_decode_dev, with one svs_rse_decode_dev.
// tests/rs_lib.py compiles it with g++ into a shared library (tests/rse_lib.py loads the same one); with -DRS_EMU_MAIN or
// -DRSE_EMU_MAIN it is a stand-alone program (its own main: errors only, or errors and erasures) that tests/test_rs_cpu.py and
// tests/test_rse_cpu.py build with -fsanitize=address,undefined and run once.
#include "svs_rs.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

using namespace svsrs;

constexpr Field kField = make_field();
constexpr Generator kGenerator = make_generator(kField);
constexpr LfsrTable kLfsr = make_lfsr(kField, kGenerator);
constexpr int kLanes = 64;
constexpr int kMaxErased = 32;

uint32_t repair(uint8_t *stream, uint64_t k, uint64_t C, uint64_t c, uint32_t k_c, const uint8_t *r, const uint8_t *list, int f) {
    const Gf gf{kField.exp2, kField.log};
    uint8_t syn[kParity], lambda[kParity + 1], omega[kParity];
    uint32_t map[8] = {0};
    const int n_c = (int)k_c + kParity;
    for (int lane = 0; lane < kParity; ++lane) syn[lane] = (uint8_t)syndrome(lane, r, gf);
    for (int lane = 0; lane < f; ++lane) {
        const int p = n_c - 1 - (int)list[lane];
        map[erased_word(p)] |= erased_bit(p);
    }

    uint32_t lam[kLanes] = {1};
    for (int t = 0; t < f; ++t) {
        uint32_t up[kLanes];
        for (int lane = 0; lane < kLanes; ++lane) up[lane] = lane == 0 ? 0u : lam[lane - 1];
        for (int lane = 0; lane < kLanes; ++lane) lam[lane] = gamma_step(lam[lane], up[lane], n_c - 1 - (int)list[t], gf);
    }
    uint32_t shifted_b[kLanes], b = 1;
    for (int lane = 0; lane < kLanes; ++lane) shifted_b[lane] = lane == 0 ? 0u : lam[lane - 1];
    int L = f;
    for (int n = f; n < kParity; ++n) {
        uint32_t d = 0;
        for (int lane = 0; lane < kLanes; ++lane) d ^= bm_term(lane, n, lam[lane], syn, gf);
        const bool longer = bm_longer(d, L, n, f);
        uint32_t pass[kLanes];
        for (int lane = 0; lane < kLanes; ++lane) {
            const BmLane next = bm_update(lam[lane], shifted_b[lane], d, b, longer, gf);
            lam[lane] = next.lambda;
            pass[lane] = next.pass;
        }
        for (int lane = 0; lane < kLanes; ++lane) shifted_b[lane] = lane == 0 ? 0u : pass[lane - 1];
        if (longer) {
            L = bm_length(L, n, f);
            b = d;
            if (bm_beyond(L, f)) return kUncorrectable;
        }
    }
    if (L < 1 || L > kParity || (f == 0 && L > kT)) abort();
    for (int lane = (f ? kParity : kT) + 1; lane < kLanes; ++lane)
        if (lam[lane]) abort();                                   // the lanes above L hold 0
    for (int lane = 0; lane <= kParity; ++lane) lambda[lane] = (uint8_t)lam[lane];
    for (int lane = 0; lane < kParity; ++lane) omega[lane] = (uint8_t)omega_coefficient(lane, L, lambda, syn, gf);

    std::vector<uint32_t> value((size_t)n_c);
    int roots = 0, changed = 0;
    bool bad = false;
    for (int p = 0; p < n_c; ++p) {
        value[p] = errata_value(p, L, lambda, omega, is_erased(map, p), gf);
        bad |= value[p] == kBadRoot;
        roots += value[p] != 0;
        if (value[p] >= 256u) value[p] = 0;
        changed += value[p] != 0;
    }
    if (roots != L || bad) return kUncorrectable;
    if (f == 0 && changed != L) abort();                          // with no erased position every root carries a value
    for (int p = 0; p < n_c; ++p)
        if (value[p]) stream[stream_offset(k, C, c, k_c, (uint32_t)(n_c - 1 - p))] ^= (uint8_t)value[p];
    return (uint32_t)changed;
}

}  // namespace

extern "C" {

// svs_rse_decode_dev on host memory, and with erased = NULL svs_rs_decode_dev: in place on k + 32 C bytes, erased (may be NULL)
// of the same size, C status bytes, counts (may be NULL) added to
int rs_emu_decode(uint8_t *stream, uint64_t k, const uint8_t *erased, uint8_t *status, uint32_t *counts) {
    if (k == 0) return 0;
    const uint64_t C = codewords(k), extra = k % C;
    const uint32_t rows = (uint32_t)(k / C);
    for (uint64_t c = 0; c < C; ++c) {
        uint32_t w[8] = {0}, f = 0;
        uint8_t list[kMaxErased];
        const uint32_t k_c = rows + (c < extra ? 1u : 0u);
        const auto note = [&](uint64_t at, uint32_t i) {
            if (erased && erased[at]) {
                if (f < (uint32_t)kMaxErased) list[f] = (uint8_t)i;
                ++f;
            }
        };
        uint64_t at = c;
        for (uint32_t i = 0; i < k_c; ++i, at += C) {
            lfsr_step(w, stream[at], &kLfsr.row[0][0]);
            note(at, i);
        }
        uint8_t r[kParity];
        bool dirty = false;
        at = k + c;
        for (int j = 0; j < kParity; ++j, at += C) {
            r[j] = (uint8_t)((w[j >> 2] >> (8 * (j & 3))) ^ stream[at]);
            dirty |= r[j] != 0;
            note(at, k_c + (uint32_t)j);
        }
        uint32_t st = 0;
        if (f > (uint32_t)kMaxErased) st = kUncorrectable;
        else if (dirty) st = repair(stream, k, C, c, k_c, r, list, (int)f);
        status[c] = (uint8_t)st;
        if (counts) {
            if (st == kUncorrectable) counts[1] += 1;
            else counts[0] += st;
        }
    }
    return 0;
}

// the encoder's LFSR, stepped as svs_rs_encode steps it
int rs_emu_encode(const uint8_t *data, uint64_t k, uint8_t *out) {
    const uint64_t C = codewords(k);
    memcpy(out, data, k);
    for (uint64_t c = 0; c < C; ++c) {
        uint32_t w[8] = {0};
        for (uint64_t i = c; i < k; i += C) lfsr_step(w, data[i], &kLfsr.row[0][0]);
        for (int j = 0; j < kParity; ++j) out[k + (uint64_t)j * C + c] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
    }
    return 0;
}

uint64_t rs_emu_data_bytes(uint64_t total) { return data_bytes(total); }
uint64_t rs_emu_coded_bytes(uint64_t k) { return coded_bytes(k); }
}

#if defined(RS_EMU_MAIN) || defined(RSE_EMU_MAIN)
// the stand-alone programs: each encodes, erases, corrupts and decodes in buffers of exactly the size a call may touch (a
// sanitizer sees one byte too many), and checks what the format promises: e errors and f erasures with 2 e + f <= 32 come back
// as sent with the status the bytes changed (f = 0: up to 16 errors, the status their number); 2 e + f = 33 is 255 with nothing
// written; more than 32 erasures are 255; whatever else decodes is a code word: decoding it again changes nothing
static uint32_t lcg(uint32_t *x) { return (*x = *x * 1664525u + 1013904223u) >> 8; }

// every length under every plan (f, e); a plan with f = 0 is decoded without a mask
static int run(const char *name, const int (*plans)[2], int n_plans) {
    const uint64_t lengths[] = {1, 2, 31, 222, 223, 224, 225, 445, 446, 447, 1000, 3000};
    uint32_t seed = 4321u;
    int runs = 0;
    for (uint64_t k : lengths)
        for (int plan = 0; plan < n_plans; ++plan) {
            const int f = plans[plan][0], e = plans[plan][1];
            const uint64_t C = codewords(k), total = coded_bytes(k);
            std::vector<uint8_t> data(k), sent(total), got(total), mask(total, 0), status(C);
            for (auto &v : data) v = (uint8_t)lcg(&seed);
            rs_emu_encode(data.data(), k, sent.data());
            got = sent;
            for (uint64_t c = 0; c < C; ++c) {                    // f + e distinct bytes of every codeword: all wrong, the first f erased
                const uint32_t k_c = (uint32_t)((k - c + C - 1) / C), n_c = k_c + kParity;
                std::vector<uint8_t> hit(n_c, 0);
                for (int t = 0; t < f + e && t < (int)n_c; ++t) {
                    uint32_t i = lcg(&seed) % n_c;
                    while (hit[i]) i = (i + 1) % n_c;
                    hit[i] = 1;
                    const uint64_t at = stream_offset(k, C, c, k_c, i);
                    got[at] ^= (uint8_t)(1 + lcg(&seed) % 255);
                    if (t < f) mask[at] = (uint8_t)(1 + lcg(&seed) % 255);
                }
            }
            const std::vector<uint8_t> received = got, mask_before = mask;
            uint32_t counts[2] = {5, 7};
            if (rs_emu_decode(got.data(), k, f ? mask.data() : nullptr, status.data(), counts) != 0) return printf("decode refused\n"), 1;
            if (mask != mask_before) return printf("the mask was written\n"), 1;
            uint32_t corrected = 0, failed = 0;
            for (uint64_t c = 0; c < C; ++c) {
                const uint32_t k_c = (uint32_t)((k - c + C - 1) / C), n_c = k_c + kParity;
                uint32_t changed = 0, wrong = 0;
                for (uint32_t i = 0; i < n_c; ++i) {
                    const uint64_t at = stream_offset(k, C, c, k_c, i);
                    changed += got[at] != received[at];
                    wrong += got[at] != sent[at];
                }
                const bool fits = f + e <= (int)n_c;              // every byte of the plan found a place
                if (fits && 2 * e + f <= kParity && (status[c] != (uint32_t)(f + e) || wrong))
                    return printf("k %llu, f %d, e %d: status %u, %u wrong\n", (unsigned long long)k, f, e, status[c], wrong), 1;
                if (fits && (2 * e + f == kParity + 1 || f > kMaxErased) && status[c] != kUncorrectable)
                    return printf("k %llu, f %d, e %d: status %u, not 255\n", (unsigned long long)k, f, e, status[c]), 1;
                if (status[c] == kUncorrectable ? changed != 0 : changed != status[c]) return printf("k %llu: status %u, %u changed\n", (unsigned long long)k, status[c], changed), 1;
                if (status[c] == kUncorrectable) ++failed;
                else corrected += status[c];
            }
            if (counts[0] != 5 + corrected || counts[1] != 7 + failed) return printf("counts\n"), 1;
            std::vector<uint8_t> again = got, status2(C);         // what decoded is a code word: decoding it again changes nothing
            rs_emu_decode(again.data(), k, nullptr, status2.data(), nullptr);
            for (uint64_t c = 0; c < C; ++c)
                if (status[c] != kUncorrectable && status2[c] != 0) return printf("k %llu: a decoded word is no code word\n", (unsigned long long)k), 1;
            if (again != got && failed == 0) return printf("k %llu: decoding a decoded stream changed it\n", (unsigned long long)k), 1;
            ++runs;
        }
    printf("%s emu ok: %d decodes\n", name, runs);
    return 0;
}

int main() {
#if defined(RS_EMU_MAIN)
    const int plans[][2] = {{0, 0}, {0, 1}, {0, 7}, {0, 16}, {0, 17}, {0, 20}, {0, 40}};   // f, e: errors only, no mask
    return run("rs", plans, 7);
#else
    const int plans[][2] = {{0, 0}, {0, 16}, {32, 0}, {1, 15}, {10, 11}, {31, 0}, {16, 8}, {1, 16}, {31, 1}, {17, 8}, {33, 0}, {0, 17}, {0, 40}};   // f, e
    return run("rse", plans, 13);
#endif
}
#endif
