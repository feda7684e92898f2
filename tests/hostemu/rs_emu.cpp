// rs_emu.cpp - test-only host build of csrc/svs_rs.hpp: the decoder of include/svsrs.h as the kernel of csrc/svs_rs.hip walks it -
// the LFSR over a codeword's bytes, and for a dirty one 64 "lanes" stepped one after the other through the syndromes,
// Berlekamp-Massey, the root search and Forney - with every per-lane value coming from the header's functions.
// tests/rs_lib.py compiles it with g++ into a shared library; with -DRS_EMU_MAIN it is a stand-alone program (its own main)
// that tests/test_rs_cpu.py builds with -fsanitize=address,undefined and runs once.
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

uint32_t repair(uint8_t *stream, uint64_t k, uint64_t C, uint64_t c, uint32_t k_c, const uint8_t *r) {
    const Gf gf{kField.exp2, kField.log};
    uint8_t syn[kParity], lambda[kT + 1], omega[kT];
    for (int lane = 0; lane < kParity; ++lane) syn[lane] = (uint8_t)syndrome(lane, r, gf);

    uint32_t lam[kLanes] = {1}, shifted_b[kLanes] = {0, 1}, b = 1;
    int L = 0;
    for (int n = 0; n < kParity; ++n) {
        uint32_t d = 0;
        for (int lane = 0; lane < kLanes; ++lane) d ^= bm_term(lane, n, lam[lane], syn, gf);
        const bool longer = d != 0 && 2 * L <= n;
        uint32_t pass[kLanes];
        for (int lane = 0; lane < kLanes; ++lane) {
            const BmLane next = bm_update(lam[lane], shifted_b[lane], d, b, longer, gf);
            lam[lane] = next.lambda;
            pass[lane] = next.pass;
        }
        for (int lane = 0; lane < kLanes; ++lane) shifted_b[lane] = lane == 0 ? 0u : pass[lane - 1];
        if (longer) {
            L = n + 1 - L;
            b = d;
            if (L > kT) return kUncorrectable;
        }
    }
    for (int lane = kT + 1; lane < kLanes; ++lane)
        if (lam[lane]) abort();                                   // the lanes above L hold 0
    for (int lane = 0; lane <= kT; ++lane) lambda[lane] = (uint8_t)lam[lane];
    for (int lane = 0; lane < kT; ++lane) omega[lane] = (uint8_t)omega_coefficient(lane, L, lambda, syn, gf);

    const int n_c = (int)k_c + kParity;
    std::vector<uint32_t> value((size_t)n_c);
    int roots = 0;
    bool bad = false;
    for (int p = 0; p < n_c; ++p) {
        value[p] = root_value(p, L, lambda, omega, gf);
        bad |= value[p] == kBadRoot;
        roots += value[p] != 0;
    }
    if (roots != L || bad) return kUncorrectable;
    for (int p = 0; p < n_c; ++p)
        if (value[p]) stream[stream_offset(k, C, c, k_c, (uint32_t)(n_c - 1 - p))] ^= (uint8_t)value[p];
    return (uint32_t)L;
}

}  // namespace

extern "C" {

// svs_rs_decode_dev on host memory: in place on k + 32 C bytes, C status bytes, counts (may be NULL) added to
int rs_emu_decode(uint8_t *stream, uint64_t k, uint8_t *status, uint32_t *counts) {
    if (k == 0) return 0;
    const uint64_t C = codewords(k), extra = k % C;
    const uint32_t rows = (uint32_t)(k / C);
    for (uint64_t c = 0; c < C; ++c) {
        uint32_t w[8] = {0};
        const uint8_t *p = stream + c;
        for (uint32_t i = 0; i < rows; ++i, p += C) lfsr_step(w, *p, &kLfsr.row[0][0]);
        if (c < extra) lfsr_step(w, *p, &kLfsr.row[0][0]);
        uint8_t r[kParity];
        bool dirty = false;
        for (int j = 0; j < kParity; ++j) {
            r[j] = (uint8_t)((w[j >> 2] >> (8 * (j & 3))) ^ stream[k + (uint64_t)j * C + c]);
            dirty |= r[j] != 0;
        }
        const uint32_t st = dirty ? repair(stream, k, C, c, rows + (c < extra ? 1u : 0u), r) : 0u;
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

#if defined(RS_EMU_MAIN)
// the stand-alone program: encodes, corrupts and decodes in buffers of exactly the size a call may touch (a sanitizer sees one
// byte too many), and checks what the format promises: up to 16 errors a codeword come back as sent with the status their number;
// 17 and more never come back as something that is no code word
static uint32_t lcg(uint32_t *x) { return (*x = *x * 1664525u + 1013904223u) >> 8; }

int main() {
    const uint64_t lengths[] = {1, 2, 31, 222, 223, 224, 225, 445, 446, 447, 1000, 3000};
    uint32_t seed = 4321u;
    int runs = 0;
    for (uint64_t k : lengths)
        for (int errors : {0, 1, 7, 16, 17, 20, 40}) {
            const uint64_t C = codewords(k), total = coded_bytes(k);
            std::vector<uint8_t> data(k), sent(total), got(total), status(C);
            for (auto &v : data) v = (uint8_t)lcg(&seed);
            rs_emu_encode(data.data(), k, sent.data());
            got = sent;
            for (uint64_t c = 0; c < C; ++c) {                    // `errors` distinct bytes of every codeword
                const uint32_t k_c = (uint32_t)((k - c + C - 1) / C), n_c = k_c + kParity;
                std::vector<uint8_t> hit(n_c, 0);
                for (int e = 0; e < errors && e < (int)n_c; ++e) {
                    uint32_t i = lcg(&seed) % n_c;
                    while (hit[i]) i = (i + 1) % n_c;
                    hit[i] = 1;
                    got[stream_offset(k, C, c, k_c, i)] ^= (uint8_t)(1 + lcg(&seed) % 255);
                }
            }
            const std::vector<uint8_t> received = got;
            uint32_t counts[2] = {5, 7};
            if (rs_emu_decode(got.data(), k, status.data(), counts) != 0) return printf("decode refused\n"), 1;
            uint32_t corrected = 0, failed = 0;
            for (uint64_t c = 0; c < C; ++c) {
                const uint32_t k_c = (uint32_t)((k - c + C - 1) / C), n_c = k_c + kParity;
                uint32_t changed = 0, wrong = 0;
                for (uint32_t i = 0; i < n_c; ++i) {
                    const uint64_t at = stream_offset(k, C, c, k_c, i);
                    changed += got[at] != received[at];
                    wrong += got[at] != sent[at];
                }
                const int there = errors < (int)n_c ? errors : (int)n_c;
                if (there <= kT && (status[c] != there || wrong)) return printf("k %llu, %d errors: status %u, %u wrong\n", (unsigned long long)k, errors, status[c], wrong), 1;
                if (status[c] == kUncorrectable ? changed != 0 : changed != status[c]) return printf("k %llu: status %u, %u changed\n", (unsigned long long)k, status[c], changed), 1;
                if (status[c] == kUncorrectable) ++failed;
                else corrected += status[c];
            }
            if (counts[0] != 5 + corrected || counts[1] != 7 + failed) return printf("counts\n"), 1;
            std::vector<uint8_t> again = got, status2(C);         // what decoded is a code word: decoding it again changes nothing
            rs_emu_decode(again.data(), k, status2.data(), nullptr);
            for (uint64_t c = 0; c < C; ++c)
                if (status[c] != kUncorrectable && status2[c] != 0) return printf("k %llu: a decoded word is no code word\n", (unsigned long long)k), 1;
            ++runs;
        }
    printf("rs emu ok: %d decodes\n", runs);
    return 0;
}
#endif
