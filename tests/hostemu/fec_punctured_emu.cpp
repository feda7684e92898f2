// fec_punctured_emu.cpp - test-only host build of the punctured codes of csrc/svs_fec.hpp: the window load of
// decode_punctured_kernel (csrc/svs_fec.hip) as its lanes walk it - S(ws) and ws mod P once a window, a lane's steps 32 apart,
// zeros at the unsent bits - with every value from the header's functions, and behind it the rate-2 segment decoder of
// fec_emu.cpp, which this file includes for that.  tests/fec_punctured_lib.py compiles it with g++ into a shared library; with
// -DFEC_PUNCTURED_EMU_MAIN it is a stand-alone program (its own main) that tests/test_fec_punctured_cpu.py builds with
// -fsanitize=address,undefined and runs once.
#include "fec_emu.cpp"

namespace {

template <typename In>
int decode_punctured(const In *in, uint64_t n_info, int code, uint8_t *out) {
    const Puncture pc = puncture(code);
    if (!pc.period) return -1;
    const uint64_t n = n_info + kTail, out_bytes = (n_info + 7) / 8, n_segments = (n_info + kSegment - 1) / kSegment;
    std::vector<int32_t> mother((size_t)kMotherRate * n);    // a weight per mother bit; a window fills its own part
    for (uint64_t seg = 0; seg < n_segments; ++seg) {
        const uint64_t a = seg * kSegment, ws = window_start(a), we = window_end(a, n);
        const int len = (int)(we - ws);
        const int phase = (int)(ws % (uint64_t)pc.period);
        const In *src = in + sent_before(pc, ws);
        for (int lane = 0; lane < 64; ++lane) {
            PunctStep at = punct_step(pc, phase + (lane >> 1));
            for (int i = lane; i < kMotherRate * len; i += 64) {
                const int k = sent_place(pc, phase, at, lane & 1);
                const int32_t v = weight_of(src[k < 0 ? 0 : k]);    // as the kernel: the lane of an unsent bit reads the run's first value
                mother[(size_t)kMotherRate * ws + i] = k < 0 ? 0 : v;
                at = punct_advance(pc, at, 32);
            }
        }
        decode_segment<kMotherRate, int32_t>(mother.data(), n_info, seg, out, out_bytes);
    }
    return 0;
}

}  // namespace

extern "C" {
int fec_punctured_emu_decode_soft(const uint8_t *soft, uint64_t n_info, int code, uint8_t *out) {
    return decode_punctured(soft, n_info, code, out);
}
int fec_punctured_emu_decode_weights(const int32_t *weights, uint64_t n_info, int code, uint8_t *out) {
    return decode_punctured(weights, n_info, code, out);
}
uint64_t fec_punctured_emu_sent_before(uint64_t t, int code) { return sent_before(puncture(code), t); }
uint64_t fec_punctured_emu_steps_that_fit(uint64_t capacity, int code) { return steps_that_fit(puncture(code), capacity); }
}

#if defined(FEC_PUNCTURED_EMU_MAIN)
// the stand-alone program: checks S and its inverse against a count, encodes with the header's step and keep test, decodes
// clean and noisy streams of both kinds from buffers of exactly n_sent values (a sanitizer sees one value too many), and checks
// the clean round trips
static uint32_t rnd(uint32_t *x) { return *x = *x * 1664525u + 1013904223u; }

int main() {
    const int codes[] = {23, 34, 56, 78};
    const uint64_t lengths[] = {1, 2, 58, 59, 506, 507, 570, 571, 1018, 1019, 1020, 1021, 1022, 1023, 1024, 1025, 2045, 5000};
    uint32_t seed = 4321u;
    int runs = 0;
    for (int code : codes) {
        const Puncture pc = puncture(code);
        uint64_t sent = 0;
        for (uint64_t t = 0; t < 300; ++t) {
            if (sent_before(pc, t) != sent) return printf("code %d: S(%llu) is wrong\n", code, (unsigned long long)t), 1;
            const uint64_t here = punct_kept(pc, (int)(t % pc.period), 0) + punct_kept(pc, (int)(t % pc.period), 1);
            if (here == 0) return printf("code %d: a step sends nothing\n", code), 1;
            for (uint64_t cap = sent; cap < sent + here; ++cap)
                if (steps_that_fit(pc, cap) != t) return printf("code %d: capacity %llu\n", code, (unsigned long long)cap), 1;
            sent += here;
        }
        for (uint64_t n_info : lengths) {
            const uint64_t n = n_info + kTail, nc = sent_before(pc, n);
            std::vector<uint8_t> info(n_info), soft(nc), out((n_info + 7) / 8);
            std::vector<int32_t> wide(nc);
            uint32_t s = 0;
            uint64_t at = 0;
            for (uint64_t t = 0; t < n; ++t) {
                const uint32_t x = t < n_info ? (info[t] = (rnd(&seed) >> 16) & 1u) : 0u;
                for (int j = 0; j < kMotherRate; ++j) {
                    if (!punct_kept(pc, (int)(t % pc.period), j)) continue;
                    const uint32_t c = output_bit(s, x, j), r = rnd(&seed) >> 8;
                    soft[at] = (uint8_t)((c << 7) | (r & 127u));
                    wide[at] = (r % 7 == 0) ? (c ? INT32_MAX : INT32_MIN) : (int32_t)((c ? 1 : -1) * (int32_t)(1 + r % 100000u));
                    ++at;
                }
                s = next_state(s, x);
            }
            if (s != 0 || at != nc) return printf("code %d: the encoder ends in state %u after %llu bits\n", code, s, (unsigned long long)at), 1;
            for (int kind = 0; kind < 3; ++kind) {
                memset(out.data(), 0xEE, out.size());
                if (kind == 2)                              // noise: flips at the lowest confidence
                    for (uint64_t i = 0; i < nc; i += 29) soft[i] = (uint8_t)((soft[i] & 0x80u) ^ 0x80u);
                const int rc = kind == 1 ? fec_punctured_emu_decode_weights(wide.data(), n_info, code, out.data())
                                         : fec_punctured_emu_decode_soft(soft.data(), n_info, code, out.data());
                if (rc != 0) return printf("decode refused\n"), 1;
                uint64_t wrong = 0;
                for (uint64_t t = 0; t < n_info; ++t) wrong += ((out[t >> 3] >> (7 - (t & 7))) & 1u) != info[t];
                if (n_info & 7 && (out.back() & (0xFFu >> (n_info & 7)))) return printf("pad bits set\n"), 1;
                if (kind < 2 && wrong)
                    return printf("code %d n_info %llu kind %d: %llu wrong\n", code, (unsigned long long)n_info, kind, (unsigned long long)wrong), 1;
                ++runs;
            }
        }
    }
    printf("fec punctured emu ok: %d decodes\n", runs);
    return 0;
}
#endif
