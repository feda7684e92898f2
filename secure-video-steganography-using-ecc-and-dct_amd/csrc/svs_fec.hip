// svs_fec.hip - the C ABI declared in include/svsfec.h: the host encoder and the windowed Viterbi decoder for gfx950.
// Build: hipcc --offload-arch=gfx950 -O3 -shared -fPIC  (see csrc/Makefile)
//
// The decoder kernel: one wave decodes one segment, lane s owns trellis state s.
//   1. the window's weights are loaded coalesced, converted (soft byte or int32 -> int16) and kept in a run of LDS private to
//      the wave; every lane then reads a step's weights from the same address (a broadcast).  Under a punctured code the
//      window's run of sent values [S(ws), S(we)) is loaded and spread over the rate-2 run, zeros at the unsent bits
//      (decode_punctured_kernel; profiles/fec_punctured_resources.txt); nothing behind the load knows of it.
//   2. add-compare-select: two cross-lane reads of the predecessors' metrics (ds_bpermute), one add, one subtract, a compare
//      and a select.  The signs of a lane's branch metric are lane constants.  The 64 decisions of a step are one ballot word;
//      lane i of the wave collects the word of step 64 c + i, and every 64 steps the words go to the wave's run of LDS in one
//      store.
//   3. traceback: the state is wave-uniform; the words come back 64 at a time, one per lane, and are read lane by lane.  The
//      512 bits of the segment leave as 64 bytes, one per lane, in one coalesced store: a segment starts on a byte boundary,
//      so no two waves write the same byte and no atomics are needed.  The last, partial segment masks its tail.
// LDS per wave: 640 words of 8 bytes and 640 * RATE int16.  No global atomics, no scratch (profiles/fec_resources.txt).
#include "svsfec.h"
#include "svs_enc_args.hpp"   // and svs_abi.hpp: fail(), launched()
#include "svs_fec.hpp"

namespace {

using svsfec::kRates;
using svsfec::punctured;
using svsfec::rate_ok;
using svsfec::stream_bits;

constexpr int kWavesPerGroup = 4;
constexpr int kThreads = 64 * kWavesPerGroup;

}  // namespace

namespace svsfec {

// CODE = 0: the RATE coded bits of every step are there.  CODE = a punctured code (RATE is 2): the window's run of sent values is
// spread over the wave's weights on the way in, zeros where a bit was not sent; everything behind the load is the same code.
template <int RATE, int CODE, typename In>
__device__ __forceinline__ void decode_segment(const In *__restrict__ in, uint64_t n_info, uint64_t n_segments,
                                               uint8_t *__restrict__ out, uint64_t out_bytes) {
    __shared__ uint64_t s_dec[kWavesPerGroup][kWindow];
    __shared__ int16_t s_w[kWavesPerGroup][kWindow * RATE];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t seg = (uint64_t)blockIdx.x * kWavesPerGroup + wave;
    const bool live = seg < n_segments;                  // wave-uniform; a wave without a segment only meets the barriers
    const uint64_t n = n_info + kTail;
    const uint64_t a = seg * kSegment;
    const uint64_t ws = window_start(a), we = live ? window_end(a, n) : ws;
    const int len = (int)(we - ws);                      // 1 .. 640 for a live wave
    int16_t *w = s_w[wave];
    uint64_t *dec = s_dec[wave];

    if constexpr (CODE == 0) {
        if (live) {
            const In *src = in + (uint64_t)RATE * ws;    // the last window ends at coded bit RATE * n - 1
            for (int i = lane; i < RATE * len; i += 64) w[i] = (int16_t)weight_of(src[i]);
        }
    } else {
        static_assert(RATE == kMotherRate, "a punctured code is the rate-2 code");
        if (live) {
            // the window reads the sent values [S(ws), S(we)): the last window ends at sent value S(n) - 1.  ws is wave-uniform,
            // so S(ws) and ws mod P are two divisions by a constant a wave; a lane owns out_(lane & 1) of the steps
            // (lane >> 1) + 32 k and walks the period 32 steps at a time.  The lanes of sent bits read neighbouring values.
            constexpr Puncture pc = puncture(CODE);
            const int phase = (int)(ws % (uint64_t)pc.period);
            const In *src = in + sent_before(pc, ws);
            PunctStep at = punct_step(pc, phase + (lane >> 1));
#pragma unroll 4
            for (int i = lane; i < RATE * len; i += 64) {
                // no branch around the load: the lane of an unsent bit reads the run's first value (a step sends at least one
                // bit, so the run is not empty) and keeps 0, and the loads of several rounds can be in flight together
                const int k = sent_place(pc, phase, at, lane & 1);
                const int32_t v = weight_of(src[k < 0 ? 0 : k]);
                w[i] = (int16_t)(k < 0 ? 0 : v);
                at = punct_advance(pc, at, 32);
            }
        }
    }
    __syncthreads();

    int32_t m = start_metric(ws, (uint32_t)lane);
    if (live) {
        const int from0 = 4 * (int)pred0((uint32_t)lane);           // ds_bpermute addresses a lane by 4 * its number
        const int sign[3] = {branch_sign(lane, 0), branch_sign(lane, 1), branch_sign(lane, 2)};
        for (int base = 0; base < len; base += 64) {
            const int count = len - base < 64 ? len - base : 64;
            uint64_t keep = 0;                                       // lane i: the decisions of step base + i
            for (int i = 0; i < count; ++i) {
                const int16_t *wt = w + RATE * (base + i);
                const int32_t ww[3] = {wt[0], wt[1], RATE == 3 ? wt[2] : 0};
                const int32_t bm = branch_metric<RATE>(sign, ww);
                const int32_t m0 = __builtin_amdgcn_ds_bpermute(from0, m);
                const int32_t m1 = __builtin_amdgcn_ds_bpermute(from0 + 4, m);
                uint32_t d;
                m = acs(m0, m1, bm, &d);
                const uint64_t word = __ballot(d);
                keep = lane == i ? word : keep;
            }
            if (lane < count) dec[base + lane] = keep;
        }
    }
    __syncthreads();

    if (!live) return;
    uint32_t s = 0;
    if (we != n) {                                       // the lowest-numbered state with the largest metric
        int32_t best = m;
        for (int o = 32; o; o >>= 1) {
            const int32_t other = __shfl_xor(best, o);
            best = other > best ? other : best;
        }
        s = (uint32_t)(__ffsll((unsigned long long)__ballot(m == best)) - 1);
    }
    s = (uint32_t)__builtin_amdgcn_readfirstlane((int)s);
    const int lead = a > 0 ? 1 : 0;                      // a - ws is 0 or 64: whole words of the window lie before the segment
    uint64_t mine = 0;                                   // lane i: the word that holds byte i of the segment
    for (int base = ((len - 1) >> 6) << 6; base >= 64 * lead; base -= 64) {
        const int count = len - base < 64 ? len - base : 64;
        const uint64_t word = lane < count ? dec[base + lane] : 0;
        const int lo = (int)(uint32_t)word, hi = (int)(uint32_t)(word >> 32);
        uint64_t bits = 0;
        for (int i = count - 1; i >= 0; --i) {
            const uint64_t d = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(hi, i) << 32) | (uint32_t)__builtin_amdgcn_readlane(lo, i);
            bits |= (uint64_t)trace_step(d, &s) << i;
        }
        if ((lane >> 3) == (base >> 6) - lead) mine = bits;
    }
    // bit k of the word is step 8 (lane & ~7) + k; the byte wants its first step in bit 7
    uint32_t byte = __brev((uint32_t)(mine >> (8 * (lane & 7))) & 0xFFu) >> 24;
    const uint64_t at = seg * (kSegment / 8) + (uint64_t)lane;
    if (at < out_bytes) {
        if (at == out_bytes - 1 && (n_info & 7)) byte &= 0xFF00u >> (n_info & 7);   // the pad bits of the last byte are 0
        out[at] = (uint8_t)byte;
    }
}

template <int RATE, typename In>
__global__ __launch_bounds__(kThreads) void decode_kernel(const In *__restrict__ in, uint64_t n_info, uint64_t n_segments,
                                                           uint8_t *__restrict__ out, uint64_t out_bytes) {
    decode_segment<RATE, 0, In>(in, n_info, n_segments, out, out_bytes);
}

// `in` holds S(n) values, one per sent bit of punctured code CODE
template <int CODE, typename In>
__global__ __launch_bounds__(kThreads) void decode_punctured_kernel(const In *__restrict__ in, uint64_t n_info, uint64_t n_segments,
                                                                     uint8_t *__restrict__ out, uint64_t out_bytes) {
    decode_segment<kMotherRate, CODE, In>(in, n_info, n_segments, out, out_bytes);
}

}  // namespace svsfec

namespace {

template <typename In>
int decode(const In *d_in, uint64_t n_info, int rate, uint8_t *d_out, uint64_t out_capacity_bytes, void *stream, const char *what) {
    if (!rate_ok(rate)) return fail(SVS_ERR_INVALID_ARG, "%s: rate %d is %s", what, rate, kRates);
    if (n_info == 0) return SVS_OK;
    if (n_info > SVS_FEC_MAX_INFO_BITS)
        return fail(SVS_ERR_INVALID_ARG, "%s: n_info %llu exceeds SVS_FEC_MAX_INFO_BITS", what, (unsigned long long)n_info);
    if (!d_in || !d_out) return fail(SVS_ERR_INVALID_ARG, "%s: NULL pointer", what);
    if (sizeof(In) == 4 && ((uintptr_t)d_in & 3u)) return fail(SVS_ERR_INVALID_ARG, "%s: weights are not 4-byte aligned", what);
    const uint64_t out_bytes = (n_info + 7) / 8;
    if (out_capacity_bytes < out_bytes)
        return fail(SVS_ERR_CAPACITY, "%s: the output holds %llu bytes, the call writes %llu", what,
                    (unsigned long long)out_capacity_bytes, (unsigned long long)out_bytes);
    const uint64_t n_segments = (n_info + svsfec::kSegment - 1) / svsfec::kSegment;   // segments behind n_info hold tail steps only
    const uint64_t groups = (n_segments + kWavesPerGroup - 1) / kWavesPerGroup;       // at most 2^29 at SVS_FEC_MAX_INFO_BITS
    hipStream_t st = (hipStream_t)stream;
    svsfec::with_rate(rate, [&](auto code) {
        constexpr int kCode = decltype(code)::value;
        void (*kernel)(const In *, uint64_t, uint64_t, uint8_t *, uint64_t);
        if constexpr (kCode <= 3) kernel = svsfec::decode_kernel<kCode, In>;
        else kernel = svsfec::decode_punctured_kernel<kCode, In>;
        hipLaunchKernelGGL(kernel, dim3((uint32_t)groups), dim3(kThreads), 0, st, d_in, n_info, n_segments, d_out, out_bytes);
    });
    return launched(what);
}

}  // namespace

extern "C" {

int svs_fec_abi_version(void) { return SVS_FEC_ABI_VERSION; }

const char *svs_fec_last_error(void) { return g_last_error.c_str(); }

uint64_t svs_fec_coded_bits(uint64_t n_info, int rate) {
    if (!rate_ok(rate) || n_info > SVS_FEC_MAX_INFO_BITS) return 0;
    return stream_bits(n_info + SVS_FEC_TAIL, rate);
}

uint64_t svs_fec_info_bits(uint64_t capacity_bits, int rate) {
    if (!rate_ok(rate)) return 0;
    const uint64_t steps = punctured(rate) ? svsfec::steps_that_fit(svsfec::puncture(rate), capacity_bits) : capacity_bits / (uint64_t)rate;
    return steps > SVS_FEC_TAIL ? steps - SVS_FEC_TAIL : 0;
}

int svs_fec_encode(const uint8_t *info_packed, uint64_t n_info, int rate, uint8_t *coded_packed_out, uint64_t capacity_bytes,
                   uint64_t *n_coded_out) {
    uint64_t n_coded = 0;
    const int rc = fec_encode_args("svs_fec_encode", info_packed, n_info, rate, coded_packed_out, capacity_bytes, false, &n_coded);
    if (rc != kEncode) {
        if (rc == SVS_OK && n_coded_out) *n_coded_out = 0;
        return rc;
    }
    const uint64_t n = n_info + SVS_FEC_TAIL;
    uint32_t s = 0, acc = 0;
    uint64_t at = 0;                                     // coded bits written so far
    const svsfec::Puncture pc = svsfec::puncture(rate);  // period 0: every bit of a step is sent
    const int outputs = pc.period ? svsfec::kMotherRate : rate;
    int step = 0;                                        // t mod P
    for (uint64_t t = 0; t < n; ++t) {
        const uint32_t x = t < n_info ? (info_packed[t >> 3] >> (7 - (t & 7))) & 1u : 0u;
        for (int j = 0; j < outputs; ++j) {
            if (pc.period && !svsfec::punct_kept(pc, step, j)) continue;
            acc = (acc << 1) | svsfec::output_bit(s, x, j);
            if ((++at & 7) == 0) {
                coded_packed_out[(at >> 3) - 1] = (uint8_t)acc;
                acc = 0;
            }
        }
        s = svsfec::next_state(s, x);
        if (pc.period && ++step == pc.period) step = 0;
    }
    if (at & 7) coded_packed_out[at >> 3] = (uint8_t)(acc << (8 - (at & 7)));
    if (n_coded_out) *n_coded_out = n_coded;
    return SVS_OK;
}

int svs_fec_decode_soft_dev(const uint8_t *d_soft, uint64_t n_info, int rate, uint8_t *d_info_packed_out, uint64_t out_capacity_bytes,
                            void *stream) {
    return decode<uint8_t>(d_soft, n_info, rate, d_info_packed_out, out_capacity_bytes, stream, "svs_fec_decode_soft_dev");
}

int svs_fec_decode_weights_dev(const int32_t *d_weights, uint64_t n_info, int rate, uint8_t *d_info_packed_out,
                               uint64_t out_capacity_bytes, void *stream) {
    return decode<int32_t>(d_weights, n_info, rate, d_info_packed_out, out_capacity_bytes, stream, "svs_fec_decode_weights_dev");
}

}  // extern "C"
