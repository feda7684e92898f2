// svs_rs_decode.hpp - the one Reed-Solomon decoder kernel for gfx950 and the host side of a *_decode_dev call.  Two libraries are
// built from it: libsvsrs.so (csrc/svs_rs.hip, svs_rs_decode_dev: errors only, the instantiation without a mask) and libsvsrse.so
// (csrc/svs_rse.hip, svs_rse_decode_dev: with a mask of erased bytes, both instantiations).  Both are loaded into one process, so
// EVERYTHING HERE HAS INTERNAL LINKAGE - one anonymous namespace around the kernel, the device tables, the last-error string (csrc/svs_abi.hpp)
// and the host functions: the same named kernel stub or __device__ variable defined in two shared objects would be interposed by the dynamic
// linker, and each library keeps a last-error string of its own.
//
// The kernel, one launch; a workgroup is four waves and owns 64 codewords:
//   1. screening, one lane per codeword, on the workgroup's first wave.  Lane c walks codeword c with the encoder's own LFSR
//      (svs_rs.hpp): 32 remainder bytes in 8 registers, the 32 products of the feedback byte from a 256 x 32-byte table in LDS
//      (two 16-byte reads).  With the stream's interleave the lanes c .. c + 63 read neighbouring bytes at every step, so every
//      load is one coalesced run; the address advances by C a step (64-bit, no division).  The k mod C codewords with one more
//      data byte take it under a predicate behind the loop (a zero remainder does not change under a zero byte, so "one more at
//      the end" is "one more in the first row").  The parity bytes are xored in: r(x) = c(x) mod g(x).
//      With a mask (kMask) the lane walks it beside the stream: a second coalesced byte load at the same offsets.  Each erased
//      byte's number within the codeword goes into a 32-byte list of the lane's own in LDS (64 x 32 B) and is counted: f.
//      f > 32: status 255 at once, whatever the remainder.  r = 0 with f <= 32: the codeword is clean, status 0, done - the
//      pass every codeword pays for.
//      The bytes are taken eight rows at a time, all sixteen loads issued before the first is used, and the eight mask bytes
//      are looked at one by one only where their OR is not 0.  With a test and a possible LDS store behind every mask byte the
//      compiler kept each load behind the branch of the one before, and the clean pass with a mask took 0.102 ms where the pass
//      without one takes 0.029; in batches it takes 0.039 ms for twice the bytes (profiles/rse_rates.txt).
//   2. repair.  A dirty lane puts its lane number and r into a worklist in LDS (its f and its list stay where the lane wrote
//      them and are found through the lane number); behind a barrier the four waves take the entries in turn, ONE WAVE A
//      CODEWORD: S_j = r(alpha^j) on lanes 0 .. 31 (no second pass over the data); Gamma(x) on the lanes 0 .. 32 with f
//      multiply-and-shift steps, and a 256-bit map of the erased positions in LDS; Berlekamp-Massey from Lambda = Gamma at step
//      n = f with Lambda and B one coefficient a lane and the discrepancy a cross-lane xor (term 32 is always 0, i <= n <= 31, so
//      the xor runs over 32 lanes), left as soon as 2 L - f > 32; Omega's 32 coefficients; the root search over the k_c + 32
//      positions 64 at a time with Forney's value on the lanes that found a root, the map telling a lane whether a zero value is
//      a right byte (erased) or a failure.  The status is the number of non-zero values.  Nothing is stored before every root is
//      in and counted: a codeword that fails is not written.  The byte stores go to the codeword's own addresses, which no other
//      wave touches: no race, no atomics.  Without a mask f is 0 at compile time: no list, no locator steps, errors only.
//      A repair is a chain of dependent LDS reads (logarithm, antilogarithm, cross-lane xor), about 10^5 cycles a codeword, so
//      it is waves in flight that pay: with 256 codewords a workgroup (every wave screening) a stream of 64 k codewords is 1 000
//      waves, one a SIMD, and the all-dirty stream took 2.77 ms; with 64 a workgroup three more waves a workgroup wait at the
//      barrier while the first screens - the clean pass has the same 1 000 screening waves and the same 0.029 ms - and repair
//      with it: 0.78 ms on the first, errors-only kernel (DESIGN_HISTORY.md, Part 0), 0.71 ms on this one (profiles/rs_rates.txt).
//   3. the counters.  Adding to d_counts once a codeword is 64 k atomics on one address in a row when every codeword is dirty;
//      a wave sums what it repaired in a register instead and adds once at its end, and only what is not 0 (at most 8 atomics a
//      workgroup, none on a clean stream); the first wave also adds the codewords it refused for f > 32.  The sums are the same.
// LDS 13.7 KB a workgroup with the mask, 11.6 KB without, no scratch, no global atomics beside those two adds
// (profiles/rs_resources.txt, profiles/rse_resources.txt).
#pragma once

#include "svsrs.h"
#include "svs_abi.hpp"
#include "svs_rs.hpp"

namespace {

using namespace svsrs;

constexpr int kWavesPerGroup = 4;
constexpr int kThreads = 64 * kWavesPerGroup;
constexpr int kScreened = 64;                     // codewords a workgroup owns: its first wave screens them
constexpr int kMaxErased = kParity;               // SVS_RSE_MAX_ERASED of include/svsrse.h
// a wave's scratch: syn[32], omega[32], the map (8 words), lambda[33]
constexpr int kScratch = 136;

__device__ const Field d_field = make_field();
__device__ const LfsrTable d_lfsr = make_lfsr(make_field(), make_generator(make_field()));

// a wave's lanes see each other's LDS stores
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// wave-uniform: the xor of v over the lanes 0 .. 31
__device__ __forceinline__ uint32_t xor_of_32(uint32_t v) {
    for (int o = 16; o; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// One wave repairs codeword c (k_c data bytes) from its remainder r and its f <= 32 erased bytes (list: their numbers within the
// codeword).  scratch: kScratch bytes of LDS private to the wave, 4-byte aligned.
// Returns the status: the bytes changed, or kUncorrectable with nothing written.
__device__ __forceinline__ uint32_t repair(uint8_t *stream, uint64_t k, uint64_t C, uint64_t c, uint32_t k_c, const uint8_t *r,
                                           const uint8_t *list, int f, uint8_t *scratch, const Gf &gf, int lane) {
    uint8_t *syn = scratch, *omega = scratch + 32, *lambda = scratch + 96;
    uint32_t *map = reinterpret_cast<uint32_t *>(scratch + 64);
    const int n_c = (int)k_c + kParity;                  // at most 255
    if (lane < kParity) syn[lane] = (uint8_t)syndrome(lane, r, gf);
    if (lane < 8) map[lane] = 0;
    wave_sync();
    if (lane < f) {
        const int p = n_c - 1 - (int)list[lane];
        atomicOr(&map[erased_word(p)], erased_bit(p));   // LDS; the result is not used
    }

    uint32_t lam = lane == 0;                            // Gamma, then Lambda
    for (int t = 0; t < f; ++t) {                        // wave-uniform
        const uint32_t up = (uint32_t)__shfl_up((int)lam, 1);
        lam = gamma_step(lam, lane == 0 ? 0u : up, n_c - 1 - (int)list[t], gf);
    }
    uint32_t shifted_b = (uint32_t)__shfl_up((int)lam, 1), b = 1;
    if (lane == 0) shifted_b = 0;
    int L = f;
    for (int n = f; n < kParity; ++n) {
        const uint32_t d = xor_of_32(bm_term(lane, n, lam, syn, gf));
        const bool longer = bm_longer(d, L, n, f);
        const BmLane next = bm_update(lam, shifted_b, d, b, longer, gf);
        lam = next.lambda;
        const uint32_t up = (uint32_t)__shfl_up((int)next.pass, 1);
        shifted_b = lane == 0 ? 0u : up;
        if (longer) {
            L = bm_length(L, n, f);
            b = d;
            if (bm_beyond(L, f)) return kUncorrectable;  // wave-uniform
        }
    }
    // 1 <= L <= 32: a dirty codeword has f >= 1 or syndromes that are not all 0
    if (lane <= kParity) lambda[lane] = (uint8_t)lam;    // the lanes above L hold 0
    wave_sync();
    if (lane < kParity) omega[lane] = (uint8_t)omega_coefficient(lane, L, lambda, syn, gf);
    wave_sync();

    uint32_t values = 0;                                 // byte q: this lane's value of round q, 0: nothing to change
    int roots = 0, changed = 0;
    bool bad = false;
    for (int q = 0; q < 4; ++q) {
        const int p = 64 * q + lane;
        const uint32_t v = p < n_c ? errata_value(p, L, lambda, omega, is_erased(map, p), gf) : 0u;
        bad |= v == kBadRoot;
        roots += __popcll(__ballot(v != 0));
        const uint32_t change = v < 256u ? v : 0u;
        changed += __popcll(__ballot(change != 0));
        values |= change << (8 * q);
    }
    if (roots != L || __ballot(bad) != 0) return kUncorrectable;
    for (int q = 0; q < 4; ++q) {
        const uint32_t v = (values >> (8 * q)) & 0xFFu;
        if (v) {
            const uint32_t i = (uint32_t)(n_c - 1 - (64 * q + lane));          // the byte that multiplies x^p is byte n_c - 1 - p
            uint8_t *at = stream + stream_offset(k, C, c, k_c, i);
            *at = (uint8_t)(*at ^ v);
        }
    }
    return (uint32_t)changed;
}

// rows = k / C and extra = k % C: the codewords c < extra hold rows + 1 data bytes, the others rows.  kMask: erased is not NULL
template <bool kMask>
__global__ __launch_bounds__(kThreads) void rse_decode_kernel(uint8_t *stream, uint64_t k, uint64_t C, uint32_t rows, uint64_t extra,
                                                               const uint8_t *erased, uint8_t *status, uint32_t *counts) {
    __shared__ __attribute__((aligned(32))) uint32_t s_lfsr[256 * 8];
    __shared__ __attribute__((aligned(32))) uint32_t s_rem[kScreened][8];    // the worklist: the remainder ..
    __shared__ uint8_t s_who[kScreened];                                      // .. and the lane it came from
    __shared__ __attribute__((aligned(4))) uint8_t s_list[kScreened][kMaxErased];   // by lane: the erased bytes' numbers ..
    __shared__ uint8_t s_f[kScreened];                                        // .. and how many, at most 32 for a worklist entry
    __shared__ __attribute__((aligned(4))) uint8_t s_exp2[512];
    __shared__ __attribute__((aligned(4))) uint8_t s_log[256];
    __shared__ __attribute__((aligned(8))) uint8_t s_scratch[kWavesPerGroup][kScratch];
    __shared__ uint32_t s_count;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    {
        const uint32_t *src = &d_lfsr.row[0][0];
        for (int i = tid; i < 256 * 8; i += kThreads) s_lfsr[i] = src[i];
        const uint32_t *e = reinterpret_cast<const uint32_t *>(d_field.exp2), *l = reinterpret_cast<const uint32_t *>(d_field.log);
        if (tid < 128) reinterpret_cast<uint32_t *>(s_exp2)[tid] = e[tid];
        else if (tid < 192) reinterpret_cast<uint32_t *>(s_log)[tid - 128] = l[tid - 128];
        if (tid == 0) s_count = 0;
    }
    __syncthreads();

    const uint64_t first = (uint64_t)blockIdx.x * kScreened;
    const uint64_t c = first + (uint64_t)tid;
    const bool active = tid < kScreened && c < C;
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t f = 0;
    if (active) {
        uint8_t *list = s_list[tid];
        const auto note = [&](uint64_t at, uint32_t i) {         // byte i of the codeword lies at stream[at]
            if (kMask && erased[at]) {
                if (f < (uint32_t)kMaxErased) list[f] = (uint8_t)i;
                ++f;
            }
        };
        // eight bytes of the codeword, C apart from stream[from]: their mask bytes are loaded together, and only a lane that
        // finds one set walks them (a branch per byte keeps the loads of the next bytes from being issued early)
        const auto note8 = [&](uint64_t from, uint32_t i0) {
            if (!kMask) return;
            uint32_t m[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) m[j] = erased[from + (uint64_t)j * C];
            if ((m[0] | m[1] | m[2] | m[3] | m[4] | m[5] | m[6] | m[7]) == 0) return;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (m[j]) {
                    if (f < (uint32_t)kMaxErased) list[f] = (uint8_t)(i0 + (uint32_t)j);
                    ++f;
                }
        };
        uint64_t at = c;
        const uint32_t k_c = rows + (c < extra ? 1u : 0u);
        uint32_t i = 0;
        for (; i + 8 <= rows; i += 8, at += 8 * C) {
            uint32_t b[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) b[j] = stream[at + (uint64_t)j * C];
            note8(at, i);
#pragma unroll
            for (int j = 0; j < 8; ++j) lfsr_step(w, b[j], s_lfsr);
        }
#pragma unroll 8
        for (; i < rows; ++i, at += C) {
            lfsr_step(w, stream[at], s_lfsr);
            note(at, i);
        }
        if (c < extra) {                                 // at = rows * C + c, below k
            lfsr_step(w, stream[at], s_lfsr);
            note(at, rows);
        }
        at = k + c;
#pragma unroll
        for (int j = 0; j < kParity; ++j, at += C) w[j >> 2] ^= (uint32_t)stream[at] << (8 * (j & 3));
        for (int j = 0; j < kParity; j += 8) note8(k + c + (uint64_t)j * C, k_c + (uint32_t)j);
    }
    const bool nonzero = (w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) != 0;
    const bool refused = active && f > (uint32_t)kMaxErased;
    const bool dirty = nonzero && !refused;
    if (active && !dirty) status[c] = refused ? (uint8_t)kUncorrectable : (uint8_t)0;
    uint32_t corrected = 0, failed = 0;                  // wave-uniform
    if (kMask) failed = (uint32_t)__popcll(__ballot(refused));
    const uint64_t dirty_lanes = __ballot(dirty);
    if (dirty_lanes) {                                   // wave-uniform
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&s_count, (uint32_t)__popcll(dirty_lanes));     // LDS
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        if (dirty) {
            const uint32_t slot = base + (uint32_t)__popcll(dirty_lanes & ((1ull << lane) - 1ull));
            for (int i = 0; i < 8; ++i) s_rem[slot][i] = w[i];
            s_who[slot] = (uint8_t)tid;
            s_f[tid] = (uint8_t)f;
        }
    }
    __syncthreads();

    const uint32_t count = s_count;
    const Gf gf{s_exp2, s_log};
    for (uint32_t e = (uint32_t)wave; e < count; e += kWavesPerGroup) {
        const uint32_t who = s_who[e];
        const uint64_t cw = first + (uint64_t)who;
        const uint32_t k_c = rows + (cw < extra ? 1u : 0u);
        const int f_c = kMask ? (int)__builtin_amdgcn_readfirstlane((int)s_f[who]) : 0;
        const uint32_t st = repair(stream, k, C, cw, k_c, reinterpret_cast<const uint8_t *>(s_rem[e]), s_list[who], f_c, s_scratch[wave], gf, lane);
        if (lane == 0) status[cw] = (uint8_t)st;
        if (st == kUncorrectable) ++failed;
        else corrected += st;
        wave_sync();                                     // the next codeword writes the same scratch
    }
    if (counts && lane == 0) {
        if (corrected) atomicAdd(&counts[0], corrected);  // the results are not used: atomics that return nothing
        if (failed) atomicAdd(&counts[1], failed);
    }
}

// The host side of svs_rs_decode_dev and svs_rse_decode_dev (`name`, which every message starts with): the five refusals in the
// order the two headers document, then the launch - of the instantiation with the mask where d_erased is not NULL, and of the one
// without it otherwise.  kTakesMask = false (a call that has no mask: d_erased is NULL) instantiates only the latter.
template <bool kTakesMask>
int decode_dev(const char *name, uint8_t *d_stream, uint64_t k, const uint8_t *d_erased, uint8_t *d_status, uint64_t status_capacity,
               uint32_t *d_counts, void *stream) {
    if (k == 0) return SVS_OK;
    if (k > SVS_RS_MAX_DATA_BYTES) return fail(SVS_ERR_INVALID_ARG, "%s: k %llu exceeds SVS_RS_MAX_DATA_BYTES", name, (unsigned long long)k);
    if (!d_stream || !d_status) return fail(SVS_ERR_INVALID_ARG, "%s: NULL pointer", name);
    if ((uintptr_t)d_counts & 3u) return fail(SVS_ERR_INVALID_ARG, "%s: d_counts is not 4-byte aligned", name);
    const uint64_t C = codewords(k);
    if (status_capacity < C)
        return fail(SVS_ERR_CAPACITY, "%s: the status buffer holds %llu bytes, the call writes %llu", name,
                    (unsigned long long)status_capacity, (unsigned long long)C);
    const uint64_t groups = (C + kScreened - 1) / kScreened;                          // at most 2^24 at SVS_RS_MAX_DATA_BYTES
    auto *kernel = rse_decode_kernel<false>;
    if constexpr (kTakesMask)
        if (d_erased) kernel = rse_decode_kernel<true>;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)groups), dim3(kThreads), 0, (hipStream_t)stream, d_stream, k, C, (uint32_t)(k / C), k % C,
                       d_erased, d_status, d_counts);
    return launched(name);
}

}  // namespace
