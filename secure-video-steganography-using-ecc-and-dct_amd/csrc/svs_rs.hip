// svs_rs.hip - the C ABI declared in include/svsrs.h: the host encoder and the bounded-distance decoder for gfx950.
// Build: hipcc --offload-arch=gfx950 -O3 -shared -fPIC  (see csrc/Makefile)
//
// The decoder kernel, one launch; a workgroup is four waves and owns 64 codewords:
//   1. screening, one lane per codeword, on the workgroup's first wave.  Lane c walks codeword c with the encoder's own LFSR
//      (svs_rs.hpp): 32 remainder bytes in 8 registers, the 32 products of the feedback byte from a 256 x 32-byte table in LDS
//      (two 16-byte reads).  With the stream's interleave the lanes c .. c + 63 read neighbouring bytes at every step, so every
//      load is one coalesced run; the address advances by C a step (64-bit, no division).  The k mod C codewords with one more
//      data byte take it under a predicate behind the loop (a zero remainder does not change under a zero byte, so "one more at
//      the end" is "one more in the first row").  The parity bytes are xored in: r(x) = c(x) mod g(x).  r = 0: the codeword is
//      clean, status 0, done - the pass every codeword pays for.
//   2. repair.  A dirty lane puts its lane number and r into a worklist in LDS; behind a barrier the four waves take the entries
//      in turn, ONE WAVE A CODEWORD: S_j = r(alpha^j) on lanes 0 .. 31 (no second pass over the data), Berlekamp-Massey with
//      Lambda and B one coefficient a lane and the discrepancy a cross-lane xor (it stops when L passes 16, so 17 lanes hold
//      everything and the xor runs over 32), the root search over the k_c + 32 positions 64 at a time with Forney's value on the
//      lanes that found a root.  Nothing is stored before every root is in and counted: a codeword that fails is not written.
//      The byte stores go to the codeword's own addresses, which no other wave touches: no race, no atomics.
//      A repair is a chain of dependent LDS reads (logarithm, antilogarithm, cross-lane xor), about 10^5 cycles a codeword, so
//      it is waves in flight that pay: with 256 codewords a workgroup (every wave screening) a stream of 64 k codewords is 1 000
//      waves, one a SIMD, and the all-dirty stream took 2.77 ms; with 64 a workgroup three more waves a workgroup wait at the
//      barrier while the first screens - the clean pass has the same 1 000 screening waves and the same 0.029 ms - and repair
//      with it: 0.78 ms (profiles/rs_rates.txt).
//   3. the counters.  Adding to d_counts once a codeword is 64 k atomics on one address in a row when every codeword is dirty;
//      a wave sums what it repaired in a register instead and adds once at its end, and only what is not 0 (at most 8 atomics a
//      workgroup, none on a clean stream).  The sums are the same.
// LDS 11.6 KB a workgroup, no scratch, no global atomics beside those two adds (profiles/rs_resources.txt).
#include "svsrs.h"
#include "svs_rs.hpp"

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>

namespace {

thread_local std::string g_last_error;

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

constexpr int kWavesPerGroup = 4;
constexpr int kThreads = 64 * kWavesPerGroup;
constexpr int kScreened = 64;                     // codewords a workgroup owns: its first wave screens them

constexpr svsrs::Field kField = svsrs::make_field();
constexpr svsrs::Generator kGenerator = svsrs::make_generator(kField);
constexpr svsrs::LfsrTable kLfsr = svsrs::make_lfsr(kField, kGenerator);
static_assert(kGenerator.low[0] == 0x74 && kGenerator.low[1] == 0x40 && kGenerator.low[31] == 0x58, "g(x) of include/svsrs.h");

}  // namespace

namespace svsrs {

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

// One wave repairs codeword c (k_c data bytes) from its remainder r.  scratch: 96 bytes of LDS private to the wave.
// Returns the status: the bytes changed, or kUncorrectable with nothing written.
__device__ __forceinline__ uint32_t repair(uint8_t *stream, uint64_t k, uint64_t C, uint64_t c, uint32_t k_c, const uint8_t *r,
                                           uint8_t *scratch, const Gf &gf, int lane) {
    uint8_t *syn = scratch, *lambda = scratch + 32, *omega = scratch + 64;
    if (lane < kParity) syn[lane] = (uint8_t)syndrome(lane, r, gf);
    wave_sync();

    uint32_t lam = lane == 0, shifted_b = lane == 1, b = 1;
    int L = 0;
    for (int n = 0; n < kParity; ++n) {
        const uint32_t d = xor_of_32(bm_term(lane, n, lam, syn, gf));
        const bool longer = d != 0 && 2 * L <= n;
        const BmLane next = bm_update(lam, shifted_b, d, b, longer, gf);
        lam = next.lambda;
        const uint32_t up = (uint32_t)__shfl_up((int)next.pass, 1);
        shifted_b = lane == 0 ? 0u : up;
        if (longer) {
            L = n + 1 - L;
            b = d;
            if (L > kT) return kUncorrectable;           // wave-uniform: a locator of degree above 16
        }
    }
    // L >= 1: the syndromes of a dirty codeword are not all 0
    if (lane <= kT) lambda[lane] = (uint8_t)lam;         // the lanes above L hold 0
    wave_sync();
    if (lane < kT) omega[lane] = (uint8_t)omega_coefficient(lane, L, lambda, syn, gf);
    wave_sync();

    const int n_c = (int)k_c + kParity;                  // at most 255: four rounds of 64 positions
    uint32_t values = 0;                                 // byte q: this lane's error value of round q, 0: no root
    int roots = 0;
    bool bad = false;
    for (int q = 0; q < 4; ++q) {
        const int p = 64 * q + lane;
        const uint32_t v = p < n_c ? root_value(p, L, lambda, omega, gf) : 0u;
        bad |= v == kBadRoot;
        roots += __popcll(__ballot(v != 0));
        values |= (v & 0xFFu) << (8 * q);
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
    return (uint32_t)L;
}

// rows = k / C and extra = k % C: the codewords c < extra hold rows + 1 data bytes, the others rows
__global__ __launch_bounds__(kThreads) void decode_kernel(uint8_t *stream, uint64_t k, uint64_t C, uint32_t rows, uint64_t extra,
                                                           uint8_t *status, uint32_t *counts) {
    __shared__ __attribute__((aligned(32))) uint32_t s_lfsr[256 * 8];
    __shared__ __attribute__((aligned(32))) uint32_t s_rem[kScreened][8];    // the worklist: the remainder ..
    __shared__ uint8_t s_who[kScreened];                                      // .. and the lane it came from
    __shared__ __attribute__((aligned(4))) uint8_t s_exp2[512];
    __shared__ __attribute__((aligned(4))) uint8_t s_log[256];
    __shared__ __attribute__((aligned(4))) uint8_t s_scratch[kWavesPerGroup][96];
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
    if (active) {
        const uint8_t *p = stream + c;
#pragma unroll 8
        for (uint32_t i = 0; i < rows; ++i, p += C) lfsr_step(w, *p, s_lfsr);
        if (c < extra) lfsr_step(w, *p, s_lfsr);         // p = stream + rows * C + c, below k
        const uint8_t *parity = stream + k + c;
#pragma unroll
        for (int j = 0; j < kParity; ++j, parity += C) w[j >> 2] ^= (uint32_t)*parity << (8 * (j & 3));
    }
    const bool dirty = (w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) != 0;
    if (active && !dirty) status[c] = 0;
    const uint64_t dirty_lanes = __ballot(dirty);
    if (dirty_lanes) {                                   // wave-uniform
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&s_count, (uint32_t)__popcll(dirty_lanes));     // LDS
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        if (dirty) {
            const uint32_t slot = base + (uint32_t)__popcll(dirty_lanes & ((1ull << lane) - 1ull));
            for (int i = 0; i < 8; ++i) s_rem[slot][i] = w[i];
            s_who[slot] = (uint8_t)tid;
        }
    }
    __syncthreads();

    const uint32_t count = s_count;
    if (count == 0) return;
    const Gf gf{s_exp2, s_log};
    uint32_t corrected = 0, failed = 0;                  // wave-uniform
    for (uint32_t e = (uint32_t)wave; e < count; e += kWavesPerGroup) {
        const uint64_t cw = first + (uint64_t)s_who[e];
        const uint32_t k_c = rows + (cw < extra ? 1u : 0u);
        const uint32_t st = repair(stream, k, C, cw, k_c, reinterpret_cast<const uint8_t *>(s_rem[e]), s_scratch[wave], gf, lane);
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

}  // namespace svsrs

extern "C" {

int svs_rs_abi_version(void) { return SVS_RS_ABI_VERSION; }

const char *svs_rs_last_error(void) { return g_last_error.c_str(); }

uint64_t svs_rs_codewords(uint64_t k) { return k > SVS_RS_MAX_DATA_BYTES ? 0 : svsrs::codewords(k); }

uint64_t svs_rs_coded_bytes(uint64_t k) { return k == 0 || k > SVS_RS_MAX_DATA_BYTES ? 0 : svsrs::coded_bytes(k); }

uint64_t svs_rs_data_bytes(uint64_t total_bytes) {
    const uint64_t k = svsrs::data_bytes(total_bytes);
    return k > SVS_RS_MAX_DATA_BYTES ? SVS_RS_MAX_DATA_BYTES : k;
}

int svs_rs_encode(const uint8_t *data, uint64_t k, uint8_t *out, uint64_t capacity_bytes, uint64_t *n_out) {
    if (k == 0) {
        if (n_out) *n_out = 0;
        return SVS_OK;
    }
    if (k > SVS_RS_MAX_DATA_BYTES) return fail(SVS_ERR_INVALID_ARG, "svs_rs_encode: k %llu exceeds SVS_RS_MAX_DATA_BYTES", (unsigned long long)k);
    if (!data || !out) return fail(SVS_ERR_INVALID_ARG, "svs_rs_encode: NULL pointer");
    const uint64_t C = svsrs::codewords(k), total = k + svsrs::kParity * C;
    if (capacity_bytes < total)
        return fail(SVS_ERR_CAPACITY, "svs_rs_encode: the output holds %llu bytes, the call writes %llu", (unsigned long long)capacity_bytes,
                    (unsigned long long)total);
    for (uint64_t i = 0; i < k; ++i) out[i] = data[i];
    for (uint64_t c = 0; c < C; ++c) {
        uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (uint64_t i = c; i < k; i += C) svsrs::lfsr_step(w, data[i], &kLfsr.row[0][0]);
        for (int j = 0; j < svsrs::kParity; ++j) out[k + (uint64_t)j * C + c] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
    }
    if (n_out) *n_out = total;
    return SVS_OK;
}

int svs_rs_decode_dev(uint8_t *d_stream, uint64_t k, uint8_t *d_status, uint64_t status_capacity, uint32_t *d_counts, void *stream) {
    if (k == 0) return SVS_OK;
    if (k > SVS_RS_MAX_DATA_BYTES)
        return fail(SVS_ERR_INVALID_ARG, "svs_rs_decode_dev: k %llu exceeds SVS_RS_MAX_DATA_BYTES", (unsigned long long)k);
    if (!d_stream || !d_status) return fail(SVS_ERR_INVALID_ARG, "svs_rs_decode_dev: NULL pointer");
    if ((uintptr_t)d_counts & 3u) return fail(SVS_ERR_INVALID_ARG, "svs_rs_decode_dev: d_counts is not 4-byte aligned");
    const uint64_t C = svsrs::codewords(k);
    if (status_capacity < C)
        return fail(SVS_ERR_CAPACITY, "svs_rs_decode_dev: the status buffer holds %llu bytes, the call writes %llu",
                    (unsigned long long)status_capacity, (unsigned long long)C);
    const uint64_t groups = (C + kScreened - 1) / kScreened;                          // at most 2^24 at SVS_RS_MAX_DATA_BYTES
    hipLaunchKernelGGL(svsrs::decode_kernel, dim3((uint32_t)groups), dim3(kThreads), 0, (hipStream_t)stream, d_stream, k, C,
                       (uint32_t)(k / C), k % C, d_status, d_counts);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SVS_ERR_HIP, "svs_rs_decode_dev: launch failed: %s", hipGetErrorString(e));
    return SVS_OK;
}

}  // extern "C"
