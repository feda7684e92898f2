// svs_enc.hip - the C ABI declared in include/svsenc.h (libsvsenc.so, ABI 1): the Reed-Solomon encoder, the convolutional encoder
// and the bit tile for gfx950.  The arithmetic of a lane is csrc/svs_enc.hpp's; here are the three kernels and the refusals.
// Build: hipcc --offload-arch=gfx950 -O3 -shared -fPIC  (see csrc/Makefile)
//
// Several of the small libraries are loaded into one process and this one instantiates svs_rs.hpp's tables as libsvsrs.so and
// libsvsrse.so do, so EVERYTHING HERE HAS INTERNAL LINKAGE (see the note at the top of csrc/svs_rs_decode.hpp).
//
//   fec_encode_kernel<CODE>   one lane a unit of the coded stream (svsenc::FecUnit: 16 .. 80 trellis steps that send one or three
//       whole dwords).  The lane reads the four to seven info bytes of its window byte by byte - any alignment, nothing behind
//       the payload; neighbouring lanes read overlapping bytes of the same cache line -, forms every output of its steps with
//       shifts and xors of the 64-bit window, interleaves or compacts them in registers and stores whole aligned dwords,
//       neighbouring lanes neighbouring dwords.  Only the stream's last, partial dword is stored by bytes.  No LDS.
//   rs_encode_kernel<kCopy>   the screening walk of the decoder (csrc/svs_rs_decode.hpp, step 1) over the data bytes only: one
//       lane a codeword, the remainder in 8 registers, the 256 x 32-byte table in LDS, eight rows at a time with every load
//       issued before the first is used; lanes c .. c + 63 read neighbouring bytes at every row and store neighbouring parity
//       bytes.  Out of place (kCopy) a lane stores each data byte it reads: the copy costs no second pass.
//   tile_kernel               one lane an output dword: the residue of its first bit by one 64-bit modulo, then runs of the source
//       shifted into place - two at most when the period is 32 bits or more, one per copy when it is shorter.
// No atomics, no scratch (profiles/enc_resources.txt).
#include "svsenc.h"
#include "svs_enc_args.hpp"   // and svs_abi.hpp: fail(), launched(), overlap()
#include "svs_enc.hpp"

namespace {

using namespace svsenc;

constexpr int kThreads = 256;
constexpr int kRsThreads = 64;                    // a workgroup is one wave: 64 codewords, as the decoder's screening wave

__device__ const svsrs::LfsrTable d_lfsr = svsrs::make_lfsr(svsrs::make_field(), svsrs::make_generator(svsrs::make_field()));

// `bytes` is the length of the stream: a dword that ends inside it is stored whole (at is 4-byte aligned), the last, partial
// one by its bytes, the first in the dword's highest byte
__device__ __forceinline__ void store_dword(uint8_t *out, uint64_t at, uint64_t bytes, uint32_t word) {
    if (at + 4 <= bytes) {
        *reinterpret_cast<uint32_t *>(out + at) = __builtin_bswap32(word);
    } else {
        for (int b = 0; b < 4; ++b)
            if (at + (uint64_t)b < bytes) out[at + (uint64_t)b] = (uint8_t)(word >> (24 - 8 * b));
    }
}

template <int CODE>
__global__ __launch_bounds__(kThreads) void fec_encode_kernel(const uint8_t *__restrict__ info, uint64_t n_info, uint64_t n_units,
                                                              uint8_t *__restrict__ out, uint64_t out_bytes) {
    const uint64_t u = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (u >= n_units) return;
    constexpr int kDwords = FecUnit<CODE>::dwords;
    uint32_t word[kDwords];
    fec_unit<CODE>(Bytes{info}, n_info, u, word);
#pragma unroll
    for (int i = 0; i < kDwords; ++i) store_dword(out, (u * kDwords + (uint64_t)i) * 4u, out_bytes, word[i]);
}

template <bool kCopy>
__global__ __launch_bounds__(kRsThreads) void rs_encode_kernel(const uint8_t *data, uint8_t *out, uint64_t k, uint64_t C, uint32_t rows,
                                                               uint64_t extra) {
    __shared__ __attribute__((aligned(32))) uint32_t s_lfsr[256 * 8];
    const int tid = threadIdx.x;
    {
        const uint32_t *src = &d_lfsr.row[0][0];
        for (int i = tid; i < 256 * 8; i += kRsThreads) s_lfsr[i] = src[i];
    }
    __syncthreads();
    const uint64_t c = (uint64_t)blockIdx.x * kRsThreads + (uint64_t)tid;
    if (c >= C) return;
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    rs_walk<kCopy>(data, out, C, rows, extra, c, s_lfsr, w);
#pragma unroll
    for (int j = 0; j < svsrs::kParity; ++j) out[rs_parity_offset(k, C, c, j)] = rs_parity_byte(w, j);
}

__global__ __launch_bounds__(kThreads) void tile_kernel(const uint8_t *__restrict__ in, uint64_t period, uint8_t *__restrict__ out,
                                                        uint64_t n_out, uint64_t n_dwords, uint64_t out_bytes) {
    const uint64_t d = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (d >= n_dwords) return;
    store_dword(out, d * 4u, out_bytes, tile_dword(Bytes{in}, period, tile_residue(d, period), d, n_out));
}

template <int CODE>
void launch_fec(const uint8_t *d_info, uint64_t n_info, uint64_t n_coded, uint8_t *d_out, uint64_t bytes, hipStream_t st) {
    const uint64_t units = fec_units<CODE>(n_coded);                      // at most 2^38 at SVS_FEC_MAX_INFO_BITS: 2^30 workgroups
    const uint64_t groups = (units + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(fec_encode_kernel<CODE>, dim3((uint32_t)groups), dim3(kThreads), 0, st, d_info, n_info, units, d_out, bytes);
}

}  // namespace

extern "C" {

int svs_enc_abi_version(void) { return SVS_ENC_ABI_VERSION; }

const char *svs_enc_last_error(void) { return g_last_error.c_str(); }

int svs_rs_encode_dev(const uint8_t *d_data, uint64_t k, uint8_t *d_stream_out, uint64_t capacity_bytes, void *stream) {
    uint64_t C = 0, total = 0;
    const int rc = rs_encode_args("svs_rs_encode_dev", d_data, k, d_stream_out, capacity_bytes, &C, &total);
    if (rc != kEncode) return rc;
    const bool in_place = d_stream_out == d_data;
    if (!in_place && overlap(d_data, k, d_stream_out, total))
        return fail(SVS_ERR_INVALID_ARG, "svs_rs_encode_dev: the data and the stream overlap without being the same buffer");
    const uint64_t groups = (C + kRsThreads - 1) / kRsThreads;            // at most 2^24 at SVS_RS_MAX_DATA_BYTES
    hipLaunchKernelGGL(in_place ? rs_encode_kernel<false> : rs_encode_kernel<true>, dim3((uint32_t)groups), dim3(kRsThreads), 0,
                       (hipStream_t)stream, d_data, d_stream_out, k, C, (uint32_t)(k / C), k % C);
    return launched("svs_rs_encode_dev");
}

int svs_fec_encode_dev(const uint8_t *d_info_packed, uint64_t n_info, int rate, uint8_t *d_coded_packed_out, uint64_t capacity_bytes,
                       void *stream) {
    uint64_t n_coded = 0;
    const int rc = fec_encode_args("svs_fec_encode_dev", d_info_packed, n_info, rate, d_coded_packed_out, capacity_bytes, true, &n_coded);
    if (rc != kEncode) return rc;
    svsfec::with_rate(rate, [&](auto code) {
        launch_fec<decltype(code)::value>(d_info_packed, n_info, n_coded, d_coded_packed_out, (n_coded + 7) / 8, (hipStream_t)stream);
    });
    return launched("svs_fec_encode_dev");
}

int svs_bits_tile_dev(const uint8_t *d_bits_packed, uint64_t period_bits, uint8_t *d_out_packed, uint64_t n_out_bits,
                      uint64_t capacity_bytes, void *stream) {
    if (n_out_bits == 0) return SVS_OK;
    if (period_bits == 0 || period_bits > SVS_ENC_MAX_TILE_BITS || n_out_bits > SVS_ENC_MAX_TILE_BITS)
        return fail(SVS_ERR_INVALID_ARG, "svs_bits_tile_dev: period %llu and length %llu must be in 1 .. SVS_ENC_MAX_TILE_BITS",
                    (unsigned long long)period_bits, (unsigned long long)n_out_bits);
    if (!d_bits_packed || !d_out_packed) return fail(SVS_ERR_INVALID_ARG, "svs_bits_tile_dev: NULL pointer");
    if ((uintptr_t)d_out_packed & 3u) return fail(SVS_ERR_INVALID_ARG, "svs_bits_tile_dev: the output is not 4-byte aligned");
    const uint64_t bytes = (n_out_bits + 7) / 8, in_bytes = (period_bits + 7) / 8;
    if (capacity_bytes < bytes)
        return fail(SVS_ERR_CAPACITY, "svs_bits_tile_dev: the output holds %llu bytes, the call writes %llu",
                    (unsigned long long)capacity_bytes, (unsigned long long)bytes);
    if (overlap(d_bits_packed, in_bytes, d_out_packed, bytes)) return fail(SVS_ERR_INVALID_ARG, "svs_bits_tile_dev: the buffers overlap");
    const uint64_t dwords = (n_out_bits + 31) / 32, groups = (dwords + kThreads - 1) / kThreads;   // at most 2^30 workgroups
    hipLaunchKernelGGL(tile_kernel, dim3((uint32_t)groups), dim3(kThreads), 0, (hipStream_t)stream, d_bits_packed, period_bits,
                       d_out_packed, n_out_bits, dwords, bytes);
    return launched("svs_bits_tile_dev");
}

}  // extern "C"
