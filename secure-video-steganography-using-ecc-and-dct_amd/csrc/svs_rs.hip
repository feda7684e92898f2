// svs_rs.hip - the C ABI declared in include/svsrs.h (libsvsrs.so, ABI 1): the sizes, the host encoder, and svs_rs_decode_dev,
// which launches the decoder kernel of csrc/svs_rs_decode.hpp in its instantiation without a mask - the only one this library
// holds.  The kernel, and why it has the shape it has, is described there.
// Build: hipcc --offload-arch=gfx950 -O3 -shared -fPIC  (see csrc/Makefile)
#include "svs_enc_args.hpp"
#include "svs_rs_decode.hpp"

namespace {

constexpr svsrs::Field kField = svsrs::make_field();
constexpr svsrs::Generator kGenerator = svsrs::make_generator(kField);
constexpr svsrs::LfsrTable kLfsr = svsrs::make_lfsr(kField, kGenerator);
static_assert(kGenerator.low[0] == 0x74 && kGenerator.low[1] == 0x40 && kGenerator.low[31] == 0x58, "g(x) of include/svsrs.h");

}  // namespace

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
    uint64_t C = 0, total = 0;
    const int rc = rs_encode_args("svs_rs_encode", data, k, out, capacity_bytes, &C, &total);
    if (rc != kEncode) {
        if (rc == SVS_OK && n_out) *n_out = 0;
        return rc;
    }
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
    return decode_dev<false>("svs_rs_decode_dev", d_stream, k, nullptr, d_status, status_capacity, d_counts, stream);
}

}  // extern "C"
