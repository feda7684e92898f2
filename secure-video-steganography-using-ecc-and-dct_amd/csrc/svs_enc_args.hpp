// svs_enc_args.hpp - the argument refusals that a host encoder shares with the device encoder of the same code: svs_fec_encode
// (csrc/svs_fec.hip) with svs_fec_encode_dev, svs_rs_encode (csrc/svs_rs.hip) with svs_rs_encode_dev (both csrc/svs_enc.hip).
// `what` is the call's name, which every message starts with; the order is the one include/svsfec.h, svsrs.h and svsenc.h document.
// Each returns kEncode when the call goes on, and otherwise what the call returns: SVS_OK for an empty input, or fail()'s code.
// Internal linkage, as everything of csrc/svs_abi.hpp.
#pragma once

#include "svsfec.h"
#include "svsrs.h"
#include "svs_abi.hpp"
#include "svs_fec.hpp"
#include "svs_rs.hpp"

namespace {

constexpr int kEncode = 1;

// aligned: the output must be 4-byte aligned (the device call).  *n_coded: the coded bits of the stream
int fec_encode_args(const char *what, const uint8_t *info, uint64_t n_info, int rate, const uint8_t *out, uint64_t capacity_bytes,
                    bool aligned, uint64_t *n_coded) {
    if (!svsfec::rate_ok(rate)) return fail(SVS_ERR_INVALID_ARG, "%s: rate %d is %s", what, rate, svsfec::kRates);
    if (n_info == 0) return SVS_OK;
    if (n_info > SVS_FEC_MAX_INFO_BITS)
        return fail(SVS_ERR_INVALID_ARG, "%s: n_info %llu exceeds SVS_FEC_MAX_INFO_BITS", what, (unsigned long long)n_info);
    if (!info || !out) return fail(SVS_ERR_INVALID_ARG, "%s: NULL pointer", what);
    if (aligned && ((uintptr_t)out & 3u)) return fail(SVS_ERR_INVALID_ARG, "%s: the output is not 4-byte aligned", what);
    *n_coded = svsfec::stream_bits(n_info + SVS_FEC_TAIL, rate);
    const uint64_t bytes = (*n_coded + 7) / 8;
    if (capacity_bytes < bytes)
        return fail(SVS_ERR_CAPACITY, "%s: the output holds %llu bytes, the call writes %llu", what, (unsigned long long)capacity_bytes,
                    (unsigned long long)bytes);
    return kEncode;
}

// *C: the codewords of k data bytes, *total: the bytes of their stream
int rs_encode_args(const char *what, const uint8_t *data, uint64_t k, const uint8_t *out, uint64_t capacity_bytes, uint64_t *C,
                   uint64_t *total) {
    if (k == 0) return SVS_OK;
    if (k > SVS_RS_MAX_DATA_BYTES) return fail(SVS_ERR_INVALID_ARG, "%s: k %llu exceeds SVS_RS_MAX_DATA_BYTES", what, (unsigned long long)k);
    if (!data || !out) return fail(SVS_ERR_INVALID_ARG, "%s: NULL pointer", what);
    *C = svsrs::codewords(k);
    *total = k + svsrs::kParity * *C;
    if (capacity_bytes < *total)
        return fail(SVS_ERR_CAPACITY, "%s: the output holds %llu bytes, the call writes %llu", what, (unsigned long long)capacity_bytes,
                    (unsigned long long)*total);
    return kEncode;
}

}  // namespace
