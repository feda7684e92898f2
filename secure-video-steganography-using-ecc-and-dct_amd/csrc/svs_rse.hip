// svs_rse.hip - the C ABI declared in include/svsrse.h (libsvsrse.so, ABI 1): svs_rse_decode_dev, which launches the decoder kernel
// of csrc/svs_rs_decode.hpp - with the mask where d_erased is not NULL, without it otherwise; this library holds both
// instantiations.  The kernel is described there.
// Build: hipcc --offload-arch=gfx950 -O3 -shared -fPIC  (see csrc/Makefile)
#include "svsrse.h"
#include "svs_rs_decode.hpp"

static_assert(kMaxErased == SVS_RSE_MAX_ERASED, "include/svsrse.h");

extern "C" {

int svs_rse_abi_version(void) { return SVS_RSE_ABI_VERSION; }

const char *svs_rse_last_error(void) { return g_last_error.c_str(); }

int svs_rse_decode_dev(uint8_t *d_stream, uint64_t k, const uint8_t *d_erased, uint8_t *d_status, uint64_t status_capacity,
                       uint32_t *d_counts, void *stream) {
    return decode_dev<true>("svs_rse_decode_dev", d_stream, k, d_erased, d_status, status_capacity, d_counts, stream);
}

}  // extern "C"
