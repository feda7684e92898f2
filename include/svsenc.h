/*
 * svsenc.h - C ABI of libsvsenc.so: the sending half of the coded path on the MI355X (gfx950) - the Reed-Solomon encoder of
 * include/svsrs.h, the convolutional encoder of include/svsfec.h at its six rate codes, and the tiling of a packed bit stream
 * (soft.tile of svsdct/soft.py) - so that a payload held on the device reaches svs_embed*_dev without a download in between.
 * A fifth, small library beside libsvsdct.so, libsvsfec.so, libsvsrs.so and libsvsrse.so.  It defines NO format: every call
 * writes the bytes that the host encoder of the same name writes (svs_rs_encode, svs_fec_encode), and those two headers hold
 * the formats.  The reference (erc-a/Secure-Video-Steganography-using-ECC-and-DCT) has no channel code; nothing here replaces a
 * function of it.
 *
 * Conventions (those of svsfec.h)
 *   - plain C types only; every function that can fail returns SVS_OK (0) or a negative SVS_ERR_* code and never throws;
 *     svs_enc_last_error() gives the message for the calling thread.
 *   - the caller owns every buffer.  The `*_dev` entry points take DEVICE pointers and a hipStream_t (as void*; NULL = the
 *     null stream), enqueue one launch and return without synchronising.  They keep no state, allocate nothing and are
 *     re-entrant and thread-safe.  The library reads no environment variable.
 *   - bits are packed MSB-first (numpy.packbits order): bit i is bit 7 - (i % 8) of byte i / 8.
 *
 * The chain of a sender: svs_rs_encode_dev (optional) -> svs_fec_encode_dev -> svs_bits_tile_dev (optional) -> svs_embed*_dev.
 * The outputs of the last two are d_bits_packed of an embed call and must be 4-byte aligned as that is.
 *
 * Refusals, in this order and before any device work:
 *   svs_rs_encode_dev    1. k = 0: SVS_OK, nothing is done, no pointer is looked at;  2. k above SVS_RS_MAX_DATA_BYTES (2^37):
 *                        SVS_ERR_INVALID_ARG;  3. a NULL pointer: SVS_ERR_INVALID_ARG;  4. capacity_bytes below k + 32 C:
 *                        SVS_ERR_CAPACITY;  5. d_stream_out != d_data and the k bytes at d_data overlap the k + 32 C bytes at
 *                        d_stream_out: SVS_ERR_INVALID_ARG.
 *   svs_fec_encode_dev   1. rate other than 2, 3, 23, 34, 56, 78: SVS_ERR_INVALID_ARG;  2. n_info = 0: SVS_OK, nothing is done,
 *                        no pointer is looked at;  3. n_info above SVS_FEC_MAX_INFO_BITS (2^40): SVS_ERR_INVALID_ARG;  4. a NULL
 *                        pointer: SVS_ERR_INVALID_ARG;  5. an output that is not 4-byte aligned: SVS_ERR_INVALID_ARG;
 *                        6. capacity_bytes below ceil(n_coded / 8): SVS_ERR_CAPACITY.
 *   svs_bits_tile_dev    1. n_out_bits = 0: SVS_OK, nothing is done, no pointer is looked at;  2. period_bits = 0, or either
 *                        length above SVS_ENC_MAX_TILE_BITS (2^43): SVS_ERR_INVALID_ARG;  3. a NULL pointer:
 *                        SVS_ERR_INVALID_ARG;  4. an output that is not 4-byte aligned: SVS_ERR_INVALID_ARG;  5. capacity_bytes
 *                        below ceil(n_out_bits / 8): SVS_ERR_CAPACITY;  6. the ceil(period_bits / 8) input bytes overlap the
 *                        output bytes: SVS_ERR_INVALID_ARG.
 *
 * Not here: decoders (svsfec.h, svsrs.h, svsrse.h), a host form of any call (svs_rs_encode, svs_fec_encode and soft.tile are
 * those), and an encoder fused into the embed kernel.
 */
#ifndef SVSENC_H
#define SVSENC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVS_ENC_ABI_VERSION 1

#ifndef SVS_OK                    /* the codes of svsdct.h, for a caller that includes both */
#define SVS_OK 0
#define SVS_ERR_INVALID_ARG (-1)  /* bad rate / NULL pointer / misaligned output / overlap / length out of range */
#define SVS_ERR_HIP (-2)          /* a HIP runtime call failed; see svs_enc_last_error() */
#define SVS_ERR_NO_DEVICE (-3)    /* no usable AMD GPU */
#define SVS_ERR_CAPACITY (-4)     /* an output buffer is too small */
#endif

/* the longest tiled stream and the longest period, in bits: 3 (2^40 + 6), the largest coded stream, rounded up */
#define SVS_ENC_MAX_TILE_BITS (1ull << 43)

int svs_enc_abi_version(void);
const char *svs_enc_last_error(void);

/* svs_rs_encode (svsrs.h: "Codeword", "Stream layout") on the device: the k + 32 C bytes of the stream of the k bytes at d_data
 * go to d_stream_out, byte for byte what the host call writes; capacity_bytes is the size of that buffer, and no byte behind
 * the stream is written.  Both pointers may have any alignment.  d_stream_out == d_data encodes in place: the data is where
 * it belongs already and only the 32 C parity bytes behind it are written.  Otherwise the buffers must not overlap, and the
 * launch copies the data as it reads it.  One launch on `stream`. */
int svs_rs_encode_dev(const uint8_t *d_data, uint64_t k, uint8_t *d_stream_out, uint64_t capacity_bytes, void *stream);

/* svs_fec_encode (svsfec.h: "Code", "Punctured codes") on the device: the first n_info bits at d_info_packed, read at any
 * byte alignment and no byte behind ceil(n_info / 8), are encoded at `rate` (2, 3, 23, 34, 56 or 78) into ceil(n_coded / 8)
 * bytes at d_coded_packed_out, n_coded = svs_fec_coded_bits(n_info, rate): byte for byte what the host call writes, the pad
 * bits of the last byte 0, no byte behind it written.  The output must be 4-byte aligned; the buffers must not overlap.  One
 * launch on `stream`. */
int svs_fec_encode_dev(const uint8_t *d_info_packed, uint64_t n_info, int rate, uint8_t *d_coded_packed_out, uint64_t capacity_bytes,
                       void *stream);

/* Output bit i = input bit i mod period_bits, for i < n_out_bits: the first period_bits bits at d_bits_packed (any byte
 * alignment; ceil(period_bits / 8) bytes are read) copy after copy, the last one cut - or, with n_out_bits below the period,
 * its first bits.  ceil(n_out_bits / 8) bytes are written to d_out_packed, 4-byte aligned: the pad bits of the last byte 0,
 * no byte behind it.  Out of place: the buffers must not overlap.  One launch on `stream`. */
int svs_bits_tile_dev(const uint8_t *d_bits_packed, uint64_t period_bits, uint8_t *d_out_packed, uint64_t n_out_bits,
                      uint64_t capacity_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SVSENC_H */
