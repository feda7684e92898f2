/*
 * svsrs.h - C ABI of libsvsrs.so: a Reed-Solomon (255, 223) outer code, byte-interleaved over all its codewords, with a
 * bounded-distance decoder on the MI355X (gfx950).  A third, small library beside libsvsdct.so (include/svsdct.h) and
 * libsvsfec.so (include/svsfec.h): it shares no code with either, takes the packed bytes that svs_fec_decode_soft_dev and
 * svs_fec_decode_weights_dev write, corrects up to 16 wrong bytes in each codeword - what a Viterbi decoder's short bursts look
 * like - and says for every codeword whether it decoded.  The reference (erc-a/Secure-Video-Steganography-using-ECC-and-DCT) has no
 * channel code; nothing here replaces a function of it.
 *
 * Conventions (those of svsfec.h)
 *   - plain C types only; every function that can fail returns SVS_OK (0) or a negative SVS_ERR_* code and never throws;
 *     svs_rs_last_error() gives the message for the calling thread.
 *   - the caller owns every buffer.  svs_rs_decode_dev takes DEVICE pointers and a hipStream_t (as void*; NULL = the null
 *     stream), enqueues one launch and returns without synchronising.  It keeps no state, allocates nothing and is re-entrant
 *     and thread-safe.  svs_rs_encode is host code: it needs no GPU.  The library reads no environment variable.
 *
 * THE FORMAT, step by step.  Host and device compute it in integers, so the result is the same bytes everywhere.
 *
 * Field
 *   GF(2^8) modulo x^8 + x^4 + x^3 + x^2 + 1 (0x11D); alpha = 0x02.  Addition is xor.
 *
 * Code
 *   RS(255, 223), shortened.  g(x) = prod over i = 0 .. 31 of (x - alpha^i); highest coefficient first:
 *       01 74 40 34 ae 36 7e 10 c2 a2 21 21 9d b0 c5 e1 0c 3b 37 fd e4 94 2f b3 b9 18 8a fd 14 8e 37 ac 58
 *
 * Codeword
 *   k_c data bytes d_0 .. d_(k_c - 1), 1 <= k_c <= 223, and 32 parity bytes p_0 .. p_31:
 *       c(x) = sum d_i x^(k_c + 31 - i) + sum p_j x^(31 - j),     p(x) = d(x) x^32 mod g(x),
 *   so that g(x) divides c(x).  Known answers: the one data byte 01 has the parity 74 40 .. 58 above; the data 00 01 .. 09 has
 *       6c 22 8c 86 1c 3e 14 d2 52 a2 ca 9c 2f a1 28 9a 54 02 15 8d b4 09 81 5c 43 eb 09 72 0b ef 59 fb
 *
 * Stream layout
 *   systematic, and interleaved over ALL codewords.  k data bytes make C = ceil(k / 223) codewords.
 *       codeword c holds the data bytes stream[c], stream[c + C], stream[c + 2 C], ..:   k_c = ceil((k - c) / C)
 *       parity byte j of codeword c is stream[k + j C + c]
 *       n_bytes = k + 32 C;  the first k bytes are the payload itself.
 *   A burst of B <= C consecutive stream bytes puts at most one byte into any codeword.
 *   Known answer: the data 0, 1, .. 223 (k = 224, C = 2) gives 288 bytes, stream[224 .. 231] = 99 cc f0 92 3b 6e eb 31.
 *
 * Sizes
 *   svs_rs_codewords(k) = C;   svs_rs_coded_bytes(k) = k + 32 C;
 *   svs_rs_data_bytes(T) = the largest k with k + 32 ceil(k / 223) <= T, 0 when there is none:
 *       32 -> 0, 33 -> 1, 255 .. 287 -> 223, 288 -> 224, 449 -> 385, 786 -> 669.
 *   k is at most SVS_RS_MAX_DATA_BYTES = 2^37; the two functions of k return 0 for a larger one.
 *
 * Decoding: defined by its result, not by an algorithm
 *   For every codeword on its own: if a word of the shortened code (k_c data bytes, g(x) divides it) lies within Hamming
 *   distance 16 of the received k_c + 32 bytes, that word replaces them - it is unique, the code's distance is 33 - and the
 *   codeword's status byte is the number of bytes changed, 0 .. 16.  Otherwise NO byte of the codeword is written and its
 *   status is 255 (SVS_RS_UNCORRECTABLE).
 *   In Berlekamp-Massey terms, with the syndromes S_j = c(alpha^j), j = 0 .. 31, these are the failures: a locator of degree
 *   above 16; a locator whose roots among the codeword's own k_c + 32 positions number other than its degree (an error
 *   "located" in the bytes that the shortening left out, or a locator that does not split); a zero derivative at a root.
 *   All of it is integer arithmetic in the field: the host model of the tests and the device give the same bytes.
 *
 * Refusals of svs_rs_decode_dev, in this order and before any device work:
 *   1. k = 0                                                   SVS_OK: nothing is done, no pointer is looked at
 *   2. k above SVS_RS_MAX_DATA_BYTES                           SVS_ERR_INVALID_ARG
 *   3. a NULL stream or status pointer                         SVS_ERR_INVALID_ARG
 *   4. d_counts neither NULL nor 4-byte aligned                SVS_ERR_INVALID_ARG
 *   5. status_capacity below C                                 SVS_ERR_CAPACITY
 *   svs_rs_encode: the same 1 (it still reports *n_out = 0), 2 and 3 (data or output NULL), then capacity_bytes below
 *   k + 32 C is SVS_ERR_CAPACITY.  n_out may be NULL.
 *
 * Not here: a host decoder (the product has no CPU path; the model lives in the tests), a device encoder, and any interleaving
 * depth other than "all codewords".  Errors-and-erasures decoding of this code is libsvsrse.so, include/svsrse.h.
 */
#ifndef SVSRS_H
#define SVSRS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVS_RS_ABI_VERSION 1

#ifndef SVS_OK                    /* the codes of svsdct.h, for a caller that includes both */
#define SVS_OK 0
#define SVS_ERR_INVALID_ARG (-1)  /* NULL pointer / misaligned counters / length out of range */
#define SVS_ERR_HIP (-2)          /* a HIP runtime call failed; see svs_rs_last_error() */
#define SVS_ERR_NO_DEVICE (-3)    /* no usable AMD GPU */
#define SVS_ERR_CAPACITY (-4)     /* an output buffer is too small */
#endif

#define SVS_RS_CODEWORD 255       /* bytes of a full codeword */
#define SVS_RS_DATA 223           /* data bytes of a full codeword */
#define SVS_RS_PARITY 32          /* parity bytes of every codeword */
#define SVS_RS_T 16               /* wrong bytes a codeword corrects */
#define SVS_RS_UNCORRECTABLE 255  /* the status of a codeword left as received */
#define SVS_RS_MAX_DATA_BYTES (1ull << 37)

int svs_rs_abi_version(void);
const char *svs_rs_last_error(void);

/* C = ceil(k / 223); 0 for k = 0 or k above SVS_RS_MAX_DATA_BYTES */
uint64_t svs_rs_codewords(uint64_t k);
/* k + 32 C; 0 for k = 0 or k above SVS_RS_MAX_DATA_BYTES */
uint64_t svs_rs_coded_bytes(uint64_t k);
/* the largest k whose coded stream fits total_bytes (at most SVS_RS_MAX_DATA_BYTES); 0 when there is none */
uint64_t svs_rs_data_bytes(uint64_t total_bytes);

/* Host only.  Writes the k + 32 C bytes of the stream of `data` (k bytes) to `out`: the data itself, then the interleaved
 * parity; capacity_bytes is the size of the output buffer, no byte behind the stream is written.  The input is not written; the
 * buffers must not overlap. */
int svs_rs_encode(const uint8_t *data, uint64_t k, uint8_t *out, uint64_t capacity_bytes, uint64_t *n_out);

/* Decodes the k + 32 C bytes at d_stream IN PLACE, at any alignment: a codeword that decodes is replaced by the code word, one
 * that does not is not written.  d_status receives C bytes, one per codeword: the bytes changed, 0 .. 16, or 255;
 * status_capacity is the size of that buffer.  d_counts may be NULL; otherwise it is uint32[2] to which the call ADDS, with
 * atomics that return nothing, [0] += the bytes corrected and [1] += the codewords left uncorrectable, so that a caller who
 * decodes in batches keeps totals.  One launch on `stream`. */
int svs_rs_decode_dev(uint8_t *d_stream, uint64_t k, uint8_t *d_status, uint64_t status_capacity, uint32_t *d_counts, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SVSRS_H */
