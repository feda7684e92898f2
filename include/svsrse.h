/*
 * svsrse.h - C ABI of libsvsrse.so: errors-and-erasures decoding of the Reed-Solomon outer code of include/svsrs.h on the MI355X
 * (gfx950).  A fourth, small library beside libsvsdct.so, libsvsfec.so and libsvsrs.so.  svs_rs_decode_dev treats every byte as
 * equally trustworthy and gives up at 17 wrong bytes in a codeword; a receiver that KNOWS which bytes are bad - the bytes a lost
 * frame maps to - tells this decoder so, and a codeword then stands e wrong bytes and f erased ones whenever 2 e + f <= 32: up to
 * 32 known-bad bytes, twice what the same parity corrects blind.  The reference (erc-a/Secure-Video-Steganography-using-ECC-and-DCT)
 * has no channel code; nothing here replaces a function of it.
 *
 * Conventions (those of svsrs.h)
 *   - plain C types only; a function that can fail returns SVS_OK (0) or a negative SVS_ERR_* code and never throws;
 *     svs_rse_last_error() gives the message for the calling thread.
 *   - the caller owns every buffer.  svs_rse_decode_dev takes DEVICE pointers and a hipStream_t (as void*; NULL = the null
 *     stream), enqueues one launch and returns without synchronising.  It keeps no state, allocates nothing and is re-entrant
 *     and thread-safe.  The library reads no environment variable.
 *
 * THE FORMAT, step by step.  Integers only, so the result is the same bytes everywhere.
 *
 * Field, code, codeword, stream layout, sizes
 *   those of svsrs.h, word for word: GF(2^8) modulo 0x11D, alpha = 0x02; RS(255, 223), shortened, g(x) with the roots alpha^0 ..
 *   alpha^31; k data bytes make C = ceil(k / 223) codewords, codeword c holds the data bytes stream[c], stream[c + C], .. and
 *   parity byte j of codeword c is stream[k + j C + c]; the stream has k + 32 C bytes; k is at most SVS_RS_MAX_DATA_BYTES = 2^37.
 *   Byte i of a codeword of n_c = k_c + 32 bytes (data before parity) multiplies x^p, p = n_c - 1 - i; X = alpha^p is its locator.
 *
 * The mask
 *   d_erased is k + 32 C bytes, at any alignment, laid out as the stream: byte a != 0 (ANY non-zero value) says that stream
 *   byte a is erased - its value is not to be trusted.  NULL: no byte is erased.  The mask is never written.  It must not
 *   overlap the stream.  E_c is the set of erased bytes of codeword c, f_c its size.
 *
 * Decoding: defined by its result, not by an algorithm
 *   For every codeword on its own.  If f_c <= 32, look for a word of the shortened code (k_c data bytes, g(x) divides it) that
 *   differs from the received k_c + 32 bytes in e bytes OUTSIDE E_c with 2 e + f_c <= 32; inside E_c it may differ in any number
 *   of bytes.  If such a word exists, it replaces the received bytes and the codeword's status byte is the number of bytes
 *   changed, 0 .. 32.  Such a word is unique: two of them would differ in at most e_1 + e_2 + f_c <= 32 < 33 bytes.  Otherwise
 *   NO byte of the codeword is written and its status is 255 (SVS_RS_UNCORRECTABLE) - this includes f_c > 32, even when the
 *   received bytes happen to be a code word.  An erased byte that was right counts as unchanged.
 *
 *   In Berlekamp-Massey terms, with the syndromes S_j = c(alpha^j), j = 0 .. 31, and f = f_c:
 *       Gamma(x) = prod (1 - X_i x) over the erased positions
 *       start: Lambda = Gamma, x B = x Gamma, L = f, b = 1; the steps run n = f .. 31
 *       d = sum over i <= n of Lambda_i S_(n - i);  d != 0: Lambda <- Lambda - (d / b) x^m B
 *       the locator gets longer when d != 0 and 2 L <= n + f: then B <- the Lambda before, b <- d, L <- n + 1 - L + f
 *       Omega = S Lambda mod x^32 (32 coefficients);  Forney's value of a root X^-1 of Lambda is e = X Omega(X^-1) / Lambda'(X^-1)
 *   these are the failures: 2 L - f > 32; roots of Lambda among the codeword's own k_c + 32 positions that number other than L;
 *   an erased position that is no root; a zero derivative at a root; a zero value at a root that is NOT erased.  A zero value
 *   at an erased root is a byte that was right, not a failure.  With f = 0 this is the decoder of svsrs.h.
 *   A codeword whose syndromes are all 0 has the status 0 when f_c <= 32 and 255 when f_c > 32.
 *
 *   Known answers.  The data 00 01 .. 09 has the parity 6c 22 .. fb of svsrs.h: 42 bytes.
 *     - its first and its last byte erased (p = 41 and p = 0): Gamma = 01 d5 d4 (Gamma_0, Gamma_1, Gamma_2; alpha^41 = d4).
 *       Received with the first byte ff and the last byte right: status 1.  Both right: status 0.
 *     - its bytes 0 .. 31 erased and all received as ff: status 32, the word comes back.  Bytes 0 .. 30 erased and received as
 *       ff and byte 41 received as 04 (one error, 2 + 31 = 33): status 255, nothing written.
 *     - its bytes 0 .. 32 erased and received right: status 255.
 *
 * With d_erased NULL or all zero the stream, the status bytes and the counters are those of svs_rs_decode_dev.
 *
 * Refusals, in this order and before any device work:
 *   1. k = 0                                                   SVS_OK: nothing is done, no pointer is looked at
 *   2. k above SVS_RS_MAX_DATA_BYTES                           SVS_ERR_INVALID_ARG
 *   3. a NULL stream or status pointer                         SVS_ERR_INVALID_ARG
 *   4. d_counts neither NULL nor 4-byte aligned                SVS_ERR_INVALID_ARG
 *   5. status_capacity below C                                 SVS_ERR_CAPACITY
 *
 * Not here: a host decoder (the model lives in the tests), an encoder (svs_rs_encode of svsrs.h is the code's), and a source
 * of erasures other than the caller's own knowledge - the Viterbi decoder gives no reliability yet.
 */
#ifndef SVSRSE_H
#define SVSRSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVS_RSE_ABI_VERSION 1

#ifndef SVS_OK                    /* the codes of svsdct.h, for a caller that includes both */
#define SVS_OK 0
#define SVS_ERR_INVALID_ARG (-1)  /* NULL pointer / misaligned counters / length out of range */
#define SVS_ERR_HIP (-2)          /* a HIP runtime call failed; see svs_rse_last_error() */
#define SVS_ERR_NO_DEVICE (-3)    /* no usable AMD GPU */
#define SVS_ERR_CAPACITY (-4)     /* an output buffer is too small */
#endif

#ifndef SVS_RS_PARITY             /* the figures of svsrs.h, for a caller that includes this header alone */
#define SVS_RS_PARITY 32          /* parity bytes of every codeword */
#define SVS_RS_UNCORRECTABLE 255  /* the status of a codeword left as received */
#define SVS_RS_MAX_DATA_BYTES (1ull << 37)
#endif
#define SVS_RSE_MAX_ERASED 32     /* erased bytes a codeword stands: 2 e + f <= 32 */

int svs_rse_abi_version(void);
const char *svs_rse_last_error(void);

/* Decodes the k + 32 C bytes at d_stream IN PLACE, at any alignment, with the bytes that d_erased marks (k + 32 C bytes, any
 * alignment, never written; NULL: none) taken as erased: a codeword that decodes is replaced by the code word, one that does
 * not is not written.  d_status receives C bytes, one per codeword: the bytes changed, 0 .. 32, or 255; status_capacity is the
 * size of that buffer.  d_counts may be NULL; otherwise it is uint32[2] to which the call ADDS, with atomics that return
 * nothing, [0] += the bytes changed and [1] += the codewords with status 255.  One launch on `stream`. */
int svs_rse_decode_dev(uint8_t *d_stream, uint64_t k, const uint8_t *d_erased, uint8_t *d_status, uint64_t status_capacity,
                       uint32_t *d_counts, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SVSRSE_H */
