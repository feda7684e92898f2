/*
 * svsfec.h - C ABI of libsvsfec.so: a constraint-length-7 convolutional code and its soft-decision Viterbi decoder on the
 * MI355X (gfx950).  A second, small library beside libsvsdct.so (include/svsdct.h): it shares no code with the DCT kernels,
 * takes what svs_soft_extract_dev and svs_soft_vote_dev produce and returns the payload.  The reference
 * (erc-a/Secure-Video-Steganography-using-ECC-and-DCT) has no channel code; nothing here replaces a function of it.
 *
 * Conventions (those of svsdct.h)
 *   - plain C types only; every function that can fail returns SVS_OK (0) or a negative SVS_ERR_* code and never throws;
 *     svs_fec_last_error() gives the message for the calling thread.
 *   - the caller owns every buffer.  The `*_dev` entry points take DEVICE pointers and a hipStream_t (as void*; NULL = the
 *     null stream), enqueue one launch and return without synchronising.  They keep no state, allocate nothing and are
 *     re-entrant and thread-safe.  svs_fec_encode is host code: it needs no GPU.  The library reads no environment variable.
 *   - bits are packed MSB-first (numpy.packbits order): bit i is bit 7 - (i % 8) of byte i / 8.
 *
 * THE FORMAT, step by step.  Host and device compute it in integers, so the result is the same bits everywhere.
 *
 * Code
 *   constraint length 7: a state s is the last six input bits, the newest in bit 5.  rate = r is 2 or 3 (or a punctured code, below).
 *   generators (octal)   g_0 = 133, g_1 = 171          at rate 2 (rate 1/2),
 *                        g_0 = 133, g_1 = 171, g_2 = 165 at rate 3 (rate 1/3).
 *   one step, state s and input bit x:
 *       reg   = (x << 6) | s
 *       out_j = parity(reg & g_j), j = 0 .. r - 1, sent in this order
 *       s     = reg >> 1
 *   the encoder starts in state 0 and takes the n_info payload bits and then six zero tail bits, which return it to state 0:
 *       n = n_info + 6 steps,   n_coded = r * n coded bits,   coded bit r * t + j is out_j of step t.
 *   svs_fec_info_bits(capacity, r) = capacity / r - 6 (integer division; 0 when that is not positive) is the largest n_info
 *   whose coded stream fits `capacity` bits.
 *
 * Punctured codes
 *   the `rate` argument of every function is a code: 2 and 3 are the two rates above, and four more values name a punctured
 *   stream - the rate-2 code (generators 133, 171) with some coded bits not sent.  Period P; step t is step i = t mod P of its
 *   period and sends out_0 and out_1 where the row has a 1; K bits are sent a period:
 *       code                    P   out_0 (133) sent   out_1 (171) sent   K
 *       23  SVS_FEC_RATE_2_3    2   1 1                1 0                3
 *       34  SVS_FEC_RATE_3_4    3   1 1 0              1 0 1              4
 *       56  SVS_FEC_RATE_5_6    5   1 1 0 1 0          1 0 1 0 1          6
 *       78  SVS_FEC_RATE_7_8    7   1 1 1 1 0 1 0      1 0 0 0 1 0 1      8
 *   Every step sends at least one bit.
 *       pre[i] = the sent bits of the steps 0 .. i - 1 of a period (pre[0] = 0)
 *       S(t)   = (t div P) * K + pre[t mod P]        the sent bits before step t; strictly increasing
 *   the encoder runs the rate-2 encoder over its n = n_info + 6 steps and sends the kept bits of step t, out_0 before out_1, at
 *   the positions S(t) and following.  The last period is simply cut: n_sent = S(n) is what svs_fec_coded_bits(n_info, code)
 *   returns, and wherever this header says r * (n_info + 6) a punctured code has n_sent.
 *   svs_fec_info_bits(capacity, code) = (the largest n with S(n) <= capacity) - 6, 0 when that is not positive.
 *   the decoders take n_sent soft bytes or int32 values, one per sent bit, and turn each into its weight as below.  Mother bit
 *   2 t + j (out_j of step t) has the weight of its sent bit when it was sent and the weight 0 when not.  From there the decoder is
 *   the rate-2 decoder below, word for word: windows, start metrics, ties, traceback.  Zeros only make |bm| smaller, so the
 *   bound on the metrics holds unchanged.
 *
 * Weights
 *   the decoder sees one integer w per coded bit, positive for 1, |w| the confidence:
 *       from a soft byte (svs_soft_extract, svsdct.h: hard bit b in bit 7, margin m in bits 0..6)
 *                                  w = (2 b - 1) (2 m + 1)              - the vote of the soft vote, odd, 1 .. 255 in size;
 *       from an int32 value v, such as an entry of svs_soft_vote's tally (how copies of a coded stream combine)
 *                                  w = clamp(v, -32767, 32767).
 *
 * Decoder: a windowed Viterbi, defined so that segments are independent
 *   SVS_FEC_SEGMENT = 512 steps, SVS_FEC_OVERLAP = 64 steps.  Segment k is the steps [a, b) = [512 k, min(512 k + 512, n)).
 *   Its window is [ws, we) = [max(a - 64, 0), min(b + 64, n)): at most 640 steps.
 *   Path metrics are int32, M[s] for the 64 states.  Start: M[s] = 0 for every s; if ws = 0 instead M[0] = 0 and
 *   M[s] = -2^30 for s != 0 (the encoder starts in state 0).
 *   One add-compare-select step t = ws .. we - 1, for every new state ns = 0 .. 63 from the metrics before the step:
 *       p0 = 2 (ns & 31),  p1 = p0 + 1          the two predecessors;  x = ns >> 5 is the input bit of both branches
 *       bm = sum over j of (2 out_j - 1) w[r t + j]   with out_j of the branch (p0, x): the branch metric of p0.
 *            Every generator has bit 0 set, so each out_j of (p1, x) is the opposite bit and p1's branch metric is -bm.
 *       c0 = M[p0] + bm,  c1 = M[p1] - bm
 *       d(t, ns) = 1 if c1 > c0 else 0          p1 wins only when strictly larger
 *       M'[ns] = d ? c1 : c0
 *   Traceback: s = 0 when we = n (the tail ends in state 0); otherwise s = the lowest-numbered state with the largest metric.
 *   For t = we - 1 down to a:  the decoded bit of step t is s >> 5;  s = 2 (s & 31) + d(t, s).
 *   Only the bits of [a, b) are kept, and of those only t < n_info: the six tail steps carry no payload.
 *   No overflow: |bm| <= 3 * 32767 and a window has at most 640 steps, so a metric moves at most
 *   640 * 3 * 32767 = 62 912 640 < 2^30 from its start, the candidates c0 and c1 of the last step included; the lowest start is -2^30 and the highest 0, so
 *   every metric and every candidate stays inside (-2^31, 2^30).  No renormalisation is needed.
 *   The windowed decoder IS the format: with enough noise it differs from an untruncated Viterbi in a few bits.
 *
 * Refusals of svs_fec_encode and the two decoders, in this order and before any device work:
 *   1. rate other than 2, 3, 23, 34, 56, 78                               SVS_ERR_INVALID_ARG
 *   2. n_info = 0                                                          SVS_OK: nothing is done, no pointer is looked at
 *                                                                          (svs_fec_encode still reports *n_coded_out)
 *   3. n_info above SVS_FEC_MAX_INFO_BITS (2^40: the coded length of a larger one leaves what any device holds long before
 *      it leaves uint64, which the same test therefore covers)             SVS_ERR_INVALID_ARG
 *   4. a NULL input or output pointer                                      SVS_ERR_INVALID_ARG
 *   5. svs_fec_decode_weights_dev: weights not 4-byte aligned              SVS_ERR_INVALID_ARG
 *   6. the output buffer smaller than the call writes                      SVS_ERR_CAPACITY
 *   svs_fec_encode's n_coded_out may be NULL.
 */
#ifndef SVSFEC_H
#define SVSFEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVS_FEC_ABI_VERSION 1

#ifndef SVS_OK                    /* the codes of svsdct.h, for a caller that includes both */
#define SVS_OK 0
#define SVS_ERR_INVALID_ARG (-1)  /* bad rate / NULL pointer / misaligned weights / length out of range */
#define SVS_ERR_HIP (-2)          /* a HIP runtime call failed; see svs_fec_last_error() */
#define SVS_ERR_NO_DEVICE (-3)    /* no usable AMD GPU */
#define SVS_ERR_CAPACITY (-4)     /* an output buffer is too small */
#endif

#define SVS_FEC_SEGMENT 512       /* steps a segment decodes */
#define SVS_FEC_OVERLAP 64        /* steps of add-compare-select before and behind a segment */
#define SVS_FEC_TAIL 6            /* zero bits behind the payload */
#define SVS_FEC_MAX_INFO_BITS (1ull << 40)

/* values of `rate` beside 2 (rate 1/2) and 3 (rate 1/3): the punctured codes of "Punctured codes" above */
#define SVS_FEC_RATE_2_3 23
#define SVS_FEC_RATE_3_4 34
#define SVS_FEC_RATE_5_6 56
#define SVS_FEC_RATE_7_8 78

int svs_fec_abi_version(void);
const char *svs_fec_last_error(void);

/* r * (n_info + 6), under a punctured code S(n_info + 6); 0 for a rate that is none of the six or an n_info above
 * SVS_FEC_MAX_INFO_BITS */
uint64_t svs_fec_coded_bits(uint64_t n_info, int rate);
/* capacity / r - 6, under a punctured code (the largest n with S(n) <= capacity) - 6; 0 when that is not positive or the rate
 * is none of the six */
uint64_t svs_fec_info_bits(uint64_t capacity_bits, int rate);

/* Host only.  Encodes the first n_info bits of info_packed into coded_packed_out at `rate` (2, 3 or a punctured code, whose
 * unsent bits are left out: n_coded = n_sent): ceil(n_coded / 8) bytes are written, the
 * pad bits of the last one 0, no byte behind it; capacity_bytes is the size of the output buffer.  The input is not written;
 * the buffers must not overlap. */
int svs_fec_encode(const uint8_t *info_packed, uint64_t n_info, int rate, uint8_t *coded_packed_out, uint64_t capacity_bytes,
                   uint64_t *n_coded_out);

/* Decodes r * (n_info + 6) soft bytes at d_soft (under a punctured code its n_sent soft bytes, one per sent bit, and no more
 * are read) - coded bit i is byte i; a caller whose coded stream starts inside a buffer
 * offsets the pointer, any alignment - into ceil(n_info / 8) bytes at d_info_packed_out: the pad bits of the last byte are 0,
 * no byte behind it is written, the input is not written.  The buffers must not overlap.  One launch on `stream`. */
int svs_fec_decode_soft_dev(const uint8_t *d_soft, uint64_t n_info, int rate, uint8_t *d_info_packed_out,
                            uint64_t out_capacity_bytes, void *stream);

/* The same call on r * (n_info + 6) int32 weights (n_sent under a punctured code; 4-byte aligned), each clamped to
 * -32767 .. 32767: the tally of svs_soft_vote_dev at period = n_coded is such an array. */
int svs_fec_decode_weights_dev(const int32_t *d_weights, uint64_t n_info, int rate, uint8_t *d_info_packed_out,
                               uint64_t out_capacity_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SVSFEC_H */
