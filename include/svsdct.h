/*
 * svsdct.h - C ABI of libsvsdct.so: the MI355X (gfx950) implementation of the per-frame
 * 8x8 block-DCT / QIM embed-and-extract operator.
 *
 * What it replaces in the reference (erc-a/Secure-Video-Steganography-using-ECC-and-DCT):
 *   proses_frame_qim_dct(frame, mode, delta, bit_payload_segment, ..., num_ac_coeffs_to_use)
 *       config_and_setup.py:106-174      (the operator: mode 'embed' -> svs_embed*, 'extract' -> svs_extract*)
 *   its two frame loops, batched:
 *       embed_process.py:108-128         (frame k takes bits [k*cap, (k+1)*cap) of the stream)
 *       extract_process.py:55-86,173-182 (per-frame bit strings concatenated in frame order)
 * The reference has no FFI of its own (it is pure Python); the binding a maintainer adds is the
 * ctypes stub shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C types only; every function returns SVS_OK (0) or a negative SVS_ERR_* code and
 *     never throws; svs_last_error() gives the message for the calling thread.
 *   - the caller owns every buffer.  `*_dev` entry points take DEVICE pointers and a
 *     hipStream_t (as void*; NULL = the null stream), enqueue work and return without
 *     synchronising.  The entry points without the suffix take HOST pointers, stage through
 *     device memory and return when the result is in the host buffers: the frames travel in
 *     chunks over the upload and the download stream of a per-thread staging context (upload of
 *     chunk k+1 beside the download of chunk k: the link is full duplex), nothing is allocated per call once the context has grown to the
 *     largest call, and a page-locked caller buffer (svs_host_alloc) is the DMA's own
 *     source / target - pageable memory goes through the HIP runtime's staging (uploads at
 *     the same rate, downloads at about half of it: prefer page-locked OUTPUT buffers).
 *   - frames are gray uint8 planes, H and W multiples of 8 (the reference's callers crop:
 *     embed_process.py:94,113; extract_process.py:34,62), laid out [frame][row][col] with byte
 *     pitches given in svs_planes.
 *   - payload bits are packed MSB-first (numpy.packbits order): stream bit i is bit 7-(i%8) of
 *     byte i/8.  Stream bit i of a batch belongs to global block i / n_ac (frames in order,
 *     blocks in raster order inside a frame) and flat row-major coefficient 1 + i % n_ac of
 *     that block (config_and_setup.py:139-140) - so numpy.unpackbits of the extract output is
 *     the reference's '0'/'1' string.
 *   - n_ac is clamped to [0, 63] as the reference does (config_and_setup.py:138).
 *   - delta is passed as double: the quantiser divides in float32 by (float)delta and
 *     requantises with q*delta rounded once to float32, which is what the reference's
 *     `int(round(c / delta))` / `float(q * delta)` do for python int/float delta under
 *     NumPy >= 2 (config_and_setup.py:148,156,160).
 */
#ifndef SVSDCT_H
#define SVSDCT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVS_ABI_VERSION 4

#define SVS_OK 0
#define SVS_ERR_INVALID_ARG (-1)  /* bad geometry / NULL pointer / size overflow */
#define SVS_ERR_HIP (-2)          /* a HIP runtime call failed; see svs_last_error() */
#define SVS_ERR_NO_DEVICE (-3)    /* no usable AMD GPU */
#define SVS_ERR_CAPACITY (-4)     /* an output buffer is too small */

/* `flags` of the embed / extract entry points.  EVERY value gives the reference's stego pixels and extracted bits, bit for
 * bit; the flags only choose between two kernel families.  (The one exception is SVS_KEEP_COLOUR below, which the fused
 * colour embed alone accepts: there the GRAY of the output under the same weights is the reference's stego plane bit for
 * bit, while the BGR bytes intentionally differ from COLOR_GRAY2BGR.)
 *   0 / SVS_EXACT_GUARDED  (identical in behaviour; SVS_EXACT_GUARDED is kept as a named value for ABI compatibility and is
 *                      what the Python layer passes by default.)  Embedding with n_ac <= 15 and 0.25 <= delta <= 4096 runs the
 *                      STREAMING kernel (csrc/svs_device.hpp): every block goes HBM -> registers -> HBM once; the kernel
 *                      computes the payload coefficients exactly as pocketfft does (every quantiser decision is the
 *                      reference's), predicts each stego pixel from the sparse inverse of the coefficient changes, and keeps
 *                      the prediction only where a RIGOROUS per-block bound on the reference's own float32 round-trip noise
 *                      (tools/guard_bound.py: running error analysis of every pocketfft operation; BETA = u (17.0 mean +
 *                      31.05 ||block - mean||_2 + KD (1.5 delta + 0.01)) + 2^-20, KD = 19.6 for n_ac <= 7, 54.8 for
 *                      n_ac <= 15, and at least 2^-14 for n_ac = 8..15) proves the truncation cannot differ
 *                      (config_and_setup.py:166-171 transforms every block forth and back and truncates: x - 1e-5 becomes
 *                      x - 1).  The blocks it cannot decide (n_ac <= 7: 8 tests per block, 0.05 - 1.7 % of the blocks, 12.5 %
 *                      of flat ones at n = 3; n_ac = 8..15: 64 tests with position-dependent bounds, 1.5 - 13 %) are redone
 *                      INSIDE the launch with the pocketfft-identical arithmetic (eight lanes per block, LDS worklist
 *                      private to the wave) - no second launch, no scratch memory.  Every other embed call (n_ac >= 16, delta
 *                      outside the range) runs the SVS_EXACT_POCKETFFT kernel.  Extraction: n_ac <= 7 the
 *                      pocketfft-identical forward transform; n_ac >= 8 an FMA-factored transform, a block with a quantiser
 *                      input within a proven error bound of a rounding tie being recomputed with the pocketfft-identical
 *                      one - the reference's bits for ANY input frame.
 *   SVS_EXACT_POCKETFFT  every float32 operation of scipy.fftpack.dct/idct(norm='ortho') (pocketfft) is replayed in order, on
 *                      all 64 coefficients of every block, one lane per block.  About 5x the arithmetic of the streaming
 *                      kernel: VALU-bound (0.33 - 0.42 of the HBM roofline).  The yardstick the other kernels are tested
 *                      against.
 * The *_dev entry points keep no state at all; the host-pointer entry points keep a per-thread staging context (below).
 * Every entry point is re-entrant and thread-safe.  The library reads no environment variable. */
#define SVS_EXACT_POCKETFFT 1u
#define SVS_EXACT_GUARDED 2u
/* SVS_KEEP_COLOUR (svs_embed_bgr_dev / svs_embed_bgr only; every other entry point rejects it with SVS_ERR_INVALID_ARG):
 * opt-in.  Stego pixels keep the cover's colour instead of B = G = R: each output pixel is the cover pixel c shifted by
 * d = stego gray - gray(c) in all three channels, clamped to [0, 255], and - only where a channel clipped - walked channel by
 * channel (decreasing weight) to the nearest pixel whose gray is the stego gray (csrc/svs_colour.hpp).  The gray of the
 * output under the same weights is the reference's stego plane exactly, so extraction (which converts to gray first) gives
 * the reference's bits; blocks past the payload budget and pixels whose gray did not change are the cover's bytes.  The
 * default (flag clear) is still the reference's COLOR_GRAY2BGR output, byte for byte. */
#define SVS_KEEP_COLOUR 0x100u
/* SVS_READBACK (the gray embed calls: svs_embed_dev, svs_embed, svs_embed_str, svs_embed_ordered_dev, svs_embed_ordered and
 * the svs_embed_readback* calls below; the extract calls and svs_embed_bgr / svs_embed_bgr_dev reject it with
 * SVS_ERR_INVALID_ARG - the fused colour embed with read-back is svs_embed_bgr_readback* below): opt-in.  The reference's own stego can fail to decode: it clips the inverse transform to
 * [0, 255] and truncates it (config_and_setup.py:166-171), and in blocks near black or white (letterbox bars, flat or
 * saturated areas) that moves payload coefficients across a decision boundary - one wrong bit makes the receiver's AES-GCM
 * reject the whole payload.  With the flag the call first produces exactly the stego it produces without it, then reads
 * every block that carries payload bits back with the exact extraction arithmetic (the block the budget ends in: its first
 * bits only).  A block that reads back keeps its bytes - on content without failures the output is byte-identical to the
 * call without the flag.  A block that does not is repaired in place by a bounded, deterministic search (csrc/svs_readback.hpp:
 * over-relaxed corrections towards the nearest lattice point of each wanted bit, the block shifted off 0 / 255 where its range
 * allows, rounded to nearest, at most 16 steps) and accepted only when the exact read-back confirms every one of its bits; a
 * block the search cannot repair keeps the reference's bytes and is counted.  Repaired blocks are no longer the reference's
 * pixels (a letterbox bar is lifted off 0: visibly lighter blocks, lower PSNR), which is why the flag is opt-in.  What the
 * search leaves: blocks that clip at both ends (no shift helps) and small delta (delta = 4, n_ac = 3: a few blocks per
 * frame); at small delta it can also overshoot, and a few accepted blocks per frame decode but are visibly destroyed.  The receiver is unchanged: any extract call decodes the result.  The call needs the reference's stego as its start
 * and not the cover, so in-place calls keep working.  Only svs_embed_readback* report the counts.  The select and dithered
 * calls reject the flag too: their read-back form is svs_embed_dithered_readback* below. */
#define SVS_READBACK 0x200u
/* SVS_NEAREST (every embed call: svs_embed_dev, svs_embed, svs_embed_str, svs_embed_ordered*, svs_embed_readback*, svs_embed_bgr*,
 * svs_embed_bgr_readback*; every extract call rejects it with SVS_ERR_INVALID_ARG before any device work): opt-in.  It combines
 * freely with the mode bits, SVS_KEEP_COLOUR, SVS_READBACK and a block order.  The reference forces a coefficient's parity in a
 * fixed direction: when the index q = round_half_even(c / delta) has the wrong parity it writes q + 1 for bit 1 and q - 1 for
 * bit 0 (config_and_setup.py:150-155), which is the FARTHER of the two neighbouring lattice points for half of those
 * coefficients - a move of up to 1.5 delta.  With the flag the move goes to the nearer one:
 *     q (float32 division, round half to even) is the reference's; when its parity equals the bit, q is requantised as always;
 *     otherwise, with c0 = the float32 value written for q (float(q * delta): (float)q * (float)delta, or the once-rounded
 *     double product when delta is not a float32), q' = q + 1 if c > c0, q' = q - 1 if c < c0, and the reference's choice (+1
 *     for bit 1, -1 for bit 0) if c == c0; q' is requantised.
 * The side comes from c0 and not from c / delta - q, so the rule has no division-rounding corner.  A forced coefficient moves
 * by at most delta (plus rounding); in the coefficient domain the expected distortion falls from 7/12 delta^2 to 1/3 delta^2.
 * Everything else is the reference's: coefficient order and bit budget, the partial block, byte-identical blocks past the
 * budget, the delta <= 0 and n_ac = 0 routes (the flag has no effect there; an empty payload is still a copy), the pocketfft
 * inverse, clip, truncate.  With SVS_READBACK the read-back pass starts from the stego this rule wrote.
 * Cost: the outputs are NO LONGER the reference's stego pixels (a block whose bits already match everywhere is).  The receiver is
 * unchanged - extraction reads only q mod 2, any extract call decodes the result - and the default (flag clear) is
 * byte-identical to before.  Measured with the CPU oracle, one 480 x 640 frame, full-capacity random payload, PSNR against the
 * cover in dB, reference -> nearest (payload bit errors of the frame, reference -> nearest); "noise" is uniform in [16, 240):
 *     noise  n_ac = 3  delta = 8    44.95 -> 46.87  (0 -> 0)          noise  n_ac = 63 delta = 8    32.43 -> 34.84  (0 -> 0)
 *     noise  n_ac = 10 delta = 8    40.25 -> 42.50  (0 -> 0)          noise in [0, 256), n_ac = 63, delta = 8 (clips)
 *     noise  n_ac = 10 delta = 20   32.48 -> 34.88  (0 -> 0)                                        32.53 -> 34.93  (268 -> 6)
 *     smooth n_ac = 10 delta = 20   32.83 -> 34.27  (0 -> 0)          noise  n_ac = 3  delta = 4    49.27 -> 50.46  (218 -> 161)
 *     noise  n_ac = 7  delta = 2    50.38 -> 51.05  (7626 -> 7998)
 * 1.4 - 2.4 dB at the settings the application offers; delta >= 8 stays error-free where the reference's stego is; only
 * delta = 2, where the reference's own stego already fails, gets slightly worse. */
#define SVS_NEAREST 0x800u
/* SVS_MINMOVE (every embed call, as SVS_NEAREST; every extract call rejects it with SVS_ERR_INVALID_ARG before any device work):
 * opt-in minimum-move embedding.  It combines freely with the mode bits, SVS_KEEP_COLOUR, SVS_READBACK, a block order and a
 * coefficient selection.  The other rules write every payload coefficient ONTO a lattice point q' delta.  The receiver only
 * needs it INSIDE the decision cell of q' - within delta / 2 of the point - and far enough from the cell's edge to survive the
 * one disturbance on the way, the clip-and-truncate of the stego pixels.  That disturbance is bounded: the truncation error of
 * a pixel is in (-1, 0], an AC basis function b_k sums to 0, so in a block that does not clip the error of coefficient
 * k = 8 u + v is at most 0.5 sum|b_k| = 0.5 S_u S_v, with S_u = sum_x |a_u cos((2 x + 1) u pi / 16)|, a_0 = sqrt(1/8),
 * a_u = 1/2: between 3.284 and 4.0, and attained (e = -1 where b_k > 0, else 0).  The rule, float32 throughout, the same
 * operations in the same order on host and device, for a payload coefficient c with bit b at flat index k (under a
 * coefficient selection k is the selected index):
 *     t    = SVS_NEAREST's index: q (float32 division, round half to even) if its parity is b, else its q +- 1.  The flag
 *            implies the nearest direction: setting SVS_NEAREST as well changes nothing;
 *     c_t  = the float32 value written for t today (float(t * delta));
 *     h    = (float)(0.5 * (double)delta), rounded once on the host;  r_k = fmaxf(0, h - MARGIN[k]);
 *     c'   = fminf(fmaxf(c, c_t - r_k), c_t + r_k):  a coefficient inside the band keeps its forward-transform value exactly.
 * MARGIN[k] = (float)(0.5 S_u S_v + 0.0625) is a table of constants (csrc/svs_block.hpp, derivation above it); the 1/16 covers
 * the float32 noise of the round trip and the quantiser's division rounding.  The margin is the derived bound and not a tuning
 * knob: a uniform 2.0 already loses bits.  For delta <= 6.69 every r_k is 0 and the output is SVS_NEAREST's, byte for byte.
 * A coefficient moves by at most delta (plus rounding), so the streaming kernels and their guard take the rule as they are.
 * Everything else is the reference's: stream order and budget, the partial block, byte-identical blocks past the budget, the
 * delta <= 0, n_ac = 0 and empty-payload routes (the flag has no effect there), the pocketfft inverse of all 64 coefficients,
 * clip, truncate.  With SVS_READBACK the read-back pass starts from the stego this rule wrote.
 * Cost: the stego is NEITHER the reference's NOR the nearest rule's pixels.  Limit: the guarantee excludes blocks that clip at
 * 0 / 255 (their error is not bounded by the margin); SVS_READBACK is the remedy there and combines with the flag (under a
 * selection or a dither: svs_embed_dithered_readback*).  The
 * receiver is unchanged and the default (flag clear) is byte-identical to before.
 * Measured ON THE CPU with the oracle's pieces (tests/minmove_lib.py model_embed), one 480 x 640 frame, full-capacity random
 * payload; PSNR against the cover in dB / payload bit errors, reference | SVS_NEAREST | SVS_MINMOVE:
 *     noise  n_ac = 10 delta = 20 (the GUI's default)  32.50 / 0 | 34.90 / 0 | 39.71 / 0
 *     noise  n_ac = 3  delta = 20                      37.62 / 0 | 39.96 / 0 | 44.45 / 0
 *     noise  n_ac = 10 delta = 12                      36.85 / 0 | 39.18 / 0 | 41.82 / 0
 *     noise  n_ac = 10 delta = 40                      26.53 / 0 | 28.90 / 0 | 35.64 / 0
 *     noise  n_ac = 63 delta = 20                      24.59 / 2 | 26.97 / 0 | 32.00 / 0
 *     noise  n_ac = 10 delta = 8                       40.22 / 0 | 42.49 / 0 | 43.00 / 0
 *     smooth n_ac = 10 delta = 20                      32.80 / 0 | 34.31 / 0 | 38.39 / 0
 *     smooth n_ac = 63 delta = 20                      25.05 / 168 | 26.18 / 0 | 30.25 / 0
 * (0x400 is deliberately not a flag.) */
#define SVS_MINMOVE 0x1000u

/* Geometry of a batch of gray planes. */
typedef struct svs_planes {
    int32_t n_frames;
    int32_t height;      /* multiple of 8 */
    int32_t width;       /* multiple of 8 */
    int32_t reserved;    /* set to 0 */
    int64_t row_pitch;   /* bytes between rows, >= width, multiple of 8 */
    int64_t frame_pitch; /* bytes between frames, >= height*row_pitch, multiple of 8 */
} svs_planes;

/* ---- library / device ------------------------------------------------------------------ */
int svs_abi_version(void);
const char *svs_last_error(void);
int svs_device_count(int *count);
/* Select the device for the calling thread (hipSetDevice) and check it is usable. */
int svs_init(int device);
/* Name of the architecture the device reports, e.g. "gfx950". */
int svs_device_arch(int device, char *buf, size_t buf_len);
/* Releases the CALLING THREAD's staging context of the host-pointer entry points (svs_embed, svs_extract, svs_embed_bgr,
 * svs_extract_bgr, svs_embed_str, svs_extract_str): two streams and device buffers sized by the calls the thread makes (a
 * buffer above 64 MB of which eight calls in a row used less than a quarter is given back).  A thread's context is also
 * released when the thread exits; calling any host-pointer entry point afterwards simply builds a new one.  The *_dev entry
 * points keep nothing. */
int svs_shutdown(void);

/* ---- device memory / stream helpers for callers that do not bring their own ------------- */
int svs_malloc(void **dev_ptr, size_t bytes);
int svs_free(void *dev_ptr);
int svs_memcpy_h2d(void *dev_dst, const void *host_src, size_t bytes, void *stream);
int svs_memcpy_d2h(void *host_dst, const void *dev_src, size_t bytes, void *stream);
int svs_memset(void *dev_dst, int value, size_t bytes, void *stream);
int svs_stream_synchronize(void *stream);
/* Streams and pinned (page-locked) host memory for callers that overlap frame I/O with the kernels
 * (svsdct/pipeline.py): copies to/from pinned memory run asynchronously and at full link rate. */
int svs_stream_create(void **stream);
int svs_stream_destroy(void *stream);
int svs_host_alloc(void **host_ptr, size_t bytes);
int svs_host_free(void *host_ptr);

/* ---- capacity arithmetic ------------------------------------------------------------------ */
/* bits one batch carries: n_frames * (H/8) * (W/8) * clamp(n_ac, 0, 63) */
uint64_t svs_capacity_bits(const svs_planes *p, int n_ac);
/* bytes svs_extract* writes for that many bits: ceil(bits / 8) */
uint64_t svs_packed_bytes(uint64_t n_bits);

/* ---- the operator: embed -----------------------------------------------------------------
 * Replaces mode 'embed' of proses_frame_qim_dct (config_and_setup.py:117-172) for a whole batch
 * and the offset bookkeeping of embed_process.py:116-128.
 *   gray / stego : [n_frames] planes described by `planes` (same geometry for both); may alias.
 *   bits_packed  : MSB-first packed payload; the first stream bit used is `bit_offset`
 *                  (lets every rank index one shared buffer by its frame offset); the buffer
 *                  must be 4-byte aligned and readable up to a multiple of 4 bytes.
 *   n_bits       : bits available from bit_offset on.  min(n_bits, capacity) are embedded.
 *                  Blocks past the budget are copied byte-identically; a block the budget ends
 *                  in has only its first coefficients modified (config_and_setup.py:130,132,141).
 *   n_embedded   : (host) receives min(n_bits, capacity); 0 when delta <= 0 or n_ac <= 0.
 * delta <= 0 or n_ac <= 0: nothing can be embedded; as in the reference every block is still transformed forth and
 * back when n_bits > 0 (config_and_setup.py:143-145,166-169) - both modes run the exact arithmetic for that.
 * No scratch memory and no state between calls: concurrent calls from several host threads or on several streams are
 * independent (work on one stream is ordered as usual).
 */
int svs_embed_dev(const uint8_t *d_gray, uint8_t *d_stego, const svs_planes *planes,
                  double delta, int n_ac,
                  const uint8_t *d_bits_packed, uint64_t bit_offset, uint64_t n_bits,
                  uint32_t flags, uint64_t *n_embedded, void *stream);

int svs_embed(const uint8_t *gray, uint8_t *stego, const svs_planes *planes,
              double delta, int n_ac,
              const uint8_t *bits_packed, uint64_t bit_offset, uint64_t n_bits,
              uint32_t flags, uint64_t *n_embedded);

/* The same call in the reference operator's own types (config_and_setup.py:106-109,172): the payload is `bit_payload_segment`,
 * a string of '0' / '1' characters (one character per bit, no terminator needed), and the operator's first return value - the
 * gray frame before embedding, as an array of its own (:113-114) - is produced as well.
 *   bits_ascii, n_chars : n_chars characters are available, min(n_chars, capacity) are read (each must be '0' or '1':
 *                         SVS_ERR_INVALID_ARG otherwise - other characters have no pinned meaning in the reference) - a frame loop may hand over the
 *                         whole remaining payload as the reference does (embed_process.py:116-121) - and are packed on the
 *                         device.  n_chars > 0 with nothing embeddable (delta <= 0, n_ac <= 0) still round-trips every block,
 *                         n_chars = 0 (or NULL) copies the frames, as in the reference (:124-126).
 *   gray_ref_out        : NULL, or a buffer of the planes' geometry that receives a copy of `gray` (pixel bytes only): the
 *                         frames BEFORE embedding, also when stego aliases gray (in-place embedding - the copy is then made
 *                         before the first download; otherwise the calling thread makes it while the GPU works).  It may be
 *                         `gray` itself (no copy); it must not overlap `stego`, nor overlap `gray` partially
 *                         (SVS_ERR_INVALID_ARG).  The up / down overlap of the call needs page-locked stego memory
 *                         (svs_host_alloc): a pageable download blocks the calling thread. */
int svs_embed_str(const uint8_t *gray, uint8_t *gray_ref_out, uint8_t *stego, const svs_planes *planes,
                  double delta, int n_ac, const char *bits_ascii, uint64_t n_chars,
                  uint32_t flags, uint64_t *n_embedded);

/* ---- the operator: extract ----------------------------------------------------------------
 * Replaces mode 'extract' (config_and_setup.py:159-165,173-174) for a whole batch and the
 * concatenation of extract_process.py:76,181.
 *   bits_packed_out : receives svs_packed_bytes(capacity) bytes (the last byte zero padded);
 *                     must be 4-byte aligned; out_capacity_bytes is its size.
 *   n_bits_out      : (host) receives the capacity in bits.
 * delta <= 0: every bit is 0 (config_and_setup.py:143-145).
 */
int svs_extract_dev(const uint8_t *d_gray, const svs_planes *planes, double delta, int n_ac,
                    uint8_t *d_bits_packed_out, uint64_t out_capacity_bytes,
                    uint32_t flags, uint64_t *n_bits_out, void *stream);

int svs_extract(const uint8_t *gray, const svs_planes *planes, double delta, int n_ac,
                uint8_t *bits_packed_out, uint64_t out_capacity_bytes, uint32_t flags,
                uint64_t *n_bits_out);

/* Extraction into the reference operator's own return type: the '0' / '1' string of config_and_setup.py:173-174, one
 * character per bit (no terminator is written).  bits_ascii_out receives capacity characters; out_capacity_chars is its size. */
int svs_extract_str(const uint8_t *gray, const svs_planes *planes, double delta, int n_ac,
                    char *bits_ascii_out, uint64_t out_capacity_chars, uint32_t flags,
                    uint64_t *n_bits_out);

/* ---- the operator with a keyed block order -------------------------------------------------------------
 * Opt-in.  Without an order, the payload fills the blocks of each frame in raster order from the top-left block, as in the
 * reference: a payload that fills part of a frame's capacity sits in its top rows, where a frame difference shows it.  With
 * an order, stream slot j of frame f of the call - stream bits bit_offset + (f*N + j)*n_ac ... + n_ac - 1, N = (H/8)*(W/8) -
 * goes to block sigma_t(j) of that frame, t = first_frame + f: a key-seeded permutation of the frame's blocks
 * (csrc/svs_order.hpp; svsdct/order.py restates it).  Frames keep the stream ranges they have without an order; only the
 * blocks inside a frame are reordered.  Every block is still embedded or extracted exactly as the reference does it, so
 *     ordered embed(F)   = P^-1(reference embed(P(F)))     ordered extract(S) = reference extract(P(S))
 * where P moves block sigma_t(j) of frame t to raster position j - stego pixels included, in every mode.
 * The permutation is NOT cryptographic: it hides where the payload sits from a look at the frame; confidentiality comes
 * from encrypting the payload.  Sender and receiver must use the same key and the same clip frame index for every frame.
 *   order : NULL = the call without an order (the same kernels, the same bytes).  Otherwise key (every value valid, 0
 *           included), first_frame (the clip index of the call's first frame), reserved (must be 0, else
 *           SVS_ERR_INVALID_ARG).
 * Every other argument, flag and contract is that of svs_embed_dev / svs_embed / svs_extract_dev / svs_extract.  A keyed
 * extract clears its output range on the call's stream and ORs each block's bits into it with 32-bit atomics; it writes no
 * byte that the call without an order does not write.  The fused colour calls and the _str calls have no ordered form. */
typedef struct svs_block_order {
    uint64_t key;
    uint32_t first_frame;   /* clip index of the call's first frame: frame f uses t = first_frame + f */
    uint32_t reserved;      /* must be 0 */
} svs_block_order;

int svs_embed_ordered_dev(const uint8_t *d_gray, uint8_t *d_stego, const svs_planes *planes,
                          const svs_block_order *order, double delta, int n_ac,
                          const uint8_t *d_bits_packed, uint64_t bit_offset, uint64_t n_bits,
                          uint32_t flags, uint64_t *n_embedded, void *stream);

int svs_extract_ordered_dev(const uint8_t *d_gray, const svs_planes *planes, const svs_block_order *order,
                            double delta, int n_ac, uint8_t *d_bits_packed_out, uint64_t out_capacity_bytes,
                            uint32_t flags, uint64_t *n_bits_out, void *stream);

/* Host-pointer forms, through the same staging context as svs_embed / svs_extract.  A keyed embed stages whole frames
 * (a frame's blocks can take any slot of its stream range), so a batch is never cut inside a frame. */
int svs_embed_ordered(const uint8_t *gray, uint8_t *stego, const svs_planes *planes, const svs_block_order *order,
                      double delta, int n_ac, const uint8_t *bits_packed, uint64_t bit_offset, uint64_t n_bits,
                      uint32_t flags, uint64_t *n_embedded);

int svs_extract_ordered(const uint8_t *gray, const svs_planes *planes, const svs_block_order *order, double delta,
                        int n_ac, uint8_t *bits_packed_out, uint64_t out_capacity_bytes, uint32_t flags,
                        uint64_t *n_bits_out);

/* ---- the operator with a coefficient selection ---------------------------------------------------------
 * Opt-in.  Without a selection the payload goes into flat row-major coefficients 1..n_ac of each block, as in the reference:
 * at n_ac = 3 only the horizontal frequencies (0,1), (0,2), (0,3) carry bits, at the GUI's default 10 the whole first row and
 * almost nothing vertical.  A SELECTION is an ordered list of `count` distinct flat row-major indices in 1..63 (index
 * 8*u + v is vertical frequency u, horizontal v; DC, index 0, is never selectable): stream bit i of a block goes to
 * coefficient index[i] instead of 1 + i, and extraction emits q mod 2 of coefficient index[i] at block-local position i.
 * Everything else is the reference's, with n_ac = count: frames and blocks take the same stream ranges, count bits per block;
 * the block the budget ends in has only its first coefficients (in selection order) modified; blocks past the budget are
 * byte-identical to the cover; delta <= 0, an empty payload and count = 0 take the routes of n_ac = 0; float32 division,
 * round half to even, the q +- 1 rule (or SVS_NEAREST), float(q * delta), pocketfft inverse, clip, truncate.  Two identities
 * hold exactly: the selection 1, 2, .., n gives the bytes and bits of the call without a selection at n_ac = n, in every mode
 * (and runs its kernels); and for any frames, selected extraction equals the n_ac = 63 extraction with each block's 63 bits
 * gathered at index[i] - 1.  Capacity is n_frames * (H/8) * (W/8) * count.  Sender and receiver must agree on the selection.
 * Why: the transform is orthonormal, so the distortion per forced coefficient does not depend on which one it is (PSNR
 * against the cover moves by less than 0.1 dB), but robustness does - with only row-0 coefficients modified the truncation
 * errors are perfectly correlated down the columns, which is what costs the reference's own stego bits at small delta.  CPU
 * oracle, one 480 x 640 frame of noise in [16, 240), full-capacity random payload, payload bit errors of row-major / zig-zag
 * from scan position 1 / zig-zag from 6:  delta = 4, count = 3 (14 400 bits): 235 / 113 / 54;  delta = 2, count = 7
 * (33 600): 7 660 / 356 / 191;  delta >= 8: 0 / 0 / 0.
 * Cost: any selection but the prefix runs the lane-per-block SVS_EXACT_POCKETFFT kernels whatever the mode bits say (the
 * streaming embed guard and the FAST extract margins are derived for row-major prefixes only): 0.34 - 0.42 of the HBM
 * roofline against 0.78 for the default n_ac <= 7 embed.  The ratio of a selected call to the SVS_EXACT_POCKETFFT call at the
 * same n_ac has NOT been measured on a GPU yet: tools/coeff_select_rates.py measures it at 200 x 4K (counts 3, 10, 63) and
 * writes profiles/coeff_select_rates.txt.  Both run the same quantiser steps; the selected loop adds scalar table reads and
 * covers all 63 positions with a wave-uniform test each, where the n_ac <= 15 exact kernels cover one or two rows.
 * There is no colour and no _str form; these calls refuse SVS_READBACK - the selected embed with read-back and repair is
 * svs_embed_dithered_readback* below (dither NULL).
 *   coeffs : the selection; the unused tail of index must be 0.  NULL, an index of 0 or above 63, a duplicate, count > 63 or
 *            a non-zero tail: SVS_ERR_INVALID_ARG before any device work.
 *   order  : NULL or a keyed block order, as in the ordered calls (a keyed host embed stages whole frames).
 *   flags  : the mode bits are accepted and do not change the output; SVS_NEAREST on embed (rejected on extract, as
 *            elsewhere); SVS_READBACK, SVS_KEEP_COLOUR and anything else: SVS_ERR_INVALID_ARG.
 * Every other argument and contract is that of the ordered calls. */
typedef struct svs_coeffs {
    uint8_t count;       /* 0..63 */
    uint8_t index[63];   /* index[i]: the coefficient of a block's stream bit i; index[count..] must be 0 */
} svs_coeffs;

#define SVS_SCAN_ROW_MAJOR 0
#define SVS_SCAN_ZIGZAG 1   /* JPEG zig-zag: 0, 1, 8, 16, 9, 2, 3, 10, ...; position 0 is DC */
/* out = scan positions first .. first + count - 1 of the scan (first >= 1, count >= 0, first + count <= 64; else
 * SVS_ERR_INVALID_ARG).  Host only: needs no GPU. */
int svs_coeffs_scan(svs_coeffs *out, int scan, int first, int count);

int svs_embed_select_dev(const uint8_t *d_gray, uint8_t *d_stego, const svs_planes *planes, const svs_block_order *order,
                         const svs_coeffs *coeffs, double delta, const uint8_t *d_bits_packed, uint64_t bit_offset,
                         uint64_t n_bits, uint32_t flags, uint64_t *n_embedded, void *stream);

int svs_extract_select_dev(const uint8_t *d_gray, const svs_planes *planes, const svs_block_order *order,
                           const svs_coeffs *coeffs, double delta, uint8_t *d_bits_packed_out, uint64_t out_capacity_bytes,
                           uint32_t flags, uint64_t *n_bits_out, void *stream);

/* Host-pointer forms, through the same staging context as svs_embed_ordered / svs_extract_ordered. */
int svs_embed_select(const uint8_t *gray, uint8_t *stego, const svs_planes *planes, const svs_block_order *order,
                     const svs_coeffs *coeffs, double delta, const uint8_t *bits_packed, uint64_t bit_offset, uint64_t n_bits,
                     uint32_t flags, uint64_t *n_embedded);

int svs_extract_select(const uint8_t *gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                       double delta, uint8_t *bits_packed_out, uint64_t out_capacity_bytes, uint32_t flags,
                       uint64_t *n_bits_out);

/* ---- the operator with a keyed dither (dither modulation, DM-QIM) ---------------------------------------
 * Opt-in.  Every embed rule (the reference's, SVS_NEAREST, SVS_MINMOVE) quantises onto the lattice q * delta anchored at 0, so
 * a stego frame announces itself - its recomputed payload coefficients sit within 0.5 S_u S_v <= 4.0 of a multiple of delta,
 * a comb in the histogram of c mod delta that anyone can test for - and anyone who knows delta and n_ac (the application's
 * defaults are public) reads the bits.  With a dither both sides shift the lattice of every payload coefficient by a
 * key-derived offset d in [-delta, delta).  QIM distortion is shift invariant, so it costs no distortion; the transform, the
 * inverse, the budget, the block order and the embedding rule do not change.
 * The rule is a FORMAT: sender and receiver must compute the same thing.  For clip frame t = first_frame + f, raster block
 * index i inside the frame (the block's physical position, not its stream slot: the rule does not depend on a keyed order)
 * and flat row-major coefficient index k in 1..63, with lb = lowbias32 (csrc/svs_order.hpp) and all integer
 * arithmetic mod 2^32:
 *     seed = lb(lb(hi32(key) ^ 0x85EBCA6B) ^ lo32(key))      (not the block order's seed: one key may serve both)
 *     s_t  = lb(seed ^ t)
 *     s_b  = lb(s_t + i * 0x9E3779B1)
 *     h    = lb(s_b ^ (k * 0x632BE5AB))
 *     r    = (float)(h >> 8) * 2^-23 - 1.0f                  (exact in float32, in [-1, 1))
 *     d    = r * (float)delta                                (one float32 multiply)
 * The dither covers a whole parity period [-delta, delta), not [-delta/2, delta/2): with the half range a receiver with the
 * wrong key still reads 75 % of the bits (the difference of two dithers is triangular on (-delta, delta), P(|x| > delta/2) =
 * 1/4); with the full period the wrong-key bit error rate is 1/2.
 *   embed, payload coefficient c, bit b:  c' = c - d (one float32 subtract);  cn' = what the call's rule writes for (c', b)
 *            (reference, SVS_NEAREST or SVS_MINMOVE; the minimum-move band is that of flat index k);  the written value is c
 *            itself when cn' equals c' bitwise, else cn' + d (one float32 add) - a coefficient that the minimum-move rule
 *            leaves alone keeps its forward-transform value exactly.
 *   extract: bit = quant_index(c - d) & 1, with the same subtract.
 * Everything else is the reference's: stream ranges and the block budget, the block the budget ends in, byte-identical blocks
 * past the budget, the delta <= 0, n_ac = 0 and empty-payload routes (the bytes of the call without a dither), the
 * pocketfft inverse of all 64 coefficients, clip and truncate.  Every float step is a single IEEE float32 operation with no
 * contraction, in the same order on the host build of the block bodies and on the device.
 * lowbias32 is NOT a cryptographic generator (as csrc/svs_order.hpp says of the block order).  The dither removes the keyless
 * test and the keyless read; the payload's confidentiality remains AES-GCM's.
 * Measured on the CPU model (tests/test_dither_cpu.py: one 240 x 320 frame of noise in [64, 192), delta = 20, n_ac = 10, full
 * payload, reference rule): the share of recomputed payload coefficients within delta/4 of a multiple of delta is 1.000
 * without a dither and 0.502 with one; bit errors 0 with the right key, a bit error rate of 0.498 with another key and 0.506
 * for the extract without a dither; PSNR against the cover 32.42 / 34.85 / 39.64 dB without a dither and 32.47 / 34.89 / 39.70
 * with one (reference / SVS_NEAREST / SVS_MINMOVE).
 * Cost: a dithered call always runs the lane-per-block SVS_EXACT_POCKETFFT kernels with all eight coefficient rows, whatever
 * the mode bits say (the streaming embed guard and the FAST extract tie margins are derived for an undithered quantiser
 * input), behind one wave-uniform branch in their eight-row instantiations; on top of that come one integer hash and two float
 * operations per payload coefficient.  tools/dither_rates.py times it against the SVS_EXACT_POCKETFFT call at the same n_ac
 * and against the selected call, at 200 x 4K (n_ac = 3, 10, 63).
 * There is no colour and no _str form; these calls refuse SVS_READBACK - the dithered embed with read-back and repair is
 * svs_embed_dithered_readback* below.
 *   order  : NULL or a keyed block order, as in the ordered calls.
 *   coeffs : NULL (the row-major prefix 1..n_ac) or a coefficient selection, checked as in the select calls; n_ac is then
 *            ignored and the selection's count rules.  The dither of a coefficient is that of its flat index k, whatever slot
 *            it carries.
 *   dither : required.  NULL or reserved != 0: SVS_ERR_INVALID_ARG before any device work.  When order is given too, the two
 *            first_frame values must be equal (else SVS_ERR_INVALID_ARG): a caller cannot desynchronise them silently.
 *   flags  : the mode bits are accepted and change nothing; SVS_NEAREST and SVS_MINMOVE on embed (rejected on extract, as
 *            elsewhere); SVS_READBACK, SVS_KEEP_COLOUR, 0x400 and anything else: SVS_ERR_INVALID_ARG.
 * The host-pointer forms go through the per-thread staging context and stage whole frames, as the keyed calls do, so that a
 * chunk boundary never changes a block's (t, i).  Every other argument and contract is that of the ordered calls. */
typedef struct svs_dither {
    uint64_t key;           /* every value valid, 0 included */
    uint32_t first_frame;   /* clip index of the call's first frame: frame f uses t = first_frame + f */
    uint32_t reserved;      /* must be 0 */
} svs_dither;

int svs_embed_dithered_dev(const uint8_t *d_gray, uint8_t *d_stego, const svs_planes *planes, const svs_block_order *order,
                           const svs_coeffs *coeffs, const svs_dither *dither, double delta, int n_ac,
                           const uint8_t *d_bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t flags,
                           uint64_t *n_embedded, void *stream);

int svs_extract_dithered_dev(const uint8_t *d_gray, const svs_planes *planes, const svs_block_order *order,
                             const svs_coeffs *coeffs, const svs_dither *dither, double delta, int n_ac,
                             uint8_t *d_bits_packed_out, uint64_t out_capacity_bytes, uint32_t flags, uint64_t *n_bits_out,
                             void *stream);

int svs_embed_dithered(const uint8_t *gray, uint8_t *stego, const svs_planes *planes, const svs_block_order *order,
                       const svs_coeffs *coeffs, const svs_dither *dither, double delta, int n_ac, const uint8_t *bits_packed,
                       uint64_t bit_offset, uint64_t n_bits, uint32_t flags, uint64_t *n_embedded);

int svs_extract_dithered(const uint8_t *gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                         const svs_dither *dither, double delta, int n_ac, uint8_t *bits_packed_out, uint64_t out_capacity_bytes,
                         uint32_t flags, uint64_t *n_bits_out);

/* ---- soft-decision extraction: a reliability byte per payload bit ----------------------------------------
 * The extract calls above return hard bits, q mod 2 per payload coefficient.  These return, per capacity bit, the hard bit
 * AND how far the coefficient sits from the nearest decision boundary of its quantiser cell - the quantity SVS_NEAREST,
 * SVS_MINMOVE, read-back, the selection and the dither all work on at the sending end.  A sender reads from it how much
 * disturbance a stego clip survives; a receiver sees which frames sit on the lattice; a caller that embedded the payload more
 * than once (by tiling it) combines the copies by their reliabilities (svsdct/soft.py, combine; on the device: svs_soft_vote*).  The per-frame view of the first two uses: svs_soft_histogram*.
 * The byte is a FORMAT, a contract between builds as the dither's rule is.  Layout: one byte per capacity bit in stream order;
 * byte i belongs to stream bit i of the hard extract call with the same order, coeffs, dither, delta and n_ac.  For the
 * payload coefficient with quantiser input x - x = c for a call without a dither, x = c - d under one, c the
 * pocketfft-identical forward transform and d exactly the dither's d above:
 *     q    = quant_index(x)                                  (the extract call's own index: int(round(x / (float)delta)))
 *     x0   = (float)q * (float)delta                         (one float32 multiply, whatever delta is)
 *     a    = fabsf(x - x0)
 *     h    = 0.5f * (float)delta
 *     s    = (float)(254.0 / (double)(float)delta)           (rounded once, on the host)
 *     m    = clamp((int)((h - a) * s), 0, 127)               (one subtract, one multiply, truncation toward zero)
 *     byte = ((q & 1) << 7) | m
 * Every float step is a single IEEE float32 operation with no contraction, in the same order on the host build of the block
 * bodies and on the device.  byte >> 7 is the hard bit; byte & 127 is the distance from the nearest decision boundary in units
 * of delta / 254: 127 on the lattice point, 0 on (or, through the roundings of x / delta and q * delta, just past) the boundary.
 * It is a DISTANCE, not a probability: what it says about the chance of a bit error depends on the disturbance, which the
 * library does not know.  delta <= 0: every byte is 0.  n_ac clamps to [0, 63]; a capacity of 0 writes nothing.
 * Limits: the dither is lowbias32's, no cryptographic generator, and a selection says which coefficients are read, nothing
 * more - a reader without the dither's key sees reliabilities uniform on 0..127 (the comb is gone), one with the wrong
 * selection reads other coefficients.  Measured on the CPU model only (tests/test_soft_extract_cpu.py; README.md has the
 * table): at delta = 20, n_ac = 10 on noise in [64, 192) undisturbed reference-rule stego has no reliability below 113 and a
 * never-embedded frame a mean of 63.5; three tiled copies under uniform pixel noise of +-8 decode with 3 bit errors by soft
 * vote, 10 by hard majority, 87 - 96 alone.  NOT measured: the call's time on the device (tools/soft_extract_rates.py is
 * there for it).  What requantisation on the 8x8 grid does to the same three copies is measured, on the CPU model of
 * svs_requantise* below; a real encoder (rate control, chroma, inter prediction, in-loop filters) is not.
 * Cost: a soft call always runs the lane-per-block SVS_EXACT_POCKETFFT extract kernel with all eight coefficient rows, whatever
 * the mode bits say, behind one wave-uniform branch of its eight-row instantiations; every wave assembles its blocks' bytes in
 * LDS that only this launch requests and copies them out coalesced, each byte written once (no clearing, no atomics).
 * There is no colour and no _str form.
 *   order, coeffs, dither : each NULL or as in the dithered calls, and checked as there (svs_coeffs, the reserved fields, equal
 *            first_frame values when order and dither are both given); with coeffs n_ac is ignored and the count rules.
 *   d_soft_out / soft_out : at least capacity bytes (else SVS_ERR_CAPACITY); the device pointer 4-byte aligned.  Exactly
 *            capacity bytes are written.
 *   flags  : as the extract calls - the mode bits are accepted and change nothing, embed flags and anything else are refused.
 *   n_bits_out : receives the capacity, the number of bytes written.
 * Every refusal comes before any device work.  The host form stages as svs_extract does. */
int svs_soft_extract_dev(const uint8_t *d_gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                         const svs_dither *dither, double delta, int n_ac, uint8_t *d_soft_out, uint64_t out_capacity_bytes,
                         uint32_t flags, uint64_t *n_bits_out, void *stream);

int svs_soft_extract(const uint8_t *gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                     const svs_dither *dither, double delta, int n_ac, uint8_t *soft_out, uint64_t out_capacity_bytes, uint32_t flags,
                     uint64_t *n_bits_out);

/* ---- fused soft vote: the copies of a tiled payload folded on the device ----------------------------------
 * A payload of `period` bits embedded copy after copy through the stream (the sender tiles the stream itself and embeds it as any
 * other, the last copy cut where the capacity ends; svsdct/soft.py, tile) is decoded by a vote of the soft bytes of its copies.
 * These calls run the soft extraction and vote in the same launch: the soft bytes are never written, each is added into a tally
 * of `period` int32 values, and the tally's 4 * period bytes are all that leaves the device.  The tally is a FORMAT, as the soft
 * byte is.  With i the index of a capacity bit within the call, in exactly the order and layout of svs_soft_extract with the
 * same order, coeffs, dither, delta and n_ac, p = stream_bit0 + i its stream position, j = p mod period, `byte` its soft byte,
 * b = byte >> 7 and m = byte & 127:
 *     tally[j] += 2 * (2b - 1) * (2m + 1)        for every capacity bit of the call
 *     tally[j] += (2b - 1)                       additionally, where p < period   (copy 0 breaks ties)
 *     bit[j]    = tally[j] > 0
 * An entry is odd once copy 0 has been counted and then never zero; its sign is svsdct/soft.py combine's bit, the rule that a
 * zero score takes copy 0's bit included, and (tally[j] - (2 b0[j] - 1)) / 2, b0 copy 0's hard bit, is combine's score.  All
 * arithmetic is integer: the result does not depend on the order of the additions, so the calls are deterministic though the
 * device adds with atomics.
 * Overflow: one copy contributes at most 511 in magnitude.  A call whose capacity exceeds period * 2^22 is refused, so the at
 * most 2^22 + 1 copies of one call stay below 2.14e9 < 2^31.  Across several calls into one tally the caller owns the bound.
 *   period      : the payload's length in bits, 1 .. 2^61 - 1; both sides agree on it (nothing in the stream says it).
 *   stream_bit0 : the stream position of the call's first capacity bit - for a clip processed in batches the capacity of the
 *            frames before the batch; under an order or a dither first_frame advances as in every other call.
 *   d_tally  : period int32 values in device memory, 4-byte aligned.  The call ADDS into it, as the read-back calls add into
 *            d_counts: zero it before the first call.  It keeps no state and allocates nothing.
 *   tally_out : period int32 values in host memory.  The host form stages as svs_extract does, votes into a zeroed tally of its
 *            per-thread staging context and WRITES exactly period values; a caller with several calls adds the arrays.
 *   order, coeffs, dither, planes, flags : as svs_soft_extract*, checked as there; the mode bits are accepted and change nothing.
 *   n_bits_out : receives the capacity, the number of bits that voted.
 * SVS_ERR_INVALID_ARG: embed flags or unknown ones; period 0 or above 2^61 - 1; delta <= 0 (every soft byte is 0 there and a
 * vote over them says nothing); with a capacity above 0, a NULL tally, a device tally that is not 4-byte aligned, or a capacity
 * above period * 2^22.  Every refusal comes before any device work and leaves the tally and *n_bits_out as they were.  A capacity
 * of 0 is SVS_OK with *n_bits_out = 0: the device form leaves the tally untouched, the host form fills it with zeros.
 * Cost: the soft call's launch (above) with another tail - a wave adds its run's bytes with global int32 atomics that return
 * nothing, and where many of them share an entry (period below the 64 n bytes of a wave's run; under an order: period <= 64) it
 * sums them per entry first.  Measured (profiles/soft_vote_rates.txt; MI355X, 200 x 4K, n_ac = 10, delta = 20): 0.89 ms at
 * period = 10^6 against 0.80 ms of the soft call; 2.08 ms at period = 2400 and 5.37 ms there under an order - every add of the
 * launch lands in the same 9.6 KB and the atomics set the time.
 * Limits: there is no colour and no _str form, no FramePipeline or drop-in form (a receiver would have to know period before it
 * can parse the header), and no repeat option of the embed calls - the sender tiles. */
int svs_soft_vote_dev(const uint8_t *d_gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                      const svs_dither *dither, double delta, int n_ac, uint64_t period, uint64_t stream_bit0, int32_t *d_tally,
                      uint32_t flags, uint64_t *n_bits_out, void *stream);

int svs_soft_vote(const uint8_t *gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                  const svs_dither *dither, double delta, int n_ac, uint64_t period, uint64_t stream_bit0, int32_t *tally_out,
                  uint32_t flags, uint64_t *n_bits_out);

/* ---- fused per-frame soft histograms: 256 counts a frame, no soft bytes --------------------------------------
 * Two of the soft byte's three uses - how much disturbance a clip survives, which frames sit on the lattice - want a few hundred
 * numbers per frame, not a byte per capacity bit.  These calls run the soft extraction and count in the same launch: the soft
 * bytes are never written, each is counted into a row of 256 uint32 values of its frame, and the rows' 1 KB per frame are all
 * that leaves the device.  The rows are a FORMAT, as the soft byte and the tally are.  For a call on n_frames planes, with i the
 * index of a capacity bit within the call and `byte` its soft byte exactly as svs_soft_extract writes it for the same coeffs,
 * dither, delta and n_ac (and no order):
 *     f = i / (N * count)              N = (height / 8) * (width / 8), count = clamp(n_ac, 0, 63) or the selection's count
 *     hist[f * 256 + byte] += 1        for every capacity bit of the call
 * Row f sums to N * count; hist[f][v] + hist[f][v + 128] is entry v of svsdct/soft.py margin_histogram; the sum of
 * hist[f][128 .. 255] is the frame's number of hard ones.  All arithmetic is integer counting: the result does not depend on the
 * order of the additions, so the calls are deterministic though the device adds with atomics.
 * There is NO svs_block_order argument and none is needed: the dither is keyed to a block's physical position and an order
 * only permutes the blocks inside a frame, so the multiset of a frame's bytes is the same under every order - a frame embedded
 * under an order is read with this same call (its dither's first_frame as in every other call).
 *   d_hist   : n_frames * 256 uint32 values in device memory, 4-byte aligned.  The call ADDS into them, as svs_soft_vote_dev adds
 *            into d_tally: zero them before the first call.  It keeps no state and allocates nothing.  A clip read in batches
 *            passes d_hist + 256 * (frames before the batch), and first_frame advanced under a dither.
 *   hist_out : n_frames * 256 uint32 values in host memory.  The host form stages whole frames in one piece as svs_extract does
 *            (no chunk boundary falls inside a frame), counts into zeroed rows of its per-thread staging context and WRITES
 *            exactly n_frames * 256 values.
 *   coeffs, dither, planes, flags : as svs_soft_extract*, checked as there; the mode bits are accepted and change nothing.
 *   n_bits_out : receives the capacity, the number of bytes counted.
 * SVS_ERR_INVALID_ARG: embed flags or unknown ones; delta <= 0 (every soft byte is 0 there and a histogram of them says
 * nothing); a faulty coeffs, dither or planes; with a capacity above 0, a NULL gray or hist pointer, a device hist that is not
 * 4-byte aligned, or N * count above 2^32 - 1 (one call must not be able to wrap an entry: 1 x 66080 x 66080 at n_ac = 63 is
 * refused; across several calls into the same rows the caller owns the bound).  Every refusal comes before any device work and
 * leaves hist and *n_bits_out as they were.  A capacity of 0 is SVS_OK with *n_bits_out = 0: the device form leaves d_hist
 * untouched, the host form fills hist_out with zeros.
 * Cost: the soft call's launch (above) with a third tail, compiled into the instantiations without an order only.  No soft byte
 * and no per-byte global atomic leaves the CU: a workgroup counts into one table of 256 counters in LDS that only this launch
 * requests, frame by frame (the frame of a block is the division by blocks per frame that its address already takes), and
 * flushes each non-zero entry once per workgroup and frame with a global atomic that returns nothing.  Times: README.md.
 * Limits: a distance histogram, not a detector; all blocks of a frame are counted, payload or not, so a partly filled frame
 * shows a mixture; there is no colour and no _str form, no FramePipeline or drop-in form. */
int svs_soft_histogram_dev(const uint8_t *d_gray, const svs_planes *planes, const svs_coeffs *coeffs, const svs_dither *dither,
                           double delta, int n_ac, uint32_t *d_hist, uint32_t flags, uint64_t *n_bits_out, void *stream);

int svs_soft_histogram(const uint8_t *gray, const svs_planes *planes, const svs_coeffs *coeffs, const svs_dither *dither,
                       double delta, int n_ac, uint32_t *hist_out, uint32_t flags, uint64_t *n_bits_out);

/* ---- requantisation channel: what an 8x8 intra codec does to stego ------------------------------------------
 * A measuring tool, not part of the sender's or the receiver's loop: it does to gray planes what the luminance path of JPEG /
 * MJPEG - the first-order model of any intra codec on the same 8x8 grid - does to them, so that a caller who picks delta, a
 * rule, a selection, a repeat count or a vote can see what survives.  The channel is a FORMAT, as the dither, the soft byte and
 * the tally are: the host model (tests/channel_lib.py, built from the CPU oracle's pieces) and the device produce the same
 * bytes, so a table made on the CPU is the table of the GPU call.  For every 8x8 block of every frame, all arithmetic IEEE
 * float32, one operation per step, no contraction, the same order on host and device:
 *     c[k]  = the pocketfft-identical forward transform of the block's uint8 pixels (k = 8u + v, row-major, k = 0..63: the
 *             transform every exact kernel computes)
 *     c[0]  = c[0] - 1024.0f                     (JPEG's level shift of 128 per pixel, applied to DC: one subtract)
 *     q[k]  = rintf(c[k] / (float)step[k])       (float32 division, round half to even)
 *     c'[k] = q[k] * (float)step[k]              (one multiply; exact: |q * step| < 2^24)
 *     c'[0] = c'[0] + 1024.0f
 *     p     = the pocketfft-identical inverse of all 64 c' (axis 0 first, as the embed does)
 *     out   = saturate_u8(round_half_even(p))    (a decoder ROUNDS; this is NOT the embed's truncation)
 * A table of all ones is "decode, round, re-encode losslessly"; it is not the identity on stego, because the embed truncates
 * and the decoder rounds.
 * Limits: luminance only, aligned to the embed's block grid, no chroma subsampling, no motion prediction, no deblocking, no
 * entropy coding (which is lossless).  Measured ON THE CPU with the model (tests/test_requantise_cpu.py; README.md has the
 * table): three 96 x 160 frames of noise in [64, 192), one 2 400-bit payload copy per frame, delta = 20, n_ac = 10, reference
 * rule: no bit error in any copy at quality 100 .. 85; at quality 75 131 - 143 errors per copy, 137 by hard majority (the copies
 * fail at the same coefficient indices) and 51 by the soft vote.  NOT measured: a real encoder (rate control, chroma, inter
 * prediction, in-loop filters) and a grid that is not aligned.
 * Cost: one launch of the lane-per-block SVS_EXACT_POCKETFFT embed kernel - the same two transforms and 2 B/pixel of traffic -
 * behind one wave-uniform branch of the single instantiation that holds the channel; per coefficient one division, one round and
 * one multiply instead of the parity logic.
 *   steps  : a HOST pointer, read during the call and passed to the kernel by value.  NULL, or an entry of 0 or above 255:
 *            SVS_ERR_INVALID_ARG (the message names the entry).  1..255 is baseline JPEG's range; the uint16 leaves room to
 *            widen it without an ABI change.
 *   flags  : must be 0.
 *   planes : as everywhere; one geometry for input and output.  n_frames = 0: SVS_OK, nothing is done.
 *   d_in / d_out : device pointers, 8-byte aligned; d_out may be d_in (in place) or must not overlap it.  Padding between rows
 *            and frames is neither read nor written.
 * Every refusal comes before any device work and leaves the output untouched.  svs_requantise_dev enqueues and returns; it keeps
 * no state and allocates nothing.  svs_requantise takes host pointers and stages through the per-thread context in chunks as
 * svs_embed does (blocks are independent: a chunk is any band of block rows).  There is no colour, FramePipeline or drop-in form. */
typedef struct svs_steps {
    uint16_t step[64];   /* step[k] for flat row-major k = 8u + v, k = 0 is DC; each 1..255 */
} svs_steps;

/* out = the ITU-T T.81 Annex K luminance table scaled as the IJG library scales it: s = quality < 50 ? 5000 / quality :
 * 200 - 2 * quality (integer division), step = clamp((base * s + 50) / 100, 1, 255).  quality 50 is the Annex K table, 100 all
 * ones.  quality outside 1..100: SVS_ERR_INVALID_ARG.  Host only: needs no GPU. */
int svs_quality_steps(svs_steps *out, int quality);

int svs_requantise_dev(const uint8_t *d_in, uint8_t *d_out, const svs_planes *planes, const svs_steps *steps, uint32_t flags,
                       void *stream);

int svs_requantise(const uint8_t *in, uint8_t *out, const svs_planes *planes, const svs_steps *steps, uint32_t flags);

/* ---- per-coefficient QIM steps: lattices matched to a codec's table ---------------------------------------------
 * Every other embed call quantises all payload coefficients with one delta; an 8x8 intra codec quantises coefficient k with
 * its own step s_k.  With delta_k = m * s_k a lattice point q * delta_k is a multiple of s_k and passes the requantiser
 * (svs_requantise*: rintf(c / s_k) * s_k) unchanged, so the step is large only where the codec's is.  Opt-in; both sides must
 * hold the same table.  A FORMAT, as the dither and the channel are: for a payload coefficient c at flat row-major index k
 * with bit b, dk = (float)delta[k], every step one IEEE float32 operation with no contraction, in the same order on host and
 * device:
 *     q = (int)rintf(c / dk)                     (float32 division, round half to even)
 *     the value written for index t is (float)t * dk                (exact: |t * dk| < 2^24)
 *     reference rule: t = q with its parity forced to b (as svs_embed);  SVS_NEAREST: the nearer lattice point of parity b, the
 *     side taken from c against c0 = (float)q * dk, the reference's choice when c == c0;  SVS_MINMOVE: c clamped into
 *     [ct - r_k, ct + r_k] around SVS_NEAREST's point ct, h_k = 0.5f * dk, r_k = fmaxf(0, h_k - MARGIN[k])
 *     under a dither: d = r * dk with the dithered calls' hash and r, the rule on c - d, the result moved back by d, and a
 *     coefficient the rule leaves alone keeps c exactly
 *     the receiver reads rintf((c - d) / dk) & 1   (d = 0 without a dither)
 * Everything else is the reference's: stream ranges, the block budget and the block it ends in, byte-identical blocks past the
 * budget, the copy of an empty payload, the round trip of every block when nothing can be embedded but n_bits > 0, the
 * pocketfft-identical inverse of all 64 coefficients, clip, truncate.  There is no delta <= 0 route: an entry is at least 1.
 * A uniform table (every delta[k] = D) gives, byte for byte and bit for bit, the output of the existing call with delta = D and
 * the same order, selection, dither and rule; the stepped side of the kernels runs all the same.
 *   steps  : required, a HOST pointer read during the call and passed to the kernels by value.  NULL, or an entry k >= 1 that is
 *            0 or above 4095: SVS_ERR_INVALID_ARG naming the entry, before the other options are checked and before any device
 *            work.  delta[0] (DC) is not read.
 *   order, coeffs, dither : each may be NULL; checked as in the dithered calls (dither, then coeffs, then flags).  With coeffs,
 *            n_ac is ignored.
 *   flags  : embed - the mode bits (accepted; a stepped call runs the lane-per-block exact kernels in every mode), SVS_NEAREST
 *            and SVS_MINMOVE; extract - the mode bits only.  SVS_READBACK, SVS_KEEP_COLOUR and anything else: refused.
 * The host forms go through the per-thread staging context: whole frames under an order or a dither, chunks otherwise.
 * Limits: both sides must hold the table; a matched table is tuned to ONE codec table on the aligned luminance grid (README.md
 * has the survival table, from the CPU model; a table matched to a fine codec table needs a floor, see svs_matched_steps); a
 * real encoder is not measured.  A stepped call has no colour or _str form; its soft, vote and histogram forms are
 * svs_stepped_soft_* below, its read-back form is svs_stepped_embed_readback* further below. */
typedef struct svs_qim_steps {
    uint16_t delta[64];   /* delta[k]: the step of flat row-major coefficient k = 8u + v; k = 1..63 each 1..4095; delta[0] (DC) is not read */
} svs_qim_steps;

/* out->delta[k] = codec->step[k] * max(multiple, ceil(floor / codec->step[k])) for k = 1..63, delta[0] = 0.  multiple 1..16,
 * floor 0..4095.  The floor keeps a step above the embed's own truncation disturbance (up to 4.0 per coefficient): the low
 * frequencies of the quality-95 table have steps of 1 - 2, and twice that table does not survive its own channel; with
 * floor = 16 it does.  SVS_ERR_INVALID_ARG for a
 * NULL pointer, a codec entry outside 1..255 or a result above 4095 (the message names the entry); *out is then left as
 * it was.  Host only: needs no GPU. */
int svs_matched_steps(svs_qim_steps *out, const svs_steps *codec, int multiple, int floor);

int svs_stepped_embed_dev(const uint8_t *d_gray, uint8_t *d_stego, const svs_planes *planes, const svs_block_order *order,
                          const svs_coeffs *coeffs, const svs_dither *dither, const svs_qim_steps *steps, int n_ac,
                          const uint8_t *d_bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t flags,
                          uint64_t *n_embedded, void *stream);

int svs_stepped_embed(const uint8_t *gray, uint8_t *stego, const svs_planes *planes, const svs_block_order *order,
                      const svs_coeffs *coeffs, const svs_dither *dither, const svs_qim_steps *steps, int n_ac,
                      const uint8_t *bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t flags, uint64_t *n_embedded);

int svs_stepped_extract_dev(const uint8_t *d_gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                            const svs_dither *dither, const svs_qim_steps *steps, int n_ac, uint8_t *d_bits_packed_out,
                            uint64_t out_capacity_bytes, uint32_t flags, uint64_t *n_bits_out, void *stream);

int svs_stepped_extract(const uint8_t *gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                        const svs_dither *dither, const svs_qim_steps *steps, int n_ac, uint8_t *bits_packed_out,
                        uint64_t out_capacity_bytes, uint32_t flags, uint64_t *n_bits_out);

/* ---- soft bytes, the fused vote and the fused histograms under per-coefficient steps -------------------------------
 * svs_soft_extract*, svs_soft_vote* and svs_soft_histogram* with a svs_qim_steps table in the place of delta, as
 * svs_stepped_extract* is to svs_extract_dithered*; the argument order is svs_stepped_extract*'s.  The layout is that of the
 * existing soft call with the same order, coeffs, dither and n_ac: one byte per capacity bit in stream order, byte i belonging to
 * stream bit i of svs_stepped_extract*; the tally and the histogram rows are exactly the formats stated above, fed with these
 * bytes.  The byte is a FORMAT.  For the payload coefficient at flat row-major index k, dk = (float)steps->delta[k], c the
 * pocketfft-identical forward coefficient, d = r * dk the stepped calls' dither (0 without one), every step one IEEE float32
 * operation with no contraction, in the same order on host and device:
 *     x    = c - d
 *     q    = (int)rintf(x / dk)          (the stepped extract's own index: float32 division, round half to even)
 *     x0   = (float)q * dk
 *     a    = fabsf(x - x0)
 *     h_k  = 0.5f * dk
 *     s_k  = 254.0f / dk                 (one float32 division; equal to (float)(254.0 / (double)dk) for every dk in 1..4095)
 *     m    = clamp((int)((h_k - a) * s_k), 0, 127)        (truncation toward zero)
 *     byte = ((q & 1) << 7) | m
 * On a lattice point (a = 0) m is (int)(h_k * s_k): 127, or 126 for the steps whose float32 product falls just below 127, as
 * in svs_soft_extract* at such a delta.
 * So m is the distance from the nearest decision boundary in units of delta[k] / 254, the coefficient's OWN cell: under a vote
 * a copy weighs by how deep it sits in its cell, whatever the size of that cell.  A uniform table (every delta[k] = D) gives,
 * byte for byte, tally entry for tally entry and count for count, the output of svs_soft_extract* / svs_soft_vote* /
 * svs_soft_histogram* at delta = D with the same options; the stepped side of the kernels runs all the same.
 *   steps  : as svs_stepped_extract*: checked first, before the other options and before any device work; NULL, or an entry
 *            k >= 1 that is 0 or above 4095, is SVS_ERR_INVALID_ARG naming the entry.  There is no delta <= 0 route.
 *   order, coeffs, dither : each may be NULL; checked next (dither, then coeffs, then flags) as in svs_stepped_extract*.  The
 *            histogram calls take no order, as svs_soft_histogram*.
 *   flags  : the mode bits are accepted and change nothing; embed flags and unknown bits are refused.
 *   every other argument, and every other check in its order (planes, a NULL or unaligned pointer, the capacity of d_soft_out,
 *            period 0 or above 2^61 - 1, capacity above period * 2^22, N * count above 2^32 - 1): as the soft call of the same
 *            name.  A capacity of 0 behaves as there: the soft call writes nothing, a device tally or hist is left untouched, a
 *            host tally or hist is filled with zeros, *n_bits_out = 0.  A refusal leaves the outputs and *n_bits_out as they were
 *            where the existing call does.
 * Cost: the soft launch of the two eight-row power-of-two-delta extract instantiations, which hold the stepped side, with this
 * byte in the place of theirs - per coefficient one more float32 division than the stepped extract; the three tails (copy, vote,
 * histogram), the tiles in LDS, the atomics and the flush rules are the existing ones.  Times: README.md.
 * Limits: as the stepped calls and the soft calls; a vote that weighs a copy by its ABSOLUTE distance (in coefficient units,
 * not in units of its own cell) was not evaluated; the survival figures (README.md) come from the CPU model of the channel, not
 * from a real encoder; there is no colour and no _str form, no FramePipeline or drop-in form. */
int svs_stepped_soft_extract_dev(const uint8_t *d_gray, const svs_planes *planes, const svs_block_order *order,
                                 const svs_coeffs *coeffs, const svs_dither *dither, const svs_qim_steps *steps, int n_ac,
                                 uint8_t *d_soft_out, uint64_t out_capacity_bytes, uint32_t flags, uint64_t *n_bits_out, void *stream);

int svs_stepped_soft_extract(const uint8_t *gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                             const svs_dither *dither, const svs_qim_steps *steps, int n_ac, uint8_t *soft_out,
                             uint64_t out_capacity_bytes, uint32_t flags, uint64_t *n_bits_out);

int svs_stepped_soft_vote_dev(const uint8_t *d_gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                              const svs_dither *dither, const svs_qim_steps *steps, int n_ac, uint64_t period, uint64_t stream_bit0,
                              int32_t *d_tally, uint32_t flags, uint64_t *n_bits_out, void *stream);

int svs_stepped_soft_vote(const uint8_t *gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                          const svs_dither *dither, const svs_qim_steps *steps, int n_ac, uint64_t period, uint64_t stream_bit0,
                          int32_t *tally_out, uint32_t flags, uint64_t *n_bits_out);

int svs_stepped_soft_histogram_dev(const uint8_t *d_gray, const svs_planes *planes, const svs_coeffs *coeffs, const svs_dither *dither,
                                   const svs_qim_steps *steps, int n_ac, uint32_t *d_hist, uint32_t flags, uint64_t *n_bits_out,
                                   void *stream);

int svs_stepped_soft_histogram(const uint8_t *gray, const svs_planes *planes, const svs_coeffs *coeffs, const svs_dither *dither,
                               const svs_qim_steps *steps, int n_ac, uint32_t *hist_out, uint32_t flags, uint64_t *n_bits_out);

/* ---- matrix embedding: k bits a block for one or two parity flips ---------------------------------------------------
 * Every other embed call writes one payload bit into the parity of one coefficient, and about half of them must be pushed into
 * the neighbouring cell.  Matrix embedding (the (2^k - 1, k) Hamming syndrome code of F5, and its "modified" form) lets a block
 * of n = 2^k - 1 payload coefficients carry k message bits as the syndrome of their n parities: the sender reaches any message
 * by flipping AT MOST ONE parity (search 0), or the cheaper of one flip and a pair of flips (search 1).  The receiver needs no
 * side information.  Opt-in, and it pays off under SVS_MINMOVE alone, where a coefficient whose parity is right mostly stays
 * where it is (README.md has the table); under the other rules every selected coefficient is pulled to a lattice point, so more
 * carriers cost more.  These are STEPPED calls: a caller with one delta passes a uniform table.  A FORMAT, step by step:
 *   selection : `coeffs` when given, else the row-major prefix 1..n_ac.  It must have exactly n = 2^k - 1 entries.  Slot t in
 *               0..n-1 of a block is entry t of the selection, as in the select calls.
 *   stream    : a block carries k bits.  Block j of the call's stream order (raster, or keyed with an order) owns stream bits
 *               [j k, j k + k); the capacity is blocks * k (svs_matrix_capacity_bits).  The block's budget is
 *               nb = clamp(n_bits - j k, 0, k); nb = 0: the block's bytes are the cover's.  Its message value is
 *               m = sum over i < nb of bit_i * 2^i; bits past the budget count as 0.
 *   parities  : p_t = rintf(x_t / delta_k) & 1 with x_t = c_t - d_t, exactly svs_stepped_extract*'s verdict (d = 0 without a
 *               dither); the syndrome S = XOR over the slots t with p_t = 1 of (t + 1).
 *   extract   : bit i of the block is (S >> i) & 1, all k bits of every block; the output is the packed stream of blocks * k
 *               bits and *n_bits_out the capacity.
 *   embed     : j = S ^ m; the flip set F is a set of slots.  j = 0: F is empty.  search 0: F = {j - 1}.  search 1: with
 *               stay_t = rule(x_t, p_t) and flip_t = rule(x_t, p_t ^ 1), the rule being the stepped calls' for the call's flags, in
 *               float32 with one IEEE operation a step  a = flip_t - x_t;  b = stay_t - x_t;  e_t = a * a - b * b;  start with
 *               best = e_{j-1}, F = {j - 1}; for a = 1, 2, .., n in this order with b = a ^ j and a < b: v = e_{a-1} + e_{b-1};
 *               if v < best (strictly) then best = v and F = {a - 1, b - 1}.
 *               Then EVERY one of the n selected coefficients is written by the stepped rule with the bit p_t ^ [t in F] -
 *               reference, SVS_NEAREST or SVS_MINMOVE as the flags say, with the band, the dither and "a coefficient the rule
 *               leaves alone keeps c exactly" as in the stepped calls.  The inverse, clip and truncate are the reference's.
 *               *n_embedded = min(n_bits, capacity).
 * Order, dither and first-frame rules are svs_stepped_embed*'s.  With k = 1 the embed gives, byte for byte,
 * svs_stepped_embed* with the same one-coefficient selection, table, order, dither and rule, and the extract gives
 * svs_stepped_extract*'s bits, for both search values; a k = 1 call runs the matrix side of the kernels all the same.
 * Refused with SVS_ERR_INVALID_ARG before any device work: a NULL matrix or steps; k outside 1..6; search > 1; reserved != 0;
 * search 1 with k = 6 (the embed keeps n floats per lane in a wave-private LDS tile and the pair search n more: 126 of them for
 * 256 lanes exceed the 64 KB a launch may request); a selection or n_ac of a size other than 2^k - 1; SVS_READBACK, SVS_KEEP_COLOUR and every flag
 * the stepped calls refuse; SVS_NEAREST or SVS_MINMOVE on extract.  The host forms stage whole frames, as the keyed calls do.
 * Limits: a message bit depends on about n / 2 parities, so one disturbed coefficient corrupts up to k bits of its block: a
 * quality option for channels the lattice survives.  Clipping blocks are not repaired (no read-back form), so SVS_MINMOVE's
 * guarantee that a stego frame decodes excludes them.  No soft, vote, histogram, read-back, margin, colour or _str form. */
typedef struct svs_matrix {
    uint32_t k;             /* message bits a block, 1..6; the selection has 2^k - 1 coefficients */
    uint32_t search;        /* 0: the syndrome's single flip;  1: the cheapest of a single flip or a pair (k <= 5) */
    uint32_t reserved[2];   /* must be 0 */
} svs_matrix;

/* blocks * k; 0 for a NULL pointer, a k outside 1..6 or planes svs_capacity_bits gives 0 for */
uint64_t svs_matrix_capacity_bits(const svs_planes *p, const svs_matrix *m);

int svs_matrix_embed_dev(const uint8_t *d_gray, uint8_t *d_stego, const svs_planes *planes, const svs_block_order *order,
                         const svs_coeffs *coeffs, const svs_dither *dither, const svs_qim_steps *steps, const svs_matrix *matrix,
                         int n_ac, const uint8_t *d_bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t flags,
                         uint64_t *n_embedded, void *stream);

int svs_matrix_embed(const uint8_t *gray, uint8_t *stego, const svs_planes *planes, const svs_block_order *order,
                     const svs_coeffs *coeffs, const svs_dither *dither, const svs_qim_steps *steps, const svs_matrix *matrix, int n_ac,
                     const uint8_t *bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t flags, uint64_t *n_embedded);

int svs_matrix_extract_dev(const uint8_t *d_gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                           const svs_dither *dither, const svs_qim_steps *steps, const svs_matrix *matrix, int n_ac,
                           uint8_t *d_bits_packed_out, uint64_t out_capacity_bytes, uint32_t flags, uint64_t *n_bits_out, void *stream);

int svs_matrix_extract(const uint8_t *gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                       const svs_dither *dither, const svs_qim_steps *steps, const svs_matrix *matrix, int n_ac,
                       uint8_t *bits_packed_out, uint64_t out_capacity_bytes, uint32_t flags, uint64_t *n_bits_out);

/* ---- the operator with read-back and repair (SVS_READBACK) ---------------------------------------------
 * svs_embed_ordered_dev / svs_embed_ordered with SVS_READBACK implied (order may be NULL), plus the counts of the read-back:
 *   d_counts : NULL, or a device buffer of two uint64 (8-byte aligned) that the call ADDS {blocks repaired, blocks left
 *              unrepaired} into, on the call's stream.
 *   counts   : NULL, or receives the counts of the whole call when it returns (every staging chunk included). */
typedef struct svs_readback_counts {
    uint64_t repaired;     /* blocks that did not read back and were repaired */
    uint64_t unrepaired;   /* blocks that did not read back and kept the reference's bytes */
} svs_readback_counts;

int svs_embed_readback_dev(const uint8_t *d_gray, uint8_t *d_stego, const svs_planes *planes, const svs_block_order *order,
                           double delta, int n_ac, const uint8_t *d_bits_packed, uint64_t bit_offset, uint64_t n_bits,
                           uint32_t flags, uint64_t *n_embedded, uint64_t *d_counts, void *stream);

int svs_embed_readback(const uint8_t *gray, uint8_t *stego, const svs_planes *planes, const svs_block_order *order, double delta,
                       int n_ac, const uint8_t *bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t flags,
                       uint64_t *n_embedded, svs_readback_counts *counts);

/* Read-back and repair under a coefficient selection and a keyed dither: svs_embed_dithered_dev / svs_embed_dithered followed,
 * on the call's stream, by a read-back pass that checks every payload block with svs_extract_select* / svs_extract_dithered*'s
 * own verdict - for every selected coefficient k whose slot lies inside the block's budget, the parity of quant_index(c_k)
 * (with a dither: of quant_index(c_k - d_k), d that of the block's physical position) against the payload bit of its slot,
 * c the pocketfft-identical forward transform - and repairs a failing block with SVS_READBACK's bounded search
 * (csrc/svs_readback.hpp, the keyed forms): the targets are the nearest lattice points of the wanted parity of the SHIFTED
 * lattice, q' delta + d_k, everything else is the same, at most 16 iterates, accepted only when that check confirms every bit.
 *   order, coeffs, dither : each may be NULL.  A NULL dither is the selected call with read-back; with all three NULL, or with
 *            a prefix selection alone, the call IS svs_embed_readback*: its kernels, its bytes and its counts.  What is given
 *            is checked as in the dithered calls (svs_coeffs, reserved, the two first_frame values).
 *   flags  : the mode bits are accepted and change nothing; SVS_NEAREST and SVS_MINMOVE; SVS_READBACK is accepted and implied;
 *            anything else: SVS_ERR_INVALID_ARG before any device work.
 *   d_counts / counts : as in svs_embed_readback*.
 * Contract: the call first writes exactly the stego of the same call without read-back (in place allowed); a block that reads
 * back keeps its bytes; an unrepaired block keeps them too and is counted; blocks past the budget are untouched.  The host
 * form stages whole frames under an order or a dither and sums the counts over its chunks.  The limits are SVS_READBACK's: a
 * block that clips at both ends can stay unrepaired, and at small delta (4) an accepted iterate can be far from the stego.
 * Cost on a GPU: not measured yet (tools/keyed_readback_rates.py writes profiles/keyed_readback_rates.txt). */
int svs_embed_dithered_readback_dev(const uint8_t *d_gray, uint8_t *d_stego, const svs_planes *planes,
                                    const svs_block_order *order, const svs_coeffs *coeffs, const svs_dither *dither,
                                    double delta, int n_ac, const uint8_t *d_bits_packed, uint64_t bit_offset, uint64_t n_bits,
                                    uint32_t flags, uint64_t *n_embedded, uint64_t *d_counts, void *stream);

int svs_embed_dithered_readback(const uint8_t *gray, uint8_t *stego, const svs_planes *planes, const svs_block_order *order,
                                const svs_coeffs *coeffs, const svs_dither *dither, double delta, int n_ac,
                                const uint8_t *bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t flags,
                                uint64_t *n_embedded, svs_readback_counts *counts);

/* Read-back and repair under per-coefficient steps: svs_stepped_embed_dev / svs_stepped_embed followed, on the call's stream, by
 * the read-back pass with coefficient k's own step in the place of delta.  A FORMAT, as the stepped and keyed formats are: it is
 * svs_embed_dithered_readback* with delta_k for delta.  For a payload coefficient c at flat row-major index k whose slot lies
 * inside the block's budget, c the pocketfft-identical forward transform of the stego block, every float step one IEEE float32
 * operation with no contraction, in the same order on host and device:
 *     dk = (float)steps->delta[k]
 *     d  = dither_value(s_b, k, dk): the stepped calls' d = r * dk of the block's physical position; without a dither no
 *          operation on d is executed
 *     check   (int)rintf((c - d) / dk) & 1 against the payload bit of the slot: svs_stepped_extract*'s own verdict
 *     target  cp = c - d
 *             q  = (int)rintf(cp / dk)
 *             where the parity is wrong:  q = cp * (1.0f / dk) >= (float)q ? q + 1 : q - 1      (the neighbour on cp's side)
 *             T  = (float)q * dk + d
 * Everything else is SVS_READBACK's, unchanged: the over-relaxed correction (T - c) * (1 + it / 2), the inverse, the shift off
 * 0 / 255, round-half-even and clip, at most 16 iterates, accepted only when the check confirms every bit.  The side test takes
 * the reciprocal so that a uniform table (every delta[k] = D) gives, byte for byte and count for count, the output of
 * svs_embed_dithered_readback* at delta = D with the same order, selection, dither and rule (1.0f / D is that call's own
 * reciprocal) - and so, without a selection and a dither, svs_embed_readback*'s; the stepped body of the kernel runs all the
 * same: a uniform table is not rerouted.
 *   steps  : as svs_stepped_embed*: checked first, before the other options and before any device work.
 *   order, coeffs, dither : each may be NULL; checked next (dither, then coeffs, then flags) as in svs_stepped_embed*.
 *   flags  : the mode bits are accepted and change nothing; SVS_NEAREST and SVS_MINMOVE; SVS_READBACK is accepted and implied;
 *            anything else: SVS_ERR_INVALID_ARG before any device work.  (svs_stepped_embed* itself keeps refusing SVS_READBACK.)
 *   d_counts / counts : as in svs_embed_readback*: d_counts is added to.
 * Contract: the call first writes exactly the stego of svs_stepped_embed* with the same arguments (in place allowed), then runs
 * the pass on the same stream; a block that reads back keeps its bytes; an unrepaired block keeps them too and is counted;
 * blocks past the budget are untouched.  The host form stages whole frames under an order or a dither, chunks otherwise, and
 * sums the counts over its chunks.
 * Limits: SVS_READBACK's - a block that clips at both ends can stay unrepaired - and the stepped calls'.  A repaired block is
 * accepted because it decodes, not because it lies on a lattice point: through a requantising channel it may survive worse than
 * an untouched block (README.md has the measured table; svs_stepped_embed_readback_margin* below adds the acceptance margin on
 * the soft byte).  There is no
 * colour and no _str form.  Cost: the stepped embed plus one launch of the read-back kernel's keyed instantiation, about 1.01 -
 * 1.06 x svs_embed_dithered_readback_dev at the same settings (README.md, profiles/stepped_readback_rates.txt). */
int svs_stepped_embed_readback_dev(const uint8_t *d_gray, uint8_t *d_stego, const svs_planes *planes, const svs_block_order *order,
                                   const svs_coeffs *coeffs, const svs_dither *dither, const svs_qim_steps *steps, int n_ac,
                                   const uint8_t *d_bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t flags,
                                   uint64_t *n_embedded, uint64_t *d_counts, void *stream);

int svs_stepped_embed_readback(const uint8_t *gray, uint8_t *stego, const svs_planes *planes, const svs_block_order *order,
                               const svs_coeffs *coeffs, const svs_dither *dither, const svs_qim_steps *steps, int n_ac,
                               const uint8_t *bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t flags,
                               uint64_t *n_embedded, svs_readback_counts *counts);

/* The soft-margin pass behind the stepped read-back (opt-in): svs_stepped_embed_readback* asks that every block decodes; these
 * calls ask in addition that every payload coefficient reaches the receiver with a soft margin of at least min_margin - the low
 * seven bits m of the byte svs_stepped_soft_extract* gives, the distance from the decision boundary in units of delta_k / 254.  A
 * FORMAT, step by step:
 *   1. Pass 1 is svs_stepped_embed_readback* with the same arguments: the same launches, the same bytes, the same `repaired` and
 *      `unrepaired`.  With min_margin = 0 the call ends here and strengthened = weak = 0.
 *   2. Pass 2 runs on the same stream and looks at every payload block again, on its bytes after pass 1.  For each payload
 *      coefficient, with the check's own values - c the pocketfft-identical forward coefficient, dk and d as above -, each step
 *      one IEEE float32 operation with no contraction, in this order (stepped_soft_byte's arithmetic):
 *          x = c - d                            (without a dither: x = c)
 *          q = (int)rintf(x / dk)
 *          v = (0.5f * dk - fabsf(x - (float)q * dk)) * (254.0f / dk)
 *      The coefficient is STRONG when q's parity is the payload bit and v >= (float)min_margin; for min_margin in 1..127 that is
 *      exactly "the receiver's soft byte has the right bit 7 and m >= min_margin".
 *        - a block with a wrong bit is skipped: it is pass 1's `unrepaired`;
 *        - a block that is strong throughout is untouched;
 *        - a block that decodes but has a weak coefficient is searched with the stepped read-back's own targets, correction,
 *          inverse, shift, rounding and sixteen iterates; only the acceptance differs: the first iterate whose payload
 *          coefficients are all strong is stored and counted `strengthened`.  A block that none of the sixteen makes strong
 *          keeps its bytes - pass 1's, which decode - and is counted `weak`.
 *   3. No fallback block is kept: a failed search stores nothing.  That is why the pass is a second launch and not fused.
 *   min_margin : 0..127; more is SVS_ERR_INVALID_ARG, checked behind `steps` and ahead of everything else.  Every other argument
 *                is checked as in svs_stepped_embed_readback*.
 *   d_counts   : NULL, or four uint64 on the device, 8-byte aligned, added to: svs_margin_counts.  The host form zeroes *counts
 *                and sums over its staging chunks.
 * A caller with one delta passes a uniform table.  There is no delta form, no colour form and no _str form.
 * Limits: the margin is the luminance model's (svsdct/channel.py: requantisation of the 8x8 luminance DCT, no real encoder);
 * `weak` blocks remain and are counted - blocks that clip at both ends, and at small delta_k any gate near 127, which is
 * unreachable there because the stored block's own rounding to uint8 moves a coefficient by up to about 2; a uniform table on
 * row-major coefficients gains nothing at the quality where its lattice, not its margin, fails.  Measured (README.md, the CPU
 * model on three 96 x 160 frames, 2 400 bits a frame, 10 coefficients, min_margin = 64, bit errors after requantisation at
 * Q = 75 with the read-back alone / with the pass):
 *     matched(75, 2), row-major 1..10, noise over 0..255 (clips)   143 / 16    108 of 720 blocks strengthened, 0 weak, -0.12 dB
 *     matched(75, 2), zig-zag 1..10, letterboxed                    18 /  0      9 strengthened, 0 weak, -0.04 dB
 *     matched(75, 2), row-major 1..10, letterboxed                  24 /  0      9 strengthened, 0 weak, -0.01 dB
 *     uniform 20, row-major 1..10, noise                           431 / 430     4 strengthened, 0 weak, -0.01 dB
 * Cost: one more launch of the read-back kernel's hosting instantiation: at g = 64 on 200 x 4K about 2.0 - 2.4 ms on top of
 * svs_stepped_embed_readback_dev's 2.9 - 4.0 ms, 1.6 - 1.7 x that call; at g = 0 that call's cost (README.md,
 * profiles/readback_margin_rates.txt). */
typedef struct svs_margin_counts {
    uint64_t repaired, unrepaired;   /* pass 1: svs_readback_counts */
    uint64_t strengthened, weak;     /* pass 2 */
} svs_margin_counts;

int svs_stepped_embed_readback_margin_dev(const uint8_t *d_gray, uint8_t *d_stego, const svs_planes *planes,
                                          const svs_block_order *order, const svs_coeffs *coeffs, const svs_dither *dither,
                                          const svs_qim_steps *steps, int n_ac, const uint8_t *d_bits_packed, uint64_t bit_offset,
                                          uint64_t n_bits, uint32_t min_margin, uint32_t flags, uint64_t *n_embedded,
                                          uint64_t *d_counts, void *stream);

int svs_stepped_embed_readback_margin(const uint8_t *gray, uint8_t *stego, const svs_planes *planes, const svs_block_order *order,
                                      const svs_coeffs *coeffs, const svs_dither *dither, const svs_qim_steps *steps, int n_ac,
                                      const uint8_t *bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t min_margin,
                                      uint32_t flags, uint64_t *n_embedded, svs_margin_counts *counts);

/* ---- colour plumbing around the operator (device resident) --------------------------------------------
 * Interleaved 8-bit BGR frames [frame][row][col][3] <-> gray planes.  bgr_row_pitch / bgr_frame_pitch in bytes,
 * multiples of 8 (3*width always is); BGR base pointers 8-byte aligned, as for the fused calls below.
 * svs_bgr_to_gray_dev replaces cv2.cvtColor(frame, COLOR_BGR2GRAY) (config_and_setup.py:112): OpenCV's fixed-point
 * (B*wb + G*wg + R*wr + 2^(shift-1)) >> shift.  weights = {wb, wg, wr, shift}; NULL = {3735, 19235, 9798, 15}
 * (OpenCV 4's 15-bit table; older builds use {1868, 9617, 4899, 14}); wb + wg + wr must equal 2^shift exactly.
 * Parity with cv2 is UNPINNED (cv2 is not available in the build image) - a caller that has cv2 should compare once
 * at start-up.
 * svs_gray_to_bgr_dev replaces cv2.cvtColor(stego, COLOR_GRAY2BGR) (embed_process.py:126): B = G = R = gray. */
int svs_bgr_to_gray_dev(const uint8_t *d_bgr, int64_t bgr_row_pitch, int64_t bgr_frame_pitch, uint8_t *d_gray,
                        const svs_planes *planes, const uint32_t *weights, void *stream);
int svs_gray_to_bgr_dev(const uint8_t *d_gray, const svs_planes *planes, uint8_t *d_bgr, int64_t bgr_row_pitch,
                        int64_t bgr_frame_pitch, void *stream);

/* Fused colour path: BGR frames in, stego BGR frames out, one pass (3 B/pixel read + 3 B/pixel written; the frame
 * loop's cvtColor -> operator -> cvtColor at embed_process.py:117-127 for the frames that carry payload).
 *   d_bgr_in / d_bgr_out : interleaved 8-bit BGR [frame][row][col][3]; pitches in bytes (multiples of 8; base
 *                          pointers 8-byte aligned); may alias when the pitches are equal.
 *   d_gray_ref           : optional (NULL to skip) gray planes, geometry `planes`: the gray frame BEFORE embedding,
 *                          i.e. the operator's first return value (config_and_setup.py:112,172).
 *   planes               : n_frames / height / width of the clip and the pitches of d_gray_ref.
 *   weights, flags, bits : as svs_bgr_to_gray_dev / svs_embed_dev, plus SVS_KEEP_COLOUR.  Every block of these frames
 *                          is written (gray replicated into B, G, R; with SVS_KEEP_COLOUR the cover's colours shifted to
 *                          the stego gray); pass only the frames that carry payload - the reference copies the remaining
 *                          frames in colour (embed_process.py:134-139).  d_gray_ref is the cover gray in both forms. */
int svs_embed_bgr_dev(const uint8_t *d_bgr_in, int64_t in_row_pitch, int64_t in_frame_pitch,
                      uint8_t *d_bgr_out, int64_t out_row_pitch, int64_t out_frame_pitch,
                      uint8_t *d_gray_ref, const svs_planes *planes, const uint32_t *weights,
                      double delta, int n_ac, const uint8_t *d_bits_packed, uint64_t bit_offset, uint64_t n_bits,
                      uint32_t flags, uint64_t *n_embedded, void *stream);
/* Extract straight from interleaved BGR frames (gray computed on the fly, pocketfft-identical forward transform:
 * the bits equal svs_extract_dev(..., SVS_EXACT_POCKETFFT) of svs_bgr_to_gray_dev's output). */
int svs_extract_bgr_dev(const uint8_t *d_bgr, int64_t bgr_row_pitch, int64_t bgr_frame_pitch,
                        const svs_planes *planes, const uint32_t *weights, double delta, int n_ac,
                        uint8_t *d_bits_packed_out, uint64_t out_capacity_bytes, uint64_t *n_bits_out, void *stream);

/* Host-pointer forms of the two calls above for tightly packed frames (BGR row pitch 3*width, gray row pitch width):
 * frames and payload are staged through device memory inside the call, which returns when the results are in the
 * caller's buffers.  bgr_out / gray_ref_out: [n_frames][height][width][3] resp. [n_frames][height][width];
 * gray_ref_out may be NULL.  `planes` must describe tightly packed gray planes (pitches width and height*width). */
int svs_embed_bgr(const uint8_t *bgr, uint8_t *bgr_out, uint8_t *gray_ref_out, const svs_planes *planes,
                  const uint32_t *weights, double delta, int n_ac, const uint8_t *bits_packed, uint64_t bit_offset,
                  uint64_t n_bits, uint32_t flags, uint64_t *n_embedded);
int svs_extract_bgr(const uint8_t *bgr, const svs_planes *planes, const uint32_t *weights, double delta, int n_ac,
                    uint8_t *bits_packed_out, uint64_t out_capacity_bytes, uint64_t *n_bits_out);

/* The fused colour embed with read-back and repair: svs_embed_bgr_dev / svs_embed_bgr followed, on the call's stream, by the
 * read-back pass in place on the BGR output (SVS_READBACK accepted and implied; flags: the mode bits and SVS_KEEP_COLOUR;
 * no keyed block order).  d_counts / counts as in svs_embed_readback*.  With gray() the call's fixed-point gray (weights),
 * G = gray(cover) and R = the stego planes and counts svs_embed_readback (order NULL) gives for G with the same delta,
 * n_ac, payload, bit_offset and mode bits:
 *   plain            the output is B = G = R = R's stego, byte for byte: gray_to_bgr(svs_embed_readback(bgr_to_gray(cover))).
 *   SVS_KEEP_COLOUR  a block that reads back keeps the bytes svs_embed_bgr_dev(..., SVS_KEEP_COLOUR) writes.  In a repaired
 *                    block every pixel is the keep-colour pixel (csrc/svs_colour.hpp) of P and t', P = the pixel the
 *                    keep-colour embed wrote (the pass works in place on the output: d_bgr_in == d_bgr_out is allowed),
 *                    t' = the repaired gray.  So gray(output) == R's stego exactly, a pixel whose gray the repair did not
 *                    change keeps its bytes, and an unrepaired block keeps its bytes.
 * The counts equal R's.  d_gray_ref / gray_ref_out stay the cover gray.  Blocks past the payload budget are not touched by
 * the pass; on content without failures the output is byte-identical to svs_embed_bgr_dev / svs_embed_bgr. */
int svs_embed_bgr_readback_dev(const uint8_t *d_bgr_in, int64_t in_row_pitch, int64_t in_frame_pitch,
                               uint8_t *d_bgr_out, int64_t out_row_pitch, int64_t out_frame_pitch,
                               uint8_t *d_gray_ref, const svs_planes *planes, const uint32_t *weights,
                               double delta, int n_ac, const uint8_t *d_bits_packed, uint64_t bit_offset, uint64_t n_bits,
                               uint32_t flags, uint64_t *n_embedded, uint64_t *d_counts, void *stream);
int svs_embed_bgr_readback(const uint8_t *bgr, uint8_t *bgr_out, uint8_t *gray_ref_out, const svs_planes *planes,
                           const uint32_t *weights, double delta, int n_ac, const uint8_t *bits_packed, uint64_t bit_offset,
                           uint64_t n_bits, uint32_t flags, uint64_t *n_embedded, svs_readback_counts *counts);

/* ---- measurement helpers (synthetic inputs and on-device checks for bench.py / tests) ------ */
/* value = lo + hash32(seed, first_frame + f, y, x) % span  - same hash as svsdct/synth.py; 1 <= span, lo + span <= 256 */
int svs_fill_synthetic_dev(uint8_t *d_frames, const svs_planes *planes, uint32_t seed,
                           uint32_t first_frame, uint32_t lo, uint32_t span, void *stream);
/* packed Bernoulli(1/2) stream, bit i = lowbias32(seed*0x632BE5AB + first_bit + i) >> 31;
 * writes ceil(n_bits/8) bytes rounded up to a multiple of 4 (buffer must be that large). */
int svs_fill_bits_dev(uint8_t *d_bits_packed, uint64_t n_bits, uint32_t seed,
                      uint64_t first_bit, void *stream);
/* per-frame sum of squared differences (exact integers) -> d_sse[n_frames] (uint64, device);
 * PSNR = 10 log10(255^2 H W / sse)   (cv2.PSNR as used at embed_process.py:205, app.py:342) */
int svs_frame_sse_dev(const uint8_t *d_a, const uint8_t *d_b, const svs_planes *planes,
                      uint64_t *d_sse, void *stream);
/* mean SSIM per frame -> d_ssim[n_frames] (double, device), as skimage.metrics.structural_similarity with its
 * defaults for 2-D uint8 input (7x7 uniform window, K1 .01, K2 .03, sample covariance, float64) - the call
 * behind the reference's evaluation.calc_ssim (evaluation.py:21-26).  d_data_range[n_frames] (double, device)
 * gives skimage's data_range per frame; pass NULL to use the reference's quirk, max - min of frame b.  A data range
 * of 0 (with NULL: a flat frame b, C1 = C2 = 0) gives skimage's result: a window's value is NaN where its denominator
 * is 0 (a window flat in both frames), and so is the frame's mean - a flat frame against itself yields NaN.
 * d_workspace: at least svs_ssim_workspace_bytes(planes) bytes of device memory.  d_a, d_b, d_data_range, d_ssim and
 * d_workspace 8-byte aligned.  H, W >= 7. */
uint64_t svs_ssim_workspace_bytes(const svs_planes *planes);
int svs_frame_ssim_dev(const uint8_t *d_a, const uint8_t *d_b, const svs_planes *planes,
                       const double *d_data_range, double *d_ssim, void *d_workspace, void *stream);
/* number of differing bits among the first n_bits of two packed streams -> *d_count (uint64,
 * device, overwritten) */
int svs_bit_errors_dev(const uint8_t *d_a_packed, const uint8_t *d_b_packed, uint64_t n_bits,
                       uint64_t *d_count, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SVSDCT_H */
