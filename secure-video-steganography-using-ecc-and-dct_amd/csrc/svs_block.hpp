// svs_block.hpp - per-block arithmetic of the fused block-DCT / QIM frame operator.
//
// Reference behaviour being implemented: proses_frame_qim_dct, config_and_setup.py:106-174.
//
// Everything here is plain C++ on values held in registers, compiled for the gfx950 device by
// svs_device.hpp (the product) and - with g++ - by tests/hostemu/ (test infrastructure only: it
// lets the CPU-only test tier and the sanitizers exercise the very same arithmetic and bit
// bookkeeping; the shipped library has no CPU path).  Build both with -ffp-contract=off: fused
// operations are spelled fmaf() explicitly so that host and device round identically.
//
// Decomposition (see DESIGN.md "Kernels"):
//   * one LANE owns one 8x8 block; the block never leaves that lane's registers, so the
//     separable transform needs no cross-lane traffic at all (no LDS, no shuffles) and a
//     wavefront (64 lanes = 64 horizontally adjacent blocks) reads/writes 512 contiguous
//     bytes per row instruction.
//   * only the coefficient rows the payload touches are transformed: flat indices 1..n live in
//     rows u < U = n/8 + 1 of the coefficient matrix, so the vertical pass produces U outputs
//     per column and the horizontal pass runs on U rows (template parameter U).
//   * the streaming embed (n <= 15) uses linearity of the DCT as a PREDICTION: trunc(clip(x + IDCT(D' - D))), where D' - D
//     is non-zero only at the n requantised coefficients and x is the exact integer pixel, is the reference's byte wherever
//     a rigorous bound on the reference's own float32 round-trip noise (BETA, tools/guard_bound.py) separates the predicted
//     value from the integer grid; the other blocks are redone with pocketfft's exact operation sequence (namespace pf).
//   * everything else (n >= 16, delta outside the guard's range, the "exact" mode) replays pocketfft on all 64 coefficients.
#pragma once
#include <math.h>
#include <stdint.h>

#include "svs_order.hpp"   // lowbias32 (the keyed dither)

#if defined(__HIPCC__)
#define SVS_HD __host__ __device__ __forceinline__
#else
#define SVS_HD inline
#endif

// compiler scheduling fence (device only): nothing is moved across it.  Used to keep the instruction scheduler from
// hoisting whole passes of independent work (and their live registers) ahead of where they are consumed.
#if defined(__HIP_DEVICE_COMPILE__)
#define SVS_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define SVS_SCHED_FENCE() ((void)0)
#endif

namespace svs {

// A block is held as two arrays of 8 little-endian dwords: rx[y] = pixels 0..3 of row y,
// ry[y] = pixels 4..7.  (Plain scalar arrays on purpose: an array of 8-byte structs is not fully
// scalarised by hipcc once 16-byte row loads are split into it, and ends up in LDS.)

// cos(k*pi/16)/2 and 1/sqrt(8): the orthonormal DCT-II basis (scipy norm='ortho',
// config_and_setup.py:135,168)
#define SVS_A0 0.35355339059327373f
#define SVS_C1 0.49039264020161522f
#define SVS_C2 0.46193976625564337f
#define SVS_C3 0.41573480615127262f
#define SVS_C4 0.35355339059327373f
#define SVS_C5 0.27778511650980114f
#define SVS_C6 0.19134171618254492f
#define SVS_C7 0.09754516100806417f

// Orthonormal 8-point DCT-II, first NOUT outputs only (even/odd split, FMA form: 36 ops for
// all eight outputs including the normalisation).
template <int NOUT>
SVS_HD void fdct8(const float (&x)[8], float (&X)[8]) {
    const float s0 = x[0] + x[7], s1 = x[1] + x[6], s2 = x[2] + x[5], s3 = x[3] + x[4];
    const float t0 = s0 + s3, t1 = s1 + s2;
    X[0] = (t0 + t1) * SVS_A0;
    if constexpr (NOUT > 1) {
        const float d0 = x[0] - x[7], d1 = x[1] - x[6], d2 = x[2] - x[5], d3 = x[3] - x[4];
        const float t2 = s0 - s3, t3 = s1 - s2;
        X[1] = fmaf(d0, SVS_C1, fmaf(d1, SVS_C3, fmaf(d2, SVS_C5, d3 * SVS_C7)));
        if constexpr (NOUT > 2) X[2] = fmaf(t2, SVS_C2, t3 * SVS_C6);
        if constexpr (NOUT > 3) X[3] = fmaf(d0, SVS_C3, fmaf(d1, -SVS_C7, fmaf(d2, -SVS_C1, d3 * -SVS_C5)));
        if constexpr (NOUT > 4) X[4] = (t0 - t1) * SVS_C4;
        if constexpr (NOUT > 5) X[5] = fmaf(d0, SVS_C5, fmaf(d1, -SVS_C1, fmaf(d2, SVS_C7, d3 * SVS_C3)));
        if constexpr (NOUT > 6) X[6] = fmaf(t2, SVS_C6, t3 * -SVS_C2);
        if constexpr (NOUT > 7) X[7] = fmaf(d0, SVS_C7, fmaf(d1, -SVS_C5, fmaf(d2, SVS_C3, d3 * -SVS_C1)));
    }
}

// Orthonormal 8-point DCT-III (inverse of the above) of a vector whose entries NIN..7 are zero.
// SKIP0: entry 0 is known to be zero as well (row 0 of the modification matrix: DC is never
// touched, config_and_setup.py:140).
template <int NIN, bool SKIP0>
SVS_HD void idct8(const float (&X)[8], float (&x)[8]) {
    if constexpr (NIN == 2 && !SKIP0) {
        // two inputs: evaluate the 8 outputs directly (1 mul + 8 fma) instead of butterflies (13 ops)
        const float p = X[0] * SVS_A0;
        x[0] = fmaf(X[1], SVS_C1, p); x[7] = fmaf(X[1], -SVS_C1, p);
        x[1] = fmaf(X[1], SVS_C3, p); x[6] = fmaf(X[1], -SVS_C3, p);
        x[2] = fmaf(X[1], SVS_C5, p); x[5] = fmaf(X[1], -SVS_C5, p);
        x[3] = fmaf(X[1], SVS_C7, p); x[4] = fmaf(X[1], -SVS_C7, p);
        return;
    }
    float a, b;  // even part: DC and X4
    {
        const float p = SKIP0 ? 0.0f : X[0] * SVS_A0;
        if constexpr (NIN > 4) {
            const float r = X[4] * SVS_C4;
            a = SKIP0 ? r : p + r;
            b = SKIP0 ? -r : p - r;
        } else {
            a = p;
            b = p;
        }
    }
    float e0 = a, e1 = b, e2 = b, e3 = a;
    if constexpr (NIN > 2) {
        float g0 = X[2] * SVS_C2, g1 = X[2] * SVS_C6;
        if constexpr (NIN > 6) {
            g0 = fmaf(X[6], SVS_C6, g0);
            g1 = fmaf(X[6], -SVS_C2, g1);
        }
        if constexpr (SKIP0 && NIN <= 4) {
            e0 = g0; e3 = -g0; e1 = g1; e2 = -g1;
        } else {
            e0 = a + g0; e3 = a - g0; e1 = b + g1; e2 = b - g1;
        }
    }
    if constexpr (NIN > 1) {
        float o0 = X[1] * SVS_C1, o1 = X[1] * SVS_C3, o2 = X[1] * SVS_C5, o3 = X[1] * SVS_C7;
        if constexpr (NIN > 3) {
            o0 = fmaf(X[3], SVS_C3, o0); o1 = fmaf(X[3], -SVS_C7, o1);
            o2 = fmaf(X[3], -SVS_C1, o2); o3 = fmaf(X[3], -SVS_C5, o3);
        }
        if constexpr (NIN > 5) {
            o0 = fmaf(X[5], SVS_C5, o0); o1 = fmaf(X[5], -SVS_C1, o1);
            o2 = fmaf(X[5], SVS_C7, o2); o3 = fmaf(X[5], SVS_C3, o3);
        }
        if constexpr (NIN > 7) {
            o0 = fmaf(X[7], SVS_C7, o0); o1 = fmaf(X[7], -SVS_C5, o1);
            o2 = fmaf(X[7], SVS_C3, o2); o3 = fmaf(X[7], -SVS_C1, o3);
        }
        x[0] = e0 + o0; x[7] = e0 - o0;
        x[1] = e1 + o1; x[6] = e1 - o1;
        x[2] = e2 + o2; x[5] = e2 - o2;
        x[3] = e3 + o3; x[4] = e3 - o3;
    } else {
        x[0] = e0; x[7] = e0; x[1] = e1; x[6] = e1;
        x[2] = e2; x[5] = e2; x[3] = e3; x[4] = e3;
    }
}

// byte B (0..3) of a dword as float: v_cvt_f32_ubyte{0..3} on the device
template <int B>
SVS_HD float ubyte_to_float(uint32_t w) {
    return (float)((w >> (8 * B)) & 0xffu);
}

// Store pixel value v - an INTEGER-valued float (pixel + floor(change)) - clipped to [0,255] into
// byte B of `old`.  np.uint8(np.clip(x, 0, 255)) of the reference (config_and_setup.py:171) is
// clip-then-truncate; for x = pixel + change with an integer pixel, trunc(clip(x)) ==
// clip(pixel + floor(change)), which is what the callers pass in.
template <int B>
SVS_HD uint32_t put_pixel(float v, uint32_t old) {
#if defined(__HIP_DEVICE_COMPILE__)
    // v_cvt_pk_u8_f32 saturates to [0,255] and rounds to nearest even (measured on gfx950:
    // profiles/history/r01_cvt_pk_u8_probe.json) - exact for the integer-valued input it gets here.
    return __builtin_amdgcn_cvt_pk_u8_f32(v, B, old);
#else
    const float c = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
    const uint32_t u = (uint32_t)c;
    return (old & ~(0xffu << (8 * B))) | (u << (8 * B));
#endif
}

// Same store for a value that is NOT integer-valued: round to nearest even, then saturate (what v_cvt_pk_u8_f32
// does; rintf on the host)
template <int B>
SVS_HD uint32_t put_pixel_rne(float v, uint32_t old) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_cvt_pk_u8_f32(v, B, old);
#else
    const float r = rintf(v);
    const float c = r < 0.0f ? 0.0f : (r > 255.0f ? 255.0f : r);
    return (old & ~(0xffu << (8 * B))) | ((uint32_t)c << (8 * B));
#endif
}

// Eight float pixel values of one row -> their bytes in two dwords: np.uint8(np.clip(v, 0, 255)) of the reference
// (config_and_setup.py:171), i.e. clip, then truncate toward zero.  On the device this is v_cvt_pk_u8_f32 executed with the
// wave's FP32 rounding mode switched to round-toward-zero for exactly these eight instructions: the conversion saturates
// to [0, 255] and follows MODE.fp_round (measured on gfx950 with tools/probes/cvt_round_mode.hip: 126.99999 -> 126,
// 0.99999994 -> 0, -0.9 -> 0, 255.7 -> 255), which saves the v_floor_f32 per pixel of the floor-then-convert form.  One asm
// statement, so that no other floating-point instruction can be scheduled into the window.  It opens with s_nop 1: two of
// these statements can end up back to back, and s_setreg -> s_setreg on the same hardware register needs 2 wait states that
// the compiler's hazard recogniser cannot insert inside inline asm.  The kernels run with the default
// round-to-nearest-even mode, which the closing s_setreg restores.
SVS_HD void store_row_trunc(float p0, float p1, float p2, float p3, float p4, float p5, float p6, float p7, uint32_t &lo4,
                            uint32_t &hi4) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t a, b;
    asm volatile(
        "s_nop 1\n\t"
        "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 3\n\t"
        "s_nop 0\n\t"
        "v_cvt_pk_u8_f32 %0, %2, 0, 0\n\t"
        "v_cvt_pk_u8_f32 %1, %6, 0, 0\n\t"
        "v_cvt_pk_u8_f32 %0, %3, 1, %0\n\t"
        "v_cvt_pk_u8_f32 %1, %7, 1, %1\n\t"
        "v_cvt_pk_u8_f32 %0, %4, 2, %0\n\t"
        "v_cvt_pk_u8_f32 %1, %8, 2, %1\n\t"
        "v_cvt_pk_u8_f32 %0, %5, 3, %0\n\t"
        "v_cvt_pk_u8_f32 %1, %9, 3, %1\n\t"
        "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 0"
        : "=&v"(a), "=&v"(b)
        : "v"(p0), "v"(p1), "v"(p2), "v"(p3), "v"(p4), "v"(p5), "v"(p6), "v"(p7));
    lo4 = a;
    hi4 = b;
#else
    const float v[8] = {p0, p1, p2, p3, p4, p5, p6, p7};
    uint32_t w[2] = {0, 0};
    for (int j = 0; j < 8; ++j) {
        const float c = v[j] < 0.0f ? 0.0f : (v[j] > 255.0f ? 255.0f : v[j]);   // NaN cannot occur (finite pixels)
        w[j >> 2] |= (uint32_t)c << (8 * (j & 3));
    }
    lo4 = w[0];
    hi4 = w[1];
#endif
}

// Forward transform of the coefficient rows u < U of one block.
// D[u][v] = sum_y sum_x a(u)a(v) p[y][x] cos((2y+1)u pi/16) cos((2x+1)v pi/16)
// (vertical axis first, as the reference does: axis=0 then axis=1, config_and_setup.py:135).
// Vertical pass for U = 2 on four columns held as the bytes of w[0..7]: the mirrored-row sums and differences the two
// outputs need are exact integers, so they are formed on 16-bit lanes (even bytes and odd bytes of the dwords: two
// columns per operation) and converted to float once - same values as the float path, fewer operations.
SVS_HD void vertical_u2_packed(const uint32_t (&w)[8], float (&v0)[4], float (&v1)[4]) {
    typedef int16_t i16x2 __attribute__((vector_size(4)));
    uint32_t lane[2][8];  // [0]: bytes 0 and 2 (columns 0, 2), [1]: bytes 1 and 3 (columns 1, 3), as 16-bit lanes
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        lane[0][r] = w[r] & 0x00ff00ffu;
        lane[1][r] = (w[r] >> 8) & 0x00ff00ffu;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        uint32_t s[4];
        i16x2 d[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s[k] = lane[h][k] + lane[h][7 - k];  // <= 510 per lane: no carry between lanes
            d[k] = __builtin_bit_cast(i16x2, lane[h][k]) - __builtin_bit_cast(i16x2, lane[h][7 - k]);
        }
        const uint32_t t = (s[0] + s[3]) + (s[1] + s[2]);  // <= 2040 per lane
#pragma unroll
        for (int c = 0; c < 2; ++c) {  // 16-bit lane c of half h is column 2c + h
            const float x0 = (float)(c ? (t >> 16) : (t & 0xffffu));
            v0[2 * c + h] = x0 * SVS_A0;
            const float d0 = (float)d[0][c], d1 = (float)d[1][c], d2 = (float)d[2][c], d3 = (float)d[3][c];
            v1[2 * c + h] = fmaf(d0, SVS_C1, fmaf(d1, SVS_C3, fmaf(d2, SVS_C5, d3 * SVS_C7)));
        }
    }
}

// U = 1: only the column sums are needed
SVS_HD void vertical_u1_packed(const uint32_t (&w)[8], float (&v0)[4]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        uint32_t t = 0;
#pragma unroll
        for (int r = 0; r < 8; ++r) t += h ? ((w[r] >> 8) & 0x00ff00ffu) : (w[r] & 0x00ff00ffu);  // <= 2040 per lane
        v0[h] = (float)(t & 0xffffu) * SVS_A0;
        v0[2 + h] = (float)(t >> 16) * SVS_A0;
    }
}

// Flat index 4 (coefficient (0, 4), basis +-1/8) exactly as pocketfft computes it, from row 0 of the vertical pass (which is
// pocketfft's, see forward_rows): for integer pixels this coefficient is a multiple of 1/8, so c / delta sits EXACTLY on a
// rounding tie in 1 of 8 delta blocks and only the reference's own float32 sequence says which way it falls.
// These are the operations of svs::pf::dct2_8 that feed output 4 (radb2 / radb4 sums, one twiddle product), nine in all.
SVS_HD float pf_row0_coefficient4(const float *v0) {
    const float c0 = 2.0f * v0[0], c7 = 2.0f * v0[7];
    const float c1 = v0[1] + v0[2], c3 = v0[3] + v0[4], c5 = v0[5] + v0[6];
    const float h0 = c0 + c7, h1 = c1 + c5;
    const float a0 = fmaf(2.0f, c3, h0);
    return fmaf(-2.0f, h1, a0) * 0x1.6a09e6p-3f;   // r[4] * (float(cos(pi/4)) / 4)
}

// `side` (optional): two by-products of row 0 of the vertical pass, V[0][x] = fl(colsum_x * a(0)) - the one part of this
// transform that is bit-identical to pocketfft's (its sums are exact integers and the product rounds once): the reference's
// own value of flat index 4 (pf_row0_coefficient4) and the sum of V[0] (= a(0) * the block's pixel sum, up to 8 roundings).
// Taken here so that the eight values need not stay in registers.
struct ForwardSide {
    float c4, v0_sum;
};
SVS_HD void forward_side(const float (&v0)[8], ForwardSide *side) {
    side->c4 = pf_row0_coefficient4(v0);
    side->v0_sum = ((v0[0] + v0[1]) + (v0[2] + v0[3])) + ((v0[4] + v0[5]) + (v0[6] + v0[7]));
}
template <int U>
SVS_HD void forward_rows(const uint32_t (&rx)[8], const uint32_t (&ry)[8], float (&D)[U][8], ForwardSide *side = nullptr) {
    float V[U][8];
    if constexpr (U == 1) {
        float a0[4], b0[4];
        vertical_u1_packed(rx, a0);
        vertical_u1_packed(ry, b0);
#pragma unroll
        for (int x = 0; x < 4; ++x) { V[0][x] = a0[x]; V[0][4 + x] = b0[x]; }
        if (side) forward_side(V[0], side);
        fdct8<8>(V[0], D[0]);
        return;
    }
    if constexpr (U == 2) {
        float a0[4], a1[4], b0[4], b1[4];
        vertical_u2_packed(rx, a0, a1);
        vertical_u2_packed(ry, b0, b1);
#pragma unroll
        for (int x = 0; x < 4; ++x) { V[0][x] = a0[x]; V[1][x] = a1[x]; V[0][4 + x] = b0[x]; V[1][4 + x] = b1[x]; }
        if (side) forward_side(V[0], side);
#pragma unroll
        for (int u = 0; u < U; ++u) fdct8<8>(V[u], D[u]);
        return;
    }
#define SVS_COL(X, W, B)                                                                \
    {                                                                                   \
        const float col[8] = {ubyte_to_float<B>(W[0]), ubyte_to_float<B>(W[1]), \
                              ubyte_to_float<B>(W[2]), ubyte_to_float<B>(W[3]), \
                              ubyte_to_float<B>(W[4]), ubyte_to_float<B>(W[5]), \
                              ubyte_to_float<B>(W[6]), ubyte_to_float<B>(W[7])}; \
        float out[8];                                                                   \
        fdct8<U>(col, out);                                                             \
        _Pragma("unroll") for (int u = 0; u < U; ++u) V[u][X] = out[u];                 \
    }
    SVS_COL(0, rx, 0) SVS_COL(1, rx, 1) SVS_COL(2, rx, 2) SVS_COL(3, rx, 3)
    SVS_COL(4, ry, 0) SVS_COL(5, ry, 1) SVS_COL(6, ry, 2) SVS_COL(7, ry, 3)
#undef SVS_COL
    if (side) forward_side(V[0], side);
#pragma unroll
    for (int u = 0; u < U; ++u) fdct8<8>(V[u], D[u]);
}

struct QimParams {
    float delta_f;      // (float)delta  - divisor
    float inv_delta_f;  // 1 / delta_f   - exact when delta is a power of two (QM_POW2)
    double delta_d;     // delta         - multiplier when (double)delta_f != delta (QM_DOUBLE)
    float tie_slope;    // FAST extraction: c00 * tie_slope bounds |c_fast/delta - c_pocketfft/delta| (see TIE_SLOPE)
    float tie2_sum, tie2_resid, tie2_c00;   // ... and its per-block refinement (SVS_TIE2_*), all per unit of 1/delta
    float tie2_max;                         // the largest value that margin takes over all blocks (any pixel sum)
    // GUARDED embed (embed_block_guarded): BETA = g_sum * (sum of pixels) + g_resid * sqrt(64 sum p^2 - (sum p)^2) + g_delta
    float g_sum, g_resid, g_delta;
};

// FAST extraction and rounding ties.  The FMA-factored forward transform (forward_rows) and pocketfft's are two float32
// evaluations of the same 64-term sums; for pixels in [0, 255] they differ by at most
//        |c_fast - c_pf| <= TIE_SLOPE * c00,     c00 = DC coefficient = (sum of the block's pixels) / 8,
// a forward error bound derived (and printed per coefficient row count) by tools/tie_bound.py: both algorithms are linear
// in the non-negative pixels, every path from a pixel to the output collects at most m factors (1 + d), |d| <= 2^-24, so
// the error is at most gamma_m * (sum of |path weights|) * (sum of pixels).  The largest slope over all coefficient
// indices and all U is 177 * 2^-24 = 1.055e-5; the constant below adds the roundings of the quantiser input itself
// (c * (1/delta): 3 more factors on |c| <= 2 c00) and 1 % of slack.  extract_block() reports a block in which some
// c/delta lies within that distance of a half-integer; the kernel then recomputes the block with the pocketfft-identical
// transform (extract_block_exact) - so FAST extraction returns the reference's bits for ANY input, ties included, while
// stego frames (coefficients sit near multiples of delta, far from ties) never take the second path.
#define SVS_TIE_SLOPE (1.055e-5 * 1.01 + 8.0 * 5.9604644775390625e-8)
// What the kernels test (round 3): the same difference bounded per block from its energy (tools/guard_bound.py --tie: first-
// order running error analysis of both operation sequences, as for the GUARDED embed),
//        |c_fast - c_pf| <= u' * (KDC * mean + KE * ||X - mean||_2),   u' = 2^-24 (1 + 2^-10),
// with ||X - mean||_2^2 = Q - S^2/64 <= S (16320 - S) / 64 (pixels <= 255), so that the block's pixel sum S is all it takes:
// 4x tighter than the global slope at mean 128 (3.5e-3 -> never-embedded noise: 0.7 % of the blocks at n = 10, delta = 8
// instead of 4 %).  Flat index 4 does not enter: its value is pocketfft's own (pf_row0_coefficient4).
// Constants of the largest row count (U = 8; U = 2: KE 24.3):
#define SVS_FAST_EXTRACT_DELTA_MIN 0x1p-10   // below, |c / delta| can reach 2^22 and extract_block_cheap's rounding constant no longer rounds: exact kernels
#define SVS_TIE2_KDC 64.0001
#define SVS_TIE2_KE 25.92

// How the quantiser is evaluated (all three give the reference's result, they differ in cost):
//   QM_F32    general delta: IEEE float32 division (about 10 instructions), float32 requantisation
//   QM_DOUBLE delta not representable in float32 (e.g. 0.1): divide by (float)delta, requantise with
//             a double multiply rounded once to float32 - what `float(q * delta)` does (:156)
//   QM_POW2   delta = 2^k: c / delta == c * (1/delta) exactly (both are the correctly rounded value of
//             the same real number), so the division is one multiply
enum QuantMode { QM_F32 = 0, QM_DOUBLE = 1, QM_POW2 = 2 };

// q = int(round(c / delta)) : float32 division, round half to even (config_and_setup.py:148,160).
// General delta: t = c * (1/delta) is within 3 * 2^-24 |t| of the correctly rounded quotient e = fl(c/delta),
// so rint(t) == rint(e) unless a half-integer lies within that distance of t; only then (about one
// coefficient in 10^5) is the 10-instruction IEEE division evaluated.  tests/test_block_arithmetic_cpu.py
// checks the shortcut against the division on 10^8 samples including every exact tie.
template <int QM>
SVS_HD int quant_index(float c, const QimParams &qp) {
    if constexpr (QM == QM_POW2) {
        return (int)rintf(c * qp.inv_delta_f);
    } else {
        const float t = c * qp.inv_delta_f;
        float r = rintf(t);
        const float miss = fabsf(fabsf(t - r) - 0.5f);       // distance of t from the nearest half-integer
        if (miss <= fabsf(t) * 4.76837158203125e-7f)          // 2^-21 |t|: comfortably above 3 * 2^-24 |t|
            r = rintf(c / qp.delta_f);
        return (int)r;
    }
}

// reference form of the above, used by the tests to validate the shortcut
// q with its parity forced to the payload bit by +1 (bit 1, q even) or -1 (bit 0, q odd) - config_and_setup.py:150-155:
// `q % 2` of a negative q is 0 or 1 in python, which is the low bit of the two's complement, so q + bit - (q & 1) is q with
// its low bit replaced by the bit: one v_bfi_b32 instead of and / subtract / add.
SVS_HD int force_parity(int q, int bit) { return (q & ~1) | bit; }
SVS_HD int quant_index_by_division(float c, float delta_f) { return (int)rintf(c / delta_f); }

// the float32 value written for index q: `float(q * delta)` (config_and_setup.py:156)
template <int QM>
SVS_HD float requantised(int q, const QimParams &qp) {
    if constexpr (QM == QM_DOUBLE) return (float)((double)q * qp.delta_d);
    else return (float)q * qp.delta_f;
}

// SVS_NEAREST (include/svsdct.h): force_parity moves a wrong parity in a fixed direction - +1 for bit 1, -1 for bit 0 - which
// is the FARTHER of the two neighbouring lattice points for half of the coefficients (a move of up to 1.5 delta).  This rule
// goes to the nearer one: with c0 = the value written for the unforced index q, q + 1 if c > c0, q - 1 if c < c0, and the
// reference's choice when c == c0 (a coefficient that is exactly 0, as every AC coefficient of a constant block).  The move
// is at most delta plus rounding; the receiver reads q mod 2 and does not change.  The side is taken from c0 and not from
// c / delta - q: no division-rounding corner, and the multiply is the one the requantisation has anyway.
template <int QM>
SVS_HD int nearest_parity(int q, int bit, float c, const QimParams &qp) {
    const float c0 = requantised<QM>(q, qp);
    const int dir = c > c0 ? 1 : (c < c0 ? -1 : 2 * bit - 1);
    return q + (((q ^ bit) & 1) ? dir : 0);
}

// SVS_MINMOVE (include/svsdct.h): the receiver needs a payload coefficient INSIDE the decision cell of its index, within
// delta / 2 of the lattice point c_t, and far enough from the cell's edge to survive the one disturbance between embedder and
// receiver: the clip-and-truncate of the stego pixels.  In a block that does not clip, the truncation error of a pixel is in
// (-1, 0]; an AC basis function b_k (k = 8 u + v) sums to 0, so the error of coefficient k is sum_x b_k(x) e(x) with e in
// (-1, 0]^64, at most 0.5 * sum |b_k| = 0.5 * S_u * S_v in magnitude, where S_u = sum_x |a_u cos((2 x + 1) u pi / 16)|,
// a_0 = sqrt(1/8), a_u = 1/2: S = {2.828427, 2.562915, 2.613126, 2.562915, 2.828427, 2.562915, 2.613126, 2.562915}.  The
// pattern e = -1 where b_k > 0, else 0, reaches it: the bound is tight, between 3.284 (S_1 S_1 / 2) and 4.0 (S_0 S_4 / 2).
// MARGIN[k] = (float)(0.5 * S_u * S_v + 0.0625): the 1/16 covers the float32 noise of the round trip (the guard's BETA is
// about 1e-3) and the division rounding of the quantiser.  Entry 0 (DC, never a payload coefficient) is not used.
// tests/test_minmove_cpu.py recomputes the table and shows that the bound is attained.
SVS_HD float minmove_margin(uint32_t k) {
    static constexpr float MARGIN[64] = {   // [8 u + v]; entry 0 is the DC position's: never a payload coefficient
        4.0625f,    3.6870098f, 3.758018f,  3.6870098f, 4.0625f,    3.6870098f, 3.758018f,  3.6870098f,
        3.6870098f, 3.346768f,  3.4111104f, 3.346768f,  3.6870098f, 3.346768f,  3.4111104f, 3.346768f,
        3.758018f,  3.4111104f, 3.4767137f, 3.4111104f, 3.758018f,  3.4111104f, 3.4767137f, 3.4111104f,
        3.6870098f, 3.346768f,  3.4111104f, 3.346768f,  3.6870098f, 3.346768f,  3.4111104f, 3.346768f,
        4.0625f,    3.6870098f, 3.758018f,  3.6870098f, 4.0625f,    3.6870098f, 3.758018f,  3.6870098f,
        3.6870098f, 3.346768f,  3.4111104f, 3.346768f,  3.6870098f, 3.346768f,  3.4111104f, 3.346768f,
        3.758018f,  3.4111104f, 3.4767137f, 3.4111104f, 3.758018f,  3.4111104f, 3.4767137f, 3.4111104f,
        3.6870098f, 3.346768f,  3.4111104f, 3.346768f,  3.6870098f, 3.346768f,  3.4111104f, 3.346768f};
    return MARGIN[k & 63u];
}

// How a payload coefficient is written.  REFERENCE: the lattice point of the reference's forced index.  NEAREST: the lattice
// point of nearest_parity's index.  MINMOVE: nearest_parity's lattice point c_t is only the centre of a band - the
// coefficient is clamped into [c_t - r_k, c_t + r_k], r_k = max(0, delta / 2 - MARGIN[k]), and keeps its forward-transform
// value when it is already inside.  With every r_k = 0 (delta <= 6.69) that is NEAREST.
enum QimRuleKind { RULE_REFERENCE = 0, RULE_NEAREST = 1, RULE_MINMOVE = 2 };

// What the EMBED bodies take: the quantiser parameters plus the rule that forces a wrong parity.  A type of its own, so that
// QimParams - a by-value argument of every kernel, the extract kernels included - keeps its layout.  A plain QimParams
// converts to the reference's rule.  The kernels build it from a wave-uniform argument (Geometry::pad, set from the plan) as a
// compile-time constant on every side of ONE branch around their whole body (svs_device.hpp), so inside a body every test
// of `kind` folds away and the default rule's instruction stream is what it was before the flags existed.
struct QimRule : QimParams {
    uint32_t kind;      // QimRuleKind: RULE_REFERENCE, RULE_NEAREST (SVS_NEAREST: nearest_parity instead of force_parity) or
                        // RULE_MINMOVE (SVS_MINMOVE: nearest_parity and the band)
    float half_cell;    // SVS_MINMOVE: h = (float)(0.5 * (double)delta), rounded once on the host; not read otherwise
    SVS_HD QimRule(const QimParams &p, uint32_t kind_ = 0u, float half_cell_ = 0.0f)
        : QimParams(p), kind(kind_), half_cell(half_cell_) {}
};

// The rule in one existing 32-bit word of the launch (Geometry::pad): 0 = the reference's, 1 = SVS_NEAREST, anything else =
// SVS_MINMOVE and the word is the bit pattern of h.  A positive float32 is never 0, and it is 1 only as the smallest
// denormal; h = 0 (delta below 2^-149) is sent as 1 too: with such an h every r_k is 0 and the rule IS the nearest one.
SVS_HD uint32_t rule_word(bool nearest, bool minmove, float half_cell) {
    if (!minmove) return nearest ? 1u : 0u;
    const uint32_t w = __builtin_bit_cast(uint32_t, half_cell);
    return w > 1u ? w : 1u;
}
SVS_HD QimRule rule_from_word(const QimParams &p, uint32_t w) {
    return w > 1u ? QimRule(p, (uint32_t)RULE_MINMOVE, __builtin_bit_cast(float, w)) : QimRule(p, w);
}

// r_k of SVS_MINMOVE for flat index k (0 under the other rules: not evaluated there).  k is a compile-time constant in the
// lane-per-block loops (the margin is then a literal) and a lane's own index in the 8-lane replays (a table read).
template <int RULE>
SVS_HD float qim_band(const QimRule &qp, uint32_t k) {
    if constexpr (RULE == RULE_MINMOVE) return fmaxf(0.0f, qp.half_cell - minmove_margin(k));
    else return 0.0f;
}

// c clamped into the band of half-width r around the lattice point ct (SVS_MINMOVE; float32, this order on host and device)
SVS_HD float minmove_clamp(float c, float ct, float r) { return fminf(fmaxf(c, ct - r), ct + r); }

// One payload coefficient through the quantiser, integer form: the value that replaces c.  RULE (a QimRuleKind; `true` is
// RULE_NEAREST) is a compile-time argument of this FUNCTION: the exact bodies choose between the forms of their quantiser loop
// with one test of qp.kind per block (a constant inside a kernel's body, see QimRule).  r: qim_band of the coefficient.
template <int QM, int RULE>
SVS_HD float qim_target(float c, int bit, const QimParams &qp, float r = 0.0f) {
    const int q = quant_index<QM>(c, qp);
    const float ct = requantised<QM>(RULE != RULE_REFERENCE ? nearest_parity<QM>(q, bit, c, qp) : force_parity(q, bit), qp);
    if constexpr (RULE == RULE_MINMOVE) return minmove_clamp(c, ct, r);
    else return ct;
}

// ---------------------------------------------------------------------------------------------------------------------
// Keyed dither modulation (svs_embed_dithered* / svs_extract_dithered*, include/svsdct.h): both sides shift the lattice of
// every payload coefficient by a key-derived offset d in [-delta, delta), a whole parity period.  A format: sender and receiver
// must compute the same d, so nothing here may change.  For clip frame t = first_frame + f, raster block i of the frame (its
// physical position, whatever its stream slot) and flat row-major coefficient k, all integer arithmetic mod 2^32:
//   seed = lb(lb(hi32(key) ^ 0x85EBCA6B) ^ lo32(key))     (dither_seed; not the block order's seed: one key may serve both)
//   s_t = lb(seed ^ t);  s_b = lb(s_t + i * 0x9E3779B1)   (dither_block_seed)
//   h = lb(s_b ^ (k * 0x632BE5AB));  r = (float)(h >> 8) * 2^-23 - 1  (exact, in [-1, 1));  d = r * (float)delta
// NOT a cryptographic generator (lb = lowbias32, as svs_order.hpp says of the order): it removes the keyless comb test and the
// keyless read of the bits; confidentiality remains AES-GCM's.  Every float step is one IEEE float32 operation (build with
// -ffp-contract=off), the same on host and device.
// ---------------------------------------------------------------------------------------------------------------------

SVS_HD uint32_t dither_seed(uint64_t key) {
    return lowbias32(lowbias32((uint32_t)(key >> 32) ^ 0x85EBCA6Bu) ^ (uint32_t)key);
}

// s_b of raster block i of clip frame t
SVS_HD uint32_t dither_block_seed(uint32_t seed, uint32_t t, uint32_t i) {
    return lowbias32(lowbias32(seed ^ t) + i * 0x9E3779B1u);
}

// d of coefficient k (a compile-time index in the lane-per-block loops: k * 0x632BE5AB is then a literal)
SVS_HD float dither_value(uint32_t s_b, uint32_t k, float delta_f) {
    const uint32_t h = lowbias32(s_b ^ (k * 0x632BE5ABu));
    const float r = (float)(h >> 8) * 0x1p-23f - 1.0f;   // 24 bits: the conversion, the power-of-two product and the sum are exact
    return r * delta_f;
}

// One payload coefficient through the dithered quantiser: today's rule on c' = c - d, moved back by d.  A coefficient the
// rule leaves alone (SVS_MINMOVE inside its band: cn' is c' bit for bit) keeps its forward-transform value exactly, not
// (c - d) + d.  The minimum-move band is that of flat index k.
template <int QM, int RULE>
SVS_HD float dithered_target(float c, int bit, const QimRule &qp, uint32_t k, uint32_t s_b) {
    const float d = dither_value(s_b, k, qp.delta_f);
    const float cp = c - d;
    const float cn = qim_target<QM, RULE>(cp, bit, qp, qim_band<RULE>(qp, k));
    return __builtin_bit_cast(uint32_t, cn) == __builtin_bit_cast(uint32_t, cp) ? c : cn + d;
}

// the receiver's side: the parity of the index of c - d
template <int QM>
SVS_HD uint32_t dithered_parity(float c, const QimParams &qp, uint32_t k, uint32_t s_b) {
    return (uint32_t)quant_index<QM>(c - dither_value(s_b, k, qp.delta_f), qp) & 1u;
}

// 64 stream bits starting at stream bit s of an MSB-first packed buffer viewed as dwords
// (touches at most dwords s/32 .. s/32+2, each only if below n_words)
SVS_HD void payload_window(const uint32_t *bits, uint32_t n_words, uint64_t s, uint32_t &hi, uint32_t &lo) {
    const uint32_t wi = (uint32_t)(s >> 5), sh = (uint32_t)(s & 31u);
    const uint32_t w0 = __builtin_bswap32(wi < n_words ? bits[wi] : 0u);
    const uint32_t w1 = __builtin_bswap32(wi + 1 < n_words ? bits[wi + 1] : 0u);
    const uint32_t w2 = __builtin_bswap32(wi + 2 < n_words ? bits[wi + 2] : 0u);
    const uint64_t a = ((uint64_t)w0 << 32) | w1, b = ((uint64_t)w1 << 32) | w2;
    hi = (uint32_t)((a << sh) >> 32);
    lo = (uint32_t)((b << sh) >> 32);
}

// n <= 15 (one and two coefficient rows): a block's window - and the windows of two adjacent blocks, 2 n <= 30 bits - lies
// inside the 64 stream bits that start at the dword holding stream bit s: two loads instead of three per block (six per lane
// with two blocks per lane).  payload_qword returns those 64 bits, MSB first; window32 the 32 stream
// bits starting `sh` bits in (sh < 32 for the block at s, < 47 for its right neighbour).
SVS_HD uint64_t payload_qword(const uint32_t *bits, uint32_t n_words, uint64_t s) {
    const uint32_t wi = (uint32_t)(s >> 5);
    const uint32_t w0 = __builtin_bswap32(wi < n_words ? bits[wi] : 0u);
    const uint32_t w1 = __builtin_bswap32(wi + 1 < n_words ? bits[wi + 1] : 0u);
    return ((uint64_t)w0 << 32) | w1;
}
SVS_HD uint32_t window32(uint64_t q, uint32_t sh) { return (uint32_t)((q << sh) >> 32); }

// bit i (0 = first) of the 64-bit MSB-first window hi:lo
SVS_HD uint32_t window_bit(uint32_t hi, uint32_t lo, int i) {
    return ((i < 32) ? (hi >> ((31 - i) & 31)) : (lo >> ((63 - i) & 31))) & 1u;
}

// A coefficient SELECTION (include/svsdct.h svs_coeffs) in the form the exact bodies read it: the inverse table.  Byte k & 3
// of w[k >> 2] is the block-local stream slot that flat row-major coefficient k carries, 0xFF for none; count = slots per
// block.  count == 0: no selection - the row-major prefix 1..n of the call.  The quantiser loops stay unrolled over k, so
// slot(k) has a compile-time position (a scalar shift and mask of a kernel-argument dword) and the coefficient registers
// keep compile-time indices; only the slot - which bit of the payload window - is a run-time, wave-uniform value.
struct CoeffTable {
    uint32_t w[16];
    uint32_t count;
    SVS_HD uint32_t slot(int k) const { return (w[k >> 2] >> (8 * (k & 3))) & 0xFFu; }
};

struct DitherArgs {          // by-value argument of the two exact kernels (read by their U = 8 instantiations only)
    uint32_t seed;           // dither_seed(key)
    uint32_t first_frame;    // frame f of the call is clip frame first_frame + f
    uint32_t on;             // 0: no dither - the kernel's side that was there before the dither
    CoeffTable sel;          // on: the call's selection, or the prefix table of n_ac (make_prefix_table) - never empty.  The
                             // dithered side's own copy: read from the kernel's `sel` as well, that table went to scratch.
                             // extract_exact_kernel: empty on its hard sides; the table of its soft side, on or off (SoftArgs)
};

// The requantisation channel (include/svsdct.h svs_steps) as embed_exact_kernel takes it, by value: byte k & 3 of w[k >> 2] is the
// step of flat row-major coefficient k, 1..255.  on == 0: an embed launch - the kernel as it was.  Read by the one
// instantiation that holds the channel body (svs_device.hpp); k is a compile-time index there, so a step is a scalar shift
// and mask of a kernel-argument dword and one scalar conversion.
struct ChannelArgs {
    uint32_t on;
    uint32_t w[16];
    SVS_HD float step(int k) const { return (float)((w[k >> 2] >> (8 * (k & 3))) & 0xFFu); }
};

// host side: the channel of a checked table (every entry 1..255)
inline ChannelArgs make_channel_args(const uint16_t (&step)[64]) {
    ChannelArgs c{};
    c.on = 1u;
    for (int k = 0; k < 64; ++k) c.w[k >> 2] |= ((uint32_t)step[k] & 0xFFu) << (8 * (k & 3));
    return c;
}

// Per-coefficient QIM steps (include/svsdct.h svs_qim_steps) as the two exact kernels take them, by value: half k & 1 of
// w[k >> 1] is delta[k] of flat row-major coefficient k, 1..4095 (entry 0, DC, is carried and never read).  on == 0: the kernel
// as it was.  Read by the instantiations that hold the stepped side (svs_device.hpp); k is a compile-time index in their loops,
// so a step is a scalar shift and mask of one kernel-argument dword and one scalar conversion, read where it is used.
#define SVS_STEP_GATE_SHIFT 8
#define SVS_STEP_MATRIX_SHIFT 16
struct StepArgs {
    uint32_t on;      // bit 0: a stepped call.  Bits 8..14, read by readback_kernel's stepped form alone: the margin pass's gate.
                      // Bits 16..19, read by the two exact kernels' stepped sides alone: a matrix call (svs_matrix_*) - k in
                      // bits 16..18, the pair search in bit 19 (make_matrix_word); a matrix call never reaches readback_kernel
    uint32_t w[32];
    SVS_HD uint32_t margin_gate() const { return on >> SVS_STEP_GATE_SHIFT; }
    SVS_HD uint32_t matrix() const { return on >> SVS_STEP_MATRIX_SHIFT; }   // 0: no matrix call; else k | search << 3
    SVS_HD float step(int k) const { return (float)((w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu); }
    // The same value with the dword's index hidden from the compiler until this point, so that the dword is loaded HERE.  Left
    // to itself the compiler loads all 32 at the kernel's entry and holds them: extract_exact_kernel then took 100 instead of
    // 80 scalar registers.  (In embed_exact_kernel the hidden index sent a copy of the table to scratch: it reads step().)
    SVS_HD float step_here(int k) const {
        int i = k >> 1;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+s"(i));
#endif
        return (float)((w[i] >> (16 * (k & 1))) & 0xFFFFu);
    }
    // dwords 2j and 2j + 1 - the steps of coefficients 4j .. 4j + 3 - loaded HERE in the same way, steps 4j and 4j + 1 in the low
    // half.  One read for four coefficients: the compiler reads this kernel argument in place only while it can follow every
    // address formed on it, up to a fixed number of them (300 in this LLVM); past that it copies the table to scratch at the
    // kernel's entry.  The stepped soft side (stepped_soft_bytes) on top of stepped_parities' two loops stays below it with 16
    // reads, not with 63 or 32.
    SVS_HD uint64_t quad_here(int j) const {
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+s"(j));
#endif
        uint64_t q;
        __builtin_memcpy(&q, &w[2 * j], sizeof q);
        return q;
    }
    static SVS_HD float step_of_quad(uint64_t quad, int k) { return (float)(uint32_t)((quad >> (16 * (k & 3))) & 0xFFFFu); }
};

// host side: the steps of a checked table (every entry k >= 1 in 1..4095)
inline StepArgs make_step_args(const uint16_t (&delta)[64]) {
    StepArgs s{};
    s.on = 1u;
    for (int k = 1; k < 64; ++k) s.w[k >> 1] |= (uint32_t)delta[k] << (16 * (k & 1));
    return s;
}

// host side: the table of `count` indices; false unless they are distinct and in 1..63 (count <= 63)
inline bool make_coeff_table(const uint8_t *index, uint32_t count, CoeffTable *t) {
    for (int i = 0; i < 16; ++i) t->w[i] = 0xFFFFFFFFu;
    t->count = 0;
    if (count > 63) return false;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t k = index[i];
        if (k < 1 || k > 63 || t->slot((int)k) != 0xFFu) return false;
        t->w[k >> 2] &= ~(0xFFu << (8 * (k & 3))) | (i << (8 * (k & 3)));
    }
    t->count = count;
    return true;
}

// the table of the selection 1, 2, .., n (n <= 63): the dithered calls without a selection run the selected loops with it
inline CoeffTable make_prefix_table(uint32_t n) {
    uint8_t index[63];
    for (uint32_t i = 0; i < 63; ++i) index[i] = (uint8_t)(i + 1);
    CoeffTable t;
    make_coeff_table(index, n < 63u ? n : 63u, &t);
    return t;
}

// the selection 1, 2, .., count: what a call without a selection does at n_ac = count
inline bool coeff_table_is_prefix(const CoeffTable &t) {
    for (uint32_t k = 1; k <= t.count; ++k)
        if (t.slot((int)k) != k - 1) return false;
    return true;
}

// bit s (0 = first; run-time, wave-uniform) of the 64-bit MSB-first window hi:lo; (63 - s) & 31 == (31 - s) & 31
SVS_HD uint32_t window_bit_at(uint32_t hi, uint32_t lo, uint32_t s) {
    return ((s < 32u ? hi : lo) >> ((31u - s) & 31u)) & 1u;
}

// bits a block takes from a budget of n_bits when its first stream bit is `first`
// (config_and_setup.py:130,132,141)
SVS_HD uint32_t block_budget(uint64_t first, uint64_t n_bits, uint32_t n) {
    if (first >= n_bits) return 0;
    const uint64_t left = n_bits - first;
    return left < n ? (uint32_t)left : n;
}

// frac(x) = x - floor(x) in [0, 1) (v_fract_f32) and min(a, |b|, |c|) (one v_min3_f32 with source modifiers)
SVS_HD float fract_f32(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_fractf(x);
#else
    const float f = x - floorf(x);
    return f < 1.0f ? f : 0x1.fffffep-1f;   // v_fract_f32 clamps to the largest float below 1
#endif
}
SVS_HD float fmin3_abs(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
    // spelled out: from the C form hipcc makes v_min_f32 |b|, |c| followed by a v_min3 that joins two such pairs - 56 instead
    // of 32 instructions of the 1.6-slot class per block (profiles/r04_valu_issue_rate.txt)
    float r;
    asm("v_min3_f32 %0, %1, |%2|, |%3|" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
#else
    return fminf(a, fminf(fabsf(b), fabsf(c)));
#endif
}

// (Rounds 1-3 had a separate FAST embed arithmetic here - FMA-factored forward transform on the payload rows, per-pixel grid
// test only for blocks that did not look "generic" - whose contract was "PSNR within 0.01 dB".  Each review found structured
// content on which the shortcut broke it (r02: exact cancellations, r03: coefficients requantised to 0 on smooth ramps,
// +0.68 dB), round 4's own probe a third family (two equal coefficients of a diagonal ramp cancelling on the anti-diagonal),
// and with the test on every pixel the arithmetic was no faster than the bit-identical kernels: n = 63 1.45 ms against the
// lane-per-block pocketfft kernel's 1.31 per 200 x 4K, n = 8..15 0.88 against the rigorous two-row kernel's 0.87
// (profiles/r04_*).  It is gone: every embed mode produces the reference's pixels.)

SVS_HD uint32_t dot4_u8(uint32_t a, uint32_t b, uint32_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(a, b, acc, false);   // v_dot4_u32_u8
#else
    for (int i = 0; i < 4; ++i) acc += ((a >> (8 * i)) & 0xffu) * ((b >> (8 * i)) & 0xffu);
    return acc;
#endif
}

SVS_HD float guard_sqrt(float v) {   // any sqrt accurate to a few ulp will do: BETA's constants carry 2^-18 of slack
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sqrtf(v);
#else
    return sqrtf(v);
#endif
}

// FAST extraction with two and more coefficient rows, in two steps (round 4).
//
// extract_block_cheap: parity bits of round(c_k/delta), k = 1..n, MSB-first into hi:lo (config_and_setup.py:160-161), from the
// FMA-factored forward transform.  t + 1.5 * 2^23 rounds t = c * (1/delta) to the nearest-even integer q and leaves q in the
// low mantissa bits of the sum (|t| < 2^22: the host routes delta < 2^-10 to the exact kernels), so the parity is bit 0 of the
// sum's pattern and one v_alignbit_b32 per coefficient - taken in DESCENDING order - shifts it into place: no rndne, no
// conversion, no shift / or (three 1.6-slot instructions per coefficient before, profiles/r04_valu_issue_rate.txt).
// Returns true when the block is a CANDIDATE: some t lies within qp.tie2_max - the largest value the per-block margin below
// can take for any block - of a rounding tie.  A block that is not a candidate has the reference's bits (the margin bounds
// |c_fast - c_pocketfft| / delta for EVERY coefficient, flat index 4 included: tools/guard_bound.py --tie), and needs nothing
// else; stego frames at delta >= 8 have no candidates at all (their coefficients sit within 4 / delta of the quantiser grid),
// so a wave of the kernel skips step two after one ballot.
// extract_block_settle (waves with a candidate; every lane of such a wave): what round 3 computed for every block - flat
// index 4 exactly as pocketfft has it (for integer pixels it is a multiple of 1/8: c / delta sits EXACTLY on a tie in 1 block of
// 8 delta, SURVEY N6, and only the reference's own float32 sequence says which way it falls; its bit is replaced), and the
// per-block margin  u' (KDC mean + KE ||X - mean||_2) / delta  from the pixel sum alone (see SVS_TIE2_*).  Returns true when
// a coefficient other than 4 is inside the margin of a tie: the caller then redoes the block with the pocketfft-identical
// transform (8 lanes per block on the device, extract_block_exact on the host emulation).  For a non-candidate block the
// result is false and the bits do not change - by the bound - so taking step two per wave (device) or per block (host
// emulation) gives the same stream.
template <int U, int QM, int NFIX = 0>
SVS_HD bool extract_block_cheap(const uint32_t (&rx)[8], const uint32_t (&ry)[8], uint32_t n_rt, const QimParams &qp,
                                uint32_t &hi, uint32_t &lo, float &off) {
    const uint32_t n = NFIX ? (uint32_t)NFIX : n_rt;
    float D[U][8];
    forward_rows<U>(rx, ry, D);
    hi = 0;
    lo = 0;
    off = 0.0f;        // largest |t - round(t)| over the used coefficients other than flat index 4 (0.5 = exactly on a tie)
    float d4 = 0.0f;   // t - round(t) of flat index 4
    const float kMagic = 12582912.0f;   // 1.5 * 2^23
#pragma unroll
    for (int k = 8 * U - 1; k >= 1; --k) {
        if ((uint32_t)k <= n) {  // wave-uniform
            const float t = D[k >> 3][k & 7] * qp.inv_delta_f;
            const float m = t + kMagic;
            const float d = t - (m - kMagic);
            if (k == 4) d4 = d;
            else off = fmaxf(off, fabsf(d));
            const uint32_t mb = __builtin_bit_cast(uint32_t, m);
            if (k - 1 < 32) hi = (mb << 31) | (hi >> 1);   // v_alignbit_b32: bit of coefficient i ends at 31 - i
            else lo = (mb << 31) | (lo >> 1);
        }
    }
    return !(fmaxf(off, fabsf(d4)) < 0.5f - qp.tie2_max);
}

template <int QM>
SVS_HD bool extract_block_settle(const uint32_t (&rx)[8], const uint32_t (&ry)[8], uint32_t n, const QimParams &qp, uint32_t &hi,
                                 float off) {
    float a0[4], b0[4], V0[8];
    vertical_u1_packed(rx, a0);      // row 0 of the vertical pass: fl(colsum * a(0)) - pocketfft's own values
    vertical_u1_packed(ry, b0);
#pragma unroll
    for (int x = 0; x < 4; ++x) { V0[x] = a0[x]; V0[4 + x] = b0[x]; }
    ForwardSide side;
    forward_side(V0, &side);
    if (n >= 4) {
        const uint32_t bit = (uint32_t)quant_index<QM>(side.c4, qp) & 1u;
        hi = (hi & ~(1u << 28)) | (bit << 28);   // i = 3 -> bit 31 - 3
    }
    // The per-block bound wants S = sum of the pixels and their energy Q = sum p^2 through 64 Q - S^2; pixels are at most
    // 255, so Q <= 255 S and 64 Q - S^2 <= S (16320 - S): no pass over the pixels (S = the vertical pass's DC row summed, over a(0)).
    const float S = side.v0_sum * (1.0000005f / SVS_A0);
    const float spread = guard_sqrt(fmaxf(S * (16320.0f - S), 0.0f)) * 1.000001f;
    const float c00 = side.v0_sum * (SVS_A0 * 1.000001f);     // the DC coefficient (a few roundings from fdct8's own value)
    const float margin = fmaf(qp.tie2_sum, S, fmaf(qp.tie2_resid, spread, fmaf(c00, qp.tie2_c00, 0x1p-20f)));
    return off >= 0.5f - margin;
}

// both steps for one block (host emulation; the kernels put a wave ballot between them)
template <int U, int QM, int NFIX = 0>
SVS_HD bool extract_block(const uint32_t (&rx)[8], const uint32_t (&ry)[8], uint32_t n_rt, const QimParams &qp,
                          uint32_t &hi, uint32_t &lo) {
    float off;
    if (!extract_block_cheap<U, QM, NFIX>(rx, ry, n_rt, qp, hi, lo, off)) return false;
    return extract_block_settle<QM>(rx, ry, NFIX ? (uint32_t)NFIX : n_rt, qp, hi, off);
}

// =====================================================================================================
// EXACT mode: bit-for-bit the float32 arithmetic of scipy.fftpack.dct/idct(norm='ortho') for length 8.
//
// scipy's DCT is pocketfft (C++, `T_dcst23<float>::exec`; scipy unpinned in the reference, vectors
// generated with scipy 1.15.3).  For N = 8 its published algorithm is: DCT-II = pre-butterfly ->
// BACKWARD real FFT of length 8 (radix passes radb2(ido=4), radb4(ido=1), factors [2,4]) scaled by
// fct = 1/sqrt(2N) = 0.25 -> twiddle post-pass with cos((k+1)pi/16) -> c[0] *= sqrt(2)/2;  DCT-III is
// the mirror image with the FORWARD real FFT (radf4(ido=1), radf2(ido=4)).  Every operation below is one
// IEEE float32 add/sub/mul in pocketfft's order (no FMA: build with -ffp-contract=off), so the results
// are bit-identical to scipy's - checked on random and integer vectors in tests/test_exact_mode_cpu.py and,
// through the whole operator, against every golden vector (stego PIXELS included).
// With these transforms the operator reproduces the reference's rounding-noise artefacts too
// (SURVEY N4/N6): exact .5 ties, 128 -> 127 on untouched flat blocks, delta <= 0 round trips.
// =====================================================================================================
namespace pf {
// float(cos((i+1) pi / 16)), i = 0..6: pocketfft's `twiddle[i]` for N = 8
#define SVS_PF_T0 0x1.f6297cp-1f
#define SVS_PF_T1 0x1.d906bcp-1f
#define SVS_PF_T2 0x1.a9b662p-1f
#define SVS_PF_T3 0x1.6a09e6p-1f
#define SVS_PF_T4 0x1.1c73b4p-1f
#define SVS_PF_T5 0x1.87de2ap-2f
#define SVS_PF_T6 0x1.8f8b84p-3f
#define SVS_PF_W 0x1.6a09e6p-1f      // cos(2pi/8) = sin(2pi/8) as float: the radix-2 pass twiddle
#define SVS_PF_SQRT2 0x1.6a09e6p+0f  // float(sqrt 2)

// Exactness-preserving rewrites used below (each keeps every result bit-identical to pocketfft's sequence):
//   * a multiplication by a power of two is exact, so it commutes with the roundings around it: the
//     `* fct` (0.25) after the FFT and the `0.5 *` of the DCT-II post-pass are folded into the twiddle
//     constants of the one multiplication every value passes through anyway (T/8, T/4 are exact floats);
//   * fl(a + fl(2*b)) == fmaf(2, b, a): pocketfft's `2*x` followed by an add/sub is one FMA.
// They remove 20 of 78 (DCT-II) and 8 of 66 (DCT-III) operations.  (Subnormal intermediates, which would
// break the first identity, cannot occur for pixel-derived data: non-zero values stay above 2^-40.)

// Every function below is written once for T = float (one line of 8 values) and T = f32x2 (two independent lines,
// component k of every value belonging to line k).  On gfx950 the two-line form compiles to packed-FP32 instructions
// (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32: two IEEE-754 single operations per issue slot), each component rounding
// exactly like the scalar operation - so the results stay bit-identical while the instruction count halves.
typedef float f32x2 __attribute__((vector_size(8)));

template <class T> SVS_HD T splat(float v);
template <> SVS_HD float splat<float>(float v) { return v; }
template <> SVS_HD f32x2 splat<f32x2>(float v) { const f32x2 r = {v, v}; return r; }

SVS_HD float fma_t(float a, float b, float c) { return fmaf(a, b, c); }
SVS_HD f32x2 fma_t(f32x2 a, f32x2 b, f32x2 c) {
#if defined(__has_builtin)
#if __has_builtin(__builtin_elementwise_fma)
#define SVS_HAVE_ELEMENTWISE_FMA 1
#endif
#endif
#if defined(SVS_HAVE_ELEMENTWISE_FMA)
    return __builtin_elementwise_fma(a, b, c);
#else
    const f32x2 r = {fmaf(a[0], b[0], c[0]), fmaf(a[1], b[1], c[1])};
    return r;
#endif
}

// backward real FFT (halfcomplex -> real) of length 8, UNSCALED (the caller folds fct)
template <class T>
SVS_HD void rfft8_backward(const T (&c)[8], T (&o)[8]) {
    const T W = splat<T>(SVS_PF_W), two = splat<T>(2.0f), mtwo = splat<T>(-2.0f);
    // radb2, ido = 4, l1 = 1   (h3 = 2*c3 and h7 = -2*c4 are consumed as FMAs below)
    const T h0 = c[0] + c[7], h4 = c[0] - c[7];
    const T h1 = c[1] + c[5], tr2 = c[1] - c[5];
    const T ti2 = c[2] + c[6], h2 = c[2] - c[6];
    const T h6 = W * ti2 + W * tr2;
    const T h5 = W * tr2 - W * ti2;
    // radb4, ido = 1, l1 = 2:  a = h[4k] + h[4k+3], b = h[4k] - h[4k+3], out = a +- 2 h[4k+1], b +- 2 h[4k+2]
    const T a0 = fma_t(two, c[3], h0), b0 = fma_t(mtwo, c[3], h0);
    o[0] = fma_t(two, h1, a0);
    o[4] = fma_t(mtwo, h1, a0);
    o[6] = fma_t(two, h2, b0);
    o[2] = fma_t(mtwo, h2, b0);
    const T a1 = fma_t(mtwo, c[4], h4), b1 = fma_t(two, c[4], h4);
    o[1] = fma_t(two, h5, a1);
    o[5] = fma_t(mtwo, h5, a1);
    o[7] = fma_t(two, h6, b1);
    o[3] = fma_t(mtwo, h6, b1);
}

// forward real FFT (real -> halfcomplex) of length 8, UNSCALED (the caller folds fct)
template <class T>
SVS_HD void rfft8_forward(const T (&c)[8], T (&o)[8]) {
    const T W = splat<T>(SVS_PF_W);
    T y[8];
    // radf4, ido = 1, l1 = 2
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const T tr1 = c[k + 6] + c[k + 2];
        y[4 * k + 2] = c[k + 6] - c[k + 2];
        const T tr2 = c[k] + c[k + 4];
        y[4 * k + 1] = c[k] - c[k + 4];
        y[4 * k] = tr2 + tr1;
        y[4 * k + 3] = tr2 - tr1;
    }
    // radf2, ido = 4, l1 = 1
    const T tr2 = W * y[5] + W * y[6];
    const T ti2 = W * y[6] - W * y[5];
    o[0] = y[0] + y[4];
    o[7] = y[0] - y[4];
    o[4] = -y[7];
    o[3] = y[3];
    o[1] = y[1] + tr2;
    o[5] = y[1] - tr2;
    o[2] = ti2 + y[2];
    o[6] = ti2 - y[2];
}

// scipy.fftpack.dct(x, type=2, norm='ortho') for 8 float32 values
template <class T>
SVS_HD void dct2_8(const T (&x)[8], T (&X)[8]) {
    T c[8];
    c[0] = x[0] * splat<T>(2.0f);
    c[7] = x[7] * splat<T>(2.0f);
#pragma unroll
    for (int k = 1; k < 7; k += 2) {  // MPINPLACE(c[k+1], c[k])
        c[k + 1] = x[k + 1] - x[k];
        c[k] = x[k] + x[k + 1];
    }
    T r[8];
    rfft8_backward(c, r);
    // post-pass: pocketfft computes 0.5*(t1 +- t2) with t = T*(0.25 r) +- T*(0.25 r); here T/8 carries both scalings
    {
        const T t1 = splat<T>(SVS_PF_T0 * 0.125f) * r[7] + splat<T>(SVS_PF_T6 * 0.125f) * r[1];
        const T t2 = splat<T>(SVS_PF_T0 * 0.125f) * r[1] - splat<T>(SVS_PF_T6 * 0.125f) * r[7];
        X[1] = t1 + t2;
        X[7] = t1 - t2;
    }
    {
        const T t1 = splat<T>(SVS_PF_T1 * 0.125f) * r[6] + splat<T>(SVS_PF_T5 * 0.125f) * r[2];
        const T t2 = splat<T>(SVS_PF_T1 * 0.125f) * r[2] - splat<T>(SVS_PF_T5 * 0.125f) * r[6];
        X[2] = t1 + t2;
        X[6] = t1 - t2;
    }
    {
        const T t1 = splat<T>(SVS_PF_T2 * 0.125f) * r[5] + splat<T>(SVS_PF_T4 * 0.125f) * r[3];
        const T t2 = splat<T>(SVS_PF_T2 * 0.125f) * r[3] - splat<T>(SVS_PF_T4 * 0.125f) * r[5];
        X[3] = t1 + t2;
        X[5] = t1 - t2;
    }
    X[4] = r[4] * splat<T>(SVS_PF_T3 * 0.25f);
    X[0] = r[0] * splat<T>(SVS_PF_SQRT2 * 0.125f);
}

// scipy.fftpack.idct(X, type=2, norm='ortho') (= DCT-III) for 8 float32 values
template <class T>
SVS_HD void dct3_8(const T (&X)[8], T (&x)[8]) {
    T c[8];  // pre-pass with the FFT's fct = 0.25 folded into the constants
    c[0] = X[0] * splat<T>(SVS_PF_SQRT2 * 0.25f);
    {
        const T t1 = X[1] + X[7], t2 = X[1] - X[7];
        c[1] = splat<T>(SVS_PF_T0 * 0.25f) * t2 + splat<T>(SVS_PF_T6 * 0.25f) * t1;
        c[7] = splat<T>(SVS_PF_T0 * 0.25f) * t1 - splat<T>(SVS_PF_T6 * 0.25f) * t2;
    }
    {
        const T t1 = X[2] + X[6], t2 = X[2] - X[6];
        c[2] = splat<T>(SVS_PF_T1 * 0.25f) * t2 + splat<T>(SVS_PF_T5 * 0.25f) * t1;
        c[6] = splat<T>(SVS_PF_T1 * 0.25f) * t1 - splat<T>(SVS_PF_T5 * 0.25f) * t2;
    }
    {
        const T t1 = X[3] + X[5], t2 = X[3] - X[5];
        c[3] = splat<T>(SVS_PF_T2 * 0.25f) * t2 + splat<T>(SVS_PF_T4 * 0.25f) * t1;
        c[5] = splat<T>(SVS_PF_T2 * 0.25f) * t1 - splat<T>(SVS_PF_T4 * 0.25f) * t2;
    }
    c[4] = X[4] * splat<T>(SVS_PF_T3 * 0.5f);  // 2 * T3 * 0.25
    T r[8];
    rfft8_forward(c, r);
    x[0] = r[0];
    x[7] = r[7];
#pragma unroll
    for (int k = 1; k < 7; k += 2) {  // MPINPLACE(c[k], c[k+1])
        x[k] = r[k] - r[k + 1];
        x[k + 1] = r[k + 1] + r[k];
    }
}
}  // namespace pf

// all 64 coefficients of a block, pocketfft arithmetic: vertical transform first (axis 0), then
// horizontal (config_and_setup.py:135).  Coefficients the caller never reads are dead code.
SVS_HD void forward_exact(const uint32_t (&rx)[8], const uint32_t (&ry)[8], float (&D)[8][8]) {
    float V[8][8];
#define SVS_COL(X, W, B)                                                                \
    {                                                                                   \
        const float col[8] = {ubyte_to_float<B>(W[0]), ubyte_to_float<B>(W[1]),         \
                              ubyte_to_float<B>(W[2]), ubyte_to_float<B>(W[3]),         \
                              ubyte_to_float<B>(W[4]), ubyte_to_float<B>(W[5]),         \
                              ubyte_to_float<B>(W[6]), ubyte_to_float<B>(W[7])};        \
        float out[8];                                                                   \
        pf::dct2_8(col, out);                                                           \
        _Pragma("unroll") for (int u = 0; u < 8; ++u) V[u][X] = out[u];                 \
    }
    SVS_COL(0, rx, 0) SVS_COL(1, rx, 1) SVS_COL(2, rx, 2) SVS_COL(3, rx, 3)
    SVS_COL(4, ry, 0) SVS_COL(5, ry, 1) SVS_COL(6, ry, 2) SVS_COL(7, ry, 3)
#undef SVS_COL
#pragma unroll
    for (int u = 0; u < 8; ++u) pf::dct2_8(V[u], D[u]);
}

// The same 64 coefficients, two lines per operation: the vertical pass transforms column pairs (2p, 2p+1), the
// horizontal pass row pairs (2q, 2q+1); D2[q][v] = (D[2q][v], D[2q+1][v]).  In between, the 2x2 sub-blocks are
// transposed in registers.
SVS_HD void forward_exact_paired(const uint32_t (&rx)[8], const uint32_t (&ry)[8], pf::f32x2 (&D2)[4][8]) {
    using pf::f32x2;
    f32x2 V2[4][8];  // V2[p][u] = (V[u][2p], V[u][2p+1])
#define SVS_COLPAIR(P, W, B0, B1)                                                       \
    {                                                                                   \
        f32x2 col[8];                                                                   \
        _Pragma("unroll") for (int r = 0; r < 8; ++r) {                                 \
            const f32x2 t = {ubyte_to_float<B0>(W[r]), ubyte_to_float<B1>(W[r])};       \
            col[r] = t;                                                                 \
        }                                                                               \
        pf::dct2_8(col, V2[P]);                                                         \
    }
    SVS_COLPAIR(0, rx, 0, 1) SVS_COLPAIR(1, rx, 2, 3) SVS_COLPAIR(2, ry, 0, 1) SVS_COLPAIR(3, ry, 2, 3)
#undef SVS_COLPAIR
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f32x2 in[8];
#pragma unroll
        for (int p2 = 0; p2 < 4; ++p2) {
            const f32x2 a = V2[p2][2 * q], b = V2[p2][2 * q + 1];
            const f32x2 e = {a[0], b[0]}, o = {a[1], b[1]};
            in[2 * p2] = e;
            in[2 * p2 + 1] = o;
        }
        pf::dct2_8(in, D2[q]);
    }
}

// EXACT embed of one block: full DCT -> QIM on 1..n (first nb take payload) -> full IDCT (vertical
// first, :168) -> clip + truncate (:171).  A block that is entered is always round-tripped, even when
// nothing is changed (delta <= 0, n = 0): that is what produces the reference's x -> x-1 artefacts.
// The 64 coefficients of a CONSTANT block (all pixels = v), pocketfft arithmetic, without transforming 16 lines: every
// column is the same vector (v, .., v), so one dct2_8 gives the whole vertical pass; its AC outputs are exact zeros
// (differences of equal values, products and sums of zeros), so rows 1..7 stay zero through the horizontal pass, and row 0 is
// again a constant vector.  Two transforms instead of sixteen, same bits (the sign of a zero coefficient cannot reach a
// pixel: x + (-0) = x, and an exactly-zero pixel truncates to 0 either way).
SVS_HD void forward_exact_paired_constant(float v, pf::f32x2 (&D2)[4][8]) {
    using pf::f32x2;
    float col[8], V[8], row[8], D0[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) col[r] = v;
    pf::dct2_8(col, V);       // V[0] = the column's DC term, V[1..7] = 0
#pragma unroll
    for (int x = 0; x < 8; ++x) row[x] = V[0];
    pf::dct2_8(row, D0);      // D0[0] = DC, D0[1..7] = 0
    const f32x2 zero = {0.0f, 0.0f};
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int c = 0; c < 8; ++c) D2[q][c] = zero;
    D2[0][0][0] = D0[0];
}

// `constant_block`: the caller knows (wave-uniformly) that all 64 pixels are equal - the forward pass is then the two-line
// shortcut above (host emulation of flat content; the device replay transforms every block in full)
template <int U, int QM, int RULE>
SVS_HD void qim_exact_paired(pf::f32x2 (&D2)[4][8], uint32_t n, uint32_t nb, uint32_t hi, uint32_t lo, const QimRule &qp) {
#pragma unroll
    for (int k = 1; k < 8 * U; ++k) {
        if ((uint32_t)k <= n) {  // wave-uniform
            const int i = k - 1;
            const int bit = (int)window_bit(hi, lo, i);
            const float c = D2[k >> 4][k & 7][(k >> 3) & 1];
            const float cn = qim_target<QM, RULE>(c, bit, qp, qim_band<RULE>(qp, (uint32_t)k));
            D2[k >> 4][k & 7][(k >> 3) & 1] = ((uint32_t)i < nb) ? cn : c;
        }
    }
}

// The same loop for a coefficient selection (CoeffTable): coefficient k carries stream slot sel.slot(k) of the block when that
// is below sel.count (0xFF is not), and takes payload while the slot is inside the block's budget nb.  k stays a compile-time
// index; the slot is wave-uniform.  The prefix table 1..n gives qim_exact_paired's result.  SVS_MINMOVE: the band is that of
// the coefficient's flat index k, whatever slot it carries.
template <int QM, int RULE>
SVS_HD void qim_exact_selected(pf::f32x2 (&D2)[4][8], const CoeffTable &sel, uint32_t nb, uint32_t hi, uint32_t lo,
                               const QimRule &qp) {
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        const uint32_t s = sel.slot(k);
        if (s < sel.count) {  // wave-uniform
            const int bit = (int)window_bit_at(hi, lo, s);
            const float c = D2[k >> 4][k & 7][(k >> 3) & 1];
            const float cn = qim_target<QM, RULE>(c, bit, qp, qim_band<RULE>(qp, (uint32_t)k));
            D2[k >> 4][k & 7][(k >> 3) & 1] = (s < nb) ? cn : c;
        }
    }
}

// The dithered calls: the same loop with dithered_target and the block's s_b instead of qim_target - the hash and two more float
// operations, for the coefficients behind the wave-uniform slot test only.  A dithered call without a selection brings the
// prefix table (make_prefix_table), so this one loop serves both.  Written as a recursion over K: 63 copies of this larger body
// are more than the compiler unrolls on a pragma, and a loop left rolled indexes the table and the coefficients at run time
// (the table went to 72 bytes of scratch).
template <int QM, int RULE, int K = 1>
SVS_HD void qim_exact_selected_dithered(pf::f32x2 (&D2)[4][8], const CoeffTable &sel, uint32_t nb, uint32_t hi, uint32_t lo,
                                        const QimRule &qp, uint32_t s_b) {
    const uint32_t s = sel.slot(K);
    if (s < sel.count) {  // wave-uniform
        const float c = D2[K >> 4][K & 7][(K >> 3) & 1];
        const float cn = dithered_target<QM, RULE>(c, (int)window_bit_at(hi, lo, s), qp, (uint32_t)K, s_b);
        D2[K >> 4][K & 7][(K >> 3) & 1] = (s < nb) ? cn : c;
    }
    if constexpr (K < 63) qim_exact_selected_dithered<QM, RULE, K + 1>(D2, sel, nb, hi, lo, qp, s_b);
}

// ---------------------------------------------------------------------------------------------------------------------
// Per-coefficient steps (svs_stepped_embed* / svs_stepped_extract*, include/svsdct.h): coefficient k is quantised with its own
// step dk = (float)delta[k] instead of the call's delta.  A format, as the dither's: every float step is one IEEE float32
// operation (build with -ffp-contract=off), in this order on host and device, whatever quantiser mode the holding kernel has:
//   q = (int)rintf(c / dk)  (the division itself);  the value written for index t is (float)t * dk  (exact: |t dk| < 2^24)
//   reference rule: force_parity;  SVS_NEAREST: nearest_parity with c0 = (float)q * dk;
//   SVS_MINMOVE: the band of half-width r_k = max(0, 0.5f * dk - MARGIN[k]) around nearest_parity's lattice point
//   dither: d = r * dk (dither_value with dk), the rule on c - d, moved back by d; a coefficient the rule leaves alone keeps c
// With every delta[k] = D the values are those of the call with delta = D (quant_index's shortcut is the division's result by
// construction, and (float)(0.5 * D) == 0.5f * D).
// ---------------------------------------------------------------------------------------------------------------------
template <int RULE>
SVS_HD float stepped_target(float c, int bit, float dk, uint32_t k) {
    const int q = quant_index_by_division(c, dk);
    int t;
    if constexpr (RULE == RULE_REFERENCE) {
        t = force_parity(q, bit);
    } else {
        const float c0 = (float)q * dk;
        const int dir = c > c0 ? 1 : (c < c0 ? -1 : 2 * bit - 1);
        t = q + (((q ^ bit) & 1) ? dir : 0);
    }
    const float ct = (float)t * dk;
    if constexpr (RULE == RULE_MINMOVE) return minmove_clamp(c, ct, fmaxf(0.0f, 0.5f * dk - minmove_margin(k)));
    else return ct;
}

// ... under a dither (DITH), as dithered_target
template <int RULE, bool DITH>
SVS_HD float stepped_value(float c, int bit, float dk, uint32_t k, uint32_t s_b) {
    if constexpr (DITH) {
        const float d = dither_value(s_b, k, dk);
        const float cp = c - d;
        const float cn = stepped_target<RULE>(cp, bit, dk, k);
        return __builtin_bit_cast(uint32_t, cn) == __builtin_bit_cast(uint32_t, cp) ? c : cn + d;
    } else {
        return stepped_target<RULE>(c, bit, dk, k);
    }
}

// The selected loop with a step per coefficient (a recursion over K, as qim_exact_selected_dithered and for its reason).  `sel` is
// never empty: the call's selection, or the prefix table of n_ac.  steps.step(K) is read here, behind the slot test.
template <int RULE, bool DITH, int K = 1>
SVS_HD void qim_stepped_selected(pf::f32x2 (&D2)[4][8], const CoeffTable &sel, const StepArgs &steps, uint32_t nb, uint32_t hi,
                                 uint32_t lo, uint32_t s_b) {
    const uint32_t s = sel.slot(K);
    if (s < sel.count) {  // wave-uniform
        const float c = D2[K >> 4][K & 7][(K >> 3) & 1];
        const float cn = stepped_value<RULE, DITH>(c, (int)window_bit_at(hi, lo, s), steps.step(K), (uint32_t)K, s_b);
        D2[K >> 4][K & 7][(K >> 3) & 1] = (s < nb) ? cn : c;
    }
    if constexpr (K < 63) qim_stepped_selected<RULE, DITH, K + 1>(D2, sel, steps, nb, hi, lo, s_b);
}

// The pocketfft-identical inverse of all 64 coefficients (vertical first, :168) into the block's row dwords; every byte is
// overwritten (the input rows are dead).  RNE false: np.uint8(np.clip(v, 0, 255)), clip then truncate (:171) - the embed.
// RNE true: round half to even, then saturate - what a decoder does (the requantisation channel).
template <bool RNE>
SVS_HD void inverse_exact_paired(const pf::f32x2 (&D2)[4][8], uint32_t (&rx)[8], uint32_t (&ry)[8]) {
    using pf::f32x2;
    f32x2 P2[4][8];  // vertical inverse of coefficient-column pairs: P2[p][y] = (P[y][2p], P[y][2p+1])
#pragma unroll
    for (int p2 = 0; p2 < 4; ++p2) {
        f32x2 col[8];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x2 a = D2[q][2 * p2], b = D2[q][2 * p2 + 1];
            const f32x2 e = {a[0], b[0]}, o = {a[1], b[1]};
            col[2 * q] = e;
            col[2 * q + 1] = o;
        }
        pf::dct3_8(col, P2[p2]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {  // horizontal inverse of pixel rows 2q, 2q+1
        f32x2 in[8], px[8];
#pragma unroll
        for (int p2 = 0; p2 < 4; ++p2) {
            const f32x2 a = P2[p2][2 * q], b = P2[p2][2 * q + 1];
            const f32x2 e = {a[0], b[0]}, o = {a[1], b[1]};
            in[2 * p2] = e;
            in[2 * p2 + 1] = o;
        }
        pf::dct3_8(in, px);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if constexpr (RNE) {
                uint32_t a = 0u, b = 0u;
                a = put_pixel_rne<0>(px[0][k], a); a = put_pixel_rne<1>(px[1][k], a);
                a = put_pixel_rne<2>(px[2][k], a); a = put_pixel_rne<3>(px[3][k], a);
                b = put_pixel_rne<0>(px[4][k], b); b = put_pixel_rne<1>(px[5][k], b);
                b = put_pixel_rne<2>(px[6][k], b); b = put_pixel_rne<3>(px[7][k], b);
                rx[2 * q + k] = a;
                ry[2 * q + k] = b;
            } else {
                store_row_trunc(px[0][k], px[1][k], px[2][k], px[3][k], px[4][k], px[5][k], px[6][k], px[7][k], rx[2 * q + k],
                                ry[2 * q + k]);
            }
        }
    }
}

// `sel`: NULL (the row-major prefix 1..n) or a selection; then n is not read, nb counts slots of the selection.  The callers
// pass a compile-time NULL or the address of a by-value kernel argument, so the test folds on either side.
// DITH (the dithered calls; U = 8, and `sel` is never NULL: the call's selection or the prefix table of n): the selected loop
// with the block's s_b (dither_block_seed); everything around it is the same.
template <int U, int QM, bool DITH = false>
SVS_HD void embed_block_exact(uint32_t (&rx)[8], uint32_t (&ry)[8], uint32_t n, uint32_t nb, uint32_t hi, uint32_t lo,
                              const QimRule &qp, bool constant_block = false, const CoeffTable *sel = nullptr, uint32_t s_b = 0u) {
    using pf::f32x2;
    static_assert(!DITH || U == 8, "a dithered call covers all eight coefficient rows");
    f32x2 D2[4][8];
    if (constant_block) forward_exact_paired_constant(ubyte_to_float<0>(rx[0]), D2);
    else forward_exact_paired(rx, ry, D2);
    if constexpr (DITH) {
        if (qp.kind == (uint32_t)RULE_MINMOVE) qim_exact_selected_dithered<QM, RULE_MINMOVE>(D2, *sel, nb, hi, lo, qp, s_b);
        else if (qp.kind == (uint32_t)RULE_NEAREST) qim_exact_selected_dithered<QM, RULE_NEAREST>(D2, *sel, nb, hi, lo, qp, s_b);
        else qim_exact_selected_dithered<QM, RULE_REFERENCE>(D2, *sel, nb, hi, lo, qp, s_b);
    } else if (sel) {
        if (qp.kind == (uint32_t)RULE_MINMOVE) qim_exact_selected<QM, RULE_MINMOVE>(D2, *sel, nb, hi, lo, qp);
        else if (qp.kind == (uint32_t)RULE_NEAREST) qim_exact_selected<QM, RULE_NEAREST>(D2, *sel, nb, hi, lo, qp);
        else qim_exact_selected<QM, RULE_REFERENCE>(D2, *sel, nb, hi, lo, qp);
    } else if (qp.kind == (uint32_t)RULE_MINMOVE) qim_exact_paired<U, QM, RULE_MINMOVE>(D2, n, nb, hi, lo, qp);
    else if (qp.kind == (uint32_t)RULE_NEAREST) qim_exact_paired<U, QM, RULE_NEAREST>(D2, n, nb, hi, lo, qp);
    else qim_exact_paired<U, QM, RULE_REFERENCE>(D2, n, nb, hi, lo, qp);
    inverse_exact_paired<false>(D2, rx, ry);
}

// The same round trip with a step per coefficient (svs_stepped_embed*): the stepped loop in place of the quantiser's; `kind` is
// a QimRuleKind, a constant on every side of the kernel's branch as QimRule::kind is.
template <bool DITH>
SVS_HD void embed_block_stepped(uint32_t (&rx)[8], uint32_t (&ry)[8], uint32_t nb, uint32_t hi, uint32_t lo, uint32_t kind,
                                const CoeffTable &sel, const StepArgs &steps, uint32_t s_b = 0u) {
    pf::f32x2 D2[4][8];
    forward_exact_paired(rx, ry, D2);
    if (kind == (uint32_t)RULE_MINMOVE) qim_stepped_selected<RULE_MINMOVE, DITH>(D2, sel, steps, nb, hi, lo, s_b);
    else if (kind == (uint32_t)RULE_NEAREST) qim_stepped_selected<RULE_NEAREST, DITH>(D2, sel, steps, nb, hi, lo, s_b);
    else qim_stepped_selected<RULE_REFERENCE, DITH>(D2, sel, steps, nb, hi, lo, s_b);
    inverse_exact_paired<false>(D2, rx, ry);
}

// ---------------------------------------------------------------------------------------------------------------------
// Matrix embedding (svs_matrix_embed* / svs_matrix_extract*, include/svsdct.h "matrix embedding"): a block's k message bits are
// the syndrome of the parities of its n = 2^k - 1 selected coefficients under the (n, k) Hamming code, so the sender flips at
// most one parity - or, with the pair search, the cheaper of one or two.  A stepped call: the parity is svs_stepped_extract*'s
// verdict, and every selected coefficient is written by the stepped rule with its own parity, flipped where the code says so.
// The parity window is the payload window's form: slot t at bit 63 - t of hi:lo.
// ---------------------------------------------------------------------------------------------------------------------
// bits of the window half (LOW: slots 32..62) whose slot t has bit I of t + 1 set
constexpr uint32_t matrix_mask_bits(int i, bool low) {
    uint32_t m = 0;
    for (int t = low ? 32 : 0; t < (low ? 63 : 32); ++t)
        if (((t + 1) >> i) & 1) m |= 1u << ((63 - t) & 31);
    return m;
}

template <int I = 0>
SVS_HD uint32_t matrix_syndrome(uint32_t hi, uint32_t lo) {   // XOR of t + 1 over the set slots t: six masked parities
    constexpr uint32_t MH = matrix_mask_bits(I, false), ML = matrix_mask_bits(I, true);
    const uint32_t bit = ((uint32_t)(__builtin_popcount(hi & MH) + __builtin_popcount(lo & ML)) & 1u) << I;
    if constexpr (I < 5) return bit | matrix_syndrome<I + 1>(hi, lo);
    else return bit;
}

// the message value of a block with a budget of nb <= 6 bits: stream bit i (bit 31 - i of the payload window) is bit i of m
SVS_HD uint32_t matrix_message(uint32_t hi, uint32_t nb) {
    uint32_t m = 0;
    for (int i = 0; i < 6; ++i) m |= ((hi >> (31 - i)) & 1u) << i;
    return m & ((1u << nb) - 1u);
}

// ... and back: the syndrome as the block's k stream bits, MSB first in hi
SVS_HD void matrix_fold(uint32_t &hi, uint32_t &lo) {
    const uint32_t S = matrix_syndrome(hi, lo);
    hi = 0;
    for (int i = 0; i < 6; ++i) hi |= ((S >> i) & 1u) << (31 - i);
    lo = 0;
}

// One pass over the selected coefficients of a block in embed_block_exact's paired layout.  For slot s of coefficient K, with
// x = c - d the rule's input: the parity p = rintf(x / dk) & 1 (stepped_parities' verdict) goes into the window hi:lo; the value
// the stepped rule writes for the bit p (stepped_value's, dither and "leave c alone" included) goes into D2; the value it writes
// for the bit p ^ 1 goes to flipped[s * stride]; and with COSTS the pair search's cost of flipping the slot goes to
// e[s * stride]: stay = rule(x, p), flip = rule(x, p ^ 1), a = flip - x; b = stay - x; e = a a - b b, one float32 operation a step.
// `flipped` and `e` are the lane's own columns of its wave's tile (device: dynamic LDS, stride 64 - written here at a wave-uniform
// slot, read back at a per-lane one).  The rule is a wave-uniform run-time branch per coefficient, not three loops: every read of
// the tables through the kernel's arguments counts against the compiler's limit for reading them in place (StepArgs::quad_here).
template <bool DITH, bool COSTS, int K = 1>
SVS_HD void matrix_pass(pf::f32x2 (&D2)[4][8], const CoeffTable &sel, const StepArgs &steps, uint32_t kind, uint32_t &hi, uint32_t &lo,
                        uint32_t s_b, float *flipped, float *e, uint32_t stride) {
    const uint32_t s = sel.slot(K);
    if (s < sel.count) {  // wave-uniform
        const float dk = steps.step(K);
        const float c = D2[K >> 4][K & 7][(K >> 3) & 1];
        float d = 0.0f, x = c;
        if constexpr (DITH) {
            d = dither_value(s_b, (uint32_t)K, dk);
            x = c - d;
        }
        const int p = quant_index_by_division(x, dk) & 1;
        const uint32_t bit = (uint32_t)p << ((31u - s) & 31u);
        if (s < 32u) hi |= bit;
        else lo |= bit;
        float stay, flip;
        if (kind == (uint32_t)RULE_MINMOVE) {
            stay = stepped_target<RULE_MINMOVE>(x, p, dk, (uint32_t)K);
            flip = stepped_target<RULE_MINMOVE>(x, p ^ 1, dk, (uint32_t)K);
        } else if (kind == (uint32_t)RULE_NEAREST) {
            stay = stepped_target<RULE_NEAREST>(x, p, dk, (uint32_t)K);
            flip = stepped_target<RULE_NEAREST>(x, p ^ 1, dk, (uint32_t)K);
        } else {
            stay = stepped_target<RULE_REFERENCE>(x, p, dk, (uint32_t)K);
            flip = stepped_target<RULE_REFERENCE>(x, p ^ 1, dk, (uint32_t)K);
        }
        if constexpr (COSTS) {
            const float a = flip - x, b = stay - x;
            const float aa = a * a, bb = b * b;
            e[s * stride] = aa - bb;
        }
        if constexpr (DITH) {   // as stepped_value: a coefficient the rule leaves alone keeps c exactly
            stay = __builtin_bit_cast(uint32_t, stay) == __builtin_bit_cast(uint32_t, x) ? c : stay + d;
            flip = __builtin_bit_cast(uint32_t, flip) == __builtin_bit_cast(uint32_t, x) ? c : flip + d;
        }
        D2[K >> 4][K & 7][(K >> 3) & 1] = stay;
        flipped[s * stride] = flip;
    }
    if constexpr (K < 63) matrix_pass<DITH, COSTS, K + 1>(D2, sel, steps, kind, hi, lo, s_b, flipped, e, stride);
}

// The flip set of a block whose syndrome misses its message by j (1..n) under the pair search: the single slot j - 1, or the
// first pair of slots {a - 1, (a ^ j) - 1}, a = 1..n in this order with a < a ^ j, whose summed cost is strictly below the best so
// far.  fb = 64: no second slot.
SVS_HD void matrix_search(uint32_t j, uint32_t n, const float *e, uint32_t stride, uint32_t &fa, uint32_t &fb) {
    float best = e[(j - 1u) * stride];
    fa = j - 1u;
    fb = 64u;
    for (uint32_t a = 1; a <= n; ++a) {
        const uint32_t b = a ^ j;
        if (a < b) {
            const float v = e[(a - 1u) * stride] + e[(b - 1u) * stride];
            if (v < best) { best = v; fa = a - 1u; fb = b - 1u; }
        }
    }
}

// the coefficients of the slots fa and fb (64: none) take the values va and vb
template <int K = 1>
SVS_HD void matrix_apply(pf::f32x2 (&D2)[4][8], const CoeffTable &sel, uint32_t fa, uint32_t fb, float va, float vb) {
    const uint32_t s = sel.slot(K);
    if (s < sel.count) {  // wave-uniform
        const float c = D2[K >> 4][K & 7][(K >> 3) & 1];
        D2[K >> 4][K & 7][(K >> 3) & 1] = s == fa ? va : (s == fb ? vb : c);
    }
    if constexpr (K < 63) matrix_apply<K + 1>(D2, sel, fa, fb, va, vb);
}

// The round trip of a matrix call: nb is the block's budget of its k stream bits (1..k), mword = StepArgs::matrix().  sel.count
// == 2^k - 1 (the callers refuse anything else), so the syndrome, the message and j are below 2^k and every slot read is < count.
// tile: the lane's column of its wave's tile - count values for the flipped forms and, with the pair search, count more for e.
template <bool DITH>
SVS_HD void embed_block_matrix(uint32_t (&rx)[8], uint32_t (&ry)[8], uint32_t nb, uint32_t hi, uint32_t kind, const CoeffTable &sel,
                               const StepArgs &steps, uint32_t mword, uint32_t s_b, float *tile, uint32_t stride) {
    pf::f32x2 D2[4][8];
    forward_exact_paired(rx, ry, D2);
    const uint32_t n = sel.count;
    float *e = tile + n * stride;
    uint32_t ph = 0, pl = 0, fa = 64u, fb = 64u;
    if (mword & 8u) {  // wave-uniform: the pair search
        matrix_pass<DITH, true>(D2, sel, steps, kind, ph, pl, s_b, tile, e, stride);
        const uint32_t j = matrix_syndrome(ph, pl) ^ matrix_message(hi, nb);
        if (j) matrix_search(j, n, e, stride, fa, fb);
    } else {
        matrix_pass<DITH, false>(D2, sel, steps, kind, ph, pl, s_b, tile, e, stride);
        const uint32_t j = matrix_syndrome(ph, pl) ^ matrix_message(hi, nb);
        if (j) fa = j - 1u;
    }
    const float va = fa < 64u ? tile[fa * stride] : 0.0f, vb = fb < 64u ? tile[fb * stride] : 0.0f;
    matrix_apply(D2, sel, fa, fb, va, vb);
    inverse_exact_paired<false>(D2, rx, ry);
}

// The requantisation channel of one block (include/svsdct.h, "requantisation channel"): the same round trip with the 64-step
// requantiser in place of the payload loop, and a decoder's store.  Every step is one float32 operation, in the header's order.
SVS_HD void requantise_block_exact(uint32_t (&rx)[8], uint32_t (&ry)[8], const ChannelArgs &ch) {
    using pf::f32x2;
    f32x2 D2[4][8];
    forward_exact_paired(rx, ry, D2);
    D2[0][0][0] = D2[0][0][0] - 1024.0f;   // the level shift of 128 per pixel, on DC
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        const float s = ch.step(k);        // wave-uniform
        const float c = D2[k >> 4][k & 7][(k >> 3) & 1];
        D2[k >> 4][k & 7][(k >> 3) & 1] = rintf(c / s) * s;
    }
    D2[0][0][0] = D2[0][0][0] + 1024.0f;
    inverse_exact_paired<true>(D2, rx, ry);
}

// =====================================================================================================
// The streaming embed arithmetic (n <= 15; every mode): the reference's stego pixels, bit for bit, at the cost of a cheap
// sparse transform for almost every block.
//
// The reference's output for a block is trunc(clip(out)), out = pf_dct3(pf_dct3(D')) in float32 (config_and_setup.py:
// 166-171).  embed_block_guarded computes, with a handful of operations,
//   * the payload-carrying coefficients EXACTLY as pocketfft does (so every quantiser decision q_k is the reference's),
//   * pred = X + G(change): the pixel plus the sparse inverse of the n coefficient changes, and
//   * BETA, a rigorous bound on |out - pred| for this block (tools/guard_bound.py: first-order running error analysis of
//     every operation of svs::pf::dct2_8 / dct3_8, stage-wise Cauchy-Schwarz over the block's energy):
//         BETA = u' * (KDC * mean + KE * ||X - mean||_2 + KD * (1.5 delta + 0.01)) + 2^-20,   u' = 2^-24 (1 + 2^-10).
// If every pred is farther than BETA from the integers, floor(pred) IS floor(out) for all 64 pixels and the cheap result
// is the reference's (values outside [0, 255] clip to the same byte either way; flagging them too is merely conservative).
// Otherwise the function returns true and the caller redoes the block with the pocketfft-identical arithmetic
// (embed_block_exact on the host emulation; the 8-lanes-per-block replay inside the kernel, svs_device.hpp).
// With one coefficient row (n <= 7) the change is the same in all 8 rows of a column, so only 8 values are tested and a
// noise block (mean 128, sigma 65, delta 8: BETA = 1.1e-3) is flagged with probability 16 * BETA = 1.7 %; smooth content 0.5 %.
// Constants printed by tools/guard_bound.py (tests/test_guarded_mode_cpu.py re-derives them):
#define SVS_GUARD_KDC 17.0001      // per unit of the mean pixel value
#define SVS_GUARD_KE 31.05         // per unit of ||X - mean||_2 (the (2 -> 1) norm is at least 30.66: the bound is tight)
#define SVS_GUARD_KD_U1 19.61      // per unit of 1.5 delta + 0.01, at most 7 modified coefficients (incl. the kernel's own sparse inverse)
#define SVS_GUARD_KD_U2 54.78      // at most 15 modified coefficients
// SVS_NEAREST changes a coefficient by at most delta plus rounding (nearest_parity), the reference's rule by up to 1.5 delta:
// the KD term - and the 16-bit range of the packed column deltas - assume 1.5 delta, so the same BETA bounds both rules.  It
// is merely not tight under the flag (g_delta could shrink by a third there; not done: a change of the flagged share of blocks
// wants its own soak).
// SVS_MINMOVE writes a value between the coefficient and SVS_NEAREST's lattice point, so its change is at most delta plus
// rounding as well.  tools/guard_bound.py uses two facts about the written value cn_k and no other: it is a float32 that the
// exact arithmetic writes verbatim (D' = D with cn_k in place), and |cn_k - c_k| <= 1.5 delta + 0.01.  Neither needs cn_k to
// be a lattice point; a coefficient that stays (cn_k = D_k, change 0) is an unmodified one to the analysis.  So the streaming
// bodies take the rule with the same BETA.
// tests/test_guard_rules_cpu.py and tests/test_guard_rules_gpu.py hold this on frames whose blocks sit at the guard's boundary
// under each rule (tests/golden/guard_rules_corpus.npz), waves of 1 to 128 replays included.
#define SVS_GUARD_UEFF (5.9604644775390625e-8 * (1.0 + 0.0009765625))
// delta range the guarded path is used for (outside it the caller takes the exact kernel): below, the changes are smaller
// than BETA and every block would be flagged; above, BETA itself exceeds 1/8
#define SVS_GUARD_DELTA_MIN 0.25
#define SVS_GUARD_DELTA_MAX 4096.0

// One coefficient through the quantiser, in the float domain: change = fl(q' delta) - c with q' = round-half-even(c / delta)
// forced to the parity of `bit` (config_and_setup.py:148-156).  t + 1.5 * 2^23 rounds t to the nearest-even integer q AND leaves
// q in the low mantissa bits of the sum (|t| < 2^22: delta >= 1/4 and |c| <= 2040 here), so the parity is forced on the bit
// pattern and q' comes back by subtracting the constant - no conversion to an integer and back (those are 1.6-slot
// instructions, profiles/r04_valu_issue_rate.txt).  Same results as quant_index / force_parity (tests: guarded mode vs the oracle).
// NEAREST (SVS_NEAREST, nearest_parity): q +- 1 is +- 1 on the bit pattern of m as well (an ulp at 1.5 * 2^23 is 1), and the side
// is a compare of c with the unforced q delta and a select - no branch.  A compile-time argument of this FUNCTION: the
// callers choose between the two forms of their quantiser loop with one test of qp.kind per block (QimRule).
// RULE_MINMOVE (SVS_MINMOVE): the change to the clamped value, minmove_clamp of c around that lattice point with the band r
// (qim_band) - 0 exactly for a coefficient inside its band.
template <int QM, int RULE = RULE_REFERENCE>
SVS_HD float qim_change(float c, uint32_t bit, const QimParams &qp, float r = 0.0f) {
    if constexpr (QM == QM_DOUBLE) {
        const int q0 = quant_index<QM>(c, qp);
        const int q = RULE != RULE_REFERENCE ? nearest_parity<QM>(q0, (int)bit, c, qp) : force_parity(q0, (int)bit);
        const float ct = (float)((double)q * qp.delta_d);
        if constexpr (RULE == RULE_MINMOVE) return minmove_clamp(c, ct, r) - c;
        else return ct - c;
    } else {
        const float kMagic = 12582912.0f;   // 1.5 * 2^23
        const float t = c * qp.inv_delta_f;
        float m = t + kMagic;
        if constexpr (QM != QM_POW2) {
            const float r = m - kMagic;
            const float miss = fabsf(fabsf(t - r) - 0.5f);       // distance of t from the nearest half-integer
            if (miss <= fabsf(t) * 4.76837158203125e-7f)          // see quant_index
                m = rintf(c / qp.delta_f) + kMagic;
        }
        uint32_t mb = __builtin_bit_cast(uint32_t, m);
        if constexpr (RULE != RULE_REFERENCE) {
            const float c0 = (m - kMagic) * qp.delta_f;
            const uint32_t dir = c > c0 ? 1u : (c < c0 ? ~0u : 2u * bit - 1u);
            mb += ((mb ^ bit) & 1u) ? dir : 0u;
        } else {
            mb = (mb & ~1u) | bit;
        }
        const float qf = __builtin_bit_cast(float, mb) - kMagic;
        if constexpr (RULE == RULE_MINMOVE) return minmove_clamp(c, qf * qp.delta_f, r) - c;
        else return qf * qp.delta_f - c;
    }
}

// ---- one coefficient row (n <= 7) in the INTEGER domain (round 6; rounds 3-5 applied the same eight floors in the float domain:
// byte -> float, add, saturating float -> byte for each of the 64 pixels) ------------------------------------------------
// With n <= 7 the change is the same in all 8 rows of a pixel column, so the block's result is pixel + d[x] with eight
// integers d[x] = floor(change of column x).  When no pixel of the block can leave [0, 255] - min pixel + min d >= 0 and
// max pixel + max d <= 255 - the saturation of the store never acts, and because  sum_j (p_j + d_j) 256^j = P + D  with
// D = sum_j d_j 256^j (mod 2^32) and every p_j + d_j a byte, the four stego bytes of a row dword are ONE 32-bit add of the
// packed column deltas: 16 v_add_u32 per block instead of 64 x (byte -> float, add, float -> saturated byte).  The price is
// the block's min / max pixel - packed 16-bit min / max on the even / odd byte lanes the column sums split the rows into
// anyway.  The decision (BETA, `worst`) is guard_decide's, value for value; the quantiser step is qim_change (the float-
// domain form of the two-row kernel, same results as quant_index / force_parity for |c / delta| < 2^22: delta >= 1/4 here).
SVS_HD uint32_t pk_min_u16(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
#else
    const uint32_t al = a & 0xffffu, bl = b & 0xffffu, ah = a >> 16, bh = b >> 16;
    return (al < bl ? al : bl) | ((ah < bh ? ah : bh) << 16);
#endif
}
SVS_HD uint32_t pk_max_u16(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
#else
    const uint32_t al = a & 0xffffu, bl = b & 0xffffu, ah = a >> 16, bh = b >> 16;
    return (al > bl ? al : bl) | ((ah > bh ? ah : bh) << 16);
#endif
}
SVS_HD int floor_to_int(float x) {   // (int)floor(x): v_cvt_flr_i32_f32
#if defined(__HIP_DEVICE_COMPILE__)
    int r;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(x));
    return r;
#else
    return (int)floorf(x);
#endif
}
SVS_HD int imin3(int a, int b, int c) { const int m = a < b ? a : b; return m < c ? m : c; }
SVS_HD int imax3(int a, int b, int c) { const int m = a > b ? a : b; return m > c ? m : c; }

// pins three running values at this point of the instruction stream (device only): an opaque, ordered use-and-redefinition,
// so that the chains feeding them are complete here and the operands they consumed are dead - without it the instruction
// selector lets the min / max / sum-of-squares chains of guard_decide_int trail the transform, with their 32 lane splits alive
#if defined(__HIP_DEVICE_COMPILE__)
#define SVS_PIN3(a, b, c) asm volatile("" : "+v"(a), "+v"(b), "+v"(c))
#else
#define SVS_PIN3(a, b, c) ((void)0)
#endif
#define SVS_ROW1_UNDECIDED 1u   // guard_decide_int: BETA does not separate some column's change from the integer grid
#define SVS_ROW1_MAY_CLIP 2u    //                   min pixel + min d < 0 or max pixel + max d > 255: the plain add must not be used

// the eight column deltas of a block as two's complement 16-bit lanes: columns (0, 2), (1, 3), (4, 6), (5, 7) - the form the
// saturating store adds to the even / odd byte lanes of a row dword.  (|d| < 2^14 for every delta the guarded range admits:
// 1.5 * 4096 * sum of 7 basis values * a(0) < 5700.)
struct ColumnDeltas {
    uint32_t e_lo, o_lo, e_hi, o_hi;
};
// ... and as ONE 32-bit addend per row dword: sum_j d_j 256^j (mod 2^32) of columns 0..3 (e = e_lo, o = o_lo) / 4..7.  A lane
// pair (a, b) read as an integer is a + 65536 b + 65536 [a < 0]; without the last term it is the addend of its two columns.
SVS_HD uint32_t packed_addend(uint32_t e, uint32_t o) {
    const uint32_t ev = e - ((e & 0x8000u) << 1), ov = o - ((o & 0x8000u) << 1);
    return ev + (ov << 8);
}

SVS_HD uint32_t pk_add_i16(uint32_t a, uint32_t b) {   // lane-wise 16-bit add (wraps; the callers stay far inside the range)
#if defined(__HIP_DEVICE_COMPILE__)
    typedef int16_t i16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(i16x2, a) + __builtin_bit_cast(i16x2, b));
#else
    return ((a + b) & 0xffffu) | (((a >> 16) + (b >> 16)) << 16);
#endif
}
SVS_HD uint32_t pk_clamp_u8_i16(uint32_t a) {   // lane-wise clamp of signed 16-bit lanes to [0, 255]
#if defined(__HIP_DEVICE_COMPILE__)
    typedef int16_t i16x2 __attribute__((ext_vector_type(2)));
    const i16x2 zero = {0, 0}, top = {255, 255};
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_elementwise_max(__builtin_bit_cast(i16x2, a), zero), top));
#else
    uint32_t r = 0;
    for (int h = 0; h < 2; ++h) {
        int v = (int16_t)(a >> (16 * h));
        v = v < 0 ? 0 : (v > 255 ? 255 : v);
        r |= (uint32_t)v << (16 * h);
    }
    return r;
#endif
}

// the quantiser loops of the streaming bodies: coefficient row 0 (flat indices 1..7) and rows 0 and 1 (1..15) replaced by
// their changes, 0 where nothing is embedded.  NEAREST as in qim_change; the budget is applied by the caller.
template <int QM, int RULE>
SVS_HD void qim_changes_row0(float (&D)[8], uint32_t n, uint32_t hi, const QimRule &qp) {
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        float change = 0.0f;
        if ((uint32_t)k <= n)  // wave-uniform; the budget is applied below, for the one block it concerns
            change = qim_change<QM, RULE>(D[k], (hi >> (32 - k)) & 1u, qp, qim_band<RULE>(qp, (uint32_t)k));
        D[k] = change;
    }
}

// -> SVS_ROW1_* flags and the column deltas (meaningful unless SVS_ROW1_UNDECIDED).
// (A compile-time coefficient count - n = 3, BASELINE configs[2] - removes a quarter of the instructions and changes nothing
// measurable: the kernel's arithmetic is hidden behind its memory traffic, 1.6144 vs 1.6056 ms per 600 x 4K in a same-process
// A/B.  Not instantiated.)
template <int QM>
SVS_HD uint32_t guard_decide_int(const uint32_t (&rx)[8], const uint32_t (&ry)[8], uint32_t n, uint32_t nb, uint32_t hi,
                                 const QimRule &qp, ColumnDeltas &cd) {
    float V[8];
    uint32_t S = 0, Q = 0, mn = 0x00ff00ffu, mx = 0u;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        uint32_t te = 0, to = 0;   // columns (0, 2) and (1, 3) of this half as 16-bit lanes, each <= 2040
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const uint32_t w = half ? ry[r] : rx[r];
            const uint32_t e = w & 0x00ff00ffu, o = (w >> 8) & 0x00ff00ffu;
            te += e;
            to += o;
            Q = dot4_u8(w, w, Q);
            mn = pk_min_u16(pk_min_u16(mn, e), o);
            mx = pk_max_u16(pk_max_u16(mx, e), o);
            if (r & 1) SVS_PIN3(mn, mx, Q);
        }
        V[4 * half + 0] = (float)(te & 0xffffu) * SVS_A0;
        V[4 * half + 1] = (float)(to & 0xffffu) * SVS_A0;
        V[4 * half + 2] = (float)(te >> 16) * SVS_A0;
        V[4 * half + 3] = (float)(to >> 16) * SVS_A0;
        const uint32_t t = te + to;
        S += (t & 0xffffu) + (t >> 16);
        SVS_SCHED_FENCE();
    }
    float D[8];
    pf::dct2_8(V, D);   // row 0 of the coefficient matrix, bit-identical to scipy's
    SVS_SCHED_FENCE();
    if (qp.kind == (uint32_t)RULE_MINMOVE) qim_changes_row0<QM, RULE_MINMOVE>(D, n, hi, qp);
    else if (qp.kind == (uint32_t)RULE_NEAREST) qim_changes_row0<QM, RULE_NEAREST>(D, n, hi, qp);
    else qim_changes_row0<QM, RULE_REFERENCE>(D, n, hi, qp);
    if (nb < n) {   // the block the payload ends in: coefficients past the budget stay as they are (config_and_setup.py:141)
#pragma unroll
        for (int k = 1; k < 8; ++k)
            if ((uint32_t)(k - 1) >= nb) D[k] = 0.0f;
    }
    D[0] = 0.0f;
    float P[8];
    idct8<8, true>(D, P);
    // BETA for this block: 64 Q - S^2 = 64 * (sum of squared deviations from the mean), an exact integer < 2^32
    const float spread = guard_sqrt((float)(64u * Q - S * S));
    const float beta = fmaf(qp.g_sum, (float)S, fmaf(qp.g_resid, spread, qp.g_delta));
    float worst = 0.0f;   // largest |frac(change) - 1/2| among the 8 columns
    int d[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) {
        const float ch = P[x] * SVS_A0;
        // v_fract_f32 is ch - floor(ch) (exact for these magnitudes) except that it stays below 1 where that difference would
        // round up to 1.0 (ch a hair below an integer): 1 - 2^-24 is flagged like 1.0 (BETA >= 2^-20)
        worst = fmaxf(worst, fabsf(fract_f32(ch) - 0.5f));
        d[x] = floor_to_int(ch);
    }
    uint32_t flags = (nb > 0 && !(worst < 0.5f - beta)) ? SVS_ROW1_UNDECIDED : 0u;   // nb == 0: the reference never enters the block (:130,:132)
    const int dmin = imin3(imin3(d[0], d[1], d[2]), imin3(d[3], d[4], d[5]), d[6] < d[7] ? d[6] : d[7]);
    const int dmax = imax3(imax3(d[0], d[1], d[2]), imax3(d[3], d[4], d[5]), d[6] > d[7] ? d[6] : d[7]);
    const uint32_t mnl = mn & 0xffffu, mnh = mn >> 16, mxl = mx & 0xffffu, mxh = mx >> 16;
    const int pmin = (int)(mnl < mnh ? mnl : mnh), pmax = (int)(mxl > mxh ? mxl : mxh);
    if (pmin + dmin < 0 || pmax + dmax > 255) flags |= SVS_ROW1_MAY_CLIP;
    cd.e_lo = ((uint32_t)d[0] & 0xffffu) | ((uint32_t)d[2] << 16);
    cd.o_lo = ((uint32_t)d[1] & 0xffffu) | ((uint32_t)d[3] << 16);
    cd.e_hi = ((uint32_t)d[4] & 0xffffu) | ((uint32_t)d[6] << 16);
    cd.o_hi = ((uint32_t)d[5] & 0xffffu) | ((uint32_t)d[7] << 16);
    return flags;
}

// the stores: pixel + d[column], clipped to [0, 255] (trunc(clip(x + c)) == clip(x + floor(c)) for integer x, :171)
SVS_HD void apply_deltas_plain(uint32_t (&rx)[8], uint32_t (&ry)[8], const ColumnDeltas &cd) {   // nothing can clip
    const uint32_t lo = packed_addend(cd.e_lo, cd.o_lo), hi = packed_addend(cd.e_hi, cd.o_hi);
#pragma unroll
    for (int r = 0; r < 8; ++r) { rx[r] += lo; ry[r] += hi; }
}
SVS_HD uint32_t add_clip_dword(uint32_t w, uint32_t de, uint32_t dodd) {
#if defined(__HIP_DEVICE_COMPILE__)
    // opaque copy: without it the compiler keeps the 64 lane splits of guard_decide_int alive for this (rare) path - 50 VGPRs
    asm("" : "+v"(w));
#endif
    const uint32_t e = pk_clamp_u8_i16(pk_add_i16(w & 0x00ff00ffu, de));
    const uint32_t o = pk_clamp_u8_i16(pk_add_i16((w >> 8) & 0x00ff00ffu, dodd));
    return e | (o << 8);
}
SVS_HD void apply_deltas_clipped(uint32_t (&rx)[8], uint32_t (&ry)[8], const ColumnDeltas &cd) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        rx[r] = add_clip_dword(rx[r], cd.e_lo, cd.o_lo);
        ry[r] = add_clip_dword(ry[r], cd.e_hi, cd.o_hi);
    }
}

// decide, then apply: on return rx/ry hold the block's stego pixels - or, when the result is true (undecided), its original
// pixels, untouched (the host emulation, the one-block-per-lane and fused-colour kernels; embed_row1_kernel chooses the
// store form per WAVE instead of per lane)
template <int QM>
SVS_HD bool embed_block_guarded(uint32_t (&rx)[8], uint32_t (&ry)[8], uint32_t n, uint32_t nb, uint32_t hi, uint32_t lo,
                                const QimRule &qp) {
    (void)lo;   // one coefficient row: the window is its first word
    ColumnDeltas cd;
    const uint32_t flags = guard_decide_int<QM>(rx, ry, n, nb, hi, qp, cd);
    if (flags & SVS_ROW1_UNDECIDED) return true;
    if (flags & SVS_ROW1_MAY_CLIP) apply_deltas_clipped(rx, ry, cd);
    else apply_deltas_plain(rx, ry, cd);
    return false;
}

// Two coefficient rows (n = 8..15), rigorous: the same construction with 64 predictions instead of 8 (the change now varies
// down a column) - pocketfft-identical rows 0 and 1, QIM with the reference's decisions, sparse inverse, and every pixel's
// prediction tested against the grid with the bound of ITS position: the (2 -> 1) norms behind KE differ by pixel (24.7 in
// rows / columns 0, 3, 4, 7 crossed with each other, 31.0 in rows / columns 1, 2, 5, 6 crossed, 27.9 mixed), which takes the
// share of undecided noise blocks from 13 % to 12 %.  Every mode runs it (round 4: flags 0 and SVS_EXACT_GUARDED are the same launch).
#define SVS_GUARD_KE_CC 24.68
#define SVS_GUARD_KE_CE 27.93

// Outputs 0 and 1 of pocketfft's vertical transform (svs::pf::dct2_8 down a pixel column), for the four columns held as the
// bytes of w[0..7] - bit for bit, at a third of the operations (round 4; before, each column ran the float sequence of which
// the compiler kept the 41 operations behind X[0] and X[1]).  Pixels are integers, so every value of that sequence up to the
// first irrational twiddle is an exact small integer whichever way it is computed:
//     c0 = 2 x0, c7 = 2 x7, c1 = x1 + x2, c2 = x2 - x1, c3 = x3 + x4, c4 = x4 - x3, c5 = x5 + x6, c6 = x6 - x5      (pre-butterfly)
//     h4 = c0 - c7 = 2 d0,  tr2 = c1 - c5 = d1 + d2,  ti2 = c2 + c6 = d2 - d1,  with d_k = x_k - x_(7-k)              (radb2)
//     a1 = h4 - 2 c4 = 2 (d0 + d3),  b1 = h4 + 2 c4 = 2 (d0 - d3),  r[0] = 2 (sum of the column)                      (radb4)
// so they are formed on packed 16-bit lanes (two columns per operation) and converted to float once.  From there on the
// operations are pocketfft's own: h6 = W ti2 + W tr2, h5 = W tr2 - W ti2, r[1] = fl(2 h5 + a1), r[7] = fl(2 h6 + b1), the
// twiddle post-pass.  Two exact rescalings: fl(2 h + 2 a') = 2 fl(h + a') - r[1] and r[7] are carried at half their value -
// and that factor 2 is folded into the twiddle constants (T / 4 instead of T / 8; powers of two commute with rounding).
// S accumulates the sum of the 32 pixels (the guard's mean term) from the column sums that are there anyway.
// tests/test_guarded_mode_cpu.py holds this function against svs::pf::dct2_8 on random and extreme columns.
SVS_HD void vertical_pf01_packed(const uint32_t (&w)[8], float (&v0)[4], float (&v1)[4], uint32_t &S);

namespace pf {
SVS_HD void column_outputs01(float colsum, float tr2, float ti2, float a1h, float b1h, float &X0, float &X1) {
    X0 = colsum * (SVS_PF_SQRT2 * 0.25f);            // r[0] * (sqrt2 / 8), r[0] = 2 * colsum
    const float wtr = SVS_PF_W * tr2, wti = SVS_PF_W * ti2;
    const float h6 = wti + wtr, h5 = wtr - wti;
    const float o1 = h5 + a1h, o7 = h6 + b1h;        // r[1] / 2, r[7] / 2
    const float t1 = (SVS_PF_T0 * 0.25f) * o7 + (SVS_PF_T6 * 0.25f) * o1;
    const float t2 = (SVS_PF_T0 * 0.25f) * o1 - (SVS_PF_T6 * 0.25f) * o7;
    X1 = t1 + t2;
}
}  // namespace pf

SVS_HD void vertical_pf01_packed(const uint32_t (&w)[8], float (&v0)[4], float (&v1)[4], uint32_t &S) {
    typedef int16_t i16x2 __attribute__((vector_size(4)));
    uint32_t lane[2][8];  // [0]: bytes 0 and 2 (columns 0, 2), [1]: bytes 1 and 3 (columns 1, 3), as 16-bit lanes
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        lane[0][r] = w[r] & 0x00ff00ffu;
        lane[1][r] = (w[r] >> 8) & 0x00ff00ffu;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        uint32_t s[4];
        i16x2 d[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s[k] = lane[h][k] + lane[h][7 - k];  // <= 510 per lane: no carry between lanes
            d[k] = __builtin_bit_cast(i16x2, lane[h][k]) - __builtin_bit_cast(i16x2, lane[h][7 - k]);
        }
        const uint32_t t = (s[0] + s[3]) + (s[1] + s[2]);  // <= 2040 per lane
        S += (t & 0xffffu) + (t >> 16);
        const i16x2 tr2 = d[1] + d[2], ti2 = d[2] - d[1], a1h = d[0] + d[3], b1h = d[0] - d[3];   // |.| <= 510
#pragma unroll
        for (int c = 0; c < 2; ++c)  // 16-bit lane c of half h is column 2c + h
            pf::column_outputs01((float)(c ? (t >> 16) : (t & 0xffffu)), (float)tr2[c], (float)ti2[c], (float)a1h[c], (float)b1h[c],
                                 v0[2 * c + h], v1[2 * c + h]);
    }
}

// NFIX (8..15, or 0 = run-time n): the coefficient count at compile time - the quantiser loop loses its wave-uniform tests,
// outputs of the row-1 transform that nobody reads and inverse inputs that are known zeros disappear from the code.
// INPLACE: the stego bytes replace the pixels of rx / ry as they are computed (each column touches only its own byte of the
// row dwords) and an UNDECIDED block is left half-written - for a caller that has parked the original rows elsewhere (the
// two-row kernel parks them in LDS, where the exact replay wants them anyway: 16 registers and 16 moves less).
template <int QM, int RULE>
SVS_HD void qim_changes_rows01(float (&D0)[8], float (&D1)[8], uint32_t n, uint32_t hi, uint32_t lo, const QimRule &qp) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        float change = 0.0f;
        if (k >= 1 && (uint32_t)k <= n)  // wave-uniform; the budget is applied below, for the one block it concerns
            change = qim_change<QM, RULE>(k < 8 ? D0[k] : D1[k - 8], window_bit(hi, lo, k - 1), qp, qim_band<RULE>(qp, (uint32_t)k));
        if (k < 8) D0[k] = change;
        else D1[k - 8] = change;
    }
}

template <int QM, int NFIX = 0, bool INPLACE = false>
SVS_HD bool embed_block_guarded2(uint32_t (&rx)[8], uint32_t (&ry)[8], uint32_t n_rt, uint32_t nb, uint32_t hi, uint32_t lo,
                                 const QimRule &qp) {
    static_assert(NFIX == 0 || (NFIX >= 8 && NFIX <= 15), "two coefficient rows");
    const uint32_t n = NFIX ? (uint32_t)NFIX : n_rt;
    float V0[8], V1[8];
    uint32_t S = 0, Q = 0;
    {
        float a0[4], a1[4], b0[4], b1[4];
        vertical_pf01_packed(rx, a0, a1, S);
        vertical_pf01_packed(ry, b0, b1, S);
#pragma unroll
        for (int x = 0; x < 4; ++x) { V0[x] = a0[x]; V1[x] = a1[x]; V0[4 + x] = b0[x]; V1[4 + x] = b1[x]; }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        Q = dot4_u8(rx[r], rx[r], Q);
        Q = dot4_u8(ry[r], ry[r], Q);
    }
    float D0[8], D1[8];
    pf::dct2_8(V0, D0);
    pf::dct2_8(V1, D1);
    if (qp.kind == (uint32_t)RULE_MINMOVE) qim_changes_rows01<QM, RULE_MINMOVE>(D0, D1, n, hi, lo, qp);
    else if (qp.kind == (uint32_t)RULE_NEAREST) qim_changes_rows01<QM, RULE_NEAREST>(D0, D1, n, hi, lo, qp);
    else qim_changes_rows01<QM, RULE_REFERENCE>(D0, D1, n, hi, lo, qp);
    if (nb < n) {   // the block the payload ends in (see embed_block): coefficients past the budget stay as they are
#pragma unroll
        for (int k = 1; k < 16; ++k) {
            if ((uint32_t)(k - 1) >= nb) {
                if (k < 8) D0[k] = 0.0f;
                else D1[k - 8] = 0.0f;
            }
        }
    }
    float P0[8], P1[8];
    idct8<8, true>(D0, P0);
    if constexpr (NFIX == 0) idct8<8, false>(D1, P1);
    else idct8<NFIX - 7, false>(D1, P1);      // row 1: entries 0..n-8 can be non-zero
    // BETA of the three position classes
    const float spread = guard_sqrt((float)(64u * Q - S * S));
    const float base = fmaf(qp.g_sum, (float)S, qp.g_delta);
    const float beta_ee = fmaf(qp.g_resid, spread, base);
    const float beta_ce = fmaf(qp.g_resid * (float)(SVS_GUARD_KE_CE / SVS_GUARD_KE), spread, base);
    const float beta_cc = fmaf(qp.g_resid * (float)(SVS_GUARD_KE_CC / SVS_GUARD_KE), spread, base);
    // Per pixel: ch = change(y, x) - (1/2 - 2^-16), small in magnitude, so its two roundings are part of KD's model of this
    // sparse inverse and the test below sees the prediction itself, not a copy rounded at the magnitude of the pixel (round
    // 3 tested pixel + change and paid 2^-14 of BETA for it).  The change lies ON the integer grid where fract(ch) = kMid.
    // The byte is v_cvt_pk_u8_f32(pixel + ch): round-to-nearest-even of a value whose fractional part is at least BETA - and
    // BETA >= 2^-14 (make_guard) - away from the rounding boundary, while the sum's own rounding is at most 2^-16: the floor.
    constexpr float kHalf = 0.5f - 0x1p-16f;
    constexpr float kMid = 0.5f + 0x1p-16f;
    float near_cc = 1.0f, near_ce = 1.0f, near_ee = 1.0f;   // smallest distance from the grid per position class
    uint32_t sx[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sy[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // !INPLACE: the stego rows, committed only if decided
    uint32_t (&nx)[8] = INPLACE ? rx : sx;
    uint32_t (&ny)[8] = INPLACE ? ry : sy;
    const float ck[4] = {SVS_C1, SVS_C3, SVS_C5, SVS_C7};
    // CLS_C: class of this column's pixels in rows 0, 3, 4, 7;  CLS_E: in rows 1, 2, 5, 6
#define SVS_PREDCOL(X, W, NW, B, CLS_C, CLS_E)                                                  \
    {                                                                                           \
        const float e = fmaf(P0[X], SVS_A0, -kHalf), p1 = P1[X];                                \
        _Pragma("unroll") for (int y = 0; y < 4; ++y) {                                         \
            const float ca = fmaf(p1, ck[y], e), cb = fmaf(p1, -ck[y], e);                      \
            if (y == 0 || y == 3) CLS_C = fmin3_abs(CLS_C, fract_f32(ca) - kMid, fract_f32(cb) - kMid); \
            else CLS_E = fmin3_abs(CLS_E, fract_f32(ca) - kMid, fract_f32(cb) - kMid);          \
            NW[y] = put_pixel_rne<B>(ca + ubyte_to_float<B>(W[y]), NW[y]);                      \
            NW[7 - y] = put_pixel_rne<B>(cb + ubyte_to_float<B>(W[7 - y]), NW[7 - y]);          \
        }                                                                                       \
    }
    SVS_PREDCOL(0, rx, nx, 0, near_cc, near_ce) SVS_PREDCOL(1, rx, nx, 1, near_ce, near_ee) SVS_PREDCOL(2, rx, nx, 2, near_ce, near_ee)
    SVS_PREDCOL(3, rx, nx, 3, near_cc, near_ce) SVS_PREDCOL(4, ry, ny, 0, near_cc, near_ce) SVS_PREDCOL(5, ry, ny, 1, near_ce, near_ee)
    SVS_PREDCOL(6, ry, ny, 2, near_ce, near_ee) SVS_PREDCOL(7, ry, ny, 3, near_cc, near_ce)
#undef SVS_PREDCOL
    const bool undecided = nb > 0 && !(near_cc >= beta_cc && near_ce >= beta_ce && near_ee >= beta_ee);
    if constexpr (!INPLACE) {
        if (undecided) return true;   // the block keeps its original pixels
#pragma unroll
        for (int r = 0; r < 8; ++r) { rx[r] = nx[r]; ry[r] = ny[r]; }
    }
    return undecided;
}

// BETA's coefficients for `rows` coefficient rows (1 or 2), rounded up; host side
inline void make_guard(double delta, int rows, QimParams *qp) {
    const double up = 1.0 + 0x1p-18;   // float evaluation of BETA in the kernel: conversions, sqrt, two FMAs
    const double kd = rows <= 1 ? SVS_GUARD_KD_U1 : SVS_GUARD_KD_U2;
    qp->g_sum = (float)(SVS_GUARD_UEFF * SVS_GUARD_KDC / 64.0 * up);
    qp->g_resid = (float)(SVS_GUARD_UEFF * SVS_GUARD_KE / 8.0 * up);
    double gd = SVS_GUARD_UEFF * kd * (1.5 * delta + 0.01) + 0x1p-20 + 0x1p-22;
    // two rows: the byte comes from v_cvt_pk_u8_f32's own rounding of pixel + (change - (1/2 - 2^-16)), which is the floor only
    // while the change's fractional part stays 2^-15 below 1 (embed_block_guarded2) - a FLOOR under BETA, not a term of it
    if (rows >= 2 && gd < 0x1p-14) gd = 0x1p-14;
    qp->g_delta = (float)(gd * up);
}

// EXACT embed of TWO horizontally adjacent blocks at once: every value is a pair (block A, block B) and every transform
// instruction a packed-FP32 one (v_pk_add / v_pk_mul / v_pk_fma_f32, each component rounding exactly like the scalar
// operation).  Unlike embed_block_exact - which pairs two LINES of one block and has to transpose 2x2 sub-blocks between
// the passes - the two blocks never exchange data, so the packed form costs no extra instructions: 2 x 928 scalar transform
// operations become 928 packed ones.  Same results as two embed_block_exact calls, bit for bit.  No kernel runs it: as a
// kernel (two blocks per lane) it measured SLOWER than the one-block form - a v_pk_*_f32 costs two issue slots on this chip,
// and the 256-register footprint costs occupancy (profiles/history/r02_ab_exact_pair.txt).  The CPU tier still checks it
// against embed_block_exact (tests/hostemu, exact == 2).
template <int U, int QM, int RULE>
SVS_HD void qim_exact_pair(pf::f32x2 (&D)[8][8], uint32_t n, uint32_t nb_a, uint32_t nb_b, uint32_t hi_a, uint32_t lo_a, uint32_t hi_b,
                           uint32_t lo_b, const QimRule &qp) {
#pragma unroll
    for (int k = 1; k < 8 * U; ++k) {
        if ((uint32_t)k <= n) {  // wave-uniform
            const int i = k - 1;
#pragma unroll
            for (int which = 0; which < 2; ++which) {
                const int bit = (int)window_bit(which ? hi_b : hi_a, which ? lo_b : lo_a, i);
                const float c = D[k >> 3][k & 7][which];
                const float cn = qim_target<QM, RULE>(c, bit, qp, qim_band<RULE>(qp, (uint32_t)k));
                D[k >> 3][k & 7][which] = ((uint32_t)i < (which ? nb_b : nb_a)) ? cn : c;
            }
        }
    }
}

template <int U, int QM>
SVS_HD void embed_block_exact_pair(uint32_t (&ax)[8], uint32_t (&ay)[8], uint32_t (&bx)[8], uint32_t (&by)[8], uint32_t n,
                                   uint32_t nb_a, uint32_t nb_b, uint32_t hi_a, uint32_t lo_a, uint32_t hi_b, uint32_t lo_b,
                                   const QimRule &qp) {
    using pf::f32x2;
    f32x2 D[8][8];  // D[u][v] = (coefficient of A, coefficient of B)
    {
        f32x2 V[8][8];  // after the vertical pass: V[u][x]
#define SVS_COL2(X, WA, WB, B)                                                          \
    {                                                                                   \
        f32x2 col[8], out[8];                                                           \
        _Pragma("unroll") for (int r = 0; r < 8; ++r) {                                 \
            const f32x2 t = {ubyte_to_float<B>(WA[r]), ubyte_to_float<B>(WB[r])};       \
            col[r] = t;                                                                 \
        }                                                                               \
        pf::dct2_8(col, out);                                                           \
        _Pragma("unroll") for (int u = 0; u < 8; ++u) V[u][X] = out[u];                 \
        SVS_SCHED_FENCE();                                                              \
    }
        SVS_COL2(0, ax, bx, 0) SVS_COL2(1, ax, bx, 1) SVS_COL2(2, ax, bx, 2) SVS_COL2(3, ax, bx, 3)
        SVS_COL2(4, ay, by, 0) SVS_COL2(5, ay, by, 1) SVS_COL2(6, ay, by, 2) SVS_COL2(7, ay, by, 3)
#undef SVS_COL2
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            pf::dct2_8(V[u], D[u]);
            SVS_SCHED_FENCE();
        }
    }
    if (qp.kind == (uint32_t)RULE_MINMOVE) qim_exact_pair<U, QM, RULE_MINMOVE>(D, n, nb_a, nb_b, hi_a, lo_a, hi_b, lo_b, qp);
    else if (qp.kind == (uint32_t)RULE_NEAREST) qim_exact_pair<U, QM, RULE_NEAREST>(D, n, nb_a, nb_b, hi_a, lo_a, hi_b, lo_b, qp);
    else qim_exact_pair<U, QM, RULE_REFERENCE>(D, n, nb_a, nb_b, hi_a, lo_a, hi_b, lo_b, qp);
    f32x2 P[8][8];  // after the vertical inverse (axis 0 first, :168): P[y][v]
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        f32x2 col[8], out[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) col[u] = D[u][v];
        pf::dct3_8(col, out);
#pragma unroll
        for (int y = 0; y < 8; ++y) P[y][v] = out[y];
        SVS_SCHED_FENCE();
    }
#pragma unroll
    for (int y = 0; y < 8; ++y) {
        f32x2 px[8];
        pf::dct3_8(P[y], px);
        // np.uint8(np.clip(v, 0, 255)): clip, then truncate
        store_row_trunc(px[0][0], px[1][0], px[2][0], px[3][0], px[4][0], px[5][0], px[6][0], px[7][0], ax[y], ay[y]);
        store_row_trunc(px[0][1], px[1][1], px[2][1], px[3][1], px[4][1], px[5][1], px[6][1], px[7][1], bx[y], by[y]);
        SVS_SCHED_FENCE();
    }
}

// EXACT extract: parity bits of round(c_k/delta) with pocketfft-identical coefficients
// DITH (the dithered calls; U = 8 only): the parity of the index of c - d, d from the block's s_b
template <int U, int QM, bool DITH = false>
SVS_HD void extract_block_exact(const uint32_t (&rx)[8], const uint32_t (&ry)[8], uint32_t n, const QimParams &qp,
                                uint32_t &hi, uint32_t &lo, uint32_t s_b = 0u) {
    static_assert(!DITH || U == 8, "a dithered call covers all eight coefficient rows");
    float D[8][8];
    forward_exact(rx, ry, D);
    hi = 0;
    lo = 0;
#pragma unroll
    for (int k = 1; k < 8 * U; ++k) {
        if ((uint32_t)k <= n) {  // wave-uniform
            uint32_t bit;
            if constexpr (DITH) bit = dithered_parity<QM>(D[k >> 3][k & 7], qp, (uint32_t)k, s_b);
            else bit = (uint32_t)quant_index<QM>(D[k >> 3][k & 7], qp) & 1u;
            const int i = k - 1;
            if (i < 32) hi |= bit << ((31 - i) & 31);
            else lo |= bit << ((63 - i) & 31);
        }
    }
}

// EXACT extract with a coefficient selection: the parity of coefficient k lands at window position sel.slot(k) (instead of
// k - 1); the caller packs sel.count bits per block as always
template <int QM, bool DITH = false>
SVS_HD void extract_block_exact_selected(const uint32_t (&rx)[8], const uint32_t (&ry)[8], const CoeffTable &sel,
                                         const QimParams &qp, uint32_t &hi, uint32_t &lo, uint32_t s_b = 0u) {
    float D[8][8];
    forward_exact(rx, ry, D);
    hi = 0;
    lo = 0;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        const uint32_t s = sel.slot(k);
        if (s < sel.count) {  // wave-uniform
            uint32_t parity;
            if constexpr (DITH) parity = dithered_parity<QM>(D[k >> 3][k & 7], qp, (uint32_t)k, s_b);
            else parity = (uint32_t)quant_index<QM>(D[k >> 3][k & 7], qp) & 1u;
            const uint32_t bit = parity << ((31u - s) & 31u);
            if (s < 32u) hi |= bit;
            else lo |= bit;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// SOFT extraction (svs_soft_extract*, include/svsdct.h): one byte per payload coefficient - the hard bit in bit 7 and, in
// bits 0..6, how far the quantiser input x sits from the nearest decision boundary of its cell, in units of delta / 254.
// A format, as the dither's rule: x = c, or c - d under a dither (the hard side's own subtract), and
//   q = quant_index<QM>(x);  x0 = (float)q * (float)delta   (one multiply in every quantiser mode);  a = fabsf(x - x0)
//   h = 0.5f * (float)delta;  s = (float)(254.0 / (double)(float)delta)                       (both rounded once, host side)
//   m = clamp((int)((h - a) * s), 0, 127)  (one subtract, one multiply, truncation toward zero);  byte = ((q & 1) << 7) | m
// Every float step is one IEEE float32 operation (build with -ffp-contract=off), in the same order on host and device.
// ---------------------------------------------------------------------------------------------------------------------
// (device only) the 64 coefficients are computed HERE: each is used under one wave-uniform test of its own, and left alone
// the compiler sinks its share of the horizontal pass into that branch, which keeps the whole vertical pass and its partial
// sums alive through the loop - 45 to 50 registers over the 80 of the eight-row extract kernels, spilled to scratch
#if defined(__HIP_DEVICE_COMPILE__)
#define SVS_PIN_COEFFICIENTS(D)                                                  \
    _Pragma("unroll") for (int pin_k = 0; pin_k < 64; ++pin_k) asm volatile("" : "+v"((D)[pin_k >> 3][pin_k & 7]))
#else
#define SVS_PIN_COEFFICIENTS(D) ((void)0)
#endif

struct SoftArgs {            // by-value argument of extract_exact_kernel (read by its U = 8 instantiations only)
    uint32_t on;             // 0: a hard call - the kernel's sides that were there before
    float half;              // h
    float scale;             // s
    uint32_t recip;          // ceil(2^20 / n): t / n == (t * recip) >> 20 for every byte index t < 64 n of a wave's run
    // the vote (svs_soft_vote*, make_vote_args): the bytes are not written - each is added into a tally of `period` int32
    uint32_t vote = 0;       // 0: a soft extract call - the bytes are copied out
    // the histogram (svs_soft_histogram*, make_hist_args): the bytes are not written - each is counted into its frame's row
    uint32_t hist = 0;       // 0: a soft extract or a vote call
    uint64_t period = 0;     // 1 .. 2^61 - 1
    uint64_t base = 0;       // stream_bit0 mod period: call-local bit i has residue (base + i) mod period
    uint64_t head = 0;       // call-local bits i < head lie in copy 0 (stream position below period) and break ties
    double inv = 0.0;        // 1.0 / period where period <= 2^38, else 0 (no quotient: base + i < 2 period, vote_residue)
};

inline SoftArgs make_soft_args(float delta_f, uint32_t n) {
    return {1u, 0.5f * delta_f, (float)(254.0 / (double)delta_f), n ? ((1u << 20) + n - 1u) / n : 0u};
}

// ---- the vote: a soft byte's place and weight in the tally (include/svsdct.h states the format) ----------------------------
constexpr uint64_t kVotePeriodMax = (1ull << 61) - 1u;    // 4 * period, the tally's bytes, fits 63 bits
constexpr uint64_t kVoteCopiesShift = 22;                 // a call is refused when capacity > period << 22 (the int32 bound)

inline SoftArgs make_vote_args(SoftArgs sa, uint64_t period, uint64_t stream_bit0) {
    sa.vote = 1u;
    sa.period = period;
    sa.base = stream_bit0 % period;
    sa.head = stream_bit0 < period ? period - stream_bit0 : 0u;
    sa.inv = period <= (1ull << 38) ? 1.0 / (double)period : 0.0;
    return sa;
}

// ---- the histogram: 256 counts a frame (include/svsdct.h states the format) -------------------------------------------------
constexpr uint32_t kHistBins = 256;                       // one per value of the soft byte; hist[frame * 256 + byte] += 1

inline SoftArgs make_hist_args(SoftArgs sa) {
    sa.hist = 1u;
    return sa;
}

// (base + i) mod period for a call-local bit index i < 2^38 (a call has fewer than 2^31 blocks of at most 63 bits).
// period <= 2^38: x = base + i < 2^39 is exact as a double, x * inv is within 2^-13 of x / period, so the truncated quotient is
// the true one or off by one either way - one conditional correction.  Larger periods: inv = 0, the quotient is 0 and
// base + i < 2 period needs the same single correction.  No 64-bit division on the device.
SVS_HD uint64_t vote_residue(uint64_t i, const SoftArgs &sa) {
    const uint64_t x = sa.base + i;
    const uint64_t q = (uint64_t)((double)x * sa.inv);
    const int64_t r = (int64_t)(x - q * sa.period), p = (int64_t)sa.period;
    return (uint64_t)(r < 0 ? r + p : (r >= p ? r - p : r));
}

// what the byte adds to its tally entry: 2 (2b - 1)(2m + 1), and (2b - 1) more where the bit lies in copy 0
SVS_HD int32_t vote_of(uint32_t byte, bool in_head) {
    const int32_t w = 4 * (int32_t)(byte & 127u) + 2 + (in_head ? 1 : 0);
    return (byte & 128u) ? w : -w;
}

// the byte of quantiser input x.  The clamp is taken on the float so that no conversion leaves the range of int: for
// every v that converts, min(max((int)v, 0), 127) is the same value ((int)v == 0 on (-1, 0]).
template <int QM>
SVS_HD uint32_t soft_byte(float x, const QimParams &qp, const SoftArgs &sa) {
    const int q = quant_index<QM>(x, qp);
    const float x0 = (float)q * qp.delta_f;
    const float a = fabsf(x - x0);
    const float v = (sa.half - a) * sa.scale;
    const uint32_t m = v >= 127.0f ? 127u : (v > 0.0f ? (uint32_t)(int)v : 0u);
    return (((uint32_t)q & 1u) << 7) | m;
}

// SOFT extract of one block: put(s, byte) for every payload coefficient, s = sel.slot(k) its block-local stream slot.  `sel`
// is the call's selection or the prefix table of n_ac (make_prefix_table), so the selected loop of the hard sides serves
// every form; `dith` (wave-uniform) switches the hard dithered side's subtract on.  Each byte leaves as it is computed:
// nothing is gathered in registers.
template <int QM, class Put>
SVS_HD void extract_block_soft(const uint32_t (&rx)[8], const uint32_t (&ry)[8], const CoeffTable &sel, const QimParams &qp,
                               const SoftArgs &sa, bool dith, uint32_t s_b, Put &&put) {
    float D[8][8];
    forward_exact(rx, ry, D);
    SVS_PIN_COEFFICIENTS(D);
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        const uint32_t s = sel.slot(k);
        if (s < sel.count) {  // wave-uniform
            float x = D[k >> 3][k & 7];
            if (dith) x = x - dither_value(s_b, (uint32_t)k, qp.delta_f);
            put(s, soft_byte<QM>(x, qp, sa));
        }
        SVS_SCHED_FENCE();   // coefficient by coefficient: the bytes are independent, and scheduled together they spill
    }
}

// EXACT extract with a step per coefficient (svs_stepped_extract*): the parity of rintf((c - d) / dk), d = 0 without a dither.
// `sel` is never empty (the call's selection or the prefix table of n_ac).  A recursion over K, as qim_stepped_selected.
template <bool DITH, int K = 1>
SVS_HD void stepped_parities(const float (&D)[8][8], const CoeffTable &sel, const StepArgs &steps, uint32_t &hi, uint32_t &lo,
                             uint32_t s_b) {
    const uint32_t s = sel.slot(K);
    if (s < sel.count) {  // wave-uniform
        const float dk = steps.step_here(K);
        float x = D[K >> 3][K & 7];
        if constexpr (DITH) x = x - dither_value(s_b, (uint32_t)K, dk);
        const uint32_t bit = ((uint32_t)quant_index_by_division(x, dk) & 1u) << ((31u - s) & 31u);
        if (s < 32u) hi |= bit;
        else lo |= bit;
    }
    if constexpr (K < 63) stepped_parities<DITH, K + 1>(D, sel, steps, hi, lo, s_b);
}

template <bool DITH>
SVS_HD void extract_block_stepped(const uint32_t (&rx)[8], const uint32_t (&ry)[8], const CoeffTable &sel, const StepArgs &steps,
                                  uint32_t &hi, uint32_t &lo, uint32_t s_b = 0u) {
    float D[8][8];
    forward_exact(rx, ry, D);
    // the 63 AC coefficients are computed HERE, as in extract_block_soft and for its reason (SVS_PIN_COEFFICIENTS); DC is never read
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int k = 1; k < 64; ++k) asm volatile("" : "+v"(D[k >> 3][k & 7]));
#endif
    hi = 0;
    lo = 0;
    stepped_parities<DITH>(D, sel, steps, hi, lo, s_b);
}

// a wave-uniform float as a scalar value on the device (a vector register less for each the stepped soft side holds)
SVS_HD float wave_uniform(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
#else
    return v;
#endif
}

// SOFT extraction with a step per coefficient (svs_stepped_soft_extract*, include/svsdct.h states the format): soft_byte with
// the stepped extract's own index and the coefficient's own cell - h_k = 0.5f * dk and s_k = 254.0f / dk are computed here, one
// float32 operation each (the division is the correctly rounded one quant_index_by_division relies on; for an integer dk in
// 1..4095 it is make_soft_args' (float)(254.0 / (double)dk) bit for bit), so SoftArgs carries no per-coefficient value.
SVS_HD uint32_t stepped_soft_byte(float x, float dk, float hk, float sk) {   // hk = 0.5f * dk, sk = 254.0f / dk
    const int q = quant_index_by_division(x, dk);
    const float x0 = (float)q * dk;
    const float a = fabsf(x - x0);
    const float v = (hk - a) * sk;
    const uint32_t m = v >= 127.0f ? 127u : (v > 0.0f ? (uint32_t)(int)v : 0u);   // the clamp on the float, as soft_byte
    return (((uint32_t)q & 1u) << 7) | m;
}

// put(s, byte) for every payload coefficient, as extract_block_soft's loop; a recursion over K, as stepped_parities and for its
// reason (the step keeps a compile-time position).  `quad` holds the table's steps of coefficients K & ~3 .. K | 3, read at the
// first of the four where any of them carries a slot (StepArgs::quad_here).  `dith` is wave-uniform.
template <int K = 1, class Put>
SVS_HD void stepped_soft_bytes(const float (&D)[8][8], const CoeffTable &sel, const StepArgs &steps, bool dith, uint32_t s_b,
                               Put &&put, uint64_t quad = 0u) {
    const uint32_t s = sel.slot(K);
    if constexpr (K == 1 || (K & 3) == 0) {
        bool any = false;   // wave-uniform
#pragma unroll
        for (int k = K; k <= (K | 3); ++k) any = any || sel.slot(k) < sel.count;
        if (any) quad = steps.quad_here(K >> 2);
    }
    if (s < sel.count) {  // wave-uniform
        // the cell's three values first, each a scalar: their division is over before the coefficient's own begins
        const float dk = wave_uniform(StepArgs::step_of_quad(quad, K));
        const float hk = wave_uniform(0.5f * dk), sk = wave_uniform(254.0f / dk);
        SVS_SCHED_FENCE();
        float x = D[K >> 3][K & 7];
        if (dith) x = x - dither_value(s_b, (uint32_t)K, dk);
        put(s, stepped_soft_byte(x, dk, hk, sk));
    }
    SVS_SCHED_FENCE();   // coefficient by coefficient, as extract_block_soft
    if constexpr (K < 63) stepped_soft_bytes<K + 1>(D, sel, steps, dith, s_b, put, quad);
}

// extract_block_soft with a step per coefficient: `sel` is never empty (the call's selection or the prefix table of n_ac)
template <class Put>
SVS_HD void extract_block_stepped_soft(const uint32_t (&rx)[8], const uint32_t (&ry)[8], const CoeffTable &sel, const StepArgs &steps,
                                       bool dith, uint32_t s_b, Put &&put) {
    float D[8][8];
    forward_exact(rx, ry, D);
    // the 63 AC coefficients are computed HERE, as in extract_block_stepped: DC is never read, and pinned too it costs a register
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int k = 1; k < 64; ++k) asm volatile("" : "+v"(D[k >> 3][k & 7]));
#endif
    stepped_soft_bytes(D, sel, steps, dith, s_b, put);
}

inline int rows_for(int n) { return (n >> 3) + 1; }  // coefficient rows holding flat indices 1..n

// quantiser parameters and the cheapest exact evaluation mode for this delta (QuantMode); host side
inline int make_qim(double delta, QimParams *qp) {
    qp->delta_f = (float)delta;
    qp->inv_delta_f = 1.0f / qp->delta_f;
    qp->delta_d = delta;
    qp->tie_slope = (float)(SVS_TIE_SLOPE / (double)qp->delta_f) * 1.0000002f;  // rounded up
    {
        const double ueff = 5.9604644775390625e-8 * (1.0 + 0.0009765625), up = (1.0 + 0x1p-18) / (double)qp->delta_f;
        qp->tie2_sum = (float)(ueff * SVS_TIE2_KDC / 64.0 * up);
        qp->tie2_resid = (float)(ueff * SVS_TIE2_KE / 8.0 * up);
        qp->tie2_c00 = (float)(8.0 * 5.9604644775390625e-8 * up);   // the roundings of the quantiser input itself, |c| <= 2 c00
        // upper bound of extract_block_settle's margin over every pixel sum S in [0, 16320] (scan + slack for the scan step,
        // the float evaluation and the two 1.000001 factors)
        double worst = 0.0;
        for (int S = 0; S <= 16320; S += 8) {
            const double m = (double)qp->tie2_sum * S + (double)qp->tie2_resid * sqrt((double)S * (16320.0 - S)) +
                             (double)qp->tie2_c00 * S / 8.0 + 0x1p-20;
            if (m > worst) worst = m;
        }
        qp->tie2_max = (float)(worst * 1.001);
    }
    qp->g_sum = qp->g_resid = qp->g_delta = 0.0f;   // make_guard
    if ((double)qp->delta_f != delta) return QM_DOUBLE;
    int e = 0;
    const bool pow2 = frexp(delta, &e) == 0.5 && e > -100 && e < 100;
    return pow2 ? QM_POW2 : QM_F32;
}

}  // namespace svs
