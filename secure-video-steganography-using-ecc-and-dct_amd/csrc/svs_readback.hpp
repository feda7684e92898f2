// svs_readback.hpp - per-block arithmetic of the opt-in read-back pass (SVS_READBACK, include/svsdct.h): read a stego block
// back with the reference's extraction arithmetic and, where its payload bits do not come back, search for a block whose
// bits do.  Plain C++ on register values, like svs_block.hpp: csrc/svs_device.hpp checks one block per lane and repairs
// one block on eight lanes with the per-line steps below and the embed kernels' eight-lane forward / inverse passes
// (readback_kernel, search8: forward8 / inverse8 on 64-float tiles); tests/hostemu builds the one-lane
// form (search_block) with g++ for the CPU tier.  Both builds use -ffp-contract=off; the repair
// rounds to nearest after float arithmetic, so host and device must execute the same operations in the same order: the
// transforms are svs_block.hpp's pocketfft replays (their fmaf only where it is exact), every other operation below is one
// IEEE float32 operation (no FMA), and min / max and the final rounding are exact.
//
// Why a block fails: the reference clips the inverse transform to [0, 255] and truncates it (config_and_setup.py:166-171).
// In a block near black or white the clipping - and anywhere the truncation - moves payload coefficients, and one moved
// across a QIM decision boundary reads back as the wrong bit.  The receiver only sees uint8 pixels, so the sender may store
// any block that the reference's extraction decodes to the right bits; the receiver stays as it is.
#pragma once
#include <stdint.h>

#include "svs_block.hpp"

namespace svs {

#define SVS_READBACK_ITERS 16   // repair iterations per block (each: one correction, one exact read-back)

// the first nb bits of the MSB-first window hi:lo as a mask pair
SVS_HD void readback_mask(uint32_t nb, uint32_t &mhi, uint32_t &mlo) {
    mhi = nb >= 32 ? 0xffffffffu : (nb == 0 ? 0u : 0xffffffffu << (32 - nb));
    mlo = nb <= 32 ? 0u : (nb >= 64 ? 0xffffffffu : 0xffffffffu << (64 - nb));
}

// do the first nb payload coefficients of the pocketfft coefficients D carry the window's bits?  The quantiser is the
// extraction's (config_and_setup.py:160-161; QM_DOUBLE divides as QM_F32 does)
template <int U, int QM>
SVS_HD bool readback_bits_ok(const float (&D)[8][8], uint32_t nb, uint32_t hi, uint32_t lo, const QimParams &qp) {
    uint32_t h = 0, l = 0;
#pragma unroll
    for (int k = 1; k < 8 * U; ++k) {
        if ((uint32_t)k <= nb) {
            const uint32_t bit = (uint32_t)quant_index<QM>(D[k >> 3][k & 7], qp) & 1u;
            const int i = k - 1;
            if (i < 32) h |= bit << ((31 - i) & 31);
            else l |= bit << ((63 - i) & 31);
        }
    }
    uint32_t mhi, mlo;
    readback_mask(nb, mhi, mlo);
    return ((h ^ hi) & mhi) == 0 && ((l ^ lo) & mlo) == 0;
}

// the read-back of one block with the extraction's own arithmetic - the reference's bits for any input - only the first nb
// coefficients compared.  Two coefficient rows (n = 8..15): FAST extraction's FMA-factored forward with its proven tie margin
// (svs_block.hpp extract_block), the block redone with the pocketfft-identical transform when a quantiser input lies within
// the margin of a tie.  One row, and eight (its FAST form needs 203 instead of 144 VGPRs): extract_block_exact's
// pocketfft-identical forward transform.
template <int U, int QM>
SVS_HD bool readback_block_ok(const uint32_t (&rx)[8], const uint32_t (&ry)[8], uint32_t nb, uint32_t hi, uint32_t lo,
                              const QimParams &qp) {
    if (U == 2 && qp.delta_f >= SVS_FAST_EXTRACT_DELTA_MIN) {
        uint32_t h, l;
        if (!extract_block<U, QM>(rx, ry, nb, qp, h, l)) {
            uint32_t mhi, mlo;
            readback_mask(nb, mhi, mlo);
            return ((h ^ hi) & mhi) == 0 && ((l ^ lo) & mlo) == 0;
        }
    }
    float D[8][8];
    forward_exact(rx, ry, D);
    return readback_bits_ok<U, QM>(D, nb, hi, lo, qp);
}

// Repair of a block that does not read back (rx / ry: its stego rows, in and out).  Bounded and deterministic:
//   target  T_k = the lattice point q' delta of the wanted parity nearest to the block's coefficient c_k (k = 1..nb): the
//           centre of the nearest decision cell that gives the bit
//   step    for it = 0 .. SVS_READBACK_ITERS - 1:
//             y = X + IDCT((T - c) * (1 + it / 2))        (over-relaxed: without it, rounding absorbs corrections below half
//                                                          a grey level and the search stalls)
//             y += s, one constant that lifts the block off 0 or lowers it below 255 where its range allows (a constant
//                                                          only moves DC, which carries no payload)
//             X = clip(round-half-even(y), 0, 255);  c = the exact forward coefficients of X
//             accept when c reads back every bit (the exact read-back above)
// The gain grows with `it` and X moves from the previous iterate, so the search can also overshoot: at small delta (4) and
// at n = 63 on high-contrast blocks an accepted iterate can be far from the reference's block.  Those blocks do decode;
// tests/test_readback_cpu.py measures how many there are.
// The search is written per LINE of the block (coefficient row u, pixel row y) so that the device can run one block on
// eight lanes (csrc/svs_device.hpp search8) with exactly these operations: the transforms between the steps are
// pocketfft's per line, the min / max over the block and the shift are exact.  search_block below is the one-lane form, the
// only copy of the loop on this side: every form further down gives it its row functions and its acceptance.

// targets of coefficient row u (flat indices 8u .. 8u + 7; only 1 .. nb are used)
template <int QM>
SVS_HD void repair_targets_row(const float (&c)[8], int u, uint32_t nb, uint32_t hi, uint32_t lo, const QimParams &qp,
                               float (&T)[8]) {
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        const int k = 8 * u + v;
        T[v] = 0.0f;
        if (k >= 1 && (uint32_t)k <= nb) {
            const int bit = (int)window_bit(hi, lo, k - 1);
            int q = quant_index<QM>(c[v], qp);
            if ((q & 1) != bit) q = c[v] * qp.inv_delta_f >= (float)q ? q + 1 : q - 1;
            T[v] = (float)q * qp.delta_f;
        }
    }
}

// the over-relaxed correction of coefficient row u
SVS_HD void repair_correction_row(const float (&T)[8], const float (&c)[8], int u, uint32_t nb, float scale, float (&d)[8]) {
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        const int k = 8 * u + v;
        d[v] = (k >= 1 && (uint32_t)k <= nb) ? (T[v] - c[v]) * scale : 0.0f;
    }
}

// does coefficient row u miss a payload bit?
template <int QM>
SVS_HD bool row_misses(const float (&c)[8], int u, uint32_t nb, uint32_t hi, uint32_t lo, const QimParams &qp) {
    bool miss = false;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        const int k = 8 * u + v;
        if (k >= 1 && (uint32_t)k <= nb)
            miss |= ((uint32_t)quant_index<QM>(c[v], qp) & 1u) != window_bit(hi, lo, k - 1);
    }
    return miss;
}

// pixel row (8 bytes in lo4 / hi4) plus the inverse transform's row: the float pixels y, and their min / max folded in
SVS_HD void repair_add_row(uint32_t lo4, uint32_t hi4, const float (&row)[8], float (&y)[8], float &mn, float &mx) {
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        const float a = (float)((lo4 >> (8 * x)) & 0xffu) + row[x];
        const float b = (float)((hi4 >> (8 * x)) & 0xffu) + row[4 + x];
        y[x] = a;
        y[4 + x] = b;
        mn = fminf(mn, fminf(a, b));
        mx = fmaxf(mx, fmaxf(a, b));
    }
}

// the constant that takes the block off 0 / below 255 where its range allows
SVS_HD float repair_shift(float mn, float mx) {
    const float span = mx - mn;
    if (mn < 0.0f && span <= 255.0f) return -mn;
    if (mx > 255.0f && span <= 255.0f) return 255.0f - mx;
    return 0.0f;
}

// shifted, rounded to nearest and clipped: the row's new bytes
SVS_HD void repair_store_row(const float (&y)[8], float s, uint32_t &lo4, uint32_t &hi4) {
    uint32_t a = 0, b = 0;
    a = put_pixel_rne<0>(y[0] + s, a); a = put_pixel_rne<1>(y[1] + s, a);
    a = put_pixel_rne<2>(y[2] + s, a); a = put_pixel_rne<3>(y[3] + s, a);
    b = put_pixel_rne<0>(y[4] + s, b); b = put_pixel_rne<1>(y[5] + s, b);
    b = put_pixel_rne<2>(y[6] + s, b); b = put_pixel_rne<3>(y[7] + s, b);
    lo4 = a;
    hi4 = b;
}

// the one-lane form (host emulation; the device searches with eight lanes per block).  What a form of the pass differs in:
//   targets_row(c_u, u, T_u)                  the targets of coefficient row u from the block's coefficients
//   correction_row(T_u, c_u, u, scale, d_u)   the row's over-relaxed correction
//   accept(c)                                 is the iterate with these 8 x 8 coefficients taken?
template <class Targets, class Correction, class Accept>
SVS_HD bool search_block(uint32_t (&rx)[8], uint32_t (&ry)[8], Targets &&targets_row, Correction &&correction_row, Accept &&accept) {
    float c[8][8], T[8][8];
    forward_exact(rx, ry, c);
    for (int u = 0; u < 8; ++u) targets_row(c[u], u, T[u]);
    uint32_t px[8], py[8];
    for (int r = 0; r < 8; ++r) { px[r] = rx[r]; py[r] = ry[r]; }
    for (int it = 0; it < SVS_READBACK_ITERS; ++it) {
        const float scale = 1.0f + 0.5f * (float)it;   // exact
        // the correction's inverse transform: columns (axis 0) first, then rows, as the reference inverts
        float d[8][8], P[8][8], Y[8][8];
        for (int u = 0; u < 8; ++u) correction_row(T[u], c[u], u, scale, d[u]);
        for (int x = 0; x < 8; ++x) {
            float col[8], out[8];
            for (int u = 0; u < 8; ++u) col[u] = d[u][x];
            pf::dct3_8(col, out);
            for (int y = 0; y < 8; ++y) P[y][x] = out[y];
        }
        float mn = 1e30f, mx = -1e30f;
        for (int y = 0; y < 8; ++y) {
            float row[8];
            pf::dct3_8(P[y], row);
            repair_add_row(px[y], py[y], row, Y[y], mn, mx);
        }
        const float s = repair_shift(mn, mx);
        for (int y = 0; y < 8; ++y) repair_store_row(Y[y], s, px[y], py[y]);
        forward_exact(px, py, c);
        if (accept(c)) {
            for (int r = 0; r < 8; ++r) { rx[r] = px[r]; ry[r] = py[r]; }
            return true;
        }
    }
    return false;
}

// the plain form: flat indices 1 .. nb; the acceptance looks at the U coefficient rows the payload can reach
template <int U, int QM>
SVS_HD bool repair_block(uint32_t (&rx)[8], uint32_t (&ry)[8], uint32_t nb, uint32_t hi, uint32_t lo, const QimParams &qp) {
    return search_block(
        rx, ry, [&](const float (&c)[8], int u, float (&T)[8]) { repair_targets_row<QM>(c, u, nb, hi, lo, qp, T); },
        [&](const float (&T)[8], const float (&c)[8], int u, float scale, float (&d)[8]) { repair_correction_row(T, c, u, nb, scale, d); },
        [&](const float (&c)[8][8]) {
            bool miss = false;
            for (int u = 0; u < U; ++u) miss |= row_misses<QM>(c[u], u, nb, hi, lo, qp);
            return !miss;
        });
}

// The whole per-block step of the read-back pass: 0 = the block reads back (untouched), 1 = repaired in place, 2 = could not
// be repaired (untouched: the reference's stego block stays)
template <int U, int QM>
SVS_HD uint32_t readback_step(uint32_t (&rx)[8], uint32_t (&ry)[8], uint32_t nb, uint32_t hi, uint32_t lo, const QimParams &qp) {
    if (readback_block_ok<U, QM>(rx, ry, nb, hi, lo, qp)) return 0;
    return repair_block<U, QM>(rx, ry, nb, hi, lo, qp) ? 1u : 2u;
}

// ---------------------------------------------------------------------------------------------------------------------
// The keyed forms (svs_embed_dithered_readback*, include/svsdct.h): the same check and the same search under a coefficient
// SELECTION and a keyed DITHER.  The payload coefficients are those of a CoeffTable - the call's inverse table, or
// make_prefix_table(n_ac) - so flat index k carries window bit slot(k) when slot(k) < nb, and with a dither the receiver
// reads the parity of the index of c_k - d_k (dithered_parity, svs_block.hpp), d_k = dither_value(s_b, k, delta) of the
// block's physical position.  What changes against the forms above, coefficient by coefficient:
//   check    quant_index(c - d) & 1 against window bit slot(k)             (no dither: quant_index(c), no subtraction)
//   target   cp = c - d;  q = quant_index(cp), moved to the neighbour on cp's side when its parity is wrong;
//            T = (float)q * delta + d                                        (no dither: cp = c and no addition)
// The correction, the inverse, the shift, the rounding and the acceptance rule are the ones above, masked by slot(k) < nb
// instead of k <= nb.  All eight coefficient rows always: a selection may name any of them.  `dith` is uniform over a call
// (wave-uniform on the device): without it no operation on d is executed, so with the prefix table these forms give the
// bytes and status of readback_step<8, QM>.
// ---------------------------------------------------------------------------------------------------------------------

// the two words of the inverse table that hold the slots of coefficient row u (flat indices 8u .. 8u + 7)
struct RowSlots {
    uint32_t w0, w1;
    SVS_HD uint32_t slot(int v) const { return ((v < 4 ? w0 : w1) >> (8 * (v & 3))) & 0xFFu; }
};
SVS_HD RowSlots row_slots(const CoeffTable &t, int u) { return RowSlots{t.w[2 * u], t.w[2 * u + 1]}; }

// d of coefficient row u of the block with seed s_b (computed once per block: the search reads it every iterate)
SVS_HD void keyed_dither_row(uint32_t s_b, uint32_t u, float delta_f, float (&d)[8]) {
#pragma unroll
    for (int v = 0; v < 8; ++v) d[v] = dither_value(s_b, 8u * u + (uint32_t)v, delta_f);
}

template <int QM>
SVS_HD void keyed_targets_row(const float (&c)[8], const RowSlots &rs, uint32_t nb, uint32_t hi, uint32_t lo, const QimParams &qp,
                              bool dith, const float (&d)[8], float (&T)[8]) {
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        const uint32_t s = rs.slot(v);
        T[v] = 0.0f;
        if (s < nb) {
            const int bit = (int)window_bit_at(hi, lo, s);
            float cp = c[v];
            if (dith) cp = c[v] - d[v];
            int q = quant_index<QM>(cp, qp);
            if ((q & 1) != bit) q = cp * qp.inv_delta_f >= (float)q ? q + 1 : q - 1;
            float t = (float)q * qp.delta_f;
            if (dith) t = t + d[v];
            T[v] = t;
        }
    }
}

SVS_HD void keyed_correction_row(const float (&T)[8], const float (&c)[8], const RowSlots &rs, uint32_t nb, float scale,
                                 float (&e)[8]) {
#pragma unroll
    for (int v = 0; v < 8; ++v) e[v] = rs.slot(v) < nb ? (T[v] - c[v]) * scale : 0.0f;
}

// does the coefficient row miss a payload bit?  svs_extract_select* / svs_extract_dithered*'s own verdict
template <int QM>
SVS_HD bool keyed_row_misses(const float (&c)[8], const RowSlots &rs, uint32_t nb, uint32_t hi, uint32_t lo, const QimParams &qp,
                             bool dith, const float (&d)[8]) {
    bool miss = false;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        const uint32_t s = rs.slot(v);
        if (s < nb) {
            float cp = c[v];
            if (dith) cp = c[v] - d[v];
            miss |= ((uint32_t)quant_index<QM>(cp, qp) & 1u) != window_bit_at(hi, lo, s);
        }
    }
    return miss;
}

// one-lane forms (host emulation; the device runs the rows above on eight lanes, svs_device.hpp KeyedRows)
template <int QM>
SVS_HD bool keyed_block_misses(const float (&c)[8][8], const CoeffTable &sel, uint32_t nb, uint32_t hi, uint32_t lo,
                               const QimParams &qp, bool dith, const float (&d)[8][8]) {
    bool miss = false;
    for (int u = 0; u < 8; ++u) miss |= keyed_row_misses<QM>(c[u], row_slots(sel, u), nb, hi, lo, qp, dith, d[u]);
    return miss;
}

template <int QM>
SVS_HD bool repair_block_keyed(uint32_t (&rx)[8], uint32_t (&ry)[8], const CoeffTable &sel, uint32_t nb, uint32_t hi, uint32_t lo,
                               const QimParams &qp, bool dith, const float (&d)[8][8]) {
    return search_block(
        rx, ry,
        [&](const float (&c)[8], int u, float (&T)[8]) { keyed_targets_row<QM>(c, row_slots(sel, u), nb, hi, lo, qp, dith, d[u], T); },
        [&](const float (&T)[8], const float (&c)[8], int u, float scale, float (&e)[8]) {
            keyed_correction_row(T, c, row_slots(sel, u), nb, scale, e);
        },
        [&](const float (&c)[8][8]) { return !keyed_block_misses<QM>(c, sel, nb, hi, lo, qp, dith, d); });
}

// the per-block step under a selection and a dither (s_b: dither_block_seed of the block's physical position, read only
// with dith): 0 = reads back (untouched), 1 = repaired in place, 2 = could not be repaired (untouched)
template <int QM>
SVS_HD uint32_t readback_step_keyed(uint32_t (&rx)[8], uint32_t (&ry)[8], const CoeffTable &sel, uint32_t nb, uint32_t hi,
                                    uint32_t lo, const QimParams &qp, bool dith, uint32_t s_b) {
    float d[8][8];
    for (int u = 0; u < 8; ++u) {
        if (dith) keyed_dither_row(s_b, (uint32_t)u, qp.delta_f, d[u]);
        else for (int v = 0; v < 8; ++v) d[u][v] = 0.0f;
    }
    float c[8][8];
    forward_exact(rx, ry, c);
    if (!keyed_block_misses<QM>(c, sel, nb, hi, lo, qp, dith, d)) return 0;
    return repair_block_keyed<QM>(rx, ry, sel, nb, hi, lo, qp, dith, d) ? 1u : 2u;
}

// ---------------------------------------------------------------------------------------------------------------------
// The stepped forms (svs_stepped_embed_readback*, include/svsdct.h): the keyed forms with coefficient k's own step
// dk = (float)delta[k] (StepArgs) in the place of delta - a format, stated in the header.  Coefficient by coefficient:
//   d        dither_value(s_b, k, dk) with a dither: the stepped calls' d = r * dk of the block's physical position
//   check    (int)rintf((c - d) / dk) & 1 against window bit slot(k): svs_stepped_extract*'s own verdict
//   target   cp = c - d;  q = (int)rintf(cp / dk), moved to the neighbour on cp's side - cp * (1.0f / dk) >= (float)q - when
//            its parity is wrong;  T = (float)q * dk + d.  The side test takes the reciprocal so that a uniform table gives
//            the keyed form's cp * qp.inv_delta_f >= (float)q exactly (make_qim: inv_delta_f = 1.0f / delta_f)
// No QimParams: none of this reads the call's delta.  The correction, the inverse, the shift, the rounding and the store are
// the keyed forms' own functions.  d is computed where it is used, from s_b - a hash and three exact float operations - not
// held: the device's eight lanes keep the row's steps as four packed dwords and s_b, five registers instead of sixteen.
// With every delta[k] = D the bytes, counts and status are readback_step_keyed's at delta = D.
// ---------------------------------------------------------------------------------------------------------------------

// the four dwords of the table that hold the steps of coefficient row u (flat indices 8u .. 8u + 7), converted at use
struct RowSteps {
    uint32_t w[4];
    SVS_HD float step(int v) const { return (float)((w[v >> 1] >> (16 * (v & 1))) & 0xFFFFu); }
};
SVS_HD RowSteps row_steps(const StepArgs &t, int u) { return RowSteps{{t.w[4 * u], t.w[4 * u + 1], t.w[4 * u + 2], t.w[4 * u + 3]}}; }

// the quantiser input of coefficient v of row u: c - d under a dither, else c untouched
SVS_HD float stepped_input(float c, bool dith, uint32_t s_b, uint32_t u, int v, float dk, float &d) {
    d = 0.0f;
    if (!dith) return c;
    d = dither_value(s_b, 8u * u + (uint32_t)v, dk);
    return c - d;
}

SVS_HD void stepped_targets_row(const float (&c)[8], const RowSlots &rs, const RowSteps &st, uint32_t u, uint32_t nb, uint32_t hi,
                                uint32_t lo, bool dith, uint32_t s_b, float (&T)[8]) {
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        const uint32_t s = rs.slot(v);
        T[v] = 0.0f;
        if (s < nb) {
            const int bit = (int)window_bit_at(hi, lo, s);
            const float dk = st.step(v);
            float d;
            const float cp = stepped_input(c[v], dith, s_b, u, v, dk, d);
            int q = quant_index_by_division(cp, dk);
            if ((q & 1) != bit) q = cp * (1.0f / dk) >= (float)q ? q + 1 : q - 1;
            float t = (float)q * dk;
            if (dith) t = t + d;
            T[v] = t;
        }
        SVS_SCHED_FENCE();   // coefficient by coefficient: the divisions are independent, and scheduled together they cost registers
    }
}

// does the coefficient row miss a payload bit?  svs_stepped_extract*'s own verdict
SVS_HD bool stepped_row_misses(const float (&c)[8], const RowSlots &rs, const RowSteps &st, uint32_t u, uint32_t nb, uint32_t hi,
                               uint32_t lo, bool dith, uint32_t s_b) {
    bool miss = false;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        const uint32_t s = rs.slot(v);
        if (s < nb) {
            const float dk = st.step(v);
            float d;
            const float cp = stepped_input(c[v], dith, s_b, u, v, dk, d);
            miss |= ((uint32_t)quant_index_by_division(cp, dk) & 1u) != window_bit_at(hi, lo, s);
        }
        SVS_SCHED_FENCE();
    }
    return miss;
}

// one-lane forms (host emulation; the device runs the rows above on eight lanes, svs_device.hpp SteppedRows)
SVS_HD bool stepped_block_misses(const float (&c)[8][8], const CoeffTable &sel, const StepArgs &steps, uint32_t nb, uint32_t hi,
                                 uint32_t lo, bool dith, uint32_t s_b) {
    bool miss = false;
    for (int u = 0; u < 8; ++u)
        miss |= stepped_row_misses(c[u], row_slots(sel, u), row_steps(steps, u), (uint32_t)u, nb, hi, lo, dith, s_b);
    return miss;
}

// search_block with the stepped targets and the keyed correction; accept(c): is the iterate with these coefficients taken?  (The
// read-back accepts one that decodes, the margin pass one that is strong throughout.)
template <class Accept>
SVS_HD bool search_block_stepped(uint32_t (&rx)[8], uint32_t (&ry)[8], const CoeffTable &sel, const StepArgs &steps, uint32_t nb,
                                 uint32_t hi, uint32_t lo, bool dith, uint32_t s_b, Accept &&accept) {
    return search_block(
        rx, ry,
        [&](const float (&c)[8], int u, float (&T)[8]) {
            stepped_targets_row(c, row_slots(sel, u), row_steps(steps, u), (uint32_t)u, nb, hi, lo, dith, s_b, T);
        },
        [&](const float (&T)[8], const float (&c)[8], int u, float scale, float (&e)[8]) {
            keyed_correction_row(T, c, row_slots(sel, u), nb, scale, e);
        },
        accept);
}

SVS_HD bool repair_block_stepped(uint32_t (&rx)[8], uint32_t (&ry)[8], const CoeffTable &sel, const StepArgs &steps, uint32_t nb,
                                 uint32_t hi, uint32_t lo, bool dith, uint32_t s_b) {
    return search_block_stepped(rx, ry, sel, steps, nb, hi, lo, dith, s_b, [&](const float (&c)[8][8]) {
        return !stepped_block_misses(c, sel, steps, nb, hi, lo, dith, s_b);
    });
}

// the per-block step under per-coefficient steps (s_b: read only with dith): 0 = reads back (untouched), 1 = repaired in
// place, 2 = could not be repaired (untouched)
SVS_HD uint32_t readback_step_stepped(uint32_t (&rx)[8], uint32_t (&ry)[8], const CoeffTable &sel, const StepArgs &steps, uint32_t nb,
                                      uint32_t hi, uint32_t lo, bool dith, uint32_t s_b) {
    float c[8][8];
    forward_exact(rx, ry, c);
    if (!stepped_block_misses(c, sel, steps, nb, hi, lo, dith, s_b)) return 0;
    return repair_block_stepped(rx, ry, sel, steps, nb, hi, lo, dith, s_b) ? 1u : 2u;
}

// ---------------------------------------------------------------------------------------------------------------------
// The margin forms (svs_stepped_embed_readback_margin*, include/svsdct.h states the format): a second pass over the bytes the
// stepped pass left, which asks of every payload coefficient not only the right parity but the receiver's soft margin
//   v = (0.5f * dk - fabsf(x - (float)q * dk)) * (254.0f / dk) >= gate,   x = c - d, q = (int)rintf(x / dk)
// - stepped_soft_byte's arithmetic (svs_block.hpp), one float32 operation a step, so that for gate = 1..127 "strong" is exactly
// "the byte svs_stepped_soft_extract* gives has the right bit 7 and m >= gate".  A block with a wrong bit is the stepped pass's
// `unrepaired` and is left; a block that decodes with a weak coefficient is searched with repair_block_stepped's own targets,
// correction, inverse, shift, rounding and iterates, and the first iterate that is strong throughout is taken.
// ---------------------------------------------------------------------------------------------------------------------
#define SVS_MARGIN_MISS 1u   // a payload coefficient of the row has the wrong parity
#define SVS_MARGIN_WEAK 2u   // a payload coefficient of the row has v < gate

// both verdicts of a coefficient row from one function, coefficient by coefficient: bit 0 miss, bit 1 weak
SVS_HD uint32_t stepped_row_verdict(const float (&c)[8], const RowSlots &rs, const RowSteps &st, uint32_t u, uint32_t nb, uint32_t hi,
                                    uint32_t lo, bool dith, uint32_t s_b, float gate) {
    uint32_t bad = 0u;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        const uint32_t s = rs.slot(v);
        if (s < nb) {
            float dk = st.step(v);
#if defined(__HIP_DEVICE_COMPILE__)
            // the step is hidden from the compiler HERE: the search calls this once per iterate with the same row, and left to
            // itself the compiler computes the row's eight 0.5f * dk and eight 254.0f / dk ahead of the loop and holds them
            asm volatile("" : "+v"(dk));
#endif
            float d;
            const float x = stepped_input(c[v], dith, s_b, u, v, dk, d);
            const int q = quant_index_by_division(x, dk);
            const float a = fabsf(x - (float)q * dk);
            const float m = (0.5f * dk - a) * (254.0f / dk);
            if (((uint32_t)q & 1u) != window_bit_at(hi, lo, s)) bad |= SVS_MARGIN_MISS;
            if (!(m >= gate)) bad |= SVS_MARGIN_WEAK;
        }
        SVS_SCHED_FENCE();
    }
    return bad;
}

// one-lane forms (host emulation; the device runs the rows on eight lanes, svs_device.hpp SteppedRows with a gate)
SVS_HD uint32_t stepped_block_verdict(const float (&c)[8][8], const CoeffTable &sel, const StepArgs &steps, uint32_t nb, uint32_t hi,
                                      uint32_t lo, bool dith, uint32_t s_b, float gate) {
    uint32_t bad = 0u;
    for (int u = 0; u < 8; ++u)
        bad |= stepped_row_verdict(c[u], row_slots(sel, u), row_steps(steps, u), (uint32_t)u, nb, hi, lo, dith, s_b, gate);
    return bad;
}

// repair_block_stepped's search with the margin's acceptance: the first iterate whose payload coefficients are all strong
SVS_HD bool strengthen_block_stepped(uint32_t (&rx)[8], uint32_t (&ry)[8], const CoeffTable &sel, const StepArgs &steps, uint32_t nb,
                                     uint32_t hi, uint32_t lo, bool dith, uint32_t s_b, float gate) {
    return search_block_stepped(rx, ry, sel, steps, nb, hi, lo, dith, s_b, [&](const float (&c)[8][8]) {
        return stepped_block_verdict(c, sel, steps, nb, hi, lo, dith, s_b, gate) == 0u;
    });
}

// the per-block step of the margin pass, gate = (float)min_margin with min_margin in 1..127: 0 = strong throughout, or a wrong
// bit (the stepped pass's unrepaired block) - untouched either way; 1 = strengthened in place; 2 = weak, could not be
// strengthened (untouched: the bytes the stepped pass left, which decode)
SVS_HD uint32_t margin_step_stepped(uint32_t (&rx)[8], uint32_t (&ry)[8], const CoeffTable &sel, const StepArgs &steps, uint32_t nb,
                                    uint32_t hi, uint32_t lo, bool dith, uint32_t s_b, float gate) {
    float c[8][8];
    forward_exact(rx, ry, c);
    const uint32_t bad = stepped_block_verdict(c, sel, steps, nb, hi, lo, dith, s_b, gate);
    if (bad == 0u || (bad & SVS_MARGIN_MISS)) return 0;
    return strengthen_block_stepped(rx, ry, sel, steps, nb, hi, lo, dith, s_b, gate) ? 1u : 2u;
}

}  // namespace svs
