// svs_route.hpp - which kernel family an embed or extract call of the C ABI runs, and with which quantiser, coefficient rows,
// tile map and payload arguments (csrc/svs_capi.hip launches the plan).  Plain C++ (no HIP): tests/hostemu compiles it, so
// the CPU tier runs the library's routing and checks it (tests/test_route_cpu.py).
#pragma once
#include <stdint.h>

#include "svs_block.hpp"
#include "svs_index.hpp"   // kEighth, the tile map the plans name
#include "svs_order.hpp"   // BlockOrderArgs

namespace svs {

// The arguments that decide a call's route.  pocketfft / guarded are the SVS_EXACT_POCKETFFT / SVS_EXACT_GUARDED bits of the
// call's flags; guarded_off, guard_scale and tie_scale are test hooks (the experiments library's SVS_GUARDED_OFF,
// SVS_GUARD_SCALE and SVS_TIE_SCALE; the product passes false, 1, 1).
struct RouteArgs {
    double delta;
    uint32_t n_ac;            // clamped to 0..63
    uint64_t total_blocks;
    uint64_t n_bits;          // payload bits the caller offers (embed)
    uint64_t bit_offset;      // (embed)
    bool pocketfft, guarded;
    bool bgr;                 // the fused colour calls (svs_embed_bgr_dev / svs_extract_bgr_dev)
    bool guarded_off;         // reaches the gray calls only
    float guard_scale, tie_scale;
    bool keyed = false;       // a keyed block order (svs_embed_ordered_dev / svs_extract_ordered_dev; gray calls only)
    bool readback = false;    // SVS_READBACK (the gray embed calls; svs_embed_bgr_readback*; svs_embed_dithered_readback*)
    bool nearest = false;     // SVS_NEAREST (every embed call)
    bool minmove = false;     // SVS_MINMOVE (every embed call)
    // a coefficient selection (svs_embed_select* / svs_extract_select*; gray calls only): NULL for none, else its table with
    // count == n_ac.  The prefix 1..n_ac plans exactly as no selection does; any other one runs the lane-per-block exact
    // kernels in every mode - the streaming embed guard and the FAST extract margins (tools/guard_bound.py) are derived for
    // row-major prefixes only.
    const CoeffTable *coeffs = nullptr;
    // a keyed dither (svs_embed_dithered* / svs_extract_dithered*; gray calls only): the lane-per-block exact kernels with all
    // eight coefficient rows in every mode, as a non-prefix selection - the streaming guard and the FAST extract tie margins
    // are derived for an undithered quantiser input
    bool dithered = false;
    // a soft call (svs_soft_extract*; gray extract only): the eight-row pocketfft-identical extract kernel in every mode, with a
    // prefix, a selection, a dither or an order - the reliability is a distance of the reference's own quantiser input
    bool soft = false;
    // a vote call (svs_soft_vote*): a soft call whose bytes are added into a tally instead of written (SoftArgs::vote)
    bool vote = false;
    // a histogram call (svs_soft_histogram*): a soft call whose bytes are counted per frame instead of written (SoftArgs::hist);
    // never keyed - the counts of a frame do not depend on an order
    bool hist = false;
    // per-coefficient steps (svs_stepped_embed* / svs_stepped_extract* / svs_stepped_soft_*; gray calls only): the lane-per-block
    // exact kernels with all eight coefficient rows in every mode, in the instantiations that hold the stepped side
    // (svs_device.hpp) - QM_DOUBLE for an embed, QM_POW2 for an extract - whatever `delta` says; the callers pass a positive
    // one, and no kernel reads it
    bool stepped = false;
    // svs_stepped_embed_readback_margin*: the gate of the soft-margin pass that follows the stepped read-back, 0..127 (0: no such
    // pass).  Read only with stepped and readback.
    uint32_t min_margin = 0;
    // a matrix call (svs_matrix_embed* / svs_matrix_extract*; stepped, never with readback): StepArgs::matrix()'s word, k in bits
    // 0..2 and the pair search in bit 3 (make_matrix_word).  n_ac is then k, the stream bits a block carries - capacity, stream
    // positions and budgets are those of k - while the table the stepped side reads has 2^k - 1 slots: the call's selection
    // (coeffs, whose count is NOT n_ac here) or the prefix table of 2^k - 1.
    uint32_t matrix = 0;
};

// the word of a matrix call and the slots of its table
inline uint32_t make_matrix_word(uint32_t k, uint32_t search) { return k | (search ? 8u : 0u); }
inline uint32_t matrix_slots(uint32_t word) { return (1u << (word & 7u)) - 1u; }
// the slots of the table a stepped side reads where the call has no selection: n_ac, or a matrix call's 2^k - 1
inline uint32_t stepped_slots(uint32_t n_ac, uint32_t matrix) { return matrix ? matrix_slots(matrix) : n_ac; }
inline StepArgs matrix_steps(const StepArgs &steps, uint32_t matrix) {
    StepArgs s = steps;
    s.on |= matrix << SVS_STEP_MATRIX_SHIFT;
    return s;
}

inline bool route_selected(const RouteArgs &a) {
    return a.coeffs && a.coeffs->count != 0 && !coeff_table_is_prefix(*a.coeffs);
}

// COPY: nothing to embed and an empty payload - the reference's loops break before the first block.  Gray: a byte copy through
// embed_row1_kernel<QM_F32> (none when the call is in place); BGR: the BGR -> gray -> BGR conversion of embed_bgr_kernel<1>.
// ROUND_TRIP: a non-empty payload of which nothing can be embedded (delta <= 0, no coefficients): the reference still enters
// and round-trips every block (config_and_setup.py:143-145,166-169), which only the exact arithmetic reproduces - the exact
// kernel with n_ac = 0 and one pass bit.
// EXACT: the lane-per-block pocketfft arithmetic.  STREAMING: the cheap arithmetic with its rigorous guard and in-kernel exact
// replay of the blocks it cannot decide.  Every path produces the reference's stego pixels.
enum class EmbedPath { COPY, ROUND_TRIP, EXACT, STREAMING };

struct EmbedPlan {
    EmbedPath path;
    int qm;                   // QuantMode of the instantiation
    int rows;                 // coefficient rows of the instantiation (EXACT / ROUND_TRIP: the U of the exact kernel)
    bool two_blocks;          // embed_row1_kernel may take two blocks per lane where the buffers allow it
    bool keyed;               // the KEYED instantiation of the family (STREAMING / EXACT only: the other paths do not depend on order)
    bool readback;            // SVS_READBACK: readback_kernel follows the embed (only when payload bits are embedded)
    bool nearest;             // SVS_NEAREST: Geometry::pad of the embed launch (the kernels' QimRule)
    bool minmove;             // SVS_MINMOVE: likewise (rule_word(nearest, minmove, half_cell)); implies the nearest direction
    float half_cell;          // SVS_MINMOVE: h = (float)(0.5 * (double)delta), rounded here once for host and device
    uint32_t n_ac;            // Geometry::n_ac of the launch
    uint32_t xcd_chunk;
    QimParams qp;
    uint64_t use;             // payload bits embedded (*n_embedded)
    uint64_t bit_offset, n_bits, n_words;   // the kernel's payload arguments; n_words >= 2^32: too large for one call
    bool selected;            // the launch passes the call's CoeffTable (EXACT with rows = 8 only), else an empty one
    bool dithered;            // the launch switches the exact kernel's dithered side on (EXACT with rows = 8 only)
    bool stepped = false;     // the launch passes the call's StepArgs (EXACT with rows = 8 and QM_DOUBLE only), else an empty one
    uint32_t min_margin = 0;  // stepped with readback: a second readback_kernel launch, the margin pass, follows with this gate
    uint32_t matrix = 0;      // stepped: the matrix word the launch puts into StepArgs::on (0: none); n_ac is then k
};

// Which kernel family (include/svsdct.h `flags`).  The streaming kernels cover one and two coefficient rows (n <= 15) inside the
// guard's delta range and serve flags 0 and SVS_EXACT_GUARDED alike; everything else - n >= 16, delta outside the range,
// SVS_EXACT_POCKETFFT - runs the lane-per-block pocketfft kernel.
inline EmbedPlan plan_embed(const RouteArgs &a) {
    EmbedPlan p{};
    const uint32_t n = a.n_ac;
    const uint64_t cap = a.total_blocks * n;
    p.use = a.n_bits < cap ? a.n_bits : cap;
    if (!(a.delta > 0.0) || n == 0) p.use = 0;   // nothing can be embedded (config_and_setup.py:143-145)
    const bool selected = route_selected(a);
    const int rows = selected || a.dithered || a.stepped ? 8 : rows_for((int)n);
    const bool in_range = a.delta >= SVS_GUARD_DELTA_MIN && a.delta <= SVS_GUARD_DELTA_MAX;
    const bool streaming = p.use > 0 && in_range && !a.pocketfft && rows <= 2 && !(a.guarded_off && !a.bgr);   // never selected or dithered: rows = 8
    p.xcd_chunk = kEighth;
    const int qm = make_qim(p.use == 0 ? 1.0 : a.delta, &p.qp);
    if (p.use > 0) {
        p.path = streaming ? EmbedPath::STREAMING : EmbedPath::EXACT;
        p.qm = a.stepped ? (int)QM_DOUBLE : qm;   // stepped: the holder of the stepped side, whose arithmetic reads no QimParams
        p.n_ac = n;
        p.bit_offset = a.bit_offset;
        p.n_bits = p.use;
        const uint64_t end = a.bit_offset + p.use;   // the callers refuse a sum that wraps
        p.n_words = end / 32 + (end % 32 != 0);      // dwords that hold bits [0, end): no rounding term that could wrap
        // the BGR exact kernel covers all eight rows; the gray one has instantiations for one, two and eight
        p.rows = streaming || (!a.bgr && rows <= 2) ? rows : 8;
        p.two_blocks = streaming && !a.bgr && rows == 1;
        p.keyed = a.keyed;
        p.readback = a.readback;
        p.nearest = a.nearest;                // STREAMING and EXACT only: the other paths have no coefficient to force
        p.minmove = a.minmove;                // likewise
        p.half_cell = a.minmove ? (float)(0.5 * a.delta) : 0.0f;
        p.selected = selected;                // likewise: the other paths touch no coefficient
        p.dithered = a.dithered;              // likewise (EXACT with rows = 8)
        p.stepped = a.stepped;                // likewise (EXACT with rows = 8, never STREAMING: rows = 8)
        p.min_margin = a.stepped && a.readback ? a.min_margin : 0u;
        p.matrix = a.stepped ? a.matrix : 0u;
        if (streaming) {
            make_guard(a.delta, rows, &p.qp);
            p.qp.g_sum *= a.guard_scale; p.qp.g_resid *= a.guard_scale; p.qp.g_delta *= a.guard_scale;
        }
        return p;
    }
    // nothing to embed: the gray calls take the F32 instantiations, the BGR calls those of make_qim(1.0); only the BGR calls
    // pass their bit_offset on
    p.path = a.n_bits == 0 ? EmbedPath::COPY : EmbedPath::ROUND_TRIP;
    p.qm = a.bgr ? qm : QM_F32;
    p.n_ac = p.path == EmbedPath::COPY ? 1 : 0;
    p.rows = p.path == EmbedPath::COPY ? 1 : 8;
    p.two_blocks = p.path == EmbedPath::COPY && !a.bgr && rows == 1;
    p.bit_offset = a.bgr ? a.bit_offset : 0;
    p.n_bits = p.path == EmbedPath::COPY ? 0 : 1;
    return p;
}

// ZEROS: delta <= 0 - every bit '0' (config_and_setup.py:143-145).  EXACT: the pocketfft-identical forward transform.  FAST:
// the FMA-factored forward whose bits are the reference's for any input by construction (a block with a quantiser input within
// the proven error bound of a rounding tie is recomputed with the pocketfft-identical one).
enum class ExtractPath { ZEROS, EXACT, FAST };

struct ExtractPlan {
    ExtractPath path;
    int qm;                   // QM_F32 or QM_POW2: the double mode only differs in requantisation, not needed here
    int rows;
    uint32_t xcd_chunk;
    QimParams qp;
    bool keyed;               // the KEYED instantiation of the family (not ZEROS: all bits 0 in any order)
    bool selected;            // the launch passes the call's CoeffTable (EXACT with rows = 8 only), else an empty one
    bool dithered;            // the launch switches the exact kernel's dithered side on (EXACT with rows = 8; not ZEROS)
    bool soft;                // the launch switches the exact kernel's soft side on (EXACT with rows = 8; ZEROS: every byte 0)
    uint32_t n_ac;            // soft: bytes per block, the count of the table the soft side reads
    bool vote = false;        // soft, and the launch switches the soft side's vote tail on: `out` is the tally (never ZEROS)
    bool hist = false;        // soft, and the launch switches the soft side's histogram tail on: `out` is n_frames * 256 uint32
                              // counts, added to; the launch requests 256 more dwords of dynamic LDS (never ZEROS, never keyed)
    bool stepped = false;     // the launch passes the call's StepArgs (EXACT with rows = 8 and QM_POW2; never ZEROS, never FAST)
    uint32_t matrix = 0;      // stepped: the matrix word the launch puts into StepArgs::on (0: none); n_ac is then k
};

// Tile maps (measured on MI355X, profiles/history/r02_ab_extract_chunk.txt): one coefficient row - runs of 32 tiles per XCD
// (+3 %); two rows of the gray kernel (n = 8..15) - the identity map (+6.7 % at 600 x 4K, +4.4 % at 2 400 x 1080p over the
// contiguous eighth); more rows - VALU-bound, the map does not matter.
inline ExtractPlan plan_extract(const RouteArgs &a) {
    ExtractPlan p{};
    p.soft = a.soft || a.vote || a.hist;
    p.vote = a.vote;
    p.hist = a.hist;
    p.n_ac = a.n_ac;
    if (!(a.delta > 0.0)) {
        p.path = ExtractPath::ZEROS;
        return p;
    }
    p.selected = route_selected(a);
    p.dithered = a.dithered;
    p.stepped = a.stepped;
    p.matrix = a.stepped ? a.matrix : 0u;
    p.rows = p.selected || p.dithered || p.soft || p.stepped ? 8 : rows_for((int)a.n_ac);
    p.xcd_chunk = p.rows == 1 ? 32u : (p.rows == 2 && !a.bgr ? 0u : kEighth);
    p.qm = make_qim(a.delta, &p.qp) == QM_POW2 || p.stepped ? QM_POW2 : QM_F32;   // stepped: the holder of the stepped side
    const float t = a.tie_scale;
    p.qp.tie_slope *= t; p.qp.tie2_sum *= t; p.qp.tie2_resid *= t; p.qp.tie2_c00 *= t; p.qp.tie2_max *= t;
    // GUARDED = FAST inside the guard's delta range (n >= 8: 0.86 instead of 1.03 ms per 600 x 4K at n = 10), the
    // pocketfft-identical kernels outside it, as for embedding.  The BGR call has no flags.
    bool exact = a.pocketfft;
    if (a.guarded) exact = !(a.delta >= SVS_GUARD_DELTA_MIN && a.delta <= SVS_GUARD_DELTA_MAX && !a.guarded_off);
    if (a.bgr) exact = false;
    // the FAST kernels with two and more rows round c / delta by adding 1.5 * 2^23, which needs |c / delta| < 2^22.  With one
    // row the pocketfft-identical forward costs 0.2-3 % (the kernel stays HBM-bound; profiles/history/r01_ab_quant_exact.txt),
    // so FAST mode uses it too; with more rows it costs ~17 % and stays opt-in.
    if ((double)p.qp.delta_f < SVS_FAST_EXTRACT_DELTA_MIN || p.rows == 1 || p.selected || p.dithered || p.soft || p.stepped) exact = true;
    p.path = exact ? ExtractPath::EXACT : ExtractPath::FAST;
    p.keyed = a.keyed && !a.hist;
    return p;
}

// ---- what a launch passes for the call's order, selection and dither ----------------------------------------------------------
// A gray call's options in the kernels' forms (csrc/svs_capi.hip derives them once per call).  ord: the order of a keyed call;
// coeffs: the table of a non-prefix selection, NULL for none; dith: seed and first_frame of the call's dither - `on` and `sel`
// are set by the rules below.  All zero: the plain call.
struct KernelOptions {
    BlockOrderArgs ord;
    const CoeffTable *coeffs;
    DitherArgs dith;
    uint64_t vote_period = 0, vote_bit0 = 0;   // a vote call: the payload length in bits and the call's first stream position
    StepArgs steps{};                          // a stepped call: its table (on = 1), else empty
};

struct LaunchTables {   // the `sel` and `dith` arguments of the two exact kernels, and extract_exact_kernel's `soft`
    CoeffTable sel;
    DitherArgs dith;
    SoftArgs soft;
    StepArgs steps{};   // the `steps` argument of the two exact kernels: the call's where the plan is stepped, else empty
};

// embed_exact_kernel: `sel` is the call's selection where the plan is selected, else empty (count 0: the row-major prefix).  The
// dither is on only where the plan says so (EXACT, rows = 8); the dithered side runs the selected loop alone, with the prefix
// table of n_ac where the call has no selection.  The stepped side reads that table too, with the dither on or off; a matrix
// call's has 2^k - 1 slots (stepped_slots) and its StepArgs carry the matrix word.
inline LaunchTables embed_tables(const EmbedPlan &p, const KernelOptions &k) {
    const CoeffTable sel = p.selected && k.coeffs ? *k.coeffs : CoeffTable{};
    return {sel, {k.dith.seed, k.dith.first_frame, p.dithered ? 1u : 0u,
                  !(p.dithered || p.stepped) ? CoeffTable{} : sel.count ? sel : make_prefix_table(stepped_slots(p.n_ac, p.matrix))},
            SoftArgs{}, p.stepped ? matrix_steps(k.steps, p.matrix) : StepArgs{}};
}

// readback_kernel's keyed form (a selected or dithered plan): one table, the call's selection or the prefix table of n_ac
inline DitherArgs readback_tables(const EmbedPlan &p, const KernelOptions &k) {
    return {k.dith.seed, k.dith.first_frame, p.dithered ? 1u : 0u, p.selected && k.coeffs ? *k.coeffs : make_prefix_table(p.n_ac)};
}

// readback_kernel's stepped form as the margin pass (svs_stepped_embed_readback_margin*): the call's table with the gate in the
// spare bits of `on` (StepArgs::margin_gate), so that no kernel signature changes.  gate 0: the table as it is, the read-back.
inline StepArgs margin_steps(const StepArgs &steps, uint32_t gate) {
    StepArgs s = steps;
    s.on = 1u | (gate << SVS_STEP_GATE_SHIFT);
    return s;
}

// extract_exact_kernel reads the selection from `sel` on either hard side: their dither carries no table.  The soft side runs
// the selected loop alone and reads its own copy from the dither's table, never empty: the call's selection, or the prefix
// table of n_ac (as embed_exact_kernel's dithered side)
// The stepped side runs the selected loop alone and reads it from `sel`: the call's selection, or the prefix table of n_ac.
// A stepped soft call (svs_stepped_soft_*: soft, vote or hist, and stepped) is planned EXACT with eight rows and QM_POW2 by
// plan_extract's own rules and gets both: the soft side's table and SoftArgs as a soft call (half and scale are those of the
// route's delta and are not read: the stepped byte takes them from its coefficient's step) and the call's StepArgs.
inline LaunchTables extract_tables(const ExtractPlan &p, const KernelOptions &k) {
    const CoeffTable own = p.selected && k.coeffs ? *k.coeffs : CoeffTable{};
    const CoeffTable sel = p.stepped && !own.count ? make_prefix_table(stepped_slots(p.n_ac, p.matrix)) : own;
    return {sel,
            {k.dith.seed, k.dith.first_frame, p.dithered ? 1u : 0u, !p.soft ? CoeffTable{} : sel.count ? sel : make_prefix_table(p.n_ac)},
            !p.soft  ? SoftArgs{}
            : p.vote ? make_vote_args(make_soft_args(p.qp.delta_f, p.n_ac), k.vote_period, k.vote_bit0)
            : p.hist ? make_hist_args(make_soft_args(p.qp.delta_f, p.n_ac))
                     : make_soft_args(p.qp.delta_f, p.n_ac),
            p.stepped ? matrix_steps(k.steps, p.matrix) : StepArgs{}};
}

}  // namespace svs
