// Test-only: the stepped block bodies (csrc/svs_block.hpp embed_block_stepped / extract_block_stepped, the code the kernels run
// per lane) and the stepped route (csrc/svs_route.hpp) compiled for the host, so that the CPU tier can hold them against the
// NumPy model of the format (tests/test_stepped_cpu.py compiles this file itself, with -ffp-contract=off as the host emulation is).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>

#include "svs_route.hpp"

namespace {

void load_block(const uint8_t *p, uint32_t (&rx)[8], uint32_t (&ry)[8]) {
    for (int r = 0; r < 8; ++r) {
        memcpy(&rx[r], p + 8 * r, 4);
        memcpy(&ry[r], p + 8 * r + 4, 4);
    }
}

void store_block(uint8_t *p, const uint32_t (&rx)[8], const uint32_t (&ry)[8]) {
    for (int r = 0; r < 8; ++r) {
        memcpy(p + 8 * r, &rx[r], 4);
        memcpy(p + 8 * r + 4, &ry[r], 4);
    }
}

svs::StepArgs steps_of(const uint16_t *delta) {
    uint16_t table[64];
    memcpy(table, delta, sizeof table);
    return svs::make_step_args(table);
}

}  // namespace

// One frame's blocks in raster order (block b is raster block b of clip frame t), 64 bytes each, rows of 8.  index / count: the
// selection (the prefix 1..n of a call without one).  bits: n_bits values 0 / 1, the stream from the frame's first slot; block b
// takes slots b * count ..; a block past the budget is copied.  rule: a QimRuleKind.  dithered: the dither of (key, t).
// Returns 0, or -1 for a selection the library would refuse.
extern "C" int stepped_emu_embed(const uint8_t *in, uint8_t *out, int64_t n_blocks, const uint16_t *delta, const uint8_t *index,
                                 int count, const uint8_t *bits, int64_t n_bits, int rule, int dithered, uint64_t key, uint32_t t) {
    svs::CoeffTable sel;
    if (!svs::make_coeff_table(index, (uint32_t)count, &sel) || count == 0) return -1;
    const svs::StepArgs steps = steps_of(delta);
    const uint32_t seed = svs::dither_seed(key);
    for (int64_t b = 0; b < n_blocks; ++b) {
        const int64_t first = b * count;
        if (first >= n_bits) {
            memcpy(out + 64 * b, in + 64 * b, 64);
            continue;
        }
        uint32_t hi = 0, lo = 0;
        for (int s = 0; s < count; ++s) {
            const uint32_t bit = first + s < n_bits ? (bits[first + s] & 1u) : 0u;
            if (s < 32) hi |= bit << (31 - s);
            else lo |= bit << (63 - s);
        }
        const uint32_t nb = svs::block_budget((uint64_t)first, (uint64_t)n_bits, (uint32_t)count);
        uint32_t rx[8], ry[8];
        load_block(in + 64 * b, rx, ry);
        if (dithered) svs::embed_block_stepped<true>(rx, ry, nb, hi, lo, (uint32_t)rule, sel, steps, svs::dither_block_seed(seed, t, (uint32_t)b));
        else svs::embed_block_stepped<false>(rx, ry, nb, hi, lo, (uint32_t)rule, sel, steps);
        store_block(out + 64 * b, rx, ry);
    }
    return 0;
}

// -> bits_out[b * count + s] = the parity read from block b for stream slot s
extern "C" int stepped_emu_extract(const uint8_t *in, int64_t n_blocks, const uint16_t *delta, const uint8_t *index, int count,
                                   int dithered, uint64_t key, uint32_t t, uint8_t *bits_out) {
    svs::CoeffTable sel;
    if (!svs::make_coeff_table(index, (uint32_t)count, &sel) || count == 0) return -1;
    const svs::StepArgs steps = steps_of(delta);
    const uint32_t seed = svs::dither_seed(key);
    for (int64_t b = 0; b < n_blocks; ++b) {
        uint32_t rx[8], ry[8], hi = 0, lo = 0;
        load_block(in + 64 * b, rx, ry);
        if (dithered) svs::extract_block_stepped<true>(rx, ry, sel, steps, hi, lo, svs::dither_block_seed(seed, t, (uint32_t)b));
        else svs::extract_block_stepped<false>(rx, ry, sel, steps, hi, lo);
        for (int s = 0; s < count; ++s) bits_out[b * count + s] = (uint8_t)svs::window_bit_at(hi, lo, (uint32_t)s);
    }
    return 0;
}

// The route of a stepped call as svs_capi.hip makes it: delta = 1.0, stepped = true.  flags: bit 0 SVS_EXACT_POCKETFFT, bit 1
// SVS_EXACT_GUARDED, bit 2 SVS_NEAREST, bit 3 SVS_MINMOVE, bit 4 a dither, bit 5 an order.  index / count: a selection, or NULL
// (the prefix 1..n_ac).  out (embed): path, rows, qm, stepped, selected, dithered, keyed, steps.on of the launch, count of the
// table the stepped side reads, use.  out (extract): path, rows, qm, stepped, selected, dithered, keyed, steps.on, count, 0.
extern "C" int stepped_emu_plan(int embed, int n_ac, uint64_t total, uint64_t n_bits, uint32_t flags, const uint8_t *index, int count,
                                const uint16_t *delta, int64_t *out) {
    svs::CoeffTable table;
    const svs::CoeffTable *coeffs = nullptr;
    if (index) {
        if (!svs::make_coeff_table(index, (uint32_t)count, &table)) return -1;
        coeffs = svs::coeff_table_is_prefix(table) ? nullptr : &table;
        n_ac = count;
    }
    svs::RouteArgs ra{1.0, (uint32_t)n_ac, total, n_bits, 0, (flags & 1u) != 0, (flags & 2u) != 0, false, false, 1.0f, 1.0f};
    ra.nearest = (flags & 4u) != 0;
    ra.minmove = (flags & 8u) != 0;
    ra.dithered = (flags & 16u) != 0;
    ra.keyed = (flags & 32u) != 0;
    ra.coeffs = coeffs;
    ra.stepped = true;
    svs::KernelOptions k{};
    k.coeffs = coeffs;
    k.steps = steps_of(delta);
    if (embed) {
        const svs::EmbedPlan p = svs::plan_embed(ra);
        const svs::LaunchTables t = svs::embed_tables(p, k);
        const int64_t v[10] = {(int64_t)p.path, p.rows, p.qm, p.stepped, p.selected, p.dithered, p.keyed, t.steps.on, t.dith.sel.count,
                               (int64_t)p.use};
        memcpy(out, v, sizeof v);
    } else {
        const svs::ExtractPlan p = svs::plan_extract(ra);
        const svs::LaunchTables t = svs::extract_tables(p, k);
        const int64_t v[10] = {(int64_t)p.path, p.rows, p.qm, p.stepped, p.selected, p.dithered, p.keyed, t.steps.on, t.sel.count, 0};
        memcpy(out, v, sizeof v);
    }
    return 0;
}
