// Test-only: the matrix block bodies (csrc/svs_block.hpp embed_block_matrix / extract_block_stepped + matrix_fold, the code the
// kernels run per lane) and the route of a matrix call (csrc/svs_route.hpp) compiled for the host, so that the CPU tier can hold
// them against the NumPy sender and receiver of the format (tests/matrix_lib.py compiles this file, with -ffp-contract=off).
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

svs::StepArgs steps_of(const uint16_t *delta, uint32_t word) {
    uint16_t table[64];
    memcpy(table, delta, sizeof table);
    return svs::matrix_steps(svs::make_step_args(table), word);
}

}  // namespace

// One frame's blocks in raster order, 64 bytes each, rows of 8 (clip frame t).  index / count: the selection, count == 2^k - 1.
// perm: NULL (raster), or perm[j] = the raster block at stream position j.  bits: n_bits values 0 / 1, the stream from the frame's
// first position; position j takes bits [j k, j k + k); a block past the budget is copied.  rule: a QimRuleKind.  dithered: the
// dither of (key, t) at the block's raster position.  Returns 0, or -1 for arguments the library would refuse.
extern "C" int matrix_emu_embed(const uint8_t *in, uint8_t *out, int64_t n_blocks, const uint16_t *delta, const uint8_t *index,
                                int count, int k, int search, const int64_t *perm, const uint8_t *bits, int64_t n_bits, int rule,
                                int dithered, uint64_t key, uint32_t t) {
    svs::CoeffTable sel;
    if (k < 1 || k > 6 || count != (1 << k) - 1 || !svs::make_coeff_table(index, (uint32_t)count, &sel)) return -1;
    const uint32_t word = svs::make_matrix_word((uint32_t)k, (uint32_t)search);
    const svs::StepArgs steps = steps_of(delta, word);
    const uint32_t seed = svs::dither_seed(key);
    float tile[126];   // the flipped forms, then the pair search's costs
    for (int64_t j = 0; j < n_blocks; ++j) {
        const int64_t b = perm ? perm[j] : j;
        const int64_t first = j * k;
        if (first >= n_bits) {
            memcpy(out + 64 * b, in + 64 * b, 64);
            continue;
        }
        uint32_t hi = 0;
        for (int s = 0; s < k; ++s) {
            // bits past the end of the stream are whatever the payload buffer holds: ones here, so that a body that forgot the
            // budget would be caught
            const uint32_t bit = first + s < n_bits ? (bits[first + s] & 1u) : 1u;
            hi |= bit << (31 - s);
        }
        const uint32_t nb = svs::block_budget((uint64_t)first, (uint64_t)n_bits, (uint32_t)k);
        uint32_t rx[8], ry[8];
        load_block(in + 64 * b, rx, ry);
        const uint32_t s_b = dithered ? svs::dither_block_seed(seed, t, (uint32_t)b) : 0u;
        if (dithered) svs::embed_block_matrix<true>(rx, ry, nb, hi, (uint32_t)rule, sel, steps, steps.matrix(), s_b, tile, 1u);
        else svs::embed_block_matrix<false>(rx, ry, nb, hi, (uint32_t)rule, sel, steps, steps.matrix(), s_b, tile, 1u);
        store_block(out + 64 * b, rx, ry);
    }
    return 0;
}

// -> bits_out[j * k + i] = stream bit i of the block at stream position j
extern "C" int matrix_emu_extract(const uint8_t *in, int64_t n_blocks, const uint16_t *delta, const uint8_t *index, int count, int k,
                                  const int64_t *perm, int dithered, uint64_t key, uint32_t t, uint8_t *bits_out) {
    svs::CoeffTable sel;
    if (k < 1 || k > 6 || count != (1 << k) - 1 || !svs::make_coeff_table(index, (uint32_t)count, &sel)) return -1;
    const svs::StepArgs steps = steps_of(delta, svs::make_matrix_word((uint32_t)k, 0u));
    const uint32_t seed = svs::dither_seed(key);
    for (int64_t j = 0; j < n_blocks; ++j) {
        const int64_t b = perm ? perm[j] : j;
        uint32_t rx[8], ry[8], hi = 0, lo = 0;
        load_block(in + 64 * b, rx, ry);
        if (dithered) svs::extract_block_stepped<true>(rx, ry, sel, steps, hi, lo, svs::dither_block_seed(seed, t, (uint32_t)b));
        else svs::extract_block_stepped<false>(rx, ry, sel, steps, hi, lo);
        if (steps.matrix()) svs::matrix_fold(hi, lo);
        for (int s = 0; s < k; ++s) bits_out[j * k + s] = (uint8_t)svs::window_bit_at(hi, lo, (uint32_t)s);
    }
    return 0;
}

// The route of a matrix call as svs_capi.hip makes it: delta = 1.0, stepped, n_ac = k, the matrix word.  flags: bit 2 SVS_NEAREST,
// bit 3 SVS_MINMOVE, bit 4 a dither, bit 5 an order.  index / count: the selection, or NULL (the prefix 1..2^k - 1).
// out: path, rows, qm, n_ac of the launch (embed; extract: the plan's), keyed, StepArgs::on of the launch, count of the table the
// stepped side reads, use (embed), dynamic LDS floats per wave of the launch (embed).
extern "C" int matrix_emu_plan(int embed, int k, int search, uint64_t total, uint64_t n_bits, uint32_t flags, const uint8_t *index,
                               int count, const uint16_t *delta, int64_t *out) {
    svs::CoeffTable table;
    const svs::CoeffTable *coeffs = nullptr;
    if (index) {
        if (!svs::make_coeff_table(index, (uint32_t)count, &table)) return -1;
        coeffs = svs::coeff_table_is_prefix(table) ? nullptr : &table;
    }
    svs::RouteArgs ra{1.0, (uint32_t)k, total, n_bits, 0, false, false, false, false, 1.0f, 1.0f};
    ra.nearest = (flags & 4u) != 0;
    ra.minmove = (flags & 8u) != 0;
    ra.dithered = (flags & 16u) != 0;
    ra.keyed = (flags & 32u) != 0;
    ra.coeffs = coeffs;
    ra.stepped = true;
    ra.matrix = svs::make_matrix_word((uint32_t)k, (uint32_t)search);
    svs::KernelOptions ko{};
    ko.coeffs = coeffs;
    ko.steps = steps_of(delta, 0u);
    if (embed) {
        const svs::EmbedPlan p = svs::plan_embed(ra);
        const svs::LaunchTables t = svs::embed_tables(p, ko);
        const int64_t v[9] = {(int64_t)p.path, p.rows, p.qm, p.n_ac, p.keyed, t.steps.on, t.dith.sel.count, (int64_t)p.use,
                              64 * (int64_t)svs::matrix_slots(p.matrix) * ((p.matrix & 8u) ? 2 : 1)};
        memcpy(out, v, sizeof v);
    } else {
        const svs::ExtractPlan p = svs::plan_extract(ra);
        const svs::LaunchTables t = svs::extract_tables(p, ko);
        const int64_t v[9] = {(int64_t)p.path, p.rows, p.qm, p.n_ac, p.keyed, t.steps.on, t.sel.count, 0, 0};
        memcpy(out, v, sizeof v);
    }
    return 0;
}
