// Test-only: the stepped soft block body (csrc/svs_block.hpp extract_block_stepped_soft, the code the kernel runs per lane), the
// soft block body it must equal under a uniform table (extract_block_soft) and the route of a stepped soft call
// (csrc/svs_route.hpp) compiled for the host, so that the CPU tier can hold them against the NumPy model of the format
// (tests/test_stepped_soft_cpu.py compiles this file itself, with -ffp-contract=off as the host emulation is).
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

svs::StepArgs steps_of(const uint16_t *delta) {
    uint16_t table[64];
    memcpy(table, delta, sizeof table);
    return svs::make_step_args(table);
}

}  // namespace

// One frame's blocks in raster order (block b is raster block b of clip frame t), 64 bytes each, rows of 8.  index / count: the
// selection (the prefix 1..n of a call without one).  dithered: the dither of (key, t).
// -> soft_out[b * count + s] = the byte of block b for stream slot s.  Returns 0, or -1 for a selection the library would refuse.
extern "C" int stepped_soft_emu_bytes(const uint8_t *in, int64_t n_blocks, const uint16_t *delta, const uint8_t *index, int count,
                                      int dithered, uint64_t key, uint32_t t, uint8_t *soft_out) {
    svs::CoeffTable sel;
    if (!svs::make_coeff_table(index, (uint32_t)count, &sel) || count == 0) return -1;
    const svs::StepArgs steps = steps_of(delta);
    const uint32_t seed = svs::dither_seed(key);
    for (int64_t b = 0; b < n_blocks; ++b) {
        uint32_t rx[8], ry[8];
        load_block(in + 64 * b, rx, ry);
        uint8_t *mine = soft_out + b * count;
        svs::extract_block_stepped_soft(rx, ry, sel, steps, dithered != 0, dithered ? svs::dither_block_seed(seed, t, (uint32_t)b) : 0u,
                                        [&](uint32_t s, uint32_t byte) { mine[s] = (uint8_t)byte; });
    }
    return 0;
}

// The same frame through extract_block_soft at one delta, in the quantiser mode and with the launch arguments the route gives a
// soft call at that delta (make_qim, make_soft_args): what a uniform table must reproduce.
extern "C" int stepped_soft_emu_uniform(const uint8_t *in, int64_t n_blocks, double delta, const uint8_t *index, int count,
                                        int dithered, uint64_t key, uint32_t t, uint8_t *soft_out) {
    svs::CoeffTable sel;
    if (!svs::make_coeff_table(index, (uint32_t)count, &sel) || count == 0) return -1;
    svs::QimParams qp{};
    const int qm = svs::make_qim(delta, &qp);
    const svs::SoftArgs sa = svs::make_soft_args(qp.delta_f, (uint32_t)count);
    const uint32_t seed = svs::dither_seed(key);
    for (int64_t b = 0; b < n_blocks; ++b) {
        uint32_t rx[8], ry[8];
        load_block(in + 64 * b, rx, ry);
        uint8_t *mine = soft_out + b * count;
        const uint32_t s_b = dithered ? svs::dither_block_seed(seed, t, (uint32_t)b) : 0u;
        const auto put = [&](uint32_t s, uint32_t byte) { mine[s] = (uint8_t)byte; };
        if (qm == svs::QM_POW2) svs::extract_block_soft<svs::QM_POW2>(rx, ry, sel, qp, sa, dithered != 0, s_b, put);
        else svs::extract_block_soft<svs::QM_F32>(rx, ry, sel, qp, sa, dithered != 0, s_b, put);
    }
    return 0;
}

// The route of a stepped soft call as svs_capi.hip makes it: delta = 1.0, stepped = true, and soft, vote or hist by `kind`
// (0 soft, 1 vote, 2 histogram).  flags: bit 0 SVS_EXACT_POCKETFFT, bit 1 SVS_EXACT_GUARDED, bit 4 a dither, bit 5 an order.
// index / count: a selection, or NULL (the prefix 1..n_ac).
// out: path, rows, qm, stepped, soft, vote, hist, keyed, steps.on, soft.on, soft.vote, soft.hist, count of the soft side's table,
// count of `sel`, dith.on, sizeof(SoftArgs)
extern "C" int stepped_soft_emu_plan(int kind, int n_ac, uint64_t total, uint32_t flags, const uint8_t *index, int count,
                                     const uint16_t *delta, uint64_t period, uint64_t bit0, int64_t *out) {
    svs::CoeffTable table;
    const svs::CoeffTable *coeffs = nullptr;
    if (index) {
        if (!svs::make_coeff_table(index, (uint32_t)count, &table)) return -1;
        coeffs = svs::coeff_table_is_prefix(table) ? nullptr : &table;
        n_ac = count;
    }
    svs::RouteArgs ra{1.0, (uint32_t)n_ac, total, 0, 0, (flags & 1u) != 0, (flags & 2u) != 0, false, false, 1.0f, 1.0f};
    ra.dithered = (flags & 16u) != 0;
    ra.keyed = (flags & 32u) != 0;
    ra.coeffs = coeffs;
    ra.stepped = true;
    ra.soft = kind == 0;
    ra.vote = kind == 1;
    ra.hist = kind == 2;
    svs::KernelOptions k{};
    k.coeffs = coeffs;
    k.steps = steps_of(delta);
    k.vote_period = period;
    k.vote_bit0 = bit0;
    const svs::ExtractPlan p = svs::plan_extract(ra);
    const svs::LaunchTables t = svs::extract_tables(p, k);
    const int64_t v[16] = {(int64_t)p.path, p.rows, p.qm, p.stepped, p.soft, p.vote, p.hist, p.keyed, t.steps.on, t.soft.on,
                           t.soft.vote, t.soft.hist, t.dith.sel.count, t.sel.count, t.dith.on, (int64_t)sizeof(svs::SoftArgs)};
    memcpy(out, v, sizeof v);
    return 0;
}
