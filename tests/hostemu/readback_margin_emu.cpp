// Test-only: the one-lane forms of the stepped read-back and of the margin pass behind it (csrc/svs_readback.hpp
// readback_step_stepped, margin_step_stepped: the arithmetic the device runs on eight lanes) compiled for the host, walked over a
// batch as readback_kernel's stepped body walks it - twice, as svs_stepped_embed_readback_margin* launches it twice
// (tests/readback_margin_lib.py compiles this file once per process, with -ffp-contract=off as the host emulation is).
#include <cmath>
#include <cstdint>
#include <cstring>

#include "svs_readback.hpp"
#include "svs_route.hpp"

// Both passes in place over `frames` ([F][H][W], contiguous): the stego of svs_stepped_embed with the same arguments.  The
// arguments of stepped_readback_emu (tests/hostemu/stepped_readback_emu.cpp) and min_margin, the gate.  status1 / status2 (one byte
// per physical block, raster order over the batch): the per-block step of pass 1 (0 reads back, 1 repaired, 2 left) and of pass 2
// (0 strong throughout, 1 strengthened, 2 weak, 4 skipped for a wrong bit; all 0 when min_margin = 0: the pass does not run); 3
// carries no payload.  counts: {repaired, unrepaired, strengthened, weak}, added to.  Returns 0, or -1 for a selection, a table or
// a gate the library would refuse.
extern "C" int readback_margin_emu(uint8_t *frames, int F, int H, int W, const uint16_t *delta, const uint8_t *index, int count,
                                   const uint8_t *bits, uint64_t bits_bytes, uint64_t bit_offset, uint64_t n_bits, int dithered,
                                   uint64_t dither_key, int order, uint64_t order_key, uint32_t first_frame, uint32_t min_margin,
                                   uint8_t *status1, uint8_t *status2, uint64_t *counts) {
    svs::CoeffTable sel;
    if (!svs::make_coeff_table(index, (uint32_t)count, &sel) || count == 0) return -1;
    uint16_t table[64];
    memcpy(table, delta, sizeof table);
    for (int k = 1; k < 64; ++k)
        if (table[k] < 1 || table[k] > 4095) return -1;
    if (min_margin > 127) return -1;
    const svs::StepArgs steps = svs::make_step_args(table);
    const uint64_t wb = (uint64_t)W / 8, bpf = wb * ((uint64_t)H / 8), total = bpf * (uint64_t)F;
    // the library's route of the call (csrc/svs_capi.hip: delta = 1.0, stepped, read-back, the gate)
    svs::RouteArgs ra{1.0, (uint32_t)count, total, n_bits, bit_offset, false, false, false, false, 1.0f, 1.0f};
    ra.keyed = order != 0;
    ra.dithered = dithered != 0;
    ra.coeffs = svs::coeff_table_is_prefix(sel) ? nullptr : &sel;
    ra.stepped = true;
    ra.readback = true;
    ra.min_margin = min_margin;
    const svs::EmbedPlan p = svs::plan_embed(ra);
    memset(status1, 3, total);
    memset(status2, 3, total);
    if (p.use == 0) return 0;
    const svs::BlockOrderArgs ord = svs::make_block_order(order_key, first_frame, (uint32_t)bpf);
    const uint32_t seed = svs::dither_seed(dither_key);
    const uint32_t n = (uint32_t)count, n_words = (uint32_t)(bits_bytes / 4);
    // the gate as the launch carries it and the kernel reads it
    const float gate = (float)svs::margin_steps(steps, p.min_margin).margin_gate();
    for (int pass = 1; pass <= (p.min_margin > 0 ? 2 : 1); ++pass) {
        for (uint64_t gb = 0; gb < total; ++gb) {
            const uint64_t f = gb / bpf, b = gb % bpf;
            // the stream slot of the block under the keyed order; the dither is that of its PHYSICAL position
            const uint64_t slot = order ? svs::block_to_slot((uint32_t)b, ord, svs::round_keys(ord, ord.first_frame + (uint32_t)f)) : b;
            const uint64_t first = (f * bpf + slot) * n;
            const uint32_t nb = svs::block_budget(first, p.n_bits, n);
            if (nb == 0) continue;
            uint8_t *px = frames + f * (uint64_t)H * W + (b / wb) * 8 * W + (b % wb) * 8;
            uint32_t rx[8], ry[8];
            for (int r = 0; r < 8; ++r) {
                memcpy(&rx[r], px + (size_t)r * W, 4);
                memcpy(&ry[r], px + (size_t)r * W + 4, 4);
            }
            uint32_t hi, lo;
            svs::payload_window(reinterpret_cast<const uint32_t *>(bits), n_words, p.bit_offset + first, hi, lo);
            const uint32_t s_b = svs::dither_block_seed(seed, first_frame + (uint32_t)f, (uint32_t)b);
            uint32_t st;
            if (pass == 1) {
                st = svs::readback_step_stepped(rx, ry, sel, steps, nb, hi, lo, dithered != 0, s_b);
                status1[gb] = (uint8_t)st;
            } else {
                st = svs::margin_step_stepped(rx, ry, sel, steps, nb, hi, lo, dithered != 0, s_b, gate);
                status2[gb] = (uint8_t)(st == 0 && status1[gb] == 2 ? 4 : st);
            }
            if (st == 1)
                for (int r = 0; r < 8; ++r) {
                    memcpy(px + (size_t)r * W, &rx[r], 4);
                    memcpy(px + (size_t)r * W + 4, &ry[r], 4);
                }
            counts[2 * (pass - 1)] += st == 1;
            counts[2 * (pass - 1) + 1] += st == 2;
        }
        if (pass == 1 && p.min_margin == 0)
            for (uint64_t gb = 0; gb < total; ++gb)
                if (status1[gb] != 3) status2[gb] = 0;
    }
    return 0;
}
