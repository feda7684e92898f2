// CPU build of the keyed forms of csrc/svs_readback.hpp for tests/test_keyed_readback_cpu.py and
// tests/test_keyed_readback_gpu.py: the read-back pass of svs_embed_dithered_readback* (csrc/svs_device.hpp readback_keyed) block
// by block on the host, with the library's own routing (svs_route.hpp), payload windows, coefficient table, dither seed and
// keyed block order.  Always the keyed forms (readback_step_keyed), also for a prefix selection without a dither, so that the
// tests can hold them to readback_step there.  Build: g++ -O2 -ffp-contract=off -std=c++17 -shared -fPIC.
#include <cstdint>
#include <cstring>

#include "svs_order.hpp"
#include "svs_readback.hpp"
#include "svs_route.hpp"

extern "C" {

// In place on stego [F][H][W] (contiguous): the stego of the same call without read-back.  index / n_index: the selection
// (n_index 0: the row-major prefix 1..n_ac).  dithered: the dither (dkey) is on.  keyed: the block order (okey).  first_frame
// serves both.  bits: packed MSB-first, padded to a multiple of 4 bytes.  status[block] (optional): 0 reads back, 1 repaired,
// 2 left unrepaired, 3 carries no payload.  counts[0] / counts[1]: repaired / unrepaired.  Returns the bits the call
// embedded, or ~0 for a selection the library refuses.
uint64_t krb_readback(uint8_t *stego, int F, int H, int W, double delta, int n_ac, const uint8_t *index, int n_index,
                      int dithered, uint64_t dkey, int keyed, uint64_t okey, uint32_t first_frame, const uint8_t *bits,
                      uint64_t bits_bytes, uint64_t bit_offset, uint64_t n_bits, uint64_t *counts, uint8_t *status) {
    counts[0] = counts[1] = 0;
    uint32_t n = (uint32_t)(n_ac < 0 ? 0 : (n_ac > 63 ? 63 : n_ac));
    svs::CoeffTable table;
    if (n_index > 0) {
        if (!svs::make_coeff_table(index, (uint32_t)n_index, &table)) return ~0ull;
        n = (uint32_t)n_index;
    } else {
        table = svs::make_prefix_table(n);
    }
    const uint64_t wb = (uint64_t)W / 8, bpf = wb * (uint64_t)(H / 8), total = bpf * (uint64_t)F;
    svs::RouteArgs ra{delta, n, total, n_bits, bit_offset, false, true, false, false, 1.0f, 1.0f};
    ra.keyed = keyed != 0;
    ra.readback = true;
    ra.coeffs = &table;
    ra.dithered = dithered != 0;
    const svs::EmbedPlan p = svs::plan_embed(ra);
    if (status) std::memset(status, 3, total);
    if (p.use == 0) return 0;
    const svs::BlockOrderArgs ord = svs::make_block_order(okey, first_frame, (uint32_t)bpf);
    const uint32_t seed = svs::dither_seed(dkey);
    const uint32_t n_words = (uint32_t)(bits_bytes / 4);
    for (uint64_t gb = 0; gb < total; ++gb) {
        const uint64_t f = gb / bpf, b = gb % bpf;
        const uint64_t slot = keyed ? svs::block_to_slot((uint32_t)b, ord, svs::round_keys(ord, ord.first_frame + (uint32_t)f)) : b;
        const uint64_t first = (f * bpf + slot) * n;
        const uint32_t nb = svs::block_budget(first, p.n_bits, n);
        if (nb == 0) continue;
        uint8_t *px = stego + f * (uint64_t)H * W + (b / wb) * 8 * (uint64_t)W + (b % wb) * 8;
        uint32_t x[8], y[8];
        for (int r = 0; r < 8; ++r) { std::memcpy(&x[r], px + r * W, 4); std::memcpy(&y[r], px + r * W + 4, 4); }
        uint32_t hi, lo;
        svs::payload_window(reinterpret_cast<const uint32_t *>(bits), n_words, p.bit_offset + first, hi, lo);
        const uint32_t s_b = svs::dither_block_seed(seed, first_frame + (uint32_t)f, (uint32_t)b);   // the PHYSICAL position
        const bool dith = dithered != 0;
        uint32_t st = 0;
        if (p.qm == svs::QM_DOUBLE) st = svs::readback_step_keyed<svs::QM_DOUBLE>(x, y, table, nb, hi, lo, p.qp, dith, s_b);
        else if (p.qm == svs::QM_POW2) st = svs::readback_step_keyed<svs::QM_POW2>(x, y, table, nb, hi, lo, p.qp, dith, s_b);
        else st = svs::readback_step_keyed<svs::QM_F32>(x, y, table, nb, hi, lo, p.qp, dith, s_b);
        if (st == 1) {
            for (int r = 0; r < 8; ++r) { std::memcpy(px + r * W, &x[r], 4); std::memcpy(px + r * W + 4, &y[r], 4); }
            ++counts[0];
        } else if (st == 2) {
            ++counts[1];
        }
        if (status) status[gb] = (uint8_t)st;
    }
    return p.use;
}

}
