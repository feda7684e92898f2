// CPU build of csrc/svs_order.hpp for tests/test_block_order_cpu.py: the keyed block order of one frame, both directions.
#include <stdint.h>

#include "svs_order.hpp"

extern "C" {

// out[x] = sigma_t(x) (inverse = 0: slot -> block) or sigma_t^-1(x) (inverse = 1: block -> slot), x = 0 .. n_blocks - 1;
// first_frame + f = t is split as the kernels split it
void bo_map(uint64_t key, uint32_t first_frame, uint32_t f, uint32_t n_blocks, int inverse, uint32_t *out) {
    const svs::BlockOrderArgs o = svs::make_block_order(key, first_frame, n_blocks);
    const svs::RoundKeys rk = svs::round_keys(o, o.first_frame + f);
    for (uint32_t x = 0; x < n_blocks; ++x) out[x] = inverse ? svs::block_to_slot(x, o, rk) : svs::slot_to_block(x, o, rk);
}

uint32_t bo_lowbias32(uint32_t h) { return svs::lowbias32(h); }

}
