// Test-only: the requantisation channel's block body (csrc/svs_block.hpp requantise_block_exact, the code the kernel runs per
// lane) compiled for the host, so that the CPU tier can hold it against the NumPy model of the format
// (tests/test_requantise_cpu.py compiles this file itself, with -ffp-contract=off as the host emulation is).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>

#include "svs_block.hpp"

// in / out: n_blocks blocks of 64 bytes, rows of 8; steps: 64 values in 1..255 (the library's entry points check them)
extern "C" void channel_emu_blocks(const uint8_t *in, uint8_t *out, int64_t n_blocks, const uint16_t *steps) {
    uint16_t table[64];
    memcpy(table, steps, sizeof table);
    const svs::ChannelArgs chan = svs::make_channel_args(table);
    for (int64_t b = 0; b < n_blocks; ++b) {
        uint32_t rx[8], ry[8];
        for (int r = 0; r < 8; ++r) {
            memcpy(&rx[r], in + 64 * b + 8 * r, 4);
            memcpy(&ry[r], in + 64 * b + 8 * r + 4, 4);
        }
        svs::requantise_block_exact(rx, ry, chan);
        for (int r = 0; r < 8; ++r) {
            memcpy(out + 64 * b + 8 * r, &rx[r], 4);
            memcpy(out + 64 * b + 8 * r + 4, &ry[r], 4);
        }
    }
}
