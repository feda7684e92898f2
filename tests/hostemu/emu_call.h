// emu_call.h - TEST INFRASTRUCTURE ONLY: one gray call of the C ABI as tests/hostemu replays it on the CPU, and what the
// replay reports.  Plain C structs: tests/testlib.py mirrors both field for field as ctypes.Structure.  Each leads with its
// own sizeof and the entry points refuse a mismatch, so a layout that drifted fails loudly instead of reading garbage.  A new
// feature of the gray calls adds its field here (and to the mirror), not a new walker.
#pragma once
#include <stdint.h>

// which bodies the embed walker runs on the blocks that carry payload: the ones the kernels launch, or a form no kernel runs
// that the CPU tier holds against them
enum EmuVariant {
    EMU_AS_LAUNCHED = 0,
    EMU_PAIR_FORM = 1,            // even / odd block pairs through embed_block_exact_pair
    EMU_CONSTANT_SHORTCUT = 2,    // constant blocks take forward_exact_paired_constant, as the replay kernel does
    EMU_GENERIC_GUARDED2 = 3,     // the two-row guard through its generic instantiation <QM, 0, false>
};

// what an extract call writes, named as csrc/svs_capi.hip names it (ExtractOutput::Kind)
enum EmuOutput { EMU_BITS = 0, EMU_SOFT = 1, EMU_VOTE = 2, EMU_HIST = 3 };

struct EmuCall {
    uint64_t size;                // sizeof(EmuCall)
    // frames: contiguous [F][H][W].  embed: in -> out; extract: in; read-back: out, in place
    const uint8_t *frames_in;
    uint8_t *frames_out;
    int32_t F, H, W;
    int32_t n_ac;                 // clamped to 0..63 as the library does; ignored with a selection, as in the C ABI
    double delta;
    const uint8_t *index;         // a coefficient selection: `count` flat indices, count = 0 for the prefix 1..n_ac
    int32_t count;
    int32_t pocketfft, guarded;   // the SVS_EXACT_POCKETFFT / SVS_EXACT_GUARDED bits of the call's flags
    const uint8_t *bits;          // payload, packed MSB-first, padded by the caller to a multiple of 4 bytes
    uint64_t bits_bytes, bit_offset, n_bits;
    int32_t nearest, minmove;     // SVS_NEAREST / SVS_MINMOVE
    int32_t dither, order;        // a keyed dither / a keyed block order (read-back and the soft extracts: the others refuse it) is on
    uint64_t dither_key, order_key;
    uint32_t first_frame;         // frame f of the call is clip frame first_frame + f, for the dither and the order alike
    float guard_scale, tie_scale; // RouteArgs::guard_scale / tie_scale: the experiments library's SVS_GUARD_SCALE / SVS_TIE_SCALE
    int32_t force_qm;             // -1: the plan's quantiser mode, else that svs::QuantMode (the caller asks only for valid ones)
    int32_t exact_rows;           // U of the exact body of an EXACT plan: 0 = the plan's rows, as launch_embed dispatches; 8
    int32_t streaming_bodies;     // 0: a STREAMING embed plan / FAST extract plan runs the exact bodies on every block
    int32_t variant;              // EmuVariant
    int32_t extract_wave;         // 0: FAST extraction settles per block; 64: per wave of 64 blocks, as the kernels' ballot does
    int32_t keyed_form;           // read-back: readback_step_keyed (svs_embed_dithered_readback*) instead of readback_step<rows>
    int32_t output;               // extract: EmuOutput
    uint64_t vote_period, vote_bit0;   // EMU_VOTE: the payload's length in bits, the call's first stream position
    // optional outputs, one byte per block of the call in raster order over the batch; the caller zeroes them
    uint8_t *replay_map;          // embed: 1 = the streaming guard handed the block to the exact replay
    uint8_t *candidate_map;       // extract, wave mode: 1 = a candidate of step one
    uint8_t *status;              // read-back: 0 reads back, 1 repaired, 2 left unrepaired, 3 carries no payload
    uint8_t *bits_out;            // extract: one byte (0 / 1) per bit, n bits per block
    // the outputs of the soft kinds, each optional.  frames_in NULL: no walk at all - the result holds the call's plan
    uint8_t *soft_out;            // EMU_SOFT: one byte per capacity bit, in stream order
    int32_t *tally;               // EMU_VOTE: vote_period values, added to
    uint32_t *hist;               // EMU_HIST: F * 256 values, added to
};

struct EmuResult {
    uint64_t size;                // sizeof(EmuResult)
    uint64_t used;                // bits embedded / extracted; ~0: the library refuses the selection
    uint64_t replayed;            // embed: blocks handed to the exact replay; extract: blocks FAST mode redid exactly
    uint64_t repaired, unrepaired;   // read-back
    // the plan of the call (svs::EmbedPlan / svs::ExtractPlan)
    int32_t path, rows, qm, selected, dithered, nearest, minmove;
    uint32_t word;                // rule_word(nearest, minmove, half_cell): what the launchers put into Geometry::pad
    int32_t soft, vote, hist, keyed;   // extract
};
