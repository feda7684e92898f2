// hostemu.cpp - TEST INFRASTRUCTURE ONLY (never loaded by the product package).
//
// Runs csrc/svs_block.hpp - the exact per-block arithmetic and bit bookkeeping the gfx950 kernels
// execute - and csrc/svs_index.hpp - their tile maps, divisions and offsets - on the CPU, block by
// block, so that the CPU-only test tier (and ASan/UBSan) can check it against the oracle without a GPU.  The lane/wave mapping, HBM access and LDS bit packing of
// the kernels are NOT modelled here; those are covered by the -m gpu tests.
// Build: g++ -O2 -ffp-contract=off -std=c++17 -shared -fPIC -I<csrc> hostemu.cpp -o libsvs_hostemu.so
#include <cmath>
#include <cstdint>
#include <cstring>

#include "svs_block.hpp"
#include "svs_index.hpp"
#include "svs_route.hpp"
#include "svs_stage.hpp"

namespace {

using svs::make_qim;   // the host-side parameter set-up the library itself uses

struct Blk {
    uint32_t x[8], y[8];
    void load(const uint8_t *p, size_t pitch) {
        for (int r = 0; r < 8; ++r) {
            std::memcpy(&x[r], p + r * pitch, 4);
            std::memcpy(&y[r], p + r * pitch + 4, 4);
        }
    }
    void store(uint8_t *p, size_t pitch) const {
        for (int r = 0; r < 8; ++r) {
            std::memcpy(p + r * pitch, &x[r], 4);
            std::memcpy(p + r * pitch + 4, &y[r], 4);
        }
    }
};

// two adjacent blocks through the packed pair form (svs_block.hpp embed_block_exact_pair; no kernel runs it)
void embed_exact_pair_dispatch(Blk &a, Blk &b, uint32_t n, uint32_t nb_a, uint32_t nb_b, uint32_t hi_a, uint32_t lo_a,
                               uint32_t hi_b, uint32_t lo_b, const svs::QimParams &qp, int qm) {
    if (qm == svs::QM_DOUBLE) svs::embed_block_exact_pair<8, svs::QM_DOUBLE>(a.x, a.y, b.x, b.y, n, nb_a, nb_b, hi_a, lo_a, hi_b, lo_b, qp);
    else if (qm == svs::QM_POW2) svs::embed_block_exact_pair<8, svs::QM_POW2>(a.x, a.y, b.x, b.y, n, nb_a, nb_b, hi_a, lo_a, hi_b, lo_b, qp);
    else svs::embed_block_exact_pair<8, svs::QM_F32>(a.x, a.y, b.x, b.y, n, nb_a, nb_b, hi_a, lo_a, hi_b, lo_b, qp);
}

bool g_constant_shortcut = false;   // exact == 3: constant blocks take forward_exact_paired_constant, as the replay kernel does

// emu_set_guard_scale / emu_set_tie_scale: the experiments library's SVS_GUARD_SCALE / SVS_TIE_SCALE, applied by the routing
float g_guard_scale = 1.0f, g_tie_scale = 1.0f;

// the library's routing (csrc/svs_route.hpp) of a gray call

svs::RouteArgs route(double delta, uint32_t n, uint64_t total, uint64_t n_bits, uint64_t bit_offset, bool pocketfft, bool guarded) {
    return svs::RouteArgs{delta, n, total, n_bits, bit_offset, pocketfft, guarded, false, false, g_guard_scale, g_tie_scale};
}

uint8_t *g_replay_map = nullptr;   // emu_set_replay_map: one byte per block of the next emu_embed calls, 1 = handed to the replay

bool g_generic_guarded2 = false;    // exact == 5: the two-row guard through its generic instantiation only

// Two coefficient rows: the instantiation the KERNEL launches (csrc/svs_device.hpp embed_kernel, svs_capi.hip launch_embed) -
// compile-time n for the GUI's default 10, and for every quantiser but the power-of-two one the in-place form (truncated
// inverse, stego bytes written over the row dwords, an undecided block left half-written: the kernel rebuilds it from the
// rows it parked in LDS, the caller here from the frame).  exact == 5 forces <QM, 0, false> so that the CPU tier can hold
// the two against each other.
template <int QM>
bool guarded2_as_launched(Blk &raw, uint32_t n, uint32_t nb, uint32_t hi, uint32_t lo, const svs::QimParams &qp) {
    if (g_generic_guarded2) return svs::embed_block_guarded2<QM, 0, false>(raw.x, raw.y, n, nb, hi, lo, qp);
    constexpr bool INPLACE = QM != svs::QM_POW2;
    if (n == 10) return svs::embed_block_guarded2<QM, 10, INPLACE>(raw.x, raw.y, n, nb, hi, lo, qp);
    return svs::embed_block_guarded2<QM, 0, INPLACE>(raw.x, raw.y, n, nb, hi, lo, qp);
}

// GUARDED (exact == 4 / 5; FAST too at n <= 15): -> true when the block has to be redone with the exact arithmetic
bool embed_guarded_dispatch(Blk &raw, uint32_t n, uint32_t nb, uint32_t hi, uint32_t lo, const svs::QimParams &qp, int qm) {
    if (svs::rows_for((int)n) == 2) {   // two coefficient rows: the per-pixel rigorous guard
        if (qm == svs::QM_DOUBLE) return guarded2_as_launched<svs::QM_DOUBLE>(raw, n, nb, hi, lo, qp);
        if (qm == svs::QM_POW2) return guarded2_as_launched<svs::QM_POW2>(raw, n, nb, hi, lo, qp);
        return guarded2_as_launched<svs::QM_F32>(raw, n, nb, hi, lo, qp);
    }
    if (qm == svs::QM_DOUBLE) return svs::embed_block_guarded<svs::QM_DOUBLE>(raw.x, raw.y, n, nb, hi, lo, qp);
    if (qm == svs::QM_POW2) return svs::embed_block_guarded<svs::QM_POW2>(raw.x, raw.y, n, nb, hi, lo, qp);
    return svs::embed_block_guarded<svs::QM_F32>(raw.x, raw.y, n, nb, hi, lo, qp);
}

void embed_exact_dispatch(Blk &raw, uint32_t n, uint32_t nb, uint32_t hi, uint32_t lo, const svs::QimParams &qp, int qm) {
    bool constant = g_constant_shortcut;
    for (int r = 0; r < 8 && constant; ++r)
        constant = raw.x[r] == (raw.x[0] & 0xffu) * 0x01010101u && raw.y[r] == (raw.x[0] & 0xffu) * 0x01010101u;
    if (qm == svs::QM_DOUBLE) svs::embed_block_exact<8, svs::QM_DOUBLE>(raw.x, raw.y, n, nb, hi, lo, qp, constant);
    else if (qm == svs::QM_POW2) svs::embed_block_exact<8, svs::QM_POW2>(raw.x, raw.y, n, nb, hi, lo, qp, constant);
    else svs::embed_block_exact<8, svs::QM_F32>(raw.x, raw.y, n, nb, hi, lo, qp, constant);
}

// -> true: some quantiser input is within the forward error bound of a tie (svs::extract_block's return value)
template <int QM>
bool extract_dispatch(int rows, const Blk &raw, uint32_t n, const svs::QimParams &d, uint32_t &hi, uint32_t &lo) {
    if (n == 10) return svs::extract_block<2, QM, 10>(raw.x, raw.y, n, d, hi, lo);   // as csrc/svs_capi.hip
    switch (rows) {
        case 1: return svs::extract_block<1, QM>(raw.x, raw.y, n, d, hi, lo);
        case 2: return svs::extract_block<2, QM>(raw.x, raw.y, n, d, hi, lo);
        case 3: return svs::extract_block<3, QM>(raw.x, raw.y, n, d, hi, lo);
        case 4: return svs::extract_block<4, QM>(raw.x, raw.y, n, d, hi, lo);
        case 5: return svs::extract_block<5, QM>(raw.x, raw.y, n, d, hi, lo);
        case 6: return svs::extract_block<6, QM>(raw.x, raw.y, n, d, hi, lo);
        case 7: return svs::extract_block<7, QM>(raw.x, raw.y, n, d, hi, lo);
        default: return svs::extract_block<8, QM>(raw.x, raw.y, n, d, hi, lo);
    }
}

template <int QM>
void extract_fast(int rows, const Blk &raw, uint32_t n, const svs::QimParams &d, uint32_t &hi, uint32_t &lo, uint64_t *redone) {
    if (extract_dispatch<QM>(rows, raw, n, d, hi, lo)) {   // near a tie: the kernels redo the block exactly
        svs::extract_block_exact<8, QM>(raw.x, raw.y, n, d, hi, lo);
        if (redone) ++*redone;
    }
}

// emu_set_extract_wave(64): step two of FAST extraction for EVERY block of an aligned group of 64 blocks in which one block
// is a candidate, as the kernels do it (one wave ballot; extract_kernel / extract_bgr_kernel).  With the product's margin
// that gives the per-block result (svs_block.hpp, extract_block); with a margin scaled below 1 (emu_set_tie_scale) it need not.
int g_extract_wave = 0;   // 0: per block
uint8_t *g_candidate_map = nullptr;   // emu_set_candidate_map: one byte per block, 1 = a candidate of step one (wave mode only)

template <int QM>
bool extract_cheap_dispatch(int rows, const Blk &raw, uint32_t n, const svs::QimParams &d, uint32_t &hi, uint32_t &lo, float &off) {
    if (n == 10) return svs::extract_block_cheap<2, QM, 10>(raw.x, raw.y, n, d, hi, lo, off);
    switch (rows) {
        case 2: return svs::extract_block_cheap<2, QM>(raw.x, raw.y, n, d, hi, lo, off);
        case 3: return svs::extract_block_cheap<3, QM>(raw.x, raw.y, n, d, hi, lo, off);
        case 4: return svs::extract_block_cheap<4, QM>(raw.x, raw.y, n, d, hi, lo, off);
        case 5: return svs::extract_block_cheap<5, QM>(raw.x, raw.y, n, d, hi, lo, off);
        case 6: return svs::extract_block_cheap<6, QM>(raw.x, raw.y, n, d, hi, lo, off);
        case 7: return svs::extract_block_cheap<7, QM>(raw.x, raw.y, n, d, hi, lo, off);
        default: return svs::extract_block_cheap<8, QM>(raw.x, raw.y, n, d, hi, lo, off);
    }
}

// one wave of FAST extraction (rows >= 2): blocks [g0, g0 + count) of `raws`
template <int QM>
void extract_fast_wave(int rows, const Blk *raws, uint64_t count, uint32_t n, const svs::QimParams &d, uint32_t *his, uint32_t *los,
                       bool *cand, uint64_t *redone) {
    float off[128];
    bool any = false;
    for (uint64_t i = 0; i < count; ++i) {
        cand[i] = extract_cheap_dispatch<QM>(rows, raws[i], n, d, his[i], los[i], off[i]);
        any = any || cand[i];
    }
    if (!any) return;
    for (uint64_t i = 0; i < count; ++i) {
        if (svs::extract_block_settle<QM>(raws[i].x, raws[i].y, n, d, his[i], off[i])) {
            svs::extract_block_exact<8, QM>(raws[i].x, raws[i].y, n, d, his[i], los[i]);
            if (redone) ++*redone;
        }
    }
}

}  // namespace

extern "C" {

void emu_set_guard_scale(float f) { g_guard_scale = f; }
void emu_set_tie_scale(float f) { g_tie_scale = f; }
void emu_set_extract_wave(int blocks) { g_extract_wave = blocks; }   // 0: per block; 64: a wave of the extract kernels
void emu_set_candidate_map(uint8_t *map) { g_candidate_map = map; }   // nullptr: off
void emu_set_replay_map(uint8_t *map) { g_replay_map = map; }   // caller zeroes it; nullptr: off

// frames: contiguous [F][H][W]; bits: packed MSB-first, padded by the caller to a multiple of 4 bytes
uint64_t emu_embed(const uint8_t *gray, uint8_t *stego, int F, int H, int W, double delta, int n_ac,
                   const uint8_t *bits, uint64_t bits_bytes, uint64_t bit_offset, uint64_t n_bits, int exact,
                   uint64_t *n_replayed) {
    if (n_replayed) *n_replayed = 0;
    // exact: 0 = flags 0, 1 = SVS_EXACT_POCKETFFT, 4 = SVS_EXACT_GUARDED, routed as svs_embed_dev routes them.  The test-only
    // modes route as 1 (2: even/odd block pairs through the packed pair form; 3: the constant shortcut) and as 4 (5: the
    // two-row guard through its generic instantiation).  Every mode gives the reference's pixels.
    g_constant_shortcut = exact == 3;
    g_generic_guarded2 = exact == 5;
    const int n = n_ac < 0 ? 0 : (n_ac > 63 ? 63 : n_ac);
    const uint64_t bpf = (uint64_t)(H / 8) * (W / 8), total = bpf * F;
    std::memcpy(stego, gray, (size_t)F * H * W);
    const svs::EmbedPlan plan = svs::plan_embed(route(delta, (uint32_t)n, total, n_bits, bit_offset, exact >= 1 && exact <= 3,
                                                      exact == 4 || exact == 5));
    const uint64_t use = plan.use;
    const svs::QimParams &qp = plan.qp;
    const int dbl = plan.qm;
    const bool guarded = plan.path == svs::EmbedPath::STREAMING;
    if (use == 0) {
        if (plan.path == svs::EmbedPath::ROUND_TRIP) {  // nothing consumed -> every block entered and round-tripped
            for (uint64_t gb = 0; gb < total; ++gb) {
                const uint64_t f = gb / bpf, b = gb % bpf;
                uint8_t *p = stego + f * (uint64_t)H * W + (b / (W / 8)) * 8 * W + (b % (W / 8)) * 8;
                Blk raw;
                raw.load(p, (size_t)W);
                svs::embed_block_exact<8, svs::QM_F32>(raw.x, raw.y, 0, 0, 0, 0, qp);
                raw.store(p, (size_t)W);
            }
        }
        return 0;
    }
    const uint32_t n_words = (uint32_t)(bits_bytes / 4);
    for (uint64_t gb = 0; gb < total; ++gb) {
        const uint64_t first = gb * n;
        const uint32_t nb = svs::block_budget(first, use, (uint32_t)n);
        if (nb == 0) break;
        const uint64_t f = gb / bpf, b = gb % bpf;
        const uint64_t by = b / (W / 8), bx = b % (W / 8);
        uint8_t *p = stego + f * (uint64_t)H * W + by * 8 * W + bx * 8;
        Blk raw;
        raw.load(p, (size_t)W);
        uint32_t hi, lo;
        svs::payload_window(reinterpret_cast<const uint32_t *>(bits), n_words, bit_offset + first, hi, lo);
        if (exact == 2 && (W / 8) % 2 == 0 && gb % 2 == 0 && svs::block_budget(first + n, use, (uint32_t)n) > 0) {
            // exact == 2: even/odd block pairs through the packed pair form
            Blk other;
            other.load(p + 8, (size_t)W);
            uint32_t hi_b, lo_b;
            svs::payload_window(reinterpret_cast<const uint32_t *>(bits), n_words, bit_offset + first + n, hi_b, lo_b);
            embed_exact_pair_dispatch(raw, other, (uint32_t)n, nb, svs::block_budget(first + n, use, (uint32_t)n), hi, lo, hi_b,
                                      lo_b, qp, dbl);
            raw.store(p, (size_t)W);
            other.store(p + 8, (size_t)W);
            ++gb;
            continue;
        }
        if (guarded) {
            if (embed_guarded_dispatch(raw, (uint32_t)n, nb, hi, lo, qp, dbl)) {
                raw.load(p, (size_t)W);
                embed_exact_dispatch(raw, (uint32_t)n, nb, hi, lo, qp, dbl);
                if (n_replayed) ++*n_replayed;
                if (g_replay_map) g_replay_map[gb] = 1;
            }
        } else {
            embed_exact_dispatch(raw, (uint32_t)n, nb, hi, lo, qp, dbl);
        }
        raw.store(p, (size_t)W);
    }
    return use;
}

// out_flags: one byte (0/1) per extracted bit, F*(H/8)*(W/8)*n entries
uint64_t emu_extract(const uint8_t *gray, int F, int H, int W, double delta, int n_ac, uint8_t *out_flags, int exact,
                     uint64_t *n_redone) {
    if (n_redone) *n_redone = 0;
    const int n = n_ac < 0 ? 0 : (n_ac > 63 ? 63 : n_ac);
    const uint64_t bpf = (uint64_t)(H / 8) * (W / 8), total = bpf * F;
    if (n == 0) return 0;
    // exact != 0: SVS_EXACT_POCKETFFT, routed as svs_extract_dev routes it
    const svs::ExtractPlan plan = svs::plan_extract(route(delta, (uint32_t)n, total, 0, 0, exact != 0, false));
    if (plan.path == svs::ExtractPath::ZEROS) {
        std::memset(out_flags, 0, total * n);
        return total * n;
    }
    const svs::QimParams &qp = plan.qp;
    const int qm = plan.qm, rows = plan.rows;
    if (g_extract_wave > 0 && plan.path == svs::ExtractPath::FAST) {
        const uint64_t wv = (uint64_t)(g_extract_wave > 128 ? 128 : g_extract_wave);
        Blk raws[128];
        uint32_t his[128], los[128];
        for (uint64_t g0 = 0; g0 < total; g0 += wv) {
            const uint64_t count = total - g0 < wv ? total - g0 : wv;
            for (uint64_t i = 0; i < count; ++i) {
                const uint64_t gb = g0 + i, f = gb / bpf, b = gb % bpf;
                raws[i].load(gray + f * (uint64_t)H * W + (b / (W / 8)) * 8 * W + (b % (W / 8)) * 8, (size_t)W);
            }
            bool cand[128];
            if (qm == svs::QM_POW2) extract_fast_wave<svs::QM_POW2>(rows, raws, count, (uint32_t)n, qp, his, los, cand, n_redone);
            else extract_fast_wave<svs::QM_F32>(rows, raws, count, (uint32_t)n, qp, his, los, cand, n_redone);
            if (g_candidate_map)
                for (uint64_t i = 0; i < count; ++i) g_candidate_map[g0 + i] = cand[i];
            for (uint64_t i = 0; i < count; ++i)
                for (int k = 0; k < n; ++k) out_flags[(g0 + i) * n + k] = (uint8_t)svs::window_bit(his[i], los[i], k);
        }
        return total * n;
    }
    for (uint64_t gb = 0; gb < total; ++gb) {
        const uint64_t f = gb / bpf, b = gb % bpf;
        const uint64_t by = b / (W / 8), bx = b % (W / 8);
        const uint8_t *p = gray + f * (uint64_t)H * W + by * 8 * W + bx * 8;
        Blk raw;
        raw.load(p, (size_t)W);
        uint32_t hi, lo;
        if (plan.path == svs::ExtractPath::EXACT) {
            if (qm == svs::QM_POW2) svs::extract_block_exact<8, svs::QM_POW2>(raw.x, raw.y, (uint32_t)n, qp, hi, lo);
            else svs::extract_block_exact<8, svs::QM_F32>(raw.x, raw.y, (uint32_t)n, qp, hi, lo);
        } else if (qm == svs::QM_POW2) extract_fast<svs::QM_POW2>(rows, raw, (uint32_t)n, qp, hi, lo, n_redone);
        else extract_fast<svs::QM_F32>(rows, raw, (uint32_t)n, qp, hi, lo, n_redone);
        for (int i = 0; i < n; ++i) out_flags[gb * n + i] = (uint8_t)svs::window_bit(hi, lo, i);
    }
    return total * n;
}

// forward coefficients of one block (for the DCT accuracy test): D[8][8]
void emu_forward_block(const uint8_t *block64, float *D64) {
    Blk raw;
    raw.load(block64, 8);
    float D[8][8];
    svs::forward_rows<8>(raw.x, raw.y, D);
    std::memcpy(D64, D, sizeof D);
}

// number of (c, delta) pairs on which the reciprocal-multiply quantiser differs from the IEEE division
uint64_t emu_quant_mismatches(const float *c, uint64_t n, double delta) {
    svs::QimParams qp;
    make_qim(delta, &qp);
    uint64_t bad = 0;
    for (uint64_t i = 0; i < n; ++i)
        bad += svs::quant_index<svs::QM_F32>(c[i], qp) != svs::quant_index_by_division(c[i], qp.delta_f);
    return bad;
}

// pocketfft-identical 8-point transforms (type 2 / type 3, norm='ortho')
void emu_pf_dct2(const float *x, float *X) {
    float a[8], b[8];
    std::memcpy(a, x, sizeof a);
    svs::pf::dct2_8(a, b);
    std::memcpy(X, b, sizeof b);
}

void emu_pf_dct3(const float *X, float *x) {
    float a[8], b[8];
    std::memcpy(a, X, sizeof a);
    svs::pf::dct3_8(a, b);
    std::memcpy(x, b, sizeof b);
}

// rows 0 and 1 of the vertical pass as the two-row guarded kernel computes them (packed integer first stages) -> V[2][8]
void emu_vertical_pf01(const uint8_t *block64, float *V16) {
    Blk raw;
    raw.load(block64, 8);
    float a0[4], a1[4], b0[4], b1[4];
    uint32_t S = 0;
    svs::vertical_pf01_packed(raw.x, a0, a1, S);
    svs::vertical_pf01_packed(raw.y, b0, b1, S);
    for (int x = 0; x < 4; ++x) { V16[x] = a0[x]; V16[4 + x] = b0[x]; V16[8 + x] = a1[x]; V16[12 + x] = b1[x]; }
    V16[16] = (float)S;
}

// number of (c, bit) pairs on which the float-domain quantiser step (qim_change) differs from the integer form
uint64_t emu_qim_change_mismatches(const float *c, const uint8_t *bit, uint64_t n, double delta) {
    svs::QimParams qp;
    const int qm = make_qim(delta, &qp);
    uint64_t bad = 0;
    for (uint64_t i = 0; i < n; ++i) {
        float got, want;
        if (qm == svs::QM_POW2) {
            got = svs::qim_change<svs::QM_POW2>(c[i], bit[i], qp);
            want = (float)svs::force_parity(svs::quant_index<svs::QM_POW2>(c[i], qp), bit[i]) * qp.delta_f - c[i];
        } else if (qm == svs::QM_DOUBLE) {
            got = svs::qim_change<svs::QM_DOUBLE>(c[i], bit[i], qp);
            want = (float)((double)svs::force_parity(svs::quant_index_by_division(c[i], qp.delta_f), bit[i]) * qp.delta_d) - c[i];
        } else {
            got = svs::qim_change<svs::QM_F32>(c[i], bit[i], qp);
            want = (float)svs::force_parity(svs::quant_index_by_division(c[i], qp.delta_f), bit[i]) * qp.delta_f - c[i];
        }
        bad += std::memcmp(&got, &want, 4) != 0;
    }
    return bad;
}

// the chunk plan of the host-pointer entry points (csrc/svs_stage.hpp): -> number of chunks; out[4 k ..] = f0, nf, r0, rows
// of chunk k (at most max_chunks are written); target_bytes = 0 takes the built-in rule for a batch of total_bytes
uint64_t emu_plan_chunks(int32_t n_frames, int32_t H, uint64_t row_bytes, uint64_t total_bytes, uint64_t target_bytes, int32_t *out,
                         uint64_t max_chunks) {
    uint64_t k = 0;
    svs::for_each_chunk(n_frames, H, (size_t)row_bytes, (size_t)(target_bytes ? target_bytes : svs::stage_chunk_rule(total_bytes)),
                        [&](const svs::Chunk &c) {
                            if (k < max_chunks) { out[4 * k] = c.f0; out[4 * k + 1] = c.nf; out[4 * k + 2] = c.r0; out[4 * k + 3] = c.rows; }
                            ++k;
                        });
    return k;
}

// the routing of the C ABI (csrc/svs_route.hpp) for tests/test_route_cpu.py.  embed: out = {path, rows, qm, xcd_chunk, n_ac,
// two_blocks, use, bit_offset, n_bits, n_words}; extract: out = {path, rows, qm, xcd_chunk}.  n_ac is clamped as the library does.
void emu_plan_embed(double delta, int n_ac, uint64_t total, uint64_t n_bits, uint64_t bit_offset, int pocketfft, int guarded, int bgr,
                    int guarded_off, int64_t *out) {
    const uint32_t n = n_ac < 0 ? 0 : (n_ac > 63 ? 63 : n_ac);
    const svs::EmbedPlan p = svs::plan_embed(svs::RouteArgs{delta, n, total, n_bits, bit_offset, pocketfft != 0, guarded != 0, bgr != 0,
                                                            guarded_off != 0, 1.0f, 1.0f});
    const int64_t v[10] = {(int64_t)p.path, p.rows, p.qm, p.xcd_chunk, p.n_ac, p.two_blocks, (int64_t)p.use, (int64_t)p.bit_offset,
                           (int64_t)p.n_bits, (int64_t)p.n_words};
    std::memcpy(out, v, sizeof v);
}

void emu_plan_extract(double delta, int n_ac, uint64_t total, int pocketfft, int guarded, int bgr, int guarded_off, int64_t *out) {
    const uint32_t n = n_ac < 0 ? 0 : (n_ac > 63 ? 63 : n_ac);
    const svs::ExtractPlan p = svs::plan_extract(svs::RouteArgs{delta, n, total, 0, 0, pocketfft != 0, guarded != 0, bgr != 0,
                                                                guarded_off != 0, 1.0f, 1.0f});
    const int64_t v[4] = {(int64_t)p.path, p.rows, p.qm, p.xcd_chunk};
    std::memcpy(out, v, sizeof v);
}

uint64_t emu_chunk_budget(uint64_t pass_bits, uint64_t use, uint64_t g0, uint32_t n) { return svs::chunk_budget(pass_bits, use, g0, n); }

// ---- the index arithmetic of the kernels (csrc/svs_index.hpp) and the payload readers, for tests/test_index_arithmetic_cpu.py ----

// make_div(d) -> out = {mul, shift, div}
void emu_make_div(uint32_t d, uint32_t *out) {
    const svs::FastDiv f = svs::make_div(d);
    out[0] = f.mul; out[1] = f.shift; out[2] = f.div;
}

// fast_div(n[i], make_div(d)) for i < count
void emu_fast_div(const uint32_t *n, uint64_t count, uint32_t d, uint32_t *out) {
    const svs::FastDiv f = svs::make_div(d);
    for (uint64_t i = 0; i < count; ++i) out[i] = svs::fast_div(n[i], f);
}

// tile_of(i, grid, chunk) for every i < grid
void emu_tile_of(uint32_t grid, uint32_t chunk, uint32_t *out) {
    for (uint32_t i = 0; i < grid; ++i) out[i] = svs::tile_of(i, grid, chunk);
}

uint32_t emu_tile_of_one(uint32_t i, uint32_t grid, uint32_t chunk) { return svs::tile_of(i, grid, chunk); }

// block_offset (bgr == 0) / block_offset_bgr of blocks gblock[i], geometry filled as the library's make_geometry fills it
void emu_block_offset(const uint32_t *gblock, uint64_t count, uint32_t wb, uint32_t bpf, int64_t row_pitch, int64_t frame_pitch,
                      int bgr, int64_t *out) {
    svs::Geometry g{};
    g.by_wb = svs::make_div(wb);
    g.by_bpf = svs::make_div(bpf);
    g.row_pitch = row_pitch;
    g.frame_pitch = frame_pitch;
    for (uint64_t i = 0; i < count; ++i)
        out[i] = bgr ? svs::block_offset_bgr(gblock[i], g, row_pitch, frame_pitch) : svs::block_offset(gblock[i], g);
}

// stream_first of blocks gblock[i]: raster (keyed == 0) or under the keyed order of (key, first_frame); second, when not
// NULL, receives the right neighbour's (keyed only)
void emu_stream_first(const uint32_t *gblock, uint64_t count, uint32_t n, uint32_t bpf, int keyed, uint64_t key, uint32_t first_frame,
                      uint64_t *first, uint64_t *second) {
    const svs::FastDiv by_bpf = svs::make_div(bpf);
    const svs::BlockOrderArgs o = svs::make_block_order(key, first_frame, bpf);
    for (uint64_t i = 0; i < count; ++i) {
        if (!keyed) first[i] = svs::stream_first_raster(gblock[i], n);
        else first[i] = svs::stream_first_keyed(gblock[i], n, by_bpf, o, second ? &second[i] : nullptr);
    }
}

// payload_window / payload_qword at stream bit s of a buffer of n_words dwords of which only dwords [word_base, word_base +
// the caller's array) exist: `window` holds those, and the readers see it through a pointer biased by word_base
void emu_payload_window(const uint32_t *window, uint64_t word_base, uint32_t n_words, uint64_t s, uint32_t *hi_lo) {
    const uint32_t *bits = reinterpret_cast<const uint32_t *>(reinterpret_cast<uintptr_t>(window) - 4u * (uintptr_t)word_base);
    svs::payload_window(bits, n_words, s, hi_lo[0], hi_lo[1]);
}

uint64_t emu_payload_qword(const uint32_t *window, uint64_t word_base, uint32_t n_words, uint64_t s) {
    const uint32_t *bits = reinterpret_cast<const uint32_t *>(reinterpret_cast<uintptr_t>(window) - 4u * (uintptr_t)word_base);
    return svs::payload_qword(bits, n_words, s);
}

uint32_t emu_window32(uint64_t q, uint32_t sh) { return svs::window32(q, sh); }

void emu_idct8(const float *X, float *x) {
    float a[8], b[8];
    std::memcpy(a, X, sizeof a);
    svs::idct8<8, false>(a, b);
    std::memcpy(x, b, sizeof b);
}

}  // extern "C"
