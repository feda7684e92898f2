// CPU build of the embed bodies of csrc/svs_block.hpp for tests/test_minmove_cpu.py: a gray embed call block by block on the
// host with the library's own routing (svs_route.hpp) and rule word (rule_word / rule_from_word, what the launchers put into
// Geometry::pad and the kernels read back), with SVS_MINMOVE and SVS_NEAREST set or clear, the row-major prefix or a
// coefficient selection.  Build: g++ -O2 -ffp-contract=off -std=c++17 -shared -fPIC.  The lane / wave mapping of the kernels
// is not modelled (tests/test_minmove_gpu.py covers it).
#include <cstdint>
#include <cstring>

#include "svs_block.hpp"
#include "svs_route.hpp"

namespace {

struct Blk {
    uint32_t x[8], y[8];
    void load(const uint8_t *p, size_t pitch) {
        for (int r = 0; r < 8; ++r) { std::memcpy(&x[r], p + r * pitch, 4); std::memcpy(&y[r], p + r * pitch + 4, 4); }
    }
    void store(uint8_t *p, size_t pitch) const {
        for (int r = 0; r < 8; ++r) { std::memcpy(p + r * pitch, &x[r], 4); std::memcpy(p + r * pitch + 4, &y[r], 4); }
    }
};

// the streaming body the kernels launch (csrc/svs_capi.hip launch_embed): one row - embed_block_guarded; two rows - the
// compile-time-n form for n = 10 and the in-place form for every quantiser but the power-of-two one.  -> undecided
template <int QM>
bool guarded(Blk &b, uint32_t n, uint32_t nb, uint32_t hi, uint32_t lo, const svs::QimRule &qp) {
    if (svs::rows_for((int)n) == 1) return svs::embed_block_guarded<QM>(b.x, b.y, n, nb, hi, lo, qp);
    constexpr bool INPLACE = QM != svs::QM_POW2;
    if (n == 10) return svs::embed_block_guarded2<QM, 10, INPLACE>(b.x, b.y, n, nb, hi, lo, qp);
    return svs::embed_block_guarded2<QM, 0, INPLACE>(b.x, b.y, n, nb, hi, lo, qp);
}

// U: the coefficient rows of the exact instantiation the plan names (1, 2 or 8)
template <int QM>
void exact(Blk &b, int rows, uint32_t n, uint32_t nb, uint32_t hi, uint32_t lo, const svs::QimRule &qp, const svs::CoeffTable *sel) {
    if (rows == 1) svs::embed_block_exact<1, QM>(b.x, b.y, n, nb, hi, lo, qp);
    else if (rows == 2) svs::embed_block_exact<2, QM>(b.x, b.y, n, nb, hi, lo, qp);
    else svs::embed_block_exact<8, QM>(b.x, b.y, n, nb, hi, lo, qp, false, sel);
}

template <int QM>
bool one_block(bool streaming, int rows, Blk &b, const uint8_t *p, size_t pitch, uint32_t n, uint32_t nb, uint32_t hi, uint32_t lo,
               const svs::QimRule &qp, const svs::CoeffTable *sel) {
    if (streaming && !guarded<QM>(b, n, nb, hi, lo, qp)) return false;
    if (streaming) b.load(p, pitch);   // undecided: the in-place form leaves the rows half-written
    exact<QM>(b, streaming ? 8 : rows, n, nb, hi, lo, qp, sel);
    return streaming;
}

}  // namespace

extern "C" {

// gray / stego: contiguous [F][H][W]; bits: packed MSB-first, padded to a multiple of 4 bytes; index / count: a coefficient
// selection, count = 0 for the prefix 1..n_ac.  pocketfft: SVS_EXACT_POCKETFFT (every block through embed_block_exact);
// otherwise the route of flags = SVS_EXACT_GUARDED.  force_qm: -1 = the plan's quantiser mode, else that svs::QuantMode (the
// caller asks only for modes that are valid for the delta).  out = {blocks the guard handed to the exact replay, the plan's
// path, its `minmove`, its `nearest`, its qm, the rule word}.  Returns the bits embedded, ~0 for an invalid selection.
// guard_scale: RouteArgs::guard_scale, what SVS_GUARD_SCALE is to the experiments library (1 = the product's BETA).
// replay_map: NULL, or one byte per block of the call (raster order over the batch), set to 1 where the guard handed the
// block to the exact replay (the caller zeroes it).
uint64_t mm_embed_scaled(const uint8_t *gray, uint8_t *stego, int F, int H, int W, double delta, int n_ac, const uint8_t *index,
                         int count, const uint8_t *bits, uint64_t bits_bytes, uint64_t bit_offset, uint64_t n_bits, int pocketfft,
                         int nearest, int minmove, int force_qm, uint64_t *out, float guard_scale, uint8_t *replay_map) {
    svs::CoeffTable table{};
    if (count && !svs::make_coeff_table(index, (uint32_t)count, &table)) return ~0ull;
    const uint32_t n = count ? table.count : (uint32_t)(n_ac < 0 ? 0 : (n_ac > 63 ? 63 : n_ac));
    const uint64_t wb = (uint64_t)W / 8, bpf = wb * (uint64_t)(H / 8), total = bpf * (uint64_t)F;
    std::memcpy(stego, gray, (size_t)F * H * W);
    svs::RouteArgs ra{delta, n, total, n_bits, bit_offset, pocketfft != 0, pocketfft == 0, false, false, guard_scale, 1.0f};
    ra.nearest = nearest != 0;
    ra.minmove = minmove != 0;
    if (count) ra.coeffs = &table;
    const svs::EmbedPlan p = svs::plan_embed(ra);
    const uint32_t word = svs::rule_word(p.nearest, p.minmove, p.half_cell);
    out[0] = 0;
    out[1] = (uint64_t)p.path;
    out[2] = p.minmove;
    out[3] = p.nearest;
    out[4] = (uint64_t)p.qm;
    out[5] = word;
    if (p.path == svs::EmbedPath::COPY) return 0;
    const bool streaming = p.path == svs::EmbedPath::STREAMING;
    const svs::QimRule rule = svs::rule_from_word(p.qp, word);   // what the kernels build from Geometry::pad
    const svs::CoeffTable *sel = p.selected ? &table : nullptr;
    const int qm = force_qm < 0 ? p.qm : force_qm;
    const uint32_t n_words = (uint32_t)(bits_bytes / 4);
    for (uint64_t gb = 0; gb < total; ++gb) {
        const uint64_t first = gb * p.n_ac;
        const uint32_t nb = p.use ? svs::block_budget(first, p.n_bits, p.n_ac) : 1u;   // ROUND_TRIP: every block is entered
        if (nb == 0) break;
        const uint64_t f = gb / bpf, b = gb % bpf;
        uint8_t *px = stego + f * (uint64_t)H * W + (b / wb) * 8 * (uint64_t)W + (b % wb) * 8;
        Blk raw;
        raw.load(px, (size_t)W);
        uint32_t hi = 0, lo = 0;
        if (p.use) svs::payload_window(reinterpret_cast<const uint32_t *>(bits), n_words, p.bit_offset + first, hi, lo);
        bool replayed;
        if (qm == svs::QM_DOUBLE) replayed = one_block<svs::QM_DOUBLE>(streaming, p.rows, raw, px, (size_t)W, p.n_ac, nb, hi, lo, rule, sel);
        else if (qm == svs::QM_POW2) replayed = one_block<svs::QM_POW2>(streaming, p.rows, raw, px, (size_t)W, p.n_ac, nb, hi, lo, rule, sel);
        else replayed = one_block<svs::QM_F32>(streaming, p.rows, raw, px, (size_t)W, p.n_ac, nb, hi, lo, rule, sel);
        out[0] += replayed;
        if (replay_map && replayed) replay_map[gb] = 1;
        raw.store(px, (size_t)W);
    }
    return p.use;
}

// the product's guard, no map: every caller from before the guard-scale argument
uint64_t mm_embed(const uint8_t *gray, uint8_t *stego, int F, int H, int W, double delta, int n_ac, const uint8_t *index,
                  int count, const uint8_t *bits, uint64_t bits_bytes, uint64_t bit_offset, uint64_t n_bits, int pocketfft,
                  int nearest, int minmove, int force_qm, uint64_t *out) {
    return mm_embed_scaled(gray, stego, F, H, W, delta, n_ac, index, count, bits, bits_bytes, bit_offset, n_bits, pocketfft, nearest,
                           minmove, force_qm, out, 1.0f, nullptr);
}

// the plan of a gray (bgr = 0) or fused colour embed call with the flag: out = {path, minmove, use, bits of half_cell, rule word}
void mm_plan(double delta, int n_ac, uint64_t total, uint64_t n_bits, int pocketfft, int bgr, int nearest, int minmove, int64_t *out) {
    const uint32_t n = (uint32_t)(n_ac < 0 ? 0 : (n_ac > 63 ? 63 : n_ac));
    svs::RouteArgs ra{delta, n, total, n_bits, 0, pocketfft != 0, pocketfft == 0, bgr != 0, false, 1.0f, 1.0f};
    ra.nearest = nearest != 0;
    ra.minmove = minmove != 0;
    const svs::EmbedPlan p = svs::plan_embed(ra);
    uint32_t hbits;
    std::memcpy(&hbits, &p.half_cell, 4);
    out[0] = (int64_t)p.path;
    out[1] = (int64_t)p.minmove;
    out[2] = (int64_t)p.use;
    out[3] = (int64_t)hbits;
    out[4] = (int64_t)svs::rule_word(p.nearest, p.minmove, p.half_cell);
}

// MARGIN[k] as the bodies read it
float mm_margin(int k) { return svs::minmove_margin((uint32_t)k); }

// one coefficient through the integer form (qim_target) and the float-domain form (qim_change) of the rule, quantiser mode qm:
// out = {the value qim_target writes, the change qim_change returns}
void mm_coefficient(float c, int bit, double delta, int k, int qm, float *out) {
    svs::QimParams qp;
    svs::make_qim(delta, &qp);
    const svs::QimRule rule(qp, (uint32_t)svs::RULE_MINMOVE, (float)(0.5 * delta));
    const float r = svs::qim_band<svs::RULE_MINMOVE>(rule, (uint32_t)k);
    if (qm == svs::QM_DOUBLE) {
        out[0] = svs::qim_target<svs::QM_DOUBLE, svs::RULE_MINMOVE>(c, bit, rule, r);
        out[1] = svs::qim_change<svs::QM_DOUBLE, svs::RULE_MINMOVE>(c, (uint32_t)bit, rule, r);
    } else if (qm == svs::QM_POW2) {
        out[0] = svs::qim_target<svs::QM_POW2, svs::RULE_MINMOVE>(c, bit, rule, r);
        out[1] = svs::qim_change<svs::QM_POW2, svs::RULE_MINMOVE>(c, (uint32_t)bit, rule, r);
    } else {
        out[0] = svs::qim_target<svs::QM_F32, svs::RULE_MINMOVE>(c, bit, rule, r);
        out[1] = svs::qim_change<svs::QM_F32, svs::RULE_MINMOVE>(c, (uint32_t)bit, rule, r);
    }
}

}
