// CPU build of the dithered block bodies of csrc/svs_block.hpp for tests/test_dither_cpu.py: a dithered gray embed / extract
// call block by block on the host, planned by the library's own routing (svs_route.hpp) with the rule word the launchers put
// into Geometry::pad, the row-major prefix 1..n_ac or a coefficient selection, raster order.  Build: g++ -O2 -ffp-contract=off
// -std=c++17 -shared -fPIC.  The lane / wave mapping of the kernels and the keyed order are not modelled
// (tests/test_dither_gpu.py covers them).
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

// what embed_exact_kernel<QM, 8, .., DitherArgs> calls (dithered) and what the U = 8 kernel without a dither calls
template <int QM>
void embed_one(Blk &b, bool dithered, uint32_t n, uint32_t nb, uint32_t hi, uint32_t lo, const svs::QimRule &qp,
               const svs::CoeffTable *sel, uint32_t s_b) {
    if (dithered) svs::embed_block_exact<8, QM, true>(b.x, b.y, n, nb, hi, lo, qp, false, sel, s_b);
    else svs::embed_block_exact<8, QM>(b.x, b.y, n, nb, hi, lo, qp, false, sel);
}

// what extract_exact_kernel<8, QM, ..> calls on its dithered side: the selected form with a selection, else the prefix form
template <int QM>
void extract_one(const Blk &b, uint32_t n, const svs::QimParams &qp, const svs::CoeffTable *sel, uint32_t s_b, uint32_t &hi,
                 uint32_t &lo) {
    if (sel) svs::extract_block_exact_selected<QM, true>(b.x, b.y, *sel, qp, hi, lo, s_b);
    else svs::extract_block_exact<8, QM, true>(b.x, b.y, n, qp, hi, lo, s_b);
}

uint32_t clamp_n(int n_ac) { return (uint32_t)(n_ac < 0 ? 0 : (n_ac > 63 ? 63 : n_ac)); }

}  // namespace

extern "C" {

// h of (key, t, i, k) and the three seeds on the way: out = {seed, s_t-free s_b, h}; returns d for `delta`
float dt_hash(uint64_t key, uint32_t t, uint32_t i, uint32_t k, float delta_f, uint32_t *out) {
    const uint32_t seed = svs::dither_seed(key);
    const uint32_t s_b = svs::dither_block_seed(seed, t, i);
    out[0] = seed;
    out[1] = s_b;
    out[2] = svs::lowbias32(s_b ^ (k * 0x632BE5ABu));
    return svs::dither_value(s_b, k, delta_f);
}

// gray / stego: contiguous [F][H][W]; bits: packed MSB-first, padded to a multiple of 4 bytes; index / count: a coefficient
// selection (count 0: none; n_ac is then ignored, as in the C ABI); flags: the mode bits (1, 2).  info = {path, rows, selected, qm, dithered} of the
// plan.  Returns the bits embedded, ~0 for an invalid selection.
uint64_t dt_embed(const uint8_t *gray, uint8_t *stego, int F, int H, int W, double delta, int n_ac, const uint8_t *index, int count,
                  uint64_t key, uint32_t first_frame, const uint8_t *bits, uint64_t bits_bytes, uint64_t bit_offset,
                  uint64_t n_bits, int flags, int nearest, int minmove, int64_t *info) {
    svs::CoeffTable table{};
    if (count && !svs::make_coeff_table(index, (uint32_t)count, &table)) return ~0ull;
    const uint32_t n = count ? (uint32_t)count : clamp_n(n_ac);
    const uint64_t wb = (uint64_t)W / 8, bpf = wb * (uint64_t)(H / 8), total = bpf * (uint64_t)F;
    std::memcpy(stego, gray, (size_t)F * H * W);
    svs::RouteArgs ra{delta, n, total, n_bits, bit_offset, (flags & 1) != 0, (flags & 2) != 0, false, false, 1.0f, 1.0f};
    ra.nearest = nearest != 0;
    ra.minmove = minmove != 0;
    ra.dithered = true;
    if (count && !svs::coeff_table_is_prefix(table)) ra.coeffs = &table;
    const svs::EmbedPlan p = svs::plan_embed(ra);
    info[0] = (int64_t)p.path; info[1] = p.rows; info[2] = p.selected; info[3] = p.qm; info[4] = p.dithered;
    if (p.path == svs::EmbedPath::COPY) return 0;
    const svs::QimRule rule = svs::rule_from_word(p.qp, svs::rule_word(p.nearest, p.minmove, p.half_cell));
    // the dithered side runs the selected loop alone: the selection, or the prefix table of n_ac (launch_embed, svs_capi.hip)
    const svs::CoeffTable prefix = svs::make_prefix_table(p.n_ac);
    const svs::CoeffTable *sel = p.selected ? &table : p.dithered ? &prefix : nullptr;
    const uint32_t seed = svs::dither_seed(key);
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
        const uint32_t s_b = svs::dither_block_seed(seed, first_frame + (uint32_t)f, (uint32_t)b);
        if (p.qm == svs::QM_DOUBLE) embed_one<svs::QM_DOUBLE>(raw, p.dithered, p.n_ac, nb, hi, lo, rule, sel, s_b);
        else if (p.qm == svs::QM_POW2) embed_one<svs::QM_POW2>(raw, p.dithered, p.n_ac, nb, hi, lo, rule, sel, s_b);
        else embed_one<svs::QM_F32>(raw, p.dithered, p.n_ac, nb, hi, lo, rule, sel, s_b);
        raw.store(px, (size_t)W);
    }
    return p.use;
}

// out: one byte per bit, n bits per block.  info = {path, rows, selected, qm, dithered}.  Returns the number of bits.
int64_t dt_extract(const uint8_t *gray, int F, int H, int W, double delta, int n_ac, const uint8_t *index, int count, uint64_t key,
                   uint32_t first_frame, int flags, uint8_t *out, int64_t *info) {
    svs::CoeffTable table{};
    if (count && !svs::make_coeff_table(index, (uint32_t)count, &table)) return -1;
    const uint32_t n = count ? (uint32_t)count : clamp_n(n_ac);
    const uint64_t wb = (uint64_t)W / 8, bpf = wb * (uint64_t)(H / 8), total = bpf * (uint64_t)F;
    svs::RouteArgs ra{delta, n, total, 0, 0, (flags & 1) != 0, (flags & 2) != 0, false, false, 1.0f, 1.0f};
    ra.dithered = true;
    if (count && !svs::coeff_table_is_prefix(table)) ra.coeffs = &table;
    const svs::ExtractPlan p = svs::plan_extract(ra);
    info[0] = (int64_t)p.path; info[1] = p.rows; info[2] = p.selected; info[3] = p.qm; info[4] = p.dithered;
    std::memset(out, 0, (size_t)(total * n));
    if (p.path == svs::ExtractPath::ZEROS) return (int64_t)(total * n);
    const uint32_t seed = svs::dither_seed(key);
    const svs::CoeffTable *sel = p.selected ? &table : nullptr;
    for (uint64_t gb = 0; gb < total; ++gb) {
        const uint64_t f = gb / bpf, b = gb % bpf;
        Blk raw;
        raw.load(gray + f * (uint64_t)H * W + (b / wb) * 8 * (uint64_t)W + (b % wb) * 8, (size_t)W);
        const uint32_t s_b = svs::dither_block_seed(seed, first_frame + (uint32_t)f, (uint32_t)b);
        uint32_t hi = 0, lo = 0;
        if (p.qm == svs::QM_POW2) extract_one<svs::QM_POW2>(raw, n, p.qp, sel, s_b, hi, lo);
        else extract_one<svs::QM_F32>(raw, n, p.qp, sel, s_b, hi, lo);
        for (uint32_t i = 0; i < n; ++i) out[gb * n + i] = (uint8_t)svs::window_bit(hi, lo, (int)i);
    }
    return (int64_t)(total * n);
}

}
