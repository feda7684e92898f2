// CPU build of the selected block bodies of csrc/svs_block.hpp for tests/test_coeff_select_cpu.py: a select embed / extract
// call block by block on the host, planned by the library's own routing (svs_route.hpp) from the table the C ABI builds
// (svs::make_coeff_table).  Build: g++ -O2 -ffp-contract=off -std=c++17 -shared -fPIC.  A plan without the table (a prefix
// selection, or nothing to embed) runs the bodies of the call without a selection, always with the exact arithmetic - the
// streaming bodies give the same bytes and have tests of their own.  The lane / wave mapping of the kernels is not modelled
// (tests/test_coeff_select_gpu.py covers it).
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

template <int QM>
void embed_one(Blk &b, uint32_t n, uint32_t nb, uint32_t hi, uint32_t lo, const svs::QimRule &qp, const svs::CoeffTable *sel) {
    svs::embed_block_exact<8, QM>(b.x, b.y, n, nb, hi, lo, qp, false, sel);   // what embed_exact_kernel<QM, 8> calls
}

svs::RouteArgs route(double delta, uint32_t n, uint64_t total, uint64_t n_bits, uint64_t bit_offset, int flags,
                     const svs::CoeffTable *t) {
    svs::RouteArgs ra{delta, n, total, n_bits, bit_offset, (flags & 1) != 0, (flags & 2) != 0, false, false, 1.0f, 1.0f};
    ra.coeffs = t;
    return ra;
}

}  // namespace

extern "C" {

// gray / stego: contiguous [F][H][W]; index: `count` flat indices; bits: packed MSB-first, padded to a multiple of 4 bytes;
// flags: the mode bits (SVS_EXACT_POCKETFFT = 1, SVS_EXACT_GUARDED = 2).  info = {path, rows, selected, qm} of the plan.
// Returns the bits embedded, -1 for an invalid selection.
int64_t cs_embed(const uint8_t *gray, uint8_t *stego, int F, int H, int W, double delta, const uint8_t *index, int count,
                 const uint8_t *bits, uint64_t bits_bytes, uint64_t bit_offset, uint64_t n_bits, int flags, int nearest,
                 int64_t *info) {
    svs::CoeffTable table;
    if (!svs::make_coeff_table(index, (uint32_t)count, &table)) return -1;
    const uint64_t wb = (uint64_t)W / 8, bpf = wb * (uint64_t)(H / 8), total = bpf * (uint64_t)F;
    std::memcpy(stego, gray, (size_t)F * H * W);
    svs::RouteArgs ra = route(delta, table.count, total, n_bits, bit_offset, flags, &table);
    ra.nearest = nearest != 0;
    const svs::EmbedPlan p = svs::plan_embed(ra);
    info[0] = (int64_t)p.path; info[1] = p.rows; info[2] = p.selected; info[3] = p.qm;
    if (p.path == svs::EmbedPath::COPY) return 0;
    const svs::CoeffTable *sel = p.selected ? &table : nullptr;
    const svs::QimRule rule(p.qp, p.nearest ? 1u : 0u);
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
        if (p.qm == svs::QM_DOUBLE) embed_one<svs::QM_DOUBLE>(raw, p.n_ac, nb, hi, lo, rule, sel);
        else if (p.qm == svs::QM_POW2) embed_one<svs::QM_POW2>(raw, p.n_ac, nb, hi, lo, rule, sel);
        else embed_one<svs::QM_F32>(raw, p.n_ac, nb, hi, lo, rule, sel);
        raw.store(px, (size_t)W);
    }
    return (int64_t)p.use;
}

// out: one byte per bit, count bits per block.  Returns the number of bits, -1 for an invalid selection.
int64_t cs_extract(const uint8_t *gray, int F, int H, int W, double delta, const uint8_t *index, int count, int flags,
                   uint8_t *out, int64_t *info) {
    svs::CoeffTable table;
    if (!svs::make_coeff_table(index, (uint32_t)count, &table)) return -1;
    const uint64_t wb = (uint64_t)W / 8, bpf = wb * (uint64_t)(H / 8), total = bpf * (uint64_t)F;
    const svs::ExtractPlan p = svs::plan_extract(route(delta, table.count, total, 0, 0, flags, &table));
    info[0] = (int64_t)p.path; info[1] = p.rows; info[2] = p.selected; info[3] = p.qm;
    const uint32_t n = table.count;
    std::memset(out, 0, (size_t)(total * n));
    if (p.path == svs::ExtractPath::ZEROS) return (int64_t)(total * n);
    for (uint64_t gb = 0; gb < total; ++gb) {
        const uint64_t f = gb / bpf, b = gb % bpf;
        Blk raw;
        raw.load(gray + f * (uint64_t)H * W + (b / wb) * 8 * (uint64_t)W + (b % wb) * 8, (size_t)W);
        uint32_t hi = 0, lo = 0;
        if (p.selected) {
            if (p.qm == svs::QM_POW2) svs::extract_block_exact_selected<svs::QM_POW2>(raw.x, raw.y, table, p.qp, hi, lo);
            else svs::extract_block_exact_selected<svs::QM_F32>(raw.x, raw.y, table, p.qp, hi, lo);
        } else {
            if (p.qm == svs::QM_POW2) svs::extract_block_exact<8, svs::QM_POW2>(raw.x, raw.y, n, p.qp, hi, lo);
            else svs::extract_block_exact<8, svs::QM_F32>(raw.x, raw.y, n, p.qp, hi, lo);
        }
        for (uint32_t i = 0; i < n; ++i) out[gb * n + i] = (uint8_t)svs::window_bit(hi, lo, (int)i);
    }
    return (int64_t)(total * n);
}

// svs::make_coeff_table: out[k] = slot of flat index k (255: none), out[64] = count.  Returns validity.
int cs_table(const uint8_t *index, int count, int32_t *out) {
    svs::CoeffTable t;
    const bool ok = svs::make_coeff_table(index, (uint32_t)count, &t);
    for (int k = 0; k < 64; ++k) out[k] = (int32_t)t.slot(k);
    out[64] = (int32_t)t.count;
    return ok ? 1 : 0;
}

}
