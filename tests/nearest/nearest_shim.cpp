// CPU build of the embed bodies of csrc/svs_block.hpp for tests/test_nearest_cpu.py: a gray embed call block by block on the
// host with the library's own routing (svs_route.hpp) and SVS_NEAREST set or clear.  Build: g++ -O2 -ffp-contract=off
// -std=c++17 -shared -fPIC.  The lane / wave mapping of the kernels is not modelled (tests/test_nearest_gpu.py covers it).
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
void exact(Blk &b, uint32_t n, uint32_t nb, uint32_t hi, uint32_t lo, const svs::QimRule &qp) {
    svs::embed_block_exact<8, QM>(b.x, b.y, n, nb, hi, lo, qp);
}

// the streaming body the kernels launch (csrc/svs_capi.hip launch_embed): one row - embed_block_guarded; two rows - the
// compile-time-n form for n = 10 and the in-place form for every quantiser but the power-of-two one.  -> undecided
template <int QM>
bool guarded(Blk &b, uint32_t n, uint32_t nb, uint32_t hi, uint32_t lo, const svs::QimRule &qp) {
    if (svs::rows_for((int)n) == 1) return svs::embed_block_guarded<QM>(b.x, b.y, n, nb, hi, lo, qp);
    constexpr bool INPLACE = QM != svs::QM_POW2;
    if (n == 10) return svs::embed_block_guarded2<QM, 10, INPLACE>(b.x, b.y, n, nb, hi, lo, qp);
    return svs::embed_block_guarded2<QM, 0, INPLACE>(b.x, b.y, n, nb, hi, lo, qp);
}

template <int QM>
bool one_block(bool streaming, Blk &b, const uint8_t *p, size_t pitch, uint32_t n, uint32_t nb, uint32_t hi, uint32_t lo,
               const svs::QimRule &qp) {
    if (streaming && !guarded<QM>(b, n, nb, hi, lo, qp)) return false;
    if (streaming) b.load(p, pitch);   // undecided: the in-place form leaves the rows half-written
    exact<QM>(b, n, nb, hi, lo, qp);
    return streaming;
}

}  // namespace

extern "C" {

// gray / stego: contiguous [F][H][W]; bits: packed MSB-first, padded to a multiple of 4 bytes.  pocketfft: SVS_EXACT_POCKETFFT
// (every block through embed_block_exact); otherwise the route of flags = SVS_EXACT_GUARDED.  out[0] = blocks the guard handed
// to the exact replay, out[1] = the plan's path (svs::EmbedPath), out[2] = the plan's `nearest`.  Returns the bits embedded.
uint64_t nr_embed(const uint8_t *gray, uint8_t *stego, int F, int H, int W, double delta, int n_ac, const uint8_t *bits,
                  uint64_t bits_bytes, uint64_t bit_offset, uint64_t n_bits, int pocketfft, int nearest, uint64_t *out) {
    const uint32_t n = (uint32_t)(n_ac < 0 ? 0 : (n_ac > 63 ? 63 : n_ac));
    const uint64_t wb = (uint64_t)W / 8, bpf = wb * (uint64_t)(H / 8), total = bpf * (uint64_t)F;
    std::memcpy(stego, gray, (size_t)F * H * W);
    svs::RouteArgs ra{delta, n, total, n_bits, bit_offset, pocketfft != 0, pocketfft == 0, false, false, 1.0f, 1.0f};
    ra.nearest = nearest != 0;
    const svs::EmbedPlan p = svs::plan_embed(ra);
    out[0] = 0;
    out[1] = (uint64_t)p.path;
    out[2] = p.nearest;
    if (p.path == svs::EmbedPath::COPY) return 0;
    const bool streaming = p.path == svs::EmbedPath::STREAMING;
    const svs::QimRule rule(p.qp, p.nearest ? 1u : 0u);   // what the kernels build from Geometry::pad
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
        if (p.qm == svs::QM_DOUBLE) replayed = one_block<svs::QM_DOUBLE>(streaming, raw, px, (size_t)W, p.n_ac, nb, hi, lo, rule);
        else if (p.qm == svs::QM_POW2) replayed = one_block<svs::QM_POW2>(streaming, raw, px, (size_t)W, p.n_ac, nb, hi, lo, rule);
        else replayed = one_block<svs::QM_F32>(streaming, raw, px, (size_t)W, p.n_ac, nb, hi, lo, rule);
        out[0] += replayed;
        raw.store(px, (size_t)W);
    }
    return p.use;
}

// the plan of a gray (bgr = 0) or fused colour embed call with the flag: out = {path, nearest, use}
void nr_plan(double delta, int n_ac, uint64_t total, uint64_t n_bits, int pocketfft, int bgr, int nearest, int64_t *out) {
    const uint32_t n = (uint32_t)(n_ac < 0 ? 0 : (n_ac > 63 ? 63 : n_ac));
    svs::RouteArgs ra{delta, n, total, n_bits, 0, pocketfft != 0, pocketfft == 0, bgr != 0, false, 1.0f, 1.0f};
    ra.nearest = nearest != 0;
    const svs::EmbedPlan p = svs::plan_embed(ra);
    out[0] = (int64_t)p.path;
    out[1] = (int64_t)p.nearest;
    out[2] = (int64_t)p.use;
}

}
