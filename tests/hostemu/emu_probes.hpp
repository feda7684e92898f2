// emu_probes.hpp - TEST INFRASTRUCTURE ONLY: the single-purpose entry points of the host library (included by hostemu.cpp, its
// only translation unit): one function of a csrc/ header each, for the CPU test that names it.
#pragma once

namespace {

// violations[0..3]: gray(out) != t, out != c + d although nothing clips, d == 0 but out != c, a channel moved against d
void check_one(uint32_t c, uint32_t t, const uint32_t *w, uint64_t *v) {
    const uint32_t c0 = c & 0xffu, c1 = (c >> 8) & 0xffu, c2 = (c >> 16) & 0xffu;
    uint32_t b = c0, g = c1, r = c2;
    svs::keep_colour_pixel(b, g, r, t, w[0], w[1], w[2], w[3]);
    const int d = (int)t - (int)svs::colour_gray(c0, c1, c2, w[0], w[1], w[2], w[3]);
    v[0] += svs::colour_gray(b, g, r, w[0], w[1], w[2], w[3]) != t;
    const int lo = (int)(c0 < c1 ? (c0 < c2 ? c0 : c2) : (c1 < c2 ? c1 : c2));
    const int hi = (int)(c0 > c1 ? (c0 > c2 ? c0 : c2) : (c1 > c2 ? c1 : c2));
    if (lo + d >= 0 && hi + d <= 255)
        v[1] += (int)b != (int)c0 + d || (int)g != (int)c1 + d || (int)r != (int)c2 + d;
    if (d == 0) v[2] += b != c0 || g != c1 || r != c2;
    const int mv[3] = {(int)b - (int)c0, (int)g - (int)c1, (int)r - (int)c2};
    for (int k = 0; k < 3; ++k) v[3] += (d > 0 && mv[k] < 0) || (d < 0 && mv[k] > 0) || (d == 0 && mv[k] != 0);
}

}  // namespace

extern "C" {

// ---- the transforms and quantisers of csrc/svs_block.hpp ---------------------------------------------------------------------

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

void emu_idct8(const float *X, float *x) {
    float a[8], b[8];
    std::memcpy(a, X, sizeof a);
    svs::idct8<8, false>(a, b);
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
    const int mode = make_qim(delta, &qp);
    uint64_t bad = 0;
    for (uint64_t i = 0; i < n; ++i) {
        bad += with_qm(mode, [&](auto qm) {
            constexpr int QM = decltype(qm)::value;
            const float got = svs::qim_change<QM>(c[i], bit[i], qp);
            float want;
            if constexpr (QM == svs::QM_POW2)
                want = (float)svs::force_parity(svs::quant_index<svs::QM_POW2>(c[i], qp), bit[i]) * qp.delta_f - c[i];
            else if constexpr (QM == svs::QM_DOUBLE)
                want = (float)((double)svs::force_parity(svs::quant_index_by_division(c[i], qp.delta_f), bit[i]) * qp.delta_d) - c[i];
            else
                want = (float)svs::force_parity(svs::quant_index_by_division(c[i], qp.delta_f), bit[i]) * qp.delta_f - c[i];
            return std::memcmp(&got, &want, 4) != 0;
        });
    }
    return bad;
}

// MARGIN[k] of SVS_MINMOVE as the bodies read it
float mm_margin(int k) { return svs::minmove_margin((uint32_t)k); }

// one coefficient through the integer form (qim_target) and the float-domain form (qim_change) of the SVS_MINMOVE rule,
// quantiser mode qm: out = {the value qim_target writes, the change qim_change returns}
void mm_coefficient(float c, int bit, double delta, int k, int qm, float *out) {
    svs::QimParams qp;
    svs::make_qim(delta, &qp);
    const svs::QimRule rule(qp, (uint32_t)svs::RULE_MINMOVE, (float)(0.5 * delta));
    const float r = svs::qim_band<svs::RULE_MINMOVE>(rule, (uint32_t)k);
    with_qm(qm, [&](auto m) {
        constexpr int QM = decltype(m)::value;
        out[0] = svs::qim_target<QM, svs::RULE_MINMOVE>(c, bit, rule, r);
        out[1] = svs::qim_change<QM, svs::RULE_MINMOVE>(c, (uint32_t)bit, rule, r);
    });
}

// svs::make_coeff_table: out[k] = slot of flat index k (255: none), out[64] = count.  Returns validity.
int cs_table(const uint8_t *index, int count, int32_t *out) {
    svs::CoeffTable t;
    const bool ok = svs::make_coeff_table(index, (uint32_t)count, &t);
    for (int k = 0; k < 64; ++k) out[k] = (int32_t)t.slot(k);
    out[64] = (int32_t)t.count;
    return ok ? 1 : 0;
}

// the keyed dither: h of (key, t, i, k) and the seeds on the way: out = {seed, s_b, h}; returns d for `delta`
float dt_hash(uint64_t key, uint32_t t, uint32_t i, uint32_t k, float delta_f, uint32_t *out) {
    const uint32_t seed = svs::dither_seed(key);
    const uint32_t s_b = svs::dither_block_seed(seed, t, i);
    out[0] = seed;
    out[1] = s_b;
    out[2] = svs::lowbias32(s_b ^ (k * 0x632BE5ABu));
    return svs::dither_value(s_b, k, delta_f);
}

// ---- the routing of the C ABI (csrc/svs_route.hpp) and the chunk plan (csrc/svs_stage.hpp) --------------------------------

// for tests/test_route_cpu.py.  embed: out = {path, rows, qm, xcd_chunk, n_ac, two_blocks, use, bit_offset, n_bits, n_words};
// extract: out = {path, rows, qm, xcd_chunk}.  n_ac is clamped as the library does.
void emu_plan_embed(double delta, int n_ac, uint64_t total, uint64_t n_bits, uint64_t bit_offset, int pocketfft, int guarded, int bgr,
                    int guarded_off, int64_t *out) {
    const svs::EmbedPlan p = svs::plan_embed(svs::RouteArgs{delta, clamp_n(n_ac), total, n_bits, bit_offset, pocketfft != 0,
                                                            guarded != 0, bgr != 0, guarded_off != 0, 1.0f, 1.0f});
    const int64_t v[10] = {(int64_t)p.path, p.rows, p.qm, p.xcd_chunk, p.n_ac, p.two_blocks, (int64_t)p.use, (int64_t)p.bit_offset,
                           (int64_t)p.n_bits, (int64_t)p.n_words};
    std::memcpy(out, v, sizeof v);
}

void emu_plan_extract(double delta, int n_ac, uint64_t total, int pocketfft, int guarded, int bgr, int guarded_off, int64_t *out) {
    const svs::ExtractPlan p = svs::plan_extract(svs::RouteArgs{delta, clamp_n(n_ac), total, 0, 0, pocketfft != 0, guarded != 0,
                                                                bgr != 0, guarded_off != 0, 1.0f, 1.0f});
    const int64_t v[4] = {(int64_t)p.path, p.rows, p.qm, p.xcd_chunk};
    std::memcpy(out, v, sizeof v);
}

// the plan of a gray (bgr = 0) or fused colour embed call with SVS_NEAREST / SVS_MINMOVE set or clear (the route of SVS_EXACT_POCKETFFT, else of
// SVS_EXACT_GUARDED): out = {path, nearest, minmove, use, bits of half_cell, rule word}
void emu_plan_rule(double delta, int n_ac, uint64_t total, uint64_t n_bits, int pocketfft, int bgr, int nearest, int minmove,
                   int64_t *out) {
    svs::RouteArgs ra{delta, clamp_n(n_ac), total, n_bits, 0, pocketfft != 0, pocketfft == 0, bgr != 0, false, 1.0f, 1.0f};
    ra.nearest = nearest != 0;
    ra.minmove = minmove != 0;
    const svs::EmbedPlan p = svs::plan_embed(ra);
    uint32_t hbits;
    std::memcpy(&hbits, &p.half_cell, 4);
    const int64_t v[6] = {(int64_t)p.path, p.nearest, p.minmove, (int64_t)p.use, (int64_t)hbits,
                          (int64_t)svs::rule_word(p.nearest, p.minmove, p.half_cell)};
    std::memcpy(out, v, sizeof v);
}

// the chunk plan of the host-pointer entry points: -> number of chunks; out[4 k ..] = f0, nf, r0, rows of chunk k (at most
// max_chunks are written); target_bytes = 0 takes the built-in rule for a batch of total_bytes
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

// ---- the keyed block order (csrc/svs_order.hpp) and the keep-colour rule (csrc/svs_colour.hpp) -----------------------------

// out[x] = sigma_t(x) (inverse = 0: slot -> block) or sigma_t^-1(x) (inverse = 1: block -> slot), x = 0 .. n_blocks - 1;
// first_frame + f = t is split as the kernels split it
void bo_map(uint64_t key, uint32_t first_frame, uint32_t f, uint32_t n_blocks, int inverse, uint32_t *out) {
    const svs::BlockOrderArgs o = svs::make_block_order(key, first_frame, n_blocks);
    const svs::RoundKeys rk = svs::round_keys(o, o.first_frame + f);
    for (uint32_t x = 0; x < n_blocks; ++x) out[x] = inverse ? svs::block_to_slot(x, o, rk) : svs::slot_to_block(x, o, rk);
}

uint32_t bo_lowbias32(uint32_t h) { return svs::lowbias32(h); }

// bgr / out: n pixels of 3 bytes; t: n target grays; w: {wb, wg, wr, shift}
void kc_apply(const uint8_t *bgr, const uint8_t *t, uint8_t *out, uint64_t n, const uint32_t *w) {
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t b = bgr[3 * i], g = bgr[3 * i + 1], r = bgr[3 * i + 2];
        svs::keep_colour_pixel(b, g, r, t[i], w[0], w[1], w[2], w[3]);
        out[3 * i] = (uint8_t)b; out[3 * i + 1] = (uint8_t)g; out[3 * i + 2] = (uint8_t)r;
    }
}

// every colour (c = B | G << 8 | R << 16, first .. first + count - 1) x every t with |t - gray(c)| <= radius
// (radius >= 255: every t); returns the number of (c, t) pairs checked, violations in v[4]
uint64_t kc_check(uint32_t first, uint32_t count, uint32_t stride, int radius, const uint32_t *w, uint64_t *v) {
    uint64_t pairs = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t c = (first + i * stride) & 0xffffffu;
        const int g0 = (int)svs::colour_gray(c & 0xffu, (c >> 8) & 0xffu, (c >> 16) & 0xffu, w[0], w[1], w[2], w[3]);
        const int lo = g0 - radius < 0 ? 0 : g0 - radius, hi = g0 + radius > 255 ? 255 : g0 + radius;
        for (int t = lo; t <= hi; ++t, ++pairs) check_one(c, (uint32_t)t, w, v);
    }
    return pairs;
}

// ---- the soft side's launch arguments and the integer side of its vote and histogram tails (csrc/svs_block.hpp, svs_index.hpp) ----

// the SoftArgs an extract call's launch passes (svs_route.hpp extract_tables, as the launch calls it): -> 0, or -1 when the call
// is refused.  emu_soft_args: fields[7] = {on, vote, hist, period, base, head, sizeof(SoftArgs)}
static int soft_args_of(const EmuCall *c, svs::SoftArgs *sa) {
    Selection s;
    const Grid g(*c);
    svs::ExtractPlan p;
    svs::LaunchTables t;
    if (c->size != sizeof(EmuCall) || !plan_extract_call(*c, s, g.total, g.bpf, p, t)) return -1;
    *sa = t.soft;
    return 0;
}

int emu_soft_args(const EmuCall *c, uint64_t *fields) {
    svs::SoftArgs sa;
    if (soft_args_of(c, &sa)) return -1;
    const uint64_t v[7] = {sa.on, sa.vote, sa.hist, sa.period, sa.base, sa.head, sizeof(svs::SoftArgs)};
    std::memcpy(fields, v, sizeof v);
    return 0;
}

// c: a vote call.  residues[k] = (vote_bit0 + i[k]) mod vote_period as the kernel takes it (vote_residue: a double-precision
// quotient with one correction, no 64-bit division), in_head[k] = whether the bit lies in copy 0
int emu_vote_residues(const EmuCall *c, const uint64_t *i, uint64_t count, uint64_t *residues, uint8_t *in_head) {
    svs::SoftArgs sa;
    if (soft_args_of(c, &sa) || !sa.vote) return -1;
    for (uint64_t k = 0; k < count; ++k) {
        residues[k] = svs::vote_residue(i[k], sa);
        in_head[k] = i[k] < sa.head;
    }
    return 0;
}

int32_t emu_vote_of(uint32_t byte, int in_head) { return svs::vote_of(byte, in_head != 0); }

uint64_t emu_vote_period_max(void) { return svs::kVotePeriodMax; }

uint32_t emu_hist_bins(void) { return svs::kHistBins; }

// The per-frame runs of the wave whose first block is wave_first, in a workgroup whose first block is wg_first, of a call of
// `total` blocks at bpf blocks per frame - the loop of hist_soft_run: for every frame the workgroup touches, the wave's part.
// out: triples {frame, begin, end} (positions within the wave's run), one per frame of the WORKGROUP, empty parts included;
// returns their number (at most `room`).
uint32_t emu_hist_runs(uint32_t wg_first, uint32_t wg_size, uint32_t wave_first, uint32_t total, uint32_t bpf, uint32_t *out,
                       uint32_t room) {
    const svs::FastDiv by_bpf = svs::make_div(bpf);
    const uint32_t wg_blocks = wg_first < total ? (total - wg_first < wg_size ? total - wg_first : wg_size) : 0u;
    if (wg_blocks == 0u) return 0u;
    const uint32_t blocks = wave_first < total ? (total - wave_first < 64u ? total - wave_first : 64u) : 0u;
    const uint32_t f_first = svs::fast_div(wg_first, by_bpf), f_last = svs::fast_div(wg_first + wg_blocks - 1u, by_bpf);
    uint32_t k = 0;
    for (uint32_t f = f_first; f <= f_last && k < room; ++f, ++k) {
        uint32_t begin, end;
        svs::frame_run(wave_first, blocks, f, bpf, &begin, &end);
        out[3 * k] = f;
        out[3 * k + 1] = begin;
        out[3 * k + 2] = end;
    }
    return k;
}

}  // extern "C"
