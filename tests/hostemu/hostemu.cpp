// hostemu.cpp - TEST INFRASTRUCTURE ONLY (never loaded by the product package).
//
// Runs the plain-C++ headers of csrc/ - the exact per-block arithmetic and bit bookkeeping the gfx950 kernels execute
// (svs_block.hpp, svs_readback.hpp), their tile maps, divisions and offsets (svs_index.hpp), the routing of the C ABI
// (svs_route.hpp), the keyed order (svs_order.hpp), the chunk plan (svs_stage.hpp) and the keep-colour rule (svs_colour.hpp) -
// on the CPU, block by block, so that the CPU-only test tier (and ASan/UBSan) can check them against the oracle without a GPU
// and the GPU tests can take their expected values from them.  The lane/wave mapping, HBM access and LDS bit packing of the
// kernels are NOT modelled here; those are covered by the -m gpu tests.
//
// The only translation unit of the host library (emu_call.h: the call and result structs; emu_probes.hpp: the single-purpose
// entry points).  A gray call is described once (EmuCall) and replayed by one of three walkers - embed_call, extract_call,
// readback_call -, the soft calls among the extracts; nothing here keeps state between calls.
// Build: g++ -O2 -ffp-contract=off -std=c++17 -shared -fPIC -I<csrc> hostemu.cpp -o libsvs_hostemu.so
#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>

#include "svs_block.hpp"
#include "svs_colour.hpp"
#include "svs_index.hpp"
#include "svs_order.hpp"
#include "svs_readback.hpp"
#include "svs_route.hpp"
#include "svs_stage.hpp"

#include "emu_call.h"

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

uint32_t clamp_n(int n_ac) { return (uint32_t)(n_ac < 0 ? 0 : (n_ac > 63 ? 63 : n_ac)); }   // as the library clamps it

// f(integral_constant<int, qm>): one instantiation of f per quantiser mode, in the style of dispatch<> in csrc/svs_capi.hip
template <class F>
auto with_qm(int qm, F &&f) {
    if (qm == svs::QM_DOUBLE) return f(std::integral_constant<int, svs::QM_DOUBLE>{});
    if (qm == svs::QM_POW2) return f(std::integral_constant<int, svs::QM_POW2>{});
    return f(std::integral_constant<int, svs::QM_F32>{});
}

// the blocks of a call's frames, contiguous [F][H][W]; gb: raster order over the batch
struct Grid {
    uint64_t H, W, wb, bpf, total;
    explicit Grid(const EmuCall &c) : H((uint64_t)c.H), W((uint64_t)c.W), wb(W / 8), bpf(wb * (H / 8)), total(bpf * (uint64_t)c.F) {}
    template <class T>
    T *block_at(T *frames, uint64_t f, uint64_t by, uint64_t bx) const { return frames + f * H * W + by * 8 * W + bx * 8; }
    template <class T>
    T *block(T *frames, uint64_t gb) const { return block_at(frames, gb / bpf, gb % bpf / wb, gb % bpf % wb); }
};

// the coefficients of a call: its selection's table, or the prefix table of n_ac (what the dithered and read-back launches
// pass without a selection), and the n the call is planned with
struct Selection {
    svs::CoeffTable table;
    uint32_t n;
    bool given;
};

bool make_selection(const EmuCall &c, Selection &s) {   // -> false: a selection the library refuses
    s.given = c.count > 0;
    s.n = s.given ? (uint32_t)c.count : clamp_n(c.n_ac);
    if (s.given) return svs::make_coeff_table(c.index, (uint32_t)c.count, &s.table);
    s.table = svs::make_prefix_table(s.n);
    return true;
}

// the library's routing (csrc/svs_route.hpp) of the call
svs::RouteArgs route(const EmuCall &c, const Selection &s, uint64_t total) {
    svs::RouteArgs ra{c.delta, s.n, total, c.n_bits, c.bit_offset, c.pocketfft != 0, c.guarded != 0, false, false, c.guard_scale,
                      c.tie_scale};
    ra.keyed = c.order != 0;
    ra.nearest = c.nearest != 0;
    ra.minmove = c.minmove != 0;
    ra.dithered = c.dither != 0;
    if (s.given) ra.coeffs = &s.table;
    ra.soft = c.output == EMU_SOFT;
    ra.vote = c.output == EMU_VOTE;
    ra.hist = c.output == EMU_HIST;
    return ra;
}

// the options of the call in the kernels' forms, as the library derives them (csrc/svs_capi.hip GrayOptions::kernel_forms)
svs::KernelOptions kernel_forms(const EmuCall &c, const Selection &s, uint64_t bpf) {
    return {svs::make_block_order(c.order_key, c.first_frame, (uint32_t)bpf), s.given ? &s.table : nullptr,
            svs::DitherArgs{svs::dither_seed(c.dither_key), c.first_frame, 1u, svs::CoeffTable{}}, c.vote_period, c.vote_bit0};
}

// -> false: the walkers refuse the call.  Else the plan of an extract call and what its launch passes (svs_route.hpp)
bool plan_extract_call(const EmuCall &c, Selection &s, uint64_t total, uint64_t bpf, svs::ExtractPlan &p, svs::LaunchTables &t) {
    // the hard keyed extract is not modelled; a vote with no period is refused by the library
    if (!make_selection(c, s) || (c.order && c.output == EMU_BITS) || (c.output == EMU_VOTE && c.vote_period == 0)) return false;
    p = svs::plan_extract(route(c, s, total));
    t = svs::extract_tables(p, kernel_forms(c, s, bpf));
    return true;
}

bool sizes_match(const EmuCall *c, EmuResult *r) {
    if (c->size != sizeof(EmuCall) || r->size != sizeof(EmuResult)) return false;
    *r = EmuResult{sizeof(EmuResult)};
    return true;
}

// ---- embed ---------------------------------------------------------------------------------------------------------------

// The streaming body as the KERNELS launch it (csrc/svs_capi.hip launch_embed): one coefficient row -
// embed_block_guarded; two rows - compile-time n for the GUI's default 10, and for every quantiser but the power-of-two one
// the in-place form (truncated inverse, stego bytes written over the row dwords, an undecided block left half-written: the
// kernel rebuilds it from the rows it parked in LDS, the caller here from the frame).  EMU_GENERIC_GUARDED2 forces
// <QM, 0, false> so that the CPU tier can hold the two against each other.  -> true: undecided, redo the block exactly
template <int QM>
bool streaming_body(int variant, Blk &b, uint32_t n, uint32_t nb, uint32_t hi, uint32_t lo, const svs::QimRule &rule) {
    if (svs::rows_for((int)n) == 1) return svs::embed_block_guarded<QM>(b.x, b.y, n, nb, hi, lo, rule);
    if (variant == EMU_GENERIC_GUARDED2) return svs::embed_block_guarded2<QM, 0, false>(b.x, b.y, n, nb, hi, lo, rule);
    constexpr bool INPLACE = QM != svs::QM_POW2;
    if (n == 10) return svs::embed_block_guarded2<QM, 10, INPLACE>(b.x, b.y, n, nb, hi, lo, rule);
    return svs::embed_block_guarded2<QM, 0, INPLACE>(b.x, b.y, n, nb, hi, lo, rule);
}

// what embed_exact_kernel<QM, U, ..> calls: its dithered side (U = 8 only), or the side from before the dither
template <int QM>
void exact_body(int rows, Blk &b, uint32_t n, uint32_t nb, uint32_t hi, uint32_t lo, const svs::QimRule &rule, bool constant,
                const svs::CoeffTable *sel, bool dithered, uint32_t s_b) {
    if (dithered) svs::embed_block_exact<8, QM, true>(b.x, b.y, n, nb, hi, lo, rule, constant, sel, s_b);
    else if (rows == 1) svs::embed_block_exact<1, QM>(b.x, b.y, n, nb, hi, lo, rule, constant);
    else if (rows == 2) svs::embed_block_exact<2, QM>(b.x, b.y, n, nb, hi, lo, rule, constant);
    else svs::embed_block_exact<8, QM>(b.x, b.y, n, nb, hi, lo, rule, constant, sel);
}

bool is_constant(const Blk &b) {
    bool constant = true;
    for (int r = 0; r < 8 && constant; ++r)
        constant = b.x[r] == (b.x[0] & 0xffu) * 0x01010101u && b.y[r] == (b.x[0] & 0xffu) * 0x01010101u;
    return constant;
}

void embed_call(const EmuCall &c, EmuResult &r) {
    Selection s;
    if (!make_selection(c, s) || c.order) { r.used = ~0ull; return; }
    const Grid g(c);
    if (c.frames_out != c.frames_in) std::memcpy(c.frames_out, c.frames_in, (size_t)(c.F * g.H * g.W));
    const svs::EmbedPlan p = svs::plan_embed(route(c, s, g.total));
    r.word = svs::rule_word(p.nearest, p.minmove, p.half_cell);
    r.path = (int32_t)p.path; r.rows = p.rows; r.qm = p.qm; r.selected = p.selected; r.dithered = p.dithered;
    r.nearest = p.nearest; r.minmove = p.minmove;
    r.used = p.use;
    if (p.path == svs::EmbedPath::COPY) return;
    const svs::QimRule rule = svs::rule_from_word(p.qp, r.word);   // what the kernels build from Geometry::pad
    // the table the exact kernel reads, as it picks it from its launch arguments (svs_route.hpp embed_tables)
    const svs::LaunchTables t = svs::embed_tables(p, svs::KernelOptions{{}, s.given ? &s.table : nullptr, {}});
    const svs::CoeffTable *sel = t.dith.on ? &t.dith.sel : t.sel.count ? &t.sel : nullptr;
    const bool streaming = p.path == svs::EmbedPath::STREAMING && c.streaming_bodies;
    const int rows = c.exact_rows ? c.exact_rows : p.rows;
    const int variant = p.use ? c.variant : EMU_AS_LAUNCHED;   // the test-only forms are forms of a block with payload
    const uint32_t seed = svs::dither_seed(c.dither_key);
    const uint32_t *words = reinterpret_cast<const uint32_t *>(c.bits);
    const uint32_t n = p.n_ac, n_words = (uint32_t)(c.bits_bytes / 4);
    // ROUND_TRIP (nothing can be embedded): every block is entered with one pass bit and no coefficient, as the kernel is launched
    auto budget = [&](uint64_t first) { return p.use ? svs::block_budget(first, p.n_bits, n) : 1u; };
    auto window = [&](uint64_t first, uint32_t &hi, uint32_t &lo) {
        hi = lo = 0;
        if (p.use) svs::payload_window(words, n_words, p.bit_offset + first, hi, lo);
    };
    with_qm(c.force_qm < 0 ? p.qm : c.force_qm, [&](auto qm) {
        constexpr int QM = decltype(qm)::value;
        for (uint64_t gb = 0; gb < g.total; ++gb) {
            const uint64_t first = gb * n;
            const uint32_t nb = budget(first);
            if (nb == 0) break;
            uint8_t *px = g.block(c.frames_out, gb);
            Blk raw;
            raw.load(px, (size_t)g.W);
            uint32_t hi, lo;
            window(first, hi, lo);
            const uint32_t nb_b = variant == EMU_PAIR_FORM && g.wb % 2 == 0 && gb % 2 == 0 ? budget(first + n) : 0u;
            if (nb_b > 0) {   // this block and its right neighbour through the packed pair form
                Blk other;
                other.load(px + 8, (size_t)g.W);
                uint32_t hi_b, lo_b;
                window(first + n, hi_b, lo_b);
                svs::embed_block_exact_pair<8, QM>(raw.x, raw.y, other.x, other.y, n, nb, nb_b, hi, lo, hi_b, lo_b, rule);
                raw.store(px, (size_t)g.W);
                other.store(px + 8, (size_t)g.W);
                ++gb;
                continue;
            }
            const uint32_t s_b = svs::dither_block_seed(seed, c.first_frame + (uint32_t)(gb / g.bpf), (uint32_t)(gb % g.bpf));
            auto exact = [&](int u) {
                exact_body<QM>(u, raw, n, nb, hi, lo, rule, variant == EMU_CONSTANT_SHORTCUT && is_constant(raw), sel, p.dithered, s_b);
            };
            if (!streaming) {
                exact(rows);
            } else if (streaming_body<QM>(variant, raw, n, nb, hi, lo, rule)) {
                raw.load(px, (size_t)g.W);   // undecided: the in-place form leaves the rows half-written
                exact(8);                    // the replay covers all eight coefficient rows
                ++r.replayed;
                if (c.replay_map) c.replay_map[gb] = 1;
            }
            raw.store(px, (size_t)g.W);
        }
    });
}

// ---- extract -------------------------------------------------------------------------------------------------------------

// f(integral_constant U, integral_constant NFIX): the FAST instantiation csrc/svs_capi.hip launches for `rows` coefficient
// rows - compile-time n for the GUI's default 10
template <class F>
auto with_fast_rows(int rows, uint32_t n, F &&f) {
    using std::integral_constant;
    if (n == 10) return f(integral_constant<int, 2>{}, integral_constant<int, 10>{});
    switch (rows) {
        case 1: return f(integral_constant<int, 1>{}, integral_constant<int, 0>{});
        case 2: return f(integral_constant<int, 2>{}, integral_constant<int, 0>{});
        case 3: return f(integral_constant<int, 3>{}, integral_constant<int, 0>{});
        case 4: return f(integral_constant<int, 4>{}, integral_constant<int, 0>{});
        case 5: return f(integral_constant<int, 5>{}, integral_constant<int, 0>{});
        case 6: return f(integral_constant<int, 6>{}, integral_constant<int, 0>{});
        case 7: return f(integral_constant<int, 7>{}, integral_constant<int, 0>{});
        default: return f(integral_constant<int, 8>{}, integral_constant<int, 0>{});
    }
}

// what extract_exact_kernel<8, QM, ..> calls: the selected form with a selection, else the prefix form; either on its dithered side
template <int QM>
void extract_exact(const Blk &b, uint32_t n, const svs::QimParams &qp, const svs::CoeffTable *sel, bool dithered, uint32_t s_b,
                   uint32_t &hi, uint32_t &lo) {
    if (dithered && sel) svs::extract_block_exact_selected<QM, true>(b.x, b.y, *sel, qp, hi, lo, s_b);
    else if (dithered) svs::extract_block_exact<8, QM, true>(b.x, b.y, n, qp, hi, lo, s_b);
    else if (sel) svs::extract_block_exact_selected<QM>(b.x, b.y, *sel, qp, hi, lo);
    else svs::extract_block_exact<8, QM>(b.x, b.y, n, qp, hi, lo);
}

// The only extract walker.  A soft kind runs the soft side of extract_exact_kernel block by block - extract_block_soft with the
// tables of the launch - and sends every byte where the kernel's tail of that kind sends it: block b of frame f owns the n
// stream positions from (f N + slot(b)) n on, slot(b) = b without an order.  The wave tile, the LDS, the pre-reductions and the
// atomics are NOT modelled here; the -m gpu tests cover them.
void extract_call(const EmuCall &c, EmuResult &r) {
    Selection s;
    const Grid g(c);
    svs::ExtractPlan p;
    svs::LaunchTables t;
    if (!plan_extract_call(c, s, g.total, g.bpf, p, t)) { r.used = ~0ull; return; }
    r.path = (int32_t)p.path; r.rows = p.rows; r.qm = p.qm; r.selected = p.selected; r.dithered = p.dithered;
    r.soft = p.soft; r.vote = p.vote; r.hist = p.hist; r.keyed = p.keyed;
    const uint32_t n = s.n;
    r.used = g.total * n;
    if (!c.frames_in) return;
    const bool zeros = p.path == svs::ExtractPath::ZEROS;
    if (!p.soft) std::memset(c.bits_out, 0, (size_t)r.used);
    else if (zeros && c.output == EMU_SOFT && c.soft_out) std::memset(c.soft_out, 0, (size_t)r.used);   // nothing votes or is counted
    if (n == 0 || zeros) return;
    const svs::CoeffTable *sel = p.selected ? &s.table : nullptr;
    const bool fast = p.path == svs::ExtractPath::FAST && c.streaming_bodies;
    const uint32_t seed = svs::dither_seed(c.dither_key);
    auto emit = [&](uint64_t gb, uint32_t hi, uint32_t lo) {
        for (uint32_t k = 0; k < n; ++k) c.bits_out[gb * n + k] = (uint8_t)svs::window_bit(hi, lo, (int)k);
    };
    auto walk = [&](auto qm) {
        constexpr int QM = decltype(qm)::value;
        if (p.soft) {
            const svs::BlockOrderArgs ord = kernel_forms(c, s, g.bpf).ord;
            for (uint64_t gb = 0; gb < g.total; ++gb) {
                const uint64_t f = gb / g.bpf, b = gb % g.bpf;
                Blk raw;
                raw.load(g.block(c.frames_in, gb), (size_t)g.W);
                const uint64_t slot = p.keyed ? svs::block_to_slot((uint32_t)b, ord, svs::round_keys(ord, ord.first_frame + (uint32_t)f)) : b;
                const uint64_t first = (f * g.bpf + slot) * n;
                const uint32_t s_b = svs::dither_block_seed(t.dith.seed, t.dith.first_frame + (uint32_t)f, (uint32_t)b);
                svs::extract_block_soft<QM>(raw.x, raw.y, t.dith.sel, p.qp, t.soft, t.dith.on != 0u, s_b, [&](uint32_t k, uint32_t byte) {
                    const uint64_t i = first + k;
                    if (p.vote) { if (c.tally) c.tally[svs::vote_residue(i, t.soft)] += svs::vote_of(byte, i < t.soft.head); }
                    else if (p.hist) { if (c.hist) c.hist[f * svs::kHistBins + byte] += 1u; }
                    else if (c.soft_out) c.soft_out[i] = (uint8_t)byte;
                });
            }
            return;
        }
        if (fast && c.extract_wave > 0) {
            // step two of FAST extraction for EVERY block of an aligned group of blocks in which one block is a candidate, as
            // the kernels do it (one wave ballot; extract_kernel / extract_bgr_kernel).  With the product's margin that gives
            // the per-block result (svs_block.hpp, extract_block); with a margin scaled below 1 (tie_scale) it need not.
            const uint64_t wv = (uint64_t)(c.extract_wave > 128 ? 128 : c.extract_wave);
            Blk raws[128];
            uint32_t his[128], los[128];
            float off[128];
            bool cand[128];
            for (uint64_t g0 = 0; g0 < g.total; g0 += wv) {
                const uint64_t count = g.total - g0 < wv ? g.total - g0 : wv;
                bool any = false;
                for (uint64_t i = 0; i < count; ++i) {
                    raws[i].load(g.block(c.frames_in, g0 + i), (size_t)g.W);
                    cand[i] = with_fast_rows(p.rows, n, [&](auto u, auto nfix) {
                        return svs::extract_block_cheap<decltype(u)::value, QM, decltype(nfix)::value>(raws[i].x, raws[i].y, n, p.qp,
                                                                                                      his[i], los[i], off[i]);
                    });
                    any = any || cand[i];
                    if (c.candidate_map) c.candidate_map[g0 + i] = cand[i];
                }
                for (uint64_t i = 0; i < count; ++i) {
                    if (any && svs::extract_block_settle<QM>(raws[i].x, raws[i].y, n, p.qp, his[i], off[i])) {
                        svs::extract_block_exact<8, QM>(raws[i].x, raws[i].y, n, p.qp, his[i], los[i]);
                        ++r.replayed;
                    }
                    emit(g0 + i, his[i], los[i]);
                }
            }
            return;
        }
        for (uint64_t gb = 0; gb < g.total; ++gb) {
            Blk raw;
            raw.load(g.block(c.frames_in, gb), (size_t)g.W);
            uint32_t hi = 0, lo = 0;
            // -> true: some quantiser input is within the forward error bound of a tie: the kernels redo the block exactly
            const bool redo = fast && with_fast_rows(p.rows, n, [&](auto u, auto nfix) {
                return svs::extract_block<decltype(u)::value, QM, decltype(nfix)::value>(raw.x, raw.y, n, p.qp, hi, lo);
            });
            const uint32_t s_b = svs::dither_block_seed(seed, c.first_frame + (uint32_t)(gb / g.bpf), (uint32_t)(gb % g.bpf));
            if (redo || !fast) extract_exact<QM>(raw, n, p.qp, sel, p.dithered, s_b, hi, lo);
            r.replayed += redo;
            emit(gb, hi, lo);
        }
    };
    // the plan names QM_F32 or QM_POW2: the double mode only differs in requantisation, not needed here
    if (p.qm == svs::QM_POW2) walk(std::integral_constant<int, svs::QM_POW2>{});
    else walk(std::integral_constant<int, svs::QM_F32>{});
}

// ---- read-back -------------------------------------------------------------------------------------------------------------

template <int QM>
uint32_t readback_rows(int rows, Blk &b, uint32_t nb, uint32_t hi, uint32_t lo, const svs::QimParams &qp) {
    if (rows == 1) return svs::readback_step<1, QM>(b.x, b.y, nb, hi, lo, qp);
    if (rows == 2) return svs::readback_step<2, QM>(b.x, b.y, nb, hi, lo, qp);
    return svs::readback_step<8, QM>(b.x, b.y, nb, hi, lo, qp);
}

// The read-back pass (csrc/svs_device.hpp readback_kernel / readback_keyed) in place over the stego of the same call without
// read-back.  keyed_form works for a prefix without a dither too, so that the tests can hold it to readback_step there.
void readback_call(const EmuCall &c, EmuResult &r) {
    Selection s;
    if (!make_selection(c, s) || (!c.keyed_form && (s.given || c.dither))) { r.used = ~0ull; return; }
    const Grid g(c);
    svs::RouteArgs ra = route(c, s, g.total);
    ra.readback = true;
    const svs::EmbedPlan p = svs::plan_embed(ra);
    if (c.status) std::memset(c.status, 3, g.total);
    r.used = p.use;
    if (p.use == 0) return;
    const svs::BlockOrderArgs ord = svs::make_block_order(c.order_key, c.first_frame, (uint32_t)g.bpf);
    const uint32_t seed = svs::dither_seed(c.dither_key);
    const uint32_t n = s.n, n_words = (uint32_t)(c.bits_bytes / 4);
    with_qm(p.qm, [&](auto qm) {
        constexpr int QM = decltype(qm)::value;
        for (uint64_t gb = 0; gb < g.total; ++gb) {
            const uint64_t f = gb / g.bpf, b = gb % g.bpf;
            // the stream slot of the block under the keyed order; the dither is that of its PHYSICAL position
            const uint64_t slot = c.order ? svs::block_to_slot((uint32_t)b, ord, svs::round_keys(ord, ord.first_frame + (uint32_t)f)) : b;
            const uint64_t first = (f * g.bpf + slot) * n;
            const uint32_t nb = svs::block_budget(first, p.n_bits, n);
            if (nb == 0) continue;
            uint8_t *px = g.block(c.frames_out, gb);
            Blk raw;
            raw.load(px, (size_t)g.W);
            uint32_t hi, lo;
            svs::payload_window(reinterpret_cast<const uint32_t *>(c.bits), n_words, p.bit_offset + first, hi, lo);
            const uint32_t s_b = svs::dither_block_seed(seed, c.first_frame + (uint32_t)f, (uint32_t)b);
            const uint32_t st = c.keyed_form ? svs::readback_step_keyed<QM>(raw.x, raw.y, s.table, nb, hi, lo, p.qp, c.dither != 0, s_b)
                                             : readback_rows<QM>(p.rows, raw, nb, hi, lo, p.qp);
            if (st == 1) raw.store(px, (size_t)g.W);
            r.repaired += st == 1;
            r.unrepaired += st == 2;
            if (c.status) c.status[gb] = (uint8_t)st;
        }
    });
}

// a call with the product's bounds, the plan's quantiser, the bodies as launched and the U = 8 exact body
EmuCall plain_call(const uint8_t *in, uint8_t *out, int F, int H, int W, double delta, int n_ac) {
    EmuCall c{sizeof(EmuCall)};
    c.frames_in = in; c.frames_out = out;
    c.F = F; c.H = H; c.W = W;
    c.delta = delta; c.n_ac = n_ac;
    c.guard_scale = c.tie_scale = 1.0f;
    c.force_qm = -1;
    c.exact_rows = 8;
    c.streaming_bodies = 1;
    return c;
}

}  // namespace

extern "C" {

// -> 0, or -1 when either struct is not the one this library was built with
int emu_embed_call(const EmuCall *c, EmuResult *r) { return sizes_match(c, r) ? (embed_call(*c, *r), 0) : -1; }
int emu_extract_call(const EmuCall *c, EmuResult *r) { return sizes_match(c, r) ? (extract_call(*c, *r), 0) : -1; }
int emu_readback_call(const EmuCall *c, EmuResult *r) { return sizes_match(c, r) ? (readback_call(*c, *r), 0) : -1; }

// The `exact` argument of emu_embed: 0 = flags 0, 1 = SVS_EXACT_POCKETFFT, 4 = SVS_EXACT_GUARDED, routed as svs_embed_dev
// routes them.  The test-only modes route as 1 (2: EMU_PAIR_FORM; 3: EMU_CONSTANT_SHORTCUT) and as 4 (5: EMU_GENERIC_GUARDED2).
// Every mode gives the reference's pixels.
void emu_exact_mode(EmuCall *c, int exact) {
    c->pocketfft = exact >= 1 && exact <= 3;
    c->guarded = exact == 4 || exact == 5;
    c->variant = exact == 2 ? EMU_PAIR_FORM : exact == 3 ? EMU_CONSTANT_SHORTCUT : exact == 5 ? EMU_GENERIC_GUARDED2 : EMU_AS_LAUNCHED;
}

// frames: contiguous [F][H][W]; bits: packed MSB-first, padded by the caller to a multiple of 4 bytes; exact: emu_exact_mode
uint64_t emu_embed(const uint8_t *gray, uint8_t *stego, int F, int H, int W, double delta, int n_ac,
                   const uint8_t *bits, uint64_t bits_bytes, uint64_t bit_offset, uint64_t n_bits, int exact,
                   uint64_t *n_replayed) {
    EmuCall c = plain_call(gray, stego, F, H, W, delta, n_ac);
    c.bits = bits; c.bits_bytes = bits_bytes; c.bit_offset = bit_offset; c.n_bits = n_bits;
    emu_exact_mode(&c, exact);
    EmuResult r{sizeof(EmuResult)};
    embed_call(c, r);
    if (n_replayed) *n_replayed = r.replayed;
    return r.used;
}

// out_flags: one byte (0/1) per extracted bit, F*(H/8)*(W/8)*n entries; exact != 0: SVS_EXACT_POCKETFFT
uint64_t emu_extract(const uint8_t *gray, int F, int H, int W, double delta, int n_ac, uint8_t *out_flags, int exact,
                     uint64_t *n_redone) {
    EmuCall c = plain_call(gray, nullptr, F, H, W, delta, n_ac);
    c.pocketfft = exact != 0;
    c.bits_out = out_flags;
    EmuResult r{sizeof(EmuResult)};
    extract_call(c, r);
    if (n_redone) *n_redone = r.replayed;
    return r.used;
}

}  // extern "C"

#include "emu_probes.hpp"
