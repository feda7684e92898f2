// svs_capi.hip - the C ABI declared in include/svsdct.h (host side + kernel launches).
// Build: hipcc --offload-arch=gfx950 -O3 -shared -fPIC  (see csrc/Makefile)
#include "svsdct.h"
#include "svs_abi.hpp"
#include "svs_device.hpp"
#include "svs_route.hpp"
#include "svs_stage.hpp"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace {

#define SVS_HIP(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return fail(SVS_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

using svs::make_div;   // svs_index.hpp

// Experiment knobs.  The PRODUCT build reads no environment variable at all: `knob()` folds to its compiled-in default, so
// no variable can reroute a kernel, let alone touch the parity guarantee of a flag.  The experiments
// library (-DSVS_EXPERIMENTS, lib/variants/libsvsdct_exp.so) reads SVS_GUARDED_OFF and SVS_STAGE_CHUNK_KB from the
// environment on every call; the tests and tools/ab_bench.py --env-sweep load it (SVSDCT_LIB=...).
#if defined(SVS_EXPERIMENTS)
uint32_t knob(const char *name, uint32_t dflt) {
    const char *v = getenv(name);
    return v ? (uint32_t)strtoul(v, nullptr, 10) : dflt;
}
#else
constexpr uint32_t knob(const char *, uint32_t dflt) { return dflt; }
#endif

// The routing arguments of a call (svs_route.hpp).  Test hooks of the experiments library: SVS_GUARDED_OFF sends the gray
// embed to the exact kernel and GUARDED extraction to the pocketfft-identical one; SVS_GUARD_SCALE multiplies BETA's
// coefficients (the streaming embed kernels' guard), SVS_TIE_SCALE the tie margin of FAST extraction.  Below 1 the result is
// NOT the reference's any more: tests/test_gpu_guard_sensitivity.py uses them to show that the suite notices a bound that is
// too tight.  tests/hostemu applies the same scales (emu_set_guard_scale / emu_set_tie_scale).
svs::RouteArgs route_args(double delta, const svs::Geometry &g, uint64_t total, uint64_t n_bits, uint64_t bit_offset,
                          uint32_t flags, bool bgr) {
    svs::RouteArgs a{delta, g.n_ac, total, n_bits, bit_offset, (flags & SVS_EXACT_POCKETFFT) != 0,
                     (flags & SVS_EXACT_GUARDED) != 0, bgr, knob("SVS_GUARDED_OFF", 0) != 0, 1.0f, 1.0f};
#if defined(SVS_EXPERIMENTS)
    if (const char *sc = getenv("SVS_GUARD_SCALE")) a.guard_scale = (float)atof(sc);
    if (const char *sc = getenv("SVS_TIE_SCALE")) a.tie_scale = (float)atof(sc);
#endif
    a.nearest = (flags & SVS_NEAREST) != 0;
    a.minmove = (flags & SVS_MINMOVE) != 0;
    return a;
}

// Occupancy cap: unused dynamic LDS such that at most `wg_per_cu` workgroups fit the CU's 160 KB.  The one-row embed kernel
// runs FASTER with fewer waves in flight than its register count allows (see embed_wg_per_cu).
uint32_t lds_pad_for(uint32_t wg_per_cu, uint32_t static_lds) {
    const uint32_t per_wg = (160u * 1024u / wg_per_cu) & ~255u;
    return per_wg > static_lds ? per_wg - static_lds : 0;
}

int clamp_ac(int n_ac) { return n_ac < 0 ? 0 : (n_ac > 63 ? 63 : n_ac); }

// validates the plane description and fills the kernel geometry
int make_geometry(const svs_planes *p, int n_ac, svs::Geometry *g, uint64_t *total_blocks) {
    if (!p) return fail(SVS_ERR_INVALID_ARG, "planes is NULL");
    if (p->reserved != 0) return fail(SVS_ERR_INVALID_ARG, "svs_planes.reserved must be 0");
    if (p->n_frames < 0 || p->height <= 0 || p->width <= 0)
        return fail(SVS_ERR_INVALID_ARG, "bad frame geometry %d x %d x %d", p->n_frames, p->height, p->width);
    if ((p->height % 8) || (p->width % 8))
        return fail(SVS_ERR_INVALID_ARG, "height and width must be multiples of 8 (got %d x %d)", p->height, p->width);
    if (p->row_pitch < p->width || (p->row_pitch % 8))
        return fail(SVS_ERR_INVALID_ARG, "row_pitch %lld must be >= width and a multiple of 8", (long long)p->row_pitch);
    if (p->frame_pitch < (int64_t)p->height * p->row_pitch || (p->frame_pitch % 8))
        return fail(SVS_ERR_INVALID_ARG, "frame_pitch %lld must be >= height*row_pitch and a multiple of 8",
                    (long long)p->frame_pitch);
    const uint64_t wb = (uint64_t)p->width / 8, hb = (uint64_t)p->height / 8;
    const uint64_t bpf = wb * hb, total = bpf * (uint64_t)p->n_frames;
    if (bpf >= (1ull << 31) || total >= (1ull << 31))
        return fail(SVS_ERR_INVALID_ARG, "batch has %llu blocks; at most 2^31-1 per call", (unsigned long long)total);
    g->by_wb = make_div((uint32_t)wb);
    g->by_bpf = make_div((uint32_t)bpf);
    g->total_blocks = (uint32_t)total;
    g->n_ac = (uint32_t)clamp_ac(n_ac);
    g->xcd_chunk = 0;
    g->pad = 0;
    g->row_pitch = p->row_pitch;
    g->frame_pitch = p->frame_pitch;
    *total_blocks = total;
    return SVS_OK;
}

// the planes of an extract call -> its geometry, blocks and capacity in bits (0: nothing to extract)
int extract_geometry(const svs_planes *p, int n_ac, svs::Geometry *g, uint64_t *total, uint64_t *cap, uint64_t *n_bits_out) {
    if (int rc = make_geometry(p, n_ac, g, total)) return rc;
    if (n_bits_out) *n_bits_out = 0;
    *cap = *total * (uint64_t)g->n_ac;
    return SVS_OK;
}

int check_capacity(uint64_t need, uint64_t have, const char *unit) {
    if (have >= need) return SVS_OK;
    return fail(SVS_ERR_CAPACITY, "extract needs %llu %s, buffer has %llu", (unsigned long long)need, unit, (unsigned long long)have);
}

uint64_t span_bytes(const svs_planes *p) {
    if (p->n_frames == 0) return 0;
    return (uint64_t)(p->n_frames - 1) * p->frame_pitch + (uint64_t)(p->height - 1) * p->row_pitch + p->width;
}

// ---- launch tuning (measured on MI355X, 600 x 4K frames; profiles/history/r01_ab_variants.txt) ----------------
// * workgroup -> tile mapping (svs::tile_id): giving each XCD-group a contiguous eighth of the batch lifts the embed kernels
//   ~+6..12 % (reads and writes of one XCD stay on neighbouring DRAM pages) and is never worse than the identity map.  The
//   extract kernels' maps: svs_route.hpp.
// * two blocks per lane (16-byte accesses) pays only for the embed kernel at one coefficient row; with more rows the extra
//   registers cost occupancy (n = 10: -17 %).  The one-row pocketfft-identical extract kernel keeps one block per lane: ahead
//   by 0.1 - 3 % on every large batch and level at 300 x 1080p, 37 instead of 54 VGPRs (profiles/r05_ab_extract_bpl.txt).
bool rows_allow_two_blocks(const svs_planes *p, const void *a, const void *b) {
    return ((p->width / 8) % 2 == 0) && (p->row_pitch % 16 == 0) && (p->frame_pitch % 16 == 0) &&
           ((uintptr_t)a % 16 == 0) && (b == nullptr || (uintptr_t)b % 16 == 0);
}

// Occupancy cap of the one-row embed kernel (workgroups of 256 threads per CU = waves per SIMD).  Round 6, the integer-domain
// kernel (66 - 71 VGPRs: 7 waves per SIMD uncapped): measured with pure copies, the rate of this access pattern falls - and its
// dependence on where the buffers were placed grows - with the BYTES IN FLIGHT per SIMD (rows per lane x waves: 8 x 4 behaves
// like 16 x 2 and 4 x 8, profiles/r06_stream_probe.txt); the kernel is fastest at 4 - 5 waves with two blocks per lane (1.52 /
// 1.61 ms per 600 x 4K on fast / slow placements against 1.55 - 1.70 uncapped, the same at n = 1, 7 and at 1080p:
// profiles/r06_place_new_vs_old.txt, r06_caps.txt) and at 6 with one block per lane.  Every other kernel has always been
// fastest uncapped.
uint32_t embed_wg_per_cu(int bpl) { return bpl == 2 ? 4u : 6u; }

// Measurement hook of the EXPERIMENTS library only (svs_guard_counter_set): a device counter the streaming embed launches add
// the number of blocks they redid exactly to.  The product library has neither the global nor the kernel parameter: no state
// survives a call (include/svsdct.h).
#if defined(SVS_EXPERIMENTS)
unsigned long long *g_guard_counter = nullptr;
#define SVS_COUNTER_ARG , g_guard_counter

struct DevBuf {  // RAII (measurement hooks)
    void *p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};
#else
#define SVS_COUNTER_ARG
#endif

// ---- kernel dispatch --------------------------------------------------------------------------------------------------
// dispatch<Vs...>(v, f) calls f(std::integral_constant<int, v>) when v is one of Vs.  Each call site lists the values it
// instantiates: the kernel families have exactly these instantiations, and nothing else is compiled.
template <int V, int... Vs, class F>
int dispatch(int v, F &&f) {
    if (v == V) return f(std::integral_constant<int, V>{});
    if constexpr (sizeof...(Vs) > 0) return dispatch<Vs...>(v, f);
    else return fail(SVS_ERR_INVALID_ARG, "internal: no kernel instantiation for %d", v);
}

template <class F>
int with_bool(bool b, F &&f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

dim3 grid_for(uint64_t total_blocks, int bpl = 1) { return dim3((uint32_t)((total_blocks + SVS_WG * bpl - 1) / (SVS_WG * bpl))); }

template <class K, class... A>
int launch(K kernel, dim3 grid, uint32_t lds, hipStream_t st, A... args) {
    hipLaunchKernelGGL(kernel, grid, dim3(SVS_WG), lds, st, args...);
    SVS_HIP(hipGetLastError());
    return SVS_OK;
}

using svs::EmbedPath;
using svs::ExtractPath;

// svs_embed_dev's plan: embed_row1_kernel (one coefficient row, and the copy), embed_kernel<2> (two rows) or embed_exact_kernel.
// `two`: two blocks per lane, where the plan and the buffers allow it.  A keyed plan (p.keyed, `ord` its order) launches the
// KEYED instantiation of the same kernel family, with the order as the last argument.  `k`: the call's options in the kernels'
// forms (svs_route.hpp, which also says which tables the exact kernel gets).
// A matrix plan is the only embed launch with dynamic LDS: per wave a tile of 64 floats a slot, and as many again with the pair
// search (svs_device.hpp).  At most 63 KB: k = 6 without the search, k = 5 with it.
uint32_t matrix_lds_bytes(const svs::EmbedPlan &p) {
    return p.matrix ? (uint32_t)(SVS_WG / 64) * 64u * 4u * svs::matrix_slots(p.matrix) * ((p.matrix & 8u) ? 2u : 1u) : 0u;
}

int launch_embed(const svs::EmbedPlan &p, bool two, uint64_t total, hipStream_t st, const uint8_t *gray, uint8_t *stego,
                 svs::Geometry g, const uint32_t *bits, const svs::KernelOptions &k) {
    const svs::LaunchTables t = svs::embed_tables(p, k);
    const svs::BlockOrderArgs &ord = k.ord;
    g.n_ac = p.n_ac;
    g.xcd_chunk = p.xcd_chunk;
    g.pad = svs::rule_word(p.nearest, p.minmove, p.half_cell);
    const uint32_t words = (uint32_t)p.n_words;
    const uint32_t exact_lds = matrix_lds_bytes(p);   // 0 for every launch but a matrix plan's
    return dispatch<svs::QM_DOUBLE, svs::QM_POW2, svs::QM_F32>(p.qm, [&](auto qm) {
        constexpr int QM = decltype(qm)::value;
        if (p.path == EmbedPath::EXACT || p.path == EmbedPath::ROUND_TRIP)
            // the exact kernel's quantiser loop is instantiated for one or two coefficient rows (n <= 7: the benchmark's 3;
            // n <= 15: the reference GUI's 10) and for all eight (any n): fewer wave-uniform tests per block, same arithmetic
            return dispatch<1, 2, 8>(p.rows, [&](auto u) {
                constexpr int U = decltype(u)::value;
                if (p.keyed)
                    return launch(svs::embed_exact_kernel<QM, U, true, svs::BlockOrderArgs>, grid_for(total), exact_lds, st, gray, stego, g,
                                  p.qp, bits, p.bit_offset, p.n_bits, words, t.sel, t.dith, svs::ChannelArgs{}, t.steps, ord);
                return launch(svs::embed_exact_kernel<QM, U>, grid_for(total), exact_lds, st, gray, stego, g, p.qp, bits,
                              p.bit_offset, p.n_bits, words, t.sel, t.dith, svs::ChannelArgs{}, t.steps);
            });
        if (p.rows == 2) {   // n = 10 (the reference GUI's default, app.py:69; BASELINE configs[1]) has a compile-time-n instantiation
            if (p.keyed)
                return launch(svs::embed_kernel<2, QM, 1, 0, true, svs::BlockOrderArgs>, grid_for(total), 0, st, gray, stego, g, p.qp,
                              bits, p.bit_offset, p.n_bits, words SVS_COUNTER_ARG, ord);
            return g.n_ac == 10 ? launch(svs::embed_kernel<2, QM, 1, 10>, grid_for(total), 0, st, gray, stego, g, p.qp, bits,
                                         p.bit_offset, p.n_bits, words SVS_COUNTER_ARG)
                                : launch(svs::embed_kernel<2, QM, 1>, grid_for(total), 0, st, gray, stego, g, p.qp, bits,
                                         p.bit_offset, p.n_bits, words SVS_COUNTER_ARG);
        }
        // one coefficient row: the integer-domain kernel (round 6), under its occupancy cap
        return dispatch<1, 2>(two ? 2 : 1, [&](auto bpl) {
            constexpr int BPL = decltype(bpl)::value;
            const uint32_t lds = lds_pad_for(embed_wg_per_cu(BPL), svs::kRow1StaticLds);
            if (p.keyed)
                return launch(svs::embed_row1_kernel<QM, BPL, true, svs::BlockOrderArgs>, grid_for(total, BPL), lds, st, gray, stego, g,
                              p.qp, bits, p.bit_offset, p.n_bits, words SVS_COUNTER_ARG, ord);
            return launch(svs::embed_row1_kernel<QM, BPL>, grid_for(total, BPL), lds, st, gray, stego, g, p.qp, bits, p.bit_offset,
                          p.n_bits, words SVS_COUNTER_ARG);
        });
    });
}

// svs_requantise_dev: the channel side of the one exact embed instantiation that holds it (svs_device.hpp).  No payload, no
// quantiser parameters, no tables: the kernel reads the geometry and `chan` alone.
int launch_requantise(uint64_t total, hipStream_t st, const uint8_t *in, uint8_t *out, svs::Geometry g, const svs::ChannelArgs &chan) {
    g.n_ac = 0;
    g.xcd_chunk = svs::kEighth;
    return launch(svs::embed_exact_kernel<svs::QM_DOUBLE, 8>, grid_for(total), 0, st, in, out, g, svs::QimParams{},
                  static_cast<const uint32_t *>(nullptr), (uint64_t)0, (uint64_t)0, (uint32_t)0, svs::CoeffTable{}, svs::DitherArgs{}, chan,
                  svs::StepArgs{});
}

// SVS_READBACK: readback_kernel<rows, QM> over the stego planes the embed has just written, on the same stream, with the
// embed's payload arguments (the plan's rows are 1 or 2 for n <= 15, else 8: the quantiser loop's coefficient rows).
// The colour calls pass their BGR output as `stego`, its pitches and the call's weights in `colour`, and form = SVS_RB_BGR:
// they run the colour body of their quantiser mode, which lives in one instantiation (plain and keep-colour output alike).
// A plan with a non-prefix selection or a dither (svs_embed_dithered_readback_dev; `k` as launch_embed takes it) runs the keyed
// form, form = SVS_RB_SEL + its quantiser mode, in the same instantiation, with svs_route.hpp's readback_tables; a call
// without an order adds SVS_RB_RASTER.  A stepped plan (svs_stepped_embed_readback_dev) runs the stepped form, form = SVS_RB_STEP,
// there too: the same tables and the call's StepArgs, which every other launch passes empty.
int launch_readback(const svs::EmbedPlan &p, uint64_t total, hipStream_t st, uint8_t *stego, svs::Geometry g, const uint32_t *bits,
                    uint64_t *counts, const svs::KernelOptions &k, const svs::ColourParams &colour, uint32_t form) {
    const svs::BlockOrderArgs &ord = k.ord;
    g.n_ac = p.n_ac;
    g.xcd_chunk = svs::kEighth;
    const uint32_t words = (uint32_t)p.n_words;
    auto *c = reinterpret_cast<unsigned long long *>(counts);
    const svs::DitherArgs none{};
    const svs::StepArgs no_steps{};
    if (form != SVS_RB_GRAY)   // the one instantiation that holds the colour bodies (svs_device.hpp SVS_RB_HOSTS_COLOUR)
        return launch(svs::readback_kernel<8, svs::QM_POW2, true, svs::BlockOrderArgs>, grid_for(total), 0, st, stego, g, p.qp, bits,
                      p.bit_offset, p.n_bits, words, c, colour, (uint32_t)(SVS_RB_BGR + p.qm), none, no_steps, svs::BlockOrderArgs{});
    if (p.stepped)   // ... the stepped body
        return launch(svs::readback_kernel<8, svs::QM_POW2, true, svs::BlockOrderArgs>, grid_for(total), 0, st, stego, g, p.qp, bits,
                      p.bit_offset, p.n_bits, words, c, colour, (uint32_t)(SVS_RB_STEP + (p.keyed ? 0u : SVS_RB_RASTER)),
                      svs::readback_tables(p, k), k.steps, ord);
    if (p.selected || p.dithered)   // ... and the keyed bodies
        return launch(svs::readback_kernel<8, svs::QM_POW2, true, svs::BlockOrderArgs>, grid_for(total), 0, st, stego, g, p.qp, bits,
                      p.bit_offset, p.n_bits, words, c, colour, (uint32_t)(SVS_RB_SEL + p.qm + (p.keyed ? 0u : SVS_RB_RASTER)),
                      svs::readback_tables(p, k), no_steps, ord);
    return dispatch<svs::QM_DOUBLE, svs::QM_POW2, svs::QM_F32>(p.qm, [&](auto qm) {
        constexpr int QM = decltype(qm)::value;
        return dispatch<1, 2, 8>(p.rows, [&](auto u) {
            constexpr int U = decltype(u)::value;
            if (p.keyed)
                return launch(svs::readback_kernel<U, QM, true, svs::BlockOrderArgs>, grid_for(total), 0, st, stego, g, p.qp, bits,
                              p.bit_offset, p.n_bits, words, c, colour, form, none, no_steps, ord);
            return launch(svs::readback_kernel<U, QM>, grid_for(total), 0, st, stego, g, p.qp, bits, p.bit_offset, p.n_bits, words, c,
                          colour, form, none, no_steps);
        });
    });
}

// svs_embed_bgr_dev's plan: embed_bgr_kernel<8, QM, true> (exact, round trip) or <1 | 2, QM, false> (streaming, convert).
// A plan with the read-back bit (svs_embed_bgr_readback_dev) is followed by readback_kernel in its colour form, in place on
// `out` (counts: device, added to; NULL for none).
int launch_embed_bgr(const svs::EmbedPlan &p, bool keep, uint64_t total, hipStream_t st, const uint8_t *in, uint8_t *out,
                     uint8_t *ref, svs::Geometry g, const svs::ColourParams &c, const uint32_t *bits, uint64_t *counts) {
    const svs::Geometry planes = g;
    g.n_ac = p.n_ac;
    g.xcd_chunk = p.xcd_chunk;
    g.pad = svs::rule_word(p.nearest, p.minmove, p.half_cell);
    const uint32_t words = (uint32_t)p.n_words;
    const bool exact = p.path == EmbedPath::EXACT || p.path == EmbedPath::ROUND_TRIP;
    if (int rc = dispatch<svs::QM_DOUBLE, svs::QM_POW2, svs::QM_F32>(p.qm, [&](auto qm) {
            return with_bool(keep, [&](auto keep_c) {
                constexpr int QM = decltype(qm)::value;
                constexpr bool KEEP = decltype(keep_c)::value;
                if (exact)
                    return launch(svs::embed_bgr_kernel<8, QM, true, KEEP>, grid_for(total), 0, st, in, out, ref, g, c, p.qp, bits,
                                  p.bit_offset, p.n_bits, words);
                return dispatch<1, 2>(p.rows, [&](auto u) {
                    return launch(svs::embed_bgr_kernel<decltype(u)::value, QM, false, KEEP>, grid_for(total), 0, st, in, out, ref, g,
                                  c, p.qp, bits, p.bit_offset, p.n_bits, words);
                });
            });
        }))
        return rc;
    if (!(p.readback && p.use > 0)) return SVS_OK;
    svs::ColourParams in_place = c;   // the pass reads and writes the output
    in_place.in_row_pitch = c.out_row_pitch;
    in_place.in_frame_pitch = c.out_frame_pitch;
    return launch_readback(p, total, st, out, planes, bits, counts, svs::KernelOptions{}, in_place, SVS_RB_BGR);
}

// svs_extract_dev's plan: extract_exact_kernel<1..8> or extract_kernel<2..8>.  A keyed plan ORs every block's bits into its
// slot with global atomics (svs_device.hpp, or_bits_global): the output is cleared first, on the same stream.  A soft plan
// (EXACT, rows = 8) switches the kernel's soft side on and is the only launch with dynamic LDS: a tile of 64 n bytes per wave;
// every byte of its output has one writer, so nothing is cleared (ZEROS: out_bytes, the capacity, of zero bytes).  A vote plan
// is a soft plan whose `out` is the caller's tally of out_bytes = 4 period bytes, added to and never cleared (never ZEROS).
// A histogram plan is a soft plan whose `out` is the caller's n_frames * 256 uint32 counts, added to and never cleared; it alone
// requests 256 dwords more, the workgroup's table of counters behind the tiles.
uint32_t soft_lds_bytes(const svs::ExtractPlan &p) {
    return p.soft ? (uint32_t)(SVS_WG / 64) * 64u * p.n_ac + (p.hist ? 4u * svs::kHistBins : 0u) : 0u;
}

int launch_extract(const svs::ExtractPlan &p, uint64_t total, hipStream_t st, const uint8_t *gray, svs::Geometry g, uint8_t *out,
                   uint64_t out_bytes, const svs::KernelOptions &k) {
    const svs::LaunchTables t = svs::extract_tables(p, k);
    const svs::BlockOrderArgs &ord = k.ord;
    if (p.path == ExtractPath::ZEROS || (p.keyed && !p.soft)) SVS_HIP(hipMemsetAsync(out, 0, out_bytes, st));
    if (p.path == ExtractPath::ZEROS) return SVS_OK;
    g.xcd_chunk = p.xcd_chunk;
    return dispatch<svs::QM_POW2, svs::QM_F32>(p.qm, [&](auto qm) {
        constexpr int QM = decltype(qm)::value;
        if (p.path == ExtractPath::EXACT)
            return dispatch<1, 2, 3, 4, 5, 6, 7, 8>(p.rows, [&](auto r) {
                constexpr int U = decltype(r)::value;
                if (p.keyed)
                    return launch(svs::extract_exact_kernel<U, QM, 1, true, svs::BlockOrderArgs>, grid_for(total), soft_lds_bytes(p), st,
                                  gray, g, p.qp, out, out_bytes, t.sel, t.dith, t.soft, t.steps, ord);
                return launch(svs::extract_exact_kernel<U, QM>, grid_for(total), soft_lds_bytes(p), st, gray, g, p.qp, out, out_bytes,
                              t.sel, t.dith, t.soft, t.steps);
            });
        if (p.keyed)
            return dispatch<2, 3, 4, 5, 6, 7, 8>(p.rows, [&](auto r) {
                return launch(svs::extract_kernel<decltype(r)::value, QM, 1, 0, true, svs::BlockOrderArgs>, grid_for(total), 0, st, gray,
                              g, p.qp, out, out_bytes, ord);
            });
        // n = 10 (the reference GUI's default) has a compile-time-n instantiation of the extract kernel: +1..7 %
        // (profiles/history/r01_ab_quant_exact.txt).  The same specialisation of the embed kernel measured SLOWER (-13 % at
        // 600 x 4K, n = 10) and n = 3 gains nothing (HBM-bound), so those stay on the run-time-n kernels.
        if (g.n_ac == 10) return launch(svs::extract_kernel<2, QM, 1, 10>, grid_for(total), 0, st, gray, g, p.qp, out, out_bytes);
        return dispatch<2, 3, 4, 5, 6, 7, 8>(p.rows, [&](auto r) {
            return launch(svs::extract_kernel<decltype(r)::value, QM, 1>, grid_for(total), 0, st, gray, g, p.qp, out, out_bytes);
        });
    });
}

// svs_extract_bgr_dev's plan: extract_bgr_kernel<1..8, QM, false> (pocketfft-identical forward) or <2..8, QM, true> (FAST)
int launch_extract_bgr(const svs::ExtractPlan &p, uint64_t total, hipStream_t st, const uint8_t *bgr, svs::Geometry g,
                       const svs::ColourParams &c, uint8_t *out, uint64_t out_bytes) {
    if (p.path == ExtractPath::ZEROS) {
        SVS_HIP(hipMemsetAsync(out, 0, out_bytes, st));
        return SVS_OK;
    }
    g.xcd_chunk = p.xcd_chunk;
    return dispatch<svs::QM_POW2, svs::QM_F32>(p.qm, [&](auto qm) {
        constexpr int QM = decltype(qm)::value;
        if (p.path == ExtractPath::FAST)
            return dispatch<2, 3, 4, 5, 6, 7, 8>(p.rows, [&](auto r) {
                return launch(svs::extract_bgr_kernel<decltype(r)::value, QM, true>, grid_for(total), 0, st, bgr, g, c, p.qp, out,
                              out_bytes);
            });
        return dispatch<1, 2, 3, 4, 5, 6, 7, 8>(p.rows, [&](auto r) {
            return launch(svs::extract_bgr_kernel<decltype(r)::value, QM, false>, grid_for(total), 0, st, bgr, g, c, p.qp, out,
                          out_bytes);
        });
    });
}

// ---------------------------------------------------------------------------------------------------------------------
// Staging context of the HOST-pointer entry points (svs_embed / svs_extract, their _str and _bgr forms).
// What the reference's per-frame call sites hit (embed_process.py:117-121, extract_process.py:64-68: NumPy arrays in, NumPy
// arrays out), so it has to run at the rate of the PCIe link, not of hipMalloc:
//   * one context per HOST THREAD (thread_local): two non-blocking streams and device buffers that grow on demand.  Once
//     they have grown to the largest call seen nothing is allocated or freed per call, except that a buffer above 64 MB
//     which eight calls in a row used less than a quarter of is given back (stage_reserve).  Every call reserves all the
//     buffers it needs at its entry, before it queues anything: hipFree waits for the device, and must not wait for the
//     call's own work.  svs_shutdown() (or the thread's exit) releases them.  No state carries RESULTS from one call to the
//     next - a call leaves nothing behind that a later call reads - and two host threads never share a context, so the
//     entry points stay re-entrant and thread-safe.
//   * the frames travel in chunks (whole frames, or bands of block rows of a large frame): every upload and kernel goes to
//     the context's UP stream, in order; every download to its DOWN stream, behind an event recorded after the chunk's
//     kernel - so chunk k+1's upload runs while chunk k's download does (the link is full duplex).  (Chunks dealt
//     round-robin to three streams fall into lockstep: all three upload together, then all three download, and the batch
//     moves at the SERIAL rate of the link, 26.6 instead of 40+ Gpixel/s, profiles/r05_pcie_rate.txt.)  The payload is
//     uploaded once; every chunk indexes it by bit offset.
//   * a host buffer that is page-locked (svs_host_alloc, hipHostMalloc, hipHostRegister) is the source / target of the DMA
//     itself; pageable memory goes through the runtime's staging (uploads at the same rate, downloads at about half of it,
//     a FRESH pageable result array - page faults - at a quarter: hand the library page-locked OUTPUT buffers, as
//     svsdct/hostmem.py does.  Page-locking a pageable output for the duration of the call - hipHostRegister - was measured:
//     17.5 instead of 22 ms per 32 x 4K into fresh arrays, but 0.54 instead of 0.45 ms per single 4K frame: not kept,
//     profiles/r05_pcie_rate.txt (G)).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kStageStreams = 2;      // st[0] = up (H2D copies + kernels), st[1] = down (D2H copies)
constexpr int kChunkEvents = 32;      // "kernel of chunk k done" events, reused round-robin (a stream wait captures the
                                      // event's record at the time of the call, so re-recording one later is safe)

struct Grow {   // device buffer of a staging context: grows on demand, shrinks when calls keep needing far less than it holds
    void *p = nullptr;
    size_t cap = 0;
    uint32_t oversized_calls = 0;   // consecutive calls that needed less than a quarter of it
};
constexpr size_t kStageKeepBytes = (size_t)64 << 20;   // a buffer up to this size is kept whatever the next call needs

struct HostStage {
    int device = -1;
    hipStream_t st[kStageStreams] = {nullptr, nullptr};
    hipEvent_t chunk_done[kChunkEvents] = {};
    uint32_t next_event = 0;
    Grow frames, second, third, bits;   // frames (in place) / BGR in; BGR out; gray reference or ASCII payload; packed payload / bits
    ~HostStage() { release(); }

    void release() {
        if (device < 0) return;
        int cur = -1;
        const bool switched = hipGetDevice(&cur) == hipSuccess && cur != device && hipSetDevice(device) == hipSuccess;
        for (auto &s : st) if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); s = nullptr; }
        for (auto &e : chunk_done) if (e) { (void)hipEventDestroy(e); e = nullptr; }
        for (Grow *g : {&frames, &second, &third, &bits}) { if (g->p) (void)hipFree(g->p); g->p = nullptr; g->cap = 0; }
        if (switched) (void)hipSetDevice(cur);
        (void)hipGetLastError();
        device = -1;
    }
};

thread_local HostStage t_stage;

// the calling thread's context on its current device (created / moved on demand)
int stage_acquire(HostStage **out) {
    int dev = 0;
    SVS_HIP(hipGetDevice(&dev));
    HostStage &c = t_stage;
    if (c.device != dev) {
        c.release();
        c.device = dev;                    // from here on release() undoes whatever has been created
        hipError_t err = hipSuccess;
        for (auto &s : c.st) if (err == hipSuccess) err = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
        for (auto &e : c.chunk_done) if (err == hipSuccess) err = hipEventCreateWithFlags(&e, hipEventDisableTiming);
        if (err != hipSuccess) {
            c.release();
            return fail(SVS_ERR_HIP, "creating the staging context failed: %s", hipGetErrorString(err));
        }
    }
    *out = &c;
    return SVS_OK;
}

int stage_reserve(Grow &g, size_t bytes) {
    const size_t want = (bytes + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);   // whole 2 MB pages
    // enough, and not grossly more for long: a thread that once staged a multi-GB batch does not keep that HBM for good (ADVICE
    // r05) - a buffer above 64 MB that eight calls in a row used less than a quarter of is given back (eight: a caller that
    // alternates large and small batches must not pay a hipFree + hipMalloc per call)
    if (bytes <= g.cap) {
        const bool oversized = g.cap > kStageKeepBytes && g.cap / 4 > want;
        g.oversized_calls = oversized ? g.oversized_calls + 1 : 0;
        if (g.oversized_calls < 8) return SVS_OK;
    }
    g.oversized_calls = 0;
    if (g.p) { SVS_HIP(hipFree(g.p)); g.p = nullptr; g.cap = 0; }
    SVS_HIP(hipMalloc(&g.p, want));
    g.cap = want;
    return SVS_OK;
}

// host -> device on `st`.  Page-locked source: the DMA reads it (the caller keeps it alive until the stream is synchronised,
// which every entry point does before it returns).  Pageable source: the runtime's own staging - hipMemcpyAsync then returns
// when the bytes have been read.  (Round 5 measured a staging ring of the context's own - memcpy into pinned slots beside
// the DMA - against it: 9.7 vs 6.3 ms per 265 MB upload, 0.39 vs 0.34 ms per 4K frame; the runtime pins the caller's pages
// in place and moves them at the rate of page-locked memory.  profiles/r05_pcie_rate.txt.)
int stage_h2d(hipStream_t st, void *d_dst, const void *h_src, size_t bytes) {
    if (bytes == 0) return SVS_OK;
    SVS_HIP(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, st));
    return SVS_OK;
}

// device -> host on `st`; complete when the call's streams are drained
int stage_d2h(hipStream_t st, void *h_dst, const void *d_src, size_t bytes) {
    if (bytes == 0) return SVS_OK;
    SVS_HIP(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, st));
    return SVS_OK;
}

// the DOWN stream may start on what the UP stream has enqueued so far
int stage_handoff(HostStage &c) {
    hipEvent_t e = c.chunk_done[c.next_event++ % kChunkEvents];
    SVS_HIP(hipEventRecord(e, c.st[0]));
    SVS_HIP(hipStreamWaitEvent(c.st[1], e, 0));
    return SVS_OK;
}

// Runs body(context) on the calling thread's context, with the buffers the call uses reserved first (0 bytes: not used).
// Both streams are drained before it returns, on the error path too: a call that fails half way must not leave a DMA in
// flight into the caller's buffers.
template <class Body>
int staged(size_t frames, size_t second, size_t third, size_t bits, Body &&body) {
    HostStage *ctx = nullptr;
    if (int rc = stage_acquire(&ctx)) return rc;
    HostStage &c = *ctx;
    int rc = SVS_OK;
    const size_t want[4] = {frames, second, third, bits};
    Grow *const buf[4] = {&c.frames, &c.second, &c.third, &c.bits};
    for (int i = 0; i < 4 && !rc; ++i)
        if (want[i]) rc = stage_reserve(*buf[i], want[i]);
    if (!rc) rc = body(c);
    for (auto &s : c.st)
        if (s && hipStreamSynchronize(s) != hipSuccess && !rc)
            rc = fail(SVS_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(hipGetLastError()));
    return rc;
}

// svs_stage.hpp's rule; the experiments library's SVS_STAGE_CHUNK_KB overrides it
size_t stage_chunk_bytes(uint64_t total) {
    const uint32_t forced = knob("SVS_STAGE_CHUNK_KB", 0);
    return forced ? (size_t)forced << 10 : svs::stage_chunk_rule(total);
}

// The payload of a host-pointer embed call: packed MSB-first bits indexed by bit_offset, or `use` '0' / '1' characters
// (ascii, bit_offset 0) that are uploaded as they are and packed on the device.  Of a packed payload only the bytes the call
// reads go to the device - [first_byte, first_byte + bytes), first_byte dword aligned, the bit offset rebased onto it (a frame
// loop that indexes one long stream by bit_offset stays O(batch) per call).
struct HostPayload {
    const uint8_t *packed;
    const char *ascii;
    uint64_t bit_offset, use;

    uint64_t first_byte() const { return use ? (bit_offset / 32) * 4 : 0; }
    uint64_t packed_bytes() const { return use ? (bit_offset + use + 7) / 8 - first_byte() : 0; }
    uint64_t words() const { return (use + 31) / 32; }
    size_t bits_bytes() const { return ascii ? 4 * words() + 8 : ((packed_bytes() + 3) / 4) * 4 + 4; }   // c.bits
    size_t ascii_bytes() const { return ascii && use ? use + 32 : 0; }                                    // c.third

    // queued on the UP stream, ahead of the kernels that read it -> the bit offset into c.bits
    int stage(HostStage &c, uint64_t *rebased) const {
        const hipStream_t up = c.st[0];
        uint8_t *d = static_cast<uint8_t *>(c.bits.p);
        const size_t alloc = bits_bytes();
        *rebased = 0;
        if (ascii) {
            SVS_HIP(hipMemsetAsync(d + 4 * words(), 0, 8, up));
            if (use == 0) return SVS_OK;
            if (int rc = stage_h2d(up, c.third.p, ascii, use)) return rc;
            const uint32_t blocks = (uint32_t)((words() + 255) / 256 < 2048 ? (words() + 255) / 256 : 2048);
            hipLaunchKernelGGL(svs::ascii_to_packed_kernel, dim3(blocks), dim3(256), 0, up, static_cast<const uint8_t *>(c.third.p),
                               use, reinterpret_cast<uint32_t *>(d), words());
            SVS_HIP(hipGetLastError());
            return SVS_OK;
        }
        *rebased = bit_offset - 8 * first_byte();
        if (packed_bytes() == 0) {
            SVS_HIP(hipMemsetAsync(d, 0, alloc, up));
            return SVS_OK;
        }
        // the kernels read whole dwords: the tail behind the last payload byte must be defined (zero)
        SVS_HIP(hipMemsetAsync(d + (alloc - 8), 0, 8, up));
        return stage_h2d(up, d, packed + first_byte(), packed_bytes());
    }
};

// The chunk pipeline of the host-pointer embed calls.  The frames (bpp bytes per pixel; the planes' pitches count pixels) go
// from `src` to the same offsets of c.frames chunk by chunk: upload and embed(sub, off, f0, bit_offset, budget, &done, up) on
// the UP stream, then download(chunk, off, down) behind the chunk's event on the DOWN stream.  A batch of one chunk runs in
// order on one stream - no event, no second stream.  `off` is the chunk's first byte, f0 its first frame; `rebased` the
// payload's first bit in c.bits.  whole_frames: no chunk cuts a frame into bands (a keyed order spreads a frame's payload
// over all its blocks).
template <class Embed, class Download>
int embed_chunks(HostStage &c, const svs_planes *p, int bpp, const uint8_t *src, uint32_t n, uint64_t use, uint64_t n_bits,
                 uint64_t rebased, Embed &&embed, Download &&download, uint64_t *done_total, bool whole_frames = false) {
    const int32_t H = p->height, W = p->width;
    const int64_t rp = bpp * p->row_pitch, fp = bpp * p->frame_pitch, row_bytes = (int64_t)bpp * W;
    const uint64_t wb = (uint64_t)W / 8, bpf = wb * ((uint64_t)H / 8);
    // a non-empty payload that cannot be embedded (delta <= 0, n_ac = 0) must still reach the kernel as "non-empty": every
    // block is then round-tripped, as in the reference
    const uint64_t pass_bits = use ? use : (n_bits ? 1 : 0);
    size_t target = stage_chunk_bytes(bpp * span_bytes(p));
    if (whole_frames && target < (size_t)H * rp) target = (size_t)H * rp;
    uint32_t n_chunks = 0;
    svs::for_each_chunk(p->n_frames, H, (size_t)rp, target, [&](const svs::Chunk &) { ++n_chunks; });
    const bool serial = n_chunks <= 1;
    const hipStream_t up = c.st[0], down = serial ? c.st[0] : c.st[1];
    uint8_t *d = static_cast<uint8_t *>(c.frames.p);
    int rc = SVS_OK;
    *done_total = 0;
    svs::for_each_chunk(p->n_frames, H, (size_t)rp, target, [&](const svs::Chunk &ch) {
        if (rc) return;
        const int64_t off = (int64_t)ch.f0 * fp + (int64_t)ch.r0 * rp;
        const size_t bytes = ch.nf == 1 ? (size_t)(ch.rows - 1) * rp + row_bytes : (size_t)(ch.nf - 1) * fp + (size_t)(H - 1) * rp + row_bytes;
        if ((rc = stage_h2d(up, d + off, src + off, bytes))) return;
        const svs_planes sub{ch.nf, ch.rows, W, 0, p->row_pitch, ch.nf == 1 ? ch.rows * p->row_pitch : p->frame_pitch};
        const uint64_t g0 = (uint64_t)ch.f0 * bpf + (uint64_t)(ch.r0 / 8) * wb;
        uint64_t done = 0;
        if ((rc = embed(sub, off, ch.f0, rebased + (use ? g0 * n : 0), svs::chunk_budget(pass_bits, use, g0, n), &done, up))) return;
        *done_total += done;
        if (!serial && (rc = stage_handoff(c))) return;
        rc = download(ch, off, down);
    });
    return rc;
}

// The staging of the host-pointer extract calls: `in_bytes` of `src` up, then device(d_in, d_bits, bits capacity, &n_bits, st)
// and download(context, st).  The download is n_ac / 512 of the upload: nothing to overlap - one stream, one copy, one kernel
// over the batch.  `third`: bytes of c.third the download uses.
template <class Device, class Download>
int extract_staged(const void *src, size_t in_bytes, uint64_t bytes, size_t third, uint64_t *n_bits_out, Device &&device,
                   Download &&download) {
    uint64_t got = 0;
    if (int rc = staged(in_bytes, 0, third, bytes + 8, [&](HostStage &c) {
            const hipStream_t st = c.st[0];
            if (int rc = stage_h2d(st, c.frames.p, src, in_bytes)) return rc;
            if (int rc = device(static_cast<const uint8_t *>(c.frames.p), static_cast<uint8_t *>(c.bits.p), bytes + 8, &got, st))
                return rc;
            return download(c, st);
        }))
        return rc;
    if (n_bits_out) *n_bits_out = got;
    return SVS_OK;
}

}  // namespace

extern "C" {

int svs_abi_version(void) { return SVS_ABI_VERSION; }

const char *svs_last_error(void) { return g_last_error.c_str(); }

int svs_device_count(int *count) {
    if (!count) return fail(SVS_ERR_INVALID_ARG, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(SVS_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return SVS_OK;
}

int svs_init(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(SVS_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n) return fail(SVS_ERR_INVALID_ARG, "device %d out of range (0..%d)", device, n - 1);
    SVS_HIP(hipSetDevice(device));
    SVS_HIP(hipFree(nullptr));  // force context creation so later failures are not init failures
    return SVS_OK;
}

int svs_device_arch(int device, char *buf, size_t buf_len) {
    if (!buf || buf_len == 0) return fail(SVS_ERR_INVALID_ARG, "buf is NULL/empty");
    hipDeviceProp_t prop;
    SVS_HIP(hipGetDeviceProperties(&prop, device));
    snprintf(buf, buf_len, "%s", prop.gcnArchName);
    return SVS_OK;
}

int svs_malloc(void **dev_ptr, size_t bytes) {
    if (!dev_ptr) return fail(SVS_ERR_INVALID_ARG, "dev_ptr is NULL");
    *dev_ptr = nullptr;
    SVS_HIP(hipMalloc(dev_ptr, bytes ? bytes : 4));
    return SVS_OK;
}

int svs_free(void *dev_ptr) {
    SVS_HIP(hipFree(dev_ptr));
    return SVS_OK;
}

int svs_memcpy_h2d(void *dev_dst, const void *host_src, size_t bytes, void *stream) {
    if (bytes == 0) return SVS_OK;
    SVS_HIP(hipMemcpyAsync(dev_dst, host_src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return SVS_OK;
}

int svs_memcpy_d2h(void *host_dst, const void *dev_src, size_t bytes, void *stream) {
    if (bytes == 0) return SVS_OK;
    SVS_HIP(hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return SVS_OK;
}

int svs_memset(void *dev_dst, int value, size_t bytes, void *stream) {
    if (bytes == 0) return SVS_OK;
    SVS_HIP(hipMemsetAsync(dev_dst, value, bytes, (hipStream_t)stream));
    return SVS_OK;
}

int svs_stream_synchronize(void *stream) {
    SVS_HIP(hipStreamSynchronize((hipStream_t)stream));
    return SVS_OK;
}

int svs_stream_create(void **stream) {
    if (!stream) return fail(SVS_ERR_INVALID_ARG, "stream is NULL");
    hipStream_t st = nullptr;
    SVS_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    *stream = st;
    return SVS_OK;
}

int svs_stream_destroy(void *stream) {
    SVS_HIP(hipStreamDestroy((hipStream_t)stream));
    return SVS_OK;
}

int svs_host_alloc(void **host_ptr, size_t bytes) {
    if (!host_ptr) return fail(SVS_ERR_INVALID_ARG, "host_ptr is NULL");
    *host_ptr = nullptr;
    SVS_HIP(hipHostMalloc(host_ptr, bytes ? bytes : 4, hipHostMallocDefault));
    return SVS_OK;
}

int svs_host_free(void *host_ptr) {
    SVS_HIP(hipHostFree(host_ptr));
    return SVS_OK;
}

uint64_t svs_capacity_bits(const svs_planes *p, int n_ac) {
    if (!p || p->n_frames <= 0 || p->height <= 0 || p->width <= 0) return 0;
    return (uint64_t)p->n_frames * (uint64_t)(p->height / 8) * (uint64_t)(p->width / 8) * (uint64_t)clamp_ac(n_ac);
}

uint64_t svs_packed_bytes(uint64_t n_bits) { return (n_bits + 7) / 8; }

}  // extern "C"

namespace {

// What an extract call writes.  BITS: the packed bits.  SOFT: one byte per capacity bit.  VOTE: the bytes' votes, added into
// a tally of `period` int32 at (stream_bit0 + the bit's index) mod period.  HIST: the bytes counted into 256 uint32 a frame.
// Everything in which the four kinds differ hangs on this value (extract_checks, extract_dev, extract_host).
struct ExtractOutput {
    enum Kind { BITS, SOFT, VOTE, HIST } kind = BITS;
    uint64_t period = 0, stream_bit0 = 0;   // VOTE

    // a tally or a histogram: the device form adds into the caller's buffer, the host form zeroes its own first (and the caller's
    // on an empty call); no capacity argument; delta <= 0 is refused; a refusal leaves *n_bits_out alone
    bool adds() const { return kind == VOTE || kind == HIST; }
    const char *call() const { return kind == VOTE ? "vote" : "histogram"; }                       // adds() only
    const char *noun() const { return kind == VOTE ? "tally" : kind == HIST ? "hist" : "bits"; }   // in the messages
    uint64_t bytes(uint64_t cap, int32_t n_frames) const {
        return kind == BITS ? (cap + 7) / 8 : kind == SOFT ? cap : kind == VOTE ? 4u * period : 4ull * svs::kHistBins * (uint64_t)n_frames;
    }
};

// What a gray call adds to the plain call (svs_embed_dev / svs_extract_dev); every member is optional.  The public entry points
// fill one - those with a selection or a dither through with_options - and the internal functions below take it.
struct GrayOptions {
    const svs_block_order *order = nullptr;    // the ordered calls: a keyed block order
    const svs::CoeffTable *coeffs = nullptr;   // the select calls: the table of a selection that is not the prefix 1..n_ac
    const svs_dither *dither = nullptr;        // the dithered calls
    uint64_t *d_counts = nullptr;              // the read-back calls, device: {repaired, unrepaired}, added to
    svs_readback_counts *counts = nullptr;     // the read-back calls, host: the counts of the whole call
    ExtractOutput out;                         // the extract calls: what the call writes (the soft calls: not the packed bits)
    const svs::StepArgs *steps = nullptr;      // the stepped calls: the checked table in the kernels' form
    uint32_t min_margin = 0;                   // the margin calls: the gate of the pass behind the stepped read-back (0: none);
                                               // d_counts is then four uint64, svs_margin_counts
    svs_margin_counts *margin_counts = nullptr;   // the margin calls, host: the counts of the whole call (in the place of `counts`)
    uint32_t matrix = 0;                       // the matrix calls: svs_route.hpp's matrix word; the call's n_ac is then k

    // the kernels' forms, for a batch of g's blocks per frame (derived once per call)
    svs::KernelOptions kernel_forms(const svs::Geometry &g) const {
        return {order ? svs::make_block_order(order->key, order->first_frame, g.by_bpf.div) : svs::BlockOrderArgs{}, coeffs,
                dither ? svs::DitherArgs{svs::dither_seed(dither->key), dither->first_frame, 1u, svs::CoeffTable{}} : svs::DitherArgs{},
                out.period, out.stream_bit0, steps ? *steps : svs::StepArgs{}};
    }

    // the routing arguments of the call (the one place that fills them from the options)
    svs::RouteArgs route(double delta, const svs::Geometry &g, uint64_t total, uint64_t n_bits, uint64_t bit_offset, uint32_t flags) const {
        svs::RouteArgs ra = route_args(delta, g, total, n_bits, bit_offset, flags, false);
        ra.keyed = order != nullptr;
        ra.readback = (flags & SVS_READBACK) != 0;   // an embed flag: the extract calls have refused it
        ra.coeffs = coeffs;                          // the select calls: n_ac == coeffs->count
        ra.dithered = dither != nullptr;
        ra.soft = out.kind == ExtractOutput::SOFT;
        ra.vote = out.kind == ExtractOutput::VOTE;
        ra.hist = out.kind == ExtractOutput::HIST;
        ra.stepped = steps != nullptr;
        ra.min_margin = min_margin;
        ra.matrix = matrix;
        return ra;
    }

    // The options of a staging chunk of whole frames that starts at frame f0 of the call: its first frame is clip frame
    // first_frame + f0 for the order and the dither alike (rebased into *o and *d), and its counts are added to `chunk_counts`.
    GrayOptions chunk(uint32_t f0, uint64_t *chunk_counts, svs_block_order *o, svs_dither *d) const {
        GrayOptions c = *this;
        if (order) c.order = &(*o = svs_block_order{order->key, order->first_frame + f0, 0u});
        if (dither) c.dither = &(*d = svs_dither{dither->key, dither->first_frame + f0, 0u});
        c.d_counts = chunk_counts;
        c.counts = nullptr;
        c.margin_counts = nullptr;
        return c;
    }
};

// the order argument of the ordered entry points: NULL (no order) or a valid one
int check_order(const svs_block_order *order) {
    if (order && order->reserved != 0) return fail(SVS_ERR_INVALID_ARG, "svs_block_order.reserved must be 0");
    return SVS_OK;
}

// the dither argument of the dithered entry points; its first_frame must be the order's when both are given (a caller must
// not desynchronise them silently)
int check_dither(const svs_dither *dither, const svs_block_order *order) {
    if (!dither) return fail(SVS_ERR_INVALID_ARG, "dither is NULL");
    if (dither->reserved != 0) return fail(SVS_ERR_INVALID_ARG, "svs_dither.reserved must be 0");
    if (order && order->first_frame != dither->first_frame)
        return fail(SVS_ERR_INVALID_ARG, "svs_dither.first_frame %u differs from svs_block_order.first_frame %u",
                    (unsigned)dither->first_frame, (unsigned)order->first_frame);
    return SVS_OK;
}

// The selection of the select entry points -> the kernels' table.  *coeffs = NULL when the selection is the prefix 1..count:
// the call is then the one without a selection at n_ac = count, streaming kernels included.
int check_coeffs(const svs_coeffs *c, svs::CoeffTable *table, const svs::CoeffTable **coeffs) {
    if (!c) return fail(SVS_ERR_INVALID_ARG, "coeffs is NULL");
    if (c->count > 63) return fail(SVS_ERR_INVALID_ARG, "svs_coeffs.count %u exceeds 63", (unsigned)c->count);
    for (int i = c->count; i < 63; ++i)
        if (c->index[i] != 0) return fail(SVS_ERR_INVALID_ARG, "svs_coeffs.index[%d] behind count must be 0", i);
    if (!svs::make_coeff_table(c->index, c->count, table))
        return fail(SVS_ERR_INVALID_ARG, "svs_coeffs.index must hold distinct flat indices in 1..63 (DC is never selectable)");
    *coeffs = svs::coeff_table_is_prefix(*table) ? nullptr : table;
    return SVS_OK;
}

constexpr uint32_t kModeFlags = SVS_EXACT_POCKETFFT | SVS_EXACT_GUARDED;
constexpr uint32_t kSelectEmbedFlags = kModeFlags | SVS_NEAREST | SVS_MINMOVE;
constexpr uint32_t kGrayEmbedFlags = kSelectEmbedFlags | SVS_READBACK;

// What an entry point with a selection or a dither checks before anything else: a NULL dither or selection is refused where
// the policy requires one and means "none" elsewhere; flags outside `allowed` are refused with `what`.
struct OptionsPolicy {
    bool dither_required, coeffs_required;
    uint32_t allowed;
    const char *what;
};
constexpr OptionsPolicy kSelectEmbed{false, true, kSelectEmbedFlags, "a select embed takes the mode bits, SVS_NEAREST and SVS_MINMOVE"};
constexpr OptionsPolicy kSelectExtract{false, true, kModeFlags, "a select extract takes the mode bits only"};
constexpr OptionsPolicy kDitheredEmbed{true, false, kSelectEmbedFlags, "a dithered embed takes the mode bits, SVS_NEAREST and SVS_MINMOVE"};
constexpr OptionsPolicy kDitheredExtract{true, false, kModeFlags, "a dithered extract takes the mode bits only"};
// order, coeffs and dither may each be NULL
constexpr OptionsPolicy kSoftExtract{false, false, kModeFlags, "a soft extract takes the mode bits only"};
constexpr OptionsPolicy kSoftVote{false, false, kModeFlags, "a soft vote takes the mode bits only"};
constexpr OptionsPolicy kSoftHistogram{false, false, kModeFlags, "a soft histogram takes the mode bits only"};
// order, coeffs and dither may each be NULL: a NULL dither is the selected call with read-back, all three NULL (or a prefix
// selection alone) svs_embed_readback* itself; SVS_READBACK is accepted and implied
constexpr OptionsPolicy kKeyedReadback{false, false, kGrayEmbedFlags,
                                       "a dithered read-back embed takes the mode bits, SVS_NEAREST, SVS_MINMOVE and SVS_READBACK"};

// Such an entry point: its public arguments are checked in this order - the dither, the selection, the flags - and then
// call(n_ac, options) runs.  With a selection n_ac is ignored and the selection's count rules (options.coeffs stays NULL for a
// prefix selection: the call without one at n_ac = count).
template <class Call>
int with_options(const OptionsPolicy &pol, const svs_block_order *order, const svs_coeffs *coeffs, const svs_dither *dither,
                 uint32_t flags, int n_ac, Call &&call) {
    svs::CoeffTable table;
    GrayOptions o{order, nullptr, dither};
    if (dither || pol.dither_required)
        if (int rc = check_dither(dither, order)) return rc;
    if (coeffs || pol.coeffs_required) {
        if (int rc = check_coeffs(coeffs, &table, &o.coeffs)) return rc;
        n_ac = coeffs->count;
    }
    if (flags & ~pol.allowed) return fail(SVS_ERR_INVALID_ARG, "flags 0x%x: %s", flags, pol.what);
    return call(n_ac, o);
}

// The stepped calls are the dithered calls with each of order, coeffs and dither optional and the table in place of delta: the
// table is checked first, then what with_options checks, then the call runs as every gray call does - with a positive delta
// that routes it and that no kernel reads (svs_route.hpp RouteArgs::stepped).
constexpr OptionsPolicy kSteppedEmbed{false, false, kSelectEmbedFlags, "a stepped embed takes the mode bits, SVS_NEAREST and SVS_MINMOVE"};
constexpr OptionsPolicy kSteppedExtract{false, false, kModeFlags, "a stepped extract takes the mode bits only"};
// the stepped embed with read-back: SVS_READBACK is accepted and implied (svs_stepped_embed* itself keeps refusing it)
constexpr OptionsPolicy kSteppedReadback{false, false, kGrayEmbedFlags,
                                         "a stepped read-back embed takes the mode bits, SVS_NEAREST, SVS_MINMOVE and SVS_READBACK"};
constexpr double kSteppedRouteDelta = 1.0;

// min_margin: the gate of the margin calls (svs_stepped_embed_readback_margin*), checked behind the table and ahead of the rest
template <class Call>
int with_steps(const OptionsPolicy &pol, const svs_block_order *order, const svs_coeffs *coeffs, const svs_dither *dither,
                      const svs_qim_steps *steps, uint32_t flags, int n_ac, Call &&call, uint32_t min_margin = 0) {
    if (!steps) return fail(SVS_ERR_INVALID_ARG, "steps is NULL");
    for (int k = 1; k < 64; ++k)
        if (steps->delta[k] < 1 || steps->delta[k] > 4095)
            return fail(SVS_ERR_INVALID_ARG, "delta[%d] = %u is not in 1..4095", k, (unsigned)steps->delta[k]);
    if (min_margin > 127) return fail(SVS_ERR_INVALID_ARG, "min_margin %u exceeds 127, the largest soft margin", (unsigned)min_margin);
    const svs::StepArgs table = svs::make_step_args(steps->delta);
    return with_options(pol, order, coeffs, dither, flags, n_ac, [&](int n, GrayOptions o) {
        o.steps = &table;
        o.min_margin = min_margin;
        return call(n, o);
    });
}

// The matrix calls are the stepped calls with k stream bits a block: the matrix struct is checked first, then what with_steps
// checks, then the size of the selection (or n_ac) against 2^k - 1; the call then runs as a stepped call at n_ac = k whose table
// has 2^k - 1 slots (svs_route.hpp RouteArgs::matrix).  The pair search keeps 2 (2^k - 1) floats per lane in LDS: k <= 5.
constexpr OptionsPolicy kMatrixEmbed{false, false, kSelectEmbedFlags, "a matrix embed takes the mode bits, SVS_NEAREST and SVS_MINMOVE"};
constexpr OptionsPolicy kMatrixExtract{false, false, kModeFlags, "a matrix extract takes the mode bits only"};

int check_matrix(const svs_matrix *m) {
    if (!m) return fail(SVS_ERR_INVALID_ARG, "matrix is NULL");
    if (m->k < 1 || m->k > 6) return fail(SVS_ERR_INVALID_ARG, "svs_matrix.k %u is not in 1..6", (unsigned)m->k);
    if (m->search > 1) return fail(SVS_ERR_INVALID_ARG, "svs_matrix.search %u is not 0 or 1", (unsigned)m->search);
    if (m->reserved[0] != 0 || m->reserved[1] != 0) return fail(SVS_ERR_INVALID_ARG, "svs_matrix.reserved must be 0");
    if (m->search == 1 && m->k > 5)
        return fail(SVS_ERR_INVALID_ARG, "svs_matrix.search 1 takes k <= 5 (the pair search's tile of 2 * 63 floats a lane exceeds a launch's LDS)");
    return SVS_OK;
}

template <class Call>
int with_matrix(const OptionsPolicy &pol, const svs_block_order *order, const svs_coeffs *coeffs, const svs_dither *dither,
                const svs_qim_steps *steps, const svs_matrix *matrix, uint32_t flags, int n_ac, Call &&call) {
    if (int rc = check_matrix(matrix)) return rc;
    return with_steps(pol, order, coeffs, dither, steps, flags, n_ac, [&](int n, GrayOptions o) {
        const int slots = (1 << matrix->k) - 1;
        if (n != slots)
            return fail(SVS_ERR_INVALID_ARG, "a matrix call with k = %u takes a selection (or n_ac) of exactly %d coefficients, not %d",
                        (unsigned)matrix->k, slots, n);
        o.matrix = svs::make_matrix_word(matrix->k, matrix->search);
        return call((int)matrix->k, o);
    });
}

int check_extract_flags(uint32_t flags) {
    if (flags & (SVS_READBACK | SVS_NEAREST | SVS_MINMOVE))
        return fail(SVS_ERR_INVALID_ARG, "SVS_READBACK, SVS_NEAREST and SVS_MINMOVE are embed flags");
    return SVS_OK;
}

// every gray device embed call: `o` says what it adds to svs_embed_dev
int embed_dev(const uint8_t *d_gray, uint8_t *d_stego, const svs_planes *planes, double delta, int n_ac,
              const uint8_t *d_bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t flags, uint64_t *n_embedded,
              void *stream, const GrayOptions &o) {
    svs::Geometry g;
    uint64_t total = 0;
    if (int rc = make_geometry(planes, n_ac, &g, &total)) return rc;
    if (n_embedded) *n_embedded = 0;
    if (int rc = check_order(o.order)) return rc;
    if (total == 0) return SVS_OK;
    if (!d_gray || !d_stego) return fail(SVS_ERR_INVALID_ARG, "gray/stego pointer is NULL");
    if (((uintptr_t)d_gray % 8) || ((uintptr_t)d_stego % 8))
        return fail(SVS_ERR_INVALID_ARG, "plane pointers must be 8-byte aligned");
    const svs::EmbedPlan p = svs::plan_embed(o.route(delta, g, total, n_bits, bit_offset, flags));
    if (p.use > 0) {
        if (!d_bits_packed) return fail(SVS_ERR_INVALID_ARG, "bits pointer is NULL");
        if ((uintptr_t)d_bits_packed % 4) return fail(SVS_ERR_INVALID_ARG, "bits pointer must be 4-byte aligned");
        if (bit_offset + p.use < bit_offset) return fail(SVS_ERR_INVALID_ARG, "bit_offset + n_bits overflows");
    }
    if (flags & ~kGrayEmbedFlags) return fail(SVS_ERR_INVALID_ARG, "unknown flags 0x%x", flags);
    if (o.d_counts && ((uintptr_t)o.d_counts % 8)) return fail(SVS_ERR_INVALID_ARG, "counts pointer must be 8-byte aligned");
    if (p.n_words >= (1ull << 32)) return fail(SVS_ERR_INVALID_ARG, "payload too large for one call");
    if (p.path == EmbedPath::COPY && d_gray == d_stego) return SVS_OK;
    const bool two = p.two_blocks && rows_allow_two_blocks(planes, d_gray, d_stego);
    const uint32_t *bits = p.use ? reinterpret_cast<const uint32_t *>(d_bits_packed) : nullptr;
    const svs::KernelOptions k = o.kernel_forms(g);
    if (int rc = launch_embed(p, two, total, (hipStream_t)stream, d_gray, d_stego, g, bits, k)) return rc;
    if (p.readback && p.use > 0)
        if (int rc = launch_readback(p, total, (hipStream_t)stream, d_stego, g, bits, o.d_counts, k, svs::ColourParams{}, SVS_RB_GRAY))
            return rc;
    if (p.min_margin > 0) {   // the margin pass: the stepped form once more, on the bytes the read-back left, with the gate
        svs::KernelOptions km = k;
        km.steps = svs::margin_steps(k.steps, p.min_margin);
        if (int rc = launch_readback(p, total, (hipStream_t)stream, d_stego, g, bits, o.d_counts, km, svs::ColourParams{}, SVS_RB_GRAY))
            return rc;
    }
    if (n_embedded) *n_embedded = p.use;
    return SVS_OK;
}

// What every gray extract call checks before any device work, in this order, for the output `o.out` describes; the host forms
// (device = false) leave the alignment to their staged buffers.  -> *bytes of output; *cap = 0: an empty call, whose pointers and
// bounds were not looked at.  A tally or a histogram: nothing is written before the last check has passed.
int extract_checks(const void *gray, const void *out, bool device, const svs_planes *planes, double delta, int n_ac,
                   uint64_t out_capacity_bytes, uint32_t flags, uint64_t *n_bits_out, const GrayOptions &o, svs::Geometry *g,
                   uint64_t *total, uint64_t *cap, uint64_t *bytes) {
    const ExtractOutput &w = o.out;
    if (w.adds()) n_bits_out = nullptr;
    if (int rc = extract_geometry(planes, n_ac, g, total, cap, n_bits_out)) return rc;
    if (int rc = check_order(o.order)) return rc;
    if (int rc = check_extract_flags(flags)) return rc;
    if (w.kind == ExtractOutput::VOTE) {
        if (w.period == 0) return fail(SVS_ERR_INVALID_ARG, "period is 0");
        if (w.period > svs::kVotePeriodMax) return fail(SVS_ERR_INVALID_ARG, "period %llu exceeds 2^61 - 1", (unsigned long long)w.period);
    }
    if (w.adds() && !(delta > 0.0))
        return fail(SVS_ERR_INVALID_ARG, "a %s needs delta > 0 (every soft byte is 0 otherwise)", w.call());
    *bytes = w.bytes(*cap, planes->n_frames);
    if (*cap == 0) return SVS_OK;
    if (!gray || !out) return fail(SVS_ERR_INVALID_ARG, "gray/%s pointer is NULL", w.noun());
    if (device && ((uintptr_t)gray % 8)) return fail(SVS_ERR_INVALID_ARG, "plane pointer must be 8-byte aligned");
    if (device && ((uintptr_t)out % 4)) return fail(SVS_ERR_INVALID_ARG, "%s pointer must be 4-byte aligned", w.noun());
    if (!w.adds()) return check_capacity(*bytes, out_capacity_bytes, "bytes");
    // no capacity argument: the caller sized the output by the call's own arguments; what is bounded is one entry's growth
    if (w.kind == ExtractOutput::VOTE && w.period < (1ull << (64 - svs::kVoteCopiesShift)) && *cap > (w.period << svs::kVoteCopiesShift))
        return fail(SVS_ERR_INVALID_ARG, "capacity %llu exceeds period * 2^22: an int32 tally entry could overflow in one call",
                    (unsigned long long)*cap);
    const uint64_t per_frame = (uint64_t)g->by_bpf.div * g->n_ac;
    if (w.kind == ExtractOutput::HIST && per_frame > 0xFFFFFFFFull)
        return fail(SVS_ERR_INVALID_ARG, "planes hold %llu bytes a frame, above 2^32 - 1: a uint32 hist entry could wrap in one call",
                    (unsigned long long)per_frame);
    return SVS_OK;
}

// every gray device extract call; d_out: the packed bits, the soft bytes, the tally or the counts (ExtractOutput)
int extract_dev(const uint8_t *d_gray, const svs_planes *planes, double delta, int n_ac, uint8_t *d_out, uint64_t out_capacity_bytes,
                uint32_t flags, uint64_t *n_bits_out, void *stream, const GrayOptions &o) {
    svs::Geometry g;
    uint64_t total = 0, cap = 0, bytes = 0;
    if (int rc = extract_checks(d_gray, d_out, true, planes, delta, n_ac, out_capacity_bytes, flags, n_bits_out, o, &g, &total, &cap, &bytes))
        return rc;
    if (cap != 0) {
        const svs::ExtractPlan p = svs::plan_extract(o.route(delta, g, total, 0, 0, flags));
        // the flags are checked only when there is something to extract: delta <= 0 gives zeros whatever they say
        if (p.path != ExtractPath::ZEROS && (flags & ~kModeFlags)) return fail(SVS_ERR_INVALID_ARG, "unknown flags 0x%x", flags);
        if (int rc = launch_extract(p, total, (hipStream_t)stream, d_gray, g, d_out, bytes, o.kernel_forms(g))) return rc;
    }
    if (n_bits_out) *n_bits_out = cap;
    return SVS_OK;
}

}  // namespace

extern "C" {

int svs_embed_dev(const uint8_t *d_gray, uint8_t *d_stego, const svs_planes *planes, double delta, int n_ac,
                  const uint8_t *d_bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t flags,
                  uint64_t *n_embedded, void *stream) {
    return embed_dev(d_gray, d_stego, planes, delta, n_ac, d_bits_packed, bit_offset, n_bits, flags, n_embedded, stream, GrayOptions{});
}

int svs_embed_ordered_dev(const uint8_t *d_gray, uint8_t *d_stego, const svs_planes *planes, const svs_block_order *order,
                          double delta, int n_ac, const uint8_t *d_bits_packed, uint64_t bit_offset, uint64_t n_bits,
                          uint32_t flags, uint64_t *n_embedded, void *stream) {
    return embed_dev(d_gray, d_stego, planes, delta, n_ac, d_bits_packed, bit_offset, n_bits, flags, n_embedded, stream, GrayOptions{order});
}

int svs_extract_dev(const uint8_t *d_gray, const svs_planes *planes, double delta, int n_ac,
                    uint8_t *d_bits_packed_out, uint64_t out_capacity_bytes, uint32_t flags, uint64_t *n_bits_out,
                    void *stream) {
    return extract_dev(d_gray, planes, delta, n_ac, d_bits_packed_out, out_capacity_bytes, flags, n_bits_out, stream, GrayOptions{});
}

int svs_extract_ordered_dev(const uint8_t *d_gray, const svs_planes *planes, const svs_block_order *order, double delta,
                            int n_ac, uint8_t *d_bits_packed_out, uint64_t out_capacity_bytes, uint32_t flags,
                            uint64_t *n_bits_out, void *stream) {
    return extract_dev(d_gray, planes, delta, n_ac, d_bits_packed_out, out_capacity_bytes, flags, n_bits_out, stream, GrayOptions{order});
}

static bool ranges_overlap(const void *a, const void *b, uint64_t span) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + span && y < x + span;
}

// the operator's first return value - the gray frames before embedding as arrays of their own (config_and_setup.py:113-114,172)
static void copy_gray_reference(uint8_t *dst, const uint8_t *gray, const svs_planes *planes, bool frames_packed, uint64_t span) {
    if (frames_packed) {
        memcpy(dst, gray, span);
        return;
    }
    for (int32_t f = 0; f < planes->n_frames; ++f)
        for (int32_t y = 0; y < planes->height; ++y)
            memcpy(dst + (int64_t)f * planes->frame_pitch + (int64_t)y * planes->row_pitch,
                   gray + (int64_t)f * planes->frame_pitch + (int64_t)y * planes->row_pitch, (size_t)planes->width);
}

// A staged chunk of gray planes back to the caller (`d`: the staging buffer, same offsets): pixel bytes only - padding in the
// caller's output buffer is left alone
static int download_pixels(uint8_t *dst, const uint8_t *d, const svs_planes *planes, const svs::Chunk &ch, int64_t off, hipStream_t st) {
    const int32_t H = planes->height, W = planes->width;
    const int64_t rp = planes->row_pitch, fp = planes->frame_pitch;
    const bool rows_packed = rp == W, frames_packed = rows_packed && fp == (int64_t)H * W;
    if (frames_packed || (rows_packed && ch.nf == 1))
        return stage_d2h(st, dst + off, d + off, ch.nf == 1 ? (size_t)ch.rows * W : (size_t)ch.nf * H * W);
    for (int32_t f = 0; f < ch.nf; ++f) {
        const int64_t o = off + (int64_t)f * fp;
        if (rows_packed) {
            if (int rc = stage_d2h(st, dst + o, d + o, (size_t)ch.rows * W)) return rc;
        } else if (hipMemcpy2DAsync(dst + o, (size_t)rp, d + o, (size_t)rp, (size_t)W, (size_t)ch.rows, hipMemcpyDeviceToHost, st) !=
                   hipSuccess) {
            return fail(SVS_ERR_HIP, "hipMemcpy2DAsync failed: %s", hipGetErrorString(hipGetLastError()));
        }
    }
    return SVS_OK;
}

// svs_embed (payload = packed MSB-first bits, indexed by bit_offset) and svs_embed_str (payload = n_bits '0' / '1' characters,
// bit_offset = 0) share everything but the way the payload reaches the device
// (`o`: what the call adds to svs_embed, with a packed payload; o.counts receives the read-back counts)
static int embed_host(const uint8_t *gray, uint8_t *stego, uint8_t *gray_ref_out, const svs_planes *planes, double delta, int n_ac,
                      const uint8_t *bits_packed, const char *bits_ascii, uint64_t bit_offset, uint64_t n_bits, uint32_t flags,
                      uint64_t *n_embedded, const GrayOptions &o) {
    svs::Geometry g;
    uint64_t total = 0;
    svs_readback_counts *const counts = o.counts;
    svs_margin_counts *const margin = o.margin_counts;   // a margin call: four counts in the place of two
    if (int rc = make_geometry(planes, n_ac, &g, &total)) return rc;
    if (n_embedded) *n_embedded = 0;
    if (counts) *counts = svs_readback_counts{0, 0};
    if (margin) *margin = svs_margin_counts{0, 0, 0, 0};
    if (int rc = check_order(o.order)) return rc;
    if (total == 0) return SVS_OK;
    if (!gray || !stego) return fail(SVS_ERR_INVALID_ARG, "gray/stego pointer is NULL");
    if (flags & ~kGrayEmbedFlags) return fail(SVS_ERR_INVALID_ARG, "unknown flags 0x%x", flags);
    const uint64_t span = span_bytes(planes);
    const uint64_t cap = total * (uint64_t)g.n_ac;
    uint64_t use = n_bits < cap ? n_bits : cap;
    if (!(delta > 0.0)) use = 0;                   // nothing can be embedded (config_and_setup.py:143-145)
    if (use && !bits_packed && !bits_ascii) return fail(SVS_ERR_INVALID_ARG, "bits pointer is NULL");
    if (use && bit_offset + use < bit_offset) return fail(SVS_ERR_INVALID_ARG, "bit_offset + n_bits overflows");
    const HostPayload payload{bits_packed, bits_ascii, bit_offset, use};
    const int32_t H = planes->height, W = planes->width;
    const int64_t rp = planes->row_pitch, fp = planes->frame_pitch;
    const bool rows_packed = rp == W, frames_packed = rows_packed && fp == (int64_t)H * W;
    // in-place embedding (stego overlaps gray) with a gray reference asked for: the reference must be taken BEFORE the first
    // download lands in the source (a pageable download blocks)
    const bool ref_first = gray_ref_out && gray_ref_out != gray && ranges_overlap(gray, stego, span);
    uint64_t done_total = 0;
    // the read-back counts of the whole call: two u64 (a margin call: four) in c.bits behind the payload, cleared before the first
    // chunk, added to by every chunk's readback_kernel, downloaded after the last
    const bool readback = (counts || margin) && (flags & SVS_READBACK);
    const size_t counts_at = (payload.bits_bytes() + 7) & ~(size_t)7, counts_bytes = margin ? 32 : 16;
    uint64_t got_counts[4] = {0, 0, 0, 0};
    if (int rc = staged(span, 0, payload.ascii_bytes(), readback ? counts_at + counts_bytes : payload.bits_bytes(), [&](HostStage &c) {
            uint64_t rebased = 0;
            if (int rc = payload.stage(c, &rebased)) return rc;
            uint64_t *d_counts = readback ? reinterpret_cast<uint64_t *>(static_cast<uint8_t *>(c.bits.p) + counts_at) : nullptr;
            if (d_counts) SVS_HIP(hipMemsetAsync(d_counts, 0, counts_bytes, c.st[0]));
            if (ref_first) copy_gray_reference(gray_ref_out, gray, planes, frames_packed, span);
            uint8_t *d = static_cast<uint8_t *>(c.frames.p);
            const int rc = embed_chunks(
                c, planes, 1, gray, g.n_ac, use, n_bits, rebased,
                [&](const svs_planes &sub, int64_t off, int32_t f0, uint64_t chunk_offset, uint64_t budget, uint64_t *done, hipStream_t up) {
                    // keyed or dithered: whole frames, so that a chunk boundary never changes a block's (t, i)
                    svs_block_order order;
                    svs_dither dither;
                    return embed_dev(d + off, d + off, &sub, delta, n_ac, static_cast<const uint8_t *>(c.bits.p), chunk_offset, budget,
                                     flags, done, up, o.chunk((uint32_t)f0, d_counts, &order, &dither));
                },
                [&](const svs::Chunk &ch, int64_t off, hipStream_t st) { return download_pixels(stego, d, planes, ch, off, st); },
                &done_total, o.order != nullptr || o.dither != nullptr || o.matrix != 0u);
            if (!rc && d_counts) SVS_HIP(hipMemcpyAsync(got_counts, d_counts, counts_bytes, hipMemcpyDeviceToHost, c.st[0]));
            // the gray reference is copied by the calling thread HERE, while the streams work: everything is enqueued, the
            // thread would only wait.  (Not when stego overlaps gray: the downloads would overwrite the source first.)
            if (!rc && gray_ref_out && gray_ref_out != gray && !ref_first) copy_gray_reference(gray_ref_out, gray, planes, frames_packed, span);
            return rc;
        }))
        return rc;
    if (n_embedded) *n_embedded = done_total;
    if (readback && margin) *margin = svs_margin_counts{got_counts[0], got_counts[1], got_counts[2], got_counts[3]};
    else if (readback) *counts = svs_readback_counts{got_counts[0], got_counts[1]};
    return SVS_OK;
}

int svs_embed(const uint8_t *gray, uint8_t *stego, const svs_planes *planes, double delta, int n_ac,
              const uint8_t *bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t flags, uint64_t *n_embedded) {
    return embed_host(gray, stego, nullptr, planes, delta, n_ac, bits_packed, nullptr, bit_offset, n_bits, flags, n_embedded,
                      GrayOptions{});
}

int svs_embed_ordered(const uint8_t *gray, uint8_t *stego, const svs_planes *planes, const svs_block_order *order, double delta,
                      int n_ac, const uint8_t *bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t flags,
                      uint64_t *n_embedded) {
    return embed_host(gray, stego, nullptr, planes, delta, n_ac, bits_packed, nullptr, bit_offset, n_bits, flags, n_embedded,
                      GrayOptions{order});
}

int svs_embed_readback_dev(const uint8_t *d_gray, uint8_t *d_stego, const svs_planes *planes, const svs_block_order *order,
                           double delta, int n_ac, const uint8_t *d_bits_packed, uint64_t bit_offset, uint64_t n_bits,
                           uint32_t flags, uint64_t *n_embedded, uint64_t *d_counts, void *stream) {
    return embed_dev(d_gray, d_stego, planes, delta, n_ac, d_bits_packed, bit_offset, n_bits, flags | SVS_READBACK, n_embedded, stream,
                     GrayOptions{order, nullptr, nullptr, d_counts});
}

int svs_embed_readback(const uint8_t *gray, uint8_t *stego, const svs_planes *planes, const svs_block_order *order, double delta,
                       int n_ac, const uint8_t *bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t flags,
                       uint64_t *n_embedded, svs_readback_counts *counts) {
    svs_readback_counts none;
    return embed_host(gray, stego, nullptr, planes, delta, n_ac, bits_packed, nullptr, bit_offset, n_bits, flags | SVS_READBACK,
                      n_embedded, GrayOptions{order, nullptr, nullptr, nullptr, counts ? counts : &none});
}

// every character '0' or '1'?  One OR-reduction over the bytes (vectorised: about 0.05 ms per million characters)
static bool ascii_bits_valid(const char *s, uint64_t n) {
    uint8_t acc = 0;
    for (uint64_t i = 0; i < n; ++i) acc |= (uint8_t)((uint8_t)s[i] ^ 0x30u);
    return (acc & 0xfeu) == 0;
}

int svs_embed_str(const uint8_t *gray, uint8_t *gray_ref_out, uint8_t *stego, const svs_planes *planes, double delta, int n_ac,
                  const char *bits_ascii, uint64_t n_chars, uint32_t flags, uint64_t *n_embedded) {
    if (n_chars && !bits_ascii) return fail(SVS_ERR_INVALID_ARG, "bits pointer is NULL");
    // Only '0' / '1' characters have a pinned meaning: the reference takes int(ch) and sends anything that is not 1 down its
    // "bit 0" branch unconditionally (config_and_setup.py:146-155) - a digit such as '3' then DECREMENTS every index, which is
    // neither bit.  The characters that would be read (the front of the string, up to the capacity) are checked; others are refused.
    if (n_chars) {
        const uint64_t cap = svs_capacity_bits(planes, n_ac);
        if (!ascii_bits_valid(bits_ascii, n_chars < cap ? n_chars : cap))
            return fail(SVS_ERR_INVALID_ARG, "the payload must consist of '0' and '1' characters");
    }
    if (gray_ref_out && planes && planes->n_frames > 0 && planes->height > 0 && planes->width > 0) {
        const uint64_t span = span_bytes(planes);
        if (ranges_overlap(gray_ref_out, stego, span)) return fail(SVS_ERR_INVALID_ARG, "gray_ref_out must not overlap the stego buffer");
        if (gray_ref_out != gray && ranges_overlap(gray_ref_out, gray, span))
            return fail(SVS_ERR_INVALID_ARG, "gray_ref_out must be the gray buffer itself or not overlap it");
    }
    return embed_host(gray, stego, gray_ref_out, planes, delta, n_ac, nullptr, bits_ascii ? bits_ascii : "", 0, n_chars, flags, n_embedded,
                      GrayOptions{});
}

int svs_extract(const uint8_t *gray, const svs_planes *planes, double delta, int n_ac, uint8_t *bits_packed_out,
                uint64_t out_capacity_bytes, uint32_t flags, uint64_t *n_bits_out) {
    return svs_extract_ordered(gray, planes, nullptr, delta, n_ac, bits_packed_out, out_capacity_bytes, flags, n_bits_out);
}

// every gray host extract call: the frames staged whole, in one piece.  A tally or a histogram is added into a zeroed buffer of
// the staging context and downloaded; an empty call zero-fills the caller's.
static int extract_host(const uint8_t *gray, const svs_planes *planes, double delta, int n_ac, uint8_t *out, uint64_t out_capacity_bytes,
                        uint32_t flags, uint64_t *n_bits_out, const GrayOptions &o) {
    svs::Geometry g;
    uint64_t total = 0, cap = 0, bytes = 0;
    if (int rc = extract_checks(gray, out, false, planes, delta, n_ac, out_capacity_bytes, flags, n_bits_out, o, &g, &total, &cap, &bytes))
        return rc;
    if (cap == 0) {
        if (o.out.adds() && out) memset(out, 0, bytes);
        if (n_bits_out) *n_bits_out = 0;
        return SVS_OK;
    }
    return extract_staged(
        gray, span_bytes(planes), bytes, 0, n_bits_out,
        [&](const uint8_t *d_in, uint8_t *d_out, uint64_t d_bytes, uint64_t *got, hipStream_t st) {
            if (o.out.adds()) SVS_HIP(hipMemsetAsync(d_out, 0, bytes, st));
            return extract_dev(d_in, planes, delta, n_ac, d_out, d_bytes, flags, got, st, o);
        },
        [&](HostStage &c, hipStream_t st) { return stage_d2h(st, out, c.bits.p, bytes); });
}

int svs_extract_ordered(const uint8_t *gray, const svs_planes *planes, const svs_block_order *order, double delta, int n_ac,
                        uint8_t *bits_packed_out, uint64_t out_capacity_bytes, uint32_t flags, uint64_t *n_bits_out) {
    return extract_host(gray, planes, delta, n_ac, bits_packed_out, out_capacity_bytes, flags, n_bits_out, GrayOptions{order});
}

// ---- coefficient selection ------------------------------------------------------------------------------------------
// JPEG zig-zag scan of the 8 x 8 block as flat row-major indices; position 0 is DC
static const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

int svs_coeffs_scan(svs_coeffs *out, int scan, int first, int count) {
    if (!out) return fail(SVS_ERR_INVALID_ARG, "out is NULL");
    if (scan != SVS_SCAN_ROW_MAJOR && scan != SVS_SCAN_ZIGZAG) return fail(SVS_ERR_INVALID_ARG, "unknown scan %d", scan);
    if (first < 1 || count < 0 || count > 63 || first + count > 64)
        return fail(SVS_ERR_INVALID_ARG, "scan positions %d..%d are not inside 1..63", first, first + count - 1);
    memset(out, 0, sizeof *out);
    out->count = (uint8_t)count;
    for (int i = 0; i < count; ++i) out->index[i] = scan == SVS_SCAN_ZIGZAG ? kZigzag[first + i] : (uint8_t)(first + i);
    return SVS_OK;
}

// ---- the requantisation channel (include/svsdct.h) ----------------------------------------------------------------------
// ITU-T T.81 Annex K, table K.1 (luminance), in natural row-major order
static const uint8_t kAnnexKLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                        14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                        18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                        49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};

int svs_quality_steps(svs_steps *out, int quality) {
    if (!out) return fail(SVS_ERR_INVALID_ARG, "out is NULL");
    if (quality < 1 || quality > 100) return fail(SVS_ERR_INVALID_ARG, "quality %d is not in 1..100", quality);
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;   // IJG's scaling
    for (int k = 0; k < 64; ++k) {
        const int v = (kAnnexKLuma[k] * s + 50) / 100;
        out->step[k] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
    return SVS_OK;
}

// what both requantise calls check before any device work, in this order -> the kernel's channel, geometry and block count
// (total = 0: an empty call, whose pointers were not looked at)
static int requantise_checks(const void *in, const void *out, bool device, const svs_planes *planes, const svs_steps *steps,
                             uint32_t flags, svs::ChannelArgs *chan, svs::Geometry *g, uint64_t *total) {
    if (!steps) return fail(SVS_ERR_INVALID_ARG, "steps is NULL");
    for (int k = 0; k < 64; ++k)
        if (steps->step[k] < 1 || steps->step[k] > 255)
            return fail(SVS_ERR_INVALID_ARG, "step[%d] = %u is not in 1..255", k, (unsigned)steps->step[k]);
    if (flags != 0) return fail(SVS_ERR_INVALID_ARG, "unknown flags 0x%x (the requantise calls take none)", flags);
    if (int rc = make_geometry(planes, 0, g, total)) return rc;
    *chan = svs::make_channel_args(steps->step);
    if (*total == 0) return SVS_OK;
    if (!in || !out) return fail(SVS_ERR_INVALID_ARG, "in/out pointer is NULL");
    if (device && (((uintptr_t)in % 8) || ((uintptr_t)out % 8)))
        return fail(SVS_ERR_INVALID_ARG, "plane pointers must be 8-byte aligned");
    if (in != out && ranges_overlap(in, out, span_bytes(planes)))
        return fail(SVS_ERR_INVALID_ARG, "the output must be the input itself (in place) or must not overlap it");
    return SVS_OK;
}

int svs_requantise_dev(const uint8_t *d_in, uint8_t *d_out, const svs_planes *planes, const svs_steps *steps, uint32_t flags,
                       void *stream) {
    svs::ChannelArgs chan;
    svs::Geometry g;
    uint64_t total = 0;
    if (int rc = requantise_checks(d_in, d_out, true, planes, steps, flags, &chan, &g, &total)) return rc;
    if (total == 0) return SVS_OK;
    return launch_requantise(total, (hipStream_t)stream, d_in, d_out, g, chan);
}

// Host form: svs_embed's chunk pipeline without a payload - blocks are independent, so a chunk is any band of block rows
int svs_requantise(const uint8_t *in, uint8_t *out, const svs_planes *planes, const svs_steps *steps, uint32_t flags) {
    svs::ChannelArgs chan;
    svs::Geometry g;
    uint64_t total = 0;
    if (int rc = requantise_checks(in, out, false, planes, steps, flags, &chan, &g, &total)) return rc;
    if (total == 0) return SVS_OK;
    return staged(span_bytes(planes), 0, 0, 0, [&](HostStage &c) {
        uint8_t *d = static_cast<uint8_t *>(c.frames.p);
        uint64_t done_total = 0;
        return embed_chunks(
            c, planes, 1, in, 0, 0, 0, 0,
            [&](const svs_planes &sub, int64_t off, int32_t, uint64_t, uint64_t, uint64_t *, hipStream_t up) {
                svs::Geometry sg;
                uint64_t sub_total = 0;
                if (int rc = make_geometry(&sub, 0, &sg, &sub_total)) return rc;
                return launch_requantise(sub_total, up, d + off, d + off, sg, chan);
            },
            [&](const svs::Chunk &ch, int64_t off, hipStream_t st) { return download_pixels(out, d, planes, ch, off, st); },
            &done_total);
    });
}

// The select calls are the ordered calls at n_ac = coeffs->count with the selection's table; the prefix 1..count passes no
// table and is the ordered call itself.  The dithered calls are the ordered calls (with a selection: the select calls) with the
// dither handed down to the plan; coeffs NULL: the row-major prefix 1..n_ac.  The dithered calls with the read-back pass take
// each of order, coeffs and dither or NULL.  with_options: what is given is checked before anything else.
int svs_embed_select_dev(const uint8_t *d_gray, uint8_t *d_stego, const svs_planes *planes, const svs_block_order *order,
                         const svs_coeffs *coeffs, double delta, const uint8_t *d_bits_packed, uint64_t bit_offset,
                         uint64_t n_bits, uint32_t flags, uint64_t *n_embedded, void *stream) {
    return with_options(kSelectEmbed, order, coeffs, nullptr, flags, 0, [&](int n, const GrayOptions &o) {
        return embed_dev(d_gray, d_stego, planes, delta, n, d_bits_packed, bit_offset, n_bits, flags, n_embedded, stream, o);
    });
}

int svs_embed_select(const uint8_t *gray, uint8_t *stego, const svs_planes *planes, const svs_block_order *order,
                     const svs_coeffs *coeffs, double delta, const uint8_t *bits_packed, uint64_t bit_offset, uint64_t n_bits,
                     uint32_t flags, uint64_t *n_embedded) {
    return with_options(kSelectEmbed, order, coeffs, nullptr, flags, 0, [&](int n, const GrayOptions &o) {
        return embed_host(gray, stego, nullptr, planes, delta, n, bits_packed, nullptr, bit_offset, n_bits, flags, n_embedded, o);
    });
}

int svs_extract_select_dev(const uint8_t *d_gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                           double delta, uint8_t *d_bits_packed_out, uint64_t out_capacity_bytes, uint32_t flags,
                           uint64_t *n_bits_out, void *stream) {
    return with_options(kSelectExtract, order, coeffs, nullptr, flags, 0, [&](int n, const GrayOptions &o) {
        return extract_dev(d_gray, planes, delta, n, d_bits_packed_out, out_capacity_bytes, flags, n_bits_out, stream, o);
    });
}

int svs_extract_select(const uint8_t *gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                       double delta, uint8_t *bits_packed_out, uint64_t out_capacity_bytes, uint32_t flags, uint64_t *n_bits_out) {
    return with_options(kSelectExtract, order, coeffs, nullptr, flags, 0, [&](int n, const GrayOptions &o) {
        return extract_host(gray, planes, delta, n, bits_packed_out, out_capacity_bytes, flags, n_bits_out, o);
    });
}

int svs_embed_dithered_dev(const uint8_t *d_gray, uint8_t *d_stego, const svs_planes *planes, const svs_block_order *order,
                           const svs_coeffs *coeffs, const svs_dither *dither, double delta, int n_ac,
                           const uint8_t *d_bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t flags,
                           uint64_t *n_embedded, void *stream) {
    return with_options(kDitheredEmbed, order, coeffs, dither, flags, n_ac, [&](int n, const GrayOptions &o) {
        return embed_dev(d_gray, d_stego, planes, delta, n, d_bits_packed, bit_offset, n_bits, flags, n_embedded, stream, o);
    });
}

int svs_embed_dithered(const uint8_t *gray, uint8_t *stego, const svs_planes *planes, const svs_block_order *order,
                       const svs_coeffs *coeffs, const svs_dither *dither, double delta, int n_ac, const uint8_t *bits_packed,
                       uint64_t bit_offset, uint64_t n_bits, uint32_t flags, uint64_t *n_embedded) {
    return with_options(kDitheredEmbed, order, coeffs, dither, flags, n_ac, [&](int n, const GrayOptions &o) {
        return embed_host(gray, stego, nullptr, planes, delta, n, bits_packed, nullptr, bit_offset, n_bits, flags, n_embedded, o);
    });
}

int svs_extract_dithered_dev(const uint8_t *d_gray, const svs_planes *planes, const svs_block_order *order,
                             const svs_coeffs *coeffs, const svs_dither *dither, double delta, int n_ac,
                             uint8_t *d_bits_packed_out, uint64_t out_capacity_bytes, uint32_t flags, uint64_t *n_bits_out,
                             void *stream) {
    return with_options(kDitheredExtract, order, coeffs, dither, flags, n_ac, [&](int n, const GrayOptions &o) {
        return extract_dev(d_gray, planes, delta, n, d_bits_packed_out, out_capacity_bytes, flags, n_bits_out, stream, o);
    });
}

int svs_extract_dithered(const uint8_t *gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                         const svs_dither *dither, double delta, int n_ac, uint8_t *bits_packed_out, uint64_t out_capacity_bytes,
                         uint32_t flags, uint64_t *n_bits_out) {
    return with_options(kDitheredExtract, order, coeffs, dither, flags, n_ac, [&](int n, const GrayOptions &o) {
        return extract_host(gray, planes, delta, n, bits_packed_out, out_capacity_bytes, flags, n_bits_out, o);
    });
}

// The soft calls are the dithered extract calls with each of order, coeffs and dither optional and an output of their own
// (include/svsdct.h, ExtractOutput): the same checks in the same order, the same staging.  svs_soft_extract*: one byte per
// capacity bit.  svs_soft_vote*: the kernel's soft side adds each byte's vote into tally[stream position mod period] instead of
// writing it.  svs_soft_histogram*: no order, and it counts each byte into hist[frame * 256 + byte].
int svs_soft_extract_dev(const uint8_t *d_gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                         const svs_dither *dither, double delta, int n_ac, uint8_t *d_soft_out, uint64_t out_capacity_bytes,
                         uint32_t flags, uint64_t *n_bits_out, void *stream) {
    return with_options(kSoftExtract, order, coeffs, dither, flags, n_ac, [&](int n, GrayOptions o) {
        o.out = {ExtractOutput::SOFT};
        return extract_dev(d_gray, planes, delta, n, d_soft_out, out_capacity_bytes, flags, n_bits_out, stream, o);
    });
}

int svs_soft_extract(const uint8_t *gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                     const svs_dither *dither, double delta, int n_ac, uint8_t *soft_out, uint64_t out_capacity_bytes, uint32_t flags,
                     uint64_t *n_bits_out) {
    return with_options(kSoftExtract, order, coeffs, dither, flags, n_ac, [&](int n, GrayOptions o) {
        o.out = {ExtractOutput::SOFT};
        return extract_host(gray, planes, delta, n, soft_out, out_capacity_bytes, flags, n_bits_out, o);
    });
}

int svs_soft_vote_dev(const uint8_t *d_gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                      const svs_dither *dither, double delta, int n_ac, uint64_t period, uint64_t stream_bit0, int32_t *d_tally,
                      uint32_t flags, uint64_t *n_bits_out, void *stream) {
    return with_options(kSoftVote, order, coeffs, dither, flags, n_ac, [&](int n, GrayOptions o) {
        o.out = {ExtractOutput::VOTE, period, stream_bit0};
        return extract_dev(d_gray, planes, delta, n, reinterpret_cast<uint8_t *>(d_tally), 0, flags, n_bits_out, stream, o);
    });
}

int svs_soft_vote(const uint8_t *gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                  const svs_dither *dither, double delta, int n_ac, uint64_t period, uint64_t stream_bit0, int32_t *tally_out,
                  uint32_t flags, uint64_t *n_bits_out) {
    return with_options(kSoftVote, order, coeffs, dither, flags, n_ac, [&](int n, GrayOptions o) {
        o.out = {ExtractOutput::VOTE, period, stream_bit0};
        return extract_host(gray, planes, delta, n, reinterpret_cast<uint8_t *>(tally_out), 0, flags, n_bits_out, o);
    });
}

int svs_soft_histogram_dev(const uint8_t *d_gray, const svs_planes *planes, const svs_coeffs *coeffs, const svs_dither *dither,
                           double delta, int n_ac, uint32_t *d_hist, uint32_t flags, uint64_t *n_bits_out, void *stream) {
    return with_options(kSoftHistogram, nullptr, coeffs, dither, flags, n_ac, [&](int n, GrayOptions o) {
        o.out = {ExtractOutput::HIST};
        return extract_dev(d_gray, planes, delta, n, reinterpret_cast<uint8_t *>(d_hist), 0, flags, n_bits_out, stream, o);
    });
}

int svs_soft_histogram(const uint8_t *gray, const svs_planes *planes, const svs_coeffs *coeffs, const svs_dither *dither,
                       double delta, int n_ac, uint32_t *hist_out, uint32_t flags, uint64_t *n_bits_out) {
    return with_options(kSoftHistogram, nullptr, coeffs, dither, flags, n_ac, [&](int n, GrayOptions o) {
        o.out = {ExtractOutput::HIST};
        return extract_host(gray, planes, delta, n, reinterpret_cast<uint8_t *>(hist_out), 0, flags, n_bits_out, o);
    });
}

int svs_embed_dithered_readback_dev(const uint8_t *d_gray, uint8_t *d_stego, const svs_planes *planes, const svs_block_order *order,
                                    const svs_coeffs *coeffs, const svs_dither *dither, double delta, int n_ac,
                                    const uint8_t *d_bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t flags,
                                    uint64_t *n_embedded, uint64_t *d_counts, void *stream) {
    return with_options(kKeyedReadback, order, coeffs, dither, flags, n_ac, [&](int n, GrayOptions o) {
        o.d_counts = d_counts;
        return embed_dev(d_gray, d_stego, planes, delta, n, d_bits_packed, bit_offset, n_bits, flags | SVS_READBACK, n_embedded, stream, o);
    });
}

int svs_embed_dithered_readback(const uint8_t *gray, uint8_t *stego, const svs_planes *planes, const svs_block_order *order,
                                const svs_coeffs *coeffs, const svs_dither *dither, double delta, int n_ac,
                                const uint8_t *bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t flags,
                                uint64_t *n_embedded, svs_readback_counts *counts) {
    return with_options(kKeyedReadback, order, coeffs, dither, flags, n_ac, [&](int n, GrayOptions o) {
        svs_readback_counts none;
        o.counts = counts ? counts : &none;
        return embed_host(gray, stego, nullptr, planes, delta, n, bits_packed, nullptr, bit_offset, n_bits, flags | SVS_READBACK,
                          n_embedded, o);
    });
}

// ---- per-coefficient QIM steps (include/svsdct.h) -------------------------------------------------------------------------
int svs_matched_steps(svs_qim_steps *out, const svs_steps *codec, int multiple, int floor) {
    if (!out) return fail(SVS_ERR_INVALID_ARG, "out is NULL");
    if (!codec) return fail(SVS_ERR_INVALID_ARG, "codec is NULL");
    if (multiple < 1 || multiple > 16) return fail(SVS_ERR_INVALID_ARG, "multiple %d is not in 1..16", multiple);
    if (floor < 0 || floor > 4095) return fail(SVS_ERR_INVALID_ARG, "floor %d is not in 0..4095", floor);
    svs_qim_steps t{};
    for (int k = 0; k < 64; ++k) {   // the codec table is checked as svs_requantise checks it, DC included
        const int s = codec->step[k];
        if (s < 1 || s > 255) return fail(SVS_ERR_INVALID_ARG, "step[%d] = %d is not in 1..255", k, s);
        if (k == 0) continue;
        const int need = (floor + s - 1) / s;   // ceil(floor / s)
        const int d = s * (multiple > need ? multiple : need);
        if (d > 4095) return fail(SVS_ERR_INVALID_ARG, "delta[%d] = %d exceeds 4095", k, d);
        t.delta[k] = (uint16_t)d;
    }
    *out = t;
    return SVS_OK;
}

int svs_stepped_embed_dev(const uint8_t *d_gray, uint8_t *d_stego, const svs_planes *planes, const svs_block_order *order,
                          const svs_coeffs *coeffs, const svs_dither *dither, const svs_qim_steps *steps, int n_ac,
                          const uint8_t *d_bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t flags,
                          uint64_t *n_embedded, void *stream) {
    return with_steps(kSteppedEmbed, order, coeffs, dither, steps, flags, n_ac, [&](int n, const GrayOptions &o) {
        return embed_dev(d_gray, d_stego, planes, kSteppedRouteDelta, n, d_bits_packed, bit_offset, n_bits, flags, n_embedded, stream, o);
    });
}

int svs_stepped_embed(const uint8_t *gray, uint8_t *stego, const svs_planes *planes, const svs_block_order *order,
                      const svs_coeffs *coeffs, const svs_dither *dither, const svs_qim_steps *steps, int n_ac,
                      const uint8_t *bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t flags, uint64_t *n_embedded) {
    return with_steps(kSteppedEmbed, order, coeffs, dither, steps, flags, n_ac, [&](int n, const GrayOptions &o) {
        return embed_host(gray, stego, nullptr, planes, kSteppedRouteDelta, n, bits_packed, nullptr, bit_offset, n_bits, flags,
                          n_embedded, o);
    });
}

// The stepped embed followed by the read-back pass in its stepped form: the keyed read-back calls inside with_steps
int svs_stepped_embed_readback_dev(const uint8_t *d_gray, uint8_t *d_stego, const svs_planes *planes, const svs_block_order *order,
                                   const svs_coeffs *coeffs, const svs_dither *dither, const svs_qim_steps *steps, int n_ac,
                                   const uint8_t *d_bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t flags,
                                   uint64_t *n_embedded, uint64_t *d_counts, void *stream) {
    return with_steps(kSteppedReadback, order, coeffs, dither, steps, flags, n_ac, [&](int n, GrayOptions o) {
        o.d_counts = d_counts;
        return embed_dev(d_gray, d_stego, planes, kSteppedRouteDelta, n, d_bits_packed, bit_offset, n_bits, flags | SVS_READBACK,
                         n_embedded, stream, o);
    });
}

int svs_stepped_embed_readback(const uint8_t *gray, uint8_t *stego, const svs_planes *planes, const svs_block_order *order,
                               const svs_coeffs *coeffs, const svs_dither *dither, const svs_qim_steps *steps, int n_ac,
                               const uint8_t *bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t flags,
                               uint64_t *n_embedded, svs_readback_counts *counts) {
    return with_steps(kSteppedReadback, order, coeffs, dither, steps, flags, n_ac, [&](int n, GrayOptions o) {
        svs_readback_counts none;
        o.counts = counts ? counts : &none;
        return embed_host(gray, stego, nullptr, planes, kSteppedRouteDelta, n, bits_packed, nullptr, bit_offset, n_bits,
                          flags | SVS_READBACK, n_embedded, o);
    });
}

// The stepped read-back embed followed by the margin pass (include/svsdct.h): the same calls with the gate in the options;
// min_margin = 0 is svs_stepped_embed_readback* itself, with two more counts that stay 0
int svs_stepped_embed_readback_margin_dev(const uint8_t *d_gray, uint8_t *d_stego, const svs_planes *planes, const svs_block_order *order,
                                          const svs_coeffs *coeffs, const svs_dither *dither, const svs_qim_steps *steps, int n_ac,
                                          const uint8_t *d_bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t min_margin,
                                          uint32_t flags, uint64_t *n_embedded, uint64_t *d_counts, void *stream) {
    return with_steps(kSteppedReadback, order, coeffs, dither, steps, flags, n_ac, [&](int n, GrayOptions o) {
        o.d_counts = d_counts;
        return embed_dev(d_gray, d_stego, planes, kSteppedRouteDelta, n, d_bits_packed, bit_offset, n_bits, flags | SVS_READBACK,
                         n_embedded, stream, o);
    }, min_margin);
}

int svs_stepped_embed_readback_margin(const uint8_t *gray, uint8_t *stego, const svs_planes *planes, const svs_block_order *order,
                                      const svs_coeffs *coeffs, const svs_dither *dither, const svs_qim_steps *steps, int n_ac,
                                      const uint8_t *bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t min_margin,
                                      uint32_t flags, uint64_t *n_embedded, svs_margin_counts *counts) {
    return with_steps(kSteppedReadback, order, coeffs, dither, steps, flags, n_ac, [&](int n, GrayOptions o) {
        svs_margin_counts none;
        o.margin_counts = counts ? counts : &none;
        return embed_host(gray, stego, nullptr, planes, kSteppedRouteDelta, n, bits_packed, nullptr, bit_offset, n_bits,
                          flags | SVS_READBACK, n_embedded, o);
    }, min_margin);
}

int svs_stepped_extract_dev(const uint8_t *d_gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                            const svs_dither *dither, const svs_qim_steps *steps, int n_ac, uint8_t *d_bits_packed_out,
                            uint64_t out_capacity_bytes, uint32_t flags, uint64_t *n_bits_out, void *stream) {
    return with_steps(kSteppedExtract, order, coeffs, dither, steps, flags, n_ac, [&](int n, const GrayOptions &o) {
        return extract_dev(d_gray, planes, kSteppedRouteDelta, n, d_bits_packed_out, out_capacity_bytes, flags, n_bits_out, stream, o);
    });
}

int svs_stepped_extract(const uint8_t *gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                        const svs_dither *dither, const svs_qim_steps *steps, int n_ac, uint8_t *bits_packed_out,
                        uint64_t out_capacity_bytes, uint32_t flags, uint64_t *n_bits_out) {
    return with_steps(kSteppedExtract, order, coeffs, dither, steps, flags, n_ac, [&](int n, const GrayOptions &o) {
        return extract_host(gray, planes, kSteppedRouteDelta, n, bits_packed_out, out_capacity_bytes, flags, n_bits_out, o);
    });
}

// The stepped soft calls are the soft calls inside with_steps, under the stepped extract's policy: the table is checked first,
// then what the soft call checks, in its order; the call routes with a positive delta that no kernel reads, so the vote's and
// the histogram's delta <= 0 refusal cannot occur (an entry is at least 1).
int svs_stepped_soft_extract_dev(const uint8_t *d_gray, const svs_planes *planes, const svs_block_order *order,
                                 const svs_coeffs *coeffs, const svs_dither *dither, const svs_qim_steps *steps, int n_ac,
                                 uint8_t *d_soft_out, uint64_t out_capacity_bytes, uint32_t flags, uint64_t *n_bits_out, void *stream) {
    return with_steps(kSteppedExtract, order, coeffs, dither, steps, flags, n_ac, [&](int n, GrayOptions o) {
        o.out = {ExtractOutput::SOFT};
        return extract_dev(d_gray, planes, kSteppedRouteDelta, n, d_soft_out, out_capacity_bytes, flags, n_bits_out, stream, o);
    });
}

int svs_stepped_soft_extract(const uint8_t *gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                             const svs_dither *dither, const svs_qim_steps *steps, int n_ac, uint8_t *soft_out,
                             uint64_t out_capacity_bytes, uint32_t flags, uint64_t *n_bits_out) {
    return with_steps(kSteppedExtract, order, coeffs, dither, steps, flags, n_ac, [&](int n, GrayOptions o) {
        o.out = {ExtractOutput::SOFT};
        return extract_host(gray, planes, kSteppedRouteDelta, n, soft_out, out_capacity_bytes, flags, n_bits_out, o);
    });
}

int svs_stepped_soft_vote_dev(const uint8_t *d_gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                              const svs_dither *dither, const svs_qim_steps *steps, int n_ac, uint64_t period, uint64_t stream_bit0,
                              int32_t *d_tally, uint32_t flags, uint64_t *n_bits_out, void *stream) {
    return with_steps(kSteppedExtract, order, coeffs, dither, steps, flags, n_ac, [&](int n, GrayOptions o) {
        o.out = {ExtractOutput::VOTE, period, stream_bit0};
        return extract_dev(d_gray, planes, kSteppedRouteDelta, n, reinterpret_cast<uint8_t *>(d_tally), 0, flags, n_bits_out, stream, o);
    });
}

int svs_stepped_soft_vote(const uint8_t *gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                          const svs_dither *dither, const svs_qim_steps *steps, int n_ac, uint64_t period, uint64_t stream_bit0,
                          int32_t *tally_out, uint32_t flags, uint64_t *n_bits_out) {
    return with_steps(kSteppedExtract, order, coeffs, dither, steps, flags, n_ac, [&](int n, GrayOptions o) {
        o.out = {ExtractOutput::VOTE, period, stream_bit0};
        return extract_host(gray, planes, kSteppedRouteDelta, n, reinterpret_cast<uint8_t *>(tally_out), 0, flags, n_bits_out, o);
    });
}

int svs_stepped_soft_histogram_dev(const uint8_t *d_gray, const svs_planes *planes, const svs_coeffs *coeffs, const svs_dither *dither,
                                   const svs_qim_steps *steps, int n_ac, uint32_t *d_hist, uint32_t flags, uint64_t *n_bits_out,
                                   void *stream) {
    return with_steps(kSteppedExtract, nullptr, coeffs, dither, steps, flags, n_ac, [&](int n, GrayOptions o) {
        o.out = {ExtractOutput::HIST};
        return extract_dev(d_gray, planes, kSteppedRouteDelta, n, reinterpret_cast<uint8_t *>(d_hist), 0, flags, n_bits_out, stream, o);
    });
}

int svs_stepped_soft_histogram(const uint8_t *gray, const svs_planes *planes, const svs_coeffs *coeffs, const svs_dither *dither,
                               const svs_qim_steps *steps, int n_ac, uint32_t *hist_out, uint32_t flags, uint64_t *n_bits_out) {
    return with_steps(kSteppedExtract, nullptr, coeffs, dither, steps, flags, n_ac, [&](int n, GrayOptions o) {
        o.out = {ExtractOutput::HIST};
        return extract_host(gray, planes, kSteppedRouteDelta, n, reinterpret_cast<uint8_t *>(hist_out), 0, flags, n_bits_out, o);
    });
}

// ---- matrix embedding (include/svsdct.h) -----------------------------------------------------------------------------------
uint64_t svs_matrix_capacity_bits(const svs_planes *p, const svs_matrix *m) {
    if (!m || m->k < 1 || m->k > 6) return 0;
    return svs_capacity_bits(p, (int)m->k);
}

int svs_matrix_embed_dev(const uint8_t *d_gray, uint8_t *d_stego, const svs_planes *planes, const svs_block_order *order,
                         const svs_coeffs *coeffs, const svs_dither *dither, const svs_qim_steps *steps, const svs_matrix *matrix,
                         int n_ac, const uint8_t *d_bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t flags,
                         uint64_t *n_embedded, void *stream) {
    return with_matrix(kMatrixEmbed, order, coeffs, dither, steps, matrix, flags, n_ac, [&](int k, const GrayOptions &o) {
        return embed_dev(d_gray, d_stego, planes, kSteppedRouteDelta, k, d_bits_packed, bit_offset, n_bits, flags, n_embedded, stream, o);
    });
}

int svs_matrix_embed(const uint8_t *gray, uint8_t *stego, const svs_planes *planes, const svs_block_order *order,
                     const svs_coeffs *coeffs, const svs_dither *dither, const svs_qim_steps *steps, const svs_matrix *matrix, int n_ac,
                     const uint8_t *bits_packed, uint64_t bit_offset, uint64_t n_bits, uint32_t flags, uint64_t *n_embedded) {
    return with_matrix(kMatrixEmbed, order, coeffs, dither, steps, matrix, flags, n_ac, [&](int k, const GrayOptions &o) {
        return embed_host(gray, stego, nullptr, planes, kSteppedRouteDelta, k, bits_packed, nullptr, bit_offset, n_bits, flags,
                          n_embedded, o);
    });
}

int svs_matrix_extract_dev(const uint8_t *d_gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                           const svs_dither *dither, const svs_qim_steps *steps, const svs_matrix *matrix, int n_ac,
                           uint8_t *d_bits_packed_out, uint64_t out_capacity_bytes, uint32_t flags, uint64_t *n_bits_out, void *stream) {
    return with_matrix(kMatrixExtract, order, coeffs, dither, steps, matrix, flags, n_ac, [&](int k, const GrayOptions &o) {
        return extract_dev(d_gray, planes, kSteppedRouteDelta, k, d_bits_packed_out, out_capacity_bytes, flags, n_bits_out, stream, o);
    });
}

int svs_matrix_extract(const uint8_t *gray, const svs_planes *planes, const svs_block_order *order, const svs_coeffs *coeffs,
                       const svs_dither *dither, const svs_qim_steps *steps, const svs_matrix *matrix, int n_ac,
                       uint8_t *bits_packed_out, uint64_t out_capacity_bytes, uint32_t flags, uint64_t *n_bits_out) {
    return with_matrix(kMatrixExtract, order, coeffs, dither, steps, matrix, flags, n_ac, [&](int k, const GrayOptions &o) {
        return extract_host(gray, planes, kSteppedRouteDelta, k, bits_packed_out, out_capacity_bytes, flags, n_bits_out, o);
    });
}

int svs_extract_str(const uint8_t *gray, const svs_planes *planes, double delta, int n_ac, char *bits_ascii_out,
                    uint64_t out_capacity_chars, uint32_t flags, uint64_t *n_bits_out) {
    svs::Geometry g;
    uint64_t total = 0, cap = 0;
    if (int rc = extract_geometry(planes, n_ac, &g, &total, &cap, n_bits_out)) return rc;
    if (int rc = check_extract_flags(flags)) return rc;
    if (cap == 0) return SVS_OK;
    if (!gray || !bits_ascii_out) return fail(SVS_ERR_INVALID_ARG, "gray/bits pointer is NULL");
    if (int rc = check_capacity(cap, out_capacity_chars, "characters")) return rc;
    const uint64_t bytes = (cap + 7) / 8;
    return extract_staged(
        gray, span_bytes(planes), bytes, 8 * bytes + 8, n_bits_out,
        [&](const uint8_t *d_in, uint8_t *d_bits, uint64_t d_bytes, uint64_t *got, hipStream_t st) {
            return svs_extract_dev(d_in, planes, delta, n_ac, d_bits, d_bytes, flags, got, st);
        },
        [&](HostStage &c, hipStream_t st) {
            const uint32_t blocks = (uint32_t)((bytes + 255) / 256 < 4096 ? (bytes + 255) / 256 : 4096);
            hipLaunchKernelGGL(svs::packed_to_ascii_kernel, dim3(blocks), dim3(256), 0, st, static_cast<const uint8_t *>(c.bits.p),
                               bytes, static_cast<svs::u32x2 *>(c.third.p));
            if (hipGetLastError() != hipSuccess) return fail(SVS_ERR_HIP, "packed_to_ascii_kernel launch failed");
            return stage_d2h(st, bits_ascii_out, c.third.p, cap);
        });
}

int svs_shutdown(void) {
    t_stage.release();
    return SVS_OK;
}

// the BGR row movers (load_bgr_row, wave_load_gray, wave_store_gray_as_bgr) access rows 8 bytes at a time
// block_offset_bgr takes the byte column of a block, 24 * (blocks before it in the row), in 32 bits
static int check_bgr_width(const svs_planes *p) {
    if (3 * (int64_t)p->width >= (1ll << 32))
        return fail(SVS_ERR_INVALID_ARG, "BGR rows of %d pixels are 4 GiB or longer; at most 1431655760 pixels per row", p->width);
    return SVS_OK;
}

static int check_bgr(const svs_planes *p, const void *bgr, int64_t rp, int64_t fp) {
    if (int rc = check_bgr_width(p)) return rc;
    if (!bgr || ((uintptr_t)bgr % 8)) return fail(SVS_ERR_INVALID_ARG, "BGR pointer NULL or not 8-byte aligned");
    if (rp < 3 * (int64_t)p->width || (rp % 8) || fp < rp * p->height || (fp % 8))
        return fail(SVS_ERR_INVALID_ARG, "BGR pitches must cover 3*width bytes per row and be multiples of 8");
    return SVS_OK;
}

// {wb, wg, wr, shift}: the sum taken in 64 bits, so that no weight above 2^shift can wrap it back to 2^shift
static int check_weights(const uint32_t *w) {
    if (w[3] < 1 || w[3] > 16 || (uint64_t)w[0] + w[1] + w[2] != (1ull << w[3]))
        return fail(SVS_ERR_INVALID_ARG, "weights must sum to 2^shift with 1 <= shift <= 16");
    return SVS_OK;
}

int svs_bgr_to_gray_dev(const uint8_t *d_bgr, int64_t bgr_row_pitch, int64_t bgr_frame_pitch, uint8_t *d_gray,
                        const svs_planes *planes, const uint32_t *weights, void *stream) {
    svs::Geometry g;
    uint64_t total = 0;
    if (int rc = make_geometry(planes, 1, &g, &total)) return rc;
    if (total == 0) return SVS_OK;
    if (!d_gray || ((uintptr_t)d_gray % 8)) return fail(SVS_ERR_INVALID_ARG, "gray pointer NULL or unaligned");
    if (int rc = check_bgr(planes, d_bgr, bgr_row_pitch, bgr_frame_pitch)) return rc;
    const uint32_t dflt[4] = {3735u, 19235u, 9798u, 15u};
    const uint32_t *w = weights ? weights : dflt;
    if (int rc = check_weights(w)) return rc;
    svs::ColourParams c{bgr_row_pitch, bgr_frame_pitch, 0, 0, w[0], w[1], w[2], w[3]};
    g.xcd_chunk = svs::kEighth;
    hipLaunchKernelGGL(svs::bgr_to_gray_kernel, dim3((uint32_t)((total + SVS_WG - 1) / SVS_WG)), dim3(SVS_WG), 0,
                       (hipStream_t)stream, d_bgr, d_gray, g, c);
    SVS_HIP(hipGetLastError());
    return SVS_OK;
}

int svs_gray_to_bgr_dev(const uint8_t *d_gray, const svs_planes *planes, uint8_t *d_bgr, int64_t bgr_row_pitch,
                        int64_t bgr_frame_pitch, void *stream) {
    svs::Geometry g;
    uint64_t total = 0;
    if (int rc = make_geometry(planes, 1, &g, &total)) return rc;
    if (total == 0) return SVS_OK;
    if (!d_gray || ((uintptr_t)d_gray % 8)) return fail(SVS_ERR_INVALID_ARG, "gray pointer NULL or unaligned");
    if (int rc = check_bgr(planes, d_bgr, bgr_row_pitch, bgr_frame_pitch)) return rc;
    svs::ColourParams c{0, 0, bgr_row_pitch, bgr_frame_pitch, 0, 0, 0, 0};
    g.xcd_chunk = svs::kEighth;
    hipLaunchKernelGGL(svs::gray_to_bgr_kernel, dim3((uint32_t)((total + SVS_WG - 1) / SVS_WG)), dim3(SVS_WG), 0,
                       (hipStream_t)stream, d_gray, d_bgr, g, c);
    SVS_HIP(hipGetLastError());
    return SVS_OK;
}

static int colour_params(const svs_planes *p, const void *in, int64_t irp, int64_t ifp, const void *out, int64_t orp,
                         int64_t ofp, const uint32_t *weights, svs::ColourParams *c) {
    const void *ptrs[2] = {in, out};
    const int64_t rps[2] = {irp, orp}, fps[2] = {ifp, ofp};
    if (int rc = check_bgr_width(p)) return rc;
    for (int i = 0; i < 2; ++i) {
        if (i == 1 && !out) break;
        if (!ptrs[i] || ((uintptr_t)ptrs[i] % 8)) return fail(SVS_ERR_INVALID_ARG, "BGR pointer NULL or not 8-byte aligned");
        if (rps[i] < 3 * (int64_t)p->width || (rps[i] % 8) || fps[i] < rps[i] * p->height || (fps[i] % 8))
            return fail(SVS_ERR_INVALID_ARG, "BGR pitches must cover 3*width bytes per row and be multiples of 8");
    }
    const uint32_t dflt[4] = {3735u, 19235u, 9798u, 15u};
    const uint32_t *w = weights ? weights : dflt;
    if (int rc = check_weights(w)) return rc;
    c->in_row_pitch = irp; c->in_frame_pitch = ifp; c->out_row_pitch = orp; c->out_frame_pitch = ofp;
    c->wb = w[0]; c->wg = w[1]; c->wr = w[2]; c->shift = w[3];
    return SVS_OK;
}

constexpr uint32_t kBgrEmbedFlags = SVS_EXACT_POCKETFFT | SVS_EXACT_GUARDED | SVS_KEEP_COLOUR | SVS_NEAREST | SVS_MINMOVE;

// svs_embed_bgr_dev (allowed = kBgrEmbedFlags: SVS_READBACK is refused) and svs_embed_bgr_readback_dev (the flag accepted and
// implied; d_counts: the read-back counts, device, added to; NULL for none)
static int embed_bgr_dev(const uint8_t *d_bgr_in, int64_t in_row_pitch, int64_t in_frame_pitch, uint8_t *d_bgr_out,
                         int64_t out_row_pitch, int64_t out_frame_pitch, uint8_t *d_gray_ref, const svs_planes *planes,
                         const uint32_t *weights, double delta, int n_ac, const uint8_t *d_bits_packed, uint64_t bit_offset,
                         uint64_t n_bits, uint32_t flags, uint32_t allowed, uint64_t *n_embedded, uint64_t *d_counts, void *stream) {
    svs::Geometry g;
    uint64_t total = 0;
    if (int rc = make_geometry(planes, n_ac, &g, &total)) return rc;
    if (n_embedded) *n_embedded = 0;
    if (total == 0) return SVS_OK;
    if (flags & ~allowed) return fail(SVS_ERR_INVALID_ARG, "unknown flags 0x%x", flags);
    if (d_gray_ref && ((uintptr_t)d_gray_ref % 8)) return fail(SVS_ERR_INVALID_ARG, "gray pointer must be 8-byte aligned");
    if (d_counts && ((uintptr_t)d_counts % 8)) return fail(SVS_ERR_INVALID_ARG, "counts pointer must be 8-byte aligned");
    svs::ColourParams c;
    if (int rc = colour_params(planes, d_bgr_in, in_row_pitch, in_frame_pitch, d_bgr_out, out_row_pitch, out_frame_pitch,
                               weights, &c))
        return rc;
    if (!d_bgr_out) return fail(SVS_ERR_INVALID_ARG, "output pointer is NULL");
    svs::RouteArgs ra = route_args(delta, g, total, n_bits, bit_offset, flags, true);
    ra.readback = (allowed & SVS_READBACK) != 0;
    const svs::EmbedPlan p = svs::plan_embed(ra);
    if (p.use > 0 && (!d_bits_packed || ((uintptr_t)d_bits_packed % 4)))
        return fail(SVS_ERR_INVALID_ARG, "bits pointer NULL or not 4-byte aligned");
    if (p.use > 0 && bit_offset + p.use < bit_offset) return fail(SVS_ERR_INVALID_ARG, "bit_offset + n_bits overflows");
    if (p.n_words >= (1ull << 32)) return fail(SVS_ERR_INVALID_ARG, "payload too large for one call");
    if (int rc = launch_embed_bgr(p, (flags & SVS_KEEP_COLOUR) != 0, total, (hipStream_t)stream, d_bgr_in, d_bgr_out, d_gray_ref, g,
                                  c, p.use ? reinterpret_cast<const uint32_t *>(d_bits_packed) : nullptr, d_counts))
        return rc;
    if (n_embedded) *n_embedded = p.use;
    return SVS_OK;
}

int svs_embed_bgr_dev(const uint8_t *d_bgr_in, int64_t in_row_pitch, int64_t in_frame_pitch, uint8_t *d_bgr_out,
                      int64_t out_row_pitch, int64_t out_frame_pitch, uint8_t *d_gray_ref, const svs_planes *planes,
                      const uint32_t *weights, double delta, int n_ac, const uint8_t *d_bits_packed, uint64_t bit_offset,
                      uint64_t n_bits, uint32_t flags, uint64_t *n_embedded, void *stream) {
    return embed_bgr_dev(d_bgr_in, in_row_pitch, in_frame_pitch, d_bgr_out, out_row_pitch, out_frame_pitch, d_gray_ref, planes,
                         weights, delta, n_ac, d_bits_packed, bit_offset, n_bits, flags, kBgrEmbedFlags, n_embedded, nullptr, stream);
}

int svs_embed_bgr_readback_dev(const uint8_t *d_bgr_in, int64_t in_row_pitch, int64_t in_frame_pitch, uint8_t *d_bgr_out,
                               int64_t out_row_pitch, int64_t out_frame_pitch, uint8_t *d_gray_ref, const svs_planes *planes,
                               const uint32_t *weights, double delta, int n_ac, const uint8_t *d_bits_packed,
                               uint64_t bit_offset, uint64_t n_bits, uint32_t flags, uint64_t *n_embedded, uint64_t *d_counts,
                               void *stream) {
    return embed_bgr_dev(d_bgr_in, in_row_pitch, in_frame_pitch, d_bgr_out, out_row_pitch, out_frame_pitch, d_gray_ref, planes,
                         weights, delta, n_ac, d_bits_packed, bit_offset, n_bits, flags, kBgrEmbedFlags | SVS_READBACK, n_embedded,
                         d_counts, stream);
}

int svs_extract_bgr_dev(const uint8_t *d_bgr, int64_t bgr_row_pitch, int64_t bgr_frame_pitch, const svs_planes *planes,
                        const uint32_t *weights, double delta, int n_ac, uint8_t *d_bits_packed_out,
                        uint64_t out_capacity_bytes, uint64_t *n_bits_out, void *stream) {
    svs::Geometry g;
    uint64_t total = 0, cap = 0;
    if (int rc = extract_geometry(planes, n_ac, &g, &total, &cap, n_bits_out)) return rc;
    if (cap == 0) return SVS_OK;
    svs::ColourParams c;
    if (int rc = colour_params(planes, d_bgr, bgr_row_pitch, bgr_frame_pitch, nullptr, 0, 0, weights, &c)) return rc;
    if (!d_bits_packed_out || ((uintptr_t)d_bits_packed_out % 4)) return fail(SVS_ERR_INVALID_ARG, "bits pointer NULL or unaligned");
    const uint64_t bytes = (cap + 7) / 8;
    if (int rc = check_capacity(bytes, out_capacity_bytes, "bytes")) return rc;
    const svs::ExtractPlan p = svs::plan_extract(route_args(delta, g, total, 0, 0, 0, true));
    if (int rc = launch_extract_bgr(p, total, (hipStream_t)stream, d_bgr, g, c, d_bits_packed_out, bytes)) return rc;
    if (n_bits_out) *n_bits_out = cap;
    return SVS_OK;
}

static int packed_planes_only(const svs_planes *p) {
    if (p->row_pitch != p->width || p->frame_pitch != (int64_t)p->height * p->width)
        return fail(SVS_ERR_INVALID_ARG, "the host-pointer colour calls take tightly packed frames");
    return SVS_OK;
}

// svs_embed_bgr (counts NULL: SVS_READBACK is refused) and svs_embed_bgr_readback (counts: the read-back counts of the whole
// call, summed over the staging chunks as embed_host does)
static int embed_bgr_host(const uint8_t *bgr, uint8_t *bgr_out, uint8_t *gray_ref_out, const svs_planes *planes,
                          const uint32_t *weights, double delta, int n_ac, const uint8_t *bits_packed, uint64_t bit_offset,
                          uint64_t n_bits, uint32_t flags, uint64_t *n_embedded, svs_readback_counts *counts) {
    svs::Geometry g;
    uint64_t total = 0;
    if (int rc = make_geometry(planes, n_ac, &g, &total)) return rc;
    if (n_embedded) *n_embedded = 0;
    if (counts) *counts = svs_readback_counts{0, 0};
    if (total == 0) return SVS_OK;
    if (int rc = packed_planes_only(planes)) return rc;
    if (!bgr || !bgr_out) return fail(SVS_ERR_INVALID_ARG, "BGR pointer is NULL");
    const uint32_t allowed = kBgrEmbedFlags | (counts ? SVS_READBACK : 0u);
    if (flags & ~allowed) return fail(SVS_ERR_INVALID_ARG, "unknown flags 0x%x", flags);
    const uint64_t px = (uint64_t)planes->n_frames * planes->height * planes->width;
    const uint64_t cap = total * (uint64_t)g.n_ac;
    uint64_t use = n_bits < cap ? n_bits : cap;
    if (!(delta > 0.0)) use = 0;
    if (use && !bits_packed) return fail(SVS_ERR_INVALID_ARG, "bits pointer is NULL");
    if (use && bit_offset + use < bit_offset) return fail(SVS_ERR_INVALID_ARG, "bit_offset + n_bits overflows");
    const HostPayload payload{bits_packed, nullptr, bit_offset, use};
    uint64_t done_total = 0;
    // the read-back counts: two u64 in c.bits behind the payload, as in embed_host
    const size_t counts_at = (payload.bits_bytes() + 7) & ~(size_t)7;
    uint64_t got_counts[2] = {0, 0};
    if (int rc = staged(3 * px, 3 * px, gray_ref_out ? px : 0, counts ? counts_at + 16 : payload.bits_bytes(), [&](HostStage &c) {
            uint64_t rebased = 0;
            if (int rc = payload.stage(c, &rebased)) return rc;
            uint64_t *d_counts = counts ? reinterpret_cast<uint64_t *>(static_cast<uint8_t *>(c.bits.p) + counts_at) : nullptr;
            if (d_counts) SVS_HIP(hipMemsetAsync(d_counts, 0, 16, c.st[0]));
            uint8_t *d_in = static_cast<uint8_t *>(c.frames.p), *d_out = static_cast<uint8_t *>(c.second.p),
                    *d_ref = gray_ref_out ? static_cast<uint8_t *>(c.third.p) : nullptr;
            const int rc = embed_chunks(
                c, planes, 3, bgr, g.n_ac, use, n_bits, rebased,
                [&](const svs_planes &sub, int64_t off, int32_t, uint64_t chunk_offset, uint64_t budget, uint64_t *done, hipStream_t up) {
                    const int64_t rp = 3 * sub.row_pitch, fp = 3 * sub.frame_pitch;
                    return embed_bgr_dev(d_in + off, rp, fp, d_out + off, rp, fp, d_ref ? d_ref + off / 3 : nullptr, &sub, weights,
                                         delta, n_ac, static_cast<const uint8_t *>(c.bits.p), chunk_offset, budget, flags, allowed,
                                         done, d_counts, up);
                },
                [&](const svs::Chunk &ch, int64_t off, hipStream_t st) {   // tightly packed frames: every chunk is one run of bytes
                    const uint64_t n_px = (uint64_t)ch.nf * ch.rows * planes->width;
                    if (int rc = stage_d2h(st, bgr_out + off, d_out + off, 3 * n_px)) return rc;
                    return d_ref ? stage_d2h(st, gray_ref_out + off / 3, d_ref + off / 3, n_px) : (int)SVS_OK;
                },
                &done_total);
            if (!rc && d_counts) SVS_HIP(hipMemcpyAsync(got_counts, d_counts, 16, hipMemcpyDeviceToHost, c.st[0]));
            return rc;
        }))
        return rc;
    if (n_embedded) *n_embedded = done_total;
    if (counts) *counts = svs_readback_counts{got_counts[0], got_counts[1]};
    return SVS_OK;
}

int svs_embed_bgr(const uint8_t *bgr, uint8_t *bgr_out, uint8_t *gray_ref_out, const svs_planes *planes,
                  const uint32_t *weights, double delta, int n_ac, const uint8_t *bits_packed, uint64_t bit_offset,
                  uint64_t n_bits, uint32_t flags, uint64_t *n_embedded) {
    return embed_bgr_host(bgr, bgr_out, gray_ref_out, planes, weights, delta, n_ac, bits_packed, bit_offset, n_bits, flags,
                          n_embedded, nullptr);
}

int svs_embed_bgr_readback(const uint8_t *bgr, uint8_t *bgr_out, uint8_t *gray_ref_out, const svs_planes *planes,
                           const uint32_t *weights, double delta, int n_ac, const uint8_t *bits_packed, uint64_t bit_offset,
                           uint64_t n_bits, uint32_t flags, uint64_t *n_embedded, svs_readback_counts *counts) {
    svs_readback_counts none;
    return embed_bgr_host(bgr, bgr_out, gray_ref_out, planes, weights, delta, n_ac, bits_packed, bit_offset, n_bits, flags,
                          n_embedded, counts ? counts : &none);
}

int svs_extract_bgr(const uint8_t *bgr, const svs_planes *planes, const uint32_t *weights, double delta, int n_ac,
                    uint8_t *bits_packed_out, uint64_t out_capacity_bytes, uint64_t *n_bits_out) {
    svs::Geometry g;
    uint64_t total = 0, cap = 0;
    if (int rc = extract_geometry(planes, n_ac, &g, &total, &cap, n_bits_out)) return rc;
    if (cap == 0) return SVS_OK;
    if (int rc = packed_planes_only(planes)) return rc;
    if (!bgr || !bits_packed_out) return fail(SVS_ERR_INVALID_ARG, "BGR/bits pointer is NULL");
    const uint64_t bytes = (cap + 7) / 8;
    if (int rc = check_capacity(bytes, out_capacity_bytes, "bytes")) return rc;
    const uint64_t px = (uint64_t)planes->n_frames * planes->height * planes->width;
    const int64_t rp = 3 * (int64_t)planes->width, fp = rp * planes->height;
    return extract_staged(
        bgr, 3 * px, bytes, 0, n_bits_out,
        [&](const uint8_t *d_in, uint8_t *d_bits, uint64_t d_bytes, uint64_t *got, hipStream_t st) {
            return svs_extract_bgr_dev(d_in, rp, fp, planes, weights, delta, n_ac, d_bits, d_bytes, got, st);
        },
        [&](HostStage &c, hipStream_t st) { return stage_d2h(st, bits_packed_out, c.bits.p, bytes); });
}

int svs_fill_synthetic_dev(uint8_t *d_frames, const svs_planes *planes, uint32_t seed, uint32_t first_frame,
                           uint32_t lo, uint32_t span, void *stream) {
    svs::Geometry g;
    uint64_t total = 0;
    if (int rc = make_geometry(planes, 1, &g, &total)) return rc;
    if (total == 0) return SVS_OK;
    if (!d_frames || ((uintptr_t)d_frames % 8)) return fail(SVS_ERR_INVALID_ARG, "frames pointer NULL or unaligned");
    if (span == 0 || span > 256 || lo > 256 - span) return fail(SVS_ERR_INVALID_ARG, "need span >= 1 and lo + span <= 256");
    hipLaunchKernelGGL(svs::fill_synthetic_kernel, dim3(4096), dim3(256), 0, (hipStream_t)stream, d_frames,
                       planes->n_frames, planes->height, planes->width, planes->row_pitch, planes->frame_pitch, seed,
                       first_frame, lo, span);
    SVS_HIP(hipGetLastError());
    return SVS_OK;
}

int svs_fill_bits_dev(uint8_t *d_bits_packed, uint64_t n_bits, uint32_t seed, uint64_t first_bit, void *stream) {
    if (n_bits == 0) return SVS_OK;
    if (!d_bits_packed || ((uintptr_t)d_bits_packed % 4)) return fail(SVS_ERR_INVALID_ARG, "bits pointer NULL or unaligned");
    const uint64_t words = (n_bits + 31) / 32;
    const uint32_t blocks = (uint32_t)((words + 255) / 256 < 4096 ? (words + 255) / 256 : 4096);
    hipLaunchKernelGGL(svs::fill_bits_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<uint32_t *>(d_bits_packed), words, n_bits, seed, first_bit);
    SVS_HIP(hipGetLastError());
    return SVS_OK;
}

int svs_frame_sse_dev(const uint8_t *d_a, const uint8_t *d_b, const svs_planes *planes, uint64_t *d_sse, void *stream) {
    svs::Geometry g;
    uint64_t total = 0;
    if (int rc = make_geometry(planes, 1, &g, &total)) return rc;
    if (total == 0) return SVS_OK;
    if (!d_a || !d_b || !d_sse) return fail(SVS_ERR_INVALID_ARG, "NULL pointer");
    if (((uintptr_t)d_a % 8) || ((uintptr_t)d_b % 8) || ((uintptr_t)d_sse % 8))
        return fail(SVS_ERR_INVALID_ARG, "pointers must be 8-byte aligned");
    if (planes->n_frames > 65535) return fail(SVS_ERR_INVALID_ARG, "at most 65535 frames per call");
    const hipStream_t st = (hipStream_t)stream;
    SVS_HIP(hipMemsetAsync(d_sse, 0, sizeof(uint64_t) * (size_t)planes->n_frames, st));
    hipLaunchKernelGGL(svs::frame_sse_kernel, dim3(64, (uint32_t)planes->n_frames), dim3(256), 0, st, d_a, d_b,
                       planes->height, planes->width, planes->row_pitch, planes->frame_pitch,
                       reinterpret_cast<unsigned long long *>(d_sse));
    SVS_HIP(hipGetLastError());
    return SVS_OK;
}

uint64_t svs_ssim_workspace_bytes(const svs_planes *p) {
    if (!p || p->n_frames <= 0 || p->height < 7 || p->width < 7) return 0;
    const uint64_t gx = ((uint64_t)(p->width - 6) + 255) / 256, gy = ((uint64_t)(p->height - 6) + SVS_SSIM_BAND - 1) / SVS_SSIM_BAND;
    return (gx * gy + 2) * (uint64_t)p->n_frames * sizeof(double);   // partials + data_range + {min, max} per frame
}

int svs_frame_ssim_dev(const uint8_t *d_a, const uint8_t *d_b, const svs_planes *planes, const double *d_data_range,
                       double *d_ssim, void *d_workspace, void *stream) {
    svs::Geometry g;
    uint64_t total = 0;
    if (int rc = make_geometry(planes, 1, &g, &total)) return rc;
    if (total == 0) return SVS_OK;
    if (!d_a || !d_b || !d_ssim || !d_workspace) return fail(SVS_ERR_INVALID_ARG, "NULL pointer");
    if (((uintptr_t)d_a % 8) || ((uintptr_t)d_b % 8) || ((uintptr_t)d_data_range % 8) || ((uintptr_t)d_ssim % 8) ||
        ((uintptr_t)d_workspace % 8))
        return fail(SVS_ERR_INVALID_ARG, "pointers must be 8-byte aligned");
    if (planes->n_frames > 65535) return fail(SVS_ERR_INVALID_ARG, "at most 65535 frames per call");
    const hipStream_t st = (hipStream_t)stream;
    const uint32_t gx = (uint32_t)(((uint64_t)(planes->width - 6) + 255) / 256);
    const uint32_t gy = (uint32_t)(((uint64_t)(planes->height - 6) + SVS_SSIM_BAND - 1) / SVS_SSIM_BAND);
    double *partial = reinterpret_cast<double *>(d_workspace);
    double *range = partial + (uint64_t)gx * gy * planes->n_frames;
    if (!d_data_range) {
        // {min, max} per frame sit behind the ranges in the workspace: start from {0xffffffff, 0}
        uint32_t *lohi = reinterpret_cast<uint32_t *>(range + planes->n_frames);
        SVS_HIP(hipMemsetAsync(lohi, 0xff, sizeof(uint32_t) * 2 * (size_t)planes->n_frames, st));
        SVS_HIP(hipMemset2DAsync(lohi + 1, 2 * sizeof(uint32_t), 0, sizeof(uint32_t), (size_t)planes->n_frames, st));
        const uint32_t gr = (uint32_t)((planes->height + SVS_RANGE_ROWS - 1) / SVS_RANGE_ROWS);
        hipLaunchKernelGGL(svs::frame_minmax_kernel, dim3(gr, (uint32_t)planes->n_frames), dim3(256), 0, st, d_b,
                           planes->height, planes->width, planes->row_pitch, planes->frame_pitch, lohi);
        SVS_HIP(hipGetLastError());
        hipLaunchKernelGGL(svs::frame_range_finish_kernel, dim3((uint32_t)((planes->n_frames + 255) / 256)), dim3(256), 0, st,
                           lohi, planes->n_frames, range);
        SVS_HIP(hipGetLastError());
        d_data_range = range;
    }
    hipLaunchKernelGGL(svs::ssim_partial_kernel, dim3(gx, gy, (uint32_t)planes->n_frames), dim3(256), 0, st, d_a, d_b,
                       planes->height, planes->width, planes->row_pitch, planes->frame_pitch, d_data_range, partial);
    SVS_HIP(hipGetLastError());
    hipLaunchKernelGGL(svs::ssim_finish_kernel, dim3((uint32_t)planes->n_frames), dim3(64), 0, st, partial, (int32_t)(gx * gy),
                       (double)(planes->width - 6) * (double)(planes->height - 6), d_ssim);
    SVS_HIP(hipGetLastError());
    return SVS_OK;
}

int svs_bit_errors_dev(const uint8_t *d_a_packed, const uint8_t *d_b_packed, uint64_t n_bits, uint64_t *d_count,
                       void *stream) {
    if (!d_count || ((uintptr_t)d_count % 8)) return fail(SVS_ERR_INVALID_ARG, "count pointer NULL or unaligned");
    const hipStream_t st = (hipStream_t)stream;
    SVS_HIP(hipMemsetAsync(d_count, 0, sizeof(uint64_t), st));
    if (n_bits == 0) return SVS_OK;
    if (!d_a_packed || !d_b_packed) return fail(SVS_ERR_INVALID_ARG, "NULL pointer");
    const uint64_t bytes = (n_bits + 7) / 8;
    const uint32_t blocks = (uint32_t)((bytes + 255) / 256 < 2048 ? (bytes + 255) / 256 : 2048);
    hipLaunchKernelGGL(svs::bit_errors_kernel, dim3(blocks), dim3(256), 0, st, d_a_packed, d_b_packed, n_bits,
                       reinterpret_cast<unsigned long long *>(d_count));
    SVS_HIP(hipGetLastError());
    return SVS_OK;
}

#if defined(SVS_EXPERIMENTS)
// ---- measurement hooks: lib/variants/libsvsdct_exp.so ONLY (the product library exports exactly what include/svsdct.h declares,
// tests/test_capi_cpu.py::test_library_exports_exactly_the_declared_symbols) ----
// device counter (uint64, caller-zeroed) that guarded embed launches add the number of blocks they redid with the exact
// arithmetic to; NULL switches it off.  Process-global: single-threaded measurement use only.
int svs_guard_counter_set(void *d_counter) {
    g_guard_counter = reinterpret_cast<unsigned long long *>(d_counter);
    return SVS_OK;
}

// measurement hooks (not part of the product ABI): plain device copy / read streams, tools/ab_bench.py
int svs_ref_copy_dev(const void *d_src, void *d_dst, uint64_t bytes, int mode, void *stream) {
    const uint64_t n16 = bytes / 16;
    const hipStream_t st = (hipStream_t)stream;
    const auto *s = reinterpret_cast<const svs::u32x4 *>(d_src);
    auto *d = reinterpret_cast<svs::u32x4 *>(d_dst);
    if (mode == 8 || mode == 9) {   // 8: 16-byte loads + 8-byte stores, 9: 8-byte loads + 16-byte stores
        const dim3 grid((uint32_t)((bytes / 16 + 255) / 256));
        if (mode == 8) hipLaunchKernelGGL(svs::copy_mixed_kernel<1>, grid, dim3(256), 0, st, (const uint8_t *)d_src, (uint8_t *)d_dst, bytes);
        else hipLaunchKernelGGL(svs::copy_mixed_kernel<0>, grid, dim3(256), 0, st, (const uint8_t *)d_src, (uint8_t *)d_dst, bytes);
        SVS_HIP(hipGetLastError());
        return SVS_OK;
    }
    if (mode == 6 || mode == 7) {
        const uint64_t n8 = bytes / 8;
        const auto *s8 = reinterpret_cast<const svs::u32x2 *>(d_src);
        auto *d8 = reinterpret_cast<svs::u32x2 *>(d_dst);
        if (mode == 6) hipLaunchKernelGGL(svs::copy8_kernel<1>, dim3((uint32_t)((n8 + 255) / 256)), dim3(256), 0, st, s8, d8, n8);
        else hipLaunchKernelGGL(svs::copy8_kernel<0>, dim3((uint32_t)((n8 + 255) / 256)), dim3(256), 0, st, s8, d8, n8);
        SVS_HIP(hipGetLastError());
        return SVS_OK;
    }
    if (mode == 0) hipLaunchKernelGGL(svs::copy_kernel<0>, dim3((uint32_t)((n16 + 255) / 256)), dim3(256), 0, st, s, d, n16);
    else if (mode == 3) hipLaunchKernelGGL(svs::copy_kernel<3>, dim3((uint32_t)((n16 + 255) / 256)), dim3(256), 0, st, s, d, n16);
    else if (mode == 4) hipLaunchKernelGGL(svs::copy_kernel<4>, dim3((uint32_t)((n16 + 255) / 256)), dim3(256), 0, st, s, d, n16);
    else if (mode == 5) hipLaunchKernelGGL(svs::copy_kernel<5>, dim3((uint32_t)((n16 + 255) / 256)), dim3(256), 0, st, s, d, n16);
    else if (mode == 1) hipLaunchKernelGGL(svs::copy_kernel<1>, dim3(256 * 8), dim3(256), 0, st, s, d, n16);
    else hipLaunchKernelGGL(svs::copy_kernel<2>, dim3(256 * 8), dim3(256), 0, st, s, d, n16);
    SVS_HIP(hipGetLastError());
    return SVS_OK;
}

int svs_ref_read_dev(const void *d_src, void *d_sink, uint64_t bytes, void *stream) {
    hipLaunchKernelGGL(svs::read_kernel, dim3(256 * 8), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const svs::u32x4 *>(d_src), reinterpret_cast<uint32_t *>(d_sink), bytes / 16);
    SVS_HIP(hipGetLastError());
    return SVS_OK;
}

// test hook (not part of the product ABI): what v_cvt_pk_u8_f32 does on this device
int svs_probe_cvt_pk_u8(const float *host_in, uint32_t *host_out, int n) {
    if (n <= 0) return SVS_OK;
    DevBuf a, b;
    SVS_HIP(hipMalloc(&a.p, sizeof(float) * n));
    SVS_HIP(hipMalloc(&b.p, sizeof(uint32_t) * n));
    SVS_HIP(hipMemcpy(a.p, host_in, sizeof(float) * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(svs::probe_cvt_pk_u8_kernel, dim3((n + 63) / 64), dim3(64), 0, nullptr, (const float *)a.p,
                       (uint32_t *)b.p, n);
    SVS_HIP(hipGetLastError());
    SVS_HIP(hipMemcpy(host_out, b.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    return SVS_OK;
}
#endif  // SVS_EXPERIMENTS

}  // extern "C"
