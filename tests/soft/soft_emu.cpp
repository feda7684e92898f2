// soft_emu.cpp - TEST INFRASTRUCTURE ONLY (never loaded by the product package).
//
// The soft side of extract_exact_kernel on the CPU, block by block, through the plain-C++ headers of csrc/: the routing of a
// soft call (svs_route.hpp plan_extract), the tables and SoftArgs its launch passes (extract_tables) and the block body
// (svs_block.hpp extract_block_soft), with the bytes placed where the kernel's tail places them - block b of frame f owns the
// n bytes at (f N + slot(b)) n, slot(b) = b without an order.  The wave tile, the LDS and the coalesced copy are NOT modelled
// here; the -m gpu tests cover them.  tests/soft_lib.py builds and loads it; tests/hostemu stays as it is.
// Build: g++ -O2 -ffp-contract=off -std=c++17 -shared -fPIC -I<csrc> soft_emu.cpp -o libsvs_soft_emu.so
#include <cstdint>
#include <cstring>
#include <type_traits>

#include "svs_block.hpp"
#include "svs_index.hpp"
#include "svs_order.hpp"
#include "svs_route.hpp"

namespace {

struct SoftCall {
    svs::CoeffTable table;    // of the call's selection, when one is given
    svs::RouteArgs route;
    uint32_t n;
    bool given;
};

// -> false: a selection the library refuses
bool make_call(double delta, int n_ac, const uint8_t *index, int count, int dither, int order, int pocketfft, int guarded,
               uint64_t total, SoftCall &c) {
    c.given = count > 0;
    c.n = c.given ? (uint32_t)count : (uint32_t)(n_ac < 0 ? 0 : (n_ac > 63 ? 63 : n_ac));   // as the library clamps it
    if (c.given && !svs::make_coeff_table(index, (uint32_t)count, &c.table)) return false;
    c.route = svs::RouteArgs{delta, c.n, total, 0, 0, pocketfft != 0, guarded != 0, false, false, 1.0f, 1.0f};
    c.route.keyed = order != 0;
    c.route.dithered = dither != 0;
    c.route.soft = true;
    if (c.given) c.route.coeffs = &c.table;
    return true;
}

}  // namespace

extern "C" {

// the plan of a soft call -> out[7] = {path, rows, qm, selected, dithered, soft, keyed}; -1: the selection is refused
int soft_emu_plan(double delta, int n_ac, const uint8_t *index, int count, int dither, int order, int pocketfft, int guarded,
                  uint64_t total_blocks, int32_t *out) {
    SoftCall c;
    if (!make_call(delta, n_ac, index, count, dither, order, pocketfft, guarded, total_blocks, c)) return -1;
    const svs::ExtractPlan p = svs::plan_extract(c.route);
    const int32_t v[7] = {(int32_t)p.path, p.rows, p.qm, p.selected, p.dithered, p.soft, p.keyed};
    std::memcpy(out, v, sizeof v);
    return 0;
}

// frames: contiguous [F][H][W]; soft_out: F (H/8) (W/8) n bytes.  -> the capacity, or ~0 when the selection is refused
uint64_t soft_emu_extract(const uint8_t *frames, int F, int H, int W, double delta, int n_ac, const uint8_t *index, int count,
                          int dither, uint64_t dither_key, int order, uint64_t order_key, uint32_t first_frame, uint8_t *soft_out) {
    const uint64_t wb = (uint64_t)W / 8, bpf = wb * ((uint64_t)H / 8), total = bpf * (uint64_t)F;
    SoftCall c;
    if (!make_call(delta, n_ac, index, count, dither, order, 0, 0, total, c)) return ~0ull;
    const uint32_t n = c.n;
    const uint64_t cap = total * n;
    const svs::ExtractPlan p = svs::plan_extract(c.route);
    if (cap == 0) return 0;
    if (p.path == svs::ExtractPath::ZEROS) {
        std::memset(soft_out, 0, (size_t)cap);
        return cap;
    }
    svs::KernelOptions k{};
    k.ord = svs::make_block_order(order_key, first_frame, (uint32_t)bpf);
    k.coeffs = c.route.coeffs;
    k.dith = svs::DitherArgs{svs::dither_seed(dither_key), first_frame, 1u, svs::CoeffTable{}};
    const svs::LaunchTables t = svs::extract_tables(p, k);   // what the soft launch passes
    auto walk = [&](auto qm) {
        constexpr int QM = decltype(qm)::value;
        for (uint64_t gb = 0; gb < total; ++gb) {
            const uint64_t f = gb / bpf, b = gb % bpf;
            const uint8_t *px = frames + f * (uint64_t)H * W + (b / wb) * 8 * (uint64_t)W + (b % wb) * 8;
            uint32_t rx[8], ry[8];
            for (int r = 0; r < 8; ++r) {
                std::memcpy(&rx[r], px + r * (size_t)W, 4);
                std::memcpy(&ry[r], px + r * (size_t)W + 4, 4);
            }
            const uint64_t slot = p.keyed ? svs::block_to_slot((uint32_t)b, k.ord, svs::round_keys(k.ord, first_frame + (uint32_t)f)) : b;
            uint8_t *mine = soft_out + (f * bpf + slot) * n;
            const uint32_t s_b = svs::dither_block_seed(t.dith.seed, t.dith.first_frame + (uint32_t)f, (uint32_t)b);
            svs::extract_block_soft<QM>(rx, ry, t.dith.sel, p.qp, t.soft, t.dith.on != 0u, s_b,
                                        [&](uint32_t s, uint32_t byte) { mine[s] = (uint8_t)byte; });
        }
    };
    // the plan names QM_F32 or QM_POW2, as for every extract launch
    if (p.qm == svs::QM_POW2) walk(std::integral_constant<int, svs::QM_POW2>{});
    else walk(std::integral_constant<int, svs::QM_F32>{});
    return cap;
}

}  // extern "C"
