// hist_emu.cpp - TEST INFRASTRUCTURE ONLY (never loaded by the product package).
//
// The integer side of the fused per-frame soft histograms on the CPU, through the plain-C++ headers of csrc/: the plan and the
// arguments a histogram launch passes (svs_route.hpp plan_extract / extract_tables as the launch calls them) and the split of
// a run of blocks into per-frame runs (svs_index.hpp frame_run, walked over the frames of a workgroup exactly as the kernel's
// histogram tail walks them).  The LDS table, the barriers and the atomics are NOT modelled here; the -m gpu tests cover them.
// tests/soft_histogram_lib.py builds and loads it; the other host builds stay as they are.
// Build: g++ -O2 -ffp-contract=off -std=c++17 -shared -fPIC -I<csrc> hist_emu.cpp -o libsvs_hist_emu.so
#include <cstdint>

#include "svs_block.hpp"
#include "svs_index.hpp"
#include "svs_order.hpp"
#include "svs_route.hpp"

extern "C" {

// plan_out[6] = {path, rows, soft, vote, hist, keyed} of a histogram call's plan (asked for with an order when `keyed`: a
// histogram plan never is); fields[3] = {on, vote, hist} of its SoftArgs; returns sizeof(SoftArgs)
uint64_t hist_emu_args(double delta, uint32_t n_ac, int keyed, int32_t *plan_out, uint32_t *fields) {
    svs::RouteArgs ra{delta, n_ac, 1000, 0, 0, false, false, false, false, 1.0f, 1.0f};
    ra.hist = true;
    ra.keyed = keyed != 0;
    const svs::ExtractPlan p = svs::plan_extract(ra);
    plan_out[0] = (int32_t)p.path;
    plan_out[1] = p.rows;
    plan_out[2] = p.soft;
    plan_out[3] = p.vote;
    plan_out[4] = p.hist;
    plan_out[5] = p.keyed;
    const svs::SoftArgs sa = svs::extract_tables(p, svs::KernelOptions{}).soft;
    fields[0] = sa.on;
    fields[1] = sa.vote;
    fields[2] = sa.hist;
    return sizeof(svs::SoftArgs);
}

// The per-frame runs of the wave whose first block is wave_first, in a workgroup whose first block is wg_first, of a call of
// `total` blocks at bpf blocks per frame - the loop of hist_soft_run: for every frame the workgroup touches, the wave's part.
// out: triples {frame, begin, end} (positions within the wave's run), one per frame of the WORKGROUP, empty parts included;
// returns their number (at most `room`).
uint32_t hist_emu_runs(uint32_t wg_first, uint32_t wg_size, uint32_t wave_first, uint32_t total, uint32_t bpf, uint32_t *out,
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

uint32_t hist_emu_bins(void) { return svs::kHistBins; }

}  // extern "C"
