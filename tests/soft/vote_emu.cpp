// vote_emu.cpp - TEST INFRASTRUCTURE ONLY (never loaded by the product package).
//
// The integer side of the fused soft vote on the CPU, through the plain-C++ headers of csrc/: the arguments a vote launch
// passes (svs_block.hpp make_vote_args, through svs_route.hpp extract_tables as the launch calls it), the residue of a
// call-local bit (vote_residue: a double-precision quotient with one correction, no 64-bit division) and a byte's vote
// (vote_of).  The wave tile, the pre-reduction and the atomics are NOT modelled here; the -m gpu tests cover them.
// tests/soft_vote_lib.py builds and loads it; tests/soft/soft_emu.cpp and tests/hostemu stay as they are.
// Build: g++ -O2 -ffp-contract=off -std=c++17 -shared -fPIC -I<csrc> vote_emu.cpp -o libsvs_vote_emu.so
#include <cstdint>

#include "svs_block.hpp"
#include "svs_index.hpp"
#include "svs_order.hpp"
#include "svs_route.hpp"

namespace {

svs::SoftArgs vote_args(double delta, uint32_t n_ac, uint64_t period, uint64_t stream_bit0, int32_t *plan_out) {
    svs::RouteArgs ra{delta, n_ac, 1000, 0, 0, false, false, false, false, 1.0f, 1.0f};
    ra.vote = true;
    const svs::ExtractPlan p = svs::plan_extract(ra);
    svs::KernelOptions k{};
    k.vote_period = period;
    k.vote_bit0 = stream_bit0;
    if (plan_out) {
        plan_out[0] = (int32_t)p.path;
        plan_out[1] = p.rows;
        plan_out[2] = p.soft;
        plan_out[3] = p.vote;
    }
    return svs::extract_tables(p, k).soft;
}

}  // namespace

extern "C" {

// out[4] = {path, rows, soft, vote} of a vote call's plan; fields[4] = {vote, period, base, head} of its SoftArgs
void vote_emu_args(double delta, uint32_t n_ac, uint64_t period, uint64_t stream_bit0, int32_t *plan_out, uint64_t *fields) {
    const svs::SoftArgs sa = vote_args(delta, n_ac, period, stream_bit0, plan_out);
    fields[0] = sa.vote;
    fields[1] = sa.period;
    fields[2] = sa.base;
    fields[3] = sa.head;
}

// residues[k] = (stream_bit0 + i[k]) mod period as the kernel takes it, in_head[k] = whether the bit lies in copy 0
void vote_emu_residues(uint64_t period, uint64_t stream_bit0, const uint64_t *i, uint64_t count, uint64_t *residues, uint8_t *in_head) {
    const svs::SoftArgs sa = vote_args(20.0, 10, period, stream_bit0, nullptr);
    for (uint64_t k = 0; k < count; ++k) {
        residues[k] = svs::vote_residue(i[k], sa);
        in_head[k] = i[k] < sa.head;
    }
}

int32_t vote_emu_vote(uint32_t byte, int in_head) { return svs::vote_of(byte, in_head != 0); }

uint64_t vote_emu_period_max(void) { return svs::kVotePeriodMax; }

}  // extern "C"
