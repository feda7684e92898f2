// svs_order.hpp - the keyed block order (svs_embed_ordered* / svs_extract_ordered*, include/svsdct.h): a key-seeded permutation
// of the blocks of each frame, so that a payload that fills only part of a frame's capacity is spread over the whole frame
// instead of filling its top rows.  Plain C++ (host and device): csrc/svs_device.hpp applies it in the kernels,
// tests/block_order builds it for the CPU tier, svsdct/order.py restates it in NumPy.
//
// NOT a cryptographic permutation.  It hides WHERE the payload sits from a look at the frame (a frame difference, a PSNR of one
// band against the rest); the payload's confidentiality comes from the AES-GCM encryption on the host.  The order is a format:
// sender and receiver must compute the same one, so nothing here may change.
//
// N = blocks per frame.  sigma_t(j) = block of frame t that takes stream slot j (slot j = stream bits j*n .. j*n+n-1 of the
// frame's range); sigma_t^-1(i) = slot of block i.  N == 1: the identity.  Otherwise a four-round unbalanced Feistel network E
// on [0, 2^k), k = max(2, ceil(log2 N)), split into h (the high a = k - b bits) and l (the low b = k >> 1 bits), with cycle
// walking into [0, N): y = E(j), repeated while y >= N.  Round keys (all arithmetic mod 2^32, lb = lowbias32):
//   s = lb(hi32(key) ^ 0x9E3779B9); s = lb(s ^ lo32(key)); s = lb(s ^ t);  K_r = lb(s + (r + 1) * 0x632BE5AB), r = 0..3
//   round r even: l ^= lb(h ^ K_r) & (2^b - 1);  odd: h ^= lb(l ^ K_r) & (2^a - 1)
// E applies rounds 0, 1, 2, 3 and D = E^-1 rounds 3, 2, 1, 0 (each round undoes itself).  2^k < 2N, so a walk is short: 1.01
// steps on average at 1080p and 4K, 1.71 at 640 x 480.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SVS_ORDER_HD __host__ __device__ __forceinline__
#else
#define SVS_ORDER_HD inline
#endif

namespace svs {

// the public-domain "lowbias32" integer finaliser (also the hash of svsdct/synth.py and the synthetic-content kernels)
SVS_ORDER_HD uint32_t lowbias32(uint32_t h) {
    h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16;
    return h;
}

// what the order of one call needs besides the frame index: the key folded to 32 bits, the clip index of the call's first
// frame, and the Feistel domain of N blocks per frame (kernel argument of the KEYED instantiations)
struct BlockOrderArgs {
    uint32_t seed;          // lb(lb(hi32(key) ^ 0x9E3779B9) ^ lo32(key))
    uint32_t first_frame;   // frame f of the call uses t = first_frame + f
    uint32_t n_blocks;      // N
    uint32_t b;             // bits of the low half l
    uint32_t mask_l, mask_h;
};

SVS_ORDER_HD BlockOrderArgs make_block_order(uint64_t key, uint32_t first_frame, uint32_t n_blocks) {
    BlockOrderArgs o;
    o.seed = lowbias32(lowbias32((uint32_t)(key >> 32) ^ 0x9E3779B9u) ^ (uint32_t)key);
    o.first_frame = first_frame;
    o.n_blocks = n_blocks;
    uint32_t k = 0;
    while (k < 32 && (1ull << k) < n_blocks) ++k;   // ceil(log2 N)
    if (k < 2) k = 2;
    o.b = k >> 1;
    o.mask_l = (1u << o.b) - 1u;
    o.mask_h = (1u << (k - o.b)) - 1u;
    return o;
}

struct RoundKeys {
    uint32_t k[4];
};

// the round keys of clip frame t
SVS_ORDER_HD RoundKeys round_keys(const BlockOrderArgs &o, uint32_t t) {
    const uint32_t s = lowbias32(o.seed ^ t);
    RoundKeys rk;
    for (uint32_t r = 0; r < 4; ++r) rk.k[r] = lowbias32(s + (r + 1u) * 0x632BE5ABu);
    return rk;
}

SVS_ORDER_HD uint32_t feistel_round(uint32_t x, const BlockOrderArgs &o, uint32_t key, bool even) {
    uint32_t h = x >> o.b, l = x & o.mask_l;
    if (even) l ^= lowbias32(h ^ key) & o.mask_l;
    else h ^= lowbias32(l ^ key) & o.mask_h;
    return (h << o.b) | l;
}

SVS_ORDER_HD uint32_t feistel_e(uint32_t x, const BlockOrderArgs &o, const RoundKeys &rk) {
    x = feistel_round(x, o, rk.k[0], true);
    x = feistel_round(x, o, rk.k[1], false);
    x = feistel_round(x, o, rk.k[2], true);
    return feistel_round(x, o, rk.k[3], false);
}

SVS_ORDER_HD uint32_t feistel_d(uint32_t x, const BlockOrderArgs &o, const RoundKeys &rk) {
    x = feistel_round(x, o, rk.k[3], false);
    x = feistel_round(x, o, rk.k[2], true);
    x = feistel_round(x, o, rk.k[1], false);
    return feistel_round(x, o, rk.k[0], true);
}

// sigma_t(j): the block that takes slot j (j < N)
SVS_ORDER_HD uint32_t slot_to_block(uint32_t j, const BlockOrderArgs &o, const RoundKeys &rk) {
    if (o.n_blocks <= 1) return j;
    uint32_t y = feistel_e(j, o, rk);
    while (y >= o.n_blocks) y = feistel_e(y, o, rk);
    return y;
}

// sigma_t^-1(i): the slot of block i (i < N)
SVS_ORDER_HD uint32_t block_to_slot(uint32_t i, const BlockOrderArgs &o, const RoundKeys &rk) {
    if (o.n_blocks <= 1) return i;
    uint32_t y = feistel_d(i, o, rk);
    while (y >= o.n_blocks) y = feistel_d(y, o, rk);
    return y;
}

}  // namespace svs
