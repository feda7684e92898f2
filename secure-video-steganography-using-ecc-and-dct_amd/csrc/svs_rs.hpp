// svs_rs.hpp - the per-step arithmetic of the Reed-Solomon outer code (include/svsrs.h and include/svsrse.h, "THE FORMAT"): the
// field, the generator, the encoder's LFSR, and the steps of an errors-and-erasures decoder - syndromes, the erasure locator,
// Berlekamp-Massey, root search, Forney - each as what ONE LANE does, in a form that compiles for the device
// (csrc/svs_rs_decode.hpp: a wave runs the lanes side by side) and for the host (svs_rs_encode; tests/hostemu/rs_emu.cpp runs the
// lanes one after the other).  What crosses lanes - the xor of the 64 discrepancy terms, the shift of B by one coefficient, the
// count of roots - is the caller's.  f is the number of a codeword's erased bytes; f = 0 is errors-only decoding.  Integers only.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SVS_RS_HD __host__ __device__ inline
#else
#define SVS_RS_HD inline
#endif

namespace svsrs {

constexpr int kParity = 32;                        // parity bytes a codeword: g(x) has the roots alpha^0 .. alpha^31
constexpr int kData = 223;                         // the most data bytes a codeword holds
constexpr int kT = 16;                             // bytes a codeword corrects
constexpr int kPoly = 0x11D;                       // x^8 + x^4 + x^3 + x^2 + 1
constexpr uint32_t kUncorrectable = 255;           // the status of a codeword that is left as received

// ---- the field: alpha = 0x02; exp2[i] = alpha^i for i = 0 .. 511 (twice round, so that a sum of two logarithms needs no
// reduction), log[alpha^i] = i ------------------------------------------------------------------------------------------------
struct Field {
    uint8_t exp2[512];
    uint8_t log[256];
};
constexpr Field make_field() {
    Field f{};
    uint32_t x = 1;
    for (int i = 0; i < 255; ++i) {
        f.exp2[i] = f.exp2[i + 255] = (uint8_t)x;
        f.log[x] = (uint8_t)i;
        x <<= 1;
        if (x & 0x100u) x ^= (uint32_t)kPoly;
    }
    f.exp2[510] = f.exp2[0];
    f.exp2[511] = f.exp2[1];
    return f;
}
constexpr uint8_t field_mul(const Field &f, uint32_t a, uint32_t b) { return a && b ? f.exp2[f.log[a] + f.log[b]] : (uint8_t)0; }

// g(x) = prod (x - alpha^i), i = 0 .. 31, without its leading 1: low[j] is the coefficient of x^(31 - j)
struct Generator {
    uint8_t low[kParity];
};
constexpr Generator make_generator(const Field &f) {
    uint8_t g[kParity + 1] = {1};                  // highest coefficient first
    for (int i = 0; i < kParity; ++i)
        for (int j = i + 1; j >= 1; --j) g[j] = (uint8_t)(g[j] ^ field_mul(f, f.exp2[i], g[j - 1]));
    Generator out{};
    for (int j = 0; j < kParity; ++j) out.low[j] = g[j + 1];
    return out;
}

// the LFSR's table: row[v] holds v * low[j], j = 0 .. 31, as eight words, byte j in bits 8 (j % 4) of word j / 4
struct LfsrTable {
    uint32_t row[256][kParity / 4];
};
constexpr LfsrTable make_lfsr(const Field &f, const Generator &g) {
    LfsrTable t{};
    for (int v = 0; v < 256; ++v)
        for (int j = 0; j < kParity; ++j) t.row[v][j / 4] |= (uint32_t)field_mul(f, (uint32_t)v, g.low[j]) << (8 * (j % 4));
    return t;
}

// the tables a lane reads: on the device copies in LDS, on the host the constants themselves
struct Gf {
    const uint8_t *exp2, *log;
    SVS_RS_HD uint32_t mul(uint32_t a, uint32_t b) const { return a && b ? exp2[log[a] + log[b]] : 0u; }
    // a / b, b != 0
    SVS_RS_HD uint32_t div(uint32_t a, uint32_t b) const { return a ? exp2[log[a] + 255u - log[b]] : 0u; }
};

// ---- sizes -------------------------------------------------------------------------------------------------------------------
SVS_RS_HD uint64_t codewords(uint64_t k) { return (k + kData - 1) / kData; }
SVS_RS_HD uint64_t coded_bytes(uint64_t k) { return k + (uint64_t)kParity * codewords(k); }
// the largest k with coded_bytes(k) <= total: whole codewords of 255, and what a last, shorter one holds beside its parity
SVS_RS_HD uint64_t data_bytes(uint64_t total) {
    const uint64_t left = total % 255u;
    return total / 255u * kData + (left > (uint64_t)kParity ? left - kParity : 0u);
}

// ---- the LFSR: w holds the 32 remainder bytes, byte j (the coefficient of x^(31 - j), parity byte p_j) in bits 8 (j % 4) of
// word j / 4.  One step takes the next data byte: r(x) <- (r(x) x + d x^32) mod g(x) ------------------------------------------------
SVS_RS_HD void lfsr_step(uint32_t *w, uint32_t byte, const uint32_t *table) {
    const uint32_t *row = table + 8u * ((w[0] & 0xFFu) ^ byte);
    for (int i = 0; i < 7; ++i) w[i] = ((w[i] >> 8) | (w[i + 1] << 24)) ^ row[i];
    w[7] = (w[7] >> 8) ^ row[7];
}

// ---- the decoder's steps.  r: the 32 bytes of r(x) = c(x) mod g(x), r[j] the coefficient of x^(31 - j).  f <= 32 bytes of the
// codeword are erased, at the positions p_0 .. p_(f - 1) (position p: the byte that multiplies x^p), X_t = alpha^(p_t); f = 0: errors
// only, and every step below is that of a bounded-distance decoder for up to kT errors ----------------------------------------------
// lane j = 0 .. 31: S_j = r(alpha^j)
SVS_RS_HD uint32_t syndrome(int j, const uint8_t *r, const Gf &gf) {
    uint32_t s = 0;
    int e = 0;                                     // j m mod 255
    for (int m = 0; m < kParity; ++m) {
        const uint32_t v = r[kParity - 1 - m];
        if (v) s ^= gf.exp2[gf.log[v] + e];
        e += j;
        if (e >= 255) e -= 255;
    }
    return s;
}

// the erasure locator Gamma(x) = prod (1 - X_t x), lane i holds Gamma_i.  Start: Gamma = 1.  One step per erased position:
// Gamma <- Gamma (1 - X x); `below` is Gamma_(i - 1) before the step, 0 on lane 0
SVS_RS_HD uint32_t gamma_step(uint32_t gamma, uint32_t below, int p, const Gf &gf) { return gamma ^ gf.mul(gf.exp2[p], below); }

// Berlekamp-Massey, lane i holds Lambda_i and coefficient i of x^m B(x).  Step n = f .. 31:
//   d = the xor over the lanes of bm_term;  d = 0: nothing but the shift of B.
//   d != 0: Lambda <- Lambda - (d / b) x^m B;  when bm_longer (2 L <= n + f) also B <- the Lambda before, b <- d,
//   L <- bm_length (n + 1 - L + f), and the codeword is given up when bm_beyond: L - f errors and f erasures, 2 (L - f) + f > 32.
//   Then B is shifted up by one coefficient: lane i takes `pass` of lane i - 1, lane 0 takes 0.
// Start: Lambda = Gamma, x^m B = x Gamma, L = f, b = 1.  f = 0: Lambda = 1, x^m B = x, L = 0; longer when 2 L <= n, L <- n + 1 - L,
// given up when L > kT.
SVS_RS_HD uint32_t bm_term(int i, int n, uint32_t lambda, const uint8_t *syn, const Gf &gf) { return i <= n ? gf.mul(lambda, syn[n - i]) : 0u; }
SVS_RS_HD bool bm_longer(uint32_t d, int L, int n, int f) { return d != 0 && 2 * L <= n + f; }
SVS_RS_HD int bm_length(int L, int n, int f) { return n + 1 - L + f; }
SVS_RS_HD bool bm_beyond(int L, int f) { return 2 * L - f > kParity; }
struct BmLane {
    uint32_t lambda, pass;
};
SVS_RS_HD BmLane bm_update(uint32_t lambda, uint32_t shifted_b, uint32_t d, uint32_t b, bool longer, const Gf &gf) {
    if (d == 0) return BmLane{lambda, shifted_b};
    return BmLane{lambda ^ gf.mul(gf.div(d, b), shifted_b), longer ? lambda : shifted_b};
}

// lane j = 0 .. 31: Omega_j = sum over i <= j of Lambda_i S_(j - i): Omega = S Lambda mod x^32, with degree = L <= 32
SVS_RS_HD uint32_t omega_coefficient(int j, int degree, const uint8_t *lambda, const uint8_t *syn, const Gf &gf) {
    uint32_t o = 0;
    for (int i = 0; i <= j && i <= degree; ++i) o ^= gf.mul(lambda[i], syn[j - i]);
    return o;
}

// sum of coef[i] z^(i - from) over i = from, from + stride, .. <= to, at z = alpha^zlog (zlog = 0 .. 254, stride 1 or 2)
SVS_RS_HD uint32_t evaluate(const uint8_t *coef, int from, int to, int stride, int zlog, const Gf &gf) {
    uint32_t acc = 0;
    int e = 0;
    for (int i = from; i <= to; i += stride) {
        if (coef[i]) acc ^= gf.exp2[gf.log[coef[i]] + e];
        e += zlog;
        if (e >= 255) e -= 255;
    }
    return acc;
}

// the map of a codeword's erased positions, 256 bits in eight words
SVS_RS_HD uint32_t erased_word(int p) { return (uint32_t)p >> 5; }
SVS_RS_HD uint32_t erased_bit(int p) { return 1u << (p & 31); }
SVS_RS_HD bool is_erased(const uint32_t *map, int p) { return (map[erased_word(p)] & erased_bit(p)) != 0; }

// the lane of position p (X = alpha^p), degree = L <= 32: is X^-1 a root of Lambda, and if so the value
//   e = X Omega(X^-1) / Lambda'(X^-1),   Lambda'(z) = sum over odd i of Lambda_i z^(i - 1).
// Returns 0: no root at a position that is not erased; 1 .. 255: the value to xor into the byte; kRightErasure: a root at an
// erased position whose value is 0, the byte was right; kBadRoot: an erased position that is no root, a zero derivative at a
// root, or a zero value at a root that is not erased.  With no erased position the number of non-zero returns of a codeword that
// decodes is L.
constexpr uint32_t kBadRoot = 256;
constexpr uint32_t kRightErasure = 257;
SVS_RS_HD uint32_t errata_value(int p, int degree, const uint8_t *lambda, const uint8_t *omega, bool erased, const Gf &gf) {
    const int zlog = p ? 255 - p : 0;
    if (evaluate(lambda, 0, degree, 1, zlog, gf) != 0) return erased ? kBadRoot : 0u;
    const int z2 = 2 * zlog >= 255 ? 2 * zlog - 255 : 2 * zlog;
    const uint32_t slope = evaluate(lambda, 1, degree, 2, z2, gf);
    if (slope == 0) return kBadRoot;
    const uint32_t top = evaluate(omega, 0, degree - 1, 1, zlog, gf);
    if (top == 0) return erased ? kRightErasure : kBadRoot;
    return gf.mul(gf.exp2[p], gf.div(top, slope));
}
// f = 0 under the name host emulations written before the mask call it by: the same steps, no second set of them
SVS_RS_HD uint32_t root_value(int p, int degree, const uint8_t *lambda, const uint8_t *omega, const Gf &gf) {
    return errata_value(p, degree, lambda, omega, false, gf);
}

// where byte i of codeword c (i < k_c: data byte d_i, otherwise parity byte p_(i - k_c)) lies in a stream of k data bytes
// interleaved over C codewords
SVS_RS_HD uint64_t stream_offset(uint64_t k, uint64_t C, uint64_t c, uint32_t k_c, uint32_t i) {
    return i < k_c ? (uint64_t)i * C + c : k + (uint64_t)(i - k_c) * C + c;
}

}  // namespace svsrs
