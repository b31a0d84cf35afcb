// Counter-based dropout masks: the keep bits of models.py:60-61 (one nn.Dropout call over cat(h, ah * norm)) and :105-113
// (the model's nn.Dropout on the input features), drawn from Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy
// as 1, 2, 3", SC 2011) so that any kernel can regenerate any element's bit from its coordinates alone.
//
//   keep(seed, rank, step, site, row, col) = philox4x32_10(ctr, key)[col % 4] >= thr,   thr = round(p 2^32) (clamped)
//   ctr = {col / 4, row, step, site}         step: completed optimiser steps (the plan's device step counter)
//   key = {seed_lo, seed_hi ^ rank 0x9E3779B9}  site: 0 = input dropout, i + 1 = hidden layer i;  row: position in the batch
//
// The bits depend on these arguments only -- not on a tile, a grid or a kernel: the forward producer, the backward consumer and
// the test hook (gte_dropout_mask / gte_dropout_mask_host) agree by construction, and no mask is ever stored.  A kept element is
// v * scale with scale = fp32(1 / (1 - p)), computed in fp32 (D_s(v) of the layer docs).  p = 0 never reaches this code.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define GTE_DROP_HD __host__ __device__ __forceinline__
#else
#define GTE_DROP_HD inline
#endif

namespace dropout {

struct Key { uint32_t k0, k1; };

GTE_DROP_HD Key make_key(uint64_t seed, int rank) {
    return Key{(uint32_t)seed, (uint32_t)(seed >> 32) ^ ((uint32_t)rank * 0x9E3779B9u)};
}

// keep iff u32 >= thr: thr = round(p 2^32), clamped to [0, 2^32 - 1] (P(keep) = 1 - p up to 2^-32)
inline uint32_t threshold(double p) {
    double t = p * 4294967296.0 + 0.5;
    if (!(t > 0.0)) return 0u;
    if (t >= 4294967295.0) return 0xffffffffu;
    return (uint32_t)t;
}
inline float scale(double p) { return (float)(1.0 / (1.0 - p)); }

// Philox4x32 with 10 rounds (the Random123 reference constants).  Known answer: ctr = key = 0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8.
GTE_DROP_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, Key key, uint32_t (&out)[4]) {
    uint32_t k0 = key.k0, k1 = key.k1;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// keep bits of the four columns col0 .. col0 + 3 of one row (bit j = column col0 + j): one Philox call when col0 % 4 == 0, two
// otherwise (the second half of a [self | agg] mask starts at column fin, which need not be a multiple of 4)
GTE_DROP_HD unsigned keep4(Key key, uint32_t thr, uint32_t step, uint32_t site, uint32_t row, uint32_t col0) {
    uint32_t u[4];
    philox4x32_10(col0 >> 2, row, step, site, key, u);
    const unsigned s = col0 & 3u;
    const unsigned lo = (unsigned)(u[0] >= thr) | ((unsigned)(u[1] >= thr) << 1) | ((unsigned)(u[2] >= thr) << 2) |
                        ((unsigned)(u[3] >= thr) << 3);
    if (s == 0) return lo;
    philox4x32_10((col0 >> 2) + 1, row, step, site, key, u);
    const unsigned hi = (unsigned)(u[0] >= thr) | ((unsigned)(u[1] >= thr) << 1) | ((unsigned)(u[2] >= thr) << 2) |
                        ((unsigned)(u[3] >= thr) << 3);
    return ((lo | (hi << 4)) >> s) & 15u;        // (shifts, not a register array indexed at run time)
}

}  // namespace dropout
