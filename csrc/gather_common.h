// Pieces the batch gathers of the device-resident uint8 training set share
// (data_gather.hip, elastic_gather.hip): block geometry, the stateless
// Feistel permutation walk, the per-position keys, the 8-byte row staging,
// the integer bilinear tap and the LUT pack.  ops/cpu_ref.py holds the
// bit-identical reference of every one of them.
#pragma once

#include "common.h"

constexpr int GATHER_THREADS = 256;
// images per block: 2 x 98 units fill one pass of the 256 threads; measured
// best of {1,2,4,8,16} at B=64 and B=1024 (docs/KERNELS.md)
constexpr int GATHER_IPB = 2;
constexpr int ROW_BYTES = 784;          // 28*28 uint8 = 49 x 16 B
constexpr int ROW_UNITS = ROW_BYTES / 8;  // 98 units of 8 px per image
constexpr int SIDE = 28;

DEV uint32_t mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x85EBCA6Bu;
  x ^= x >> 13; x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

DEV uint32_t feistel_enc(uint32_t v, int h, uint32_t mask,
                         const uint32_t key[4]) {
  uint32_t L = v >> h, R = v & mask;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    uint32_t t = L ^ (mix32(R * 0x9E3779B1u + key[r]) & mask);
    L = R;
    R = t;
  }
  return (L << h) | R;
}

// sample index of batch position j at `step`: spe = N / B, epoch = step /
// spe, perm(epoch, (step % spe) * B + j); epoch 0 is the identity
DEV uint32_t gather_sample(uint32_t N, uint32_t B, int h, uint32_t key_base,
                           uint64_t step, uint32_t j) {
  const uint64_t spe = N / B;  // B <= N checked host-side, so spe >= 1
  const uint64_t epoch = step / spe;
  uint32_t v = (uint32_t)(step % spe) * B + j;  // < N
  if (epoch != 0) {
    const uint32_t mask = (1u << h) - 1u;
    uint32_t key[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      key[r] = mix32(key_base + (uint32_t)epoch * 0x9E3779B1u + r);
    // enc is a bijection on [0, 2^(2h)) and v starts below N, so the walk
    // returns below N (at the latest when the cycle closes)
    do {
      v = feistel_enc(v, h, mask, key);
    } while (v >= N);
  }
  return v;
}

// 32-bit key of batch position j at the full 64-bit `step`; `add` separates
// the users (cpu_ref.aug_indices: 0x632BE5AB, cpu_ref.elastic_key:
// 0x3C6EF372)
DEV uint32_t position_key(uint32_t key_base, uint32_t add, uint64_t step,
                          uint32_t j) {
  uint32_t k = mix32(key_base + add + (uint32_t)step * 0x9E3779B1u);
  k = mix32(k ^ mix32((uint32_t)(step >> 32) + 0x7F4A7C15u));
  return mix32(k + j * 0x85EBCA6Bu);
}

constexpr uint32_t AUG_ROW_ADD = 0x632BE5ABu;

// source rows of the block's images into LDS, one 8-byte unit per thread per
// pass; idx[im] < N, so the loads stay inside the resident set
DEV void stage_rows(const uint8_t* __restrict__ img, const uint32_t* idx,
                    uint8_t (*s_img)[ROW_BYTES], uint32_t j0, uint32_t B,
                    int tid) {
  for (int u = tid; u < GATHER_IPB * ROW_UNITS; u += GATHER_THREADS) {
    const int im = u / ROW_UNITS;
    const int unit = u - im * ROW_UNITS;
    if (j0 + im >= B) break;  // last partial block (u is monotonic in im)
    const uint8_t* src = img + (size_t)idx[im] * ROW_BYTES + unit * 8;
    *reinterpret_cast<uint2*>(&s_img[im][unit * 8]) =
        *reinterpret_cast<const uint2*>(src);
  }
}

DEV uint32_t aug_tap(const uint8_t* __restrict__ s, int y, int x) {
  // predicated to background 0 outside the image; never a clamped read
  return ((uint32_t)x < (uint32_t)SIDE && (uint32_t)y < (uint32_t)SIDE)
             ? (uint32_t)s[y * SIDE + x] : 0u;
}

DEV uint32_t aug_pixel(const uint8_t* __restrict__ s, uint32_t SX,
                       uint32_t SY) {
  const int sx = (int)SX, sy = (int)SY;
  const int x0 = sx >> 17, y0 = sy >> 17;  // arithmetic shift = floor
  const uint32_t fx = (uint32_t)(sx >> 9) & 255u;
  const uint32_t fy = (uint32_t)(sy >> 9) & 255u;
  const uint32_t top = aug_tap(s, y0, x0) * (256u - fx) +
                       aug_tap(s, y0, x0 + 1) * fx;
  const uint32_t bot = aug_tap(s, y0 + 1, x0) * (256u - fx) +
                       aug_tap(s, y0 + 1, x0 + 1) * fx;
  return (top * (256u - fy) + bot * fy + 32768u) >> 16;  // 0..255
}

// one Q17 source coordinate of flat output pixel p (< 784): a0 / a1 / t are
// a table row's (a00, a01, t0) for x, (a10, a11, t1) for y
DEV uint32_t aug_origin(uint32_t a0, uint32_t a1, uint32_t t, int p) {
  const int r = p / SIDE, c = p - r * SIDE;
  const uint32_t uc = (uint32_t)(2 * c - (SIDE - 1));
  const uint32_t ur = (uint32_t)(2 * r - (SIDE - 1));
  return ((SIDE - 1) << 16) + a0 * uc + a1 * ur + 2u * t;
}

// two pixel bytes -> two LUT entries in one dword of the 16-byte store
DEV uint32_t lut_pair(const unsigned short* s_lut, uint32_t v0, uint32_t v1) {
  return s_lut[v0] | ((uint32_t)s_lut[v1] << 16);
}

// step-independent launch parameters of the permuting gathers
static inline void gather_params(uint32_t N, uint64_t seed,
                                 uint32_t* key_base, int* h) {
  // host mirror of mix32
  auto hmix = [](uint32_t v) {
    v ^= v >> 16; v *= 0x85EBCA6Bu;
    v ^= v >> 13; v *= 0xC2B2AE35u;
    v ^= v >> 16;
    return v;
  };
  *key_base = hmix((uint32_t)seed ^ hmix((uint32_t)(seed >> 32) + 0x9E3779B9u));
  int bits = 0;
  for (uint32_t m = N - 1; m; m >>= 1) ++bits;
  if (bits < 2) bits = 2;
  bits += bits & 1;
  *h = bits / 2;
}
