// MXFP8 gradient wire (--grad_dtype mxfp8; docs/KERNELS.md "MXFP8 gradient
// wire").  OCP microscaling: blocks of 32 e4m3 codes with one E8M0 scale byte,
// packed and unpacked by gfx950's v_cvt_scalef32_pk_fp8_f32 /
// v_cvt_scalef32_pk_f32_fp8.  ops/cpu_ref.py::mx_encode / mx_decode /
// mx_reduce are the contract: every kernel here equals them bit for bit.
//
// Wire layout: W shards of sb blocks (sb a multiple of 16), shard w = the
// 32 * sb code bytes of blocks [w * sb, (w + 1) * sb) of the bucket, then
// their sb scale bytes; 33 * sb bytes, a multiple of 16.
//   mx_encode_kernel  lane = 8 consecutive floats (two 16 B loads), four
//                     lanes = one block.  Block amax over the quad by DPP
//                     quad_perm, the scale byte from amax's exponent and
//                     mantissa bits, stochastic rounding onto the e4m3 grid in
//                     integer arithmetic, the on-grid values packed by the
//                     hardware conversion (exact on them, unit scale: the
//                     kernel has already scaled, so fp32 subnormals cost
//                     nothing), one 8 B code store per lane, the scale bytes
//                     of four blocks gathered by lane permutes into one 4 B
//                     store.  Padding blocks are written too (zeros).
//   mx_reduce_kernel  lane = half a block (one 16 B code load per row), W
//                     rows decoded by the hardware conversion with the row's
//                     scale and added in fp32 registers in rank order; block
//                     amax over the lane pair, re-encoded as above (stage 1),
//                     one 16 B code store per lane.  The sum never reaches
//                     memory.
//   mx_decode_kernel  lane = 8 codes (one 8 B load) -> two 16 B stores; the
//                     tail at n is stored element by element.
// No LDS, no atomics, every output byte a pure function of the inputs.

#include "gather_common.h"
#include "kernels.h"

#define MX_THREADS 256
#define MX_KEY_ADD 0x4D58F8E4u
#define MX_NAN_BITS 0x7FC00000u

typedef short mx_v2s __attribute__((ext_vector_type(2)));
typedef float mx_v2f __attribute__((ext_vector_type(2)));

// cpu_ref.mx_key: seed fold and 64-bit step fold of the gathers' position
// keys, then the (rank, stage) pair
DEV uint32_t mx_key(uint64_t seed, uint64_t step, uint32_t stage,
                    uint32_t rank) {
  const uint32_t base =
      mix32((uint32_t)seed ^ mix32((uint32_t)(seed >> 32) + 0x9E3779B9u));
  uint32_t k = mix32(base + MX_KEY_ADD + (uint32_t)step * 0x9E3779B1u);
  k = mix32(k ^ mix32((uint32_t)(step >> 32) + 0x7F4A7C15u));
  return mix32(k + (2u * rank + stage + 1u) * 0xC2B2AE35u);
}

DEV uint32_t mx_amax8(const float* v) {
  uint32_t a = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) a = max(a, __float_as_uint(v[j]) & 0x7fffffffu);
  return a;
}

// max with the lane's quad neighbours (xor 1, then xor 2) by DPP quad_perm
DEV uint32_t mx_max_xor1(uint32_t a) {
  return max(a, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)a, 0xB1, 0xf,
                                                      0xf, true));
}
DEV uint32_t mx_max_xor2(uint32_t a) {
  return max(a, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)a, 0x4E, 0xf,
                                                      0xf, true));
}

// E8M0 byte of a block from A = max(bits & 0x7fffffff): 0xFF for a
// non-finite element, else the smallest e = byte - 127 >= -127 with amax *
// 2^-e <= 1.75 * 2^8
DEV uint32_t mx_scale_byte(uint32_t A) {
  if (A >= 0x7f800000u) return 0xFFu;
  const int b = (int)(A >> 23) - 8 + ((A & 0x7fffffu) > 0x600000u ? 1 : 0);
  return (uint32_t)max(b, 0);
}

// x * 2^-e rounded stochastically onto the e4m3 grid, as an fp32 value
DEV float mx_round(float x, int e, uint32_t rnd) {
  const uint32_t bits = __float_as_uint(x), mag = bits & 0x7fffffffu;
  int ef = (int)(mag >> 23);
  uint32_t M = mag & 0x7fffffu;
  if (ef == 0) {  // subnormal (or zero: M stays 0)
    const int lz = __clz((int)M) - 8;
    M <<= lz;
    ef = 1 - lz;
  } else {
    M |= 0x800000u;
  }
  const int k = ef - 127 - e;
  const int sh = min(63, 20 + max(0, -6 - k));
  const uint64_t T = ((uint64_t)M << 32) >> sh;
  const uint32_t q = (uint32_t)(T >> 32) + (rnd < (uint32_t)T ? 1u : 0u);
  const float y =
      (float)q * __uint_as_float((uint32_t)(max(k, -6) + 124) << 23);
  return q ? __uint_as_float(__float_as_uint(y) | (bits & 0x80000000u)) : 0.f;
}

// 8 elements from index i0 of the encoded vector -> their 8 code bytes
DEV uint2 mx_codes8(const float* v, uint32_t byte, uint32_t key,
                    uint32_t i0) {
  if (byte == 0xFFu) return make_uint2(0u, 0u);
  const int e = (int)byte - 127;
  float y[8];
#pragma unroll
  for (int j = 0; j < 8; ++j)
    y[j] = mx_round(v[j], e, mix32(key + (i0 + j) * 0x85EBCA6Bu));
  union { mx_v2s v; uint32_t u; } a, b;
  a.v = mx_v2s{0, 0};
  b.v = mx_v2s{0, 0};
  a.v = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(a.v, y[0], y[1], 1.f, false);
  a.v = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(a.v, y[2], y[3], 1.f, true);
  b.v = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(b.v, y[4], y[5], 1.f, false);
  b.v = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(b.v, y[6], y[7], 1.f, true);
  return make_uint2(a.u, b.u);
}

// 8 code bytes -> 8 fp32 values, times 2^(byte - 127)
DEV void mx_vals8(uint2 c, uint32_t byte, float* v) {
  const float scale = __uint_as_float(byte << 23);
  const mx_v2f d0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(c.x, scale, false);
  const mx_v2f d1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(c.x, scale, true);
  const mx_v2f d2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(c.y, scale, false);
  const mx_v2f d3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(c.y, scale, true);
  v[0] = d0.x; v[1] = d0.y; v[2] = d1.x; v[3] = d1.y;
  v[4] = d2.x; v[5] = d2.y; v[6] = d3.x; v[7] = d3.y;
}

extern "C" __global__ __launch_bounds__(MX_THREADS)
void mx_encode_kernel(const float* __restrict__ x, long n, int sb, int nbt,
                      uint64_t seed, uint64_t step, const long* step_dev,
                      uint32_t stage, uint32_t rank,
                      uint8_t* __restrict__ wire, float* __restrict__ keep) {
  const long g = (long)blockIdx.x * MX_THREADS + threadIdx.x;
  if (g >= 4L * nbt) return;  // wave-uniform: nbt is a multiple of 16
  if (step_dev) step = (uint64_t)*step_dev;
  const long i0 = g * 8;
  float v[8];
  if (i0 + 8 <= n) {
    const float4 a = *reinterpret_cast<const float4*>(x + i0);
    const float4 b = *reinterpret_cast<const float4*>(x + i0 + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    if (keep) {
      *reinterpret_cast<float4*>(keep + i0) = a;
      *reinterpret_cast<float4*>(keep + i0 + 4) = b;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[j] = i0 + j < n ? x[i0 + j] : 0.f;
      if (keep && i0 + j < n) keep[i0 + j] = v[j];
    }
  }
  const uint32_t byte = mx_scale_byte(mx_max_xor2(mx_max_xor1(mx_amax8(v))));
  const uint2 codes =
      mx_codes8(v, byte, mx_key(seed, step, stage, rank), (uint32_t)i0);
  const long b = g >> 2;
  const long w = b / sb, lb = b - w * sb;
  uint8_t* row = wire + w * 33L * sb;
  *reinterpret_cast<uint2*>(row + lb * 32 + (g & 3) * 8) = codes;
  // four blocks = 16 lanes: their scale bytes leave in one dword (lb is a
  // multiple of 4 there, and four blocks never straddle a shard)
  const uint32_t s4 = byte | ((uint32_t)__shfl_down((int)byte, 4, 64) << 8) |
                      ((uint32_t)__shfl_down((int)byte, 8, 64) << 16) |
                      ((uint32_t)__shfl_down((int)byte, 12, 64) << 24);
  if ((threadIdx.x & 15) == 0)
    *reinterpret_cast<uint32_t*>(row + 32L * sb + lb) = s4;
}

extern "C" __global__ __launch_bounds__(MX_THREADS)
void mx_reduce_kernel(const uint8_t* __restrict__ rows, int W, int sb,
                      uint64_t seed, uint64_t step, const long* step_dev,
                      uint32_t owner, uint8_t* __restrict__ shard) {
  const int h = blockIdx.x * MX_THREADS + threadIdx.x;  // half block
  // 2 * sb is a multiple of 32: lane pairs and groups of eight leave together
  if (h >= 2 * sb) return;
  if (step_dev) step = (uint64_t)*step_dev;
  const int lb = h >> 1, at = lb * 32 + (h & 1) * 16;
  float acc[16];
  for (int r = 0; r < W; ++r) {  // rank order
    const uint8_t* row = rows + (long)r * 33 * sb;
    const uint4 c = *reinterpret_cast<const uint4*>(row + at);
    const uint32_t byte = row[32 * sb + lb];  // 0xFF decodes to NaN
    float v[16];
    mx_vals8(make_uint2(c.x, c.y), byte, v);
    mx_vals8(make_uint2(c.z, c.w), byte, v + 8);
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = r ? acc[j] + v[j] : v[j];
  }
  const uint32_t byte =
      mx_scale_byte(mx_max_xor1(max(mx_amax8(acc), mx_amax8(acc + 8))));
  const uint32_t key = mx_key(seed, step, 1u, owner);
  const uint2 lo = mx_codes8(acc, byte, key, (uint32_t)at);
  const uint2 hi = mx_codes8(acc + 8, byte, key, (uint32_t)at + 8u);
  *reinterpret_cast<uint4*>(shard + at) = make_uint4(lo.x, lo.y, hi.x, hi.y);
  const uint32_t s4 = byte | ((uint32_t)__shfl_down((int)byte, 2, 64) << 8) |
                      ((uint32_t)__shfl_down((int)byte, 4, 64) << 16) |
                      ((uint32_t)__shfl_down((int)byte, 6, 64) << 24);
  if ((threadIdx.x & 7) == 0)
    *reinterpret_cast<uint32_t*>(shard + 32 * sb + lb) = s4;
}

extern "C" __global__ __launch_bounds__(MX_THREADS)
void mx_decode_kernel(const uint8_t* __restrict__ wire, int sb, long n,
                      float* __restrict__ out) {
  const long g = (long)blockIdx.x * MX_THREADS + threadIdx.x;
  const long i0 = g * 8;
  if (i0 >= n) return;
  const long b = g >> 2;
  const long w = b / sb, lb = b - w * sb;
  const uint8_t* row = wire + w * 33L * sb;
  const uint2 c = *reinterpret_cast<const uint2*>(row + lb * 32 + (g & 3) * 8);
  const uint32_t byte = row[32L * sb + lb];
  float v[8];
  mx_vals8(c, byte, v);
#pragma unroll
  for (int j = 0; j < 8; ++j)  // one NaN: scale byte 0xFF, codes 0x7F / 0xFF
    if (v[j] != v[j]) v[j] = __uint_as_float(MX_NAN_BITS);
  if (i0 + 8 <= n) {
    *reinterpret_cast<float4*>(out + i0) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(out + i0 + 4) =
        make_float4(v[4], v[5], v[6], v[7]);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (i0 + j < n) out[i0 + j] = v[j];
  }
}

int mx_shard_blocks(long n, int world) {
  const long nb = (n + 31) / 32;
  return (int)(((nb + world - 1) / world + 15) / 16 * 16);
}

void launch_mx_encode(const float* x, long n, int world, uint64_t seed,
                      uint64_t step, const long* step_dev, int stage, int rank,
                      uint8_t* wire, float* keep, hipStream_t s) {
  const int sb = mx_shard_blocks(n, world);
  const int nbt = world * sb;
  const int blocks = (4 * nbt + MX_THREADS - 1) / MX_THREADS;
  hipLaunchKernelGGL(mx_encode_kernel, dim3(blocks), dim3(MX_THREADS), 0, s, x,
                     n, sb, nbt, seed, step, step_dev, (uint32_t)stage,
                     (uint32_t)rank, wire, keep);
}

void launch_mx_reduce(const uint8_t* rows, int world, int sb, uint64_t seed,
                      uint64_t step, const long* step_dev, int owner,
                      uint8_t* shard, hipStream_t s) {
  const int blocks = (2 * sb + MX_THREADS - 1) / MX_THREADS;
  hipLaunchKernelGGL(mx_reduce_kernel, dim3(blocks), dim3(MX_THREADS), 0, s,
                     rows, world, sb, seed, step, step_dev, (uint32_t)owner,
                     shard);
}

void launch_mx_decode(const uint8_t* wire, int world, long n, float* out,
                      hipStream_t s) {
  const int sb = mx_shard_blocks(n, world);
  const long groups = (n + 7) / 8;
  const int blocks = (int)((groups + MX_THREADS - 1) / MX_THREADS);
  hipLaunchKernelGGL(mx_decode_kernel, dim3(blocks), dim3(MX_THREADS), 0, s,
                     wire, sb, n, out);
}
