// Device-resident MNIST input pipeline: build one training batch straight
// from the uint8 training set held in HBM.
//
//   x[j] = lut[ img_u8[ perm(epoch, pos + j) ] ]      bf16 [B,28,28,1]
//   y[j] =      lab_u8[ perm(epoch, pos + j) ]        int64 [B]
//
// with spe = N / B, epoch = step / spe, pos = (step % spe) * B.  `perm` is a
// stateless cycle-walking 4-round Feistel permutation of [0, N) keyed on
// (seed, epoch); epoch 0 is the identity (first epoch unshuffled, as
// data/mnist_data.py DataSet).  ops/cpu_ref.py holds the bit-identical
// reference; the two definitions must stay in lock-step.
//
// `step` comes either from the host or from `step_dev` (the device step
// counter dropout / drop-connect already use), which makes the launch
// hipGraph-capturable: under replay the batch follows the device counter.
#include "kernels.h"

namespace {

constexpr int GATHER_THREADS = 256;
// images per block: 2 x 98 units fill one pass of the 256 threads; measured
// best of {1,2,4,8,16} at B=64 and B=1024 (docs/KERNELS.md)
constexpr int GATHER_IPB = 2;
constexpr int ROW_BYTES = 784;          // 28*28 uint8 = 49 x 16 B
constexpr int ROW_UNITS = ROW_BYTES / 8;  // 98 units of 8 px per image

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x85EBCA6Bu;
  x ^= x >> 13; x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

__device__ __forceinline__ uint32_t feistel_enc(uint32_t v, int h,
                                                uint32_t mask,
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

}  // namespace

extern "C" __global__ __launch_bounds__(GATHER_THREADS)
void batch_gather_kernel(const uint8_t* __restrict__ img,
                         const uint8_t* __restrict__ lab,
                         const unsigned short* __restrict__ lut,
                         unsigned short* __restrict__ x, long* __restrict__ y,
                         uint32_t N, uint32_t B, int h, uint32_t key_base,
                         uint64_t step, const long* __restrict__ step_dev) {
  __shared__ unsigned short s_lut[256];
  __shared__ uint32_t s_idx[GATHER_IPB];
  const int tid = threadIdx.x;
  const uint32_t j0 = blockIdx.x * GATHER_IPB;

  s_lut[tid] = lut[tid];  // GATHER_THREADS == 256 entries
  if (tid < GATHER_IPB && j0 + tid < B) {
    // one lane per image: the permuted index is computed once, never per
    // pixel thread
    if (step_dev) step = (uint64_t)*step_dev;
    const uint64_t spe = N / B;  // B <= N checked host-side, so spe >= 1
    const uint64_t epoch = step / spe;
    uint32_t v = (uint32_t)(step % spe) * B + j0 + tid;  // < N
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
    s_idx[tid] = v;
    y[j0 + tid] = (long)lab[v];
  }
  __syncthreads();

  for (int u = tid; u < GATHER_IPB * ROW_UNITS; u += GATHER_THREADS) {
    const int im = u / ROW_UNITS;
    const int unit = u - im * ROW_UNITS;
    const uint32_t j = j0 + im;
    if (j >= B) break;  // last partial block (u is monotonic in im)
    const uint8_t* src = img + (size_t)s_idx[im] * ROW_BYTES + unit * 8;
    const uint2 px = *reinterpret_cast<const uint2*>(src);
    uint4 o;
    o.x = s_lut[px.x & 0xFF] | ((uint32_t)s_lut[(px.x >> 8) & 0xFF] << 16);
    o.y = s_lut[(px.x >> 16) & 0xFF] | ((uint32_t)s_lut[px.x >> 24] << 16);
    o.z = s_lut[px.y & 0xFF] | ((uint32_t)s_lut[(px.y >> 8) & 0xFF] << 16);
    o.w = s_lut[(px.y >> 16) & 0xFF] | ((uint32_t)s_lut[px.y >> 24] << 16);
    *reinterpret_cast<uint4*>(x + (size_t)j * ROW_BYTES + unit * 8) = o;
  }
}

// ---------------------------------------------------------------------------
// batch_gather_aug_kernel — the same batch, each image warped by one entry of
// an int32 [T,6] Q16 inverse-affine table before the LUT (definition and
// bit-exact oracle: ops/cpu_ref.py::affine_warp_u8 / aug_indices).
//
// Block = GATHER_IPB images.  One lane per image walks the permutation as
// above and picks the table row from (seed, step, batch position); the block
// stages the source rows into LDS with the same 8-byte loads, then a thread
// produces one 8-pixel unit of the flat output row as two 4-pixel halves (4
// divides 28, so a half never straddles an image row) walking the Q17
// source coordinates by +2*a00 / +2*a10 per column.
//
// Memory safety for ANY int32 table content: the coordinate arithmetic is
// unsigned (wraps, no UB); a tap reads LDS only under (unsigned)x < 28 &&
// (unsigned)y < 28, so its offset y*28+x lies in [0, 784); the table row is
// r % T with T >= 1 checked host-side.  Global addresses never depend on the
// table.
// ---------------------------------------------------------------------------
namespace {

constexpr int SIDE = 28;

__device__ __forceinline__ uint32_t aug_tap(const uint8_t* __restrict__ s,
                                            int y, int x) {
  // predicated to background 0 outside the image; never a clamped read
  return ((uint32_t)x < (uint32_t)SIDE && (uint32_t)y < (uint32_t)SIDE)
             ? (uint32_t)s[y * SIDE + x] : 0u;
}

__device__ __forceinline__ uint32_t aug_pixel(const uint8_t* __restrict__ s,
                                              uint32_t SX, uint32_t SY) {
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

}  // namespace

extern "C" __global__ __launch_bounds__(GATHER_THREADS)
void batch_gather_aug_kernel(const uint8_t* __restrict__ img,
                             const uint8_t* __restrict__ lab,
                             const unsigned short* __restrict__ lut,
                             const int* __restrict__ table, uint32_t T,
                             unsigned short* __restrict__ x,
                             long* __restrict__ y, uint32_t N, uint32_t B,
                             int h, uint32_t key_base, uint64_t step,
                             const long* __restrict__ step_dev) {
  __shared__ unsigned short s_lut[256];
  __shared__ uint32_t s_idx[GATHER_IPB];
  __shared__ uint32_t s_ent[GATHER_IPB][6];
  __shared__ __attribute__((aligned(8))) uint8_t s_img[GATHER_IPB][ROW_BYTES];
  const int tid = threadIdx.x;
  const uint32_t j0 = blockIdx.x * GATHER_IPB;

  s_lut[tid] = lut[tid];  // GATHER_THREADS == 256 entries
  if (tid < GATHER_IPB && j0 + tid < B) {
    if (step_dev) step = (uint64_t)*step_dev;
    const uint64_t spe = N / B;  // B <= N checked host-side, so spe >= 1
    const uint64_t epoch = step / spe;
    uint32_t v = (uint32_t)(step % spe) * B + j0 + tid;  // < N
    if (epoch != 0) {
      const uint32_t mask = (1u << h) - 1u;
      uint32_t key[4];
#pragma unroll
      for (int r = 0; r < 4; ++r)
        key[r] = mix32(key_base + (uint32_t)epoch * 0x9E3779B1u + r);
      do {  // terminates below N: see batch_gather_kernel
        v = feistel_enc(v, h, mask, key);
      } while (v >= N);
    }
    s_idx[tid] = v;
    y[j0 + tid] = (long)lab[v];
    // table row of batch position j0 + tid: mirror of cpu_ref.aug_indices
    uint32_t k = mix32(key_base + 0x632BE5ABu + (uint32_t)step * 0x9E3779B1u);
    k = mix32(k ^ mix32((uint32_t)(step >> 32) + 0x7F4A7C15u));
    const uint32_t row = mix32(k + (j0 + tid) * 0x85EBCA6Bu) % T;  // < T
#pragma unroll
    for (int e = 0; e < 6; ++e)
      s_ent[tid][e] = (uint32_t)table[(size_t)row * 6 + e];
  }
  __syncthreads();

  for (int u = tid; u < GATHER_IPB * ROW_UNITS; u += GATHER_THREADS) {
    const int im = u / ROW_UNITS;
    const int unit = u - im * ROW_UNITS;
    if (j0 + im >= B) break;  // last partial block (u is monotonic in im)
    const uint8_t* src = img + (size_t)s_idx[im] * ROW_BYTES + unit * 8;
    *reinterpret_cast<uint2*>(&s_img[im][unit * 8]) =
        *reinterpret_cast<const uint2*>(src);
  }
  __syncthreads();

  for (int u = tid; u < GATHER_IPB * ROW_UNITS; u += GATHER_THREADS) {
    const int im = u / ROW_UNITS;
    const int unit = u - im * ROW_UNITS;
    const uint32_t j = j0 + im;
    if (j >= B) break;
    const uint8_t* s = s_img[im];
    const uint32_t a00 = s_ent[im][0], a01 = s_ent[im][1];
    const uint32_t a10 = s_ent[im][2], a11 = s_ent[im][3];
    const uint32_t t0 = s_ent[im][4], t1 = s_ent[im][5];
    uint32_t o[4];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int p = unit * 8 + half * 4;  // flat pixel, < 784
      const int r = p / SIDE, c = p - r * SIDE;
      const uint32_t uc = (uint32_t)(2 * c - (SIDE - 1));
      const uint32_t ur = (uint32_t)(2 * r - (SIDE - 1));
      uint32_t SX = ((SIDE - 1) << 16) + a00 * uc + a01 * ur + 2u * t0;
      uint32_t SY = ((SIDE - 1) << 16) + a10 * uc + a11 * ur + 2u * t1;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const uint32_t v0 = aug_pixel(s, SX, SY);
        SX += 2u * a00; SY += 2u * a10;
        const uint32_t v1 = aug_pixel(s, SX, SY);
        SX += 2u * a00; SY += 2u * a10;
        o[half * 2 + q] = s_lut[v0] | ((uint32_t)s_lut[v1] << 16);
      }
    }
    *reinterpret_cast<uint4*>(x + (size_t)j * ROW_BYTES + unit * 8) =
        make_uint4(o[0], o[1], o[2], o[3]);
  }
}

namespace {

// step-independent launch parameters shared by the two gathers
inline void gather_params(uint32_t N, uint64_t seed, uint32_t* key_base,
                          int* h) {
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

}  // namespace

void launch_batch_gather_aug(const uint8_t* img, const uint8_t* lab,
                             const unsigned short* lut, const int* table,
                             uint32_t T, unsigned short* x, long* y,
                             uint32_t N, uint32_t B, uint64_t seed,
                             uint64_t step, const long* step_dev,
                             hipStream_t s) {
  uint32_t key_base;
  int h;
  gather_params(N, seed, &key_base, &h);
  const int blocks = (int)((B + GATHER_IPB - 1) / GATHER_IPB);
  hipLaunchKernelGGL(batch_gather_aug_kernel, dim3(blocks),
                     dim3(GATHER_THREADS), 0, s, img, lab, lut, table, T, x,
                     y, N, B, h, key_base, step, step_dev);
}

void launch_batch_gather(const uint8_t* img, const uint8_t* lab,
                         const unsigned short* lut, unsigned short* x,
                         long* y, uint32_t N, uint32_t B, uint64_t seed,
                         uint64_t step, const long* step_dev, hipStream_t s) {
  // host mirror of mix32 for the step-independent part of the key schedule
  auto hmix = [](uint32_t v) {
    v ^= v >> 16; v *= 0x85EBCA6Bu;
    v ^= v >> 13; v *= 0xC2B2AE35u;
    v ^= v >> 16;
    return v;
  };
  const uint32_t key_base =
      hmix((uint32_t)seed ^ hmix((uint32_t)(seed >> 32) + 0x9E3779B9u));
  int bits = 0;
  for (uint32_t m = N - 1; m; m >>= 1) ++bits;
  if (bits < 2) bits = 2;
  bits += bits & 1;
  const int blocks = (int)((B + GATHER_IPB - 1) / GATHER_IPB);
  hipLaunchKernelGGL(batch_gather_kernel, dim3(blocks), dim3(GATHER_THREADS),
                     0, s, img, lab, lut, x, y, N, B, bits / 2, key_base,
                     step, step_dev);
}
