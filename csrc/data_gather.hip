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
//
// The pieces shared with elastic_gather.hip live in gather_common.h.
#include "gather_common.h"
#include "kernels.h"

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
    const uint32_t v = gather_sample(N, B, h, key_base, step, j0 + tid);
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
    o.x = lut_pair(s_lut, px.x & 0xFF, (px.x >> 8) & 0xFF);
    o.y = lut_pair(s_lut, (px.x >> 16) & 0xFF, px.x >> 24);
    o.z = lut_pair(s_lut, px.y & 0xFF, (px.y >> 8) & 0xFF);
    o.w = lut_pair(s_lut, (px.y >> 16) & 0xFF, px.y >> 24);
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
    const uint32_t v = gather_sample(N, B, h, key_base, step, j0 + tid);
    s_idx[tid] = v;
    y[j0 + tid] = (long)lab[v];
    // table row of batch position j0 + tid: mirror of cpu_ref.aug_indices
    const uint32_t row =
        position_key(key_base, AUG_ROW_ADD, step, j0 + tid) % T;  // < T
#pragma unroll
    for (int e = 0; e < 6; ++e)
      s_ent[tid][e] = (uint32_t)table[(size_t)row * 6 + e];
  }
  __syncthreads();

  stage_rows(img, s_idx, s_img, j0, B, tid);
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
      uint32_t SX = aug_origin(a00, a01, t0, p);
      uint32_t SY = aug_origin(a10, a11, t1, p);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const uint32_t v0 = aug_pixel(s, SX, SY);
        SX += 2u * a00; SY += 2u * a10;
        const uint32_t v1 = aug_pixel(s, SX, SY);
        SX += 2u * a00; SY += 2u * a10;
        o[half * 2 + q] = lut_pair(s_lut, v0, v1);
      }
    }
    *reinterpret_cast<uint4*>(x + (size_t)j * ROW_BYTES + unit * 8) =
        make_uint4(o[0], o[1], o[2], o[3]);
  }
}

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
  uint32_t key_base;
  int h;
  gather_params(N, seed, &key_base, &h);
  const int blocks = (int)((B + GATHER_IPB - 1) / GATHER_IPB);
  hipLaunchKernelGGL(batch_gather_kernel, dim3(blocks), dim3(GATHER_THREADS),
                     0, s, img, lab, lut, x, y, N, B, h, key_base, step,
                     step_dev);
}
