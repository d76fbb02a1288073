// batch_gather_elastic_kernel — the batch of batch_gather_aug_kernel with an
// elastic distortion (Simard et al. 2003) added to the affine warp: every
// output pixel's source position moves by a per-image random displacement
// field, uniform noise smoothed by a Gaussian.  Definition and bit-exact
// oracle: ops/cpu_ref.py::elastic_key / elastic_noise / elastic_field /
// elastic_warp_u8.  Everything is integer, and integer accumulation does not
// depend on the summation order, so the matrix instruction below and the
// numpy products of the oracle give the same bits.
//
// Per (image, axis) the field is two 28x28 products with the symmetric
// Toeplitz tap matrix G[i][k] = g[|i-k|] (zero outside the image):
//
//   T  = G . N            N[k][c] int8 noise, hashed from (key, axis, pixel)
//   T8 = (T + 128) >> 8   back to int8
//   F  = T8 . G           =>  F^T = G . T8^T
//   dS = (A * F) >> 6     Q17 displacement, added to SX (axis 0) / SY (1)
//
// Work split.  Block = GATHER_IPB = 2 images, 4 waves.  In the field phase
// wave w owns (image w >> 1, axis w & 1) and issues two
// v_mfma_i32_32x32x32_i8, each one whole 32x32x32 product (28 padded to 32):
//
//   operands   lane l supplies row (A) / column (B) l % 32 and the 16 k
//              values 16 * (l / 32) + e, byte e of its 4 VGPRs.  The same k
//              assignment on both sides is all an integer sum needs.
//   A = G      built once per wave from the 32-entry tap table in LDS
//              (index |i-k| <= 31) and used by BOTH products, since G is
//              symmetric and the second product is taken transposed.
//   B1 = N     never in memory: lane (c, half) hashes its 16 noise bytes
//              straight into the operand registers; rows / columns 28..31
//              are zero.
//   C layout   lane l holds column l % 32, register r row
//              (r & 3) + 8 * (r >> 2) + 4 * (l / 32)  (as conv1_mfma.hip).
//   B2 = T8^T  after product 1 a lane holds one COLUMN c of T, product 2
//              contracts over c, so T8 makes one round trip through the
//              wave's private LDS tile: 16 byte stores tile[i][c], one
//              16-byte load tile[i = l % 32][16 * (l / 32) ..].  Pitch 48 B:
//              the 16 lanes of a load phase start 12 banks apart and cover
//              the 64 banks exactly once.
//   result     lane l holds image row l % 32 of F, register r image column
//              (r & 3) + 8 * (r >> 2) + 4 * (l / 32): four registers are
//              four consecutive pixels, one 16-byte store of dS each.
//
// The tile is private to its wave, so the round trip needs wave-level
// ordering only (LDS operations of a wave execute in order; the fence keeps
// the compiler from reordering).  One block barrier separates the field
// phase from the warp phase, which is the loop of batch_gather_aug_kernel
// with dS read from LDS and added before aug_pixel.
//
// Memory safety for ANY table / taps / alpha_q content: the coordinate and
// displacement arithmetic is unsigned (wraps, no UB); a pixel tap reads LDS
// only under the (unsigned) < 28 predicates of aug_tap; the tap table index
// is |i-k| <= 31, inside its 32 entries; operand bytes are the low 8 bits of
// whatever the taps / T8 hold; the table row is r % T with T >= 1 checked
// host-side.  Neither a global address nor an LDS address outside aug_tap
// depends on the table, the taps, alpha_q or the field.
#include "gather_common.h"
#include "kernels.h"

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(16))) int i32x16;

namespace {

constexpr uint32_t ELASTIC_KEY_ADD = 0x3C6EF372u;    // cpu_ref.elastic_key
constexpr uint32_t ELASTIC_NOISE_MUL = 0xB5297A4Du;  // cpu_ref.elastic_noise
constexpr int TILE_PITCH = 48;
constexpr int TILE_BYTES = 32 * TILE_PITCH;  // 1536 B per wave

// A operand: row i of G, k = 16 * half + e in byte e
DEV i32x4 elastic_g_operand(const int* s_taps, int i, int half) {
  i32x4 a;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    uint32_t w = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = 16 * half + 4 * d + e;
      const int dist = i > k ? i - k : k - i;  // 0..31
      const uint32_t g = (i < SIDE && k < SIDE) ? (uint32_t)s_taps[dist] : 0u;
      w |= (g & 0xFFu) << (8 * e);
    }
    a[d] = (int)w;
  }
  return a;
}

// B operand of the first product: column c of the noise of `axis`, rows
// k = 16 * half + e; n = (mix32(key + (axis*784 + k*28 + c) * MUL) >> 24)
// - 128, whose int8 byte is the hash byte with the top bit flipped
DEV i32x4 elastic_noise_operand(uint32_t key, int axis, int c, int half) {
  i32x4 b;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    uint32_t w = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = 16 * half + 4 * d + e;
      const uint32_t el = (uint32_t)(axis * ROW_BYTES + k * SIDE + c);
      const uint32_t n = (mix32(key + el * ELASTIC_NOISE_MUL) >> 24) ^ 0x80u;
      w |= ((c < SIDE && k < SIDE) ? n : 0u) << (8 * e);
    }
    b[d] = (int)w;
  }
  return b;
}

}  // namespace

extern "C" __global__ __launch_bounds__(GATHER_THREADS)
void batch_gather_elastic_kernel(const uint8_t* __restrict__ img,
                                 const uint8_t* __restrict__ lab,
                                 const unsigned short* __restrict__ lut,
                                 const int* __restrict__ table, uint32_t T,
                                 const int* __restrict__ taps,
                                 uint32_t alpha_q,
                                 unsigned short* __restrict__ x,
                                 long* __restrict__ y, uint32_t N, uint32_t B,
                                 int h, uint32_t key_base, uint64_t step,
                                 const long* __restrict__ step_dev) {
  __shared__ unsigned short s_lut[256];
  __shared__ uint32_t s_idx[GATHER_IPB];
  __shared__ uint32_t s_ent[GATHER_IPB][6];
  __shared__ uint32_t s_key[GATHER_IPB];
  __shared__ int s_taps[32];
  __shared__ __attribute__((aligned(8))) uint8_t s_img[GATHER_IPB][ROW_BYTES];
  __shared__ __attribute__((aligned(16))) uint8_t s_tile[4][TILE_BYTES];
  __shared__ __attribute__((aligned(16))) int s_ds[GATHER_IPB][2][ROW_BYTES];
  static_assert(GATHER_THREADS == 2 * GATHER_IPB * 64,
                "one wave per (image, axis)");
  const int tid = threadIdx.x;
  const uint32_t j0 = blockIdx.x * GATHER_IPB;

  s_lut[tid] = lut[tid];  // GATHER_THREADS == 256 entries
  if (tid >= 64 && tid < 96) s_taps[tid - 64] = taps[tid - 64];
  if (tid < GATHER_IPB && j0 + tid < B) {
    if (step_dev) step = (uint64_t)*step_dev;
    const uint32_t v = gather_sample(N, B, h, key_base, step, j0 + tid);
    s_idx[tid] = v;
    y[j0 + tid] = (long)lab[v];
    const uint32_t row =
        position_key(key_base, AUG_ROW_ADD, step, j0 + tid) % T;  // < T
#pragma unroll
    for (int e = 0; e < 6; ++e)
      s_ent[tid][e] = (uint32_t)table[(size_t)row * 6 + e];
    s_key[tid] = position_key(key_base, ELASTIC_KEY_ADD, step, j0 + tid);
  }
  __syncthreads();

  stage_rows(img, s_idx, s_img, j0, B, tid);

  // ---- field phase: wave -> (image, axis) -------------------------------
  const int lane = tid & 63, wave = tid >> 6;
  const int fim = wave >> 1, axis = wave & 1;
  if (j0 + fim < B) {  // wave-uniform
    const int col = lane & 31, half = lane >> 5;
    const i32x4 g = elastic_g_operand(s_taps, col, half);
    const i32x4 nz = elastic_noise_operand(s_key[fim], axis, col, half);
    i32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0;
    // T[i][c]: this lane holds column c = col
    i32x16 t = __builtin_amdgcn_mfma_i32_32x32x32_i8(g, nz, acc, 0, 0, 0);
    uint8_t* tile = s_tile[wave];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = (r & 3) + 8 * (r >> 2) + 4 * half;  // < 32
      tile[i * TILE_PITCH + col] =
          (uint8_t)(((uint32_t)t[r] + 128u) >> 8);  // low 8 bits of T8
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // T8^T operand: row i = col of T8, columns 16 * half ..
    const i32x4 t8 =
        *reinterpret_cast<const i32x4*>(tile + col * TILE_PITCH + 16 * half);
    // F^T[j][i]: this lane holds image row i = col, register r column j
    i32x16 f = __builtin_amdgcn_mfma_i32_32x32x32_i8(g, t8, acc, 0, 0, 0);
    int* ds = s_ds[fim][axis];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int jc = 8 * q + 4 * half;  // image column of register 4q
      if (col < SIDE && jc < SIDE) {
        i32x4 d;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          d[e] = (int)(alpha_q * (uint32_t)f[4 * q + e]) >> 6;
        *reinterpret_cast<i32x4*>(ds + col * SIDE + jc) = d;
      }
    }
  }
  __syncthreads();

  // ---- warp phase --------------------------------------------------------
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
      const int p = unit * 8 + half * 4;  // flat pixel, < 784, 16 B aligned
      uint32_t SX = aug_origin(a00, a01, t0, p);
      uint32_t SY = aug_origin(a10, a11, t1, p);
      const i32x4 dx = *reinterpret_cast<const i32x4*>(&s_ds[im][0][p]);
      const i32x4 dy = *reinterpret_cast<const i32x4*>(&s_ds[im][1][p]);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const uint32_t v0 = aug_pixel(s, SX + (uint32_t)dx[2 * q],
                                      SY + (uint32_t)dy[2 * q]);
        SX += 2u * a00; SY += 2u * a10;
        const uint32_t v1 = aug_pixel(s, SX + (uint32_t)dx[2 * q + 1],
                                      SY + (uint32_t)dy[2 * q + 1]);
        SX += 2u * a00; SY += 2u * a10;
        o[half * 2 + q] = lut_pair(s_lut, v0, v1);
      }
    }
    *reinterpret_cast<uint4*>(x + (size_t)j * ROW_BYTES + unit * 8) =
        make_uint4(o[0], o[1], o[2], o[3]);
  }
}

void launch_batch_gather_elastic(const uint8_t* img, const uint8_t* lab,
                                 const unsigned short* lut, const int* table,
                                 uint32_t T, const int* taps,
                                 uint32_t alpha_q, unsigned short* x, long* y,
                                 uint32_t N, uint32_t B, uint64_t seed,
                                 uint64_t step, const long* step_dev,
                                 hipStream_t s) {
  uint32_t key_base;
  int h;
  gather_params(N, seed, &key_base, &h);
  const int blocks = (int)((B + GATHER_IPB - 1) / GATHER_IPB);
  hipLaunchKernelGGL(batch_gather_elastic_kernel, dim3(blocks),
                     dim3(GATHER_THREADS), 0, s, img, lab, lut, table, T,
                     taps, alpha_q, x, y, N, B, h, key_base, step, step_dev);
}
