// LeNet conv1 (H=W=28, Cin=1, Cout=32, 5x5 SAME) on v_mfma_f32_32x32x16_bf16.
//
// The Cin=1 layer was a pair of VALU v_dot2c kernels (ops_misc.hip) because
// the im2col implicit-GEMM form gathers every A element from global memory
// (579 us at B=8192).  Here the image sits in LDS as a zero-haloed slab and
// the GEMM K axis is laid out so that one lane's 8 operand elements are 8
// CONTIGUOUS slab pixels of one row: an A fragment is a single 16-byte LDS
// read, no gather.
//
//   forward  out[pixel][co] = sum_k patch[pixel][k] * Wp[k][co]
//            k = kh*8 + kw', rows padded 5 -> 8 taps (zero weights), kh 0..5
//            (row 5 all zero): 3 MFMAs per 32-pixel tile, M pool-grouped
//            (m = window*4 + pos) so a lane ends up holding four complete
//            2x2 windows of one channel — bias/relu/maxpool/argmax stay in
//            registers.
//   dW       dw[tap][co] = sum_pixel patch[pixel][tap] * g[pixel][co]
//            M = 25 taps (padded to 32), N = co, K = pixels walked as 16-
//            pixel half rows of a 32-wide padded row; g is decoded on the
//            fly from the pooled (dy, argmax) pair and is 0 on the halo.
//
// Padding taps / halo pixels multiply REAL slab contents by zero, so every
// LDS location a fragment can touch is zero-filled before use (NaN*0=NaN).
//
// Unaligned fragments: a fragment starts at an arbitrary pixel (2-byte
// aligned).  The slab is kept twice — the second copy shifted left by one
// pixel — so odd-based fragments read the shifted copy at an even pixel and
// every read is 4-byte aligned; the read itself is a __builtin_memcpy so the
// compiler picks a legal LDS instruction for that alignment.

#include "common.h"
#include "kernels.h"
#include <stdlib.h>

typedef __attribute__((ext_vector_type(16))) float f32x16;

// Slab geometry (elements are bf16).  Rows 0..32 x cols 0..35: the forward
// touches rows <= 27+5 and cols <= 27+7, the dW rows <= 27+4 and cols <=
// 24+4+7.  Pitch 36 (18 dwords): the three slab rows one forward fragment
// read spans land 18 banks apart and the 8 windows of a tile on consecutive
// banks; the odd copy starts at dword 648 = 8 mod 64, next to them.
#define C1_PITCH 36
#define C1_ROWS 33
#define C1_ODD 1296                 // element offset of the shifted copy
#define C1_SLAB 2496                // 1296 + 33*36 = 2484, rounded up to x8
#define C1_IMG (28 * 28)
#define C1_QPI (14 * 14)            // pooled windows per image

DEV void c1_zero_slab(ushort_t* slab, int tid) {
  for (int i = tid; i < C1_SLAB / 8; i += 256)
    *reinterpret_cast<short8*>(slab + i * 8) = short8{0, 0, 0, 0, 0, 0, 0, 0};
}

// interior of both copies from one image: 196 threads x one 8-byte load
// (4 pixels; image rows are 56 B so every 4-pixel group is 8-byte aligned)
DEV void c1_stage_image(ushort_t* slab, const ushort_t* xi, int tid) {
  if (tid < C1_IMG / 4) {
    uint2 v = *reinterpret_cast<const uint2*>(xi + tid * 4);
    int row = tid / 7, col = (tid % 7) * 4;
    ushort_t* a = slab + (row + 2) * C1_PITCH + col + 2;   // even: 4B aligned
    *reinterpret_cast<unsigned*>(a) = v.x;
    *reinterpret_cast<unsigned*>(a + 2) = v.y;
    // shifted copy: odd[r][c] = even[r][c + 1]
    ushort_t* b = slab + C1_ODD + (row + 2) * C1_PITCH + col + 1;
    b[0] = (ushort_t)(v.x & 0xffffu);
    *reinterpret_cast<unsigned*>(b + 1) = (v.x >> 16) | (v.y << 16);
    b[3] = (ushort_t)(v.y >> 16);
  }
}

// 8 consecutive slab pixels starting at a 4-byte-aligned address
DEV short8 c1_frag(const ushort_t* p) {
  short8 v;
  __builtin_memcpy(&v, __builtin_assume_aligned(p, 4), 16);
  return v;
}

// ---------------------------------------------------------------------------
// forward: one image per block, 4 waves x (25 tiles of 8 pooled windows)
// ---------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(256)
void conv1_mfma_fwd_kernel(const ushort_t* __restrict__ x,
                           const ushort_t* __restrict__ w,   // [25][32]
                           const float* __restrict__ bias,
                           ushort_t* __restrict__ y,
                           uint8_t* __restrict__ amax, int NB) {
  __shared__ __align__(16) ushort_t slab[C1_SLAB];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int img = blockIdx.x;
  c1_zero_slab(slab, tid);

  // B fragments (12 VGPR, once per block): lane (co, h) element e of MFMA j
  // is Wp[kh = 2j + h][kw' = e][co]; taps kw' >= 5 and row kh = 5 are zero
  const int co = lane & 31, h = lane >> 5;
  short8 bf[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    int kh = 2 * j + h;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      bf[j][e] = (e < 5 && kh < 5) ? (short)w[(kh * 5 + e) * 32 + co] : (short)0;
  }
  const float b = bias[co];

  __syncthreads();
  c1_stage_image(slab, x + (size_t)img * C1_IMG, tid);
  __syncthreads();

  // A row of this lane: m = window*4 + pos within the tile
  const int pos = lane & 3, win = (lane & 31) >> 2;
  ushort_t* yi = y + (size_t)img * C1_QPI * 32;
  uint8_t* ai = amax + (size_t)img * C1_QPI * 32;
  for (int tile = wave; tile < (C1_QPI + 7) / 8; tile += 4) {
    int q = tile * 8 + win;
    if (q >= C1_QPI) q = 0;            // pad rows of the last tile: any valid
    int ho = q / 14, wo = q - ho * 14;  // window, results discarded
    // fragment j = slab[oy + 2j + h][ox .. ox+7], (oy, ox) = conv pixel in
    // padded coords; odd ox reads the shifted copy at ox - 1
    const ushort_t* p = slab + (pos & 1) * C1_ODD +
                        (2 * ho + (pos >> 1) + h) * C1_PITCH + 2 * wo;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = b;
#pragma unroll
    for (int j = 0; j < 3; ++j)
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          c1_frag(p + j * 2 * C1_PITCH), bf[j], acc, 0, 0, 0);
    // C layout: col = co, row = (reg&3) + 8*(reg>>2) + 4h -> registers
    // 4g..4g+3 are the four positions of window 2g + h
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float best = -1.0f / 0.0f;
      int barg = 0;
#pragma unroll
      for (int pz = 0; pz < 4; ++pz) {
        float v = acc[4 * g + pz];
        v = v > 0.f ? v : 0.f;
        if (v > best) { best = v; barg = pz; }
      }
      int qq = tile * 8 + 2 * g + h;
      if (qq < C1_QPI) {
        yi[qq * 32 + co] = f2bf(best);
        // 7 = dead window (liveness for the pooled-consumer backward)
        ai[qq * 32 + co] = (uint8_t)(best > 0.f ? barg : 7);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// dW + db from the pooled gradient: G images per block, wave w owns pooled
// rows w, w+4, ... of each image and one 32x32 fp32 accumulator; waves
// reduce through LDS and the block flushes 800 + 32 atomics once.
// ---------------------------------------------------------------------------
// DET (deterministic mode): dw is the plane set [blocks][CONV1_DET_PLANE];
// block b stores its 800 dW sums and 32 db sums into plane b instead of
// adding into the bucket (db unused).
template <bool DET>
__global__ __launch_bounds__(256)
void conv1_mfma_dw_kernel(const ushort_t* __restrict__ x,
                          const ushort_t* __restrict__ dyp,
                          const uint8_t* __restrict__ am,
                          float* __restrict__ dw, float* __restrict__ db,
                          int NB, int G) {
  __shared__ __align__(16) ushort_t slab[C1_SLAB];
  __shared__ float red[4][25 * 32];
  __shared__ float reddb[8][32];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int co = lane & 31, h = lane >> 5;
  c1_zero_slab(slab, tid);

  // A row = tap (kh, kw); pad rows 25..31 re-read tap 0, outputs discarded.
  // Fragment for pixel row yy, half-row s: slab[yy + kh][16s + 8h + kw ..+7]
  int tap = lane & 31;
  if (tap >= 25) tap = 0;
  const int kh = tap / 5, kw = tap - kh * 5;
  const ushort_t* abase = slab + (kw & 1) * C1_ODD + kh * C1_PITCH + 8 * h +
                          (kw & ~1);

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float dbacc = 0.f;

  const int img0 = blockIdx.x * G;
  for (int g = 0; g < G; ++g) {
    const int img = img0 + g;
    if (img >= NB) break;  // uniform across the block
    // this wave's pooled loads for the whole image go out first (up to 32
    // dy + 32 argmax, one latency wall per image), then the slab is staged
    // under them.  Lane (co, h) decodes windows 8s + 4h + i of each row.
    // (Loading one image AHEAD into a second register set was measured and
    // gained nothing: 20.8 vs 19.2 us at B=1024, 67.6 vs 65.6 at 8192.)
    ushort_t rdy[4][2][4];
    uint8_t ram[4][2][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int rq = wave + 4 * k;
      if (rq >= 14) break;  // wave-uniform
      size_t rb = (((size_t)img * 14 + rq) * 14) * 32 + co;
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          int wq = 8 * s + 4 * h + i;
          if (wq > 13) wq = 13;  // halo windows: clamped read, zeroed below
          rdy[k][s][i] = dyp[rb + wq * 32];
          ram[k][s][i] = am[rb + wq * 32];
        }
    }
    __syncthreads();  // zero-fill / previous image's fragment reads done
    c1_stage_image(slab, x + (size_t)img * C1_IMG, tid);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int rq = wave + 4 * k;
      if (rq >= 14) break;
      // B fragment of (row 2rq + ry, half s): pixel pair of window i is
      // (g, 0) / (0, g) when the argmax lies in this row, else 0
      unsigned gp[2][2][4];
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          unsigned a = ram[k][s][i];  // 0..3 live, 7 dead
          bool live = (8 * s + 4 * h + i < 14) && a < 4u;
          unsigned gb = live ? (unsigned)rdy[k][s][i] : 0u;
          dbacc += bf2f((ushort_t)gb);  // db once per window
          unsigned placed = (a & 1u) ? (gb << 16) : gb;
          gp[s][0][i] = (a & 2u) ? 0u : placed;
          gp[s][1][i] = (a & 2u) ? placed : 0u;
        }
#pragma unroll
      for (int ry = 0; ry < 2; ++ry)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          union { unsigned u[4]; short8 v; } bfr;
#pragma unroll
          for (int i = 0; i < 4; ++i) bfr.u[i] = gp[s][ry][i];
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              c1_frag(abase + (2 * rq + ry) * C1_PITCH + 16 * s), bfr.v, acc,
              0, 0, 0);
        }
    }
  }

  // cross-wave reduction in fixed order, then one flush per block
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int row = (r & 3) + 8 * (r >> 2) + 4 * h;
    if (row < 25) red[wave][row * 32 + co] = acc[r];
  }
  reddb[wave * 2 + h][co] = dbacc;
  __syncthreads();
  if (DET) {
    float* pl = dw + (size_t)blockIdx.x * CONV1_DET_PLANE;
    for (int i = tid; i < 25 * 32; i += 256)
      pl[i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
    if (tid < 32) {
      float v = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) v += reddb[k][tid];
      pl[25 * 32 + tid] = v;
    }
    return;
  }
  for (int i = tid; i < 25 * 32; i += 256)
    atomicAdd(&dw[i], (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]));
  if (db && tid < 32) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) v += reddb[k][tid];
    atomicAdd(&db[tid], v);
  }
}

// ---- host side -------------------------------------------------------------

bool conv1_mfma_supported(int H, int W, int Cin, int Cout) {
  return H == 28 && W == 28 && Cin == 1 && Cout == 32;
}

// DMNIST_CONV1_VALU=1 forces the v_dot2c kernels (read on every call so the
// two paths can be A/B-compared in one process)
bool conv1_mfma_enabled() {
  const char* e = getenv("DMNIST_CONV1_VALU");
  return !(e && atoi(e));
}

void launch_conv1_mfma_fwd(const unsigned short* x, const unsigned short* w,
                           const float* bias, unsigned short* y,
                           uint8_t* amax, int NB, hipStream_t s) {
  if (NB <= 0) return;
  hipLaunchKernelGGL(conv1_mfma_fwd_kernel, dim3(NB), dim3(256), 0, s, x, w,
                     bias, y, amax, NB);
}

int conv1_mfma_dw_group(int NB) {
  int G = NB >= 4096 ? 16 : (NB >= 512 ? 4 : 1);
  if (const char* e = getenv("DMNIST_DW1_G")) G = atoi(e);  // flush sweep
  return G < 1 ? 1 : G;
}

void launch_conv1_mfma_dw(const unsigned short* x, const unsigned short* dyp,
                          const uint8_t* am, float* dw, float* db, int NB,
                          hipStream_t s) {
  if (NB <= 0) return;
  int G = conv1_mfma_dw_group(NB);
  int blocks = (NB + G - 1) / G;
  hipLaunchKernelGGL(conv1_mfma_dw_kernel<false>, dim3(blocks), dim3(256), 0,
                     s, x, dyp, am, dw, db, NB, G);
}

int conv1_mfma_dw_blocks(int NB) {
  int G = conv1_mfma_dw_group(NB);
  return NB <= 0 ? 0 : (NB + G - 1) / G;
}

void launch_conv1_mfma_dw_det(const unsigned short* x,
                              const unsigned short* dyp, const uint8_t* am,
                              float* planes, int NB, hipStream_t s) {
  if (NB <= 0) return;
  hipLaunchKernelGGL(conv1_mfma_dw_kernel<true>,
                     dim3(conv1_mfma_dw_blocks(NB)), dim3(256), 0, s, x, dyp,
                     am, planes, (float*)nullptr, NB, conv1_mfma_dw_group(NB));
}
