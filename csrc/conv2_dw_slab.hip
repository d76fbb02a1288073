// LeNet conv2 dW (H=W=14, Cin=32, Cout=64, 5x5 SAME, NHWC bf16) from
// per-image PIXEL-MAJOR LDS slabs: glds staging + ds_read_b64_tr_b16
// fragments, no im2col gather.
//
//   dW[kh,kw,ci,co] += sum_{n,h,w} x[n,h+kh-2,w+kw-2,ci] * dact[n,h,w,co]
//
// dw_tr.hip's AM_CONV5 mode computes the same thing as an im2col GEMM and
// fetches every 16-byte chunk of x from L2 once per tap (25x, ~321 MB per
// step at B=1024).  Here a block stages each image ONCE per kernel row and
// all taps read the same slab at shifted rows.
//
// Layout.  Both slabs keep the pixel as the LDS row (k-major, exactly what
// tr16 wants) with a row pitch of 16 pixels:
//   D[k][co]  k = h*16 + w, h 0..13, w 0..15   224 rows x 128 B = 28 KB
//   X[s][ci]  s = MG + sr*16 + c, sr 0..NRX-1, c 0..15, 64 B rows,
//             plus MG = 8 zero pixels in front and behind
// A block owns KHB consecutive kernel rows kh0..kh0+KHB-1 (KHB = 1: five
// blocks per image group, 160 x 64 outputs each; KHB = 5: one block, all
// 800 x 64).  Slab row sr holds image row sr + kh0 - 2, NRX = 13 + KHB.
// Columns 14, 15 of every row (both slabs) and every slab row whose image
// row is outside 0..13 are zero: the staging lanes that own them source
// from a zeroed device page, so they are rewritten as zero with every image.
//
// The reduction runs over the padded-linear k = h*16 + w, 224 values in 7
// k-steps of 32 (196 real, 87.5 %).  For tap (khl, kw), khl = kh - kh0, the
// x operand row of pixel k is
//   s = MG + khl*16 + k + (kw - 2)
// a whole-row offset, so every tr16 address stays 8-byte aligned for all 25
// taps.  Why the single pitch-16 slab is enough (no 18-wide rows):
//   * w <= 13 (real pixel).  c = w + kw - 2 is in -2..15.
//       c in 0..13 : X holds x[h+kh-2][c], or zero when that image row is
//                    out of range (zero slab row) — the wanted value.
//       c = 14, 15 : the zero columns of the same slab row — the right halo.
//       c = -2, -1 : s lands on columns 14, 15 of slab row sr - 1 (linear
//                    wrap), zero — the left halo; for sr = 0 it lands in the
//                    front margin, zero.
//   * w = 14, 15 (padding k).  D[k] is zero; X[s] is some real pixel or a
//     zero, always finite staged data, and the product is an exact zero.
//   Range: s - MG = khl*16 + k + kw - 2 with khl <= KHB-1, k <= 223,
//   kw - 2 in -2..2 lies in [-2, (KHB-1)*16 + 225] = [-2, NRX*16 + 1]:
//   two margin pixels on each side are touched, MG = 8 are provided, and
//   everything in between is a staged slab row.  No read leaves the slab.
//
// Staging.  One glds wave-instruction writes 1 KB of LDS linearly: one X
// row of 16 pixels, or half a D row (8 pixels).  A 14-pixel image row is
// contiguous in global memory, so NRX + 28 glds stage an image (42 at
// KHB = 1), spread over the 4 waves.  The margins are zero-filled once.
//
// Bank swizzle.  ds_read_b64_tr_b16 is serviced per 32-lane half: two
// 16-lane groups, 8 rows apart, each reading 4 consecutive rows x 32 B.
// With 64 B rows the 4 rows cover 4 distinct 16-bank quarters but the
// second group aliases the first; with 128 B rows rows r and r+2 alias as
// well.  The 16-byte chunk index is therefore XORed with
//   X: ((s >> 3) & 1) << 1            D: (((k >> 1) & 1) | ((k >> 3) & 1) << 1) << 1
// (pairs of chunks, so an operand tile's 32 B stay together), on the glds
// SOURCE side (the LDS destination of glds is fixed) and in the tr16
// address.  Both depend on the row modulo 16 only, and every tap / k-step /
// kernel-row offset is a multiple of 16 rows plus a per-kw constant, so the
// swizzled fragment addresses are loop-invariant per lane.
//
// Waves: 2 x 2.  wr picks the ci half (16 rows of every tap), wc the co
// half (two 16-wide tiles): KHB*5*2 accumulators of 4 VGPRs per lane.
//
// A block accumulates G images in registers and flushes once with fp32
// atomics.  Shipped: KHB = 1, NBUF = 1 (165 VGPR, 44 KB LDS, 3 blocks/CU,
// no scratch).  KHB = 5 (200 AGPRs, 1 wave/SIMD) and NBUF = 2 (image g+1
// staged under image g's MFMAs, 88 KB LDS, 1 block/CU) were measured and
// lose at every G; they stay instantiated for tools/conv2_dw_sweep.py.
// Numbers: profiles/conv2_dw_slab_b1024_b8192.md.
//
// POOLED (KHB = 1, NBUF = 1 only).  `dact` is the pooled gradient gp
// [NB][7][7][64] and `am` the pool argmax bytes of the same shape; the dense
// pre-pool gradient exists only in D.  X is staged by glds as above.  D's 28
// glds jobs are replaced by 392 (window, 8-channel chunk) jobs over the 256
// lanes: one 16 B load of gp, one 8 B load of am, and for each of the four
// window positions k = (2wy+rr)*16 + 2wx+cc one 16 B LDS write of
// (am[e] == rr*2+cc ? gp[e] : 0) at D + k*128 + ((chunk ^ c2_dswz(k)) << 4)
// — the swizzle moves from the glds source side to the LDS destination, the
// tr16 fragment addresses do not change.
//   * Coverage.  49 windows x 4 positions are the 196 real rows k (h, w <=
//     13), 8 chunks each: every real byte of D is rewritten, zeros included,
//     with every image, so nothing is stale.
//   * Padding rows k = h*16 + 14, 15 are never touched by the decode (2wx+cc
//     <= 13); they are zero-filled ONCE per block before the first barrier.
//     The w = 14, 15 argument above then holds unchanged: D[k] is an exact
//     zero, X[s] is finite staged data (glds from the image or the zero
//     page), the product is an exact zero.
//   * Bounds.  k <= 13*16 + 13 = 221 < 224 rows; chunk ^ swz < 8; the global
//     reads are win*64 + chunk*8 + 0..7 < 3136 inside this image.  am only
//     feeds a compare, so any byte value is memory-safe (non-0..3 = dead).

#include "common.h"
#include "kernels.h"
#include <stdlib.h>
#include <stdexcept>

#define C2_MG 8            // margin pixels in front of / behind the X slab
#define C2_XIMG (14 * 14 * 32)
#define C2_DIMG (14 * 14 * 64)
#define C2_PIMG (7 * 7 * 64)   // pooled gradient / argmax bytes per image

static __device__ __align__(16) unsigned short c2_zero_page[8];  // zero-init

DEV int c2_xswz(int s) { return ((s >> 3) & 1) << 1; }
DEV int c2_dswz(int k) { return (((k >> 1) & 1) | (((k >> 3) & 1) << 1)) << 1; }

extern __shared__ __align__(16) ushort_t c2_lds[];

template <int KHB, int NBUF, bool POOLED = false, bool DET = false>
__global__ __launch_bounds__(256, (KHB == 1 && NBUF == 1) ? 3 : 1)
void conv2_dw_slab_kernel(const ushort_t* __restrict__ x,
                          const ushort_t* __restrict__ dact,
                          float* __restrict__ dw, int NB, int G,
                          const uint8_t* __restrict__ am) {
  static_assert(!POOLED || (KHB == 1 && NBUF == 1), "pooled: shipped form only");
  constexpr int NRX = 13 + KHB;                   // X slab rows
  constexpr int XPIX = C2_MG + NRX * 16 + C2_MG;  // X slab pixels
  constexpr int NJOB = POOLED ? NRX : NRX + 28;   // glds per image
  constexpr int NQ = (NJOB + 3) / 4;              // glds per wave per image
  constexpr int NKB = 5 / KHB;                    // blocks per image group
  constexpr int KS_UNROLL = KHB == 1 ? 7 : 1;
  constexpr int BUF = XPIX * 32 + 224 * 64;       // elements per buffer
  ushort_t* const X = c2_lds;                     // buffer b: X + b*BUF
  ushort_t* const D = c2_lds + XPIX * 32;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;

  // the NKB blocks of one image group sit on one XCD (flat % 8) back to
  // back, so dact / x are fetched from HBM once and re-read from that L2
  const int pos = blockIdx.x >> 3;
  const int grp = (pos / NKB) * 8 + (blockIdx.x & 7);
  const int kh0 = (pos % NKB) * KHB;
  const int img0 = grp * G;
  if (img0 >= NB) return;  // grid is rounded up to 8 groups; block-uniform

  // front / back margins of every buffer: 2 x 512 B each, written once
  if (tid < 64 * NBUF) {
    int t = tid & 63;
    int o = (t < 32) ? t * 8 : (C2_MG + NRX * 16) * 32 + (t - 32) * 8;
    *reinterpret_cast<short8*>(X + (tid >> 6) * BUF + o) =
        short8{0, 0, 0, 0, 0, 0, 0, 0};
  }

  // POOLED: columns 14, 15 of every D row, zero for the whole block
  if (POOLED && tid < 224) {
    int k = (tid >> 4) * 16 + 14 + ((tid >> 3) & 1);
    *reinterpret_cast<short8*>(D + k * 64 + (tid & 7) * 8) =
        short8{0, 0, 0, 0, 0, 0, 0, 0};
  }

  // ---- per-lane glds sources (element offset inside one image, -1 = zero)
  int soff[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    int j = wave + 4 * q;
    soff[q] = -1;
    if (j < NRX) {
      int ir = j + kh0 - 2, px = lane >> 2;
      int lc = (lane & 3) ^ c2_xswz(C2_MG + j * 16 + px);
      if (px < 14 && ir >= 0 && ir < 14) soff[q] = (ir * 14 + px) * 32 + lc * 8;
    } else if (j < NJOB) {
      int jj = j - NRX;
      int h = jj >> 1, px = (jj & 1) * 8 + (lane >> 3);
      int lc = (lane & 7) ^ c2_dswz(h * 16 + px);
      if (px < 14) soff[q] = (h * 14 + px) * 64 + lc * 8;
    }
  }
  const auto issue = [&](int buf, int img) {
    const ushort_t* xi = x + (size_t)img * C2_XIMG;
    const ushort_t* di = dact + (size_t)img * C2_DIMG;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      int j = wave + 4 * q;  // wave-uniform
      if (j < NRX) {
        const ushort_t* src = soff[q] >= 0 ? xi + soff[q] : c2_zero_page;
        glds16(src, X + buf * BUF + (C2_MG + j * 16) * 32);
      } else if (j < NJOB) {
        const ushort_t* src = soff[q] >= 0 ? di + soff[q] : c2_zero_page;
        glds16(src, D + buf * BUF + (j - NRX) * 8 * 64);
      }
    }
  };

  // ---- tr16 fragment addresses for k-step 0, kernel row kh0 ---------------
  // lane 4q+p of a 16-lane group addresses row kq + q, elements 4p..4p+3 of
  // the 16-wide tile (chunk p>>1, byte 8*(p&1)); the four groups take rows
  // 8*group.. of the 32-row k-step, the second read is 4 rows further down
  const int r0 = (lane >> 4) * 8 + ((lane & 15) >> 2);
  const int cp = (lane & 3) >> 1, off8 = (lane & 1) * 8;
  unsigned aaddr[5][2], baddr[2][2];
#pragma unroll
  for (int kw = 0; kw < 5; ++kw)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      int s = C2_MG + r0 + 4 * t + kw - 2;
      aaddr[kw][t] = (unsigned)(uintptr_t)X +
                     (unsigned)(s * 64 + (((wr * 2 + cp) ^ c2_xswz(s)) << 4) +
                                off8);
    }
#pragma unroll
  for (int ni = 0; ni < 2; ++ni)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      int k = r0 + 4 * t;
      baddr[ni][t] = (unsigned)(uintptr_t)D +
                     (unsigned)(k * 128 +
                                (((wc * 4 + ni * 2 + cp) ^ c2_dswz(k)) << 4) +
                                off8);
    }

  f32x4 acc[KHB][5][2];
#pragma unroll
  for (int a = 0; a < KHB; ++a)
#pragma unroll
    for (int b = 0; b < 5; ++b)
#pragma unroll
      for (int c = 0; c < 2; ++c) acc[a][b][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  // NBUF = 1: stage, wait, compute per image (latency hidden by the other
  // resident blocks).  NBUF = 2: image g+1 is in flight under image g's
  // MFMAs; the one barrier per image both publishes image g and retires
  // every wave's reads of the buffer image g+1 is about to overwrite.
  const int n = min(G, NB - img0);  // block-uniform
  if (NBUF == 2) issue(0, img0);
  for (int g = 0; g < n; ++g) {
    if (NBUF == 1) {
      __syncthreads();  // previous image's fragment reads done
      issue(0, img0 + g);
      if (POOLED) {
        const ushort_t* gi = dact + (size_t)(img0 + g) * C2_PIMG;
        const uint8_t* ai = am + (size_t)(img0 + g) * C2_PIMG;
        // both jobs' loads go out before the first select: one memory
        // round trip per image (job c covers elements c*8 .. c*8+7)
        short8 gv[2];
        uint2 av[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          int c = tid + j * 256;
          if (c < 49 * 8) {
            gv[j] = *reinterpret_cast<const short8*>(gi + c * 8);
            av[j] = *reinterpret_cast<const uint2*>(ai + c * 8);
          }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          int c = tid + j * 256;
          if (c < 49 * 8) {
            int chunk = c & 7, win = c >> 3;
            int wy = win / 7, wx = win - wy * 7;
#pragma unroll
            for (int pos = 0; pos < 4; ++pos) {
              int k = (2 * wy + (pos >> 1)) * 16 + 2 * wx + (pos & 1);
              *reinterpret_cast<short8*>(D + k * 64 +
                                         ((chunk ^ c2_dswz(k)) << 3)) =
                  pool_bwd_select(gv[j], av[j], pos);
            }
          }
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (NBUF == 2 && g + 1 < n) issue((g + 1) & 1, img0 + g + 1);
    const unsigned boff = (unsigned)((g & (NBUF - 1)) * BUF * 2);
#pragma unroll KS_UNROLL
    for (int ks = 0; ks < 7; ++ks) {
      uint2 br[2][2];
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int t = 0; t < 2; ++t)
          br[ni][t] = tr16_issue(baddr[ni][t] + boff + ks * (32 * 128));
#pragma unroll
      for (int khl = 0; khl < KHB; ++khl) {
        uint2 ar[5][2];
#pragma unroll
        for (int kw = 0; kw < 5; ++kw)
#pragma unroll
          for (int t = 0; t < 2; ++t)
            ar[kw][t] = tr16_issue(aaddr[kw][t] + boff +
                                   (ks * 32 + khl * 16) * 64);
        short8 af[5], bf[2];
#pragma unroll
        for (int kw = 0; kw < 5; ++kw) af[kw] = pack_wait(ar[kw][0], ar[kw][1]);
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) bf[ni] = pack_wait(br[ni][0], br[ni][1]);
#pragma unroll
        for (int kw = 0; kw < 5; ++kw)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
            acc[khl][kw][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                af[kw], bf[ni], acc[khl][kw][ni], 0, 0, 0);
      }
    }
  }

  // flush: C tile row = (lane>>4)*4 + r, column = lane & 15
  const int frow = (lane >> 4) * 4, fcol = lane & 15;
#pragma unroll
  for (int khl = 0; khl < KHB; ++khl)
#pragma unroll
    for (int kw = 0; kw < 5; ++kw)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int m = ((kh0 + khl) * 5 + kw) * 32 + wr * 16 + frow + r;
          int n = wc * 32 + ni * 16 + fcol;
          if (DET)  // deterministic mode: dw is this group's private plane
            dw[(size_t)grp * CONV2_DET_PLANE + m * 64 + n] =
                acc[khl][kw][ni][r];
          else
            atomicAdd(dw + m * 64 + n, acc[khl][kw][ni][r]);
        }
}

// ---- host side -------------------------------------------------------------

bool conv2_dw_slab_supported(int H, int W, int Cin, int Cout) {
  return H == 14 && W == 14 && Cin == 32 && Cout == 64;
}

// DMNIST_DW2_SLAB=0 routes the shape back to conv_dw_tr (read on every call
// so the two kernels can be compared in one process)
bool conv2_dw_slab_enabled() {
  const char* e = getenv("DMNIST_DW2_SLAB");
  return !(e && atoi(e) == 0);
}

// Images per block.  The flush (10 240 fp32 atomics per block) is paid once
// per G images and is the dominant cost at small G; at large G too few
// blocks are left to hide the per-image staging latency.  Measured optimum
// 12 at NB=1024 and 20..32 at NB=8192 (profiles/conv2_dw_slab_b1024_b8192.md);
// the tiers below 512 are not measured and only keep >= ~300 blocks.
int conv2_dw_group(int NB) {
  int G = NB >= 4096 ? 32 : (NB >= 512 ? 12 : (NB >= 128 ? 4 : 1));
  if (const char* e = getenv("DMNIST_DW2_G")) G = atoi(e);  // flush sweep
  return G < 1 ? 1 : G;
}

template <int KHB, int NBUF, bool POOLED = false, bool DET = false>
static void c2_launch(const unsigned short* x, const unsigned short* dact,
                      float* dw, int NB, int G, int blocks, hipStream_t s,
                      const uint8_t* am = nullptr) {
  constexpr int BYTES = NBUF * ((C2_MG * 2 + (13 + KHB) * 16) * 32 + 224 * 64) * 2;
  if (BYTES > 65536) {
    // above 64 KB the dynamic LDS size has to be granted once per kernel
    static const hipError_t granted = hipFuncSetAttribute(
        reinterpret_cast<const void*>(
            &conv2_dw_slab_kernel<KHB, NBUF, POOLED, DET>),
        hipFuncAttributeMaxDynamicSharedMemorySize, BYTES);
    if (granted != hipSuccess)
      throw std::runtime_error("conv2_dw_slab: LDS size not granted");
  }
  hipLaunchKernelGGL((conv2_dw_slab_kernel<KHB, NBUF, POOLED, DET>), dim3(blocks),
                     dim3(256), BYTES, s, x, dact, dw, NB, G, am);
}

void launch_conv2_dw_slab(const unsigned short* x, const unsigned short* dact,
                          float* dw, int NB, hipStream_t s) {
  if (NB <= 0) return;
  int G = conv2_dw_group(NB);
  int groups = (NB + G - 1) / G;
  int g8 = (groups + 7) / 8 * 8;
  // sweep switches: DMNIST_DW2_KHB=5 all 25 taps in one block,
  // DMNIST_DW2_NBUF=1|2 single- / double-buffered slabs
  const char* e = getenv("DMNIST_DW2_KHB");
  const char* b = getenv("DMNIST_DW2_NBUF");
  bool all_taps = e && atoi(e) == 5;
  int nbuf = b ? atoi(b) : 1;
  if (all_taps && nbuf == 2)
    c2_launch<5, 2>(x, dact, dw, NB, G, g8, s);
  else if (all_taps)
    c2_launch<5, 1>(x, dact, dw, NB, G, g8, s);
  else if (nbuf == 2)
    c2_launch<1, 2>(x, dact, dw, NB, G, g8 * 5, s);
  else
    c2_launch<1, 1>(x, dact, dw, NB, G, g8 * 5, s);
}

// conv2 dW from the pooled gradient gp and the pool argmax bytes am (the
// POOLED staging): same G tiers and XCD grouping as the dense launcher
void launch_conv2_dw_slab_pooled(const unsigned short* x,
                                 const unsigned short* gp, const uint8_t* am,
                                 float* dw, int NB, hipStream_t s) {
  if (NB <= 0) return;
  int G = conv2_dw_group(NB);
  int groups = (NB + G - 1) / G;
  int g8 = (groups + 7) / 8 * 8;
  c2_launch<1, 1, true>(x, gp, dw, NB, G, g8 * 5, s, am);
}

// deterministic mode: the same kernels storing one plane per image group
int conv2_dw_groups(int NB) {
  int G = conv2_dw_group(NB);
  return NB <= 0 ? 0 : (NB + G - 1) / G;
}

void launch_conv2_dw_slab_det(const unsigned short* x,
                              const unsigned short* dact, float* planes,
                              int NB, hipStream_t s) {
  if (NB <= 0) return;
  int g8 = (conv2_dw_groups(NB) + 7) / 8 * 8;
  c2_launch<1, 1, false, true>(x, dact, planes, NB, conv2_dw_group(NB),
                               g8 * 5, s);
}

void launch_conv2_dw_slab_pooled_det(const unsigned short* x,
                                     const unsigned short* gp,
                                     const uint8_t* am, float* planes, int NB,
                                     hipStream_t s) {
  if (NB <= 0) return;
  int g8 = (conv2_dw_groups(NB) + 7) / 8 * 8;
  c2_launch<1, 1, true, true>(x, gp, planes, NB, conv2_dw_group(NB), g8 * 5,
                              s, am);
}
