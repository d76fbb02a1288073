// Persistent, weight-resident conv2 forward and dX kernels (gfx950).
//
// The per-image slab kernels in conv_slab.hip stream the whole conv2 weight
// tensor (25 x 32 x 64 bf16 = 102 400 B) from L2 into LDS once PER IMAGE, in
// 64-wide K tiles that each sit behind a block-wide barrier.  The weights are
// the same for every image of a launch, and gfx950 has 160 KB of LDS per CU:
// weights and one image slab fit together.  These kernels launch one block
// per CU, stage the weights ONCE per block, and walk images blockIdx.x,
// blockIdx.x + gridDim.x, ...  Per image: stage the slab, one barrier, all
// K-steps with no barrier and no global traffic, epilogue, one barrier.
//
// Numerics: one fp32 accumulator per output element, v_mfma_f32_16x16x32_bf16
// in ascending k, K never split across waves — the MFMA sequence every output
// element sees is the one conv_slab.hip issues, so y, amax and dx are bitwise
// the same.  (The old forward's zero-padded K tail adds +0 products to an
// accumulator that is never -0, which changes no bit; here K is exactly
// 25 x 32 and the tail does not exist.)
//
// Wave layout: the 13 real 16-row M fragments of an image (196 rows) are
// dealt round-robin to the NW waves; a wave owns ALL N fragments of its rows
// (NI = 2 for dX, 4 for forward), so each A fragment is read from LDS once
// and feeds every N fragment.  Fragment 13 of the old BM = 224 tile held pad
// rows only and is not computed.
//
// LDS layout (dynamic, granted with hipFuncAttributeMaxDynamicSharedMemorySize):
//   dX : Wl[32][1608] n-major (102 912 B) | slab[324][72] (46 656 B)
//        -> 149 568 B
//   fwd: Wl[800][64] k-major, chunk-swizzled (102 400 B) | slab[324][40]
//        (25 920 B) -> 128 320 B
// both under the 163 840 B of a CU; a static_assert holds them there.
//
// Bank argument for the dX B-fragment reads (ds_read_b128, 64 banks x 4 B =
// 16 units of 16 B per LDS row): the 16 lanes of a fragment row group read 16
// consecutive n rows at the same k.  The n-row stride is 1608 x 2 B = 201
// units, and 201 mod 16 = 9 is odd, so the 16 lanes land on 16 distinct
// 16 B units — conflict-free whether the hardware serves a b128 in groups of
// 8 or of 16 lanes.  (An unpadded 3200 B row is 200 units = 8 mod 16: an
// 8-way conflict.)  The forward keeps the k-major tile of conv_slab.hip with
// its per-row chunk XOR, so its ds_read_b64_tr_b16 addresses are those of the
// old kernel with the tile offset folded into the row.
//
// Hazards, and how each is designed out:
//  * LDS reads stay inside the allocation and read initialised data.  The
//    whole slab (halo ring, interior, pad columns) is zero-filled once per
//    block; the interior is fully rewritten for every image (all four window
//    positions for dX, all 196 pixels for forward).  A-fragment rows past 196
//    are clamped to pixel (0, 0) and read real slab bytes (NaN x 0 is NaN);
//    tap shifts keep every padded coordinate in 0..17.  The largest B read
//    is element 31*1608 + 1599 of Wl (dX) and row 799 (forward).
//  * A block with no image exits before it touches LDS.  No cross-block
//    synchronisation, no spinning, no tickets.
//  * The barrier between the MFMA loop of image i and the slab writes of
//    image i+1 is the explicit __syncthreads() at the bottom of the image
//    loop; `nxt` is block-uniform, so every thread reaches the same barriers.
//  * The next image's global loads are issued before the MFMA loop into
//    registers and written to LDS after that barrier (PF); nothing in the
//    loop waits on them.
//  * The forward's transposed B reads (ds_read_b64_tr_b16) are inline asm
//    whose result registers the hardware writes up to one K-step AFTER the
//    statement: fwd_mainloop issues step ks+1's reads before step ks's MFMAs
//    and drains them with wait_tr16x8 at the top of the next step.  The
//    compiler does not know the registers are still in flight.  What is
//    enforced: every consumer takes them through wait_tr16x8's "+v" operands,
//    so no use can be scheduled before the wait.  What is NOT enforced: that
//    the register allocator never copies or spills such a register between
//    the issue and the wait.  It does not today (122 / 142 VGPR, no scratch;
//    the issue-to-wait values are plain 64-bit pairs with no tuple
//    constraint), and the bitwise tests would show it, but a compiler change
//    could break it silently.  pack_wait in common.h drains within one step
//    and carries no such risk.  This is one reason the forward kernel is off
//    by default.
//
// Measured and dropped (profiles/conv2_resident_b1024_b8192.md): staging the
// output tile through wave-private LDS to store 16 B per lane.  It changed
// dX by under 1 % and made the forward 2 to 6 % slower, so both epilogues
// store per accumulator element as conv_slab.hip does.

#include "common.h"
#include "kernels.h"
#include <stdlib.h>
#include <string.h>
#include <stdexcept>

typedef ushort_t u16;

namespace {

constexpr int RH = 14, RW = 14, RHP = 18, RWP = 18;
constexpr int RCIN = 32, RCOUT = 64;
constexpr int RM = RH * RW;          // 196 rows per image
constexpr int RFRAG = 13;            // real 16-row fragments
constexpr int LDS_LIMIT = 160 * 1024;

}  // namespace

extern __shared__ __align__(16) ushort_t c2r_lds[];

// target builtins stay out of the templates (see common.h)
DEV int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
DEV f32x4 mfma_bf16(short8 a, short8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// ---------------------------------------------------------------------------
// dX: dx[hi,wi,ci] = sum_{kh,kw,co} dact[hi-kh+2, wi-kw+2, co] * w[kh,kw,ci,co]
// dact is rebuilt in the slab from (gp, am) as conv_dx_slab_kernel<POOLED>.
// ---------------------------------------------------------------------------
constexpr int DX_K = 25 * RCOUT;        // 1600
constexpr int DX_WLD = DX_K + 8;        // n-row stride, see the bank argument
constexpr int DX_PST = RCOUT + 8;       // 144 B pixel stride (conv_slab.hip)
constexpr int DX_NWJ = 49 * (RCOUT / 8);  // (window, 8-channel chunk) jobs

template <int MI, int MJ>
DEV void dx_mainloop(const u16* slab, const u16* Wl, const int (&aoff)[MJ],
                     f32x4 (&acc)[MJ][2], int lane) {
  const int kq = (lane >> 4) * 8;
  const u16* bp = Wl + (lane & 15) * DX_WLD + kq;
  short8 a0[MI], b0[2];
  const auto load = [&](int ks, short8 (&a)[MI], short8 (&b)[2]) {
    int khkw = ks >> 1, co = (ks & 1) * 32 + kq;   // k = khkw*64 + co
    int kh = khkw / 5, kw = khkw % 5;
    int shift = (-(kh - 2) * RWP - (kw - 2)) * DX_PST + co;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
      a[mi] = *reinterpret_cast<const short8*>(slab + aoff[mi] + shift);
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
      b[ni] = *reinterpret_cast<const short8*>(bp + ni * 16 * DX_WLD + ks * 32);
  };
  load(0, a0, b0);
#pragma unroll
  for (int ks = 0; ks < 50; ++ks) {
    short8 a1[MI], b1[2];
    if (ks + 1 < 50) load(ks + 1, a1, b1);   // in flight under the MFMAs
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        acc[mi][ni] = mfma_bf16(a0[mi], b0[ni], acc[mi][ni]);
    if (ks + 1 < 50) {
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) a0[mi] = a1[mi];
      b0[0] = b1[0]; b0[1] = b1[1];
    }
  }
}

template <int NW, bool PF>
__global__ __launch_bounds__(NW * 64)
void conv2_dx_resident_kernel(const u16* __restrict__ gp,
                              const uint8_t* __restrict__ am,
                              const u16* __restrict__ w,  // [25][32][64]
                              u16* __restrict__ dx, int NB) {
  constexpr int NT = NW * 64;
  constexpr int MJ = (RFRAG + NW - 1) / NW;      // fragments of wave 0
  constexpr int NJ = (DX_NWJ + NT - 1) / NT;
  u16* Wl = c2r_lds;                             // [32][DX_WLD]
  u16* slab = Wl + RCIN * DX_WLD;                // [18*18][DX_PST]

  int img = blockIdx.x;
  if (img >= NB) return;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = wave_uniform(tid >> 6);

  // weights, once: job c = (khkw, ci, 8-co chunk) is 16 B at w + c*8
  for (int c = tid; c < 25 * RCIN * (RCOUT / 8); c += NT) {
    int ch = c & 7, ci = (c >> 3) & 31, khkw = c >> 8;
    *reinterpret_cast<short8*>(Wl + ci * DX_WLD + khkw * RCOUT + ch * 8) =
        *reinterpret_cast<const short8*>(w + (size_t)c * 8);
  }
  for (int c = tid; c < RHP * RWP * DX_PST / 8; c += NT)
    *reinterpret_cast<short8*>(slab + c * 8) = short8{0, 0, 0, 0, 0, 0, 0, 0};
  __syncthreads();  // zero fill lands before other threads' interior writes

  int aoff[MJ];
#pragma unroll
  for (int j = 0; j < MJ; ++j) {
    int lm = (wave + j * NW) * 16 + (lane & 15);
    int wi = lm % RW, hi = lm / RW;
    if (lm >= RM) { wi = 0; hi = 0; }
    aoff[j] = ((hi + 2) * RWP + (wi + 2)) * DX_PST;
  }
  const bool last_frag = wave + (MJ - 1) * NW < RFRAG;   // wave-uniform

  short8 g[NJ];
  uint2 a[NJ];
  const auto load_img = [&](int im) {
    const u16* gi = gp + (size_t)im * DX_NWJ * 8;
    const uint8_t* ai = am + (size_t)im * DX_NWJ * 8;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      int c = tid + j * NT;
      if (c < DX_NWJ) {
        g[j] = *reinterpret_cast<const short8*>(gi + (size_t)c * 8);
        a[j] = *reinterpret_cast<const uint2*>(ai + (size_t)c * 8);
      }
    }
  };
  load_img(img);

  for (;;) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      int c = tid + j * NT;
      if (c < DX_NWJ) {
        int co = (c & 7) * 8;
        int win = c >> 3;
        int wx = win % 7, wy = win / 7;
#pragma unroll
        for (int pos = 0; pos < 4; ++pos) {
          int yy = 2 * wy + (pos >> 1) + 2, xx = 2 * wx + (pos & 1) + 2;
          *reinterpret_cast<short8*>(slab + (yy * RWP + xx) * DX_PST + co) =
              pool_bwd_select(g[j], a[j], pos);
        }
      }
    }
    __syncthreads();  // slab (first image: weights too) visible to all waves
    const int nxt = img + gridDim.x;
    if (PF && nxt < NB) load_img(nxt);

    f32x4 acc[MJ][2];
#pragma unroll
    for (int j = 0; j < MJ; ++j)
      acc[j][0] = acc[j][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (last_frag) dx_mainloop<MJ, MJ>(slab, Wl, aoff, acc, lane);
    else if (MJ > 1) dx_mainloop<(MJ > 1 ? MJ - 1 : 1), MJ>(slab, Wl, aoff, acc, lane);

    const int frow = (lane >> 4) * 4;
    const int fcol = lane & 15;
    u16* xo = dx + (size_t)img * RM * RCIN;
#pragma unroll
    for (int j = 0; j < MJ; ++j) {
      int mi = wave + j * NW;
      if (mi >= RFRAG) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int lm = mi * 16 + frow + r;
        if (lm >= RM) continue;
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          xo[(size_t)lm * RCIN + ni * 16 + fcol] = f2bf(acc[j][ni][r]);
      }
    }
    if (nxt >= NB) break;
    __syncthreads();  // every wave is done reading image i's slab
    if (!PF) load_img(nxt);
    img = nxt;
  }
}

// ---------------------------------------------------------------------------
// forward: y = maxpool(relu(conv5x5(x) + b)), amax = argmax byte (7 = dead)
// ---------------------------------------------------------------------------
constexpr int FW_PST = RCIN + 8;         // 80 B pixel stride (conv_slab.hip)
constexpr int FW_NJOB = RM * (RCIN / 8); // (pixel, 8-channel chunk) jobs

// drain every outstanding LDS read; the eight transposed-read results are
// operands, so nothing that consumes them can be placed before the wait
DEV void wait_tr16x8(uint2 (&br)[4][2]) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(br[0][0]), "+v"(br[0][1]), "+v"(br[1][0]), "+v"(br[1][1]),
                 "+v"(br[2][0]), "+v"(br[2][1]), "+v"(br[3][0]), "+v"(br[3][1]));
}
DEV short8 pack8(uint2 lo, uint2 hi) {
  union { unsigned u[4]; short8 s; } r;
  r.u[0] = lo.x; r.u[1] = lo.y; r.u[2] = hi.x; r.u[3] = hi.y;
  return r.s;
}

// One wave per SIMD has no neighbour to cover LDS latency, so both operands
// of K-step ks+1 are issued before the MFMAs of K-step ks.  The transposed
// B reads are inline asm the compiler does not track: they are drained by
// wait_tr16x8 at the top of the next step, before anything touches them.
template <int MI, int MJ>
DEV void fwd_mainloop(const u16* slab, const u16* Wl, const int (&aoff)[MJ],
                      f32x4 (&acc)[MJ][4], int lane) {
  const int kq = (lane >> 4) * 8;
  const int slot_r = (lane & 15) >> 2;   // tr16 slot addressing (see dw_tr)
  const int slot_c = (lane & 3) * 4;
  const unsigned wbase = (unsigned)(uintptr_t)Wl;
  short8 a0[MI];
  uint2 br[4][2];
  const auto load = [&](int ks, short8 (&a)[MI]) {   // ks = khkw, k = ks*32 + ci
    int kh = ks / 5, kw = ks % 5;
    int shift = ((kh - 2) * RWP + (kw - 2)) * FW_PST + kq;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
      a[mi] = *reinterpret_cast<const short8*>(slab + aoff[mi] + shift);
  };
  // B address = tbase[ks & 1][ni][half] + (ks >> 1) * 8192 B: the chunk XOR
  // of row r = ks*32 + kq + slot_r (+4) depends on ks only through its
  // parity ((r >> 3) & 7 = (4*ks + lane/16) & 7), so 16 address registers
  // serve all 25 K-steps and the rest rides in the instruction's 16-bit
  // offset field (second base 64 KB up from K-step 16 on).
  unsigned tbase[2][4][2];
#pragma unroll
  for (int par = 0; par < 2; ++par)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        int cb = (ni * 16 + slot_c) * 2;
        int r = par * 32 + kq + slot_r + h * 4;
        int xs = (r ^ (r >> 3)) & 7;
        tbase[par][ni][h] = wbase + (unsigned)(r * (RCOUT * 2) +
                                (((cb >> 4) ^ xs) << 4) + (cb & 15));
      }
#define C2R_TR16(d, addr, off)                                   \
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"             \
               : "=&v"(d) : "v"(addr), "i"(off) : "memory")
  const auto issueB = [&](int ks) {
    const int hi = ks >= 16;
    const int off = (ks >> 1) * 8192 - hi * 65536;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int h = 0; h < 2; ++h)
        C2R_TR16(br[ni][h], tbase[ks & 1][ni][h] + (hi ? 65536u : 0u), off);
  };
  issueB(0);
  load(0, a0);
#pragma unroll
  for (int ks = 0; ks < 25; ++ks) {
    wait_tr16x8(br);
    short8 bf[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) bf[ni] = pack8(br[ni][0], br[ni][1]);
    short8 a1[MI];
    if (ks + 1 < 25) {
      issueB(ks + 1);
      load(ks + 1, a1);
    }
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        acc[mi][ni] = mfma_bf16(a0[mi], bf[ni], acc[mi][ni]);
    if (ks + 1 < 25) {
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) a0[mi] = a1[mi];
    }
  }
#undef C2R_TR16
}

template <int NW, bool PF>
__global__ __launch_bounds__(NW * 64)
void conv2_fwd_resident_kernel(const u16* __restrict__ x,
                               const u16* __restrict__ w,  // [800][64] k-major
                               const float* __restrict__ bias,
                               u16* __restrict__ y, uint8_t* __restrict__ amax,
                               int NB) {
  constexpr int NT = NW * 64;
  constexpr int MJ = (RFRAG + NW - 1) / NW;
  constexpr int NJ = (FW_NJOB + NT - 1) / NT;
  u16* Wl = c2r_lds;                             // [800][64], chunk-swizzled
  u16* slab = Wl + 25 * RCIN * RCOUT;            // [18*18][FW_PST]

  int img = blockIdx.x;
  if (img >= NB) return;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = wave_uniform(tid >> 6);

  // weights, once: physical 16 B chunk p of row r holds logical chunk
  // p ^ xs(r), the swizzle the tr16 fragment reads undo
  for (int c = tid; c < 25 * RCIN * (RCOUT / 8); c += NT) {
    int p = c & 7, r = c >> 3;
    int xs = (r ^ (r >> 3)) & 7;
    *reinterpret_cast<short8*>(Wl + r * RCOUT + p * 8) =
        *reinterpret_cast<const short8*>(w + (size_t)r * RCOUT + (p ^ xs) * 8);
  }
  for (int c = tid; c < RHP * RWP * FW_PST / 8; c += NT)
    *reinterpret_cast<short8*>(slab + c * 8) = short8{0, 0, 0, 0, 0, 0, 0, 0};
  __syncthreads();  // zero fill lands before other threads' interior writes

  // row lm -> conv-output pixel, pool-grouped (lm = window*4 + pos)
  int aoff[MJ];
#pragma unroll
  for (int j = 0; j < MJ; ++j) {
    int lm = (wave + j * NW) * 16 + (lane & 15);
    int q = lm >> 2, pos = lm & 3;
    int wo = q % 7, ho = q / 7;
    if (lm >= RM) { wo = 0; ho = 0; pos = 0; }
    int oy = ho * 2 + (pos >> 1) + 2, ox = wo * 2 + (pos & 1) + 2;
    aoff[j] = (oy * RWP + ox) * FW_PST;
  }
  const bool last_frag = wave + (MJ - 1) * NW < RFRAG;   // wave-uniform

  const int fcol = lane & 15;
  float bias_v[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) bias_v[ni] = bias[ni * 16 + fcol];

  short8 xr[NJ];
  const auto load_img = [&](int im) {
    const u16* xi = x + (size_t)im * FW_NJOB * 8;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      int c = tid + j * NT;
      if (c < FW_NJOB)
        xr[j] = *reinterpret_cast<const short8*>(xi + (size_t)c * 8);
    }
  };
  load_img(img);

  for (;;) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      int c = tid + j * NT;
      if (c < FW_NJOB) {
        int ci = (c & 3) * 8, pix = c >> 2;
        int sx = pix % RW, sy = pix / RW;
        *reinterpret_cast<short8*>(
            slab + ((sy + 2) * RWP + sx + 2) * FW_PST + ci) = xr[j];
      }
    }
    __syncthreads();  // slab (first image: weights too) visible to all waves
    const int nxt = img + gridDim.x;
    if (PF && nxt < NB) load_img(nxt);

    f32x4 acc[MJ][4];
#pragma unroll
    for (int j = 0; j < MJ; ++j)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[j][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (last_frag) fwd_mainloop<MJ, MJ>(slab, Wl, aoff, acc, lane);
    else if (MJ > 1) fwd_mainloop<(MJ > 1 ? MJ - 1 : 1), MJ>(slab, Wl, aoff, acc, lane);

    // pool epilogue: a lane's 4 accumulator rows are one 2x2 window
    u16* yi = y + (size_t)img * 49 * RCOUT;
    uint8_t* ai = amax + (size_t)img * 49 * RCOUT;
#pragma unroll
    for (int j = 0; j < MJ; ++j) {
      int mi = wave + j * NW;
      if (mi >= RFRAG) continue;
      int gq = mi * 4 + (lane >> 4);      // window of this lane
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        int gc = ni * 16 + fcol;
        float best = -1.0f / 0.0f;
        int barg = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = acc[j][ni][r] + bias_v[ni];
          v = v > 0.f ? v : 0.f;
          if (v > best) { best = v; barg = r; }
        }
        if (gq < 49) {
          yi[(size_t)gq * RCOUT + gc] = f2bf(best);
          // liveness rides in the argmax byte: 7 = dead window
          ai[(size_t)gq * RCOUT + gc] = (uint8_t)(best > 0.f ? barg : 7);
        }
      }
    }
    if (nxt >= NB) break;
    __syncthreads();  // every wave is done reading image i's slab
    if (!PF) load_img(nxt);
    img = nxt;
  }
}

// ---- host side -------------------------------------------------------------
namespace {

int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e && *e ? atoi(e) : dflt;
}

constexpr int dx_lds_bytes() {
  return (RCIN * DX_WLD + RHP * RWP * DX_PST) * 2;
}
constexpr int fwd_lds_bytes() {
  return (25 * RCIN * RCOUT + RHP * RWP * FW_PST) * 2;
}
static_assert(dx_lds_bytes() <= LDS_LIMIT && fwd_lds_bytes() <= LDS_LIMIT,
              "resident conv2 kernels must fit the 160 KB of a gfx950 CU");

template <int NW, bool PF>
void dx_launch(const u16* gp, const uint8_t* am, const u16* w, u16* dx, int NB,
               int blocks, hipStream_t s) {
  constexpr int BYTES = dx_lds_bytes();
  static const hipError_t granted = hipFuncSetAttribute(
      reinterpret_cast<const void*>(&conv2_dx_resident_kernel<NW, PF>),
      hipFuncAttributeMaxDynamicSharedMemorySize, BYTES);
  if (granted != hipSuccess)
    throw std::runtime_error("conv2_dx_resident: LDS size not granted");
  hipLaunchKernelGGL((conv2_dx_resident_kernel<NW, PF>), dim3(blocks),
                     dim3(NW * 64), BYTES, s, gp, am, w, dx, NB);
}

template <int NW, bool PF>
void fwd_launch(const u16* x, const u16* w, const float* bias, u16* y,
                uint8_t* amax, int NB, int blocks, hipStream_t s) {
  constexpr int BYTES = fwd_lds_bytes();
  static const hipError_t granted = hipFuncSetAttribute(
      reinterpret_cast<const void*>(&conv2_fwd_resident_kernel<NW, PF>),
      hipFuncAttributeMaxDynamicSharedMemorySize, BYTES);
  if (granted != hipSuccess)
    throw std::runtime_error("conv2_fwd_resident: LDS size not granted");
  hipLaunchKernelGGL((conv2_fwd_resident_kernel<NW, PF>), dim3(blocks),
                     dim3(NW * 64), BYTES, s, x, w, bias, y, amax, NB);
}

// one block per CU; DMNIST_CONV2_RES_BLOCKS=n caps the grid (tests, sweeps)
int resident_blocks(int NB) {
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess)
    throw std::runtime_error("conv2 resident: no device");
  int n = 0;
  if (dev >= 0 && dev < 64) n = cus[dev];
  if (n <= 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount,
                              dev) != hipSuccess || n <= 0)
      throw std::runtime_error("conv2 resident: no CU count");
    if (dev >= 0 && dev < 64) cus[dev] = n;
  }
  int cap = env_int("DMNIST_CONV2_RES_BLOCKS", 0);
  if (cap > 0 && cap < n) n = cap;
  return NB < n ? NB : n;
}

}  // namespace

// Route, decided here for both ops and read on every call.
// DMNIST_CONV2_RESIDENT: unset = the measured default (dX resident, forward
// per-image: the forward kernel wins solo but not inside the step), 0 = both
// per-image, fwd / dx = that resident kernel only, both = both resident; any
// other value is an error.  The NB tier is measured
// (profiles/conv2_resident_b1024_b8192.md).  DMNIST_CONV2_RES_MIN_NB=n
// (a positive integer, anything else is an error) replaces the tier of
// whichever op is enabled; it is a hook for the tests and the sweep tool.
bool conv2_resident_route(int op, int NB) {
  const char* e = getenv("DMNIST_CONV2_RESIDENT");
  bool on = op == CONV2_RES_DX;
  if (e && *e) {
    if (!strcmp(e, "0")) on = false;
    else if (!strcmp(e, "fwd")) on = op == CONV2_RES_FWD;
    else if (!strcmp(e, "dx")) on = op == CONV2_RES_DX;
    else if (!strcmp(e, "both")) on = true;
    else throw std::runtime_error(
        "DMNIST_CONV2_RESIDENT must be 0, fwd, dx or both");
  }
  if (!on) return false;
  int min_nb = CONV2_RES_MIN_NB;
  const char* m = getenv("DMNIST_CONV2_RES_MIN_NB");
  if (m && *m) {
    char* end = nullptr;
    long v = strtol(m, &end, 10);
    if (*end || v < 1 || v > (1 << 30))
      throw std::runtime_error(
          "DMNIST_CONV2_RES_MIN_NB must be a positive integer");
    min_nb = (int)v;
  }
  return NB >= min_nb;
}

// sweep switches: DMNIST_CONV2_RES_WAVES=4|8, DMNIST_CONV2_RES_PF=0|1 (next
// image's loads under the MFMA loop)
void launch_conv2_dx_resident(const unsigned short* gp, const uint8_t* am,
                              const unsigned short* w, unsigned short* dx,
                              int NB, hipStream_t s) {
  if (NB <= 0) return;
  int blocks = resident_blocks(NB);
  bool w8 = env_int("DMNIST_CONV2_RES_WAVES", CONV2_RES_WAVES) == 8;
  bool pf = env_int("DMNIST_CONV2_RES_PF", 1) != 0;
  if (w8 && pf) dx_launch<8, true>(gp, am, w, dx, NB, blocks, s);
  else if (w8) dx_launch<8, false>(gp, am, w, dx, NB, blocks, s);
  else if (pf) dx_launch<4, true>(gp, am, w, dx, NB, blocks, s);
  else dx_launch<4, false>(gp, am, w, dx, NB, blocks, s);
}

void launch_conv2_fwd_resident(const unsigned short* x, const unsigned short* w,
                               const float* bias, unsigned short* y,
                               uint8_t* amax, int NB, hipStream_t s) {
  if (NB <= 0) return;
  int blocks = resident_blocks(NB);
  bool w8 = env_int("DMNIST_CONV2_RES_WAVES", CONV2_RES_WAVES) == 8;
  bool pf = env_int("DMNIST_CONV2_RES_PF", 1) != 0;
  if (w8 && pf) fwd_launch<8, true>(x, w, bias, y, amax, NB, blocks, s);
  else if (w8) fwd_launch<8, false>(x, w, bias, y, amax, NB, blocks, s);
  else if (pf) fwd_launch<4, true>(x, w, bias, y, amax, NB, blocks, s);
  else fwd_launch<4, false>(x, w, bias, y, amax, NB, blocks, s);
}
