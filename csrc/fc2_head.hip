// fc2 head: the whole 512 -> 10 classifier layer of the training step in one
// launch — fc2 forward (+bias), softmax cross-entropy (+db2, loss, accuracy),
// fc2 dX with the fc1 relu/dropout mask (+db1) and fc2 dW.  Everything but
// the batch reductions is row-local, so a block that holds R rows of a1 in
// LDS reads a1 once and neither the logits nor dlogits ever reach memory.
// docs/KERNELS.md, "fc2 head".
//
// Block: R rows as R / 16 groups of 16, FC2H_WPG waves per group (the kernel
// is a chain of short latency-bound stages, so each stage is spread over as
// many waves as it has independent pieces).  All matrix products run on
// v_mfma_f32_16x16x32_bf16 (A: lane l holds A[l & 15][8 (l >> 4) + j], B:
// B[8 (l >> 4) + j][l & 15], C/D: row 4 (l >> 4) + reg, column l & 15); the
// 10 classes are padded to 16 (and, as a reduction axis, to 32) with zeros.
// No block waits on another: the only cross-block step is the softmax
// kernel's last-block ticket.

#include "common.h"
#include "kernels.h"

// LDS row pitch (elements): 16 B slots advance by two per row, which keeps
// every ds_read_b128 lane group of the row-major MFMA operand reads on 16
// distinct slots of the 256 B bank row
#define FC2H_PITCH (FC2_HEAD_K + 16)
#define FC2H_C 10
#define FC2H_WPG 4  // waves per 16-row group

// sum over the 16 lanes of a DPP row (row_ror 8, 4, 2, 1), left in every lane
DEV float row_sum16(float x) {
#define FC2H_ROR(n)                                                         \
  x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(               \
           0, __builtin_bit_cast(int, x), 0x120 + (n), 0xf, 0xf, false))
  FC2H_ROR(8);
  FC2H_ROR(4);
  FC2H_ROR(2);
  FC2H_ROR(1);
#undef FC2H_ROR
  return x;
}

template <int R>
__global__ __launch_bounds__(R * 4 * FC2H_WPG)
void fc2_head_kernel(const ushort_t* a1, const ushort_t* w2T, const float* b2,
                     const long* labels, ushort_t* dyeff, float* dw2,
                     float* db2, float* db1, float* out, int B,
                     float inv_keep, float inv_n, float* part,
                     unsigned* ticket) {
  constexpr int K = FC2_HEAD_K;  // compile time: every loop below unrolls
  constexpr int C = FC2H_C;
  constexpr int WPG = FC2H_WPG;
  constexpr int NG = R / 16;    // row groups
  constexpr int NW = NG * WPG;  // waves
  constexpr int NT = NW * 64;   // threads
  static_assert(K == 512, "a row is 64 chunks of 16 B: one per lane");
  static_assert(NT <= 1024 && 1024 % NT == 0 && (K / 16) % NW == 0, "split");
  __shared__ __attribute__((aligned(16))) ushort_t a_s[R][FC2H_PITCH];
  __shared__ __attribute__((aligned(16))) ushort_t wT_s[16][FC2H_PITCH];
  __shared__ __attribute__((aligned(16))) ushort_t wp_s[K][16];
  __shared__ __attribute__((aligned(16))) ushort_t lg_s[R][16];
  __shared__ __attribute__((aligned(16))) ushort_t dl_s[R][16];
  __shared__ float db2_s[NG][16];
  __shared__ float lc_s[NG][2];
  __shared__ __attribute__((aligned(16))) float db1_s[NG][K];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;
  const int grp = wv / WPG, prt = wv % WPG;  // row group, wave within it
  const int r = lane & 15, h = lane >> 4;
  const int row0 = blockIdx.x * R;  // first batch row of the block
  const int grow = grp * 16;        // first tile row of the group
  const bool head = prt == 0;       // the group's logits / softmax wave

  // ---- 1. stage: the group's 16 rows of a1 (rows >= B as zeros), four per
  // wave, and w2T.  Every load is issued before the first LDS store; the
  // softmax's label and the bias are fetched here too ----
  const int brow = row0 + grow + r;  // softmax: one lane per row
  const bool live = head && h == 0 && brow < B;
  const int lab = live ? (int)labels[brow] : 0;
  const float bias = (head && r < C) ? b2[r] : 0.f;
  {
    constexpr int AI = 16 / WPG;
    uint4 v[AI];
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      int gr = row0 + grow + prt + i * WPG;
      v[i] = uint4{0u, 0u, 0u, 0u};
      if (gr < B)
        v[i] = *reinterpret_cast<const uint4*>(a1 + (size_t)gr * K + lane * 8);
    }
    constexpr int WI = 16 * 64 / NT;  // w2T chunks per thread
    uint4 w[WI];
#pragma unroll
    for (int it = 0; it < WI; ++it) {
      int i = tid + it * NT;
      int rr = i >> 6, ch = i & 63;
      w[it] = uint4{0u, 0u, 0u, 0u};
      if (rr < C)
        w[it] = *reinterpret_cast<const uint4*>(w2T + (size_t)rr * K + ch * 8);
    }
#pragma unroll
    for (int i = 0; i < AI; ++i)
      *reinterpret_cast<uint4*>(&a_s[grow + prt + i * WPG][lane * 8]) = v[i];
#pragma unroll
    for (int it = 0; it < WI; ++it) {
      int i = tid + it * NT;
      int rr = i >> 6, ch = i & 63;
      *reinterpret_cast<uint4*>(&wT_s[rr][ch * 8]) = w[it];
    }
  }
  __syncthreads();

  if (!head) {
    // w2 rows padded to 16 classes ([K][16], the dX operand), from wT_s, by
    // the waves that have no logits to compute
    constexpr int BT = NG * (WPG - 1) * 64;  // threads building
    const int bt = (grp * (WPG - 1) + prt - 1) * 64 + lane;
#pragma unroll
    for (int n = bt; n < K; n += BT) {
      union { ushort_t u[16]; uint4 v[2]; } row;
#pragma unroll
      for (int c = 0; c < 16; ++c) row.u[c] = c < C ? wT_s[c][n] : (ushort_t)0;
      *reinterpret_cast<uint4*>(&wp_s[n][0]) = row.v[0];
      *reinterpret_cast<uint4*>(&wp_s[n][8]) = row.v[1];
    }
  } else {
    // ---- 2. logits = a1 @ w2 + b2, one accumulator walked in k order (the
    // chain gemm_tile's forward runs), rounded to bf16 ----
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const ushort_t* ap = &a_s[grow + r][8 * h];
    const ushort_t* bp = &wT_s[r][8 * h];
#pragma unroll
    for (int kk = 0; kk < K; kk += 32) {
      short8 a = *reinterpret_cast<const short8*>(ap + kk);
      short8 b = *reinterpret_cast<const short8*>(bp + kk);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      lg_s[grow + 4 * h + q][r] = r < C ? f2bf(acc[q] + bias) : (ushort_t)0;
    // the rows were written by this wave alone: order its LDS writes before
    // its reads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

    // ---- 3. softmax-xent, one lane per row (lanes 0..15), the arithmetic
    // of softmax_xent_t_kernel<10> ----
    float d[C];
    float loss = 0.f, correct = 0.f;
    {
      float v[C];
      float mx = -1e30f;
      int arg = 0;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        v[c] = bf2f(lg_s[grow + r][c]);
        if (v[c] > mx) { mx = v[c]; arg = c; }
      }
      float se = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        v[c] = __expf(v[c] - mx);
        se += v[c];
      }
      float inv_se = 1.f / se;
      float invB = 1.f / (float)B;
      float vlab = 0.f;
      union { ushort_t u[16]; uint4 q[2]; } rowo;
#pragma unroll
      for (int c = 0; c < 16; ++c) rowo.u[c] = 0;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        float pp = v[c] * inv_se;
        d[c] = live ? (pp - (c == lab ? 1.f : 0.f)) * invB : 0.f;
        rowo.u[c] = f2bf(d[c]);
        if (c == lab) vlab = v[c];
      }
      if (h == 0) {  // rows >= B and classes >= C are stored as zeros
        *reinterpret_cast<uint4*>(&dl_s[grow + r][0]) = rowo.q[0];
        *reinterpret_cast<uint4*>(&dl_s[grow + r][8]) = rowo.q[1];
      }
      if (live) {
        loss = -(__logf(vlab * inv_se)) * invB;
        correct = (arg == lab) ? 1.f : 0.f;
      }
    }
    // the group's 16 rows sit in lanes 0..15: one fixed rotate-add tree each,
    // so loss / accuracy are bitwise reproducible
    float ls = row_sum16(loss), cs = row_sum16(correct * inv_n);
    if (lane == 0) {
      lc_s[grp][0] = ls;
      lc_s[grp][1] = cs;
    }
    // db2: column sums of the fp32 d
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float dsum = row_sum16(d[c]);
      if (lane == 0) db2_s[grp][c] = dsum;
    }
  }
  __syncthreads();  // dl_s, lc_s, db2_s, wp_s complete

  // the last wave flushes db2 and runs the ticket (wave 0 has had the most
  // to do so far)
  if (wv == NW - 1 && lane < C) {
    float v = db2_s[0][lane];
    for (int g = 1; g < NG; ++g) v += db2_s[g][lane];
    if (v != 0.f) atomicAdd(&db2[lane], v);
  }
  if (wv == NW - 1 && lane == 0) {
    // the softmax kernel's last-block ticket on the same workspace: partials
    // parked per block, summed in block order by whichever block arrives
    // last; the counter resets itself.  Nothing waits.
    const unsigned nblk = gridDim.x;
    float r0 = 0.f, r1 = 0.f;
    for (int g = 0; g < NG; ++g) {
      r0 += lc_s[g][0];
      r1 += lc_s[g][1];
    }
    if (nblk == 1) {
      out[0] = r0;
      out[1] = r1;
    } else {
      __hip_atomic_store(&part[2 * blockIdx.x], r0, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&part[2 * blockIdx.x + 1], r1, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
      __threadfence();  // partials visible device-wide before the ticket
      if (atomicAdd(ticket, 1u) == nblk - 1) {
        __threadfence();
        float s0 = 0.f, s1 = 0.f;
        for (unsigned i = 0; i < nblk; ++i) {
          s0 += __hip_atomic_load(&part[2 * i], __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
          s1 += __hip_atomic_load(&part[2 * i + 1], __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
        }
        out[0] = s0;
        out[1] = s1;
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }

  // ---- 5. dW2 [K][C] += a1_tile^T @ dl: M = feature, N = class, reduction
  // over the R tile rows in steps of 32 (R = 16: rows 16..31 are zeros).  The
  // waves split the K / 16 feature tiles, each reducing over all R rows ----
  {
    constexpr int KS = R >= 32 ? R / 32 : 1;
    short8 bfr[KS];  // dl: B[row 8h + j][class r]
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int row = ks * 32 + 8 * h + j;
        bfr[ks][j] = row < R ? (short)dl_s[row < R ? row : 0][r] : (short)0;
      }
#pragma unroll
    for (int i = 0; i < (K >> 4) / NW; ++i) {
      const int t = wv + i * NW;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        short8 afr;  // a1^T: A[feature 16t + r][row 8h + j]
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          int row = ks * 32 + 8 * h + j;
          afr[j] = row < R ? (short)a_s[row < R ? row : 0][t * 16 + r]
                           : (short)0;
        }
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr, bfr[ks], acc, 0, 0, 0);
      }
      if (r < C) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          atomicAdd(&dw2[(size_t)(t * 16 + 4 * h + q) * C + r], acc[q]);
      }
    }
  }
  __syncthreads();  // every wave is done reading a_s

  // ---- 4. dyeff1^T = mask(w2 @ dl^T) for the group's 16 rows, a quarter of
  // the features per wave: M = feature, N = row, so a lane holds four
  // consecutive features of one row — one 8 B LDS read of the a1 signs and
  // one 8 B write of dyeff1 over them in place (each element by the lane
  // that read it).  db1 += column sums of the masked fp32 values: a 16-lane
  // rotate-add per feature, no atomics inside the block ----
  {
    short8 bfr = {0, 0, 0, 0, 0, 0, 0, 0};  // dl^T: B[class 8h + j][row r]
    if (h < 2) bfr = *reinterpret_cast<const short8*>(&dl_s[grow + r][8 * h]);
    constexpr int TW = (K >> 4) / WPG;  // feature tiles per wave
#pragma unroll
    for (int i = 0; i < TW; ++i) {
      const int t = prt * TW + i;
      short8 afr = {0, 0, 0, 0, 0, 0, 0, 0};  // w2: A[feature 16t + r][class]
      if (h < 2) afr = *reinterpret_cast<const short8*>(&wp_s[t * 16 + r][8 * h]);
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr, bfr, acc, 0, 0, 0);
      const int n = t * 16 + 4 * h;
      union { ushort_t u[4]; uint2 v; } e;
      e.v = *reinterpret_cast<const uint2*>(&a_s[grow + r][n]);
      float s[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float v = (bf2f(e.u[q]) > 0.f) ? acc[q] * inv_keep : 0.f;
        e.u[q] = f2bf(v);
        s[q] = row_sum16(v);
      }
      *reinterpret_cast<uint2*>(&a_s[grow + r][n]) = e.v;
      if (r == 0)
        *reinterpret_cast<float4*>(&db1_s[grp][n]) =
            float4{s[0], s[1], s[2], s[3]};
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 16 / WPG; ++i) {
    int rr = prt + i * WPG;
    int gr = row0 + grow + rr;
    if (gr < B)
      *reinterpret_cast<uint4*>(dyeff + (size_t)gr * K + lane * 8) =
          *reinterpret_cast<const uint4*>(&a_s[grow + rr][lane * 8]);
  }
#pragma unroll
  for (int n = tid; n < K; n += NT) {
    float s = db1_s[0][n];
#pragma unroll
    for (int g = 1; g < NG; ++g) s += db1_s[g][n];
    atomicAdd(&db1[n], s);
  }
}

int fc2_head_blocks(int B, int R) { return (B + R - 1) / R; }

void launch_fc2_head(int R, const unsigned short* a1,
                     const unsigned short* w2T, const float* b2,
                     const long* labels, unsigned short* dyeff, float* dw2,
                     float* db2, float* db1, float* out, int B,
                     float inv_keep, float inv_n, float* part,
                     unsigned* ticket, hipStream_t s) {
  dim3 grid(fc2_head_blocks(B, R));
#define FC2H_LAUNCH(RR)                                                      \
  hipLaunchKernelGGL((fc2_head_kernel<RR>), grid, dim3(RR * 4 * FC2H_WPG),   \
                     0, s, a1, w2T, b2, labels, dyeff, dw2, db2, db1, out,   \
                     B, inv_keep, inv_n, part, ticket)
  if (R == 16) FC2H_LAUNCH(16);
  else if (R == 32) FC2H_LAUNCH(32);
  else FC2H_LAUNCH(64);
#undef FC2H_LAUNCH
}
