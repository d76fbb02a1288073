// PowerSGD rank-R gradient compression with error feedback (--grad_lowrank,
// docs/KERNELS.md "Low-rank compression") on the flat fp32 bucket.  A
// compressed tensor is a row-major [rows][cols] matrix G at a 16 B aligned
// bucket offset, rows and cols multiples of 16, with a residual E of the same
// shape and a factor Q [cols][R]:
//   lowrank_p_kernel       M = G + E (stored over E), P = M Q          [rows][R]
//   (sum of P over ranks)
//   lowrank_orth_kernel    P^ = modified Gram-Schmidt of P, in place
//   lowrank_q_kernel       Q_r = M^T P^                                [cols][R]
//   (sum of Q_r over ranks -> Q_S)
//   lowrank_expand_kernel  bucket = P^ Q_S^T,  E = M - P^ Q_r^T
// All operands are fp32 and every product runs on v_mfma_f32_16x16x4_f32 with
// R padded to the 16-wide N tile by zero columns.  A lane feeds the MFMA
//   A[m = l & 15][k = l >> 4], B[k = l >> 4][n = l & 15]
// and holds D[m = (l >> 4)*4 + r][n = l & 15], r = 0..3.  Where a lane loads
// four consecutive floats of M with one 16 B read, the four values go to four
// MFMAs; the K (or M) index each MFMA covers is then a fixed permutation,
// applied to both operands (or to the store address).
//
// No float atomics: partial tiles meet in LDS in wave order and in fp32 planes
// in plane order, so every sum's order is a function of the launch geometry.
// Contraction is off: each fp32 operation outside the MFMAs rounds once.
#pragma clang fp contract(off)

#include "grad_norm_common.h"

#define LR_THREADS 256
#define LR_WAVES (LR_THREADS / 64)

DEV f32x4 lr_mfma(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

DEV float lr_ld(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

DEV void lr_st(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the tensor whose block range [blk[t], blk[t + 1]) holds b; d.n when b lies
// behind the last one (the blocks that move the dense tensors)
DEV int lr_tensor_of(const int* blk, int n, int b) {
  int t = 0;
  while (t < n && b >= blk[t + 1]) ++t;
  return t;
}

// dense tensors <-> the wire behind P, one element per thread and stride; the
// gaps have no alignment, so plain 4 B copies (a few thousand elements)
template <bool PACK>
DEV void lr_dense_copy(float* grad, float* wire, const LowrankDesc& d, int blk,
                       int nblk) {
  for (int s = 0; s < d.nd; ++s) {
    float* const g = grad + d.doff[s];
    float* const w = wire + d.dwire[s];
    for (long i = (long)blk * LR_THREADS + threadIdx.x; i < d.dlen[s];
         i += (long)nblk * LR_THREADS) {
      if (PACK) w[i] = g[i];
      else g[i] = w[i];
    }
  }
}

// ---------------------------------------------------------------------------
// P = (G + E) Q.  One workgroup per 16-row tile; Q [cols][16] zero-padded in
// LDS (32 KB at cols = 512); the 16-column chunks of K dealt round-robin to
// the four waves, each lane one 16 B read of G and of E per chunk, M stored
// over E in the same pass; the waves' 16 x 16 partial tiles summed in LDS in
// wave order.  Blocks behind the last tile pack the dense tensors.
// ---------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(LR_THREADS)
void lowrank_p_kernel(float* grad, float* resid, const float* q, float* wire,
                      LowrankDesc d) {
  __shared__ float Qs[LOWRANK_MAX_COLS * 16];
  __shared__ float part[LR_WAVES][256];
  const int t = lr_tensor_of(d.pblk, d.n, blockIdx.x);
  if (t == d.n) {
    lr_dense_copy<true>(grad, wire, d, blockIdx.x - d.pblk[d.n],
                        gridDim.x - d.pblk[d.n]);
    return;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cols = d.cols[t], R = d.R;
  const int m0 = (blockIdx.x - d.pblk[t]) * 16;
  const float* const qt = q + d.qoff[t];
  for (int i = tid; i < cols * 16; i += LR_THREADS)
    Qs[i] = (i & 15) < R ? qt[(i >> 4) * R + (i & 15)] : 0.f;
  __syncthreads();

  const long row0 = d.off[t] + (long)(m0 + (lane & 15)) * cols;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int c = wave; c < (cols >> 4); c += LR_WAVES) {
    const int k = c * 16 + (lane >> 4) * 4;
    const float4 g = *reinterpret_cast<const float4*>(grad + row0 + k);
    const float4 e = *reinterpret_cast<const float4*>(resid + row0 + k);
    const float4 m = float4{g.x + e.x, g.y + e.y, g.z + e.z, g.w + e.w};
    *reinterpret_cast<float4*>(resid + row0 + k) = m;
    const float* const b = Qs + k * 16 + (lane & 15);
    acc = lr_mfma(m.x, b[0], acc);
    acc = lr_mfma(m.y, b[16], acc);
    acc = lr_mfma(m.z, b[32], acc);
    acc = lr_mfma(m.w, b[48], acc);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
    part[wave][((lane >> 4) * 4 + r) * 16 + (lane & 15)] = acc[r];
  __syncthreads();
  float v = part[0][tid];
#pragma unroll
  for (int w = 1; w < LR_WAVES; ++w) v += part[w][tid];
  if ((tid & 15) < R)
    wire[d.poff[t] + (long)(m0 + (tid >> 4)) * R + (tid & 15)] = v;
}

// ---------------------------------------------------------------------------
// Modified Gram-Schmidt of P [rows][R] in column order, each column divided by
// (|column| + 1e-8); the divided column q is a little short of unit length, so
// the later columns lose (q.rest / q.q) q.  One workgroup of 1024 threads per
// tensor; thread i keeps rows i, i + 1024, i + 2048, i + 3072 (rows <= 4096)
// x 16 columns in registers.  Column i costs three reductions: a second pass
// against the finished columns, its squared norm, then q.q and the dot
// products with all later columns at once.  A
// reduction is the thread's rows in row order, the fixed shuffle tree, and the
// 16 waves' values from LDS in wave order (every thread forms the same sum).
// ---------------------------------------------------------------------------
#define LR_ORTH_THREADS 1024
#define LR_ORTH_WAVES (LR_ORTH_THREADS / 64)

extern "C" __global__ __launch_bounds__(LR_ORTH_THREADS)
void lowrank_orth_kernel(float* wire, LowrankDesc d) {
  __shared__ float red[16][LR_ORTH_WAVES];
  const int t = blockIdx.x;
  const int rows = d.rows[t], R = d.R;
  float* const P = wire + d.poff[t];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float p[4][16];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int row = tid + s * LR_ORTH_THREADS;
#pragma unroll
    for (int c = 0; c < 16; ++c)
      p[s][c] = (row < rows && c < R) ? P[(long)row * R + c] : 0.f;
  }
  float qqv[16];  // q.q of the finished columns (the same in every thread)
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if (i >= R) continue;  // block-uniform
    if (i > 0) {
      // second pass against the finished columns, all at once: what rounding
      // left of them in column i goes, so that a dependent column (nothing
      // but rounding noise) still ends up orthogonal to them
#pragma unroll
      for (int k = 0; k < i; ++k) {
        float dk = 0.f;
#pragma unroll
        for (int s = 0; s < 4; ++s) dk += p[s][k] * p[s][i];
        dk = gn_wave_sum(dk);
        if (lane == 0) red[k][wave] = dk;
      }
      __syncthreads();
      float coef[15];
#pragma unroll
      for (int k = 0; k < i; ++k) {
        float dot = red[k][0];
#pragma unroll
        for (int w = 1; w < LR_ORTH_WAVES; ++w) dot += red[k][w];
        coef[k] = qqv[k] > 0.f ? dot / qqv[k] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < i; ++k)
#pragma unroll
        for (int s = 0; s < 4; ++s) p[s][i] = p[s][i] - coef[k] * p[s][k];
      __syncthreads();  // the dots are read before the norm reuses red
    }
    float s2 = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) s2 += p[s][i] * p[s][i];
    s2 = gn_wave_sum(s2);
    if (lane == 0) red[i][wave] = s2;
    __syncthreads();
    float tot = red[i][0];
#pragma unroll
    for (int w = 1; w < LR_ORTH_WAVES; ++w) tot += red[i][w];
    const float den = sqrtf(tot) + 1e-8f;
#pragma unroll
    for (int s = 0; s < 4; ++s) p[s][i] = p[s][i] / den;
    __syncthreads();  // red[i] is read before the dots reuse the rows below
    // q.q of the divided column (slot i) rides with the dots (slots j > i)
#pragma unroll
    for (int j = i; j < 16; ++j) {
      if (j >= R) continue;
      float dj = 0.f;
#pragma unroll
      for (int s = 0; s < 4; ++s) dj += p[s][i] * p[s][j];
      dj = gn_wave_sum(dj);
      if (lane == 0) red[j][wave] = dj;
    }
    __syncthreads();
    float qq = red[i][0];
#pragma unroll
    for (int w = 1; w < LR_ORTH_WAVES; ++w) qq += red[i][w];
    qqv[i] = qq;
#pragma unroll
    for (int j = i + 1; j < 16; ++j) {
      if (j >= R) continue;
      float dot = red[j][0];
#pragma unroll
      for (int w = 1; w < LR_ORTH_WAVES; ++w) dot += red[j][w];
      const float coef = qq > 0.f ? dot / qq : 0.f;
#pragma unroll
      for (int s = 0; s < 4; ++s) p[s][j] = p[s][j] - coef * p[s][i];
    }
    __syncthreads();  // the dots are read before the next column's writes
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int row = tid + s * LR_ORTH_THREADS;
#pragma unroll
    for (int c = 0; c < 16; ++c)
      if (row < rows && c < R) P[(long)row * R + c] = p[s][c];
  }
}

// ---------------------------------------------------------------------------
// Q_r = M^T P^.  A block owns 64 columns of M and a slice of LOWRANK_Q_SLICE
// rows (the K extent); its waves take the slice's 4-row steps round-robin.
// Lanes 0..15 of a step read 256 contiguous bytes of one row of M (16 B each);
// the j-th value of a lane is column c0 + 4*(l & 15) + j, so MFMA j produces
// the output rows c0 + 4*m + j.  The waves' tiles meet in LDS in wave order,
// the block stores its plane, and the last block of a column group to arrive
// (integer ticket, self-resetting) adds the planes in plane order.
// ---------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(LR_THREADS)
void lowrank_q_kernel(const float* resid, const float* wire, float* qr,
                      float* planes, unsigned* tickets, LowrankDesc d) {
  __shared__ float part[LR_WAVES][1024];
  __shared__ int is_last;
  const int t = lr_tensor_of(d.qblk, d.n, blockIdx.x);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rows = d.rows[t], cols = d.cols[t], R = d.R;
  const int ng = (cols + 63) >> 6;
  const int S = (rows + LOWRANK_Q_SLICE - 1) / LOWRANK_Q_SLICE;
  const int b = blockIdx.x - d.qblk[t];
  const int cg = b % ng, z = b / ng;
  const float* const M = resid + d.off[t];
  const float* const P = wire + d.poff[t];
  const int col = cg * 64 + (lane & 15) * 4;
  const int n = lane & 15;
  const int kend = min(rows, (z + 1) * LOWRANK_Q_SLICE);

  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kb = z * LOWRANK_Q_SLICE + wave * 4; kb < kend;
       kb += LR_WAVES * 4) {
    const int row = kb + (lane >> 4);  // < kend: slices end at multiples of 16
    float4 a = float4{0.f, 0.f, 0.f, 0.f};
    if (col < cols)
      a = *reinterpret_cast<const float4*>(M + (long)row * cols + col);
    const float pv = n < R ? P[(long)row * R + n] : 0.f;
    acc[0] = lr_mfma(a.x, pv, acc[0]);
    acc[1] = lr_mfma(a.y, pv, acc[1]);
    acc[2] = lr_mfma(a.z, pv, acc[2]);
    acc[3] = lr_mfma(a.w, pv, acc[3]);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      part[wave][(4 * ((lane >> 4) * 4 + r) + j) * 16 + n] = acc[j][r];
  __syncthreads();
  float* const plane = planes + (long)t * LOWRANK_PLANE_FLOATS;
  float* const mine = plane + (long)(z * ng + cg) * 1024;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int e = tid + s * LR_THREADS;
    float v = part[0][e];
#pragma unroll
    for (int w = 1; w < LR_WAVES; ++w) v += part[w][e];
    lr_st(mine + e, v);
  }
  __threadfence();  // this thread's stores visible before the ticket
  __syncthreads();
  if (tid == 0) {
    unsigned* const ticket = tickets + t * LOWRANK_MAX_GROUPS + cg;
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int last = atomicAdd(ticket, 1u) == (unsigned)(S - 1);
    if (last) {
      __threadfence();
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
    is_last = last;
  }
  __syncthreads();
  if (!is_last) return;
  float* const out = qr + d.qoff[t];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int e = tid + s * LR_THREADS;
    float v = lr_ld(plane + (long)cg * 1024 + e);
    for (int zz = 1; zz < S; ++zz)
      v += lr_ld(plane + (long)(zz * ng + cg) * 1024 + e);
    const int c = cg * 64 + (e >> 4);
    if (c < cols && (e & 15) < R) out[(long)c * R + (e & 15)] = v;
  }
}

// ---------------------------------------------------------------------------
// bucket = P^ Q_S^T and E = M - P^ Q_r^T.  A wave owns a 16-row x 64-column
// strip: four transposed tiles D' = Q P^T (K = 16: four MFMAs each), so a lane
// holds four consecutive columns of one row and moves M, the bucket and E with
// 16 B accesses.  `same` (one rank): Q_S is Q_r, one product serves both
// outputs.  Blocks behind the last strip unpack the reduced dense tensors.
// ---------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(LR_THREADS)
void lowrank_expand_kernel(float* grad, float* resid, float* wire,
                           const float* qr, const float* qsum, int same,
                           LowrankDesc d) {
  const int t = lr_tensor_of(d.xblk, d.n, blockIdx.x);
  if (t == d.n) {
    lr_dense_copy<false>(grad, wire, d, blockIdx.x - d.xblk[d.n],
                         gridDim.x - d.xblk[d.n]);
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rows = d.rows[t], cols = d.cols[t], R = d.R;
  const int ng = (cols + 63) >> 6;
  const int task = (blockIdx.x - d.xblk[t]) * LR_WAVES + wave;
  if (task >= (rows >> 4) * ng) return;  // wave-uniform, no barrier below
  const int r0 = (task / ng) * 16, c0 = (task % ng) * 64;
  const int kq = lane >> 4, n = lane & 15;
  const float* const P = wire + d.poff[t] + (long)(r0 + n) * R;
  float bp[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) bp[j] = kq + 4 * j < R ? P[kq + 4 * j] : 0.f;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int cb = c0 + ct * 16;
    if (cb >= cols) break;
    const long qrow = d.qoff[t] + (long)(cb + n) * R;
    f32x4 as = f32x4{0.f, 0.f, 0.f, 0.f}, ar = as;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (4 * j >= R) continue;
      const int k = kq + 4 * j;
      as = lr_mfma(k < R ? qsum[qrow + k] : 0.f, bp[j], as);
      if (!same) ar = lr_mfma(k < R ? qr[qrow + k] : 0.f, bp[j], ar);
    }
    if (same) ar = as;
    const long at = d.off[t] + (long)(r0 + n) * cols + cb + kq * 4;
    const float4 m = *reinterpret_cast<const float4*>(resid + at);
    *reinterpret_cast<float4*>(grad + at) = float4{as[0], as[1], as[2], as[3]};
    *reinterpret_cast<float4*>(resid + at) =
        float4{m.x - ar[0], m.y - ar[1], m.z - ar[2], m.w - ar[3]};
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static int lr_dense_blocks(const LowrankDesc& d) {
  long total = 0;
  for (int s = 0; s < d.nd; ++s) total += d.dlen[s];
  const long b = (total + 4 * LR_THREADS - 1) / (4 * LR_THREADS);
  return (int)(b > 64 ? 64 : b);
}

bool lowrank_fits(long off, long rows, long cols) {
  return off % 4 == 0 && rows % 16 == 0 && cols % 16 == 0 && rows >= 64 &&
         rows <= LOWRANK_MAX_ROWS && cols >= 64 && cols <= LOWRANK_MAX_COLS;
}

void lowrank_blocks(LowrankDesc* d) {
  d->pblk[0] = d->qblk[0] = d->xblk[0] = 0;
  for (int t = 0; t < d->n; ++t) {
    const int ng = (d->cols[t] + 63) / 64;
    const int S = (d->rows[t] + LOWRANK_Q_SLICE - 1) / LOWRANK_Q_SLICE;
    d->pblk[t + 1] = d->pblk[t] + d->rows[t] / 16;
    d->qblk[t + 1] = d->qblk[t] + ng * S;
    d->xblk[t + 1] = d->xblk[t] +
                     (d->rows[t] / 16 * ng + LR_WAVES - 1) / LR_WAVES;
  }
}

void launch_lowrank_p(float* grad, float* resid, const float* q, float* wire,
                      const LowrankDesc& d, hipStream_t s) {
  hipLaunchKernelGGL(lowrank_p_kernel, dim3(d.pblk[d.n] + lr_dense_blocks(d)),
                     dim3(LR_THREADS), 0, s, grad, resid, q, wire, d);
}

void launch_lowrank_orth(float* wire, const LowrankDesc& d, hipStream_t s) {
  hipLaunchKernelGGL(lowrank_orth_kernel, dim3(d.n), dim3(LR_ORTH_THREADS), 0,
                     s, wire, d);
}

void launch_lowrank_q(const float* resid, const float* wire, float* qr,
                      float* ws, const LowrankDesc& d, hipStream_t s) {
  unsigned* tickets = reinterpret_cast<unsigned*>(
      ws + (long)LOWRANK_MAX_TENSORS * LOWRANK_PLANE_FLOATS);
  hipLaunchKernelGGL(lowrank_q_kernel, dim3(d.qblk[d.n]), dim3(LR_THREADS), 0,
                     s, resid, wire, qr, ws, tickets, d);
}

void launch_lowrank_expand(float* grad, float* resid, float* wire,
                           const float* qr, const float* qsum,
                           const LowrankDesc& d, hipStream_t s) {
  hipLaunchKernelGGL(lowrank_expand_kernel,
                     dim3(d.xblk[d.n] + lr_dense_blocks(d)), dim3(LR_THREADS),
                     0, s, grad, resid, wire, qr, qsum, qr == qsum ? 1 : 0, d);
}
