// Muon (--optimizer muon) on the flat fp32 bucket (docs/KERNELS.md "Muon"):
// Nesterov momentum whose per-matrix update is replaced by its nearest
// semi-orthogonal matrix, five Newton-Schulz iterations on the matrix cores.
// With g the aggregated bucket, s = grad_scale, coef the clip coefficient:
//   gh = ((g * s) * coef), then the --drop_connect_post mask
//   v = mu*v + gh                     u = gh + mu*v
// Weight tensors (bit t of `adapt`), viewed as [rows][cols]:
//   X = bf16(u), s_t = 1 / (|u|_F + 1e-7); per iteration
//   G = bf16(sc^2 * X^T X), P = bf16(b*G + c * G G), X = bf16(sc * (a*X + X P))
//   with sc = s_t in the first iteration and 1 after it, fp32 accumulation;
//   w = w*(1 - lr*wd) - (lr * 0.2*sqrt(max(rows, cols))) * X
// Biases: w -= lr*v.  lr = lr_scale * contrib as in adam.hip.  Then the moving
// average, the bf16 shadow and the re-zeroed bucket of the other optimizers.
//
// muon_momentum_kernel: one streaming pass with grad_norm_kernel's geometry;
//   v in place, bf16(u) into the per-tensor workspace matrix, sum u^2 per
//   tensor (fixed chunks, shuffle tree, last block's ordered sum, no float
//   atomics) -> tab[t] = s_t.
// muon_ns_lds_kernel: cols <= 64; one workgroup per tensor, X, G and P
//   resident in LDS for all iterations.
// muon_gram_kernel / muon_gram_sum_kernel / muon_poly_kernel /
//   muon_apply_kernel: the tiled route (cols % 64 == 0, rows % 8 == 0).
// muon_update_kernel: the final streaming pass.
//
// Every summation order is a function of the launch geometry only, so ranks
// that hold the same bucket get the same bits.  Contraction is off for the
// whole file: each fp32 operation rounds once, in the order written, and the
// elementwise parts agree bit for bit with ops/cpu_ref.py::muon_step.
#pragma clang fp contract(off)

#include "grad_norm_common.h"

#define MU_A 3.4445f
#define MU_B (-4.7750f)
#define MU_C 2.0315f

struct MuonHyper {
  float mu, wd;
  float s, contrib;  // grad_scale and its exact inverse
  unsigned adapt;    // bit t: tensor t is a weight tensor
};

// where the momentum pass writes bf16(u) of tensor t: element offset into the
// workspace, < 0 for a bias
struct MuonUoff {
  long off[GRAD_NORM_MAX_SEGS];
};

// what the update pass reads per tensor: the orthogonalised matrix (nullptr
// for a bias) and 0.2*sqrt(max(rows, cols))
struct MuonOut {
  const ushort_t* x[GRAD_NORM_MAX_SEGS];
  float scale[GRAD_NORM_MAX_SEGS];
};

DEV float muon_keep(uint32_t r, float dc_keep) {
  return (r * (1.0f / 4294967296.0f) < dc_keep) ? 1.f : 0.f;
}

// one element of the momentum update: v in place, returns u
DEV float muon_u(float g, float keep, float& v, float coef,
                 const MuonHyper& h) {
  const float gh = ((g * h.s) * coef) * keep;
  v = h.mu * v + gh;
  return gh + h.mu * v;
}

// the last segment that starts at or before idx (the segments tile [0, n))
DEV int muon_seg_of(const GradNormSegs& segs, long idx) {
  int t = 0;
#pragma unroll
  for (int s = 1; s < GRAD_NORM_MAX_SEGS; ++s)
    t += (s < segs.n && idx >= segs.off[s]) ? 1 : 0;
  return t;
}

// ---------------------------------------------------------------------------
// pass 1: v in place, bf16(u) of the weight tensors, s_t per tensor
// ---------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(GN_THREADS)
void muon_momentum_kernel(const float* grad, float* mom, ushort_t* ws, long n,
                          GradNormSegs segs, MuonUoff uo, long chunk,
                          MuonHyper h, uint64_t offset, const long* offset_dev,
                          float dc_keep, uint64_t seed,
                          const float* clip_coef_dev, float* tab, float* part,
                          unsigned* ticket) {
  __shared__ float wred[GRAD_NORM_MAX_SEGS][GN_WAVES];
  __shared__ int is_last;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const long c0 = (long)blockIdx.x * chunk;
  const long cend = min(n, c0 + chunk);
  if (offset_dev) offset = (uint64_t)*offset_dev;
  const float coef = clip_coef_dev ? *clip_coef_dev : 1.f;

  // ---- 1. this block's chunk, one segment at a time (block-uniform loop) --
  for (int s = 0; s < segs.n; ++s) {
    const long a = max(c0, segs.off[s]);
    const long b = min(cend, segs.off[s] + segs.len[s]);
    if (a >= b) continue;
    const bool wt = ((h.adapt >> s) & 1u) != 0;
    // element e of the bucket is element e - off[s] of the tensor's matrix
    ushort_t* const ub = wt ? ws + (uo.off[s] - segs.off[s]) : nullptr;
    float acc = 0.f;
    // [a, a4): scalar head, [a4, b4): 16 B groups, [b4, b): scalar tail
    const long a4 = min(b, (a + 3) & ~3L);
    const long b4 = max(a4, b & ~3L);
    const long g1 = b4 >> 2;
    for (long g = (a4 >> 2) + tid; g < g1; g += 4 * GN_THREADS) {
      float4 gg[4], vv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long gj = g + j * GN_THREADS;
        if (gj < g1) {
          gg[j] = *reinterpret_cast<const float4*>(grad + gj * 4);
          vv[j] = *reinterpret_cast<const float4*>(mom + gj * 4);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long gj = g + j * GN_THREADS;
        if (gj >= g1) break;
        float kp[4] = {1.f, 1.f, 1.f, 1.f};
        if (dc_keep > 0.f) {
          Philox4 ph = philox4x32(seed, offset, (uint64_t)gj);
          kp[0] = muon_keep(ph.x, dc_keep); kp[1] = muon_keep(ph.y, dc_keep);
          kp[2] = muon_keep(ph.z, dc_keep); kp[3] = muon_keep(ph.w, dc_keep);
        }
        float4 u;
        u.x = muon_u(gg[j].x, kp[0], vv[j].x, coef, h);
        u.y = muon_u(gg[j].y, kp[1], vv[j].y, coef, h);
        u.z = muon_u(gg[j].z, kp[2], vv[j].z, coef, h);
        u.w = muon_u(gg[j].w, kp[3], vv[j].w, coef, h);
        *reinterpret_cast<float4*>(mom + gj * 4) = vv[j];
        if (wt) {
          ushort_t* o = ub + gj * 4;
          o[0] = f2bf(u.x); o[1] = f2bf(u.y);
          o[2] = f2bf(u.z); o[3] = f2bf(u.w);
          acc += gn_sq4(u);
        }
      }
    }
    // head and tail: at most three elements each, one per thread
#pragma unroll
    for (int part_i = 0; part_i < 2; ++part_i) {
      const long e = (part_i == 0 ? a : b4) + tid;
      if (e < (part_i == 0 ? a4 : b)) {
        float kp = 1.f;
        if (dc_keep > 0.f) {
          Philox4 ph = philox4x32(seed, offset, (uint64_t)(e >> 2));
          const int c = (int)(e & 3);
          kp = muon_keep(c == 0 ? ph.x : c == 1 ? ph.y : c == 2 ? ph.z : ph.w,
                         dc_keep);
        }
        float ve = mom[e];
        const float u = muon_u(grad[e], kp, ve, coef, h);
        mom[e] = ve;
        if (wt) {
          ub[e] = f2bf(u);
          acc += u * u;
        }
      }
    }
    acc = gn_wave_sum(acc);
    if (lane == 0) wred[s][wave] = acc;
  }
  __syncthreads();
  if (tid == 0) {
    for (int s = 0; s < segs.n; ++s) {
      const long a = max(c0, segs.off[s]);
      const long b = min(cend, segs.off[s] + segs.len[s]);
      if (a >= b) continue;
      float r = wred[s][0];
      for (int w = 1; w < GN_WAVES; ++w) r += wred[s][w];
      __hip_atomic_store(&part[(long)s * GRAD_NORM_MAX_BLOCKS + blockIdx.x], r,
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __threadfence();  // partials visible device-wide before the ticket
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    if (last) __threadfence();
    is_last = last;
  }
  __syncthreads();
  if (!is_last) return;

  // ---- 2. last block: per segment, the partials in block order ------------
  for (int s = 0; s < segs.n; ++s) {
    const float acc = gn_wave_sum(
        gn_partials(part, segs.off[s], segs.len[s], s, chunk, tid));
    if (lane == 0) wred[s][wave] = acc;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int s = 0; s < segs.n; ++s) {
    float r = wred[s][0];
    for (int w = 1; w < GN_WAVES; ++w) r += wred[s][w];
    tab[s] = ((h.adapt >> s) & 1u) ? 1.f / (sqrtf(r) + 1e-7f) : 0.f;
  }
  __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------
// MFMA fragment helpers (v_mfma_f32_16x16x32_bf16).  Lane l holds
//   A[m = l & 15][k = (l >> 4)*8 .. +7], B[k = (l >> 4)*8 .. +7][n = l & 15],
//   D[m = (l >> 4)*4 + r][n = l & 15].
// A fragment of a k-major LDS image (row = k) comes from two transpose reads
// four rows apart (common.h); of an m-major image it is one 16 B read.
// ---------------------------------------------------------------------------
DEV unsigned muon_lds_addr(const void* p) { return (unsigned)(uintptr_t)p; }

// rows k0 + (l >> 4)*8 .. +7 of the image, columns c0 .. c0 + 15; ld in
// elements (ld*2 and c0*2 multiples of 8 bytes)
DEV short8 muon_frag_kmajor(const ushort_t* img, int ld, int k0, int c0,
                            int lane) {
  const int krow = k0 + (lane >> 4) * 8 + ((lane & 15) >> 2);
  const unsigned a0 = muon_lds_addr(img + krow * ld + c0 + (lane & 3) * 4);
  const uint2 lo = tr16_issue(a0);
  const uint2 hi = tr16_issue(a0 + (unsigned)(8 * ld));  // 4 rows down
  return pack_wait(lo, hi);
}

// rows m0 .. m0 + 15 of the image, columns k0 + (l >> 4)*8 .. +7 (16 B
// aligned)
DEV short8 muon_frag_mmajor(const ushort_t* img, int ld, int m0, int k0,
                            int lane) {
  return *reinterpret_cast<const short8*>(
      img + (m0 + (lane & 15)) * ld + k0 + (lane >> 4) * 8);
}

DEV f32x4 muon_mfma(short8 a, short8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// ---------------------------------------------------------------------------
// the LDS route: one workgroup per tensor, all iterations in LDS
// ---------------------------------------------------------------------------
#define MUON_LDS_THREADS 512
#define MUON_LDS_WAVES (MUON_LDS_THREADS / 64)
#define MUON_LDS_BYTES 163840  // 160 KB

struct MuonLdsArgs {
  const ushort_t* src[GRAD_NORM_MAX_SEGS];
  ushort_t* dst[GRAD_NORM_MAX_SEGS];
  int rows[GRAD_NORM_MAX_SEGS], cols[GRAD_NORM_MAX_SEGS];
  int tab[GRAD_NORM_MAX_SEGS];  // index of s_t in the device table
};

// Padded geometry.  CP: columns in 16-wide tiles; CK: the same as an MFMA K
// extent (32-deep); RP: rows as a K extent; LD: row stride of every bf16 image
// (8 elements of padding against bank conflicts, rows stay 16 B aligned).
static __host__ __device__ inline int muon_cp(int cols) { return (cols + 15) & ~15; }
static __host__ __device__ inline int muon_ck(int cols) { return (cols + 31) & ~31; }
static __host__ __device__ inline int muon_rp(int rows) { return (rows + 31) & ~31; }

static long muon_lds_bytes(int rows, int cols) {
  const long CP = muon_cp(cols), CK = muon_ck(cols), RP = muon_rp(rows);
  const long LD = CK + 8;
  return (RP * LD + 2 * CK * LD) * 2 + CP * CP * 4;
}

extern __shared__ __align__(16) ushort_t muon_lds[];

extern "C" __global__ __launch_bounds__(MUON_LDS_THREADS)
void muon_ns_lds_kernel(MuonLdsArgs a, const float* tab, int iters) {
  const int t = blockIdx.x;
  const int rows = a.rows[t], cols = a.cols[t];
  const ushort_t* const src = a.src[t];
  ushort_t* const dst = a.dst[t];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int CP = muon_cp(cols), CK = muon_ck(cols), RP = muon_rp(rows);
  const int LD = CK + 8, NT = CP >> 4, NK = CK >> 5, LC = LD >> 3;
  const int frow = (lane >> 4) * 4, fcol = lane & 15;
  ushort_t* const X = muon_lds;           // [RP][LD]
  ushort_t* const Gb = X + RP * LD;       // [CK][LD]
  ushort_t* const Pb = Gb + CK * LD;      // [CK][LD]
  float* const Gs = reinterpret_cast<float*>(Pb + CK * LD);  // [CP][CP]

  // ---- load: zero G and P (their padding stays zero), X with zero padding --
  for (int i = tid; i < 2 * CK * LC; i += MUON_LDS_THREADS)
    reinterpret_cast<uint4*>(Gb)[i] = uint4{0u, 0u, 0u, 0u};
  const bool vec = (cols & 7) == 0;
  for (int c = tid; c < RP * LC; c += MUON_LDS_THREADS) {
    const int r = c / LC, c8 = (c % LC) * 8;
    union { uint4 v; ushort_t e[8]; } x;
    x.v = uint4{0u, 0u, 0u, 0u};
    if (r < rows && c8 < cols) {
      if (vec) {
        x.v = *reinterpret_cast<const uint4*>(src + (long)r * cols + c8);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (c8 + j < cols) x.e[j] = src[(long)r * cols + c8 + j];
      }
    }
    *reinterpret_cast<uint4*>(X + r * LD + c8) = x.v;
  }
  __syncthreads();
  const float s_t = tab[a.tab[t]];

  for (int it = 0; it < iters; ++it) {
    const float sc = it == 0 ? s_t : 1.f;
    // ---- G = X^T X: each wave its 32-row blocks, upper tiles only ----------
    f32x4 acc[4][4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kb = wave; kb < (RP >> 5); kb += MUON_LDS_WAVES) {
      short8 f[4];
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) {
        f[ti] = short8{0, 0, 0, 0, 0, 0, 0, 0};
        if (ti < NT) f[ti] = muon_frag_kmajor(X, LD, kb * 32, ti * 16, lane);
      }
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = mi; ni < 4; ++ni)
          if (ni < NT) acc[mi][ni] = muon_mfma(f[mi], f[ni], acc[mi][ni]);
    }
    // the waves' accumulators through LDS in wave order, mirrored
    for (int w = 0; w < MUON_LDS_WAVES; ++w) {
      if (wave == w) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int ni = mi; ni < 4; ++ni) {
            if (ni >= NT) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int m = mi * 16 + frow + r, n = ni * 16 + fcol;
              float v = acc[mi][ni][r];
              if (w) v = Gs[m * CP + n] + v;
              Gs[m * CP + n] = v;
              if (mi != ni) Gs[n * CP + m] = v;
            }
          }
      }
      __syncthreads();
    }
    const float sc2 = sc * sc;
    for (int i = tid; i < CP * CP; i += MUON_LDS_THREADS)
      Gb[(i / CP) * LD + (i % CP)] = f2bf(Gs[i] * sc2);
    __syncthreads();
    // ---- P = b*G + c*G G: the upper tiles dealt to the waves, mirrored ----
    {
      int idx = 0;
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = mi; ni < 4; ++ni) {
          if (ni >= NT) continue;
          if ((idx++ & (MUON_LDS_WAVES - 1)) != wave) continue;
          f32x4 pa = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            if (ks >= NK) continue;
            const short8 fa = muon_frag_mmajor(Gb, LD, mi * 16, ks * 32, lane);
            const short8 fb = muon_frag_kmajor(Gb, LD, ks * 32, ni * 16, lane);
            pa = muon_mfma(fa, fb, pa);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = mi * 16 + frow + r, n = ni * 16 + fcol;
            const float g = bf2f(Gb[m * LD + n]);
            const ushort_t p = f2bf(MU_B * g + MU_C * pa[r]);
            Pb[m * LD + n] = p;
            if (mi != ni) Pb[n * LD + m] = p;
          }
        }
    }
    __syncthreads();
    // ---- X = sc*(a*X + X P): a wave owns whole 16-row tiles, in place ------
    for (int mt = wave; mt < (RP >> 4); mt += MUON_LDS_WAVES) {
      short8 fa[2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        fa[ks] = short8{0, 0, 0, 0, 0, 0, 0, 0};
        if (ks < NK) fa[ks] = muon_frag_mmajor(X, LD, mt * 16, ks * 32, lane);
      }
      f32x4 xa[4];
      float xo[4][4];
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        xa[ni] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ni >= NT) continue;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          if (ks >= NK) continue;
          const short8 fb = muon_frag_kmajor(Pb, LD, ks * 32, ni * 16, lane);
          xa[ni] = muon_mfma(fa[ks], fb, xa[ni]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
          xo[ni][r] = bf2f(X[(mt * 16 + frow + r) * LD + ni * 16 + fcol]);
      }
      // every read of the tile's rows is complete before its first write
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        if (ni >= NT) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          X[(mt * 16 + frow + r) * LD + ni * 16 + fcol] =
              f2bf(sc * (MU_A * xo[ni][r] + xa[ni][r]));
      }
    }
    __syncthreads();
  }

  // ---- the result, once ----------------------------------------------------
  if (vec) {
    const int cc = cols >> 3;
    for (int c = tid; c < rows * cc; c += MUON_LDS_THREADS) {
      const int r = c / cc, c8 = (c % cc) * 8;
      *reinterpret_cast<uint4*>(dst + (long)r * cols + c8) =
          *reinterpret_cast<const uint4*>(X + r * LD + c8);
    }
  } else {
    for (int i = tid; i < rows * cols; i += MUON_LDS_THREADS)
      dst[i] = X[(i / cols) * LD + (i % cols)];
  }
}

// ---------------------------------------------------------------------------
// the tiled route.  C = M^T M of a row-major bf16 M [K][cols] in 64 x 64
// output tiles on or above the diagonal: both operands are 64-column panels
// of the same K-major matrix, staged 64 rows at a time (registers -> LDS, two
// buffers, one barrier per step) and read with the transpose read.  The Gram
// matrix takes M = X and splits K over blocks into fp32 planes; the
// polynomial takes M = G (G G = G^T G, G is stored mirrored and so exactly
// symmetric) with the whole K in one block.
// ---------------------------------------------------------------------------
#define MT_LD 72  // row stride of a staged 64-column image, elements
#define MT_IMG (64 * MT_LD)

// 64 rows x 64 columns of row-major M at (k0, c0) -> two 16 B chunks per
// thread; rows at or past kend are zero
DEV void muon_tile_load(const ushort_t* M, int ld, int k0, int kend, int c0,
                        int tid, uint4 (&r)[2]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = tid + j * 256;
    const int k = k0 + (c >> 3);
    r[j] = uint4{0u, 0u, 0u, 0u};
    if (k < kend)
      r[j] = *reinterpret_cast<const uint4*>(M + (long)k * ld + c0 +
                                             (c & 7) * 8);
  }
}

DEV void muon_tile_store(ushort_t* img, int tid, const uint4 (&r)[2]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = tid + j * 256;
    *reinterpret_cast<uint4*>(img + (c >> 3) * MT_LD + (c & 7) * 8) = r[j];
  }
}

// upper-triangle tile p of a T x T tile grid, row by row
DEV void muon_pair(int p, int T, int& ti, int& tj) {
  ti = 0;
  while (p >= T - ti) {
    p -= T - ti;
    ++ti;
  }
  tj = ti + p;
}

// acc (wave (wr, wc): rows 32*wr .. +31, columns 32*wc .. +31 of the tile)
// = sum over k in [kbeg, kend) of M[k][ti*64 + .]^T M[k][tj*64 + .]
DEV void muon_ata_block(const ushort_t* M, int ld, int kbeg, int kend, int ti,
                        int tj, ushort_t* img, f32x4 (&acc)[2][2]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const bool diag = ti == tj;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nt = kend > kbeg ? (kend - kbeg + 63) >> 6 : 0;
  uint4 ra[2], rb[2];
  int cur = 0;
  if (nt > 0) {
    muon_tile_load(M, ld, kbeg, kend, ti * 64, tid, ra);
    muon_tile_store(img, tid, ra);
    if (!diag) {
      muon_tile_load(M, ld, kbeg, kend, tj * 64, tid, rb);
      muon_tile_store(img + MT_IMG, tid, rb);
    }
  }
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const bool more = t + 1 < nt;
    if (more) {  // the next tile's loads fly under this tile's MFMAs
      muon_tile_load(M, ld, kbeg + (t + 1) * 64, kend, ti * 64, tid, ra);
      if (!diag)
        muon_tile_load(M, ld, kbeg + (t + 1) * 64, kend, tj * 64, tid, rb);
    }
    const ushort_t* aimg = img + cur * 2 * MT_IMG;
    const ushort_t* bimg = diag ? aimg : aimg + MT_IMG;
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      short8 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        fa[i] = muon_frag_kmajor(aimg, MT_LD, kh * 32, wr * 32 + i * 16, lane);
        fb[i] = muon_frag_kmajor(bimg, MT_LD, kh * 32, wc * 32 + i * 16, lane);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = muon_mfma(fa[i], fb[j], acc[i][j]);
    }
    if (more) {
      ushort_t* nimg = img + (cur ^ 1) * 2 * MT_IMG;
      muon_tile_store(nimg, tid, ra);
      if (!diag) muon_tile_store(nimg + MT_IMG, tid, rb);
    }
    __syncthreads();
    cur ^= 1;
  }
}

// block (pair p, slice z) stores its tile of X^T X over rows [z*kslice,
// (z+1)*kslice) into plane z; every element of every upper tile of every
// plane is written
extern "C" __global__ __launch_bounds__(256)
void muon_gram_kernel(const ushort_t* X, int rows, int cols, int kslice,
                      float* planes) {
  __shared__ __align__(16) ushort_t img[4 * MT_IMG];
  const int T = cols >> 6, np = T * (T + 1) / 2;
  const int p = blockIdx.x % np, z = blockIdx.x / np;
  int ti, tj;
  muon_pair(p, T, ti, tj);
  f32x4 acc[2][2];
  muon_ata_block(X, cols, z * kslice, min(rows, (z + 1) * kslice), ti, tj,
                 img, acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  float* pl = planes + (long)z * cols * cols;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = ti * 64 + wr * 32 + i * 16 + (lane >> 4) * 4 + r;
        const int n = tj * 64 + wc * 32 + j * 16 + (lane & 15);
        pl[(long)m * cols + n] = acc[i][j][r];
      }
}

// G = bf16(sc^2 * (plane 0 + plane 1 + ...)), planes in index order, each
// upper tile mirrored on store; one block per upper tile
extern "C" __global__ __launch_bounds__(256)
void muon_gram_sum_kernel(const float* planes, int S, int cols,
                          const float* tab, int tab_idx, int first,
                          ushort_t* G) {
  const int T = cols >> 6;
  int ti, tj;
  muon_pair(blockIdx.x, T, ti, tj);
  const float sc = first ? tab[tab_idx] : 1.f;
  const float sc2 = sc * sc;
  const long plane = (long)cols * cols;
  for (int e = threadIdx.x; e < 64 * 64; e += 256) {
    const int m = ti * 64 + (e >> 6), n = tj * 64 + (e & 63);
    const long at = (long)m * cols + n;
    float v = planes[at];
    for (int z = 1; z < S; ++z) v += planes[z * plane + at];
    const ushort_t g = f2bf(v * sc2);
    G[at] = g;
    if (ti != tj) G[(long)n * cols + m] = g;
  }
}

// P = bf16(b*G + c * G G), upper tiles mirrored on store
extern "C" __global__ __launch_bounds__(256)
void muon_poly_kernel(const ushort_t* G, int cols, ushort_t* P) {
  __shared__ __align__(16) ushort_t img[4 * MT_IMG];
  const int T = cols >> 6;
  int ti, tj;
  muon_pair(blockIdx.x, T, ti, tj);
  f32x4 acc[2][2];
  muon_ata_block(G, cols, 0, cols, ti, tj, img, acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = ti * 64 + wr * 32 + i * 16 + (lane >> 4) * 4 + r;
        const int n = tj * 64 + wc * 32 + j * 16 + (lane & 15);
        const long at = (long)m * cols + n;
        const ushort_t pv = f2bf(MU_B * bf2f(G[at]) + MU_C * acc[i][j][r]);
        P[at] = pv;
        if (ti != tj) P[(long)n * cols + m] = pv;
      }
}

// X' = bf16(sc * (a*X + X P)).  A block owns 32 rows of X, resident in LDS as
// both the A operand and the a*X term, and streams P in 64 x 64 tiles (the
// staging of muon_ata_block).  Wave w: row tile w & 1, column tiles 2*(w >> 1)
// and 2*(w >> 1) + 1 of each 64-column chunk.
#define MA_ROWS 32

extern "C" __global__ __launch_bounds__(256)
void muon_apply_kernel(const ushort_t* X, const ushort_t* P, ushort_t* Xn,
                       int rows, int cols, const float* tab, int tab_idx,
                       int first) {
  __shared__ __align__(16) ushort_t panel[MA_ROWS * (MUON_MAX_COLS + 8)];
  __shared__ __align__(16) ushort_t img[2 * MT_IMG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int mt = wave & 1, nh = wave >> 1;
  const int frow = (lane >> 4) * 4, fcol = lane & 15;
  const int ldp = cols + 8, cc = cols >> 3;
  const int m0 = blockIdx.x * MA_ROWS;
  const float sc = first ? tab[tab_idx] : 1.f;
  for (int c = tid; c < MA_ROWS * cc; c += 256) {
    const int r = c / cc, c8 = (c % cc) * 8;
    uint4 v = uint4{0u, 0u, 0u, 0u};
    if (m0 + r < rows)
      v = *reinterpret_cast<const uint4*>(X + (long)(m0 + r) * cols + c8);
    *reinterpret_cast<uint4*>(panel + r * ldp + c8) = v;
  }
  const int nk = cols >> 6, steps = nk * nk;
  uint4 rg[2];
  muon_tile_load(P, cols, 0, cols, 0, tid, rg);
  muon_tile_store(img, tid, rg);
  __syncthreads();
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  int cur = 0;
  for (int st = 0; st < steps; ++st) {
    const int nc = st / nk, kt = st % nk;
    const bool more = st + 1 < steps;
    if (more)
      muon_tile_load(P, cols, ((st + 1) % nk) * 64, cols,
                     ((st + 1) / nk) * 64, tid, rg);
    const ushort_t* pimg = img + cur * MT_IMG;
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      const short8 fa =
          muon_frag_mmajor(panel, ldp, mt * 16, kt * 64 + kh * 32, lane);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const short8 fb =
            muon_frag_kmajor(pimg, MT_LD, kh * 32, (nh * 2 + i) * 16, lane);
        acc[i] = muon_mfma(fa, fb, acc[i]);
      }
    }
    if (kt == nk - 1) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = mt * 16 + frow + r;
          const int col = nc * 64 + (nh * 2 + i) * 16 + fcol;
          const float x = bf2f(panel[row * ldp + col]);
          if (m0 + row < rows)
            Xn[(long)(m0 + row) * cols + col] =
                f2bf(sc * (MU_A * x + acc[i][r]));
        }
        acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    if (more) muon_tile_store(img + (cur ^ 1) * MT_IMG, tid, rg);
    __syncthreads();
    cur ^= 1;
  }
}

// ---------------------------------------------------------------------------
// the final pass: decay + scaled orthogonal update on the weight tensors,
// heavy-ball momentum on the biases; master, average, shadow, zeroed bucket
// ---------------------------------------------------------------------------
DEV float muon_ema_weight(float k, float ema_decay) {
  return 1.f - fminf(ema_decay, (1.f + k) / (10.f + k));
}

template <bool EMA>
__global__ __launch_bounds__(256)
void muon_update_kernel(float* master, float* grad, const float* mom,
                        ushort_t* shadow, long n, GradNormSegs segs,
                        MuonOut out, MuonHyper h, float lr_scale,
                        uint64_t offset, const float* lr_scale_dev,
                        const long* offset_dev, int zero_grad, float* ema,
                        float ema_decay) {
  if (lr_scale_dev) lr_scale = *lr_scale_dev;
  if (offset_dev) offset = (uint64_t)*offset_dev;
  const float lr = lr_scale * h.contrib;
  const float decay = 1.f - lr * h.wd;
  const float ema_w = EMA ? muon_ema_weight((float)(offset + 1), ema_decay)
                          : 0.f;
  const long stride = (long)gridDim.x * blockDim.x;
  const long groups = (n + 3) >> 2;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < groups;
       i += stride) {
    const long base = i * 4;
    const int seg = muon_seg_of(segs, base);
    // a whole group inside one tensor takes the vector path
    const bool vec = base + 3 < n && seg == muon_seg_of(segs, base + 3);
    if (vec) {
      float4 w = *reinterpret_cast<const float4*>(master + base);
      const ushort_t* xo = out.x[seg];
      if (xo) {
        xo += base - segs.off[seg];
        const float step = lr * out.scale[seg];
        w.x = w.x * decay - step * bf2f(xo[0]);
        w.y = w.y * decay - step * bf2f(xo[1]);
        w.z = w.z * decay - step * bf2f(xo[2]);
        w.w = w.w * decay - step * bf2f(xo[3]);
      } else {
        const float4 v = *reinterpret_cast<const float4*>(mom + base);
        w.x = w.x - lr * v.x; w.y = w.y - lr * v.y;
        w.z = w.z - lr * v.z; w.w = w.w - lr * v.w;
      }
      *reinterpret_cast<float4*>(master + base) = w;
      if (EMA) {
        float4 e = *reinterpret_cast<const float4*>(ema + base);
        e.x = e.x - ema_w * (e.x - w.x); e.y = e.y - ema_w * (e.y - w.y);
        e.z = e.z - ema_w * (e.z - w.z); e.w = e.w - ema_w * (e.w - w.w);
        *reinterpret_cast<float4*>(ema + base) = e;
      }
      if (zero_grad)
        *reinterpret_cast<float4*>(grad + base) = float4{0.f, 0.f, 0.f, 0.f};
      if (shadow) {
        shadow[base] = f2bf(w.x); shadow[base + 1] = f2bf(w.y);
        shadow[base + 2] = f2bf(w.z); shadow[base + 3] = f2bf(w.w);
      }
    } else {
      // the scalar tail, and a group that straddles a tensor boundary
      const long jend = min(n, base + 4);
      for (long e = base; e < jend; ++e) {
        const int se = muon_seg_of(segs, e);
        float w = master[e];
        if (out.x[se])
          w = w * decay - (lr * out.scale[se]) *
                              bf2f(out.x[se][e - segs.off[se]]);
        else
          w = w - lr * mom[e];
        master[e] = w;
        if (EMA) {
          const float a = ema[e];
          ema[e] = a - ema_w * (a - w);
        }
        if (zero_grad) grad[e] = 0.f;
        if (shadow) shadow[e] = f2bf(w);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
bool muon_lds_fits(int rows, int cols) {
  return rows >= 1 && cols >= 1 && cols <= 64 &&
         muon_lds_bytes(rows, cols) <= MUON_LDS_BYTES;
}

bool muon_tiled_fits(int rows, int cols) {
  return rows >= 8 && rows % 8 == 0 && cols >= 64 && cols % 64 == 0 &&
         cols <= MUON_MAX_COLS;
}

int muon_gram_split(int rows, int cols, int* kslice) {
  // about one block per CU: the upper tiles times the row slices
  const int T = cols / 64, np = T * (T + 1) / 2;
  int want = 256 / np;
  want = want < 1 ? 1 : want > MUON_MAX_SPLIT ? MUON_MAX_SPLIT : want;
  int ks = ((rows + want - 1) / want + 63) & ~63;
  *kslice = ks;
  return (rows + ks - 1) / ks;
}

bool muon_plan(const GradNormSegs& segs, const int* cols, unsigned adapt,
               int force_route, MuonPlan* pl, int* bad) {
  *pl = MuonPlan{};
  pl->n = segs.n;
  long at = 0, gmax = 0, planes = 0;
  for (int t = 0; t < segs.n; ++t) {
    pl->uoff[t] = pl->x2off[t] = -1;
    if (!((adapt >> t) & 1u)) continue;
    const long numel = segs.len[t];
    const int c = cols[t];
    *bad = t;
    if (c < 1 || numel < c || numel % c != 0 || numel / c > (1L << 24))
      return false;
    const int r = (int)(numel / c);
    int route = force_route;
    if (route == MUON_NONE)
      route = muon_lds_fits(r, c) ? MUON_LDS
              : muon_tiled_fits(r, c) ? MUON_TILED : MUON_NONE;
    if (route == MUON_LDS ? !muon_lds_fits(r, c)
                          : !(route == MUON_TILED && muon_tiled_fits(r, c)))
      return false;
    pl->route[t] = route;
    pl->rows[t] = r;
    pl->cols[t] = c;
    pl->scale[t] = (float)(0.2 * sqrt((double)(r > c ? r : c)));
    pl->uoff[t] = at;
    at += (numel + 7) & ~7L;  // every matrix starts 16 B aligned
    if (route == MUON_TILED) {
      pl->x2off[t] = at;
      at += numel;  // rows % 8 == 0 and cols % 64 == 0
      if ((long)c * c > gmax) gmax = (long)c * c;
      int ks;
      const long need = (long)muon_gram_split(r, c, &ks) * c * c;
      if (need > planes) planes = need;
    }
  }
  *bad = -1;
  pl->goff = at;
  pl->poff = at + gmax;
  pl->bf16_elems = at + 2 * gmax;
  pl->plane_floats = planes;
  return true;
}

static MuonHyper muon_hyper(const MuonArgs& a) {
  MuonHyper h;
  h.mu = (float)a.mu;
  h.wd = (float)a.wd;
  h.s = a.grad_scale;
  h.contrib = rintf(1.f / a.grad_scale);
  h.adapt = a.adapt;
  return h;
}

void launch_muon_momentum(const float* grad, float* mom, unsigned short* ws,
                          long n, const GradNormSegs& segs,
                          const MuonPlan& pl, const MuonArgs& a,
                          uint64_t offset, const long* offset_dev,
                          const float* clip_coef_dev, float* tab, float* part,
                          unsigned* ticket, hipStream_t s) {
  int blocks, chain;
  grad_norm_plan(n, &blocks, &chain);
  MuonUoff uo;
  for (int t = 0; t < GRAD_NORM_MAX_SEGS; ++t) uo.off[t] = pl.uoff[t];
  hipLaunchKernelGGL(muon_momentum_kernel, dim3(blocks), dim3(GN_THREADS), 0,
                     s, grad, mom, ws, n, segs, uo, grad_norm_chunk(n),
                     muon_hyper(a), offset, offset_dev, a.dc_keep, a.seed,
                     clip_coef_dev, tab, part, ticket);
}

void launch_muon_ns(const MuonPlan& pl, unsigned short* ws, float* planes,
                    const float* tab, int iters, const unsigned short** out,
                    hipStream_t s) {
  // ---- every LDS tensor in one launch, in place ----------------------------
  MuonLdsArgs la{};
  int nl = 0;
  long bytes = 0;
  for (int t = 0; t < pl.n; ++t) {
    out[t] = nullptr;
    if (pl.route[t] != MUON_LDS) continue;
    la.src[nl] = la.dst[nl] = ws + pl.uoff[t];
    la.rows[nl] = pl.rows[t];
    la.cols[nl] = pl.cols[t];
    la.tab[nl] = t;
    const long b = muon_lds_bytes(pl.rows[t], pl.cols[t]);
    if (b > bytes) bytes = b;
    out[t] = ws + pl.uoff[t];
    ++nl;
  }
  if (nl) {
    // above 64 KB the dynamic LDS size has to be granted once per kernel
    static const hipError_t granted = hipFuncSetAttribute(
        reinterpret_cast<const void*>(&muon_ns_lds_kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize, MUON_LDS_BYTES);
    if (granted != hipSuccess)
      fprintf(stderr, "muon_ns_lds_kernel: %s\n", hipGetErrorString(granted));
    hipLaunchKernelGGL(muon_ns_lds_kernel, dim3(nl), dim3(MUON_LDS_THREADS),
                       (size_t)bytes, s, la, tab, iters);
  }
  // ---- the tiled tensors, one after the other, ping-pong X ------------------
  for (int t = 0; t < pl.n; ++t) {
    if (pl.route[t] != MUON_TILED) continue;
    const int rows = pl.rows[t], cols = pl.cols[t];
    const int T = cols / 64, np = T * (T + 1) / 2;
    int ks;
    const int S = muon_gram_split(rows, cols, &ks);
    unsigned short* src = ws + pl.uoff[t];
    unsigned short* dst = ws + pl.x2off[t];
    unsigned short* G = ws + pl.goff;
    unsigned short* P = ws + pl.poff;
    for (int it = 0; it < iters; ++it) {
      const int first = it == 0;
      hipLaunchKernelGGL(muon_gram_kernel, dim3(np * S), dim3(256), 0, s, src,
                         rows, cols, ks, planes);
      hipLaunchKernelGGL(muon_gram_sum_kernel, dim3(np), dim3(256), 0, s,
                         planes, S, cols, tab, t, first, G);
      hipLaunchKernelGGL(muon_poly_kernel, dim3(np), dim3(256), 0, s, G, cols,
                         P);
      hipLaunchKernelGGL(muon_apply_kernel,
                         dim3((rows + MA_ROWS - 1) / MA_ROWS), dim3(256), 0, s,
                         src, P, dst, rows, cols, tab, t, first);
      unsigned short* x = src;
      src = dst;
      dst = x;
    }
    out[t] = src;
  }
}

void launch_muon_update(float* master, float* grad, const float* mom,
                        unsigned short* shadow, long n,
                        const GradNormSegs& segs, const MuonPlan& pl,
                        const unsigned short* const* out, const MuonArgs& a,
                        float lr_scale, uint64_t offset,
                        const float* lr_scale_dev, const long* offset_dev,
                        int zero_grad, float* ema, float ema_decay,
                        hipStream_t s) {
  MuonOut o{};
  for (int t = 0; t < pl.n; ++t) {
    o.x[t] = out[t];
    o.scale[t] = pl.scale[t];
  }
  const long groups = (n + 3) / 4;
  long blocks = (groups + 255) / 256;
  blocks = blocks > 2048 ? 2048 : blocks < 1 ? 1 : blocks;
  const MuonHyper h = muon_hyper(a);
  if (ema)
    hipLaunchKernelGGL((muon_update_kernel<true>), dim3((int)blocks),
                       dim3(256), 0, s, master, grad, mom, shadow, n, segs, o,
                       h, lr_scale, offset, lr_scale_dev, offset_dev,
                       zero_grad, ema, ema_decay);
  else
    hipLaunchKernelGGL((muon_update_kernel<false>), dim3((int)blocks),
                       dim3(256), 0, s, master, grad, mom, shadow, n, segs, o,
                       h, lr_scale, offset, lr_scale_dev, offset_dev,
                       zero_grad, ema, ema_decay);
}
