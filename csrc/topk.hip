// Top-k gradient sparsification with error feedback on the flat fp32 bucket
// (--grad_topk; docs/KERNELS.md "Top-k sparsification").
//
// Per tensor t (segment [off_t, off_t + n_t) of the bucket) the k_t elements
// of a = resid + grad that come first under "larger |a| first, then smaller
// index first" are selected, written as (index, value bits) pairs in ascending
// index order into the slots [base_t, base_t + k_t) of the payload, and taken
// out of the residual.  Five launches on one stream, no float atomics:
//   topk_hist_kernel x 3   radix select of the k_t-th largest key over the
//                          31-bit key bits(a) & 0x7fffffff, digits of 11, 10
//                          and 10 bits from the top.  Pass 0 also stores a into
//                          resid.  Per block and segment an LDS histogram of
//                          the digit (keys whose higher digits equal the
//                          prefix chosen so far), flushed with integer atomics
//                          into the segment's global histogram; the last block
//                          (ticket) walks the bins from the top, one wave per
//                          segment, fixes the digit and the count still needed
//                          and clears the histogram for the next pass.
//   topk_count_kernel      per (segment, block) the number of keys above and
//                          equal to the threshold T_t; the last block turns
//                          them into exclusive prefix sums in block order.
//   topk_compact_kernel    ranks every element in index order (ballots,
//                          popcounts of the lower lanes, an LDS table over the
//                          waves, the two block prefixes) and writes the pair,
//                          the residual and the bucket.
// grad_norm_kernel's geometry: block b owns the fixed chunk [b * chunk,
// (b + 1) * chunk) and walks it one segment at a time.  Integer adds commute,
// every slot is a pure function of the input: equal inputs give equal bits.
// topk_scatter_kernel adds one rank's pairs into the dense bucket; launched
// once per rank in rank order, the stream fixes the order of the sums.

#include "grad_norm_common.h"

#define TK_THREADS GN_THREADS
#define TK_WAVES GN_WAVES
#define TK_TILE (4 * TK_THREADS)  // elements per compaction tile

// workspace layout (ints): the per-segment histograms, the table (T / prefix,
// keys above T, need_eq / count still needed, k_t per segment), the per
// (segment, block) counts of keys above and equal, the ticket
#define TK_HIST 0
#define TK_TAB (TK_HIST + GRAD_NORM_MAX_SEGS * TOPK_BINS)
#define TK_CGT (TK_TAB + 4 * GRAD_NORM_MAX_SEGS)
#define TK_CEQ (TK_CGT + GRAD_NORM_MAX_SEGS * GRAD_NORM_MAX_BLOCKS)
#define TK_TICKET (TK_CEQ + GRAD_NORM_MAX_SEGS * GRAD_NORM_MAX_BLOCKS)
static_assert(TK_TICKET + 1 == TOPK_WS_INTS, "workspace layout");

DEV unsigned tk_key(float x) { return __float_as_uint(x) & 0x7fffffffu; }

DEV int tk_ld(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

DEV void tk_st(int* p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One thread's share of [a, b): 16 B groups, four per thread in flight per
// trip, then a scalar head / tail element where the range starts or ends off
// a 16 B boundary.  FIRST: the value is resid + grad and is stored to resid
// (every element is read and written by exactly one thread).
template <bool FIRST, class F>
DEV void tk_walk(const float* grad, float* resid, long a, long b, int tid,
                 F& f) {
  const long a4 = min(b, (a + 3) & ~3L);
  const long b4 = max(a4, b & ~3L);
  const long g1 = b4 >> 2;
  for (long g = (a4 >> 2) + tid; g < g1; g += 4 * TK_THREADS) {
    float4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long gj = g + j * TK_THREADS;
      if (gj < g1) {
        v[j] = *reinterpret_cast<const float4*>(resid + gj * 4);
        if (FIRST) {
          const float4 w = *reinterpret_cast<const float4*>(grad + gj * 4);
          v[j].x += w.x; v[j].y += w.y; v[j].z += w.z; v[j].w += w.w;
          *reinterpret_cast<float4*>(resid + gj * 4) = v[j];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (g + j * TK_THREADS < g1) {
        f(v[j].x); f(v[j].y); f(v[j].z); f(v[j].w);
      }
  }
  for (int side = 0; side < 2; ++side) {
    const long i = (side ? b4 : a) + tid;
    if (i < (side ? b : a4)) {
      float x = resid[i];
      if (FIRST) { x += grad[i]; resid[i] = x; }
      f(x);
    }
  }
}

struct TkHistF {
  int* hist;
  unsigned prefix;
  int shift, bits, pass;
  DEV void operator()(float x) {
    const unsigned key = tk_key(x);
    if (pass == 0 || (key >> (shift + bits)) == prefix)
      atomicAdd(&hist[(key >> shift) & ((1u << bits) - 1u)], 1);
  }
};

struct TkCountF {
  unsigned T;
  int gt, eq;
  DEV void operator()(float x) {
    const unsigned key = tk_key(x);
    gt += key > T;
    eq += key == T;
  }
};

// tid 0 after a __syncthreads that follows every thread's __threadfence:
// true in the last block to arrive
DEV int tk_ticket(unsigned* ticket) {
  __threadfence();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const int last = atomicAdd(ticket, 1u) == gridDim.x - 1;
  if (last) __threadfence();
  return last;
}

// inclusive scan over the lanes of one wave, lane 0 first
DEV int tk_wave_scan(int v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(v, off, 64);
    if (lane >= off) v += t;
  }
  return v;
}

extern "C" __global__ __launch_bounds__(TK_THREADS)
void topk_hist_kernel(const float* grad, float* resid, long n,
                      GradNormSegs segs, TopkSegs ks, long chunk, int pass,
                      int* ws) {
  __shared__ int hist[TOPK_BINS];
  __shared__ int is_last;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const long c0 = (long)blockIdx.x * chunk;
  const long c1 = min(n, c0 + chunk);
  const int bits = pass == 0 ? 11 : 10;
  const int shift = pass == 0 ? 20 : pass == 1 ? 10 : 0;
  const int nb = 1 << bits;
  int* ghist = ws + TK_HIST;
  int* tab = ws + TK_TAB;

  // ---- 1. this block's chunk, one segment at a time (block-uniform loop) --
  for (int s = 0; s < segs.n; ++s) {
    const long a = max(c0, segs.off[s]);
    const long b = min(c1, segs.off[s] + segs.len[s]);
    if (a >= b) continue;
    for (int i = tid; i < nb; i += TK_THREADS) hist[i] = 0;
    __syncthreads();
    TkHistF f{hist, pass ? (unsigned)tab[4 * s] : 0u, shift, bits, pass};
    if (pass == 0) tk_walk<true>(grad, resid, a, b, tid, f);
    else tk_walk<false>(grad, resid, a, b, tid, f);
    __syncthreads();
    for (int i = tid; i < nb; i += TK_THREADS) {
      const int c = hist[i];
      if (c) atomicAdd(&ghist[s * TOPK_BINS + i], c);
    }
    __syncthreads();  // the next segment clears hist
  }
  __threadfence();  // this thread's flushes visible before the ticket
  __syncthreads();
  if (tid == 0) is_last = tk_ticket(reinterpret_cast<unsigned*>(ws + TK_TICKET));
  __syncthreads();
  if (!is_last) return;

  // ---- 2. last block: one wave per segment walks the bins from the top ----
  for (int s = wave; s < segs.n; s += TK_WAVES) {
    const unsigned prefix = pass ? (unsigned)tab[4 * s] : 0u;
    const int need = pass ? tab[4 * s + 2] : ks.k[s];
    if (segs.len[s] <= 0 || need <= 0) {
      // empty tensor: a threshold no key reaches, nothing needed
      if (lane == 0) {
        tab[4 * s] = -1; tab[4 * s + 1] = 0;
        tab[4 * s + 2] = 0; tab[4 * s + 3] = 0;
      }
      continue;
    }
    int above = 0, digit = 0;
    for (int top = nb - 1; top >= 0; top -= 64) {  // wave-uniform
      const int c = tk_ld(&ghist[s * TOPK_BINS + top - lane]);
      const int inc = tk_wave_scan(c, lane);
      const unsigned long long m = __ballot(above + inc >= need);
      if (m) {
        const int l = __ffsll((long long)m) - 1;
        digit = top - l;
        above += __shfl(inc - c, l, 64);
        break;
      }
      above += __shfl(inc, 63, 64);
    }
    if (lane == 0) {
      tab[4 * s] = (int)((prefix << bits) | (unsigned)digit);
      tab[4 * s + 2] = need - above;  // >= 1
      if (pass == 2) {
        tab[4 * s + 1] = ks.k[s] - (need - above);
        tab[4 * s + 3] = ks.k[s];
      }
    }
  }
  __syncthreads();
  // re-arm: the next pass (or the next step) adds into zeroed histograms
  for (int i = tid; i < segs.n * TOPK_BINS; i += TK_THREADS) ghist[i] = 0;
  if (tid == 0) tk_st(ws + TK_TICKET, 0);
}

extern "C" __global__ __launch_bounds__(TK_THREADS)
void topk_count_kernel(float* resid, long n, GradNormSegs segs, long chunk,
                       int* ws) {
  __shared__ int cnt[GRAD_NORM_MAX_SEGS][2];
  __shared__ int is_last;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const long c0 = (long)blockIdx.x * chunk;
  const long c1 = min(n, c0 + chunk);
  const int* tab = ws + TK_TAB;
  int* cgt = ws + TK_CGT;
  int* ceq = ws + TK_CEQ;

  if (tid < 2 * GRAD_NORM_MAX_SEGS) cnt[tid >> 1][tid & 1] = 0;
  __syncthreads();
  for (int s = 0; s < segs.n; ++s) {
    const long a = max(c0, segs.off[s]);
    const long b = min(c1, segs.off[s] + segs.len[s]);
    if (a >= b) continue;
    TkCountF f{(unsigned)tab[4 * s], 0, 0};
    tk_walk<false>(nullptr, resid, a, b, tid, f);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      f.gt += __shfl_down(f.gt, off, 64);
      f.eq += __shfl_down(f.eq, off, 64);
    }
    if (lane == 0) {
      atomicAdd(&cnt[s][0], f.gt);
      atomicAdd(&cnt[s][1], f.eq);
    }
  }
  __syncthreads();
  if (tid == 0) {
    for (int s = 0; s < segs.n; ++s) {
      const long a = max(c0, segs.off[s]);
      const long b = min(c1, segs.off[s] + segs.len[s]);
      if (a >= b) continue;
      tk_st(&cgt[s * GRAD_NORM_MAX_BLOCKS + blockIdx.x], cnt[s][0]);
      tk_st(&ceq[s * GRAD_NORM_MAX_BLOCKS + blockIdx.x], cnt[s][1]);
    }
    is_last = tk_ticket(reinterpret_cast<unsigned*>(ws + TK_TICKET));
  }
  __syncthreads();
  if (!is_last) return;

  // last block: exclusive prefix sums over each segment's blocks, in block
  // order, one wave per segment, 64 blocks per trip
  for (int s = wave; s < segs.n; s += TK_WAVES) {
    if (segs.len[s] <= 0) continue;
    const long first = segs.off[s] / chunk;
    const long lastb = (segs.off[s] + segs.len[s] - 1) / chunk;
    int run_gt = 0, run_eq = 0;
    for (long b0 = first; b0 <= lastb; b0 += 64) {  // wave-uniform
      const long b = b0 + lane;
      const bool ok = b <= lastb;
      const long at = s * GRAD_NORM_MAX_BLOCKS + (ok ? b : lastb);
      const int g = ok ? tk_ld(&cgt[at]) : 0;
      const int e = ok ? tk_ld(&ceq[at]) : 0;
      const int ig = tk_wave_scan(g, lane), ie = tk_wave_scan(e, lane);
      if (ok) {
        cgt[at] = run_gt + ig - g;
        ceq[at] = run_eq + ie - e;
      }
      run_gt += __shfl(ig, 63, 64);
      run_eq += __shfl(ie, 63, 64);
    }
  }
  if (tid == 0) tk_st(ws + TK_TICKET, 0);
}

// Tiles of TK_TILE elements in index order; inside a tile element j * 256 +
// tid, so the index order is (j, wave, lane): the lane rank is a popcount of
// the ballot's lower lanes, the (j, wave) prefix a walk over a 4 x 4 LDS
// table, the block prefix comes from topk_count_kernel.  An element with
// key == T is selected while its rank among the equal keys is below need_eq;
// the number of selected elements before element i of the segment is then
// (keys above T before i) + min(keys equal to T before i, need_eq).
extern "C" __global__ __launch_bounds__(TK_THREADS)
void topk_compact_kernel(float* grad, float* resid, long n, GradNormSegs segs,
                         TopkSegs ks, long chunk, int K, int* payload,
                         int dense, const int* ws) {
  __shared__ int wc[2][4][TK_WAVES];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const long c0 = (long)blockIdx.x * chunk;
  const long c1 = min(n, c0 + chunk);
  const int* tab = ws + TK_TAB;
  const unsigned long long lower = (1ull << lane) - 1ull;

  for (int s = 0; s < segs.n; ++s) {
    const long a = max(c0, segs.off[s]);
    const long b = min(c1, segs.off[s] + segs.len[s]);
    if (a >= b) continue;
    const unsigned T = (unsigned)tab[4 * s];
    const int need_eq = tab[4 * s + 2];
    const int k = ks.k[s], base = ks.base[s];
    int run_gt = ws[TK_CGT + s * GRAD_NORM_MAX_BLOCKS + blockIdx.x];
    int run_eq = ws[TK_CEQ + s * GRAD_NORM_MAX_BLOCKS + blockIdx.x];
    for (long t0 = a; t0 < b; t0 += TK_TILE) {  // block-uniform
      float x[4];
      bool pg[4], pe[4];
      int rg[4], re[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long i = t0 + j * TK_THREADS + tid;
        x[j] = i < b ? resid[i] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long i = t0 + j * TK_THREADS + tid;
        const unsigned key = tk_key(x[j]);
        pg[j] = i < b && key > T;
        pe[j] = i < b && key == T;
        const unsigned long long bg = __ballot(pg[j]);
        const unsigned long long be = __ballot(pe[j]);
        rg[j] = __popcll(bg & lower);
        re[j] = __popcll(be & lower);
        if (lane == 0) {
          wc[0][j][wave] = __popcll(bg);
          wc[1][j][wave] = __popcll(be);
        }
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int w = 0; w < TK_WAVES; ++w) {
          if (w == wave) {
            const long i = t0 + j * TK_THREADS + tid;
            const int eq_rank = run_eq + re[j];
            const bool sel = pg[j] || (pe[j] && eq_rank < need_eq);
            const int rank = run_gt + rg[j] + min(eq_rank, need_eq);
            if (i < b) {
              if (sel && rank < k) {
                payload[base + rank] = (int)i;
                payload[K + base + rank] = (int)__float_as_uint(x[j]);
                resid[i] = 0.f;
              }
              grad[i] = sel && dense ? x[j] : 0.f;
            }
          }
          run_gt += wc[0][j][w];
          run_eq += wc[1][j][w];
        }
      }
      __syncthreads();  // the next tile rewrites wc
    }
  }
}

// one rank's pairs into the dense bucket: indices are unique within one
// payload, so load-add-store is race-free.  assign: the bucket is known to be
// zero (the first rank), the load is skipped; 0 + v keeps the sum's bits.
extern "C" __global__ __launch_bounds__(TK_THREADS)
void topk_scatter_kernel(const int* payload, int K, float* grad, long n,
                         int assign) {
  const int i = blockIdx.x * TK_THREADS + threadIdx.x;
  if (i >= K) return;
  const long idx = payload[i];
  if (idx < 0 || idx >= n) return;  // a foreign payload never writes outside
  const float v = __uint_as_float((unsigned)payload[K + i]);
  grad[idx] = (assign ? 0.f : grad[idx]) + v;
}

void launch_topk_compress(float* grad, float* resid, long n, GradNormSegs segs,
                          TopkSegs ks, int K, int* payload, int dense, int* ws,
                          hipStream_t s) {
  const long chunk = grad_norm_chunk(n);
  const int blocks = (int)((n + chunk - 1) / chunk);
  for (int pass = 0; pass < 3; ++pass)
    hipLaunchKernelGGL(topk_hist_kernel, dim3(blocks), dim3(TK_THREADS), 0, s,
                       grad, resid, n, segs, ks, chunk, pass, ws);
  hipLaunchKernelGGL(topk_count_kernel, dim3(blocks), dim3(TK_THREADS), 0, s,
                     resid, n, segs, chunk, ws);
  hipLaunchKernelGGL(topk_compact_kernel, dim3(blocks), dim3(TK_THREADS), 0, s,
                     grad, resid, n, segs, ks, chunk, K, payload, dense, ws);
}

void launch_topk_scatter(const int* payload, int K, float* grad, long n,
                         int assign, hipStream_t s) {
  if (K < 1) return;
  hipLaunchKernelGGL(topk_scatter_kernel, dim3((K + TK_THREADS - 1) / TK_THREADS),
                     dim3(TK_THREADS), 0, s, payload, K, grad, n, assign);
}
