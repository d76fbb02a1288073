// Segmented squared norm of the flat fp32 gradient bucket -> per-tensor and
// global gradient norms plus the clip_grad_norm_ coefficient, all on the
// device in ONE launch (--clip_grad_norm; docs/KERNELS.md "grad_norm").
//
// Reduction order (no float atomics anywhere, so the result is a pure
// function of the bucket contents, n, the segment table and the geometry
// below; two launches on the same input give the same bits):
//   1. block b owns the fixed chunk [b*chunk, (b+1)*chunk) and, for every
//      segment that meets it, reduces the intersection: a thread squares its
//      float4 groups (x*x + y*y) + (z*z + w*w) and adds them in address order,
//      then a scalar head / tail element where the segment starts or ends off
//      a 16 B boundary; a fixed shuffle tree per wave; the wave sums are added
//      in wave order and STORED as part[s][b]
//   2. the last block to take a ticket adds, per segment, the partials of the
//      blocks that meet it: thread t takes blocks first + t, first + t + 256,
//      ... in index order, then the same shuffle tree and wave order
//   3. one thread adds the segment sums in index order -> the total
// The softmax_xent_t_kernel idiom: agent-scope stores and loads of the
// partials, __threadfence, a self-resetting ticket, a persistent workspace.

#include "common.h"
#include "kernels.h"

#define GN_THREADS 256
#define GN_WAVES (GN_THREADS / 64)

// fixed shuffle tree of one wave; lane 0 holds the sum
DEV float gn_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

DEV float gn_sq4(float4 g) {
  return (g.x * g.x + g.y * g.y) + (g.z * g.z + g.w * g.w);
}

extern "C" __global__ __launch_bounds__(GN_THREADS)
void grad_norm_kernel(const float* grad, long n, GradNormSegs segs, long chunk,
                      float grad_scale, float clip, float* stats,
                      long* clipped_steps, float* part, unsigned* ticket) {
  __shared__ float wred[GRAD_NORM_MAX_SEGS][GN_WAVES];
  __shared__ int is_last;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const long c0 = (long)blockIdx.x * chunk;
  const long c1 = min(n, c0 + chunk);

  // ---- 1. this block's chunk, one segment at a time (block-uniform loop) --
  for (int s = 0; s < segs.n; ++s) {
    const long a = max(c0, segs.off[s]);
    const long b = min(c1, segs.off[s] + segs.len[s]);
    if (a >= b) continue;
    // [a, a4): scalar head, [a4, b4): 16 B groups, [b4, b): scalar tail
    long a4 = min(b, (a + 3) & ~3L);
    long b4 = max(a4, b & ~3L);
    float acc = 0.f;
    const long g1 = b4 >> 2;
    // four 16 B loads per thread in flight per trip: a group past the end
    // re-reads the range's last group (an address inside it, so the loads
    // need no branch) and counts as zero
    for (long g = (a4 >> 2) + tid; g < g1; g += 4 * GN_THREADS) {
      float4 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        long gj = min(g + j * GN_THREADS, g1 - 1);
        v[j] = *reinterpret_cast<const float4*>(grad + gj * 4);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc += g + j * GN_THREADS < g1 ? gn_sq4(v[j]) : 0.f;
    }
    if (a + tid < a4) { float x = grad[a + tid]; acc += x * x; }
    if (b4 + tid < b) { float x = grad[b4 + tid]; acc += x * x; }
    acc = gn_wave_sum(acc);
    if (lane == 0) wred[s][wave] = acc;
  }
  __syncthreads();
  if (tid == 0) {
    for (int s = 0; s < segs.n; ++s) {
      const long a = max(c0, segs.off[s]);
      const long b = min(c1, segs.off[s] + segs.len[s]);
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
    float acc = 0.f;
    if (segs.len[s] > 0) {
      const long first = segs.off[s] / chunk;
      const long lastb = (segs.off[s] + segs.len[s] - 1) / chunk;
      for (long b = first + tid; b <= lastb; b += GN_THREADS)
        acc += __hip_atomic_load(&part[(long)s * GRAD_NORM_MAX_BLOCKS + b],
                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    acc = gn_wave_sum(acc);
    if (lane == 0) wred[s][wave] = acc;
  }
  __syncthreads();
  if (tid != 0) return;
  // ---- 3. segments in index order ------------------------------------------
  float total = 0.f;
  for (int s = 0; s < segs.n; ++s) {
    float r = wred[s][0];
    for (int w = 1; w < GN_WAVES; ++w) r += wred[s][w];
    stats[2 + s] = grad_scale * sqrtf(r);
    total += r;
  }
  const float norm = grad_scale * sqrtf(total);
  // torch.nn.utils.clip_grad_norm_: clip = +inf gives exactly 1
  const float coef = fminf(1.f, clip / (norm + 1e-6f));
  stats[0] = norm;
  stats[1] = coef;
  if (coef < 1.f) *clipped_steps += 1;
  __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// elements per block: GRAD_NORM_CHUNK while that needs at most
// GRAD_NORM_MAX_BLOCKS blocks, the next multiple of it above that
static long grad_norm_chunk(long n) {
  long per = (long)GRAD_NORM_CHUNK * GRAD_NORM_MAX_BLOCKS;
  long k = (n + per - 1) / per;
  return (long)GRAD_NORM_CHUNK * (k < 1 ? 1 : k);
}

void grad_norm_plan(long n, int* blocks, int* chain) {
  const long chunk = grad_norm_chunk(n);
  const long nb = n < 1 ? 1 : (n + chunk - 1) / chunk;
  *blocks = (int)nb;
  // the longest run of fp32 additions one element passes through:
  // in a 16 B group 2, one add per group of the thread (4 per
  // GRAD_NORM_CHUNK elements of the chunk), head + tail 2, shuffle tree 6,
  // waves GN_WAVES; last block: ceil(blocks / 256) partials per thread,
  // tree 6, waves GN_WAVES; then at most GRAD_NORM_MAX_SEGS segments
  const long trips = chunk / GRAD_NORM_CHUNK;
  *chain = (int)(2 + 4 * trips + 2 + 6 + GN_WAVES +
                 (nb + GN_THREADS - 1) / GN_THREADS + 6 + GN_WAVES +
                 GRAD_NORM_MAX_SEGS);
}

void launch_grad_norm(const float* grad, long n, GradNormSegs segs,
                      float grad_scale, float clip, float* stats,
                      long* clipped_steps, float* part, unsigned* ticket,
                      hipStream_t s) {
  int blocks, chain;
  grad_norm_plan(n, &blocks, &chain);
  hipLaunchKernelGGL(grad_norm_kernel, dim3(blocks), dim3(GN_THREADS), 0, s,
                     grad, n, segs, grad_norm_chunk(n), grad_scale, clip,
                     stats, clipped_steps, part, ticket);
}
