// What grad_norm_kernel (grad_norm.hip) and lars_norm_kernel (lars.hip) share:
// the fixed geometry, the shuffle tree and the last block's ordered sum of
// the partials.  The per-chunk reduction they also share is
// grad_norm_range.inc.  Both kernels inline the SAME code, so the gradient
// side of lars_norm_kernel adds the same values in the same order as
// grad_norm_kernel and gives the same bits (docs/KERNELS.md "LARS").
#pragma once

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

// Last block: one thread's share of segment s's per-block partials, blocks
// first + tid, first + tid + 256, ... in index order (agent-scope loads)
DEV float gn_partials(const float* part, long off, long len, int s,
                      long chunk, int tid) {
  float acc = 0.f;
  if (len > 0) {
    const long first = off / chunk;
    const long lastb = (off + len - 1) / chunk;
    for (long b = first + tid; b <= lastb; b += GN_THREADS)
      acc += __hip_atomic_load(&part[(long)s * GRAD_NORM_MAX_BLOCKS + b],
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return acc;
}

// elements per block: GRAD_NORM_CHUNK while that needs at most
// GRAD_NORM_MAX_BLOCKS blocks, the next multiple of it above that
static inline long grad_norm_chunk(long n) {
  long per = (long)GRAD_NORM_CHUNK * GRAD_NORM_MAX_BLOCKS;
  long k = (n + per - 1) / per;
  return (long)GRAD_NORM_CHUNK * (k < 1 ? 1 : k);
}
