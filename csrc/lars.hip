// LARS (--lars_eta; You, Gitman, Ginsburg 2017): per-tensor trust ratios of
// the flat fp32 master and the flat fp32 gradient bucket, on the device in ONE
// launch (docs/KERNELS.md "LARS").  lars_norm_kernel is grad_norm_kernel with
// a second operand: the same fixed chunks, the same by-value segment table,
// the same per-(segment, block) partials and last-block order, taken over the
// gradient AND the master in the same trip (eight 16 B loads in flight per
// thread, two accumulators).  The gradient side inlines grad_norm_kernel's
// own code (grad_norm_common.h, grad_norm_range.inc), so its sums are the same bits, and with
// clip > 0 the kernel also writes what grad_norm_kernel writes (clip_stats,
// clipped_steps): LARS + clipping is one reduction launch, not two.
//
// Everything is STORED (no accumulation, no fill launch, no float atomics):
//   lars_tab[2t]     a_t = ratio_t * coef          (the SGD pass: g = a_t * g)
//   lars_tab[2t + 1] d_t = ratio_t * wd / s        (then g += d_t * w)
//   lars_stats[3t..] (wn_t, gn_t, ratio_t)
// with wn_t = sqrt(sum w^2), gn_t = coef * (s * sqrt(sum g^2)), s =
// grad_scale, coef the clip coefficient (exactly 1 without clipping) and, for
// the tensors whose bit is set in `adapt`,
//   ratio_t = (wn_t > 0 && gn_t > 0) ? eta * wn_t / (gn_t + wd * wn_t) : 1;
// the others keep ratio 1 and get no decay (d_t = 0, a_t = coef).

#include "grad_norm_common.h"

// new code is built without the packed-fp32 VALU forms
#define LARS_TARGET __attribute__((target("no-packed-fp32-ops")))

// gn_sq4 as grad_norm_kernel's build contracts it (a packed multiply of
// (y, z), a packed fma of (x, w) onto it): (x*x + fl(y*y)) + (w*w + fl(z*z)),
// each bracket one fma.  Spelled out here because without the packed forms the
// compiler contracts the same source the other way round for (z, w), which
// rounds differently; tests/test_lars_gpu.py holds the two kernels to the
// same bits.
DEV float lars_sq4(float4 g) {
  return fmaf(g.x, g.x, g.y * g.y) + fmaf(g.w, g.w, g.z * g.z);
}

extern "C" __global__ __launch_bounds__(GN_THREADS) LARS_TARGET
void lars_norm_kernel(const float* master, const float* grad, long n,
                      GradNormSegs segs, long chunk, unsigned adapt,
                      float grad_scale, float eta, float wd, float clip,
                      float* lars_tab, float* lars_stats, float* clip_stats,
                      long* clipped_steps, float* part, unsigned* ticket) {
  // [0]: gradient, [1]: master
  __shared__ float wred[2][GRAD_NORM_MAX_SEGS][GN_WAVES];
  __shared__ int is_last;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const long c0 = (long)blockIdx.x * chunk;
  const long c1 = min(n, c0 + chunk);
  float* const partw = part + GRAD_NORM_MAX_SEGS * GRAD_NORM_MAX_BLOCKS;

  // ---- 1. this block's chunk, one segment at a time (block-uniform loop) --
  for (int s = 0; s < segs.n; ++s) {
    const long a = max(c0, segs.off[s]);
    const long b = min(c1, segs.off[s] + segs.len[s]);
    if (a >= b) continue;
    float acc = 0.f, accw = 0.f;
#define GN_RANGE_TWO 1
#define GN_RANGE_SQ4 lars_sq4
#include "grad_norm_range.inc"
#undef GN_RANGE_TWO
#undef GN_RANGE_SQ4
    acc = gn_wave_sum(acc);
    accw = gn_wave_sum(accw);
    if (lane == 0) {
      wred[0][s][wave] = acc;
      wred[1][s][wave] = accw;
    }
  }
  __syncthreads();
  if (tid == 0) {
    for (int s = 0; s < segs.n; ++s) {
      const long a = max(c0, segs.off[s]);
      const long b = min(c1, segs.off[s] + segs.len[s]);
      if (a >= b) continue;
      float r = wred[0][s][0], rw = wred[1][s][0];
      for (int w = 1; w < GN_WAVES; ++w) {
        r += wred[0][s][w];
        rw += wred[1][s][w];
      }
      const long slot = (long)s * GRAD_NORM_MAX_BLOCKS + blockIdx.x;
      __hip_atomic_store(&part[slot], r, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&partw[slot], rw, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
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
    float acc = gn_wave_sum(
        gn_partials(part, segs.off[s], segs.len[s], s, chunk, tid));
    float accw = gn_wave_sum(
        gn_partials(partw, segs.off[s], segs.len[s], s, chunk, tid));
    if (lane == 0) {
      wred[0][s][wave] = acc;
      wred[1][s][wave] = accw;
    }
  }
  __syncthreads();
  if (tid != 0) return;
  // ---- 3. segments in index order: the global norm and the coefficient ----
  float total = 0.f;
  for (int s = 0; s < segs.n; ++s) {
    float r = wred[0][s][0], rw = wred[1][s][0];
    for (int w = 1; w < GN_WAVES; ++w) {
      r += wred[0][s][w];
      rw += wred[1][s][w];
    }
    wred[0][s][0] = grad_scale * sqrtf(r);
    wred[1][s][0] = sqrtf(rw);
    total += r;
  }
  float coef = 1.f;
  if (clip > 0.f) {
    const float norm = grad_scale * sqrtf(total);
    // torch.nn.utils.clip_grad_norm_: clip = +inf gives exactly 1
    coef = fminf(1.f, clip / (norm + 1e-6f));
    clip_stats[0] = norm;
    clip_stats[1] = coef;
    for (int s = 0; s < segs.n; ++s) clip_stats[2 + s] = wred[0][s][0];
    if (coef < 1.f) *clipped_steps += 1;
  }
  // ---- 4. trust ratios -------------------------------------------------------
  for (int s = 0; s < segs.n; ++s) {
    const float gn = coef * wred[0][s][0];
    const float wn = wred[1][s][0];
    const bool ad = (adapt >> s) & 1u;
    float ratio = 1.f;
    if (ad && wn > 0.f && gn > 0.f) ratio = eta * wn / (gn + wd * wn);
    lars_tab[2 * s] = ratio * coef;
    lars_tab[2 * s + 1] = ad ? ratio * wd / grad_scale : 0.f;
    lars_stats[3 * s] = wn;
    lars_stats[3 * s + 1] = gn;
    lars_stats[3 * s + 2] = ratio;
  }
  __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

void lars_norm_plan(long n, int* blocks, int* chain) {
  // grad_norm_kernel's grid; the two sides are independent chains of its
  // length
  grad_norm_plan(n, blocks, chain);
}

void launch_lars_norm(const float* master, const float* grad, long n,
                      GradNormSegs segs, unsigned adapt, float grad_scale,
                      float eta, float wd, float clip, float* lars_tab,
                      float* lars_stats, float* clip_stats,
                      long* clipped_steps, float* part, unsigned* ticket,
                      hipStream_t s) {
  int blocks, chain;
  lars_norm_plan(n, &blocks, &chain);
  hipLaunchKernelGGL(lars_norm_kernel, dim3(blocks), dim3(GN_THREADS), 0, s,
                     master, grad, n, segs, grad_norm_chunk(n), adapt,
                     grad_scale, eta, wd, clip, lars_tab, lars_stats,
                     clip_stats, clipped_steps, part, ticket);
}
