// Adam / AdamW and LAMB (--optimizer adam|lamb; You et al. 2019) on the flat
// fp32 bucket (docs/KERNELS.md "Adam and LAMB").  With g the aggregated
// bucket, s = grad_scale, coef the clip coefficient and k = offset + 1:
//   gh = (g * s) * coef, then the --drop_connect_post mask (sgd_step's stream)
//   m = b1*m + (1 - b1)*gh          v = b2*v + (1 - b2)*gh*gh
//   c1 = 1 - b1^k, c2 = 1 - b2^k    (-expm1(k * ln b), no cancellation)
//   u = (m / c1) / (sqrt(v / c2) + eps)
//   adam: w -= lr * (u + wd_t*w)
//   lamb: u_t = u + wd_t*w, r_t = |w_t| / |u_t|, w -= (lr * r_t) * u_t
// wd_t = wd on the tensors of `adapt`, 0 elsewhere; r_t = 1 for a tensor that
// is not adaptive or has a zero norm; lr = lr_scale * contrib (contrib = 1/s,
// an exact integer).  After the weight write: the moving average, the bf16
// shadow and the gradient re-zeroing of the SGD pass.
//
// adam_step_kernel: one streaming pass, two 16 B groups of g, w, m, v per
// thread in flight (eight loads, ten with the average).
// LAMB: lamb_moments_kernel updates m and v and reduces sum u_t^2 and sum w^2
// per tensor with grad_norm_kernel's geometry (fixed chunks, the fixed
// shuffle tree, per-(tensor, block) partials, the last block's ordered sum, no
// float atomics); its last block STORES lamb_tab[t] = r_t and lamb_stats[3t..]
// = (|w_t|, |u_t|, r_t).  lamb_apply_kernel recomputes u_t from the m, v, w
// that pass left (adam_u / adam_decayed below, the same code in the same
// build: the same bits) and writes w, the average, the shadow, the zeroed
// gradient.
//
// Every fp32 operation here rounds once, in the order written: contraction is
// off for the whole file, and fp32 '/' and sqrtf are correctly rounded in
// this build.  ops/cpu_ref.py::adam_step does the same operations in the same
// order, so the elementwise results agree bit for bit.
#pragma clang fp contract(off)

#include "grad_norm_common.h"

struct AdamHyper {
  float b1, b2;      // beta1, beta2
  float omb1, omb2;  // 1 - beta, rounded once from double on the host
  float lnb1, lnb2;  // ln beta, rounded once from double on the host
  float eps, wd;
  float s, contrib;  // grad_scale and its exact inverse
  unsigned adapt;    // bit t: tensor t is a weight tensor (decay, trust ratio)
};

// 1 - b^k: the correctly rounded fp32 expm1 of the fp32 product k * ln b
// (through double, so the device and the CPU reference agree on the bits)
DEV float adam_correction(float k, float lnb) {
  return (float)(-expm1((double)(k * lnb)));
}

DEV float adam_keep(uint32_t r, float dc_keep) {
  return (r * (1.0f / 4294967296.0f) < dc_keep) ? 1.f : 0.f;
}

// one element of the moment update: m, v in place, returns u
DEV float adam_moments(float g, float keep, float& m, float& v, float coef,
                       float c1, float c2, const AdamHyper& h) {
  float gh = ((g * h.s) * coef) * keep;
  m = h.b1 * m + h.omb1 * gh;
  v = h.b2 * v + h.omb2 * (gh * gh);
  return (m / c1) / (sqrtf(v / c2) + h.eps);
}

// u from moments that are already updated (the LAMB apply pass)
DEV float adam_u(float m, float v, float c1, float c2, const AdamHyper& h) {
  return (m / c1) / (sqrtf(v / c2) + h.eps);
}

DEV float adam_decayed(float u, float w, float wd_t) { return u + wd_t * w; }

// the last segment that starts at or before idx (the segments tile [0, n))
DEV int adam_seg_of(const GradNormSegs& segs, long idx) {
  int t = 0;
#pragma unroll
  for (int s = 1; s < GRAD_NORM_MAX_SEGS; ++s)
    t += (s < segs.n && idx >= segs.off[s]) ? 1 : 0;
  return t;
}

DEV float adam_ema_weight(float k, float ema_decay) {
  return 1.f - fminf(ema_decay, (1.f + k) / (10.f + k));
}

// what follows the weight write, one element
template <bool EMA>
DEV void adam_publish(long j, float w, float* ema, float ema_w,
                      ushort_t* shadow, float* grad, int zero_grad) {
  if (EMA) {
    float e = ema[j];
    ema[j] = e - ema_w * (e - w);
  }
  if (zero_grad) grad[j] = 0.f;
  if (shadow) shadow[j] = f2bf(w);
}

template <bool EMA>
DEV void adam_publish4(long base, float4 w, float* ema, float ema_w,
                       ushort_t* shadow, float* grad, int zero_grad) {
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
}

// ---------------------------------------------------------------------------
// Adam / AdamW
// ---------------------------------------------------------------------------
#define ADAM_UNROLL 2  // 16 B groups of each stream in flight per thread

template <bool EMA, bool CLIP>
__global__ __launch_bounds__(256)
void adam_step_kernel(float* master, float* grad, float* am, float* av,
                      ushort_t* shadow, long n, AdamHyper h, GradNormSegs segs,
                      float lr_scale, uint64_t offset,
                      const float* lr_scale_dev, const long* offset_dev,
                      float dc_keep, uint64_t seed, int zero_grad, float* ema,
                      float ema_decay, const float* clip_coef_dev) {
  // resolved once per thread
  if (lr_scale_dev) lr_scale = *lr_scale_dev;
  if (offset_dev) offset = (uint64_t)*offset_dev;
  const float coef = CLIP ? *clip_coef_dev : 1.f;
  const float k = (float)(offset + 1);
  const float c1 = adam_correction(k, h.lnb1);
  const float c2 = adam_correction(k, h.lnb2);
  const float lr = lr_scale * h.contrib;
  const float ema_w = EMA ? adam_ema_weight(k, ema_decay) : 0.f;
  const long stride = (long)gridDim.x * blockDim.x;
  const long groups = (n + 3) >> 2;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < groups;
       i += ADAM_UNROLL * stride) {
    float4 g[ADAM_UNROLL], w[ADAM_UNROLL], m[ADAM_UNROLL], v[ADAM_UNROLL];
    int seg[ADAM_UNROLL];
    bool vec[ADAM_UNROLL];
    // every load of the trip is issued before the first use
#pragma unroll
    for (int j = 0; j < ADAM_UNROLL; ++j) {
      const long base = (i + j * stride) * 4;
      seg[j] = adam_seg_of(segs, base);
      // a whole group inside one tensor takes the vector path
      vec[j] = base + 3 < n && seg[j] == adam_seg_of(segs, base + 3);
      if (vec[j]) {
        g[j] = *reinterpret_cast<const float4*>(grad + base);
        w[j] = *reinterpret_cast<const float4*>(master + base);
        m[j] = *reinterpret_cast<const float4*>(am + base);
        v[j] = *reinterpret_cast<const float4*>(av + base);
      }
    }
#pragma unroll
    for (int j = 0; j < ADAM_UNROLL; ++j) {
      const long gi = i + j * stride;
      const long base = gi * 4;
      if (base >= n) break;
      float kp[4] = {1.f, 1.f, 1.f, 1.f};
      if (dc_keep > 0.f) {
        Philox4 ph = philox4x32(seed, offset, (uint64_t)gi);
        kp[0] = adam_keep(ph.x, dc_keep); kp[1] = adam_keep(ph.y, dc_keep);
        kp[2] = adam_keep(ph.z, dc_keep); kp[3] = adam_keep(ph.w, dc_keep);
      }
      if (vec[j]) {
        const float wd_t = ((h.adapt >> seg[j]) & 1u) ? h.wd : 0.f;
        float4 u;
        u.x = adam_moments(g[j].x, kp[0], m[j].x, v[j].x, coef, c1, c2, h);
        u.y = adam_moments(g[j].y, kp[1], m[j].y, v[j].y, coef, c1, c2, h);
        u.z = adam_moments(g[j].z, kp[2], m[j].z, v[j].z, coef, c1, c2, h);
        u.w = adam_moments(g[j].w, kp[3], m[j].w, v[j].w, coef, c1, c2, h);
        *reinterpret_cast<float4*>(am + base) = m[j];
        *reinterpret_cast<float4*>(av + base) = v[j];
        float4 x = w[j];
        x.x = x.x - lr * adam_decayed(u.x, x.x, wd_t);
        x.y = x.y - lr * adam_decayed(u.y, x.y, wd_t);
        x.z = x.z - lr * adam_decayed(u.z, x.z, wd_t);
        x.w = x.w - lr * adam_decayed(u.w, x.w, wd_t);
        *reinterpret_cast<float4*>(master + base) = x;
        adam_publish4<EMA>(base, x, ema, ema_w, shadow, grad, zero_grad);
      } else {
        // the scalar tail, and a group that straddles a tensor boundary
        const long jend = min(n, base + 4);
        for (long e = base; e < jend; ++e) {
          const int se = adam_seg_of(segs, e);
          const float wd_t = ((h.adapt >> se) & 1u) ? h.wd : 0.f;
          float me = am[e], ve = av[e], x = master[e];
          const float u = adam_moments(grad[e], kp[e - base], me, ve, coef,
                                       c1, c2, h);
          am[e] = me;
          av[e] = ve;
          x = x - lr * adam_decayed(u, x, wd_t);
          master[e] = x;
          adam_publish<EMA>(e, x, ema, ema_w, shadow, grad, zero_grad);
        }
      }
    }
  }
}

static int adam_blocks(long n, int unroll) {
  const long groups = (n + 3) / 4;
  const long per = 256L * unroll;
  long blocks = (groups + per - 1) / per;
  if (blocks > 2048) blocks = 2048;
  return blocks < 1 ? 1 : (int)blocks;
}

static AdamHyper adam_hyper(const AdamArgs& a) {
  AdamHyper h;
  h.b1 = (float)a.beta1;
  h.b2 = (float)a.beta2;
  h.omb1 = (float)(1.0 - a.beta1);
  h.omb2 = (float)(1.0 - a.beta2);
  h.lnb1 = a.lnb1;
  h.lnb2 = a.lnb2;
  h.eps = (float)a.eps;
  h.wd = (float)a.wd;
  h.s = a.grad_scale;
  h.contrib = rintf(1.f / a.grad_scale);
  h.adapt = a.adapt;
  return h;
}

void launch_adam_step(float* master, float* grad, float* am, float* av,
                      unsigned short* shadow, long n, const AdamArgs& a,
                      const GradNormSegs& segs, float lr_scale,
                      uint64_t offset, const float* lr_scale_dev,
                      const long* offset_dev, int zero_grad, float* ema,
                      float ema_decay, const float* clip_coef_dev,
                      hipStream_t s) {
  const AdamHyper h = adam_hyper(a);
  const dim3 grid(adam_blocks(n, ADAM_UNROLL)), block(256);
#define ADAM_LAUNCH(E, C)                                                     \
  hipLaunchKernelGGL((adam_step_kernel<E, C>), grid, block, 0, s, master,     \
                     grad, am, av, shadow, n, h, segs, lr_scale, offset,      \
                     lr_scale_dev, offset_dev, a.dc_keep, a.seed, zero_grad,  \
                     ema, ema_decay, clip_coef_dev)
  if (ema && clip_coef_dev) ADAM_LAUNCH(true, true);
  else if (ema) ADAM_LAUNCH(true, false);
  else if (clip_coef_dev) ADAM_LAUNCH(false, true);
  else ADAM_LAUNCH(false, false);
#undef ADAM_LAUNCH
}

// ---------------------------------------------------------------------------
// LAMB pass 1: moments in place + per-tensor sum u_t^2 and sum w^2
// ---------------------------------------------------------------------------
DEV float lamb_sq4(float4 x) {
  return (x.x * x.x + x.y * x.y) + (x.z * x.z + x.w * x.w);
}

extern "C" __global__ __launch_bounds__(GN_THREADS)
void lamb_moments_kernel(const float* master, const float* grad, float* am,
                         float* av, long n, GradNormSegs segs, long chunk,
                         AdamHyper h, uint64_t offset, const long* offset_dev,
                         float dc_keep, uint64_t seed,
                         const float* clip_coef_dev, float* lamb_tab,
                         float* lamb_stats, float* part, unsigned* ticket) {
  // [0]: u_t, [1]: master
  __shared__ float wred[2][GRAD_NORM_MAX_SEGS][GN_WAVES];
  __shared__ int is_last;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const long c0 = (long)blockIdx.x * chunk;
  const long cend = min(n, c0 + chunk);
  float* const partw = part + GRAD_NORM_MAX_SEGS * GRAD_NORM_MAX_BLOCKS;
  if (offset_dev) offset = (uint64_t)*offset_dev;
  const float coef = clip_coef_dev ? *clip_coef_dev : 1.f;
  const float k = (float)(offset + 1);
  const float c1 = adam_correction(k, h.lnb1);
  const float c2 = adam_correction(k, h.lnb2);

  // ---- 1. this block's chunk, one segment at a time (block-uniform loop) --
  for (int s = 0; s < segs.n; ++s) {
    const long a = max(c0, segs.off[s]);
    const long b = min(cend, segs.off[s] + segs.len[s]);
    if (a >= b) continue;
    const float wd_t = ((h.adapt >> s) & 1u) ? h.wd : 0.f;
    float acc = 0.f, accw = 0.f;
    // [a, a4): scalar head, [a4, b4): 16 B groups, [b4, b): scalar tail
    const long a4 = min(b, (a + 3) & ~3L);
    const long b4 = max(a4, b & ~3L);
    const long g1 = b4 >> 2;
    // four 16 B groups of each of g, w, m, v in flight per trip
    for (long g = (a4 >> 2) + tid; g < g1; g += 4 * GN_THREADS) {
      float4 gg[4], ww[4], mm[4], vv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long gj = g + j * GN_THREADS;
        if (gj < g1) {
          gg[j] = *reinterpret_cast<const float4*>(grad + gj * 4);
          ww[j] = *reinterpret_cast<const float4*>(master + gj * 4);
          mm[j] = *reinterpret_cast<const float4*>(am + gj * 4);
          vv[j] = *reinterpret_cast<const float4*>(av + gj * 4);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long gj = g + j * GN_THREADS;
        if (gj >= g1) break;
        float kp[4] = {1.f, 1.f, 1.f, 1.f};
        if (dc_keep > 0.f) {
          Philox4 ph = philox4x32(seed, offset, (uint64_t)gj);
          kp[0] = adam_keep(ph.x, dc_keep); kp[1] = adam_keep(ph.y, dc_keep);
          kp[2] = adam_keep(ph.z, dc_keep); kp[3] = adam_keep(ph.w, dc_keep);
        }
        float4 u;
        u.x = adam_decayed(adam_moments(gg[j].x, kp[0], mm[j].x, vv[j].x,
                                        coef, c1, c2, h), ww[j].x, wd_t);
        u.y = adam_decayed(adam_moments(gg[j].y, kp[1], mm[j].y, vv[j].y,
                                        coef, c1, c2, h), ww[j].y, wd_t);
        u.z = adam_decayed(adam_moments(gg[j].z, kp[2], mm[j].z, vv[j].z,
                                        coef, c1, c2, h), ww[j].z, wd_t);
        u.w = adam_decayed(adam_moments(gg[j].w, kp[3], mm[j].w, vv[j].w,
                                        coef, c1, c2, h), ww[j].w, wd_t);
        *reinterpret_cast<float4*>(am + gj * 4) = mm[j];
        *reinterpret_cast<float4*>(av + gj * 4) = vv[j];
        acc += lamb_sq4(u);
        accw += lamb_sq4(ww[j]);
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
          kp = adam_keep(c == 0 ? ph.x : c == 1 ? ph.y : c == 2 ? ph.z : ph.w,
                         dc_keep);
        }
        float me = am[e], ve = av[e];
        const float x = master[e];
        const float u = adam_decayed(
            adam_moments(grad[e], kp, me, ve, coef, c1, c2, h), x, wd_t);
        am[e] = me;
        av[e] = ve;
        acc += u * u;
        accw += x * x;
      }
    }
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
      const long b = min(cend, segs.off[s] + segs.len[s]);
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
  // ---- 3. trust ratios, segments in index order ------------------------------
  for (int s = 0; s < segs.n; ++s) {
    float r = wred[0][s][0], rw = wred[1][s][0];
    for (int w = 1; w < GN_WAVES; ++w) {
      r += wred[0][s][w];
      rw += wred[1][s][w];
    }
    const float un = sqrtf(r), wn = sqrtf(rw);
    float ratio = 1.f;
    if (((h.adapt >> s) & 1u) && wn > 0.f && un > 0.f) ratio = wn / un;
    lamb_tab[s] = ratio;
    lamb_stats[3 * s] = wn;
    lamb_stats[3 * s + 1] = un;
    lamb_stats[3 * s + 2] = ratio;
  }
  __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

void lamb_norm_plan(long n, int* blocks, int* chain) {
  // grad_norm_kernel's grid; the two sums are independent chains of its
  // length
  grad_norm_plan(n, blocks, chain);
}

void launch_lamb_moments(const float* master, const float* grad, float* am,
                         float* av, long n, const AdamArgs& a,
                         const GradNormSegs& segs, uint64_t offset,
                         const long* offset_dev, const float* clip_coef_dev,
                         float* lamb_tab, float* lamb_stats, float* part,
                         unsigned* ticket, hipStream_t s) {
  int blocks, chain;
  lamb_norm_plan(n, &blocks, &chain);
  hipLaunchKernelGGL(lamb_moments_kernel, dim3(blocks), dim3(GN_THREADS), 0,
                     s, master, grad, am, av, n, segs, grad_norm_chunk(n),
                     adam_hyper(a), offset, offset_dev, a.dc_keep, a.seed,
                     clip_coef_dev, lamb_tab, lamb_stats, part, ticket);
}

// ---------------------------------------------------------------------------
// LAMB pass 2: w -= (lr * r_t) * u_t, u_t recomputed from pass 1's m, v and w
// ---------------------------------------------------------------------------
template <bool EMA>
__global__ __launch_bounds__(256)
void lamb_apply_kernel(float* master, float* grad, const float* am,
                       const float* av, ushort_t* shadow, long n, AdamHyper h,
                       GradNormSegs segs, float lr_scale, uint64_t offset,
                       const float* lr_scale_dev, const long* offset_dev,
                       int zero_grad, float* ema, float ema_decay,
                       const float* lamb_tab) {
  // per tensor: lr * r_t and wd_t, resolved once per block
  __shared__ float lr_t[GRAD_NORM_MAX_SEGS], wd_t[GRAD_NORM_MAX_SEGS];
  if (lr_scale_dev) lr_scale = *lr_scale_dev;
  if (offset_dev) offset = (uint64_t)*offset_dev;
  const float lr = lr_scale * h.contrib;
  if (threadIdx.x < GRAD_NORM_MAX_SEGS) {
    const bool live = (int)threadIdx.x < segs.n;
    lr_t[threadIdx.x] = live ? lr * lamb_tab[threadIdx.x] : 0.f;
    wd_t[threadIdx.x] = (live && ((h.adapt >> threadIdx.x) & 1u)) ? h.wd : 0.f;
  }
  __syncthreads();
  const float k = (float)(offset + 1);
  const float c1 = adam_correction(k, h.lnb1);
  const float c2 = adam_correction(k, h.lnb2);
  const float ema_w = EMA ? adam_ema_weight(k, ema_decay) : 0.f;
  const long stride = (long)gridDim.x * blockDim.x;
  const long groups = (n + 3) >> 2;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < groups;
       i += ADAM_UNROLL * stride) {
    float4 w[ADAM_UNROLL], m[ADAM_UNROLL], v[ADAM_UNROLL];
    int seg[ADAM_UNROLL];
    bool vec[ADAM_UNROLL];
#pragma unroll
    for (int j = 0; j < ADAM_UNROLL; ++j) {
      const long base = (i + j * stride) * 4;
      seg[j] = adam_seg_of(segs, base);
      vec[j] = base + 3 < n && seg[j] == adam_seg_of(segs, base + 3);
      if (vec[j]) {
        w[j] = *reinterpret_cast<const float4*>(master + base);
        m[j] = *reinterpret_cast<const float4*>(am + base);
        v[j] = *reinterpret_cast<const float4*>(av + base);
      }
    }
#pragma unroll
    for (int j = 0; j < ADAM_UNROLL; ++j) {
      const long base = (i + j * stride) * 4;
      if (base >= n) break;
      if (vec[j]) {
        const float l = lr_t[seg[j]], d = wd_t[seg[j]];
        float4 x = w[j];
        x.x = x.x - l * adam_decayed(adam_u(m[j].x, v[j].x, c1, c2, h), x.x, d);
        x.y = x.y - l * adam_decayed(adam_u(m[j].y, v[j].y, c1, c2, h), x.y, d);
        x.z = x.z - l * adam_decayed(adam_u(m[j].z, v[j].z, c1, c2, h), x.z, d);
        x.w = x.w - l * adam_decayed(adam_u(m[j].w, v[j].w, c1, c2, h), x.w, d);
        *reinterpret_cast<float4*>(master + base) = x;
        adam_publish4<EMA>(base, x, ema, ema_w, shadow, grad, zero_grad);
      } else {
        const long jend = min(n, base + 4);
        for (long e = base; e < jend; ++e) {
          const int se = adam_seg_of(segs, e);
          float x = master[e];
          x = x - lr_t[se] * adam_decayed(adam_u(am[e], av[e], c1, c2, h), x,
                                          wd_t[se]);
          master[e] = x;
          adam_publish<EMA>(e, x, ema, ema_w, shadow, grad, zero_grad);
        }
      }
    }
  }
}

void launch_lamb_apply(float* master, float* grad, const float* am,
                       const float* av, unsigned short* shadow, long n,
                       const AdamArgs& a, const GradNormSegs& segs,
                       float lr_scale, uint64_t offset,
                       const float* lr_scale_dev, const long* offset_dev,
                       int zero_grad, float* ema, float ema_decay,
                       const float* lamb_tab, hipStream_t s) {
  const AdamHyper h = adam_hyper(a);
  const dim3 grid(adam_blocks(n, ADAM_UNROLL)), block(256);
  if (ema)
    hipLaunchKernelGGL((lamb_apply_kernel<true>), grid, block, 0, s, master,
                       grad, am, av, shadow, n, h, segs, lr_scale, offset,
                       lr_scale_dev, offset_dev, zero_grad, ema, ema_decay,
                       lamb_tab);
  else
    hipLaunchKernelGGL((lamb_apply_kernel<false>), grid, block, 0, s, master,
                       grad, am, av, shadow, n, h, segs, lr_scale, offset,
                       lr_scale_dev, offset_dev, zero_grad, ema, ema_decay,
                       lamb_tab);
}
