// Device-side evaluation: sequential chunks of the resident uint8 set and
// evaluation statistics accumulated across launches.
//
// range_gather_kernel — chunk [start, start + B) of the resident set, tail
// included:
//   i = start + j <  N : x[j] = lut[img_u8[i]]  (bf16 [B,28,28,1]), y[j] = lab_u8[i]
//   i = start + j >= N : x[j] = +0.0 (all 784),                    y[j] = -1
// `start` comes from the host or from `start_dev` (device int64), the
// hipGraph-capturable form.  Row I/O is batch_gather_kernel's (8-byte load,
// 256-entry LUT in LDS, 16-byte store), so a live row is bit-identical to
// the training gather's row of the same image.
//
// softmax_eval_kernel — per launch, over the rows with 0 <= label < C:
//   loss_sum[0]              += sum -log softmax(logits)[label]
//   counts[0], counts[1]     += live rows, correct rows
//   counts[2 + t*C + p]      += rows of true class t predicted p
//   pred[b] (optional)        = predicted class, 255 for a row that is not live
//   cursor_dev[0] (optional) += B
// The prediction is the LOWEST index among the maximal logits
// (ops/cpu_ref.py::softmax_eval implements the same rule).  Any other label
// contributes to nothing, so a bad label cannot index outside `counts`.
//
// Loss path: no float atomics.  Shuffle tree per wave, wave partials summed
// by thread 0, block partials parked in `part`; the last block to take a
// ticket sums them in block order and that one thread adds the launch total
// to loss_sum and advances cursor_dev.  Launches on one stream are ordered,
// so the running sum is the same bits on every repetition.
// Count path: LDS integer atomics, then one global integer atomic per
// non-zero cell per block (integer sums do not depend on arrival order).
//
// Workspace: the kernel has its OWN partial/ticket workspace (one per
// device, csrc/bindings.cpp::softmax_eval), not the training softmax's.
// Eval launches sit on the training stream between steps and inside a
// different hipGraph; a private 16 KB buffer makes "can an eval launch and
// a training softmax ever be in flight together" a question that does not
// need answering.  Eval launches themselves never overlap: one evaluator,
// one stream.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int GATHER_THREADS = 256;
constexpr int GATHER_IPB = 2;             // as batch_gather_kernel
constexpr int ROW_BYTES = 784;            // 28*28 uint8 = 49 x 16 B
constexpr int ROW_UNITS = ROW_BYTES / 8;  // 98 units of 8 px per image
constexpr int EVAL_THREADS = 256;
constexpr int EVAL_MAX_C = 16;
constexpr int EVAL_CELLS = 2 + EVAL_MAX_C * EVAL_MAX_C;

}  // namespace

extern "C" __global__ __launch_bounds__(GATHER_THREADS)
void range_gather_kernel(const uint8_t* __restrict__ img,
                         const uint8_t* __restrict__ lab,
                         const unsigned short* __restrict__ lut,
                         unsigned short* __restrict__ x, long* __restrict__ y,
                         uint32_t N, uint32_t B, uint64_t start,
                         const long* __restrict__ start_dev) {
  __shared__ unsigned short s_lut[256];
  const int tid = threadIdx.x;
  const uint32_t j0 = blockIdx.x * GATHER_IPB;
  // a negative device cursor wraps to a huge value: every row is padding
  if (start_dev) start = (uint64_t)*start_dev;

  s_lut[tid] = lut[tid];  // GATHER_THREADS == 256 entries
  if (tid < GATHER_IPB && j0 + tid < B) {
    const uint64_t i = start + j0 + tid;
    y[j0 + tid] = i < N ? (long)lab[i] : -1L;
  }
  __syncthreads();

  for (int u = tid; u < GATHER_IPB * ROW_UNITS; u += GATHER_THREADS) {
    const int im = u / ROW_UNITS;
    const int unit = u - im * ROW_UNITS;
    const uint32_t j = j0 + im;
    if (j >= B) break;  // last partial block (u is monotonic in im)
    const uint64_t i = start + j;
    uint4 o = make_uint4(0u, 0u, 0u, 0u);  // padding row: +0.0 bf16
    if (i < N) {
      const uint8_t* src = img + (size_t)i * ROW_BYTES + unit * 8;
      const uint2 px = *reinterpret_cast<const uint2*>(src);
      o.x = s_lut[px.x & 0xFF] | ((uint32_t)s_lut[(px.x >> 8) & 0xFF] << 16);
      o.y = s_lut[(px.x >> 16) & 0xFF] | ((uint32_t)s_lut[px.x >> 24] << 16);
      o.z = s_lut[px.y & 0xFF] | ((uint32_t)s_lut[(px.y >> 8) & 0xFF] << 16);
      o.w = s_lut[(px.y >> 16) & 0xFF] | ((uint32_t)s_lut[px.y >> 24] << 16);
    }
    *reinterpret_cast<uint4*>(x + (size_t)j * ROW_BYTES + unit * 8) = o;
  }
}

void launch_range_gather(const uint8_t* img, const uint8_t* lab,
                         const unsigned short* lut, unsigned short* x,
                         long* y, uint32_t N, uint32_t B, uint64_t start,
                         const long* start_dev, hipStream_t s) {
  const int blocks = (int)((B + GATHER_IPB - 1) / GATHER_IPB);
  hipLaunchKernelGGL(range_gather_kernel, dim3(blocks), dim3(GATHER_THREADS),
                     0, s, img, lab, lut, x, y, N, B, start, start_dev);
}

// One thread per row.  CC > 0: compile-time class count.  CC == 0: runtime
// C <= 16 — the per-class loops still unroll to 16 with the tail PREDICATED
// (never an early break, never a runtime index), so v[] stays in registers
// in both forms (the scratch trap softmax_xent_t_kernel's header records).
template <int CC>
__global__ __launch_bounds__(EVAL_THREADS)
void softmax_eval_kernel(const ushort_t* __restrict__ logits,
                         const long* __restrict__ labels, float* loss_sum,
                         int* counts, uint8_t* __restrict__ pred,
                         long* cursor_dev, int B, int C, float* part,
                         unsigned* ticket) {
  constexpr int CM = CC ? CC : EVAL_MAX_C;
  if (CC) C = CC;
  __shared__ float wred[EVAL_THREADS / 64];
  __shared__ int s_cnt[EVAL_CELLS];
  const int tid = threadIdx.x;
  const int cells = 2 + C * C;
  for (int i = tid; i < cells; i += EVAL_THREADS) s_cnt[i] = 0;
  __syncthreads();

  const int b = blockIdx.x * EVAL_THREADS + tid;
  const bool inb = b < B;
  const long lab = inb ? labels[b] : -1L;
  const bool live = lab >= 0 && lab < (long)C;  // label -1 marks padding
  float loss = 0.f;
  int arg = 0;
  if (inb) {
    float v[CM];
    if (CC == 10) {
      // one 16B + one 4B load per row (20B, always 4B-aligned)
      ushort_t row[10];
      __builtin_memcpy(&row[0], logits + (size_t)b * 10, 16);
      __builtin_memcpy(&row[8], logits + (size_t)b * 10 + 8, 4);
#pragma unroll
      for (int c = 0; c < 10; ++c) v[c] = bf2f(row[c]);
    } else {
#pragma unroll
      for (int c = 0; c < CM; ++c)
        v[c] = (CC || c < C) ? bf2f(logits[(size_t)b * C + c]) : -INFINITY;
    }
    float mx = v[0];
    float xl = v[0];  // the label's logit, picked by compares (no v[lab])
#pragma unroll
    for (int c = 1; c < CM; ++c) {
      if (v[c] > mx) { mx = v[c]; arg = c; }  // strict: lowest index wins
      if (c == (int)lab) xl = v[c];
    }
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c) se += __expf(v[c] - mx);  // pad: exp(-inf)=0
    if (live) loss = __logf(se) - (xl - mx);
    if (pred) pred[b] = live ? (uint8_t)arg : (uint8_t)255;
  }

  if (live) atomicAdd(&s_cnt[2 + (int)lab * C + arg], 1);
  {
    // live / correct rows: one LDS atomic per wave from the lane masks
    const unsigned long long ml = __ballot(live);
    const unsigned long long mc = __ballot(live && arg == (int)lab);
    if ((tid & 63) == 0) {
      if (ml) atomicAdd(&s_cnt[0], __popcll(ml));
      if (mc) atomicAdd(&s_cnt[1], __popcll(mc));
    }
    float ls = loss;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ls += __shfl_down(ls, off, 64);
    if ((tid & 63) == 0) wred[tid >> 6] = ls;
  }
  __syncthreads();
  for (int i = tid; i < cells; i += EVAL_THREADS) {
    const int n = s_cnt[i];
    if (n) atomicAdd(&counts[i], n);
  }
  if (tid == 0) {
    const unsigned nblk = gridDim.x;
    float r0 = 0.f;
#pragma unroll
    for (int wv = 0; wv < EVAL_THREADS / 64; ++wv) r0 += wred[wv];
    bool last = nblk == 1;
    if (!last) {
      __hip_atomic_store(&part[blockIdx.x], r0, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
      __threadfence();  // partial visible device-wide before the ticket
      if (atomicAdd(ticket, 1u) == nblk - 1) {
        __threadfence();
        r0 = 0.f;
        for (unsigned i = 0; i < nblk; ++i)
          r0 += __hip_atomic_load(&part[i], __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        last = true;
      }
    }
    if (last) {
      // the only writer of both words in this launch; earlier launches are
      // ordered before it by the stream
      loss_sum[0] += r0;
      if (cursor_dev) cursor_dev[0] += (long)B;
    }
  }
}

void launch_softmax_eval(const unsigned short* logits, const long* labels,
                         float* loss_sum, int* counts, uint8_t* pred,
                         long* cursor_dev, int B, int C, float* part,
                         unsigned* ticket, hipStream_t s) {
  dim3 grid((B + EVAL_THREADS - 1) / EVAL_THREADS);
  if (C == 10) {
    hipLaunchKernelGGL((softmax_eval_kernel<10>), grid, dim3(EVAL_THREADS), 0,
                       s, logits, labels, loss_sum, counts, pred, cursor_dev,
                       B, C, part, ticket);
  } else {
    hipLaunchKernelGGL((softmax_eval_kernel<0>), grid, dim3(EVAL_THREADS), 0,
                       s, logits, labels, loss_sum, counts, pred, cursor_dev,
                       B, C, part, ticket);
  }
}
