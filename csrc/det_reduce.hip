// Ordered plane reduction of the deterministic mode (docs/KERNELS.md,
// "Deterministic mode").  A gradient kernel launched in that mode does not add
// into the bucket: every block stores its contribution into a plane that only
// it writes.  This kernel then computes, per output element i,
//
//   S[i]   = ((p_0[i] + p_1[i]) + p_2[i]) + ... + p_{P-1}[i]
//   out[i] = out[i] + S[i]
//
// in fp32, planes in index order starting from p_0, one add into out.  One
// thread owns an element (or four), so the order does not depend on how the
// blocks are scheduled.  (store = 1 writes S itself: the first stage of a
// two-stage sum whose second stage adds into the bucket.)  Up to
// PLANE_REDUCE_MAX destinations ride in one
// launch (the transpose_bf16_batch_kernel pattern: block -> descriptor by a
// prefix table).
//
// Addressing: a descriptor is split into head / body / tail.  The body is the
// part that 16 B loads and stores can reach: it exists when out and the plane
// base have the same phase inside a 16 B line and the plane stride is a
// multiple of 4 floats; the head (up to 3 elements before out's first 16 B
// boundary) and the tail go one float per thread.  Anything else (a plane
// stride that is no multiple of 4, mismatched phases) runs all-scalar.
// Loads of PR_AHEAD planes are issued before the adds that consume them.

#include "common.h"
#include "kernels.h"

#define PR_THREADS 64
#define PR_AHEAD 8

template <typename T>
DEV T pr_sum(const float* __restrict__ base, long stride, int P) {
  // p_0 first: S starts from p_0, not from +0 (keeps -0 and the formula exact)
  T s = *reinterpret_cast<const T*>(base);
  int p = 1;
  for (; p + PR_AHEAD <= P; p += PR_AHEAD) {
    T t[PR_AHEAD];
#pragma unroll
    for (int j = 0; j < PR_AHEAD; ++j)
      t[j] = *reinterpret_cast<const T*>(base + (size_t)(p + j) * stride);
#pragma unroll
    for (int j = 0; j < PR_AHEAD; ++j) s = s + t[j];
  }
  for (; p < P; ++p)
    s = s + *reinterpret_cast<const T*>(base + (size_t)p * stride);
  return s;
}

__global__ __launch_bounds__(PR_THREADS)
void plane_reduce_kernel(PlaneReduceArgs a) {
  int d = 0;
#pragma unroll
  for (int i = 1; i < PLANE_REDUCE_MAX; ++i)
    if (i < a.n && (int)blockIdx.x >= a.block0[i]) d = i;
  const PlaneReduceDesc& de = a.d[d];
  const long u = (long)((int)blockIdx.x - a.block0[d]) * PR_THREADS +
                 threadIdx.x;
  const long nvec = de.nvec;
  if (u < nvec) {
    const long i = de.head + 4 * u;
    f32x4 s = pr_sum<f32x4>(de.planes + i, de.stride, de.P);
    f32x4* o = reinterpret_cast<f32x4*>(de.out + i);
    *o = de.store ? s : *o + s;
    return;
  }
  // scalar head [0, head) and tail [head + 4*nvec, n)
  long sidx = u - nvec;
  long i = sidx < de.head ? sidx : de.head + 4 * nvec + (sidx - de.head);
  if (i >= de.n) return;
  float s = pr_sum<float>(de.planes + i, de.stride, de.P);
  de.out[i] = de.store ? s : de.out[i] + s;
}

void launch_plane_reduce(const PlaneReduceDesc* descs, int n, hipStream_t s) {
  PlaneReduceArgs a{};
  int blocks = 0;
  for (int i = 0; i < n && a.n < PLANE_REDUCE_MAX; ++i) {
    PlaneReduceDesc d = descs[i];
    if (d.n <= 0 || d.P <= 0) continue;
    const uintptr_t po = reinterpret_cast<uintptr_t>(d.out) >> 2;
    const uintptr_t pp = reinterpret_cast<uintptr_t>(d.planes) >> 2;
    const bool vec = d.stride % 4 == 0 && ((po ^ pp) & 3) == 0;
    long head = vec ? (long)((4 - (po & 3)) & 3) : d.n;
    if (head > d.n) head = d.n;
    d.head = (int)head;
    d.nvec = (d.n - head) / 4;
    const long units = d.nvec + (d.n - 4 * d.nvec);
    a.d[a.n] = d;
    a.block0[a.n] = blocks;
    blocks += (int)((units + PR_THREADS - 1) / PR_THREADS);
    a.n++;
  }
  if (blocks == 0) return;
  hipLaunchKernelGGL(plane_reduce_kernel, dim3(blocks), dim3(PR_THREADS), 0, s,
                     a);
}
