// The per-chunk reduction of grad_norm_kernel and lars_norm_kernel, included
// as TEXT into both (as an inlined function the compiler orders the operands
// of three commutative adds differently, and grad_norm_kernel's ISA is kept
// as it was).  Expects in scope: grad, a < b (the intersection of one segment
// with the block's chunk), tid, and `float acc = 0.f`; adds this thread's
// share of sum g^2 over [a, b) to acc: its 16 B groups in address order, then
// a scalar head / tail element where the range starts or ends off a 16 B
// boundary.  With GN_RANGE_TWO defined to 1 also: master and `float accw =
// 0.f`, reduced over the same range with the same schedule, the four groups
// of both arrays issued before the first use (eight 16 B loads in flight).
// GN_RANGE_SQ4(float4): the includer's sum of the four squares.
{
  // [a, a4): scalar head, [a4, b4): 16 B groups, [b4, b): scalar tail
  long a4 = min(b, (a + 3) & ~3L);
  long b4 = max(a4, b & ~3L);
  const long g1 = b4 >> 2;
  // four 16 B loads per thread in flight per trip: a group past the end
  // re-reads the range's last group (an address inside it, so the loads
  // need no branch) and counts as zero
  for (long g = (a4 >> 2) + tid; g < g1; g += 4 * GN_THREADS) {
    float4 v[4];
#if GN_RANGE_TWO
    float4 w[4];
#endif
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      long gj = min(g + j * GN_THREADS, g1 - 1);
      v[j] = *reinterpret_cast<const float4*>(grad + gj * 4);
#if GN_RANGE_TWO
      w[j] = *reinterpret_cast<const float4*>(master + gj * 4);
#endif
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      acc += g + j * GN_THREADS < g1 ? GN_RANGE_SQ4(v[j]) : 0.f;
#if GN_RANGE_TWO
#pragma unroll
    for (int j = 0; j < 4; ++j)
      accw += g + j * GN_THREADS < g1 ? GN_RANGE_SQ4(w[j]) : 0.f;
#endif
  }
  if (a + tid < a4) { float x = grad[a + tid]; acc += x * x; }
  if (b4 + tid < b) { float x = grad[b4 + tid]; acc += x * x; }
#if GN_RANGE_TWO
  if (a + tid < a4) { float x = master[a + tid]; accw += x * x; }
  if (b4 + tid < b) { float x = master[b4 + tid]; accw += x * x; }
#endif
}
