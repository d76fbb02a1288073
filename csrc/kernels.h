// Host-visible API of the HIP kernel library (implemented in *.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct GemmParams {
  const unsigned short* A;
  const unsigned short* B;
  const float* bias;
  void* C;
  uint8_t* amax;
  int M, N, K;
  int lda, ldb, ldc;
  int splitk;
  int CB, CH, CW, CHo, CWo, Cin, Cout;
  float p_keep;
  uint64_t seed, offset;
  const long* offset_dev;  // when set, RNG offset is read from device memory
                           // (hipGraph replay: host args are frozen)
  float* db;  // EPI_UNPOOL / EPI_MASK_DB: bias-grad accumulator
  const unsigned short* actm;  // EPI_MASK_DB: saved activation (mask source)
  int unpool_lines;   // EPI_UNPOOL: stage the tile in LDS, store 128 B lines
                      // EPI_POOLMASK_DB: the same, whole 16 B row chunks
  unsigned* tickets;  // OUT_F32_SLICES_FIX: per-tile counters; the last slice
                      // of a tile sums the planes and writes bf16 y (p.Y)
  unsigned short* Y;  // OUT_F32_SLICES_FIX: final bf16 output [M][N]
  int relu;           // OUT_F32_SLICES_FIX: relu in the fix-up
  // deterministic mode (det_reduce.hip): the *_det entries store the block's
  // contribution into its private plane instead of adding into C / db.
  // dw_tr: plane = k-slice, [M][ldc] floats at det_planes + slice*det_stride.
  // GEMM bias tails: plane = block row, [N] floats at det_planes +
  // blockIdx.x * det_stride.
  float* det_planes;
  long det_stride;
};

// gemm_tile.hip — implicit-GEMM MFMA entry points
void gemm_fwd_bias_128(const GemmParams&, hipStream_t);
void gemm_fwd_bias_64(const GemmParams&, hipStream_t);
void gemm_fwd_relu_128(const GemmParams&, hipStream_t);
void gemm_fwd_relu_64(const GemmParams&, hipStream_t);
void gemm_fwd_drop_128(const GemmParams&, hipStream_t);
void gemm_fwd_drop_64(const GemmParams&, hipStream_t);
void gemm_dx_128(const GemmParams&, hipStream_t);
void gemm_dx_64(const GemmParams&, hipStream_t);
void gemm_dx_unpool_128(const GemmParams&, hipStream_t);
void gemm_dx_unpool_64(const GemmParams&, hipStream_t);
void gemm_dx_poolmask_128(const GemmParams&, hipStream_t);
void gemm_dx_poolmask_64(const GemmParams&, hipStream_t);
void gemm_dx_mask_128(const GemmParams&, hipStream_t);
void gemm_dx_mask_64(const GemmParams&, hipStream_t);
void gemm_dw_128(const GemmParams&, hipStream_t);
void gemm_dw_64(const GemmParams&, hipStream_t);
void conv_fwd_pool(const GemmParams&, hipStream_t);
void conv1_fwd_pool(const GemmParams&, hipStream_t);
void conv_dx_gemm(const GemmParams&, hipStream_t);
void conv_dw_gemm(const GemmParams&, hipStream_t);
// dw_tr.hip — glds + ds_read_b64_tr_b16 k-major dW GEMMs (no staging scatter)
void conv_dw_tr(const GemmParams&, hipStream_t);    // 5x5-SAME gather A
// plain k-major A; tbm, bn in {64, 128}.  single_writer (splitk == 1, C and
// ldc 16-byte aligned): each output element is read-added-written once by
// one lane, no atomics
void gemm_dw_tr(const GemmParams&, int tbm, int bn, bool single_writer,
                hipStream_t);
// the same split over k-slices, each slice storing its own plane
// (p.det_planes / p.det_stride); p.C is not touched
void gemm_dw_tr_det(const GemmParams&, int tbm, int bn, hipStream_t);

// ops_misc.hip — host wrappers
void launch_relu_drop_bwd(const unsigned short* dy, const unsigned short* y,
                          unsigned short* dyeff, float* db, int B, int N,
                          float inv_keep, int apply_mask, hipStream_t);
void launch_pool_bwd_scatter(const unsigned short* dy, const unsigned short* y,
                             const uint8_t* amax, unsigned short* dact,
                             float* db, int Mpool, int C, int H, int W, int Wo,
                             hipStream_t);
// out[2] is stored (no pre-zeroing); part/ticket: persistent workspace of
// 2*SOFTMAX_MAX_BLOCKS floats + one zero-initialised, self-resetting counter
#define SOFTMAX_MAX_BLOCKS 4096
void launch_softmax_xent(const unsigned short* logits, const long* labels,
                         unsigned short* dlogits, float* out, int B, int C,
                         float* db, float inv_n, float* part,
                         unsigned* ticket, hipStream_t);
int softmax_xent_blocks(int B);  // grid of the launch above
// deterministic form: `dbplanes` [softmax_xent_blocks(B)][C] receives every
// block's column sums by plain stores (fixed in-block order); db is not
// touched
void launch_softmax_xent_det(const unsigned short* logits, const long* labels,
                             unsigned short* dlogits, float* out, int B, int C,
                             float* dbplanes, float inv_n, float* part,
                             unsigned* ticket, hipStream_t);
// fc2_head.hip — fc2 forward + softmax-xent + fc2 dX/mask/db1 + fc2 dW in one
// launch for the LeNet shape (K == FC2_HEAD_K features, 10 classes); R in
// {16, 32, 64} rows per block.  a1, w2T and dyeff must be 16 B aligned.  out
// and part/ticket as launch_softmax_xent (the same workspace: the grid,
// fc2_head_blocks(B, R), must not exceed SOFTMAX_MAX_BLOCKS); dw2 [K][10],
// db2 [10] and db1 [K] are accumulated into; inv_keep = 1 / p_keep.
#define FC2_HEAD_K 512
int fc2_head_blocks(int B, int R);
void launch_fc2_head(int R, const unsigned short* a1,
                     const unsigned short* w2T, const float* b2,
                     const long* labels, unsigned short* dyeff, float* dw2,
                     float* db2, float* db1, float* out, int B,
                     float inv_keep, float inv_n, float* part,
                     unsigned* ticket, hipStream_t);
void launch_sgd_step(float* master, float* grad, unsigned short* shadow,
                     int has_shadow, long n, float lr_scale, float dc_keep,
                     uint64_t seed, uint64_t offset, float* momentum, float mu,
                     float* ema, float ema_decay, const float* clip_coef_dev,
                     hipStream_t);
// graph-capturable variants: lr_scale / RNG offset read from device memory
void launch_sgd_step_dev(float* master, float* grad,
                         unsigned short* shadow, int has_shadow, long n,
                         const float* lr_scale_dev, float dc_keep,
                         uint64_t seed, const long* offset_dev,
                         float* momentum, float mu, int zero_grad,
                         float* ema, float ema_decay,
                         const float* clip_coef_dev, hipStream_t);
// clip_coef_dev != nullptr (both launchers): the gradient is multiplied by
// *clip_coef_dev (launch_grad_norm's stats[1]) before the drop-connect mask
// and the momentum filter, v = mu*v + coef*g (two more instantiations;
// nullptr launches the unchanged sgd_step_kernel / sgd_step_kernel_ema).
// grad_norm.hip — per-tensor and global norms of the flat fp32 gradient and
// the clip_grad_norm_ coefficient, one launch, no float atomics.  segs: up to
// GRAD_NORM_MAX_SEGS (element offset, length) pairs that tile [0, n) in
// order; grad 16 B aligned.  STORED (no pre-zeroing): stats[0] = grad_scale *
// sqrt(sum g^2), stats[1] = fminf(1, clip / (stats[0] + 1e-6f)) (clip = +inf
// gives exactly 1), stats[2 + s] = grad_scale * sqrt(sum of g^2 over segment
// s); *clipped_steps += 1 when stats[1] < 1.  part/ticket: a persistent
// workspace of GRAD_NORM_MAX_SEGS * GRAD_NORM_MAX_BLOCKS floats + one
// zero-initialised, self-resetting counter (launches on one device must not
// overlap).  The result is a pure function of (grad, n, segs, geometry).
#define GRAD_NORM_MAX_SEGS 16
#define GRAD_NORM_MAX_BLOCKS 1024
#define GRAD_NORM_CHUNK 4096  // elements per block up to MAX_BLOCKS chunks
struct GradNormSegs {
  long off[GRAD_NORM_MAX_SEGS];
  long len[GRAD_NORM_MAX_SEGS];
  int n;
};
// grid of the launch and the longest run of fp32 additions any element
// passes through (the error bound of the norms is chain + 4 roundings)
void grad_norm_plan(long n, int* blocks, int* chain);
void launch_grad_norm(const float* grad, long n, GradNormSegs segs,
                      float grad_scale, float clip, float* stats,
                      long* clipped_steps, float* part, unsigned* ticket,
                      hipStream_t);
// ema != nullptr (both launchers): the same pass also moves the fp32 moving
// average towards the new master, e -= (1 - d_k)*(e - w) with
// d_k = min(ema_decay, (1 + k)/(10 + k)), k = offset + 1 (a second
// instantiation; ema == nullptr launches the unchanged sgd_step_kernel).
// ema_publish: flat fp32 `src` [n] -> bf16 `shadow` [n] plus the transposed
// bf16 copies dst[C][R] of up to 4 row-major [R][C] slices of src, one launch.
struct EmaTransposeDesc {
  long offset;  // element offset of the [R][C] slice in src
  unsigned short* dst;
  int R, C;
};
struct EmaPublishArgs {
  const float* src;
  unsigned short* shadow;
  long n;
  EmaTransposeDesc d[4];
  int tile0[4];
  int nt, flat_blocks;
};
void launch_ema_publish(const float* src, unsigned short* shadow, long n,
                        const EmaTransposeDesc* descs, int nt, hipStream_t);
void launch_conv1_dw_pooled(const unsigned short* x, const unsigned short* dyp,
                            const uint8_t* am, float* dw, float* db, int NB,
                            int H, int W, int Cout, hipStream_t s);
void launch_grad_mask(float* g, long n, long base, float keep, uint64_t seed,
                      uint64_t step, uint64_t rank, const long* step_dev,
                      hipStream_t s);
void launch_step_advance(long* step_dev, float* lr_scale_dev, float lr0,
                         float decay, int decay_steps, float inv_contrib,
                         hipStream_t);
// data_gather.hip — batch gather from the device-resident uint8 training set
// (stateless Feistel epoch permutation keyed on seed + step / step_dev)
void launch_batch_gather(const uint8_t* img, const uint8_t* lab,
                         const unsigned short* lut, unsigned short* x,
                         long* y, uint32_t N, uint32_t B, uint64_t seed,
                         uint64_t step, const long* step_dev, hipStream_t);
// the same batch with on-device affine augmentation: image j is warped
// (integer bilinear, zero background) by row aug_indices(seed, step, j) of
// the int32 [T,6] Q16 inverse-affine `table` before the LUT.  Memory-safe
// for any table content; T >= 1.
void launch_batch_gather_aug(const uint8_t* img, const uint8_t* lab,
                             const unsigned short* lut, const int* table,
                             uint32_t T, unsigned short* x, long* y,
                             uint32_t N, uint32_t B, uint64_t seed,
                             uint64_t step, const long* step_dev,
                             hipStream_t);
// eval_ops.hip — device-side evaluation.  range_gather: the sequential chunk
// [start, start+B) of the resident set (start from the host or *start_dev),
// rows past N zero-filled with label -1.  softmax_eval: loss / live / correct
// / confusion counts ACCUMULATED into loss_sum[1] / counts[2 + C*C] over the
// rows with 0 <= label < C; optional pred[B] (255 = not live) and
// cursor_dev += B.  part/ticket: its own persistent workspace of
// SOFTMAX_MAX_BLOCKS floats + one zero-initialised, self-resetting counter.
void launch_range_gather(const uint8_t* img, const uint8_t* lab,
                         const unsigned short* lut, unsigned short* x,
                         long* y, uint32_t N, uint32_t B, uint64_t start,
                         const long* start_dev, hipStream_t);
void launch_softmax_eval(const unsigned short* logits, const long* labels,
                         float* loss_sum, int* counts, uint8_t* pred,
                         long* cursor_dev, int B, int C, float* part,
                         unsigned* ticket, hipStream_t);
void launch_transpose_bf16(const unsigned short* src, unsigned short* dst,
                           int R, int C, hipStream_t);
struct TransposeDesc {
  const unsigned short* src;
  unsigned short* dst;
  int R, C;
};
struct TransposeBatchArgs {
  TransposeDesc d[4];
  int tile0[4];
  int n, total;
  // optional fused step/LR advance (graph tail: saves one dispatch)
  int do_advance;
  long* step_dev;
  float* lr_scale_dev;
  float lr0, decay, inv_contrib;
  int decay_steps;
};
void launch_transpose_bf16_batch(const TransposeDesc* descs, int n,
                                 hipStream_t);
void launch_transpose_bf16_batch_adv(const TransposeDesc* descs, int n,
                                     long* step_dev, float* lr_scale_dev,
                                     float lr0, float decay, int decay_steps,
                                     float inv_contrib, hipStream_t);
void launch_conv1_direct_fwd(const unsigned short* x, const unsigned short* w,
                             const float* bias, unsigned short* y,
                             uint8_t* amax, int NB, int H, int W, int Cout,
                             hipStream_t);
// gemm_tile.hip — deterministic-mode entries.  The bias tails reduce in a
// fixed in-block order and store one [N] plane per block row (p.det_planes);
// the scatter-staged dW stores one [M][ldc] plane per k-slice at p.C
void gemm_dx_poolmask_128_det(const GemmParams&, hipStream_t);
void gemm_dx_poolmask_64_det(const GemmParams&, hipStream_t);
void gemm_dx_mask_128_det(const GemmParams&, hipStream_t);
void gemm_dx_mask_64_det(const GemmParams&, hipStream_t);
void gemm_dw_planes_128(const GemmParams&, hipStream_t);
void gemm_dw_planes_64(const GemmParams&, hipStream_t);
// det_reduce.hip — out[i] += ((p_0[i] + p_1[i]) + ...) + p_{P-1}[i], planes
// in index order, for up to PLANE_REDUCE_MAX destinations in one launch
#define PLANE_REDUCE_MAX 4
struct PlaneReduceDesc {
  const float* planes;  // plane p starts at planes + p * stride
  float* out;
  long n, stride;
  int P;
  int store;  // 1: out = S (an intermediate of a two-stage sum), 0: out += S
  int head;   // filled by the launcher: scalar elements before the 16 B body
  long nvec;  // filled by the launcher: 16 B groups in the body
};
struct PlaneReduceArgs {
  PlaneReduceDesc d[PLANE_REDUCE_MAX];
  int block0[PLANE_REDUCE_MAX];
  int n;
};
void launch_plane_reduce(const PlaneReduceDesc* descs, int n, hipStream_t);
// B-transposed (pre-transposed weight) forward GEMM entries
void gemm_fwd_bias_128_bt(const GemmParams&, hipStream_t);
void gemm_fwd_bias_64_bt(const GemmParams&, hipStream_t);
void gemm_fwd_relu_128_bt(const GemmParams&, hipStream_t);
void gemm_fwd_relu_64_bt(const GemmParams&, hipStream_t);
void gemm_fwd_drop_128_bt(const GemmParams&, hipStream_t);
void gemm_fwd_drop_64_bt(const GemmParams&, hipStream_t);
void conv_fwd_pool_bt(const GemmParams&, hipStream_t);
void conv1_dw_gemm(const GemmParams&, hipStream_t);
// conv_slab.hip — per-image LDS-slab conv kernels (H=W=14, Cin=32, Cout=64)
bool conv_slab_supported(int H, int W, int Cin, int Cout);
void launch_conv_fwd_slab(const unsigned short* x, const unsigned short* w,
                          const float* bias, unsigned short* y, uint8_t* amax,
                          int NB, int H, int W, int Cin, int Cout, hipStream_t);
void launch_conv_dx_slab(const unsigned short* dact, const unsigned short* w,
                         unsigned short* dx, int NB, int H, int W, int Cin,
                         int Cout, hipStream_t);
// the same from the pooled gradient gp [NB][7][7][64] + pool argmax bytes:
// the dense dact is rebuilt in the LDS slab only.  force_db = 1 | 2 picks the
// large- / small-batch instantiation at any NB, 0 = by NB
void launch_conv_dx_slab_pooled(const unsigned short* gp, const uint8_t* am,
                                const unsigned short* w, unsigned short* dx,
                                int NB, int force_db, hipStream_t);
void launch_conv_dw_slab(const unsigned short* x, const unsigned short* dact,
                         float* dw, int NB, int H, int W, int Cin, int Cout,
                         hipStream_t);
bool conv1_slab_supported(int H, int W, int Cin, int Cout);
void launch_conv1_dw_slab(const unsigned short* x, const unsigned short* dact,
                          float* dw, int NB, int H, int W, int Cout,
                          hipStream_t);
// ops_misc.hip — direct-VALU conv1 dW (Cin==1, H,W<=28, Cout<=32)
void launch_conv1_dw_direct(const unsigned short* x,
                            const unsigned short* dact, float* dw, int NB,
                            int H, int W, int Cout, hipStream_t s);
// conv1_mfma.hip — LeNet conv1 (28x28, Cin=1, Cout=32) fwd and pooled dW on
// v_mfma_f32_32x32x16_bf16; DMNIST_CONV1_VALU=1 (read per call) forces the
// v_dot2c kernels above
bool conv1_mfma_supported(int H, int W, int Cin, int Cout);
bool conv1_mfma_enabled();
int conv1_mfma_dw_group(int NB);  // images per block the dW launcher picks
void launch_conv1_mfma_fwd(const unsigned short* x, const unsigned short* w,
                           const float* bias, unsigned short* y,
                           uint8_t* amax, int NB, hipStream_t);
void launch_conv1_mfma_dw(const unsigned short* x, const unsigned short* dyp,
                          const uint8_t* am, float* dw, float* db, int NB,
                          hipStream_t);
// deterministic form: block b stores its 800 dW + 32 db sums into
// planes[b][0..832); returns the block (= plane) count
#define CONV1_DET_PLANE 832
int conv1_mfma_dw_blocks(int NB);
void launch_conv1_mfma_dw_det(const unsigned short* x,
                              const unsigned short* dyp, const uint8_t* am,
                              float* planes, int NB, hipStream_t);
// conv2_dw_slab.hip — LeNet conv2 dW (14x14, Cin=32, Cout=64) from pixel-
// major per-image LDS slabs (glds + tr16); DMNIST_DW2_SLAB=0 (read per call)
// routes the shape back to conv_dw_tr
bool conv2_dw_slab_supported(int H, int W, int Cin, int Cout);
bool conv2_dw_slab_enabled();
int conv2_dw_group(int NB);  // images per block the launcher picks
void launch_conv2_dw_slab(const unsigned short* x, const unsigned short* dact,
                          float* dw, int NB, hipStream_t);
// the same from the pooled gradient gp [NB][7][7][64] + pool argmax bytes
void launch_conv2_dw_slab_pooled(const unsigned short* x,
                                 const unsigned short* gp, const uint8_t* am,
                                 float* dw, int NB, hipStream_t);
// deterministic forms of the two launchers: image group g stores its 51 200
// sums into planes[g][..] (its five kernel-row blocks write disjoint rows).
// Only the conv2_dw_groups(NB) real groups write; the blocks that pad the
// grid to a multiple of 8 groups write nothing and their planes are not read.
#define CONV2_DET_PLANE (25 * 32 * 64)
int conv2_dw_groups(int NB);
void launch_conv2_dw_slab_det(const unsigned short* x,
                              const unsigned short* dact, float* planes,
                              int NB, hipStream_t);
void launch_conv2_dw_slab_pooled_det(const unsigned short* x,
                                     const unsigned short* gp,
                                     const uint8_t* am, float* planes, int NB,
                                     hipStream_t);
// gemm_tile.hip — split-K fwd slice entries + their summing epilogue
void gemm_fwd_slices_64(const GemmParams&, hipStream_t);
void gemm_fwd_slices_64_bt(const GemmParams&, hipStream_t);
// the same with the in-kernel fix-up: needs p.tickets, p.Y, p.relu
void gemm_fwd_slices_fix_64(const GemmParams&, hipStream_t);
void gemm_fwd_slices_fix_64_bt(const GemmParams&, hipStream_t);
// ops_misc.hip — fwd epilogue: y = [drop][relu](sum_slices + bias), bf16
void launch_fwd_epilogue(const float* acc, const float* bias,
                         unsigned short* y, int M, int N, int slices,
                         int relu, float p_keep, uint64_t seed,
                         uint64_t offset, const long* offset_dev,
                         hipStream_t);
