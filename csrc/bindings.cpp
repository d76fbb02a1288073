// PyTorch bindings for the gfx950 kernel library (_dmnist_hip).
// Every op validates dtype/contiguity and fails loudly — no silent
// fallbacks (the GPU path must run these kernels, _C.py policy).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <map>
#include <tuple>

#include "kernels.h"

namespace {

#define CHECK_BF16(t) TORCH_CHECK((t).scalar_type() == at::kBFloat16, #t " must be bf16")
#define CHECK_F32(t) TORCH_CHECK((t).scalar_type() == at::kFloat, #t " must be fp32")
#define CHECK_CONTIG(t) TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")
#define CHECK_CUDA(t) TORCH_CHECK((t).is_cuda(), #t " must be on GPU")

const unsigned short* bf16_ptr(const torch::Tensor& t) {
  return reinterpret_cast<const unsigned short*>(t.data_ptr());
}
unsigned short* bf16_mut(torch::Tensor& t) {
  return reinterpret_cast<unsigned short*>(t.data_ptr());
}

hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

int cdiv(int a, int b) { return (a + b - 1) / b; }

// Zeroed per-device workspace of a kernel that keeps self-resetting state
// (partials, tickets) between launches: allocated on the first call per
// device, which must therefore run outside graph capture.  Each op owns its
// slots (one launch at a time per device and op); the vectors are leaked on
// purpose, so no tensor is freed after the runtime has shut down.
using WorkspaceSlots = std::vector<torch::Tensor>;

torch::Tensor& device_workspace(WorkspaceSlots& slots,
                                const torch::Tensor& like, int64_t numel,
                                at::ScalarType dtype, hipStream_t s,
                                const char* op, const char* capture_msg) {
  int dev = like.get_device();
  TORCH_CHECK(dev >= 0 && dev < (int)slots.size(), op, ": bad device index");
  if (!slots[dev].defined()) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    hipStreamIsCapturing(s, &cap);
    TORCH_CHECK(cap == hipStreamCaptureStatusNone, capture_msg);
    slots[dev] = torch::zeros({numel}, like.options().dtype(dtype));
  }
  return slots[dev];
}

// --------------------------------------------------------------------------
// Deterministic mode (docs/KERNELS.md, "Deterministic mode").  A per-process
// switch read on every call.  With it on, the gradient ops of the default
// fused LeNet route launch their *_det sibling: blocks store private planes,
// plane_reduce adds them in index order on the producer's stream and does the
// one add into the bucket.  Ops whose route still needs float atomics across
// blocks (or LDS float atomics) raise instead of running.
// --------------------------------------------------------------------------
std::atomic<bool> g_deterministic{false};
bool det_on() { return g_deterministic.load(std::memory_order_relaxed); }

[[noreturn]] void det_refuse(const char* op, const char* route) {
  TORCH_CHECK(false, op, ": deterministic mode is on and this route is not "
              "covered (", route, "); refusing to run it");
  abort();
}

// One plane region per (device, site, destination size): the ops of one site
// and size are ordered on a stream or graph (as the softmax workspace is), and
// sites that run concurrently (conv2 dW on the side stream, the bias tails
// while fc dW is in flight) never share a region.  Planes are never assumed
// to hold anything: every element the reduction reads is stored in the same
// step.  (Re)allocated only outside graph capture.
enum DetSite { DET_SOFTMAX_DB = 0, DET_MASK_DB, DET_POOLED_DB, DET_FC_DW,
               DET_CONV2_DW, DET_CONV1 };
#define DET_MAX_BYTES (int64_t(1) << 30)
using DetRegions = std::map<std::tuple<int, int, int64_t>, torch::Tensor>;
DetRegions& det_regions() {
  static auto* r = new DetRegions();  // leaked like the other workspaces
  return *r;
}

float* det_region(DetSite site, const torch::Tensor& like, int64_t n,
                  int64_t planes, hipStream_t s, const char* op,
                  const char* setting) {
  const int64_t need = planes * n;
  TORCH_CHECK(need * 4 <= DET_MAX_BYTES, op, ": deterministic mode needs ",
              planes, " planes of ", n, " floats (", need * 4,
              " bytes), above the 1 GiB workspace limit; ", setting);
  auto key = std::make_tuple((int)like.get_device(), (int)site, n);
  auto& regions = det_regions();
  auto it = regions.find(key);
  if (it == regions.end() || it->second.numel() < need) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    hipStreamIsCapturing(s, &cap);
    TORCH_CHECK(cap == hipStreamCaptureStatusNone, op,
                ": deterministic-mode plane workspace is missing or too "
                "small and cannot be allocated during graph capture; run the "
                "op once outside capture first");
    if (it != regions.end()) {
      // a graph captured earlier may still hold the smaller region's address:
      // it is retired, never freed
      static auto* retired = new std::vector<torch::Tensor>();
      retired->push_back(it->second);
    }
    regions[key] = torch::empty({need}, like.options().dtype(at::kFloat));
    it = regions.find(key);
  }
  return it->second.data_ptr<float>();
}

void reduce_planes(const float* planes, float* out, int64_t n, int64_t stride,
                   int P, hipStream_t s, bool store = false) {
  PlaneReduceDesc d{};
  d.planes = planes; d.out = out; d.n = n; d.stride = stride; d.P = P;
  d.store = store ? 1 : 0;
  launch_plane_reduce(&d, 1, s);
}

int pick_splitk(int mtiles, int ntiles, int ksteps) {
  int tiles = mtiles * ntiles;
  if (tiles >= 256 || ksteps <= 1) return 1;
  int want = std::min(ksteps, std::max(1, 512 / tiles));
  return want;
}

// Largest split <= want that leaves no k-slice empty: the kernels give each
// slice ceil(ksteps/splitk) steps of THEIR K-step, so the last slice starts
// at (splitk-1)*ceil(ksteps/splitk), which must be < ksteps.
int clamp_splitk(int want, int ksteps) {
  int s = std::max(1, std::min(want, ksteps));
  int per = cdiv(ksteps, s);
  return cdiv(ksteps, per);
}

// glds + tr16 dW staging (dw_tr.hip); DMNIST_DW_TR=0 reverts to the
// scatter-staged gemm_tile path for A/B comparison
int dw_tr_level() {
  static int v = [] {
    const char* e = getenv("DMNIST_DW_TR");
    return e ? atoi(e) : 1;
  }();
  return v;
}
bool dw_tr_enabled() { return dw_tr_level() != 0; }

// conv2 dW from pixel-major LDS slabs (conv2_dw_slab.hip) replaces
// conv_dw_tr for its one shape; DMNIST_DW2_SLAB=0 (read per call) and the
// DMNIST_DW_SPREAD contention probe keep conv_dw_tr
bool conv2_dw_slab_route(int H, int W, int Cin, int Cout) {
  return conv2_dw_slab_supported(H, W, Cin, Cout) && dw_tr_enabled() &&
         conv2_dw_slab_enabled() && !getenv("DMNIST_DW_SPREAD");
}

// fc dW (dW += x^T dyeff) route: tile shape and split of the batch axis.
// tr = 1: dw_tr_kernel<bn, AM_PLAIN, tbm>; tr = 0: the scatter-staged
// gemm_tile path (tbm = bn = its square tile).  Both kernels step the batch
// axis by 64, so the split is clamped against cdiv(B, 64) and never leaves a
// slice empty.  splitk == 1 on the tr route is single-writer (no atomics)
// when the bucket view is 16 B aligned.
// DMNIST_DW_PLAN (read per call): "0" keeps the pre-plan choice (128-row
// tiles, split from pick_splitk); "tbm,bn,splitk" forces one (sweeps).
struct DwPlan { int tr, tbm, bn, splitk; };
DwPlan linear_dw_plan(int K, int N, int B) {
  const int ksteps = cdiv(B, 64);
  if (!(dw_tr_enabled() && K % 8 == 0 && N % 64 == 0)) {
    int bm = cdiv(K, 128) * cdiv(N, 128) >= 128 ? 128 : 64;
    int want = pick_splitk(cdiv(K, bm), cdiv(N, bm), cdiv(B, 32));
    return {0, bm, bm, clamp_splitk(want, ksteps)};
  }
  int bn = (N % 128 == 0) ? 128 : 64;
  DwPlan old{1, 128, bn,
             clamp_splitk(pick_splitk(cdiv(K, 128), cdiv(N, bn), cdiv(B, 32)),
                          ksteps)};
  if (const char* e = getenv("DMNIST_DW_PLAN")) {
    int tbm = 0, fbn = 0, sk = 0;
    if (sscanf(e, "%d,%d,%d", &tbm, &fbn, &sk) == 3 &&
        (tbm == 64 || tbm == 128) && (fbn == 64 || fbn == 128) &&
        N % fbn == 0)
      return {1, tbm, fbn, clamp_splitk(sk, ksteps)};
    return old;
  }
  // Problems whose 64-row tiles fill the chip by themselves (fc1: 49 x 8 =
  // 392 blocks of 64 x 64) need no deep split to find parallelism, and the
  // flush (one fp32 atomic per element per slice) is what the short batches
  // pay for.  Measured on fc1, solo (profiles/fc1_epilogues_b1024_b8192.md):
  // B=1024 single-writer 64x64 17.6 us against 27.7; B=2048 / 4096 64x128
  // split 2 25.8 / 36.6 against 33.7 / 43.0; at B=8192 the pre-plan choice
  // (57.8) is level with the best of the sweep (57.4) and stays.  The tier
  // edges sit halfway between the measured batches.
  if (cdiv(K, 64) * cdiv(N, 64) >= 256) {
    if (B < 1536) return {1, 64, 64, 1};
    if (B < 6144) return {1, 64, bn, clamp_splitk(2, ksteps)};
  }
  return old;
}

void launch_linear_dw(GemmParams& p, int K, int N, int B, hipStream_t s,
                      const torch::Tensor& like) {
  DwPlan pl = linear_dw_plan(K, N, B);
  p.splitk = pl.splitk;
  if (det_on() && pl.splitk > 1) {
    // deterministic mode: one stored plane per k-slice, summed in slice
    // order.  splitk == 1 launches below are already one writer per element.
    const int64_t n = (int64_t)K * N;
    float* planes = det_region(DET_FC_DW, like, n, pl.splitk, s,
                               "linear_dw_into", "lower the split "
                               "(DMNIST_DW_PLAN)");
    float* out = reinterpret_cast<float*>(p.C);
    if (pl.tr) {
      p.det_planes = planes; p.det_stride = n;
      gemm_dw_tr_det(p, pl.tbm, pl.bn, s);
    } else {
      p.C = planes;  // OUT_F32_SLICES: slice z at C + z*M*ldc
      (pl.tbm == 128 ? gemm_dw_planes_128 : gemm_dw_planes_64)(p, s);
    }
    reduce_planes(planes, out, n, n, pl.splitk, s);
    return;
  }
  if (pl.tr) {
    bool sw = pl.splitk == 1 && ((uintptr_t)p.C & 15) == 0 && p.ldc % 4 == 0;
    gemm_dw_tr(p, pl.tbm, pl.bn, sw, s);
  } else {
    (pl.tbm == 128 ? gemm_dw_128 : gemm_dw_64)(p, s);
  }
}

// --------------------------------------------------------------------------
torch::Tensor linear_act_fwd_impl(torch::Tensor x, torch::Tensor w,
                                  torch::Tensor b, bool relu, double p_keep,
                                  int64_t seed, int64_t offset,
                                  const long* offset_dev,
                                  const c10::optional<torch::Tensor>& wT) {
  CHECK_CUDA(x); CHECK_BF16(x); CHECK_CONTIG(x);
  CHECK_BF16(w); CHECK_CONTIG(w);
  CHECK_F32(b); CHECK_CONTIG(b);
  int M = x.size(0), K = x.size(1), N = w.size(1);
  TORCH_CHECK(w.size(0) == K, "w/x shape mismatch");
  auto y = torch::empty({M, N}, x.options());
  GemmParams p{};
  p.A = bf16_ptr(x);
  p.bias = b.data_ptr<float>();
  p.C = y.data_ptr(); p.amax = nullptr;
  p.M = M; p.N = N; p.K = K;
  p.lda = K; p.ldc = N;
  p.splitk = 1;
  p.p_keep = (float)p_keep; p.seed = (uint64_t)seed; p.offset = (uint64_t)offset;
  p.offset_dev = offset_dev;
  bool drop = p_keep < 1.0;
  TORCH_CHECK(!drop || relu, "dropout path requires relu epilogue");
  // 128x128 tiles amortize staging best, but a 128^2 grid below ~2 blocks/CU
  // is occupancy-starved (fc1 fwd @8192: 256 blocks = 1/CU, MFMA 6.9%);
  // drop to 64x64 when the 128-grid can't fill the chip twice
  int g128 = cdiv(M, 128) * cdiv(N, 128);
  bool big = g128 >= 512;
  if (const char* e = getenv("DMNIST_FC_TILE")) big = atoi(e) >= 128;
  auto s = cur_stream();
  bool bt = wT.has_value() && wT->defined();
  if (bt) {
    // pre-transposed weight copy [N][K] -> vector B staging (B_NMAJ)
    CHECK_BF16((*wT)); CHECK_CONTIG((*wT));
    TORCH_CHECK(wT->size(0) == N && wT->size(1) == K, "wT shape mismatch");
    p.B = bf16_ptr(*wT); p.ldb = K;
  } else {
    p.B = bf16_ptr(w); p.ldb = N;
  }
  // split-K forward for grid-starved shapes (fc1 fwd @B=1024: 128 blocks
  // = half the chip idle): each k-slice writes its own fp32 [M][N] plane
  // (deterministic — no atomics), a fused epilogue sums planes + applies
  // bias/relu/philox-dropout.  DMNIST_FC_NOSPLIT=1 disables.
  int tiles64 = cdiv(M, 64) * cdiv(N, 64);
  int ksteps = cdiv(K, 64);
  // only deep-K shapes: short k-chains (fc2: ksteps=8) lose the plane +
  // epilogue overhead (measured 9.7 -> 16.4 us)
  if (!big && tiles64 < 256 && ksteps >= 16 &&
      !getenv("DMNIST_FC_NOSPLIT")) {
    int sk = std::min(ksteps, std::max(2, 512 / tiles64));
    auto acc = torch::empty({(int64_t)sk, (int64_t)M, (int64_t)N},
                            x.options().dtype(at::kFloat));
    p.C = acc.data_ptr();
    p.splitk = sk;
    // In-kernel fix-up, DMNIST_FC_FIXUP=1 (read per call): the last slice
    // block of a tile sums the planes and writes y, no second launch.  NOT
    // dispatched by default: publishing the fp32 planes across the XCDs
    // costs more than the launch it saves (fc1 @B=1024 solo: 35 us against
    // 28 us for the two launches; step 0.277-0.279 against 0.269-0.270 ms,
    // docs/KERNELS.md).  One zeroed, self-resetting ticket per tile (tiles64
    // < 256 on this route) lives in a per-device workspace, allocated on
    // the first call outside graph capture.  Like softmax's workspace it
    // serves ONE launch at a time per device: split-K forwards of one
    // device must be ordered on a stream (or graph), never concurrent.
    const char* fe = getenv("DMNIST_FC_FIXUP");
    bool fixup = fe && atoi(fe) != 0 && N % 8 == 0;
    if (fixup) {
      static auto* ws = new WorkspaceSlots(64);
      auto& tickets = device_workspace(
          *ws, x, 256, at::kInt, s, "linear_act_fwd",
          "linear_act_fwd: first split-K call on a device allocates "
          "its ticket workspace and must run outside graph capture");
      p.tickets = reinterpret_cast<unsigned*>(tickets.data_ptr<int>());
      p.Y = bf16_mut(y);
      p.relu = relu ? 1 : 0;
    }
    if (bt) {
      CHECK_BF16((*wT)); CHECK_CONTIG((*wT));
      TORCH_CHECK(wT->size(0) == N && wT->size(1) == K, "wT shape mismatch");
      p.B = bf16_ptr(*wT); p.ldb = K;
      (fixup ? gemm_fwd_slices_fix_64_bt : gemm_fwd_slices_64_bt)(p, s);
    } else {
      p.B = bf16_ptr(w); p.ldb = N;
      (fixup ? gemm_fwd_slices_fix_64 : gemm_fwd_slices_64)(p, s);
    }
    if (!fixup)
      launch_fwd_epilogue(acc.data_ptr<float>(), b.data_ptr<float>(),
                          bf16_mut(y), M, N, sk, relu ? 1 : 0, (float)p_keep,
                          (uint64_t)seed, (uint64_t)offset, offset_dev, s);
    return y;
  }
  if (bt) {
    // pre-transposed weight copy [N][K] -> vector B staging (B_NMAJ)
    CHECK_BF16((*wT)); CHECK_CONTIG((*wT));
    TORCH_CHECK(wT->size(0) == N && wT->size(1) == K, "wT shape mismatch");
    p.B = bf16_ptr(*wT); p.ldb = K;
    if (drop) (big ? gemm_fwd_drop_128_bt : gemm_fwd_drop_64_bt)(p, s);
    else if (relu) (big ? gemm_fwd_relu_128_bt : gemm_fwd_relu_64_bt)(p, s);
    else (big ? gemm_fwd_bias_128_bt : gemm_fwd_bias_64_bt)(p, s);
  } else {
    p.B = bf16_ptr(w); p.ldb = N;
    if (drop) (big ? gemm_fwd_drop_128 : gemm_fwd_drop_64)(p, s);
    else if (relu) (big ? gemm_fwd_relu_128 : gemm_fwd_relu_64)(p, s);
    else (big ? gemm_fwd_bias_128 : gemm_fwd_bias_64)(p, s);
  }
  return y;
}

torch::Tensor linear_act_fwd(torch::Tensor x, torch::Tensor w, torch::Tensor b,
                             bool relu, double p_keep, int64_t seed,
                             int64_t offset,
                             c10::optional<torch::Tensor> wT) {
  return linear_act_fwd_impl(x, w, b, relu, p_keep, seed, offset, nullptr, wT);
}

// hipGraph-capturable variant: dropout RNG offset read from device memory
torch::Tensor linear_act_fwd_dev(torch::Tensor x, torch::Tensor w,
                                 torch::Tensor b, bool relu, double p_keep,
                                 int64_t seed, torch::Tensor offset_dev,
                                 c10::optional<torch::Tensor> wT) {
  TORCH_CHECK(offset_dev.scalar_type() == at::kLong && offset_dev.is_cuda(),
              "offset_dev must be a cuda int64 tensor");
  return linear_act_fwd_impl(x, w, b, relu, p_keep, seed, 0,
                             offset_dev.data_ptr<long>(), wT);
}

// --------------------------------------------------------------------------
// Linear backward steps.  Each route decision lives in ONE function here; the
// composite (autograd path) and the fine-grained ops of the hand-scheduled
// fused step (engine/fused_step.py) both call it.
// --------------------------------------------------------------------------
// dyeff = dy masked by relu/dropout (recovered from sign(y)), db += column
// sums.  Without a mask dyeff IS dy (no allocation) and y is not read.
torch::Tensor mask_step(const torch::Tensor& dy, const torch::Tensor& y,
                        bool relu, double p_keep, float* db, hipStream_t s) {
  if (det_on())
    det_refuse("mask_db / linear_act_bwd",
               "relu_drop_bwd adds its column sums into db with float atomics");
  int B = dy.size(0), N = dy.size(1);
  bool mask = relu || p_keep < 1.0;
  torch::Tensor dyeff = mask ? torch::empty_like(dy) : dy;
  launch_relu_drop_bwd(bf16_ptr(dy), mask ? bf16_ptr(y) : bf16_ptr(dy),
                       bf16_mut(dyeff), db, B, N, (float)(1.0 / p_keep),
                       mask ? 1 : 0, s);
  return dyeff;
}

// dW[K,N] += x^T @ dyeff  (fp32; route and split from linear_dw_plan)
void linear_dw_step(const torch::Tensor& x, const torch::Tensor& dyeff,
                    void* dw, hipStream_t s) {
  int B = x.size(0), K = x.size(1), N = dyeff.size(1);
  GemmParams p{};
  p.A = bf16_ptr(x); p.B = bf16_ptr(dyeff);
  p.C = dw;
  p.M = K; p.N = N; p.K = B;
  p.lda = K;  // A_T: A[m][k'] = x[k'*lda + m]
  p.ldb = N; p.ldc = N;
  launch_linear_dw(p, K, N, B, s, x);
}

// out[B,K] = dyeff[B,N] @ w[K,N]^T: the block every dX GEMM shares; the
// fused variants add only their epilogue fields
GemmParams dx_params(const torch::Tensor& dyeff, const torch::Tensor& w,
                     void* out) {
  int B = dyeff.size(0), N = dyeff.size(1), K = w.size(0);
  GemmParams p{};
  p.A = bf16_ptr(dyeff); p.B = bf16_ptr(w);
  p.C = out;
  p.M = B; p.N = K; p.K = N;
  p.lda = N; p.ldb = N; p.ldc = K;  // B_NMAJ: Bs[n'][k'] = w[n'*N + k']
  p.splitk = 1;
  return p;
}

// plain 64/128 tile choice of a dX GEMM: 128-tiles once they fill a grid
bool dx_big_tiles(const GemmParams& p) {
  return cdiv(p.M, 128) * cdiv(p.N, 128) >= 128;
}

torch::Tensor linear_dx_step(const torch::Tensor& dyeff,
                             const torch::Tensor& w, hipStream_t s) {
  auto dx = torch::empty({dyeff.size(0), w.size(0)}, dyeff.options());
  GemmParams p = dx_params(dyeff, w, dx.data_ptr());
  (dx_big_tiles(p) ? gemm_dx_128 : gemm_dx_64)(p, s);
  return dx;
}

// core backward; when dw/db are passed they are accumulated into
// (pre-zeroed fp32 bucket views — the direct-grad path); else allocated.
std::vector<torch::Tensor> linear_act_bwd_impl(torch::Tensor dy, torch::Tensor x,
                                               torch::Tensor w, torch::Tensor y,
                                               bool relu, double p_keep,
                                               bool need_dx,
                                               torch::Tensor dw, torch::Tensor db) {
  CHECK_CUDA(dy); CHECK_BF16(dy); CHECK_CONTIG(dy);
  CHECK_BF16(x); CHECK_CONTIG(x);
  CHECK_BF16(w); CHECK_CONTIG(w);
  int K = x.size(1), N = w.size(1);
  auto s = cur_stream();
  if (!db.defined())
    db = torch::zeros({N}, x.options().dtype(at::kFloat));
  CHECK_F32(db); CHECK_CONTIG(db);
  auto dyeff = mask_step(dy, y, relu, p_keep, db.data_ptr<float>(), s);
  if (!dw.defined())
    dw = torch::zeros({K, N}, x.options().dtype(at::kFloat));
  CHECK_F32(dw); CHECK_CONTIG(dw);
  linear_dw_step(x, dyeff, dw.data_ptr(), s);
  auto dx = need_dx ? linear_dx_step(dyeff, w, s)
                    : torch::empty({0}, x.options());
  return {dx, dw, db};
}

std::vector<torch::Tensor> linear_act_bwd(torch::Tensor dy, torch::Tensor x,
                                          torch::Tensor w, torch::Tensor y,
                                          bool relu, double p_keep,
                                          bool need_dx) {
  return linear_act_bwd_impl(dy, x, w, y, relu, p_keep, need_dx,
                             torch::Tensor(), torch::Tensor());
}

torch::Tensor linear_act_bwd_into(torch::Tensor dy, torch::Tensor x,
                                  torch::Tensor w, torch::Tensor y,
                                  bool relu, double p_keep, bool need_dx,
                                  torch::Tensor dw_out, torch::Tensor db_out) {
  auto r = linear_act_bwd_impl(dy, x, w, y, relu, p_keep, need_dx,
                               dw_out.view({x.size(1), w.size(1)}), db_out);
  return r[0];
}

// --------------------------------------------------------------------------
std::vector<torch::Tensor> conv_pool_fwd(torch::Tensor x, torch::Tensor w,
                                         torch::Tensor b,
                                         c10::optional<torch::Tensor> wT) {
  CHECK_CUDA(x); CHECK_BF16(x); CHECK_CONTIG(x);
  CHECK_BF16(w); CHECK_CONTIG(w);
  CHECK_F32(b); CHECK_CONTIG(b);
  int NB = x.size(0), H = x.size(1), W = x.size(2), Cin = x.size(3);
  TORCH_CHECK(w.dim() == 4 && w.size(0) == 5 && w.size(1) == 5 &&
              w.size(2) == Cin, "conv weight must be [5,5,Cin,Cout]");
  int Cout = w.size(3);
  int Ho = H / 2, Wo = W / 2;
  auto y = torch::empty({NB, Ho, Wo, Cout}, x.options());
  auto amax = torch::empty({NB, Ho, Wo, Cout}, x.options().dtype(at::kByte));
  GemmParams p{};
  p.A = bf16_ptr(x); p.B = bf16_ptr(w);
  p.bias = b.data_ptr<float>();
  p.C = y.data_ptr(); p.amax = amax.data_ptr<uint8_t>();
  p.M = NB * Ho * Wo * 4; p.N = Cout; p.K = 25 * Cin;
  p.ldb = Cout; p.ldc = Cout;
  p.splitk = 1;
  p.CB = NB; p.CH = H; p.CW = W; p.CHo = Ho; p.CWo = Wo;
  p.Cin = Cin; p.Cout = Cout;
  auto s = cur_stream();
  if (Cin == 1 && conv1_mfma_supported(H, W, Cin, Cout) &&
      conv1_mfma_enabled() &&
      reinterpret_cast<uintptr_t>(x.data_ptr()) % 8 == 0) {
    // LeNet conv1: per-image LDS slab feeding 32x32x16 MFMAs with
    // contiguous-pixel A fragments (conv1_mfma.hip)
    launch_conv1_mfma_fwd(bf16_ptr(x), bf16_ptr(w), b.data_ptr<float>(),
                          bf16_mut(y), amax.data_ptr<uint8_t>(), NB, s);
  } else if (Cin == 1) {
    // other Cin=1 shapes (and DMNIST_CONV1_VALU=1): direct v_dot2c kernel.
    // The im2col MFMA form loses here (per-element global A gather,
    // 579 us at B=8192); only the slab form above beats the VALU kernel.
    launch_conv1_direct_fwd(bf16_ptr(x), bf16_ptr(w), b.data_ptr<float>(),
                            bf16_mut(y), amax.data_ptr<uint8_t>(), NB, H, W,
                            Cout, s);
  } else if (conv_slab_supported(H, W, Cin, Cout)) {
    // per-image LDS slab: activations cross the fabric once (not 25x)
    launch_conv_fwd_slab(bf16_ptr(x), bf16_ptr(w), b.data_ptr<float>(),
                         bf16_mut(y), amax.data_ptr<uint8_t>(), NB, H, W,
                         Cin, Cout, s);
  } else {
    TORCH_CHECK(Cin % 8 == 0, "conv requires Cin==1 or Cin%8==0");
    if (wT.has_value() && wT->defined()) {
      CHECK_BF16((*wT)); CHECK_CONTIG((*wT));
      p.B = bf16_ptr(*wT); p.ldb = 25 * Cin;
      conv_fwd_pool_bt(p, s);
    } else {
      conv_fwd_pool(p, s);
    }
  }
  return {y, amax};
}

// --------------------------------------------------------------------------
// Conv backward steps, shared like the linear ones above.
// --------------------------------------------------------------------------
// scatter the pooled grad (relu-masked) back to conv-output positions
// [NB][H][W][C]; db += the conv bias grad
torch::Tensor pool_scatter_step(const torch::Tensor& dy, const torch::Tensor& y,
                                const torch::Tensor& amax, float* db, int H,
                                int W, hipStream_t s) {
  if (det_on())
    det_refuse("pool_scatter / conv_pool_bwd",
               "pool_bwd_scatter adds db with float atomics");
  int NB = dy.size(0), Ho = dy.size(1), Wo = dy.size(2), C = dy.size(3);
  auto dact = torch::empty({NB, H, W, C}, dy.options());
  launch_pool_bwd_scatter(bf16_ptr(dy), bf16_ptr(y), amax.data_ptr<uint8_t>(),
                          bf16_mut(dact), db, NB * Ho * Wo, C, H, W, Wo, s);
  return dact;
}

// THE conv dW route: dw[(khkw,ci), co] += sum_pixels x_shift * dact.  Both
// conv_dw_into and the composite conv_pool_bwd come through here.  The
// DMNIST_DW_SPREAD contention probe (atomics redirected to a throwaway
// scratch: dw is NOT produced) therefore applies to both; before the ladder
// had one copy, only conv_dw_into redirected.
void route_conv_dw(const torch::Tensor& x, const torch::Tensor& dact,
                   float* dw, int NB, int H, int W, int Cin, int Cout,
                   hipStream_t s) {
  if (det_on()) {
    // deterministic mode covers the dense conv2 slab kernel in its shipped
    // form (it shares its flush with the pooled one); every other conv dW
    // route adds into dw with float atomics across blocks
    bool slab = Cin != 1 && conv2_dw_slab_route(H, W, Cin, Cout) &&
                !(conv_slab_supported(H, W, Cin, Cout) &&
                  ((dw_tr_level() == 0 && NB >= 2048) ||
                   getenv("DMNIST_DW_G"))) &&
                !getenv("DMNIST_DW2_KHB") && !getenv("DMNIST_DW2_NBUF");
    if (!slab)
      det_refuse("conv_dw_into / conv_pool_bwd",
                 "only the conv2 slab route (14x14, 32->64, no sweep "
                 "switches) has a plane flush; this route uses float atomics");
    if (NB <= 0) return;
    int groups = conv2_dw_groups(NB);
    float* planes = det_region(DET_CONV2_DW, x, CONV2_DET_PLANE, groups, s,
                               "conv_dw_into", "raise DMNIST_DW2_G");
    launch_conv2_dw_slab_det(bf16_ptr(x), bf16_ptr(dact), planes, NB, s);
    reduce_planes(planes, dw, CONV2_DET_PLANE, CONV2_DET_PLANE, groups, s);
    return;
  }
  GemmParams p{};
  p.A = bf16_ptr(x); p.B = bf16_ptr(dact);
  p.C = dw;
  p.M = 25 * Cin; p.N = Cout; p.K = NB * H * W;
  p.ldb = Cout; p.ldc = Cout;
  p.CB = NB; p.CH = H; p.CW = W; p.Cin = Cin; p.Cout = Cout;
  if (Cin == 1 && H <= 28 && W <= 28 && Cout <= 32 &&
      !getenv("DMNIST_DW1_SLAB")) {
    launch_conv1_dw_direct(bf16_ptr(x), bf16_ptr(dact), dw, NB, H, W, Cout,
                           s);
  } else if (Cin == 1 && conv1_slab_supported(H, W, Cin, Cout)) {
    launch_conv1_dw_slab(bf16_ptr(x), bf16_ptr(dact), dw, NB, H, W, Cout, s);
  } else if (Cin == 1) {
    // single 32x32 tile: target ~2048 blocks so the latency-bound gather
    // k-chain is short and the chip stays full
    p.splitk = std::min(cdiv(p.K, 64), 2048);
    conv1_dw_gemm(p, s);
  } else if (conv_slab_supported(H, W, Cin, Cout) &&
             ((dw_tr_level() == 0 && NB >= 2048) || getenv("DMNIST_DW_G"))) {
    // per-image-group slab dW: wins when the flush atomics amortize over
    // >=4 images/block; below that the implicit-GEMM form is faster
    launch_conv_dw_slab(bf16_ptr(x), bf16_ptr(dact), dw, NB, H, W, Cin, Cout,
                        s);
  } else if (conv2_dw_slab_route(H, W, Cin, Cout)) {
    launch_conv2_dw_slab(bf16_ptr(x), bf16_ptr(dact), dw, NB, s);
  } else {
    int tiles = cdiv(p.M, 128) * cdiv(p.N, 64);
    // total blocks target (DMNIST_DW_BLOCKS sweeps it): at BK=32 the
    // small-batch optimum is 1024 blocks (63 vs 76 us @1024), large
    // batches want 2048 (tools/dwsweep.py)
    int want = p.K <= 262144 ? 1024 : 2048;
    if (const char* e = getenv("DMNIST_DW_BLOCKS")) want = atoi(e);
    p.splitk = std::min(cdiv(p.K, 64), std::max(1, want / tiles));
    if (getenv("DMNIST_DW_SPREAD")) {
      // contention probe: atomics land in a throwaway 16-plane scratch
      static torch::Tensor scratch;
      int64_t need = 16LL * p.M * p.N;
      if (!scratch.defined() || scratch.numel() < need)
        scratch = torch::zeros({need}, dact.options().dtype(at::kFloat));
      p.C = scratch.data_ptr();
      p.offset = 1;
    }
    if (dw_tr_enabled() && Cin % 8 == 0 && Cout % 64 == 0)
      conv_dw_tr(p, s);
    else
      conv_dw_gemm(p, s);
  }
}

// conv dX: the per-image LDS slab where it fits, the implicit GEMM elsewhere
torch::Tensor conv_dx_step(const torch::Tensor& dact, const torch::Tensor& w,
                           int Cin, hipStream_t s) {
  int NB = dact.size(0), H = dact.size(1), W = dact.size(2),
      Cout = dact.size(3);
  auto dx = torch::empty({NB, H, W, Cin}, dact.options());
  if (conv_slab_supported(H, W, Cin, Cout)) {
    launch_conv_dx_slab(bf16_ptr(dact), bf16_ptr(w), bf16_mut(dx), NB, H, W,
                        Cin, Cout, s);
  } else {
    TORCH_CHECK(Cout % 32 == 0, "conv_dx requires Cout%32==0");
    GemmParams p{};
    p.A = bf16_ptr(dact); p.B = bf16_ptr(w);
    p.C = dx.data_ptr();
    p.M = NB * H * W; p.N = Cin; p.K = 25 * Cout;
    p.ldc = Cin;
    p.CB = NB; p.CH = H; p.CW = W; p.Cin = Cin; p.Cout = Cout;
    p.splitk = 1;
    conv_dx_gemm(p, s);
  }
  return dx;
}

std::vector<torch::Tensor> conv_pool_bwd_impl(torch::Tensor dy, torch::Tensor x,
                                              torch::Tensor w, torch::Tensor y,
                                              torch::Tensor amax, bool need_dx,
                                              torch::Tensor dw, torch::Tensor db) {
  CHECK_CUDA(dy); CHECK_BF16(dy); CHECK_CONTIG(dy);
  CHECK_BF16(x); CHECK_CONTIG(x); CHECK_BF16(w); CHECK_CONTIG(w);
  int NB = x.size(0), H = x.size(1), W = x.size(2), Cin = x.size(3);
  int Cout = w.size(3);
  auto s = cur_stream();
  if (!db.defined())
    db = torch::zeros({Cout}, x.options().dtype(at::kFloat));
  CHECK_F32(db); CHECK_CONTIG(db);
  auto dact = pool_scatter_step(dy, y, amax, db.data_ptr<float>(), H, W, s);
  if (!dw.defined())
    dw = torch::zeros({5, 5, Cin, Cout}, x.options().dtype(at::kFloat));
  CHECK_F32(dw); CHECK_CONTIG(dw);
  route_conv_dw(x, dact, dw.data_ptr<float>(), NB, H, W, Cin, Cout, s);
  auto dx = need_dx ? conv_dx_step(dact, w, Cin, s)
                    : torch::empty({0}, x.options());
  return {dx, dw, db};
}

std::vector<torch::Tensor> conv_pool_bwd(torch::Tensor dy, torch::Tensor x,
                                         torch::Tensor w, torch::Tensor y,
                                         torch::Tensor amax, bool need_dx) {
  return conv_pool_bwd_impl(dy, x, w, y, amax, need_dx, torch::Tensor(),
                            torch::Tensor());
}

torch::Tensor conv_pool_bwd_into(torch::Tensor dy, torch::Tensor x,
                                 torch::Tensor w, torch::Tensor y,
                                 torch::Tensor amax, bool need_dx,
                                 torch::Tensor dw_out, torch::Tensor db_out) {
  auto r = conv_pool_bwd_impl(dy, x, w, y, amax, need_dx,
                              dw_out.view_as(w), db_out);
  return r[0];
}

// --------------------------------------------------------------------------
// Fine-grained backward pieces for the hand-scheduled fused step
// (engine/fused_step.py): the composite linear_act_bwd/conv_pool_bwd above
// stay for the autograd path; these expose the same *_step functions one at
// a time, so dW can run on a side stream while the dX chain proceeds.
// --------------------------------------------------------------------------
torch::Tensor mask_db(torch::Tensor dy, torch::Tensor y, bool relu,
                      double p_keep, torch::Tensor db_out) {
  CHECK_CUDA(dy); CHECK_BF16(dy); CHECK_CONTIG(dy);
  CHECK_F32(db_out); CHECK_CONTIG(db_out);
  return mask_step(dy, y, relu, p_keep, db_out.data_ptr<float>(),
                   cur_stream());
}

void linear_dw_into(torch::Tensor x, torch::Tensor dyeff,
                    torch::Tensor dw_out) {
  CHECK_BF16(x); CHECK_CONTIG(x); CHECK_BF16(dyeff); CHECK_CONTIG(dyeff);
  CHECK_F32(dw_out);
  linear_dw_step(x, dyeff, dw_out.data_ptr(), cur_stream());
}

torch::Tensor linear_dx(torch::Tensor dyeff, torch::Tensor w) {
  CHECK_BF16(dyeff); CHECK_CONTIG(dyeff); CHECK_BF16(w); CHECK_CONTIG(w);
  return linear_dx_step(dyeff, w, cur_stream());
}

torch::Tensor linear_dx_unpool(torch::Tensor dyeff, torch::Tensor w,
                               torch::Tensor amax, torch::Tensor db_out,
                               int64_t Ho, int64_t Wo, int64_t C) {
  // dx = dyeff @ W^T fused with maxpool2x2-backward: the dX rows are pooled
  // [Ho][Wo][C] features; the epilogue scatters each value to its argmax
  // position of the 2x2 window (amax byte: 0..3 live, 7 dead — liveness
  // encoded at forward time so no y read is needed here) and accumulates
  // the conv bias grad — dact [B][2Ho][2Wo][C] comes straight out of the
  // GEMM (replaces linear_dx + pool_scatter on the backward critical path).
  CHECK_BF16(dyeff); CHECK_CONTIG(dyeff); CHECK_BF16(w); CHECK_CONTIG(w);
  if (det_on())
    det_refuse("linear_dx_unpool",
               "the EPI_UNPOOL bias tail uses LDS and global float atomics; "
               "use linear_dx_pooled");
  int B = dyeff.size(0), K = w.size(0);
  TORCH_CHECK(K == Ho * Wo * C, "linear_dx_unpool: K != Ho*Wo*C");
  auto dact = torch::empty({B, 2 * (int)Ho, 2 * (int)Wo, (int)C},
                           dyeff.options());
  GemmParams p = dx_params(dyeff, w, dact.data_ptr());
  p.CHo = Ho; p.CWo = Wo; p.Cout = C;
  p.amax = amax.data_ptr<uint8_t>();
  p.db = db_out.defined() ? db_out.data_ptr<float>() : nullptr;
  // C % 64 == 0: every 64-column chunk of a tile is 64 channels of one
  // pooled pixel, so the epilogue stages the tile in LDS and stores whole
  // 128 B lines of dact.  DMNIST_UNPOOL_LINES=0 (read per call) keeps the
  // per-element 2-byte stores; other channel counts always take them.
  const char* le = getenv("DMNIST_UNPOOL_LINES");
  p.unpool_lines = !(le && atoi(le) == 0) && C % 64 == 0 &&
                   ((uintptr_t)p.amax & 15) == 0 && ((uintptr_t)p.C & 15) == 0;
  // 128-tile under ~2 blocks/CU is grid-starved (PMC: 57% parked at
  // B=1024's 200-block grid); 64-tiles quadruple the grid.  With line
  // stores the 128-tile already wins at 400 blocks (fc1 @B=2048: 49.7 us
  // against 59.5; at B=1024 it loses 40.8 to 36.6).
  bool big = cdiv(B, 128) * cdiv(K, 128) >= (p.unpool_lines ? 400 : 512);
  // DMNIST_UNPOOL_TILE=64|128 forces either tile at any B (read per call)
  if (const char* e = getenv("DMNIST_UNPOOL_TILE")) big = atoi(e) >= 128;
  (big ? gemm_dx_unpool_128 : gemm_dx_unpool_64)(p, cur_stream());
  return dact;
}

// 128-tile threshold of linear_dx_pooled, in 128 x 128 tiles.  Swept solo at
// fc1's 3136 x 512 (64-tile / 128-tile us): B=512 (100 tiles) 21.1 / 23.7,
// B=640 (125) 24.2 / 24.9, B=768 (150) 26.6 / 26.2, B=1024 (200) 32.1 / 28.8,
// B=2048 (400) 55.4 / 39.9.  linear_dx_unpool's 400 was set by its 4x larger
// write burst, which this epilogue does not have.
#define POOLED_DX_BIG_TILES 150

torch::Tensor linear_dx_pooled(torch::Tensor dyeff, torch::Tensor w,
                               torch::Tensor amax, torch::Tensor db_out,
                               int64_t Ho, int64_t Wo, int64_t C,
                               int64_t tile) {
  // gp = mask(dyeff @ W^T): linear_dx_unpool without the scatter.  The dX
  // rows are pooled [Ho][Wo][C] features; the epilogue zeroes the dead
  // windows (amax byte >= 4), accumulates the conv bias grad and stores the
  // POOLED gradient [B][Ho][Wo][C].  The pre-pool dact (4x the bytes, 75 %
  // zeros) is never written: conv_dx_pooled / conv_dw_pooled_into rebuild it
  // in LDS from (gp, amax).  tile = 64 | 128 forces a tile, 0 = by grid size.
  CHECK_BF16(dyeff); CHECK_CONTIG(dyeff); CHECK_BF16(w); CHECK_CONTIG(w);
  CHECK_CONTIG(amax);
  TORCH_CHECK(amax.scalar_type() == at::kByte, "amax must be uint8");
  int B = dyeff.size(0), N = dyeff.size(1), K = w.size(0);
  TORCH_CHECK(K == Ho * Wo * C, "linear_dx_pooled: K != Ho*Wo*C");
  TORCH_CHECK(w.size(1) == N, "linear_dx_pooled: w is [K][N]");
  TORCH_CHECK(amax.numel() == (int64_t)B * K, "linear_dx_pooled: amax shape");
  TORCH_CHECK(tile == 0 || tile == 64 || tile == 128,
              "linear_dx_pooled: tile is 0, 64 or 128");
  auto gp = torch::empty({B, (int)Ho, (int)Wo, (int)C}, dyeff.options());
  GemmParams p = dx_params(dyeff, w, gp.data_ptr());
  p.CHo = Ho; p.CWo = Wo; p.Cout = C;
  p.amax = amax.data_ptr<uint8_t>();
  p.db = db_out.defined() ? db_out.data_ptr<float>() : nullptr;
  // row stores (16 B per lane) need whole 16-column chunks and aligned rows;
  // anything else takes the per-element epilogue
  p.unpool_lines = K % 16 == 0 && ((uintptr_t)p.amax & 15) == 0 &&
                   ((uintptr_t)p.C & 15) == 0;
  bool big = cdiv(B, 128) * cdiv(K, 128) >= POOLED_DX_BIG_TILES;
  if (tile) big = tile == 128;
  if (det_on() && p.db && B > 0) {
    // deterministic mode: block row r stores its [K] column sums into plane
    // r.  Two ordered stages (a single one would walk rows * Ho*Wo planes of
    // C floats serially): T = sum over block rows, stored into the spare
    // plane behind them; then K = (pixel, channel), so T read as [Ho*Wo][C]
    // is the plane set of the C channel sums, added in pixel order into db
    auto s = cur_stream();
    int rows = cdiv(B, big ? 128 : 64);
    float* planes = det_region(DET_POOLED_DB, dyeff, K, rows + 1, s,
                               "linear_dx_pooled", "lower the batch size");
    float* colsum = planes + (size_t)rows * K;
    p.det_planes = planes; p.det_stride = K;
    (big ? gemm_dx_poolmask_128_det : gemm_dx_poolmask_64_det)(p, s);
    reduce_planes(planes, colsum, K, K, rows, s, /*store=*/true);
    reduce_planes(colsum, p.db, C, C, (int)(Ho * Wo), s);
    return gp;
  }
  (big ? gemm_dx_poolmask_128 : gemm_dx_poolmask_64)(p, cur_stream());
  return gp;
}

torch::Tensor linear_dx_mask(torch::Tensor dyeff, torch::Tensor w,
                             torch::Tensor actm, torch::Tensor db_out,
                             double p_keep) {
  // dx = dyeff @ W^T with the downstream relu+dropout mask folded into the
  // epilogue (mask recovered from sign(actm): kept positions are scaled by
  // 1/p_keep, dropped/clipped are 0) + bias-grad column sums into db_out —
  // replaces linear_dx + the standalone mask_db pass (fc2-dX -> dyeff1).
  CHECK_BF16(dyeff); CHECK_CONTIG(dyeff); CHECK_BF16(w); CHECK_CONTIG(w);
  CHECK_BF16(actm); CHECK_CONTIG(actm);
  int B = dyeff.size(0), K = w.size(0);
  TORCH_CHECK(actm.size(0) == B && actm.size(1) == K, "actm shape mismatch");
  auto dx = torch::empty({B, K}, dyeff.options());
  GemmParams p = dx_params(dyeff, w, dx.data_ptr());
  p.p_keep = (float)(1.0 / p_keep);  // kernel multiplies by the inverse
  p.actm = bf16_ptr(actm);
  p.db = db_out.defined() ? db_out.data_ptr<float>() : nullptr;
  if (det_on() && p.db && B > 0) {
    // deterministic mode: one [K] plane of column sums per block row
    auto s = cur_stream();
    bool big = dx_big_tiles(p);
    int rows = cdiv(B, big ? 128 : 64);
    float* planes = det_region(DET_MASK_DB, dyeff, K, rows, s,
                               "linear_dx_mask", "lower the batch size");
    p.det_planes = planes; p.det_stride = K;
    (big ? gemm_dx_mask_128_det : gemm_dx_mask_64_det)(p, s);
    reduce_planes(planes, p.db, K, K, rows, s);
    return dx;
  }
  (dx_big_tiles(p) ? gemm_dx_mask_128 : gemm_dx_mask_64)(p, cur_stream());
  return dx;
}

torch::Tensor pool_scatter(torch::Tensor dy, torch::Tensor y,
                           torch::Tensor amax, torch::Tensor db_out,
                           int64_t H, int64_t W) {
  CHECK_BF16(dy); CHECK_CONTIG(dy);
  return pool_scatter_step(dy, y, amax, db_out.data_ptr<float>(), (int)H,
                           (int)W, cur_stream());
}

void conv_dw_into(torch::Tensor x, torch::Tensor dact, torch::Tensor dw_out) {
  CHECK_BF16(x); CHECK_CONTIG(x); CHECK_BF16(dact); CHECK_CONTIG(dact);
  route_conv_dw(x, dact, dw_out.data_ptr<float>(), x.size(0), x.size(1),
                x.size(2), x.size(3), dact.size(3), cur_stream());
}

void conv1_dw_pooled(torch::Tensor x, torch::Tensor dyp, torch::Tensor am,
                     torch::Tensor dw_out, torch::Tensor db_out) {
  // conv1 dW+db straight from the pooled gradient (pool backward fused in
  // the consumer; dact1 never materialized; liveness in the amax byte) —
  // see conv1_dw_pooled_kernel.
  CHECK_BF16(x); CHECK_CONTIG(x);
  CHECK_BF16(dyp); CHECK_CONTIG(dyp);
  int NB = x.size(0), H = x.size(1), W = x.size(2);
  int Cout = dyp.size(3);
  TORCH_CHECK(x.size(3) == 1 && H == 28 && W == 28 && Cout == 32 &&
                  dyp.size(1) == H / 2 && dyp.size(2) == W / 2,
              "conv1_dw_pooled: LeNet conv1 shapes only");
  CHECK_CONTIG(am); CHECK_F32(dw_out); CHECK_CONTIG(dw_out);
  if (det_on()) {
    // deterministic mode: the MFMA kernel stores one 832-float plane (800 dW
    // + 32 db) per block; both destinations are reduced in one launch
    if (!(conv1_mfma_supported(H, W, 1, Cout) && conv1_mfma_enabled() &&
          reinterpret_cast<uintptr_t>(x.data_ptr()) % 8 == 0))
      det_refuse("conv1_dw_pooled",
                 "the DMNIST_CONV1_VALU=1 / unaligned-x kernel flushes with "
                 "float atomics");
    TORCH_CHECK(dw_out.numel() == 25 * 32, "conv1_dw_pooled: dw size");
    if (NB <= 0) return;
    auto s = cur_stream();
    int blocks = conv1_mfma_dw_blocks(NB);
    float* planes = det_region(DET_CONV1, x, CONV1_DET_PLANE, blocks, s,
                               "conv1_dw_pooled", "raise DMNIST_DW1_G");
    launch_conv1_mfma_dw_det(bf16_ptr(x), bf16_ptr(dyp),
                             am.data_ptr<uint8_t>(), planes, NB, s);
    PlaneReduceDesc d[2] = {};
    d[0].planes = planes; d[0].out = dw_out.data_ptr<float>();
    d[0].n = 25 * 32; d[0].stride = CONV1_DET_PLANE; d[0].P = blocks;
    int nd = 1;
    if (db_out.defined()) {
      CHECK_F32(db_out); CHECK_CONTIG(db_out);
      TORCH_CHECK(db_out.numel() == 32, "conv1_dw_pooled: db size");
      d[1].planes = planes + 25 * 32; d[1].out = db_out.data_ptr<float>();
      d[1].n = 32; d[1].stride = CONV1_DET_PLANE; d[1].P = blocks;
      nd = 2;
    }
    launch_plane_reduce(d, nd, s);
    return;
  }
  if (conv1_mfma_supported(H, W, 1, Cout) && conv1_mfma_enabled() &&
      reinterpret_cast<uintptr_t>(x.data_ptr()) % 8 == 0) {
    launch_conv1_mfma_dw(bf16_ptr(x), bf16_ptr(dyp), am.data_ptr<uint8_t>(),
                         dw_out.data_ptr<float>(),
                         db_out.defined() ? db_out.data_ptr<float>() : nullptr,
                         NB, cur_stream());
    return;
  }
  launch_conv1_dw_pooled(bf16_ptr(x), bf16_ptr(dyp),
                         am.data_ptr<uint8_t>(), dw_out.data_ptr<float>(),
                         db_out.defined() ? db_out.data_ptr<float>() : nullptr,
                         NB, H, W, Cout, cur_stream());
}

torch::Tensor conv_dx(torch::Tensor dact, torch::Tensor w, int64_t Cin) {
  CHECK_BF16(dact); CHECK_CONTIG(dact); CHECK_BF16(w); CHECK_CONTIG(w);
  return conv_dx_step(dact, w, (int)Cin, cur_stream());
}

// conv2 backward from the pooled gradient gp [NB][7][7][64] and the pool
// argmax bytes am: pool2 backward happens in the consumers' LDS staging and
// the dense dact [NB][14][14][64] never exists in memory.
static void check_pooled(const torch::Tensor& gp, const torch::Tensor& am) {
  CHECK_CUDA(gp); CHECK_BF16(gp); CHECK_CONTIG(gp);
  CHECK_CUDA(am); CHECK_CONTIG(am);
  TORCH_CHECK(am.scalar_type() == at::kByte, "am must be uint8");
  TORCH_CHECK(gp.dim() == 4 && gp.size(1) == 7 && gp.size(2) == 7 &&
                  gp.size(3) == 64,
              "pooled conv2 backward: gp is [NB][7][7][64]");
  TORCH_CHECK(am.numel() == gp.numel(), "am / gp shape mismatch");
  TORCH_CHECK(((uintptr_t)gp.data_ptr() & 15) == 0 &&
                  ((uintptr_t)am.data_ptr() & 7) == 0,
              "pooled conv2 backward: gp 16 B / am 8 B alignment");
}

torch::Tensor conv_dx_pooled(torch::Tensor gp, torch::Tensor am,
                             torch::Tensor w, int64_t Cin, int64_t force_db) {
  check_pooled(gp, am);
  CHECK_BF16(w); CHECK_CONTIG(w);
  TORCH_CHECK(Cin == 32 && w.numel() == 25 * 32 * 64,
              "conv_dx_pooled: LeNet conv2 shapes only");
  TORCH_CHECK(force_db >= 0 && force_db <= 2, "force_db is 0, 1 or 2");
  int NB = gp.size(0);
  auto dx = torch::empty({NB, 14, 14, 32}, gp.options());
  if (NB > 0)
    launch_conv_dx_slab_pooled(bf16_ptr(gp), am.data_ptr<uint8_t>(),
                               bf16_ptr(w), bf16_mut(dx), NB, (int)force_db,
                               cur_stream());
  return dx;
}

void conv_dw_pooled_into(torch::Tensor x, torch::Tensor gp, torch::Tensor am,
                         torch::Tensor dw_out) {
  check_pooled(gp, am);
  CHECK_CUDA(x); CHECK_BF16(x); CHECK_CONTIG(x);
  CHECK_F32(dw_out); CHECK_CONTIG(dw_out);
  TORCH_CHECK(x.dim() == 4 && x.size(0) == gp.size(0) && x.size(1) == 14 &&
                  x.size(2) == 14 && x.size(3) == 32,
              "conv_dw_pooled_into: x is [NB][14][14][32]");
  TORCH_CHECK(dw_out.numel() == 25 * 32 * 64, "conv_dw_pooled_into: dw size");
  TORCH_CHECK(((uintptr_t)x.data_ptr() & 15) == 0, "x 16 B alignment");
  if (det_on()) {
    // deterministic mode: one stored plane per image group, summed in group
    // order; the reduction is given the true group count, so the planes of
    // the blocks that pad the grid are neither written nor read
    int NB = x.size(0);
    if (NB <= 0) return;
    auto s = cur_stream();
    int groups = conv2_dw_groups(NB);
    float* planes = det_region(DET_CONV2_DW, x, CONV2_DET_PLANE, groups, s,
                               "conv_dw_pooled_into", "raise DMNIST_DW2_G");
    launch_conv2_dw_slab_pooled_det(bf16_ptr(x), bf16_ptr(gp),
                                    am.data_ptr<uint8_t>(), planes, NB, s);
    reduce_planes(planes, dw_out.data_ptr<float>(), CONV2_DET_PLANE,
                  CONV2_DET_PLANE, groups, s);
    return;
  }
  launch_conv2_dw_slab_pooled(bf16_ptr(x), bf16_ptr(gp),
                              am.data_ptr<uint8_t>(),
                              dw_out.data_ptr<float>(), (int)x.size(0),
                              cur_stream());
}

// --------------------------------------------------------------------------
// Per-device workspace of the softmax last-block reduction: two partials per
// block + the self-resetting ticket behind them.  softmax_xent_fwd and
// fc2_head share it: a step runs one or the other, ordered on its stream.
float* softmax_workspace(const torch::Tensor& like, hipStream_t s) {
  static auto* ws = new WorkspaceSlots(64);
  return device_workspace(
      *ws, like, 2 * SOFTMAX_MAX_BLOCKS + 1, at::kFloat, s, "softmax_xent",
      "softmax_xent_fwd / fc2_head: first call on a device allocates its "
      "workspace and must run outside graph capture").data_ptr<float>();
}

std::vector<torch::Tensor> softmax_xent_fwd(torch::Tensor logits,
                                            torch::Tensor labels,
                                            c10::optional<torch::Tensor> db_out,
                                            double inv_n) {
  // db_out (optional): fc2 bias grad accumulated in the same pass (column
  // sums of dlogits) — removes the standalone mask_db launch.
  // inv_n: scale on the correct-count output (pass 1/B to get the MEAN
  // accuracy straight out of the kernel; default 1.0 = raw count)
  CHECK_CUDA(logits); CHECK_BF16(logits); CHECK_CONTIG(logits);
  TORCH_CHECK(labels.scalar_type() == at::kLong, "labels must be int64");
  CHECK_CONTIG(labels);
  int B = logits.size(0), C = logits.size(1);
  TORCH_CHECK(C <= 16, "softmax_xent kernel supports C<=16");
  TORCH_CHECK(B <= 256 * SOFTMAX_MAX_BLOCKS, "softmax_xent: batch too large");
  auto dl = torch::empty_like(logits);
  // the kernel STORES both outputs (last-block reduction), so no zero-fill
  // launch per step.  Its workspace (per-block partials + ticket counter)
  // is allocated and zeroed once per device; the counter resets itself.
  auto out = torch::empty({2}, logits.options().dtype(at::kFloat));
  float* part = softmax_workspace(logits, cur_stream());
  unsigned* ticket = reinterpret_cast<unsigned*>(part + 2 * SOFTMAX_MAX_BLOCKS);
  float* dbp = nullptr;
  if (db_out.has_value() && db_out->defined())
    dbp = db_out->data_ptr<float>();
  if (det_on() && dbp && B > 0) {
    // deterministic mode: one [C] plane of column sums per block
    auto s = cur_stream();
    int blocks = softmax_xent_blocks(B);
    float* planes = det_region(DET_SOFTMAX_DB, logits, C, blocks, s,
                               "softmax_xent_fwd", "lower the batch size");
    launch_softmax_xent_det(bf16_ptr(logits), labels.data_ptr<long>(),
                            bf16_mut(dl), out.data_ptr<float>(), B, C, planes,
                            (float)inv_n, part, ticket, s);
    reduce_planes(planes, dbp, C, C, blocks, s);
  } else {
    launch_softmax_xent(bf16_ptr(logits), labels.data_ptr<long>(),
                        bf16_mut(dl), out.data_ptr<float>(), B, C, dbp,
                        (float)inv_n, part, ticket, cur_stream());
  }
  auto loss = out.select(0, 0);
  auto correct = out.select(0, 1);
  return {loss, correct, dl};
}

// Rows per block of the fused fc2 head, by batch size (solo sweep,
// profiles/fc2_head_b1024_b8192.md); DMNIST_FC2_R=16|32|64 (read per call)
// forces one.
int fc2_head_rows(int B) {
  if (const char* e = getenv("DMNIST_FC2_R")) {
    int r = atoi(e);
    if (r == 16 || r == 32 || r == 64) return r;
  }
  // 64 rows per block from B = 256 up (fewest dW2 / db1 flushes: the kernel's
  // cost above B = 1024 is its fp32 atomics, 5632 per block); at B = 64 two
  // blocks of 32 beat one of 64.  The edge sits between the measured sizes.
  return B < 160 ? 32 : 64;
}

// The 512 -> 10 layer of the training step: fc2 forward, softmax-xent (+db2),
// fc2 dW and fc2 dX with the fc1 mask (+db1).  Returns (loss, acc, dyeff1);
// dw2_out / db2_out / db1_out are accumulated into.  THE route decision of
// this layer: one fc2_head_kernel launch, or the four separate steps when
// DMNIST_FC2_FUSED=0 (read per call), in deterministic mode (its planes route
// stays as it is) and for every shape or alignment the kernel does not cover.
std::vector<torch::Tensor> fc2_head(torch::Tensor a1, torch::Tensor w2,
                                    torch::Tensor w2T, torch::Tensor b2,
                                    torch::Tensor labels,
                                    torch::Tensor dw2_out,
                                    torch::Tensor db2_out,
                                    torch::Tensor db1_out, double p_keep,
                                    double inv_n) {
  CHECK_CUDA(a1); CHECK_BF16(a1); CHECK_CONTIG(a1);
  CHECK_BF16(w2); CHECK_CONTIG(w2);
  CHECK_BF16(w2T); CHECK_CONTIG(w2T);
  CHECK_F32(b2); CHECK_CONTIG(b2);
  TORCH_CHECK(labels.scalar_type() == at::kLong, "labels must be int64");
  CHECK_CONTIG(labels);
  CHECK_F32(dw2_out); CHECK_CONTIG(dw2_out);
  CHECK_F32(db2_out); CHECK_CONTIG(db2_out);
  CHECK_F32(db1_out); CHECK_CONTIG(db1_out);
  TORCH_CHECK(a1.dim() == 2 && w2.dim() == 2 && w2T.dim() == 2,
              "fc2_head: a1, w2 and w2T are 2-D");
  const int64_t B = a1.size(0), K = a1.size(1), C = w2.size(1);
  TORCH_CHECK(w2.size(0) == K, "fc2_head: w2 is [K][C]");
  TORCH_CHECK(w2T.size(0) == C && w2T.size(1) == K, "fc2_head: w2T is [C][K]");
  TORCH_CHECK(b2.numel() == C && db2_out.numel() == C,
              "fc2_head: b2 and db2_out hold C values");
  TORCH_CHECK(dw2_out.numel() == K * C, "fc2_head: dw2_out holds K*C values");
  TORCH_CHECK(db1_out.numel() == K, "fc2_head: db1_out holds K values");
  TORCH_CHECK(labels.numel() == B, "fc2_head: one label per row");
  TORCH_CHECK(p_keep > 0.0 && p_keep <= 1.0, "fc2_head: p_keep in (0, 1]");
  TORCH_CHECK(B <= 256 * SOFTMAX_MAX_BLOCKS, "fc2_head: batch too large");
  auto s = cur_stream();

  const char* fe = getenv("DMNIST_FC2_FUSED");
  const int R = fc2_head_rows((int)B);
  const bool fused =
      !(fe && atoi(fe) == 0) && !det_on() && B > 0 && C == 10 &&
      K == FC2_HEAD_K &&
      fc2_head_blocks((int)B, R) <= SOFTMAX_MAX_BLOCKS &&
      ((uintptr_t)a1.data_ptr() & 15) == 0 &&
      ((uintptr_t)w2T.data_ptr() & 15) == 0;
  if (!fused) {
    auto logits = linear_act_fwd_impl(a1, w2, b2, false, 1.0, 0, 0, nullptr,
                                      w2T);
    auto sm = softmax_xent_fwd(logits, labels, db2_out, inv_n);
    linear_dw_step(a1, sm[2], dw2_out.data_ptr(), s);
    auto dyeff1 = linear_dx_mask(sm[2], w2, a1, db1_out, p_keep);
    return {sm[0], sm[1], dyeff1};
  }
  auto dyeff1 = torch::empty_like(a1);
  TORCH_CHECK(((uintptr_t)dyeff1.data_ptr() & 15) == 0,
              "fc2_head: dyeff1 must be 16-byte aligned");
  auto out = torch::empty({2}, a1.options().dtype(at::kFloat));
  float* part = softmax_workspace(a1, s);
  unsigned* ticket = reinterpret_cast<unsigned*>(part + 2 * SOFTMAX_MAX_BLOCKS);
  launch_fc2_head(R, bf16_ptr(a1), bf16_ptr(w2T), b2.data_ptr<float>(),
                  labels.data_ptr<long>(), bf16_mut(dyeff1),
                  dw2_out.data_ptr<float>(), db2_out.data_ptr<float>(),
                  db1_out.data_ptr<float>(), out.data_ptr<float>(), (int)B,
                  (float)(1.0 / p_keep), (float)inv_n, part, ticket, s);
  return {out.select(0, 0), out.select(0, 1), dyeff1};
}

// optional moving-average buffer of the SGD pass: nullptr = off
static float* ema_ptr(const c10::optional<torch::Tensor>& ema,
                      const torch::Tensor& master, double ema_decay) {
  if (!ema.has_value() || !ema->defined()) return nullptr;
  CHECK_CUDA((*ema)); CHECK_F32((*ema)); CHECK_CONTIG((*ema));
  TORCH_CHECK(ema->numel() >= master.numel(),
              "sgd_step: ema is shorter than master");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(ema->data_ptr()) % 16 == 0,
              "sgd_step: ema must be 16-byte aligned");
  TORCH_CHECK(ema_decay >= 0.0 && ema_decay < 1.0,
              "sgd_step: ema_decay must lie in [0, 1)");
  return ema->data_ptr<float>();
}

// optional momentum buffer of the SGD pass: nullptr = plain SGD
static float* momentum_ptr(const c10::optional<torch::Tensor>& momentum) {
  if (!momentum.has_value() || !momentum->defined()) return nullptr;
  CHECK_F32((*momentum)); CHECK_CONTIG((*momentum));
  return momentum->data_ptr<float>();
}

// optional clip coefficient of the SGD pass (grad_norm's stats[1:2], read on
// the device): nullptr = the pass without clipping
static const float* clip_coef_ptr(const c10::optional<torch::Tensor>& coef,
                                  const torch::Tensor& master) {
  if (!coef.has_value() || !coef->defined()) return nullptr;
  CHECK_CUDA((*coef)); CHECK_F32((*coef));
  TORCH_CHECK(coef->numel() == 1 && coef->get_device() == master.get_device(),
              "sgd_step: clip_coef is one fp32 value on master's device");
  return coef->data_ptr<float>();
}

void sgd_step(torch::Tensor master, torch::Tensor grad, torch::Tensor shadow,
              bool has_shadow, double lr, double scale, double dc_keep,
              int64_t seed, int64_t offset,
              c10::optional<torch::Tensor> momentum, double mu,
              c10::optional<torch::Tensor> ema, double ema_decay,
              c10::optional<torch::Tensor> clip_coef) {
  CHECK_CUDA(master); CHECK_F32(master); CHECK_CONTIG(master);
  CHECK_F32(grad); CHECK_CONTIG(grad);
  float* mom = momentum_ptr(momentum);
  float* emap = ema_ptr(ema, master, ema_decay);
  launch_sgd_step(master.data_ptr<float>(), grad.data_ptr<float>(),
                  has_shadow ? bf16_mut(shadow) : nullptr,
                  has_shadow ? 1 : 0, master.numel(),
                  (float)(lr * scale), (float)dc_keep, (uint64_t)seed,
                  (uint64_t)offset, mom, (float)mu, emap, (float)ema_decay,
                  clip_coef_ptr(clip_coef, master), cur_stream());
}

void sgd_step_dev(torch::Tensor master, torch::Tensor grad,
                  torch::Tensor shadow, bool has_shadow,
                  torch::Tensor lr_scale_dev, double dc_keep, int64_t seed,
                  torch::Tensor offset_dev,
                  c10::optional<torch::Tensor> momentum, double mu,
                  bool zero_grad, c10::optional<torch::Tensor> ema,
                  double ema_decay, c10::optional<torch::Tensor> clip_coef) {
  CHECK_CUDA(master); CHECK_F32(master); CHECK_CONTIG(master);
  CHECK_F32(grad); CHECK_CONTIG(grad);
  CHECK_F32(lr_scale_dev);
  float* mom = momentum_ptr(momentum);  // same fp32 + contiguity checks
  launch_sgd_step_dev(master.data_ptr<float>(), grad.data_ptr<float>(),
                      has_shadow ? bf16_mut(shadow) : nullptr,
                      has_shadow ? 1 : 0, master.numel(),
                      lr_scale_dev.data_ptr<float>(), (float)dc_keep,
                      (uint64_t)seed, offset_dev.data_ptr<long>(),
                      mom, (float)mu, zero_grad ? 1 : 0,
                      ema_ptr(ema, master, ema_decay), (float)ema_decay,
                      clip_coef_ptr(clip_coef, master), cur_stream());
}

// Per-tensor and global gradient norms + the clip coefficient of the flat
// fp32 bucket, on the device (grad_norm.hip).  offsets/numels: the tensors of
// FlatParams; they must tile [0, grad.numel()) in order.
void grad_norm(torch::Tensor grad, std::vector<int64_t> offsets,
               std::vector<int64_t> numels, double grad_scale, double clip,
               torch::Tensor stats, torch::Tensor clipped_steps) {
  CHECK_CUDA(grad); CHECK_F32(grad); CHECK_CONTIG(grad);
  CHECK_CUDA(stats); CHECK_F32(stats); CHECK_CONTIG(stats);
  CHECK_CUDA(clipped_steps); CHECK_CONTIG(clipped_steps);
  TORCH_CHECK(clipped_steps.scalar_type() == at::kLong &&
              clipped_steps.numel() == 1,
              "grad_norm: clipped_steps is one int64");
  const int64_t n = grad.numel();
  const size_t ns = offsets.size();
  TORCH_CHECK(n >= 1, "grad_norm: empty gradient");
  TORCH_CHECK(ns >= 1 && ns <= GRAD_NORM_MAX_SEGS && numels.size() == ns,
              "grad_norm: 1 to ", GRAD_NORM_MAX_SEGS,
              " segments, one length per offset");
  TORCH_CHECK(stats.numel() == (int64_t)(2 + ns),
              "grad_norm: stats holds 2 + segments values");
  TORCH_CHECK(stats.get_device() == grad.get_device() &&
              clipped_steps.get_device() == grad.get_device(),
              "grad_norm: stats and clipped_steps live on grad's device");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(grad.data_ptr()) % 16 == 0,
              "grad_norm: grad must be 16-byte aligned");
  TORCH_CHECK(clip > 0.0, "grad_norm: clip must be > 0 (inf = never clip)");
  TORCH_CHECK(grad_scale > 0.0 && std::isfinite(grad_scale),
              "grad_norm: grad_scale must be finite and > 0");
  GradNormSegs segs{};
  int64_t at = 0;
  for (size_t i = 0; i < ns; ++i) {
    TORCH_CHECK(offsets[i] == at && numels[i] >= 0,
                "grad_norm: the segments must tile [0, n) in order");
    segs.off[i] = offsets[i];
    segs.len[i] = numels[i];
    at += numels[i];
  }
  TORCH_CHECK(at == n, "grad_norm: the segments must tile [0, n) in order");
  segs.n = (int)ns;
  auto s = cur_stream();
  static auto* ws = new WorkspaceSlots(64);
  float* part = device_workspace(
      *ws, grad, GRAD_NORM_MAX_SEGS * GRAD_NORM_MAX_BLOCKS + 1, at::kFloat, s,
      "grad_norm",
      "grad_norm: first call on a device allocates its workspace and must "
      "run outside graph capture").data_ptr<float>();
  unsigned* ticket = reinterpret_cast<unsigned*>(
      part + GRAD_NORM_MAX_SEGS * GRAD_NORM_MAX_BLOCKS);
  launch_grad_norm(grad.data_ptr<float>(), n, segs, (float)grad_scale,
                   (float)clip, stats.data_ptr<float>(),
                   clipped_steps.data_ptr<long>(), part, ticket, s);
}

void ema_publish(torch::Tensor ema, torch::Tensor shadow,
                 std::vector<int64_t> offsets, std::vector<int64_t> rows,
                 std::vector<int64_t> cols, std::vector<torch::Tensor> dsts) {
  // flat fp32 parameters -> flat bf16 shadow + the transposed bf16 copies
  // dsts[i] [C][R] of the row-major [R][C] slice at offsets[i]; one launch
  CHECK_CUDA(ema); CHECK_F32(ema); CHECK_CONTIG(ema);
  CHECK_CUDA(shadow); CHECK_BF16(shadow); CHECK_CONTIG(shadow);
  TORCH_CHECK(shadow.numel() == ema.numel(), "ema_publish: shadow size");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(ema.data_ptr()) % 16 == 0 &&
              reinterpret_cast<uintptr_t>(shadow.data_ptr()) % 8 == 0,
              "ema_publish: ema must be 16-byte and shadow 8-byte aligned");
  size_t nt = dsts.size();
  TORCH_CHECK(nt <= 4 && offsets.size() == nt && rows.size() == nt &&
              cols.size() == nt, "ema_publish: up to 4 transposed tensors");
  EmaTransposeDesc d[4];
  for (size_t i = 0; i < nt; ++i) {
    CHECK_CUDA(dsts[i]); CHECK_BF16(dsts[i]); CHECK_CONTIG(dsts[i]);
    TORCH_CHECK(rows[i] > 0 && cols[i] > 0 && offsets[i] >= 0 &&
                rows[i] * cols[i] <= ema.numel() - offsets[i],
                "ema_publish: slice ", i, " lies outside the buffer");
    TORCH_CHECK(dsts[i].numel() == rows[i] * cols[i],
                "ema_publish: transposed copy ", i, " has the wrong size");
    d[i] = {(long)offsets[i], bf16_mut(dsts[i]), (int)rows[i], (int)cols[i]};
  }
  launch_ema_publish(ema.data_ptr<float>(), bf16_mut(shadow), ema.numel(), d,
                     (int)nt, cur_stream());
}

// checks up to 4 (src [R][C], dst [C][R]) bf16 pairs and fills their
// descriptors; returns the pair count
static int fill_transposes(TransposeDesc (&d)[4],
                           std::vector<torch::Tensor>& srcs,
                           std::vector<torch::Tensor>& dsts) {
  TORCH_CHECK(srcs.size() == dsts.size() && srcs.size() <= 4,
              "up to 4 transpose pairs");
  for (size_t i = 0; i < srcs.size(); ++i) {
    CHECK_BF16(srcs[i]); CHECK_CONTIG(srcs[i]);
    CHECK_BF16(dsts[i]); CHECK_CONTIG(dsts[i]);
    d[i] = {bf16_ptr(srcs[i]), bf16_mut(dsts[i]),
            (int)srcs[i].size(0), (int)srcs[i].size(1)};
  }
  return (int)srcs.size();
}

void transpose_bf16_batch(std::vector<torch::Tensor> srcs,
                          std::vector<torch::Tensor> dsts) {
  TransposeDesc d[4];
  int n = fill_transposes(d, srcs, dsts);
  launch_transpose_bf16_batch(d, n, cur_stream());
}

void transpose_bf16_batch_adv(std::vector<torch::Tensor> srcs,
                              std::vector<torch::Tensor> dsts,
                              torch::Tensor step_dev,
                              torch::Tensor lr_scale_dev, double lr0,
                              double decay, int64_t decay_steps,
                              double inv_contrib) {
  // graph-tail variant: the batched transposes + the device step/LR
  // advance in ONE dispatch (step_advance folded into the last launch)
  TransposeDesc d[4];
  int n = fill_transposes(d, srcs, dsts);  // pair count, bf16, contiguity
  launch_transpose_bf16_batch_adv(
      d, n, step_dev.data_ptr<long>(),
      lr_scale_dev.data_ptr<float>(), (float)lr0, (float)decay,
      (int)decay_steps, (float)inv_contrib, cur_stream());
}

void transpose_bf16(torch::Tensor src, torch::Tensor dst) {
  CHECK_CUDA(src); CHECK_BF16(src); CHECK_CONTIG(src);
  CHECK_BF16(dst); CHECK_CONTIG(dst);
  TORCH_CHECK(src.dim() == 2 && dst.size(0) == src.size(1) &&
              dst.size(1) == src.size(0), "transpose shape mismatch");
  launch_transpose_bf16(bf16_ptr(src), bf16_mut(dst), src.size(0),
                        src.size(1), cur_stream());
}

void step_advance(torch::Tensor step_dev, torch::Tensor lr_scale_dev,
                  double lr0, double decay, int64_t decay_steps,
                  double inv_contrib) {
  launch_step_advance(step_dev.data_ptr<long>(),
                      lr_scale_dev.data_ptr<float>(), (float)lr0,
                      (float)decay, (int)decay_steps, (float)inv_contrib,
                      cur_stream());
}

void grad_mask(torch::Tensor g, double keep, int64_t seed, int64_t step,
               int64_t rank, int64_t base,
               c10::optional<torch::Tensor> step_dev) {
  CHECK_CUDA(g); CHECK_F32(g); CHECK_CONTIG(g);
  TORCH_CHECK(base % 4 == 0,
              "grad_mask: slice base must be 16B-aligned so slice-wise "
              "masks compose to the whole-buffer mask");
  const long* sd = nullptr;
  if (step_dev.has_value() && step_dev->defined())
    sd = step_dev->data_ptr<long>();
  launch_grad_mask(g.data_ptr<float>(), g.numel(), base, (float)keep,
                   (uint64_t)seed, (uint64_t)step, (uint64_t)rank, sd,
                   cur_stream());
}

// Argument checks shared by the three gathers of the device-resident uint8
// set.  `op` prefixes every message; `pos` names the host position argument
// ("step" / "start") whose device form is `pos_dev`.  A batch drawn from the
// epoch permutation needs B <= N; a sequential chunk may run past N (the rows
// past N are padding), so it sets chunk.  sd is the device position, or
// nullptr when the host value is used.
struct GatherArgs { int64_t N, B; const long* sd; };
static GatherArgs check_gather(const char* op, const torch::Tensor& img_u8,
                               const torch::Tensor& lab_u8,
                               const torch::Tensor& lut,
                               const torch::Tensor& x, const torch::Tensor& y,
                               const char* pos, int64_t pos_host,
                               const c10::optional<torch::Tensor>& pos_dev,
                               bool chunk) {
  CHECK_CUDA(img_u8); CHECK_CONTIG(img_u8);
  CHECK_CUDA(lab_u8); CHECK_CONTIG(lab_u8);
  CHECK_CUDA(lut); CHECK_BF16(lut); CHECK_CONTIG(lut);
  CHECK_CUDA(x); CHECK_BF16(x); CHECK_CONTIG(x);
  CHECK_CUDA(y); CHECK_CONTIG(y);
  TORCH_CHECK(img_u8.scalar_type() == at::kByte &&
              lab_u8.scalar_type() == at::kByte,
              op, ": images/labels must be uint8");
  TORCH_CHECK(y.scalar_type() == at::kLong, op, ": y must be int64");
  const int64_t N = lab_u8.numel(), B = y.numel();
  TORCH_CHECK(N >= 1 && N < (int64_t(1) << 31), op, ": N out of range");
  if (chunk) {
    TORCH_CHECK(B >= 1 && B < (int64_t(1) << 31),
                op, ": chunk size out of range");
  } else {
    TORCH_CHECK(B >= 1 && B <= N, op, ": batch size ", B,
                " must be in [1, N=", N, "]");
  }
  TORCH_CHECK(img_u8.numel() == N * 784, op, ": images must be [N,784]");
  TORCH_CHECK(x.numel() == B * 784, op, ": x must hold B*784 values");
  TORCH_CHECK(lut.numel() == 256, op, ": lut must have 256 entries");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(img_u8.data_ptr()) % 8 == 0 &&
              reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              op, ": images must be 8B- and x 16B-aligned");
  const long* sd = nullptr;
  if (pos_dev.has_value() && pos_dev->defined()) {
    TORCH_CHECK(pos_dev->is_cuda() && pos_dev->scalar_type() == at::kLong &&
                pos_dev->numel() >= 1, op, ": ", pos,
                "_dev must be a device int64 tensor");
    sd = pos_dev->data_ptr<long>();
  } else {
    TORCH_CHECK(pos_host >= 0, op, ": ", pos, " must be >= 0");
  }
  return {N, B, sd};
}

void batch_gather(torch::Tensor img_u8, torch::Tensor lab_u8,
                  torch::Tensor lut, torch::Tensor x, torch::Tensor y,
                  int64_t seed, int64_t step,
                  c10::optional<torch::Tensor> step_dev) {
  GatherArgs a = check_gather("batch_gather", img_u8, lab_u8, lut, x, y,
                              "step", step, step_dev, false);
  launch_batch_gather(img_u8.data_ptr<uint8_t>(), lab_u8.data_ptr<uint8_t>(),
                      bf16_ptr(lut), bf16_mut(x), y.data_ptr<long>(),
                      (uint32_t)a.N, (uint32_t)a.B, (uint64_t)seed,
                      (uint64_t)step, a.sd, cur_stream());
}

void batch_gather_aug(torch::Tensor img_u8, torch::Tensor lab_u8,
                      torch::Tensor lut, torch::Tensor table, torch::Tensor x,
                      torch::Tensor y, int64_t seed, int64_t step,
                      c10::optional<torch::Tensor> step_dev) {
  CHECK_CUDA(table); CHECK_CONTIG(table);
  TORCH_CHECK(table.scalar_type() == at::kInt && table.dim() == 2 &&
              table.size(1) == 6 && table.size(0) >= 1 &&
              table.size(0) < (int64_t(1) << 31),
              "batch_gather_aug: table must be int32 [T >= 1, 6]");
  GatherArgs a = check_gather("batch_gather_aug", img_u8, lab_u8, lut, x, y,
                              "step", step, step_dev, false);
  launch_batch_gather_aug(img_u8.data_ptr<uint8_t>(),
                          lab_u8.data_ptr<uint8_t>(), bf16_ptr(lut),
                          table.data_ptr<int>(), (uint32_t)table.size(0),
                          bf16_mut(x), y.data_ptr<long>(), (uint32_t)a.N,
                          (uint32_t)a.B, (uint64_t)seed, (uint64_t)step, a.sd,
                          cur_stream());
}

void range_gather(torch::Tensor img_u8, torch::Tensor lab_u8,
                  torch::Tensor lut, torch::Tensor x, torch::Tensor y,
                  int64_t start, c10::optional<torch::Tensor> start_dev) {
  GatherArgs a = check_gather("range_gather", img_u8, lab_u8, lut, x, y,
                              "start", start, start_dev, true);
  launch_range_gather(img_u8.data_ptr<uint8_t>(), lab_u8.data_ptr<uint8_t>(),
                      bf16_ptr(lut), bf16_mut(x), y.data_ptr<long>(),
                      (uint32_t)a.N, (uint32_t)a.B, (uint64_t)start, a.sd,
                      cur_stream());
}

void softmax_eval(torch::Tensor logits, torch::Tensor labels,
                  torch::Tensor loss_sum, torch::Tensor counts,
                  c10::optional<torch::Tensor> pred,
                  c10::optional<torch::Tensor> cursor_dev) {
  CHECK_CUDA(logits); CHECK_BF16(logits); CHECK_CONTIG(logits);
  CHECK_CUDA(labels); CHECK_CONTIG(labels);
  CHECK_CUDA(loss_sum); CHECK_F32(loss_sum); CHECK_CONTIG(loss_sum);
  CHECK_CUDA(counts); CHECK_CONTIG(counts);
  TORCH_CHECK(logits.dim() == 2, "softmax_eval: logits must be [B,C]");
  TORCH_CHECK(labels.scalar_type() == at::kLong,
              "softmax_eval: labels must be int64");
  TORCH_CHECK(counts.scalar_type() == at::kInt,
              "softmax_eval: counts must be int32");
  const int64_t B = logits.size(0), C = logits.size(1);
  TORCH_CHECK(C >= 1 && C <= 16, "softmax_eval kernel supports 1<=C<=16");
  TORCH_CHECK(B >= 1 && B <= 256 * SOFTMAX_MAX_BLOCKS,
              "softmax_eval: batch out of range");
  TORCH_CHECK(labels.numel() == B, "softmax_eval: labels must be [B]");
  TORCH_CHECK(loss_sum.numel() >= 1, "softmax_eval: loss_sum must be [1]");
  TORCH_CHECK(counts.numel() == 2 + C * C,
              "softmax_eval: counts must hold 2 + C*C = ", 2 + C * C,
              " values");
  uint8_t* pp = nullptr;
  if (pred.has_value() && pred->defined()) {
    TORCH_CHECK(pred->is_cuda() && pred->scalar_type() == at::kByte &&
                pred->is_contiguous() && pred->numel() == B,
                "softmax_eval: pred must be a contiguous device uint8 [B]");
    pp = pred->data_ptr<uint8_t>();
  }
  long* cp = nullptr;
  if (cursor_dev.has_value() && cursor_dev->defined()) {
    TORCH_CHECK(cursor_dev->is_cuda() &&
                cursor_dev->scalar_type() == at::kLong &&
                cursor_dev->numel() >= 1, "softmax_eval: cursor_dev must be "
                "a device int64 tensor");
    cp = cursor_dev->data_ptr<long>();
  }
  // the kernel's own partial/ticket workspace (never the training
  // softmax's), allocated and zeroed once per device; the counter resets
  // itself
  static auto* ws = new WorkspaceSlots(64);
  float* part = device_workspace(
      *ws, logits, SOFTMAX_MAX_BLOCKS + 1, at::kFloat, cur_stream(),
      "softmax_eval",
      "softmax_eval: first call on a device allocates its "
      "workspace and must run outside graph capture").data_ptr<float>();
  unsigned* ticket = reinterpret_cast<unsigned*>(part + SOFTMAX_MAX_BLOCKS);
  launch_softmax_eval(bf16_ptr(logits), labels.data_ptr<long>(),
                      loss_sum.data_ptr<float>(), counts.data_ptr<int>(), pp,
                      cp, (int)B, (int)C, part, ticket, cur_stream());
}

void plane_reduce(torch::Tensor planes, torch::Tensor out) {
  // out[i] += ((p_0[i] + p_1[i]) + ...) + p_{P-1}[i], fp32, planes in index
  // order; out may be any contiguous 1-D view (16 B alignment not required)
  CHECK_CUDA(planes); CHECK_F32(planes); CHECK_CONTIG(planes);
  CHECK_CUDA(out); CHECK_F32(out); CHECK_CONTIG(out);
  TORCH_CHECK(planes.dim() == 2 && planes.size(0) >= 1,
              "plane_reduce: planes must be [P >= 1, n]");
  TORCH_CHECK(out.numel() == planes.size(1),
              "plane_reduce: out must hold n = planes.size(1) values");
  TORCH_CHECK(planes.size(0) < (int64_t(1) << 31), "plane_reduce: P too large");
  TORCH_CHECK(planes.get_device() == out.get_device(),
              "plane_reduce: planes and out on different devices");
  if (out.numel() == 0) return;
  reduce_planes(planes.data_ptr<float>(), out.data_ptr<float>(), out.numel(),
                planes.size(1), (int)planes.size(0), cur_stream());
}

std::vector<torch::Tensor> det_workspace() {
  int dev = -1;
  hipGetDevice(&dev);
  std::vector<torch::Tensor> r;
  for (auto& kv : det_regions())
    if (std::get<0>(kv.first) == dev) r.push_back(kv.second);
  return r;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("set_deterministic", [](bool on) { g_deterministic.store(on); },
        "deterministic mode: gradient ops store per-block planes and reduce "
        "them in a fixed order; uncovered routes raise", py::arg("on"));
  m.def("get_deterministic", [] { return det_on(); });
  m.def("det_workspace", &det_workspace,
        "plane workspace tensors currently allocated on the current device");
  m.def("plane_reduce", &plane_reduce,
        "out[i] += ((p_0[i] + p_1[i]) + ...) + p_{P-1}[i] (fp32, index order)",
        py::arg("planes"), py::arg("out"));
  m.def("linear_act_fwd", &linear_act_fwd, "fused linear+bias+relu+dropout",
        py::arg("x"), py::arg("w"), py::arg("b"), py::arg("relu"),
        py::arg("p_keep"), py::arg("seed"), py::arg("offset"),
        py::arg("wT") = c10::nullopt);
  m.def("transpose_bf16", &transpose_bf16, "bf16 2-D transpose (wT refresh)");
  m.def("transpose_bf16_batch_adv", &transpose_bf16_batch_adv,
        "batched transposes + fused device step/LR advance (graph tail)");
  m.def("transpose_bf16_batch", &transpose_bf16_batch,
        "up to 4 transposes in one launch");
  m.def("mask_db", &mask_db, "relu/dropout grad mask + bias-grad column sums");
  m.def("linear_dw_into", &linear_dw_into, "dW = x^T dyeff into bucket view");
  m.def("linear_dx", &linear_dx, "dx = dyeff @ W^T");
  m.def("linear_dx_mask", &linear_dx_mask,
        "dx GEMM with fused relu/dropout mask + bias-grad column sums",
        py::arg("dyeff"), py::arg("w"), py::arg("actm"), py::arg("db_out"),
        py::arg("p_keep"));
  m.def("linear_dx_unpool", &linear_dx_unpool,
        "dx GEMM fused with maxpool2x2 backward scatter + conv db",
        py::arg("dyeff"), py::arg("w"), py::arg("amax"),
        py::arg("db_out"), py::arg("Ho"), py::arg("Wo"), py::arg("C"));
  m.def("linear_dx_pooled", &linear_dx_pooled,
        "dx GEMM masked by the pool argmax byte + conv db: pooled gradient",
        py::arg("dyeff"), py::arg("w"), py::arg("amax"),
        py::arg("db_out"), py::arg("Ho"), py::arg("Wo"), py::arg("C"),
        py::arg("tile") = 0);
  m.def("linear_dx_pooled_tile", [](int64_t B, int64_t K) {
          return (int64_t)(cdiv((int)B, 128) * cdiv((int)K, 128) >=
                                   POOLED_DX_BIG_TILES ? 128 : 64);
        }, "tile linear_dx_pooled picks for dyeff[B,*], w[K,*]");
  m.def("conv_dx_pooled", &conv_dx_pooled,
        "conv2 dX from the pooled gradient + pool argmax bytes",
        py::arg("gp"), py::arg("am"), py::arg("w"), py::arg("Cin"),
        py::arg("force_db") = 0);
  m.def("conv_dw_pooled_into", &conv_dw_pooled_into,
        "conv2 dW from the pooled gradient + pool argmax bytes, into bucket",
        py::arg("x"), py::arg("gp"), py::arg("am"), py::arg("dw_out"));
  m.def("linear_dw_plan", [](int64_t K, int64_t N, int64_t B) {
    DwPlan pl = linear_dw_plan((int)K, (int)N, (int)B);
    return std::make_tuple(pl.tbm, pl.bn, pl.splitk);
  }, "(tbm, bn, splitk) the fc dW launcher picks for x[B,K], dyeff[B,N]");
  m.def("pool_scatter", &pool_scatter, "maxpool bwd scatter + conv db");
  m.def("conv_dw_into", &conv_dw_into, "conv dW into bucket view");
  m.def("conv1_dw_pooled", &conv1_dw_pooled,
        "conv1 dW+db from the pooled gradient (pool bwd fused, no dact1)",
        py::arg("x"), py::arg("dyp"), py::arg("am"),
        py::arg("dw_out"), py::arg("db_out"));
  m.def("conv1_dw_group", [](int64_t NB) {
          return (int64_t)conv1_mfma_dw_group((int)NB);
        }, "images per block the MFMA conv1 dW launcher picks for batch NB");
  m.def("conv2_dw_group", [](int64_t NB) {
          return (int64_t)conv2_dw_group((int)NB);
        }, "images per block the slab conv2 dW launcher picks for batch NB");
  m.def("conv_dx", &conv_dx, "conv dX");
  m.def("linear_act_bwd", &linear_act_bwd, "linear backward (dx, dw, db)");
  m.def("linear_act_bwd_into", &linear_act_bwd_into,
        "linear backward accumulating dw/db into bucket views");
  m.def("conv_pool_fwd", &conv_pool_fwd, "fused conv5x5+bias+relu+maxpool",
        py::arg("x"), py::arg("w"), py::arg("b"), py::arg("wT") = c10::nullopt);
  m.def("conv_pool_bwd", &conv_pool_bwd, "conv+pool backward (dx, dw, db)");
  m.def("conv_pool_bwd_into", &conv_pool_bwd_into,
        "conv backward accumulating dw/db into bucket views");
  m.def("softmax_xent_fwd", &softmax_xent_fwd, "fused softmax-CE (+grad, +optional fc2 db, +optional acc-mean scale)",
        py::arg("logits"), py::arg("labels"),
        py::arg("db_out") = c10::nullopt, py::arg("inv_n") = 1.0);
  m.def("fc2_head", &fc2_head,
        "fc2 forward + softmax-xent (+db2) + fc2 dW + fc2 dX with the fc1 "
        "mask (+db1): one launch, or the four separate steps; returns "
        "(loss, acc, dyeff1)",
        py::arg("a1"), py::arg("w2"), py::arg("w2T"), py::arg("b2"),
        py::arg("labels"), py::arg("dw2_out"), py::arg("db2_out"),
        py::arg("db1_out"), py::arg("p_keep"), py::arg("inv_n") = 1.0);
  m.def("fc2_head_rows", [](int64_t B) { return fc2_head_rows((int)B); },
        "rows per block the fused fc2 head picks at batch size B");
  m.def("sgd_step", &sgd_step, "fused flat SGD(+momentum) apply",
        py::arg("master"), py::arg("grad"), py::arg("shadow"),
        py::arg("has_shadow"), py::arg("lr"), py::arg("scale"),
        py::arg("dc_keep"), py::arg("seed"), py::arg("offset"),
        py::arg("momentum") = c10::nullopt, py::arg("mu") = 0.0,
        py::arg("ema") = c10::nullopt, py::arg("ema_decay") = 0.0,
        py::arg("clip_coef") = c10::nullopt);
  m.def("grad_norm", &grad_norm,
        "stats[0] = grad_scale * |grad|, stats[1] = min(1, clip / (stats[0] "
        "+ 1e-6)), stats[2 + s] = grad_scale * |segment s|; clipped_steps "
        "+= 1 when stats[1] < 1; one launch, no float atomics",
        py::arg("grad"), py::arg("offsets"), py::arg("numels"),
        py::arg("grad_scale"), py::arg("clip"), py::arg("stats"),
        py::arg("clipped_steps"));
  m.def("grad_norm_plan", [](int64_t n) {
          TORCH_CHECK(n >= 1, "grad_norm_plan: n must be >= 1");
          int blocks, chain;
          grad_norm_plan((long)n, &blocks, &chain);
          return std::make_tuple(blocks, chain);
        }, "(blocks, chain) of grad_norm on n elements: the grid, and the "
        "longest run of fp32 additions any element passes through");
  m.def("ema_publish", &ema_publish,
        "flat fp32 parameters -> flat bf16 shadow + transposed bf16 copies "
        "of the [rows][cols] slices at `offsets`, one launch",
        py::arg("ema"), py::arg("shadow"), py::arg("offsets"),
        py::arg("rows"), py::arg("cols"), py::arg("dsts"));
  m.def("sgd_step_dev", &sgd_step_dev,
        "SGD apply with device-side lr/offset (hipGraph-capturable); "
        "zero_grad clears the bucket in the same pass",
        py::arg("master"), py::arg("grad"), py::arg("shadow"),
        py::arg("has_shadow"), py::arg("lr_scale_dev"), py::arg("dc_keep"),
        py::arg("seed"), py::arg("offset_dev"),
        py::arg("momentum") = c10::nullopt, py::arg("mu") = 0.0,
        py::arg("zero_grad") = false,
        py::arg("ema") = c10::nullopt, py::arg("ema_decay") = 0.0,
        py::arg("clip_coef") = c10::nullopt);
  m.def("step_advance", &step_advance,
        "device-side staircase LR + step increment (inside the graph)");
  m.def("grad_mask", &grad_mask,
        "per-rank pre-aggregation drop-connect mask (in-place, philox; "
        "reference distributed_train.py:194-203)",
        py::arg("g"), py::arg("keep"), py::arg("seed"), py::arg("step"),
        py::arg("rank"), py::arg("base") = 0,
        py::arg("step_dev") = c10::nullopt);
  m.def("batch_gather", &batch_gather,
        "gather one training batch from the device-resident uint8 set "
        "(Feistel epoch permutation keyed on seed + step; LUT-normalised "
        "to bf16) into x [B,28,28,1] bf16 / y [B] int64",
        py::arg("img_u8"), py::arg("lab_u8"), py::arg("lut"), py::arg("x"),
        py::arg("y"), py::arg("seed"), py::arg("step"),
        py::arg("step_dev") = c10::nullopt);
  m.def("batch_gather_aug", &batch_gather_aug,
        "batch_gather with on-device affine augmentation: image j is warped "
        "(integer bilinear, zero background) by row aug_indices(seed, step, "
        "j) of the int32 [T,6] Q16 inverse-affine table before the LUT",
        py::arg("img_u8"), py::arg("lab_u8"), py::arg("lut"),
        py::arg("table"), py::arg("x"), py::arg("y"), py::arg("seed"),
        py::arg("step"), py::arg("step_dev") = c10::nullopt);
  m.def("range_gather", &range_gather,
        "sequential chunk [start, start+B) of the device-resident uint8 set "
        "(LUT-normalised to bf16) into x [B,28,28,1] bf16 / y [B] int64; "
        "rows past N are zero-filled with label -1",
        py::arg("img_u8"), py::arg("lab_u8"), py::arg("lut"), py::arg("x"),
        py::arg("y"), py::arg("start"),
        py::arg("start_dev") = c10::nullopt);
  m.def("softmax_eval", &softmax_eval,
        "evaluation statistics accumulated across launches: loss_sum[1] "
        "fp32, counts[2 + C*C] int32 (live, correct, confusion), optional "
        "pred[B] uint8 and cursor_dev += B; rows with a label outside "
        "[0, C) contribute to nothing",
        py::arg("logits"), py::arg("labels"), py::arg("loss_sum"),
        py::arg("counts"), py::arg("pred") = c10::nullopt,
        py::arg("cursor_dev") = c10::nullopt);
  m.def("linear_act_fwd_dev", &linear_act_fwd_dev,
        "linear fwd with device-side dropout offset",
        py::arg("x"), py::arg("w"), py::arg("b"), py::arg("relu"),
        py::arg("p_keep"), py::arg("seed"), py::arg("offset_dev"),
        py::arg("wT") = c10::nullopt);
}
