"""fp32 PyTorch reference implementations of every hot-path primitive.

These are (a) the CPU execution path (no GPU required — BASELINE config 1),
and (b) the numerics oracle the HIP/CDNA4 kernels are unit-tested against
(SURVEY.md section 4).  Layouts follow the reference model (TF NHWC / HWIO,
/root/reference/src/mnist.py:107-145): activations are NHWC, conv weights are
[KH, KW, Cin, Cout], fc weights are [in, out] with y = x @ W + b.

All functions are pure tensor->tensor (no autograd); autograd wiring lives in
ops/functional.py.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F


# ---------------------------------------------------------------------------
# conv 5x5 SAME + bias + ReLU + maxpool 2x2 s2, fused (fwd + bwd)
# Reference call sites: mnist.py:107-127 (conv/bias_add/relu/max_pool x2).
# ---------------------------------------------------------------------------

def conv_pool_fwd(x, w, b):
    """x: [N,H,W,Cin], w: [5,5,Cin,Cout], b: [Cout] ->
    (y: [N,H/2,W/2,Cout], argmax: [N,H/2,W/2,Cout] uint8 in 0..3)

    y = maxpool2x2(relu(conv2d_same(x, w) + b)); argmax records which of the
    2x2 window (r*2+c) won, for routing the pooled gradient back.
    """
    N, H, W, Cin = x.shape
    Cout = w.shape[3]
    xc = x.permute(0, 3, 1, 2)                       # NCHW
    wc = w.permute(3, 2, 0, 1)                       # [Cout,Cin,5,5]
    conv = F.conv2d(xc.float(), wc.float(), b.float(), padding=2)
    act = F.relu(conv)                               # [N,Cout,H,W]
    # maxpool 2x2 stride 2 with argmax
    pooled, idx = F.max_pool2d(act, 2, 2, return_indices=True)
    # idx is flat index into H*W; convert to 0..3 position within the window
    Ho, Wo = pooled.shape[2], pooled.shape[3]
    ar = torch.arange(Ho, device=x.device).view(1, 1, Ho, 1)
    ac = torch.arange(Wo, device=x.device).view(1, 1, 1, Wo)
    r = idx // W - ar * 2
    c = idx % W - ac * 2
    amax = (r * 2 + c).to(torch.uint8)               # [N,Cout,Ho,Wo]
    # liveness rides in the argmax byte (matches the HIP kernels): 7 marks
    # a dead window (relu zeroed all four) so pooled-consumer backward
    # kernels need no y read
    amax = torch.where(pooled > 0, amax,
                       torch.tensor(7, dtype=torch.uint8))
    y = pooled.permute(0, 2, 3, 1).contiguous()      # NHWC
    amax = amax.permute(0, 2, 3, 1).contiguous()
    return y, amax


def conv_pool_bwd(dy, x, w, y, amax):
    """Backward of conv_pool_fwd. Returns (dx, dw, db).

    dy, y, amax: [N,Ho,Wo,Cout]; x: [N,H,W,Cin]; w: [5,5,Cin,Cout].
    ReLU mask: the pooled max is the relu output at the argmax position, so
    grad passes iff y > 0.
    """
    N, Ho, Wo, Cout = dy.shape
    H, W = Ho * 2, Wo * 2
    Cin = x.shape[3]
    # route pooled grad (masked by relu) back to the argmax position
    g = (dy * (y > 0)).permute(0, 3, 1, 2).float()   # [N,Cout,Ho,Wo]
    # clamp the dead-window marker (7) to a valid position: its g is zero
    # by the relu mask, so the scatter target is irrelevant but must be
    # in-bounds
    am = amax.permute(0, 3, 1, 2).long().clamp(max=3)
    dact = x.new_zeros((N, Cout, H, W), dtype=torch.float32)
    ar = torch.arange(Ho, device=x.device).view(1, 1, Ho, 1)
    ac = torch.arange(Wo, device=x.device).view(1, 1, 1, Wo)
    rows = ar * 2 + am // 2
    cols = ac * 2 + am % 2
    flat = (rows * W + cols)
    dact.view(N, Cout, H * W).scatter_(2, flat.view(N, Cout, -1),
                                       g.view(N, Cout, -1))
    xc = x.permute(0, 3, 1, 2).float()               # [N,Cin,H,W]
    wc = w.permute(3, 2, 0, 1).float()               # [Cout,Cin,5,5]
    dxc = torch.nn.grad.conv2d_input(xc.shape, wc, dact, padding=2)
    dwc = torch.nn.grad.conv2d_weight(xc, wc.shape, dact, padding=2)
    db = dact.sum(dim=(0, 2, 3))
    dx = dxc.permute(0, 2, 3, 1).contiguous().to(x.dtype)
    dw = dwc.permute(2, 3, 1, 0).contiguous()        # [5,5,Cin,Cout] fp32
    return dx, dw, db


# ---------------------------------------------------------------------------
# Linear (+ bias [+ ReLU] [+ dropout]) — mnist.py:136-145
# ---------------------------------------------------------------------------

def linear_fwd(x, w, b, relu: bool = False):
    """x: [B,K], w: [K,N], b: [N] -> y: [B,N] (= relu(x@w+b) if relu)."""
    y = x.float() @ w.float() + b.float()
    if relu:
        y = F.relu(y)
    return y.to(x.dtype)


def linear_bwd(dy, x, w, y=None, relu: bool = False):
    """Returns (dx, dw fp32, db fp32). If relu, y (post-relu) masks dy."""
    dyf = dy.float()
    if relu:
        dyf = dyf * (y > 0)
    dx = (dyf @ w.float().t()).to(x.dtype)
    dw = x.float().t() @ dyf
    db = dyf.sum(dim=0)
    return dx, dw, db


def dropout_fwd(x, p_drop: float, gen: torch.Generator | None = None):
    """TF-style dropout (mnist.py:139-140): keep with prob 1-p, scale by
    1/(1-p). Returns (y, mask bool)."""
    keep = 1.0 - p_drop
    # generator lives on CPU; sample there and move (device-agnostic ref)
    mask = (torch.rand(x.shape, device="cpu", dtype=torch.float32,
                       generator=gen) < keep).to(x.device)
    y = x * mask.to(x.dtype) / keep
    return y.to(x.dtype), mask


def dropout_bwd(dy, mask, p_drop: float):
    keep = 1.0 - p_drop
    return (dy * mask.to(dy.dtype) / keep).to(dy.dtype)


# ---------------------------------------------------------------------------
# Fused softmax cross-entropy (+ accuracy): mnist.py:149-164
# ---------------------------------------------------------------------------

def softmax_xent_fwd(logits, labels):
    """logits: [B,C], labels: [B] int64.

    Returns (loss_mean fp32 scalar, correct_count fp32 scalar, dlogits
    [B,C] in logits.dtype).  dlogits = (softmax - onehot)/B — precomputed in
    the forward since the backward needs nothing else (single fused kernel on
    GPU; logsumexp trick).
    """
    lf = logits.float()
    m = lf.max(dim=1, keepdim=True).values
    z = lf - m
    ez = z.exp()
    se = ez.sum(dim=1, keepdim=True)
    logp = z - se.log()
    B = logits.shape[0]
    loss = -logp.gather(1, labels.view(-1, 1)).mean()
    p = ez / se
    dl = p
    dl.scatter_add_(1, labels.view(-1, 1), torch.full((B, 1), -1.0, device=logits.device))
    dl = (dl / B).to(logits.dtype)
    correct = (lf.argmax(dim=1) == labels).float().sum()
    return loss, correct, dl


def fc2_head(a1, w2, b2, labels, p_keep: float):
    """The fc2 layer of the training step in one piece: forward, softmax
    cross-entropy, fc2 dW and fc2 dX with the fc1 relu/dropout mask.

    a1: [B,K] post-relu/dropout activation, w2: [K,C], b2: [C], labels: [B].
    fp64 arithmetic with the GPU route's rounding points: the logits and
    dlogits are rounded to a1.dtype, db2 sums the unrounded dlogits, the mask
    is a1 > 0 and kept gradients are scaled by 1/p_keep.

    Returns (loss, correct, dyeff1 [B,K] in a1.dtype, dw2 [K,C], db1 [K],
    db2 [C]); the scalars and the three sums are fp64.
    """
    B = a1.shape[0]
    af, wf = a1.double(), w2.double()
    logits = (af @ wf + b2.double()).to(a1.dtype).double()
    z = logits - logits.max(dim=1, keepdim=True).values
    ez = z.exp()
    se = ez.sum(dim=1, keepdim=True)
    onehot = torch.zeros_like(ez).scatter_(1, labels.view(-1, 1), 1.0)
    loss = -((z - se.log()) * onehot).sum() / B
    correct = (logits.argmax(dim=1) == labels).double().sum()
    d = (ez / se - onehot) / B
    db2 = d.sum(dim=0)
    dl = d.to(a1.dtype).double()
    dw2 = af.t() @ dl
    g = (dl @ wf.t()) * (a1 > 0) / p_keep
    db1 = g.sum(dim=0)
    return loss, correct, g.to(a1.dtype), dw2, db1, db2


# ---------------------------------------------------------------------------
# Fused SGD apply (+ drop-connect): distributed_train.py:176,414-416
# ---------------------------------------------------------------------------

def sgd_step(master, grad, lr: float, grad_scale: float = 1.0,
             drop_connect_keep: float | None = None,
             gen: torch.Generator | None = None, shadow=None,
             momentum=None, mu: float = 0.0, ema=None,
             ema_decay: float = 0.0, offset: int = 0, clip_coef=None):
    """In-place w -= lr * grad_scale * (g or momentum-filtered g).

    clip_coef: optional one-element fp32 tensor (grad_norm()'s stats[1:2]);
    the gradient is multiplied by it first, before the drop-connect mask and
    before momentum: v = mu*v + coef*g.

    drop_connect_keep: if set, per-element Bernoulli(keep) mask on the grad
    (reference drop_connect: grad * mask, NO rescale —
    distributed_train.py:414-416).
    momentum/mu: optional heavyweight-ball momentum v = mu*v + g; w -= lr*v
    (the reference used plain GradientDescentOptimizer; momentum is the
    north-star's optional extension).
    shadow: optional flat low-precision copy refreshed after the update.
    ema/ema_decay/offset: optional moving average of the weights
    (TensorFlow's ExponentialMovingAverage with num_updates): update
    k = offset + 1 does e -= (1 - d_k)*(e - w_new), d_k = min(ema_decay,
    (1 + k)/(10 + k)), everything in fp32.
    """
    g = grad.float() * grad_scale
    if clip_coef is not None:
        g = g * clip_coef.float().reshape(())
    if drop_connect_keep is not None:
        mask = (torch.rand(g.shape, device=g.device, dtype=torch.float32,
                           generator=gen) < drop_connect_keep).float()
        g = g * mask
    if momentum is not None:
        momentum.mul_(mu).add_(g)
        g = momentum
    master.add_(g, alpha=-lr)
    if ema is not None:
        ema.sub_((ema - master) * ema_weight(ema_decay, offset))
    if shadow is not None:
        shadow.copy_(master.to(shadow.dtype))
    return master


def grad_norm(flat, offsets, numels, grad_scale: float, clip: float):
    """Per-tensor and global L2 norms of a flat fp32 gradient and the
    torch.nn.utils.clip_grad_norm_ coefficient -> fp32 `stats` [2 + segments]
    on flat's device, the layout of csrc/grad_norm.hip:

      stats[0]     = grad_scale * sqrt(sum of g^2)       (the global norm)
      stats[1]     = min(1, clip / (stats[0] + 1e-6))    (fp32 arithmetic)
      stats[2 + s] = grad_scale * sqrt(sum of g^2 over segment s)

    The sums of squares are taken per segment in float64 from the fp32
    values, the total is their float64 sum, the norms are rounded to fp32.
    `flat` is the SUM over contributors, grad_scale = 1 / contributors, so the
    norms are those of the averaged gradient.  The segments (offsets, numels)
    must tile [0, flat.numel()) in order; clip > 0, inf = never clip (the
    coefficient is then exactly 1)."""
    import numpy as np
    n = flat.numel()
    if flat.dtype != torch.float32 or flat.dim() != 1:
        raise ValueError("grad_norm: flat must be a 1-D fp32 tensor")
    if not (len(offsets) == len(numels) and len(offsets) >= 1):
        raise ValueError("grad_norm: one length per offset, at least one")
    at = 0
    for o, m in zip(offsets, numels):
        if o != at or m < 0:
            raise ValueError("grad_norm: the segments must tile [0, n) in "
                             "order")
        at += m
    if at != n:
        raise ValueError("grad_norm: the segments must tile [0, n) in order")
    if not clip > 0.0:  # also refuses nan
        raise ValueError(f"grad_norm: clip must be > 0, got {clip}")
    g = flat.detach().double()
    sq = [float((g[o:o + m] * g[o:o + m]).sum())
          for o, m in zip(offsets, numels)]
    total = 0.0
    for v in sq:
        total += v
    f32 = np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        norm = f32(float(grad_scale) * np.sqrt(total))
        coef = np.minimum(f32(1), f32(clip) / (norm + f32(1e-6)))
        if np.isnan(coef):
            coef = f32(1)  # fminf(1, nan)
    out = [norm, coef] + [f32(float(grad_scale) * np.sqrt(v)) for v in sq]
    return torch.tensor([float(v) for v in out], dtype=torch.float32,
                        device=flat.device)


def ema_weight(ema_decay: float, offset: int) -> float:
    """1 - d_k of update k = offset + 1, in numpy.float32 (the arithmetic
    of sgd_step_kernel_ema)."""
    if not 0.0 <= ema_decay < 1.0:
        raise ValueError(f"ema_decay must lie in [0, 1), got {ema_decay}")
    import numpy as np
    k = np.float32(int(offset) + 1)
    d = min(np.float32(ema_decay),
            (np.float32(1) + k) / (np.float32(10) + k))
    return float(np.float32(1) - d)


# ---------------------------------------------------------------------------
# Device-resident input pipeline: stateless epoch permutation + batch gather.
# Bit-exact oracle of csrc/data_gather.hip (and the CPU / fp32-on-GPU path).
# All permutation arithmetic is unsigned mod 2^32.
# ---------------------------------------------------------------------------

_M32 = 0xFFFFFFFF


def _mix32(x):
    """murmur3 finalizer on python ints or uint64 numpy arrays (values kept
    below 2^32, so the 64-bit products never overflow before masking)."""
    x = x ^ (x >> 16)
    x = (x * 0x85EBCA6B) & _M32
    x = x ^ (x >> 13)
    x = (x * 0xC2B2AE35) & _M32
    return x ^ (x >> 16)


def feistel_perm(n: int, seed: int, epoch: int, p):
    """Cycle-walking 4-round Feistel permutation of [0, n) keyed on
    (64-bit seed, epoch).  p: int array of positions in [0, n) -> int64
    array of sample indices.  Epoch 0 is the identity (first epoch
    unshuffled, as data/mnist_data.py DataSet)."""
    import numpy as np
    p = np.asarray(p, dtype=np.int64)
    if p.size and not (0 <= p.min() and p.max() < n):
        raise ValueError(f"positions must lie in [0, {n})")
    if epoch == 0:
        return p.copy()
    seed &= 0xFFFFFFFFFFFFFFFF
    base = _mix32((seed & _M32) ^ _mix32(((seed >> 32) + 0x9E3779B9) & _M32))
    keys = [_mix32((base + (epoch & _M32) * 0x9E3779B1 + r) & _M32)
            for r in range(4)]
    bits = max(2, (n - 1).bit_length())
    bits += bits & 1
    h = np.uint64(bits // 2)
    mask = np.uint64((1 << (bits // 2)) - 1)
    m32 = np.uint64(_M32)

    def enc(v):
        L, R = v >> h, v & mask
        for k in keys:
            f = _mix32((R * np.uint64(0x9E3779B1) + np.uint64(k)) & m32)
            L, R = R, L ^ (f & mask)
        return (L << h) | R

    v = enc(p.astype(np.uint64))
    out = v >= np.uint64(n)
    while out.any():
        v[out] = enc(v[out])
        out = v >= np.uint64(n)
    return v.astype(np.int64)


def batch_indices(n: int, batch_size: int, seed: int, step: int):
    """Sample indices of the batch at `step`: spe = n // B batches per epoch
    (the n % B tail is dropped, as DataSet.next_batch drops it), epoch =
    step // spe, sample j = perm(epoch, (step % spe) * B + j)."""
    import numpy as np
    if not 1 <= batch_size <= n:
        raise ValueError(f"batch size {batch_size} must be in [1, N={n}]")
    if step < 0:
        raise ValueError("step must be >= 0")
    spe = n // batch_size
    epoch, pos = divmod(int(step), spe)
    p = pos * batch_size + np.arange(batch_size, dtype=np.int64)
    return feistel_perm(n, seed, epoch, p)


# -- affine augmentation (integer only; csrc/data_gather.hip mirrors it) -----
#
# A transform table is int32 [T, 6]: rows (a00, a01, a10, a11, t0, t1) in
# Q16, the INVERSE map (output pixel -> source position) about the image
# centre (13.5, 13.5):
#
#   src_col = 13.5 + a00 (c - 13.5) + a01 (r - 13.5) + t0
#   src_row = 13.5 + a10 (c - 13.5) + a11 (r - 13.5) + t1
#
# evaluated in Q17 on the doubled coordinates uc = 2c - 27, ur = 2r - 27 so
# that the half-pixel centre stays an integer.  The bilinear weights keep 8
# fractional bits; pixels outside the image are background byte 0.

AUG_ONE = 1 << 16
AUG_IDENTITY = (AUG_ONE, 0, 0, AUG_ONE, 0, 0)
AUG_MAX_A = 4 * AUG_ONE     # |a| bound the builder guarantees
AUG_MAX_T = 64 * AUG_ONE    # |t| bound the builder guarantees
_SIDE = 28


def augment_table(T: int, seed: int, shift_px: float = 0.0,
                  rotate_deg: float = 0.0, scale_frac: float = 0.0):
    """Seeded table of T random inverse affine maps -> int32 numpy [T, 6].
    Angle uniform in +-rotate_deg, scale log-uniform in [1/(1+scale_frac),
    1+scale_frac], translation uniform real in +-shift_px per axis; each
    entry is the inverse of rotate o scale (plus the translation of the
    source position), rounded to nearest.  All-zero magnitudes give the
    identity everywhere.  Arguments that could leave |a| <= 4 or |t| <= 64
    (in pixels) are rejected: inside those bounds the Q17 coordinates of
    affine_warp_u8 cannot overflow int32."""
    import numpy as np
    T = int(T)
    if T < 1:
        raise ValueError("augment_table: T must be >= 1")
    for name, v, hi in (("shift_px", shift_px, 64.0),
                        ("rotate_deg", rotate_deg, 180.0),
                        ("scale_frac", scale_frac, 3.0)):
        if not (0.0 <= float(v) <= hi):  # NaN fails both compares
            raise ValueError(f"augment_table: {name}={v} outside [0, {hi}]")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    rng = np.random.RandomState([seed & _M32, seed >> 32, 0xA0F1])
    theta = np.deg2rad(rng.uniform(-rotate_deg, rotate_deg, size=T))
    ls = np.log1p(float(scale_frac))
    inv_s = np.exp(-rng.uniform(-ls, ls, size=T))
    t = rng.uniform(-shift_px, shift_px, size=(T, 2))
    co, si = np.cos(theta) * inv_s, np.sin(theta) * inv_s
    # inverse of s*R(theta) is (1/s)*R(-theta)
    tab = np.stack([co, si, -si, co, t[:, 0], t[:, 1]], axis=1) * AUG_ONE
    tab = np.rint(tab).astype(np.int64)
    assert np.abs(tab[:, :4]).max() <= AUG_MAX_A
    assert np.abs(tab[:, 4:]).max() <= AUG_MAX_T
    return tab.astype(np.int32)


def aug_indices(T: int, seed: int, step: int, b: int):
    """Table row of batch position j at `step` -> int64 numpy [b] in [0, T):
    a pure function of (seed, step, j) that takes the full 64-bit step.
    Keyed on the batch POSITION, not on the sample index, so an image meets
    a different transform in every epoch."""
    import numpy as np
    T, step = int(T), int(step)
    if T < 1:
        raise ValueError("aug_indices: T must be >= 1")
    if step < 0:
        raise ValueError("step must be >= 0")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    base = _mix32((seed & _M32) ^ _mix32(((seed >> 32) + 0x9E3779B9) & _M32))
    lo, hi = step & _M32, (step >> 32) & _M32
    k = _mix32((base + 0x632BE5AB + lo * 0x9E3779B1) & _M32)
    k = _mix32(k ^ _mix32((hi + 0x7F4A7C15) & _M32))
    j = np.arange(int(b), dtype=np.uint64)
    r = _mix32((np.uint64(k) + j * np.uint64(0x85EBCA6B)) & np.uint64(_M32))
    return (r % np.uint64(T)).astype(np.int64)


def affine_warp_u8(rows_u8, entries):
    """Integer bilinear warp of uint8 images.  rows_u8: [b, 784] uint8,
    entries: [b, 6] integer (one table row per image) -> uint8 [b, 784].
    Defined for entries within the builder's bounds (int64 here; the kernel's
    int32 arithmetic agrees there)."""
    b = rows_u8.shape[0]
    dev = rows_u8.device
    e = entries.to(device=dev, dtype=torch.int64).view(b, 6, 1, 1)
    u = 2 * torch.arange(_SIDE, device=dev, dtype=torch.int64) - (_SIDE - 1)
    uc, ur = u.view(1, 1, _SIDE), u.view(1, _SIDE, 1)
    half = (_SIDE - 1) * AUG_ONE
    SX = half + e[:, 0] * uc + e[:, 1] * ur + 2 * e[:, 4]
    SY = half + e[:, 2] * uc + e[:, 3] * ur + 2 * e[:, 5]
    x0, y0 = SX >> 17, SY >> 17  # arithmetic shift = floor
    fx, fy = (SX >> 9) & 255, (SY >> 9) & 255
    src = rows_u8.reshape(b, _SIDE * _SIDE).long()

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < _SIDE) & (yy >= 0) & (yy < _SIDE)
        flat = yy.clamp(0, _SIDE - 1) * _SIDE + xx.clamp(0, _SIDE - 1)
        v = src.gather(1, flat.view(b, -1)).view(b, _SIDE, _SIDE)
        return torch.where(ok, v, torch.zeros_like(v))

    top = tap(y0, x0) * (256 - fx) + tap(y0, x0 + 1) * fx
    bot = tap(y0 + 1, x0) * (256 - fx) + tap(y0 + 1, x0 + 1) * fx
    v = (top * (256 - fy) + bot * fy + 32768) >> 16
    return v.to(torch.uint8).view(b, _SIDE * _SIDE)


def batch_gather(img_u8, lab_u8, lut, x, y, seed: int, step: int,
                 aug_table=None):
    """x[j] = lut[img_u8[idx[j]]], y[j] = lab_u8[idx[j]] written into the
    caller's buffers (any device; x takes lut's dtype).  With `aug_table`
    (int32 [T, 6]) row j is warped by table entry aug_indices(...)[j]
    between the permutation and the LUT; labels are unchanged."""
    n, b = lab_u8.shape[0], y.shape[0]
    idx = torch.from_numpy(batch_indices(n, b, seed, step)).to(img_u8.device)
    rows = img_u8[idx]
    if aug_table is not None:
        if aug_table.dim() != 2 or aug_table.shape[1] != 6 \
                or aug_table.shape[0] < 1:
            raise ValueError("aug_table must be [T >= 1, 6]")
        t = torch.from_numpy(aug_indices(aug_table.shape[0], seed, step, b))
        rows = affine_warp_u8(rows.reshape(b, -1),
                              aug_table[t.to(aug_table.device)])
    x.copy_(lut[rows.long()].reshape(x.shape))
    y.copy_(lab_u8[idx].long())
    return x, y


# ---------------------------------------------------------------------------
# Device-side evaluation: sequential chunk gather + accumulated statistics.
# Oracles of csrc/eval_ops.hip (and the CPU / fp32-on-GPU path).
# ---------------------------------------------------------------------------

def range_gather(img_u8, lab_u8, lut, x, y, start: int):
    """Chunk [start, start + B) of the resident set into the caller's
    buffers: a row i < N is lut[img_u8[i]] with its label, a row past N is
    exactly zero with label -1.  start >= N is legal (all padding)."""
    n, b = lab_u8.shape[0], y.shape[0]
    start = int(start)
    if start < 0:
        raise ValueError("start must be >= 0")
    live = max(0, min(b, n - start))
    xf = x.view(b, -1)
    if live:
        xf[:live] = lut[img_u8[start:start + live].long()]
        y[:live] = lab_u8[start:start + live].long()
    if live < b:
        xf[live:] = 0
        y[live:] = -1
    return x, y


def softmax_eval(logits, labels, loss_sum, counts, pred=None,
                 cursor_dev=None):
    """Evaluation statistics of one chunk, ACCUMULATED into the running
    state: loss_sum[0] (fp32) += sum of -log softmax(logits)[label],
    counts (int32 [2 + C*C]) += (live rows, correct rows, confusion[t, p]).
    A row is live iff 0 <= label < C; every other row contributes to
    nothing.  The prediction is the LOWEST index among the maximal logits
    (not torch.argmax, whose tie order is unspecified).  pred (uint8 [B]):
    predicted class, 255 where the row is not live.  cursor_dev (int64 [1])
    advances by B."""
    B, C = logits.shape
    lf = logits.float()
    live = (labels >= 0) & (labels < C)
    mx = lf.max(dim=1, keepdim=True).values
    idx = torch.arange(C, device=logits.device).expand(B, C)
    p = torch.where(lf == mx, idx, torch.full_like(idx, C)).min(dim=1).values
    t = labels.clamp(0, C - 1)
    xl = lf.gather(1, t.view(-1, 1)).squeeze(1)
    row_loss = (lf - mx).exp().sum(dim=1).log() - (xl - mx.squeeze(1))
    loss_sum += row_loss[live].double().sum().to(loss_sum.dtype)
    tl, pl = t[live], p[live]
    counts[0] += int(live.sum())
    counts[1] += int((tl == pl).sum())
    counts[2:] += torch.bincount(tl * C + pl, minlength=C * C).to(counts.dtype)
    if pred is not None:
        pred.copy_(torch.where(live, p, torch.full_like(p, 255)).to(pred.dtype))
    if cursor_dev is not None:
        cursor_dev += B


def plane_reduce(planes, out):
    """The deterministic mode's ordered reduction, in place:
    S = ((p_0 + p_1) + p_2) + ... + p_{P-1} (fp32, planes in index order,
    starting from p_0), then out += S (one fp32 add).  A sequential loop over
    the planes; each step is one elementwise fp32 add, so no reassociation."""
    assert planes.dim() == 2 and planes.shape[0] >= 1
    assert planes.dtype == torch.float32 and out.dtype == torch.float32
    assert out.numel() == planes.shape[1]
    p = planes.detach().cpu()
    s = p[0].clone()
    for i in range(1, p.shape[0]):
        s = s + p[i]
    out += s.to(out.device).view_as(out)
    return out
