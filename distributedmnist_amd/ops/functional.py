"""Autograd wiring for the fused primitives, dispatching CPU-ref vs HIP ext.

Dispatch rule: CUDA tensors -> the in-tree HIP extension (fails loudly if the
.so is missing on a GPU box — _C.ext()); CPU tensors -> ops/cpu_ref.py fp32
reference.  Both paths share autograd semantics so the engine/ and models/
code is device-agnostic.

Mixed precision: parameters are fp32 masters; on GPU the model holds bf16
shadow copies used for compute (passed as the non-differentiable `w_comp` /
`b_comp` args).  Weight gradients are always produced in fp32 so they can
accumulate straight into the flat fp32 all-reduce bucket
(parallel/sync.py).
"""

from __future__ import annotations

import torch

from .. import _C
from . import cpu_ref


def _use_hip(t: torch.Tensor) -> bool:
    # the HIP kernels are the bf16 compute path (bf16 operands, fp32
    # epilogues); fp32-on-GPU routes to the torch reference ops (MIOpen /
    # rocBLAS) — a numerics-debug mode, never the bench path
    return t.is_cuda and t.dtype == torch.bfloat16


class ConvPoolFn(torch.autograd.Function):
    """Fused conv5x5-SAME + bias + ReLU + maxpool2x2s2 (mnist.py:107-127).

    GPU direct-grad mode: when dw_out/db_out (fp32 views into the flat
    all-reduce bucket, pre-zeroed each step) are passed, the backward
    kernels accumulate straight into them and None is returned to autograd
    for w/b — no per-param zeros() or AccumulateGrad adds on the hot path.
    """

    @staticmethod
    def forward(ctx, x, w, b, w_comp, b_comp, need_dx: bool,
                dw_out, db_out, w_t):
        if _use_hip(x):
            y, amax = _C.ext().conv_pool_fwd(x, w_comp, b_comp, w_t)
        else:
            y, amax = cpu_ref.conv_pool_fwd(x, w_comp, b_comp)
        ctx.save_for_backward(x, w_comp, y, amax)
        ctx.need_dx = need_dx
        ctx.outs = (dw_out, db_out) if (dw_out is not None and _use_hip(x)) else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w_comp, y, amax = ctx.saved_tensors
        if _use_hip(dy):
            if ctx.outs is not None:
                dw_out, db_out = ctx.outs
                dx = _C.ext().conv_pool_bwd_into(
                    dy.contiguous(), x, w_comp, y, amax, ctx.need_dx,
                    dw_out, db_out)
                dw = db = None
            else:
                dx, dw, db = _C.ext().conv_pool_bwd(
                    dy.contiguous(), x, w_comp, y, amax, ctx.need_dx)
        else:
            dx, dw, db = cpu_ref.conv_pool_bwd(dy, x, w_comp, y, amax)
        if not ctx.need_dx:
            dx = None
        return dx, dw, db, None, None, None, None, None, None


def conv_pool(x, w, b, w_comp=None, b_comp=None, need_dx=True,
              dw_out=None, db_out=None, w_t=None):
    return ConvPoolFn.apply(x, w, b, w_comp if w_comp is not None else w,
                            b_comp if b_comp is not None else b, need_dx,
                            dw_out, db_out, w_t)


class LinearActFn(torch.autograd.Function):
    """x @ W + b [+ReLU] [+TF-dropout(1-p_keep)] (mnist.py:136-145).

    Dropout is folded into the epilogue; the backward recovers BOTH the relu
    and the dropout mask from sign(y): dropped or relu-clipped positions have
    y == 0, kept positions are scaled by 1/p_keep.
    """

    @staticmethod
    def forward(ctx, x, w, b, w_comp, b_comp, relu: bool, p_keep: float,
                seed: int, offset: int, dw_out, db_out, offset_dev, w_t):
        if _use_hip(x):
            if offset_dev is not None and p_keep < 1.0:
                y = _C.ext().linear_act_fwd_dev(x, w_comp, b_comp, relu,
                                                p_keep, seed, offset_dev,
                                                wT=w_t)
            else:
                y = _C.ext().linear_act_fwd(x, w_comp, b_comp, relu, p_keep,
                                            seed, offset, wT=w_t)
        else:
            y = cpu_ref.linear_fwd(x, w_comp, b_comp, relu)
            if p_keep < 1.0:
                gen = torch.Generator(device="cpu")
                gen.manual_seed((seed * 0x9E3779B97F4A7C15 + offset) % (2**63))
                mask = (torch.rand(y.shape, generator=gen) < p_keep)
                y = y * mask.to(device=y.device, dtype=y.dtype) / p_keep
        ctx.save_for_backward(x, w_comp, y)
        ctx.relu = relu
        ctx.p_keep = p_keep
        ctx.outs = (dw_out, db_out) if (dw_out is not None and _use_hip(x)) else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w_comp, y = ctx.saved_tensors
        relu, p_keep = ctx.relu, ctx.p_keep
        if _use_hip(dy):
            if ctx.outs is not None:
                dw_out, db_out = ctx.outs
                dx = _C.ext().linear_act_bwd_into(
                    dy.contiguous(), x, w_comp, y, relu, p_keep,
                    ctx.needs_input_grad[0], dw_out, db_out)
                dw = db = None
            else:
                dx, dw, db = _C.ext().linear_act_bwd(
                    dy.contiguous(), x, w_comp, y, relu, p_keep,
                    ctx.needs_input_grad[0])
        else:
            dyf = dy.float()
            if relu or p_keep < 1.0:
                dyf = dyf * (y > 0).float()
                if p_keep < 1.0:
                    dyf = dyf / p_keep
            dx = (dyf @ w_comp.float().t()).to(x.dtype)
            dw = x.float().t() @ dyf
            db = dyf.sum(dim=0)
        if not ctx.needs_input_grad[0]:
            dx = None
        return (dx, dw, db, None, None, None, None, None, None, None, None,
                None, None)


def linear_act(x, w, b, w_comp=None, b_comp=None, relu=False, p_keep=1.0,
               seed=0, offset=0, dw_out=None, db_out=None, offset_dev=None,
               w_t=None):
    return LinearActFn.apply(x, w, b, w_comp if w_comp is not None else w,
                             b_comp if b_comp is not None else b, relu,
                             float(p_keep), int(seed), int(offset),
                             dw_out, db_out, offset_dev, w_t)


class SoftmaxXentFn(torch.autograd.Function):
    """Fused mean sparse-softmax-CE + top-1-correct count (mnist.py:149-164).

    Forward also produces dlogits = (softmax - onehot)/B so backward is a
    saved-tensor multiply — one fused GPU kernel total.
    Returns (loss, correct_count); correct_count is non-differentiable.
    """

    @staticmethod
    def forward(ctx, logits, labels):
        if _use_hip(logits):
            loss, correct, dl = _C.ext().softmax_xent_fwd(logits, labels)
        else:
            loss, correct, dl = cpu_ref.softmax_xent_fwd(logits, labels)
        ctx.save_for_backward(dl)
        ctx.mark_non_differentiable(correct)
        return loss, correct

    @staticmethod
    def backward(ctx, dloss, _dcorrect):
        (dl,) = ctx.saved_tensors
        return (dl * dloss).to(dl.dtype), None


def softmax_xent(logits, labels):
    return SoftmaxXentFn.apply(logits, labels)


def grad_mask(grad: torch.Tensor, keep: float, seed: int, step: int,
              rank: int, step_dev=None, base: int = 0):
    """Per-rank PRE-AGGREGATION drop-connect: in-place Bernoulli(keep) mask
    of this rank's local gradient BEFORE the all-reduce, seeded by
    (seed, step, rank) so every worker's mask is distinct — the reference's
    estimator (distributed_train.py:194-203: masks applied per worker, then
    averaged).  Mask, NO rescale (:414-416)."""
    if grad.is_cuda:
        _C.ext().grad_mask(grad, float(keep), int(seed), int(step),
                           int(rank), base=int(base), step_dev=step_dev)
    else:
        gen = torch.Generator(device="cpu")
        gen.manual_seed(((seed ^ 0x9D5AD0C5) * 0x9E3779B97F4A7C15
                         + (step << 20) + rank + 1) % (2**63))
        mask = (torch.rand(grad.shape, generator=gen) < keep).float()
        grad.mul_(mask.to(grad.device))


def batch_gather(img_u8: torch.Tensor, lab_u8: torch.Tensor,
                 lut: torch.Tensor, x: torch.Tensor, y: torch.Tensor,
                 seed: int, step: int | None = None, step_dev=None,
                 aug_table: torch.Tensor | None = None):
    """Build the batch at `step` from the resident uint8 training set into
    the caller's buffers: x[j] = lut[img[perm(...)]] ([B,28,28,1], lut's
    dtype), y[j] = labels ([B] int64).  The sample order is a pure function
    of (seed, step) — ops/cpu_ref.py::batch_indices.  Exactly one of `step`
    (host int) / `step_dev` (device int64, hipGraph-capturable on the HIP
    path) is given.  With `aug_table` (int32 [T,6], ops/cpu_ref.py::
    augment_table) image j is warped by table row aug_indices(seed, step, j)
    before the LUT (batch_gather_aug_kernel on the HIP path); without it the
    plain kernel runs."""
    if (step is None) == (step_dev is None):
        raise ValueError("batch_gather: pass exactly one of step / step_dev")
    if y.shape[0] > lab_u8.shape[0]:
        raise ValueError(f"batch size {y.shape[0]} exceeds the "
                         f"{lab_u8.shape[0]} examples of this rank")
    if aug_table is not None and (
            aug_table.dtype != torch.int32 or aug_table.dim() != 2
            or aug_table.shape[1] != 6 or aug_table.shape[0] < 1):
        raise ValueError("batch_gather: aug_table must be int32 [T >= 1, 6]")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    if _use_hip(x):
        if seed >= 1 << 63:
            seed -= 1 << 64  # int64 carrier of the same 64 bits
        if aug_table is None:
            _C.ext().batch_gather(img_u8, lab_u8, lut, x, y, seed,
                                  0 if step is None else int(step),
                                  step_dev=step_dev)
        else:
            _C.ext().batch_gather_aug(img_u8, lab_u8, lut, aug_table, x, y,
                                      seed, 0 if step is None else int(step),
                                      step_dev=step_dev)
    else:
        if step is None:
            step = int(step_dev.item())  # reference path: host sync is fine
        cpu_ref.batch_gather(img_u8, lab_u8, lut, x, y, seed, int(step),
                             aug_table=aug_table)
    return x, y


def range_gather(img_u8: torch.Tensor, lab_u8: torch.Tensor,
                 lut: torch.Tensor, x: torch.Tensor, y: torch.Tensor,
                 start: int | None = None, start_dev=None):
    """Sequential chunk [start, start + B) of the resident uint8 set into
    the caller's buffers, tail included: rows past N are zero-filled with
    label -1 (ops/cpu_ref.py::range_gather).  Exactly one of `start` (host
    int) / `start_dev` (device int64, hipGraph-capturable on the HIP path)
    is given.  Unlike batch_gather, B > N and start >= N are legal."""
    if (start is None) == (start_dev is None):
        raise ValueError("range_gather: pass exactly one of start / start_dev")
    if _use_hip(x):
        _C.ext().range_gather(img_u8, lab_u8, lut, x, y,
                              0 if start is None else int(start),
                              start_dev=start_dev)
    else:
        if start is None:
            start = int(start_dev.item())  # reference path: host sync is fine
        cpu_ref.range_gather(img_u8, lab_u8, lut, x, y, int(start))
    return x, y


def softmax_eval(logits: torch.Tensor, labels: torch.Tensor,
                 loss_sum: torch.Tensor, counts: torch.Tensor, pred=None,
                 cursor_dev=None):
    """Accumulate one chunk's evaluation statistics into the running state
    (loss_sum fp32 [1], counts int32 [2 + C*C]: live rows, correct rows,
    confusion[true, predicted]); rows whose label lies outside [0, C)
    contribute to nothing.  Optional pred (uint8 [B], 255 = not live) and
    cursor_dev (int64 [1], advanced by B).  No autograd: this is the
    evaluation kernel, it produces no dlogits."""
    if _use_hip(logits):
        _C.ext().softmax_eval(logits, labels, loss_sum, counts, pred=pred,
                              cursor_dev=cursor_dev)
    else:
        cpu_ref.softmax_eval(logits, labels, loss_sum, counts, pred=pred,
                             cursor_dev=cursor_dev)


def grad_norm(flat: torch.Tensor, offsets, numels, grad_scale: float,
              clip: float, stats=None, clipped_steps=None):
    """Per-tensor and global L2 norms of the flat fp32 gradient `flat` (the
    SUM over contributors, grad_scale = 1 / contributors) and the
    clip_grad_norm_ coefficient -> `stats` (fp32 [2 + segments]: norm,
    min(1, clip / (norm + 1e-6)), then one norm per (offset, numel) segment;
    ops/cpu_ref.py::grad_norm).  `stats` is written in place when given;
    `clipped_steps` (int64 [1], optional) counts the calls whose coefficient
    is below 1.  On the GPU one grad_norm_kernel launch: device-resident,
    hipGraph-capturable (after a first call outside capture), no float
    atomics, so equal inputs give equal bits."""
    offsets, numels = [int(o) for o in offsets], [int(m) for m in numels]
    if stats is None:
        stats = torch.empty(2 + len(offsets), dtype=torch.float32,
                            device=flat.device)
    if flat.is_cuda:
        if clipped_steps is None:
            clipped_steps = torch.zeros(1, dtype=torch.int64,
                                        device=flat.device)
        _C.ext().grad_norm(flat, offsets, numels, float(grad_scale),
                           float(clip), stats, clipped_steps)
    else:
        stats.copy_(cpu_ref.grad_norm(flat, offsets, numels, grad_scale,
                                      clip))
        if clipped_steps is not None and float(stats[1]) < 1.0:
            clipped_steps += 1
    return stats


def sgd_step(master: torch.Tensor, grad: torch.Tensor, lr: float,
             grad_scale: float = 1.0, drop_connect_keep=None,
             seed: int = 0, offset: int = 0, shadow=None,
             momentum=None, mu: float = 0.0, ema=None,
             ema_decay: float = 0.0, clip_coef=None):
    """Fused flat SGD apply: master -= lr*scale*(grad [* bernoulli(keep)]).

    `clip_coef` (optional one-element fp32 tensor on master's device,
    grad_norm()'s stats[1:2]) multiplies the gradient first, before the
    drop-connect mask and before momentum; it is read on the device.

    Optionally refreshes the bf16 `shadow` copy (one kernel on GPU).
    Reference semantics: GradientDescentOptimizer + drop_connect mask with NO
    rescale (distributed_train.py:176,414-416).
    `ema` (optional fp32, master's layout) is moved towards the new master
    in the same pass: e -= (1 - d_k)*(e - w), d_k = min(ema_decay,
    (1 + k)/(10 + k)), k = offset + 1 (ops/cpu_ref.py::sgd_step).
    """
    if ema is not None and not 0.0 <= ema_decay < 1.0:
        raise ValueError(f"ema_decay must lie in [0, 1), got {ema_decay}")
    if master.is_cuda:
        _C.ext().sgd_step(master, grad,
                          shadow if shadow is not None else master,
                          shadow is not None, float(lr), float(grad_scale),
                          -1.0 if drop_connect_keep is None else float(drop_connect_keep),
                          int(seed), int(offset),
                          momentum=momentum, mu=float(mu), ema=ema,
                          ema_decay=float(ema_decay), clip_coef=clip_coef)
    else:
        gen = None
        if drop_connect_keep is not None:
            gen = torch.Generator(device="cpu")
            gen.manual_seed((seed * 0x9E3779B97F4A7C15 + offset) % (2**63))
        cpu_ref.sgd_step(master, grad, lr, grad_scale,
                         drop_connect_keep, gen, shadow,
                         momentum=momentum, mu=mu, ema=ema,
                         ema_decay=ema_decay, offset=offset,
                         clip_coef=clip_coef)
