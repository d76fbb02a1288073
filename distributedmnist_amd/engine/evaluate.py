"""Checkpoint-polling evaluator — re-expression of /root/reference/src/nn_eval.py.

Behavior kept: restore latest checkpoint (nn_eval.py:70-78), skip when the
step hasn't advanced (:84-88), single full-validation-set batch
accuracy+loss (:95-100), scraper-compatible result line (:102), optional
TensorBoard scalars (:107-110), poll loop every eval_interval_secs
(:136-140).
"""

from __future__ import annotations

import logging
import time

import torch

from ..models import build_model
from .supervisor import Supervisor

log = logging.getLogger("dmnist.eval")


def do_eval(model, images, labels, device, dtype, batch_size: int = 10000):
    """Full-set eval in chunks (the reference feeds all 10k in one batch;
    we chunk to bound activation memory, identical result)."""
    model.eval()
    total = images.shape[0]
    correct_sum = 0.0
    loss_sum = 0.0
    with torch.no_grad():
        for s in range(0, total, batch_size):
            e = min(s + batch_size, total)
            x = images[s:e].to(device=device, dtype=dtype)
            y = labels[s:e].to(device=device)
            logits = model(x, train=False)
            loss, correct = model.loss_and_accuracy(logits, y)
            n = e - s
            correct_sum += float(correct) * n  # loss_and_accuracy returns mean acc
            loss_sum += float(loss) * n
    return correct_sum / total, loss_sum / total


def resolve_eval_device(flags):
    """(device, compute dtype) of the evaluator process."""
    device = torch.device(flags.device) if flags.device not in ("auto", "") else (
        torch.device("cuda:0") if torch.cuda.is_available() else torch.device("cpu"))
    dtype = torch.bfloat16 if device.type == "cuda" else torch.float32
    return device, dtype


def checkpoint_flat(payload, flags):
    """The flat fp32 weights to evaluate: the raw master, or with
    --use_moving_average the checkpoint's weight moving average — never a
    silent fallback from one to the other."""
    if not getattr(flags, "use_moving_average", False):
        return payload["flat_master"]
    if payload.get("flat_ema") is None:
        raise ValueError(
            "--use_moving_average: this checkpoint carries no weight moving "
            "average; train with --moving_average_decay D (0 < D < 1) to "
            "write one")
    return payload["flat_ema"]


def evaluate_resident(dataset, flags, writer=None):
    """--device_data poll loop: `dataset` is a DeviceDataSet already on the
    evaluator's device (uploaded once, before the loop); the model, its
    FlatParams and the DeviceEvaluator are built once and every new
    checkpoint is loaded in place.  Same result lines as evaluate()."""
    import os

    import numpy as np

    from ..parallel import FlatParams
    from .device_eval import DeviceEvaluator
    device, dtype = resolve_eval_device(flags)
    start_time = time.time()
    last_step = -1
    results = []
    n_evals = 0
    fp = ev = model_name = None
    while True:
        restored = Supervisor.restore(flags.checkpoint_dir)
        if restored is not None:
            step, payload = restored
            if step != last_step:
                name = payload.get("model", flags.model)
                if ev is None or name != model_name:
                    model = build_model(name, seed=payload.get("seed", 66478),
                                        compute_dtype=dtype).to(device)
                    fp = FlatParams(model, device=device, compute_dtype=dtype)
                    ev = DeviceEvaluator(model, dataset,
                                         flags.eval_batch_size, device)
                    model_name = name
                fp.load_flat(checkpoint_flat(payload, flags))
                print('Succesfully loaded model from %s at step=%s.' %
                      (Supervisor.latest_checkpoint(flags.checkpoint_dir)[1], step),
                      flush=True)
                res = ev.run()
                print('Num examples: %d  Precision @ 1: %f Loss: %f Time: %f' %
                      (res.num_examples, res.precision, res.loss,
                       time.time() - start_time), flush=True)
                if writer is not None:
                    writer.add_scalar("Validation Accuracy", res.precision, step)
                    writer.add_scalar("Validation Loss", res.loss, step)
                if getattr(flags, "confusion", False):
                    conf = res.confusion.numpy()
                    os.makedirs(flags.eval_dir, exist_ok=True)
                    np.save(os.path.join(flags.eval_dir,
                                         f"confusion-{step}.npy"), conf)
                    recall = conf.diagonal() / np.maximum(conf.sum(axis=1), 1)
                    log.info("step %d per-class recall: %s", step,
                             " ".join("%d:%.4f" % (c, r)
                                      for c, r in enumerate(recall)))
                results.append((step, res.precision, res.loss))
                last_step = step
                n_evals += 1
        if flags.run_once or (flags.max_evals and n_evals >= flags.max_evals):
            break
        time.sleep(flags.eval_interval_secs)
    return results


def evaluate(dataset, flags, writer=None):
    """Poll loop. Returns list of (step, precision, loss)."""
    if getattr(flags, "device_data", False):
        return evaluate_resident(dataset, flags, writer=writer)
    device, dtype = resolve_eval_device(flags)
    start_time = time.time()
    last_step = -1
    results = []
    n_evals = 0
    while True:
        restored = Supervisor.restore(flags.checkpoint_dir)
        if restored is not None:
            step, payload = restored
            if step != last_step:
                ema_flat = (checkpoint_flat(payload, flags)
                            if getattr(flags, "use_moving_average", False)
                            else None)
                model = build_model(payload.get("model", flags.model),
                                    seed=payload.get("seed", 66478),
                                    compute_dtype=dtype).to(device)
                with torch.no_grad():
                    for name in model.PARAM_ORDER:
                        getattr(model, name).copy_(
                            payload["model_state"][name].to(device))
                # first-class GPU eval: FlatParams builds the bf16 shadows
                # AND the pre-transposed shadow_T copies, so evaluation
                # runs the SAME transposed-GEMM kernel path as training
                # (round-1 built shadows ad hoc without shadows_T and fell
                # onto the non-transposed GEMMs)
                from ..parallel import FlatParams
                fp = FlatParams(model, device=device, compute_dtype=dtype)
                if ema_flat is not None:
                    fp.load_flat(ema_flat)
                print('Succesfully loaded model from %s at step=%s.' %
                      (Supervisor.latest_checkpoint(flags.checkpoint_dir)[1], step),
                      flush=True)
                images = torch.as_tensor(dataset.images)
                labels = torch.as_tensor(dataset.labels)
                acc, loss = do_eval(model, images, labels, device, dtype)
                # exact reference line (nn_eval.py:102) — scraped by
                # benchmark.py extract_times_losses_precision
                print('Num examples: %d  Precision @ 1: %f Loss: %f Time: %f' %
                      (dataset.num_examples, acc, loss,
                       time.time() - start_time), flush=True)
                if writer is not None:
                    writer.add_scalar("Validation Accuracy", acc, step)
                    writer.add_scalar("Validation Loss", loss, step)
                results.append((step, acc, loss))
                last_step = step
                n_evals += 1
        if flags.run_once or (flags.max_evals and n_evals >= flags.max_evals):
            break
        time.sleep(flags.eval_interval_secs)
    return results
