#!/usr/bin/env python3
"""Cost of global-norm gradient clipping (--clip_grad_norm).  For every batch
size it times the graphed LeNet training step (synthetic data, one GPU) with
the flag off, with the never-clipping telemetry setting and with a finite
threshold, and then the grad_norm launch alone.

  off     the trainer as it is without the flag (sgd_step_kernel)
  inf     --clip_grad_norm inf: grad_norm_kernel + sgd_step_kernel_clip, the
          coefficient is 1 on every step
  finite  --clip_grad_norm C, C = --clip (small enough to clip every step)
  solo    one grad_norm launch on the trainer's 1,663,370-element bucket,
          back to back on one stream

Every variant is warmed up (the capture happens there), then timed over
`--steps` steps between two device events with one synchronise at the end.
The variants alternate inside each of `--repeats` rounds so drift hits all
of them alike; the spread over the rounds is reported next to every
difference.  `--only_off` times the flag-off trainer alone and never names
the flag, so the same file also measures a tree that predates it (copy it
there; run both trees in turn in one session for the flag-off comparison).
Prints one JSON line.  Needs a GPU: there is no fallback.
"""

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    """Seconds for `reps` calls, by device events around the whole window."""
    import torch
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1000.0


def spread(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs)}


def make_step(batch, clip, seed, train_dir):
    """A zero-argument function that runs one training step on a fixed
    synthetic batch, and its trainer.  clip: None = the flag is not named."""
    import torch

    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    argv = ["--synthetic_data", "--model", "lenet", "--batch_size",
            str(batch), "--train_dir", train_dir, "--seed", str(seed)]
    if clip is not None:
        argv += ["--clip_grad_norm", str(clip)]
    flags = build_train_parser().parse_args(argv)
    t = Trainer(flags, device=torch.device("cuda:0"))
    ds = make_dataset(flags, 0, 1, t.device, t.compute_dtype)
    x, y = t.to_device(*ds.next_batch(batch))
    return (lambda: t.graph_or_eager_step(x, y)), t


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batches", default="1024,8192")
    ap.add_argument("--clip", type=float, default=0.01,
                    help="threshold of the `finite` variant")
    ap.add_argument("--steps", type=int, default=200,
                    help="training steps per timed window")
    ap.add_argument("--solos", type=int, default=500,
                    help="grad_norm launches per timed window")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=66478)
    ap.add_argument("--only_off", action="store_true",
                    help="time the flag-off trainer alone (also on a tree "
                         "without the flag)")
    ap.add_argument("--out", default="", help="also write the JSON here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("clipbench: no GPU visible; this tool measures the device "
                 "training step and has no CPU fallback")
    result = {"metric": "ms_per_step", "model": "lenet",
              "device": torch.cuda.get_device_name(0), "clip": args.clip,
              "steps_per_window": args.steps, "warmup": args.warmup,
              "repeats": args.repeats, "only_off": args.only_off,
              "batches": {}}
    for batch in [int(b) for b in args.batches.split(",")]:
        fns, trainers = {}, {}
        for name, clip in (("off", None), ("inf", "inf"),
                           ("finite", args.clip)):
            if name != "off" and args.only_off:
                continue
            fns[name], trainers[name] = make_step(
                batch, clip, args.seed, "/tmp/clipbench_" + name)
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        if any(t._graph is None for t in trainers.values()):
            sys.exit("clipbench: the training step was not captured; "
                     "refusing to time the wrong path")
        ms = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():  # alternate inside each round
                ms[k].append(round(1e3 * timed(fn, args.steps) / args.steps,
                                   5))
        entry = {k: dict(spread(v), runs=v) for k, v in ms.items()}
        if not args.only_off:
            for k in ("inf", "finite"):
                entry[k + "-off_us"] = spread(
                    [round(1e3 * (a - b), 3)
                     for a, b in zip(ms[k], ms["off"])])
            t = trainers["finite"]
            entry["finite_clipped_steps"] = int(t.clipped_steps.item())
            entry["finite_updates"] = t.clip_updates
            entry["inf_clipped_steps"] = int(
                trainers["inf"].clipped_steps.item())
            from distributedmnist_amd.ops import functional as Fx
            fp = t.fp
            fp.flat_grad.normal_()  # the graph's tail left the bucket zeroed
            stats = torch.empty_like(t.clip_stats)
            count = torch.zeros_like(t.clipped_steps)

            def solo():
                Fx.grad_norm(fp.flat_grad, fp.offsets, fp.numels, 1.0,
                             args.clip, stats=stats, clipped_steps=count)

            for _ in range(args.warmup):
                solo()
            entry["solo_us"] = dict(spread(
                [round(1e6 * timed(solo, args.solos) / args.solos, 3)
                 for _ in range(args.repeats)]),
                launches_per_window=args.solos)
            fp.flat_grad.zero_()
        result["batches"][str(batch)] = entry
        del fns, trainers
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
