#!/usr/bin/env python3
"""Cost of the deterministic mode (--deterministic).  For every batch size it
times the graphed LeNet training step (synthetic data, one GPU) with the flag
off and on in the same build, and reports the bytes of plane workspace the
mode holds.

  off  the trainer as it is without the flag (fp32 atomics in the flushes)
  on   --deterministic: every gradient flush stores per-block planes, and
       plane_reduce launches add them in index order

The switch is per process and read on every call, but a captured graph keeps
the route it was captured with: each trainer is built AND warmed up (the
capture happens there) before the next one is built, so the two graphs hold
one route each and can then be replayed in turn.  Every variant is timed over
`--steps` steps between two device events with one synchronise at the end.
The variants alternate inside each of `--repeats` rounds so drift hits both
alike; the spread over the rounds is reported next to the difference.
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


def make_step(batch, det, seed, train_dir, warmup):
    """A zero-argument function that runs one (captured) training step on a
    fixed synthetic batch, and its trainer; warmed up before returning."""
    import torch

    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    argv = ["--synthetic_data", "--model", "lenet", "--batch_size",
            str(batch), "--train_dir", train_dir, "--seed", str(seed)]
    if det:
        argv += ["--deterministic"]
    flags = build_train_parser().parse_args(argv)
    t = Trainer(flags, device=torch.device("cuda:0"))
    ds = make_dataset(flags, 0, 1, t.device, t.compute_dtype)
    x, y = t.to_device(*ds.next_batch(batch))

    def fn():
        return t.graph_or_eager_step(x, y)
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return fn, t


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batches", default="1024,8192")
    ap.add_argument("--steps", type=int, default=200,
                    help="training steps per timed window")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=66478)
    ap.add_argument("--out", default="", help="also write the JSON here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("detbench: no GPU visible; this tool measures the device "
                 "training step and has no CPU fallback")
    from distributedmnist_amd import _C
    ext = _C.ext()
    result = {"metric": "ms_per_step", "model": "lenet",
              "device": torch.cuda.get_device_name(0),
              "steps_per_window": args.steps, "warmup": args.warmup,
              "repeats": args.repeats, "batches": {}}
    seen = set()
    for batch in [int(b) for b in args.batches.split(",")]:
        fns, trainers = {}, {}
        for name, det in (("off", False), ("on", True)):
            fns[name], trainers[name] = make_step(
                batch, det, args.seed, "/tmp/detbench_" + name, args.warmup)
        if any(t._graph is None for t in trainers.values()):
            sys.exit("detbench: the training step was not captured; "
                     "refusing to time the wrong path")
        ms = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():  # alternate inside each round
                ms[k].append(round(1e3 * timed(fn, args.steps) / args.steps,
                                   5))
        entry = {k: dict(spread(v), runs=v) for k, v in ms.items()}
        entry["on-off_us"] = spread(
            [round(1e3 * (a - b), 3) for a, b in zip(ms["on"], ms["off"])])
        # regions are kept per destination size and only grow: what this
        # batch size added (or grew) is its own plane workspace
        ws = [(t.data_ptr(), t.numel() * 4) for t in ext.det_workspace()]
        entry["workspace_bytes"] = sum(b for p, b in ws if (p, b) not in seen)
        entry["workspace_regions"] = sorted(
            b for p, b in ws if (p, b) not in seen)
        entry["workspace_bytes_process"] = sum(b for _, b in ws)
        seen.update(ws)
        result["batches"][str(batch)] = entry
        ext.set_deterministic(False)
        del fns, trainers
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
