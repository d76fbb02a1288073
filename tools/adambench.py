#!/usr/bin/env python3
"""Cost of --optimizer adam|lamb|muon.  For every batch size it times the
graphed LeNet training step (synthetic data, one GPU) in five variants:

  momentum  --momentum 0.9 (sgd_step_kernel with momentum), the baseline
  sgd       no optimizer flag, the default path
  adam      --optimizer adam --weight_decay 1e-2: adam_step_kernel
  lamb      --optimizer lamb --weight_decay 1e-2: lamb_moments_kernel +
            lamb_apply_kernel
  muon      --optimizer muon --momentum 0.95 --weight_decay 1e-2: the kernel
            sequence of csrc/muon.hip

Every variant is warmed up (the capture happens there), then timed over
`--steps` steps between two device events with one synchronise at the end.
The variants alternate inside each of `--repeats` rounds.  `--only_sgd` times
the first two alone and names no new flag, so the same file also measures a
tree that predates the optimizers.  Prints one JSON line.  Needs a GPU: there
is no fallback.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.clipbench import spread, timed  # noqa: E402

VARIANTS = {"momentum": ["--momentum", "0.9"], "sgd": [],
            "adam": ["--optimizer", "adam", "--weight_decay", "1e-2"],
            "lamb": ["--optimizer", "lamb", "--weight_decay", "1e-2"],
            "muon": ["--optimizer", "muon", "--momentum", "0.95",
                     "--weight_decay", "1e-2"]}


def make_step(batch, extra, seed, train_dir):
    import torch

    from distributedmnist_amd.engine.train import Trainer, make_dataset
    from distributedmnist_amd.utils.flags import build_train_parser
    flags = build_train_parser().parse_args(
        ["--synthetic_data", "--model", "lenet", "--batch_size", str(batch),
         "--train_dir", train_dir, "--seed", str(seed)] + extra)
    t = Trainer(flags, device=torch.device("cuda:0"))
    ds = make_dataset(flags, 0, 1, t.device, t.compute_dtype)
    x, y = t.to_device(*ds.next_batch(batch))
    return (lambda: t.graph_or_eager_step(x, y)), t


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batches", default="1024,8192")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=66478)
    ap.add_argument("--only_sgd", action="store_true")
    ap.add_argument("--out", default="", help="also write the JSON here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("adambench: no GPU visible; this tool measures the device "
                 "training step and has no CPU fallback")
    result = {"metric": "ms_per_step", "model": "lenet",
              "device": torch.cuda.get_device_name(0),
              "steps_per_window": args.steps, "warmup": args.warmup,
              "repeats": args.repeats, "only_sgd": args.only_sgd,
              "batches": {}}
    names = ["momentum", "sgd"] if args.only_sgd else list(VARIANTS)
    for batch in [int(b) for b in args.batches.split(",")]:
        fns, trainers = {}, {}
        for name in names:
            fns[name], trainers[name] = make_step(
                batch, VARIANTS[name], args.seed, "/tmp/adambench_" + name)
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        if any(t._graph is None for t in trainers.values()):
            sys.exit("adambench: the training step was not captured; "
                     "refusing to time the wrong path")
        ms = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():  # alternate inside each round
                ms[k].append(round(1e3 * timed(fn, args.steps) / args.steps,
                                   5))
        entry = {k: dict(spread(v), runs=v) for k, v in ms.items()}
        for a in ("adam", "lamb", "muon"):
            if a in ms:
                entry[f"{a}-momentum_us"] = spread(
                    [round(1e3 * (p - q), 3)
                     for p, q in zip(ms[a], ms["momentum"])])
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
