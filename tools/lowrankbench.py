#!/usr/bin/env python3
"""Cost of --grad_lowrank at world 1.  For every batch size it times the
graphed LeNet training step (synthetic data, one GPU) in two variants:

  momentum  --momentum 0.9, the baseline
  lowrank   --momentum 0.9 --grad_lowrank R: the four kernels of
            csrc/lowrank.hip between the gradients and the update

Both are warmed up (the capture happens there), then timed over `--steps`
steps between two device events with one synchronise at the end; they
alternate inside each of `--repeats` rounds.  `--only_momentum` times the
baseline alone and names no new flag, so the same file also measures a tree
that predates the feature.  At world 1 the feature only adds work: the wire
saving exists with more than one rank and is reported from the shapes, not
measured.  Prints one JSON line.  Needs a GPU: there is no fallback.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.adambench import make_step  # noqa: E402
from tools.clipbench import spread, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batches", default="1024,8192")
    ap.add_argument("--rank", default="4")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=66478)
    ap.add_argument("--only_momentum", action="store_true")
    ap.add_argument("--out", default="", help="also write the JSON here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("lowrankbench: no GPU visible; this tool measures the device "
                 "training step and has no CPU fallback")
    variants = {"momentum": ["--momentum", "0.9"]}
    if not args.only_momentum:
        variants["lowrank"] = ["--momentum", "0.9", "--grad_lowrank",
                               args.rank]
    result = {"metric": "ms_per_step", "model": "lenet",
              "device": torch.cuda.get_device_name(0), "rank": args.rank,
              "steps_per_window": args.steps, "warmup": args.warmup,
              "repeats": args.repeats, "batches": {}}
    for batch in [int(b) for b in args.batches.split(",")]:
        fns, trainers = {}, {}
        for name, extra in variants.items():
            fns[name], trainers[name] = make_step(
                batch, extra, args.seed, "/tmp/lowrankbench_" + name)
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        if any(t._graph is None for t in trainers.values()):
            sys.exit("lowrankbench: the training step was not captured; "
                     "refusing to time the wrong path")
        ms = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():  # alternate inside each round
                ms[k].append(round(1e3 * timed(fn, args.steps) / args.steps,
                                   5))
        entry = {k: dict(spread(v), runs=v) for k, v in ms.items()}
        if "lowrank" in ms:
            entry["lowrank-momentum_us"] = spread(
                [round(1e3 * (p - q), 3)
                 for p, q in zip(ms["lowrank"], ms["momentum"])])
            st = trainers["lowrank"].lowrank
            result["wire_from_shapes"] = {
                "first_allreduce_floats": st.p_floats + st.dense_floats,
                "second_allreduce_floats": st.q_floats,
                "dense_floats": st.n}
            result["residual_share"] = trainers["lowrank"].lowrank_stats()
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
