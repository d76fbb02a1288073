#!/usr/bin/env python3
"""Cost of --grad_dtype mxfp8 at world 1.  For every batch size it times the
graphed LeNet training step (synthetic data, one GPU) in two variants:

  momentum  --momentum 0.9, the baseline
  mxfp8     --momentum 0.9 --grad_dtype mxfp8: mx_encode_kernel and
            mx_decode_kernel of csrc/mxwire.hip between the gradients and the
            update

Both are warmed up (the capture happens there), then timed over `--steps`
steps between two device events with one synchronise at the end; they
alternate inside each of `--repeats` rounds.  `--only_momentum` times the
baseline alone and names no new flag value, so the same file also measures a
tree that predates the feature.  Then the three kernels alone on LeNet's
bucket (mx_reduce_kernel on the W = 8 shard), `--solos` launches per window,
against a device-to-device copy_ of the bucket in the same process: achieved
bytes/s from the bytes each one must move.  At world 1 the feature only adds
work: the wire saving exists with more than one rank and is reported from the
shapes, not measured.  Prints one JSON line.  Needs a GPU: there is no
fallback.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.adambench import make_step  # noqa: E402
from tools.clipbench import spread, timed  # noqa: E402


def kernels(n, solos, repeats):
    """{name: bytes moved, us per launch, GB/s} of the kernels alone."""
    import torch

    from distributedmnist_amd.ops import cpu_ref
    from distributedmnist_amd.ops import functional as Fx
    x = torch.randn(n, device="cuda") * 0.01
    keep, out, dst = (torch.empty_like(x) for _ in range(3))
    wire = Fx.mx_encode(x, 1, 0, 0, 0)
    sb8 = cpu_ref.mx_shard_blocks(n, 8)
    rows = Fx.mx_encode(x, 1, 0, 0, 0, world=8)  # eight rows of shard size
    shard = torch.empty(33 * sb8, dtype=torch.uint8, device="cuda")
    cases = {
        "copy_": (8 * n, lambda: dst.copy_(x)),
        "mx_encode_kernel": (4 * n + wire.numel(),
                             lambda: Fx.mx_encode(x, 1, 0, 0, 0, out=wire)),
        "mx_encode_kernel+keep": (
            8 * n + wire.numel(),
            lambda: Fx.mx_encode(x, 1, 0, 0, 0, out=wire, keep=keep)),
        "mx_reduce_kernel_w8": (rows.numel() + shard.numel(),
                                lambda: Fx.mx_reduce(rows, 1, 0, 0, out=shard)),
        "mx_decode_kernel": (4 * n + wire.numel(),
                             lambda: Fx.mx_decode(wire, n, out=out)),
    }
    res = {}
    for name, (nbytes, fn) in cases.items():
        for _ in range(20):
            fn()
        us = [1e6 * timed(fn, solos) / solos for _ in range(repeats)]
        res[name] = {"bytes": nbytes, "us": spread([round(u, 3) for u in us]),
                     "GBps_at_median": round(
                         nbytes / spread(us)["median"] / 1e3, 1)}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batches", default="1024,8192")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--solos", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=66478)
    ap.add_argument("--only_momentum", action="store_true")
    ap.add_argument("--out", default="", help="also write the JSON here")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("mxbench: no GPU visible; this tool measures the device "
                 "training step and has no CPU fallback")
    variants = {"momentum": ["--momentum", "0.9"]}
    if not args.only_momentum:
        variants["mxfp8"] = ["--momentum", "0.9", "--grad_dtype", "mxfp8"]
    result = {"metric": "ms_per_step", "model": "lenet",
              "device": torch.cuda.get_device_name(0),
              "steps_per_window": args.steps, "warmup": args.warmup,
              "repeats": args.repeats, "batches": {}}
    for batch in [int(b) for b in args.batches.split(",")]:
        fns, trainers = {}, {}
        for name, extra in variants.items():
            fns[name], trainers[name] = make_step(
                batch, extra, args.seed, "/tmp/mxbench_" + name)
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        if any(t._graph is None for t in trainers.values()):
            sys.exit("mxbench: the training step was not captured; refusing "
                     "to time the wrong path")
        ms = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():  # alternate inside each round
                ms[k].append(round(1e3 * timed(fn, args.steps) / args.steps,
                                   5))
        entry = {k: dict(spread(v), runs=v) for k, v in ms.items()}
        if "mxfp8" in ms:
            entry["mxfp8-momentum_us"] = spread(
                [round(1e3 * (p - q), 3)
                 for p, q in zip(ms["mxfp8"], ms["momentum"])])
            t = trainers["mxfp8"]
            n = t.fp.flat_grad.numel()
            from distributedmnist_amd.ops import cpu_ref
            result["wire_from_shapes"] = {
                "dense_floats": n,
                "bytes_per_rank_and_step": {
                    str(w): 2 * (w - 1) * 33 * cpu_ref.mx_shard_blocks(n, w)
                    for w in (2, 4, 8)}}
            result["relative_l2_error"] = t.mx_stats()
        result["batches"][str(batch)] = entry
        del fns, trainers
    if not args.only_momentum:
        result["kernels"] = kernels(n, args.solos, args.repeats)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
