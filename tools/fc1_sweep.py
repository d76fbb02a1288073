#!/usr/bin/env python3
"""Sweep the three fc1 (3136 -> 512) GEMMs on GPU, old and new epilogues in
one process (every switch is read per call):
  dW      DMNIST_DW_PLAN = tbm,bn,splitk over {64,128} x {64,128} x {1,2,4},
          against the pre-plan choice (DMNIST_DW_PLAN=0) and the launcher's
          default plan;
  dX      DMNIST_UNPOOL_LINES x DMNIST_UNPOOL_TILE, and the pooled-gradient
          producer linear_dx_pooled at both tiles;
  forward DMNIST_FC_FIXUP (split-K route only).
Solo launches timed with device events, median of 60, us."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from distributedmnist_amd import _C
from tools.kernbench import timeit

bf16 = torch.bfloat16
ext = _C.ext()
KEYS = ("DMNIST_DW_PLAN", "DMNIST_UNPOOL_LINES", "DMNIST_UNPOOL_TILE",
        "DMNIST_FC_FIXUP")
for k in KEYS:
    os.environ.pop(k, None)


def timed(run, **env):
    for k, v in env.items():
        os.environ[k] = v
    us = timeit(run, iters=60)
    for k in env:
        del os.environ[k]
    return us


for B in [int(a) for a in sys.argv[1:]] or [1024, 8192]:
    h2 = (torch.randn(B, 3136) * 0.5).to("cuda", bf16)
    dyeff1 = (torch.randn(B, 512) * 0.1).to("cuda", bf16)
    w = (torch.randn(3136, 512) * 0.05).to("cuda", bf16)
    wT = w.t().contiguous()
    bias = torch.full((512,), 0.1, device="cuda")
    am = torch.randint(0, 4, (B, 7, 7, 64), device="cuda").to(torch.uint8)
    am[torch.rand(B, 7, 7, 64, device="cuda") < 0.25] = 7
    dw = torch.zeros(3136, 512, device="cuda")
    dbc = torch.zeros(64, device="cuda")
    print(f"## B={B}")

    run = lambda: ext.linear_dw_into(h2, dyeff1, dw)
    os.environ["DMNIST_DW_PLAN"] = "0"
    old = ext.linear_dw_plan(3136, 512, B)
    del os.environ["DMNIST_DW_PLAN"]
    print(f"dW pre-plan {old}: {timed(run, DMNIST_DW_PLAN='0'):.1f} us")
    print(f"dW launcher default {ext.linear_dw_plan(3136, 512, B)}: "
          f"{timeit(run, iters=60):.1f} us")
    print("| tbm x bn | splitk=1 | splitk=2 | splitk=4 |")
    print("|---|---|---|---|")
    for tbm in (64, 128):
        for bn in (64, 128):
            row = [f"{timed(run, DMNIST_DW_PLAN=f'{tbm},{bn},{sk}'):.1f}"
                   for sk in (1, 2, 4)]
            print(f"| {tbm} x {bn} | " + " | ".join(row) + " |", flush=True)

    run = lambda: ext.linear_dx_unpool(dyeff1, w, am, dbc, 7, 7, 64)
    print("| dX+unpool | element stores | line stores |")
    print("|---|---|---|")
    for tile in ("64", "128"):
        a = timed(run, DMNIST_UNPOOL_TILE=tile, DMNIST_UNPOOL_LINES="0")
        b = timed(run, DMNIST_UNPOOL_TILE=tile)
        print(f"| tile {tile} | {a:.1f} | {b:.1f} |", flush=True)

    print("| dX+poolmask (gp2, no dact2) | us |")
    print("|---|---|")
    for tile in (64, 128):
        us = timeit(lambda: ext.linear_dx_pooled(dyeff1, w, am, dbc, 7, 7,
                                                 64, tile=tile), iters=60)
        print(f"| tile {tile} | {us:.1f} |", flush=True)
    print(f"launcher default: tile {ext.linear_dx_pooled_tile(B, 3136)}")

    run = lambda: ext.linear_act_fwd(h2, w, bias, True, 0.5, 1, 2, wT=wT)
    a = timed(run, DMNIST_FC_FIXUP="0")
    b = timed(run, DMNIST_FC_FIXUP="1")
    print(f"forward: two launches {a:.1f} us, in-kernel fix-up {b:.1f} us "
          f"(same number when B is off the split-K route)", flush=True)
