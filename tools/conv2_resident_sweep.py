#!/usr/bin/env python3
"""Sweep the weight-resident conv2 forward and pooled-dX kernels on GPU against
the per-image slab kernels they replace: batch size, waves per block
(DMNIST_CONV2_RES_WAVES) and next-image prefetch (DMNIST_CONV2_RES_PF).  Solo
launches timed with device events, median of 60, us.  Every resident result is first compared
bitwise with the slab kernel's.

Usage: python tools/conv2_resident_sweep.py [batch ...]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from distributedmnist_amd import _C
from tools.kernbench import timeit

bf16 = torch.bfloat16
ext = _C.ext()
KEYS = ("DMNIST_CONV2_RESIDENT", "DMNIST_CONV2_RES_BLOCKS",
        "DMNIST_CONV2_RES_MIN_NB", "DMNIST_CONV2_RES_WAVES",
        "DMNIST_CONV2_RES_PF")
VARIANTS = [(w, pf) for w in (4, 8) for pf in (1, 0)]


def clear():
    for k in KEYS:
        os.environ.pop(k, None)


def variant(w, pf):
    os.environ["DMNIST_CONV2_RES_WAVES"] = str(w)
    os.environ["DMNIST_CONV2_RES_PF"] = str(pf)
    os.environ["DMNIST_CONV2_RESIDENT"] = "both"
    os.environ["DMNIST_CONV2_RES_MIN_NB"] = "1"


clear()
print("| B | op | old | " +
      " | ".join(f"w{w} pf{pf}" for w, pf in VARIANTS) + " |")
print("|---|---|---|" + "---|" * len(VARIANTS))
for B in [int(a) for a in sys.argv[1:]] or [64, 128, 256, 512, 1024, 2048,
                                            4096, 8192]:
    x = (torch.randn(B, 14, 14, 32) * 0.5).to("cuda", bf16)
    w = (torch.randn(5, 5, 32, 64) * 0.05).to("cuda", bf16)
    b = (torch.randn(64) * 0.1).to("cuda")
    gp = (torch.randn(B, 7, 7, 64) * 0.1).to("cuda", bf16)
    am = torch.randint(0, 4, (B, 7, 7, 64), device="cuda").to(torch.uint8)
    am[torch.rand(B, 7, 7, 64, device="cuda") < 0.25] = 7
    fwd = lambda: ext.conv_pool_fwd(x, w, b, None)
    dx_old = [lambda: ext.conv_dx_pooled(gp, am, w, 32, force_db=1),
              lambda: ext.conv_dx_pooled(gp, am, w, 32, force_db=2)]
    dx_res = lambda: ext.conv_dx_pooled(gp, am, w, 32, force_db=3)

    os.environ["DMNIST_CONV2_RESIDENT"] = "0"
    y0, a0 = fwd()
    d0 = dx_old[1]()
    t_fwd = timeit(fwd, iters=60)
    t_dx = [timeit(f, iters=60) for f in dx_old]
    clear()
    row_f, row_d = [], []
    for v in VARIANTS:
        variant(*v)
        y1, a1 = fwd()
        d1 = dx_res()
        ok_f = torch.equal(y1.view(torch.int16), y0.view(torch.int16)) and \
            torch.equal(a1, a0)
        ok_d = torch.equal(d1.view(torch.int16), d0.view(torch.int16))
        row_f.append(f"{timeit(fwd, iters=60):.1f}" if ok_f else "MISMATCH")
        row_d.append(f"{timeit(dx_res, iters=60):.1f}" if ok_d else "MISMATCH")
        clear()
    print(f"| {B} | fwd | {t_fwd:.1f} | " + " | ".join(row_f) + " |")
    print(f"| {B} | dx | db1 {t_dx[0]:.1f} / db2 {t_dx[1]:.1f} | " +
          " | ".join(row_d) + " |", flush=True)
