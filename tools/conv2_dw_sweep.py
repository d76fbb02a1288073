#!/usr/bin/env python3
"""Sweep the slab conv2 dW kernel on GPU: images per block (DMNIST_DW2_G)
for the kernel-row split (KHB=1) and the all-taps block (DMNIST_DW2_KHB=5),
single- and double-buffered slabs (DMNIST_DW2_NBUF), against conv_dw_tr
(DMNIST_DW2_SLAB=0), and the pooled-operand form conv_dw_pooled_into (KHB=1,
NBUF=1; D rebuilt in LDS from the pooled gradient and the argmax bytes) over
the same G.  Solo launches timed with device events, median of 60, us.

Usage: python tools/conv2_dw_sweep.py [batch ...]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from distributedmnist_amd import _C
from tools.kernbench import timeit

bf16 = torch.bfloat16
ext = _C.ext()
GS = [1, 2, 4, 6, 8, 12, 16, 20, 24, 32, 48, 64]
for k in ("DMNIST_DW2_G", "DMNIST_DW2_KHB", "DMNIST_DW2_NBUF",
          "DMNIST_DW2_SLAB"):
    os.environ.pop(k, None)
for B in [int(a) for a in sys.argv[1:]] or [1024, 8192]:
    y1 = (torch.randn(B, 14, 14, 32) * 0.1).to("cuda", bf16)
    dact2 = (torch.randn(B, 14, 14, 64) * 0.1).to("cuda", bf16)
    dw = torch.zeros(5, 5, 32, 64, device="cuda")
    gp2 = (torch.randn(B, 7, 7, 64) * 0.1).to("cuda", bf16)
    am2 = torch.randint(0, 4, (B, 7, 7, 64), device="cuda").to(torch.uint8)
    am2[torch.rand(B, 7, 7, 64, device="cuda") < 0.25] = 7
    runp = lambda: ext.conv_dw_pooled_into(y1, gp2, am2, dw.view(-1))
    run = lambda: ext.conv_dw_into(y1, dact2, dw)
    print(f"## B={B}")
    os.environ["DMNIST_DW2_SLAB"] = "0"
    print(f"conv_dw_tr: {timeit(run, iters=60):.1f} us")
    del os.environ["DMNIST_DW2_SLAB"]
    print(f"slab, launcher default (G={ext.conv2_dw_group(B)}): "
          f"{timeit(run, iters=60):.1f} us")
    print(f"pooled, launcher default (G={ext.conv2_dw_group(B)}): "
          f"{timeit(runp, iters=60):.1f} us")
    print("| G | " + " | ".join(str(g) for g in GS) + " |")
    print("|---|" + "---|" * len(GS))
    row = []
    for g in GS:
        os.environ["DMNIST_DW2_G"] = str(g)
        row.append(f"{timeit(runp, iters=60):.1f}")
    del os.environ["DMNIST_DW2_G"]
    print("| pooled KHB=1 NBUF=1 | " + " | ".join(row) + " |", flush=True)
    for khb, nbuf in ((1, 1), (1, 2), (5, 1), (5, 2)):
        os.environ["DMNIST_DW2_KHB"] = str(khb)
        os.environ["DMNIST_DW2_NBUF"] = str(nbuf)
        row = []
        for g in GS:
            os.environ["DMNIST_DW2_G"] = str(g)
            row.append(f"{timeit(run, iters=60):.1f}")
        print(f"| KHB={khb} NBUF={nbuf} | " + " | ".join(row) + " |",
              flush=True)
        for k in ("DMNIST_DW2_G", "DMNIST_DW2_KHB", "DMNIST_DW2_NBUF"):
            del os.environ[k]
