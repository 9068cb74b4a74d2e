#!/usr/bin/env python3
"""Where a block of sgemm_nn_w4_kernel spends the time outside its MFMAs
(diagnostic build with -DTNS_W4_STAMPS, loaded with TNS_LIB=...): every wave
records s_memtime at entry, at its first MFMA, after its last MFMA and after
its last store has completed.  Medians over the waves of the stamped launch of
(first MFMA - entry), (last MFMA - first MFMA), (exit - last MFMA), for the
flat and the row-ordered schedule, at 4096^3 and at 1024 x 1024^3 (strict
beta = 0: C is read).  One JSON document.

  python scripts/ab_build.py w4s -DTNS_W4_STAMPS sgemm_nn_w4.hip
  TNS_LIB=ab/w4s/libtensorium_hip.so python scripts/w4_stamps.py [--out profiles/x.json]
"""
import argparse
import ctypes
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from tensorium_amd._abi import load  # noqa: E402
from tensorium_amd.nnhip import TNNHip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="")
ap.add_argument("--warm", type=int, default=40, help="launches before the stamped one (4096^3)")
a = ap.parse_args()
hip = TNNHip(0)
lib = load()
fn = lib.tns_debug_w4_stamps
fn.argtypes = [ctypes.c_void_p]
names = TNNHip.gemmVariants()
forms = {"flat": names.index("256x256x32_w2x2_dma_flat_nn_big"),
         "rows": names.index("256x256x32_w2x2_dma_nn_big")}
stamps = torch.zeros(65536 * 4 * 4, dtype=torch.int64, device="cuda")


def q(v):
    return [round(float(np.percentile(v, x)), 1) for x in (10, 50, 90)]


def measure(v, n, nb, warm):
    A = torch.rand(nb, n, n, device="cuda") * 2 - 1
    B = torch.rand(nb, n, n, device="cuda") * 2 - 1
    C = torch.rand(nb, n, n, device="cuda") * 2 - 1

    def run():
        hip.gemmVariant(v, False, False, n, n, n, 1.0, A, 0, n, n * n, B, 0, n, n * n, 0.0, C, 0, n,
                        n * n, nb)
    for _ in range(warm):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(max(warm // 4, 1)):
        run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / max(warm // 4, 1)
    stamps.zero_()
    fn(stamps.data_ptr())
    run()
    torch.cuda.synchronize()
    fn(None)
    st = stamps.cpu().numpy().reshape(-1, 4).astype(np.float64)
    st = st[st[:, 3] > 0]
    front, loop, back = st[:, 1] - st[:, 0], st[:, 2] - st[:, 1], st[:, 3] - st[:, 2]
    total = st[:, 3] - st[:, 0]
    return {"launch_ms": round(ms, 4), "waves": int(len(st)),
            "entry_to_first_mfma_cycles_p10_p50_p90": q(front),
            "first_to_last_mfma_cycles_p10_p50_p90": q(loop),
            "last_mfma_to_exit_cycles_p10_p50_p90": q(back),
            "entry_to_exit_cycles_p10_p50_p90": q(total)}


doc = {"note": "s_memtime ticks per wave; strict beta = 0 (C read); medians over every wave of "
               "the first 65536 blocks of one stamped launch after a warm-up"}
for label, (n, nb, warm) in {"4096^3": (4096, 1, a.warm), "1024x1024^3": (1024, 1024, 3)}.items():
    doc[label] = {k: measure(v, n, nb, warm) for k, v in forms.items()}
text = json.dumps(doc, indent=1)
print(text)
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text + "\n")
