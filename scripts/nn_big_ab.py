#!/usr/bin/env python3
"""A/B of the large-NN SGEMM variants at one size: interleaved rounds of
warm-up + timed launches (HIP events), outputs compared bit for bit.  The
first variant listed is the baseline: every other one is reported against its
median and its round-to-round spread (max - min), and counts as faster only
when its median is below the baseline's by more than that spread.

  python scripts/nn_big_ab.py [--n 4096] [--k K] [--rounds 5] [--variants 0,3]
  python scripts/nn_big_ab.py --n 1024 --batch 1024 --reps 3 --warm 2 --variants 7,6
      (config 4: 1024 independent 1024^3 products, strict beta = 0)
"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from tensorium_amd.nnhip import TNNHip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--k", type=int, default=0, help="K of the n x n x K product (default n)")
ap.add_argument("--batch", type=int, default=1, help="strided-batched: independent n^3 products")
ap.add_argument("--beta", type=float, default=0.0)
ap.add_argument("--blas-beta0", action="store_true",
                help="beta = 0 by the BLAS convention (C not read) instead of the reference's 0*C")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--warm", type=int, default=30, help="untimed launches before each timed run")
ap.add_argument("--preheat-ms", type=float, default=300.0,
                help="launches before round 0 until this much GPU time has passed (warm clock)")
ap.add_argument("--variants", default="0,3", help="indices among the *_nn_big forms; first = baseline")
ap.add_argument("--out", default="", help="also write the JSON here")
a = ap.parse_args()
hip = TNNHip(0)
if a.blas_beta0:
    hip.lib.tns_set_option(0, 0)  # TNS_OPT_STRICT_BETA0
names = TNNHip.gemmVariants()
base = [i for i, nm in enumerate(names) if nm.endswith("nn_big")][0]
vs = [base + int(v) for v in a.variants.split(",")]
n, nb, k = a.n, a.batch, a.k or a.n
g = torch.Generator(device="cuda").manual_seed(1)
A = torch.rand(nb, n, k, device="cuda", generator=g) * 2 - 1
B = torch.rand(nb, k, n, device="cuda", generator=g) * 2 - 1
outs = {}
res = {names[v]: [] for v in vs}


def run(v, C):
    hip.gemmVariant(v, False, False, n, n, k, 1.0, A, 0, k, n * k, B, 0, n, k * n, a.beta, C, 0, n,
                    n * n, nb)


# (beta != 0 accumulates: the bit comparison is of this first launch from
# equal C; the timed launches only need C to stay finite, which beta <= 1 of
# operands in (-1, 1) does not promise for long — time beta = 0 or 1 over few reps)
for v in vs:
    C = torch.zeros(nb, n, n, device="cuda")
    run(v, C)
    torch.cuda.synchronize()
    outs[v] = C
ref = outs[vs[0]]
exact = {names[v]: bool(torch.equal(outs[v], ref)) for v in vs}
if nb > 1:  # one C for all: 4 GB each at config 4
    outs = {v: ref for v in vs}
heat = 0.0
while heat < a.preheat_ms:  # the clock ramps over the first launches: no round starts cold
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for v in vs:
        for _ in range(10):
            run(v, outs[v])
    e1.record()
    torch.cuda.synchronize()
    heat += e0.elapsed_time(e1)
for r in range(a.rounds):
    for v in vs:
        C = outs[v]
        for _ in range(a.warm):
            run(v, C)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            run(v, C)
        e1.record()
        torch.cuda.synchronize()
        res[names[v]].append(e0.elapsed_time(e1) / a.reps)


def median(x):
    s = sorted(x)
    return s[len(s) // 2]


b_ms = res[names[vs[0]]]
b_med, b_spread = median(b_ms), max(b_ms) - min(b_ms)
out = {"n": n, "k": k, "batch": nb, "beta": a.beta, "blas_beta0": a.blas_beta0, "rounds": a.rounds, "reps": a.reps,
       "baseline": names[vs[0]], "baseline_spread_ms": b_spread, "forms": {}}
for v in vs:
    ms = res[names[v]]
    med = median(ms)
    out["forms"][names[v]] = {
        "ms_rounds": [round(x, 5) for x in ms], "ms_median": med, "ms_min": min(ms),
        "spread_ms": max(ms) - min(ms), "tflops_median": 2 * n * n * k * nb / med / 1e9,
        "ratio_to_baseline": med / b_med, "faster_than_baseline": bool(b_med - med > b_spread),
        "bit_exact_vs_first": exact[names[v]]}
text = json.dumps(out, indent=1)
print(text)
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text + "\n")
