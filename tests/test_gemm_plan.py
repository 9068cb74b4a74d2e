"""Which kernel the SGEMM dispatch picks, pinned without a GPU.

plan_gemm (tensorium_amd/csrc/gemm_plan.cpp) is a pure host function of the
problem's shape and the options; tns_gemm_plan is its C entry point.
tests/gemm_plan_dump.cpp calls it in libtensorium_hip.so and prints the plans;
this test compiles it, runs it once over every case below and checks

  * the default-option plans of the GEMMs the project issues against
    tests/golden/gemm_plans.json (every path is bit-exact against the oracle,
    so nothing else notices a changed pick);
  * that every table variant and every large-NN form, forced, gives its own
    family and form where it supports the problem and "unsupported" where its
    KIND or `applies` rule says so (the expectation is tests/_gemm_cases.py's
    support table, never the library's word);
  * for each numeric rule of the three pickers, one shape on either side of the
    threshold: the two plans differ;
  * that planning is pure, and that every leaf the library exports is reached
    by a GPU case of tests/test_gpu_gemm_variants.py.

``python tests/test_gemm_plan.py`` rewrites the golden file from the built
library; that is only right after a kernel trace has shown the library runs
the kernels the golden's author meant (GEMM dispatch).
"""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _gemm_cases as gc  # noqa: E402
from tensorium_amd._abi import GEMM_PLAN_FIELDS  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "gemm_plans.json"
CONV_GOLDEN = ROOT / "tests" / "golden" / "conv_plans.json"


def _line(cid, variant=-1, **kw):
    """One dumper line; the defaults of tensorium_amd._abi.gemm_plan."""
    v = dict(strideA=0, strideB=0, strideC=0, batch=1, alpha1=1, beta_mode=2, epi=0, a16=1, b16=1,
             nt_sdot=1, tt_exact=1, sdot_form=-1)
    v.update(kw)
    v.setdefault("lda", v["M"] if v["transA"] else v["K"])
    v.setdefault("ldb", v["K"] if v["transB"] else v["N"])
    v.setdefault("ldc", v["N"])
    assert " " not in cid
    return " ".join([cid, str(variant), *(str(int(v[k])) for k in GEMM_PLAN_FIELDS)])


def _case_line(c: gc.Case):
    a = c.plan_args()
    return _line(c.id, a.pop("variant"), **a)


def _g(cid, ta, tb, M, N, K, beta=0.0, **kw):
    """A GEMM as the Python driver issues it: BETA = 0 is scaled (strict), 1 read."""
    return _line(cid, transA=ta, transB=tb, M=M, N=N, K=K, beta_mode=1 if beta == 1.0 else 2, **kw)


def _sub_layer(cid, S, I, O):
    """A connected (sub-)layer over S rows: forward, dW, dX
    (darknet/connected.py, forward / backward)."""
    return [_g(f"{cid}/fwd", 0, 1, S, O, I), _g(f"{cid}/dW", 1, 0, O, I, S, 1.0),
            _g(f"{cid}/dX", 0, 0, S, I, O, 1.0)]


def _recurrent(cid, l, T, S):
    I, O = l.in_size, l.filters
    n = S * O
    if l.kind == "lstm":  # the fused-gate path: four gates as one strided batch
        return [
            _g(f"{cid}/fwd-u", 0, 1, T * S, O, I, strideB=O * I, strideC=T * n, batch=4),
            _g(f"{cid}/fwd-w", 0, 1, S, O, O, strideB=O * O, strideC=T * n, batch=4),
            _g(f"{cid}/dW-w", 1, 0, O, O, S, 1.0, strideA=T * n, strideC=O * O, batch=4),
            _g(f"{cid}/dW-u", 1, 0, O, I, S, 1.0, strideA=T * n, strideC=O * I, batch=4),
            _g(f"{cid}/dH", 0, 0, S, O, O, 1.0), _g(f"{cid}/dX", 0, 0, T * S, I, O, 1.0),
            *_sub_layer(f"{cid}/step-u", S, I, O), *_sub_layer(f"{cid}/step-w", S, O, O)]
    H = l.hidden
    return [_g(f"{cid}/fwd-in", 0, 1, T * S, H, I), _g(f"{cid}/fwd-self", 0, 1, S, H, H),
            _g(f"{cid}/fwd-out", 0, 1, T * S, O, H), _g(f"{cid}/dX", 0, 0, T * S, I, H, 1.0),
            *_sub_layer(f"{cid}/step-in", S, I, H), *_sub_layer(f"{cid}/step-self", S, H, H),
            *_sub_layer(f"{cid}/step-out", S, H, O)]


def golden_cases():
    """The GEMMs the project issues, at default options."""
    import test_conv_plan as tcp
    from tensorium_amd import darknet as dn
    lines = [_g("bench/sgemm-4096", 0, 0, 4096, 4096, 4096),
             _g("bench/batched-1024x1024", 0, 0, 1024, 1024, 1024, strideA=1 << 20,
                strideB=1 << 20, strideC=1 << 20, batch=1024)]
    nets = [(name, dn.Network(dn.parse_cfg(cfg), batch)) for name, cfg, batch in tcp._nets()]
    nets.append(("char-lstm", dn.Network(dn.parse_cfg(dn.lstm_cfg(batch=32, time_steps=16)))))
    nets.append(("char-rnn", dn.Network(dn.parse_cfg(dn.rnn_cfg(batch=32, time_steps=16)), None,
                                        rnn=True)))
    for name, net in nets:
        for l in net.layers:
            cid = f"{name}/b{net.batch}/L{l.index}"
            if l.kind == "connected":
                lines += _sub_layer(cid, net.batch, l.in_size, l.filters)
            elif l.kind in ("lstm", "rnn"):
                lines += _recurrent(cid, l, l.steps, net.batch // l.steps)
    # the conv paths that end in a GEMM, from the golden conv plans
    conv = {k: g["plan"] for g in json.loads(CONV_GOLDEN.read_text()) for k in g["layers"]}
    for ln in tcp.golden_cases():
        f = ln.split()
        kind, cid = f[0], f[1]
        batch, C, H, W, F, k, stride, pad, dil = map(int, f[2:11])
        p = conv[f"{kind} {cid}"]
        oh = (H + 2 * pad - (dil * (k - 1) + 1)) // stride + 1
        ow = (W + 2 * pad - (dil * (k - 1) + 1)) // stride + 1
        m, n, kk = F, C * k * k, oh * ow  # dW is m x n over kk pixels
        if kind == "fwd":
            # tns_hip_conv2d (and the unfused forward): im2col, then one
            # strided-batched NN with the weights shared (strideA = 0); no
            # default forward plan ends in a GEMM, this entry point always does
            lines.append(_line(f"conv2d/{cid}", transA=0, transB=0, M=m, N=kk, K=n, strideB=n * kk,
                               strideC=m * kk, batch=batch, beta_mode=0))
            continue
        # dW as NT through launch_sgemm_nt_sdot: the plan's own path, or the one
        # a residue plan falls back to when its scratch is refused
        dw, tag = (p["dw"], "conv-dW") if p["dw"]["path"] != "res" else \
            (p["dw_fallback"], "conv-dW-fallback")
        if dw["path"] == "sdot":  # one batched launch, products stored
            lines.append(_line(f"{tag}/{cid}", transA=0, transB=1, M=m, N=n, K=kk,
                               strideA=m * kk, strideB=n * kk, strideC=m * n, batch=batch,
                               beta_mode=3))
        if dw["path"] == "gemm":  # image by image into weight_updates
            lines.append(_line(f"{tag}/{cid}", transA=0, transB=1, M=m, N=n, K=kk, beta_mode=1))
        if p["dx"] == "tn":
            lines.append(_line(f"conv-dX/{cid}", transA=1, transB=0, M=n, N=kk, K=m, strideB=m * kk,
                               strideC=n * kk, batch=batch, beta_mode=0,
                               epi=2 if p["dx_direct"] else 0))
    ids = [l.split()[0] for l in lines]
    assert len(ids) == len(set(ids))
    return lines


# ---- forced variants --------------------------------------------------------------------
# problems for the forced variants: aligned multiples of every tile, ragged
# ones, each transpose, a misaligned A, an odd leading dimension, a bad stride
FORCED_PROBLEMS = [
    dict(M=512, N=768, K=96), dict(M=512, N=768, K=96, ta=1), dict(M=512, N=768, K=96, tb=1),
    dict(M=512, N=768, K=96, ta=1, tb=1), dict(M=512, N=768, K=100), dict(M=516, N=768, K=96),
    dict(M=512, N=770, K=96), dict(M=512, N=768, K=96, offA=1), dict(M=512, N=768, K=96, offB=2),
    dict(M=512, N=768, K=96, lda=97), dict(M=512, N=768, K=96, ldb=772),
    dict(M=512, N=768, K=96, batch=2, strideA=512 * 96 + 2),
    dict(M=512, N=768, K=96, batch=2, strideB=0), dict(M=37, N=53, K=61),
    dict(M=256, N=256, K=32, ldc=2097152), dict(M=256, N=256, K=32, lda=67108864),
]


def forced_cases():
    out = []
    for v, name in enumerate(gc.VARIANT_NAMES):
        for i, pr in enumerate(FORCED_PROBLEMS):
            out.append(gc.Case(f"forced/{name}/{i}", variant=v, **{"ta": 0, "tb": 0, **pr}))
    return out


# ---- threshold edges: (rule, below, above) — the plans on the two sides differ ----------
def _nn(M, N, K, **kw):
    return dict(transA=0, transB=0, M=M, N=N, K=K, **kw)


def _tn(M, N, K, **kw):
    return dict(transA=1, transB=0, M=M, N=N, K=K, **kw)


def _nt(M, N, K, **kw):
    return dict(transA=0, transB=1, M=M, N=N, K=K, **kw)


_MF = dict(nt_sdot=0)  # the MFMA kernel's NT: pick_tile_variant's last rules
EDGES = [
    # pick_tile_variant, TN
    ("tile/tn/K<=1024", _tn(2048, 2048, 1024), _tn(2048, 2048, 1028)),
    ("tile/tn/M>64", _tn(64, 4096, 512), _tn(65, 4096, 512)),
    ("tile/tn/blocks64<512", _tn(1024, 1984, 512), _tn(1024, 2048, 512)),
    ("tile/tn/K>=1024", _tn(2048, 2048, 1020), _tn(2048, 2048, 1024)),
    ("tile/tn/blocks256>=240", _tn(3840, 3840, 512), _tn(3840, 4096, 512)),
    # pick_tile_variant, NN (K = 40: no large-NN form)
    ("tile/nn/M<=32:K<32", _nn(32, 1000, 31), _nn(32, 1000, 32)),
    ("tile/nn/M<=32:blocks32x64>=1024", _nn(32, 65472, 40), _nn(32, 65536, 40)),
    ("tile/nn/M<=32", _nn(32, 65536, 40), _nn(33, 65536, 40)),
    ("tile/nn/M<=64:b64>=600", _nn(64, 38336, 40), _nn(64, 38400, 40)),
    ("tile/nn/M<=64", _nn(64, 38400, 40), _nn(65, 38400, 40)),
    ("tile/nn/b64>=1200", _nn(128, 38336, 1024), _nn(128, 38400, 1024)),
    ("tile/nn/b64>=1200:K>=1024", _nn(128, 38400, 1020), _nn(128, 38400, 1024)),
    ("tile/nn/b64>=600", _nn(128, 19136, 40), _nn(128, 19200, 40)),
    ("tile/nn/b64>=256", _nn(128, 8128, 40), _nn(128, 8192, 40)),
    ("tile/nn/K<2048", _nn(128, 8192, 2044), _nn(128, 8192, 2048)),
    ("tile/nn/blocks256>=240", _nn(3840, 3840, 40), _nn(3840, 4096, 40)),
    # pick_tile_variant, a transposed B
    ("tile/nt/M<=32", _nt(32, 300, 40, **_MF), _nt(33, 300, 40, **_MF)),
    ("tile/nt/M<=64", _nt(64, 300, 40, **_MF), _nt(65, 300, 40, **_MF)),
    ("tile/nt/blocks256>=240", _nt(256, 256, 40, batch=239, strideA=10240, strideB=10240, **_MF),
     _nt(256, 256, 40, batch=240, strideA=10240, strideB=10240, **_MF)),
    ("tile/nt/M>=256", _nt(255, 256, 40, batch=240, strideA=10240, strideB=10240, **_MF),
     _nt(256, 256, 40, batch=240, strideA=10240, strideB=10240, **_MF)),
    ("tile/nt/N>=1024", _nt(65, 1023, 40, **_MF), _nt(65, 1024, 40, **_MF)),
    # nn_big_pick and the w4 kernel's template choices
    ("nn_big/tiles>=192", _nn(4096, 2816, 256), _nn(4096, 3072, 256)),
    ("nn_big/w4:C-offsets-32-bit", _nn(256, 256, 64, batch=192, ldc=2097150),
     _nn(256, 256, 64, batch=192, ldc=2097151)),
    ("nn_big/w4:A-offsets-32-bit", _nn(256, 256, 64, batch=192, lda=67108860),
     _nn(256, 256, 64, batch=192, lda=67108864)),
    ("nn_big/w4:rows-from-4-k-tiles", _nn(4096, 3072, 96), _nn(4096, 3072, 128)),
    ("nn_big/w4:pre-from-8-k-tiles", _nn(4096, 3072, 224), _nn(4096, 3072, 256)),
    # plan_gemm_nt_sdot
    ("nt_sdot/chains:K>=4096", _nt(32, 27, 4092), _nt(32, 27, 4096)),
    ("nt_sdot/chains:t32<=64", _nt(256, 256, 4096), _nt(256, 257, 4096)),
    ("nt_sdot/chains:outs<=8192", _nt(32, 256, 4096), _nt(32, 257, 4096)),
    ("nt_sdot/chains:outs<=32768", _nt(128, 256, 4096), _nt(128, 257, 4096)),
    ("nt_sdot/rc:K<=1024", _nt(1000, 2100, 1024), _nt(1000, 2100, 1028)),
    ("nt_sdot/rc:t64>=512", _nt(1024, 1984, 40), _nt(1024, 2048, 40)),
    ("nt_sdot/rc:31-bit-offsets", _nt(1000, 2100, 40, lda=475948), _nt(1000, 2100, 40, lda=475952)),
    ("nt_sdot/tn:b64>=1024", _nt(1024, 1984, 1028), _nt(1024, 2048, 1028)),
    ("nt_sdot/tn:o32", _nt(1000, 2100, 1029, lda=2149632), _nt(1000, 2100, 1029, lda=2149633)),
    ("nt_sdot/tn:K>=16384", _nt(288, 250, 16380), _nt(288, 250, 16384)),
    ("nt_sdot/tn:t32<512", _nt(512, 992, 16384), _nt(512, 1024, 16384)),
    # plan_gemm_tt
    ("tt/b128>=512", dict(transA=1, transB=1, M=128, N=128, K=40, batch=511),
     dict(transA=1, transB=1, M=128, N=128, K=40, batch=512)),
]


def edge_cases():
    out = []
    for rule, lo, hi in EDGES:
        out += [_line(f"edge/{rule}/below", **lo), _line(f"edge/{rule}/above", **hi)]
    return out


# ---- the dumper ----------------------------------------------------------------------------
def build_dumper(out_dir: Path) -> Path:
    from tensorium_amd import build
    exe = out_dir / "gemm_plan_dump"
    pkg = build.LIB.parent
    subprocess.run([build.HIPCC, "-O1", "-std=c++17", "-Wall", str(ROOT / "tests" /
                                                                      "gemm_plan_dump.cpp"),
                    "-o", str(exe), f"-L{pkg}", "-ltensorium_hip", f"-Wl,-rpath,{pkg}"], check=True)
    return exe


def run_dumper(exe: Path, lines: list[str]) -> dict:
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = [json.loads(l) for l in r.stdout.splitlines()]
    assert [p["id"] for p in out] == [l.split()[0] for l in lines]
    return {p.pop("id"): p for p in out}


@pytest.fixture(scope="module")
def dumper(hiplib, tmp_path_factory):
    return build_dumper(tmp_path_factory.mktemp("gemm_plan"))


@pytest.fixture(scope="module")
def gpu_cases():
    return gc.all_cases()


@pytest.fixture(scope="module")
def plans(dumper, gpu_cases):
    """One run of the dumper over every case of this file and of the GPU test."""
    groups = [golden_cases(), [_case_line(c) for c in forced_cases()], edge_cases(),
              [_case_line(c) for c in gpu_cases]]
    out = run_dumper(dumper, [l for g in groups for l in g])
    assert len(out) == sum(map(len, groups))  # no id twice
    return [{l.split()[0]: out[l.split()[0]] for l in g} for g in groups]


@pytest.fixture(scope="module")
def golden_plans():
    """The file lists each distinct plan once, with the GEMMs that get it."""
    groups = json.loads(GOLDEN.read_text())
    plans = {k: g["plan"] for g in groups for k in g["gemms"]}
    assert len(plans) == sum(len(g["gemms"]) for g in groups)
    return plans


def test_default_plans_match_golden(plans, golden_plans):
    got = plans[0]
    assert len(got) > 150
    odd = sorted(set(got) ^ set(golden_plans))
    assert not odd, f"GEMMs in the cases or in the golden file only: {odd}"
    diff = {k: (got[k], golden_plans[k]) for k in got if got[k] != golden_plans[k]}
    assert not diff, f"{len(diff)} plans changed, e.g. {next(iter(diff.items()))}"
    # the paths the golden is there to pin are all in it
    fams = {p["family"] for p in got.values()}
    assert {"tile", "nn_big", "nt_sdot", "sdot_chains", "sdot_rc"} <= fams, fams
    for tag in ("bench/", "conv2d/", "conv-dW/", "conv-dW-fallback/", "conv-dX/", "char-lstm/",
                "char-rnn/", "cifar10-deep/"):
        assert any(k.startswith(tag) for k in got), tag


def test_forced_variants_give_their_form_or_refuse(plans):
    f = plans[1]
    nb = len(gc.TILES)
    took = {v: 0 for v in range(len(gc.VARIANT_NAMES))}
    for c in forced_cases():
        p = f[c.id]
        if gc.supported(c):
            want = ("tile", c.variant) if c.variant < nb else ("nn_big", c.variant - nb)
            assert (p["err"], p["family"], p["form"]) == (0, *want), (c.id, p)
            assert p["name"] == gc.VARIANT_NAMES[c.variant] and p["leaf"], (c.id, p)
            took[c.variant] += 1
        else:
            assert p["err"] == 4 and p["msg"] and p["leaf"] == "", (c.id, p)
    # no variant refuses everything, none takes everything it is meant to refuse
    assert all(n > 0 for n in took.values()), took
    for v, name in enumerate(gc.VARIANT_NAMES):
        kind = gc.TILES[v][5] if v < nb else "nn_big"
        assert (took[v] == len(FORCED_PROBLEMS)) == (kind == "full"), (name, took[v])


@pytest.mark.parametrize("rule", [e[0] for e in EDGES])
def test_threshold_edges(plans, rule):
    lo, hi = plans[2][f"edge/{rule}/below"], plans[2][f"edge/{rule}/above"]
    assert lo["err"] == 0 and hi["err"] == 0, (lo, hi)
    assert lo != hi, f"{rule}: the same plan on both sides: {lo}"


def test_planning_is_pure(dumper, plans):
    lines = golden_cases()[:40] + edge_cases()
    a = run_dumper(dumper, lines)
    b = run_dumper(dumper, list(reversed(lines)) + lines)
    assert a == b
    assert all(a[k] == {**plans[0], **plans[2]}[k] for k in a)


def test_bad_arguments_are_rejected(dumper):
    out = run_dumper(dumper, [_line("bad-beta", transA=0, transB=0, M=8, N=8, K=8, beta_mode=7),
                              _line("bad-variant", 99, transA=0, transB=0, M=8, N=8, K=8)])
    assert "rejected" in out["bad-beta"] and "rejected" in out["bad-variant"]


def test_every_leaf_is_reached_by_a_gpu_case(plans, hiplib, gpu_cases):
    """The census: the leaves the GPU cases reach, against the exported list.
    A leaf no case reaches fails here by name, so a new kernel form cannot
    arrive untested.  The one exemption is named, with its size, in
    _gemm_cases.EXEMPT."""
    leaves = [hiplib.tns_gemm_plan_leaf_name(i).decode()
              for i in range(hiplib.tns_gemm_plan_leaf_count())]
    assert len(leaves) == len(set(leaves)) and all(leaves)
    reached = {p["leaf"] for p in plans[3].values() if p["err"] == 0}
    everywhere = reached | {p["leaf"] for g in plans[:3] for p in g.values() if p["err"] == 0}
    assert everywhere - {""} <= set(leaves), everywhere - set(leaves)
    missing = [l for l in leaves if l not in reached and l not in gc.EXEMPT]
    assert not missing, f"plan leaves no GPU case reaches: {missing}"
    assert list(gc.EXEMPT) == ["nt_sdot/tn<2,1,64>"]
    assert not set(gc.EXEMPT) & reached, "an exempt leaf is reached: drop the exemption"
    # a GPU case the support table marks unsupported is one the planner refuses
    for c in gpu_cases:
        assert (plans[3][c.id]["err"] == 0) == gc.supported(c), c.id
    # the leaves the named cases promise
    for c, leaf in gc.leaf_cases():
        assert plans[3][c.id]["leaf"] == leaf, (c.id, plans[3][c.id])
    for c, tile in gc.option_cases():
        assert plans[3][c.id]["name"] == tile, (c.id, plans[3][c.id])


def test_matrix_makes_operands_scalar_for_every_reason():
    """Each of the four reasons an operand is not staged by float4 occurs for
    A and for B under both values of that operand's transpose."""
    seen = set()
    for v in range(len(gc.TILES)):
        for c in gc.matrix_cases(v):
            if not gc.supported(c):
                continue
            for who, t in (("A", c.ta), ("B", c.tb)):
                if who in c.why:
                    seen.add((who, t, c.why[who]))
    want = {(w, t, r) for w in "AB" for t in (0, 1) for r in gc.REASONS}
    assert want <= seen, sorted(want - seen)


def test_oracle_nt_and_tt_orders_differ_from_the_ascending_chain(ora):
    """The GPU test compares the MFMA kernel's NT / TT with the oracle's NN / TN
    on a materialised B^T.  That only tells the kernel's order from the
    reference's own NT (sdot) and TT (unfused) orders if those differ at the
    shapes used: they do, at every option case and every matrix NT / TT case
    sampled here."""
    import test_gpu_gemm_variants as tv
    cases = [c for c, _ in gc.option_cases()]
    cases += [c for c in gc.matrix_cases(0) + gc.matrix_cases(13) if c.tb and c.id.endswith("ab1")]
    assert len(cases) >= 20
    for c in cases:
        A, B, C0 = tv.operands(c)
        asc = tv.reference(ora, c, A, B, C0)
        own = tv.reference(ora, gc.replace(c, variant=-1, nt_sdot=1, tt_exact=1), A, B, C0)
        assert not np.array_equal(asc, own), c.id


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        got = run_dumper(build_dumper(Path(d)), golden_cases())
    groups = {}
    for k in got:
        groups.setdefault(json.dumps(got[k], sort_keys=True), []).append(k)
    GOLDEN.write_text("[\n" + ",\n".join(f'{{"gemms": {json.dumps(ks)},\n "plan": {p}}}'
                                         for p, ks in groups.items()) + "\n]\n")
    print(f"{len(got)} GEMMs, {len(groups)} distinct plans -> {GOLDEN}")
