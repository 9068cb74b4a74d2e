"""Which kernels the conv dispatch picks, pinned without a GPU.

plan_conv_forward / plan_conv_backward (tensorium_amd/csrc/conv_api.cpp) are
pure host functions of the layer shape and the options.  tests/conv_plan_dump.cpp
calls them in libtensorium_hip.so and prints the plans; this test compiles it,
runs it once over every case below and checks

  * the default-option plans of every convolutional layer of the networks the
    project drives against tests/golden/conv_plans.json (every conv path is
    bit-exact against the oracle, so nothing else notices a changed pick);
  * that each forcing option gives its family and form, and -2 disables it;
  * that every plan is consistent in itself;
  * that planning is pure.

``python tests/test_conv_plan.py`` rewrites the golden file from the built
library; that is only right after a kernel trace has shown the library runs
the kernels the golden's author meant (conv dispatch).
"""
import json
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
GOLDEN = ROOT / "tests" / "golden" / "conv_plans.json"

# shapes for the forced options: batch C H W filters k stride pad dil act
L3X3 = (8, 64, 52, 52, 128, 3, 1, 1, 1, 7)      # 3x3 stride 1, k = 576
L3X3S2 = (8, 64, 52, 52, 128, 3, 2, 1, 1, 7)    # 3x3 stride 2
L1X1 = (8, 128, 26, 26, 256, 1, 1, 0, 1, 7)     # 1x1 stride 1 unpadded
LDIL = (8, 64, 52, 52, 128, 3, 1, 1, 2, 7)      # dilated: no fused / conv3 state.delta form


def _nets():
    from tensorium_amd import darknet as dn
    return [("yolov3-416", dn.yolov3_cfg(416), 1), ("yolov3-416", dn.yolov3_cfg(416), 8),
            ("yolov3-tiny-416", dn.yolov3_tiny_cfg(416), 1),
            ("cifar10-deep", dn.cifar10_deep_cfg(4), 4),
            ("lenet-cifar10", dn.lenet_cifar10_cfg(4), 4), ("lenet-mnist", dn.lenet_mnist_cfg(4), 4)]


def _fwd(cid, shape, fused=1, bias_act=1, aligned=1, **opts):
    return " ".join(["fwd", cid, *map(str, shape), str(fused), str(bias_act), str(aligned),
                     *(f"{k}={v}" for k, v in opts.items())])


def _bwd(cid, shape, bn=1, state_delta=1, aligned=1, **opts):
    return " ".join(["bwd", cid, *map(str, shape), str(int(bn)), str(int(state_delta)),
                     str(aligned), *(f"{k}={v}" for k, v in opts.items())])


def golden_cases():
    """Every convolutional layer of the driven networks, from darknet.Network:
    forward at fused = 1 (bias + activation fused unless batch norm follows),
    backward with the layer's batch norm, a state delta except for layer 0."""
    from tensorium_amd import darknet as dn
    lines = []
    for name, cfg, batch in _nets():
        net = dn.Network(dn.parse_cfg(cfg), batch)
        for l in net.layers:
            if l.kind != "convolutional":
                continue
            shape = (batch, l.c, l.h, l.w, l.filters, l.size, l.stride, l.pad, 1, l.activation)
            cid = f"{name}/b{batch}/L{l.index}"
            lines.append(_fwd(cid, shape, bias_act=int(not l.bn)))
            lines.append(_bwd(cid, shape, bn=l.bn, state_delta=l.index != 0))
    return lines


def _counts(lib):
    return {"tile": lib.tns_conv_tile_variant_count(), "slab": lib.tns_conv_slab_count(),
            "conv1x1": lib.tns_conv1x1_count(), "dw_tile": lib.tns_conv_dw_tile_count(),
            "dw_res": lib.tns_conv_dw_res_count(), "dx_tile": lib.tns_conv_dx_tile_count(),
            "dx_conv": lib.tns_conv_dx_conv_count()}


def forced_cases(n):
    lines = []
    for v in range(n["tile"]):
        lines.append(_fwd(f"force/tile/{v}", L3X3, conv_variant=100 + v))
    for v in range(n["slab"]):
        lines.append(_fwd(f"force/slab/{v}", L3X3, conv_variant=500 + v))
    for v in range(n["conv1x1"]):
        lines.append(_fwd(f"force/conv1x1/{v}", L1X1, conv_variant=600 + v))
    for v in range(n["dw_tile"]):
        lines.append(_bwd(f"force/dw_tile/{v}", L3X3, dw_tile=v))
    for v in range(n["dw_res"]):
        lines.append(_bwd(f"force/dw_res/{v}", L3X3, dw_res=v))
    for v in range(n["dx_tile"]):
        lines.append(_bwd(f"force/dx_tile/{v}", LDIL, dx_tile=v))
    for v in range(n["dx_conv"]):
        lines.append(_bwd(f"force/dx_conv/{v}", L3X3, dx_conv=v))
        lines.append(_bwd(f"force/dx_conv_s2/{v}", L3X3S2, dx_conv=v))
    lines.append(_fwd("force/600_on_3x3", L3X3, conv_variant=600))
    lines.append(_fwd("force/removed_250", L3X3, conv_variant=250))
    lines.append(_bwd("off/dx_tile", LDIL, dx_tile=-2))
    return lines


def build_dumper(out_dir: Path) -> Path:
    from tensorium_amd import build
    exe = out_dir / "conv_plan_dump"
    pkg = build.LIB.parent
    subprocess.run([build.HIPCC, "-O1", "-std=c++17", "-Wall", "-Wno-unused-function",
                    "-Wno-unused-value", "-Wno-unused-result",
                    str(ROOT / "tests" / "conv_plan_dump.cpp"), "-o", str(exe), f"-L{pkg}",
                    "-ltensorium_hip", f"-Wl,-rpath,{pkg}"], check=True)
    return exe


def run_dumper(exe: Path, lines: list[str]) -> list[dict]:
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = [json.loads(l) for l in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def _keyed(plans):
    return {f"{p['kind']} {p['id']}": {k: v for k, v in p.items() if k not in ("id", "kind")}
            for p in plans}


@pytest.fixture(scope="module")
def dumper(hiplib, tmp_path_factory):
    return build_dumper(tmp_path_factory.mktemp("conv_plan"))


@pytest.fixture(scope="module")
def golden_plans():
    """The file lists each distinct plan once, with the layers that get it."""
    groups = json.loads(GOLDEN.read_text())
    plans = {k: g["plan"] for g in groups for k in g["layers"]}
    assert len(plans) == sum(len(g["layers"]) for g in groups)  # no layer listed twice
    return plans


@pytest.fixture(scope="module")
def plans(hiplib, dumper):
    """One run of the dumper over the golden cases, then the forced ones."""
    g, f = golden_cases(), forced_cases(_counts(hiplib))
    out = run_dumper(dumper, g + f)
    return _keyed(out[:len(g)]), _keyed(out[len(g):])


def test_default_plans_match_golden(plans, golden_plans):
    got = plans[0]
    assert len(got) > 2 * (75 + 75 + 13)  # both passes of every layer listed
    assert sorted(got) == sorted(golden_plans)
    diff = {k: (got[k], golden_plans[k]) for k in got if got[k] != golden_plans[k]}
    assert not diff, f"{len(diff)} plans changed, e.g. {next(iter(diff.items()))}"


def test_forced_options_give_their_family_and_form(plans, hiplib):
    f, n = plans[1], _counts(hiplib)
    assert all(c > 0 for c in n.values()), n
    for fam, path in (("tile", "tile"), ("slab", "slab"), ("conv1x1", "conv1x1")):
        for v in range(n[fam]):
            p = f[f"fwd force/{fam}/{v}"]
            assert (p["err"], p["path"], p["form"]) == (0, path, v), (fam, v, p)
    for v in range(n["dw_tile"]):
        p = f[f"bwd force/dw_tile/{v}"]
        assert (p["dw"]["path"], p["dw"]["form"]) == ("tile", v), p
    for v in range(n["dw_res"]):
        p = f[f"bwd force/dw_res/{v}"]
        assert (p["dw"]["path"], p["dw"]["form"], p["dw_res_forced"]) == ("res", v, True), p
    for v in range(n["dx_tile"]):
        p = f[f"bwd force/dx_tile/{v}"]
        assert (p["dx"], p["dx_form"], p["dx_tile"], p["dx_tile_forced"]) == ("tile", v, v, True), p
    for v in range(n["dx_conv"]):
        p, q = f[f"bwd force/dx_conv/{v}"], f[f"bwd force/dx_conv_s2/{v}"]
        assert (p["dx"], p["dx_form"]) == ("conv3", v), p
        assert (q["dx"], q["dx_form"]) == ("conv3s2", v), q
    p = f["fwd force/600_on_3x3"]
    assert p["err"] == 4 and p["msg"] == "conv1x1 forms need a 1x1 stride-1 unpadded layer", p
    p = f["fwd force/removed_250"]
    assert p["err"] == 4 and p["msg"] == ("conv variant 250: the ping-pong, LDS-DMA-ring and "
                                          "input-patch tile families (200..499) were removed"), p
    p = f["bwd off/dx_tile"]
    assert (p["dx"], p["dx_tile"]) == ("tn", -1), p


def _shape_of(golden_lines, key):
    kind, cid = key.split()
    line = next(l for l in golden_lines if l.split()[:2] == [kind, cid])
    return " ".join(line.split()[2:])


@pytest.mark.parametrize("opt,taken", [
    ("dw_res", lambda p: p["dw"]["path"] == "res"),
    ("dw_tile", lambda p: "tile" in (p["dw"]["path"], p["dw_fallback"]["path"])),
    ("dx_tile", lambda p: p["dx"] == "tile"),
    ("dx_conv", lambda p: p["dx"] in ("conv3", "conv3s2")),
])
def test_minus_two_disables_the_family(opt, taken, plans, dumper):
    """On a layer whose default plan takes the family, option = -2 does not."""
    lines = golden_cases()
    key = next((k for k, p in plans[0].items() if k.startswith("bwd") and taken(p)), None)
    if key is None:
        pytest.fail(f"no layer takes {opt}'s family by default")
    kind, cid = key.split()
    (p,) = run_dumper(dumper, [f"{kind} {cid} {_shape_of(lines, key)} {opt}=-2"])
    assert p["err"] == 0 and not taken(p), p


def test_plans_are_consistent(plans):
    for key, p in {**plans[0], **plans[1]}.items():
        if p["err"] or p.get("empty"):
            continue
        if key.startswith("fwd"):
            if p["path"] != "implicit":  # (there -1 leaves the tile to the GEMM's heuristic)
                assert (p["form"] >= 0) == (p["path"] in ("conv1x1", "slab", "tile")), (key, p)
            assert (p["col_elems"] > 0) == (p["path"] == "slab" or
                                            (p["path"] == "im2col" and p["needs_col"])), (key, p)
            if p["stage1_elems"] > 0:
                assert p["path"] == "implicit" and p["padded"], (key, p)
            assert (p["chunk"] >= 1) == (p["path"] in ("tile", "implicit")), (key, p)
            continue
        dw, fb = p["dw"], p["dw_fallback"]
        for d in (dw, fb):  # one path each; a form where the family has forms
            assert d["path"] in ("res", "tile", "sdot", "gemm"), (key, p)
            assert (d["form"] >= 0) == (d["path"] in ("res", "tile")), (key, p)
            assert d["col"] == (p["needs_col"] and d["path"] in ("sdot", "gemm")), (key, p)
            assert (d["part_elems"] > 0) == (d["path"] != "gemm"), (key, p)
        assert fb["path"] != "res", (key, p)  # a residue plan names where it falls back to
        assert (dw["path"] == "res") == (p["res_a_elems"] > 0) == (p["res_b_elems"] > 0), (key, p)
        if dw["path"] != "res":
            assert dw == fb and not p["dw_res_forced"], (key, p)
        dx = p["dx"]
        assert (p["dx_form"] >= 0) == (dx in ("conv1x1", "conv3", "conv3s2", "tile")), (key, p)
        assert p["dx_col"] == (dx in ("tile", "tn") and not p["dx_direct"]), (key, p)
        if dx == "conv1x1":
            assert p["dx_direct"], (key, p)
        if dx == "tile":
            assert p["dx_tile"] == p["dx_form"], (key, p)
        assert (p["wt_elems"] > 0) == (dx in ("conv1x1", "fused", "conv3", "conv3s2")), (key, p)
        if dx == "none":  # no state delta: nothing of dX is planned
            assert (p["dx_tile"], p["dx_col"], p["dx_direct"], p["wt_elems"]) == \
                (-1, False, False, 0), (key, p)
        assert p["bn_elems"] > 0, (key, p)
        assert (p["col_elems"] > 0) == (dw["col"] or fb["col"] or p["dx_col"]), (key, p)


def test_layer_zero_has_no_state_delta_plan(plans):
    zeros = [p for k, p in plans[0].items() if k.startswith("bwd") and k.endswith("/L0")]
    assert len(zeros) == len(_nets())
    assert all(p["dx"] == "none" for p in zeros)
    assert all(p["dx"] != "none" for k, p in plans[0].items()
               if k.startswith("bwd") and not k.endswith("/L0"))


def test_planning_is_pure(dumper):
    a, b = _bwd("a", L3X3), _fwd("a", L1X1)
    other = [_bwd("x", LDIL, dw_res=0, bwd_overlap=2), _fwd("x", L3X3, conv_variant=250)]
    out = run_dumper(dumper, [a, b, *other, a, b])
    assert out[0] == out[-2] and out[1] == out[-1]


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        got = _keyed(run_dumper(build_dumper(Path(d)), golden_cases()))
    groups = {}
    for k in sorted(got):
        groups.setdefault(json.dumps(got[k], sort_keys=True), []).append(k)
    GOLDEN.write_text("[\n" + ",\n".join(f'{{"layers": {json.dumps(ks)},\n "plan": {p}}}'
                                         for p, ks in groups.items()) + "\n]\n")
    print(f"{len(got)} layers, {len(groups)} distinct plans -> {GOLDEN}")
