"""The darknet drivers' backend call sequence, recorded without a GPU (test
infrastructure for tests/test_driver_calls.py and
tests/golden/make_driver_calls.py).

``Recorder`` stands in for ``TNNHip``: every method call becomes one line, the
method name and then its arguments,

* a tensor as ``b<k>+<element offset>``: k numbers the storages in order of
  first appearance in the trace, the base is ``untyped_storage().data_ptr()``,
  the offset counts 4-byte elements;
* a raw address (what ``_at`` returns, or ``counts.data_ptr()``) resolved
  against the storages seen or registered and rendered like a tensor: the ABI
  sees only the address;
* a sequence element-wise, a NumPy array as a digest of its bytes, a scalar by
  ``repr`` (NumPy scalars as the Python value), keyword arguments as
  ``name=value`` in name order.

Every traced tensor is kept alive for the life of the recorder, so no address
is reused within a case.

``CASES`` are tiny networks with fixed seeds, driven on CPU tensors
(``device = "cpu"``) by phase: ``forward``, ``backward``, ``update``; an
inference case is one ``forward``.  The values in the buffers do not matter:
nothing computes.
"""
from __future__ import annotations

import functools
import hashlib
import sys
from collections import Counter
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


class Recorder:
    def __init__(self):
        self.phases = {}      # phase -> lines
        self.lines = None
        self.keep = []        # every tensor traced or registered
        self.seen = {}        # storage base address -> (k, bytes)
        self.registered = {}  # storage base address -> bytes, not yet in the trace

    def phase(self, name):
        self.lines = self.phases.setdefault(name, [])

    def register(self, obj):
        """Every tensor under obj (dicts, lists, tuples, object attributes one
        level deep), so that a raw address into it resolves."""
        if isinstance(obj, Recorder):
            return
        if hasattr(obj, "untyped_storage"):
            s = obj.untyped_storage()
            self.keep.append(obj)
            self.registered.setdefault(s.data_ptr(), s.nbytes())
        elif isinstance(obj, dict):
            for v in obj.values():
                self.register(v)
        elif isinstance(obj, (list, tuple)):
            for v in obj:
                self.register(v)

    def _storage(self, base, nbytes):
        if base not in self.seen:
            self.seen[base] = (len(self.seen), nbytes)
            self.registered.pop(base, None)
        return self.seen[base][0]

    def _address(self, a):
        for base, (k, nbytes) in self.seen.items():
            if base <= a < base + max(nbytes, 1):
                return f"b{k}+{(a - base) // 4}"
        for base, nbytes in list(self.registered.items()):
            if base <= a < base + max(nbytes, 1):
                return f"b{self._storage(base, nbytes)}+{(a - base) // 4}"
        return None

    def render(self, v):
        if hasattr(v, "untyped_storage"):
            s = v.untyped_storage()
            self.keep.append(v)
            k = self._storage(s.data_ptr(), s.nbytes())
            return f"b{k}+{(v.data_ptr() - s.data_ptr()) // 4}"
        if isinstance(v, np.ndarray):
            return "nd:" + hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()[:16]
        if isinstance(v, np.generic):
            v = v.item()
        if isinstance(v, (list, tuple)):
            return "[" + ",".join(self.render(e) for e in v) + "]"
        if isinstance(v, int) and not isinstance(v, bool):
            r = self._address(v)
            if r is not None:
                return r
            if v >= 1 << 40:
                raise AssertionError(f"an address {v:#x} into no known storage")
        return repr(v)

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*args, **kw):
            parts = [name, *(self.render(a) for a in args),
                     *(f"{k}={self.render(kw[k])}" for k in sorted(kw))]
            self.lines.append(" ".join(parts))

        return call


def summary(lines):
    return {"calls": len(lines),
            "methods": dict(sorted(Counter(l.split(" ", 1)[0] for l in lines).items())),
            "sha256": hashlib.sha256("\n".join(lines).encode()).hexdigest()}


# ---- cases ------------------------------------------------------------------

def _fc_cfg(widths, acts, bn, B, head):
    body = "".join(f"[connected]\noutput={o}\nactivation={a}\nbatch_normalize={bn}\n"
                   for o, a in zip(widths[1:], acts))
    return f"[net]\nbatch={B}\nwidth={widths[0]}\nheight=1\nchannels=1\n" + body + head


_POOL0 = ("[net]\nbatch=2\nwidth=8\nheight=8\nchannels=2\n[{first}]\nsize=2\nstride=2\n"
          "[convolutional]\nbatch_normalize=1\nfilters=3\nsize=3\nstride=1\npad=1\n"
          "activation=leaky\n[{second}]\nsize=2\nstride=2\n[connected]\noutput=4\n"
          "activation=linear\n[softmax]\n")
_MIXED = ("[net]\nbatch=3\ntime_steps=2\ninputs=7\n[lstm]\noutput=5\n"
          "[rnn]\nhidden=4\noutput=6\nactivation=leaky\n"
          "[connected]\noutput=7\nactivation=linear\n[softmax]\n")


def _cases():
    from tensorium_amd import darknet as dn
    cases = {}

    def add(name, cfg, train, truth=None, **kw):
        assert name not in cases, name
        cases[name] = dict(cfg=cfg, train=train, truth=truth, **kw)

    # YOLO
    for name, cfg in (("yolov3-tiny", dn.yolov3_tiny_cfg(64, 1, 2)),
                      ("yolov3", dn.yolov3_cfg(64, 1, 2))):
        add(f"{name}/infer", cfg, False)
        add(f"{name}/train", cfg, True, yolo_deltas=True)
    add("yolov3-tiny/train-loss", dn.yolov3_tiny_cfg(64, 1, 2), True, truth="boxes",
        opts=dict(yolo_loss=True))
    # classifiers
    for name, cfg in (("lenet-cifar10", dn.lenet_cifar10_cfg(2)),
                      ("cifar10-deep", dn.cifar10_deep_cfg(2)),
                      ("lenet-mnist", dn.lenet_mnist_cfg(2))):
        add(f"{name}/train", cfg, True, truth="rows", seeds=True)
        add(f"{name}/infer", cfg, False)
    add("cifar10-deep/train-no-truth", dn.cifar10_deep_cfg(2), True, seeds=True)
    for hname, head in (("cost", "[cost]\n"), ("cost-l2", "[cost]\ntype=L2\nscale=0.5\n"),
                        ("logistic", "[logistic]\n")):
        for bn in (0, 1):
            cfg = _fc_cfg([23, 17, 6], ["relu", "linear"], bn, 5, head)
            add(f"head-{hname}/bn{bn}/train", cfg, True, truth="rows")
            add(f"head-{hname}/bn{bn}/infer", cfg, False)
    drop0 = ("[net]\nbatch=2\ninputs=6\n[dropout]\nprobability=0.3\n[connected]\noutput=4\n"
             "activation=linear\n[softmax]\n")
    add("dropout-first/train", drop0, True, truth="rows", seeds=True)
    add("dropout-first/infer", drop0, False)
    for first, second in (("maxpool", "local_avgpool"), ("local_avgpool", "maxpool")):
        cfg = _POOL0.format(first=first, second=second)
        add(f"{first}-first/train", cfg, True, truth="rows")
        add(f"{first}-first/infer", cfg, False)
    for head in ("softmax", "logistic", "cost"):  # a loss layer with nothing below it
        add(f"{head}-alone/train", f"[net]\nbatch=2\ninputs=5\n[{head}]\n", True, truth="rows")
    # recurrent
    for T in (1, 2, 3):
        for bn in (False, True):
            for fused in (True, False):
                for train in (True, False):
                    mode = "train" if train else "infer"
                    tag = f"T{T}/bn{int(bn)}/{'fused' if fused else 'unfused'}/{mode}"
                    add(f"lstm/{tag}", dn.lstm_cfg(batch=2 * T, time_steps=T, inputs=3, hidden=5,
                                                   layers=2, bn=bn),
                        train, truth="rows" if train else None, opts=dict(lstm_fused=fused))
                    for sc in (False, True):
                        add(f"rnn/{tag}/shortcut{int(sc)}",
                            dn.rnn_cfg(batch=2 * T, time_steps=T, inputs=3, hidden=5, layers=2,
                                       bn=bn),
                            train, truth="rows" if train else None, opts=dict(rnn_fused=fused),
                            shortcut=sc)
    for fused in (True, False):
        tag = "fused" if fused else "unfused"
        add(f"lstm-rnn/{tag}/train", _MIXED, True, truth="rows",
            opts=dict(lstm_fused=fused, rnn_fused=fused))
        add(f"lstm-rnn/{tag}/infer", _MIXED, False, opts=dict(lstm_fused=fused, rnn_fused=fused))
    return cases


CASES = _cases()


@functools.lru_cache(maxsize=2)
def _params(cfg):
    """(the yolov3 cases share their 62M parameters)"""
    from tensorium_amd import darknet as dn
    net = dn.Network(dn.parse_cfg(cfg), rnn=True)
    return dn.random_params(net, seed=11)


def trace(name):
    """Run case ``name``; returns {phase: lines}."""
    import torch
    from tensorium_amd import darknet as dn
    case = CASES[name]
    net = dn.Network(dn.parse_cfg(case["cfg"]), rnn=True)
    for l in net.rnns():
        l.shortcut = case.get("shortcut", False)
    params = _params(case["cfg"])
    base = dn.HipDarknetTrain if case["train"] else dn.HipDarknet
    cls = type(base.__name__, (base,), {"device": "cpu"})
    rec = Recorder()
    model = cls(rec, net, params, torch, **case.get("opts", {}))
    shape = (net.batch, net.c, net.h, net.w) if net.c else (net.batch, net.inputs)
    x = torch.zeros(shape)
    rec.register(x)
    rec.register(vars(model))
    rec.phase("forward")
    if not case["train"]:
        model.forward(x)
        return rec.phases
    yolos = [l for l in net.layers if l.kind == "yolo"]
    truth = None
    if case["truth"] == "boxes":
        truth = torch.zeros(net.batch, yolos[0].max_boxes * 6)
    elif case["truth"] == "rows":
        truth = torch.zeros(net.batch, net.layers[-1].out_size)
    if case.get("yolo_deltas"):
        model.set_yolo_deltas([torch.zeros(net.batch * l.out_size) for l in yolos])
    drops = [l for l in net.layers if l.kind == "dropout"]
    seeds = [1000 + 7 * k for k in range(len(drops))] if case.get("seeds") else None
    model.forward(x, truth, seeds)
    rec.phase("backward")
    model.backward(x)
    rec.phase("update")
    model.update(0.01, 0.9, 0.0005)
    return rec.phases


def text(phases):
    return "".join(f"## {p}\n" + "\n".join(lines) + "\n" for p, lines in phases.items())
