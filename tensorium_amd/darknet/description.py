"""Darknet network description: .cfg parsing, .weights I/O, batch-norm folding
and the layer plan of a forward pass — the part of TDarknetParser / TNNet
(nparser.pas, nnet.pas) that a YOLOv3 forward needs.

* ``parse_cfg(text)``: darknet INI sections (nparser.pas:154-246 reads the
  same format through TCFGList): ``[type]`` lines, ``key=value`` options,
  ``#`` / ``;`` comments.
* ``Network(sections, batch, rnn=False)``: shapes of every layer exactly as the
  reference's parser derives them (nparser.pas:782-930): convolutional
  (``pad=1`` => padding = size div 2, nparser.pas:186-189; out = (in + 2p - k)
  div stride + 1, nConvolutionLayer.pas:92-100), shortcut (TAddLayer,
  naddlayer.pas), route (TConcatLayer, nconcatlayer.pas), upsample
  (TUpSampleLayer, nupsamplelayer.pas), yolo (TYoloLayer, nyololayer.pas) and
  maxpool / local_avgpool (TMaxPoolLayer, nMaxPoolLayer.pas:107-109; options
  as parseMaxPool / parseLocalAvgPool read them, nparser.pas:248-292), avgpool
  (TAvgPoolLayer, navgpoollayer.pas; parseAvgPool, nparser.pas:294-299), and the
  classifier kinds connected / dropout / softmax / cost / logistic
  (parseConnected 146-152, parseDropOut 301-331, parseLogistic 714-720,
  parseSoftmax 722-738, parseCost 740-755), and lstm (TLSTMLayer,
  nlstmlayer.pas; parseLSTM 501-504) and rnn (TRNNLayer, nrnnlayer.pas;
  parseRNN 489-499) with ``[net]``'s ``time_steps`` and ``inputs``
  (nparser.pas:813-818, 962-972).
* ``load_weights`` / ``write_weights``: the darknet .weights layout read by
  TDarknetParser.loadWeights (nparser.pas:1275-1330): int32 major, minor,
  revision, then ``seen`` as uint64 when major*10+minor >= 2 (else uint32),
  then per convolutional layer biases[n], (scales, rolling_mean,
  rolling_variance)[n] when batch-normalized, weights[n*c*k*k]
  (loadConvolutionalWeights, nparser.pas:1140-1185); per connected layer
  biases[O], weights[O*I], then (scales, rolling_mean, rolling_variance)[O]
  when batch-normalized (loadConnectedWeights, nparser.pas:1102-1128); per
  lstm layer eight connected blocks in the order wf wi wg wo uf ui ug uo
  (nparser.pas:1347-1357); per rnn layer three connected blocks in the order
  input, self, output (nparser.pas:1326-1331).
* ``fuse_batchnorm``: TBaseConvolutionalLayer.fuseBatchNorm
  (nConvolutionLayer.pas:102-126) in float32: p = scale / sqrt(max(var,
  1e-6)); bias -= mean * p; W *= p.

The forward pass itself runs on the HIP backend (``drivers.HipDarknet``); the
oracle restates it on the CPU for the parity tests.  This module needs NumPy
only.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

from .._abi import ACT

SEPS = np.float32(0.000001)  # sEPSILON, ntensors.pas:95


@dataclass
class Section:
    kind: str
    opts: dict = field(default_factory=dict)

    def get(self, key, default=None):
        return self.opts.get(key, default)

    def int(self, key, default=0):
        return int(self.opts.get(key, default))


def parse_cfg(text: str) -> list[Section]:
    sections: list[Section] = []
    for raw in text.splitlines():
        line = raw.strip()
        if not line or line[0] in "#;":
            continue
        if line.startswith("["):
            sections.append(Section(line[1:line.index("]")].strip().lower()))
            continue
        if "=" not in line or not sections:
            raise ValueError(f"bad cfg line: {raw!r}")
        k, v = line.split("=", 1)
        sections[-1].opts[k.strip()] = v.strip()
    if not sections or sections[0].kind not in ("net", "network"):
        raise ValueError("1st section in config file must be a [net] parameters.")
    return sections


@dataclass
class Layer:
    index: int
    kind: str            # convolutional | shortcut | route | upsample | yolo |
                         # maxpool | local_avgpool | avgpool | connected |
                         # dropout | softmax | cost | logistic | lstm | rnn
    c: int               # input channels / height / width
    h: int
    w: int
    out_c: int
    out_h: int
    out_w: int
    filters: int = 0
    size: int = 1
    stride: int = 1
    pad: int = 0
    activation: int = ACT["LINEAR"]
    bn: bool = False
    inputs: tuple = ()   # shortcut: (from,), route: the layers, others: ()
    anchors: int = 0     # yolo: anchors of this scale (len(mask))
    classes: int = 0
    stride_x: int = 0    # pools: the two strides (pad holds their padding);
    stride_y: int = 0    # every other layer: both = stride
    probability: float = 0.0   # dropout (a float32 value)
    scale: float = 1.0         # dropout: 1/(1-probability) as float32; cost: scale
    groups: int = 1            # softmax
    temperature: float = 1.0
    noloss: bool = False
    steps: int = 1             # lstm / rnn: time steps; its batch is Network.batch div steps
    gate: str = ""             # a connected block of an lstm layer: wf .. uo; of an rnn
                               # layer: input | self | output
    hidden: int = 0            # rnn: the state's width (filters is its output's)
    self_activation: int = ACT["LINEAR"]  # rnn: the self sub-layer's (logistic=1: LOGISTIC)
    shortcut: bool = False     # rnn: TRNNLayer.isShortcut, a public field no cfg key sets
    # yolo, what its training loss reads (parseYolo, nparser.pas:516-643)
    mask: tuple = ()           # the anchors of this scale, indices into `total`
    total: int = 0             # num=
    biases: tuple = ()         # anchors= as float32 values, 2*total of them (0.5 where absent)
    max_boxes: int = 200       # max=
    ignore_thresh: float = 0.5  # the thresholds and normalizers: float32 values
    truth_thresh: float = 1.0
    iou_thresh: float = 1.0
    iou_normalizer: float = 0.75
    obj_normalizer: float = 1.0
    delta_normalizer: float = 1.0
    unbuilt: tuple = ()        # the keys set that the device loss does not build

    def __post_init__(self):
        self.stride_x = self.stride_x or self.stride
        self.stride_y = self.stride_y or self.stride

    @property
    def out_size(self) -> int:
        return self.out_c * self.out_h * self.out_w

    @property
    def in_size(self) -> int:
        return self.c * self.h * self.w


def _act(name: str) -> int:
    return ACT[name.strip().upper()]


def _flag(sec: Section, key: str) -> bool:
    """TCFGSection.getBool (nconfig.pas:228-237): val() as an integer, <> 0
    (text that is no integer reads as 0)."""
    try:
        return int(str(sec.get(key, "0")).strip()) != 0
    except ValueError:
        return False


def _f32(sec: Section, key: str, default: float) -> float:
    """getFloat into a single field: the value as float32."""
    return float(np.float32(float(str(sec.get(key, default)).strip())))


def _yolo_loss_fields(sec: Section, mask: list) -> dict:
    """The [yolo] keys the training loss reads, with parseYolo's defaults
    (nparser.pas:516-643), and in ``unbuilt`` the keys whose setting the
    device loss does not build (HipDarknetTrain(yolo_loss=True) refuses
    them; inference and set_yolo_deltas training do not read them)."""
    total = sec.int("num", 1)
    vals = [v for v in str(sec.get("anchors", "")).split(",") if v.strip()]
    biases = [np.float32(0.5)] * (2 * total)  # TYoloLayer.Create: biases.fill(0.5)
    for k in range(min(len(vals), 2 * total)):
        biases[k] = np.float32(float(vals[k].strip()))
    unbuilt = []
    if str(sec.get("iou_loss", "mse")).strip() != "mse":
        unbuilt.append("iou_loss")
    if str(sec.get("iou_thresh_kind", "iou")).strip() != "iou":
        unbuilt.append("iou_thresh_kind")
    unbuilt += [k for k in ("focal_loss", "objectness_smooth", "new_coords") if _flag(sec, k)]
    if _f32(sec, "label_smooth_eps", 0.0) != 0.0:
        unbuilt.append("label_smooth_eps")
    if _f32(sec, "scale_x_y", 1.0) != 1.0:
        unbuilt.append("scale_x_y")
    unbuilt += [k for k in ("counters_per_class", "map") if str(sec.get(k, "")).strip()]
    if sec.int("embedding_layer", 999999) != 999999:
        unbuilt.append("embedding_layer")
    return dict(mask=tuple(int(m) for m in mask), total=total,
                biases=tuple(float(v) for v in biases), max_boxes=sec.int("max", 200),
                ignore_thresh=_f32(sec, "ignore_thresh", 0.5),
                truth_thresh=_f32(sec, "truth_thresh", 1.0),
                iou_thresh=_f32(sec, "iou_thresh", 1.0),
                iou_normalizer=_f32(sec, "iou_normalizer", 0.75),
                obj_normalizer=_f32(sec, "obj_normalizer", 1.0),
                delta_normalizer=_f32(sec, "delta_normalizer", 1.0), unbuilt=tuple(unbuilt))


# [net] keys that switch on what the device yolo loss does not build: the
# adversarial branch and the bad-label rejection block (nyololayer.pas:589-613,
# 896-990; nparser.pas:975-977)
_NET_YOLO_UNBUILT = ("adversarial", "adversarial_lr", "equidistant_point",
                     "badlabels_rejection_percentage", "num_sigmas_reject_badlabels")


# kinds that read params.c / h / w, which the reference leaves stale after a
# layer that is no TBaseImageLayer (nparser.pas:913-919)
LSTM_GATES = ("wf", "wi", "wg", "wo", "uf", "ui", "ug", "uo")  # file / update order
RNN_SUBS = ("input", "self", "output")  # file / update order
# the activations the backend implements (act_supported, elementwise.hip)
ACT_SUPPORTED = tuple(ACT[k] for k in ("LOGISTIC", "RELU", "LINEAR", "TANH", "REVLEAKY", "LEAKY",
                                       "HARDTAN"))

_IMAGE_KINDS = ("convolutional", "conv", "shortcut", "route", "concat", "upsample", "yolo",
                "maxpool", "max", "local_avgpool", "avgpool", "avg")


class Network:
    """Layer plan with shapes (nparser.pas:782-930).

    ``rnn=True`` plans ``[rnn]`` sections.  Without it they are refused as
    before the layer was built, with the other recurrent kinds: callers (and
    tests/test_lstm.py) that rely on a plan holding only what they know keep
    that, and a caller that drives rnn layers says so."""

    def __init__(self, sections: list[Section], batch: int | None = None, rnn: bool = False):
        net = sections[0]
        # Neural.batch := mini_batch * timeSteps (nparser.pas:962-972); a
        # batch argument replaces the whole product (ABatch, 802-803)
        self.time_steps = net.int("time_steps", 1)
        if self.time_steps < 1:
            raise ValueError(f"[net] time_steps={self.time_steps}")
        self.batch = batch if batch is not None else net.int("batch", 1) * self.time_steps
        self.h, self.w, self.c = net.int("height"), net.int("width"), net.int("channels", 3)
        # the [net] keys set that the device yolo loss does not build
        self.yolo_unbuilt = tuple(k for k in _NET_YOLO_UNBUILT if _f32(net, k, 0.0) != 0.0)
        self.layers: list[Layer] = []
        c, h, w = self.c, self.h, self.w
        flat = False  # a [connected] has been planned: c, h, w are the parser's no longer
        self.inputs = c * h * w
        if self.inputs == 0:  # no image shape: rows of inputs= floats (nparser.pas:813-818)
            self.inputs = net.int("inputs", 0)
            if self.inputs < 1:
                raise ValueError("[net] has neither an image shape nor inputs=")
            self.h = self.w = self.c = 0
            c, h, w, flat = self.inputs, 1, 1, True
        for sec in sections[1:]:
            i = len(self.layers)
            if flat and sec.kind in _IMAGE_KINDS:
                raise ValueError(f"[{sec.kind}] layer {i} after a [connected], [lstm] or [rnn] "
                                 "layer, or in a network of inputs= rows: the reference plans it "
                                 "on the image shape of an earlier layer (nparser.pas:913-919); "
                                 "refused")
            if sec.kind in ("convolutional", "conv"):
                size = sec.int("size", 1)
                stride = sec.int("stride", 1)
                pad = size // 2 if sec.int("pad", 0) else sec.int("padding", 0)
                f = sec.int("filters", 1)
                oh = (h + 2 * pad - size) // stride + 1
                ow = (w + 2 * pad - size) // stride + 1
                lay = Layer(i, "convolutional", c, h, w, f, oh, ow, filters=f, size=size,
                            stride=stride, pad=pad, activation=_act(sec.get("activation", "logistic")),
                            bn=bool(sec.int("batch_normalize", 0)))
            elif sec.kind == "shortcut":
                src = int(sec.get("from"))
                src = src + i if src < 0 else src
                lay = Layer(i, "shortcut", c, h, w, c, h, w,
                            activation=_act(sec.get("activation", "linear")), inputs=(src,))
            elif sec.kind in ("route", "concat"):
                srcs = tuple(int(v) + i if int(v) < 0 else int(v)
                             for v in sec.get("layers").split(","))
                first = self.layers[srcs[0]]
                oc = sum(self.layers[s].out_c for s in srcs)
                lay = Layer(i, "route", c, h, w, oc, first.out_h, first.out_w, inputs=srcs)
            elif sec.kind == "upsample":
                s = sec.int("stride", 2)
                lay = Layer(i, "upsample", c, h, w, c, h * s, w * s, stride=s)
            elif sec.kind == "yolo":
                mask = [m for m in sec.get("mask", "").split(",") if m.strip()]
                classes = sec.int("classes", 20)
                lay = Layer(i, "yolo", c, h, w, c, h, w, anchors=len(mask), classes=classes,
                            **_yolo_loss_fields(sec, mask))
                if c != len(mask) * (classes + 5):
                    raise ValueError(f"yolo layer {i}: {c} channels for {len(mask)} anchors")
            elif sec.kind in ("maxpool", "max", "local_avgpool"):
                # parseMaxPool / parseLocalAvgPool (nparser.pas:248-292), shapes
                # TMaxPoolLayer.Create (nMaxPoolLayer.pas:79-82, 107-109)
                kind = "local_avgpool" if sec.kind == "local_avgpool" else "maxpool"
                stride = sec.int("stride", 1)
                sx, sy = sec.int("stride_x", stride), sec.int("stride_y", stride)
                size = sec.int("size", stride)
                padding = sec.int("padding", size - 1)
                if kind == "maxpool" and (sec.int("maxpool_depth", 0)
                                          or sec.int("antialiasing", 0)):
                    raise ValueError(f"[{sec.kind}] layer {i}: maxpool_depth / antialiasing are "
                                     "not built (the reference's device path has neither)")
                if h * w * c == 0:
                    raise ValueError(f"Layer before [{sec.kind}] layer must output image.")
                sx, sy = sx or size, sy or size
                if size < 1 or padding < 0 or h + padding < size or w + padding < size:
                    raise ValueError(f"[{sec.kind}] layer {i}: size {size}, padding {padding} on "
                                     f"{h}x{w}")
                lay = Layer(i, kind, c, h, w, c, (h + padding - size) // sy + 1,
                            (w + padding - size) // sx + 1, size=size, stride=sx, pad=padding,
                            stride_x=sx, stride_y=sy)
            elif sec.kind in ("avgpool", "avg"):
                # parseAvgPool (nparser.pas:294-299): the whole plane, no
                # options; a TBaseImageLayer, so the parser carries on with
                # c x 1 x 1 (navgpoollayer.pas:27-43)
                if h * w * c == 0:
                    raise ValueError("Layer before avgpool layer must output image.")
                lay = Layer(i, "avgpool", c, h, w, c, 1, 1)
            elif sec.kind in ("connected", "conn"):
                o = sec.int("output", 1)
                if o < 1 or c * h * w < 1:
                    raise ValueError(f"[connected] layer {i}: {c * h * w} inputs, output={o}")
                lay = Layer(i, "connected", c, h, w, o, 1, 1, filters=o,
                            activation=_act(sec.get("activation", "relu")),
                            bn=_flag(sec, "batch_normalize"))
                flat = True
            elif sec.kind == "lstm":
                # parseLSTM (nparser.pas:501-504); the layer's own batch is
                # Network.batch div time_steps (nlstmlayer.pas:44) — the
                # reference truncates, here the remainder is refused
                o = sec.int("output", 1)
                if o < 1 or c * h * w < 1:
                    raise ValueError(f"[lstm] layer {i}: {c * h * w} inputs, output={o}")
                if self.batch % self.time_steps:
                    raise ValueError(f"[lstm] layer {i}: batch {self.batch} is no multiple of "
                                     f"time_steps {self.time_steps}")
                lay = Layer(i, "lstm", c, h, w, o, 1, 1, filters=o, bn=_flag(sec, "batch_normalize"),
                            steps=self.time_steps)
                flat = True
            elif sec.kind == "rnn" and rnn:
                # parseRNN (nparser.pas:489-499); the layer's own batch is
                # Network.batch div time_steps (nrnnlayer.pas:49), a remainder
                # refused as for [lstm].  The self sub-layer's activation is
                # the layer's, LOGISTIC with logistic=1, LOGGY with logistic=2
                # (nrnnlayer.pas:66)
                o, hid = sec.int("output", 1), sec.int("hidden", 1)
                if o < 1 or hid < 1 or c * h * w < 1:
                    raise ValueError(f"[rnn] layer {i}: {c * h * w} inputs, hidden={hid}, "
                                     f"output={o}")
                if self.batch % self.time_steps:
                    raise ValueError(f"[rnn] layer {i}: batch {self.batch} is no multiple of "
                                     f"time_steps {self.time_steps}")
                name = sec.get("activation", "logistic").strip().upper()
                log = sec.int("logistic", 0)
                if log == 2:
                    raise ValueError(f"[rnn] layer {i}: logistic=2 selects the LOGGY activation "
                                     "for the self sub-layer, which is not built")
                if ACT.get(name) not in ACT_SUPPORTED:
                    raise ValueError(f"[rnn] layer {i}: activation={name.lower()} is not built")
                lay = Layer(i, "rnn", c, h, w, o, 1, 1, filters=o, activation=ACT[name],
                            bn=_flag(sec, "batch_normalize"), steps=self.time_steps, hidden=hid,
                            self_activation=ACT["LOGISTIC"] if log == 1 else ACT[name])
                flat = True
            elif sec.kind == "dropout":
                # probability is a single; scale := 1 / (1.0 - probability) in
                # double, stored as single (ndropoutlayer.pas:65)
                p = np.float32(sec.get("probability", 0.2))
                if not p < 1:  # the constructor's assert
                    raise ValueError(f"[dropout] layer {i}: probability {p} must be below one")
                if _flag(sec, "dropblock"):
                    raise ValueError(f"[dropout] layer {i}: dropblock is not built (the "
                                     "reference's device path has none)")
                lay = Layer(i, "dropout", c, h, w, c, h, w, probability=float(p),
                            scale=float(np.float32(1.0 / (1.0 - float(p)))))
            elif sec.kind in ("softmax", "soft"):
                if sec.get("tree", ""):
                    raise ValueError(f"[softmax] layer {i}: tree= is not built")
                g = sec.int("groups", 1)
                if g < 1 or (c * h * w) % g:
                    raise ValueError(f"[softmax] layer {i}: {c * h * w} inputs in {g} groups")
                lay = Layer(i, "softmax", c, h, w, c, h, w, groups=g,
                            temperature=float(np.float32(sec.get("temperature", 1))),
                            noloss=_flag(sec, "noloss"))
            elif sec.kind == "cost":
                # the reference's device path runs costL2 whatever the type
                # says (ncostlayer.pas:218-228): only the L2 types are taken
                ty = str(sec.get("type", "sse")).strip().lower()
                if ty not in ("sse", "l2"):
                    raise ValueError(f"[cost] layer {i}: type={ty} is not built (sse / L2 only)")
                lay = Layer(i, "cost", c, h, w, c, h, w,
                            scale=float(np.float32(sec.get("scale", 1))))
            elif sec.kind == "logistic":
                lay = Layer(i, "logistic", c, h, w, c, h, w, activation=ACT["LOGISTIC"])
            elif sec.kind == "rnn":
                raise ValueError("[Parser][rnn] layer is not yet implemented! (in the default "
                                 "plan: Network(sections, batch, rnn=True) plans it)")
            else:
                raise ValueError(f"[Parser][{sec.kind}] layer is not yet implemented!")
            self.layers.append(lay)
            c, h, w = lay.out_c, lay.out_h, lay.out_w

    def convs(self) -> list[Layer]:
        return [l for l in self.layers if l.kind == "convolutional"]

    def param_layers(self) -> list[Layer]:
        """The parameter blocks in file order (loadWeights' order,
        nparser.pas:1309-1357): the convolutional and connected layers, and
        for an lstm layer its eight connected sub-layers wf wi wg wo ([O][O])
        uf ui ug uo ([O][inputs]) as connected blocks carrying the layer's
        index and their name in ``gate``; for an rnn layer its three connected
        sub-layers input ([hidden][inputs]), self ([hidden][hidden]) and
        output ([O][hidden]) the same way, each with its own activation."""
        out = []
        for l in self.layers:
            if l.kind in ("convolutional", "connected"):
                out.append(l)
            elif l.kind == "lstm":
                for g in LSTM_GATES:
                    n = l.filters if g[0] == "w" else l.in_size
                    out.append(Layer(l.index, "connected", n, 1, 1, l.filters, 1, 1,
                                     filters=l.filters, bn=l.bn, gate=g))
            elif l.kind == "rnn":
                for g, n, o, act in (("input", l.in_size, l.hidden, l.activation),
                                     ("self", l.hidden, l.hidden, l.self_activation),
                                     ("output", l.hidden, l.filters, l.activation)):
                    out.append(Layer(l.index, "connected", n, 1, 1, o, 1, 1, filters=o,
                                     activation=act, bn=l.bn, gate=g))
        return out

    def lstms(self) -> list[Layer]:
        return [l for l in self.layers if l.kind == "lstm"]

    def rnns(self) -> list[Layer]:
        return [l for l in self.layers if l.kind == "rnn"]

    def yolos(self) -> list[Layer]:
        return [l for l in self.layers if l.kind == "yolo"]


def _bn_conv(f, k, s=1, act="leaky", bn=True):
    return (f"[convolutional]\n{'batch_normalize=1' + chr(10) if bn else ''}"
            f"filters={f}\nsize={k}\nstride={s}\npad=1\nactivation={act}\n")


def _darknet53_backbone() -> list[str]:
    """Layers 0..74 of YOLOv3, the darknet53 feature extractor: 52
    convolutions and 23 shortcuts."""
    out = [_bn_conv(32, 3)]
    for n, c in ((1, 64), (2, 128), (8, 256), (8, 512), (4, 1024)):
        out.append(_bn_conv(c, 3, 2))
        for _ in range(n):
            out += [_bn_conv(c // 2, 1), _bn_conv(c, 3),
                    "[shortcut]\nfrom=-3\nactivation=linear\n"]
    return out


def yolov3_cfg(size: int = 416, batch: int = 1, classes: int = 80) -> str:
    """The darknet YOLOv3 network (the public yolov3.cfg structure; the
    reference loads that file from outside its tree, MSCOCOYolo.pas:28-34)."""
    out = [f"[net]\nbatch={batch}\nsubdivisions=1\nwidth={size}\nheight={size}\nchannels=3\n"]

    def conv(f, k, s=1, act="leaky", bn=True):
        out.append(_bn_conv(f, k, s, act, bn))

    anchors = "10,13, 16,30, 33,23, 30,61, 62,45, 59,119, 116,90, 156,198, 373,326"

    def yolo(mask):
        out.append(f"[yolo]\nmask = {mask}\nanchors = {anchors}\nclasses={classes}\nnum=9\n"
                   "jitter=.3\nignore_thresh = .7\ntruth_thresh = 1\nrandom=1\n")

    det = 3 * (classes + 5)
    out += _darknet53_backbone()
    for _ in range(2):
        conv(512, 1); conv(1024, 3)
    conv(512, 1); conv(1024, 3); conv(det, 1, act="linear", bn=False)
    yolo("6,7,8")
    out.append("[route]\nlayers = -4\n")
    conv(256, 1)
    out.append("[upsample]\nstride=2\n")
    out.append("[route]\nlayers = -1, 61\n")
    for _ in range(2):
        conv(256, 1); conv(512, 3)
    conv(256, 1); conv(512, 3); conv(det, 1, act="linear", bn=False)
    yolo("3,4,5")
    out.append("[route]\nlayers = -4\n")
    conv(128, 1)
    out.append("[upsample]\nstride=2\n")
    out.append("[route]\nlayers = -1, 36\n")
    for _ in range(3):
        conv(128, 1); conv(256, 3)
    conv(det, 1, act="linear", bn=False)
    yolo("0,1,2")
    return "\n".join(out)


def yolov3_tiny_cfg(size: int = 416, batch: int = 1, classes: int = 80) -> str:
    """The darknet YOLOv3-tiny network (the public yolov3-tiny.cfg structure):
    six conv + maxpool stages, the last pool 2x2 with stride 1, and two
    detection scales."""
    out = [f"[net]\nbatch={batch}\nsubdivisions=1\nwidth={size}\nheight={size}\nchannels=3\n"]

    def conv(f, k, act="leaky", bn=True):
        out.append(f"[convolutional]\n{'batch_normalize=1' + chr(10) if bn else ''}"
                   f"filters={f}\nsize={k}\nstride=1\npad=1\nactivation={act}\n")

    def maxpool(stride):
        out.append(f"[maxpool]\nsize=2\nstride={stride}\n")

    anchors = "10,14, 23,27, 37,58, 81,82, 135,169, 344,319"

    def yolo(mask):
        out.append(f"[yolo]\nmask = {mask}\nanchors = {anchors}\nclasses={classes}\nnum=6\n"
                   "jitter=.3\nignore_thresh = .7\ntruth_thresh = 1\nrandom=1\n")

    det = 3 * (classes + 5)
    for f in (16, 32, 64, 128, 256):
        conv(f, 3); maxpool(2)
    conv(512, 3); maxpool(1)
    conv(1024, 3)
    conv(256, 1); conv(512, 3); conv(det, 1, act="linear", bn=False)
    yolo("3,4,5")
    out.append("[route]\nlayers = -4\n")
    conv(128, 1)
    out.append("[upsample]\nstride=2\n")
    out.append("[route]\nlayers = -1, 8\n")
    conv(256, 3); conv(det, 1, act="linear", bn=False)
    yolo("0,1,2")
    return "\n".join(out)


def darknet19_cfg(size: int = 256, batch: int = 1, classes: int = 1000) -> str:
    """The darknet19 ImageNet classifier (the public darknet19.cfg structure;
    the file is not in the reference's tree, so this is the common structure,
    not a file that can be compared against): 3x3 batch-normalised leaky
    convolutions of 32 and 64 filters, each followed by a 2x2/2 max pool; the
    groups 128-64-128, 256-128-256, 512-256-512-256-512 (each followed by a
    pool) and 1024-512-1024-512-1024, their middle convolutions 1x1; a 1x1
    linear convolution to ``classes`` without batch norm; [avgpool]; [softmax].
    26 layers, 19 of them convolutional."""
    out = [f"[net]\nbatch={batch}\nsubdivisions=1\nwidth={size}\nheight={size}\nchannels=3\n"]
    pool = "[maxpool]\nsize=2\nstride=2\n"
    out += [_bn_conv(32, 3), pool, _bn_conv(64, 3), pool]
    for c, n in ((128, 3), (256, 3), (512, 5), (1024, 5)):
        out += [_bn_conv(c if k % 2 == 0 else c // 2, 3 if k % 2 == 0 else 1) for k in range(n)]
        if c != 1024:
            out.append(pool)
    out += [_bn_conv(classes, 1, act="linear", bn=False), "[avgpool]\n", "[softmax]\ngroups=1\n"]
    return "\n".join(out)


def darknet53_cfg(size: int = 256, batch: int = 1, classes: int = 1000) -> str:
    """The darknet53 ImageNet classifier (the public darknet53.cfg structure;
    the file is not in the reference's tree, so this is the common structure,
    not a file that can be compared against): YOLOv3's layers 0..74, then
    [avgpool], a linear [connected] to ``classes`` and [softmax].  78 layers."""
    out = [f"[net]\nbatch={batch}\nsubdivisions=1\nwidth={size}\nheight={size}\nchannels=3\n"]
    out += _darknet53_backbone()
    out += ["[avgpool]\n", f"[connected]\noutput={classes}\nactivation=linear\n",
            "[softmax]\ngroups=1\n"]
    return "\n".join(out)


def _classifier_cfg(batch: int, size: int, channels: int, body: list[str]) -> str:
    head = (f"[net]\nbatch={batch}\nsubdivisions=1\nwidth={size}\nheight={size}\n"
            f"channels={channels}\n")
    return "\n".join([head, *body])


def _cconv(f, k, padding, bn):
    return (f"[convolutional]\n{'batch_normalize=1' + chr(10) if bn else ''}filters={f}\n"
            f"size={k}\nstride=1\npadding={padding}\nactivation=relu\n")


_CPOOL = "[maxpool]\nsize=2\nstride=2\npadding=0\n"


def _cfc(o, act):
    return f"[connected]\noutput={o}\nactivation={act}\n"


def cifar10_deep_cfg(batch: int = 1) -> str:
    """deepCIFAR10 (nmodels.pas:82-108): three stages of two batch-normalised
    3x3 convolutions and a 2x2 max pool, then dropout 0.2, connected 1024
    (relu), dropout 0.2, connected 10 (linear), softmax."""
    body = []
    for f in (32, 64, 128):
        body += [_cconv(f, 3, 1, True), _cconv(f, 3, 1, True), _CPOOL]
    body += ["[dropout]\nprobability=0.2\n", _cfc(1024, "relu"), "[dropout]\nprobability=0.2\n",
             _cfc(10, "linear"), "[softmax]\n"]
    return _classifier_cfg(batch, 32, 3, body)


def lenet_cifar10_cfg(batch: int = 1) -> str:
    """leNetCIFAR10 (nmodels.pas:66-80): batch-normalised 5x5 convolutions
    (6, 12, 120 filters, no padding) with two 2x2 max pools, connected 84
    (relu), connected 10 (linear), softmax."""
    body = [_cconv(6, 5, 0, True), _CPOOL, _cconv(12, 5, 0, True), _CPOOL, _cconv(120, 5, 0, True),
            _cfc(84, "relu"), _cfc(10, "linear"), "[softmax]\n"]
    return _classifier_cfg(batch, 32, 3, body)


def lenet_mnist_cfg(batch: int = 1) -> str:
    """leNetMNIST (nmodels.pas:50-64): 5x5 convolutions without batch norm
    (6 filters at padding 2, then 16 and 120 at padding 0) with two 2x2 max
    pools, connected 84 (relu), connected 10 (linear), softmax."""
    body = [_cconv(6, 5, 2, False), _CPOOL, _cconv(16, 5, 0, False), _CPOOL,
            _cconv(120, 5, 0, False), _cfc(84, "relu"), _cfc(10, "linear"), "[softmax]\n"]
    return _classifier_cfg(batch, 28, 1, body)


def lstm_cfg(batch: int = 1, time_steps: int = 1, inputs: int = 256, hidden: int = 1024,
             layers: int = 3, bn: bool = True, cost: bool = False) -> str:
    """The public char-LSTM structure: ``layers`` stacked [lstm] of ``hidden``
    outputs over rows of ``inputs`` floats, a linear [connected] back to
    ``inputs``, [softmax], optionally [cost].  The reference's sample loads
    its cfg from outside its tree (lstm_shakespeare_train.pas:25, 207), so
    this is the common structure, not a file that can be compared against."""
    out = [f"[net]\nbatch={batch}\nsubdivisions=1\ninputs={inputs}\ntime_steps={time_steps}\n"]
    for _ in range(layers):
        out.append(f"[lstm]\n{'batch_normalize=1' + chr(10) if bn else ''}output={hidden}\n")
    out += [f"[connected]\noutput={inputs}\nactivation=linear\n", "[softmax]\n"]
    if cost:
        out.append("[cost]\ntype=sse\n")
    return "\n".join(out)


def rnn_cfg(batch: int = 1, time_steps: int = 1, inputs: int = 256, hidden: int = 1024,
            layers: int = 3, bn: bool = True, activation: str = "leaky", cost: bool = True) -> str:
    """The public char-RNN structure: ``layers`` stacked [rnn] of ``hidden``
    state and outputs over rows of ``inputs`` floats, a linear [connected]
    back to ``inputs``, [softmax], optionally [cost] type=sse.  The
    reference's sample loads its cfg from outside its tree
    (shakespeare_infer_rnn.pas), so this is the common structure, not a file
    that can be compared against.  Plan it with ``Network(parse_cfg(...),
    rnn=True)``."""
    out = [f"[net]\nbatch={batch}\nsubdivisions=1\ninputs={inputs}\ntime_steps={time_steps}\n"]
    for _ in range(layers):
        out.append(f"[rnn]\n{'batch_normalize=1' + chr(10) if bn else ''}output={hidden}\n"
                   f"hidden={hidden}\nactivation={activation}\n")
    out += [f"[connected]\noutput={inputs}\nactivation=linear\n", "[softmax]\n"]
    if cost:
        out.append("[cost]\ntype=sse\n")
    return "\n".join(out)


# ---- parameters -------------------------------------------------------------

@dataclass
class ConvParams:
    biases: np.ndarray
    weights: np.ndarray                 # [filters][c*k*k]
    scales: np.ndarray | None = None    # batch norm (before folding)
    rolling_mean: np.ndarray | None = None
    rolling_var: np.ndarray | None = None


def random_params(net: Network, seed: int = 3) -> list[ConvParams]:
    """Synthetic parameters, one entry per convolutional or connected layer in
    file order.  Convolutions: the reference's initialisation scale
    (nConvolutionLayer.pas:216-220: U[-s, s], s = sqrt(2/(k*k*c))).  Connected
    layers: TConnectedLayer.Create (nconnectedlayer.pas:78-99): weights
    [outputs][inputs] U[-s, s] with s = single(sqrt(2/inputs)), biases 0,
    scales 1 and rolling statistics 0 when batch-normalised."""
    rng = np.random.default_rng(seed)
    ps = []
    for l in net.param_layers():
        if l.kind == "connected":
            s = float(np.float32(np.sqrt(2.0 / l.in_size)))
            w = rng.uniform(-s, s, (l.filters, l.in_size)).astype(np.float32)
            z = lambda: np.zeros(l.filters, np.float32)  # noqa: E731
            ps.append(ConvParams(z(), w, np.ones(l.filters, np.float32), z(), z()) if l.bn
                      else ConvParams(z(), w))
            continue
        s = np.sqrt(2.0 / (l.size * l.size * l.c))
        w = rng.uniform(-s, s, (l.filters, l.c * l.size * l.size)).astype(np.float32)
        b = rng.uniform(-0.1, 0.1, l.filters).astype(np.float32)
        if l.bn:
            ps.append(ConvParams(b, w, rng.uniform(0.5, 1.5, l.filters).astype(np.float32),
                                 rng.uniform(-0.1, 0.1, l.filters).astype(np.float32),
                                 rng.uniform(0.5, 2.0, l.filters).astype(np.float32)))
        else:
            ps.append(ConvParams(b, w))
    return ps


def _no_transpose(major, minor):
    if major > 1000 or minor > 1000:  # loadWeights' transpose flag (nparser.pas:1307)
        raise ValueError("weights file with the transpose flag (major or minor > 1000) is "
                         "not supported")


def write_weights(path, net: Network, params: list[ConvParams], major=0, minor=2, revision=0,
                  seen=0) -> None:
    _no_transpose(major, minor)
    with open(path, "wb") as f:
        f.write(struct.pack("<3i", major, minor, revision))
        f.write(struct.pack("<Q" if major * 10 + minor >= 2 else "<I", seen))
        for l, p in zip(net.param_layers(), params):
            f.write(p.biases.astype("<f4").tobytes())
            if l.kind == "connected":  # weights before the batch-norm arrays
                f.write(p.weights.astype("<f4").tobytes())
            if l.bn:
                for t in (p.scales, p.rolling_mean, p.rolling_var):
                    f.write(t.astype("<f4").tobytes())
            if l.kind == "convolutional":
                f.write(p.weights.astype("<f4").tobytes())


def load_weights(path, net: Network) -> tuple[list[ConvParams], int]:
    """Returns the per-layer parameters (convolutional and connected layers
    in file order) and ``seen``."""
    data = Path(path).read_bytes()
    major, minor, _rev = struct.unpack_from("<3i", data, 0)
    _no_transpose(major, minor)
    off = 12
    if major * 10 + minor >= 2:
        (seen,) = struct.unpack_from("<Q", data, off)
        off += 8
    else:
        (seen,) = struct.unpack_from("<I", data, off)
        off += 4

    def take(n):
        nonlocal off
        if off + 4 * n > len(data):
            raise ValueError("Unexpected end of weights-file")
        a = np.frombuffer(data, "<f4", n, off).astype(np.float32)
        off += 4 * n
        return a

    ps = []
    for l in net.param_layers():
        b = take(l.filters)
        sc = rm = rv = None
        if l.kind == "connected":
            w = take(l.filters * l.in_size).reshape(l.filters, -1)
            if l.bn:
                sc, rm, rv = take(l.filters), take(l.filters), take(l.filters)
        else:
            if l.bn:
                sc, rm, rv = take(l.filters), take(l.filters), take(l.filters)
            w = take(l.filters * l.c * l.size * l.size).reshape(l.filters, -1)
        ps.append(ConvParams(b, w, sc, rm, rv))
    return ps, seen


def fuse_batchnorm(l: Layer, p: ConvParams) -> ConvParams:
    """fuseBatchNorm (nConvolutionLayer.pas:102-126), float32 throughout."""
    if not l.bn:
        return ConvParams(p.biases.copy(), p.weights.copy())
    pre = (p.scales / np.sqrt(np.maximum(p.rolling_var, SEPS))).astype(np.float32)
    b = (p.biases - (p.rolling_mean * pre).astype(np.float32)).astype(np.float32)
    w = (p.weights * pre[:, None]).astype(np.float32)
    return ConvParams(b, w)

