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
  as parseMaxPool / parseLocalAvgPool read them, nparser.pas:248-292), and the
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

The forward pass itself runs on the HIP backend (``HipDarknet``); the oracle
restates it on the CPU for the parity tests.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

from ._abi import ACT, TnsError

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
                         # maxpool | local_avgpool | connected | dropout |
                         # softmax | cost | logistic | lstm | rnn
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
                "maxpool", "max", "local_avgpool")


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


def yolov3_cfg(size: int = 416, batch: int = 1, classes: int = 80) -> str:
    """The darknet YOLOv3 network (the public yolov3.cfg structure; the
    reference loads that file from outside its tree, MSCOCOYolo.pas:28-34)."""
    out = [f"[net]\nbatch={batch}\nsubdivisions=1\nwidth={size}\nheight={size}\nchannels=3\n"]

    def conv(f, k, s=1, act="leaky", bn=True):
        out.append(f"[convolutional]\n{'batch_normalize=1' + chr(10) if bn else ''}"
                   f"filters={f}\nsize={k}\nstride={s}\npad=1\nactivation={act}\n")

    def res(n, c):
        for _ in range(n):
            conv(c // 2, 1)
            conv(c, 3)
            out.append("[shortcut]\nfrom=-3\nactivation=linear\n")

    anchors = "10,13, 16,30, 33,23, 30,61, 62,45, 59,119, 116,90, 156,198, 373,326"

    def yolo(mask):
        out.append(f"[yolo]\nmask = {mask}\nanchors = {anchors}\nclasses={classes}\nnum=9\n"
                   "jitter=.3\nignore_thresh = .7\ntruth_thresh = 1\nrandom=1\n")

    det = 3 * (classes + 5)
    conv(32, 3)
    conv(64, 3, 2); res(1, 64)
    conv(128, 3, 2); res(2, 128)
    conv(256, 3, 2); res(8, 256)
    conv(512, 3, 2); res(8, 512)
    conv(1024, 3, 2); res(4, 1024)
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


class _LstmLayers:
    """The lstm layers of a driver (TLSTMLayer.forwardGPU / backwardGPU /
    updateGPU, nlstmlayer.pas:876-1294), shared by HipDarknet and
    HipDarknetTrain.  Rows are [step][stream]; n = streams * outputs floats
    make one step's slice.

    State per layer, as the reference keeps it: ``c``, ``h``, ``dc``,
    ``prevCell``, ``prevState`` (n floats each; never cleared by a pass),
    ``cell`` and the layer's output (steps * n), and per sub-layer what
    ``_fc_forward`` / ``_fc_backward`` keep for a connected layer, its output
    and delta steps * n long.  The four w* (and the four u*) sub-layers'
    weights, weight_updates, outputs and deltas are slices of one buffer
    each, in the order f, i, g, o, so a strided-batched GEMM can cover them.

    ``lstm_fused=False`` is the reference's call sequence, call for call
    through the existing TNNHip methods.  ``lstm_fused=True`` is the product
    path: one ``lstmGatesForward`` / ``lstmGatesBackward`` per step, and
    GEMMs batched only where every output element keeps its operands and its
    order of additions (the LSTM section)."""

    W, U = LSTM_GATES[:4], LSTM_GATES[4:]

    def _lstm_init(self, blocks, training):
        torch, dev = self.torch, "cuda"
        z = lambda n: torch.zeros(n, device=dev)  # noqa: E731
        self.lstm = {}
        by_layer = {}
        for l, p in blocks:
            by_layer.setdefault(l.index, {})[l.gate] = p
        for l in self.net.lstms():
            T = l.steps
            S = self.net.batch // T
            O, I = l.filters, l.in_size
            n = S * O
            ps = by_layer[l.index]
            L = {"S": S, "T": T, "n": n, "sub": {}, "cell": z(T * n)}
            for k in ("c", "h", "dc", "prevCell", "prevState"):
                L[k] = z(n)
            if not self.lstm_fused:
                for k in ("f", "i", "g", "o", "temp", "temp2", "temp3"):
                    L["_" + k] = z(n)
            for side, names, K in (("w", self.W, O), ("u", self.U, I)):
                L[side + "_w"] = z(4 * O * K)
                L[side + "_out"] = z(4 * T * n)
                if training:
                    L[side + "_wu"] = z(4 * O * K)
                    L[side + "_delta"] = z(4 * T * n)
                for q, g in enumerate(names):
                    p = ps[g]
                    st = {"I": K, "w": L[side + "_w"][q * O * K:(q + 1) * O * K],
                          "b": self._t(p.biases), "out": L[side + "_out"][q * T * n:(q + 1) * T * n]}
                    st["w"].copy_(self._t(p.weights).reshape(-1))
                    if l.bn:
                        st.update(scales=self._t(p.scales), rm=self._t(p.rolling_mean),
                                  rv=self._t(p.rolling_var))
                    if training:
                        st.update(wu=L[side + "_wu"][q * O * K:(q + 1) * O * K], bu=z(O),
                                  delta=L[side + "_delta"][q * T * n:(q + 1) * T * n])
                        if l.bn:
                            st.update(mean=z(O), var=z(O), x=z(T * n), xn=z(T * n), su=z(O),
                                      md=z(O), vd=z(O))
                    L["sub"][g] = st
            self.lstm[l.index] = L

    def _t(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda")

    def reset_state(self):
        """Zero c, h, dc, prevCell and prevState of every lstm layer (no pass
        does: the reference carries them from call to call)."""
        for L in self.lstm.values():
            for k in ("c", "h", "dc", "prevCell", "prevState"):
                L[k].zero_()

    # -- one sub-layer, one step: TConnectedLayer.forwardGPU / backwardGPU ----
    @staticmethod
    def _sub_dims(l, L, st):
        """A sub-layer's outputs and one step's slice of them: the layer's for
        an lstm gate; an rnn sub-layer carries its own (``O``, and ``act``)."""
        O = st.get("O", l.filters)
        return O, L["S"] * O

    def _sub_bn_forward(self, l, L, st, step, training, activate=True):
        """What follows the product (nconnectedlayer.pas:654-733) on step's
        slice; one mean / variance pair per sub-layer, overwritten each step.
        activate=False: without the bias add (no batch norm) and the
        activation, which rnnStateForward makes."""
        hip, S = self.hip, L["S"]
        O, n = self._sub_dims(l, L, st)
        out, off = st["out"], step * n
        if not l.bn:
            if activate:
                hip.forwardBias(n, out, off, O, st["b"], 1, S)
        else:
            if training:
                mom = np.float32(0.05)  # bnMomentum (nconnectedlayer.pas:67)
                keep = float(np.float32(1) - mom)
                hip.means(n, O, S, out, off, st["mean"])
                hip.variances(n, O, S, out, off, st["mean"], st["var"])
                hip.scale(O, keep, st["rm"], 1)
                hip.axpy(O, float(mom), st["mean"], 0, 1, st["rm"], 0, 1)
                hip.scale(O, keep, st["rv"], 1)
                hip.axpy(O, float(mom), st["var"], 0, 1, st["rv"], 0, 1)
                hip.copy(n, out, off, 1, st["x"], off, 1)
                hip.normalize(O, n, S, st["mean"], 1, st["var"], 1, out, off)
                hip.copy(n, out, off, 1, st["xn"], off, 1)
            else:
                hip.normalize(O, n, S, st["rm"], 1, st["rv"], 1, out, off)
            hip.forwardScaleAdd(n, out, off, O, st["scales"], st["b"], 1, S)
        if activate:
            hip.ActivateArray(n, out, off, st.get("act", ACT["LINEAR"]))

    def _sub_forward(self, l, L, st, step, inp, in_step, training):
        S, I = L["S"], st["I"]
        O, n = self._sub_dims(l, L, st)
        self.hip.gemm(False, True, S, O, I, 1.0, inp, in_step * S * I, I, st["w"], 0, I, 0.0,
                      st["out"], step * n, O)
        self._sub_bn_forward(l, L, st, step, training)

    def _sub_bn_backward(self, l, L, st, step, clamp):
        """Up to the two products (nconnectedlayer.pas:771-821).  clamp=False:
        lstmGatesBackward stored the slice clamped already (rnnDeltaBackward:
        clamped and derived)."""
        hip, S, T = self.hip, L["S"], L["T"]
        O, n = self._sub_dims(l, L, st)
        d, off = st["delta"], step * n
        if clamp:
            hip.clamp(T * n, 1.0, d, d)
            # (the slice's own delta: with an lstm gate's LINEAR it multiplies by one)
            hip.DeriveArray(n, st["out"], off, st.get("act", ACT["LINEAR"]), self._at(d, off))
        hip.backwardBias(O, st["bu"], n, d, off, 1, S)
        if l.bn:
            hip.addDots(n, O, S, st["xn"], d, off, st["su"])
            hip.forwardScale(n, d, off, O, st["scales"], 1, S)
            hip.meansAndVarsDelta(n, O, S, d, st["x"], off, st["mean"], st["var"], st["md"],
                                  st["vd"])
            hip.normalizeDelta(n, O, S, d, st["x"], off, st["mean"], st["var"], st["md"], st["vd"])

    def _sub_backward(self, l, L, st, step, inp, in_step, sd, sd_step, clamp=True):
        hip, S, I = self.hip, L["S"], st["I"]
        O, n = self._sub_dims(l, L, st)
        self._sub_bn_backward(l, L, st, step, clamp)
        d, off = st["delta"], step * n
        hip.gemm(True, False, O, I, S, 1.0, d, off, O, inp, in_step * S * I, I, 1.0, st["wu"], 0, I)
        if sd is not None:
            hip.gemm(False, False, S, I, O, 1.0, d, off, O, st["w"], 0, I, 1.0, sd,
                     sd_step * S * I, I)

    @staticmethod
    def _at(t, off):  # a raw device pointer off floats into t
        return t.data_ptr() + 4 * off

    # -- forward ---------------------------------------------------------------
    def _lstm_forward(self, l, inp, training):
        hip, L = self.hip, self.lstm[l.index]
        S, T, n, O, I = L["S"], L["T"], L["n"], l.filters, l.in_size
        sub, out, cell = L["sub"], self.out[l.index], L["cell"]
        inp = inp.reshape(-1)
        if training:  # nlstmlayer.pas:901-911 (the layer's own delta: the caller)
            for g in LSTM_GATES:
                hip.fill(T * n, sub[g]["delta"], 0, 0.0, 1)
        if not self.lstm_fused:
            for i in range(T):
                off = i * n
                for g in self.W:
                    self._sub_forward(l, L, sub[g], i, L["h"], 0, training)
                for g in self.U:
                    self._sub_forward(l, L, sub[g], i, inp, i, training)
                for g, dst in zip("figo", ("_f", "_i", "_g", "_o")):
                    hip.addvv(n, sub["w" + g]["out"], off, 1, sub["u" + g]["out"], off, 1, L[dst],
                              0, 1)
                hip.ActivateArray(n, L["_f"], 0, ACT["LOGISTIC"])
                hip.ActivateArray(n, L["_i"], 0, ACT["LOGISTIC"])
                hip.ActivateArray(n, L["_o"], 0, ACT["LOGISTIC"])
                hip.ActivateArray(n, L["_g"], 0, ACT["TANH"])
                hip.mulvv(n, L["_i"], 0, 1, L["_g"], 0, 1, L["_temp"], 0, 1)
                hip.fmavv(n, L["c"], 0, 1, L["_f"], 0, 1, L["_temp"], 0, 1, L["c"], 0, 1)
                hip.copy(n, L["c"], 0, 1, L["h"], 0, 1)
                hip.ActivateArray(n, L["h"], 0, ACT["TANH"])
                hip.mulvv(n, L["_o"], 0, 1, L["h"], 0, 1, L["h"], 0, 1)
                hip.copy(n, L["c"], 0, 1, cell, off, 1)
                hip.copy(n, L["h"], 0, 1, out, off, 1)
            return
        # the input-side products of every step and gate at once: an NT
        # product's element is one sdot of an input row and a weight row
        hip.gemmStridedBatched(False, True, T * S, O, I, 1.0, inp, 0, I, 0, L["u_w"], 0, I, O * I,
                               0.0, L["u_out"], 0, O, T * n, 4)
        for g in self.U:
            if l.bn:  # statistics are per step
                for i in range(T):
                    self._sub_bn_forward(l, L, sub[g], i, training)
            else:     # a row's bias add does not depend on its step
                hip.forwardBias(T * n, sub[g]["out"], 0, O, sub[g]["b"], 1, T * S)
        at = self._at
        for i in range(T):
            off = i * n
            hip.gemmStridedBatched(False, True, S, O, O, 1.0, L["h"], 0, O, 0, L["w_w"], 0, O,
                                   O * O, 0.0, L["w_out"], off, O, T * n, 4)
            for g in self.W:
                self._sub_bn_forward(l, L, sub[g], i, training)
            hip.lstmGatesForward(n, [at(sub[g]["out"], off) for g in self.W],
                                 [at(sub[g]["out"], off) for g in self.U], L["c"], L["h"],
                                 at(cell, off), at(out, off))

    # -- backward ----------------------------------------------------------------
    def _lstm_backward(self, l, inp, sd):
        hip, L = self.hip, self.lstm[l.index]
        S, T, n, O, I = L["S"], L["T"], L["n"], l.filters, l.in_size
        sub, out, cell, delta = L["sub"], self.out[l.index], L["cell"], self.delta[l.index]
        inp = inp.reshape(-1)
        if not self.lstm_fused:
            for i in range(T - 1, -1, -1):
                off = i * n
                if i:
                    hip.copy(n, cell, off - n, 1, L["prevCell"], 0, 1)
                hip.copy(n, cell, off, 1, L["c"], 0, 1)
                if i:
                    hip.copy(n, out, off - n, 1, L["prevState"], 0, 1)
                hip.copy(n, out, off, 1, L["h"], 0, 1)
                for g, dst in zip("figo", ("_f", "_i", "_g", "_o")):
                    hip.addvv(n, sub["w" + g]["out"], off, 1, sub["u" + g]["out"], off, 1, L[dst],
                              0, 1)
                hip.ActivateArray(n, L["_f"], 0, ACT["LOGISTIC"])
                hip.ActivateArray(n, L["_i"], 0, ACT["LOGISTIC"])
                hip.ActivateArray(n, L["_o"], 0, ACT["LOGISTIC"])
                hip.ActivateArray(n, L["_g"], 0, ACT["TANH"])
                t1, t2, t3 = L["_temp"], L["_temp2"], L["_temp3"]
                hip.copy(n, delta, off, 1, t3, 0, 1)
                hip.copy(n, L["c"], 0, 1, t1, 0, 1)
                hip.ActivateArray(n, t1, 0, ACT["TANH"])
                hip.mulvv(n, t3, 0, 1, L["_o"], 0, 1, t2, 0, 1)
                hip.DeriveArray(n, t1, 0, ACT["TANH"], t2)
                hip.addvv(n, L["dc"], 0, 1, t2, 0, 1, t2, 0, 1)
                hip.copy(n, L["c"], 0, 1, t1, 0, 1)
                hip.ActivateArray(n, t1, 0, ACT["TANH"])
                hip.mulvv(n, t3, 0, 1, t1, 0, 1, t1, 0, 1)
                hip.DeriveArray(n, L["_o"], 0, ACT["LOGISTIC"], t1)
                dh = delta if i else None
                for g, other, act in (("o", None, None), ("g", "_i", "TANH"),
                                      ("i", "_g", "LOGISTIC"), ("f", "prevCell", "LOGISTIC")):
                    if other is not None:
                        hip.mulvv(n, t2, 0, 1, L[other], 0, 1, t1, 0, 1)
                        hip.DeriveArray(n, L["_" + g], 0, ACT[act], t1)
                    hip.copy(n, t1, 0, 1, sub["w" + g]["delta"], off, 1)
                    self._sub_backward(l, L, sub["w" + g], i, L["prevState"], 0, dh, i - 1)
                    hip.copy(n, t1, 0, 1, sub["u" + g]["delta"], off, 1)
                    self._sub_backward(l, L, sub["u" + g], i, inp, i, sd, i)
                hip.mulvv(n, t2, 0, 1, L["_f"], 0, 1, t1, 0, 1)
                hip.copy(n, t1, 0, 1, L["dc"], 0, 1)
            return
        at = self._at
        for i in range(T - 1, -1, -1):
            off = i * n
            if i == 0 and T > 1:  # the copies of step 1; step 0 makes none (stale operands)
                hip.copy(n, cell, 0, 1, L["prevCell"], 0, 1)
                hip.copy(n, out, 0, 1, L["prevState"], 0, 1)
            cprev = at(cell, off - n) if i else L["prevCell"]
            hprev, hoff = (out, off - n) if i else (L["prevState"], 0)
            hip.lstmGatesBackward(n, [at(sub[g]["out"], off) for g in self.W],
                                  [at(sub[g]["out"], off) for g in self.U], at(cell, off), cprev,
                                  at(delta, off), L["dc"],
                                  [at(sub[g]["delta"], off) for g in self.W],
                                  [at(sub[g]["delta"], off) for g in self.U])
            for g in LSTM_GATES:
                self._sub_bn_backward(l, L, sub[g], i, False)
            # the dW products: four outputs each, one operand shared
            hip.gemmStridedBatched(True, False, O, O, S, 1.0, L["w_delta"], off, O, T * n, hprev,
                                   hoff, O, 0, 1.0, L["w_wu"], 0, O, O * O, 4)
            hip.gemmStridedBatched(True, False, O, I, S, 1.0, L["u_delta"], off, O, T * n, inp,
                                   i * S * I, I, 0, 1.0, L["u_wu"], 0, I, O * I, 4)
            if i:  # into the layer's own delta, slice i-1, in the reference's order
                for g in ("wo", "wg", "wi", "wf"):
                    hip.gemm(False, False, S, O, O, 1.0, sub[g]["delta"], off, O, sub[g]["w"], 0, O,
                             1.0, delta, off - n, O)
        if sd is not None:  # slice i of the layer below's delta takes step i's four products
            for g in ("uo", "ug", "ui", "uf"):
                hip.gemm(False, False, T * S, I, O, 1.0, sub[g]["delta"], 0, O, sub[g]["w"], 0, I,
                         1.0, sd, 0, I)
        hip.copy(n, cell, 0, 1, L["c"], 0, 1)
        hip.copy(n, out, 0, 1, L["h"], 0, 1)

    def _lstm_update(self, l, learning_rate, momentum, decay):
        for g in LSTM_GATES:  # TLSTMLayer.updateGPU's order (nlstmlayer.pas:1281-1288)
            st = self.lstm[l.index]["sub"][g]
            self.hip.sgdUpdate(st["w"], st["wu"], st["b"], st["bu"], learning_rate,
                               self.net.batch, decay, momentum, st.get("scales"), st.get("su"))


class _RnnLayers:
    """The rnn layers of a driver (TRNNLayer.forward / backward / update, the
    CPU path, nrnnlayer.pas:148-257, 345-400 — the reference's device path
    disagrees with it), beside ``_LstmLayers``, whose sub-layer
    helpers it uses.  Rows are [step][stream]; n = streams * hidden floats
    make one hidden slice, m = streams * outputs one output slice.

    State per layer: ``state`` ((steps + 1) * n, zero at construction; a
    training forward zeroes slice 0, an inference forward nothing) and the
    three connected sub-layers input, self, output with what ``_fc_forward`` /
    ``_fc_backward`` keep, outputs and deltas steps * n (steps * m) long.  The
    output sub-layer's output and delta ARE the layer's.

    ``rnn_fused=False`` is the reference's call sequence, call for call
    through the existing TNNHip methods, the whole-delta clamp of every
    sub-layer backward included.  ``rnn_fused=True`` is the product path: one
    ``rnnStateForward`` per step, ``rnnDeltaBackward`` for the clamp + derive
    (+ copy + clamp + derive), and products regrouped only where every output
    element keeps its operands and its order of additions (the RNN
    section)."""

    def _rnn_init(self, blocks, training):
        torch, dev = self.torch, "cuda"
        z = lambda n: torch.zeros(n, device=dev)  # noqa: E731
        self.rnn = {}
        by_layer = {}
        for l, p in blocks:
            by_layer.setdefault(l.index, {})[l.gate] = (l, p)
        for l in self.net.rnns():
            T = l.steps
            S = self.net.batch // T
            L = {"S": S, "T": T, "n": S * l.hidden, "m": S * l.filters,
                 "state": z((T + 1) * S * l.hidden), "sub": {}}
            for g in RNN_SUBS:
                b, p = by_layer[l.index][g]
                O, K = b.filters, b.in_size
                own = g == "output"  # the layer's own buffers
                st = {"I": K, "O": O, "act": b.activation, "w": self._t(p.weights).reshape(-1),
                      "b": self._t(p.biases),
                      "out": self.out[l.index] if own else z(T * S * O)}
                if l.bn:
                    st.update(scales=self._t(p.scales), rm=self._t(p.rolling_mean),
                              rv=self._t(p.rolling_var))
                if training:
                    st.update(wu=z(O * K), bu=z(O),
                              delta=self.delta[l.index] if own else z(T * S * O))
                    if l.bn:
                        st.update(mean=z(O), var=z(O), x=z(T * S * O), xn=z(T * S * O), su=z(O),
                                  md=z(O), vd=z(O))
                L["sub"][g] = st
            self.rnn[l.index] = L

    def reset_state(self):
        """Zero every rnn layer's whole ``state`` (no inference pass does: the
        reference carries it from call to call), and the lstm layers' state."""
        for L in self.rnn.values():
            L["state"].zero_()
        super().reset_state()

    # -- forward ---------------------------------------------------------------
    def _rnn_forward(self, l, inp, training):
        hip, L, at = self.hip, self.rnn[l.index], self._at
        S, T, n, m, H, O, I = L["S"], L["T"], L["n"], L["m"], l.hidden, l.filters, l.in_size
        si, ss, so = (L["sub"][g] for g in RNN_SUBS)
        state = L["state"]
        inp = inp.reshape(-1)
        if training:  # nrnnlayer.pas:241-246: delta.multiply(0), state.FillExt(0, 0, n)
            hip.scale(T * m, 0.0, so["delta"], 1)
            hip.scale(T * n, 0.0, ss["delta"], 1)
            hip.scale(T * n, 0.0, si["delta"], 1)
            hip.fill(n, state, 0, 0.0, 1)
        j0 = 1 if training else 0  # step i writes state[i + j0] (rnnStepForward's j)
        if not self.rnn_fused:
            for i in range(T):
                j = i + j0
                self._sub_forward(l, L, si, i, inp, i, training)
                self._sub_forward(l, L, ss, i, state, i, training)
                if not l.shortcut:
                    hip.fill(n, state, j * n, 0.0, 1)
                elif j != i:  # (j = i: the slice onto itself)
                    hip.copy(n, state, i * n, 1, state, j * n, 1)
                hip.addvv(n, state, j * n, 1, si["out"], i * n, 1, state, j * n, 1)
                hip.addvv(n, state, j * n, 1, ss["out"], i * n, 1, state, j * n, 1)
                self._sub_forward(l, L, so, i, state, j, training)
            return
        # the input sub-layer's products of every step at once: an NT product's
        # element is one sdot of an input row and a weight row
        hip.gemm(False, True, T * S, H, I, 1.0, inp, 0, I, si["w"], 0, I, 0.0, si["out"], 0, H)
        if l.bn and not training:  # by the rolling statistics: per element, any grouping
            hip.normalize(H, T * n, T * S, si["rm"], 1, si["rv"], 1, si["out"], 0)
            hip.forwardScaleAdd(T * n, si["out"], 0, H, si["scales"], si["b"], 1, T * S)
        for i in range(T):
            off = i * n
            hip.gemm(False, True, S, H, H, 1.0, state, off, H, ss["w"], 0, H, 0.0, ss["out"], off,
                     H)
            if l.bn:  # training: the statistics are per step
                if training:
                    self._sub_bn_forward(l, L, si, i, True, activate=False)
                self._sub_bn_forward(l, L, ss, i, training, activate=False)
            hip.rnnStateForward(n, H, at(si["out"], off), None if l.bn else si["b"], si["act"],
                                at(ss["out"], off), None if l.bn else ss["b"], ss["act"],
                                at(state, off) if l.shortcut else None, at(state, off + j0 * n))
        # the output sub-layer after the loop: step i reads state[i + j0], which
        # step i alone writes and no later step changes (in inference the steps
        # of one call do not chain: step i + 1 reads state[i + 1], not this one)
        hip.gemm(False, True, T * S, O, H, 1.0, state, j0 * n, H, so["w"], 0, H, 0.0, so["out"], 0,
                 O)
        if not l.bn:
            hip.forwardBias(T * m, so["out"], 0, O, so["b"], 1, T * S)
        elif training:
            for i in range(T):
                self._sub_bn_forward(l, L, so, i, True, activate=False)
        else:
            hip.normalize(O, T * m, T * S, so["rm"], 1, so["rv"], 1, so["out"], 0)
            hip.forwardScaleAdd(T * m, so["out"], 0, O, so["scales"], so["b"], 1, T * S)
        hip.ActivateArray(T * m, so["out"], 0, so["act"])

    # -- backward ----------------------------------------------------------------
    def _rnn_backward(self, l, inp, sd):
        hip, L, at = self.hip, self.rnn[l.index], self._at
        S, T, n, m, H, I = L["S"], L["T"], L["n"], L["m"], l.hidden, l.in_size
        si, ss, so = (L["sub"][g] for g in RNN_SUBS)
        state = L["state"]
        inp = inp.reshape(-1)
        fused = self.rnn_fused
        for i in range(T - 1, -1, -1):
            off, offm = i * n, i * m
            # one add over the forward's value (the shortcut term dropped, as
            # the reference drops it); state[i] below is still the forward's
            hip.addvv(n, si["out"], off, 1, ss["out"], off, 1, state, off + n, 1)
            if fused:
                hip.rnnDeltaBackward(m, at(so["delta"], offm), at(so["out"], offm), so["act"])
            self._sub_backward(l, L, so, i, state, i + 1, ss["delta"], i, clamp=not fused)
            if fused:  # without batch norm the slice is final here: the input
                # sub-layer's copy, clamp and derive ride along
                chain = not l.bn
                hip.rnnDeltaBackward(n, at(ss["delta"], off), at(ss["out"], off), ss["act"],
                                     at(si["delta"], off) if chain else None,
                                     at(si["out"], off) if chain else None, si["act"])
            self._sub_backward(l, L, ss, i, state, i, ss["delta"] if i else None, i - 1,
                               clamp=not fused)
            if not fused or l.bn:
                hip.copy(n, ss["delta"], off, 1, si["delta"], off, 1)
            if fused and l.bn:
                hip.rnnDeltaBackward(n, at(si["delta"], off), at(si["out"], off), si["act"])
            if i and l.shortcut:
                hip.addvv(n, ss["delta"], off - n, 1, ss["delta"], off, 1, ss["delta"], off - n, 1)
            self._sub_backward(l, L, si, i, inp, i, None if fused else sd, i, clamp=not fused)
        if not fused:
            return
        if sd is not None:  # slice i of the layer below's delta takes step i's product alone
            hip.gemm(False, False, T * S, I, H, 1.0, si["delta"], 0, H, si["w"], 0, I, 1.0, sd, 0,
                     I)
        if l.bn and T > 1:
            # the reference clamps the whole delta at every step: a slice that
            # normalizeDelta pushed outside [-1, 1] is clamped by the next step
            # (and no further: clamping is idempotent).  Nothing reads slice i
            # after step i, so one clamp of slices 1 .. T-1 leaves the layer's
            # delta as the reference does; slice 0 is processed last
            hip.clamp((T - 1) * m, 1.0, so["delta"], so["delta"], 1, m)

    def _rnn_update(self, l, learning_rate, momentum, decay):
        for g in RNN_SUBS:  # TRNNLayer.update's order (nrnnlayer.pas:393-395)
            st = self.rnn[l.index]["sub"][g]
            self.hip.sgdUpdate(st["w"], st["wu"], st["b"], st["bu"], learning_rate,
                               self.net.batch, decay, momentum, st.get("scales"), st.get("su"))


def detection_rows_to_host(torch, taken, cap, classes, boxes, obj, probs, pin=None):
    """The first taken[b] rows of every image b out of the device row buffers
    (``cap`` rows an image) as NumPy arrays: asynchronous copies of exactly
    those rows into one pinned host buffer, then one synchronisation.
    ``pin``: the buffer of an earlier call, reused while it is large enough.
    Returns ([(boxes [n, 4], objectness [n], probs [n, classes])], pin)."""
    total = sum(taken)
    need = max(total * (5 + classes), 1)
    if pin is None or pin.numel() < need:
        pin = torch.empty(need, dtype=torch.float32).pin_memory()
    hb, ho, hp = pin[:4 * total], pin[4 * total:5 * total], pin[5 * total:need]
    at = 0
    for b, n in enumerate(taken):
        if n:
            hb[4 * at:4 * (at + n)].copy_(boxes[b * cap * 4:(b * cap + n) * 4], non_blocking=True)
            ho[at:at + n].copy_(obj[b * cap:b * cap + n], non_blocking=True)
            if classes:
                hp[classes * at:classes * (at + n)].copy_(
                    probs[b * cap * classes:(b * cap + n) * classes], non_blocking=True)
        at += n
    torch.cuda.current_stream().synchronize()
    res, at = [], 0
    for n in taken:
        res.append((hb[4 * at:4 * (at + n)].numpy().reshape(n, 4).copy(),
                    ho[at:at + n].numpy().copy(),
                    hp[classes * at:classes * (at + n)].numpy().reshape(n, classes).copy()))
        at += n
    return res, pin


@dataclass
class Placement:
    """Where ``images_to_input`` put one image: the resize target new_w x
    new_h at (dx, dy) of the net input, the source's extent, and
    letterBoxEx's ratio (None without ``letter``)."""
    new_w: int
    new_h: int
    dx: int
    dy: int
    w: int
    h: int
    ratio: object = None


def images_to_input(hip, torch, images, channels, net_w, net_h, dst, letter=False, table="fpc"):
    """TImageData.resize, or with ``letter`` letterBoxEx (ntypes.pas:837-947),
    of every image into dst [len(images), channels, net_h, net_w] on the
    device (TNNHip.imageToInput, one launch).  ``images``: uint8 [h, w, c]
    arrays (interleaved, as decoders deliver them; c >= channels, the first
    ``channels`` of a pixel are taken) or float32 [channels, h, w] arrays
    (TImageData's layout), NumPy or device tensors, all of one kind, of
    differing sizes.  Host images cross as their own bytes in one copy.
    Returns a Placement per image."""
    if not images:
        return []
    on_dev = [hasattr(im, "is_cuda") for im in images]
    if any(on_dev) and not all(on_dev):
        raise ValueError("images: NumPy arrays and tensors in one call")
    kinds = {str(im.dtype).replace("torch.", "") for im in images}
    if len(kinds) != 1 or kinds & {"uint8", "float32"} != kinds:
        raise ValueError(f"images: one of uint8 / float32 for all of them, got {sorted(kinds)}")
    as_bytes = kinds == {"uint8"}
    geom, at, ps = [], 0, None
    for n, im in enumerate(images):
        if im.ndim != 3:
            raise ValueError(f"image {n}: shape {tuple(im.shape)}")
        h, w, c = im.shape if as_bytes else (im.shape[1], im.shape[2], im.shape[0])
        if (c < channels or c > 4) if as_bytes else c != channels:
            raise ValueError(f"image {n}: {c} channels for a network of {channels}")
        if as_bytes and ps not in (None, c):
            raise ValueError(f"image {n}: {c} bytes a pixel after images of {ps}")
        ps = c
        geom.append((at, w, h, w * c if as_bytes else w))
        at += h * w * c
    if all(on_dev):
        src = torch.cat([im.contiguous().reshape(-1) for im in images])
    else:
        src = torch.from_numpy(np.concatenate(
            [np.ascontiguousarray(im).reshape(-1) for im in images])).cuda()
    placed = hip.imageToInput(src, geom, channels, net_w, net_h, dst, letter=letter, table=table,
                              pixelStride=ps if as_bytes else None)
    res = []
    for (nw, nh, dx, dy), (_, w, h, _) in zip(placed, geom):
        ratio = None
        if letter:  # letterBoxEx: aWidth / self.w or aHeight / self.h, a real stored to a single
            ratio = np.float32(net_w / w) if net_w * h < net_h * w else np.float32(net_h / h)
        res.append(Placement(nw, nh, dx, dy, w, h, ratio))
    return res


def letterbox_truth(boxes, placements, net_w, net_h, max_boxes):
    """loadVOCBatch's truth rows (Samples/FPC/MSCOCO_Yolo/MSCOCOYolo.pas:
    461-480) for images letterboxed by ``images_to_input(letter=True)``:
    ``boxes[b]`` is image b's objects in file order, each (xmin, ymin, xmax,
    ymax, class) in source pixels, or None for one the sample skips
    (`difficult`), whose row stays zero.  left = dx + trunc(single(xmin) *
    ratio) and so on, then x = (left+right) / (2*netW), y likewise, w =
    (right-left) / netW, h likewise: integer quotients, reals stored to
    singles.  Returns float32 [len(boxes), max_boxes, 6] rows x, y, w, h,
    class, 0, zero after the last.  More than ``max_boxes`` objects are
    refused (the sample's loop admits one more and writes it into the next
    image's rows)."""
    F = np.float32
    out = np.zeros((len(boxes), max_boxes, 6), F)
    for b, (objs, p) in enumerate(zip(boxes, placements)):
        if len(objs) > max_boxes:
            raise ValueError(f"image {b}: {len(objs)} objects, max_boxes {max_boxes}")
        for j, o in enumerate(objs):
            if o is None:
                continue
            left, top, right, bottom = (d + int(np.trunc(F(v) * p.ratio))
                                        for d, v in zip((p.dx, p.dy, p.dx, p.dy), o[:4]))
            out[b, j] = (F((left + right) / (2 * net_w)), F((top + bottom) / (2 * net_h)),
                         F((right - left) / net_w), F((bottom - top) / net_h), F(o[4]), 0)
    return out


class HipDarknet(_RnnLayers, _LstmLayers):
    """TNNet.forward over a darknet layer plan on the HIP backend (nnet.pas:
    275-310 selects forwardGPU per layer): every layer's output stays in a
    device buffer of its own; convolutions take BN-folded parameters
    (fuseBatchNorm) and run the fused implicit-GEMM driver.  Connected layers
    run TConnectedLayer.forwardGPU's inference branch (nconnectedlayer.pas:
    640-733: NT gemm, normalize by the rolling statistics + forwardScaleAdd,
    or forwardBias, then ActivateArray).  A dropout layer's output is its
    input buffer and nothing runs (ndropoutlayer.pas:156-161); softmax is
    softmaxBatch, logistic copy + ActivateArray, cost nothing (no truth).
    An lstm layer (``_LstmLayers``) carries c and h from one forward to the
    next until ``reset_state()``; its batch-normalized sub-layers normalize
    by the rolling statistics.  An rnn layer (``_RnnLayers``) likewise carries
    its ``state``: with time_steps = 1 from call to call; with more, step i of
    a call reads what step i of the call before left (the reference's
    inference does not chain the steps of one call)."""

    def __init__(self, hip, net: Network, params: list[ConvParams], torch,
                 lstm_fused: bool = True, rnn_fused: bool = True):
        self.hip, self.net, self.torch = hip, net, torch
        self.lstm_fused = bool(lstm_fused)
        self.rnn_fused = bool(rnn_fused)
        B = net.batch
        dev = "cuda"
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
        self.out = []
        for l in net.layers:  # (a dropout at layer 0 takes the input in forward)
            alias = l.kind == "dropout" and l.index > 0
            self.out.append(self.out[-1] if alias else torch.empty(B * l.out_size, device=dev))
        self.conv_params, self.fc_params = {}, {}
        blocks = list(zip(net.param_layers(), params))
        kind = lambda b: net.layers[b[0].index].kind if b[0].gate else ""  # noqa: E731
        self._lstm_init([b for b in blocks if kind(b) == "lstm"], training=False)
        self._rnn_init([b for b in blocks if kind(b) == "rnn"], training=False)
        for l, p in blocks:
            if l.gate:
                continue
            if l.kind == "connected":
                st = {"w": t(p.weights), "b": t(p.biases)}
                if l.bn:
                    st.update(scales=t(p.scales), rm=t(p.rolling_mean), rv=t(p.rolling_var))
                self.fc_params[l.index] = st
                continue
            f = fuse_batchnorm(l, p)
            self.conv_params[l.index] = (t(f.weights), t(f.biases))

    def forward(self, x):
        """x: device tensor [batch, c, h, w] (contiguous).  Returns the per-
        layer output buffers (``detections`` turns the yolo layers' into
        boxes and scores)."""
        hip, B = self.hip, self.net.batch
        prev = x
        for l in self.net.layers:
            out = self.out[l.index]
            if l.kind == "convolutional":
                w, b = self.conv_params[l.index]
                hip.convForward(B, l.c, l.h, l.w, prev, w, b, l.filters, l.size, l.stride, l.pad,
                                1, l.activation, None, out, fused=True)
            elif l.kind == "shortcut":
                src = self.out[l.inputs[0]]
                hip.shortcut(B * l.out_size, prev, 0, src, 0, out, 0, l.activation)
            elif l.kind == "route":  # TTensor.concat: whole tensors in order
                off = 0
                for s in l.inputs:
                    n = B * self.net.layers[s].out_size
                    hip.copy(n, self.out[s], 0, 1, out, off, 1)
                    off += n
            elif l.kind == "upsample":
                hip.upSample(B, l.c, l.h, l.w, prev, l.stride, 1, 1.0, out)
            elif l.kind == "yolo":
                hip.yoloForward(B, l.anchors, l.classes, l.h * l.w, prev, out)
            elif l.kind == "maxpool":  # inference: no indexes
                hip.forwardMaxPool(B, l.out_c, l.out_h, l.out_w, prev, l.c, l.h, l.w, l.stride_x,
                                   l.stride_y, l.pad, l.size, None, out)
            elif l.kind == "local_avgpool":
                hip.forwardAvgPool(B, l.out_c, l.out_h, l.out_w, prev, l.c, l.h, l.w, l.stride_x,
                                   l.stride_y, l.pad, l.size, out)
            elif l.kind == "connected":
                st, n = self.fc_params[l.index], B * l.filters
                hip.gemm(False, True, B, l.filters, l.in_size, 1.0, prev, 0, l.in_size, st["w"], 0,
                         l.in_size, 0.0, out, 0, l.filters)
                if l.bn:
                    hip.normalize(l.filters, n, B, st["rm"], 1, st["rv"], 1, out, 0)
                    hip.forwardScaleAdd(n, out, 0, l.filters, st["scales"], st["b"], 1, B)
                else:
                    hip.forwardBias(n, out, 0, l.filters, st["b"], 1, B)
                hip.ActivateArray(n, out, 0, l.activation)
            elif l.kind == "lstm":
                self._lstm_forward(l, prev, False)
            elif l.kind == "rnn":
                self._rnn_forward(l, prev, False)
            elif l.kind == "dropout":
                out = self.out[l.index] = prev.reshape(-1)
            elif l.kind == "softmax":
                g = l.in_size // l.groups
                hip.softmaxBatch(g, prev, 0, B, l.in_size, l.groups, g, 1, l.temperature, out, 0)
            elif l.kind == "logistic":
                hip.copy(B * l.in_size, prev, 0, 1, out, 0, 1)
                hip.ActivateArray(B * l.in_size, out, 0, l.activation)
            prev = out
        return self.out

    def detections(self, im_w, im_h, thresh=0.5, relative=False, letter=False, nms=None,
                   capacity=None):
        """TNNet.Detections (nnet.pas:584-677) for every image of the batch,
        then TDetections.doNMSSort (ntypes.pas:1612-1649) when ``nms`` is a
        threshold, on the device; call it after ``forward``.  The [yolo]
        layers are collected in network order into one row buffer
        (TNNHip.yoloDetections appends through a per-image device counter),
        so the rows stand in the reference's order: layer, then cell, then
        anchor.  Returns, per image, ``(boxes [rows, 4], objectness [rows],
        probs [rows, classes])`` as NumPy arrays of exactly the taken rows;
        only the counters and those rows are copied back.  After NMS the rows
        keep their place (the reference leaves them in the last class's sort
        order).  ``capacity``: rows an image; the default, the sum of
        anchors*h*w over the yolo layers, cannot overflow, a smaller one
        raises TnsError when an image has more taken candidates."""
        hip, torch, B = self.hip, self.torch, self.net.batch
        yolos = [l for l in self.net.layers if l.kind == "yolo"]
        if not yolos:
            raise ValueError("detections: the network has no [yolo] layer")
        # the reference sizes every row's prob by the first layer's classes
        # (nnet.pas:625) and lets a later layer write its own count into it
        if len({l.classes for l in yolos}) > 1:
            raise ValueError("detections: the [yolo] layers disagree on classes: "
                             f"{[l.classes for l in yolos]}")
        bad = [f"layer {l.index} {k}" for l in yolos for k in l.unbuilt
               if k in ("new_coords", "embedding_layer")]
        if bad:
            raise ValueError("detections: not built: " + ", ".join(bad))
        classes = yolos[0].classes
        cap = sum(l.anchors * l.h * l.w for l in yolos) if capacity is None else int(capacity)
        if cap < 1:
            raise ValueError(f"detections: capacity {cap}")
        key = (cap, classes)
        if getattr(self, "_det_key", None) != key:
            self._det_key = key
            self._det = (torch.zeros(B, dtype=torch.int64, device="cuda"),
                         torch.empty(B * cap * 4, device="cuda"),
                         torch.empty(B * cap, device="cuda"),
                         torch.empty(B * cap * max(classes, 1), device="cuda"))
        counts, boxes, obj, probs = self._det
        hip.fill(2 * B, counts.data_ptr(), 0, 0.0, 1)  # int64 zeros, on the backend's stream
        for l in yolos:
            hip.yoloDetections(B, l.anchors, classes, l.h, l.w, l.total, l.mask, l.biases,
                               self.net.w, self.net.h, im_w, im_h, thresh, relative, letter,
                               self.out[l.index], cap, counts, boxes, obj, probs)
        if nms is not None:
            hip.nmsSort(B, cap, classes, counts, boxes, obj, probs, nms)
        hip.finish()
        taken = counts.cpu().tolist()
        for b, n in enumerate(taken):
            if n > cap:
                raise TnsError(f"detections: image {b} has {n} taken candidates, capacity {cap}")
        res, self._det_pin = detection_rows_to_host(torch, taken, cap, classes, boxes, obj, probs,
                                                    getattr(self, "_det_pin", None))
        return res

    def load_images(self, images, letter=False, table="fpc"):
        """The batch's images (``images_to_input``: uint8 [h, w, c] or float32
        [c, h, w], NumPy or device, of differing sizes) resized to the net
        input as the sample does before ``predict`` (MSCOCOYolo.pas:348-358),
        or letterboxed with ``letter``, on the device.  Returns the [batch, c,
        h, w] device input, a buffer this object keeps and the next call
        overwrites, and a Placement per image."""
        net = self.net
        if len(images) != net.batch:
            raise ValueError(f"{len(images)} images for a batch of {net.batch}")
        if getattr(self, "_input", None) is None:
            self._input = self.torch.empty((net.batch, net.c, net.h, net.w), device="cuda")
        placed = images_to_input(self.hip, self.torch, images, net.c, net.w, net.h, self._input,
                                 letter=letter, table=table)
        return self._input, placed

    def detect_images(self, images, thresh=0.5, nms=None, letter=False, relative=True,
                      table="fpc"):
        """``load_images`` -> ``forward`` -> ``detections``: decoded images in,
        per image (boxes, objectness, probs) out.  ``detections`` corrects the
        boxes by one image extent for the whole batch, and with ``letter`` or
        without ``relative`` the boxes depend on it, so images of differing
        sizes are then refused; the sample's mode (resize, relative) takes
        them mixed."""
        x, placed = self.load_images(images, letter=letter, table=table)
        sizes = {(p.w, p.h) for p in placed}
        if len(sizes) > 1 and (letter or not relative):
            raise ValueError("detect_images: images of differing sizes "
                             f"{sorted(sizes)} with letter=True or relative=False: the boxes' "
                             "correction takes one image extent for the whole batch")
        self.forward(x)
        im_w, im_h = (placed[0].w, placed[0].h)
        return self.detections(im_w, im_h, thresh=thresh, relative=relative, letter=letter,
                               nms=nms)


class HipDarknetTrain(_RnnLayers, _LstmLayers):
    """One training pass of a darknet network on the HIP backend, in the
    reference's call order: TNet.forward in training (nnet.pas:275-322; each
    layer's delta zeroed by ``cuda.scale(size, 0, delta, 1)`` before its
    forward) and TNet.backward (nnet.pas:323-366: layers from the last to the
    first, layer i's state.delta = layer i-1's delta, none for layer 0),
    each layer through the TNNHip call its backwardGPU makes:

    * convolutional: ``convBackwardBN`` (batch-normalized layers:
      Derivative + batchNormBack + dW + state.delta, nConvolutionLayer.pas:
      571-671 -> nbaselayer.pas:372-395) or ``convBackward`` (the 1x1
      detection heads: Derivative + addSums + dW + state.delta);
    * shortcut (TAddLayer.backwardGPU, naddlayer.pas:924-949): DeriveArray,
      then ``addvv`` of its delta into state.delta and into the from-layer's
      delta;
    * route (TConcatLayer.backwardGPU, nconcatlayer.pas:234-256): ``addvv`` of
      its delta slices into each input layer's delta;
    * upsample (TUpSampleLayer.backwardGPU, nupsamplelayer.pas:214-228):
      ``upSample(..., isForward = 0)`` accumulating into state.delta;
    * yolo (TYoloLayer.backwardGPU, nyololayer.pas:1112-1125): ``axpy`` of its
      delta (scaled by lossScale*deltaNormalizer) into state.delta.  With
      ``yolo_loss=True`` the training forward fills that delta and the
      layer's cost from the truth boxes (``yoloLoss``, TYoloLayer.forward
      under state.isTraining, nyololayer.pas:835-1003); without it
      ``set_yolo_deltas`` supplies the delta;
    * maxpool / local_avgpool (TMaxPoolLayer.backwardGPU, nMaxPoolLayer.pas:
      689-706; CPU loops 501-542): ``backwardMaxPool`` with the indexes its
      forward stored, or ``backwardAvgPool``, accumulating into state.delta;
      nothing when the pool is layer 0 (no state.delta);
    * connected (TConnectedLayer.forwardGPU / backwardGPU, nconnectedlayer.pas:
      612-871): NT ``gemm``; with batch norm ``means``, ``variances``, the
      rolling statistics by ``scale`` / ``axpy`` (bnMomentum 0.05, line 67),
      ``copy`` to x, ``normalize``, ``copy`` to x_norm, ``forwardScaleAdd``,
      otherwise ``forwardBias``; ``ActivateArray``.  Backward: ``clamp(delta,
      1)``, ``DeriveArray``, ``backwardBias``, with batch norm ``addDots``,
      ``forwardScale``, ``meansAndVarsDelta``, ``normalizeDelta``, then the
      TN ``gemm`` into weight_updates and the NN ``gemm`` into state.delta;
    * dropout (ndropoutlayer.pas:156-172): ``output := state.input^`` — the
      layer's output buffer IS the layer below's, so ``forwardDropout`` runs
      in place on it (the layer below derives its activation from the dropped,
      scaled output) with the layer's rnd buffer; ``backwardDropout`` in place
      on state.delta, which the layer's delta aliases.  (The reference assigns
      that alias only at the end of the first backward, so its first step
      passes no gradient below a dropout layer; here the alias holds from the
      start);
    * softmax (nsoftmaxlayer.pas:279-341): ``softmaxBatch``; with truth and
      not noloss ``crossEntropySoftmax`` and cost = ``sum(loss)`` (vssum
      order); backward ``addvv`` of its delta into state.delta;
    * cost (ncostlayer.pas:218-228): ``costL2``, cost = ``sum(output)``;
      backward ``axpy(scale, delta, state.delta)``;
    * logistic (nlogisticlayer.pas:181-): ``copy``, ``ActivateArray``,
      ``crossEntropyLogistic``, cost = ``sum(loss)``; backward ``addvv``.

    Convolutions with batch norm run ``convForwardTrain`` (training-time BN,
    nbaselayer.pas:336-370) in the forward, the heads ``convForward``.
    ``update`` is TNNet.update (nnet.pas:371-403): ``sgdUpdate`` per layer,
    for an lstm layer on its eight sub-layers in the order wf wi wg wo uf ui
    ug uo, for an rnn layer on input, self, output.  lstm layers:
    ``_LstmLayers``; rnn layers: ``_RnnLayers``; ``lstm_fused=False`` /
    ``rnn_fused=False`` select the reference's call sequence, call for call."""

    LOSS_KINDS = ("softmax", "cost", "logistic")

    def __init__(self, hip, net: Network, params: list[ConvParams], torch, loss_scale: float = 1.0,
                 seed: int = 0, lstm_fused: bool = True, rnn_fused: bool = True,
                 yolo_loss: bool = False):
        self.hip, self.net, self.torch = hip, net, torch
        self.lstm_fused = bool(lstm_fused)
        self.rnn_fused = bool(rnn_fused)
        self.loss_scale = float(loss_scale)
        self.yolo_loss = bool(yolo_loss)
        yolos = [l for l in net.layers if l.kind == "yolo"]
        if self.yolo_loss:
            # what the device loss does not build is refused here, and only
            # here: inference and set_yolo_deltas training take these cfgs
            bad = [f"[net] {k}" for k in net.yolo_unbuilt]
            bad += [f"[yolo] layer {l.index} {k}" for l in yolos for k in l.unbuilt]
            if bad:
                raise ValueError("yolo_loss=True: the device loss does not build "
                                 + ", ".join(bad))
            if len({l.max_boxes for l in yolos}) > 1:
                raise ValueError("yolo_loss=True: the [yolo] layers disagree on max: "
                                 f"{[l.max_boxes for l in yolos]} (one truth tensor feeds all)")
        self.rng = np.random.default_rng(seed)  # default dropout seeds
        B = net.batch
        dev = "cuda"
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
        self.out, self.delta = [], []
        for l in net.layers:  # a dropout's output and delta are the layer below's
            alias = l.kind == "dropout" and l.index > 0
            self.out.append(self.out[-1] if alias else torch.zeros(B * l.out_size, device=dev))
            self.delta.append(self.delta[-1] if alias
                              else torch.zeros(B * l.out_size, device=dev))
        self.rnd = {l.index: torch.zeros(B * l.out_size, device=dev)
                    for l in net.layers if l.kind == "dropout"}
        # softmax / logistic: loss[batch*inputs]; every loss layer: cost[1]
        self.loss = {l.index: torch.zeros(B * l.out_size, device=dev)
                     for l in net.layers if l.kind in ("softmax", "logistic")}
        self.costs = {l.index: torch.zeros(1, device=dev)
                      for l in net.layers if l.kind in self.LOSS_KINDS}
        # the device yolo loss: cost[1] and the per-image {count, tot_iou} of
        # every yolo layer, and the network's {totalBBox, rewrittenBBox}
        self.yolo_stats = {}
        if self.yolo_loss:
            for l in yolos:
                self.costs[l.index] = torch.zeros(1, device=dev)
                self.yolo_stats[l.index] = torch.zeros(2 * B, device=dev)
            self.yolo_counters = torch.zeros(2, dtype=torch.int64, device=dev)
        self.fc = {}
        # a maxpool's indexes (TSizeIntTensor, int64): filled by its forward
        self.indexes = {l.index: torch.zeros(B * l.out_size, dtype=torch.int64, device=dev)
                        for l in net.layers if l.kind == "maxpool"}
        self.conv = {}
        ws = 1
        blocks = list(zip(net.param_layers(), params))
        kind = lambda b: net.layers[b[0].index].kind if b[0].gate else ""  # noqa: E731
        self._lstm_init([b for b in blocks if kind(b) == "lstm"], training=True)
        self._rnn_init([b for b in blocks if kind(b) == "rnn"], training=True)
        for l, p in blocks:
            if l.gate:
                continue
            n = B * l.out_size
            st = {"w": t(p.weights), "b": t(p.biases),
                  "wu": torch.zeros(p.weights.size, device=dev),
                  "bu": torch.zeros(l.filters, device=dev)}
            if l.bn:
                st.update(scales=t(p.scales), rm=t(p.rolling_mean), rv=t(p.rolling_var),
                          mean=torch.zeros(l.filters, device=dev),
                          var=torch.zeros(l.filters, device=dev),
                          x=torch.zeros(n, device=dev), xn=torch.zeros(n, device=dev),
                          su=torch.zeros(l.filters, device=dev),
                          md=torch.zeros(l.filters, device=dev),
                          vd=torch.zeros(l.filters, device=dev))
            if l.kind == "connected":
                self.fc[l.index] = st
                continue
            self.conv[l.index] = st
            ws = max(ws, B * l.c * l.size * l.size * l.out_h * l.out_w)
        self.ws = torch.empty(ws, device=dev)

    def load_batch(self, images, boxes, table="fpc"):
        """loadVOCBatch (MSCOCOYolo.pas:432-484) without the files: every
        image letterboxed into the net input on the device
        (``images_to_input(letter=True)``) and its objects' pixel boxes
        mapped into it (``letterbox_truth``; ``boxes[b]``: (xmin, ymin, xmax,
        ymax, class) per object).  Returns the device input [batch, c, h, w],
        kept by this object and overwritten by the next call, and the device
        truth [batch, max_boxes*6] that ``forward`` takes under
        ``yolo_loss``."""
        net, torch = self.net, self.torch
        yolos = [l for l in net.layers if l.kind == "yolo"]
        if not yolos:
            raise ValueError("load_batch: the network has no [yolo] layer")
        if len(images) != net.batch or len(boxes) != net.batch:
            raise ValueError(f"{len(images)} images and {len(boxes)} box lists for a batch of "
                             f"{net.batch}")
        if getattr(self, "_input", None) is None:
            self._input = torch.empty((net.batch, net.c, net.h, net.w), device="cuda")
        placed = images_to_input(self.hip, torch, images, net.c, net.w, net.h, self._input,
                                 letter=True, table=table)
        rows = letterbox_truth(boxes, placed, net.w, net.h, yolos[0].max_boxes)
        return self._input, torch.from_numpy(rows.reshape(net.batch, -1)).cuda()

    def forward(self, x, truth=None, seeds=None):
        """TNet.forward with state.isTraining (BN statistics of the batch,
        rolling statistics updated with bnMomentum 0.1, connected layers
        0.05).  truth: device tensor of the loss layers' size (state.truth),
        or None (no loss is computed); with ``yolo_loss`` the truth boxes
        [batch, max_boxes*6], the same tensor for every yolo layer.  seeds: one integer in [0, 2^32) per
        dropout layer, in layer order; by default drawn in [0, 2^28), the
        reference's random($10000000), from the generator seeded at
        construction."""
        hip, B = self.hip, self.net.batch
        drops = [l for l in self.net.layers if l.kind == "dropout"]
        if seeds is None:
            seeds = [int(self.rng.integers(0, 1 << 28)) for _ in drops]
        if len(seeds) != len(drops):
            raise ValueError(f"{len(seeds)} seeds for {len(drops)} dropout layers")
        seeds = dict(zip((l.index for l in drops), seeds))
        if truth is not None:
            truth = truth.reshape(-1)
        prev = x
        for l in self.net.layers:
            if l.kind == "dropout":  # its delta is the layer below's, zeroed there
                n = B * l.out_size
                if l.index == 0:
                    self.out[0] = prev.reshape(-1)
                out = self.out[l.index]
                hip.forwardDropout(n, out, l.probability, l.scale, self.rnd[l.index], out,
                                   seeds[l.index])
                prev = out
                continue
            hip.scale(self.delta[l.index].numel(), 0.0, self.delta[l.index], 1)
            out = self.out[l.index]
            if l.kind == "convolutional":
                st = self.conv[l.index]
                if l.bn:
                    hip.convForwardTrain(B, l.c, l.h, l.w, prev, st["w"], l.filters, l.size,
                                         l.stride, l.pad, 1, l.activation, st["scales"], st["b"],
                                         st["rm"], st["rv"], 0.1, True, st["mean"], st["var"],
                                         st["x"], st["xn"], self.ws, out)
                else:
                    hip.convForward(B, l.c, l.h, l.w, prev, st["w"], st["b"], l.filters, l.size,
                                    l.stride, l.pad, 1, l.activation, self.ws, out, fused=True)
            elif l.kind == "shortcut":
                hip.shortcut(B * l.out_size, prev, 0, self.out[l.inputs[0]], 0, out, 0,
                             l.activation)
            elif l.kind == "route":
                off = 0
                for s in l.inputs:
                    n = B * self.net.layers[s].out_size
                    hip.copy(n, self.out[s], 0, 1, out, off, 1)
                    off += n
            elif l.kind == "upsample":
                hip.upSample(B, l.c, l.h, l.w, prev, l.stride, 1, 1.0, out)
            elif l.kind == "yolo":
                hip.yoloForward(B, l.anchors, l.classes, l.h * l.w, prev, out)
                if self.yolo_loss and truth is not None:
                    if truth.numel() != B * l.max_boxes * 6:
                        raise ValueError(f"truth has {truth.numel()} floats, batch {B} x max "
                                         f"{l.max_boxes} x 6 expected")
                    hip.yoloLoss(B, l.anchors, l.classes, l.h, l.w, l.total, l.mask, l.biases,
                                 l.max_boxes, self.net.w, self.net.h, l.ignore_thresh,
                                 l.truth_thresh, l.iou_thresh, l.iou_normalizer, l.obj_normalizer,
                                 out, truth, self.delta[l.index], self.costs[l.index],
                                 self.yolo_stats[l.index], self.yolo_counters)
            elif l.kind == "maxpool":
                hip.forwardMaxPool(B, l.out_c, l.out_h, l.out_w, prev, l.c, l.h, l.w, l.stride_x,
                                   l.stride_y, l.pad, l.size, self.indexes[l.index], out)
            elif l.kind == "local_avgpool":
                hip.forwardAvgPool(B, l.out_c, l.out_h, l.out_w, prev, l.c, l.h, l.w, l.stride_x,
                                   l.stride_y, l.pad, l.size, out)
            elif l.kind == "connected":
                self._fc_forward(l, prev, out)
            elif l.kind == "lstm":
                hip.fill(out.numel(), self.delta[l.index], 0, 0.0, 1)
                self._lstm_forward(l, prev, True)
            elif l.kind == "rnn":
                self._rnn_forward(l, prev, True)
            elif l.kind == "softmax":
                n, g = B * l.in_size, l.in_size // l.groups
                hip.softmaxBatch(g, prev, 0, B, l.in_size, l.groups, g, 1, l.temperature, out, 0)
                if truth is not None and not l.noloss:
                    hip.crossEntropySoftmax(n, out, truth, self.delta[l.index], self.loss[l.index])
                    hip.sum(n, self.loss[l.index], 0, self.costs[l.index])
            elif l.kind == "cost":
                if truth is not None:
                    n = B * l.in_size
                    hip.costL2(n, prev, truth, self.delta[l.index], out)
                    hip.sum(n, out, 0, self.costs[l.index])
            elif l.kind == "logistic":
                n = B * l.in_size
                hip.copy(n, prev, 0, 1, out, 0, 1)
                hip.ActivateArray(n, out, 0, l.activation)
                if truth is not None:
                    hip.crossEntropyLogistic(n, out, truth, self.delta[l.index],
                                             self.loss[l.index])
                    hip.sum(n, self.loss[l.index], 0, self.costs[l.index])
            prev = out
        return self.out

    def _fc_forward(self, l, prev, out):
        hip, B, st = self.hip, self.net.batch, self.fc[l.index]
        O, I = l.filters, l.in_size
        n = B * O
        hip.gemm(False, True, B, O, I, 1.0, prev, 0, I, st["w"], 0, I, 0.0, out, 0, O)
        if l.bn:
            mom = np.float32(0.05)  # bnMomentum (nconnectedlayer.pas:67), single arithmetic
            keep = float(np.float32(1) - mom)
            hip.means(n, O, B, out, 0, st["mean"])
            hip.variances(n, O, B, out, 0, st["mean"], st["var"])
            hip.scale(O, keep, st["rm"], 1)
            hip.axpy(O, float(mom), st["mean"], 0, 1, st["rm"], 0, 1)
            hip.scale(O, keep, st["rv"], 1)
            hip.axpy(O, float(mom), st["var"], 0, 1, st["rv"], 0, 1)
            hip.copy(n, out, 0, 1, st["x"], 0, 1)
            hip.normalize(O, n, B, st["mean"], 1, st["var"], 1, out, 0)
            hip.copy(n, out, 0, 1, st["xn"], 0, 1)
            hip.forwardScaleAdd(n, out, 0, O, st["scales"], st["b"], 1, B)
        else:
            hip.forwardBias(n, out, 0, O, st["b"], 1, B)
        hip.ActivateArray(n, out, 0, l.activation)

    def _fc_backward(self, l, inp, sd):
        hip, B, st = self.hip, self.net.batch, self.fc[l.index]
        O, I = l.filters, l.in_size
        n, d = B * O, self.delta[l.index]
        hip.clamp(n, 1.0, d, d)
        hip.DeriveArray(n, self.out[l.index], 0, l.activation, d)
        hip.backwardBias(O, st["bu"], n, d, 0, 1, B)
        if l.bn:
            hip.addDots(n, O, B, st["xn"], d, 0, st["su"])
            hip.forwardScale(n, d, 0, O, st["scales"], 1, B)
            hip.meansAndVarsDelta(n, O, B, d, st["x"], 0, st["mean"], st["var"], st["md"],
                                  st["vd"])
            hip.normalizeDelta(n, O, B, d, st["x"], 0, st["mean"], st["var"], st["md"], st["vd"])
        hip.gemm(True, False, O, I, B, 1.0, d, 0, O, inp, 0, I, 1.0, st["wu"], 0, I)
        if sd is not None:
            hip.gemm(False, False, B, I, O, 1.0, d, 0, O, st["w"], 0, I, 1.0, sd, 0, I)

    def cost(self) -> float:
        """TNNet.cost (nnet.pas:551-564): the loss layers' cost[0] summed and
        divided by their count, in single arithmetic."""
        if not self.costs:
            raise ValueError("the network has no loss layer")
        r = np.float32(0)
        for i in sorted(self.costs):
            r = np.float32(r + np.float32(self.costs[i].item()))
        return float(np.float32(r / np.float32(len(self.costs))))

    def update(self, learning_rate, momentum, decay):
        """TNNet.update (nnet.pas:371-403) at a constant learning rate:
        ``sgdUpdate`` (updateGPU's axpy / scale sequence fused) on every
        convolutional and connected layer of layers 0 .. n-2 — the reference's
        loop stops before the last layer — with args.batch = net.batch."""
        for l in self.net.layers[:-1]:
            if l.kind == "lstm":
                self._lstm_update(l, learning_rate, momentum, decay)
                continue
            if l.kind == "rnn":
                self._rnn_update(l, learning_rate, momentum, decay)
                continue
            st = self.conv.get(l.index) or self.fc.get(l.index)
            if st is None:
                continue
            self.hip.sgdUpdate(st["w"], st["wu"], st["b"], st["bu"], learning_rate, self.net.batch,
                               decay, momentum, st.get("scales"), st.get("su"))

    def set_yolo_deltas(self, deltas):
        """The yolo layers' deltas (what their training forward's loss would
        leave), in layer order."""
        ys = [l for l in self.net.layers if l.kind == "yolo"]
        for l, d in zip(ys, deltas):
            self.delta[l.index].copy_(d.reshape(-1))

    def backward(self, x, on_backward=None):
        """TNet.backward (nnet.pas:323-366) over every layer; on_backward(l)
        after each layer's calls (TNet.OnBackward, nnet.pas:361-362)."""
        hip, B, L = self.hip, self.net.batch, self.net.layers
        for l in reversed(L):
            i = l.index
            inp = x if i == 0 else self.out[i - 1]
            sd = None if i == 0 else self.delta[i - 1]
            d = self.delta[i]
            if l.kind == "convolutional":
                st = self.conv[i]
                if l.bn:
                    hip.convBackwardBN(B, l.c, l.h, l.w, inp, st["w"], l.filters, l.size,
                                       l.stride, l.pad, 1, l.activation, self.out[i], d,
                                       st["scales"], st["x"], st["xn"], st["mean"], st["var"],
                                       st["su"], st["md"], st["vd"], st["wu"], self.ws, sd)
                else:
                    hip.convBackward(B, l.c, l.h, l.w, inp, st["w"], l.filters, l.size, l.stride,
                                     l.pad, 1, l.activation, self.out[i], d, st["bu"], st["wu"],
                                     self.ws, sd)
            elif l.kind == "shortcut":
                n = d.numel()
                hip.DeriveArray(n, self.out[i], 0, l.activation, d)
                hip.addvv(n, d, 0, 1, sd, 0, 1, sd, 0, 1)
                src = self.delta[l.inputs[0]]
                hip.addvv(n, src, 0, 1, d, 0, 1, src, 0, 1)
            elif l.kind == "route":
                off = 0
                for s in l.inputs:
                    pt = self.delta[s]
                    hip.addvv(pt.numel(), pt, 0, 1, d, off, 1, pt, 0, 1)
                    off += pt.numel()
            elif l.kind == "upsample":
                hip.upSample(B, l.c, l.h, l.w, sd, l.stride, 0, 1.0, d)
            elif l.kind == "yolo":
                # lossScale*deltaNormalizer, a single product (nyololayer.pas:1119)
                hip.axpy(sd.numel(), float(np.float32(self.loss_scale)
                                           * np.float32(l.delta_normalizer)), d, 0, 1, sd, 0, 1)
            elif l.kind == "maxpool" and sd is not None:
                hip.backwardMaxPool(B, l.out_c, l.out_h, l.out_w, sd, self.indexes[i], d, l.h, l.w,
                                    l.stride_x, l.stride_y, l.pad, l.size)
            elif l.kind == "local_avgpool" and sd is not None:
                hip.backwardAvgPool(B, l.out_c, l.out_h, l.out_w, sd, d, l.h, l.w, l.stride_x,
                                    l.stride_y, l.pad, l.size)
            elif l.kind == "connected":
                self._fc_backward(l, inp.reshape(-1), sd)
            elif l.kind == "lstm":
                self._lstm_backward(l, inp, sd)
            elif l.kind == "rnn":
                self._rnn_backward(l, inp, sd)
            elif l.kind == "dropout" and sd is not None:
                hip.backwardDropout(sd.numel(), sd, l.probability, l.scale, self.rnd[i], sd)
            elif l.kind in ("softmax", "logistic") and sd is not None:
                hip.addvv(d.numel(), d, 0, 1, sd, 0, 1, sd, 0, 1)
            elif l.kind == "cost" and sd is not None:
                hip.axpy(d.numel(), l.scale, d, 0, 1, sd, 0, 1)
            if on_backward is not None:
                on_backward(l)
