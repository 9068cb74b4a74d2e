"""The darknet drivers on the HIP backend: ``HipDarknet`` (TNNet.forward,
inference) and ``HipDarknetTrain`` (one training pass: TNet.forward in
training, TNet.backward, TNNet.update; nnet.pas:275-403), both over
``_Driver``, which holds what does not depend on the mode; and the image and
detection helpers around them (ntypes.pas:837-947, nnet.pas:584-677,
MSCOCOYolo.pas:348-358, 432-484).  Connected layers and sub-layers:
``connected.py``; lstm and rnn layers: ``recurrent.py``.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .._abi import TnsError
from . import connected as fc
from .description import ConvParams, Network, fuse_batchnorm
from .recurrent import _LstmLayers, _RnnLayers


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
            [np.ascontiguousarray(im).reshape(-1) for im in images])).to(dst.device)
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


class _Driver(_RnnLayers, _LstmLayers):
    """What HipDarknet and HipDarknetTrain share: the buffers and parameter
    states a constructor builds, the lazily allocated net input, and the
    layer forwards that do not depend on the mode."""

    device = "cuda"  # where every buffer is allocated and every parameter uploaded

    def _t(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)

    def _z(self, n, dtype=None):
        return self.torch.zeros(n, dtype=dtype, device=self.device)

    def _build(self, hip, net, params, torch, lstm_fused, rnn_fused, training):
        """Every layer's output (zeros in training, uninitialised in
        inference) and, in training, delta; the lstm, rnn and connected
        layers' states.  Returns the convolutional blocks [(layer, params)],
        which each driver keeps in its own form."""
        self.hip, self.net, self.torch = hip, net, torch
        self.lstm_fused = bool(lstm_fused)
        self.rnn_fused = bool(rnn_fused)
        B = net.batch
        new = self._z if training else lambda n: torch.empty(n, device=self.device)
        self.out = []
        if training:
            self.delta = []
        for l in net.layers:
            # a dropout's output and delta are the layer below's (at layer 0
            # the output is the input: forward sets it)
            alias = l.kind == "dropout" and l.index > 0
            self.out.append(self.out[-1] if alias else new(B * l.out_size))
            if training:
                self.delta.append(self.delta[-1] if alias else new(B * l.out_size))
        blocks = list(zip(net.param_layers(), params))
        subs = {(l.index, l.gate): (l, p) for l, p in blocks if l.gate}
        self._lstm_init(subs, training)
        self._rnn_init(subs, training)
        self.fc, convs = {}, []
        for l, p in blocks:
            if l.gate:
                continue
            if l.kind == "connected":
                self.fc[l.index] = fc.state(self._t, self._z, p, l.filters, l.in_size,
                                            l.activation, l.bn, B, training,
                                            out=self.out[l.index],
                                            delta=self.delta[l.index] if training else None)
            else:
                convs.append((l, p))
        return convs

    def _net_input(self):
        """The [batch, c, h, w] input buffer ``load_images`` / ``load_batch``
        fill, allocated at the first call."""
        net = self.net
        if getattr(self, "_input", None) is None:
            self._input = self.torch.empty((net.batch, net.c, net.h, net.w), device=self.device)
        return self._input

    def _forward_layer(self, l, prev, out):
        """The forwards that are the same calls in inference and in training
        (a [cost] layer's inference forward is nothing)."""
        hip, B = self.hip, self.net.batch
        if l.kind == "shortcut":
            hip.shortcut(B * l.out_size, prev, 0, self.out[l.inputs[0]], 0, out, 0, l.activation)
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
        elif l.kind == "local_avgpool":
            hip.forwardAvgPool(B, l.out_c, l.out_h, l.out_w, prev, l.c, l.h, l.w, l.stride_x,
                               l.stride_y, l.pad, l.size, out)
        elif l.kind == "avgpool":
            hip.forwardGlobalAvgPool(B, l.c, l.h, l.w, prev, out)
        elif l.kind == "softmax":
            g = l.in_size // l.groups
            hip.softmaxBatch(g, prev, 0, B, l.in_size, l.groups, g, 1, l.temperature, out, 0)
        elif l.kind == "logistic":
            hip.copy(B * l.in_size, prev, 0, 1, out, 0, 1)
            hip.ActivateArray(B * l.in_size, out, 0, l.activation)


class HipDarknet(_Driver):
    """TNNet.forward over a darknet layer plan on the HIP backend (nnet.pas:
    275-310 selects forwardGPU per layer): every layer's output stays in a
    device buffer of its own; convolutions take BN-folded parameters
    (fuseBatchNorm) and run the fused implicit-GEMM driver.  Connected layers
    run TConnectedLayer.forwardGPU's inference branch (``connected.forward``:
    NT gemm, normalize by the rolling statistics + forwardScaleAdd, or
    forwardBias, then ActivateArray).  A dropout layer's output is its
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
        self.conv_params = {}
        for l, p in self._build(hip, net, params, torch, lstm_fused, rnn_fused, training=False):
            f = fuse_batchnorm(l, p)
            self.conv_params[l.index] = (self._t(f.weights), self._t(f.biases))

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
            elif l.kind == "maxpool":  # inference: no indexes
                hip.forwardMaxPool(B, l.out_c, l.out_h, l.out_w, prev, l.c, l.h, l.w, l.stride_x,
                                   l.stride_y, l.pad, l.size, None, out)
            elif l.kind == "connected":
                fc.forward(hip, self.fc[l.index], B, 0, prev, 0, False)
            elif l.kind == "lstm":
                self._lstm_forward(l, prev, False)
            elif l.kind == "rnn":
                self._rnn_forward(l, prev, False)
            elif l.kind == "dropout":
                out = self.out[l.index] = prev.reshape(-1)
            else:
                self._forward_layer(l, prev, out)
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
        yolos = self.net.yolos()
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
            dev = self.device
            self._det = (torch.zeros(B, dtype=torch.int64, device=dev),
                         torch.empty(B * cap * 4, device=dev), torch.empty(B * cap, device=dev),
                         torch.empty(B * cap * max(classes, 1), device=dev))
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
        x = self._net_input()
        placed = images_to_input(self.hip, self.torch, images, net.c, net.w, net.h, x,
                                 letter=letter, table=table)
        return x, placed

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


class HipDarknetTrain(_Driver):
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
    * avgpool (TAvgPoolLayer.forward / backward, navgpoollayer.pas:60-108,
      which the reference runs on the CPU): ``forwardGlobalAvgPool``;
      ``backwardGlobalAvgPool`` accumulating delta / (h*w) into state.delta,
      nothing when it is layer 0;
    * connected (TConnectedLayer.forwardGPU / backwardGPU, nconnectedlayer.pas:
      612-871): ``connected.forward`` / ``connected.backward`` over one step
      of ``batch`` rows;
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
        self.loss_scale = float(loss_scale)
        self.yolo_loss = bool(yolo_loss)
        yolos = net.yolos()
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
        convs = self._build(hip, net, params, torch, lstm_fused, rnn_fused, training=True)
        B, z, t = net.batch, self._z, self._t
        self.rnd = {l.index: z(B * l.out_size) for l in net.layers if l.kind == "dropout"}
        # softmax / logistic: loss[batch*inputs]; every loss layer: cost[1]
        self.loss = {l.index: z(B * l.out_size)
                     for l in net.layers if l.kind in ("softmax", "logistic")}
        self.costs = {l.index: z(1) for l in net.layers if l.kind in self.LOSS_KINDS}
        # the device yolo loss: cost[1] and the per-image {count, tot_iou} of
        # every yolo layer, and the network's {totalBBox, rewrittenBBox}
        self.yolo_stats = {}
        if self.yolo_loss:
            for l in yolos:
                self.costs[l.index] = z(1)
                self.yolo_stats[l.index] = z(2 * B)
            self.yolo_counters = z(2, torch.int64)
        # a maxpool's indexes (TSizeIntTensor, int64): filled by its forward
        self.indexes = {l.index: z(B * l.out_size, torch.int64)
                        for l in net.layers if l.kind == "maxpool"}
        self.conv = {}
        ws = 1
        for l, p in convs:
            n, F = B * l.out_size, l.filters
            st = {"w": t(p.weights), "b": t(p.biases), "wu": z(p.weights.size), "bu": z(F)}
            if l.bn:
                st.update(scales=t(p.scales), rm=t(p.rolling_mean), rv=t(p.rolling_var),
                          mean=z(F), var=z(F), x=z(n), xn=z(n), su=z(F), md=z(F), vd=z(F))
            self.conv[l.index] = st
            ws = max(ws, B * l.c * l.size * l.size * l.out_h * l.out_w)
        self.ws = torch.empty(ws, device=self.device)

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
        yolos = net.yolos()
        if not yolos:
            raise ValueError("load_batch: the network has no [yolo] layer")
        if len(images) != net.batch or len(boxes) != net.batch:
            raise ValueError(f"{len(images)} images and {len(boxes)} box lists for a batch of "
                             f"{net.batch}")
        x = self._net_input()
        placed = images_to_input(self.hip, torch, images, net.c, net.w, net.h, x, letter=True,
                                 table=table)
        rows = letterbox_truth(boxes, placed, net.w, net.h, yolos[0].max_boxes)
        return x, torch.from_numpy(rows.reshape(net.batch, -1)).to(self.device)

    def forward(self, x, truth=None, seeds=None):
        """TNet.forward with state.isTraining (BN statistics of the batch,
        rolling statistics updated with bnMomentum 0.1, connected layers
        0.05).  truth: device tensor of the loss layers' size (state.truth),
        or None (no loss is computed); with ``yolo_loss`` the truth boxes
        [batch, max_boxes*6], the same tensor for every yolo layer.  seeds:
        one integer in [0, 2^32) per dropout layer, in layer order; by default
        drawn in [0, 2^28), the reference's random($10000000), from the
        generator seeded at construction."""
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
            elif l.kind == "maxpool":
                hip.forwardMaxPool(B, l.out_c, l.out_h, l.out_w, prev, l.c, l.h, l.w, l.stride_x,
                                   l.stride_y, l.pad, l.size, self.indexes[l.index], out)
            elif l.kind == "connected":
                fc.forward(hip, self.fc[l.index], B, 0, prev, 0, True)
            elif l.kind == "lstm":
                hip.fill(out.numel(), self.delta[l.index], 0, 0.0, 1)
                self._lstm_forward(l, prev, True)
            elif l.kind == "rnn":
                self._rnn_forward(l, prev, True)
            elif l.kind == "cost":
                if truth is not None:
                    n = B * l.in_size
                    hip.costL2(n, prev, truth, self.delta[l.index], out)
                    hip.sum(n, out, 0, self.costs[l.index])
            else:
                self._forward_layer(l, prev, out)
                if truth is not None:
                    self._loss(l, out, truth)
            prev = out
        return self.out

    def _loss(self, l, out, truth):
        """What a yolo, softmax or logistic layer's training forward adds
        when there is truth: its delta and its cost."""
        hip, B, n = self.hip, self.net.batch, self.net.batch * l.in_size
        if l.kind == "yolo" and self.yolo_loss:
            if truth.numel() != B * l.max_boxes * 6:
                raise ValueError(f"truth has {truth.numel()} floats, batch {B} x max "
                                 f"{l.max_boxes} x 6 expected")
            hip.yoloLoss(B, l.anchors, l.classes, l.h, l.w, l.total, l.mask, l.biases,
                         l.max_boxes, self.net.w, self.net.h, l.ignore_thresh, l.truth_thresh,
                         l.iou_thresh, l.iou_normalizer, l.obj_normalizer, out, truth,
                         self.delta[l.index], self.costs[l.index], self.yolo_stats[l.index],
                         self.yolo_counters)
        elif l.kind == "softmax" and not l.noloss:
            hip.crossEntropySoftmax(n, out, truth, self.delta[l.index], self.loss[l.index])
            hip.sum(n, self.loss[l.index], 0, self.costs[l.index])
        elif l.kind == "logistic":
            hip.crossEntropyLogistic(n, out, truth, self.delta[l.index], self.loss[l.index])
            hip.sum(n, self.loss[l.index], 0, self.costs[l.index])

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
            if st is not None:
                fc.update(self.hip, st, self.net.batch, learning_rate, momentum, decay)

    def export_params(self) -> list[ConvParams]:
        """The trained parameters read back from the device state, one
        ConvParams per block in ``Network.param_layers()`` order
        (convolutional and connected layers, an lstm layer's eight and an rnn
        layer's three sub-layers): weights and biases, and scales and the
        rolling mean and variance when batch-normalised — what saveWeights
        stores (nparser.pas:1227-1273).  ``write_weights(path, net,
        train.export_params())`` writes the file ``load_weights`` and
        ``HipDarknet`` run as the trained network."""
        self.hip.finish()
        ps = []
        for l in self.net.param_layers():
            if l.gate:
                owner = self.lstm if self.net.layers[l.index].kind == "lstm" else self.rnn
                st = owner[l.index]["sub"][l.gate]
            else:
                st = self.conv[l.index] if l.kind == "convolutional" else self.fc[l.index]
            host = lambda k: st[k].detach().cpu().numpy().astype(np.float32, copy=True)  # noqa: E731
            w = host("w").reshape(l.filters, -1)
            bn = [host(k) for k in ("scales", "rm", "rv")] if l.bn else []
            ps.append(ConvParams(host("b"), w, *bn))
        return ps

    def set_yolo_deltas(self, deltas):
        """The yolo layers' deltas (what their training forward's loss would
        leave), in layer order."""
        for l, d in zip(self.net.yolos(), deltas):
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
            elif l.kind == "avgpool" and sd is not None:
                hip.backwardGlobalAvgPool(B, l.c, l.h, l.w, d, sd)
            elif l.kind == "connected":
                fc.backward(hip, self.fc[i], B, 0, inp.reshape(-1), 0, sd, 0)
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
