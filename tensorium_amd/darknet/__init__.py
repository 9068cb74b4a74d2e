"""Darknet networks on the HIP backend.

* ``description`` (NumPy only): .cfg parsing, the layer plan with shapes,
  the sample cfg builders, .weights I/O and batch-norm folding — the part of
  TDarknetParser / TNNet (nparser.pas, nnet.pas) a network needs before it
  runs.
* ``connected``: TConnectedLayer's forward / backward / update
  (nconnectedlayer.pas), the one statement of it for the [connected] layer
  and the lstm and rnn sub-layers.
* ``recurrent``: the lstm and rnn layers' step logic (nlstmlayer.pas,
  nrnnlayer.pas).
* ``drivers``: ``HipDarknet`` (inference) and ``HipDarknetTrain`` (a training
  pass), with the image and detection helpers.

Every public name is importable from this package.
"""
from .._abi import ACT, TnsError
from .description import (ACT_SUPPORTED, LSTM_GATES, RNN_SUBS, SEPS, ConvParams, Layer, Network,
                          Section, cifar10_deep_cfg, darknet19_cfg, darknet53_cfg,
                          fuse_batchnorm, lenet_cifar10_cfg,
                          lenet_mnist_cfg, load_weights, lstm_cfg, parse_cfg, random_params,
                          rnn_cfg, write_weights, yolov3_cfg, yolov3_tiny_cfg)
from .drivers import (HipDarknet, HipDarknetTrain, Placement, detection_rows_to_host,
                      images_to_input, letterbox_truth)
