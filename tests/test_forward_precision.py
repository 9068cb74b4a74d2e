"""HipDarknetTrain's forward_precision keyword is checked before anything is built."""
import pytest

from _conv_bf16_ref import BRANCH_CFG
from tensorium_amd import darknet as dn


@pytest.mark.parametrize("value", ["int8", "BF16", None])
def test_unknown_forward_precision(value):
    net = dn.Network(dn.parse_cfg(BRANCH_CFG))
    with pytest.raises(ValueError, match="forward_precision"):
        dn.HipDarknetTrain(None, net, dn.random_params(net, seed=1), None,
                           forward_precision=value)
