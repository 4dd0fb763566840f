"""RPN.train_any_width: a PointPillars-shaped neck in small whose maps are 24 x 20, 12 x 10 and 6 x 5 -- widths 20 (% 4 == 0), 10
(even) and 5 (odd), none a multiple of 8 -- so that by default ops.conv2d_train_covers refuses all six convs and with the switch
on covers them all: the three stride-2 convs (64 -> 64, 64 -> 128, 128 -> 256) take the LDS-staged weight-gradient kernel, the
three stride-1 convs the general one, each in its ragged-row class (sessd_conv2d_wgrad_any_width).

The rule is the one of tests/test_rpn_train_gpu.py (its case / run / hold): against a float64 copy of the same modules on the CPU,
e_device <= max(4 e_torch32, 64 * 2^-24 * max|t64|) for the output, the input gradient, every parameter gradient and every running
statistic. The BatchNorm node count is not pinned: the 6 x 5 plane is no multiple of 4, ops.bn2d_relu_train falls back there."""
import copy

import pytest
from torch import nn

import dense_grad_ref as R
from det3d.models.necks.rpn_v1 import RPN
from sessd_hip import ops
from test_rpn_train_gpu import case, graph_nodes, hold, layer_inputs, run

pytestmark = pytest.mark.gpu

ARGS = dict(layer_nums=[1, 1, 1], ds_layer_strides=[2, 2, 2], ds_num_filters=[64, 128, 256], us_layer_strides=[1, 2, 4],
            us_num_filters=[128, 128, 128], num_input_features=64, norm_cfg=None)


@pytest.fixture(scope="module")
def shared():
    """the master neck, its input and output gradient, the float32 and float64 CPU references: computed once, left unchanged"""
    return case(ARGS, 3, (2, 64, 48, 40), (2, 384, 24, 20))


def _convs(neck, xd, any_width):
    layers = layer_inputs(copy.deepcopy(neck), xd)
    convs = [(m, inp, ops.conv2d_train_covers(m, inp, padded=padded, any_width=any_width)) for m, inp, padded in layers
             if not isinstance(m, nn.ConvTranspose2d)]
    ups = [ops.deconv_ks_covers(m, inp) for m, inp, _ in layers if isinstance(m, nn.ConvTranspose2d)]
    assert len(convs) == 6 and ups == [True, True, True]
    return convs


def test_default_refuses_every_conv(dev, shared):
    master, x, gout, ref32, ref64 = shared
    neck = copy.deepcopy(master).to(dev)
    assert neck.train_any_width is False and RPN.train_any_width is False and neck.fused_train is True
    xd, gd = x.to(dev), gout.to(dev)
    assert [c for _, _, c in _convs(neck, xd, False)] == [False] * 6
    got, out = run(neck, xd, gd)
    names = graph_nodes(out)
    assert names.count("ConvolutionBackward0") == 6 and names.count("DeconvKsFunctionBackward") == 3
    assert not any(n.startswith("Conv2dFunction") for n in names)
    hold("PointPillars-shaped neck, default", got, ref32, ref64)


def test_any_width_runs_every_conv_on_the_device_path(dev, shared):
    master, x, gout, ref32, ref64 = shared
    neck = copy.deepcopy(master).to(dev)
    neck.train_any_width = True
    xd, gd = x.to(dev), gout.to(dev)
    convs = _convs(neck, xd, True)
    assert [c for _, _, c in convs] == [True] * 6
    # the widths and the weight-gradient kernels the six layers take
    seen = []
    for m, inp, _ in convs:
        B, ci, H, W = inp.shape
        s = m.stride[0]
        seen.append((W // s, R.direct_chunks(B, ci, m.out_channels, H // s, 3, s)[0]))
    assert seen == [(20, "s2_lds"), (20, "general"), (10, "s2_lds"), (10, "general"), (5, "s2_lds"), (5, "general")]
    got, out = run(neck, xd, gd)
    names = graph_nodes(out)
    assert sum(n.startswith("Conv2dFunction") for n in names) == 6 and names.count("Conv2dFunctionAnyWidthBackward") == 6
    assert names.count("DeconvKsFunctionBackward") == 3
    assert not any(n.startswith("ConvolutionBackward") for n in names)
    hold("PointPillars-shaped neck, train_any_width", got, ref32, ref64)
