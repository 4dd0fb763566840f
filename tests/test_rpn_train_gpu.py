"""The train-mode RPN neck on the device (RPN._forward_train, fused_train = True): convs on ops.Conv2dFunction, the k = s transposed
up-samplers on ops.DeconvKsFunction, BatchNorm2d + ReLU on ops.bn2d_relu_train, against a float64 copy of the same modules composed
by hand on the CPU (test_rpn_train_cpu.compose).

Rule (tests/test_pillar_train_gpu.py): for the output, the input gradient, every parameter gradient and every running statistic,
e_device = max|t - t64| must stay within max(4 e_torch32, 64 * 2^-24 * max|t64|), e_torch32 being the error of the same modules
in float32 on the CPU against float64.

Small config (test_rpn_train_cpu.ARGS, 64 x 32 x 32 input, batch 2): the maps are 16 x 16, 8 x 8 and 4 x 4, so block 2's convs
(wout = 4) are refused by ops.conv2d_train_covers and run their torch modules next to covered layers; the three up-samplers
(s = 1, 2, 4) are all covered. Three-class neck in small: one block of 1 + 2 layers, stride 1, 128 filters, up-sampler s = 1,
16 x 16: everything on the device path."""
import copy

import pytest
import torch
from torch import nn

from det3d.models.necks.rpn_v1 import RPN
from sessd_hip import ops
from test_rpn_train_cpu import ARGS, compose, make_neck

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ARGS_3CLASS = dict(layer_nums=[2], ds_layer_strides=[1], ds_num_filters=[128], us_layer_strides=[1], us_num_filters=[128],
                   num_input_features=128, norm_cfg=None)


def graph_nodes(t):
    """names of the autograd nodes behind t"""
    seen, todo, names = set(), [t.grad_fn], []
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.append(type(f).__name__)
        todo.extend(n for n, _ in f.next_functions)
    return names


def layer_inputs(neck, x):
    """[(module, its input, behind a ZeroPad2d(1))] of every conv layer, from a run of the torch modules"""
    rec, hooks = {}, []
    convs = [m for m in neck.modules() if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d))]
    pads = [m for m in neck.modules() if isinstance(m, nn.ZeroPad2d)]
    for m in convs + pads:
        hooks.append(m.register_forward_hook(lambda mod, inp, out: rec.__setitem__(mod, inp[0])))
    was = neck.fused_train
    neck.fused_train = False
    with torch.no_grad():
        neck(x)
    neck.fused_train = was
    for h in hooks:
        h.remove()
    # the running statistics moved: the caller works on a copy
    out = []
    for seq in list(neck.blocks) + list(neck.deblocks):
        mods = list(seq._modules.values())
        for i, m in enumerate(mods):
            if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
                padded = i > 0 and isinstance(mods[i - 1], nn.ZeroPad2d)
                out.append((m, rec[mods[i - 1]] if padded else rec[m], padded))
    return out


def run(neck, x, gout):
    """forward + backward: (output, input gradient, parameter gradients, running statistics)"""
    x = x.clone().requires_grad_(True)
    for p in neck.parameters():
        p.grad = None
    assert isinstance(neck, RPN) and neck.training
    out = neck(x)
    out.backward(gout)
    got = {"out": out.detach(), "gx": x.grad}
    got.update({"grad " + k: p.grad for k, p in neck.named_parameters()})
    got.update({k: v.clone() for k, v in neck.state_dict().items() if "running_" in k})
    return got, out


def run_composed(neck, x, gout):
    x = x.clone().requires_grad_(True)
    out = compose(neck, x)
    out.backward(gout)
    got = {"out": out.detach(), "gx": x.grad}
    got.update({"grad " + k: p.grad for k, p in neck.named_parameters()})
    got.update({k: v.clone() for k, v in neck.state_dict().items() if "running_" in k})
    return got


def hold(tag, got, ref32, ref64):
    worst = 0.0
    assert set(got) == set(ref32) == set(ref64)
    for k, t64 in ref64.items():
        assert got[k] is not None, k
        e_dev = float((got[k].detach().cpu().double() - t64).abs().max())
        e_t32 = float((ref32[k].double() - t64).abs().max())
        allowed = max(4 * e_t32, 64 * U * float(t64.abs().max()))
        assert allowed > 0, k
        print("%s %-40s e_device %.2e  e_torch32 %.2e  e_device / allowed %.3f" % (tag, k, e_dev, e_t32, e_dev / allowed))
        assert e_dev <= allowed, (tag, k, e_dev, e_t32)
        worst = max(worst, e_dev / allowed)
    print("%s: worst e_device / allowed = %.3f" % (tag, worst))
    return worst


def case(args, seed, shape, out_shape):
    master = make_neck(seed, args).train()
    g = torch.Generator().manual_seed(seed + 100)
    x = torch.randn(*shape, generator=g)
    gout = torch.randn(*out_shape, generator=g)
    ref64 = run_composed(copy.deepcopy(master).double(), x.double(), gout.double())
    ref32 = run_composed(copy.deepcopy(master), x, gout)
    return master, x, gout, ref32, ref64


def test_small_config_against_float64(dev):
    master, x, gout, ref32, ref64 = case(ARGS, 0, (2, 64, 32, 32), (2, 96, 16, 16))
    neck = copy.deepcopy(master).to(dev)
    assert neck.fused_train is True and neck.training
    xd, gd = x.to(dev), gout.to(dev)
    # what the predicates say about every conv layer at these sizes: covered and refused layers side by side
    layers = layer_inputs(copy.deepcopy(neck), xd)
    convs = [(m, ops.conv2d_train_covers(m, inp, padded=padded)) for m, inp, padded in layers if not isinstance(m, nn.ConvTranspose2d)]
    ups = [(m, ops.deconv_ks_covers(m, inp)) for m, inp, _ in layers if isinstance(m, nn.ConvTranspose2d)]
    assert len(convs) == 6 and len(ups) == 3
    assert [c for _, c in convs] == [True, True, True, True, False, False]     # block 2: wout = 4
    assert all(c for _, c in ups) and sorted(m.stride[0] for m, _ in ups) == [1, 2, 4]
    got, out = run(neck, xd, gd)
    names = graph_nodes(out)
    assert names.count("Conv2dFunctionBackward") == 4 and names.count("DeconvKsFunctionBackward") == 3
    assert names.count("ConvolutionBackward0") == 2                            # the two refused convs ran their torch modules
    assert names.count("Bn2dReluTrainFunctionBackward") == 9 and "NativeBatchNormBackward0" not in names
    hold("small config", got, ref32, ref64)
    for k, v in neck.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1, k
    # .eval() afterwards: the eval lowering again, no graph, equal to a fresh eval-mode copy of the same state
    fresh = make_neck(0, ARGS)
    fresh.load_state_dict(neck.state_dict())
    a, b = neck.eval()(xd), fresh.to(dev).eval()(xd)
    assert a.grad_fn is None and torch.equal(a, b)


def test_three_class_neck_runs_entirely_on_the_device_path(dev):
    master, x, gout, ref32, ref64 = case(ARGS_3CLASS, 1, (2, 128, 16, 16), (2, 128, 16, 16))
    neck = copy.deepcopy(master).to(dev)
    xd, gd = x.to(dev), gout.to(dev)
    for m, inp, padded in layer_inputs(copy.deepcopy(neck), xd):
        assert ops.deconv_ks_covers(m, inp) if isinstance(m, nn.ConvTranspose2d) else ops.conv2d_train_covers(m, inp, padded=padded)
    got, out = run(neck, xd, gd)
    names = graph_nodes(out)
    assert names.count("Conv2dFunctionBackward") == 3 and names.count("DeconvKsFunctionBackward") == 1
    assert names.count("Bn2dReluTrainFunctionBackward") == 4
    assert not any(n.startswith(("ConvolutionBackward", "NativeBatchNormBackward", "ReluBackward")) for n in names)
    hold("three-class neck", got, ref32, ref64)


@pytest.fixture()
def deterministic_torch_convs():
    """torch's own convolution backward may pick a solver that adds with atomics: two runs of the SAME modules then differ in the
    last bits of a weight gradient. Bit-for-bit comparisons of two torch runs ask torch for its deterministic solvers."""
    was = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = was


def test_fused_train_off_is_the_torch_composition_on_the_device(dev, deterministic_torch_convs):
    master = make_neck(2, ARGS).train()
    neck, twin = copy.deepcopy(master).to(dev), copy.deepcopy(master).to(dev)
    neck.fused_train = False
    g = torch.Generator().manual_seed(5)
    xd, gd = torch.randn(2, 64, 32, 32, generator=g).to(dev), torch.randn(2, 96, 16, 16, generator=g).to(dev)
    got, out = run(neck, xd, gd)
    want = run_composed(twin, xd, gd)
    assert not any(n.endswith("FunctionBackward") for n in graph_nodes(out))
    for k in want:
        assert torch.equal(got[k], want[k]), k
