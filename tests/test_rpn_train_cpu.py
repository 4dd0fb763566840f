"""A train-mode RPN neck on CPU tensors: every layer runs its torch module, so the output equals the hand-composed torch modules
bit for bit, carries a graph, moves the running statistics and leaves module tree and state_dict keys alone. Before the train
branch existed a train-mode RPN ran the eval lowering: on CPU tensors it raised, on the device it returned a map without grad_fn.

Config: layer_nums [1, 1, 1], strides [2, 2, 2], filters [32, 32, 64], up-samplers [1, 2, 4] -> 32 each, 64 input features, a
32 x 32 map, batch 2."""
import copy

import pytest
import torch
from torch import nn

from det3d.models.necks.rpn_v1 import RPN

ARGS = dict(layer_nums=[1, 1, 1], ds_layer_strides=[2, 2, 2], ds_num_filters=[32, 32, 64], us_layer_strides=[1, 2, 4],
            us_num_filters=[32, 32, 32], num_input_features=64, norm_cfg=None)


def make_neck(seed=0, args=ARGS):
    torch.manual_seed(seed)
    neck = RPN(**args)
    with torch.no_grad():
        for m in neck.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    return neck


def compose(neck, x):
    """rpn_v1.py:107-116 with the neck's own torch modules, one after the other"""
    ups = []
    start = len(neck.blocks) - len(neck.deblocks)
    for i, block in enumerate(neck.blocks):
        for m in block._modules.values():
            x = m(x)
        if i - start >= 0:
            u = x
            for m in neck.deblocks[i - start]._modules.values():
                u = m(u)
            ups.append(u)
    return torch.cat(ups, dim=1)


def test_train_mode_on_cpu_tensors_is_the_torch_composition():
    assert RPN.fused_train is True
    neck = make_neck().train()
    twin = copy.deepcopy(neck)
    eval_keys = list(make_neck().eval().state_dict().keys())
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 64, 32, 32, generator=g)
    gout = torch.randn(2, 96, 16, 16, generator=g)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    before = {k: v.clone() for k, v in neck.state_dict().items()}

    out = neck(xa)
    ref = compose(twin, xb)
    assert out.shape == (2, 96, 16, 16) and out.grad_fn is not None
    assert torch.equal(out, ref)
    out.backward(gout)
    ref.backward(gout)
    assert xa.grad is not None and torch.equal(xa.grad, xb.grad) and float(xa.grad.abs().max()) > 0
    for (k, p), (_, q) in zip(neck.named_parameters(), twin.named_parameters()):
        assert p.grad is not None and torch.equal(p.grad, q.grad), k
        assert float(p.grad.abs().max()) > 0, k
    # the running statistics moved, the batches were counted -- the same way as the modules do it
    after = neck.state_dict()
    assert list(after.keys()) == eval_keys == list(twin.state_dict().keys())
    for k, v in after.items():
        assert torch.equal(v, twin.state_dict()[k]), k
        if k.endswith("running_mean") or k.endswith("running_var"):
            assert not torch.equal(v, before[k]), k
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(before[k]) + 1, k
    assert [n for n, _ in neck.named_modules()] == [n for n, _ in make_neck().named_modules()]


def test_fused_train_off_and_eval_afterwards():
    neck = make_neck(2).train()
    neck.fused_train = False
    x = torch.randn(2, 64, 32, 32, generator=torch.Generator().manual_seed(3))
    twin = copy.deepcopy(neck)
    assert torch.equal(neck(x), compose(twin, x))
    # .eval() afterwards takes the eval path again: the HIP lowering, which has no CPU fallback
    neck.eval()
    with pytest.raises(ValueError, match="CUDA"):
        neck(x)


def test_a_stride_below_one_up_sampler_runs_its_torch_module():
    args = dict(ARGS, layer_nums=[1, 1], ds_layer_strides=[1, 2], ds_num_filters=[32, 32], us_layer_strides=[0.5, 1], us_num_filters=[32, 32])
    neck = make_neck(4, args).train()
    assert isinstance(neck.deblocks[0][0], nn.Conv2d) and not isinstance(neck.deblocks[0][0], nn.ConvTranspose2d)
    x = torch.randn(1, 64, 16, 16, generator=torch.Generator().manual_seed(5)).requires_grad_(True)
    twin = copy.deepcopy(neck)
    out = neck(x)
    assert out.shape == (1, 64, 8, 8) and out.grad_fn is not None and torch.equal(out, compose(twin, x))
