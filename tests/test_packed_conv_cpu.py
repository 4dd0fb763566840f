"""ops.PackedConv without a device: pack_conv2d packs nothing until a launch asks, so the geometry rule (out_hw / tile_hw), the
3x3 stride-1 property, the eligibility tests in front of every lazily made packing and the re-pack registry's hook can be held
on CPU tensors."""
import pytest
import torch
import torch.nn.functional as F

from sessd_hip import ops

SIZES = [(7, 9), (8, 10)]


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("k,stride", [(1, 1), (3, 1), (3, 2)])
def test_conv_geometry_is_torchs(k, stride, H, W):
    pc = ops.pack_conv2d(torch.randn(2, 2, k, k), stride)
    ref = F.conv2d(torch.zeros(1, 2, H, W), torch.zeros(2, 2, k, k), stride=stride, padding=k // 2)
    assert pc.out_hw(H, W) == tuple(ref.shape[2:])
    assert pc.tile_hw(H, W) == pc.out_hw(H, W)
    assert pc.is_3x3_s1 == ((k, stride) == (3, 1))
    assert (pc.kind, pc.stride, pc.cin, pc.cout, len(pc.launches)) == ("conv", stride, 2, 2, 1)


@pytest.mark.parametrize("H,W", SIZES)
def test_transposed_geometry_is_torchs(H, W):
    x = torch.zeros(1, 2, H, W)
    pc = ops.PackedConv([], 2, 2, "deconv", 2)   # (the packers of the transposed convs need a device)
    assert pc.out_hw(H, W) == tuple(F.conv_transpose2d(x, torch.zeros(2, 2, 3, 3), None, 2, 1, 1).shape[2:])
    assert pc.tile_hw(H, W) == (H, W) and not pc.is_3x3_s1
    for s in (2, 4):
        pc = ops.PackedConv([], 2, 2, "deconv_ks", s)
        assert pc.out_hw(H, W) == tuple(F.conv_transpose2d(x, torch.zeros(2, 2, s, s), None, s).shape[2:])
        assert pc.tile_hw(H, W) == (H, W) and not pc.is_3x3_s1


def test_ineligible_layer_packs_nothing():
    """cin 6 fails cin % 8 / % 16 in front of every packing: all None, and the library was not asked for anything (a pack entry
    would have refused the CPU tensor)."""
    pc = ops.pack_conv2d(torch.randn(32, 6, 3, 3))
    assert pc.is_3x3_s1
    assert pc.upk is None
    assert [pc.upk_sk(shape) for shape in range(4)] == [None] * 4
    assert pc.sk_args() is None
    assert pc.wsplit() is None
    assert all(la._wpk is None for la in pc.launches)
    la = pc.launches[0]
    assert (la.ntaps, la.in_mul, la.out_mul, la.py, la.px) == (9, 1, 1, 0, 0)
    assert la.dy.tolist() == [-1, -1, -1, 0, 0, 0, 1, 1, 1] and la.dx.tolist() == [-1, 0, 1] * 3
    assert not hasattr(la, "__dict__")   # a record of fixed fields, not a bag


def test_registry_marks_the_owner_only():
    w = torch.nn.Parameter(torch.randn(32, 6, 3, 3))
    reg = ops.RepackRegistry()
    reg.gen = ops.param_generation()   # nothing to refresh: the registry holds no jobs
    pc = reg.cached(("dense", 0), w, lambda: ops.pack_conv2d(w))
    assert isinstance(pc, ops.PackedConv) and pc._registry is reg
    assert reg.cached(("dense", 0), w, lambda: None) is pc
    la = pc.launches[0]
    assert la._owner is pc and la._wpk is None and not hasattr(la, "_registry")
    assert reg.jobs == {"dense": [], "sparse": []}
