"""The three-way bf16 split of stream-K Winograd shape 3 (csrc/dense_conv.hip layout 4, csrc/dense_wino_sk.hip SPLIT): a float32
value is the exact sum of three bfloat16 terms, each rounded to nearest from the residual of the previous one, and the three
products the kernel drops are at the size of float32 rounding."""
import numpy as np
import torch


def _bf16_rne(x):
    """float32 -> bfloat16 round to nearest even, as the packer does it (bits of the upper half, as float32)"""
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def _split3(a):
    a0 = _bf16_rne(a)
    r = (a - a0).astype(np.float32)
    a1 = _bf16_rne(r)
    a2 = _bf16_rne((r - a1).astype(np.float32))
    return a0, a1, a2


def _samples():
    rng = np.random.default_rng(0)
    # magnitudes down to 2^-90: below ~2^-102 the third term would be subnormal (no weight of a trained layer is near there)
    mags = np.exp2(rng.uniform(-90, 100, 200000)).astype(np.float32)
    a = (rng.standard_normal(200000).astype(np.float32) * mags).astype(np.float32)
    edge = np.array([0.0, -0.0, 1.0, -1.0, 3.0, 1.0 / 3.0, np.float32(np.pi), 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, 65504.0,
                     np.finfo(np.float32).tiny, 3.0e38, -3.0e38], dtype=np.float32)
    return np.concatenate([a, edge, rng.standard_normal(100000).astype(np.float32) * 0.05])


def test_split_reconstructs_exactly():
    a = _samples()
    a0, a1, a2 = _split3(a)
    for t in (a0, a1, a2):
        assert np.isfinite(t).all()
        assert np.array_equal(t.view(np.uint32) & 0xFFFF, np.zeros_like(t.view(np.uint32)))   # representable in bfloat16
    assert np.array_equal(a0.astype(np.float64) + a1.astype(np.float64) + a2.astype(np.float64), a.astype(np.float64))


def test_rounding_matches_torch_bfloat16():
    """the packer's integer rounding is round-to-nearest-even, the rounding of the kernel's v_cvt_pk_bf16_f32 and of torch"""
    a = _samples()
    want = torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(_bf16_rne(a), want)


def test_dropped_products_below_f32_rounding():
    """sum over i + j <= 2 of a_i b_j against a * b in float64: the three dropped terms stay near 2^-23 |a b|"""
    rng = np.random.default_rng(1)
    a = rng.standard_normal(100000).astype(np.float32)
    b = rng.standard_normal(100000).astype(np.float32)
    A, B = [t.astype(np.float64) for t in _split3(a)], [t.astype(np.float64) for t in _split3(b)]
    kept = A[2] * B[0] + A[1] * B[1] + A[0] * B[2] + A[1] * B[0] + A[0] * B[1] + A[0] * B[0]
    exact = a.astype(np.float64) * b.astype(np.float64)
    assert float(np.max(np.abs(kept - exact) / np.abs(exact))) < 2.0 ** -22
