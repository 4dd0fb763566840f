"""The cases of the any-width dense weight gradient (sessd_conv2d_wgrad_any_width, ops.conv2d_wgrad(..., any_width=True)): every
width here is NO multiple of 8, so sessd_conv2d_wgrad refuses each of them. References and bounds are those of
tests/dense_grad_ref.py (float64 torch, the derived direct bound gamma(B Hout Wout + 2) x the gradient of the absolute inputs):
nothing new is introduced. No GPU is needed here: tests/test_wgrad_any_width_cpu.py shows the bounds can be met and are not
vacuous, tests/test_wgrad_any_width_gpu.py holds the kernels to them.

id -> (k, stride, B, cin, cout, Hin, Win, (kernel, nchunks, rows per chunk) of dense_grad_ref.direct_chunks). The classes of
csrc/dense_grad.hip: wout % 4 == 0 (16-byte loads, whole groups masked), even (8-byte loads of grad_out), odd (dword loads)."""
import torch

import dense_grad_ref as R

ANY_WIDTH_CASES = {
    # general kernel, 3x3 stride 1
    "s1-w12": (3, 1, 2, 6, 34, 5, 12, ("general", 10, 1)),        # one full step and one 4-pixel group
    "s1-w10": (3, 1, 2, 6, 34, 5, 10, ("general", 10, 1)),        # even width: rows 8-byte aligned
    "s1-w7": (3, 1, 3, 34, 6, 3, 7, ("general", 9, 1)),           # odd width
    "s1-w4": (3, 1, 1, 2, 2, 4, 4, ("general", 4, 1)),            # less than one step
    "s1-w20": (3, 1, 2, 6, 34, 5, 20, ("general", 10, 1)),        # the unrolled loop's prefetch of x0 + 16
    "s1-w54": (3, 1, 1, 2, 2, 9, 54, ("general", 9, 1)),          # PointPillars' own width
    "s1-w1": (3, 1, 2, 2, 2, 3, 1, ("general", 6, 1)),            # one column: kx = 0 and kx = 2 only ever read padding
    # general kernel, 3x3 stride 2
    "s2-w12": (3, 2, 2, 6, 34, 6, 24, ("general", 6, 1)),
    "s2-w10": (3, 2, 2, 6, 34, 6, 20, ("general", 6, 1)),
    "s2-w7": (3, 2, 2, 6, 34, 5, 14, ("general", 6, 1)),
    "s2-w4": (3, 2, 1, 6, 34, 2, 8, ("general", 1, 1)),
    "s2-w1": (3, 2, 1, 2, 2, 2, 2, ("general", 1, 1)),
    # general kernel, 1x1
    "1x1-w12": (1, 1, 2, 6, 34, 5, 12, ("general", 10, 1)),
    "1x1-w10": (1, 1, 2, 6, 34, 5, 10, ("general", 10, 1)),
    "1x1-w7": (1, 1, 2, 6, 34, 5, 7, ("general", 10, 1)),
    # 1x1, the 64 x 64 wave-tile kernel
    "1x1_64-w12": (1, 1, 2, 64, 64, 5, 12, ("1x1_64", 10, 1)),
    "1x1_64-w10": (1, 1, 2, 66, 98, 5, 10, ("1x1_64", 10, 1)),
    "1x1_64-w7": (1, 1, 2, 64, 64, 5, 7, ("1x1_64", 10, 1)),
    # 3x3 stride 2, the LDS-staged kernel
    "lds-w12": (3, 2, 2, 64, 64, 6, 24, ("s2_lds", 6, 1)),        # 1.5 stages per row
    "lds-w10": (3, 2, 2, 64, 128, 6, 20, ("s2_lds", 6, 1)),
    "lds-w7": (3, 2, 3, 128, 64, 46, 14, ("s2_lds", 35, 2)),      # two rows per chunk, chunks that lie in two images
    "lds-w4": (3, 2, 2, 64, 64, 5, 8, ("s2_lds", 6, 1)),
    "lds-w54": (3, 2, 1, 64, 64, 4, 108, ("s2_lds", 2, 1)),
    # ConvTranspose2d(3, 2, 1, 1) with the roles swapped (as 14-lds / 14-general of dense_grad_ref.WGRAD_CASES): x (2, 128, 3, 6) ->
    # 64 couts and x (2, 34, 3, 5) -> 6 couts; "cin" is the layer's cout
    "deconv-lds-w6": (3, 2, 2, 64, 128, 6, 12, ("s2_lds", 6, 1)),
    "deconv-general-w5": (3, 2, 2, 6, 34, 6, 10, ("general", 6, 1)),
}
DECONV_CASES = {"deconv-lds-w6": (128, 64, (2, 128, 3, 6)), "deconv-general-w5": (34, 6, (2, 34, 3, 5))}   # the layer's cin, cout, x


def inputs(name):
    """(inp, gout) of an ANY_WIDTH_CASES entry: float32 standard normals from a seed of the case's own (as R.wgrad_inputs)"""
    k, s, B, ci, co, hi, wi, _ = ANY_WIDTH_CASES[name]
    g = torch.Generator().manual_seed(sorted(ANY_WIDTH_CASES).index(name) + 300)
    ho, wo = R.out_hw(k, s, hi, wi)
    return torch.randn(B, ci, hi, wi, generator=g), torch.randn(B, co, ho, wo, generator=g)


_refs = {}


def reference(name):
    """(inp, gout, float64 gradient, bound), computed once per case and shared: callers leave them unchanged"""
    if name not in _refs:
        k, s = ANY_WIDTH_CASES[name][:2]
        inp, gout = inputs(name)
        _refs[name] = (inp, gout) + R.wgrad_reference(inp, gout, k, s)
    return _refs[name]


def reachable(k, stride, hin, win):
    """(k, k) bool: the taps that reach the image from at least one output pixel (the others only ever read padding)"""
    ho, wo = R.out_hw(k, stride, hin, win)
    p = k // 2
    rows = [any(0 <= y * stride + t - p < hin for y in range(ho)) for t in range(k)]
    cols = [any(0 <= x * stride + t - p < win for x in range(wo)) for t in range(k)]
    return torch.tensor([[r and c for c in cols] for r in rows])
