"""Stream-K Winograd shape 3 (csrc/dense_wino_sk.hip SPLIT): the main loop that runs the patch transform of the next round in the
MFMA gaps of this round (variant 0, ships) against the loop that runs it as one block at the end of the round (SESSD_WINO_VAR=4).
Same IEEE additions in the same association, so the outputs are held equal BIT FOR BIT, on the same inputs, packing and workspace
size. The variant is read from the environment once per process: the end-of-round arm runs in one child process (this file as a
script) that saves every case's output; the cases are the smallest shapes at which the pipeline can go wrong."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD_VAR = 4

# (cin, cout, B, H, W, workgroups), tile_cfg 25
FULL = [(16, 128, 1, 8, 8, 8),      # a unit is one round: prologue only
        (32, 40, 1, 4, 66, 8),      # two rounds, a cout tail, tw = 33: the last tile block is partial, both edge masks
        (48, 128, 3, 10, 66, 16),   # three rounds, shares cut units: segments start at r0 > 0 and end before rpu
        (16, 128, 1, 2, 4, 8)]      # every tile a left- or right-edge tile, rows above and below out of the image
LIST_GEOM = (48, 128, 2, 16, 16)    # cin, cout, B, H, W
COUNTS = [0, 1, 31, 32, 33, 70]
MIN_ROUNDS = [-1, 1, 2]


def _full_inputs(case):
    cin, cout, B, H, W, _ = case
    g = torch.Generator().manual_seed(cin * 1000 + H * 10 + W)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.05
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    res = torch.randn(B, cout, H, W, generator=g)
    return x, w, sc, sh, res


def _run_full(dev, case, epilogue):
    from sessd_hip import ops
    cin, cout, B, H, W, wgs = case
    x, w, sc, sh, res = (t.to(dev) for t in _full_inputs(case))
    pc = ops.pack_conv2d(w, 1)
    ws = ops.winograd_sk_workspace(B, H, W, cout, dev, wgs, 3)
    if epilogue:
        out = ops.conv2d(x, pc, sc, sh, True, residual=res, tile_cfg=25, workspace=ws, workgroups=wgs)
    else:
        out = ops.conv2d(x, pc, None, None, False, tile_cfg=25, workspace=ws, workgroups=wgs)
    torch.cuda.synchronize()
    return out.cpu()


def _list_entries(count):
    """`count` entries (image * ntiles + tile, sorted) of one seeded random set of 70 over both images of the 16 x 16 map; from 2
    entries on the first and the last of the set are among them, so the entries span both images"""
    _, _, B, H, W = LIST_GEOM
    full = np.sort(np.random.default_rng(11).choice(B * (H // 2) * (W // 2), 70, replace=False)).astype(np.int32)
    assert full[0] < (H // 2) * (W // 2) <= full[-1]
    return full[np.round(np.linspace(0, 69, count)).astype(np.int64)] if count else full[:0]


def _run_list(dev, count, min_rounds, launches=1):
    from sessd_hip import ops
    cin, cout, B, H, W = LIST_GEOM
    g = torch.Generator().manual_seed(77)
    x = torch.randn(B, cin, H, W, generator=g).to(dev)
    w = (torch.randn(cout, cin, 3, 3, generator=g) * 0.05).to(dev)
    pc = ops.pack_conv2d(w, 1)
    e = _list_entries(count)
    tl = torch.zeros(70, dtype=torch.int32)
    tl[:count] = torch.from_numpy(e)
    tl, n = tl.to(dev), torch.tensor([count], dtype=torch.int32, device=dev)
    ws = ops.winograd_sk_workspace(B, H, W, cout, dev, 0, 3)
    outs = []
    for _ in range(launches):
        out = torch.full((B, cout, H, W), float("nan"), device=dev)
        ops.conv2d_winograd_sk_active(x, pc.upk_sk(3), cout, None, None, False, out, 3, ws, tl, n, min_rounds=min_rounds)
        outs.append(out)
    torch.cuda.synchronize()
    return [o.cpu() for o in outs]


def _full_name(i, epilogue):
    return "full%d_%s" % (i, "epi" if epilogue else "bare")


def _list_name(count, min_rounds):
    return "list%d_mr%d" % (count, min_rounds)


def _bits(t):
    return t.contiguous().view(torch.int32)


if __name__ == "__main__":   # the child: the end-of-round arm, every case, outputs as .npy under argv[1]
    for p in (ROOT, os.path.join(ROOT, "se-ssd_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    assert int(os.environ["SESSD_WINO_VAR"]) == OLD_VAR
    d = torch.device("cuda:0")
    for i, case in enumerate(FULL):
        for epi in (False, True):
            np.save(os.path.join(sys.argv[1], _full_name(i, epi) + ".npy"), _run_full(d, case, epi).numpy())
    for c in COUNTS:
        for mr in MIN_ROUNDS:
            np.save(os.path.join(sys.argv[1], _list_name(c, mr) + ".npy"), _run_list(d, c, mr)[0].numpy())
    print("saved")
    sys.exit(0)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def old_arm(tmp_path_factory):
    """outputs of the end-of-round loop: one fresh child process for all cases"""
    assert not int(os.environ.get("SESSD_WINO_VAR", "0")) & OLD_VAR, "this process must run the pipelined loop (variant bit 2 clear)"
    out = tmp_path_factory.mktemp("wino_old_arm")
    env = dict(os.environ, SESSD_WINO_VAR=str(OLD_VAR))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=env, capture_output=True, text=True, timeout=300,
                       cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    return lambda name: torch.from_numpy(np.load(os.path.join(str(out), name + ".npy")))


@pytest.mark.parametrize("epilogue", [False, True], ids=["bare", "bn_relu_residual"])
@pytest.mark.parametrize("i", range(len(FULL)), ids=["%dx%d_b%d_%dx%d_wg%d" % c for c in FULL])
def test_full_map_bits(dev, old_arm, i, epilogue):
    new = _run_full(dev, FULL[i], epilogue)
    assert torch.isfinite(new).all()
    old = old_arm(_full_name(i, epilogue))
    assert new.shape == old.shape and torch.equal(_bits(new), _bits(old)), float((new - old).abs().max())


@pytest.mark.parametrize("min_rounds", MIN_ROUNDS)
@pytest.mark.parametrize("count", COUNTS)
def test_list_bits(dev, old_arm, count, min_rounds):
    _, cout, B, H, W = LIST_GEOM
    a, b = _run_list(dev, count, min_rounds, launches=2)
    assert torch.equal(_bits(a), _bits(b)), "two launches differ"
    e = _list_entries(count).astype(np.int64)
    nt, tw = (H // 2) * (W // 2), W // 2
    listed = torch.zeros(B, H, W, dtype=torch.bool)
    for a0 in (0, 1):
        for b0 in (0, 1):
            listed[e // nt, 2 * ((e % nt) // tw) + a0, 2 * ((e % nt) % tw) + b0] = True
    assert int(listed.sum()) == 4 * count
    m = listed[:, None].expand(B, cout, H, W)
    assert torch.isfinite(a[m]).all() and torch.isnan(a[~m]).all()   # count 0: nothing written
    assert torch.equal(_bits(a), _bits(old_arm(_list_name(count, min_rounds))))
