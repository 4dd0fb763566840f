"""SHA-256 of the output bytes of every dense launch entry of include/sessd_hip.h, through the public functions of sessd_hip.ops
only -- so the same file runs on a tree before and after a change of the C boundary (copy it into the other tree's scripts/ and
run it there, on the same machine: the stream-K kernels' default workgroup count follows the device). Two runs agree when every
line agrees (profiles/dense_args_outputs_ab.txt).

Shapes: batch 2, cin 32, cout 160 (a second, partial 128-cout group), map 12 x 20 (60 2x2 tiles: the last block of 32 is partial).
List launches run over four lists: some tiles (the first and last of both images and a few inner ones), every tile, an empty list
(count 0) and a count above the capacity, which the kernels clamp; their outputs start from a fixed pattern, so the hash also
covers the pixels a launch must leave alone. Stream-K launches run at 8 workgroups and at the default.
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "se-ssd_amd"))

import torch  # noqa: E402
from sessd_hip import ops  # noqa: E402

B, CIN, COUT, H, W = 2, 32, 160, 12, 20


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(20240611)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    x = rnd(B, CIN, H, W)
    scale, shift = rnd(COUT) * 0.5 + 1.0, rnd(COUT)
    scale2, shift2 = rnd(2, COUT) * 0.5 + 1.0, rnd(2, COUT)
    w3, w3b, w1, wt_a, wt_b = rnd(COUT, CIN, 3, 3), rnd(COUT, CIN, 3, 3), rnd(COUT, CIN, 1, 1), rnd(CIN, COUT, 3, 3), rnd(CIN, COUT, 3, 3)
    pc3, pc3b, pc3s2, pc1 = ops.pack_conv2d(w3), ops.pack_conv2d(w3b), ops.pack_conv2d(w3, stride=2), ops.pack_conv2d(w1)
    pcd_a, pcd_b = ops.pack_deconv2d_s2(wt_a), ops.pack_deconv2d_s2(wt_b)
    res = {hw: rnd(B, COUT, *hw) for hw in ((H, W), (H // 2, W // 2), (2 * H, 2 * W))}
    pattern = {hw: rnd(B, COUT, *hw) for hw in res}
    lines = []

    def put(name, *outs):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for o in outs:
            h.update(o.detach().cpu().numpy().tobytes())
        lines.append("%-64s %s" % (name, h.hexdigest()))

    def fresh(hw):
        return pattern[hw].clone()

    def lists(nt):
        """name -> (tile_list, n_list) over B images of nt tiles each"""
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
        some = [0, 3, nt // 2, nt - 1, nt, nt + 5, 2 * nt - 2, 2 * nt - 1]
        every = list(range(B * nt))
        return {"some": (i32(some), i32([len(some)])), "every": (i32(every), i32([len(every)])), "empty": (i32(some), i32([0])),
                "count>cap": (i32(every), i32([len(every) + 7]))}

    wsk_ws = lambda shape, wg, batch=B: ops.winograd_sk_workspace(batch, H, W, COUT, dev, wg, shape)
    csk_ws = lambda pc, wg: ops.conv2d_sk_workspace(B, *pc.tile_hw(H, W), COUT, len(pc.launches), dev, wg)

    # ---- whole-map launches
    for cfg in (4, 11, 10):
        put("conv2d_mfma 3x3 s1 tile_cfg %d" % cfg, ops.conv2d(x, pc3, scale, shift, True, res[(H, W)], tile_cfg=cfg))
    put("conv2d_mfma 3x3 s2 tile_cfg 6", ops.conv2d(x, pc3s2, scale, shift, True, res[(H // 2, W // 2)], tile_cfg=6))
    put("conv2d_mfma 1x1 tile_cfg 3, no epilogue", ops.conv2d(x, pc1, None, None, False, None, tile_cfg=3))
    for cfg in (20, 21):
        put("conv3x3_winograd tile_cfg %d" % cfg, ops.conv2d(x, pc3, scale, shift, True, res[(H, W)], tile_cfg=cfg))
    for wg in (8, 0):
        for cfg in (22, 23, 24, 25):
            put("conv3x3_winograd_sk shape %d workgroups %d" % (cfg - 22, wg),
                ops.conv2d(x, pc3, scale, shift, True, res[(H, W)], tile_cfg=cfg, workspace=wsk_ws(cfg - 22, wg), workgroups=wg))
        for shape in (0, 1, 2, 3):
            upk = torch.cat([pc3.upk_sk(shape).reshape(-1).view(torch.uint8), pc3b.upk_sk(shape).reshape(-1).view(torch.uint8)])
            out = torch.empty((B, COUT, H, W), device=dev)
            ops.conv2d_winograd_sk_sets(x, upk, 2, COUT, scale2, shift2, True, out, shape, wsk_ws(shape, wg), wg, res[(H, W)])
            put("conv3x3_winograd_sk_sets shape %d workgroups %d" % (shape, wg), out)
        for name, pc, hw in (("3x3 s2", pc3s2, (H // 2, W // 2)), ("1x1", pc1, (H, W)), ("deconv", pcd_a, (2 * H, 2 * W))):
            put("conv2d_sk %s workgroups %d" % (name, wg),
                ops.conv2d(x, pc, scale, shift, True, res[hw], tile_cfg=30, workspace=csk_ws(pc, wg), workgroups=wg))
    for cfg in (4, 12, 40, 42):
        put("deconv2d_s2_mfma tile_cfg %d" % cfg, ops.conv2d(x, pcd_a, scale, shift, True, res[(2 * H, 2 * W)], tile_cfg=cfg))
    for cfg in (4, 11):
        oa, ob = torch.empty((B, COUT, 2 * H, 2 * W), device=dev), torch.empty((B, COUT, 2 * H, 2 * W), device=dev)
        ops.deconv2d_s2_pair(x, pcd_a, pcd_b, scale2[0], shift2[0], scale2[1], shift2[1], True, oa, ob, res[(2 * H, 2 * W)], None, cfg)
        put("deconv2d_s2_mfma_pair tile_cfg %d" % cfg, oa, ob)

    # ---- list launches
    for kind, (tl, nl) in lists((H // 2) * (W // 2)).items():
        for wg in (8, 0):
            for shape in (0, 1, 3):
                for mr in (2, -1):
                    out = fresh((H, W))
                    ops.conv2d_winograd_sk_active(x, pc3.upk_sk(shape), COUT, scale, shift, True, out, shape, wsk_ws(shape, wg), tl, nl, wg,
                                                  res[(H, W)], mr)
                    put("conv3x3_winograd_sk_active shape %d workgroups %d min_rounds %d list %s" % (shape, wg, mr, kind), out)
            out = fresh((H, W))
            ops.conv2d_sk_active(x, pc1, scale, shift, True, out, csk_ws(pc1, wg), tl, nl, wg, res[(H, W)], 4)
            put("conv2d_sk_active 1x1 workgroups %d list %s" % (wg, kind), out)
        for cfg in (11, 3):
            out = fresh((H, W))
            ops.conv2d_mfma_active(x, pc1, scale, shift, True, out, tl, nl, cfg, res[(H, W)])
            put("conv2d_mfma_active tile_cfg %d list %s" % (cfg, kind), out)
        for cfg in (11, 4):
            oa, ob = fresh((2 * H, 2 * W)), fresh((2 * H, 2 * W))
            ops.deconv2d_s2_pair_active(x, pcd_a, pcd_b, scale2[0], shift2[0], scale2[1], shift2[1], True, oa, ob, tl, nl, res[(2 * H, 2 * W)],
                                        None, cfg)
            put("deconv2d_s2_mfma_pair_active tile_cfg %d list %s" % (cfg, kind), oa, ob)
        oa, ob = fresh((2 * H, 2 * W)), fresh((2 * H, 2 * W))
        ops.deconv2d_s2_pair_split_active(x, pcd_a, pcd_b, scale2[0], shift2[0], scale2[1], shift2[1], True, oa, ob, tl, nl, None,
                                          res[(2 * H, 2 * W)])
        put("deconv2d_s2_pair_split_active list %s" % kind, oa, ob)
    for kind, (tl, nl) in lists((H // 4) * (W // 4)).items():   # the stride-2 layer's lists hold tiles of its OUTPUT map
        for wg in (8, 0):
            out = fresh((H // 2, W // 2))
            ops.conv2d_sk_active(x, pc3s2, scale, shift, True, out, csk_ws(pc3s2, wg), tl, nl, wg, res[(H // 2, W // 2)], 1)
            put("conv2d_sk_active 3x3 s2 workgroups %d list %s" % (wg, kind), out)
        out = fresh((H // 2, W // 2))
        ops.conv2d_s2_split_active(x, pc3s2, scale, shift, True, out, tl, nl, res[(H // 2, W // 2)])
        put("conv2d_s2_split_active list %s" % kind, out)
    print("\n".join(lines))
    print("# %d launches, %s" % (len(lines), torch.cuda.get_device_name(0)))


if __name__ == "__main__":
    main()
