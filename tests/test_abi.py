"""The C-ABI library loads and exports every symbol include/sessd_hip.h declares (no compute)."""
import os
import re

from conftest import ROOT


def _header_functions():
    txt = open(os.path.join(ROOT, "include", "sessd_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(sessd_[a-z0-9_]+)\s*\(", txt)))


def test_header_symbols_exported_and_bound():
    import sessd_hip
    names = _header_functions()
    assert len(names) >= 10
    for n in names:
        assert hasattr(sessd_hip.lib, n), "libsessd_hip.so does not export %s" % n
        assert n in sessd_hip.SIGNATURES, "sessd_hip/_lib.py has no binding for %s" % n
    for n in sessd_hip.SIGNATURES:
        assert n in names, "%s is bound but not declared in include/sessd_hip.h" % n
    assert b"gfx950" in sessd_hip.lib.sessd_version()


def test_product_does_not_import_oracle():
    """The product package must never route through the CPU oracle."""
    pkg = os.path.join(ROOT, "se-ssd_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), os.path.join(dp, f)


def test_ops_refuse_cpu_tensors():
    import pytest
    import torch
    from sessd_hip import ops
    with pytest.raises(ValueError):
        ops.boxes_pairwise(1, torch.zeros(2, 5), torch.zeros(2, 5))


def _struct_fields(name):
    """(C type, is pointer, field name, array length or None) of every member of a typedef struct of sessd_hip_types.h"""
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sessd_hip_types.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, txt).group(1)
    decls = [re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)(?:\[(\d+)\])?", d.strip()).groups() for d in body.split(";") if d.strip()]
    return [(ctype, bool(star), field, int(dim) if dim else None) for ctype, star, field, dim in decls]


def test_dense_argument_structs_mirror_the_header():
    """sessd_conv_epilogue_t, sessd_tile_list_t and sessd_stream_k_t against their ctypes mirrors in _lib.py: the same fields in the
    same order with the same C types, and the size a C compiler gives the struct as the header spells it."""
    import ctypes
    from sessd_hip import _lib
    scalar = {"int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t}
    want = {"sessd_conv_epilogue_t": (_lib.ConvEpilogue, ["scale", "shift", "residual", "relu"]),
            "sessd_tile_list_t": (_lib.TileList, ["tiles", "count", "cap"]),
            "sessd_stream_k_t": (_lib.StreamK, ["workspace", "workspace_bytes", "workgroups", "min_rounds"])}
    for cname, (mirror, names) in want.items():
        parsed = _struct_fields(cname)
        assert [f[2] for f in parsed] == names == [n for n, _ in mirror._fields_], cname
        for (ctype, star, field, dim), (_, ptype) in zip(parsed, mirror._fields_):
            assert dim is None and ptype is (ctypes.c_void_p if star else scalar[ctype]), (cname, field)
        header = type("header_" + cname, (ctypes.Structure,),
                      {"_fields_": [(f, ctypes.c_void_p if star else scalar[ctype]) for ctype, star, f, _ in parsed]})
        assert ctypes.sizeof(mirror) == ctypes.sizeof(header), cname
    assert ctypes.sizeof(_lib.ConvEpilogue) == 32 and ctypes.sizeof(_lib.TileList) == 24 and ctypes.sizeof(_lib.StreamK) == 24   # LP64


def test_dense_entry_points_reject_bad_shapes_before_touching_the_device():
    """Argument checks of the dense-conv entry points come before any device call: they can be exercised here (null device
    pointers, no GPU). SESSD_EINVAL = -1; workspace-size queries return 0 for bad arguments. A merged entry (NULL list = the whole
    map) refuses what either of the two entries it replaces refused."""
    import ctypes
    import sessd_hip
    from sessd_hip._lib import ConvEpilogue, StreamK, TileList
    lib = sessd_hip.lib
    one = ctypes.c_int32(1)
    ptr = ctypes.addressof(one)
    epi = ConvEpilogue(relu=1)
    wg8 = StreamK(workgroups=8)
    ints = lambda *v: ctypes.cast((ctypes.c_int * len(v))(*v), ctypes.c_void_p)
    # LDS-tiled stream-K conv: cin % 16, class count, workgroups % 8, 32-bit buffer offsets, no stream-K block
    sk = lambda cin=32, nclass=1, wgs=8, hw=16, batch=1, tl=None, sk=True: lib.sessd_conv2d_sk(
        None, batch, cin, hw, hw, nclass, None, None, None, None, 1, hw, hw, None, 32, hw, hw, 1, None, None, epi, tl,
        StreamK(workgroups=wgs, min_rounds=1) if sk else None, None)
    assert sk(cin=24) == -1 and sk(nclass=5) == -1 and sk(wgs=12) == -1 and sk(cin=4096, hw=1024) == -1 and sk(sk=False) == -1
    assert lib.sessd_conv2d_sk_workspace_bytes(0, 8, 8, 32, 1, 8) == 0 and lib.sessd_conv2d_sk_workspace_bytes(1, 8, 8, 32, 5, 8) == 0
    # explicit workgroup count: pure arithmetic (counters of nclass * batch * pixel tiles * cout groups + two 64 KB slots per workgroup)
    assert lib.sessd_conv2d_sk_workspace_bytes(2, 100, 88, 256, 1, 256) == 256 * ((2 * 69 * 2 * 4 + 255) // 256) + 2 * 256 * 65536
    assert lib.sessd_conv2d_sk_pack(None, 1, 1, None, 1, 32, 24, None, None) == -1
    # its active-tile mode: a tile list with its device count, even tile space, the WHOLE batch inside 32-bit offsets
    assert sk(tl=TileList(None, ptr, 4)) == -1 and sk(tl=TileList(ptr, None, 4)) == -1 and sk(tl=TileList(ptr, ptr, 0)) == -1
    assert sk(tl=TileList(ptr, ptr, 4), hw=15) == -1
    assert sk(tl=TileList(ptr, ptr, 4), hw=1024, batch=32, cin=16) == -1
    # tile activity: a stride-2 step that takes a slot needs an output of even size; at most eight slots; step 4 only behind a step 3
    steps = lambda *v: (ctypes.c_int32 * len(v))(*v)
    act = lambda st, h=200, w=176: lib.sessd_bev_tile_activity(ptr, ptr, 1, 1, h, w, st, len(st), ptr, ptr, ptr, 1, None, 0, None)
    assert act(steps(2), h=202) == -1 and act(steps(0, 0, 0, 2, 0, 0, 0, 0, 0)) == -1 and act(steps(4)) == -1 and act(steps(0, 4)) == -1 and act(steps(3), w=192) == -1
    assert act(steps(3, 4, 0), h=200, w=100) == -1   # the doubled map must fit the kernel's pixel rows
    assert lib.sessd_fill_inactive_tiles(None, 13, 1, None) == -1
    # Winograd stream-K over weight sets: the batch must split evenly, even maps; with a list: one set, not shape 2, a whole list
    wsk = lambda batch=2, nsets=1, h=8, w=8, tl=None, shape=0, sk=wg8: lib.sessd_conv3x3_winograd_sk(
        None, batch, nsets, 128, h, w, None, None, 128, epi, tl, sk, shape, None)
    lst = TileList(ptr, ptr, 4)
    assert wsk(batch=3, nsets=2) == -1 and wsk(nsets=2, h=7) == -1 and wsk(sk=None) == -1 and wsk(sk=StreamK(workgroups=12)) == -1
    assert wsk(nsets=2, tl=lst) == -1 and wsk(tl=lst, shape=2) == -1
    assert wsk(tl=TileList(None, ptr, 4)) == -1 and wsk(tl=TileList(ptr, None, 4)) == -1 and wsk(tl=TileList(ptr, ptr, 0)) == -1
    assert wsk() == -2 and wsk(nsets=2) == -2 and wsk(tl=lst) == -2 and wsk(shape=2) == -2   # past every check: no workspace given
    # the direct kernel over a tile list: four effective taps, tile_cfg 3 / 4 / 11 / 12, even tile space, the whole batch in 32 bits
    z9 = ints(*([0] * 9))
    mf = lambda ntaps=1, cfg=11, hw=16, batch=1, cin=32, tl=lst: lib.sessd_conv2d_mfma(
        None, batch, cin, hw, hw, None, ntaps, z9, z9, 1, hw, hw, None, 32, hw, hw, 1, 0, 0, epi, tl, cfg, None)
    assert mf(cfg=1) == -1 and mf(ntaps=9) == -1 and mf(cin=36) == -1 and mf(hw=15) == -1 and mf(cfg=13) == -1
    assert mf(hw=1024, batch=32, cin=16) == -1
    assert mf(tl=TileList(None, ptr, 4)) == -1 and mf(tl=TileList(ptr, None, 4)) == -1 and mf(tl=TileList(ptr, ptr, 0)) == -1
    assert mf(cin=31, tl=None) == -1 and mf(ntaps=10, tl=None) == -1 and mf(cfg=9, tl=None) == -1   # the whole-map launch's own
    # two transposed convs in one launch: cin % 8; with a list also even hin / win
    pair = lambda cin=16, hin=8, tl=None: lib.sessd_deconv2d_s2_mfma_pair(None, 1, cin, hin, 8, None, None, None, None, None, None, None, 32,
                                                                        epi, epi, tl, 4, None)
    assert pair(cin=12) == -1 and pair(hin=7, tl=lst) == -1 and pair(tl=TileList(ptr, ptr, 0)) == -1
    # fused SSFA tail + heads
    assert lib.sessd_ssfa_fuse_head(None, None, None, None, 1.0, 0.0, 1.0, 0.0, 1, 100, 64, None, None, None, 22, None, None) == -1
    assert lib.sessd_ssfa_fuse_head(None, None, None, None, 1.0, 0.0, 1.0, 0.0, 1, 128, 64, None, None, None, 21, None, None) == -1


def test_sparse_entry_points_reject_what_their_kernels_cannot_cover():
    """Round-2 advisor / review items, checked before any device call (null device pointers, no GPU):
    * sessd_sparse_chain_rulebooks: chain_rulebook_kernel covers at most 12 (kz, ky) pairs and 3 taps in x -- a (5,5,1) or
      (1,1,5) kernel passed the old volume <= 32 check and would have left neighbour-table rows unwritten;
    * sessd_sparse_hash_build: one batch element's D*H*W must stay below the empty marker 0x7F7F7F7F of the 31-bit keys."""
    import ctypes as C
    import sessd_hip
    from sessd_hip._lib import ChainLevel, RulebookJob
    lib = sessd_hip.lib
    lv = (ChainLevel * 1)()
    lv[0].ksize[:] = [3, 3, 3]
    lv[0].stride[:] = [2, 2, 2]
    lv[0].pad[:] = [1, 1, 1]
    lv[0].out_dims[:] = [21, 800, 704]
    lv[0].cap = 1024
    dims0 = (C.c_int * 3)(41, 1600, 1408)
    ws = (C.c_char * 16)()

    def rulebooks(ks):
        job = (RulebookJob * 1)()
        job[0].in_level, job[0].out_level = 1, 1
        job[0].ksize[:] = ks
        job[0].stride[:] = [1, 1, 1]
        job[0].pad[:] = [k // 2 for k in ks]
        job[0].nbr, job[0].tile_mask = 16, 16  # non-null, never dereferenced: the call must fail first
        return lib.sessd_sparse_chain_rulebooks(None, None, 1024, None, None, 1024, C.cast(dims0, C.c_void_p), 1, 1, C.cast(lv, C.c_void_p),
                                                C.cast(ws, C.c_void_p), 1, C.cast(job, C.c_void_p), None)

    assert rulebooks([5, 5, 1]) == -1 and rulebooks([1, 1, 5]) == -1 and rulebooks([4, 4, 2]) == -1 and rulebooks([0, 3, 3]) == -1
    big = (C.c_int * 3)(2048, 2048, 1024)
    assert lib.sessd_sparse_hash_build(None, None, 16, C.cast(big, C.c_void_p), None, None, 64, None) == -1
    assert lib.sessd_sparse_hash_build(None, None, 16, None, None, None, 64, None) == -1
    assert lib.sessd_sparse_hash_build(None, None, 16, C.cast(dims0, C.c_void_p), None, None, 48, None) == -1  # capacity not a power of two


def test_round3_training_entry_points_reject_bad_arguments_before_touching_the_device():
    """Argument checks of the training-path entry points of round 3, before any device call (null pointers, no GPU):
    the Winograd-domain weight gradient's shape rule and workspace arithmetic, the fused SSFA attention tail, the train-mode
    BatchNorm layouts, the batched packers, the channel sum and the host box functions."""
    import ctypes as C
    import numpy as np
    import sessd_hip
    lib = sessd_hip.lib
    wb = lib.sessd_conv3x3_wgrad_winograd_workspace_bytes
    # covered: cin, cout % 64, even H, W >= 16;  64 chunks x 16 xi x cin x cout floats for the SSFA layers at batch 4
    assert wb(4, 128, 128, 200, 176) == 64 * 16 * 128 * 128 * 4 and wb(4, 256, 256, 100, 88) == 16 * 16 * 256 * 256 * 4
    assert wb(1, 48, 128, 64, 64) == 0 and wb(1, 128, 128, 63, 64) == 0 and wb(1, 128, 128, 64, 12) == 0 and wb(0, 128, 128, 64, 64) == 0
    assert lib.sessd_conv3x3_wgrad_winograd(None, 1, 128, 64, 64, None, 128, None, None, 0, None) == -1        # null tensors
    assert lib.sessd_conv3x3_wgrad_winograd(16, 1, 128, 64, 64, 16, 128, 16, None, 0, None) == -2               # workspace too small
    # fused SSFA tail: channels % 4, plane % 4, all-or-none running statistics
    sb = lib.sessd_ssfa_fuse_train_workspace_bytes
    assert sb(4, 128, 35200) > 4352 and sb(4, 126, 35200) == 0 and sb(4, 128, 35202) == 0 and sb(0, 128, 64) == 0
    assert lib.sessd_ssfa_fuse_train_fwd(None, None, 1, 128, 64, None, None, None, None, None, None, 1e-3, 0.01, None, None, None, None, None,
                                         None, None, None, 0, None) == -1
    assert lib.sessd_ssfa_fuse_train_fwd(16, 16, 1, 128, 64, 16, 16, None, None, None, None, 1e-3, 0.01, 16, None, None, None, 16, 16, 16, 16,
                                         1 << 20, None) == -1   # one of the four running-statistics pointers
    # train-mode BatchNorm: power-of-two channels <= 256 (sparse layout), plane % 4 and <= 1024 channels (dense layout)
    assert lib.sessd_bn_relu_train_fwd(None, None, 64, 24, None, None, 1e-3, 0.01, 1, None, None, None, None, None, None, 0, None) == -1
    assert lib.sessd_bn_relu_train_fwd(None, None, 64, 16, None, None, 1e-3, 0.01, 1, None, None, None, None, None, None, 0, None) == -2
    assert lib.sessd_bn2d_relu_train_fwd(None, 1, 8, 30, None, None, 1e-3, 0.01, 1, None, None, None, None, None, None, 0, None) == -1
    assert lib.sessd_bn2d_relu_train_bwd_x(None, None, 1, 2048, 64, None, None, None, None, 1, None, None, None, None, 0, None) == -1
    assert lib.sessd_bn2d_relu_train_bwd(None, None, None, 1, 8, 64, None, None, None, 1, None, 16, 16, 16, 1 << 20, None) == -1   # relu without y
    assert lib.sessd_nchw_channel_sum(None, 1, 8, 30, None, None, 0, None) == -1
    assert lib.sessd_bn2d_relu_train_workspace_bytes(128) == 4096 + 128 * 16 * 2 * 8
    assert lib.sessd_bn_relu_train_workspace_bytes(64) == 256 + 128 * 2 * 64 * 8
    # batched packers, adjoint pack
    assert lib.sessd_dense_pack_batch(None, 3, 10, None) == -1 and lib.sessd_sparse_pack_batch(16, 0, 10, None) == -1
    assert lib.sessd_sparse_pack_weight_adjoint(None, 27, 24, 64, 1, None, None) == -1
    # host box functions run here: two overlapping unit squares, one far away
    sq = np.array([[[0, 0], [0, 1], [1, 1], [1, 0]]], dtype=np.float64)
    qs = np.concatenate([sq + 0.5, sq + 5.0], 0)
    out = np.zeros((1, 2), dtype=np.uint8)
    assert lib.sessd_box_collision_host(sq.ctypes.data, 1, qs.ctypes.data, 2, 0, 1, out.ctypes.data) == 0 and out.tolist() == [[1, 0]]
    assert lib.sessd_box_collision_host(None, 1, qs.ctypes.data, 2, 0, 1, out.ctypes.data) == -1
    assert lib.sessd_noise_per_box_host(None, None, None, None, None, None, 2, 3, 0, None) == -1


def test_head_loss_entry_point_checks_its_arguments():
    """sessd_head_loss (round 4): configuration and pointer checks come before any device call (no GPU here)."""
    import ctypes as C
    import sessd_hip
    from sessd_hip._lib import HeadLossCfg, HeadLossNet
    lib = sessd_hip.lib
    c = HeadLossCfg()
    assert lib.sessd_head_loss_workspace_bytes(C.addressof(c)) == 0          # batch 0
    c.batch, c.num_anchors, c.pos_capacity, c.cons_capacity = 4, 70400, 4096, 2048
    c.pos_cls_weight = c.neg_cls_weight = 1.0
    c.smooth_l1_sigma = 3.0
    need = lib.sessd_head_loss_workspace_bytes(C.addressof(c))
    # counts per block + 12 doubles per block + the positive / candidate lists: a few MB, growing with the capacities
    assert 1 << 19 < need < 64 << 20
    c.cons_capacity = 4096
    assert lib.sessd_head_loss_workspace_bytes(C.addressof(c)) > need
    n = HeadLossNet()
    assert lib.sessd_head_loss(C.addressof(c), C.addressof(n), C.addressof(n), None, None, None, None, None, None, None, None, None, 0, None) == -1
    assert lib.sessd_head_loss(None, None, None, None, None, None, None, None, None, None, None, None, 0, None) == -1
    c.batch = 65
    assert lib.sessd_head_loss_workspace_bytes(C.addressof(c)) == 0


def test_predict_args_mirror_and_argument_checks():
    """sessd_predict_args_t and _lib.PredictArgs are one layout: the same size as the library compiled it, the same fields in the
    same order, pointer for pointer and scalar for scalar. The entry point's argument checks come before any device call (null
    pointers, no GPU): SESSD_EINVAL = -1, SESSD_EWORKSPACE = -2; the workspace query returns 0 for what it refuses."""
    import ctypes
    import sessd_hip
    from sessd_hip._lib import DiCfg, PredictArgs
    lib = sessd_hip.lib
    assert ctypes.sizeof(PredictArgs) == lib.sessd_predict_args_bytes()
    decls = _struct_fields("sessd_predict_args_t")
    scalar = dict(int32_t=ctypes.c_int, float=ctypes.c_float)
    assert len(decls) == len(PredictArgs._fields_) == 29
    for (ctype, star, name, dim), (pname, ptype) in zip(decls, PredictArgs._fields_):
        assert name == pname
        if star:
            assert ptype is ctypes.c_void_p or (ctype == "sessd_di_cfg_t" and ptype is ctypes.POINTER(DiCfg)), name
        else:
            assert ptype is (scalar[ctype] * int(dim) if dim else scalar[ctype]), name

    def call(**kw):
        v = dict(batch=1, num_tasks=1, num_pixels=64, score_thresh=0.3, pre_max_size=100, post_max_size=10, nms_iou_thresh=0.01)
        v.update(kw)
        return lib.sessd_predict(PredictArgs(**v), None, 0, None)

    di = DiCfg(n_interval=4)
    assert lib.sessd_predict(None, None, 0, None) == -1
    assert call() == -2 and call(di=ctypes.pointer(di)) == -2          # valid scalars: every check passes, no workspace given
    assert call(num_tasks=0) == -1 and call(num_tasks=5) == -1
    assert call(batch=0) == -1 and call(num_pixels=0) == -1 and call(post_max_size=0) == -1 and call(pre_max_size=1985) == -1
    assert call(pre_max_size=1025) == -2 and call(pre_max_size=1025, di=ctypes.pointer(di)) == -1
    assert call(di=ctypes.pointer(DiCfg(n_interval=9))) == -1 and call(di=ctypes.pointer(DiCfg(n_interval=-1))) == -1
    assert call(ext_keys=16) == -1 and call(ext_key_count=16) == -1 and call(di_keep=16) == -1   # both or neither
    assert call(records=16) == -1 and call(records=16, record_counts=16, cursor=16, capacity_frames=0) == -1
    assert call(anchors_per_frame=64) == -1 and call(anchors_per_frame=128) == -2
    wb = lib.sessd_predict_workspace_bytes
    assert wb(0, 1, 128, 100, 10, 0) == 0 and wb(1, 0, 128, 100, 10, 0) == 0 and wb(1, 5, 128, 100, 10, 1) == 0
    assert wb(1, 1, 128, 1025, 10, 1) == 0 and wb(1, 1, 128, 0, 10, 1) == 0 and wb(1, 1, 128, 1025, 10, 0) > 0
