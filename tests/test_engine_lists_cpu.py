"""The engine's table of list layers and the reach rule of the inactive-tile fill (sessd_hip.engine.fill_reach) as a pure function:
no device, no weights. The tables are the plan classes' own list_layers() over stand-in buffers (the rule reads names, kinds, masks
and near ids only).

The expected jobs are DATA: what InferenceEngine._fill_jobs returned for the same id sets on an MI355X before the rule was
separated from its buffers (commit e8bb4e2; an SSFA engine of the benchmark model, an RPN engine of the three-class config with six
block layers). One entry per fill job, in order: (layer id, mask slot, tile size, near slot, near kind)."""
from types import SimpleNamespace

from sessd_hip.engine import DensePlan, RpnPlan, fill_reach


def _ssfa_table():
    plan = SimpleNamespace(b0=["b0.0", "b0.1", "b0.2"], b1=["b1.0", "b1.1", "b1.2"], trans_0="trans_0", trans_1="trans_1",
                           deconv_0="deconv_0", deconv_1="deconv_1", conv_0="conv_0", conv_1="conv_1")
    t = {k: "t." + k for k in ("a", "b", "x0", "tr0", "out", "mid0", "mid1", "o0", "o1")}
    h = {k: "h." + k for k in ("a", "b", "x1", "tr1")}
    return DensePlan.list_layers(plan, "bev", t, h)


def _rpn_table(nl=6):
    plan = SimpleNamespace(layers=["blk0.%d" % i for i in range(nl)])
    return RpnPlan.list_layers(plan, "bev", {"l%d" % i: "t.l%d" % i for i in range(nl)}, {})


PAIR = [(8, 6, 4, None, 0)] * 2       # one job per output of the transposed pair: 4x4 blocks, filled everywhere
BRANCHES = [(9, 7, 6, None, 0)] * 2   # one job per branch behind conv_0 / conv_1
ALL = set(range(10))
SSFA_CASES = [
    # (ids, near_fill, coarse_fill, jobs)
    (ALL, True, True, [(0, 0, 2, 1, 0), (1, 1, 2, 2, 0), (2, 2, 2, 3, 2), (3, 3, 2, 4, 0), (4, 4, 2, 5, 0), (6, 2, 2, 6, 1),
                       (7, 5, 2, None, 0)] + PAIR + BRANCHES),
    (ALL - {3}, True, True, [(0, 0, 2, 1, 0), (1, 1, 2, 2, 0), (2, 2, 2, None, 0), (4, 4, 2, 5, 0), (6, 2, 2, 6, 1),
                             (7, 5, 2, None, 0)] + PAIR + BRANCHES),
    (ALL - {6}, True, True, [(0, 0, 2, 1, 0), (1, 1, 2, 2, 0), (2, 2, 2, None, 0), (3, 3, 2, 4, 0), (4, 4, 2, 5, 0),
                             (7, 5, 2, None, 0)] + PAIR + BRANCHES),
    (ALL - {7}, True, True, [(0, 0, 2, 1, 0), (1, 1, 2, 2, 0), (2, 2, 2, 3, 2), (3, 3, 2, 4, 0), (4, 4, 2, 5, 0), (5, 5, 2, None, 0),
                             (6, 2, 2, 6, 1)] + PAIR + BRANCHES),
    (ALL - {8}, True, True, [(0, 0, 2, 1, 0), (1, 1, 2, 2, 0), (2, 2, 2, 3, 2), (3, 3, 2, 4, 0), (4, 4, 2, 5, 0), (6, 2, 2, None, 0),
                             (7, 5, 2, None, 0)] + BRANCHES),
    ({0, 1, 2}, True, True, [(0, 0, 2, 1, 0), (1, 1, 2, 2, 0), (2, 2, 2, None, 0)]),
    (ALL, False, True, [(0, 0, 2, None, 0), (1, 1, 2, None, 0), (2, 2, 2, None, 0), (3, 3, 2, None, 0), (4, 4, 2, None, 0),
                        (5, 5, 2, None, 0), (6, 2, 2, None, 0), (7, 5, 2, None, 0)] + PAIR + BRANCHES),
    (ALL, True, False, [(0, 0, 2, 1, 0), (1, 1, 2, 2, 0), (2, 2, 2, None, 0), (3, 3, 2, 4, 0), (4, 4, 2, 5, 0), (5, 5, 2, None, 0),
                        (6, 2, 2, None, 0), (7, 5, 2, None, 0)] + PAIR + BRANCHES),
]
RPN_ALL_SIX = [(0, 0, 2, 1, 0), (1, 1, 2, 2, 0), (2, 2, 2, 3, 0), (3, 3, 2, 4, 0), (4, 4, 2, 5, 0), (5, 5, 2, None, 0)]


def _jobs(table, ids, near_fill=True, coarse_fill=True):
    jobs = fill_reach(table, sorted(ids), near_fill, coarse_fill)
    # a row with two outputs gives one job per output, in order; every other job names no part
    for l in set(j[0] for j in jobs):
        parts = [j[1] for j in jobs if j[0] == l]
        assert parts == ([0, 1] if table[l].kind in ("pair", "branches") else [None]), (l, parts)
    return [(l, slot, tile, near, kind) for l, _, slot, tile, near, kind in jobs]


def test_the_tables_the_plans_supply():
    ssfa = _ssfa_table()
    assert [r.name for r in ssfa.values()] == ["b0.0", "b0.1", "b0.2", "b1.0", "b1.1", "b1.2", "trans_0", "trans_1",
                                               "deconv_0+deconv_1", "conv_0+conv_1"]
    assert [r.kind for r in ssfa.values()] == ["wino"] * 3 + ["direct", "wino", "wino", "direct", "direct", "pair", "branches"]
    assert {l: r.mask for l, r in ssfa.items()} == {0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 2, 7: 5, 8: 6, 9: 7}
    assert {l: r.near for l, r in ssfa.items() if r.near is not None} == {0: 1, 1: 2, 3: 4, 4: 5}
    assert tuple(ssfa[8][:4]) == ("deconv_0+deconv_1", ("deconv_0", "deconv_1"), "h.tr1", ("t.mid0", "t.mid1"))   # positional reads
    assert tuple(ssfa[3][:4]) == ("b1.0", "b1.0", "t.x0", "h.a")
    assert max(r.mask for r in ssfa.values()) < 8 and len(DensePlan.ACTIVITY_STEPS) == 9   # 8 slots, 9 steps
    rpn = _rpn_table()
    assert [tuple(r) for r in rpn.values()] == [("blk0.%d" % i, "blk0.%d" % i, "t.l%d" % (i - 1) if i else "bev", "t.l%d" % i, i, "wino",
                                                 i + 1 if i < 5 else None) for i in range(6)]
    assert _rpn_table(6) and RpnPlan.list_layers(SimpleNamespace(layers=[None] * 6), "bev", {"l0": 0, "l1": 1, "out": 2}, {}) == {}


def test_fill_reach_of_the_ssfa_table():
    table = _ssfa_table()
    for ids, near_fill, coarse_fill, want in SSFA_CASES:
        assert _jobs(table, ids, near_fill, coarse_fill) == want, (sorted(ids), near_fill, coarse_fill)
        assert len(want) <= 12   # sessd_fill_inactive_tiles takes at most 12 jobs


def test_fill_reach_of_a_six_layer_rpn_table():
    assert _jobs(_rpn_table(), range(6)) == RPN_ALL_SIX
