"""tests/partition_model.py against the sources and against itself (no GPU).

- the constants the model's launch geometry depends on are the ones in csrc/spmv.hip, csrc/api.cpp, csrc/colcode.hip:
  a retuned kernel cannot move the operator families off their edges silently;
- every family puts interior_lo where its alignment class says, the lopsided and empty interiors exist;
- the (family, form) table agrees with the builders' rules on every rank and in both halo modes, and every form is
  expected-available on at least one family of every alignment class -- the staged family through the one-launch-with-hole
  path and through the two-launch path;
- the NumPy emulation of the partitioned product passes every comparison of `judge`, and every injected fault is rejected by
  the same `judge` on a stencil family and on a non-stencil family.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import partition_model as pm  # noqa: E402

MODES = ("neighbour", "gather")
CLASSES = ("a256", "a64", "a32", "odd")


def test_constants_are_those_of_the_sources():
    c = pm.source_constants()
    assert c["hole_align"] == pm.HOLE_ALIGN and c["blockptr_align"] == pm.BLOCKPTR_ALIGN
    assert c["slice"] == {pm.SLICE}
    assert c["row_blocks"] == {pm.ROW_BLOCKS}                    # the stream and the staged branch of spmv_plan
    assert c["stage_window"] == {pm.STAGE_WINDOW}
    assert c["one_range"] == tuple(sorted(pm.ONE_RANGE_OPTIONS))
    assert c["staged_family"] == pm.STAGED_FAMILY and c["takes_two_ranges"] and c["delta_guard"]
    assert c["coded_max_row"] == pm.CODED_MAX_ROW and c["code_max"] == pm.CODE_MAX and c["sell_max_pad"] == pm.SELL_MAX_PAD
    assert c["sell_rule"] and c["sell_limits"] and c["try32_rule"] and c["big"]
    assert c["template"] == (pm.TMPL_MAX_LEN, pm.TMPL_MAX, pm.TMPL_LDS_MAX // 1024) and c["template_rule"]
    assert c["split_rule"] and c["interior_launch"] and c["boundary_launch"] and c["ghost_range"]


def test_interior_range_restates_the_kernel():
    # rows 1 and 6 of 8 touch a ghost column: [2, 6); only row 5: [0, 5); rows 3 and 4 (m / 2 = 4): they cross -> empty at 4
    def slab(touching, m=8):
        rowptr = np.arange(m + 1)
        col = np.array([m if i in touching else i for i in range(m)])
        return pm.interior_range(rowptr, col, m)
    assert slab({1, 6}) == (2, 6) and slab({5}) == (0, 5) and slab({2}) == (3, 8) and slab(set()) == (0, 8)
    assert slab({3, 4}) == (4, 4) and slab({0, 7}) == (1, 7)
    assert slab({0}, m=1) == (0, 0)                                            # one row: m / 2 = 0, the row is in the upper half


@pytest.mark.parametrize("fam", pm.FAMILIES, ids=lambda f: f.name)
def test_families_sit_on_their_edges(fam):
    P = pm.partitioned(fam.name)
    assert P.n == fam.starts[-1] and fam.world in (2, 3, 4, 8)
    assert np.all(np.diff(P.rowptr) >= 0) and P.col.min() >= 0 and P.col.max() < P.n
    for s in P.slabs:                                                           # columns increase along a row
        inner = np.ones(s.gcol.size, dtype=bool)
        inner[s.rowptr[:-1][s.lens > 0]] = False
        assert np.all(np.diff(s.gcol.astype(np.int64))[inner[1:]] > 0)
    for mode in MODES:
        ranges = [s.interior(mode) for s in P.slabs]
        if fam.align in CLASSES:
            middle = [(s, r) for s, r in zip(P.slabs, ranges) if 0 < r[0] and r[1] < s.m]
            assert middle, fam.name                                             # a rank with a hole
            for s, (lo, hi) in middle:
                assert hi > lo and pm.align_class(lo) == fam.align, (fam.name, s.rank, lo, hi)
            if fam.stencil:                                                     # rank 0: ghosts only at the bottom; the last rank: only at the top
                assert ranges[0][0] == 0 and ranges[0][1] < P.slabs[0].m
                assert ranges[-1][1] == P.slabs[-1].m and ranges[-1][0] > 0
        elif fam.align == "empty":
            assert all(hi == lo for lo, hi in ranges)
    if fam.kind == "midrow":
        for s in P.slabs:
            info = s.info("neighbour")
            assert info["max_row"] > pm.CODED_MAX_ROW and 30 <= info["mean_row"] <= 90 and info["max_row"] <= 100
            assert pm.predict(info, pm.BASE)["form"] == "Stream"
    if fam.name == "bd_shapes":
        assert [s.m for s in P.slabs] == [40, 1, 300, 130]
    if fam.name == "g7_256":
        assert len({s.m for s in P.slabs}) > 1                                  # gather mode: m < maxm on a rank


def test_world_sizes_and_unsymmetric_values():
    assert {f.world for f in pm.FAMILIES} == {2, 3, 4, 8}
    for name in ("g7_odd", "g27_32", "bd_32"):
        P = pm.partitioned(name)
        import scipy.sparse as sp
        S = sp.csr_matrix((P.val, P.col, P.rowptr), shape=(P.n, P.n))
        assert abs(S - S.T).max() > 0.1


@pytest.mark.parametrize("fam", pm.FAMILIES, ids=lambda f: f.name)
def test_table_agrees_with_the_builders_rules(fam):
    """What spmv_plan and the builders give on every rank, in both halo modes, is what the table says: the wanted form where it
    is marked available, another one -- with a reason -- where it is not."""
    P = pm.partitioned(fam.name)
    tab = pm.table()
    for form, spec in pm.FORMS.items():
        available, reason = tab[(fam.name, form)]
        assert available or reason
        got = {pm.predict(s.info(mode), spec["opts"], form == "template" and s.templates(mode) > 0)["form"] for s in P.slabs for mode in MODES}
        if available:
            assert got == {spec["want"]}, (fam.name, form, got)
        else:                                       # the same fallback on every rank, in both halo modes
            assert spec["want"] not in got and len(got) == 1, (fam.name, form, got)


def _paths(fam, form):
    """The boundary paths the ranks with a hole take under a form: 'hole' (one launch, two ranges) / 'two' (two launches)."""
    P = pm.partitioned(fam.name)
    spec = pm.FORMS[form]
    out = set()
    for mode in MODES:
        for s in P.slabs:
            lo, hi = s.interior(mode)
            if not (0 < lo < hi < s.m):
                continue
            pred = pm.predict(s.info(mode), spec["opts"], form == "template" and s.templates(mode) > 0)
            ls = pm.launches(pred["form"], dict(spec["opts"], overlap_halo=1), lo, hi, s.m, pred["delta_rows"])
            b = [L for L in ls if L["part"] == "boundary"]
            assert ls[0]["part"] == "interior" and ls[0]["ranges"] == [(lo, hi)]
            out.add("hole" if len(b) == 1 and len(b[0]["ranges"]) == 2 else "two")
            assert sorted(r for L in ls for r in L["ranges"]) == [(0, lo), (lo, hi), (hi, s.m)]
    return out


def test_every_form_is_available_in_every_alignment_class():
    tab = pm.table()
    by_family = {}
    for form, spec in pm.FORMS.items():
        for cls in CLASSES:
            fams = [f for f in pm.FAMILIES if f.align == cls and tab[(f.name, form)][0]]
            assert fams, (form, cls)
            for f in fams:
                by_family.setdefault(pm.family_of(spec["want"]), set()).update((cls, p) for p in _paths(f, form))
    for fam in pm.STAGED_FAMILY:                    # the one launch with a hole and the two launches
        assert {p for _, p in by_family[fam]} == {"hole", "two"}, (fam, by_family[fam])
        assert ("a256", "hole") in by_family[fam] and {c for c, p in by_family[fam] if p == "two"} >= {"a64", "a32", "odd"}
    for fam in ("Stream", "Wave", "Template", "Ordered", "Vector"):
        assert {p for _, p in by_family[fam]} == {"two"}
    # the interior launch reads the delta stream where interior_lo is a multiple of the delta block, and not elsewhere
    for name, form, want in (("mid_256", "delta8", True), ("mid_64", "delta8", True), ("g7_odd", "delta8", False), ("g7_32", "delta8", False),
                             ("g7_256", "delta16", True), ("g7_64", "delta16", False)):
        P = pm.partitioned(name)
        s = P.slabs[1]
        lo, hi = s.interior("neighbour")
        pred = pm.predict(s.info("neighbour"), pm.FORMS[form]["opts"])
        ls = pm.launches(pred["form"], dict(pm.FORMS[form]["opts"], overlap_halo=1), lo, hi, s.m, pred["delta_rows"])
        assert ls[0]["delta"] == want, (name, form, lo, pred)


def test_launches_degenerate_ranges():
    o = dict(pm.BASE, overlap_halo=1)
    assert pm.launches("Staged", o, 0, 700, 1000)[1:] == [dict(ranges=[(700, 1000)], part="boundary", delta=False, blockptr=False)]
    assert [L["ranges"] for L in pm.launches("Staged", o, 256, 1000, 1000)] == [[(256, 1000)], [(0, 256)]]
    assert [L["ranges"] for L in pm.launches("Staged", o, 256, 256, 1000)] == [[(0, 1000)]]                  # empty interior: no split
    assert [L["ranges"] for L in pm.launches("Staged", dict(o, overlap_halo=0), 256, 512, 1000)] == [[(0, 1000)]]
    assert [L["ranges"] for L in pm.launches("Staged", o, 256, 512, 1000)] == [[(256, 512)], [(0, 256), (512, 1000)]]
    assert [L["ranges"] for L in pm.launches("Staged", dict(o, spmv_delta=2), 256, 512, 1000)] == [[(256, 512)], [(0, 256)], [(512, 1000)]]
    assert [L["ranges"] for L in pm.launches("Stream", o, 256, 512, 1000)] == [[(256, 512)], [(0, 256)], [(512, 1000)]]
    assert [L["ranges"] for L in pm.launches("Sliced", o, 192, 512, 1000)] == [[(192, 512)], [(0, 192)], [(512, 1000)]]


_INPUTS = {}


def _inputs(name):
    if name not in _INPUTS:
        _INPUTS[name] = pm.make_inputs(pm.partitioned(name))
    return _INPUTS[name]


def _judge(name, form, mode, overlap=1, fault=None):
    P = pm.partitioned(name)
    want = pm.FORMS[form]["want"]
    outs = pm.emulate_case(P, _inputs(name), form, mode, overlap, fault)
    return pm.judge(P, _inputs(name), outs, want)


@pytest.mark.parametrize("fam", pm.FAMILIES, ids=lambda f: f.name)
def test_inputs_and_emulation_pass_every_comparison(fam):
    P = pm.partitioned(fam.name)
    inp = _inputs(fam.name)
    assert inp["cond"] >= 1e10 / 2                                          # the ill-conditioned dotw really is
    i, j = P.starts[1] - 1, P.starts[-2]
    assert abs(inp["w_ill"][i] * inp["y_ref"][0][i]) > 1e6 * abs(pm.er.exact_dot(inp["w_ill"], inp["y_ref"][0])) or \
        abs(inp["w_ill"][j] * inp["y_ref"][0][j]) > 1e6 * abs(pm.er.exact_dot(inp["w_ill"], inp["y_ref"][0]))
    for k in (2, 3):                                                        # the special vectors: some rows are not finite, most are
        bad = ~np.isfinite(inp["y_ref"][k])
        assert 0 < bad.sum() < P.n // 4
        (ci, cn) = pm.special_columns(P)[k - 2]
        rows = np.union1d(P.has_column(ci), P.has_column(cn))
        assert np.array_equal(np.flatnonzero(bad), rows)                   # exactly the rows that reference the columns
        def rank_of(g):
            return int(np.searchsorted(P.starts, g, side="right") - 1)
        private = pm.special_columns(P)[2]
        for c in (ci, cn):
            readers = {rank_of(r) for r in P.has_column(c)}
            if k == 2:
                assert readers <= {rank_of(c)} or not private           # owned: nobody else reads it
            else:
                assert readers - {rank_of(c)}                            # a ghost on a neighbour
    tab = pm.table()
    forms = [f for f in ("staged", "sliced", "sliced32", "stream64", "delta8", "wave", "vector", "template") if tab[(fam.name, f)][0]]
    for form in forms:
        for mode in MODES:
            for overlap in (1, 0):
                assert _judge(fam.name, form, mode, overlap) == [], (fam.name, form, mode, overlap)


# fault -> [(stencil family, form, halo mode), (non-stencil family, form, halo mode)]
REJECTIONS = {
    "hole_twice": [("g7_256", "staged", "neighbour"), ("bd_256", "staged", "neighbour")],
    "hole_never": [("g27_64", "coded8", "gather"), ("mid_64", "stream32_vec2", "neighbour")],
    "first_range_overrun": [("g7_odd", "sliced", "neighbour"), ("bd_odd", "coded16", "gather")],
    "second_range_at_hole_lo": [("g7_256", "sliced", "neighbour"), ("bd_256", "sliced32", "gather")],
    "ghost_off_by_stride": [("g27_32", "coded8", "gather"), ("bd_64", "wave", "gather")],
    "stale_ghost": [("dg_poisson_odd", "template", "neighbour"), ("mid_256", "delta16", "gather")],
    "dropped_boundary_partial": [("g7_64", "stream256", "neighbour"), ("bd_32", "sliced", "neighbour")],
    "padding_as_entry": [("g27_256", "sliced", "neighbour"), ("bd_32", "sliced", "gather")],
    "delta_from_launch_row": [("g7_64", "delta8", "neighbour"), ("mid_64", "delta8", "neighbour")],
    "slice_by_tid": [("g7_32", "sliced", "neighbour"), ("bd_odd", "sliced32", "neighbour")],
}


@pytest.mark.parametrize("fault", pm.FAULTS)
def test_every_injected_fault_is_rejected(fault):
    cases = REJECTIONS[fault]
    assert {pm.FAMILY[c[0]].stencil for c in cases} == {True, False}
    for name, form, mode in cases:
        assert pm.table()[(name, form)][0]
        assert _judge(name, form, mode) == [], (name, form, mode)                  # the same case without the fault passes
        fails = _judge(name, form, mode, fault=fault)
        assert fails, (fault, name, form, mode)


def test_judge_rejects_a_silent_fallback_and_differing_ranks():
    P, inp = pm.partitioned("g7_256"), _inputs("g7_256")
    outs = pm.emulate_case(P, inp, "staged", "neighbour", 1)
    assert pm.judge(P, inp, outs, "Sliced") and pm.judge(P, inp, outs, "Staged") == []
    outs[1]["dot"] = np.nextafter(outs[1]["dot"], np.inf)
    assert any("same bits" in f for f in pm.judge(P, inp, outs, "Staged"))
    outs = pm.emulate_case(P, inp, "staged", "neighbour", 1)
    outs[2]["y_dot"][1] = outs[2]["y_dot"][1].copy()
    outs[2]["y_dot"][1][5] *= 2
    assert any("fused" in f for f in pm.judge(P, inp, outs, "Staged"))
    # the vector form's row bound: a row off by a few ulps passes, a dropped entry does not
    outs = pm.emulate_case(P, inp, "vector", "neighbour", 1)
    assert pm.judge(P, inp, outs, "Vector", exact_y=False) == []
    outs[0]["y"][1] = outs[0]["y"][1] + inp["xs"][1][:P.slabs[0].m] * 1e-3
    assert pm.judge(P, inp, outs, "Vector", exact_y=False)
