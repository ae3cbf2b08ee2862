"""tests/spmm_model.py without a GPU: its constants against the sources, the group orders and walks of every case of the GPU
table (every group exactly once; the edge walks the table is there for are shown to be in it), the threshold families on the
intended side of each builder rule from the model's own numbers, and the record checker: sound records pass, every hand-made
corruption is rejected."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spmm_model as sm  # noqa: E402


def test_model_constants_equal_the_sources():
    src = sm.constants_in_sources()
    assert src == {k: getattr(sm, k) for k in src}, src
    # CAP = 44 KiB / 16 L of the window kernel, the flag limits the issue names
    assert [sm.win_shape(L)["CAP"] for L in (2, 4, 8, 16, 32)] == [1408, 704, 352, 176, 88]
    assert [sm.win_shape(L)["ENTRIES"] for L in (2, 4, 8, 16, 32)] == [4096, 2048, 1024, 512, 256]


def test_option_table_matches_the_library_defaults():
    text = open(os.path.join(sm._CSRC, "khip_internal.hpp")).read()
    import re
    for k, v in sm.OPTION_DEFAULTS.items():
        m = re.search(r"\bint %s = (-?\d+);" % k, text)
        assert m and int(m.group(1)) == v, (k, v, m and m.group(1))


# ---- orders --------------------------------------------------------------------------------------------------------------------
def _order_of(opname, **kw):
    op = sm.get_op(opname)
    b = sm.tile_build(op, sm.options(**kw))
    assert b["state"] == 1, b["why"]
    return op, b


@pytest.mark.parametrize("opname,kw,kind", [
    ("band72", dict(spmm_tile_slide=0), "identity"), ("band72", dict(spmm_tile_slide=7), "identity"),
    ("g27", dict(spmm_tile_slide=0), "pencil"), ("g27_pen", dict(spmm_tile_slide=0, spmm_tile_pencil=4), "pencil"),
    ("g27", dict(spmm_tile_slide=1), "runs"), ("g27", dict(spmm_tile_slide=3), "runs"), ("g27", dict(spmm_tile_slide=2, spmm_tile_shape=4), "runs"),
    ("plane", dict(spmm_tile_slide=3), "runs"), ("plane", dict(spmm_tile_slide=0), "pencil"), ("g7", dict(spmm_tile_shape=4), "runs")])
def test_every_row_lands_in_exactly_one_group_slot(opname, kw, kind):
    op, b = _order_of(opname, **kw)
    rows = b["rows"]
    assert (b["order"].kind if b["order"].s1 else "identity") == kind
    real = rows[rows >= 0]
    assert np.array_equal(np.sort(real), np.arange(op.m))
    assert rows.shape == (b["groups"], 32) and (b["run_len"] == 0 or b["groups"] == b["runs"] * b["run_len"])


def test_orders_hand_counted():
    # 13 x 10 x 9, 4 x 4 x 2 tiles: 4 x 3 x 5 tiles; runs of 3 along k: 5 tiles = 2 pieces of 3 -> 6 per line, one padding group per line
    op, b = _order_of("g27", spmm_tile_slide=3)
    o = b["order"]
    assert (o.gi, o.gj, o.gk, o.run_len, o.run_pieces) == (4, 3, 5, 3, 2) and b["runs"] == 24 and b["groups"] == 72
    assert sum(1 for g in range(72) if np.all(b["rows"][g] < 0)) == 12
    # whole lines (slide = 1): 5 groups per run, no padding; default (-1): runs of <= 27, the same here
    assert _order_of("g27", spmm_tile_slide=1)[1]["run_len"] == 5 == _order_of("g27")[1]["run_len"]
    # slide = 7 >= the line: whole lines; slide = 2: 3 pieces of 2
    assert _order_of("g27", spmm_tile_slide=7)[1]["run_len"] == 5 and _order_of("g27", spmm_tile_slide=2)[1]["run_len"] == 2
    # identity order: slide = 1 means runs of 64 groups; 1000 rows = 32 groups are padded to one run of 64
    b = _order_of("band72", spmm_tile_slide=1)[1]
    assert (b["run_len"], b["runs"], b["groups"]) == (64, 1, 64)
    b = _order_of("band72", spmm_tile_slide=7)[1]
    assert (b["run_len"], b["runs"], b["groups"]) == (7, 5, 35)
    # pencils of 4 tile rows on gj = 6: a full pencil of 4 and a last one of 2
    op, b = _order_of("g27_pen", spmm_tile_slide=0, spmm_tile_pencil=4)
    o = b["order"]
    assert (o.gi, o.gj, o.gk, o.pj) == (3, 6, 3, 4) and o.gj % o.pj == 2
    # a single plane: 8 x 4 x 1 tiles, runs along j
    op, b = _order_of("plane", spmm_tile_slide=1)
    o = b["order"]
    assert (o.bi, o.bj, o.bk, o.gi, o.gj, o.gk, o.run_len) == (8, 4, 1, 3, 4, 1, 4) and b["runs"] == 3


def test_plane_detection_hand_counted():
    assert sm.get_op("g27").planes() == (13, 130) and sm.get_op("g7").planes() == (11, 99) and sm.get_op("plane").planes() == (19, 19)
    assert sm.get_op("band72").planes()[0] == 0 and sm.get_op("band_m100").planes() == (0, 0)
    # a line distance below 5 cannot be reported: offsets 1 and 4 stay in one cluster (4 <= 2 x 1 + 2), 1 and 5 do not
    assert sm.get_op("g_line4").planes()[0] != 4 and sm.get_op("g_line5").planes() == (5, 45)
    # ... so the rule's own edge is held on the rule
    assert not sm.grid_ok_of(1000, 3, 0) and sm.grid_ok_of(1000, 4, 0) and sm.grid_ok_of(1000, 4, 4)
    assert not sm.grid_ok_of(1000, 8, 24) and sm.grid_ok_of(1000, 8, 32) and not sm.grid_ok_of(1000, 8, 30) and not sm.grid_ok_of(8, 8, 0)


# ---- walks -----------------------------------------------------------------------------------------------------------------------
_WALKED = []


def _walked():
    """(case, launch, walk, stats, operator) of every case with a forced grid; a tile_dist case once per rank, on its slab."""
    if not _WALKED:
        for c in sm.cases():
            for op in (sm.case_slabs(c) if c.group == "tile_dist" else [None]):
                ln, w, st = sm.case_walk(c, op)
                if w is not None:
                    _WALKED.append((c, ln, w, st, op if op is not None else sm.get_op(c.op)))
    return _WALKED


def test_every_walk_of_the_gpu_table_visits_every_group_exactly_once():
    n = 0
    for c, ln, w, st, op in _walked():
        if ln["family"] in ("tile1", "tile2"):
            total = sm.tile_build(op, c.options)["groups"]
        elif ln["family"] == "window":
            total = sm.window_build(op, ln["L"])["all_groups"]
        else:
            total = (op.m + sm.kBlock // ln["L"] - 1) // (sm.kBlock // ln["L"])
        assert st["visits"] == list(range(total)), (c.name, ln["family"], ln["grid"], len(st["visits"]), total)
        n += 1
    assert n >= 150


FORMS8 = ("tile1-plain", "tile1-dbuf", "tile1-slide", "tile2-plain", "tile2-slide", "tile2-ahead", "window", "window-sweep")


def loop_depths():
    """Per kernel form: the largest number of groups (and runs) one workgroup takes over the cases of the GPU table."""
    depth = {f: [0, 0] for f in FORMS8}
    for c, ln, w, st, op in _walked():
        f = sm.form_name(ln)
        if f in depth:
            depth[f][0] = max(depth[f][0], st["max_groups"])
            depth[f][1] = max(depth[f][1], st["max_runs"])
    return depth


def test_the_table_reaches_the_loops_it_was_written_for():
    depth = loop_depths()
    print(depth)
    for f in FORMS8:
        assert depth[f][0] >= 3, (f, depth[f])
    for f in ("tile1-slide", "tile2-slide", "tile2-ahead"):
        assert depth[f][1] >= 3, (f, depth[f])                    # rr += G twice and more
    walked = _walked()
    tile = [(c, ln, w, st, op) for c, ln, w, st, op in walked if ln["family"] in ("tile1", "tile2")]
    # an XCD with no group, and an XCD with no run (eighths on a grid that is a multiple of 8)
    assert any(st["empty_xcds"] and ln["run_len"] == 0 and ln["grid"] % 8 == 0 and not (ln["xcd"] & 8) for c, ln, w, st, op in tile)
    assert any(st["empty_xcds"] and ln["run_len"] > 0 and ln["grid"] % 8 == 0 for c, ln, w, st, op in tile)
    # the forced grid of 67 became 64 (&= ~7) on all six forms; the chunked front and the round-robin order run on the two-wave kernel
    assert {sm.form_name(ln) for c, ln, w, st, op in tile if c.options["spmm_tile_grid"] == 67 and ln["grid"] == 64} == set(FORMS8[:6])
    assert {ln["xcd"] for c, ln, w, st, op in tile if ln["family"] == "tile2" and ln["grid"] % 8 == 0} == {0, 8, 128}
    assert {ln["xcd"] for c, ln, w, st, op in tile if ln["family"] == "tile1" and ln["grid"] % 8 == 0} == {0, 8, 128}
    # groups padded to whole runs; a last pencil narrower than pj
    assert any(ln["run_len"] > 0 and np.any(np.all(sm.tile_build(op, c.options)["rows"] < 0, axis=1)) for c, ln, w, st, op in tile)
    pens = [sm.tile_build(op, c.options)["order"] for c, ln, w, st, op in tile if c.want.get("narrow_pencil")]
    assert pens and all(o.kind == "pencil" and o.gj % o.pj != 0 for o in pens)
    # the window kernel's plane sweep meets padding slots of phys(); both unrolled set roles (an odd and an even trip count)
    win = [(c, ln, w, st, op) for c, ln, w, st, op in walked if ln["family"] == "window"]
    assert any(ln["sweep_S"] > 0 and st["padding"] > 0 for c, ln, w, st, op in win)
    trips = {len(s) % 2 for c, ln, w, st, op in win for s in w if len(s) >= 3}
    assert trips == {0, 1}
    assert {ln["L"] for c, ln, w, st, op in win} == {2, 4, 8, 16} and {ln["pow2"] for c, ln, w, st, op in win} == {0, 1}


def test_walks_hand_counted():
    # eighths: 60 groups, 16 workgroups: XCD x walks 8 x .. 8 x + 7 (the last one 56 .. 59) with two workgroups side by side
    w = sm.walk_tile("tile2", 60, 0, 0, 16, 0)
    assert w[0] == [0, 2, 4, 6] and w[8] == [1, 3, 5, 7] and w[7] == [56, 58] and w[15] == [57, 59]
    # round-robin; the chunked front (two-wave kernel only: the one-wave kernel keeps the eighths under bit 128)
    assert sm.walk_tile("tile2", 60, 0, 0, 16, 8)[3] == [3, 19, 35, 51]
    assert sm.walk_tile("tile2", 60, 0, 0, 16, 128)[1] == [2, 18, 34, 50] and sm.walk_tile("tile2", 60, 0, 0, 16, 128)[9] == [3, 19, 35, 51]
    assert sm.walk_tile("tile1", 60, 0, 0, 16, 128) == sm.walk_tile("tile1", 60, 0, 0, 16, 0) == w
    # runs: 24 runs of 3, 3 workgroups: workgroup 1 takes the runs 1, 4, 7, ...
    w = sm.walk_tile("tile1", 72, 24, 3, 3, 0)
    assert w[1][:7] == [3, 4, 5, 12, 13, 14, 21] and len(w[1]) == 24
    # runs by eighths: 3 runs per XCD
    w = sm.walk_tile("tile2", 72, 24, 3, 8, 0)
    assert w[2] == [18, 19, 20, 21, 22, 23, 24, 25, 26]
    # the one-wave kernel walks runs by eighths whatever the order bits say; the two-wave kernel follows them
    assert sm.walk_tile("tile1", 72, 24, 3, 8, 8) == w and sm.walk_tile("tile2", 72, 24, 3, 8, 8)[2] == [6, 7, 8, 30, 31, 32, 54, 55, 56]
    # window kernel, sweep: S = 20 groups per plane, W = 2, 64 workgroups (8 per XCD): 2 columns per XCD, the second all padding
    w = sm.walk_window(141, 64, 20, 2, 8, 2)
    assert w[0] == [0, 80, 16, 96] and w[8][:2] == [1, 81] and w[1][0] == 2 and w[2] == [4, 84, None, None]


# ---- the threshold families --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sm.cases(), ids=lambda c: c.group + "-" + c.name)
def test_case_lands_where_it_was_meant_to(case):
    if case.group == "tile_dist":
        return _dist_case_lands(case)
    op = sm.get_op(case.op)
    ln, w, st = sm.case_walk(case)
    want = dict(case.want)
    b = sm.tile_build(op, case.options) if ln["tile_built"] else None
    assert ln["error"] is None
    for k in ("family", "dbuf", "ahead", "NL", "L", "launches", "nt"):
        if want.get(k) is not None and k in want:
            assert ln[k] == want[k], (k, ln[k], want[k])
    if "slide" in want:
        assert (ln["run_len"] > 0) == want["slide"]
    if "form" in want:
        assert sm.form_name(ln) == want["form"]
    for k in ("state", "cap", "cap0", "run_len", "direct", "line_rows", "plane_rows", "grid_ok", "reuse"):
        if k in want:
            assert b is not None and b.get(k) == want[k], (k, b.get(k), want[k], b["why"])
    if "order" in want:
        assert b["state"] == 1 and b["order"].kind == want["order"]
    if "direct_min" in want:
        assert b["direct"] >= want["direct_min"]
    if want.get("family_not_tile"):
        assert ln["family"] in ("window", "spmm2_kernel")
    if case.group in ("tile_loops", "tile_chain", "window"):
        assert (w is None) == bool(want.get("no_grid")), "forced grid"
    wb = sm.window_build(op, ln["L"]) if ln["win_L"] else None
    if want.get("by_columns"):
        assert wb["by_columns"] >= 1 and wb["by_entries"] == 0 and 0 < np.nonzero(wb["flags"])[0][0] < wb["all_groups"] - 1
    if want.get("by_entries"):
        assert wb["by_entries"] >= 1 and wb["by_columns"] == 0 and 0 < np.nonzero(wb["flags"])[0][0] < wb["all_groups"] - 1
    if want.get("win_refused"):
        assert ln["win_L"] < 0
    if want.get("sweep"):
        assert ln["sweep_S"] > 0
    if want.get("padding"):
        assert st["padding"] > 0


def _dist_case_lands(case):
    slabs = sm.case_slabs(case)
    assert len(slabs) == case.want["world"] and sum(s.m for s in slabs) == sm.get_op(case.op).m
    for rank, slab in enumerate(slabs):
        ln, w, st = sm.case_walk(case, slab)
        assert ln["error"] is None and w is not None and ln["dist"] == 1 and slab.ghosts.size > 0
        assert ln["family"] == case.want.get("family", ln["family"]) and (ln["family"] == "window" or sm.tile_build(slab, case.options)["state"] == 1)
        assert np.array_equal(np.where(slab.col < slab.m, slab.col + slab.r0, slab.ghosts[np.maximum(slab.col - slab.m, 0)]), slab.global_cols)
        if rank > 0:
            assert slab.planes()[0] == 0           # global columns against local rows: one cluster of offsets, no grid on this rank
    if case.want.get("long_ghost"):                # a flagged group holds a long row with a ghost column
        hit = 0
        for slab in slabs:
            b = sm.tile_build(slab, case.options)
            for g in range(b["groups"]):
                if b["cols"][g] is None:
                    rr = b["rows"][g][b["rows"][g] >= 0]
                    hit += any(slab.lens[r] > 32 and slab.col[slab.rowptr[r]:slab.rowptr[r + 1]].max() >= slab.m for r in rr)
        assert hit >= 1


def test_threshold_families_sit_next_to_their_rule():
    tb = lambda name, **kw: sm.tile_build(sm.get_op(name), sm.options(**kw))
    # 1.5 references per column: exactly on it (kept: the refusal is <), one column more (refused)
    assert tb("reuse_at")["reuse"] == 1.5 and tb("reuse_below")["state"] == -1 and 1.49 < tb("reuse_below")["score"] < 1.5
    # the 99 % window: the multiple of 8 that holds the widest group, 64 / 72 from 64 / 72 distinct columns
    for name, cap in (("band64", 64), ("band72", 72), ("band128", 128), ("band136", 136), ("band192", 192), ("band200", 200), ("band256", 256)):
        b = tb(name, spmm_tile_slide=0)
        assert b["cap"] == cap and int(b["counts"].max()) == cap and b["direct"] == 0, (name, b["cap"])
    # ... and the percentage itself: 200 groups, 2 widened to 72 columns sit exactly on 100 fit >= 99 groups (the window stays at the
    # band's 40 slots, both go down the direct path), 3 are below it (the window grows to take them); 73 columns: the next octet
    b = tb("fit99_two", spmm_tile_slide=0)
    assert (b["groups"], b["cap"], b["direct"]) == (200, 40, 2) and 100 * 198 == sm.FIT_PERCENT * 200
    assert sorted(int(c) for c in b["counts"] if c > 40) == [72, 72] and int(np.sum(b["counts"] <= 40)) == 198
    b = tb("fit99_three", spmm_tile_slide=0)
    assert (b["groups"], b["cap"], b["direct"]) == (200, 72, 0) and 100 * 197 < sm.FIT_PERCENT * 200 and int(np.sum(b["counts"] == 72)) == 3
    b = tb("fit99_three73", spmm_tile_slide=0)
    assert (b["groups"], b["cap"], b["direct"]) == (200, 80, 0) and int(np.sum(b["counts"] == 73)) == 3
    # a flagged group is outside the 99 %: with 4 in 524 groups the window stays at the band's 56 columns
    b = tb("band_chain", spmm_tile_slide=4)
    assert (b["cap"], b["direct"], b["groups"]) == (56, 4, 524) and 99 * b["groups"] <= 100 * (b["groups"] - 4)
    # the ceiling: half of the groups over 256 columns is kept (2 fit < groups is the refusal), one more is refused
    b = tb("band_over_fit", spmm_tile_slide=0)
    assert (b["state"], b["cap"], b["direct"], b["fit"], b["groups"]) == (1, 256, 16, 16, 32)
    b = tb("band_over_refuse", spmm_tile_slide=0)
    assert b["state"] == -1 and (b["fit"], b["ngroups"]) == (15, 32)
    # look-ahead: 168 + 84 = 252 <= 256 (rounded up to 256), 176 + 88 > 256; 72 + 36 = 108 rounds up to 112
    assert (tb("band168", spmm_tile_slide=4, spmm_tile_ahead=1)["cap"], tb("band176", spmm_tile_slide=4, spmm_tile_ahead=1)["ahead"]) == (256, 0)
    assert tb("band72", spmm_tile_slide=4, spmm_tile_ahead=1)["cap"] == 112
    # dbuf by rule at p = 16: 2 x 104 x 128 B = 26 KiB exactly, 112 is over
    assert 2 * 104 * 128 == sm.DBUF_BYTES < 2 * 112 * 128
    # the window builder at L = 4: 768 columns against CAP = 704, 2112 entries against 2048; 7 of 12 flagged refuses, 6 keeps
    W = sm.win_shape(4)
    wb = sm.window_build(sm.get_op("win_cols"), 4)
    assert wb["win_L"] == 4 and wb["all_flagged"] == 1 and wb["by_columns"] == 1 and W["CAP"] == 704
    wb = sm.window_build(sm.get_op("win_entries"), 4)
    assert wb["win_L"] == 4 and wb["all_flagged"] == 1 and wb["by_entries"] == 1 and wb["by_columns"] == 0
    assert sm.window_build(sm.get_op("win_refuse_flag"), 4)["all_flagged"] == 7 and sm.window_build(sm.get_op("win_refuse_flag"), 4)["win_L"] == -4
    assert sm.window_build(sm.get_op("win_half_flag"), 4)["all_flagged"] == 6 and sm.window_build(sm.get_op("win_half_flag"), 4)["win_L"] == 4
    keep, ref = sm.get_op("win_keep_reuse"), sm.get_op("win_refuse_reuse")
    assert 2 * keep.nnz == 3 * sm.window_build(keep, 4)["total"] and sm.window_build(keep, 4)["win_L"] == 4
    assert 2 * ref.nnz == 3 * sm.window_build(ref, 4)["total"] - 3 and sm.window_build(ref, 4)["win_L"] == -4


def test_chain_operators_place_their_flagged_groups():
    for name, sl in (("band_chain", 4), ("g7_chain", 8)):
        op = sm.get_op(name)
        b = sm.tile_build(op, sm.options(spmm_tile_slide=sl, spmm_tile_ahead=1))
        assert b["state"] == 1 and b["ahead"] == 1 and b["run_len"] == sl and b["direct"] == 4
        flagged = [g for g in range(b["groups"]) if b["counts"][g] < 0 or b["counts"][g] > b["cap"]]
        pos = sorted(g % sl for g in flagged)
        assert 0 in pos and sl - 1 in pos and any(0 < q < sl - 1 for q in pos)
        assert any(g + 1 in flagged and (g + 1) % sl != 0 for g in flagged)                    # two in a row inside one run
        assert any(np.all(b["rows"][g] < 0) for g in range(b["groups"]))                       # a run-padding group
        if name == "band_chain":
            assert any(np.all(b["rows"][g] >= 0) and b["counts"][g] == 0 for g in range(b["groups"]))   # a group of empty rows
    assert sm.get_op("band_chain").lens[-1] == 0
    assert any(b is None for b in sm.tile_build(sm.get_op("band_chain"), sm.options(spmm_tile_slide=4))["cols"])
    wide = [c for c in sm.tile_build(sm.get_op("band_chain"), sm.options(spmm_tile_slide=4))["cols"] if c is not None and len(c) > 256]
    assert len(wide) == 1                                                                       # ... and one flagged by its columns


# ---- the record checker ------------------------------------------------------------------------------------------------------
def _records(opname, ahead_tight=False, **kw):
    op = sm.get_op(opname)
    b = sm.tile_build(op, sm.options(**kw))
    assert b["state"] == 1
    meta, dl = sm.reference_records(op, b, ahead=1 if ahead_tight else None)
    return op, b, meta, dl


@pytest.mark.parametrize("opname,kw", [("g27", dict(spmm_tile_slide=0)), ("g27", dict(spmm_tile_slide=3)),
                                       ("g27", dict(spmm_tile_slide=3, spmm_tile_ahead=1)), ("band72", dict(spmm_tile_slide=4, spmm_tile_ahead=1)),
                                       ("band_chain", dict(spmm_tile_slide=4, spmm_tile_ahead=1)), ("g7_chain", dict(spmm_tile_slide=8)),
                                       ("band_over_fit", dict(spmm_tile_slide=0))])
def test_checker_accepts_sound_records(opname, kw):
    op, b, meta, dl = _records(opname, **kw)
    assert sm.check_records(op, meta, b["cap"], b["run_len"], dl) == []
    if b["ahead"]:
        desc = sm.split_records(meta, b["cap"])[0]
        assert int(desc[:, 3, 3].sum()) > 0                         # look-ahead groups exist in what was checked


def _desc_view(meta):
    return meta[:, :sm.kTileDescBytes].view(np.int32).reshape(meta.shape[0], 32, 4)        # a writable view of the descriptors


def test_checker_rejects_hand_corrupted_records():
    op, b, meta, dl = _records("g27", spmm_tile_slide=3, spmm_tile_ahead=1)
    cap, rl = b["cap"], b["run_len"]
    ok = lambda m, d=dl: sm.check_records(op, m, cap, rl, d)
    assert ok(meta) == []
    off = sm.kTileDescBytes + 4 * cap
    # a wrong slot byte: entry 0 of row slot 0 of group 1 points at the slot of another column
    bad = meta.copy()
    lst = sm.split_records(bad, cap)[1]
    s0 = int(bad[1, off])
    other = next(q for q in range(cap) if lst[1, q] != lst[1, s0])
    bad[1, off] = other
    assert any("slot %d" % other in f for f in ok(bad)), ok(bad)
    # a missing mask bit at a chain start (group 0 is the first of a run): the octet of a slot it reads
    bad = meta.copy()
    d = _desc_view(bad)
    d[0, 2, 3] &= ~(1 << (int(bad[0, off]) >> 3))
    assert any("group 0" in f and ("misses an octet" in f or "sliding window holds" in f) for f in ok(bad)), ok(bad)
    # ... and inside a chain: a new column's octet not copied leaves the old column in its slot
    desc, lst, slots = sm.split_records(meta, cap)
    g = next(g for g in range(1, meta.shape[0]) if g % rl and desc[g, 1, 3] == 0 and desc[g - 1, 1, 3] == 0 and desc[g, 2, 3] != 0 and desc[g, 0, 3] > 0)
    bad = meta.copy()
    _desc_view(bad)[g, 2, 3] = 0
    assert any("group %d: sliding window holds" % g in f for f in ok(bad)), ok(bad)
    # a row listed twice (and so another one missing)
    bad = meta.copy()
    d = _desc_view(bad)
    d[2, 5, 0] = d[2, 4, 0]
    assert any("listed" in f for f in ok(bad)), ok(bad)
    # first entry / length of a row slot
    bad = meta.copy()
    _desc_view(bad)[2, 4, 1] += 1
    assert any("first entry" in f for f in ok(bad))
    bad = meta.copy()
    _desc_view(bad)[2, 4, 2] -= 1
    assert any("length" in f for f in ok(bad))
    # aux words: distinct columns, flag; a list entry that is no column; the direct list
    bad = meta.copy()
    _desc_view(bad)[3, 0, 3] += 1
    assert any("aux[0]" in f for f in ok(bad))
    bad = meta.copy()
    _desc_view(bad)[3, 1, 3] = 1
    assert any("flag" in f for f in ok(bad))
    bad = meta.copy()
    bad[4, sm.kTileDescBytes:sm.kTileDescBytes + 4] = np.array([op.n], dtype=np.int32).view(np.uint8)
    assert any("valid column" in f for f in ok(bad))
    assert any("direct list" in f for f in ok(meta, np.array([3], dtype=np.int32)))
    # records without runs must carry the full mask
    op2, b2, meta2, dl2 = _records("g27", spmm_tile_slide=0)
    assert sm.check_records(op2, meta2, b2["cap"], 0, dl2) == []
    bad = meta2.copy()
    _desc_view(bad)[1, 2, 3] = 1
    assert any("mask" in f for f in sm.check_records(op2, bad, b2["cap"], 0, dl2))


def test_checker_rejects_a_look_flag_on_a_slot_the_predecessor_reads():
    # a window with no room to spare: the groups whose new columns had to take slots their predecessor reads carry look = 0
    op = sm.get_op("g27")
    b = sm.tile_build(op, sm.options(spmm_tile_slide=3))
    meta, dl = sm.reference_records(op, b, ahead=1)
    cap, rl = b["cap"], b["run_len"]
    assert sm.check_records(op, meta, cap, rl, dl) == []
    desc = sm.split_records(meta, cap)[0]
    cands = [g for g in range(meta.shape[0]) if g % rl and desc[g, 3, 3] == 0 and desc[g, 0, 3] > 0 and desc[g - 1, 0, 3] > 0 and desc[g, 2, 3] != 0]
    assert cands
    hit = 0
    for g in cands:
        bad = meta.copy()
        _desc_view(bad)[g, 3, 3] = 1
        f = sm.check_records(op, bad, cap, rl, dl)
        hit += any("look-ahead copy changes slot" in x and "group %d" % g in x for x in f)
    assert hit >= 1 and hit == len(cands)       # the builder gave look = 0 only where a slot of the predecessor is overwritten
    # ... and at the start of a chain
    bad = meta.copy()
    _desc_view(bad)[0, 3, 3] = 1
    assert any("start of a chain" in x for x in sm.check_records(op, bad, cap, rl, dl))


def test_form_comparisons_reject_a_wrong_field():
    op = sm.get_op("g27")
    opts = sm.options(spmm_tile=2, spmm_tile_slide=3, spmm_tile_ahead=1, spmm_tile_grid=67)
    want = sm.launch(op, opts, 16)
    assert want["family"] == "tile2" and want["ahead"] == 1 and want["grid"] == 24 and sm.launch_failures(want, dict(want)) == []
    for k in sm.LAUNCH_FIELDS + ("grid", "lds"):
        got = dict(want)
        got[k] = "tile1" if k == "family" else want[k] + 1
        assert sm.launch_failures(want, got), k
    b = sm.tile_build(op, opts)
    meta, dl = sm.reference_records(op, b)
    got = dict({k: b[k] for k in sm.BUILD_FIELDS}, reuse=b["reuse"], meta=meta)
    assert sm.build_failures(b, got) == []
    for k in sm.BUILD_FIELDS + ("reuse",):
        assert sm.build_failures(b, dict(got, **{k: got[k] + 1})), k
    swapped = meta.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    assert sm.build_failures(b, dict(got, meta=swapped))          # the same rows in another group order


# ---- the judge -----------------------------------------------------------------------------------------------------------------
def test_serial_product_and_bit_comparison():
    op = sm.get_op("band_m100")
    X, Xs = sm.inputs(op, 4)
    ref = np.zeros((op.m, 4))
    with np.errstate(all="ignore"):
        for i in range(op.m):
            for q in range(op.rowptr[i], op.rowptr[i + 1]):
                ref[i] = ref[i] + op.val[q] * Xs[op.col[q]]
    assert sm.same_bits(sm.serial_spmm(op, Xs), ref) and np.isnan(ref).any() and np.isinf(ref).any()
    assert sm.same_bits(np.array([np.nan, 0.0]), np.array([np.nan, 0.0])) and not sm.same_bits(np.array([0.0]), np.array([-0.0]))
    # the judge sees: a wrong bit, a negative zero in a padding row, an unwritten row (NaN prefill)
    Y = sm.y_prefill(op.m, 4)
    Y[:op.m] = sm.serial_spmm(op, X)
    assert sm.judge_y(op, X, Y.ravel(), "t") == []
    for i, j, v in ((3, 1, None), (op.m + 2, 0, -0.0), (50, 2, np.nan)):
        Z = Y.copy()
        Z[i, j] = np.nextafter(Z[i, j], 9.0) if v is None else v
        assert sm.judge_y(op, X, Z.ravel(), "t"), (i, j)
    # the non-finite twin keeps the structure and puts Inf / NaN at last entries, after short rows and at the matrix end
    nf = sm.nonfinite_values(sm.get_op("band72"))
    o = sm.get_op("band72")
    assert np.array_equal(nf.col, o.col) and not np.isfinite(nf.val[-1]) and not np.isfinite(nf.val[o.rowptr[1] - 1])
    assert np.count_nonzero(~np.isfinite(nf.val)) >= 40
