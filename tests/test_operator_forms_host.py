"""Host checks of tests/operator_forms_model.py, the model behind tests/test_gpu_operator_forms_exact.py: its constants are the
sources', its table states a form for every case and the model predicts that form, the coverage condition holds (both sides of
every builder and plan threshold, every sell_head_words value of modes 0, 1, 4, 5, uniform and offset layouts of every mode), the
NumPy emulation of every case passes the comparison the GPU file uses, and every injected fault is rejected by it.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import operator_forms_model as fm  # noqa: E402
import partition_model as pm  # noqa: E402


def test_constants_equal_the_sources():
    got = fm.forms_source_constants()
    assert got == fm.EXPECTED_SOURCE_CONSTANTS, {k: (got[k], v) for k, v in fm.EXPECTED_SOURCE_CONSTANTS.items() if got.get(k) != v}
    # ... and those restated from partition_model are still pinned there
    sc = pm.source_constants()
    assert sc["code_max"] == fm.CODE_MAX and sc["sell_max_pad"] == fm.SELL_MAX_PAD and sc["coded_max_row"] == fm.CODED_MAX_ROW
    assert sc["template"] == (fm.TMPL_MAX_LEN, fm.TMPL_MAX, fm.TMPL_LDS_MAX // 1024) and sc["stage_window"] == {fm.PLAN_WINDOW}


def test_head_words_are_the_inverse_of_the_units():
    """sell_head_words takes the units of a slice apart again: for every longest row 1 .. 64 (mode 3: 1 .. 8) the value words left
    are the row length, rounded up to an even count in the pair layouts."""
    for mode in range(6):
        for L in range(1, (8 if mode in (2, 3) else 64) + 1):
            T = pm._sell_units(L, mode)
            W = int(fm.head_words(np.array([T]), mode)[0])
            assert T - W == (L + (L & 1) if mode in (4, 5) else (T - 1 if mode == 3 else L)), (mode, L, T, W)
            assert mode != 3 or (T % 2 == 0 and L <= T - 1 <= L + 1)
    assert int(fm.head_words(np.array([0]), 5)[0]) == 0


def test_table_states_a_form_for_every_case_and_the_model_predicts_it():
    names = [c.name for c in fm.CASES]
    assert len(set(names)) == len(names) and {c.group for c in fm.CASES} == set(fm.GROUPS)
    bad = []
    for c in fm.CASES:
        assert c.op in fm.OPS and c.edge, c.name
        assert c.want and (not c.transpose or (c.want_t and c.want_tt)), "%s states no form" % c.name
        bad += fm.want_mismatches(c)
        exp = fm.expected_of(c)
        assert exp["form"] in ("Template", "Sliced", "SlicedNarrow", "Sliced32", "Coded8", "Coded16", "Staged", "Stream", "StreamWide",
                               "StreamDelta8", "StreamDelta16", "Vector"), (c.name, exp["form"])
        for form, reason in c.unavailable.items():                        # a refusal that is the case's purpose: the model refuses too, with a reason
            key = {"sliced": "sell", "sliced32": "sell32", "coded": "codes", "delta": "delta", "template": "template"}[form]
            assert key in exp["why"] and reason, (c.name, form, exp["why"])
    assert not bad, bad
    # every group is populated, every option set touches known options only
    assert all(len(fm.cases_of(g)) >= 10 for g in fm.GROUPS), {g: len(fm.cases_of(g)) for g in fm.GROUPS}
    assert all(set(c.opts) <= set(fm.BASE) for c in fm.CASES)


def test_coverage_condition():
    cov = fm.coverage()
    missing = {e: [s for s in sides if not cov.get(e, {}).get(s)] for e, sides in fm.REQUIRED_SIDES.items()}
    missing = {e: s for e, s in missing.items() if s}
    assert not missing, missing
    empty = [(e, s) for e, sides in cov.items() for s, v in sides.items() if not v]
    assert not empty, empty
    # the sliced modes are all reached, with both layouts
    assert all(("layout of mode %d" % mode) in cov for mode in range(6))


def test_families_sit_on_their_edges():
    """The sizes the builders' integer rules turn on, counted on the operators themselves."""
    for T in (1, 15, 16, 255, 256, 257, 2048, 2049):
        assert fm.get_op("diag%d" % T).info()["diagonals"] == T
    op = fm.get_op("diag256_last")
    d = op.col.astype(np.int64) - op.row_of
    assert (d == d.max()).sum() == 1 and op.row_of[np.argmax(d)] == op.m - 1
    assert (fm.get_op("diag16_neg").col.astype(np.int64) - fm.get_op("diag16_neg").row_of).max() < 0
    assert sorted(set(fm.sell_layout(fm.get_op("ragged64"), 0)["Ls"].tolist())) == list(range(1, 65))
    assert fm.get_op("row64").info()["max_row"] == 64 and fm.get_op("row65").info()["max_row"] == 65
    for name, entries in (("block65535", 65535), ("block65536", 65536)):
        assert int(fm.get_op(name).rowptr[32]) == entries
    a, r = fm.get_op("by_admit"), fm.get_op("by_refuse")
    assert a.nnz == r.nnz == (1 << 22) + 2 and a.nnz >= fm.BIG_NNZ
    da, dr = (fm.delta_model(o, dict(fm.BASE, spmv_kernel=1, spmv_delta=2), 256) for o in (a, r))
    assert 6 * da["by"] == 5 * da["by32"] and 6 * dr["by"] == 5 * dr["by32"] + 36
    assert fm.get_op("mean12").info()["mean_row"] == 12.0 and fm.get_op("mean96").info()["mean_row"] == 96.0
    assert 256 * fm.get_op("mean8").info()["mean_row"] == 2048.0 < 256 * fm.get_op("mean8_plus").info()["mean_row"]
    assert fm.get_op("band_perm12").info()["max_row"] > 8 and fm.get_op("band_split12").info()["max_row"] > 8
    for name in ("band_perm", "band_split", "band_perm12", "band_split12", "tr_repeats"):
        op = fm.get_op(name)
        unsorted = any(np.any(np.diff(op.col[a:b]) < 0) for a, b in zip(op.rowptr[:-1], op.rowptr[1:]))
        repeated = any(np.unique(op.col[a:b]).size < b - a for a, b in zip(op.rowptr[:-1], op.rowptr[1:]))
        assert unsorted and (repeated or name.startswith("band_perm")), name
    # special values are in every family's inputs and, but for the template families, in its values
    for c in fm.CASES:
        op = fm.get_op(c.op)
        xs = op.inputs()["xs"]
        assert np.isnan(xs).any() and (np.isinf(xs).any() or op.n < 4)
        if c.group != "template" and op.lens.max() >= 2 and op.n > 1:
            assert np.signbit(op.val[op.val == 0.0]).any(), c.op
        nf = op.nonfinite()                                              # the second handle: Inf and NaN in val, finite rows left
        assert np.isnan(nf.val).any() and np.isinf(nf.val).any() and np.array_equal(nf.col, op.col)
        assert np.isfinite(nf.inputs()["y"]).any() or op.m < 4, c.op


@pytest.mark.parametrize("group", fm.GROUPS)
def test_emulation_reproduces_the_serial_product(group):
    """Encode as the builder, decode as the kernel, multiply in stored order: bit for bit the plain serial product, so the GPU
    file's comparisons can pass."""
    for c in fm.cases_of(group):
        fails = fm.judge(c, fm.emulate(c))
        assert not fails, (c.name, fails[:3])


_FAULT_GROUPS = {
    "delta_escape_bound_off_by_one": ("delta",), "delta_below_base_not_escaped": ("delta",),
    "sentinel_ff_read_as_entry": ("codes", "sliced"), "sentinel_f_read_as_entry": ("codes", "sliced"),
    "mode5_head_words_off_in_one_range": ("sliced",), "uniform_units_on_offset_layout": ("sliced",),
    "pair_value_word_swapped": ("sliced", "unsorted"), "code16_truncated_to_8": ("codes",),
    "template_match_by_value": ("template",), "template_id_byte_truncated": ("template",),
    "transpose_unstable_among_repeats": ("transpose", "unsorted"), "scan_tile_offset_dropped": ("transpose",),
}


@pytest.mark.parametrize("fault", fm.FAULTS)
def test_every_injected_fault_is_rejected(fault):
    """The project's standing way of showing that a pin can fail: each fault in the emulation makes the comparison the GPU file
    uses reject at least one case (and a case the fault cannot touch still passes)."""
    assert len(fm.FAULTS) >= 12 and set(_FAULT_GROUPS) == set(fm.FAULTS)
    rejected = []
    for group in _FAULT_GROUPS[fault]:
        for c in fm.cases_of(group):
            if c.op.startswith("by_") or c.op == "sell32_heads":         # the two largest families: the smaller ones carry every fault
                continue
            if fm.judge(c, fm.emulate(c, fault)):
                rejected.append(c.name)
    assert rejected, fault
    assert not fm.judge(fm.CASE["plan_mean12_plus"], fm.emulate(fm.CASE["plan_mean12_plus"], fault))     # the plain stream: untouched by all
