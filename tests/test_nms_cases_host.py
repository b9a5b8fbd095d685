"""The NMS edge cases of tests/nms_cases.py on the CPU: the oracle's C NonMaxSuppressionV5 against its pure-Python twin on
every kind x parameter set, and the conditions that keep the device tests (tests/test_gpu_nms_edges.py) from passing
vacuously - asserted on the reference alone."""
import functools

import numpy as np
import pytest

import nms_cases as NC
from oracle import post_ref as P

SIZES = (1, 7, 130, 400)


@functools.lru_cache(maxsize=None)
def _ref(kind, n, ps):
    b, s = NC.make_for(kind, n, ps)
    b.setflags(write=False)
    s.setflags(write=False)
    return b, s, P.nms_v5(b, s, ps[0], ps[1], ps[2], ps[3], True)


def _iou(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return np.float32(P._lib().oracle_iou(a.ctypes.data, b.ctypes.data))


@pytest.mark.parametrize("kind", NC.KINDS)
def test_generator_is_deterministic_and_finite_in_the_boxes(kind):
    for n in SIZES + (1025,):
        b, s = NC.make(kind, n, 3)
        b2, s2 = NC.make(kind, n, 3)
        assert b.dtype == np.float32 and s.dtype == np.float32 and b.shape == (n, 4) and s.shape == (n,)
        assert np.array_equal(NC.bits(b), NC.bits(b2)) and np.array_equal(NC.bits(s), NC.bits(s2))
        assert np.isfinite(b).all()
        if kind != "special_scores":
            assert np.isfinite(s).all()
    assert not np.array_equal(NC.make(kind, 130, 0)[0], NC.make(kind, 130, 1)[0])


def test_the_issues_parameter_sets_are_all_there():
    inf = float("-inf")
    for ps in ((100, 0.5, 0.001, 0.25), (128, 0.5, inf, 0.0), (1, 0.5, inf, 0.25), (65, NC.THIRD, -0.5, 0.0),
               (64, 0.5, -2.0, 0.15), (63, 0.5, 0.001, 0.25), (100, 0.0, inf, 0.0), (100, -1.0, inf, 0.0),
               (100, 1.0, 0.25, 0.0), (100, 0.5, 0.5, 0.0)):
        assert ps in NC.PARAM_SETS
    assert np.float32(NC.THIRD) == np.float32(1.0) / np.float32(3.0)


@pytest.mark.parametrize("ps", NC.PARAM_SETS, ids=lambda ps: "M%d-iou%.3g-thr%g-sig%g" % ps)
@pytest.mark.parametrize("kind", NC.KINDS)
def test_c_oracle_equals_python_twin(kind, ps):
    for n in SIZES:
        b, s, (idx, sc, valid) = _ref(kind, n, ps)
        pidx, psc, pvalid = P.nms_v5_py(b, s, ps[0], ps[1], ps[2], ps[3], True)
        assert valid == pvalid, (n, valid, pvalid)
        np.testing.assert_array_equal(idx, pidx, err_msg="n %d" % n)
        np.testing.assert_array_equal(NC.bits(sc), NC.bits(psc), err_msg="n %d" % n)
        assert not np.isnan(sc).any(), "the reference result must be NaN-free (n %d)" % n


@pytest.mark.parametrize("kind", [k for k in NC.KINDS if k != "plain"])
def test_some_set_selects_and_some_set_runs_dry(kind):
    """Every kind is selected from (0 < valid) and exhausted (valid < max_out) by at least one parameter set."""
    for n in (130, 400):
        valids = [(int(_ref(kind, n, ps)[2][2]), ps[0]) for ps in NC.PARAM_SETS]
        assert any(v > 0 for v, _ in valids), (n, valids)
        assert any(v < m for v, m in valids), (n, valids)


def test_grid_meets_the_threshold_exactly():
    """Hard NMS on the integer grid: some (candidate, selected) pair has IoU == iou_thresh bit for bit (the `sim > thr`
    branch must not fire) and some pair lies strictly above it - for 1/2 and for float32(1/3)."""
    for ps in NC.PARAM_SETS:
        if NC.is_soft(ps) or ps[1] not in (0.5, NC.THIRD):
            continue
        b, s, (idx, sc, valid) = _ref("grid", 400, ps)
        thr = np.float32(ps[1])
        sel = idx[:valid]
        assert valid > 1
        sims = np.array([[_iou(b[i], b[j]) for j in sel] for i in range(0, 400, 3)], np.float32)
        assert (sims == thr).any(), ps
        assert (sims > thr).any(), ps
        assert (sims == 0).any() and (sims == 1).any(), ps
    # boxes that touch edge to edge exist (IoU 0 by a zero-width intersection)
    b = NC.make("grid", 400)[0]
    assert ((b[:, None, 3] == b[None, :, 1]) & (b[:, None, 0] == b[None, :, 0])).any()


def test_zero_area_boxes_are_selected():
    hit = 0
    for n in (7, 130, 400):
        for ps in NC.PARAM_SETS:
            b, s, (idx, sc, valid) = _ref("zero_area", n, ps)
            sb = b[idx[:valid]]
            hit += int((((sb[:, 2] - sb[:, 0]) * (sb[:, 3] - sb[:, 1])) == 0).sum())
    assert hit > 0


def test_negative_scores_grow_under_soft_nms():
    """The growing-score regime is reached: under a soft set with a negative threshold some selected score is greater
    than that candidate's input score."""
    grown = 0
    for ps in NC.PARAM_SETS:
        if not (NC.is_soft(ps) and ps[2] < 0):
            continue
        for n in (130, 400):
            b, s, (idx, sc, valid) = _ref("negative", n, ps)
            assert NC.grows(ps, s)
            grown += int((sc[:valid] > s[idx[:valid]]).sum())
    assert grown > 0
    assert not NC.grows((100, 0.5, NC.NEG_INF, 0.0), np.float32([-1.0]))          # hard: no weight below 1
    assert not NC.grows((100, 0.5, 0.001, 0.25), np.float32([-1.0]))               # never live
    assert not NC.grows((100, 0.5, -2.0, 0.25), np.float32([-0.0, 0.5, np.nan]))   # -0.0 is not below 0


def test_special_scores_never_select_nan_or_minus_inf_but_do_select_zeros():
    zeros = infs = 0
    for n in (130, 400):
        for ps in NC.PARAM_SETS:
            b, s, (idx, sc, valid) = _ref("special_scores", n, ps)
            chosen = s[idx[:valid]]
            assert not np.isnan(chosen).any() and not (chosen == -np.inf).any(), ps
            assert np.isinf(s).any() and np.isnan(s).any()
            assert (s == np.inf).sum() == (3 if NC.takes_inf(ps) else 0)
            infs += int((chosen == np.inf).sum())
            if ps[2] < 0:
                zeros += int((chosen == 0).sum())
                both = NC.bits(chosen[chosen == 0])
                if len(both):
                    # a -0.0 comes out as -0.0: the bit pattern is part of the comparison
                    assert np.array_equal(NC.bits(sc[:valid][chosen == 0]), both)
    assert zeros > 0 and infs > 0
    s = NC.make("special_scores", 400)[1]
    assert (NC.bits(s) == 0x80000000).any() and (NC.bits(s) == 0).any()
    assert (np.isnan(s) & (NC.bits(s) >> 31 == 1)).any() and (np.isnan(s) & (NC.bits(s) >> 31 == 0)).any()


def test_both_zeros_tie_and_the_lower_index_wins():
    """-0.0 == +0.0 for the reference's heap: among zero scores of either sign the smaller index is selected first, and
    each keeps its own bit pattern on the way out."""
    b = np.float32([[0, 0, 1, 1], [10, 10, 11, 11], [20, 20, 21, 21], [30, 30, 31, 31]])
    s = np.float32([-0.0, 0.0, -0.0, 0.0])
    idx, sc, valid = P.nms_v5(b, s, 4, 0.5, -1.0, 0.0, True)
    assert valid == 4 and idx.tolist() == [0, 1, 2, 3]
    assert NC.bits(sc).tolist() == [0x80000000, 0, 0x80000000, 0]


def test_half_below_moves_half_to_the_threshold():
    for ps in NC.PARAM_SETS:
        s = NC.make_for("plain", 400, ps)[1] + np.float32(1.0)
        h = NC.half_below(s, ps)
        dead = ~(h > np.float32(ps[2]))
        assert 120 < dead.sum() < 280
        assert np.array_equal(h[~dead], s[~dead])


def test_epoch_rule_is_not_exact_on_growing_scores():
    """Why `uda_nms` refuses soft NMS over live negative scores: the kernels' epoch rule (its CPU model,
    tests/test_nms_multiwinner_model.py) caches an exact score as an upper bound, which a growing score breaks - on the
    `negative` kind the model's selections differ from the reference's, while the same inputs under hard NMS agree."""
    from test_nms_multiwinner_model import EpochModel
    b, s = NC.make("negative", 130)
    differ = 0
    for ps in NC.PARAM_SETS:
        if ps[0] < 2 or ps[2] >= 0:
            continue
        m = EpochModel(b, s, ps[0], ps[1], ps[2], ps[3], blocks=8, winners=1)
        m.run()
        idx, sc, valid = P.nms_v5(b, s, ps[0], ps[1], ps[2], ps[3], False)
        same = list(m.sel) == idx.tolist() and np.array_equal(NC.bits(np.float32(m.sel_score)), NC.bits(sc))
        if NC.grows(ps, s):
            differ += not same
        else:
            assert same, ps
    assert differ > 0
