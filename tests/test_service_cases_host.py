"""The evaluation-service edge cases of tests/service_cases.py on the CPU: the inputs are the ones the reference saw
(checksums of tests/golden/service_edges_golden.npz), the numpy mirrors reproduce what the reference's own functions returned
on the assign and coco cases, and every case reaches the boundary it is named after - asserted on the mirrors' values alone,
so that the device test (tests/test_gpu_service_edges.py) cannot pass vacuously."""
import math
import os

import numpy as np
import pytest

import service_cases as SC
import validate_ref as V

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "service_edges_golden.npz"))


# ------------------------------------------------------------------ the fixture belongs to these inputs
def test_fixture_checksums_and_size():
    for name in SC.ASSIGN_CASES:
        c = SC.assign_case(name)
        assert SC.checksum(c["dets"], c["gt_boxes"], c["gt_classes"]) == GOLD["a_%s_crc" % name], name
    for name in SC.COCO_GOLDEN_CASES:
        c = SC.coco_case(name)
        assert SC.checksum(c["det"], c["gt"]) == GOLD["c_%s_crc" % name], name
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    assert os.path.getsize(os.path.join(here, "service_edges_golden.npz")) < os.path.getsize(os.path.join(here, "pseudo_golden.npz"))
    assert not [k for k in GOLD.files if k.endswith(("_dets", "_gt", "_det", "_gt_boxes", "_gt_classes"))]      # outputs only


def test_generators_are_deterministic_and_finite():
    a, b = SC.assign_case("m65", 3), SC.assign_case("m65", 3)
    assert all(np.array_equal(a[k], b[k]) for k in a) and not np.array_equal(a["dets"], SC.assign_case("m65", 4)["dets"])
    for name in SC.ASSIGN_CASES:
        assert all(np.isfinite(v).all() and v.dtype == np.float32 for v in SC.assign_case(name).values()), name
    for name in SC.SCORE_CASES + SC.PSEUDO_CASES:
        cols = (SC.score_case(name) if name in SC.SCORE_CASES else SC.pseudo_case(name))["cols"]
        assert all(np.isfinite(v).all() and v.dtype == np.float32 for v in cols.values()), name
    for name in SC.COCO_CASES:
        c = SC.coco_case(name)
        assert np.isfinite(c["det"]).all() and np.isfinite(c["gt"]).all() and c["det"].dtype == c["gt"].dtype == np.float32
    for name in SC.THR_CASES:
        c = SC.thr_case(name)
        assert np.isfinite(c["uncerts"]).all() and np.isfinite(c["params"]).all()


def test_the_issues_shapes_are_all_there():
    assert SC.ASSIGN_M == (0, 1, 63, 64, 65, 129, 4095, 4096) and SC.ASSIGN_G == (1, 4, 5, 257, 16384)
    assert [s[0] for s in SC.SCORE_SHAPES] == [1, 64, 65, 255, 256, 257, 513, 4096]
    assert {s[1] for s in SC.SCORE_SHAPES} == {1, 8, 129, 8192} and {s[2] for s in SC.SCORE_SHAPES} == {1, 7, 8, 9, 128}
    single = SC.COCO_SINGLE.values()
    assert {s[0] for s in single} >= {127, 128, 129, 300} and {s[1] for s in single} == {0, 1, 33, 256} and {s[2] for s in single} == {1, 32}
    for name in SC.ASSIGN_CASES:
        c = SC.assign_case(name)
        M, G = c["dets"].shape[1], c["gt_classes"].shape[1]
        assert (M, G) == ((int(name[1:]), 9) if name[0] == "m" and name != "mse_tie" else (65, int(name[1:])) if name[0] == "g" else (200, G))


# ------------------------------------------------------------------ assign: the mirror against the reference, the boundaries
@pytest.mark.parametrize("name", SC.ASSIGN_CASES)
def test_assign_mirror_reproduces_the_reference(name):
    identical = True
    for method in SC.ASSIGN_METHODS:
        for keep in SC.ASSIGN_KEEPS:
            tag = "a_%s_%s_%s" % (name, method, keep)
            want = SC.expected_assign(name, method, keep)
            assert (want is not None) == bool(GOLD[tag + "_ok"][0]), tag
            if want is None:
                continue
            np.testing.assert_array_equal(want[0], GOLD[tag + "_idx"], err_msg=tag)
            np.testing.assert_array_equal(want[2], (GOLD[tag + "_idx"] >= 0).sum(1), err_msg=tag)
            np.testing.assert_allclose(want[1], GOLD[tag + "_iou"], rtol=0, atol=1e-12, err_msg=tag)
            identical &= np.array_equal(want[1].view(np.uint64), GOLD[tag + "_iou"].view(np.uint64))
    print("%s: IoU bit-identical to the reference: %s" % (name, identical))


def test_assign_cases_reach_their_boundaries():
    E = SC.expected_assign
    # M = 0: every kept row under `validate` has nothing to match (the reference fails too); `calibrate` keeps rows < min(G, M): none
    for method in SC.ASSIGN_METHODS:
        assert E("m0", method, "validate") is None
        idx, iou, count = E("m0", method, "calibrate")
        assert (idx == -1).all() and (count == 0).all() and (iou == 0).all()
    # the rank branch past the detections: refused, as the reference would index past them
    for name in ("m1", "m63", "m64", "m65", "m129", "m4095", "m4096", "g1", "g4", "g5", "ident", "mse_tie"):
        M = SC.assign_case(name)["dets"].shape[1]
        kept_past = (np.nonzero(SC.assign_case(name)["gt_classes"] > 0)[1] >= M).any()
        assert (E(name, "rank", "validate") is None) == kept_past, name
    assert E("g257", "rank", "validate") is None and E("g16384", "rank", "validate") is None
    assert E("g257", "rank", "calibrate")[2].tolist() == [58, 58]           # rows < 65 with class >= 0
    for method in ("IoU", "MSE"):
        for keep in SC.ASSIGN_KEEPS:
            # lanes without a candidate (M < 64), the second and third step of the lane loop, the cap
            for name, least in (("m1", 0), ("m63", 62), ("m64", 63), ("m65", 64), ("m129", 128), ("m4095", 4094), ("m4096", 4095)):
                idx, _, count = E(name, method, keep)
                assert idx.max() == least and count.min() > 0, (name, method, keep)
                assert (idx[1][idx[1] >= 0] < max(1, 2 * (least + 1) // 3)).all()          # image 1: never a padded slot
            for name in ("g1", "g4", "g5", "g257", "g16384"):
                idx, _, count = E(name, method, keep)
                G = idx.shape[1]
                assert idx.max() == 64 and count.min() > 0
                if keep == "validate":
                    assert (idx[:, G - 1] >= 0).all() or (G - 1) % 9 in (6, 8)              # the last row is a kept one
            assert E("g16384", method, "validate")[2].min() > 150
            assert (E("g16384", method, "validate")[0][:, 16383] >= 0).all() and (E("g16384", method, "calibrate")[0][:, 65:] == -1).all()
    # identical boxes across ranks 63 / 64 and 127 / 128: the first of the block wins, between lanes (60 against 64 .. 67 and
    # 128 .. 131 of lanes 0 .. 3) and between the strides of one lane (70 against 134)
    c = SC.assign_case("ident")
    for im, (lo, hi) in enumerate(SC.IDENT_BLOCKS):
        assert lo < 64 <= 127 < 128 < hi or (64 <= lo < 128 < hi)
        assert (c["dets"][im, lo:hi] == c["dets"][im, lo]).all()
        for row in (0, 1):
            iou, mse = V.iou_keys(c["gt_boxes"][im, row], c["dets"][im]), V.mse_keys(c["gt_boxes"][im, row], c["dets"][im])
            assert (iou[lo:hi] == iou.max()).all() and (np.delete(iou, np.s_[lo:hi]) < iou.max()).all()
            assert (mse[lo:hi] == mse.min()).all() and (np.delete(mse, np.s_[lo:hi]) > mse.min()).all()
            for method in ("IoU", "MSE"):
                assert E("ident", method, "validate")[0][im, row] == lo
    assert SC.IDENT_BLOCKS[1][0] >= 64 and SC.IDENT_BLOCKS[1][0] + 64 < SC.IDENT_BLOCKS[1][1]      # 70 and 134: one lane, two strides
    # MSE: two different boxes at exactly equal distance; the lower rank wins inside a lane across strides and between lanes
    c = SC.assign_case("mse_tie")
    same_lane = across_63_64 = 0
    for im in range(2):
        for row, (minus, plus) in enumerate(SC.MSE_TIES[im]):
            mse = V.mse_keys(c["gt_boxes"][im, row], c["dets"][im])
            assert mse[minus] == mse[plus] == 16.0 and not np.array_equal(c["dets"][im, minus], c["dets"][im, plus])
            assert (np.delete(mse, [minus, plus]) > 1000).all()
            assert E("mse_tie", "MSE", "validate")[0][im, row] == min(minus, plus)
            same_lane += (plus - minus) % 64 == 0
            across_63_64 += (minus, plus) == (63, 64)
    assert same_lane == 2 and across_63_64 == 1


# ------------------------------------------------------------------ score
@pytest.mark.parametrize("name", SC.SCORE_CASES)
def test_score_cases_reach_their_boundaries(name):
    c = SC.score_case(name)
    comp, count, cls = SC.expected_score(name)
    cols, M, C = c["cols"], c["cols"]["scores"].shape[1], c["num_classes"]
    assert np.isfinite(comp).all()
    for i, (kind, lo, hi) in enumerate(c["layout"]):
        kept = np.nonzero(cols["scores"][i] > np.float32(c["min_score"]))[0]
        assert count[i] == len(kept) > 0 and cls[i].sum() == count[i]
        assert cls[i, C - 1] >= 1 and (cls[i, 0] >= 1 or len(kept) == 1)   # class ids 1 and C among the kept rows
        if kind == "kept_wave3":                                          # waves 0 .. 2 hold nothing, wave 3 holds real values
            assert kept.min() >= 192 and kept.max() < 256
        if kind == "kept_stride2":                                        # the first step of the row loop holds nothing
            assert kept.min() >= 256
        if kind.startswith("top") and not c["reduce_mean"]:
            r = min(SC.TOP_ROWS[kind], M - 1)
            assert r in kept and comp[i].tolist() == list(SC.TOP_VALUES)
            if kind == "top_wave3":
                assert r < 256 and r // 64 == 3
            if kind == "top_stride2":
                assert r >= 256
            other = np.delete(kept, np.searchsorted(kept, r))            # and no other row comes near the planted values
            if len(other):
                rel = cols["mcbox"][i, other].astype(np.float64).max() / 8.0
                assert rel < 125.0 and cols["mcclass"][i, other].max() < 100.0
        if c["reduce_mean"]:
            # the mirror's pairwise np.mean against the exactly rounded sum: inside the suite's rtol, so a device that sums in
            # another order can be too; and the order does matter at this spread
            ent = cols["entropy"][i, kept].astype(np.float64)
            al = cols["albox"][i, kept].astype(np.float64)
            exact = [math.fsum(ent) / len(kept), math.fsum((((al[:, 0] + al[:, 1]) + al[:, 2]) + al[:, 3]) / 4.0) / len(kept)]
            np.testing.assert_allclose(comp[i, :2], exact, rtol=1e-12, atol=0)
            assert ent.max() / ent.min() > 2.0 ** 20 or len(kept) == 1
    if c["reduce_mean"] and M >= 255:
        differs = False                                                   # (np.sum of a reversed view: numpy's pairwise sum, backwards)
        for i in range(len(c["layout"])):
            kept = np.nonzero(cols["scores"][i] > np.float32(c["min_score"]))[0]
            al = cols["albox"][i, kept].astype(np.float64)
            per_row = [cols["entropy"][i, kept].astype(np.float64), (((al[:, 0] + al[:, 1]) + al[:, 2]) + al[:, 3]) / 4.0]
            differs |= any(np.sum(v[::-1]) / len(kept) != comp[i, k] for k, v in enumerate(per_row))
        assert differs, "no mean of the case depends on the order of summation"
    if M == 4096:
        assert count.max() == 4096


# ------------------------------------------------------------------ pseudo
def test_pseudo_cases_reach_their_boundaries():
    (res, minmax, kept, cand, _), sel = SC.expected_pseudo("n258")
    assert len(cand) == 258 and set(cand.tolist()) == {0, 1, 2}
    assert cand[:256].sum() > 0 and cand[256] > 0 and cand[257] > 0       # image 257's offset: thread 0 adds cand[0] and cand[256]
    assert (res["image"] >= 256).sum() == cand[256:].sum() and len(sel[0]) > 0
    (res99, _, kept99, cand99, _), _ = SC.expected_pseudo("m4096_r99")
    (res, _, kept, cand, _), sel = SC.expected_pseudo("m4096_r4096")
    assert kept99[0] == kept[0] > 3000 and 0 < cand99[0] < 99 and cand[0] > 1024
    assert res99["row"].max() < 256 <= 4000 < res["row"].max() and len(sel[0]) == 1


# ------------------------------------------------------------------ coco: the mirror against the reference, the boundaries
@pytest.mark.parametrize("name", SC.COCO_GOLDEN_CASES)
def test_coco_mirror_reproduces_the_reference(name):
    c = SC.coco_case(name)
    rec, npig, used = SC.expected_coco(name, True)
    want, ev = GOLD["c_%s_rec" % name], GOLD["c_%s_evaluated" % name]
    np.testing.assert_array_equal(ev, SC.evaluated_rows(c["det"], c["gt"], c["num_classes"]))
    np.testing.assert_array_equal(used, GOLD["c_%s_used" % name])
    for f in ("rank", "cls", "score"):
        np.testing.assert_array_equal(rec[f], want[f], err_msg=f)
    for f in ("matched", "ignored"):
        picked = np.zeros_like(rec[f])
        for k, t in enumerate(SC.STD_PICK):
            picked |= ((want[f] >> np.uint32(t)) & np.uint32(1)) << np.uint32(k)
        np.testing.assert_array_equal(rec[f][ev], picked[ev], err_msg=f)
    np.testing.assert_array_equal(npig[used > 0], GOLD["c_%s_npig" % name][used > 0])
    assert ev.any() == (c["gt"].shape[1] > 0)


def test_coco_cases_reach_their_boundaries():
    for name, (M, G, T, per_image) in SC.COCO_SINGLE.items():
        c = SC.coco_case(name)
        rec, npig, used = SC.expected_coco(name)
        assert c["det"].shape[1] == M and c["gt"].shape[1] == G and len(c["thrs"]) == T and used.tolist() == list(per_image)
        assert (c["gt"][:, :, 6] == 1).all() and (npig[:, 0, 0] + (c["gt"][:, :, 4] != 0).sum(1) == G).all()
        full = (1 << T) - 1
        if G:
            assert (rec["matched"][:, 0, 0] == full).all() and (rec["matched"] >> np.uint32(T) == 0).all()      # every thread t < T matches
        if M > 100:
            for i in range(len(per_image)):
                r, s = rec[i]["rank"], rec[i]["score"]
                assert (r >= 100).any() and (rec[i]["matched"][r >= 100] == 0).all() and (rec[i]["ignored"][r >= 100] == 0).all()
                assert s[r == 99][0] == s[r == 100][0], "no tie across rank 99 / 100"
                assert s[40] == s[3] and r[3] < r[40]                     # ties go by row
                if per_image[i] > 127:
                    assert s[127] == s[3] and r[3] < r[127]
                if per_image[i] > 128:
                    assert s[127] == s[128] and r[128] == r[127] + 1      # a tie across row 127 / 128
                if per_image[i] > 130:                                    # (at 129 rows, row 128 is the tie's last: rank 100)
                    assert (r[128:per_image[i]] < 100).any() and (r[128:per_image[i]] >= 100).any()
        if G > 32:
            # detection row 0 copies ground-truth row 32, which lies 3000 away from every other one: it is matched at every
            # threshold, which only bit 32 of `taken` (the second word) can have recorded
            assert (c["gt"][:, 32, 0] >= 3000).all() and (np.delete(c["gt"][:, :, 0], 32, 1) < 1000).all()
            assert (rec["matched"][:, 0, 0] == full).all() and (rec["rank"][:, 0] == 0).all()
    # areas exactly on the inclusive ends and one ulp either side
    c = SC.coco_case("area")
    rec, npig, used = SC.expected_coco("area")
    a32 = np.asarray(c["plant"]["areas"], np.float32)
    for k, end in ((1, 1024.0), (4, 9216.0)):
        assert a32[k] == np.float32(end) and a32[k - 1] == np.nextafter(np.float32(end), np.float32(0)) and a32[k + 1] == np.nextafter(np.float32(end), np.float32(1e9))
    gt_area = (c["gt"][0, :6, 3] - c["gt"][0, :6, 1]) * (c["gt"][0, :6, 2] - c["gt"][0, :6, 0])
    assert np.array_equal(gt_area, a32) and np.array_equal(c["det"][0, :12:2, 3] * c["det"][0, :12:2, 4], a32)
    assert npig[0, 0].tolist() == [6, 2, 4, 2]                            # small: below, on 1024; medium: 1024 .. 9216 inclusive; large: on, above 9216
    ign = rec["ignored"][0, :12] != 0                                     # [row, area range]: matched rows 0, 2, .. take the box's flag, unmatched 1, 3, .. their own
    for rows in (slice(0, 12, 2), slice(1, 12, 2)):
        assert ign[rows, 1].tolist() == [False, False, True, True, True, True]       # small flips between 1024 and the next float
        assert ign[rows, 2].tolist() == [True, False, False, False, False, True]     # medium flips below 1024 and above 9216
        assert ign[rows, 3].tolist() == [True, True, True, True, False, False]       # large flips below 9216
    assert (rec["matched"][0, 0:12:2, 0] == 3).all() and (rec["matched"][0, 1:12:2] == 0).all()
    # crowds at orders 0, 31, 32, 255: each one matched by two detections
    c = SC.coco_case("crowd")
    rec, npig, used = SC.expected_coco("crowd")
    assert np.nonzero(c["gt"][0, :, 4])[0].tolist() == list(SC.CROWD_ORDERS) and npig[0, 0, 0] == 252
    rows = c["plant"]["crowd_det_rows"]
    assert len(rows) == 8 and (rec["matched"][0, rows, 0] == 3).all() and (rec["ignored"][0, rows, 0] == 3).all()
    # equal IoUs: two detections on one box (the better score takes it), one detection between two boxes
    rec, npig, used = SC.expected_coco("equal_iou")
    assert rec["matched"][0, :3, 0].tolist() == [7, 0, 1] and rec["rank"][0, :3].tolist() == [0, 1, 2]
    # class values 2.5, 0.0, -0.5 and C + 1
    c = SC.coco_case("classes")
    rec, npig, used = SC.expected_coco("classes")
    assert c["det"][0, 16:20, 6].tolist() == list(SC.ODD_CLASSES) and used[0] == 20
    assert rec["cls"][0, 16:20].tolist() == [2, 0, 0, 4] and rec["rank"][0, 16] >= 0 and (rec["rank"][0, 17:20] == -1).all()
    assert (rec["cls"][0] == 2).sum() >= 3
    # C = 8192: blocks 1, 4096 and 8192 hold rows, every block between them is empty
    c = SC.coco_case("c8192")
    rec, npig, used = SC.expected_coco("c8192")
    assert set(rec["cls"][0, :12].tolist()) == {1, 4096, 8192} and np.nonzero(npig[0, :, 0])[0].tolist() == [0, 4095, 8191]
    assert (rec["matched"][0] != 0).any()
    c = SC.coco_case("m4096")
    rec, npig, used = SC.expected_coco("m4096")
    assert c["det"].shape[1] == 4096 and used[0] == 4000 and rec["rank"].max() > 1900 and (rec["matched"][0, :, 0] == 3).any()


# ------------------------------------------------------------------ thr
def test_thr_cases_reach_their_boundaries():
    import thr_ref as R
    for name, N in (("n2047", 2047), ("n2048", 2048), ("n2049", 2049)):
        assert SC.thr_case(name)["uncerts"].shape == (2, N)
    for name, runs in (("runs512", 512), ("runs513", 513)):
        c = SC.thr_case(name)
        for p in c["params"]:
            assert len(np.unique(R.combined(c["uncerts"], p))) == runs
    assert SC.thr_case("u4")["uncerts"].shape[0] == 4 and SC.thr_case("u4")["params"].shape == (3, 4)
    c = SC.thr_case("g8192")
    assert c["group"].min() == 0 and c["group"].max() == 8191 and c["params"].shape == (2, 2 * 8192)
    for name in SC.THR_CASES:
        for fix_cd in (1, 0):
            thr, rate, auc = SC.expected_thr(name, fix_cd)
            assert np.isfinite(thr).all() and np.isfinite(rate).all() and ((auc > 0) & (auc < 1)).all(), name
