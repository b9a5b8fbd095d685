"""Label correction on the device (`uda_label_check[_np[_f32]]`, csrc/kernels_glc.hip; `label_correction.check_labels`,
`ServingDriver.serve_label_check` / `label_check`; reference src/ssl_utils/glc.py): both host-array entries against the numpy
mirror (tests/glc_ref.py) entry for entry at every size where the kernel takes another path, the reference's own returns and
file bytes (tests/golden/glc_golden.npz) through the float64 entry, the served flow against the mirror applied to the
detections and cons_iou the device produced, and the refusals.  Everything is exact: IoUs are compared bit for bit."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import glc_ref as R
from common import FULL_MC, make_images, make_params, make_weights

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glc_golden.npz"))
MIN_SCORE = 0.1
# the defaults but correct_max_inter: below 1, so that rows fail the noisy conditions through their IoU
THR = dict(iou_consist=0.90, md_max_inter=0, correct_max_inter=0.75, correct_score=0.40)
MS = (1, 63, 64, 65, 100, 257)                       # below, at and above a wave's lanes and the 256 threads of a block
ROWS = (0, 1, 3, 4, 5, 63, 64, 65, 257)              # fewer than, equal to and more than the 4 waves of a block; across 64
G = 260
KEYS = ("det_rank", "iou", "gt_flags", "gt_boxes_out", "det_flags", "det_max_iou", "counts")


def make_image(rng, M, kept, rows, dt):
    """One image: `kept` of the M ranks above min_score (spread over the ranks, not a prefix, unless all are kept), `rows`
    counted ground-truth rows among G (padding rows in between).  Counted rows: jittered copies of kept boxes, exact copies
    (IoU 1 > correct_max_inter), boxes that touch nothing, boxes around not-kept detections.  Arbitrary (non-grid) values."""
    y, x = rng.uniform(0, 900, M), rng.uniform(0, 1500, M)
    boxes = np.stack([y, x, y + rng.uniform(8, 90, M), x + rng.uniform(8, 90, M)], 1)
    scores = rng.uniform(0.001, MIN_SCORE, M)
    kr = np.sort(rng.choice(M, kept, replace=False)) if kept else np.zeros((0,), np.int64)
    scores[kr] = rng.uniform(0.11, 0.99, kept)
    cons = rng.uniform(0.6, 1.0, M)
    cons[rng.random(M) < 0.2] = 0.90                       # exactly at iou_consist: md yes, noisy no
    scores[kr[rng.random(kept) < 0.15]] = 0.40            # exactly at correct_score (as the array's own type rounds it)
    if kept >= 2:                                          # duplicate boxes: the tie goes to the lower rank
        boxes[kr[-1]] = boxes[kr[0]]
    gtb, gtc = rng.uniform(0, 50, (G, 4)), np.full((G,), -1.0)
    gr = np.sort(rng.choice(G, rows, replace=False)) if rows else np.zeros((0,), np.int64)
    for j, g in enumerate(gr):
        kind = rng.random()
        src = boxes[kr[rng.integers(kept)]] if kept and kind < 0.75 else boxes[rng.integers(M)]
        if kind < 0.25:
            gtb[g] = src
        elif kind < 0.85:
            gtb[g] = src + rng.normal(0, 6.0, 4)
        else:
            gtb[g] = [3000 + 200 * j, 3000, 3050 + 200 * j, 3100]
        gtc[g] = float(rng.integers(1, 8))
    return boxes.astype(dt), scores.astype(dt), cons, gtb.astype(dt), gtc.astype(dt)


def plant_groups(b, s, c, gb, gc):
    """Into image 0 (M >= 100, every rank kept): rows 8, 9 and 14 matched to rank 70 - row 8 (wave 0) an exact copy that fails
    correct_max_inter, row 9 (wave 1) and row 14 (wave 2) at IoU 0.5 that meet it - so the FIRST member is replaced and lies in
    another wave than the qualifying ones; rank 70's box also sits at ranks 5 and 130: equal IoUs on both sides of 64, and the
    group moves to rank 5."""
    box = np.array([2000.0, 2000.0, 2040.0, 2040.0])
    for r in (70, 130) if b.shape[1] > 130 else (70,):
        b[0, r], s[0, r], c[0, r] = box, 0.8, 0.97
    gb[0, 8], gb[0, 9], gb[0, 14] = box, [2000.0, 2000.0, 2040.0, 2080.0], [2000.0, 1960.0, 2040.0, 2040.0]
    gc[0, [8, 9, 14]] = 1.0
    return box


def run_np(cols, f32, md_rule="eq", methods=("md", "mistakes", "noisy"), **thr):
    from uda_amd import label_correction as lc
    return lc.label_check_np(*cols, MIN_SCORE, md_rule=md_rule, methods=methods, as_float32=f32, **dict(THR, **thr))


def expect(cols, f32, md_rule="eq", methods=("md", "mistakes", "noisy"), **thr):
    t = dict(THR, **thr)
    return R.check(*cols, MIN_SCORE, t["iou_consist"], t["md_max_inter"], md_rule, t["correct_max_inter"], t["correct_score"], methods, f32=f32)


def assert_same(got, want, what=""):
    for k in KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        if got[k].dtype == np.float64:
            assert np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)), (what, k)          # bit for bit
        else:
            np.testing.assert_array_equal(got[k], want[k], err_msg="%s %s" % (what, k))


def stack(images):
    return tuple(np.stack([im[q] for im in images]) for q in range(5))


# ------------------------------------------------------------------ both host-array entries against the mirror
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("M", MS)
def test_np_entries_match_the_mirror(M, f32):
    """n = 3 per call, the sizes mixed within a call: kept detections 0, 1 and M against every row count."""
    dt = np.float32 if f32 else np.float64
    rng = np.random.default_rng([M, int(f32)])
    seen = np.zeros(5, np.int64)
    for c0 in range(len(ROWS)):
        images = [make_image(rng, M, kept, ROWS[(c0 + j) % len(ROWS)], dt) for j, kept in enumerate((0, 1, M))]
        cols = stack(images)
        rule = "le" if c0 % 2 else "eq"
        got, want = run_np(cols, f32, rule), expect(cols, f32, rule)
        assert_same(got, want, "M %d call %d" % (M, c0))
        assert list(got["counts"][:, 0]) == [0, 1, M] and list(got["counts"][:, 1]) == [ROWS[(c0 + j) % len(ROWS)] for j in range(3)]
        seen += got["counts"].sum(0)
    assert seen[2] > 0 and seen[4] > 0 and (M == 1 or seen[3] > 0)          # mistakes, missing labels and replaced rows occurred


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("M", [100, 257])
def test_planted_groups_across_waves_and_lanes(M, f32):
    dt = np.float32 if f32 else np.float64
    rng = np.random.default_rng([7, M, int(f32)])
    images = [make_image(rng, M, M, 65, dt), make_image(rng, M, M // 2, 64, dt), make_image(rng, M, 3, 257, dt)]
    cols = [a.copy() for a in stack(images)]
    b, s, c, gb, gc = cols
    box = plant_groups(b, s, c, gb, gc)
    got = run_np(cols, f32)
    assert_same(got, expect(cols, f32), "planted")
    assert list(got["det_rank"][0, [8, 9, 14]]) == [70, 70, 70]
    assert list(got["gt_flags"][0, [8, 9, 14]]) == [R.GT_REPLACED, R.GT_NOISY, R.GT_NOISY] and got["iou"][0, 9] == 0.5
    assert got["counts"][1, 0] == M // 2 and not (np.where(s[1] > MIN_SCORE)[0] == np.arange(M // 2)).all()      # kept: not a prefix
    # the same box at a lower rank on the other side of 64 takes the group over, whichever lane saw it
    b[0, 5], s[0, 5], c[0, 5] = box, 0.95, 0.5
    got = run_np(cols, f32)
    assert_same(got, expect(cols, f32), "tie")
    assert list(got["det_rank"][0, [8, 9, 14]]) == [5, 5, 5] and not got["gt_flags"][0, [8, 9, 14]].any()   # (rank 5 is not consistent)


def test_second_call_returns_identical_arrays():
    rng = np.random.default_rng(11)
    cols = stack([make_image(rng, 100, k, r, np.float32) for k, r in ((100, 65), (37, 5), (1, 257))])
    first, second = run_np(cols, True), run_np(cols, True)
    for k in KEYS:
        assert first[k].tobytes() == second[k].tobytes(), k
    only = run_np(cols, True, methods=("mistakes",))
    np.testing.assert_array_equal(only["gt_flags"], first["gt_flags"] & R.GT_MISTAKE)
    assert not (only["det_flags"] & R.DET_MISSING).any() and not only["counts"][:, 3:].any()
    assert np.array_equal(only["iou"], first["iou"]) and np.array_equal(only["det_rank"], first["det_rank"])


def test_largest_sizes_launch():
    """M = 4096 float64 boxes take the largest LDS a block asks for; G = 16384 the longest row loop."""
    rng = np.random.default_rng(5)
    cols = stack([make_image(rng, 4096, 4096, 5, np.float64)])
    assert_same(run_np(cols, False), expect(cols, False), "M 4096")
    M = 4
    b, s, c = rng.uniform(0, 100, (1, M, 4)), np.full((1, M), 0.5), np.full((1, M), 0.95)
    b[..., 2:] += b[..., :2]
    gb, gc = np.zeros((1, 16384, 4)), np.full((1, 16384), -1.0)
    gb[0, [0, 16383]], gc[0, [0, 16383]] = [b[0, 3], [500, 500, 510, 510]], 1.0
    got = run_np((b, s, c, gb, gc), False)
    assert_same(got, expect((b, s, c, gb, gc), False), "G 16384")
    assert got["det_rank"][0, 0] == 3 and got["gt_flags"][0, 16383] & R.GT_MISTAKE


def test_limits_are_refused_with_outputs_untouched():
    from uda_amd import capi
    lib = capi.load()
    for n, M, Gt, words in ((1, 4097, 2, b"4097 detection rows per image, at most 4096"), (1, 4, 16385, b"16385 ground-truth rows per image, at most 16384"),
                            (0, 4, 2, b"0 images, at least 1")):
        nn = max(n, 1)
        ins = [np.ones((nn, M, 4)), np.ones((nn, M)), np.ones((nn, M)), np.ones((nn, Gt, 4)), np.ones((nn, Gt))]
        outs = [np.full((nn, Gt), 77, np.int32), np.full((nn, Gt), 7.5), np.full((nn, Gt), 77, np.uint8), np.full((nn, Gt, 4), 7.5, np.float32),
                np.full((nn, M), 77, np.uint8), np.full((nn, M), 7.5), np.full((nn, 5), 77, np.int32)]
        for fn, dt in ((lib.uda_label_check_np, np.float64), (lib.uda_label_check_np_f32, np.float32)):
            args = [a.astype(dt) if k != 2 else a for k, a in enumerate(ins)]
            rc = fn(0, *[a.ctypes.data_as(C.c_void_p) for a in args], n, M, Gt, 0.1, 0.9, 0.0, 0, 1.0, 0.4, 7,
                    *[a.ctypes.data_as(C.c_void_p) for a in outs])
            assert rc == 1 and words in lib.uda_last_error(None), lib.uda_last_error(None)
            for a in outs:
                assert (a == (77 if a.dtype.kind in "iu" else 7.5)).all()
    ok = [np.ones((1, 2, 4)), np.ones((1, 2)), None, np.ones((1, 2, 4)), np.ones((1, 2))]
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    outs = [None] * 7
    assert lib.uda_label_check_np(0, *map(p, ok), 1, 2, 2, 0.1, 0.9, 0.0, 0, 1.0, 0.4, 7, *outs) == 1
    assert b"md and noisy read cons_iou, which is not given" in lib.uda_last_error(None)
    assert lib.uda_label_check_np(0, *map(p, ok), 1, 2, 2, 0.1, 0.9, 0.0, 0, 1.0, 0.4, 8, *outs) == 1 and b"methods is a bit set" in lib.uda_last_error(None)
    assert lib.uda_label_check_np(0, *map(p, ok), 1, 2, 2, 0.1, 0.9, 0.0, 2, 1.0, 0.4, 2, *outs) == 1 and b"md_rule is 0" in lib.uda_last_error(None)
    assert lib.uda_label_check_np(0, *map(p, ok), 1, 2, 2, 0.1, 0.9, 0.0, 0, 1.0, 0.4, 2, *outs) == 0      # mistakes alone, every output NULL


# ------------------------------------------------------------------ the reference's own results through the float64 entry
@pytest.mark.parametrize("ci", range(len(GOLD["cases"])))
def test_golden_through_device_and_writers(ci, tmp_path):
    from test_glc_host import MODES, _kitti_inputs, check_against_golden
    from uda_amd import label_correction as lc, writers
    ic, md, cmi, cs = (float(v) for v in GOLD["cases"][ci])
    kw = dict(min_score=float(GOLD["min_score"][0]), iou_consist=ic, md_max_inter=md, correct_max_inter=cmi, correct_score=cs)
    dense = lc.check_labels(GOLD["boxes"], GOLD["scores"], GOLD["cons_iou"], GOLD["gt_boxes"], GOLD["gt_classes"], GOLD["classes"], **kw)
    check_against_golden(dense, ci)
    check_against_golden(lc.check_labels(GOLD["boxes"], GOLD["scores"], GOLD["cons_iou"], GOLD["gt_boxes"], GOLD["gt_classes"],
                                         md_rule="le", **kw), ci, "le")
    # the lists read_predictions returns: the kept rows only, the ground truth as lists of boxes
    keep = [np.where(GOLD["scores"][i] > kw["min_score"])[0] for i in range(len(GOLD["names"]))]
    rows = [np.where(GOLD["gt_classes"][i] > 0)[0] for i in range(len(GOLD["names"]))]
    ragged = lc.check_labels([GOLD["boxes"][i, k].tolist() for i, k in enumerate(keep)], [GOLD["scores"][i, k].tolist() for i, k in enumerate(keep)],
                             [GOLD["cons_iou"][i, k].tolist() for i, k in enumerate(keep)], [GOLD["gt_boxes"][i, r].tolist() for i, r in enumerate(rows)],
                             classes=[GOLD["classes"][i, k].tolist() for i, k in enumerate(keep)], **kw)
    check_against_golden(ragged, ci)
    src, files = _kitti_inputs(tmp_path)
    data = json.loads(str(GOLD["bdd_json"][0]))
    for tag, mode in MODES.items():
        for chk in (dense, ragged):
            out = tmp_path / ("k_%s_%d" % (tag, chk is ragged))
            writers.write_kitti_corrected_gt(src, str(out), files, list(GOLD["kitti_classes"]), check=chk, **mode)
            assert [open(out / f, newline="").read() for f in files] == [str(t) for t in GOLD["k%d_kitti_%s_texts" % (ci, tag)]]
        out = tmp_path / ("b_" + tag)
        writers.write_bdd_corrected_gt(data, str(out), [nm + ".jpg" for nm in GOLD["names"]], list(GOLD["bdd_classes"]), check=dense, **mode)
        assert open(out / "bdd100k_labels_images_train.json", newline="").read() == str(GOLD["k%d_bdd_%s_texts" % (ci, tag)][0])


# ------------------------------------------------------------------ on a handle
SIZE, RAW, SEED = "256x128", (140, 260), 23


def _driver(**over):
    from uda_amd.infer_lib import KerasDriver
    p = make_params(image_size=SIZE, **dict(FULL_MC, **over))
    d = KerasDriver("_", False, p["name"], 2, False, p, weights=make_weights(p, seed=12, cls_spread=20.0))
    d.set_dropout_seed(SEED)
    return d


@pytest.fixture(scope="module")
def cons_driver():
    d = _driver(consistency_ssl=True)
    yield d
    d.close()


def handle_gt(det, cons, min_score, G=9):
    """Ground truth from the run's own detections: jittered and exact copies of kept boxes, a far-away box, a class-0 row
    (not counted), padding."""
    rng = np.random.default_rng(3)
    n = det[0].shape[0]
    gb, gc = np.full((n, G, 4), -1, np.float32), np.full((n, G), -1, np.float32)
    for i in range(n):
        kept = np.where(det[1][i] > min_score)[0]
        order = kept[np.argsort(-cons[i, kept])]              # the most consistent first: some of them above iou_consist
        picks = list(order[:3]) + [kept[-1]]
        rowsb = [det[0][i, k, :4] + rng.normal(0, 0.4, 4).astype(np.float32) for k in picks]
        rowsb.insert(1, det[0][i, picks[0], :4] + np.float32([0, 0, 0, 1.5]))        # a second row on the same detection
        rowsb.insert(2, np.array([5000, 5000, 5100, 5200], np.float32))
        rowsb.append(det[0][i, kept[0], :4].copy())
        cls = [float(c) for c in rng.integers(1, 8, len(rowsb))]
        cls[3] = 0.0
        gb[i, :len(rowsb)], gc[i, :len(rowsb)] = np.stack(rowsb), cls
    return gb, gc


def check_handle(chk, det, cons, gb, gc, min_score, thr, methods=("md", "mistakes", "noisy")):
    from uda_amd import label_correction as lc
    want = R.check(det[0][..., :4], det[1], cons, gb, gc, min_score, thr["iou_consist"], 0, "eq", 1.0, thr["correct_score"], methods, f32=True)
    cls = det[2] if det[2].ndim == 2 else det[2][..., 0]
    ref = lc.LabelCheck.from_arrays(want, det[0][..., :4], gb, gc, cls, methods)
    np.testing.assert_array_equal(chk.counts, want["counts"])
    for k in ("wrong_gt", "extra_correct_dets", "matched_det", "noisy_rows", "replaced", "pred_ranks"):
        for a, b in zip(getattr(chk, k), getattr(ref, k)):
            np.testing.assert_array_equal(a, b, err_msg=k)
    for a, b in zip(chk.ious_gt + chk.det_max_iou, ref.ious_gt + ref.det_max_iou):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert chk.corrected_gt_boxes == ref.corrected_gt_boxes
    return want


def test_serve_label_check_matches_the_mirror(cons_driver):
    d = cons_driver
    imgs = make_images(2, *RAW, seed=3)
    det, cons, _ = d.serve_consistency(imgs)
    min_score = float(np.median(det[1]))                      # about half of every image's rows are kept
    thr = dict(iou_consist=float(np.median(cons[det[1] > min_score])), correct_score=min_score)
    gb, gc = handle_gt(det, cons, min_score)
    chk = d.serve_label_check(imgs, gb, gc, min_score=min_score, **thr)
    want = check_handle(chk, det, cons, gb, gc, min_score, thr)
    assert want["counts"][:, 2].min() >= 1 and want["counts"][:, 4].sum() > 0 and want["counts"][:, 3].sum() > 0
    assert 0 < want["counts"][0, 0] < d.M
    assert chk.pred_boxes[0] is not None and len(chk.pred_classes[0]) == want["counts"][0, 0]      # fetched: a missing label is flagged
    # on the resident run, without serving again: other thresholds, other methods, no detection columns
    thr2 = dict(iou_consist=0.0, correct_score=0.0)
    again = d.label_check(gb, gc, min_score=min_score, missing_boxes=False, **thr2)
    check_handle(again, det, cons, gb, gc, min_score, thr2)
    assert again.pred_boxes[0] is None
    same = d.label_check(gb, gc, min_score=min_score, **thr)
    check_handle(same, det, cons, gb, gc, min_score, thr)
    only = d.label_check(gb, gc, methods=("mistakes",), min_score=min_score)
    assert [list(w) for w in only.wrong_gt] == [list(w) for w in chk.wrong_gt] and not only.counts[:, 3:].any()
    # the default min_score is 0.1 (GLC's own inference writes with it) and the defaults are AdvancedLabels' own
    check_handle(d.label_check(gb, gc), det, cons, gb, gc, 0.1, dict(iou_consist=0.90, correct_score=0.40))


def test_handle_refusals(cons_driver):
    from uda_amd import capi
    d = cons_driver
    imgs = make_images(2, *RAW, seed=4)
    fresh = _driver(consistency_ssl=True)
    try:
        rc = fresh._lib.uda_label_check(fresh._h, 0.1, 0.9, 0.0, 0, 1.0, 0.4, 7)
        assert rc == 1 and b"no ground truth is set" in fresh._lib.uda_last_error(fresh._h)
        gb, gc = np.zeros((2, 3, 4), np.float32), np.ones((2, 3), np.float32)
        with pytest.raises(capi.UdaError, match="no global post-process has run yet"):
            fresh.label_check(gb, gc)
    finally:
        fresh.close()
    det, cons, _ = d.serve_consistency(imgs)
    gb, gc = handle_gt(det, cons, float(np.median(det[1])))
    with pytest.raises(capi.UdaError, match="ground truth of 1 images, the last post-process holds 2"):
        d.label_check(gb[:1], gc[:1])
    d.serve_consistency(imgs, post_mode="per_class")
    with pytest.raises(capi.UdaError, match="the last post-process ran per class; the label check reads the global post-process"):
        d.label_check(gb, gc)
    d.stage_images(imgs)
    ticket = d.run_async()
    with pytest.raises(capi.UdaError, match=r"label_check: a pipelined run \(uda_run_async\) is in flight"):
        d.label_check(gb, gc)
    d.collect(ticket)
    with pytest.raises(ValueError, match="unknown method"):
        d.label_check(gb, gc, methods=("noise",))
    with pytest.raises(ValueError, match="ground truth of 1 images for a batch of 2"):
        d.serve_label_check(imgs, gb[:1], gc[:1])


def test_mistakes_alone_after_a_plain_run():
    from uda_amd import capi
    d = _driver()
    try:
        imgs = make_images(2, *RAW, seed=3)
        det = d.serve(imgs)
        n = d.serve_resident(imgs)
        assert n == 2
        min_score = float(np.median(det[1]))
        gb, gc = handle_gt(det, np.zeros(det[1].shape), min_score)
        chk = d.label_check(gb, gc, methods=("mistakes",), min_score=min_score)
        want = R.check(det[0][..., :4], det[1], None, gb, gc, min_score, methods=("mistakes",), f32=True)
        np.testing.assert_array_equal(chk.counts, want["counts"])
        assert [list(w) for w in chk.wrong_gt] == [list(np.where(want["gt_flags"][i, gc[i] > 0] & R.GT_MISTAKE)[0]) for i in range(2)]
        assert chk.counts[:, 2].min() >= 1 and chk.methods == ("mistakes",)
        for methods in (("md",), ("mistakes", "noisy")):
            with pytest.raises(capi.UdaError, match="md and noisy read cons_iou, and the resident run is not a consistency run"):
                d.label_check(gb, gc, methods=methods, min_score=min_score)
        with pytest.raises(ValueError, match="consistency_ssl=True"):
            d.serve_label_check(imgs, gb, gc)
    finally:
        d.close()
