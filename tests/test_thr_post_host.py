"""The post-thresholding analysis, host side (`uda_amd.post_thresholding`: box_slices, heat_maps, spider_metrics, rank_images,
post_threshold_analysis; reference uncertainty_analysis.py:838-880, :920-1068): the numpy mirrors (tests/thr_post_ref.py,
tests/thr_report_ref.py) standing in for the device through `heat=` / `post=` / `report=`, against what the reference's own methods
produced (tests/golden/thr_post_golden.npz), and the refusals.

Bounds.  Every map is numpy's slice += loop in the same order: bit-equal.  The spider's columns 1-4 are integer ratios put through
the reference's own numpy operations: bit-equal.  Column 0 averages sums of N positive IoUs taken in two orders, each within
(N - 1) * 2^-53 of the exact sum relatively: the two differ by at most 2 * N * 2^-53, and so do their quotients and means."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import thr_post_ref as PR
import thr_report_ref as RR
from uda_amd import capi
from uda_amd import post_thresholding as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "thr_post_golden.npz"))
CASES = [str(c) for c in GOLD["cases"]]
RANKED = [c for c in CASES if c + "_image_names" in GOLD.files]
MASK = tuple(int(v) for v in GOLD["mask_size"])


def gold_case(c):
    g = {}
    for k in ("gt_boxes", "pred_boxes", "albox", "calib_albox", "entropy", "calib_entropy", "opt_uncert", "ious"):
        g[k] = GOLD["%s_%s" % (c, k)].astype(np.float64) if "%s_%s" % (c, k) in GOLD.files else None
    g["tp_class"] = GOLD[c + "_tp_class"].astype(bool)
    g["image_names"] = GOLD[c + "_image_names"] if c in RANKED else None
    g["iou_thrs"], g["seed"] = [float(t) for t in GOLD[c + "_iou_thrs"]], int(GOLD[c + "_seed"])
    g["params"] = {"thr_cd": bool(GOLD[c + "_fix_cd"]), "thr_fpr_tpr": float(GOLD[c + "_budget"]), "thr_iou_thrs": g["iou_thrs"]}
    g["maps"] = {k[len(c) + 5:]: GOLD[k] for k in GOLD.files if k.startswith(c + "_map_")}
    g["spider"], g["collect_thr"], g["collect_counts"] = GOLD[c + "_spider"], float(GOLD[c + "_collect_thr"]), GOLD[c + "_collect_counts"]
    g["lists"] = {k: [str(v) for v in GOLD["%s_list_%s" % (c, k)]] for k in PT.LIST_KEYS} if c in RANKED else None
    return g


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_analysis(out, g):
    """What post_threshold_analysis returned against the fixture (the lists only where the case ranks images)."""
    N = g["opt_uncert"].size
    assert sorted(out["heat"]) == sorted(g["maps"])
    for key, want in g["maps"].items():
        got = out["heat"][key]
        print(key, "differing pixels:", int(np.sum(bits(got) != bits(want))))
        assert got.shape == MASK and np.array_equal(bits(got), bits(want)), key
    sp, want = out["spider"], g["spider"]
    assert sp.shape == (3, 5) and np.array_equal(bits(sp[:, 1:]), bits(want[:, 1:]))
    err = np.max(np.abs(sp[:, 0] - want[:, 0]) / np.abs(want[:, 0]))
    print("mIoU relative error %.3g of the bound %.3g" % (err, 2 * N * 2.0 ** -53))
    assert err <= 2 * N * 2.0 ** -53
    if g["lists"] is not None:
        assert out["images"] == g["lists"]


def analyse(g, rng, **stand_ins):
    names = g["image_names"] if g["image_names"] is not None else np.array(["a.png", "b.png"])[np.arange(g["ious"].size) % 2]
    return PT.post_threshold_analysis(g["gt_boxes"], g["pred_boxes"], MASK, names, g["opt_uncert"], g["ious"], g["tp_class"],
                                      params=g["params"], albox=g["albox"], calib_albox=g["calib_albox"], entropy=g["entropy"],
                                      calib_entropy=g["calib_entropy"], rng=rng, **stand_ins)


MIRRORS = dict(heat=PR.heat_np, post=PR.post_np, report=RR.report_np)


def test_fixture_covers_what_it_should():
    gs = {c: gold_case(c) for c in CASES}
    assert sorted(g["ious"].size for g in gs.values()) == [2, 65, 1025, 3000] and MASK == (37, 53)
    assert [c for c, g in gs.items() if g["calib_albox"] is None] == ["n65_nocalib"] and len(RANKED) == 3
    assert sorted(gs["n3000"]["maps"]) == sorted(PT.HEAT_KEYS) and len(gs["n65_nocalib"]["maps"]) == 7
    boxes = np.concatenate([gs["n3000"]["gt_boxes"], gs["n3000"]["pred_boxes"]])
    assert (boxes < 0).any() and (boxes[:, 2] > MASK[0]).any() and (boxes[:, 3] > MASK[1]).any()
    assert (boxes[:, 2] == boxes[:, 0]).any() and (boxes[:, 2] < boxes[:, 0]).any() and (boxes[:, 3] < boxes[:, 1]).any()
    frac = boxes - np.round(boxes)
    assert ((frac > 0) & (frac < 1e-5)).any() and ((frac < 0) & (frac > -1e-5)).any()
    for c in RANKED:                                        # the tie rule and the sample are exercised
        g = gs[c]
        thr, u, names = g["collect_thr"], g["opt_uncert"], g["image_names"]
        assert sum(bool(np.all(u[names == n] < thr)) for n in np.unique(names)) >= 12
        assert len(g["lists"]["random_noremoval"]) == 10


def test_module_constants_mirror_the_header():
    src = open(capi.HEADER).read()
    defined = {k: int(v) for k, v in re.findall(r"#define UDA_HEAT_(\w+) (\d+)", src)}
    assert defined == dict(TILE_H=PT.TILE_H, TILE_W=PT.TILE_W, CHUNK=PT.CHUNK, MAX_MAPS=PT.MAX_MAPS, MAX_RECTS=PT.MAX_RECTS,
                           MAX_VALUES=PT.MAX_VALUES, MAX_SELS=PT.MAX_SELS, MAX_PIXELS=PT.MAX_PIXELS)
    assert (PT.TILE_H * PT.TILE_W) % PT.CHUNK == 0 and PT.CHUNK % PT.TILE_W == 0


def test_box_slices_resolve_like_python_slices():
    rng = np.random.default_rng(0)
    for size in (1, 37, 53, 720):
        v = np.concatenate([rng.uniform(-3 * size, 3 * size, 700), rng.integers(-2 * size, 2 * size + 1, 700).astype(np.float64),
                            rng.integers(-2 * size, 2 * size + 1, 90) + rng.choice([-1e-9, 1e-9, 0.5, -0.5], 90),
                            [1e300, -1e300, 0.5, -0.5, -0.0, 0.0, size, -size, size + 0.5, -size - 0.5]])
        a, b = v, rng.permutation(v)
        boxes = np.stack([a, a, b, b], 1)
        got = PT.box_slices(boxes, size, size)
        for i in range(len(v)):
            lo, hi, _ = slice(int(a[i]), int(b[i])).indices(size)
            assert tuple(got[i]) == (lo, hi, lo, hi), (size, a[i], b[i], got[i])
    assert PT.box_slices(np.zeros((0, 4)), 3, 3).shape == (0, 4) and PT.box_slices([[0, 1, 2, 3]], 5, 7).dtype == np.int32
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            PT.box_slices([[0, 0, bad, 1]], 5, 5)


@pytest.mark.parametrize("c", CASES)
def test_mirrors_reproduce_the_reference(c):
    g = gold_case(c)
    check_analysis(analyse(g, random.Random(g["seed"]), **MIRRORS), g)


@pytest.mark.parametrize("c", RANKED)
def test_rank_images_default_rng_is_the_random_module(c):
    g = gold_case(c)
    random.seed(g["seed"])
    got = PT.rank_images(g["image_names"], g["opt_uncert"], g["ious"], g["tp_class"], max(g["iou_thrs"]), params=g["params"],
                         report=RR.report_np, post=PR.post_np)
    assert got == g["lists"]


def test_rank_images_with_few_untouched_images_takes_them_all():
    g = gold_case("n65_nocalib")
    got = PT.rank_images(g["image_names"], g["opt_uncert"], g["ious"], g["tp_class"], max(g["iou_thrs"]), params=g["params"], top=1000,
                         rng=random.Random(1), report=RR.report_np, post=PR.post_np)
    u, names = g["opt_uncert"], g["image_names"]
    untouched = sorted(str(n) for n in np.unique(names) if np.all(u[names == n] < g["collect_thr"]))
    assert sorted(got["random_noremoval"]) == untouched and len(untouched) < 1000
    assert len(got["top_correctremove"]) == len({str(n) for n in names[(u >= g["collect_thr"]) & ~(g["tp_class"] & (g["ious"] >= 0.75))]})


def test_heat_maps_return_only_what_their_inputs_allow():
    g = gold_case("n1025")
    only = PT.heat_maps(g["gt_boxes"], g["pred_boxes"], MASK, heat=PR.heat_np)
    assert list(only) == ["gt_loc"] and np.array_equal(bits(only["gt_loc"]), bits(g["maps"]["gt_loc"]))
    calls = []

    def counting(*a, **kw):
        calls.append(len(a[3]))
        return PR.heat_np(*a, **kw)

    some = PT.heat_maps(g["gt_boxes"], g["pred_boxes"], MASK, entropy=g["entropy"], calib_albox=g["calib_albox"], heat=counting)
    assert list(some) == ["gt_loc", "uncert_calib_albox", "rmse_calib_albox", "entropy"] and calls == [4]
    for k, v in some.items():
        assert np.array_equal(bits(v), bits(g["maps"][k])), k


def order_sensitive_rows(n):
    """n rows over one pixel whose values mix 1e16, 1 and -1e16: the sequential fold and numpy's pairwise sum differ."""
    v = np.tile([1e16, 1.0, -1e16, 1.0, 1.0], n // 5 + 1)[:n]
    assert np.sum(v) != PR.fold(v)
    return v


def test_mirror_follows_the_row_order():
    n = 3 * PT.CHUNK + 5
    v = order_sensitive_rows(n)
    rects = np.zeros((n, 4), np.int32)
    rects[:, 1], rects[:, 3] = 1, 1                         # every row covers pixel (0, 0) of a 2 x 2 map
    heat, cnt = PR.heat_np(rects, v[None], None, [0, 0], [0, 0], [-1, -1], [0, 1], 2, 2)
    assert heat[0, 0, 0] == PR.fold(v) and heat[0, 0, 0] != np.sum(v) and cnt[0, 0, 0] == n
    assert heat[1, 0, 0] == PR.fold(v) / n and (heat[:, 1, 1] == 0).all() and not np.signbit(heat[:, 1, 1]).any()
    by_value = np.sort(v)                                   # the same rows in another order give another sum
    assert PR.heat_np(rects, by_value[None], None, [0], [0], [-1], [0], 2, 2)[0][0, 0, 0] == PR.fold(by_value) != PR.fold(v)


def test_post_mirror_counts_and_image_tallies():
    u = np.array([0.9, 0.1, 0.5, 0.5, 0.2, 0.8])
    ious = np.array([0.9, 0.9, 0.6, 0.4, 0.9, 0.9])
    tp = np.array([1, 1, 1, 1, 0, 1], bool)
    image = np.array([2, 0, 2, 2, 1, 0])
    counts, iou_sum, img_count, img_first = PR.post_np(u, ious, tp, [0.5, 0.95], [0.5, np.inf], image=image, k_img=0)
    assert counts[0].tolist() == [[4, 4, 3, 1], [2, 1, 1, 1]] and counts[1].tolist() == [[0, 0, 0, 0], [6, 5, 0, 6]]
    assert iou_sum[0, 0] == (0.9 + 0.0) + (0.6 + 0.4) + 0.9 and iou_sum[1, 0] == 0.0
    assert img_count.tolist() == [[0, 1, 0, 1], [0, 0, 1, 0], [1, 2, 0, 3]]
    assert img_first.tolist() == [[6, 5, 6], [6, 6, 4], [3, 0, 6]]


def test_python_refusals():
    r = np.zeros((1, 3, 4), np.int32)
    ok = dict(rects=r, values=np.ones((1, 3)), sel=None, map_rect=[0], map_value=[0], map_sel=[-1], map_mean=[0], H=4, W=4)
    PT.check_heat_problem(**ok)
    bad_rect = r.copy()
    bad_rect[0, 1, 1] = 5
    for change in (dict(rects=bad_rect), dict(rects=-1 - r), dict(values=np.full((1, 3), np.nan)), dict(map_value=[1]), dict(map_sel=[0]),
                   dict(map_rect=[1]), dict(map_rect=[0, 0]), dict(H=0), dict(H=4096, W=1025), dict(rects=np.zeros((5, 3, 4))),
                   dict(map_rect=[0] * 17, map_value=[0] * 17, map_sel=[-1] * 17, map_mean=[0] * 17), dict(rects=np.zeros((3, 3)))):
        with pytest.raises(ValueError):
            PT.check_heat_problem(**dict(ok, **change))
    u, iou, tp = np.array([0.1, 0.2]), np.array([0.5, 0.6]), [1, 0]
    PT.check_post_problem(u, iou, tp, [0.5], [np.inf])
    for args, kw in (((u[:1], iou[:1], tp[:1], [0.5], [0.1]), {}), ((u, iou, tp, [0.5], [np.nan]), {}),
                     ((np.array([np.nan, 1]), iou, tp, [0.5], [0.1]), {}), ((u, iou, tp, [0.5, 0.6], [0.1]), {}),
                     ((u, iou, tp, [0.5], [0.1]), dict(k_img=1)), ((u, iou, tp, [0.5], [0.1]), dict(k_img=0)),
                     ((u, iou, tp, [0.5], [0.1]), dict(k_img=0, image=[0, 2])), ((u, iou, tp, [0.5], [0.1]), dict(k_img=0, image=[-1, 0])),
                     ((u, iou, tp, [0.5] * 33, [0.1] * 33), {})):
        with pytest.raises(ValueError):
            PT.check_post_problem(*args, **kw)
    with pytest.raises(ValueError):
        PT.heat_maps(np.zeros((2, 4)), np.zeros((3, 4)), (4, 4), heat=PR.heat_np)
    with pytest.raises(ValueError):
        PT.rank_images(["a"], u, iou, tp, 0.5, report=RR.report_np, post=PR.post_np)


def test_library_refuses_before_it_touches_a_device():
    """The C entry points check everything on the host first: each refusal names the entry point and leaves the sentinel-filled
    outputs as they were (no GPU is needed to be refused)."""
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    lib = capi.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                    # noqa: E731
    N, H, W = 3, 4, 5
    rects, values, sel = np.zeros((1, N, 4), np.int32), np.ones((1, N)), np.ones((1, N), np.uint8)
    tabs = [np.zeros(1, np.int32) for _ in range(4)]
    heat, count = np.full((1, H, W), 7.0), np.full((1, H, W), 7, np.int32)

    def call(rects=rects, R=1, V=1, Q=1, N=N, tabs=tabs, M=1, H=H, W=W):
        return lib.uda_heat_maps_np(0, p(rects), R, p(values), V, p(sel), Q, N, p(tabs[0]), p(tabs[1]), p(tabs[2]), p(tabs[3]), M, H, W,
                                    p(heat), p(count))

    outside = rects.copy()
    outside[0, 2] = [0, H + 1, 0, 1]
    negative = rects.copy()
    negative[0, 0] = [0, 1, -1, 1]
    for kw in (dict(N=0), dict(N=capi.THR_MAX_N + 1), dict(M=0), dict(M=17), dict(R=0), dict(R=5), dict(V=17), dict(Q=9), dict(H=0),
               dict(W=0), dict(H=4096, W=1025), dict(rects=outside), dict(rects=negative),
               dict(tabs=[np.ones(1, np.int32)] + tabs[1:]), dict(tabs=[tabs[0], np.ones(1, np.int32)] + tabs[2:]),
               dict(tabs=tabs[:2] + [np.ones(1, np.int32), tabs[3]]), dict(tabs=[tabs[0], np.full(1, -2, np.int32)] + tabs[2:])):
        assert call(**kw) == 1, kw
        assert lib.uda_last_error(None).decode().startswith("uda_heat_maps_np: "), kw
    assert (heat == 7.0).all() and (count == 7).all()

    u, iou, tp, image = np.array([0.1, 0.2, 0.3]), np.array([0.5, 0.6, 0.7]), np.ones(3, np.uint8), np.zeros(3, np.int32)
    thr = np.array([0.5])
    outs = [np.full((1, 2, 4), 7, np.int64), np.full((1, 2), 7.0), np.full((3, 4), 7, np.int32), np.full((3, 3), 7, np.int32)]

    def post(u=u, iou=iou, image=image, N=3, I=1, iou_thr=thr, thr=thr, K=1, k_img=0):
        return lib.uda_thr_post_np(0, p(u), p(iou), p(tp), p(image) if image is not None else None, N, I, p(iou_thr), p(thr), K, k_img,
                                   *[p(o) for o in outs])

    nan = np.array([np.nan])
    for kw in (dict(N=1), dict(N=capi.THR_MAX_N + 1), dict(K=0), dict(K=33), dict(k_img=1), dict(k_img=-2), dict(image=None),
               dict(I=0), dict(I=4), dict(image=np.array([0, 1, 0], np.int32)), dict(image=np.array([0, -1, 0], np.int32)),
               dict(thr=nan), dict(iou_thr=nan), dict(u=np.array([0.1, np.nan, 0.3])), dict(iou=np.array([0.1, 0.2, np.nan]))):
        assert post(**kw) == 1, kw
        assert lib.uda_last_error(None).decode().startswith("uda_thr_post_np: "), kw
    assert all((o == 7).all() for o in outs)
