"""The post-thresholding analysis on the device (`post_thresholding.heat_np` -> `uda_heat_maps_np`, `post_np` -> `uda_thr_post_np`;
reference uncertainty_analysis.py:838-880, :920-1068) against the numpy mirrors (tests/thr_post_ref.py): every map, count, tally and
IoU sum bit for bit - at the tile seams, at the chunk boundaries, on an order-sensitive pixel, with 16 mixed maps in one call - and
every case of tests/golden/thr_post_golden.npz (what the reference's own methods produced) end to end through the device."""
import ctypes
import random

import numpy as np
import pytest

import test_thr_post_host as H
import thr_post_ref as PR
from uda_amd import capi
from uda_amd import post_thresholding as PT

pytestmark = pytest.mark.gpu

TH_, TW_, CH = PT.TILE_H, PT.TILE_W, PT.CHUNK
DEFAULT6 = [0.5, 0.55, 0.6, 0.65, 0.7, 0.75]


def both_heat(rects, values, sel, map_rect, map_value, map_sel, map_mean, Hm, Wm):
    args = (rects, values, sel, map_rect, map_value, map_sel, map_mean, Hm, Wm)
    (heat, cnt), (w_heat, w_cnt) = PT.heat_np(*args), PR.heat_np(*args)
    print("differing pixels: heat %d, count %d" % (int(np.sum(H.bits(heat) != H.bits(w_heat))), int(np.sum(cnt != w_cnt))))
    assert heat.shape == w_heat.shape and np.array_equal(H.bits(heat), H.bits(w_heat)) and np.array_equal(cnt, w_cnt)
    only_heat, none = PT.heat_np(*args, count=False)
    assert none is None and np.array_equal(H.bits(only_heat), H.bits(heat))
    return heat, cnt


def random_rects(rng, N, Hm, Wm):
    r = np.stack([rng.integers(0, Hm + 1, N), rng.integers(0, Hm + 1, N), rng.integers(0, Wm + 1, N), rng.integers(0, Wm + 1, N)], 1)
    return r.astype(np.int32)                               # about a quarter of them cover something


def pixel(y, x):
    return [y, y + 1, x, x + 1]


def test_four_tiles_and_their_seams():
    Hm, Wm, N = TH_ + 1, TW_ + 1, CH + 1
    rng = np.random.default_rng(1)
    rects = random_rects(rng, N, Hm, Wm)
    placed = [[0, Hm, 0, Wm], pixel(0, 0), pixel(0, Wm - 1), pixel(Hm - 1, 0), pixel(Hm - 1, Wm - 1),
              pixel(TH_ - 1, 5), pixel(TH_, 5), pixel(5, TW_ - 1), pixel(5, TW_), pixel(TH_ - 1, TW_ - 1), pixel(TH_, TW_),
              [TH_ - 3, TH_ + 1, TW_ - 7, TW_ + 1], [4, 4, 0, Wm], [0, Hm, 9, 9], [20, 3, 0, Wm], [0, Hm, 40, 2], [0, 0, 0, 0],
              [Hm, Hm, Wm, Wm]]
    where = rng.choice(N - 2, len(placed), replace=False)
    rects[where] = placed
    rects[N - 1] = [0, Hm, 0, Wm]                           # the one row of the second chunk covers every pixel
    values = rng.normal(0, 1, (2, N)) * 10.0 ** rng.integers(-3, 4, (2, N))
    sel = np.stack([rng.random(N) < 0.5, np.zeros(N, bool)])
    sel[0, where[0]] = False                                # the whole-map box is deselected in the maps that use selector 0
    heat, cnt = both_heat(rects, values, sel, [0] * 6, [0, 1, -1, 0, 1, 0], [-1, -1, -1, 0, 0, 1], [0, 1, 0, 0, 1, 1], Hm, Wm)
    assert (cnt[0] >= 2).all() and np.array_equal(heat[2], cnt[2].astype(np.float64))
    assert (cnt[5] == 0).all() and (heat[5] == 0).all() and not np.signbit(heat[5]).any()


@pytest.mark.parametrize("N", [1, CH - 1, CH, CH + 1])
def test_row_counts_at_the_chunk_boundary(N):
    Hm, Wm = TH_ + 7, 2 * TW_ + 3
    rng = np.random.default_rng(N)
    rects = random_rects(rng, N, Hm, Wm)
    rects[N - 1] = [0, Hm, 0, Wm]                           # the last row reaches every tile
    both_heat(rects, rng.normal(0, 1, (1, N)), rng.random((1, N)) < 0.8, [0, 0, 0], [0, 0, -1], [-1, 0, 0], [1, 0, 0], Hm, Wm)


def test_chunks_that_miss_a_tile_and_chunks_that_fill_it():
    Hm, Wm, N = 2 * TH_, 2 * TW_, 3 * CH
    rng = np.random.default_rng(3)
    rects = random_rects(rng, N, Hm, Wm)
    rects[:CH] = np.stack([rng.integers(0, TH_ // 2, CH), rng.integers(TH_ // 2, TH_ + 1, CH), rng.integers(0, TW_ // 2, CH),
                           rng.integers(TW_ // 2, TW_ + 1, CH)], 1)          # chunk 0 lies inside tile (0, 0) and meets it
    rects[CH:2 * CH, 0], rects[CH:2 * CH, 2] = rng.integers(0, TH_, CH), rng.integers(0, TW_, CH)
    rects[CH:2 * CH, 1], rects[CH:2 * CH, 3] = rng.integers(TH_ + 1, Hm + 1, CH), rng.integers(TW_ + 1, Wm + 1, CH)   # chunk 1 meets all four
    heat, cnt = both_heat(rects, rng.normal(0, 1, (1, N)), None, [0, 0], [0, -1], [-1, -1], [1, 0], Hm, Wm)
    assert cnt[1, TH_ - 1:TH_ + 1, TW_ - 1:TW_ + 1].min() >= CH


def test_the_sum_follows_the_row_order():
    n = 3 * CH + 5
    v = H.order_sensitive_rows(n)
    rects = np.zeros((n, 4), np.int32)
    rects[:, 0], rects[:, 1], rects[:, 2], rects[:, 3] = TH_, TH_ + 1, TW_ + 2, TW_ + 3       # one pixel of the last tile
    heat, cnt = both_heat(rects, v[None], None, [0, 0], [0, 0], [-1, -1], [0, 1], TH_ + 2, TW_ + 4)
    assert heat[0, TH_, TW_ + 2] == PR.fold(v) != np.sum(v) and cnt[0, TH_, TW_ + 2] == n and cnt[0].sum() == n


def test_one_pixel_map():
    rects = np.array([[0, 1, 0, 1], [0, 0, 0, 1], [1, 0, 0, 1], [0, 1, 0, 1]], np.int32)
    heat, cnt = both_heat(rects, np.array([[0.1, 5.0, 7.0, 0.2]]), None, [0, 0], [0, 0], [-1, -1], [0, 1], 1, 1)
    assert heat[:, 0, 0].tolist() == [0.0 + 0.1 + 0.2, (0.0 + 0.1 + 0.2) / 2] and cnt[:, 0, 0].tolist() == [2, 2]


def test_sixteen_mixed_maps_equal_sixteen_calls():
    Hm, Wm, N, M = 40, 90, 700, 16
    rng = np.random.default_rng(16)
    rects = np.stack([random_rects(rng, N, Hm, Wm) for _ in range(4)])
    values, sel = rng.normal(0, 3, (16, N)), rng.random((8, N)) < 0.6
    m_rect, m_value, m_sel = rng.integers(0, 4, M), rng.integers(-1, 16, M), rng.integers(-1, 8, M)
    m_value[:2], m_sel[:2], m_mean = -1, [-1, 3], rng.integers(0, 2, M)
    heat, cnt = both_heat(rects, values, sel, m_rect, m_value, m_sel, m_mean, Hm, Wm)
    for m in range(M):
        one, one_cnt = PT.heat_np(rects, values, sel, [m_rect[m]], [m_value[m]], [m_sel[m]], [m_mean[m]], Hm, Wm)
        assert np.array_equal(H.bits(one[0]), H.bits(heat[m])) and np.array_equal(one_cnt[0], cnt[m]), m


def test_mean_map_leaves_uncovered_pixels_at_plus_zero():
    rects = np.array([[2, 5, 3, 70], [4, 9, 60, 66]], np.int32)
    heat, cnt = both_heat(rects, np.array([[-2.5, -0.5]]), None, [0], [0], [-1], [1], 12, 80)
    assert (cnt[0] == 0).sum() == 12 * 80 - (3 * 67 + 5 * 6 - 6) and (heat[0][cnt[0] == 0] == 0).all()
    assert not np.signbit(heat[0][cnt[0] == 0]).any() and heat[0, 4, 60] == (0.0 + -2.5 + -0.5) / 2


def test_random_rectangles():
    Hm, Wm, N = 70, 130, 1000
    rng = np.random.default_rng(70)
    y, x = rng.integers(0, Hm, N), rng.integers(0, Wm, N)
    rects = np.stack([y, np.minimum(y + rng.integers(0, 30, N), Hm), x, np.minimum(x + rng.integers(0, 50, N), Wm)], 1).astype(np.int32)
    both_heat(rects, rng.gamma(2.0, 0.1, (2, N)), rng.random((1, N)) < 0.3, [0, 0, 0], [0, 1, -1], [-1, 0, -1], [1, 1, 0], Hm, Wm)


@pytest.mark.parametrize("c", H.CASES)
def test_device_reproduces_the_reference(c):
    g = H.gold_case(c)
    H.check_analysis(H.analyse(g, random.Random(g["seed"])), g)


def tally_problem(N, seed):
    rng = np.random.default_rng(seed)
    tp = rng.random(N) < 0.85
    ious = np.round(rng.uniform(0.05, 0.999, N), 3)
    u = np.round(rng.uniform(0, 1.2, N), 2)                 # two decimals: many rows sit exactly on a threshold
    return u, ious, tp


def both_post(u, ious, tp, iou_thrs, thrs, image=None, k_img=-1):
    got, want = PT.post_np(u, ious, tp, iou_thrs, thrs, image, k_img), PR.post_np(u, ious, tp, iou_thrs, thrs, image, k_img)
    assert np.array_equal(got[0], want[0]) and np.array_equal(H.bits(got[1]), H.bits(want[1]))
    if k_img < 0:
        assert got[2] is None and got[3] is None
    else:
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert (got[0][:, :, 0].sum(1) == u.size).all() and (got[0][:, :, 2] + got[0][:, :, 3] == got[0][:, :, 0]).all()
    return got


@pytest.mark.parametrize("N", [2, 63, 64, 65, 255, 256, 257, 2049])
def test_tallies_at_the_wave_and_block_boundaries(N):
    u, ious, tp = tally_problem(N, N)
    ious[0] = -0.0
    rng = np.random.default_rng(N + 1)
    n_img = max(1, N // 5)
    image = rng.integers(0, n_img, N)
    image[rng.integers(0, N)] = n_img - 1
    both_post(u, ious, tp, [0.5], [0.6], image, 0)
    thrs = [0.6, np.inf, -1.0, 5.0, 0.0, float(u[N // 2])]            # nothing removed, everything removed, a threshold on a row
    for k_img in (-1, 1, 2, 5):
        counts, _, img_count, _ = both_post(u, ious, tp, DEFAULT6, thrs, image, k_img)
        assert counts[1, 0].tolist() == [0, 0, 0, 0] and counts[3, 0, 0] == 0 and counts[2, 1, 0] == 0 and counts[4, 0, 0] == N
    assert img_count[:, 3].sum() == counts[5, 0, 0]
    both_post(u, ious, tp, [0.5], [0.6], np.arange(N), 0)             # images of one row
    got = both_post(u, ious, tp, [0.5], [0.6], np.zeros(N, np.int64), 0)   # one image holds every row
    assert got[2].shape == (1, 4) and got[2][0, 3] == got[0][0, 0, 0]


def test_null_outputs_are_skipped():
    N = 300
    u, ious, tp = tally_problem(N, 9)
    image = np.random.default_rng(9).integers(0, 20, N).astype(np.int32)
    image[0] = 19
    want = PR.post_np(u, ious, tp, [0.5, 0.75], [0.5, 0.7], image, 1)
    lib = capi.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                    # noqa: E731
    tp8, it, th = tp.astype(np.uint8), np.array([0.5, 0.75]), np.array([0.5, 0.7])
    for keep in range(4):
        outs = [np.zeros_like(w) for w in want]
        ptrs = [p(o) if j == keep else None for j, o in enumerate(outs)]
        assert lib.uda_thr_post_np(0, p(u), p(ious), p(tp8), p(image), N, 20, p(it), p(th), 2, 1, *ptrs) == 0
        assert outs[keep].tobytes() == want[keep].tobytes()
    assert lib.uda_thr_post_np(0, p(u), p(ious), p(tp8), None, N, 0, p(it), p(th), 2, -1, None, None, None, None) == 0


def test_refusals_leave_the_outputs_untouched_and_the_device_usable():
    H.test_library_refuses_before_it_touches_a_device()
    with pytest.raises(capi.UdaError):
        lib = capi.load()
        rects = np.array([[0, 9, 0, 1]], np.int32)
        heat = np.full((1, 4, 4), 7.0)
        tab = np.zeros(1, np.int32)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                # noqa: E731
        rc = lib.uda_heat_maps_np(0, p(rects), 1, None, 0, None, 0, 1, p(tab), p(tab - 1), p(tab - 1), p(tab), 1, 4, 4, p(heat), None)
        assert (heat == 7.0).all()
        capi.check(lib, None, rc, "uda_heat_maps_np")
    heat, cnt = both_heat(np.array([[0, 4, 0, 1]], np.int32), None, None, [0], [-1], [-1], [0], 4, 4)
    assert heat[0, :, 0].tolist() == [1.0] * 4 and cnt.sum() == 4
