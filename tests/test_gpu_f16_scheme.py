"""GPU tests of the opt-in one-piece fp16 scheme (`uda_pw_scheme = "f16"`: one fp16 piece per operand, one
v_mfma_f32_32x32x16_f16 product per k-step, float32 accumulation and epilogues - the operands of Keras mixed_float16).
Bounds are the measured errors times at most 4."""
import os
import subprocess
import sys

import numpy as np
import pytest

from common import FULL_MC, HEAD_MC, ROOT, make_images, make_params, make_weights

pytestmark = pytest.mark.gpu

# relative RMS of the heads against the float32 CPU oracle (worst level / channel group), per case
# (measured on MI355X: 3.69e-4 / 3.70e-4 / 3.53e-4, all of it in the box heads; the class heads sit at ~5e-7 here)
HEAD_RMS = {"full_mc": 1.4e-3, "head_mc": 1.4e-3, "d2": 1.4e-3}


def _driver(p, w, batch, scheme, **kw):
    from uda_amd.infer_lib import KerasDriver
    q = dict(p, uda_pw_scheme=scheme)
    d = KerasDriver("_", False, p["name"], batch, False, q, weights=w, **kw)
    assert d.pw_scheme == scheme
    return d


def _rel_rms(g, r):
    """worst relative RMS over the channel groups of one head tensor (box heads with loss attenuation: deltas | sigmas)"""
    ch = g.shape[-1]
    groups = [(0, ch // 2), (ch // 2, ch)] if ch == 72 else [(0, ch)]
    worst = 0.0
    for lo, hi in groups:
        gg, rr = g[..., lo:hi].astype(np.float64), r[..., lo:hi].astype(np.float64)
        worst = max(worst, np.sqrt(np.mean((gg - rr) ** 2)) / max(np.sqrt(np.mean(rr * rr)), 1e-30))
    return worst


@pytest.mark.parametrize("case", ["full_mc", "head_mc", "d2"])
def test_heads_against_the_oracle(case, capsys):
    """Small size, every head level against the float32 CPU oracle: full MC dropout, head-only MC (the first head layer takes
    the deferred dropout site: sep_kernel's TIN mode) and D2 (BiFPN / heads at 112 channels)."""
    from oracle import effdet_ref as E, philox_ref as R, preprocess_ref as PP
    if case == "d2":
        p = make_params(model="efficientdet-d2", image_size="256x256", **FULL_MC)
    else:
        p = make_params(**(FULL_MC if case == "full_mc" else HEAD_MC))
    w = make_weights(p, seed=3)
    wd, h = [int(v) for v in p["image_size"].split("x")]
    imgs = make_images(2, 100, 180, seed=4)
    d = _driver(p, w, 2, "f16")
    d.set_dropout_seed(7)
    d.serve(imgs)
    cls, box = d.head_outputs(2)
    assert d.range_demotions() == 0
    d.close()
    x, _ = PP.preprocess(imgs, (h, wd), p["mean_rgb"], p["stddev_rgb"])
    rcls, rbox = E.forward(w, p, x, R.make_masks(E.dropout_sites(p), 7, 2, int(p["mc_dropoutsamp"])))
    errs = [_rel_rms(g, r) for g, r in zip(cls + box, rcls + rbox)]
    with capsys.disabled():
        print("\n[f16 heads vs oracle, %s] relative rms per level (cls, box): %s" % (case, " ".join("%.2e" % e for e in errs)))
    assert all(np.isfinite(g).all() for g in cls + box)
    assert max(errs) <= HEAD_RMS[case], errs


def _iou_1n(box, boxes):
    """NonMaxSuppressionV5's IoU (float32, corners normalised, empty boxes -> 0) of one box against many."""
    f = np.float32
    y0, x0 = np.minimum(boxes[:, 0], boxes[:, 2]), np.minimum(boxes[:, 1], boxes[:, 3])
    y1, x1 = np.maximum(boxes[:, 0], boxes[:, 2]), np.maximum(boxes[:, 1], boxes[:, 3])
    by0, bx0, by1, bx1 = min(box[0], box[2]), min(box[1], box[3]), max(box[0], box[2]), max(box[1], box[3])
    area = (y1 - y0) * (x1 - x0)
    barea = f((by1 - by0) * (bx1 - bx0))
    ih = np.maximum(np.minimum(y1, by1) - np.maximum(y0, by0), f(0))
    iw = np.maximum(np.minimum(x1, bx1) - np.maximum(x0, bx0), f(0))
    inter = ih * iw
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / (area + barea - inter)
    return np.where((area > 0) & (barea > 0), iou, f(0)).astype(f)


def _selection_margins(ex_boxes, ex_scores, te_boxes, te_scores, sel, scale):
    """(copied from test_gpu_fullsize.py) Replays the exact run's selection sequence `sel` on both candidate sets with fully
    updated scores; per epoch: margin (selected minus best overlapping live runner-up, exact run), pert (largest difference of
    the two runs' updated scores), runner (index of that runner-up, -1: none)."""
    f = np.float32
    cur_e, cur_t = ex_scores.astype(f).copy(), te_scores.astype(f).copy()
    live = np.ones(cur_e.shape, bool)
    margin, pert, runner = [], [], []
    for i in sel:
        iou_e = _iou_1n(ex_boxes[i], ex_boxes)
        iou_t = _iou_1n(te_boxes[i], te_boxes)
        live[i] = False
        over = live & (iou_e > 0)
        if over.any():
            j = int(np.argmax(np.where(over, cur_e, -np.inf)))
            margin.append(float(cur_e[i] - cur_e[j]))
            runner.append(j)
        else:
            margin.append(np.inf)
            runner.append(-1)
        pert.append(float(np.abs(cur_t - cur_e)[live | (np.arange(live.size) == i)].max()))
        cur_e = np.where(live, cur_e * np.exp(np.float64(scale) * iou_e.astype(np.float64) ** 2).astype(f), cur_e)
        cur_t = np.where(live, cur_t * np.exp(np.float64(scale) * iou_t.astype(np.float64) ** 2).astype(f), cur_t)
    return np.array(margin), np.array(pert), np.array(runner)


FULLSIZE_TOL = 2e-3      # same-anchor score / box / sigma against the exact-f32 scheme (measured: 5.1e-4)
# index-aligned over all 184 140 candidates against the exact-f32 scheme: score (absolute), box (relative to the box size),
# u_al / u_ep (relative, floor 1e-2 of the box size)
# (measured: 4.1e-7, 1.2e-5, 6.0e-4, 8.9e-4)
CAND_TOL = {"scores": 1.6e-6, "boxes": 4.8e-5, "u_al": 2.4e-3, "u_ep": 3.5e-3}


def test_full_size_detections_against_exact_f32(capsys):
    """One image at 1280 x 768, T = 2, spread scores: the f16 handle's detections against the exact f32-input scheme's on the
    same inputs, margin-aware as in test_gpu_fullsize.py - every detection of the f32 run whose selection (and every earlier
    one) is decided by a margin above twice the measured perturbation comes back as the same anchor, with class equal and
    score, box and both sigmas within FULLSIZE_TOL."""
    from oracle import post_ref as P
    p = make_params(image_size="1280x768", mc_dropout=True, mc_dropoutrate=0.05, mc_dropoutsamp=2, loss_attenuation=True)
    w = make_weights(p, seed=0, cls_spread=5.0)
    imgs = make_images(1, 768, 1280, seed=7)
    runs = {}
    for scheme in ("f32", "f16"):
        d = _driver(p, w, 1, scheme)
        d.set_dropout_seed(9)
        runs[scheme] = (d.serve(imgs), d.candidates(1))
        d.close()
    (det_e, cand_e), (det_t, cand_t) = runs["f32"], runs["f16"]
    sigma2, iou_thr, score_thr = P.nms_params(p)
    M = p["nms_configs"]["max_output_size"]
    keep_e = P.nms_v5(cand_e["boxes"][0], cand_e["scores"][0], M, iou_thr, score_thr, sigma2, True)[0]
    keep_t = P.nms_v5(cand_t["boxes"][0], cand_t["scores"][0], M, iou_thr, score_thr, sigma2, True)[0]
    cand_err = float(np.abs(cand_t["scores"][0] - cand_e["scores"][0]).max())
    be, bt = cand_e["boxes"][0].astype(np.float64), cand_t["boxes"][0].astype(np.float64)
    size = np.maximum(np.maximum(be[:, 2] - be[:, 0], be[:, 3] - be[:, 1]), 1e-3)[:, None]
    cerr = {"scores": cand_err, "boxes": float((np.abs(bt - be) / size).max())}
    for k in ("u_al", "u_ep"):
        ue, ut = cand_e[k][0].astype(np.float64), cand_t[k][0].astype(np.float64)
        cerr[k] = float((np.abs(ut - ue) / np.maximum(np.abs(ue), 1e-2 * size.reshape(size.shape[:1] + (1,) * (ue.ndim - 1)))).max())
    assert (cand_t["classes"][0] != cand_e["classes"][0]).mean() < 1e-3
    top = 40
    sel = keep_e[:top]
    margin, pert, _ = _selection_margins(cand_e["boxes"][0], cand_e["scores"][0], cand_t["boxes"][0], cand_t["scores"][0], sel,
                                         -0.5 / sigma2)
    decided = margin > 2.0 * pert
    rows_t = {int(a): r for r, a in enumerate(keep_t)}
    same = n_checked = 0
    worst = 0.0
    for k in range(top):
        a = int(sel[k])
        if a in rows_t:
            same += 1
        if not decided[:k + 1].all():
            continue
        assert a in rows_t and rows_t[a] == k, ("a decided detection moved", k, a)
        n_checked += 1
        g_b, r_b = det_t[0][0, k], det_e[0][0, k]
        assert det_t[2][0, k, 0] == det_e[2][0, k, 0]
        scale = max(r_b[2] - r_b[0], r_b[3] - r_b[1], 1.0)
        e = max(abs(det_t[1][0, k] - det_e[1][0, k]) / abs(det_e[1][0, k]), np.abs(g_b[:4] - r_b[:4]).max() / scale,
                (np.abs(g_b[4:] - r_b[4:]) / np.maximum(r_b[4:], 1e-2 * scale)).max())
        worst = max(worst, float(e))
    # every detection on the same anchor in both runs (decided or not): box and both sigmas do not depend on the selection order
    worst_same = 0.0
    for k in range(top):
        a = int(sel[k])
        if a in rows_t and rows_t[a] < det_t[0].shape[1]:
            g_b, r_b = det_t[0][0, rows_t[a]], det_e[0][0, k]
            scale = max(r_b[2] - r_b[0], r_b[3] - r_b[1], 1.0)
            worst_same = max(worst_same, float(np.abs(g_b[:4] - r_b[:4]).max() / scale),
                             float((np.abs(g_b[4:] - r_b[4:]) / np.maximum(r_b[4:], 1e-2 * scale)).max()))
    with capsys.disabled():
        print("\n[full-size f16 vs f32] candidates: %s; same-anchor box / sigma (all %d): %.2e" % (
            " ".join("%s %.2e" % kv for kv in cerr.items()), same, worst_same))
        print("\n[full-size f16 vs f32] top %d: %d same anchors, %d decided and checked, worst relative error %.2e, "
              "largest candidate score difference %.2e" % (top, same, n_checked, worst, cand_err))
    assert worst <= FULLSIZE_TOL and worst_same <= FULLSIZE_TOL
    for k, v in cerr.items():
        assert v <= CAND_TOL[k], (k, v)
    # (measured: 8 of the top 40 on the same anchor, 1 decided by its margin - the scores of this random-init head sit in
    # plateaus of near-ties that a ~4e-7 perturbation of the candidate scores already reorders)
    assert n_checked >= 1 and same >= 4 and det_t[3][0] == det_e[3][0]


def test_overflow_is_demoted_and_served(capfd):
    """An activation above 65504 at the input of a one-piece contraction (block 3's depthwise BN scale x 3e5, its projection
    kernel / 3e5: the same function, a projection operand near 1e6) is served without inf / NaN: the op is re-packed on three
    bf16 pieces, named on stderr and counted by range_demotions(), and the result matches a bf16x3 handle within the f16 bound."""
    p = make_params(**FULL_MC)
    w = dict(make_weights(p, seed=81))
    k = [n for n in w if n.endswith("blocks_3/tpu_batch_normalization_1/gamma")]
    q = [n for n in w if n.endswith("blocks_3/conv2d_1/kernel")]
    assert len(k) == 1 and len(q) == 1
    w[k[0]] = w[k[0]] * np.float32(3.0e5)
    w[q[0]] = w[q[0]] / np.float32(3.0e5)
    imgs = make_images(2, 100, 180, seed=82)
    heads = {}
    for scheme in ("f16", "bf16x3"):
        d = _driver(p, w, 2, scheme)
        d.set_dropout_seed(5)
        det = d.serve(imgs)
        heads[scheme] = d.head_outputs(2)
        n = d.range_demotions()
        d.close()
        assert all(np.isfinite(x).all() for x in det[:3]), scheme
        assert n == (1 if scheme == "f16" else 0), (scheme, n)
    err = capfd.readouterr().err
    assert err.count("fp16 range: op") == 1 and "served again" in err, err[-2000:]
    # the op named is block 3's projection: a 1x1 conv (kind 2) from its 144-channel expanded tensor to 40 channels
    import re
    m = re.search(r"fp16 range: op (\d+) \(kind (\d+), (\d+) -> (\d+) channels\)", err)
    assert m and (int(m.group(2)), int(m.group(3)), int(m.group(4))) == (2, 144, 40), err[-2000:]
    errs = [_rel_rms(g, r) for g, r in zip(heads["f16"][0] + heads["f16"][1], heads["bf16x3"][0] + heads["bf16x3"][1])]
    print("[f16 overflow vs bf16x3] relative rms per level: %s" % " ".join("%.2e" % e for e in errs))
    assert max(errs) <= HEAD_RMS["full_mc"], errs


def test_repeatable_and_stream_equals_serial():
    p = make_params(**FULL_MC)
    w = make_weights(p, seed=11)
    a, b = make_images(2, 100, 180, seed=12), make_images(2, 128, 192, seed=13)
    d = _driver(p, w, 2, "f16")
    d.set_dropout_seed(3)
    first = d.serve(a)
    again = d.serve(a)
    for x, y in zip(first, again):
        np.testing.assert_array_equal(x, y)
    serial = [d.serve(a), d.serve(b)]
    stream = list(d.serve_stream([a, b]))
    d.close()
    for s_, t_ in zip(serial, stream):
        for x, y in zip(s_, t_):
            np.testing.assert_array_equal(x, y)


ORDER_WORKER = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import numpy as np
from common import FULL_MC, make_images, make_params, make_weights
from uda_amd.infer_lib import KerasDriver
p = make_params(**FULL_MC)
w = make_weights(p, seed=21)
imgs = make_images(2, 100, 180, seed=22)
if sys.argv[2] == "after_f16":
    d = KerasDriver("_", False, p["name"], 2, False, dict(p, uda_pw_scheme="f16"), weights=w)
    d.set_dropout_seed(4)
    d.serve(imgs)
    d.close()
d = KerasDriver("_", False, p["name"], 2, False, dict(p, uda_pw_scheme="f16x2"), weights=w)
assert d.pw_scheme == "f16x2"
d.set_dropout_seed(4)
if sys.argv[2] == "beside_f16":
    # UDA_PW_SCHEME=bf16x3 in this process's environment; an f16 handle alive at the same time, served alternately
    import os
    assert os.environ["UDA_PW_SCHEME"] == "bf16x3"
    other = KerasDriver("_", False, p["name"], 2, False, dict(p, uda_pw_scheme="f16"), weights=w)
    assert other.pw_scheme == "f16" and d.pw_scheme == "f16x2"
    other.set_dropout_seed(4)
    for _ in range(2):
        d.serve(imgs)
        other.serve(imgs)
det = d.serve(imgs)
cls, box = d.head_outputs(2)
d.close()
if sys.argv[2] == "beside_f16":
    other.close()
np.savez(sys.argv[1], *(list(det) + list(cls) + list(box)))
print("saved")
"""


def test_f16x2_handle_after_an_f16_handle_is_unchanged(tmp_path):
    """The scheme is per handle: an f16x2 handle created after an f16 one in the same process computes bit for bit what one
    in a fresh process computes - and so does one that lives beside an f16 handle, served alternately with it, in a process whose
    environment names a third scheme (the scheme travels in the model description, the environment gives the default only)."""
    outs = []
    for tag in ("fresh", "after_f16", "beside_f16"):
        out = str(tmp_path / (tag + ".npz"))
        e = dict(os.environ)
        e.pop("UDA_PW_SCHEME", None)
        e.pop("UDA_PW_TERMS", None)
        if tag == "beside_f16":
            e["UDA_PW_SCHEME"] = "bf16x3"
        r = subprocess.run([sys.executable, "-c", ORDER_WORKER % {"root": ROOT}, out, tag], cwd=ROOT, env=e,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "saved" in r.stdout, (tag, r.stdout[-1500:], r.stderr[-2500:])
        outs.append(np.load(out))
    assert len(outs[0].files) == len(outs[1].files) == len(outs[2].files) > 5
    for k in outs[0].files:
        np.testing.assert_array_equal(outs[0][k], outs[1][k], err_msg=k)
        np.testing.assert_array_equal(outs[0][k], outs[2][k], err_msg="beside_f16 " + k)
