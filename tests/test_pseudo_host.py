"""Pseudo-labelling, host side (`uda_amd.pseudo_labels`; reference SSL_stac.py:202-642): the numpy restatement
(tests/pseudo_ref.py) against what the reference's own `STAC.score_image` returned (tests/golden/pseudo_golden.npz), the
selection grammar and where it differs from the active-learning one, `PseudoLabelSet` (finalize, merge, pickling) against the
fixture through the restatement's rows as a stand-in for the device, the writers' bytes against the reference's files, and the
refusals."""
import os
import pickle

import numpy as np
import pytest

import pseudo_ref as R
from common import FULL_MC, HEAD_MC, LOSS_ATT, PLAIN, make_params
from uda_amd import active_learning as AL
from uda_amd import pseudo_labels as PL

G = R.Golden()
ALL_SOURCES = dict.fromkeys(AL.SOURCES)


def stand_in_rows(cols, sel, tau):
    """(records, minmax, kept, cand) as the device returns them, from the restatement."""
    res, minmax, kept, cand, _ = R.rows(cols, sel.components, sel.invert, sel.gate, G.min_score, tau, G.max_rows)
    return R.as_records(res, cols, PL.RECORD_DTYPE), minmax, kept, cand


# ------------------------------------------------------------------ the restatement against the reference's own results
@pytest.mark.parametrize("ci", range(len(G.cases)), ids=G.ids)
def test_restatement_equals_the_reference(ci):
    ds, strategy, tau = G.cases[ci]
    cols, C, names, g = G.case(ci)
    comps, invert, gate, rule = R.components_of(strategy, G.opt)
    res, minmax, kept, cand, _ = R.rows(cols, comps, invert, gate, G.min_score, tau, G.max_rows)
    np.testing.assert_array_equal(kept, G.z["%s_kept" % ds][:len(kept)])
    np.testing.assert_array_equal(res["image"], g["cand_image"])
    np.testing.assert_array_equal(res["row"], g["cand_row"])
    np.testing.assert_array_equal(res["cls"], g["cand_classes"])
    np.testing.assert_array_equal(cand, g["cand"])
    # a value is at most ~20 float64 operations on non-negative terms; the restatement makes the reference's own numpy calls
    np.testing.assert_allclose(res["v"], g["cand_v"], rtol=1e-12, atol=0)
    if "minmax" in g:
        np.testing.assert_allclose(minmax, g["minmax"], rtol=1e-12, atol=0)
    R.same_selection(R.select(cols, names, strategy, tau, G.min_score, G.opt, G.opt_thrs, G.max_rows), G.returned(ci))


def test_fixture_covers_what_it_should():
    strategies = {c[1] for c in G.cases}
    assert {"score", "pseudoscore_score", "combo", "pseudoscore_combo", "alluncert", "pseudoscore_epuncert", "ental", "entropy",
            "box_norm_albox", "box_albox", "class_mcclass", "sota"} <= strategies
    assert {c[2] for c in G.cases} == {0.4, 0.9}
    assert {0, 1, 2, 63, 64, 65, 98, 99, 100} <= set(G.z["kept"].tolist())
    assert {int(G.z["%s_num_classes" % d][0]) for d in G.z["datasets"]} == {3, 10}
    for ci, (ds, strategy, tau) in enumerate(G.cases):
        n = int(G.z["k%d_n" % ci][0])
        multi = any(w in strategy for w in ("combo", "alluncert", "epuncert", "ental"))
        assert (100 in G.z["%s_kept" % ds][:n].tolist()) == (not multi and ds != "z")
    # the non-finite dataset: an inf survives the single-column rule; under combo the maximum inf leaves nothing
    z = {s: ci for ci, (ds, s, _) in enumerate(G.cases) if ds == "z"}
    assert np.isinf(G.z["k%d_pseudo" % z["pseudoscore_box_norm_albox"]]).sum() == 1
    assert len(G.z["k%d_names" % z["pseudoscore_combo"]]) == 0 and len(G.z["k%d_cand_v" % z["pseudoscore_combo"]]) > 0
    assert np.isnan(G.z["k%d_cand_v" % z["pseudoscore_ental"]]).sum() == 1 and (G.z["k%d_cand_v" % z["pseudoscore_ental"]] == 0).sum() == 1
    assert os.path.getsize(G.path) < 1 << 20


# ------------------------------------------------------------------ the selection grammar
PARAMS = {"full_mc": FULL_MC, "head_mc": HEAD_MC, "loss_att": LOSS_ATT, "plain": PLAIN}


@pytest.mark.parametrize("strategy", sorted({c[1] for c in G.cases}) + ["box_norm_mcbox", "selftrain_pseudoscore_ental", "curr_alluncert"])
def test_grammar_agrees_with_the_restatement(strategy):
    sel = PL.resolve_selection(strategy, ALL_SOURCES, G.opt)
    comps, invert, gate, rule = R.components_of(strategy, G.opt)
    assert sel.components == [[(s, t, float(w)) for s, t, w in comp] for comp in comps]
    assert (sel.invert, sel.gate, sel.rule) == (invert, gate, rule)
    assert sel.activate_pseudoscore == ("pseudoscore" in strategy)
    assert not sel.calibrated and sel.desc().n_comp == len(comps)


def test_grammar_follows_stac_not_the_active_learning_loop():
    # STAC has no `sota` branch: the word falls through to det_score; the active-learning loop reads three columns
    sota = PL.resolve_selection("sota", ALL_SOURCES)
    assert sota.components == [[("det_score", "scalar", 1.0)]] and sota.rule == "tau" and sota.gate == 1
    assert AL.resolve_strategy("sota", ALL_SOURCES).n_comp == 3
    # `combo` beside another branch word is `combo` in STAC and refused by the active-learning grammar
    both = PL.resolve_selection("combo_alluncert", ALL_SOURCES, G.opt)
    assert both.rule == "combo" and both.n_comp == 1
    with pytest.raises(ValueError, match="combo"):
        AL.resolve_strategy("combo_alluncert", ALL_SOURCES, G.opt)
    # epuncert is tested before ental
    assert PL.resolve_selection("epuncert_ental", ALL_SOURCES).components[1] == [("mcclass", "mean", 1.0)]
    # there is no mean / max over the image, and the refactored active-learning grammar is what it was
    assert PL.resolve_selection("mean_entropy", ALL_SOURCES).reduce_mean is False
    st = AL.resolve_strategy("mean_alluncert_highep_lowal", ALL_SOURCES)
    assert st.reduce_mean and st.combine == "highep_lowal" and st.n_comp == 3


@pytest.mark.parametrize("cfg", sorted(PARAMS))
def test_grammar_reads_what_the_model_emits(cfg):
    p = make_params(**dict(PARAMS[cfg], enable_softmax=True))
    has = AL.emitted_sources(p)
    for strategy, needs in (("combo", {"entropy", "albox"}), ("alluncert", {"mcbox", "albox", "mcclass"}), ("epuncert", {"mcbox", "mcclass"}),
                            ("ental", {"albox", "entropy"})):
        if needs <= has:
            assert set(PL.resolve_selection(strategy, p, G.opt).sources()) == needs
        else:
            with pytest.raises(ValueError, match="does not emit"):
                PL.resolve_selection(strategy, p, G.opt)
    # the last branch falls back to det_score when a line would not hold the key
    sel = PL.resolve_selection("box_albox", p)
    assert sel.sources() == (["albox"] if "albox" in has else ["det_score"])
    calib = PL.resolve_selection("calib_entropy", p)
    assert calib.calibrated and calib.columns == {"entropy": "iso_percls_entropy"}
    with pytest.raises(ValueError, match="opt_params"):
        PL.resolve_selection("combo", ALL_SOURCES)
    with pytest.raises(ValueError, match="no box shape"):
        PL.resolve_selection("class_box_norm_mcclass", ALL_SOURCES)


# ------------------------------------------------------------------ PseudoLabelSet
@pytest.mark.parametrize("ci", range(len(G.cases)), ids=G.ids)
def test_finalize_split_and_merge(ci):
    ds, strategy, tau = G.cases[ci]
    cols, C, names, g = G.case(ci)
    sel = PL.resolve_selection(strategy, ALL_SOURCES, G.opt)
    want = G.returned(ci)

    def part(lo, hi, acc):
        sub = {k: v[lo:hi] for k, v in cols.items()}
        acc.add(names[lo:hi], stand_in_rows(sub, sel, tau), boxes=sub["boxes"])
        return acc

    new = lambda: PL.PseudoLabelSet(sel, tau, G.opt_thrs)      # noqa: E731
    n = len(names)
    one = part(0, n, new())
    got = one.finalize()
    assert len(got) == (4 if sel.activate_pseudoscore else 3)
    forced = PL.PseudoLabelSet(PL.resolve_selection("pseudoscore_" + strategy, ALL_SOURCES, G.opt), tau, G.opt_thrs)
    R.same_selection(part(0, n, forced).finalize(), want)
    R.same_selection(got + (() if len(got) == 4 else (want[3],)), want)
    if "minmax" in g and len(g["cand_v"]):
        lo, hi = min(g["minmax"][:, 0]), max(g["minmax"][:, 1])
        assert (one.min, one.max) == pytest.approx((lo, hi), rel=1e-12)
    # batches, then shards merged in order: the same result as one pass
    two = part(n // 2, n, part(0, n // 2, forced.__class__(forced.selection, tau, G.opt_thrs)))
    merged = part(0, 3, forced.__class__(forced.selection, tau, G.opt_thrs)).merge(pickle.loads(pickle.dumps(part(3, n, forced.__class__(forced.selection, tau, G.opt_thrs)))))
    for other in (two, merged):
        a, b = other.finalize(), part(0, n, forced.__class__(forced.selection, tau, G.opt_thrs)).finalize()
        R.same_selection(a, b, pseudo_rtol=0)
        assert other.n_images == n and (other.min, other.max) == (one.min, one.max)


def test_record_boxes_are_used_when_no_columns_are_given():
    ci = G.cases.index(("a", "entropy", 0.9))
    cols, C, names, g = G.case(ci)
    sel = PL.resolve_selection("entropy", ALL_SOURCES)
    acc = PL.PseudoLabelSet(sel, 0.9)
    assert acc.add(names, stand_in_rows(cols, sel, 0.9)) == len(g["names"])
    got, want = acc.finalize(), G.returned(ci)
    assert [str(v) for v in got[0]] == [str(v) for v in want[0]]
    for a, b in zip(got[2], want[2]):
        assert a.dtype == np.float64
        np.testing.assert_array_equal(a, np.asarray(b, np.float32).astype(np.float64))          # float32, as the device stores them


# ------------------------------------------------------------------ the writers
@pytest.mark.parametrize("ci", [ci for ci in range(len(G.cases)) if "k%d_bdd" % ci in G.z.files], ids=lambda ci: G.ids[ci])
def test_writers_write_the_reference_files(ci, tmp_path):
    ds, strategy, tau = G.cases[ci]
    g = G.case(ci)[3]
    want = G.returned(ci)
    selected = want if "pseudoscore" in strategy else want[:3]
    label_map = dict(enumerate([str(v) for v in G.z["%s_class_names" % ds]], start=1))
    assert PL.write_kitti_pseudo_gt(str(tmp_path / "k"), selected, label_map) == int(g["n_dets"][0])
    files = sorted(os.listdir(tmp_path / "k"))
    assert files == [str(v) for v in g["kitti_files"]]
    for f, text in zip(files, g["kitti_texts"]):
        assert open(tmp_path / "k" / f, "rb").read() == str(text).encode()
    assert PL.write_bdd_pseudo_gt(str(tmp_path / "b"), selected, label_map) == int(g["n_dets"][0])
    assert open(tmp_path / "b" / "pseudo_labels.json", "rb").read() == str(g["bdd"][0]).encode()


def test_writers_take_the_dataset_label_maps(tmp_path):
    sel = (np.asarray(["000003.png"]), [np.asarray([1.0, 6.0])], [np.asarray([[1.5, 2.0, 30.25, 40.0], [5.0, 6.0, 7.0, 8.5]])], [np.asarray([0.123, 0.987])])
    assert PL.write_kitti_pseudo_gt(str(tmp_path), sel) == 2
    assert open(tmp_path / "000003.txt").read() == ("Car 0.0 0 -10 2.0 1.5 40.0 30.25 0.0 0.0 0.0 0.0 0.0 0.0 0.12\n"
                                                    "Cyclist 0.0 0 -10 6.0 5.0 8.5 7.0 0.0 0.0 0.0 0.0 0.0 0.0 0.99\n")
    assert PL.write_kitti_pseudo_gt(str(tmp_path), sel[:3], "datasets/KITTI/pseudo") == 2
    assert open(tmp_path / "000003.txt").read().splitlines()[0].endswith(" -10")
    assert PL.write_bdd_pseudo_gt(str(tmp_path), sel) == 2
    import json
    labels = json.load(open(tmp_path / "pseudo_labels.json"))[0]["labels"]
    assert [lb["category"] for lb in labels] == ["pedestrian", "train"] and labels[1]["pseudo_score"] == 0.99


# ------------------------------------------------------------------ refusals
def test_refusals():
    cols, C = G.columns("a")
    sel = PL.resolve_selection("combo", ALL_SOURCES, G.opt)
    with pytest.raises(ValueError, match="opt_thrs"):
        PL.PseudoLabelSet(sel, 0.4)
    with pytest.raises(ValueError, match="tau"):
        PL.PseudoLabelSet(sel, -0.1, G.opt_thrs)
    with pytest.raises(ValueError, match="tau"):
        PL.PseudoLabelSet(sel, float("nan"), G.opt_thrs)
    with pytest.raises(TypeError):
        PL.PseudoLabelSet(AL.resolve_strategy("combo", ALL_SOURCES, G.opt), 0.4, G.opt_thrs)
    acc = PL.PseudoLabelSet(sel, 0.4, G.opt_thrs)
    rows = stand_in_rows({k: v[:3] for k, v in cols.items()}, sel, 0.4)
    with pytest.raises(ValueError, match="names"):
        acc.add(G.names[:2], rows)
    with pytest.raises(ValueError, match="RECORD_DTYPE"):
        acc.add(G.names[:3], (rows[0][:-1],) + rows[1:])
    with pytest.raises(ValueError, match="merge"):
        acc.merge(PL.PseudoLabelSet(sel, 0.9, G.opt_thrs))
    assert len(acc) == 0 and acc.finalize()[0].shape == (0,)
    # the host-array entry point refuses before it touches a device
    with pytest.raises(ValueError, match="tau"):
        PL.select_detections(cols, "entropy", -1.0)
    with pytest.raises(ValueError, match="max_rows"):
        PL.select_detections(cols, "entropy", 0.4, max_rows=0)
    with pytest.raises(ValueError, match="not given"):
        PL.select_detections({k: v for k, v in cols.items() if k != "albox"}, sel, 0.4)
    with pytest.raises(ValueError, match="finite"):
        PL.select_detections(dict(cols, entropy=np.where(cols["entropy"] > 1, np.nan, cols["entropy"])), "entropy", 0.4)
    assert AL.default_min_score({}, ssl=True) == G.min_score
    # a sample-sharded serve holds no whole batch: it points to the host-array entry point
    from uda_amd import dist
    sharded = dist.SampleShardedDriver.__new__(dist.SampleShardedDriver)
    for call in (lambda: sharded.pseudo_rows("entropy", 0.4), lambda: sharded.serve_pseudo_labels([], "entropy", 0.4)):
        with pytest.raises(ValueError, match="select_detections"):
            call()


def test_host_array_entry_points_fail_loudly_without_gpu():
    """No CPU fallback: without a HIP device both entry points return an error that names them and carries HIP's words."""
    import subprocess
    import sys
    from common import ROOT
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import pseudo_ref as R\n"
            "from uda_amd import capi, pseudo_labels as PL\n"
            "cols, C = R.Golden().columns('z')\n"
            "for f32 in (False, True):\n"
            "    try:\n"
            "        PL.select_detections(cols, 'entropy', 0.4, num_classes=C, as_float32=f32)\n"
            "        print('no error')\n"
            "    except capi.UdaError as e:\n"
            "        print('refused|%%s' %% e)\n" % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == 2 and all(ln.startswith("refused|") and "no ROCm-capable device is detected" in ln for ln in lines), out.stdout
    assert "uda_pseudo_rows_np:" in lines[0] and "uda_pseudo_rows_np_f32:" in lines[1]
