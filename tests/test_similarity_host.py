"""The host side of the set-similarity analysis (`set_similarity`, reference active_learning_eval.py:458-583, 946-1029) without a
GPU: the package's formulas fed by the numpy mirror of the neighbour search (tests/knn_ref.py, through the `nn_dist2=` hook)
against the reference's own values (tests/golden/similarity_golden.npz, maker beside it).  The goldens hold every case twice:
`exact`, the reference with its KD-trees queried at eps=0 - what this project computes, bit for bit - and `eps`, the reference as
shipped (eps=0.01), which may lie up to D * ln 1.01 away: each of the two distances of a log-ratio term is within a factor 1.01
of the nearest, the terms are averaged and multiplied by D.  That bound is on the reference's approximation; nothing here has a
tolerance."""
import os

import numpy as np
import pytest

import knn_ref as R
from uda_amd import capi
from uda_amd import set_similarity as S

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "similarity_golden.npz"))
KL_CASES = [str(c) for c in GOLD["kl_cases"]]
JSD_CASES = [str(c) for c in GOLD["jsd_cases"]]
LN101 = float(np.log(1.01))


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def sim_inputs():
    classes, methods = [str(c) for c in GOLD["sim_classes"]], [str(m) for m in GOLD["sim_methods"]]
    sets = [{cl: [list(row) for row in GOLD["sim_in_%d_%s" % (s, cl)]] for cl in classes} for s in range(len(methods) + 1)]
    return classes, methods, sets


@pytest.mark.parametrize("c", KL_CASES)
def test_kl_equals_the_exact_reference_bit_for_bit(c):
    p, q = GOLD["kl_%s_p" % c], GOLD["kl_%s_q" % c]
    got = S.emp_kl_divergence(p, q, nn_dist2=R.nn_dist2)
    print(c, got, GOLD["kl_%s_exact" % c][0])
    assert same_bits([got], GOLD["kl_%s_exact" % c])
    assert same_bits([R.emp_kl(p, q)], GOLD["kl_%s_exact" % c])


def test_kl_of_many_pairs_is_the_single_pairs_and_covers_inf_and_nan():
    pairs = [(GOLD["kl_%s_p" % c], GOLD["kl_%s_q" % c]) for c in KL_CASES if "d3" in c]
    got = S.emp_kl_divergences(pairs, nn_dist2=R.nn_dist2)
    assert same_bits(got, [GOLD["kl_%s_exact" % c][0] for c in KL_CASES if "d3" in c])
    assert GOLD["kl_d3_dup_exact"][0] == np.inf and GOLD["kl_d3_common_exact"][0] == -np.inf and np.isnan(GOLD["kl_d3_both_exact"][0])


@pytest.mark.parametrize("c", JSD_CASES)
def test_jsd_from_the_stored_resampled_sets_equals_the_exact_reference(c):
    g = lambda k: GOLD["jsd_%s_%s" % (c, k)]  # noqa: E731
    (jsd, kl_pm, kl_qm), = S.jensen_shannon_from_samples([(g("sp"), g("sq"), g("sm"))], nn_dist2=R.nn_dist2)
    print(c, jsd, kl_pm, kl_qm)
    assert same_bits([kl_pm, kl_qm], g("kl_exact")) and same_bits([jsd], g("jsd_exact"))


def test_shipped_values_lie_within_d_ln_101_of_the_exact_ones():
    """The derived bound on the reference's eps=0.01, per KL: D * ln 1.01; a JSD is the mean of two KLs, a per-class metric a JSD
    plus an exact offset."""
    for c in KL_CASES:
        eps, exact, d = GOLD["kl_%s_eps" % c][0], GOLD["kl_%s_exact" % c][0], GOLD["kl_%s_p" % c].shape[1]
        if np.isfinite(exact):
            print(c, eps - exact)
            assert abs(eps - exact) <= d * LN101
        else:
            assert same_bits([eps], [exact])
    for c in JSD_CASES:
        assert (np.abs(GOLD["jsd_%s_kl_eps" % c] - GOLD["jsd_%s_kl_exact" % c]) <= 3 * LN101).all()
        assert abs(GOLD["jsd_%s_jsd_eps" % c][0] - GOLD["jsd_%s_jsd_exact" % c][0]) <= 3 * LN101
    a, b = GOLD["sim_perclass_eps"], GOLD["sim_perclass_exact"]
    assert np.array_equal(np.isnan(a), np.isnan(b)) and (np.abs(a - b)[~np.isnan(b)] <= 3 * LN101).all()


def test_similarity_table_equals_the_exact_reference():
    """Same order, same floats, same flag; the cell of the method without boxes of a class is nan.  The table's resampled sets
    are too large to store, so this test resamples, which needs scipy."""
    pytest.importorskip("scipy.stats", reason="scipy is not installed: gaussian_kde resampling cannot run")
    classes, methods, sets = sim_inputs()
    pairs, flag, perclass = S.calculate_set_similarity(sets, classes, methods, return_perclass=True, nn_dist2=R.nn_dist2,
                                                       num_samples=int(GOLD["sim_samples"][0]))
    print(pairs, flag)
    assert [k for k, _ in pairs] == [str(k) for k in GOLD["sim_names_exact"]]
    assert same_bits([v for _, v in pairs], GOLD["sim_values_exact"])
    assert bool(flag) == bool(GOLD["sim_flag_exact"][0])
    assert same_bits(np.asarray(perclass), GOLD["sim_perclass_exact"]) and np.isnan(perclass[2][1])
    assert S.calculate_set_similarity(sets, classes, methods, nn_dist2=R.nn_dist2, num_samples=int(GOLD["sim_samples"][0]))[2] is None


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_kd_tree_at_eps_0_equals_the_mirror(d):
    spatial = pytest.importorskip("scipy.spatial", reason="scipy is not installed: no KD-tree to compare the mirror with")
    rng = np.random.default_rng([7, d])
    p, q = np.exp(rng.normal(0, 0.7, (700, d))), np.exp(rng.normal(0.2, 0.7, (600, d)))
    p[5] = p[300]
    own = spatial.cKDTree(p).query(p, k=2, eps=0, p=2)[0][:, 1]
    cross = spatial.cKDTree(q).query(p, k=1, eps=0, p=2)[0]
    assert same_bits(own, np.sqrt(R.dist2(p, p, self=True))) and own[5] == 0 and own[300] == 0
    assert same_bits(cross, np.sqrt(R.dist2(p, q)))
    one = spatial.cKDTree(p[:1]).query(p[:1], k=2, eps=0, p=2)[0][:, 1]
    assert same_bits(one, R.dist2(p[:1], p[:1], self=True)) and one[0] == np.inf


@pytest.mark.parametrize("c", JSD_CASES)
def test_resampled_sets_equal_the_stored_ones(c):
    pytest.importorskip("scipy.stats", reason="scipy is not installed: gaussian_kde resampling cannot run")
    g = lambda k: GOLD["jsd_%s_%s" % (c, k)]  # noqa: E731
    sp, sq, sm = S.resample_sets(g("P"), g("Q"), int(g("n")[0]))
    assert same_bits(sp, g("sp")) and same_bits(sq, g("sq")) and same_bits(sm, g("sm"))
    assert sp.shape == (int(g("n")[0]), 3) and sp.flags.c_contiguous
    got = S.empirical_jensen_shannon_divergence(g("P"), g("Q"), int(g("n")[0]), nn_dist2=R.nn_dist2)
    assert same_bits([got], g("jsd_exact"))


def test_mirror_blocks_do_not_change_the_result():
    rng = np.random.default_rng(3)
    p = rng.normal(size=(1100, 3))
    assert same_bits(R.dist2(p, p, self=True), R.dist2(p, p, self=True, block=97))
    assert same_bits(R.dist2(p[:40], p), R.dist2(p[:40], p, block=7))
    full = ((p[:, None, :] - p[None, :, :]) ** 2)
    d = (full[..., 0] + full[..., 1]) + full[..., 2]
    np.fill_diagonal(d, np.inf)
    assert same_bits(R.dist2(p, p, self=True), d.min(axis=1))


def test_dimension_mismatch_and_empty_after_filter_raise():
    rng = np.random.default_rng(0)
    with pytest.raises(ValueError, match="same number of dimensions"):
        S.emp_kl_divergence(rng.random((10, 3)), rng.random((10, 2)), nn_dist2=R.nn_dist2)
    with pytest.raises(ValueError, match="Filtered data is empty"):
        S.resample_sets(np.zeros((5, 3)), rng.random((10, 3)) + 0.1, 10)
    with pytest.raises(ValueError, match="Filtered data is empty"):
        S.empirical_jensen_shannon_divergence(rng.random((10, 3)) + 0.1, -np.ones((4, 3)), 10, nn_dist2=R.nn_dist2)


def test_bad_points_are_refused_before_the_device_is_touched():
    ok = np.random.default_rng(0).random((10, 3))
    for bad in (np.nan, np.inf, -np.inf):
        p = ok.copy()
        p[3, 1] = bad
        with pytest.raises(ValueError, match="not finite"):
            S.nn_dist2([(p, None)])
        with pytest.raises(ValueError, match="not finite"):
            S.nn_dist2([(ok, p)])
        with pytest.raises(ValueError, match="not finite"):
            S.emp_kl_divergence(ok, p)
    with pytest.raises(ValueError, match="1..4"):
        S.nn_dist2([(np.ones((3, 5)), None)])
    with pytest.raises(ValueError, match="share one dimension"):
        S.nn_dist2([(np.ones((3, 2)), None), (np.ones((3, 3)), None)])
    with pytest.raises(ValueError, match=r"points \[n, D\]"):
        S.nn_dist2([(np.ones(3), None)])
    with pytest.raises(ValueError, match="empty set"):
        S.nn_dist2([(np.ones((3, 2)), np.ones((0, 2)))])
    assert S.nn_dist2([]) == []


def test_binding_lists_the_entry_point_and_the_header_limits():
    assert "uda_nn_dist2_np" in capi.EXPORTS
    import re
    defs = dict(re.findall(r"#define (UDA_KNN_[A-Z_]+) +\(?([0-9l<> ]+)\)?", open(capi.HEADER).read()))
    assert (int(defs["UDA_KNN_ROWS"]), int(defs["UDA_KNN_COLS"]), int(defs["UDA_KNN_MAX_D"]), int(defs["UDA_KNN_MAX_N"]),
            int(defs["UDA_KNN_MAX_B"])) == (capi.KNN_ROWS, capi.KNN_COLS, capi.KNN_MAX_D, capi.KNN_MAX_N, capi.KNN_MAX_B)
    assert defs["UDA_KNN_MAX_PAIRS"].replace(" ", "") == "1ll<<38" and capi.KNN_MAX_PAIRS == 1 << 38


def test_entry_point_fails_loudly_without_a_device():
    """No CPU fallback: without a HIP device the call returns 1 and the message names the entry point; bad arguments are
    refused before a device is looked for."""
    import subprocess
    import sys
    from common import ROOT
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import numpy as np\n"
            "from uda_amd import capi\n"
            "lib = capi.load()\n"
            "p, off, out = np.ones((4, 3)), np.array([0, 4], np.int64), np.full(4, -7.0)\n"
            "for D in (3, 5):\n"
            "    rc = lib.uda_nn_dist2_np(0, D, 1, p.ctypes.data, off.ctypes.data, p.ctypes.data, off.ctypes.data, None, out.ctypes.data)\n"
            "    print('%%d|%%d|%%s|%%s' %% (D, rc, lib.uda_last_error(None).decode(), out.tolist()))\n" % ROOT)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0, res.stderr
    rows = [line.split("|") for line in res.stdout.splitlines() if line.count("|") == 3]
    assert [r[:2] for r in rows] == [["3", "1"], ["5", "1"]], res.stdout
    assert rows[0][2].startswith("uda_nn_dist2_np:") and "no ROCm-capable device is detected" in rows[0][2]
    assert rows[1][2].startswith("uda_nn_dist2_np: 5 coordinates")
    assert all(r[3] == "[-7.0, -7.0, -7.0, -7.0]" for r in rows)
