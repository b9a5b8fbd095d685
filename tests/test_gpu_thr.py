"""The thresholding objective on the device (`thresholding.roc_objective` -> `uda_thr_objective_np`; reference
uncertainty_analysis.py:44-152): every case of tests/golden/thr_golden.npz (what the reference's own `roc_metrics` returned), the
large-N path and the upper limit against the numpy mirror (tests/thr_ref.py), candidate chunking, the library's refusals, and the
search on the device against the search on the mirror."""
import ctypes as C
import os

import numpy as np
import pytest

import thr_ref as R
from uda_amd import capi
from uda_amd import thresholding as TH

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "thr_golden.npz"))
CASES = [str(c) for c in GOLD["cases"]]
DEFAULT6 = [0.5, 0.55, 0.6, 0.65, 0.7, 0.75]


def gold_case(c):
    g = {k: GOLD["%s_%s" % (c, k)] for k in ("uncerts", "ious", "tp_class", "iou_thrs", "params", "thr", "rate", "auc")}
    g["fix_cd"], g["budget"] = int(GOLD[c + "_fix_cd"]), float(GOLD[c + "_budget"])
    g["group"] = GOLD[c + "_group"] if c + "_group" in GOLD.files else None
    return g


def assert_matches(got, want, N):
    """thr and rate identical (NaN = NaN, +inf = +inf; -0.0 is 0.0), auc within N * 2^-52: the worst case of summing N terms that
    add up to at most 1 in another order."""
    for a, b, name in zip(got[:2], want[:2], ("thr", "rate")):
        print(name, "differing entries:", int(np.sum(~((a == b) | (np.isnan(a) & np.isnan(b))))))
        assert np.array_equal(a, b, equal_nan=True), name
    auc, ref = got[2], want[2]
    assert np.array_equal(np.isnan(auc), np.isnan(ref))
    ok = ~np.isnan(ref)
    err = np.abs(auc[ok] - ref[ok]).max() if ok.any() else 0.0
    print("auc error %.3g of the bound %.3g" % (err, N * 2.0 ** -52))
    assert err <= N * 2.0 ** -52


def seeded(N, P, U=2, seed=0, decimals=3):
    rng = np.random.default_rng(seed)
    tp = rng.random(N) < 0.85
    ious = np.round(rng.uniform(0.05, 0.999, N), 3)
    wrong = ~(tp & (ious >= 0.5))
    unc = np.stack([np.round(rng.uniform(0, 1.2, N) * np.where(wrong, 1.0, 0.6), decimals)] +
                   [np.round(rng.gamma(2.0, 0.05, N), decimals) for _ in range(U - 1)])
    params = rng.uniform(0, 1, (P, U))
    params[0] = np.round(params[0], 1)
    return unc, ious, tp, params


@pytest.mark.parametrize("c", CASES)
def test_device_reproduces_the_reference(c):
    g = gold_case(c)
    got = TH.roc_objective(g["uncerts"], g["ious"], g["tp_class"], g["iou_thrs"], g["params"], g["fix_cd"], g["budget"], g["group"])
    assert_matches(got, (g["thr"], g["rate"], g["auc"]), g["uncerts"].shape[1])


@pytest.mark.parametrize("N,P,K", [(70001, 5, 6), (262144, 2, 6)])
def test_large_n_against_the_mirror(N, P, K):
    """N above one tile of the sort (the global merge steps) and at the limit; scores on a 3-decimal grid tie by the thousand."""
    unc, ious, tp, params = seeded(N, P, seed=N)
    for fix_cd in ((1, 0) if N < 100000 else (1,)):
        got = TH.roc_objective(unc, ious, tp, DEFAULT6[:K], params, fix_cd, 0.95)
        assert_matches(got, R.roc_objective(unc, ious, tp, DEFAULT6[:K], params, fix_cd, 0.95), N)


def test_chunked_candidates_equal_one_at_a_time():
    """P = 1000 at N = 257 through the library's chunk loop: at K = 32 a candidate takes 12 * 2048 + 8 * 257 * 32 + 24 * 32 + 16 =
    91152 bytes of scratch, so 64 MiB hold 736 and the call runs two chunks.  Bit for bit what the same candidates give alone
    (on both sides of the chunk boundary), and what the mirror gives."""
    N, P = 257, 1000
    unc, ious, tp, params = seeded(N, P, seed=5, decimals=2)
    thrs = np.linspace(0.05, 0.95, 32)
    got = TH.roc_objective(unc, ious, tp, thrs, params, 1, 0.95)
    for p in (0, 1, 735, 736, 737, 999):
        one = TH.roc_objective(unc, ious, tp, thrs, params[p], 1, 0.95)
        for a, b in zip(got, one):
            assert np.array_equal(a[p], b[0], equal_nan=True)
    sel = np.r_[0:8, 732:740, 992:1000]
    want = R.roc_objective(unc, ious, tp, thrs, params[sel], 1, 0.95)
    assert_matches(tuple(a[sel] for a in got), want, N)


def _raw(N=8, U=1, G=0, K=1, P=1, group=None, budget=0.95):
    lib = capi.load()
    n = max(N, 1)
    unc, iou, tp = np.zeros((max(U, 1), n)), np.ones(n), np.ones(n, np.uint8)
    unc[0, : n // 2] = 1.0
    tp[::2] = 0
    thrs, par = np.full(max(K, 1), 0.5), np.ones((max(P, 1), max(U, 1) * max(G, 1)))
    out = [np.zeros((max(P, 1), max(K, 1))) for _ in range(3)]
    p = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731
    grp = None if group is None else np.ascontiguousarray(group, np.int32)
    rc = lib.uda_thr_objective_np(0, p(unc), p(iou), p(tp), None if grp is None else p(grp), N, U, G, p(thrs), K, p(par), P, 1,
                                  budget, p(out[0]), p(out[1]), p(out[2]))
    return rc, (lib.uda_last_error(None) or b"").decode(), out


def test_library_refuses_what_is_outside_its_limits():
    rc, msg, out = _raw()
    assert rc == 0 and np.isfinite(out[1]).all()
    for kw, word in ((dict(N=1), "rows"), (dict(N=TH.MAX_N + 1), "rows"), (dict(K=33), "IoU thresholds"), (dict(K=0), "IoU thresholds"),
                     (dict(U=5), "uncertainties"), (dict(P=0), "candidates"), (dict(G=TH.MAX_G + 1, group=np.zeros(8)), "groups"),
                     (dict(G=2, group=np.r_[np.zeros(7), 2]), "group id 2"), (dict(G=2, group=np.r_[np.zeros(7), -1]), "group id -1"),
                     (dict(G=2), "go together"), (dict(budget=1.0), "budget"), (dict(budget=0.0), "budget")):
        rc, msg, _ = _raw(**kw)
        assert rc != 0 and word in msg, (kw, msg)


def test_search_on_the_device_equals_the_search_on_the_mirror(tmp_path):
    g = gold_case("n257p64")
    found = []
    for name, objective in (("device", None), ("mirror", R.roc_objective)):
        os.makedirs(str(tmp_path / name))
        o = TH.UncertOptimal(None, g["tp_class"], g["ious"], list(g["uncerts"]), source_path=str(tmp_path / name),
                             objective=objective, population=48, rounds=3)
        found.append((o.get_optimal_uncertainty(), o.opt_thrs, o.loss, o.evaluated[1]))
    assert found[0][0] == found[1][0] and found[0][1] == found[1][1] and found[0][2] == found[1][2]
    assert np.array_equal(found[0][3], found[1][3])


def test_roc_metrics_is_the_batched_row():
    g = gold_case("n1025")
    u = R.combined(g["uncerts"], g["params"][1])
    for fix_cd, budget in ((1, 0.95), (0, 0.8)):
        for t in (0.5, 0.75):
            y = (g["ious"] >= t) & (g["tp_class"] != 0)
            one = TH.roc_metrics(u, y.astype(int), fix_cd=fix_cd, budget=budget)
            row = TH.roc_objective(g["uncerts"], g["ious"], g["tp_class"], [t], g["params"][1], fix_cd, budget)
            assert one == (row[0][0, 0], row[1][0, 0], row[2][0, 0])
            assert one[:2] == R.roc_metrics(u, y, fix_cd, budget)[:2]
    assert TH.roc_metrics(u, y.astype(int))[:2] == R.roc_metrics(u, y, True, 0.95)[:2]      # the hyper-parameters' defaults
