"""The epistemic-vs-aleatoric comparison on the host (`uda_amd.epal`, `writers.write_epal_highlow`; reference
src/uncertainty_ep_vs_al.py): the grid, the corners, the metric lists and the two text files against what the REAL reference
computed (tests/golden/epal_golden.npz, made by tests/golden/make_epal_golden.py) and against a scalar restatement of its loops;
the numpy mirror of the KDE entry point (tests/kde_ref.py) against the golden's scipy values and against live
scipy.stats.gaussian_kde; the entry point's refusals and its failure without a device.  No GPU is needed: wherever the package
would call the device, the mirror stands in through `engine=`.

KDE tolerance: all terms are non-negative, scipy sums the n of them sequentially and each exp is within an ulp, so a point's
relative error is at most (n + 16) * 2^-52, with 1e-300 * sum(w) absolute for points whose terms underflow."""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kde_ref as R
from common import ROOT
from uda_amd import capi, epal, writers

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "epal_golden.npz"))
CLASS_NAMES = [str(c) for c in GOLD["class_names"]]
RUNS = [(str(case), k) for case in GOLD["cases"] for k in range(len(GOLD["%s_runs" % case]))]
EPS = 2.0 ** -52
_RECORDS = {}


def records(case):
    if case not in _RECORDS:
        _RECORDS[case] = R.golden_case(GOLD, case)
    return _RECORDS[case]


def run_of(case, k):
    uncert, ent, numb = str(GOLD["%s_runs" % case][k]).split("|")
    return uncert, bool(int(ent)), int(numb), "%s_r%d_" % (case, k)


def close_to_scipy(got, want, n, sum_w=1.0):
    got, want = np.asarray(got), np.asarray(want)
    return np.all(np.abs(got - want) <= (n + 16) * EPS * np.abs(want) + 1e-300 * sum_w)


# ---- the reference's loops, restated scalar by scalar
def scalar_cell_indices(g, data):
    x_min, x_max = min(data[:, 0]), max(data[:, 0])
    y_min, y_max = min(data[:, 1]), max(data[:, 1])
    x_step = (x_max + (x_max - x_min) * 0.05 - x_min) / g
    y_step = (y_max + (y_max - y_min) * 0.05 - y_min) / g
    cells = []
    for i in range(len(data)):
        row = int(min((data[i, 1] - y_min) // y_step, g - 1))
        col = int(min((data[i, 0] - x_min) // x_step, g - 1))
        cells.append(row * g + col)
    return np.asarray(cells), x_min, x_step, y_min, y_step


def scalar_find_grid(al, mc, min_samples=3):
    data = np.stack([al, mc], axis=-1)

    def empty(g):
        cells = scalar_cell_indices(g, data)[0]
        return len(cells[cells == g ** 2 - g]) < min_samples, len(cells[cells == g - 1]) < min_samples

    g = 2
    tl, br = empty(g)
    if not tl or not br:
        while not tl or not br:
            g += 1
            tl, br = empty(g)
        g -= 1
    return g


def planes():
    rng = np.random.default_rng(5)
    lattice = rng.integers(0, 65, (500, 2)) / 64.0            # values exactly on cell edges of many grids
    lattice[0], lattice[1] = (0.0, 0.0), (1.0, 1.0)
    anti = np.stack([np.concatenate([rng.uniform(0.9, 1.0, 40), rng.uniform(0.0, 0.1, 40), rng.uniform(0, 1, 40)]),
                     np.concatenate([rng.uniform(0.0, 0.1, 40), rng.uniform(0.9, 1.0, 40), rng.uniform(0, 1, 40)])], 1)
    diag = np.stack([np.linspace(0, 1, 50), np.linspace(0, 3, 50)], 1)
    return {"random": rng.lognormal(-3, 0.7, (700, 2)), "lattice": lattice, "anti": anti, "diag": diag,
            "lattice_scaled": lattice * np.array([0.21, 21.0 / 64])}


@pytest.mark.parametrize("name", sorted(planes()))
def test_cell_indices_equal_the_scalar_loop(name):
    data = planes()[name]
    for g in list(range(1, 26)) + [64]:
        got, want = epal.cell_indices(g, data), scalar_cell_indices(g, data)
        assert got[0].dtype == np.int64 and np.array_equal(got[0], want[0]), (name, g)
        assert got[1:] == want[1:], (name, g)
        assert got[0].min() >= 0 and got[0].max() <= g * g - 1


@pytest.mark.parametrize("name", sorted(planes()))
def test_find_grid_equals_the_scalar_search(name):
    data = planes()[name]
    g, cells = epal.find_grid(data[:, 0], data[:, 1])
    assert g == scalar_find_grid(data[:, 0], data[:, 1])
    assert np.array_equal(cells[0], scalar_cell_indices(g, data)[0])
    if name == "anti":
        assert g > 4
    if name == "diag":
        assert g == 2                                         # a search that never grew does not step back


def test_grid_refusals():
    ok = np.random.default_rng(0).random((20, 2))
    for bad in (np.nan, np.inf):
        d = ok.copy()
        d[3, 1] = bad
        with pytest.raises(ValueError, match="not finite"):
            epal.cell_indices(3, d)
    flat = ok.copy()
    flat[:, 0] = 0.25
    with pytest.raises(ValueError, match="zero range"):
        epal.cell_indices(2, flat)
    with pytest.raises(ValueError, match=r"\[N, 2\]"):
        epal.cell_indices(2, np.ones((4, 3)))
    with pytest.raises(RuntimeError, match="64 x 64"):
        epal.find_grid(ok[:, 0], ok[:, 1], min_samples=0)     # no cell ever holds fewer than 0: the search cannot end


def test_golden_records_are_the_file_the_reference_read(tmp_path):
    for case in GOLD["cases"]:
        path = tmp_path / ("%s.txt" % case)
        writers.write_validate_results(str(path), records(str(case)))
        assert hashlib.sha256(path.read_bytes()).hexdigest() == str(GOLD["%s_text_sha" % case][0])
        assert epal.read_records(str(path)) == records(str(case))


@pytest.mark.parametrize("case,k", RUNS)
def test_comparison_equals_the_reference(case, k, tmp_path):
    uncert, ent, numb, pre = run_of(case, k)
    c = epal.compare_epal(records(case), CLASS_NAMES, im_numbs=numb, iou_thr=0.1, uncert=uncert, ent=ent, engine=R.kde_eval_np)
    assert c.grid_size == int(GOLD[pre + "grid_size"])
    assert np.array_equal(c.cell_indices, GOLD[pre + "cell_indices"])
    assert (c.x_min, c.x_step, c.y_min, c.y_step) == tuple(GOLD[pre + "cell_steps"])
    assert np.array_equal(c.hal_lep_ind, GOLD[pre + "hal_lep_ind"]) and np.array_equal(c.lal_hep_ind, GOLD[pre + "lal_hep_ind"])
    assert len(c.grid_x) == c.grid_size - 1 and c.grid_x[0] == c.x_min + c.x_step
    # the lists handed to plot_unc_metrics, in the reference's order
    n_metrics = int(GOLD[pre + "n_metrics"])
    assert len(c.metrics) == n_metrics == len(c.labels) == len(c.colors) == len(c.trends)
    assert c.labels == [str(v) for v in GOLD[pre + "labels"]][:n_metrics]
    for j, data in enumerate(c.metrics):
        assert len(data) == 9 and data[6] is None
        for col in (0, 3, 4, 5, 7, 8):
            assert np.array_equal(np.asarray(data[col], np.float64), GOLD["%sm%d_%d" % (pre, j, col)]), (j, col)
        for col in (1, 2):
            assert list(data[col]) == [str(v) for v in GOLD["%sm%d_%d" % (pre, j, col)]]
        x = np.arange(len(data[0]))
        if len(x) > 1:
            assert sorted(c.trends[j]) == list(epal.TREND_COLUMNS)
            for col in epal.TREND_COLUMNS:
                with np.testing.suppress_warnings() as sup:
                    sup.filter(np.exceptions.RankWarning)
                    assert np.array_equal(c.trends[j][col], np.poly1d(np.polyfit(x, data[col], 3))(x))
        else:
            assert c.trends[j] == {}
    # the two files, byte for byte, where the reference puts them
    assert c.subdir == str(GOLD[pre + "subdir"][0])
    paths = writers.write_epal_highlow(str(tmp_path), c)
    for path, stem in zip(paths, ("hal_lep", "lal_hep")):
        assert os.path.relpath(path, str(tmp_path)) == os.path.join(c.subdir, "%s_%s_iou_0.1.txt" % (stem, uncert))
        assert open(path).read() == str(GOLD[pre + stem + "_txt"][0])
    # the KDE on the mirror against the values scipy gave the reference
    n = int(c.keep.sum())
    assert c.pdf.shape == c.pdf_x.shape == c.pdf_y.shape == (100, 100)
    assert c.pdf_x[0, 0] == c.raw_al.min() and c.pdf_x[0, -1] == c.raw_al.max() and c.pdf_y[-1, 0] == c.raw_mc.max()
    want = GOLD[pre + "kde"]
    assert close_to_scipy(c.pdf.ravel()[::int(GOLD["kde_stride"])], want, n) and (want > 0).any()


def test_a_path_and_many_configurations_give_the_same(tmp_path):
    path = tmp_path / "validate_results.txt"
    writers.write_validate_results(str(path), records("main"))
    calls = []

    def engine(*a, **kw):
        calls.append(len(a[2]) - 1)
        return R.kde_eval_np(*a, **kw)

    configs = [run_of("main", k)[:2] for k in range(3)]
    many = epal.compare_many(str(path), CLASS_NAMES, configs, im_numbs=4, engine=engine)
    assert calls == [3]                                       # all KDEs in one call
    for (uncert, ent), c in zip(configs, many):
        one = epal.compare_epal(records("main"), CLASS_NAMES, im_numbs=4, uncert=uncert, ent=ent, engine=R.kde_eval_np)
        assert (c.uncert, c.ent) == (uncert, ent) and c.grid_size == one.grid_size
        assert np.array_equal(c.hal_lep_ind, one.hal_lep_ind) and np.array_equal(c.lal_hep_ind, one.lal_hep_ind)
        assert c.pdf.tobytes() == one.pdf.tobytes()
    small = epal.compare_epal(records("main"), CLASS_NAMES, mesh=7, engine=R.kde_eval_np)
    assert small.pdf.shape == (7, 7)


def test_what_is_not_built_says_so():
    for switch in ("brisque", "draw", "crops"):
        with pytest.raises(NotImplementedError):
            epal.compare_epal(records("empty"), CLASS_NAMES, engine=R.kde_eval_np, **{switch: True})
    with pytest.raises(ValueError, match="iso_percoo_albox"):
        epal.compare_epal(records("empty"), CLASS_NAMES, uncert="iso_percoo", engine=R.kde_eval_np)
    with pytest.raises(ValueError, match="no record has an IoU"):
        epal.compare_epal(records("empty"), CLASS_NAMES, iou_thr=1.0, engine=R.kde_eval_np)
    with pytest.raises(ValueError, match="no validation records"):
        epal.compare_epal([], CLASS_NAMES, engine=R.kde_eval_np)


# ---- the mirror and the host half of kde_eval against live scipy
def test_the_mirror_sums_runs_sequentially_and_folds_them_pairwise():
    rng = np.random.default_rng(3)
    d, p, w = rng.normal(size=(11, 2)), rng.normal(size=(5, 2)), rng.uniform(0.5, 2, 11)
    for weight in (None, w):
        got = R.kde_sum(d, p, weight, run=4)
        for j in range(5):
            t = []
            for i in range(11):
                arg = (p[j, 0] - d[i, 0]) ** 2 + (p[j, 1] - d[i, 1]) ** 2
                e = np.exp(arg * -0.5)
                t.append(e if weight is None else w[i] * e)
            r = [((0.0 + t[0]) + t[1] + t[2]) + t[3], ((0.0 + t[4]) + t[5] + t[6]) + t[7], ((0.0 + t[8]) + t[9]) + t[10]]
            assert got[j] == (r[0] + r[1]) + (r[2] + 0.0)
    assert R.kde_sum(d, p[:0]).shape == (0,)


@pytest.mark.parametrize("D", [1, 2, 3, 4])
@pytest.mark.parametrize("weighted", [False, True])
def test_mirror_and_host_half_equal_live_scipy(D, weighted):
    from scipy.stats import gaussian_kde
    for n, bw in ((7, None), (300, "silverman"), (5000, None), (777, 0.37)):
        rng = np.random.default_rng([D, weighted, n])
        mix = rng.normal(size=(D, D)) + 2 * np.eye(D)
        data = mix @ rng.normal(size=(D, n))
        pts = mix @ rng.normal(size=(D, 150)) * 1.5
        w = rng.uniform(0.2, 3.0, n) if weighted else None
        want = gaussian_kde(data, bw_method=bw, weights=w)(pts)
        assert close_to_scipy(R.pdf(data, pts, w, bw), want, n), (n, bw)
        got, = epal.kde_eval([data], [pts], None if w is None else [w], bw_method=bw, engine=R.kde_eval_np)
        assert close_to_scipy(got, want, n), (n, bw)


def test_far_points_underflow_as_scipy_does():
    from scipy.stats import gaussian_kde
    rng = np.random.default_rng(9)
    data = rng.normal(size=(2, 400))
    pts = np.stack([np.linspace(0, 400, 60), np.linspace(0, -300, 60)])
    want = gaussian_kde(data)(pts)
    got, = epal.kde_eval([data], [pts], engine=R.kde_eval_np)
    assert (want == 0).any() and (want > 0).any() and close_to_scipy(got, want, 400)
    assert np.array_equal(got == 0, want == 0)


def test_kde_eval_takes_a_batch_and_refuses_what_scipy_refuses():
    from scipy import linalg
    from scipy.stats import gaussian_kde
    rng = np.random.default_rng(2)
    sets = [rng.normal(size=(2, n)) for n in (5, 300, 40)]
    pts = [rng.normal(size=(2, m)) for m in (3, 0, 17)]
    w = [None, rng.uniform(1, 2, 300), None]
    got = epal.kde_eval(sets, pts, w, engine=R.kde_eval_np)
    assert [g.shape for g in got] == [(3,), (0,), (17,)]
    for k in (0, 2):
        assert close_to_scipy(got[k], gaussian_kde(sets[k])(pts[k]), sets[k].shape[1])
    one, = epal.kde_eval([rng.normal(size=50)], [np.linspace(-1, 1, 9)], engine=R.kde_eval_np)   # D = 1 as a vector
    assert one.shape == (9,)
    assert epal.kde_eval([], []) == []
    line = np.stack([np.arange(10.0), 2 * np.arange(10.0)])
    with pytest.raises(linalg.LinAlgError, match="lower-dimensional subspace"):
        epal.kde_eval([line], [np.zeros((2, 1))], engine=R.kde_eval_np)
    with pytest.raises(linalg.LinAlgError):
        gaussian_kde(line)
    with pytest.raises(ValueError, match="greater than number of samples"):
        epal.kde_eval([np.ones((3, 2))], [np.zeros((3, 1))], engine=R.kde_eval_np)
    with pytest.raises(ValueError, match="multiple elements"):
        epal.kde_eval([np.ones((1, 1))], [np.zeros((1, 1))], engine=R.kde_eval_np)
    with pytest.raises(ValueError, match="not finite"):
        epal.kde_eval([np.array([[0.0, 1.0, np.nan]])], [np.zeros((1, 1))], engine=R.kde_eval_np)
    with pytest.raises(ValueError, match="not finite"):
        epal.kde_eval([sets[0]], [np.full((2, 1), np.inf)], engine=R.kde_eval_np)
    with pytest.raises(ValueError, match="of length n"):
        epal.kde_eval([sets[0]], [pts[0]], [np.ones(4)], engine=R.kde_eval_np)
    with pytest.raises(ValueError, match="1..4"):
        epal.kde_eval([rng.normal(size=(5, 30))], [np.zeros((5, 2))], engine=R.kde_eval_np)
    with pytest.raises(ValueError, match="share one dimension"):
        epal.kde_eval([sets[0], rng.normal(size=(3, 30))], [pts[0], np.zeros((3, 2))], engine=R.kde_eval_np)
    with pytest.raises(ValueError, match="points have dimension 3"):
        epal.kde_eval([sets[0]], [np.zeros((3, 2))], engine=R.kde_eval_np)
    with pytest.raises(ValueError, match="bw_method"):
        epal.kde_eval([sets[0]], [pts[0]], bw_method="nope", engine=R.kde_eval_np)


def test_array_form_checks_its_arguments_before_the_device_is_touched():
    d, p = np.ones((4, 2)), np.zeros((3, 2))
    off = lambda *v: np.array(v, np.int64)                      # noqa: E731
    with pytest.raises(ValueError, match="not finite"):
        epal.kde_eval_np(2, np.full((4, 2), np.nan), off(0, 4), None, p, off(0, 3))
    with pytest.raises(ValueError, match="not finite"):
        epal.kde_eval_np(2, d, off(0, 4), np.array([1, 1, np.inf, 1]), p, off(0, 3))
    with pytest.raises(ValueError, match=r"weight must be"):
        epal.kde_eval_np(2, d, off(0, 4), np.ones(3), p, off(0, 3))
    with pytest.raises(ValueError, match="must hold"):
        epal.kde_eval_np(2, d, off(0, 5), None, p, off(0, 3))
    with pytest.raises(ValueError, match=r"\[B \+ 1\]"):
        epal.kde_eval_np(2, d, off(0, 4), None, p, off(0, 1, 3))


def test_binding_lists_the_entry_point_and_the_header_limits():
    assert "uda_kde_eval_np" in capi.EXPORTS
    defs = dict(re.findall(r"#define (UDA_KDE_[A-Z_]+) +\(?([0-9l<> ]+)\)?", open(capi.HEADER).read()))
    assert (int(defs["UDA_KDE_POINTS"]), int(defs["UDA_KDE_RUN"]), int(defs["UDA_KDE_MAX_D"]), int(defs["UDA_KDE_MAX_N"]),
            int(defs["UDA_KDE_MAX_B"])) == (capi.KDE_POINTS, capi.KDE_RUN, capi.KDE_MAX_D, capi.KDE_MAX_N, capi.KDE_MAX_B)
    assert defs["UDA_KDE_MAX_PAIRS"].replace(" ", "") == "1ll<<36" and capi.KDE_MAX_PAIRS == 1 << 36
    assert R.RUN == capi.KDE_RUN and capi.KDE_RUN <= capi.KDE_POINTS


def test_entry_point_fails_loudly_without_a_device():
    """No CPU fallback: without a HIP device the call returns 1 and the message names the entry point; bad arguments are refused
    before a device is looked for, and `sum` keeps what it held either way."""
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import numpy as np\n"
            "from uda_amd import capi\n"
            "lib = capi.load()\n"
            "d, p, out = np.ones((6, 3)), np.zeros((4, 3)), np.full(4, -7.0)\n"
            "big = capi.KDE_MAX_PAIRS // 6 + 1\n"
            "cases = [('ok', 3, 1, [0, 6], [0, 4]), ('nopoint', 3, 1, [0, 6], [0, 0]), ('D', 5, 1, [0, 6], [0, 4]), ('B', 3, 0, [0, 6], [0, 4]),\n"
            "         ('start', 3, 1, [1, 6], [0, 4]), ('d_desc', 3, 2, [0, 6, 5], [0, 2, 4]), ('p_desc', 3, 2, [0, 3, 6], [0, 4, 2]),\n"
            "         ('empty', 3, 2, [0, 6, 6], [0, 2, 4]), ('rows', 3, 1, [0, capi.KDE_MAX_N + 1], [0, 4]), ('pairs', 3, 1, [0, 6], [0, big])]\n"
            "for name, D, B, d_off, p_off in cases:\n"
            "    d_off, p_off = np.array(d_off, np.int64), np.array(p_off, np.int64)\n"
            "    rc = lib.uda_kde_eval_np(0, D, B, d.ctypes.data, d_off.ctypes.data, None, p.ctypes.data, p_off.ctypes.data, out.ctypes.data)\n"
            "    print('%%s|%%d|%%s|%%s' %% (name, rc, lib.uda_last_error(None).decode(), out.tolist()))\n" % ROOT)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0, res.stderr
    rows = {r[0]: r[1:] for r in (line.split("|") for line in res.stdout.splitlines()) if len(r) == 4}
    assert len(rows) == 10 and all(r[0] == "1" and r[1].startswith("uda_kde_eval_np: ") for r in rows.values()), res.stdout
    assert all(r[2] == "[-7.0, -7.0, -7.0, -7.0]" for r in rows.values())
    assert "no ROCm-capable device is detected" in rows["ok"][1]
    assert "no ROCm-capable device is detected" in rows["nopoint"][1]      # a call without a point needs its device like any other
    for name, text in (("D", "5 coordinates"), ("B", "0 problems"), ("start", "not at 0"), ("d_desc", "problem 1 descend"),
                       ("p_desc", "problem 1 descend"), ("empty", "problem 1 has no data row"), ("rows", "data rows, at most"),
                       ("pairs", "pairs of a point and a data row")):
        assert text in rows[name][1], (name, rows[name][1])
