"""Generates tests/golden/similarity_golden.npz by running the REAL reference functions `emp_KL_divergence`,
`empirical_jensen_shannon_divergence` and `Similarity.calculate_set_similarity` (src/active_learning_eval.py:458-583, 946-1029)
on sets made here.  Their bodies are numpy and scipy only; the module imports TensorFlow and friends at the top, which are
stubbed.  Run once where a checkout of the reference and scipy exist; the .npz (data only) is committed and is what the tests
read.

    python tests/golden/make_similarity_golden.py <src directory of the reference's checkout>

Every case is recorded twice: as shipped (the KD-trees are queried with eps=0.01: `*_eps`), and under a shim, in this maker only,
that forwards `KDTree.query` with eps=0 (`*_exact`) - the values this project's exact search has to equal bit for bit.

Two more shims, in this maker only: `emp_KL_divergence` is wrapped to capture the three resampled sets of a JSD, and the
`num_samples=10000` that calculate_set_similarity hard-codes is lowered to SIM_SAMPLES by a wrapper around the real JSD function.

Stored:
  kl_cases, kl_<c>_p / _q (sets), kl_<c>_eps / _exact                                   the estimator
  jsd_cases, jsd_<c>_P / _Q (inputs), _n (num_samples), _sp / _sq / _sm (resampled sets),
             _kl_eps / _kl_exact ([kl_PM, kl_QM]), _jsd_eps / _jsd_exact                 the JSD
  sim_classes, sim_methods, sim_samples, sim_in_<set>_<class> ([3, boxes]; [0] = the set has no box of the class; the last set
             is the reference set), sim_perclass_eps / _exact [classes, methods], sim_names_eps / _exact and
             sim_values_eps / _exact (the sorted pairs), sim_flag_eps / _exact            the table"""
import os
import sys
from unittest import mock

sys.dont_write_bytecode = True          # never write into the reference's checkout
if len(sys.argv) != 2:
    sys.exit("usage: make_similarity_golden.py <src directory of a checkout of the reference>")
REF_SRC = sys.argv[1]
for name in ("tensorflow", "cv2", "matplotlib", "matplotlib.lines", "matplotlib.patches", "matplotlib.pyplot", "matplotlib.colors",
             "matplotlib.path", "seaborn", "yaml", "tensorboard", "tensorboard.backend", "tensorboard.backend.event_processing",
             "tensorboard.backend.event_processing.event_accumulator", "datasets", "datasets.BDD100K",
             "datasets.BDD100K.bdd_tf_creator", "datasets.CODA", "datasets.CODA.coda_tf_creator", "datasets.KITTI",
             "datasets.KITTI.kitti_tf_creator"):
    sys.modules[name] = mock.MagicMock()
sys.path.insert(0, REF_SRC)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np                       # noqa: E402
import active_learning_eval as ALE      # noqa: E402  (the reference module)
import knn_ref as R                      # noqa: E402  (to assert that the mirror is the eps=0 reference)

SIM_SAMPLES = 300
SHIPPED_TREE = ALE.KDTree


class ExactTree:
    """The reference's KD-tree with every query forwarded at eps=0."""

    def __init__(self, data):
        self.tree = SHIPPED_TREE(data)

    def query(self, x, k=1, eps=0, p=2):
        return self.tree.query(x, k=k, eps=0, p=p)


def both(fn):
    """fn() as shipped and under the exact tree."""
    shipped = fn()
    with mock.patch.object(ALE, "KDTree", ExactTree):
        exact = fn()
    return shipped, exact


def lognormal(rng, n, d, shift=0.0):
    return np.exp(rng.normal(shift, 0.6, (n, d)) + np.arange(d) * 0.3)


def kl_cases(rng):
    c = {"d1": (lognormal(rng, 300, 1), lognormal(rng, 250, 1, 0.2)),
         "d3": (lognormal(rng, 200, 3), lognormal(rng, 150, 3, 0.2)),
         "d4": (lognormal(rng, 120, 4), lognormal(rng, 100, 4, -0.1))}
    p, q = lognormal(rng, 60, 3), lognormal(rng, 50, 3, 0.1)
    p[41] = p[7]                                               # an exact duplicate inside P: dp = 0, KL = +inf
    c["d3_dup"] = (p, q)
    p, q = lognormal(rng, 60, 3), lognormal(rng, 50, 3, 0.1)
    q[13] = p[20]                                              # a point common to P and Q: dq = 0, KL = -inf
    c["d3_common"] = (p, q)
    p, q = lognormal(rng, 60, 3), lognormal(rng, 50, 3, 0.1)
    p[3] = p[50]
    q[0] = p[31]                                               # both: +inf and -inf in one sum, KL = nan
    c["d3_both"] = (p, q)
    return c


def jsd_cases(rng):
    p = lognormal(rng, 90, 3)
    p[17, 1] = 0.0                                             # log -> -inf: the box is filtered out
    return {"a": (p, lognormal(rng, 110, 3, 0.3), 150), "b": (lognormal(rng, 40, 3, -0.2), lognormal(rng, 70, 3), 200)}


def run_jsd(P, Q, n):
    seen = []
    real = ALE.emp_KL_divergence

    def capture(sample_p, sample_q):
        seen.append((np.array(sample_p), np.array(sample_q)))
        return real(sample_p, sample_q)

    with mock.patch.object(ALE, "emp_KL_divergence", capture):
        jsd = ALE.empirical_jensen_shannon_divergence(P, Q, num_samples=n)
    (sp, sm), (sq, sm2) = seen
    assert np.array_equal(sm, sm2)
    return dict(sp=sp, sq=sq, sm=sm, kl=np.array([real(sp, sm), real(sq, sm)]), jsd=np.array([jsd]))


def sim_table(rng):
    """3 classes x 3 methods plus the reference set; method `entropy` has no box of class `cyclist`."""
    classes, methods = ["car", "pedestrian", "cyclist"], ["random", "entropy", "mcbox"]
    boxes = {"random": (80, 40, 25), "entropy": (60, 55, 0), "mcbox": (70, 20, 30), "val": (90, 50, 35)}
    sets = []
    for s, name in enumerate(methods + ["val"]):
        sets.append({cl: ([list(row) for row in lognormal(rng, n, 3, 0.1 * s + 0.15 * c).T] if n else [])
                     for c, (cl, n) in enumerate(zip(classes, boxes[name]))})
    return classes, methods, sets


def run_sim(classes, methods, sets):
    real = ALE.empirical_jensen_shannon_divergence
    with mock.patch.object(ALE, "empirical_jensen_shannon_divergence", lambda P, Q, num_samples: real(P, Q, num_samples=SIM_SAMPLES)):
        pairs, flag, perclass = ALE.Similarity.calculate_set_similarity(sets, classes, methods, return_perclass=True)
    return dict(names=np.array([k for k, _ in pairs]), values=np.array([v for _, v in pairs], np.float64), flag=np.array([bool(flag)]),
                perclass=np.asarray(perclass, np.float64))


def main():
    rng = np.random.default_rng(20241019)
    out = {}
    kc = kl_cases(rng)
    out["kl_cases"] = np.array(list(kc))
    for c, (p, q) in kc.items():
        eps, exact = both(lambda: ALE.emp_KL_divergence(p, q))
        out.update({"kl_%s_p" % c: p, "kl_%s_q" % c: q, "kl_%s_eps" % c: np.array([eps]), "kl_%s_exact" % c: np.array([exact])})
        mirror = R.emp_kl(p, q)
        assert np.array([mirror]).tobytes() == np.array([exact]).tobytes(), (c, mirror, exact)
        print("kl  %-10s D %d  exact %-22r eps - exact %r" % (c, p.shape[1], exact, eps - exact))
    assert out["kl_d3_dup_exact"][0] == np.inf and out["kl_d3_common_exact"][0] == -np.inf and np.isnan(out["kl_d3_both_exact"][0])
    jc = jsd_cases(rng)
    out["jsd_cases"] = np.array(list(jc))
    for c, (P, Q, n) in jc.items():
        eps, exact = both(lambda: run_jsd(P, Q, n))
        for k in ("sp", "sq", "sm"):
            assert np.array_equal(eps[k], exact[k])            # the resampling does not know about the trees
            out["jsd_%s_%s" % (c, k)] = exact[k]
        out.update({"jsd_%s_P" % c: P, "jsd_%s_Q" % c: Q, "jsd_%s_n" % c: np.array([n])})
        for k in ("kl", "jsd"):
            out["jsd_%s_%s_eps" % (c, k)], out["jsd_%s_%s_exact" % (c, k)] = eps[k], exact[k]
        mirror = np.array([R.emp_kl(exact["sp"], exact["sm"]), R.emp_kl(exact["sq"], exact["sm"])])
        assert mirror.tobytes() == exact["kl"].tobytes() and 0.5 * (mirror[0] + mirror[1]) == exact["jsd"][0]
        print("jsd %-10s n %d  exact %r  eps - exact: kl %s jsd %r" % (c, n, exact["jsd"][0], (eps["kl"] - exact["kl"]).tolist(),
                                                                         eps["jsd"][0] - exact["jsd"][0]))
    classes, methods, sets = sim_table(rng)
    out.update(sim_classes=np.array(classes), sim_methods=np.array(methods), sim_samples=np.array([SIM_SAMPLES]))
    for s, entry in enumerate(sets):
        for cl in classes:
            out["sim_in_%d_%s" % (s, cl)] = np.asarray(entry[cl], np.float64) if len(entry[cl]) else np.zeros(0)
    eps, exact = both(lambda: run_sim(classes, methods, sets))
    for k in ("names", "values", "flag", "perclass"):
        out["sim_%s_eps" % k], out["sim_%s_exact" % k] = eps[k], exact[k]
    assert np.isnan(exact["perclass"][2, 1]) and np.isfinite(np.delete(exact["perclass"].reshape(-1), 7)).all()
    print("sim exact %s flag %s\n    eps - exact %s" % (list(zip(exact["names"].tolist(), exact["values"].tolist())), exact["flag"][0],
                                                         (eps["perclass"] - exact["perclass"]).tolist()))
    dst = os.path.join(HERE, "similarity_golden.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")
    assert os.path.getsize(dst) < 100000


if __name__ == "__main__":
    main()
