"""The NMS kernels at their boundaries and on degenerate inputs (run with -m gpu on an MI355X).

Every execution path `run_nms` can take - `nms_reg_kernel<1|2|3|4|6|8>`, `nms_solo_kernel`, the co-resident grid
`nms_coop_kernel<4|8|24>`, the two-launches-per-epoch grid, the score prefix - is driven through `d.nms` with the inputs
of tests/nms_cases.py (every kind x every parameter set) at candidate counts on the edges of its index arithmetic, and
compared with the oracle's NonMaxSuppressionV5 bit for bit: `valid`, the indices, the scores as uint32.  The one case
`uda_nms` refuses (soft NMS with a negative threshold over a live negative score: the scores grow, see include/uda_hip.h)
must be refused, with a message, and is not compared.

The switches that select a path are read once per process, so each path runs in its own interpreter: one worker per
path, three problems per call (two seeds, and a third with half of its candidates at or just below the threshold)."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r"""
import json, sys, time
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import numpy as np
import nms_cases as NC
from common import make_params, make_weights
from uda_amd import capi
from uda_amd.infer_lib import KerasDriver, ServingDriver
from oracle import post_ref as P
cfg = json.loads(sys.argv[1])
p = make_params()
d = KerasDriver("_", False, p["name"], batch_size=4, model_params=p, weights=make_weights(p))
t0 = time.time()
inputs = {}
def problem(kind, K, ps, j):
    key = (kind, K, j, NC.takes_inf(ps))
    if key not in inputs:
        inputs[key] = NC.make_for(kind, K, ps, seed=j)
    b, s = inputs[key]
    return b, (NC.half_below(s, ps, j) if j == 2 else s)
failures = []
def compare(tag, boxes, scores, ps):
    idx, sc, valid = d.nms(boxes, scores, ps[0], ps[1], ps[2], ps[3])
    for i in range(len(scores)):
        ridx, rsc, rvalid = P.nms_v5(boxes[i], scores[i], ps[0], ps[1], ps[2], ps[3], True)
        if valid[i] != rvalid:
            failures.append((tag, i, "valid", int(valid[i]), int(rvalid)))
        elif not (idx[i] == ridx).all():
            j = int(np.argmax(idx[i] != ridx))
            failures.append((tag, i, "index at", j, int(idx[i][j]), int(ridx[j])))
        elif not (NC.bits(sc[i]) == NC.bits(rsc)).all():
            j = int(np.argmax(NC.bits(sc[i]) != NC.bits(rsc)))
            failures.append((tag, i, "score bits at", j, hex(NC.bits(sc[i])[j]), hex(NC.bits(rsc)[j])))
    return valid
compared = refused = 0
fell_by_kind = {}
for K in cfg["sizes"]:
    for kind in NC.KINDS:
        for ps in NC.PARAM_SETS:
            probs = [problem(kind, K, ps, j) for j in range(3)]
            boxes = np.stack([b for b, _ in probs]); scores = np.stack([s for _, s in probs])
            tag = (cfg["id"], kind, K, ps)
            before = d.nms_prefix_fallbacks()
            if any(NC.grows(ps, s) for s in scores):
                try:
                    d.nms(boxes, scores, ps[0], ps[1], ps[2], ps[3])
                except capi.UdaError as e:
                    assert "soft NMS" in str(e) and "negative score" in str(e), (tag, str(e))
                    refused += 1
                else:
                    raise AssertionError(("growing scores were not refused", tag))
                continue
            compare(tag, boxes, scores, ps)
            compared += 1
            fell = d.nms_prefix_fallbacks() - before
            assert 0 <= fell <= 3, (tag, fell)
            fell_by_kind[kind] = fell_by_kind.get(kind, 0) + fell
if cfg.get("prefix"):
    assert fell_by_kind["grid"] > 0 and fell_by_kind["nested_identical"] > 0, fell_by_kind
    for K in cfg["sizes"]:          # the sparse control: nothing overlaps, the prefix holds every winner
        ps = NC.PARAM_SETS[0]
        probs = [NC.sparse_boxes(K, j) for j in range(3)]
        boxes = np.stack([b for b, _ in probs]); scores = np.stack([s for _, s in probs])
        before = d.nms_prefix_fallbacks()
        valid = compare((cfg["id"], "sparse", K, ps), boxes, scores, ps)
        assert (valid == ps[0]).all() and not failures, failures[:5]
        assert d.nms_prefix_fallbacks() == before, ("sparse control fell back", K)
else:
    assert sum(fell_by_kind.values()) == 0, fell_by_kind
if cfg.get("coop"):
    assert d.nms_coop_fallbacks() == 0 and d.nms_coop_not_launched() == 0, (d.nms_coop_fallbacks(), d.nms_coop_not_launched())
for f in failures[:60]:
    print("MISMATCH", f)
assert not failures, "%%d problems differ from the oracle" %% len(failures)
assert refused > 0 and compared > 10 * refused
print("edges ok %%s: %%d calls compared, %%d refused, prefix redone %%s, %%.1f s" %% (cfg["id"], compared, refused, fell_by_kind, time.time() - t0))
d.close()
"""


def _nms_chunk():
    """NMS_CHUNK of the build: 256 * UDA_NMS_ITEMS (csrc/kernels_nms.hip, unless the Makefile defines it)."""
    csrc = os.path.join(ROOT, "uncertainty-detection-autolabeling_amd", "csrc")
    items = None
    with open(os.path.join(csrc, "Makefile")) as f:
        m = re.search(r"-DUDA_NMS_ITEMS=(\d+)", f.read())
        if m:
            items = int(m.group(1))
    if items is None:
        with open(os.path.join(csrc, "kernels_nms.hip")) as f:
            items = int(re.search(r"#define UDA_NMS_ITEMS (\d+)", f.read()).group(1))
    return 256 * items


def _coop_sizes(ipt):
    return [1, 1025, ipt * 1024, ipt * 1024 + 1, 8193]


CHUNK = _nms_chunk()
SOLO0 = dict(UDA_NMS_SOLO="0")
PATHS = [
    # id, environment, sizes, flags, timeout (s)
    ("registers", {}, [1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3072, 3073, 4096, 4097, 6144, 6145, 8191, 8192], {}),
    ("solo", dict(UDA_NMS_REG="0"), [1, 65, 1024, 1025, 4097, 8192], {}),
    ("hand-over", {}, [8193], dict(coop=True)),
    ("coop-small", SOLO0, _coop_sizes(4), dict(coop=True)),             # K <= 8193, three problems: the launcher picks IPT 4
    ("coop-small-ipt8", dict(SOLO0, UDA_NMS_COOP_IPT="8"), _coop_sizes(8), dict(coop=True)),
    ("coop-small-ipt24", dict(SOLO0, UDA_NMS_COOP_IPT="24"), _coop_sizes(24), dict(coop=True)),
    ("grid", dict(UDA_NMS_SOLO="0", UDA_NMS_COOP="0", UDA_NMS_PREFIX="0"),
     [1, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1], {}),
    ("prefix-small", dict(UDA_NMS_SOLO="256", UDA_NMS_COOP="0", UDA_NMS_PREFIX="128"), [257, 513, 600, 4097], dict(prefix=True)),
]
# every switch a path does not set must be at its default, whatever the caller's environment says
SWITCHES = ("UDA_NMS_SOLO", "UDA_NMS_REG", "UDA_NMS_COOP", "UDA_NMS_COOP_IPT", "UDA_NMS_PREFIX", "UDA_NMS_WINNERS",
            "UDA_NMS_COOP_SPIN", "UDA_NMS_COOP_CAP")


@pytest.mark.parametrize("pid,env,sizes,flags", PATHS, ids=[p[0] for p in PATHS])
def test_nms_path_at_its_edges(pid, env, sizes, flags):
    # the smallest sizes at which a path's index arithmetic can go wrong: nothing above 8193 candidates, except the block edge
    # IPT * 1024 (+ 1) of the cooperative kernel with 24 candidates per thread
    assert max(sizes) <= (24 * 1024 + 1 if env.get("UDA_NMS_COOP_IPT") == "24" else 8193)
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env)
    cfg = dict(flags, id=pid, sizes=sizes)
    r = subprocess.run([sys.executable, "-c", WORKER % {"root": ROOT}, json.dumps(cfg)], cwd=ROOT, env=e,
                       capture_output=True, text=True, timeout=60)      # (a worker takes 1 - 4 s)
    last = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    print(last)
    for line in sorted({l for l in r.stderr.splitlines() if l.startswith("[uda] cooperative NMS:")})[:16]:
        print(line)                 # (UDA_NMS_DEBUG=1: the shapes of the co-resident grid this path launched)
    assert r.returncode == 0 and last.startswith("edges ok " + pid), (r.returncode, r.stdout[-6000:], r.stderr[-3000:])
