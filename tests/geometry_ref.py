"""Helpers of the odd-size geometry tests (test_geometry_host.py, test_gpu_geometry.py); no GPU needed to import or use.

  * `oracle_run` / `oracle_taps`: every named activation of the CPU oracle for EVERY MC sample, {tap: [n, T, H, W, C]}.
  * `compare_taps`: every oracle tap the device's plan names, read back with `read_buffer` and held per tap to
    max|got - ref| <= tol * max|ref| + 1e-6; a failure names the tap (the first wrong operator, the taps are walked in
    network order) and the (row, y, x, c) of its worst element.
  * wrong-geometry variants of the oracle (context managers that patch `oracle.effdet_ref` and restore it): what a kernel
    with a plausible indexing mistake would compute.  `src = dst >> 1` for the nearest-up is NOT among them: it equals the
    reference's floor rule on every pyramid `same_out` produces (2H and 2H - 1 alike).
"""
import collections
import contextlib
import os

import numpy as np

from common import make_params  # noqa: F401  (puts the repository root on sys.path)

# the two odd-size network inputs ("WxH") and their maps from the stem down to P7
SIZES = {
    "201x137": [(69, 101), (35, 51), (18, 26), (9, 13), (5, 7), (3, 4), (2, 2)],
    "200x136": [(68, 100), (34, 50), (17, 25), (9, 13), (5, 7), (3, 4), (2, 2)],
}
# per-tap bars (relative to max|ref| of the tap): the float32-class schemes at the bar test_gpu_round5.py holds the default
# scheme to; one fp16 piece at a twelfth of the smallest first-tap deviation of a wrong geometry (0.127, measured on the oracle)
TAP_TOL = {"f16x2": 1e-4, "bf16x3": 1e-4, "f32": 1e-4, "f16": 1e-2}
LOOSEST_TAP_TOL = max(TAP_TOL.values())

TapReport = collections.namedtuple("TapReport", "count worst worst_tap names")


def oracle_run(p, w, x, seed):
    """`effdet_ref.forward_once` for every MC sample t: ({tap: [n, T, H, W, C]}, class heads, box heads), the heads stacked
    as `effdet_ref.forward` stacks them."""
    from oracle import effdet_ref as E, philox_ref as R
    sites = E.dropout_sites(p)
    T = int(p["mc_dropoutsamp"]) if p["mc_dropout"] else 1
    masks = R.make_masks(sites, seed, x.shape[0], T) if sites else None
    per_t, all_cls, all_box = [], [], []
    for t in range(T):
        taps = {}
        c, b = E.forward_once(w, p, x, masks, t, taps)
        per_t.append(taps)
        all_cls.append(c)
        all_box.append(b)
    taps = {k: np.stack([per_t[t][k] for t in range(T)], 1) for k in per_t[0]}
    if not p["mc_dropout"]:
        return taps, all_cls[0], all_box[0]
    stack = lambda runs, on: [np.stack([r[l] for r in runs], 0) for l in range(len(runs[0]))] if on else runs[-1]
    cls = stack(all_cls, bool(p["mc_classheadrate"] or p["mc_dropoutrate"]))
    box = stack(all_box, bool(p["mc_boxheadrate"] or p["mc_dropoutrate"]))
    return taps, cls, box


def oracle_taps(p, w, x, seed):
    return oracle_run(p, w, x, seed)[0]


def deferred_taps(plan):
    """Taps that are other tensors on the device BY DESIGN: a dropout site deferred into a squeeze-excite gate leaves
    the depthwise output without its keep-scale and puts the keep-scale into the gate (block 0 under full MC dropout)."""
    from uda_amd import capi
    names = {i: n for n, i in plan.buffer_names.items()}
    out = set()
    for o in plan.ops:
        if o["kind"] == capi.OP_SE and o["drop_site"] >= 0:
            out.add(names[o["out"]])
            out.add(names[o["ins"][1]])
    return out


def comparable_taps(plan, taps):
    """oracle taps the plan names, in network order, minus the by-design exceptions"""
    skip = deferred_taps(plan)
    return [k for k in taps if k in plan.buffer_names and k not in skip]


def compare_taps(driver, taps, tol):
    """Every oracle tap that `driver.plan.buffer_names` knows against `driver.read_buffer`, all images and all MC samples.
    A per-sample buffer has rows [image][sample]; a shared one has one row per image and must serve every sample of the
    oracle.  Returns TapReport(count, worst, worst_tap, names): worst = largest error in units of the bar (<= 1 passes)."""
    plan = driver.plan
    names, worst, worst_tap = [], 0.0, None
    for tap in comparable_taps(plan, taps):
        ref = taps[tap]
        n, T = ref.shape[:2]
        b = plan.bufs[plan.buffer_names[tap]]
        got = driver.read_buffer(tap, n)
        rows_t = T if b.per_sample else 1
        assert got.shape[0] == n * rows_t, (tap, got.shape, ref.shape)
        assert got.shape[1:] == ref.shape[2:], "%s: device %s, oracle %s" % (tap, got.shape[1:], ref.shape[2:])
        got = got.reshape((n, rows_t) + got.shape[1:])
        assert np.isfinite(got).all(), "%s: non-finite values on the device" % tap
        err = np.abs(got.astype(np.float64) - ref.astype(np.float64))       # (a shared buffer broadcasts over the samples)
        bar = tol * float(np.abs(ref).max()) + 1e-6
        ratio = float(err.max()) / bar
        if ratio > 1.0:
            i, t, y, x, c = np.unravel_index(int(np.argmax(err)), err.shape)
            raise AssertionError("%s: error %.4g above %g * max|ref| + 1e-6 = %.4g (max|ref| %.4g) at (row %d, y %d, x %d, c %d) of "
                                 "[%d, %d, %d, %d]: device %.7g, oracle %.7g" % (
                                     tap, err.max(), tol, bar, np.abs(ref).max(), i * rows_t + (t if rows_t > 1 else 0), y, x, c,
                                     n * rows_t, ref.shape[2], ref.shape[3], ref.shape[4],
                                     got[i, t if rows_t > 1 else 0, y, x, c], ref[i, t, y, x, c]))
        if ratio > worst:
            worst, worst_tap = ratio, tap
        names.append(tap)
    return TapReport(len(names), worst, worst_tap, names)


def absorbed_outputs(plan):
    """block outputs that exist on no device: a projection the NEXT block's fused kernel computes in its prologue (plan.py,
    `absorb`: block 0's 16-channel tensor under the split schemes) is never stored - its first stored consumer, the next
    block's depthwise tap, is compared instead"""
    from uda_amd import capi
    names = {i: n for n, i in plan.buffer_names.items()}
    out = set()
    for o in plan.ops:
        if o["kind"] == capi.OP_MBX and o["se_scale"] >= 0:
            out.add("blocks_%d/out" % (int(names[o["out"]].split("/")[0].split("_")[1]) - 1))
    return out


def required_taps(taps, plan):
    """the taps no lowering may leave out: stem, every block output it stores, P6 / P7, every BiFPN node"""
    gone = absorbed_outputs(plan)
    return [k for k in taps if k == "stem" or (k.startswith("blocks_") and k.endswith("/out") and k not in gone)
            or k in ("p6_in", "p7_in") or (k.startswith("cell") and k.endswith("/out"))]


@contextlib.contextmanager
def plan_switches(**env):
    """Planner switches (plan.PLAN_SWITCHES, read once per Plan) for the construction of ONE driver: set inside, restored after."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ------------------------------------------------------------------ wrong geometries
@contextlib.contextmanager
def _patched(name, fn):
    from oracle import effdet_ref as E
    orig = getattr(E, name)
    setattr(E, name, fn)
    try:
        yield
    finally:
        setattr(E, name, orig)


def swapped_same_pad():
    """TF SAME with the halves swapped: the larger half in front.  Differs wherever the total padding is odd (stride 2 on an
    even input); an odd input pads (1, 1) either way."""
    import torch.nn.functional as F

    def _same_pad(x, k, s, value=0.0):
        H, W = x.shape[-2:]
        ph = max((-(-H // s) - 1) * s + k - H, 0)
        pw = max((-(-W // s) - 1) * s + k - W, 0)
        if ph or pw:
            x = F.pad(x, (pw - pw // 2, pw // 2, ph - ph // 2, ph // 2), value=value)
        return x
    return _patched("_same_pad", _same_pad)


def zero_padded_max_pool():
    """max pool whose padding takes part in the maximum as 0 instead of never winning"""
    import torch.nn.functional as F
    from oracle import effdet_ref as E

    def max_pool_same(x, k, s):
        return F.max_pool2d(E._same_pad(x, k, s, value=0.0), k, s)
    return _patched("max_pool_same", max_pool_same)


def _nearest(src_of):
    import torch

    def nearest_upsample(x, th, tw):
        H, W = x.shape[-2:]
        ys = torch.clamp(src_of(torch.arange(th, dtype=torch.float32), H / th).long(), min=0, max=H - 1)
        xs = torch.clamp(src_of(torch.arange(tw, dtype=torch.float32), W / tw).long(), min=0, max=W - 1)
        return x[:, :, ys][:, :, :, xs]
    return _patched("nearest_upsample", nearest_upsample)


def half_pixel_nearest_up():
    """src = floor((dst + 0.5) * in / out): half_pixel_centers=True"""
    import torch
    return _nearest(lambda d, s: torch.floor((d + 0.5) * s))


def rounded_nearest_up():
    """src = round(dst * in / out): align-to-nearest instead of floor"""
    import torch
    return _nearest(lambda d, s: torch.floor(d * s + 0.5))


VARIANTS = {"swapped_same_pad": swapped_same_pad, "zero_padded_max_pool": zero_padded_max_pool,
            "half_pixel_nearest_up": half_pixel_nearest_up, "rounded_nearest_up": rounded_nearest_up}


def first_changed_tap(ref_taps, taps):
    """(tap, max|a - b| / max|b|) of the first tap (network order) that is not bit-equal, or (None, 0.0)"""
    for k, r in ref_taps.items():
        if not np.array_equal(taps[k], r):
            return k, float(np.abs(taps[k].astype(np.float64) - r).max() / np.abs(r).max())
    return None, 0.0
