"""GPU tests of the opt-in one-piece bf16 scheme (`uda_pw_scheme = "bf16"`, UDA_SPLIT_BF16X1 = 6: one bf16 piece per operand, one
v_mfma_f32_32x32x16_bf16 product per k-step, float32 accumulation and epilogues - the operands of Keras mixed_bfloat16).

Op level: elementwise inside the bound of the rounding-exact model (tests/bf16x1_ref.py: float32 accumulation error only, derived).
Network level: worst relative rms per head level and channel group against the float32 CPU oracle; the bounds are the values
measured on an MI355X times at most 4:
    measured  full_mc 3.02e-3  head_mc 3.02e-3  d2 2.48e-3   (all of it in the box heads; the class heads sit at ~4e-6 here)
    against a bf16x3 handle on the same inputs: operand near 1e6 3.41e-3 (bar: full_mc's), deferred-input sep x 2^30 2.48e-3 (d2's)
    block 3's taps against the oracle's: expanded tensor 5.8e-3, projection output 7.5e-3 of the tap's maximum (bar 1e-2, not ours)
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from common import FULL_MC, HEAD_MC, ROOT, make_images, make_params, make_weights

pytestmark = pytest.mark.gpu

UDA_OP_SEP = 8
UDA_SPLIT_BF16X1 = 6
HEAD_RMS = {"full_mc": 1.2e-2, "head_mc": 1.2e-2, "d2": 9.9e-3}
TAP_TOL = 1e-2          # the per-tap bar of tests/test_gpu_geometry.py for a one-piece scheme (of the tap's maximum)
SEED = 7


def _driver(p, w, batch, scheme, **kw):
    from uda_amd.infer_lib import KerasDriver
    d = KerasDriver("_", False, p["name"], batch, False, dict(p, uda_pw_scheme=scheme), weights=w, **kw)
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


# ---------------------------------------------------------------- op level: uda_debug_pw(terms = 8)
OP_CASES = [
    # rows_in, in_div, hw, cin, cout, flags
    (1, 1, 1, 8, 4, ""),                        # one pixel, half a k-step
    (1, 1, 77, 24, 144, "bn,act"),              # a partial second k-step
    (2, 2, 100, 64, 63, "bias"),                # column tails
    (2, 1, 100, 64, 72, "bias"),
    (3, 1, 31, 88, 528, "bn,act"),              # row tail, cin not a multiple of 16
    (2, 1, 129, 672, 112, "bn,se,res"),         # the gate before the rounding
    (1, 1, 96, 1152, 320, "bn,se"),             # the K-heavy one-wave kernel
    (1, 3, 200, 16, 96, "bn,act,mask"),         # shared input rows
    (2, 5, 300, 32, 16, "bn,se"),
]


def _op_inputs(case, seed):
    rows_in, in_div, hw, cin, cout, flags = case
    f = set(flags.split(",")) if flags else set()
    rng = np.random.default_rng(seed)
    rows = rows_in * in_div
    x = rng.normal(0, 1, (rows_in, hw, cin)).astype(np.float32)
    w = (rng.normal(0, 1, (cin, cout)) / np.sqrt(cin)).astype(np.float32)
    bias = rng.normal(0, 0.5, cout).astype(np.float32) if "bias" in f else None
    sc = rng.uniform(0.5, 1.5, cout).astype(np.float32) if "bn" in f else None
    sh = rng.normal(0, 0.3, cout).astype(np.float32) if "bn" in f else None
    se = rng.uniform(0.1, 1.0, (rows_in, cin)).astype(np.float32) if "se" in f else None
    mask = ((rng.uniform(0, 1, (rows, cout)) >= 0.1) / 0.9).astype(np.float32) if "mask" in f else None
    res = rng.normal(0, 1, (rows, hw, cout)).astype(np.float32) if "res" in f else None
    return (x, w, bias, sc, sh, se, mask, res, in_div, int("act" in f))


def _check_model(got, args, separate):
    """|got - model| <= bound elementwise (as test_gpu_ops._check_model); with `separate`, the exact-operand model and the
    fp16-rounded model must each fall outside the bound on more than half the outputs that dropout does not zero.
    Returns the worst err / bound."""
    import bf16x1_ref as B
    from oracle import split_ref as S
    x, w, bias, sc, sh, se, mask, res, in_div, act = args
    val, bnd = B.pointwise(x, w, bias, sc, sh, se, mask, res, in_div, act)
    diff = np.abs(got.astype(np.float64) - val)
    ratio = np.where(bnd > 0, diff / np.where(bnd > 0, bnd, 1.0), np.where(diff == 0, 0.0, np.inf))   # (0 / 0: a dropped output)
    worst = float(ratio.max())
    assert worst <= 1.0, ("outside the model's bound", worst, np.unravel_index(int(np.argmax(ratio)), ratio.shape))
    if separate:
        exact, _ = B.pointwise(x, w, bias, sc, sh, se, mask, res, in_div, act, exact_operands=True)
        half, _ = S.pointwise(x, w, bias, sc, sh, se, mask, res, in_div, act, S.F16X1)
        for name, wrong in (("exact operands", exact), ("fp16 operands", half)):
            away = np.abs(got.astype(np.float64) - wrong) > bnd
            if mask is not None:          # (outputs that dropout zeroes are exact under any model)
                away = away[np.broadcast_to(mask[:, None, :] != 0, away.shape)]
            assert away.mean() > 0.5, ("the bound does not separate rounding models", name, float(away.mean()))
    return worst


@pytest.mark.parametrize("case", OP_CASES, ids=lambda c: "%dx%d_hw%d_%d-%d_%s" % c)
def test_pointwise_is_inside_the_models_bound(case):
    import bf16x1_ref as B
    from test_gpu_ops import _run
    args = _op_inputs(case, 500 + OP_CASES.index(case))
    got, _ = _run(*args, B.TERMS)
    worst = _check_model(got, args, separate=case[3] >= 16)
    print("terms 8 %s: worst err / bound %.3f" % (case, worst))


@pytest.mark.parametrize("big", [1e6, 1e30])
def test_pointwise_takes_inputs_far_above_fp16_range(big):
    """An input of 1e6 / 1e30 (case two: 24 -> 144, BN + swish): rc 0, finite outputs inside the model's bound.  Both fp16
    schemes fail the same call by design (terms 1 / 16: `an input above 65504 cannot be split`)."""
    import bf16x1_ref as B
    from test_gpu_ops import _run
    args = list(_op_inputs(OP_CASES[1], 501))
    args[0] = args[0].copy()
    args[0][0, 40, 5] = np.float32(big)
    args[0][0, 41, 17] = np.float32(-big)
    rc, msg = _run(*args, B.TERMS, expect_rc=True)
    assert rc == 0, msg
    got, _ = _run(*args, B.TERMS)
    assert np.isfinite(got).all()
    _check_model(got, args, separate=False)
    rc, msg = _run(*args, 1, expect_rc=True)
    assert rc != 0 and "65504" in msg


# ---------------------------------------------------------------- network level
_REF, _DEV = {}, {}


def _case_params(case):
    if case == "d2":
        return make_params(model="efficientdet-d2", image_size="256x256", **FULL_MC)
    return make_params(**(FULL_MC if case == "full_mc" else HEAD_MC))


def _reference(case):
    """(params, weights, images, oracle taps, oracle class heads, oracle box heads): computed once per case, read-only"""
    if case not in _REF:
        import geometry_ref as G
        from oracle import preprocess_ref as PP
        p = _case_params(case)
        w = make_weights(p, seed=3)
        wd, h = [int(v) for v in p["image_size"].split("x")]
        imgs = make_images(2, 100, 180, seed=4)
        x, _ = PP.preprocess(imgs, (h, wd), p["mean_rgb"], p["stddev_rgb"])
        taps, rcls, rbox = G.oracle_run(p, w, x, SEED)
        for a in list(taps.values()) + list(rcls) + list(rbox):
            a.setflags(write=False)
        _REF[case] = (p, w, imgs, taps, rcls, rbox)
    return _REF[case]


def _device(case):
    """One bf16 serve of the case: heads, range_demotions, per-op schemes and (full_mc) the two buffers of block 3"""
    if case not in _DEV:
        p, w, imgs = _reference(case)[:3]
        # (full_mc: every buffer keeps an arena slot of its own, so that block 3's can be read after the run)
        d = _driver(dict(p, uda_keep_buffers=True) if case == "full_mc" else p, w, 2, "bf16")
        d.set_dropout_seed(SEED)
        d.serve(imgs)
        cls, box = d.head_outputs(2)
        out = dict(cls=cls, box=box, demotions=d.range_demotions(), ops=d.plan.ops,
                   schemes=[d.op_scheme(i) for i in range(len(d.plan.ops))])
        if case == "full_mc":
            out["bufs"] = {k: d.read_buffer(k, 2) for k in ("blocks_3/dw", "blocks_3/out")}
            out["per_sample"] = {k: d.plan.bufs[d.plan.buffer_names[k]].per_sample for k in out["bufs"]}
            out["storage"] = {k: d.plan.bufs[d.plan.buffer_names[k]].storage for k in out["bufs"]}
        d.close()
        _DEV[case] = out
    return _DEV[case]


@pytest.mark.parametrize("case", ["full_mc", "head_mc", "d2"])
def test_heads_against_the_oracle(case, capsys):
    """Small size, every head level against the float32 CPU oracle: full MC dropout, head-only MC (the first head layer takes
    the deferred dropout site: sep_kernel's TIN mode) and D2 (BiFPN / heads at 112 channels).  Nothing is demoted, every split
    contraction runs scheme 6."""
    rcls, rbox = _reference(case)[4:]
    dev = _device(case)
    errs = [_rel_rms(g, r) for g, r in zip(dev["cls"] + dev["box"], list(rcls) + list(rbox))]
    with capsys.disabled():
        print("\n[bf16 heads vs oracle, %s] relative rms per level (cls, box): %s" % (case, " ".join("%.2e" % e for e in errs)))
    assert all(np.isfinite(g).all() for g in dev["cls"] + dev["box"])
    assert dev["demotions"] == 0
    assert {s[0] for s in dev["schemes"]} == {UDA_SPLIT_BF16X1, -1}
    assert all(s[1] == 1.0 and s[2] == 1.0 for s in dev["schemes"])           # weight scale 1, unscaled depthwise taps
    assert max(errs) <= HEAD_RMS[case], errs


def test_expanded_tensor_is_stored_as_bf16_and_widened(capsys):
    """Block 3's fused front half under full MC: every value `read_buffer` returns has its low 16 bits zero (a bf16 value, widened
    by a shift) and the tap is within the per-tap bar of the oracle's; the projection's output stays float32."""
    from uda_amd import capi
    taps = _reference("full_mc")[3]
    dev = _device("full_mc")
    marked = [i for i, s in enumerate(dev["schemes"]) if s[3]]
    assert marked and all(dev["ops"][i]["kind"] == capi.OP_MBX for i in marked)       # 16-bit outputs: fused front halves only
    assert dev["storage"] == {"blocks_3/dw": "bf16", "blocks_3/out": "f32"}
    for name in ("blocks_3/dw", "blocks_3/out"):
        got, ref = dev["bufs"][name], taps[name]
        n, T = ref.shape[:2]
        got = got.reshape((n, T if dev["per_sample"][name] else 1) + got.shape[1:])
        err = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
        bar = TAP_TOL * float(np.abs(ref).max()) + 1e-6
        with capsys.disabled():
            print("\n[bf16 tap %s] error %.3g of max|ref| (bar %g)" % (name, err / float(np.abs(ref).max()), TAP_TOL))
        assert np.isfinite(got).all() and err <= bar, (name, err, bar)
        low = got.view(np.uint32) & 0xFFFF
        if name == "blocks_3/dw":
            assert got.any() and not low.any()
        else:
            assert (low != 0).mean() > 0.9


# ---------------------------------------------------------------- range: the point of the feature
def _heads_of(p, w, imgs, scheme, seed):
    d = _driver(p, w, 2, scheme)
    ops = d.plan.ops
    d.set_dropout_seed(seed)
    det = d.serve(imgs)
    out = dict(det=det, heads=d.head_outputs(2), demotions=d.range_demotions(), ops=ops,
               schemes=[d.op_scheme(i)[0] for i in range(len(ops))])
    d.close()
    return out


def test_operand_near_1e6_is_served_without_a_demotion(capfd):
    """The weights of test_gpu_range_paths._overflow_block3 (an A operand of block 3's projection near 1e6): the fp16 schemes
    demote the op and serve the run again; bf16 serves it once, every op on scheme 6, and matches a bf16x3 handle."""
    from test_gpu_range_paths import _overflow_block3
    p = make_params(**FULL_MC)
    w = _overflow_block3(make_weights(p, seed=81))
    imgs = make_images(2, 100, 180, seed=82)
    dev, ref = _heads_of(p, w, imgs, "bf16", 5), _heads_of(p, w, imgs, "bf16x3", 5)
    assert dev["demotions"] == 0 and set(dev["schemes"]) == {UDA_SPLIT_BF16X1, -1}
    assert "fp16 range" not in capfd.readouterr().err
    assert all(np.isfinite(x).all() for x in dev["det"][:3])
    assert all(np.isfinite(g).all() for g in dev["heads"][0] + dev["heads"][1])
    errs = [_rel_rms(g, r) for g, r in zip(dev["heads"][0] + dev["heads"][1], ref["heads"][0] + ref["heads"][1])]
    print("[bf16 operand 1e6 vs bf16x3] relative rms per level: %s" % " ".join("%.2e" % e for e in errs))
    assert max(errs) <= HEAD_RMS["full_mc"], errs


def test_deferred_input_sep_beyond_fp16_range_is_served():
    """D2 under head-only MC dropout, class-net layer 1's depthwise taps x 2^30 and its 1x1 kernel x 2^-30
    (test_gpu_range_paths.test_deferred_input_sep_overflow_is_refused_before_anything_changes): both fp16 schemes refuse that
    serve - the deferred-input separable conv has no three-piece kernel to fall back to.  bf16 serves it: the ten deferred-input
    ops keep scheme 6 and the heads match a bf16x3 handle."""
    p = make_params(model="efficientdet-d2", image_size="256x256", **HEAD_MC)
    w = dict(make_weights(p, seed=3))
    dk, pk = "class_net/class-1/depthwise_kernel", "class_net/class-1/pointwise_kernel"
    w[dk] = w[dk] * np.float32(2.0 ** 30)
    w[pk] = w[pk] * np.float32(2.0 ** -30)
    imgs = make_images(2, 100, 180, seed=4)
    dev, ref = _heads_of(p, w, imgs, "bf16", 7), _heads_of(p, w, imgs, "bf16x3", 7)
    tin = [i for i, o in enumerate(dev["ops"]) if o["kind"] == UDA_OP_SEP and o["drop_site2"] >= 0 and not o["fuse_in"]]
    assert len(tin) == 10, tin            # class and box layer 1, five levels each
    assert all(dev["schemes"][i] == UDA_SPLIT_BF16X1 for i in tin) and dev["demotions"] == 0
    assert all(np.isfinite(x).all() for x in dev["det"][:3])
    errs = [_rel_rms(g, r) for g, r in zip(dev["heads"][0] + dev["heads"][1], ref["heads"][0] + ref["heads"][1])]
    print("[bf16 deferred-input sep x 2^30 vs bf16x3] relative rms per level: %s" % " ".join("%.2e" % e for e in errs))
    assert max(errs) <= HEAD_RMS["d2"], errs


# ---------------------------------------------------------------- neighbours untouched
ORDER_WORKER = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import numpy as np
from common import FULL_MC, make_images, make_params, make_weights
from uda_amd.infer_lib import KerasDriver
p = make_params(**FULL_MC)
w = make_weights(p, seed=21)
imgs = make_images(2, 100, 180, seed=22)
d = KerasDriver("_", False, p["name"], 2, False, dict(p, uda_pw_scheme="f16x2"), weights=w)
assert d.pw_scheme == "f16x2"
d.set_dropout_seed(4)
if sys.argv[2] == "beside_bf16":
    other = KerasDriver("_", False, p["name"], 2, False, dict(p, uda_pw_scheme="bf16"), weights=w)
    assert other.pw_scheme == "bf16" and d.pw_scheme == "f16x2"
    other.set_dropout_seed(4)
    for _ in range(2):
        d.serve(imgs)
        other.serve(imgs)
det = d.serve(imgs)
cls, box = d.head_outputs(2)
d.close()
if sys.argv[2] == "beside_bf16":
    other.close()
np.savez(sys.argv[1], *(list(det) + list(cls) + list(box)))
print("saved")
"""


def test_f16x2_handle_beside_a_bf16_handle_is_unchanged(tmp_path):
    """An f16x2 handle that lives beside a bf16 handle, served alternately with it, computes bit for bit what an f16x2 handle
    served alone in a fresh process computes."""
    outs = []
    for tag in ("alone", "beside_bf16"):
        out = str(tmp_path / (tag + ".npz"))
        e = dict(os.environ)
        e.pop("UDA_PW_SCHEME", None)
        e.pop("UDA_PW_TERMS", None)
        r = subprocess.run([sys.executable, "-c", ORDER_WORKER % {"root": ROOT}, out, tag], cwd=ROOT, env=e,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "saved" in r.stdout, (tag, r.stdout[-1500:], r.stderr[-2500:])
        outs.append(np.load(out))
    assert len(outs[0].files) == len(outs[1].files) > 5
    for k in outs[0].files:
        np.testing.assert_array_equal(outs[0][k], outs[1][k], err_msg=k)
