"""The piece model of the split-precision schemes (oracle/split_ref.py) on the CPU: what each scheme's pieces hold,
rounding ties, fp16's subnormal and overflow ends, bf16 against torch's cast, and the contraction bound - that it holds for
a float32 accumulator and that it is tight enough to tell a wrong rounding point from the right one."""
import numpy as np
import pytest

from oracle import split_ref as S

RNG = np.random.default_rng(20261016)


def _log_uniform(lo, hi, n):
    x = np.exp2(RNG.uniform(lo, hi, n)) * RNG.choice([-1.0, 1.0], n)
    return x.astype(np.float32)


@pytest.mark.parametrize("scheme,rel,lo,hi", [
    (S.F16X1, 2.0 ** -11, -14, 15.9),      # one fp16 piece: normal fp16 numbers
    (S.F16X2, 2.0 ** -22, -3, 15.9),       # two fp16 pieces: the low piece is normal from |x| >= 2^-3 on
    (S.BF16X2, 2.0 ** -17, -100, 100),
    (S.BF16X3, 0.0, -100, 100),            # three bf16 pieces: 24 bits, every normal float32 exactly (below 2^-24)
])
def test_pieces_rebuild_the_operand(scheme, rel, lo, hi):
    x = _log_uniform(lo, hi, 200000)
    p = S.pieces(x, scheme)
    assert len(p) == S.n_pieces(scheme)
    got = np.sum([q.astype(np.float64) for q in p], axis=0)
    err = np.abs(got - x.astype(np.float64)) / np.abs(x.astype(np.float64))
    assert err.max() <= rel, (S.NAMES[scheme], err.max() / rel)
    # every piece is a value of the piece type, and the leading piece is the operand rounded once
    for q in p:
        np.testing.assert_array_equal(S.round_piece(q, scheme), q)
    np.testing.assert_array_equal(p[0], S.round_piece(x, scheme))
    # (the bound is reached: a scheme with one bit more would fail the test above)
    assert err.max() > rel / 4 or rel == 0.0


def test_ties_round_to_even():
    one = np.float32(1.0)
    f16 = S.f16_rne(np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 2049.0, 2051.0], np.float32))
    np.testing.assert_array_equal(f16, np.array([one, 1 + 2.0 ** -9, -one, 2048.0, 2052.0], np.float32))
    bf = S.bf16_rne(np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 257.0, 259.0, 1 + 2.0 ** -8 + 2.0 ** -20], np.float32))
    np.testing.assert_array_equal(bf, np.array([one, 1 + 2.0 ** -6, 256.0, 260.0, 1 + 2.0 ** -7], np.float32))


def test_fp16_subnormals_are_kept_and_overflow_is_infinite():
    sub = np.array([2.0 ** -20, 3 * 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26, -2.0 ** -24], np.float32)
    np.testing.assert_array_equal(S.f16_rne(sub), np.array([2.0 ** -20, 3 * 2.0 ** -24, 0.0, 2.0 ** -24, -2.0 ** -24], np.float32))
    big = np.array([65504.0, 65519.0, 65520.0, 7.0e4, -1.0e6], np.float32)
    np.testing.assert_array_equal(S.f16_rne(big), np.array([65504.0, 65504.0, np.inf, np.inf, -np.inf], np.float32))
    # the pieces of an operand above 65504: infinite leading piece (the kernels raise the range flag instead)
    assert np.isinf(S.pieces(np.array([7.0e4], np.float32), S.F16X2)[0]).all()
    # bf16 keeps float32's exponent range
    assert np.isfinite(S.bf16_rne(np.array([3.0e38], np.float32))).all()


def test_bf16_matches_torch():
    torch = pytest.importorskip("torch")
    x = np.concatenate([_log_uniform(-126, 127, 100000),
                        # exact ties and their neighbours
                        (np.float32(1.0) + np.float32(2.0 ** -8) * RNG.integers(0, 512, 2000)).astype(np.float32),
                        np.array([0.0, -0.0, np.inf, -np.inf, 1e-40, -3e-39], np.float32)])
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    np.testing.assert_array_equal(S.bf16_rne(x), want)


def test_split_weight_scale():
    for mx in (1e-4, 0.3, 1.0, 3.0, 8191.0, 16384.0, 1e6):
        w = np.array([mx, -mx / 3, 0.0], np.float32)
        s = S.split_weight_scale(w)
        assert s == 2.0 ** round(np.log2(s))
        assert 2.0 ** 13 <= abs(mx) * s < 2.0 ** 14, (mx, s)
    assert S.split_weight_scale(np.zeros(4, np.float32)) == 1.0


def _device_like(a, b, scheme):
    """A float32 accumulator that rounds once per matrix instruction (one cross term of one k-step), the products of an
    instruction summed exactly: the arithmetic the bound is written for."""
    pa, pb = S.pieces(a, scheme), S.pieces(b, scheme)
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
    ks = S.K_STEP[scheme]
    for k0 in range(0, a.shape[1], ks):
        sl = slice(k0, k0 + ks)
        for i, j in S.CROSS_TERMS[scheme]:
            acc = (acc.astype(np.float64) + pa[i][:, sl].astype(np.float64) @ pb[j][sl].astype(np.float64)).astype(np.float32)
    return acc


@pytest.mark.parametrize("scheme", [S.NONE, S.F16X1, S.F16X2, S.BF16X2, S.BF16X3])
def test_contraction_bound_holds_and_separates_rounding_models(scheme):
    M, K, N = 96, 200, 40                 # K = 12.5 k-steps: a ragged last step
    a = RNG.normal(0, 1, (M, K)).astype(np.float32)
    b = (RNG.normal(0, 1, (K, N)) / np.sqrt(K) * (S.split_weight_scale(np.ones(1)) if S.is_f16(scheme) else 1.0)).astype(np.float32)
    dev = _device_like(a, b, scheme).astype(np.float64)
    val, bnd = S.contract(a, b, scheme)
    ratio = np.abs(dev - val) / bnd
    assert ratio.max() <= 1.0, ratio.max()
    # a model with the wrong rounding point sits outside the bound on most outputs
    if scheme == S.F16X1:
        wrong, _ = S.contract(a, b, scheme, exact_operands=True)
    elif S.n_pieces(scheme) == 2:
        wrong, _ = S.contract(a, b, scheme, drop_low_a=True)
    else:
        return
    assert (np.abs(dev - wrong) > bnd).mean() > 0.9


def test_pointwise_model_of_the_exact_scheme_is_the_float64_op():
    """Scheme NONE (no operand rounding) reduces `pointwise` to the plain float64 1x1 convolution."""
    x = RNG.normal(0, 1, (2, 33, 24)).astype(np.float32)
    w = RNG.normal(0, 0.2, (24, 40)).astype(np.float32)
    se = RNG.uniform(0.1, 1, (2, 24)).astype(np.float32)
    sc, sh = RNG.uniform(0.5, 1.5, 40), RNG.normal(0, 0.3, 40)
    y, bnd = S.pointwise(x, w, None, sc, sh, se, None, None, 1, True, S.NONE)
    xi = (x * se[:, None, :]).astype(np.float32).astype(np.float64)
    z = (xi @ w.astype(np.float64)) * sc + sh
    np.testing.assert_allclose(y, z / (1 + np.exp(-z)), rtol=1e-12, atol=1e-12)
    assert (bnd > 0).all() and (bnd < 1e-5 * np.abs(y).max()).all()
