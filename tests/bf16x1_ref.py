"""Rounding-exact model of the one-piece bf16 scheme (UDA_SPLIT_BF16X1 = 6, `uda_pw_scheme = "bf16"`), in the manner of
oracle/split_ref.py, whose helpers, constants and bound derivation it uses (that module enumerates the schemes in dicts
and does not know code 6).

What the scheme computes (csrc/mfma_common.h): every operand is ONE bf16 piece, the round-to-nearest-even of its float32
value (`pack_piece`'s bf16 case, v_cvt_pk_bf16_f32; weights: f32_to_bf16_rne on the host); one
v_mfma_f32_32x32x16_bf16 per 16-deep k-step into a float32 accumulator.  Weight scale 1 (bf16 has float32's exponent
range: nothing to pre-scale, nothing to track).  A gated operand is bf16_rne(float32(x * se)): the gate multiplies in
float32 and the product is rounded once into the operand - with one piece there is no remainder for the compiler to
contract the multiplication into.

Error bound: split_ref's, with ONE cross term per k-step:

    C_BOUND * U * (sum over 16-deep k-steps of |partial sum| + sum |a_i b_i|)

i.e. float32 ACCUMULATION error only (about 2^-24 of the summed magnitudes); the 2^-9 relative operand rounding is part
of the model, not of the bound.
"""
import numpy as np

import common  # noqa: F401  (puts the repository root on sys.path)
from oracle import split_ref as S

BF16X1 = 6
TERMS = 8              # uda_debug_pw's `terms` code of the scheme
K_STEP = 16            # depth of v_mfma_f32_32x32x16_bf16
U, C_BOUND = S.U, S.C_BOUND


def contract(a, b, exact_operands=False):
    """sum_k a[m, k] b[k, n] as the scheme computes it: (value, bound), float64 [M, N].  exact_operands: no operand
    rounding (the float64 product of the float32 operands) - a model the bound must reject."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    pa = (a if exact_operands else S.bf16_rne(a)).astype(np.float64)
    pb = (b if exact_operands else S.bf16_rne(b)).astype(np.float64)
    M, K = a.shape
    N = b.shape[1]
    value, run_abs, prod_abs = np.zeros((M, N)), np.zeros((M, N)), np.zeros((M, N))
    for k0 in range(0, K, K_STEP):
        sl = slice(k0, min(K, k0 + K_STEP))
        value += pa[:, sl] @ pb[sl]
        prod_abs += np.abs(pa[:, sl]) @ np.abs(pb[sl])
        run_abs += np.abs(value)
    return value, C_BOUND * U * (run_abs + prod_abs)


def pointwise(x, w, bias, sc, sh, se, mask, res, in_div, act, scheme=BF16X1, exact_operands=False, drop_low_a=False):
    """uda_debug_pw's 1x1 convolution under the scheme: (value, bound), both float64 [rows, hw, cout] - the signature and
    the epilogue bound propagation of split_ref.pointwise (pwb_kernel / pws_kernel: v = fma(acc, 1, bias);
    v = fma(v, bn_scale, bn_shift); swish; * mask; + res)."""
    assert scheme == BF16X1 and not drop_low_a          # (one piece: there is no low piece to drop)
    x = np.asarray(x, np.float32)
    w = np.asarray(w, np.float32)
    rows_in, hw, cin = x.shape
    rows = rows_in * in_div
    a = x
    if se is not None:
        with np.errstate(over="ignore"):
            a = (x.astype(np.float64) * np.asarray(se, np.float32).astype(np.float64)[:, None, :]).astype(np.float32)
    acc, bnd = contract(a.reshape(rows_in * hw, cin), w, exact_operands)
    acc = np.repeat(acc.reshape(rows_in, hw, -1), in_div, axis=0)
    bnd = np.repeat(bnd.reshape(rows_in, hw, -1), in_div, axis=0)
    y = acc + (0.0 if bias is None else np.asarray(bias, np.float64))
    bnd = bnd + U * np.abs(y)                                    # fma(acc, un, bias): one rounding
    if sc is not None:
        sc64 = np.asarray(sc, np.float64)
        y = y * sc64 + np.asarray(sh, np.float64)
        bnd = bnd * np.abs(sc64) + U * np.abs(y)
    if act:
        with np.errstate(over="ignore"):
            s = 1.0 / (1.0 + np.exp(-y))
        y = y * s
        # |d swish / dx| <= 1.1; __expf / v_rcp_f32 / the products: a few float32 ulps of the result (8 u)
        bnd = 1.1 * bnd + 8.0 * U * np.abs(y)
    if mask is not None:
        m = np.asarray(mask, np.float64)[:, None, :]
        y = y * m
        bnd = bnd * np.abs(m) + U * np.abs(y)
    if res is not None:
        y = y + np.asarray(res, np.float64)
        bnd = bnd + U * np.abs(y)
    assert y.shape[0] == rows
    return y, bnd
