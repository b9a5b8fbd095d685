"""Rounding-exact model of the split-precision contractions (numpy, float64), with an elementwise error bound.

The HIP kernels never multiply float32 operands directly: each operand is cut into pieces of a narrower type and only
some cross products of the pieces are summed on the matrix cores (csrc/mfma_common.h, "split schemes").  A float64
reference of the plain operation can only be held to the scheme's own resolution (2^-11 per operand for one fp16 piece),
which hides any bug smaller than that.  This module restates what a scheme computes, rounding for rounding, so that a
kernel can be held to float32 ACCUMULATION error instead:

  * `pieces`: piece p = round-to-nearest-even of what pieces 0..p-1 left over (split_parts / pwb_pack_weights), the
    remainder taken in float32 (exact: the piece is the leading part of the float32 value);
  * `contract`: the cross terms of mfma_terms, in float64 - the device value then differs from it only by the float32
    rounding of the running sums;
  * `pointwise`: uda_debug_pw's 1x1 convolution (pwb_kernel / pws_kernel / pwb_shared_kernel epilogue) on top of it.

Nothing here calls the C packers: a packing bug has to show up as a difference.  Scheme numbers are UDA_SPLIT_* of
csrc/uda_internal.h.

Error bound.  The matrix cores add each instruction's 16-deep products to the float32 accumulator: one rounding of the
running sum per instruction, i.e. `nterms` roundings per 16-deep k-step, each at most u |running sum| (u = 2^-24), plus
whatever the instruction loses while it sums its 16 products (bounded by u sum |a_i b_i| per rounding).  The bound of a
contraction is therefore

    C_BOUND * u * (nterms * sum_s |S_s| + sum_i |a_i b_i|)

with S_s the float64 partial sums after k-step s and the second sum over all products of pieces that are summed.
C_BOUND = 4: one factor of 2 covers the running sum between the instructions of a k-step and across the k-split of the
deep kernels differing from the k-step partial sums S_s; the other covers an accumulator that truncates instead of rounding
(a full ulp, 2u, instead of half of one).  The same value is used everywhere.  Epilogue operations add their own
roundings (a few u of the value) and propagate the bound with absolute-value arithmetic.
"""
import numpy as np

NONE, BF16X2, BF16X3, F16X2, F16X1 = 0, 2, 3, 4, 5
NAMES = {NONE: "f32", BF16X2: "bf16x2", BF16X3: "bf16x3", F16X2: "f16x2", F16X1: "f16"}
# uda_debug_pw's `terms` argument -> scheme
TERMS_SCHEME = {0: NONE, 1: F16X1, 3: BF16X2, 6: BF16X3, 16: F16X2}

U = 2.0 ** -24
C_BOUND = 4.0
F16_MAX = 65504.0

# (A piece, B piece) of every product mfma_terms sums, in its order
CROSS_TERMS = {
    NONE: [(0, 0)],
    F16X1: [(0, 0)],
    BF16X2: [(1, 0), (0, 1), (0, 0)],
    F16X2: [(1, 0), (0, 1), (0, 0)],
    BF16X3: [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)],
}
# depth of one matrix instruction: v_mfma_f32_32x32x16_{bf16,f16} for the split schemes, v_mfma_f32_32x32x2_f32 for NONE
K_STEP = {NONE: 2, F16X1: 16, BF16X2: 16, F16X2: 16, BF16X3: 16}


def n_pieces(scheme):
    return {NONE: 1, F16X1: 1, BF16X2: 2, F16X2: 2, BF16X3: 3}[scheme]


def is_f16(scheme):
    return scheme in (F16X2, F16X1)


def f16_rne(x):
    """float32 -> nearest fp16 (ties to even), back as float32: v_cvt_pk_f16_f32 / f32_to_f16_rne.  Subnormals are kept,
    a value beyond fp16's range becomes inf (numpy's float32 -> float16 conversion is IEEE round-to-nearest-even)."""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def bf16_rne(x):
    """float32 -> nearest bf16 (ties to even) on the bit pattern, back as float32: v_cvt_pk_bf16_f32 / f32_to_bf16_rne.
    NaN stays NaN; a value that rounds past the largest bf16 becomes inf."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    out = r.view(np.float32).copy()
    nan = np.isnan(x)
    out[nan] = x[nan]
    return out


def round_piece(x, scheme):
    if scheme == NONE:
        return np.asarray(x, np.float32)
    return f16_rne(x) if is_f16(scheme) else bf16_rne(x)


def pieces(x, scheme, exact=None):
    """float32 array -> list of n_pieces(scheme) float32 arrays; piece p rounds what pieces 0..p-1 left over, the
    remainder is taken in float32 (split_parts, mfma_common.h; pwb_pack_weights, kernels_pwb.hip).

    exact: the float64 value that `x` is the float32 rounding of (a gated operand x = fl(v * g)).  The kernels write the
    gate product and the first remainder as `r = v * g; ...; r -= piece0`, which the compiler contracts into ONE fused
    multiply-add, v_fma_f32(v, g, -piece0) (as the ISA of pwb_shared_kernel shows; test_gpu_ops holds the 1x1 kernels to it): the leading piece
    rounds the float32 product, the remainder is the EXACT product minus that piece, rounded once."""
    r = np.asarray(x, np.float32)
    out = []
    for p in range(n_pieces(scheme)):
        q = round_piece(r, scheme)
        out.append(q)
        if p + 1 < n_pieces(scheme):
            with np.errstate(invalid="ignore"):
                if p == 0 and exact is not None:
                    r = (np.asarray(exact, np.float64) - q).astype(np.float32)
                else:
                    r = (r - q).astype(np.float32)
    return out


def split_weight_scale(w):
    """split_weight_scale (kernels_pwb.hip): the power of two that puts max|w| into [2^13, 2^14); 1 for an all-zero or
    non-finite kernel."""
    mx = float(np.abs(np.asarray(w, np.float32)).max()) if np.size(w) else 0.0
    if not (mx > 0.0) or not (mx < 3.0e38):
        return 1.0
    _, e = np.frexp(np.float32(mx))
    return float(np.ldexp(1.0, 14 - int(e)))


def contract(a, b, scheme, exact_operands=False, drop_low_a=False, a_exact=None):
    """sum_k a[m, k] b[k, n] as scheme `scheme` computes it: float32 operands a [M, K] and b [K, N] (b already times its
    weight scale) are split into pieces and the cross terms of mfma_terms are summed in float64.  Returns (value, bound):
    the device's float32 accumulator differs from `value` by at most `bound` (see the module docstring).

    exact_operands: no operand rounding (the float64 product of the float32 operands) - a model the bound must reject
    for the one-piece scheme.  drop_low_a: the low A piece left out (two-piece schemes) - one the bound must reject.
    a_exact: float64 [M, K], the exact value `a` is the float32 rounding of (a gated operand, see `pieces`)."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    M, K = a.shape
    N = b.shape[1]
    if exact_operands:
        pa, pb, terms = [a], [b], [(0, 0)]
    else:
        pa, pb, terms = pieces(a, scheme, a_exact), pieces(b, scheme), CROSS_TERMS[scheme]
        if drop_low_a:
            terms = [(i, j) for i, j in terms if i == 0]
    pa = [p.astype(np.float64) for p in pa]
    pb = [p.astype(np.float64) for p in pb]
    ks = K_STEP[scheme]
    value = np.zeros((M, N))
    run_abs = np.zeros((M, N))         # sum over k-steps of |partial sum|
    prod_abs = np.zeros((M, N))        # sum of |a_i b_j| over every product that is summed
    for k0 in range(0, K, ks):
        sl = slice(k0, min(K, k0 + ks))
        for i, j in terms:
            value += pa[i][:, sl] @ pb[j][sl]
            prod_abs += np.abs(pa[i][:, sl]) @ np.abs(pb[j][sl])
        run_abs += np.abs(value)
    bound = C_BOUND * U * (len(CROSS_TERMS[scheme]) * run_abs + prod_abs)
    return value, bound


def pointwise(x, w, bias, sc, sh, se, mask, res, in_div, act, scheme, exact_operands=False, drop_low_a=False):
    """uda_debug_pw's 1x1 convolution under `scheme`: (value, bound), both float64 [rows, hw, cout].

    A operand: float32(x * se), its remainders from the exact product (the gate multiplies before the split:
    pwb_kernel's store_chunk, contracted with the first remainder - see `pieces`).  B operand:
    float32(w * split_weight_scale(w)) for fp16 pieces (uda_debug_pw / uda_create), w otherwise.  Epilogue
    (pwb_kernel / pws_kernel): v = fma(acc, 1/scale, bias); v = fma(v, bn_scale, bn_shift); swish; * mask; + res."""
    x = np.asarray(x, np.float32)
    w = np.asarray(w, np.float32)
    rows_in, hw, cin = x.shape
    rows = rows_in * in_div
    a, a_exact = x, None
    if se is not None:
        a_exact = x.astype(np.float64) * np.asarray(se, np.float32).astype(np.float64)[:, None, :]    # (exact: 24 + 24 bits)
        a = a_exact.astype(np.float32)
    scale = split_weight_scale(w) if is_f16(scheme) else 1.0
    bw = (w * np.float32(scale)).astype(np.float32)
    acc, bnd = contract(a.reshape(rows_in * hw, cin), bw, scheme, exact_operands, drop_low_a,
                        None if a_exact is None else a_exact.reshape(rows_in * hw, cin))
    acc = np.repeat(acc.reshape(rows_in, hw, -1), in_div, axis=0) / scale
    bnd = np.repeat(bnd.reshape(rows_in, hw, -1), in_div, axis=0) / scale
    y = acc + (0.0 if bias is None else np.asarray(bias, np.float64))
    bnd = bnd + U * np.abs(y)                                    # fma(acc, un, bias): one rounding
    if sc is not None:
        sc64 = np.asarray(sc, np.float64)
        y = y * sc64 + np.asarray(sh, np.float64)
        bnd = bnd * np.abs(sc64) + U * np.abs(y)
    if act:
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
