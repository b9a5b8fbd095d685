"""numpy restatement of the consistency check (`consistency_ssl`, reference infer_model.py:768-848, utils_box.py:56-89)
that `ServingDriver.serve_consistency` computes on the device: the fixed-point 9x9 Gaussian blur of the blur variant, the
un-flip of the flip variant's boxes, calc_iou_np, and the cons_iou / cons_cls columns.  Shared by
test_consistency_host.py (CPU) and test_gpu_consistency.py."""
import math

import numpy as np

BLUR_TAPS = (4, 13, 30, 51, 60, 51, 30, 13, 4)      # csrc/kernels_post.hip blur_tap
NOISE_TAG = 0x4E                                   # Philox stream of the noise variant (kernels_post.hip raw_px)


def fixed_point_taps(n=9, sigma=0.0, frac_bits=8):
    """OpenCV's 8-bit Gaussian taps (getGaussianKernelBitExact + getGaussianKernelFixedPoint_ED): sigma <= 0 means
    0.15 n + 0.35 (= 0.3 ((n - 1) / 2 - 1) + 0.8); the normalised taps times 2^frac_bits, rounded from the outside in with
    the rounding error carried to the next tap, the centre tap takes the rest."""
    sig = sigma if sigma > 0 else n * 0.15 + 0.35
    scale2 = -0.125 / (sig * sig)
    half = (n - 1) // 2
    vals = [math.exp(float(x * x) * scale2) for x in range(1 - n, 0, 2)]
    total = 2.0 * sum(vals) + 1.0
    one = 1 << frac_bits
    out, err = [], 0.0
    for v in vals:
        adj = v / total * one + err
        r = int(round(adj))
        err = adj - r
        out.append(r)
    centre = one - 2 * sum(out)
    assert len(out) == half
    return tuple(out + [centre] + out[::-1])


def reflect101(p, n):
    """cv::borderInterpolate for BORDER_REFLECT_101 (BORDER_DEFAULT), iterated for coordinates more than n away."""
    if n == 1:
        return 0
    while not 0 <= p < n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def blur_u8(im):
    """cv2.GaussianBlur(im, (9, 9), 0) as the device computes it: rows r = sum c p, columns s = sum c r, (s + 32768) >> 16."""
    im = np.asarray(im)
    h, w = im.shape[:2]
    ys = np.array([reflect101(y, h) for y in range(-4, h + 4)])
    xs = np.array([reflect101(x, w) for x in range(-4, w + 4)])
    pad = im[ys][:, xs].astype(np.int64)
    r = sum(c * pad[:, i:i + w] for i, c in enumerate(BLUR_TAPS))
    s = sum(c * r[j:j + h] for j, c in enumerate(BLUR_TAPS))
    return ((s + 32768) >> 16).astype(np.uint8)


def unflip(boxes, width):
    """[y1, x1, y2, x2] of the flipped image -> [y1, W - x2, y2, W - x1] (infer_model.py:818-822), float32."""
    b = np.asarray(boxes, np.float32)[..., :4]
    w = np.float32(width)
    return np.stack([b[..., 0], w - b[..., 3], b[..., 2], w - b[..., 1]], -1).astype(np.float32)


def calc_iou_np(gt_boxes, pred_boxes):
    """utils_box.calc_iou_np: float32 coordinate differences, float64 products, 0 where the union is 0."""
    gt = np.asarray(gt_boxes, np.float32)
    pr = np.asarray(pred_boxes, np.float32)
    yA = np.maximum(gt[:, 0], pr[:, 0])
    xA = np.maximum(gt[:, 1], pr[:, 1])
    yB = np.minimum(gt[:, 2], pr[:, 2])
    xB = np.minimum(gt[:, 3], pr[:, 3])
    inter = np.maximum(np.float32(0), xB - xA).astype(np.float64) * np.maximum(np.float32(0), yB - yA).astype(np.float64)
    area_a = np.abs(gt[:, 3] - gt[:, 1]).astype(np.float64) * np.abs(gt[:, 2] - gt[:, 0]).astype(np.float64)
    area_b = np.abs(pr[:, 3] - pr[:, 1]).astype(np.float64) * np.abs(pr[:, 2] - pr[:, 0]).astype(np.float64)
    union = (area_a + area_b) - inter
    return np.divide(inter, union, out=np.zeros_like(inter), where=union != 0)


def consistency_scores(boxes, variants, widths):
    """boxes [N, M, >=4] of the originals; variants: ((boxes, classes) of flip, blur, noise), boxes [N, M, >=4], classes
    [N, M] (column 0 of an MC class output); widths [N] raw widths.  -> (cons_iou [N, M] float64, cons_cls [N, M] bool)."""
    boxes = np.asarray(boxes, np.float32)
    N, M = boxes.shape[:2]
    iou = np.zeros((N, M), np.float64)
    agree = np.zeros((N, M), bool)
    for i in range(N):
        best = []
        for v, (vb, _) in enumerate(variants):
            vb = np.asarray(vb, np.float32)[i, :, :4]
            if v == 0:
                vb = unflip(vb, widths[i])
            best.append(np.array([calc_iou_np(boxes[i, k:k + 1, :4], vb).max() for k in range(M)]))
        iou[i] = ((best[0] + best[1]) + best[2]) / 3.0
        cls = [np.asarray(vc, np.float32)[i] for _, vc in variants]
        mean = np.mean(np.stack(cls, -1), axis=-1)          # float32, as the reference's np.mean of float32 classes
        agree[i] = [bool(float(m).is_integer()) for m in mean]
    return iou, agree


def noisy_images(images, seed, image0=0):
    """uint8 images -> float64 im + sqrt(0.5) philox_normal(seed, raw pixel, image, channel, NOISE_TAG)."""
    from oracle import philox_ref
    out = []
    for n, im in enumerate(images):
        im = np.asarray(im)
        h, w = im.shape[:2]
        px = np.repeat(np.arange(h * w, dtype=np.uint32), 3)
        ch = np.tile(np.arange(3, dtype=np.uint32), h * w)
        img = np.full(px.shape, image0 + n, np.uint32)
        z, _ = philox_ref.normal2(seed, px, img, ch, NOISE_TAG)
        out.append(im.astype(np.float64) + np.sqrt(0.5) * z.reshape(h, w, 3))
    return out
