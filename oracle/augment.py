"""numpy restatement of the reference's per-image augmentation arithmetic - TEST INFRASTRUCTURE (see oracle/__init__.py).

The reference calls OpenCV (cv2.warpAffine / cv2.resize, utils.py:16-36) from data/batch_provider.py:196-266.  OpenCV is not
in this image (and is an un-vendored dependency of the reference), so its published resampling rules are restated here and
PARITY WITH cv2 IS UNPINNED (OpenCV's fixed-point coordinate tables are not modelled):
  warpAffine(src, getRotationMatrix2D((W/2, H/2), angle, 1), INTER_LINEAR, BORDER_CONSTANT 0): dst(x, y) = bilinear src at M^-1 (x, y)
  resize(src, (W, H), INTER_LINEAR): source coordinate (o + 0.5) * scale - 0.5, taps clamped to the image
  *_as_onehot: one-hot channels through the same resampling, then argmax (first maximum).

`dtype` is the type of every coordinate, weight and sum: float32 (the default) is the arithmetic of csrc/augment.hip, float64 the
reference the kernel is gated against.  With float64 `augment` also returns the MARGIN of every output label: the top one-hot
weight minus the runner-up at the stage that decided it (+inf where nothing was resampled, or with a single label), minimised,
where the resize reads rotated labels, over the rotate-stage margins of the taps it reads with a non-zero weight.  Where every
tap of a rotated pixel lies outside the image all weights are exactly 0 and label 0 wins in any precision; top minus runner-up
is 0 - 0 there, so the margin is instead how far the source coordinate is from the nearest position at which a tap enters the
image (a weight can only appear by moving the coordinate that far).  A label whose margin is far above the fp32 rounding of a
weight (~ 1e-5 at these sizes) is the same in any precision; below it the argmax is decided by rounding.

`defects` names deliberate mistakes ("centre": H and W swapped in the rotation centre, "scale": r / W on both axes, "argmax":
last maximum); tests/test_aux_cases_cpu.py uses them to show that its cases would catch a kernel that made them."""
import numpy as np


def _taps_zero(img, sx, sy, T):
    H, W = img.shape
    x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
    fx, fy = (sx - x0).astype(T), (sy - y0).astype(T)

    def at(x, y):
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        return np.where(ok, img[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], 0).astype(T)
    return ((1 - fy) * ((1 - fx) * at(x0, y0) + fx * at(x0 + 1, y0)) + fy * ((1 - fx) * at(x0, y0 + 1) + fx * at(x0 + 1, y0 + 1))).astype(T)


def _bilinear_zero(img, sx, sy):
    return _taps_zero(img, sx, sy, np.float32)


def _rot_coords(shape, c, s, T, defects=()):
    H, W = shape
    yy, xx = np.mgrid[0:H, 0:W].astype(T)
    cx, cy = (T(H * 0.5), T(W * 0.5)) if "centre" in defects else (T(W * 0.5), T(H * 0.5))
    dx, dy = xx - cx, yy - cy
    return T(c) * dx - T(s) * dy + cx, T(s) * dx + T(c) * dy + cy


def rotate_image(img, c, s, dtype=np.float32, defects=()):
    sx, sy = _rot_coords(img.shape, c, s, dtype, defects)
    return _taps_zero(img.astype(dtype), sx, sy, dtype)


def _resize_taps(h, w, size, T, defects=()):
    H, W = size
    fy = ((np.arange(H, dtype=T) + T(0.5)) * T(T(h) / T(W if "scale" in defects else H)) - T(0.5))
    fx = ((np.arange(W, dtype=T) + T(0.5)) * T(T(w) / T(W)) - T(0.5))
    y0, x0 = np.floor(fy).astype(int), np.floor(fx).astype(int)
    wy, wx = (fy - y0).astype(T), (fx - x0).astype(T)
    wy[y0 < 0], wx[x0 < 0] = 0, 0
    y0, x0 = np.clip(y0, 0, h - 1), np.clip(x0, 0, w - 1)
    y1, x1 = np.clip(y0 + 1, 0, h - 1), np.clip(x0 + 1, 0, w - 1)
    return y0, y1, x0, x1, wy, wx


def resize_image(img, size, dtype=np.float32, defects=()):
    h, w = img.shape
    y0, y1, x0, x1, wy, wx = _resize_taps(h, w, size, dtype, defects)
    a = img.astype(dtype)
    top = (1 - wx)[None, :] * a[y0][:, x0] + wx[None, :] * a[y0][:, x1]
    bot = (1 - wx)[None, :] * a[y1][:, x0] + wx[None, :] * a[y1][:, x1]
    return ((1 - wy)[:, None] * top + wy[:, None] * bot).astype(dtype)


def _onehot(lbl, nlabels, dtype=np.float32):
    return [(lbl == k).astype(dtype) for k in range(nlabels)]


def _argmax(stack, defects=()):
    """First maximum over the last axis (np.argmax), and top minus runner-up (+inf with a single channel)."""
    n = stack.shape[-1]
    lbl = n - 1 - np.argmax(stack[..., ::-1], axis=-1) if "argmax" in defects else np.argmax(stack, axis=-1)
    if n == 1:
        return lbl, np.full(lbl.shape, np.inf)
    top2 = np.sort(stack, axis=-1)[..., -2:]
    return lbl, (top2[..., 1] - top2[..., 0]).astype(np.float64)


def augment(img, lbl, prm, nlabels, dtype=np.float32, defects=()):
    """One image / label pair through batch_provider.py:186-266 with the parameter row `prm` of draw_augmentation.
    Returns (image, label); with dtype=np.float64 (image, label, margin)."""
    T = dtype
    do_rot, c, s, do_scale, p_x, p_y, r, flips = [float(v) for v in prm]
    img, lbl = img.astype(T), lbl.astype(np.int64)
    margin = np.full(lbl.shape, np.inf)
    if do_rot:
        H, W = img.shape
        img = rotate_image(img, c, s, T, defects)
        lbl, margin = _argmax(np.stack([rotate_image(ch, c, s, T, defects) for ch in _onehot(lbl, nlabels, T)], -1), defects)
        sx, sy = _rot_coords((H, W), c, s, np.float64, defects)
        away = np.maximum(np.maximum(-1 - sx, sx - W), np.maximum(-1 - sy, sy - H))     # > 0: every tap is outside the image
        margin = np.where(away >= 0, np.inf if nlabels == 1 else away, margin)
    if do_scale:
        p_x, p_y, r = int(p_x), int(p_y), int(r)
        n_x, n_y = img.shape
        img = resize_image(img[p_y:p_y + r, p_x:p_x + r], (n_x, n_y), T, defects)
        y0, y1, x0, x1, wy, wx = _resize_taps(r, r, (n_x, n_y), np.float64, defects)
        m = margin[p_y:p_y + r, p_x:p_x + r]
        lbl, margin = _argmax(np.stack([resize_image(ch[p_y:p_y + r, p_x:p_x + r], (n_x, n_y), T, defects) for ch in _onehot(lbl, nlabels, T)], -1),
                              defects)
        for ys, wys in ((y0, 1 - wy), (y1, wy)):
            for xs, wxs in ((x0, 1 - wx), (x1, wx)):
                margin = np.minimum(margin, np.where(wys[:, None] * wxs[None, :] > 0, m[ys][:, xs], np.inf))
    if int(flips) & 1:
        img, lbl, margin = np.fliplr(img), np.fliplr(lbl), np.fliplr(margin)
    if int(flips) & 2:
        img, lbl, margin = np.flipud(img), np.flipud(lbl), np.flipud(margin)
    return (img, lbl, margin) if T is np.float64 else (img, lbl)
