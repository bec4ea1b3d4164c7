"""A numpy restatement of the three OpenCV calls the reference's defor_2D makes (datasets/data_augmentation.py:319-342), as the
fixture recorder's ``cv2`` stand-in and the tests' oracle.  OpenCV is not installed: this restates its documented behaviour and is
pinned against scipy.ndimage (tests/test_defor_cpu.py), not against OpenCV itself.

  * getStructuringElement(MORPH_ELLIPSE, (w, h)): OpenCV's ellipse rows (imgproc/src/morph.dispatch.cpp); (2, 2) -> [[0,1],[1,1]].
  * erode / dilate(src, kernel, dst=None, anchor=(-1,-1), iterations=1): min / max of src(y + i - ay, x + j - ax) over the
    element's non-zero (i, j), anchor (-1,-1) = (w // 2, h // 2); the element is not reflected; the default border
    (BORDER_CONSTANT with morphologyDefaultBorderValue) makes neighbours outside the image not count.  The reference passes
    rand_r as the third positional argument, which is ``dst``: accepted and ignored here, as OpenCV's binding overwrites it.
"""
import math

import numpy as np

MORPH_RECT, MORPH_CROSS, MORPH_ELLIPSE = 0, 1, 2


def getStructuringElement(shape, ksize, anchor=(-1, -1)):
    w, h = ksize
    el = np.zeros((h, w), np.uint8)
    if shape == MORPH_RECT:
        el[:] = 1
        return el
    r, c = h // 2, w // 2
    inv_r2 = 1.0 / (r * r) if r else 0.0
    for i in range(h):
        dy = i - r
        if shape == MORPH_CROSS:
            j1, j2 = (0, w) if dy == 0 else (c, c + 1)
        elif abs(dy) <= r:
            dx = int(round(c * math.sqrt((r * r - dy * dy) * inv_r2)))       # cvRound; no .5 ties for the sizes used here
            j1, j2 = max(c - dx, 0), min(c + dx + 1, w)
        else:
            j1 = j2 = 0
        el[i, j1:j2] = 1
    return el


def _morph(src, kernel, anchor, reduce_, iterations):
    src = np.asarray(src)
    kernel = np.asarray(kernel)
    h, w = kernel.shape
    ax, ay = anchor
    ax, ay = (w // 2 if ax < 0 else ax), (h // 2 if ay < 0 else ay)
    out = src.copy()
    for _ in range(iterations):
        cur, acc = out, None
        H, W = cur.shape[:2]
        for i in range(h):
            for j in range(w):
                if not kernel[i, j]:
                    continue
                dy, dx = i - ay, j - ax
                # shifted view: value src(y + dy, x + dx); outside the image -> the identity of the reduction (does not count)
                fill = np.inf if reduce_ is np.minimum else -np.inf
                sh = np.full(cur.shape, fill, dtype=np.float64)
                ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
                xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
                sh[yd, xd] = cur[ys, xs]
                acc = sh if acc is None else reduce_(acc, sh)
        out = acc.astype(src.dtype)
    return out


def erode(src, kernel, dst=None, anchor=(-1, -1), iterations=1):
    return _morph(src, kernel, anchor, np.minimum, iterations)


def dilate(src, kernel, dst=None, anchor=(-1, -1), iterations=1):
    return _morph(src, kernel, anchor, np.maximum, iterations)


def band(mask):
    """defor_2D's band: erode != dilate of the 2x2 ellipse (the pixel differs from its up or left neighbour inside the image)"""
    k = getStructuringElement(MORPH_ELLIPSE, (2, 2))
    return erode(mask, k) != dilate(mask, k)


def defor_mask(mask, drop_ranks):
    """defor_2D's result for a given choice of band ranks to drop (data_augmentation.py:335-341)"""
    out = np.array(mask, dtype=np.float32, copy=True)
    b = band(out)
    ch = np.ones(int(b.sum()), np.float32)
    ch[np.asarray(drop_ranks, dtype=np.int64)] = 0.0
    out[b] = ch
    out[out > 0.0] = 1.0
    return out
