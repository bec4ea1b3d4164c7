"""The frames of the segmentation tests, built with fixed RandomStates.  The small frames are 37 x 53 like plane_cases.small_frames:
neither side is a multiple of the kernel's 32 x 16 tile (csrc/segment.hip TW, TH), so every one has partial tiles, two tiles across
and three down.  ``cases()`` is the whole set: (name, depth (H,W) uint16, max_step)."""
import functools

import numpy as np

from tests import plane_cases as pc
from tests import plane_ref

SH, SW = pc.SH, pc.SW
TILE_W, TILE_H = 32, 16
STEP, MIN_PIXELS = 10, 50          # the rule for table scenes: pose.Segmenter's defaults


def serpentine(H, W, z=800):
    """a one-pixel-wide path through the whole frame: the even rows, joined at alternating ends by one pixel of the odd rows.  One
    component whose root (0, 0) is one end and whose last pixel in path order is the other"""
    d = np.zeros((H, W), np.uint16)
    d[0::2] = z
    for k, y in enumerate(range(1, H - (H % 2 == 0), 2)):
        d[y, W - 1 if k % 2 == 0 else 0] = z
    if H % 2 == 0:
        d[H - 1] = 0
    return d


def checkerboard(H, W, z=900):
    ys, xs = np.mgrid[0:H, 0:W]
    return np.where((ys + xs) % 2 == 0, z, 0).astype(np.uint16)


def step_columns(H, W, step=STEP):
    """columns of constant depth: neighbours differ by exactly ``step`` (joined) or ``step + 1`` (not), by turns of three; the last
    four columns hold 1 | 65535 | 65535 - step | 65535 - 2 step - 1: 1 and 65535 are 65534 apart and must not be joined by
    arithmetic that wraps at 16 bits (there they would be 2 apart)"""
    cols, z = [], 500
    for x in range(W - 4):
        cols.append(z)
        z += step + 1 if x % 3 == 2 else step
    cols += [1, 65535, 65535 - step, 65535 - 2 * step - 1]
    return np.tile(np.asarray(cols, np.uint16), (H, 1))


def combs(H, W):
    """left: a comb -- teeth in every other column that meet only in the last row; right: nested U shapes, each one's arms meeting only
    in its bottom row, a pixel's gap and 30 mm between one U and the next"""
    d = np.zeros((H, W), np.uint16)
    d[:H - 1, 0:21:2] = 700
    d[H - 1, 0:21] = 700
    for k in range(6):
        xl, xr, yb, z = 24 + 2 * k, W - 1 - 2 * k, H - 1 - 2 * k, 900 + 30 * k
        d[:yb + 1, xl] = z
        d[:yb + 1, xr] = z
        d[yb, xl:xr + 1] = z
    return d


def blobs(H, W, r, n=6):
    """random discs at bases 40 mm apart with 8 % holes and +-3 mm noise (a later disc covers an earlier one)"""
    ys, xs = np.mgrid[0:H, 0:W]
    d = np.zeros((H, W), np.float64)
    for k in range(n):
        cy, cx, rad = r.uniform(0, H), r.uniform(0, W), r.uniform(4, min(H, W) / 3.0)
        inside = (ys - cy) ** 2 + (xs - cx) ** 2 < rad ** 2
        d[inside] = 600 + 40 * k + r.randint(-3, 4, int(inside.sum()))
    d[r.rand(H, W) < 0.08] = 0
    return d.astype(np.uint16)


def many_tiles():
    """41 rows x 75 columns = 3 tiles down (16 + 16 + 9) and 3 across (32 + 32 + 11), a multiple of the tile in neither: blobs, and in
    the first 21 columns a vertical serpentine (the even columns, joined at alternating ends) that crosses every tile row"""
    H, W = 2 * TILE_H + 9, 2 * TILE_W + 11
    d = blobs(H, W, np.random.RandomState(11), n=9)
    d[:, :22] = 0
    d[:, :21] = serpentine(21, H, z=1200).T
    return d


def small_cases():
    """the seven 37 x 53 frames, in order: (name, depth, max_step)"""
    r = np.random.RandomState(3)
    return [("serpentine", serpentine(SH, SW), STEP), ("invalid", np.zeros((SH, SW), np.uint16), STEP),
            ("one_depth", np.full((SH, SW), 1000, np.uint16), STEP), ("checkerboard", checkerboard(SH, SW), STEP),
            ("step_columns", step_columns(SH, SW), STEP), ("combs", combs(SH, SW), STEP), ("blobs", blobs(SH, SW, r), STEP)]


@functools.lru_cache(maxsize=None)
def cut_frame(k):
    """frame k of plane_cases with its plane fitted and cut by tests/plane_ref.py, as the tracking tests see it"""
    ft = pc.fitted(k)
    assert ft["info"][0] == 0
    return plane_ref.cut(pc.rendered(k), ft["plane"], 0, pc.CAMK, pc.MARGIN)[0]


@functools.lru_cache(maxsize=None)
def cases():
    """small_cases, many_tiles, the six cut frames, and cut frame 4 again with a 4 mm step (213 components over 150 tiles)"""
    return tuple(small_cases() + [("many_tiles", many_tiles(), STEP)] + [("cut%d" % k, cut_frame(k), STEP) for k in range(pc.FRAMES)]
                 + [("fragmented", cut_frame(4), 4)])
