"""The ball crop on the GPU (csrc/ballcrop.hip through ops.ball_cloud / ball_cloud_pts / ball_select / ball_sample) against the
NumPy restatement of its contract (tests/ball_ref.py) with torch.equal on records, counts, points and pixels; the rectangle against
the whole-frame scan; the points against the ROI path's; the compatibility functions of network.point_sample.pc_sample_sphere against
what the reference returned (tests/golden/ball_crop_ref.npz).  Frames are 96 x 128 unless stated; every case is one or two launches."""
import numpy as np
import pytest
import torch

from tests import ball_ref as br
from tests.test_ball_crop_cpu import NUM, fixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
CAMK = (118.2, 117.9, 64.5, 48.8)
BIG = np.full(br.LEVELS, 1e9, F)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")


def make_frame(seed, H=96, W=128, holes=0.05):
    """a tilted table with an object in front of it, holes (depth 0) and one saturated pixel"""
    r = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    dep = 900.0 + 1.5 * ys * (96.0 / H) + r.rand(H, W) * 3.0
    cx, cy, rad = 0.55 * W, 0.45 * H, 0.2 * H
    rr = (xs - cx) ** 2 + (ys - cy) ** 2
    obj = rr < rad ** 2
    dep[obj] = 600.0 - np.sqrt(rad ** 2 - rr[obj]) * (120.0 / rad) + r.rand(int(obj.sum())) * 2.0
    if holes:
        dep[r.rand(H, W) < holes] = 0
        dep[1, 2] = 65535
    return dep.astype(np.uint16), obj


def dev_t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def gpu_crop(depth, jobs, cap=None, full_scan=False, masks=None, camk=CAMK):
    """depth (I,H,W) uint16; jobs: list of (img, centre, ladder[, mask_off, mask_stride, mask_val]); masks: flat uint8 array"""
    from tgpose_amd import ops
    I = depth.shape[0]
    kw = {}
    if masks is not None:
        kw = dict(masks=dev_t(masks), mask_off=dev_t(np.asarray([j[3] for j in jobs], np.int64)),
                  mask_stride=dev_t(np.asarray([j[4] for j in jobs], np.int32)), mask_val=dev_t(np.asarray([j[5] for j in jobs], np.int32)))
    return ops.ball_cloud(dev_t(depth.view(np.int16)), dev_t(np.asarray([j[0] for j in jobs], np.int32)),
                          dev_t(np.stack([np.asarray(j[1], F) for j in jobs])), dev_t(np.stack([np.asarray(j[2], F) for j in jobs])),
                          dev_t(np.tile(np.asarray(camk, F), (I, 1))), cap=cap, full_scan=full_scan, **kw)


def same_as_ref(rec, j, want_recs, want_counts):
    """job j of a BallRecords equals the restatement's (recs, counts): torch.equal on the counts and the written records"""
    assert torch.equal(rec.counts[j].cpu(), torch.from_numpy(want_counts)), (j, rec.counts[j].tolist(), want_counts.tolist())
    n = min(int(want_counts[1]), rec.cap)
    assert torch.equal(rec.recs[j, :n].cpu(), torch.from_numpy(want_recs.astype(np.int32))), j


def sorted_distances(depth, center, mask=None, mask_val=0, camk=CAMK):
    pix = br.valid_pixels(depth, mask, mask_val)
    W = depth.shape[1]
    return np.sort(br.distances(br.pixel_points(pix % W, pix // W, depth.reshape(-1)[pix], camk), center))


def ladder_holding(d, cum):
    """an ascending ladder whose level i holds exactly cum[i] of the sorted distances d (a radius halfway between two of them)"""
    lad = []
    for c in cum:
        lo = d[c - 1] if c > 0 else F(0.5) * d[0]
        hi = d[c] if c < len(d) else F(2.0) * d[-1]
        assert lo < hi, "two equal distances at the cut: pick another count"
        lad.append(F(0.5) * (lo + hi) if c > 0 else lo)
    lad = np.asarray(lad, F)
    assert (np.diff(lad) >= 0).all() and [int((d <= r).sum()) for r in lad] == list(cum)
    return lad


CENTER = np.array([0.03, -0.02, 0.52], F)          # near the object of make_frame


def test_ladder_outcomes():
    dep, _ = make_frame(1)
    assert (dep == 0).any() and (dep == 65535).any()
    d = sorted_distances(dep, CENTER)
    cums = {"level0": [40, 50, 60, 70, 80, 90, 100, 110, 120, 130], "level3": [2, 5, 9, 31, 40, 50, 60, 70, 80, 90],
            "exact10": [3, 6, 10, 20, 30, 40, 50, 60, 70, 80], "exact9": [3, 6, 9, 20, 30, 40, 50, 60, 70, 80],
            "none": [0] * 10}
    for k in range(1, 10):
        cums["last%d" % k] = [0] * 8 + [1 if k > 1 else 0, k]
    want_L = {"level0": 0, "level3": 3, "exact10": 2, "exact9": 3, "none": 9}
    jobs = [(0, CENTER, ladder_holding(d, c)) for c in cums.values()]
    jobs.append((1, CENTER, ladder_holding(d, cums["level0"])))                     # frame 1: no valid pixel at all
    rec = gpu_crop(np.stack([dep, np.zeros_like(dep)]), jobs)
    for j, (name, c) in enumerate(cums.items()):
        recs, counts = br.ball_cloud(dep, CAMK, CENTER, jobs[j][2])
        L = want_L.get(name, 9)
        assert counts[2] == L and counts[1] == c[L] and counts[3] == (1 if name == "none" else 0), name
        same_as_ref(rec, j, recs, counts)
    assert rec.counts[-1].tolist() == [0, 0, 9, 2]
    # the Python layer's fall-back for status 1: a ladder of 1e9 takes every valid pixel
    rec = gpu_crop(dep[None], [(0, CENTER, BIG)])
    recs, counts = br.ball_cloud(dep, CAMK, CENTER, BIG)
    assert counts[1] == counts[0] == (dep > 0).sum() and counts[3] == 0
    same_as_ref(rec, 0, recs, counts)


def _pixel_center(u, v, z):
    return np.array([(u - CAMK[2]) * z / CAMK[0], (v - CAMK[3]) * z / CAMK[1], z], F)


@pytest.mark.parametrize("W", [128, 125])           # 16-byte depth loads; plain loads (rows not 16-byte aligned)
def test_rectangle_equals_full_scan(W):
    H = 96
    dep, _ = make_frame(2, H, W)
    lad = lambda r: (r * 1.1 ** np.arange(br.LEVELS)).astype(F)         # unclamped: a ladder is the kernel's input, whatever made it
    cases = {"inside": (_pixel_center(0.55 * W, 0.45 * H, 0.52), lad(0.02)), "left": (_pixel_center(2.0, 50.0, 0.9), lad(0.03)),
             "right": (_pixel_center(W - 2.5, 40.0, 0.9), lad(0.03)), "top": (_pixel_center(60.0, 1.0, 0.9), lad(0.03)),
             "bottom": (_pixel_center(70.0, H - 1.5, 0.97), lad(0.03)), "outside": (_pixel_center(-9.0, H + 7.0, 0.95), lad(0.08)),
             "behind": (np.array([0.0, 0.0, 0.05], F), lad(0.9)), "one_pixel": (_pixel_center(-1.5, -1.5, 1.0), lad(1e-5)),
             "far_outside": (_pixel_center(-900.0, 50.0, 0.9), lad(0.05)), "nan": (np.array([np.nan, 0.0, 0.9], F), lad(0.05)),
             "everything": (_pixel_center(60.0, 40.0, 0.8), lad(30.0))}
    jobs = [(0, c, l) for c, l in cases.values()]
    rects = {n: br.rect(c, l[-1], CAMK, H, W) for n, (c, l) in cases.items()}
    assert rects["one_pixel"] == (0, 1, 0, 1) and rects["behind"] == rects["nan"] == rects["everything"] == (0, W, 0, H)
    x0, x1, y0, y1 = rects["inside"]
    assert 0 < x0 < x1 < W and 0 < y0 < y1 < H and (x1 - x0) % 8 and rects["far_outside"][0] == rects["far_outside"][1]
    assert rects["left"][0] == 0 and rects["right"][1] == W and rects["top"][2] == 0 and rects["bottom"][3] == H
    a, b = gpu_crop(dep[None], jobs), gpu_crop(dep[None], jobs, full_scan=True)
    assert torch.equal(a.counts, b.counts)
    hits = 0
    for j, (name, (c, r)) in enumerate(cases.items()):
        recs, counts = br.ball_cloud(dep, CAMK, c, jobs[j][2])
        same_as_ref(a, j, recs, counts), same_as_ref(b, j, recs, counts)
        hits += counts[1] > 0
    assert hits >= 7


def test_rectangle_equals_full_scan_at_480_x_640():
    dep, _ = make_frame(3, 480, 640)
    camk = (591.0125, 590.16775, 322.525, 244.11084)
    c = np.array([(352.0 - camk[2]) * 0.52 / camk[0], (216.0 - camk[3]) * 0.52 / camk[1], 0.52], F)
    lad = lambda r: (r * 1.1 ** np.arange(br.LEVELS)).astype(F)
    jobs = [(0, c, np.full(br.LEVELS, 0.07, F)), (0, c, lad(0.03)), (0, c + F(0.2), lad(0.02))]
    x0, x1, y0, y1 = br.rect(c, jobs[0][2][-1], camk, 480, 640)
    assert 0 < x0 < x1 < 640 and 0 < y0 < y1 < 480
    a, b = gpu_crop(dep[None], jobs, camk=camk), gpu_crop(dep[None], jobs, camk=camk, full_scan=True)
    for j in range(3):
        recs, counts = br.ball_cloud(dep, camk, jobs[j][1], jobs[j][2])
        assert counts[1] > 2000 or j
        same_as_ref(a, j, recs, counts), same_as_ref(b, j, recs, counts)


@pytest.mark.parametrize("W", [128, 125])
def test_ordered_compaction(W):
    """counts round the workgroup's round (1024 lanes, x 8 pixels on the 16-byte path), rows without a hit between rows with hits,
    rectangle widths that are no multiple of 8 or 64, a cap below the count"""
    H = 96
    dep, _ = make_frame(4, H, W, holes=0)
    stripes = np.ones((H, W), np.uint8)
    stripes[10:40:3] = 0
    stripes[41] = 0
    c = _pixel_center(0.5 * W + 3.3, 0.5 * H, 0.9)
    d = sorted_distances(dep, c, stripes)
    jobs = []
    for n in (777, 1023, 1024, 1025, 8191, 8192, 8193):
        jobs.append((0, c, ladder_holding(d, [n] * 10), 0, 1, 0))
    rec = gpu_crop(dep[None], jobs, masks=stripes.reshape(-1))
    capped = gpu_crop(dep[None], jobs, masks=stripes.reshape(-1), cap=1000)
    for j, n in enumerate((777, 1023, 1024, 1025, 8191, 8192, 8193)):
        recs, counts = br.ball_cloud(dep, CAMK, c, jobs[j][2], mask=stripes)
        assert counts[1] == n and counts[2] == 0
        rows = np.unique(recs // W)
        assert len(rows) < rows.max() - rows.min() + 1            # rows with no hit in between
        same_as_ref(rec, j, recs, counts)
        same_as_ref(capped, j, recs[:1000], counts)               # the first cap records, the true count
    widths = [x1 - x0 for x0, x1, _, _ in (br.rect(c, j[2][-1], CAMK, H, W) for j in jobs)]
    assert any(w % 8 and w < W for w in widths)


def test_mask_modes():
    dep, obj = make_frame(5)
    H, W = dep.shape
    r = np.random.RandomState(0)
    m3 = np.zeros((H, W, 3), np.uint8)                            # the (H,W,n) layout: stride 3
    m3[..., 0], m3[..., 1], m3[..., 2] = obj, r.randint(0, 4, (H, W)), np.where(obj, 7, r.randint(0, 3, (H, W)))
    flat = np.stack([obj.astype(np.uint8) * 200, m3[..., 1]])     # (H,W) images: stride 1
    lad = br.ladder_of(F(0.07))
    ref_jobs = [(m3[..., 0], 0), (m3[..., 1], 0), (m3[..., 1], 3), (m3[..., 2], 7), (m3[..., 2], 1)]
    jobs3 = [(0, CENTER, lad, ch, 3, v) for ch, v in ((0, 0), (1, 0), (1, 3), (2, 7), (2, 1))]
    rec = gpu_crop(dep[None], jobs3, masks=m3.reshape(-1))
    for j, (m, v) in enumerate(ref_jobs):
        same_as_ref(rec, j, *br.ball_cloud(dep, CAMK, CENTER, lad, mask=m, mask_val=v))
    jobs1 = [(0, CENTER, lad, 0, 1, 0), (0, CENTER, lad, H * W, 1, 2), (0, CENTER, lad, 0, 1, 200), (0, CENTER, lad, 0, 1, 5)]
    rec = gpu_crop(dep[None], jobs1, masks=flat.reshape(-1))
    for j, (m, v) in enumerate(((flat[0], 0), (flat[1], 2), (flat[0], 200), (flat[0], 5))):
        want = br.ball_cloud(dep, CAMK, CENTER, lad, mask=m, mask_val=v)
        same_as_ref(rec, j, *want)
    assert want[1].tolist() == [0, 0, 9, 2]                       # a byte no pixel has: no valid pixel
    none = gpu_crop(dep[None], [(0, CENTER, lad)])
    same_as_ref(none, 0, *br.ball_cloud(dep, CAMK, CENTER, lad))
    assert none.counts[0, 0] > rec.counts[0, 0] > 0


def test_jobs_are_independent():
    frames = np.stack([make_frame(s)[0] for s in (6, 7, 8)])
    r = np.random.RandomState(5)
    jobs = []
    for j in range(17):
        c = _pixel_center(r.uniform(-10, 138), r.uniform(-10, 106), r.uniform(0.4, 1.0))
        jobs.append((int(r.randint(3)), c, br.ladder_of(F(r.uniform(0.01, 0.2)))))
    assert sorted({j[0] for j in jobs}) == [0, 1, 2] and min(sum(j[0] == i for j in jobs) for i in range(3)) >= 2      # several per frame
    jobs.append((3, jobs[0][1], jobs[0][2]))                      # an 18th that names no frame: reported, the others untouched
    both = gpu_crop(frames, jobs)
    again = gpu_crop(frames, jobs)
    assert torch.equal(both.counts, again.counts)
    assert both.counts[17].tolist() == [0, 0, 9, 3]
    hits = 0
    for j in range(17):
        one = gpu_crop(frames, [jobs[j]])
        n = int(one.counts[0, 1])
        hits += n > 0
        assert torch.equal(one.counts[0], both.counts[j]) and torch.equal(one.recs[0, :n], both.recs[j, :n])
        assert torch.equal(again.recs[j, :n], both.recs[j, :n])
        same_as_ref(both, j, *br.ball_cloud(frames[jobs[j][0]], CAMK, jobs[j][1], jobs[j][2]))
    assert hits >= 8


def test_distance_decided_at_equality():
    """rungs that ARE sorted distances d[k], and the float just below: `d <= ladder[i]` is decided at equality, so a root that is
    one ulp off changes a level.  Many k, depth frame and point list."""
    from tgpose_amd import ops
    dep, _ = make_frame(11)
    jobs, r = [], np.random.RandomState(3)
    for t in range(24):
        c = _pixel_center(r.uniform(20, 108), r.uniform(15, 80), r.uniform(0.45, 0.95))
        d = np.unique(sorted_distances(dep, c))
        ks = np.sort(r.choice(np.arange(5, 3000), 5, replace=False))
        rungs = np.stack([np.nextafter(d[ks], F(0)), d[ks]], 1).reshape(-1)         # below d[k], then d[k] itself: ascending
        jobs.append((0, c, rungs.astype(F)))
    rec = gpu_crop(dep[None], jobs)
    full = gpu_crop(dep[None], jobs, full_scan=True)
    for j, (_, c, lad) in enumerate(jobs):
        recs, counts = br.ball_cloud(dep, CAMK, c, lad)
        assert counts[1] >= 5
        same_as_ref(rec, j, recs, counts), same_as_ref(full, j, recs, counts)
    # every rung as its own last level: the counts at d[k] and just below it, for 40 distances of one centre
    c = jobs[0][1]
    d = np.unique(sorted_distances(dep, c))
    ks = np.sort(r.choice(np.arange(10, 4000), 40, replace=False))
    lads = [np.full(br.LEVELS, v, F) for k in ks for v in (np.nextafter(d[k], F(0)), d[k])]
    rec = gpu_crop(dep[None], [(0, c, l) for l in lads])
    for j, l in enumerate(lads):
        same_as_ref(rec, j, *br.ball_cloud(dep, CAMK, c, l))
    assert (np.diff(rec.counts[:, 1].cpu().numpy().reshape(-1, 2), axis=1) >= 1).all()       # d[k] itself is inside, one ulp below is not
    # the point-list source
    lists = (r.randn(1, 2000, 3) * 0.06 + np.array([0.03, -0.02, 0.8])).astype(F)
    c = np.array([0.03, -0.02, 0.8], F)
    d = np.unique(br.distances(lists[0], c))
    ks = np.sort(r.choice(np.arange(10, 1900), 40, replace=False))
    lads = np.stack([np.full(br.LEVELS, v, F) for k in ks for v in (np.nextafter(d[k], F(0)), d[k])])
    rec = ops.ball_cloud_pts(dev_t(lists), dev_t(np.zeros(len(lads), np.int32)), dev_t(np.tile(c, (len(lads), 1))), dev_t(lads))
    for j, l in enumerate(lads):
        same_as_ref(rec, j, *br.ball_cloud_pts(lists[0], c, l))


def _select_jobs():
    dep, _ = make_frame(9)
    d = sorted_distances(dep, CENTER)
    cums = ([12] * 10, [96] * 10, [700] * 10, [0] * 10)            # 12 -> 96 entries for 64 samples; 96; more than asked for; none
    jobs = [(0, CENTER, ladder_holding(d, c)) for c in cums] + [(1, CENTER, BIG)]
    frames = np.stack([dep, np.zeros_like(dep)])
    return frames, jobs, gpu_crop(frames, jobs)


def test_ball_select():
    from tgpose_amd import ops
    frames, jobs, rec = _select_jobs()
    n_pts = 64
    sel = np.zeros((5, n_pts), np.int32)
    sel[0] = np.r_[np.arange(48) * 2, -1, 96, 97, 10 ** 9, -2 ** 31, 95, np.arange(10)]       # the doubled list holds 96
    sel[1] = np.r_[np.arange(60) + 36, 96, 100, -1, 95]                                       # 96 entries, none doubled
    sel[2] = np.r_[np.arange(60) * 11, 699, 700, 701, 0]
    sel[3], sel[4] = np.arange(n_pts), np.arange(n_pts)                                       # empty crops: NaN throughout
    out, pix = ops.ball_select(rec, dev_t(sel))
    for j in range(5):
        recs, counts = br.ball_cloud(frames[jobs[j][0]], CAMK, jobs[j][1], jobs[j][2])
        want, wpix = br.ball_select(recs, counts[1], rec.cap, sel[j], br.depth_points_of(frames[jobs[j][0]], CAMK))
        assert torch.equal(pix[j].cpu(), torch.from_numpy(wpix)), j
        assert np.array_equal(out[j].cpu().numpy(), want, equal_nan=True), j
    assert (pix[0, 48:53] == -1).all() and pix[0, 53] >= 0 and (pix[3:] == -1).all() and torch.isnan(out[3:]).all()
    assert set(pix[0][pix[0] >= 0].tolist()) <= set(rec.recs[0, :12].tolist())
    # a cap below the count: the selection works from the first cap records
    frames, jobs = frames[:1], jobs[2:3]
    capped = gpu_crop(frames, jobs, cap=100)
    out, pix = ops.ball_select(capped, dev_t(np.arange(128, dtype=np.int32)[None] * 2))
    recs, counts = br.ball_cloud(frames[0], CAMK, jobs[0][1], jobs[0][2], cap=100)
    want, wpix = br.ball_select(recs, counts[1], 100, np.arange(128) * 2, br.depth_points_of(frames[0], CAMK))
    assert counts[1] == 700 and (wpix[:100] >= 0).all() and (wpix[100:] == -1).all()
    assert torch.equal(pix[0].cpu(), torch.from_numpy(wpix)) and np.array_equal(out[0].cpu().numpy(), want, equal_nan=True)


def test_ball_sample():
    from tgpose_amd import ops
    frames, jobs, rec = _select_jobs()
    for n_pts in (64, 96):
        out, pix = ops.ball_sample(rec, n_pts, seed=1234)
        out2, pix2 = ops.ball_sample(rec, n_pts, seed=1234)
        assert torch.equal(pix, pix2) and np.array_equal(out.cpu().numpy(), out2.cpu().numpy(), equal_nan=True)     # repeatable
        other = ops.ball_sample(rec, n_pts, seed=1235)[1]
        assert not torch.equal(pix[2], other[2])
        for j in range(3):
            n = int(rec.counts[j, 1])
            members = rec.recs[j, :n].tolist()
            assert set(pix[j].tolist()) <= set(members), j                                  # every row a set of crop members
            sel = br.sample_selection(n, n_pts, 1234, j)
            want, wpix = br.ball_select(np.asarray(members, np.uint32), n, rec.cap, sel, br.depth_points_of(frames[0], CAMK))
            assert torch.equal(pix[j].cpu(), torch.from_numpy(wpix)) and np.array_equal(out[j].cpu().numpy(), want), j
            if n_pts == br.doubled_len(n, n_pts):                                           # the whole doubled list is drawn:
                assert set(pix[j].tolist()) == set(members)                                 # all crop members appear
                assert sorted(sel.tolist()) == list(range(n_pts))
            if n > n_pts:
                assert len(set(pix[j].tolist())) == n_pts                                   # a subset without repetition
        assert (pix[3:] == -1).all() and torch.isnan(out[3:]).all()                         # status 1 and 2: NaN rows
    assert rec.counts[3, 3] == 1 and rec.counts[4, 3] == 2
    # a status that is not 0 blanks the row whatever the count says
    counts = rec.counts.clone()
    counts[2, 3] = 1
    assert (ops.ball_sample(rec, 64, 1, counts=counts)[1][2] == -1).all()


def test_points_equal_the_roi_path():
    """a pixel cropped by the ball and by tgp_roi_cloud gives the same bits"""
    from tgpose_amd import ops
    dep, _ = make_frame(10)
    H, W = dep.shape
    camk = (591.0125, 590.16775, 62.525, 44.11084)
    cmin, rmin, roi = 20, 10, 64                                  # a 64 x 64 window at scale 1: ROI pixel (x, y) = source (20 + x, 10 + y)
    depth, camk_t = dev_t(dep.view(np.int16))[None], dev_t(np.asarray(camk, F))[None]
    one = torch.ones(H * W, dtype=torch.uint8, device=DEV)
    z32 = torch.zeros(1, dtype=torch.int32, device=DEV)
    rr = ops.roi_cloud(depth, one, torch.zeros(1, dtype=torch.int64, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV), z32,
                       dev_t(np.asarray([[2 * cmin + roi, 2 * rmin + roi, roi]], np.int32)), camk_t, roi_size=roi, cut_frac=0.0)
    n = int(rr.counts[0, 2])
    assert n > 3000
    roi_pts = ops.cloud_select(rr, torch.arange(n, dtype=torch.int32, device=DEV)[None])[0]
    p = (rr.recs[0, :n].cpu().numpy().view(np.uint32) >> 16).astype(np.int64)
    src = (rmin + p // roi) * W + cmin + p % roi
    assert np.array_equal(rr.recs[0, :n].cpu().numpy().view(np.uint32) & 0xffff, dep.reshape(-1)[src])
    ball = ops.ball_cloud(depth, z32, torch.zeros(1, 3, device=DEV), dev_t(BIG)[None], camk_t)
    everything = ball.recs[0, :int(ball.counts[0, 1])].cpu().numpy()
    assert np.array_equal(everything, np.nonzero(dep.reshape(-1) > 0)[0])
    pos = np.searchsorted(everything, src)
    assert np.array_equal(everything[pos], src)
    ball_pts, pix = ops.ball_select(ball, dev_t(pos.astype(np.int32))[None])
    assert np.array_equal(pix[0].cpu().numpy(), src) and torch.equal(ball_pts[0], roi_pts)
    assert np.array_equal(roi_pts.cpu().numpy(), br.pixel_points(src % W, src // W, dep.reshape(-1)[src], camk))


@pytest.mark.parametrize("N", [1, 63, 1025])
def test_point_list_source(N):
    from tgpose_amd import ops
    r = np.random.RandomState(N)
    lists = (r.randn(2, N, 3) * 0.06 + np.array([0.03, -0.02, 0.8])).astype(F)
    c = np.array([0.03, -0.02, 0.8], F)
    d = np.sort(br.distances(lists[1], c))
    k = lambda n: min(n, N)
    cums = ([k(40)] * 10, [0, k(2), k(5), k(31)] + [k(40)] * 6, [0] * 9 + [k(4)], [0] * 10, [N] * 10)
    jobs = [(1, c, ladder_holding(d, cu)) for cu in cums] + [(0, c, br.ladder_of(F(0.01))), (2, c, BIG)]
    rec = ops.ball_cloud_pts(dev_t(lists), dev_t(np.asarray([j[0] for j in jobs], np.int32)), dev_t(np.stack([j[1] for j in jobs])),
                             dev_t(np.stack([j[2] for j in jobs])))
    seen = set()
    for j, (i, cc, lad) in enumerate(jobs[:-1]):
        recs, counts = br.ball_cloud_pts(lists[i], cc, lad)
        seen.add((int(counts[2]), int(counts[3])))
        same_as_ref(rec, j, recs, counts)
    assert rec.counts[-1].tolist() == [0, 0, 9, 3] and (9, 1) in seen and ((0, 0) in seen or N < 10)
    if N > 31:
        assert (3, 0) in seen and (9, 0) in seen
    sel = dev_t((np.arange(len(jobs) * 8).reshape(len(jobs), 8) % (2 * N)).astype(np.int32))
    out, pix = ops.ball_select(rec, sel)
    for j, (i, cc, lad) in enumerate(jobs[:-1]):
        recs, counts = br.ball_cloud_pts(lists[i], cc, lad)
        want, wpix = br.ball_select(recs, counts[1], rec.cap, sel[j].cpu().numpy(), lambda p: lists[i][p])
        assert torch.equal(pix[j].cpu(), torch.from_numpy(wpix)) and np.array_equal(out[j].cpu().numpy(), want, equal_nan=True), j
    capped = ops.ball_cloud_pts(dev_t(lists), dev_t(np.asarray([1], np.int32)), dev_t(c[None]), dev_t(jobs[4][2][None]), cap=max(1, N // 2))
    same_as_ref(capped, 0, *br.ball_cloud_pts(lists[1], c, jobs[4][2], cap=max(1, N // 2)))


def test_compatibility_functions_equal_the_reference():
    from tgpose_amd.network.point_sample import pc_sample_sphere as ps
    fx = fixture()
    pts = torch.from_numpy(fx["pts.cloud"])
    for name in (str(n) for n in fx["pts.names"]):
        c, radius = torch.from_numpy(fx["pts.%s.center" % name]), torch.tensor(float(fx["pts.%s.radius" % name]))
        got = ps.crop_ball_from_pts(pts, c, radius)
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), fx["pts.%s.all" % name]), name
        torch.manual_seed(int(fx["pts.%s.seed" % name]))
        got = ps.crop_ball_from_pts(pts.to(DEV), c, radius, num_points=NUM)
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), fx["pts.%s.drawn" % name]), name
        assert np.array_equal(torch.randperm(5).numpy(), fx["pts.%s.next" % name]), name
    got = ps.crop_ball_from_pts(pts, torch.from_numpy(fx["pts.twelve.center"]), torch.tensor(float(fx["pts.twelve.radius"])),
                                num_points=NUM, device=DEV, fps_sample=True)
    assert np.array_equal(got.numpy(), fx["pts.twelve.fps"])
    got = ps.crop_ball_from_pts(pts, torch.from_numpy(fx["pts.level0.center"]), torch.tensor(float(fx["pts.level0.fps_radius"])),
                                num_points=NUM, device=DEV, fps_sample=True)
    assert np.array_equal(got.numpy(), fx["pts.level0.fps"])
    assert len(ps.crop_ball_from_pts(pts[:0], torch.zeros(3), 0.1, num_points=4)) == 0
    # a Python-number radius: doubles, rounded when compared
    got = ps.crop_ball_from_pts(pts, torch.from_numpy(fx["pts.level0.center"]), 0.2)
    assert np.array_equal(got.numpy(), br.ball_cloud_pts(fx["pts.cloud"], fx["pts.level0.center"], [F(0.2)] * 10)[0])

    dep, mask, camk = fx["img.depth"], fx["img.mask"], fx["img.camk"]
    H, W = dep.shape
    allpix = np.arange(H * W)
    cloud = br.pixel_points(allpix % W, allpix // W, dep.reshape(-1), camk)
    image = torch.from_numpy(np.repeat(allpix.reshape(H, W, 1), 3, axis=2)).to(DEV)
    depth3 = torch.from_numpy(cloud.reshape(H, W, 3)).to(DEV)
    pose, scale, ratio = torch.from_numpy(fx["img.pose"]), torch.from_numpy(fx["img.scale"]), float(fx["img.ratio"])     # on the host, as recorded
    for name, m, kw in (("nomask_all", None, {}), ("mask_all", mask, {}), ("nomask_drawn", None, dict(num_points=NUM)),
                        ("mask_drawn", mask, dict(num_points=NUM)), ("mask_fps", mask, dict(num_points=NUM, device=DEV, fps_sample=True))):
        torch.manual_seed(int(fx["img.seed"]))
        rgb, p, nocs = ps.crop_ball_from_depth_image(image, depth3, None if m is None else torch.from_numpy(m).to(DEV), pose, scale, ratio,
                                                     None, coord=depth3, **kw)
        pix = rgb[:, 0].cpu().numpy()
        assert np.array_equal(pix, fx["img.%s.pix" % name]), name
        assert np.array_equal(p.cpu().numpy(), cloud[pix]) and torch.equal(p, nocs)
    # valid pixels but none within the first radius, num_points=None: retried with the ratio grown by 1.2, as the reference
    rgb, p, nocs = ps.crop_ball_from_depth_image(image, depth3, torch.from_numpy(mask).to(DEV), torch.from_numpy(fx["img.grow.pose"]), scale,
                                                 ratio, None)
    assert nocs is None and np.array_equal(rgb[:, 0].cpu().numpy(), fx["img.grow.pix"]) and len(fx["img.grow.radii"]) >= 3
    with pytest.raises(ValueError, match="no valid pixel"):
        ps.crop_ball_from_depth_image(image, torch.zeros_like(depth3), None, pose, scale, ratio, None, num_points=8)
    with pytest.raises(ValueError, match="no ball"):              # valid pixels, but no distance to a NaN centre is within any radius
        ps.crop_ball_from_depth_image(image, depth3, None, pose * float("nan"), scale, ratio, None)
    idx = ps.farthest_point_sample(pts, 1000, DEV)
    assert torch.equal(idx, torch.arange(len(pts)))
