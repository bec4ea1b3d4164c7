"""CPU tests of the ball crop (csrc/ballcrop.hip, ops.ball_*, network/point_sample/pc_sample_sphere.py): the NumPy restatement of the
contract (tests/ball_ref.py) against what the reference itself returned (tests/golden/ball_crop_ref.npz, recorded by
tests/golden/make_ball_crop_golden.py), the two branches of the radius ladder, the C ABI of the new entry points, their argument
errors (which return before any launch) and the host-only helpers."""
import os

import numpy as np
import pytest
import torch

from tests import ball_ref as br
from tests import fps_ref
from tests.util import ROOT

NUM = 64
_FX = {}


def fixture():
    if not _FX:
        path = os.path.join(ROOT, "tests", "golden", "ball_crop_ref.npz")
        assert os.path.exists(path), "tests/golden/ball_crop_ref.npz is missing: run tests/golden/make_ball_crop_golden.py"
        _FX.update(np.load(path))
    return _FX


def crop_with_fallback(crop, ladder):
    """the reference's `if len(idx) == 0: idx = where(distance <= 1e9)` as the Python layer does it: a second crop"""
    recs, counts = crop(ladder)
    if counts[3] == 1:
        recs, counts = crop(np.full(br.LEVELS, 1e9, np.float32))
    return recs.astype(np.int64), counts


def drawn(recs, seed):
    """random_sample on the doubled list under the recorded seed -> (chosen records, the generator's next randperm(5))"""
    torch.manual_seed(int(seed))
    sel = torch.randperm(br.doubled_len(len(recs), NUM))[:NUM].numpy()
    return recs[sel % len(recs)], torch.randperm(5).numpy()


def fps_chosen(recs, points):
    """farthest point sampling (the contract of tgp_fps, tests/fps_ref.py) of the doubled list"""
    dbl = np.arange(br.doubled_len(len(recs), NUM)) % len(recs)
    idx = fps_ref.fps(points[recs[dbl]], NUM, init_center=True)[0]
    return recs[dbl[idx]]


def test_point_list_crops_equal_the_reference_bit_for_bit():
    fx = fixture()
    pts = fx["pts.cloud"]
    seen = set()
    for name in (str(n) for n in fx["pts.names"]):
        c, radius = fx["pts.%s.center" % name], fx["pts.%s.radius" % name]
        lad = br.ladder_of(radius)
        first, counts0 = br.ball_cloud_pts(pts, c, np.repeat(lad[:1], br.LEVELS))          # num_points=None: the first radius alone
        assert np.array_equal(first, fx["pts.%s.all" % name]), name
        recs, counts = crop_with_fallback(lambda l: br.ball_cloud_pts(pts, c, l), lad)
        _, raw = br.ball_cloud_pts(pts, c, lad)
        seen.add((int(raw[2]), int(raw[3])))
        got, nxt = drawn(recs, fx["pts.%s.seed" % name])
        assert np.array_equal(got, fx["pts.%s.drawn" % name]), name
        assert np.array_equal(nxt, fx["pts.%s.next" % name]), name
    # every ladder outcome: the first level, a middle one, the last with a few points, the last with none
    assert {(0, 0), (1, 0), (3, 0), (9, 0), (9, 1)} <= seen
    # the doubling: 12 points -> 64 samples draw only from those 12, and all of them
    assert len(fx["pts.twelve.all"]) == 12 and set(fx["pts.twelve.drawn"]) <= set(fx["pts.twelve.all"])
    assert len(fx["pts.exact10.all"]) == 10 and len(fx["pts.exact9.all"]) == 9
    # nothing within the last radius: every point is a candidate
    assert len(fx["pts.none9.all"]) == 0 and len(set(fx["pts.none9.drawn"])) == NUM


def test_point_list_farthest_point_selection_equals_the_reference():
    fx = fixture()
    pts = fx["pts.cloud"]
    c = fx["pts.twelve.center"]
    recs, _ = crop_with_fallback(lambda l: br.ball_cloud_pts(pts, c, l), br.ladder_of(fx["pts.twelve.radius"]))
    got = fps_chosen(recs, pts)
    assert np.array_equal(got, fx["pts.twelve.fps"])
    # on a doubled list: the distinct points once, then row 0 of the list
    assert len(set(got[:12])) == 12 and (got[12:] == recs[0]).all()
    c = fx["pts.level0.center"]
    recs, _ = crop_with_fallback(lambda l: br.ball_cloud_pts(pts, c, l), br.ladder_of(fx["pts.level0.fps_radius"]))
    assert len(recs) > NUM and np.array_equal(fps_chosen(recs, pts), fx["pts.level0.fps"])


def test_depth_frame_crops_equal_the_reference_bit_for_bit():
    fx = fixture()
    dep, camk, pose = fx["img.depth"], fx["img.camk"], fx["img.pose"]
    lad = br.ladder_of(fx["img.radius"])
    radius = (float(fx["img.ratio"]) * torch.norm(torch.from_numpy(pose)[:, :3] @ torch.from_numpy(fx["img.scale"]))).numpy()
    assert radius == fx["img.radius"]
    assert (dep == 0).any() and (dep == 65535).any()
    allpix = np.arange(dep.size)
    cloud = br.pixel_points(allpix % dep.shape[1], allpix // dep.shape[1], dep.reshape(-1), camk)
    for tag, mask in (("nomask", None), ("mask", fx["img.mask"])):
        first, _ = br.ball_cloud(dep, camk, pose[:, 3], np.repeat(lad[:1], br.LEVELS), mask=mask)
        assert np.array_equal(first, fx["img.%s_all.pix" % tag]), tag
        recs, counts = crop_with_fallback(lambda l: br.ball_cloud(dep, camk, pose[:, 3], l, mask=mask), lad)
        assert counts[0] == len(br.valid_pixels(dep, mask)) and counts[3] == 0
        assert np.array_equal(drawn(recs, fx["img.seed"])[0], fx["img.%s_drawn.pix" % tag]), tag
        if mask is not None:
            assert np.array_equal(fps_chosen(recs, cloud), fx["img.mask_fps.pix"])


def test_empty_first_ball_grows_the_ratio_as_the_reference():
    """num_points=None with valid pixels but none within the first radius: the reference calls itself with ratio * 1.2 until a ball
    holds a point, and returns that ball's crop"""
    fx = fixture()
    dep, camk, pose, mask = fx["img.depth"], fx["img.camk"], fx["img.grow.pose"], fx["img.mask"]
    extent = torch.norm(torch.from_numpy(pose)[:, :3] @ torch.from_numpy(fx["img.scale"]))
    ratio, radii = float(fx["img.ratio"]), []
    while True:
        radii.append((ratio * extent).numpy())
        recs, counts = br.ball_cloud(dep, camk, pose[:, 3], np.repeat(br.ladder_of(radii[-1])[:1], br.LEVELS), mask=mask)
        if len(recs):
            break
        assert counts[3] == 1 and counts[0] > 0
        ratio = ratio * 1.2
    assert len(radii) >= 3 and np.array_equal(np.asarray(radii, np.float32), fx["img.grow.radii"])
    assert np.array_equal(recs, fx["img.grow.pix"])


def test_ladder_branches_equal_the_reference():
    from tgpose_amd import ops
    fx = fixture()
    radii = np.asarray([fx["ladder.big.radius"], fx["ladder.small.radius"]], np.float32)
    want = np.stack([fx["ladder.big.rungs"], fx["ladder.small.rungs"]])
    assert radii[0] >= 0.05 > radii[1]
    got = ops.ball_ladder(torch.from_numpy(radii))
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
    assert np.array_equal(np.stack([br.ladder_of(r) for r in radii]), want)
    # more radii: the restatement against the torch ops, including exactly 0.05 and a NaN
    more = np.asarray([0.05, 0.049999997, 0.3, 1e-9, 7.5, np.nan], np.float32)
    got = ops.ball_ladder(torch.from_numpy(more)).numpy()
    assert np.array_equal(got, np.stack([br.ladder_of(r) for r in more]), equal_nan=True)
    with pytest.raises(TypeError):
        ops.ball_ladder(torch.zeros(3, dtype=torch.float64))


def test_new_symbols_are_declared_bound_and_exported():
    """the ABI number, the ball constants against the NumPy restatement's, and the Python surface; tests/test_abi_cpu.py holds every
    symbol, type and value against the header"""
    from tgpose_amd import _lib, ops
    assert _lib.lib().tgp_version() == _lib.ABI_VERSION             # additive: the ABI number stays
    assert {k: v for k, v in _lib.CONSTANTS.items() if k.startswith("BALL_")} == {"BALL_LEVELS": 10, "BALL_THREADS": 1024}
    assert _lib.BALL_LEVELS == br.LEVELS == ops.BALL_LEVELS == 10 and _lib.BALL_THREADS == br.THREADS == 1024
    for name in ("ball_cloud", "ball_cloud_pts", "ball_select", "ball_sample", "ball_ladder", "BallRecords"):
        assert hasattr(ops, name), name
    from tgpose_amd.network.point_sample import pc_sample_sphere as ps
    for name in ("backproject", "sample_bp_depth", "crop_ball_from_pts", "random_sample", "farthest_point_sample", "crop_mask_depth_image",
                 "crop_ball_from_depth_image", "occlude_obj_by_bboxes", "get_proj_corners", "project", "get_corners", "bbox_from_corners",
                 "get_bbox_from_scale"):
        assert callable(getattr(ps, name)), name
    from tgpose_amd.evaluation import load_data_eval as lde
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    assert callable(lde.clouds_from_poses) and callable(myEvaluater.track)


def test_argument_errors_return_before_any_launch():
    """every call below is refused with TGP_EINVAL: the pointers (8) are never followed and nothing is launched, so this runs
    without a GPU"""
    from tgpose_amd import _lib
    h = _lib.lib()
    P = 8
    cloud = dict(depth=P, masks=None, mask_off=None, mask_stride=None, mask_val=None, job_img=P, centers=P, ladder=P, camk=P, J=1, I=1,
                 H=4, W=4, cap=4, full=0, recs=P, counts=P)

    def call_cloud(**kw):
        a = dict(cloud, **kw)
        return h.tgp_ball_cloud(*[a[k] for k in cloud], None)
    for bad in (dict(depth=None), dict(job_img=None), dict(centers=None), dict(ladder=None), dict(camk=None), dict(recs=None),
                dict(counts=None), dict(masks=P), dict(masks=P, mask_off=P), dict(J=0), dict(I=0), dict(H=0), dict(W=0), dict(cap=0),
                dict(H=32768), dict(H=4096, W=4096)):
        assert call_cloud(**bad) == -1, bad
    pts = dict(pts=P, job_img=P, centers=P, ladder=P, J=1, I=1, N=5, cap=5, recs=P, counts=P)
    for bad in (dict(pts=None), dict(job_img=None), dict(centers=None), dict(ladder=None), dict(recs=None), dict(counts=None), dict(J=0),
                dict(I=0), dict(N=0), dict(N=2 ** 30), dict(cap=0)):
        a = dict(pts, **bad)
        assert h.tgp_ball_cloud_pts(*[a[k] for k in pts], None) == -1, bad
    sel = dict(recs=P, counts=P, sel=P, job_img=P, depth=P, camk=P, pts=None, J=1, I=1, H=4, W=4, cap=4, n_pts=4, out=P, pix=P)
    for bad in (dict(recs=None), dict(counts=None), dict(sel=None), dict(job_img=None), dict(depth=None), dict(pts=P), dict(camk=None),
                dict(out=None), dict(pix=None), dict(J=0), dict(n_pts=0), dict(cap=0), dict(cap=2 ** 30), dict(n_pts=2 ** 30),
                dict(depth=None, pts=P, H=2), dict(H=4096, W=4096)):
        a = dict(sel, **bad)
        assert h.tgp_ball_select(*[a[k] for k in sel], None) == -1, bad
    smp = dict(recs=P, counts=P, job_img=P, depth=P, camk=P, pts=None, J=1, I=1, H=4, W=4, cap=4, n_pts=4, seed=1, out=P, pix=P)
    for bad in (dict(recs=None), dict(counts=None), dict(job_img=None), dict(depth=None), dict(pts=P), dict(out=None), dict(pix=None),
                dict(J=0), dict(n_pts=0), dict(cap=0)):
        a = dict(smp, **bad)
        assert h.tgp_ball_sample(*[a[k] for k in smp], None) == -1, bad


def test_random_sample_consumes_randperm_as_the_reference():
    from tgpose_amd.network.point_sample import pc_sample_sphere as ps
    fx = fixture()
    # the "twelve" case: the reference's own draw from the doubled list of 96 entries
    recs = fx["pts.twelve.all"]
    dbl = np.tile(recs, 8)
    torch.manual_seed(int(fx["pts.twelve.seed"]))
    pick = ps.random_sample(dbl, NUM)
    assert np.array_equal(dbl[pick.numpy()], fx["pts.twelve.drawn"]) and np.array_equal(torch.randperm(5).numpy(), fx["pts.twelve.next"])
    # a list shorter than the request: further permutations, each a prefix of what is still missing
    torch.manual_seed(3)
    got = ps.random_sample(np.zeros((5, 3)), 12)
    torch.manual_seed(3)
    want = torch.cat([torch.randperm(5), torch.randperm(5), torch.randperm(5)[:2]])
    assert torch.equal(got, want)
    with pytest.raises(ValueError):
        ps.random_sample(np.zeros((0, 3)), 4)


def test_host_helpers_equal_the_reference():
    from tgpose_amd.network.point_sample import pc_sample_sphere as ps
    fx = fixture()
    m = torch.from_numpy(fx["occ.mask"])
    shares = []
    for k, b in enumerate(fx["occ.boxes"]):
        om, share = ps.occlude_obj_by_bboxes(torch.from_numpy(b), m)
        assert np.array_equal(om.numpy(), fx["occ.%d.mask" % k]) and share == float(fx["occ.%d.share" % k]), k
        shares.append(share)
    assert min(shares) < 1.0 and max(shares) == 1.0           # a box that occludes and one that misses the mask
    assert torch.equal(m, torch.from_numpy(fx["occ.mask"]))
    pts, K, c3 = fx["pts.cloud"][:50], fx["geo.K"], fx["geo.center"]
    cs = ps.get_corners(pts)
    assert np.array_equal(cs, fx["geo.corners"]) and np.array_equal(ps.get_corners(torch.from_numpy(pts)), fx["geo.corners"])
    box = ps.bbox_from_corners(cs)
    assert box.dtype == fx["geo.bbox"].dtype and np.array_equal(box, fx["geo.bbox"])
    assert np.array_equal(ps.bbox_from_corners([cs[0], cs[1]]), fx["geo.bbox"])
    assert np.array_equal(ps.project(pts.astype(np.float64), K), fx["geo.project"])
    depth = np.zeros(fx["img.depth"].shape)
    for radius, key in ((0.11, "geo.proj_corners"), (0.01, "geo.proj_corners_small")):
        got = ps.get_proj_corners(depth, c3, radius, K)
        assert got.dtype == fx[key].dtype and np.array_equal(got, fx[key]), key
    got = ps.get_bbox_from_scale(np.array([0.2, 0.1, 0.3]))
    assert got.dtype == np.float32 and np.array_equal(got, fx["geo.bbox_from_scale"])


def test_index_plumbing_on_the_cpu_equals_the_reference_values():
    """backproject / sample_bp_depth / crop_mask_depth_image are torch code on the inputs' device: on the CPU, against the golden
    frame (the reference's rows are the valid pixels in row-major order)"""
    from tgpose_amd.network.point_sample import pc_sample_sphere as ps
    fx = fixture()
    dep, mask = fx["img.depth"], fx["img.mask"]
    H, W = dep.shape
    allpix = np.arange(H * W)
    cloud = br.pixel_points(allpix % W, allpix // W, dep.reshape(-1), fx["img.camk"])
    image = torch.from_numpy(np.repeat(allpix.reshape(H, W, 1), 3, axis=2))
    depth3 = torch.from_numpy(cloud.reshape(H, W, 3))
    rgb, pts, nocs = ps.sample_bp_depth(image, depth3, None, torch.from_numpy(mask))
    want = br.valid_pixels(dep, mask)
    assert nocs is None and np.array_equal(rgb[:, 0].numpy(), want) and np.array_equal(pts.numpy(), cloud[want])
    z = torch.from_numpy(dep.astype(np.float32))
    fxv, fyv, cx, cy = (float(v) for v in fx["img.camk"])
    K = torch.tensor([[fxv, 0, cx], [0, fyv, cy], [0, 0, 1]])
    got = ps.backproject(z, K, torch.from_numpy(mask))
    xs, ys = (want % W).astype(np.float32), (want // W).astype(np.float32)
    zz = dep.reshape(-1)[want].astype(np.float32)
    ref = np.stack([(xs - np.float32(cx)) * zz / np.float32(fxv), (ys - np.float32(cy)) * zz / np.float32(fyv), zz], 1)
    assert np.array_equal(got.numpy(), ref)
    torch.manual_seed(5)
    rgb, pts, nocs = ps.crop_mask_depth_image(image, depth3, torch.from_numpy(mask), coord=depth3, num_points=16)
    torch.manual_seed(5)
    pick = want[torch.randperm(len(want))[:16].numpy()]
    assert np.array_equal(rgb[:, 0].numpy(), pick) and np.array_equal(pts.numpy(), cloud[pick]) and torch.equal(pts, nocs)
