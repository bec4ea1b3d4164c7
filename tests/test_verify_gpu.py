"""Pose verification on the GPU (csrc/verify.hip, ops.pose_verify) against the NumPy restatement of its contract
(tests/verify_ref.py): counts equal, score bit-equal, on the cases of tests/verify_cases.py; against the classification computed
with torch from ops.render_depth run with one scene per job; and called twice, from a captured graph and on a side stream."""
import numpy as np
import pytest
import torch

from tests import render_cases as rc
from tests import verify_cases as vc
from tests import verify_ref as vr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = vr.COL


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")


_MESHSETS = {}


def _args(c):
    """the case on the device: (positional arguments, keywords) of ops.pose_verify"""
    from tgpose_amd import ops
    key = id(c["meshes"])
    if key not in _MESHSETS:
        _MESHSETS[key] = (c["meshes"], ops.MeshSet(c["meshes"], device=DEV))
    up = lambda a: torch.from_numpy(np.array(a, order="C")).to(DEV)
    kw = dict(tau=c["tau"], near=c["near"])
    if c["mask"] is not None:
        kw.update(mask=up(c["mask"]), job_mask_val=up(c["job_mask_val"]))
    return (_MESHSETS[key][1], up(c["depth"].view(np.int16))) + tuple(up(c[k]) for k in ("camk", "job_img", "job_mesh", "job_pose")), kw


def _verify(c):
    from tgpose_amd import ops
    args, kw = _args(c)
    return ops.pose_verify(*args, **kw)


def _assert_equal(out, ref, what=""):
    got, want = out["counts"].cpu().numpy(), ref["counts"]
    assert got.shape == want.shape and got.dtype == want.dtype == np.int32
    bad = got != want
    assert not bad.any(), "%s counts differ at (job, column) %s: kernel\n%s\nrestatement\n%s" % (what, np.argwhere(bad).tolist(), got, want)
    score = out["score"].cpu().numpy()
    assert score.dtype == np.float32 and np.array_equal(score.view(np.int32), ref["score"].view(np.int32)), (what, score, ref["score"])


CASES = [("rectangle", s) for s in sorted(rc.RECT_SPLITS)] + [("rules", None), ("tails", None), ("tiny_triangles", None), ("seven_jobs", None)]


@pytest.mark.parametrize("name,arg", CASES, ids=["%s-%s" % c if c[1] is not None else c[0] for c in CASES])
def test_kernel_equals_restatement(name, arg):
    """the CPU file's closed-form cases; a job off-screen, a vertex behind near, the guard band, a surface beyond 65.535 m; tile
    tails and a mesh larger than the image at 123 x 157; 20 480 triangles in about one tile; seven jobs over three frames with a
    camk each, two sharing a frame and a mesh, one with job_img out of range -- each with its mask and without"""
    c, ref = vc.reference(name, arg)
    out = _verify(c)
    torch.cuda.synchronize()
    print("%s: counts (%s)\n%s\nscore %s" % (name, ", ".join(vr.COUNTS), out["counts"].cpu().numpy(), out["score"].cpu().numpy()))
    _assert_equal(out, ref, name)
    if c["mask"] is not None:
        bare = _verify(vc.without_mask(c))
        want = ref["counts"].copy()
        want[:, C["in_mask"]] = 0
        _assert_equal(bare, dict(counts=want, score=ref["score"]), name + " without a mask")
    n = ref["counts"]
    if name == "tails":
        assert n[0, C["occluded"]] > 500 and n[0, C["rendered"]] > 0.9 * 123 * 157          # the table behind the objects, over all the image
        assert n[3, C["violation"]] > 100 and n[4, C["occluded"]] > 100
    if name == "tiny_triangles":
        assert 100 <= n[0, C["rendered"]] <= 160 and n[0, C["match"]] == n[0, C["rendered"]] and n[0, C["abs_sum"]] == 3 * n[0, C["rendered"]]
        assert len(c["meshes"][0][1]) == 20480
    if name == "rules":
        assert not n[0].any() and n[1, C["dropped"]] == 1 and n[4, C["nodata"]] == n[4, C["rendered"]] > 0


def test_counts_equal_the_classification_of_separately_rendered_frames():
    """an independent path to the same integers: ops.render_depth with one scene per job (J full frames), classified with torch"""
    from tgpose_amd import ops
    c, ref = vc.reference("seven_jobs")
    (ms, depth, camk, job_img, job_mesh, job_pose), kw = _args(c)
    out = ops.pose_verify(ms, depth, camk, job_img, job_mesh, job_pose, **kw)
    S, H, W = depth.shape
    valid = (job_img >= 0) & (job_img < S)                                                 # host knowledge: the test built the jobs
    keep = torch.nonzero(valid).reshape(-1)
    J = keep.numel()
    assert J == 6
    ren = ops.render_depth(ms, torch.arange(J + 1, device=DEV, dtype=torch.int32), job_mesh[keep].contiguous(),
                           torch.ones(J, device=DEV, dtype=torch.uint8), job_pose[keep].contiguous(), camk[job_img[keep].long()].contiguous(),
                           H, W, near=c["near"])
    wide = lambda t: t.view(torch.int16).to(torch.int32) & 0xffff
    d_r, d_o, covered = wide(ren["depth"]), wide(depth)[job_img[keep].long()], ren["mask"] > 0
    tau = c["tau"]
    nodata = covered & ((d_o == 0) | (d_r == 0))
    rest = covered & ~nodata
    occluded = rest & (d_o + tau < d_r)
    match = rest & ((d_o - d_r).abs() <= tau)
    violation = rest & (d_o > d_r + tau)
    in_mask = covered & (kw["mask"][job_img[keep].long()] == kw["job_mask_val"][keep][:, None, None])
    cols = [covered, match, violation, occluded, nodata, in_mask]
    want = torch.zeros(len(c["job_img"]), 8, dtype=torch.int32, device=DEV)
    want[keep] = torch.stack([x.sum((1, 2)) for x in cols] + [((d_o - d_r).abs() * match).sum((1, 2)), ren["dropped"].sum(1)], 1).to(torch.int32)
    assert torch.equal(out["counts"], want), (out["counts"], want)
    assert torch.equal(ren["visible"], out["counts"][keep, 0])


def test_repeatability_graph_replay_and_a_side_stream():
    """two calls give the same bytes; so does a replay of the call captured in a graph; a call on a side stream is correct"""
    from tgpose_amd import ops
    c, ref = vc.reference("tails")
    args, kw = _args(c)
    a, b = ops.pose_verify(*args, **kw), ops.pose_verify(*args, **kw)
    for k in ("counts", "score"):
        assert torch.equal(a[k], b[k]), k
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.pose_verify(*args, **kw)
    for v in out.values():
        v.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    for k in ("counts", "score"):
        assert torch.equal(out[k], a[k]), k
    _assert_equal(out, ref, "graph replay")
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        s = ops.pose_verify(*args, **kw)
    side.synchronize()
    _assert_equal(s, ref, "side stream")


def test_no_job_and_the_4x4_form():
    """J = 0 returns empty tensors without a launch; pose.verify_poses and pose.Verify on 4x4 poses equal ops.pose_verify on their
    first three rows, and on a normalised mesh with the scales"""
    from tgpose_amd import ops, pose
    c, ref = vc.reference("seven_jobs")
    (ms, depth, camk, job_img, job_mesh, job_pose), kw = _args(c)
    none = ops.pose_verify(ms, depth, camk, job_img[:0], job_mesh[:0], job_pose[:0].contiguous(), tau=c["tau"])
    assert none["counts"].shape == (0, 8) and none["score"].shape == (0,)
    RTs = torch.zeros(len(job_pose), 4, 4, device=DEV)
    RTs[:, :3, :4], RTs[:, 3, 3] = job_pose, 1.0
    out = pose.verify_poses(ms, job_mesh, depth, camk, RTs, job_img=job_img, **kw)
    _assert_equal(out, ref, "verify_poses")
    v = pose.Verify(ms, job_mesh, tau=c["tau"], min_score=0.9)(depth, camk, RTs, None, job_img, kw["mask"], kw["job_mask_val"])
    _assert_equal(v, ref, "Verify")
    assert np.array_equal(v["verified"].cpu().numpy(), ref["score"] >= np.float32(0.9)) and v["verified"].dtype == torch.bool
    # a normalised mesh: the pose's columns divided by the scales, the scales handed in -- powers of two, so the products are exact
    sc = torch.tensor([[2.0, 0.5, 4.0]], device=DEV).expand(len(job_pose), 3).contiguous()
    squeezed = RTs.clone()
    squeezed[:, :3, :3] /= sc[:, None, :]
    n = pose.Verify(ms, job_mesh, tau=c["tau"], normalised=True)(depth, camk, squeezed, sc, job_img, kw["mask"], kw["job_mask_val"])
    _assert_equal(n, ref, "normalised")
