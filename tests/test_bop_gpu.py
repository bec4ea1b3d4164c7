"""The BOP pose errors on the GPU (csrc/poseerr.hip, csrc/vsd.hip; ops.pose_errors, ops.pose_vsd, evaluation/bop.py) against the
NumPy restatement of their contracts (tests/bop_ref.py) on the cases of tests/bop_cases.py.

The point errors are float64 on float32 inputs that float64 holds exactly, so the bound is derived, not measured:
|difference| <= 2^-40 L with L = 1 + the largest absolute coordinate of any transformed point of the job, for mspd times
max(fx, fy) / z_min * (1 + L / z_min); a few dozen roundings of 2^-53 L each stay three decimal orders below it.  L and z_min are
computed from the case (bop_ref.scale_L).  VSD is all-integer up to one division: counts, within and the bits of err are equal."""
import numpy as np
import pytest
import torch

from tests import bop_cases as bc
from tests import bop_ref as br

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V = br.VCOL


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")


_SETS = {}


def up(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def meshset(meshes):
    from tgpose_amd import ops
    if id(meshes) not in _SETS:
        _SETS[id(meshes)] = (meshes, ops.MeshSet(meshes, device=DEV))
    return _SETS[id(meshes)][1]


def symset():
    from tgpose_amd import ops
    if "sym" not in _SETS:
        _SETS["sym"] = ops.SymmetrySet(bc.groups(), device=DEV)
    return _SETS["sym"]


def point_args(c):
    return (meshset(c["meshes"]), up(c["job_mesh"]), up(c["pose_est"]), up(c["pose_gt"]), symset(), up(c["job_sym"]), up(c["camk"])), dict(near=c["near"])


def assert_points(out, c, ref, scale, what):
    err, best, status = out["err"].cpu().numpy(), out["sym_best"].cpu().numpy(), out["status"].cpu().numpy()
    J = len(c["job_mesh"])
    assert err.shape == (J, 4) and err.dtype == np.float64 and best.shape == (J, 2) and best.dtype == np.int32 and status.dtype == np.int32
    assert np.array_equal(status, ref["status"]), (what, status, ref["status"])
    tol = bc.tolerances(c, scale)
    for j in range(J):
        if ref["status"][j] & 5:                                       # an index out of range, or something not finite
            assert np.isnan(err[j]).all() and (best[j] == -1).all(), (what, j)
            continue
        cols = 3 if ref["status"][j] & 2 else 4
        diff = np.abs(err[j, :cols] - ref["err"][j, :cols])
        print("%s job %d: err %s |difference| %s bound %s" % (what, j, err[j].tolist(), diff.tolist(), tol[j].tolist()))
        assert (diff <= tol[j, :cols]).all(), (what, j, diff, tol[j])
        if cols == 3:
            assert np.isposinf(err[j, 3]) and best[j, 1] == -1, (what, j)
        for col in range(cols - 2):
            per = ref["per_sym"][j][:, col]
            assert 0 <= best[j, col] < len(per) and per[best[j, col]] - per.min() <= tol[j, 2 + col], (what, j, col, best[j])
            ranked = np.sort(per)
            if len(per) == 1 or ranked[1] - ranked[0] > 2 * tol[j, 2 + col]:
                assert best[j, col] == ref["sym_best"][j, col], (what, j, col, best[j], ref["sym_best"][j])


@pytest.mark.parametrize("name", ["sizes", "single", "mixed", "cube", "translated", "planar", "swapped", "high_sym", "pushed", "tied", "nonfinite"])
def test_point_errors_equal_the_restatement(name):
    """1, 63, 64, 65, 257, 2500 and 8300 vertices (one; around a wave; past a workgroup; three LDS tiles of ground-truth points;
    two rounds per workgroup slice) against groups of 1, 2, 4 and 315 transforms; J = 1; J = 7 with a bad mesh index, a bad group
    index and points behind the camera; the closed forms of the CPU file; the best symmetry at 200, 314 and 130 of 315 (the second
    and third round of the symmetry loop, its tail, workgroups 18, 14 and 0); bit 2 from a transform that workgroup 1 alone sees;
    equal values in two workgroups' slots; a NaN and an infinity in the poses and a NaN in the intrinsics (status 4, NaN)"""
    from tgpose_amd import ops
    c, ref, scale = bc.point_reference(name)
    args, kw = point_args(c)
    out = ops.pose_errors(*args, **kw)
    torch.cuda.synchronize()
    assert_points(out, c, ref, scale, name)
    err, best = out["err"].cpu().numpy(), out["sym_best"].cpu().numpy()
    if name == "translated":
        assert err[0, 0] == err[0, 2] == bc.STEP and best[0].tolist() == [0, 0]                      # exact on the device too
    if name == "cube":
        assert err[1, 2] == 0 and best[1].tolist() == [1, 1] and err[0, 2] > 0.1
    if name == "swapped":
        assert err[0, 1] == 0 and err[0, 0] > 0.2
    if name == "mixed":
        assert (err[6] == 0).all()
    if name == "high_sym":
        assert best.tolist() == [[q, q] for q in bc.HIGH]
    if name == "pushed":
        assert out["status"].tolist() == [2] and best[0].tolist() == [0, -1]
    if name == "tied":
        assert best[0].tolist() == [1, 1] and err[0, 2] == 0 and err[0, 3] == 0                    # the lowest of the equal indices 1, 3, 5
    if name == "nonfinite":
        assert out["status"].tolist() == [4, 4, 4, 0]


def test_point_errors_repeat_replay_and_a_side_stream():
    """two calls, a graph replay and a side stream give identical bytes; a job's result does not depend on the other jobs"""
    from tgpose_amd import ops
    c, ref, scale = bc.point_reference("mixed")
    args, kw = point_args(c)
    a, b = ops.pose_errors(*args, **kw), ops.pose_errors(*args, **kw)
    keys = ("err", "sym_best", "status")
    same = lambda x, y: x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()                       # NaN rows compare by their bytes
    for k in keys:
        assert same(a[k], b[k]), k
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.pose_errors(*args, **kw)
    for v in out.values():
        v.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        s = ops.pose_errors(*args, **kw)
    side.synchronize()
    for k in keys:
        assert same(out[k], a[k]) and same(s[k], a[k]), k
    ms, jm, pe, pg, ss, js, camk = args
    one = ops.pose_errors(ms, jm[3:4].contiguous(), pe[3:4].contiguous(), pg[3:4].contiguous(), ss, js[3:4].contiguous(), camk[3:4].contiguous())
    for k in keys:
        assert same(one[k], a[k][3:4]), k
    none = ops.pose_errors(ms, jm[:0], pe[:0].contiguous(), pg[:0].contiguous(), ss, js[:0], camk[:0].contiguous())
    assert none["err"].shape == (0, 4) and none["sym_best"].shape == (0, 2) and none["status"].shape == (0,)


def test_errors_on_4x4_poses_with_and_without_scales():
    from tgpose_amd import ops
    from tgpose_amd.evaluation import bop
    c, ref, scale = bc.point_reference("sizes")
    args, kw = point_args(c)
    ms, jm, pe, pg, ss, js, camk = args
    want = ops.pose_errors(*args, **kw)
    J = len(jm)
    wide = lambda p: torch.cat([p, torch.tensor([0.0, 0, 0, 1], device=DEV).expand(J, 1, 4)], 1)
    got = bop.errors(ms, c["job_mesh"], wide(pe), wide(pg), ss, c["job_sym"], camk)
    for k in ("err", "sym_best", "status"):
        assert torch.equal(got[k], want[k]), k
    # a normalised mesh: the poses' columns divided by the scales, the scales handed in -- powers of two, so the products are exact
    sc = torch.tensor([[2.0, 0.5, 4.0]], device=DEV).expand(J, 3).contiguous()
    sq = lambda p: torch.cat([p[:, :, :3] / sc[:, None, :], p[:, :, 3:]], 2)
    got = bop.errors(ms, jm, wide(sq(pe)), wide(sq(pg)), ss, js, camk[0], scales=sc)
    for k in ("err", "sym_best", "status"):
        assert torch.equal(got[k], want[k]), k
    assert_points(got, c, ref, scale, "4x4 with scales")


# ---- VSD
def vsd_args(c):
    return (meshset(c["meshes"]), up(c["depth"].view(np.int16))) + tuple(up(c[k]) for k in ("camk", "job_img", "job_mesh", "pose_est", "pose_gt", "job_tau")), \
        dict(delta=c["delta"], near=c["near"])


def assert_vsd(out, ref, what=""):
    for k in ("counts", "within"):
        got, want = out[k].cpu().numpy(), ref[k]
        assert got.shape == want.shape and got.dtype == want.dtype == np.int32, (what, k)
        bad = got != want
        assert not bad.any(), "%s %s differ at %s: kernel\n%s\nrestatement\n%s" % (what, k, np.argwhere(bad).tolist(), got, want)
    err = out["err"].cpu().numpy()
    assert err.dtype == np.float32 and np.array_equal(err.view(np.int32), ref["err"].view(np.int32)), (what, err, ref["err"])


VSD_CASES = [("rectangle", 1), ("rectangle", 3), ("rectangle", 10), ("rectangle", 16), ("rectangle", 10, "diag13"), ("rectangle", 10, "reversed"), ("tails",), ("rules",),
             ("tiny_triangles",), ("seven_jobs",)]


@pytest.mark.parametrize("case", VSD_CASES, ids=["-".join(str(x) for x in c) for c in VSD_CASES])
def test_vsd_equals_the_restatement(case):
    """the CPU file's closed-form rectangle cases with 1, 10 and 16 thresholds; occluders, tile tails at 123 x 157 and a table larger
    than the image; the near rule and the guard band in dropped_*, a surface at 70 m never rendered; 20 480 triangles in about one
    tile, for both poses; seven jobs over three frames with a camk each, one with job_img out of range"""
    from tgpose_amd import ops
    c, ref = bc.vsd_reference(*case)
    args, kw = vsd_args(c)
    out = ops.pose_vsd(*args, **kw)
    torch.cuda.synchronize()
    print("%s: counts (%s)\n%s\nwithin\n%s\nerr\n%s" % (case, ", ".join(br.VSD_COUNTS), out["counts"].cpu().numpy(), out["within"].cpu().numpy(),
                                                        out["err"].cpu().numpy()))
    assert_vsd(out, ref, str(case))


def test_vsd_equals_the_logic_on_separately_rendered_frames():
    """an independent path to the same integers: ops.render_depth with one scene per pose (2 J full frames), classified with torch"""
    from tgpose_amd import ops
    c, ref = bc.vsd_reference("seven_jobs")
    (ms, depth, camk, job_img, job_mesh, pe, pg, job_tau), kw = vsd_args(c)
    out = ops.pose_vsd(ms, depth, camk, job_img, job_mesh, pe, pg, job_tau, **kw)
    S, H, W = depth.shape
    keep = torch.nonzero((job_img >= 0) & (job_img < S)).reshape(-1)                                # host knowledge: the test built the jobs
    J = keep.numel()
    assert J == 6
    wide = lambda t: t.view(torch.int16).to(torch.int32) & 0xffff
    ren = [ops.render_depth(ms, torch.arange(J + 1, device=DEV, dtype=torch.int32), job_mesh[keep].contiguous(), torch.ones(J, device=DEV, dtype=torch.uint8),
                            p[keep].contiguous(), camk[job_img[keep].long()].contiguous(), H, W, near=c["near"]) for p in (pe, pg)]
    d_e, d_g, d_o = wide(ren[0]["depth"]), wide(ren[1]["depth"]), wide(depth)[job_img[keep].long()]
    vis = lambda d: (d > 0) & ((d_o == 0) | (d - d_o <= c["delta"]))
    vg = vis(d_g)
    ve = vis(d_e) | (vg & (d_e > 0))
    inter, union = vg & ve, vg | ve
    cols = [d_g > 0, d_e > 0, vg, ve, inter, union]
    want = torch.zeros(7, 8, dtype=torch.int32, device=DEV)
    want[keep] = torch.stack([x.sum((1, 2)) for x in cols] + [ren[1]["dropped"].sum(1), ren[0]["dropped"].sum(1)], 1).to(torch.int32)
    assert torch.equal(out["counts"], want), (out["counts"], want)
    within = torch.zeros(7, job_tau.shape[1], dtype=torch.int32, device=DEV)
    within[keep] = (inter[:, None] & ((d_g - d_e).abs()[:, None] < job_tau[keep][:, :, None, None])).sum((2, 3)).to(torch.int32)
    assert torch.equal(out["within"], within)
    un = want[:, 5:6]
    err = torch.where(un > 0, (un - within).float() / un.clamp(min=1).float(), torch.ones((), device=DEV))
    assert torch.equal(out["err"], err)


def test_vsd_repeat_replay_a_side_stream_and_the_4x4_form():
    from tgpose_amd import ops
    from tgpose_amd.evaluation import bop
    c, ref = bc.vsd_reference("tails")
    args, kw = vsd_args(c)
    a, b = ops.pose_vsd(*args, **kw), ops.pose_vsd(*args, **kw)
    keys = ("counts", "within", "err")
    for k in keys:
        assert torch.equal(a[k], b[k]), k
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.pose_vsd(*args, **kw)
    for v in out.values():
        v.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        s = ops.pose_vsd(*args, **kw)
    side.synchronize()
    for k in keys:
        assert torch.equal(out[k], a[k]) and torch.equal(s[k], a[k]), k
    assert_vsd(out, ref, "graph replay")
    ms, depth, camk, job_img, job_mesh, pe, pg, job_tau = args
    none = ops.pose_vsd(ms, depth, camk, job_img[:0], job_mesh[:0], pe[:0].contiguous(), pg[:0].contiguous(), job_tau[:0].contiguous())
    assert none["counts"].shape == (0, 8) and none["within"].shape == (0, 10) and none["err"].shape == (0, 10)
    # the 4x4 form: job_tau = ceil(float64(tau) * float64(diameter in millimetres))
    J = len(job_img)
    wide = lambda p: torch.cat([p, torch.tensor([0.0, 0, 0, 1], device=DEV).expand(J, 1, 4)], 1)
    v = bop.vsd(ms, depth, camk, c["job_img"], c["job_mesh"], wide(pe), wide(pg), torch.full((J,), 100.0, device=DEV), delta=c["delta"])
    assert np.array_equal(v["job_tau"].cpu().numpy(), np.broadcast_to(np.ceil(bop.TAUS * 100.0).astype(np.int32), (J, 10)))
    direct = ops.pose_vsd(ms, depth, camk, job_img, job_mesh, pe, pg, v["job_tau"], **kw)
    for k in keys:
        assert torch.equal(v[k], direct[k]), k
    assert torch.equal(v["counts"], a["counts"]) and torch.equal(v["within"][:, :2], a["within"][:, :2])   # bop_cases.MM starts 5, 10 too
