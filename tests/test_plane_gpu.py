"""The supporting plane on the GPU (csrc/plane.hip) against the NumPy restatement of its contract (tests/plane_ref.py).

The hypotheses, their counts, the best index, the info words and the cut are compared bit for bit.  After a refit the plane may differ
from the restatement's by the float64 summation order and the eigen-solver: 1e-6 per component, the bound tests/test_icp_gpu.py uses
for the same reason; the inlier count after a further refit may then differ by at most the pixels whose distance lies within 1e-6 m of
the tolerance, which on these frames are at most 0.1 % of the inliers (asserted on the restatement alone; measured: none).

Frames (tests/plane_cases.py): five of 37 x 53 -- scalar loads, a tail group, less than one scoring tile, 70 hypotheses; a tilted
plane with an object, holes and a 65535; an empty frame; two valid pixels; two planes that tie; a half-empty noisy plane -- and the
rendered table scene at 240 x 320 with 256 hypotheses (16-byte loads, 38 tiles)."""
import os

import numpy as np
import pytest
import torch

from tests import plane_cases as pc
from tests import plane_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plane_utils_ref.npz")
_S = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")


def up(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(DEV)


def cases():
    """name -> dict(frames (S,H,W) uint16, camk, keys, seed, hyp) and, per refine_iters, the restatement's result per frame"""
    if not _S:
        _S["small"] = dict(frames=pc.small_frames(), camk=pc.SMALL_CAMK, keys=pc.SMALL_KEYS, seed=0, hyp=pc.SMALL_HYPOTHESES, ref={})
        _S["scene"] = dict(frames=pc.rendered(0)[None], camk=pc.CAMK, keys=(0,), seed=pc.SEED, hyp=pc.HYPOTHESES, ref={})
    return _S


def ref(case, iters):
    c = cases()[case]
    if iters not in c["ref"]:
        c["ref"][iters] = [plane_ref.fit(f, c["camk"], key=k, seed=c["seed"], hypotheses_n=c["hyp"], tol=pc.TOL, refine_iters=iters, min_inliers=100)
                           for f, k in zip(c["frames"], c["keys"])]
    return c["ref"][iters]


def fit(case, iters, frames=None, keys=None, depth=None):
    from tgpose_amd import ops
    c = cases()[case]
    frames = c["frames"] if frames is None else frames
    keys = c["keys"] if keys is None else keys
    camk = up(np.tile(np.asarray(c["camk"], np.float32), (len(frames), 1)))
    depth = up(frames) if depth is None else depth
    plane, info, counts = ops.plane_fit(depth, camk, tol=pc.TOL, hypotheses=c["hyp"], seed=c["seed"], keys=list(keys), refine_iters=iters,
                                        min_inliers=100, return_counts=True)
    return plane.cpu().numpy(), info.cpu().numpy(), counts.cpu().numpy(), (depth, camk, plane, info)


@pytest.mark.parametrize("case", ["small", "scene"])
def test_counts_best_and_plane_are_bit_exact(case):
    plane, info, counts, _ = fit(case, 0)
    want = ref(case, 0)
    for s, w in enumerate(want):
        assert np.array_equal(counts[s], w["counts"]), (s, np.nonzero(counts[s] != w["counts"])[0][:8])
        assert int(np.argmax(counts[s])) == w["best"]
        assert info[s].tolist() == w["info"].tolist(), (s, info[s], w["info"])
        assert np.array_equal(plane[s].view(np.int32), w["plane"].view(np.int32)), (s, plane[s], w["plane"])
        print("%s frame %d: status %d, best %d with %d of %d valid pixels, %d void hypotheses" % (case, s, info[s, 0], w["best"], info[s, 1], info[s, 3],
                                                                                              int(np.isnan(w["hyp"][:, 0]).sum())))
    if case == "small":
        assert [w["info"][0] for w in want] == [0, 1, 1, 0, 0] and want[2]["info"][3] == 2
        assert (cases()["small"]["frames"][0] == 65535).sum() == 1
        top = np.nonzero(want[3]["counts"] == 962)[0]                              # the two planes tie; both are hit; the first index wins
        assert want[3]["best"] == top[0] and len({float(d) for d in want[3]["hyp"][top, 3]}) == 2


@pytest.mark.parametrize("case", ["small", "scene"])
def test_refit(case):
    for iters in (1, 2):
        plane, info, counts, _ = fit(case, iters)
        want = ref(case, iters)
        for s, w in enumerate(want):
            assert info[s, 0] == w["info"][0] and info[s, 1] == w["info"][1] and info[s, 3] == w["info"][3], (s, info[s], w["info"])
            if w["info"][0] != 0:
                assert not plane[s].any() and info[s, 2] == 0
                continue
            assert all(n <= 0.001 * w["info"][2] for n in w["near"]), (s, w["near"])     # on the restatement alone
            diff = float(np.abs(plane[s].astype(np.float64) - w["plane"].astype(np.float64)).max())
            print("%s frame %d, %d refit(s): plane %s, largest difference to the restatement %.3e; inliers %d (restatement %d, %d pixels within "
                  "1e-6 m of the tolerance)" % (case, s, iters, plane[s], diff, info[s, 2], w["info"][2], w["near"][0]))
            if iters == 1 or w["near"][0] == 0:
                assert diff <= 1e-6, (s, iters, diff)
            assert abs(int(info[s, 2]) - int(w["info"][2])) <= w["near"][0], (s, iters)     # pixels within 1e-6 m of tol under the first refit
            assert plane[s, 3] >= 0 and abs(float(np.linalg.norm(plane[s, :3].astype(np.float64))) - 1.0) < 1e-6


def test_a_frame_gives_the_same_bits_alone_in_a_batch_and_again():
    c = cases()["small"]
    plane, info, counts, _ = fit("small", 2)
    again = fit("small", 2)
    assert all(np.array_equal(a, b) for a, b in zip((plane.view(np.int32), info, counts), (again[0].view(np.int32), again[1], again[2])))
    for s in range(len(c["frames"])):
        p1, i1, c1, _ = fit("small", 2, frames=c["frames"][s:s + 1], keys=c["keys"][s:s + 1])
        assert np.array_equal(p1[0].view(np.int32), plane[s].view(np.int32)) and np.array_equal(i1[0], info[s]) and np.array_equal(c1[0], counts[s]), s
    # the 16-byte loads and the scalar loads of the same frame: a base that is 2 bytes off
    sc = cases()["scene"]
    aligned = fit("scene", 2)
    buf = torch.zeros(pc.H * pc.W + 8, dtype=torch.int16, device=DEV)
    buf[1:1 + pc.H * pc.W] = up(sc["frames"]).reshape(-1)
    off = fit("scene", 2, depth=buf[1:1 + pc.H * pc.W].view(1, pc.H, pc.W))
    assert off[3][0].data_ptr() % 16 == 2
    assert all(np.array_equal(a, b) for a, b in zip((aligned[0].view(np.int32), aligned[1], aligned[2]), (off[0].view(np.int32), off[1], off[2])))


@pytest.mark.parametrize("case", ["small", "scene"])
@pytest.mark.parametrize("margin", [0.006, 0.0])
def test_cut_is_bit_exact(case, margin):
    from tgpose_amd import ops
    c = cases()[case]
    plane, info, _, (depth, camk, plane_d, info_d) = fit(case, 2)
    out, side = ops.plane_cut(depth, plane_d, info_d, camk, margin, return_side=True)
    only = ops.plane_cut(depth, plane_d, info_d, camk, margin)
    assert out.dtype == depth.dtype and torch.equal(out, only)
    out, side = out.cpu().numpy().view(np.uint16), side.cpu().numpy()
    for s, f in enumerate(c["frames"]):
        w_out, w_side = plane_ref.cut(f, plane[s], int(info[s, 0]), c["camk"], margin)
        assert np.array_equal(out[s], w_out) and np.array_equal(side[s], w_side), s
        if info[s, 0] != 0:
            assert np.array_equal(out[s], f)                                        # no plane: copied through
        print("%s frame %d margin %.3f: %d of %d valid pixels left; side counts %s" % (case, s, margin, (w_out > 0).sum(), (f > 0).sum(),
                                                                                    np.bincount(w_side.ravel(), minlength=4).tolist()))
    if case == "small":
        assert info[:, 0].tolist() == [0, 1, 1, 0, 0]
    with pytest.raises(ValueError):
        ops.plane_cut(depth, plane_d, info_d, camk, -0.001)
    with pytest.raises(ValueError):
        ops.plane_fit(depth, camk, hypotheses=0)


def test_check_status_names_the_frame():
    from tgpose_amd import _lib, ops
    info = fit("small", 0)[3][3]
    with pytest.raises(_lib.TgpError, match="frame 1"):
        ops.plane_check_status(info)
    ops.plane_check_status(info[:1])


def test_regression_against_the_reference():
    from tgpose_amd import ops
    from tgpose_amd.tools import plane_utils
    g = np.load(GOLDEN)
    P, Wt = up(g["pc"]), up(g["pc_w"])
    margin = lambda key: max(float(np.abs(g["f32." + key].astype(np.float64) - g["f64." + key]).max()), 1e-6)

    def check(key, got, want_shape):
        got = got.cpu().numpy()
        assert got.shape == want_shape == g["f64." + key].shape[-len(want_shape):], (key, got.shape)
        return got.astype(np.float64)
    normal, dn, p2 = plane_utils.get_plane_in_batch(P, Wt)
    for name, val in (("normal", normal), ("dn", dn), ("p2plane", p2)):
        key = "batch." + name
        assert val.shape == g["f64." + key].shape and val.dtype == torch.float32
        err = float(np.abs(val.cpu().numpy().astype(np.float64) - g["f64." + key]).max())
        print("%s: error %.3e against the reference in float64; the reference's own float32 error %.3e" % (key, err, margin(key)))
        assert err <= margin(key), key
    for i in range(2):
        for j in range(3):
            normal, dn, p2 = plane_utils.get_plane(P[i, j], Wt[i, j])
            X = plane_utils.get_plane_parameter(P[i, j], Wt[i, j])
            for name, val, shape in (("normal", normal, (3,)), ("dn", dn, (3,)), ("p2plane", p2, (1,)), ("X", X, (3, 1))):
                key = "single." + name
                err = float(np.abs(check(key, val, shape) - g["f64." + key][i, j]).max())
                assert err <= margin(key), (key, i, j, err)
    # against the restatement, and the singular systems: NaN, no fault
    X, normal, dn, p2 = (x.cpu().numpy() for x in ops.plane_lsq(P.reshape(6, 64, 3), Wt.reshape(6, 64)))
    for b in range(6):
        w = plane_ref.lsq(g["pc"].reshape(6, 64, 3)[b], g["pc_w"].reshape(6, 64)[b])
        for got, want in zip((X[b], normal[b], dn[b], p2[b]), w):
            assert np.abs(got.astype(np.float64) - np.asarray(want, np.float64)).max() <= 1e-6
    for n in (1, 2):
        out = ops.plane_lsq(P.reshape(6, 64, 3)[:, :n].contiguous(), Wt.reshape(6, 64)[:, :n].contiguous())
        assert all(torch.isnan(x).all() for x in out), n
    line = np.stack([np.linspace(-0.1, 0.1, 300), np.linspace(-0.1, 0.1, 300) * 0.5, np.linspace(0, 1, 300)], 1).astype(np.float32)
    out = ops.plane_lsq(up(line[None]), torch.ones(1, 300, device=DEV))                # more points than one workgroup's threads
    assert all(torch.isnan(x).all() for x in out)
    ok = ops.plane_lsq(up(np.concatenate([g["pc"].reshape(1, -1, 3)] * 2, 1)), up(np.concatenate([g["pc_w"].reshape(1, -1)] * 2, 1)))
    assert all(torch.isfinite(x).all() for x in ok)                                    # 768 points: every thread takes three
