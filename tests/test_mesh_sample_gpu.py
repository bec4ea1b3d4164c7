"""Mesh surface sampling on the GPU (csrc/meshsample.hip, ops.mesh_sample / mesh_sample_fps) against the numpy restatement of its
contract (tests/mesh_sample_ref.py) bit for bit, against what the reference itself returned (tests/golden/mesh_sample_ref.npz), and
the surfaces above it: network.point_sample.pc_sample_sphere, datasets.synthetic.mesh_labels / category_tables into the training
loader and one training step."""
import numpy as np
import pytest
import torch

from tests import mesh_sample_ref as mr
from tests.test_mesh_sample_cpu import fixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PASS_FACES = 256 * mr.CHUNK             # the faces one pass of the area kernel's workgroup covers


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")


def _triangle():
    return np.array([[0.0, 0.0, 0.0], [1.0, 0.25, 0.0], [0.25, 1.0, 0.5]], np.float32), np.array([[0, 1, 2]], np.int32)


def _meshes(kind):
    from tgpose_amd.datasets import shapes
    if kind == "small":                 # F = 1, 12, 80
        return [_triangle(), shapes.box((0.3, 0.2, 0.1)), shapes.icosphere(0.5, 1)]
    if kind == "chunks":                # one face past a chunk; more faces than one pass covers (and not a multiple of the chunk)
        v, f = shapes.plane(1.0, 0.7, 33, 1)
        big = shapes.plane(1.3, 0.9, 91, 91)
        assert len(big[1]) > PASS_FACES + mr.CHUNK and len(big[1]) % mr.CHUNK
        return [(v, f[:mr.CHUNK + 1]), big]
    v, f = shapes.box((0.3, 0.2, 0.1))  # degenerate: a zero-area face in the middle; every face of zero area
    mid = f.copy()
    mid[5] = (3, 3, 7)
    return [(v, mid), (v, np.repeat(f[:, :1], 3, axis=1))]


_SETS, _CDF = {}, {}


def _set(kind):
    from tgpose_amd import ops
    if kind not in _SETS:
        meshes = _meshes(kind)
        _SETS[kind] = (meshes, ops.MeshSet(meshes, device=DEV))
        _CDF[kind] = [mr.area_cdf(v, f) for v, f in meshes]
    return _SETS[kind] + (_CDF[kind],)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("draws", ["host", "device"])
@pytest.mark.parametrize("kind", ["small", "chunks", "degenerate"])
def test_kernel_equals_restatement(kind, draws):
    """float64 points and normals, face ids and status, bit for bit; float32 = the float64 rounded once"""
    from tgpose_amd import ops
    meshes, ms, cdfs = _set(kind)
    table = ms.area_cdf().cpu().numpy()
    assert _same(table, np.concatenate(cdfs))
    many = [2, 0, 2, 1, 0] if len(meshes) == 3 else [1, 0, 1, 1, 0]
    seed = 11
    for jobs in ([len(meshes) - 1], many):
        for n in (1, 100, 1024):
            B = len(jobs)
            if draws == "host":
                u = np.random.RandomState(100 * B + n).random_sample((B, n, 3))
                kw = dict(u=torch.from_numpy(u).to(DEV))
            else:
                keys = [2 ** 63 + 5 * b + 1 for b in range(B)]
                u = np.stack([mr.device_uniforms(seed, k, n) for k in keys])
                kw = dict(keys=keys, seed=seed)
            got = ops.mesh_sample(ms, jobs, n, normals=True, dtype=torch.float64, return_face=True, **kw)
            g32 = ops.mesh_sample(ms, jobs, n, normals=True, dtype=torch.float32, **kw)
            pts, face, status = got["points"].cpu().numpy(), got["face"].cpu().numpy(), got["status"].cpu().numpy()
            assert pts.shape == (B, n, 6) and face.shape == (B, n) and face.dtype == np.int32
            for b, m in enumerate(jobs):
                want, wface, wstatus = mr.sample(*meshes[m], u[b], cdf=cdfs[m])
                assert _same(face[b], wface), (kind, draws, jobs, n, b)
                assert _same(pts[b], want), (kind, draws, jobs, n, b)
                assert status[b] == wstatus
            assert _same(g32["points"].cpu().numpy(), pts.astype(np.float32)) and torch.equal(g32["status"], got["status"])
            lean = ops.mesh_sample(ms, jobs, n, dtype=torch.float64, **kw)["points"].cpu().numpy()
            assert _same(lean, pts[..., :3])
    st = ops.mesh_sample(ms, list(range(len(meshes))), 4, keys=list(range(len(meshes))))["status"].tolist()
    assert st == ([0, 1] if kind == "degenerate" else [0] * len(meshes))
    if kind == "degenerate":
        with pytest.raises(Exception, match="positive finite"):
            ops.mesh_sample(ms, [1], 4, keys=[0], check_status=True)
        # the last call's jobs are [1, 0, 1, 1, 0]: every normal of the all-degenerate mesh is NaN, its points are its vertices
        assert np.isnan(pts[0, :, 3:]).all() and np.isfinite(pts[..., :3]).all() and np.isfinite(pts[1]).all()


def test_rows_do_not_depend_on_the_rest_of_the_set():
    from tgpose_amd import ops
    meshes, ms, _ = _set("small")
    alone = ops.MeshSet([meshes[2]], device=DEV)
    u = torch.from_numpy(np.random.RandomState(5).random_sample((1, 300, 3))).to(DEV)
    for kw in (dict(u=u), dict(keys=[77], seed=3)):
        a = ops.mesh_sample(ms, [2], 300, normals=True, dtype=torch.float64, return_face=True, **kw)
        b = ops.mesh_sample(alone, [0], 300, normals=True, dtype=torch.float64, return_face=True, **kw)
        assert torch.equal(a["points"], b["points"]) and torch.equal(a["face"], b["face"])
    on_gpu = ops.mesh_sample(ms, torch.tensor([2, 7], dtype=torch.int32, device=DEV), 8, keys=[1, 2])      # not read back: status 2
    assert on_gpu["status"].tolist() == [0, 2] and (on_gpu["points"][1] == 0).all()


def test_reference_fixture():
    """uniform_sample under np.random.seed(seed) = the reference's output, np.random left where the reference leaves it;
    farthest_point_sampling and sample_points_from_mesh(fps=True) = the reference's"""
    from tgpose_amd.network.point_sample import pc_sample_sphere as ps
    fx = fixture()
    for name in fx["names"]:
        v, f = fx["mesh.%s.verts" % name], fx["mesh.%s.faces" % name]
        for n in fx["sizes"]:
            key = "case.%s.%d" % (name, n)
            np.random.seed(int(fx[key + ".seed"]))
            got = ps.uniform_sample(v, f, int(n), with_normal=True)
            nxt = np.random.random()
            assert _same(got, fx[key + ".out"]), key
            assert nxt == float(fx[key + ".next"]), key
            np.random.seed(int(fx[key + ".seed"]))
            assert _same(ps.uniform_sample(v, f, int(n)), fx[key + ".out"][:, :3]), key
    idx = ps.farthest_point_sampling(fx["fps.points"], 256)
    assert idx.dtype == np.int64 and np.array_equal(idx, fx["fps.index"])
    np.random.seed(int(fx["fps.seed"]))
    got = ps.sample_points_from_mesh((fx["fps.verts"], fx["fps.faces"]), 256, fps=True, ratio=2)
    assert _same(got, fx["fps.points"][fx["fps.index"]])


def test_device_draw_distribution():
    from tgpose_amd import ops
    from tgpose_amd.datasets import shapes
    v, f = shapes.box((0.3, 0.2, 0.1))
    ms = ops.MeshSet([(v, f)], device=DEV)
    got = ops.mesh_sample(ms, [0], mr.DIST_N, keys=[mr.DIST_KEY], seed=mr.DIST_SEED, dtype=torch.float64, return_face=True)
    face, points = got["face"][0].cpu().numpy(), got["points"][0].cpu().numpy()
    chi2, dev, bound = mr.distribution_statistics(v, f, face, points)          # faces and weights both from the kernel's output
    print("chi-square %.3f (11 degrees of freedom), barycentric mean deviation %s, bound %.5f" % (chi2, dev, bound))
    assert chi2 < 31.26
    assert (dev <= bound).all()


def test_mesh_sample_fps_equals_its_composition():
    from tgpose_amd import ops
    from tgpose_amd.datasets import shapes
    ms = ops.MeshSet([shapes.icosphere(0.5, 2), shapes.lathe(shapes.PROFILES["bowl"], 20)], device=DEV)
    for kw in (dict(keys=[4, 9], seed=1), dict(u=torch.from_numpy(np.random.RandomState(2).random_sample((2, 512, 3))).to(DEV))):
        got = ops.mesh_sample_fps(ms, [0, 1], 256, 2, normals=True, **kw)
        dense = ops.mesh_sample(ms, [0, 1], 512, normals=True, **kw)["points"]
        idx = ops.farthest_points(dense[..., :3].contiguous(), 256, init_center=False)
        assert torch.equal(got["index"], idx) and (idx[:, 0] == 0).all()
        for b in range(2):
            assert torch.equal(got["points"][b], dense[b][idx[b].long()])
            assert idx[b].unique().numel() == 256
        assert got["points"].shape == (2, 256, 6) and got["status"].tolist() == [0, 0]


CATS = ("bottle", "bowl", "can", "mug")


def _labelled_scene():
    from tests.render_cases import rot
    from tgpose_amd import ops
    from tgpose_amd.datasets import shapes, synthetic
    from tgpose_amd.evaluation.load_data_eval import CAMERA_INTRINSICS
    meshes = [shapes.lathe(shapes.PROFILES[c], 24) for c in CATS]
    ms = ops.MeshSet(meshes, device=DEV)
    spots = [(-0.14, -0.09, 0.62), (0.13, -0.08, 0.6), (-0.12, 0.1, 0.58), (0.14, 0.09, 0.64)]
    scene = []
    for k, c in enumerate(CATS):
        s = 0.09 + 0.01 * k
        R = rot("x", 200 + 10 * k) @ rot("y", 30 * k) @ rot("z", 8 * k)
        scene.append(dict(mesh=k, inst_id=k + 1, R=R, t=spots[k], s=s, labels=synthetic.mesh_labels(ms, k, c, s)))
    rendered = synthetic.render_scenes(ms, [scene], CAMERA_INTRINSICS, 480, 640)
    return meshes, ms, scene, rendered


def test_labels_close_the_loop():
    """a scene whose labels all come from mesh_labels: the size label is the mesh extent times s; every observed point maps back
    onto the model cloud; category_tables feeds TrainBatches and one training step"""
    from tests.test_gpu_parity import _trainer
    from tgpose_amd.datasets import load_data as ld, synthetic
    from tgpose_amd.evaluater.RT_TDA_Evaluater import SYNSET_NAMES
    meshes, ms, scene, rendered = _labelled_scene()
    items = synthetic.scene_items([scene], rendered)
    assert len(items) == 4 and (rendered["visible"] > 1500).all()
    clouds = ld.train_clouds(items, rng=np.random.RandomState(0), device=DEV)
    for k, (it, (pc, pcl_in)) in enumerate(zip(items, clouds)):
        inst = scene[k]
        assert it["cat_id"] == SYNSET_NAMES.index(CATS[k]) - 1 and it["model_point"].shape == (1024, 3)
        assert it["model_point"].dtype == np.float32 and np.isclose(it["nocs_scale"], inst["s"])
        size = it["fsnet_scale"].astype(np.float64) + it["mean_shape"].astype(np.float64)
        want = ms.extent[k].astype(np.float64) * inst["s"]
        print("%s: size label off by %.3g m" % (CATS[k], np.abs(size - want).max()))
        assert np.abs(size - want).max() <= 1e-6
        model = torch.from_numpy(it["model_point"]).double().to(DEV)
        dense = mr.sample(*meshes[k], np.random.RandomState(40 + k).random_sample((16384, 3)))[0][:, :3]
        r_c = torch.cdist(torch.from_numpy(dense).to(DEV), model).min(1).values.max().item()
        p = pcl_in.double().cpu().numpy()
        q = (p - np.asarray(inst["t"], np.float64)) @ np.asarray(inst["R"], np.float64) / inst["s"]        # R^T (p - t) / s
        d = torch.cdist(torch.from_numpy(q).to(DEV), model).min(1).values.max().item()
        print("%s: coverage radius %.5f model units, farthest observed point %.5f; in metres %.5f against the bound %.5f"
              % (CATS[k], r_c, d, d * inst["s"], r_c * inst["s"] + 1e-3))
        assert pcl_in.shape == (1024, 3) and d * inst["s"] <= r_c * inst["s"] + 1e-3
    again = synthetic.mesh_labels(ms, 2, CATS[2], scene[2]["s"])
    assert np.array_equal(again["model_point"], scene[2]["labels"]["model_point"])          # keyed by (seed, mesh), not by call order
    cat_mesh = [None] * 6
    for k, c in enumerate(CATS):
        cat_mesh[SYNSET_NAMES.index(c) - 1] = k
    tables = synthetic.category_tables(ms, cat_mesh)
    assert [t.shape for t in tables] == [(6, 1024, 3), (6, 2500), (6, 2500)]
    assert np.array_equal(tables[0][3], scene[2]["labels"]["model_point"]) and not tables[0][2].any()
    assert all(np.isfinite(t).all() for t in tables) and tables[1][[0, 1, 3, 5]].any(1).all()
    src = ld.TrainBatches(items, 4, rng=np.random.RandomState(1), gen=torch.Generator().manual_seed(1), device=DEV, prefetch=False,
                          persistence=True, category_tables=tables, shuffle=False)
    db = next(iter(src))
    assert db["points_category"].shape == (4, 1024, 3) and db["pdh1_category"].shape == (4, 2500)
    tr = _trainer(3)
    _, losses = tr.RL_TDA_train_step(db)
    torch.cuda.synchronize()
    vals = [torch.as_tensor(v) for d in losses.values() for v in (d.values() if isinstance(d, dict) else [d])]
    assert vals and all(torch.isfinite(v).all() for v in vals)
