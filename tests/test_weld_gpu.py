"""Indexed meshes from volumes on the device (csrc/weld.hip: ops.tsdf_mesh_indexed, ops.mesh_vertex_normals, ops.MeshSet.from_device,
ops.tsdf_meshset(indexed=True), ops.IcpModels.from_vertices, myEvaluater.scan(indexed=True)) against the NumPy restatement
tests/weld_ref.py: the vertices', faces', masks' and normals' BYTES are equal, and the welded set serves downstream exactly as the
soup set does (DESIGN.md section 3 "Indexed meshes from volumes")."""
import functools

import numpy as np
import pytest
import torch

from tests import tsdf_cases as tc
from tests import tsdf_ref as tr
from tests import weld_ref as wr
from tests.test_weld_cpu import zero_pole

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def shell_volume():
    """G = 16, every voxel seen once; inside iff a coordinate is 0 or G - 1: the surface lies in the first and the last cube row of
    every axis"""
    G = 16
    i = np.arange(G)
    edge = (i == 0) | (i == G - 1)
    inside = edge[:, None, None] | edge[None, :, None] | edge[None, None, :]
    h = (i[:, None, None] * 7 + i[None, :, None] * 13 + i[None, None, :] * 29) % 97
    return np.where(inside, -(200 + h), 150 + h).astype(np.int32), np.ones((G, G, G), np.int32), tr.tsdf_meta([0, 0, 0], [1, 1, 1], G)


def empty_volume():
    G = 16
    return np.zeros((G, G, G), np.int32), np.zeros((G, G, G), np.int32), tr.tsdf_meta([0, 0, 0], [1, 1, 1], G)


def weak():
    return tc.weak_corner()[:3]


CASES = {"sphere16": (lambda: tc.sphere(16), {}), "sphere24": (lambda: tc.sphere(24), {}), "all_patterns": (tc.all_patterns, {}),
         "tail": (tc.tail_volume, {}), "weak_corner": (weak, dict(min_weight=3)), "zero_pole": (zero_pole, {}), "empty": (empty_volume, {}),
         "shell": (shell_volume, {})}


@functools.lru_cache(maxsize=None)
def case(name):
    """(volume, keywords, the restatement's mesh): computed once and shared (do not write to it)"""
    make, kw = CASES[name]
    vol = make()
    return vol, kw, wr.weld(*vol, **kw)


def volumes_of(*vols):
    from tgpose_amd import ops
    G = vols[0][0].shape[0]
    out = ops.TsdfVolumes.from_meta(np.stack([v[2] for v in vols]), G, DEV)
    for m, (vsum, weight, _) in enumerate(vols):
        out.sum[m].copy_(up(vsum)), out.weight[m].copy_(up(weight))
    return out


def device_weld(vol, **kw):
    """the volume as model 1 of two (model 0 holds other numbers: the base offset) -> ops.tsdf_mesh_indexed's dict"""
    from tgpose_amd import ops
    other = (np.full_like(vol[0], -7), np.ones_like(vol[1]), vol[2])
    return ops.tsdf_mesh_indexed(volumes_of(other, vol), 1, **kw)


def same(out, want, what):
    nv, nf = int(out["n_verts"]), int(out["n_faces"])
    assert (nv, nf, int(out["status"])) == (want["n_verts"], want["n_faces"], want["status"]), what
    verts, faces = out["verts"].cpu().numpy(), out["faces"].cpu().numpy()
    assert verts.dtype == F and faces.dtype == np.int32 and out["n_verts"].dtype == torch.int64 and out["status"].dtype == torch.int64
    assert verts[:nv].tobytes() == want["verts"].tobytes(), (what, "verts")
    assert faces[:nf].tobytes() == want["faces"].tobytes(), (what, "faces")
    assert not verts[nv:].any() and not faces[nf:].any(), (what, "rows beyond the counts")
    assert out["mask"].cpu().numpy().tobytes() == want["mask"].tobytes(), (what, "mask")


# ------------------------------------------------------------------------------------------------------------------ welding
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_restatement(name):
    vol, kw, want = case(name)
    out = device_weld(vol, **kw)
    same(out, want, name)
    assert out["verts"].shape == (want["n_verts"], 3) and out["faces"].shape == (want["n_faces"], 3)       # caps None: exact sizes
    if name == "empty":
        assert want["n_verts"] == want["n_faces"] == 0
    else:
        assert want["n_faces"] > 0
    if name == "shell":
        first = want["keys"] // 8 // 256
        assert first.min() == 0 and first.max() == 14 and want["status"] == 0
    if name == "zero_pole":
        assert want["n_verts"] == 1742 and len(np.unique(want["verts"], axis=0)) == 1739
    if name in ("sphere16", "all_patterns"):
        from tgpose_amd import ops
        soup = ops.tsdf_mesh(volumes_of(vol), 0)["verts"]
        assert torch.equal(out["verts"][out["faces"].long()].reshape(-1, 3), soup)                         # the defining property
        again = device_weld(vol, **kw)
        assert all(torch.equal(out[k], again[k]) for k in ("verts", "faces", "mask", "n_verts", "n_faces", "status"))


@pytest.mark.parametrize("vert_cap, face_cap, status", [(2000, 4000, 0), (1742, 3480, 0), (1500, 2000, 3), (1742, 1000, 1), (1, 3480, 2),
                                                         (0, 0, 2)])
def test_caps_read_nothing_back(vert_cap, face_cap, status):
    vol, _, _ = case("sphere16")
    want = wr.weld(*vol, vert_cap=vert_cap, face_cap=face_cap)
    assert want["status"] == status
    out = device_weld(vol, vert_cap=vert_cap, face_cap=face_cap)
    assert out["verts"].shape == (vert_cap, 3) and out["faces"].shape == (face_cap, 3)
    same(out, want, (vert_cap, face_cap))


def test_model_zero_of_one():
    from tgpose_amd import ops
    vol, _, want = case("sphere16")
    same(ops.tsdf_mesh_indexed(volumes_of(vol), 0), want, "model 0")


# ------------------------------------------------------------------------------------------------------------------ clusters, normals
@pytest.mark.parametrize("name", ["sphere16", "all_patterns"])
@pytest.mark.parametrize("c", [1, 2, 4])
def test_clusters_and_normals(name, c):
    from tgpose_amd import ops
    vol, _, _ = case(name)
    want = wr.weld(*vol, cluster=c)
    out = device_weld(vol, cluster=c)
    same(out, want, (name, c))
    if c > 1:
        capped = device_weld(vol, cluster=c, vert_cap=want["mask"].size, face_cap=20000)                   # the capped path underneath
        assert torch.equal(capped["verts"], out["verts"]) and torch.equal(capped["faces"], out["faces"])
    normals = ops.mesh_vertex_normals(out)
    ref = wr.vertex_normals(want["verts"], want["faces"], [0, want["n_verts"]], [0, want["n_faces"]], [wr.volume_scale(vol[2][3])])
    assert out["normal_scale"] == wr.volume_scale(vol[2][3])
    assert normals.cpu().numpy().tobytes() == ref.tobytes()
    assert torch.equal(normals, ops.mesh_vertex_normals(out))                                               # two calls, identical bytes
    if name == "sphere16":
        assert (np.abs(np.linalg.norm(ref.astype(np.float64), axis=1) - 1) < 1e-6).all()


def test_normals_of_a_set():
    """a two-mesh welded set with normals, and a host-made set (a CAD mesh with an unused vertex, and a welded mesh) at the default
    scale"""
    from tests import icp_ref
    from tgpose_amd import ops
    a, b = case("sphere16")[0], case("zero_pole")[0]
    ms = ops.tsdf_meshset(volumes_of(a, b), indexed=True, normals=True)
    wa, wb = case("sphere16")[2], case("zero_pole")[2]
    verts, faces = np.concatenate([wa["verts"], wb["verts"]]), np.concatenate([wa["faces"], wb["faces"]])
    vptr, fptr = [0, wa["n_verts"], len(verts)], [0, wa["n_faces"], len(faces)]
    assert ms.n_verts == [wa["n_verts"], wb["n_verts"]] and ms.n_faces == [wa["n_faces"], wb["n_faces"]]
    assert ms.verts.cpu().numpy().tobytes() == verts.tobytes() and ms.faces.cpu().numpy().tobytes() == faces.tobytes()
    assert ms.vptr.cpu().tolist() == vptr and ms.fptr.cpu().tolist() == fptr
    assert np.array_equal(ms.extent, np.stack([w["verts"].max(0) - w["verts"].min(0) for w in (wa, wb)]))
    ref = wr.vertex_normals(verts, faces, vptr, fptr, [wr.volume_scale(a[2][3]), wr.volume_scale(b[2][3])])
    assert ms.vert_normals.cpu().numpy().tobytes() == ref.tobytes()
    assert torch.equal(ms.vert_normals, ops.mesh_vertex_normals(ms))
    bv, bf = icp_ref.two_boxes()
    bv = np.concatenate([bv, [[9, 9, 9]]]).astype(F)
    cad = ops.MeshSet([(bv, bf), (wa["verts"], wa["faces"])], device=DEV)
    ref = wr.vertex_normals(np.concatenate([bv, wa["verts"]]), np.concatenate([bf, wa["faces"]]), [0, len(bv), len(bv) + wa["n_verts"]],
                            [0, len(bf), len(bf) + wa["n_faces"]], [wr.extent_scale(bv), wr.extent_scale(wa["verts"])])
    got = ops.mesh_vertex_normals(cad).cpu().numpy()
    assert got.tobytes() == ref.tobytes() and got[len(bv) - 1].tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------------------------------ downstream
def turntable_frames():
    """scanned_two_boxes' 12 frames and poses again (it does not keep them)"""
    from tests import icp_ref
    from tgpose_amd import ops
    true = ops.MeshSet([icp_ref.two_boxes()], device=DEV)
    rts = np.stack([tc.pose44(*tc.turntable_pose(k), tc.TURN_SCALE) for k in range(tc.TURN_FRAMES)])
    n = tc.TURN_FRAMES
    camk = up(np.tile(np.array([tc.LOOP_K[0, 0], tc.LOOP_K[1, 1], tc.LOOP_K[0, 2], tc.LOOP_K[1, 2]], dtype=F), (n, 1)))
    ren = ops.render_depth(true, torch.arange(n + 1, dtype=torch.int32, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV),
                           torch.ones(n, dtype=torch.uint8, device=DEV), up(rts[:, :3, :4]), camk, tc.LOOP_H, tc.LOOP_W)
    depth = ren["depth"].cpu().numpy()
    return true, [dict(depth=depth[k]) for k in range(n)], [rts[k][None] for k in range(n)]


def test_indexed_set_equals_soup_set_downstream():
    from tgpose_amd import PoseNet9D, ops
    from tgpose_amd.evaluater.RT_TDA_Evaluater import myEvaluater
    c = tc.scanned_two_boxes(DEV, 32)
    sphere = tc.sphere(32)
    two = ops.TsdfVolumes.from_meta(np.stack([c["volumes"].meta_host[0], sphere[2]]), 32, DEV)
    two.sum[0].copy_(c["volumes"].sum[0]), two.weight[0].copy_(c["volumes"].weight[0])
    two.sum[1].copy_(up(sphere[0])), two.weight[1].copy_(up(sphere[1]))
    soup, welded = ops.tsdf_meshset(two), ops.tsdf_meshset(two, indexed=True)
    assert welded.n_faces == soup.n_faces and all(5 * v < s for v, s in zip(welded.n_verts, soup.n_verts))
    assert welded.vert_normals is None and np.array_equal(welded.extent, soup.extent)
    sv, sf, wv, wf = soup.verts.cpu().numpy(), soup.faces.cpu().numpy(), welded.verts.cpu().numpy(), welded.faces.cpu().numpy()
    for m in range(2):
        sp, wp = np.cumsum([0] + soup.n_verts), np.cumsum([0] + welded.n_verts)
        fp = np.cumsum([0] + soup.n_faces)
        a = sv[sp[m]:sp[m + 1]][sf[fp[m]:fp[m + 1]]]
        b = wv[wp[m]:wp[m + 1]][wf[fp[m]:fp[m + 1]]]
        assert a.tobytes() == b.tobytes()
    # the same triangles in the same order: the renderer, render-and-compare and the sampler return the same bytes
    pose = up(np.stack([c["held_rt"][:3, :4], c["held_rt"][:3, :4]]).astype(F))
    camk = c["held_camk"].repeat(2, 1).contiguous()
    args = (torch.arange(3, dtype=torch.int32, device=DEV), torch.arange(2, dtype=torch.int32, device=DEV),
            torch.ones(2, dtype=torch.uint8, device=DEV), pose, camk, tc.LOOP_H, tc.LOOP_W)
    ra, rb = ops.render_depth(soup, *args, return_face=True), ops.render_depth(welded, *args, return_face=True)
    assert int((ra["depth"][0].view(torch.int16) != 0).sum()) > 1000 and int((ra["depth"][1].view(torch.int16) != 0).sum()) > 1000
    for k in ra:
        assert torch.equal(ra[k].view(torch.int16) if ra[k].dtype == torch.uint16 else ra[k], rb[k].view(torch.int16) if rb[k].dtype == torch.uint16 else rb[k]), k
    jobs = (c["held_depth"].view(torch.int16).repeat(2, 1, 1).contiguous(), camk, torch.arange(2, dtype=torch.int32, device=DEV),
            torch.arange(2, dtype=torch.int32, device=DEV), pose)
    va, vb = ops.pose_verify(soup, *jobs, tau=tc.LOOP_TAU), ops.pose_verify(welded, *jobs, tau=tc.LOOP_TAU)
    assert torch.equal(va["counts"], vb["counts"]) and torch.equal(va["score"], vb["score"]) and float(va["score"][0]) > 0.8
    u = up(np.random.RandomState(3).rand(2, 256, 3))
    pa, pb = ops.mesh_sample(soup, [0, 1], 256, u=u, normals=True), ops.mesh_sample(welded, [0, 1], 256, u=u, normals=True)
    assert torch.equal(pa["points"], pb["points"]) and int(pa["status"].abs().sum()) == 0
    # myEvaluater.scan(indexed=True) returns that set
    true, frames, rts = turntable_frames()
    ev = myEvaluater(PoseNet9D().to(DEV).eval(), sampler="device")
    vol, got = ev.scan(frames, rts, tc.LOOP_K, volumes=ops.TsdfVolumes.from_meshset(true, 32), indexed=True)
    assert torch.equal(vol.sum, c["volumes"].sum) and torch.equal(vol.weight, c["volumes"].weight)
    assert got.n_verts == welded.n_verts[:1] and got.n_faces == welded.n_faces[:1]
    assert torch.equal(got.verts, welded.verts[:got.n_verts[0]]) and torch.equal(got.faces, welded.faces[:got.n_faces[0]])


def test_refusals():
    from tgpose_amd import ops
    vol = volumes_of(case("sphere16")[0], case("empty")[0])
    for kw in (dict(cluster=3), dict(cluster=0), dict(cluster=16), dict(face_cap=10), dict(vert_cap=10), dict(face_cap=-1, vert_cap=10),
               dict(face_cap=10, vert_cap=-1), dict(face_cap=ops.TSDF_MAX_FACES + 1, vert_cap=10), dict(face_cap=10, vert_cap=ops.WELD_MAX_VERTS + 1),
               dict(face_cap=10.0, vert_cap=10), dict(min_weight=0)):
        with pytest.raises(ValueError):
            ops.tsdf_mesh_indexed(vol, 0, **kw)
    with pytest.raises(ValueError):
        ops.tsdf_mesh_indexed(vol, 2)
    with pytest.raises(TypeError):
        ops.tsdf_mesh_indexed(None, 0)
    with pytest.raises(ValueError, match="cluster"):
        ops.tsdf_meshset(vol, indexed=True, cluster=3)
    with pytest.raises(ValueError, match="indexed"):
        ops.tsdf_meshset(vol, cluster=2)
    with pytest.raises(ValueError, match="volume 1 has no face"):
        ops.tsdf_meshset(vol, indexed=True)
    out = ops.tsdf_mesh_indexed(vol, 0)
    V, Fc = out["verts"].shape[0], out["faces"].shape[0]
    with pytest.raises(ValueError, match="mesh 1 is empty"):
        ops.MeshSet.from_device(out["verts"], out["faces"], [V, 0], [Fc, 0])
    with pytest.raises(ValueError, match="mesh 0 is empty"):
        ops.MeshSet.from_device(out["verts"], out["faces"][:0], [V], [0])
    with pytest.raises(ValueError, match="add up"):
        ops.MeshSet.from_device(out["verts"], out["faces"], [V - 1], [Fc])
    with pytest.raises(ValueError, match="outside its"):
        ops.MeshSet.from_device(out["verts"][:100].contiguous(), out["faces"], [100], [Fc])
    with pytest.raises(ValueError, match="the cap is"):
        ops.MeshSet.from_device(out["verts"], torch.zeros(ops.render_max_faces(), 3, dtype=torch.int32, device=DEV), [V], [ops.render_max_faces()])
    with pytest.raises(TypeError):
        ops.MeshSet.from_device(out["verts"].double(), out["faces"], [V], [Fc])
    ms = ops.MeshSet.from_device(out["verts"], out["faces"], [V], [Fc])
    with pytest.raises(ValueError, match="no vert_normals"):
        ops.IcpModels.from_vertices(ms, [0], 64)
    ms.vert_normals = ops.mesh_vertex_normals(ms)
    with pytest.raises(ValueError, match="fewer than n"):
        ops.IcpModels.from_vertices(ms, [0], V + 1)
    with pytest.raises(ValueError, match="outside the set"):
        ops.IcpModels.from_vertices(ms, [1], 64)
    models = ops.IcpModels.from_vertices(ms, [0, 0], 64)
    pn = models.points_normals.cpu().numpy()
    assert pn.shape == (2, 64, 6) and pn[0].tobytes() == pn[1].tobytes()
    rows = {r.tobytes() for r in np.concatenate([out["verts"].cpu().numpy(), ms.vert_normals.cpu().numpy()], 1)}
    assert all(r.tobytes() in rows for r in pn[0]) and len({r.tobytes() for r in pn[0]}) == 64            # 64 of the mesh's own vertices
    with pytest.raises(TypeError):
        ops.mesh_vertex_normals(out["verts"])
    with pytest.raises(ValueError, match="scale"):
        ops.mesh_vertex_normals(ms, scale=[1.0, 2.0])


# ------------------------------------------------------------------------------------------------------------------ the chain
@pytest.mark.parametrize("c", [1, 2])
def test_vertex_model_registers_the_held_out_view(c):
    """ICP against the scanned model's own vertices (IcpModels.from_vertices: 1024 of the welded model's 12846 with their vertex
    normals, 512 of the 877 of the model decimated by 2) from 5 degrees and 10 mm off on the held-out view at G = 32: within the
    true mesh's own translation error plus c voxel edges, and within the angle c voxels subtend at the object's radius --
    tests/test_tsdf_gpu.py's bound for a scanned model, c voxels for a model decimated by c."""
    from tests import icp_ref
    from tgpose_amd import ops, pose
    s = tc.scanned_two_boxes(DEV, 32)
    R_true, t_true = s["held_pose"]
    start = tc.pose44(icp_ref.rot([1, 2, -1], 5.0) @ R_true, t_true + 0.010 * np.array([2.0, -1.0, 2.0]) / 3.0, tc.TURN_SCALE)
    ms = ops.tsdf_meshset(s["volumes"], indexed=True, cluster=c, normals=True)
    n = 1024 // c
    assert ms.n_verts[0] >= n
    err = {}
    for name, models in (("true", ops.IcpModels.from_meshset(s["true"], [0], 1024)), ("scanned", ops.IcpModels.from_vertices(ms, [0], n))):
        got, info, rmse = pose.refine_poses(models, torch.zeros(1, dtype=torch.int32, device=DEV), up(s["cloud"][None]), up(start[None]), 0.02,
                                            mode="plane", iters=50)
        deg, mm = tc._pose_error(got[0].cpu().numpy(), s["held_pose"])
        err[name] = dict(rot_deg=float(deg), trans_mm=float(mm), icp_status=int(info[0, 0]))
    voxel_mm = 1000 * s["voxel_m"]
    angle = float(np.rad2deg(np.arctan(c * s["voxel_m"] / s["radius_m"])))
    print(dict(c=c, verts=ms.n_verts[0], faces=ms.n_faces[0], voxel_mm=voxel_mm, angle_deg=angle, **err))
    assert err["true"]["icp_status"] == 0 and err["scanned"]["icp_status"] == 0
    assert err["scanned"]["trans_mm"] <= err["true"]["trans_mm"] + c * voxel_mm, err
    assert err["scanned"]["rot_deg"] <= angle, err
