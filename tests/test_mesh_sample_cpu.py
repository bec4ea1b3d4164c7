"""CPU tests of mesh surface sampling (csrc/meshsample.hip, ops.mesh_sample, network/point_sample/pc_sample_sphere.py,
datasets/load_data.get_fs_net_scale / get_sym_info): the NumPy restatement of the contract against what the reference itself
returned (tests/golden/mesh_sample_ref.npz, recorded by tests/golden/make_mesh_sample_golden.py), the new entry points'
constants and argument errors (which return before any launch), the label functions and the OBJ reader."""
import ctypes
import os

import numpy as np
import pytest

from tests import mesh_sample_ref as mr
from tests.util import ROOT

_FX = {}


def fixture():
    if not _FX:
        path = os.path.join(ROOT, "tests", "golden", "mesh_sample_ref.npz")
        assert os.path.exists(path), "tests/golden/mesh_sample_ref.npz is missing: run tests/golden/make_mesh_sample_golden.py"
        _FX.update(np.load(path))
    return _FX


def cases():
    fx = fixture()
    for name in fx["names"]:
        for n in fx["sizes"]:
            yield str(name), int(n)


def test_restatement_equals_the_reference_bit_for_bit():
    fx = fixture()
    count = 0
    for name, n in cases():
        v, f = fx["mesh.%s.verts" % name], fx["mesh.%s.faces" % name]
        u = np.random.RandomState(int(fx["case.%s.%d.seed" % (name, n)])).random_sample((n, 3))
        got, face, status = mr.sample(v, f, u)
        want = fx["case.%s.%d.out" % (name, n)]
        assert status == 0 and got.shape == want.shape == (n, 6)
        assert np.array_equal(got, want), (name, n)
        tri = v.astype(np.float64)[f]
        serial = np.cumsum(0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1))
        assert np.array_equal(face, np.searchsorted(serial, u[:, 0] * serial[-1])), (name, n)
        count += 1
    assert count == 15


def test_chunked_sum_is_the_stated_order():
    """the restated table against a plain loop over the header's definition, at sizes around the chunk"""
    rng = np.random.RandomState(1)
    for F in (1, 63, 64, 65, 128, 129, 200):
        v = rng.rand(3 * F, 3).astype(np.float32)
        f = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
        area = 0.5 * mr.cross_norm(mr.corners(v, f))[1]
        want, off = np.zeros(F), 0.0
        for c0 in range(0, F, mr.CHUNK):
            s = 0.0
            for k in range(c0, min(c0 + mr.CHUNK, F)):
                s = s + area[k]
                want[k] = off + s
            off = off + s
        assert np.array_equal(mr.area_cdf(v, f), want), F


def test_new_symbols_are_declared_bound_and_exported():
    """the ABI number and the mesh constants against the NumPy restatement's; tests/test_abi_cpu.py holds every symbol, type and value
    against the header"""
    from tgpose_amd import _lib
    assert _lib.lib().tgp_version() == _lib.ABI_VERSION == 9
    assert {k: v for k, v in _lib.CONSTANTS.items() if k.startswith("MESH_")} == {"MESH_SITE": 8, "MESH_AREA_CHUNK": 64}
    assert _lib.MESH_SITE == mr.SITE == 8 and _lib.MESH_AREA_CHUNK == mr.CHUNK == 64
    assert _lib.MESH_SITE == _lib.SITE_SHUFFLE + 1                              # the next free draw site


def _args(**kw):
    from tgpose_amd import _lib
    a = _lib.MeshSampleArgs()
    for k in ("verts", "faces", "vptr", "fptr", "cdf", "job_mesh", "out", "status", "u"):
        setattr(a, k, 8)                    # non-null pointers that are never followed: every call below is refused
    a.M, a.n_verts, a.n_faces, a.B, a.n = 1, 3, 1, 1, 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_argument_errors_return_before_any_launch():
    from tgpose_amd import _lib
    h = _lib.lib()
    one = ctypes.c_void_p(8)
    assert h.tgp_mesh_area_cdf(None, one, one, one, 1, 3, 1, one, None) == -1
    assert h.tgp_mesh_area_cdf(one, one, one, one, 1, 3, 1, None, None) == -1
    assert h.tgp_mesh_area_cdf(one, one, one, one, 0, 3, 1, one, None) == -1
    assert h.tgp_mesh_area_cdf(one, one, one, one, 1, 3, 0, one, None) == -1
    assert h.tgp_mesh_sample(None, None) == -1
    for k in ("verts", "faces", "vptr", "fptr", "cdf", "job_mesh", "out", "status"):
        assert h.tgp_mesh_sample(_args(**{k: None}), None) == -1, k
    assert h.tgp_mesh_sample(_args(n=0), None) == -1 and h.tgp_mesh_sample(_args(B=0), None) == -1
    assert h.tgp_mesh_sample(_args(M=0), None) == -1
    assert h.tgp_mesh_sample(_args(keys=8), None) == -1                         # both u and keys
    assert h.tgp_mesh_sample(_args(u=None), None) == -1                         # neither
    assert h.tgp_mesh_sample(_args(B=65536), None) == -2


def test_python_argument_errors():
    import torch
    from tgpose_amd import ops
    from tgpose_amd.datasets import shapes
    ms = ops.MeshSet([shapes.box(1.0)], device="cpu")
    with pytest.raises(TypeError, match="MeshSet"):
        ops.mesh_sample(None, [0], 4, keys=[0])
    with pytest.raises(ValueError, match="outside the set"):
        ops.mesh_sample(ms, [1], 4, keys=[0])
    with pytest.raises(ValueError, match="outside the set"):
        ops.mesh_sample(ms, [-1], 4, keys=[0])
    with pytest.raises(TypeError, match="integer"):
        ops.mesh_sample(ms, [0.5], 4, keys=[0])
    with pytest.raises(ValueError, match="at least one job"):
        ops.mesh_sample(ms, [], 4, keys=[])
    with pytest.raises(ValueError, match="n must be"):
        ops.mesh_sample(ms, [0], 0, keys=[0])
    with pytest.raises(ValueError, match="exactly one"):
        ops.mesh_sample(ms, [0], 4)
    with pytest.raises(ValueError, match="exactly one"):
        ops.mesh_sample(ms, [0], 4, u=torch.zeros(1, 4, 3, dtype=torch.float64), keys=[0])
    with pytest.raises(TypeError, match="float64 GPU"):
        ops.mesh_sample(ms, [0], 4, u=torch.zeros(1, 4, 3, dtype=torch.float64))
    with pytest.raises(TypeError, match="dtype"):
        ops.mesh_sample(ms, [0], 4, keys=[0], dtype=torch.float16)
    with pytest.raises(ValueError, match=r"keys must be \(B\)"):
        ops.mesh_sample(ms, [0], 4, keys=[0, 1])
    with pytest.raises(ValueError, match="above the cap"):
        ops.mesh_sample_fps(ms, [0], ops.fps_max_points(), 2, keys=[0])
    from tgpose_amd.datasets import synthetic
    with pytest.raises(ValueError, match="outside the set"):
        synthetic.mesh_labels(ms, 3, "mug", 0.1)
    with pytest.raises(ValueError, match="no category"):
        synthetic.category_tables(ms, [None, -1])


def test_label_functions_return_the_reference_values():
    from tgpose_amd.datasets import load_data as ld
    fx = fixture()
    model, s = fx["labels.model"], float(fx["labels.nocs_scale"])
    assert [str(c) for c in fx["labels.names"]] == ["bottle", "bowl", "camera", "can", "laptop", "mug"]
    for c in fx["labels.names"]:
        c = str(c)
        res, mean = ld.get_fs_net_scale(c, model, s)
        assert np.array_equal(res, fx["labels.%s.fsnet_scale" % c]) and res.dtype == fx["labels.%s.fsnet_scale" % c].dtype, c
        assert np.array_equal(mean, fx["labels.%s.mean_shape" % c]), c
        sym = ld.get_sym_info(c)
        assert np.array_equal(sym, fx["labels.%s.sym" % c]) and sym.dtype == np.int32, c
    assert np.array_equal(ld.get_sym_info("mug", mug_handle=0), fx["labels.mug.sym_no_handle"])
    assert np.array_equal(ld.get_sym_info("teapot"), fx["labels.unknown.sym"])
    with pytest.raises(NotImplementedError):
        ld.get_fs_net_scale("teapot", model, s)


def test_load_obj(tmp_path):
    from tgpose_amd.network.point_sample.pc_sample_sphere import load_obj
    p = tmp_path / "m.obj"
    p.write_text("# a comment\nmtllib x.mtl\nv 0 0 0\nv 1.5 0 0\nv 0 2e-1 0\nvn 0 0 1\nvt 0 0\nv 0 0 -3\n\n"
                 "f 1 2 3\nf 1/1/1 3/2/1 4/3/1\nf 2//1 3//1 4//1\n")
    v, f = load_obj(str(p))
    assert v.dtype == np.float64 and np.array_equal(v, [[0, 0, 0], [1.5, 0, 0], [0, 0.2, 0], [0, 0, -3]])
    assert np.array_equal(f, [[0, 1, 2], [0, 2, 3], [1, 2, 3]])


def test_distribution_seed_passes_on_the_restatement():
    """the statistic test_mesh_sample_gpu.test_device_draw_distribution asserts on the kernel's output, on the restatement of the
    same draws: the kernel equals the restatement bit for bit, so the GPU test is decided here"""
    from tgpose_amd.datasets import shapes
    v, f = shapes.box((0.3, 0.2, 0.1))
    chi2, dev, bound = mr.distribution_statistics(v, f, *mr.distribution_draws(v, f))
    assert chi2 < 31.26 and (dev <= bound).all(), (chi2, dev, bound)
