"""Host-side checks of the point-gradient entry points: they refuse bad arguments before any launch (tests/test_abi_cpu.py holds
their symbols and argument types against the header)."""
import os

import torch

from tgpose_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def test_bad_arguments_return_negative_without_launch():
    """null pointers and bad strides: TGP_EINVAL; valid-looking pointers with an unsupported shape: TGP_EUNSUPPORTED -- both before any
    launch (the pointers below are never dereferenced: every check runs on the host first)"""
    import ctypes
    lib = _lib.lib()
    assert lib.tgp_version() == _lib.ABI_VERSION == 9
    P = ctypes.c_void_p(256)                    # a non-null dummy: the calls must return before anything reads it
    assert lib.tgp_gconv_dirgrad(None, None, None, 0, None, None, 0, None, 1, 1, 1, 7, 128, None, None) == -1
    assert lib.tgp_gconv_dirgrad(P, P, None, 0, P, P, 64, None, 1, 1, 20, 7, 128, P, None) == -1           # ldg < C
    assert lib.tgp_gconv_dirgrad(P, P, P, 512, P, P, 128, None, 1, 1, 20, 7, 128, P, None) == -1           # ldp < 8C
    assert lib.tgp_gconv_dirgrad(P, P, None, 0, P, P, 128, P, 1, 1, 20, 7, 128, P, None) == -1             # slots without proj
    assert lib.tgp_gconv_dirgrad(P, P, None, 0, P, P, 128, None, 1, 1, 20, 6, 128, P, None) == -2          # S != 7
    assert lib.tgp_gconv_dirgrad(P, P, None, 0, P, P, 128, None, 1, 1, 65, 7, 128, P, None) == -2          # k > 64
    assert lib.tgp_gconv_dirgrad(P, P, None, 0, P, P, 2048, None, 1, 1, 20, 7, 2048, P, None) == -2        # LDS beyond 60 KB
    assert lib.tgp_dirs_to_xyz(None, None, None, None, 0, None, None, 1, 1, 1, None, 0, None) == -1
    assert lib.tgp_dirs_to_xyz(P, P, P, P, 0, P, None, 1, 100, 65, P, 0, None) == -2                        # (i << 6) | j lists, k > 64
    assert lib.tgp_neighbor_dirs(None, None, 1, 1, 1, None, None, None) == -1
    assert lib.tgp_neighbor_dirs(P, P, 0, 1, 1, P, None, None) == -1
    assert lib.tgp_center_bwd(None, None, 1, 1, None, None) == -1
    assert lib.tgp_center_bwd(P, None, 1, 0, P, None) == -1
    assert lib.tgp_bn_eval_bwd(*([None, 0, None, 0, 1, 1, None, None, 1e-5, None, None, 0, 0.0, None, 0, None, None, None, None])) == -1
    assert lib.tgp_bn_eval_bwd(*([P, 8, P, 8, 4, 8, P, P, 1e-5, P, P, 2, 0.0, P, 8, P, P, P, None])) == -1    # act 2
    assert lib.tgp_bn_eval_bwd_pooled(*([None, 0, None, 0, None, 0, 1, 1, 1, None, None, 1e-5, None, None, 0, 0.0, None, 0, None, None,
                                         None, None])) == -1
    assert lib.tgp_bn_eval_bwd_pooled(*([P, 4, P, 8, P, 8, 2, 4, 8, P, P, 1e-5, P, P, 0, 0.0, P, 8, P, P, P, None])) == -1   # ldp < C
    assert lib.tgp_bn_eval_workspace_floats(128) == 64 * 2 * 128


GROUPS = {"rot": ["p_green_R", "p_red_R", "f_green_R", "f_red_R"], "ts": ["Pred_T", "Pred_s"], "recon": ["recon"], "h": ["h1", "h2"],
          "feat": ["feat"], "fglob": ["feat_global"]}


def _group_weights(out, keys, seed):
    """tests/golden/make_xyz_grad_golden.py's xyz_grad_weights"""
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(tuple(out[k].shape), generator=g) for k in keys}


def test_fixture_matches_oracle_autograd_per_output_group():
    """tests/golden/xyz_grad.npz (the reference's own points.grad) against the oracle's autograd in fp64 on the fixture's graphs and
    subsample: every output group of eval mode, training mode and the duplicated cloud (per point, copies included).  The bar is the
    GPU tests' (3e-2 of the norm): fp32 near-ties of the reference that fp64 resolves the other way stay inside it."""
    import numpy as np
    from oracle import posenet_ref
    from tgpose_amd import seeded_state_dict
    z = np.load(os.path.join(ROOT, "tests", "golden", "xyz_grad.npz"))
    P = {k: (v.double() if v.is_floating_point() else v) for k, v in seeded_state_dict(int(z["weight_seed"])).items()}
    cases = (("eval", 0, ["rot", "ts"]), ("dup", 0, ["rot", "ts"]), ("train", 1, ["feat", "fglob", "h", "recon", "rot", "ts"]))
    for tag, train, grps in cases:
        pts = torch.from_numpy(z[tag + ".points"]).double().requires_grad_(True)
        obj = torch.from_numpy(z[tag + ".obj_id"])
        idx = {k[len(tag) + 5:]: torch.from_numpy(z[k].astype(np.int64)) for k in z.files if k.startswith(tag + ".idx.")}
        s = tuple(torch.from_numpy(z["%s.sample_idx_%d" % (tag, i)].astype(np.int64)) for i in (1, 2))
        out = posenet_ref.posenet_forward(P, pts, obj, sample_idx=s, train_keys=bool(train), mode="exact", inject=idx, bn_train=bool(train))
        for gi, grp in enumerate(sorted(grps)):
            w = _group_weights(out, GROUPS[grp], 100 + gi)
            (g,) = torch.autograd.grad(sum((out[k] * w[k].double()).sum() for k in GROUPS[grp]), pts, retain_graph=True)
            ref = torch.from_numpy(z["%s.grad.%s" % (tag, grp)]).double()
            assert torch.isfinite(ref).all()
            assert float((g - ref).norm()) <= 3e-2 * float(ref.norm()), (tag, grp)
