"""Gradients with respect to the point coordinates on an MI355X: PoseNet9D in eval and training mode, the encoder-only net and the
gcn3d seam layers against the oracle's autograd (plain torch, fp64) on the same neighbour graphs and subsample draws."""
import os

import numpy as np
import pytest
import torch

from oracle import gcn_ref, posenet_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_TOL = 3e-2         # the bar of the parameter-gradient tests (tests/test_gpu_parity.py), relative to the reference's norm


def _cloud(B, N, seed, dup=False):
    g = torch.Generator().manual_seed(seed)
    pts = 0.1 * torch.randn(B, N, 3, generator=g) + torch.tensor([0.1, -0.1, 0.9])
    if dup:                                             # tiled clouds repeat points (_sample_points): coincident neighbours
        pts[:, N // 2:] = pts[:, : N - N // 2]
    return pts


def _close(got, want, tol=GRAD_TOL):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert torch.isfinite(got).all()
    ref = float(want.norm())
    assert ref > 0
    err = float((got - want).norm())
    assert err <= tol * ref, (err, ref)


def _weights(out, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(v.shape, generator=g, dtype=torch.float64) for k, v in out.items()}


def _loss(out, w):
    return sum((out[k].double() * w[k].to(out[k].device)).sum() for k in sorted(w))


def _net(only_encoder=False, train=False):
    from tgpose_amd import PoseNet9D, seeded_state_dict
    sd = seeded_state_dict(0)
    net = PoseNet9D(only_encoder=only_encoder)
    if only_encoder:
        sd = {k.replace("face_all.", "face_enc."): v for k, v in sd.items() if k.startswith("face_all.encoder") or k.startswith("face_all.decoder")}
    net.load_state_dict(sd, strict=not only_encoder)
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    net = net.to(DEV)
    return (net.train() if train else net.eval()), {k: v.detach().cpu() for k, v in net.state_dict().items()}


def _sample(N, seed=1):
    torch.manual_seed(seed)
    i1 = torch.randperm(N)[: N // 4]
    return i1, torch.randperm(i1.numel())[: i1.numel() // 4]


def _p64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


GROUPS = {"rot": ["p_green_R", "p_red_R", "f_green_R", "f_red_R"], "ts": ["Pred_T", "Pred_s"], "recon": ["recon"], "h": ["h1", "h2"],
          "feat": ["feat"], "fglob": ["feat_global"]}
CASE_GROUPS = {"eval": ["rot", "ts"], "dup": ["rot", "ts"], "train": ["feat", "fglob", "h", "recon", "rot", "ts"], "enc": ["fglob", "recon"]}


def _group_weights(out, keys, seed):
    """tests/golden/make_xyz_grad_golden.py's xyz_grad_weights: one seeded generator per output group, the keys in order"""
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(tuple(out[k].shape), generator=g) for k in keys}


def _fixture():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xyz_grad.npz"))


def _fixture_case(tag):
    """PoseNet9D on the fixture's cloud with the reference's graphs and subsample injected: d points of every output group on its own
    (one forward, one autograd.grad per group) -> {group: (got, reference's)}"""
    from tgpose_amd import FLAGS
    z = _fixture()
    train = tag == "train"
    net, _ = _net(only_encoder=tag == "enc", train=train)
    pts, obj = torch.from_numpy(z[tag + ".points"]), torch.from_numpy(z[tag + ".obj_id"])
    idx = {k[len(tag) + 5:]: torch.from_numpy(z[k].astype(np.int64)).to(DEV) for k in z.files if k.startswith(tag + ".idx.")}
    sample = tuple(torch.from_numpy(z["%s.sample_idx_%d" % (tag, i)].astype(np.int64)) for i in (1, 2))
    FLAGS.train = int(train)
    try:
        x = pts.to(DEV).requires_grad_(True)
        out = net(x, obj.to(DEV), sample_idx=sample, inject=idx)
        res = {}
        for gi, grp in enumerate(sorted(CASE_GROUPS[tag])):
            w = _group_weights(out, GROUPS[grp], 100 + gi)
            loss = sum((out[k] * w[k].to(DEV)).sum() for k in GROUPS[grp])
            (g,) = torch.autograd.grad(loss, x, retain_graph=True)
            res[grp] = (g, torch.from_numpy(z["%s.grad.%s" % (tag, grp)]))
    finally:
        FLAGS.train = 0
    return res


@pytest.mark.parametrize("tag", ["eval", "train", "enc"])
def test_points_grad_matches_reference_per_output_group(tag):
    """eval / training mode / encoder-only: each output group's d points against the reference's (tests/golden/xyz_grad.npz), so that
    no path hides behind a larger one (the rotation heads, Pred_T / Pred_s with the centring and Pose_Ts's xyz columns, recon + mean,
    feat and feat_global separately)"""
    for grp, (got, want) in _fixture_case(tag).items():
        _close(got, want)


def test_points_grad_duplicated_points_finite_and_match_reference_per_copy():
    """a cloud whose second half repeats the first (coincident points, as _sample_points' tiling makes): finite, and the reference's
    per copy"""
    for grp, (got, want) in _fixture_case("dup").items():
        assert torch.isfinite(got).all()
        _close(got, want)


def _full_net_case(train, dup=False, B=3, N=256):
    """one loss over every output against the fp64 oracle's autograd (graphs from the oracle): the smoke-level end-to-end check"""
    from tgpose_amd import FLAGS
    net, sd = _net(train=train)
    pts = _cloud(B, N, 5, dup)
    obj = torch.tensor([[0.0], [2.0], [5.0]])[:B]
    sample = _sample(N)
    p64 = pts.double().requires_grad_(True)
    want, inter = posenet_ref.posenet_forward(_p64(sd), p64, obj, sample_idx=sample, train_keys=train, mode="exact",
                                              want_intermediates=True, bn_train=train)
    want = {k: v for k, v in want.items() if not k.startswith("_")}
    w = _weights(want, 7)
    _loss(want, w).backward()
    FLAGS.train = int(train)
    try:
        x = pts.to(DEV).requires_grad_(True)
        got = net(x, obj.to(DEV), sample_idx=sample, inject=inter["indices"])
        assert set(got) == set(want)
        _loss(got, w).backward()
    finally:
        FLAGS.train = 0
    return x.grad, p64.grad, net


def test_points_grad_forced_decisions_b32_n1028():
    """the benchmark's shape (k = 20 at the first coarse level, the reverse lists of every level): the HIP run's decisions forced on the
    oracle (autograd.TAPS -> posenet_ref.posenet_forward(force=...), as test_backward_full_network_with_forced_decisions), training mode;
    d points of the pose keys and of recon, each on its own, within rounding of the oracle's"""
    from tgpose_amd import FLAGS, autograd, seeded_state_dict
    B, N, seed = 32, 1028, 44
    sd = seeded_state_dict(0)
    pts = _cloud(B, N, seed)
    obj = (torch.arange(B) % 6).float().view(B, 1)
    sample = _sample(N, seed)
    with torch.no_grad():
        _, inter = posenet_ref.posenet_forward(sd, pts, obj, sample_idx=sample, train_keys=True, mode="exact", bn_train=True,
                                               want_intermediates=True)
    net, _ = _net(train=True)
    FLAGS.train = 1
    autograd.TAPS = taps = {}
    try:
        x = pts.to(DEV).requires_grad_(True)
        out = net(x, obj.to(DEV), sample_idx=sample, inject=inter["indices"])
    finally:
        FLAGS.train = 0
        autograd.TAPS = None
    p = pts.clone().requires_grad_(True)
    forced = posenet_ref.posenet_forward(sd, p, obj, sample_idx=sample, train_keys=True, mode="exact", bn_train=True,
                                         inject=inter["indices"], force=taps)
    for gi, grp in enumerate(("rot", "ts", "recon")):
        keys = GROUPS[grp]
        w = _group_weights(forced, keys, 200 + gi)
        (want,) = torch.autograd.grad(sum((forced[k] * w[k]).sum() for k in keys), p, retain_graph=True)
        (got,) = torch.autograd.grad(sum((out[k] * w[k].to(DEV)).sum() for k in keys), x, retain_graph=True)
        _close(got, want, tol=5e-3)


def test_points_grad_bit_repeatable():
    a, _, _ = _full_net_case(train=False)
    b, _, _ = _full_net_case(train=False)
    assert torch.equal(a, b)


def test_training_parameter_grads_and_buffers_unchanged_by_points_grad():
    from tgpose_amd import FLAGS
    B, N = 3, 256
    pts, obj, sample = _cloud(B, N, 11), torch.tensor([[0.0], [2.0], [5.0]]), _sample(N)
    res = []
    for req in (False, True):
        net, _ = _net(train=True)
        FLAGS.train = 1
        try:
            x = pts.to(DEV).requires_grad_(req)
            out = net(x, obj.to(DEV), sample_idx=sample)
            sum(v.square().mean() for v in out.values()).backward()
        finally:
            FLAGS.train = 0
        res.append(({n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None},
                    {n: b.clone() for n, b in net.named_buffers()}, x.grad))
    (g0, b0, _), (g1, b1, xg) = res
    assert xg is not None and torch.isfinite(xg).all()
    assert g0.keys() == g1.keys() and all(torch.equal(g0[k], g1[k]) for k in g0)
    assert all(torch.equal(b0[k], b1[k]) for k in b0)


def test_eval_outputs_match_fused_forward_and_buffers_stay():
    from tgpose_amd import FLAGS
    net, _ = _net()
    FLAGS.train = 0
    for B in (1, 3):
        pts, obj, sample = _cloud(B, 256, 13), torch.tensor([[0.0], [2.0], [5.0]])[:B].to(DEV), _sample(256)
        bufs = {n: b.clone() for n, b in net.named_buffers()}
        with torch.no_grad():
            ref = net(pts.to(DEV), obj, sample_idx=sample)
        x = pts.to(DEV).requires_grad_(True)
        got = net(x, obj, sample_idx=sample)
        assert set(got) == set(ref)
        for k in ref:
            assert got[k].grad_fn is not None, k
            assert (got[k].detach() - ref[k]).abs().max().item() < 2e-5, k
        sum(v.sum() for v in got.values()).backward()
        assert x.grad is not None and torch.isfinite(x.grad).all()
        assert all(torch.equal(bufs[n], b) for n, b in net.named_buffers())


# ------------------------------------------------------------------------------------------------ the gcn3d seam stand-alone
def _layer_p(layer, name):
    P = {name + "." + k: v.detach().cpu().double() for k, v in layer.state_dict().items()}
    P["_support_num"] = 7
    return P


def test_seam_surface_layer_points_grad():
    from tgpose_amd.network.fs_net_repo import gcn3d
    torch.manual_seed(0)
    layer = gcn3d.HSlayer_surface(128, 7).to(DEV)
    pts, k = _cloud(2, 300, 21), 20
    x = pts.to(DEV).requires_grad_(True)
    out = layer(x, k)
    w = torch.randn(out.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    (out.double() * w.to(DEV)).sum().backward()
    p64 = pts.double().requires_grad_(True)
    (gcn_ref.surface_conv(_layer_p(layer, "L"), "L", p64, k, gcn_ref.GraphCache()) * w).sum().backward()
    _close(x.grad, p64.grad)


def test_seam_hs_layer_points_grad():
    from tgpose_amd.network.fs_net_repo import gcn3d
    torch.manual_seed(0)
    layer = gcn3d.HS_layer(128, 128, 7).to(DEV)
    pts, k = _cloud(2, 300, 22), 20
    fm = torch.randn(2, 300, 128, generator=torch.Generator().manual_seed(2))
    x = pts.to(DEV).requires_grad_(True)
    out = layer(x, fm.to(DEV), k)
    w = torch.randn(out.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    (out.double() * w.to(DEV)).sum().backward()
    p64 = pts.double().requires_grad_(True)
    (gcn_ref.hs_conv(_layer_p(layer, "L"), "L", p64, fm.double(), k, gcn_ref.GraphCache()) * w).sum().backward()
    _close(x.grad, p64.grad)


def test_seam_pool_layer_points_grad():
    from tgpose_amd.network.fs_net_repo import gcn3d
    pts = _cloud(2, 256, 23)
    fm = torch.randn(2, 256, 128, generator=torch.Generator().manual_seed(3))
    x = pts.to(DEV).requires_grad_(True)
    torch.manual_seed(5)
    v, f = gcn3d.Pool_layer()(x, fm.to(DEV))
    assert v.grad_fn is not None
    torch.manual_seed(5)
    sample = gcn_ref.draw_sample_idx(256)
    wv = torch.randn(v.shape, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    (v.double() * wv.to(DEV)).sum().backward()
    p64 = pts.double().requires_grad_(True)
    v64, _ = gcn_ref.pool(p64, fm.double(), sample, gcn_ref.GraphCache(), "p")
    (v64 * wv).sum().backward()
    _close(x.grad, p64.grad, tol=1e-6)


def test_seam_layers_match_reference_fixture():
    """HSlayer_surface, HS_layer and Pool_layer stand-alone on the fixture's cloud (layers.npz's weights): d vertices against the
    reference's own (tests/golden/xyz_grad.npz); the kNN graphs are the HIP kernels' (bit-exact to the reference's)"""
    from tgpose_amd import seeded_state_dict
    from tgpose_amd.network.fs_net_repo import gcn3d
    z = _fixture()
    sd = seeded_state_dict(3)
    pre = "face_all.encoder."
    conv0, conv1 = gcn3d.HSlayer_surface(128, 7), gcn3d.HS_layer(128, 128, 7)
    conv0.load_state_dict({k[len(pre + "conv_0."):]: v for k, v in sd.items() if k.startswith(pre + "conv_0.")})
    conv1.load_state_dict({k[len(pre + "conv_1."):]: v for k, v in sd.items() if k.startswith(pre + "conv_1.")})
    conv0, conv1 = conv0.to(DEV), conv1.to(DEV)
    xyz, fin = torch.from_numpy(z["layer.xyz"]), torch.from_numpy(z["layer.fin"]).to(DEV)
    x = xyz.to(DEV).requires_grad_(True)
    out = conv0(x, 20)
    (got,) = torch.autograd.grad((out * _group_weights({"o": out}, ["o"], 1)["o"].to(DEV)).sum(), x)
    _close(got, torch.from_numpy(z["layer.grad.surface"]))
    x = xyz.to(DEV).requires_grad_(True)
    out = conv1(x, fin, 20)
    (got,) = torch.autograd.grad((out * _group_weights({"o": out}, ["o"], 2)["o"].to(DEV)).sum(), x)
    _close(got, torch.from_numpy(z["layer.grad.hs"]))
    x = xyz.to(DEV).requires_grad_(True)
    torch.manual_seed(77)
    vp, _ = gcn3d.Pool_layer(4, 4)(x, fin)
    (got,) = torch.autograd.grad((vp * _group_weights({"v": vp}, ["v"], 3)["v"].to(DEV)).sum(), x)
    _close(got, torch.from_numpy(z["layer.grad.pool"]), tol=1e-6)


def _nbr_dirs_case(pts, k=16):
    from tgpose_amd.network.fs_net_repo import gcn3d
    idx = gcn_ref.knn_index(pts.double(), k)
    x = pts.to(DEV).requires_grad_(True)
    unit, raw = gcn3d.get_neighbor_direction_norm(x, idx.to(DEV), return_unnormed=True)
    g = torch.Generator().manual_seed(6)
    wu, wr = torch.randn(unit.shape, generator=g, dtype=torch.float64), torch.randn(raw.shape, generator=g, dtype=torch.float64)
    ((unit.double() * wu.to(DEV)).sum() + (raw.double() * wr.to(DEV)).sum()).backward()
    p64 = pts.double().requires_grad_(True)
    nb = gcn_ref.gather_rows(p64, idx) - p64.unsqueeze(2)
    ((torch.nn.functional.normalize(nb, dim=-1) * wu).sum() + (nb * wr).sum()).backward()
    assert torch.isfinite(x.grad).all()
    return x, idx, unit, x.grad, p64.grad


def test_seam_neighbor_direction_norm_points_grad():
    """distinct points: F.normalize's radial term, the centre term and the reverse-list sums of tgp_dirs_to_xyz"""
    from tgpose_amd.network.fs_net_repo import gcn3d
    x, idx, unit, got, want = _nbr_dirs_case(_cloud(2, 200, 24))
    _close(got, want, tol=1e-5)
    d2, _ = gcn3d.get_receptive_fields(16, x, mode="RF-P")
    assert d2.shape == unit.shape and d2.grad_fn is not None


def test_seam_neighbor_direction_norm_coincident_points():
    """coincident points (rows 100:110 repeat 0:10): their zero directions take torch's d / 1e-12 (finite); those rows and all the other
    rows are each held to their own norm"""
    pts = _cloud(2, 200, 24)
    pts[:, 100:110] = pts[:, 0:10]
    _, _, _, got, want = _nbr_dirs_case(pts)
    got = got.detach().cpu()
    co = torch.zeros(200, dtype=torch.bool)
    co[0:10] = co[100:110] = True
    _close(got[:, co], want[:, co], tol=1e-5)
    _close(got[:, ~co], want[:, ~co], tol=1e-5)


def test_dirs_to_xyz_reverse_list_forms_agree():
    """tgp_dirs_to_xyz over tgp_reverse_graph's lists (rev_global = 0) and over tgp_child_lists' (rev_global = 1, the form for graphs
    too large for the LDS sort): the same sums in the same order, bit for bit; accumulate adds to the buffer"""
    from tgpose_amd import ops
    pts = _cloud(2, 300, 25).to(DEV)
    idx = ops.knn_xyz(pts.contiguous(), 20)
    ddir = torch.randn(2, 300, 20, 3, generator=torch.Generator().manual_seed(8)).to(DEV)
    a = ops.dirs_to_xyz(pts, idx, ddir, rev=ops.reverse_graph(idx, 300))
    ptr, ent = ops.child_lists(idx.view(2, 300 * 20), 300)
    b = ops.dirs_to_xyz(pts, idx, ddir, rev=(ptr, ent, 1))
    assert torch.equal(a, b)
    c = ops.dirs_to_xyz(pts, idx, ddir, rev=(ptr, ent, 1), out=a.clone(), accumulate=True)
    assert torch.equal(c, a + b)


def test_center_backward_matches_torch():
    """tgp_center_bwd against torch's autograd of (points - points.mean(1), points.mean(1)), including the -mean(d xyz) term"""
    from tgpose_amd import autograd
    pts = _cloud(3, 257, 26)
    g = torch.Generator().manual_seed(9)
    wx, wm = torch.randn(3, 257, 3, generator=g, dtype=torch.float64), torch.randn(3, 3, generator=g, dtype=torch.float64)
    x = pts.to(DEV).requires_grad_(True)
    xyz, mean = autograd._Center.apply(x)
    ((xyz.double() * wx.to(DEV)).sum() + (mean.double() * wm.to(DEV)).sum()).backward()
    p = pts.double().requires_grad_(True)
    m = p.mean(dim=1)
    (((p - m.unsqueeze(1)) * wx).sum() + (m * wm).sum()).backward()
    _close(x.grad, p.grad, tol=1e-5)
    x2 = pts.to(DEV).requires_grad_(True)
    xyz, _ = autograd._Center.apply(x2)
    (xyz.double() * wx.to(DEV)).sum().backward()                   # d mean absent: only the centring term
    _close(x2.grad, p.grad - (wm / 257).unsqueeze(1), tol=1e-5)


def test_pose_ts_xyz_columns_gradient_matches_torch():
    """_FeatConsumersFactored.backward's d tail: Pose_Ts's first GEMM reads the centred xyz after the one-hot (PoseNet9D.py:63); its
    gradient to those three columns against torch on the same operands (one 1289-wide layer beside a 1286-wide one)"""
    from tgpose_amd import autograd, engine, ops
    B, N, N1, N2 = 2, 64, 16, 4
    g = torch.Generator().manual_seed(10)
    fm01, fm23, fm4 = torch.randn(B, N, 256, generator=g), torch.randn(B, N1, 512, generator=g), torch.randn(B, N2, 512, generator=g)
    xyz = torch.randn(B, N, 3, generator=g)
    onehot = torch.zeros(B, N, 6)
    onehot[:, :, 2] = 1
    near1, near2 = torch.randint(0, N1, (B, N), generator=g), torch.randint(0, N2, (B, N), generator=g)
    W1, b1 = 0.05 * torch.randn(64, 1286, generator=g), torch.randn(64, generator=g)
    W2, b2 = 0.05 * torch.randn(32, 1289, generator=g), torch.randn(32, generator=g)
    w1, w2 = torch.randn(B, N, 64, generator=g), torch.randn(B, N, 32, generator=g)
    d = lambda t: t.to(DEV)
    x = d(xyz).requires_grad_(True)
    tail = torch.cat([d(onehot), x, torch.zeros(B, N, engine.FINE_LD - 256 - 9, device=DEV)], 2)
    n1, n2 = d(near1).int().contiguous(), d(near2).int().contiguous()
    base = torch.arange(B, device=DEV, dtype=torch.int32).view(B, 1)
    parts = (d(fm01), d(fm23), d(fm4), tail, n1 + base * N1, n2 + base * N2, ops.child_lists(n1, N1), ops.child_lists(n2, N2))
    y1, y2 = autograd.feat_consumers_factored(parts, [(d(W1), d(b1)), (d(W2), d(b2))])
    ((y1 * d(w1)).sum() + (y2 * d(w2)).sum()).backward()
    p = xyz.double().requires_grad_(True)
    up = lambda t, nr: torch.stack([t[b][nr[b]] for b in range(B)])
    feat = torch.cat([fm01.double(), up(fm23.double(), near1), up(fm4.double(), near2), onehot.double(), p], 2)
    ((feat[:, :, :1286] @ W1.double().t() + b1.double()) * w1).sum().add_(((feat @ W2.double().t() + b2.double()) * w2).sum()).backward()
    _close(x.grad, p.grad, tol=1e-4)
