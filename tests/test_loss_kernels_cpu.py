"""Pins tests/loss_kernels_ref.py (the float64 reference tests/test_loss_kernels_gpu.py holds the loss kernels to) without a GPU:
in float64 against the oracle (oracle/tda_loss_ref.py, oracle/loss_ref.py) and against losses.dcd.pose_rotation_torch on a
synth_loss_batch case, an all-symmetric batch and a batch with sym[:, 0] in {2, -1}; and against the values and gradients the imported
reference recorded in tests/golden/{tda_loss,dcd,recon_completion,pose_assembly}.npz, at the tolerances the GPU tests hold those
fixtures to."""
import math

import numpy as np
import pytest
import torch

from tests import loss_kernels_ref as K
from tests.util import golden, synth_loss_batch

F64 = torch.float64
POSE_W = [8.0, 8.0, 8.0, 8.0, 4.0, 8.0, 8.0, 1.0]               # config/config.py:71-114 in the order of the kernel's terms
NAMES = ["Rot1", "Rot1_cos", "Rot2", "Rot2_cos", "Rot_regular", "Tran", "Size", "R_con"]


def _pose_ops(pred, gt):
    p = tuple(pred[k].detach() for k in ("Rot1", "Rot2", "Rot1_f", "Rot2_f", "Tran", "Size"))
    return p, (gt["Rot1"], gt["Rot2"], gt["Tran"], gt["Size"])


def _batches():
    """name -> (pred, gt, sym, extra): the synthetic batch as it is, all objects symmetric about y, and sym0 in {2, -1} mixed in"""
    out = {}
    for name in ("mixed", "all_sym", "sym0_2_m1"):
        pred, gt, sym, extra = synth_loss_batch(seed=7, B=11, N=33, D=20, C=30)
        if name == "all_sym":
            sym[:, 0] = 1
        if name == "sym0_2_m1":
            sym[1, 0], sym[5, 0], sym[6, 0] = 2, -1, 2
            sym[9] = torch.tensor([1, -1, 0, -1])                                    # sym0 == 1 with a negative rest: mode 3 as well
        out[name] = (pred, gt, sym, extra)
    return out


BATCHES = _batches()


@pytest.mark.parametrize("kind", [0, 1], ids=["l1", "smoothl1"])
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_pose_terms_vs_oracle_fp64(name, kind):
    from oracle import tda_loss_ref as T
    pred, gt, sym, _ = BATCHES[name]
    p, g_ = _pose_ops(pred, gt)
    gw = torch.tensor([0.7, -1.3, 2.0, 0.4, 1.1, -0.6, 0.9, 1.7])
    out, grads, amb = K.pose_terms(p, g_, sym, kind, 0.5, gw)
    dp = {k: v.detach().double().requires_grad_(True) for k, v in pred.items()}
    want = T.pose_terms(dp, {k: v.double() for k, v in gt.items()}, sym, "l1" if kind == 0 else "smoothl1")
    for i, k in enumerate(NAMES):
        assert abs(out[i].item() - want[k].item()) <= 1e-13 * max(1.0, abs(want[k].item())), (k, out[i].item(), want[k].item())
    assert out[8].item() == int((sym[:, 0] != 1).sum())
    if name == "all_sym":
        assert out[8].item() == 0 and out[2].item() == 0 and out[3].item() == 0 and out[4].item() == 0
    sum(w * want[k] for w, k in zip(gw.double(), NAMES)).backward()
    for got, k, a in zip(grads, ("Rot1", "Rot2", "Rot1_f", "Rot2_f", "Tran", "Size"), amb):
        r = dp[k].grad if dp[k].grad is not None else torch.zeros_like(dp[k])
        assert torch.allclose(got, r, atol=1e-14, rtol=1e-12), (k, float((got - r).abs().max()))
        assert not bool(a.any()), k                                                     # no sign sits inside the excluded band


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_sym_recon_vs_oracle_fp64(name):
    from oracle import tda_loss_ref as T
    pred, gt, sym, extra = BATCHES[name]
    gl = torch.tensor([1.75])
    loss, (dpc, dre), amb = K.sym_recon(pred["Recon"].detach(), extra["recon2"], gt["R"], gt["Tran"], sym, gloss=gl)
    a, b = pred["Recon"].detach().double().requires_grad_(True), extra["recon2"].double().requires_grad_(True)
    want = T.prop_sym_matching_loss(a, b, gt["R"].double(), gt["Tran"].double(), sym)
    (want * 1.75).backward()
    assert abs(loss.item() - want.item()) <= 1e-14
    ga = a.grad if a.grad is not None else torch.zeros_like(a)
    assert torch.allclose(dpc, ga, atol=1e-16, rtol=1e-12) and torch.allclose(dre, b.grad, atol=1e-16, rtol=1e-12)
    assert not bool(amb[0].any()) and not bool(amb[1].any())
    modes = set(K.sym_mode(sym, 4).tolist())
    assert modes == ({1, 4} if name == "all_sym" else {0, 1, 2, 3, 4} if name == "sym0_2_m1" else {0, 1, 2, 4})


def test_sym_mode_routes_and_one_column():
    sym = torch.tensor([[0, 0, 0, 0], [0, 1, 0, 0], [1, 1, 0, 0], [1, 0, 0, 0], [2, 1, 1, 1], [-1, 0, 0, 0], [1, -1, 0, 0], [1, 1, -1, -1]])
    assert K.sym_mode(sym, 4).tolist() == [0, 2, 1, 4, 3, 3, 3, 3]
    assert K.sym_mode(sym, 1).tolist() == [0, 0, 4, 4, 3, 3, 4, 4]                  # one column: no mirror, no half turn


def test_ph_loss_and_feat_consistency_vs_oracle_fp64():
    from oracle import tda_loss_ref as T
    pred, gt, sym, extra = BATCHES["mixed"]
    a, b = pred["TDA_h1"].detach(), gt["h1"]
    loss, live, w, da, amb = K.rowl1(a, b, b, gout=torch.tensor([0.875]))
    ad = a.double().requires_grad_(True)
    want = T.ph_loss(ad, b.double())
    (0.875 * want).backward()
    assert live == 1.0 and abs(loss.item() - want.item()) <= 1e-15 and torch.allclose(da, ad.grad, atol=1e-18, rtol=1e-12)
    assert torch.equal(w, (b.sum(1) > 0).double()) and 0 < w.sum() < w.numel() and not bool(amb.any())
    bad_a, bad_b = a.clone(), b.clone()
    bad_a[1, 3], bad_b[2, 5] = float("inf"), float("nan")
    for x, y in ((bad_a, b), (bad_a, bad_b)):
        loss, live, _, da, _ = K.rowl1(x, y, b, gout=torch.tensor([0.875]))
        assert math.isnan(loss.item()) and torch.isnan(T.ph_loss(x, y)) and live == 0.0 and float(da.abs().max()) == 0.0
    loss, live, _, da, _ = K.rowl1(a, bad_b, b, gout=torch.tensor([0.875]))
    assert loss.item() == 0.0 == T.ph_loss(a, bad_b).item() and live == 0.0 and float(da.abs().max()) == 0.0
    x1, x2 = extra["feat1"].clone(), extra["feat2"].clone()
    x1[5] = 0.0                                                                          # floors: x2 row 3, x1 row 5 ...
    x1[6], x2[6] = 0.0, 0.0                                                              # ... and both in row 6
    loss, (d1, d2) = K.feat_consistency(x1, x2, gloss=torch.tensor([1.25]))
    u, v = x1.double().requires_grad_(True), x2.double().requires_grad_(True)
    want = T.feat_consistency(u, v)
    (1.25 * want).backward()
    assert abs(loss.item() - want.item()) <= 1e-14
    # F.normalize's floor in float64 is 1e-12, the kernels' is the float32 nearest to it: 4e-9 apart, relatively
    assert torch.allclose(d1, u.grad, atol=1e-14, rtol=1e-8) and torch.allclose(d2, v.grad, atol=1e-14, rtol=1e-8)
    assert float(d2[3].abs().max()) > 1e9 and float(d1[3].abs().max()) == 0.0           # the gradient F.normalize's floor gives


def _chain(pred, gt, i1, i2, gd1, gd2):
    """d/d pred, d/d gt of sum(gd1 * dist1) + sum(gd2 * dist2) with the Chamfer distances expressed through the found indices"""
    p, q = pred.double().requires_grad_(True), gt.double().requires_grad_(True)
    take = lambda src, idx: torch.gather(src, 1, idx.long().unsqueeze(-1).expand(-1, -1, 3))
    d1, d2 = ((p - take(q, i1)) ** 2).sum(-1), ((q - take(p, i2)) ** 2).sum(-1)
    ((d1 * gd1).sum() + (d2 * gd2).sum()).backward()
    return p.grad, q.grad


def test_dcd_canonicalize_and_rotation_vs_oracle_fp64():
    from oracle import loss_ref as L
    from tgpose_amd.losses.dcd import pose_rotation_torch
    pred, gt, sym, extra = BATCHES["mixed"]
    B = sym.shape[0]
    gen = torch.Generator().manual_seed(3)
    f_g, f_r = torch.rand(B, generator=gen) * 0.9 + 0.05, torch.rand(B, generator=gen) * 0.9 + 0.05
    symf = sym.float()
    args = (pred["Recon"].detach(), gt["R"], pred["Rot1"].detach(), f_g, pred["Rot2"].detach(), f_r, pred["Tran"].detach(), pred["Size"].detach())
    canon, R = K.canonicalize(*args, symf)
    wc, wR = L.canonicalize(*[a.double() for a in args], symf.double())
    assert torch.allclose(R, wR, atol=1e-13) and torch.allclose(canon, wc, atol=1e-13)
    dR = torch.randn(B, 3, 3, generator=gen)
    R2, din = K.pose_rotation(gt["R"][..., 0], args[2], f_g, args[4], f_r, symf[:, 0], dR=dR)
    leaves = [t.double().requires_grad_(True) for t in (args[2], f_g, args[4], f_r)]
    Rt = pose_rotation_torch(gt["R"].double(), leaves[0], leaves[1], leaves[2], leaves[3], symf.double())
    (Rt * dR.double()).sum().backward()
    assert torch.allclose(R2, Rt, atol=1e-13)
    want = torch.cat([leaves[0].grad, leaves[1].grad.unsqueeze(1), leaves[2].grad, leaves[3].grad.unsqueeze(1)], 1)
    assert torch.allclose(din, want, atol=1e-11, rtol=1e-10), float((din - want).abs().max())
    assert float(din[symf[:, 0] == 1][:, 4:].abs().max()) == 0.0                        # symmetric: nothing flows to the red axis
    # calc_dcd: the oracle's weights are float32 (`.float()` in the reference), so agreement is to float32 rounding of the weights
    a, b = canon.float(), (torch.rand(B, 40, 3, generator=gen) - 0.5) * 0.4
    ws = []
    for non_reg in (False, True):
        want, (d1, d2, i1, i2) = L.calc_dcd(a, b, 70.0, 0.3, non_reg)
        loss, w1, w2 = K.dcd(d1, d2, i1, i2, 70.0, 0.3, non_reg)
        assert torch.allclose(loss, want.double(), atol=1e-6), float((loss - want).abs().max())
        ws.append((w1, w2))
    # n = 33 < m = 40: non_reg clamps frac_12 = n / m to 1 and leaves frac_21 = m / n alone
    assert torch.equal(ws[0][0], ws[1][0]) and torch.allclose(ws[0][1], ws[1][1] * K.f32c(33 / 40), rtol=1e-15)


@pytest.mark.parametrize("kind", ["l1", "smoothl1"])
def test_reference_vs_recorded_tda_loss(kind):
    """the tolerances of tests/test_gpu_parity.py::test_tda_loss_vs_reference_and_oracle / test_consistency_losses_vs_reference"""
    from tests.test_oracle_golden import tda_loss_case
    gd, pred, gt, sym, extra = tda_loss_case()
    k = 0 if kind == "l1" else 1
    p, g_ = _pose_ops(pred, gt)
    out, grads, _ = K.pose_terms(p, g_, sym, k, 0.5, torch.tensor(POSE_W))
    want = {n.split(".", 2)[2]: float(gd[n][0]) for n in gd.files if n.startswith(kind + ".loss.")}
    close = lambda v, w: abs(v - w) <= 2e-6 * max(1.0, abs(w))
    for i, n in enumerate(NAMES):
        key = "Rot_r_a" if n == "Rot_regular" else n
        assert close(POSE_W[i] * out[i].item(), want[key]), (kind, n, POSE_W[i] * out[i].item(), want[key])
    gclose = lambda got, r: np.allclose(got.numpy(), r, atol=1e-7 + 2e-5 * np.abs(r).max(), rtol=2e-5)
    for got, n in zip(grads, ("Rot1", "Rot2", "Rot1_f", "Rot2_f", "Tran", "Size")):
        assert gclose(got, gd["%s.grad.%s" % (kind, n)]), (kind, n)
    for h, cat in (("h1", "pdh1_category"), ("h2", "pdh2_category")):
        a = pred["TDA_" + h].detach()
        om = 2.0 * math.exp(-K.rowl1(gt[cat], gt[h], gt[h])[0].item())                  # omega(gt_h, cate_h), k = 2, lam = 1 (:313-322)
        l1, _, _, da1, _ = K.rowl1(a, gt[h], gt[h], gout=torch.tensor([4.0]))
        l2, _, _, da2, _ = K.rowl1(a, gt[cat], gt[cat], gout=torch.tensor([om]))
        assert close(4.0 * l1.item(), want["TDA_" + h]) and close(om * l2.item(), want["TDA_%s_cate" % h])
        assert gclose(da1 + da2, gd["%s.grad.TDA_%s" % (kind, h)]), (kind, h)
    if kind == "l1":
        loss, (_, dre), _ = K.sym_recon(gt["Recon"], pred["Recon"].detach(), gt["R"], gt["Tran"], sym, gloss=torch.tensor([1.0]))
        assert close(loss.item(), want["Prop_sym"]) and gclose(dre, gd["l1.grad.Recon"])
        x1, x2 = extra["feat1"], extra["feat2"]
        loss, (d1, d2) = K.feat_consistency(x1, x2, gloss=torch.tensor([2.0]))
        assert abs(2.0 * loss.item() - gd["con.feat"][0]) < 2e-6
        assert np.allclose(d1.numpy(), gd["con.feat.g1"], atol=2e-7, rtol=1e-5) and np.allclose(d2.numpy(), gd["con.feat.g2"], atol=2e-7, rtol=1e-5)
        loss, (dpc, dre), _ = K.sym_recon(pred["Recon"].detach(), extra["recon2"], gt["R"], gt["Tran"], sym, gloss=torch.tensor([1.0]))
        assert abs(loss.item() - gd["con.sym"][0]) < 1e-7
        for got, key in ((dpc, "con.sym.gPC"), (dre, "con.sym.gRe")):
            d = np.abs(got.numpy() - gd[key])
            assert (d > 1e-8).mean() < 1e-3, (key, (d > 1e-8).mean())
        bad_pred, bad_gt = pred["TDA_h1"].detach().clone(), gt["h1"].clone()
        bad_pred[1, 3], bad_gt[2, 5] = float("inf"), float("nan")
        assert math.isnan(K.rowl1(bad_pred, gt["h1"], gt["h1"])[0].item()) and np.isnan(gd["ph.bad_pred"][0])
        z = K.rowl1(pred["TDA_h1"].detach(), bad_gt, bad_gt, gout=torch.tensor([1.0]))
        assert z[0].item() == 0 == gd["ph.bad_gt"][0] and float(z[3].abs().max()) == 0


def test_reference_vs_recorded_dcd_and_pose_assembly():
    """the tolerances of tests/test_gpu_parity.py::test_dcd_and_r_dcd_vs_reference_golden, test_recon_completion_vs_reference_golden and
    test_generate_rt_vs_reference_golden; the Chamfer search is the C oracle's (bit-exact against the kernel, out of scope here)"""
    from oracle import loss_ref as L
    gd, gr, ga = golden("dcd.npz"), golden("recon_completion.npz"), golden("pose_assembly.npz")
    t = lambda k: torch.from_numpy(gd[k])
    canon, R = K.canonicalize(*[t(k) for k in ("recon", "gR", "p_g", "f_g", "p_r", "f_r", "t", "s", "sym")])
    assert np.allclose(R.numpy()[[2, 4, 5]], gd["p_R"][[2, 4, 5]], atol=1e-6)
    ny, nx = K.vertical_axes(t("f_g"), t("f_r"), t("p_g"), t("p_r"))
    assert np.allclose(ny.numpy(), gd["new_y"], atol=1e-6) and np.allclose(nx.numpy(), gd["new_x"], atol=1e-6)
    d1, d2, i1, i2 = L.chamfer(t("recon"), t("prior"))
    B = d1.shape[0]
    loss, w1, w2, (g1, g2) = K.dcd(d1, d2, i1, i2, 70.0, 0.3, gloss=torch.full((B,), 1.0 / B))
    assert np.allclose(loss.numpy(), gd["dcd"], atol=2e-6)
    ga_, _ = _chain(t("recon"), t("prior"), i1, i2, g1, g2)
    assert np.allclose(ga_.numpy(), gd["dcd_grad"], atol=1e-7, rtol=1e-4)
    c1, c2, j1, j2 = L.chamfer(canon.float(), t("prior"))
    assert abs(K.dcd(c1, c2, j1, j2, 70.0, 0.3)[0].mean().item() - float(gd["r_dcd"])) < 2e-6
    # recon_completion (:453-490): 0.9 mean_b(loss1) + 0.1 mean_b(loss2); d / d dist through exp(-alpha d) with the weights detached
    e1, e2 = torch.exp(-d1.double() * K.f32c(70.0)), torch.exp(-d2.double() * K.f32c(70.0))
    val = 0.9 * (1 - e1 * w1).mean(1).mean() + 0.1 * (1 - e2 * w2).mean(1).mean()
    assert abs(val.item() - float(gr["value"])) < 2e-6
    n, m = d1.shape[1], d2.shape[1]
    pa, pb = _chain(t("recon"), t("prior"), i1, i2, 0.9 * 70.0 * e1 * w1 / (B * n), 0.1 * 70.0 * e2 * w2 / (B * m))
    assert np.allclose(pa.numpy(), gr["grad_a"], atol=1e-7, rtol=1e-4) and np.allclose(pb.numpy(), gr["grad_b"], atol=1e-7, rtol=1e-4)
    # the loss's own derivative agrees with that closed form: loss1 + 0.5 loss2, gloss = 1
    _, _, _, (h1, h2) = K.dcd(d1, d2, i1, i2, 70.0, 0.3, gloss=torch.ones(B))
    assert torch.allclose(h1, K.f32c(70.0) * e1 * w1 / n, rtol=1e-12, atol=0) and torch.allclose(h2, 0.5 * K.f32c(70.0) * e2 * w2 / m, rtol=1e-12, atol=0)
    s1, s2, k1, k2 = L.chamfer(t("recon")[:, :700].contiguous(), t("prior"))
    _, v1, v2 = K.dcd(s1, s2, k1, k2, 0.1, 0.3, non_reg=True)
    plain = 0.9 * (1 - torch.exp(-s1.double() * K.f32c(0.1)) * v1).mean(1).mean() + 0.1 * (1 - torch.exp(-s2.double() * K.f32c(0.1)) * v2).mean(1).mean()
    assert abs(plain.item() - float(gr["non_reg_700"])) < 2e-6
    a = lambda k: torch.from_numpy(ga[k])
    rt = K.generate_rt(a("p_g"), a("p_r"), a("f_g"), a("f_r"), a("T"), a("sym")).numpy()
    assert np.allclose(rt[:, :3, :3], ga["R_sym"], atol=2e-6) and np.array_equal(rt[:, :3, 3], ga["T"].astype(np.float64))
    assert np.array_equal(rt[:, 3], np.tile(np.array([0, 0, 0, 1.0]), (16, 1)))
    plain = K.generate_rt(a("p_g"), a("p_r"), a("f_g"), a("f_r"), a("T"), None).numpy()
    assert np.allclose(plain[:, :3, :3], ga["R_plain"], atol=2e-6)


def test_head_post_reference_and_zero_axis():
    gen = torch.Generator().manual_seed(11)
    green, red, ts, mean = torch.randn(5, 4, generator=gen), torch.randn(5, 4, generator=gen), torch.randn(5, 6, generator=gen), torch.randn(5, 3, generator=gen)
    green[2, 1:] = 0.0
    grads = [torch.randn(5, 3, generator=gen), torch.randn(5, 3, generator=gen), torch.randn(5, generator=gen), torch.randn(5, generator=gen),
             torch.randn(5, 3, generator=gen), torch.randn(5, 3, generator=gen)]
    outs, (dg, dr, dt) = K.head_post(green, red, ts, mean, grads)
    assert torch.allclose(outs[0].norm(dim=1)[[0, 1, 3, 4]], torch.ones(4, dtype=F64), atol=1e-5) and float(outs[0][2].abs().max()) == 0.0
    # a zero axis: torch's norm backward gives 0 there, so what is left is g / (0 + 1e-6)
    assert torch.allclose(dg[2, 1:], grads[0][2].double() / 1e-6, rtol=1e-12) and bool(torch.isfinite(dg).all())
    assert torch.equal(dt, torch.cat([grads[4], grads[5]], 1).double())
    f = torch.sigmoid(red[:, 0].double())
    assert torch.allclose(dr[:, 0], grads[3].double() * f * (1 - f), rtol=1e-12)
    _, (dg0, dr0, dt0) = K.head_post(green, red, ts, mean, [None, grads[1], None, None, None, grads[5]])
    assert float(dg0.abs().max()) == 0.0 and float(dt0[:, :3].abs().max()) == 0.0 and torch.equal(dr0[:, 1:], dr[:, 1:])


def test_float32_restatement_and_the_bound():
    """oracle32 is the same code in float32: close to the reference, and the bound it gives is a few float32 roundings wide"""
    pred, gt, sym, extra = BATCHES["mixed"]
    p, g_ = _pose_ops(pred, gt)
    r64, r32 = K.pose_terms(p, g_, sym, 1, 0.5), K.pose_terms(p, g_, sym, 1, 0.5, dtype=torch.float32)
    assert r32.dtype == torch.float32 and r64.dtype == F64
    b = K.bound(r64[:8], r32[:8])
    assert 4 * K.EPS32 * float(r64[:8].abs().max()) <= b <= 64 * K.EPS32 * float(r64[:8].abs().max())
    d = torch.tensor([0.0, 1e-9, -1e-9, 1e-3], dtype=F64)
    assert K.ambiguous(d, torch.ones(1)).tolist() == [False, True, True, False]         # an exact zero is not ambiguous
    assert K.excluded_share_ok(torch.zeros(5000, dtype=torch.bool)) and not K.excluded_share_ok(torch.tensor([True] + [False] * 500))
