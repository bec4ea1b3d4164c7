#!/usr/bin/env python3
"""Writes tests/golden/xyz_grad.npz: the REFERENCE's own gradients with respect to the points (points.grad), recorded with every
neighbour graph and both subsample draws, by importing the reference unmodified as make_golden.py does (run_reference(grad=True)).

Cases (seeded weights, seeded clouds; one forward each, one autograd.grad per output group so that every path is seen on its own):
  eval.*     PoseNet9D().eval(), FLAGS.train = 0, B = 3, N = 256:     groups rot (the four rotation keys), ts (Pred_T, Pred_s)
  train.*    PoseNet9D().train() (dropout p = 0), FLAGS.train = 1:   groups rot, ts, recon, h (h1, h2), feat, fglob (feat_global)
  enc.*      PoseNet9D(only_encoder=True).eval(), B = 2, N = 256:   groups fglob, recon
  dup.*      eval mode on a cloud whose second half repeats the first (tiled clouds, coincident points): groups rot, ts
  layer.*    HSlayer_surface, HS_layer, Pool_layer stand-alone (B = 2, n = 160, as layers.npz)
The loss of a group is sum_k <out_k, w_k> over its keys with w_k = xyz_grad_weights(...) (restated in tests/test_xyz_grad_*.py).

Usage:  python tests/golden/make_xyz_grad_golden.py   (from the repo root)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (sets up the reference's import path and flags)
import numpy as np  # noqa: E402
import torch  # noqa: E402

GROUPS = {"eval": {"rot": ["p_green_R", "p_red_R", "f_green_R", "f_red_R"], "ts": ["Pred_T", "Pred_s"]},
          "train": {"rot": ["p_green_R", "p_red_R", "f_green_R", "f_red_R"], "ts": ["Pred_T", "Pred_s"], "recon": ["recon"],
                    "h": ["h1", "h2"], "feat": ["feat"], "fglob": ["feat_global"]},
          "enc": {"fglob": ["feat_global"], "recon": ["recon"]}}
GROUPS["dup"] = GROUPS["eval"]
NAMES = ["conv_0.rf", "conv_0.orl_xyz", "conv_1.rf", "conv_1.orl_xyz", "pool_1.xyz", "conv_2.rf",
         "conv_2.orl_xyz", "conv_3.rf", "conv_3.orl_xyz", "pool_2.xyz", "conv_4.rf", "conv_4.orl_xyz"]


def xyz_grad_weights(out, keys, seed):
    """the loss weights of one output group: one seeded generator, the keys in the given order"""
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(tuple(out[k].shape), generator=g) for k in keys}


def run(net, pts, obj, fseed, train, prefix):
    """reference forward with its graphs recorded (make_golden.run_reference, for either face prefix); pts requires grad"""
    knn_rec, nn_rec = [], []
    o_knn, o_nn = mg.ref_gcn.get_neighbor_index, mg.ref_gcn.get_nearest_index
    mg.ref_gcn.get_neighbor_index = lambda v, k: (knn_rec.append(o_knn(v, k)), knn_rec[-1])[1]
    mg.ref_gcn.get_nearest_index = lambda t, s_: (nn_rec.append(o_nn(t, s_)), nn_rec[-1])[1]
    try:
        mg.FLAGS.train = train
        torch.manual_seed(fseed)
        out = net(pts, obj)
    finally:
        mg.ref_gcn.get_neighbor_index, mg.ref_gcn.get_nearest_index = o_knn, o_nn
    idx = {prefix + n: r for n, r in zip(NAMES, knn_rec)}
    idx[prefix + "up_1"], idx[prefix + "up_2"] = nn_rec
    return out, idx


def case(arrays, tag, net, pts, obj, fseed, train, prefix):
    x = pts.clone().requires_grad_(True)
    out, idx = run(net, x, obj, fseed, train, prefix)
    for gi, (grp, keys) in enumerate(sorted(GROUPS[tag].items())):
        w = xyz_grad_weights(out, keys, 100 + gi)
        loss = sum((out[k] * w[k]).sum() for k in keys)
        (g,) = torch.autograd.grad(loss, x, retain_graph=True)
        arrays["%s.grad.%s" % (tag, grp)] = g
    i1, i2 = mg.sample_indices(pts.shape[1], fseed)
    arrays[tag + ".points"], arrays[tag + ".obj_id"] = pts, obj
    arrays[tag + ".sample_idx_1"], arrays[tag + ".sample_idx_2"] = mg.small_idx(i1), mg.small_idx(i2)
    for k, v in idx.items():
        arrays["%s.idx.%s" % (tag, k)] = mg.small_idx(v)


def main():
    sd = mg.iw.seeded_state_dict(0)
    arrays = dict(weight_seed=np.int64(0), forward_seed=np.int64(35))
    pts, obj = mg.synth_points(3, 256, 5)
    net = mg.RefPoseNet9D().eval()
    net.load_state_dict(sd, strict=True)
    case(arrays, "eval", net, pts, obj, 35, 0, "face_all.encoder.")
    dup = pts.clone()
    dup[:, 128:] = dup[:, :128]
    case(arrays, "dup", net, dup, obj, 35, 0, "face_all.encoder.")
    net = mg.RefPoseNet9D().train()
    net.load_state_dict(sd, strict=True)
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    case(arrays, "train", net, pts, obj, 35, 1, "face_all.encoder.")
    enc = mg.RefPoseNet9D(only_encoder=True).eval()
    esd = {k.replace("face_all.", "face_enc."): v for k, v in sd.items()
           if k.startswith("face_all.encoder.") or k.startswith("face_all.decoder.")}
    enc.load_state_dict(esd, strict=False)
    pe, oe = mg.synth_points(2, 256, 9)
    case(arrays, "enc", enc, pe, oe, 36, 0, "face_enc.encoder.")

    # the three seam layers stand-alone (layers.npz's weights and cloud)
    lsd = mg.iw.seeded_state_dict(3)
    g = torch.Generator().manual_seed(5)
    xyz = 0.1 * torch.randn(2, 160, 3, generator=g)
    pre = "face_all.encoder."
    conv0 = mg.ref_gcn.HSlayer_surface(kernel_num=128, support_num=7)
    conv1 = mg.ref_gcn.HS_layer(128, 128, support_num=7)
    conv0.load_state_dict({k[len(pre + "conv_0."):]: v for k, v in lsd.items() if k.startswith(pre + "conv_0.")})
    conv1.load_state_dict({k[len(pre + "conv_1."):]: v for k, v in lsd.items() if k.startswith(pre + "conv_1.")})
    with torch.no_grad():
        fin = torch.relu(conv0(xyz, 20))
    arrays["layer.xyz"], arrays["layer.fin"] = xyz, fin
    x = xyz.clone().requires_grad_(True)
    out = conv0(x, 20)
    (arrays["layer.grad.surface"],) = torch.autograd.grad((out * xyz_grad_weights({"o": out}, ["o"], 1)["o"]).sum(), x)
    x = xyz.clone().requires_grad_(True)
    out = conv1(x, fin, 20)
    (arrays["layer.grad.hs"],) = torch.autograd.grad((out * xyz_grad_weights({"o": out}, ["o"], 2)["o"]).sum(), x)
    x = xyz.clone().requires_grad_(True)
    torch.manual_seed(77)
    vp, _ = mg.ref_gcn.Pool_layer(4, 4)(x, fin)
    (arrays["layer.grad.pool"],) = torch.autograd.grad((vp * xyz_grad_weights({"v": vp}, ["v"], 3)["v"]).sum(), x)
    mg.save("xyz_grad.npz", **arrays)


if __name__ == "__main__":
    main()
