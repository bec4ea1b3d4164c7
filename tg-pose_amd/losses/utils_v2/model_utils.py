"""Drop-in for the metric helpers of ``losses/utils_v2/model_utils.py`` (``calc_cd`` :94-111, ``calc_emd`` :114-119) on the HIP
kernels.  The density-aware Chamfer loss the training uses is ``losses/dcd.py``; its ``calc_cd`` keeps the (pred, gt) order of
``losses/TDA_loss_sym_recon.py``, the one here the (gt, output) order of this file's reference."""
import torch

from ..metrics import cd, emd, fscore


def calc_cd(output, gt, calc_f1=False, return_raw=False, normalize=False, separate=False):
    """-> [cd_p, cd_t] (or their two directed halves stacked when `separate`) [+ f1] [+ dist1, dist2, idx1, idx2].  The Chamfer
    kernel is called with (gt, output), as the reference calls it: dist1 / idx1 belong to the points of gt."""
    dist1, dist2, idx1, idx2 = cd()(gt, output)
    if separate:
        res = [torch.cat([torch.sqrt(dist1).mean(1).unsqueeze(0), torch.sqrt(dist2).mean(1).unsqueeze(0)]),
               torch.cat([dist1.mean(1).unsqueeze(0), dist2.mean(1).unsqueeze(0)])]
    else:
        res = [(torch.sqrt(dist1).mean(1) + torch.sqrt(dist2).mean(1)) / 2, dist1.mean(1) + dist2.mean(1)]
    if calc_f1:
        res.append(fscore(dist1, dist2)[0])
    if return_raw:
        res.extend([dist1, dist2, idx1, idx2])
    return res


def calc_emd(output, gt, eps=0.005, iterations=50):
    """-> (B,) mean matched distance of `output` to `gt` after `iterations` auction iterations"""
    dist, _ = emd()(output, gt, eps, iterations)
    return torch.sqrt(dist).mean(1)
