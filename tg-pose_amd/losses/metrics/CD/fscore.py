"""Drop-in for ``losses/metrics/CD/fscore.py``: element-wise torch on the Chamfer kernel's device tensors, no kernel of its own."""
import torch


def fscore(dist1, dist2, threshold=0.0001):
    """dist1 (B,n), dist2 (B,m) SQUARED nearest-neighbour distances -> (fscore, precision_1, precision_2), each (B,):
    the fractions of each cloud's points closer than `threshold` to the other cloud and their harmonic mean, 0 where both
    fractions are 0 (the reference replaces the NaN of 0 / 0)."""
    precision_1 = (dist1 < threshold).float().mean(dim=1)
    precision_2 = (dist2 < threshold).float().mean(dim=1)
    f = 2 * precision_1 * precision_2 / (precision_1 + precision_2)
    f = torch.where(torch.isnan(f), torch.zeros_like(f), f)
    return f, precision_1, precision_2
