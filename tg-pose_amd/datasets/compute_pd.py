"""datasets/compute_pd.py of the reference: the ground-truth persistence images of one cloud, computed on the device.

The reference builds a gudhi AlphaComplex and turns its H1 / H2 diagrams into persim PersImage(spread=1e-2, pixels=[50, 50])
images on the CPU.  Here the same contract runs as tgp_persistence; for a batch use
``ops.persistence_images`` or ``load_data.train_batch(..., persistence=True)``.
"""
import numpy as np
import torch

from .. import ops


def compute_pd(points, device="cuda"):
    """points (n, 3) array (n <= 1024) -> (pis1, pis2): two CPU float32 tensors of shape (2500,)"""
    pc = torch.from_numpy(np.ascontiguousarray(np.asarray(points, dtype=np.float32)).reshape(1, -1, 3)).to(device)
    pdh1, pdh2 = ops.persistence_images(pc)
    return pdh1[0].cpu(), pdh2[0].cpu()
