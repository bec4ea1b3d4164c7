"""Drop-in for ``losses/metrics``: the metric bundle beside the training loss -- Chamfer (``cd``), F-score and the
auction-matching earth mover's distance (``emd``) -- on the HIP kernels."""
from .CD import cd, fscore
from .EMD import emd

__all__ = ['cd', 'fscore', 'emd']
