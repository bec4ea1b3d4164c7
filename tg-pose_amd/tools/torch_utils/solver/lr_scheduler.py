"""``flat_and_anneal_lr_scheduler`` of ``tools/torch_utils/solver/lr_scheduler.py`` (:177-263) as a ``LambdaLR``.

The factor of iteration x: during the first ``warmup_iters`` iterations a constant ``warmup_factor`` or a linear ramp from it to 1;
then 1 until the anneal starts (``anneal_point * total_iters``, or the first of ``steps`` for the step method); then the chosen anneal
towards ``target_lr_factor``.  The arithmetic is the reference's, term for term and in the same order, so the factors are the same
doubles; the argument checks raise the same errors.
"""
import logging
from bisect import bisect_right
from math import cos, pi

import torch

logger = logging.getLogger(__name__)

WARMUP_METHODS = ("constant", "linear")
ANNEAL_METHODS = ("cosine", "linear", "poly", "exp", "step", "none")


def flat_and_anneal_lr_scheduler(optimizer, total_iters, warmup_iters=0, warmup_factor=0.1, warmup_method="linear", anneal_point=0.72,
                                 anneal_method="cosine", target_lr_factor=0, poly_power=1.0, step_gamma=0.1, steps=(2 / 3.0, 8 / 9.0)):
    if warmup_method not in WARMUP_METHODS:
        raise ValueError("Only 'constant' or 'linear' warmup_method accepted,got {}".format(warmup_method))
    if anneal_method not in ANNEAL_METHODS:
        raise ValueError("Only 'cosine', 'linear', 'poly', 'exp', 'step' or 'none' anneal_method accepted,got {}".format(anneal_method))
    if anneal_method == "step":
        lowest = warmup_iters / total_iters
        if any(s < lowest or s > 1 for s in steps):
            raise ValueError("error in steps: {}. warmup_iters: {} total_iters: {}.steps should be in ({},1)".format(
                steps, warmup_iters, total_iters, lowest))
        if list(steps) != sorted(steps):
            raise ValueError("steps {} is not in ascending order.".format(steps))
        logger.warning("ignore anneal_point when using step anneal_method")
        anneal_start = steps[0] * total_iters
    else:
        if anneal_point > 1 or anneal_point < 0:
            raise ValueError("anneal_point should be in [0,1], got {}".format(anneal_point))
        anneal_start = anneal_point * total_iters
    milestones = [s * total_iters for s in steps]
    span = total_iters - anneal_start          # the anneal's length; every method divides by it in the same place

    def warmup(x):
        if warmup_method == "constant":
            return warmup_factor
        a = float(x) / warmup_iters
        return warmup_factor * (1 - a) + a

    def anneal(x):
        x = float(x)
        if anneal_method == "cosine":
            return target_lr_factor + 0.5 * (1 - target_lr_factor) * (1 + cos(pi * ((x - anneal_start) / span)))
        if anneal_method == "linear":
            return target_lr_factor + (1 - target_lr_factor) * (total_iters - x) / span
        if anneal_method == "poly":
            return target_lr_factor + (1 - target_lr_factor) * ((total_iters - x) / span) ** poly_power
        if anneal_method == "exp":
            return max(target_lr_factor, 5e-3) ** ((x - anneal_start) / span)   # a floor of 5e-3: never all the way to 0
        if anneal_method == "step":
            return step_gamma ** bisect_right(milestones, x)
        return 1

    def factor(x):
        if x < warmup_iters:
            return warmup(x)
        if x >= anneal_start:
            return anneal(x)
        return 1

    return torch.optim.lr_scheduler.LambdaLR(optimizer, factor)
