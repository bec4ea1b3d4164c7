"""``build_optimizer`` / ``build_lr_rate`` of ``tools/training_utils`` (bytecode only in the reference): Ranger over
the trainer's parameter groups with the flags' weight decay, and flat_and_anneal with relative decay steps (0.5, 0.75) and the flags'
warmup / anneal settings."""
from ..config import FLAGS
from .torch_utils.solver.lr_scheduler import flat_and_anneal_lr_scheduler
from .torch_utils.solver.ranger2020 import Ranger

REL_STEPS = (0.5, 0.75)


def build_optimizer(params):
    if str(FLAGS.optimizer_type).lower() != "ranger":
        raise ValueError("Unknown optimizer: {} (only Ranger is rebuilt)".format(FLAGS.optimizer_type))
    return Ranger(params=params, lr=float(FLAGS.lr) * FLAGS.lr_pose, weight_decay=FLAGS.weight_decay)


def build_lr_rate(optimizer, total_iters):
    if str(FLAGS.lr_scheduler_name).lower() != "flat_and_anneal":
        raise ValueError("Unknown LR scheduler: {} (only flat_and_anneal is rebuilt)".format(FLAGS.lr_scheduler_name))
    return flat_and_anneal_lr_scheduler(optimizer, total_iters=total_iters, warmup_factor=FLAGS.warmup_factor,
                                        warmup_iters=FLAGS.warmup_iters, warmup_method=FLAGS.warmup_method,
                                        anneal_method=FLAGS.anneal_method, anneal_point=FLAGS.anneal_point, steps=REL_STEPS,
                                        target_lr_factor=0, poly_power=FLAGS.poly_power, step_gamma=FLAGS.gamma)
