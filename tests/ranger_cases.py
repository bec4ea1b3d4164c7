"""The Ranger fixture's cases, shared by tests/golden/make_ranger_golden.py (which runs the reference's optimizer on them) and the
tests: a small parameter set with net1's shape classes, seeded gradients (regenerated bit for bit, never stored), the configurations
and the schedule.  Nothing here imports the reference or the package."""
import numpy as np

# net1's classes: a 3-element GC row (conv_0.STE_layer), 128- and 512-element rows, a short 2-D row, 1-D tensors (no GC), a
# 7-element 3-D row, and rows longer than the kernel's register bound (4096); few rows each, to keep the fixture small
SHAPES = [(128, 3, 1), (8, 128, 1), (4, 512), (3, 224), (256,), (1,), (5, 7, 1), (2, 4100)]
STEPS = 13                  # crosses N_sma's threshold at step 6 and lookahead at steps 6 and 12
CHECKPOINTS = (5, 6, 13)
BASE_LR = 1e-2
MAX_NORM = 5.0
SCHED = dict(total_iters=STEPS, warmup_iters=3, warmup_factor=0.1, warmup_method="linear", anneal_point=0.5, anneal_method="cosine")
CONFIGS = {
    "default": dict(kw={}, none={}),
    "wd": dict(kw=dict(weight_decay=1e-2), none={}),
    "nogc": dict(kw=dict(use_gc=False), none={}),
    "convonly": dict(kw=dict(gc_conv_only=True), none={}),
    "none39": dict(kw={}, none={3: (3, 9)}),            # parameter 3's grad is None on steps 3 and 9
}
# what the fixture keeps of each configuration: {checkpoint step: state fields}
STORED = {
    "default": {5: ("p",), 6: ("p", "slow_buffer"), 13: ("p", "exp_avg", "exp_avg_sq", "slow_buffer", "grad")},
    "wd": {13: ("p", "exp_avg")},
    "nogc": {13: ("p",)},                                # the gradients GC leaves alone are checked against the inputs
    "convonly": {13: ("p",)},
    "none39": {13: ("p", "exp_avg")},
}
SD_STEP = 7                 # the reference state_dict of "default" after this step is stored, to load and continue
SCHED_TABLE = dict(total_iters=60, warmup_iters=10, warmup_factor=0.05, anneal_point=0.5, target_lr_factor=0.01, poly_power=0.9,
                   step_gamma=0.1, steps=(0.5, 0.75))


def init_params():
    rs = np.random.RandomState(20261015)
    return [(0.1 * rs.standard_normal(s)).astype(np.float32) for s in SHAPES]


def grad(step, i):
    """parameter i's gradient at step (1-based): unit normals plus a per-row offset (something for GC to remove), scaled so that
    clip_grad_norm_(5) clips on every third step and not on the others"""
    rs = np.random.RandomState(1000 * step + i)
    s = SHAPES[i]
    g = rs.standard_normal(s) + rs.standard_normal((s[0],) + (1,) * (len(s) - 1)) * 0.5
    scale = 0.08 if step % 3 == 0 else 0.01
    return (scale * g).astype(np.float32)


def has_grad(config, step, i):
    return step not in CONFIGS[config]["none"].get(i, ())
