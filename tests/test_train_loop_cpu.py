"""Host-only parts of the training loop (trainer/RL_TDA.py RL_TDA_train, datasets/load_data.py TrainBatches): the FLAGS defaults
against the reference's config, init_RL_TDA_model's renaming rule, the refill and epoch order of TrainBatches, the checkpoint's
file name and epoch rule, the log line, and the fixture tests/golden/train_loop.npz itself."""
import json

import numpy as np
import pytest
import torch

from tests.util import golden


def test_loop_flags_have_the_reference_defaults():
    """config/config.py:59-61, 136-143"""
    from tgpose_amd import FLAGS
    want = dict(batch_size=24, total_epoch=150, train_steps=2000, save_every=1, log_every=100, model_save="output/models/distr",
                resume=0, resume_model="", RL_model_path="")
    for k, v in want.items():
        assert getattr(FLAGS, k) == v, k


def test_rl_stage_renaming():
    from tgpose_amd.trainer.RL_TDA import rl_stage_renamed
    rl = {"face_enc.conv_0.w": 1, "face_enc.ph_pred.w": 2, "face_enc.only_rl.w": 3, "rot_green.w": 4, "x.face_enc.y": 5}
    own = ["face_all.conv_0.w", "face_all.ph_pred.w", "rot_green.w", "x.face_all.y"]
    assert rl_stage_renamed(rl, own) == {"face_all.conv_0.w": 1, "x.face_all.y": 5}


def test_checkpoint_name_and_epoch_rule(tmp_path):
    from tgpose_amd import FLAGS
    from tgpose_amd.trainer.RL_TDA import checkpoint_path, saves_checkpoint, CHECKPOINT_KEYS
    old = FLAGS.model_save, FLAGS.save_every
    try:
        FLAGS.model_save = str(tmp_path)
        assert checkpoint_path(3) == str(tmp_path / "rl_tda_model_03.pth")
        assert checkpoint_path(123).endswith("rl_tda_model_123.pth")
        FLAGS.save_every = 1
        assert [saves_checkpoint(e, 4) for e in range(4)] == [True] * 4
        FLAGS.save_every = 3
        assert [e for e in range(7) if saves_checkpoint(e, 7)] == [2, 5, 6]
        assert [e for e in range(6) if saves_checkpoint(e, 6)] == [2, 5]
    finally:
        FLAGS.model_save, FLAGS.save_every = old
    assert CHECKPOINT_KEYS == ('epoch', 'net1_state_dict', 'net2_state_dict', 'optimizer_state_dict', 'scheduler_state_dict')


def test_log_line_has_the_reference_layout():
    """the fixture's log lines, rebuilt from their own numbers, are the same text"""
    import re
    from tgpose_amd.trainer.RL_TDA import log_line
    lines = [l for l in json.loads(str(golden("train_loop.npz")["log"])) if l.startswith("Stage")]
    assert len(lines) == 3
    for l in lines:
        e, b = (int(v) for v in re.match(r"Stage 2 Epoch (\d+) Batch (\d+) ", l).groups())
        vals = [float(v) for v in re.findall(r":(-?\d+\.\d+)", l)]
        assert len(vals) == 14 and log_line(e, b, vals) == l


def test_fixture_draws_are_the_seeded_generators():
    """the reference loop's subsamples are torch.randperm from the seeded CPU generator, net1's pair then net2's per step -- the
    draws engine.draw_sample_idx makes in the same order, so the device loop sees the same subsamples"""
    g = golden("train_loop.npz")
    torch.manual_seed(int(g["forward_seed"]))
    N = int(g["n_points"])
    for j in range(16):
        assert np.array_equal(torch.randperm(N if j % 2 == 0 else N // 4).numpy(), g["draw.%d" % j]), j
    assert g["stepped"].tolist() == [True, True, False, True]
    assert np.isnan(g["loss"][int(g["nan_batch"]) - 1]).any() and not np.isnan(np.delete(g["loss"], 2, 0)).any()


def test_refill_takes_the_next_index():
    """fill_batch: an abandoned item is retried at (index + 1) % n, round after round, and the batch keeps its size"""
    from tgpose_amd.datasets.load_data import fill_batch
    bad = {1, 2, 9}
    calls = []

    def build(idx):
        calls.append(list(idx))
        kept = [k for k, i in enumerate(idx) if i not in bad]
        return (kept, {"rows": [idx[k] for k in kept]}) if kept else None

    parts, at = fill_batch([9, 1, 5, 2], 10, build)
    # round 1 keeps item 5; positions 0, 1, 3 move on to items 0, 2, 3; round 2 keeps 0 and 3; position 1 moves on to item 3
    assert calls == [[9, 1, 5, 2], [0, 2, 3], [3]]
    assert at == [0, 3, 5, 3]
    assert [p for p, _ in parts] == [[2], [0, 3], [1]]
    assert sorted(p for ps, _ in parts for p in ps) == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        fill_batch([0], 2, lambda idx: None)


def test_epoch_order_is_dataloaders():
    """shuffle as DataLoader(shuffle=True) draws it (RandomSampler from torch's generator), batches of the order, the last short
    one kept unless drop_last; ranks take strided slices of the padded order"""
    from tgpose_amd.datasets.load_data import epoch_batches
    g = torch.Generator().manual_seed(5)
    got = epoch_batches(10, 4, gen=g)
    want = [list(b) for b in torch.utils.data.DataLoader(list(range(10)), batch_size=4, shuffle=True,
                                                          generator=torch.Generator().manual_seed(5))]
    assert got == [[int(x) for x in b] for b in want]
    torch.manual_seed(8)
    want = [[int(x) for x in b] for b in torch.utils.data.DataLoader(list(range(10)), batch_size=4, shuffle=True)]
    torch.manual_seed(8)
    assert epoch_batches(10, 4) == want
    assert [len(b) for b in epoch_batches(10, 4, gen=g, drop_last=True)] == [4, 4]
    r0 = epoch_batches(5, 8, shuffle=False, rank=0, world_size=2)
    r1 = epoch_batches(5, 8, shuffle=False, rank=1, world_size=2)
    assert r0 == [[0, 2, 4]] and r1 == [[1, 3, 0]]


def test_train_batches_lengths():
    from tgpose_amd.datasets.load_data import TrainBatches
    tb = TrainBatches([{}] * 10, 4, device="cpu")
    assert len(tb) == 3 and not tb.prefetch
    assert len(TrainBatches([{}] * 10, 4, device="cpu", drop_last=True)) == 2
    assert len(TrainBatches([{}] * 10, 4, device="cpu", rank=1, world_size=3)) == 1


def test_ranks_partition_every_epoch_whatever_they_draw():
    """data parallel: two ranks whose batches consume different amounts of the shared generator (as different items do: point
    counts, operators, refills, subsamples) still split every epoch's items between them, each item once"""
    from tgpose_amd.datasets.load_data import TrainBatches

    class Fake(TrainBatches):
        def build(self, indices):
            torch.rand(len(indices) * (7 + 13 * self.rank) + sum(indices), generator=self.gen)    # data-dependent draws
            return {"item_index": list(indices)}

    n, world = 12, 2
    ranks = []
    for r in range(world):
        torch.manual_seed(0)                             # gen=None: torch's default generator, seeded alike on every rank
        ranks.append(Fake([{}] * n, 2, device="cpu", rank=r, world_size=world))
    seen = [[] for _ in range(3)]
    for e in range(3):
        for tb in ranks:
            for db in tb:
                seen[e] += db["item_index"]
        assert sorted(seen[e]) == list(range(n)), (e, seen[e])
    assert seen[0] != seen[1]                            # still a new order every epoch
    assert ranks[0].order(1) == ranks[0].order(1)       # (no draw: the same order whenever asked)
    ranks[0].set_epoch(1)
    assert [b for b in ranks[0]] and ranks[0].epoch == 2
