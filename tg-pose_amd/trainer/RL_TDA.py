"""Drop-in for ``trainer/RL_TDA.py``: ``RT_TDA_Trainer.RL_TDA_train_step`` (:110-200), the loop ``RL_TDA_train`` (:202-263) and
``train`` (:265-267), and the checkpoint methods ``load_old_model_params`` (:88-97) / ``init_RL_TDA_model`` (:64-86), on the HIP path.

One step is: net1 = PoseNet9D() on the cloud with gradients (tgpose_amd.autograd: HIP forward and backward), net2 =
PoseNet9D(only_encoder=True) on the augmented cloud under ``no_grad`` (the fused training-mode forward of tgpose_amd.engine:
batch-statistics BatchNorm that moves its running statistics), ``feat_consistency_loss`` + two ``prop_sym_matching_loss``
(losses/consistency_loss.py), the fourteen ``control_loss('TDA')`` terms of ``TDA_loss``, and
``total = 0.1 (con + recon_1 + recon_consistency) + 0.9 sum(TDA)`` (:214).  Nothing in it reads a value back from the device,
so forward + loss + backward replay as one hipGraph (``graphed_step``); the gradient exchange between ranks
(tgpose_amd.shard), ``clip_grad_norm_(net1, 5)`` (:223) and the optimizer step stay outside the graph.

The optimizer and its schedule are the reference's (:58-62 ``set_optimizer_scheduler``): Ranger (tgpose_amd.tools.torch_utils.solver.
ranger2020: its step is one HIP launch over every parameter with a gradient) and flat_and_anneal (tgpose_amd.tools.torch_utils.solver.
lr_scheduler), built by tgpose_amd.tools.training_utils from FLAGS; ``setup`` still accepts any ``torch.optim`` optimizer / scheduler.

``RL_TDA_train`` replays the captured step (one capture per batch shape; a batch of another shape -- an epoch's smaller last batch
-- runs the eager ``train_iteration``), applies the loop's NaN skip after the replay through ``finish_step(total=...)``, and, when
the batch source can prefetch (datasets.load_data.TrainBatches), enqueues the next batch's preparation before it reads the step's
NaN flag.  It logs the reference's line every FLAGS.log_every batches and writes the reference's checkpoint file
(``rl_tda_model_{e:02d}.pth``, tensors on the CPU) on rank 0 only.
"""
import math
import os
import time

import torch

from ..config import FLAGS
from ..losses.TDA_loss_sym_recon import TDA_loss
from ..losses.consistency_loss import feat_consistency_loss, prop_sym_matching_loss
from ..network.fs_net_repo.PoseNet9D import PoseNet9D
from .organize_loss import control_loss

PRED_KEYS = ['recon', 'p_green_R', 'p_red_R', 'f_green_R', 'f_red_R', 'Pred_T', 'Pred_s', 'h1', 'h2']


def get_gt_v(Rs, axis=2):
    """tools/training_utils.get_gt_v (bytecode only in the reference): the ground-truth green (y) and red (x) axes"""
    return Rs[:, :, 1].contiguous(), Rs[:, :, 0].contiguous()


def create_network(mode):
    if mode == 'RL_TDA':
        return PoseNet9D(), PoseNet9D(only_encoder=True)
    raise NotImplementedError(mode)


# net2's forward on a second stream beside net1's.  Built in round 3 and left off then (18.45 ms per step against 18.25 serial); on
# the round-5 kernels the branch pays: 16.44 against 17.10 ms per step (same box, alternating runs), so it is the default.  Bit for bit
# the serial step's results (tests/test_gpu_parity.py::test_train_step_with_net2_beside_net1_equals_serial).  TGP_NET2_BESIDE=0: serial.
NET2_BESIDE = os.environ.get("TGP_NET2_BESIDE", "1") != "0"
_TOTAL_W = {}


def total_loss(loss_dict):
    """trainer/RL_TDA.py:209-214: 0.1 (RL + recon_1 + recon_consistency) + 0.9 sum over the TDA terms -- as one concatenation, one
    multiply with the constant weights and one sum (Python's `sum` over seventeen device scalars is ~35 launches forward and ~70
    backward; the value differs from the left-to-right sum by the rounding of a 17-term fp32 sum)."""
    head = [loss_dict[k].reshape(-1) for k in ('RL_loss', 'recon_1_loss', 'recon_consistency_loss') if k in loss_dict]
    tda = [v.reshape(-1) for v in loss_dict['TDA_loss'].values()]
    terms = torch.cat(head + tda)
    key = (terms.device, sum(t.numel() for t in head), terms.numel())
    if key not in _TOTAL_W:          # built once per shape (the first call of a shape is an eager warm-up, outside any capture)
        w = torch.full((key[2],), 0.9)
        w[: key[1]] = 0.1
        _TOTAL_W[key] = w.to(terms.device)
    return (terms * _TOTAL_W[key]).sum()



# ----------------------------------------------------------------------------------------------------------- the loop's files
CHECKPOINT_KEYS = ('epoch', 'net1_state_dict', 'net2_state_dict', 'optimizer_state_dict', 'scheduler_state_dict')   # (:258-262)


def checkpoint_path(epoch):
    """the loop's checkpoint file (:263): ``rl_tda_model_{epoch:02d}.pth`` in FLAGS.model_save"""
    return os.path.join(str(FLAGS.model_save), 'rl_tda_model_{:02d}.pth'.format(epoch))


def saves_checkpoint(epoch, total_epoch):
    """(:257) a checkpoint after every FLAGS.save_every-th epoch (0-based ``epoch``) and after the last one"""
    return (epoch + 1) % FLAGS.save_every == 0 or (epoch + 1) == total_epoch


# the log line of :229-248 as data: (text in front of the value, value) -- the values are read back in one copy
_LOG_FIELDS = (('L:', 'total'), (', con_l:', 'RL_loss'), (',recon_1:', 'recon_1_loss'), (',recon_consist:', 'recon_consistency_loss'),
               (', TDA_l:', 'TDA'), (', rot_l:', 'Rot1+Rot2'), (', size_l:', 'Size'), (', trans_l:', 'Tran'), (', h1_l:', 'TDA_h1'),
               (', h2_l:', 'TDA_h2'), (', h1_l_cate:', 'TDA_h1_cate'), (', h2_l_cate:', 'TDA_h2_cate'),
               (',R_DCD_cate_pred:', 'R_DCD_cate_pred'), (',Prop_sym:', 'Prop_sym'))


def log_values(total, loss_dict):
    """the fourteen numbers of the log line, in its order, with one device-to-host copy"""
    tda = loss_dict['TDA_loss']
    names = list(tda)
    dev = [total.reshape(-1)[:1]] + [loss_dict[k].reshape(-1)[:1] for k in ('RL_loss', 'recon_1_loss', 'recon_consistency_loss')]
    dev += [tda[k].reshape(-1)[:1] for k in names]
    host = torch.cat([v.detach().float().to(dev[0].device) for v in dev]).cpu().tolist()
    t = dict(zip(names, host[4:]))
    val = {'total': host[0], 'RL_loss': host[1], 'recon_1_loss': host[2], 'recon_consistency_loss': host[3],
           'TDA': sum(host[4:]), 'Rot1+Rot2': t['Rot1'] + t['Rot2']}
    return [val[k] if k in val else t[k] for _, k in _LOG_FIELDS]


def log_line(epoch, batch, values):
    """the reference's log line (:229-248) for stage 2: the same labels, separators, order and four decimals"""
    return 'Stage {} Epoch {} Batch {} '.format(2, epoch, batch) + ''.join('{}{:.4f}'.format(label, v) for (label, _), v in zip(_LOG_FIELDS, values))


def rl_stage_renamed(rl_net1_state, own_keys):
    """init_RL_TDA_model's rule (:76-84): every key of an RL-stage net1 that names ``face_enc`` (and not ``ph_pred``) is taken
    as the same key with ``face_all`` -- if this net1 has that key; every other key is dropped.  -> {new key: tensor}"""
    own = set(own_keys)
    out = {}
    for k, v in rl_net1_state.items():
        if 'face_enc' in k and 'ph_pred' not in k:
            nk = k.replace('face_enc', 'face_all')
            if nk in own:
                out[nk] = v
    return out


def _to_cpu(obj):
    """a state dict with every tensor copied to the host (a view is copied alone, not the flat buffer behind it)"""
    if torch.is_tensor(obj):
        return obj.detach().cpu().clone() if obj.device.type == 'cpu' else obj.detach().cpu()
    if isinstance(obj, dict):
        return type(obj)((k, _to_cpu(v)) for k, v in obj.items())
    if isinstance(obj, (list, tuple)):
        return type(obj)(_to_cpu(v) for v in obj)
    return obj


def _rank0():
    import torch.distributed as dist
    return not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0


def _signature(db):
    return tuple(sorted((k, tuple(v.shape), v.dtype) for k, v in db.items() if torch.is_tensor(v)))


class RT_TDA_Trainer(object):
    def __init__(self, logger=None, device=None):
        self.logger = logger
        self.device = torch.device('cuda:0') if device is None else torch.device(device)
        self.net1, self.net2 = None, None
        self.loss_tda_net = None
        self.optimizer = None
        self.scheduler = None
        self._graphed = None          # the last GraphedStep captured over net1 (its static .grad buffers must stay in place)
        self._buckets = None          # shard.GradBuckets of a graphed_step(overlap=True): p.grad are views into its flat buffers
        self._exchanged = False       # set by a replay whose gradient exchange has already run, cleared by finish_step
        self._loop = None             # (batch signature, step) of the capture RL_TDA_train replays
        self._skipped = False         # whether the last train_iteration skipped its step (NaN total)

    def setup(self, mode, optimizer=None, scheduler=None):
        self.init_network(mode)
        self.init_loss()
        self.optimizer, self.scheduler = optimizer, scheduler

    def init_network(self, mode):
        self.net1, self.net2 = create_network(mode)
        self.net1, self.net2 = self.net1.to(self.device), self.net2.to(self.device)

    def init_loss(self):
        self.loss_tda_net = TDA_loss()
        (self.name_fs_list, self.name_recon_list, self.name_geo_list, self.name_prop_list, self.name_TDA_list) = control_loss('TDA')

    def set_optimizer_scheduler(self):
        """trainer/RL_TDA.py:58-62: Ranger over build_params() and flat_and_anneal over train_steps * total_epoch // accumulate
        iterations (finish_step steps both)"""
        from ..tools.training_utils import build_optimizer, build_lr_rate
        self.optimizer = build_optimizer(self.build_params())
        self.scheduler = build_lr_rate(self.optimizer, total_iters=FLAGS.train_steps * FLAGS.total_epoch // FLAGS.accumulate)

    def build_params(self, training_stage_freeze=None):
        return [{"params": filter(lambda p: p.requires_grad, self.net1.parameters()), "lr": float(FLAGS.lr) * FLAGS.lr_pose}]

    # -------------------------------------------------------------------------------------------------------------------
    def losses(self, db, results, results_2, only_TDA=False, gt_pred_flag=False):
        """the loss half of RL_TDA_train_step (:121-178) on tensors already on the device"""
        dev = self.device
        PC = db['pcl_in']
        gt_R, gt_t, sym = db['rotation'], db['translation'], db['sym_info']
        loss_dict = {}
        if not only_TDA:
            recon_1 = results['recon']
            loss_dict['RL_loss'] = feat_consistency_loss(results['feat_global'], results_2['feat_global'])
            loss_dict['recon_1_loss'] = prop_sym_matching_loss(PC, recon_1, gt_R, gt_t, sym)
            loss_dict['recon_consistency_loss'] = 0.2 * prop_sym_matching_loss(recon_1, results_2['recon'], gt_R, gt_t, sym)
        else:
            loss_dict['RL_loss'] = torch.zeros(1, device=dev)
        pred_TDA_list = {'Rot1': results['p_green_R'], 'Rot1_f': results['f_green_R'], 'Rot2': results['p_red_R'],
                         'Rot2_f': results['f_red_R'], 'Recon': results['recon'], 'Tran': results['Pred_T'], 'Size': results['Pred_s'],
                         'TDA_h1': results['h1'], 'TDA_h2': results['h2']}
        gt_green_v, gt_red_v = get_gt_v(gt_R)
        gt_TDA_list = {'Rot1': gt_green_v, 'Rot2': gt_red_v, 'Recon': PC, 'Tran': gt_t, 'Size': db['fsnet_scale'], 'h1': db['pdh1'],
                       'h2': db['pdh2'], 'proto': None, 'pdh1_category': db['pdh1_category'], 'pdh2_category': db['pdh2_category'],
                       'points_category': db['points_category'], 'R': gt_R}
        loss_dict['TDA_loss'] = self.loss_tda_net(self.name_TDA_list, pred_TDA_list, gt_TDA_list, sym, gt_pred_flag)
        return loss_dict

    def RL_TDA_train_step(self, db, only_TDA=False, gt_pred_flag=False, *, sample_idx=None, inject=None, cut=None):
        """trainer/RL_TDA.py:110-200.  db: the loader's batch dict (tensors on any device).  sample_idx: optionally the
        subsamples of the two forwards, [(pool_1, pool_2) of net1, (pool_1, pool_2) of net2] (drawn from torch's global CPU
        generator in that order otherwise, as the reference does); inject: neighbour graphs for parity tests."""
        dev = self.device
        db = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in db.items()}
        PC, obj_id = db['pcl_in'], db['cat_id']
        FLAGS.train = 1                                           # the trainer runs with FLAGS.train set (engine/train.py)
        s = sample_idx if sample_idx is not None else [None, None]
        results_2 = None
        beside = NET2_BESIDE and not only_TDA and dev.type == 'cuda'
        if beside:
            # net2 (no gradients, its own cloud) shares nothing with net1 until the losses: it runs on a second stream -- in a
            # captured step a parallel branch of the graph -- and fills the gaps between net1's chains of small launches.  The
            # subsamples are drawn up front in the reference's order (net1's two, then net2's: gcn3d.py:241-242).
            from .. import engine
            s = [x if x is not None else engine.draw_sample_idx(n) for x, n in zip(s, (PC.shape[1], db['aug_pcl_in'].shape[1]))]
            cur, side = torch.cuda.current_stream(dev), engine._side_stream(dev, ("train", "net2"))
            fork = torch.cuda.Event()
            fork.record(cur)
            with torch.cuda.stream(side):
                side.wait_event(fork)
                with torch.no_grad():
                    results_2 = self.net2(db['aug_pcl_in'], obj_id, sample_idx=s[1], inject=inject)
                join = torch.cuda.Event()
                join.record(side)
            if not torch.cuda.is_current_stream_capturing():      # (a captured graph owns its pool: nothing to protect)
                db['aug_pcl_in'].record_stream(side), obj_id.record_stream(side)
        results = self.net1(PC, obj_id, sample_idx=s[0], inject=inject, cut=cut)
        if beside:
            cur.wait_event(join)
            if not torch.cuda.is_current_stream_capturing():
                for t in results_2.values():
                    if torch.is_tensor(t):
                        t.record_stream(cur)
        elif not only_TDA:
            with torch.no_grad():
                results_2 = self.net2(db['aug_pcl_in'], obj_id, sample_idx=s[1], inject=inject)
        loss_dict = self.losses(db, results, results_2, only_TDA, gt_pred_flag)
        output_dict = {'enc_feat_1': results['feat_global'], 'PC': PC, 'obj_id': obj_id, 'gt_R': db['rotation'],
                       'gt_t': db['translation'], 'gt_s': db['fsnet_scale'], 'gt_h1': db['pdh1'], 'gt_h2': db['pdh2'], 'sem_pro': None}
        if not only_TDA:
            output_dict['enc_feat_2'] = results_2['feat_global']
        for key in PRED_KEYS:
            output_dict[key] = results[key]
        return output_dict, loss_dict

    # -------------------------------------------------------------------------------------------------------------------
    def loss_is_nan(self, total, n_alive=None):
        """the loop's NaN test (:217-220) -- one host read of the device scalar.  Data parallel: the ranks must skip or step
        TOGETHER (a rank that skipped would miss the collective the others wait in), so the flag is max-reduced first.
        n_alive (a draws='device' batch's count of slots that hold an item of their own, a device int32): read in the same host
        copy; a batch without an alive item counts as a NaN step, and ``last_n_alive`` keeps the count for the loop."""
        import torch.distributed as dist
        bad = torch.isnan(total.detach()).reshape(-1).any().to(torch.int32)
        if n_alive is not None:
            bad = torch.maximum(bad, (n_alive.reshape(-1)[0] == 0).to(torch.int32))
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            bad = bad.to(self.device) if dist.get_backend() == "nccl" else bad.cpu()
            dist.all_reduce(bad, op=dist.ReduceOp.MAX)
        if n_alive is None:
            self.last_n_alive = None
            return bool(bad.item())
        flag, self.last_n_alive = torch.stack([bad.to(n_alive.device).reshape(()), n_alive.reshape(-1)[0].to(torch.int32)]).tolist()
        return bool(flag)

    def finish_step(self, total=None, n_alive=None):
        """what follows total_loss.backward() in the loop (:223-226), with the data-parallel gradient exchange in front: the
        clip must see the averaged gradients.  After a graphed_step(overlap=True) replay the exchange has already
        run (bucket by bucket, overlapped with the backward): the replay says so through ``_exchanged``.

        total: the replayed step's loss (graphed_step's return value).  When given, the reference's NaN test (:217-220) is
        applied here -- a captured step has run its backward before anyone can look at the loss, so a NaN step is undone by
        zeroing the gradients instead of skipping backward(): no clip, no optimizer / scheduler step, weights untouched.
        Returns False for such a skipped step."""
        from .. import shard
        if total is not None and self.loss_is_nan(total, n_alive):
            print('Found nan in total loss' if self.last_n_alive != 0 else 'No alive item in the batch')
            self._exchanged = False
            grads = [p.grad for p in self.net1.parameters() if p.grad is not None]
            if grads:
                torch._foreach_zero_(grads)
            return False
        if not self._exchanged:
            shard.allreduce_gradients(self.net1.parameters())
        self._exchanged = False
        torch.nn.utils.clip_grad_norm_(self.net1.parameters(), 5)
        if self.optimizer is not None:
            self.optimizer.step()
        if self.scheduler is not None:
            self.scheduler.step()
        return True

    def train_iteration(self, db):
        """one eager iteration of RL_TDA_train's loop body (:205-226); returns (total loss, loss_dict).  A NaN total skips
        backward, clip and the optimizer step, as the reference's loop does (:217-220)."""
        if self.optimizer is not None:
            # once a captured step or flat gradient buckets exist, .grad tensors are static storage: zero them in place
            self.optimizer.zero_grad(set_to_none=self._graphed is None and self._buckets is None)
        _, loss_dict = self.RL_TDA_train_step(db)
        total = total_loss(loss_dict)
        self._skipped = self.loss_is_nan(total, db.get('n_alive'))
        if self._skipped:
            print('Found nan in total loss' if self.last_n_alive != 0 else 'No alive item in the batch')
            return total.detach(), loss_dict
        total.backward()
        self._exchanged = False
        self.finish_step()
        return total.detach(), loss_dict

    def graphed_step(self, db, overlap=False, _debug=""):
        """Capture forward (both nets) + losses + backward for batches of db's shapes as hipGraphs; returns a callable
        ``step(db=None, sample_idx=None) -> total loss`` that copies a new batch into the static buffers, replays, and leaves the
        gradients in net1's ``.grad`` buffers; then call ``finish_step(total=loss)``, which applies the loop's NaN test
        (:217-220) to the returned device scalar and skips clip + optimizer for a NaN step (``finish_step()`` without the loss
        steps unconditionally and reads nothing back).

        overlap=True (the data-parallel form): the backward is captured in two segments split at the encoder's output, net1's
        gradients live in two flat buckets (shard.GradBuckets), and the exchange of the late layers' bucket (84 of 97 MB) is
        started between the segments, so it runs while the encoder's backward computes; the encoder's bucket follows.  With one
        process the exchanges are no-ops and the step computes exactly what overlap=False computes."""
        from ..autograd import GraphedStep, EncoderCut, LATE_PREFIXES
        from .. import shard
        dev = self.device
        static = {k: v.to(dev).clone() for k, v in db.items() if torch.is_tensor(v)}
        N = static['pcl_in'].shape[1]
        cut = EncoderCut() if (overlap and "nocut" not in _debug) else None
        pending = []
        terms = {}

        def step_fn(samples):
            _, loss_dict = self.RL_TDA_train_step(static, sample_idx=samples, cut=cut)
            # the loss terms of the captured run stay allocated: every replay rewrites them (the loop's log line reads them)
            terms.clear()
            terms.update({k: (v.detach() if torch.is_tensor(v) else {kk: vv.detach() for kk, vv in v.items()})
                          for k, v in loss_dict.items()})
            return total_loss(loss_dict)

        between = after = None
        if overlap and "nobuckets" not in _debug:
            self._buckets = buckets = shard.GradBuckets(self.net1.named_parameters(), LATE_PREFIXES)

            def between():
                # reduce-scatter, the shard's average and the all-gather of the late bucket are all enqueued here, on the
                # exchange stream: the whole exchange travels while the encoder's backward (graph 2) computes
                pending.append(buckets.reduce(0))

            def after():
                pending.append(buckets.reduce(1))
                while pending:
                    buckets.wait(pending.pop(0))
                self._exchanged = True                            # finish_step must not exchange again
        else:
            self._buckets = None                                  # an earlier overlap capture's buckets no longer describe this step

        g = GraphedStep(list(self.net1.parameters()), step_fn, [N, N], dev, cut=cut, between=between, after=after,
                        own_pool="ownpool" in _debug, buckets=self._buckets)
        self._graphed = g

        def step(db=None, sample_idx=None):
            if db is not None:
                for k, v in db.items():
                    if torch.is_tensor(v):
                        static[k].copy_(v.reshape(static[k].shape), non_blocking=True)
            return g(sample_idx)
        step.graph = g
        step.loss_dict = terms
        return step

    # ------------------------------------------------------------------------------------------------------------ the loop
    def _loop_step(self, db, overlap):
        """the captured step RL_TDA_train replays for batches of db's shapes; None for a batch of another shape (it runs eagerly).
        The capture's warm-up runs both forwards twice and draws subsamples: the BatchNorm buffers and torch's CPU generator are put
        back as they were, so the loop's state equals the eager loop's."""
        sig = _signature(db)
        if self._loop is None:
            rng = torch.get_rng_state()
            keep = [{k: v.detach().clone() for k, v in net.state_dict().items()} for net in (self.net1, self.net2)]
            step = self.graphed_step(db, overlap=overlap)
            for net, sd in zip((self.net1, self.net2), keep):
                net.load_state_dict(sd)
            torch.set_rng_state(rng)
            self._loop = (sig, step)
        return self._loop[1] if self._loop[0] == sig else None

    def RL_TDA_train(self, train_dataloader, total_epoch, graph=True, overlap=None):
        """trainer/RL_TDA.py:202-263.  train_dataloader: any iterable of batch dicts (datasets.load_data.TrainBatches, a
        DataLoader, a list).  Per batch: the step, then -- unless its total is NaN -- clip_grad_norm_(net1, 5), the optimizer, the
        scheduler.  Every FLAGS.log_every batches (1-based) the reference's log line goes to self.logger; after the epochs that
        saves_checkpoint names, checkpoint_path(e) gets the reference's five keys with every tensor on the CPU.  Rank 0 alone logs
        and writes; the ranks skip a NaN step together (loss_is_nan).

        graph=True replays the step captured at the first batch (graphed_step; overlap: its data-parallel form, by default when
        more than one rank runs) and applies the NaN skip in finish_step(total=...); a batch of another shape runs the eager
        train_iteration.  graph=False runs train_iteration for every batch.  When the iterator has ``prefetch()``, it is called
        after the step is enqueued and before its NaN flag is read: the next batch is prepared while the step runs."""
        import torch.distributed as dist
        rank0 = _rank0()
        if overlap is None:
            overlap = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        for e in range(total_epoch):
            epoch_s_time = time.time()
            batches = iter(train_dataloader)
            prefetch = getattr(batches, 'prefetch', None)
            partial = None                       # draws='device' batches: how many trained with fewer alive items than slots
            for i, data in enumerate(batches, 1):
                iter_s_time = time.time()
                step = self._loop_step(data, overlap) if graph else None
                n_alive = data.get('n_alive') if isinstance(data, dict) else None
                if step is not None:
                    total = step(data)
                    if prefetch is not None:
                        prefetch()
                    stepped = self.finish_step(total=total, n_alive=n_alive) if n_alive is not None else self.finish_step(total=total)
                    loss_dict = step.loss_dict
                else:
                    total, loss_dict = self.train_iteration(data)
                    if prefetch is not None:
                        prefetch()
                    stepped = not self._skipped
                if n_alive is not None:
                    partial = (partial or 0) + (0 < self.last_n_alive < data['pcl_in'].shape[0])
                if stepped and i % FLAGS.log_every == 0 and rank0 and self.logger is not None:
                    self.logger.info(log_line(e, i, log_values(total, loss_dict)))
                    self.logger.info('The average running time of every {} is {:.4f} sec'.format(FLAGS.log_every, time.time() - iter_s_time))
                del total, loss_dict, data          # an eager step's autograd graph must not outlive it
            if rank0 and self.logger is not None:
                self.logger.info('>>>>>>>>----------Epoch {:02d} train finish,time is {:02f} sec---------<<<<<<<<'.format(
                    e, time.time() - epoch_s_time))
                if partial is not None:
                    self.logger.info('Epoch {:02d}: {} batches trained with fewer alive items than slots'.format(e, partial))
            if rank0 and saves_checkpoint(e, total_epoch):
                self.save_checkpoint(e)

    def train(self, train_dataloader, mode):
        """(:265-267) the reference hard-codes 150 epochs, FLAGS.total_epoch's default"""
        if mode == 'RL_TDA':
            self.RL_TDA_train(train_dataloader, FLAGS.total_epoch)

    def checkpoint(self, epoch):
        """the reference's checkpoint dict (:258-262) with every tensor copied to the host"""
        return _to_cpu({'epoch': epoch, 'net1_state_dict': self.net1.state_dict(), 'net2_state_dict': self.net2.state_dict(),
                        'optimizer_state_dict': self.optimizer.state_dict(), 'scheduler_state_dict': self.scheduler.state_dict()})

    def save_checkpoint(self, epoch, path=None):
        path = checkpoint_path(epoch) if path is None else path
        d = os.path.dirname(path)
        if d:
            os.makedirs(d, exist_ok=True)
        torch.save(self.checkpoint(epoch), path)
        return path

    def load_old_model_params(self, path, mode):
        """(:88-97) net1, net2, the optimizer and -- when the file has it -- the scheduler from a checkpoint of RL_TDA_train (this
        package's or the reference's; tensors saved on any device are read on the host first).  Everything is copied into the
        existing tensors: parameters, BatchNorm buffers and the static .grad buffers keep their storage, and Ranger flattens the
        loaded state again at its next step (its buffer is outside the graph).  net2's captured forward, however, reads the
        kernel-ready copy of its weights packed when the step was captured (PoseNet9D.packed), which a load cannot reach: the loop's
        capture is dropped and RL_TDA_train captures again at its next batch (a step the caller captured with graphed_step must be
        captured again as well)."""
        checkpoint = torch.load(path, map_location='cpu')
        self._loop = None
        if mode == 'RL_TDA':
            if self.net1 is not None:
                self.net1.load_state_dict(checkpoint['net1_state_dict'])
            if self.net2 is not None:
                self.net2.load_state_dict(checkpoint['net2_state_dict'])
            self.optimizer.load_state_dict(checkpoint['optimizer_state_dict'])
            if 'scheduler_state_dict' in checkpoint:
                self.scheduler.load_state_dict(checkpoint['scheduler_state_dict'])
        return checkpoint.get('epoch')

    def init_RL_TDA_model(self, model_path):
        """(:64-86) net1 from an RL-stage checkpoint: its ``face_enc`` weights become this net1's ``face_all`` ones
        (rl_stage_renamed); the rest of net1 keeps its values"""
        if self.logger is not None:
            self.logger.info('[RT_TDA] loading model from {} '.format(model_path))
        checkpoint = torch.load(model_path, map_location='cpu')
        self._loop = None                   # (as in load_old_model_params)
        own = self.net1.state_dict()
        upd = rl_stage_renamed(checkpoint['net1_state_dict'], own.keys())
        for k in upd:
            print('update {} to {}'.format(k.replace('face_all', 'face_enc'), k))
        own.update(upd)
        self.net1.load_state_dict(own)
        return sorted(upd)
