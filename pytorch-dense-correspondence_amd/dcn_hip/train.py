"""Training from a frame store with no host read: the reference's ``DenseCorrespondenceTraining.run()``
(dense_correspondence/training/training.py:228-456) over a ``dcn_hip.frames.FrameStore``.

The reference skips an iteration whose sample is empty (training.py:304-306): no ``zero_grad``, no learning-rate adjustment,
no forward pass, no optimizer step, no logging.  Whether a batch drawn on the device is empty is known on the device only, so
the decision is taken there (csrc/train_kernels.hip, include/dcn_hip.h section 13): ``TrainState.advance`` sets ``active`` and
applies the schedule (``adjust_learning_rate``, :544-558, runs after the ``continue``: a decay boundary on an empty iteration is
NOT applied), ``GuardedAdam.step`` updates nothing when the iteration is inactive, the batch-norm buffers the forward pass of
such an iteration has changed are put back, and the log is a row of a device tensor instead of five ``.item()`` calls.  The
host reads the state at save points only.

``Validation`` is what the reference's ``compute_test_loss`` hook (training.py:427-441; dead code there) was for: every
``rate`` iterations a held-out store is evaluated (``evaluate.evaluate_frame_pairs``) and reduced on the device to the
reference's curves (``evaluate.evaluation_curves``, csrc/curve_kernels.hip): eight numbers per curve in a row of a second
device history, read with the log at save points."""
import ctypes
import logging
import os

import numpy as np
import torch

from . import _lib, evaluate, frames
from .optim import GuardedAdam

STATE_WORDS = 6                      # struct dcn_train_state: 48 bytes
LOG_COLUMNS = 16                     # DCN_TRAIN_LOG_COLUMNS
TERM_KEYS = ("loss", "match_loss", "masked_non_match_loss", "background_non_match_loss", "blind_non_match_loss")
TYPE_NAMES = ("SINGLE_OBJECT_WITHIN_SCENE", "SINGLE_OBJECT_ACROSS_SCENE", "DIFFERENT_OBJECT", "MULTI_OBJECT",
              "SYNTHETIC_MULTI_OBJECT")


class StateSnapshot(object):
    """One read of the state block and of the history rows written so far (``TrainState.read()``)."""

    def __init__(self, words, history):
        self.active = int(words[:1].view(np.int32)[0])
        self.t = int(words[1])
        self.lr = float(words[2:3].view(np.float64)[0])
        f = words[3:4].view(np.float32)
        self.step_size, self.bc2_sqrt = float(f[0]), float(f[1])
        self.num_active, self.num_skipped = int(words[4]), int(words[5])
        self.history = history          # float64 [rows, LOG_COLUMNS]


class TrainState(object):
    """The device-resident training state (struct dcn_train_state) and the history tensor behind it, in ONE device buffer so
    that ``read()`` is one copy.  ``betas`` are Adam's: ``advance`` computes the bias corrections of the step it counts."""

    def __init__(self, device, learning_rate, steps_between_learning_rate_decay, learning_rate_decay, betas=(0.9, 0.999),
                 rows=1024):
        self.device = torch.device(device)
        self.steps_between_decay = int(steps_between_learning_rate_decay)
        self.decay = float(learning_rate_decay)
        self.betas = (float(betas[0]), float(betas[1]))
        if self.steps_between_decay < 1:
            raise ValueError("steps_between_learning_rate_decay must be >= 1")
        self.capacity = max(int(rows), 1)
        self.buf = torch.zeros(STATE_WORDS + self.capacity * LOG_COLUMNS, dtype=torch.int64, device=self.device)
        _lib.require_device(self.buf)
        self.rows = 0
        self._bn = None
        self.seed(0, float(learning_rate))

    # ---- the block
    def state_ptr(self):
        return self.buf.data_ptr()

    def _history_ptr(self):
        return self.buf.data_ptr() + 8 * STATE_WORDS

    def seed(self, t, lr):
        """Set the Adam step count and the learning rate (a start, or a loaded checkpoint).  Stream-ordered, no read."""
        self.buf[1:2].fill_(int(t))
        self.buf[2:3].view(torch.float64).fill_(float(lr))

    def _ensure_rows(self, rows):
        if rows <= self.capacity:
            return
        cap = max(rows, 2 * self.capacity)
        buf = torch.zeros(STATE_WORDS + cap * LOG_COLUMNS, dtype=torch.int64, device=self.device)
        buf[:self.buf.numel()].copy_(self.buf)      # device to device, stream-ordered
        self.buf, self.capacity = buf, cap

    def _check_types(self, types):
        if not torch.is_tensor(types) or types.dtype != torch.int32:
            raise TypeError("types must be an int32 tensor (SampleBatch.type), got %s"
                            % (types.dtype if torch.is_tensor(types) else type(types).__name__))
        if types.device != self.buf.device:
            raise ValueError("types is on %s, the training state on %s" % (types.device, self.buf.device))
        if types.dim() != 1 or types.numel() < 1 or not types.is_contiguous():
            raise ValueError("types must be a contiguous 1-D tensor with one entry per pair")

    # ---- the iteration
    def advance(self, types, iteration):
        """Before the forward pass: active = any(types != -1); if active, the learning-rate decay of this iteration and Adam's
        next step count with its bias corrections."""
        self._check_types(types)
        rc = _lib.get().dcn_train_advance(ctypes.c_void_p(self.state_ptr()), _lib.ptr(types), int(types.numel()), int(iteration),
                                          self.steps_between_decay, self.decay, self.betas[0], self.betas[1], _lib.stream_ptr())
        _lib.check(rc, "dcn_train_advance")

    def _check_types_all(self, types_all):
        if not torch.is_tensor(types_all) or types_all.dtype != torch.int32:
            raise TypeError("types_all must be an int32 tensor [G, B] (every rank's SampleBatch.type), got %s"
                            % (types_all.dtype if torch.is_tensor(types_all) else type(types_all).__name__))
        if types_all.device != self.buf.device:
            raise ValueError("types_all is on %s, the training state on %s" % (types_all.device, self.buf.device))
        if types_all.dim() != 2 or types_all.numel() < 1 or not types_all.is_contiguous():
            raise ValueError("types_all must be a contiguous tensor [G, B]: one row per rank, one entry per pair")
        return int(types_all.shape[0]), int(types_all.shape[1])

    def advance_ranks(self, types_all, rank, weight_out, iteration):
        """``advance`` for G data-parallel ranks: active = any pair of ANY rank is not empty (types_all int32 [G, B], gathered
        in rank order), the same schedule and step count on every rank; weight_out (one device float) receives this rank's
        share n_rank / N of the non-empty pairs, 0 when there is none."""
        G, B = self._check_types_all(types_all)
        if not torch.is_tensor(weight_out) or weight_out.dtype != torch.float32 or weight_out.numel() != 1 \
                or weight_out.device != self.buf.device:
            raise ValueError("weight_out: one float32 on %s" % self.buf.device)
        if not 0 <= int(rank) < G:
            raise ValueError("rank %d of %d" % (rank, G))
        rc = _lib.get().dcn_train_advance_ranks(ctypes.c_void_p(self.state_ptr()), _lib.ptr(types_all), G, B, int(rank),
                                                _lib.ptr(weight_out), int(iteration), self.steps_between_decay, self.decay,
                                                self.betas[0], self.betas[1], _lib.stream_ptr())
        _lib.check(rc, "dcn_train_advance_ranks")

    def _bn_tables(self, dcn):
        bufs = list(dcn.buffers())
        bn = self._bn
        if bn is None or len(bn["bufs"]) != len(bufs) or any(a is not b for a, b in zip(bn["bufs"], bufs)) \
                or any(s.shape != b.shape or s.dtype != b.dtype or s.device != b.device for s, b in zip(bn["snap"], bufs)):
            for b in bufs:
                if not b.is_contiguous() or (b.numel() * b.element_size()) % 4:
                    raise ValueError("batch-norm buffers must be contiguous with a whole number of 32-bit words")
            _lib.require_device(*bufs)
            bn = self._bn = {"bufs": bufs, "snap": [torch.empty_like(b) for b in bufs],
                             "bytes": (ctypes.c_int64 * len(bufs))(*[b.numel() * b.element_size() for b in bufs])}
        n = len(bufs)
        live = (ctypes.c_void_p * n)(*[b.data_ptr() for b in bufs])
        snap = (ctypes.c_void_p * n)(*[s.data_ptr() for s in bn["snap"]])
        return n, live, snap, bn["bytes"]

    def snapshot_bn(self, dcn):
        """Before the forward pass: copy every buffer of ``dcn`` (running_mean, running_var, num_batches_tracked)."""
        n, live, snap, nbytes = self._bn_tables(dcn)
        if n:
            _lib.check(_lib.get().dcn_guarded_copy(n, snap, live, nbytes, None, 0, _lib.stream_ptr()), "dcn_guarded_copy")

    def restore_bn_if_skipped(self, dcn):
        """After the forward pass: put the snapshot back when the iteration is inactive (decided on the device)."""
        n, live, snap, nbytes = self._bn_tables(dcn)
        if n:
            _lib.check(_lib.get().dcn_guarded_copy(n, live, snap, nbytes, ctypes.c_void_p(self.state_ptr()), 0,
                                                   _lib.stream_ptr()), "dcn_guarded_copy")

    def log(self, iteration, loss, terms, types):
        """One history row: iteration, active, lr, num_valid, loss, (mean, count) of the five terms over the pairs whose type
        composes them, type of the first non-empty pair."""
        self._check_types(types)
        B = int(types.numel())
        if loss.dtype != torch.float32 or terms.dtype != torch.float32 or tuple(terms.shape) != (B, 5) \
                or not terms.is_contiguous() or loss.numel() != 1:
            raise ValueError("loss: one float32, terms: contiguous float32 [B, 5]")
        _lib.require_device(loss, terms, types)
        self._ensure_rows(self.rows + 1)
        rc = _lib.get().dcn_train_log(ctypes.c_void_p(self._history_ptr()), self.rows, int(iteration),
                                      ctypes.c_void_p(self.state_ptr()), _lib.ptr(loss.detach()), _lib.ptr(terms.detach()),
                                      _lib.ptr(types), B, _lib.stream_ptr())
        _lib.check(rc, "dcn_train_log")
        self.rows += 1

    def log_ranks(self, iteration, gathered, types_all):
        """``log`` over the global batch of G ranks: gathered float32 [G, 1 + 5 B] (every rank's weighted loss, then its terms),
        types_all int32 [G, B], both in rank order.  Column 4 is the sum of the weighted losses: the loss of the global batch."""
        G, B = self._check_types_all(types_all)
        if not torch.is_tensor(gathered) or gathered.dtype != torch.float32 or tuple(gathered.shape) != (G, 1 + 5 * B) \
                or not gathered.is_contiguous():
            raise ValueError("gathered: contiguous float32 [G, 1 + 5 B] = [%d, %d]" % (G, 1 + 5 * B))
        _lib.require_device(gathered, types_all)
        self._ensure_rows(self.rows + 1)
        rc = _lib.get().dcn_train_log_ranks(ctypes.c_void_p(self._history_ptr()), self.rows, int(iteration),
                                            ctypes.c_void_p(self.state_ptr()), _lib.ptr(gathered), _lib.ptr(types_all), G, B,
                                            _lib.stream_ptr())
        _lib.check(rc, "dcn_train_log_ranks")
        self.rows += 1

    # ---- the host's reads
    def read(self):
        """ONE copy to the host: the state block and the history rows so far -> StateSnapshot."""
        words = self.buf[:STATE_WORDS + self.rows * LOG_COLUMNS].cpu().numpy()
        return StateSnapshot(words[:STATE_WORDS], words[STATE_WORDS:].view(np.float64).reshape(self.rows, LOG_COLUMNS).copy())

    def read_step_and_lr(self):
        s = StateSnapshot(self.buf[:STATE_WORDS].cpu().numpy(), None)
        return s.t, s.lr


def empty_logging_dict():
    """training.py:272-281"""
    return {"train": {"iteration": [], "loss": [], "match_loss": [], "masked_non_match_loss": [],
                      "background_non_match_loss": [], "blind_non_match_loss": [], "learning_rate": [],
                      "different_object_non_match_loss": []},
            "test": {"iteration": [], "loss": [], "match_loss": [], "non_match_loss": []}}


def log_calls(row):
    """What ``update_plots`` (training.py:353-413) does for one ACTIVE history row: ([(train key, value) appended to the
    logging dict], [(tensorboard name, value) passed to log_value]), in the reference's order.  A term is there when its count
    is > 0 (the type rule in place of ``is_zero_loss``); the data type is the first non-empty pair's (``metadata['type'][0]``).
    As in the reference, only learning_rate, match_loss, masked_non_match_loss and background_non_match_loss reach the dict."""
    lr, loss, dt = float(row[2]), float(row[4]), int(row[15])
    mean = lambda k: float(row[5 + 2 * k])
    has = lambda k: row[6 + 2 * k] > 0
    appends, board = [("learning_rate", lr)], [("learning rate", lr)]
    for k, name in ((1, "train match loss"), (2, "train masked non match loss"), (3, "train background non match loss")):
        if has(k):
            appends.append((TERM_KEYS[k], mean(k)))
            board.append((name, mean(k)))
    if has(4):
        if dt == 0:
            board.append(("train blind SINGLE_OBJECT_WITHIN_SCENE", mean(4)))
        if dt == 2:
            board.append(("train blind DIFFERENT_OBJECT", mean(4)))
    if not 0 <= dt < len(TYPE_NAMES):
        raise ValueError("unknown data type")
    board.append(("train loss " + TYPE_NAMES[dt], loss))
    if dt == 2:
        board.append(("train different object", loss))
    return appends, board


VALIDATION_HEAD = 4                  # a validation row: iteration, active, the table's status, the curves' status, [C][8]


def validation_key(field):
    """The logging dict's key for a field's area above the curve; stats.yaml's name for ``norm_diff_pred_3d``"""
    return "norm_diff_3d_area_above_curve" if field == "norm_diff_pred_3d" else field + "_area_above_curve"


class Validation(object):
    """A held-out ``FrameStore`` evaluated while training (``StoreTrainer(..., validation=...)``): after iteration ``it`` with
    ``it % rate == 0 and it > after`` (the reference's condition for its test loss, training.py:428), ``num_image_pairs`` pairs
    by ``evaluate.choose_pairs`` with this object's OWN ``host_rng``, ``evaluate.evaluate_frame_pairs`` with its OWN
    ``generator`` (eval mode; ``dcn.training`` and the batch-norm buffers are left as found) and ``evaluate.evaluation_curves``
    of ``fields`` over ``num_bins`` bins, the summaries written straight into the next row of ``history``: float64
    [rows, 4 + 8 C] on the device -- iteration, ``active`` of that iteration (copied from the training state on the device),
    the table's status word, the curves' status word, then evaluate.CURVE_SUMMARY per field.  Nothing is read back; the
    training's generator and ``host_rng`` are not touched."""

    def __init__(self, store, rate, num_image_pairs=25, num_matches_per_image_pair=100, fields=evaluate.CURVE_FIELDS,
                 num_bins=100, after=5, generator=None, host_rng=None, batch_pairs=8):
        self.store, self.rate, self.after = store, int(rate), int(after)
        self.num_image_pairs, self.num_matches = int(num_image_pairs), int(num_matches_per_image_pair)
        self.fields, self.num_bins, self.batch_pairs = tuple(fields), int(num_bins), int(batch_pairs)
        self.generator, self.host_rng = generator, host_rng
        if self.rate < 1:
            raise ValueError("Validation: rate must be >= 1, got %d" % self.rate)
        if not 1 <= self.num_image_pairs <= 1024:
            raise ValueError("Validation: num_image_pairs must be 1 .. 1024, got %d" % self.num_image_pairs)
        unknown = [f for f in self.fields if f not in evaluate.COLUMNS]
        if unknown or not 1 <= len(self.fields) <= evaluate.MAX_CURVES:
            raise ValueError("Validation: 1 .. %d fields out of evaluate.COLUMNS, got %s" % (evaluate.MAX_CURVES, self.fields))
        if not 2 <= self.num_bins <= evaluate.MAX_CURVE_BINS:
            raise ValueError("Validation: num_bins must be 2 .. %d, got %d" % (evaluate.MAX_CURVE_BINS, self.num_bins))
        self.width = VALIDATION_HEAD + len(self.fields) * len(evaluate.CURVE_SUMMARY)
        self.history = torch.zeros((16, self.width), dtype=torch.float64, device=store.device)
        self.rows = 0

    def due(self, iteration):
        return iteration % self.rate == 0 and iteration > self.after

    def _next_row(self):
        if self.rows == self.history.shape[0]:
            grown = torch.zeros((2 * self.rows, self.width), dtype=torch.float64, device=self.history.device)
            grown[:self.rows].copy_(self.history)       # device to device, stream-ordered
            self.history = grown
        return self.history[self.rows]

    def run(self, dcn, state, iteration):
        """One pass after iteration ``iteration`` of the training ``state`` (a TrainState) -> the EvalCurves, on the device."""
        chosen = evaluate.choose_pairs(self.store, self.num_image_pairs, self.host_rng)
        row = self._next_row()
        row[0:1].fill_(float(iteration))
        row[1:2].copy_(state.buf[:1].view(torch.int32)[:1])          # struct dcn_train_state.active, on the device
        if chosen.shape[0] == 0:                 # no two frames far enough apart: a table without rows, every curve empty
            summary = row[VALIDATION_HEAD:].view(len(self.fields), len(evaluate.CURVE_SUMMARY))
            summary.fill_(float("nan"))
            summary[:, :2].fill_(0.0)
            summary[:, 7].fill_(float(evaluate.CURVE_EMPTY))
            row[2:3].fill_(0.0)
            row[3:4].fill_(float(evaluate.CURVE_EMPTY))
            self.rows += 1
            return None
        table = evaluate.evaluate_frame_pairs(dcn, self.store, chosen, self.num_matches, generator=self.generator,
                                              batch_pairs=self.batch_pairs)
        C = len(self.fields)
        curves = evaluate.evaluation_curves(table, self.fields, self.num_bins,
                                            out_summary=row[VALIDATION_HEAD:].view(C, len(evaluate.CURVE_SUMMARY)))
        row[2:3].copy_(table.status)
        row[3:4].copy_(curves.status)
        self.rows += 1
        return curves

    def read(self):
        """ONE copy to the host: the rows so far, float64 [rows, 4 + 8 C]"""
        return self.history[:self.rows].cpu().numpy()

    def logging_dict(self, rows):
        """``logging_dict["validation"]`` of the rows read: the iterations that counted (``active``), per field the area above
        the curve and the number of values behind it"""
        d = {"iteration": []}
        for f in self.fields:
            d[validation_key(f)] = []
            d[f + "_count"] = []
        for row in rows:
            if row[1] == 0:
                continue
            d["iteration"].append(int(row[0]))
            for k, f in enumerate(self.fields):
                s = row[VALIDATION_HEAD + 8 * k:VALIDATION_HEAD + 8 * (k + 1)]
                d[validation_key(f)].append(float(s[6]))
                d[f + "_count"].append(int(s[0]))
        return d


def logging_dict_from_history(history):
    d = empty_logging_dict()
    for row in history:
        if row[1] != 0:
            for key, value in log_calls(row)[0]:
                d["train"][key].append(value)
    return d


class StoreTrainer(object):
    """The reference's ``run()`` over a ``FrameStore``.  ``config``: the reference's training.yaml dict (keys used, under
    ``training``: learning_rate, learning_rate_decay, steps_between_learning_rate_decay, weight_decay, num_iterations,
    batch_size, logging_rate, save_rate, data_type_probabilities and the sampling keys ``draw_training_batch`` reads).

    Every iteration: draw_training_batch, TrainState.advance, zero_grad, batch-norm snapshot, forward_pair, get_loss_mixed,
    backward, GuardedAdam.step(state), guarded batch-norm restore, TrainState.log.  Between save points the host reads nothing.

    An INACTIVE iteration (every pair of the batch empty) still costs a forward and a backward pass: with the host out of the
    loop there is no way to know before they are enqueued, and such iterations are rare.  Their effects are undone or withheld
    on the device: parameters, moments, step count, learning rate and batch-norm buffers are as if the iteration had been
    skipped, as the reference skips it.

    The logging dict is the reference's: ``update_plots`` appends learning_rate, match_loss, masked_non_match_loss and
    background_non_match_loss only (its other ``train`` lists stay empty); ``history`` holds every row in full.

    DATA PARALLEL (``gradients=``: a ``dcn_hip.distributed.FlatGradients(dcn, reduce="sum")`` attached to the optimizer; one
    process per GPU, every rank with its own store or its own generator and ``host_rng`` seeds, the same batch size B): the
    global batch is the G B pairs of all ranks.  Every iteration the ranks gather their types (one small collective, waited for
    after the forward pass), ``TrainState.advance_ranks`` takes the SAME decision on every rank -- the iteration counts when any
    pair of any rank is not empty -- and gives the rank its share w = n_rank / N of the non-empty pairs; the backward pass is
    seeded with ``loss * w`` and the gradients are SUMMED over the ranks: the gradient of the mean over all non-empty pairs of
    the global batch.  A second small collective gathers the ranks' log rows, and every rank writes the same history row.  Every
    rank issues the same collectives in the same order whatever the device decided, and still reads nothing back.  Batch-norm
    statistics stay per rank; ``run()`` writes files on ``save_rank`` only.  ``dcn_hip.distributed.broadcast_module`` before
    the first iteration is the caller's job."""

    def __init__(self, dcn, pcl, store, config, *, optimizer=None, generator=None, host_rng=None, logging_dir=None,
                 batch_size=None, per_pair_types=True, synthetic_multi_object=False, validation=None, gradients=None,
                 save_rank=0):
        t = config["training"]
        self.dcn, self.pcl, self.store, self.config = dcn, pcl, store, config
        self.generator, self.host_rng = generator, host_rng
        self.per_pair_types, self.synthetic_multi_object = bool(per_pair_types), bool(synthetic_multi_object)
        self.batch_size = int(batch_size if batch_size is not None else t["batch_size"])
        self.num_iterations, self.save_rate = int(t["num_iterations"]), int(t["save_rate"])
        self.logging_rate = int(t.get("logging_rate", 0) or 0)
        if optimizer is None:
            optimizer = GuardedAdam(dcn.parameters(), lr=float(t["learning_rate"]), weight_decay=float(t["weight_decay"]))
            if gradients is not None and hasattr(gradients, "attach"):
                gradients.attach(optimizer)      # (the trainer's own optimizer: nobody else could have attached it)
        if not isinstance(optimizer, GuardedAdam):
            raise TypeError("StoreTrainer needs a dcn_hip.optim.GuardedAdam (the update is skipped on the device), got %s"
                            % type(optimizer).__name__)
        self.optimizer = optimizer
        self.gradients, self.save_rank = gradients, int(save_rank)
        self.world, self.rank = 1, 0
        self._refuse_distributed()
        if gradients is not None:
            self._accept_gradients()
        device = next(dcn.parameters()).device
        self.state = TrainState(device, optimizer.param_groups[0]["lr"], t["steps_between_learning_rate_decay"],
                                t["learning_rate_decay"], betas=optimizer.param_groups[0]["betas"],
                                rows=self.num_iterations + 64)
        optimizer.bind(self.state)
        self._weight = torch.zeros((), dtype=torch.float32, device=device) if gradients is not None else None
        self.logging_dir = logging_dir
        self.logging_dict = empty_logging_dict()
        self.history = np.zeros((0, LOG_COLUMNS))
        self._board, self._board_rows = None, 0
        self.last = None                     # (loss, terms, num_valid, SampleBatch) of the latest iteration, on the device
        if validation is not None:
            if not isinstance(validation, Validation):
                raise TypeError("validation must be a dcn_hip.train.Validation, got %s" % type(validation).__name__)
            if [int(validation.store.h), int(validation.store.w)] != [int(v) for v in dcn.image_shape]:
                raise ValueError("validation store of %d x %d images, network of %s" % (validation.store.h, validation.store.w,
                                                                                      list(dcn.image_shape)))
            if torch.device(validation.store.device).type != device.type:
                raise ValueError("validation store on %s, network on %s" % (validation.store.device, device))
        self.validation = validation
        self.validation_history = None       # float64 [rows, 4 + 8 C] as of the latest read_log()
        self._validation_board_rows = 0

    def _refuse_distributed(self):
        if self.gradients is not None:
            return
        owners = [m for m in self.dcn.modules() if getattr(m, "_flat_grad_owner", None) is not None]
        if getattr(self.optimizer, "_flat_gradients", None) is not None or owners:
            raise NotImplementedError("StoreTrainer: dcn_hip.distributed gradients are attached; a skip decision that is "
                                      "consistent across ranks is not implemented")

    def _accept_gradients(self):
        """``gradients=``: the checks of the constructor, and once, on the host, that the ranks agree on B and the world size."""
        import torch.distributed as dist
        from .distributed import FlatGradients
        g = self.gradients
        if not isinstance(g, FlatGradients):
            raise TypeError("gradients must be a dcn_hip.distributed.FlatGradients, got %s" % type(g).__name__)
        if g.reduce != "sum":
            raise ValueError("StoreTrainer: gradients must be FlatGradients(..., reduce='sum'), got reduce=%r: every rank's loss "
                             "is weighted with its share of the non-empty pairs, the gradients are added" % (g.reduce,))
        mine = [p for p in self.dcn.parameters() if p.requires_grad]
        if len(mine) != len(g.params) or any(a is not b for a, b in zip(mine, g.params)):
            raise ValueError("StoreTrainer: gradients does not own the parameters of dcn")
        if getattr(self.optimizer, "_flat_gradients", None) is not g:
            raise ValueError("StoreTrainer: gradients is not attached to the optimizer (gradients.attach(optimizer))")
        owners = [m for m in self.dcn.modules() if getattr(m, "_flat_grad_owner", None) not in (None, g)]
        if owners:
            raise ValueError("StoreTrainer: another FlatGradients is installed on dcn")
        if dist.is_available() and dist.is_initialized():
            self.world, self.rank = dist.get_world_size(g.group), dist.get_rank(g.group)
        if self.world > 1:
            said = [None] * self.world
            dist.all_gather_object(said, (self.batch_size, self.world), group=g.group)
            if any(x != said[0] for x in said):
                raise ValueError("StoreTrainer: the ranks disagree on (batch size, world size): %s" % (said,))

    def _gather(self, tensor, async_op=False):
        from .distributed import gather_ranks
        return gather_ranks(tensor, self.gradients.group, self.gradients.single_rank_collectives, async_op=async_op)

    # ---- one iteration: nothing here reads the device
    def iteration(self, iteration):
        B = self.batch_size
        sb, _, _ = frames.draw_training_batch(self.store, B, self.config, generator=self.generator, host_rng=self.host_rng,
                                              per_pair_types=self.per_pair_types,
                                              synthetic_multi_object=self.synthetic_multi_object)
        return self.step_on_batch(sb, iteration)

    def step_on_batch(self, sb, iteration):
        from dense_correspondence.loss_functions import loss_composer
        B = int(sb.type.numel())
        dcn, state = self.dcn, self.state
        if self.gradients is not None:
            return self._step_on_batch_ranks(sb, iteration)
        state.advance(sb.type, iteration)
        self.optimizer.zero_grad()
        state.snapshot_bn(dcn)
        ya, yb = dcn.forward_pair(sb.input_a, sb.input_b)
        loss, terms, _, num_valid = loss_composer.get_loss_mixed(self.pcl, dcn.process_network_output(ya, B),
                                                                 dcn.process_network_output(yb, B), sb.device_lists())
        loss.backward()
        self.optimizer.step(state)
        state.restore_bn_if_skipped(dcn)
        state.log(iteration, loss, terms, sb.type)
        self.last = (loss.detach(), terms, num_valid, sb)
        return loss

    def _step_on_batch_ranks(self, sb, iteration):
        """The data-parallel iteration.  Two collectives of a few bytes besides the gradients'; the host's control flow does not
        depend on what the device finds, so the ranks' collective sequences cannot go out of step."""
        from dense_correspondence.loss_functions import loss_composer
        B = int(sb.type.numel())
        if B != self.batch_size:
            raise ValueError("StoreTrainer: a batch of %d pairs, the ranks agreed on %d" % (B, self.batch_size))
        dcn, state, grads = self.dcn, self.state, self.gradients
        types_all, gathered_types = self._gather(sb.type, async_op=True)       # waited for behind the forward pass
        self.optimizer.zero_grad()
        state.snapshot_bn(dcn)
        ya, yb = dcn.forward_pair(sb.input_a, sb.input_b)
        loss, terms, _, num_valid = loss_composer.get_loss_mixed(self.pcl, dcn.process_network_output(ya, B),
                                                                 dcn.process_network_output(yb, B), sb.device_lists())
        gathered_types.wait()
        state.advance_ranks(types_all, self.rank, self._weight, iteration)
        weighted = loss * self._weight
        weighted.backward()
        grads.all_reduce_mean()                  # reduce="sum"; the join of a bucketed backward
        self.optimizer.step(state)
        state.restore_bn_if_skipped(dcn)
        row = torch.cat([weighted.detach().reshape(1), terms.detach().reshape(-1)])
        state.log_ranks(iteration, self._gather(row), types_all)
        self.last = (loss.detach(), terms, num_valid, sb)
        return loss

    def validate(self, iteration):
        """The validation pass of ``iteration`` (run() calls it when ``validation.due(iteration)``): nothing here reads the
        device.  An iteration the device finds inactive still gets its pass -- the host cannot know -- and its row carries
        ``active == 0``."""
        if self.validation is None:
            raise ValueError("StoreTrainer: no validation configured")
        return self.validation.run(self.dcn, self.state, iteration)

    # ---- the host's side: save points and the end
    def read_log(self):
        snap = self.state.read()
        self.history = snap.history
        self.logging_dict = logging_dict_from_history(snap.history)
        if self.validation is not None:
            self.validation_history = self.validation.read()       # one more copy at a save point
            self.logging_dict["validation"] = self.validation.logging_dict(self.validation_history)
        if self.logging_dir is not None and self.rank == self.save_rank:
            if self._board is None:
                import tensorboard_logger
                self._board = tensorboard_logger.Logger(os.path.join(self.logging_dir, "tensorboard"))
            for row in snap.history[self._board_rows:]:
                if row[1] != 0:
                    for name, value in log_calls(row)[1]:
                        self._board.log_value(name, value, int(row[0]))
            if self.validation is not None:
                for row in self.validation_history[self._validation_board_rows:]:
                    if row[1] != 0:
                        for k, f in enumerate(self.validation.fields):
                            self._board.log_value("validation %s area above curve" % f,
                                                  float(row[VALIDATION_HEAD + 8 * k + 6]), int(row[0]))
        self._board_rows = len(snap.history)
        if self.validation is not None:
            self._validation_board_rows = len(self.validation_history)
        return snap

    def save_network(self, iteration, snap=None, logging_dict=None):
        """training.py:501-521: %06d.pth, %06d.pth.opt and, with a logging dict, %06d_log_history.yaml and loss.yaml."""
        from dense_correspondence_manipulation.utils import utils
        os.makedirs(self.logging_dir, exist_ok=True)
        f = os.path.join(self.logging_dir, utils.getPaddedString(iteration, width=6) + ".pth")
        torch.save(self.dcn.state_dict(), f)
        torch.save(self.optimizer.state_dict(known=(snap.t, snap.lr) if snap is not None else None), f + ".opt")
        if logging_dict is not None:
            utils.saveToYaml(logging_dict, os.path.join(self.logging_dir,
                                                        utils.getPaddedString(iteration, width=6) + "_log_history.yaml"))
            current = {}
            for key in ("train", "test"):        # (loss.yaml as the reference writes it: no validation key)
                current[key] = {field: (vec[-1] if len(vec) > 0 else -1) for field, vec in logging_dict[key].items()}
            utils.saveToYaml(current, os.path.join(self.logging_dir, "loss.yaml"))

    def save_configs(self):
        """training.py:525-532: training.yaml, with the network's own config under dense_correspondence_network when the
        dict given has none (DenseCorrespondenceNetwork.from_model_folder reads it from there)."""
        from dense_correspondence_manipulation.utils import utils
        os.makedirs(self.logging_dir, exist_ok=True)
        cfg = dict(self.config)
        if "dense_correspondence_network" not in cfg and getattr(self.dcn, "config", None) is not None:
            cfg["dense_correspondence_network"] = {k: v for k, v in self.dcn.config.items()
                                                   if k not in ("model_param_file", "path_to_network_params_folder",
                                                                "model_param_filename_tail")}
        utils.saveToYaml(cfg, os.path.join(self.logging_dir, "training.yaml"))

    def run(self, loss_current_iteration=0):
        """The loop of training.py:290-456 from iteration ``loss_current_iteration`` + 1.  A save point is ``iteration %
        save_rate == 0``: one read of the state; nothing is saved when that iteration was inactive (the reference has
        ``continue``d past its save).  The end follows the reference's ``>``: after ``num_iterations`` + start iterations the
        host reads ``active`` once per further iteration and stops, with a final save, at the first active one.
        -> the logging dict."""
        self._refuse_distributed()
        writes = self.logging_dir is not None and self.rank == self.save_rank      # (reads happen on every rank alike)
        start = int(loss_current_iteration)
        max_num_iterations = self.num_iterations + start
        self.dcn.train()
        if writes:
            self.save_configs()
            if start == 0:
                self.save_network(0)
        it = start
        while True:
            it += 1
            self.iteration(it)
            if self.validation is not None and self.validation.due(it):
                self.validate(it)
            snap = None
            if self.logging_dir is not None and self.save_rate > 0 and it % self.save_rate == 0:
                snap = self.read_log()
                if snap.active and writes:
                    self.save_network(it, snap, self.logging_dict)
            if self.logging_rate and it % self.logging_rate == 0:
                logging.info("Training on iteration %d of %d" % (it, max_num_iterations))
            if it > max_num_iterations:
                saved = snap is not None
                if snap is None:
                    snap = self.read_log()      # the one read of this iteration: `active`, and the rows for the final save
                if not snap.active:
                    continue
                logging.info("Finished testing after %d iterations" % max_num_iterations)
                if writes and not saved:
                    self.save_network(it, snap, self.logging_dict)
                return self.logging_dict
