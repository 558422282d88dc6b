"""Evaluation: one pass of a model over a held-out record set, scored by the metric kernels (ops/metrics.py).

``Evaluator.run()`` reads every record exactly once over the job's ranks (``DeviceLoader(train=False,
drop_last=False)``), runs the model in ``eval()`` under ``no_grad``, and per batch launches ``xent_topk`` and
``metric_accumulate`` into one device-resident fp64 accumulator: nothing is read on the host inside the loop.  After
the loop the accumulator is all-reduced once (jobs of more than one rank) and read once.

In data-parallel training every rank keeps BatchNorm running statistics of its own batches, and the chief's are the
ones a checkpoint holds.  So that a record scores the same whichever rank reads it -- and the same as the checkpoint
would -- a job of several ranks evaluates with the module buffers of rank ``buffers_from`` (one broadcast before the
pass) and gets its own back afterwards.

``BertEvaluator`` is the same pass (``_EvalPass``: only the batch's scoring and the result differ) for BERT
pre-training, with each rank's own buffers: a ``TokenLoader(train=False, drop_last=False)``, the model's
``pretraining_logits``, and the two metric launches twice per batch -- masked-LM predictions ``[B*P, V]`` and
next-sentence pairs ``[B, 2]`` -- into one fp64 ``[2, ACC_SLOTS]`` accumulator.

``EvalHook`` runs an evaluator from a training session every N global steps and at the end.
"""
import time

import torch

from ..ops import metrics
from .hooks import SessionRunArgs, SessionRunHook


class _EvalPass:
    """The pass both evaluators share.  A subclass gives ``_loader_name``, ``_acc_shape`` (of the fp64 accumulator),
    ``_score(batch, acc)`` (the model and the metric launches of one batch: no host read) and ``_result(values,
    seconds)`` (the accumulator as nested lists -> the result dictionary)."""
    _loader_name = _acc_shape = None

    def __init__(self, model, loader, ks, group, buffers_from):
        ks = tuple(int(k) for k in ks)
        if not 1 <= len(ks) <= metrics.MAX_KS or min(ks) < 1:
            raise ValueError("1 <= len(ks) <= %d and every k >= 1 required" % metrics.MAX_KS)
        if getattr(loader, "drop_last", False):
            raise ValueError("%s needs a loader that visits every record: %s(drop_last=False)" % (
                type(self).__name__, self._loader_name))
        self.model, self.loader, self.ks, self.group, self.buffers_from = model, loader, ks, group, buffers_from
        self.runs = 0

    def _world(self):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_world_size(self.group)
        return 1

    def _borrow_buffers(self):
        """Evaluate with rank ``buffers_from``'s floating-point buffers: -> [(buffer, this rank's own values)]."""
        if self.buffers_from is None or self._world() == 1:
            return []
        bufs = [b for b in self.model.buffers() if b.is_floating_point()]
        if not bufs:
            return []
        import torch.distributed as dist
        own = [(b, b.clone()) for b in bufs]
        packed = torch.cat([b.detach().reshape(-1).to(torch.float64) for b in bufs])  # exact for fp32 and bf16
        dist.broadcast(packed, self.buffers_from, group=self.group)
        o = 0
        with torch.no_grad():
            for b in bufs:
                b.copy_(packed[o:o + b.numel()].view_as(b))
                o += b.numel()
        return own

    def run(self):
        """One pass over the whole set -> the subclass's result dictionary (the same on every rank)."""
        model, loader = self.model, self.loader
        was_training = model.training
        acc = torch.zeros(self._acc_shape, dtype=torch.float64, device=loader.device)
        t0 = time.perf_counter()
        model.eval()
        own = []
        try:
            own = self._borrow_buffers()
            loader.seek(0)
            with torch.no_grad():
                for _ in range(loader.steps_per_epoch):
                    self._score(loader.next(), acc)
        finally:
            model.train(was_training)
            with torch.no_grad():
                for b, mine in own:
                    b.copy_(mine)
        if self._world() > 1:
            import torch.distributed as dist
            dist.all_reduce(acc, op=dist.ReduceOp.SUM, group=self.group)
        values = acc.tolist()  # the one host read
        seconds = time.perf_counter() - t0
        self.runs += 1
        return self._result(values, seconds)

    def close(self):
        self.loader.close()


class Evaluator(_EvalPass):
    _loader_name, _acc_shape = "DeviceLoader", (metrics.ACC_SLOTS,)

    def __init__(self, model, loader, ks=(1, 5), group=None, logits_fn=None, buffers_from=0):
        """loader: a ``DeviceLoader(train=False, drop_last=False)`` (anything with ``seek``, ``next`` ->
        ``(images, labels, indices)``, ``steps_per_epoch`` and ``close``).  logits_fn: ``(model, images) -> [B, V]``
        logits for models whose forward returns something else (default: ``model(images)``).  buffers_from: the rank
        (of the default group) whose module buffers every rank evaluates with; None: each rank its own."""
        super().__init__(model, loader, ks, group, buffers_from)
        self.logits_fn = logits_fn

    def _score(self, batch, acc):
        images, labels, _ = batch
        logits = self.logits_fn(self.model, images) if self.logits_fn is not None else self.model(images)
        loss, rank = metrics.xent_topk(logits, labels)
        metrics.metric_accumulate(acc, loss, rank, self.ks, logits.shape[1])
        self._classes = logits.shape[1]

    def _result(self, a, seconds):
        """-> {"n", "loss", "top<k>"..., "bad_labels", "nonfinite", "seconds", "images_per_sec"}.  Raises ValueError
        when a label is >= the number of classes."""
        n = int(a[0])
        res = {"n": n, "loss": a[1] / n if n else float("nan")}
        for i, k in enumerate(self.ks):
            res["top%d" % k] = a[4 + i] / n if n else float("nan")
            res["top%d_count" % k] = int(a[4 + i])
        res.update(bad_labels=int(a[2]), nonfinite=int(a[3]), loss_sum=a[1], seconds=seconds,
                   images_per_sec=n / seconds if seconds > 0 else float("nan"))
        if res["bad_labels"] > 0:
            raise ValueError("Evaluator: %d records have a label outside the model's %d classes" % (
                res["bad_labels"], self._classes))
        return res


class BertEvaluator(_EvalPass):
    _loader_name, _acc_shape = "TokenLoader", (2, metrics.ACC_SLOTS)  # rows: masked-LM, next-sentence

    def __init__(self, model, loader, ks=(1, 5), group=None, unpad=False):
        """loader: a ``TokenLoader(train=False, drop_last=False)`` (anything with ``seek``, ``next`` -> ``((ids,
        token_types, attention_mask, mlm_positions, mlm_labels, nsp_labels), num_valid, indices)``,
        ``steps_per_epoch`` and ``close``).  ks: the k of the masked-LM top-k accuracies.  Every rank scores with its
        own buffers: the pass launches no broadcast.  unpad=True: the encoder runs on the packed token rows of the
        loader's packs (a ``TokenLoader(pack=True)``, whose ``next`` returns the batch's SeqPack fourth); the same
        records and predictions are scored, by logits that differ in rounding only."""
        if unpad and not getattr(loader, "pack", False):
            raise ValueError("unpad=True needs a loader that returns packs: TokenLoader(pack=True)")
        self.unpad = bool(unpad)
        super().__init__(model, loader, ks, group, buffers_from=None)

    def _score(self, batch, acc):
        ids, tt, am, pos, lab, nsp = batch[0]
        mlm_logits, nsp_logits = self.model.pretraining_logits(ids, tt, am, pos, pack=batch[3] if self.unpad else None)
        loss, rank = metrics.xent_topk(mlm_logits, lab.reshape(-1))
        metrics.metric_accumulate(acc[0], loss, rank, self.ks, mlm_logits.shape[1])
        loss, rank = metrics.xent_topk(nsp_logits, nsp)
        metrics.metric_accumulate(acc[1], loss, rank, (1,), 2)

    def _result(self, values, seconds):
        """-> {"n" (sequences), "mlm_n" (predictions), "mlm_loss", "mlm_top<k>"..., "nsp_loss", "nsp_acc",
        "bad_labels", "nonfinite", "seconds", "sequences_per_sec"}."""
        m, s = values
        n, mlm_n = int(s[0]), int(m[0])
        nan = float("nan")
        res = {"n": n, "mlm_n": mlm_n, "mlm_loss": m[1] / mlm_n if mlm_n else nan}
        for i, k in enumerate(self.ks):
            res["mlm_top%d" % k] = m[4 + i] / mlm_n if mlm_n else nan
            res["mlm_top%d_count" % k] = int(m[4 + i])
        res.update(nsp_loss=s[1] / n if n else nan, nsp_acc=s[4] / n if n else nan, nsp_correct=int(s[4]),
                   mlm_loss_sum=m[1], nsp_loss_sum=s[1], bad_labels=int(m[2] + s[2]), nonfinite=int(m[3] + s[3]),
                   seconds=seconds, sequences_per_sec=n / seconds if seconds > 0 else nan)
        if res["bad_labels"] > 0:
            raise ValueError("BertEvaluator: %d labels lie outside the model's vocabulary or the two pair classes" %
                             res["bad_labels"])
        return res


def format_result(step, res, ks):
    """The one result line of the hook and of examples/ResNet50/resnet50_eval.py."""
    return "eval step %d: n=%d loss=%.6f %s" % (step, res["n"], res["loss"], " ".join(
        "top%d=%.6f" % (k, res["top%d" % k]) for k in ks))


def format_bert_result(step, res, ks):
    """The one result line of the hook in examples/BERT/bert_train.py and of examples/BERT/bert_eval.py."""
    return "eval step %d: n=%d mlm_n=%d mlm_loss=%.6f %s nsp_loss=%.6f nsp_acc=%.6f" % (
        step, res["n"], res["mlm_n"], res["mlm_loss"],
        " ".join("mlm_top%d=%.6f" % (k, res["mlm_top%d" % k]) for k in ks), res["nsp_loss"], res["nsp_acc"])


class EvalHook(SessionRunHook):
    """Runs ``evaluator`` when the global step reaches a multiple of ``every_n_steps`` and, with ``at_end``, once more
    at ``end`` unless that step was just evaluated.  It must run on every rank (the evaluator's all-reduce is a
    collective); ``log`` chooses who prints, ``formatter(step, result, ks)`` what (default: ``format_result``).
    ``results`` keeps ``(step, dict)`` of every evaluation."""

    def __init__(self, evaluator, every_n_steps, global_step, at_end=True, log=True, formatter=None):
        if every_n_steps is not None and every_n_steps < 1:
            raise ValueError("every_n_steps >= 1 (or None: only at the end) required")
        self._ev, self._n, self._gs, self._at_end, self._log = evaluator, every_n_steps, global_step, at_end, log
        self._format = formatter or format_result
        self._last = None
        self.results = []

    def _evaluate(self, step):
        res = self._ev.run()
        self._last = step
        self.results.append((step, res))
        if self._log:
            print(self._format(step, res, self._ev.ks), flush=True)

    def before_run(self, run_context):
        return SessionRunArgs(self._gs)

    def after_run(self, run_context, run_values):
        step = int(run_values.results)
        if self._n and step > 0 and step % self._n == 0 and step != self._last:
            self._evaluate(step)

    def end(self, session):
        step = int(session._read(self._gs))
        if self._at_end and step != self._last:
            self._evaluate(step)
        self._ev.close()
