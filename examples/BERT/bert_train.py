"""BERT pre-training (MLM + NSP) as a training job on the reference's session surface (BASELINE.json config 5;
SURVEY §7.4).  Synthetic token batches of BERT's input signature (no dataset offline), random-init weights.

Same structure as /root/reference/Synchronous-SGD/ssgd.py:51-69 and /root/reference/DOWNPOUR/DOWNPOUR.py:116-127:
``SyncReplicasOptimizer`` (all-reduce mode: no PS, one process per GPU over RCCL) wrapping the fused AdamW
(dtg.optim.FusedAdam; ``--opt lamb`` / ``--clip_norm``: FusedLAMB, global-norm clipping), a linear-warmup / linear-decay learning rate, ``MonitoredTrainingSession`` with
StopAtStepHook, a StepCounterHook reporting sequences/sec per worker and for the whole job, and a checkpoint
directory: the chief saves every ``--save_every`` steps (TensorBundle keyed by parameter name, AdamW slots
``<param>/m`` / ``<param>/v``, ``optimizer/step``, ``global_step``); a restarted job resumes from the latest
checkpoint at its global step, with the same learning-rate schedule position and dropout seeds.
``--accum_steps A`` runs A micro-batches of ``--batch`` sequences per optimizer step (gradients summed in fp32,
dtg.parallel.GradAccumulator): the large batches ``--opt lamb`` is for, at the memory of one micro-batch.
``--unpad`` (with ``--data_dir``) runs the encoder on the packed token rows of every batch instead of on ``batch * seq``
padded ones (dtg.ops.seqpack): the loader hands each batch's SeqPack to the model, micro-batch ``i`` of an
accumulating step uses ``pack.chunk(i, A)``, and the evaluation hook scores without padding too.

    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 bert_train.py \\
        --steps 1000 --ckpt_dir /path/to/ckpt
    python bert_train.py --tiny --steps 20 --ckpt_dir /tmp/bert_ck        # CPU, 2-layer model

With ``--data_dir`` the job reads token record shards (tools/make_shards.py --synthetic_tokens / --from_npy) through
dtg.data.TokenLoader instead: a sharded sampler keyed by the global step, a pinned prefetch ring and one dynamic
masking launch per batch (ops/mlm.py), a new mask for every record in every epoch; ``--seq`` and the token ids come
from the set (its tokens.json; BERT's uncased ids without one).  Each rank normalises its masked-LM loss by its own
batch's prediction count, counted on the host.  With ``--eval_dir`` and ``--eval_every`` every rank scores its slice of a
held-out set every N global steps and at the end (dtg.train.BertEvaluator: every record once over the ranks, the same
masks every time, one all-reduce) and the chief prints ``eval step N: n=... mlm_n=... mlm_loss=... mlm_top1=...
mlm_top5=... nsp_loss=... nsp_acc=...``; bert_eval.py scores a saved checkpoint the same way.
"""
import argparse

import _path  # noqa: F401

import torch

import dtg
from dtg.models import bert
from dtg.optim import FusedAdam, FusedLAMB
from dtg.parallel import FlatParams, comm


def lr_at(step, base, warmup, total):
    """BERT's schedule: linear warmup to ``base`` over ``warmup`` steps, then linear decay to 0 at ``total``."""
    if step < warmup:
        return base * (step + 1) / warmup
    return base * max(0.0, (total - step) / max(1, total - warmup))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000, help="last global step (absolute, like StopAtStepHook)")
    ap.add_argument("--batch", type=int, default=256, help="per-GPU sequences")
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--ckpt_dir", default="bert_logdir")
    ap.add_argument("--save_every", type=int, default=200)
    ap.add_argument("--log_every", type=int, default=20)
    ap.add_argument("--tiny", action="store_true", help="2-layer, 64-wide BERT (CPU tests)")
    ap.add_argument("--opt", choices=["adam", "lamb"], default="adam",
                    help="adam: fused AdamW; lamb: layer-wise adaptive moments (large-batch BERT), same m / v slots")
    ap.add_argument("--clip_norm", type=float, default=None,
                    help="clip the gradient to this global norm first (the original BERT recipe uses 1.0)")
    ap.add_argument("--accum_steps", type=int, default=1,
                    help="micro-batches of --batch sequences per optimizer step (gradient accumulation in fp32): the "
                         "per-GPU step batch is accum_steps * batch, the memory that of one --batch")
    ap.add_argument("--total_steps", type=int, default=None,
                    help="length of the learning-rate schedule (default: --steps); a job stopped early at --steps and "
                         "resumed later keeps one schedule")
    ap.add_argument("--data_dir", default=None,
                    help="directory of *.dtgrec token shards (tools/make_shards.py); default: synthetic batches")
    ap.add_argument("--data_seed", type=int, default=0, help="seed of the sampler and the masking draws")
    ap.add_argument("--loader_depth", type=int, default=3, help="slots of the loader's prefetch ring")
    ap.add_argument("--max_predictions", type=int, default=20, help="masked positions per sequence (with --data_dir)")
    ap.add_argument("--unpad", action="store_true",
                    help="run the encoder on packed token rows, without the [PAD] positions (needs --data_dir)")
    ap.add_argument("--eval_dir", default=None, help="directory of held-out *.dtgrec token shards to evaluate on")
    ap.add_argument("--eval_every", type=int, default=0, help="evaluate every N global steps (and at the end)")
    ap.add_argument("--eval_batch", type=int, default=None, help="per-GPU evaluation batch (default: --batch)")
    a, _ = ap.parse_known_args()
    if a.unpad and not a.data_dir:
        ap.error("--unpad needs --data_dir: the synthetic batches have no padding")
    rank, _, world, device = comm.init()
    is_chief = rank == 0
    cfg = bert.BertConfig.tiny() if a.tiny else bert.BertConfig.base()
    if a.tiny:
        a.seq = min(a.seq, 32)
    torch.manual_seed(1234)
    model = bert.BertForPreTraining(cfg).to(device)
    dtype = torch.bfloat16 if device.type == "cuda" else torch.float32
    flat = FlatParams(model, compute_dtype=dtype)
    model.train()

    batch_ph = [dtg.placeholder(name=n) for n in ("input_ids", "token_type_ids", "attention_mask",
                                                  "masked_lm_positions", "masked_lm_ids", "next_sentence_labels")]
    global_step = dtg.train.get_or_create_global_step()
    adam = (FusedLAMB if a.opt == "lamb" else FusedAdam)(flat, lr=a.lr, weight_decay=0.01, clip_norm=a.clip_norm)
    opt = dtg.train.SyncReplicasOptimizer(adam, replicas_to_aggregate=world, total_num_replicas=world, bucket_mb=25.0)
    num_valid = [None]  # the fed batch's prediction count (TokenFeedHook); None: every slot, as the synthetic batch
    seq_pack = [None]   # --unpad: the fed batch's SeqPack (TokenFeedHook)
    A = a.accum_steps
    step_batch = A * a.batch  # what one sess.run consumes per rank: A micro-batches of --batch sequences

    def loss_fn(*b, micro=(0, 1)):
        # the MLM loss is normalised by the WHOLE step's prediction count: each micro-batch passes its share n / A, so
        # the mean of the A losses is the loss of one batch of A * batch sequences
        nv = num_valid[0]
        pack = seq_pack[0].chunk(*micro) if seq_pack[0] is not None else None  # --unpad: the micro-batch's own pack
        return model(*b, num_valid=nv if nv is None or micro[1] == 1 else nv / micro[1], pack=pack)

    train_op = opt.minimize(loss_fn, global_step=global_step, inputs=batch_ph, accum_steps=A)
    hooks = [opt.make_session_run_hook(is_chief), dtg.train.StopAtStepHook(last_step=a.steps),
             dtg.train.StepCounterHook(every_n_steps=a.log_every, batch_size=step_batch, aggregate=True, log=is_chief)]
    loader = None
    if a.data_dir:
        # every rank reads its own disjoint part of each global batch; the batch is a function of the global step,
        # so a restarted job continues with the batch it would have seen next (TokenFeedHook seeks on restore)
        from dtg.data import TokenFeedHook, TokenLoader, masking_args, read_token_meta
        loader = TokenLoader(a.data_dir, step_batch, device, world=world, rank=rank, seed=a.data_seed,
                             depth=a.loader_depth, P=a.max_predictions, pack=a.unpad,
                             **masking_args(read_token_meta(a.data_dir)))
        hooks.append(TokenFeedHook(loader, batch_ph, global_step, lambda n: num_valid.__setitem__(0, n),
                                   (lambda p: seq_pack.__setitem__(0, p)) if a.unpad else None))
    if a.eval_dir and a.eval_every > 0:
        from dtg.data import TokenLoader, masking_args, read_token_meta
        from dtg.train.evaluation import format_bert_result
        eval_loader = TokenLoader(a.eval_dir, a.eval_batch or a.batch, device, world=world, rank=rank, train=False,
                                  drop_last=False, depth=a.loader_depth, P=a.max_predictions, pack=a.unpad,
                                  **masking_args(read_token_meta(a.eval_dir)))
        hooks.append(dtg.train.EvalHook(dtg.train.BertEvaluator(model, eval_loader, unpad=a.unpad), a.eval_every,
                                        global_step,
                                        log=is_chief, formatter=format_bert_result))
    with dtg.train.MonitoredTrainingSession(is_chief=is_chief, checkpoint_dir=a.ckpt_dir, hooks=hooks,
                                            save_checkpoint_secs=None, save_checkpoint_steps=a.save_every,
                                            log_step_count_steps=None, save_summaries_steps=None) as sess:
        step = int(sess.run(global_step))
        model._step = step * A  # dropout seeds follow the global step across a resume (one draw per micro-batch)
        if is_chief and sess.restored_from:
            print("resumed from %s (global step %d)" % (sess.restored_from, step), flush=True)
        while not sess.should_stop():
            adam.set_lr(lr_at(step, a.lr, a.warmup, a.total_steps or a.steps))  # a device-side scalar: no sync
            if loader is None:
                b = bert.synthetic_batch(step_batch, a.seq, cfg, device, max_predictions=20, seed=step * 1000 + rank)
                feed = dict(zip(batch_ph, b))
            else:
                feed = {}
            if (step + 1) % a.log_every == 0:
                _, loss, step = sess.run([train_op, train_op.loss, global_step], feed_dict=feed)
                if is_chief:
                    print("step %d loss %.4f lr %.3g" % (step, float(loss), adam.lr), flush=True)
            else:
                _, step = sess.run([train_op, global_step], feed_dict=feed)
            step = int(step)
    comm.barrier()
    if is_chief:
        if loader is not None:
            print("loader: %s" % loader.counters(), flush=True)
        print("done at global step %d" % step, flush=True)
    comm.shutdown()


if __name__ == "__main__":
    main()
