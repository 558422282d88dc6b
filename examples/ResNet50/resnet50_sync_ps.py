"""ResNet-50, synchronous SGD with backup workers on a GPU parameter server: the reference's
``SyncReplicasOptimizer(replicas_to_aggregate=N, total_num_replicas=M)`` ("aggregate N of M gradients, drop the
M - N stale ones", Synchronous-SGD/README.md:3, ssgd.py:51-60) with the parameters in the PS's HBM
(dtg.parallel.sync_ps).  Same launch idiom as resnet50_async_ps.py (``--job_name ps|worker --task_index i``).

    bash run_sync_ps.sh [--workers 7] [--replicas_to_aggregate 6] [--steps 50]

--steps counts GLOBAL steps (the PS's): every worker stops once the PS reports that step, a backup worker whose
last gradient was dropped included.  --ps_opt picks the PS's optimizer.

--ckpt_dir D makes the PS checkpoint (--save_every N global steps and / or --save_secs S, and once more when it
finishes) and restart from D's latest checkpoint ("[ps] restored <prefix> at step U"): the global step continues,
so a restarted job runs only the remainder of --steps.
"""
import argparse
import time

import _path  # noqa: F401

import torch

import dtg
from dtg import ops
from dtg.models import resnet
from dtg.optim import make_optimizer
from dtg.parallel import FlatParams
from dtg.parallel.ps_ckpt import PSCheckpointer
from dtg.parallel.sync_ps import SyncPSServer, init_from_cluster


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--job_name", default="")
    ap.add_argument("--task_index", type=int, default=0)
    ap.add_argument("--workers", type=int, default=7)
    ap.add_argument("--replicas_to_aggregate", type=int, default=None, help="R <= workers (default: workers - 1)")
    ap.add_argument("--base_port", type=int, default=2222)
    ap.add_argument("--steps", type=int, default=50, help="global steps")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--image", type=int, default=224)
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--ps_opt", default="momentum", choices=("sgd", "adagrad", "momentum", "adam", "lamb", "lars"),
                    help="the PS's optimizer (lamb / lars: layer-wise adaptive, norms of the summed gradient)")
    ap.add_argument("--tiny", action="store_true", help="narrow 4-block ResNet, 32x32 images (CPU smoke tests)")
    ap.add_argument("--ckpt_dir", default=None, help="the PS checkpoints here and restarts from its latest checkpoint")
    ap.add_argument("--save_every", type=int, default=None, help="checkpoint every N global steps")
    ap.add_argument("--save_secs", type=float, default=None, help="checkpoint every so many seconds")
    a, _ = ap.parse_known_args()
    R = a.replicas_to_aggregate or max(1, a.workers - 1)
    cluster = {"ps": [f"localhost:{a.base_port}"],
               "worker": [f"localhost:{a.base_port + 1 + i}" for i in range(a.workers)]}
    rank, world, device = init_from_cluster(cluster, a.job_name, a.task_index)
    torch.manual_seed(1234)
    model = (resnet.resnet18_like_tiny(10) if a.tiny else resnet.resnet50()).to(device)
    model = model.to(memory_format=torch.channels_last)
    ncls = 10 if a.tiny else 1000
    flat = FlatParams(model)
    if a.job_name == "ps":
        opt = make_optimizer(a.ps_opt, flat, a.lr, momentum=0.9, weight_decay=5e-5)
        ck = PSCheckpointer(flat, opt, a.ckpt_dir, every_n=a.save_every, every_secs=a.save_secs) if a.ckpt_dir else None
        ps = SyncPSServer(flat, opt, workers=range(1, world), replicas_to_aggregate=R, checkpointer=ck)
        if ps.restored_step is not None:
            print(f"[ps] restored {ck.restored[0]} at step {ps.restored_step}", flush=True)
        t0 = time.time()
        ps.serve()
        dt = time.time() - t0
        print(ps.summary(), flush=True)
        print(f"[ps] {len(ps.steps) / dt:.2f} global steps/sec, {len(ps.steps) * R * a.batch / dt:.1f} aggregated "
              f"images/sec (R={R} of {a.workers})", flush=True)
        if ck is not None:
            print(f"[ps] global step {ps.global_step}, checkpoints at {ck.saved}, {ck.skipped} skipped "
                  "(previous one in flight)", flush=True)
        ps.close()
    else:
        # the reference's worker loop (Synchronous-SGD/ssgd.py:62-69): a SyncReplicasOptimizer train op run under a
        # session until StopAtStepHook fires; the optimizer's hook does the initial pull and finish()
        sro = dtg.train.SyncReplicasOptimizer(dtg.train.GradientDescentOptimizer(a.lr), replicas_to_aggregate=R,
                                              total_num_replicas=a.workers, ps_rank=0)
        dt_ = torch.bfloat16 if device.type == "cuda" else torch.float32
        x, y = resnet.synthetic_batch(a.batch, device, dt_, a.image, ncls, seed=rank)
        images, labels = dtg.placeholder(name="images"), dtg.placeholder(name="labels")
        global_step = dtg.train.get_or_create_global_step()
        train_op = sro.minimize(lambda xb, yb: ops.softmax_cross_entropy(model(xb), yb), global_step=global_step,
                                var_list=flat, inputs=(images, labels))
        w = sro.ps_worker
        hooks = [sro.make_session_run_hook(is_chief=False), dtg.train.StopAtStepHook(last_step=a.steps)]
        t0 = time.time()
        with dtg.train.MonitoredTrainingSession(is_chief=False, hooks=hooks, log_step_count_steps=None,
                                                save_summaries_steps=None, save_checkpoint_secs=None) as sess:
            while not sess.should_stop():
                _, loss, step = sess.run([train_op, train_op.loss, global_step], feed_dict={images: x, labels: y})
                print(f"[worker {a.task_index}] global step {int(step)} loss {float(loss):.4f}", flush=True)
            if device.type == "cuda":
                torch.cuda.synchronize()
            dt = time.time() - t0
        print(f"[worker {a.task_index}] {w.pushes} pushes, {w.contributed} contributed, {w.dropped} dropped, "
              f"stopped={w.stopped}, {w.pushes * a.batch / dt:.1f} images/sec", flush=True)


if __name__ == "__main__":
    main()
