#!/usr/bin/env python
"""Headline benchmark (BASELINE.json): ResNet-50, ImageNet-shape, bf16, synthetic data,
images/sec for the WHOLE job across N MI355X (one process per GPU, RCCL over xGMI).

    python bench.py --gpus N --steps K --warmup W
    torchrun --nproc-per-node N bench.py --gpus N ...   (the driver's multi-GPU form)

Each timed step = H2D copy of a pinned uint8 batch on a side stream + fused
normalise kernel + forward + backward (bucketed gradient all-reduce overlapped with
backward when N > 1) + SGD-momentum update of every parameter.  Weak scaling: the
per-GPU batch is fixed, global batch = N * per-GPU batch.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=None, help="per-GPU batch (resnet50/vgg16 256, bert 32)")
    ap.add_argument("--image", type=int, default=224)
    ap.add_argument("--bucket-mb", type=float, default=None)
    ap.add_argument("--no-overlap", action="store_true")
    ap.add_argument("--profile-steps", type=int, default=0)
    ap.add_argument("--model", default="resnet50", choices=["resnet50", "vgg16", "bert", "nyiso_gru", "nyiso_lstm"],
                    help="resnet50 = the BASELINE headline; vgg16 / bert = the other BASELINE.json DP configs; "
                         "nyiso_gru / nyiso_lstm = the reference's own published workload (ADAG, 4 workers, "
                         "batch 32, window 5, 20 epochs): training time in seconds, lower is better")
    ap.add_argument("--workers", type=int, default=4, help="nyiso_*: dist-keras workers (reference: 2 x 2 = 4)")
    ap.add_argument("--epochs", type=int, default=20, help="nyiso_*: epochs (reference: 20)")
    ap.add_argument("--hours", type=int, default=11664,
                    help="nyiso_*: length of the synthetic hourly series; 11,664 hours give the reference's 11,519 "
                         "training rows (SURVEY 6.3), i.e. ragged shards of 2,879 / 2,880 / 2,880 / 2,880 rows")
    ap.add_argument("--reduce-dtype", default=None, choices=["fp32", "bf16"],
                    help="gradient all-reduce wire dtype (default DDL_REDUCE_DTYPE or fp32)")
    ap.add_argument("--graph", type=int, default=None,
                    help="1 = replay the whole step from a hipGraph (1-GPU runs without a process group only; "
                         "N > 1 steps stay eager: their bucket all-reduces are issued from backward hooks).  "
                         "Default: on for a 1-GPU run — measured +0.7-0.8 %% on ResNet-50 at 402 launches per step "
                         "(12,461-12,480 -> 12,550-12,586 img/s interleaved on one box, profiles/r6/ab_graph.txt)")
    ap.add_argument("--via-dataframe", action="store_true",
                    help="ResNet-50 through the DataFrame/trainer API: an ImageNet-shape uint8 frame, one partition "
                         "per rank, SynchronousDataParallel(...).train(df); the timed window is the trainer's own "
                         "steps after --warmup (barrier + synchronize on both sides)")
    ap.add_argument("--executor-pool", action="store_true",
                    help="--via-dataframe at N = 1: train in an executor process (the Spark-executor path: shard "
                         "handed over through shared memory) instead of in the driver")
    ap.add_argument("--ingest", default="auto", choices=["auto", "resident", "stream"],
                    help="--via-dataframe: shard residency in HBM or the pinned-ring stream (ShardLoader)")
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write DIR/loss.npy (the loss the last timed step returned) and "
                         "DIR/weight_norms.npy (the L2 norm of every fp32 parameter not initialised to zero, after "
                         "that step's update), float32; the run rewinds to its seeded initial weights before its "
                         "last timed step so that the arrays repeat from run to run (see rewind_state; figures "
                         "in docs/PERFORMANCE.md)")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements that are not part of the headline figure (they take runs of "
                         "their own): the stand-alone full-gradient all-reduce time of an N > 1 job (config.comm_ms)")
    args = ap.parse_args()
    if args.model == "vgg16" and args.image == 224:
        args.image = 32
    if args.batch is None:
        args.batch = 32 if args.model == "bert" else 256
    if args.model.startswith("nyiso_"):
        return bench_nyiso(args)  # driver + executor processes, no torchrun process group

    from distributeddeeplearningspark_amd.parallel import comm
    from distributeddeeplearningspark_amd.data.ingest import SyntheticImageStream
    from distributeddeeplearningspark_amd.models import ResNet50
    from distributeddeeplearningspark_amd.models.optimizers import SGD
    from distributeddeeplearningspark_amd.parallel.ddp import DataParallel

    pg = comm.init_from_env(prefer_gpu=True)
    rank, world = pg.rank, pg.world_size
    dev = pg.device
    if world != args.gpus and rank == 0:
        print(f"[bench] warning: --gpus {args.gpus} but world size {world}", file=sys.stderr)

    torch.manual_seed(1234 + rank)
    if args.model == "bert":
        return bench_bert(args, pg)
    if args.via_dataframe:
        return bench_via_dataframe(args, pg)
    if args.model == "vgg16":
        from distributeddeeplearningspark_amd.models.zoo import vgg16

        n_cls = 10
        model = vgg16(nb_classes=n_cls, input_shape=(args.image, args.image, 3))
    else:
        n_cls = 1000
        model = ResNet50(input_shape=(args.image, args.image, 3), num_classes=n_cls)
    model.compile(SGD(lr=0.1 if args.model == "resnet50" else 0.01, momentum=0.9, weight_decay=5e-5),
                  "sparse_categorical_crossentropy")
    model.place(dev, seed=0)
    ddp = make_ddp(model, pg, args)
    ddp.broadcast_parameters()

    stream = SyntheticImageStream(args.batch, args.image, n_cls, device=dev, seed=rank, n_buffers=4)
    step_fn = make_step(ddp, args)

    def step():
        x, y = stream.next()
        return step_fn(x, y)

    w0 = model.arena.master.clone() if args.dump_outputs else None
    for _ in range(args.warmup):
        step()
    pg.barrier()
    torch.cuda.synchronize(dev) if dev.type == "cuda" else None
    ddp.exposed_comm_ms(reset=True)  # exposed-comm statistics cover the timed steps only
    t0 = time.perf_counter()
    loss = None
    for i in range(args.steps):
        if w0 is not None and i == max(args.steps - _REWIND, 0):
            rewind_state(model, w0)
        loss = step()
    torch.cuda.synchronize(dev) if dev.type == "cuda" else None
    pg.barrier()
    dt = time.perf_counter() - t0
    dt_max = pg.max_scalar(dt)
    comm = comm_stats(ddp, pg, args.full)
    ms = dt_max * 1000.0 / args.steps
    gb = args.batch * world
    ips = gb * args.steps / dt_max
    lossv = float(loss) if loss is not None else float("nan")
    if rank == 0:
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, loss=lossv, weight_norms=weight_norms(model, w0))
        out = {
            "metric": ("images/sec (whole node) ResNet-50 ImageNet-shape at 1/2/4/8 MI355X" if args.model == "resnet50"
                       else "images/sec (whole node) VGG-16 CIFAR-shape"),
            "value": round(ips, 2),
            "unit": "images/sec",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16",
            "data": "synthetic",
            "config": {"model": args.model, "global_batch": gb, "seq_len": None, "image": args.image,
                       "per_gpu_batch": args.batch, "parallelism": f"dp{world}", "optimizer": "sgd-momentum",
                       "final_loss": round(lossv, 4), **comm},
        }
        print(json.dumps(out), flush=True)
    pg.shutdown()


def make_ddp(model, pg, args):
    import torch as _t

    from distributeddeeplearningspark_amd.parallel.ddp import DataParallel

    rd = None if args.reduce_dtype is None else (_t.bfloat16 if args.reduce_dtype == "bf16" else _t.float32)
    return DataParallel(model, pg, bucket_mb=args.bucket_mb, overlap=not args.no_overlap, reduce_dtype=rd,
                        timing=pg.distributed)


def make_step(ddp, args):
    """The timed step: ``ddp.train_step`` (eager launches + bucket hooks) or, on a 1-GPU run
    without a process group, the same step replayed from a hipGraph (``models/step.py``)."""
    use_graph = args.graph if args.graph is not None else 1
    if (not use_graph or ddp.pg.distributed or ddp.model.device.type != "cuda"
            or not getattr(ddp.model, "graph_capturable", True)):  # BERT: host-seeded dropout, eager steps
        return ddp.train_step
    from distributeddeeplearningspark_amd.models.step import CompiledTrainStep

    m = ddp.model
    if m.optimizer.arena is not m.arena:
        m.optimizer.bind(m.arena)
    return CompiledTrainStep(m, warmup=2)


_DUMP_CAP = 8 << 20  # elements per dumped array (32 MB of float32; --dump-outputs stays far below 64 MB in all)


def dump_outputs(directory, **arrays):
    """--dump-outputs: write each array as ``directory/<name>.npy`` in float32.  An array of more than
    ``_DUMP_CAP`` elements is reduced to that many of its elements, at sorted positions drawn once from a fixed
    seed (the same positions for the same size in every run and build)."""
    if not directory:
        return
    os.makedirs(directory, exist_ok=True)
    for name, a in arrays.items():
        if isinstance(a, torch.Tensor):
            a = a.detach().float().cpu().numpy()
        a = np.atleast_1d(np.asarray(a, dtype=np.float32))
        if a.size > _DUMP_CAP:
            idx = np.sort(np.random.default_rng(20240229).choice(a.size, _DUMP_CAP, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(directory, name + ".npy"), np.ascontiguousarray(a))


_REWIND = 1  # timed steps run after the rewind


def rewind_state(model, w0):
    """--dump-outputs: put the model back to its initial weights ``w0`` and an empty optimizer state, in stream
    order and without a host synchronisation (three device copies / fills, about 0.1 ms for ResNet-50, once per
    run).  The steps themselves are the default ones (same kernels, same captured graph).  Why: the default kernels
    add partial sums with fp32 atomics in no fixed order, and training amplifies that rounding from step to step,
    so after a few dozen steps two runs of one build are far apart.  From the same state the last step's loss
    (its forward pass) and the weight norms after it (its backward pass and update) agree to rounding; already one
    update at lr 0.1 between the rewind and the loss multiplies the rounding by a factor that depends on the shape."""
    a = model.arena
    with torch.no_grad():
        a.master.copy_(w0)
        a.sync_compute()
        for v in model.optimizer.state.values():
            v.zero_()


def weight_norms(model, w0):
    """L2 norm of the fp32 weights of every parameter, in arena order, that does not start at zero (``w0``: the
    initial arena).  A zero-initialised bias or BatchNorm shift holds nothing but the last update, so its
    norm is the norm of a gradient whose rounding noise is a tenth of it; beside its starting weights that
    noise is small."""
    with torch.no_grad():
        keep = [p for p in model.arena.params if bool(w0[p.offset:p.offset + p.snumel].any())]
        return torch.stack([p.master.detach().float().norm() for p in keep])


def comm_stats(ddp, pg, full=False):
    """Communication evidence for the JSON line: exposed (un-overlapped) all-reduce time per
    timed step and, with ``--full``, the stand-alone full-gradient all-reduce time (max over ranks)."""
    if not pg.distributed:
        return {"comm_ms": None, "exposed_comm_ms": None, "bucket_mb": ddp.bucket_mb, "buckets": len(ddp.buckets)}
    exposed = ddp.exposed_comm_ms()
    exposed = pg.max_scalar(exposed if exposed is not None else 0.0)
    if full:  # a measurement of its own (warm-up + 5 all-reduces of the whole gradient arena)
        full = ddp.measure_allreduce(iters=5)
        full = round(pg.max_scalar(full if full is not None else 0.0), 3)
    else:
        full = None
    return {"comm_ms": full, "exposed_comm_ms": round(exposed, 3), "bucket_mb": ddp.bucket_mb,
            "buckets": len(ddp.buckets), "reduce_dtype": "bf16" if ddp.bf16_algo is not None else "fp32",
            "bf16_algo": ddp.bf16_algo, "optimizer_overlap": ddp.overlap_optimizer and ddp.model.optimizer.ranged_ok,
            "grad_mb": round(ddp.grad_bytes / 2**20, 1), "backend": pg.backend, "forced_pg": pg.forced,
            "allreduce_fit": ddp.calibration}


# the reference's published NYISO numbers (ddl_nyiso_hdi.ipynb:608-609,730,817-818,934)
_NYISO_REF = {"GRU": {"time_s": 88.4753541946, "updates": 1425, "mape": 2.8088},
              "LSTM": {"time_s": 99.2543179989, "updates": 1425, "mape": 3.5871}}


def bench_nyiso(args):
    """The reference's own workload end to end (examples/ddl_nyiso.py): synthetic NYISO-shaped
    CSV -> Spark-style ETL -> ADAG(GRU|LSTM, 4 workers, batch 32, window 5, 20 epochs) ->
    ModelPredictor -> inverse MinMax -> MAPE.  ``value`` is ``trainer.get_training_time()``
    (the reference's metric); workers share the GPUs present (DDL_WORKERS_PER_GPU)."""
    import contextlib
    import math

    from distributeddeeplearningspark_amd.parallel.launcher import _gpu_count

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "examples"))
    import ddl_nyiso

    cell = args.model.split("_")[1].upper()
    gpus = _gpu_count()
    wpg = max(1, math.ceil(args.workers / max(gpus, 1)))
    argv = ["--workers", str(args.workers), "--epochs", str(args.epochs), "--models", cell,
            "--device", "auto" if gpus else "cpu", "--workers-per-gpu", str(wpg), "--hours", str(args.hours)]
    with contextlib.redirect_stdout(sys.stderr):  # the workflow's own report goes to stderr
        out = ddl_nyiso.main(argv)
    r = out["results"][cell]
    ref = _NYISO_REF[cell]
    dump_outputs(args.dump_outputs, mape=r["mape"])  # the workflow hands back the trained model's test error
    print(json.dumps({
        "metric": f"training time (s) NYISO {cell}(128)+Dense(1) ADAG {args.workers} workers {args.epochs} epochs",
        "value": round(r["time_s"], 4), "unit": "s", "n_gpus": gpus, "steps": int(r["updates"]), "warmup": 0,
        "ms_per_step": None, "higher_is_better": False, "scaling": "strong",
        "vs_baseline": round(r["time_s"] / ref["time_s"], 5), "dtype": "fp32",
        "data": f"synthetic NYISO-shaped hourly load ({args.hours:,} hours, "
                f"{sum(out.get('train_rows') or [0]):,} training rows in shards of {out.get('train_rows')})",
        "config": {"model": f"nyiso_{cell.lower()}", "algorithm": "ADAG", "workers": args.workers, "batch": 32,
                   "communication_window": 5, "epochs": args.epochs, "units": 128, "input": [25, 1],
                   "workers_per_gpu": wpg, "num_updates": r["updates"], "mape_pct": round(r["mape"], 4),
                   "wall_incl_executor_start_s": r.get("wall_incl_executor_start_s"),
                   "executor_start_s": r.get("executor_start_s"), "worker_s": r["worker_s"],
                   "commit_s": r.get("commit_s"), "commit_wait_s": r.get("commit_wait_s"),
                   "replicas_batched": r.get("batched"), "reference": ref},
    }), flush=True)


def bench_via_dataframe(args, pg):
    """ResNet-50 trained by ``SynchronousDataParallel(...).train(df)`` on an ImageNet-shape
    uint8 frame (the reference's path: DataFrame -> repartition -> one worker per partition,
    ``ddl_mnist_aztk.py:155-161,216-219``).  Each rank holds the frame (SPMD driver program),
    trains its partition: uint8 shard -> HBM (resident copy or the pinned-ring stream) ->
    normalize_u8 -> forward/backward/all-reduce/SGD; timed by the trainer's worker."""
    from distributeddeeplearningspark_amd.models import ResNet50
    from distributeddeeplearningspark_amd.models.optimizers import SGD
    from distributeddeeplearningspark_amd.sql.dataframe import from_columns
    from distributeddeeplearningspark_amd.trainers import SynchronousDataParallel

    rank, world = pg.rank, pg.world_size
    if args.executor_pool:
        os.environ["DDL_FORCE_POOL"] = "1"
    per_rank = args.batch * (args.warmup + args.steps)
    rng = np.random.default_rng(7)
    n = per_rank * world
    images = rng.integers(0, 256, (n, args.image, args.image, 3), dtype=np.uint8)
    labels = rng.integers(0, 1000, n)
    df = from_columns({"features": images, "label": labels}, num_partitions=world)
    model = ResNet50(input_shape=(args.image, args.image, 3), num_classes=1000)
    opt = SGD(lr=0.1, momentum=0.9, weight_decay=5e-5)
    model.compile(opt, "sparse_categorical_crossentropy")
    trainer = SynchronousDataParallel(model, worker_optimizer=opt, loss="sparse_categorical_crossentropy",
                                      num_workers=world, batch_size=args.batch, num_epoch=1,
                                      features_col="features", label_col="label", bucket_mb=args.bucket_mb,
                                      ingest=args.ingest, timing_warmup=args.warmup)
    trainer.train(df)
    res = trainer._results
    dt_max = max(r["timed_s"] for r in res)
    steps = res[0]["timed_steps"]
    gb = args.batch * world
    if rank == 0:
        dump_outputs(args.dump_outputs, loss=float(res[0]["history"][-1]))  # the trainer's own loop: no rewind
        print(json.dumps({
            "metric": "images/sec (whole node) ResNet-50 ImageNet-shape at 1/2/4/8 MI355X",
            "value": round(gb * steps / dt_max, 2), "unit": "images/sec", "n_gpus": world, "steps": steps,
            "warmup": args.warmup, "ms_per_step": round(dt_max * 1000.0 / steps, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
            "data": "synthetic uint8 ImageNet-shape DataFrame via SynchronousDataParallel.train",
            "config": {"model": "resnet50", "global_batch": gb, "seq_len": None, "image": args.image,
                       "per_gpu_batch": args.batch, "parallelism": f"dp{world}", "optimizer": "sgd-momentum",
                       "path": "dataframe" + ("+executor-pool" if args.executor_pool else ""),
                       "ingest": res[0]["ingest"],
                       "final_loss": round(float(res[0]["history"][-1]), 4)},
        }), flush=True)
    pg.shutdown()


def bench_bert(args, pg):
    """BERT-base MLM, seq 512, AdamW; whole-job tokens/sec (synthetic pretraining batches)."""
    from distributeddeeplearningspark_amd.data.synthetic import mlm_batch
    from distributeddeeplearningspark_amd.models.bert import BertConfig, BertForMaskedLM
    from distributeddeeplearningspark_amd.models.optimizers import AdamW
    from distributeddeeplearningspark_amd.parallel.ddp import DataParallel

    rank, world, dev = pg.rank, pg.world_size, pg.device
    cfg = BertConfig(num_hidden_layers=args.layers, max_position_embeddings=max(512, args.seq))
    model = BertForMaskedLM(cfg)
    model.compile(AdamW(lr=1e-4, weight_decay=0.01), "sparse_categorical_crossentropy")
    model.place(dev, seed=0)
    ddp = make_ddp(model, pg, args)
    ddp.broadcast_parameters()
    step_fn = make_step(ddp, args)
    batches = [mlm_batch(args.batch, args.seq, cfg.vocab_size, seed=rank * 100 + i) for i in range(4)]
    batches = [(model.to_input(x), model.to_target(y)) for x, y in batches]
    it = [0]

    def step():
        x, y = batches[it[0] % len(batches)]
        it[0] += 1
        return step_fn(x, y)

    w0 = model.arena.master.clone() if args.dump_outputs else None
    for _ in range(args.warmup):
        step()
    pg.barrier()
    torch.cuda.synchronize(dev) if dev.type == "cuda" else None
    ddp.exposed_comm_ms(reset=True)  # exposed-comm statistics cover the timed steps only
    t0 = time.perf_counter()
    loss = None
    for i in range(args.steps):
        if w0 is not None and i == max(args.steps - _REWIND, 0):
            rewind_state(model, w0)
        loss = step()
    torch.cuda.synchronize(dev) if dev.type == "cuda" else None
    pg.barrier()
    dt_max = pg.max_scalar(time.perf_counter() - t0)
    comm = comm_stats(ddp, pg, args.full)
    gb = args.batch * world
    tps = gb * args.seq * args.steps / dt_max
    if rank == 0:
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, loss=float(loss), weight_norms=weight_norms(model, w0))
        print(json.dumps({
            "metric": "tokens/sec (whole node) BERT-base MLM seq-len 512",
            "value": round(tps, 1), "unit": "tokens/sec", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(dt_max * 1000.0 / args.steps, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            "config": {"model": "bert-base-mlm" if args.layers == 12 else f"bert-{args.layers}l-mlm",
                       "global_batch": gb, "seq_len": args.seq, "per_gpu_batch": args.batch,
                       "parallelism": f"dp{world}", "optimizer": "adamw", "max_predictions": 80,
                       "sequences_per_sec": round(gb * args.steps / dt_max, 2),
                       "final_loss": round(float(loss), 4), **comm},
        }), flush=True)
    pg.shutdown()


if __name__ == "__main__":
    main()
