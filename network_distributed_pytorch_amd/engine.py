"""Training engine behind the reference-compatible ``ddp_init`` modules.

The reference's four experiment directories each re-implement ``setup()`` /
``run_task()`` / ``cleanup()`` around a module-level ``config`` dict
(ddp_guide_cifar10/ddp_init.py:64-137, ddp_powersgd_guide_cifar10/ddp_init.py:67-194,
ddp_powersgd_distillBERT_IMDb/ddp_init.py:103-238).  Here one engine implements them for
every task; the workload modules (``network_distributed_pytorch_amd.workloads.*``) keep
the reference's config keys and defaults and call into it.

Behaviour kept from the reference: seeds ``seed + rank`` for torch and numpy; per-rank
batch = global batch / world size (256 dense, 512 PowerSGD, 16·N DistilBERT);
``DataPartitioner`` shards with seed 1234; the per-epoch "Rank r, epoch e: mean loss"
print; the PowerSGD Algorithm-2 update and the dense SGD(momentum) update.
Fixed / added: rank-0 parameter broadcast (Q3/Q4), a rank-identical
IMDb split (Q2), a private PowerSGD RNG (Q1), configurable ``n_workers`` / batch
(Q11/Q12), synthetic device-resident data, JSONL metrics, checkpoint/resume,
replica-divergence checks, link emulation, hipGraph step capture, held-out evaluation
(``eval_every``: :func:`evaluate`, the fused loss / top-1 / top-k pass of ops/metrics.py), and
training / evaluating on the CIFAR-10 files of ``data_root`` (utils/cifar.py), held as bytes and
turned into batches by one launch each (ops/image_batch.py); ``data_root=None`` = synthetic data;
a learning-rate schedule (utils/schedule.py) and L2 weight decay, handed to the gradient sync before
every step (``sync.set_hyper``), which on the native engines reaches the captured step too.
"""
from __future__ import annotations

import datetime
import math
import os
import time
from typing import Any, Dict, Optional

import numpy as np
import torch
import torch.distributed as dist

from .ops import gemm_tuning
from .ops.ema import WeightEma
from .ops.loss import CrossEntropyLoss
from .ops.metrics import ClassificationMetrics
from .models import build_model
from .parallel.comm import LINK_PRESETS, Communicator
from .parallel.trainer import build_grad_sync
from .utils.checkpoint import load_checkpoint, restore_ema, save_checkpoint
from .utils.config import ConfigError, validate_config
from .utils.cifar import load_cifar10
from .utils.data import (NORMALIZE, DeviceLoader, SyntheticCIFAR10, SyntheticIMDb, SyntheticMLPData,
                         TensorDictDataset, Uint8ImageDataset, train_val_split)
from .utils.divergence import ReplicaChecker
from .utils.metrics import JsonlLogger, PhaseTimer, print_epoch, print_eval
from .utils.partition_helper import DataPartitioner
from .utils.schedule import LrSchedule

__all__ = ["setup", "run_task", "cleanup", "device_for", "default_config", "evaluate", "Evaluator", "ema_targets"]


def default_config(**over) -> Dict[str, Any]:
    cfg = dict(
        seed=714, rank=0, cuda_rank=0, n_workers=1, distributed_init_file=None, output_dir="./output.tmp",
        distributed_backend="nccl", init_method=None, timeout_s=600,
        learning_rate=1e-3, momentum=0.9, nesterov=False, training_epochs=1, batch_size=32, reducer_rank=4,
        # additions
        task="cifar", model="resnet18", num_classes=1000, global_batch=512, grad_sync="powersgd",
        dataset_size=None, data_seed=0, max_steps_per_epoch=None, graph_mode="auto", link="none",
        emulate_world=None, bucket_mb=None, reuse_query=True, overlap=None, psgd_groups=None,
        checkpoint_dir=None, resume=None, log_file=None, log_every=1, check_replicas_every=0,
        check_health_every=50, write_grad=False, verbose=True, trace_phases=False,
        # MIOpen's deterministic solver for any conv the native kernels do not cover (bitwise
        # resume); restored to the caller's setting by cleanup()
        deterministic=True,
        # held-out evaluation every N epochs (0 = off), held-out size, k of the top-k accuracy
        eval_every=0, eval_size=None, eval_topk=5,
        # CIFAR-10 from files (None = synthetic data), training augmentation, normalisation
        data_root=None, augment="none", normalize="half",
        # learning-rate schedule (utils/schedule.py) and L2 weight decay
        lr_schedule="constant", lr_warmup_steps=0, lr_min=0.0, lr_milestones="", lr_gamma=0.1, weight_decay=0.0,
        # clip the gradient by its global L2 norm (ops/gradclip.py): 0 = off, inf = measure only
        max_grad_norm=0.0,
        # label smoothing (ops/loss.py) and mixup / CutMix of the byte-image batches (ops/image_batch.py)
        label_smoothing=0.0, mix="none", mix_prob=1.0,
        # exponential moving average of the weights (ops/ema.py): 0 = off
        ema_decay=0.0, ema_warmup=True,
        # the optimiser behind the gradient sync: "sgd" or "adamw" (ops/adamw.py; weight_decay is then decoupled)
        optimizer="sgd", adam_beta1=0.9, adam_beta2=0.999, adam_eps=1e-8, decay_1d=True,
    )
    cfg.update(over)
    return cfg


def device_for(config) -> torch.device:
    if torch.cuda.is_available():
        idx = int(config.get("cuda_rank", 0)) % max(1, torch.cuda.device_count())
        return torch.device("cuda", idx)
    return torch.device("cpu")


def _log(config, *a):
    if config.get("verbose", True):
        print(*a, flush=True)


_SAVED_CUDNN: list = []


def setup(config) -> None:
    """Seed, then ``init_process_group`` (ddp_guide_cifar10/ddp_init.py:64-99)."""
    torch.manual_seed(config["seed"] + config["rank"])
    np.random.seed(config["seed"] + config["rank"])
    device = device_for(config)
    if device.type == "cuda":
        torch.cuda.set_device(device)
        # a library conv left on a path the native kernels do not cover runs MIOpen's
        # deterministic solution (no find-database / benchmark choice): a resumed run then
        # reproduces the uninterrupted one bitwise.  Opt out with config["deterministic"] =
        # False; cleanup() restores the previous process-wide values.
        if config.get("deterministic", True):
            _SAVED_CUDNN.append((torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark))
            torch.backends.cudnn.deterministic = True
            torch.backends.cudnn.benchmark = False
    if not dist.is_available():
        print("[Failure] Distributed Environment Failed")
        return
    if dist.is_initialized():
        return
    backend = config["distributed_backend"]
    if backend == "nccl" and device.type != "cuda":
        backend = "gloo"  # "gloo is more compatible" (ddp_guide/ddp_init.py:16)
    init_method = config.get("init_method")
    if not init_method:
        if config.get("distributed_init_file") is None:
            os.makedirs(config["output_dir"], exist_ok=True)
            config["distributed_init_file"] = os.path.join(config["output_dir"], "dist_init")
        init_method = "file://" + os.path.abspath(config["distributed_init_file"])
    _log(config, "==============================")
    _log(config, ">>>>> PyTorch DDP Initialization Step <<<<<")
    _log(config, "Distributed Init: rank {}/{}(Total: {}) - socket ({})".format(
        config["rank"], config["n_workers"] - 1, config["n_workers"], init_method))
    kw = dict(backend=backend, init_method=init_method, timeout=datetime.timedelta(seconds=config["timeout_s"]),
              world_size=config["n_workers"], rank=config["rank"])
    if backend == "nccl":
        kw["device_id"] = device
    dist.init_process_group(**kw)
    _log(config, "All ranks successfully initialized")
    _log(config, "==============================\n")


def cleanup(config=None) -> None:
    """``destroy_process_group`` with banners (ddp_guide_cifar10/ddp_init.py:132-137)."""
    if config is None or config.get("verbose", True):
        print("==============================")
        print(">>>>> PyTorch DDP Destroy <<<<<")
    if dist.is_available() and dist.is_initialized():
        dist.destroy_process_group()
    if _SAVED_CUDNN:  # setup()'s determinism switch is process-wide: hand the old values back
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = _SAVED_CUDNN[0]
        _SAVED_CUDNN.clear()
    if config is None or config.get("verbose", True):
        print("All ranks successfully destroyed")
        print("==============================\n")


def _world():
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(), dist.get_rank()
    return 1, 0


def _build_data(config, device, world, rank):
    """(this rank's training partition, per-rank batch, held-out set or None).  Held-out data is
    built only when ``eval_every`` > 0, and never changes the training data."""
    task = config["task"]
    seed = config["data_seed"]
    want_val = bool(config.get("eval_every"))
    eval_size = config.get("eval_size")
    if task == "cifar" and config.get("data_root"):
        # the CIFAR-10 files, resident as bytes; batches come from ops.image_batch (one launch)
        mean, std = NORMALIZE[config.get("normalize", "half")]
        crop = config.get("augment", "none") == "crop_flip"
        images, labels = load_cifar10(config["data_root"], train=True)
        n = min(config["dataset_size"] or len(images), len(images))
        ds = Uint8ImageDataset(images[:n], labels[:n], mean, std, pad=4 if crop else 0, flip=crop,
                               mix=config.get("mix", "none"), mix_prob=config.get("mix_prob", 1.0)).to(device)
        val = None
        if want_val:  # the test split, never augmented or mixed
            vi, vl = load_cifar10(config["data_root"], train=False)
            nv = min(eval_size or len(vi), len(vi))
            val = Uint8ImageDataset(vi[:nv], vl[:nv], mean, std).to(device)
        bsz = int(config["global_batch"] / float(world))
        part = DataPartitioner(ds, [1.0 / world for _ in range(world)]).use(rank)
        return part, bsz, val
    if task == "cifar":
        n = config["dataset_size"] or 50000
        val = None
        if want_val:
            ds, val = SyntheticCIFAR10(n=n, seed=seed, device=device, holdout=eval_size or 10000)
        else:
            ds = SyntheticCIFAR10(n=n, seed=seed, device=device)
        bsz = int(config["global_batch"] / float(world))
        part = DataPartitioner(ds, [1.0 / world for _ in range(world)]).use(rank)
        return part, bsz, val
    if task == "imdb":
        n = config["dataset_size"] or 25000
        seq = config.get("seq_len", 512)
        full = SyntheticIMDb(n=n, seq_len=seq, seed=seed, device=device)
        train, val = train_val_split(full, test_size=0.2, seed=seed + 42)
        total_batch = config.get("global_batch") or 16 * world
        bsz = int(total_batch / float(world))
        part = DataPartitioner(train, [1.0 / world for _ in range(world)]).use(rank)
        if not want_val:
            val = None
        elif eval_size is not None and eval_size < len(val):  # cap on the 20 % validation split
            val = TensorDictDataset({k: v[:eval_size] for k, v in val.columns.items()}, val.as_tuple)
        return part, bsz, val
    if task == "mlp":
        n = config["dataset_size"] or 1024
        val = None
        if want_val:
            ds, val = SyntheticMLPData(n=n, seed=seed, device=device, holdout=eval_size or 256)
        else:
            ds = SyntheticMLPData(n=n, seed=seed, device=device)
        bsz = int(config["global_batch"] / float(world))
        part = DataPartitioner(ds, [1.0 / world for _ in range(world)]).use(rank)
        return part, bsz, val
    raise ValueError(f"unknown task {task!r}")


def _loss_fn(config, model, crit):
    if config["task"] == "imdb":
        def f(batch):
            out = model(batch["input_ids"], attention_mask=batch["attention_mask"], labels=batch["labels"])
            return out[0]
    else:
        def f(batch):  # (data, target), or (data, target, target_b, lam) from a dataset that mixes samples
            data, target, *mixed = batch
            return crit(model(data), target, *mixed)
    return f


class Evaluator:
    """Held-out evaluation of ``model`` on ``dataset``: loss, top-1 and top-k by the fused metrics
    kernel (ops/metrics.py), accumulated on the device; one fp64[4] all-reduce and one host sync
    close the pass.

    * runs under ``model.eval()`` and ``torch.no_grad()`` and puts the model back in the mode it
      found; no buffer of the model changes;
    * rank r evaluates ``index[r::world]``: every sample exactly once, none duplicated;
    * batches are cut at ``batch`` (the per-rank TRAINING batch size: the same conv plans and
      weight-bank schedule as training, one shape for the whole pass); the ragged last batch is
      padded with zero inputs and ``target = ignore_index``, which the kernel drops;
    * ``graph_mode != "none"`` on device: one eager warm-up batch, then forward + metrics launch
      captured once as a linear graph on static inputs and replayed per batch; the graph is kept
      on the evaluator and reused by later calls (the model's weights are read by the graph at
      replay time, weight transforms included, so it always sees the current parameters);
    * DistilBERT-style datasets (``input_ids`` / ``attention_mask`` / ``labels`` columns) call the
      model without ``labels``; its logits feed the kernel;
    * a dataset with ``gather_into`` (``Uint8ImageDataset``) loads batch, targets and tail padding
      into fp32 static inputs in one launch, unaugmented; every other dataset takes the
      gather + copy path.
    """

    def __init__(self, model, dataset, *, batch: int, comm=None, device=None, topk: int = 5,
                 graph_mode: str = "none", ignore_index: int = -100):
        first = next(iter(dataset.columns.values()))
        self.device = torch.device(device) if device is not None else first.device
        self.model = model
        self.comm = comm
        self.batch = int(batch)
        assert self.batch >= 1, "evaluate: batch >= 1"
        self.ignore_index = int(ignore_index)
        self.ds = dataset if first.device == self.device else dataset.to(self.device)
        world = comm.world_size if comm is not None else 1
        rank = comm.rank if comm is not None else 0
        self.index = torch.arange(len(dataset), device=self.device)[rank::world]
        self.total = len(dataset)
        if dataset.as_tuple:
            self.inputs, self.target_key = [dataset.as_tuple[0]], dataset.as_tuple[1]
        else:
            self.inputs, self.target_key = ["input_ids", "attention_mask"], "labels"
        cols = self.ds.columns
        # a dataset that assembles its own batches (Uint8ImageDataset) delivers fp32 whatever it stores
        self.fused_load = hasattr(self.ds, "gather_into")
        self.static = {k: torch.zeros((self.batch,) + tuple(cols[k].shape[1:]),
                                      dtype=torch.float32 if self.fused_load else cols[k].dtype,
                                      device=self.device) for k in self.inputs}
        self.static_target = torch.full((self.batch,), self.ignore_index, dtype=torch.int64, device=self.device)
        self.metrics = ClassificationMetrics(k=topk, ignore_index=self.ignore_index, device=self.device)
        self.graph_mode = graph_mode if self.device.type == "cuda" else "none"
        self.graph = None
        self.replays = 0

    def _forward(self):
        if len(self.inputs) == 1:
            logits = self.model(self.static[self.inputs[0]])
        else:
            logits = self.model(self.static["input_ids"], attention_mask=self.static["attention_mask"])[-1]
        self.metrics.update(logits, self.static_target)

    def _load(self, idx: torch.Tensor):
        if self.fused_load:  # batch, targets and tail padding in one launch
            self.ds.gather_into(idx, self.static[self.inputs[0]], self.static_target, pad_target=self.ignore_index)
            return
        m = int(idx.numel())
        for k in self.inputs:
            self.static[k][:m].copy_(self.ds.columns[k].index_select(0, idx))
        self.static_target[:m].copy_(self.ds.columns[self.target_key].index_select(0, idx))
        if m < self.batch:  # ragged tail: zero inputs, ignored targets
            for k in self.inputs:
                self.static[k][m:].zero_()
            self.static_target[m:].fill_(self.ignore_index)

    def _capture(self):
        import gc

        torch.cuda.synchronize()
        gc.collect()  # no cyclic GC while capturing (see utils/graph.StepRunner.capture)
        was = gc.isenabled()
        gc.disable()
        try:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._forward()
        finally:
            if was:
                gc.enable()
        self.graph = g

    def __call__(self) -> Dict[str, Any]:
        t0 = time.perf_counter()
        was_training = self.model.training
        self.model.eval()
        self.metrics.reset()
        try:
            with torch.no_grad():
                for s in range(0, len(self.index), self.batch):
                    self._load(self.index[s: s + self.batch])
                    if self.graph is not None:
                        self.graph.replay()
                        self.replays += 1
                    else:
                        self._forward()
                        if self.graph_mode != "none":  # that was the eager warm-up batch
                            state = self.metrics.state.clone()
                            self._capture()  # a capture enqueues nothing: the state is untouched,
                            self.metrics.state.copy_(state)  # restored all the same
                rec = self.metrics.compute(self.comm)
                if hasattr(self.ds, "check_errors"):
                    self.ds.check_errors()  # after compute(): the pass's one host sync is behind us
        finally:
            self.model.train(was_training)
        rec["comm_bytes"] = self.metrics.comm_bytes
        rec["eval_s"] = time.perf_counter() - t0
        return rec


def evaluate(model, dataset, *, batch: int, comm=None, device=None, topk: int = 5, graph_mode: str = "none",
             ignore_index: int = -100) -> Dict[str, Any]:
    """One held-out pass (see :class:`Evaluator`): ``{"loss", "top1", "topk", "n", "k",
    "comm_bytes", "eval_s"}``; ``topk`` is None when ``k`` is not below the class count.  Build an
    :class:`Evaluator` yourself to reuse its captured graph across passes."""
    return Evaluator(model, dataset, batch=batch, comm=comm, device=device, topk=topk, graph_mode=graph_mode,
                     ignore_index=ignore_index)()


def _batch_len(batch) -> int:
    first = next(iter(batch.values())) if isinstance(batch, dict) else batch[0]
    return int(first.shape[0])


def run_task(config) -> Dict[str, Any]:
    """The reference's training loop for the configured task (returns a summary)."""
    validate_config(config, strict=False)  # typed schema: types, choices, cross-field rules
    if config.get("_unknown_keys"):
        _log(config, f"[config] ignoring unknown keys {config['_unknown_keys']}")
    _log(config, "==============================")
    _log(config, ">>>>> Run Designated Task <<<<<")
    device = device_for(config)
    world, rank = _world()
    part, bsz, val = _build_data(config, device, world, rank)
    graph_mode = config.get("graph_mode", "auto")
    if device.type != "cuda":
        graph_mode = "none"
    else:
        gemm_tuning.enable()  # measured GEMM solutions for the library GEMMs (ops/gemm_tuning.py)

    model_name = config["model"] if config["task"] != "imdb" else "distilbert"
    if config["task"] == "mlp":
        model_name = "mlp"
    model = build_model(model_name, config["num_classes"] if config["task"] != "imdb" else 2).to(device)
    label_smoothing = float(config.get("label_smoothing") or 0.0)
    mix = config.get("mix", "none")
    # fused gfx950 kernels on device (ops/loss.py)
    crit = CrossEntropyLoss(label_smoothing=label_smoothing).to(device)
    if config["task"] == "imdb" and label_smoothing:
        model.config.label_smoothing = label_smoothing  # DistilBERT computes its own loss
    link = None if config.get("link", "none") == "none" else LINK_PRESETS[config["link"]]
    comm = Communicator(link=link, emulate_world=config.get("emulate_world"),
                        device=device if device.type == "cuda" else None)
    extra = {}
    if config["grad_sync"] in ("powersgd", "powersgd-adamw"):
        extra = {"write_grad": config.get("write_grad", False), "reuse_query": config.get("reuse_query", True),
                 "overlap": config.get("overlap"), "groups": config.get("psgd_groups")}
        if not extra["reuse_query"]:
            graph_mode = "none"  # the per-step query re-draw is host-side (not capturable)
    elif config["grad_sync"] == "dense":
        extra = {"overlap": config.get("overlap")}
    max_grad_norm = float(config.get("max_grad_norm") or 0.0)
    if max_grad_norm > 0:  # off: build_grad_sync is called exactly as before
        extra["max_grad_norm"] = max_grad_norm
    optimizer = config.get("optimizer") or "sgd"
    if optimizer != "sgd":  # sgd: build_grad_sync is called exactly as before
        extra.update(optimizer=optimizer, betas=(float(config["adam_beta1"]), float(config["adam_beta2"])),
                     eps=float(config["adam_eps"]), decay_1d=bool(config.get("decay_1d", True)))
    sync = build_grad_sync(config["grad_sync"], model, comm, lr=config["learning_rate"],
                           momentum=config["momentum"], rank=config["reducer_rank"],
                           bucket_mb=config.get("bucket_mb"), seed=config["seed"], **extra)
    start_epoch = 0
    step = 0
    info = None
    if config.get("resume"):
        info = load_checkpoint(config["resume"], model, sync)
        start_epoch = info["epoch"] + 1
        step = info["step"]
    # weight EMA (ops/ema.py): built over the (resumed) weights, then updated by the sync behind every
    # step's last update launch.  Off: nothing is allocated, launched, logged or uploaded.
    ema = None
    ema_decay = float(config.get("ema_decay") or 0.0)
    if ema_decay > 0:
        ema_names, ema_tensors = ema_targets(model)
        ema = WeightEma(ema_tensors, ema_decay, warmup=bool(config.get("ema_warmup", True)))
        if info is not None:
            restore_ema(ema, info.get("ema"), config["resume"])
        sync.attach_ema(ema)
    log_path = config.get("log_file")
    if log_path and "{rank}" in log_path:  # one file per rank
        logger = JsonlLogger(log_path.format(rank=rank), rank, all_ranks=True)
    else:
        logger = JsonlLogger(log_path, rank)
    log_every = int(config.get("log_every") or 0) if logger.enabled else 0
    checker = None
    if config.get("check_replicas_every") and sync.flat_weights is not None:
        checker = ReplicaChecker(comm, sync.flat_weights, every=config["check_replicas_every"])

    loss_fn = _loss_fn(config, model, crit)
    runner = None
    static = {}
    loss_static = torch.zeros((), device=device)
    if graph_mode != "none":
        from .utils.graph import StepRunner

        def pre():
            sync.zero_grad()
            loss = loss_fn(static["batch"])
            loss.backward()
            loss_static.copy_(loss.detach())
        runner = StepRunner(pre, sync, mode=graph_mode, state_tensors=list(model.buffers()))
        graph_mode = runner.mode
        if graph_mode == "none":
            runner = None
    # every batch is trained, the ragged last one too (the reference's DataLoader keeps it,
    # ddp_powersgd_guide_cifar10/ddp_init.py:53,142): in graph mode a batch whose shape
    # differs from the captured one runs as an eager step (see _eager_step)
    loader = DeviceLoader(part, bsz, shuffle=True, seed=config["seed"] + rank, device=device, drop_last=False)
    loader.set_epoch(start_epoch)
    num_batches = math.ceil(len(part) / float(bsz))  # reference: ceil(len(partition) / bsz)
    health_every = int(config.get("check_health_every") or 0)
    # learning-rate schedule and weight decay: a pure function of the global step, which continues
    # across epochs and a resume.  With the defaults nothing below is called, logged or uploaded.
    steps_per_epoch = min(num_batches, config.get("max_steps_per_epoch") or num_batches)
    try:
        schedule = LrSchedule.from_config(config, steps_per_epoch)  # checks lr_warmup_steps < total steps
    except ValueError as exc:
        raise ConfigError(str(exc)) from None
    weight_decay = float(config.get("weight_decay") or 0.0)
    hyper_on = schedule.varies or weight_decay != 0.0
    lr_now = None
    if hyper_on:  # the pinned source rows of the whole run, written once
        sync.plan_hyper((schedule.lr_at(s), weight_decay) for s in range(step, schedule.T))

    timer = PhaseTimer() if (config.get("trace_phases") and runner is None) else None
    eval_every = int(config.get("eval_every") or 0)
    evaluator = None
    if eval_every and val is not None:
        evaluator = Evaluator(model, val, batch=bsz, comm=comm, device=device, topk=config.get("eval_topk", 5),
                              graph_mode=graph_mode)
    evals = []
    eval_s = 0.0
    losses = []
    clip_on = max_grad_norm > 0
    clipped_base = None  # the block's counter when this run began (a resume restarts clipped_steps)

    def ema_record():
        # host read of the EMA block; after a replay its last write may sit on the side stream
        if runner is not None:
            runner.join()
        return {"ema_decay": ema_decay, "ema_warmup": ema.warmup, "ema_updates": ema.read()["updates"]}

    def clip_read():
        # host read of the clip block; after a replay the block's last write may sit on the side stream
        if runner is not None:
            runner.join()
        return sync.clip_stats()
    if clip_on:
        clipped_base = clip_read()["clipped"]

    def adam_record():
        # host read of the AdamW block; after a replay its last write may sit on the side stream
        if runner is not None:
            runner.join()
        return {"optimizer": optimizer, "adam_steps": sync.adam_stats()["steps"]}
    t_start = time.perf_counter()
    samples = 0
    last_log = (time.perf_counter(), comm.stats.payload_bytes, comm.stats.wire_bytes, step)
    for epoch in range(start_epoch, config["training_epochs"]):
        _log(config, ">>>>> Rank ", rank, ", epoch ", epoch, " Started...")
        epoch_loss = torch.zeros((), device=device, dtype=torch.float64)
        i = 0
        for batch in loader:
            if config.get("max_steps_per_epoch") and i >= config["max_steps_per_epoch"]:
                break
            if hyper_on:  # before a replay, the ragged eager step and the plain eager step alike
                lr_now = schedule.lr_at(step)
                sync.set_hyper(lr_now, weight_decay)
            if runner is not None and "batch" in static and not _same_shape(static["batch"], batch):
                runner.join()  # ragged batch: eager step, ordered after the last replay
                sync.zero_grad()
                loss = loss_fn(batch)
                epoch_loss += loss.detach()
                loss.backward()
                sync.step()
                loss_static.copy_(loss.detach())
            elif runner is not None:
                if "batch" not in static:
                    static["batch"] = _clone_batch(batch)
                    if not isinstance(batch, dict):  # later full batches: written in place, one launch
                        loader.deliver_into(static["batch"][0], static["batch"][1], extra=static["batch"][2:])
                elif not _delivered(static["batch"], batch):
                    _copy_batch(static["batch"], batch)
                runner()
                epoch_loss += loss_static
            elif timer is not None:  # eager + per-phase HIP-event tracing
                sync.zero_grad()
                with timer.phase("forward"):
                    loss = loss_fn(batch)
                epoch_loss += loss.detach()
                with timer.phase("backward"):
                    loss.backward()
                phases = sync.phases()
                if phases is None:
                    with timer.phase("grad_sync+update"):
                        sync.step()
                else:
                    for fn, is_comm in phases:
                        with timer.phase(("comm:" if is_comm else "compute:") + fn.__name__):
                            fn()
            else:
                sync.zero_grad()
                loss = loss_fn(batch)
                epoch_loss += loss.detach()
                loss.backward()
                sync.step()
            i += 1
            step += 1
            samples += _batch_len(batch) * world  # the ragged last batch counts what it holds
            if checker is not None:
                if runner is not None and step % checker.every == 0:
                    runner.join()
                checker.check(step)
            if health_every and step % health_every == 0:
                if runner is not None:
                    runner.join()
                sync.check_errors()  # flag-wait timeouts / MGS barrier / RCCL async errors: fatal
            if health_every and step % health_every == 0 and hasattr(loader.ds, "check_errors"):
                loader.ds.check_errors()  # image-batch error word: an index outside the dataset
            if log_every and step % log_every == 0:  # per-step record (host sync at this cadence)
                loss_now = float((loss_static if runner is not None else loss.detach()).item())
                now = time.perf_counter()
                t_prev, pay_prev, wire_prev, step_prev = last_log
                n = max(1, step - step_prev)
                logger.log(kind="step", epoch=epoch, step=step, loss=loss_now,
                           step_ms=1e3 * (now - t_prev) / n,
                           samples_per_s=bsz * world * n / max(now - t_prev, 1e-9),
                           payload_bytes=(comm.stats.payload_bytes - pay_prev) / n
                           if runner is None or graph_mode == "piecewise" else sync.bytes_per_step,
                           wire_bytes=(comm.stats.wire_bytes - wire_prev) / n
                           if runner is None or graph_mode == "piecewise" else
                           _ring_wire(sync.bytes_per_step, comm.paced_world),
                           bytes_per_step=sync.bytes_per_step,
                           **({"lr": lr_now} if hyper_on else {}),
                           **(_clip_step_record(clip_read()) if clip_on else {}))
                last_log = (now, comm.stats.payload_bytes, comm.stats.wire_bytes, step)
        if runner is not None:
            runner.join()  # parameters / sync state are read below (checks, checkpoint)
        # reference: epoch_loss / num_batches (ddp_powersgd_guide_cifar10/ddp_init.py:118,183);
        # a step cap (max_steps_per_epoch, an addition) divides by the steps actually run
        mean = float(epoch_loss.item()) / max(1, num_batches if i == num_batches else i)
        sync.check_errors()  # MGS barrier timeouts / RCCL async errors (epoch cadence)
        if hasattr(loader.ds, "check_errors"):
            loader.ds.check_errors()
        losses.append(mean)
        epoch_rec = {}
        if clip_on:
            epoch_rec = {"clipped_steps": clip_read()["clipped"] - clipped_base, "max_grad_norm": max_grad_norm}
        if label_smoothing:
            epoch_rec["label_smoothing"] = label_smoothing
        if mix != "none":
            epoch_rec.update(mix=mix, mix_prob=float(config["mix_prob"]))
        if ema is not None:
            epoch_rec.update(ema_record())
        if optimizer != "sgd":
            epoch_rec.update(adam_record())
        if config.get("verbose", True):
            print_epoch(rank, epoch, mean)
            print(">>>>> Rank ", rank, ", epoch ", epoch, " Finished...\n", flush=True)
        logger.log(kind="epoch", epoch=epoch, mean_loss=mean, steps=i, num_batches=num_batches,
                   bytes_per_step=sync.bytes_per_step, comm=comm.stats.as_dict(),
                   phase_ms=timer.summary() if timer is not None else None, **({"lr": lr_now} if hyper_on else {}),
                   **epoch_rec)
        if config.get("checkpoint_dir"):
            save_checkpoint(os.path.join(config["checkpoint_dir"], "last.pt"), model, sync, epoch=epoch, step=step,
                            rank=rank, world=world,
                            **({"ema": ema.state_dict(ema_names) if rank == 0 else None} if ema is not None else {}))
        if evaluator is not None and (epoch + 1) % eval_every == 0:
            # after runner.join() above: the pass reads the parameters of the last update.  Its
            # all-reduce is accounted in the record, not in comm.stats / bytes_per_step, and its
            # time is kept out of the training throughput
            rec = dict(evaluator(), epoch=epoch)
            if ema is not None:
                # the same evaluator (same captured graph) on the averaged weights: exchanged in place,
                # no second model.  Every weight-derived tensor (Winograd / Toeplitz banks) is rebuilt
                # by each forward pass from the weights it finds, so nothing stale crosses a swap.
                ema.swap()
                try:
                    avg = evaluator()
                finally:
                    ema.swap()
                rec.update(ema_loss=avg["loss"], ema_top1=avg["top1"], ema_topk=avg["topk"],
                           eval_s=rec["eval_s"] + avg["eval_s"], comm_bytes=rec["comm_bytes"] + avg["comm_bytes"])
            if device.type == "cuda":
                torch.cuda.synchronize()
            eval_s += rec["eval_s"]
            evals.append(rec)
            if config.get("verbose", True):
                print_eval(rank, epoch, rec)
            logger.log(kind="eval", **rec)
    if device.type == "cuda":
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t_start - eval_s  # training time: evaluation is reported as eval_s
    _log(config, "All Task Finished")
    _log(config, "==============================\n")
    flat = sync.flat_weights
    if flat is None:
        flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    summary = {"epoch_losses": losses, "steps": step, "elapsed_s": elapsed, "samples": samples,
               "samples_per_s": samples / elapsed if elapsed > 0 else None,
               "bytes_per_step": sync.bytes_per_step, "comm": comm.stats.as_dict(),
               "comm_backend": comm.backend, "world_size": world, "per_rank_batch": bsz, "graph_mode": graph_mode,
               "param_checksum": float(flat.double().sum().item())}
    if hyper_on:
        summary["lr_schedule"] = schedule.schedule
        summary["weight_decay"] = weight_decay
    if label_smoothing:
        summary["label_smoothing"] = label_smoothing
    if mix != "none":
        summary["mix"] = mix
        summary["mix_prob"] = float(config["mix_prob"])
    if clip_on:
        summary["clipped_steps"] = sync.clip_stats()["clipped"] - clipped_base
        summary["max_grad_norm"] = max_grad_norm
    if eval_every:
        summary["eval"] = evals
        summary["eval_s"] = eval_s
    if ema is not None:
        summary.update(ema_record())
    if optimizer != "sgd":
        summary.update(adam_record())
    logger.log(kind="summary", **{k: v for k, v in summary.items()})
    logger.close()
    if ema is not None:
        summary["ema"] = ema
    summary["model"] = model
    summary["sync"] = sync
    return summary


def ema_targets(model: torch.nn.Module):
    """``(names, tensors)`` a weight EMA of ``model`` covers: every parameter, then every persistent
    fp32 buffer (BatchNorm running statistics), under their ``state_dict`` names.  Integer buffers
    (``num_batches_tracked``) and non-persistent scratch are left out."""
    live = model.state_dict(keep_vars=True)  # persistent tensors only, the objects themselves
    params = {id(p) for p in model.parameters()}
    seen, names = set(), []
    for want_param in (True, False):
        for k, v in live.items():
            if (id(v) in params) == want_param and id(v) not in seen and (want_param or v.dtype == torch.float32):
                seen.add(id(v))  # a tied tensor is averaged once, under its first name
                names.append(k)
    return names, [live[k].detach() for k in names]


def _clip_step_record(stats) -> Dict[str, Any]:
    return {"grad_norm": stats["norm"], "clip_coef": stats["coef"]}


def _ring_wire(payload: int, n: int) -> float:
    return 0.0 if n <= 1 else 2.0 * (n - 1) / n * payload


def _same_shape(a, b) -> bool:
    if isinstance(a, dict):
        return all(a[k].shape == b[k].shape for k in a)
    return all(x.shape == y.shape for x, y in zip(a, b))


def _delivered(static_batch, batch) -> bool:
    """True when the loader wrote ``batch`` straight into the static tensors (DeviceLoader.deliver_into)."""
    return not isinstance(batch, dict) and batch[0] is static_batch[0]


def _clone_batch(b):
    if isinstance(b, dict):
        return {k: v.clone() for k, v in b.items()}
    return tuple(v.clone() for v in b)


def _copy_batch(dst, src):
    if isinstance(dst, dict):
        for k in dst:
            dst[k].copy_(src[k], non_blocking=True)
    else:
        for d, s in zip(dst, src):
            d.copy_(s, non_blocking=True)
