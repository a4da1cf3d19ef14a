"""Typed training configuration.

The reference keeps each experiment's settings in a module-level ``config`` dict
(ddp_powersgd_guide_cifar10/ddp_init.py:24-39); the workloads here keep that dict API.
:class:`TrainConfig` is the typed schema behind it: every key the engine reads, with its
type, default and allowed values.  :func:`validate_config` checks a dict against it (unknown
keys, types, choices, cross-field rules) and returns it with defaults filled in, so a typo
(``-reducer_rnak``) or an impossible combination fails at start-up with a clear message
instead of a KeyError deep in a run.
"""
from __future__ import annotations

import dataclasses
import typing
from typing import Any, Dict, Optional

import numpy as np

__all__ = ["TrainConfig", "validate_config", "ConfigError"]


class ConfigError(ValueError):
    pass


GRAD_SYNCS = ("powersgd", "powersgd-adamw", "powersgd-ref", "powersgd-api", "dense", "dense-ref", "local-sgd-nesterov",
              "local-adamw")
PSGD_ENGINE_SYNCS = ("powersgd", "powersgd-adamw")  # the fused native engine (parallel/powersgd.py)
TASKS = ("cifar", "imdb", "mlp")
GRAPH_MODES = ("auto", "full", "piecewise", "none")
LINKS = ("none", "1g", "10g", "100g")
BACKENDS = ("nccl", "gloo")
AUGMENTS = ("none", "crop_flip")
NORMALIZES = ("half", "cifar")
MIXES = ("none", "mixup", "cutmix", "mixup_cutmix")  # ops/image_batch.py: image_mix_batch
LR_SCHEDULES = ("constant", "step", "cosine")  # utils/schedule.py
OPTIMIZERS = ("sgd", "adamw")
ADAMW_GRAD_SYNCS = ("dense", "dense-ref", "powersgd-ref", "powersgd-api")  # parallel/trainer.py ADAMW_SYNCS


@dataclasses.dataclass
class TrainConfig:
    # reference keys (ddp_init.py config dicts)
    seed: int = 714
    rank: int = 0
    cuda_rank: int = 0
    n_workers: int = 1
    distributed_init_file: Optional[str] = None
    output_dir: str = "./output.tmp"
    distributed_backend: str = "nccl"
    init_method: Optional[str] = None
    timeout_s: float = 600
    learning_rate: float = 1e-3
    momentum: float = 0.9
    nesterov: bool = False
    training_epochs: int = 1
    batch_size: int = 32
    reducer_rank: int = 4
    # additions
    task: str = "cifar"
    model: str = "resnet18"
    num_classes: int = 1000
    global_batch: Optional[int] = 512
    seq_len: int = 512
    grad_sync: str = "powersgd"
    dataset_size: Optional[int] = None
    data_seed: int = 0
    max_steps_per_epoch: Optional[int] = None
    graph_mode: str = "auto"
    link: str = "none"
    emulate_world: Optional[int] = None
    bucket_mb: Optional[float] = None
    reuse_query: bool = True
    overlap: Optional[bool] = None
    psgd_groups: Optional[int] = None
    checkpoint_dir: Optional[str] = None
    resume: Optional[str] = None
    log_file: Optional[str] = None
    log_every: int = 1
    check_replicas_every: int = 0
    check_health_every: int = 50  # host check of flag-wait / MGS / RCCL errors (fatal), 0 = epoch end only
    write_grad: bool = False
    verbose: bool = True
    trace_phases: bool = False
    toy_mlp_steps: int = 0
    deterministic: bool = True  # MIOpen's deterministic solver while the run lasts (engine.setup)
    # held-out evaluation (engine.evaluate): fused loss / top-1 / top-k pass over data never trained on
    eval_every: int = 0  # evaluate every N epochs; 0 = off (no held-out data is built)
    eval_size: Optional[int] = None  # held-out size (cifar 10,000, mlp 256; imdb: cap on its validation split)
    eval_topk: int = 5  # k of the top-k accuracy
    # real CIFAR-10 from files (utils/cifar.py), held as bytes; batches by ops/image_batch.py
    data_root: Optional[str] = None  # directory with the CIFAR-10 files; None = synthetic data
    augment: str = "none"  # "crop_flip": random crop (pad 4) + horizontal flip, training only
    normalize: str = "half"  # "half" = 0.5 / 0.5 per channel (the reference), "cifar" = dataset statistics
    # learning-rate schedule (utils/schedule.py) and L2 weight decay; the update kernels read both from
    # the optimiser's device block, so they reach a captured step too
    lr_schedule: str = "constant"  # after the warm-up: "constant", "step" (milestones / gamma), "cosine" (to lr_min)
    lr_warmup_steps: int = 0  # linear warm-up over the first N steps: base * (s + 1) / N
    lr_min: float = 0.0  # floor of the cosine
    lr_milestones: str = ""  # "step": comma-separated epochs, e.g. "15,25"
    lr_gamma: float = 0.1  # "step": factor per milestone passed
    weight_decay: float = 0.0  # L2, every parameter (torch.optim.SGD's weight_decay)
    max_grad_norm: float = 0.0  # clip by the global L2 norm (ops/gradclip.py); 0 = off, inf = measure only
    # regularisers of the training loss: label smoothing (ops/loss.py, every task) and mixup / CutMix of the
    # byte-image batches (ops/image_batch.py), lambda ~ Beta(1, 1); both reach a captured step
    label_smoothing: float = 0.0  # eps of CrossEntropyLoss(label_smoothing=eps), 0 <= eps < 1
    mix: str = "none"  # "mixup", "cutmix", "mixup_cutmix" (either, per row); training only, needs data_root
    mix_prob: float = 1.0  # probability that a row is mixed at all, 0 < p <= 1
    # exponential moving average of the weights (ops/ema.py), evaluated and checkpointed next to them
    ema_decay: float = 0.0  # 0 = off; 0 < decay < 1: shadow += (1 - d) * (weights - shadow) after every step
    ema_warmup: bool = True  # d = min(decay, (n + 1) / (n + 10)) for update n (the TF / timm warm-up)
    # the optimiser behind the gradient sync: "sgd" (momentum) or "adamw" (ops/adamw.py; dense, dense-ref,
    # powersgd-ref and powersgd-api only; grad_sync="powersgd-adamw" is the fused engine with AdamW and sets
    # it); with "adamw", weight_decay is the decoupled decay
    optimizer: str = "sgd"
    adam_beta1: float = 0.9
    adam_beta2: float = 0.999
    adam_eps: float = 1e-8
    decay_1d: bool = True  # False: biases, LayerNorm / BatchNorm weights (tensors of <= 1 dimension) do not decay


_FIELDS = {f.name: f for f in dataclasses.fields(TrainConfig)}
_HINTS = typing.get_type_hints(TrainConfig)


def _check_type(name: str, value: Any):
    hint = _HINTS[name]
    optional = typing.get_origin(hint) is typing.Union and type(None) in typing.get_args(hint)
    base = [a for a in typing.get_args(hint) if a is not type(None)][0] if optional else hint
    if value is None:
        if optional:
            return None
        raise ConfigError(f"config[{name!r}] must not be None")
    if base is bool:
        if isinstance(value, bool) or value in (0, 1):
            return bool(value)
    elif base is int:
        if isinstance(value, int) and not isinstance(value, bool):
            return value
        if isinstance(value, float) and value.is_integer():
            return int(value)
    elif base is float:
        if isinstance(value, (int, float)) and not isinstance(value, bool):
            return float(value)
    elif base is str:
        if isinstance(value, str):
            return value
    raise ConfigError(f"config[{name!r}] = {value!r}: expected {base.__name__}{' or None' if optional else ''}")


def validate_config(config: Dict[str, Any], strict: bool = True) -> Dict[str, Any]:
    """Type-check ``config`` in place against :class:`TrainConfig` and fill defaults.

    ``strict``: unknown keys raise (set False to only warn via the returned dict's
    ``_unknown_keys``).  Returns the same dict object (the workloads mutate it)."""
    unknown = sorted(k for k in config if k not in _FIELDS and not k.startswith("_"))
    if unknown and strict:
        raise ConfigError(f"unknown config keys {unknown}; known: {sorted(_FIELDS)}")
    for name, f in _FIELDS.items():
        if name not in config:
            config[name] = f.default
        else:
            config[name] = _check_type(name, config[name])
    c = config
    for key, allowed in (("grad_sync", GRAD_SYNCS), ("task", TASKS), ("graph_mode", GRAPH_MODES), ("link", LINKS),
                         ("distributed_backend", BACKENDS), ("augment", AUGMENTS), ("normalize", NORMALIZES),
                         ("lr_schedule", LR_SCHEDULES), ("mix", MIXES)):
        if c[key] not in allowed:
            raise ConfigError(f"config[{key!r}] = {c[key]!r}; allowed: {list(allowed)}")
    if c["n_workers"] < 1 or not 0 <= c["rank"] < c["n_workers"]:
        raise ConfigError(f"rank {c['rank']} / n_workers {c['n_workers']}: need 0 <= rank < n_workers")
    if not 1 <= c["reducer_rank"] <= 64:
        raise ConfigError("reducer_rank must be in [1, 64] (csrc kMaxRank)")
    if c["learning_rate"] <= 0 or not 0 <= c["momentum"] < 1:
        raise ConfigError("learning_rate > 0 and 0 <= momentum < 1 required")
    if c["global_batch"] is not None and c["global_batch"] < c["n_workers"]:
        raise ConfigError(f"global_batch {c['global_batch']} < n_workers {c['n_workers']}: empty per-rank batch")
    if c["emulate_world"] is not None and c["emulate_world"] < 1:
        raise ConfigError("emulate_world must be >= 1")
    if c["bucket_mb"] is not None and c["bucket_mb"] <= 0:
        raise ConfigError("bucket_mb must be > 0")
    if c["psgd_groups"] is not None and c["psgd_groups"] < 1:
        raise ConfigError("psgd_groups must be >= 1")
    if c["graph_mode"] in ("full", "piecewise") and c["grad_sync"] in PSGD_ENGINE_SYNCS and not c["reuse_query"]:
        raise ConfigError("graph capture needs reuse_query=True (the per-step query re-draw is host-side)")
    if c["log_every"] < 1 or c["training_epochs"] < 0 or c["timeout_s"] <= 0:
        raise ConfigError("log_every >= 1, training_epochs >= 0, timeout_s > 0 required")
    if c["eval_every"] < 0 or c["eval_topk"] < 1 or (c["eval_size"] is not None and c["eval_size"] < 1):
        raise ConfigError("eval_every >= 0, eval_topk >= 1 and eval_size >= 1 (or None) required")
    if c["data_root"] is not None and c["task"] != "cifar":
        raise ConfigError(f"data_root is for task='cifar' only (task = {c['task']!r})")
    if c["augment"] != "none" and c["data_root"] is None:
        raise ConfigError(f"augment = {c['augment']!r} needs data_root (the synthetic data is never augmented)")
    if c["mix"] != "none" and c["data_root"] is None:
        raise ConfigError(f"mix = {c['mix']!r} needs data_root (the synthetic data is never mixed)")
    if not 0 <= c["label_smoothing"] < 1:  # NaN fails the comparison too
        raise ConfigError(f"label_smoothing = {c['label_smoothing']} must lie in [0, 1)")
    if not 0 < c["mix_prob"] <= 1 or c["mix_prob"] * (1 << 24) < 1:
        raise ConfigError(f"mix_prob = {c['mix_prob']} must lie in (0, 1] (resolution 2^-24)")
    if c["weight_decay"] < 0:
        raise ConfigError("weight_decay must be >= 0")
    if not 0 <= c["ema_decay"] < 1 or (c["ema_decay"] > 0 and not 0 < np.float32(c["ema_decay"]) < 1):
        # NaN fails the comparison too; a decay that rounds to 0 or 1 in fp32 is no average
        raise ConfigError(f"ema_decay = {c['ema_decay']} must lie in [0, 1) (0 = off)")
    if c["optimizer"] not in OPTIMIZERS:
        raise ConfigError(f"config['optimizer'] = {c['optimizer']!r}; allowed: {list(OPTIMIZERS)}")
    for key in ("adam_beta1", "adam_beta2"):  # as fp32, what the kernel receives; NaN fails the comparison too
        if not 0 <= np.float32(c[key]) < 1:
            raise ConfigError(f"{key} = {c[key]} must lie in [0, 1)")
    if not np.float32(c["adam_eps"]) > 0 or not np.isfinite(c["adam_eps"]):
        raise ConfigError(f"adam_eps = {c['adam_eps']} must be a finite number > 0 (as fp32)")
    if c["grad_sync"] == "powersgd-adamw":  # the kind is the optimiser choice, as local-adamw
        c["optimizer"] = "adamw"
    elif c["optimizer"] == "adamw" and c["grad_sync"] not in ADAMW_GRAD_SYNCS:
        raise ConfigError(f"optimizer='adamw' is not available with grad_sync={c['grad_sync']!r} (the fused PowerSGD "
                          f"engine and the local optimisers have no AdamW); allowed: {list(ADAMW_GRAD_SYNCS)}")
    if not c["max_grad_norm"] >= 0:  # NaN fails the comparison too
        raise ConfigError(f"max_grad_norm = {c['max_grad_norm']} must be >= 0 (0 = off, inf = measure only)")
    if c["max_grad_norm"] > 0 and c["grad_sync"] in PSGD_ENGINE_SYNCS and c["overlap"]:
        raise ConfigError(f"grad_sync={c['grad_sync']!r} with overlap=True cannot be combined with max_grad_norm > 0: the "
                          "global norm needs every gradient before a group's pipeline may start")
    if not 0 <= c["lr_min"] <= c["learning_rate"]:
        raise ConfigError(f"lr_min {c['lr_min']} must lie in [0, learning_rate = {c['learning_rate']}]")
    if c["lr_warmup_steps"] < 0 or not c["lr_gamma"] > 0:
        raise ConfigError("lr_warmup_steps >= 0 and lr_gamma > 0 required")
    from .schedule import parse_milestones
    try:
        milestones = parse_milestones(c["lr_milestones"])
    except ValueError as exc:
        raise ConfigError(f"config['lr_milestones'] = {c['lr_milestones']!r}: {exc}") from None
    if milestones and c["lr_schedule"] != "step":
        raise ConfigError(f"lr_milestones are for lr_schedule='step' only (lr_schedule = {c['lr_schedule']!r})")
    if unknown:
        config["_unknown_keys"] = unknown
    return config
