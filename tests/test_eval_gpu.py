"""Held-out evaluation on the device (engine.evaluate): the captured eval graph against the
eager pass, fresh weights after training steps, no side effects on the model, the trained
model's logits against an fp64 stock model, and the DistilBERT path."""
import pytest
import torch

from network_distributed_pytorch_amd import engine
from network_distributed_pytorch_amd.models import build_model, distilbert_base
from network_distributed_pytorch_amd.ops.metrics import ClassificationMetrics
from network_distributed_pytorch_amd.utils.data import SyntheticCIFAR10, SyntheticIMDb, SyntheticMLPData

from .metric_rule import loss_sum_fp64, rule_counts

pytestmark = pytest.mark.gpu

BATCH, TRAIN_N, EVAL_N = 32, 64, 40  # held-out: one full batch + 8 rows padded to 32


def _cfg(mode, eval_every):
    return engine.default_config(task="cifar", model="resnet18", num_classes=10, grad_sync="powersgd",
                                 training_epochs=1, dataset_size=TRAIN_N, global_batch=BATCH, eval_size=EVAL_N,
                                 max_steps_per_epoch=2, eval_every=eval_every, graph_mode=mode, verbose=False)


@pytest.fixture(scope="module")
def runs():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    out = {}
    for mode in ("full", "none"):
        for ev in (1, 0):
            torch.manual_seed(0)  # the engine builds the model from the current RNG
            out[mode, ev] = engine.run_task(_cfg(mode, ev))
    return out


@pytest.fixture(scope="module")
def heldout():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return SyntheticCIFAR10(TRAIN_N, seed=0, device=torch.device("cuda", 0), holdout=EVAL_N)[1]


def _padded_logits(model, columns, names, batch, call):
    """Eager eval-mode logits of every row, in batches cut and zero-padded as evaluate() does."""
    n = len(columns[names[0]])
    out = []
    model.eval()
    with torch.no_grad():
        for s in range(0, n, batch):
            m = min(batch, n - s)
            args = []
            for k in names:
                buf = torch.zeros((batch,) + tuple(columns[k].shape[1:]), dtype=columns[k].dtype,
                                  device=columns[k].device)
                buf[:m] = columns[k][s: s + m]
                args.append(buf)
            out.append(call(model, *args)[:m].clone())
    return torch.cat(out)


def _resnet_logits(model, heldout):
    return _padded_logits(model, heldout.columns, ["data"], BATCH, lambda m, x: m(x))


def _strip(rec):
    return {k: v for k, v in rec.items() if k not in ("eval_s", "epoch")}


def test_eval_graph_equals_eager_and_perturbs_nothing(runs, heldout):
    g, e = runs["full", 1], runs["none", 1]
    assert g["graph_mode"] == "full" and e["graph_mode"] == "none"
    assert len(g["eval"]) == len(e["eval"]) == 1 and g["eval"][0]["n"] == EVAL_N
    print("eval record, graph:", _strip(g["eval"][0]), "eager:", _strip(e["eval"][0]))
    # evaluation does not touch training: the eval_every=0 twins end on the same parameters
    assert g["param_checksum"] == runs["full", 0]["param_checksum"]
    assert e["param_checksum"] == runs["none", 0]["param_checksum"]
    assert g["epoch_losses"] == runs["full", 0]["epoch_losses"]
    assert "eval" not in runs["full", 0] and "eval" not in runs["none", 0]
    # on one set of weights, the captured pass and the eager pass give the same record, bitwise
    model = g["model"]
    dev = torch.device("cuda", 0)
    ev = engine.Evaluator(model, heldout, batch=BATCH, device=dev, topk=5, graph_mode="full")
    first, second = ev(), ev()  # warm-up + capture, then replays only
    assert ev.graph is not None and ev.replays >= 3
    eager = engine.evaluate(model, heldout, batch=BATCH, device=dev, topk=5, graph_mode="none")
    assert _strip(first) == _strip(second) == _strip(eager) == _strip(g["eval"][0])
    # the two training modes: identical eval records (counts exact, loss bitwise)
    assert _strip(g["eval"][0]) == _strip(e["eval"][0])


def test_eval_reads_fresh_weights(runs, heldout):
    """A stale Winograd / Toeplitz weight image inside the eval graph would show here: the
    engine's record (eval graph, after two training steps) against a FRESH instance (fresh
    weight banks) carrying the trained state_dict, run eagerly."""
    rec = runs["full", 1]["eval"][0]
    dev = torch.device("cuda", 0)
    fresh = build_model("resnet18", 10).to(dev)
    fresh.load_state_dict(runs["full", 1]["model"].state_dict())
    logits = _resnet_logits(fresh, heldout)
    target = heldout.columns["target"]
    n, c1, ck = rule_counts(logits, target, 5)
    assert (rec["n"], rec["top1"], rec["topk"], rec["k"]) == (n, c1 / n, ck / n, 5)
    ref = loss_sum_fp64(logits, target) / n
    assert abs(rec["loss"] - ref) <= 2e-6 * abs(ref) + 2e-6, (rec["loss"], ref)
    # and bitwise, through the same kernel in the same batches
    m = ClassificationMetrics(k=5, device=dev)
    for s in range(0, EVAL_N, BATCH):
        m.update(logits[s: s + BATCH].contiguous(), target[s: s + BATCH].contiguous())
    assert m.compute()["loss"] == rec["loss"]


def test_evaluate_has_no_side_effects(runs, heldout):
    model = runs["none", 1]["model"]
    dev = torch.device("cuda", 0)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    assert any(k.endswith("num_batches_tracked") for k in before)
    for training in (True, False):
        model.train(training)
        for mode in ("full", "none"):
            engine.evaluate(model, heldout, batch=BATCH, device=dev, topk=5, graph_mode=mode)
            assert model.training is training
    after = model.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v), k


def _rel_l2(a, b):
    return float((a.double().cpu() - b).norm() / b.norm())


def test_trained_logits_against_fp64_stock_model(runs, heldout):
    """Yardstick: the native model's own fp32 error against the fp64 stock model, measured on an
    UNTRAINED instance (no staleness possible).  Two SGD steps change the weights' scale only
    slightly, so the trained model stays within 4x of it; a one-step-stale weight image is
    orders of magnitude outside."""
    dev = torch.device("cuda", 0)
    x64 = heldout.columns["data"].double().cpu()

    def err(native):
        stock = build_model("resnet18", 10, fused_bn=False, gemm_convs=False).double()
        stock.load_state_dict({k: v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()
                               for k, v in native.state_dict().items()})
        stock.eval()
        with torch.no_grad():
            ref = stock(x64)
        return _rel_l2(_resnet_logits(native, heldout), ref)

    torch.manual_seed(1)
    yard = err(build_model("resnet18", 10).to(dev))
    trained = err(runs["full", 1]["model"])
    print(f"relative L2 error vs fp64 stock model: untrained {yard:.3e}, trained {trained:.3e}")
    assert trained <= 4 * yard, f"trained-model error {trained:.3e} vs untrained yardstick {yard:.3e} (bound 4x)"


@pytest.mark.parametrize("mode", ["full", "none"])
def test_evaluate_distilbert(device, mode):
    torch.manual_seed(2)
    model = distilbert_base(n_layers=2).to(device)
    ds = SyntheticIMDb(n=10, seq_len=64, seed=4, device=device)
    rec = engine.evaluate(model, ds, batch=4, device=device, topk=5, graph_mode=mode)
    assert model.training
    logits = _padded_logits(model, ds.columns, ["input_ids", "attention_mask"], 4,
                            lambda m, ids, mask: m(ids, attention_mask=mask)[-1])
    n, c1, _ = rule_counts(logits, ds.columns["labels"], 2)
    assert (rec["n"], rec["top1"], rec["k"]) == (10, c1 / n, 5) and n == 10
    assert rec["topk"] is None  # k >= the 2-class head
    ref = loss_sum_fp64(logits, ds.columns["labels"]) / n
    assert abs(rec["loss"] - ref) <= 2e-6 * abs(ref) + 2e-6, (rec["loss"], ref)


IPC_WORKER = r'''
import os, sys, json
sys.path.insert(0, ROOT)
import torch, torch.distributed as dist
os.environ["NDP_COMM"] = "ipc"
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dist.init_process_group("gloo")
from network_distributed_pytorch_amd import engine
from network_distributed_pytorch_amd.models import ToyMLP
from network_distributed_pytorch_amd.parallel.comm import Communicator
from network_distributed_pytorch_amd.utils.data import SyntheticMLPData
dev = torch.device("cuda", 0)
comm = Communicator(device=dev)
assert comm.backend == "ipc-native", comm.backend
torch.manual_seed(5)
model = ToyMLP().to(dev)
val = SyntheticMLPData(8, seed=2, device=dev, holdout=101)[1]
rec = engine.evaluate(model, val, batch=16, comm=comm, device=dev, topk=2, graph_mode="full")
print("RESULT " + json.dumps(rec), flush=True)
dist.barrier()
dist.destroy_process_group()
'''


@pytest.mark.timeout(120)
def test_two_ranks_reduce_fp64_state_beside_the_fp32_ipc_plane(device):
    """The opt-in IPC data plane carries fp32 only: the fp64[4] state is reduced through the c10d
    group instead, never downcast.  Uneven shards (51 / 50 rows) and ragged tails at batch 16."""
    from .test_ipc_gpu import _spawn

    recs = _spawn(2, IPC_WORKER, timeout=100)
    assert _strip(recs[0]) == _strip(recs[1]) and recs[0]["comm_bytes"] == 32
    torch.manual_seed(5)
    model = build_model("mlp").to(device)
    val = SyntheticMLPData(8, seed=2, device=device, holdout=101)[1]
    single = engine.evaluate(model, val, batch=16, device=device, topk=2, graph_mode="none")
    for key in ("n", "top1", "topk", "k"):
        assert recs[0][key] == single[key], key
    assert recs[0]["n"] == 101
    assert abs(recs[0]["loss"] - single["loss"]) <= 1e-12 * abs(single["loss"])  # fp64 addition order only
