"""csrc/image_batch.hip: image_mix_batch_kernel against the CPU twin (ops/image_batch.py), bitwise on
all four outputs and the error word: the cases of tests/test_mix_batch_cpu.py, a second seed / epoch,
more than one workgroup wave, in-place writes inside larger tensors, bad indices (never
dereferenced) and a captured launch replayed on changed indices."""
import pytest
import torch

from network_distributed_pytorch_amd import ops

from .image_rule import MEANSTD

pytestmark = pytest.mark.gpu

N = 40
IDX = [(7 * k + 3) % 40 for k in range(13)]
MODES = ("mixup", "cutmix", "mixup_cutmix")


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(0)
    return {C: (torch.randint(0, 256, (N, C, 32, 32), dtype=torch.uint8, generator=g),
                torch.randint(0, 10, (N,), generator=g)) for C in (3, 1)}


def _both(src, labels, idx, device, **kw):
    """(device result, CPU-twin result) of one call, each with its own error word."""
    err_d = torch.zeros(1, dtype=torch.int32, device=device)
    err_c = torch.zeros(1, dtype=torch.int32)
    got = ops.image_mix_batch(src.to(device), labels.to(device), idx.to(device), err=err_d, **kw)
    ref = ops.image_mix_batch(src, labels, idx, err=err_c, **kw)
    torch.cuda.synchronize()
    return got, ref, int(err_d), int(err_c)


def _assert_same(got, ref):
    for name, a, b in zip(("out", "target", "target_b", "lam"), got, ref):
        assert a.dtype == b.dtype and torch.equal(a.cpu(), b), name


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed,epoch", [(3, 2), (714, 5)])
def test_kernel_equals_cpu_twin(device, data, C, mode, seed, epoch):
    src, labels = data[C]
    mean, std = (v[:C] for v in MEANSTD["cifar"])
    idx = torch.tensor(IDX, dtype=torch.int64)
    for flip in (True, False):
        for mix_prob in (0.5, 1.0):
            got, ref, err_d, err_c = _both(src, labels, idx, device, mode=mode, mix_prob=mix_prob, rows=16, mean=mean,
                                           std=std, pad=4, flip=flip, seed=seed, epoch=epoch, pad_target=-7)
            _assert_same(got, ref)
            assert err_d == err_c == 0
            mixed = int((ref[3][:13] != 1).sum())  # lam == 1: unmixed (or a CutMix box that came out empty)
            print(f"C={C} {mode} seed={seed} epoch={epoch} flip={flip} p={mix_prob}: {mixed} of 12 rows mixed")
            assert 1 <= mixed <= 12


@pytest.mark.parametrize("m,B", [(1, 1), (2, 2), (67, 67), (64, 70)])
def test_one_row_even_batches_and_many_workgroups(device, data, m, B):
    src, labels = data[3]
    mean, std = MEANSTD["half"]
    idx = torch.randint(0, N, (m,), generator=torch.Generator().manual_seed(m))
    for pad, flip in ((0, False), (4, True)):
        got, ref, err_d, err_c = _both(src, labels, idx, device, mode="mixup_cutmix", mix_prob=0.75, rows=B,
                                       mean=mean, std=std, pad=pad, flip=flip, seed=9, epoch=1)
        _assert_same(got, ref)
        assert err_d == err_c == 0
    if m == 1:  # its own partner: never mixed
        assert float(ref[3][0]) == 1.0 and int(ref[2][0]) == int(ref[1][0])


def test_outputs_are_views_inside_sentinel_buffers(device, data):
    src, labels = data[3]
    B, lead, total = 16, 2, 21
    big = torch.full((total, 3, 32, 32), 777.0, device=device)
    big_t = torch.full((total,), 777, dtype=torch.int64, device=device)
    big_b = torch.full((total,), 777, dtype=torch.int64, device=device)
    big_l = torch.full((total,), 777.0, device=device)
    mean, std = MEANSTD["cifar"]
    kw = dict(mode="mixup_cutmix", mix_prob=0.5, rows=B, mean=mean, std=std, pad=4, flip=True, seed=3, epoch=2,
              pad_target=-1)
    idx = torch.tensor(IDX)
    ops.image_mix_batch(src.to(device), labels.to(device), idx.to(device), out=big[lead:], out_target=big_t[lead:],
                        out_target_b=big_b[lead:], out_lam=big_l[lead:], **kw)
    ref = ops.image_mix_batch(src, labels, idx, **kw)
    for buf, r in zip((big, big_t, big_b, big_l), ref):
        assert torch.equal(buf[lead: lead + B].cpu(), r)
        assert bool((buf[:lead] == 777).all()) and bool((buf[lead + B:] == 777).all())


@pytest.mark.parametrize("mode", MODES)
def test_bad_indices_are_never_dereferenced_and_set_the_error_word(device, data, mode):
    src, labels = data[3]
    mean, std = MEANSTD["half"]
    # partners 0-7, 1-6, 2-5, 3-4: row 5 has a good own index and a bad partner, rows 1, 2, 6 a bad own index
    idx = torch.tensor([3, -1, 2 ** 40, N - 1, 7, 2, -2 ** 40, 5])
    got, ref, err_d, err_c = _both(src, labels, idx, device, mode=mode, mix_prob=1.0, rows=9, mean=mean, std=std,
                                   pad=4, flip=True, seed=1, epoch=1)
    _assert_same(got, ref)
    assert err_d == err_c == 1
    out, tgt, tgt_b, lam = (t.cpu() for t in got)
    for b in (1, 2, 6, 8):
        assert float(out[b].abs().max()) == 0 and int(tgt[b]) == int(tgt_b[b]) == -100 and float(lam[b]) == 1.0
    assert int(tgt_b[0]) == int(labels[5]) and int(tgt_b[3]) == int(labels[7])
    assert int(tgt[5]) == int(tgt_b[5]) == int(labels[2]) and float(lam[5]) == 1.0  # unmixed, not padding
    assert float(out[5].abs().max()) > 0
    _, _, err_d, err_c = _both(src, labels, idx[[0, 3, 4, 7]], device, mode=mode, mean=mean, std=std)
    assert err_d == err_c == 0


def test_binding_rejects_bad_arguments(device, data):
    src, labels = (t.to(device) for t in data[3])
    idx = torch.tensor([0, 1], device=device)
    X = ops.ext()
    out, tgt = torch.empty(2, 3, 32, 32, device=device), torch.empty(2, dtype=torch.int64, device=device)
    tgt_b, lam = torch.empty(2, dtype=torch.int64, device=device), torch.empty(2, device=device)
    err = torch.zeros(1, dtype=torch.int32, device=device)
    sc, sh = ops.image_norm_constants(*MEANSTD["half"])
    tail = (sc, sh, 0, False, 0, 0, -100, err)
    with pytest.raises(RuntimeError, match="m <= B"):
        X.image_mix_batch(src, labels, idx, out, tgt, tgt_b, lam, 3, 2, *tail, 1, 1 << 24)
    with pytest.raises(RuntimeError, match="out_target_b"):
        X.image_mix_batch(src, labels, idx, out, tgt, tgt_b[:1], lam, 2, 2, *tail, 1, 1 << 24)
    with pytest.raises(RuntimeError, match="out_lam"):
        X.image_mix_batch(src, labels, idx, out, tgt, tgt_b, lam.double(), 2, 2, *tail, 1, 1 << 24)
    with pytest.raises(RuntimeError, match="mode"):
        X.image_mix_batch(src, labels, idx, out, tgt, tgt_b, lam, 2, 2, *tail, 0, 1 << 24)
    with pytest.raises(RuntimeError, match="thr"):
        X.image_mix_batch(src, labels, idx, out, tgt, tgt_b, lam, 2, 2, *tail, 1, (1 << 24) + 1)
    with pytest.raises(RuntimeError, match="uint8"):
        X.image_mix_batch(src.float(), labels, idx, out, tgt, tgt_b, lam, 2, 2, *tail, 1, 1 << 24)


def test_captured_launch_replays_on_changed_indices(device, data):
    src_c, labels_c = data[3]
    src, labels = src_c.to(device), labels_c.to(device)
    mean, std = MEANSTD["cifar"]
    kw = dict(mode="mixup_cutmix", mix_prob=0.5, rows=8, mean=mean, std=std, pad=4, flip=True, seed=714, epoch=6)
    idx = torch.tensor([0, 1, 2, 3, 4, 5], device=device)
    bufs = dict(out=torch.zeros(8, 3, 32, 32, device=device),
                out_target=torch.zeros(8, dtype=torch.int64, device=device),
                out_target_b=torch.zeros(8, dtype=torch.int64, device=device), out_lam=torch.zeros(8, device=device))
    err = torch.zeros(1, dtype=torch.int32, device=device)
    ops.image_mix_batch(src, labels, idx, err=err, **bufs, **kw)  # eager warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.image_mix_batch(src, labels, idx, err=err, **bufs, **kw)
    for new in ([N - 1, 0, 9, 9, 30, 12], [7, 36, 1, 22, 5, 38]):
        idx.copy_(torch.tensor(new, device=device))
        for t in bufs.values():
            t.fill_(-5)
        g.replay()
        torch.cuda.synchronize()
        ref = ops.image_mix_batch(src_c, labels_c, torch.tensor(new), **kw)
        _assert_same(tuple(bufs.values()), ref)
    assert int(err) == 0
