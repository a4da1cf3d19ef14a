"""csrc/image_batch.hip against the CPU rule (ops/image_batch.py), bitwise: shapes around one and
many workgroups, crop / flip at the extreme offsets, sentinel-guarded outputs, out-of-range
indices (never dereferenced) and a captured launch replayed on changed indices."""
import itertools

import pytest
import torch

from network_distributed_pytorch_amd import ops

from .image_rule import MEANSTD

pytestmark = pytest.mark.gpu

N = 37


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(11)
    return {C: (torch.randint(0, 256, (N, C, 32, 32), dtype=torch.uint8, generator=g),
                torch.randint(0, 10, (N,), generator=g)) for C in (1, 3)}


def _indices(m):
    base = [0, N - 1, 5, 5, 17, 0, N - 1, 20]  # repeats, the first and the last image
    g = torch.Generator().manual_seed(m)
    idx = base[:m] + torch.randint(0, N, (max(0, m - len(base)),), generator=g).tolist()
    return torch.tensor(idx, dtype=torch.int64)


def _both(src, labels, idx, device, **kw):
    """(device result, CPU-rule result) of one call, each with its own error word."""
    err_d = torch.zeros(1, dtype=torch.int32, device=device)
    err_c = torch.zeros(1, dtype=torch.int32)
    got = ops.image_batch(src.to(device), labels.to(device), idx.to(device), err=err_d, **kw)
    ref = ops.image_batch(src, labels, idx, err=err_c, **kw)
    torch.cuda.synchronize()
    return got, ref, int(err_d), int(err_c)


@pytest.mark.parametrize("B,m", [(1, 1), (3, 3), (8, 5), (64, 64), (67, 67)])
@pytest.mark.parametrize("C", [1, 3])
def test_kernel_equals_cpu_rule(device, data, B, m, C):
    src, labels = data[C]
    idx = _indices(m)
    for pad, flip, normalize in itertools.product((0, 1, 4), (False, True), ("half", "cifar")):
        mean, std = (v[:C] for v in MEANSTD[normalize])
        (out, tgt), (ref, ref_t), err_d, err_c = _both(src, labels, idx, device, rows=B, mean=mean, std=std, pad=pad,
                                                       flip=flip, seed=714, epoch=3, pad_target=-100)
        assert tuple(out.shape) == (B, C, 32, 32) and out.dtype == torch.float32
        assert torch.equal(out.cpu(), ref), (pad, flip, normalize)
        assert torch.equal(tgt.cpu(), ref_t)
        assert err_d == err_c == 0


def _find(pad, want):
    """A (seed, epoch, index) triple whose draw is ``want`` = (dx, dy, flip), by the Python twin."""
    for seed, epoch, i in itertools.product((714, 0, 1), range(8), range(N)):
        if ops.crop_flip_draw(seed, epoch, i, pad) == want:
            return seed, epoch, i
    raise AssertionError(f"no triple draws {want}")


@pytest.mark.parametrize("pad", [1, 4])
def test_corners_and_edges_at_extreme_offsets(device, pad):
    img = torch.full((1, 32, 32), 9, dtype=torch.uint8)
    img[0, 0, :], img[0, 31, :], img[0, :, 0], img[0, :, 31] = 50, 60, 70, 80  # top, bottom, left, right
    img[0, 0, 0], img[0, 0, 31], img[0, 31, 0], img[0, 31, 31] = 201, 202, 203, 204
    src = img.repeat(N, 1, 1, 1).contiguous()
    labels = torch.arange(N)
    mean, std = (0.0,), (1.0 / 255.0,)  # scale 1, shift 0: the output is the byte
    for dx, dy, fl in itertools.product((-pad, pad), (-pad, pad), (0, 1)):
        seed, epoch, i = _find(pad, (dx, dy, fl))
        (out, tgt), (ref, _), _, _ = _both(src, labels, torch.tensor([i]), device, mean=mean, std=std, pad=pad,
                                           flip=True, seed=seed, epoch=epoch)
        out = out.cpu()
        assert torch.equal(out, ref) and int(tgt) == i
        plane = out[0, 0]
        # where the source's corner (sy, sx) lands: y = sy - dy, x = sx - dx, mirrored when flipped
        for (sy, sx), byte in (((0, 0), 201), ((0, 31), 202), ((31, 0), 203), ((31, 31), 204)):
            y, x = sy - dy, sx - dx
            x = 31 - x if fl else x
            if 0 <= y < 32 and 0 <= x < 32:
                assert plane[y, x] == byte, (dx, dy, fl, sy, sx)
        # the padding: `pad` rows and columns of byte 0 on the sides the crop moved away from
        rows = slice(0, pad) if dy < 0 else slice(32 - pad, 32)
        edge = dx < 0 if not fl else dx > 0
        cols = slice(0, pad) if edge else slice(32 - pad, 32)
        assert float(plane[rows].abs().max()) == 0 and float(plane[:, cols].abs().max()) == 0
        assert int((plane == 0).sum()) == 32 * 32 - (32 - pad) ** 2


def test_outputs_are_views_inside_sentinel_buffers(device, data):
    src, labels = data[3]
    B, m, lead, total = 5, 3, 2, 9
    big = torch.full((total, 3, 32, 32), 777.0, device=device)
    big_t = torch.full((total,), 777, dtype=torch.int64, device=device)
    idx = torch.tensor([N - 1, 0, 8])
    mean, std = MEANSTD["cifar"]
    ops.image_batch(src.to(device), labels.to(device), idx.to(device), out=big[lead:], out_target=big_t[lead:], rows=B,
                    mean=mean, std=std, pad=4, flip=True, seed=2, epoch=5, pad_target=-1)
    ref, ref_t = ops.image_batch(src, labels, idx, rows=B, mean=mean, std=std, pad=4, flip=True, seed=2, epoch=5,
                                 pad_target=-1)
    assert torch.equal(big[lead: lead + B].cpu(), ref) and torch.equal(big_t[lead: lead + B].cpu(), ref_t)
    assert bool((big[:lead] == 777.0).all()) and bool((big[lead + B:] == 777.0).all())
    assert bool((big_t[:lead] == 777).all()) and bool((big_t[lead + B:] == 777).all())


def test_out_of_range_indices_are_padding_and_set_the_error_word(device, data):
    src, labels = data[3]
    idx = torch.tensor([3, -1, N, N - 1, 2 ** 40, -2 ** 40])
    mean, std = MEANSTD["half"]
    (out, tgt), (ref, ref_t), err_d, err_c = _both(src, labels, idx, device, rows=7, mean=mean, std=std, pad=4,
                                                   flip=True, seed=1, epoch=1, pad_target=-100)
    assert torch.equal(out.cpu(), ref) and torch.equal(tgt.cpu(), ref_t)
    assert err_d == err_c == 1
    for b in (1, 2, 4, 5, 6):
        assert float(out[b].abs().max()) == 0 and int(tgt[b]) == -100
    assert int(tgt[0]) == int(labels[3]) and int(tgt[3]) == int(labels[N - 1])
    _, _, err_d, err_c = _both(src, labels, idx[[0, 3]], device, mean=mean, std=std)
    assert err_d == err_c == 0


def test_binding_rejects_bad_arguments(device, data):
    src, labels = (t.to(device) for t in data[3])
    idx = torch.tensor([0, 1], device=device)
    kw = dict(mean=MEANSTD["half"][0], std=MEANSTD["half"][1])
    with pytest.raises(ValueError):
        ops.image_batch(src, labels, idx, rows=1, **kw)  # m > B
    with pytest.raises(ValueError):
        ops.image_batch(src, labels, idx, pad=9, **kw)
    with pytest.raises(ValueError):
        ops.image_batch(src, labels, idx, out=torch.empty(1, 3, 32, 32, device=device), rows=2, **kw)
    X = ops.ext()
    out, tgt = torch.empty(2, 3, 32, 32, device=device), torch.empty(2, dtype=torch.int64, device=device)
    err = torch.zeros(1, dtype=torch.int32, device=device)
    sc, sh = ops.image_norm_constants(*MEANSTD["half"])
    with pytest.raises(RuntimeError, match="32"):
        X.image_batch(src[:, :, :16].contiguous(), labels, idx, out, tgt, 2, 2, sc, sh, 0, False, 0, 0, -100, err)
    with pytest.raises(RuntimeError, match="m <= B"):
        X.image_batch(src, labels, idx, out, tgt, 3, 2, sc, sh, 0, False, 0, 0, -100, err)
    with pytest.raises(RuntimeError, match="out_target"):
        X.image_batch(src, labels, idx, out, tgt[:1], 2, 2, sc, sh, 0, False, 0, 0, -100, err)
    with pytest.raises(RuntimeError, match="uint8"):
        X.image_batch(src.float(), labels, idx, out, tgt, 2, 2, sc, sh, 0, False, 0, 0, -100, err)


def test_captured_launch_replays_on_changed_indices(device, data):
    src_c, labels_c = data[3]
    src, labels = src_c.to(device), labels_c.to(device)
    mean, std = MEANSTD["cifar"]
    kw = dict(rows=8, mean=mean, std=std, pad=4, flip=True, seed=714, epoch=6, pad_target=-100)
    idx = torch.tensor([0, 1, 2, 3, 4], device=device)
    out = torch.zeros(8, 3, 32, 32, device=device)
    tgt = torch.zeros(8, dtype=torch.int64, device=device)
    err = torch.zeros(1, dtype=torch.int32, device=device)
    ops.image_batch(src, labels, idx, out=out, out_target=tgt, err=err, **kw)  # eager warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.image_batch(src, labels, idx, out=out, out_target=tgt, err=err, **kw)
    for new in ([N - 1, 0, 9, 9, 30], [7, 36, 1, 22, 5]):
        idx.copy_(torch.tensor(new, device=device))
        out.fill_(-5.0)
        tgt.fill_(-5)
        g.replay()
        torch.cuda.synchronize()
        ref, ref_t = ops.image_batch(src_c, labels_c, torch.tensor(new), **kw)
        assert torch.equal(out.cpu(), ref) and torch.equal(tgt.cpu(), ref_t)
    assert int(err) == 0
