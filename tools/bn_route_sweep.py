"""Run BatchNorm launch routes once, through the bindings, on seeded inputs, for a byte comparison
of two builds.

    python tools/bn_route_sweep.py [--dump DIR]

About fifty shapes at the sizes the models use, over the kinds of route of tools/bn_route_table.py:
each single-launch column-block width in its float4 and scalar form, the 8x8 maps with 1 / 2 / 4
row splits, the three-kernel and two-kernel paths, evaluation mode, slabs summed inside the launch
and by a sum launch first (with and without the grad-x addend), statistics from a conv epilogue,
misaligned operands, the float4 switch off, the BN pair and the stem tail.  It compares with
nothing and does not claim to be complete: the complete list of route variants (one call per
binding, mode, map size and route row of the recorded table) is tests/bn_route_cases.py, which
tests/test_bn_route_cases_cpu.py pins and tests/test_bn_routes_gpu.py runs against fp64.  Every
shape here runs one forward and
one backward per (residual, relu) case.  Inputs are made on the CPU from a seed and copied over, so
two builds see the same bits: with --dump every output is written as DIR/<case>.<name>.npy for a
byte comparison, and under a kernel trace the launches of two builds can be compared in order.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

CASES = [(False, False), (False, True), (True, True)]  # (residual, relu)

# (N, C, H, W), then options
SHAPES = [
    ((512, 512, 1, 1), {}), ((512, 2048, 1, 1), {}), ((512, 4096, 1, 1), {}), ((64, 512, 1, 1), {}),
    ((512, 256, 2, 2), {}), ((64, 256, 2, 2), {}), ((512, 1024, 2, 2), {}), ((512, 128, 4, 4), {}),
    ((64, 128, 4, 4), {}), ((100, 64, 4, 2), {}), ((40, 96, 2, 1), {}), ((3, 5, 1, 1), {}), ((130, 7, 2, 2), {}),
    ((64, 64, 8, 8), {}), ((128, 64, 8, 8), {}), ((7, 16, 8, 8), {}), ((129, 64, 8, 8), {}),
    ((600, 8, 2, 2), {}), ((8192, 64, 1, 1), {}), ((513, 40, 2, 1), {}),
    ((8, 64, 16, 16), {}), ((16, 24, 7, 7), {}), ((3, 5, 2, 3), {}), ((512, 64, 8, 8), {}), ((4, 8, 32, 32), {}),
    ((64, 128, 4, 4), {"single": False}), ((64, 256, 2, 2), {"single": False}),
    ((8, 64, 16, 16), {"training": False}), ((64, 512, 1, 1), {"training": False}),
    ((64, 128, 4, 4), {"nslab": 2}), ((64, 128, 4, 4), {"nslab": 8}), ((129, 64, 8, 8), {"nslab": 3}),
    ((64, 64, 8, 8), {"nslab": 4}), ((600, 8, 2, 2), {"nslab": 2}), ((16, 24, 7, 7), {"nslab": 2}),
    ((8, 64, 16, 16), {"ext": True}), ((129, 64, 8, 8), {"ext": True}),
    ((130, 8, 4, 4), {"shift": True}), ((20, 16, 8, 8), {"shift": True}), ((4, 8, 16, 16), {"shift": True}),
    ((600, 8, 2, 2), {"shift": True}),
    ((512, 256, 2, 2), {"vec4": False}), ((64, 64, 8, 8), {"vec4": False}), ((64, 128, 4, 4), {"vec4": False}),
]
PAIRS = [((64, 128, 4, 4), {}), ((512, 256, 2, 2), {}), ((64, 512, 1, 1), {}), ((512, 512, 1, 1), {}),
         ((64, 128, 4, 4), {"nslab": 3, "nslab2": 5}), ((100, 256, 2, 2), {"nslab": 8, "nslab2": 2}),
         ((130, 8, 4, 4), {"shift": True})]
STEMS = [((8, 64, 16, 16), {}), ((8, 64, 16, 16), {"ext": True}), ((5, 16, 12, 12), {})]


class Sweep:
    def __init__(self, X, dev, dump):
        self.X, self.dev, self.dump = X, dev, dump
        self.gen = torch.Generator().manual_seed(1234)
        self.count = 0

    def rand(self, *shape, scale=1.0, bias=0.0, shift=False):
        """seeded on the CPU; shift: a contiguous view one float past a 16-byte boundary"""
        t = torch.randn(*shape, generator=self.gen) * scale + bias
        if not shift:
            return t.to(self.dev)
        buf = torch.empty(t.numel() + 1, device=self.dev)
        v = buf[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        return v

    def slabs(self, t, n):
        """n slabs shaped like t (the bindings take slabs of whole float4 tensors only), or None"""
        if n < 2 or t.numel() % 4 != 0:
            return None
        return torch.stack([self.rand(*t.shape, scale=0.6) for _ in range(n)]).contiguous()

    def save(self, case, **tensors):
        self.count += len(tensors)
        if self.dump:
            for k, v in tensors.items():
                if v is not None:
                    np.save(os.path.join(self.dump, f"{case}.{k}.npy"), v.detach().cpu().numpy())

    def params(self, C):
        return dict(gamma=self.rand(C, scale=0.3, bias=1.0), beta=self.rand(C, scale=0.3),
                    rmean=self.rand(C, scale=0.1), rvar=self.rand(C, scale=0.05, bias=1.0).abs(),
                    nbt=torch.zeros(1, dtype=torch.int64, device=self.dev),
                    sm=torch.zeros(C, device=self.dev), si=torch.zeros(C, device=self.dev))

    def part(self, N, C, HW):
        return torch.zeros(int(self.X.bn_part_numel(N, C, HW)), dtype=torch.float64, device=self.dev)

    @staticmethod
    def image_stats(a, b, C):
        """[C][N][2] fp64 per-image sums of a and a * b, as a conv epilogue emits them"""
        a, b = a.double().cpu(), b.double().cpu()
        N = a.shape[0]
        s = torch.stack([a.reshape(N, C, -1).sum(2), (a * b).reshape(N, C, -1).sum(2)], dim=2)  # [N][C][2]
        return s.permute(1, 0, 2).contiguous()

    def bn(self, tag, shape, single=True, training=True, nslab=0, ext=False, shift=False, vec4=True):
        X, (N, C, H, W) = self.X, shape
        HW = H * W
        X.bn_set_vec4(vec4)
        try:
            for res, relu in CASES:
                case = f"{tag}.res{int(res)}relu{int(relu)}"
                p = self.params(C)
                part = self.part(N, C, HW)
                x = self.rand(*shape, scale=1.7, bias=0.4, shift=shift)
                r = self.rand(*shape, shift=shift) if res else None
                xpart = self.slabs(x, nslab)
                if xpart is not None:
                    x = torch.empty_like(x)  # the launch writes the summed input
                xst = self.image_stats(x, x, C).to(self.dev) if ext and training and xpart is None else None
                y = torch.empty_like(x)
                X.bn_fwd(x, r, y, p["gamma"], p["beta"], p["rmean"], p["rvar"], p["nbt"] if training else None,
                         p["sm"], p["si"], part, 1e-5, 0.1, relu, training, single, xpart,
                         nslab if xpart is not None else 0, xst, N if xst is not None else 0)
                self.save(case, y=y, x=x, save_mean=p["sm"], save_invstd=p["si"], running_mean=p["rmean"],
                          running_var=p["rvar"], num_batches_tracked=p["nbt"])
                if not training:
                    continue
                dy = self.rand(*shape, shift=shift)
                dypart = self.slabs(dy, nslab) if xpart is not None else None
                dyadd = self.rand(*shape) if dypart is not None and res else None
                if dypart is not None:
                    dy = torch.empty_like(dy)
                dst = None
                if ext and dypart is None:  # sums of dz and dz * xhat per image
                    dz = dy * (y > 0) if relu else dy
                    xh = (x - p["sm"].view(1, C, 1, 1)) * p["si"].view(1, C, 1, 1)
                    dst = self.image_stats(dz, xh, C).to(self.dev)
                dx = torch.empty_like(y)
                dres = torch.empty_like(y) if res else None
                dg, db = torch.zeros(C, device=self.dev), torch.zeros(C, device=self.dev)
                X.bn_bwd(dy, y if relu else None, x, p["gamma"], p["sm"], p["si"], dx, dres, dg, db, part, relu, single,
                         dypart, nslab if dypart is not None else 0, dyadd, None, dst, N if dst is not None else 0)
                self.save(case, dx=dx, dres=dres, dgamma=dg, dbeta=db, dy=dy)
        finally:
            X.bn_set_vec4(True)

    def pair(self, tag, shape, nslab=0, nslab2=0, shift=False):
        X, (N, C, H, W) = self.X, shape
        p, p2 = self.params(C), self.params(C)
        x = self.rand(*shape, scale=1.3, bias=0.2)
        x2 = self.rand(*shape, scale=0.7, bias=-0.1, shift=shift)
        xpart, x2part = self.slabs(x, nslab), self.slabs(x2, nslab2)
        x = torch.empty_like(x) if xpart is not None else x
        x2 = torch.empty_like(x2) if x2part is not None else x2
        y = torch.empty_like(x)
        X.bn_pair_fwd(x, x2, y, p["gamma"], p["beta"], p["rmean"], p["rvar"], p["nbt"], p["sm"], p["si"], p2["gamma"],
                      p2["beta"], p2["rmean"], p2["rvar"], p2["nbt"], p2["sm"], p2["si"], 1e-5, 0.1, xpart, nslab,
                      x2part, nslab2)
        self.save(tag, y=y, x=x, x2=x2, save_mean=p["sm"], save_invstd=p["si"], save_mean2=p2["sm"],
                  save_invstd2=p2["si"], running_mean=p["rmean"], running_var=p["rvar"], running_mean2=p2["rmean"],
                  running_var2=p2["rvar"], num_batches_tracked=p["nbt"], num_batches_tracked2=p2["nbt"])
        dy = self.rand(*shape)
        dypart = self.slabs(dy, nslab)
        dyadd = self.rand(*shape) if dypart is not None else None
        dy = torch.empty_like(dy) if dypart is not None else dy
        dx, dx2 = torch.empty_like(y), torch.empty_like(y)
        g = [torch.zeros(C, device=self.dev) for _ in range(4)]
        X.bn_pair_bwd(dy, y, x, x2, p["gamma"], p["sm"], p["si"], p2["gamma"], p2["sm"], p2["si"], dx, dx2, g[0], g[1],
                      g[2], g[3], dypart, nslab, dyadd)
        self.save(tag, dx=dx, dx2=dx2, dgamma=g[0], dbeta=g[1], dgamma2=g[2], dbeta2=g[3], dy=dy)

    def stem(self, tag, shape, ext=False):
        """BN -> ReLU -> max-pool forward, then the BN backward with the mask recomputed from x"""
        X, (N, C, H, W) = self.X, shape
        p = self.params(C)
        part = self.part(N, C, H * W)
        x = self.rand(*shape, scale=1.7, bias=0.4)
        y = torch.empty(N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1, device=self.dev)
        idx = torch.empty(y.shape, dtype=torch.uint8, device=self.dev)
        xst = self.image_stats(x, x, C).to(self.dev) if ext else None
        X.bn_relu_maxpool(x, y, idx, p["gamma"], p["beta"], p["rmean"], p["rvar"], p["nbt"], p["sm"], p["si"], part,
                          1e-5, 0.1, xst, N if ext else 0)
        self.save(tag, y=y, idx=idx, save_mean=p["sm"], save_invstd=p["si"], running_mean=p["rmean"],
                  running_var=p["rvar"], num_batches_tracked=p["nbt"])
        dz = self.rand(*shape)  # the pool backward's output
        dst = None
        if ext:
            sc = p["gamma"] * p["si"]
            mask = torch.addcmul((p["beta"] - p["sm"] * sc).view(1, C, 1, 1), x, sc.view(1, C, 1, 1)) > 0
            xh = (x - p["sm"].view(1, C, 1, 1)) * p["si"].view(1, C, 1, 1)
            dst = self.image_stats(dz * mask, xh, C).to(self.dev)
        dx = torch.empty_like(x)
        dg, db = torch.zeros(C, device=self.dev), torch.zeros(C, device=self.dev)
        X.bn_bwd(dz, None, x, p["gamma"], p["sm"], p["si"], dx, None, dg, db, part, True, True, None, 0, None, p["beta"],
                 dst, N if ext else 0)
        self.save(tag, dx=dx, dgamma=dg, dbeta=db)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", help="write every output as .npy into this directory")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from network_distributed_pytorch_amd.ops import ext

    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
    sw = Sweep(ext(), torch.device("cuda", 0), args.dump)

    def tag(kind, i, shape, opt):
        return f"{kind}{i:02d}_" + "x".join(map(str, shape)) + "".join(f"_{k}{int(v)}" for k, v in sorted(opt.items()))

    for i, (shape, opt) in enumerate(SHAPES):
        sw.bn(tag("bn", i, shape, opt), shape, **opt)
    for i, (shape, opt) in enumerate(PAIRS):
        sw.pair(tag("pair", i, shape, opt), shape, **opt)
    for i, (shape, opt) in enumerate(STEMS):
        sw.stem(tag("stem", i, shape, opt), shape, **opt)
    torch.cuda.synchronize()
    print(f"bn_route_sweep: {len(SHAPES)} shapes x {len(CASES)} cases, {len(PAIRS)} pairs, {len(STEMS)} stem tails, "
          f"{sw.count} outputs" + (f" dumped to {args.dump}" if args.dump else ""))


if __name__ == "__main__":
    main()
