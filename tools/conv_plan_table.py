"""The direct-conv dispatch plan as the bindings report it, for every shape class, a set of near
misses, a ladder of batches and every runtime switch that the plan depends on.

    python tools/conv_plan_table.py > tests/golden/conv_plan_table.json

writes the fixture that tests/test_conv_plan_cpu.py compares a build against (host code only, no
GPU).  Regenerate it only from a build whose plan is known good: the fixture is the record of what
the dispatch chose before a change to csrc/conv.hip.
"""
from __future__ import annotations

import json
import os
import sys

# geometry = [C, H, W, Co, KH, KW, stride, pad]
GEOMS = [
    [64, 8, 8, 64, 3, 3, 1, 1], [128, 8, 8, 64, 3, 3, 1, 1],          # 3x3 s1 on 8x8
    [128, 4, 4, 128, 3, 3, 1, 1], [64, 4, 4, 192, 3, 3, 1, 1],        # 3x3 s1 on 4x4
    [64, 8, 8, 128, 3, 3, 2, 1], [128, 8, 8, 128, 3, 3, 2, 1],        # 3x3 s2 on 8x8
    [3, 32, 32, 64, 7, 7, 2, 3],                                      # stem
    [64, 8, 8, 128, 1, 1, 2, 0], [256, 8, 8, 512, 1, 1, 2, 0],        # 1x1 s2 on 8x8
    [128, 4, 4, 256, 1, 1, 2, 0], [512, 4, 4, 1024, 1, 1, 2, 0],      # 1x1 s2 on 4x4
    # near misses: no direct kernel (class -1)
    [64, 16, 16, 64, 3, 3, 1, 1],                                     # 3x3 on a 16x16 map
    [48, 8, 8, 64, 3, 3, 1, 1],                                       # C = 48
    [64, 8, 8, 64, 3, 3, 1, 0],                                       # pad 0 on a 3x3
    [4, 32, 32, 64, 7, 7, 2, 3],                                      # stem with C = 4
    [64, 8, 8, 128, 1, 1, 1, 0],                                      # 1x1 with stride 1
]
BATCHES = [1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512, 1024]
WINO = [1, 0]            # wino_set_enabled
PSPLIT = [0, 1, 2, 4]    # conv_set_stem_psplit (0 = by batch)
COLUMNS = ["geom", "batch", "wino", "psplit", "class", "fwd_imgs", "wgrad_imgs", "dgrad_direct", "fwd_ksplit",
           "dgrad_ksplit", "fwd_stats_slices", "dgrad_stats_slices", "fwd_wino", "dgrad_wino"]


def rows(X):
    """One list per (geometry index, batch, wino, psplit); leaves the switches at their defaults."""
    out = []
    try:
        for wino in WINO:
            X.wino_set_enabled(bool(wino))
            for ps in PSPLIT:
                X.conv_set_stem_psplit(ps)
                for gi, geom in enumerate(GEOMS):
                    for B in BATCHES:
                        plan = [int(v) for v in X.conv_plan(geom, B)]
                        out.append([gi, B, wino, ps] + plan + [
                            int(X.conv_stats_slices(geom, B)), int(X.conv_dgrad_stats_slices(geom, B)),
                            int(X.conv_wino(geom, B, False)), int(X.conv_wino(geom, B, True))])
    finally:
        X.wino_set_enabled(True)
        X.conv_set_stem_psplit(0)
    return out


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from network_distributed_pytorch_amd.ops import ext

    body = ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows(ext()))
    print('{"columns":%s,\n"geoms":%s,\n"rows":[\n%s\n]}' % (json.dumps(COLUMNS), json.dumps(GEOMS), body))


if __name__ == "__main__":
    main()
