#!/usr/bin/env python3
"""tests/soak/layout_soak.py [first_seed] [count] [plain|pipe|posed|fused] [oracle_threads] -- the seeded batch layouts of
tests/layouts.py beyond the seeds the suite pins, through the checks of tests/test_gpu_layouts.py: plain calls against the
oracle (guard and input checks included), pipelined calls and the fused low-pass against the plain call, posed calls
against the plain call and an oracle per pose.  fused counts `count` fusable layouts from first_seed on (the others are
passed over).  Development soak: prints every mismatch, exits 1 if there was one."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import t360_oracle as O  # noqa: E402
from tests import layouts as LY  # noqa: E402
from tests import test_gpu_layouts as G  # noqa: E402
from transform360_amd import handler as T  # noqa: E402

first = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
count = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
mode = sys.argv[3] if len(sys.argv) > 3 else "plain"
LY.ORACLE_THREADS = int(sys.argv[4]) if len(sys.argv) > 4 else 4
assert mode in ("plain", "pipe", "posed", "fused"), mode
O.build(ref=False)
bad = done = fused_ran = refused = 0
kernels = set()
t0 = time.time()
seed = first
while done < count:
    L = LY.draw_layout(seed)
    seed += 1
    if mode == "fused" and not L.fusable():
        continue
    done += 1
    try:
        if mode == "plain":
            k = G.check_plain(T, O, L)
            kernels.add(k.split("<")[0])
        elif mode == "pipe":
            k = G.check_pipelined(T, O, L)
        elif mode == "posed":
            k = G.check_posed(T, O, L)
        else:
            k = G.check_fused(T, O, L)
            fused_ran += "remap_fused_kernel" in k
        refused += k == "refused"
    except AssertionError as e:
        bad += 1
        print("seed %d: %s" % (L.seed, str(e)[:1500]), flush=True)
extra = " (fused kernel ran in %d)" % fused_ran if mode == "fused" else " (kernels %s)" % sorted(kernels) if kernels else ""
print("%s: %d layouts, seeds %d..%d: %d mismatches, %d maps refused by both the oracle and the library%s, %.0f s" % (
    mode, done, first, seed - 1, bad, refused, extra, time.time() - t0))
sys.exit(1 if bad else 0)
