"""dev helper: whole-matrix comparison of two tools/gemm_bench GB_DUMP runs (e.g. old vs new bf16 kernel); given two DIRECTORIES
written by `bench.py --dump-outputs`, compares their adj.npy / node.npy element by element instead and exits 1 unless both are
identical (a change that only leaves work undone must not move a single value)"""
import sys, glob, numpy as np
a_pref, b_pref = sys.argv[1], sys.argv[2]
import os
if os.path.isdir(a_pref) and os.path.isdir(b_pref):
    bad = 0
    for name in ("adj.npy", "node.npy"):
        a, b = np.load(os.path.join(a_pref, name)), np.load(os.path.join(b_pref, name))
        same = a.shape == b.shape and bool(np.array_equal(a, b))
        ndiff = -1 if a.shape != b.shape else int((a != b).sum())
        print("%s: %s  shape %s  differing elements %d  max|a| %.4g" % (name, "identical" if same else "DIFFERENT", a.shape, ndiff, float(np.abs(a).max())))
        bad += 0 if same else 1
    sys.exit(1 if bad else 0)
tol = float(sys.argv[3]) if len(sys.argv) > 3 else 1e-3
for fa in sorted(glob.glob(a_pref + "_*.bin")):
    fb = b_pref + fa[len(a_pref):]
    a, b = np.fromfile(fa, np.float32), np.fromfile(fb, np.float32)
    d = np.abs(a - b)
    print(fa.split("_")[-1], "n=%d max|a-b|=%.3g  count(>%g)=%d" % (a.size, d.max(), tol, int((d > tol).sum())))
