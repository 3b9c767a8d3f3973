#!/usr/bin/env python
"""Bit-equality report of two ``bench.py --dump-outputs`` directories (same arguments = same seeded inputs).

    python tools/compare_dumps.py DIR_A DIR_B          exit status 1 if any array differs in a single bit
"""
import glob, os, sys
import numpy as np

a_dir, b_dir = sys.argv[1:3]
names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(a_dir, "*.npy")))
assert names and names == sorted(os.path.basename(p) for p in glob.glob(os.path.join(b_dir, "*.npy"))), "different sets of arrays"
bad = 0
for n in names:
    a, b = np.load(os.path.join(a_dir, n)), np.load(os.path.join(b_dir, n))
    same = a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    bad += not same
    print(f"{n:32s} {str(a.dtype):8s} {str(a.shape):24s} {'bit-identical' if same else 'DIFFERENT'}")
print(f"{len(names) - bad} of {len(names)} arrays bit-identical")
sys.exit(1 if bad else 0)
