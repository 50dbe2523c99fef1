"""np.array_equal of every array of two bench.py --dump-outputs directories."""
import os, sys
import numpy as np
a, b = sys.argv[1], sys.argv[2]
names = sorted(set(os.listdir(a)) | set(os.listdir(b)))
bad = 0
for n in names:
    if not n.endswith(".npy"):
        continue
    pa, pb = os.path.join(a, n), os.path.join(b, n)
    if not (os.path.exists(pa) and os.path.exists(pb)):
        print(f"{n}: MISSING in one"); bad += 1; continue
    x, y = np.load(pa), np.load(pb)
    eq = x.shape == y.shape and np.array_equal(x, y)
    print(f"{n}: shape {x.shape} dtype {x.dtype} array_equal {eq}")
    bad += 0 if eq else 1
print(f"{a} vs {b}: {'BITWISE EQUAL' if bad == 0 else str(bad) + ' ARRAYS DIFFER'}")
sys.exit(1 if bad else 0)
