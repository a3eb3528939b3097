"""Compare two `bench.py --dump-outputs DIR` directories (the tables of profiles/*_bench_outputs_vs_parent.txt):
    python tools/compare_bench_outputs.py <parent dir> <change dir>
Per file the max abs difference over the parent's max abs value; grad_norms.npy as the relative difference of each norm.  Exit
status 1 when a loss differs by more than 2e-4, an output by more than 1e-2 of its scale, or a gradient norm by more than 2e-3
(gradients whose norm is below 1e-4 of the median norm are rounding residue of analytically zero gradients: printed, not gated)."""
import os
import sys

import numpy as np

a_dir, b_dir = sys.argv[1], sys.argv[2]
names = sorted(set(os.listdir(a_dir)) | set(os.listdir(b_dir)))
bad, worst = [], 0.0
for n in names:
    pa, pb = os.path.join(a_dir, n), os.path.join(b_dir, n)
    if not (os.path.exists(pa) and os.path.exists(pb)):
        print(f"{n}: only in {'parent' if os.path.exists(pa) else 'change'}")
        bad.append(n)
        continue
    a, b = np.load(pa).astype(np.float64), np.load(pb).astype(np.float64)
    if a.shape != b.shape:
        print(f"{n}: shape {a.shape} vs {b.shape}")
        bad.append(n)
        continue
    if n == "grad_norms.npy":
        rel = np.abs(a - b) / np.maximum(np.abs(a), 1e-30)
        print(f"{n}: {a.size} gradients; relative difference of the norms worst {rel.max():.2e} median {np.median(rel):.2e}")
        # A gradient that is analytically zero (a conv bias in front of a norm layer) is the rounding residue of its kernels:
        # any change of a summation order upstream replaces it.  Those are listed apart and gated by their size, not their ratio.
        floor = 1e-4 * float(np.median(a))
        residue = np.maximum(a, b) < floor
        if residue.any():
            real = ~residue
            print(f"{n}: {int(real.sum())} gradients with a norm above {floor:.1e} (1e-4 of the median norm): worst "
                  f"{rel[real].max():.2e} median {np.median(rel[real]):.2e}; smallest of them {a[real].min():.2e}")
            print(f"{n}: {int(residue.sum())} gradients below it (largest norm {max(a[residue].max(), b[residue].max()):.2e}, "
                  f"{int((a[residue] == 0).sum())} exactly zero): worst {rel[residue].max():.2e}")
            rel = rel[real]
        if not rel.max() <= 2e-3:
            bad.append(n)
        continue
    scale = max(float(np.abs(a).max()) if a.size else 0.0, 1e-30)
    err = float(np.abs(a - b).max()) / scale if a.size else 0.0
    vals = f"  values {a.reshape(-1)[:1]} {b.reshape(-1)[:1]}" if n.startswith("loss") else ""
    print(f"{n}: max abs err / scale {err:.2e}{vals}")
    if n != "grad_sample.npy":
        worst = max(worst, err)
    if not err <= (2e-4 if n.startswith("loss") else 1e-2):
        bad.append(n)
print(f"worst output / loss error relative to scale: {worst:.2e}")
if bad:
    print("OUTSIDE THE GATES:", ", ".join(bad))
    sys.exit(1)
