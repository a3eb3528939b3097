"""Digest of everything ops._ConvPlan decides, built on the CPU: one line per layer geometry (key, routes, SHA-256 over vars(plan))
and a total.  A change to the plan builder that is meant to keep behaviour is checked by running this at both commits against
ONE built library and comparing the two files: equal digests = equal attribute names, geom arrays, tables, split counts, routes.

    python tools/conv_plan_digest.py --out head.txt [--keys profiles/conv_plan_keys.json]
    C2M_AMD_LIB=$PWD/c2m_amd/lib/libc2m_hip.so python tools/conv_plan_digest.py --root ../parent --out parent.txt [--keys ...]
    python tools/conv_plan_digest.py --compare parent.txt head.txt            # prints the differing cases, exit 1 if any

Cases: every row of tests/conv_route_cases.TABLE under its knobs, conv_route_cases.sweep() under the default knobs, and optionally
a JSON list of ops._geom_cache keys without the device index ([xs, ws, stride, pad, reflect, bf16, dgrad_rows], --keys).  --root
names the tree whose c2m_amd and tests/conv_route_cases.py are imported (default: this file's); only ops._ConvPlan, ops.WG and
TABLE / knobs / sweep are used, so the tool runs as it is on an older tree that has the cases file copied in."""
import argparse
import hashlib
import json
import os
import sys
import time


def _feed(h, v):
    """Hash a plan value: arrays and tensors by dtype, shape and bytes, dicts by sorted key, sequences in order, scalars by repr."""
    import numpy as np
    import torch
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().contiguous()
        h.update(f"T{v.dtype}{tuple(v.shape)}".encode())
        h.update(v.view(torch.uint8).numpy().tobytes() if v.numel() else b"")
    elif isinstance(v, np.ndarray):
        h.update(f"A{v.dtype}{v.shape}".encode())
        h.update(np.ascontiguousarray(v).tobytes())
    elif isinstance(v, dict):
        h.update(f"D{len(v)}".encode())
        for k in sorted(v):
            h.update(f"K{k!r}".encode())
            _feed(h, v[k])
    elif isinstance(v, (list, tuple)):
        h.update(f"{type(v).__name__[0].upper()}{len(v)}".encode())
        for a in v:
            _feed(h, a)
    else:
        h.update(f"S{v!r};".encode())


def plan_digest(ops, case):
    """(routes, digest) of one case; a case the builder refuses is hashed by its exception type."""
    import torch
    xs, ws, stride, pad, reflect, bf16, rows = case
    try:
        pl = ops._ConvPlan(xs, ws, stride, pad, reflect, torch.device("cpu"), bf16, rows)
    except Exception as e:          # noqa: BLE001 (any refusal is part of the behaviour)
        return "raised", hashlib.sha256(type(e).__name__.encode()).hexdigest()
    attrs = dict(vars(pl))
    if attrs.get("wino3d_pairs"):           # geom[PTAB] is the address of wino_pair_tab (hashed itself): differs per process
        g = attrs["wino_dgrad_geom"] = attrs["wino_dgrad_geom"].copy()
        g[ops.WG.PTAB] = 0
    h = hashlib.sha256()
    _feed(h, attrs)
    return "/".join((pl.fwd_route, pl.dgrad_route, pl.wgrad_route)), h.hexdigest()


def _tup(v):
    return tuple(_tup(a) for a in v) if isinstance(v, list) else v


def digest(root, keys_file, out):
    sys.path[:0] = [root, os.path.join(root, "tests")]
    from c2m_amd import ops
    from conv_route_cases import TABLE, knobs, sweep
    lines, triples = [], set()

    def run(section, cases):          # cases: (case, knob settings)
        t0, n = time.perf_counter(), 0
        for n, (case, kn) in enumerate(cases, 1):
            with knobs(kn):
                routes, d = plan_digest(ops, case)
            triples.add(routes)
            lines.append(f"{section}[{n - 1}] {case!r} {routes} {d}")
        print(f"{section}: {n} cases, {time.perf_counter() - t0:.2f} s")

    run("table", ((row[:7], row[7]) for row in TABLE))
    run("sweep", ((case, {}) for case in sweep()))
    if keys_file:
        with open(keys_file) as f:
            run("keys", [(_tup(k), {}) for k in json.load(f)])
    total = hashlib.sha256("\n".join(lines).encode()).hexdigest()
    refused = sum(" raised " in ln for ln in lines)
    lines.append(f"total {len(lines)} cases, {refused} refused, {len(triples - {'raised'})} route triples, digest {total}")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1])


def compare(a, b):
    def read(path):
        with open(path) as f:
            return {ln.rsplit(" ", 2)[0]: ln.rsplit(" ", 2)[1:] for ln in f.read().splitlines() if not ln.startswith("total ")}
    A, B = read(a), read(b)
    diff = [k for k in list(A) + [k for k in B if k not in A] if A.get(k) != B.get(k)]
    for k in diff:
        print(k, A.get(k), "->", B.get(k))
    print(f"{len(diff)} differing cases of {len(A)} / {len(B)}")
    return 1 if diff else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--keys", help="JSON list of _geom_cache keys (without the device index)")
    ap.add_argument("--out", default="conv_plan_digest.txt")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    sys.exit(compare(*args.compare) if args.compare else digest(os.path.abspath(args.root), args.keys, args.out))
