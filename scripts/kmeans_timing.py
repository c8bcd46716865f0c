"""Timing of k-means over whole rows (mi_kmeans_train) beside mi_pqw_train with one book on the same rows in the same
process: 1 005 994 x 2048 clustered float32 rows made on the device (4096 centres + noise), k = 256 / 1024 / 8192, five iterations
from the default initial rows.  Per iteration it records the device times mi_pq_train_timing reports (assignment with its move
count, update) for both calls and the rows the matrix kernel left to the direct form, and whether both calls returned the same
bytes.  Nothing here is asserted: the record is for DESIGN 5.14g, with the shape and the date.

The parent touches no GPU: every case is a child process of its own under `timeout`, one after the other, and the first case that
fails or runs out of time ends the run.

    python scripts/kmeans_timing.py [--rows N] [--dim D] [--ks 256,1024,8192] [--iters 5] [--limit 900] [--out out.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_case(n, d, k, iters):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import isehr_amd  # noqa: F401
    from isehr_amd import _lib

    centers = 4096
    gen = torch.Generator(device="cuda").manual_seed(7)
    centres = 3 * torch.randn((centers, d), device="cuda", generator=gen)
    rows = torch.empty((n, d), device="cuda")
    for r0 in range(0, n, 65536):                  # (block by block: no second array of the rows' size)
        b = min(65536, n - r0)
        which = torch.randint(0, centers, (b,), device="cuda", generator=gen)
        rows[r0:r0 + b] = centres[which] + 0.5 * torch.randn((b, d), device="cuda", generator=gen)
    torch.cuda.synchronize()
    rec = {"rows": n, "d": d, "k": k, "iters": iters}
    t0 = time.time()
    c_m, moved_m, flagged = _lib.kmeans_train_device(rows.data_ptr(), n, d, k, iters, return_flagged=True)
    rec["matrix_seconds"] = time.time() - t0
    a, u = _lib.pq_train_timing()
    rec.update({"matrix_assign_ms": a.tolist(), "matrix_update_ms": u.tolist(), "flagged": flagged.tolist(), "moved": moved_m.tolist()})
    t0 = time.time()
    c_v, moved_v = _lib.pqw_train_device(rows.data_ptr(), n, d, 1, k, iters)
    rec["vector_seconds"] = time.time() - t0
    a, u = _lib.pq_train_timing()
    rec.update({"vector_assign_ms": a.tolist(), "vector_update_ms": u.tolist()})
    rec["same_bytes"] = bool(np.array_equal(c_m.view(np.uint32), c_v[0].view(np.uint32)) and np.array_equal(moved_m, moved_v))
    rec["assign_ratio_vector_over_matrix"] = float(np.median(rec["vector_assign_ms"]) / np.median(rec["matrix_assign_ms"]))
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1005994)
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--ks", default="256,1024,8192")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--limit", type=int, default=900, help="seconds a case may take")
    ap.add_argument("--case", type=int, default=0, help="(internal) run this k in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_timing.json"))
    args = ap.parse_args()
    if args.case:
        return run_case(args.rows, args.dim, args.case, args.iters)
    rec = {"date": time.strftime("%Y-%m-%d"), "cases": []}
    for k in [int(v) for v in args.ks.split(",")]:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--rows", str(args.rows), "--dim",
               str(args.dim), "--iters", str(args.iters), "--case", str(k)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            rec["stopped"] = {"k": k, "returncode": r.returncode, "stderr": r.stderr[-2000:]}
            print(json.dumps(rec["stopped"]), flush=True)
            break                                  # nothing more is started after a case that failed or hung
        rec["cases"].append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(rec["cases"][-1]), flush=True)
    line = json.dumps(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 1 if "stopped" in rec else 0


if __name__ == "__main__":
    sys.exit(main())
