"""Timing of the random-projection forest (mi_forest_build, mi_forest_search_device) at a shape the caller names:
synthetic clustered rows made on the device (rows / 16 centres + noise) in a squared-L2 gallery, queries drawn near stored rows.
Records
  - the build time of the forest (wall; the projection of every row onto every direction included);
  - queries/s of mi_forest_search_device with k = K (HIP events on the stream, median of 5 after a warm-up call);
  - recall@K against mi_knn_search_l2_device on the same gallery, and that search's own queries/s in the same process;
  - the forest's shape: depth, leaf_max, candidate slots per query, table bytes per row.
Nothing here is asserted: the record is for DESIGN 5.17, with the shape and the date.  One GPU process:

    timeout -k 10 600 python scripts/forest_timing.py [--rows N] [--dim D] [--trees T] [--depth L] [--queries Q] [--k K] [--out out.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import isehr_amd  # noqa: E402,F401
from isehr_amd import _lib  # noqa: E402

REPS = 5


def median_ms(fn, reps=REPS):
    fn()                                           # warm-up (grows the handle's buffers)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--depth", type=int, default=None)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, d, nq, k = args.rows, args.dim, args.queries, args.k
    centers = max(16, n // 16)
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(7)
    centres = torch.randn((centers, d), device="cuda", generator=gen)
    rows = torch.empty((n, d), device="cuda")
    for r0 in range(0, n, 65536):                  # (block by block: no second array of the gallery's size)
        b = min(65536, n - r0)
        which = torch.randint(0, centers, (b,), device="cuda", generator=gen)
        rows[r0:r0 + b] = centres[which] + 0.3 * torch.randn((b, d), device="cuda", generator=gen)
    pick = torch.randint(0, n, (nq,), device="cuda", generator=gen)
    q = (rows[pick] + 0.05 * torch.randn((nq, d), device="cuda", generator=gen)).contiguous()
    torch.cuda.synchronize()
    g = _lib.Gallery.l2_from_device_ptr(rows.data_ptr(), n, d)
    del rows
    t0 = time.time()
    f = _lib.ForestIndex.build(g, n_trees=args.trees, depth=args.depth)
    rec = {"rows": n, "d": d, "queries": nq, "k": k, "trees": f.n_trees, "depth": f.depth, "leaf_max": f.leaf_max,
           "candidate_slots": f.n_trees * f.leaf_max, "build_seconds": time.time() - t0,
           "table_bytes_per_row": 4 * f.n_trees + 8.0 * f.n_trees * ((1 << f.depth) - 1) / n}
    idx = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    exact = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    ms = median_ms(lambda: g.search_l2_device(q.data_ptr(), nq, k, exact.data_ptr(), stream=s))
    rec["exact_search_ms"] = ms
    rec["exact_queries_per_s"] = nq / (ms * 1e-3)
    ms = median_ms(lambda: f.search_device(q.data_ptr(), nq, k, idx.data_ptr(), stream=s))
    rec["forest_search_ms"] = ms
    rec["forest_queries_per_s"] = nq / (ms * 1e-3)
    got, want = idx.cpu().numpy(), exact.cpu().numpy()
    rec["recall_at_k"] = float(np.mean([len(set(a) & set(b)) / k for a, b in zip(got.tolist(), want.tolist())]))
    f.close()
    g.close()
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
