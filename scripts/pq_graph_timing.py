"""Timing of the graph index over PQ codes (mi_pq_graph_build, mi_pq_graph_search_device): synthetic clustered rows
made on the device (CENTERS centres + noise), codebooks learned on them (M = 16 books of 256 codewords, ITERS iterations), rows
encoded, R = 32, 16 entry rows, 1024 queries drawn near stored rows.  Records
  - the build time of the graph (wall: the exhaustive N x N ADC search inside it included; training and encoding are not);
  - per ef in 16, 64, 256: queries/s of mi_pq_graph_search_device with k = 10 (HIP events on the stream, median of 5 after a
    warm-up call), the mean number of rows evaluated per query and recall@10 against mi_pq_search_device on the same index
    (what the graph loses against the exhaustive scan of the same codes, not what the codes lose against the raw rows);
  - mi_pq_search_device's own queries/s on the same index, same batch, same process;
  - index bytes per row: M code bytes + 4 R table bytes.
One GPU process:

    timeout -k 10 600 python scripts/pq_graph_timing.py [--rows N] [--dim D] [--out out.json]
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

ROWS, D, NQ, K, M, KS, R, NE, REPS, ITERS = 65536, 2048, 1024, 10, 16, 256, 32, 16, 5, 8
EFS = [16, 64, 256]


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
    ap.add_argument("--rows", type=int, default=ROWS)
    ap.add_argument("--dim", type=int, default=D)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, d = args.rows, args.dim
    centers = max(16, n // 16)          # (far more centres than codewords per book: rows of a cluster share a code, clusters do not)
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(7)
    centres = torch.randn((centers, d), device="cuda", generator=gen)
    rows = torch.empty((n, d), device="cuda")
    for r0 in range(0, n, 65536):                  # (block by block: no second array of the gallery's size)
        b = min(65536, n - r0)
        which = torch.randint(0, centers, (b,), device="cuda", generator=gen)
        rows[r0:r0 + b] = centres[which] + 0.3 * torch.randn((b, d), device="cuda", generator=gen)
    pick = torch.randint(0, n, (NQ,), device="cuda", generator=gen)
    q = (rows[pick] + 0.05 * torch.randn((NQ, d), device="cuda", generator=gen)).contiguous()
    torch.cuda.synchronize()
    t0 = time.time()
    books, _ = _lib.pq_train_device(rows.data_ptr(), n, d, M, KS, ITERS)
    pq = _lib.PQIndex.empty(books, n)
    pq.add_device(rows.data_ptr(), n)
    rec = {"rows": n, "d": d, "queries": NQ, "k": K, "M": M, "Ks": KS, "R": R, "entries": NE, "train_iters": ITERS,
           "train_and_encode_seconds": time.time() - t0, "index_bytes_per_row": M + 4 * R, "points": []}
    del rows
    t0 = time.time()
    gi = _lib.PQGraphIndex.build(pq, R=R, n_entry=NE)
    rec["build_seconds"] = time.time() - t0
    idx = torch.empty((NQ, K), dtype=torch.int64, device="cuda")
    exact = torch.empty((NQ, K), dtype=torch.int64, device="cuda")
    vis = torch.empty(NQ, dtype=torch.int32, device="cuda")
    ms = median_ms(lambda: pq.search_device(q.data_ptr(), NQ, K, exact.data_ptr(), stream=s))
    rec["pq_search_ms"] = ms
    rec["pq_search_queries_per_s"] = NQ / (ms * 1e-3)
    want = exact.cpu().numpy()
    for ef in EFS:
        ms = median_ms(lambda: gi.search_device(q.data_ptr(), NQ, K, idx.data_ptr(), ef=ef, visited_ptr=vis.data_ptr(), stream=s))
        got = idx.cpu().numpy()
        recall = float(np.mean([len(set(a) & set(b)) / K for a, b in zip(got.tolist(), want.tolist())]))
        mean_vis = float(vis.cpu().numpy().mean())
        rec["points"].append({"ef": ef, "ms": ms, "queries_per_s": NQ / (ms * 1e-3), "mean_visited": mean_vis, "recall_at_10": recall,
                              "bytes_read_per_query": mean_vis * (M + 4), "scan_bytes_per_query": n * M})
    rec["graph_hbm_bytes"] = gi.hbm_bytes
    rec["pq_hbm_bytes"] = pq.hbm_bytes
    gi.close()
    pq.close()
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
