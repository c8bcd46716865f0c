"""Timing of the graph index (mi_graph_build, mi_graph_search_device) at full size: 1 005 994 x 2048 synthetic
clustered rows made on the device (CENTERS centres + noise), squared-L2 gallery, R = 32, 16 entry rows, 1024 queries drawn near
stored rows.  Records
  - the build time (wall, the exact N x N search inside it included);
  - per ef in 16, 64, 256: queries/s of mi_graph_search_device with k = 10 (HIP events on the stream, median of 5 after a
    warm-up call), the mean number of rows evaluated per query, recall@10 against mi_knn_search_l2_device on the same gallery,
    and the bytes per second the search gathers (rows evaluated x 4 x dp) as a fraction of the 6.0 TB/s a gather of whole rows
    reaches from HBM on this chip;
  - the exact search's queries/s at the same batch size.
One GPU process:

    timeout -k 10 1100 python scripts/graph_timing.py [out.json] [rows]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import isehr_amd  # noqa: E402,F401
from isehr_amd import _lib  # noqa: E402

N, D, NQ, K, R, NE, REPS, CENTERS = 1005994, 2048, 1024, 10, 32, 16, 5, 4096
EFS = [16, 64, 256]
HBM_GATHER_BYTES_PER_S = 6.0e12


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
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    n = int(sys.argv[2]) if len(sys.argv) > 2 else N
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(7)
    centres = torch.randn((CENTERS, D), device="cuda", generator=gen)
    rows = torch.empty((n, D), device="cuda")
    for r0 in range(0, n, 65536):                  # (block by block: no second array of the gallery's size)
        b = min(65536, n - r0)
        which = torch.randint(0, CENTERS, (b,), device="cuda", generator=gen)
        rows[r0:r0 + b] = centres[which] + 0.3 * torch.randn((b, D), device="cuda", generator=gen)
    pick = torch.randint(0, n, (NQ,), device="cuda", generator=gen)
    q = (rows[pick] + 0.05 * torch.randn((NQ, D), device="cuda", generator=gen)).contiguous()
    torch.cuda.synchronize()
    g = _lib.Gallery.l2_from_device_ptr(rows.data_ptr(), n, D)
    del rows
    rec = {"rows": n, "d": D, "queries": NQ, "k": K, "R": R, "entries": NE, "points": []}
    t0 = time.time()
    gi = _lib.GraphIndex.build(g, R=R, n_entry=NE)
    rec["build_seconds"] = time.time() - t0
    idx = torch.empty((NQ, K), dtype=torch.int64, device="cuda")
    exact = torch.empty((NQ, K), dtype=torch.int64, device="cuda")
    vis = torch.empty(NQ, dtype=torch.int32, device="cuda")
    ms = median_ms(lambda: g.search_l2_device(q.data_ptr(), NQ, K, exact.data_ptr(), stream=s))
    rec["exact_queries_per_s"] = NQ / (ms * 1e-3)
    want = exact.cpu().numpy()
    dp = (D + 3 + 63) // 64 * 64                   # (an L2 gallery stores three hidden columns behind the caller's)
    for ef in EFS:
        ms = median_ms(lambda: gi.search_device(q.data_ptr(), NQ, K, idx.data_ptr(), ef=ef, visited_ptr=vis.data_ptr(), stream=s))
        got = idx.cpu().numpy()
        recall = float(np.mean([len(set(a) & set(b)) / K for a, b in zip(got.tolist(), want.tolist())]))
        mean_vis = float(vis.cpu().numpy().mean())
        rate = mean_vis * NQ * 4 * dp / (ms * 1e-3)
        rec["points"].append({"ef": ef, "ms": ms, "queries_per_s": NQ / (ms * 1e-3), "mean_visited": mean_vis, "recall_at_10": recall,
                              "gather_bytes_per_s": rate, "fraction_of_hbm_gather_rate": rate / HBM_GATHER_BYTES_PER_S})
    gi.close()
    g.close()
    line = json.dumps(rec)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
