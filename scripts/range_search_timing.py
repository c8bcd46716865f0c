"""Timing of the exact range search on the full-size gallery: 1 005 994 x 2048 rows synthesised on the device
(synth_fill_device), 1024 queries, thresholds taken from top-K runs so that the mean hit count is about 10, 100 and 1000
per query; every figure next to Gallery.search at K = 100 on the same queries.  Then near_duplicate_pairs over a 1 M-row
gallery with planted exact duplicates.  Every shape is run once before it is timed; every figure is the wall time of
synchronous host calls (the library synchronises the device before it returns).  One GPU process:

    timeout -k 10 900 python scripts/range_search_timing.py [out.json]
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
from isehr_amd.dedup import near_duplicate_pairs  # noqa: E402
from isehr_amd.synth import synth_rows  # noqa: E402

N, D, NQ, REPS = 1005994, 2048, 1024, 5


def timed(fn, reps=REPS):
    fn()                                           # warm-up of this shape
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def gallery(seed, planted=0):
    s = torch.cuda.current_stream().cuda_stream
    raw = torch.empty((N, D), dtype=torch.float32, device="cuda")
    _lib.synth_fill_device(raw.data_ptr(), seed, 0, N, D, s)
    if planted:
        g = torch.Generator(device="cpu").manual_seed(seed)
        perm = torch.randperm(N, generator=g)
        src, dst = perm[:planted].cuda(), perm[planted:2 * planted].cuda()
        raw[dst] = raw[src]
    torch.cuda.synchronize()
    g = _lib.Gallery.from_device_ptr(raw.data_ptr(), N, D)
    del raw
    torch.cuda.empty_cache()
    return g


def main():
    out = {"rows": N, "dim": D, "queries": NQ}
    g = gallery(1234)
    q = synth_rows(4321, 0, NQ, D)
    t_knn, _ = timed(lambda: g.search(q, 100))
    out["search_k100_s"] = t_knn
    for h in (10, 100, 1000):
        _, sc, _ = g.search(q, h)
        tau = float(np.median(sc[:, h - 1]))
        t, (lims, _, _, _) = timed(lambda: g.range_search(q, tau))
        out["range_%d" % h] = {"tau": tau, "mean_hits": float(lims[-1]) / NQ, "s": t, "vs_search_k100": t / t_knn}
        print("hits ~%4d/query (mean %.1f): %.2f ms per %d-query batch; search K=100 %.2f ms (x%.2f)"
              % (h, lims[-1] / NQ, t * 1e3, NQ, t_knn * 1e3, t / t_knn), flush=True)
    g.close()
    gd = gallery(999, planted=5000)
    t0 = time.perf_counter()
    i, j, _ = near_duplicate_pairs(gd, 0.999)
    t_pairs = time.perf_counter() - t0
    out["near_duplicate_pairs"] = {"planted": 5000, "min_score": 0.999, "pairs": int(len(i)), "s": t_pairs}
    print("near_duplicate_pairs: %d rows, %d pairs at >= 0.999, %.2f s" % (N, len(i), t_pairs), flush=True)
    gd.close()
    print(json.dumps(out))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
