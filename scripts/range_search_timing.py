"""Timing of the exact range search on the full-size gallery: 1 005 994 x 2048 rows synthesised on the device
(synth_fill_device), 1024 queries, thresholds taken from top-K runs so that the mean hit count is about 10, 100 and 1000
per query; every figure next to Gallery.search at K = 100 on the same queries.  A fourth threshold, extrapolated one doubling
below the 2048-th score, gives several thousand hits per query: lists longer than one sorted run of the ordering stage
(csrc/csr_order.hip), so its merge passes run ("range_merge"; the mean and the largest hit count are recorded).  Then
near_duplicate_pairs over a 1 M-row gallery with planted exact duplicates.  Every shape is run once before it is timed; every
figure is the wall time of synchronous host calls (the library synchronises the device before it returns).  One GPU process:

    timeout -k 10 900 python scripts/range_search_timing.py [--no-pairs] [out.json]

Wall time is dominated by scoring.  For the kernel time of the ordering stage alone, run the merge case by itself (one warm-up
and one call, no near_duplicate_pairs) under the profiler, in a process of its own, and read csr_sort_kernel, csr_merge_kernel
and csr_write_kernel out of the kernel statistics:

    timeout -k 10 900 rocprofv3 --kernel-trace --stats -d DIR -- python scripts/range_search_timing.py --merge-only
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


def merge_case(g, q, out, reps):
    """a threshold with several thousand hits per query: s(4096) ~ 2 s(2048) - s(1024), the scores falling about linearly in log k"""
    _, sc, _ = g.search(q, 2048)
    tau = float(np.median(2.0 * sc[:, 2047] - sc[:, 1023]))
    t, (lims, _, _, _) = timed(lambda: g.range_search(q, tau), reps)
    hits = np.diff(lims)
    out["range_merge"] = {"tau": tau, "mean_hits": float(hits.mean()), "max_hits": int(hits.max()), "s": t}
    print("merge case: hits mean %.1f, max %d per query: %.2f ms per %d-query batch" % (hits.mean(), hits.max(), t * 1e3, NQ), flush=True)


def main():
    out = {"rows": N, "dim": D, "queries": NQ}
    g = gallery(1234)
    q = synth_rows(4321, 0, NQ, D)
    if "--merge-only" in sys.argv:
        merge_case(g, q, out, 1)
        g.close()
        print(json.dumps(out))
        return
    t_knn, _ = timed(lambda: g.search(q, 100))
    out["search_k100_s"] = t_knn
    for h in (10, 100, 1000):
        _, sc, _ = g.search(q, h)
        tau = float(np.median(sc[:, h - 1]))
        t, (lims, _, _, _) = timed(lambda: g.range_search(q, tau))
        out["range_%d" % h] = {"tau": tau, "mean_hits": float(lims[-1]) / NQ, "s": t, "vs_search_k100": t / t_knn}
        print("hits ~%4d/query (mean %.1f): %.2f ms per %d-query batch; search K=100 %.2f ms (x%.2f)"
              % (h, lims[-1] / NQ, t * 1e3, NQ, t_knn * 1e3, t / t_knn), flush=True)
    merge_case(g, q, out, REPS)
    g.close()
    if "--no-pairs" not in sys.argv:
        gd = gallery(999, planted=5000)
        t0 = time.perf_counter()
        i, j, _ = near_duplicate_pairs(gd, 0.999)
        t_pairs = time.perf_counter() - t0
        out["near_duplicate_pairs"] = {"planted": 5000, "min_score": 0.999, "pairs": int(len(i)), "s": t_pairs}
        print("near_duplicate_pairs: %d rows, %d pairs at >= 0.999, %.2f s" % (N, len(i), t_pairs), flush=True)
        gd.close()
    print(json.dumps(out))
    files = [a for a in sys.argv[1:] if not a.startswith("--")]
    if files:
        with open(files[0], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
