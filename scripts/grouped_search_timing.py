"""Timing of the exact grouped top-K search on the full-size gallery: 1 005 994 x 2048 rows synthesised on the
device (synth_fill_device), K = 100, nq in {1, 70, 1024}, groups of 1, 8 and 64 consecutive rows, and one adversarial labelling
in which the 4096 top-scoring rows of every query share one label of that query's own (the over-fetch certifies nothing, the
dense fallback answers).  Per point: the over-fetch factor f ("group_overfetch") in {2, 4, 8} on the automatic path, and the
forced fallback ("group_path" 1) for nq <= 70, next to the unfiltered Gallery.search on the same queries.  Every figure is the
median of 5 wall times of synchronous host calls after a warm-up call.  One GPU process:

    timeout -k 10 1200 python scripts/grouped_search_timing.py profiles/grouped_search_timing.json

The default of "group_overfetch" is to be chosen from the table this prints; it goes into DESIGN.md 5.10b.
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
from isehr_amd.synth import synth_rows  # noqa: E402

N, D, K, REPS = 1005994, 2048, 100, 5
NQS = (1, 70, 1024)
SIZES = (1, 8, 64)
FACTORS = (2, 4, 8)
GIANT = 4096
FALLBACK_MAX_NQ = 70          # the forced fallback scores every row in float64: 1024 queries of it are not a case anyone runs


def median_time(fn, reps=REPS):
    fn()                                           # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def gallery(seed):
    s = torch.cuda.current_stream().cuda_stream
    raw = torch.empty((N, D), dtype=torch.float32, device="cuda")
    _lib.synth_fill_device(raw.data_ptr(), seed, 0, N, D, s)
    torch.cuda.synchronize()
    g = _lib.Gallery.from_device_ptr(raw.data_ptr(), N, D)
    del raw
    torch.cuda.empty_cache()
    return g


def point(g, q, pt):
    for f in FACTORS:
        _lib.set_global_option("group_overfetch", f)
        pt["auto_f%d_ms" % f] = median_time(lambda: g.search_grouped(q, K)) * 1e3
        pt["auto_f%d_info" % f] = g.search_grouped(q, K, return_info=True)[3]
    _lib.set_global_option("group_overfetch", 0)
    if len(q) <= FALLBACK_MAX_NQ:
        g.set_option("group_path", 1)
        pt["fallback_ms"] = median_time(lambda: g.search_grouped(q, K)) * 1e3
        g.set_option("group_path", 0)
    for f in FACTORS:
        pt["auto_f%d_vs_unfiltered" % f] = pt["auto_f%d_ms" % f] / pt["unfiltered_ms"]
    print(json.dumps(pt), flush=True)
    return pt


def main():
    g = gallery(1234)
    out = {"rows": N, "dim": D, "k": K, "group_dense_bytes": _lib.get_global_option("group_dense_bytes"), "points": []}
    for nq in NQS:
        q = synth_rows(4321, 0, nq, D)
        t_plain = median_time(lambda: g.search(q, K)) * 1e3
        for size in SIZES:
            g.set_groups((np.arange(N) // size).astype(np.int32) if size > 1 else np.full(N, -1, np.int32))
            out["points"].append(point(g, q, {"nq": nq, "case": "groups of %d" % size, "unfiltered_ms": t_plain}))
        if nq <= FALLBACK_MAX_NQ:
            labels = np.full(N, -1, np.int32)
            top = g.rank_prefix(q, GIANT)[0]
            for i in range(nq - 1, -1, -1):                      # a row in two queries' tops keeps the lower query's label
                labels[top[i] - g.row_offset] = i
            g.set_groups(labels)
            out["points"].append(point(g, q, {"nq": nq, "case": "own group of %d top rows" % GIANT, "unfiltered_ms": t_plain}))
    g.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
