"""Timing of the exact filtered top-K search on the full-size gallery: 1 005 994 x 2048 rows synthesised on the
device (synth_fill_device), K = 100, nq in {1, 70, 1024}, random allow bitmaps of selectivity s in {0.001 .. 1.0}.  Per point:
the automatic path and both forced paths (filter_path 1 / 2), each as a FIRST call (a bitmap other than the one the handle's
sub-gallery was built from: path 1 compacts and gathers) and as a REPEAT call (the same bitmap again: path 1 reuses the
sub-gallery), next to the unfiltered Gallery.search on the same queries.  Every figure is the median of 5 wall times of
synchronous host calls after a warm-up call.  One GPU process:

    timeout -k 10 1200 python scripts/filtered_search_timing.py [out.json]

`--gather` instead runs only forced compactions (first calls) at s = 0.01, 0.1 and 0.5, for a kernel trace of
subset_gather_kernel (rocprofv3 --kernel-trace --stats -- python scripts/filtered_search_timing.py --gather); it prints the
rows gathered per call, from which the algorithmic bytes are (rows + padding rows) x (dp * 6 + 12), read once and written once.
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
SELS = (0.001, 0.01, 0.1, 0.25, 0.5, 0.9, 1.0)
NQS = (1, 70, 1024)


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


def words(sel, seed):
    m = np.random.default_rng(seed).random(N) < sel if sel < 1.0 else np.ones(N, bool)
    return _lib.allow_bitmap(m, N)


def main():
    g = gallery(1234)
    if "--gather" in sys.argv:
        g.set_option("filter_path", 1)
        for sel in (0.01, 0.1, 0.5):
            a, b = words(sel, 1), words(sel, 2)
            q = synth_rows(4321, 0, 1, D)
            for i in range(6):
                info = g.search_filtered(q, K, a if i % 2 else b)[3]
            print("gather s=%g: %d rows per call, 6 calls" % (sel, info["allowed"]), flush=True)
        g.close()
        return
    out = {"rows": N, "dim": D, "k": K, "points": []}
    for nq in NQS:
        q = synth_rows(4321, 0, nq, D)
        t_plain = median_time(lambda: g.search(q, K))
        for sel in SELS:
            a, b = words(sel, 1), words(sel, 2)
            pt = {"nq": nq, "s": sel, "unfiltered_ms": t_plain * 1e3}
            for name, path in (("auto", 0), ("compact", 1), ("overfetch", 2)):
                g.set_option("filter_path", path)
                flip = [0]

                def first():                        # a bitmap other than the stored one every call
                    flip[0] ^= 1
                    return g.search_filtered(q, K, a if flip[0] else b)
                pt[name + "_first_ms"] = median_time(first) * 1e3
                pt[name + "_repeat_ms"] = median_time(lambda: g.search_filtered(q, K, a)) * 1e3
                pt[name + "_info"] = g.search_filtered(q, K, a)[3]
            g.set_option("filter_path", 0)
            best_first = min(pt["compact_first_ms"], pt["overfetch_first_ms"])
            best_rep = min(pt["compact_repeat_ms"], pt["overfetch_repeat_ms"])
            pt["auto_first_vs_best"] = pt["auto_first_ms"] / best_first
            pt["auto_repeat_vs_best"] = pt["auto_repeat_ms"] / best_rep
            out["points"].append(pt)
            print("nq %4d s %-5g: unfiltered %7.3f | auto %7.3f / %7.3f (path %d) | compact %7.3f / %7.3f | overfetch %7.3f / "
                  "%7.3f (K' %d, re-run %d)  ms first / repeat"
                  % (nq, sel, pt["unfiltered_ms"], pt["auto_first_ms"], pt["auto_repeat_ms"], pt["auto_info"]["path"],
                     pt["compact_first_ms"], pt["compact_repeat_ms"], pt["overfetch_first_ms"], pt["overfetch_repeat_ms"],
                     pt["overfetch_info"]["kprime"], pt["overfetch_info"]["rerun_queries"]), flush=True)
    g.close()
    print(json.dumps(out))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
