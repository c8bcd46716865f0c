"""Timing of the Minkowski radius search (mi_range_search_minkowski_device) beside the top-K search on the same rows
(mi_knn_search_minkowski_device, k = 100): synthetic Gaussian rows made on the device in a NORM_NONE gallery, Gaussian queries.
For L1 and Lp with p = 2 at Q in 8 / 64 the radius is the median of the queries' 100th-smallest values (taken from the top-K search):
half of the queries have 100 hits or more, the others fewer -- on Gaussian rows the counts spread widely around 100, and the record
holds their minimum, maximum and sum.  HIP events on the stream, median of 5 after a warm-up call: the whole radius search (query
staging, scan, count, offsets, emit, order, write-out; capacity Q * 65536, the record says whether the hits fit) and the whole top-K
search.  Nothing here is asserted: the record is for DESIGN 5.19b, with the shape and the date.  One GPU process:

    timeout -k 10 900 python scripts/minkowski_range_timing.py [--rows N] [--dim D] [--out out.json]
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

REPS, K = 5, 100
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    ap.add_argument("--rows", type=int, default=1005994)
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "minkowski_range_timing.json"))
    args = ap.parse_args()
    n, d = args.rows, args.dim
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(7)
    rows = torch.empty((n, d), device="cuda")
    for r0 in range(0, n, 65536):                  # (block by block: no second array of the gallery's size)
        b = min(65536, n - r0)
        rows[r0:r0 + b] = torch.randn((b, d), device="cuda", generator=gen)
    q = torch.randn((64, d), device="cuda", generator=gen).contiguous()
    torch.cuda.synchronize()
    g = _lib.Gallery.from_device_ptr(rows.data_ptr(), n, d, norm_mode=_lib.NORM_NONE)
    del rows
    rec = {"rows": n, "d": d, "k": K, "range_bytes": _lib.get_global_option("minkowski_range_bytes"),
           "date": time.strftime("%Y-%m-%d"), "cases": []}
    for metric, p in (("l1", None), ("lp", 2.0)):
        for nq in (8, 64):
            idx = torch.empty((nq, K), dtype=torch.int64, device="cuda")
            d64 = torch.empty((nq, K), dtype=torch.float64, device="cuda")
            topk = lambda: g.search_minkowski_device(q.data_ptr(), nq, K, idx.data_ptr(), metric=metric, p=p,   # noqa: E731
                                                     dist64_ptr=d64.data_ptr(), stream=s)
            topk_ms = median_ms(topk)
            radius = float(d64[:, K - 1].median().item())
            cap = nq * 65536
            lims = torch.empty(nq + 1, dtype=torch.int64, device="cuda")
            ridx = torch.empty(cap, dtype=torch.int64, device="cuda")
            rd64 = torch.empty(cap, dtype=torch.float64, device="cuda")
            rng = lambda: g.range_search_minkowski_device(q.data_ptr(), nq, radius, cap, lims.data_ptr(), ridx.data_ptr(),   # noqa: E731
                                                          metric=metric, p=p, dist64_ptr=rd64.data_ptr(), stream=s)
            range_ms = median_ms(rng)
            hits = np.diff(lims.cpu().numpy())
            rec["cases"].append({"metric": metric, "p": p, "queries": nq, "radius": radius, "hits_total": int(hits.sum()),
                                 "hits_min": int(hits.min()), "hits_max": int(hits.max()), "fits": bool(hits.sum() <= cap),
                                 "range_ms": range_ms, "topk_ms": topk_ms, "range_over_topk": range_ms / topk_ms,
                                 "rows_per_second": n * nq / (range_ms * 1e-3)})
            print(json.dumps(rec["cases"][-1]), flush=True)
    g.close()
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
