"""Timing of the Minkowski search (mi_knn_search_minkowski_device): synthetic Gaussian rows made on the device in a
NORM_NONE gallery, Gaussian queries.  Records, for L1, Lp with p = 0.5 and Lp with p = 3 at Q in 1 / 8 / 64, k = 100, HIP events on
the stream, median of 5 after a warm-up call: the whole search (query staging, scan, selection, merge), and from it the rows a
second, the float64 column terms a second and the HBM bytes a second of the scan's own count (4 d bytes of every row once per tile
of queries).  Nothing here is asserted: the record is for DESIGN 5.19, with the shape and the date.  One GPU process:

    timeout -k 10 900 python scripts/minkowski_timing.py [--rows N] [--dim D] [--out out.json]
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


def query_tile(d):
    """kernels.h mink_query_tile: queries of a scan tile"""
    row = (d + 3) // 4 * 4 * 8
    return next((qt for qt in (8, 4, 2, 1) if qt * row <= 160 * 1024), 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1005994)
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "minkowski_timing.json"))
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
    qt = query_tile(d)
    rec = {"rows": n, "d": d, "k": K, "query_tile": qt, "date": time.strftime("%Y-%m-%d"), "cases": []}
    for metric, p in (("l1", None), ("lp", 0.5), ("lp", 3.0)):
        for nq in (1, 8, 64):
            idx = torch.empty((nq, K), dtype=torch.int64, device="cuda")
            ms = median_ms(lambda: g.search_minkowski_device(q.data_ptr(), nq, K, idx.data_ptr(), metric=metric, p=p, stream=s))
            tiles = -(-nq // qt)
            rec["cases"].append({"metric": metric, "p": p, "queries": nq, "search_ms": ms, "rows_per_second": n * nq / (ms * 1e-3),
                                 "column_terms_per_second": n * nq * d / (ms * 1e-3),
                                 "scan_hbm_bytes_per_second": tiles * n * d * 4 / (ms * 1e-3)})
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
