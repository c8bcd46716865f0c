#!/usr/bin/env python3
"""Timing of the binary index (mi_hamming_search_device) on one MI355X -> profiles/hamming_bench.json.

Codes are generated on the device (torch.randint), the index is built from the device pointer, queries are random codes.
Per case: warm-up steps, then `--steps` timed steps between two HIP events (one search_device call each), median and spread.
The work of the distance kernel is computed from the shapes: 2 lane-operations (xor, popcount-accumulate) per (row, query,
32-bit word) against the VALU roof 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz; its bytes (gallery once per query chunk + distance
matrix written) against 8 TB/s.  Per-kernel times come from a kernel trace taken in a run of its own:

    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/hamming_bench.py --cases 1m --steps 5 --tag trace
    python scripts/hamming_bench.py --merge-stats <dir>        # adds the kernels' shares to the JSON

The 1-query case also times the numpy restatement of matching_Greedyhash (packed popcount) on the host."""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "hamming_bench.json")

VALU_ROOF = 256 * 4 * 16 * 2.4e9          # lane-operations / s
HBM_ROOF = 8e12                           # bytes / s


def bench_case(_lib, torch, n, nbits, nq, k, steps, warmup, numpy_baseline):
    dev = torch.device("cuda", 0)
    nb = nbits // 8
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    codes = torch.empty((n, nb), dtype=torch.uint8, device=dev)
    step_rows = 1 << 22
    for r in range(0, n, step_rows):
        m = min(step_rows, n - r)
        codes[r:r + m] = torch.randint(0, 256, (m, nb), dtype=torch.uint8, device=dev, generator=gen)
    q = torch.randint(0, 256, (nq, nb), dtype=torch.uint8, device=dev, generator=gen)
    torch.cuda.synchronize()
    idx = _lib.BinaryGallery.from_device_ptr(codes.data_ptr(), n, nbits)
    host_codes = codes[:min(n, 1005994)].cpu().numpy() if numpy_baseline else None
    del codes
    torch.cuda.empty_cache()
    out_i = torch.empty((nq, k), dtype=torch.int64, device=dev)
    out_d = torch.empty((nq, k), dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(warmup):
        idx.search_device(q.data_ptr(), nq, k, out_i.data_ptr(), out_d.data_ptr(), stream=s)
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        idx.search_device(q.data_ptr(), nq, k, out_i.data_ptr(), out_d.data_ptr(), stream=s)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = np.array(ms)
    w32 = (nbits + 31) // 32
    npad = (n + 63) // 64 * 64
    budget = _lib.get_global_option("hamming_matrix_bytes")
    qc = max(1, min(nq, int(budget // (npad * 2))))
    chunks = (nq + qc - 1) // qc
    lane_ops = 2.0 * n * nq * w32
    dist_bytes = chunks * n * w32 * 4.0 + nq * npad * 2.0
    rec = {"n": n, "nbits": nbits, "queries": nq, "k": k, "steps": steps, "warmup": warmup,
           "ms_per_batch_median": float(np.median(ms)), "ms_per_batch_min": float(ms.min()), "ms_per_batch_max": float(ms.max()),
           "queries_per_s": nq / (float(np.median(ms)) * 1e-3), "query_chunks": chunks,
           "dist_lane_ops": lane_ops, "dist_valu_floor_ms": lane_ops / VALU_ROOF * 1e3,
           "dist_bytes": dist_bytes, "dist_hbm_floor_ms": dist_bytes / HBM_ROOF * 1e3,
           "select_bytes_min": 2.0 * nq * npad * 2.0, "hbm_bytes_index": idx.hbm_bytes,
           "step_over_floor": float(np.median(ms)) / (max(lane_ops / VALU_ROOF, dist_bytes / HBM_ROOF) * 1e3),
           "note": "step = one mi_hamming_search_device call (query words + distance kernel + selection kernel per chunk); "
                   "kernel shares: see kernel_stats when merged"}
    ids = out_i.cpu().numpy()
    if numpy_baseline and nq == 1 and host_codes.shape[0] == n:
        qh = q.cpu().numpy()
        t0 = time.perf_counter()
        reps = 3
        for _ in range(reps):
            x = host_codes ^ qh[0][None, :]
            d = np.bitwise_count(x.view(np.uint64)).sum(axis=1) if nb % 8 == 0 else np.bitwise_count(x).sum(axis=1)
            order = np.lexsort((np.arange(n), d))[:k]
        dt = (time.perf_counter() - t0) / reps
        rec["numpy_restatement_queries_per_s"] = 1.0 / dt
        rec["numpy_agrees"] = bool(np.array_equal(order, ids[0]))
    idx.close()
    return rec


def merge_stats(stats_dir):
    """kernel_stats CSV of a rocprofv3 --kernel-trace --stats run -> share of each hamming kernel, written into the JSON"""
    import csv
    files = glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_stats.csv under " + stats_dir)
    rows = list(csv.DictReader(open(files[0])))
    ham = {}
    for r in rows:
        name = r.get("Name", "")
        if "hamming_" in name:
            key = name.split("hamming_")[1].split("_kernel")[0]
            ham[key] = ham.get(key, 0.0) + float(r.get("TotalDurationNs", 0) or 0)
    tot = sum(ham.values())
    doc = json.load(open(OUT)) if os.path.exists(OUT) else {}
    doc["kernel_stats"] = {"source": "rocprofv3 --kernel-trace --stats, a run of its own", "total_ns": ham,
                           "share": {k: v / tot for k, v in ham.items()} if tot else {}}
    json.dump(doc, open(OUT, "w"), indent=1)
    print(json.dumps(doc["kernel_stats"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1m", help="comma list of: 1m (1 005 994 x 2048 bits at 1 / 70 / 1024 queries), 100m "
                                                  "(10^8 x 2048 bits at 1 / 70 queries), 1m-1024 / 1m-70 / 1m-1 (one batch size)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--merge-stats", default="")
    args = ap.parse_args()
    if args.merge_stats:
        return merge_stats(args.merge_stats)
    import torch
    import isehr_amd  # noqa: F401
    from isehr_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this benchmark measures the device and has no other path")
    shapes = []
    for c in args.cases.split(","):
        if c == "1m":
            shapes += [(1005994, 2048, nq) for nq in (1, 70, 1024)]
        elif c.startswith("1m-"):
            shapes.append((1005994, 2048, int(c[3:])))
        elif c == "100m":
            shapes += [(10 ** 8, 2048, nq) for nq in (1, 70)]
        else:
            raise SystemExit("unknown case " + c)
    results = []
    for n, nbits, nq in shapes:
        rec = bench_case(_lib, torch, n, nbits, nq, args.k, args.steps, args.warmup, numpy_baseline=n < 10 ** 7)
        print(json.dumps(rec), flush=True)
        results.append(rec)
    if args.tag != "trace":
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
        doc.update({"device": torch.cuda.get_device_name(0), "valu_roof_lane_ops_per_s": VALU_ROOF, "hbm_roof_bytes_per_s": HBM_ROOF,
                    "cases": results})
        json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
