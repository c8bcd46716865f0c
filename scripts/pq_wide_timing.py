"""Timing of the wide PQ index (mi_pqw_search_device, mi_pqw_train) at a shape the caller names: random codebooks and
random codes made on the device (the scan's time does not depend on what the codes mean), random float32 rows for the training.
Records
  - ms of mi_pqw_search_device at Ks = --words for every batch of --queries (HIP events on the stream, median of 5 after a warm-up
    call; table, scan, selection and emit together), k = --k;
  - in the same process mi_pq_search_device at Ks = 256 on the same N and M (the byte index, the yardstick), and the wide index at
    Ks = 256 (its one-pass path on the byte index's input);
  - the algorithmic bytes of each scan: codes N * 4 * ceil(M / 2) (the byte index: N * 4 * ceil(M / 4)) plus the tables
    nq * M * Ks * 4, read once per slab by the wide scan (the slab rule of launch_pqw_scan, restated below);
  - one training iteration at Ks = --words on --train-rows rows: the assignment (one encode pass) and the update, device times
    from mi_pq_train_timing.
Nothing here is asserted: the record is for DESIGN 5.14f, with the shape and the date.  One GPU process:

    timeout -k 10 900 python scripts/pq_wide_timing.py [--rows N] [--dim D] [--books M] [--words Ks] [--queries 1,70,1024]
        [--train-rows N] [--k K] [--out out.json]
"""
import argparse
import json
import os
import sys

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


def wide_slabs(n, ks, nq):
    """(QT, book pairs per group, slabs) of launch_pqw_scan (csrc/pq_wide.hip) for one chunk of nq queries"""
    pair = 2 * ks * 4
    qt = 4 if nq >= 3 and 4 * pair <= 128 * 1024 else 2 if nq >= 2 and 2 * pair <= 128 * 1024 else 1
    nblk, tiles, waves = (n + 63) // 64, (nq + qt - 1) // qt, 16
    cap = _lib.PQW_SLAB_ROWS // 64
    slabs = max(min((512 + tiles - 1) // tiles, (nblk + waves - 1) // waves), (nblk + cap - 1) // cap, 1)
    per = (nblk + slabs - 1) // slabs
    return qt, (128 * 1024) // (pair * qt), (nblk + per - 1) // per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1005994)
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--books", type=int, default=16)
    ap.add_argument("--words", type=int, default=8192)
    ap.add_argument("--queries", default="1,70,1024")
    ap.add_argument("--train-rows", type=int, default=None, help="0 skips the training")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, d, M, Ks, k = args.rows, args.dim, args.books, args.words, args.k
    L = d // M
    batches = [int(v) for v in args.queries.split(",")]
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(7)
    rng = np.random.default_rng(7)
    rec = {"rows": n, "d": d, "books": M, "words": Ks, "k": k, "searches": []}
    q = torch.randn((max(batches), d), device="cuda", generator=gen)
    idx = torch.empty((max(batches), k), dtype=torch.int64, device="cuda")
    dist = torch.empty((max(batches), k), dtype=torch.float32, device="cuda")
    codes8 = torch.randint(0, 256, (n, M), device="cuda", generator=gen, dtype=torch.int32).to(torch.uint8)
    codes16 = torch.randint(0, Ks, (n, M), device="cuda", generator=gen, dtype=torch.int32).to(torch.int16)
    torch.cuda.synchronize()
    cb_wide = rng.standard_normal((M, Ks, L)).astype(np.float32)
    cb_byte = rng.standard_normal((M, 256, L)).astype(np.float32)
    codes8w = codes8.to(torch.int16)
    torch.cuda.synchronize()
    indexes = [("wide", Ks, _lib.WidePQIndex.from_device_ptr(cb_wide, codes16.data_ptr(), n)),
               ("byte", 256, _lib.PQIndex.from_device_ptr(cb_byte, codes8.data_ptr(), n)),
               ("wide_one_pass", 256, _lib.WidePQIndex.from_device_ptr(cb_byte, codes8w.data_ptr(), n))]
    for name, ks, g in indexes:
        code_bytes = n * 4 * ((M + 1) // 2 if name != "byte" else (M + 3) // 4)
        for nq in batches:
            ms = median_ms(lambda: g.search_device(q.data_ptr(), nq, k, idx.data_ptr(), dist_ptr=dist.data_ptr(), stream=s))
            one = {"index": name, "words": ks, "queries": nq, "search_ms": ms, "queries_per_s": nq / (ms * 1e-3)}
            if name == "byte":
                one["scan_bytes"] = code_bytes * ((nq + 3) // 4) + nq * M * ks * 4
            else:
                qt, gp, slabs = wide_slabs(n, ks, nq)
                one.update(query_tile=qt, books_per_group=min(2 * gp, M), slabs=slabs)
                one["scan_bytes"] = code_bytes * ((nq + qt - 1) // qt) + nq * M * ks * 4 * slabs
            one["matrix_bytes"] = nq * ((n + 63) // 64 * 64) * 4
            rec["searches"].append(one)
            print(json.dumps(one), flush=True)
        g.close()
    del codes8, codes16, codes8w
    tn = n if args.train_rows is None else args.train_rows
    if tn:
        x = torch.empty((tn, d), device="cuda")
        for r0 in range(0, tn, 65536):
            x[r0:r0 + 65536] = torch.randn((min(65536, tn - r0), d), device="cuda", generator=gen)
        torch.cuda.synchronize()
        _lib.pqw_train_device(x.data_ptr(), tn, d, M, Ks, 1)
        assign, update = _lib.pq_train_timing()
        rec["training"] = {"rows": tn, "iterations": 1, "assign_ms": float(assign[0]), "update_ms": float(update[0])}
        print(json.dumps(rec["training"]), flush=True)
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
