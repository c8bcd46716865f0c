"""Timing of the IVF-Flat index (mi_ivfflat_build, mi_ivfflat_search_device): synthetic clustered rows made on the
device (rows / 16 centres + noise) in a squared-L2 gallery, queries drawn near stored rows.  Records
  - the training time of the centroids (IVFFlatIndex.train on a sample of at most 65 536 rows) and the build time of the lists;
  - for nprobe in 1 / 16 / 64 and Q in 1 / 70 / 1024, k = 100, HIP events on the stream, median of 5 after a warm-up call: the whole
    search (probe, prefix, scan-and-select, merge), the same search fed its own probes (prefix, scan-and-select, merge), and their
    difference, the probe; scan and merge are one figure here (the ABI has no entry that stops between them);
  - the mean rows evaluated per query, recall@100 against mi_knn_search_l2_device, and that search's own time at the same Q;
  - the update in place: --append-frac of the rows (1 %) appended on the device, then the wall time of IVFFlatIndex.sync() beside the
    wall time of a new IVFFlatIndex.build() on the same gallery, and whether both hold the same tables; then as many random rows
    removed by IVFFlatIndex.remove() (the gallery's own removal included) beside a new build, likewise.  Both calls are synchronous.
Nothing here is asserted: the record is for DESIGN 5.18, with the shape and the date.  One GPU process:

    timeout -k 10 900 python scripts/ivfflat_timing.py [--rows N] [--dim D] [--nlist L] [--append-frac F] [--out out.json]
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


def same_tables(a, b):
    (a_off, a_rows), (b_off, b_rows) = a.lists(), b.lists()
    return bool(a.n == b.n and a_off.tobytes() == b_off.tobytes() and a_rows.tobytes() == b_rows.tobytes())


def time_update(g, f, cent, centres, m, gen, s):
    """Wall seconds of a sync after m appended rows and of a removal of m rows, each beside a new build on the same gallery."""
    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    which = torch.randint(0, centres.shape[0], (m,), device="cuda", generator=gen)
    extra = (centres[which] + 0.3 * torch.randn((m, centres.shape[1]), device="cuda", generator=gen)).contiguous()
    torch.cuda.synchronize()
    g.append_device(extra.data_ptr(), m, stream=s)
    torch.cuda.synchronize()
    added, sync_s = wall(f.sync)
    fresh, rebuild_s = wall(lambda: _lib.IVFFlatIndex.build(g, cent))
    out = {"rows_before": g.n - m, "rows_appended": int(added), "sync_seconds": sync_s, "rebuild_after_append_seconds": rebuild_s,
           "sync_equals_rebuild": same_tables(f, fresh)}
    fresh.close()
    gone = np.zeros(g.n, bool)
    gone[np.random.default_rng(7).permutation(g.n)[:m]] = True
    removed, remove_s = wall(lambda: f.remove(gone))
    fresh, rebuild_s = wall(lambda: _lib.IVFFlatIndex.build(g, cent))
    out.update({"rows_removed": int(removed), "remove_seconds_gallery_and_index": remove_s, "rebuild_after_remove_seconds": rebuild_s,
                "remove_equals_rebuild": same_tables(f, fresh)})
    fresh.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1005994)
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--append-frac", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivfflat_timing.json"))
    args = ap.parse_args()
    n, d, nlist = args.rows, args.dim, args.nlist
    m = max(1, int(n * args.append_frac))
    centers = max(16, n // 16)
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(7)
    centres = torch.randn((centers, d), device="cuda", generator=gen)
    rows = torch.empty((n, d), device="cuda")
    for r0 in range(0, n, 65536):                  # (block by block: no second array of the gallery's size)
        b = min(65536, n - r0)
        which = torch.randint(0, centers, (b,), device="cuda", generator=gen)
        rows[r0:r0 + b] = centres[which] + 0.3 * torch.randn((b, d), device="cuda", generator=gen)
    pick = torch.randint(0, n, (1024,), device="cuda", generator=gen)
    q = (rows[pick] + 0.05 * torch.randn((1024, d), device="cuda", generator=gen)).contiguous()
    sample = rows[torch.randperm(n, device="cuda", generator=gen)[:min(n, 65536)]].cpu().numpy()
    torch.cuda.synchronize()
    g = _lib.Gallery.l2_from_device_ptr(rows.data_ptr(), n, d, capacity=n + m)
    del rows
    t0 = time.time()
    cent = _lib.IVFFlatIndex.train(sample, nlist)
    t1 = time.time()
    f = _lib.IVFFlatIndex.build(g, cent)
    sizes = f.list_sizes()
    rec = {"rows": n, "d": d, "nlist": nlist, "k": K, "train_seconds": t1 - t0, "build_seconds": time.time() - t1,
           "index_hbm_bytes": f.hbm_bytes, "largest_list": int(sizes.max()), "empty_lists": int((sizes == 0).sum()), "cases": []}
    for nq in (1, 70, 1024):
        exact = torch.empty((nq, K), dtype=torch.int64, device="cuda")
        exact_ms = median_ms(lambda: g.search_l2_device(q.data_ptr(), nq, K, exact.data_ptr(), stream=s))
        want = exact.cpu().numpy()
        for nprobe in (1, 16, 64):
            if nprobe > nlist:
                continue
            idx = torch.empty((nq, K), dtype=torch.int64, device="cuda")
            scanned = torch.empty((nq,), dtype=torch.int64, device="cuda")
            all_ms = median_ms(lambda: f.search_device(q.data_ptr(), nq, K, idx.data_ptr(), nprobe=nprobe, scanned_ptr=scanned.data_ptr(),
                                                       stream=s))
            probes = torch.from_numpy(f.probe(q[:nq].cpu().numpy(), nprobe)).cuda()
            tail_ms = median_ms(lambda: f.search_device(q.data_ptr(), nq, K, idx.data_ptr(), nprobe=nprobe, probes_ptr=probes.data_ptr(),
                                                        stream=s))
            got = idx.cpu().numpy()
            rec["cases"].append({"queries": nq, "nprobe": nprobe, "search_ms": all_ms, "probe_ms": all_ms - tail_ms,
                                 "scan_and_merge_ms": tail_ms, "exact_search_ms": exact_ms,
                                 "rows_evaluated_per_query": float(scanned.cpu().numpy().mean()),
                                 "recall_at_100": float(np.mean([len(set(a) & set(b)) / K for a, b in zip(got.tolist(), want.tolist())]))})
            print(json.dumps(rec["cases"][-1]), flush=True)
    rec["update"] = time_update(g, f, cent, centres, m, gen, s)
    print(json.dumps(rec["update"]), flush=True)
    f.close()
    g.close()
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
