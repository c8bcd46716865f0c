"""Timing of mi_pq_remove_rows / mi_ivfpq_remove_rows against the only route to the same result without them:
get_codes / get_rows to the host, a numpy filter, from_codes into a second index.

    python scripts/pq_remove_timing.py profiles/pq_remove_timing.json [rows]

16 777 216 rows (or `rows`), M = 16, Ks = 256, nlist = 256, d = 64; codes and lists are random bytes generated on the device.  A
random 10 % and a random 90 % of the rows leave.  Per case:

  remove_ms   median wall time of the synchronous C call over REPS indexes rebuilt from the device codes (after a warm-up);
              the bitmap is packed beforehand and given as a host buffer, as PQIndex.remove gives it
  route_ms    wall time of get_codes / get_rows + filter + from_codes, once, in the same process (both indexes alive)
  bytes       what the in-place path has to move: flat -- the source rows from the first block that loses a row on are read, the
              survivors among them written to the staging area, read back and written to the index (16 bytes each time); IVF --
              every filled slot is read (16 code bytes + 4 id bytes) and every survivor written (20 bytes)
  TB_per_s    bytes / remove_ms, next to the 8 TB/s HBM figure of DESIGN.md"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import isehr_amd  # noqa: E402,F401
from isehr_amd import _lib  # noqa: E402

M, KS, NLIST, D, REPS = 16, 256, 256, 64, 3


def time_remove(make, entry, bits, n):
    lib, removed, ts = _lib.load(), C.c_int64(), []
    for rep in range(REPS + 1):                        # the first one is the warm-up
        idx = make()
        t0 = time.perf_counter()
        rc = getattr(lib, entry)(idx._h, C.c_void_p(bits.ctypes.data), _lib.MI_HOST, C.byref(removed))
        ts.append(time.perf_counter() - t0)
        _lib.check(rc)
        idx.close()
    return float(np.median(ts[1:])) * 1e3, min(ts[1:]) * 1e3, int(removed.value)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else None
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 24
    gen = torch.Generator(device="cuda").manual_seed(1234)
    codes = torch.randint(0, KS, (n, M), dtype=torch.uint8, device="cuda", generator=gen)
    lists = torch.randint(0, NLIST, (n,), dtype=torch.uint8, device="cuda", generator=gen)
    torch.cuda.synchronize()
    rng = np.random.default_rng(5)
    cb = rng.standard_normal((M, KS, D // M)).astype(np.float32)
    coarse = rng.standard_normal((NLIST, D)).astype(np.float32)
    make_flat = lambda: _lib.PQIndex.from_device_ptr(cb, codes.data_ptr(), n)                                    # noqa: E731
    make_ivf = lambda: _lib.IVFPQIndex.from_device_ptr(coarse, cb, codes.data_ptr(), lists.data_ptr(), n)        # noqa: E731
    out = {"rows": n, "M": M, "Ks": KS, "nlist": NLIST, "reps": REPS, "hbm_TB_per_s": 8.0,
           "pq_remove_block_rows": _lib.get_global_option("pq_remove_block_rows")}
    for frac in (0.1, 0.9):
        gone = np.random.default_rng(int(frac * 10)).random(n) < frac
        keep = ~gone
        bits = np.asarray(_lib.allow_bitmap(gone, n))
        first = int(np.argmax(gone))
        kept = int(keep.sum())
        # flat
        ms, lo, removed = time_remove(make_flat, "mi_pq_remove_rows", bits, n)
        moved = int(keep[first // 64 * 64:].sum())
        nbytes = (n - first // 64 * 64) * M + 3 * moved * M
        idx = make_flat()
        t0 = time.perf_counter()
        second = _lib.PQIndex.from_codes(cb, idx.get_codes()[keep], capacity=n)
        route = (time.perf_counter() - t0) * 1e3
        idx.remove(gone)
        same = bool(np.array_equal(idx.get_codes(), second.get_codes()))
        idx.close(), second.close()
        out["flat_%d" % int(frac * 100)] = {"removed": removed, "remove_ms": ms, "min_ms": lo, "route_ms": route, "bytes": nbytes,
                                            "TB_per_s": nbytes / ms / 1e9, "same_codes_as_route": same}
        print("flat", frac, json.dumps(out["flat_%d" % int(frac * 100)]), flush=True)
        # IVF
        ms, lo, removed = time_remove(make_ivf, "mi_ivfpq_remove_rows", bits, n)
        nbytes = n * (M + 4) + kept * (M + 4)
        idx = make_ivf()
        t0 = time.perf_counter()
        c, l = idx.get_rows()
        second = _lib.IVFPQIndex.from_codes(coarse, cb, c[keep], l[keep], capacity=n)
        route = (time.perf_counter() - t0) * 1e3
        idx.remove(gone)
        a, b = idx.get_rows(), second.get_rows()
        same = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(idx.list_sizes(), second.list_sizes()))
        idx.close(), second.close()
        out["ivf_%d" % int(frac * 100)] = {"removed": removed, "remove_ms": ms, "min_ms": lo, "route_ms": route, "bytes": nbytes,
                                           "TB_per_s": nbytes / ms / 1e9, "same_rows_as_route": same}
        print("ivf", frac, json.dumps(out["ivf_%d" % int(frac * 100)]), flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
