"""Timing of mi_gallery_remove_rows on the full-size gallery: 1 005 994 x 2048 rows synthesised on the device, one
case per process so that each can run under its own time limit:

    for c in row0 rand1 rand50 last1 sweep yardstick; do
        timeout -k 10 300 python scripts/remove_rows_timing.py $c profiles/remove_rows_timing.json || break
    done

  row0       remove row 0: every row moves
  rand1      remove a random 1 %
  rand50     remove a random 50 %
  last1      remove the last 1 %: nothing moves
  sweep      row0 at remove_block_rows 16 384 .. 131 072 (the default is chosen from this)
  yardstick  the existing path: subset_gather_kernel on the complementary bitmap (a forced compaction of the filtered search,
             one query), complement of rand1 and of rand50 -- wall time of the call minus the cached call on the same bitmap

Every figure is the median of 5 wall times of the synchronous C call (the bitmap is already on the device) after a warm-up; the gallery is rebuilt from the raw device
rows before every repetition.  Bytes per second are the algorithmic bytes 2 (dp 6 + 12) per moved row (rows at or behind the
tile of the first removed row), once for the gather and once for the write-back.  Results are merged into the JSON file."""
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
from isehr_amd.synth import synth_rows  # noqa: E402

N, D, REPS = 1005994, 2048, 5
ROW_BYTES = 2 * (D * 6 + 12)


def raw_rows():
    raw = torch.empty((N, D), dtype=torch.float32, device="cuda")
    _lib.synth_fill_device(raw.data_ptr(), 1234, 0, N, D, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return raw


def mask_of(case):
    m = np.zeros(N, bool)
    if case == "row0":
        m[0] = True
    elif case == "rand1":
        m[np.random.default_rng(1).random(N) < 0.01] = True
    elif case == "rand50":
        m[np.random.default_rng(2).random(N) < 0.5] = True
    elif case == "last1":
        m[N - N // 100:] = True
    return m


def time_remove(raw, mask, block=0):
    _lib.set_global_option("remove_block_rows", block)
    # the bitmap is packed and uploaded outside the timer, and the C entry point is called directly: the timed region is the
    # library call alone (D2H of the 126 KB bitmap, its complement, the keep-list, the move, the maxima, one synchronisation)
    bits = torch.from_numpy(_lib.allow_bitmap(mask, N).view(np.int64)).cuda()
    torch.cuda.synchronize()
    lib, removed = _lib.load(), C.c_int64()
    ts = []
    for rep in range(REPS + 1):                        # the first one is the warm-up
        g = _lib.Gallery.from_device_ptr(raw.data_ptr(), N, D)
        t0 = time.perf_counter()
        rc = lib.mi_gallery_remove_rows(g._h, C.c_void_p(bits.data_ptr()), _lib.MI_DEVICE, C.byref(removed))
        ts.append(time.perf_counter() - t0)
        _lib.check(rc)
        g.close()
    _lib.set_global_option("remove_block_rows", 0)
    kept = N - removed.value
    first = int(np.argmax(mask))
    moved = 0 if kept == first else kept - first // 256 * 256      # nothing moves when only trailing rows leave
    t = float(np.median(ts[1:]))
    return {"removed": int(removed.value), "moved_rows": moved, "ms": t * 1e3, "min_ms": min(ts[1:]) * 1e3,
            "TB_per_s": 2 * moved * ROW_BYTES / t / 1e12, "block_rows": block}


def time_yardstick(raw, mask):
    g = _lib.Gallery.from_device_ptr(raw.data_ptr(), N, D)
    g.set_option("filter_path", 1)
    q = synth_rows(4321, 0, 1, D)
    a, b = ~mask, ~mask
    b = b.copy()
    b[0] = not b[0]                                    # another bitmap: the call after it compacts and gathers again
    first, cached = [], []
    for rep in range(REPS + 1):
        g.search_filtered(q, 10, b)
        t0 = time.perf_counter()
        g.search_filtered(q, 10, a)
        first.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        g.search_filtered(q, 10, a)
        cached.append(time.perf_counter() - t0)
    g.close()
    t = float(np.median(first[1:]) - np.median(cached[1:]))
    rows = int(a.sum())
    return {"gathered_rows": rows, "first_ms": float(np.median(first[1:])) * 1e3, "cached_ms": float(np.median(cached[1:])) * 1e3,
            "gather_ms": t * 1e3, "TB_per_s": rows * ROW_BYTES / t / 1e12}


def main():
    case, path = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else None
    raw = raw_rows()
    if case == "sweep":
        res = [time_remove(raw, mask_of("row0"), b) for b in (16384, 32768, 65536, 131072)]
    elif case == "yardstick":
        res = {c: time_yardstick(raw, mask_of(c)) for c in ("rand1", "rand50")}
    else:
        res = time_remove(raw, mask_of(case))
    print(case, json.dumps(res), flush=True)
    if path:
        out = json.load(open(path)) if os.path.exists(path) else {"rows": N, "dim": D, "reps": REPS}
        out[case] = res
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
