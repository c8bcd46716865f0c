"""Timing of the near-duplicate GROUPS of a binary index: 1 005 994 codes of 256 bits generated on the device, with
planted clusters of near copies (sizes 2, 16 and 3 000: every member is its cluster's source with at most 4 bits flipped, so two
members differ in at most 8 bits, while unrelated random codes lie some 15 standard deviations further out) at radius 8, where
only planted pairs hit.  Two paths to the same labels:

    groups   dedup.near_duplicate_groups_hamming: the union-find reads the self-join's ballots, no pair exists
    pairs    what there was before it: dedup.near_duplicate_pairs_hamming, then a union-find on the host over the pair list

Per path: wall time, and the peak of the device memory in use over the call (the device's free memory sampled every 5 ms from a
side thread, against its value before the index was built -- the library's allocations are not torch's, so torch's own counters
do not see them).  Then: are the two label vectors equal.  Each path runs in a fresh child process under its own time limit, and
the first failure stops the script:

    python scripts/components_timing.py profiles/components_timing.json [--rows N]

No figure is asserted anywhere; the script exits non-zero if a step fails or the labels differ.
"""
import json
import os
import subprocess
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NBITS, RADIUS, FLIPS, BATCH = 1005994, 256, 8, 4, 4096
CLUSTERS = ((2, 1000), (16, 100), (3000, 1))           # (size, how many)
STEP_LIMIT = 900                                       # seconds per child


def planted_codes(n):
    """-> uint8 [n, 32] on the device and the number of planted pairs"""
    import torch
    gen = torch.Generator(device="cuda").manual_seed(20240521)
    codes = torch.randint(0, 256, (n, NBITS // 8), dtype=torch.uint8, device="cuda", generator=gen)
    clusters = [(size, count) for size, count in CLUSTERS if size * count <= n // 4]
    rows = torch.randperm(n, device="cuda", generator=gen)[:sum(size * count for size, count in clusters)]
    at, pairs = 0, 0
    for size, count in clusters:
        for _ in range(count):
            members = rows[at:at + size]
            at += size
            pairs += size * (size - 1) // 2
            noise = torch.zeros((size, NBITS // 8), dtype=torch.uint8, device="cuda")
            bits = torch.randint(0, NBITS, (size, FLIPS), device="cuda", generator=gen)
            keep = torch.rand((size, FLIPS), device="cuda", generator=gen) < 0.75        # 0 .. FLIPS flips a member
            for f in range(FLIPS):                      # a bit drawn twice flips back: still within FLIPS of the source
                one = (torch.ones(size, dtype=torch.int64, device="cuda") << (bits[:, f] & 7)).to(torch.uint8) * keep[:, f].to(torch.uint8)
                noise[torch.arange(size, device="cuda"), bits[:, f] >> 3] ^= one
            noise[0] = 0
            codes[members] = codes[members[0]].unsqueeze(0) ^ noise
    torch.cuda.synchronize()
    return codes, pairs


class PeakDeviceBytes:
    """the least free device memory seen while the block runs, as bytes in use beyond `base_free`"""

    def __init__(self, base_free):
        self.base, self.low, self.stop = base_free, base_free, threading.Event()

    def _run(self):
        import torch
        while not self.stop.is_set():
            self.low = min(self.low, torch.cuda.mem_get_info()[0])
            time.sleep(0.005)

    def __enter__(self):
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()
        return self

    def __exit__(self, *exc):
        import torch
        self.stop.set()
        self.thread.join()
        self.low = min(self.low, torch.cuda.mem_get_info()[0])

    @property
    def bytes(self):
        return int(self.base - self.low)


def host_union_find(n, i, j):
    """smaller root wins: labels[v] = the smallest row of v's component"""
    import numpy as np
    parent = list(range(n))
    for a, b in zip(i.tolist(), j.tolist()):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        if a < b:
            parent[b] = a
        elif b < a:
            parent[a] = b
    labels = np.arange(n, dtype=np.int32)
    for v in range(n):
        r = v
        while parent[r] != r:
            r = parent[r]
        labels[v] = r
    return labels


def step(name, n, labels_path):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import isehr_amd  # noqa: F401
    from isehr_amd import _lib, dedup
    torch.cuda.init()
    base_free = torch.cuda.mem_get_info()[0]
    codes, planted = planted_codes(n)
    idx = _lib.BinaryGallery.from_device_ptr(codes.data_ptr(), n, NBITS)
    del codes
    torch.cuda.empty_cache()
    out = {"step": name, "rows": n, "planted_pairs": planted, "index_bytes": idx.hbm_bytes}
    with PeakDeviceBytes(base_free) as peak:
        t0 = time.perf_counter()
        if name == "groups":
            labels, groups = dedup.near_duplicate_groups_hamming(idx, RADIUS, batch=BATCH)
            out["seconds"] = time.perf_counter() - t0
        else:
            i, j, _ = dedup.near_duplicate_pairs_hamming(idx, RADIUS, batch=BATCH)
            out["join_seconds"] = time.perf_counter() - t0
            labels = host_union_find(n, i, j)
            groups = int((labels == np.arange(n)).sum())
            out["seconds"] = time.perf_counter() - t0
            out["pairs"] = int(i.size)
            out["host_pair_bytes"] = int(i.nbytes + j.nbytes + 4 * i.size)
    out["peak_device_bytes"] = peak.bytes
    out["groups"] = int(groups)
    idx.close()
    np.save(labels_path, labels)
    print(json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--step":
        return step(args[1], int(args[2]), args[3])
    n = int(args[args.index("--rows") + 1]) if "--rows" in args else N
    out_path = args[0] if args and not args[0].startswith("--") else None
    import numpy as np
    result = {"rows": n, "nbits": NBITS, "radius": RADIUS, "batch": BATCH, "steps": []}
    with tempfile.TemporaryDirectory() as tmp:
        paths = {}
        for name in ("groups", "pairs"):
            paths[name] = os.path.join(tmp, name + ".npy")
            r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--step", name, str(n),
                                paths[name]], capture_output=True, text=True)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit("step %r failed with exit status %d: stopping" % (name, r.returncode))
            result["steps"].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(json.dumps(result["steps"][-1]), flush=True)
        result["labels_equal"] = bool(np.array_equal(np.load(paths["groups"]), np.load(paths["pairs"])))
    print(json.dumps({"labels_equal": result["labels_equal"]}), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
    if not result["labels_equal"]:
        sys.exit("the two paths disagree on the labels")


if __name__ == "__main__":
    main()
