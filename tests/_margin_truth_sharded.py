"""The worst-case rounding data of tests/_margin_truth.py laid out over the shards of the two-phase protocol, its
truth and a host model of the protocol.

The gallery is cut into SHARDS = 3 contiguous row ranges by shard_bounds (the rule of isehr_amd.sharded).  Shards 0 and 1 are
LOUD: they hold imposters and victims with f = 31/64, so their own max |g^ - g| is f ulp sqrt(d).  Shard 2 is QUIET: it holds
fillers (image error zero) and the victims of the quiet patterns, whose rows drop only f' = 8/64 of an ulp, so its own
max |g^ - g| is f' ulp sqrt(d).  Pattern p is quiet when p is odd; its imposters (and a split pattern's) lie on loud shard
(p // 2) % 2.

  split pattern  K imposters at s^ = T on one loud shard, K victims (f = 31/64) on the OTHER loud shard, on the levels of the
                 single-gallery problem T - ceil(2 d f) + 1 ... T - ceil(d f): the lowest victim needs 0.95 ... 0.985 of the margin,
                 measured from the GATHERED L = T, which its own shard never sees among its rows.
  quiet pattern  K imposters (f) on a loud shard, K victims (f') on the quiet shard on the levels T - ceil(d (f + f')) + 1 ...
                 T - ceil(d f'): a victim's exact score (level + d f') is above every imposter's (T - d f), and the lowest victim
                 lies ceil(d (f + f')) - 1 units below L -- more than twice the quiet shard's OWN margin (2 d f' units and the
                 gamma term), about 0.62 of the agreed one.  0.62 is inherent: eps_q bounds each row's error by the worst
                 shard's, and the pair attains (eps_imposter + eps_victim) / (2 max eps) = (f + f') / (2 f).

Every value is dyadic as in _margin_truth.py, so every score is exact in any order.  protocol(theta, own) is the protocol on the
host: per-shard top-K of the 16-bit scores, L = the K-th of the gathered lists, per shard the rows at s^ >= L - theta margin with
the margin from the agreed norm maxima (own: from the shard's own), exact re-score, per-shard top-K, merge."""
import math

import numpy as np

import _margin_truth as mt

SHARDS = 3
QUIET_NUM = 8                   # f' = 8/64
QUIET_SHARD = 2


def shard_bounds(n, world, rank):
    """isehr_amd.sharded.shard_bounds, restated (the CPU file imports no library code; the GPU file asserts they agree)"""
    per = -(-n // world)
    lo = min(n, rank * per)
    return lo, min(n, lo + per)


class ShardedProblem(mt.Problem):
    """mt.Problem's attributes and methods over the sharded layout; fnum[row] = t f 64 of the row (signed, 0 for fillers)"""

    def __init__(self, d, image, n, k=mt.K, patterns=mt.PATTERNS, seed=3):
        # (seed: one whose magnitudes stay inside the binade, which _magnitudes asserts)
        fm = mt.FORMATS[image]
        rng = np.random.default_rng([seed, d, n, image == "f16"])
        self.d, self.image, self.n, self.k, self.patterns, self.ulp = d, image, n, k, patterns, fm["ulp"]
        self.dp = -(-d // 64) * 64
        self.unit = mt.C_Q * self.ulp
        self.grid = self.ulp / mt.F_DEN
        self.T = d * fm["mean"]
        f, fq = mt.F_NUM, QUIET_NUM
        ceil = lambda num: math.ceil(d * num / mt.F_DEN)  # noqa: E731
        self.v_low, self.v_high = self.T - ceil(2 * f) + 1, self.T - ceil(f)                # split victims
        self.vq_low, self.vq_high = self.T - ceil(f + fq) + 1, self.T - ceil(fq)            # quiet victims
        lv_split = self.v_low + np.arange(k) % (self.v_high - self.v_low + 1)
        lv_quiet = self.vq_low + np.arange(k) % (self.vq_high - self.vq_low + 1)
        self.quiet = np.arange(patterns) % 2 == 1
        self.bounds = [shard_bounds(n, SHARDS, r) for r in range(SHARDS)]
        free = [list(lo + rng.permutation(hi - lo)) for lo, hi in self.bounds]

        def take(r, m):
            rows, free[r] = np.sort(np.array(free[r][:m], np.int64)), free[r][m:]
            assert len(rows) == m, "shard %d is too small" % r
            return rows

        self.sigma = rng.choice(np.array([-1, 1], np.int64), size=(patterns, d))
        self.kind = np.zeros(n, np.int8)
        self.pattern = np.full(n, -1, np.int64)
        self.fnum = np.zeros(n, np.int64)
        self.imposter_shard = (np.arange(patterns) // 2) % 2
        self.victim_shard = np.where(self.quiet, QUIET_SHARD, 1 - self.imposter_shard)
        ints = np.zeros((n, d), np.int64)
        vic, imp = [], []
        for p in range(patterns):
            vnum, levels = (fq, lv_quiet) if self.quiet[p] else (f, lv_split)
            vic.append(take(int(self.victim_shard[p]), k))
            imp.append(take(int(self.imposter_shard[p]), k))
            for rows, kind, tf, sums in ((vic[p], mt.VICTIM, vnum, levels), (imp[p], mt.IMPOSTER, -f, np.full(k, self.T))):
                self.kind[rows], self.pattern[rows], self.fnum[rows] = kind, p, tf
                ints[rows] = self.sigma[p] * (mt.F_DEN * mt._magnitudes(rng, sums, d, fm) + tf)
        self.victims, self.imposters = np.stack(vic), np.stack(imp)
        fill = np.flatnonzero(self.kind == mt.FILLER)
        ints[fill] = rng.choice(np.array([-1, 1], np.int64), size=(len(fill), d)) * mt.F_DEN * \
            mt._magnitudes(rng, rng.integers(self.v_low, self.T + 1, size=len(fill)), d, fm)
        self.X_int = ints
        self.X = (ints.astype(np.float64) * self.grid).astype(np.float32)
        assert (self.X.astype(np.float64) == ints * self.grid).all()
        self.Xh = mt.round16(self.X, image)
        self._cache = {}

    def shard_of(self, rows):
        return np.searchsorted(np.array([lo for lo, _ in self.bounds]), rows, side="right") - 1

    # ---- norm maxima
    def shard_norm_bounds(self, r):
        """shard r's own maxima of (|g|, |g^|, |g^ - g|), float32"""
        lo, hi = self.bounds[r]
        x, xh = self.X[lo:hi].astype(np.float64), self.Xh[lo:hi].astype(np.float64)
        return mt._norm32(x).max(), mt._norm32(xh).max(), mt._norm32(xh - x).max()

    def agreed_bounds(self):
        """the all-reduce (MAX) of ShardedGallery._agree"""
        return tuple(np.max(np.array([self.shard_norm_bounds(r) for r in range(SHARDS)], np.float32), axis=0))

    def shard_margin(self, r=None):
        """float64 [patterns]: the margin from the agreed maxima (r None) or from shard r's own"""
        return self.margin(0, self.agreed_bounds() if r is None else self.shard_norm_bounds(r)).astype(np.float64)

    # ---- the protocol on the host
    def gathered_kth(self):
        """L float64 [patterns]: the K-th largest of the shards' K largest 16-bit scores"""
        A = self.approx()
        tops = [-np.sort(-A[:, lo:hi], axis=1)[:, :self.k] for lo, hi in self.bounds]
        return -np.sort(-np.concatenate(tops, 1), axis=1)[:, self.k - 1]

    def protocol(self, theta=1.0, own=False):
        """-> merged ids int64 [patterns, k] (-1 where fewer candidates), scores float64, candidates int64 [patterns, SHARDS],
        per-shard lists: ids int64 [SHARDS, patterns, k] (-1 padded) and scores float64 (-inf padded)"""
        A, S, L = self.approx(), self.exact(), self.gathered_kth()
        P, k = self.patterns, self.k
        ids, sc = np.full((P, k), -1, np.int64), np.full((P, k), -np.inf)
        sid, ssc = np.full((SHARDS, P, k), -1, np.int64), np.full((SHARDS, P, k), -np.inf)
        count = np.zeros((P, SHARDS), np.int64)
        for r, (lo, hi) in enumerate(self.bounds):
            mg = self.shard_margin(r if own else None)
            for p in range(P):
                cand = lo + np.flatnonzero(A[p, lo:hi] >= L[p] - theta * mg[p])
                count[p, r] = len(cand)
                top = self._ranked(cand, S[p])[:k]
                sid[r, p, :len(top)], ssc[r, p, :len(top)] = top, S[p][top]
        for p in range(P):
            rows = sid[:, p][sid[:, p] >= 0]
            top = self._ranked(rows, S[p])[:k]
            ids[p, :len(top)], sc[p, :len(top)] = top, S[p][top]
        return ids, sc, count, sid, ssc

    def cut_clearance(self):
        """the smallest distance, in units, of any 16-bit score to the cut L - margin of its shard under the agreed maxima"""
        A, L, mg = self.approx(), self.gathered_kth(), self.shard_margin()
        return float(np.abs(A - (L - mg)[:, None]).min() / self.unit)

    def tightness_against(self, r=None):
        """float64 [patterns]: (L - the lowest 16-bit score of a true top-K row) / the margin from the agreed maxima (r None) or
        from shard r's own"""
        ids, _ = self.truth()
        low = np.take_along_axis(self.approx(), ids, 1).min(1)
        return (self.gathered_kth() - low) / self.shard_margin(r)


# (d, image, n, patterns) of the GPU file: 6000 rows a shard, the single gallery of 18 000 rows is on the sample schedule
CASES = [(64, "f16", 18000, mt.PATTERNS), (64, "bf16", 18000, mt.PATTERNS), (100, "f16", 18000, mt.PATTERNS),
         (100, "bf16", 18000, mt.PATTERNS)]
_problems = {}


def problem(d, image, n, patterns):
    """the shared, unchanged ShardedProblem of a case"""
    key = (d, image, n, patterns)
    if key not in _problems:
        _problems[key] = ShardedProblem(d, image, n, patterns=patterns)
    return _problems[key]
