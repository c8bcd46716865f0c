"""Worst-case rounding data for the certificate's margin on a squared-L2 gallery, its exact truth and a BANDED host
model of the filter.

An L2 gallery ranks by s = q.g - 1/2 |g|^2 = [q, 1, 1, 1] . [g, c1, c2, c3] and the certificate's margin is taken on the augmented
vectors.  As in tests/_margin_truth.py the rows' rounding errors all point one way:

  query         q = q^ = sigma in {+-1}^d (exact in 16 bits): |q^'| = sqrt(d + 3), and the part of |q^'||g^' - g'| that data can
                attain, |q^| / |q^'| = sqrt(d / (d + 3)), is 0.976 at d = 61 (c1 has no image error, so g^' - g' cannot be parallel
                to the three ones; with 0.25 sigma it would be 0.75)
  special row   g_j = sigma_j (m_j + t f) ulp, m_j integers strictly inside the binade [0.125, 0.25) of the image type (ulp 2^-13 fp16,
                2^-10 bf16; |[g, b]| <= 2.2 at d = 100, so a gallery created with capacity = n takes the fp16 image, and one with
                capacity > n is bf16 from the start), f = 31/64: g^ - g = -t f ulp sigma is parallel to q^
  level         one unit = ulp.  The 16-bit score is ulp sum m + c1 + r16(c2) + r16(c3) =: a16, the exact key s = a16 + t d f ulp
                up to the image error of c2, c3 (at most 2^-7 unit).  b = -1/2 |g|^2 moves with sum m^2, so a row is PLACED: sum m is
                chosen so that a16 lands within a unit of its target level, then sum m^2 is steered by +-1 transfers between two
                columns (sum m stays, b moves by ulp (m_a - m_b + 1) units) until a16 is within TOL = 1/16 unit of the target
  imposters     t = -1, K rows at level T
  victims       t = +1, K rows on the levels T - 2 d f + GAP + i, i = 0 ... floor(d f - GAP): each beats every imposter in exact s
                by GAP - 2 TOL or more, and the lowest lies 2 d f - GAP units below L: 0.93 ... 0.97 of the shipped margin
  fillers       t = 0 under random signs; they and the rows of the other patterns score tens of thousands of units lower

Truth: q.g, |g|^2 and the direct-form distance sum (q_j - g_j)^2 are integers in units of (ulp / 64)^2 below 2^53, so the float64
distances are exact in any order: ids by (distance asc, id asc), float64 distance bits.

Band: c2 and c3 contribute products below the f32 ulp of the score, so the device's 16-bit score depends on the summation order.
The model takes the exactly rounded value a16 +- beta with beta = gamma |q^'| max|g^'|, the f32 accumulation bound the certificate
itself uses; "end" +1 moves every true top-K row DOWN and every other row UP by beta (the worst case for finding them), -1 the
other way.  Every statement the GPU file relies on is proved for both ends in tests/test_margin_truth_l2_cpu.py."""
import math

import numpy as np

import _gallery_file as gf
import _margin_truth as mt

K = mt.K
PATTERNS = mt.PATTERNS
F_NUM, F_DEN = mt.F_NUM, mt.F_DEN
GAP = 0.5                       # units by which the lowest victim's exact key beats an imposter's, before TOL
TOL = 1.0 / 16                  # units: |a16 - target level| of every placed row
# the binade [0.125, 0.25); the spread leaves room for the placement to move entries without leaving [lo, hi]
FORMATS = {"f16": dict(ulp=2.0 ** -13, lo=1025, hi=1536, mean=1280, spread=96),
           "bf16": dict(ulp=2.0 ** -10, lo=129, hi=192, mean=160, spread=10)}
FILLER, VICTIM, IMPOSTER = mt.FILLER, mt.VICTIM, mt.IMPOSTER


def _bias_units(m, tf, ulp):
    """b / ulp = -1/2 sum ((64 m + t f 64) ulp / 64)^2 / ulp, exact in float64 (an integer below 2^41 times a power of two)"""
    return -((F_DEN * m + tf) ** 2).sum(1).astype(np.float64) * (ulp / (2.0 * F_DEN * F_DEN))


def _place(rng, levels, tf, d, fm):
    """int64 magnitudes [len(levels), d] in [lo, hi] with sum m + b / ulp within a few ulp-steps of levels (see the module docstring)"""
    levels = np.asarray(levels, np.float64)
    R, ulp, lo, hi = len(levels), fm["ulp"], fm["lo"], fm["hi"]
    rows = np.arange(R)
    m = mt._magnitudes(rng, np.full(R, d * fm["mean"]), d, fm)
    for _ in range(16):                                       # sum m: a16 moves by 1 - ulp m_j ~ 0.84 units per step
        err = levels - (m.sum(1) + _bias_units(m, tf, ulp))
        dm = np.round(err / (1.0 - ulp * fm["mean"])).astype(np.int64)
        if not dm.any():
            break
        each = dm // d
        m += each[:, None]
        m += rng.random((R, d)).argsort(1) < (dm - each * d)[:, None]
    for _ in range(400):                                      # sum m^2: +1 on column a, -1 on column j
        err = levels - (m.sum(1) + _bias_units(m, tf, ulp))
        w = np.round(-err / ulp).astype(np.int64)             # wanted m_a - m_j + 1, summed over the transfers to come
        a = np.where(w > 0, np.where(m < hi, m, -1).argmax(1), m.argmin(1))
        step = m[rows, a][:, None] - m + 1
        cost = np.abs(w[:, None] - step)
        cost[m <= lo] = np.iinfo(np.int64).max
        cost[rows, a] = np.iinfo(np.int64).max
        j = cost.argmin(1)
        do = (w != 0) & (cost[rows, j] < np.abs(w)) & (m[rows, a] < hi)
        if not do.any():
            break
        m[rows[do], a[do]] += 1
        m[rows[do], j[do]] -= 1
    assert m.min() >= lo and m.max() <= hi
    return m


class L2Problem:
    """One L2 gallery [n, d] for one image type with `patterns` planted queries.  Scores are float64 [patterns, n] in the score's
    own scale (one unit = self.ulp); a batch of nq queries repeats the patterns, query i being pattern i % patterns."""

    def __init__(self, d, image, n, k=K, patterns=PATTERNS, seed=1):
        fm = FORMATS[image]
        rng = np.random.default_rng([seed, d, n, image == "f16"])
        self.d, self.image, self.n, self.k, self.patterns, self.ulp = d, image, n, k, patterns, fm["ulp"]
        self.f16 = image == "f16"
        self.dp = -(-(d + 3) // 64) * 64
        self.unit = self.ulp
        self.grid = self.ulp / F_DEN
        self.qg = int(round(1.0 / self.grid))                 # a query element, +-1, in units of grid
        self.df = d * F_NUM / F_DEN
        self.T = float(round(d * fm["mean"] * (1.0 - 0.5 * fm["mean"] * self.ulp)))
        self.nlev = int(math.floor(self.df - GAP)) + 1
        self.v_levels = self.T - 2 * self.df + GAP + np.arange(k) % self.nlev
        assert self.v_levels.max() <= self.T - self.df and n >= patterns * 2 * k + k
        self.sigma = rng.choice(np.array([-1, 1], np.int64), size=(patterns, d))
        nspecial = patterns * 2 * k
        place = rng.permutation(n)
        self.kind = np.zeros(n, np.int8)
        self.pattern = np.full(n, -1, np.int64)
        self.level = np.full(n, np.nan)
        self.victims = np.sort(place[:patterns * k].reshape(patterns, k), axis=1)
        self.imposters = np.sort(place[patterns * k:nspecial].reshape(patterns, k), axis=1)
        ints = np.zeros((n, d), np.int64)
        for p in range(patterns):
            for rows, kind, t, levels in ((self.victims[p], VICTIM, 1, self.v_levels), (self.imposters[p], IMPOSTER, -1, np.full(k, self.T))):
                self.kind[rows], self.pattern[rows], self.level[rows] = kind, p, levels
                ints[rows] = self.sigma[p] * (F_DEN * _place(rng, levels, t * F_NUM, d, fm) + t * F_NUM)
        fill = place[nspecial:]
        ints[fill] = rng.choice(np.array([-1, 1], np.int64), size=(len(fill), d)) * F_DEN * \
            mt._magnitudes(rng, d * fm["mean"] + rng.integers(-2 * d, 2 * d + 1, size=len(fill)), d, fm)
        self.X_int = ints
        self.X = (ints.astype(np.float64) * self.grid).astype(np.float32)
        assert (self.X.astype(np.float64) == ints * self.grid).all()
        self.Xh = mt.round16(self.X, image)
        self.P = (ints * ints).sum(1)                         # |g|^2 in units of grid^2, int64 (< 2^41)
        self.b = -0.5 * self.P.astype(np.float64) * (self.grid * self.grid)
        b, c1, c2, c3 = gf.split_bias(self.X, self.f16)
        assert np.array_equal(b, self.b)                      # the float64 plain sum is exact
        self.hidden = np.stack([c1, c2, c3], 1)               # float32 [n, 3]
        self.hidden16 = mt.round16(self.hidden, image)
        self._cache = {}

    # ---- queries
    def base_queries(self):
        return self.sigma.astype(np.float32)

    def queries(self, nq):
        return np.ascontiguousarray(self.base_queries()[np.arange(nq) % self.patterns])

    def of_query(self, nq):
        return np.arange(nq) % self.patterns

    # ---- scores
    def approx(self):
        """the exactly rounded 16-bit score q^.g^ + c1 + r16(c2) + r16(c3), float64 [patterns, n]"""
        if "approx" not in self._cache:
            xh = self.Xh.astype(np.float64) / self.ulp
            xi = xh.astype(np.int64)
            assert (xi == xh).all() and np.abs(xi).sum(1).max() < 2 ** 18
            h = self.hidden16.astype(np.float64)
            self._cache["approx"] = (self.sigma @ xi.T).astype(np.float64) * self.ulp + ((h[:, 0] + h[:, 1]) + h[:, 2])[None, :]
        return self._cache["approx"]

    def exact(self):
        """the exact key s = q.g - 1/2 |g|^2, float64 [patterns, n] (a multiple of grid^2 / 2 below 16: 43 bits)"""
        if "exact" not in self._cache:
            self._cache["exact"] = (self.sigma @ self.X_int.T).astype(np.float64) * self.grid + self.b[None, :]
        return self._cache["exact"]

    def dist_int(self):
        """the direct-form distance sum (q_j - g_j)^2 in units of grid^2, int64 [patterns, n] (< 2^46)"""
        if "dist" not in self._cache:
            self._cache["dist"] = self.d * self.qg * self.qg - 2 * self.qg * (self.sigma @ self.X_int.T) + self.P[None, :]
        return self._cache["dist"]

    # ---- the certificate on the augmented vectors, as csrc/l2_metric.hip, csrc/ingest.hip and csrc/select.hip compute it
    def aug_bounds(self, variant=None):
        """gallery maxima of (|g'|, |g^'|, |g^' - g'|) over the augmented rows, float32.  Damaged variants: "no_bias_img" /
        "no_bias_f32" leave the hidden columns out of |g^'| / |g'|, "diff_d_only" takes |g^' - g'| over the d user columns"""
        if ("bounds", variant) not in self._cache:
            x, xh = self.X.astype(np.float64), self.Xh.astype(np.float64)
            h, hh = self.hidden.astype(np.float64), self.hidden16.astype(np.float64)
            g = x if variant == "no_bias_f32" else np.concatenate([x, h], 1)
            gh = xh if variant == "no_bias_img" else np.concatenate([xh, hh], 1)
            diff = xh - x if variant == "diff_d_only" else np.concatenate([xh - x, hh - h], 1)
            self._cache["bounds", variant] = mt._norm32(g).max(), mt._norm32(gh).max(), mt._norm32(diff).max()
        return self._cache["bounds", variant]

    def _gamma(self):
        return np.float32(2.0) * np.float32(self.dp) * np.float32(5.9604645e-08)

    def margin(self, variant=None):
        """float32: 2 eps 1.001 + 1e-30 with eps = gamma |q^'||g^'| + |q^'||g^' - g'| (q^' = q': the third term is zero; the same
        for every pattern).  variant "no_plus_3" takes the query norm over the d user columns"""
        g_f32, g_img, g_diff = self.aug_bounds(variant)
        q_img = mt._norm32(np.ones(self.d + (0 if variant == "no_plus_3" else 3)))
        eps = self._gamma() * q_img * g_img + q_img * g_diff + np.float32(0.0) * g_f32
        return np.float32(2.0) * eps * np.float32(1.001) + np.float32(1e-30)

    def beta(self):
        """the band: gamma |q^'| max|g^'|, float64"""
        return float(self._gamma()) * float(mt._norm32(np.ones(self.d + 3))) * float(self.aug_bounds()[1])

    # ---- top-K
    def _allowed(self, allow):
        return np.ones(self.n, bool) if allow is None else np.asarray(allow, bool)

    def truth(self, allow=None, nq=None):
        """ids int64 [nq, k] by (direct-form distance asc, id asc) over the allowed rows, distances float64 [nq, k]"""
        key = ("truth", None if allow is None else np.asarray(allow, bool).tobytes())
        if key not in self._cache:
            D, rows = self.dist_int(), np.flatnonzero(self._allowed(allow))
            ids = np.stack([rows[np.lexsort((rows, dd[rows]))][:self.k] for dd in D])
            self._cache[key] = ids, np.take_along_axis(D, ids, 1).astype(np.float64) * (self.grid * self.grid)
        ids, dist = self._cache[key]
        pick = self.of_query(self.patterns if nq is None else nq)
        return ids[pick], dist[pick]

    def banded(self, end=0, allow=None):
        """the 16-bit scores at one end of the band: true top-K rows moved by -end beta, every other row by +end beta"""
        A = self.approx().copy()
        if end:
            sign = np.full(A.shape, float(end))
            np.put_along_axis(sign, self.truth(allow)[0], -float(end), 1)
            A += sign * self.beta()
        return A

    def kth(self, end=0, allow=None):
        """L: the k-th largest 16-bit score over the allowed rows at that end of the band, float64 [patterns]"""
        A = self.banded(end, allow)[:, self._allowed(allow)]
        return -np.partition(-A, self.k - 1, axis=1)[:, self.k - 1]

    def model_answer(self, theta, end=0, allow=None, variant=None):
        """The filter on the host: banded 16-bit scores, L, the candidates at s^ >= L - theta margin, the k largest exact keys
        (ties to the lower id), ordered by (distance asc, id asc) -> ids [patterns, k] (-1 where fewer candidates), distances"""
        A, S, D, ok = self.banded(end, allow), self.exact(), self.dist_int(), self._allowed(allow)
        L, mg = self.kth(end, allow), float(self.margin(variant))
        ids = np.full((self.patterns, self.k), -1, np.int64)
        dist = np.full((self.patterns, self.k), np.inf)
        for p in range(self.patterns):
            cand = np.flatnonzero(ok & (A[p] >= L[p] - theta * mg))
            top = cand[np.lexsort((cand, -S[p][cand]))][:self.k]
            top = top[np.lexsort((top, D[p][top]))]
            ids[p, :len(top)], dist[p, :len(top)] = top, D[p][top].astype(np.float64) * (self.grid * self.grid)
        return ids, dist

    def candidates(self, allow=None):
        """rows within the margin of L, per pattern, on the exactly rounded scores (cut_clearance says the band cannot change it)"""
        A, L = self.approx()[:, self._allowed(allow)], self.kth(0, allow)
        return (A >= (L - float(self.margin()))[:, None]).sum(1)

    def cut_clearance(self, allow=None):
        """the smallest distance of any allowed row's exactly rounded score to the cut L - margin, in units"""
        A, L = self.approx()[:, self._allowed(allow)], self.kth(0, allow)
        return float(np.abs(A - (L - float(self.margin()))[:, None]).min() / self.unit)

    def tightness(self, end=0, allow=None, variant=None):
        """float64 [patterns]: (L - the lowest 16-bit score of a true top-K row) / margin at that end of the band"""
        low = np.take_along_axis(self.banded(end, allow), self.truth(allow)[0], 1).min(1)
        return (self.kth(end, allow) - low) / float(self.margin(variant))

    def allow_sets(self):
        """the two allow sets of tests/_margin_truth.py: every other filler dropped; the odd-numbered imposters dropped"""
        fillers = np.flatnonzero(self.kind == FILLER)
        a = np.ones(self.n, bool)
        a[fillers[1::2]] = False
        b = np.ones(self.n, bool)
        b[self.imposters[:, 1::2].ravel()] = False
        return {"every other filler dropped": a, "odd imposters dropped": b}


# (d, image, n, patterns) of the GPU file: d + 3 = 64 fills dp; d = 62 puts c2, c3 into a second 64-column block; d = 100
N = 17000
CASES = [(d, image, N, PATTERNS) for d in (61, 62, 100) for image in ("f16", "bf16")]
_problems = {}


def problem(d, image, n, patterns):
    """the shared, unchanged L2Problem of a case"""
    key = (d, image, n, patterns)
    if key not in _problems:
        _problems[key] = L2Problem(d, image, n, patterns=patterns)
    return _problems[key]
