"""Worst-case rounding data for the exactness certificate, its exact truth and a host model of the filter.

The certificate bounds |s^ - s| <= eps_q = gamma |q^||g^| + |q^||g^ - g| + |q^ - q||g| and every threshold consumer keeps the rows
within margin = 2 eps_q 1.001 + 1e-30 of the K-th 16-bit score.  On random data the rounding errors of a row cancel and a
margin of half the size loses nothing; here they all point the same way, so the Cauchy-Schwarz term is ATTAINED:

  sign pattern  sigma in {+-1}^d, 16-bit query q^ = c sigma, c = 0.25
  special row   g_j = sigma_j (m_j + t f) ulp: m_j integers strictly inside one 16-bit binade (ulp its spacing), f = 31/64 < 1/2,
                so the image is g^_j = sigma_j m_j ulp and g^ - g = -t f ulp sigma is parallel to q^: q^.(g^ - g) = -t |q^||g^ - g|
  victims       t = +1: the image UNDERESTIMATES the exact score by d f units (one unit = c ulp)
  imposters     t = -1: the image OVERESTIMATES it by d f units
  fillers       t = 0, magnitudes of the same kind under random signs: they score near 0, as do the rows of the other patterns

In units, s^ = sum m_j and s = sum m_j + t d f.  K imposters sit at s^ = T, K victims on the levels T - ceil(2 d f) + 1 ... T -
ceil(d f): every victim's exact score is above every imposter's, so the float64 top-K is the victims (ties by id) while the 16-bit
top-K is the imposters, and the lowest victim lies ceil(2 d f) - 1 units below L = T: 0.95 ... 0.985 of the shipped margin.  A
consumer that applies 85 % of the margin loses rows.  PATTERNS patterns share a gallery, each with victims and imposters of its own.

Query form 1 (range search) moves the query itself off the 16-bit grid, q = q^ + f ulp sigma (float32, its image is q^): the
third term |q^ - q||g| is attained within ~1 % (the cosine between (m_j) and the all-ones vector) with the sign of the second.

Every value is a multiple of ulp / 64 with at most 17 significant bits, so every product and every float64 sum is exact in any
order (the device's f64 re-score equals the truth bit for bit) and every 16-bit score is an integer number of units below 2^18:
exact in f32 whatever the summation order.  tests/test_margin_truth_cpu.py proves these premises on the numbers made."""
import math

import numpy as np

C_Q = 0.25                     # |q^_j|
F_NUM, F_DEN = 31, 64          # f: the part of an ulp the 16-bit rounding drops
K = 100
PATTERNS = 16
# per image type: the ulp of the binade [0.25, 0.5) and the range of m_j (strictly inside the binade, m ulp <= 0.375 so that a row
# of 100 columns has norm <= 3.75: beyond 4 a raw gallery takes a bf16 image whatever was asked for)
FORMATS = {"f16": dict(ulp=2.0 ** -12, lo=1025, hi=1536, mean=1280, spread=160),
           "bf16": dict(ulp=2.0 ** -9, lo=129, hi=192, mean=160, spread=24)}
FILLER, VICTIM, IMPOSTER = 0, 1, 2


def bf16_round(x32):
    """float32 -> nearest-even bfloat16, returned as float32"""
    u = np.ascontiguousarray(x32, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def round16(x32, image):
    """float32 -> the 16-bit image type and back"""
    x32 = np.ascontiguousarray(x32, np.float32)
    return x32.astype(np.float16).astype(np.float32) if image == "f16" else bf16_round(x32)


def _magnitudes(rng, sums, d, fm):
    """int64 [len(sums), d], every entry in [lo, hi], row i summing to sums[i]"""
    sums = np.asarray(sums, np.int64)
    m = rng.integers(fm["mean"] - fm["spread"], fm["mean"] + fm["spread"] + 1, size=(len(sums), d)).astype(np.int64)
    diff = sums - m.sum(1)
    each = diff // d
    m += each[:, None]
    rest = diff - each * d                                   # in [0, d): one more on that many random columns
    m += rng.random((len(sums), d)).argsort(1) < rest[:, None]
    assert (m.sum(1) == sums).all() and m.min() >= fm["lo"] and m.max() <= fm["hi"]
    return m


def _norm32(v):
    """the stored rounding norm: (float)(sqrt(sum v^2) (1 + 1e-6)), csrc/ingest.hip"""
    v = np.asarray(v, np.float64)
    return (np.sqrt((v * v).sum(-1)) * (1.0 + 1e-6)).astype(np.float32)


class Problem:
    """One gallery [n, d] for one image type ("f16" | "bf16") with `patterns` planted queries; see the module docstring.
    Scores are float64 arrays [patterns, n]; a batch of nq queries repeats the patterns, query i being pattern i % patterns."""

    def __init__(self, d, image, n, k=K, patterns=PATTERNS, seed=1):
        fm = FORMATS[image]
        rng = np.random.default_rng([seed, d, n, image == "f16"])
        self.d, self.image, self.n, self.k, self.patterns, self.ulp = d, image, n, k, patterns, fm["ulp"]
        self.dp = -(-d // 64) * 64
        self.unit = C_Q * self.ulp                            # one step of a 16-bit score
        self.grid = self.ulp / F_DEN                          # every element of X and Q is a multiple of it
        self.T = d * fm["mean"]
        two_df, df = math.ceil(2 * d * F_NUM / F_DEN), math.ceil(d * F_NUM / F_DEN)
        self.v_low, self.v_high = self.T - two_df + 1, self.T - df
        levels = self.v_low + np.arange(k) % (self.v_high - self.v_low + 1)
        assert levels.min() == self.v_low and levels.max() <= self.v_high and n >= patterns * 2 * k + k
        self.sigma = rng.choice(np.array([-1, 1], np.int64), size=(patterns, d))
        nspecial = patterns * 2 * k
        place = rng.permutation(n)                            # special rows first, then the fillers
        self.kind = np.zeros(n, np.int8)
        self.pattern = np.full(n, -1, np.int64)
        self.victims = np.sort(place[:patterns * k].reshape(patterns, k), axis=1)
        self.imposters = np.sort(place[patterns * k:nspecial].reshape(patterns, k), axis=1)
        ints = np.zeros((n, d), np.int64)                     # rows in units of grid
        for p in range(patterns):
            for rows, kind, t, sums in ((self.victims[p], VICTIM, 1, levels), (self.imposters[p], IMPOSTER, -1, np.full(k, self.T))):
                self.kind[rows], self.pattern[rows] = kind, p
                ints[rows] = self.sigma[p] * (F_DEN * _magnitudes(rng, sums, d, fm) + t * F_NUM)
        fill = place[nspecial:]
        ints[fill] = rng.choice(np.array([-1, 1], np.int64), size=(len(fill), d)) * F_DEN * \
            _magnitudes(rng, rng.integers(self.v_low, self.T + 1, size=len(fill)), d, fm)
        self.X_int = ints
        self.X = (ints.astype(np.float64) * self.grid).astype(np.float32)
        assert (self.X.astype(np.float64) == ints * self.grid).all()
        self.Xh = round16(self.X, image)
        self._cache = {}

    # ---- queries
    def base_queries(self, form):
        """float32 [patterns, d]: form 0 = q^ = c sigma, form 1 = q^ + f ulp sigma (the same image)"""
        q = self.sigma * (C_Q + (F_NUM / F_DEN * self.ulp if form else 0.0))
        q32 = q.astype(np.float32)
        assert (q32.astype(np.float64) == q).all()
        return q32

    def queries(self, form, nq):
        return np.ascontiguousarray(self.base_queries(form)[np.arange(nq) % self.patterns])

    def of_query(self, nq):
        return np.arange(nq) % self.patterns

    # ---- scores: integer arithmetic, then one exact conversion
    def approx(self, form=0):
        """16-bit scores q^.g^ as float64 [patterns, n] (an integer number of units, exact in f32 in any order)"""
        if "approx" not in self._cache:
            qh = round16(self.base_queries(form), self.image).astype(np.float64) / C_Q
            xh = self.Xh.astype(np.float64) / self.ulp
            qi, xi = qh.astype(np.int64), xh.astype(np.int64)
            assert (qi == qh).all() and (np.abs(qi) == 1).all() and (xi == xh).all()
            units = qi @ xi.T
            assert np.abs(xi).sum(1).max() < 2 ** 18          # every partial sum of every order fits 24 bits
            self._cache["approx"] = units.astype(np.float64) * self.unit
        return self._cache["approx"]

    def exact(self, form=0):
        """exact scores q.g as float64 [patterns, n]"""
        key = ("exact", form)
        if key not in self._cache:
            q = self.base_queries(form).astype(np.float64) / self.grid
            qi = q.astype(np.int64)
            assert (qi == q).all()
            s = qi @ self.X_int.T                             # < 2^18 * 2^18 * 128 = 2^43
            assert np.abs(qi).max() * np.abs(self.X_int).sum(1).max() < 2 ** 53
            self._cache[key] = s.astype(np.float64) * (self.grid * self.grid)
        return self._cache[key]

    # ---- the certificate, as csrc/ingest.hip and csrc/select.hip compute it (float32 arithmetic)
    def norm_bounds(self):
        """gallery maxima of (|g|, |g^|, |g^ - g|), float32"""
        x, xh = self.X.astype(np.float64), self.Xh.astype(np.float64)
        return _norm32(x).max(), _norm32(xh).max(), _norm32(xh - x).max()

    def eps(self, form=0, bounds=None):
        """float32 [patterns]: eps_q = gamma |q^||g^| + |q^||g^ - g| + |q^ - q||g|; bounds: other maxima than the gallery's own"""
        g_f32, g_img, g_diff = self.norm_bounds() if bounds is None else (np.float32(v) for v in bounds)
        q = self.base_queries(form)
        qh = round16(q, self.image)
        q_img, q_diff = _norm32(qh), _norm32(qh.astype(np.float64) - q.astype(np.float64))
        gamma = np.float32(2.0) * np.float32(self.dp) * np.float32(5.9604645e-08)
        return gamma * q_img * g_img + q_img * g_diff + q_diff * g_f32

    def margin(self, form=0, bounds=None):
        """float32 [patterns]: 2 eps 1.001 + 1e-30"""
        return np.float32(2.0) * self.eps(form, bounds) * np.float32(1.001) + np.float32(1e-30)

    # ---- top-K
    def _allowed(self, allow):
        return np.ones(self.n, bool) if allow is None else np.asarray(allow, bool)

    def _ranked(self, rows, s):
        return rows[np.lexsort((rows, -s[rows]))]

    def truth(self, form=0, allow=None, nq=None):
        """ids int64 [nq, k] by (exact score desc, id asc) over the allowed rows, scores float64 [nq, k]"""
        S, rows = self.exact(form), np.flatnonzero(self._allowed(allow))
        ids = np.stack([self._ranked(rows, s)[:self.k] for s in S])
        sc = np.take_along_axis(S, ids, 1)
        pick = self.of_query(self.patterns if nq is None else nq)
        return ids[pick], sc[pick]

    def kth_approx(self, allow=None):
        """L: the k-th largest 16-bit score over the allowed rows, float64 [patterns]"""
        A = self.approx()[:, self._allowed(allow)]
        return -np.partition(-A, self.k - 1, axis=1)[:, self.k - 1]

    def model_answer(self, theta, form=0, allow=None):
        """The filter on the host: 16-bit scores, L, the candidates at s^ >= L - theta margin, exact re-score, sort, cut.
        -> ids [patterns, k] (-1 where fewer than k candidates), scores float64"""
        A, S, ok = self.approx(), self.exact(form), self._allowed(allow)
        L, mg = self.kth_approx(allow), self.margin(form).astype(np.float64)
        ids = np.full((self.patterns, self.k), -1, np.int64)
        sc = np.full((self.patterns, self.k), -np.inf)
        for p in range(self.patterns):
            cand = self._ranked(np.flatnonzero(ok & (A[p] >= L[p] - theta * mg[p])), S[p])[:self.k]
            ids[p, :len(cand)], sc[p, :len(cand)] = cand, S[p][cand]
        return ids, sc

    def candidates(self, theta=1.0, form=0, allow=None):
        """rows within theta margin of L, per pattern"""
        A, L, mg = self.approx()[:, self._allowed(allow)], self.kth_approx(allow), self.margin(form).astype(np.float64)
        return (A >= (L - theta * mg)[:, None]).sum(1)

    def tightness(self, form=0, allow=None):
        """float64 [patterns]: (L - the lowest 16-bit score of a true top-K row) / margin, the part of the shipped margin this
        data needs"""
        ids, _ = self.truth(form, allow)
        low = np.take_along_axis(self.approx(), ids, 1).min(1)
        return (self.kth_approx(allow) - low) / self.margin(form).astype(np.float64)

    # ---- range search
    def range_min_score(self, form=0, units_up=0):
        """the lowest victim's exact score (the same for every pattern), raised by units_up units"""
        S = self.exact(form)
        low = np.array([S[p][self.victims[p]].min() for p in range(self.patterns)])
        assert (low == low[0]).all()
        return float(low[0] + units_up * self.unit)

    def range_truth(self, min_score, form=0, nq=None):
        """-> lims int64 [nq + 1], ids int64, scores float64: per query the rows with exact score >= min_score by (score desc, id asc)"""
        return self.range_model(None, min_score, form, nq)

    def range_model(self, theta, min_score, form=0, nq=None):
        """the range filter on the host: rows with s^ >= min_score - theta eps (theta None: every row), exact re-score, the
        rows at >= min_score kept and sorted -> lims, ids, scores float64.  eps is margin / 2, what csrc/range_select.hip takes."""
        A, S = self.approx(), self.exact(form)
        half = 0.5 * self.margin(form).astype(np.float64)
        per = []
        for p in range(self.patterns):
            keep = S[p] >= min_score
            if theta is not None:
                keep &= A[p] >= min_score - theta * half[p]
            per.append(self._ranked(np.flatnonzero(keep), S[p]))
        pick = self.of_query(self.patterns if nq is None else nq)
        lims = np.concatenate([[0], np.cumsum([len(per[p]) for p in pick])]).astype(np.int64)
        ids = np.concatenate([per[p] for p in pick]) if len(pick) else np.zeros(0, np.int64)
        sc = np.concatenate([S[p][per[p]] for p in pick]) if len(pick) else np.zeros(0)
        return lims, ids.astype(np.int64), sc

    def range_tightness(self, form=0, units_up=0):
        """float64 [patterns]: (min_score - the lowest 16-bit score of a true hit) / eps"""
        ms = self.range_min_score(form, units_up)
        A, S = self.approx(), self.exact(form)
        need = np.array([ms - A[p][S[p] >= ms].min() for p in range(self.patterns)])
        return need / (0.5 * self.margin(form).astype(np.float64))

    # ---- allow sets of the filtered search
    def allow_sets(self):
        """name -> bool [n]: every special row and every other filler (the truth is unchanged); everything but the odd-numbered
        imposters (the truth is still the victims, L moves down)"""
        fillers = np.flatnonzero(self.kind == FILLER)
        a = np.ones(self.n, bool)
        a[fillers[1::2]] = False
        b = np.ones(self.n, bool)
        b[self.imposters[:, 1::2].ravel()] = False
        return {"every other filler dropped": a, "odd imposters dropped": b}


# (d, image, n, patterns) of the GPU file; the CPU file proves the premises for each
CASES = [(64, "f16", 20000, PATTERNS), (64, "bf16", 20000, PATTERNS), (100, "f16", 20000, PATTERNS), (100, "bf16", 20000, PATTERNS),
         (64, "f16", 3000, 8)]
_problems = {}


def problem(d, image, n, patterns):
    """the shared, unchanged Problem of a case"""
    key = (d, image, n, patterns)
    if key not in _problems:
        _problems[key] = Problem(d, image, n, patterns=patterns)
    return _problems[key]
