"""The CPU reference of do_sample (generation.py, "Sampling"; include/kdstep.h, kd_gen_sample):
Philox4x32-10 in plain Python ints, the keep set and the weights in fp64 from the fp32 processed
scores, the fp64 CDF in ascending id order, and the acceptance rule for a drawn token."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
EPS = 2.0 ** -15   # acceptance: fp32 exp (<= 2 ulp), the rounding of t - max and the 2^-40 floor stay below 4e-6 of Z


def philox(counter, key):
    """Philox4x32-10: counter (4 words), key (2 words) -> 4 words."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def word0(seed: int, stream: int, pos: int) -> int:
    return philox((pos & MASK, stream & MASK, (stream >> 32) & MASK, 0), (seed & MASK, (seed >> 32) & MASK))[0]


def u_of(seed: int, stream: int, pos: int) -> float:
    """u = (word 0 >> 8) * 2^-24: exact in fp32 and in fp64."""
    return (word0(seed, stream, pos) >> 8) * 2.0 ** -24


def u_many(seed: int, streams, pos: int) -> np.ndarray:
    """u_of over an array of stream ids (numpy uint64 arithmetic, the same words)."""
    st = np.asarray(streams, dtype=np.uint64)
    m = np.uint64(MASK)
    c0 = np.full(st.shape, pos & MASK, dtype=np.uint64)
    c1, c2, c3 = st & m, st >> np.uint64(32), np.zeros(st.shape, dtype=np.uint64)
    k0, k1 = seed & MASK, (seed >> 32) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return (c0 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


class Ref:
    """processed: the fp32 processed scores of one row (oracle.generation.process_scores, -inf outside an
    allowed set, or a compact row).  -> t (fp32), keep (bool), w (fp64 weights, 0 outside keep), the CDF,
    p_margin: the smallest |mass strictly above - top_p| over the entries top-k kept, and cut_ties: how
    many entries share the lowest score top-p kept (more than one: an exact tie at the cut)."""

    def __init__(self, processed, temperature=1.0, top_k=0, top_p=1.0):
        s = np.asarray(processed, dtype=np.float32)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            t = (s / np.float32(temperature)).astype(np.float32)
        t = np.where(np.isnan(t), np.float32(-np.inf), t)
        self.t = t
        n = t.size
        keep = np.ones(n, dtype=bool)
        if 1 <= top_k < n:
            keep = t >= np.partition(t, n - top_k)[n - top_k]
        self.keep_k = keep.copy()
        mx = t.max()
        self.empty = not np.isfinite(mx) and mx < 0
        t64 = t.astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            w = np.where(keep & (t > -np.inf), np.exp(t64 - (0.0 if self.empty else float(mx))), 0.0)
        w = np.where(t == mx, 1.0, w) if not self.empty else np.zeros(n)
        w = np.where(keep, w, 0.0)
        self.p_margin, self.cut_ties = np.inf, 1
        if top_p < 1.0 and not self.empty:
            z = w.sum()
            vals, inv = np.unique(t, return_inverse=True)            # ascending
            mass = np.bincount(inv, weights=w, minlength=vals.size)   # per distinct score
            above = (np.cumsum(mass[::-1])[::-1] - mass) / z          # mass of strictly larger scores
            a = above[inv]
            self.p_margin = float(np.abs(a[keep & (w > 0)] - top_p).min())
            keep = keep & (a < top_p)
            self.cut_ties = int((t[keep] == t[keep].min()).sum())
            w = np.where(keep, w, 0.0)
        self.keep, self.w = keep, w
        self.cdf = np.cumsum(w)
        self.z = float(self.cdf[-1])

    def probs(self):
        return self.w / self.z

    def interval(self, j):
        """[C_{j-1} / Z, C_j / Z]."""
        return (float(self.cdf[j - 1]) / self.z if j > 0 else 0.0), float(self.cdf[j]) / self.z

    def token(self, u):
        """The smallest j with C_j > u * Z (token 0 for a row without a score above -inf)."""
        if self.empty:
            return 0
        j = int(np.searchsorted(self.cdf, u * self.z, side="right"))
        return min(j, int(np.nonzero(self.w > 0)[0][-1]))

    def deviation(self, j, u):
        """How far u lies outside j's interval (0: inside); inf where j has no weight."""
        if self.empty:
            return 0.0 if j == 0 else np.inf
        if not (0 <= j < self.w.size) or not self.w[j] > 0:
            return np.inf
        lo, hi = self.interval(j)
        return max(0.0, lo - u, u - hi)

    def decisive(self, u, eps=EPS):
        """u is farther than eps from both ends of the reference token's interval: one acceptable token."""
        if self.empty:
            return True
        lo, hi = self.interval(self.token(u))
        return u - lo > eps and hi - u > eps
