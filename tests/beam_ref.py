"""The CPU reference of num_beams > 1 (generation.py, "Beam search"; include/kdstep.h, kd_gen_beam_topk /
kd_gen_beam_step): transformers 5.x GenerationMixin._beam_search with do_sample=False, early_stopping=False and
one returned sequence, for one prompt, in NumPy float64, fed by a logits_fn.  test_generate_beams.py checks it
against transformers' own generate(num_beams=...).

Precision.  Log-probabilities and scores are float64 here and fp32 in the kernels (and in transformers).  Where
fp32 *absorbs* -- a value next to the kill score -1e9, whose fp32 spacing is 64 -- the reference takes what fp32
gives (_kill, and the accumulated score of a killed beam): those values tie exactly on both sides and the tie
rules settle them, so they never count towards a margin.  Everything else differs from fp32 by rounding alone.

EPS: the bound on |kernel fp32 - reference float64| of an accumulated (or length-normalised) score, derived from
fp32 rounding under the magnitudes the reference itself enforces (search(check_bounds=True) raises outside them):
|score| < S_MAX = 512, |log-probability| and |lse| < L_MAX = 64, penalty <= P_MAX = 2, at most STEPS = 32 steps.
With U_S = ulp32 below 512 = 2^-15 and U_L = ulp32 below 64 = 2^-18, one step adds at most
  lse: the fixed-point sum (expf within 2 ulp relative, truncation V * 2^-40 <= 2^-22: together < 2^-21 on
       log Z), the cast of log Z <= 12.5 to fp32 (2^-21) and the rounding of max + log Z (U_L / 2) ..... <= 1.0 U_L
  l = s - lse, one rounding ........................................................................... 0.5 U_L
  the penalty l * p: p times the 1.5 U_L above, and one rounding below 128 (ulp 2 U_L) ............. (1.5 p + 1) U_L
  acc = l + running score, one rounding below 512 ..................................................... 0.5 U_S
and the division by den once at the end adds den's own rounding (2^-24 relative of < 512: U_S) and the quotient's
(U_S / 2).  EPS = 32 * (U_S / 2 + (1.5 * 2 + 1) U_L) + 1.5 U_S = 1.02e-3.  It is derived, not fitted: a GPU result
outside it is a finding about the kernel.

Tie rules (ours: torch.topk leaves ties unspecified, so transformers has none to follow).  Candidates: larger
score, then lower beam, then lower token.  Running beams: larger r, then lower candidate rank.  Finished set:
larger score, then the earlier entry of (stored hypotheses ++ candidates).  An entry at -inf carries token 0.

Margins.  search() returns the smallest gap met at any decision: the M / M+1 cut and neighbours inside the top M,
the running cut and its neighbours, every finished-set comparison, and best against every worst_k.  A pair that is
an exact tie of one beam (same logit, same flags: bit-identical on both sides) or that sits at the kill score on
both sides is settled by the tie rule and does not count.
"""
import numpy as np

KILL = -1.0e9
F32 = np.float32
S_MAX, L_MAX, P_MAX, STEPS = 512.0, 64.0, 2.0, 32
U_S, U_L = 2.0 ** -15, 2.0 ** -18
assert float(np.spacing(F32(511.0))) == U_S and float(np.spacing(F32(63.0))) == U_L
EPS = STEPS * (0.5 * U_S + (1.5 * P_MAX + 1.0) * U_L) + 1.5 * U_S
assert 1.0e-3 < EPS < 1.1e-3
DEAD = -1.0e8   # at or below: a killed value (fp32 has absorbed whatever was added to -1e9)


def _kill(x):
    """x + -1e9 as fp32 gives it (the spacing there is 64: x is absorbed), in either precision."""
    return float(F32(F32(x) + F32(KILL)))


def _gap(a, b):
    """The margin a comparison of a and b has; inf where the tie rule settles it on both sides."""
    if (a <= DEAD and b <= DEAD) or (a == b and np.isinf(a)):
        return np.inf
    return abs(a - b)


def log_probs(row, seq, penalty=1.0, ngram=0, allowed=None):
    """One beam's processed log-probabilities: row [V] logits (any float dtype; NaN counts as -inf), seq = its ids
    so far -> (l [V] float64, flags [V] uint8: 1 = seen, 2 = banned, 4 = allowed).  log-softmax over the full
    row, then the repetition penalty (float32(penalty), as the kernels hold it) and the n-gram ban on the
    log-probabilities, then -inf outside `allowed`."""
    s = np.asarray(row, dtype=np.float64)
    V = s.shape[0]
    flags = np.zeros(V, dtype=np.uint8)
    ok = ~np.isnan(s)
    if not ok.any() or not s[ok].max() > -np.inf:
        return np.full(V, -np.inf), flags
    mx = s[ok].max()
    lse = mx + np.log(np.exp(s[ok] - mx).sum())
    l = np.where(ok, s - lse, -np.inf)
    seq = [int(t) for t in seq]
    if penalty != 1.0:
        ids = np.unique(np.array([t for t in seq if 0 <= t < V], dtype=np.int64))
        p = float(F32(penalty))
        l[ids] = np.where(l[ids] < 0, l[ids] * p, l[ids] / p)
        flags[ids] |= 1
    n = len(seq)
    if ngram > 0 and n + 1 >= ngram:
        prefix = tuple(seq[n - ngram + 1:])
        for i in range(0, n - ngram + 1):
            if tuple(seq[i:i + ngram - 1]) == prefix and 0 <= seq[i + ngram - 1] < V:
                l[seq[i + ngram - 1]] = -np.inf
                flags[seq[i + ngram - 1]] |= 2
    if allowed is not None:
        keep = np.zeros(V, dtype=bool)
        keep[np.asarray(list(allowed), dtype=np.int64)] = True
        l[~keep] = -np.inf
        flags[keep] |= 4
    return l, flags


def accumulate(l, run_score):
    """acc = l + run_score; a killed beam's as fp32 gives it."""
    if run_score <= DEAD:
        return (l.astype(F32) + F32(run_score)).astype(np.float64)
    return l + run_score


def _top(flat, n):
    """Indices of the n largest of flat, descending, the lower index first among equals (flat holds no NaN)."""
    idx = np.arange(flat.shape[0])
    if flat.shape[0] > n:   # everything at or above the n-th largest value, ties included, then the full order of those
        idx = np.nonzero(flat >= np.partition(flat, flat.shape[0] - n)[flat.shape[0] - n])[0]
    return idx[np.lexsort((idx, -flat[idx]))][:n]


def row_top(acc, M):
    """The M best (score, token) of one row, descending, the lower token first among equals, an entry at -inf
    as (-inf, 0) -> (scores [M], tokens [M], the (M+1)-th score or -inf)."""
    order = _top(acc, M + 1)
    sc = [float(acc[i]) for i in order] + [-np.inf] * (M + 1 - len(order))
    tk = [int(i) if acc[i] > -np.inf else 0 for i in order] + [0] * (M + 1 - len(order))
    return sc[:M], tk[:M], sc[M]


def candidates(rows, run_seq, run_score, M, penalty=1.0, ngram=0, allowed=None):
    """The M largest accumulated scores over (beam, token), descending; ties: lower beam, then lower token ->
    (list of (score, beam, token), margin, the largest |log-probability| and |score| among them)."""
    rows = np.asarray(rows)
    K, V = rows.shape
    acc, flags = np.empty((K, V)), np.empty((K, V), dtype=np.uint8)
    for j in range(K):
        l, flags[j] = log_probs(rows[j], run_seq[j], penalty, ngram, allowed)
        acc[j] = accumulate(l, run_score[j])
    flat = acc.ravel()
    order = _top(flat, M + 1)   # index = beam * V + token: the lower beam, then the lower token
    # the 4th field names what is bit-identical on both sides: same beam, same logit, same flags
    cand = [(float(flat[i]), int(i // V), int(i % V) if flat[i] > -np.inf else 0,
             (int(i // V), float(rows[i // V, i % V]), int(flags[i // V, i % V]))) for i in order[:M]]
    while len(cand) < M:
        cand.append((-np.inf, K - 1, 0, None))
    margin = np.inf
    for a, b in zip(order[:-1], order[1:]):
        ja, ta, jb, tb = a // V, a % V, b // V, b % V
        same = ja == jb and flags[ja, ta] == flags[jb, tb] and (rows[ja, ta] == rows[jb, tb] or flat[a] == -np.inf)
        if not same:
            margin = min(margin, _gap(float(flat[a]), float(flat[b])))
    fin = [c[0] for c in cand if c[0] > DEAD]
    big_l = max((abs(c[0] - run_score[c[1]]) for c in cand if c[0] > DEAD), default=0.0)
    return cand, margin, big_l, max((abs(v) for v in fin), default=0.0)


class State:
    """One prompt's search: the running beams, the finished store and the heuristic's flag."""

    def __init__(self, prompt, K):
        self.K, self.L, self.cur = K, len(prompt), len(prompt)
        self.run_seq = [list(prompt) for _ in range(K)]
        self.run_score = [0.0] + [KILL] * (K - 1)
        self.fin = [(KILL, False, list(prompt)) for _ in range(K)]   # (score, flag, sequence)
        self.unsat, self.done = True, False


def den_table(max_new, length_penalty):
    """den[g] = float32(g ** length_penalty), g ** length_penalty in Python double."""
    return [1.0] + [float(F32(float(g) ** length_penalty)) for g in range(1, max_new + 1)]


def advance(st, cand, eos, max_len, den, ft=np.float64):
    """Everything of a step behind the candidates (kd_gen_beam_step) -> (parents, tokens, margin).  ft = np.float32
    rounds every operation as the kernel does (bit for bit on the same candidates)."""
    K, M, L = st.K, len(cand), st.L
    f = lambda x: float(ft(x))
    cand = [tuple(c) + (None,) * (4 - len(c)) for c in cand]   # (score, beam, token[, twin class])
    twin = [None] * K + [c[3] for c in cand]

    def gap(va, vb, ia, ib):   # candidates that are exact ties of one beam stay tied through every later value
        return np.inf if twin[ia] is not None and twin[ia] == twin[ib] else _gap(va, vb)

    hit = [tok in eos or st.cur + 1 >= max_len for _, _, tok, _ in cand]
    r = [_kill(s) if h else f(s) for (s, _, _, _), h in zip(cand, hit)]
    order = sorted(range(M), key=lambda c: (-r[c], c))
    margin = min([gap(r[a], r[b], K + a, K + b) for a, b in zip(order[:K], order[1:K + 1])], default=np.inf)
    dn = den[st.cur + 1 - L]
    items = list(st.fin)
    for c, (s, j, tok, _) in enumerate(cand):
        just = hit[c] and c < K
        q = f(f(f(s) / f(dn)) + 0.0)
        items.append((q if just else _kill(q), just, st.run_seq[j] + [tok]))
    forder = sorted(range(K + M), key=lambda i: (-items[i][0], i))
    margin = min([margin] + [gap(items[a][0], items[b][0], a, b) for a, b in zip(forder[:K], forder[1:K + 1])])
    parents = [cand[c][1] for c in order[:K]]
    tokens = [cand[c][2] for c in order[:K]]
    st.run_seq = [st.run_seq[cand[c][1]] + [cand[c][2]] for c in order[:K]]
    st.run_score = [r[c] for c in order[:K]]
    st.fin = [items[i] for i in forder[:K]]
    st.cur += 1
    best = f(f(st.run_score[0]) / f(den[st.cur - L]))
    low = min(s for s, _, _ in st.fin)
    worst = [low if flag else KILL for _, flag, _ in st.fin]
    margin = min([margin] + [_gap(best, w) for w in worst])
    st.unsat = st.unsat and any(best > w for w in worst)
    st.done = not st.unsat or all(hit)
    return parents, tokens, margin


def search(logits_fn, prompt, K, eos=(), max_new=10, penalty=1.0, ngram=0, length_penalty=1.0, allowed=None,
           check_bounds=True):
    """logits_fn(run_seq: K id lists, step) -> [K, V] logits.  -> dict(seq, score, margin, steps, on_eos, trace:
    per step (parents, tokens, running scores), done_at)."""
    eos = {int(e) for e in eos}
    M = max(2, 1 + len(eos)) * K
    st = State([int(t) for t in prompt], K)
    den = den_table(max_new, length_penalty)
    margin, trace = np.inf, []
    if check_bounds and (max_new > STEPS or penalty > P_MAX):
        raise ValueError("beam_ref: outside the magnitudes EPS is derived for")
    while not st.done:
        rows = logits_fn([list(s) for s in st.run_seq], st.cur - st.L)
        cand, m, big_l, big_s = candidates(rows, st.run_seq, st.run_score, M, penalty, ngram, allowed)
        if check_bounds and (big_l >= L_MAX or big_s >= S_MAX):
            raise ValueError("beam_ref: outside the magnitudes EPS is derived for")
        parents, tokens, m2 = advance(st, cand, eos, st.L + max_new, den)
        margin = min(margin, m, m2)
        trace.append((parents, tokens, list(st.run_score)))
    score, flag, seq = st.fin[0]
    assert flag
    return dict(seq=seq, score=score, margin=margin, steps=len(trace), trace=trace,
                on_eos=seq[-1] in eos and len(seq) < st.L + max_new)
