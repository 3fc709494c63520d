"""The CPU reference of kd_score_rows (include/kdstep.h) in NumPy float64: from one row of scores
(bf16 values, as float) and a target column, the log-softmax entry, the rank, the argmax and its
log-probability.  A NaN is dropped from the sum and counts as -inf; ties go to the lower column."""
import numpy as np

NEG = -np.inf


def score_row(row, target: int):
    """-> (logprob, rank, top1, top1_logprob) of one row [N] at column target."""
    s = np.asarray(row, dtype=np.float64).reshape(-1)
    N = s.size
    s = np.where(np.isnan(s), NEG, s)
    mx = s.max()
    dead = not mx > NEG
    lse = 0.0 if dead else mx + np.log(np.exp(s - mx).sum())
    top1 = 0 if dead else int(np.argmax(s))   # the first of the maxima
    top1_lp = NEG if dead else mx - lse
    t = int(target)
    if not 0 <= t < N:
        return NEG, N, top1, top1_lp
    st = s[t]
    rank = int(np.sum(s > st) + np.sum(s[:t] == st))
    lp = NEG if dead or not st > NEG else st - lse
    return float(lp), rank, top1, float(top1_lp)


def score_rows(rows, targets):
    """rows [R, N] (or [1, N] / [N] for every target) -> four arrays [len(targets)]."""
    rows = np.asarray(rows, dtype=np.float64)
    rows = rows.reshape(1, -1) if rows.ndim == 1 else rows
    out = [score_row(rows[r if rows.shape[0] > 1 else 0], t) for r, t in enumerate(targets)]
    lp, rk, t1, t1lp = zip(*out)
    return np.array(lp), np.array(rk, dtype=np.int64), np.array(t1, dtype=np.int64), np.array(t1lp)
