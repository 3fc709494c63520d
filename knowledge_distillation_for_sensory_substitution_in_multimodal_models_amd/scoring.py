"""score_answers(): how likely given answers are, on the kernels generate() decodes with.

generation.py produces an answer; this module scores answers that are given: the log-probability
of every token of a candidate under teacher forcing, for a closed list of candidates per prompt
(yes / no, a colour, a count), for the gold answers of a validation split (NLL, perplexity, top-1
agreement) or for what the teacher and the student assign to the same answer.

For prompt ids x[0 .. L) and a candidate c_0 .. c_{n-1}, z_j is the bf16 logits row at position
L - 1 + j of x ++ c[:j], and entry j of the result is kd_score_rows on z_j at target c_j: the raw
logits, no repetition penalty, no n-gram ban.  The softmax runs over the full vocabulary, or with
allowed_token_ids over the allowed columns only (transformers' log-softmax behind the evaluation's
RestrictedLogitsProcessor).

The route is generate_grouped()'s with the whole prompt as the shared prefix.  A prompt is prefilled
once, whatever the number of its candidates (_prefill(): generate_batch()'s own, so z_0 has the bits
of its first returned row), and every candidate is scored on z_0 in one kd_score_rows launch with
ld_scores = 0.  Candidates of two or more tokens take a cache slot seeded with the prompt's K/V; the
rows c_0 .. c_{n-2} of up to MAX_BATCH such candidates (at most KD_GEMV_ROWS_MAX rows, across prompts)
run through the layers together (kd_gemv_rows, kd_attn_extend), every row through the final norm and
the head, and one kd_score_rows launch scores them at c_1 .. c_{n-1}.  No HIP graph (there is no loop
to replay) and no host sync beyond the prefill's; the results stay on the device.

A candidate's outputs depend on its prompt, its own tokens and the allowed set alone, bit for bit:
not on the other candidates or prompts, their order, the chunk or the slot.
"""
from __future__ import annotations

import math
import numbers
import typing

import torch

from . import ops
from ._native import KD_GEMV_ROWS_MAX
from .generation import MAX_BATCH, _Allowed, _decode_layers, _extend_rows, _final_norm, _prefill, allowed_ids


class ScoreResult(typing.NamedTuple):
    """Nested [prompt][candidate], each a 1-D device tensor of the candidate's length (with eos_token_id: + 1)."""
    logprobs: list        # fp32: log p(c_j | x ++ c[:j])
    ranks: list           # int32: tokens the greedy choice takes before c_j (0: c_j is the argmax)
    top1: list            # int64: the argmax token id of z_j (lowest id on a tie)
    top1_logprobs: list   # fp32: its log-probability
    logits: list | None = None   # return_logits: bf16 [n, V] (with a set [n, A]), the rows that were scored


class _Keep:
    """_prefill()'s chooser where nothing is chosen: the prompt's full logits row is kept."""

    def first(self, logits, seq_row, L, row):
        return logits


def _candidate(c, vocab: int, who: str) -> list:
    if isinstance(c, torch.Tensor):
        if c.dim() != 1 or c.dtype.is_floating_point or c.dtype.is_complex or c.dtype == torch.bool:
            raise ValueError(f"{who}: a 1-D tensor of integer ids expected, got {tuple(c.shape)} {c.dtype}")
        toks = c.detach().cpu().tolist()
    else:
        toks = list(c)
        if any(isinstance(t, bool) or not isinstance(t, numbers.Integral) for t in toks):
            raise ValueError(f"{who}: integer ids expected")
    if not toks:
        raise ValueError(f"{who}: an empty candidate")
    toks = [int(t) for t in toks]
    if min(toks) < 0 or max(toks) >= vocab:
        raise ValueError(f"{who}: every id must lie in [0, {vocab})")
    return toks


def _head(model, hn, allowed):
    """Final-norm rows hn [R, hidden] -> the rows scored: [R, V], or [R, A] of the allowed ids (the gathered head per
    16-row slab, or the full head's columns: the same bits)."""
    w = model.lm_head_weight()
    if allowed is not None and allowed.gather:
        slabs = [ops.gemv_batch_gather(hn[r:r + MAX_BATCH], w, allowed.ids) for r in range(0, hn.shape[0], MAX_BATCH)]
        return slabs[0] if len(slabs) == 1 else torch.cat(slabs)
    lg = ops.gemv_rows(hn, w)
    return lg if allowed is None else allowed.columns(lg)


@torch.no_grad()
def score_answers(model, prompts, answers, *, eos_token_id: int | None = None, allowed_token_ids=None,
                  restrict_head: bool | None = None, return_logits: bool = False,
                  stats: dict | None = None) -> ScoreResult:
    """The log-probabilities of candidate answers (module docstring): prompts as generate_batch() takes them, a
    sequence of (input_ids [1, L], pixel_values, image_sizes); answers one sequence of candidates per prompt, each a
    1-D int tensor or an int sequence of n >= 1 ids (at most KD_GEMV_ROWS_MAX + 1).  eos_token_id (one int) is
    appended to every candidate, so that the answer's end is scored too.  allowed_token_ids, restrict_head: as in
    generate_batch(); the softmax then runs over the allowed columns, every candidate token must be in the set, and
    top1 is a token id of the set.  return_logits: the bf16 rows that were scored.  stats (a dict) receives prefills,
    chunks, extend_rows and scored_rows.  Every ValueError comes before any device work."""
    who = "score_answers"
    prompts, answers = list(prompts), list(answers)
    if not prompts:
        raise ValueError(f"{who}: no prompts")
    if len(answers) != len(prompts):
        raise ValueError(f"{who}: {len(prompts)} prompts but {len(answers)} lists of candidates")
    vocab = int(model.cfg.text.vocab)
    if eos_token_id is not None:
        if isinstance(eos_token_id, bool) or not isinstance(eos_token_id, numbers.Integral) \
                or not 0 <= int(eos_token_id) < vocab:
            raise ValueError(f"{who}: eos_token_id must be one int in [0, {vocab}) or None")
    if allowed_token_ids is None and restrict_head is not None:
        raise ValueError(f"{who}: restrict_head is about allowed_token_ids, which is None")
    column = None   # token id -> column of the compact row
    if allowed_token_ids is not None:
        column = {t: j for j, t in enumerate(allowed_ids(allowed_token_ids, vocab).tolist())}
    cands = []
    for pi, ((ids, _, _), cs) in enumerate(zip(prompts, answers)):
        if ids.dim() != 2 or ids.shape[0] != 1:
            raise ValueError(f"{who}: every prompt's input_ids must be [1, L]")
        cs = [_candidate(c, vocab, f"{who}: prompt {pi}") for c in cs]
        if not cs:
            raise ValueError(f"{who}: prompt {pi} has no candidates")
        if eos_token_id is not None:
            cs = [c + [int(eos_token_id)] for c in cs]
        for c in cs:
            if len(c) > KD_GEMV_ROWS_MAX + 1:
                raise ValueError(f"{who}: prompt {pi}: a candidate of more than {KD_GEMV_ROWS_MAX + 1} tokens")
            if column is not None and any(t not in column for t in c):
                raise ValueError(f"{who}: prompt {pi}: a candidate token is not in allowed_token_ids")
        cands.append(cs)
    allowed = None if allowed_token_ids is None else _Allowed(model, allowed_token_ids, restrict_head, who)

    T, dev = model.cfg.text, model.device
    nkv, hd = T.kv_heads, T.head_dim
    Ls = [int(ids.shape[1]) for ids, _, _ in prompts]
    counts = {"prefills": 0, "chunks": 0, "extend_rows": 0, "scored_rows": 0}

    def targets(toks):
        return torch.tensor([t if column is None else column[t] for t in toks], dtype=torch.int32, device=dev)

    def tokens(top1):
        return top1.long() if allowed is None else allowed.cols.index_select(0, top1.long())

    def score(rows, toks):
        counts["scored_rows"] += len(toks)
        lp, rk, t1, t1lp = ops.score_rows(rows, targets(toks))
        return lp, rk, tokens(t1), t1lp

    # ---- per prompt: its prefill (once) and every candidate's first token on the prefill's row
    first = [None] * len(prompts)   # (logprob, rank, top1, top1_logprob) [candidates], and z_0
    prefix = [-1, None, None]       # the prompt prefilled last: its index and K/V [layers, HKV, L, hd]

    def prefill(upto: int):
        while prefix[0] < upto:
            pi = prefix[0] + 1
            L = Ls[pi]
            pk = torch.empty((T.layers, nkv, L, hd), dtype=torch.bfloat16, device=dev)
            pv = torch.empty_like(pk)
            seq_row = torch.empty((1, L), dtype=torch.int64, device=dev)
            z0, _ = _prefill(model, prompts[pi], pk, pv, seq_row, _Keep())
            if allowed is not None:
                z0 = allowed.columns(z0)
            first[pi] = (*score(z0, [c[0] for c in cands[pi]]), z0)
            prefix[:] = [pi, pk, pv]
            counts["prefills"] += 1

    # ---- the rows behind the first token: candidates of n >= 2 tokens, in chunks of slots and rows
    items = [(pi, ci) for pi, cs in enumerate(cands) for ci, c in enumerate(cs) if len(c) > 1]
    rest = {}   # (pi, ci) -> (logprob, rank, top1, top1_logprob, rows) of entries 1 .. n - 1
    layers = _decode_layers(model)
    i0 = 0
    while i0 < len(items):
        i1, R = i0, 0
        while i1 < len(items) and i1 - i0 < MAX_BATCH and R + len(cands[items[i1][0]][items[i1][1]]) - 1 <= KD_GEMV_ROWS_MAX:
            R += len(cands[items[i1][0]][items[i1][1]]) - 1
            i1 += 1
        chunk = items[i0:i1]
        nb = len(chunk)
        ns = [len(cands[pi][ci]) - 1 for pi, ci in chunk]   # rows per slot
        smax = max(Ls[pi] + n for (pi, _), n in zip(chunk, ns))
        kc = torch.empty((T.layers, nb, nkv, smax, hd), dtype=torch.bfloat16, device=dev)
        vc = torch.empty_like(kc)
        for b, (pi, _) in enumerate(chunk):
            prefill(pi)
            kc[:, b, :, :Ls[pi]].copy_(prefix[1])
            vc[:, b, :, :Ls[pi]].copy_(prefix[2])
        toks = torch.tensor([t for pi, ci in chunk for t in cands[pi][ci][:-1]], dtype=torch.int64, device=dev)
        x, _ = _extend_rows(model, layers, kc, vc, toks, ns, [Ls[pi] for pi, _ in chunk])   # the prompt is the prefix
        rows = _head(model, _final_norm(model, x), allowed)   # every row, not a candidate's last alone
        out = score(rows, [t for pi, ci in chunk for t in cands[pi][ci][1:]])
        lo = 0
        for key, n in zip(chunk, ns):
            rest[key] = tuple(o[lo:lo + n] for o in out) + ((rows[lo:lo + n],) if return_logits else ())   # rows: if asked for
            lo += n
        counts["chunks"] += 1
        counts["extend_rows"] += R
        i0 = i1
    prefill(len(prompts) - 1)

    # ---- per candidate: entry 0 from the prefill's row, entries 1 .. n - 1 from its slot's rows
    fields = [[[] for _ in prompts] for _ in range(5)]   # ScoreResult's, in order
    for pi, cs in enumerate(cands):
        for ci in range(len(cs)):
            more = rest.get((pi, ci))
            heads = [f[ci:ci + 1] for f in first[pi][:4]] + [first[pi][4]]
            for f in range(5 if return_logits else 4):
                fields[f][pi].append(heads[f] if more is None else torch.cat([heads[f], more[f]]))
    if stats is not None:
        stats.update(counts)
    return ScoreResult(*fields[:4], fields[4] if return_logits else None)


def pick_answers(result: ScoreResult, length_penalty: float = 1.0) -> list:
    """Per prompt (index, score) of its best candidate: score = sum(logprobs) / n ** length_penalty on the host in
    double precision, generate()'s sequences_scores convention (0: the joint log-probability, 1: the per-token mean).
    A candidate with a -inf entry scores -inf; ties go to the lower index."""
    picks = []
    for cs in result.logprobs:
        best, best_score = 0, None
        for ci, lp in enumerate(cs):
            vals = lp.detach().double().cpu().tolist()
            s = -math.inf if any(v == -math.inf for v in vals) else math.fsum(vals) / float(len(vals)) ** float(length_penalty)
            if best_score is None or s > best_score:
                best, best_score = ci, s
        picks.append((best, best_score))
    return picks
