"""Student generate(): prefill + KV-cache greedy decode on the HIP kernels.

Drop-in for the call the reference's evaluation makes on the trained student
(evaluation/onevisionv3/evaluate_onevision.py:185-195):

    model.generate(**inputs, max_new_tokens=32, pad_token_id=pad_token_id,
                   repetition_penalty=1.2, no_repeat_ngram_size=2, temperature=0.7)

`do_sample` is not set there, so decoding is greedy and `temperature` has no effect (transformers
only applies it when sampling; with do_sample=True see "Sampling" below).  The prompt runs through the same forward as training
(LlavaOnevisionModel.forward: SigLIP, projector, anyres pack, Qwen2), whose roped keys and values
seed a per-layer KV cache [HKV, L + max_new_tokens, hd]; each new token then runs one row through
every layer (kd_gemv with the RMSNorms fused in front and bias / residual / SwiGLU epilogues, kd_qkv_split with its
RoPE row, split-KV kd_attn_decode) and kd_gen_select picks it on the device.  The position lives in a device counter, so
every launch of a step has fixed arguments: the first step runs eagerly, the step is captured
once as a HIP graph (torch.cuda.CUDAGraph) and replayed for the rest.  kd_gen_finish, the last
launch of the step, keeps on the device which rows have emitted an EOS; the loop reads that count
every STOP_CHECK_EVERY steps (one 4-byte copy and an event wait between two replays) and ends once
every row has, and the few steps past a row's EOS are discarded afterwards, so the result does
not depend on how often it looks.  Returns prompt + generated ids like transformers' generate
(B = 1, as the evaluation runs it).

generate_batch() decodes up to 16 such prompts per step (ragged lengths, per-row device counters,
batch-invariant kernels): the evaluation's one-question-at-a-time loop with the weights streamed
once per step for all rows.

generate_grouped() takes the questions grouped by image, as the evaluation's prompts are laid out
(image first, then the question): the SigLIP tower, the projector and every layer's K/V up to the
last image token depend on the image alone, so that prefix is prefilled once per image and copied
into the cache of each of its questions; the ragged question suffixes of a chunk then run through
the layers together (kd_gemv_rows: the decode GEMV for more than 16 rows without reading the
weights again per 16 rows; kd_attn_extend: suffix queries against prefix + own suffix) and the
batched decode of generate_batch() takes over.  A question's result depends on its image, the
shared prefix and its own suffix only (bit for bit); it is held to generate_batch()'s oracle
bounds but is not bit-identical to generate_batch() on the same prompt.

Constrained decoding.  The evaluation restricts the choice to the tokens of its answers table
(evaluate_onevision.py:141-158: a user logits processor that adds 0 to the allowed ids and -inf to
every other id, which transformers runs behind its own processors).  All three entry points take
that set as allowed_token_ids (any int sequence or int tensor; allowed_ids() sorts and deduplicates
it once, before the graph capture, and raises ValueError for an empty set, an id outside
[0, vocab) or more than KD_GEN_ALLOWED_MAX ids, before any device work); None is the unrestricted
call, launch for launch.  With a set:
  - the mask comes after the repetition penalty and the no-repeat-n-gram ban; the token is the
    allowed id with the largest processed fp32 score, the lowest id on a tie, never a NaN;
  - the penalty applies to an allowed id that occurs in the sequence (prompt or generated); ids of
    the sequence that are not allowed matter as n-gram context only;
  - if every allowed id is banned (or -inf / NaN) the token is 0, allowed or not: the argmax of an
    all -inf row, the unrestricted kernels' rule;
  - a row ends only if an EOS id is in the set and is chosen; otherwise it runs max_new_tokens;
  - return_logits gives compact bf16 rows [1, A]: column j is the logit of the j-th smallest allowed
    id (the order of allowed_ids()), bit-identical to the full row's element at that id.
The prefill's token comes from the full logits row's allowed columns (generate_grouped(): from the
gathered head behind its extend pass).  A decode step reads only the A allowed rows of the lm_head
(kd_gemv_gather / kd_gemv_batch_gather) and searches A scores (kd_gen_select_ids: flags per allowed
entry, sequence tokens found by binary search) where ops.gemv_gather_supported(vocab, hidden) holds;
elsewhere, or with restrict_head=False, it runs the full head and takes the allowed columns: the
same bits either way.  restrict_head=True raises ValueError where the gathered head does not exist.

Sampling.  do_sample=True (default False: the greedy call, launch for launch; temperature, top_k,
top_p, seed and sample_streams are then ignored, as transformers ignores its warpers) draws every
token of a row with kd_gen_sample in place of the select: the prefill's token, the token behind
generate_grouped()'s extend pass and every decode step inside the captured graph, behind the same
gathered head or full-head columns when allowed_token_ids is given.  It is transformers' _sample
made reproducible.  Per row and step:
  1. the processed fp32 scores of the greedy kernels: repetition penalty, n-gram ban, and with
     allowed_token_ids every other id at -inf;
  2. t = s / temperature in fp32 (None: 1.0; must be > 0);
  3. top_k >= 1 keeps every entry with t >= the k-th largest t, ties at that value included, as
     TopKLogitsWarper; top_k >= the row's width keeps everything, 0 is off;
  4. top_p < 1: with p = softmax(t) over what top-k kept, an entry is kept iff the entries with a
     strictly larger score have mass < top_p.  That is TopPLogitsWarper's set whenever no two scores
     at the cut are exactly equal; equal scores are kept or dropped together here, where
     transformers' result depends on its sort order.  The largest entry is always kept;
  5. w = exp(t - max t) on what is kept, Z = sum w, and the token is the smallest id whose inclusive
     cumulative weight (ascending ids) exceeds u * Z; an entry of weight 0 (dropped, banned, -inf,
     NaN) is never chosen, and a row without a score above -inf gives token 0;
  6. u = (x >> 8) * 2^-24 with x the first word of Philox4x32-10 under key (seed & 0xffffffff,
     seed >> 32) at counter (pos, stream & 0xffffffff, stream >> 32, 0): pos is the index in the
     row's sequence the token is written to, stream the row's entry of sample_streams.
So a row's tokens are a function of its prompt, the decode settings, seed and its own stream: not of
the batch it sits in, its slot, the chunking, graph, stop_check_every or the head taken.  seed: an
int in [0, 2^64); None draws one from torch's default CPU generator (torch.manual_seed governs it)
and stats["seed"] reports it.  sample_streams: one int in [0, 2^63) per prompt (generate(): one int
or a one-element sequence); the default is the prompt's index in the call (generate_grouped(): in
the flattened question order; generate(): 0), so row r alone with sample_streams=[r] reproduces row
r of the batch.  A bad temperature, top_k, top_p, seed or sample_streams raises ValueError before any
device work.  return_logits gives the raw rows, as in the greedy call.

Beam search.  num_beams = K > 1 (default 1: today's call, launch for launch and bit for bit; length_penalty and
early_stopping are then ignored) is transformers 5.x GenerationMixin._beam_search with do_sample=False,
early_stopping=False and one returned sequence, per prompt; prompts never interact.  With L the prompt's length, E
the EOS ids, M = max(2, 1 + |E|) * K, max_len = L + max_new_tokens and den[g] = float32(g ** length_penalty):

    run_seq[K] = prompt; run_score = [0, -1e9, ...] (fp32); fin_score[K] = -1e9; fin_flag[K] = False
    unsat = True; cur = L
    loop:
      for beam j: l = log_softmax(fp32(logits_j)) over the FULL vocabulary
                  l = no-repeat-ngram(repetition_penalty(l))   # on log-probs (l < 0: l * p), over run_seq[j]
                  l = -inf outside allowed_token_ids (if given)
                  acc_j = l + run_score[j]                       (fp32)
      cand[0..M) = the M largest of acc over (j, token), descending; ties: lower j, then lower token
      seq_c = run_seq[j_c] + [tok_c];  hit_c = tok_c in E  or  cur + 1 >= max_len
      running: r_c = score_c + (hit_c ? -1e9 : 0) (fp32); the K largest r (ties: lower c) become run_seq / run_score
      finished: just_c = hit_c and c < K
                f_c = score_c / den[cur + 1 - L] + (unsat ? 0 : -1e9) + (just_c ? 0 : -1e9)   (fp32, in this order)
                fin = the K largest of (fin ++ cands) by score; ties: earlier in that concatenation; the flag travels
      cur += 1
      best = run_score[0] / den[cur - L];  worst_k = fin_flag[k] ? min(fin_score) : -1e9
      unsat = unsat and any_k(best > worst_k)
      stop when not unsat, or when every one of the M candidates was a hit
    result: fin_seq[0] (its EOS included if it ended on one), sequences_score = fin_score[0]

torch.topk leaves ties unspecified; the tie rules above are this project's.  A NaN logit counts as -inf, and a
candidate at -inf carries token 0.  A prompt whose search has stopped is closed: its finished set never changes
again, and what its rows hold afterwards is unspecified.  tests/beam_ref.py restates this in NumPy and is checked
against transformers' own generate(num_beams=...).
  - Rows are beams: a chunk holds MAX_BATCH // K prompts (questions for generate_grouped()) in slots p * K + j.  Each
    prompt is prefilled once, exactly as without beams; its cache, ids and logits row are copied into its K rows (the
    first choice sees K equal rows, and run_score kills beams 1 .. K - 1).  generate_grouped() runs its extend pass
    once per question and copies the suffix K/V along.  generate(num_beams=K) takes the batched route and is
    generate_batch([prompt], num_beams=K)[0], bit for bit (fuse_norm does not apply there).
  - A step is the batched decode step with three launches in place of the select: kd_gen_beam_topk (per row the M
    best accumulated log-probabilities), kd_gen_beam_step (per prompt: the candidates, the running and the finished
    hypotheses, the reorder of the ids by parent, the heuristic) and kd_kv_beam_reorder (the generated tail of the
    K/V cache permuted by parent), all with fixed arguments, so the step still replays from one captured graph.
    max_new_tokens * K <= 4096 (kd_gen_beam_step stages the generated windows in LDS; ValueError otherwise).
  - allowed_token_ids works, but the full head always runs (the log-softmax is over the whole vocabulary, as
    transformers computes it before the user's mask); restrict_head=True raises ValueError.  So do do_sample=True,
    early_stopping other than False, a length_penalty that is not finite, num_beams outside [1, KD_GEN_BEAMS_MAX] and
    more than KD_GEN_EOS_MAX EOS ids, all before any device work.
  - The early stop reads one int32, the number of prompts still open, which kd_gen_beam_step writes; it is active
    whenever stop_check_every > 0 (the heuristic needs no EOS id).  steps_run / checks as without beams;
    finished_at is the returned length.
  - stats additionally receives, per chunk: sequences_scores (one float per prompt: fin_score[0]) and the replay
    trace beam_tokens, beam_parents, beam_scores: per choice (the prefill's first) a [prompts][K] nest of the tokens
    appended, the parent beam (0 .. K - 1) of each new beam and the running scores.  Entries of a prompt behind the
    choice that closed it are unspecified.  The trace costs three small device copies per step (between two
    replays, no host sync), made only when stats is given: the step times of profiles/generate_beams are without.
  - return_logits gives, per prompt, one [K, V] bf16 tensor per choice of its chunk: the rows that fed that choice
    (the first: K copies of the prefill's row); those behind the prompt's last choice are unspecified.
  - A prompt's tokens and score do not depend on the other prompts of the call, on its slot, on the chunking, on
    graph or on stop_check_every.
"""
from __future__ import annotations

import copy
import dataclasses
import typing

import torch

from . import ops
from ._native import KD_GEMV_ROWS_MAX, KD_GEN_ALLOWED_MAX, KD_GEN_BEAMS_MAX, KD_GEN_EOS_MAX


EOS_TOKEN_IDS = (151645,)   # <|im_end|>: generation_config.eos_token_id of the -ov-hf chat checkpoints


FUSE_NORM_DEFAULT = True   # RMSNorm fused into the decode GEMVs (generate(fuse_norm=False): the A/B route)


# decode steps between two host reads of the rows still running (0: never stop early).  Measured
# (profiles/generate_stop/bench.txt): a read costs < 0.1 ms, a step 1.2 - 1.6 ms, so every step wins
STOP_CHECK_EVERY = 1


def _stop_every(stop_check_every, who: str) -> int:
    k = STOP_CHECK_EVERY if stop_check_every is None else int(stop_check_every)
    if k < 0:
        raise ValueError(f"{who}: stop_check_every must be >= 0")
    return k


def _stats_begin(stats):
    if stats is not None:
        for key in ("steps_run", "steps_max", "checks", "finished_at"):
            stats[key] = []


class _Stop:
    """The early stop of one decode loop: kd_gen_finish keeps, on the device, every row's length at
    its first EOS (fin) and the number of rows still running (live); the loop reads live every k
    steps and ends once it is 0.  Inactive (k = 0, no EOS id, or more ids than kd_gen_finish takes)
    it launches and reads nothing: the loop is then the plain max_new_tokens one.  With beams (a
    _BeamRows) live is the number of prompts still open, which kd_gen_beam_step itself writes: mark()
    launches nothing, and the stop is active whenever k > 0 (the heuristic needs no EOS id)."""

    def __init__(self, model, nb: int, eos, k: int, beam=None):
        self.k, self.checks, self.beam = k, 0, beam
        self.ids = sorted(eos)
        self.active = k > 0 and (beam is not None or 0 < len(self.ids) <= KD_GEN_EOS_MAX)
        if not self.active:
            return
        dev = model.device
        if beam is None:
            self.fin = torch.zeros(nb, dtype=torch.int32, device=dev)
            self.live = torch.zeros(1, dtype=torch.int32, device=dev)
        else:
            self.live = beam.live[:1]
        cached = getattr(model, "_gen_stop_host", None)   # one pinned word and its event per model
        if cached is None:
            cached = (torch.zeros(1, dtype=torch.int32).pin_memory(), torch.cuda.Event())
            model._gen_stop_host = cached
        self.host, self.event = cached

    def mark(self, tok, cur):
        """Behind a select (also inside the captured step: its arguments never change)."""
        if self.active and self.beam is None:
            ops.gen_finish(tok, cur, self.ids, self.fin, self.live)

    def done(self, ran: int, n_steps: int) -> bool:
        """After `ran` of n_steps steps, between two replays: has every row ended?  One 4-byte copy
        and a wait on its own event (no device-wide synchronize: other streams keep running)."""
        if not self.active or ran % self.k or ran >= n_steps:
            return False
        self.checks += 1
        self.host.copy_(self.live, non_blocking=True)
        self.event.record()
        self.event.synchronize()
        return int(self.host[0]) == 0

    def ends(self):
        """Per row the length at its first EOS (0: none), or None when inactive."""
        return self.fin.tolist() if self.active else None


def _stats_chunk(stats, ran, n_steps, checks, finished_at):
    if stats is not None:
        stats["steps_run"].append(ran)
        stats["steps_max"].append(n_steps)
        stats["checks"].append(checks)
        stats["finished_at"].append(finished_at)


def _eos_set(eos_token_id) -> set:
    return {int(e) for e in ([eos_token_id] if isinstance(eos_token_id, int) else (eos_token_id or ()))}


def allowed_ids(allowed_token_ids, vocab: int) -> torch.Tensor:
    """allowed_token_ids (any sequence of ints or an integer tensor, any order, repeats welcome) as
    the kernels take them: a sorted, unique int32 tensor on the host.  ValueError for an empty set,
    an id outside [0, vocab), more than KD_GEN_ALLOWED_MAX distinct ids or anything but integers.
    Touches no device."""
    t = allowed_token_ids.detach().cpu() if isinstance(allowed_token_ids, torch.Tensor) \
        else torch.tensor(list(allowed_token_ids))
    if t.numel() == 0:
        raise ValueError("allowed_token_ids: the set is empty")
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise ValueError(f"allowed_token_ids: integer ids expected, got {t.dtype}")
    t = torch.unique(t.reshape(-1).to(torch.int64))   # sorted ascending
    if int(t[0]) < 0 or int(t[-1]) >= int(vocab):
        raise ValueError(f"allowed_token_ids: every id must lie in [0, {int(vocab)})")
    if t.numel() > KD_GEN_ALLOWED_MAX:
        raise ValueError(f"allowed_token_ids: more than {KD_GEN_ALLOWED_MAX} ids")
    return t.to(torch.int32)


class _Allowed:
    """The allowed set of one call, normalised once (before the graph capture: the step's arguments
    stay fixed): ids ascending on the device, and which head the decode step takes.  gather: only the
    allowed rows of the lm_head are read (kd_gemv_gather / kd_gemv_batch_gather); else the full head
    runs and its allowed columns are taken.  Both give the same bits."""

    def __init__(self, model, allowed_token_ids, restrict_head, who: str):
        T = model.cfg.text
        host = allowed_ids(allowed_token_ids, T.vocab)
        supported = ops.gemv_gather_supported(T.vocab, T.hidden)
        if restrict_head and not supported:
            raise ValueError(f"{who}: restrict_head=True, but the gathered head does not exist for a "
                             f"[{T.vocab}, {T.hidden}] lm_head (ops.gemv_gather_supported)")
        self.gather = supported if restrict_head is None else bool(restrict_head)
        self.ids = host.to(model.device)
        self.cols = self.ids.long()

    def columns(self, logits):
        """Full logits [nb, V] -> their allowed columns [nb, A], ascending ids."""
        return logits.index_select(1, self.cols)


def _allowed(model, allowed_token_ids, restrict_head, who: str):
    if allowed_token_ids is None:
        if restrict_head is not None:
            raise ValueError(f"{who}: restrict_head is about allowed_token_ids, which is None")
        return None
    return _Allowed(model, allowed_token_ids, restrict_head, who)


class _Sampler:
    """The sampling settings of one call (do_sample=True), validated once, before any device work:
    temperature, top_k, top_p, the seed and one Philox stream id per prompt of the call.  rows(lo, hi)
    of the chooser puts a chunk's stream ids on the device, fixed for the captured step."""

    def __init__(self, temperature, top_k, top_p, seed, sample_streams, n_rows: int, who: str):
        import math
        import numbers
        t = 1.0 if temperature is None else temperature
        if isinstance(t, bool) or not isinstance(t, numbers.Real) or not math.isfinite(t) or t <= 0:
            raise ValueError(f"{who}: temperature must be a finite number > 0, got {temperature!r}")
        if isinstance(top_k, bool) or not isinstance(top_k, numbers.Integral) or top_k < 0:
            raise ValueError(f"{who}: top_k must be an int >= 0 (0: off), got {top_k!r}")
        if isinstance(top_p, bool) or not isinstance(top_p, numbers.Real) or not 0.0 < top_p <= 1.0:
            raise ValueError(f"{who}: top_p must lie in (0, 1], got {top_p!r}")
        if seed is not None and (isinstance(seed, bool) or not isinstance(seed, numbers.Integral)
                                 or not 0 <= seed < 1 << 64):
            raise ValueError(f"{who}: seed must be an int in [0, 2^64) or None, got {seed!r}")
        if sample_streams is None:
            streams = list(range(n_rows))
        else:
            streams = [sample_streams] if isinstance(sample_streams, numbers.Integral) else list(sample_streams)
            if len(streams) != n_rows:
                raise ValueError(f"{who}: sample_streams must hold one stream id per prompt ({n_rows}), "
                                 f"got {len(streams)}")
            for v in streams:
                if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= v < 1 << 63:
                    raise ValueError(f"{who}: every sample_streams entry must be an int in [0, 2^63), got {v!r}")
        if seed is None:   # torch's default CPU generator: torch.manual_seed governs it
            lo, hi = torch.randint(0, 1 << 32, (2,), dtype=torch.int64).tolist()
            seed = hi << 32 | lo
        self.temperature, self.top_k, self.top_p = float(t), min(int(top_k), 2 ** 31 - 1), float(top_p)
        self.seed, self.streams = int(seed), [int(v) for v in streams]


BEAM_KILL = -1.0e9   # transformers' score of a beam that must not be chosen
BEAM_WINDOW = 4096   # include/kdstep.h, kd_gen_beam_step: K * max_new, the generated windows it stages in LDS


class _Beams:
    """The beam-search settings of one call (num_beams > 1), validated once, before any device work (_beams())."""

    def __init__(self, num_beams: int, length_penalty: float, eos: set):
        self.K, self.length_penalty, self.eos = num_beams, float(length_penalty), sorted(eos)
        self.M = max(2, 1 + len(self.eos)) * num_beams   # candidates per step, as transformers takes them

    def den(self, max_new: int) -> list:
        """den[g] = g ** length_penalty (Python double; the kernel holds it as fp32), g = 0 unused."""
        return [1.0] + [float(g) ** self.length_penalty for g in range(1, max_new + 1)]


def _beams(who: str, num_beams, length_penalty, early_stopping, do_sample, restrict_head, eos_token_id, max_new_tokens):
    """num_beams == 1 -> None (the other two arguments are ignored); else the call's _Beams, or ValueError."""
    import math
    import numbers
    if isinstance(num_beams, bool) or not isinstance(num_beams, numbers.Integral) \
            or not 1 <= num_beams <= KD_GEN_BEAMS_MAX:
        raise ValueError(f"{who}: num_beams must be an int in [1, {KD_GEN_BEAMS_MAX}], got {num_beams!r}")
    if num_beams == 1:
        return None
    if isinstance(length_penalty, bool) or not isinstance(length_penalty, numbers.Real) \
            or not math.isfinite(length_penalty):
        raise ValueError(f"{who}: length_penalty must be a finite number, got {length_penalty!r}")
    if early_stopping is not False:
        raise ValueError(f"{who}: early_stopping must be False (True and 'never' are not built), got {early_stopping!r}")
    if do_sample:
        raise ValueError(f"{who}: num_beams > 1 with do_sample=True (beam sampling) is not built")
    if restrict_head:
        raise ValueError(f"{who}: num_beams > 1 runs the full head (the log-softmax is over the whole vocabulary): "
                         f"restrict_head=True cannot hold")
    eos = _eos_set(eos_token_id)
    if len(eos) > KD_GEN_EOS_MAX:
        raise ValueError(f"{who}: num_beams > 1 takes at most {KD_GEN_EOS_MAX} EOS ids, got {len(eos)}")
    if int(max_new_tokens) * int(num_beams) > BEAM_WINDOW:
        raise ValueError(f"{who}: num_beams > 1 needs max_new_tokens * num_beams <= {BEAM_WINDOW} (kd_gen_beam_step stages "
                         f"the generated windows in LDS), got {int(max_new_tokens)} * {int(num_beams)}")
    return _Beams(int(num_beams), length_penalty, eos)


class _BeamRows:
    """The device state of one chunk's beam search: rows p * K + j are the beams of prompt p.  choose() is the
    step behind the head: kd_gen_beam_topk, kd_gen_beam_step, kd_kv_beam_reorder, every argument fixed."""

    def __init__(self, beams: _Beams, model, processors, allowed, seq, Ls, max_new: int, kc, vc, trace: bool):
        dev, K, P = model.device, beams.K, len(Ls)
        nb = P * K
        self.beams, self.K, self.P, self.Ls, self.max_new, self.kc, self.vc = beams, K, P, list(Ls), max_new, kc, vc
        self.processors, self.ids = processors, None if allowed is None else allowed.ids
        self.run_score = torch.tensor(([0.0] + [BEAM_KILL] * (K - 1)) * P, dtype=torch.float32, device=dev)
        self.fin_seq = seq.clone()   # the prompts below every hypothesis
        self.fin_score = torch.full((nb,), BEAM_KILL, dtype=torch.float32, device=dev)
        self.fin_len = torch.zeros(nb, dtype=torch.int32, device=dev)
        self.open = torch.ones(P, dtype=torch.int32, device=dev)
        self.live = torch.tensor([P, 0], dtype=torch.int32, device=dev)
        self.parent = torch.zeros(nb, dtype=torch.int32, device=dev)
        self.tok = torch.zeros(nb, dtype=torch.int64, device=dev)
        self.prompt_len = torch.tensor(self.Ls, dtype=torch.int32, device=dev)
        self.den = torch.tensor(beams.den(max_new), dtype=torch.float64).to(torch.float32).to(dev)
        self.cand_score = torch.empty((nb, beams.M), dtype=torch.float32, device=dev)
        self.cand_tok = torch.empty((nb, beams.M), dtype=torch.int32, device=dev)
        self.trace = ([], [], []) if trace else None   # per step: tokens, parents, running scores

    def choose(self, scores, seq, cur, out=None):
        self.tok = self.tok if out is None else out
        ops.gen_beam_topk(scores, seq, cur, self.run_score, self.beams.M, ids=self.ids,
                          repetition_penalty=self.processors[0], no_repeat_ngram_size=self.processors[1],
                          cand_score=self.cand_score, cand_tok=self.cand_tok)
        ops.gen_beam_step(self.cand_score, self.cand_tok, self.K, seq, cur, self.run_score, self.tok, self.parent,
                          self.fin_seq, self.fin_score, self.fin_len, self.open, self.live, self.den, self.beams.eos,
                          self.prompt_len)
        ops.kv_beam_reorder(self.kc, self.vc, self.K, self.parent, cur, self.prompt_len, self.max_new)

    def record(self):
        """Between two steps: what the last one chose (the replay trace of stats)."""
        if self.trace is not None:
            for kept, t in zip(self.trace, (self.tok, self.parent, self.run_score)):
                kept.append(t.clone())

    def results(self, steps, return_logits: bool, stats):
        """-> (per prompt its best finished hypothesis [1, n], its kept logits rows); the scores and trace into stats."""
        K, P = self.K, self.P
        lens = self.fin_len.view(P, K)[:, 0].tolist()
        if min(lens) < 1:
            raise RuntimeError("beam search: a prompt ended without a finished hypothesis")
        if stats is not None:
            stats["sequences_scores"].append(self.fin_score.view(P, K)[:, 0].tolist())
            for key, kept in zip(("beam_tokens", "beam_parents", "beam_scores"), self.trace):
                stats[key].append([t.view(P, K).tolist() for t in kept])
        outs = [self.fin_seq[p * K, :n].view(1, n) for p, n in enumerate(lens)]
        return outs, (steps if return_logits else []), lens


class _Chooser:
    """The token choice of one call: the one place that knows whether a token is drawn (sampler), taken among the
    allowed ids (allowed), searched over beams (beams; beam_rows: a chunk's device state) or the plain argmax, and
    which head the scores come from.  rows(): one chunk's chooser."""

    def __init__(self, model, repetition_penalty, no_repeat_ngram_size, allowed, sampler, beams=None):
        self.model, self.allowed, self.sampler, self.single, self.streams = model, allowed, sampler, False, None
        self.processors = (repetition_penalty, no_repeat_ngram_size)
        self.beams, self.beam_rows = beams, None

    def spread(self, kc, vc, seq, Ls, logits, max_new: int, trace: bool):
        """Beam search behind the prefill: P prompts' caches, ids and logits rows [P, V] copied into their K beam rows,
        and the first choice made -> (the chunk's chooser, kc, vc, seq of P * K rows, the [P * K, V] rows chosen from)."""
        K = self.beams.K
        kc, vc, seq = kc.repeat_interleave(K, dim=1), vc.repeat_interleave(K, dim=1), seq.repeat_interleave(K, dim=0)
        lg = logits.repeat_interleave(K, dim=0)   # run_score kills beams 1 .. K - 1 of the first choice
        c = copy.copy(self)
        c.beam_rows = _BeamRows(self.beams, self.model, self.processors, self.allowed, seq, Ls, max_new, kc, vc, trace)
        cur = torch.tensor([L for L in Ls for _ in range(K)], dtype=torch.int32, device=self.model.device)
        c.choose(lg, seq, cur)
        c.beam_rows.record()
        return c, kc, vc, seq, lg

    def rows(self, lo: int, hi: int, single: bool = False):
        """Prompts [lo, hi) of the call: their stream ids on the device.  single: generate(), plain kd_gen_select."""
        c = copy.copy(self)
        c.single = single
        if self.sampler is not None:
            c.streams = torch.tensor(self.sampler.streams[lo:hi], dtype=torch.int64, device=self.model.device)
        return c

    def head(self, hn, batch: bool):
        """Final-norm rows hn -> logits [nb, V], or [nb, A] of the allowed ids (gathered head or the full head's)."""
        w, a = self.model.lm_head_weight(), self.allowed
        if a is not None and a.gather:
            return ops.gemv_batch_gather(hn, w, a.ids) if batch else ops.gemv_gather(hn, w, a.ids)
        lg = (ops.gemv_batch if batch else ops.gemv)(hn, w)
        return lg if a is None or self.beams is not None else a.columns(lg)   # beams: the full row, masked in the kernel

    def choose(self, scores, seq, cur, out=None, row=None):
        """Every row's next token from head()'s scores: seq[b, cur[b]], out[b], cur[b] += 1.  row = b: row b alone."""
        a, s = self.allowed, self.sampler
        if self.beam_rows is not None:
            self.beam_rows.choose(scores, seq, cur, out)
        elif s is not None:   # kd_gen_sample in place of the select of the same scores
            ops.gen_sample(scores, seq, cur, ids=None if a is None else a.ids, repetition_penalty=self.processors[0],
                           no_repeat_ngram_size=self.processors[1], temperature=s.temperature, top_k=s.top_k,
                           top_p=s.top_p, seed=s.seed, out=out,
                           streams=self.streams if row is None else self.streams[row:row + 1])
        elif a is not None:
            ops.gen_select_ids(scores, a.ids, seq, cur, *self.processors, out=out)
        elif self.single:
            ops.gen_select(scores, seq, 0, *self.processors, out=out, cur=cur)
        else:
            ops.gen_select_batch(scores, seq, cur, *self.processors, out=out)

    def first(self, logits, seq_row, L: int, row: int):
        """The prefill's token from the prompt's full logits row [1, V], into seq_row [1, smax] at L -> the row kept.
        Beams: the full row and no token yet (spread() chooses for the whole chunk)."""
        if self.beams is not None:
            return logits
        if self.allowed is not None:
            logits = self.allowed.columns(logits)
        if self.allowed is None and self.sampler is None:
            ops.gen_select(logits, seq_row, L, *self.processors)
        else:
            self.choose(logits, seq_row, torch.full((1,), L, dtype=torch.int32, device=logits.device), row=row)
        return logits


@dataclasses.dataclass
class _Run:
    """The decode settings of one call, as its entry point checked them; rows() is a chunk's."""
    max_new_tokens: int
    eos: set
    return_logits: bool
    graph: bool
    k_stop: int
    stats: dict | None
    chooser: _Chooser

    def rows(self, lo: int, hi: int) -> "_Run":
        return dataclasses.replace(self, chooser=self.chooser.rows(lo, hi))


def _begin(who: str, model, n_rows: int, stop_check_every, allowed_token_ids, restrict_head, stats, sampling,
           beam_args=(1, 1.0, False, None, 1)):
    """The entry points' front matter, every ValueError before any device work: stop_check_every, beam_args =
    (num_beams, length_penalty, early_stopping, eos_token_id, max_new_tokens), allowed_token_ids / restrict_head, the stats keys,
    then sampling = (do_sample, temperature, top_k, top_p, seed, sample_streams) for n_rows prompts (do_sample=False:
    ignored, as transformers ignores its warpers) -> (k_stop, _Allowed, _Sampler, _Beams)."""
    k_stop = _stop_every(stop_check_every, who)
    beams = _beams(who, *beam_args[:3], sampling[0], restrict_head, *beam_args[3:])
    if beams is not None and allowed_token_ids is not None:
        restrict_head = False   # the full head always runs under beams
    allowed = _allowed(model, allowed_token_ids, restrict_head, who)
    _stats_begin(stats)
    if beams is not None and stats is not None:
        for key in ("sequences_scores", "beam_tokens", "beam_parents", "beam_scores"):
            stats[key] = []
    sampler = _Sampler(*sampling[1:], n_rows, who) if sampling[0] else None
    if sampler is not None and stats is not None:
        stats["seed"] = sampler.seed
    return k_stop, allowed, sampler, beams


class _Layers(typing.NamedTuple):
    eps: float
    inter: int
    weights: list   # per layer: (input norm, q|k|v weight, q|k|v bias, o_proj, post-attention norm, gate|up, down)


def _decode_layers(model) -> _Layers:
    T, P = model.cfg.text, model.P
    qd, kd = T.heads * T.head_dim, T.kv_heads * T.head_dim
    lp = "language_model.model."
    layers = []
    for i in range(T.layers):
        p = f"{lp}layers.{i}."
        layers.append((P[p + "input_layernorm.weight"],
                       P.span(p + "self_attn.q_proj.weight", p + "self_attn.v_proj.weight", qd + 2 * kd, T.hidden),
                       P.span(p + "self_attn.q_proj.bias", p + "self_attn.v_proj.bias", 1, qd + 2 * kd).view(-1),
                       P[p + "self_attn.o_proj.weight"], P[p + "post_attention_layernorm.weight"],
                       P.span(p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight", 2 * T.inter, T.hidden),
                       P[p + "mlp.down_proj.weight"]))
    return _Layers(T.eps, T.inter, layers)


def _layer_pass(x, layers: _Layers, linear, attend):
    """x through every decoder layer; linear: ops.gemv / gemv_batch / gemv_rows; attend(i, qkv): layer i's attention."""
    for i, (w_in, Wqkv, bqkv, Wo, w_post, Wgu, Wdown) in enumerate(layers.weights):
        qkv = linear(x, Wqkv, bias=bqkv, norm_w=w_in, eps=layers.eps)      # input_layernorm fused
        o = attend(i, qkv)
        x_mid = linear(o, Wo, residual=x)
        a = linear(x_mid, Wgu, swiglu_inter=layers.inter, norm_w=w_post, eps=layers.eps)  # post_attention_layernorm
        x = linear(a, Wdown, residual=x_mid)
    return x


def _gemv_unfused(x, w, norm_w=None, eps=None, **epilogue):
    """ops.gemv with the RMSNorm as its own launch in front (generate()'s fuse_norm=False A/B route)."""
    if norm_w is not None:
        x, _, _ = ops.norm_fwd(x, norm_w, None, eps, rms=True, save_stats=False)
    return ops.gemv(x, w, **epilogue)


def _final_norm(model, x):
    # its own launch: fused into the 38k-workgroup lm_head GEMV every workgroup would recompute it (measured slower)
    return ops.norm_fwd(x, model.P["language_model.model.norm.weight"], None, model.cfg.text.eps, rms=True,
                        save_stats=False)[0]


def _prefill(model, prompt, kc, vc, seq_row, chooser: _Chooser, row: int = 0):
    """One prompt (input_ids, pixel_values, image_sizes) of generate() / generate_batch(): the training forward, its
    roped k/v kept in the cache views kc, vc [layers, HKV, smax, hd], the ids in seq_row [1, smax] and the first token
    behind them (row: the prompt's slot in its chunk) -> (its logits row, the last layer's k/v).  The caller holds both
    while it decodes: freed, their storage is in the allocator's cache, which torch.cuda.graph empties before a capture
    and the next forward refills (1.7 ms per generate() call, profiles/generate_chooser/bench_ab.txt)."""
    input_ids, pixel_values, image_sizes = prompt
    L = int(input_ids.shape[1])
    kv = []
    fwd = model.forward(input_ids, pixel_values, image_sizes, save=False, kv_out=kv)
    for i, (k, v) in enumerate(kv):
        kc[i, :, :L].copy_(k[0])
        vc[i, :, :L].copy_(v[0])
    held = kv[-1]
    del kv
    seq_row[0, :L].copy_(input_ids[0])
    logits = model.logits(fwd["hn"][L - 1:L])
    del fwd
    return chooser.first(logits, seq_row, L, row), held


def _run_steps(step, n_steps: int, graph: bool, stop: _Stop, on_logits=None) -> int:
    """The decode loop of every entry point: step() (one token for every row; returns its logits) up
    to n_steps times, the first eagerly (warm-up: allocations, workspaces), the rest as replays of
    one HIP graph captured at the second; on_logits(lg) after each (lg is the graph's static buffer:
    clone what is kept); ends early once stop.done().  -> the steps run."""
    graph_obj, ran = None, 0
    for t_ in range(n_steps):
        if graph and t_ == 1:
            graph_obj = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph_obj):
                lg_static = step()
        if graph_obj is not None:
            graph_obj.replay()
            lg = lg_static
        else:
            lg = step()
        if on_logits is not None:
            on_logits(lg)
        ran = t_ + 1
        if stop.done(ran, n_steps):
            break
    return ran


def _first_eos(stop: _Stop, seq, Ls, max_new_tokens: int, eos) -> list:
    """Per row of seq [nb, smax] the length at its first EOS among its new tokens (0: none), where
    transformers stops; the steps past it are discarded.  Kept by the device when the stop is active
    (after an early stop the positions past it were never written), else one scan on the host."""
    fin = stop.ends()
    if fin is None:
        fin = [0] * len(Ls)
        if eos:
            host = seq.tolist()
            for b, L in enumerate(Ls):
                for j, t_ in enumerate(host[b][L:L + max_new_tokens]):
                    if t_ in eos:
                        fin[b] = L + j + 1
                        break
    return fin


@torch.no_grad()
def generate(model, input_ids: torch.Tensor, pixel_values: torch.Tensor, image_sizes, max_new_tokens: int = 32,
             repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, eos_token_id=EOS_TOKEN_IDS,
             pad_token_id: int | None = None, temperature: float | None = None, return_logits: bool = False,
             graph: bool = True, fuse_norm: bool | None = None, stop_check_every: int | None = None,
             stats: dict | None = None, allowed_token_ids=None, restrict_head: bool | None = None,
             do_sample: bool = False, top_k: int = 0, top_p: float = 1.0, seed: int | None = None,
             sample_streams=None, num_beams: int = 1, length_penalty: float = 1.0, early_stopping=False):
    """-> int64 [1, L + n_new] on the device (and the bf16 logits row of every step if
    return_logits).  Greedy unless do_sample (module docstring, "Sampling": temperature, top_k, top_p,
    seed and sample_streams, one int here, then take effect; stats also receives "seed").
    fuse_norm: RMSNorm fused into the q|k|v and gate|up GEMVs (default: FUSE_NORM_DEFAULT).
    stop_check_every = k (default STOP_CHECK_EVERY; 0: never): with 1..KD_GEN_EOS_MAX EOS ids the
    loop asks the device every k steps whether the row has emitted one and then ends, after
    min(n, k * max(1, ceil(s / k))) of its n = max_new_tokens - 1 steps (s: the step that produced the
    EOS, 0 for the prefill's token, n if none).  The result is the same bits for every k.
    stats (a dict) receives one-entry lists steps_run, steps_max, checks (host reads) and finished_at
    ([length at the first EOS, or 0]).
    allowed_token_ids, restrict_head: constrained decoding, see the module docstring (the logits
    returned are then the compact rows [1, A]).
    num_beams > 1 (length_penalty, early_stopping=False): beam search, module docstring; the call is then
    generate_batch([prompt], ...)[0], bit for bit (fuse_norm does not apply there)."""
    del pad_token_id   # batch of one: no padding of finished rows
    sampling = (do_sample, temperature, top_k, top_p, seed, sample_streams)
    k_stop, allowed, sampler, beams = _begin("generate", model, 1, stop_check_every, allowed_token_ids, restrict_head,
                                             stats, sampling, (num_beams, length_penalty, early_stopping, eos_token_id, max_new_tokens))
    if input_ids.dim() != 2 or input_ids.shape[0] != 1:
        raise ValueError("generate: batch size 1 (as evaluate_onevision.py runs it)")
    if beams is not None:   # the batched route: rows are beams
        got = generate_batch(model, [(input_ids, pixel_values, image_sizes)], max_new_tokens, repetition_penalty,
                             no_repeat_ngram_size, eos_token_id, None, temperature, return_logits, graph,
                             stop_check_every, stats, allowed_token_ids, restrict_head, num_beams=num_beams,
                             length_penalty=length_penalty, early_stopping=early_stopping)
        return (got[0][0], got[1][0]) if return_logits else got[0]
    chooser = _Chooser(model, repetition_penalty, no_repeat_ngram_size, allowed, sampler).rows(0, 1, single=True)
    T = model.cfg.text
    dev = model.device
    L = int(input_ids.shape[1])
    smax = L + int(max_new_tokens)
    eos = _eos_set(eos_token_id)
    nq, nkv, hd = T.heads, T.kv_heads, T.head_dim

    # ---- prefill: the training forward, its roped k/v kept
    kc = torch.empty((T.layers, nkv, smax, hd), dtype=torch.bfloat16, device=dev)
    vc = torch.empty_like(kc)
    seq = torch.empty((1, smax), dtype=torch.int64, device=dev)
    first, held = _prefill(model, (input_ids, pixel_values, image_sizes), kc, vc, seq, chooser)
    steps = [first]

    cos, sin = model._rope_for(smax)
    src = torch.full((1,), -2, dtype=torch.int32, device=dev)   # token embedding (kd_embed_assemble)
    table = model.P["language_model.model.embed_tokens.weight"]
    layers = _decode_layers(model)
    linear = ops.gemv if (FUSE_NORM_DEFAULT if fuse_norm is None else bool(fuse_norm)) else _gemv_unfused
    # device-resident step state: the sequence length (tokens so far, the one being decoded
    # included), the token being decoded and its RoPE row -> every launch of a step has fixed
    # arguments and the step replays from one captured HIP graph
    cur = torch.full((1,), L + 1, dtype=torch.int32, device=dev)
    tok = seq[0, L:L + 1].clone()   # the token being decoded (the chooser rewrites it each step)
    cos_row = torch.empty((1, cos.shape[1]), dtype=torch.float32, device=dev)
    sin_row = torch.empty_like(cos_row)
    stop = _Stop(model, 1, eos, k_stop)
    stop.mark(tok, cur)   # the prefill's token

    def attend(i, qkv):
        q, k, v = ops.qkv_split(qkv, 1, 1, nq, nkv, hd, hd, cos_row, sin_row)
        return ops.attn_decode(q.view(nq, hd), k.view(nkv, hd), v.view(nkv, hd), kc[i], vc[i], 0, hd, cur=cur)

    def step():
        ops.rope_row(cos, sin, cur, cos_row, sin_row)
        x = _layer_pass(ops.embed_assemble(tok, src, table, None, None, model.err), layers, linear, attend)
        lg = chooser.head(_final_norm(model, x), batch=False)
        chooser.choose(lg, seq, cur, out=tok)
        stop.mark(tok, cur)
        return lg

    n_steps = smax - (L + 1)
    ran = _run_steps(step, n_steps, graph, stop, (lambda lg: steps.append(lg.clone())) if return_logits else None)
    del held   # not before the decode is over: see _prefill
    end = _first_eos(stop, seq, [L], int(max_new_tokens), eos)[0]
    n = end or smax
    _stats_chunk(stats, ran, n_steps, stop.checks, [end])
    out = seq[0, :n].view(1, n)
    return (out, steps[:n - L]) if return_logits else out


MAX_BATCH = 16   # rows per decode step: the M dimension of the MFMA behind kd_gemv_batch


@torch.no_grad()
def generate_batch(model, prompts, max_new_tokens: int = 32, repetition_penalty: float = 1.0,
                   no_repeat_ngram_size: int = 0, eos_token_id=EOS_TOKEN_IDS, pad_token_id: int | None = None,
                   temperature: float | None = None, return_logits: bool = False, graph: bool = True,
                   stop_check_every: int | None = None, stats: dict | None = None, allowed_token_ids=None,
                   restrict_head: bool | None = None, do_sample: bool = False, top_k: int = 0, top_p: float = 1.0,
                   seed: int | None = None, sample_streams=None, num_beams: int = 1, length_penalty: float = 1.0,
                   early_stopping=False):
    """generate() for several prompts at once: prompts is a sequence of (input_ids [1, L_i],
    pixel_values [1, P_i, 3, 384, 384], image_sizes [1, 2]), ragged in L_i and P_i (no padding, no
    attention mask) -> list of int64 [1, L_i + n_i] (and, with return_logits, a list per row of the
    bf16 logits row of every step).

    Each prompt is prefilled on its own, exactly as generate() prefills it (the training forward's
    GEMM plan depends on M, so a batched prefill would make a row depend on its neighbours); the
    decode steps then run up to MAX_BATCH rows through every layer at once, so a step streams the
    weights once for all rows (kd_gemv_batch / kd_attn_decode_batch / kd_gen_select_batch, per-row
    lengths in a device counter).  A row's tokens and logits do not depend on which other prompts
    share its batch (bit-identical), longer lists run in chunks of MAX_BATCH.  Each row is cut
    after its first EOS; a chunk stops decoding once all its rows have emitted one, which the loop
    asks the device every stop_check_every = k steps (generate(): s is then the step that produced
    the last row's first EOS), so the results are the same bits for every k.  stats (a dict)
    receives, per chunk, steps_run, steps_max, checks and finished_at (per row the length at its
    first EOS, or 0).  allowed_token_ids, restrict_head: constrained decoding, see the module
    docstring (the logits returned are then the compact rows [1, A]).  do_sample, temperature, top_k,
    top_p, seed, sample_streams (one stream id per prompt; default: its index): module docstring,
    "Sampling"; a row's tokens depend on its prompt, the settings, seed and its own stream only.
    num_beams = K > 1, length_penalty, early_stopping=False: beam search (module docstring, "Beam search"): rows are
    beams, a chunk holds MAX_BATCH // K prompts, each result is its prompt's best finished hypothesis; stats also
    receives sequences_scores and the replay trace; return_logits gives per prompt and step the [K, V] rows."""
    del pad_token_id   # finished rows are cut, not padded
    prompts = list(prompts)
    sampling = (do_sample, temperature, top_k, top_p, seed, sample_streams)
    k_stop, allowed, sampler, beams = _begin("generate_batch", model, len(prompts), stop_check_every, allowed_token_ids,
                                             restrict_head, stats, sampling,
                                             (num_beams, length_penalty, early_stopping, eos_token_id, max_new_tokens))
    if not prompts:
        raise ValueError("generate_batch: no prompts")
    if int(max_new_tokens) < 1:
        raise ValueError("generate_batch: max_new_tokens must be >= 1")
    for ids, _, _ in prompts:
        if ids.dim() != 2 or ids.shape[0] != 1:
            raise ValueError("generate_batch: every prompt's input_ids must be [1, L]")
    run = _Run(int(max_new_tokens), _eos_set(eos_token_id), return_logits, graph, k_stop, stats,
               _Chooser(model, repetition_penalty, no_repeat_ngram_size, allowed, sampler, beams))
    outs, logs = [], []
    chunk = MAX_BATCH // (1 if beams is None else beams.K)   # rows are beams
    for c0 in range(0, len(prompts), chunk):
        o, lg = _generate_rows(model, prompts[c0:c0 + chunk], run.rows(c0, c0 + chunk))
        outs += o
        logs += lg
    return (outs, logs) if return_logits else outs


def _beam_spread(model, kc, vc, seq, Ls, logits, run: _Run):
    """Beam search takes over behind the prefill (chooser.spread) -> (run, kc, vc, seq, Ls of the P * K beam rows,
    steps: per prompt the [K, V] rows of the first choice)."""
    K = run.chooser.beams.K
    chooser, kc, vc, seq, lg = run.chooser.spread(kc, vc, seq, Ls, logits, run.max_new_tokens, run.stats is not None)
    steps = [[lg[p * K:(p + 1) * K]] if run.return_logits else [] for p in range(len(Ls))]
    return dataclasses.replace(run, chooser=chooser), kc, vc, seq, [L for L in Ls for _ in range(K)], steps


def _generate_rows(model, prompts, run: _Run):
    T = model.cfg.text
    nb = len(prompts)
    Ls = [int(ids.shape[1]) for ids, _, _ in prompts]
    smax = max(Ls) + run.max_new_tokens

    # ---- prefill, one prompt at a time: generate()'s own (row b of the caches and of seq)
    kc = torch.empty((T.layers, nb, T.kv_heads, smax, T.head_dim), dtype=torch.bfloat16, device=model.device)
    vc = torch.empty_like(kc)
    seq = torch.zeros((nb, smax), dtype=torch.int64, device=model.device)
    steps = [[] for _ in range(nb)]
    for b, prompt in enumerate(prompts):
        first, held = _prefill(model, prompt, kc[:, b], vc[:, b], seq[b:b + 1], run.chooser, b)
        steps[b].append(first)
    if run.chooser.beams is not None:
        run, kc, vc, seq, Ls, steps = _beam_spread(model, kc, vc, seq, Ls, torch.cat([s[0] for s in steps]), run)
    done = _decode_rows(model, kc, vc, seq, Ls, steps, run)
    del held   # not before the decode is over: see _prefill
    return done


def _decode_rows(model, kc, vc, seq, Ls, steps, run: _Run):
    """The batched decode loop behind generate_batch() and generate_grouped(): row b's caches hold
    its L_b prompt positions, seq[b, L_b] its first new token and steps[b] that token's logits row.
    The loop ends early once every row has emitted an EOS (_Stop)."""
    T = model.cfg.text
    dev = model.device
    nb, smax = seq.shape
    nq, nkv, hd = T.heads, T.kv_heads, T.head_dim
    cos, sin = model._rope_for(smax)
    src = torch.full((nb,), -2, dtype=torch.int32, device=dev)   # token embedding (kd_embed_assemble)
    table = model.P["language_model.model.embed_tokens.weight"]
    layers = _decode_layers(model)
    # device-resident per-row step state (generate()'s, one entry per row)
    cur = torch.tensor([L + 1 for L in Ls], dtype=torch.int32, device=dev)
    tok = torch.stack([seq[b, Ls[b]] for b in range(nb)])   # the tokens being decoded
    cos_rows = torch.empty((nb, cos.shape[1]), dtype=torch.float32, device=dev)
    sin_rows = torch.empty_like(cos_rows)
    beam = run.chooser.beam_rows   # beams: rows p * K + j, Ls per row, steps per prompt
    stop = _Stop(model, nb, run.eos, run.k_stop, beam)
    stop.mark(tok, cur)   # the prefill's tokens

    def attend(i, qkv):
        q, k, v = ops.qkv_split(qkv, 1, nb, nq, nkv, hd, hd, cos_rows, sin_rows)   # token b rotated by row b
        return ops.attn_decode_batch(q[0], k[0], v[0], kc[i], vc[i], cur, hd)

    def step():
        ops.rope_rows(cos, sin, cur, cos_rows, sin_rows)
        x = _layer_pass(ops.embed_assemble(tok, src, table, None, None, model.err), layers, ops.gemv_batch, attend)
        lg = run.chooser.head(_final_norm(model, x), batch=True)
        run.chooser.choose(lg, seq, cur, out=tok)
        stop.mark(tok, cur)
        return lg

    def keep(lg):
        if run.return_logits:
            lg = lg.clone()
            w = 1 if beam is None else beam.K   # beams: a prompt's [K, V] rows
            for b in range(nb // w):
                steps[b].append(lg[b * w:(b + 1) * w])
        if beam is not None:
            beam.record()

    n_steps = run.max_new_tokens - 1
    ran = _run_steps(step, n_steps, run.graph, stop,
                     keep if run.return_logits or (beam is not None and beam.trace is not None) else None)
    if beam is not None:   # per prompt its best finished hypothesis; steps past a prompt's last one are unspecified
        outs, steps, lens = beam.results(steps, run.return_logits, run.stats)
        _stats_chunk(run.stats, ran, n_steps, stop.checks, lens)
        return outs, steps
    # every row is cut after its own first EOS (fin[b]: its length there, 0 if none)
    fin = _first_eos(stop, seq, Ls, run.max_new_tokens, run.eos)
    ends = [fin[b] or L + run.max_new_tokens for b, L in enumerate(Ls)]
    _stats_chunk(run.stats, ran, n_steps, stop.checks, fin)
    outs = [seq[b, :ends[b]].view(1, ends[b]) for b in range(nb)]
    return outs, ([steps[b][:ends[b] - L] for b, L in enumerate(Ls)] if run.return_logits else [])


@torch.no_grad()
def generate_grouped(model, groups, max_new_tokens: int = 32, repetition_penalty: float = 1.0,
                     no_repeat_ngram_size: int = 0, eos_token_id=EOS_TOKEN_IDS, pad_token_id: int | None = None,
                     temperature: float | None = None, return_logits: bool = False, graph: bool = True,
                     stop_check_every: int | None = None, stats: dict | None = None, allowed_token_ids=None,
                     restrict_head: bool | None = None, do_sample: bool = False, top_k: int = 0, top_p: float = 1.0,
                     seed: int | None = None, sample_streams=None, num_beams: int = 1, length_penalty: float = 1.0,
                     early_stopping=False):
    """generate_batch() for questions grouped by image: groups is a sequence of (pixel_values
    [1, P, 3, 384, 384], image_sizes [1, 2], [input_ids [1, L_q], ...]) -> one list per group of int64
    [1, L_q + n_q] (and, with return_logits, the same nesting of per-step bf16 logits rows).

    P0 is the index of the group's last image token plus one.  Every question of a group must
    agree on ids[:P0] and have at least one token after it (ValueError otherwise).  The prefix
    ids[:P0] (template head + image) runs once per group through the training forward and seeds
    the cache of each of its questions; the suffixes ids[P0:] of up to MAX_BATCH questions then run
    through the layers together as ragged rows on the decode kernels' route (kd_gemv_rows,
    kd_attn_extend), and the batched decode of generate_batch() produces the remaining tokens.
    P0 is set by the image tokens, not by what the questions happen to share, so a question's
    tokens and logits depend only on its image, ids[:P0] and its own suffix, bit for bit: not on the
    other questions of its group, on other groups, on the chunk or on its slot.

    Not bit-identical to generate_batch() on the same prompt (the prefix forward runs at M = P0
    instead of M = L and the suffix rows take the decode kernels); both are held to the same bounds
    against the oracle.

    stop_check_every and stats as in generate_batch(): a chunk of up to MAX_BATCH questions stops
    decoding once all of them have emitted an EOS (one stats entry per chunk).
    allowed_token_ids, restrict_head: constrained decoding, see the module docstring (the logits
    returned are then the compact rows [1, A]; the head behind the extend pass is gathered too).
    do_sample, temperature, top_k, top_p, seed, sample_streams: module docstring, "Sampling"; one
    stream id per question in the flattened order of the groups (default: that index), and the token
    behind the extend pass is drawn too.  num_beams = K > 1, length_penalty, early_stopping=False: beam search as in
    generate_batch(); a chunk holds MAX_BATCH // K questions, the extend pass runs once per question and its
    suffix K/V is copied to the question's other beam rows."""
    del pad_token_id   # finished rows are cut, not padded
    groups = [(px, sizes, list(qs)) for px, sizes, qs in groups]
    sampling = (do_sample, temperature, top_k, top_p, seed, sample_streams)
    k_stop, allowed, sampler, beams = _begin("generate_grouped", model, sum(len(qs) for _, _, qs in groups),
                                             stop_check_every, allowed_token_ids, restrict_head, stats, sampling,
                                             (num_beams, length_penalty, early_stopping, eos_token_id, max_new_tokens))
    if not groups:
        raise ValueError("generate_grouped: no groups")
    if int(max_new_tokens) < 1:
        raise ValueError("generate_grouped: max_new_tokens must be >= 1")
    image_token = int(model.cfg.image_token_id)
    items = []   # (group, pixel_values, image_sizes, input_ids, P0), flattened in order
    for gi, (px, sizes, qs) in enumerate(groups):
        if not qs:
            raise ValueError(f"generate_grouped: group {gi} has no question")
        head, P0 = None, 0
        for ids in qs:
            if ids.dim() != 2 or ids.shape[0] != 1:
                raise ValueError("generate_grouped: every question's input_ids must be [1, L]")
            host = ids[0].tolist()
            last = max((i for i, t in enumerate(host) if t == image_token), default=-1)
            if last < 0:
                raise ValueError(f"generate_grouped: a question of group {gi} has no image token")
            if head is None:
                head, P0 = host[:last + 1], last + 1
            elif last + 1 != P0 or host[:P0] != head:
                raise ValueError(f"generate_grouped: the questions of group {gi} differ up to the last image token")
            if len(host) <= P0:
                raise ValueError(f"generate_grouped: a question of group {gi} ends on an image token")
            if len(host) - P0 > KD_GEMV_ROWS_MAX:
                raise ValueError(f"generate_grouped: more than {KD_GEMV_ROWS_MAX} tokens after the image")
            items.append((gi, px, sizes, ids, P0))
    run = _Run(int(max_new_tokens), _eos_set(eos_token_id), return_logits, graph, k_stop, stats,
               _Chooser(model, repetition_penalty, no_repeat_ngram_size, allowed, sampler, beams))
    outs, logs = [[] for _ in groups], [[] for _ in groups]
    carry = (None, None)   # the prefix K/V of the group a chunk ended in: its next chunk reuses them
    rows = MAX_BATCH // (1 if beams is None else beams.K)   # rows are beams
    for c0 in range(0, len(items), rows):
        chunk = items[c0:c0 + rows]
        o, lg, carry = _generate_grouped_rows(model, chunk, carry, run.rows(c0, c0 + rows))
        for (gi, *_), ob, lb in zip(chunk, o, lg if return_logits else [None] * len(o)):
            outs[gi].append(ob)
            logs[gi].append(lb)
    return (outs, logs) if return_logits else outs


def _extend_rows(model, layers: _Layers, kc, vc, toks, lens, bases):
    """Ragged rows behind cached prefixes, through every layer at once (generate_grouped(): the questions behind an
    image; score_answers(): the answers behind a prompt).  Slot b of the caches kc, vc [layers, nb, HKV, smax, hd]
    holds bases[b] positions; its lens[b] tokens (toks: int64 on the device, slot after slot, at most
    KD_GEMV_ROWS_MAX) sit at positions bases[b] + j, see the prefix and their own slot's rows up to themselves, and
    leave their k/v in the cache -> (x [R, hidden] behind the last layer, row_start [nb + 1] int32)."""
    T, dev = model.cfg.text, model.device
    nq, nkv, hd = T.heads, T.kv_heads, T.head_dim
    starts = [0]
    for n in lens:
        starts.append(starts[-1] + n)
    R = starts[-1]
    row_start = torch.tensor(starts, dtype=torch.int32, device=dev)
    base = torch.tensor(list(bases), dtype=torch.int32, device=dev)
    cur_rows = torch.tensor([P + j + 1 for P, n in zip(bases, lens) for j in range(n)],
                            dtype=torch.int32, device=dev)   # position + 1, as the decode step's counter
    src = torch.full((R,), -2, dtype=torch.int32, device=dev)   # token embedding (kd_embed_assemble)
    cos, sin = model._rope_for(kc.shape[3])
    cos_rows = torch.empty((R, cos.shape[1]), dtype=torch.float32, device=dev)
    sin_rows = torch.empty_like(cos_rows)
    ops.rope_rows(cos, sin, cur_rows, cos_rows, sin_rows)
    table = model.P["language_model.model.embed_tokens.weight"]

    def attend(i, qkv):
        q, k, v = ops.qkv_split(qkv, 1, R, nq, nkv, hd, hd, cos_rows, sin_rows)   # row r rotated by its position
        return ops.attn_extend(q[0], k[0], v[0], kc[i], vc[i], row_start, base, hd)

    x = _layer_pass(ops.embed_assemble(toks, src, table, None, None, model.err), layers, ops.gemv_rows, attend)
    return x, row_start


def _generate_grouped_rows(model, chunk, carry, run: _Run):
    T = model.cfg.text
    dev = model.device
    nb = len(chunk)
    Ls = [int(ids.shape[1]) for _, _, _, ids, _ in chunk]
    P0s = [P0 for *_, P0 in chunk]
    smax = max(Ls) + run.max_new_tokens
    nkv, hd = T.kv_heads, T.head_dim

    kc = torch.empty((T.layers, nb, nkv, smax, hd), dtype=torch.bfloat16, device=dev)
    vc = torch.empty_like(kc)
    seq = torch.zeros((nb, smax), dtype=torch.int64, device=dev)
    # ---- prefix prefill, once per group: the training forward over ids[:P0], copied into every slot of the group
    for b, (gi, px, sizes, ids, P0) in enumerate(chunk):
        if carry[0] != gi:
            kv = []
            model.forward(ids[:, :P0], px, sizes, save=False, kv_out=kv)
            carry = (gi, kv)
        for i, (k, v) in enumerate(carry[1]):
            kc[i, b, :, :P0].copy_(k[0])
            vc[i, b, :, :P0].copy_(v[0])
        seq[b, :Ls[b]].copy_(ids[0])

    # ---- extend pass: every suffix row of the chunk through the layers at once (sub-ranges of
    # questions only if the rows exceed the kernels' cap; a question's bits do not depend on the split)
    layers = _decode_layers(model)
    last = []
    b0 = 0
    while b0 < nb:
        b1, R = b0, 0
        while b1 < nb and R + Ls[b1] - P0s[b1] <= KD_GEMV_ROWS_MAX:
            R += Ls[b1] - P0s[b1]
            b1 += 1
        toks = torch.cat([chunk[b][3][0, P0s[b]:] for b in range(b0, b1)]).contiguous()
        x, row_start = _extend_rows(model, layers, kc[:, b0:b1], vc[:, b0:b1], toks,
                                    [Ls[b] - P0s[b] for b in range(b0, b1)], P0s[b0:b1])
        last.append(x.index_select(0, (row_start[1:] - 1).long()))   # each question's last suffix row
        b0 = b1
    xl = last[0] if len(last) == 1 else torch.cat(last)
    hn = _final_norm(model, xl)
    cur = torch.tensor(Ls, dtype=torch.int32, device=dev)
    lg = run.chooser.head(hn, batch=True)
    if run.chooser.beams is not None:
        run, kc, vc, seq, Ls, steps = _beam_spread(model, kc, vc, seq, Ls, lg, run)
    else:
        run.chooser.choose(lg, seq, cur)   # seq[b, L_b]; cur = L_b + 1
        steps = [[lg[b:b + 1]] if run.return_logits else [] for b in range(nb)]
    outs, steps = _decode_rows(model, kc, vc, seq, Ls, steps, run)
    return outs, steps, carry
