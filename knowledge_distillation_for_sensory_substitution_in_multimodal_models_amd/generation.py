"""Student generate(): prefill + KV-cache greedy decode on the HIP kernels.

Drop-in for the call the reference's evaluation makes on the trained student
(evaluation/onevisionv3/evaluate_onevision.py:185-195):

    model.generate(**inputs, max_new_tokens=32, pad_token_id=pad_token_id,
                   repetition_penalty=1.2, no_repeat_ngram_size=2, temperature=0.7)

`do_sample` is not set there, so decoding is greedy and `temperature` has no effect (transformers
only applies it when sampling).  The prompt runs through the same forward as training
(LlavaOnevisionModel.forward: SigLIP, projector, anyres pack, Qwen2), whose roped keys and values
seed a per-layer KV cache [HKV, L + max_new_tokens, hd]; each new token then runs one row through
every layer (kd_gemv with the RMSNorms fused in front and bias / residual / SwiGLU epilogues, kd_qkv_split with its
RoPE row, split-KV kd_attn_decode) and kd_gen_select picks it on the device.  The position lives in a device counter, so
every launch of a step has fixed arguments: the first step runs eagerly, the step is captured
once as a HIP graph (torch.cuda.CUDAGraph) and replayed for the rest; steps past an EOS are
discarded afterwards (one host read at the end instead of one per token).  Returns prompt + generated ids like
transformers' generate (B = 1, as the evaluation runs it).

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
"""
from __future__ import annotations

import torch

from . import ops
from ._native import KD_GEMV_ROWS_MAX


EOS_TOKEN_IDS = (151645,)   # <|im_end|>: generation_config.eos_token_id of the -ov-hf chat checkpoints


FUSE_NORM_DEFAULT = True   # RMSNorm fused into the decode GEMVs (tools/bench_generate.py passes fuse_norm for A/B)


@torch.no_grad()
def generate(model, input_ids: torch.Tensor, pixel_values: torch.Tensor, image_sizes, max_new_tokens: int = 32,
             repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, eos_token_id=EOS_TOKEN_IDS,
             pad_token_id: int | None = None, temperature: float | None = None, return_logits: bool = False,
             graph: bool = True, fuse_norm: bool | None = None):
    """-> int64 [1, L + n_new] on the device (and the bf16 logits row of every step if
    return_logits).  `temperature` is accepted for signature parity and ignored (greedy).
    fuse_norm: RMSNorm fused into the q|k|v and gate|up GEMVs (default: FUSE_NORM_DEFAULT)."""
    del temperature, pad_token_id   # greedy, batch of one: no padding of finished rows
    FUSE_NORM = FUSE_NORM_DEFAULT if fuse_norm is None else bool(fuse_norm)
    if input_ids.dim() != 2 or input_ids.shape[0] != 1:
        raise ValueError("generate: batch size 1 (as evaluate_onevision.py runs it)")
    T, P = model.cfg.text, model.P
    dev = model.device
    L = int(input_ids.shape[1])
    smax = L + int(max_new_tokens)
    eos = {int(e) for e in ([eos_token_id] if isinstance(eos_token_id, int) else (eos_token_id or ()))}
    nq, nkv, hd = T.heads, T.kv_heads, T.head_dim
    qd, kd = nq * hd, nkv * hd
    lp = "language_model.model."

    # ---- prefill: the training forward, its roped k/v kept
    kv = []
    fwd = model.forward(input_ids, pixel_values, image_sizes, save=False, kv_out=kv)
    kc = torch.empty((T.layers, nkv, smax, hd), dtype=torch.bfloat16, device=dev)
    vc = torch.empty_like(kc)
    for i, (k, v) in enumerate(kv):
        kc[i, :, :L].copy_(k[0])
        vc[i, :, :L].copy_(v[0])
    del kv
    seq = torch.empty(smax, dtype=torch.int64, device=dev)
    seq[:L].copy_(input_ids[0])
    logits = model.logits(fwd["hn"][L - 1:L])
    del fwd
    steps = [logits] if return_logits else None
    ops.gen_select(logits, seq, L, repetition_penalty, no_repeat_ngram_size)

    cos, sin = model._rope_for(smax)
    src = torch.full((1,), -2, dtype=torch.int32, device=dev)   # token embedding (kd_embed_assemble)
    table = P[lp + "embed_tokens.weight"]
    layers = []
    for i in range(T.layers):
        p = f"{lp}layers.{i}."
        layers.append((P[p + "input_layernorm.weight"],
                       P.span(p + "self_attn.q_proj.weight", p + "self_attn.v_proj.weight", qd + 2 * kd, T.hidden),
                       P.span(p + "self_attn.q_proj.bias", p + "self_attn.v_proj.bias", 1, qd + 2 * kd).view(-1),
                       P[p + "self_attn.o_proj.weight"], P[p + "post_attention_layernorm.weight"],
                       P.span(p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight", 2 * T.inter, T.hidden),
                       P[p + "mlp.down_proj.weight"]))
    # device-resident step state: the sequence length (tokens so far, the one being decoded
    # included), the token being decoded and its RoPE row -> every launch of a step has fixed
    # arguments and the step replays from one captured HIP graph
    cur = torch.full((1,), L + 1, dtype=torch.int32, device=dev)
    tok = seq[L:L + 1].clone()   # the token being decoded (kd_gen_select rewrites it each step)
    cos_row = torch.empty((1, cos.shape[1]), dtype=torch.float32, device=dev)
    sin_row = torch.empty_like(cos_row)

    def step():
        ops.rope_row(cos, sin, cur, cos_row, sin_row)
        x = ops.embed_assemble(tok, src, table, None, None, model.err)
        for i, (w_in, Wqkv, bqkv, Wo, w_post, Wgu, Wdown) in enumerate(layers):
            if FUSE_NORM:
                qkv = ops.gemv(x, Wqkv, bias=bqkv, norm_w=w_in, eps=T.eps)      # input_layernorm fused
            else:
                h, _, _ = ops.norm_fwd(x, w_in, None, T.eps, rms=True, save_stats=False)
                qkv = ops.gemv(h, Wqkv, bias=bqkv)
            q, k, v = ops.qkv_split(qkv, 1, 1, nq, nkv, hd, hd, cos_row, sin_row)
            o = ops.attn_decode(q.view(nq, hd), k.view(nkv, hd), v.view(nkv, hd), kc[i], vc[i], 0, hd, cur=cur)
            x_mid = ops.gemv(o, Wo, residual=x)
            if FUSE_NORM:
                a = ops.gemv(x_mid, Wgu, swiglu_inter=T.inter, norm_w=w_post, eps=T.eps)  # post_attention_layernorm
            else:
                h2, _, _ = ops.norm_fwd(x_mid, w_post, None, T.eps, rms=True, save_stats=False)
                a = ops.gemv(h2, Wgu, swiglu_inter=T.inter)
            x = ops.gemv(a, Wdown, residual=x_mid)
        # final norm as its own launch: fused into the 38k-workgroup lm_head GEMV it would be recomputed
        # by every workgroup (measured slower)
        hn, _, _ = ops.norm_fwd(x, P[lp + "norm.weight"], None, T.eps, rms=True, save_stats=False)
        lg = ops.gemv(hn, model.lm_head_weight())
        ops.gen_select(lg, seq, 0, repetition_penalty, no_repeat_ngram_size, out=tok, cur=cur)
        return lg

    n_steps = smax - (L + 1)
    graph_obj = None
    for t_ in range(n_steps):
        if graph and t_ == 1:   # step 0 ran eagerly (warm-up: allocations, workspaces); capture the rest
            graph_obj = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph_obj):
                lg_static = step()
        if graph_obj is not None:
            graph_obj.replay()
            lg = lg_static
        else:
            lg = step()
        if return_logits:
            steps.append(lg.clone())
    n = smax
    if eos:   # transformers stops after the first EOS; the steps past it are discarded
        gen = seq[L:smax].tolist()
        for j, t_ in enumerate(gen):
            if t_ in eos:
                n = L + j + 1
                break
        if return_logits:
            steps = steps[:n - L]
    out = seq[:n].view(1, n)
    return (out, steps) if return_logits else out


MAX_BATCH = 16   # rows per decode step: the M dimension of the MFMA behind kd_gemv_batch


@torch.no_grad()
def generate_batch(model, prompts, max_new_tokens: int = 32, repetition_penalty: float = 1.0,
                   no_repeat_ngram_size: int = 0, eos_token_id=EOS_TOKEN_IDS, pad_token_id: int | None = None,
                   temperature: float | None = None, return_logits: bool = False, graph: bool = True):
    """generate() for several prompts at once: prompts is a sequence of (input_ids [1, L_i],
    pixel_values [1, P_i, 3, 384, 384], image_sizes [1, 2]), ragged in L_i and P_i (no padding, no
    attention mask) -> list of int64 [1, L_i + n_i] (and, with return_logits, a list per row of the
    bf16 logits row of every step).

    Each prompt is prefilled on its own, exactly as generate() prefills it (the training forward's
    GEMM plan depends on M, so a batched prefill would make a row depend on its neighbours); the
    decode steps then run up to MAX_BATCH rows through every layer at once, so a step streams the
    weights once for all rows (kd_gemv_batch / kd_attn_decode_batch / kd_gen_select_batch, per-row
    lengths in a device counter).  A row's tokens and logits do not depend on which other prompts
    share its batch (bit-identical), longer lists run in chunks of MAX_BATCH.  All rows run
    max_new_tokens steps; each is cut after its first EOS with one host read at the end."""
    del temperature, pad_token_id   # greedy; finished rows are cut, not padded
    prompts = list(prompts)
    if not prompts:
        raise ValueError("generate_batch: no prompts")
    if int(max_new_tokens) < 1:
        raise ValueError("generate_batch: max_new_tokens must be >= 1")
    for ids, _, _ in prompts:
        if ids.dim() != 2 or ids.shape[0] != 1:
            raise ValueError("generate_batch: every prompt's input_ids must be [1, L]")
    outs, logs = [], []
    for c0 in range(0, len(prompts), MAX_BATCH):
        o, lg = _generate_rows(model, prompts[c0:c0 + MAX_BATCH], int(max_new_tokens), repetition_penalty,
                               no_repeat_ngram_size, eos_token_id, return_logits, graph)
        outs += o
        logs += lg
    return (outs, logs) if return_logits else outs


def _generate_rows(model, prompts, max_new_tokens, repetition_penalty, no_repeat_ngram_size, eos_token_id,
                   return_logits, graph):
    T = model.cfg.text
    dev = model.device
    nb = len(prompts)
    Ls = [int(ids.shape[1]) for ids, _, _ in prompts]
    smax = max(Ls) + max_new_tokens
    eos = {int(e) for e in ([eos_token_id] if isinstance(eos_token_id, int) else (eos_token_id or ()))}
    nkv, hd = T.kv_heads, T.head_dim

    # ---- prefill, one prompt at a time: generate()'s own (row b of the caches and of seq)
    kc = torch.empty((T.layers, nb, nkv, smax, hd), dtype=torch.bfloat16, device=dev)
    vc = torch.empty_like(kc)
    seq = torch.zeros((nb, smax), dtype=torch.int64, device=dev)
    steps = [[] for _ in range(nb)]
    for b, (input_ids, pixel_values, image_sizes) in enumerate(prompts):
        L = Ls[b]
        kv = []
        fwd = model.forward(input_ids, pixel_values, image_sizes, save=False, kv_out=kv)
        for i, (k, v) in enumerate(kv):
            kc[i, b, :, :L].copy_(k[0])
            vc[i, b, :, :L].copy_(v[0])
        del kv
        seq[b, :L].copy_(input_ids[0])
        logits = model.logits(fwd["hn"][L - 1:L])
        del fwd
        if return_logits:
            steps[b].append(logits)
        ops.gen_select(logits, seq[b], L, repetition_penalty, no_repeat_ngram_size)

    return _decode_rows(model, kc, vc, seq, Ls, steps, max_new_tokens, repetition_penalty, no_repeat_ngram_size, eos,
                        return_logits, graph)


def _decode_layers(model):
    """Per layer: (input norm, q|k|v weight, q|k|v bias, o_proj, post-attention norm, gate|up, down)."""
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
    return layers


def _decode_rows(model, kc, vc, seq, Ls, steps, max_new_tokens, repetition_penalty, no_repeat_ngram_size, eos,
                 return_logits, graph):
    """The batched decode loop behind generate_batch() and generate_grouped(): row b's caches hold
    its L_b prompt positions, seq[b, L_b] its first new token and steps[b] that token's logits row."""
    T, P = model.cfg.text, model.P
    dev = model.device
    nb, smax = seq.shape
    nq, nkv, hd = T.heads, T.kv_heads, T.head_dim
    lp = "language_model.model."
    cos, sin = model._rope_for(smax)
    src = torch.full((nb,), -2, dtype=torch.int32, device=dev)   # token embedding (kd_embed_assemble)
    table = P[lp + "embed_tokens.weight"]
    layers = _decode_layers(model)
    # device-resident per-row step state (generate()'s, one entry per row)
    cur = torch.tensor([L + 1 for L in Ls], dtype=torch.int32, device=dev)
    tok = torch.stack([seq[b, Ls[b]] for b in range(nb)])   # the tokens being decoded
    cos_rows = torch.empty((nb, cos.shape[1]), dtype=torch.float32, device=dev)
    sin_rows = torch.empty_like(cos_rows)

    def step():
        ops.rope_rows(cos, sin, cur, cos_rows, sin_rows)
        x = ops.embed_assemble(tok, src, table, None, None, model.err)
        for i, (w_in, Wqkv, bqkv, Wo, w_post, Wgu, Wdown) in enumerate(layers):
            qkv = ops.gemv_batch(x, Wqkv, bias=bqkv, norm_w=w_in, eps=T.eps)      # input_layernorm fused
            q, k, v = ops.qkv_split(qkv, 1, nb, nq, nkv, hd, hd, cos_rows, sin_rows)   # token b rotated by row b
            o = ops.attn_decode_batch(q[0], k[0], v[0], kc[i], vc[i], cur, hd)
            x_mid = ops.gemv_batch(o, Wo, residual=x)
            a = ops.gemv_batch(x_mid, Wgu, swiglu_inter=T.inter, norm_w=w_post, eps=T.eps)  # post_attention_layernorm
            x = ops.gemv_batch(a, Wdown, residual=x_mid)
        hn, _, _ = ops.norm_fwd(x, P[lp + "norm.weight"], None, T.eps, rms=True, save_stats=False)
        lg = ops.gemv_batch(hn, model.lm_head_weight())
        ops.gen_select_batch(lg, seq, cur, repetition_penalty, no_repeat_ngram_size, out=tok)
        return lg

    graph_obj = None
    for t_ in range(max_new_tokens - 1):
        if graph and t_ == 1:   # step 0 ran eagerly (warm-up: allocations, workspaces); capture the rest
            graph_obj = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph_obj):
                lg_static = step()
        if graph_obj is not None:
            graph_obj.replay()
            lg = lg_static
        else:
            lg = step()
        if return_logits:
            lg = lg.clone()
            for b in range(nb):
                steps[b].append(lg[b:b + 1])
    ends = [L + max_new_tokens for L in Ls]
    if eos:   # every row is cut after its own first EOS; the steps past it are discarded
        host = seq.tolist()
        for b, L in enumerate(Ls):
            for j, t_ in enumerate(host[b][L:ends[b]]):
                if t_ in eos:
                    ends[b] = L + j + 1
                    break
            steps[b] = steps[b][:ends[b] - L]
    outs = [seq[b, :ends[b]].view(1, ends[b]) for b in range(nb)]
    return outs, (steps if return_logits else [])


@torch.no_grad()
def generate_grouped(model, groups, max_new_tokens: int = 32, repetition_penalty: float = 1.0,
                     no_repeat_ngram_size: int = 0, eos_token_id=EOS_TOKEN_IDS, pad_token_id: int | None = None,
                     temperature: float | None = None, return_logits: bool = False, graph: bool = True):
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
    against the oracle."""
    del temperature, pad_token_id   # greedy; finished rows are cut, not padded
    groups = [(px, sizes, list(qs)) for px, sizes, qs in groups]
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
    outs, logs = [[] for _ in groups], [[] for _ in groups]
    carry = (None, None)   # the prefix K/V of the group a chunk ended in: its next chunk reuses them
    for c0 in range(0, len(items), MAX_BATCH):
        chunk = items[c0:c0 + MAX_BATCH]
        o, lg, carry = _generate_grouped_rows(model, chunk, carry, int(max_new_tokens), repetition_penalty,
                                              no_repeat_ngram_size, eos_token_id, return_logits, graph)
        for (gi, *_), ob, lb in zip(chunk, o, lg if return_logits else [None] * len(o)):
            outs[gi].append(ob)
            logs[gi].append(lb)
    return (outs, logs) if return_logits else outs


def _generate_grouped_rows(model, chunk, carry, max_new_tokens, repetition_penalty, no_repeat_ngram_size, eos_token_id,
                           return_logits, graph):
    T, P = model.cfg.text, model.P
    dev = model.device
    nb = len(chunk)
    Ls = [int(ids.shape[1]) for _, _, _, ids, _ in chunk]
    P0s = [P0 for *_, P0 in chunk]
    smax = max(Ls) + max_new_tokens
    eos = {int(e) for e in ([eos_token_id] if isinstance(eos_token_id, int) else (eos_token_id or ()))}
    nq, nkv, hd = T.heads, T.kv_heads, T.head_dim
    lp = "language_model.model."

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
    cos, sin = model._rope_for(smax)
    table = P[lp + "embed_tokens.weight"]
    layers = _decode_layers(model)
    last = []
    b0 = 0
    while b0 < nb:
        b1, R = b0, 0
        while b1 < nb and R + Ls[b1] - P0s[b1] <= KD_GEMV_ROWS_MAX:
            R += Ls[b1] - P0s[b1]
            b1 += 1
        starts = [0]
        for b in range(b0, b1):
            starts.append(starts[-1] + Ls[b] - P0s[b])
        row_start = torch.tensor(starts, dtype=torch.int32, device=dev)
        base = torch.tensor(P0s[b0:b1], dtype=torch.int32, device=dev)
        cur_rows = torch.tensor([P0s[b] + j + 1 for b in range(b0, b1) for j in range(Ls[b] - P0s[b])],
                                dtype=torch.int32, device=dev)   # position + 1, as the decode step's counter
        toks = torch.cat([chunk[b][3][0, P0s[b]:] for b in range(b0, b1)]).contiguous()
        src = torch.full((R,), -2, dtype=torch.int32, device=dev)   # token embedding (kd_embed_assemble)
        cos_rows = torch.empty((R, cos.shape[1]), dtype=torch.float32, device=dev)
        sin_rows = torch.empty_like(cos_rows)
        ops.rope_rows(cos, sin, cur_rows, cos_rows, sin_rows)
        x = ops.embed_assemble(toks, src, table, None, None, model.err)
        for i, (w_in, Wqkv, bqkv, Wo, w_post, Wgu, Wdown) in enumerate(layers):
            qkv = ops.gemv_rows(x, Wqkv, bias=bqkv, norm_w=w_in, eps=T.eps)      # input_layernorm fused
            q, k, v = ops.qkv_split(qkv, 1, R, nq, nkv, hd, hd, cos_rows, sin_rows)   # row r rotated by its position
            o = ops.attn_extend(q[0], k[0], v[0], kc[i, b0:b1], vc[i, b0:b1], row_start, base, hd)
            x_mid = ops.gemv_rows(o, Wo, residual=x)
            a = ops.gemv_rows(x_mid, Wgu, swiglu_inter=T.inter, norm_w=w_post, eps=T.eps)  # post_attention_layernorm
            x = ops.gemv_rows(a, Wdown, residual=x_mid)
        last.append(x.index_select(0, (row_start[1:] - 1).long()))   # each question's last suffix row
        b0 = b1
    xl = last[0] if len(last) == 1 else torch.cat(last)
    hn, _, _ = ops.norm_fwd(xl, P[lp + "norm.weight"], None, T.eps, rms=True, save_stats=False)
    lg = ops.gemv_batch(hn, model.lm_head_weight())
    cur = torch.tensor(Ls, dtype=torch.int32, device=dev)
    ops.gen_select_batch(lg, seq, cur, repetition_penalty, no_repeat_ngram_size)   # seq[b, L_b]; cur = L_b + 1
    steps = [[lg[b:b + 1]] if return_logits else [] for b in range(nb)]
    outs, steps = _decode_rows(model, kc, vc, seq, Ls, steps, max_new_tokens, repetition_penalty,
                               no_repeat_ngram_size, eos, return_logits, graph)
    return outs, steps, carry
