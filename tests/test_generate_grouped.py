"""generate_grouped(): one image prefill shared by its questions.  kd_gemv_rows against kd_gemv_batch
(bit for bit, slab by slab and row by row) and torch fp32; kd_attn_extend against fp32 torch
attention, its cache stores, its independence of the other questions and the batched decode kernel;
the grouped decode on the tiny student against the CPU oracle model, eager launches, a
one-question call, generate_batch(), the EOS cut and chunking (GPU); argument validation of the new
entry points (CPU)."""
import ctypes
import functools
from types import SimpleNamespace

import pytest
import torch

from oracle import generation as G

PKG = "knowledge_distillation_for_sensory_substitution_in_multimodal_models_amd"

GEMV_SHAPES = [(1152, 896, "bias"), (896, 4864, "residual"), (4864, 896, "swiglu"),
               (21, 40, "none")]   # 4864 as K: the K split; (21, 40): an N tail and a K tail
ROWS = (1, 17, 40, 81)   # one slab, one row past a slab, two and a half slabs; six slabs over the four slab
                         # groups of a weight tile: groups 0 and 1 run their slab loop twice, the last slab has one row


# ----------------------------------------------------------------------------- CPU ----

def test_abi_grouped_symbols_reject_bad_arguments():
    """Validation runs before any device work: null pointers -> KD_ERR_ARG (7), bad shapes ->
    KD_ERR_SHAPE (1), a short workspace -> KD_ERR_WORKSPACE (8) (host memory stands in for the
    pointers: it is never dereferenced)."""
    from importlib import import_module
    NV = import_module(f"{PKG}._native")
    lib = NV.lib()
    MAXR = NV.KD_GEMV_ROWS_MAX
    assert lib.kd_gemv_rows(None, 8, 1, None, 8, None, None, 4, 8, 0, 0, None, 1e-6, None, 0, None) == 7
    assert lib.kd_attn_extend(None, None, None, None, None, None, 1, 1, 2, 1, 64, 64, 8, None, None, None, 0, None) == 7
    buf = ctypes.create_string_buffer(256 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    assert lib.kd_gemv_rows(p, 8, 0, p, 8, None, p, 4, 8, 0, 0, None, 1e-6, None, 0, None) == 1            # rows < 1
    assert lib.kd_gemv_rows(p, 8, MAXR + 1, p, 8, None, p, 4, 8, 0, 0, None, 1e-6, None, 0, None) == 1     # rows > max
    assert lib.kd_gemv_rows(p, 8, 1, p, 8, None, p, 4, 12, 0, 0, None, 1e-6, None, 0, None) == 1           # K % 8
    assert lib.kd_gemv_rows(p, 4864, 17, p, 4864, p, p, 896, 4864, 2, 0, None, 1e-6, None, 0, None) == 8   # K split
    assert lib.kd_gemv_rows(p, 4864, 17, p, 4864, p, p, 896, 4864, 2, 0, None, 1e-6, p,
                            lib.kd_gemv_rows_workspace_size(16, 896, 4864, 2), None) == 8                  # 32 rows' worth
    assert lib.kd_attn_extend(p, p, p, p, p, p, 1, 1, 2, 1, 96, 96, 8, p, p, p, 0, None) == 1              # head dim
    assert lib.kd_attn_extend(p, p, p, p, p, p, 1, 0, 2, 1, 64, 64, 8, p, p, p, 1 << 20, None) == 1        # rows < 1
    assert lib.kd_attn_extend(p, p, p, p, p, p, 1, MAXR + 1, 2, 1, 64, 64, 8, p, p, p, 1 << 30, None) == 1
    assert lib.kd_attn_extend(p, p, p, p, p, p, 3, 2, 2, 1, 64, 64, 8, p, p, p, 1 << 20, None) == 1        # nb > rows
    assert lib.kd_attn_extend(p, p, p, p, p, p, 2, 3, 2, 1, 64, 64, 8, p, p, p, 16, None) == 8
    # the slab layout is kd_gemv_batch's: 16 rows need exactly its workspace; the plan depends on (N, K) only
    for N, K, e in ((896, 4864, 2), (4864, 896, 3), (1152, 896, 1), (21, 40, 0)):
        assert lib.kd_gemv_rows_workspace_size(16, N, K, e) == lib.kd_gemv_batch_workspace_size(N, K, e)
        assert lib.kd_gemv_rows_workspace_size(1, N, K, e) == lib.kd_gemv_batch_workspace_size(N, K, e)
    assert lib.kd_gemv_rows_workspace_size(40, 896, 4864, 2) == 3 * lib.kd_gemv_batch_workspace_size(896, 4864, 2) > 0
    assert lib.kd_attn_extend_workspace_size(40, 14, 64, 320) == 40 * lib.kd_attn_decode_workspace_size(14, 64, 320)


def test_generate_grouped_refuses_bad_groups_before_any_device_work():
    """Every check runs on host copies of the ids before the model is touched: a model stub with
    nothing but the image token id is enough."""
    from importlib import import_module
    gen = import_module(f"{PKG}.generation")
    IMG = import_module(f"{PKG}.modeling").IMAGE_TOKEN_ID
    model = SimpleNamespace(cfg=SimpleNamespace(image_token_id=IMG))
    px, sizes = torch.zeros(1, 2, 3, 384, 384), torch.tensor([[336, 336]])

    def ids(*toks):
        return torch.tensor([list(toks)], dtype=torch.int64)

    good = ids(5, 6, IMG, IMG, 7, 8)
    with pytest.raises(ValueError, match="no groups"):
        gen.generate_grouped(model, [])
    with pytest.raises(ValueError, match="no question"):
        gen.generate_grouped(model, [(px, sizes, [])])
    with pytest.raises(ValueError, match="differ"):
        gen.generate_grouped(model, [(px, sizes, [good, ids(5, 9, IMG, IMG, 7, 8)])])      # differs before the image
    with pytest.raises(ValueError, match="differ"):
        gen.generate_grouped(model, [(px, sizes, [good, ids(5, 6, IMG, IMG, IMG, 8)])])    # another last image token
    with pytest.raises(ValueError, match="ends on an image token"):
        gen.generate_grouped(model, [(px, sizes, [good, ids(5, 6, IMG, IMG)])])
    with pytest.raises(ValueError, match="max_new_tokens"):
        gen.generate_grouped(model, [(px, sizes, [good])], max_new_tokens=0)
    with pytest.raises(ValueError, match="no image token"):
        gen.generate_grouped(model, [(px, sizes, [ids(5, 6, 7)])])
    with pytest.raises(ValueError, match=r"\[1, L\]"):
        gen.generate_grouped(model, [(px, sizes, [good[0]])])


# ----------------------------------------------------------------------------- GPU ----

@functools.lru_cache(maxsize=2)
def _gemv_case(N, K, epi):
    """max(ROWS) rows of inputs (test_gpu_gemv_batch_matches_torch's distribution) and their fp32 reference."""
    g = torch.Generator(device="cpu").manual_seed(N + K)
    wrows = 2 * N if epi == "swiglu" else N
    w = (torch.randn(wrows, K + 8, generator=g) * 0.05).bfloat16()[:, :K]   # row stride K + 8 (span views)
    x = torch.randn(max(ROWS), K, generator=g).bfloat16()
    e = torch.randn(max(ROWS), N, generator=g).bfloat16()
    nw = (1 + 0.1 * torch.randn(K, generator=g)).bfloat16()
    acc = x.float() @ w.float().t()
    if epi == "swiglu":
        ref = torch.nn.functional.silu(acc[:, :N]) * acc[:, N:]
    elif epi == "bias":
        ref = acc + e[0].float()
    elif epi == "residual":
        ref = acc + e.float()
    else:
        ref = acc
    dev = torch.device("cuda:0")
    return w.to(dev), x.to(dev), e.to(dev), nw.to(dev), ref


def _run_gemv(fn, w, x, e, N, epi, bias=None, **kw):
    if epi == "swiglu":
        return fn(x, w, swiglu_inter=N, **kw)
    if epi == "bias":
        return fn(x, w, bias=bias, **kw)
    if epi == "residual":
        return fn(x, w, residual=e.contiguous(), **kw)
    return fn(x, w, **kw)


def _check_rows_against_batch(ops, w, x, e, N, epi, rows, **kw):
    kw["bias"] = e[0].contiguous()   # the reference's bias row, whatever rows a call takes
    got = _run_gemv(ops.gemv_rows, w, x[:rows].contiguous(), e[:rows], N, epi, **kw)
    assert got.shape == (rows, N)
    for s in range(0, rows, 16):   # every 16-row slab == kd_gemv_batch on that slab
        t = min(rows, s + 16)
        slab = _run_gemv(ops.gemv_batch, w, x[s:t].contiguous(), e[s:t], N, epi, **kw)
        assert torch.equal(got[s:t], slab), (rows, s)
    if rows > 16:                  # a row of the second slab == kd_gemv_batch on it alone
        r = 16 + (rows - 17) // 4
        alone = _run_gemv(ops.gemv_batch, w, x[r:r + 1].contiguous(), e[r:r + 1], N, epi, **kw)
        assert torch.equal(got[r], alone[0]), (rows, r)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("N,K,epi", GEMV_SHAPES)
@pytest.mark.parametrize("rows", ROWS)
def test_gpu_gemv_rows_is_gemv_batch_row_by_row(rows, N, K, epi, dev):
    from importlib import import_module
    ops = import_module(f"{PKG}.ops")
    w, x, e, _, ref = _gemv_case(N, K, epi)
    got = _check_rows_against_batch(ops, w, x, e, N, epi, rows)
    torch.testing.assert_close(got.float().cpu(), ref[:rows], rtol=1e-2, atol=1e-2)


@pytest.mark.gpu
@pytest.mark.parametrize("N,K,epi", [(1152, 896, "bias"), (4864, 896, "swiglu")])
@pytest.mark.parametrize("rows", ROWS)
def test_gpu_gemv_rows_fused_rmsnorm_is_gemv_batch_row_by_row(rows, N, K, epi, dev):
    from importlib import import_module
    ops = import_module(f"{PKG}.ops")
    w, x, e, nw, _ = _gemv_case(N, K, epi)
    x = (x.float() * torch.linspace(0.5, 3.0, x.shape[0], device=x.device)[:, None]).bfloat16()   # every row its own rms
    _check_rows_against_batch(ops, w, x, e, N, epi, rows, norm_w=nw, eps=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("epi", ["residual", "bias"])
@pytest.mark.parametrize("rows", [17, 33])
def test_gpu_gemv_rows_one_tile_per_wave_plan_is_gemv_batch_slab_by_slab(rows, epi, dev):
    """N = 32776 > 32752 gives the lm_head's plan (one weight tile per wave, K not split), which
    kd_gemv_rows serves with one kd_gemv_batch pass per slab: the launcher's per-slab offsets of x, y
    and the residual (the bias must not move).  The N tail is 8 columns; K = 64 keeps the weight at 4 MB."""
    from importlib import import_module
    ops = import_module(f"{PKG}.ops")
    N, K = 32776, 64
    g = torch.Generator(device="cpu").manual_seed(N + K)
    w = (torch.randn(N, K, generator=g) * 0.05).bfloat16()
    x = torch.randn(33, K, generator=g).bfloat16()
    e = torch.randn(33, N, generator=g).bfloat16()
    got = _check_rows_against_batch(ops, w.to(dev), x.to(dev), e.to(dev), N, epi, rows)
    ref = x[:rows].float() @ w.float().t() + (e[:rows] if epi == "residual" else e[0]).float()
    torch.testing.assert_close(got.float().cpu(), ref, rtol=1e-2, atol=1e-2)


QUESTIONS = [(1, 1), (63, 2), (64, 17), (60, 10), (200, 40), (65, 1)]   # (base, S): both sides of the 64-key
SMAX = 320                                                               # boundary, straddling it, one query alone


@pytest.mark.gpu
@pytest.mark.parametrize("hd,H,HKV", [(64, 14, 2), (128, 28, 4), (64, 2, 1)])
def test_gpu_attn_extend_matches_torch(hd, H, HKV, dev):
    """One call over six questions; the suffix keys come from k_new / v_new and are stored at
    [base, base + S), nothing else in the caches changes; each question equals the same kernel run
    on it alone, and the one-row questions agree with kd_attn_decode_batch."""
    from importlib import import_module
    ops = import_module(f"{PKG}.ops")
    nb = len(QUESTIONS)
    starts = [0]
    for _, S in QUESTIONS:
        starts.append(starts[-1] + S)
    rows = starts[-1]
    g = torch.Generator(device="cpu").manual_seed(hd + H)
    q = torch.randn(H, rows, hd, generator=g).bfloat16()
    kc = torch.randn(nb, HKV, SMAX, hd, generator=g).bfloat16()
    vc = torch.randn(nb, HKV, SMAX, hd, generator=g).bfloat16()
    kn = torch.cat([kc[b, :, base:base + S] for b, (base, S) in enumerate(QUESTIONS)], 1).contiguous()   # [HKV, rows, hd]
    vn = torch.cat([vc[b, :, base:base + S] for b, (base, S) in enumerate(QUESTIONS)], 1).contiguous()
    kcd, vcd = kc.to(dev), vc.to(dev)
    for b, (base, S) in enumerate(QUESTIONS):   # the kernel must take the suffix rows from k_new / v_new ...
        kcd[b, :, base:base + S] = 0
        vcd[b, :, base:base + S] = 0
    kc0, vc0 = kcd.clone(), vcd.clone()
    row_start = torch.tensor(starts, dtype=torch.int32, device=dev)
    base_d = torch.tensor([b for b, _ in QUESTIONS], dtype=torch.int32, device=dev)
    qd, knd, vnd = q.to(dev), kn.to(dev), vn.to(dev)
    o = ops.attn_extend(qd, knd, vnd, kcd, vcd, row_start, base_d, hd)
    assert o.shape == (rows, H * hd)
    assert torch.equal(kcd.cpu(), kc) and torch.equal(vcd.cpu(), vc)   # ... store them, and touch nothing else
    rep = H // HKV
    oc = o.float().cpu()
    for b, (base, S) in enumerate(QUESTIONS):
        r0 = starts[b]
        for j in range(S):
            n = base + j + 1
            k = kc[b, :, :n].float().repeat_interleave(rep, 0)
            v = vc[b, :, :n].float().repeat_interleave(rep, 0)
            p = torch.softmax((k @ q[:, r0 + j].float()[:, :, None]).squeeze(-1) / hd ** 0.5, -1)
            ref = (p[:, None, :] @ v).squeeze(1)
            torch.testing.assert_close(oc[r0 + j].view(H, hd), ref, rtol=2e-2, atol=1e-2)
        # the question alone, in slot 0 of a one-question call: the same bits in o and in its cache
        k1, v1 = kc0[b:b + 1].clone(), vc0[b:b + 1].clone()
        alone = ops.attn_extend(qd[:, r0:r0 + S].contiguous(), knd[:, r0:r0 + S].contiguous(),
                                vnd[:, r0:r0 + S].contiguous(), k1, v1,
                                torch.tensor([0, S], dtype=torch.int32, device=dev), base_d[b:b + 1].clone(), hd)
        assert torch.equal(alone, o[r0:r0 + S]), b
        assert torch.equal(k1[0], kcd[b]) and torch.equal(v1[0], vcd[b]), b
    # the two one-row questions against the batched decode kernel on the same data
    ones = [b for b, (_, S) in enumerate(QUESTIONS) if S == 1]
    assert len(ones) == 2
    rws = [starts[b] for b in ones]
    cur = torch.tensor([QUESTIONS[b][0] + 1 for b in ones], dtype=torch.int32, device=dev)
    od = ops.attn_decode_batch(qd[:, rws].contiguous(), knd[:, rws].contiguous(), vnd[:, rws].contiguous(),
                               kc0[ones].clone(), vc0[ones].clone(), cur, hd)
    torch.testing.assert_close(o[rws].float(), od.float(), rtol=2e-2, atol=1e-2)


KW = dict(repetition_penalty=1.2, no_repeat_ngram_size=2, eos_token_id=())
P0 = 24 + 1485            # template head + the image tokens of a 336x336 prompt
SUFFIX = ((5, 27), (18,))  # group A (image seed 9): two questions; group B (image seed 11): one


@pytest.fixture(scope="module")
def run_g(dev):
    """The tiny student (test_generate_batch's run3 model), two images with 2 + 1 questions and
    their 8-token graph-replayed grouped decode, shared by the tests below."""
    from importlib import import_module
    data = import_module(f"{PKG}.data")
    gen = import_module(f"{PKG}.generation")
    M = import_module(f"{PKG}.modeling")
    cfg = M.tiny_config(False)
    model = M.LlavaOnevisionModel(cfg, dev, seed=5, cpu_rng=True)
    groups = []
    for gi, (seed, sufs) in enumerate(zip((9, 11), SUFFIX)):
        b = data.synthetic_batch(1, dev, L=P0 + max(sufs), seed=seed, pixel_dtype=torch.bfloat16, cpu_rng=True)
        ids = b["depth_input_ids"]
        assert int(ids[0, P0 - 1]) == M.IMAGE_TOKEN_ID and int(ids[0, P0]) != M.IMAGE_TOKEN_ID
        qs = []
        for qi, S in enumerate(sufs):
            g = torch.Generator().manual_seed(1000 + 10 * gi + qi)
            suf = torch.randint(0, data.TEXT_VOCAB, (1, S), generator=g, dtype=torch.int64).to(dev)
            qs.append(torch.cat([ids[:, :P0], suf], 1))
        groups.append((b["depth_pixel_values"], b["image_sizes"], qs))
    outs, logs = gen.generate_grouped(model, groups, max_new_tokens=8, return_logits=True, **KW)
    flat = [(gi, qi) for gi, (_, _, qs) in enumerate(groups) for qi in range(len(qs))]
    return dict(cfg=cfg, model=model, groups=groups, outs=outs, logs=logs, gen=gen, flat=flat)


@pytest.mark.gpu
def test_gpu_generate_grouped_matches_oracle_teacher_forced(run_g, dev):
    from model_fixtures import tiny_weights
    from oracle.model import OracleLlava
    gen, model, groups, outs, logs = (run_g[k] for k in ("gen", "model", "groups", "outs", "logs"))
    outs_e, logs_e = gen.generate_grouped(model, groups, max_new_tokens=8, return_logits=True, graph=False, **KW)
    orc = OracleLlava(tiny_weights(False, 5), run_g["cfg"])
    assert [len(o) for o in outs] == [2, 1] and [len(l) for l in logs] == [2, 1]
    for gi, qi in run_g["flat"]:
        px, sizes, qs = groups[gi]
        ids, L = qs[qi], int(qs[qi].shape[1])
        out, lgs = outs[gi][qi], logs[gi][qi]
        assert torch.equal(out, outs_e[gi][qi])               # graph replay == eager launches, bit for bit
        assert len(lgs) == len(logs_e[gi][qi]) == 8 and all(torch.equal(a, b) for a, b in zip(lgs, logs_e[gi][qi]))
        seq = out[0].cpu().tolist()
        assert out.shape == (1, L + 8) and L == P0 + SUFFIX[gi][qi]
        assert seq[:L] == ids[0].cpu().tolist()
        full, _ = orc(torch.tensor([seq[:-1]]), px.float().cpu(), sizes)
        for t, lg in enumerate(lgs):
            got = lg.float().cpu()[0]
            want = full[0, L - 1 + t]
            cos = torch.nn.functional.cosine_similarity(got, want, dim=0)
            print(f"group {gi} question {qi} step {t}: cos {float(cos):.6f} "
                  f"max|d| {float((got - want).abs().max()):.4f} max|want| {float(want.abs().max()):.4f}")
            assert cos > 0.999, (gi, qi, t, float(cos))
            assert (got - want).abs().max() < 0.05 * want.abs().max() + 0.05, (gi, qi, t)
            assert seq[L + t] == G.select(got.numpy(), seq[:L + t], 1.2, 2), (gi, qi, t)


@pytest.mark.gpu
def test_gpu_generate_grouped_question_does_not_depend_on_its_group(run_g, dev):
    gen, model, groups = run_g["gen"], run_g["model"], run_g["groups"]
    px, sizes, qs = groups[0]
    outs, logs = gen.generate_grouped(model, [(px, sizes, [qs[1]])], max_new_tokens=8, return_logits=True, **KW)
    assert len(outs) == 1 and len(outs[0]) == 1 and torch.equal(outs[0][0], run_g["outs"][0][1])
    assert len(logs[0][0]) == 8 and all(torch.equal(a, b) for a, b in zip(logs[0][0], run_g["logs"][0][1]))


@pytest.mark.gpu
def test_gpu_generate_grouped_first_step_is_close_to_generate_batch(run_g, dev):
    """Same oracle bounds, not the same bits: only the first logits row is compared (a near tie may
    fall the other way, after which the sequences differ legitimately)."""
    gen, model, groups = run_g["gen"], run_g["model"], run_g["groups"]
    prompts = [(ids, px, sizes) for px, sizes, qs in groups for ids in qs]
    _, logs = gen.generate_batch(model, prompts, max_new_tokens=1, return_logits=True, **KW)
    for r, (gi, qi) in enumerate(run_g["flat"]):
        a, b = run_g["logs"][gi][qi][0].float()[0], logs[r][0].float()[0]
        cos = torch.nn.functional.cosine_similarity(a, b, dim=0)
        assert cos > 0.999, (gi, qi, float(cos))


@pytest.mark.gpu
def test_gpu_generate_grouped_cuts_every_question_after_its_own_eos(run_g, dev):
    gen, model, groups = run_g["gen"], run_g["model"], run_g["groups"]
    L1 = P0 + SUFFIX[0][1]
    eos = run_g["outs"][0][1][0].cpu().tolist()[L1 + 2]   # pretend the token question A.2 produced third is EOS
    cut = gen.generate_grouped(model, groups, max_new_tokens=8, repetition_penalty=1.2, no_repeat_ngram_size=2,
                               eos_token_id=(eos,))
    for gi, qi in run_g["flat"]:
        L = P0 + SUFFIX[gi][qi]
        full = run_g["outs"][gi][qi][0].cpu().tolist()
        new = full[L:]
        want = full[:L + new.index(eos) + 1] if eos in new else full
        assert cut[gi][qi][0].cpu().tolist() == want, (gi, qi)
    assert cut[0][1].shape[1] <= L1 + 3 and int(cut[0][1][0, -1]) == eos


@pytest.mark.gpu
def test_gpu_generate_grouped_chunks_of_16_keep_the_prefix(run_g, dev):
    """17 copies of one question: the group spans two chunks, the second reuses the prefix K/V."""
    gen, model, groups = run_g["gen"], run_g["model"], run_g["groups"]
    px, sizes, qs = groups[0]
    outs = gen.generate_grouped(model, [(px, sizes, [qs[0]] * 17)], max_new_tokens=3, **KW)
    assert len(outs) == 1 and len(outs[0]) == 17
    L = P0 + SUFFIX[0][0]
    assert torch.equal(outs[0][0], outs[0][16]) and torch.equal(outs[0][0], run_g["outs"][0][0][:, :L + 3])
