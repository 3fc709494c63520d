"""generate_batch(): batched greedy decode over ragged prompts.  The batched kernels against torch
fp32 / the CPU oracle, batch invariance (a row's bits do not depend on nb, on the other rows or on
its slot) by torch.equal, and the whole batched decode against the CPU oracle model teacher-forced
on every row's own generated sequence (GPU); argument validation of the new entry points (CPU)."""
import ctypes
import functools

import pytest
import torch

from oracle import generation as G
from test_generate import CASES, _seq_scores

PKG = "knowledge_distillation_for_sensory_substitution_in_multimodal_models_amd"

GEMV_SHAPES = [(1152, 896, "bias"), (896, 4864, "residual"), (4864, 896, "swiglu"), (151936, 896, "none"),
               (21, 40, "none")]   # (21, 40): the smallest shape with both an N tail and a K tail


# ----------------------------------------------------------------------------- CPU ----

def test_abi_batch_symbols_reject_bad_arguments():
    """Validation runs before any device work: null pointers -> KD_ERR_ARG (7), bad shapes ->
    KD_ERR_SHAPE (1), a short workspace -> KD_ERR_WORKSPACE (8) (host memory stands in for the
    pointers: it is never dereferenced)."""
    from importlib import import_module
    lib = import_module(f"{PKG}._native").lib()
    assert lib.kd_gemv_batch(None, 8, 1, None, 8, None, None, 4, 8, 0, 0, None, 1e-6, None, 0, None) == 7
    assert lib.kd_attn_decode_batch(None, None, None, None, None, None, 1, 2, 1, 64, 64, 8, None, None, 0, None) == 7
    assert lib.kd_gen_select_batch(None, 10, 10, None, 8, 1, None, 1.2, 2, None, 0, None, None) == 7
    assert lib.kd_rope_rows(None, None, 32, 8, 1, None, None, None, None) == 7
    buf = ctypes.create_string_buffer(256 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    assert lib.kd_gemv_batch(p, 8, 17, p, 8, None, p, 4, 8, 0, 0, None, 1e-6, None, 0, None) == 1     # nb > 16
    assert lib.kd_gemv_batch(p, 8, 1, p, 8, None, p, 4, 12, 0, 0, None, 1e-6, None, 0, None) == 1     # K % 8
    assert lib.kd_gemv_batch(p, 4864, 1, p, 4864, p, p, 896, 4864, 2, 0, None, 1e-6, None, 0, None) == 8   # K split
    assert lib.kd_attn_decode_batch(p, p, p, p, p, p, 1, 2, 1, 96, 96, 8, p, p, 0, None) == 1         # head dim
    assert lib.kd_attn_decode_batch(p, p, p, p, p, p, 2, 2, 1, 64, 64, 8, p, p, 16, None) == 8
    assert lib.kd_gen_select_batch(p, 10, 10, p, 8, 0, p, 1.2, 2, p, 256, None, None) == 1            # nb < 1
    assert lib.kd_gen_select_batch(p, 10, 10, p, 8, 2, p, 1.2, 2, p, 19, None, None) == 8             # < nb * V
    assert lib.kd_rope_rows(p, p, 0, 8, 1, p, p, p, None) == 1
    # the launch plan is a function of the layer's shape only
    assert lib.kd_gemv_batch_workspace_size(896, 4864, 2) > 0
    assert lib.kd_attn_decode_batch_workspace_size(4, 14, 64, 1568) == 4 * lib.kd_attn_decode_workspace_size(14, 64, 1568)


# ----------------------------------------------------------------------------- GPU ----

@functools.lru_cache(maxsize=2)
def _gemv_case(N, K, epi):
    """16 rows of inputs (test_gpu_gemv_matches_torch's distribution) and their fp32 reference."""
    g = torch.Generator(device="cpu").manual_seed(N + K)
    rows = 2 * N if epi == "swiglu" else N
    w = (torch.randn(rows, K + 8, generator=g) * 0.05).bfloat16()[:, :K]   # row stride K + 8 (span views)
    x = torch.randn(16, K, generator=g).bfloat16()
    e = torch.randn(16, N, generator=g).bfloat16()
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
    return w.to(dev), x.to(dev), e.to(dev), ref


def _run_gemv(ops, w, x, e, N, epi, **kw):
    if epi == "swiglu":
        return ops.gemv_batch(x, w, swiglu_inter=N, **kw)
    if epi == "bias":
        return ops.gemv_batch(x, w, bias=e[0].contiguous(), **kw)
    if epi == "residual":
        return ops.gemv_batch(x, w, residual=e[:x.shape[0]].contiguous(), **kw)
    return ops.gemv_batch(x, w, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("N,K,epi", GEMV_SHAPES)
@pytest.mark.parametrize("nb", [1, 3, 16])
def test_gpu_gemv_batch_matches_torch(nb, N, K, epi, dev):
    from importlib import import_module
    ops = import_module(f"{PKG}.ops")
    w, x, e, ref = _gemv_case(N, K, epi)
    got = _run_gemv(ops, w, x[:nb].contiguous(), e, N, epi)
    assert got.shape == (nb, N)
    torch.testing.assert_close(got.float().cpu(), ref[:nb], rtol=1e-2, atol=1e-2)


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", [(1152, 896), (151936, 896), (4864, 896)])
def test_gpu_gemv_batch_fused_rmsnorm_matches_norm_then_gemv(N, K, dev):
    """The per-row fused RMSNorm prologue against kd_norm_fwd followed by the unfused call."""
    from importlib import import_module
    ops = import_module(f"{PKG}.ops")
    g = torch.Generator(device="cpu").manual_seed(K + N)
    x = (torch.randn(3, K, generator=g) * torch.tensor([[3.0], [0.5], [1.0]])).bfloat16().to(dev)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).bfloat16().to(dev)
    w = (torch.randn(N, K, generator=g) * 0.05).bfloat16().to(dev)
    h, _, _ = ops.norm_fwd(x, nw, None, 1e-6, rms=True, save_stats=False)
    ref = ops.gemv_batch(h, w).float()
    got = ops.gemv_batch(x, w, norm_w=nw, eps=1e-6).float()
    torch.testing.assert_close(got, ref, rtol=2e-2, atol=2e-2)
    # and the fused form is batch invariant as well
    alone = ops.gemv_batch(x[1:2].contiguous(), w, norm_w=nw, eps=1e-6).float()
    assert torch.equal(alone, got[1:2])


@pytest.mark.gpu
@pytest.mark.parametrize("N,K,epi", GEMV_SHAPES)
def test_gpu_gemv_batch_is_batch_invariant(N, K, epi, dev):
    """Row r of an nb = 16 call == the nb = 1 call on that row alone == the same row in another slot
    of an nb = 3 call, bit for bit."""
    from importlib import import_module
    ops = import_module(f"{PKG}.ops")
    w, x, e, _ = _gemv_case(N, K, epi)
    full = _run_gemv(ops, w, x, e, N, epi)
    for r, slot in ((0, 2), (5, 1), (15, 0)):
        alone = _run_gemv(ops, w, x[r:r + 1].contiguous(), e[r:r + 1] if epi == "residual" else e, N, epi)
        assert torch.equal(alone[0], full[r]), (r, "nb = 1")
        pick = [7, 9, 11]
        pick[slot] = r
        three = _run_gemv(ops, w, x[pick].contiguous(), e[pick] if epi == "residual" else e, N, epi)
        assert torch.equal(three[slot], full[r]), (r, slot, "nb = 3")


@pytest.mark.gpu
@pytest.mark.parametrize("hd,H,HKV", [(64, 14, 2), (128, 28, 4), (64, 2, 1)])
def test_gpu_attn_decode_batch_matches_torch(hd, H, HKV, dev):
    """One batch with per-row lengths on both sides of the 64-key chunk boundary and over several
    chunks; the own row comes from k_new / v_new and is stored at cur[b] - 1, nothing else in the
    caches changes, and each row equals the same kernel run on that row alone."""
    from importlib import import_module
    ops = import_module(f"{PKG}.ops")
    lens = [1, 63, 64, 65, 200]
    nb, smax = len(lens), 256
    g = torch.Generator(device="cpu").manual_seed(hd + H)
    q = torch.randn(H, nb, hd, generator=g).bfloat16()
    kc = torch.randn(nb, HKV, smax, hd, generator=g).bfloat16()
    vc = torch.randn(nb, HKV, smax, hd, generator=g).bfloat16()
    kn = torch.stack([kc[b, :, n - 1] for b, n in enumerate(lens)], 1).contiguous()   # [HKV, nb, hd]
    vn = torch.stack([vc[b, :, n - 1] for b, n in enumerate(lens)], 1).contiguous()
    kcd, vcd = kc.to(dev), vc.to(dev)
    for b, n in enumerate(lens):   # the kernel must take the token's own row from k_new / v_new ...
        kcd[b, :, n - 1] = 0
        vcd[b, :, n - 1] = 0
    kc0, vc0 = kcd.clone(), vcd.clone()
    cur = torch.tensor(lens, dtype=torch.int32, device=dev)
    o = ops.attn_decode_batch(q.to(dev), kn.to(dev), vn.to(dev), kcd, vcd, cur, hd)
    assert torch.equal(cur.cpu(), torch.tensor(lens, dtype=torch.int32))
    assert torch.equal(kcd.cpu(), kc) and torch.equal(vcd.cpu(), vc)   # ... store it, and touch nothing else
    rep = H // HKV
    for b, n in enumerate(lens):
        k = kc[b, :, :n].float().repeat_interleave(rep, 0)
        v = vc[b, :, :n].float().repeat_interleave(rep, 0)
        p = torch.softmax((k @ q[:, b].float()[:, :, None]).squeeze(-1) / hd ** 0.5, -1)
        ref = (p[:, None, :] @ v).squeeze(1)
        torch.testing.assert_close(o[b].float().cpu().view(H, hd), ref, rtol=2e-2, atol=1e-2)
        k1, v1 = kc0[b:b + 1].clone(), vc0[b:b + 1].clone()
        alone = ops.attn_decode_batch(q[:, b:b + 1].contiguous().to(dev), kn[:, b:b + 1].contiguous().to(dev),
                                      vn[:, b:b + 1].contiguous().to(dev), k1, v1, cur[b:b + 1].clone(), hd)
        assert torch.equal(alone[0], o[b]), b
        assert torch.equal(k1[0], kcd[b]) and torch.equal(v1[0], vcd[b])


@pytest.mark.gpu
@pytest.mark.parametrize("penalty,ngram", CASES)
def test_gpu_gen_select_batch_matches_oracle(penalty, ngram, dev):
    from importlib import import_module
    ops = import_module(f"{PKG}.ops")
    rows = [_seq_scores(100 * seed + ngram, n=200 + 37 * seed) for seed in range(4)]
    lens = [len(s) for s, _ in rows]
    smax = max(lens) + 3
    seq = torch.zeros((4, smax), dtype=torch.int64)
    for b, (s, _) in enumerate(rows):
        seq[b, :lens[b]] = torch.tensor(s)
    lg = torch.stack([torch.from_numpy(sc).bfloat16() for _, sc in rows])
    seq_d = seq.to(dev)
    cur = torch.tensor(lens, dtype=torch.int32, device=dev)
    out = torch.empty(4, dtype=torch.int64, device=dev)
    ops.gen_select_batch(lg.to(dev), seq_d, cur, penalty, ngram, out=out)
    assert cur.cpu().tolist() == [n + 1 for n in lens]
    for b, (s, _) in enumerate(rows):
        want = G.select(lg[b].float().numpy(), s, penalty, ngram)
        assert int(out[b]) == want == int(seq_d[b, lens[b]]), b
        assert torch.equal(seq_d[b, :lens[b]].cpu(), seq[b, :lens[b]])


KW = dict(repetition_penalty=1.2, no_repeat_ngram_size=2, eos_token_id=())
LENS = (1490, 1536, 1511)   # just above the 1,485 image tokens of a 336x336 prompt


@pytest.fixture(scope="module")
def run3(dev):
    """The tiny student (real vocab, real 336x336 token layout), three ragged prompts with different
    seeds and their 8-token graph-replayed batched decode, shared by the tests below."""
    from importlib import import_module
    data = import_module(f"{PKG}.data")
    gen = import_module(f"{PKG}.generation")
    M = import_module(f"{PKG}.modeling")
    cfg = M.tiny_config(False)
    model = M.LlavaOnevisionModel(cfg, dev, seed=5, cpu_rng=True)
    prompts = []
    for i, L in enumerate(LENS):
        b = data.synthetic_batch(1, dev, L=L, seed=9 + 2 * i, pixel_dtype=torch.bfloat16, cpu_rng=True)
        prompts.append((b["depth_input_ids"], b["depth_pixel_values"], b["image_sizes"]))
    outs, logs = gen.generate_batch(model, prompts, max_new_tokens=8, return_logits=True, **KW)
    return dict(cfg=cfg, model=model, prompts=prompts, outs=outs, logs=logs, gen=gen)


@pytest.mark.gpu
def test_gpu_generate_batch_matches_oracle_teacher_forced(run3, dev):
    from model_fixtures import tiny_weights
    from oracle.model import OracleLlava
    gen, model, prompts, outs, logs = (run3[k] for k in ("gen", "model", "prompts", "outs", "logs"))
    outs_e, logs_e = gen.generate_batch(model, prompts, max_new_tokens=8, return_logits=True, graph=False, **KW)
    orc = OracleLlava(tiny_weights(False, 5), run3["cfg"])
    for r, L in enumerate(LENS):
        assert torch.equal(outs[r], outs_e[r])               # graph replay == eager launches, bit for bit
        assert len(logs[r]) == len(logs_e[r]) == 8 and all(torch.equal(a, b) for a, b in zip(logs[r], logs_e[r]))
        seq = outs[r][0].cpu().tolist()
        assert outs[r].shape == (1, L + 8)
        ids, px, sizes = prompts[r]
        assert seq[:L] == ids[0].cpu().tolist()
        full, _ = orc(torch.tensor([seq[:-1]]), px.float().cpu(), sizes)
        for t, lg in enumerate(logs[r]):
            got = lg.float().cpu()[0]
            want = full[0, L - 1 + t]
            cos = torch.nn.functional.cosine_similarity(got, want, dim=0)
            assert cos > 0.999, (r, t, float(cos))
            assert (got - want).abs().max() < 0.05 * want.abs().max() + 0.05, (r, t)
            assert seq[L + t] == G.select(got.numpy(), seq[:L + t], 1.2, 2), (r, t)
        # the prefill is generate()'s own code: first token and first logits row, bit for bit
        one, one_lg = gen.generate(model, ids, px, sizes, max_new_tokens=1, return_logits=True, **KW)
        assert torch.equal(one, outs[r][:, :L + 1]) and torch.equal(one_lg[0], logs[r][0])


@pytest.mark.gpu
def test_gpu_generate_batch_row_does_not_depend_on_the_batch(run3, dev):
    gen, model, prompts = run3["gen"], run3["model"], run3["prompts"]
    outs, logs = gen.generate_batch(model, [prompts[1]], max_new_tokens=8, return_logits=True, **KW)
    assert len(outs) == 1 and torch.equal(outs[0], run3["outs"][1])
    assert len(logs[0]) == 8 and all(torch.equal(a, b) for a, b in zip(logs[0], run3["logs"][1]))


@pytest.mark.gpu
def test_gpu_generate_batch_cuts_every_row_after_its_own_eos(run3, dev):
    gen, model, prompts = run3["gen"], run3["model"], run3["prompts"]
    full = [o[0].cpu().tolist() for o in run3["outs"]]
    eos = full[1][LENS[1] + 2]   # pretend the token row 1 produced third is EOS
    cut = gen.generate_batch(model, prompts, max_new_tokens=8, repetition_penalty=1.2, no_repeat_ngram_size=2,
                             eos_token_id=(eos,))
    for r, L in enumerate(LENS):
        new = full[r][L:]
        want = full[r][:L + new.index(eos) + 1] if eos in new else full[r]
        assert cut[r][0].cpu().tolist() == want, r
    assert cut[1].shape[1] <= LENS[1] + 3 and int(cut[1][0, -1]) == eos


@pytest.mark.gpu
def test_gpu_generate_batch_chunks_of_16_and_empty_list(run3, dev):
    gen, model, prompts = run3["gen"], run3["model"], run3["prompts"]
    outs = gen.generate_batch(model, [prompts[0]] * 17, max_new_tokens=3, **KW)
    assert len(outs) == 17
    assert torch.equal(outs[0], outs[16]) and torch.equal(outs[0], run3["outs"][0][:, :LENS[0] + 3])
    with pytest.raises(ValueError):
        gen.generate_batch(model, [])
