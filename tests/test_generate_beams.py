"""num_beams: beam search inside the captured decode step (kd_gen_beam_topk, kd_gen_beam_step, kd_kv_beam_reorder,
num_beams= / length_penalty= / early_stopping= of generate() / generate_batch() / generate_grouped()).
CPU: the reference (beam_ref) against transformers' own generate(num_beams=...) on a random tiny Qwen2, our tie
rules (torch.topk leaves ties unspecified: the rules are this project's, stated in beam_ref), argument validation
of the C ABI and of the entry points.  GPU: the three kernels against the float64 reference, torch.index_select and
the fp32 restatement of the step; the entry points on the tiny student, replayed step by step by the reference on
the returned rows, held to the oracle model, and bit for bit across their routes."""
import ctypes
import itertools
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import beam_ref as R
from test_generate import CASES
from test_generate_batch import LENS, run3   # noqa: F401  (fixture)
from test_generate_grouped import run_g      # noqa: F401  (fixture)

PKG = "knowledge_distillation_for_sensory_substitution_in_multimodal_models_amd"
V = 151936
NEG = -np.inf
EPS = R.EPS


# ----------------------------------------------------------------------------- CPU ----

def _tiny_qwen2(seed):
    from transformers import Qwen2Config, Qwen2ForCausalLM
    cfg = Qwen2Config(vocab_size=61, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=64, pad_token_id=60, tie_word_embeddings=False)
    torch.manual_seed(seed)
    model = Qwen2ForCausalLM(cfg).eval()
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(3.0)
    return model


def _model_logits(model):
    def fn(run_seq, step):
        with torch.no_grad():
            return model(torch.tensor(run_seq)).logits[:, -1].double().numpy()
    return fn


SETTINGS = [(K, n_eos, pn) for K in (2, 3, 4, 5) for n_eos in (1, 2) for pn in ((1.2, 2), (1.0, 0), (1.5, 3))]
LENGTH_PENALTIES = (1.0, 0.0, 2.0)
MUST_END_ON_EOS = [i % 2 == 0 for i in range(len(SETTINGS))]   # half of the cases: more than the third asked for


def _pick(case):
    """The model seed and EOS ids of a case, from the reference alone: the first seed whose margin exceeds 1e-4
    (and, where the case must, whose result ends on an EOS before max_new_tokens).  The EOS ids are tokens the
    EOS-free search of that seed generates, so that an early end is likely."""
    K, n_eos, (penalty, ngram) = SETTINGS[case]
    lp = LENGTH_PENALTIES[case % 3]
    for seed in range(100 * case, 100 * case + 60):
        model = _tiny_qwen2(seed)
        prompt = np.random.default_rng(seed).integers(0, 60, 5 + seed % 4).tolist()   # never the pad id 60
        kw = dict(K=K, max_new=10, penalty=penalty, ngram=ngram, length_penalty=lp)
        free = R.search(_model_logits(model), prompt, eos=(), **kw)
        new = free["seq"][len(prompt):]
        eos = [new[3]] if n_eos == 1 else [new[3], new[6]]
        if len(set(eos)) != n_eos or 60 in eos:
            continue
        ref = R.search(_model_logits(model), prompt, eos=eos, **kw)
        if ref["margin"] > 1e-4 and (ref["on_eos"] or not MUST_END_ON_EOS[case]):
            return model, prompt, eos, kw, ref
    raise AssertionError("no seed with the margin")


@pytest.mark.parametrize("case", range(len(SETTINGS)))
def test_reference_matches_transformers_beam_search(case):
    """24 settings: K in {2, 3, 4, 5}, one or two EOS ids, three (penalty, n-gram) pairs, length_penalty cycling
    through {1, 0, 2}, 10 new tokens; prompts without the pad id (transformers would infer an attention mask)."""
    model, prompt, eos, kw, ref = _pick(case)
    assert ref["on_eos"] or not MUST_END_ON_EOS[case]
    out = model.generate(torch.tensor([prompt]), num_beams=kw["K"], do_sample=False, early_stopping=False,
                         max_new_tokens=10, eos_token_id=eos, pad_token_id=60, repetition_penalty=kw["penalty"],
                         no_repeat_ngram_size=kw["ngram"], length_penalty=kw["length_penalty"], num_return_sequences=1,
                         output_scores=True, return_dict_in_generate=True)
    hf = out.sequences[0].tolist()
    n = len(ref["seq"])
    assert hf[:n] == ref["seq"] and all(t == 60 for t in hf[n:]), (hf, ref["seq"])
    assert abs(float(out.sequences_scores[0]) - ref["score"]) < 1e-4


def test_at_least_a_third_of_the_cases_end_on_an_eos():
    assert 3 * sum(MUST_END_ON_EOS) >= len(SETTINGS) == 24


def _rows_fn(rows_per_step):
    return lambda run_seq, step: np.asarray(rows_per_step[step], dtype=np.float64)


def test_tie_rules_equal_tokens_across_beams_and_equal_scores_inside_a_beam():
    """Our rules (torch.topk has none): larger score, then lower beam, then lower token."""
    row = np.full(12, -4.0)
    row[[2, 7]] = 1.0                                    # two equal maxima inside every beam
    st = R.State([3, 3], 2)
    st.run_score = [-1.0, -1.0]                          # equal beams: equal (beam, token) scores across beams
    cand, margin, _, _ = R.candidates(np.stack([row, row]), st.run_seq, st.run_score, 4)
    assert [(j, t) for _, j, t, _ in cand] == [(0, 2), (0, 7), (1, 2), (1, 7)] and margin == 0.0
    assert cand[0][0] == cand[3][0]
    # the running cut between equal r goes to the lower candidate rank
    parents, tokens, _ = R.advance(st, cand, set(), 10, R.den_table(8, 1.0))
    assert parents == [0, 0] and tokens == [2, 7]
    # a killed beam ties at -1e9 exactly (fp32 absorbs the log-probability): lower beam, then lower token
    st = R.State([3], 3)
    cand, _, _, _ = R.candidates(np.stack([np.array([0.0, NEG, NEG])] * 3), st.run_seq, st.run_score, 3)
    assert [(j, t) for _, j, t, _ in cand] == [(0, 0), (1, 0), (2, 0)] and cand[1][0] == cand[2][0] == R.KILL
    # an entry at -inf carries token 0
    assert R.row_top(np.array([NEG, 1.0, NEG]), 3) == ([1.0, NEG, NEG], [1, 0, 0], NEG)


def test_tie_rules_a_finished_tie_keeps_the_earlier_entry():
    """Finished set: larger score, then the earlier entry of (stored ++ candidates); the flag travels along."""
    st = R.State([9], 2)
    den = R.den_table(8, 0.0)                            # length_penalty 0: den = 1, scores compare as they are
    cand = [(-1.0, 0, 5), (-1.0, 0, 6), (-3.0, 0, 1), (-3.5, 0, 2)]
    R.advance(st, cand, {5, 6}, 20, den)                 # both EOS candidates finish with the same score
    assert [(s, f, q[-1]) for s, f, q in st.fin] == [(-1.0, True, 5), (-1.0, True, 6)]
    assert st.run_seq == [[9, 1], [9, 2]] and st.run_score == [-3.0, -3.5]
    cand = [(-1.0, 0, 5), (-4.0, 1, 3), (-5.0, 0, 4), (-6.0, 1, 4)]
    R.advance(st, cand, {5, 6}, 20, den)                 # a third hypothesis at -1.0: the stored ones stay
    assert [(s, f, q) for s, f, q in st.fin] == [(-1.0, True, [9, 5]), (-1.0, True, [9, 6])]
    assert not st.unsat and st.done                      # best -4.0 against worst -1.0


def test_advance_in_fp32_and_float64_agree_on_representable_candidates():
    den = R.den_table(8, 2.0)
    for ft in (np.float64, np.float32):
        st = R.State([1, 2], 2)
        R.advance(st, [(-0.5, 0, 7), (-1.5, 0, 3), (-2.0, 0, 4), (-2.5, 0, 5)], {7}, 12, den, ft=ft)
        assert st.fin[0] == (-0.5, True, [1, 2, 7]) and st.fin[1][1] is False and st.fin[1][0] == R.KILL
        assert st.run_seq == [[1, 2, 3], [1, 2, 4]] and st.run_score == [-1.5, -2.0] and st.unsat


def _abi():
    NV = import_module(f"{PKG}._native")
    buf = ctypes.create_string_buffer(256 + 16)
    return NV, NV.lib(), buf, (ctypes.addressof(buf) + 15) & ~15


def test_abi_gen_beam_topk_rejects_bad_arguments():
    """Validation runs before any device work (host memory stands in for the pointers: it is never
    dereferenced): KD_ERR_ARG = 7, KD_ERR_SHAPE = 1, KD_ERR_WORKSPACE = 8."""
    NV, lib, buf, p = _abi()
    assert NV.KD_GEN_BEAMS_MAX == 8 and NV.ABI_VERSION == 9
    size = lib.kd_gen_beam_topk_workspace_size
    assert 0 < size(1, 13) <= size(1, 4097) < size(1, V) and size(16, V) == 16 * size(1, V)
    assert size(0, V) == 0 and size(1, 0) == 0 and size(1, 2 ** 18 + 1) == 0
    big = size(1, 8)

    def call(logits=p, ld=8, N=8, ids=None, A=0, seq=p, smax=16, nb=1, cur=p, run=p, penalty=1.2, ngram=2, M=4, ws=p,
             wsb=big, cs=p, ct=p):
        return lib.kd_gen_beam_topk(logits, ld, N, ids, A, seq, smax, nb, cur, run, penalty, ngram, M, ws, wsb, cs, ct, None)

    for name in ("logits", "seq", "cur", "run", "ws", "cs", "ct"):
        assert call(**{name: None}) == 7, name
    assert b"null" in lib.kd_last_error()
    assert call(penalty=0.0) == 7 and call(penalty=-1.0) == 7 and call(ngram=-1) == 7
    assert call(nb=0) == 1 and call(nb=17, wsb=17 * big) == 1
    assert call(N=0) == 1 and call(N=2 ** 18 + 1, ld=2 ** 18 + 1, wsb=2 ** 40) == 1
    assert call(smax=0) == 1 and call(ld=7) == 1
    assert call(M=0) == 1 and call(M=73) == 1 and call(ids=p, A=0) == 1 and call(ids=p, A=9) == 1
    assert call(wsb=big - 1) == 8 and call(nb=2, wsb=big) == 8
    assert b"workspace" in lib.kd_last_error()


def test_abi_gen_beam_step_and_kv_beam_reorder_reject_bad_arguments():
    NV, lib, buf, p = _abi()

    def step(M=4, K=2, P=1, smax=16, max_new=8, n_eos=1, **holes):
        names = ("cs", "ct", "seq", "cur", "run", "out", "parent", "fin_seq", "fin_score", "fin_len", "open", "live",
                 "den", "eos", "plen")
        a = {n: holes.get(n, p) for n in names}
        return lib.kd_gen_beam_step(a["cs"], a["ct"], M, K, P, a["seq"], smax, a["cur"], a["run"], a["out"], a["parent"],
                                    a["fin_seq"], a["fin_score"], a["fin_len"], a["open"], a["live"], a["den"], max_new,
                                    a["eos"], n_eos, a["plen"], None)

    for name in ("cs", "ct", "seq", "cur", "run", "out", "parent", "fin_seq", "fin_score", "fin_len", "open", "live",
                 "den", "eos", "plen"):
        assert step(**{name: None}) == 7, name
    assert b"null" in lib.kd_last_error()
    assert step(K=0) == 1 and step(K=9, M=18) == 1 and step(K=3, M=2) == 1 and step(M=73) == 1
    assert step(P=0) == 1 and step(P=33) == 1 and step(n_eos=-1) == 1 and step(n_eos=9) == 1
    assert step(max_new=0) == 1 and step(max_new=17) == 1 and step(smax=0) == 1
    assert step(K=8, M=16, smax=1024, max_new=513) == 1        # the windows no longer fit the LDS

    def reorder(layers=2, P=1, K=3, HKV=2, smax=24, hd=64, tail=8, **holes):
        a = {n: holes.get(n, p) for n in ("kc", "vc", "parent", "cur", "plen")}
        return lib.kd_kv_beam_reorder(a["kc"], a["vc"], layers, P, K, HKV, smax, hd, a["parent"], a["cur"], a["plen"],
                                      tail, None)

    for name in ("kc", "vc", "parent", "cur", "plen"):
        assert reorder(**{name: None}) == 7, name
    assert reorder(hd=96) == 1 and reorder(hd=0) == 1 and reorder(K=0) == 1 and reorder(K=9) == 1 and reorder(P=0) == 1
    assert reorder(layers=0) == 1 and reorder(HKV=0) == 1 and reorder(smax=0) == 1 and reorder(tail=0) == 1
    assert reorder(tail=25) == 1


def _stub_calls():
    gen = import_module(f"{PKG}.generation")
    IMG = import_module(f"{PKG}.modeling").IMAGE_TOKEN_ID
    stub = SimpleNamespace(cfg=SimpleNamespace(text=SimpleNamespace(vocab=V, hidden=896), image_token_id=IMG))
    ids = torch.tensor([[5, 6, IMG, IMG, 7, 8]], dtype=torch.int64)
    px, sizes = torch.zeros(1, 2, 3, 384, 384), torch.tensor([[336, 336]])
    return ((lambda **kw: gen.generate(stub, ids, px, sizes, **kw)),
            (lambda **kw: gen.generate_batch(stub, [(ids, px, sizes)] * 2, **kw)),
            (lambda **kw: gen.generate_grouped(stub, [(px, sizes, [ids]), (px, sizes, [ids])], **kw)))


BAD = [("num_beams", dict(num_beams=0)), ("num_beams", dict(num_beams=9)), ("num_beams", dict(num_beams=2.0)),
       ("num_beams", dict(num_beams=True)), ("num_beams", dict(num_beams=-1)),
       ("length_penalty", dict(num_beams=2, length_penalty=float("nan"))),
       ("length_penalty", dict(num_beams=2, length_penalty=float("inf"))),
       ("length_penalty", dict(num_beams=2, length_penalty="1")),
       ("early_stopping", dict(num_beams=2, early_stopping=True)),
       ("early_stopping", dict(num_beams=2, early_stopping="never")),
       ("do_sample", dict(num_beams=2, do_sample=True)),
       ("restrict_head", dict(num_beams=2, restrict_head=True, allowed_token_ids=[1, 2, 3])),
       ("EOS", dict(num_beams=2, eos_token_id=tuple(range(100, 109)))),
       ("max_new_tokens", dict(num_beams=8, max_new_tokens=513)), ("max_new_tokens", dict(num_beams=2, max_new_tokens=2049))]


def test_entry_points_refuse_bad_beam_arguments_before_any_device_work():
    """A model stub with nothing but the sizes: the checks come first.  With num_beams = 1 the other two
    arguments are ignored: the stub then fails where the plain call fails on it, at its first use of the model."""
    for call in _stub_calls():
        for word, kw in BAD:
            with pytest.raises(ValueError, match=word):
                call(**kw)
        for kw in (dict(), dict(num_beams=1, length_penalty=float("nan"), early_stopping=True),
                   dict(num_beams=2, length_penalty=0.0, eos_token_id=tuple(range(100, 108)))):
            with pytest.raises(AttributeError):
                call(**kw)


# ----------------------------------------------------------------- GPU, kernel level ----

def _bf16(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float32)).bfloat16()


def _topk(dev, rows, seqs, run_score, M, ids=None, penalty=1.0, ngram=0):
    """ops.gen_beam_topk over rows [nb, V] (bf16 tensor) -> (scores [nb, M], tokens [nb, M]) on the host; seq and cur
    must come back untouched."""
    ops = import_module(f"{PKG}.ops")
    nb = rows.shape[0]
    smax = max(len(s) for s in seqs) + 3
    seq = torch.full((nb, smax), -3, dtype=torch.int64)
    for b, s in enumerate(seqs):
        seq[b, :len(s)] = torch.tensor(s, dtype=torch.int64)
    cur = torch.tensor([len(s) for s in seqs], dtype=torch.int32)
    seq_d, cur_d = seq.to(dev), cur.to(dev)
    sc, tk = ops.gen_beam_topk(rows.to(dev), seq_d, cur_d, torch.tensor(run_score, dtype=torch.float32, device=dev), M,
                               ids=None if ids is None else torch.tensor(ids, dtype=torch.int32, device=dev),
                               repetition_penalty=penalty, no_repeat_ngram_size=ngram)
    torch.cuda.synchronize()
    assert torch.equal(seq_d.cpu(), seq) and torch.equal(cur_d.cpu(), cur)
    return sc.cpu().numpy(), tk.cpu().numpy()


def _check_row(got_s, got_t, row, seq, rs, M, ids, penalty, ngram):
    """One row of kd_gen_beam_topk against the float64 reference: every score within EPS, the set by margin."""
    l, _ = R.log_probs(row.float().numpy(), seq, penalty, ngram, ids)
    acc = R.accumulate(l, float(np.float32(rs)))
    ref_s, ref_t, _ = R.row_top(acc, M)
    n_fin = int(np.sum(np.asarray(ref_s) > NEG))
    assert int(np.sum(got_s > NEG)) == n_fin
    assert np.all(got_s[n_fin:] == NEG) and np.all(got_t[n_fin:] == 0)
    toks = got_t[:n_fin]
    assert len(set(toks.tolist())) == n_fin and np.all(acc[toks] > NEG)
    assert np.abs(got_s[:n_fin] - acc[toks]).max(initial=0.0) <= EPS
    assert np.all(np.diff(got_s[:n_fin]) <= 0)
    for a in range(n_fin - 1):                                # equal scores: the lower token first
        assert got_s[a] > got_s[a + 1] or toks[a] < toks[a + 1]
    if n_fin:
        cut = ref_s[n_fin - 1]
        assert acc[toks].min() >= cut - EPS
        rest = acc.copy()
        rest[toks] = NEG
        assert n_fin < M or rest.max() <= cut + EPS
    return float(np.abs(got_s[:n_fin] - acc[toks]).max(initial=0.0))


def _case_rows(Vv, nb, seed):
    g = torch.Generator().manual_seed(seed)
    rows = (torch.randn(nb, Vv, generator=g) * 4.0).bfloat16()
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(0, min(50, Vv), 40 + 7 * b).tolist() for b in range(nb)]   # many repeats and bigram hits
    run = (-rng.random(nb) * 400.0).astype(np.float32).tolist()
    return rows, seqs, run


@pytest.mark.gpu
@pytest.mark.parametrize("M", [4, 72])
@pytest.mark.parametrize("nb", [1, 3, 16])
@pytest.mark.parametrize("Vv", [13, 4097, V])
def test_gpu_gen_beam_topk_matches_the_float64_reference(Vv, nb, M, dev):
    rows, seqs, run = _case_rows(Vv, nb, 1000 + Vv % 97 + nb)
    worst = 0.0
    for ci, use_ids in enumerate((False, True)):
        penalty, ngram = CASES[(nb + ci + M) % len(CASES)]
        ids = None
        if use_ids:
            ids = np.unique(np.random.default_rng(Vv + nb).integers(0, Vv, max(5, min(Vv // 3, 300)))).tolist()
        got_s, got_t = _topk(dev, rows, seqs, run, M, ids, penalty, ngram)
        for b in range(nb):
            worst = max(worst, _check_row(got_s[b], got_t[b], rows[b], seqs[b], run[b], M, ids, penalty, ngram))
    print(f"V = {Vv}, nb = {nb}, M = {M}: largest |fp32 - float64| {worst:.3e} (EPS {EPS:.3e})")


@pytest.mark.gpu
def test_gpu_gen_beam_topk_value_edges(dev):
    Vv, M = 4097, 6                                          # odd V: row 1 of a batch starts unaligned
    rows, seqs, run = _case_rows(Vv, 4, 7)
    rows = rows.float()
    rows[0, :] = NEG                                         # nothing above -inf: (-inf, 0) entries
    rows[1, 100] = float("nan")                              # a NaN never wins and does not poison the lse
    rows[1, Vv - 1] = 60.0                                   # the largest entry in the last element, unaligned row
    seqs[2] = [5, 9, 5]                                      # bigram (5, 9) seen: 9 is banned behind the last 5
    rows[2, 9] = 50.0                                        # ... and it is the maximum
    rows[3, 0] = NEG
    rows = rows.bfloat16()
    got_s, got_t = _topk(dev, rows, seqs, run, M, None, 1.2, 2)
    assert np.all(got_s[0] == NEG) and np.all(got_t[0] == 0)
    assert got_t[1][0] == Vv - 1 and 100 not in got_t[1].tolist() and np.all(np.isfinite(got_s[1]))
    assert 9 not in got_t[2].tolist()
    assert 0 not in got_t[3].tolist()
    for b in range(1, 4):
        _check_row(got_s[b], got_t[b], rows[b], seqs[b], run[b], M, None, 1.2, 2)
    # every logit equal and a killed beam: all V entries tie at -1e9 exactly, the lowest tokens win in order
    flat = torch.zeros(2, Vv).bfloat16()
    s2, t2 = _topk(dev, flat, [[1, 2], [3]], [0.0, R.KILL], 72)
    assert t2[0].tolist() == list(range(72)) and t2[1].tolist() == list(range(72)) and np.all(s2[1] == np.float32(R.KILL))
    # a single allowed id: one finite entry, the rest (-inf, 0)
    s3, t3 = _topk(dev, flat, [[1, 2], [3]], [0.0, -2.0], 4, ids=[77])
    assert t3.tolist() == [[77, 0, 0, 0]] * 2 and np.all(s3[:, 1:] == NEG) and np.all(np.isfinite(s3[:, 0]))


@pytest.mark.gpu
@pytest.mark.parametrize("use_ids", [False, True])
def test_gpu_gen_beam_topk_is_batch_invariant(use_ids, dev):
    rows, seqs, run = _case_rows(V, 16, 31)
    ids = np.unique(np.random.default_rng(5).integers(0, V, 300)).tolist() if use_ids else None
    all_s, all_t = _topk(dev, rows, seqs, run, 72, ids, 1.2, 2)
    for b in (0, 5, 15):                                     # row r of nb = 16 == the nb = 1 call on that row
        s1, t1 = _topk(dev, rows[b:b + 1].clone(), [seqs[b]], [run[b]], 72, ids, 1.2, 2)
        assert np.array_equal(s1[0].view(np.uint32), all_s[b].view(np.uint32)) and np.array_equal(t1[0], all_t[b])
    perm = list(reversed(range(16)))
    p_s, p_t = _topk(dev, rows[perm].clone(), [seqs[b] for b in perm], [run[b] for b in perm], 72, ids, 1.2, 2)
    assert np.array_equal(p_s.view(np.uint32), all_s[perm].view(np.uint32)) and np.array_equal(p_t, all_t[perm])


class _StepRig:
    """P prompts of K beams on the device and their beam_ref.State twins (fp32 mode): call() feeds both the same
    synthetic per-row candidate lists and compares everything kd_gen_beam_step keeps."""

    def __init__(self, dev, K, eos, length_penalty, Ls, max_new, seed):
        self.dev, self.K, self.eos, self.P, self.Ls, self.max_new = dev, K, sorted(eos), len(Ls), list(Ls), max_new
        self.M = max(2, 1 + len(eos)) * K
        self.smax = max(Ls) + max_new + 2
        self.rng = np.random.default_rng(seed)
        nb = self.P * K
        seq = torch.full((nb, self.smax), -7, dtype=torch.int64)
        self.states = []
        for p, L in enumerate(Ls):
            prompt = self.rng.integers(0, 1000, L).tolist()
            seq[p * K:(p + 1) * K, :L] = torch.tensor(prompt)
            self.states.append(R.State(prompt, K))
        self.seq = seq.to(dev)
        self.fin_seq = self.seq.clone()
        self.cur = torch.tensor([L for L in Ls for _ in range(K)], dtype=torch.int32, device=dev)
        self.run = torch.tensor(([0.0] + [R.KILL] * (K - 1)) * self.P, dtype=torch.float32, device=dev)
        self.fin_score = torch.full((nb,), R.KILL, dtype=torch.float32, device=dev)
        self.fin_len = torch.zeros(nb, dtype=torch.int32, device=dev)
        self.open = torch.ones(self.P, dtype=torch.int32, device=dev)
        self.live = torch.tensor([self.P, 0], dtype=torch.int32, device=dev)
        self.parent = torch.full((nb,), -1, dtype=torch.int32, device=dev)
        self.out = torch.full((nb,), -1, dtype=torch.int64, device=dev)
        self.den_host = R.den_table(max_new, length_penalty)
        self.den = torch.tensor(self.den_host, dtype=torch.float64).to(torch.float32).to(dev)
        self.plen = torch.tensor(Ls, dtype=torch.int32, device=dev)

    def lists(self, plant=()):
        """Per row M (score, token) pairs, descending; plant: (row, rank, token) puts a token at a rank."""
        nb, M = self.P * self.K, self.M
        sc = (-self.rng.random((nb, M)) * 20.0).astype(np.float32) + self.run.cpu().numpy()[:, None]   # killed: all -1e9
        sc = -np.sort(-sc.astype(np.float32), axis=1)
        tk = self.rng.integers(2000, 3000, (nb, M)).astype(np.int32)
        for row, rank, token in plant:
            tk[row, rank] = token
        return sc, tk

    def ranked(self, sc, p):
        """Prompt p's (row, m) entries in the global candidate order: larger score, lower beam, lower position."""
        K, M = self.K, self.M
        return [(p * K + j, m) for _, j, m in sorted(((-float(sc[p * K + j, m]), j, m) for j in range(K) for m in range(M)))]

    def call(self, sc, tk):
        ops = import_module(f"{PKG}.ops")
        K, M, P = self.K, self.M, self.P
        before = [t.clone() for t in (self.seq, self.fin_seq, self.cur, self.run, self.fin_score, self.fin_len)]
        ops.gen_beam_step(torch.tensor(sc, device=self.dev), torch.tensor(tk, device=self.dev), K, self.seq, self.cur,
                          self.run, self.out, self.parent, self.fin_seq, self.fin_score, self.fin_len, self.open,
                          self.live, self.den, self.eos, self.plen)
        torch.cuda.synchronize()
        seq, fin_seq, cur, run, fs, fl = (t.cpu() for t in (self.seq, self.fin_seq, self.cur, self.run, self.fin_score,
                                                            self.fin_len))
        open_, live, parent, out = self.open.cpu().tolist(), self.live.cpu().tolist(), self.parent.cpu(), self.out.cpu()
        for p, st in enumerate(self.states):
            rows = slice(p * K, (p + 1) * K)
            if st.done:                                      # a closed prompt: nothing of it changes
                for now, was in zip((seq, fin_seq, cur, run, fs, fl), before):
                    assert torch.equal(now[rows], was[rows].cpu()), p
                assert parent[rows].tolist() == list(range(K)) and open_[p] == 0
                continue
            merged = sorted(((float(sc[p * K + j, m]), j, m, int(tk[p * K + j, m])) for j in range(K) for m in range(M)),
                            key=lambda e: (-e[0], e[1], e[2]))[:M]
            parents, tokens, _ = R.advance(st, [(s, j, t) for s, j, _, t in merged], set(self.eos), st.L + self.max_new,
                                           self.den_host, ft=np.float32)
            L = st.L
            assert parent[rows].tolist() == parents and out[rows].tolist() == tokens, p
            assert cur[rows].tolist() == [st.cur] * K
            for j in range(K):
                assert seq[p * K + j, :st.cur].tolist() == st.run_seq[j], (p, j)
                assert np.float32(st.run_score[j]) == run[p * K + j].numpy(), (p, j)
                score, flag, hyp = st.fin[j]
                assert np.float32(score) == fs[p * K + j].numpy(), (p, j)
                assert int(fl[p * K + j]) == (len(hyp) if flag else 0), (p, j)
                if flag:
                    assert fin_seq[p * K + j, :len(hyp)].tolist() == hyp, (p, j)
                assert fin_seq[p * K + j, :L].tolist() == hyp[:L]
            assert open_[p] == (0 if st.done else 1), p
            assert torch.all(seq[rows, L + self.max_new:] == -7) and torch.all(fin_seq[rows, L + self.max_new:] == -7)
        assert live == [sum(0 if st.done else 1 for st in self.states), 0]
        return parent[:].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("length_penalty", [0.0, 1.0, 2.0])
@pytest.mark.parametrize("n_eos", [1, 8])
@pytest.mark.parametrize("K", [2, 3, 8])
def test_gpu_gen_beam_step_matches_the_fp32_restatement(K, n_eos, length_penalty, dev):
    eos = [2 ** 40 + 5, 7, 11, 13, 17, 19, 23, 29][:n_eos] if n_eos == 8 else [7]
    rig = _StepRig(dev, K, eos, length_penalty, Ls=[5, 9], max_new=6, seed=K * 10 + n_eos)
    M = rig.M
    first = rig.call(*rig.lists())                           # the first choice: beams 1 .. K - 1 killed, so every
    assert first == [0] * (2 * K)                            # new beam descends from beam 0: a duplicated parent
    rig.call(*rig.lists(plant=[(0, 0, 5)]))                  # free choice; token 5 is no EOS although 2^40 + 5 is
    #                                                          one (ids compare as int64)
    sc, tk = rig.lists()
    tk[rig.ranked(sc, 0)[0]] = 7                             # prompt 0: an EOS at candidate rank 0 (< K): finished
    tk[rig.ranked(sc, 1)[K + 1]] = eos[-1]                   # prompt 1: an EOS at rank K + 1 (>= K): killed, not finished
    rig.call(sc, tk)
    assert rig.states[0].fin[0][1] and not any(flag for _, flag, _ in rig.states[1].fin)
    # prompt 0: its K best candidates are EOS: K finished at once, the best running beam is worse: unsat turns false
    sc, tk = rig.lists()
    for e in rig.ranked(sc, 0)[:K]:
        tk[e] = 7
    rig.call(sc, tk)
    assert rig.states[0].done and not rig.states[0].unsat and not rig.states[1].done
    rig.call(*rig.lists())                                   # prompt 0 closed: left unchanged by a further call
    rig.call(*rig.lists())                                   # prompt 1 reaches max_len: all M hit
    assert rig.states[1].done and rig.states[1].cur == 9 + 6
    rig.call(*rig.lists())                                   # both closed


@pytest.mark.gpu
def test_gpu_gen_beam_step_two_prompts_give_what_each_gives_alone(dev):
    K, eos = 3, [7]
    both = _StepRig(dev, K, eos, 1.0, Ls=[5, 9], max_new=6, seed=3)
    alone = [_StepRig(dev, K, eos, 1.0, Ls=[L], max_new=6, seed=4 + p) for p, L in enumerate((5, 9))]
    for p, rig in enumerate(alone):                          # the same prompts as in the pair
        rig.seq[:, :rig.Ls[0]] = both.seq[p * K:(p + 1) * K, :rig.Ls[0]]
        rig.fin_seq[:, :rig.Ls[0]] = both.fin_seq[p * K:(p + 1) * K, :rig.Ls[0]]
        rig.states[0] = R.State(both.states[p].run_seq[0], K)
    for step in range(6):
        sc, tk = both.lists(plant=[(1, 0, 7)] if step == 2 else ())
        both.call(sc, tk)
        for p, rig in enumerate(alone):
            rows = slice(p * K, (p + 1) * K)
            rig.call(sc[rows], tk[rows])
            w = rig.Ls[0] + 6
            assert torch.equal(rig.seq[:, :w], both.seq[rows, :w]) and torch.equal(rig.fin_seq[:, :w], both.fin_seq[rows, :w])
            for a, b in ((rig.run, both.run), (rig.fin_score, both.fin_score), (rig.fin_len, both.fin_len),
                         (rig.cur, both.cur), (rig.parent, both.parent), (rig.out, both.out)):
                assert torch.equal(a, b[rows])


@pytest.mark.gpu
@pytest.mark.parametrize("hd", [64, 128])
def test_gpu_kv_beam_reorder_matches_index_select(hd, dev):
    ops = import_module(f"{PKG}.ops")
    layers, HKV, smax, K = 2, 2, 24, 3
    Ls = [4, 9]
    g = torch.Generator().manual_seed(hd)
    for tails, parents in itertools.product(((0, 1), (1, 5), (5, 0)), (([0, 0, 2], [2, 0, 1]), ([2, 0, 1], [0, 1, 2]))):
        kc = torch.randn(layers, 2 * K, HKV, smax, hd, generator=g).bfloat16().to(dev)
        vc = torch.randn(layers, 2 * K, HKV, smax, hd, generator=g).bfloat16().to(dev)
        want = [kc.clone(), vc.clone()]
        for w in want:
            for p in range(2):
                lo, hi = Ls[p], Ls[p] + tails[p]
                src = torch.tensor([p * K + j for j in parents[p]], device=dev)
                w[:, p * K:(p + 1) * K, :, lo:hi] = w[:, :, :, lo:hi].index_select(1, src)
        cur = torch.tensor([Ls[p] + tails[p] + 1 for p in range(2) for _ in range(K)], dtype=torch.int32, device=dev)
        parent = torch.tensor(parents[0] + parents[1], dtype=torch.int32, device=dev)
        ops.kv_beam_reorder(kc, vc, K, parent, cur, torch.tensor(Ls, dtype=torch.int32, device=dev), 8)
        torch.cuda.synchronize()
        # everything outside the ranges is random data no other element equals: untouched means bit-equal
        assert torch.equal(kc, want[0]) and torch.equal(vc, want[1]), (tails, parents)


# ------------------------------------------------------------------ GPU, end to end ----

KW = dict(repetition_penalty=1.2, no_repeat_ngram_size=2, eos_token_id=())
BKW = dict(num_beams=3, length_penalty=1.0)
ALLOWED = sorted(set(range(0, 600, 2)) | {151646, 7, V - 1})
NEW = 6


def _replay(prompt_ids, logs, K, eos, max_new, allowed=None, length_penalty=1.0):
    """beam_ref on the rows the call returned, step by step."""
    def fn(run_seq, step):
        return logs[step].float().cpu().numpy()
    return R.search(fn, prompt_ids, K, eos=eos, max_new=max_new, penalty=1.2, ngram=2, length_penalty=length_penalty,
                    allowed=allowed)


def _flat(x):
    return [r for g in x for r in g]


@pytest.fixture(scope="module")
def beams3(run3, dev):
    gen, model, prompts = run3["gen"], run3["model"], run3["prompts"]
    stats = {}
    outs, logs = gen.generate_batch(model, prompts, max_new_tokens=NEW, return_logits=True, stats=stats, **KW, **BKW)
    return dict(outs=outs, logs=logs, stats=stats)


N10, NEW10 = 10, 4   # ten prompt seeds (two chunks of five at K = 3), four new tokens: the pool the margin picks from


@pytest.fixture(scope="module")
def prompts10(run3, dev):
    """The tiny student's logits are nearly flat (std 0.2 over 151,936 ids), so most prompts meet a decision
    closer than 2 * EPS somewhere: ten seeds, of which the reference's margin admits a few."""
    data = import_module(f"{PKG}.data")
    prompts = []
    for i in range(N10):
        b = data.synthetic_batch(1, dev, L=1490 + 7 * i, seed=9 + 2 * i, pixel_dtype=torch.bfloat16, cpu_rng=True)
        prompts.append((b["depth_input_ids"], b["depth_pixel_values"], b["image_sizes"]))
    return prompts


def _replay_all(prompts, outs, logs, stats, allowed=None):
    """Every prompt replayed by the reference on its returned rows; those whose margin exceeds 2 * EPS (chosen from
    the reference alone) must give equal tokens, equal scores within EPS and the trace the call reports -> how many."""
    per = 16 // 3
    taken = 0
    for r, (ids, px, sizes) in enumerate(prompts):
        c, s = divmod(r, per)
        assert all(lg.shape == (3, V) and lg.dtype == torch.bfloat16 for lg in logs[r])
        ref = _replay(ids[0].cpu().tolist(), logs[r], 3, (), NEW10, allowed=allowed)
        print(f"prompt {r}: reference margin {ref['margin']:.3e} (2 EPS = {2 * EPS:.3e}), steps {ref['steps']}")
        if ref["margin"] <= 2 * EPS:
            continue
        taken += 1
        assert outs[r][0].cpu().tolist() == ref["seq"] and stats["finished_at"][c][s] == len(ref["seq"])
        assert abs(stats["sequences_scores"][c][s] - ref["score"]) <= EPS
        for t, (parents, tokens, scores) in enumerate(ref["trace"]):
            assert stats["beam_parents"][c][t][s] == parents and stats["beam_tokens"][c][t][s] == tokens
            assert np.abs(np.array(stats["beam_scores"][c][t][s]) - np.array(scores)).max() <= EPS
    return taken


@pytest.fixture(scope="module")
def beams10(run3, prompts10, dev):
    stats = {}
    outs, logs = run3["gen"].generate_batch(run3["model"], prompts10, max_new_tokens=NEW10, return_logits=True,
                                            stats=stats, **KW, **BKW)
    return dict(outs=outs, logs=logs, stats=stats)


@pytest.mark.gpu
def test_gpu_beam_generate_batch_replays_on_the_reference(prompts10, beams10, dev):
    """Of the ten seeds the reference's margin admits two (seeds 1 and 3; the kernels are deterministic, so the
    margins computed on their rows are too): fewer means the rows, and so something in the step, changed."""
    outs, logs, stats = beams10["outs"], beams10["logs"], beams10["stats"]
    assert stats["steps_max"] == [NEW10 - 1] * 2 and [len(c) for c in stats["sequences_scores"]] == [5, 5]
    assert _replay_all(prompts10, outs, logs, stats) >= 2, "fewer prompts with the margin than the pool was chosen for"


def _beam_sequences(prompt, parents, tokens):
    """Per choice t the K sequences that fed its rows: the prompt, then each beam's parent's ids and its token."""
    seqs = [[list(prompt)] * len(parents[0])]
    for par, tok in zip(parents, tokens):
        seqs.append([seqs[-1][p] + [t] for p, t in zip(par, tok)])
    return seqs


@pytest.mark.gpu
@pytest.mark.parametrize("r", range(3))
def test_gpu_beam_every_returned_row_matches_the_oracle(r, run3, beams3, dev):
    """No margin is needed here: whatever the search chose, row j of choice t must be the oracle model's logits
    behind the ids of the beam that fed it, under test_generate_batch's bounds.  The beams' ids come from the
    trace (parents, tokens), so a K/V tail reordered to the wrong row or position shows as a row that belongs to
    another sequence.  One teacher-forced oracle forward per sequence that is no prefix of another serves all its
    prefixes (6 new tokens: tails of up to 4 positions are reordered)."""
    from model_fixtures import tiny_weights
    from oracle.model import OracleLlava
    ids, px, sizes = run3["prompts"][r]
    stats, logs = beams3["stats"], beams3["logs"][r]
    parents = [stats["beam_parents"][0][t][r] for t in range(NEW)]
    tokens = [stats["beam_tokens"][0][t][r] for t in range(NEW)]
    seqs = _beam_sequences(ids[0].cpu().tolist(), parents, tokens)
    assert len(logs) == NEW and beams3["outs"][r][0].cpu().tolist() in seqs[NEW]   # all hit at max_len: a final beam
    assert torch.equal(logs[0][1], logs[0][0]) and torch.equal(logs[0][2], logs[0][0])   # K copies of the prefill's row
    need = {}                                                  # sequence -> the (t, j) rows it fed
    for t in range(NEW):
        for j in range(3 if t else 1):
            need.setdefault(tuple(seqs[t][j]), []).append((t, j))
    orc = OracleLlava(tiny_weights(False, 5), run3["cfg"])
    done, forwards = set(), 0
    for s in sorted(need, key=len, reverse=True):
        if s in done:
            continue
        full, _ = orc(torch.tensor([list(s)]), px.float().cpu(), sizes)
        forwards += 1
        for q in need:
            if q not in done and q == s[:len(q)]:
                done.add(q)
                want = full[0, len(q) - 1]
                for t, j in need[q]:
                    got = logs[t][j].float().cpu()
                    assert torch.nn.functional.cosine_similarity(got, want, dim=0) > 0.999, (r, t, j)
                    assert (got - want).abs().max() < 0.05 * want.abs().max() + 0.05, (r, t, j)
    moved = [t for t in range(1, NEW - 1) if parents[t] != [0, 1, 2]]   # choices whose reorder moved a non-empty tail
    print(f"prompt {r}: {sum(len(v) for v in need.values())} rows, {forwards} oracle forwards, parents {parents}")
    assert len(done) == len(need)
    assert moved, "no choice of this prompt permuted its beams: the K/V reorder was not exercised"


def _same(a, b):
    (oa, la), (ob, lb) = a, b
    assert len(oa) == len(ob)
    for r in range(len(oa)):
        assert torch.equal(oa[r], ob[r]), r
        assert len(la[r]) == len(lb[r]) and all(torch.equal(x, y) for x, y in zip(la[r], lb[r])), r


@pytest.mark.gpu
def test_gpu_beam_routes_give_the_same_bits(run3, beams3, dev):
    gen, model, prompts = run3["gen"], run3["model"], run3["prompts"]
    base = (beams3["outs"], beams3["logs"])
    scores = beams3["stats"]["sequences_scores"][0]

    def call(ps=prompts, **kw):
        stats = {}
        res = gen.generate_batch(model, ps, max_new_tokens=NEW, return_logits=True, stats=stats, **KW, **BKW, **kw)
        return res, stats

    for kw in (dict(graph=False), dict(stop_check_every=0), dict(stop_check_every=3), dict(graph=False, stop_check_every=3)):
        res, stats = call(**kw)
        n = stats["steps_run"][0] + 1                        # rows past the last step run are not there to compare
        _same((res[0], [l[:n] for l in res[1]]), (base[0], [l[:n] for l in base[1]]))
        assert stats["sequences_scores"][0] == scores
    # generate() takes the batched route; a prompt alone; a prompt inside a chunk of four (K = 3: 5 per chunk)
    for r in range(3):
        stats = {}
        one, one_lg = gen.generate(model, *prompts[r], max_new_tokens=NEW, return_logits=True, stats=stats, **KW, **BKW)
        res, s2 = call(ps=[prompts[r]])
        _same(([one], [one_lg]), res)
        assert torch.equal(one, base[0][r]) and stats["sequences_scores"] == s2["sequences_scores"] == [[scores[r]]]
    four, s4 = call(ps=[prompts[2], prompts[0], prompts[1], prompts[0]])
    for slot, r in enumerate((2, 0, 1, 0)):
        assert torch.equal(four[0][slot], base[0][r]) and s4["sequences_scores"][0][slot] == scores[r]
    six = gen.generate_batch(model, [prompts[i % 3] for i in range(6)], max_new_tokens=NEW, **KW, **BKW)   # two chunks
    assert all(torch.equal(six[i], base[0][i % 3]) for i in range(6))


@pytest.mark.gpu
def test_gpu_beam_num_beams_1_is_the_plain_call(run3, run_g, dev):
    gen, model, prompts = run3["gen"], run3["model"], run3["prompts"]
    outs, logs = gen.generate_batch(model, prompts, max_new_tokens=8, return_logits=True, num_beams=1,
                                    length_penalty=float("nan"), early_stopping=True, **KW)
    _same((outs, logs), (run3["outs"], run3["logs"]))
    one = gen.generate(model, *prompts[0], max_new_tokens=8, num_beams=1, **KW)
    assert torch.equal(one, run3["outs"][0])
    gg = gen.generate_grouped(run_g["model"], run_g["groups"], max_new_tokens=8, num_beams=1, **KW)
    assert all(torch.equal(a, b) for a, b in zip(_flat(gg), _flat(run_g["outs"])))


GROUP_TAKEN = 4   # of the ten questions below the reference's margin admits four (3, 6, 7, 9; deterministic)


@pytest.mark.gpu
def test_gpu_beam_generate_grouped_alone_against_in_a_group(run_g, dev):
    """Ten questions behind one image (two chunks of five at K = 3; suffixes of 5 .. 32 ids): the pool the margin
    picks from.  Three of them alone against in the group, bit for bit; all of them replayed by the reference."""
    from test_generate_grouped import P0
    data = import_module(f"{PKG}.data")
    gen, model = run_g["gen"], run_g["model"]
    px, sizes, q0 = run_g["groups"][0][0], run_g["groups"][0][1], run_g["groups"][0][2][0]
    qs = []
    for qi in range(10):
        g = torch.Generator().manual_seed(1000 + qi)
        suf = torch.randint(0, data.TEXT_VOCAB, (1, 5 + 3 * qi), generator=g, dtype=torch.int64).to(dev)
        qs.append(torch.cat([q0[:, :P0], suf], 1))
    stats = {}
    outs, logs = gen.generate_grouped(model, [(px, sizes, qs)], max_new_tokens=NEW10, return_logits=True, stats=stats,
                                      **KW, **BKW)
    assert len(outs) == 1 and len(outs[0]) == 10 and logs[0][0][0].shape == (3, V)
    for qi in (0, 4, 7):                                      # slots 0 and 4 of chunk 0, slot 2 of chunk 1
        s1 = {}
        o1, l1 = gen.generate_grouped(model, [(px, sizes, [qs[qi]])], max_new_tokens=NEW10, return_logits=True,
                                      stats=s1, graph=False, **KW, **BKW)
        _same((_flat(o1), _flat(l1)), ([outs[0][qi]], [logs[0][qi]]))
        assert s1["sequences_scores"][0][0] == stats["sequences_scores"][qi // 5][qi % 5]
    taken = _replay_all([(q, px, sizes) for q in qs], outs[0], logs[0], stats)
    assert taken >= GROUP_TAKEN, "fewer questions with the margin than the pool was chosen for"


@pytest.mark.gpu
def test_gpu_beam_allowed_token_ids_and_an_early_end_on_eos(run3, prompts10, beams10, dev):
    gen, model = run3["gen"], run3["model"]
    stats = {}
    outs, logs = gen.generate_batch(model, prompts10, max_new_tokens=NEW10, return_logits=True, stats=stats,
                                    allowed_token_ids=ALLOWED, **KW, **BKW)
    for r, (ids, _, _) in enumerate(prompts10):                # the rows returned are the full head's
        assert all(int(t) in ALLOWED for t in outs[r][0, ids.shape[1]:]) and logs[r][0].shape == (3, V)
    assert _replay_all(prompts10, outs, logs, stats, allowed=ALLOWED) >= 2   # seeds 7 and 9
    # EOS ids: the tokens a prompt's three beams took at the second choice of the EOS-free search.  Its K best
    # candidates there are then hits, K hypotheses finish at once and the best running beam is worse than all of
    # them: every prompt's search ends early, behind its second choice.  The reference replays those it admits.
    taken = 0
    for r, prompt in enumerate(prompts10):
        L = int(prompt[0].shape[1])
        eos = sorted(set(beams10["stats"]["beam_tokens"][r // 5][1][r % 5]))
        stats = {}
        cut, cut_lg = gen.generate_batch(model, [prompt], max_new_tokens=32, return_logits=True, stats=stats,
                                         repetition_penalty=1.2, no_repeat_ngram_size=2, eos_token_id=eos, **BKW)
        got = cut[0][0].cpu().tolist()
        assert stats["steps_run"][0] < stats["steps_max"][0] == 31 and stats["finished_at"][0] == [len(got)], r
        assert got[-1] in eos and not set(eos) & set(got[L:-1]) and len(got) <= L + 2, r
        ref = _replay(prompt[0][0].cpu().tolist(), cut_lg[0], 3, eos, 32)
        print(f"EOS {eos}, prompt {r}: steps run {stats['steps_run']}, length {len(got) - L}, margin {ref['margin']:.3e}")
        if ref["margin"] > 2 * EPS:
            taken += 1
            assert got == ref["seq"] and abs(stats["sequences_scores"][0][0] - ref["score"]) <= EPS, r
    assert taken >= 1, "no prompt with the margin: the EOS replay checked nothing"
