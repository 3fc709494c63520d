"""do_sample: temperature / top-k / top-p sampling in the decode step (kd_gen_sample, ops.gen_sample,
do_sample= of generate() / generate_batch() / generate_grouped()).
CPU: Philox known answers, the reference (sampling_ref.Ref) against transformers' warpers, argument
validation of the C ABI and of the entry points.  GPU: kd_gen_sample's u, writes, distribution (every
draw checked by the acceptance rule against the fp64 reference), value edges that each see one wrong
entry and batch invariance; the three entry points on the tiny student, bit for bit across their
routes, teacher-forced against the CPU oracle model, the greedy limit, EOS and the seed."""
import ctypes
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sampling_ref as R
from oracle import generation as G
from test_generate import CASES, _seq_scores
from test_generate_batch import LENS, run3   # noqa: F401  (fixture)
from test_generate_grouped import run_g      # noqa: F401  (fixture)

PKG = "knowledge_distillation_for_sensory_substitution_in_multimodal_models_amd"
V = 151936
NEG = -np.inf
EPS = R.EPS
assert EPS == 2.0 ** -15


def _bf16(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float32)).bfloat16().float().numpy()


def _randn_row(seed, scale=4.0, bf16=True):
    """bf16(randn(V, seed) * scale) as fp32 (bf16=False: not rounded, so without exact ties)."""
    g = torch.Generator().manual_seed(seed)
    row = torch.randn(V, generator=g) * scale
    return (row.bfloat16().float() if bf16 else row).numpy()


# ----------------------------------------------------------------------------- CPU ----

def test_philox_known_answers_and_worked_draws():
    F = 0xFFFFFFFF
    assert R.philox((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert R.philox((F, F, F, F), (F, F)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert R.philox((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)
    assert R.word0(0x0123456789ABCDEF, 5, 1536) == 0x7F749BBA
    assert R.u_of(0x0123456789ABCDEF, 5, 1536) == 0.4978730082511902
    assert R.word0(2 ** 64 - 1, 2 ** 63 - 1, 1567) == 0x06F82BD9
    assert R.u_of(2 ** 64 - 1, 2 ** 63 - 1, 1567) == 0.027224242687225342
    assert 0.0 <= R.u_of(3, 4, 5) < 1.0 and float(np.float32(R.u_of(3, 4, 5))) == R.u_of(3, 4, 5)


def _hf_warped(processed, temperature, top_k, top_p):
    from transformers.generation.logits_process import (TemperatureLogitsWarper, TopKLogitsWarper,
                                                        TopPLogitsWarper)
    s = torch.from_numpy(np.asarray(processed, dtype=np.float32))[None].clone()
    dummy = torch.zeros((1, 1), dtype=torch.int64)
    s = TemperatureLogitsWarper(float(temperature))(dummy, s)
    if top_k >= 1:
        s = TopKLogitsWarper(int(top_k))(dummy, s)
    if top_p < 1.0:
        s = TopPLogitsWarper(float(top_p))(dummy, s)
    return s[0]


# (temperature, top_k, top_p): the settings of the distribution test
SETTINGS = [(0.7, 50, 1.0), (0.7, 64, 0.9), (1.0, 0, 0.9), (1.5, 1000, 1.0), (1.0, 0, 1.0)]


@pytest.mark.parametrize("case", range(len(SETTINGS)))
def test_reference_matches_transformers_warpers(case):
    """Behind RepetitionPenalty / NoRepeatNGram (oracle.generation.process_scores, itself checked against
    transformers in test_generate.py) and the additive allowed mask: the same finite set and the same
    probabilities as Temperature -> TopK -> TopP, on rows with the 1e-4 top-p margin and no exact tie at
    the top-p cut (fp32 rows: bf16 logits tie at every cut in the bulk; the first row seed that qualifies is
    taken, from the reference alone)."""
    temperature, top_k, top_p = SETTINGS[case]
    penalty, ngram = CASES[case % len(CASES)]
    seq, _ = _seq_scores(40 + case)
    for ids in (None, np.unique(np.random.default_rng(case).integers(0, V, 300))):
        for row_seed in range(1 + case, 200, 10):
            s = G.process_scores(_randn_row(row_seed, bf16=False), seq, penalty, ngram)
            if ids is not None:
                m = np.full_like(s, NEG)
                m[ids] = s[ids]
                s = m
            ref = R.Ref(s, temperature, top_k, top_p)
            if ref.p_margin > 1e-4 and ref.cut_ties == 1:
                break
        assert ref.p_margin > 1e-4 and ref.cut_ties == 1, (ref.p_margin, ref.cut_ties)
        hf = _hf_warped(s, temperature, top_k, top_p)
        np.testing.assert_array_equal(np.isfinite(hf.numpy()), ref.keep & np.isfinite(ref.t))
        p = torch.softmax(hf.double(), -1).numpy()
        assert np.abs(p - ref.probs()).max() < 1e-6


def test_reference_ties_at_the_top_k_cut_are_all_kept_as_transformers_keeps_them():
    s = np.full(40, -5.0, dtype=np.float32)
    s[[3, 9, 17, 30]] = [4.0, 2.0, 2.0, 2.0]     # top_k = 2: the second largest value occurs three times
    ref = R.Ref(s, 0.7, 2, 1.0)
    assert sorted(np.nonzero(ref.keep)[0].tolist()) == [3, 9, 17, 30]
    hf = _hf_warped(s, 0.7, 2, 1.0).numpy()
    np.testing.assert_array_equal(np.isfinite(hf), ref.keep)
    assert np.abs(torch.softmax(torch.from_numpy(hf).double(), -1).numpy() - ref.probs()).max() < 1e-6


def test_reference_ties_at_the_top_p_cut_are_kept_or_dropped_together():
    """p = [0.4, 0.2, 0.2, 0.2]: at top_p = 0.7 transformers keeps the first and, by its sort order, two
    of the three tied entries; the reference keeps all three (mass above them: 0.4 < 0.7) -- and at
    top_p = 0.3 none of them (0.4 >= 0.3)."""
    s = np.log(np.array([0.2, 0.4, 0.2, 0.2])).astype(np.float32)
    ref = R.Ref(s, 1.0, 0, 0.7)
    assert ref.keep.tolist() == [True, True, True, True]
    hf = np.isfinite(_hf_warped(s, 1.0, 0, 0.7).numpy())
    assert hf[1] and hf.sum() == 3                 # transformers splits the tie
    assert R.Ref(s, 1.0, 0, 0.3).keep.tolist() == [False, True, False, False]


def test_abi_gen_sample_rejects_bad_arguments():
    """Validation runs before any device work (host memory stands in for the pointers: it is never
    dereferenced): KD_ERR_ARG = 7, KD_ERR_SHAPE = 1."""
    NV = import_module(f"{PKG}._native")
    lib = NV.lib()
    MAXA = NV.KD_GEN_ALLOWED_MAX
    buf = ctypes.create_string_buffer(256 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    size = lib.kd_gen_sample_workspace_size
    assert 0 < size(1, 13) <= size(1, 4097) < size(1, V) < size(2, V) and size(16, V) == 16 * size(1, V)
    assert size(0, V) == 0 and size(1, 0) == 0
    big = size(1, 8)

    def call(scores=p, ld=8, N=8, ids=None, seq=p, smax=16, nb=1, cur=p, penalty=1.2, ngram=2, T=0.7, top_k=50,
             top_p=0.9, seed=2 ** 64 - 1, streams=p, ws=p, wsb=big, out=p, u_out=None):
        return lib.kd_gen_sample(scores, ld, N, ids, seq, smax, nb, cur, penalty, ngram, T, top_k, top_p, seed, streams,
                                 ws, wsb, out, u_out, None)

    for name in ("scores", "seq", "cur", "streams", "ws", "out"):
        assert call(**{name: None}) == 7, name
    assert b"null" in lib.kd_last_error()
    assert call(penalty=0.0) == 7 and call(penalty=-1.0) == 7 and call(ngram=-1) == 7
    for bad_t in (0.0, -0.5, float("inf"), float("nan")):
        assert call(T=bad_t) == 7, bad_t
    assert call(top_k=-1) == 7
    for bad_p in (0.0, -0.1, 1.0001, float("nan")):
        assert call(top_p=bad_p) == 7, bad_p
    assert call(nb=0) == 1 and call(nb=17, wsb=17 * big) == 1
    assert call(N=0) == 1 and call(N=2 ** 18 + 1, ld=2 ** 18 + 1, wsb=2 ** 40) == 1
    assert call(ids=p, N=MAXA + 1, ld=MAXA + 1, wsb=2 ** 40) == 1      # with ids: N <= KD_GEN_ALLOWED_MAX
    assert call(smax=0) == 1 and call(ld=7) == 1
    assert call(wsb=big - 1) == 1 and call(nb=2, wsb=big) == 1
    assert b"workspace" in lib.kd_last_error()


def _stub_calls():
    gen = import_module(f"{PKG}.generation")
    IMG = import_module(f"{PKG}.modeling").IMAGE_TOKEN_ID
    stub = SimpleNamespace(cfg=SimpleNamespace(text=SimpleNamespace(vocab=V, hidden=896), image_token_id=IMG))
    ids = torch.tensor([[5, 6, IMG, IMG, 7, 8]], dtype=torch.int64)
    px, sizes = torch.zeros(1, 2, 3, 384, 384), torch.tensor([[336, 336]])
    return stub, ((lambda **kw: gen.generate(stub, ids, px, sizes, **kw)),
                  (lambda **kw: gen.generate_batch(stub, [(ids, px, sizes)] * 2, **kw)),
                  (lambda **kw: gen.generate_grouped(stub, [(px, sizes, [ids]), (px, sizes, [ids])], **kw)))


BAD = [("temperature", dict(temperature=0.0)), ("temperature", dict(temperature=-1.0)),
       ("temperature", dict(temperature=float("nan"))), ("temperature", dict(temperature=float("inf"))),
       ("top_k", dict(top_k=-1)), ("top_k", dict(top_k=1.5)),
       ("top_p", dict(top_p=0.0)), ("top_p", dict(top_p=1.5)), ("top_p", dict(top_p=float("nan"))),
       ("seed", dict(seed=-1)), ("seed", dict(seed=2 ** 64)), ("seed", dict(seed=0.5)),
       ("sample_streams", dict(sample_streams=[0, 1, 2])), ("sample_streams", dict(sample_streams=[-1, 0])),
       ("sample_streams", dict(sample_streams=[0, 2 ** 63])), ("sample_streams", dict(sample_streams=[0.5, 1]))]


def test_entry_points_refuse_bad_sampling_arguments_before_any_device_work():
    """A model stub with nothing but the sizes: the checks come first."""
    _, calls = _stub_calls()
    for i, call in enumerate(calls):
        for word, kw in BAD:
            if i == 0 and word == "sample_streams":
                kw = dict(sample_streams=[v for v in kw["sample_streams"] if v != 0] or [0, 1])
            with pytest.raises(ValueError, match=word):
                call(do_sample=True, **kw)
    with pytest.raises(ValueError, match="sample_streams"):
        calls[0](do_sample=True, sample_streams=2 ** 63)


def test_greedy_call_ignores_the_sampling_arguments(monkeypatch):
    """do_sample=False: no check of the sampling arguments and no sampler; the stub then fails where the
    greedy call fails on it, at its first use of the model."""
    ops = import_module(f"{PKG}.ops")

    def boom(*a, **kw):
        raise AssertionError("gen_sample on the greedy path")
    monkeypatch.setattr(ops, "gen_sample", boom)
    _, calls = _stub_calls()
    for call in calls:
        with pytest.raises(AttributeError):
            call()
        for _, kw in BAD:
            with pytest.raises(AttributeError):
                call(do_sample=False, **kw)
        stats = {}
        with pytest.raises(AttributeError):
            call(do_sample=False, temperature=0.7, top_k=50, top_p=0.9, seed=3, stats=stats)
        assert "seed" not in stats


# ----------------------------------------------------------------- GPU, kernel level ----

def _sample(dev, seqs, scores, *, ids=None, lens=None, smax=None, streams, seed, penalty=1.0, ngram=0,
            temperature=1.0, top_k=0, top_p=1.0, fill=-3):
    """ops.gen_sample over rows (seqs[b], scores[b]): -> (out, u, seq after, cur after, seq before) on the host."""
    ops = import_module(f"{PKG}.ops")
    nb = len(seqs)
    lens = [len(s) for s in seqs] if lens is None else lens
    smax = max(lens) + 3 if smax is None else smax
    seq = torch.full((nb, smax), fill, dtype=torch.int64)
    for b, s in enumerate(seqs):
        seq[b, :len(s)] = torch.tensor(s, dtype=torch.int64)
    sc = scores if isinstance(scores, torch.Tensor) else torch.as_tensor(np.asarray(scores, dtype=np.float32)).bfloat16()
    seq_d = seq.to(dev)
    cur = torch.tensor(lens, dtype=torch.int32, device=dev)
    out = torch.full((nb,), -7, dtype=torch.int64, device=dev)
    u = torch.full((nb,), -1.0, dtype=torch.float32, device=dev)
    ops.gen_sample(sc.to(dev), seq_d, cur, ids=None if ids is None else torch.tensor(ids, dtype=torch.int32, device=dev),
                   repetition_penalty=penalty, no_repeat_ngram_size=ngram, temperature=temperature, top_k=top_k,
                   top_p=top_p, seed=seed, streams=torch.tensor(streams, dtype=torch.int64, device=dev), out=out, u_out=u)
    return out.cpu().tolist(), u.cpu().tolist(), seq_d.cpu(), cur.cpu().tolist(), seq


def _find_stream(seed, pos, pred, start=0):
    """The first stream id >= start whose u(seed, stream, pos) satisfies pred (pred works on arrays)."""
    for lo in range(start, start + (1 << 26), 1 << 18):
        hit = np.nonzero(pred(R.u_many(seed, np.arange(lo, lo + (1 << 18)), pos)))[0]
        if hit.size:
            assert pred(R.u_of(seed, lo + int(hit[0]), pos))
            return lo + int(hit[0])
    raise AssertionError("no stream found")


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [1, 3, 16])
def test_gpu_gen_sample_u_is_the_host_philox_and_the_writes_are_the_selects(nb, dev):
    seed = 0xFEDCBA9876543210
    streams = ([0, 2 ** 32, 2 ** 63 - 1] + [2 ** 32 + 7 * b for b in range(13)])[:nb]
    g = np.random.default_rng(nb)
    lens = [int(n) for n in g.integers(1, 200, nb)]
    seqs = [list(g.integers(0, 70, n)) for n in lens]
    scores = _bf16(g.standard_normal((nb, 77)) * 3)
    out, u, seq_after, cur, seq0 = _sample(dev, seqs, scores, streams=streams, seed=seed, penalty=1.2, ngram=2,
                                           temperature=0.7, top_k=20, top_p=0.9, smax=203)
    for b in range(nb):
        want_u = R.u_of(seed, streams[b], lens[b])
        assert u[b] == want_u, (b, u[b], want_u)
        ref = R.Ref(G.process_scores(scores[b], seqs[b], 1.2, 2), 0.7, 20, 0.9)
        assert ref.deviation(out[b], want_u) <= EPS, (b, out[b], ref.token(want_u))
        assert cur[b] == lens[b] + 1 and int(seq_after[b, lens[b]]) == out[b]
        seq0[b, lens[b]] = out[b]
    assert torch.equal(seq_after, seq0)            # nothing else in seq is touched


@pytest.mark.gpu
def test_gpu_gen_sample_full_row_writes_out_only(dev):
    seqs = [[4, 9, 8, 7], [5, 9]]
    scores = [[6.0, 5.5, -9.0] + [-20.0] * 7, [1.0, 6.0, 5.5] + [-20.0] * 7]
    out, u, seq_after, cur, seq0 = _sample(dev, seqs, scores, streams=[3, 4], seed=11, smax=4, top_k=1, fill=0)
    assert out == [0, 1] and cur == [5, 3]
    assert torch.equal(seq_after[0], seq0[0]) and seq_after[1].tolist() == [5, 9, 1, 0]
    assert u == [R.u_of(11, 3, 4), R.u_of(11, 4, 2)]


# the five settings, then (0.7, 50, 0.9) among about 300 and among KD_GEN_ALLOWED_MAX allowed ids
DIST = [(s, None, share) for s, share in zip(SETTINGS, (0.95, 0.95, 0.90, 0.90, 0.75))] + \
       [((0.7, 50, 0.9), 300, 0.95), ((0.7, 50, 0.9), 16384, 0.95)]
MAX_DEV = {}


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(DIST)))
def test_gpu_gen_sample_distribution(case, dev):
    """1,024 draws (64 launches x 16 streams) of one row, each held to the acceptance rule; the decisive
    share (draws with exactly one acceptable token) is asserted from the reference alone first."""
    (temperature, top_k, top_p), A, share = DIST[case]
    penalty, ngram = CASES[case % len(CASES)]
    seq, _ = _seq_scores(40 + case, n=200 + 37 * (case % 4))
    scores = _randn_row(1 + case)
    s = G.process_scores(scores, seq, penalty, ngram)
    ids = None
    if A is not None:
        g = np.random.default_rng(case)
        ids = np.unique(np.concatenate([g.integers(0, V, A), np.arange(0, 60, 2), [151646, 7]]))
        if A == 16384:
            ids = np.unique(np.concatenate([ids, np.arange(1000, 1000 + 2 * A, 2)]))[:A]
            assert ids.size == A
    row = s if ids is None else s[ids]
    ref = R.Ref(row, temperature, top_k, top_p)
    if top_p < 1.0:
        assert ref.p_margin > 1e-4, ref.p_margin
    seed, pos = 1234567 + case, len(seq)
    us = [R.u_of(seed, st, pos) for st in range(1024)]
    decisive = sum(ref.decisive(u) for u in us) / 1024
    print(f"case {case}: kept {int(ref.keep.sum())}, decisive share {decisive:.3f}")
    assert decisive >= share, decisive
    banned = set(np.nonzero(np.isneginf(row))[0].tolist())
    sc = torch.from_numpy(scores if ids is None else scores[ids]).bfloat16()[None].expand(16, -1).contiguous()
    worst = 0.0
    for launch in range(64):
        streams = list(range(16 * launch, 16 * launch + 16))
        out, u, _, _, _ = _sample(dev, [seq] * 16, sc, ids=None if ids is None else ids.tolist(), streams=streams,
                                  seed=seed, penalty=penalty, ngram=ngram, temperature=temperature, top_k=top_k, top_p=top_p)
        for b in range(16):
            assert u[b] == us[streams[b]]
            j = out[b] if ids is None else int(np.searchsorted(ids, out[b]))
            assert ids is None or (j < ids.size and ids[j] == out[b]), "an id outside the allowed set"
            assert ref.keep[j] and j not in banned, (launch, b, out[b])
            d = ref.deviation(j, u[b])
            worst = max(worst, d)
            assert d <= EPS, (launch, b, out[b], ref.token(u[b]), d)
    MAX_DEV[case] = worst
    print(f"case {case}: largest acceptance deviation {worst:.3e} (eps {EPS:.3e})")
    assert worst <= 2.0 ** -17, "inside eps, but larger than the error budget explains: find out why"


@pytest.mark.gpu
def test_gpu_gen_sample_value_edges(dev):
    """Each case is decided by one entry."""
    MAXA = import_module(f"{PKG}._native").KD_GEN_ALLOWED_MAX
    seed = 99

    def draw(row, stream, seq=(1, 2, 3), ids=None, **kw):
        out, u, _, cur, _ = _sample(dev, [list(seq)], [row], ids=ids, streams=[stream], seed=seed, **kw)
        assert u[0] == R.u_of(seed, stream, len(seq)) and cur[0] == len(seq) + 1
        return out[0], u[0]

    def streams_with(pred, n, pos=3):
        got, s = [], 0
        while len(got) < n:
            s = _find_stream(seed, pos, pred, s)
            got.append(s)
            s += 1
        return got

    low, mid, high = (streams_with(p, 2)
                      for p in ((lambda u: u < 0.1), (lambda u: (0.45 < u) & (u < 0.55)), (lambda u: u > 0.9)))
    g = np.random.default_rng(3)
    row = _bf16(g.standard_normal(4097) * 2)
    row[1234] = 9.0
    # top_k = 1: the argmax whatever u is; with a two-way tie either tied id and nothing else
    for st in low + mid + high:
        assert draw(row, st, top_k=1)[0] == 1234
    tie = row.copy()
    tie[77] = 9.0
    seen = {draw(tie, st, top_k=1)[0] for st in low + mid + high}
    assert seen == {77, 1234}
    # top_k = N and N + 5 are top_k = 0
    for st in low + mid + high:
        base = draw(row, st, temperature=1.5)[0]
        assert draw(row, st, temperature=1.5, top_k=4097)[0] == base == draw(row, st, temperature=1.5, top_k=4102)[0]
        assert R.Ref(row, 1.5).deviation(base, R.u_of(seed, st, 3)) <= EPS
    # fewer finite scores than k: the two finite ones share the draw
    few = np.full(300, NEG, dtype=np.float32)
    few[[5, 250]] = [1.0, 1.0]
    assert [draw(few, st, top_k=10)[0] for st in (low[0], high[0])] == [5, 250]
    # weights [0.5, 0.3, 0.2] as logits: top_p = 0.79 never gives the third id, 0.81 does for u > 0.8
    w = np.log(np.array([0.5, 0.3, 0.2])).astype(np.float32)
    wb = _bf16(w)
    for st in low + mid + high:
        u = R.u_of(seed, st, 3)
        for tp in (0.79, 0.81):
            ref = R.Ref(wb, 1.0, 0, tp)
            assert ref.keep.tolist() == [True, True, tp > 0.8] and ref.decisive(u, 2.0 ** -8)
            assert draw(w, st, top_p=tp)[0] == ref.token(u)
    assert {draw(w, st, top_p=0.79)[0] for st in high} == {1} and {draw(w, st, top_p=0.81)[0] for st in high} == {2}
    # top_p = 1e-6: the argmax
    for st in low + high:
        assert draw(row, st, top_p=1e-6)[0] == 1234
    # a penalised id drops out of the top-k it would otherwise be in
    pen = np.array([5.0, 4.0, 3.0, -9.0], dtype=np.float32)
    assert {draw(pen, st, seq=(0, 9, 8), top_k=2, penalty=2.0)[0] for st in low + mid + high} == {1, 2}   # 5 / 2 = 2.5
    assert {draw(pen, st, seq=(7, 9, 8), top_k=2, penalty=2.0)[0] for st in low + mid + high} == {0, 1}
    # the only kept id is the last column, and separately the first; N = 1, 13, 4097, MAXA compact and N = V full
    for N in (1, 13, 4097, MAXA):
        ids = list(range(3, 3 + 9 * N, 9))
        for at in (0, N - 1):
            r = np.full(N, NEG, dtype=np.float32)
            r[at] = -2.0
            for st in (low[0], high[0]):
                assert draw(r, st, ids=ids, temperature=0.7, top_k=50, top_p=0.9)[0] == ids[at], (N, at)
    for at in (0, V - 1):
        r = np.full(V, -30.0, dtype=np.float32)
        r[at] = 8.0
        assert draw(r, high[0], temperature=0.7, top_k=50, top_p=0.9)[0] == at
    # seen and banned entries of a compact row: 6 / 1.2 = 5 < 5.5, and the bigram (7, 40) bans 40
    ids = [40, 50, 60]
    assert {draw([6.0, 5.5, -9.0], st, seq=(40, 9, 8), ids=ids, penalty=1.2, top_k=1)[0] for st in low + high} == {50}
    assert {draw([6.0, 5.5, -9.0], st, seq=(41, 9, 8), ids=ids, penalty=1.2, top_k=1)[0] for st in low + high} == {40}
    assert {draw([6.0, 5.5, -9.0], st, seq=(7, 40, 5, 7), ids=ids, ngram=2)[0] for st in low + mid + high} <= {50, 60}
    # NaN entries are never chosen; all banned / -inf / NaN: token 0
    nan = [float("nan"), 1.0, float("nan"), 1.0]
    assert {draw(nan, st)[0] for st in low + mid + high} == {1, 3}
    assert draw([float("nan"), NEG, float("nan")], mid[0], ids=[10, 20, 30])[0] == 0
    assert draw([3.0, 2.0], mid[0], seq=(7, 5, 7, 9, 7), ids=[5, 9], ngram=2)[0] == 0
    assert draw([NEG] * 9, mid[0])[0] == 0
    # u below 2^-20: the first kept id; u above 1 - 2^-20: the last kept id with w > 0
    flat = np.zeros(1000, dtype=np.float32)
    flat[:10] = NEG
    flat[990:] = -200.0        # kept, but exp(-200) = 0 in fp32 and below the fixed-point floor: never chosen
    tiny = _find_stream(seed, 3, lambda u: u < 2.0 ** -20)
    top = _find_stream(seed, 3, lambda u: u > 1 - 2.0 ** -20)
    assert draw(flat, tiny)[0] == 10 and draw(flat, top)[0] == 989


@pytest.mark.gpu
def test_gpu_gen_sample_row_with_an_unaligned_logits_pointer(dev):
    """Row 1 of a batch with an odd row stride: its logits are 2-byte aligned only."""
    ops = import_module(f"{PKG}.ops")
    g = torch.Generator().manual_seed(5)
    N = 4099
    base = (torch.randn(2, N, generator=g) * 4).bfloat16()
    assert base.stride(0) % 8 != 0
    seq = torch.tensor([[1, 2, 3, 0], [3, 2, 1, 0]], dtype=torch.int64)
    kw = dict(repetition_penalty=1.2, no_repeat_ngram_size=2, temperature=0.7, top_k=50, top_p=0.9, seed=5)
    both_seq, both_cur = seq.to(dev), torch.tensor([3, 3], dtype=torch.int32, device=dev)
    both = ops.gen_sample(base.to(dev), both_seq, both_cur, streams=torch.tensor([8, 9], device=dev), **kw)
    for b in range(2):
        one = ops.gen_sample(base[b:b + 1].clone().to(dev), seq[b:b + 1].to(dev),
                             torch.tensor([3], dtype=torch.int32, device=dev), streams=torch.tensor([8 + b], device=dev), **kw)
        assert torch.equal(one, both[b:b + 1])
        ref = R.Ref(G.process_scores(base[b].float().numpy(), [int(t) for t in seq[b, :3]], 1.2, 2), 0.7, 50, 0.9)
        assert ref.deviation(int(both[b]), R.u_of(5, 8 + b, 3)) <= EPS


@pytest.mark.gpu
@pytest.mark.parametrize("A", [None, 700])
def test_gpu_gen_sample_is_batch_invariant_and_repeatable(A, dev):
    """Row b of a 16-row call == the nb = 1 call on row b with its stream; a permutation of the rows
    permutes the results; two identical calls agree; and the compact call equals the full-row call on
    logits that are -inf outside the set."""
    ops = import_module(f"{PKG}.ops")
    rows = [_seq_scores(100 * s + 2, n=150 + 11 * s) for s in range(16)]
    N = V if A is None else A
    g = torch.Generator().manual_seed(17)
    lg = (torch.randn(16, V, generator=g) * 4).bfloat16()
    ids = None if A is None else torch.unique(torch.cat([torch.randint(0, V, (A,), generator=g), torch.arange(0, 60, 2)]))[:A]
    lens = [len(s) for s, _ in rows]
    smax = max(lens) + 2
    seq = torch.zeros((16, smax), dtype=torch.int64)
    for b, (s, _) in enumerate(rows):
        seq[b, :lens[b]] = torch.tensor(s)
    streams = torch.tensor([5 * b + 2 ** 33 for b in range(16)], dtype=torch.int64)
    kw = dict(repetition_penalty=1.2, no_repeat_ngram_size=2, temperature=0.7, top_k=50, top_p=0.9, seed=4242)
    sc = lg if ids is None else lg[:, ids]
    ids_d = None if ids is None else ids.to(torch.int32).to(dev)
    assert sc.shape[1] == N

    def run(order):
        o = torch.tensor(order)
        seq_d = seq[o].to(dev)
        cur = torch.tensor([lens[i] for i in order], dtype=torch.int32, device=dev)
        u = torch.empty(len(order), dtype=torch.float32, device=dev)
        out = ops.gen_sample(sc[o].contiguous().to(dev), seq_d, cur, ids=ids_d, streams=streams[o].to(dev), u_out=u, **kw)
        return out.cpu(), u.cpu(), seq_d.cpu(), cur.cpu()

    full = run(list(range(16)))
    again = run(list(range(16)))
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    perm = [int(i) for i in torch.randperm(16, generator=g)]
    p = run(perm)
    assert torch.equal(p[0], full[0][perm]) and torch.equal(p[1], full[1][perm]) and torch.equal(p[2], full[2][perm])
    for b in range(16):
        one = run([b])
        assert torch.equal(one[0], full[0][b:b + 1]) and torch.equal(one[1], full[1][b:b + 1])
        assert torch.equal(one[2][0], full[2][b]) and int(one[3]) == int(full[3][b])
    if ids is not None:   # the compact call against the full row, -inf outside the set
        masked = torch.full((16, V), float("-inf")).bfloat16()
        masked[:, ids] = lg[:, ids]
        seq_d = seq.to(dev)
        cur = torch.tensor(lens, dtype=torch.int32, device=dev)
        wide = ops.gen_sample(masked.to(dev), seq_d, cur, streams=streams.to(dev), **kw)
        assert torch.equal(wide.cpu(), full[0]) and torch.equal(seq_d.cpu(), full[2])


# -------------------------------------------------------------------- GPU, end to end ----

KW = dict(repetition_penalty=1.2, no_repeat_ngram_size=2, eos_token_id=())
SKW = dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.9, seed=0x5EED5EED5EED)
ALLOWED = sorted(set(range(0, 600, 2)) | {151646, 7, V - 1})


def _flat(x):
    return [r for g in x for r in g]


def _same(a, b):
    (oa, la), (ob, lb) = a, b
    assert len(oa) == len(ob)
    for r in range(len(oa)):
        assert torch.equal(oa[r], ob[r]), r
        assert len(la[r]) == len(lb[r]) and all(torch.equal(x, y) for x, y in zip(la[r], lb[r])), r


def _entry(run3, run_g, which):
    """-> call(**kw) -> (outs, logs) as flat per-row lists, alone(r, **kw) the same for row r on its own."""
    if which == "batch":
        gen, model, prompts = run3["gen"], run3["model"], run3["prompts"]

        def call(**kw):
            return gen.generate_batch(model, prompts, max_new_tokens=8, return_logits=True, **KW, **kw)

        def alone(r, **kw):
            return gen.generate_batch(model, [prompts[r]], max_new_tokens=8, return_logits=True, sample_streams=[r], **KW, **kw)
    elif which == "single":
        gen, model, prompts = run3["gen"], run3["model"], run3["prompts"]

        def call(**kw):
            res = [gen.generate(model, *p, max_new_tokens=8, return_logits=True, sample_streams=r, **KW, **kw)
                   for r, p in enumerate(prompts)]
            return [o for o, _ in res], [l for _, l in res]
        alone = None
    else:
        gen, model, groups = run_g["gen"], run_g["model"], run_g["groups"]

        def call(**kw):
            o, l = gen.generate_grouped(model, groups, max_new_tokens=8, return_logits=True, **KW, **kw)
            return _flat(o), _flat(l)

        def alone(r, **kw):
            gi, qi = run_g["flat"][r]
            px, sizes, qs = groups[gi]
            o, l = gen.generate_grouped(model, [(px, sizes, [qs[qi]])], max_new_tokens=8, return_logits=True,
                                        sample_streams=[r], **KW, **kw)
            return _flat(o), _flat(l)
    return call, alone


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["batch", "single", "grouped"])
def test_gpu_sampled_routes_give_the_same_bits(which, run3, run_g, dev):
    call, alone = _entry(run3, run_g, which)
    base = call(**SKW)
    assert len(base[0]) == 3 and all(len(l) == 8 for l in base[1])
    _same(call(graph=False, stop_check_every=0, **SKW), base)
    _same(call(stop_check_every=3, **SKW), base)
    _same(call(graph=False, stop_check_every=1, **SKW), base)
    a = call(allowed_token_ids=ALLOWED, **SKW)
    assert all(int(t) in ALLOWED for o, l in zip(*a) for t in o[0, -8:]) and a[1][0][0].shape == (1, len(ALLOWED))
    _same(call(allowed_token_ids=ALLOWED, restrict_head=False, **SKW), a)
    _same(call(allowed_token_ids=ALLOWED, restrict_head=True, graph=False, stop_check_every=3, **SKW), a)
    if which == "single":   # the prefill is generate_batch()'s own code: the first draw and its logits row, bit for bit
        outs_b, logs_b = _entry(run3, run_g, "batch")[0](**SKW)
        for r, L in enumerate(LENS):
            assert torch.equal(base[0][r][:, :L + 1], outs_b[r][:, :L + 1]) and torch.equal(base[1][r][0], logs_b[r][0])
    else:
        for r in range(3):
            one = alone(r, **SKW)
            _same(one, ([base[0][r]], [base[1][r]]))
            one = alone(r, allowed_token_ids=ALLOWED, **SKW)
            _same(one, ([a[0][r]], [a[1][r]]))


@pytest.mark.gpu
def test_gpu_sampled_chunks_seeds_and_streams(run3, run_g, dev):
    gen, model, prompts = run3["gen"], run3["model"], run3["prompts"]
    kw = dict(max_new_tokens=4, **KW, **SKW)
    many = [prompts[i % 3] for i in range(17)]
    streams = [100 + 3 * i for i in range(17)]
    outs = gen.generate_batch(model, many, sample_streams=streams, **kw)
    first = gen.generate_batch(model, many[:16], sample_streams=streams[:16], **kw)
    last = gen.generate_batch(model, many[16:], sample_streams=streams[16:], **kw)
    assert len(outs) == 17 and all(torch.equal(a, b) for a, b in zip(outs, first + last))
    # the grouped form: 17 questions of one group span two chunks; the flattened index is the default stream
    px, sizes, qs = run_g["groups"][0]
    g17 = gen.generate_grouped(run_g["model"], [(px, sizes, [qs[1]] * 17)], **kw)[0]
    g1 = gen.generate_grouped(run_g["model"], [(px, sizes, [qs[1]])], sample_streams=[16], **kw)[0]
    assert torch.equal(g17[16], g1[0])
    # another seed changes some row; another stream changes that row and no other
    kw8 = dict(max_new_tokens=8, **KW)
    base = gen.generate_batch(model, prompts, **kw8, **SKW)
    other = gen.generate_batch(model, prompts, **kw8, **{**SKW, "seed": SKW["seed"] + 1})
    assert any(not torch.equal(a, b) for a, b in zip(base, other))
    moved = gen.generate_batch(model, prompts, sample_streams=[0, 77, 2], **kw8, **SKW)
    assert torch.equal(moved[0], base[0]) and torch.equal(moved[2], base[2]) and not torch.equal(moved[1], base[1])


def _teacher_forced(orc, rows, temperature, top_k, top_p, seed, min_share):
    """rows: (ids, px, sizes, out, logs, stream).  The returned logits rows against the oracle model, and
    every token against the reference built from the returned row."""
    refs = []
    for ids, px, sizes, out, logs, stream in rows:
        L = int(ids.shape[1])
        seq = out[0].cpu().tolist()
        assert out.shape == (1, L + 8) and seq[:L] == ids[0].cpu().tolist() and len(logs) == 8
        full, _ = orc(torch.tensor([seq[:-1]]), px.float().cpu(), sizes)
        for t, lg in enumerate(logs):
            got = lg.float().cpu()[0]
            want = full[0, L - 1 + t]
            cos = torch.nn.functional.cosine_similarity(got, want, dim=0)
            assert cos > 0.999, (stream, t, float(cos))
            assert (got - want).abs().max() < 0.05 * want.abs().max() + 0.05, (stream, t)
            ref = R.Ref(G.process_scores(got.numpy(), seq[:L + t], 1.2, 2), temperature, top_k, top_p)
            refs.append((ref, R.u_of(seed, stream, L + t), seq[L + t], stream, t))
    share = sum(ref.decisive(u) for ref, u, *_ in refs) / len(refs)
    print(f"T = {temperature}: decisive share {share:.3f} of {len(refs)} draws")
    assert share >= min_share, share
    worst = 0.0
    for ref, u, tok, stream, t in refs:
        d = ref.deviation(tok, u)
        worst = max(worst, d)
        assert d <= EPS, (stream, t, tok, ref.token(u), d)
    print(f"T = {temperature}: largest acceptance deviation {worst:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("temperature,min_share", [(0.7, 0.0), (0.05, 0.9)])
def test_gpu_sampled_generate_batch_matches_oracle_teacher_forced(temperature, min_share, run3, dev):
    """The tiny student's logits are nearly flat; T = 0.05 sharpens them so that most draws are decisive."""
    from model_fixtures import tiny_weights
    from oracle.model import OracleLlava
    gen, model, prompts = run3["gen"], run3["model"], run3["prompts"]
    skw = {**SKW, "temperature": temperature}
    outs, logs = gen.generate_batch(model, prompts, max_new_tokens=8, return_logits=True, **KW, **skw)
    orc = OracleLlava(tiny_weights(False, 5), run3["cfg"])
    _teacher_forced(orc, [(*prompts[r], outs[r], logs[r], r) for r in range(3)], temperature, 50, 0.9, SKW["seed"], min_share)


@pytest.mark.gpu
def test_gpu_sampled_generate_grouped_matches_oracle_teacher_forced(run_g, dev):
    from model_fixtures import tiny_weights
    from oracle.model import OracleLlava
    gen, model, groups = run_g["gen"], run_g["model"], run_g["groups"]
    skw = {**SKW, "temperature": 0.05}
    outs, logs = gen.generate_grouped(model, groups, max_new_tokens=8, return_logits=True, **KW, **skw)
    orc = OracleLlava(tiny_weights(False, 5), run_g["cfg"])
    rows = [(groups[gi][2][qi], groups[gi][0], groups[gi][1], outs[gi][qi], logs[gi][qi], r)
            for r, (gi, qi) in enumerate(run_g["flat"])]
    _teacher_forced(orc, rows, 0.05, 50, 0.9, SKW["seed"], 0.9)


@pytest.mark.gpu
def test_gpu_sampled_top_k_1_is_the_greedy_call(run3, run_g, monkeypatch, dev):
    gen, model, prompts = run3["gen"], run3["model"], run3["prompts"]
    outs, logs = gen.generate_batch(model, prompts, max_new_tokens=8, return_logits=True, do_sample=True, top_k=1,
                                    temperature=0.7, seed=1, **KW)
    for r, L in enumerate(LENS):
        seq, greedy = outs[r][0].cpu().tolist(), run3["outs"][r][0].cpu().tolist()
        for t in range(8):
            s = G.process_scores(logs[r][t].float().cpu()[0].numpy(), seq[:L + t], 1.2, 2)
            tied = np.nonzero(s == s.max())[0].tolist()
            assert seq[L + t] in tied, (r, t)
            if len(tied) > 1 or seq[L + t] != greedy[L + t]:
                break   # past a tie the sequences may part
            assert torch.equal(logs[r][t], run3["logs"][r][t])
        else:
            assert seq == greedy
    # do_sample=False with every sampling argument set: the greedy launches, gen_sample never called
    ops = import_module(f"{PKG}.ops")
    monkeypatch.setattr(ops, "gen_sample", lambda *a, **kw: (_ for _ in ()).throw(AssertionError("gen_sample")))
    stats = {}
    g2 = gen.generate_batch(model, prompts, max_new_tokens=8, do_sample=False, temperature=0.7, top_k=50, top_p=0.9,
                            seed=3, sample_streams=[9, 9, 9], stats=stats, **KW)
    assert all(torch.equal(a, b) for a, b in zip(g2, run3["outs"])) and "seed" not in stats
    gg = gen.generate_grouped(run_g["model"], run_g["groups"], max_new_tokens=8, top_k=5, top_p=0.5, seed=3, **KW)
    assert all(torch.equal(a, b) for a, b in zip(_flat(gg), _flat(run_g["outs"])))


@pytest.mark.gpu
def test_gpu_sampled_eos_cuts_a_row_and_stats_report_the_seed(run3, dev):
    gen, model, prompts = run3["gen"], run3["model"], run3["prompts"]
    kw = dict(max_new_tokens=8, repetition_penalty=1.2, no_repeat_ngram_size=2)
    stats = {}
    full = [o[0].cpu().tolist() for o in gen.generate_batch(model, prompts, eos_token_id=(), stats=stats, **kw, **SKW)]
    assert stats["seed"] == SKW["seed"]
    eos = full[1][LENS[1] + 2]   # the token row 1 drew third
    stats = {}
    cut = gen.generate_batch(model, [prompts[1]], eos_token_id=(eos,), sample_streams=[1], stats=stats, **kw, **SKW)
    new = full[1][LENS[1]:]
    assert cut[0][0].cpu().tolist() == full[1][:LENS[1] + new.index(eos) + 1]
    assert stats["steps_run"][0] < stats["steps_max"][0] and stats["seed"] == SKW["seed"]
    cut = gen.generate_batch(model, prompts, eos_token_id=(eos,), **kw, **SKW)
    for r, L in enumerate(LENS):
        new = full[r][L:]
        assert cut[r][0].cpu().tolist() == (full[r][:L + new.index(eos) + 1] if eos in new else full[r]), r
    # seed=None: torch's default CPU generator; the seed used is reported and reproduces the tokens
    torch.manual_seed(7)
    skw = {k: v for k, v in SKW.items() if k != "seed"}
    s1, s2 = {}, {}
    a = gen.generate_batch(model, prompts, eos_token_id=(), stats=s1, **kw, **skw)
    b = gen.generate_batch(model, prompts, eos_token_id=(), stats=s2, **kw, **skw)
    assert 0 <= s1["seed"] < 2 ** 64 and 0 <= s2["seed"] < 2 ** 64 and s1["seed"] != s2["seed"]
    torch.manual_seed(7)
    s3 = {}
    gen.generate_batch(model, prompts[:1], max_new_tokens=1, eos_token_id=(), stats=s3, **skw)
    assert s3["seed"] == s1["seed"]                # torch.manual_seed governs it
    for outs, s in ((a, s1), (b, s2)):
        again = gen.generate_batch(model, prompts, eos_token_id=(), seed=s["seed"], **kw, **skw)
        assert all(torch.equal(x, y) for x, y in zip(outs, again))
