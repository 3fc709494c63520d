"""Constrained decoding (allowed_token_ids of generate() / generate_batch() / generate_grouped()).
The token-choice oracle (oracle.generation.process_scores, -inf outside the ids, argmax) against
transformers' own processors followed by an additive 0 / -inf mask, argument validation, the support
query and the id normalisation (CPU); the gathered GEMVs against the full head's columns by
torch.equal, kd_gen_select_ids against the oracle with edges that each see one wrong entry, and the
three entry points on the tiny student, bit for bit across graph / eager, gathered / full head,
stop_check_every and alone / in a batch, and teacher-forced against the CPU oracle model (GPU)."""
import ctypes
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import generation as G
from test_generate import CASES, _seq_scores

PKG = "knowledge_distillation_for_sensory_substitution_in_multimodal_models_amd"
V = 151936
NEG = -np.inf


def _masked(scores, seq, penalty, ngram, ids):
    """The oracle: the processors' scores, then -inf on every id that is not allowed."""
    s = G.process_scores(scores, seq, penalty, ngram)
    m = np.full_like(s, NEG)
    m[np.asarray(ids)] = s[np.asarray(ids)]
    return m


def _choose(scores, seq, penalty, ngram, ids):
    return int(np.argmax(_masked(scores, seq, penalty, ngram, ids)))


def _choose_compact(row, ids, seq, penalty, ngram):
    """The oracle's choice from a compact row (column j: the score of ids[j])."""
    full = np.zeros(V, dtype=np.float32)
    full[np.asarray(ids)] = np.asarray(row, dtype=np.float32)
    return _choose(full, seq, penalty, ngram, ids)


# ----------------------------------------------------------------------------- CPU ----

@pytest.mark.parametrize("penalty,ngram", CASES)
def test_oracle_matches_transformers_processors_then_mask(penalty, ngram):
    from transformers.generation.logits_process import (LogitsProcessorList, NoRepeatNGramLogitsProcessor,
                                                        RepetitionPenaltyLogitsProcessor)
    seq, scores = _seq_scores(int(penalty * 10) + ngram)
    procs = LogitsProcessorList()
    if penalty != 1.0:
        procs.append(RepetitionPenaltyLogitsProcessor(penalty))
    if ngram > 0:
        procs.append(NoRepeatNGramLogitsProcessor(ngram))
    ref = procs(torch.tensor([seq]), torch.from_numpy(scores)[None].clone())[0]
    free = int(torch.argmax(ref))                       # the unrestricted choice
    g = np.random.default_rng(ngram)
    drawn = g.integers(0, V, 300)
    with_free = np.unique(np.concatenate([drawn, np.arange(0, 60), [free, 151646]]))
    without = np.setdiff1d(with_free, [free])            # the unrestricted argmax is not allowed
    seen_only = np.unique(np.array(seq))                 # every allowed id penalised, some banned
    for ids in (with_free, without, seen_only, np.array([V - 1])):
        mask = torch.full((V,), float("-inf"))
        mask[torch.from_numpy(ids)] = 0.0                # the user processor: 0 on allowed ids, -inf elsewhere
        want = (ref + mask).numpy()
        np.testing.assert_array_equal(_masked(scores, seq, penalty, ngram, ids), want)
        assert _choose(scores, seq, penalty, ngram, ids) == int(np.argmax(want))
    assert _choose(scores, seq, penalty, ngram, with_free) == free
    assert free not in without and _choose(scores, seq, penalty, ngram, without) != free


def test_abi_allowed_symbols_reject_bad_arguments():
    """Validation runs before any device work: null pointers -> KD_ERR_ARG (7), bad shapes ->
    KD_ERR_SHAPE (1) (host memory stands in for the pointers: it is never dereferenced)."""
    NV = import_module(f"{PKG}._native")
    lib = NV.lib()
    MAXA = NV.KD_GEN_ALLOWED_MAX
    assert MAXA == 16384
    assert lib.kd_gemv_gather(None, None, 896, None, 4, None, V, 896, None) == 7
    assert lib.kd_gemv_batch_gather(None, 896, 1, None, 896, None, 4, None, V, 896, None) == 7
    assert lib.kd_gen_select_ids(None, 4, None, 4, None, 8, 1, None, 1.2, 2, None, None) == 7
    assert b"null" in lib.kd_last_error()
    buf = ctypes.create_string_buffer(256 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    assert lib.kd_gemv_gather(p, p, 896, None, 4, p, V, 896, None) == 7                       # ids alone null
    assert lib.kd_gemv_batch_gather(p, 896, 1, p, 896, None, 4, p, V, 896, None) == 7
    assert lib.kd_gemv_gather(p, p, 896, p, 0, p, V, 896, None) == 1                          # A < 1
    assert lib.kd_gemv_gather(p, p, 896, p, V + 1, p, V, 896, None) == 1                      # A > N_full
    assert lib.kd_gemv_gather(p, p, 900, p, 4, p, V, 900, None) == 1                          # K % 8
    assert lib.kd_gemv_gather(p, p, 896, p, 4, p, 4864, 896, None) == 1                       # unsupported shape
    assert b"kd_gemv_gather_supported" in lib.kd_last_error()
    assert lib.kd_gemv_batch_gather(p, 896, 0, p, 896, p, 4, p, V, 896, None) == 1            # nb < 1
    assert lib.kd_gemv_batch_gather(p, 896, 17, p, 896, p, 4, p, V, 896, None) == 1           # nb > 16
    assert lib.kd_gemv_batch_gather(p, 896, 1, p, 896, p, 0, p, V, 896, None) == 1            # A < 1
    assert lib.kd_gemv_batch_gather(p, 896, 1, p, 896, p, 4, p, 4864, 896, None) == 1         # unsupported shape
    assert lib.kd_gemv_batch_gather(p, 2048, 1, p, 2048, p, 4, p, V, 2048, None) == 1         # K split over slices
    assert lib.kd_gen_select_ids(p, 4, p, 0, p, 8, 1, p, 1.2, 2, None, None) == 1             # A < 1
    assert lib.kd_gen_select_ids(p, MAXA + 1, p, MAXA + 1, p, 8, 1, p, 1.2, 2, None, None) == 1   # A > max
    assert lib.kd_gen_select_ids(p, 3, p, 4, p, 8, 1, p, 1.2, 2, None, None) == 1             # ld < A
    assert lib.kd_gen_select_ids(p, 4, p, 4, p, 8, 0, p, 1.2, 2, None, None) == 1             # nb < 1
    assert lib.kd_gen_select_ids(p, 4, p, 4, p, 8, 17, p, 1.2, 2, None, None) == 1            # nb > 16
    assert lib.kd_gen_select_ids(p, 4, p, 4, p, 0, 1, p, 1.2, 2, None, None) == 1             # smax < 1
    assert lib.kd_gen_select_ids(p, 4, p, 4, p, 8, 1, p, 0.0, 2, None, None) == 7             # penalty <= 0
    assert lib.kd_gen_select_ids(p, 4, p, 4, p, 8, 1, p, 1.2, -1, None, None) == 7            # ngram < 0


def test_gemv_gather_supported_is_where_a_row_does_not_depend_on_n():
    lib = import_module(f"{PKG}._native").lib()
    ops = import_module(f"{PKG}.ops")
    assert lib.kd_gemv_gather_supported(V, 896) == 1 and ops.gemv_gather_supported(V, 896) is True
    assert lib.kd_gemv_gather_supported(V, 128) == 1
    assert lib.kd_gemv_gather_supported(4864, 896) == 0 and ops.gemv_gather_supported(4864, 896) is False
    assert lib.kd_gemv_gather_supported(896, 4864) == 0     # the workgroup-per-row kd_gemv, a split K in kd_gemv_batch
    assert lib.kd_gemv_gather_supported(V, 2048) == 0       # more 32-k steps than one K slice holds
    assert lib.kd_gemv_gather_supported(V, 900) == 0 and lib.kd_gemv_gather_supported(0, 896) == 0
    # the set is exactly the plans without a split: those kd_gemv_batch runs without a workspace, tile per wave
    assert lib.kd_gemv_gather_supported(32753, 1536) == 1 and lib.kd_gemv_gather_supported(32752, 1536) == 0
    assert lib.kd_gemv_gather_supported(32753, 1544) == 0


def test_allowed_ids_are_sorted_unique_and_checked():
    gen = import_module(f"{PKG}.generation")
    MAXA = import_module(f"{PKG}._native").KD_GEN_ALLOWED_MAX
    want = torch.tensor([0, 3, 9, V - 1], dtype=torch.int32)
    for given in ([9, 3, V - 1, 0, 3, 9], (9, 0, 3, V - 1), torch.tensor([[9, 3], [0, V - 1]]),
                  np.array([V - 1, 9, 3, 0]), torch.tensor([3, 9, 0, V - 1, 3], dtype=torch.int32)):
        got = gen.allowed_ids(given, V)
        assert got.dtype == torch.int32 and got.device.type == "cpu" and torch.equal(got, want)
    assert gen.allowed_ids(range(MAXA), V).numel() == MAXA
    assert gen.allowed_ids(list(range(MAXA)) * 2, V).numel() == MAXA      # counted after deduplication
    for bad in ([], torch.tensor([], dtype=torch.int64), [-1, 5], [5, V], range(MAXA + 1), [1.5, 2.0]):
        with pytest.raises(ValueError, match="allowed_token_ids"):
            gen.allowed_ids(bad, V)


def test_entry_points_refuse_a_bad_allowed_set_before_any_device_work():
    """A model stub with nothing but the sizes is enough: the checks come first."""
    gen = import_module(f"{PKG}.generation")
    IMG = import_module(f"{PKG}.modeling").IMAGE_TOKEN_ID

    def stub(vocab, hidden):
        return SimpleNamespace(cfg=SimpleNamespace(text=SimpleNamespace(vocab=vocab, hidden=hidden), image_token_id=IMG))

    ids = torch.tensor([[5, 6, IMG, IMG, 7, 8]], dtype=torch.int64)
    px, sizes = torch.zeros(1, 2, 3, 384, 384), torch.tensor([[336, 336]])
    calls = (lambda m, **kw: gen.generate(m, ids, px, sizes, **kw),
             lambda m, **kw: gen.generate_batch(m, [(ids, px, sizes)], **kw),
             lambda m, **kw: gen.generate_grouped(m, [(px, sizes, [ids])], **kw))
    for call in calls:
        for bad in ([], [-1], [V], range(gen.KD_GEN_ALLOWED_MAX + 1)):
            with pytest.raises(ValueError, match="allowed_token_ids"):
                call(stub(V, 896), allowed_token_ids=bad)
        with pytest.raises(ValueError, match="restrict_head"):
            call(stub(4864, 896), allowed_token_ids=[1, 2], restrict_head=True)    # no gathered head for this shape
        with pytest.raises(ValueError, match="restrict_head"):
            call(stub(V, 896), restrict_head=False)                                # nothing to restrict


# ----------------------------------------------------------------------------- GPU ----

EDGE_IDS = [0, 15, 16, 31, 32, 4095, 4096, V - 17, V - 16, V - 1]   # both ends, both sides of 16-row tile boundaries


def _gather_ids(A, dev):
    if A == 1:
        return torch.tensor([V - 1], dtype=torch.int32, device=dev)
    g = np.random.default_rng(A)
    ids = set(EDGE_IDS)
    while len(ids) < A:
        ids.update(int(i) for i in g.integers(0, V, A - len(ids)))
    return torch.tensor(sorted(ids), dtype=torch.int32, device=dev)


@pytest.fixture(scope="module")
def heads(dev):
    """Per K one [V, K] weight (row stride K + 8, as the span views), 16 rows of x and the full heads:
    computed once, left unchanged."""
    ops = import_module(f"{PKG}.ops")
    out = {}
    for K in (896, 128):
        g = torch.Generator(device=dev).manual_seed(K)
        w = (torch.randn(V, K + 8, generator=g, device=dev) * 0.05).bfloat16()[:, :K]
        x = torch.randn(16, K, generator=g, device=dev).bfloat16()
        out[K] = SimpleNamespace(w=w, x=x, full={nb: ops.gemv_batch(x[:nb].contiguous(), w) for nb in (1, 3, 16)},
                                 one=ops.gemv(x[:1].contiguous(), w))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("K", [896, 128])
@pytest.mark.parametrize("nb", [1, 3, 16])
def test_gpu_gemv_gather_has_the_full_heads_bits(nb, K, heads, dev):
    ops = import_module(f"{PKG}.ops")
    h = heads[K]
    for A in (1, 17, 700):
        ids = _gather_ids(A, dev)
        assert ids.numel() == A and (A == 1 or set(EDGE_IDS) <= set(ids.tolist()))
        xb = h.x[:nb].contiguous()
        got = ops.gemv_batch_gather(xb, h.w, ids)
        assert got.shape == (nb, A) and got.dtype == torch.bfloat16
        assert torch.equal(got, h.full[nb][:, ids.long()]), (A, "gemv_batch columns")
        for b in range(nb):   # row b alone == row b inside the batch
            alone = ops.gemv_batch_gather(h.x[b:b + 1].contiguous(), h.w, ids)
            assert torch.equal(alone[0], got[b]), (A, b)
        if nb == 1:
            one = ops.gemv_gather(xb, h.w, ids)
            assert one.shape == (1, A) and torch.equal(one, h.one[:, ids.long()]), (A, "gemv columns")


@pytest.mark.gpu
def test_gpu_gemv_gather_refuses_an_unsupported_shape(dev):
    ops = import_module(f"{PKG}.ops")
    NV = import_module(f"{PKG}._native")
    w = torch.zeros(4864, 896, dtype=torch.bfloat16, device=dev)
    x = torch.zeros(1, 896, dtype=torch.bfloat16, device=dev)
    ids = torch.tensor([1, 2], dtype=torch.int32, device=dev)
    for fn in (ops.gemv_gather, ops.gemv_batch_gather):
        with pytest.raises(NV.KdError, match="KD_ERR_SHAPE"):
            fn(x, w, ids)


def _select(dev, rows, ids, penalty, ngram, smax=None, lens=None):
    """kd_gen_select_ids over rows = [(seq, compact scores [A])]: -> (out, seq after, cur after) on the host."""
    ops = import_module(f"{PKG}.ops")
    lens = [len(s) for s, _ in rows] if lens is None else lens
    smax = max(lens) + 3 if smax is None else smax
    seq = torch.zeros((len(rows), smax), dtype=torch.int64)
    for b, (s, _) in enumerate(rows):
        seq[b, :len(s)] = torch.tensor(s, dtype=torch.int64)
    sc = torch.stack([torch.as_tensor(np.asarray(c, dtype=np.float32)).bfloat16() for _, c in rows])
    seq_d = seq.to(dev)
    cur = torch.tensor(lens, dtype=torch.int32, device=dev)
    out = torch.full((len(rows),), -7, dtype=torch.int64, device=dev)
    ops.gen_select_ids(sc.to(dev), torch.tensor(ids, dtype=torch.int32, device=dev), seq_d, cur, penalty, ngram, out=out)
    return out.cpu().tolist(), seq_d.cpu(), cur.cpu().tolist(), seq


@pytest.mark.gpu
@pytest.mark.parametrize("penalty,ngram", CASES)
def test_gpu_gen_select_ids_matches_oracle(penalty, ngram, dev):
    """The ragged rows of the batch-select test; the allowed set holds half of the small ids the
    sequences repeat (penalised and banned entries), the repeated high id and 300 drawn ones."""
    rows = [_seq_scores(100 * seed + ngram, n=200 + 37 * seed) for seed in range(4)]
    g = np.random.default_rng(7 + ngram)
    ids = np.unique(np.concatenate([g.integers(0, V, 300), np.arange(0, 60, 2), [151646, 7]]))
    bf = [torch.from_numpy(sc).bfloat16().float().numpy() for _, sc in rows]
    out, seq_after, cur, seq0 = _select(dev, [(s, f[ids]) for (s, _), f in zip(rows, bf)], ids.tolist(), penalty, ngram)
    for b, (s, _) in enumerate(rows):
        want = _choose(bf[b], s, penalty, ngram, ids)
        assert want in ids
        assert out[b] == want == int(seq_after[b, len(s)]), b
        assert cur[b] == len(s) + 1
        assert torch.equal(seq_after[b, :len(s)], seq0[b, :len(s)]) and torch.equal(seq_after[b, len(s) + 1:], seq0[b, len(s) + 1:])


@pytest.mark.gpu
def test_gpu_gen_select_ids_value_edges(dev):
    """Each case is decided by one entry: a wrong flag, a lost tie or a search that hits a
    neighbour changes the token."""
    MAXA = import_module(f"{PKG}._native").KD_GEN_ALLOWED_MAX

    def check(seq, ids, row, penalty, ngram, want):
        out, seq_after, cur, _ = _select(dev, [(seq, row)], ids, penalty, ngram)
        assert _choose_compact(torch.tensor(row).bfloat16().float().numpy(), ids, seq, penalty, ngram) == want
        assert out[0] == want == int(seq_after[0, len(seq)]) and cur[0] == len(seq) + 1, (out, want)

    # the global maximum lies outside the allowed set: the kernel never sees it, the oracle masks it
    full = np.full(V, -3.0, dtype=np.float32)
    full[100], full[200], full[300] = 9.0, 2.0, 1.0
    ids = [200, 300, 5000]
    assert _choose(full, [1, 2, 3], 1.2, 2, ids) == 200 and int(np.argmax(full)) == 100
    check([1, 2, 3], ids, full[ids], 1.2, 2, 200)
    # a tie between two allowed ids, in different waves and strides of the scan: the lower id wins ...
    A = 2000
    ids = list(range(10, 10 + 3 * A, 3))
    row = np.full(A, -1.0, dtype=np.float32)
    row[5] = row[A - 1] = 4.0
    check([1, 2, 3], ids, row, 1.2, 2, ids[5])
    row[A - 1] = 4.0625                       # ... and loses to a larger score (next bf16 above 4)
    check([1, 2, 3], ids, row, 1.2, 2, ids[A - 1])
    # penalty: an allowed id present in the sequence is penalised, an absent one is not
    ids = [40, 50, 60]
    check([40, 9, 8], ids, [6.0, 5.5, -9.0], 1.2, 0, 50)      # 6 / 1.2 = 5 < 5.5
    check([41, 9, 8], ids, [6.0, 5.5, -9.0], 1.2, 0, 40)      # 40 absent: 6 stands
    check([40, 9, 8], ids, [6.0, 5.5, -9.0], 1.0, 0, 40)      # no penalty
    check([50, 9, 8], ids, [-1.0, -0.9, -9.0], 1.2, 0, 40)    # negative scores are multiplied: -0.9 * 1.2 < -1
    check([9, 8, 50], ids, [-1.0, -0.9, -9.0], 1.2, 0, 40)    # ... wherever the id sits in the sequence
    # a sequence token just below / just above an allowed id is a search miss: nothing changes
    check([39, 41, 49, 51, 59, 61], ids, [6.0, 5.5, -9.0], 1.2, 0, 40)
    check([7, 39, 7, 41, 7], ids, [6.0, 5.5, -9.0], 1.0, 2, 40)   # the bigram bans fall on 39 and 41
    check([7, 40, 7, 41, 7], ids, [6.0, 5.5, -9.0], 1.0, 2, 50)   # ... and on 40 once it is the one
    # A = 1, and A not a multiple of 8
    check([3, 3, 3], [V - 1], [0.5], 1.2, 2, V - 1)
    ids = list(range(1000, 1013))
    row = np.arange(13, dtype=np.float32)
    check([1012, 5, 1011], ids, row, 2.0, 0, 1010)               # 12 -> 6, 11 -> 5.5, 10 stands
    # ids 0 and V - 1, both in the sequence: the penalty reaches the first and the last entry
    check([0, V - 1, 4], [0, 77, V - 1], [5.0, 4.5, 5.0], 1.2, 0, 77)
    check([4, 4, 4], [0, 77, V - 1], [5.0, 4.5, 5.0], 1.2, 0, 0)
    # A = KD_GEN_ALLOWED_MAX (and a size with 1024-thread strides that end unevenly): the winner in the
    # last entry, a penalised one next to it, a banned one first
    for A in (4097, MAXA):
        ids = list(range(3, 3 + 9 * A, 9))
        row = np.full(A, -2.0, dtype=np.float32)
        row[0], row[A - 2], row[A - 1] = 8.0, 6.0, 5.5
        seq = [5, ids[0], ids[A - 2], 5]                         # bigram (5, ids[0]) bans ids[0]; ids[-2] seen: 6 -> 5
        check(seq, ids, row, 1.2, 2, ids[A - 1])
    # every allowed id n-gram-banned: token 0, which is not allowed
    check([7, 5, 7, 9, 7], [5, 9], [3.0, 2.0], 1.2, 2, 0)
    check([7, 5, 7, 9, 8], [5, 9], [3.0, 2.0], 1.2, 2, 5)        # another last token: nothing banned
    # NaN never wins, -inf never wins over token 0
    out, _, _, _ = _select(dev, [([1, 2, 3], [float("nan"), 1.0, float("nan")])], [10, 20, 30], 1.2, 2)
    assert out == [20]
    out, _, _, _ = _select(dev, [([1, 2, 3], [float("nan"), NEG, float("nan")])], [10, 20, 30], 1.2, 2)
    assert out == [0]


@pytest.mark.gpu
def test_gpu_gen_select_ids_full_row_writes_out_only(dev):
    """Row 0 is full (cur == smax): out is written, seq untouched, cur = smax + 1; row 1 has room."""
    ids = [40, 50, 60]
    rows = [([40, 9, 8, 7], [6.0, 5.5, -9.0]), ([41, 9], [6.0, 5.5, -9.0])]
    out, seq_after, cur, seq0 = _select(dev, rows, ids, 1.2, 0, smax=4)
    assert out == [50, 40] and cur == [5, 3]
    assert torch.equal(seq_after[0], seq0[0])
    assert seq_after[1].tolist() == [41, 9, 40, 0]


KW = dict(repetition_penalty=1.2, no_repeat_ngram_size=2, eos_token_id=())
LENS = (1490, 1536, 1511)   # test_generate_batch's run3: just above the 1,485 image tokens of a 336x336 prompt
EOS_DEFAULT = 151645


def _draw_ids(seed, exclude):
    """About 300 seeded ids without `exclude` (and without the default EOS id)."""
    g = np.random.default_rng(seed)
    return sorted(set(int(i) for i in g.integers(0, V, 300)) - set(exclude) - {EOS_DEFAULT})


def _same(a, b):
    """(outs, logs) of two runs, any nesting: the same bits."""
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and torch.equal(a, b)
    return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


def _check_row(orc, ids, prompt_ids, px, sizes, out, lgs, n_new, first_full):
    """One row of a constrained run against the oracle model, teacher-forced on its own sequence:
    the compact logits on the allowed columns within the bounds the unrestricted tests hold the full
    row to, every token in the set and equal to the oracle's choice from the returned row, the first
    one also to the oracle's masked choice from the unrestricted run's full row."""
    L = int(prompt_ids.shape[1])
    seq = out[0].cpu().tolist()
    assert out.shape == (1, L + n_new) and len(lgs) == n_new and seq[:L] == prompt_ids[0].cpu().tolist()
    assert all(t in set(ids) for t in seq[L:]), seq[L:]
    full, _ = orc(torch.tensor([seq[:-1]]), px.float().cpu(), sizes)
    cols = torch.tensor(ids)
    for t, lg in enumerate(lgs):
        assert lg.shape == (1, len(ids)) and lg.dtype == torch.bfloat16
        got = lg.float().cpu()[0]
        want = full[0, L - 1 + t][cols]
        cos = torch.nn.functional.cosine_similarity(got, want, dim=0)
        print(f"step {t}: cos {float(cos):.6f} max|d| {float((got - want).abs().max()):.4f} "
              f"max|want| {float(want.abs().max()):.4f}")
        assert cos > 0.999, (t, float(cos))
        assert (got - want).abs().max() < 0.05 * want.abs().max() + 0.05, t
        assert seq[L + t] == _choose_compact(got.numpy(), ids, seq[:L + t], 1.2, 2), t
    assert seq[L] == _choose(first_full.float().cpu()[0].numpy(), seq[:L], 1.2, 2, ids)


@pytest.fixture(scope="module")
def tiny(dev):
    """The tiny student (real vocab, real 336x336 token layout), run3's three ragged prompts, the
    unrestricted first token and first full logits row of each, an allowed set of about 300 ids
    without those tokens and its 8-token constrained batched decode."""
    from model_fixtures import tiny_weights
    from oracle.model import OracleLlava
    data = import_module(f"{PKG}.data")
    gen = import_module(f"{PKG}.generation")
    M = import_module(f"{PKG}.modeling")
    cfg = M.tiny_config(False)
    model = M.LlavaOnevisionModel(cfg, dev, seed=5, cpu_rng=True)
    prompts = []
    for i, L in enumerate(LENS):
        b = data.synthetic_batch(1, dev, L=L, seed=9 + 2 * i, pixel_dtype=torch.bfloat16, cpu_rng=True)
        prompts.append((b["depth_input_ids"], b["depth_pixel_values"], b["image_sizes"]))
    free, free_logs = gen.generate_batch(model, prompts, max_new_tokens=1, return_logits=True, **KW)
    first = [int(o[0, -1]) for o in free]
    ids = _draw_ids(3, first)
    outs, logs = gen.generate_batch(model, prompts, max_new_tokens=8, return_logits=True, allowed_token_ids=ids, **KW)
    return SimpleNamespace(cfg=cfg, model=model, prompts=prompts, gen=gen, first=first, first_full=[l[0] for l in free_logs],
                           ids=ids, outs=outs, logs=logs, orc=OracleLlava(tiny_weights(False, 5), cfg), M=M, data=data)


@pytest.mark.gpu
def test_gpu_generate_batch_allowed_is_one_result_on_every_route(tiny, dev):
    gen, model, prompts, ids = tiny.gen, tiny.model, tiny.prompts, tiny.ids
    assert 250 < len(ids) <= 300 and not set(tiny.first) & set(ids)      # the mask cannot be vacuous
    for r, L in enumerate(LENS):
        new = tiny.outs[r][0, L:].tolist()
        assert len(new) == 8 and set(new) <= set(ids) and new[0] != tiny.first[r]
    base = (tiny.outs, tiny.logs)
    run = lambda p, **kw: gen.generate_batch(model, p, max_new_tokens=8, return_logits=True, **{**KW, **kw})
    assert _same(run(prompts, allowed_token_ids=ids, graph=False), base)                    # graph replay == eager
    assert _same(run(prompts, allowed_token_ids=ids, restrict_head=False), base)            # gathered head == full head
    assert _same(run(prompts, allowed_token_ids=ids, restrict_head=True), base)
    assert _same(run(prompts, allowed_token_ids=ids, restrict_head=False, graph=False), base)
    assert _same(run(prompts, allowed_token_ids=torch.tensor(ids[::-1] + ids[:5], device=dev)), base)   # any order, a tensor
    for k in (0, 1, 3):
        assert _same(run(prompts, allowed_token_ids=ids, stop_check_every=k), base), k
    for r in (1, 2):   # a row alone == the same row in the batch
        o, lg = run([prompts[r]], allowed_token_ids=ids)
        assert _same((o[0], lg[0]), (tiny.outs[r], tiny.logs[r])), r


@pytest.mark.gpu
def test_gpu_generate_batch_allowed_matches_oracle_teacher_forced(tiny, dev):
    for r in range(len(LENS)):
        ids_r, px, sizes = tiny.prompts[r]
        _check_row(tiny.orc, tiny.ids, ids_r, px, sizes, tiny.outs[r], tiny.logs[r], 8, tiny.first_full[r])
        # compact logits: the full row's elements at the allowed ids, bit for bit (first step: the same prefill)
        assert torch.equal(tiny.logs[r][0], tiny.first_full[r][:, torch.tensor(tiny.ids, device=dev)])


@pytest.mark.gpu
def test_gpu_generate_allowed(tiny, dev):
    """generate(): the same checks on one prompt."""
    gen, model = tiny.gen, tiny.model
    p_ids, px, sizes = tiny.prompts[1]
    free, free_lg = gen.generate(model, p_ids, px, sizes, max_new_tokens=1, return_logits=True, **KW)
    ids = _draw_ids(4, [int(free[0, -1])])
    assert int(free[0, -1]) not in ids
    run = lambda **kw: gen.generate(model, p_ids, px, sizes, max_new_tokens=8, return_logits=True,
                                    allowed_token_ids=ids, **{**KW, **kw})
    base = run()
    assert _same(run(graph=False), base)
    assert _same(run(restrict_head=False), base)
    assert _same(run(restrict_head=False, graph=False), base)
    for k in (0, 1, 3):
        assert _same(run(stop_check_every=k), base), k
    _check_row(tiny.orc, ids, p_ids, px, sizes, base[0], base[1], 8, free_lg[0])
    assert torch.equal(base[1][0], free_lg[0][:, torch.tensor(ids, device=dev)])


P0 = 24 + 1485            # template head + the image tokens of a 336x336 prompt
SUFFIX = ((5, 27), (18,))  # test_generate_grouped's run_g: group A has two questions, group B one


@pytest.mark.gpu
def test_gpu_generate_grouped_allowed(tiny, dev):
    gen, model, M, data = tiny.gen, tiny.model, tiny.M, tiny.data
    groups = []
    for gi, (seed, sufs) in enumerate(zip((9, 11), SUFFIX)):
        b = data.synthetic_batch(1, dev, L=P0 + max(sufs), seed=seed, pixel_dtype=torch.bfloat16, cpu_rng=True)
        p_ids = b["depth_input_ids"]
        assert int(p_ids[0, P0 - 1]) == M.IMAGE_TOKEN_ID and int(p_ids[0, P0]) != M.IMAGE_TOKEN_ID
        qs = []
        for qi, S in enumerate(sufs):
            g = torch.Generator().manual_seed(1000 + 10 * gi + qi)
            suf = torch.randint(0, data.TEXT_VOCAB, (1, S), generator=g, dtype=torch.int64).to(dev)
            qs.append(torch.cat([p_ids[:, :P0], suf], 1))
        groups.append((b["depth_pixel_values"], b["image_sizes"], qs))
    flat = [(gi, qi) for gi, (_, _, qs) in enumerate(groups) for qi in range(len(qs))]
    free, free_lg = gen.generate_grouped(model, groups, max_new_tokens=1, return_logits=True, **KW)
    first = [int(free[gi][qi][0, -1]) for gi, qi in flat]
    ids = _draw_ids(5, first)
    assert not set(first) & set(ids)
    run = lambda gr, **kw: gen.generate_grouped(model, gr, max_new_tokens=8, return_logits=True,
                                                allowed_token_ids=ids, **{**KW, **kw})
    base = run(groups)
    assert [len(o) for o in base[0]] == [2, 1] and [len(l) for l in base[1]] == [2, 1]
    assert _same(run(groups, graph=False), base)
    assert _same(run(groups, restrict_head=False), base)
    assert _same(run(groups, restrict_head=False, graph=False), base)
    for k in (0, 1, 3):
        assert _same(run(groups, stop_check_every=k), base), k
    px, sizes, qs = groups[0]
    o, lg = run([(px, sizes, [qs[1]])])   # a question alone == the same question inside its group
    assert _same((o[0][0], lg[0][0]), (base[0][0][1], base[1][0][1]))
    cols = torch.tensor(ids, device=dev)
    for gi, qi in flat:
        px, sizes, qs = groups[gi]
        _check_row(tiny.orc, ids, qs[qi], px, sizes, base[0][gi][qi], base[1][gi][qi], 8, free_lg[gi][qi][0])
        assert torch.equal(base[1][gi][qi][0], free_lg[gi][qi][0][:, cols])   # the gathered head behind the extend pass


@pytest.mark.gpu
def test_gpu_two_allowed_ids_run_out_of_bigrams_and_give_token_0(tiny, dev):
    """Two ids have four bigrams: with no_repeat_ngram_size = 2 at most five tokens can come from the
    set, then both are banned and the choice is token 0 (not allowed), as argmax of an all -inf row."""
    ids = [1234, 77777]
    outs, logs = tiny.gen.generate_batch(tiny.model, tiny.prompts, max_new_tokens=8, return_logits=True,
                                         allowed_token_ids=ids, **KW)
    one, one_lg = tiny.gen.generate(tiny.model, *tiny.prompts[0], max_new_tokens=8, return_logits=True,
                                    allowed_token_ids=ids, **KW)
    for L, out, lgs in [(LENS[r], outs[r], logs[r]) for r in range(3)] + [(LENS[0], one, one_lg)]:
        seq = out[0].cpu().tolist()
        assert len(seq) == L + 8 and set(seq[L:]) <= {0, 1234, 77777}
        assert 0 in seq[L:] and seq[L] != 0
        for t, lg in enumerate(lgs):
            assert lg.shape == (1, 2)
            assert seq[L + t] == _choose_compact(lg.float().cpu()[0].numpy(), ids, seq[:L + t], 1.2, 2), t


@pytest.mark.gpu
def test_gpu_allowed_eos_ends_a_row_only_when_it_is_chosen(tiny, dev):
    gen, model, prompts, ids = tiny.gen, tiny.model, tiny.prompts, tiny.ids
    full = [o[0].cpu().tolist() for o in tiny.outs]
    eos = full[1][LENS[1] + 2]   # an allowed id: the token row 1 produced third
    assert eos in ids
    kw = dict(max_new_tokens=8, repetition_penalty=1.2, no_repeat_ngram_size=2, allowed_token_ids=ids)
    for k in (0, 1, 3):
        cut = gen.generate_batch(model, prompts, eos_token_id=(eos,), stop_check_every=k, **kw)
        for r, L in enumerate(LENS):
            new = full[r][L:]
            want = full[r][:L + new.index(eos) + 1] if eos in new else full[r]
            assert cut[r][0].cpu().tolist() == want, (k, r)
        assert cut[1].shape[1] <= LENS[1] + 3 and int(cut[1][0, -1]) == eos
    for call in (lambda **kw2: gen.generate_batch(model, [prompts[1]], **kw, **kw2)[0],
                 lambda **kw2: gen.generate(model, *prompts[1], **kw, **kw2)):
        # the default EOS id is not allowed, so it is never chosen: the row runs max_new_tokens
        stats = {}
        whole = call(stats=stats)
        assert EOS_DEFAULT not in ids and whole.shape[1] == LENS[1] + 8
        assert stats["steps_run"][0] == stats["steps_max"][0] == 7
        eos = int(whole[0, LENS[1] + 2])
        stats = {}
        cut1 = call(eos_token_id=(eos,), stats=stats)
        assert eos in ids and int(cut1[0, -1]) == eos and cut1.shape[1] <= LENS[1] + 3
        assert torch.equal(cut1, whole[:, :cut1.shape[1]])
        assert stats["steps_run"][0] < stats["steps_max"][0] == 7
