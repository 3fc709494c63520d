"""The bits of the decode path, to compare two builds (a refactor must not change one of them).
    python tools/decode_bits.py dump OUT.npz [--tree DIR]   one call per shape of every decode op (gemv, gemv_batch,
                                                 gemv_rows, attn_decode, attn_decode_batch, attn_extend, gen_select,
                                                 gen_select_batch, gemv_gather, gemv_batch_gather, gen_select_ids,
                                                 gen_sample over the full row and over allowed ids, rope_row,
                                                 rope_rows, gen_finish) on seeded inputs, at
                                                 the shapes of tests/test_generate*.py and tests/test_decode_edges.py,
                                                 then generate / generate_batch / generate_grouped on the tests' tiny
                                                 student (graph on and off, stop_check_every 0 and 1, no EOS id, the
                                                 rows' third new tokens as EOS ids, nine ids: the host scan; then
                                                 with allowed_token_ids on the default head and restrict_head=False,
                                                 do_sample with and without allowed_token_ids, each without an EOS id
                                                 and with an active stop; generate(fuse_norm=False)); every
                                                 output tensor goes into OUT.npz as raw bytes.  KDSTEP_LIB selects the
                                                 library, --tree the checkout the Python package is imported from
    python tools/decode_bits.py compare A.npz B.npz   same keys, every array byte-identical: prints the first key that
                                                 differs and exits 1, else a summary (keys, bytes) and exits 0
One dump per process: two libraries cannot be loaded side by side."""
import argparse
import sys
from pathlib import Path

import numpy as np

PKG = "knowledge_distillation_for_sensory_substitution_in_multimodal_models_amd"
GEMV_SHAPES = [(1152, 896, "bias"), (896, 4864, "residual"), (4864, 896, "swiglu"), (151936, 896, "none"),
               (21, 40, "none"), (32776, 64, "residual"), (32776, 64, "bias")]
NBS, ROWS = (1, 3, 16), (1, 17, 40, 81)
HEADS = [(64, 14, 2), (128, 28, 4)]                                       # hd, H, HKV
QUESTIONS = [(1, 1), (63, 2), (64, 17), (60, 10), (200, 40), (65, 1)]   # (base, S) of kd_attn_extend
SMAX = 320
VS = (8197, 151936)
KW = dict(repetition_penalty=1.2, no_repeat_ngram_size=2)
AS = (1, 17, 700)                                                         # allowed ids of the gathered head
SETTINGS = [(0.7, 50, 1.0), (0.7, 64, 0.9), (1.0, 0, 0.9), (1.5, 1000, 1.0), (1.0, 0, 1.0)]   # tests/test_generate_sample.py
SEED = 0x5EED5EED5EED
ALLOWED = sorted(set(range(0, 600, 2)) | {151646, 7, 151935})
SKW = dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.9, seed=SEED)
MODES = (("allowed", dict(allowed_token_ids=ALLOWED)),
         ("allowed_full_head", dict(allowed_token_ids=ALLOWED, restrict_head=False)),
         ("sampled", SKW), ("sampled_allowed", dict(allowed_token_ids=ALLOWED, **SKW)))


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    ka, kb = sorted(a.files), sorted(b.files)
    if ka != kb:
        print(f"DIFFERENT keys: only in {a_path}: {sorted(set(ka) - set(kb))[:5]}, only in {b_path}: "
              f"{sorted(set(kb) - set(ka))[:5]}")
        return 1
    nbytes = 0
    for k in ka:
        if a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes():
            print(f"DIFFERENT at key {k!r} ({a[k].size} vs {b[k].size} bytes)")
            return 1
        nbytes += a[k].size
    print(f"{a_path} == {b_path}: {len(ka)} keys, {nbytes} bytes compared, no difference")
    return 0


def dump(out_path, tree):
    sys.path.insert(0, str(Path(tree).resolve() if tree else Path(__file__).resolve().parent.parent))
    from importlib import import_module
    import torch
    ops = import_module(f"{PKG}.ops")
    gen = import_module(f"{PKG}.generation")
    M = import_module(f"{PKG}.modeling")
    data = import_module(f"{PKG}.data")
    dev = torch.device("cuda:0")
    BF = torch.bfloat16
    out = {}

    def keep(key, *tensors):
        for i, t in enumerate(tensors):
            assert key + f"/{i}" not in out, key
            out[key + f"/{i}"] = np.frombuffer(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes(), np.uint8)

    def rand(g, *shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(BF).to(dev)

    # ---- the linears: every epilogue, plain and with the fused RMSNorm, strided weight rows
    for N, K, epi in GEMV_SHAPES:
        g = torch.Generator().manual_seed(N + K)
        w = rand(g, 2 * N if epi == "swiglu" else N, K + 8, scale=0.05)[:, :K]
        x, e = rand(g, max(ROWS), K), rand(g, max(ROWS), N)
        nw = (1 + 0.1 * torch.randn(K, generator=g)).to(BF).to(dev)

        def run(fn, r, **kw):
            xs = x[:r].contiguous()
            if epi == "swiglu":
                return fn(xs, w, swiglu_inter=N, **kw)
            if epi == "bias":
                return fn(xs, w, bias=e[0].contiguous(), **kw)
            if epi == "residual":
                return fn(xs, w, residual=e[:r].contiguous(), **kw)
            return fn(xs, w, **kw)

        for name, kw in (("plain", {}), ("norm", dict(norm_w=nw, eps=1e-6))):
            keep(f"gemv/{N}x{K}/{epi}/{name}", run(ops.gemv, 1, **kw))
            for nb in NBS:
                keep(f"gemv_batch/{N}x{K}/{epi}/{name}/nb{nb}", run(ops.gemv_batch, nb, **kw))
            for rows in ROWS:
                keep(f"gemv_rows/{N}x{K}/{epi}/{name}/rows{rows}", run(ops.gemv_rows, rows, **kw))

    # ---- attention: one token per row (host length, device counter, batched), then the ragged extend
    lens = [1, 63, 64, 65, 200, SMAX]
    for hd, H, HKV in HEADS:
        g = torch.Generator().manual_seed(hd + H)
        nb = len(lens)
        q, kn, vn = rand(g, H, nb, hd), rand(g, HKV, nb, hd), rand(g, HKV, nb, hd)
        kc, vc = rand(g, nb, HKV, SMAX, hd), rand(g, nb, HKV, SMAX, hd)
        for b, n in enumerate(lens):
            for cur in (None, torch.tensor([n], dtype=torch.int32, device=dev)):
                k1, v1 = kc[b].clone(), vc[b].clone()
                o = ops.attn_decode(q[:, b].contiguous(), kn[:, b].contiguous(), vn[:, b].contiguous(), k1, v1,
                                    n if cur is None else 0, hd, cur=cur)
                keep(f"attn_decode/hd{hd}/n{n}/{'host' if cur is None else 'dev'}", o, k1, v1)
        k1, v1 = kc.clone(), vc.clone()
        o = ops.attn_decode_batch(q, kn, vn, k1, v1, torch.tensor(lens, dtype=torch.int32, device=dev), hd)
        keep(f"attn_decode_batch/hd{hd}", o, k1, v1)
        starts = [0]
        for _, S in QUESTIONS:
            starts.append(starts[-1] + S)
        rows, nq = starts[-1], len(QUESTIONS)
        q, kn, vn = rand(g, H, rows, hd), rand(g, HKV, rows, hd), rand(g, HKV, rows, hd)
        k1, v1 = rand(g, nq, HKV, SMAX, hd), rand(g, nq, HKV, SMAX, hd)
        o = ops.attn_extend(q, kn, vn, k1, v1, torch.tensor(starts, dtype=torch.int32, device=dev),
                            torch.tensor([b for b, _ in QUESTIONS], dtype=torch.int32, device=dev), hd)
        keep(f"attn_extend/hd{hd}", o, k1, v1)

    # ---- the token choice: both forms of the single kernel, aligned and not; ragged batches
    for V in VS:
        g = torch.Generator().manual_seed(V)
        lg = rand(g, 3, V + 1, scale=3.0)
        seqs = [torch.randint(0, V, (n,), generator=g).tolist() for n in (3, 40, 1100)]
        for b, sq in enumerate(seqs):
            sq[-1] = sq[len(sq) // 2]   # the last id occurred before: its follower is banned
            for off in (0, 1):
                for form in ("len", "cur"):
                    s = torch.tensor(sq + [-1], dtype=torch.int64, device=dev)
                    o = torch.full((1,), -1, dtype=torch.int64, device=dev)
                    cur = torch.tensor([len(sq)], dtype=torch.int32, device=dev) if form == "cur" else None
                    ops.gen_select(lg[b, off:off + V][None], s, 0 if cur is not None else len(sq), 1.2, 2, out=o, cur=cur)
                    keep(f"gen_select/V{V}/row{b}/off{off}/{form}", s, o, *([cur] if cur is not None else []))
        for pad in (0, 1):
            s = torch.full((3, 1200), -1, dtype=torch.int64)
            for b, sq in enumerate(seqs):
                s[b, :len(sq)] = torch.tensor(sq)
            s, o = s.to(dev), torch.full((3,), -1, dtype=torch.int64, device=dev)
            cur = torch.tensor([len(sq) for sq in seqs], dtype=torch.int32, device=dev)
            ops.gen_select_batch(lg[:, :V] if pad else lg[:, :V].contiguous(), s, cur, 1.2, 2, out=o)   # ldl = V + pad
            keep(f"gen_select_batch/V{V}/pad{pad}", s, o, cur)

    # ---- constrained decoding: the gathered lm_head (the real head shape: gemv_gather_supported needs it), the
    # select among the allowed ids, and the draw over the full row and over the allowed ids
    V, K = 151936, 896
    g = torch.Generator().manual_seed(V + K)
    w, x = rand(g, V, K + 8, scale=0.05)[:, :K], rand(g, max(NBS), K)
    id_sets = {}
    for A in AS:
        pick = torch.randperm(V, generator=g)[:A].tolist() if A > 1 else [V - 1]
        if A >= 17:
            pick = ([0, 15, 16, 31, 32, 4095, 4096, V - 17, V - 16, V - 1] + pick)[:A]   # both sides of 16-row tile boundaries
        id_sets[A] = torch.tensor(sorted(set(pick)), dtype=torch.int32, device=dev)
        keep(f"gemv_gather/A{A}", ops.gemv_gather(x[:1].contiguous(), w, id_sets[A]))
        for nb in NBS:
            keep(f"gemv_batch_gather/A{A}/nb{nb}", ops.gemv_batch_gather(x[:nb].contiguous(), w, id_sets[A]))
    del w

    def rows_for(g, nb, N, ids):
        """nb ragged sequences whose tokens hit the row (or the allowed ids), each ending on a repeated bigram head."""
        lens = [3 + (37 * b) % 200 for b in range(nb)]
        seq = torch.full((nb, max(lens) + 3), -1, dtype=torch.int64)
        for b, n in enumerate(lens):
            sq = torch.randint(0, N, (n,), generator=g)
            sq = sq if ids is None else ids.cpu().long()[sq]
            sq[-1] = sq[n // 2]
            seq[b, :n] = sq
        return seq.to(dev), torch.tensor(lens, dtype=torch.int32, device=dev)

    ids = id_sets[700]
    for nb in NBS:
        g = torch.Generator().manual_seed(700 + nb)
        sc = rand(g, nb, 700 + 1, scale=3.0)[:, :700]   # ld = A + 1
        for name, (penalty, ngram) in (("on", (1.2, 2)), ("off", (1.0, 0))):
            s, cur = rows_for(g, nb, 700, ids)
            o = torch.full((nb,), -1, dtype=torch.int64, device=dev)
            ops.gen_select_ids(sc, ids, s, cur, penalty, ngram, out=o)
            keep(f"gen_select_ids/nb{nb}/{name}", s, o, cur)
    for N, sample_ids in [(N, None) for N in VS] + [(700, ids)]:
        g = torch.Generator().manual_seed(N + 1)
        sc = rand(g, 3, N, scale=4.0)
        for case, (temperature, top_k, top_p) in enumerate(SETTINGS):
            s, cur = rows_for(g, 3, N, sample_ids)
            o = torch.full((3,), -1, dtype=torch.int64, device=dev)
            u = torch.full((3,), -1.0, dtype=torch.float32, device=dev)
            ops.gen_sample(sc, s, cur, ids=sample_ids, **KW, temperature=temperature, top_k=top_k, top_p=top_p,
                           seed=SEED + case, streams=torch.tensor([0, 2 ** 32 + 5, 2 ** 63 - 1], device=dev), out=o, u_out=u)
            keep(f"gen_sample/N{N}/{'ids' if sample_ids is not None else 'full'}/case{case}", o, u, s, cur)

    # ---- RoPE rows and the EOS latch
    g = torch.Generator().manual_seed(5)
    cos, sin = torch.randn(50, 288, generator=g).to(dev), torch.randn(50, 288, generator=g).to(dev)
    for pos in (1, 2, 50):
        cr, sr = torch.zeros(1, 288, device=dev), torch.zeros(1, 288, device=dev)
        ops.rope_row(cos, sin, torch.tensor([pos], dtype=torch.int32, device=dev), cr, sr)
        keep(f"rope_row/pos{pos}", cr, sr)
    for nb in (1, 16, 40):
        cs = [(7 * b + 1) % 50 + 1 for b in range(nb)]
        cs[0], cs[-1] = (0, 53) if nb > 1 else (53, 53)
        cr, sr = torch.zeros(nb, 288, device=dev), torch.zeros(nb, 288, device=dev)
        ops.rope_rows(cos, sin, torch.tensor(cs, dtype=torch.int32, device=dev), cr, sr)
        keep(f"rope_rows/nb{nb}", cr, sr)
    for nb in (1, 3, 16):
        fin = torch.zeros(nb, dtype=torch.int32, device=dev)
        live = torch.zeros(1, dtype=torch.int32, device=dev)
        for c in range(3):
            tok = torch.tensor([(5 if (b + c) % 3 == 0 else 1000 + b) for b in range(nb)], dtype=torch.int64, device=dev)
            cur = torch.tensor([100 * (c + 1) + b for b in range(nb)], dtype=torch.int32, device=dev)
            ops.gen_finish(tok, cur, [5, 9], fin, live)
            keep(f"gen_finish/nb{nb}/call{c}", fin, live)

    # ---- the three entry points on the tests' tiny student
    model = M.LlavaOnevisionModel(M.tiny_config(False), dev, seed=5, cpu_rng=True)

    def prompt(L, seed):
        b = data.synthetic_batch(1, dev, L=L, seed=seed, pixel_dtype=BF, cpu_rng=True)
        return b["depth_input_ids"], b["depth_pixel_values"], b["image_sizes"]

    one = prompt(1536, 9)
    three = [prompt(L, 9 + 2 * i) for i, L in enumerate((1490, 1536, 1511))]
    P0, groups = 24 + 1485, []
    for gi, (seed, sufs) in enumerate(zip((9, 11), ((5, 27), (18,)))):
        ids, px, sizes = prompt(P0 + max(sufs), seed)
        qs = []
        for qi, S in enumerate(sufs):
            gq = torch.Generator().manual_seed(1000 + 10 * gi + qi)
            qs.append(torch.cat([ids[:, :P0], torch.randint(0, data.TEXT_VOCAB, (1, S), generator=gq).to(dev)], 1))
        groups.append((px, sizes, qs))
    entries = (("generate", lambda **k: [gen.generate(model, *one, max_new_tokens=8, **KW, **k)], [1536]),
               ("generate_batch", lambda **k: [gen.generate_batch(model, three, max_new_tokens=8, **KW, **k)],
                [1490, 1536, 1511]),
               ("generate_grouped", lambda **k: [gen.generate_grouped(model, groups, max_new_tokens=8, **KW, **k)],
                [P0 + 5, P0 + 27, P0 + 18]))

    def flat(x):   # any nesting of lists of tensors -> the tensors in order
        return [x] if isinstance(x, torch.Tensor) else [t for y in x for t in flat(y)]

    for name, call, Ls in entries:
        full = flat(call(eos_token_id=(), return_logits=False))
        third = sorted({int(o[0, L + 2]) for o, L in zip(full, Ls)})   # as tests/test_generate_stop.py's "third" sets
        nine = third + [t for t in range(151000, 151020) if t not in third][:9 - len(third)]
        for eos_name, eos in (("none", ()), ("third", tuple(third)), ("nine", tuple(nine))):
            for graph in (True, False):
                for k in (0, 1):
                    stats = {}
                    r = call(eos_token_id=eos, return_logits=True, graph=graph, stop_check_every=k, stats=stats)
                    keep(f"{name}/eos_{eos_name}/graph{int(graph)}/k{k}", *flat(r),
                         torch.tensor([x for f in stats["finished_at"] for x in f], dtype=torch.int64))
        for mode, kw in MODES:   # constrained and sampled calls, no EOS id and the rows' third new tokens of that mode
            plain = flat(call(eos_token_id=(), return_logits=False, **kw))
            mine = sorted({int(o[0, L + 2]) for o, L in zip(plain, Ls)})
            for eos_name, eos in (("none", ()), ("third", tuple(mine))):
                for graph in (True, False):
                    for k in (0, 1):
                        stats = {}
                        r = call(eos_token_id=eos, return_logits=True, graph=graph, stop_check_every=k, stats=stats,
                                 **kw)
                        keep(f"{name}/{mode}/eos_{eos_name}/graph{int(graph)}/k{k}", *flat(r),
                             torch.tensor([x for f in stats["finished_at"] for x in f], dtype=torch.int64))
        if name == "generate":   # the RMSNorm as its own launch: the A/B route of generate() alone
            keep("generate/fuse_norm0", *flat(call(eos_token_id=(), return_logits=True, fuse_norm=False)))
    torch.cuda.synchronize()
    np.savez(out_path, **out)
    print(f"{out_path}: {len(out)} arrays, {sum(v.size for v in out.values())} bytes")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="mode", required=True)
    d = sub.add_parser("dump")
    d.add_argument("out")
    d.add_argument("--tree", default=None, metavar="DIR", help="import the package from this checkout instead")
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    args = ap.parse_args()
    sys.exit(dump(args.out, args.tree) if args.mode == "dump" else compare(args.a, args.b))
