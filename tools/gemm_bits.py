"""The bits of every route of the GEMM launcher (csrc/gemm.hip launch_gemm / launch_gemm_f8 /
launch_gemm_group), to compare two builds (a launcher refactor must not change one of them).
    python tools/gemm_bits.py dump OUT.npz [--tree DIR]   one seeded call per route at the smallest shapes that reach it:
                                                 v1 in four layouts; the tiled kernels (variants 2, 3, 4, 16 forced) in four
                                                 layouts and with every epilogue; forced split-K on a v3 tile and on v8; the
                                                 in-launch fold (32); a hybrid plan; stream-K (21) plain and SwiGLU; SwiGLU
                                                 plain and pre-tiled; b_pretiled; row_stats; the q|k|v scatter; the backward
                                                 activations; fp8; grouped launches of 1, 2 and 4 members.  Every output
                                                 goes into OUT.npz as raw bytes.  KDSTEP_LIB selects the library, --tree the
                                                 checkout the Python package is imported from
    python tools/gemm_bits.py compare A.npz B.npz   tools/decode_bits.py's compare: the first differing key and exit 1,
                                                 else a one-line summary and exit 0
One dump per process: two libraries cannot be loaded side by side."""
import argparse
import ctypes as C
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from decode_bits import PKG, compare   # noqa: E402

LAYOUTS = ("kk", "kn", "nk", "nn")
HYBRID = (1792, 9472, 1024)     # the smallest whole-tile shape whose plan has dp_tiles > 0 (kd_gemm_plan, on the CPU)
GROUP_SYMBOL = "_ZN2kd17launch_gemm_groupEPKPK12kd_gemm_desciPv"


def dump(out_path, tree):
    sys.path.insert(0, str(Path(tree).resolve() if tree else Path(__file__).resolve().parent.parent))
    from importlib import import_module
    import torch
    ops = import_module(f"{PKG}.ops")
    NV = import_module(f"{PKG}._native")
    dev = torch.device("cuda:0")
    BF, F32 = torch.bfloat16, torch.float32
    out = {}

    def keep(key, *tensors):
        for i, t in enumerate(tensors):
            assert key + f"/{i}" not in out, key
            out[key + f"/{i}"] = np.frombuffer(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes(), np.uint8)

    def rand(seed, *shape, scale=1.0, dtype=BF):
        g = torch.Generator().manual_seed(seed)
        return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev)

    def operands(M, N, K, lay, seed):
        """a [M, K], b [N, K] as K-contiguous tensors or transposed views of [K, rows] ones."""
        a = rand(seed, M, K) if lay[0] == "k" else rand(seed, K, M).t()
        b = rand(seed + 1, N, K, scale=0.05) if lay[1] == "k" else rand(seed + 1, K, N, scale=0.05).t()
        return a, b

    # ---- v1 and the tiled kernels, every layout (M % 8 == 0 where A is MN-major, N % 8 where B is)
    for M, N, K in ((7, 13, 8), (129, 130, 72)):
        for lay in LAYOUTS:
            Ml, Nl = (M + 7) // 8 * 8 if lay[0] == "n" else M, (N + 7) // 8 * 8 if lay[1] == "n" else N
            a, b = operands(Ml, Nl, K, lay, 10)
            keep(f"v1/{M}x{N}x{K}/{lay}", ops.gemm(a, b), ops.gemm(a, b, out_dtype=F32, variant=1))
    for M, N, K in ((1024, 1024, 264), (1032, 1096, 264)):
        bias, bias32 = rand(20, N), rand(21, N, dtype=F32)
        res, res32, half = rand(22, M, N), rand(23, M, N, dtype=F32), rand(24, M // 2, N)
        s = torch.tensor([0.75], device=dev)
        for variant in (2, 3, 4, 16):
            for lay in LAYOUTS:
                a, b = operands(M, N, K, lay, 30)
                acc = rand(25, M, N, dtype=F32)
                ops.gemm(a, b, out=acc, accumulate=True, variant=variant, split_k=1)
                keep(f"tiled/{M}x{N}x{K}/v{variant}/{lay}", ops.gemm(a, b, variant=variant, split_k=1), acc)
            a, b = operands(M, N, K, "kk", 30)
            aux = torch.empty(M, N, dtype=BF, device=dev)
            o = ops.gemm(a, b, bias=bias, act="gelu_tanh", residual=half, residual_row_mod=M // 2, aux=aux, alpha=1.5,
                         alpha_dev=s, variant=variant, split_k=1)
            keep(f"tiled/{M}x{N}x{K}/v{variant}/epilogue", o, aux)
            o = rand(26, M, N)
            ops.gemm(a, b, out=o, bias=bias32, residual=res, accumulate=True, variant=variant, split_k=1)
            keep(f"tiled/{M}x{N}x{K}/v{variant}/bias32_res_acc", o)
            keep(f"tiled/{M}x{N}x{K}/v{variant}/res32",
                 ops.gemm(a, b, bias=bias, residual=res32, out_dtype=F32, variant=variant, split_k=1))
            for act in ("gelu_erf", "silu"):
                keep(f"tiled/{M}x{N}x{K}/v{variant}/{act}", ops.gemm(a, b, bias=bias, act=act, variant=variant, split_k=1))

    # ---- split-K: forced on a v3 tile and on v8, the in-launch fold, a hybrid plan, stream-K
    M, N, K = 1024, 1024, 2304
    bias = rand(40, N)
    for variant in (3, 16):
        for lay in LAYOUTS:
            a, b = operands(M, N, K, lay, 41)
            acc = rand(42, M, N, dtype=F32)
            ops.gemm(a, b, out=acc, accumulate=True, variant=variant, split_k=3)
            keep(f"split3/v{variant}/{lay}", ops.gemm(a, b, bias=bias, act="gelu_tanh" if lay == "kk" else None,
                                                      variant=variant, split_k=3), acc)
    for M, N, K, split in ((896, 896, 6144, 8), (1152, 4304, 5832, 3), (6144, 3584, 3584, 0)):
        a, b = operands(M, N, K, "nn", 43)
        got = torch.ones(M, N, dtype=F32, device=dev)
        ops.gemm(a, b, out=got, accumulate=True, variant=32, split_k=split)
        keep(f"fold/{M}x{N}x{K}/s{split}", got)
    M, N, K = HYBRID
    a, b = operands(M, N, K, "kk", 44)
    plan = ops.gemm_plan(a, b)
    assert plan[1] > 1 and plan[2] > 0, plan
    keep("hybrid", ops.gemm(a, b, bias=rand(45, N), act="gelu_tanh"), torch.tensor(plan))
    M, N, K = 1024, 1024, 1024   # 16 tiles x 32 k-steps: the least work stream-K's 256 runs take
    for lay in LAYOUTS:
        a, b = operands(M, N, K, lay, 46)
        assert ops.gemm_plan(a, b, variant=21)[0] == 21
        keep(f"stream_k/{lay}", ops.gemm(a, b, bias=rand(47, N), variant=21))
    h, w = operands(M, N, K, "kk", 48)
    aux = torch.empty(M, N, dtype=BF, device=dev)
    keep("stream_k/swiglu", ops.gemm(h, w, act="swiglu", aux=aux, variant=21), aux)

    # ---- the v8-only routes: SwiGLU plain and pre-tiled, b_pretiled, row statistics
    for M, I, K in ((300, 256, 96), (512, 384, 600)):
        h, w = rand(50, M, K), rand(51, 2 * I, K, scale=0.05)
        aux, aux_t = torch.empty(M, 2 * I, dtype=BF, device=dev), torch.empty(M, 2 * I, dtype=BF, device=dev)
        keep(f"swiglu/{M}x{I}x{K}", ops.gemm(h, w, act="swiglu", aux=aux), aux, ops.gemm(h, w, act="swiglu", alpha=0.5),
             ops.gemm(h, w, act="swiglu", aux=aux_t, b_pretiled=ops.pretile_b(w, glu=True)), aux_t)
    for M, N, K in ((1024, 1024, 264), (1032, 1096, 264)):
        a, b = operands(M, N, K, "kk", 52)
        bt = ops.pretile_b(b)
        keep(f"pretiled/{M}x{N}x{K}", bt, ops.gemm(a, b, bias=rand(53, N), act="silu", residual=rand(54, M, N), b_pretiled=bt))
        for top2 in (False, True):
            st = torch.zeros(M, (N + 255) // 256, 8, dtype=F32, device=dev)
            keep(f"row_stats/{M}x{N}x{K}/top2_{int(top2)}",
                 ops.gemm(a, b, row_stats=st, row_stats_vs=N - 8, row_stats_inv_t=1.25, row_stats_top2=top2), st)

    # ---- the fused epilogues that are never split: the q|k|v scatter, the backward activations
    for name, (B, S, K, nq, nkv, hd, hdp, rope) in (("rope", (2, 512, 264, 8, 4, 64, 64, True)),
                                                    ("plain", (2, 729, 264, 4, 4, 72, 96, False))):
        Mq, Nq = B * S, (nq + 2 * nkv) * hd
        x, w, bias = rand(60, Mq, K), rand(61, Nq, K, scale=0.05), rand(62, Nq)
        cos = sin = None
        if rope:
            f = torch.arange(S, dtype=F32)[:, None] / (1e6 ** (torch.arange(0, hd, 2, dtype=F32) / hd))[None]
            cos, sin = f.cos().to(dev).contiguous(), f.sin().to(dev).contiguous()
        for variant in (0, 5, 16):
            q, k, v = (torch.full((B, n, S, hdp), 7.0, dtype=BF, device=dev) for n in (nq, nkv, nkv))
            ops.gemm_qkv(x, w, bias, q, k, v, S, nq, nkv, hd, hdp, cos, sin, variant=variant)
            keep(f"qkv/{name}/v{variant}", q, k, v)
    M, N, K = 1100, 1040, 392
    dy, w = rand(63, M, K), rand(64, K, N, scale=K ** -0.5)
    for variant in (0, 6, 16):
        keep(f"dact/v{variant}", ops.gemm(dy, w.t(), act="dgelu_tanh", aux=rand(65, M, N), variant=variant),
             ops.gemm(dy, w.t(), act="dswiglu", aux=rand(66, M, 2 * N), variant=variant))

    # ---- fp8: the four activations and SwiGLU
    M, N, K = 520, 512, 272
    (qa, sa), (qb, sb) = ops.quant_rows_fp8(rand(70, M, K)), ops.quant_rows_fp8(rand(71, N, K, scale=0.05))
    for act in (None, "gelu_tanh", "gelu_erf", "silu"):
        keep(f"fp8/{act}", ops.gemm_fp8(qa, sa, qb, sb, bias=rand(72, N), act=act, residual=rand(73, M, N), alpha=1.5))
    aux = torch.empty(M, N, dtype=BF, device=dev)
    keep("fp8/swiglu", ops.gemm_fp8(qa, sa, qb, sb, act="swiglu", aux=aux), aux)

    # ---- grouped weight gradients: 1, 2 and 4 members of unequal size, fp32 +=
    group = getattr(NV.lib(), GROUP_SYMBOL)
    group.restype, group.argtypes = C.c_int, [C.POINTER(C.POINTER(NV.KdGemmDesc)), C.c_int, C.c_void_p]
    sizes = [(384, 640, 2304), (128, 136, 520), (1032, 256, 264), (896, 128, 4096)]
    for n in (1, 2, 4):
        descs, held = [], []
        for i, (M, N, K) in enumerate(sizes[:n]):
            a, b, c = rand(80 + i, K, M), rand(90 + i, K, N, scale=0.05), rand(100 + i, M, N, dtype=F32)
            d = NV.KdGemmDesc()
            d.M, d.N, d.K, d.a_layout, d.b_layout = M, N, K, NV.KD_LAYOUT_MN_MAJOR, NV.KD_LAYOUT_MN_MAJOR
            d.A, d.lda, d.B, d.ldb, d.C, d.ldc = a.data_ptr(), M, b.data_ptr(), N, c.data_ptr(), N
            d.c_dtype, d.accumulate, d.alpha = NV.KD_DTYPE_F32, 1, 0.5
            descs.append(d)
            held.append((a, b, c))
        arr = (C.POINTER(NV.KdGemmDesc) * n)(*[C.pointer(d) for d in descs])
        NV.check("launch_gemm_group", group(arr, n, ops._stream()))
        keep(f"group/n{n}", *[c for _, _, c in held])
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
