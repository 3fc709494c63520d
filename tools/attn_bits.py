"""The bits of every route of the attention launchers (csrc/attention.hip launch_attn_fwd /
launch_attn_bwd), to compare two builds (a launcher refactor must not change one of them).
    python tools/attn_bits.py dump OUT.npz [--tree DIR] [--ab]
            one seeded call per route at the smallest shape that reaches it.  Product routes: the forward at the
            three padded head dims x causal; the backward with split dq / dk / dv (MHA and GQA), with the fused
            MHA dqkv, and with the GQA dqkv with and without RoPE.  --ab (the A/B library, which reads
            KD_ATTN_FWD_V / KD_ATTN_BWD_V on every call): also every code of the two variant tables at one
            head-dim-64 and one head-dim-96 shape, except the DIAG builds (KD_ATTN_BWD_V=5..8: wrong results by
            design) and the stamp build (KD_ATTN_FWD_V=34: it overwrites Q).  Every output goes into OUT.npz as
            raw bytes, the head-dim padding cut off (nothing writes all of it).  KDSTEP_LIB selects the library,
            --tree the checkout the Python package is imported from
    python tools/attn_bits.py compare A.npz B.npz   tools/decode_bits.py's compare: the first differing key and exit 1,
                                                 else a one-line summary and exit 0
One dump per process: two libraries cannot be loaded side by side."""
import argparse
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from decode_bits import PKG, compare   # noqa: E402

# B, H, HKV, S, hd, hdp: two 64-key tiles and a second 128-row query block each, MHA and GQA
SHAPES = [(1, 2, 2, 129, 64, 64), (1, 4, 2, 129, 64, 64), (1, 2, 2, 129, 72, 96), (1, 4, 2, 129, 72, 96),
          (1, 2, 2, 129, 128, 128), (1, 4, 1, 129, 128, 128)]
AB_SHAPES = [(1, 4, 2, 193, 64, 64), (1, 2, 2, 193, 72, 96)]   # a second 192-row block of the six-wave build too
FWD_CODES = (0, 16, 32, 33, 35, 36, 64)     # 34: the stamp build
BWD_CODES = (0, 2, 3, 16, 32)               # 5..8: the DIAG builds


def dump(out_path, tree, ab):
    sys.path.insert(0, str(Path(tree).resolve() if tree else Path(__file__).resolve().parent.parent))
    from importlib import import_module
    import torch
    ops = import_module(f"{PKG}.ops")
    dev = torch.device("cuda:0")
    out = {}

    def keep(key, *tensors):
        for i, t in enumerate(tensors):
            assert key + f"/{i}" not in out, key
            out[key + f"/{i}"] = np.frombuffer(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes(), np.uint8)

    def inputs(B, H, HKV, S, hd, hdp, seed):
        g = torch.Generator().manual_seed(seed)
        pad = lambda t: torch.nn.functional.pad(t, (0, hdp - hd)).to(dev, torch.bfloat16).contiguous()
        q, k, v = (pad(torch.randn(B, n, S, hd, generator=g)) for n in (H, HKV, HKV))
        do = torch.randn(B, S, H, hd, generator=g).to(dev, torch.bfloat16)
        ang = torch.rand(S, hd // 2, generator=g) * 6.0
        return q, k, v, do, torch.cos(ang).to(dev).contiguous(), torch.sin(ang).to(dev).contiguous()

    def routes(key, shape, causal):
        """forward, split backward, fused dqkv (wider rows than needed) and, where the launcher takes them, RoPE tables"""
        B, H, HKV, S, hd, hdp = shape
        q, k, v, do, cos, sin = inputs(*shape, seed=11)
        o, lse = ops.attn_fwd(q, k, v, hd, causal)
        keep(f"{key}/fwd", o, lse, ops.attn_fwd(q, k, v, hd, causal, want_lse=False)[0])
        keep(f"{key}/bwd", *[t[..., :hd] for t in ops.attn_bwd(q, k, v, o, do, lse, hd, causal)])
        wide = torch.full((B * S, (H + 2 * HKV) * hd + 8), 7.0, dtype=torch.bfloat16, device=dev)
        keep(f"{key}/dqkv", ops.attn_bwd(q, k, v, o, do, lse, hd, causal, dqkv=wide))
        if H != HKV and hd == hdp:
            wide = torch.full((B * S, (H + 2 * HKV) * hd), 3.0, dtype=torch.bfloat16, device=dev)
            keep(f"{key}/dqkv_rope", ops.attn_bwd(q, k, v, o, do, lse, hd, causal, dqkv=wide, cos=cos, sin=sin))

    for shape in SHAPES:
        for causal in (False, True):
            routes("product/" + "x".join(map(str, shape)) + f"/c{int(causal)}", shape, causal)
    if ab:
        assert "KD_ATTN_FWD_V" not in os.environ and "KD_ATTN_BWD_V" not in os.environ
        try:
            for shape in AB_SHAPES:
                B, H, HKV, S, hd, hdp = shape
                for causal in (False, True):
                    key = "x".join(map(str, shape)) + f"/c{int(causal)}"
                    q, k, v, do, cos, sin = inputs(*shape, seed=12)
                    for code in FWD_CODES:
                        os.environ["KD_ATTN_FWD_V"] = str(code)
                        keep(f"ab/fwd{code}/{key}", *ops.attn_fwd(q, k, v, hd, causal))
                    os.environ.pop("KD_ATTN_FWD_V")
                    o, lse = ops.attn_fwd(q, k, v, hd, causal)
                    for code in BWD_CODES:
                        os.environ["KD_ATTN_BWD_V"] = str(code)
                        keep(f"ab/bwd{code}/{key}", *[t[..., :hd] for t in ops.attn_bwd(q, k, v, o, do, lse, hd, causal)])
                        if H != HKV and hd == hdp:
                            wide = torch.full((B * S, (H + 2 * HKV) * hd), 3.0, dtype=torch.bfloat16, device=dev)
                            keep(f"ab/bwd{code}/{key}/dqkv_rope",
                                 ops.attn_bwd(q, k, v, o, do, lse, hd, causal, dqkv=wide, cos=cos, sin=sin))
                    os.environ.pop("KD_ATTN_BWD_V")
        finally:
            os.environ.pop("KD_ATTN_FWD_V", None)
            os.environ.pop("KD_ATTN_BWD_V", None)
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
    d.add_argument("--ab", action="store_true", help="the library is the A/B one: also dump the variant tables' codes")
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    args = ap.parse_args()
    sys.exit(dump(args.out, args.tree, args.ab) if args.mode == "dump" else compare(args.a, args.b))
