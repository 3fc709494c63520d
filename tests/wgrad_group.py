"""Shared by tests/test_wgrad_group_gpu.py (product library) and
tools/ab_tests/test_wgrad_group_ab_gpu.py (A/B library): a student just large enough that both
weight-gradient groups of both towers take the grouped launch (csrc/gemm.hip k_gemm8_group), with
dimensions at which the 256 x 256 tile kernel's edges bite:

  SigLIP  hidden 384 (3 x 128: half-filled edge tiles in M and N, as 1152 and 896 are), inter 896
          (7 x 128), 6 heads x 64, 2 layers; 8 tiles of 729 patches = 5832 tokens, K % 32 == 8 (the
          c1 step's own count), so the k-loop ends in a partial stage
  Qwen2   hidden 384, inter 640 (5 x 128), 6 query / 2 kv heads x 64, 2 layers; 4 x 1536 = 6144
          tokens, K % 32 == 0 and K >= 2048 (the k-loop stagger's condition)
  groups  LM A: down 384 x 640 (6 tiles) + gate|up 1280 x 384 (10); LM B: o 384 x 384 (4) + q|k|v
          640 x 384 (6); ViT A: fc2 384 x 896 (8) + fc1 896 x 384 (8); ViT B: out 384 x 384 (4) +
          q|k|v 1152 x 384 (10) -- members of different tile counts, member offsets that are not
          multiples of 8 (the XCD remap runs on the member-local index)
  layers  two per tower: four norm backwards per tower, so the three-buffer rotation of the
          residual gradient wraps
"""
import math
from dataclasses import replace

import torch

PKG = "knowledge_distillation_for_sensory_substitution_in_multimodal_models_amd"

B, L = 4, 1536
GROUP_KEYS = {   # the timer keys of the four grouped launches per layer (largest member, ":g2")
    "gemm_nn:1280x384x6144:f32:acc:g2",   # LM A: gate|up (+ down)
    "gemm_nn:640x384x6144:f32:acc:g2",    # LM B: q|k|v (+ o)
    "gemm_nn:384x896x5832:f32:acc:g2",    # ViT A: fc2 + fc1 (equal flops: the first member names it)
    "gemm_nn:1152x384x5832:f32:acc:g2",   # ViT B: q|k|v (+ out)
}
# the members' own shapes: none may appear as a launch of its own when the groups run (SigLIP's
# out_proj, 384x384x5832, is left out: the two projector weight gradients, never grouped, share it)
MEMBER_SHAPES = {"384x640x6144", "1280x384x6144", "384x384x6144", "640x384x6144",
                 "384x896x5832", "896x384x5832", "1152x384x5832"}


def config():
    from importlib import import_module
    M = import_module(f"{PKG}.modeling")
    base = M.tiny_config(False)
    return replace(base, vision=replace(base.vision, hidden=384, inter=896, heads=6),
                   text=replace(base.text, hidden=384, inter=640, heads=6, kv_heads=2, head_dim=64))


def atomic_sum(name: str) -> bool:
    """Gradients the runtime sums with fp32 atomics, whose order is not fixed from run to run: the
    linear biases (k_colsum adds one partial per 64-row chunk), image_newline and embed_tokens
    (k_embed_bwd).  Their bits are no property of the weight-gradient lane; the bit-for-bit checks
    cover every other parameter and hold these to a reorder bound (REORDER_REL)."""
    if name == "image_newline" or name.endswith("embed_tokens.weight"):
        return True
    return name.endswith(".bias") and "layer_norm" not in name and "layernorm" not in name


# |a - b| <= REORDER_REL |a| for two orders of the same fp32 sum of n <= 96 partials (5832 or 6144
# rows in 64-row chunks; embed rows fewer): each order's error is <= (n - 1) 2^-24 sum |partial|,
# and the column sums of ~6000 zero-mean terms cancel to ~ sqrt(n) / n of sum |partial|, so
# 2 x 95 x 6e-8 x ~10 ~ 1e-4 of the norm bounds the difference
REORDER_REL = 1e-4


def reorder_close(va, vb, name):
    """-> (ok, difference norm, scale): two orders of the same fp32 sums.  The scale is the
    gradient's own norm, except for the SigLIP k_proj.bias, whose sum cancels to zero in exact
    arithmetic: there it is the same layer's q_proj.bias gradient (the existing rule's scale)."""
    scale_of = name
    if name.startswith("vision_tower.") and name.endswith("self_attn.k_proj.bias"):
        scale_of = name.replace("k_proj.bias", "q_proj.bias")
    d = float((va[name].double() - vb[name].double()).norm())
    s = float(va[scale_of].double().norm())
    return d <= REORDER_REL * s, d, s


def build(dev, seed=3):
    """The model, its seeded batch, a saved forward and the upstream gradient."""
    from importlib import import_module
    M = import_module(f"{PKG}.modeling")
    D = import_module(f"{PKG}.data")
    cfg = config()
    m = M.LlavaOnevisionModel(cfg, dev, trainable=True, seed=seed, cpu_rng=True)
    b = D.synthetic_batch(B, "cpu", L=L, seed=4, pixel_dtype=torch.bfloat16, cpu_rng=True)
    ids, px = b["depth_input_ids"].to(dev), b["depth_pixel_values"].to(dev)
    fwd = m.forward(ids, px, b["image_sizes"], save=True)
    g = torch.Generator().manual_seed(5)
    dhn = torch.randn(fwd["hn"].shape, generator=g) * 1e-2
    return dict(cfg=cfg, m=m, batch=b, fwd=fwd, dhn=dhn, dhn_dev=dhn.to(dev, torch.bfloat16))


def backward(r, zero=True):
    """One backward into the model's flat gradient (zeroed first unless zero=False); -> a copy."""
    m = r["m"]
    if zero:
        m.P.grad.zero_()
    m.backward(r["fwd"], r["dhn_dev"])
    torch.cuda.synchronize()
    return m.P.grad.clone()


def views(r, flat):
    """name -> that parameter's slice of a flat gradient copy."""
    P = r["m"].P
    return {s.name: P.view(s.name, flat) for s in P.specs}


def oracle_grads(r):
    """The fp32 CPU oracle's gradient of sum(hn * dhn) on the same (bf16-valued) weights.  The
    oracle's lm_head is given an 8-row stand-in: hn is taken before it, the logits are not used."""
    from oracle.model import OracleLlava
    m, b = r["m"], r["batch"]
    sd = {k: v.detach().float().cpu() for k, v in m.P.state_dict().items() if k != "language_model.lm_head.weight"}
    sw = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    sw["language_model.lm_head.weight"] = torch.zeros(8, r["cfg"].text.hidden)
    o = OracleLlava(sw, r["cfg"])
    o(b["depth_input_ids"], b["depth_pixel_values"].float(), b["image_sizes"])
    hn = o.last_hn
    (hn * r["dhn"].bfloat16().float().view_as(hn)).sum().backward()
    return {k: v.grad for k, v in sw.items() if v.grad is not None}


def figures(r, flat, ref):
    """Per parameter (cosine, | |g| / |g_ref| - 1 |) against the oracle; the SigLIP k_proj.bias
    (exactly zero in exact arithmetic, tests/step_parity.py) as |g| / |q_proj.bias gradient|."""
    P = r["m"].P
    out = {}
    for spec in P.specs:
        rr = ref.get(spec.name)
        if rr is None or float(rr.norm()) == 0.0:
            continue
        gv = P.view(spec.name, flat)
        if spec.ckpt_shape is not None:
            gv = gv[:, :math.prod(spec.ckpt_shape[1:])]
        a, q = gv.double().cpu().reshape(-1), rr.double().reshape(-1)
        if spec.name.startswith("vision_tower.") and spec.name.endswith("self_attn.k_proj.bias"):
            qn = float(P.view(spec.name.replace("k_proj.bias", "q_proj.bias"), flat).double().norm())
            out[spec.name] = dict(zero_ratio=float(a.norm()) / qn)
            continue
        out[spec.name] = dict(cos=float(a @ q / (a.norm() * q.norm())), nrel=abs(float(a.norm() / q.norm()) - 1))
    return out
