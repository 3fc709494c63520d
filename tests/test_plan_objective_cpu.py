"""kd_gemm_plan_objective (csrc/gemm.hip plan_gemm_objective) through the C ABI on the CPU: the GEMM
planner's second objective, least CU-time instead of least isolated latency.  Descriptors
as tests/test_gemm_launcher_cpu.py builds them: every shape of tools/step_shapes_c1.json in the layout
and dtypes its name gives, aligned fake pointers, the runtime's split-K workspace.

    PYTHONPATH=. python tests/test_plan_objective_cpu.py --record    rewrites the fixture from the loaded library

One limit of the design shows here: the CU-time plan is handed to the launch as a forced descriptor, and
split_k = 1 on an output under 2^20 elements leaves the tiled kernels (gemm.hip tiled_ok: such an output
is tiled only when split).  Those descriptors keep the latency plan, split included; "never a split" is
asserted for every output of 2^20 elements or more, and "the same plan as objective 0" for the rest."""
import ctypes as C
import json
import sys
from pathlib import Path

import pytest

from knowledge_distillation_for_sensory_substitution_in_multimodal_models_amd import _native as NV
from knowledge_distillation_for_sensory_substitution_in_multimodal_models_amd import ops

REPO = Path(__file__).resolve().parent.parent
FIXTURE = REPO / "tests" / "golden" / "plan_objective_c1.json"
KM, MN = NV.KD_LAYOUT_K_MAJOR, NV.KD_LAYOUT_MN_MAJOR
BF16, F32, FP8 = NV.KD_DTYPE_BF16, NV.KD_DTYPE_F32, NV.KD_DTYPE_FP8_E4M3
PA, PB, PC, PX, PW = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20   # fake 16-B aligned device pointers
LATENCY, CU_TIME = 0, 1
MARGIN = 0.05   # gemm.hip kCuMargin


def desc(M, N, K, lay="kk", f32=False, acc=False, **kw):
    d = NV.KdGemmDesc()
    d.M, d.N, d.K = M, N, K
    d.a_layout = KM if lay[0] == "k" else MN
    d.b_layout = KM if lay[1] == "k" else MN
    d.A, d.B, d.C = PA, PB, PC
    d.lda = K if lay[0] == "k" else M
    d.ldb = K if lay[1] == "k" else N
    d.ldc = N
    d.c_dtype = F32 if f32 else BF16
    d.accumulate = int(acc)
    d.alpha = 1.0
    d.workspace, d.workspace_bytes = PW, ops.GEMM_SPLITK_WS
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def plan(d, objective):
    """(variant, split_k, dp_tiles, latency_us, cu_us)"""
    v, s, dp, lat, cu = C.c_int32(), C.c_int32(), C.c_int32(), C.c_double(), C.c_double()
    st = NV.lib().kd_gemm_plan_objective(C.byref(d), objective, C.byref(v), C.byref(s), C.byref(dp), C.byref(lat),
                                         C.byref(cu))
    assert st == 0, NV.lib().kd_last_error()
    return v.value, s.value, dp.value, lat.value, cu.value


def plan0(d):
    v, s, dp = C.c_int32(), C.c_int32(), C.c_int32()
    assert NV.lib().kd_gemm_plan(C.byref(d), C.byref(v), C.byref(s), C.byref(dp)) == 0
    return v.value, s.value, dp.value


def step_shapes():
    """(name, M, N, K, layout, fp32 C, accumulate) of every plain GEMM of the c1 step."""
    out = []
    for rec in json.loads((REPO / "tools" / "step_shapes_c1.json").read_text()):
        kind, mnk, *rest = rec["shape"].split(":")
        M, N, K = map(int, mnk.split("x"))
        out.append((rec["shape"], M, N, K, kind.split("_")[1], rest[0] == "f32", "acc" in rest))
    return out


SHAPES = step_shapes()


def test_objective_0_is_kd_gemm_plan():
    for name, M, N, K, lay, f32, acc in SHAPES:
        for variant in (0, 1, 2, 3, 4, 16, 21, 32):
            for split_k in (0, 1, 3):
                d = desc(M, N, K, lay, f32, acc, variant=variant, split_k=split_k)
                assert plan(d, LATENCY)[:3] == plan0(d), (name, variant, split_k)


def test_cu_time_never_splits_and_never_costs_more():
    for name, M, N, K, lay, f32, acc in SHAPES:
        d = desc(M, N, K, lay, f32, acc)
        p0, p1 = plan(d, LATENCY), plan(d, CU_TIME)
        if M * N >= 1 << 20:
            assert p1[1] == 1 and p1[2] == 0, (name, p1)
        else:   # tiled only when split: not forceable, the latency plan stays
            assert p1 == p0, (name, p0, p1)
        assert p1[4] <= p0[4], (name, p0, p1)
        if p1[:3] != p0[:3] and p0[1] == 1:   # a changed tile kernel saves at least the margin
            assert p1[4] <= p0[4] * (1 - MARGIN), (name, p0, p1)
        assert p1[3] > 0 and p1[4] > 0 and p1[4] <= p1[3] * (1 + 1e-12), (name, p1)   # CU-time has no wave rounding


def test_cu_time_honours_forced_variant_and_split():
    for name, M, N, K, lay, f32, acc in SHAPES:
        if M * N < 1 << 20:
            continue
        for variant in (2, 3, 4, 16):
            p = plan(desc(M, N, K, lay, f32, acc, variant=variant), CU_TIME)
            assert p[0] == variant and p[1] == 1, (name, variant, p)
            forced = desc(M, N, K, lay, f32, acc, variant=variant, split_k=3)
            assert plan(forced, CU_TIME)[:3] == plan0(forced), (name, variant)
        forced = desc(M, N, K, lay, f32, acc, split_k=3)
        p = plan(forced, CU_TIME)
        assert p[1] == plan0(forced)[1], (name, p)   # a forced split stays (3 where K allows it); the tile may change
        for variant in (1, 21, 32):   # codes the objective does not plan: the descriptor's own plan
            other = desc(M, N, K, lay, f32, acc, variant=variant)
            assert plan(other, CU_TIME) == plan(other, LATENCY), (name, variant)


# DESIGN §5.2 / the table the change was proposed with: the student chain's plain forward and dgrad
# GEMMs of c1, (variant, split_k) under latency -> under CU-time
C1_PICKS = {
    "gemm_kk:6144x1152x896:bf16": ((3, 1), (2, 1)),     # LM q|k|v fwd
    "gemm_kk:6144x896x896:f32": ((3, 1), (2, 1)),       # LM o fwd
    "gemm_kk:6144x896x4864:f32": ((16, 2), (16, 1)),    # LM down fwd
    "gemm_kn:6144x896x9728:bf16": ((16, 2), (16, 1)),   # LM dgrad gate|up
    "gemm_kn:6144x896x896:bf16": ((4, 1), (16, 1)),     # LM dgrad o
    "gemm_kn:6144x896x1152:bf16": ((4, 1), (16, 1)),    # LM dgrad q|k|v
    "gemm_kk:5832x1152x1152:f32": ((3, 1), (2, 1)),     # ViT out fwd
    "gemm_kk:5832x1152x4304:f32": ((3, 1), (16, 1)),    # ViT fc2 fwd
    "gemm_kn:5832x1152x4304:bf16": ((16, 2), (16, 1)),  # ViT dgrad fc1
    "gemm_kn:5832x1152x1152:bf16": ((4, 1), (16, 1)),   # ViT dgrad out
    "gemm_kn:5832x1152x3456:bf16": ((16, 2), (16, 1)),  # ViT dgrad q|k|v
    # keep their plans: ViT q|k|v fwd, fc1 fwd, the fused dact dgrads
    "gemm_kk:5832x3456x1152:bf16": ((2, 1), (2, 1)),
    "gemm_kk:5832x4304x1152:bf16": ((2, 1), (2, 1)),
    "gemm_kn_dact:6144x4864x896:bf16": ((16, 1), (16, 1)),
    "gemm_kn_dact:5832x4304x1152:bf16": ((16, 1), (16, 1)),
}


def _fixture_rows():
    rows = {}
    for name, M, N, K, lay, f32, acc in SHAPES:
        p = plan(desc(M, N, K, lay, f32, acc), CU_TIME)
        rows[name] = [p[0], p[1], p[2]]
    return rows


def test_c1_picks():
    by_name = {s[0]: s for s in SHAPES}
    for name, (lat, cu) in C1_PICKS.items():
        _, M, N, K, lay, f32, acc = by_name[name]
        d = desc(M, N, K, lay, f32, acc)
        p0, p1 = plan(d, LATENCY), plan(d, CU_TIME)
        assert p0[:2] == lat and p1[:2] == cu, (name, p0, p1)
        if lat != cu:
            assert p1[4] <= 0.85 * p0[4], (name, p0, p1)   # every changed pick saves at least 15 % of its CU-time
    want = json.loads(FIXTURE.read_text())
    assert _fixture_rows() == want


def test_other_routes_keep_their_plan():
    scatter = NV.KdQkvScatter(PX, PX, PX, None, None, 1536, 14, 2, 64, 64)
    fused = {
        "fp8": dict(ab_dtype=FP8, a_scale=PX, b_scale=PX, split_k=1),
        "row statistics": dict(row_stats=PX, row_stats_vs=1024),
        "swiglu": dict(act=NV.KD_ACT_SWIGLU),
        "v1": dict(variant=1),
        "unaligned C rows": dict(ldc=1027),
    }
    for what, kw in fused.items():
        d = desc(6144, 1024, 4864, **kw)
        assert plan(d, CU_TIME) == plan(d, LATENCY), what
    # the fused epilogues stay unsplit under both objectives; only their tile kernel may change
    for what, kw in {"q|k|v scatter": dict(qkv=C.cast(C.pointer(scatter), C.c_void_p), split_k=1),
                     "dact": dict(act=NV.KD_ACT_DSWIGLU, aux=PX, ld_aux=2 * 4864, lay="kn")}.items():
        lay = kw.pop("lay", "kk")
        d = desc(6144, 1152 if what != "dact" else 4864, 896, lay, **kw)
        p0, p1 = plan(d, LATENCY), plan(d, CU_TIME)
        assert p0[1] == 1 and p1[1] == 1 and p1[4] <= p0[4], (what, p0, p1)
    d = desc(1024, 1024, 256)
    v, s, dp, lat, cu = C.c_int32(), C.c_int32(), C.c_int32(), C.c_double(), C.c_double()
    assert NV.lib().kd_gemm_plan_objective(C.byref(d), 2, C.byref(v), C.byref(s), C.byref(dp), C.byref(lat),
                                           C.byref(cu)) != 0   # unknown objective


if __name__ == "__main__":
    if "--record" in sys.argv:
        FIXTURE.write_text(json.dumps(_fixture_rows(), indent=0, sort_keys=True) + "\n")
        print(f"wrote {FIXTURE}")
