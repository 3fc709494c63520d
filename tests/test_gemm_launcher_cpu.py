"""The host half of csrc/gemm.hip through the C ABI, on the CPU (no kernel is launched):

1. kd_gemm_plan and kd_gemm_workspace_size over a fixed table (tests/golden/gemm_plan_table.json:
   every shape of tools/step_shapes_c1.json in the layout and dtypes its name gives, no fused
   epilogue, aligned fake pointers, x variant x split_k x workspace), recorded before the launcher
   was reorganised: the routing and the plan must reproduce every row.
       PYTHONPATH=. python tests/test_gemm_launcher_cpu.py --record     rewrites the table from the loaded library
2. one descriptor per argument check of launch_gemm / launch_gemm_f8 through kd_gemm: every check
   runs before any device call, so the status and the message come back with no device present;
   where a descriptor violates several checks the first one reports.
3. kd_gemm_plan follows kd_gemm where the launch overrides the plan: the fused q|k|v / backward
   activation epilogues are never split, row_stats and b_pretiled run v8 unsplit, and unaligned
   C / residual rows or an oversized MN-major lda leave the tiled kernels."""
import ctypes as C
import json
import sys
from pathlib import Path

import pytest

from knowledge_distillation_for_sensory_substitution_in_multimodal_models_amd import _native as NV
from knowledge_distillation_for_sensory_substitution_in_multimodal_models_amd import ops

REPO = Path(__file__).resolve().parent.parent
TABLE = REPO / "tests" / "golden" / "gemm_plan_table.json"
VARIANTS = (0, 1, 2, 3, 4, 5, 6, 7, 16, 21, 24, 32)
SPLITS = (0, 1, 3)
OK, SHAPE, ALIGN, ARG = 0, 1, 3, 7
KM, MN = NV.KD_LAYOUT_K_MAJOR, NV.KD_LAYOUT_MN_MAJOR
BF16, F32, FP8 = NV.KD_DTYPE_BF16, NV.KD_DTYPE_F32, NV.KD_DTYPE_FP8_E4M3
PA, PB, PC, PX, PW = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20   # fake 16-B aligned device pointers


def _desc(M=1024, N=1024, K=256, lay="kk", f32=False, acc=False, **kw):
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
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _query(d):
    v, s, dp = C.c_int32(), C.c_int32(), C.c_int32()
    assert NV.lib().kd_gemm_plan(C.byref(d), C.byref(v), C.byref(s), C.byref(dp)) == OK
    return v.value, s.value, dp.value


# ---------------------------------------------------------------- 1. the plan / workspace table
def _step_shapes():
    """(name, M, N, K, layout, fp32 C, accumulate) of every GEMM of the c1 step."""
    out = []
    for rec in json.loads((REPO / "tools" / "step_shapes_c1.json").read_text()):
        kind, mnk, *rest = rec["shape"].split(":")
        M, N, K = map(int, mnk.split("x"))
        out.append((rec["shape"], M, N, K, kind.split("_")[1], rest[0] == "f32", "acc" in rest))
    return out


def _table_rows():
    """name -> [[var, split, dp_tiles, workspace_size], ...] in VARIANTS x SPLITS x (no workspace, one) order."""
    rows = {}
    for name, M, N, K, lay, f32, acc in _step_shapes():
        r = []
        for variant in VARIANTS:
            for split_k in SPLITS:
                for ws in (0, ops.GEMM_SPLITK_WS):
                    d = _desc(M, N, K, lay, f32, acc, variant=variant, split_k=split_k,
                              workspace=PW if ws else None, workspace_bytes=ws)
                    r.append([*_query(d), int(NV.lib().kd_gemm_workspace_size(C.byref(d)))])
        rows[name] = r
    return rows


def test_plan_and_workspace_table():
    want = json.loads(TABLE.read_text())
    assert want["variants"] == list(VARIANTS) and want["split_k"] == list(SPLITS)
    got = _table_rows()
    assert sorted(got) == sorted(want["rows"]) and len(got) == 42
    keys = [(v, s, w) for v in VARIANTS for s in SPLITS for w in (0, ops.GEMM_SPLITK_WS)]
    for name in got:
        for key, g, w in zip(keys, got[name], want["rows"][name]):
            assert g == w, (name, dict(zip(("variant", "split_k", "workspace_bytes"), key)), g, w)


def test_swiglu_reports_v8_unsplit():
    for variant in (0, 16, 24):
        d = _desc(6144, 9728, 896, act=NV.KD_ACT_SWIGLU, variant=variant, workspace=PW, workspace_bytes=ops.GEMM_SPLITK_WS)
        assert _query(d) == (16, 1, 0)
        assert NV.lib().kd_gemm_workspace_size(C.byref(d)) == 0


# ---------------------------------------------------------------- 2. the argument checks through kd_gemm
def _run(d):
    st = NV.lib().kd_gemm(C.byref(d) if d is not None else None, None)
    return st, NV.lib().kd_last_error().decode()


def _qkv(**kw):
    """A well-formed q|k|v scatter for N = 1024: 8 + 2 * 4 heads of 64."""
    f = dict(q=PX, k=PX + (1 << 16), v=PX + (2 << 16), S=256, nq=8, nkv=4, hd=64, hdp=64)
    f.update(kw)
    return NV.KdQkvScatter(f["q"], f["k"], f["v"], f.get("cos_t"), f.get("sin_t"), f["S"], f["nq"], f["nkv"], f["hd"],
                           f["hdp"])


_KEEP = []   # the scatter structs the descriptors point to


def _with_qkv(sc=None, **kw):
    sc = sc if sc is not None else _qkv()
    _KEEP.append(sc)
    d = _desc(**kw)
    d.C, d.ldc = None, 0
    d.qkv = C.cast(C.pointer(sc), C.c_void_p)
    return d


def _f8(**kw):
    return _desc(**{**dict(ab_dtype=FP8, a_scale=PX, b_scale=PX + 4096), **kw})


DGELU, DSWIGLU, SWIGLU, GELU = NV.KD_ACT_DGELU_TANH, NV.KD_ACT_DSWIGLU, NV.KD_ACT_SWIGLU, NV.KD_ACT_GELU_TANH
RS = dict(M=1024, N=1024, row_stats=PX, row_stats_inv_t=1.0)

# (id, descriptor, status, fragment of the message): launch_gemm's checks in their order
GEMM_CHECKS = [
    ("null_desc", lambda: None, ARG, "gemm: null descriptor"),
    ("null_operand", lambda: _desc(A=None), ARG, "gemm: null operand"),
    ("empty_shape", lambda: _desc(M=0), SHAPE, "gemm: empty shape"),
    ("a_layout", lambda: _desc(a_layout=2), ARG, "gemm: a_layout"),
    ("b_layout", lambda: _desc(b_layout=2), ARG, "gemm: b_layout"),
    ("c_dtype", lambda: _desc(c_dtype=2), ARG, "gemm: c_dtype"),
    ("ab_dtype", lambda: _desc(ab_dtype=1), ARG, "gemm: ab_dtype"),
    ("qkv_fp8", lambda: _with_qkv(ab_dtype=FP8), ARG, "gemm qkv: bf16 operands only"),
    ("pretiled_split", lambda: _desc(b_pretiled=1, split_k=3), ARG, "gemm b_pretiled: K-major bf16 operands on the 256x256"),
    ("pretiled_variant", lambda: _desc(b_pretiled=1, variant=2), ARG, "gemm b_pretiled: K-major bf16 operands on the 256x256"),
    ("act_range", lambda: _desc(act=7), ARG, "gemm: act"),
    ("act_needs_bf16", lambda: _desc(act=GELU, f32=True), ARG, "an activation epilogue needs K-major operands"),
    ("dact_no_aux", lambda: _desc(lay="kn", act=DGELU), ARG, "gemm backward activation: aux (forward pre-activation)"),
    ("dact_ld_aux", lambda: _desc(lay="kn", act=DSWIGLU, aux=PX, ld_aux=1024, ldc=2048), SHAPE,
     "gemm backward activation: ldc / ld_aux >= N"),
    ("unknown_variant", lambda: _desc(variant=17), ARG, "gemm: unknown variant (the diagnostic / A-B builds 17-20, 22, 23, 26-28"),
    ("variant_31", lambda: _desc(variant=31), ARG, "gemm: unknown variant"),
    ("a_align", lambda: _desc(A=PA + 8), ALIGN, "gemm: A must be 16-B aligned"),
    ("b_align", lambda: _desc(B=PB + 8), ALIGN, "gemm: B must be 16-B aligned"),
    ("bias_align_bf16", lambda: _desc(bias=PX + 4), ALIGN, "gemm: bias must be 16-B (fp32) / 8-B (bf16) aligned"),
    ("bias_align_f32", lambda: _desc(bias=PX + 8, bias_dtype=F32), ALIGN, "gemm: bias must be"),
    ("ld_mult_8", lambda: _desc(lda=260), SHAPE, "gemm: lda/ldb must be multiples of 8"),
    ("a_kmajor", lambda: _desc(K=252, lda=256, ldb=256), SHAPE, "gemm: K-major A needs K % 8 == 0"),
    ("a_mnmajor", lambda: _desc(M=1028, lay="nk", lda=1032), SHAPE, "gemm: MN-major A needs M % 8 == 0"),
    ("a_mn_lda", lambda: _desc(lay="nk", lda=1 << 24), SHAPE, "gemm: lda too large"),
    ("b_kmajor", lambda: _desc(ldb=248), SHAPE, "gemm: K-major B needs K % 8 == 0, ldb >= K"),
    ("b_mnmajor", lambda: _desc(lay="kn", ldb=1016), SHAPE, "gemm: MN-major B needs N % 8 == 0, ldb >= N"),
    ("ldc", lambda: _desc(ldc=1016), SHAPE, "gemm: ldc < N (N/2 for swiglu)"),
    ("ldr", lambda: _desc(residual=PX, ldr=1016), SHAPE, "gemm: ldr < N"),
    ("res_f32", lambda: _desc(residual=PX, ldr=1024, residual_dtype=F32), ARG, "gemm: an fp32 residual needs an fp32 C"),
    ("ld_aux", lambda: _desc(aux=PX, ld_aux=1016), SHAPE, "gemm: ld_aux < N"),
    ("ld_31bit", lambda: _desc(lda=1 << 22), SHAPE, "gemm: leading dimension too large for 31-bit buffer records"),
    ("qkv_null_q", lambda: _with_qkv(_qkv(q=None)), ARG, "gemm qkv: null q / k / v or cos without sin"),
    ("qkv_cos_only", lambda: _with_qkv(_qkv(cos_t=PX)), ARG, "gemm qkv: null q / k / v or cos without sin"),
    ("qkv_accumulate", lambda: _with_qkv(acc=True), ARG, "gemm qkv: K-major operands, no activation"),
    ("qkv_heads", lambda: _with_qkv(_qkv(nq=9)), SHAPE, "gemm qkv: N = (nq + 2 nkv) hd"),
    ("qkv_q_align", lambda: _with_qkv(_qkv(q=PX + 8)), ALIGN, "gemm qkv: q must be 16-B aligned"),
    ("qkv_k_align", lambda: _with_qkv(_qkv(k=PX + 8)), ALIGN, "gemm qkv: k must be 16-B aligned"),
    ("qkv_v_align", lambda: _with_qkv(_qkv(v=PX + 8)), ALIGN, "gemm qkv: v must be 16-B aligned"),
    ("dact_small", lambda: _desc(M=128, N=128, lay="kn", act=DGELU, aux=PX, ld_aux=128), ARG,
     "gemm backward activation: needs the tiled kernels"),
    ("qkv_v1", lambda: _with_qkv(variant=1), ARG, "gemm qkv: needs the tiled kernels"),
    ("qkv_small", lambda: _with_qkv(_qkv(nq=2, nkv=1), M=256, N=256), ARG, "gemm qkv: needs the tiled kernels"),
    ("rs_bias", lambda: _desc(bias=PX + 64, **RS), ARG, "gemm row_stats: K-major bf16 operands, bf16 C"),
    ("rs_vs", lambda: _desc(row_stats_vs=4, **RS), SHAPE, "gemm row_stats: N and row_stats_vs multiples of 8"),
    ("rs_small", lambda: _desc(**{**RS, "M": 64}), SHAPE, "gemm row_stats: N and row_stats_vs multiples of 8"),
    ("rs_inv_t", lambda: _desc(**{**RS, "row_stats_inv_t": 0.0}), ARG, "gemm row_stats: row_stats_inv_t must be > 0"),
    ("rs_align", lambda: _desc(**{**RS, "row_stats": PX + 8}), ALIGN, "gemm row_stats: 16-B aligned"),
    ("glu_n", lambda: _desc(N=1152, act=SWIGLU), SHAPE, "gemm swiglu: N = 2I needs I % 128 == 0"),
    ("glu_bias", lambda: _desc(act=SWIGLU, bias=PX), ARG, "gemm swiglu: no bias / residual / accumulate / split-K"),
    ("glu_split", lambda: _desc(act=SWIGLU, split_k=3), ARG, "gemm swiglu: no bias / residual / accumulate / split-K"),
    ("glu_c_align", lambda: _desc(act=SWIGLU, C=PC + 8), ARG, "gemm swiglu: K-major operands, 16-B aligned bf16 output"),
    ("glu_aux_align", lambda: _desc(act=SWIGLU, aux=PX + 8, ld_aux=1024), ARG, "gemm swiglu: aux alignment"),
    ("pretiled_c_align", lambda: _desc(b_pretiled=1, C=PC + 8), ARG, "gemm b_pretiled: N % 8 == 0 and 16-B aligned C"),
    # variant 32 on ragged tiles: 25 tiles x 3 pieces of 256 KiB exceed the 3 M N 4 bytes the plan asks for
    ("fold_workspace", lambda: _desc(M=1032, N=1096, K=2304, variant=32, split_k=3, workspace=PW, workspace_bytes=14 << 20),
     ARG, "gemm: split-K fold workspace too small"),
]

F8_CHECKS = [
    ("f8_layout", lambda: _f8(lay="kn"), ARG, "gemm fp8: K-major operands only"),
    ("f8_scales", lambda: _f8(a_scale=None), ARG, "gemm fp8: null a_scale / b_scale"),
    ("f8_c_dtype", lambda: _f8(f32=True), ARG, "gemm fp8: bf16 output"),
    ("f8_split", lambda: _f8(split_k=3), ARG, "gemm fp8: no split-K"),
    ("f8_res_f32", lambda: _f8(residual=PX, ldr=1024, residual_dtype=F32), ARG, "gemm fp8: bf16 residual only"),
    ("f8_a_align", lambda: _f8(A=PA + 8), ALIGN, "gemm fp8: A must be 16-B aligned"),
    ("f8_b_align", lambda: _f8(B=PB + 8), ALIGN, "gemm fp8: B must be 16-B aligned"),
    ("f8_k16", lambda: _f8(K=264), SHAPE, "gemm fp8: K, lda, ldb must be multiples of 16"),
    ("f8_ld_31bit", lambda: _f8(lda=1 << 23), SHAPE, "gemm fp8: leading dimension too large for 31-bit buffer records"),
    ("f8_n8", lambda: _f8(N=1028, ldc=1032), SHAPE, "gemm fp8: N % 8 == 0 and 16-B aligned C / residual / aux rows"),
    ("f8_c_align", lambda: _f8(C=PC + 8), SHAPE, "gemm fp8: N % 8 == 0 and 16-B aligned C / residual / aux rows"),
    ("f8_ldc", lambda: _f8(ldc=1016), SHAPE, "gemm fp8: ldc < N (N/2 for swiglu)"),
    ("f8_ldr", lambda: _f8(residual=PX, ldr=1016), SHAPE, "gemm fp8: ldr < N"),
    ("f8_ld_aux", lambda: _f8(aux=PX, ld_aux=1016), SHAPE, "gemm fp8: ld_aux < N"),
    ("f8_glu_n", lambda: _f8(N=1152, act=SWIGLU), SHAPE, "gemm fp8 swiglu: N = 2I needs I % 128 == 0"),
    ("f8_glu_bias", lambda: _f8(act=SWIGLU, bias=PX), ARG, "gemm fp8 swiglu: no bias / residual / accumulate"),
    ("f8_aux", lambda: _f8(aux=PX, ld_aux=1024), ARG, "gemm fp8: aux (pre-activation) output only with KD_ACT_SWIGLU"),
]

# several violations at once: the first check in the launcher's order reports
FIRST_WINS = [
    ("null_before_shape_before_layout", lambda: _desc(A=None, M=0, a_layout=2), ARG, "gemm: null operand"),
    ("align_before_ld_before_ldc", lambda: _desc(A=PA + 8, lda=260, ldc=1016), ALIGN, "gemm: A must be 16-B aligned"),
    ("variant_before_align", lambda: _desc(variant=99, B=PB + 8, ldc=8), ARG, "gemm: unknown variant"),
    ("f8_dtype_before_split_before_align", lambda: _f8(f32=True, split_k=3, A=PA + 8), ARG, "gemm fp8: bf16 output"),
]


@pytest.mark.parametrize("make,status,fragment", [pytest.param(*c[1:], id=c[0]) for c in GEMM_CHECKS + F8_CHECKS + FIRST_WINS])
def test_argument_check(make, status, fragment):
    st, msg = _run(make())
    assert st == status and fragment in msg, (st, msg)


# ---------------------------------------------------------------- 3. the query follows the launch
WS = dict(workspace=PW, workspace_bytes=ops.GEMM_SPLITK_WS)


def test_query_plain_shape_splits():
    # the shape the cases below start from: alone, the cost model splits it
    assert _query(_desc(6144, 896, 4864, f32=True, **WS))[1] > 1
    assert _query(_desc(6144, 896, 9728, lay="kn", **WS))[1] > 1


def test_query_qkv_is_never_split():
    d = _with_qkv(_qkv(nq=10, nkv=2), M=6144, N=896, K=4864, **WS)
    v, s, dp = _query(d)
    assert s == 1 and dp == 0 and v in (2, 3, 4, 16)


@pytest.mark.parametrize("act", [DGELU, DSWIGLU])
def test_query_backward_activation_is_never_split(act):
    d = _desc(6144, 896, 9728, lay="kn", act=act, aux=PX, ld_aux=1792, ldc=1792, **WS)
    v, s, dp = _query(d)
    assert s == 1 and dp == 0 and v in (2, 3, 4, 16)


def test_query_row_stats_and_pretiled_run_v8_unsplit():
    assert _query(_desc(6144, 896, 4864, row_stats=PX, row_stats_inv_t=1.0, **WS)) == (16, 1, 0)
    assert _query(_desc(6144, 896, 4864, b_pretiled=1, **WS)) == (16, 1, 0)


def test_query_unaligned_rows_leave_the_tiled_kernels():
    assert _query(_desc(6144, 896, 4864, **WS))[0] != 1
    assert _query(_desc(6144, 896, 4864, ldc=900, **WS)) == (1, 1, 0)
    assert _query(_desc(6144, 896, 4864, C=PC + 8, **WS)) == (1, 1, 0)
    assert _query(_desc(6144, 896, 4864, residual=PX, ldr=900, **WS)) == (1, 1, 0)
    assert _query(_desc(6144, 896, 4864, residual=PX + 8, ldr=896, **WS)) == (1, 1, 0)


def test_query_oversized_mn_major_lda_leaves_the_tiled_kernels():
    assert _query(_desc(1152, 1152, 5832, lay="nn", f32=True, acc=True, **WS))[0] != 1
    assert _query(_desc(1152, 1152, 5832, lay="nn", f32=True, acc=True, lda=1 << 25, **WS)) == (1, 1, 0)


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        TABLE.write_text(json.dumps({"variants": list(VARIANTS), "split_k": list(SPLITS),
                                     "workspace_bytes": [0, ops.GEMM_SPLITK_WS], "columns": ["var", "split", "dp_tiles",
                                                                                               "workspace_size"],
                                     "rows": _table_rows()}, separators=(",", ":")) + "\n")
        print(f"{TABLE}: {len(_step_shapes())} shapes")
