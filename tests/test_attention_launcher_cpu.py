"""The host half of csrc/attention.hip through the C ABI, on the CPU (no kernel is launched):

1. one descriptor per argument check of kd_attn_fwd / kd_attn_bwd: every check runs before any
   device call, so the status and the message come back with no device present; where a
   descriptor violates several checks the first one in the launcher's order reports.
2. kd_attn_bwd_workspace_size over MHA, GQA and a null descriptor.

The expected status, message and size of every row live in tests/golden/attn_reject_table.json.
That table was recorded from the library of the commit BEFORE the attention launcher was
reorganised (named builds, one dispatch, one shape check), so the reorganised launcher has to
reproduce the old one's status codes, texts and order of first failure row by row.
    PYTHONPATH=. python tests/test_attention_launcher_cpu.py --record     rewrites the table from the loaded library
(KDSTEP_LIB=<path> selects the library to record from)."""
import ctypes as C
import json
import sys
from pathlib import Path

import pytest

from knowledge_distillation_for_sensory_substitution_in_multimodal_models_amd import _native as NV

REPO = Path(__file__).resolve().parent.parent
TABLE = REPO / "tests" / "golden" / "attn_reject_table.json"
SHAPE, ARG, WORKSPACE = 1, 7, 8
# fake 16-B aligned device pointers
PQ, PK, PV, PO, PDO, PLSE, PDEL, PDQ, PDK, PDV, PW, PQKV, PCOS, PSIN = ((i + 1) << 20 for i in range(14))


def _fwd(**kw):
    f = dict(q=PQ, k=PK, v=PV, o=PO, lse=PLSE, B=1, H=4, HKV=4, S=100, hd=64, hdp=64, causal=0)
    f.update(kw)
    d = NV.KdAttnDesc()
    for k, v in f.items():
        setattr(d, k, v)
    return d


def _bwd(**kw):
    """MHA with split dq / dk / dv outputs unless the keywords say otherwise."""
    f = dict(q=PQ, k=PK, v=PV, o=PO, dO=PDO, lse=PLSE, delta=PDEL, dq=PDQ, dk=PDK, dv=PDV, B=1, H=4, HKV=4, S=100,
             hd=64, hdp=64, causal=0)
    f.update(kw)
    d = NV.KdAttnBwdDesc()
    for k, v in f.items():
        setattr(d, k, v)
    return d


def _gqa(**kw):
    """GQA (4 query heads per kv head) with a workspace of exactly the size the library asks for."""
    d = _bwd(**{**dict(H=8, HKV=2), **kw})
    if "workspace" not in kw:
        d.workspace, d.workspace_bytes = PW, NV.lib().kd_attn_bwd_workspace_size(C.byref(d))
    return d


def _dqkv(make=_bwd, **kw):
    """The fused token-major dq | dk | dv output, ld_qkv = (H + 2 HKV) hd unless given."""
    d = make(**{**dict(dq=None, dk=None, dv=None, dqkv=PQKV), **kw})
    if "ld_qkv" not in kw:
        d.ld_qkv = (d.H + 2 * d.HKV) * d.hd
    return d


def _rope(**kw):
    return _dqkv(_gqa, **{**dict(cos_t=PCOS, sin_t=PSIN), **kw})


# (id, descriptor): launch_attn_fwd's checks in their order
FWD_CHECKS = [
    ("fwd_null_desc", lambda: None),
    *[(f"fwd_null_{n}", lambda n=n: _fwd(**{n: None})) for n in ("q", "k", "v", "o")],
    ("fwd_B", lambda: _fwd(B=0)),
    ("fwd_S", lambda: _fwd(S=0)),
    ("fwd_H", lambda: _fwd(H=0)),
    ("fwd_HKV", lambda: _fwd(HKV=0)),
    ("fwd_H_mod_HKV", lambda: _fwd(H=6, HKV=4)),
    ("fwd_hd_zero", lambda: _fwd(hd=0)),
    ("fwd_hd_mod_4", lambda: _fwd(hd=62)),
    ("fwd_hd_gt_hdp", lambda: _fwd(hd=68, hdp=64)),
    ("fwd_hdp_80", lambda: _fwd(hd=72, hdp=80)),
    ("fwd_hdp_256", lambda: _fwd(hd=128, hdp=256)),
    *[(f"fwd_hd_{hd}_at_96", lambda hd=hd: _fwd(hd=hd, hdp=96)) for hd in (84, 88, 92, 96)],
]

# launch_attn_bwd's checks in their order
BWD_CHECKS = [
    ("bwd_null_desc", lambda: None),
    *[(f"bwd_null_{n}", lambda n=n: _bwd(**{n: None})) for n in ("q", "k", "v", "o", "dO", "lse", "delta", "dq", "dk", "dv")],
    ("bwd_dqkv_ld_small", lambda: _dqkv(ld_qkv=12 * 64 - 4)),
    ("bwd_dqkv_ld_mod_4", lambda: _dqkv(ld_qkv=12 * 64 + 2)),
    ("bwd_dqkv_align", lambda: _dqkv(dqkv=PQKV + 4)),
    ("bwd_rope_cos_only", lambda: _rope(sin_t=None)),
    ("bwd_rope_sin_only", lambda: _rope(cos_t=None)),
    ("bwd_rope_no_dqkv", lambda: _gqa(cos_t=PCOS, sin_t=PSIN)),
    ("bwd_rope_mha", lambda: _dqkv(cos_t=PCOS, sin_t=PSIN)),
    ("bwd_rope_hd_ne_hdp", lambda: _rope(hd=32, hdp=64)),
    ("bwd_rope_hd_mod_32", lambda: _rope(hd=72, hdp=72)),
    ("bwd_dqkv_gqa_hd_mod_8", lambda: _dqkv(_gqa, hd=68, hdp=96)),
    ("bwd_B", lambda: _bwd(B=0)),
    ("bwd_S", lambda: _bwd(S=0)),
    ("bwd_HKV", lambda: _bwd(HKV=0)),
    ("bwd_H_mod_HKV", lambda: _bwd(H=6, HKV=4)),
    ("bwd_hd_mod_4", lambda: _bwd(hd=62)),
    ("bwd_hd_gt_hdp", lambda: _bwd(hd=72, hdp=64)),
    ("bwd_hdp_80", lambda: _bwd(hd=72, hdp=80)),
    ("bwd_hdp_256", lambda: _bwd(hd=128, hdp=256)),
    *[(f"bwd_hd_{hd}_at_96", lambda hd=hd: _bwd(hd=hd, hdp=96)) for hd in (84, 88, 92, 96)],
    ("bwd_hd_mod_8", lambda: _bwd(hd=68, hdp=96)),
    ("bwd_hd_mod_8_dqkv_mha", lambda: _dqkv(hd=60, hdp=64)),
    ("bwd_gqa_no_workspace", lambda: _gqa(workspace=None, workspace_bytes=1 << 30)),
    ("bwd_gqa_workspace_small", lambda: _gqa(workspace=PW, workspace_bytes=2 * 1 * 8 * 100 * 64 * 4 - 1)),
    ("bwd_gqa_dqkv_workspace_small", lambda: _dqkv(_gqa, workspace=PW, workspace_bytes=0)),
]

# several violations at once: the first check in the launcher's order reports
FIRST_WINS = [
    ("fwd_null_before_heads_before_hdp", lambda: _fwd(q=None, H=6, HKV=4, hdp=80)),
    ("fwd_heads_before_hd_before_hdp", lambda: _fwd(H=6, HKV=4, hd=62, hdp=80)),
    ("fwd_hd_before_hdp", lambda: _fwd(hd=90, hdp=100)),
    ("bwd_dqkv_before_rope_before_shape", lambda: _dqkv(dqkv=PQKV + 4, cos_t=PCOS, B=0, hdp=80)),
    ("bwd_rope_before_gqa_hd_before_shape", lambda: _dqkv(_gqa, hd=68, hdp=96, cos_t=PCOS, workspace=None, S=0)),
    ("bwd_shape_before_hdp_before_workspace", lambda: _gqa(hd=66, hdp=80, workspace=None)),
    ("bwd_cover_before_hd_mod_8_before_workspace", lambda: _gqa(hd=84, hdp=96, workspace=None)),
]

CHECKS = FWD_CHECKS + BWD_CHECKS + FIRST_WINS

# kd_attn_bwd_workspace_size: 0 for MHA and for a null descriptor, 2 B H S hdp fp32 partials for GQA
WORKSPACE_CASES = [
    ("null_desc", lambda: None),
    ("mha_64", lambda: _bwd()),
    ("mha_siglip", lambda: _bwd(B=2, H=16, HKV=16, S=729, hd=72, hdp=96)),
    ("gqa_qwen_05b", lambda: _bwd(B=2, H=14, HKV=2, S=1000, hd=64, hdp=64)),
    ("gqa_qwen_7b", lambda: _bwd(B=1, H=28, HKV=4, S=4096, hd=128, hdp=128)),
    ("gqa_hkv_zero", lambda: _bwd(H=8, HKV=0)),
]


def _run(cid, d):
    f = NV.lib().kd_attn_fwd if cid.startswith("fwd_") else NV.lib().kd_attn_bwd
    st = f(C.byref(d) if d is not None else None, None)
    return st, NV.lib().kd_last_error().decode()


def _size(d):
    return int(NV.lib().kd_attn_bwd_workspace_size(C.byref(d) if d is not None else None))


def _table():
    return json.loads(TABLE.read_text())


def test_table_covers_every_case():
    t = _table()
    assert sorted(t["checks"]) == sorted(c[0] for c in CHECKS) and len(t["checks"]) == len(CHECKS)
    assert sorted(t["workspace"]) == sorted(c[0] for c in WORKSPACE_CASES)
    # every recorded row is a rejection made before any device call
    assert all(r["status"] in (SHAPE, ARG, WORKSPACE) for r in t["checks"].values())


@pytest.mark.parametrize("cid,make", [pytest.param(*c, id=c[0]) for c in CHECKS])
def test_argument_check(cid, make):
    want = _table()["checks"][cid]
    st, msg = _run(cid, make())
    assert (st, msg) == (want["status"], want["message"])


@pytest.mark.parametrize("cid,make", [pytest.param(*c, id=c[0]) for c in WORKSPACE_CASES])
def test_bwd_workspace_size(cid, make):
    assert _size(make()) == _table()["workspace"][cid]


def test_bwd_workspace_size_formula():
    assert _size(_bwd(B=2, H=14, HKV=2, S=1000, hd=64, hdp=64)) == 2 * 2 * 14 * 1000 * 64 * 4
    assert _size(_bwd()) == 0 and _size(None) == 0


if __name__ == "__main__":
    if sys.argv[1:] == ["--record"]:
        rows = {}
        for cid, make in CHECKS:
            st, msg = _run(cid, make())
            rows[cid] = {"status": st, "message": msg}
        TABLE.write_text(json.dumps({"library": "the parent commit's (before the launcher was reorganised)",
                                     "checks": rows, "workspace": {cid: _size(make()) for cid, make in WORKSPACE_CASES}},
                                    indent=1) + "\n")
        print(f"{TABLE}: {len(rows)} checks, {len(WORKSPACE_CASES)} workspace sizes")
