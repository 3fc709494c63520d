"""The grouped weight-gradient launches against the same GEMMs launched one by one (A/B library):
with KD_WGRAD_GROUP=0 and KD_WGRAD_V8_UNSPLIT=1 the lane runs every weight gradient alone on the
256 x 256 v8 tile kernel, unsplit (a one-member launch), at the per-GEMM lane's launch points; every
gradient must equal the grouped run's bit for bit (tests/wgrad_group.py: the config, and the
parameters summed with fp32 atomics, which are held to the reorder bound instead).  And with
KD_WGRAD_GROUP=0 alone -- the planned, split-K per-GEMM lane -- the gradients agree to summation
order."""
import os

import pytest
import torch

import wgrad_group as WG

pytestmark = pytest.mark.gpu


def _grads(dev, **env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        r = WG.build(dev)   # the knobs are read when the model handle is created
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    from importlib import import_module
    ops = import_module(f"{WG.PKG}.ops")
    ops.TIMER.reset()
    ops.TIMER.enabled = True
    try:
        g = WG.backward(r)
        keys = [k for k, _, _ in ops.TIMER.records()]
    finally:
        ops.TIMER.enabled = False
        ops.TIMER.reset()
    return r, g, keys


@pytest.fixture(scope="module")
def grouped(dev):
    return _grads(dev, KD_WGRAD_GROUP=1)


def test_one_by_one_unsplit_v8_equals_grouped_bit_for_bit(grouped, dev):
    r, g, keys = grouped
    assert {k for k in keys if k.endswith(":g2")} == WG.GROUP_KEYS
    r1, g1, keys1 = _grads(dev, KD_WGRAD_GROUP=0, KD_WGRAD_V8_UNSPLIT=1)
    assert not [k for k in keys1 if k.endswith(":g2")]
    assert len([k for k in keys1 if k.endswith(":g1")]) == 16   # 8 grouped GEMMs per layer pair, 2 layers
    va, vb = WG.views(r, g), WG.views(r1, g1)
    for n in va:
        if WG.atomic_sum(n):
            ok, d, s = WG.reorder_close(va, vb, n)
            assert ok, (n, d, s)
        else:
            assert torch.equal(va[n], vb[n]), (n, float((va[n] - vb[n]).abs().max()))


def test_planned_per_gemm_lane_agrees_to_summation_order(grouped, dev):
    r, g, _ = grouped
    r0, g0, keys0 = _grads(dev, KD_WGRAD_GROUP=0)
    assert not [k for k in keys0 if k.rsplit(":", 1)[-1].startswith("g")]
    va, vb = WG.views(r, g), WG.views(r0, g0)
    for n in va:
        ok, d, s = WG.reorder_close(va, vb, n)   # fp32 sums of ~6000 bf16 products in another order
        assert ok, (n, d, s)
