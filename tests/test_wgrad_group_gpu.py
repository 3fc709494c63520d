"""The weight-gradient lane's grouped, unsplit launches (csrc/gemm.hip k_gemm8_group, csrc/model.hip):
a student (tests/wgrad_group.py: hidden 384, inter 640 / 896, two layers per tower, 4 x 1536 tokens,
8 SigLIP tiles = 5832 rows with K % 32 == 8) whose four groups per layer all take the grouped path,
through the product library.

Held:
  * the grouped path ran: the timer shows the four ":g2" keys twice (two layers) per backward and no
    member as a launch of its own;
  * every trainable parameter's gradient of sum(hn * g) against the fp32 CPU oracle on the same
    weights: norm within 1 %, cosine >= 0.999, the SigLIP k_proj.bias (zero in exact arithmetic) at
    |g| <= 1e-2 |q_proj.bias gradient| -- the full-depth tests' bounds;
  * a second backward into the same buffer gives exactly twice the first gradient, and two runs give
    identical bits, for every parameter the lane's GEMMs and the norm backward write; the linear
    biases, image_newline and embed_tokens are summed with fp32 atomics in no fixed order
    (k_colsum, k_embed_bwd; not this lane's work) and are held to the reorder bound
    wgrad_group.REORDER_REL instead;
  * with the vision tower frozen, and separately with the language model frozen, the frozen range
    stays exactly zero and everything else matches the unfrozen run (bits / the reorder bound).

Measured against the oracle at this config (one MI355X; the parent commit, whose lane splits K and
folds fp32 partial planes, beside it): see FIGURES below.
"""
import pytest
import torch

import wgrad_group as WG

pytestmark = pytest.mark.gpu

# worst figures over the 66 parameters against the oracle, one MI355X (wgrad_group.figures); both meet
# the bounds, so the bounds are held as stated
FIGURES = {
    "parent (split-K lane)": "cosine 0.99990418, norm miss 1.47199e-3, k_proj.bias ratio 3.17730e-4",
    "grouped": "cosine 0.99990418, norm miss 1.47202e-3, k_proj.bias ratio 3.17730e-4",
}


@pytest.fixture(scope="module")
def run(dev):
    from importlib import import_module
    ops = import_module(f"{WG.PKG}.ops")
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    r = WG.build(dev)
    ops.TIMER.reset()
    ops.TIMER.enabled = True
    try:
        r["g1"] = WG.backward(r)
        r["keys"] = [k for k, _, _ in ops.TIMER.records()]
    finally:
        ops.TIMER.enabled = False
        ops.TIMER.reset()
    return r


def _same(r, a, b, what):
    va, vb = WG.views(r, a), WG.views(r, b)
    for n in va:
        if WG.atomic_sum(n):
            ok, d, s = WG.reorder_close(va, vb, n)
            assert ok, (what, n, d, s)
        else:
            assert torch.equal(va[n], vb[n]), (what, n, float((va[n] - vb[n]).abs().max()))


def test_grouped_path_ran(run):
    keys = run["keys"]
    grouped = [k for k in keys if k.rsplit(":", 1)[-1].startswith("g")]
    assert set(grouped) == WG.GROUP_KEYS, sorted(set(grouped))
    for k in WG.GROUP_KEYS:
        assert grouped.count(k) == 2, (k, grouped.count(k))   # two layers per tower
    alone = [k for k in keys if k.startswith("gemm_nn:") and k.split(":")[1] in WG.MEMBER_SHAPES
             and not k.rsplit(":", 1)[-1].startswith("g")]
    assert not alone, alone


def test_gradients_match_fp32_oracle(run):
    ref = WG.oracle_grads(run)
    fig = WG.figures(run, run["g1"], ref)
    assert len(fig) >= 40
    worst = dict(cos=1.0, nrel=0.0, zero_ratio=0.0)
    for n, v in fig.items():
        print(n, v)
        for k in v:
            worst[k] = min(worst[k], v[k]) if k == "cos" else max(worst[k], v[k])
    print("worst", worst)
    for n, v in fig.items():
        if "zero_ratio" in v:
            assert v["zero_ratio"] <= 1e-2, (n, v)
        else:
            assert v["cos"] >= 0.999 and v["nrel"] <= 1e-2, (n, v)


def test_second_backward_accumulates_exactly_twice(run):
    first = WG.backward(run)
    both = WG.backward(run, zero=False)   # on top of the first
    _same(run, 2 * first, both, "accumulate")


def test_two_runs_give_identical_bits(run):
    _same(run, run["g1"], WG.backward(run), "rerun")


@pytest.mark.parametrize("frozen", ["vision", "language"])
def test_frozen_tower_drops_out_of_its_groups(run, frozen):
    m = run["m"]
    m.set_trainable(frozen != "vision", True, frozen != "language")
    try:
        g = WG.backward(run)
    finally:
        m.set_trainable(True, True, True)
    vf, v1 = WG.views(run, g), WG.views(run, run["g1"])
    tower = "vision_tower." if frozen == "vision" else "language_model."
    for n in vf:
        if n.startswith(tower):
            assert not bool(vf[n].any()), (frozen, n)
        elif WG.atomic_sum(n):
            ok, d, s = WG.reorder_close(v1, vf, n)
            assert ok, (frozen, n, d, s)
        else:
            assert torch.equal(vf[n], v1[n]), (frozen, n)
