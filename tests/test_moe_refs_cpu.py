"""Pins the references of tests/moe_refs.py (which tests/test_gpu_moe_kernels.py
holds the HIP MoE kernels to) against a second, independent statement of
each, on CPU:

* integer grouped GEMM: float64 vs fp32-accumulated matmul, bitwise after the
  bf16 cast, and every possible partial sum far below 2^24;
* rows combine: the ordered fp32 sum vs a float64 index_add, within 1 bf16 ulp;
* SparseMoE layer: the sort-free float64 restatement vs the module's own CPU
  eager path in float64; the routing filter keeps enough tokens.
"""

import pytest
import torch

from tests import moe_refs as R


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("case", R.GEMM_CASES, ids=R.GEMM_IDS)
def test_int_gemm_reference_is_exact(case, bias):
    E, N, K, counts = case
    inp = R.int_gemm_inputs(E, N, K, counts, bias)
    for k in ("x", "w", "dy"):
        v = inp[k].double()
        assert v.abs().max() <= 3 and torch.equal(v, v.round())
    if bias:
        v = inp["b"].double()
        assert v.abs().max() <= 8 and torch.equal(v, v.round())

    # any partial sum, in any order, is an integer of magnitude <= these
    bounds = R.gemm_sum_bounds(inp, counts)
    print("SUMBOUNDS", case[:3], bounds)
    assert max(bounds) < 2**24
    assert bounds[0] <= 9 * K + 8 and bounds[1] <= 9 * N and bounds[2] <= 9 * max(counts)

    e64 = R.gemm_expected(inp, counts, torch.float64)
    e32 = R.gemm_expected(inp, counts, torch.float32)
    for k in ("y", "dx", "dw", "db"):
        if e64[k] is None:
            assert not bias and e32[k] is None
            continue
        assert torch.equal(R.bits(e64[k]), R.bits(e32[k])), k
        assert not (R.bits(e64[k]) == R.bits(torch.tensor(-0.0, dtype=R.BF16))).any(), f"{k} has a -0"
    # empty experts: +0 bits in dw
    for e, c in enumerate(counts):
        if c == 0:
            assert not R.bits(e64["dw"][e]).any()


def test_int_gemm_cast_does_round():
    """The sums must exceed 256 somewhere, or the final bf16 cast (8
    significand bits) would never round and a truncating store would pass."""
    E, N, K, counts = R.GEMM_CASES[1]
    inp = R.int_gemm_inputs(E, N, K, counts, True)
    e = R.gemm_expected(inp, counts)
    off = R._offsets(counts)
    y64 = inp["x"][off[2]:off[3]].double() @ inp["w"][2].double().T + inp["b"][2].double()
    assert y64.abs().max() > 256
    assert not torch.equal(e["y"][off[2]:off[3]].double(), y64)


@pytest.mark.parametrize("T,K,k_top", R.COMBINE_CASES)
def test_combine_reference_vs_float64_index_add(T, K, k_top):
    inp = R.combine_inputs(T, K, k_top)
    h, inv, batch_index = inp["h"], inp["inv"], inp["batch_index"]
    # inv is a permutation and inverts the sort: slot inv[p] belongs to token p // k_top
    assert sorted(inv.tolist()) == list(range(T * k_top))
    assert torch.equal(batch_index[inv.long()], torch.arange(T * k_top) // k_top)

    got = R.combine_expected(h, inv, T, k_top)
    ref = torch.zeros(T, K, dtype=torch.float64).index_add(0, batch_index, h.double())
    # 1 bf16 ulp of the result's binade: 2^(floor(log2|ref|) - 7)
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0**-126))) - 7)
    assert ((got.double() - ref).abs() <= ulp).all()


@pytest.fixture(scope="module", params=R.LAYER_CONFIGS, ids=R.LAYER_IDS)
def layer_case(request):
    cfg = request.param
    inp = R.layer_inputs(*cfg)
    return cfg, inp, R.layer_ref64(inp, cfg[1], cfg[4])


def test_routing_filter_keeps_enough_tokens(layer_case):
    (E, top_k, n_embd, n_inner, act, bias, dead), inp, ref = layer_case
    print("KEPT", inp["n_kept"], "of", R.LAYER_CANDIDATES)
    assert inp["n_kept"] >= R.LAYER_T
    assert inp["h"].shape == (R.LAYER_T, n_embd)
    lg = ref["logits"]
    assert lg.abs().max() <= R.MAX_LOGIT
    top = lg.sort(dim=-1, descending=True).values
    assert (top[:, top_k - 1] - top[:, top_k]).min() >= R.MIN_GAP
    # logits rounded to bf16 (what the layer's gate returns) pick the same sets
    assert torch.equal(R.expert_sets(lg.to(R.BF16), top_k), R.expert_sets(lg, top_k))
    if dead is not None:
        assert not R.expert_sets(lg, top_k)[:, dead].any()
        assert not ref["fc_w"][dead].any() and not ref["proj_w"][dead].any()
        # every other expert is used
        assert R.expert_sets(lg, top_k).any(0).sum() == E - 1


def test_layer_reference_vs_module_float64(layer_case):
    (E, top_k, n_embd, n_inner, act, bias, dead), inp, ref = layer_case
    layer = R.build_sparse_moe(inp, E, top_k, n_embd, n_inner, act, bias, torch.float64)
    h = inp["h"].double().requires_grad_(True)
    out, logits = layer(h)
    out.backward(inp["dout"].double())
    torch.testing.assert_close(logits, ref["logits"], rtol=1e-12, atol=1e-12)
    got = dict(R.layer_grads(layer, h), out=out)
    assert set(got) == set(ref) - {"logits"}
    # The module's softmax over the k chosen logits is fp32 by design even
    # here (`.float()`), forward and backward; all else is float64. A gate
    # then carries a few fp32 roundings (2^-24 each) and everything is linear
    # in the gates, so 2e-6 of each tensor's largest magnitude bounds it.
    for k, v in got.items():
        err = R.rel_err(v, ref[k])
        print(f"RELERR {k} {err:.3e}")
        assert err <= 2e-6, (k, err)
