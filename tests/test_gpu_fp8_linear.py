"""fp8 (e4m3) weight-only linear on hardware: the skinny-GEMM kernel against a
float64 reference built from the same quantised weight.

Shapes sit on the kernel's edges: M on both sides of the 16-row block and at
its 64-row limit, N = 24 / 200 (no multiple of the 16-channel slab, 200 not of
the 64-channel workgroup either), K = 48 / 320 (a partial 64-chunk, a partial
256-tile), K = 2560 (several tiles per split, default split count > 1), and a
forced 3-way split on every K (K = 48 and 64 leave splits without any k).

Tolerance (derived): e4m3 -> bf16 and the bf16 products are exact, so the
error is the fp32 accumulation of K terms in some order, one fp32 multiply,
one fp32 add, and the rounding to bf16:
    |y - ref| <= 2^-8 |ref| + K 2^-23 S,   S = sum_k |x_k wq_k| scale + |bias|.
"""

import functools

import pytest
import torch

from dolomite_engine_amd.ops import functional as Fx
from dolomite_engine_amd.ops import hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _check_env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


MS = [1, 3, 16, 17, 64]
NKS = [(16, 64), (24, 48), (200, 320), (272, 2560)]


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """Inputs from a fixed seed (weight rows spread over four orders of
    magnitude) and the float64 pieces of the reference, on the CPU."""
    g = torch.Generator().manual_seed(1000 * M + N + K)
    w = torch.randn(N, K, generator=g) * 10.0 ** (torch.rand(N, 1, generator=g) * 4 - 2)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    bias = torch.randn(N, generator=g).to(torch.bfloat16)
    wq, scale = Fx.quantize_weight_e4m3(w)
    wd = wq.double() * scale.double()[:, None]
    return x, wq, scale, bias, x.double() @ wd.T, x.double().abs() @ wd.abs().T


def _assert_close(y, M, N, K, with_bias):
    _, _, _, bias, ref, S = _case(M, N, K)
    if with_bias:
        ref, S = ref + bias.double(), S + bias.double().abs()
    err = (y.double().cpu() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * S
    print(f"max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("num_splits", [None, 3])
@pytest.mark.parametrize("N,K", NKS)
@pytest.mark.parametrize("M", MS)
def test_fp8_linear_matches_float64(M, N, K, num_splits, with_bias):
    x, wq, scale, bias, _, _ = _case(M, N, K)
    y = Fx.fp8_linear(x.cuda(), wq.cuda(), scale.cuda(), bias.cuda() if with_bias else None, num_splits=num_splits)
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    _assert_close(y, M, N, K, with_bias)


@pytest.mark.parametrize("M", MS)
def test_default_split_count_exceeds_one_at_k2560(M):
    assert Fx.fp8_linear_num_splits(M, 272, 2560) > 1


def test_row_strided_view():
    M, N, K = 17, 200, 320
    x, wq, scale, bias, _, _ = _case(M, N, K)
    base = torch.full((M, 2, K), float("nan"), dtype=torch.bfloat16, device="cuda")
    base[:, 0] = x.cuda()
    view = base[:, 0]
    assert view.stride() == (2 * K, 1)
    _assert_close(Fx.fp8_linear(view, wq.cuda(), scale.cuda(), bias.cuda()), M, N, K, True)


@pytest.mark.parametrize("num_splits", [1, 2])
@pytest.mark.parametrize("K", [64, 128])
def test_small_integers_are_exact(K, num_splits):
    """Integer x and weights with power-of-two row scales: every partial sum
    and the result are representable, so the k permutation, the row guards and
    the split join are pinned bit for bit. K = 128 gives both splits k."""
    M, N = 5, 40
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-2, 3, (M, K), generator=g).to(torch.bfloat16)
    wq = torch.randint(-2, 3, (N, K), generator=g).float().to(Fx.FP8_KV_DTYPE)
    scale = 2.0 ** torch.randint(-6, 7, (N,), generator=g).float()
    ref = (x.double() @ (wq.double() * scale.double()[:, None]).T).to(torch.bfloat16)
    y = Fx.fp8_linear(x.cuda(), wq.cuda(), scale.cuda(), num_splits=num_splits)
    assert torch.equal(y.cpu(), ref)


def test_forced_split_is_reproducible():
    x, wq, scale, bias = (t.cuda() for t in _case(17, 272, 2560)[:4])
    a =Fx.fp8_linear(x, wq, scale, bias, num_splits=3)
    b = Fx.fp8_linear(x, wq, scale, bias, num_splits=3)
    assert torch.equal(a, b)


def test_abi_rejects_65_rows():
    x = torch.zeros(65, 64, dtype=torch.bfloat16, device="cuda")
    wq = torch.zeros(16, 64, device="cuda").to(Fx.FP8_KV_DTYPE)
    scale = torch.ones(16, device="cuda")
    y = torch.empty(65, 16, dtype=torch.bfloat16, device="cuda")
    ret = hip.lib().dolomite_fp8_linear(hip.stream(), hip.ptr(x), hip.ptr(wq), hip.ptr(scale), hip.ptr(None),
                                        hip.ptr(y), hip.ptr(None), 65, 16, 64, 64, 1, hip.BF16)
    assert ret == 9071


@pytest.mark.parametrize("M,K,dtype", [(65, 64, torch.bfloat16), (3, 40, torch.bfloat16), (3, 64, torch.float32)],
                         ids=["M65", "K40", "fp32"])
def test_dequantised_route(M, K, dtype):
    """More than 64 rows, K % 16 != 0 and fp32 x take the documented
    dequantised route and still match the reference (fp32 x: to fp32 accuracy,
    well inside the bf16 bound)."""
    N = 24
    g = torch.Generator().manual_seed(11)
    x = torch.randn(M, K, generator=g).to(dtype)
    wq, scale = Fx.quantize_weight_e4m3(torch.randn(N, K, generator=g))
    wd = wq.double() * scale.double()[:, None]
    ref, S = x.double() @ wd.T, x.double().abs() @ wd.abs().T
    y = Fx.fp8_linear(x.cuda(), wq.cuda(), scale.cuda())
    assert y.dtype == dtype
    # bf16: scale and the dequantised weight are each rounded to bf16 before the GEMM, 2^-9 relative
    # apiece on every term: (1 + 2^-9)^2 - 1 < 2^-7
    slack = 2.0 ** -7 * S if dtype == torch.bfloat16 else 0.0
    assert bool(((y.double().cpu() - ref).abs() <= 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * S + slack).all())


# --- model: quantised linears under the KV cache ----------------------------------------


def _model():
    from dolomite_engine_amd.hf_models import GPTDolomiteConfig, GPTDolomiteForCausalLM, quantize_linears_fp8

    torch.manual_seed(5)
    cfg = GPTDolomiteConfig(
        vocab_size=512, n_positions=256, n_embd=320, n_layer=2, n_head=4,
        attention_head_type="mqa", n_inner=512,
        activation_function="swiglu", normalization_function="rmsnorm",
        position_embedding_type="rope", resid_pdrop=0.0, embd_pdrop=0.0,
        attn_pdrop=0.0, tie_word_embeddings=False,
    )
    cfg._attn_implementation = "flash_attention_2"
    return quantize_linears_fp8(GPTDolomiteForCausalLM(cfg).to(torch.bfloat16).cuda().eval())


def _left_padded(seqs):
    S = max(len(s) for s in seqs)
    ids = torch.zeros(len(seqs), S, dtype=torch.long)
    mask = torch.zeros(len(seqs), S, dtype=torch.long)
    pos = torch.zeros(len(seqs), S, dtype=torch.long)
    for b, s in enumerate(seqs):
        ids[b, S - len(s):] = torch.tensor(s)
        mask[b, S - len(s):] = 1
        pos[b, S - len(s):] = torch.arange(len(s))
    return ids.cuda(), mask.cuda(), pos.cuda()


def test_quantised_model_cached_logits_match_recompute():
    """Prefill + 4 decode steps (3 rows each: the kernel) against no-cache
    forwards of the grown batch (3 * 71+ rows: the dequantised route) on the
    same quantised weights, at the project's bf16 logits gate."""
    model = _model()
    g = torch.Generator().manual_seed(9)
    seqs = [torch.randint(0, 512, (n,), generator=g).tolist() for n in (70, 1, 33)]
    feed = torch.randint(0, 512, (4, 3), generator=g)
    with torch.no_grad():
        ids, mask, pos = _left_padded(seqs)
        cache = model(input_ids=ids, attention_mask=mask, position_ids=pos, use_cache=True).past_key_values
        for step in range(4):
            for b in range(3):
                seqs[b].append(int(feed[step, b]))
            out = model(input_ids=feed[step].cuda()[:, None], past_key_values=cache, use_cache=True)
            ids, mask, pos = _left_padded(seqs)
            want = model(input_ids=ids, attention_mask=mask, position_ids=pos).logits[:, -1].float()
            got = out.logits[:, 0].float()
            print(f"step {step}: max|cached - recomputed logits| {float((got - want).abs().max()):.4e}")
            torch.testing.assert_close(got, want, rtol=1e-2, atol=2e-2)
    assert cache.get_seq_length() == 74


def test_quantised_generate_is_reproducible():
    model = _model()
    g = torch.Generator().manual_seed(4)
    ids, mask, _ = _left_padded([torch.randint(0, 512, (n,), generator=g).tolist() for n in (20, 3, 11)])
    a = model.generate(ids, attention_mask=mask, max_new_tokens=12)
    b = model.generate(ids, attention_mask=mask, max_new_tokens=12)
    assert a.shape == (3, 32) and torch.equal(a, b)
