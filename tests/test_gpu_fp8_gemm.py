"""fp8 (e4m3) weight-only linear above 64 rows on hardware: the tiled GEMM
kernel (128-row x 128-channel tiles, 128-wide k tiles) through ops.fp8_linear
against a float64 reference built from the same quantised weight.

Shapes sit on the kernel's edges: M = 65 (first served row count, half a
tile's rows empty), 128 / 129 (both sides of the row tile), 300 (three row
tiles, the last partial); N = 16 / 24 / 200 / 272 (below a tile, off the
16-channel block, a partial second tile, a partial third tile); K = 48 / 64
(less than one k tile, k = 48 not a multiple of a 64-chunk), 320 (a partial
third k tile), 2560 (twenty k tiles, default split count > 1); a forced
3-way split on every K (K = 48 and 64 leave splits without any k).

Tolerance (derived, tests/test_gpu_fp8_linear.py): the conversion and the
products are exact, so the error is the fp32 accumulation of K terms in some
order, one fp32 multiply, one fp32 add, and the rounding to bf16:
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


MS = [65, 128, 129, 300]
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
def test_fp8_gemm_matches_float64(M, N, K, num_splits, with_bias):
    x, wq, scale, bias, _, _ = _case(M, N, K)
    y = Fx.fp8_linear(x.cuda(), wq.cuda(), scale.cuda(), bias.cuda() if with_bias else None, num_splits=num_splits)
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    _assert_close(y, M, N, K, with_bias)


def test_default_split_count_exceeds_one_at_k2560():
    assert Fx.fp8_gemm_num_splits(128, 272, 2560) > 1


def test_row_strided_view():
    M, N, K = 129, 200, 320
    x, wq, scale, bias, _, _ = _case(M, N, K)
    base = torch.full((M, 2, K), float("nan"), dtype=torch.bfloat16, device="cuda")
    base[:, 0] = x.cuda()
    view = base[:, 0]
    assert view.stride() == (2 * K, 1)
    _assert_close(Fx.fp8_linear(view, wq.cuda(), scale.cuda(), bias.cuda()), M, N, K, True)


@pytest.mark.parametrize("num_splits", [1, 2])
@pytest.mark.parametrize("K", [64, 128])
@pytest.mark.parametrize("M", [70, 130])
def test_small_integers_are_exact(M, K, num_splits):
    """Integer x and weights with power-of-two row scales: every partial sum
    and the result are representable, so the k permutation, the row guards and
    the split join are pinned bit for bit."""
    N = 40
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-2, 3, (M, K), generator=g).to(torch.bfloat16)
    wq = torch.randint(-2, 3, (N, K), generator=g).float().to(Fx.FP8_KV_DTYPE)
    scale = 2.0 ** torch.randint(-6, 7, (N,), generator=g).float()
    ref = (x.double() @ (wq.double() * scale.double()[:, None]).T).to(torch.bfloat16)
    y = Fx.fp8_linear(x.cuda(), wq.cuda(), scale.cuda(), num_splits=num_splits)
    assert torch.equal(y.cpu(), ref)


def test_forced_split_is_reproducible():
    x, wq, scale, bias = (t.cuda() for t in _case(129, 272, 2560)[:4])
    a = Fx.fp8_linear(x, wq, scale, bias, num_splits=3)
    b = Fx.fp8_linear(x, wq, scale, bias, num_splits=3)
    assert torch.equal(a, b)


@pytest.mark.parametrize("M,K,code", [(0, 64, 9080), (70, 40, 9082)], ids=["M0", "K40"])
def test_abi_error_codes(M, K, code):
    x = torch.zeros(max(M, 1), K, dtype=torch.bfloat16, device="cuda")
    wq = torch.zeros(16, K, device="cuda").to(Fx.FP8_KV_DTYPE)
    scale = torch.ones(16, device="cuda")
    y = torch.empty(max(M, 1), 16, dtype=torch.bfloat16, device="cuda")
    ret = hip.lib().dolomite_fp8_gemm(hip.stream(), hip.ptr(x), hip.ptr(wq), hip.ptr(scale), hip.ptr(None),
                                      hip.ptr(y), hip.ptr(None), M, 16, K, K, 1, hip.BF16)
    assert ret == code


def test_quantised_model_chunked_prefill_matches_one_shot():
    """B = 3 prompts of 96 tokens prefilled in chunks of 32 (96 rows per
    linear call: the tiled kernel under the extend attention) against the
    one-shot forward (288 rows), last-position logits at the project's bf16
    logits gate."""
    from dolomite_engine_amd.hf_models import KVCache

    from tests.test_gpu_fp8_linear import _model

    model = _model()
    ids = torch.randint(0, 512, (3, 96), generator=torch.Generator().manual_seed(6)).cuda()
    with torch.no_grad():
        want = model(input_ids=ids).logits[:, -1].float()
        cache = KVCache(model.config, 3, 96, torch.bfloat16, "cuda", multi_token=True)
        for a in range(0, 96, 32):
            out = model(input_ids=ids[:, a:a + 32], past_key_values=cache, use_cache=True)
    got = out.logits[:, -1].float()
    print(f"max|chunked - one-shot logits| {float((got - want).abs().max()):.4e}")
    torch.testing.assert_close(got, want, rtol=1e-2, atol=2e-2)
