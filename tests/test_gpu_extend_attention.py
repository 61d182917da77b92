"""Extend attention (several new tokens over the KV cache) on hardware.

Shapes sit on the kernel's edges: n * G on both sides of the 128-column
workgroup tile (43 * 3 = 129, 5 * 32 = 160), a 16-column block that straddles
queries (G = 3), past + n on both sides of the 64-key tile and of every split
boundary (max_len = 200: chunk = 256 / 128 / 128 / 64 keys for nsplit =
1 / 2 / 3 / 5, so 3 and 5 have splits without keys), n = 0, spans left- and
right-aligned in their rows. Everything behind a sequence's cache_len is NaN.

Measured on an MI355X (printed by the tests): see DESIGN.md §7.
"""

import math

import pytest
import torch

from dolomite_engine_amd.hf_models import KVCache
from dolomite_engine_amd.ops import functional as Fx
from dolomite_engine_amd.ops import hip
from dolomite_engine_amd.ops.functional import QKVLayout
from tests.test_gpu_decode_attention import MODELS, _model, _padded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _check_env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


LAYOUTS = [("mha", 4, 4, 64), ("gqa", 6, 2, 80), ("mqa", 32, 1, 128), ("gqa", 16, 2, 80)]
_IDS = [f"{t}-H{h}-Hkv{j}-D{d}" for t, h, j, d in LAYOUTS]
PAST_N = [(0, 43), (1, 5), (63, 1), (64, 17), (65, 2), (127, 0), (129, 43), (0, 1), (63, 17), (127, 5), (129, 2)]
S, S_CAP, MAX_LEN, MAX_NEW = 48, 256, 200, 43
NSPLITS = [1, 2, 3, 5]
TOL = dict(rtol=2e-2, atol=2e-2)  # the decode test's bound


def _spans(ns, device="cuda"):
    """Row spans of len(ns) sequences in a (B*S) buffer, alternately left- and right-aligned."""
    begin = [b * S if b % 2 == 0 else (b + 1) * S - n for b, n in enumerate(ns)]
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=device)
    return begin, i32(begin), i32([s + n for s, n in zip(begin, ns)])


def _inputs(lo, past_n, seed):
    g = torch.Generator().manual_seed(seed)
    B = len(past_n)
    qkv = (torch.randn(B * S, lo.row_len, generator=g) * 0.7).to(torch.bfloat16)
    k = (torch.randn(B, S_CAP, lo.Hkv, lo.D, generator=g) * 0.7).to(torch.bfloat16)
    v = (torch.randn(B, S_CAP, lo.Hkv, lo.D, generator=g) * 0.7).to(torch.bfloat16)
    for b, (past, n) in enumerate(past_n):
        k[b, past + n :] = float("nan")
        v[b, past + n :] = float("nan")
    return qkv, k, v


def _ref64(qkv, k, v, begin, past_n, lo, scale):
    """float64 softmax attention with the bottom-right causal mask, from the same bf16 inputs."""
    q, _, _ = lo.unpack_cpu(qkv)
    o = torch.zeros(qkv.shape[0], lo.H, lo.D, dtype=torch.float64)
    for b, (past, n) in enumerate(past_n):
        if n == 0:
            continue
        kk = k[b, : past + n].double().repeat_interleave(lo.G, dim=1)
        vv = v[b, : past + n].double().repeat_interleave(lo.G, dim=1)
        sc = torch.einsum("ihd,khd->hik", q[begin[b] : begin[b] + n].double(), kk) * scale
        hidden = torch.arange(past + n)[None, :] > past + torch.arange(n)[:, None]
        o[begin[b] : begin[b] + n] = torch.einsum("hik,khd->ihd", torch.softmax(sc.masked_fill(hidden, -math.inf), -1), vv)
    return o


def _extend(lo, qkv, sb, se, k, v, past_n, scale, nsplit, max_new=MAX_NEW):
    lens = torch.tensor([p + n for p, n in past_n], dtype=torch.int32, device="cuda")
    with torch.no_grad():
        return Fx.extend_attention(qkv, lo, sb, se, max_new, k, v, lens, scale, MAX_LEN, num_splits=nsplit)


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture(scope="module", params=LAYOUTS, ids=_IDS)
def random_case(request):
    """Inputs and the float64 reference, computed once per layout."""
    head_type, H, Hkv, D = request.param
    lo = QKVLayout.make(H, Hkv, D, head_type)
    qkv, k, v = _inputs(lo, PAST_N, 11)
    begin, sb, se = _spans([n for _, n in PAST_N])
    scale = 1.0 / math.sqrt(D)
    return lo, scale, (qkv.cuda(), sb, se, k.cuda(), v.cuda()), begin, _ref64(qkv, k, v, begin, PAST_N, lo, scale)


@pytest.mark.parametrize("nsplit", NSPLITS)
def test_extend_matches_float64(random_case, nsplit):
    lo, scale, dev, begin, ref = random_case
    o = _extend(lo, *dev, PAST_N, scale, nsplit)
    o2 = _extend(lo, *dev, PAST_N, scale, nsplit)
    torch.cuda.synchronize()
    assert o.shape == (len(PAST_N) * S, lo.H * lo.D) and o.dtype == torch.bfloat16
    assert not torch.isnan(o).any(), "NaN leaked from behind cache_len"
    got = o.cpu().double().view(-1, lo.H, lo.D)
    print(f"nsplit {nsplit}: max|o - ref64| {float((got - ref).abs().max()):.4e}")
    torch.testing.assert_close(got, ref, **TOL)
    gap = torch.ones(o.shape[0], dtype=torch.bool)
    for b, (_, n) in enumerate(PAST_N):
        gap[begin[b] : begin[b] + n] = False
    assert gap.sum() > 0 and not _bits(o.cpu())[gap].any(), "gap rows and n = 0 rows: +0"
    assert torch.equal(_bits(o), _bits(o2)), "not reproducible run to run"
    if nsplit == 1:  # the default rule: ceil(4 tiles / 4) = 1 split
        assert Fx.extend_num_splits(len(PAST_N), lo, MAX_NEW, MAX_LEN) == 1
        assert torch.equal(_bits(_extend(lo, *dev, PAST_N, scale, None)), _bits(o))


@pytest.mark.parametrize("head_type,H,Hkv,D", LAYOUTS, ids=_IDS)
def test_empty_cache_first_row_is_v0_and_matches_span_attention(head_type, H, Hkv, D):
    """past = 0: query 0 sees exactly key 0, so its output IS v[0], bitwise —
    one key more or less breaks it — and the whole result is the forward
    kernel's over the same rows."""
    lo = QKVLayout.make(H, Hkv, D, head_type)
    past_n = [(0, 43), (0, 1), (0, 17), (0, 5)]
    qkv, k, v = _inputs(lo, [(0, 0)] * 4, 5)   # caches all NaN: filled by the append
    begin, sb, se = _spans([n for _, n in past_n])
    qkv, k, v = qkv.cuda(), k.cuda(), v.cuda()
    scale = 1.0 / math.sqrt(D)
    with torch.no_grad():
        Fx.kv_cache_append(qkv, lo, sb, se, k, v, torch.zeros(4, dtype=torch.int32, device="cuda"))
        o_span = Fx.span_attention(qkv, sb, se, 43, lo, scale)
    for nsplit in (1, 3):
        o = _extend(lo, qkv, sb, se, k, v, past_n, scale, nsplit)
        want = v[:, 0].repeat_interleave(lo.G, dim=1).reshape(4, H * D)
        assert torch.equal(_bits(o[begin]), _bits(want))
        torch.testing.assert_close(o.float(), o_span.float(), **TOL)


@pytest.mark.parametrize("head_type,H,Hkv,D", LAYOUTS, ids=_IDS)
def test_one_token_matches_decode_attention(head_type, H, Hkv, D):
    lo = QKVLayout.make(H, Hkv, D, head_type)
    past_n = [(p, 1) for p in (0, 1, 63, 64, 65, 127, 129)]
    qkv, k, v = _inputs(lo, past_n, 7)
    begin, sb, se = _spans([1] * len(past_n))
    qkv, k, v = qkv.cuda(), k.cuda(), v.cuda()
    scale = 1.0 / math.sqrt(D)
    lens = torch.tensor([p + 1 for p, _ in past_n], dtype=torch.int32, device="cuda")
    with torch.no_grad():
        o_dec = Fx.decode_attention(qkv[begin], lo, k, v, lens, scale, MAX_LEN, num_splits=1)
    for nsplit in (1, 2):
        o = _extend(lo, qkv, sb, se, k, v, past_n, scale, nsplit, max_new=1)
        torch.testing.assert_close(o[begin].float(), o_dec.float(), **TOL)


def test_error_codes():
    L = hip.lib()
    lo = QKVLayout.make(4, 2, 64, "gqa")
    qkv = torch.zeros(4, lo.row_len, dtype=torch.bfloat16, device="cuda")
    k = torch.zeros(2, 8, 2, 64, dtype=torch.bfloat16, device="cuda")
    i32 = torch.zeros(2, dtype=torch.int32, device="cuda")
    o = torch.full((4, 4 * 64), 7.0, dtype=torch.bfloat16, device="cuda")

    def extend(D=64, H=4, scale=0.125, nsplit=1, dtype=hip.BF16, batch=2, row=lo.row_len):
        return L.dolomite_fa_extend(
            hip.stream(), hip.ptr(qkv), hip.ptr(k), hip.ptr(k), hip.ptr(o), hip.ptr(None), hip.ptr(i32),
            hip.ptr(i32), hip.ptr(i32), batch, 2, 4, H, 2, D, 2, 8, nsplit, row, lo.q_gstride,
            k.stride(0), k.stride(1), k.stride(2), k.stride(0), k.stride(1), k.stride(2), scale, dtype)

    codes = [extend(dtype=hip.F32), extend(D=136), extend(scale=0.0), extend(scale=float("nan")), extend(D=60),
             extend(row=lo.row_len + 4), extend(H=6), extend(batch=-1), extend(nsplit=0), extend(nsplit=2)]
    assert codes == [9010, 9011, 9015, 9015, 9041, 9041, 9042, 9042, 9043, 9044]
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()), "an argument error launched something"
    assert extend() == 0 and bool((o == 0).all())   # two empty spans: every row is a gap row
    assert L.dolomite_fa_extend_scratch_floats(2, 5, 4, 64, 3) == 2 * 5 * 4 * 3 * 66
    assert L.dolomite_fa_extend_scratch_floats(2, 5, 4, 64, 1) == 0
    assert L.dolomite_fa_extend_scratch_floats(2, 5, 4, 64, 0) == -1


# ---------------------------------------------------------------------------
# the model on hardware
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module", params=MODELS, ids=[f"{t}-D{d}" for t, _, _, d in MODELS])
def model_case(request):
    """A 2-layer bf16 model, a left-padded 13-column batch (lengths 13 / 1 / 6)
    and the unchunked cached run: prefill logits, then 4 decode steps."""
    model = _model(*request.param)
    g = torch.Generator().manual_seed(9)
    ids, mask, _ = _padded([torch.randint(0, 512, (n,), generator=g).tolist() for n in (13, 1, 6)], "left")
    feed = torch.randint(0, 512, (3, 4), generator=g).cuda()
    with torch.no_grad():
        out = model(input_ids=ids, attention_mask=mask, use_cache=True)
        steps = [model(input_ids=feed[:, t : t + 1], past_key_values=out.past_key_values).logits[:, 0].float()
                 for t in range(4)]
    return model, ids, mask, feed, out.logits.float(), torch.stack(steps, dim=1)


def _fresh_cache(model):
    return KVCache(model.config, 3, 32, torch.bfloat16, "cuda", multi_token=True)


def test_model_chunked_prefill_then_decode(model_case):
    model, ids, mask, feed, prefill, steps = model_case
    cache, worst = _fresh_cache(model), 0.0
    real = mask.bool()
    with torch.no_grad():
        for a in range(0, 13, 5):
            e = min(a + 5, 13)
            pos = torch.arange(a, e, device="cuda").expand(3, -1)
            got = model(input_ids=ids[:, a:e], attention_mask=mask[:, a:e], position_ids=pos,
                        past_key_values=cache).logits.float()
            worst = max(worst, float((got - prefill[:, a:e])[real[:, a:e]].abs().max()))
            torch.testing.assert_close(got[real[:, a:e]], prefill[:, a:e][real[:, a:e]], rtol=1e-2, atol=2e-2)
        assert cache.lengths.tolist() == [13, 1, 6] and cache.get_seq_length() == 13
        for t in range(3):
            got = model(input_ids=feed[:, t : t + 1], past_key_values=cache).logits[:, 0].float()
            worst = max(worst, float((got - steps[:, t]).abs().max()))
            torch.testing.assert_close(got, steps[:, t], rtol=1e-2, atol=2e-2)
    print(f"max|chunked - unchunked logits| {worst:.4e}")


def test_model_verify_step_matches_decode_steps(model_case):
    model, ids, mask, feed, _, steps = model_case
    cache = _fresh_cache(model)
    with torch.no_grad():
        model(input_ids=ids, attention_mask=mask, past_key_values=cache)
        got = model(input_ids=feed, past_key_values=cache).logits.float()
    print(f"max|verify - decode logits| {float((got - steps).abs().max()):.4e}")
    torch.testing.assert_close(got, steps, rtol=1e-2, atol=2e-2)
    assert cache.lengths.tolist() == [17, 5, 10]
