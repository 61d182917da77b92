"""Extend attention over the fp8 (e4m3) KV cache on hardware.

The shapes are test_gpu_extend_attention.py's edge set (n * G on both sides of
the 128-column tile, past + n on both sides of the 64-key tile and of every
split boundary, splits without keys, n = 0, spans left- and right-aligned)
plus D = 40, where an 8-byte piece is the widest that stays inside a row.
S_CAP = 250 is no multiple of 4 or 64: a row or scale read past max_len leaves
the last sequence's arrays. Behind every cache_len the cache holds 0xff bytes
(an e4m3 NaN) and NaN scales; per-key magnitudes make a neighbouring key's
scale wrong by 1.5x .. 7x.

The quantisation sits on both sides of every comparison (the reference attends
q8 * scale in float64), so the error sources are the bf16 extend kernel's —
bf16 P, fp32 accumulation, a bf16 output — and so is the tolerance.

Measured on an MI355X (printed by the tests): see DESIGN.md §7.
"""

import math

import pytest
import torch

from dolomite_engine_amd.ops import functional as Fx
from dolomite_engine_amd.ops import hip
from dolomite_engine_amd.ops.functional import QKVLayout
from tests.test_gpu_decode_fp8 import _dequant64, _poison_tail, _quantize_cache
from tests.test_gpu_extend_attention import MAX_LEN, MAX_NEW, NSPLITS, PAST_N, S, TOL, _bits, _ref64, _spans

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _check_env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


LAYOUTS = [("mha", 4, 4, 64), ("gqa", 6, 2, 80), ("mqa", 32, 1, 128), ("gqa", 4, 2, 40)]
_IDS = [f"{t}-H{h}-Hkv{j}-D{d}" for t, h, j, d in LAYOUTS]
S_CAP = 250


def _case(lo, past_n, seed):
    """bf16 qkv rows, a quantised cache poisoned behind every cache_len (on
    the device) and the float64 dequantised K, V the reference attends."""
    g = torch.Generator().manual_seed(seed)
    B = len(past_n)
    key = torch.arange(S_CAP)[None, :, None, None]
    qkv = (torch.randn(B * S, lo.row_len, generator=g) * 0.7).to(torch.bfloat16)
    k = (torch.randn(B, S_CAP, lo.Hkv, lo.D, generator=g) * 0.7 * (0.5 + 0.5 * (key % 3))).to(torch.bfloat16)
    v = (torch.randn(B, S_CAP, lo.Hkv, lo.D, generator=g) * 0.7 * (1 + key % 7)).to(torch.bfloat16)
    (k8, ks), (v8, vs) = _quantize_cache(k), _quantize_cache(v)
    kd, vd = _dequant64(k8, ks), _dequant64(v8, vs)
    lens = [p + n for p, n in past_n]
    dev = dict(zip(("k", "ks", "v", "vs"), (t.cuda() for t in (*_poison_tail(k8, ks, lens), *_poison_tail(v8, vs, lens)))))
    dev["lens"] = torch.tensor(lens, dtype=torch.int32, device="cuda")
    return qkv, dev, kd, vd


def _extend(lo, qkv, sb, se, dev, scale, nsplit, max_new=MAX_NEW):
    with torch.no_grad():
        return Fx.extend_attention(qkv, lo, sb, se, max_new, dev["k"], dev["v"], dev["lens"], scale, MAX_LEN,
                                   num_splits=nsplit, k_scale=dev["ks"], v_scale=dev["vs"])


@pytest.fixture(scope="module", params=LAYOUTS, ids=_IDS)
def random_case(request):
    """Inputs and the float64 reference over the dequantised cache, once per layout."""
    head_type, H, Hkv, D = request.param
    lo = QKVLayout.make(H, Hkv, D, head_type)
    qkv, dev, kd, vd = _case(lo, PAST_N, 11)
    begin, sb, se = _spans([n for _, n in PAST_N])
    scale = 1.0 / math.sqrt(D)
    return lo, scale, (qkv.cuda(), sb, se, dev), begin, _ref64(qkv, kd, vd, begin, PAST_N, lo, scale)


@pytest.mark.parametrize("nsplit", NSPLITS)
def test_extend_fp8_matches_float64(random_case, nsplit):
    lo, scale, args, begin, ref = random_case
    o = _extend(lo, *args, scale, nsplit)
    o2 = _extend(lo, *args, scale, nsplit)
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
    if nsplit == Fx.extend_num_splits(len(PAST_N), lo, MAX_NEW, MAX_LEN):   # the rule: ceil(4 tiles / 4) = 1 split
        assert nsplit == 1 and torch.equal(_bits(_extend(lo, *args, scale, None)), _bits(o))


@pytest.mark.parametrize("head_type,H,Hkv,D", LAYOUTS, ids=_IDS)
def test_one_token_matches_decode_fp8(head_type, H, Hkv, D):
    lo = QKVLayout.make(H, Hkv, D, head_type)
    past_n = [(p, 1) for p in (0, 1, 63, 64, 65, 127, 129)]
    qkv, dev, _, _ = _case(lo, past_n, 7)
    begin, sb, se = _spans([1] * len(past_n))
    qkv = qkv.cuda()
    scale = 1.0 / math.sqrt(D)
    with torch.no_grad():
        o_dec = Fx.decode_attention(qkv[begin], lo, dev["k"], dev["v"], dev["lens"], scale, MAX_LEN, num_splits=1,
                                    k_scale=dev["ks"], v_scale=dev["vs"])
    for nsplit in (1, 2):
        o = _extend(lo, qkv, sb, se, dev, scale, nsplit, max_new=1)
        torch.testing.assert_close(o[begin].float(), o_dec.float(), **TOL)


@pytest.mark.parametrize("head_type,H,Hkv,D", LAYOUTS, ids=_IDS)
def test_append_then_extend(head_type, H, Hkv, D):
    """Sequence b's rows [b*192, b*192 + past + n) of one qkv buffer are its
    history and its new tokens: the history is appended at 0, the new rows at
    dst_pos = past, into a cache of 0xff bytes and NaN scales; the reference
    attends quantize_kv_e4m3 of the same rows."""
    lo = QKVLayout.make(H, Hkv, D, head_type)
    past_n, R = [(0, 17), (63, 5), (129, 43)], 192
    g = torch.Generator().manual_seed(13)
    qkv = (torch.randn(3 * R, lo.row_len, generator=g) * 0.7).to(torch.bfloat16)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device="cuda")
    begin = [b * R + p for b, (p, _) in enumerate(past_n)]
    row0, sb, se = i32([0, R, 2 * R]), i32(begin), i32([s + n for s, (_, n) in zip(begin, past_n)])
    dev = dict(k=torch.full((3, S_CAP, Hkv, D), 0xFF, dtype=torch.uint8, device="cuda").view(Fx.FP8_KV_DTYPE),
               ks=torch.full((3, Hkv, S_CAP), float("nan"), device="cuda"),
               lens=i32([p + n for p, n in past_n]))
    dev["v"], dev["vs"] = dev["k"].clone(), dev["ks"].clone()
    qd = qkv.cuda()
    with torch.no_grad():
        for s0, s1, dst in ((row0, sb, torch.zeros_like(sb)), (sb, se, sb - row0)):
            Fx.kv_cache_append(qd, lo, s0, s1, dev["k"], dev["v"], dst, k_scale=dev["ks"], v_scale=dev["vs"])
    _, k, v = lo.unpack_cpu(qkv)
    kd, vd = (q8.double().mul(sc.double()[..., None]).view(3, R, Hkv, D) for q8, sc in map(Fx.quantize_kv_e4m3, (k, v)))
    scale = 1.0 / math.sqrt(D)
    ref = _ref64(qkv, kd, vd, begin, past_n, lo, scale)
    for nsplit in (1, 3):
        got = _extend(lo, qd, sb, se, dev, scale, nsplit).cpu().double().view(-1, H, D)
        assert not torch.isnan(got).any()
        print(f"nsplit {nsplit}: max|o - ref64| {float((got - ref).abs().max()):.4e}")
        torch.testing.assert_close(got, ref, **TOL)


def test_refusals_and_error_codes():
    lo = QKVLayout.make(4, 2, 64, "gqa")
    qkv = torch.zeros(4, lo.row_len, dtype=torch.bfloat16, device="cuda")
    k = torch.zeros(2, 8, 2, 64, dtype=Fx.FP8_KV_DTYPE, device="cuda")
    sc = torch.ones(2, 2, 8, device="cuda")
    i32 = torch.zeros(2, dtype=torch.int32, device="cuda")
    call = lambda q=qkv, **kw: Fx.extend_attention(q, lo, i32, i32, 2, k, k, i32, 0.125, 8, **kw)
    with torch.no_grad():
        for bad in (dict(), dict(k_scale=sc, v_scale=sc[..., :4])):
            with pytest.raises(ValueError):
                call(**bad)
        with pytest.raises(TypeError):
            call(qkv.float(), k_scale=sc, v_scale=sc)
        assert bool((call(k_scale=sc, v_scale=sc) == 0).all())   # two empty spans: every row is a gap row

    o = torch.full((4, 4 * 64), 7.0, dtype=torch.bfloat16, device="cuda")

    def extend(dtype=hip.BF16, ks=sc):
        return hip.lib().dolomite_fa_extend_fp8(
            hip.stream(), hip.ptr(qkv), hip.ptr(k), hip.ptr(k), hip.ptr(ks), hip.ptr(sc), hip.ptr(o), hip.ptr(None),
            hip.ptr(i32), hip.ptr(i32), hip.ptr(i32), 2, 2, 4, 4, 2, 64, 2, 8, 1, lo.row_len, lo.q_gstride,
            k.stride(0), k.stride(1), k.stride(2), k.stride(0), k.stride(1), k.stride(2),
            sc.stride(0), sc.stride(1), 0.125, dtype)

    assert [extend(dtype=hip.F32), extend(ks=None)] == [9010, 9045]
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()), "an argument error launched something"
