"""fp8 (e4m3) KV cache on hardware: the quantising append and the decode
kernel that reads it.

The shapes are test_gpu_decode_attention.py's (the 64-key wave tile, the
4-wave round-robin, splits without a key, G = 3 / 32 / 40) plus D = 40, where
an 8-byte piece is the widest that stays inside a row. S_CAP = 250 is no
multiple of 4 or 64: a scale or a cache row loaded past max_len would leave
the last sequence's arrays. Behind every cache_len the cache holds 0xff bytes
(an e4m3 NaN) and NaN scales.

The quantisation sits on both sides of every comparison (the reference
attends q8 * scale in float64), so the error sources are the bf16 decode
kernel's — bf16 P, fp32 accumulation, a bf16 output — and so is the tolerance.

Measured on an MI355X (printed by the tests): max|o - ref64| 4.5e-3 .. 9.3e-3
over the seven layouts, the same for every split count; append + decode
against the float64 reference 6.4e-4, against the bf16 cache's decode 5.9e-3.
"""

import math

import pytest
import torch

from dolomite_engine_amd.ops import functional as Fx
from dolomite_engine_amd.ops import hip
from dolomite_engine_amd.ops.functional import QKVLayout

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _check_env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


FP8 = torch.float8_e4m3fn
LAYOUTS = [
    ("mqa", 4, 1, 80), ("gqa", 4, 2, 128), ("mha", 2, 2, 64),
    ("gqa", 6, 2, 64),    # G = 3: padded head columns
    ("mqa", 32, 1, 80),   # two 16-head blocks
    ("mqa", 40, 1, 64),   # G > 32: a second head group on grid.z
    ("gqa", 4, 2, 40),    # 40-byte rows: 16-byte pieces would straddle them
]
_IDS = [f"{t}-H{h}-Hkv{j}-D{d}" for t, h, j, d in LAYOUTS]
CACHE_LEN = [1, 63, 64, 65, 127, 128, 129, 193, 200, 0]
S_CAP, MAX_LEN = 250, 200
NSPLITS = [1, 2, 3, 5]
TOL = dict(rtol=2e-2, atol=2e-2)  # the bf16 decode kernel's (test_gpu_decode_attention.py)


def _poison_tail(q8, scale, lens):
    """0xff bytes and NaN scales behind each sequence's length."""
    for b, n in enumerate(lens):
        q8.view(torch.uint8)[b, n:] = 0xFF
        scale[b, :, n:] = float("nan")
    return q8, scale


def _quantize_cache(x):
    """(B, S, Hkv, D) bf16 -> e4m3 cache and (B, Hkv, S) scales by the rule."""
    q8, scale = Fx.quantize_kv_e4m3(x)
    return q8, scale.transpose(1, 2).contiguous()


def _dequant64(q8, scale):
    return q8.double() * scale.double().transpose(1, 2).unsqueeze(-1)


def _ref64(q, k, v, lens, lo, scale):
    """float64 softmax attention; k, v (B, S, Hkv, D) float64, q (B, H, D)."""
    G = lo.H // lo.Hkv
    o = torch.zeros(q.shape[0], lo.H, lo.D, dtype=torch.float64)
    for b, n in enumerate(lens):
        for h in range(lo.H if n else 0):
            p = torch.softmax((k[b, :n, h // G] @ q[b, h].double()) * scale, dim=0)
            o[b, h] = p @ v[b, :n, h // G]
    return o


def _pack_q(q, lo):
    """(B, H, D) q into the q slots of packed rows whose K/V slots are NaN."""
    rows = torch.full((q.shape[0], lo.row_len), float("nan"), dtype=q.dtype)
    for h in range(lo.H):
        off = (h // lo.G) * lo.q_gstride + (h % lo.G) * lo.D
        rows[:, off : off + lo.D] = q[:, h]
    return rows


def _decode(qkv, lo, dev, scale, nsplit=None):
    with torch.no_grad():
        return Fx.decode_attention(qkv, lo, dev["k"], dev["v"], dev["lens"], scale, MAX_LEN, num_splits=nsplit,
                                   k_scale=dev["ks"], v_scale=dev["vs"])


def _to_dev(k8, ks, v8, vs):
    return dict(k=k8.cuda(), ks=ks.cuda(), v=v8.cuda(), vs=vs.cuda(),
                lens=torch.tensor(CACHE_LEN, dtype=torch.int32).cuda())


@pytest.fixture(scope="module", params=LAYOUTS, ids=_IDS)
def random_case(request):
    """Inputs and the float64 reference over the dequantised cache, once per layout."""
    head_type, H, Hkv, D = request.param
    lo = QKVLayout.make(H, Hkv, D, head_type)
    B = len(CACHE_LEN)
    g = torch.Generator().manual_seed(11)
    key = torch.arange(S_CAP)[None, :, None, None]
    q = (torch.randn(B, H, D, generator=g) * 0.7).to(torch.bfloat16)
    # row magnitudes differ key to key, so a scale from a neighbouring key is wrong by 1.5x .. 7x
    k = (torch.randn(B, S_CAP, Hkv, D, generator=g) * 0.7 * (0.5 + 0.5 * (key % 3))).to(torch.bfloat16)
    v = (torch.randn(B, S_CAP, Hkv, D, generator=g) * 0.7 * (1 + key % 7)).to(torch.bfloat16)
    k8, ks = _quantize_cache(k)
    v8, vs = _quantize_cache(v)
    scale = 1.0 / math.sqrt(D)
    ref = _ref64(q, _dequant64(k8, ks), _dequant64(v8, vs), CACHE_LEN, lo, scale)
    return lo, scale, _pack_q(q, lo).cuda(), _to_dev(*_poison_tail(k8, ks, CACHE_LEN), *_poison_tail(v8, vs, CACHE_LEN)), ref


@pytest.mark.parametrize("nsplit", NSPLITS)
def test_decode_fp8_matches_float64(random_case, nsplit):
    lo, scale, qkv, dev, ref = random_case
    o = _decode(qkv, lo, dev, scale, nsplit)
    o2 = _decode(qkv, lo, dev, scale, nsplit)
    torch.cuda.synchronize()
    assert o.shape == (len(CACHE_LEN), lo.H * lo.D) and o.dtype == torch.bfloat16
    assert not torch.isnan(o).any(), "NaN leaked from behind cache_len"
    got = o.cpu().double().view(-1, lo.H, lo.D)
    print(f"nsplit {nsplit}: max|o - ref64| {float((got - ref).abs().max()):.4e}")
    torch.testing.assert_close(got, ref, **TOL)
    empty = CACHE_LEN.index(0)
    assert torch.equal(o[empty].view(torch.int16), torch.zeros_like(o[empty]).view(torch.int16)), "empty cache: +0"
    assert torch.equal(o.view(torch.int16), o2.view(torch.int16)), "not reproducible run to run"


def _marker_candidates(n, H):
    """Key 0, the newest key, both sides of every tile / wave / split
    boundary, then filler so every head gets a key of its own."""
    edges = [0, n - 1, 63, 64, 127, 128, 191, 192]
    cand = []
    for p in edges + list(range(n)):
        if 0 <= p < n and p not in cand:
            cand.append(p)
        if len(cand) >= max(H, len(edges)):
            break
    return cand


@pytest.mark.parametrize("head_type,H,Hkv,D", LAYOUTS, ids=_IDS)
def test_decode_fp8_markers_exact(head_type, H, Hkv, D):
    """One dropped key, or a scale taken from the wrong key, among 200.
    V row p: v[p, 0] = 14 * 2^(p%3), v[p, 1+j] = bit_j(p) * 2^(p%3): its
    amax gives the scale 2^(p%3 - 5) exactly and it dequantises exactly, so a
    neighbour's scale is off by 2x or 4x. Head h's query is 20*e_h and one
    chosen key per head is 20*e_h (its row's amax: the K scale is 20/448, ten
    times its neighbours'), the other keys are zero in the first H dims. The
    chosen key leads by 400/sqrt(D) >= 35 nats, so where its V row is nonzero
    o must EQUAL it. Where the row is zero the other keys leave
    <= 200 * e^-35 * 56 < 1e-11 in the float64 reference and in any correct
    kernel — bf16 keeps such values, so there the test asks for |o| <= 1e-10
    (a wrong key or scale is off by >= 1)."""
    lo = QKVLayout.make(H, Hkv, D, head_type)
    assert D >= H and D >= 9
    B = len(CACHE_LEN)
    scale = 1.0 / math.sqrt(D)
    assert 400 * scale >= 35
    q = torch.zeros(B, H, D, dtype=torch.bfloat16)
    for h in range(H):
        q[:, h, h] = 20.0
    qkv = _pack_q(q, lo).cuda()
    p = torch.arange(S_CAP)
    vrow = torch.zeros(S_CAP, D)
    vrow[:, 0] = 14.0
    for j in range(8):
        vrow[:, 1 + j] = (p >> j) & 1
    vrow = vrow * (2.0 ** (p % 3))[:, None]
    v8, vs = _quantize_cache(vrow[None, :, None, :].expand(B, S_CAP, Hkv, D).to(torch.bfloat16))
    assert torch.equal(vs[0, 0], (2.0 ** (p % 3 - 5.0)).float()) and torch.equal(_dequant64(v8, vs)[0, :, 0], vrow.double())
    vdeq = _dequant64(v8, vs)
    v8, vs = _poison_tail(v8, vs, CACHE_LEN)
    g = torch.Generator().manual_seed(3)
    rounds = max(-(-len(_marker_candidates(n, H)) // H) for n in CACHE_LEN if n > 0)
    for r in range(rounds):
        k = (torch.randn(B, S_CAP, Hkv, D, generator=g) * 0.5).to(torch.bfloat16)
        k[..., :H] = 0
        want = torch.zeros(B, H, D)
        for b, n in enumerate(CACHE_LEN):
            if n == 0:
                continue
            cand = _marker_candidates(n, H)
            for h in range(H):
                key = cand[(r * H + h) % len(cand)]
                k[b, key, h // lo.G, h] = 20.0
                want[b, h] = vrow[key]
        k8, ks = _quantize_cache(k)
        ref = _ref64(q, _dequant64(k8, ks), vdeq, CACHE_LEN, lo, scale)
        assert float((ref - want.double()).abs().max()) < 1e-11
        dev = _to_dev(*_poison_tail(k8, ks, CACHE_LEN), v8, vs)
        for nsplit in NSPLITS:
            got = _decode(qkv, lo, dev, scale, nsplit).cpu().float().view(B, H, D)
            ok = torch.where(want != 0, got == want, got.abs() <= 1e-10)
            bad = (~ok).any(-1).nonzero().tolist()
            assert not bad, f"round {r} nsplit {nsplit}: wrong (sequence, head) {bad[:8]}"


# ---------------------------------------------------------------------------
# kv_cache_append into the fp8 cache
# ---------------------------------------------------------------------------

AB, AS, ACAP = 4, 40, 46
ALENS = [40, 1, 17, 0]
# D = 8 / 16 / 32: groups of 1 / 2 / 4 lanes; 40 and 80: 5 of 8 and 10 of 16 lanes
APPEND_LAYOUTS = LAYOUTS[:4] + [("gqa", 4, 2, 40), ("mqa", 4, 1, 8), ("mha", 2, 2, 16), ("gqa", 4, 2, 32)]


def _sentinel_cache(Hkv, D, device):
    k = torch.full((AB, ACAP, Hkv, D), 0xFF, dtype=torch.uint8, device=device).view(FP8)
    s = torch.full((AB, Hkv, ACAP), float("nan"), device=device)
    return k, s, k.clone(), s.clone()


@pytest.mark.parametrize("side", ["right", "left"])
@pytest.mark.parametrize("head_type,H,Hkv,D", APPEND_LAYOUTS, ids=[f"{t}-H{h}-Hkv{j}-D{d}" for t, h, j, d in APPEND_LAYOUTS])
def test_append_fp8_bitwise(head_type, H, Hkv, D, side):
    """Prefill spans, one decode row per sequence, an overflowing append: the
    cache bytes and the scales against the torch rule (the op's CPU branch),
    bit for bit; what no append named keeps its 0xff bytes and NaN scales."""
    lo = QKVLayout.make(H, Hkv, D, head_type)
    g = torch.Generator().manual_seed(8)
    rows = torch.arange(AB * AS)[:, None]
    qkv = (torch.randn(AB * AS, lo.row_len, generator=g) * (0.25 + rows % 5)).to(torch.bfloat16)
    qkv[7] = 0                                    # an all-zero row: zeros, scale 2^-64 / 448
    qkv[9] = torch.finfo(torch.bfloat16).tiny / 4  # a row of bf16 subnormals
    begin = [b * AS + (0 if side == "right" else AS - n) for b, n in enumerate(ALENS)]
    end = [s + n for s, n in zip(begin, ALENS)]
    starts = [b * AS for b in range(AB)]
    appends = [  # (seq_begin, seq_end, dst_pos, max_rows)
        (begin, end, [0] * AB, max(ALENS)),
        ([b * AS + 3 for b in range(AB)], [b * AS + 4 for b in range(AB)], ALENS, 1),
        (starts, [s + 5 for s in starts], [ACAP - 2] * AB, None),   # 2 of 5 rows land
        (starts, [s + 5 for s in starts], [ACAP] * AB, None),       # none does
    ]
    caches = {d: _sentinel_cache(Hkv, D, d) for d in ("cpu", "cuda")}
    for step, (sb, se, dp, max_rows) in enumerate(appends):
        for d, (k, ks, v, vs) in caches.items():
            i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=d)
            with torch.no_grad():
                Fx.kv_cache_append(qkv.to(d), lo, i32(sb), i32(se), k, v, i32(dp), max_rows=max_rows,
                                   k_scale=ks, v_scale=vs)
        for name, want, got in zip(("k", "k_scale", "v", "v_scale"), caches["cpu"], caches["cuda"]):
            bits = torch.uint8 if want.dtype == FP8 else torch.int32
            assert torch.equal(got.cpu().view(bits), want.view(bits)), f"{name} after append {step}"
    k, ks = caches["cuda"][:2]     # sequence 1 holds its prompt token and its decode row, then the 2 overflow rows
    assert bool((k.view(torch.uint8)[1, 2 : ACAP - 2] == 0xFF).all()) and bool(ks[1, :, 2 : ACAP - 2].isnan().all())
    assert not ks[0, :, :41].isnan().any() and not ks[:, :, ACAP - 2 :].isnan().any()


def test_append_then_decode_fp8():
    """Append + decode on the fp8 cache against float64 attention over the
    dequantised rows; the distance to the bf16 cache's decode_attention on
    the unquantised rows is the quantisation's cost: printed, not bounded."""
    worst = cost = 0.0
    for head_type, H, Hkv, D in LAYOUTS:
        lo = QKVLayout.make(H, Hkv, D, head_type)
        L = 200
        g = torch.Generator().manual_seed(21)
        qkv = (torch.randn(L, lo.row_len, generator=g) * 0.7).to(torch.bfloat16)
        scale = 1.0 / math.sqrt(D)
        i32 = lambda x: torch.tensor([x], dtype=torch.int32, device="cuda")
        k8 = torch.full((1, S_CAP, Hkv, D), 0xFF, dtype=torch.uint8, device="cuda").view(FP8)
        v8 = k8.clone()
        ks = torch.full((1, Hkv, S_CAP), float("nan"), device="cuda")
        vs = ks.clone()
        kb = torch.full((1, S_CAP, Hkv, D), float("nan"), dtype=torch.bfloat16, device="cuda")
        vb = kb.clone()
        qq, kk, vv = lo.unpack_cpu(qkv)
        kq, vq = Fx.quantize_kv_e4m3(kk), Fx.quantize_kv_e4m3(vv)
        ref = _ref64(qq[L - 1 :], (kq[0].double() * kq[1].double()[..., None])[None],
                     (vq[0].double() * vq[1].double()[..., None])[None], [L], lo, scale)
        with torch.no_grad():
            Fx.kv_cache_append(qkv.cuda(), lo, i32(0), i32(L), k8, v8, i32(0), k_scale=ks, v_scale=vs)
            Fx.kv_cache_append(qkv.cuda(), lo, i32(0), i32(L), kb, vb, i32(0))
            o_bf16 = Fx.decode_attention(qkv[L - 1 :].cuda(), lo, kb, vb, i32(L), scale, L, num_splits=1)
            for nsplit in (1, 3):
                o = Fx.decode_attention(qkv[L - 1 :].cuda(), lo, k8, v8, i32(L), scale, L, num_splits=nsplit,
                                        k_scale=ks, v_scale=vs)
                got = o.cpu().double().view(1, H, D)
                worst = max(worst, float((got - ref).abs().max()))
                cost = max(cost, float((o.float() - o_bf16.float()).abs().max()))
                torch.testing.assert_close(got, ref, **TOL)
    print(f"max|fp8 decode - ref64 over the dequantised cache| {worst:.4e}; "
          f"max|fp8 decode - bf16-cache decode| {cost:.4e}")


def test_error_codes_fp8():
    L = hip.lib()
    lo = QKVLayout.make(4, 2, 64, "gqa")
    qkv = torch.zeros(4, lo.row_len, dtype=torch.bfloat16, device="cuda")
    k = torch.zeros(2, 8, 2, 64, dtype=torch.uint8, device="cuda")
    v = torch.zeros_like(k)
    ks = torch.ones(2, 2, 8, device="cuda")
    vs = torch.ones_like(ks)
    i32 = torch.zeros(2, dtype=torch.int32, device="cuda")
    o = torch.zeros(2, 4 * 64, dtype=torch.bfloat16, device="cuda")

    def append(batch=2, max_rows=1, Hkv=2, D=64, S_cap=8, row=lo.row_len, c_ts=k.stride(1), dtype=hip.BF16):
        return L.dolomite_kv_cache_append_fp8(
            hip.stream(), hip.ptr(qkv), hip.ptr(i32), hip.ptr(i32), hip.ptr(i32), hip.ptr(k), hip.ptr(v),
            hip.ptr(ks), hip.ptr(vs), batch, max_rows, Hkv, D, S_cap, row, lo.k_off, lo.v_off, lo.kv_hstride,
            k.stride(0), c_ts, k.stride(2), ks.stride(0), ks.stride(1), dtype)

    assert append() == 0
    assert append(dtype=hip.F32) == 9010
    assert append(batch=-1) == 9030
    assert append(max_rows=-1) == 9030
    assert append(S_cap=-1) == 9030
    assert append(D=12) == 9031
    assert append(D=0) == 9031
    assert append(D=136) == 9031
    assert append(row=lo.row_len + 4) == 9031
    assert append(c_ts=k.stride(1) + 4) == 9031

    def decode(D=64, scale=0.125, nsplit=1, scratch=None, dtype=hip.BF16, batch=2, H=4, k_ts=k.stride(1)):
        return L.dolomite_fa_decode_fp8(
            hip.stream(), hip.ptr(qkv), hip.ptr(k), hip.ptr(v), hip.ptr(ks), hip.ptr(vs), hip.ptr(o),
            hip.ptr(scratch), hip.ptr(i32), batch, H, 2, D, 2, 8, nsplit, lo.row_len, lo.q_gstride,
            k.stride(0), k_ts, k.stride(2), v.stride(0), v.stride(1), v.stride(2),
            ks.stride(0), ks.stride(1), scale, dtype)

    assert decode() == 0
    assert decode(dtype=hip.F32) == 9010
    assert decode(D=136) == 9011
    assert decode(scale=0.0) == 9015
    assert decode(scale=float("nan")) == 9015
    assert decode(D=60) == 9031
    assert decode(k_ts=k.stride(1) + 4) == 9031
    assert decode(batch=-1) == 9032
    assert decode(H=6) == 9032
    assert decode(nsplit=0) == 9033
    assert decode(nsplit=2) == 9034
    torch.cuda.synchronize()
    with torch.no_grad(), pytest.raises(TypeError, match="bf16 qkv"):   # a non-bf16 model on the GPU
        Fx.decode_attention(qkv[:2].float(), lo, k.view(FP8), v.view(FP8), i32 + 1, 0.125, 8, k_scale=ks, v_scale=vs)
