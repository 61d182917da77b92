"""KV cache append and single-token decode attention on hardware.

Shapes sit on the decode kernel's edges, not the workload's: the 64-key wave
tile, the 4-wave round-robin inside a workgroup, the split boundaries
(chunk = ceil(max_len / nsplit) rounded up to 64: with max_len = 200 that is
256 / 128 / 128 / 64 keys for nsplit = 1 / 2 / 3 / 5, so nsplit = 3 and 5 have
splits without a single key), G = 3 (padded head columns), G = 32 (two
16-head blocks) and G = 40 (a second head group). Everything behind a
sequence's cache_len is NaN.

Measured on an MI355X (printed by the tests): see DESIGN.md §7.
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


LAYOUTS = [
    ("mqa", 4, 1, 80), ("gqa", 4, 2, 128), ("mha", 2, 2, 64),
    ("gqa", 6, 2, 64),    # G = 3: padded head columns
    ("mqa", 32, 1, 80),   # two 16-head blocks
    ("mqa", 40, 1, 64),   # G > 32: a second head group on grid.z, 8 of its 32 columns real
]
_IDS = [f"{t}-H{h}-Hkv{j}-D{d}" for t, h, j, d in LAYOUTS]
# +-1 around the 64-key tile and every chunk boundary above, one empty cache
CACHE_LEN = [1, 63, 64, 65, 127, 128, 129, 193, 200, 0]
S_CAP, MAX_LEN = 256, 200
NSPLITS = [1, 2, 3, 5]
TOL = dict(rtol=2e-2, atol=2e-2)  # the forward's tolerance against its oracle (test_gpu_kernels.py)


def _nan_tail(cache, lens):
    for b, n in enumerate(lens):
        cache[b, n:] = float("nan")
    return cache


def _ref64(q, k_cache, v_cache, lens, lo, scale):
    """float64 softmax attention from the same bf16 inputs. q (B, H, D)."""
    B = q.shape[0]
    G = lo.H // lo.Hkv
    o = torch.zeros(B, lo.H, lo.D, dtype=torch.float64)
    for b, n in enumerate(lens):
        if n == 0:
            continue
        for h in range(lo.H):
            kk = k_cache[b, :n, h // G].double()
            vv = v_cache[b, :n, h // G].double()
            p = torch.softmax((kk @ q[b, h].double()) * scale, dim=0)
            o[b, h] = p @ vv
    return o


def _pack_q(q, lo):
    """(B, H, D) q into the q slots of a packed (B, row_len) row; the row's
    own K/V slots hold NaN (decode must not read them)."""
    B = q.shape[0]
    rows = torch.full((B, lo.row_len), float("nan"), dtype=q.dtype)
    for h in range(lo.H):
        off = (h // lo.G) * lo.q_gstride + (h % lo.G) * lo.D
        rows[:, off : off + lo.D] = q[:, h]
    return rows


@pytest.fixture(scope="module", params=LAYOUTS, ids=_IDS)
def random_case(request):
    """Inputs and the float64 reference, computed once per layout."""
    head_type, H, Hkv, D = request.param
    lo = QKVLayout.make(H, Hkv, D, head_type)
    B = len(CACHE_LEN)
    g = torch.Generator().manual_seed(11)
    q = (torch.randn(B, H, D, generator=g) * 0.7).to(torch.bfloat16)
    k = _nan_tail((torch.randn(B, S_CAP, Hkv, D, generator=g) * 0.7).to(torch.bfloat16), CACHE_LEN)
    v = _nan_tail((torch.randn(B, S_CAP, Hkv, D, generator=g) * 0.7).to(torch.bfloat16), CACHE_LEN)
    scale = 1.0 / math.sqrt(D)
    ref = _ref64(q, k, v, CACHE_LEN, lo, scale)
    dev = dict(
        qkv=_pack_q(q, lo).cuda(), k=k.cuda(), v=v.cuda(),
        lens=torch.tensor(CACHE_LEN, dtype=torch.int32).cuda(),
    )
    return lo, scale, dev, ref


@pytest.mark.parametrize("nsplit", NSPLITS)
def test_decode_matches_float64(random_case, nsplit):
    lo, scale, dev, ref = random_case
    with torch.no_grad():
        o = Fx.decode_attention(dev["qkv"], lo, dev["k"], dev["v"], dev["lens"], scale, MAX_LEN, num_splits=nsplit)
        o2 = Fx.decode_attention(dev["qkv"], lo, dev["k"], dev["v"], dev["lens"], scale, MAX_LEN, num_splits=nsplit)
    torch.cuda.synchronize()
    assert o.shape == (len(CACHE_LEN), lo.H * lo.D) and o.dtype == torch.bfloat16
    assert not torch.isnan(o).any(), "NaN leaked from behind cache_len"
    got = o.cpu().double().view(-1, lo.H, lo.D)
    print(f"nsplit {nsplit}: max|o - ref64| {float((got - ref).abs().max()):.4e}")
    torch.testing.assert_close(got, ref, **TOL)
    empty = CACHE_LEN.index(0)
    assert torch.equal(o[empty].view(torch.int16), torch.zeros_like(o[empty]).view(torch.int16)), "empty cache: +0"
    assert torch.equal(o.view(torch.int16), o2.view(torch.int16)), "not reproducible run to run"


def test_default_split_rule_runs(random_case):
    lo, scale, dev, ref = random_case
    with torch.no_grad():
        o = Fx.decode_attention(dev["qkv"], lo, dev["k"], dev["v"], dev["lens"], scale, MAX_LEN)
    assert Fx.decode_num_splits(len(CACHE_LEN), lo, MAX_LEN) == 1  # ceil(4 tiles / 4)
    torch.testing.assert_close(o.cpu().double().view(-1, lo.H, lo.D), ref, **TOL)


def _marker_candidates(n, H):
    """Keys worth a marker for a cache of n keys: key 0, the newest key, both
    sides of every tile / wave / split boundary, then filler so that (where
    the cache is long enough) every head gets a key of its own."""
    edges = [0, n - 1, 63, 64, 127, 128, 191, 192]
    cand = []
    for p in edges + list(range(n)):
        if 0 <= p < n and p not in cand:
            cand.append(p)
        if len(cand) >= max(H, len(edges)):
            break
    return cand


@pytest.mark.parametrize("head_type,H,Hkv,D", LAYOUTS, ids=_IDS)
def test_decode_markers_exact(head_type, H, Hkv, D):
    """2e-2 cannot see one dropped key among 200; this can. v[key, :] = key + 1
    (integers <= 256, exact in bf16); head h's query is 20*e_h and one chosen
    key per head is 20*e_h, every other key is zero in the first H dims. The
    chosen key's score leads by 400 / sqrt(D) >= 35 nats, so o[b, h, :] must
    EQUAL marker + 1 — for the float64 reference too, by construction."""
    lo = QKVLayout.make(H, Hkv, D, head_type)
    assert D >= H
    B = len(CACHE_LEN)
    scale = 1.0 / math.sqrt(D)
    assert 400 * scale >= 35
    q = torch.zeros(B, H, D, dtype=torch.bfloat16)
    for h in range(H):
        q[:, h, h] = 20.0
    qkv = _pack_q(q, lo).cuda()
    v = torch.arange(1, S_CAP + 1, dtype=torch.float32)[None, :, None, None].expand(B, S_CAP, Hkv, D)
    v = _nan_tail(v.to(torch.bfloat16).contiguous(), CACHE_LEN)
    lens = torch.tensor(CACHE_LEN, dtype=torch.int32).cuda()
    g = torch.Generator().manual_seed(3)
    rounds = max(-(-len(_marker_candidates(n, H)) // H) for n in CACHE_LEN if n > 0)
    for r in range(rounds):
        k = (torch.randn(B, S_CAP, Hkv, D, generator=g) * 0.5).to(torch.bfloat16)
        k[..., :H] = 0
        want = torch.zeros(B, H)
        for b, n in enumerate(CACHE_LEN):
            if n == 0:
                continue
            cand = _marker_candidates(n, H)
            for h in range(H):
                key = cand[(r * H + h) % len(cand)]
                k[b, key, h // lo.G, h] = 20.0
                want[b, h] = key + 1
        k = _nan_tail(k, CACHE_LEN)
        ref = _ref64(q, k, v, CACHE_LEN, lo, scale)
        assert float((ref - want[:, :, None].double()).abs().max()) < 1e-9
        for nsplit in NSPLITS:
            with torch.no_grad():
                o = Fx.decode_attention(qkv, lo, k.cuda(), v.cuda(), lens, scale, MAX_LEN, num_splits=nsplit)
            got = o.cpu().float().view(B, H, D)
            bad = (got != want[:, :, None]).any(-1).nonzero().tolist()
            assert not bad, f"round {r} nsplit {nsplit}: wrong (sequence, head) {bad[:8]}"


def test_decode_matches_forward_last_row():
    """decode_attention of a packed sequence's last token against the last
    row of varlen_attention over the whole sequence."""
    worst = 0.0
    for head_type, H, Hkv, D in LAYOUTS:
        lo = QKVLayout.make(H, Hkv, D, head_type)
        L = 200
        g = torch.Generator().manual_seed(21)
        qkv = (torch.randn(L, lo.row_len, generator=g) * 0.7).to(torch.bfloat16).cuda()
        scale = 1.0 / math.sqrt(D)
        i32 = lambda x: torch.tensor([x], dtype=torch.int32, device="cuda")
        k = torch.full((1, S_CAP, Hkv, D), float("nan"), dtype=torch.bfloat16, device="cuda")
        v = torch.full_like(k, float("nan"))
        with torch.no_grad():
            o_fwd = Fx.varlen_attention(qkv, torch.tensor([0, L], dtype=torch.int32).cuda(), L, lo, scale)
            Fx.kv_cache_append(qkv, lo, i32(0), i32(L), k, v, i32(0))
            for nsplit in (1, 3):
                o_dec = Fx.decode_attention(qkv[L - 1 :], lo, k, v, i32(L), scale, L, num_splits=nsplit)
                diff = float((o_dec.float() - o_fwd[L - 1 :].float()).abs().max())
                worst = max(worst, diff)
                torch.testing.assert_close(o_dec.float(), o_fwd[L - 1 :].float(), **TOL)
    print(f"max|decode - forward last row| {worst:.4e}")


# ---------------------------------------------------------------------------
# kv_cache_append
# ---------------------------------------------------------------------------

AB, AS, ACAP = 4, 40, 48
ALENS = [40, 1, 17, 0]
_NAN_BITS = torch.tensor(float("nan"), dtype=torch.bfloat16).view(torch.int16).item()


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("side", ["right", "left"])
@pytest.mark.parametrize("head_type,H,Hkv,D", LAYOUTS[:4], ids=_IDS[:4])
def test_append_prefill_then_decode_rows(head_type, H, Hkv, D, side):
    lo = QKVLayout.make(H, Hkv, D, head_type)
    g = torch.Generator().manual_seed(8)
    qkv = torch.randn(AB * AS, lo.row_len, generator=g).to(torch.bfloat16)
    begin = [b * AS + (0 if side == "right" else AS - n) for b, n in enumerate(ALENS)]
    end = [s + n for s, n in zip(begin, ALENS)]
    _, kk, vv = lo.unpack_cpu(qkv)
    k_want = torch.full((AB, ACAP, Hkv, D), float("nan"), dtype=torch.bfloat16)
    v_want = torch.full_like(k_want, float("nan"))
    for b, (s, e) in enumerate(zip(begin, end)):
        k_want[b, : e - s] = kk[s:e]
        v_want[b, : e - s] = vv[s:e]
    dev = lambda x: torch.tensor(x, dtype=torch.int32).cuda()
    k = torch.full((AB, ACAP, Hkv, D), float("nan"), dtype=torch.bfloat16, device="cuda")
    v = torch.full_like(k, float("nan"))
    with torch.no_grad():
        Fx.kv_cache_append(qkv.cuda(), lo, dev(begin), dev(end), k, v, dev([0] * AB), max_rows=max(ALENS))
    assert torch.equal(_bits(k.cpu()), _bits(k_want)), "K after prefill append"
    assert torch.equal(_bits(v.cpu()), _bits(v_want)), "V after prefill append"

    # one decode row per sequence at dst_pos = lengths (row 3 + b*AS of the buffer)
    rows = [b * AS + 3 for b in range(AB)]
    for b, r in enumerate(rows):
        k_want[b, ALENS[b]] = kk[r]
        v_want[b, ALENS[b]] = vv[r]
    with torch.no_grad():
        Fx.kv_cache_append(qkv.cuda(), lo, dev(rows), dev([r + 1 for r in rows]), k, v, dev(ALENS), max_rows=1)
    assert torch.equal(_bits(k.cpu()), _bits(k_want)), "K after decode append"
    assert torch.equal(_bits(v.cpu()), _bits(v_want)), "V after decode append"

    # positions >= S_cap are skipped: 5 rows from ACAP - 2 land 2, nothing else moves
    starts = [b * AS for b in range(AB)]
    for b, s in enumerate(starts):
        k_want[b, ACAP - 2 :] = kk[s : s + 2]
        v_want[b, ACAP - 2 :] = vv[s : s + 2]
    guard = torch.full((64,), float("nan"), dtype=torch.bfloat16, device="cuda")
    with torch.no_grad():
        Fx.kv_cache_append(qkv.cuda(), lo, dev(starts), dev([s + 5 for s in starts]), k, v, dev([ACAP - 2] * AB))
        Fx.kv_cache_append(qkv.cuda(), lo, dev(starts), dev([s + 5 for s in starts]), k, v, dev([ACAP] * AB))
    torch.cuda.synchronize()
    assert torch.equal(_bits(k.cpu()), _bits(k_want)), "K after the overflowing append"
    assert torch.equal(_bits(v.cpu()), _bits(v_want)), "V after the overflowing append"
    assert bool((_bits(guard.cpu()) == _NAN_BITS).all())


def test_error_codes():
    L = hip.lib()
    lo = QKVLayout.make(4, 2, 64, "gqa")
    qkv = torch.zeros(4, lo.row_len, dtype=torch.bfloat16, device="cuda")
    k = torch.zeros(2, 8, 2, 64, dtype=torch.bfloat16, device="cuda")
    v = torch.zeros_like(k)
    i32 = torch.zeros(2, dtype=torch.int32, device="cuda")
    o = torch.zeros(2, 4 * 64, dtype=torch.bfloat16, device="cuda")

    def append(batch=2, max_rows=1, Hkv=2, D=64, S_cap=8, row=lo.row_len, dtype=hip.BF16):
        return L.dolomite_kv_cache_append(
            hip.stream(), hip.ptr(qkv), hip.ptr(i32), hip.ptr(i32), hip.ptr(i32), hip.ptr(k), hip.ptr(v),
            batch, max_rows, Hkv, D, S_cap, row, lo.k_off, lo.v_off, lo.kv_hstride,
            k.stride(0), k.stride(1), k.stride(2), dtype)

    assert append() == 0
    assert append(dtype=hip.F32) == 9010
    assert append(batch=-1) == 9030
    assert append(max_rows=-1) == 9030
    assert append(S_cap=-1) == 9030
    assert append(D=12) == 9031
    assert append(D=0) == 9031
    assert append(row=lo.row_len + 4) == 9031

    def decode(D=64, scale=0.125, nsplit=1, scratch=None, dtype=hip.BF16, batch=2, H=4):
        return L.dolomite_fa_decode(
            hip.stream(), hip.ptr(qkv), hip.ptr(k), hip.ptr(v), hip.ptr(o), hip.ptr(scratch), hip.ptr(i32),
            batch, H, 2, D, 2, 8, nsplit, lo.row_len, lo.q_gstride,
            k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2), scale, dtype)

    assert decode() == 0
    assert decode(dtype=hip.F32) == 9010
    assert decode(D=136) == 9011
    assert decode(scale=0.0) == 9015
    assert decode(scale=float("nan")) == 9015
    assert decode(D=60) == 9031
    assert decode(batch=-1) == 9032
    assert decode(H=6) == 9032
    assert decode(nsplit=0) == 9033
    assert decode(nsplit=2) == 9034
    assert L.dolomite_fa_decode_scratch_floats(2, 4, 64, 3) == 2 * 4 * 3 * 66
    assert L.dolomite_fa_decode_scratch_floats(2, 4, 64, 1) == 0
    assert L.dolomite_fa_decode_scratch_floats(2, 4, 64, 0) == -1
    torch.cuda.synchronize()


def test_ops_refuse_grad():
    lo = QKVLayout.make(4, 2, 64, "gqa")
    qkv = torch.zeros(2, lo.row_len, dtype=torch.bfloat16, device="cuda", requires_grad=True)
    k = torch.zeros(2, 8, 2, 64, dtype=torch.bfloat16, device="cuda")
    lens = torch.ones(2, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="inference only"):
        Fx.decode_attention(qkv, lo, k, k.clone(), lens, 0.125, 8)


# ---------------------------------------------------------------------------
# the model on hardware
# ---------------------------------------------------------------------------

MODELS = [("mqa", 4, 1, 80), ("gqa", 4, 2, 128)]


def _model(head_type, H, Hkv, D):
    from dolomite_engine_amd.hf_models import GPTDolomiteConfig, GPTDolomiteForCausalLM

    torch.manual_seed(5)
    cfg = GPTDolomiteConfig(
        vocab_size=512, n_positions=256, n_embd=H * D, n_layer=2, n_head=H,
        attention_head_type=head_type, num_key_value_heads=Hkv, n_inner=512,
        activation_function="swiglu", normalization_function="rmsnorm",
        position_embedding_type="rope", resid_pdrop=0.0, embd_pdrop=0.0,
        attn_pdrop=0.0, tie_word_embeddings=False,
    )
    cfg._attn_implementation = "flash_attention_2"
    return GPTDolomiteForCausalLM(cfg).to(torch.bfloat16).cuda().eval()


def _padded(seqs, side, pad=0):
    S = max(len(s) for s in seqs)
    ids = torch.full((len(seqs), S), pad, dtype=torch.long)
    mask = torch.zeros(len(seqs), S, dtype=torch.long)
    pos = torch.zeros(len(seqs), S, dtype=torch.long)
    for b, s in enumerate(seqs):
        a = 0 if side == "right" else S - len(s)
        ids[b, a : a + len(s)] = torch.tensor(s)
        mask[b, a : a + len(s)] = 1
        pos[b, a : a + len(s)] = torch.arange(len(s))
    return ids.cuda(), mask.cuda(), pos.cuda()


def _last_logits(model, seqs, side):
    ids, mask, pos = _padded(seqs, side)
    logits = model(input_ids=ids, attention_mask=mask, position_ids=pos).logits
    last = [(len(s) - 1) if side == "right" else ids.shape[1] - 1 for s in seqs]
    return logits[torch.arange(len(seqs)), torch.tensor(last)]


@pytest.mark.parametrize("side", ["right", "left"])
@pytest.mark.parametrize("head_type,H,Hkv,D", MODELS, ids=[f"{t}-D{d}" for t, _, _, d in MODELS])
def test_model_cached_logits_match_recompute(head_type, H, Hkv, D, side):
    """Prefill + 4 decode steps against no-cache forwards of the grown batch
    at the project's bf16 logits gate (rtol 1e-2 / atol 2e-2)."""
    model = _model(head_type, H, Hkv, D)
    g = torch.Generator().manual_seed(9)
    seqs = [torch.randint(0, 512, (n,), generator=g).tolist() for n in (70, 1, 33)]
    feed = torch.randint(0, 512, (4, 3), generator=g)
    worst = 0.0
    with torch.no_grad():
        ids, mask, pos = _padded(seqs, side)
        out = model(input_ids=ids, attention_mask=mask, position_ids=pos, use_cache=True)
        cache = out.past_key_values
        for step in range(4):
            for b in range(3):
                seqs[b].append(int(feed[step, b]))
            out = model(input_ids=feed[step].cuda()[:, None], past_key_values=cache, use_cache=True)
            assert out.past_key_values is cache
            want = _last_logits(model, seqs, side).float()
            got = out.logits[:, 0].float()
            worst = max(worst, float((got - want).abs().max()))
            torch.testing.assert_close(got, want, rtol=1e-2, atol=2e-2)
    print(f"max|cached - recomputed logits| {worst:.4e}")
    assert cache.get_seq_length() == 74


def test_generate_greedy_is_reproducible():
    model = _model(*MODELS[0])
    g = torch.Generator().manual_seed(4)
    seqs = [torch.randint(0, 512, (n,), generator=g).tolist() for n in (20, 3, 11)]
    ids, mask, _ = _padded(seqs, "left")
    a = model.generate(ids, attention_mask=mask, max_new_tokens=12)
    b = model.generate(ids, attention_mask=mask, max_new_tokens=12)
    assert a.shape == (3, 32) and torch.equal(a[:, :20], ids)
    assert torch.equal(a, b)
