"""KV cache, decode attention and generate() through the CPU branches (fp32,
tiny models): the cached path must reproduce the no-cache forward, for left-
and right-padded prompts, rope and learned positions, every head layout."""

import math

import pytest
import torch

from dolomite_engine_amd.hf_models import GPTDolomiteConfig, GPTDolomiteForCausalLM, KVCache
from dolomite_engine_amd.model_wrapper import ModelWrapper
from dolomite_engine_amd.ops import QKVLayout, decode_attention, kv_cache_append

HEADS = [("mqa", 1), ("gqa", 2), ("mha", 4)]
POSITIONS = ["rope", "learned_absolute"]
VOCAB = 97


def _kw(head_type, Hkv, pos):
    return dict(
        vocab_size=VOCAB, n_positions=64, n_embd=64, n_layer=2, n_head=4,
        attention_head_type=head_type, num_key_value_heads=Hkv, n_inner=128,
        activation_function="swiglu", normalization_function="rmsnorm",
        position_embedding_type=pos, resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0,
        tie_word_embeddings=False, initializer_range=0.2,
    )


def _model(head_type="mqa", Hkv=1, pos="rope", impl="flash_attention_2", seed=0):
    torch.manual_seed(seed)
    cfg = GPTDolomiteConfig(**_kw(head_type, Hkv, pos))
    cfg._attn_implementation = impl
    return GPTDolomiteForCausalLM(cfg).eval()


def _padded(seqs, side, pad=0):
    S = max(len(s) for s in seqs)
    ids = torch.full((len(seqs), S), pad, dtype=torch.long)
    mask = torch.zeros(len(seqs), S, dtype=torch.long)
    for b, s in enumerate(seqs):
        a = 0 if side == "right" else S - len(s)
        ids[b, a : a + len(s)] = torch.tensor(s)
        mask[b, a : a + len(s)] = 1
    return ids, mask


def _prompts(seed=1, lens=(7, 1, 4)):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(1, VOCAB, (n,), generator=g).tolist() for n in lens]


def _grow(seqs, width, side, new):
    """The (B, width + t) batch after t generated tokens per sequence. Left
    padding keeps the pad columns and appends on the right; right padding
    puts a sequence's new tokens straight behind its prompt. Positions are
    the no-cache default (arange over the columns) either way, which is what
    the cache continues."""
    t = len(new[0])
    ids = torch.zeros(len(seqs), width + t, dtype=torch.long)
    mask = torch.zeros(len(seqs), width + t, dtype=torch.long)
    last = []
    for b, s in enumerate(seqs):
        a = 0 if side == "right" else width - len(s)
        full = s + new[b]
        ids[b, a : a + len(full)] = torch.tensor(full)
        mask[b, a : a + len(full)] = 1
        last.append(a + len(full) - 1)
    pos = torch.arange(width + t).unsqueeze(0).expand(len(seqs), -1)
    return ids, mask, pos, torch.tensor(last)


# ---------------------------------------------------------------------------
# ops
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("head_type,Hkv", HEADS)
def test_ops_cpu_against_float64(head_type, Hkv):
    H, D, S_cap = 4, 16, 32
    lens = [1, 5, 0, 17]
    B = len(lens)
    lo = QKVLayout.make(H, Hkv, D, head_type)
    g = torch.Generator().manual_seed(2)
    # the cache is filled through kv_cache_append from a padded (B, 20) batch
    S = 20
    qkv = torch.randn(B * S, lo.row_len, generator=g)
    begin = torch.tensor([b * S + 2 for b in range(B)], dtype=torch.int32)
    end = begin + torch.tensor(lens, dtype=torch.int32)
    k = torch.full((B, S_cap, Hkv, D), float("nan"))
    v = torch.full((B, S_cap, Hkv, D), float("nan"))
    kv_cache_append(qkv, lo, begin, end, k, v, torch.zeros(B, dtype=torch.int32))
    _, kk, vv = lo.unpack_cpu(qkv)
    for b, n in enumerate(lens):
        assert torch.equal(k[b, :n], kk[b * S + 2 : b * S + 2 + n])
        assert torch.equal(v[b, :n], vv[b * S + 2 : b * S + 2 + n])
        assert torch.isnan(k[b, n:]).all() and torch.isnan(v[b, n:]).all()

    # positions >= S_cap are skipped
    k2, v2 = k.clone(), v.clone()
    kv_cache_append(qkv, lo, begin, begin + 3, k2, v2, torch.full((B,), S_cap - 1, dtype=torch.int32))
    assert torch.equal(k2[:, S_cap - 1], kk[begin.long()])
    assert torch.equal(torch.nan_to_num(k2[:, : S_cap - 1], 7.0), torch.nan_to_num(k[:, : S_cap - 1], 7.0))

    new = torch.randn(B, lo.row_len, generator=g)
    q, _, _ = lo.unpack_cpu(new)
    scale = 1.0 / math.sqrt(D)
    o = decode_attention(new, lo, k, v, torch.tensor(lens, dtype=torch.int32), scale, max(lens))
    assert o.shape == (B, H * D) and not torch.isnan(o).any()
    G = H // Hkv
    for b, n in enumerate(lens):
        for h in range(H):
            got = o[b, h * D : (h + 1) * D]
            if n == 0:
                assert torch.equal(got, torch.zeros(D))
                continue
            sc = (k[b, :n, h // G].double() @ q[b, h].double()) * scale
            p = (sc - sc.max()).exp()
            want = (p / p.sum()) @ v[b, :n, h // G].double()
            torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=1e-6)


def test_ops_are_inference_only():
    lo = QKVLayout.make(4, 1, 16, "mqa")
    k = torch.zeros(2, 8, 1, 16)
    qkv = torch.zeros(2, lo.row_len, requires_grad=True)
    lens = torch.ones(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="inference only"):
        decode_attention(qkv, lo, k, k.clone(), lens, 0.25, 8)
    with pytest.raises(RuntimeError, match="inference only"):
        kv_cache_append(qkv, lo, lens - 1, lens, k, k.clone(), lens - 1)
    with torch.no_grad():
        decode_attention(qkv, lo, k, k.clone(), lens, 0.25, 8)


# ---------------------------------------------------------------------------
# cached logits == recomputed logits
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("head_type,Hkv", HEADS)
def test_cached_logits_equal_recomputed(head_type, Hkv, pos, side):
    model = _model(head_type, Hkv, pos)
    seqs = _prompts()
    width = 7
    g = torch.Generator().manual_seed(5)
    feed = torch.randint(1, VOCAB, (5, 3), generator=g)
    ids, mask = _padded(seqs, side)
    assert ids.shape == (3, 7)
    with torch.no_grad():
        out = model(input_ids=ids, attention_mask=mask, use_cache=True)
        cache = out.past_key_values
        assert isinstance(cache, KVCache) and cache.max_length == 64
        assert cache.get_seq_length() == 7 and cache.lengths.tolist() == [7, 1, 4]
        plain = model(input_ids=ids, attention_mask=mask).logits
        torch.testing.assert_close(out.logits, plain)  # the prefill is today's span path
        new = [[] for _ in seqs]
        for step in range(5):
            for b in range(3):
                new[b].append(int(feed[step, b]))
            out = model(input_ids=feed[step][:, None], past_key_values=cache, use_cache=True)
            assert out.past_key_values is cache and out.logits.shape == (3, 1, VOCAB)
            gids, gmask, gpos, last = _grow(seqs, width, side, new)
            want = model(input_ids=gids, attention_mask=gmask, position_ids=gpos).logits[torch.arange(3), last]
            torch.testing.assert_close(out.logits[:, 0], want)
        assert cache.get_seq_length() == 12 and cache.lengths.tolist() == [12, 6, 9]


def test_explicit_position_ids_and_allpad_row():
    """Positions that restart at 0 on each sequence's first real token (the
    reference's mask-cumsum convention), passed explicitly at prefill, are
    continued by the decode steps; an all-pad row has length 0."""
    model = _model("gqa", 2, "rope")
    seqs = _prompts()
    ids, mask = _padded(seqs, "left")
    ids = torch.cat([ids, torch.zeros(1, 7, dtype=torch.long)])
    mask = torch.cat([mask, torch.zeros(1, 7, dtype=torch.long)])
    pos = (mask.cumsum(-1) - 1).clamp(min=0)
    with torch.no_grad():
        out = model(input_ids=ids, attention_mask=mask, position_ids=pos, use_cache=True)
        cache = out.past_key_values
        assert cache.lengths.tolist() == [7, 1, 4, 0] and cache.next_position.tolist() == [7, 1, 4, 0]
        tok = torch.tensor([[3], [4], [5], [6]])
        out = model(input_ids=tok, past_key_values=cache, attention_mask=torch.ones(4, 8, dtype=torch.long))
        assert cache.next_position.tolist() == [8, 2, 5, 1]
        gids = torch.cat([ids, tok], dim=1)
        gmask = torch.cat([mask, torch.ones(4, 1, dtype=torch.long)], dim=1)
        gpos = torch.cat([pos, torch.tensor([[7], [1], [4], [0]])], dim=1)
        want = model(input_ids=gids, attention_mask=gmask, position_ids=gpos).logits[:, -1]
    torch.testing.assert_close(out.logits[:, 0], want)


# ---------------------------------------------------------------------------
# generate
# ---------------------------------------------------------------------------


def _argmax_loop(model, seqs, width, side, n):
    new = [[] for _ in seqs]
    with torch.no_grad():
        for _ in range(n):
            gids, gmask, gpos, last = _grow(seqs, width, side, new)
            logits = model(input_ids=gids, attention_mask=gmask, position_ids=gpos).logits
            nxt = logits[torch.arange(len(seqs)), last].argmax(-1)
            for b in range(len(seqs)):
                new[b].append(int(nxt[b]))
    return torch.tensor(new)


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("head_type,Hkv", HEADS)
def test_generate_greedy_is_the_argmax_loop(head_type, Hkv, pos, side):
    model = _model(head_type, Hkv, pos)  # seed 0 for every case: no near-tie met
    seqs = _prompts()
    ids, mask = _padded(seqs, side)
    out = model.generate(ids, attention_mask=mask, max_new_tokens=6)
    assert out.shape == (3, 13) and torch.equal(out[:, :7], ids)
    assert torch.equal(out[:, 7:], _argmax_loop(model, seqs, 7, side, 6))


def test_generate_without_mask():
    model = _model()
    ids = torch.tensor(_prompts(lens=(5, 5)))
    out = model.generate(ids, max_new_tokens=4)
    assert torch.equal(out[:, 5:], _argmax_loop(model, ids.tolist(), 5, "right", 4))


def test_generate_eos_and_wrapper_counts():
    model = _model()
    seqs = _prompts()
    ids, mask = _padded(seqs, "left")
    free = model.generate(ids, attention_mask=mask, max_new_tokens=8)[:, 7:]
    eos = int(free[0, 1])  # sequence 0 emits it as its 2nd token
    stop = [free[b].tolist().index(eos) if eos in free[b].tolist() else None for b in range(3)]
    assert stop[0] is not None and stop[0] <= 1
    pad = 96
    out = model.generate(ids, attention_mask=mask, max_new_tokens=8, eos_token_id=eos, pad_token_id=pad)[:, 7:]
    for b in range(3):
        n = 8 if stop[b] is None else stop[b] + 1
        n = min(n, out.shape[1])
        assert torch.equal(out[b, :n], free[b, :n])          # unchanged up to and including eos
        assert (out[b, n:] == pad).all()                      # pad thereafter
    if all(s is not None for s in stop):
        assert out.shape[1] == max(stop) + 1                  # early stop when all are done
    # default pad is eos
    out2 = model.generate(ids, attention_mask=mask, max_new_tokens=8, eos_token_id=eos)[:, 7:]
    assert torch.equal(torch.where(out == pad, torch.full_like(out, eos), out), out2)

    # early stop: a 1-sequence batch whose sequence finishes
    one = model.generate(ids[:1], attention_mask=mask[:1], max_new_tokens=8, eos_token_id=eos)
    assert one.shape[1] == 7 + stop[0] + 1

    # ModelWrapper.generate: prompt trimmed, tokens counted as the reference does
    wrapper = ModelWrapper(None, dict(_kw("mqa", 1, "rope"), eos_token_id=eos), torch.float32, "flash_attention_2", False)
    wrapper.model.load_state_dict(model.state_dict())
    wrapper.eval()
    gen, counts = wrapper.generate({"input_ids": ids, "attention_mask": mask}, {"max_new_tokens": 8})
    assert torch.equal(gen, out2)
    assert counts == ((out2 != eos).sum(-1) + 1).tolist()


def test_sampling_is_seeded_and_topk1_is_greedy():
    model = _model()
    ids, mask = _padded(_prompts(), "left")
    kw = dict(attention_mask=mask, max_new_tokens=6, do_sample=True, temperature=0.8, top_k=20, top_p=0.9)
    a = model.generate(ids, generator=torch.Generator().manual_seed(7), **kw)
    b = model.generate(ids, generator=torch.Generator().manual_seed(7), **kw)
    c = model.generate(ids, generator=torch.Generator().manual_seed(8), **kw)
    assert torch.equal(a, b)
    assert not torch.equal(a, c)
    greedy = model.generate(ids, attention_mask=mask, max_new_tokens=6)
    k1 = model.generate(ids, attention_mask=mask, max_new_tokens=6, do_sample=True, top_k=1,
                        generator=torch.Generator().manual_seed(1))
    assert torch.equal(greedy, k1)


# ---------------------------------------------------------------------------
# what raises
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("impl", ["eager", "sdpa"])
def test_cache_needs_flash_attention_2(impl):
    model = _model(impl=impl)
    with pytest.raises(NotImplementedError, match="flash_attention_2"):
        model(input_ids=torch.ones(1, 3, dtype=torch.long), use_cache=True)


def test_cache_misuse_raises():
    model = _model()
    ids = torch.ones(2, 3, dtype=torch.long)
    with torch.no_grad():
        cache = model(input_ids=ids, use_cache=True).past_key_values
        with pytest.raises(NotImplementedError, match="chunked prefill"):
            model(input_ids=ids, past_key_values=cache, use_cache=True)
        with pytest.raises(ValueError, match="attention_mask"):
            model(input_ids=ids[:, :1], past_key_values=cache, attention_mask=torch.ones(2, 3, dtype=torch.long))
        with pytest.raises(ValueError, match="sequences"):
            model(input_ids=ids[:1, :1], past_key_values=cache)

        small = KVCache(model.config, 2, 4, torch.float32, "cpu")
        with pytest.raises(ValueError, match="overflow"):
            model(input_ids=torch.ones(2, 5, dtype=torch.long), past_key_values=small)
        model(input_ids=ids, past_key_values=small)
        model(input_ids=ids[:, :1], past_key_values=small)
        assert small.get_seq_length() == 4
        before = [k.clone() for k in small.k]
        with pytest.raises(ValueError, match="overflow"):
            model(input_ids=ids[:, :1], past_key_values=small)
        assert small.get_seq_length() == 4 and small.lengths.tolist() == [4, 4]
        assert all(torch.equal(a, b) for a, b in zip(before, small.k))

    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        model(input_ids=ids, use_cache=True)


def test_padding_free_refuses_cache_and_generate():
    torch.manual_seed(0)
    cfg = GPTDolomiteConfig(**_kw("mqa", 1, "rope"))
    cfg._attn_implementation = "flash_attention_2"
    model = GPTDolomiteForCausalLM(cfg, use_padding_free_transformer=True).eval()
    with pytest.raises(NotImplementedError):
        model(input_ids=[[1, 2, 3]], use_cache=True)
    with pytest.raises(NotImplementedError):
        model.generate(torch.ones(1, 3, dtype=torch.long))
    wrapper = ModelWrapper(None, _kw("mqa", 1, "rope"), torch.float32, "flash_attention_2", True)
    with pytest.raises(NotImplementedError, match="padding free"):
        wrapper.generate({"input_ids": torch.ones(1, 3, dtype=torch.long)}, {"max_new_tokens": 2})


def test_moe_keeps_refusing_the_cache():
    from dolomite_engine_amd.hf_models import MoEDolomiteConfig, MoEDolomiteForCausalLM

    torch.manual_seed(0)
    cfg = MoEDolomiteConfig(**_kw("mqa", 1, "rope"), num_experts=2, num_experts_per_tok=1)
    cfg._attn_implementation = "sdpa"
    model = MoEDolomiteForCausalLM(cfg).eval()
    with pytest.raises(AssertionError, match="out of scope"):
        model.transformer(torch.ones(1, 3, dtype=torch.long), use_cache=True)
    with pytest.raises(AssertionError, match="out of scope"):
        model.generate(torch.ones(1, 3, dtype=torch.long), max_new_tokens=2)
