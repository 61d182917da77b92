"""Several new tokens on a non-empty KV cache through the CPU branches (fp32,
tiny models): extend_attention against float64, the model's extend step
against the no-cache forward, chunked prefill and continued conversations in
generate() against the unchunked runs, and what still raises."""

import math

import pytest
import torch

from dolomite_engine_amd.hf_models import KVCache
from dolomite_engine_amd.model_wrapper import ModelWrapper
from dolomite_engine_amd.ops import QKVLayout, extend_attention, extend_num_splits
from tests.test_kv_cache_cpu import HEADS, POSITIONS, VOCAB, _kw, _model, _padded, _prompts


def _cache(model, B, max_length=32, multi_token=True):
    return KVCache(model.config, B, max_length, torch.float32, "cpu", multi_token=multi_token)


def _ids(shape, seed):
    return torch.randint(1, VOCAB, shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("head_type,Hkv", HEADS)
def test_extend_attention_cpu_against_float64(head_type, Hkv):
    H, D, S_cap, S = 4, 16, 32, 8
    past_n = [(0, 3), (5, 0), (1, 1), (9, 8), (0, 1)]
    B = len(past_n)
    lo = QKVLayout.make(H, Hkv, D, head_type)
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(B * S, lo.row_len, generator=g)
    k = torch.randn(B, S_cap, Hkv, D, generator=g)
    v = torch.randn(B, S_cap, Hkv, D, generator=g)
    for b, (past, n) in enumerate(past_n):
        k[b, past + n :] = float("nan")
        v[b, past + n :] = float("nan")
    # spans right-aligned in their S rows: gap rows in front of each
    end = torch.tensor([(b + 1) * S for b in range(B)], dtype=torch.int32)
    begin = end - torch.tensor([n for _, n in past_n], dtype=torch.int32)
    lens = torch.tensor([p + n for p, n in past_n], dtype=torch.int32)
    scale = 1.0 / math.sqrt(D)
    o = extend_attention(qkv, lo, begin, end, 8, k, v, lens, scale, 17)
    assert o.shape == (B * S, H * D) and not torch.isnan(o).any()
    q, _, _ = lo.unpack_cpu(qkv)
    want = torch.zeros(B * S, H, D, dtype=torch.float64)
    for b, (past, n) in enumerate(past_n):
        for i in range(n):
            row, see = int(begin[b]) + i, past + i + 1
            for h in range(H):
                j = h // (H // Hkv)
                p = torch.softmax((k[b, :see, j].double() @ q[row, h].double()) * scale, dim=0)
                want[row, h] = p @ v[b, :see, j].double()
    torch.testing.assert_close(o.double().view(-1, H, D), want, rtol=1e-5, atol=1e-6)
    assert extend_num_splits(16, QKVLayout.make(32, 1, 80, "mqa"), 4, 4096) == 16  # min(ceil(512/16), 64/4)


@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("head_type,Hkv", HEADS)
def test_prefill_extend_extend_logits_equal_no_cache(head_type, Hkv, pos):
    model = _model(head_type, Hkv, pos)
    ids = _ids((3, 8), 1)
    cache = _cache(model, 3)
    with torch.no_grad():
        plain = model(input_ids=ids).logits
        for a, e in ((0, 4), (4, 7), (7, 8)):
            out = model(input_ids=ids[:, a:e], past_key_values=cache, use_cache=True)
            assert out.past_key_values is cache
            torch.testing.assert_close(out.logits, plain[:, a:e])
    assert cache.get_seq_length() == 8 and cache.lengths.tolist() == [8] * 3 == cache.next_position.tolist()


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("pos", POSITIONS)
def test_generate_chunked_prefill_is_unchunked(pos, side):
    model = _model("gqa", 2, pos)
    ids, mask = _padded(_prompts(), side)  # lengths 7 / 1 / 4
    want = model.generate(ids, attention_mask=mask, max_new_tokens=6, eos_token_id=0)
    assert torch.equal(model.generate(ids, attention_mask=mask, max_new_tokens=6, eos_token_id=0,
                                      prefill_chunk_size=3), want)
    wrapper = ModelWrapper(None, dict(_kw("gqa", 2, pos), eos_token_id=0), torch.float32, "flash_attention_2", False)
    wrapper.model.load_state_dict(model.state_dict())
    wrapper.eval()
    gen, _ = wrapper.generate({"input_ids": ids, "attention_mask": mask},
                              {"max_new_tokens": 6, "prefill_chunk_size": 3, "past_key_values": None})
    assert torch.equal(gen, want[:, 7:])


@pytest.mark.parametrize("chunk", [None, 2])
def test_generate_continues_a_cached_conversation(chunk):
    model = _model()
    turn1, turn2 = _ids((2, 5), 3), _ids((2, 4), 4)
    cache = _cache(model, 2)
    with torch.no_grad():
        model(input_ids=turn1, past_key_values=cache, use_cache=True)
    got = model.generate(turn2, max_new_tokens=4, past_key_values=cache, prefill_chunk_size=chunk)
    want = model.generate(torch.cat([turn1, turn2], dim=1), max_new_tokens=4)
    assert torch.equal(got, want[:, 5:])
    assert cache.get_seq_length() == 12  # the last new token is not fed back


def test_default_positions_continue_explicit_ones():
    """Prefill left-padded with positions restarting at each first real token,
    then a right-padded chunk (one row all pad) with default positions."""
    model = _model("gqa", 2, "rope")
    ids, mask = _padded(_prompts(lens=(7, 1, 4, 2)), "left")
    pos = (mask.cumsum(-1) - 1).clamp(min=0)
    chunk = _ids((4, 3), 6)
    cmask = torch.tensor([[1, 1, 1], [1, 0, 0], [1, 1, 0], [0, 0, 0]])
    cpos = torch.tensor([[7, 8, 9], [1, 1, 1], [4, 5, 5], [2, 2, 2]])
    cache = _cache(model, 4)
    with torch.no_grad():
        model(input_ids=ids, attention_mask=mask, position_ids=pos, past_key_values=cache, use_cache=True)
        out = model(input_ids=chunk, attention_mask=cmask, past_key_values=cache, use_cache=True)
        assert cache.lengths.tolist() == [10, 2, 6, 2] == cache.next_position.tolist()
        assert cache.get_seq_length() == 10
        want = model(input_ids=torch.cat([ids, chunk], 1), attention_mask=torch.cat([mask, cmask], 1),
                     position_ids=torch.cat([pos, cpos], 1)).logits[:, 7:]
        torch.testing.assert_close(out.logits[cmask.bool()], want[cmask.bool()])
        # explicit positions of an extend step are what the next step continues
        model(input_ids=chunk[:, :2], position_ids=torch.tensor([[20, 21]] * 4), past_key_values=cache, use_cache=True)
    assert cache.next_position.tolist() == [22] * 4 and cache.lengths.tolist() == [12, 4, 8, 4]


def test_extend_refusals():
    model = _model()
    ids = _ids((2, 3), 7)
    bits = lambda cache: [t.clone().view(torch.int32) for t in cache.k + cache.v]
    with torch.no_grad():
        plain = _cache(model, 2, multi_token=False)
        model(input_ids=ids, past_key_values=plain, use_cache=True)
        with pytest.raises(NotImplementedError, match="chunked prefill.*multi_token"):
            model(input_ids=ids, past_key_values=plain, use_cache=True)

        cache = _cache(model, 2, max_length=8)
        model(input_ids=ids, past_key_values=cache, use_cache=True)
        with pytest.raises(ValueError, match="contiguous"):
            model(input_ids=ids, attention_mask=torch.tensor([[1, 0, 1], [1, 1, 1]]), past_key_values=cache)
        before = bits(cache)
        with pytest.raises(ValueError, match="overflow"):
            model(input_ids=_ids((2, 6), 8), past_key_values=cache, use_cache=True)
        with pytest.raises(ValueError, match="overflow"):  # 3 cached + 3 prompt + 3 new > 8
            model.generate(ids, max_new_tokens=3, past_key_values=cache)
        assert all(torch.equal(a, b) for a, b in zip(before, bits(cache)))
        assert cache.get_seq_length() == 3 and cache.lengths.tolist() == [3, 3]
    for impl in ("eager", "sdpa"):
        with pytest.raises(NotImplementedError, match="flash_attention_2"):
            _model(impl=impl).generate(ids, max_new_tokens=2, prefill_chunk_size=2)
