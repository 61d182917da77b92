"""Autograd ops over the dolomite_hip C-ABI.

Each torch.autograd.Function dispatches per device:
  - CUDA (= ROCm/HIP here): the hand-written gfx950 kernels via ctypes.
    A missing extension raises — no eager fallback on GPU.
  - CPU: a plain-torch restatement of the SAME math, so the identical
    padding-free graph (including the ZeRO-2 training loop) is exercisable
    in CPU tests. The reference itself cannot run its padding-free path on
    CPU (flash-attn gated, attention/padding_free.py:10); the CPU branch
    here is a test vehicle, never what bench.py or smoke() measures.

Reference anchors for the math are in include/dolomite_hip.h and
oracle/model.py.
"""

from dataclasses import dataclass

import torch

from . import hip


# ---------------------------------------------------------------------------
# Packed-QKV layout bookkeeping (attention/base.py:72-81 fused c_attn output)
# ---------------------------------------------------------------------------


@dataclass(frozen=True)
class QKVLayout:
    H: int      # query heads
    Hkv: int    # kv heads
    D: int      # head dim
    G: int      # query heads per kv group
    row_len: int
    q_gstride: int  # elements between q groups within a row
    k_off: int      # element offset of kv-head-0 K within a row
    kv_hstride: int # elements between kv heads (K->K and V->V)
    v_off: int      # element offset of kv-head-0 V within a row

    @staticmethod
    def make(H: int, Hkv: int, D: int, attention_head_type: str) -> "QKVLayout":
        """Mirrors the reference's per-head-type QKV split on the packed
        (T, h + 2*Hkv*D) c_attn output (attention/padding_free.py:79-116)."""
        row_len = H * D + 2 * Hkv * D
        if attention_head_type == "mha":
            # view (T, H, 3D): [q | k | v] per head
            return QKVLayout(H, Hkv, D, 1, row_len, 3 * D, D, 3 * D, 2 * D)
        if attention_head_type == "gqa":
            G = H // Hkv
            # view (T, Hkv, (G+2)D): [q*G | k | v] per group
            return QKVLayout(H, Hkv, D, G, row_len, (G + 2) * D, G * D, (G + 2) * D, (G + 1) * D)
        if attention_head_type == "mqa":
            # split (H*D, D, D)
            return QKVLayout(H, 1, D, H, row_len, 0, H * D, 0, H * D + D)
        raise ValueError(attention_head_type)

    def operands(self, qkv: torch.Tensor):
        """The q, k, v pointers of the C-ABI: head 0 of each in qkv's row 0."""
        return hip.ptr(qkv), hip.ptr(qkv, self.k_off), hip.ptr(qkv, self.v_off)

    def strides(self, token_stride: int | None = None):
        """The C-ABI's (q_tstride, q_gstride, k_tstride, k_hstride, v_tstride,
        v_hstride); token_stride defaults to the dense row_len."""
        ts = self.row_len if token_stride is None else token_stride
        return ts, self.q_gstride, ts, self.kv_hstride, ts, self.kv_hstride

    def unpack_cpu(self, qkv: torch.Tensor):
        """CPU view/reshape of packed qkv -> q (T,H,D), k/v (T,Hkv,D)
        (copies where the reference needs a reshape too)."""
        T = qkv.shape[0]
        H, Hkv, D, G = self.H, self.Hkv, self.D, self.G
        if G == 1:  # mha
            hs = qkv.view(T, Hkv, 3 * D)
            q, k, v = hs.chunk(3, dim=-1)
        elif self.Hkv > 1:  # gqa
            hs = qkv.view(T, Hkv, (G + 2) * D)
            q, k, v = hs.split((G * D, D, D), dim=-1)
            q = q.reshape(T, H, D)
        else:  # mqa
            q, k, v = qkv.split((H * D, D, D), dim=-1)
            q = q.view(T, H, D)
            k = k.unsqueeze(1)
            v = v.unsqueeze(1)
        return q.reshape(T, H, D), k.reshape(T, Hkv, D), v.reshape(T, Hkv, D)


# ---------------------------------------------------------------------------
# Fused (residual-add +) RMSNorm
# ---------------------------------------------------------------------------


def _rmsnorm_fwd_cpu(x, res, w, eps):
    s = x if res is None else x + res
    s32 = s.float()
    rstd = torch.rsqrt(s32.pow(2).mean(-1, keepdim=True) + eps)
    y = w * (s32 * rstd).to(x.dtype)
    return y, s, rstd.squeeze(-1)


def _rmsnorm_bwd_cpu(dy, s, w, rstd, dtype):
    s32 = s.float()
    r = rstd.unsqueeze(-1)
    shat = s32 * r
    wdy = (w * dy).float()
    dot = (wdy * shat).mean(-1, keepdim=True)
    dx = (r * (wdy - shat * dot)).to(dtype)
    dw = (dy.float() * shat.to(dtype).float()).sum(0).to(dtype)
    return dx, dw


def _norm_fwd_gpu(name, x2, residual, params, eps):
    """GPU forward of both fused norms. name: "rmsnorm" with params (weight,),
    or "layernorm" with params (weight, bias). Returns y, s and the fp32 row
    statistics the backward needs: [rstd], or [mean, rstd]."""
    rows, H = x2.shape
    x2 = x2.contiguous()
    res2 = residual.reshape(-1, H).contiguous() if residual is not None else None
    y = torch.empty_like(x2)
    # without a residual the pre-norm sum is x2 itself and res_out is null
    s = torch.empty_like(x2) if residual is not None else x2
    # rstd | mean, rstd: each norm keeps as many row statistics as it has parameters
    stats = [torch.empty(rows, dtype=torch.float32, device=x2.device) for _ in params]
    with hip.prof(f"{name}_fwd"):
        hip.check(
            getattr(hip.lib(), f"dolomite_{name}_fwd")(
                hip.stream(), hip.ptr(x2), hip.ptr(res2), *map(hip.ptr, params),
                hip.ptr(y), hip.ptr(s if residual is not None else None),
                *map(hip.ptr, stats), rows, H, float(eps), hip.dt(x2),
            ),
            f"{name}_fwd",
        )
    return y, s, stats


def _norm_bwd_gpu(name, dy2, ds, s, weight, stats):
    """GPU backward of both fused norms (stats as _norm_fwd_gpu returned them).
    Returns dx and the parameter grads in weight.dtype: [dw], or [dw, db]."""
    rows, H = s.shape
    dy2 = dy2.contiguous()
    ds2 = ds.reshape(-1, H).contiguous() if ds is not None else None
    dx = torch.empty_like(s)
    nb = hip.lib().dolomite_rmsnorm_bwd_nblocks(rows)
    # one block of nb partial rows per parameter grad: dw's, then layernorm's db's
    partial = torch.empty(len(stats) * nb, H, dtype=torch.float32, device=s.device)
    with hip.prof(f"{name}_bwd"):
        hip.check(
            getattr(hip.lib(), f"dolomite_{name}_bwd")(
                hip.stream(), hip.ptr(dy2), hip.ptr(s), hip.ptr(weight), *map(hip.ptr, stats),
                hip.ptr(dx), hip.ptr(partial),
                hip.ptr(ds2),  # residual-stream grad folded into dx in-kernel
                rows, H, hip.dt(s),
            ),
            f"{name}_bwd",
        )
    # fixed-order reduce (reduce_partials_ref): the grads are bitwise reproducible
    grads = [torch.empty(H, dtype=torch.float32, device=s.device) for _ in stats]
    with hip.prof("reduce_partials"):
        for i, g in enumerate(grads):
            hip.check(
                hip.lib().dolomite_reduce_partials(hip.stream(), hip.ptr(partial, i * nb * H), hip.ptr(g), nb, H),
                "reduce_partials",
            )
    return dx, [g.to(weight.dtype) for g in grads]


class FusedRMSNorm(torch.autograd.Function):
    """y, s = rmsnorm(x [+ residual]); s is the pre-norm sum (next residual).
    Semantics: rmsnorm/base.py:18-25 (fp32 accum, cast before weight)."""

    @staticmethod
    def forward(ctx, x, weight, eps, residual):
        H = x.shape[-1]
        x2 = x.reshape(-1, H)
        if x2.is_cuda:
            y, s, (rstd,) = _norm_fwd_gpu("rmsnorm", x2, residual, (weight,), eps)
        else:
            y, s, rstd = _rmsnorm_fwd_cpu(x2, residual.reshape(-1, H) if residual is not None else None, weight, eps)
        ctx.save_for_backward(s, weight, rstd)
        ctx.has_residual = residual is not None
        ctx.shape = x.shape
        return y.view(x.shape), s.view(x.shape)

    @staticmethod
    def backward(ctx, dy, ds):
        s, weight, rstd = ctx.saved_tensors
        H = s.shape[-1]
        dy2 = dy.reshape(-1, H)
        if s.is_cuda:
            dx, (dw,) = _norm_bwd_gpu("rmsnorm", dy2, ds, s, weight, (rstd,))
            dx = dx.view(ctx.shape)
        else:
            dx, dw = _rmsnorm_bwd_cpu(dy2, s, weight, rstd, dy.dtype)
            dx = dx.view(ctx.shape)
            if ds is not None:
                dx = dx + ds
        dres = dx if ctx.has_residual else None
        return dx, dw, None, dres


def fused_rmsnorm(x, weight, eps, residual=None):
    return FusedRMSNorm.apply(x, weight, eps, residual)


def reduce_partials_ref(partial: torch.Tensor) -> torch.Tensor:
    """The summation order of dolomite_reduce_partials (definition:
    include/dolomite_hip.h), restated with sequential fp32 adds on CPU.
    partial: (nblocks, H) fp32. fp32 adds are IEEE-exact on both sides, so
    the kernel's result equals this bit for bit."""
    p = partial.detach().to("cpu", torch.float32)
    nblocks, H = p.shape
    nsplit = max(1, min(32, -(-nblocks // 128)))
    chunk = -(-nblocks // nsplit)
    out = torch.zeros(H, dtype=torch.float32)
    for c in range(nsplit):
        acc = torch.zeros(H, dtype=torch.float32)
        for i in range(c * chunk, min((c + 1) * chunk, nblocks)):
            acc = torch.add(acc, p[i])
        if nsplit == 1:
            return acc
        if c * chunk < nblocks:
            out = torch.add(out, acc)
    return out


# ---------------------------------------------------------------------------
# Fused (residual-add +) LayerNorm
# ---------------------------------------------------------------------------


def _layernorm_fwd_cpu(x, res, w, b, eps):
    s = x if res is None else x + res
    s32 = s.float()
    mu = s32.mean(-1, keepdim=True)
    var = (s32 - mu).pow(2).mean(-1, keepdim=True)
    rstd = torch.rsqrt(var + eps)
    y = ((s32 - mu) * rstd * w.float() + b.float()).to(x.dtype)
    return y, s, mu.squeeze(-1), rstd.squeeze(-1)


class FusedLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps, residual):
        H = x.shape[-1]
        x2 = x.reshape(-1, H)
        if x2.is_cuda:
            y, s, (mean, rstd) = _norm_fwd_gpu("layernorm", x2, residual, (weight, bias), eps)
        else:
            y, s, mean, rstd = _layernorm_fwd_cpu(
                x2, residual.reshape(-1, H) if residual is not None else None, weight, bias, eps
            )
        ctx.save_for_backward(s, weight, mean, rstd)
        ctx.has_residual = residual is not None
        ctx.shape = x.shape
        return y.view(x.shape), s.view(x.shape)

    @staticmethod
    def backward(ctx, dy, ds):
        s, weight, mean, rstd = ctx.saved_tensors
        H = s.shape[-1]
        dy2 = dy.reshape(-1, H)
        if s.is_cuda:
            dx, (dw, db) = _norm_bwd_gpu("layernorm", dy2, ds, s, weight, (mean, rstd))
            dx = dx.view(ctx.shape)
        else:
            s32 = s.float()
            xhat = (s32 - mean.unsqueeze(-1)) * rstd.unsqueeze(-1)
            wdy = dy2.float() * weight.float()
            m1 = wdy.mean(-1, keepdim=True)
            m2 = (wdy * xhat).mean(-1, keepdim=True)
            dx = (rstd.unsqueeze(-1) * (wdy - m1 - xhat * m2)).to(dy.dtype)
            dw = (dy2.float() * xhat).sum(0).to(weight.dtype)
            db = dy2.float().sum(0).to(weight.dtype)
            dx = dx.view(ctx.shape)
            if ds is not None:
                dx = dx + ds
        dres = dx if ctx.has_residual else None
        return dx, dw, db, None, dres


def fused_layernorm(x, weight, bias, eps, residual=None):
    return FusedLayerNorm.apply(x, weight, bias, eps, residual)


# ---------------------------------------------------------------------------
# RoPE on the packed QKV buffer (in-place)
# ---------------------------------------------------------------------------


def _rope_cpu(qkv, cos, sin, lo: QKVLayout, inverse: bool):
    out = qkv.clone()
    q, k, _ = lo.unpack_cpu(out)
    D = lo.D
    c = cos.to(torch.float32)  # (T, D)
    s = sin.to(torch.float32) * (-1.0 if inverse else 1.0)

    def rot(x):  # x: (T, D)
        x32 = x.float()
        x1, x2 = x32.chunk(2, dim=-1)
        rotated = torch.cat((-x2, x1), dim=-1)
        return (x32 * c + rotated * s).to(x.dtype)

    # write back through the packed layout
    for h in range(lo.H):
        off = (h // lo.G) * lo.q_gstride + (h % lo.G) * D
        out[:, off : off + D] = rot(q[:, h]).to(qkv.dtype)
    for j in range(lo.Hkv):
        off = lo.k_off + j * lo.kv_hstride
        out[:, off : off + D] = rot(k[:, j]).to(qkv.dtype)
    return out


class RoPEPackedQKV(torch.autograd.Function):
    """In-place rotary embedding of q,k heads inside the packed c_attn output
    (rope.py:104-121 at padding_free.py:38-40). cos/sin: (T, D) fp32 gathered
    per token. Backward is the inverse rotation (R^T = -R; tables duplicated)."""

    @staticmethod
    def forward(ctx, qkv, cos, sin, layout: QKVLayout):
        ctx.layout = layout
        ctx.save_for_backward(cos, sin)
        if qkv.is_cuda:
            lo = layout
            hip.check(
                hip.lib().dolomite_rope_qkv(
                    hip.stream(), hip.ptr(qkv), hip.ptr(qkv), hip.ptr(cos), hip.ptr(sin),
                    qkv.shape[0], lo.row_len, lo.H, lo.Hkv, lo.D, lo.G,
                    lo.q_gstride, lo.k_off, lo.kv_hstride, 1, 0, hip.dt(qkv),
                ),
                "rope_qkv fwd",
            )
            ctx.mark_dirty(qkv)
            return qkv
        out = _rope_cpu(qkv, cos, sin, layout, inverse=False)
        return out

    @staticmethod
    def backward(ctx, dqkv):
        cos, sin = ctx.saved_tensors
        lo = ctx.layout
        if dqkv.is_cuda:
            # The incoming grad may be shared (the caller's own tensor, or a
            # grad autograd still holds for another consumer), so it is not
            # rotated in place: q,k go out of place through the kernel, which
            # leaves the v slots alone, and v (a sliver of the row) is copied.
            dqkv = dqkv.contiguous()
            T = dqkv.shape[0]
            out = torch.empty_like(dqkv)
            if T > 0:
                # as_strided offsets are absolute in the storage: add each
                # tensor's own (dqkv may be a slice of a larger buffer)
                size, stride = (T, lo.Hkv, lo.D), (lo.row_len, lo.kv_hstride, 1)
                out.as_strided(size, stride, out.storage_offset() + lo.v_off).copy_(
                    dqkv.as_strided(size, stride, dqkv.storage_offset() + lo.v_off)
                )
            hip.check(
                hip.lib().dolomite_rope_qkv(
                    hip.stream(), hip.ptr(dqkv), hip.ptr(out), hip.ptr(cos), hip.ptr(sin),
                    T, lo.row_len, lo.H, lo.Hkv, lo.D, lo.G,
                    lo.q_gstride, lo.k_off, lo.kv_hstride, -1, 0, hip.dt(dqkv),
                ),
                "rope_qkv bwd",
            )
            return out, None, None, None
        return _rope_cpu(dqkv, cos, sin, lo, inverse=True), None, None, None


def rope_packed_qkv(qkv, cos, sin, layout: QKVLayout):
    return RoPEPackedQKV.apply(qkv, cos, sin, layout)


# ---------------------------------------------------------------------------
# Varlen causal flash attention on the packed QKV buffer
# ---------------------------------------------------------------------------


_U32 = 0xFFFFFFFF
_DROP_CQ, _DROP_CK, _DROP_CH = 0x9E3779B1, 0x85EBCA77, 0xC2B2AE3D
_DROP_M1, _DROP_M2 = 0x7FEB352D, 0x846CA68B


def _drop_mix32(x: torch.Tensor) -> torch.Tensor:
    """The 32-bit avalanche mixer of the keep-mask on int64 lanes (values
    stay in [0, 2^32); int64 products wrap, the low 32 bits are exact)."""
    x = x ^ (x >> 16)
    x = (x * _DROP_M1) & _U32
    x = x ^ (x >> 15)
    x = (x * _DROP_M2) & _U32
    return x ^ (x >> 16)


def attention_dropout_threshold(p: float) -> int:
    """floor(p * 2^32) with p taken as the IEEE float32 the C-ABI receives."""
    p32 = float(torch.tensor(float(p), dtype=torch.float32))
    return int(p32 * 4294967296.0)


def attention_dropout_keep_mask(seed: int, H: int, tq, tk, p: float) -> torch.Tensor:
    """Attention-dropout keep mask, the torch-int64 restatement of the device
    function in csrc/attention.hip (definition: include/dolomite_hip.h).

    tq / tk: 1-D integer tensors of GLOBAL packed token indices. Returns a
    bool (H, len(tq), len(tk)) tensor on CPU: True = kept. Pure function of
    its arguments — the same bits the fwd/dkv/dq kernels regenerate."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    seed_lo, seed_hi = seed & _U32, seed >> 32
    tq = torch.as_tensor(tq, dtype=torch.int64).cpu() & _U32
    tk = torch.as_tensor(tk, dtype=torch.int64).cpu() & _U32
    h = torch.arange(H, dtype=torch.int64)
    rw = _drop_mix32(((tq * _DROP_CQ) & _U32) ^ seed_lo)                    # (nq,)
    hw = _drop_mix32(((h * _DROP_CH) & _U32) ^ seed_hi)                     # (H,)
    cw = _drop_mix32(((tk * _DROP_CK) & _U32)[None, :] ^ hw[:, None])       # (H, nk)
    x = rw[None, :, None] ^ cw[:, None, :]
    x = x ^ (x >> 16)
    x = (x * _DROP_M1) & _U32
    x = x ^ (x >> 15)
    x = (x * _DROP_M2) & _U32
    return x >= attention_dropout_threshold(p)


def draw_attention_dropout_seed() -> int:
    """One int64 from torch's default CPU generator: no device sync, restored
    with the checkpointed torch RNG state (bit-exact resume), and replayed by
    torch.utils.checkpoint's preserve_rng_state during block recompute."""
    return int(torch.randint(0, 2**63 - 1, (1,), dtype=torch.int64))


def _drop_scale(p: float) -> float:
    """1/(1-p) as the kernels compute it (float32 arithmetic)."""
    one = torch.tensor(1.0, dtype=torch.float32)
    return float(one / (one - torch.tensor(float(p), dtype=torch.float32)))


def _attn_fwd_cpu(qkv, begins, ends, scale, lo: QKVLayout, dropout_p: float = 0.0, seed: int = 0):
    """fp32-softmax causal attention + lse over the row spans
    [begins[i], ends[i]) of the packed qkv, CPU restatement of the kernel.
    Rows outside every span: o is zero, lse is zero (unspecified on GPU)."""
    q, k, v = lo.unpack_cpu(qkv)
    T = q.shape[0]
    o = torch.zeros(T, lo.H * lo.D, dtype=qkv.dtype)
    lse = torch.zeros(lo.H, T, dtype=torch.float32)
    for s, e in zip(begins, ends):
        if e == s:
            continue
        qi = q[s:e].float()
        ki = k[s:e].float()
        vi = v[s:e].float()
        L = e - s
        mask = torch.ones(L, L, dtype=torch.bool).tril()
        if dropout_p > 0:
            tok = torch.arange(s, e)
            keep = attention_dropout_keep_mask(seed, lo.H, tok, tok, dropout_p)
            rp = _drop_scale(dropout_p)
        for h in range(lo.H):
            j = h // (lo.H // lo.Hkv) if lo.Hkv > 1 else 0
            sc = (qi[:, h] @ ki[:, j].T) * scale
            sc = sc.masked_fill(~mask, float("-inf"))
            m = sc.max(-1, keepdim=True).values
            p = (sc - m).exp()
            l = p.sum(-1, keepdim=True)
            lse[h, s:e] = (m + l.log()).squeeze(-1)
            pn = p / l
            if dropout_p > 0:  # lse / the softmax itself are undropped
                pn = pn * keep[h] * rp
            o[s:e, h * lo.D : (h + 1) * lo.D] = (pn @ vi[:, j]).to(qkv.dtype)
    return o, lse


def _span_lists(seq_begin, seq_end):
    """SpanAttention's sequence bounds as (begins, ends) lists."""
    if seq_end is None:  # seq_begin is cu_seqlens
        cul = seq_begin.tolist()
        return cul[:-1], cul[1:]
    return seq_begin.tolist(), seq_end.tolist()


def _span_abi(seq_begin, seq_end):
    """SpanAttention's sequence bounds for the C-ABI: the entry points' family
    (fa_<kind>_fwd / _bwd, the hip.prof region names too), the batch and the
    bound pointers."""
    if seq_end is None:  # seq_begin is cu_seqlens
        return "varlen", seq_begin.shape[0] - 1, (hip.ptr(seq_begin),)
    return "spans", seq_begin.shape[0], (hip.ptr(seq_begin), hip.ptr(seq_end))


class SpanAttention(torch.autograd.Function):
    """Causal attention over row spans of the packed qkv (T, row_len):
    sequence b is rows [seq_begin[b], seq_end[b]). Output o (T, H*D); LSE
    saved for the recompute backward. Two callers, one set of kernels:

    seq_end=None, seq_begin = cu_seqlens (batch + 1,): back-to-back
    sequences, the flash_attn_varlen_func replacement (padding_free.py:51-62).
    Every row is in a span; the fa_varlen_* entry points.

    seq_begin, seq_end (batch,): sequences that are NOT back to back — a
    padded (B, S) batch viewed as B*S rows, run in place. The dense
    flash_attention_2 replacement (attention/flash.py:95-135) without its
    unpad / pad copies. Rows outside every span: o and dqkv are exactly zero
    (pad_input's semantics), by a gap-zeroing launch per buffer; the
    fa_spans_* entry points."""

    @staticmethod
    def forward(ctx, qkv, seq_begin, seq_end, max_seqlen: int, layout: QKVLayout, scale: float,
                dropout_p: float = 0.0, seed: int = 0):
        lo = layout
        T = qkv.shape[0]
        dropout_p = float(dropout_p)
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        if qkv.is_cuda:
            qkv = qkv.contiguous()
            o = torch.empty(T, lo.H * lo.D, dtype=qkv.dtype, device=qkv.device)
            lse = torch.empty(lo.H, T, dtype=torch.float32, device=qkv.device)
            kind, batch, bounds = _span_abi(seq_begin, seq_end)
            # the varlen entry point that takes (p_drop, seed); fa_spans_fwd
            # zeroes o's gap rows itself
            lib = hip.lib()
            fwd = lib.dolomite_fa_varlen_fwd_dropout if seq_end is None else lib.dolomite_fa_spans_fwd
            with hip.prof(f"fa_{kind}_fwd"):
                hip.check(
                    fwd(
                        hip.stream(), *lo.operands(qkv), hip.ptr(o), hip.ptr(lse), *bounds,
                        batch, int(max_seqlen), T, lo.H, lo.Hkv, lo.D, lo.G, *lo.strides(),
                        float(scale), hip.dt(qkv), dropout_p, seed,
                    ),
                    f"fa_{kind}_fwd",
                )
        else:
            o, lse = _attn_fwd_cpu(qkv, *_span_lists(seq_begin, seq_end), scale, lo, dropout_p, seed)
        ctx.save_for_backward(qkv, o, lse, seq_begin, seq_end)
        ctx.layout = lo
        ctx.scale = scale
        ctx.max_seqlen = int(max_seqlen)
        ctx.dropout_p = dropout_p
        ctx.seed = seed
        return o

    @staticmethod
    def backward(ctx, dout):
        qkv, o, lse, seq_begin, seq_end = ctx.saved_tensors
        lo: QKVLayout = ctx.layout
        T = qkv.shape[0]
        if qkv.is_cuda:
            dout = dout.contiguous()
            delta = torch.empty(lo.H, T, dtype=torch.float32, device=qkv.device)
            hip.check(
                hip.lib().dolomite_fa_bwd_preprocess(
                    hip.stream(), hip.ptr(o), hip.ptr(dout), hip.ptr(delta),
                    T, lo.H, lo.D, lo.H * lo.D, lo.H * lo.D, hip.dt(qkv),
                ),
                "fa_bwd_preprocess",
            )
            # (T, H, D) per-q-head partials. Span rows of the partials and of
            # dqkv are stored exclusively by the kernels (no zero-init needed);
            # gap rows are left as allocated, reduced as they are by the
            # finalize, and zeroed in dqkv afterwards (no whole-buffer memset:
            # the partials are the largest buffers of the step)
            dk_acc = torch.empty(T, lo.H, lo.D, dtype=torch.float32, device=qkv.device)
            dv_acc = torch.empty(T, lo.H, lo.D, dtype=torch.float32, device=qkv.device)
            dqkv = torch.empty_like(qkv)
            kind, batch, bounds = _span_abi(seq_begin, seq_end)
            lib = hip.lib()
            bwd = lib.dolomite_fa_varlen_bwd_dropout if seq_end is None else lib.dolomite_fa_spans_bwd
            with hip.prof(f"fa_{kind}_bwd"):
                hip.check(
                    bwd(
                        hip.stream(), *lo.operands(qkv), hip.ptr(dout), hip.ptr(lse), hip.ptr(delta),
                        hip.ptr(dqkv), hip.ptr(dk_acc), hip.ptr(dv_acc), *bounds,
                        batch, ctx.max_seqlen, T, lo.H, lo.Hkv, lo.D, lo.G, *lo.strides(), lo.H * lo.D,
                        float(ctx.scale), hip.dt(qkv), ctx.dropout_p, ctx.seed,
                    ),
                    f"fa_{kind}_bwd",
                )
            hip.check(
                hip.lib().dolomite_fa_grad_finalize(
                    hip.stream(), hip.ptr(dk_acc), hip.ptr(dv_acc), hip.ptr(dqkv),
                    T, lo.Hkv, lo.D, lo.G, lo.row_len,
                    lo.k_off, lo.kv_hstride, lo.v_off, hip.dt(qkv),
                ),
                "fa_grad_finalize",
            )
            if seq_end is not None:
                with hip.prof("fa_zero_gap_rows"):
                    hip.check(
                        hip.lib().dolomite_fa_zero_gap_rows(
                            hip.stream(), hip.ptr(dqkv), lo.row_len * dqkv.element_size(),
                            *bounds, batch, T,
                        ),
                        "fa_zero_gap_rows",
                    )
            return dqkv, None, None, None, None, None, None, None
        # CPU: differentiate the CPU restatement with torch autograd
        qkv_l = qkv.detach().requires_grad_(True)
        with torch.enable_grad():
            o2, _ = _attn_fwd_cpu_autograd(qkv_l, *_span_lists(seq_begin, seq_end), ctx.scale, lo,
                                           ctx.dropout_p, ctx.seed)
            (dqkv,) = torch.autograd.grad(o2, qkv_l, dout)
        return dqkv, None, None, None, None, None, None, None


def _attn_fwd_cpu_autograd(qkv, begins, ends, scale, lo: QKVLayout, dropout_p: float = 0.0, seed: int = 0):
    """Differentiable twin of _attn_fwd_cpu (spans ascending and disjoint):
    gap rows are constant zeros, so no gradient reaches their qkv rows."""
    q, k, v = lo.unpack_cpu(qkv)
    T = q.shape[0]
    pieces = []
    row = 0  # rows emitted so far
    for s, e in zip(begins, ends):
        if e == s:
            continue
        if s > row:
            pieces.append(qkv.new_zeros(s - row, lo.H * lo.D))
        row = e
        qi = q[s:e].float()
        ki = k[s:e].float()
        vi = v[s:e].float()
        L = e - s
        mask = torch.ones(L, L, dtype=torch.bool).tril()
        if dropout_p > 0:
            tok = torch.arange(s, e)
            keep = attention_dropout_keep_mask(seed, lo.H, tok, tok, dropout_p)
            rp = _drop_scale(dropout_p)
        hs = []
        for h in range(lo.H):
            j = h // (lo.H // lo.Hkv) if lo.Hkv > 1 else 0
            sc = (qi[:, h] @ ki[:, j].T) * scale
            sc = sc.masked_fill(~mask, float("-inf"))
            p = torch.softmax(sc, dim=-1)
            if dropout_p > 0:
                p = p * keep[h] * rp
            hs.append(p @ vi[:, j])
        pieces.append(torch.cat(hs, dim=-1).to(qkv.dtype))
    if T > row:
        pieces.append(qkv.new_zeros(T - row, lo.H * lo.D))
    o = torch.cat(pieces, dim=0) if pieces else qkv.new_zeros(0, lo.H * lo.D)
    return o, None


def _dropout_args(dropout_p, seed):
    """Validated (dropout_p, seed) of the attention wrappers; seed=None draws
    one, and only for dropout_p > 0: the RNG stream of p = 0 runs is untouched."""
    dropout_p = float(dropout_p)
    if not 0.0 <= dropout_p < 1.0:
        raise ValueError(f"dropout_p must be in [0, 1), got {dropout_p}")
    if dropout_p == 0.0:
        return 0.0, 0
    return dropout_p, draw_attention_dropout_seed() if seed is None else int(seed)


def varlen_attention(qkv, cu_seqlens, max_seqlen, layout: QKVLayout, scale: float,
                     dropout_p: float = 0.0, seed: int | None = None):
    """Causal varlen attention on the packed qkv. dropout_p > 0 drops
    attention probabilities with the counter-based keep mask
    (attention_dropout_keep_mask); seed=None draws one from torch's default
    CPU generator (draw_attention_dropout_seed)."""
    return SpanAttention.apply(qkv, cu_seqlens, None, int(max_seqlen), layout, scale,
                               *_dropout_args(dropout_p, seed))


def span_attention(qkv, seq_begin, seq_end, max_seqlen, layout: QKVLayout, scale: float,
                   dropout_p: float = 0.0, seed: int | None = None):
    """Causal attention over the row spans [seq_begin[b], seq_end[b]) of the
    packed qkv (T, row_len); int32 (batch,) tensors on qkv's device with
    0 <= begin <= end <= T, ascending and disjoint, empty spans allowed.
    max_seqlen is the longest span. Output (T, H*D) with zeros on the rows
    outside every span. Dropout as in varlen_attention: the keep mask is a
    function of the global row indices of the buffer."""
    dropout_p, seed = _dropout_args(dropout_p, seed)
    if seq_begin.shape != seq_end.shape or seq_begin.dim() != 1:
        raise ValueError("seq_begin and seq_end must be 1-D tensors of one length")
    if seq_begin.dtype != torch.int32 or seq_end.dtype != torch.int32:
        raise TypeError("seq_begin and seq_end must be int32")
    return SpanAttention.apply(qkv, seq_begin, seq_end, int(max_seqlen), layout, scale, dropout_p, seed)


# ---------------------------------------------------------------------------
# KV cache append + single-token decode attention (inference only)
# ---------------------------------------------------------------------------

DECODE_KEY_TILE = 64          # keys per wave step of the decode kernel
_DECODE_TARGET_WORKGROUPS = 512  # 2 per CU of the MI355X's 256


def _no_grad_inputs(name, *tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError(f"{name} is inference only (no backward): call it under torch.no_grad()")


def _check_cache(layout: QKVLayout, k_cache, v_cache):
    if k_cache.dim() != 4 or k_cache.shape != v_cache.shape or k_cache.shape[2:] != (layout.Hkv, layout.D):
        raise ValueError(
            f"k_cache / v_cache must both be (B, S_cap, Hkv={layout.Hkv}, D={layout.D}), "
            f"got {tuple(k_cache.shape)} and {tuple(v_cache.shape)}"
        )
    if k_cache.stride() != v_cache.stride() or k_cache.stride(3) != 1:
        raise ValueError("k_cache and v_cache must share strides, with a unit stride on the head dim")


def kv_cache_append(qkv, layout: QKVLayout, seq_begin, seq_end, k_cache, v_cache, dst_pos,
                    max_rows: int | None = None):
    """Copy the K and V slots of packed (RoPE'd) qkv rows into the cache, in
    place: row seq_begin[b] + i of qkv (T, row_len) goes to cache position
    dst_pos[b] + i of sequence b, for i in [0, seq_end[b] - seq_begin[b]).
    k_cache / v_cache: (B, S_cap, Hkv, D) in qkv's dtype. A position >= S_cap
    is skipped; nothing else in the cache is touched. seq_begin, seq_end,
    dst_pos: (B,) int32 on qkv's device. max_rows bounds the longest span
    (launch sizing on the GPU; default T). Serves the prefill (the span
    arrays, dst_pos = 0) and the decode step (one row per sequence)."""
    lo = layout
    _no_grad_inputs("kv_cache_append", qkv, k_cache, v_cache)
    _check_cache(lo, k_cache, v_cache)
    B, S_cap = k_cache.shape[:2]
    for name, t in (("seq_begin", seq_begin), ("seq_end", seq_end), ("dst_pos", dst_pos)):
        if t.dtype != torch.int32 or t.shape != (B,):
            raise TypeError(f"{name} must be an int32 tensor of shape ({B},)")
    if qkv.dim() != 2 or qkv.shape[1] != lo.row_len or qkv.dtype != k_cache.dtype:
        raise ValueError("qkv must be (T, row_len) in the cache dtype")
    T = qkv.shape[0]
    max_rows = T if max_rows is None else min(int(max_rows), T)
    if qkv.is_cuda:
        qkv = qkv.contiguous()
        with hip.prof("kv_cache_append"):
            hip.check(
                hip.lib().dolomite_kv_cache_append(
                    hip.stream(), hip.ptr(qkv), hip.ptr(seq_begin), hip.ptr(seq_end), hip.ptr(dst_pos),
                    hip.ptr(k_cache), hip.ptr(v_cache), B, max_rows, lo.Hkv, lo.D, S_cap,
                    lo.row_len, lo.k_off, lo.v_off, lo.kv_hstride,
                    k_cache.stride(0), k_cache.stride(1), k_cache.stride(2), hip.dt(qkv),
                ),
                "kv_cache_append",
            )
        return
    _, k, v = lo.unpack_cpu(qkv)
    for b, (s, e, p) in enumerate(zip(seq_begin.tolist(), seq_end.tolist(), dst_pos.tolist())):
        n = min(e - s, max_rows, S_cap - p)
        if n > 0:
            k_cache[b, p : p + n] = k[s : s + n]
            v_cache[b, p : p + n] = v[s : s + n]


def decode_num_splits(batch: int, layout: QKVLayout, max_len: int) -> int:
    """The split count decode_attention picks for num_splits=None."""
    tiles = -(-max(int(max_len), 1) // DECODE_KEY_TILE)
    base = max(batch, 1) * layout.Hkv * -(-layout.G // 32)
    return max(1, min(-(-_DECODE_TARGET_WORKGROUPS // base), -(-tiles // 4)))


def decode_attention(qkv, layout: QKVLayout, k_cache, v_cache, cache_len, scale: float, max_len: int,
                     num_splits: int | None = None):
    """Attention of ONE new token per sequence over its cached keys.
    qkv: (B, row_len) packed rows of the new tokens (only the q slots are
    read; their K/V are already in the cache). k_cache / v_cache:
    (B, S_cap, Hkv, D). cache_len: (B,) int32, the valid keys of each
    sequence including the new token. No causal mask: keys [0, cache_len[b])
    are attended, everything behind them is ignored whatever it holds.
    cache_len[b] == 0 gives a zero row. max_len: host upper bound on
    cache_len, <= S_cap. Returns (B, H*D).

    num_splits: workgroups along the keys (split-KV, combined in ascending
    split order — bitwise reproducible). None picks
        min(ceil(512 / (B * Hkv * ceil(G / 32))), ceil(ceil(max_len / 64) / 4))
    (at least 1): enough splits for about two workgroups on each of the 256
    CUs, but never less than four 64-key tiles (one per wave) in a split.
    Inference only: no backward."""
    lo = layout
    _no_grad_inputs("decode_attention", qkv, k_cache, v_cache)
    _check_cache(lo, k_cache, v_cache)
    B, S_cap = k_cache.shape[:2]
    if qkv.dim() != 2 or qkv.shape != (B, lo.row_len):
        raise ValueError(f"qkv must be (B, row_len) = {(B, lo.row_len)}, got {tuple(qkv.shape)}")
    if cache_len.dtype != torch.int32 or cache_len.shape != (B,):
        raise TypeError(f"cache_len must be an int32 tensor of shape ({B},)")
    max_len = int(max_len)
    if not 0 <= max_len <= S_cap:
        raise ValueError(f"max_len {max_len} outside [0, S_cap = {S_cap}]")
    if not scale > 0:
        raise ValueError("scale must be > 0")
    nsplit = decode_num_splits(B, lo, max_len) if num_splits is None else int(num_splits)
    if nsplit < 1:
        raise ValueError("num_splits must be >= 1")
    if qkv.is_cuda:
        qkv = qkv.contiguous()
        o = torch.empty(B, lo.H * lo.D, dtype=qkv.dtype, device=qkv.device)
        scratch = None
        if nsplit > 1:
            n = hip.lib().dolomite_fa_decode_scratch_floats(B, lo.H, lo.D, nsplit)
            scratch = torch.empty(n, dtype=torch.float32, device=qkv.device)
        with hip.prof("fa_decode"):
            hip.check(
                hip.lib().dolomite_fa_decode(
                    hip.stream(), hip.ptr(qkv), hip.ptr(k_cache), hip.ptr(v_cache), hip.ptr(o),
                    hip.ptr(scratch), hip.ptr(cache_len), B, lo.H, lo.Hkv, lo.D, lo.G, max_len, nsplit,
                    lo.row_len, lo.q_gstride,
                    k_cache.stride(0), k_cache.stride(1), k_cache.stride(2),
                    v_cache.stride(0), v_cache.stride(1), v_cache.stride(2),
                    float(scale), hip.dt(qkv),
                ),
                "fa_decode",
            )
        return o
    # CPU restatement: fp32 math, one sequence at a time
    q, _, _ = lo.unpack_cpu(qkv)
    G = lo.H // lo.Hkv
    o = torch.zeros(B, lo.H, lo.D, dtype=torch.float32)
    for b, n in enumerate(cache_len.tolist()):
        n = min(max(n, 0), max_len)
        if n == 0:
            continue
        kb = k_cache[b, :n].float().repeat_interleave(G, dim=1)  # (n, H, D)
        vb = v_cache[b, :n].float().repeat_interleave(G, dim=1)
        sc = torch.einsum("hd,nhd->hn", q[b].float(), kb) * scale
        o[b] = torch.einsum("hn,nhd->hd", torch.softmax(sc, dim=-1), vb)
    return o.reshape(B, lo.H * lo.D).to(qkv.dtype)


# ---------------------------------------------------------------------------
# Fused cross entropy (mean over non-ignored rows)
# ---------------------------------------------------------------------------


class FusedCrossEntropy(torch.autograd.Function):
    """F.cross_entropy(mean, ignore_index=-100) replacement
    (model_wrapper/pretraining.py:125 / gpt_dolomite/main.py:200).
    Backward recomputes softmax from logits + saved lse (no softmax tensor
    materialized in forward)."""

    @staticmethod
    def forward(ctx, logits, labels, ignore_index: int = -100):
        T, V = logits.shape
        if logits.is_cuda:
            row_stride = logits.stride(0)
            assert logits.stride(1) == 1 and (T <= 1 or row_stride >= V), "logits rows must be dense and disjoint"
            row_loss = torch.empty(T, dtype=torch.float32, device=logits.device)
            lse = torch.empty(T, dtype=torch.float32, device=logits.device)
            with hip.prof("ce_fwd"):
             hip.check(
                hip.lib().dolomite_ce_fwd(
                    hip.stream(), hip.ptr(logits), hip.ptr(labels), hip.ptr(row_loss),
                    hip.ptr(lse), T, V, row_stride, ignore_index, hip.dt(logits),
                ),
                "ce_fwd",
            )
        else:
            l32 = logits.float()
            lse = torch.logsumexp(l32, dim=-1)
            valid = labels != ignore_index
            picked = l32.gather(-1, labels.clamp_min(0).unsqueeze(-1)).squeeze(-1)
            row_loss = (lse - picked) * valid
        n_valid = (labels != ignore_index).sum()
        loss = row_loss.sum() / n_valid
        ctx.save_for_backward(logits, labels, lse, n_valid)
        ctx.ignore_index = ignore_index
        return loss

    @staticmethod
    def backward(ctx, gout):
        logits, labels, lse, n_valid = ctx.saved_tensors
        T, V = logits.shape
        if logits.is_cuda:
            # device-side scale: no host readback of gout/n_valid
            gs_dev = (gout.float() / n_valid.float()).reshape(1).contiguous()
            # the kernel reads logits and writes dlogits with ONE row stride:
            # give dlogits the logits' stride (empty_like of a row-strided
            # view would be dense, and the kernel would write past its end)
            row_stride = logits.stride(0)
            dlogits = torch.empty_strided((T, V), (row_stride, 1), dtype=logits.dtype, device=logits.device)
            with hip.prof("ce_bwd"):
             hip.check(
                hip.lib().dolomite_ce_bwd(
                    hip.stream(), hip.ptr(logits), hip.ptr(labels), hip.ptr(lse),
                    hip.ptr(dlogits), hip.ptr(gs_dev), T, V, row_stride,
                    ctx.ignore_index, hip.dt(logits),
                ),
                "ce_bwd",
            )
        else:
            gs = float(gout) / float(n_valid)
            p = torch.softmax(logits.float(), dim=-1)
            onehot = torch.zeros_like(p)
            onehot.scatter_(-1, labels.clamp_min(0).unsqueeze(-1), 1.0)
            valid = (labels != ctx.ignore_index).unsqueeze(-1)
            dlogits = ((p - onehot) * valid * gs).to(logits.dtype)
        return dlogits, None, None


def fused_cross_entropy(logits, labels, ignore_index: int = -100):
    return FusedCrossEntropy.apply(logits, labels, ignore_index)


# ---------------------------------------------------------------------------
# Fused AdamW on a flat fp32 master shard (not an autograd op)
# ---------------------------------------------------------------------------


def adamw_step_flat(master, grad, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, weight_decay, param_out=None,
                    grad_scale=None):
    """torch.optim.AdamW semantics on flat fp32 tensors, optional bf16
    write-out of the updated params (the ZeRO-2 local shard step).
    grad may be bf16 (the flat autograd bucket) — the kernel upcasts per
    element. grad_scale: optional 0-dim DEVICE tensor (the grad-clip
    coefficient) fused into the kernel's grad read."""
    if master.is_cuda:
        hip.check(
            hip.lib().dolomite_adamw_step(
                hip.stream(), hip.ptr(master), hip.ptr(param_out), hip.ptr(grad),
                hip.dt(grad), hip.ptr(exp_avg), hip.ptr(exp_avg_sq),
                master.numel(), float(lr), float(beta1), float(beta2), float(eps),
                float(weight_decay), int(step), hip.ptr(grad_scale),
            ),
            "adamw_step",
        )
        return
    g = grad.float()
    if grad_scale is not None:
        g = g * float(grad_scale)
    master.mul_(1 - lr * weight_decay)
    exp_avg.mul_(beta1).add_(g, alpha=1 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1 - beta1**step
    bc2 = 1 - beta2**step
    denom = (exp_avg_sq / bc2).sqrt().add_(eps)
    master.addcdiv_(exp_avg, denom, value=-(lr / bc1))
    if param_out is not None:
        param_out.copy_(master.to(param_out.dtype))


# ---------------------------------------------------------------------------
# Grouped expert GEMM (MoE) — replaces the reference's scattermoe grouped
# path (moe_dolomite/moe/scatter.py:109-138) for the SparseMoE expert
# matmuls (moe/base.py:137-156). Input rows are expert-sorted; `offsets`
# is the (E+1,) int32 cumulative group boundary array on device.
# ---------------------------------------------------------------------------


class GroupedExpertGemm(torch.autograd.Function):
    """y[t] = x[t] @ W[e(t)]^T (+ b[e(t)]); one HIP launch over all experts.

    backward: dX via the dgrad kernel, dW via the wgrad kernel, db via
    per-expert segment sums (E is small)."""

    @staticmethod
    def forward(ctx, x, weight, bias, offsets, max_rows):
        E, N, K = weight.shape
        # the kernels index weight as dense (E, N, K) and bias as dense (E, N)
        weight = weight.contiguous()
        bias = bias.contiguous() if bias is not None else None
        y = torch.empty(x.shape[0], N, dtype=x.dtype, device=x.device)
        with hip.prof("moe_gemm_fwd"):
            hip.check(
                hip.lib().dolomite_moe_gemm_fwd(
                    hip.stream(), hip.ptr(x), hip.ptr(weight),
                    hip.ptr(bias) if bias is not None else None, hip.ptr(y),
                    hip.ptr(offsets), E, int(max_rows), N, K, hip.dt(x),
                ),
                "moe_gemm_fwd",
            )
        ctx.save_for_backward(x, weight, offsets)
        ctx.max_rows = int(max_rows)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, offsets = ctx.saved_tensors
        E, N, K = weight.shape
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        with hip.prof("moe_gemm_dgrad"):
            hip.check(
                hip.lib().dolomite_moe_gemm_dgrad(
                    hip.stream(), hip.ptr(dy), hip.ptr(weight), hip.ptr(dx),
                    hip.ptr(offsets), E, ctx.max_rows, N, K, hip.dt(dy),
                ),
                "moe_gemm_dgrad",
            )
        dw = torch.empty(weight.shape, dtype=weight.dtype, device=weight.device)
        with hip.prof("moe_gemm_wgrad"):
            hip.check(
                hip.lib().dolomite_moe_gemm_wgrad(
                    hip.stream(), hip.ptr(dy), hip.ptr(x), hip.ptr(dw),
                    hip.ptr(offsets), E, N, K, hip.dt(dy),
                ),
                "moe_gemm_wgrad",
            )
        db = None
        if ctx.has_bias:
            off = offsets.tolist()
            db = torch.stack([dy[off[e]:off[e + 1]].sum(0) for e in range(E)])
        return dx, dw, db, None, None


class MoERowsGather(torch.autograd.Function):
    """expert_inputs = x[batch_index] with a deterministic, roofline-rate
    backward: torch's indexing backward for this pattern (indexing_backward
    / indexFuncLargeIndex) runs ~9x off the HBM roofline; the combine
    kernel sums each token's top-k slot rows in FIXED order instead
    (moe/base.py:108-127 semantics)."""

    @staticmethod
    def forward(ctx, x, batch_index, inv, k_top):
        ctx.save_for_backward(batch_index, inv)
        ctx.k_top = k_top
        ctx.total_q = x.shape[0]
        return x[batch_index]

    @staticmethod
    def backward(ctx, dexp):
        batch_index, inv = ctx.saved_tensors
        dx = _rows_combine(dexp, inv, batch_index, ctx.total_q, ctx.k_top)
        return dx, None, None, None


class MoERowsCombine(torch.autograd.Function):
    """out = zeros(total_q, K).index_add(0, batch_index, h)
    (moe/base.py:127) with the deterministic combine kernel on the forward
    and a plain gather backward."""

    @staticmethod
    def forward(ctx, h, inv, batch_index, total_q, k_top):
        ctx.save_for_backward(batch_index)
        return _rows_combine(h, inv, batch_index, total_q, k_top)

    @staticmethod
    def backward(ctx, dout):
        (batch_index,) = ctx.saved_tensors
        return dout[batch_index], None, None, None, None


def _rows_combine(h, inv, batch_index, total_q, k_top):
    h = h.contiguous()
    if h.is_cuda and h.dtype == torch.bfloat16 and h.shape[1] % 8 == 0:
        out = torch.empty(total_q, h.shape[1], dtype=h.dtype, device=h.device)
        hip.check(
            hip.lib().dolomite_moe_rows_combine(
                hip.stream(), hip.ptr(h), hip.ptr(inv), hip.ptr(out),
                total_q, h.shape[1], k_top, hip.dt(h),
            ),
            "moe_rows_combine",
        )
        return out
    return torch.zeros(total_q, h.shape[1], dtype=h.dtype, device=h.device).index_add(0, batch_index, h)


def grouped_expert_gemm(x, weight, bias, num_tokens_per_expert):
    """Dispatch helper: HIP grouped kernel when x, weight and bias are all
    CUDA bf16 and the dims 8-aligned (one launch for all experts); returns
    None if unsupported so the caller can fall back to the eager per-expert
    loop. weight and bias may be strided views: the kernels get dense copies."""
    E, N, K = weight.shape
    tensors = (x, weight) if bias is None else (x, weight, bias)
    if not all(t.is_cuda and t.dtype == torch.bfloat16 for t in tensors):
        return None
    if K % 8 != 0 or N % 8 != 0:
        return None
    # Measured crossover (tools_moe_gemm_probe.py, 1xMI355X): the one-launch
    # grouped kernel wins up to ~6x when per-expert GEMMs are small/launch-
    # bound (E=32, 512 rows/expert: 342 vs 54 TF), while the per-expert
    # rocBLAS loop wins for few large experts (E=8, 4096 rows/expert:
    # 630 vs 373 TF) — route the large-expert regime to the eager loop.
    if E <= 16 and x.shape[0] // max(E, 1) >= 2048:
        return None
    offsets = torch.zeros(E + 1, dtype=torch.int32, device=x.device)
    offsets[1:] = num_tokens_per_expert.cumsum(0).to(torch.int32)
    max_rows = int(num_tokens_per_expert.max())
    if max_rows == 0:
        return torch.zeros(x.shape[0], N, dtype=x.dtype, device=x.device)
    return GroupedExpertGemm.apply(x.contiguous(), weight, bias, offsets, max_rows)
