"""float64 references and derived error bounds for the elementwise kernels,
shared by tests/test_gpu_elementwise_edges.py (HIP kernels) and
tests/test_property_cpu.py (the CPU branches of the same ops). Pure CPU
torch; nothing here touches a GPU.

Bounds come from the roundings involved (u = one rounding of the dtype),
never from what the code under test produces."""

import torch

import oracle

BF16, F32 = torch.bfloat16, torch.float32
SENTINEL = -777.0  # exactly representable in bf16
ADAM_HP = dict(lr=1e-3, b1=0.9, b2=0.95, eps=1e-8, wd=0.1)


def _within(name, got, ref, bound):
    """Print the worst error/bound ratio, then assert every element is in."""
    diff = (got.detach().cpu().double() - ref).abs()
    bad = ~(diff <= bound)  # NaN-safe: a NaN in got counts as out of bound
    ratio = float(torch.nan_to_num(diff / bound, nan=0.0, posinf=float("inf")).max()) if diff.numel() else 0.0
    print(f"MAXRATIO {name} {ratio:.3f}")
    assert not bad.any(), f"{name}: {int(bad.sum())} of {diff.numel()} out of bound, worst ratio {ratio:.3f}"


def _rand(g, shape, dtype, scale=1.0, shift=0.0):
    # asymmetric (shifted) seeded data, rounded to the tensor dtype
    return (torch.randn(*shape, generator=g) * scale + shift).to(dtype)


def _norm_inputs(kind, T, H, dtype, fused, seed):
    g = torch.Generator().manual_seed(seed)
    d = dict(
        x=_rand(g, (T, H), dtype, 1.0, 0.3),
        w=_rand(g, (H,), dtype, 0.1, 1.0),
        b=_rand(g, (H,), dtype, 0.1, 0.05) if kind == "ln" else None,
        dy=_rand(g, (T, H), dtype, 1.0, 0.1),
        res=_rand(g, (T, H), dtype, 0.7, -0.2) if fused else None,
        ds=_rand(g, (T, H), dtype, 0.5, 0.1) if fused else None,
    )
    return d


def norm_ref64(kind, inp, eps, dtype):
    """float64 reference. s is the tensor-dtype residual sum (the kernels
    round the fp32 sum to the dtype, as torch's CPU add does); RMSNorm's dw
    uses the normalized value cast to the dtype (cast before the weight)."""
    x, w, b, dy, res, ds = (inp[k] for k in ("x", "w", "b", "dy", "res", "ds"))
    s_t = x if res is None else x + res
    s, w64, dy64 = s_t.double(), w.double(), dy.double()
    wdy = w64 * dy64
    out = dict(s=s_t)
    if kind == "rms":
        rstd = torch.rsqrt(s.pow(2).mean(-1, keepdim=True) + eps)
        shat = s * rstd
        out["y"] = w64 * shat
        out["y_mag"] = out["y"].abs()
        dx = rstd * (wdy - shat * (wdy * shat).mean(-1, keepdim=True))
        out["dw"] = (dy64 * shat.to(dtype).double()).sum(0)
    else:
        mu = s.mean(-1, keepdim=True)
        rstd = torch.rsqrt((s - mu).pow(2).mean(-1, keepdim=True) + eps)
        xhat = (s - mu) * rstd
        out["y"] = xhat * w64 + b.double()
        # magnitude the fp32 evaluation noise of y scales with: its two terms,
        # plus the error of mu (relative to mean|s|) carried through rstd*w
        out["y_mag"] = (xhat * w64).abs() + b.double().abs() + rstd * w64.abs() * s.abs().mean(-1, keepdim=True)
        dx = rstd * (wdy - wdy.mean(-1, keepdim=True) - xhat * (wdy * xhat).mean(-1, keepdim=True))
        out["dw"] = (dy64 * xhat).sum(0)
        out["db"] = dy64.sum(0)
        out["mean"] = mu.squeeze(-1)
    out["dx"] = dx if ds is None else dx + ds.double()
    out["rstd"] = rstd.squeeze(-1)
    out["dy_norm"] = dy64.pow(2).sum(0).sqrt()
    return out


def norm_bounds(kind, ref, dtype, grads_fp32=False):
    """u = 2^-7 (bf16: two bf16 roundings) / 2^-20 (fp32: a handful of fp32
    roundings plus reduction-order noise).
      RMSNorm y : rounded twice (cast before the weight, then the store):
                  1.05*u*|y64| (5% for fp32 reduction-order noise) + a floor
                  of 2^-10 * u * max|y64|.
      LayerNorm y: rounded ONCE: bf16 1.05*2^-8*|y64|, plus the fp32
                  evaluation noise of (x-mu)*rstd*w + b, which scales with
                  the magnitude of its terms (not of their possibly
                  cancelling sum) and with the error of mu itself, an fp32
                  sum relative to mean|s|:
                  2^-18*(|xhat*w| + |b| + rstd*|w|*mean|s|). fp32: 2^-20 of
                  that magnitude (16 fp32 roundings' worth).
      dx        : u*(|ref| + max|ref| per row)
      dw, db    : u*(|ref| + ||dy[:,h]||_2). With grads_fp32 (the kernels'
                  fp32 sums, compared before the cast to the weight dtype)
                  LayerNorm's dw/db take the fp32 u = 2^-20 for bf16 inputs
                  too: no bf16 rounding enters them, they are fp32 sums of
                  fp32 products of exactly converted inputs. RMSNorm's bf16
                  dw keeps 2^-7: each term holds the bf16 cast of s_hat,
                  which may round the other way than the reference's."""
    u = 2.0**-7 if dtype == BF16 else 2.0**-20
    y = ref["y"]
    if kind == "rms":
        by = 1.05 * u * y.abs() + 2.0**-10 * u * y.abs().max()
    elif dtype == BF16:
        by = 1.05 * 2.0**-8 * y.abs() + 2.0**-18 * ref["y_mag"]
    else:
        by = 2.0**-20 * ref["y_mag"]
    dx = ref["dx"]
    b = dict(y=by, dx=u * (dx.abs() + dx.abs().max(-1, keepdim=True).values))
    uw = 2.0**-20 if (grads_fp32 and kind == "ln") else u
    b["dw"] = uw * (ref["dw"].abs() + ref["dy_norm"])
    if kind == "ln":
        b["db"] = uw * (ref["db"].abs() + ref["dy_norm"])
    return b


def check_norm_against_ref(tag, kind, got, ref, dtype):
    bounds = norm_bounds(kind, ref, dtype, grads_fp32=got["dw"].dtype == F32)
    for k in ("y", "dx", "dw") + (("db",) if kind == "ln" else ()):
        _within(f"{tag}.{k}", got[k], ref[k], bounds[k])
    if "rstd" not in got:  # the CPU branch (tests/test_property_cpu.py) keeps no statistics
        return
    # fp32 row statistics: a few fp32 roundings + the hardware rsqrt
    _within(f"{tag}.rstd", got["rstd"], ref["rstd"], 2.0**-20 * ref["rstd"].abs())
    if kind == "ln":
        _within(f"{tag}.mean", got["mean"], ref["mean"], 2.0**-20 * (ref["mean"].abs() + 1.0))


def _rope_tables(D, T):
    cos, sin = oracle.rope_cos_sin_ref(D, 32, 10000.0)
    pos = (torch.arange(T) * 5 + 3) % 32
    return cos[pos].contiguous(), sin[pos].contiguous()


def _rope_ref64(qkv, cos, sin, lo, direction):
    """float64 rotation of every q/k head in the packed row; returns the
    result (v columns copied) and |x1|+|x2| per rotated element (0 for v)."""
    x = qkv.double()
    out, mag = x.clone(), torch.zeros_like(x)
    h2 = lo.D // 2
    c, s = cos.double(), sin.double() * direction
    offs = [(h // lo.G) * lo.q_gstride + (h % lo.G) * lo.D for h in range(lo.H)]
    offs += [lo.k_off + j * lo.kv_hstride for j in range(lo.Hkv)]
    for off in offs:
        x1, x2 = x[:, off:off + h2], x[:, off + h2:off + lo.D]
        out[:, off:off + h2] = x1 * c[:, :h2] - x2 * s[:, :h2]
        out[:, off + h2:off + lo.D] = x2 * c[:, h2:] + x1 * s[:, h2:]
        mag[:, off:off + h2] = mag[:, off + h2:off + lo.D] = x1.abs() + x2.abs()
    return out, mag


def _rope_bound(ref64, mag, dtype):
    """bf16: one bf16 ulp of the float64 result rounded once to bf16.
    fp32: 4 * 2^-24 * (|x1| + |x2|). v columns (mag == 0) must be exact."""
    if dtype == F32:
        return 4 * 2.0**-24 * mag
    r = ref64.to(BF16).double()
    _, e = torch.frexp(r)  # |r| = m * 2^e, m in [0.5, 1): ulp = 2^(e-1-7)
    ulp = torch.where(r == 0, torch.zeros_like(r), torch.ldexp(torch.ones_like(r), e - 8))
    return torch.where(mag == 0, torch.zeros_like(r), ulp)


def _rope_rounded(ref64, dtype):
    return ref64.to(dtype).double()


def _ce_labels(g, T, V):
    labels = torch.randint(0, V, (T,), generator=g)
    labels[0], labels[1], labels[2] = 0, V - 1, -100
    if T > 4:
        labels[4] = -100
    return labels


def ce_ref64(logits, labels):
    x = logits.double()
    lse = torch.logsumexp(x, dim=-1)
    valid = labels != -100
    picked = x.gather(-1, labels.clamp_min(0).unsqueeze(-1)).squeeze(-1)
    row_loss = (lse - picked) * valid
    n_valid = int(valid.sum())
    onehot = torch.zeros_like(x).scatter_(-1, labels.clamp_min(0).unsqueeze(-1), 1.0)
    p = (x - lse.unsqueeze(-1)).exp()
    dlogits = (p - onehot) * valid.unsqueeze(-1) / n_valid
    return dict(x=x, lse=lse, row_loss=row_loss, picked=picked, loss=row_loss.sum() / n_valid,
                p=p, dlogits=dlogits, n_valid=n_valid, valid=valid)


def ce_bounds(ref, dtype):
    """fp32 evaluation of lse = max + log(sum exp(x - max)):
      - each exp argument carries ~2 fp32 roundings (subtract, scale by
        log2 e): relative error 2*|arg|*2^-24 of that term; terms below
        exp(-88) are flushed, so |arg| counts up to 88;
      - the online sum runs V/256 steps per thread, each one add and at
        most one running-max rescale, then 6 shuffle + 4 LDS steps, plus
        the hardware exp/log (~1 ulp each): (2*V/256 + 16) roundings, all
        terms positive;
      - the final add rounds relative to |lse|.
    p = exp(x - lse) inherits the lse error plus its own argument error,
    and is flushed to zero below the smallest normal fp32 (2^-126);
    dlogits = (p - onehot) * gs is then rounded ONCE to the dtype."""
    x, lse = ref["x"], ref["lse"]
    V = x.shape[1]
    rng = (x.max(-1).values - x.min(-1).values).clamp_max(88.0)
    b_lse = (2 * V / 256 + 16 + 2 * rng) * 2.0**-24 + 2.0**-23 * lse.abs()
    b_row = b_lse + 2.0**-23 * (lse.abs() + ref["picked"].abs())
    arg = (x - lse.unsqueeze(-1)).abs().clamp_max(88.0)
    b_p = ref["p"] * (b_lse.unsqueeze(-1) + (2 * arg + 4) * 2.0**-24) + 2.0**-126
    u_store = 1.01 * 2.0**-8 if dtype == BF16 else 2.0**-23
    gs = 1.0 / ref["n_valid"]
    b_d = (gs * b_p) * (1 + u_store) + u_store * ref["dlogits"].abs() + 2.0**-126
    b_d = b_d * ref["valid"].unsqueeze(-1)  # ignored rows: exactly zero
    b_loss = float(b_row.max()) + 2.0**-22 * abs(float(ref["loss"]))  # mean of T row losses in fp32
    return dict(lse=b_lse, row_loss=b_row * ref["valid"], dlogits=b_d, loss=b_loss)


def adamw_ref64(p0, grads, gs, steps, hp):
    """float64 restatement of torch.optim.AdamW (decoupled wd, bias-corrected
    moments), on the fp32 values the C ABI receives. Also accumulates the
    rounding budget of an fp32 evaluation, per element:
      m: every term passes <= 12 fp32 roundings in five steps -> 2^-20 of the
         sum of |terms| (m_abs: the same recurrence on |g|, since m itself
         may cancel);  v: two more per term (g*g, all positive) -> 2^-19*v;
      p: each step adds an update lr/bc1 * m / (sqrt(v/bc2) + eps). m's error
         enters through m_abs (second term below); the rest — half the
         relative error of v (2^-21.2), the fp32 bias corrections (1 - b^t
         cancels: <= 2^-22 for bc1, 2^-21.8 for sqrt(bc2)) and ~5 roundings
         of the expression itself — sums to 1.3*2^-20 < 2^-19 of |update|.
         p itself takes 3 roundings per step (decay multiply, subtract,
         store)."""
    f = lambda v: float(torch.tensor(v, dtype=F32))  # noqa: E731
    lr, b1, b2, eps, wd = (f(hp[k]) for k in ("lr", "b1", "b2", "eps", "wd"))
    p = p0.double().clone()
    m, v, m_abs, tol_p = (torch.zeros_like(p) for _ in range(4))
    for t in range(1, steps + 1):
        gr = grads[t - 1].double() * gs
        p = p * (1 - lr * wd)
        m = b1 * m + (1 - b1) * gr
        m_abs = b1 * m_abs + (1 - b1) * gr.abs()
        v = b2 * v + (1 - b2) * gr * gr
        bc1, bc2 = 1 - b1**t, 1 - b2**t
        denom = (v / bc2).sqrt() + eps
        upd = (lr / bc1) * m / denom
        p = p - upd
        tol_p = tol_p + 2.0**-19 * upd.abs() + (lr / bc1) * (2.0**-20 * m_abs) / denom + 3 * 2.0**-24 * p.abs()
    return dict(p=p, m=m, v=v, tol_p=tol_p, tol_m=2.0**-20 * m_abs, tol_v=2.0**-19 * v)
