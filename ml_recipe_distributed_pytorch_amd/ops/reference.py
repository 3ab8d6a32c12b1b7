"""Pure-PyTorch implementations of every fused op (CPU path + numerics oracle).

Each function has the same signature and the same side effects (grad accumulation into fp32
arena views) as its HIP kernel twin in ``csrc/kernels``.  Math is done in fp32; outputs are
cast to the compute dtype of the activations.  Dropout masks come from ``ops.rng`` so the CPU
and GPU paths draw *identical* masks for the same (seed, opid).

Semantics follow HF ``BertModel`` as used by the reference (``modules/model/model/model.py:20-25``):
erf GELU, LayerNorm with fp32 statistics, additive ``-10000`` key mask, dropout after the
embedding LayerNorm, on attention probabilities, and before each residual add.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from . import f32 as _f32
from . import rng

Tensor = torch.Tensor


def _acc(dst: Optional[Tensor], val: Tensor, accumulate: bool) -> None:
    if dst is None:
        return
    if accumulate:
        dst.add_(val.to(dst.dtype))
    else:
        dst.copy_(val.to(dst.dtype))


def _drop_keep(shape, seed, opid, p, device):
    if p <= 0.0:
        return None
    return rng.keep_mask(shape, seed, opid, p, device=device).to(torch.float32) * rng.keep_scale(p)


def _ln_stats(x: Tensor, eps: float):
    mean = x.mean(-1)
    var = ((x - mean[:, None]) ** 2).mean(-1)
    rstd = torch.rsqrt(var + eps)
    return mean, rstd


def _ln_bwd_core(g: Tensor, xhat: Tensor, gamma: Tensor, rstd: Tensor) -> Tensor:
    dxhat = g * gamma.float()[None, :]
    return rstd[:, None] * (dxhat - dxhat.mean(-1, keepdim=True) - xhat * (dxhat * xhat).mean(-1, keepdim=True))


# ------------------------------------------------------------------------------------ embedding
def embed_fwd(ids, pos_ids, type_ids, w_word, w_pos, w_type, gamma, beta, eps, p, seed, opid, out_dtype):
    x = w_word.float()[ids] + w_pos.float()[pos_ids] + w_type.float()[type_ids]
    mean, rstd = _ln_stats(x, eps)
    y = (x - mean[:, None]) * rstd[:, None] * gamma.float()[None] + beta.float()[None]
    keep = _drop_keep(y.shape, seed, opid, p, y.device)
    if keep is not None:
        y = y * keep
    return y.to(out_dtype), mean, rstd


def embed_bwd(dy, ids, pos_ids, type_ids, w_word, w_pos, w_type, gamma, mean, rstd, p, seed, opid,
              g_word, g_pos, g_type, g_gamma, g_beta, accumulate: bool, pad_word: int = -1, pad_pos: int = -1):
    """``pad_word``/``pad_pos``: rows that receive no gradient (nn.Embedding ``padding_idx``; -1 = none)."""
    x = w_word.float()[ids] + w_pos.float()[pos_ids] + w_type.float()[type_ids]
    xhat = (x - mean[:, None]) * rstd[:, None]
    g = dy.float()
    keep = _drop_keep(g.shape, seed, opid, p, g.device)
    if keep is not None:
        g = g * keep
    _acc(g_gamma, (g * xhat).sum(0), accumulate)
    _acc(g_beta, g.sum(0), accumulate)
    dx = _ln_bwd_core(g, xhat, gamma, rstd)
    for table, idx, pad in ((g_word, ids, pad_word), (g_pos, pos_ids, pad_pos), (g_type, type_ids, -1)):
        if table is None:
            continue
        if not accumulate:
            table.zero_()
        src = dx if pad < 0 else dx * (idx != pad).to(dx.dtype)[:, None]
        table.index_add_(0, idx, src.to(table.dtype))


# ------------------------------------------------------------------ residual + dropout + LayerNorm
def ln_fwd(a, resid, gamma, beta, eps, p, seed, opid):
    """z = dropout(a) + resid ; y = LN(z).  Returns (y, z, mean, rstd)."""
    af = a.float()
    keep = _drop_keep(af.shape, seed, opid, p, af.device)
    if keep is not None:
        af = af * keep
    z = af + resid.float()
    mean, rstd = _ln_stats(z, eps)
    y = (z - mean[:, None]) * rstd[:, None] * gamma.float()[None] + beta.float()[None]
    return y.to(a.dtype), z.to(a.dtype), mean, rstd


def ln_bwd(dy, dy2, z, gamma, mean, rstd, p, seed, opid, g_gamma, g_beta, g_bias, accumulate: bool, beta=None):
    """Returns (dz, da): dz = dL/dz (residual grad), da = dropout_bwd(dz) (GEMM-output grad).  With ``beta``,
    ``z`` is the forward output y and x̂ = (y − β)/γ (0 where γ = 0), as the GPU kernel's FROMY form."""
    g = dy.float()
    if dy2 is not None:
        g = g + dy2.float()
    if beta is not None:
        gf = gamma.float()
        ig = torch.where(gf != 0, 1.0 / gf, torch.zeros_like(gf))
        xhat = z.float() * ig[None] - (beta.float() * ig)[None]
    else:
        xhat = (z.float() - mean[:, None]) * rstd[:, None]
    _acc(g_gamma, (g * xhat).sum(0), accumulate)
    _acc(g_beta, g.sum(0), accumulate)
    dz = _ln_bwd_core(g, xhat, gamma, rstd)
    keep = _drop_keep(dz.shape, seed, opid, p, dz.device)
    da = dz * keep if keep is not None else dz
    _acc(g_bias, da.sum(0), accumulate)
    return dz.to(dy.dtype), da.to(dy.dtype)


# ------------------------------------------------------------------------------------------ GELU
_INV_SQRT2 = 1.0 / math.sqrt(2.0)
_INV_SQRT2PI = 1.0 / math.sqrt(2.0 * math.pi)


def gelu_fwd(pre):
    x = pre.float()
    return (0.5 * x * (1.0 + torch.erf(x * _INV_SQRT2))).to(pre.dtype)


def gelu_bwd(dout, pre, g_bias, accumulate: bool):
    x = pre.float()
    d = dout.float() * (0.5 * (1.0 + torch.erf(x * _INV_SQRT2)) + x * torch.exp(-0.5 * x * x) * _INV_SQRT2PI)
    _acc(g_bias, d.sum(0), accumulate)
    return d.to(dout.dtype)


# ------------------------------------------------------------------------------------- attention
def _split_qkv(qkv, B, L, nh):
    H = qkv.shape[1] // 3
    dh = H // nh
    t = qkv.float().view(B, L, 3, nh, dh).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def _attn_keep(B, nh, L, seed, opid, p, device):
    return _drop_keep((B, nh, L, L), seed, opid, p, device)


def attn_fwd(qkv, key_bias, B, L, nh, p, seed, opid, scale):
    q, k, v = _split_qkv(qkv, B, L, nh)
    s = torch.matmul(q, k.transpose(-1, -2)) * scale + key_bias.float()[:, None, None, :]
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    keep = _attn_keep(B, nh, L, seed, opid, p, qkv.device)
    if keep is not None:
        P = P * keep
    o = torch.matmul(P, v)
    T = B * L
    return o.permute(0, 2, 1, 3).reshape(T, -1).to(qkv.dtype), lse


def attn_bwd(dctx, qkv, ctx, lse, key_bias, B, L, nh, p, seed, opid, scale):
    q, k, v = _split_qkv(qkv, B, L, nh)
    H = qkv.shape[1] // 3
    dh = H // nh
    do = dctx.float().view(B, L, nh, dh).permute(0, 2, 1, 3)
    o = ctx.float().view(B, L, nh, dh).permute(0, 2, 1, 3)
    s = torch.matmul(q, k.transpose(-1, -2)) * scale + key_bias.float()[:, None, None, :]
    P = torch.exp(s - lse[..., None])
    keep = _attn_keep(B, nh, L, seed, opid, p, qkv.device)
    Pd = P * keep if keep is not None else P
    dv = torch.matmul(Pd.transpose(-1, -2), do)
    dP = torch.matmul(do, v.transpose(-1, -2))
    if keep is not None:
        dP = dP * keep
    delta = (do * o).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dq = torch.matmul(dS, k) * scale
    dk = torch.matmul(dS.transpose(-1, -2), q) * scale
    out = torch.stack([dq, dk, dv], 0)  # [3,B,nh,L,dh]
    return out.permute(1, 3, 0, 2, 4).reshape(B * L, 3 * H).to(dctx.dtype)


# --------------------------------------------------------------------------------------- linear
def split_bf16x3(x: Tensor) -> Tuple[Tensor, Tensor]:
    """The two-term bf16 split of ``gemm_f32x3_kernel``: hi = bf16_rne(x), mid = bf16_rne(x − hi) (the subtraction
    is exact in fp32), |x − hi − mid| ≤ 2⁻¹⁶·|x|.  Returned as bf16 tensors."""
    x = x.float()
    hi = x.to(torch.bfloat16)
    mid = (x - hi.float()).to(torch.bfloat16)
    return hi, mid


def matmul_bf16x3(a: Tensor, b_t: Tensor) -> Tensor:
    """a[M, K]·b_t[N, K]ᵀ as the fp32 mode's ``bf16x3`` GEMM computes it: the three leading products of the split
    operands, the two small ones summed first.  Runs in the dtype of ``a`` (fp32; fp64 for the tests' oracle) —
    every bf16·bf16 product is exact in either, so only the summation order over k differs from the kernel."""
    dt = a.dtype if a.dtype == torch.float64 else torch.float32
    ah, am = (t.to(dt) for t in split_bf16x3(a))
    bh, bm = (t.to(dt).t() for t in split_bf16x3(b_t))
    return (am @ bh + ah @ bm) + ah @ bh


def _mm_t(a: Tensor, b_t: Tensor) -> Tensor:
    """a·b_tᵀ in fp32; through the bf16x3 oracle for fp32 tensors while ``ops.f32.MATMUL`` selects that mode."""
    if _f32.MATMUL == "bf16x3" and a.dtype == torch.float32 and b_t.dtype == torch.float32:
        return matmul_bf16x3(a, b_t)
    return a.float() @ b_t.float().t()


def linear_fwd(x, w, b):
    y = _mm_t(x, w)
    if b is not None:
        y = y + b.float()
    return y.to(x.dtype)


def linear_dgrad(dy, w):
    return _mm_t(dy, w.t()).to(dy.dtype)


def linear_dgrad_add(dy, w, resid):
    return (resid.float() + _mm_t(dy, w.t())).to(dy.dtype)


def linear_wgrad(dy, x, g_w, g_b, accumulate: bool):
    _acc(g_w, _mm_t(dy.t(), x.t()), accumulate)
    if g_b is not None:
        _acc(g_b, dy.float().sum(0), accumulate)


# ------------------------------------------------------------------------------------ optimizer
def grad_sq_norm(grad: Tensor) -> Tensor:
    return (grad.float() ** 2).sum()


def adamw_step(master, compute, grad, exp_avg, exp_avg_sq, segments, *, lr, beta1, beta2, eps,
               clip_coef: Optional[Tensor], correct_bias: bool, step: int):
    """HF ``AdamW`` (decay AFTER the update, reference ``init.py:137``) over flat arena segments.

    ``segments``: list of (start, numel, weight_decay).
    """
    g = grad if clip_coef is None else grad * clip_coef
    for start, numel, wd in segments:
        sl = slice(start, start + numel)
        gg = g[sl]
        m = exp_avg[sl]
        v = exp_avg_sq[sl]
        p = master[sl]
        m.mul_(beta1).add_(gg, alpha=1.0 - beta1)
        v.mul_(beta2).addcmul_(gg, gg, value=1.0 - beta2)
        denom = v.sqrt().add_(eps)
        step_size = lr
        if correct_bias:
            step_size = lr * math.sqrt(1.0 - beta2 ** step) / (1.0 - beta1 ** step)
        p.addcdiv_(m, denom, value=-step_size)
        if wd > 0.0:
            p.add_(p, alpha=-lr * wd)
    if compute is not None and compute.data_ptr() != master.data_ptr():
        for start, numel, _ in segments:
            compute[start:start + numel].copy_(master[start:start + numel])


def adamod_step(master, compute, grad, exp_avg, exp_avg_sq, exp_avg_lr, segments, *, lr, beta1, beta2, beta3,
                eps, clip_coef: Optional[Tensor], step: int):
    """AdaMod (reference ``modules/model/trainer/optim.py:76-98``): decay BEFORE the update."""
    g = grad if clip_coef is None else grad * clip_coef
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    base = lr * math.sqrt(bc2) / bc1
    for start, numel, wd in segments:
        sl = slice(start, start + numel)
        gg = g[sl]
        m, v, n, p = exp_avg[sl], exp_avg_sq[sl], exp_avg_lr[sl], master[sl]
        m.mul_(beta1).add_(gg, alpha=1.0 - beta1)
        v.mul_(beta2).addcmul_(gg, gg, value=1.0 - beta2)
        denom = v.sqrt().add_(eps)
        if wd != 0.0:
            p.add_(p, alpha=-wd * lr)
        ss = torch.full_like(denom, base).div_(denom)
        n.mul_(beta3).add_(ss, alpha=1.0 - beta3)
        ss = torch.minimum(ss, n).mul_(m)
        p.add_(-ss)
    if compute is not None and compute.data_ptr() != master.data_ptr():
        for start, numel, _ in segments:
            compute[start:start + numel].copy_(master[start:start + numel])


def lamb_step(master, compute, grad, exp_avg, exp_avg_sq, segments, *, lr, beta1, beta2, eps,
              clip_coef: Optional[Tensor], correct_bias: bool, step: int, adapt: bool = True) -> Tensor:
    """LAMB (You et al. 2020, Algorithm 2) over flat arena segments; one segment = one parameter = one "layer".

        u = (m·bc1) / (sqrt(v·bc2) + eps) + wd·p      eps AFTER the bias correction of v, decay inside u
        r = ‖p‖ / ‖u‖ over the segment (p before the update) if adapt and both norms > 0, else 1
        p = p − (lr·r)·u

    ``segments``: list of (start, numel, weight_decay).  Returns ``[len(segments), 3]`` = (‖p‖, ‖u‖, r) per segment.
    """
    g = grad if clip_coef is None else grad * clip_coef
    bc1 = 1.0 / (1.0 - beta1 ** step) if correct_bias else 1.0
    bc2 = 1.0 / (1.0 - beta2 ** step) if correct_bias else 1.0
    norms = torch.ones(len(segments), 3, dtype=master.dtype, device=master.device)
    lr_t = torch.tensor(lr, dtype=master.dtype, device=master.device)
    for i, (start, numel, wd) in enumerate(segments):
        sl = slice(start, start + numel)
        gg = g[sl]
        m, v, p = exp_avg[sl], exp_avg_sq[sl], master[sl]
        m.mul_(beta1).add_(gg, alpha=1.0 - beta1)
        v.mul_(beta2).addcmul_(gg, gg, value=1.0 - beta2)
        u = (m * bc1).div_((v * bc2).sqrt_().add_(eps))
        if wd != 0.0:
            u.add_(p, alpha=wd)
        W, U = p.square().sum().sqrt(), u.square().sum().sqrt()
        r = W / U if (adapt and bool(W > 0) and bool(U > 0)) else torch.ones_like(W)
        norms[i, 0], norms[i, 1], norms[i, 2] = W, U, r
        p.sub_(u.mul_(lr_t * r))
    if compute is not None and compute.data_ptr() != master.data_ptr():
        for start, numel, _ in segments:
            compute[start:start + numel].copy_(master[start:start + numel])
    return norms


# ------------------------------------------------------------------------------------ inference decode
def qa_decode(start, end, cls, start_reg, end_reg, lo, hi, max_answer_len: int) -> Tensor:
    """Joint valid-span decode, the definition ``csrc/kernels/decode.hip`` implements bit for bit.

    Per row: window ``lo' = clamp(lo, 0, L)``, ``hi' = clamp(hi, 0, L)``; candidates ``lo' <= s <= e < hi'`` with
    ``e - s < max_answer_len``; ``key = fl32(start[s] + end[e])``; the largest key wins, then the smallest ``s``,
    then the smallest ``e``; ``score = fl32(key - fl32(start[0] + end[0]))``; no candidate → ``s = e = -1``,
    ``score = -inf``; ``label`` = first argmax of ``cls``.  Returns fp32 ``[B, 6]`` = (score, s, e, start_reg,
    end_reg, label).  Ties are resolved by the smallest flat index among the maxima, never by ``argmax``, whose
    choice among equal values differs between devices.
    """
    W = int(max_answer_len)
    if W < 1:
        raise ValueError(f"max_answer_len must be >= 1, got {max_answer_len}")
    start, end, cls = start.float(), end.float(), cls.float()
    B, L = start.shape
    dev = start.device
    lo = lo.to(dev).long().clamp(0, L).view(B, 1, 1)
    hi = hi.to(dev).long().clamp(0, L).view(B, 1, 1)
    s = torch.arange(L, device=dev).view(1, L, 1)
    e = torch.arange(L, device=dev).view(1, 1, L)
    valid = ((s >= lo) & (e < hi) & (e >= s) & (e - s < W)).view(B, L * L)
    key = (start.unsqueeze(2) + end.unsqueeze(1)).view(B, L * L)
    best = torch.where(valid, key, key.new_full((), float("-inf"))).amax(1)
    flat = torch.arange(L * L, device=dev).expand(B, L * L)
    first = torch.where(valid & (key == best.unsqueeze(1)), flat, flat.new_full((), L * L)).amin(1)
    found = first < L * L
    s_id = torch.where(found, first // L, first.new_full((), -1))
    e_id = torch.where(found, first % L, first.new_full((), -1))
    score = torch.where(found, best - (start[:, 0] + end[:, 0]), best.new_full((), float("-inf")))
    NL = cls.shape[1]
    c = torch.arange(NL, device=dev).expand(B, NL)
    label = torch.where(cls == cls.amax(1, keepdim=True), c, c.new_full((), NL)).amin(1)
    return torch.stack([score, s_id.float(), e_id.float(), start_reg.float().reshape(-1), end_reg.float().reshape(-1),
                        label.float()], 1)
