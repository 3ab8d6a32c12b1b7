"""The bindings' operand contract: a malformed call raises on the host, names the op and the operand, and launches
nothing.

Every test makes one valid call on the smallest operands the op launches at (so a later raise is due to the probe
alone), then replaces exactly one operand per probe and expects ``RuntimeError`` "<op>: <operand> ...".  At the end
every tensor the op writes — and every probe tensor — must still hold its bits.

Probes are wrong only in ways that keep a MISSED check in bounds: more elements than expected, a wider dtype of the
same shape, or a column slice of a wider buffer.  Checks whose only violation is an undersized or off-device operand
have no GPU probe.
"""
import itertools

import pytest
import torch

from ml_recipe_distributed_pytorch_amd import _native

pytestmark = pytest.mark.gpu

T, H, V, P, NTYPES = 8, 128, 16, 8, 2   # 2 sequences x 4 tokens
EPI_BIAS = 1


def _bits(t):
    return t.contiguous().view(-1).view(torch.uint8).clone()


def _check(op, fn, args, written, probes):
    """``args``: the valid call's operands by name, in call order.  ``written``: names of the tensors the op writes.
    ``probes``: (argument name, operand name in the message, replacement)."""
    fn(*args.values())                       # the baseline is accepted
    torch.cuda.synchronize()
    kept = [(args[n], _bits(args[n])) for n in written] + [(bad, _bits(bad)) for _, _, bad in probes]
    for key, name, bad in probes:
        call = dict(args)
        assert key in call
        call[key] = bad
        with pytest.raises(RuntimeError, match=rf"{op}: {name} "):
            fn(*call.values())
    torch.cuda.synchronize()
    for t, before in kept:
        assert torch.equal(_bits(t), before)


def _wide(t):
    """A non-contiguous tensor of t's shape and dtype: the left columns of a buffer twice as wide."""
    return torch.zeros(t.shape[0], 2 * t.shape[1], dtype=t.dtype, device=t.device)[:, :t.shape[1]]


def _f32(dev, *shape):
    return torch.randn(*shape, device=dev)


# ------------------------------------------------------------------------------------------------ embedding
def _embed_args(cuda, k, dt):
    f32 = dt == torch.float32
    fwd = k.f32_embed_fwd if f32 else k.embed_fwd
    ids = torch.arange(T, device=cuda) % V
    pids = torch.arange(T, device=cuda) % 4
    tids = torch.arange(T, device=cuda) % NTYPES
    ww, wp, wt = (_f32(cuda, n, H).to(dt) for n in (V, P, NTYPES))
    gamma, beta = _f32(cuda, H), _f32(cuda, H)
    fargs = dict(ids=ids, pids=pids, tids=tids, ww=ww, wp=wp, wt=wt, gamma=gamma, beta=beta, eps=1e-12, p=0.0, seed=1, opid=1)
    _, mean, rstd = fwd(*fargs.values())
    bargs = dict(dy=_f32(cuda, T, H).to(dt), ids=ids, pids=pids, tids=tids, ww=ww, wp=wp, wt=wt, gamma=gamma, mean=mean,
                 rstd=rstd, p=0.0, seed=1, opid=1, g_word=torch.zeros(V, H, device=cuda),
                 g_pos=torch.zeros(P, H, device=cuda), g_type=torch.zeros(NTYPES, H, device=cuda),
                 g_gamma=torch.zeros(H, device=cuda), g_beta=torch.zeros(H, device=cuda), accumulate=False, pad_word=0,
                 pad_pos=-1)
    return fargs, bargs


@pytest.mark.parametrize("op", ["embed_bwd", "f32_embed_bwd"])
def test_embedding_backward(cuda, op):
    k = _native.kernels()
    dt = torch.float32 if op.startswith("f32") else torch.bfloat16
    _, a = _embed_args(cuda, k, dt)
    _check(op, getattr(k, op), a, ("g_word", "g_pos", "g_type", "g_gamma", "g_beta"), [
        ("mean", "mean", torch.zeros(T + 1, device=cuda)),
        ("gamma", "gamma", torch.ones(2 * H, device=cuda)),
        ("g_beta", "g_beta", torch.zeros(2 * H, device=cuda)),
        ("pids", "pos_ids", torch.zeros(T + 1, dtype=torch.int64, device=cuda)),
        ("dy", "dy", _wide(a["dy"])),
        ("wp", "w_pos", torch.zeros(P, 2 * H, dtype=dt, device=cuda)),
    ])


def test_embedding_forward_fp32(cuda):
    k = _native.kernels()
    a, _ = _embed_args(cuda, k, torch.float32)
    _check("f32_embed_fwd", k.f32_embed_fwd, a, (), [("beta", "beta", torch.zeros(2 * H, device=cuda))])


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln_args(cuda, k, dt):
    f32 = dt == torch.float32
    a, resid = _f32(cuda, T, H).to(dt), _f32(cuda, T, H).to(dt)
    gamma, beta = _f32(cuda, H), _f32(cuda, H)
    fargs = dict(a=a, resid=resid, gamma=gamma, beta=beta, eps=1e-12, p=0.0, seed=1, opid=1)
    y, z, mean, rstd = (k.f32_ln_fwd if f32 else k.ln_fwd)(*fargs.values())[:4]
    bargs = dict(dy=_f32(cuda, T, H).to(dt), dy2=None, z=y, gamma=gamma, mean=mean, rstd=rstd, p=0.0, seed=1, opid=1,
                 g_gamma=torch.zeros(H, device=cuda), g_beta=torch.zeros(H, device=cuda),
                 g_bias=torch.zeros(H, device=cuda), accumulate=False)
    if not f32:
        bargs.update(q8=None, phase=0, write_da=True)
    bargs["beta"] = beta          # z is the forward output y
    return fargs, bargs


@pytest.mark.parametrize("op", ["ln_bwd", "f32_ln_bwd"])
def test_layernorm_backward(cuda, op):
    k = _native.kernels()
    dt = torch.float32 if op.startswith("f32") else torch.bfloat16
    _, a = _ln_args(cuda, k, dt)
    _check(op, getattr(k, op), a, ("g_gamma", "g_beta", "g_bias"), [
        ("g_gamma", "g_gamma", torch.zeros(2 * H, device=cuda)),
        ("g_bias", "g_bias", torch.zeros(H, dtype=torch.float64, device=cuda)),
        ("rstd", "rstd", torch.ones(T + 1, device=cuda)),
        ("beta", "beta", torch.zeros(2 * H, device=cuda)),
        ("z", "z", _wide(a["z"])),
    ])


def test_layernorm_forward_fp32(cuda):
    k = _native.kernels()
    a, _ = _ln_args(cuda, k, torch.float32)
    _check("f32_ln_fwd", k.f32_ln_fwd, a, (), [("beta", "beta", torch.zeros(2 * H, device=cuda))])


# ------------------------------------------------------------------------------------------- GELU and bias
@pytest.mark.parametrize("op", ["gelu_bwd", "f32_gelu_bwd"])
def test_gelu_backward(cuda, op):
    k = _native.kernels()
    dt = torch.float32 if op.startswith("f32") else torch.bfloat16
    a = dict(dout=_f32(cuda, T, H).to(dt), pre=_f32(cuda, T, H).to(dt), g_bias=torch.zeros(H, device=cuda),
             accumulate=False)
    _check(op, getattr(k, op), a, ("g_bias",), [
        ("g_bias", "g_bias", torch.zeros(2 * H, device=cuda)),
        ("g_bias", "g_bias", torch.zeros(H, dtype=torch.float64, device=cuda)),
    ])


# ------------------------------------------------------------------------------------------------ span head
def test_span_backward(cuda):
    k = _native.kernels()
    a = dict(seq=_f32(cuda, T, H).bfloat16(), w=_f32(cuda, 2, H), grad_logits=_f32(cuda, T, 2),
             dw=torch.zeros(2, H, device=cuda), accumulate=False)
    _check("span_bwd", k.span_bwd, a, ("dw",), [
        ("dw", "dw", torch.zeros(4, H, device=cuda)),
        ("grad_logits", "grad_logits", torch.zeros(T + 1, 2, device=cuda)),
    ])


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("op", ["attn_bwd", "f32_attn_bwd"])
def test_attention_backward(cuda, op):
    k = _native.kernels()
    f32 = op.startswith("f32")
    dt = torch.float32 if f32 else torch.bfloat16
    B, L, nh = 1, 1, 1                      # the smallest length of tests/test_attention_oracle_gpu.py
    qkv, kb = _f32(cuda, B * L, 3 * nh * 64).to(dt), torch.zeros(B, L, device=cuda)
    dctx = _f32(cuda, B * L, nh * 64).to(dt)
    if f32:
        ctx, lse = k.f32_attn_fwd(qkv, kb, B, L, nh, 0.0, 1, 1, 0.125)
        a = dict(dctx=dctx, qkv=qkv, ctx=ctx, lse=lse, key_bias=kb, B=B, L=L, nh=nh, p=0.0, seed=1, opid=1, scale=0.125)
    else:
        ctx, lse, bits = k.attn_fwd(qkv, kb, B, L, nh, 0.0, 1, 1, 0.125)
        a = dict(dctx=dctx, qkv=qkv, ctx=ctx, lse=lse, key_bias=kb, mbits=bits, B=B, L=L, nh=nh, p=0.0, scale=0.125,
                 deterministic=True)
    probes = [("lse", "lse", torch.zeros(B, nh, L + 1, device=cuda))]
    if not f32:
        probes.append(("dctx", "dctx", dctx.float()))
    _check(op, getattr(k, op), a, (), probes)


# ---------------------------------------------------------------------------------------------------- GEMMs
def _smallest(query):
    """The smallest (by volume) shape of 64 .. 512 per dimension for which the op's own query answers yes."""
    dims = (64, 128, 256, 512)
    for s in sorted(itertools.product(dims, repeat=3), key=lambda s: (s[0] * s[1] * s[2], s)):
        if query(*s):
            return s
    raise AssertionError("no supported shape")


def test_gemm_nt(cuda):
    k = _native.kernels()
    M, N, K = _smallest(k.gemm_nt_supported)
    a = dict(A=_f32(cuda, M, K).bfloat16(), B=_f32(cuda, N, K).bfloat16(), epi=EPI_BIAS, bias=_f32(cuda, N), pre=None,
             resid=None, part=None, out=torch.zeros(M, N, dtype=torch.bfloat16, device=cuda))
    _check("gemm_nt", k.gemm_nt, a, ("out",), [
        ("bias", "bias", torch.zeros(N + 128, device=cuda)),
        ("out", "out", torch.zeros(M + 128, N, dtype=torch.bfloat16, device=cuda)),
    ])


def test_gemm_tn(cuda):
    k = _native.kernels()
    Tn, N, K = _smallest(k.gemm_tn_splits)
    a = dict(dy=_f32(cuda, Tn, N).bfloat16(), x=_f32(cuda, Tn, K).bfloat16(), out=torch.zeros(N, K, device=cuda),
             accumulate=False, splits=0, bias_out=torch.zeros(N, device=cuda))
    _check("gemm_tn", k.gemm_tn, a, ("out", "bias_out"), [
        ("out", "out", torch.zeros(N + 128, K, device=cuda)),
        ("bias_out", "bias_out", torch.zeros(N + 128, device=cuda)),
    ])


def test_gemm_tn8(cuda):
    k = _native.kernels()
    Tn, N, K = _smallest(k.gemm_tn8_splits)
    one = torch.ones(1, device=cuda)
    a = dict(dy8=torch.ones(Tn, N, device=cuda).to(torch.float8_e5m2), x8=torch.ones(Tn, K, device=cuda).to(torch.float8_e4m3fn),
             sa=one, sb=one, out=torch.zeros(N, K, device=cuda), accumulate=False)
    _check("gemm_tn8", k.gemm_tn8, a, ("out",), [("out", "out", torch.zeros(N + 128, K, device=cuda))])


def test_gemm_fp8(cuda):
    k = _native.kernels()
    M, N, K = _smallest(k.gemm_fp8_supported)
    one = torch.ones(1, device=cuda)
    a = dict(A8=torch.ones(M, K, device=cuda).to(torch.float8_e4m3fn), B8=torch.ones(N, K, device=cuda).to(torch.float8_e4m3fn),
             epi=EPI_BIAS, bias=_f32(cuda, N), sa=one, sb=one)
    _check("gemm_fp8", k.gemm_fp8, a, (), [("bias", "bias", torch.zeros(N + 128, device=cuda))])


def test_gemm_f32(cuda):
    k = _native.kernels()
    M = N = K = 64
    a = dict(A=_f32(cuda, M, K), B=_f32(cuda, N, K), C=torch.zeros(M, N, device=cuda), M=M, N=N, K=K, sa=[K, 1, 0, 0],
             sb=[K, 1, 0, 0], sc=[N, 0, 0], batch=1, nb_in=1, alpha=1.0, bias=_f32(cuda, N))
    _check("gemm_f32", k.gemm_f32, a, ("C",), [("bias", "bias", torch.zeros(N + 64, device=cuda))])


# ------------------------------------------------------------------------------------------------ optimizer
def test_adamw(cuda):
    k = _native.kernels()
    n = 64
    a = dict(master=_f32(cuda, n), compute=torch.zeros(n, dtype=torch.bfloat16, device=cuda), grad=_f32(cuda, n),
             exp_avg=torch.zeros(n, device=cuda), exp_avg_sq=torch.zeros(n, device=cuda),
             chunks=torch.tensor([[0, n]], dtype=torch.int64, device=cuda), lr=[1e-3], wd=[0.0], beta1=0.9, beta2=0.999,
             eps=1e-8, step_mult=1.0, clip_coef=None)
    _check("adamw", k.adamw, a, ("master", "compute", "exp_avg", "exp_avg_sq"),
           [("exp_avg", "exp_avg", torch.zeros(n + 4, device=cuda))])


# ------------------------------------------------------------------------------------------------- QA heads
def test_qa_heads_backward(cuda):
    k = _native.kernels()
    B, L, NL = 2, 4, 5
    shapes = [(H, H), (H,), (NL, H), (NL,), (1, H), (1,), (1, H), (1,), (2, H), (2,)]
    w = [_f32(cuda, *s) * 0.05 for s in shapes]
    seq = _f32(cuda, B * L, H).bfloat16()
    _, pooled, _, reg = k.qa_heads_fwd(seq, L, w, 0.0, 1, 1)
    grads = [torch.zeros_like(t) for t in w]
    a = dict(seq=seq, L=L, dlog=_f32(cuda, B * L, 2), dheads=_f32(cuda, B, 16), gscale=None, pooled=pooled, reg=reg, w=w,
             grads=grads, accumulate=False, p=0.0, seed=1, opid=1)
    fn = k.qa_heads_bwd
    fn(*a.values())
    torch.cuda.synchronize()
    before = [_bits(t) for t in grads]
    bad = torch.zeros(B + 1, H, device=cuda)
    with pytest.raises(RuntimeError, match=r"qa_heads_bwd: pooled "):
        fn(*{**a, "pooled": bad}.values())
    wrong = list(grads)
    wrong[1] = torch.zeros(2 * H, device=cuda)
    with pytest.raises(RuntimeError, match=r"qa_heads_bwd: g_bp "):
        fn(*{**a, "grads": wrong}.values())
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(t), b) for t, b in zip(grads, before))
    assert not bad.any() and not wrong[1].any()
