"""HIP kernel numerics vs the fp32 PyTorch reference of the same op (ops/reference.py).

Inputs are bf16 (what the kernels consume); the oracle runs the same math in fp32 on the CPU on
those exact bf16 values, including the identical dropout masks (shared counter hash)."""
import math

import pytest
import torch

from ml_recipe_distributed_pytorch_amd import _native
from ml_recipe_distributed_pytorch_amd.ops import reference as ref

pytestmark = pytest.mark.gpu


def _close(a, b, atol, rtol, what):
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol).sum().item()
    assert bad == 0, f"{what}: {bad} / {a.numel()} outside tol, max err {err.max().item():.3e}"


def _bf(x):
    return x.to(torch.bfloat16)


@pytest.mark.parametrize("H", [128, 768, 1024])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_ln_fwd_bwd(cuda, H, p):
    k = _native.kernels()
    torch.manual_seed(0)
    T = 1000
    a, r = _bf(torch.randn(T, H)), _bf(torch.randn(T, H))
    gamma, beta = torch.randn(H) * 0.5 + 1, torch.randn(H) * 0.1
    y, z, m, rs = k.ln_fwd(a.to(cuda), r.to(cuda), gamma.to(cuda), beta.to(cuda), 1e-12, p, 1234, 7)
    yr, zr, mr, rr = ref.ln_fwd(a, r, gamma, beta, 1e-12, p, 1234, 7)
    _close(z, zr, 1e-2, 1e-2, "z")
    _close(y, yr, 3e-2, 2e-2, "y")
    _close(m, mr, 1e-3, 1e-3, "mean")
    _close(rs, rr, 1e-3, 2e-3, "rstd")
    dy, dy2 = _bf(torch.randn(T, H)), _bf(torch.randn(T, H))
    for acc in (False, True):
        gg = [torch.randn(H).to(cuda) for _ in range(3)]
        ggr = [g.cpu().clone() for g in gg]
        dz, da = k.ln_bwd(dy.to(cuda), dy2.to(cuda), z, gamma.to(cuda), m, rs, p, 1234, 7, gg[0], gg[1], gg[2], acc)
        dzr, dar = ref.ln_bwd(dy, dy2, z.cpu(), gamma, m.cpu(), rs.cpu(), p, 1234, 7, ggr[0], ggr[1], ggr[2], acc)
        _close(dz, dzr, 3e-2, 2e-2, "dz")
        _close(da, dar, 3e-2, 2e-2, "da")
        for i, n in enumerate(["dgamma", "dbeta", "dbias"]):
            _close(gg[i], ggr[i], 5e-2, 1e-3, n)


@pytest.mark.parametrize("H,T", [(768, 1000), (768, 24576), (1024, 1000)])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_ln_bwd_from_y(cuda, H, T, p):
    """Memory-efficient LayerNorm: the forward with store_z=False writes no z and the backward recomputes
    x̂ = (y − β)/γ from the output (beta=).  Against the CPU form of the same recompute (ref.ln_bwd(beta=)) and
    against the exact-input fp32 oracle (x̂ from z) at the bf16-gradient tolerance; y / mean / rstd are
    bitwise those of the z-storing forward.  A γ = 0 column gets x̂ = 0 (its x̂ is not recoverable from y), so its
    own dz and γ gradient are excluded from the exact-input comparison — the documented limit of this form."""
    k = _native.kernels()
    torch.manual_seed(1)
    a, r = _bf(torch.randn(T, H)), _bf(torch.randn(T, H))
    # γ in [0.5, 1.5) (x̂'s error from y's bf16 rounding grows as |β/γ| + |x̂| over 2⁹), plus one γ = 0 column
    gamma, beta = torch.rand(H) + 0.5, torch.randn(H) * 0.1
    gamma[5] = 0.0
    y, z, m, rs = k.ln_fwd(a.to(cuda), r.to(cuda), gamma.to(cuda), beta.to(cuda), 1e-12, p, 99, 4)
    y2, z2, m2, rs2 = k.ln_fwd(a.to(cuda), r.to(cuda), gamma.to(cuda), beta.to(cuda), 1e-12, p, 99, 4, store_z=False)
    assert z2.numel() == 0
    assert torch.equal(y, y2) and torch.equal(m, m2) and torch.equal(rs, rs2)
    dy, dy2 = _bf(torch.randn(T, H)), _bf(torch.randn(T, H))
    gg = [torch.zeros(H, device=cuda) for _ in range(3)]
    ggy = [torch.zeros(H) for _ in range(3)]
    ggz = [torch.zeros(H) for _ in range(3)]
    dz, da = k.ln_bwd(dy.to(cuda), dy2.to(cuda), y2, gamma.to(cuda), m2, rs2, p, 99, 4, gg[0], gg[1], gg[2], False,
                      beta=beta.to(cuda))
    dzy, day = ref.ln_bwd(dy, dy2, y2.cpu(), gamma, m2.cpu(), rs2.cpu(), p, 99, 4, ggy[0], ggy[1], ggy[2], False,
                          beta=beta)
    dzz, daz = ref.ln_bwd(dy, dy2, z.cpu(), gamma, m.cpu(), rs.cpu(), p, 99, 4, ggz[0], ggz[1], ggz[2], False)
    _close(dz, dzy, 3e-2, 2e-2, "dz vs the same recompute")
    _close(da, day, 3e-2, 2e-2, "da vs the same recompute")
    # a γ = 0 column's x̂ cannot be recovered from y: its own dz (through x̂·mean(g·γ·x̂)) and γ gradient differ
    # from the exact-input form by construction; every other column must agree
    keep = torch.arange(H) != 5
    _close(dz[:, keep.to(cuda)], dzz[:, keep], 5e-2, 3e-2, "dz vs the exact-input oracle")
    for i, n in enumerate(["dgamma", "dbeta", "dbias"]):
        _close(gg[i], ggy[i], 5e-2 * (T / 1000) ** 0.5, 1e-3, n)
    # Σ_t g·x̂ over T rows: y's bf16 rounding in x̂ is a random walk of ~2⁻⁹ per row (0.3-0.6 % of dγ at T = 24576)
    _close(gg[0][keep.to(cuda)], ggz[0][keep], 0.5 * (T / 1000) ** 0.5, 1e-2, "dgamma vs the exact-input oracle")
    _close(gg[1], ggz[1], 5e-2 * (T / 1000) ** 0.5, 1e-3, "dbeta vs the exact-input oracle")


@pytest.mark.parametrize("T", [1000, 24576])
def test_ln_bwd_from_y_guarded_range(cuda, T):
    """The from-y backward across pretrained-like LayerNorm weights: γ log-uniform over [1e-3, 2], β ~ N(0, 0.5).
    The model's guard (BertForQuestionAnswering.refresh_ln_modes) admits a LayerNorm for the from-y backward only
    if EVERY column has γ != 0 and |β| <= LN_FROM_Y_MAX_RATIO·|γ|; with these weights it must reject (the model
    then stores z: exact).  Within the admitted region — β clipped to ±8|γ|, every γ magnitude of the range —
    the from-y gradients must match the exact-input oracle to the rounding model of x̂ = (y − β)/γ: y is bf16,
    so |δx̂| <= (|x̂| + |β/γ|)·2⁻⁸ per element, and dγ = Σ_t g·x̂ collects it as a random walk over T rows."""
    from ml_recipe_distributed_pytorch_amd.models.bert import BertForQuestionAnswering
    ratio = BertForQuestionAnswering.LN_FROM_Y_MAX_RATIO
    k = _native.kernels()
    torch.manual_seed(11)
    H = 768
    a, r = _bf(torch.randn(T, H)), _bf(torch.randn(T, H))
    gamma = torch.exp(torch.empty(H).uniform_(math.log(1e-3), math.log(2.0)))
    beta = torch.randn(H) * 0.5
    admitted = beta.abs() <= ratio * gamma
    assert not bool(admitted.all()), "the guard must reject this LayerNorm (it then keeps z)"
    beta = torch.where(admitted, beta, ratio * gamma * torch.sign(beta))   # the worst admitted weights
    y, z, m, rs = k.ln_fwd(a.to(cuda), r.to(cuda), gamma.to(cuda), beta.to(cuda), 1e-12, 0.0, 99, 4)
    y2, _, m2, rs2 = k.ln_fwd(a.to(cuda), r.to(cuda), gamma.to(cuda), beta.to(cuda), 1e-12, 0.0, 99, 4, store_z=False)
    dy, dy2 = _bf(torch.randn(T, H)), _bf(torch.randn(T, H))
    gg = [torch.zeros(H, device=cuda) for _ in range(3)]
    ggz = [torch.zeros(H) for _ in range(3)]
    dz, _ = k.ln_bwd(dy.to(cuda), dy2.to(cuda), y2, gamma.to(cuda), m2, rs2, 0.0, 99, 4, gg[0], gg[1], gg[2], False,
                     beta=beta.to(cuda))
    dzz, _ = ref.ln_bwd(dy, dy2, z.cpu(), gamma, m.cpu(), rs.cpu(), 0.0, 99, 4, ggz[0], ggz[1], ggz[2], False)
    _close(dz, dzz, 5e-2, 3e-2, "dz vs the exact-input oracle")
    _close(gg[1], ggz[1], 5e-2 * (T / 1000) ** 0.5, 1e-3, "dbeta vs the exact-input oracle")
    # per-column dγ bound: 4σ of the random walk Σ_t g_t·δx̂_t with |δx̂_t| <= (|x̂_t| + |β/γ|)·2⁻⁸
    xh = (z.cpu().float() - m.cpu().float()[:, None]) * rs.cpu().float()[:, None]
    g = (dy.float() + dy2.float())
    bound = 4.0 * 2.0 ** -8 * torch.sqrt(((g * (xh.abs() + (beta / gamma).abs()[None, :])) ** 2).sum(0)) + 1e-2
    err = (gg[0].cpu() - ggz[0]).abs()
    assert bool((err <= bound).all()), f"dgamma: {int((err > bound).sum())} columns beyond the rounding bound"


@pytest.mark.parametrize("H,ntypes", [(768, 2), (128, 1)])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("layout", ["flat", "seq", "seq_randpos"])
def test_embedding(cuda, H, ntypes, p, layout):
    """embed fwd/bwd vs the fp32 oracle.  ``seq`` passes L so the backward walks positions across the
    batch (register-summed position grads); ``seq_randpos`` gives every token a random position id so
    the per-pid flush path is exercised; ``flat`` = unknown layout (seq_len 0)."""
    k = _native.kernels()
    torch.manual_seed(1)
    V, P, B, L = 1000, 64, 4, 50
    T = B * L
    ww, wp, wt = _bf(torch.randn(V, H) * 0.05), _bf(torch.randn(P, H) * 0.05), _bf(torch.randn(ntypes, H) * 0.05)
    gamma, beta = torch.randn(H) * 0.3 + 1, torch.randn(H) * 0.1
    ids = torch.randint(0, V, (T,))
    ids[::7] = 0
    pids = torch.randint(0, P, (T,)) if layout == "seq_randpos" else torch.arange(L).repeat(B)
    tids = torch.randint(0, ntypes, (T,))
    dev = lambda t: t.to(cuda)  # noqa: E731
    y, m, rs = k.embed_fwd(dev(ids), dev(pids), dev(tids), dev(ww), dev(wp), dev(wt), dev(gamma), dev(beta), 1e-12, p, 99, 0)
    yr, mr, rr = ref.embed_fwd(ids, pids, tids, ww, wp, wt, gamma, beta, 1e-12, p, 99, 0, torch.float32)
    _close(y, yr, 3e-2, 2e-2, "y")
    _close(m, mr, 1e-4, 1e-3, "mean")
    dy = _bf(torch.randn(T, H))
    gw, gp, gt = torch.zeros(V, H), torch.zeros(P, H), torch.zeros(ntypes, H)
    gg, gb = torch.zeros(H), torch.zeros(H)
    out = [dev(t) for t in (gw, gp, gt, gg, gb)]
    k.embed_bwd(dev(dy), dev(ids), dev(pids), dev(tids), dev(ww), dev(wp), dev(wt), dev(gamma), m, rs, p, 99, 0, *out,
                False, 0, -1, 0 if layout == "flat" else L)
    ref.embed_bwd(dy, ids, pids, tids, ww, wp, wt, gamma, m.cpu(), rs.cpu(), p, 99, 0, gw, gp, gt, gg, gb, False, 0, -1)
    for a, b, n in zip(out, (gw, gp, gt, gg, gb), ["word", "pos", "type", "gamma", "beta"]):
        _close(a, b, 5e-2, 2e-2, n)
    assert out[0][0].abs().max().item() == 0.0, "padding row must get no gradient"


@pytest.mark.parametrize("V,T", [(200, 1000), (30522, 98304 + 17), (30522, 1), (70000, 5000), (1000, 4096)])
def test_sort_ids_is_a_stable_sort(cuda, V, T):
    """The embedding backward's own LSD radix sort (sort.hip sort_*_kernel, 1 / 2 / 3 passes of 8 bits) equals a
    stable sort: ids ascending, rows of one id in token order — and the same permutation every run."""
    k = _native.kernels()
    g = torch.Generator().manual_seed(V + T)
    ids = torch.randint(0, V, (T,), generator=g)
    if T > 100:
        ids[torch.randperm(T, generator=g)[: T // 10]] = V // 2    # one long run
    skeys, srows = k.sort_ids(ids.to(cuda), V)
    want_k, want_r = torch.sort(ids, stable=True)
    assert torch.equal(skeys.cpu().long(), want_k)
    assert torch.equal(srows.cpu().long(), want_r)
    k2, r2 = k.sort_ids(ids.to(cuda), V)
    assert torch.equal(k2, skeys) and torch.equal(r2, srows)


@pytest.mark.parametrize("accumulate", [False, True])
def test_embedding_bwd_sorted_runs(cuda, accumulate):
    """The id-sorted word-gradient pass: runs of one id that stay inside a 16-row chunk, end exactly on a chunk
    boundary, or cross many chunks (id 5: 100 rows -> start piece, middle pieces, end piece), the padding id
    (no gradient) and single rows, in both the fresh and the accumulating mode, vs the fp32 oracle."""
    k = _native.kernels()
    torch.manual_seed(4)
    V, P, B, L, H = 300, 64, 8, 64, 768
    T = B * L
    ww, wp, wt = _bf(torch.randn(V, H) * 0.05), _bf(torch.randn(P, H) * 0.05), _bf(torch.randn(2, H) * 0.05)
    gamma = torch.randn(H) * 0.3 + 1
    ids = torch.randint(8, V, (T,))
    perm = torch.randperm(T)
    ids[perm[:100]] = 5      # a long run
    ids[perm[100:116]] = 7   # exactly one chunk's worth
    ids[perm[116:156]] = 0   # padding
    ids[perm[156:173]] = 3   # 17 rows
    pids = torch.arange(L).repeat(B)
    tids = torch.randint(0, 2, (T,))
    dev = lambda t: t.to(cuda)  # noqa: E731
    _, m, rs = k.embed_fwd(dev(ids), dev(pids), dev(tids), dev(ww), dev(wp), dev(wt), dev(gamma), dev(torch.zeros(H)),
                           1e-12, 0.1, 7, 0)
    dy = _bf(torch.randn(T, H))
    init = [torch.randn(V, H) if accumulate else torch.zeros(V, H), torch.randn(P, H) if accumulate else torch.zeros(P, H),
            torch.zeros(2, H), torch.zeros(H), torch.zeros(H)]
    out = [dev(t.clone()) for t in init]
    refs = [t.clone() for t in init]
    k.embed_bwd(dev(dy), dev(ids), dev(pids), dev(tids), dev(ww), dev(wp), dev(wt), dev(gamma), m, rs, 0.1, 7, 0, *out,
                accumulate, 0, -1, L)
    ref.embed_bwd(dy, ids, pids, tids, ww, wp, wt, gamma, m.cpu(), rs.cpu(), 0.1, 7, 0, *refs, accumulate, 0, -1)
    for a, b, n in zip(out, refs, ["word", "pos", "type", "gamma", "beta"]):
        _close(a, b, 5e-2, 2e-2, n)
    assert torch.equal(out[0][0].cpu(), init[0][0]), "padding row must get no gradient"
    # rows of ids that never occur keep their initial value exactly
    absent = torch.ones(V, dtype=torch.bool)
    absent[ids.unique()] = False
    assert torch.equal(out[0][absent.to(cuda)].cpu(), init[0][absent])


def test_gelu_and_bias_grad(cuda):
    k = _native.kernels()
    torch.manual_seed(2)
    T, N = 300, 3072
    pre = _bf(torch.randn(T, N) * 2)
    out = k.gelu_fwd(pre.to(cuda))
    _close(out, ref.gelu_fwd(pre.float()), 2e-2, 1e-2, "gelu")
    dout = _bf(torch.randn(T, N))
    gb = torch.randn(N)
    gbd = gb.to(cuda)
    d = k.gelu_bwd(dout.to(cuda), pre.to(cuda), gbd, True)
    dr = ref.gelu_bwd(dout, pre, gb, True)
    _close(d, dr, 2e-2, 2e-2, "dgelu")
    _close(gbd, gb, 5e-2, 1e-3, "gelu bias grad")
    g2 = torch.zeros(N, device=cuda)
    k.bias_grad(d, g2, False)
    _close(g2, d.float().sum(0), 1e-2, 1e-4, "bias_grad")


def _attn_case(cuda, B, L, nh, p, masked, ramp=0.0, amp=1.0, ctx_tol=2e-2, left_pad=0, det=False, bwd_atol=3e-2):
    k = _native.kernels()
    torch.manual_seed(3)
    H = nh * 64
    qkv = _bf(torch.randn(B * L, 3 * H) * amp)
    kb = ramp * torch.arange(L, dtype=torch.float32).expand(B, L).clone()
    if masked:
        for b in range(B):
            kb[b, L - 1 - 7 * b:] = -10000.0
    if left_pad:
        kb[:, :left_pad] = -10000.0
    scale = 1.0 / 8.0
    ctx, lse, bits = k.attn_fwd(qkv.to(cuda), kb.to(cuda), B, L, nh, p, 555, 3, scale)
    ctxr, lser = ref.attn_fwd(qkv, kb, B, L, nh, p, 555, 3, scale)
    _close(lse, lser, 1e-2, 1e-3, "lse")
    _close(ctx, ctxr, ctx_tol, 2e-2, "ctx")
    dctx = _bf(torch.randn(B * L, H))
    dq = k.attn_bwd(dctx.to(cuda), qkv.to(cuda), ctx, lse, kb.to(cuda), bits, B, L, nh, p, scale, det)
    dqr = ref.attn_bwd(dctx, qkv, ctx.cpu(), lse.cpu(), kb, B, L, nh, p, 555, 3, scale)
    _close(dq, dqr, bwd_atol, 3e-2, "dqkv")


@pytest.mark.parametrize("L", [384, 512, 256, 128, 100, 24, 7])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention(cuda, L, p):
    """Ring forward + the two-kernel backward (ring dQ + register dK/dV) against the fp32 oracle."""
    _attn_case(cuda, 2, L, 2, p, masked=True, det=True)


def test_attention_bwd_deterministic_mode_repeatable(cuda):
    """The backward (no atomics) is bitwise repeatable."""
    k = _native.kernels()
    torch.manual_seed(5)
    B, L, nh = 4, 384, 12
    H = nh * 64
    qkv = _bf(torch.randn(B * L, 3 * H)).to(cuda)
    kb = torch.zeros(B, L, device=cuda)
    kb[1, 300:] = -10000.0
    ctx, lse, bits = k.attn_fwd(qkv, kb, B, L, nh, 0.1, 7, 1, 0.125)
    dctx = _bf(torch.randn(B * L, H)).to(cuda)
    d0 = k.attn_bwd(dctx, qkv, ctx, lse, kb, bits, B, L, nh, 0.1, 0.125, True)
    for det in (True, False, True):
        assert torch.equal(k.attn_bwd(dctx, qkv, ctx, lse, kb, bits, B, L, nh, 0.1, 0.125, det), d0)


def test_attention_bert_base_shape(cuda):
    _attn_case(cuda, 2, 384, 12, 0.1, masked=False)


@pytest.mark.parametrize("ramp", [0.05, 0.3, -0.05])
def test_attention_growing_row_max(cuda, ramp):
    """Row maxima that keep growing across key tiles (a key-bias ramp: +2.3 / +14 log2 units per tile, or
    falling).  The ring forward keeps m at the first tile's max, so P grows to 2^25 (ramp 0.05) or 2^150
    (ramp 0.3: l overflows 2^64 → the workgroup's in-kernel slow path); both against the fp32 reference,
    forward and backward.  The ramp also checks that the bias rides the 5th MFMA as bf16 hi + lo.

    Backward tolerance at ramp 0.3: the last ~10 keys take all the mass, so dV/dK of those keys are sums of 384
    terms of size ~0.3 that cancel to ~0.2; the bf16 rounding of P / dS (2^-9 relative, the MFMA operand
    precision) leaves ~0.012 per sum at 1 sigma, ~0.04-0.06 for the worst of 98k elements (measured: worst
    error/tolerance 0.96 at atol 3e-2 — 0.186 vs 0.222 — identical before and after the round-4 mask rewrite,
    and one element over it in one run)."""
    _attn_case(cuda, 2, 384, 2, 0.1, masked=True, ramp=ramp, bwd_atol=6e-2 if ramp == 0.3 else 3e-2)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("L", [384, 100])
def test_attention_slow_path_forced(cuda, p, L):
    """attn_set_force_slow(1) sends every workgroup of the ring forward down its slow path (per-tile max and
    rescale, per-wave LDS staging): rule 26 of the kernel playbook — the rare branch gets its own test."""
    k = _native.kernels()
    k.attn_set_force_slow(1)
    try:
        _attn_case(cuda, 2, L, 2, p, masked=True)
    finally:
        k.attn_set_force_slow(0)


def test_attention_left_padded(cuda):
    """Left padding of 40 keys: the first key tile is fully masked, so the forward's m comes from masked
    scores (−10000·log2e) and the real keys overflow P — the natural trigger of the slow path."""
    _attn_case(cuda, 2, 384, 2, 0.1, masked=False, left_pad=40)


def test_adamw_and_norm(cuda):
    k = _native.kernels()
    torch.manual_seed(4)
    n = 20011
    master = torch.randn(n)
    grad = torch.randn(n)
    m, v = torch.randn(n) * 0.01, torch.rand(n) * 0.01
    segs = [(0, 5003, 0.01), (5003, 15000, 0.0), (20003, 8, 0.01)]
    chunks = []
    for gi, (s, c, wd) in enumerate(segs):
        for off in range(0, c, 8192):
            chunks.append([s + off, min(8192, c - off) | ((0 if wd > 0 else 1) << 32)])
    ch = torch.tensor(chunks, dtype=torch.int64)
    md, gd, mmd, vvd = master.to(cuda), grad.to(cuda), m.to(cuda), v.to(cuda)
    comp = torch.empty(n, dtype=torch.bfloat16, device=cuda)
    norm, coef = k.grad_norm(gd, 1.0)
    assert abs(norm.item() - grad.norm().item()) / grad.norm().item() < 1e-5
    assert abs(coef.item() - 1.0 / (grad.norm().item() + 1e-6)) < 1e-6
    k.adamw(md, comp, gd, mmd, vvd, ch.to(cuda), [1e-3, 1e-3], [0.01, 0.0], 0.9, 0.999, 1e-6, 1.0, coef)
    ref.adamw_step(master, None, grad, m, v, [(s, c, wd) for s, c, wd in segs], lr=1e-3, beta1=0.9, beta2=0.999,
                   eps=1e-6, clip_coef=coef.cpu(), correct_bias=False, step=1)
    _close(md, master, 1e-6, 1e-5, "master")
    _close(mmd, m, 1e-7, 1e-5, "exp_avg")
    _close(vvd, v, 1e-9, 1e-5, "exp_avg_sq")
    _close(comp, master, 1e-2, 1e-2, "bf16 copy")


@pytest.mark.gpu
def test_native_rccl_reducer_single_rank(cuda):
    """RCCL communicator bootstrap + allreduce(avg) fp32/bf16 + broadcast on the comm stream (world 1)."""
    k = _native.kernels()
    red = k.Reducer(0, 1, bytes(k.rccl_unique_id()), cuda.index)
    x = torch.randn(1 << 20, device=cuda)
    ref_x = x.clone()
    stream = torch.cuda.current_stream().cuda_stream
    red.allreduce_f32(x.data_ptr(), x.numel(), stream)
    red.wait(stream)
    torch.cuda.synchronize()
    assert torch.equal(x, ref_x)
    scratch = torch.empty(x.numel(), dtype=torch.bfloat16, device=cuda)
    red.allreduce_bf16(x.data_ptr(), scratch.data_ptr(), x.numel(), stream)
    red.wait(stream)
    torch.cuda.synchronize()
    torch.testing.assert_close(x, ref_x.bfloat16().float())
    red.broadcast(x.data_ptr(), x.numel(), 0, 0, stream)
    red.wait(stream)
    red.synchronize()
    assert red.world == 1 and red.rank == 0


@pytest.mark.gpu
def test_fp8_quantize_and_linear(cuda):
    k = _native.kernels()
    x = (torch.randn(512, 768, device=cuda) * 3).bfloat16()
    x8, sx = k.fp8_quantize(x)
    assert x8.dtype == torch.float8_e4m3fn and sx.numel() == 1
    amax = x.float().abs().max()
    torch.testing.assert_close(sx.float(), amax / 448.0, rtol=1e-6, atol=0)
    ref8 = (x.float() / sx).clamp(-448, 448).to(torch.float8_e4m3fn)
    assert torch.equal(x8.view(torch.uint8), ref8.view(torch.uint8))
    from ml_recipe_distributed_pytorch_amd import ops
    w = (torch.randn(256, 768, device=cuda) * 0.05).bfloat16()
    b = torch.randn(256, device=cuda).bfloat16()
    y = ops.linear_fwd_fp8(x, tuple(k.fp8_quantize(w)), b)
    ref = x.float() @ w.float().t() + b.float()
    rel = ((y.float() - ref).norm() / ref.norm()).item()
    assert rel < 0.06, rel


@pytest.mark.gpu
def test_span_head_fwd_bwd(cuda):
    k = _native.kernels()
    T, H = 1000, 768
    seq = torch.randn(T, H, device=cuda).bfloat16()
    w = torch.randn(2, H, device=cuda) * 0.05
    b = torch.randn(2, device=cuda)
    logits = k.span_fwd(seq, w, b)
    ref = seq.float() @ w.t() + b
    torch.testing.assert_close(logits, ref, atol=2e-3, rtol=2e-3)
    g = torch.randn(T, 2, device=cuda)
    dw = torch.zeros(2, H, device=cuda)
    dseq = k.span_bwd(seq, w, g, dw, False)
    torch.testing.assert_close(dseq.float(), g @ w, atol=2e-2, rtol=1e-2)
    torch.testing.assert_close(dw, g.t() @ seq.float(), atol=2e-2, rtol=1e-3)
    k.span_bwd(seq, w, g, dw, True)
    torch.testing.assert_close(dw, 2 * (g.t() @ seq.float()), atol=4e-2, rtol=1e-3)


def test_attention_grid_scale_vs_fp32_oracle(cuda):
    """Production-sized grid (B=64, 12 heads, L=384, dropout 0.1 — 2304 workgroups per launch, every CU busy
    several times over) against the fp32 oracle run on the GPU (ops/reference.py is device-agnostic)."""
    k = _native.kernels()
    torch.manual_seed(7)
    B, L, nh = 64, 384, 12
    H = nh * 64
    qkv = _bf(torch.randn(B * L, 3 * H, device=cuda))
    kb = torch.zeros(B, L, device=cuda)
    kb[::3, L - 40:] = -10000.0
    ctx, lse, bits = k.attn_fwd(qkv, kb, B, L, nh, 0.1, 99, 5, 0.125)
    ctxr, lser = ref.attn_fwd(qkv, kb, B, L, nh, 0.1, 99, 5, 0.125)
    _close(lse, lser, 1e-2, 1e-3, "lse")
    _close(ctx, ctxr, 2e-2, 2e-2, "ctx")
    dctx = _bf(torch.randn(B * L, H, device=cuda))
    dq = k.attn_bwd(dctx, qkv, ctx, lse, kb, bits, B, L, nh, 0.1, 0.125, False)
    dqr = ref.attn_bwd(dctx, qkv, ctx, lse, kb, B, L, nh, 0.1, 99, 5, 0.125)
    _close(dq, dqr, 3e-2, 3e-2, "dqkv")


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_ln_grid_scale_vs_fp32_oracle(cuda, p):
    """LayerNorm fwd/bwd at the bench's token count (T = 256·384 = 98304, H = 768) vs the fp32 oracle on GPU."""
    k = _native.kernels()
    torch.manual_seed(8)
    T, H = 98304, 768
    a, r = _bf(torch.randn(T, H, device=cuda)), _bf(torch.randn(T, H, device=cuda))
    gamma, beta = torch.randn(H, device=cuda) * 0.5 + 1, torch.randn(H, device=cuda) * 0.1
    y, z, m, rs = k.ln_fwd(a, r, gamma, beta, 1e-12, p, 4321, 3)
    yr, zr, mr, rr = ref.ln_fwd(a, r, gamma, beta, 1e-12, p, 4321, 3)
    _close(z, zr, 1e-2, 1e-2, "z")
    _close(y, yr, 3e-2, 2e-2, "y")
    dy, dy2 = _bf(torch.randn(T, H, device=cuda)), _bf(torch.randn(T, H, device=cuda))
    gg = [torch.zeros(H, device=cuda) for _ in range(3)]
    ggr = [torch.zeros(H, device=cuda) for _ in range(3)]
    dz, da = k.ln_bwd(dy, dy2, z, gamma, m, rs, p, 4321, 3, gg[0], gg[1], gg[2], False)
    dzr, dar = ref.ln_bwd(dy, dy2, z, gamma, m, rs, p, 4321, 3, ggr[0], ggr[1], ggr[2], False)
    _close(dz, dzr, 3e-2, 2e-2, "dz")
    _close(da, dar, 3e-2, 2e-2, "da")
    # column sums over 98304 rows of the SAME bf16 inputs: the two sides differ only by fp32 summation order, so
    # the bound is relative to each column's Σ|term| (fp32 order error ~ sqrt(T)·2^-24 of it), not an absolute 2.0
    g = dy.float() + dy2.float()
    xh = (z.float() - m[:, None]) * rs[:, None]
    abs_sums = [(g * xh).abs().sum(0), g.abs().sum(0), dar.float().abs().sum(0)]
    for i, n in enumerate(["dgamma", "dbeta", "dbias"]):
        err = (gg[i] - ggr[i]).abs()
        bound = 1e-4 * abs_sums[i] + 1e-4
        assert bool((err <= bound).all()), f"{n}: max err/bound {float((err / bound).max()):.3f}"
