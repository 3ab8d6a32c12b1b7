"""Attention kernels (csrc/kernels/attention_fwd.hip, attention_bwd.hip, the fp32 flash attention of
f32_attention.hip) against a float64 oracle with per-row error bounds, and exact probes of every (query, key) term.

Oracle (tests/attn_oracle.py): float64 forward and backward from the bf16 inputs; its own lse, ctx and δ; the
dropout mask of ``ops.rng.keep_mask``.  Beside each output it returns the sum of the absolute values of the terms
that form it:

    A_ctx = Pd·|V|      A_v = Pdᵀ·|dO|      A_q = scale·Ŝ·|K|      A_k = scale·Ŝᵀ·|Q|
    Ŝ = P∘(|dP∘keep·ks| + Σ_d |dO_d·ctx_d|)        (the terms of dS = P∘dP − P·δ, δ = Σ_d dO_d·ctx_d)

Ŝ and not |dS|: where one key holds all the mass of a row (a single live key, L = 1, the key-bias ramp 0.3) dS
cancels to exactly 0 in the oracle, while the kernels form δ from the bf16 ctx they stored (dq kernel, ``dpart``),
which is 2⁻⁹ of its terms away; with |dS| the CPU emulation itself sits at 24 (ramp 0.3) or ∞ (one live key, L = 1
with dropout) times 2⁻⁹·‖A‖.

Checks, per output and case (a row is the 64-vector of one batch, head and token):

    per row     ‖kernel − oracle‖₂ <= K_ROW · 2⁻⁹ · ‖A_row‖₂ + TINY
    aggregate   ‖kernel − oracle‖_F / ‖oracle‖_F <= G_REL[output]
    gain        |<kernel − oracle, oracle>| / ‖oracle‖²_F <= G_GAIN
    lse         |kernel − oracle| <= 1e-2 + 1e-3·|oracle|

The constants come from the CPU emulation of the kernels' roundings (attn_oracle.emulate), not from the kernels:
K_ROW = 4 × its worst per-row ratio over CASES, rounded up; G_REL = 3 × its worst relative Frobenius error, per
output, rounded up at the second digit; G_GAIN = 3 × its worst gain.  The factors cover what the emulation does
not model (accumulation order, FMA contraction, exp2 / log2 approximations).
``test_emulation_pins_the_constants`` holds the emulation to K_ROW/4, G_REL/3 and G_GAIN/3 on every case and fails
if a constant is more than 5 % (the gain: 10 %) above what its rule gives; ``test_mutants_are_rejected`` shows each
planted mistake beyond twice a bound.  Both run without a GPU.

    K_ROW = 7      G_REL = ctx 8.6e-3, dq 9.0e-3, dk 1.03e-2, dv 9.1e-3      G_GAIN = 7e-4      K_F32 = 24

* G_REL of dK is not below 1e-2: dK carries four bf16 roundings in series (Q·c in the scores, dS, Q·c as the MFMA
  operand, the output), each of rms 1.67e-3 relative (bf16 keeps 8 significant bits), 3.4e-3 together on every
  case; the other outputs carry three.
* The gain check is there for the mistake "dQ scaled by 1.01": it reaches 1.0–1.2 per row and 1.0e-2 in the
  Frobenius norm — under 2·K_ROW and 2·G_REL, since 1 % is only 3.4 × the rounding noise — but 1.0e-2 of gain
  against 2.3e-4 for the emulation's worst.
* An aggregate is not formed for an output that is smaller as a whole than 2⁻⁹ of its own A (dQ, dK with a single
  live key: 1e-16 against 25); its rows are still bounded.
* TINY = 1e-30 is the absolute floor for rows whose A is 0 (dK, dV of masked keys: exactly 0 on both sides) or
  below what fp32 can hold (under the ramp 0.3 the first keys have P = 2⁻¹⁶⁵: A = 1e-47).  It is 1e9 below the
  smallest bound of a row without underflow (ramp 0.3 at L = 160: K_ROW·2⁻⁹·7e-19 = 1e-20).

Worst figures over CASES (SLOW_CASES for the forced slow path): per-row ratio in units of 2⁻⁹·‖A_row‖, relative
Frobenius error, gain; the kernels' are from an MI355X.

    output   emulation                 kernels, fast path        kernels, forced slow path
    ctx      1.74  2.84e-3  1.5e-4     3.02  2.93e-3  3.6e-4     0.92  2.73e-3  2.7e-5
    dq       0.75  2.96e-3  1.7e-4     0.97  3.19e-3  1.7e-4     0.55  2.93e-3  4.8e-5
    dk       0.75  3.41e-3  1.9e-4     0.76  3.64e-3  1.8e-4     0.69  3.37e-3  6.6e-5
    dv       1.68  2.98e-3  2.2e-4     1.67  2.98e-3  2.2e-4     0.64  2.90e-3  9.3e-5
    lse      7.0e-3 (3.6e-2 where a batch has no live key, |lse| = 1e4): the same for the emulation and the kernels

The kernels' ctx reaches 3.0 (2.3 at L = 1) on rows with a single live key, where the emulation has 0: the fast
path keeps the first tile's max rounded to bf16, so that key's P is not exactly 1 and is rounded to bf16, while the
emulation, like the slow path, subtracts the true max.
fp8 modes: the bf16 outputs are bitwise those of the plain kernels (asserted), so the figures above hold for them;
the bpart column sums reach 0.005 of their bound.  fp32 flash attention, per-row ratio in units of 2⁻²⁴·‖A_row‖:
fp32 CPU reference 5.63 (K_F32 = 4 × 5.63, rounded up to 24 to leave room for another fp32 summation order on
another CPU), kernels 3.22.
"""
import math
from unittest import mock

import pytest
import torch

import attn_oracle as ao
from ml_recipe_distributed_pytorch_amd import _native
from ml_recipe_distributed_pytorch_amd.ops import reference as ref
from ml_recipe_distributed_pytorch_amd.ops import rng

K_ROW = 7
G_REL = {"ctx": 8.6e-3, "dq": 9.0e-3, "dk": 1.03e-2, "dv": 9.1e-3}
G_GAIN = 7e-4
TINY = 1e-30
K_F32 = 24
SCALE, SEED, OPID = ao.SCALE, ao.SEED, ao.OPID

LENGTHS = [1, 31, 32, 33, 64, 96, 100, 127, 128, 129, 160, 200, 256, 300, 384, 385, 480, 511, 512]
MASKS = [("left40", 0.0), ("tile", 0.0), ("one", 0.0), ("allmasked", 0.0), ("tail", 0.05), ("tail", 0.3)]
# (B, L, nh, p, mask, ramp).  B = nh = 3: 9·ceil(L/128) workgroups, never a multiple of 8 (the remainder branch of
# the XCD remap), and a ragged tail that overran batch b would land in compared rows of batch b + 1
CASES = [(3, L, 3, p, "tail", 0.0) for L in LENGTHS for p in (0.0, 0.1)]
CASES += [(3, 200, 3, 0.5, "tail", 0.0), (1, 300, 1, 0.1, "tail", 0.0)]       # p = 0.5; a grid of 3 < 8 workgroups
CASES += [(3, L, 3, p, mask, ramp) for L in (100, 160, 384) for mask, ramp in MASKS for p in (0.0, 0.1)]
SLOW_CASES = [(3, 100, 3, 0.1, "tail", 0.0), (3, 160, 3, 0.1, "tail", 0.0), (3, 384, 3, 0.0, "tail", 0.0)]
F32_CASES = [(2, L, 3, p) for L in (1, 33, 77, 128, 200) for p in (0.0, 0.1)]
MUTANT_CASES = [(3, 384, 3, 0.1, "tail", 0.0), (3, 100, 3, 0.1, "tail", 0.0)]
FLIP_CASES = [(3, 33, 3, 0.1, "tail", 0.0), (3, 64, 3, 0.1, "tail", 0.0)]      # one dropout bit: L <= 64


def _id(case):
    return "-".join(str(x) for x in case)


def _check(got, orc, what, k_row=K_ROW, u=ao.U_BF16, aggregates=True):
    """The per-row, aggregate and gain bounds for every output in ``got``; returns the measured figures."""
    m = ao.measure(got, orc, u, TINY)
    print(f"[attn-oracle] {what}: " + "  ".join(f"{n} {r:.2f} {g:.2e} {gn:.1e}" for n, (r, g, gn) in m.items()))
    for n, (r, g, gn) in m.items():
        assert r <= k_row, f"{what}: {n} row error {r:.2f} × u·‖A_row‖ (bound {k_row})"
        if aggregates:
            assert g <= G_REL[n], f"{what}: {n} relative Frobenius error {g:.3e} (bound {G_REL[n]:.1e})"
            assert gn <= G_GAIN, f"{what}: {n} gain {gn:.3e} (bound {G_GAIN:.1e})"
    return m


def _check_lse(lse, orc, what):
    err = (lse.detach().double().cpu() - orc["lse"]).abs()
    tol = 1e-2 + 1e-3 * orc["lse"].abs()
    print(f"[attn-oracle] {what}: lse {float(err.max()):.2e}")
    assert bool((err <= tol).all()), f"{what}: lse error {float(err.max()):.3e}"


# ===================================================================================== CPU: oracle and constants
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_oracle_matches_reference_in_float64(p):
    """The oracle is ops.reference.attn_fwd / attn_bwd evaluated in float64 (their ``.float()`` made ``.double()``
    for the call; the keep scale stays the fp32 one, 3e-8 away), fed its own ctx and lse."""
    B, L, nh = 2, 77, 2
    qkv, kb, dctx = ao.make_inputs(B, L, nh, "tail", 0.05)
    orc = ao.oracle(qkv, kb, dctx, B, L, nh, p, ao.keep_matrix(B, nh, L, p))
    with mock.patch.object(torch.Tensor, "float", lambda self: self.double()):
        ctx, lse = ref.attn_fwd(qkv.double(), kb.double(), B, L, nh, p, SEED, OPID, SCALE)
        dqkv = ref.attn_bwd(dctx.double(), qkv.double(), ctx, lse, kb.double(), B, L, nh, p, SEED, OPID, SCALE)
    assert ctx.dtype == torch.float64 and dqkv.dtype == torch.float64
    got = dict(zip(("dq", "dk", "dv"), ao.unpack_dqkv(dqkv, B, L, nh)), ctx=ao.unpack_ctx(ctx, B, L, nh))
    for n in ("ctx", "dq", "dk", "dv"):
        assert float((got[n] - orc[n]).abs().max()) <= 1e-6 * float(orc[n].abs().max()), n
    assert float((lse - orc["lse"]).abs().max()) <= 1e-9


def test_emulation_pins_the_constants():
    """The emulation of the kernels' roundings stays within K_ROW/4, G_REL/3 and G_GAIN/3 on every GPU case, and
    no constant is larger than its rule gives (K_ROW the next integer, the others within 5 %)."""
    worst = {n: [0.0, 0.0, 0.0] for n, _ in ao.OUTPUTS}
    lse_worst = 0.0
    for case in CASES:
        _, orc, emu = ao.bf16_case(*case)
        m = ao.measure(emu, orc, ao.U_BF16, TINY)
        for n, fig in m.items():
            worst[n] = [max(a, b) for a, b in zip(worst[n], fig)]
            assert fig[0] <= K_ROW / 4 and fig[1] <= G_REL[n] / 3 and fig[2] <= G_GAIN / 3, (case, n, fig)
        lse_err = (emu["lse"] - orc["lse"]).abs()
        assert bool((lse_err <= 1e-2 + 1e-3 * orc["lse"].abs()).all()), case
        lse_worst = max(lse_worst, float(lse_err.max()))
    print("[attn-oracle] emulation worst (row, frobenius, gain): "
          + "  ".join(f"{n} {w[0]:.3f} {w[1]:.3e} {w[2]:.2e}" for n, w in worst.items()) + f"  lse {lse_worst:.1e}")
    assert math.ceil(4 * max(w[0] for w in worst.values())) == K_ROW
    for n, w in worst.items():
        assert 0.95 * G_REL[n] <= 3 * w[1] <= G_REL[n], (n, w[1])
    assert 0.9 * G_GAIN <= 3 * max(w[2] for w in worst.values()) <= G_GAIN


@pytest.mark.parametrize("mutant", ao.MUTANTS)
def test_mutants_are_rejected(mutant):
    """Each planted mistake is beyond TWICE a bound (a row, the aggregate or the gain of some output) on every
    case it is planted in: the seam and scale mistakes at L = 384 and 100, the flipped dropout bit at L <= 64."""
    for case in (FLIP_CASES if mutant == "keep_bit_flip" else MUTANT_CASES):
        B, L, nh, p, mask, ramp = case
        inp, orc, _ = ao.bf16_case(*case)
        bad = ao.oracle(*inp, B, L, nh, p, ao.keep_matrix(B, nh, L, p), mutant=mutant)
        m = ao.measure(bad, orc, ao.U_BF16, TINY)
        print(f"[attn-oracle] mutant {mutant} {_id(case)}: "
              + "  ".join(f"{n} {r:.1f} {g:.1e} {gn:.1e}" for n, (r, g, gn) in m.items()))
        assert any(r > 2 * K_ROW or g > 2 * G_REL[n] or gn > 2 * G_GAIN for n, (r, g, gn) in m.items()), (case, m)


def test_fp32_reference_pins_k_f32():
    """Noise model of the fp32 flash attention: the fp32 CPU reference (ops.reference on the fp32 inputs, fed its
    own ctx and lse) against the oracle stays within K_F32/4 per row, in units of 2⁻²⁴·‖A_row‖."""
    worst = 0.0
    for B, L, nh, p in F32_CASES:
        (qkv, kb, dctx), orc = ao.f32_case(B, L, nh, p)
        ctx, lse = ref.attn_fwd(qkv, kb, B, L, nh, p, SEED, OPID, SCALE)
        dqkv = ref.attn_bwd(dctx, qkv, ctx, lse, kb, B, L, nh, p, SEED, OPID, SCALE)
        got = dict(zip(("dq", "dk", "dv"), ao.unpack_dqkv(dqkv, B, L, nh)), ctx=ao.unpack_ctx(ctx, B, L, nh))
        m = ao.measure(got, orc, ao.U_F32, TINY)
        worst = max([worst] + [fig[0] for fig in m.values()])
        assert all(fig[0] <= K_F32 / 4 for fig in m.values()), ((B, L, nh, p), m)
    print(f"[attn-oracle] fp32 reference worst row ratio {worst:.2f}")
    assert 4 * worst > 0.85 * K_F32, "K_F32 is larger than its rule gives"


# ============================================================================================ GPU: bf16 kernels
def _run_bf16(cuda, case):
    """Ring forward and the two-kernel backward on the case's inputs -> (outputs in head layout, lse, raw)."""
    B, L, nh, p, _, _ = case
    (qkv, kb, dctx), orc, _ = ao.bf16_case(*case)
    k = _native.kernels()
    qkv, kb, dctx = qkv.to(cuda), kb.to(cuda), dctx.to(cuda)
    ctx, lse, bits = k.attn_fwd(qkv, kb, B, L, nh, p, SEED, OPID, SCALE)
    dqkv = k.attn_bwd(dctx, qkv, ctx, lse, kb, bits, B, L, nh, p, SCALE, True)
    got = dict(zip(("dq", "dk", "dv"), ao.unpack_dqkv(dqkv, B, L, nh)), ctx=ao.unpack_ctx(ctx, B, L, nh))
    return got, lse, orc, (qkv, kb, dctx, ctx, bits, dqkv)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_attention_against_oracle(cuda, case):
    """Every instantiation of the ring kernels — unrolled (L = 128, 256, 384, 512), rolled even (L % 32 == 0) and
    rolled ragged, with and without dropout, on both sides of each 32-key and 128-row seam — and every mask
    pattern, against the float64 oracle."""
    got, lse, orc, _ = _run_bf16(cuda, case)
    _check_lse(lse, orc, _id(case))
    _check(got, orc, _id(case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", SLOW_CASES, ids=_id)
def test_attention_forced_slow_path_against_oracle(cuda, case):
    """The forward's slow path (per-tile max and rescale) in a ragged, a rolled-even and an unrolled kernel."""
    k = _native.kernels()
    k.attn_set_force_slow(1)
    try:
        got, lse, orc, _ = _run_bf16(cuda, case)
    finally:
        k.attn_set_force_slow(0)
    _check_lse(lse, orc, "slow " + _id(case))
    _check(got, orc, "slow " + _id(case))


# ================================================================================================ GPU: exact probes
PB, PNH = 2, 2


def _probe_bias(L, cuda):
    """No bias but a padded tail (1 key in batch 0, 8 in batch 1) -> (key_bias, live [B, L] bool, live counts)."""
    kb = ao.key_bias(PB, L, "tail")
    live = kb == 0
    return kb.to(cuda), live, live.sum(-1).double()


def _want_keep(L, p, live):
    keep = ao.keep_matrix(PB, PNH, L, p)
    keep = torch.ones(PB, PNH, L, L, dtype=torch.bool) if keep is None else keep
    return keep & live[:, None, None, :]


def _block_onehot(L, j):
    """[L, 64] with row 64j + c one-hot at column c (c < 64, 64j + c < L), every other row 0."""
    x = torch.zeros(L, 64)
    n = min(64, L - 64 * j)
    x[64 * j + torch.arange(n), torch.arange(n)] = 1.0
    return x


def _tokens(x_heads, L):
    """[L, 64] per-head pattern -> [B·L, nh·64] bf16 (the same pattern in every batch and head)."""
    return x_heads.repeat(PB, PNH).to(torch.bfloat16)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [128, 160, 100])
@pytest.mark.parametrize("p", [0.1, 0.0])
def test_probe_forward_terms(cuda, L, p):
    """Q = 0 makes P uniform over the live keys; V one-hot over a 64-key block makes ctx[q, c] =
    keep[q, 64j + c]·ks/n_live: ⌈L/64⌉ launches read back the whole keep matrix the forward applied.  It equals
    ops.rng.keep_mask on the live keys (all ones at p = 0: each term once) and is exactly 0 on padded keys."""
    k = _native.kernels()
    kb, live, nlive = _probe_bias(L, cuda)
    ks = rng.keep_scale(p) if p > 0 else 1.0
    H = PNH * 64
    got = torch.zeros(PB, PNH, L, L)
    for j in range((L + 63) // 64):
        qkv = torch.zeros(PB * L, 3 * H, dtype=torch.bfloat16)
        qkv[:, 2 * H:] = _tokens(_block_onehot(L, j), L)
        ctx, _, _ = k.attn_fwd(qkv.to(cuda), kb, PB, L, PNH, p, SEED, OPID, SCALE)
        n = min(64, L - 64 * j)
        got[..., 64 * j:64 * j + n] = ao.unpack_ctx(ctx, PB, L, PNH)[..., :n].float()
    padded = ~live[:, None, None, :].expand_as(got)
    assert bool((got[padded] == 0).all()), "padded keys must contribute exactly 0"
    unit = (ks / nlive)[:, None, None, None]
    read = got.double() / unit
    assert float((read - read.round()).abs().max()) < 0.02, "values are 0 or ks/n_live up to bf16 rounding"
    assert torch.equal(read > 0.5, _want_keep(L, p, live))


@pytest.mark.gpu
@pytest.mark.parametrize("L", [128, 160, 100])
@pytest.mark.parametrize("p", [0.1, 0.0])
def test_probe_backward_dv_terms(cuda, L, p):
    """The bits the dK/dV kernel gathers: with Q = 0 and dO one-hot over a 64-query block,
    dV[k, c] = keep[64j + c, k]·ks/n_live for a live key k and exactly 0 for a padded one."""
    k = _native.kernels()
    kb, live, nlive = _probe_bias(L, cuda)
    ks = rng.keep_scale(p) if p > 0 else 1.0
    H = PNH * 64
    g = torch.Generator().manual_seed(L)
    qkv = torch.zeros(PB * L, 3 * H, dtype=torch.bfloat16)
    qkv[:, H:] = torch.randn(PB * L, 2 * H, generator=g).to(torch.bfloat16)     # K, V: no part in dV here
    qkv = qkv.to(cuda)
    ctx, lse, bits = k.attn_fwd(qkv, kb, PB, L, PNH, p, SEED, OPID, SCALE)
    got = torch.zeros(PB, PNH, L, L)                                         # [.., q, k]
    for j in range((L + 63) // 64):
        dctx = _tokens(_block_onehot(L, j), L).to(cuda)
        dqkv = k.attn_bwd(dctx, qkv, ctx, lse, kb, bits, PB, L, PNH, p, SCALE, True)
        n = min(64, L - 64 * j)
        dv = ao.unpack_dqkv(dqkv, PB, L, PNH)[2]                              # [.., k, c]
        got[..., 64 * j:64 * j + n, :] = dv[..., :n].transpose(-1, -2).float()
    padded = ~live[:, None, None, :].expand_as(got)
    assert bool((got[padded] == 0).all()), "padded keys must receive exactly 0"
    read = got.double() / (ks / nlive)[:, None, None, None]
    assert float((read - read.round()).abs().max()) < 0.02
    assert torch.equal(read > 0.5, _want_keep(L, p, live))


@pytest.mark.gpu
@pytest.mark.parametrize("L", [128, 160, 100])
@pytest.mark.parametrize("p", [0.1, 0.0])
def test_probe_backward_dq_terms(cuda, L, p):
    """The bits the dQ kernel applies: Q = 0, K one-hot over the 64-key block j, V = e₀ on that block only and
    dO = e₀, so dP[q, k] = [k in block], δ_q = ks·(kept live keys of the block)/n_live and
    dQ[q, c] = scale/n_live·(keep[q, 64j + c]·ks − δ_q) for a live key, exactly 0 for a padded one.  δ is taken
    from ops.rng.keep_mask, not from the kernel."""
    k = _native.kernels()
    kb, live, nlive = _probe_bias(L, cuda)
    ks = rng.keep_scale(p) if p > 0 else 1.0
    H = PNH * 64
    want = _want_keep(L, p, live)
    dctx = torch.zeros(L, 64)
    dctx[:, 0] = 1.0
    dctx = _tokens(dctx, L).to(cuda)
    read = torch.zeros(PB, PNH, L, L, dtype=torch.float64)
    raw = torch.zeros(PB, PNH, L, L)
    for j in range((L + 63) // 64):
        n = min(64, L - 64 * j)
        v = torch.zeros(L, 64)
        v[64 * j:64 * j + n, 0] = 1.0
        qkv = torch.zeros(PB * L, 3 * H, dtype=torch.bfloat16)
        qkv[:, H:2 * H] = _tokens(_block_onehot(L, j), L)
        qkv[:, 2 * H:] = _tokens(v, L)
        qkv = qkv.to(cuda)
        ctx, lse, bits = k.attn_fwd(qkv, kb, PB, L, PNH, p, SEED, OPID, SCALE)
        dqkv = k.attn_bwd(dctx, qkv, ctx, lse, kb, bits, PB, L, PNH, p, SCALE, True)
        dq = ao.unpack_dqkv(dqkv, PB, L, PNH)[0][..., :n]                     # [.., q, c]
        delta = ks * want[..., 64 * j:64 * j + n].double().sum(-1, keepdim=True) / nlive[:, None, None, None]
        raw[..., 64 * j:64 * j + n] = dq.float()
        # a block that holds every live key of a batch has δ = 1 at p = 0 (dS = 0): L > 64 rules it out
        read[..., 64 * j:64 * j + n] = (dq * nlive[:, None, None, None] / SCALE + delta) / ks
    padded = ~live[:, None, None, :].expand_as(raw)
    assert bool((raw[padded] == 0).all()), "padded keys must contribute exactly 0"
    livem = ~padded
    assert float((read - read.round()).abs()[livem].max()) < 0.05
    assert torch.equal((read > 0.5) & livem, want)


# ==================================================================================================== GPU: fp8 modes
def _close_codes(got, exp, frac):
    diff = (got.view(torch.uint8).int() - exp.view(torch.uint8).int()).abs()
    assert diff.max().item() <= 1 and (diff > 0).float().mean().item() < frac


@pytest.mark.gpu
@pytest.mark.parametrize("L", [100, 160, 128, 256, 512])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_fp8_backward_modes_away_from_384(cuda, L, p):
    """The e5m2-writing backward (MODE 1) and the e5m2-only backward with bias-gradient partials (MODE 2): a ring
    three tiles deep and another LDS layout than the bf16 path, in the rolled ragged and rolled even kernels and the
    unrolled ones of L = 128, 256, 512 (384: tests/test_fp8_gpu.py)."""
    from test_fp8_gpu import _q5
    case = (3, L, 3, p, "tail", 0.0)
    B, nh, H = 3, 3, 192
    _, lse, orc, (qkv, kb, dctx, ctx, bits, plain) = _run_bf16(cuda, case)
    k = _native.kernels()
    state = torch.zeros(4, device=cuda)
    dqkv, dqkv8 = k.attn_bwd_q8(dctx, qkv, ctx, lse, kb, bits, B, L, nh, p, SCALE, False, state, 0)
    assert torch.equal(dqkv, plain), "MODE 1: the bf16 dQKV is the plain backward's, bitwise"
    assert dqkv8.dtype == torch.float8_e5m2 and state[3].item() == 1.0
    _close_codes(dqkv8, _q5(dqkv, 1.0), 0.05)
    dqkv_b, d8b = k.attn_bwd_q8(dctx, qkv, ctx, lse, kb, bits, B, L, nh, p, SCALE, False, state, 1)
    s = state[3].item()
    assert torch.equal(dqkv_b, plain)
    _close_codes(d8b, _q5(dqkv, s), 0.05)
    st2 = state.clone()
    r2 = k.attn_bwd_q8(dctx, qkv, ctx, lse, kb, bits, B, L, nh, p, SCALE, False, st2, 1, write_bf16=False)
    assert r2[0].numel() == 0 and torch.equal(r2[1].view(torch.uint8), d8b.view(torch.uint8))
    bpart = r2[2]
    assert bpart.shape == (B * ((L + 31) // 32), 3 * H)
    assert bool(torch.isfinite(bpart).all())
    colsum = bpart.double().sum(0).cpu()
    want = ao.pack_dqkv(orc["dq"], orc["dk"], orc["dv"]).sum(0)
    bound = K_ROW * ao.U_BF16 * ao.pack_dqkv(orc["A_q"], orc["A_k"], orc["A_v"]).sum(0)
    ratio = float(((colsum - want).abs() / bound).max())
    print(f"[attn-oracle] fp8 L{L} p{p}: bpart column sums at {ratio:.3f} of their bound")
    assert ratio <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("L", [100, 160, 128, 256, 512])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_fp8_forward_ctx8_away_from_384(cuda, L, p):
    """The forward with the e4m3 copy of ctx: ctx, lse and the keep bits are the plain forward's bitwise, and
    ctx8 = e4m3(bf16 ctx / s)."""
    case = (3, L, 3, p, "tail", 0.0)
    B, nh = 3, 3
    (qkv, kb, _), _, _ = ao.bf16_case(*case)
    k = _native.kernels()
    qkv, kb = qkv.to(cuda), kb.to(cuda)
    plain = k.attn_fwd(qkv, kb, B, L, nh, p, SEED, OPID, SCALE)
    state = torch.zeros(4, device=cuda)
    out = k.attn_fwd(qkv, kb, B, L, nh, p, SEED, OPID, SCALE, q8=state, phase=0)
    for x, y in zip(out[:3], plain):
        assert torch.equal(x, y)
    ctx = out[0].float()
    assert out[3].dtype == torch.float8_e4m3fn and state[3].item() == 1.0
    assert torch.equal(out[3].view(torch.uint8), ctx.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8))
    amax = state[:3].view(torch.int32)[0].view(torch.float32).item()
    assert amax == ctx.abs().max().item()
    out2 = k.attn_fwd(qkv, kb, B, L, nh, p, SEED, OPID, SCALE, q8=state, phase=1)
    s = state[3].item()
    assert torch.equal(out2[0], plain[0])
    exp = (ctx / s).clamp(-448, 448).to(torch.float8_e4m3fn)
    diff = (out2[3].view(torch.uint8).int() - exp.view(torch.uint8).int()).abs()
    assert diff.max().item() <= 1 and (diff > 0).float().mean().item() < 1e-4   # x·(1/s) against x/s


# ============================================================================================ GPU: fp32 attention
@pytest.mark.gpu
@pytest.mark.parametrize("case", F32_CASES, ids=_id)
def test_f32_attention_against_oracle(cuda, case):
    """The fp32 flash attention (f32_attention.hip) in the same per-row form with u = 2⁻²⁴."""
    B, L, nh, p = case
    (qkv, kb, dctx), orc = ao.f32_case(*case)
    k = _native.kernels()
    qkv, kb, dctx = qkv.to(cuda), kb.to(cuda), dctx.to(cuda)
    ctx, lse = k.f32_attn_fwd(qkv, kb, B, L, nh, p, SEED, OPID, SCALE)
    dqkv = k.f32_attn_bwd(dctx, qkv, ctx, lse, kb, B, L, nh, p, SEED, OPID, SCALE)
    got = dict(zip(("dq", "dk", "dv"), ao.unpack_dqkv(dqkv, B, L, nh)), ctx=ao.unpack_ctx(ctx, B, L, nh))
    err = (lse.double().cpu() - orc["lse"]).abs()
    assert float(err.max()) <= 1e-5 * float(orc["lse"].abs().max()), f"lse {float(err.max()):.2e}"
    _check(got, orc, "f32 " + _id(case), k_row=K_F32, u=ao.U_F32, aggregates=False)
