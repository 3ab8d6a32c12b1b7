"""Float64 oracle, rounding emulation, per-element bounds, planted mistakes and exact integer probes for the bf16 NT
GEMM tests (test_gemm_oracle_gpu.py).  Nothing here takes a value from a kernel; every function works on the device
of its inputs, so the CPU tests and the GPU tests share the code.

``oracle``     C = A·Bᵀ of the bf16 inputs in float64 with S = |A|·|B|ᵀ (the sum of the absolute terms), the exact
               result of each of the eight epilogues of csrc/include/hq_gemm_epi.h (C, P where the epilogue writes it,
               the column sums per ``M_block`` rows for DGELU / DMUL), GELU in the erf form (``torch.erfc``), the
               BDR keep mask from ``ops.rng.keep_mask`` at the element index m·N + n.
``bounds``     per element, from the oracle's float64 values alone, how far a correct kernel may be from them.
``emulate``    the same computation in fp32 with the kernels' bf16 roundings and the Abramowitz–Stegun Φ of
               hq_common.h: the noise model the bounds are checked against on the CPU, and the host of ``MUTANTS``.
               It models no accumulation order (the product is rounded once).
``int_probe``  integer-valued inputs for which every fp32 partial sum in any order is exact, so the kernels' output
               is determined bit for bit; ``probe_expected`` is that output.

Two rounding orders exist in the code, both correct, and the bounds accept both:

* *staged*: every main kernel (v1, v2, v3, vS without split-K) rounds acc (+ bias) to bf16 into its LDS staging tile;
  hq_epi_piece (hq_gemm_epi.h) then works on that bf16 value and rounds its result again.  RESID is
  bf16(bf16(acc) + r), DMUL bf16(bf16(acc)·gd), BDR bf16(bf16(acc + bias)·keep·ks + r).
* *splitk*: vS with ksplit > 1 (NONE / BIAS / RESID on low-fill grids with a long K) writes fp32 slabs and
  splitk_epi_kernel adds the bias or the residual to the fp32 sum and rounds once: RESID is bf16(acc + r).
  NONE and BIAS round once in either order; only RESID differs.

The accumulation term E_acc = 2·K·2⁻²⁴·S is the order-independent worst case (γ_K) of a K-term fp32 dot product,
doubled so that it also holds for an accumulator that truncates.  It is a worst-case term that grows with K: at
K = 768 it is half the bound and at K = 3072 a truncating store is no longer seen, which is why the bound tests
stop at K = 256 and long K is held by the exact probes.

Two terms beside half_ulp(exact) + E_acc keep the bounds true statements about a correct kernel (``bounds``):

* each fp32 operation of an epilogue after the accumulation (the bias add, the residual add, the products) rounds
  once more, 2⁻²⁴ of its result — 2⁻¹⁵ of a half ulp.  Where |bias| is much larger than S (the mixed-magnitude set)
  E_acc does not cover it, and a sum within 2⁻²⁴ of a bf16 tie may round either way.  The emulation stays inside
  without these terms on every test input; they are derived, not fitted.
* the half ulp is that of the value the kernel rounds, at most the one at |exact| + (the error bound of that value):
  where a staged error carries a cancelled sum (BDR, RESID) over a power of two, it is twice the half ulp of the
  exact value.  With half_ulp(exact) alone the emulation's BDR lies outside at 1 to 4 elements per shape, by up to
  1.29 times.
"""
import functools
import math

import torch

from ml_recipe_distributed_pytorch_amd.ops import rng

EPI_NONE, EPI_BIAS, EPI_GELU, EPI_DGELU, EPI_RESID, EPI_GELUD, EPI_DMUL, EPI_BDR = range(8)
EPIS = (EPI_NONE, EPI_BIAS, EPI_GELU, EPI_DGELU, EPI_RESID, EPI_GELUD, EPI_DMUL, EPI_BDR)
EPI_NAMES = ("NONE", "BIAS", "GELU", "DGELU", "RESID", "GELUD", "DMUL", "BDR")
SPLITTABLE = (EPI_NONE, EPI_BIAS, EPI_RESID)          # nts_can_split
HAS_BIAS = (EPI_BIAS, EPI_GELU, EPI_GELUD, EPI_BDR)   # hq_epi_has_bias
WRITES_P = (EPI_GELU, EPI_GELUD)                      # hq_epi_writes_p
COL_PARTIALS = (EPI_DGELU, EPI_DMUL)                  # hq_epi_col_partials
SEED, OPID, P_DROP = 77, 5, 0.1

U32 = 2.0 ** -24
# hq_normal_cdf_pdf (hq_common.h): Abramowitz–Stegun 7.1.25 with 1/√2 and ½ folded in; pinned against the header
# text by test_constants_are_those_of_the_header
C_P, C_A1, C_A2, C_A3 = 0.33267340, 0.1740121, -0.0479399, 0.3739278
C_EXP2, C_PDF = -0.72134752044448170, 0.3989422804014327
# sup |Φ_formula − Φ| over [−12, 12], measured by test_phi_formula_error (the header documents < 1.3e-5); the bounds
# use the measured figure plus 10 %
E_PHI_MEASURED = 1.10e-5
E_PHI = 1.1 * E_PHI_MEASURED
L_GELU, L_GELU_GRAD = 1.13, 0.80    # sup |gelu'| = 1.1289 (at x = √2), sup |gelu''| = 2φ(0) = 0.7979


# ------------------------------------------------------------------------------------------- number formats
def half_ulp_bf16(x):
    """The exact half ulp of bf16 at |x| (float64): 2^(floor(log2|x|) − 8), 2⁻¹³⁴ below the smallest normal."""
    _, ex = torch.frexp(x.double().abs())                 # |x| = m·2^ex, m in [0.5, 1): floor(log2|x|) = ex − 1
    hu = torch.ldexp(torch.ones_like(x, dtype=torch.float64), ex - 9)
    return torch.where(x == 0, torch.zeros_like(hu), hu).clamp_min(2.0 ** -134)


def _bf(x):
    """fp32 -> nearest bf16 (RNE, as v_cvt_pk_bf16_f32) -> fp32."""
    return x.bfloat16().float()


def _bf_trunc(x):
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def phi64(x):
    return 0.5 * torch.erfc(-x / math.sqrt(2.0))


def pdf64(x):
    return torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu64(x):
    return x * phi64(x)


def gelu_grad64(x):
    return phi64(x) + x * pdf64(x)


def normal_cdf_pdf(x, cdf_mutant=False):
    """hq_normal_cdf_pdf in the dtype of ``x`` (fp32: one rounding per operation, as the VALU code without
    contraction; rcp and exp2 correctly rounded)."""
    t = 1.0 / (C_P * x.abs() + 1.0)
    poly = ((C_A3 * t + C_A2) * t + C_A1) * t
    e = torch.exp2((x * x * C_EXP2).double()).to(x.dtype)
    q = poly * e
    cdf = torch.where(x >= 0, 1.0 - q, q)
    if cdf_mutant:
        cdf = torch.where(x < -3.0, torch.zeros_like(cdf), cdf)
    return cdf, C_PDF * e


def _block_sums(d, M_block):
    """[M, N] -> [ceil(M / M_block), N]: column sums per block of M_block rows (rows >= M do not exist)."""
    M, N = d.shape
    nb = -(-M // M_block)
    pad = torch.zeros(nb * M_block, N, dtype=d.dtype, device=d.device)
    pad[:M] = d
    return pad.view(nb, M_block, N).sum(1)


def keep_of(M, N, p, seed, opid, device):
    """(keep as float64 0/1 [M, N], keep scale): the dropout of EPI_BDR at the element index m·ldc + n, ldc = N."""
    if p <= 0.0:
        return torch.ones(M, N, dtype=torch.float64, device=device), 1.0
    return rng.keep_mask((M, N), seed, opid, p, device=device).double(), rng.keep_scale(p)


# ---------------------------------------------------------------------------------------------------- oracle
def oracle(A, B, epi, bias=None, pre=None, resid=None, p=0.0, seed=0, opid=0, M_block=256):
    """dict of float64: acc, S, C, P (None unless GELU / GELUD), part (None unless DGELU / DMUL) and what ``bounds``
    needs beside them (x: the exact pre-activation, g: the exact factor of the multiplying epilogues, m: keep·ks)."""
    Ad, Bd = A.double(), B.double()
    acc, S = Ad @ Bd.t(), Ad.abs() @ Bd.abs().t()
    M, N = acc.shape
    o = {"epi": epi, "K": A.shape[1], "M_block": M_block, "acc": acc, "S": S, "P": None, "part": None}
    if epi == EPI_NONE:
        o["C"] = acc
    elif epi == EPI_BIAS:
        o["C"] = acc + bias.double()
    elif epi in (EPI_GELU, EPI_GELUD):
        x = acc + bias.double()
        o.update(x=x, C=gelu64(x), P=x if epi == EPI_GELU else gelu_grad64(x))
    elif epi in (EPI_DGELU, EPI_DMUL):
        g = gelu_grad64(pre.double()) if epi == EPI_DGELU else pre.double()
        o.update(g=g, pre=pre.double(), C=acc * g)
        o["part"] = _block_sums(o["C"], M_block)
    elif epi == EPI_RESID:
        o["C"] = acc + resid.double()
    elif epi == EPI_BDR:
        keep, ks = keep_of(M, N, p, seed, opid, acc.device)
        x = acc + bias.double()
        o.update(x=x, m=keep * ks, C=x * (keep * ks) + resid.double())
    else:
        raise ValueError(epi)
    return o


def bounds(o):
    """{'C', 'P', 'part', 'd'}: the largest |kernel − oracle| a correct kernel may show, per element, in either
    rounding order.  A value rounded to bf16 is written rnd(v, e): v the exact value, e the bound of the error of
    what the kernel rounds; the rounding adds the half ulp of what is rounded, which is at most that at |v| + e
    (the half ulp at |v| itself where e does not reach the next binade, twice that where the staged error carries
    a cancelled sum across it), so rnd(v, e) = half_ulp_bf16(|v| + e) + e.  E_acc and the fp32 terms: module
    docstring."""
    epi, acc, C = o["epi"], o["acc"], o["C"]
    E_acc = 2.0 * o["K"] * U32 * o["S"]

    def rnd(v, e):
        return half_ulp_bf16(v.abs() + e) + e

    b = {"P": None, "part": None, "d": None}
    if epi == EPI_NONE:
        b["C"] = rnd(C, E_acc)
    elif epi == EPI_BIAS:
        b["C"] = rnd(C, E_acc + U32 * C.abs())
    elif epi in (EPI_GELU, EPI_GELUD):
        x = o["x"]
        b_pre = rnd(x, E_acc + U32 * x.abs())                       # the staged (and, for GELU, stored) pre-activation
        slack = 16.0 * U32 * (1.0 + x.abs())                        # the fp32 operations of the formula, rcp, exp2
        lip = (gelu_grad64(x).abs() + L_GELU_GRAD * b_pre).clamp_max(L_GELU)   # sup |gelu'| over x ± b_pre (Taylor)
        b["C"] = rnd(C, lip * b_pre + x.abs() * E_PHI + slack)
        b["P"] = b_pre if epi == EPI_GELU else rnd(o["P"], L_GELU_GRAD * b_pre + E_PHI + slack)
    elif epi == EPI_RESID:
        b["C"] = rnd(C, rnd(acc, E_acc) + U32 * C.abs())
    elif epi == EPI_BDR:
        x, m = o["x"], o["m"]
        b_st = rnd(x, E_acc + U32 * x.abs())
        b["C"] = rnd(C, m * b_st + U32 * (2.0 * (x * m).abs() + C.abs()))   # ks, the product, the sum: one rounding each
    elif epi in (EPI_DGELU, EPI_DMUL):
        b_st = rnd(acc, E_acc)
        b_d = o["g"].abs() * b_st + U32 * C.abs()                   # d: the unrounded product the kernel sums
        if epi == EPI_DGELU:
            e_g = E_PHI + 16.0 * U32 * (1.0 + o["pre"].abs())       # the formula's gelu' against the exact one
            b_d = b_d + (acc.abs() + b_st) * e_g
        b["d"] = b_d
        b["C"] = rnd(C, b_d)
        M, Mb = C.shape[0], o["M_block"]
        R = torch.tensor([min(Mb, M - r0) for r0 in range(0, M, Mb)], dtype=torch.float64, device=C.device)
        b["part"] = 2.0 * R[:, None] * U32 * _block_sums(C.abs() + b_d, Mb) + _block_sums(b_d, Mb)
    return b


# ------------------------------------------------------------------------------------------------- emulation
MUTANTS = ("trunc_round", "drop_last_k", "gain_1.01", "bias_next_col", "resid_next_row", "no_keep_scale",
           "keep_bit_flip", "dgelu_uses_gelu", "cdf_zero_below_-3", "part_skips_last_row", "part_sums_rows_past_M")
FLIP_AT = (5, 37)     # keep_bit_flip: the element (5 % M, 37 % N)


def emulate(A, B, epi, bias=None, pre=None, resid=None, p=0.0, seed=0, opid=0, M_block=256, order="staged",
            mutant=None):
    """{'C', 'P', 'part'} as float64 tensors holding what the kernels store, computed in fp32 with their roundings
    (module docstring); ``order`` 'staged' or 'splitk' (NONE / BIAS / RESID only); ``mutant`` plants one of MUTANTS."""
    assert order in ("staged", "splitk") and (order == "staged" or epi in SPLITTABLE)
    assert mutant is None or mutant in MUTANTS
    f32 = torch.float32
    rnd = _bf_trunc if mutant == "trunc_round" else _bf
    Ad, Bd = A.double(), B.double()
    if mutant == "drop_last_k":
        Ad, Bd = Ad[:, :-1], Bd[:, :-1]
    acc = (Ad @ Bd.t()).float()                  # ONE rounding: no accumulation order is modelled
    if mutant == "gain_1.01":
        acc = acc * 1.01
    M, N = acc.shape
    out = {"P": None, "part": None}
    if bias is not None:
        bias = bias.to(f32)
        if mutant == "bias_next_col":
            bias = bias.roll(-1)
    if resid is not None:
        resid = resid.to(f32)
        if mutant == "resid_next_row":
            resid = resid.roll(-1, 0)
    cdfm = mutant == "cdf_zero_below_-3"
    if order == "splitk":
        v = acc + bias if epi == EPI_BIAS else acc + resid if epi == EPI_RESID else acc
        out["C"] = rnd(v)
        return {n: (t.double() if t is not None else None) for n, t in out.items()}
    st = rnd(acc + bias) if epi in HAS_BIAS else rnd(acc)          # the staged tile
    if epi in (EPI_NONE, EPI_BIAS):
        out["C"] = st
    elif epi in (EPI_GELU, EPI_GELUD):
        cdf, pdf = normal_cdf_pdf(st, cdfm)
        out["C"] = rnd(st * cdf)
        out["P"] = st if epi == EPI_GELU else rnd(st * pdf + cdf)
    elif epi in (EPI_DGELU, EPI_DMUL):
        if epi == EPI_DGELU:
            x = pre.to(f32)
            cdf, pdf = normal_cdf_pdf(x, cdfm)
            g = x * cdf if mutant == "dgelu_uses_gelu" else x * pdf + cdf
        else:
            g = pre.to(f32)
        d = st * g
        out["C"] = rnd(d)
        dd = d.double()
        if mutant == "part_skips_last_row":       # the last row of the last block is left out of its column sums
            dd = dd.clone()
            dd[M - 1] = 0.0
        part = _block_sums(dd, M_block)
        if mutant == "part_sums_rows_past_M" and M % M_block:   # the tail block goes on over rows it does not own
            part[-1] += d[:M_block - M % M_block].double().sum(0)
        out["part"] = part.float()
    elif epi == EPI_RESID:
        out["C"] = rnd(st + resid)
    elif epi == EPI_BDR:
        keep, ks = keep_of(M, N, p, seed, opid, acc.device)
        if mutant == "keep_bit_flip":
            keep = keep.clone()
            keep[FLIP_AT[0] % M, FLIP_AT[1] % N] = 1.0 - keep[FLIP_AT[0] % M, FLIP_AT[1] % N]
        m = keep.float() * (1.0 if mutant == "no_keep_scale" else torch.tensor(ks, dtype=f32))
        out["C"] = rnd(st * m + resid)
    return {n: (t.double() if t is not None else None) for n, t in out.items()}


def fp32_reference(A, B, epi, bias=None, pre=None, resid=None, p=0.0, seed=0, opid=0, M_block=256):
    """The plain fp32 torch computation of the epilogue (erf GELU, no staging) rounded to bf16 once: what the
    older tests compare with.  {'C', 'P', 'part'} as float64."""
    f32 = torch.float32
    acc = A.float() @ B.float().t()
    M, N = acc.shape
    P = part = None
    x = acc + bias.to(f32) if epi in HAS_BIAS else acc
    if epi in (EPI_NONE, EPI_BIAS):
        C = x
    elif epi in (EPI_GELU, EPI_GELUD):
        C = torch.nn.functional.gelu(x)
        P = x if epi == EPI_GELU else gelu_grad64(x.double()).float()
    elif epi in (EPI_DGELU, EPI_DMUL):
        C = acc * (gelu_grad64(pre.double()).float() if epi == EPI_DGELU else pre.to(f32))
        part = _block_sums(C.double(), M_block).float()
    elif epi == EPI_RESID:
        C = acc + resid.to(f32)
    else:
        keep, ks = keep_of(M, N, p, seed, opid, acc.device)
        C = x * (keep.float() * ks) + resid.to(f32)
    return {"C": _bf(C).double(), "P": _bf(P).double() if P is not None else None,
            "part": part.double() if part is not None else None}


# ---------------------------------------------------------------------------------------------------- inputs
BOUND_SHAPES = ((256, 256, 128), (512, 384, 192), (100, 128, 64), (1268, 256, 256))
INPUT_SETS = ("small", "unit", "mixed")


def make_inputs(M, N, K, input_set, device="cpu"):
    """dict A, B (bf16), bias (fp32 [N]), resid, pre, gd (bf16 [M, N]).  'small': A ~ 0.5·N(0,1), B ~ 0.1·N(0,1);
    'unit': both N(0,1); 'mixed': 'small' with the rows of A and the columns of bias / resid scaled by powers of two
    from 2⁻¹² to 2¹² (what a max-norm check cannot see).  bias ~ U(−6, 6) puts the GELU pre-activations across
    [−6, 6], the negative tail included; pre (DGELU's stored pre-activation) ~ U(−6, 6), gd = gelu'(pre)."""
    assert input_set in INPUT_SETS
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K + INPUT_SETS.index(input_set))
    sa, sb = (1.0, 1.0) if input_set == "unit" else (0.5, 0.1)
    A = torch.randn(M, K, generator=g) * sa
    B = torch.randn(N, K, generator=g) * sb
    bias = torch.rand(N, generator=g) * 12.0 - 6.0
    resid = torch.randn(M, N, generator=g)
    pre = (torch.rand(M, N, generator=g) * 12.0 - 6.0).bfloat16()
    if input_set == "mixed":
        A = A * torch.exp2(((7 * torch.arange(M)) % 25 - 12).float())[:, None]
        cs = torch.exp2(((11 * torch.arange(N)) % 25 - 12).float())
        bias, resid = bias * cs, resid * cs
    gd = gelu_grad64(pre.double()).float().bfloat16()
    t = {"A": A.bfloat16(), "B": B.bfloat16(), "bias": bias, "resid": resid.bfloat16(), "pre": pre, "gd": gd}
    return {n: v.to(device) for n, v in t.items()}


def epi_args(inp, epi):
    """The operands of ``epi`` among the inputs, as the keywords of oracle / emulate."""
    kw = {}
    if epi in HAS_BIAS:
        kw["bias"] = inp["bias"]
    if epi in (EPI_RESID, EPI_BDR):
        kw["resid"] = inp["resid"]
    if epi == EPI_DGELU:
        kw["pre"] = inp["pre"]
    if epi == EPI_DMUL:
        kw["pre"] = inp["gd"]
    if epi == EPI_BDR:
        kw.update(p=P_DROP, seed=SEED, opid=OPID)
    return kw


@functools.lru_cache(maxsize=None)
def cpu_inputs(M, N, K, input_set):
    return make_inputs(M, N, K, input_set)


def check(got, o, b):
    """[(output, elements outside the bound, elements, largest |got − oracle| / bound, index of the worst)] for the
    outputs the epilogue has.  ``got``: float64-convertible tensors C, P, part."""
    res = []
    for n in ("C", "P", "part"):
        if o[n] is None:
            continue
        r = (got[n].double() - o[n]).abs() / b[n]
        r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
        worst = int(r.argmax())
        res.append((n, int((r > 1.0).sum()), r.numel(), float(r.flatten()[worst]),
                    (worst // r.shape[1], worst % r.shape[1])))
    return res


# ------------------------------------------------------------------------------------------ exact probes
def _hash(n, seed, device):
    """int64 tensor of n well-mixed 32-bit values, the same on every device."""
    h = (torch.arange(n, dtype=torch.int64, device=device) + 1) * 0x9E3779B1 + seed * 0x85EBCA6B
    h &= 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & 0xFFFFFFFF
    h ^= h >> 12
    h = (h * 0x297A2D39) & 0xFFFFFFFF
    h ^= h >> 15
    return h


GD_SET = (1.0, 0.5, 0.25, 0.75, -0.5, -0.125, 0.0, 1.0)     # DMUL's stored gelu': dyadic, so acc·gd is exact in fp32
PRE_SET = (16.0, -16.0, 32.0, -32.0, 64.0, -64.0, 24.0, -48.0)   # DGELU's stored pre: |x| >= 16, see int_probe


def int_probe(M, N, K, seed=0, device="cpu"):
    """Integer-valued inputs whose GEMM is exact in fp32 in ANY accumulation order, with the exact product.

    A, B: integers in [0, 7], so every partial sum is an integer <= 49·K < 2²⁴ (K <= 3072).  bias: fp32 integers,
    in [16, 79] on the even columns and −(49·K + [16, 79]) on the odd ones, so acc + bias is an integer >= 16 or
    <= −16: there hq_normal_cdf_pdf is exact (e = exp2(−0.72·x²) = 0 below 2⁻¹⁴⁹, so Φ is exactly 1 or +0 and φ is 0),
    gelu(x) = x or −0 and gelu'(x) = 1 or 0 bit for bit, while the bias add and both signs of the rounding are
    exercised.  resid: bf16 integers in [−128, 128].  gd, pre: from GD_SET / PRE_SET.  BDR runs with p = 0.5, keep
    scale exactly 2.  Sums are in the hundreds and thousands, where bf16 has a spacing of 4 and more: the generator
    asserts that at least a quarter of the staged values (acc and acc + bias) are not bf16 numbers and that exact
    ties occur, and that the DGELU / DMUL column sums are exact in any order (every term a multiple of a power of
    two g with Σ|d| <= 2²⁴·g per column block of 256 rows)."""
    assert 49 * K < 2 ** 24
    A = (_hash(M * K, 3 * seed + 1, device) % 8).view(M, K)
    B = (_hash(N * K, 3 * seed + 2, device) % 8).view(N, K)
    hb = _hash(N, 3 * seed + 3, device)
    n = torch.arange(N, device=device)
    bias = torch.where(n % 2 == 0, 16 + hb % 64, -(49 * K + 16 + hb % 64))
    hr = _hash(M * N, 3 * seed + 4, device)
    resid = (hr % 257 - 128).view(M, N)
    sel = ((hr >> 10) % 8).view(M, N)
    gd = torch.tensor(GD_SET, dtype=torch.float64, device=device)[sel]
    pre = torch.tensor(PRE_SET, dtype=torch.float64, device=device)[sel]
    pr = {"M": M, "N": N, "K": K, "A": A.bfloat16(), "B": B.bfloat16(), "bias": bias.float(),
          "resid": resid.bfloat16(), "gd": gd.bfloat16(), "pre": pre.bfloat16(), "p": 0.5, "seed": 1234 + seed,
          "opid": 9}
    acc = pr["A"].double() @ pr["B"].double().t()
    pr["acc"] = acc
    assert float(acc.max()) <= 49 * K and bool((acc == acc.round()).all())
    for v in (acc, acc + bias.double()):
        hu = half_ulp_bf16(v)
        rem = torch.remainder(v, 2.0 * hu)
        assert float((rem != 0).double().mean()) >= 0.25, "too few staged values that bf16 has to round"
        assert bool((rem == hu).any()), "no exact tie among the staged values"
    st = _rne(acc)
    for g in (gd, (pre > 0).double()):           # DMUL: acc·gd; DGELU: acc·gelu'(pre) = acc or 0
        d = st * g
        gran = 2.0 ** -3                          # every term is a multiple of 1/8; the largest common power of two
        while gran < 2.0 ** 24 and bool((torch.remainder(d, 2.0 * gran) == 0).all()):
            gran *= 2.0
        assert float(_block_sums(d.abs(), 256).max()) <= 2.0 ** 24 * gran, "column sums not exact in any order"
    return pr


def _rne(v):
    """float64 values that fp32 holds exactly -> the nearest bf16 (ties to even), as float64."""
    f = v.float()
    assert bool((f.double() == v).all()), "not exact in fp32"
    return f.bfloat16().double()


def probe_args(pr, epi):
    kw = {}
    if epi in HAS_BIAS:
        kw["bias"] = pr["bias"]
    if epi in (EPI_RESID, EPI_BDR):
        kw["resid"] = pr["resid"]
    if epi == EPI_DGELU:
        kw["pre"] = pr["pre"]
    if epi == EPI_DMUL:
        kw["pre"] = pr["gd"]
    if epi == EPI_BDR:
        kw.update(p=pr["p"], seed=pr["seed"], opid=pr["opid"])
    return kw


def probe_expected(pr, epi, order="staged", M_block=256):
    """{'C', 'P' (bf16), 'part' (fp32)}: the output of a correct kernel, bit for bit: exact integer / dyadic
    arithmetic in float64 followed by RNE, in the staged or the splitk rounding order."""
    assert order == "staged" or epi in SPLITTABLE
    acc, M, N = pr["acc"], pr["M"], pr["N"]
    bias, resid = pr["bias"].double(), pr["resid"].double()
    P = part = None
    if order == "splitk":
        C = _rne(acc + bias if epi == EPI_BIAS else acc + resid if epi == EPI_RESID else acc)
        return {"C": C.bfloat16(), "P": None, "part": None}
    st = _rne(acc + bias) if epi in HAS_BIAS else _rne(acc)
    if epi in (EPI_NONE, EPI_BIAS):
        C = st
    elif epi in (EPI_GELU, EPI_GELUD):
        assert float(st.abs().min()) >= 16.0
        pos = (st > 0).double()
        C = st * pos                                   # gelu(x) = x·1 or x·(+0)
        P = st if epi == EPI_GELU else pos             # gelu'(x) = fma(x, 0, Φ) = 1 or 0
    elif epi in (EPI_DGELU, EPI_DMUL):
        g = (pr["pre"].double() > 0).double() if epi == EPI_DGELU else pr["gd"].double()
        d = st * g
        C = _rne(d)
        part = _block_sums(d, M_block).float()
    elif epi == EPI_RESID:
        C = _rne(st + resid)
    else:
        keep, ks = keep_of(M, N, pr["p"], pr["seed"], pr["opid"], acc.device)
        assert ks == 2.0
        C = _rne(st * keep * ks + resid)
    return {"C": C.bfloat16(), "P": P.bfloat16() if P is not None else None, "part": part}
