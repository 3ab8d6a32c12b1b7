"""LAMB (train.optim.FusedLamb, ops.reference.lamb_step, csrc/kernels/optim.hip lamb_*): the float64 oracle, its
tolerance and its mutants, the CPU optimizer class, the factory and the CLI.  tests/test_lamb_gpu.py runs the
kernels through the same oracle and tolerance.

The contract (one step, one arena segment s of param group k; c = clip coefficient or 1):

    g = grad·c;  m = β1·m + (1−β1)·g;  v = β2·v + (1−β2)·g²
    u = (m·bc1) / (sqrt(v·bc2) + eps) + wd_k·p          bc = 1/(1 − β^t) or 1; eps AFTER the correction of v
    W = sqrt(Σ_s p²), U = sqrt(Σ_s u²)                   p before the update
    r = W/U if adapt_k and W > 0 and U > 0 else 1
    p = p − (lr_k·r)·u

``_step64`` writes this out in float64 (numpy, segment by segment; ``test_oracle_is_the_scalar_loop`` ties it to a
plain per-element Python loop).  It does not use ops.reference.

Tolerance, u = 2⁻²⁴, K = 16 as in tests/test_optim_gpu.py, magnitudes from the oracle:

    m   K·u·(|β1·m| + |(1−β1)·g|)          v   K·u·|v|
    W   D_s·u·W                            the inputs p are exact, so only the summation rounds: a sum of D
                                           non-negative fp32 additions is within D·u relative, the square root
                                           halves that and adds its own u: (D/2 + 1)·u <= D·u
    U   (κ_s·K + D_s)·u·U                  each u_i carries K·u·mag_i (mag_i = bc1·(|β1·m| + |(1−β1)·g|)/denom + wd·|p|,
                                           the terms that are added, with m's own cancellation counted), so
                                           δ(Σu²) <= 2·K·u·Σ|u_i|·mag_i; κ_s = Σ|u_i|·mag_i / Σu_i² >= 1 is the
                                           condition number of the segment; the square root halves the 2
    r   (κ_s·K + 2·D_s + 1)·u·r            quotient of the two, plus the division
    p   K·u·(|p| + |lr·r·u|) + |lr·r·u|·(bound of r)/r

D_s is the longest addition chain behind a segment's sum, from the order documented above lamb_moments_kernel and
lamb_ratio_kernel: 32 per-thread additions + 6 (wave butterfly) + 3 (four waves) per chunk, then
ceil(chunks_s / 64) lane-strided additions + 6 (wave butterfly): D_s = 47 + ceil(chunks_s / 64).
Where r is 1 by rule (adapt off, W = 0 or U = 0) it must be exactly 1."""
import copy
import functools
import math
import os

import numpy as np
import pytest
import torch

from ml_recipe_distributed_pytorch_amd.models.bert import BertForQuestionAnswering
from ml_recipe_distributed_pytorch_amd.models.config import get_config
from ml_recipe_distributed_pytorch_amd.ops import reference as ref
from ml_recipe_distributed_pytorch_amd.train.optim import CHUNK, FusedAdaMod, FusedAdamW, FusedLamb
from ml_recipe_distributed_pytorch_amd.train.trainer import optimizer_groups

UNIT = 2.0 ** -24
K = 16
B1, B2, EPS = 0.9, 0.999, 1e-6
LR = [0.02, 0.01, 0.02]
WD = [0.1, 0.0, 0.05]
ADAPT = [True, True, False]
STEP = 3
CLIP = float(np.float32(0.37))
P_FLOOR = 0.25
SENT = -7.25
PAD = 64

# name, numel, group, start misalignment, weight scale
SEGMENTS = [("one_chunk", CHUNK, 0, 0, 1.0),
            ("chunk_plus_one", CHUNK + 1, 1, 0, 2.0),
            ("five_unaligned", 5, 0, 3, 0.5),
            ("two", 2, 1, 0, 1.0),
            ("wrap", 70 * CHUNK, 0, 0, 1.5),
            ("zero_weights", 1031, 0, 0, 0.0),
            ("zero_update", 1028, 1, 0, 1.0),
            ("no_adapt", 2051, 2, 1, 3.0),
            ("unaligned_chunks", 2 * CHUNK + 1000, 1, 2, 0.75)]


@functools.lru_cache(maxsize=None)
def layout():
    """(segments [(start, numel, group)], arena size), in SEGMENTS order, >= PAD sentinel floats around each."""
    segs, off = [], PAD
    for _, n, g, mis, _ in SEGMENTS:
        start = (off + 3) // 4 * 4 + mis
        segs.append((start, n, g))
        off = start + n + PAD
    return tuple(segs), (off + 3) // 4 * 4


def seg_index(name):
    return [s[0] for s in SEGMENTS].index(name)


def chunk_tables():
    """The chunk table as _ArenaOptimizer builds it, and seg_first_chunk."""
    rows, first = [], [0]
    for s, n, g in layout()[0]:
        for off in range(0, n, CHUNK):
            rows.append([s + off, min(CHUNK, n - off) | (g << 32)])
        first.append(len(rows))
    return torch.tensor(rows, dtype=torch.int64), torch.tensor(first, dtype=torch.int32)


def chain_length(numel):
    return 47 + math.ceil(math.ceil(numel / CHUNK) / 64)


@functools.lru_cache(maxsize=None)
def seg_mask():
    segs, N = layout()
    mask = np.zeros(N, dtype=bool)
    for s, n, _ in segs:
        mask[s:s + n] = True
    return mask


@functools.lru_cache(maxsize=None)
def grads():
    """Gradients of steps 1..5 (float32 numpy): |g| log-uniform over 1e-4 … 1e1 through a per-element scale, 3 %
    exact zeros per step; the zero_update segment is zero in every step."""
    segs, N = layout()
    rng = np.random.default_rng(20250301)
    scale = 10.0 ** (rng.random(N) * 5.0 - 4.0)
    out = []
    for _ in range(5):
        g = scale * (0.2 + 0.8 * rng.random(N)) * np.where(rng.random(N) < 0.5, -1.0, 1.0)
        g[rng.random(N) < 0.03] = 0.0
        s, n, _ = segs[seg_index("zero_update")]
        g[s:s + n] = 0.0
        g[~seg_mask()] = SENT
        out.append(g.astype(np.float32))
    return tuple(out)


def step64(st, step=STEP, clip=CLIP, correct_bias=True, mut=None):
    """One LAMB step in float64 on ``st`` = {p, m, v, g} (numpy, any float dtype; not modified).  Returns the new
    p, m, v, ``norms`` [nseg, 3] = (W, U, r), and the magnitudes the tolerance needs."""
    segs, N = layout()
    p0, m0, v0, g0 = (np.asarray(st[k], dtype=np.float64) for k in ("p", "m", "v", "g"))
    c = 1.0 if (clip is None or mut == "no_clip") else clip
    bc1 = 1.0 / (1.0 - B1 ** step) if correct_bias else 1.0
    bc2 = 1.0 / (1.0 - B2 ** step) if correct_bias else 1.0
    out = {k: np.array(x) for k, x in (("p", p0), ("m", m0), ("v", v0))}
    out.update(m_mag=np.zeros(N), u=np.zeros(N), u_mag=np.zeros(N), step_size=np.zeros(N))
    norms = np.ones((len(segs), 3))
    group_sq = {}
    for s, n, k in segs:
        sl = slice(s, s + n)
        g = g0[sl] * c
        m = B1 * m0[sl] + (1.0 - B1) * g
        v = B2 * v0[sl] + (1.0 - B2) * g * g
        if mut == "eps_in_sqrt":
            denom = np.sqrt(v * bc2 + EPS)
        elif mut == "eps_before_correction":
            denom = (np.sqrt(v) + EPS) * math.sqrt(bc2)
        else:
            denom = np.sqrt(v * bc2) + EPS
        adam = (m * bc1) / denom
        u = adam if mut == "decay_outside" else adam + WD[k] * p0[sl]
        out["m"][sl], out["v"][sl], out["u"][sl] = m, v, u
        out["m_mag"][sl] = np.abs(B1 * m0[sl]) + np.abs((1.0 - B1) * g)
        out["u_mag"][sl] = out["m_mag"][sl] * bc1 / denom + WD[k] * np.abs(p0[sl])
        acc = group_sq.setdefault(k, [0.0, 0.0])
        acc[0] += float(np.sum(p0[sl] ** 2))
        acc[1] += float(np.sum(u ** 2))
    for i, (s, n, k) in enumerate(segs):
        sl = slice(s, s + n)
        u, p = out["u"][sl], p0[sl]
        adapt = ADAPT[k] or mut == "adapt_ignored"
        if mut == "ratio_post_update":
            W = math.sqrt(float(np.sum((p - LR[k] * u) ** 2)))
        else:
            W = math.sqrt(float(np.sum(p ** 2)))
        U = math.sqrt(float(np.sum(u ** 2)))
        if mut == "ratio_per_group":
            W, U = math.sqrt(group_sq[k][0]), math.sqrt(group_sq[k][1])
        if mut == "zero_w_zero_ratio" and adapt and W == 0.0:
            r = 0.0
        else:
            r = W / U if (adapt and W > 0.0 and U > 0.0) else 1.0
        norms[i] = (W, U, r)
        rr = np.full(n, r)
        if mut == "ratio_per_chunk" and adapt:
            for off in range(0, n, CHUNK):
                cw = math.sqrt(float(np.sum(p[off:off + CHUNK] ** 2)))
                cu = math.sqrt(float(np.sum(u[off:off + CHUNK] ** 2)))
                rr[off:off + CHUNK] = cw / cu if (cw > 0.0 and cu > 0.0) else 1.0
        out["step_size"][sl] = LR[k] * rr
        out["p"][sl] = p - (LR[k] * rr) * u
        if mut == "decay_outside":
            out["p"][sl] -= LR[k] * WD[k] * p
    out["norms"] = norms
    return out


MUTANTS = ["eps_in_sqrt", "eps_before_correction", "ratio_post_update", "decay_outside", "ratio_per_chunk",
           "ratio_per_group", "adapt_ignored", "no_clip", "zero_w_zero_ratio"]


@functools.lru_cache(maxsize=None)
def state():
    """float32 state before step 3 plus the gradient of step 3 (numpy; read-only, every user copies).  The moments come
    from two oracle steps from zero, rounded to fp32.  |p| >= P_FLOOR·scale for the reason given in
    tests/test_optim_gpu.py::_state (the bound of p takes u as exact to K·u·|u|; where m cancels, u's error is a few
    u·mag instead, which K·u·|p| covers from the floor up).  The zero-weight segment has no |p| to cover it, so its m
    is given the sign of g: no cancellation there."""
    segs, N = layout()
    rng = np.random.default_rng(7)
    p = rng.standard_normal(N)
    p = np.where(p < 0, p - P_FLOOR, p + P_FLOOR)
    for (s, n, _), (_, _, _, _, scale) in zip(segs, SEGMENTS):
        p[s:s + n] *= scale
    st = {"p": p.astype(np.float32), "m": np.zeros(N, np.float32), "v": np.zeros(N, np.float32)}
    for t in (1, 2):
        st["g"] = grads()[t - 1]
        o = step64(st, step=t)
        st["m"], st["v"] = o["m"].astype(np.float32), o["v"].astype(np.float32)
    st["g"] = grads()[STEP - 1]
    s, n, _ = segs[seg_index("zero_weights")]
    st["m"][s:s + n] = np.abs(st["m"][s:s + n]) * np.where(st["g"][s:s + n] < 0, -1.0, 1.0)
    for k in ("p", "m", "v"):
        st[k][~seg_mask()] = SENT
    for a in st.values():
        a.setflags(write=False)
    return st


def tolerance(orc):
    segs, _ = layout()
    tol = {"m": K * UNIT * orc["m_mag"], "v": K * UNIT * np.abs(orc["v"])}
    nt = np.zeros((len(segs), 3))
    move = np.abs(orc["step_size"] * orc["u"])
    tol["p"] = K * UNIT * (np.abs(orc["p"]) + move)
    for i, (s, n, k) in enumerate(segs):
        sl = slice(s, s + n)
        W, U, r = orc["norms"][i]
        D = chain_length(n)
        su = float(np.sum(orc["u"][sl] ** 2))
        kappa = float(np.sum(np.abs(orc["u"][sl]) * orc["u_mag"][sl])) / su if su > 0 else 1.0
        nt[i, 0] = D * UNIT * W
        nt[i, 1] = (kappa * K + D) * UNIT * U
        if ADAPT[k] and W > 0 and U > 0:
            rel = (kappa * K + 2 * D + 1) * UNIT
            nt[i, 2] = rel * r
            tol["p"][sl] += move[sl] * rel
    tol["norms"] = nt
    return tol


def ratios(got, orc, tol=None):
    """err / tolerance: per element of the segments for p, m, v, per segment for W, U, r (0 where both are 0)."""
    tol = tol or tolerance(orc)
    mask = seg_mask()
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for name in ("p", "m", "v"):
            g = np.asarray(got[name], dtype=np.float64)
            assert np.isfinite(g[mask]).all(), name
            err = np.abs(g - orc[name])[mask]
            out[name] = np.where(err == 0, 0.0, err / tol[name][mask])
        err = np.abs(np.asarray(got["norms"], dtype=np.float64) - orc["norms"])
        q = np.where(err == 0, 0.0, err / tol["norms"])
    out["W"], out["U"], out["r"] = q[:, 0], q[:, 1], q[:, 2]
    return out


def worst(r):
    return {k: round(float(v.max()), 3) for k, v in r.items()}


@functools.lru_cache(maxsize=None)
def chain64():
    """Oracle steps 3, 4, 5 chained in float64: (final result, 3x the largest single-step bound, element by
    element), as tests/test_optim_gpu.py::_chain64."""
    st = {k: np.asarray(v, dtype=np.float64) for k, v in state().items()}
    tol = None
    for t in (3, 4, 5):
        st["g"] = grads()[t - 1].astype(np.float64)
        orc = step64(st, step=t)
        one = tolerance(orc)
        tol = one if tol is None else {k: np.maximum(tol[k], one[k]) for k in one}
        st.update(p=orc["p"], m=orc["m"], v=orc["v"])
    return orc, {k: 3 * v for k, v in tol.items()}


def ref_step(st, step, clip, correct_bias=True):
    """ops.reference.lamb_step group by group, as FusedLamb's CPU path calls it; ``st``: torch tensors, in place.
    Returns norms [nseg, 3] in layout order."""
    segs, _ = layout()
    norms = torch.ones(len(segs), 3, dtype=st["p"].dtype)
    for k in range(len(LR)):
        rows = [i for i, sg in enumerate(segs) if sg[2] == k]
        norms[rows] = ref.lamb_step(st["p"], None, st["g"], st["m"], st["v"], [segs[i][:2] + (WD[k],) for i in rows],
                                    lr=LR[k], beta1=B1, beta2=B2, eps=EPS, clip_coef=clip, correct_bias=correct_bias,
                                    step=step, adapt=ADAPT[k])
    return norms


def torch_state(dtype=torch.float32):
    return {k: torch.from_numpy(np.array(v)).to(dtype) for k, v in state().items()}


def to_numpy(st, norms):
    out = {k: v.detach().cpu().numpy() for k, v in st.items()}
    out["norms"] = norms.detach().cpu().numpy()
    return out


# ------------------------------------------------------------------------------------------ layout and oracle
def test_layout_covers_every_path():
    segs, N = layout()
    assert N < 1_000_000
    by = {name: sg for (name, *_), sg in zip(SEGMENTS, segs)}
    ends = [0] + [s + n for s, n, _ in segs]
    starts = [s for s, _, _ in segs] + [N]
    assert all(b - a >= PAD for a, b in zip(ends, starts))
    assert by["one_chunk"][1] == CHUNK and by["one_chunk"][0] % 4 == 0
    assert by["chunk_plus_one"][1] == CHUNK + 1 and by["chunk_plus_one"][0] % 4 == 0     # second chunk: one element
    assert by["five_unaligned"][1] == 5 and by["five_unaligned"][0] % 4 != 0
    assert by["two"][1] == 2 and by["two"][0] % 4 == 0
    assert by["wrap"][1] == 70 * CHUNK and by["wrap"][1] // CHUNK > 64
    assert by["unaligned_chunks"][0] % 4 != 0 and by["unaligned_chunks"][1] > 2 * CHUNK   # scalar path, full chunks
    assert by["zero_weights"][1] % 4 == 3 and by["zero_weights"][1] // 4 > 256           # remainder loop + 3-tail
    st = state()
    orc = step64(st)
    s, n, k = by["zero_weights"]
    assert ADAPT[k] and not st["p"][s:s + n].any() and st["g"][s:s + n].any()
    assert tuple(orc["norms"][seg_index("zero_weights")][[0, 2]]) == (0.0, 1.0)
    s, n, k = by["zero_update"]
    assert ADAPT[k] and WD[k] == 0.0 and not (st["g"][s:s + n].any() or st["m"][s:s + n].any() or st["v"][s:s + n].any())
    W, U, r = orc["norms"][seg_index("zero_update")]
    assert W > 0 and U == 0.0 and r == 1.0
    assert not ADAPT[by["no_adapt"][2]]
    W, U, r = orc["norms"][seg_index("no_adapt")]
    assert r == 1.0 and abs(W / U - 1.0) > 0.5
    adapting = [k for k in range(len(LR)) if ADAPT[k] and any(sg[2] == k for sg in segs)]
    assert len(adapting) >= 2 and len({LR[k] for k in adapting}) >= 2 and len({WD[k] for k in adapting}) >= 2
    chunks, first = chunk_tables()
    assert first[-1].item() == chunks.shape[0] and len(first) == len(segs) + 1
    # ratios of one group's segments differ (else "per group" could not be told from "per segment")
    r0 = [orc["norms"][i][2] for i, sg in enumerate(segs) if sg[2] == 0]
    assert max(r0) / min(r0) > 1.5
    g = st["g"][seg_mask()]
    nz = np.abs(g[g != 0])
    assert nz.min() < 1e-3 and nz.max() > 3.0 and 0.02 < (g == 0).mean() < 0.06


def test_oracle_is_the_scalar_loop():
    """step64 against the contract as a plain per-element Python loop (floats, math.sqrt) on the two smallest
    segments and the zero-weight one."""
    segs, _ = layout()
    st = state()
    for clip, cb in ((CLIP, True), (None, False)):
        orc = step64(st, clip=clip, correct_bias=cb)
        bc1 = 1.0 / (1.0 - B1 ** STEP) if cb else 1.0
        bc2 = 1.0 / (1.0 - B2 ** STEP) if cb else 1.0
        for name in ("five_unaligned", "two", "zero_weights"):
            i = seg_index(name)
            s, n, k = segs[i]
            us, ms, vs, sw, su = [], [], [], 0.0, 0.0
            for j in range(s, s + n):
                p, g = float(st["p"][j]), float(st["g"][j]) * (1.0 if clip is None else clip)
                m = B1 * float(st["m"][j]) + (1.0 - B1) * g
                v = B2 * float(st["v"][j]) + (1.0 - B2) * g * g
                u = (m * bc1) / (math.sqrt(v * bc2) + EPS) + WD[k] * p
                us.append(u), ms.append(m), vs.append(v)
                sw += p * p
                su += u * u
            W, U = math.sqrt(sw), math.sqrt(su)
            r = W / U if (ADAPT[k] and W > 0 and U > 0) else 1.0
            np.testing.assert_allclose(orc["norms"][i], (W, U, r), rtol=1e-13)
            want_p = [float(st["p"][s + j]) - (LR[k] * r) * us[j] for j in range(n)]
            np.testing.assert_allclose(orc["p"][s:s + n], want_p, rtol=1e-13, atol=1e-300)
            np.testing.assert_allclose(orc["m"][s:s + n], ms, rtol=1e-13)
            np.testing.assert_allclose(orc["v"][s:s + n], vs, rtol=1e-13)


def test_fp32_reference_within_half_tolerance():
    """ops.reference.lamb_step in fp32 uses at most half the tolerance, one step at t = 3 (clip / none, bias
    correction on / off), and three chained steps against 3x the chain's bound.

    Measured worst err / tolerance (0.5 allowed):
        one step   p 0.130   m 0.124   v 0.251   W 0.019   U 0.031   r 0.026
        chained    p 0.053   m 0.073   v 0.104   W 0.010   U 0.010   r 0.010"""
    top = {}
    for clip, cb in ((CLIP, True), (None, True), (CLIP, False)):
        orc = step64(state(), clip=clip, correct_bias=cb)
        st = torch_state()
        norms = ref_step(st, STEP, None if clip is None else torch.tensor(clip), cb)
        r = worst(ratios(to_numpy(st, norms), orc))
        print(f"[lamb] fp32 reference clip={clip} correct_bias={cb}: worst err/tol {r}")
        for k, v in r.items():
            top[k] = max(top.get(k, 0.0), v)
        for name in ("zero_weights", "zero_update", "no_adapt"):
            assert norms[seg_index(name), 2].item() == 1.0, name
        for k in ("p", "m", "v"):
            assert (st[k].numpy()[~seg_mask()] == SENT).all(), k
    assert max(top.values()) <= 0.5, top
    st = torch_state()
    for t in (3, 4, 5):
        st["g"] = torch.from_numpy(np.array(grads()[t - 1]))
        norms = ref_step(st, t, torch.tensor(CLIP))
    orc, tol = chain64()
    r = worst(ratios(to_numpy(st, norms), orc, tol))
    print(f"[lamb] fp32 reference, 3 chained steps vs 3x bound: worst err/tol {r}")
    assert max(r.values()) <= 0.5, r


def test_reference_in_float64_is_the_oracle():
    """ops.reference.lamb_step on float64 copies equals step64 to float64 rounding: both implement the contract."""
    orc = step64(state())
    st = torch_state(torch.float64)
    norms = ref_step(st, STEP, CLIP)
    r = worst(ratios(to_numpy(st, norms), orc))
    assert max(r.values()) <= 1e-6, r


@pytest.mark.parametrize("mut", MUTANTS)
def test_oracle_mutants_exceed_tolerance(mut):
    """Every mutant of the oracle puts more than half of the weights of some segment >= 10x outside the tolerance
    (some mistakes show in one segment only: ``adapt_ignored`` in the adapt=False group, ``zero_w_zero_ratio`` in
    the zero-weight segment): an implementation with that mistake cannot pass the comparison."""
    orc = step64(state())
    bad = step64(state(), mut=mut)
    r = ratios(bad, orc)
    frac, off = {}, 0
    for (name, *_), (s, n, _) in zip(SEGMENTS, layout()[0]):
        frac[name] = round(float((r["p"][off:off + n] > 10.0).mean()), 3)
        off += n
    print(f"[lamb] mutant {mut}: fraction of p > 10x tolerance per segment {frac}; worst r {r['r'].max():.3g}x, "
          f"U {r['U'].max():.3g}x, W {r['W'].max():.3g}x")
    assert max(frac.values()) > 0.5, frac


# ------------------------------------------------------------------------------------------- optimizer class
def _tiny(seed=0):
    return BertForQuestionAnswering(get_config("bert-tiny-test"), precision="fp32", seed=seed)


def _lamb(model):
    groups = optimizer_groups(list(model.named_parameters()), 0.01)
    groups[1]["adapt"] = False
    return FusedLamb(groups, model.store, lr=1e-3)


def _fill_grads(model, gen):
    for _, p in model.named_parameters():
        p.grad.copy_(torch.randn(p.shape, generator=gen))


def test_fused_lamb_cpu_state_dict_round_trip():
    """Two steps, then a state_dict round trip into a fresh optimizer: the third step is bit-identical.  The state
    layout is AdamW's, and trust_ratios() names every trainable parameter once."""
    a = _tiny()
    oa = _lamb(a)
    gen = torch.Generator().manual_seed(3)
    before = a.store.master.clone()
    for _ in range(2):
        _fill_grads(a, gen)
        oa.step(clip_coef=torch.tensor(0.5))
    assert not torch.equal(a.store.master, before)
    tr = oa.trust_ratios()
    names = [n for n, p in a.named_parameters() if p.requires_grad]
    assert sorted(tr) == sorted(names) and len(set(names)) == len(names)
    from ml_recipe_distributed_pytorch_amd.models.params import no_decay
    for n, (W, U, r) in tr.items():
        assert math.isfinite(W) and math.isfinite(U) and U > 0
        if no_decay(n):
            assert r == 1.0, n
        elif W > 0:
            assert r == pytest.approx(W / U, rel=1e-6), n
    sd = copy.deepcopy(oa.state_dict())     # the state tensors are views of the arenas: keep the step-2 values
    assert {k for st in sd["state"].values() for k in st} == {"step", "exp_avg", "exp_avg_sq"}
    assert sd["param_groups"][1]["adapt"] is False and sd["param_groups"][0]["adapt"] is True
    b = _tiny()
    b.store.master.copy_(a.store.master)
    ob = _lamb(b)
    ob.load_state_dict(sd)
    g3 = torch.Generator().manual_seed(99)
    _fill_grads(a, g3)
    b.store.grad.copy_(a.store.grad)
    oa.step(), ob.step()
    assert torch.equal(a.store.master, b.store.master)
    for name in oa.state_names:
        assert torch.equal(oa._arenas[name], ob._arenas[name]), name
    assert oa.trust_ratios() == ob.trust_ratios()
    # an AdamW optimizer loads the same checkpoint layout
    c = _tiny()
    oc = FusedAdamW(optimizer_groups(list(c.named_parameters()), 0.01), c.store, lr=1e-3)
    state_only = {"state": sd["state"], "param_groups": oc.state_dict()["param_groups"]}
    oc.load_state_dict(state_only)
    for i, p in enumerate(p for g in oc.param_groups for p in g["params"]):
        assert torch.equal(oc.state[p]["exp_avg_sq"], sd["state"][i]["exp_avg_sq"])
    assert {int(oc.state[p]["step"]) for g in oc.param_groups for p in g["params"]} == {2}


def test_init_optimizer_lamb_and_untouched_groups():
    from types import SimpleNamespace
    from ml_recipe_distributed_pytorch_amd import factories
    base = dict(lr=1e-4, weight_decay=0.01, finetune=False)
    model = _tiny()
    opt = factories.init_optimizer(SimpleNamespace(optimizer="lamb", **base), model)
    assert isinstance(opt, FusedLamb)
    assert [g["adapt"] for g in opt.param_groups] == [True, False]
    assert [g["weight_decay"] for g in opt.param_groups] == [0.01, 0.0]
    assert opt.defaults["eps"] == 1e-6 and opt.defaults["correct_bias"] is True and opt.defaults["betas"] == (0.9, 0.999)
    # adam / adamod: the groups carry exactly the keys of the class built directly, as before LAMB existed
    def direct(name, m):
        groups = optimizer_groups(list(m.named_parameters()), 0.01)
        if name == "adam":
            return FusedAdamW(groups, m.store, lr=1e-4, eps=1e-6, correct_bias=False)
        return FusedAdaMod(groups, m.store, lr=1e-4)

    own = {"adam": {"params", "lr", "betas", "eps", "weight_decay", "correct_bias"},
           "adamod": {"params", "lr", "betas", "beta3", "eps", "weight_decay"}}
    for name in ("adam", "adamod"):
        o = factories.init_optimizer(SimpleNamespace(optimizer=name, **base), _tiny())
        d = direct(name, _tiny())
        assert type(o) is type(d) and len(o.param_groups) == 2
        for g, dg in zip(o.param_groups, d.param_groups):
            assert set(g) == set(dg) and own[name] <= set(g) and "adapt" not in g, (name, set(g) ^ set(dg))
            assert {k: v for k, v in g.items() if k != "params"} == {k: v for k, v in dg.items() if k != "params"}


# ------------------------------------------------------------------------------------------------------- CLI
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = os.path.join(ROOT, "config", "test_bert.cfg")
TINY = ["--model", "bert-tiny-test", "--max_seq_len", "48", "--max_question_len", "8", "--n_jobs", "0",
        "--test_batch_size", "8"]


def _train(argv):
    from ml_recipe_distributed_pytorch_amd.cli.train import main
    main(argv)


def test_train_debug_smoke_lamb(tmp_path):
    """modules/train.py ... --optimizer lamb --debug on the dummy dataset: trains on the CPU and logs the trust
    ratios next to the loss."""
    _train(["-c", BASE, "--dump_dir", str(tmp_path), "--train_batch_size", "8", "--batch_split", "2",
            "--dummy_dataset_len", "32", "--optimizer", "lamb"] + TINY)
    exp = tmp_path / "test"
    assert (exp / "trainer.cfg").exists() and "lamb" in (exp / "trainer.cfg").read_text()
    ev = list((tmp_path / "board" / "test").glob("events.out.tfevents.*"))
    assert ev
    from ml_recipe_distributed_pytorch_amd.utils.tb import read_events
    events = list(read_events(str(ev[0])))
    tags = {t for _, t, _ in events}
    assert {"train/loss", "train/lr", "test/loss", "opt/trust_ratio_min", "opt/trust_ratio_median",
            "opt/trust_ratio_max"} <= tags
    by = {t: v for _, t, v in events if t.startswith("opt/")}
    assert 0 < by["opt/trust_ratio_min"] <= by["opt/trust_ratio_median"] <= by["opt/trust_ratio_max"]


def test_train_resume_lamb(tmp_path):
    """One epoch with --optimizer lamb, then a resume from last.ch into a second epoch with the restored state."""
    def cfg(n_epochs):
        lines = []
        over = dict(debug="False", n_epochs=str(n_epochs), train_batch_size="8", batch_split="1",
                    dummy_dataset_len="32", experiment_name="lamb", drop_optimizer="False", optimizer="lamb")
        for line in open(BASE).read().splitlines():
            key = line.split("=")[0].strip()
            if key in over:
                line = f"{key} = {over.pop(key)}"
            lines.append(line)
        lines += [f"{k} = {v}" for k, v in over.items()]
        path = tmp_path / f"run{n_epochs}.cfg"
        path.write_text("\n".join(lines) + "\n")
        return str(path)

    _train(["-c", cfg(1), "--dump_dir", str(tmp_path)] + TINY)
    exp = tmp_path / "lamb"
    st = torch.load(exp / "last.ch", weights_only=True)
    assert st["global_step"] == 4 and st["epoch"] == 1
    state0 = st["optimizer"]["state"][0]
    assert set(state0) == {"step", "exp_avg", "exp_avg_sq"} and int(state0["step"]) == 4
    assert [g["adapt"] for g in st["optimizer"]["param_groups"]] == [True, False]
    _train(["-c", cfg(2), "--dump_dir", str(tmp_path), "--last", str(exp / "last.ch")] + TINY)
    st2 = torch.load(exp / "last.ch", weights_only=True)
    assert st2["global_step"] == 8 and st2["epoch"] == 2
    assert int(st2["optimizer"]["state"][0]["step"]) == 8
    assert not torch.equal(st2["optimizer"]["state"][0]["exp_avg"], state0["exp_avg"])
