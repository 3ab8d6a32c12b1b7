"""The LAMB kernels (csrc/kernels/optim.hip: lamb_moments_kernel, lamb_ratio_kernel, lamb_apply_kernel) and
FusedLamb on the GPU, against the float64 oracle, layout and tolerance of tests/test_lamb_cpu.py (its module
docstring derives every bound; none of them is fitted to what the kernels give)."""
import numpy as np
import pytest
import torch

import test_lamb_cpu as L
from ml_recipe_distributed_pytorch_amd import _native
from ml_recipe_distributed_pytorch_amd.models.bert import BertForQuestionAnswering
from ml_recipe_distributed_pytorch_amd.models.config import get_config
from ml_recipe_distributed_pytorch_amd.train.optim import CHUNK, FusedLamb, get_linear_schedule_with_warmup
from ml_recipe_distributed_pytorch_amd.train.trainer import optimizer_groups

STATE = ("p", "m", "v")


def _bc(step, correct_bias):
    if not correct_bias:
        return 1.0, 1.0
    return 1.0 / (1.0 - L.B1 ** step), 1.0 / (1.0 - L.B2 ** step)


class _Arena:
    """The layout's state on the device with a plan and scratch; ``step`` is one lamb_step launch triple."""

    def __init__(self, cuda, with_compute=True):
        self.k = _native.kernels()
        self.d = {name: torch.from_numpy(np.array(t)).to(cuda) for name, t in L.state().items()}
        n = self.d["p"].numel()
        self.comp = torch.full((n,), L.SENT, dtype=torch.bfloat16, device=cuda) if with_compute else None
        chunks, first = L.chunk_tables()
        self.plan = self.k.lamb_plan(self.d["p"], chunks, first)
        self.partials = torch.full((chunks.shape[0], 2), -1.0, device=cuda)
        self.norms = torch.full((len(first) - 1, 3), -1.0, device=cuda)

    def args(self, step, correct_bias):
        return (L.LR, L.WD, L.ADAPT, L.B1, L.B2, L.EPS) + _bc(step, correct_bias)

    def step(self, step=L.STEP, clip=None, correct_bias=True):
        d = self.d
        self.k.lamb_step(self.plan, d["p"], self.comp, d["g"], d["m"], d["v"], *self.args(step, correct_bias), clip,
                         self.partials, self.norms)

    def host(self):
        torch.cuda.synchronize()
        out = {name: t.cpu().numpy() for name, t in self.d.items()}
        out["norms"] = self.norms.cpu().numpy()
        return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check_exact_parts(got, comp, first_step=True):
    """What holds bit for bit: padding, the rule-given ratios, the bf16 copy.  The zero-weight segment has W = 0 in
    its first step only (that step moves it)."""
    st, mask = L.state(), L.seg_mask()
    for name in STATE:
        assert np.array_equal(_bits(got[name][~mask]), _bits(st[name][~mask])), f"{name}: padding"
    for name in ("zero_update", "no_adapt") + (("zero_weights",) if first_step else ()):
        assert got["norms"][L.seg_index(name), 2] == 1.0, name
    assert got["norms"][L.seg_index("zero_update"), 1] == 0.0
    assert (got["norms"][L.seg_index("zero_weights"), 0] == 0.0) == first_step
    if comp is not None:
        c = comp.cpu()
        m = torch.from_numpy(mask)
        assert torch.equal(c[~m].view(torch.int16), torch.full_like(c[~m], L.SENT).view(torch.int16)), "bf16 padding"
        assert torch.equal(c[m].view(torch.int16), torch.from_numpy(got["p"])[m].bfloat16().view(torch.int16)), "bf16 copy"


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.gpu
def test_moments_sum_p2_partials_exact(cuda):
    """Σp² per chunk, exactly, on power-of-two weights (the construction of test_sq_norm_chunks_exact): all ones
    gives the chunk's numel (a dropped or doubled element shows as ±1), and a single 4.0 among zeros at the first /
    last element, around every 1024-float pass of the float4 loop and around the two-quartet seam gives 16.0.
    The padding holds 64.0, so an over-read changes a partial.  Also Σu² = wd²·Σp² where g = m = v = 0."""
    k = _native.kernels()
    segs, N = L.layout()
    chunks, first = L.chunk_tables()
    rows = [(int(s), int(w) & 0xFFFFFFFF, int(w) >> 32) for s, w in chunks.tolist()]
    inside = torch.from_numpy(L.seg_mask()).to(cuda)
    zeros = torch.zeros(N, device=cuda)
    plan = k.lamb_plan(zeros, chunks, first)
    C = len(rows)
    assert plan.nchunks == C and plan.nseg == len(segs) and plan.ngroups == 3
    assert plan.chunk_seg.cpu().tolist() == [i for i, (s, n, g) in enumerate(segs) for _ in range(0, n, CHUNK)]
    norms = torch.zeros(len(segs), 3, device=cuda)
    wd = [0.5, 0.0, 2.0]    # powers of two: u = wd·p and its square are exact

    def run(p):
        m, v = torch.zeros(N, device=cuda), torch.zeros(N, device=cuda)
        part = torch.full((C, 2), -1.0, device=cuda)
        k.lamb_moments(plan, p, zeros, m, v, L.LR, wd, L.ADAPT, L.B1, L.B2, L.EPS, 1.0, 1.0, None, part, norms)
        assert not m.any() and not v.any()
        return part.cpu()

    part = run(torch.where(inside, 1.0, 64.0))
    assert part[:, 0].tolist() == [float(n) for _, n, _ in rows]
    assert part[:, 1].tolist() == [float(n) * wd[g] ** 2 for _, n, g in rows]
    pos = []
    for s, n, _ in rows:
        cand = [0, n - 1, 3, n - 4, n - n % 4 - 1, n - n % 4]
        for b in (1024, 2048, 3072, 4096, 5120, 7168):
            cand += [b - 1, b]
        pos.append(sorted({c for c in cand if 0 <= c < n}))
    for r in range(max(len(p) for p in pos)):
        p = torch.where(inside, 0.0, 64.0)
        want = []
        for (s, n, _), ps in zip(rows, pos):
            if r < len(ps):
                p[s + ps[r]] = 4.0
            want.append(16.0 if r < len(ps) else 0.0)
        part = run(p)
        assert part[:, 0].tolist() == want, r
        assert part[:, 1].tolist() == [w * wd[g] ** 2 for w, (_, _, g) in zip(want, rows)], r


@pytest.mark.gpu
@pytest.mark.parametrize("correct_bias", [True, False], ids=["step3", "nobias"])
@pytest.mark.parametrize("with_compute", [True, False], ids=["bf16copy", "nocopy"])
@pytest.mark.parametrize("with_clip", [True, False], ids=["clip", "noclip"])
def test_lamb_step_vs_float64(cuda, with_clip, with_compute, correct_bias):
    """The three launches, one step at t = 3, against the float64 oracle: m, v within K·2⁻²⁴ of their terms; W, U, r
    within the bounds derived in tests/test_lamb_cpu.py from the summation order documented in optim.hip
    (D_s = 32 + 6 + 3 per chunk + ceil(chunks/64) + 6 per segment; W: D_s·u, U: (κ_s·K + D_s)·u,
    r: (κ_s·K + 2·D_s + 1)·u, relative); p within K·u·(|p| + |lr·r·u|) + |lr·r·u|·(relative bound of r).
    The ratios that a rule sets to 1 are exactly 1; padding, gradient and bf16 copy are exact statements.

    Measured on an MI355X, worst err / bound over the eight cases (1.0 allowed):
        p 0.144   m 0.173   v 0.287   W 0.019   U 0.031   r 0.026
    (the fp32 CPU reference: p 0.130, m 0.124, v 0.251, W 0.019, U 0.031, r 0.026)."""
    a = _Arena(cuda, with_compute)
    clip = torch.tensor([L.CLIP], device=cuda) if with_clip else None
    a.step(clip=clip, correct_bias=correct_bias)
    got = a.host()
    assert np.array_equal(_bits(got["g"]), _bits(L.state()["g"])), "the gradient arena was written"
    _check_exact_parts(got, a.comp)
    orc = L.step64(L.state(), clip=L.CLIP if with_clip else None, correct_bias=correct_bias)
    r = L.ratios(got, orc)
    print(f"[lamb] kernels clip={with_clip} compute={with_compute} correct_bias={correct_bias}: "
          f"worst err/tol {L.worst(r)}")
    for name, val in r.items():
        assert val.max() <= 1.0, f"{name}: {(val > 1).sum()} outside, worst {val.max():.2f}x"
    # lr·r·u moved every weight that had an update
    s, n, _ = L.layout()[0][L.seg_index("zero_update")]
    assert np.array_equal(_bits(got["p"][s:s + n]), _bits(L.state()["p"][s:s + n]))


@pytest.mark.gpu
def test_lamb_three_chained_steps(cuda):
    """Steps 3, 4, 5 stay finite and within 3x the chain's single-step bound (test_lamb_cpu.chain64).
    Measured on an MI355X, worst err / bound: p 0.053, m 0.068, v 0.100, W 0.010, U 0.010, r 0.007."""
    a = _Arena(cuda)
    clip = torch.tensor([L.CLIP], device=cuda)
    for t in (3, 4, 5):
        a.d["g"] = torch.from_numpy(np.array(L.grads()[t - 1])).to(cuda)
        a.step(step=t, clip=clip)
    got = a.host()
    orc, tol = L.chain64()
    r = L.ratios(got, orc, tol)
    print(f"[lamb] kernels, 3 chained steps vs 3x bound: worst err/tol {L.worst(r)}")
    for name, val in r.items():
        assert val.max() <= 1.0, f"{name}: worst {val.max():.2f}x"
    _check_exact_parts(got, a.comp, first_step=False)


@pytest.mark.gpu
def test_bf16_copy_and_gradient_bits(cuda):
    """The bf16 copy is master.to(bfloat16) bit for bit over the whole arena region the step owns, and the gradient
    arena keeps every bit (bench.py --dump-outputs, the reducer's snapshot and the replica check read it later)."""
    a = _Arena(cuda)
    g0 = a.d["g"].clone()
    a.step(clip=torch.tensor([L.CLIP], device=cuda))
    torch.cuda.synchronize()
    assert torch.equal(a.d["g"].view(torch.int32), g0.view(torch.int32))
    m = torch.from_numpy(L.seg_mask()).to(cuda)
    assert torch.equal(a.comp[m].view(torch.int16), a.d["p"].to(torch.bfloat16)[m].view(torch.int16))
    assert (a.comp[~m] == L.SENT).all()
    assert not torch.equal(a.d["p"][m], torch.from_numpy(np.array(L.state()["p"])).to(cuda)[m])


@pytest.mark.gpu
def test_lamb_step_is_deterministic(cuda):
    """The same step from cloned state twice, and once as three separate phase launches: p, m, v, the partials and
    the ratios are bit-identical (fixed summation order, no atomics)."""
    clip = torch.tensor([L.CLIP], device=cuda)
    runs = []
    for phases in (False, False, True):
        a = _Arena(cuda)
        if phases:
            d, args = a.d, a.args(L.STEP, True)
            a.k.lamb_moments(a.plan, d["p"], d["g"], d["m"], d["v"], *args, clip, a.partials, a.norms)
            a.k.lamb_ratio(a.plan, L.LR, L.WD, L.ADAPT, a.partials, a.norms)
            a.k.lamb_apply(a.plan, d["p"], a.comp, d["m"], d["v"], *args, a.partials, a.norms)
        else:
            a.step(clip=clip)
        torch.cuda.synchronize()
        runs.append({**{n: a.d[n].clone() for n in STATE}, "partials": a.partials.clone(), "norms": a.norms.clone(),
                     "comp": a.comp.clone().view(torch.int16)})
    for other in runs[1:]:
        for name, t in runs[0].items():
            assert torch.equal(t.view(torch.int32) if t.dtype == torch.float32 else t,
                               other[name].view(torch.int32) if t.dtype == torch.float32 else other[name]), name
    assert (runs[0]["partials"] >= 0).all() and (runs[0]["norms"] >= 0).all()    # every slot was written


@pytest.mark.gpu
def test_bindings_reject_bad_arguments(cuda):
    """Bad tables are refused where the plan is made, bad arenas where the step is called; nothing is launched."""
    k = _native.kernels()
    a = _Arena(cuda)
    before = {name: t.clone() for name, t in a.d.items()}
    chunks, first = L.chunk_tables()
    p, N = a.d["p"], a.d["p"].numel()
    # tables
    past = chunks.clone()
    past[-1, 0] = N - 2
    with pytest.raises(RuntimeError, match="outside the arena"):
        k.lamb_plan(p, past, first)
    grp = chunks.clone()
    grp[3, 1] = (grp[3, 1] & 0xFFFFFFFF) | (8 << 32)
    with pytest.raises(RuntimeError, match="group index"):
        k.lamb_plan(p, grp, first)
    bad_first = first.clone()
    bad_first[-1] -= 1
    with pytest.raises(RuntimeError, match="does not match the chunk table"):
        k.lamb_plan(p, chunks, bad_first)
    shifted = first.clone()
    shifted[2] += 1          # segment 1 would swallow the first chunk of segment 2: not contiguous with it
    with pytest.raises(RuntimeError, match="does not match the chunk table"):
        k.lamb_plan(p, chunks, shifted)
    with pytest.raises(RuntimeError, match="int32"):
        k.lamb_plan(p, chunks, first.long())
    with pytest.raises(RuntimeError, match=r"\[n,2\]"):
        k.lamb_plan(p, torch.zeros(chunks.shape[0], 3, dtype=torch.int64), first)
    # arenas and scratch
    d, args = a.d, a.args(L.STEP, True)
    with pytest.raises(RuntimeError, match="dtype"):
        k.lamb_step(a.plan, d["p"], a.comp, d["g"].double(), d["m"], d["v"], *args, None, a.partials, a.norms)
    with pytest.raises(RuntimeError, match="dtype"):
        k.lamb_step(a.plan, d["p"], a.comp.float(), d["g"], d["m"], d["v"], *args, None, a.partials, a.norms)
    with pytest.raises(RuntimeError, match="the plan was made for"):
        k.lamb_step(a.plan, d["p"], a.comp, d["g"], d["m"][:-4], d["v"], *args, None, a.partials, a.norms)
    with pytest.raises(RuntimeError, match="partials"):
        k.lamb_step(a.plan, d["p"], a.comp, d["g"], d["m"], d["v"], *args, None, a.partials[:-1], a.norms)
    with pytest.raises(RuntimeError, match="groups"):
        k.lamb_step(a.plan, d["p"], a.comp, d["g"], d["m"], d["v"], L.LR[:2], L.WD[:2], L.ADAPT[:2], *args[3:], None,
                    a.partials, a.norms)
    with pytest.raises(RuntimeError, match="groups"):
        k.lamb_step(a.plan, d["p"], a.comp, d["g"], d["m"], d["v"], [0.1] * 9, [0.0] * 9, [True] * 9, *args[3:], None,
                    a.partials, a.norms)
    torch.cuda.synchronize()
    for name in d:
        assert torch.equal(d[name], before[name]), name
    assert (a.partials == -1).all() and (a.norms == -1).all() and (a.comp == L.SENT).all()


# --------------------------------------------------------------------------------------- the optimizer class
def _make(model):
    groups = optimizer_groups(list(model.named_parameters()), 0.01)
    groups[1]["adapt"] = False
    return FusedLamb(groups, model.store, lr=1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_fused_lamb_gpu_matches_cpu(cuda, precision):
    """FusedLamb on bert-tiny-test (bf16 store, and the fp32 store whose compute arena IS the master): two steps
    under a warm-up schedule against the same class on a CPU copy fed identical gradients — the comparison of
    test_optim_gpu.py::test_optimizer_class_gpu_matches_cpu — plus the trust ratios and the state_dict."""
    cfg = get_config("bert-tiny-test")
    gm = BertForQuestionAnswering(cfg, precision=precision, seed=0).to(cuda)
    cm = BertForQuestionAnswering(cfg, precision="fp32", seed=0)
    assert torch.equal(gm.store.master.cpu(), cm.store.master)
    assert (gm.store.compute.data_ptr() == gm.store.master.data_ptr()) == (precision == "fp32")
    go, co = _make(gm), _make(cm)
    gs, cs = get_linear_schedule_with_warmup(go, 4, 10), get_linear_schedule_with_warmup(co, 4, 10)
    go.step(), co.step(), gs.step(), cs.step()   # the schedule starts at lr 0
    gen = torch.Generator().manual_seed(11)
    for _ in range(2):
        for (_, gp), (_, cp) in zip(gm.named_parameters(), cm.named_parameters()):
            g = torch.randn(cp.shape, generator=gen)
            cp.grad.copy_(g)
            gp.grad.copy_(g)
        assert go.param_groups[0]["lr"] == co.param_groups[0]["lr"] > 0
        grad_before = gm.store.grad.clone()
        go.step(), co.step(), gs.step(), cs.step()
        assert torch.equal(gm.store.grad, grad_before)
    torch.cuda.synchronize()
    for (name, gp), (_, cp) in zip(gm.named_parameters(), cm.named_parameters()):
        torch.testing.assert_close(gp.detach().cpu(), cp.detach(), atol=1e-6, rtol=1e-5, msg=name)
    for name in go.state_names:
        torch.testing.assert_close(go._arenas[name].cpu(), co._arenas[name], atol=1e-6, rtol=1e-5, msg=name)
    gt, ct = go.trust_ratios(), co.trust_ratios()
    assert list(gt) == list(ct) and len(gt) == len(list(gm.named_parameters()))
    for name in gt:
        assert gt[name] == pytest.approx(ct[name], rel=1e-5), name
    assert len({round(v[2], 4) for v in gt.values()}) > 3    # the ratios are per parameter
    if precision == "bf16":
        master, compute = gm.store.master.cpu(), gm.store.compute.cpu()
        for s, n, name in gm.store.segments():
            assert torch.equal(compute[s:s + n].view(torch.int16), master[s:s + n].bfloat16().view(torch.int16)), name
    fresh = BertForQuestionAnswering(cfg, precision="fp32", seed=0)
    fo = _make(fresh)
    fo.load_state_dict(go.state_dict())
    for name in go.state_names:
        assert torch.equal(fo._arenas[name], go._arenas[name].cpu()) and not fo._arenas[name].is_cuda, name
    assert {int(fo.state[p]["step"]) for g in fo.param_groups for p in g["params"]} == {3}
