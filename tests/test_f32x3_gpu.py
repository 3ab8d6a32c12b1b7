"""The fp32 mode's opt-in ``bf16x3`` projection GEMM on the GPU (``gemm_f32x3_kernel``): against fp64 products
within the split's error bound, against the op-for-op oracle ``ops.reference.matmul_bf16x3`` to accumulation
rounding, memory safety / determinism / non-finite propagation, and BERT-tiny fp32 with the mode on against the CPU
path (which then runs the oracle)."""
import copy

import pytest
import torch

from ml_recipe_distributed_pytorch_amd.models.bert import BertForQuestionAnswering
from ml_recipe_distributed_pytorch_amd.models.config import get_config
from ml_recipe_distributed_pytorch_amd.ops import f32
from ml_recipe_distributed_pytorch_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -14   # of |alpha|·(|A|·|B|ᵀ): 4/3 of the provable 3·2⁻¹⁶
EPI = 2.0 ** -22     # of |bias| + |R| + |result|: the fp32 epilogue
# (M, N, K): one partial tile with K below a stage · every tail, K no stage multiple · exact tiles · split-K
SHAPES = [(4, 4, 4), (200, 132, 68), (128, 256, 64), (36, 128, 4096)]
# BERT-tiny fp32 on the CPU, bf16x3 against exact (tests/test_f32x3_cpu.py, docs/PARITY.md C07): outputs, gradients
CPU_DEVIATION = (7.3e-7, 1.6e-5)


@pytest.fixture(autouse=True)
def _restore_mode():
    prev = f32.MATMUL
    yield
    f32.MATMUL = prev


def _k():
    from ml_recipe_distributed_pytorch_amd._native import kernels
    return kernels()


def _operands(M, N, K, cuda, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, K, generator=g).to(cuda), torch.randn(N, K, generator=g).to(cuda)


def _launch(layout, a, b, c, mode="bf16x3", ldc=None, **kw):
    """C[M, N] = alpha·a[M, K]·b[N, K]ᵀ … with the operands stored as the step's three GEMMs store them:
    forward (both k-contiguous), dgrad (B j-contiguous: stored [K, N]), wgrad (both i/j-contiguous: [K, M], [K, N])."""
    M, K = a.shape
    N = b.shape[0]
    ldc = N if ldc is None else ldc
    if layout == "forward":
        A, sa, B, sb = a.contiguous(), [K, 1, 0, 0], b.contiguous(), [K, 1, 0, 0]
    elif layout == "dgrad":
        A, sa, B, sb = a.contiguous(), [K, 1, 0, 0], b.t().contiguous(), [1, N, 0, 0]
    else:
        A, sa, B, sb = a.t().contiguous(), [1, M, 0, 0], b.t().contiguous(), [1, N, 0, 0]
    _k().gemm_f32(A, B, c, M, N, K, sa, sb, [ldc, 0, 0], mode=mode, **kw)
    return c


def _check_bound(got, a, b, alpha=1.0, bias=None, R=None):
    exact = alpha * (a.double() @ b.double().t())
    allow = abs(alpha) * BOUND * (a.double().abs() @ b.double().abs().t())
    epi = torch.zeros_like(exact)
    if bias is not None:
        exact, epi = exact + bias.double(), epi + bias.double().abs()
    if R is not None:
        exact, epi = exact + R.double(), epi + R.double().abs()
    allow = allow + EPI * (epi + exact.abs())
    err = (got.double() - exact).abs()
    worst = float((err / allow).max())
    print(f"  max err / allowed = {worst:.3f}")
    assert worst <= 1.0
    return worst


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_x3_layouts_against_fp64(cuda, M, N, K):
    a, b = _operands(M, N, K, cuda)
    g = torch.Generator().manual_seed(1)
    bias, r = torch.randn(N, generator=g).to(cuda), torch.randn(M, N, generator=g).to(cuda)
    # forward: bias + residual epilogue, alpha != 1
    y = _launch("forward", a, b, torch.empty(M, N, device=cuda), alpha=0.375, bias=bias, R=r, ldr=N)
    _check_bound(y, a, b, alpha=0.375, bias=bias, R=r)
    # dgrad: plain, and with the residual
    _check_bound(_launch("dgrad", a, b, torch.empty(M, N, device=cuda)), a, b)
    _check_bound(_launch("dgrad", a, b, torch.empty(M, N, device=cuda), R=r, ldr=N), a, b, R=r)
    # weight gradient accumulating onto a prior value: R aliases C
    dw = torch.randn(M, N, generator=g).to(cuda)
    dw0 = dw.clone()
    _launch("wgrad", a, b, dw, R=dw, ldr=N)
    _check_bound(dw, a, b, R=dw0)


def _ratio(got, want64, a, b):
    return float(((got.double() - want64).abs() / (a.double().abs() @ b.double().abs().t())).max())


# the ratio is a maximum over the output: the 16 elements of (4, 4, 4) leave it to chance, so that shape is left
# to the bound test above
@pytest.mark.parametrize("M,N,K", SHAPES[1:])
@pytest.mark.parametrize("layout", ["forward", "dgrad", "wgrad"])
def test_x3_against_oracle(cuda, layout, M, N, K):
    """Against the same split and the same three products in fp64 only the fp32 accumulation is left: within 4× of
    what the exact kernel's accumulation shows against fp64 on these inputs."""
    a, b = _operands(M, N, K, cuda, seed=2)
    got = _launch(layout, a, b, torch.empty(M, N, device=cuda))
    exact = _launch(layout, a, b, torch.empty(M, N, device=cuda), mode="exact")
    r_exact = _ratio(exact, a.double() @ b.double().t(), a, b)
    r_x3 = _ratio(got, ref.matmul_bf16x3(a.double(), b.double()), a, b)
    print(f"  {layout} {(M, N, K)}: exact kernel {r_exact:.3e}, bf16x3 kernel vs its oracle {r_x3:.3e}")
    assert r_x3 <= 4 * r_exact


def test_truncating_split_is_told_apart(cuda):
    """A kernel that truncated instead of rounding would match this mutant oracle; the real one must not."""
    M, N, K = 128, 256, 64
    a, b = _operands(M, N, K, cuda, seed=2)
    got = _launch("forward", a, b, torch.empty(M, N, device=cuda))
    exact = _launch("forward", a, b, torch.empty(M, N, device=cuda), mode="exact")
    r_exact = _ratio(exact, a.double() @ b.double().t(), a, b)

    def trunc_split(x):
        hi = (x.view(torch.int32) & -65536).view(torch.float32)
        mid = ((x - hi).view(torch.int32) & -65536).view(torch.float32)
        return hi.double(), mid.double()

    (ah, am), (bh, bm) = trunc_split(a), trunc_split(b)
    mutant = (am @ bh.t() + ah @ bm.t()) + ah @ bh.t()
    r_mut = _ratio(got, mutant, a, b)
    print(f"  truncating-split oracle: {r_mut:.3e} (allowance {4 * r_exact:.3e})")
    assert r_mut > 4 * r_exact


def test_x3_batched_attention_layout(cuda):
    """The two-level batch (b, h) over qkv [B·L, 3H] views: S = scale·Q·Kᵀ, in the new mode."""
    B, L, nh, dh = 3, 96, 4, 32
    H = nh * dh
    qkv = torch.randn(B * L, 3 * H, device=cuda)
    s = torch.empty(B, nh, L, L, device=cuda)
    _k().gemm_f32(qkv, qkv[:, H:], s, L, L, dh, [3 * H, 1, L * 3 * H, dh], [3 * H, 1, L * 3 * H, dh],
                  [L, nh * L * L, L * L], batch=B * nh, nb_in=nh, alpha=0.125, mode="bf16x3")
    t = qkv.double().view(B, L, 3, nh, dh).permute(2, 0, 3, 1, 4)
    exact = 0.125 * t[0] @ t[1].transpose(-1, -2)
    allow = 0.125 * BOUND * (t[0].abs() @ t[1].abs().transpose(-1, -2)) + EPI * exact.abs()
    assert bool(((s.double() - exact).abs() <= allow).all())
    assert not torch.equal(s, torch.zeros_like(s))


@pytest.mark.parametrize("M,N,K", [(200, 132, 68), (36, 128, 4096)])
@pytest.mark.parametrize("layout", ["forward", "wgrad"])
def test_x3_writes_only_the_output(cuda, layout, M, N, K):
    a, b = _operands(M, N, K, cuda, seed=3)
    ldc = N + 8
    buf = torch.full((M + 3, ldc), 777.0, device=cuda)
    _launch(layout, a, b, buf, ldc=ldc)
    assert bool((buf[:, N:] == 777.0).all()) and bool((buf[M:] == 777.0).all())
    _check_bound(buf[:M, :N], a, b)


@pytest.mark.parametrize("M,N,K", [(200, 132, 68), (36, 128, 4096)])
def test_x3_is_bitwise_repeatable(cuda, M, N, K):
    a, b = _operands(M, N, K, cuda, seed=4)
    for layout in ("forward", "dgrad", "wgrad"):
        c1 = _launch(layout, a, b, torch.empty(M, N, device=cuda))
        c2 = _launch(layout, a, b, torch.empty(M, N, device=cuda))
        assert torch.equal(c1, c2), layout


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_x3_non_finite_inputs_propagate(cuda, bad):
    M, N, K = 200, 132, 68
    a, b = _operands(M, N, K, cuda, seed=5)
    a[3, 5] = bad
    b[7, 66] = bad
    for layout in ("forward", "wgrad"):
        c = _launch(layout, a, b, torch.empty(M, N, device=cuda))
        fin = torch.isfinite(c)
        assert not bool(fin[3].any()) and not bool(fin[:, 7].any()), layout
        rest = torch.ones_like(fin)
        rest[3], rest[:, 7] = False, False
        assert bool(fin[rest].all()), layout


def test_x3_rejects_out_of_bounds_view_and_bad_mode(cuda):
    a = torch.randn(64, 64, device=cuda)
    c = torch.empty(64, 64, device=cuda)
    with pytest.raises(RuntimeError, match="exceeds"):
        _k().gemm_f32(a, a, c, 128, 64, 64, [64, 1, 0, 0], [64, 1, 0, 0], [64, 0, 0], mode="bf16x3")
    with pytest.raises(RuntimeError, match="mode"):
        _k().gemm_f32(a, a, c, 64, 64, 64, [64, 1, 0, 0], [64, 1, 0, 0], [64, 0, 0], mode="tf32")


def test_old_signature_is_exact_mode(cuda):
    M, N, K = 200, 132, 68
    a, b = _operands(M, N, K, cuda, seed=6)
    bias = torch.randn(N, device=cuda)
    old = torch.empty(M, N, device=cuda)
    _k().gemm_f32(a, b, old, M, N, K, [K, 1, 0, 0], [K, 1, 0, 0], [N, 0, 0], 1, 1, 0.5, bias, None, 0)
    new = _launch("forward", a, b, torch.empty(M, N, device=cuda), mode="exact", alpha=0.5, bias=bias)
    x3 = _launch("forward", a, b, torch.empty(M, N, device=cuda), mode="bf16x3", alpha=0.5, bias=bias)
    assert torch.equal(old, new) and not torch.equal(old, x3)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


@pytest.mark.parametrize("train", [False, True])
def test_x3_model_gpu_matches_cpu(cuda, train):
    """BERT-tiny fp32 with the mode on: the GPU kernels against the CPU path, whose linears now run the oracle —
    the bounds of the exact mode's test, since the two sides again differ in summation order only."""
    f32.set_matmul("bf16x3")
    cfg = get_config("bert-tiny-test")
    cpu = BertForQuestionAnswering(cfg, seed=0, precision="fp32")
    gpu = copy.deepcopy(cpu).to(cuda)
    cpu.train(train)
    gpu.train(train)
    g = torch.Generator().manual_seed(5)
    B, L = 3, 64
    ids = torch.randint(1, cfg.vocab_size, (B, L), generator=g)
    ids[1, L - 5:] = 0
    tt = torch.zeros_like(ids)
    tt[:, L // 3:] = 1
    mask = ids > 0
    torch.manual_seed(11)
    oc = cpu(ids, mask, tt)
    torch.manual_seed(11)
    og = gpu(ids.to(cuda), mask.to(cuda), tt.to(cuda))
    for k in oc:
        assert og[k].dtype == torch.float32
        assert _rel(og[k].cpu(), oc[k]) < 1e-4, k
    cpu.zero_grad()
    gpu.zero_grad()
    sum(v.sum() for v in oc.values()).backward()
    sum(v.sum() for v in og.values()).backward()
    gmax = max(float(p.grad.abs().max()) for p in cpu.parameters())
    for (n, pc), (_, pg) in zip(cpu.named_parameters(), gpu.named_parameters()):
        err = float((pg.grad.cpu().double() - pc.grad.double()).abs().max())
        assert err <= 1e-3 * float(pc.grad.abs().max()) + 1e-6 * gmax, (n, err)


def test_x3_train_steps_gpu(cuda):
    from types import SimpleNamespace
    from ml_recipe_distributed_pytorch_amd.data.dummy import SpecialIds, synth_batch_native
    from ml_recipe_distributed_pytorch_amd.models.losses import build_loss
    from ml_recipe_distributed_pytorch_amd.train.engine import TrainEngine, to_device
    from ml_recipe_distributed_pytorch_amd.train.optim import FusedAdamW
    from ml_recipe_distributed_pytorch_amd.train.trainer import optimizer_groups
    f32.set_matmul("bf16x3")
    cfg = get_config("bert-tiny-test")
    lp = SimpleNamespace(loss="smooth", smooth_alpha=0.01, w_start=1, w_end=1, w_start_reg=1, w_end_reg=1, w_cls=1)
    batch = synth_batch_native(8, 64, 16, SpecialIds(vocab_size=cfg.vocab_size), seed=0)
    losses = {}
    for dev in ("cpu", cuda):
        m = BertForQuestionAnswering(cfg, seed=0, precision="fp32").to(dev).eval()
        opt = FusedAdamW(optimizer_groups(m.named_parameters(), 1e-4), m.store, lr=1e-3, correct_bias=False,
                         zero_grad_fn=m.zero_grad)
        eng = TrainEngine(m, build_loss(lp), opt)
        inputs, labels = to_device(batch[0], dev), to_device(batch[1], dev)
        losses[str(dev)] = [eng.step([(inputs, labels)]).losses.to_floats()["loss"] for _ in range(4)]
    lc, lg = losses["cpu"], losses[str(cuda)]
    assert all(v == v for v in lg) and lg[-1] < lg[0], lg
    for a, b in zip(lg, lc):
        assert abs(a - b) <= 1e-3 * (1 + abs(b)), (lg, lc)


def test_x3_differs_from_exact_within_cpu_measured_cost(cuda):
    """One process, both modes on the GPU: the outputs and gradients differ, by no more than 4× the deviation the
    CPU path measured between the modes on the same model and inputs."""
    from test_f32x3_cpu import model_deviation
    d_out, d_grad = model_deviation(cuda)
    print(f"  bert-tiny fp32 GPU, bf16x3 vs exact: outputs {d_out:.3e}, gradients {d_grad:.3e}")
    assert 0 < d_out <= 4 * CPU_DEVIATION[0]
    assert 0 < d_grad <= 4 * CPU_DEVIATION[1]
