"""The atomic-free embedding backward behind ``ops.deterministic()``: the fp32 kernels' sorted-run path for the word,
position and (> 2 types) type tables, and the bf16 kernels' deterministic-positions / sorted-type modes.

Every table row is summed in a documented order (stated above embed.hip embed_word_kernel; the fp32 pair of kernels
is f32_embed.hip f32_embed_run_kernel): tokens sorted stably by the table's
key, the sorted list cut into chunks of ``embed_run_chunk()`` positions; the rows
of one key inside one chunk (a piece) are summed from zero in token order, the pieces of a run that crosses chunks are
added in chunk order, and accumulate adds the existing row last.  The tests check that order bit for bit, the values
against the fp32 oracle, run-to-run equality, and whole training steps."""
import copy
from types import SimpleNamespace

import pytest
import torch

from ml_recipe_distributed_pytorch_amd import _native
from ml_recipe_distributed_pytorch_amd.models.bert import BertForQuestionAnswering
from ml_recipe_distributed_pytorch_amd.models.config import get_config
from ml_recipe_distributed_pytorch_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

PAD = 3          # the skipped key of the run pattern (4th smallest key)
B_, L_ = 8, 72   # the token layout of the kernel tests: T = 576
T_ = B_ * L_
NAMES = ("word", "pos", "type", "gamma", "beta")


# ------------------------------------------------------------------------------------------------ inputs
def _pattern(T, NK, g, CH=16):
    """Keys [T] in [0, NK) whose sorted order holds, from sorted position 0 (CH = 16 rows per chunk):
      key 0:  5 rows  [0, 5)      a run shorter than a chunk
      key 1: 11 rows  [5, 16)     a run that ends on a chunk boundary
      key 2: 16 rows  [16, 32)    a run of exactly one chunk
      key 3: 23 rows  [32, 55)    the padding key, across a chunk boundary
      key 4: 100 rows [55, 155)   start piece (9 rows), five whole-chunk middle pieces, end piece (11 rows)
      key 5: 16 rows  [155, 171)  a chunk's worth of rows across a boundary
      key 6:  5 rows  [171, 176)  ends on a chunk boundary
      keys 7 … 9: never occur
      keys 10 … 39: single rows
      the rest: random keys of the upper part of the range (some of them never occur)
    and whose token order is a random permutation (the rows of a run are scattered over the batch)."""
    assert CH == 16 and NK >= 60 and T >= 176 + 30 + 50
    counts = [5, 11, 16, 23, 100, 16, 5]
    keys = [torch.full((c,), k, dtype=torch.int64) for k, c in enumerate(counts)]
    keys.append(torch.arange(10, 40))
    rest = T - 176 - 30
    keys.append(torch.randint(40, NK, (rest,), generator=g))
    keys = torch.cat(keys)
    return keys[torch.randperm(T, generator=g)]


def _roberta_pids(g):
    """Position ids of a right-padded RoBERTa batch: cumsum(mask)·mask + pad with pad = 1 (offset 2)."""
    lens = torch.randint(L_ // 2, L_ + 1, (B_,), generator=g)
    lens[0] = L_
    mask = (torch.arange(L_)[None, :] < lens[:, None]).to(torch.int64)
    return (torch.cumsum(mask, 1) * mask + 1).reshape(-1), L_ + 2, 1   # pids, P, pad_pos


def _case(poscase, NTY, H, seed):
    g = torch.Generator().manual_seed(seed)
    V = 700
    ids = _pattern(T_, V, g)
    if poscase == "default":
        pids, P, pad_pos = torch.arange(L_).repeat(B_), L_ + 8, -1
    elif poscase == "pattern":
        pids, P, pad_pos = _pattern(T_, 300, g), 300, PAD
    else:
        pids, P, pad_pos = _roberta_pids(g)
    if NTY == 4:   # type 1 never occurs; the others are runs across many chunks
        tids = torch.tensor([0, 2, 3])[torch.randint(0, 3, (T_,), generator=g)]
    else:
        tids = torch.randint(0, NTY, (T_,), generator=g)
    ww, wp, wt = (torch.randn(V, H, generator=g) * 0.05, torch.randn(P, H, generator=g) * 0.05,
                  torch.randn(NTY, H, generator=g) * 0.05)
    gamma, beta = torch.randn(H, generator=g) * 0.3 + 1, torch.randn(H, generator=g) * 0.1
    dy = torch.randn(T_, H, generator=g)
    return SimpleNamespace(ids=ids, pids=pids, tids=tids, ww=ww, wp=wp, wt=wt, gamma=gamma, beta=beta, dy=dy, V=V, P=P,
                           NTY=NTY, H=H, pad_word=PAD, pad_pos=pad_pos, g=g)


def _init(c, accumulate):
    shapes = [(c.V, c.H), (c.P, c.H), (c.NTY, c.H), (c.H,), (c.H,)]
    return [torch.randn(*s, generator=c.g) if accumulate else torch.zeros(*s) for s in shapes]


def _bf(x):
    return x.to(torch.bfloat16)


def _run(k, cuda, c, prec, init, accumulate, det=True, p=0.1, seed=9, old_signature=False):
    """Forward (for mean / rstd) and backward of one precision on the GPU -> (grads on the CPU, mean, rstd, tables)."""
    dev = lambda t: t.to(cuda)  # noqa: E731
    out = [dev(t.clone()) for t in init]
    if prec == "fp32":
        tabs = (c.ww, c.wp, c.wt)
        _, m, rs = k.f32_embed_fwd(dev(c.ids), dev(c.pids), dev(c.tids), *map(dev, tabs), dev(c.gamma), dev(c.beta), 1e-12,
                                   p, seed, 0)
        args = (dev(c.dy), dev(c.ids), dev(c.pids), dev(c.tids), *map(dev, tabs), dev(c.gamma), m, rs, p, seed, 0, *out,
                accumulate, c.pad_word, c.pad_pos)
        k.f32_embed_bwd(*args) if old_signature else k.f32_embed_bwd(*args, det)
        dy = c.dy
    else:
        tabs = (_bf(c.ww), _bf(c.wp), _bf(c.wt))
        _, m, rs = k.embed_fwd(dev(c.ids), dev(c.pids), dev(c.tids), *map(dev, tabs), dev(c.gamma), dev(c.beta), 1e-12, p,
                               seed, 0)
        dy = _bf(c.dy)
        args = (dev(dy), dev(c.ids), dev(c.pids), dev(c.tids), *map(dev, tabs), dev(c.gamma), m, rs, p, seed, 0, *out,
                accumulate, c.pad_word, c.pad_pos, L_)
        k.embed_bwd(*args) if old_signature else k.embed_bwd(*args, det, det)   # deterministic, det_positions
    return [o.cpu() for o in out], m.cpu(), rs.cpu(), tabs, dy


def _oracle(c, tabs, dy, m, rs, init, accumulate, p=0.1, seed=9):
    refs = [t.clone() for t in init]
    ref.embed_bwd(dy.float(), c.ids, c.pids, c.tids, *(t.float() for t in tabs), c.gamma, m, rs, p, seed, 0, *refs,
                  accumulate, c.pad_word, c.pad_pos)
    return refs


def _close(prec, a, b, what):
    a, b = a.detach().double(), b.detach().double()
    err = (a - b).abs()
    if prec == "fp32":   # tests/test_f32_ops_gpu.py: 1e-5 relative to the largest value
        scale = float(b.abs().max()) + 1e-12
        assert float(err.max()) <= 1e-5 * scale, f"{what}: max err {float(err.max()):.3e} vs scale {scale:.3e}"
    else:                # tests/test_kernels_gpu.py::test_embedding: _close(a, b, 5e-2, 2e-2)
        bad = int((err > 5e-2 + 2e-2 * b.abs()).sum())
        assert bad == 0, f"{what}: {bad} / {a.numel()} outside tol, max err {float(err.max()):.3e}"


def _untouched(out, init, keys, NK, pad, what):
    """Rows of keys that never occur, and the skipped key's row, keep their initial value exactly."""
    absent = torch.ones(NK, dtype=torch.bool)
    absent[keys.unique()] = False
    assert bool(absent.any()), f"{what}: the case has no absent key"
    assert torch.equal(out[absent], init[absent]), f"{what}: absent rows changed"
    if pad >= 0:
        assert int((keys == pad).sum()) > 0
        assert torch.equal(out[pad], init[pad]), f"{what}: the padding row got a gradient"


# ------------------------------------------------------------------------- a. the sorted path against the oracle
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("poscase,NTY", [("default", 2), ("pattern", 4), ("roberta", 1)])
@pytest.mark.parametrize("H", [128, 768])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_sorted_path_matches_oracle(cuda, prec, H, poscase, NTY, accumulate):
    k = _native.kernels()
    c = _case(poscase, NTY, H, seed=H + NTY)
    init = _init(c, accumulate)
    out, m, rs, tabs, dy = _run(k, cuda, c, prec, init, accumulate)
    refs = _oracle(c, tabs, dy, m, rs, init, accumulate)
    for a, b, n in zip(out, refs, NAMES):
        _close(prec, a, b, f"{n} ({prec}, H={H}, {poscase}, NTY={NTY}, accumulate={accumulate})")
    _untouched(out[0], init[0], c.ids, c.V, c.pad_word, "word")
    _untouched(out[1], init[1], c.pids, c.P, c.pad_pos, "pos")
    if NTY == 4:
        _untouched(out[2], init[2], c.tids, c.NTY, -1, "type")


# ----------------------------------------------------------------------- b. bitwise against the documented order
def _documented_sum(keys, dx, init, pad, accumulate, CH):
    """The documented order on the CPU with fp32 adds: dx [T, H] one row per token -> the table [NK, H]."""
    out = init.clone()
    skeys, srows = torch.sort(keys, stable=True)
    chunk = torch.arange(keys.numel()) // CH
    for key in skeys.unique().tolist():
        if key == pad:
            continue
        pos = (skeys == key).nonzero().flatten()
        total = None
        for ch in chunk[pos].unique().tolist():         # pieces in chunk order
            piece = torch.zeros(dx.shape[1])
            for j in pos[chunk[pos] == ch].tolist():      # a piece from zero, in token order
                piece = piece + dx[srows[j]]
            total = piece if total is None else total + piece
        out[key] = total + init[key] if accumulate else total
    return out


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("H", [128, 768])
@pytest.mark.parametrize("prec,table", [("fp32", "word"), ("fp32", "pos"), ("fp32", "type"), ("bf16", "word"),
                                        ("bf16", "pos"), ("bf16", "type")])
def test_bitwise_documented_order(cuda, prec, table, H, accumulate):
    """Run A gives every token a key of its own, so each stored row is that token's dx; run B gives the tokens of a
    group the group's key.  The table rows of a group are equal, so both runs see the same x, dy, statistics and
    dropout mask and compute the same dx per token; run B's rows must equal the documented sum of run A's rows."""
    k = _native.kernels()
    CH = k.embed_run_chunk()
    assert CH == 16
    c = _case("default", 2, H, seed=7 * H)
    g = c.g
    NKB = 200
    keys_b = _pattern(T_, NKB, g, CH)                       # the long run: 100 rows over 7 chunks
    keys_a = NKB + torch.arange(T_)                          # one key per token
    base = torch.randn(NKB, H, generator=g) * 0.05
    tab = torch.cat([base, base[keys_b]])                    # row NKB + t equals row keys_b[t]
    if prec == "bf16":
        tab = _bf(tab).float()
    if table == "word":
        c.ww, c.V = tab, NKB + T_
    elif table == "pos":
        c.wp, c.P, c.pad_pos = tab, NKB + T_, PAD
    else:   # more than 2 types: the type rows come from the sorted runs too, and no type is skipped
        c.wt, c.NTY = tab, NKB + T_
    field = {"word": "ids", "pos": "pids", "type": "tids"}[table]
    ti = NAMES.index(table)
    pad = -1 if table == "type" else PAD
    # run A: fresh tables, the statistics of run B's forward (equal x), one row per token
    setattr(c, field, keys_b)
    init_b = _init(c, accumulate)
    out_b, m, rs, _, _ = _run(k, cuda, c, prec, init_b, accumulate)
    setattr(c, field, keys_a)
    out_a, m_a, rs_a, _, _ = _run(k, cuda, c, prec, _init(c, False), False)
    assert torch.equal(m, m_a) and torch.equal(rs, rs_a), "both runs must see the same x"
    dx = out_a[ti][NKB:]
    want = _documented_sum(keys_b, dx, init_b[ti], pad, accumulate, CH)
    assert int((keys_b == 4).sum()) > 4 * CH
    assert torch.equal(out_b[ti], want), (
        f"{prec} {table} rows differ from the documented order in "
        f"{int((out_b[ti] != want).any(1).sum())} rows, max diff {float((out_b[ti] - want).abs().max()):.3e}")


# ----------------------------------------------------------------------------------------------- c. run to run
@pytest.mark.parametrize("prec,poscase,NTY", [("fp32", "pattern", 4), ("fp32", "roberta", 2), ("bf16", "roberta", 4)])
def test_run_to_run_bitwise(cuda, prec, poscase, NTY):
    k = _native.kernels()
    c = _case(poscase, NTY, 768, seed=21)
    init = _init(c, False)
    first = _run(k, cuda, c, prec, init, False)[0]
    second = _run(k, cuda, c, prec, init, False)[0]
    for a, b, n in zip(first, second, NAMES):
        assert torch.equal(a, b), f"{prec} {n}: two runs differ"


# -------------------------------------------------------------------------------------------------- f. flag off
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_old_signature_still_matches_oracle(cuda, prec):
    """The trailing flags default to off: the positional signatures of before still run (the atomic paths)."""
    k = _native.kernels()
    c = _case("pattern", 4, 768, seed=33)
    for accumulate in (False, True):
        init = _init(c, accumulate)
        out, m, rs, tabs, dy = _run(k, cuda, c, prec, init, accumulate, old_signature=True)
        refs = _oracle(c, tabs, dy, m, rs, init, accumulate)
        for a, b, n in zip(out, refs, NAMES):
            _close(prec, a, b, f"{n} ({prec}, accumulate={accumulate})")


# --------------------------------------------------------------------------------------------- d / e. whole steps
def _engine(model):
    from ml_recipe_distributed_pytorch_amd.models.losses import build_loss
    from ml_recipe_distributed_pytorch_amd.train.engine import TrainEngine
    from ml_recipe_distributed_pytorch_amd.train.optim import FusedAdamW
    from ml_recipe_distributed_pytorch_amd.train.trainer import optimizer_groups
    lp = SimpleNamespace(loss="smooth", smooth_alpha=0.01, w_start=1, w_end=1, w_start_reg=1, w_end_reg=1, w_cls=1)
    opt = FusedAdamW(optimizer_groups(model.named_parameters(), 1e-4), model.store, lr=1e-3, correct_bias=False,
                     zero_grad_fn=model.zero_grad)
    return TrainEngine(model, build_loss(lp), opt)


def _batches(V, pad, B, L, n, seed, types):
    """n batches of right-padded rows with ids in [0, V) that are not the padding id."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        ids = torch.randint(0, V - 1, (B, L), generator=g)
        ids[ids >= pad] += 1
        lens = torch.randint(L // 2, L + 1, (B,), generator=g)
        lens[0] = L
        mask = torch.arange(L)[None, :] < lens[:, None]
        ids[~mask] = pad
        tt = torch.zeros_like(ids)
        if types > 1:
            tt[:, L // 3:] = 1
        labels = {"start_class": torch.zeros(B, dtype=torch.int64), "end_class": torch.full((B,), L - 1, dtype=torch.int64),
                  "start_reg": torch.zeros(B), "end_reg": torch.ones(B), "cls": torch.zeros(B, dtype=torch.int64)}
        out.append(({"input_ids": ids, "attention_mask": mask, "token_type_ids": tt}, labels))
    return out


def _two_runs(cuda, cfg, precision, batches):
    from ml_recipe_distributed_pytorch_amd.train.engine import to_device
    arenas = []
    for _ in range(2):
        m = BertForQuestionAnswering(cfg, seed=0, precision=precision).to(cuda).train()
        eng = _engine(m)
        torch.manual_seed(17)   # the steps draw their dropout seeds from the host generator
        for inputs, labels in batches:
            res = eng.step([(to_device(inputs, cuda), to_device(labels, cuda))])
            loss = res.losses.to_floats()["loss"]
            assert loss == loss
        torch.cuda.synchronize()
        arenas.append((m.store.master.cpu().clone(), m.store.grad.cpu().clone()))
    return arenas


def test_fp32_steps_are_bitwise_reproducible(cuda, monkeypatch):
    """bert-tiny with a 64-word vocabulary (every id repeats many times), dropout on, 3 optimizer steps in fp32 under
    HQ_DETERMINISTIC=1: two models from the same seed fed the same batches end bitwise equal."""
    monkeypatch.setenv("HQ_DETERMINISTIC", "1")
    cfg = get_config("bert-tiny-test", vocab_size=64)
    (m1, g1), (m2, g2) = _two_runs(cuda, cfg, "fp32", _batches(64, 0, 8, 64, 3, seed=1, types=2))
    assert m1.dtype == torch.float32 and float(g1.abs().sum()) > 0
    assert torch.equal(m1, m2), f"master arenas differ in {int((m1 != m2).sum())} elements"
    assert torch.equal(g1, g2), f"grad arenas differ in {int((g1 != g2).sum())} elements"


def _roberta_cfg():
    return get_config("roberta-base", vocab_size=1024, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                      intermediate_size=256)


def test_roberta_bf16_steps_are_bitwise_reproducible(cuda, monkeypatch):
    """RoBERTa position ids (cumsum(mask)·mask + 1) take the deterministic-positions mode under HQ_DETERMINISTIC=1."""
    monkeypatch.setenv("HQ_DETERMINISTIC", "1")
    cfg = _roberta_cfg()
    (m1, g1), (m2, g2) = _two_runs(cuda, cfg, "bf16", _batches(cfg.vocab_size, cfg.pad_token_id, 8, 64, 3, seed=2, types=1))
    assert float(g1.abs().sum()) > 0
    assert torch.equal(m1, m2), f"master arenas differ in {int((m1 != m2).sum())} elements"
    assert torch.equal(g1, g2), f"grad arenas differ in {int((g1 != g2).sum())} elements"


def test_roberta_bf16_grads_match_cpu(cuda, monkeypatch):
    """One RoBERTa step's outputs and gradients, deterministic-positions mode on, against the CPU path of the same
    model at the bounds tests/test_model_gpu.py uses for BERT."""
    monkeypatch.setenv("HQ_DETERMINISTIC", "1")
    cfg = _roberta_cfg()
    cpu = BertForQuestionAnswering(cfg, seed=0)
    gpu = copy.deepcopy(cpu).to(cuda)
    cpu.train()
    gpu.train()
    inputs, _ = _batches(cfg.vocab_size, cfg.pad_token_id, 4, 64, 1, seed=3, types=1)[0]
    ids, mask, tt = inputs["input_ids"], inputs["attention_mask"], inputs["token_type_ids"]
    torch.manual_seed(11)
    oc = cpu(ids, mask, tt)
    torch.manual_seed(11)
    og = gpu(ids.to(cuda), mask.to(cuda), tt.to(cuda))
    for key in oc:
        a, b = og[key].float().cpu(), oc[key].float()
        assert (a - b).abs().max().item() < 5e-2 * (1 + b.abs().max().item()), key
    lc = sum(v.float().sum() for n, v in oc.items() if n != "cls")
    lg = sum(v.float().sum() for n, v in og.items() if n != "cls")
    cpu.zero_grad()
    gpu.zero_grad()
    lc.backward()
    lg.backward()
    gc, gg = cpu.store.grad, gpu.store.grad.cpu()
    rel = (gc - gg).norm() / gc.norm()
    assert rel.item() < 5e-2, f"grad arena rel err {rel.item():.3e}"
    # the position table alone (its rows come from the sorted runs), and the padding position gets nothing
    pc = cpu.store.view("transformer.embeddings.position_embeddings.weight", "grad")
    pg = gpu.store.view("transformer.embeddings.position_embeddings.weight", "grad").cpu()
    assert ((pc - pg).norm() / pc.norm()).item() < 5e-2
    assert float(pg[cfg.pad_token_id].abs().max()) == 0.0
