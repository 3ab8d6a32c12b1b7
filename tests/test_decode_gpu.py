"""Joint valid-span decoding on the GPU (csrc/kernels/decode.hip) against ``ops.reference.qa_decode`` on the CPU,
bit for bit in all six columns: shapes around the wave width and the row-per-block count, the window and length
edge cases, tie-heavy logits, the three memory layouts (contiguous, interleaved stride-2 views with 8-byte loads,
misaligned stride-2 views with scalar loads), the binding's refusals and the predictor on a real model's outputs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_DECOR = 7


def _decorate(r, k, start, end, lo, hi, L, W):
    """Edge case ``k`` in row ``r``.  Every case leaves lo / hi such that the oracle defines the answer."""
    if k == 0:      # empty window
        lo[r] = hi[r] = L // 2
    elif k == 1:    # a single candidate
        lo[r] = L // 3
        hi[r] = lo[r] + 1
    elif k == 2:    # the whole row
        lo[r], hi[r] = 0, L
    elif k == 3:    # out of range on both sides: the kernel clamps
        lo[r], hi[r] = -3, L + 9
    elif k == 4:    # the winner forced to (63, 64), across the lane boundary (rows of at least 65 positions)
        lo[r], hi[r] = 0, L
        if L >= 65 and W >= 2:
            start[r, 63] += 50.0
            end[r, 64] += 50.0
    elif k == 5:    # the winner forced to the last candidate (hi - 1, hi - 1)
        lo[r], hi[r] = L // 5, L - L // 7
        if hi[r] > lo[r]:
            start[r, hi[r] - 1] += 50.0
            end[r, hi[r] - 1] += 50.0
    elif k == 6:    # +1e4 planted just outside [lo, hi) and one position beyond the length bound
        lo[r], hi[r] = L // 4 + 1, max(L // 4 + 1, (3 * L) // 4)
        for p in (lo[r] - 1, hi[r]):
            if 0 <= p < L:
                start[r, p] = end[r, p] = 1e4
        e = hi[r] - 1
        if e - W >= lo[r]:   # (e - W, e) is one token too long; every shorter span ending at e is allowed
            end[r, e] = 1e4
            start[r, e - W] = 30.0


def make_case(B, L, W, grid, shift, seed):
    g = torch.Generator().manual_seed(seed)
    if grid:   # 0.5 grid: many keys tie
        logits = torch.randint(-4, 5, (B, L, 2), generator=g).float() * 0.5
        cls = torch.randint(-2, 3, (B, 5), generator=g).float() * 0.5
    else:
        logits = torch.randn(B, L, 2, generator=g) * 3
        cls = torch.randn(B, 5, generator=g)
    reg = torch.rand(B, 2, generator=g)
    lo = torch.randint(0, L, (B,), generator=g).tolist()
    hi = [int(torch.randint(l, L + 1, (1,), generator=g)) for l in lo]
    start, end = logits[..., 0], logits[..., 1]   # views: the decorations write into `logits`
    for r in range(B):
        _decorate(r, (r + shift) % N_DECOR, start, end, lo, hi, L, W)
    return logits, cls, reg, torch.tensor(lo, dtype=torch.int32), torch.tensor(hi, dtype=torch.int32)


# (B, L, W, grid, shift): L around the wave width, B no multiple of the 4 rows per block, W in {1, 30, L, 10 L}
CASES = [(1, 1, 1, False, 2), (1, 1, 10, False, 3), (5, 33, 1, True, 0), (5, 33, 330, False, 2), (7, 64, 30, False, 0),
         (7, 64, 64, True, 0), (5, 65, 65, False, 3), (7, 65, 30, True, 0), (7, 65, 1, False, 0),
         (7, 512, 30, False, 0), (5, 512, 5120, False, 2), (1, 512, 512, True, 4)]


def _bytes(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


@pytest.mark.parametrize("B,L,W,grid,shift", CASES)
def test_kernel_matches_oracle_in_every_layout(cuda, B, L, W, grid, shift):
    from ml_recipe_distributed_pytorch_amd import ops
    from ml_recipe_distributed_pytorch_amd._native import kernels
    logits, cls, reg, lo, hi = make_case(B, L, W, grid, shift, seed=B * 10000 + L * 10 + W % 7)
    want = ops.reference.qa_decode(logits[..., 0], logits[..., 1], cls, reg[:, 0], reg[:, 1], lo, hi, W)
    assert want.device.type == "cpu"
    cls_d, lo_d, hi_d = cls.to(cuda), lo.to(cuda), hi.to(cuda)

    # contiguous inputs: scalar loads, element stride 1
    args = (logits[..., 0].contiguous().to(cuda), logits[..., 1].contiguous().to(cuda), cls_d,
            reg[:, 0].contiguous().to(cuda), reg[:, 1].contiguous().to(cuda), lo_d, hi_d)
    assert not kernels().qa_decode_interleaved(*args)
    got = ops.qa_decode(*args, W)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, 6) and got.is_cuda
    assert _bytes(got) == _bytes(want), (got.cpu(), want)

    # the views the fused heads return: one [B, L, 2] buffer and one [B, 2] reg buffer, read in place (8-byte loads)
    buf, rbuf = logits.to(cuda), reg.to(cuda)
    start, end = buf[..., 0], buf[..., 1]
    assert start.data_ptr() == buf.data_ptr() and end.data_ptr() == buf.data_ptr() + 4 and start.stride() == (2 * L, 2)
    args = (start, end, cls_d, rbuf[:, 0], rbuf[:, 1], lo_d, hi_d)
    assert kernels().qa_decode_interleaved(*args)
    keep = buf.clone()
    got_v = ops.qa_decode(*args, W)
    assert _bytes(got_v) == _bytes(want), (got_v.cpu(), want)
    assert torch.equal(buf, keep)

    # the same views four bytes off an 8-byte boundary: stride-2 scalar loads
    flat = torch.empty(B * L * 2 + 1, device=cuda)
    flat[1:].copy_(buf.reshape(-1))
    off = flat[1:].view(B, L, 2)
    assert off.data_ptr() % 8 == 4
    args = (off[..., 0], off[..., 1], cls_d, rbuf[:, 0], rbuf[:, 1], lo_d, hi_d)
    assert not kernels().qa_decode_interleaved(*args)
    got_o = ops.qa_decode(*args, W)
    assert _bytes(got_o) == _bytes(want), (got_o.cpu(), want)


def test_forced_winners_are_where_the_cases_put_them():
    """The decorations do what they say (checked on the oracle, so the kernel test above covers those rows)."""
    from ml_recipe_distributed_pytorch_amd import ops
    logits, cls, reg, lo, hi = make_case(7, 512, 30, False, 0, seed=1)
    r = ops.reference.qa_decode(logits[..., 0], logits[..., 1], cls, reg[:, 0], reg[:, 1], lo, hi, 30)
    assert r[0, 0] == float("-inf") and r[0, 1] == -1 and r[0, 2] == -1
    assert r[1, 1] == 170 and r[1, 2] == 170
    assert (r[4, 1], r[4, 2]) == (63, 64)
    assert (r[5, 1], r[5, 2]) == (hi[5] - 1, hi[5] - 1)
    assert r[6, 2] == hi[6] - 1 and hi[6] - 30 < r[6, 1] <= hi[6] - 1   # the planted start one token too far loses


def test_binding_refuses_bad_inputs(cuda):
    from ml_recipe_distributed_pytorch_amd import ops

    def args(B=3, L=16, dev=cuda):
        z = torch.zeros(B, L, device=dev)
        return [z, z.clone(), torch.zeros(B, 5, device=dev), torch.zeros(B, device=dev), torch.zeros(B, device=dev),
                torch.zeros(B, dtype=torch.int32, device=dev), torch.full((B,), L, dtype=torch.int32, device=dev)]
    assert tuple(ops.qa_decode(*args(), 30).shape) == (3, 6)
    with pytest.raises(RuntimeError, match="L <= 512"):
        ops.qa_decode(*args(L=513), 30)
    with pytest.raises(RuntimeError, match="max answer length"):
        ops.qa_decode(*args(), 0)
    a = args()
    a[5] = a[5].long()
    with pytest.raises(RuntimeError, match="qa_decode: lo has dtype Long, expected Int"):
        ops.qa_decode(*a, 30)
    a = args()
    a[6] = a[6].cpu()
    with pytest.raises(RuntimeError, match="qa_decode: hi is on cpu, expected cuda"):
        ops.qa_decode(*a, 30)
    a = args()
    a[2] = torch.zeros(3, 9, device=cuda)
    with pytest.raises(RuntimeError, match="classes"):
        ops.qa_decode(*a, 30)
    empty = ops.qa_decode(*args(B=0), 30)
    assert tuple(empty.shape) == (0, 6)
    half = args()
    half[0], half[1] = half[0].bfloat16(), half[1].bfloat16()   # non-fp32 logits are widened first
    assert ops.qa_decode(*half, 30).dtype == torch.float32


def test_predictor_decodes_the_models_own_outputs(cuda):
    from ml_recipe_distributed_pytorch_amd import ops
    from ml_recipe_distributed_pytorch_amd.data.collate import collate_fun
    from ml_recipe_distributed_pytorch_amd.data.dummy import DummyChunkDataset, SpecialIds
    from ml_recipe_distributed_pytorch_amd.infer.predictor import Predictor
    from ml_recipe_distributed_pytorch_amd.models.bert import BertForQuestionAnswering
    from ml_recipe_distributed_pytorch_amd.models.config import get_config
    from ml_recipe_distributed_pytorch_amd.train.engine import to_device
    cfg = get_config("bert-base-uncased", num_hidden_layers=1, hidden_size=128, num_attention_heads=2,
                     intermediate_size=512)
    model = BertForQuestionAnswering(cfg, seed=3).to(cuda).eval()
    sp = SpecialIds()
    ds = DummyChunkDataset(max_seq_len=64, max_question_len=8, dataset_len=2, n_chunks=3, special_ids=sp)
    items = ds[0] + ds[1]
    inputs, _, items = collate_fun(items, return_items=True, pad_token_id=sp.pad_token_id,
                                   sep_token_id=sp.sep_token_id, model_name="bert")
    p = Predictor(model, cuda, n_jobs=0, span_decode="joint", max_answer_len=30)
    with torch.no_grad():
        preds = model(**to_device(inputs, cuda))
        L = preds["start_class"].shape[1]
        # the stride-2 views of the fused heads' buffers, handed to the kernel as they are
        assert preds["start_class"].stride() == (2 * L, 2) and preds["start_reg"].stride() == (2,)
        assert preds["end_class"].data_ptr() == preds["start_class"].data_ptr() + 4
        r = p.decode_batch(preds, items)
    assert r.dtype == np.float64 and r.shape == (6, 6)
    lo = torch.tensor([it.question_len + 2 for it in items], dtype=torch.int32)
    hi = torch.tensor([len(it.input_ids) - 1 for it in items], dtype=torch.int32)
    want = ops.reference.qa_decode(*(preds[k].float().cpu() for k in ("start_class", "end_class", "cls", "start_reg",
                                                                        "end_reg")), lo, hi, 30)
    assert r.astype(np.float32).tobytes() == want.numpy().tobytes(), (r, want)
    assert (r[:, 1] >= 10).all() and (r[:, 2] < 63).all() and (r[:, 2] - r[:, 1] < 30).all()
