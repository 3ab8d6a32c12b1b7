"""Joint valid-span decoding on the CPU: the torch formulation (``ops.reference.qa_decode``) against a double-loop
``numpy.float32`` brute force, bit for bit; the predictor's two decode modes on a stub model with crafted logits; the
parser flags; the validate CLI in joint mode.  Everything here is exact: no tolerance appears anywhere."""
import json
import os

import numpy as np
import pytest
import torch

from ml_recipe_distributed_pytorch_amd import ops
from ml_recipe_distributed_pytorch_amd.data.collate import collate_fun
from ml_recipe_distributed_pytorch_amd.data.items import ChunkItem
from ml_recipe_distributed_pytorch_amd.infer.predictor import Predictor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------ oracle against brute force
def brute_force(start, end, cls, start_reg, end_reg, lo, hi, W):
    """The definition, as two plain loops in numpy.float32 (every add / subtract is one rounded fp32 operation)."""
    B, L = start.shape
    out = np.empty((B, 6), np.float32)
    for b in range(B):
        lo_b, hi_b = min(max(int(lo[b]), 0), L), min(max(int(hi[b]), 0), L)
        best = None
        for s in range(lo_b, hi_b):
            for e in range(s, min(s + W, hi_b)):
                key = np.float32(start[b, s] + end[b, e])
                if best is None or key > best[0]:   # strict: the first (smallest s, then smallest e) of equals wins
                    best = (key, s, e)
        if best is None:
            score, s_id, e_id = np.float32(-np.inf), -1, -1
        else:
            score, s_id, e_id = np.float32(best[0] - np.float32(start[b, 0] + end[b, 0])), best[1], best[2]
        label = 0
        for c in range(1, cls.shape[1]):
            if cls[b, c] > cls[b, label]:
                label = c
        out[b] = (score, s_id, e_id, start_reg[b], end_reg[b], label)
    return out


def make_case(B, L, W, grid, seed):
    rng = np.random.default_rng(seed)
    if grid:   # logits on a 0.5 grid: many candidate keys tie
        start = (rng.integers(-4, 5, (B, L)) * 0.5).astype(np.float32)
        end = (rng.integers(-4, 5, (B, L)) * 0.5).astype(np.float32)
        cls = (rng.integers(-2, 3, (B, 5)) * 0.5).astype(np.float32)
    else:
        start = (rng.standard_normal((B, L)) * 3).astype(np.float32)
        end = (rng.standard_normal((B, L)) * 3).astype(np.float32)
        cls = rng.standard_normal((B, 5)).astype(np.float32)
    lo = rng.integers(0, L, B).astype(np.int32)
    hi = np.array([rng.integers(l, L + 1) for l in lo], np.int32)
    lo[0], hi[0] = L // 2, L // 2          # empty window
    lo[1], hi[1] = L // 3, L // 3 + 1      # a single candidate
    lo[2], hi[2] = 0, L                    # the whole row
    sreg, ereg = rng.random(B).astype(np.float32), rng.random(B).astype(np.float32)
    return start, end, cls, sreg, ereg, lo, hi


CASES = [(7, 40, 5, False), (9, 33, 1, True), (5, 64, 64, False), (6, 65, 30, False), (8, 37, 1000, False),
         (4, 512, 30, False)]


@pytest.mark.parametrize("B,L,W,grid", CASES)
def test_reference_matches_brute_force(B, L, W, grid):
    arrs = make_case(B, L, W, grid, seed=B * 1000 + L)
    want = brute_force(*arrs, W)
    got = ops.reference.qa_decode(*(torch.from_numpy(a) for a in arrs), W)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, 6)
    assert want[0, 1] == -1 and want[0, 2] == -1 and want[0, 0] == -np.inf, want[0]
    assert want[1, 1] == L // 3 and want[1, 2] == L // 3
    assert got.numpy().tobytes() == want.tobytes(), (got, want)
    # the public op on CPU tensors is the reference
    pub = ops.qa_decode(*(torch.from_numpy(a) for a in arrs), W)
    assert pub.numpy().tobytes() == want.tobytes()


def test_reference_rejects_zero_length():
    arrs = make_case(4, 8, 1, False, seed=0)
    with pytest.raises(ValueError):
        ops.reference.qa_decode(*(torch.from_numpy(a) for a in arrs), 0)


# ------------------------------------------------------------------------------------ predictor on a stub model
Q = 2            # question_len of every stub chunk: the document part starts at Q + 2 = 4
PAD_L = 16       # the longest chunk; every batch holds all chunks, so every row is padded to this length


class _Stub(torch.nn.Module):
    """Returns the logits crafted for each chunk; input_ids[1] carries the chunk's key."""

    def __init__(self, table):
        super().__init__()
        self.table = table

    def forward(self, input_ids, **kw):
        B, L = input_ids.shape
        start, end = torch.zeros(B, L), torch.zeros(B, L)
        cls = torch.zeros(B, 5)
        for b in range(B):
            spec = self.table[int(input_ids[b, 1])]
            for pos, v in spec["start"].items():
                start[b, pos] = v
            for pos, v in spec["end"].items():
                end[b, pos] = v
            cls[b, spec["label"]] = 1.0
        key = input_ids[:, 1].float()
        return {"start_class": start, "end_class": end, "cls": cls, "start_reg": key / 100, "end_reg": key / 50}


# key -> (document, chunk length, chunk_start, logits).  Unlisted positions have logit 0.
CHUNKS = {
    # independent argmaxes are inverted (start 9 > end 6); the best valid span is (5, 6) with key 3 + 5
    11: ("inverted", 12, 0, {"start": {9: 5.0, 5: 3.0}, "end": {6: 5.0, 7: 2.0}, "label": 2}),
    # the largest key (4, 12) is 9 tokens long; within 4 tokens the best is (10, 12) with key 2 + 6
    21: ("long", 16, 0, {"start": {4: 6.0, 10: 2.0}, "end": {12: 6.0}, "label": 3}),
    # the best span scores below CLS: key 2 against start[0] + end[0] = 8
    31: ("negative", 12, 0, {"start": {0: 4.0, 6: 1.0}, "end": {0: 4.0, 7: 1.0}, "label": 1}),
    # huge logits inside the question (2), on the final separator (9) and in the padding (13, 14)
    41: ("outside", 10, 0, {"start": {2: 100.0, 9: 100.0, 13: 100.0, 5: 1.0},
                            "end": {3: 100.0, 9: 100.0, 14: 100.0, 6: 1.0}, "label": 0}),
    # three chunks of one document with scores 3, 7, 7: the later of the equal scores replaces the earlier
    51: ("multi", 12, 0, {"start": {5: 1.0}, "end": {6: 2.0}, "label": 2}),
    52: ("multi", 12, 7, {"start": {6: 3.0}, "end": {8: 4.0}, "label": 2}),
    53: ("multi", 12, 14, {"start": {7: 5.0}, "end": {7: 2.0}, "label": 4}),
    # no document tokens at all: [CLS] q q [SEP] [SEP]
    61: ("empty", 5, 0, {"start": {0: 1.0}, "end": {0: 1.0}, "label": 0}),
}


class _Docs:
    def __init__(self):
        by_doc = {}
        for key, (doc, n, cs, _) in CHUNKS.items():
            ids = [7] * n
            ids[1] = key
            by_doc.setdefault(doc, []).append(ChunkItem(doc, ids, 0, 0, 0, "", "", 0, -1, -1, question_len=Q,
                                                         chunk_start=cs))
        self.docs = list(by_doc.values())

    def __len__(self):
        return len(self.docs)

    def __getitem__(self, i):
        return self.docs[i]


def _run(**kw):
    model = _Stub({k: v[3] for k, v in CHUNKS.items()})
    p = Predictor(model, "cpu", batch_size=64, n_jobs=0, **kw,
                  collate_fun=lambda items: collate_fun(items, return_items=True, pad_token_id=0, sep_token_id=3,
                                                        model_name="bert"))
    return p(_Docs())


def test_predictor_argmax_default_is_the_score_batch_path(monkeypatch):
    def never(*a, **k):
        raise AssertionError("argmax mode must not call decode_batch")
    monkeypatch.setattr(Predictor, "decode_batch", never)
    p = _run()
    assert p.span_decode == "argmax" and p.max_answer_len == 30
    # today's rule, written out: independent argmaxes scored by score_batch, then _is_valid
    docs = _Docs()
    items = [c for d in docs.docs for c in d]
    inputs, _, _ = collate_fun(items, return_items=True, pad_token_id=0, sep_token_id=3, model_name="bert")
    r = Predictor.score_batch(_Stub({k: v[3] for k, v in CHUNKS.items()})(**inputs))
    best, want = {}, {}
    for (sc, s, e, sr, er, lb), it in zip(r, items):
        if s > e or s < it.question_len + 2 or best.get(it.item_id, 0.0) > sc:
            continue
        best[it.item_id] = sc
        want[it.item_id] = (int(s), int(e), float(sr), float(er), int(lb), float(sc))
    got = {k: (c.start_id, c.end_id, c.start_reg, c.end_reg, c.label, c.score) for k, c in p.candidates.items()}
    assert got == want
    # the shortcut loses the documents whose argmax pair is no span
    assert "inverted" not in got and "negative" not in got and "outside" not in got
    assert got["long"][:2] == (4, 12)
    assert p.metrics()["chunks"] == len(CHUNKS)


def test_predictor_joint_mode(tmp_path):
    p = _run(span_decode="joint", max_answer_len=4)
    c = p.candidates
    assert (c["inverted"].start_id, c["inverted"].end_id, c["inverted"].score) == (5, 6, 8.0)
    assert (c["long"].start_id, c["long"].end_id, c["long"].score) == (10, 12, 8.0)
    assert (c["negative"].start_id, c["negative"].end_id, c["negative"].score) == (6, 7, -6.0)
    assert (c["outside"].start_id, c["outside"].end_id, c["outside"].score) == (5, 6, 2.0)
    assert (c["multi"].start_id, c["multi"].end_id, c["multi"].score) == (7, 7, 7.0)
    assert p.items["multi"].chunk_start == 14 and c["multi"].label == 4
    assert c["inverted"].label == 2 and c["inverted"].start_reg == pytest.approx(0.11)
    assert "empty" not in c and "empty" not in p.items
    m = p.metrics()
    assert m["documents"] == 5 and m["chunks"] == len(CHUNKS)
    # decode_batch alone: [B, 6] float64, equal to the reference on the same logits and windows
    items = [x for d in _Docs().docs for x in d]
    inputs, _, _ = collate_fun(items, return_items=True, pad_token_id=0, sep_token_id=3, model_name="bert")
    preds = p.model(**inputs)
    r = p.decode_batch(preds, items)
    assert r.dtype == np.float64 and r.shape == (len(items), 6)
    lo = torch.tensor([it.question_len + 2 for it in items], dtype=torch.int32)
    hi = torch.tensor([len(it.input_ids) - 1 for it in items], dtype=torch.int32)
    want = ops.reference.qa_decode(preds["start_class"], preds["end_class"], preds["cls"], preds["start_reg"],
                                   preds["end_reg"], lo, hi, 4)
    assert r.astype(np.float32).tobytes() == want.numpy().tobytes()
    # with the default length bound the long span is allowed again
    assert _run(span_decode="joint").candidates["long"].end_id == 12
    assert _run(span_decode="joint").candidates["long"].start_id == 4
    # predictions file: joint mode records its settings, argmax mode keeps today's two keys
    p.save_predictions(str(tmp_path / "joint.json"))
    doc = json.load(open(tmp_path / "joint.json"))
    assert doc["span_decode"] == "joint" and doc["max_answer_len"] == 4 and len(doc["predictions"]) == 5
    q = _run()
    q.save_predictions(str(tmp_path / "argmax.json"))
    assert list(json.load(open(tmp_path / "argmax.json"))) == ["metrics", "predictions"]


def test_predictor_rejects_unknown_mode():
    with pytest.raises(ValueError, match="span_decode"):
        Predictor(torch.nn.Linear(1, 1), "cpu", n_jobs=0, span_decode="nbest")
    with pytest.raises(ValueError, match="max_answer_len"):
        Predictor(torch.nn.Linear(1, 1), "cpu", n_jobs=0, span_decode="joint", max_answer_len=0)


# ------------------------------------------------------------------------------------ flags and CLI
def test_parser_flags():
    from ml_recipe_distributed_pytorch_amd.utils import flags
    base = ["--data_path", "x", "--processed_data_path", "y", "--checkpoint", "None"]
    parser = flags.get_predictor_parser()
    a = parser.parse_known_args(base)[0]
    assert a.span_decode == "argmax" and a.max_answer_len == 30
    a = parser.parse_known_args(base + ["--span_decode", "joint", "--max_answer_len", "12"])[0]
    assert a.span_decode == "joint" and a.max_answer_len == 12
    with pytest.raises(SystemExit):
        parser.parse_known_args(base + ["--span_decode", "nbest"])


def test_validate_cli_joint(host_lib):
    from ml_recipe_distributed_pytorch_amd.cli import validate
    vcfg = os.path.join(ROOT, "config", "validate.cfg")
    pred = validate.cli(["-c", vcfg, "--checkpoint", "None", "--dummy_dataset", "--dummy_dataset_len", "6",
                         "--data_path", "x", "--processed_data_path", "x", "--span_decode", "joint",
                         "--model", "bert-tiny-test", "--max_seq_len", "48", "--max_question_len", "8", "--n_jobs", "0"])
    m = pred.metrics()
    assert pred.span_decode == "joint" and pred.max_answer_len == 30
    assert m["chunks"] == 18 and m["documents"] == 6
