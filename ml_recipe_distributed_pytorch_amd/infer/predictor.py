"""Chunked QA inference (reference ``modules/model/inference/predictor.py:14-144``).

Two span-decoding rules, chosen by ``span_decode``:

* ``"argmax"`` (default; the reference's rule, outputs unchanged): per chunk the argmax of the start logits and the
  argmax of the end logits, taken *independently*, softmax-argmax class, and the score
  ``max_start + max_end − (start[CLS] + end[CLS])``.  This is a shortcut, not the rule of arXiv:1901.08634: the two
  maxima need not form a span, and a chunk whose pair is invalid (start after end, or start inside the question,
  ``< question_len + 2``) is dropped.  Per document the best valid chunk wins (score not below the best so far).
* ``"joint"`` (the paper's rule): per chunk the maximum of ``start[s] + end[e]`` over the *valid* spans only — both
  ends inside the document part ``[question_len + 2, len(input_ids) − 1)``, ``s ≤ e``, at most ``max_answer_len``
  tokens — minus ``start[CLS] + end[CLS]`` (``ops.qa_decode``: one HIP kernel on the GPU, ``ops.reference`` on the
  CPU, bit-identical).  Every chunk with a non-empty document part yields a candidate; a negative score (the model
  prefers "no answer" for that chunk) is legal, and the document keeps its best span.

Either way scoring runs per batch on device; a single device→host copy per batch carries everything the
candidate update needs.

Additions (D12): ``metrics()`` — label accuracy, span exact-match / token-F1 against the true
document-token span, and coverage — and ``predicted_text`` for ``show_predictions``.
"""
from __future__ import annotations

import json
import logging
from collections import defaultdict
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch

from .. import ops
from ..data.items import ID2LABELS
from ..data.list_loader import ListDataloader
from ..train.engine import to_device

logger = logging.getLogger(__name__)

SPAN_DECODE_MODES = ("argmax", "joint")


def _neg_inf() -> float:
    return float("-inf")


@dataclass
class PredictorCandidate:
    start_id: int
    end_id: int
    start_reg: float
    end_reg: float
    label: int
    score: float = 0.0


def doc_span(item, start_id: int, end_id: int):
    """Chunk token positions → document token positions."""
    off = item.chunk_start - (item.question_len + 2)
    return start_id + off, end_id + off


class Predictor:
    def __init__(self, model, device, *, batch_size=256, n_jobs=16, collate_fun=None, buffer_size=4096, limit=None,
                 timeout_s: float = 600.0, span_decode: str = "argmax", max_answer_len: int = 30):
        if span_decode not in SPAN_DECODE_MODES:
            raise ValueError(f"span_decode must be one of {SPAN_DECODE_MODES}, got {span_decode!r}")
        if int(max_answer_len) < 1:
            raise ValueError(f"max_answer_len must be >= 1, got {max_answer_len}")
        self.span_decode, self.max_answer_len = span_decode, int(max_answer_len)
        self.model = model
        self.device = torch.device(device)
        self.model.to(self.device)
        # a document's running best: 0.0 under the argmax rule (its scores are >= 0), -inf under the joint rule
        self.scores: Dict[str, float] = defaultdict(float if span_decode == "argmax" else _neg_inf)
        self.candidates: Dict[str, PredictorCandidate] = {}
        self.items = {}
        self.batch_size, self.n_jobs, self.collate_fun = batch_size, n_jobs, collate_fun
        self.buffer_size, self.limit, self.timeout_s = buffer_size, limit, timeout_s
        self.dump = None
        self.n_chunks = 0
        logger.info(f"Predictor uses {self.device} device. Batch size: {self.batch_size}. #workers: {self.n_jobs}. "
                    f"Buffer size: {self.buffer_size}. Set limit: {self.limit}.")

    def _is_valid(self, item, score, start_id, end_id) -> bool:
        assert score >= 0
        if start_id > end_id or start_id < item.question_len + 2:
            return False
        return not (self.scores[item.item_id] > score)

    def _update_candidates(self, scores, start_ids, end_ids, start_regs, end_regs, labels, items):
        for sc, s, e, sr, er, lb, item in zip(scores, start_ids, end_ids, start_regs, end_regs, labels, items):
            if self._is_valid(item, sc, s, e):
                self.scores[item.item_id] = float(sc)
                self.candidates[item.item_id] = PredictorCandidate(int(s), int(e), float(sr), float(er), int(lb),
                                                                   float(sc))
                self.items[item.item_id] = item

    @staticmethod
    def score_batch(preds):
        """Device-side scoring → one [B, 6] float64 host array (score, start, end, sreg, ereg, cls)."""
        sp, ep = preds["start_class"].float(), preds["end_class"].float()
        s_logit, s_id = sp.max(-1)
        e_logit, e_id = ep.max(-1)
        cls_id = torch.softmax(preds["cls"].float(), -1).argmax(-1)
        score = s_logit + e_logit - (sp[:, 0] + ep[:, 0])
        out = torch.stack([score, s_id.float(), e_id.float(), preds["start_reg"].float().reshape(-1),
                           preds["end_reg"].float().reshape(-1), cls_id.float()], 1)
        return out.double().cpu().numpy()

    def decode_batch(self, preds, items) -> np.ndarray:
        """Joint valid-span decode → one [B, 6] float64 host array (score, start, end, sreg, ereg, cls).  The window
        of chunk b is its document part: from ``question_len + 2`` (the start ``_is_valid`` and ``doc_span`` use, for
        both model families) up to ``len(input_ids) − 1`` (the final separator and all padding excluded)."""
        dev = preds["start_class"].device
        lo = torch.tensor([it.question_len + 2 for it in items], dtype=torch.int32).to(dev)
        hi = torch.tensor([len(it.input_ids) - 1 for it in items], dtype=torch.int32).to(dev)
        out = ops.qa_decode(preds["start_class"], preds["end_class"], preds["cls"], preds["start_reg"],
                            preds["end_reg"], lo, hi, self.max_answer_len)
        return out.double().cpu().numpy()

    def _update_candidates_joint(self, r, items):
        for (sc, s, e, sr, er, lb), item in zip(r, items):
            if s < 0 or self.scores[item.item_id] > sc:   # empty window, or the stored score is strictly greater
                continue
            self.scores[item.item_id] = float(sc)
            self.candidates[item.item_id] = PredictorCandidate(int(s), int(e), float(sr), float(er), int(lb), float(sc))
            self.items[item.item_id] = item

    @torch.no_grad()
    def __call__(self, dataset, *, save_dump=False):
        self.model.eval()
        loader = ListDataloader(dataset, batch_size=self.batch_size, n_jobs=self.n_jobs, collate_fun=self.collate_fun,
                                buffer_size=self.buffer_size, shuffle=True, timeout_s=self.timeout_s)
        if save_dump:
            self.dump = []
        for batch_i, (inputs, _labels, items) in enumerate(loader):
            inputs = to_device(inputs, self.device)
            preds = self.model(**inputs)
            self.n_chunks += len(items)
            if self.span_decode == "joint":
                r = self.decode_batch(preds, items)
                self._update_candidates_joint(r, items)
            else:
                r = self.score_batch(preds)
                self._update_candidates(r[:, 0], r[:, 1].astype(np.int64), r[:, 2].astype(np.int64), r[:, 3], r[:, 4],
                                        r[:, 5].astype(np.int64), items)
            if save_dump:
                self.dump.append((r[:, 0], r[:, 1].astype(np.int64), r[:, 2].astype(np.int64),
                                  r[:, 5].astype(np.int64), [it.item_id for it in items]))
            if self.limit is not None and batch_i >= self.limit:
                break
        return self

    # ------------------------------------------------------------------------------------ reporting
    def predicted_text(self, item_id) -> str:
        item, c = self.items[item_id], self.candidates[item_id]
        ds, de = doc_span(item, c.start_id, c.end_id)
        if not item.t2o:
            return ""
        words = item.true_text.split()
        w0 = item.t2o[min(max(ds, 0), len(item.t2o) - 1)]
        w1 = item.t2o[min(max(de, 0), len(item.t2o) - 1)]
        return " ".join(words[w0:w1 + 1])

    def metrics(self) -> Dict[str, float]:
        n = len(self.candidates)
        if n == 0:
            return {"documents": 0, "chunks": self.n_chunks}
        acc = em = f1 = 0.0
        n_span = 0
        for k, c in self.candidates.items():
            item = self.items[k]
            acc += float(c.label == item.true_label)
            if item.true_start >= 0:
                n_span += 1
                ps, pe = doc_span(item, c.start_id, c.end_id)
                ts, te = item.true_start, item.true_end
                em += float(ps == ts and pe == te)
                inter = max(0, min(pe, te) - max(ps, ts))
                if inter > 0:
                    p, r = inter / max(pe - ps, 1), inter / max(te - ts, 1)
                    f1 += 2 * p * r / (p + r)
        return {"documents": n, "chunks": self.n_chunks, "label_accuracy": acc / n,
                "span_exact": em / max(n_span, 1), "span_f1": f1 / max(n_span, 1), "span_documents": n_span}

    def show_predictions(self, *, n_docs=None):
        for doc_i, doc_id in enumerate(self.scores.keys()):
            if n_docs is not None and doc_i >= n_docs:
                break
            doc, cand = self.items[doc_id], self.candidates[doc_id]
            logger.info(f"Text: {doc.true_text}")
            logger.info(f"Question: {doc.true_question}")
            logger.info(f"True label: {ID2LABELS[doc.true_label]}. Pred label: {ID2LABELS[cand.label]}.")
            logger.info(f"Predicted answer: {self.predicted_text(doc_id)}")

    def save_predictions(self, path: str):
        out = {str(k): {"label": ID2LABELS[c.label], "score": c.score, "start_id": c.start_id, "end_id": c.end_id,
                        "start_reg": c.start_reg, "end_reg": c.end_reg, "text": self.predicted_text(k)}
               for k, c in self.candidates.items()}
        doc = {"metrics": self.metrics()}
        if self.span_decode != "argmax":   # the argmax file stays byte for byte what it was
            doc.update(span_decode=self.span_decode, max_answer_len=self.max_answer_len)
        doc["predictions"] = out
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
