"""Result record of the two evaluation drivers (dalm/eval/eval_results.py, plus what the rank sweep gives for free)."""
from __future__ import annotations

from typing import Dict, Optional

from pydantic import BaseModel


class EvalResults(BaseModel):
    total_examples: int
    recall: float
    precision: float
    hit_rate: float
    # from the same sweep as the three above: mean reciprocal rank of the gold passage, and recall at a ladder of k
    mrr: Optional[float] = None
    recall_at: Optional[Dict[int, float]] = None
