"""`dalm eval-retriever` on the MI355X path: recall / precision / hit-rate @ top-k of a (LoRA-tuned) retriever, with the
reference's parameters (dalm/eval/eval_retriever_only.py:33-196).

Every unique passage of the dataset is embedded once, every query is ranked against all of them and the metrics come from the
rank of each query's own passage (`dalm_amd.retrieval.gold_rank`): the reference's numbers for a corpus of unique passages,
exact instead of through an approximate index, plus MRR and recall at a ladder of k from the same sweep.  float16 stays the
default dtype because it is the reference's; `packed_sweep=True` (bfloat16) embeds on the live tokens only.

Deliberate differences from the reference:

1. No shuffle.  The reference shuffles its evaluation DataLoader; the metrics do not depend on the order, rows are kept in
   dataset order here.
2. A query whose retrieved scores are all below the threshold 0.0 scores 0 (the reference divides by zero).
"""
from __future__ import annotations

import logging
from argparse import Namespace
from typing import Literal, Optional

import torch

from ..models.retriever_only_base_model import AutoModelForSentenceEmbedding
from ..training.common import build_parser
from ..utils import load_dataset
from .eval_results import EvalResults
from .utils import preprocess_dataset, print_eval_results, retrieval_metrics

logger = logging.getLogger(__name__)

TORCH_DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32}


def select_dtype(torch_dtype: str) -> torch.dtype:
    if torch_dtype not in TORCH_DTYPES:
        raise ValueError(f"torch_dtype must be one of {sorted(TORCH_DTYPES)}, got {torch_dtype!r}")
    return TORCH_DTYPES[torch_dtype]


_DTYPE_HELP = "Autocast dtype: float16, bfloat16 or float32."
_BATCH_HELP = ("Rows per batch of the padded layout; a packed sweep spends the same token budget "
               "(test_batch_size * max_length) on live tokens only.")
# flag table: (name, argparse spec); names and defaults are the reference's (tests/golden/eval_signatures.json)
COMMON_FLAGS = {
    "dataset_path": dict(type=str, default=None, required=True, help="A csv file or a directory written by Dataset.save_to_disk."),
    "query_column_name": dict(type=str, default="query", help="Column holding the queries."),
    "passage_column_name": dict(type=str, default="passage", help="Column holding the passages."),
    "embed_dim": dict(type=int, default=1024, help="Width of the retriever's embeddings."),
    "retriever_name_or_path": dict(type=str, required=True, help="Retriever checkpoint directory or hub identifier."),
    "retriever_peft_model_path": dict(type=str, required=False, help="Directory of a saved retriever LoRA adapter."),
    "test_batch_size": dict(type=int, default=8, help=_BATCH_HELP),
    "device": dict(type=str, default="cuda", help="cuda or cpu."),
    "torch_dtype": dict(type=str, default="float16", help=_DTYPE_HELP),
    "top_k": dict(type=int, default=10, help="Passages retrieved per query."),
}


def flag_table(order, extra):
    """[(flag, spec)] in the given order, looked up in `extra` first and COMMON_FLAGS second."""
    return [(name, extra.get(name) or COMMON_FLAGS[name]) for name in order]


RETRIEVER_FLAGS = flag_table(
    ["dataset_path", "query_column_name", "passage_column_name", "embed_dim", "max_length", "retriever_name_or_path",
     "retriever_peft_model_path", "test_batch_size", "device", "torch_dtype", "top_k", "is_autoregressive"],
    {"max_length": dict(type=int, default=128, help="Token rows are truncated / padded to this length."),
     "is_autoregressive": dict(action="store_true", help="The retriever is a causal LM (last-token pooling).")})


def parse_args(argv=None) -> Namespace:
    return build_parser("Recall / precision / hit-rate of a retriever on a (query, passage) dataset", RETRIEVER_FLAGS).parse_args(argv)


def evaluate_retriever(
    dataset_or_path,
    retriever_name_or_path: str,
    retriever_peft_model_path: Optional[str],
    passage_column_name: str,
    query_column_name: str,
    embed_dim: int,
    max_length: int,
    test_batch_size: int = 8,
    device: str = "cuda",
    torch_dtype: Literal["float16", "bfloat16", "float32"] = "float16",
    top_k: int = 10,
    is_autoregressive: bool = False,
    *,
    model: Optional[AutoModelForSentenceEmbedding] = None,
    packed_sweep: Optional[bool] = None,
) -> EvalResults:
    """Runs retriever evaluation. See `dalm eval-retriever --help` for details on params.  packed_sweep=True embeds on the live
    tokens only (bfloat16 encoder retrievers; an error elsewhere); the default is the padded forward."""
    test_dataset = load_dataset(dataset_or_path)
    selected_torch_dtype = select_dtype(torch_dtype)
    retriever_model = model if model is not None else AutoModelForSentenceEmbedding(
        retriever_name_or_path, get_peft=False, use_bnb=False, is_autoregressive=is_autoregressive, device=device)
    processed_datasets = preprocess_dataset(test_dataset, retriever_model.tokenizer, query_column_name, passage_column_name,
                                            max_length)
    if retriever_peft_model_path is not None:
        retriever_model.attach_pre_trained_peft_layers(retriever_peft_model_path, device)
    retriever_model.eval()
    eval_results, _state = retrieval_metrics(processed_datasets, passage_column_name, retriever_model.forward, device,
                                             embed_dim, selected_torch_dtype, test_batch_size, top_k, packed_sweep=packed_sweep)
    print_eval_results(eval_results)
    return eval_results


def main() -> None:
    kw = vars(parse_args())
    kw["dataset_or_path"] = kw.pop("dataset_path")
    evaluate_retriever(**kw)


if __name__ == "__main__":
    main()
