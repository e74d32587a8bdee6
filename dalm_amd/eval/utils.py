"""Embedding sweep and metric helpers of the evaluation drivers, with the reference's names (dalm/eval/utils.py) so callers
can swap imports.  What differs underneath:

* embeddings stay on the device as one f32 [N, D] tensor (the reference moves every batch to a host numpy array);
* the search is exact (`dalm_amd.retrieval`) instead of an hnswlib index;
* with `packed_sweep=True` an encoder retriever in bfloat16 is swept in the packed layout: token counts are known on the host
  from tokenisation, rows are sorted by length and cut into batches by a live-token budget, the encoder runs once per batch on
  the live tokens only and `dalm_pool_l2norm_packed_fwd` pools straight from the packed rows into the batch's slice of the
  result.  It is opt-in (PACKED_SWEEP_DEFAULT): the measurement on record has it slower than the padded forward, see DESIGN.md
  section 9a.  Everything else - and bfloat16 by default - takes the padded forward batch by batch.
"""
from __future__ import annotations

import logging
from typing import Any, Callable, Dict, List, Optional, Tuple, Union

import torch

from .. import packed
from ..ops import default_ops
from ..retrieval import (ExactIndex, calculate_precision_recall, construct_search_index,  # noqa: F401  (re-exported)
                         get_nearest_neighbours)
from .eval_results import EvalResults

logger = logging.getLogger(__name__)

RECALL_LADDER = (1, 5, 10, 20, 50, 100)
PACKED_SWEEP_DEFAULT = False      # opt-in: the one measurement on record (profiles/eval_bench.txt) has it slower than the padded forward
PACKED_POOL_LAST_MAX_WIDTH = 8192    # dalm_pool_last_packed_fwd (causal-LM retrievers)
PACKED_POOL_MAX_WIDTH = 1024     # dalm_pool_l2norm_packed_fwd on f32 rows (the final LayerNorm under autocast returns f32)


def preprocess_function(examples, retriever_tokenizer, query_column_name: str = "query", passage_column_name: str = "passage",
                        max_length: int = 128) -> Dict[str, Any]:
    """Tokenised columns `retriever_query_*` / `retriever_passage_*` of a batch of rows, padded to `max_length`."""
    out: Dict[str, Any] = {}
    for prefix, column in (("retriever_query", query_column_name), ("retriever_passage", passage_column_name)):
        enc = retriever_tokenizer(examples[column], padding="max_length", max_length=max_length, truncation=True)
        out.update({f"{prefix}_{field}": values for field, values in enc.items()})
    return out


def preprocess_dataset(dataset, tokenizer, query_column_name: str, passage_column_name: str, max_length: int):
    """Runs the tokenizer on the dataset, returning the tokenized columns next to the original ones."""
    return dataset.map(
        lambda example: preprocess_function(example, tokenizer, query_column_name=query_column_name,
                                            passage_column_name=passage_column_name, max_length=max_length),
        batched=True, desc="Running tokenizer on dataset", num_proc=4 if len(dataset) >= 20000 else None)


def filter_unique_passages(dataset, passage_column_name: str, *, return_gold_index: bool = False):
    """The rows that hold the FIRST occurrence of each passage text, in dataset order (as the reference filters).
    return_gold_index=True also yields, for every row of `dataset`, the position of its passage in that unique list: the
    corpus row of the row's gold passage."""
    first: Dict[Any, int] = {}
    keep: List[int] = []
    gold: List[int] = []
    for i, text in enumerate(dataset[passage_column_name]):
        at = first.get(text)
        if at is None:
            at = first[text] = len(keep)
            keep.append(i)
        gold.append(at)
    unique = dataset.select(keep)
    return (unique, gold) if return_gold_index else unique


def mixed_collate_fn(batch: List[Dict[str, Any]]) -> Dict[str, Union[torch.Tensor, List[str]]]:
    """Collate that stacks numeric columns and keeps text (or None) columns as plain lists, which torch's default collate
    cannot batch.  The first sample decides a column's kind."""
    def is_text(v) -> bool:
        return v is None or isinstance(v, str)

    return {key: [row[key] for row in batch] if is_text(first) else torch.stack([torch.as_tensor(row[key]) for row in batch])
            for key, first in batch[0].items()}


def get_retriever_embeddings(forward_fn: Callable[[torch.Tensor, torch.Tensor], torch.Tensor], device: str,
                             retriever_input_ids: torch.Tensor, retriever_attention_masks: torch.Tensor) -> torch.Tensor:
    """Runs the forward function on the inputs and masks; the f32 embeddings stay on the device."""
    return forward_fn(retriever_input_ids.to(device), retriever_attention_masks.to(device)).detach().float()


def _autocast(device: str, torch_dtype: torch.dtype):
    kind = torch.device(device).type
    return torch.autocast(device_type=kind, dtype=torch_dtype, enabled=torch_dtype in (torch.float16, torch.bfloat16))


def _packable_encoder(forward_fn, torch_dtype: torch.dtype, device: str, T: Optional[int] = None):
    """(encoder module, autoregressive) behind `forward_fn` (the bound `forward` / `retrieval_forward` of this package's two
    model classes) when the packed sweep can run it, else None.  An autoregressive owner qualifies when the sweep can call its
    decoder stack directly (models.rag_e2e_base_model.decoder_only; the model classes' own padded call stays the reference's):
    the sweep then keeps the pooled column in its plans and pools with
    `dalm_pool_last_packed_fwd`, whose width limit is 8192, not PACKED_POOL_MAX_WIDTH."""
    owner = getattr(forward_fn, "__self__", None)
    if owner is None or torch_dtype != torch.bfloat16 or torch.device(device).type != "cuda":
        return None
    name = getattr(forward_fn, "__name__", "")
    if name == "forward" and hasattr(owner, "is_autoregressive") and hasattr(owner, "model"):
        enc, autoregressive = owner.model, owner.is_autoregressive
    elif name == "retrieval_forward" and hasattr(owner, "retriever_model"):
        enc, autoregressive = owner.retriever_model, owner.retriever_is_autoregressive
    else:
        return None
    if not getattr(owner, "normalize", False) or not packed.attention_is_packable(enc):
        return None
    if autoregressive:
        from ..models.rag_e2e_base_model import decoder_only

        width = getattr(enc.config, "hidden_size", 1 << 30)
        return (enc, True) if decoder_only(enc, T) and width <= PACKED_POOL_LAST_MAX_WIDTH and width % 8 == 0 else None
    if getattr(enc.config, "hidden_size", 1 << 30) > PACKED_POOL_MAX_WIDTH:       # wider rows: the padded pooling kernel
        return None
    return enc, False


def token_budget_batches(lengths: torch.Tensor, budget: int) -> Tuple[torch.Tensor, List[Tuple[int, int]]]:
    """HOST side.  (order, [(a, b), ...]): rows sorted by token count (stable) and cut into consecutive ranges of the sorted
    order holding at most `budget` live tokens each (a single longer row forms its own range)."""
    order = torch.argsort(lengths, stable=True)
    sorted_len = lengths[order].tolist()
    cuts: List[Tuple[int, int]] = []
    a, tokens = 0, 0
    for i, n in enumerate(sorted_len):
        if i > a and tokens + n > budget:
            cuts.append((a, i))
            a, tokens = i, 0
        tokens += n
    if a < len(sorted_len):
        cuts.append((a, len(sorted_len)))
    return order, cuts


def _column(dataset, name: str) -> torch.Tensor:
    return torch.as_tensor(dataset.with_format("numpy", columns=[name])[:][name]).to(torch.int64)     # one stacked [N, T] array


def embed_dataset(dataset, prefix: str, forward_fn, device: str, torch_dtype: torch.dtype, batch_size: int, *,
                  packed_sweep: Optional[bool] = None) -> torch.Tensor:
    """f32 [len(dataset), D] device tensor of the embeddings of the tokenised column pair `<prefix>_input_ids` /
    `<prefix>_attention_mask`, in dataset order.  `batch_size` counts rows of the padded layout: the packed sweep turns it
    into a budget of batch_size * max_length live tokens per encoder call.
    packed_sweep: None = PACKED_SWEEP_DEFAULT, False = padded forward, True = packed sweep, or an error where it cannot run."""
    ids, mask = _column(dataset, f"{prefix}_input_ids"), _column(dataset, f"{prefix}_attention_mask")
    N, T = ids.shape
    if N == 0:
        raise ValueError("nothing to embed: the dataset has no rows")
    enc, causal = None, False
    if packed_sweep or (packed_sweep is None and PACKED_SWEEP_DEFAULT):
        found = _packable_encoder(forward_fn, torch_dtype, device, T)
        if found is not None and bool(((mask == 0) | (mask == 1)).all()):
            enc, causal = found
        if enc is None and packed_sweep:
            raise ValueError("packed_sweep=True needs bfloat16 on a GPU, 0/1 masks and a retriever of this package with packable "
                             f"attention: an encoder of width <= {PACKED_POOL_MAX_WIDTH}, or a causal LM whose decoder stack is "
                             f"called directly, of width <= {PACKED_POOL_LAST_MAX_WIDTH}")
    out: Optional[torch.Tensor] = None
    if enc is None:
        for a in range(0, N, batch_size):
            with torch.no_grad(), _autocast(device, torch_dtype):
                e = get_retriever_embeddings(forward_fn, device, ids[a:a + batch_size], mask[a:a + batch_size])
            if out is None:
                out = torch.empty((N, e.shape[1]), device=e.device, dtype=torch.float32)
            out[a:a + batch_size] = e
        assert out is not None
        return out
    ops = default_ops()
    kept = mask != 0
    if causal:                                    # the pooled column stays in every plan (packed.pack_plan, last_column)
        kept = kept.clone()
        kept[:, -1] = True
    order, cuts = token_budget_batches(kept.sum(dim=1), batch_size * T)
    for a, b in cuts:
        idx = order[a:b]
        ids_b, mask_b = ids[idx], mask[idx]
        rows, cu = packed.pack_plan(mask_b, shifted=False, last_column=causal)
        ids_p, pos, desc, _valid = packed.packed_inputs(ids_b.to(device), mask_b.to(device), rows.to(device), cu.to(device),
                                                        causal=causal, model=enc)
        with torch.no_grad(), _autocast(device, torch_dtype):
            if causal:
                h = enc.base_model(input_ids=ids_p, attention_mask=desc, position_ids=pos, use_cache=False)[0][0]
            else:
                h = enc(input_ids=ids_p, attention_mask=desc, position_ids=pos)[0][0]             # [n, D]
        if out is None:
            out = torch.empty((N, h.shape[1]), device=h.device, dtype=torch.float32)
        if causal:
            ops.pool_last_packed_fwd(h, packed.packed_of(desc).cu, nseq_out=b - a, normalize=True, out=out[a:b])
        else:
            ops.pool_packed_fwd(h, packed.packed_of(desc).cu, nseq_out=b - a, out=out[a:b])       # sorted order
    assert out is not None
    return torch.empty_like(out).index_copy_(0, order.to(out.device), out)                        # back to dataset order


def _embed_unique_passages(unique, forward_fn, device: str, embed_dim: int, torch_dtype: torch.dtype, batch_size: int,
                           packed_sweep: Optional[bool] = None):
    logger.info(f"Starting to generate passage embeddings (Number of passages: {len(unique)})")
    embs = embed_dataset(unique, "retriever_passage", forward_fn, device, torch_dtype, batch_size, packed_sweep=packed_sweep)
    if embs.shape[1] != embed_dim:
        raise ValueError(f"embed_dim={embed_dim} but the retriever produces embeddings of width {embs.shape[1]}")
    return embs


def get_passage_embeddings(passage_dataset, passage_column_name: str,
                           forward_fn: Callable[[torch.Tensor, torch.Tensor], torch.Tensor], device: str, embed_dim: int,
                           torch_dtype: torch.dtype, batch_size: int):
    """(unique passage dataset, f32 [N, embed_dim] device tensor of its embeddings)."""
    unique = filter_unique_passages(passage_dataset, passage_column_name)
    return unique, _embed_unique_passages(unique, forward_fn, device, embed_dim, torch_dtype, batch_size)


def evaluate_retriever_on_batch(batch, passage_column_name: str, forward_fn, search_index: ExactIndex, torch_dtype: torch.dtype,
                                device: str, top_k: int, id_to_passage: Dict[int, str]):
    """The reference's per-batch loop on the exact index: (list[precision], list[recall], total hit, list[top passage]).
    The drivers of this package do not call it (they rank the whole query set in one sweep, `retrieval_metrics`); it is
    kept for callers of the reference's function.  A query whose retrieved scores are all negative scores 0 / 0 and has no
    top passage (None) - the reference divides by zero there."""
    with torch.no_grad(), _autocast(device, torch_dtype):
        query_embeddings = get_retriever_embeddings(forward_fn, device, batch["retriever_query_input_ids"],
                                                    batch["retriever_query_attention_mask"])
    search_results = get_nearest_neighbours(top_k, search_index, query_embeddings, id_to_passage, threshold=0.0)
    correct_passages = batch[passage_column_name]
    batch_precision, batch_recall, total_hit, top_passages = [], [], 0, []
    for i, result in enumerate(search_results):
        retrieved = [passage for passage, _score in result]
        top_passages.append(retrieved[0] if retrieved else None)
        precision, recall = calculate_precision_recall(retrieved, [correct_passages[i]]) if retrieved else (0.0, 0.0)
        batch_precision.append(precision)
        batch_recall.append(recall)
        total_hit += int(correct_passages[i] in retrieved)
    return batch_precision, batch_recall, total_hit, top_passages


def calc_eval_results(total_examples: int, precisions: List[float], recalls: List[float], total_hit: int) -> EvalResults:
    return EvalResults(total_examples=total_examples, recall=sum(recalls) / total_examples,
                       precision=sum(precisions) / total_examples, hit_rate=total_hit / float(total_examples))


def print_eval_results(eval_results: EvalResults) -> None:
    logger.info("Retriever results:")
    logger.info(f"Recall: {eval_results.recall}")
    logger.info(f"Precision: {eval_results.precision}")
    logger.info(f"Hit Rate: {eval_results.hit_rate}")
    if eval_results.mrr is not None:
        logger.info(f"MRR: {eval_results.mrr}")
    if eval_results.recall_at:
        logger.info("Recall@k: " + ", ".join(f"{k}: {v:.4f}" for k, v in sorted(eval_results.recall_at.items())))
    logger.info("*************")


def retrieval_metrics(processed_datasets, passage_column_name: str, forward_fn, device: str, embed_dim: int,
                      torch_dtype: torch.dtype, test_batch_size: int, top_k: int, threshold: float = 0.0, *,
                      packed_sweep: Optional[bool] = None):
    """What both drivers share: unique passages -> corpus embeddings, query embeddings, one rank sweep, metrics.
    Returns (EvalResults, state) with state = {"unique", "gold", "passage_embeddings", "query_embeddings", "rank", "n_ge"}."""
    from ..retrieval import gold_rank, metrics_from_rank

    unique, gold = filter_unique_passages(processed_datasets, passage_column_name, return_gold_index=True)
    passage_embs = _embed_unique_passages(unique, forward_fn, device, embed_dim, torch_dtype, test_batch_size, packed_sweep)
    logger.info("Evaluation start")
    query_embs = embed_dataset(processed_datasets, "retriever_query", forward_fn, device, torch_dtype, test_batch_size,
                               packed_sweep=packed_sweep)
    rank, n_ge, _score = gold_rank(query_embs, passage_embs, torch.tensor(gold, dtype=torch.int64), threshold=threshold)
    rank, n_ge = rank.cpu(), n_ge.cpu()
    ladder = sorted({k for k in RECALL_LADDER if k <= len(unique)} | {int(top_k)})
    per_k = {m["top_k"]: m for m in metrics_from_rank(rank, n_ge, ladder)}
    at = per_k[int(top_k)]
    results = EvalResults(total_examples=len(processed_datasets), recall=at["recall"], precision=at["precision"],
                          hit_rate=at["hit_rate"], mrr=at["mrr"], recall_at={k: m["recall"] for k, m in per_k.items()})
    state = {"unique": unique, "gold": gold, "passage_embeddings": passage_embs, "query_embeddings": query_embs,
             "rank": rank, "n_ge": n_ge}
    return results, state
