"""One optimisation step of the RAG-end2end / retriever-only trainers.

Same work as the reference's step bodies (train_rage2e.py:429-474, train_retriever_only.py:365-379)
with the loss path on the HIP kernels:
    passage tower -> [async all-gather of P on a side stream] -> query tower -> generator ->
    fused contrastive + marginalised-CE loss (gradient of the logits written in the same pass) ->
    backward -> gradient all-reduce (W>1) -> Adam -> scheduler -> zero_grad
The reference runs the query tower first; the order is swapped so the passage all-gather overlaps
the query tower (numerically irrelevant with dropout off; changes only the dropout RNG stream).
"""
from __future__ import annotations

import contextlib
import os
from typing import Dict, Optional

import torch

from .. import streams as _streams

from .. import live_rows as _live_rows
from .. import packed as _packed
from ..fused import (GatherHandle, LocalComm, contrastive_loss, pool_l2norm, rag_e2e_loss, rag_e2e_loss_from_hidden,
                     rag_e2e_loss_packed)
from ..sharded import GradBucket, allreduce_grads
from .graphed import GraphedEncoders, GraphedTowers, GraphSets


def _advance_dropout(batch) -> None:
    """New LoRA dropout masks for this step: one device op on the current stream (captured with the step when it runs as a
    hipGraph, so every replay advances too).  See dalm_amd/models/lora_ops.py."""
    t = next((v for v in batch.values() if torch.is_tensor(v)), None)
    if t is not None and t.is_cuda:
        from ..models import lora_ops

        lora_ops.advance_dropout_seed(t.device)


def _logits_scaled(hidden: torch.Tensor, generator_model) -> torch.Tensor:
    """Hidden states that meet `lm_head.weight` WITHOUT the generator's own forward (fuse_lm_head, the packed route), for a generator
    whose forward scales its logits: GraniteForCausalLM returns `lm_head(h) / config.logits_scaling`, CohereForCausalLM
    `lm_head(h) * config.logit_scale`.  The head is linear and has no bias on these routes, so the factor goes onto h in front of
    it - exact for the released powers of two (Granite 8, 16; Cohere 0.0625), one rounding of h in its dtype otherwise.  On the
    GPU one `dalm_scale_add` launch each way."""
    cfg = getattr(generator_model, "config", None)
    div, mul = getattr(cfg, "logits_scaling", None), getattr(cfg, "logit_scale", None)
    s = (1.0 if div is None else 1.0 / float(div)) * (1.0 if mul is None else float(mul))
    if s == 1.0:
        return hidden
    from ..models import tower_ops

    if tower_ops.scale_add_supported(hidden):
        return tower_ops.scale_add(None, hidden, s)
    return hidden * s


class _StepBase:
    def __init__(self, model, optimizer, lr_scheduler, logit_scale, comm=None, autocast_dtype=None, ops=None,
                 grad_overlap: bool = True, track_grad_norm: bool = False, grad_accum: int = 1, skip_dead_rows: bool = True):
        self.model, self.optimizer, self.lr_scheduler = model, optimizer, lr_scheduler
        # padded tower calls tell the row-wise HIP kernels which rows nothing depends on (padding: dalm_amd/live_rows.py); those
        # rows are then not read and leave as zeros - same loss, same gradients, less memory traffic.  False: every row is computed
        self.skip_dead_rows = bool(skip_dead_rows)
        # global L2 norm of the (all-reduced) trainable gradients, left on the device in self.grad_norm right before
        # the optimizer consumes them - the quantity north_star's tolerance is stated on next to the loss
        self.track_grad_norm = track_grad_norm
        self.grad_norm: Optional[torch.Tensor] = None
        # --gradient_accumulation_steps N: N micro-batches (each scaled 1/N, as accelerate scales them) per optimizer /
        # scheduler step; `synced` tells the trainer whether the call it just made took that step.  The reference zeroes the
        # model's gradients after EVERY micro-batch (train_rage2e.py:474), so its update only ever sees the last one of the N -
        # the step COUNT and schedule are the reference's, the dropped micro-batches are not reproduced.
        self.grad_accum = max(1, int(grad_accum))
        self._micro = 0
        self.synced = True
        if self.grad_accum > 1:
            grad_overlap = False          # the all-reduce runs once per optimizer step, after the last micro-batch
        self.logit_scale = logit_scale
        self.comm = comm or LocalComm()
        self.autocast_dtype = autocast_dtype
        self.ops = ops
        self.side_stream = None
        if not isinstance(self.comm, LocalComm) and torch.cuda.is_available():
            self.side_stream = torch.cuda.Stream()
        self.trainable = [p for p in model.parameters() if p.requires_grad]
        # W > 1: gradients live in one flat bucket (no per-step flatten / copy-back); fp32 trainables only
        self.bucket = None
        if not isinstance(self.comm, LocalComm) and self.trainable and \
                all(p.dtype == torch.float32 for p in self.trainable) and \
                len({p.device for p in self.trainable}) == 1:
            # bucketed all-reduce issued from post-accumulate hooks while the backward is still running
            self.bucket = GradBucket(self.trainable, self.comm, overlap=None if grad_overlap else False)
        # sets of tower graphs alive at once (every set keeps its own activations between its forward and backward graphs)
        self.tower_sets_cap = int(os.environ.get("DALM_TOWER_SETS", "4"))
        self.tower_stream = None
        self.towers = None                # the tower-graph set of the current call, None: eager towers

    # autocast keeps a cache of the low-precision copies of fp32 parameters (here: the LoRA matrices).  Two towers of
    # the SAME model running on two streams would share those copies without any stream dependency - the second
    # stream can read a copy the first is still writing (seen as NaN losses under hipGraph replay at the bge-small
    # shape).  Steps that run one model on two streams therefore turn the cache off.
    autocast_cache = True

    def _autocast(self):
        if self.autocast_dtype is None:
            return contextlib.nullcontext()
        return torch.autocast("cuda", dtype=self.autocast_dtype, cache_enabled=self.autocast_cache)

    def _retrieve_pair(self, batch, q_prefix: str, p_prefix: str):
        """Queries AND passages through the encoder in one packed call (one rank: there is no passage all-gather to overlap with
        the query tower) - or None when the batch / model does not allow it."""
        m = self.model
        enc = getattr(m, "retriever_model", None) or getattr(m, "model", None)
        if (not isinstance(self.comm, LocalComm)
                or f"{q_prefix}_pack_rows" not in batch or f"{p_prefix}_pack_rows" not in batch
                or not self._retriever_packable(enc, batch, q_prefix) or not self._retriever_packable(enc, batch, p_prefix)):
            return None
        q = (batch[f"{q_prefix}_input_ids"], batch[f"{q_prefix}_attention_mask"], batch[f"{q_prefix}_pack_rows"], batch[f"{q_prefix}_pack_cu"])
        p = (batch[f"{p_prefix}_input_ids"], batch[f"{p_prefix}_attention_mask"], batch[f"{p_prefix}_pack_rows"], batch[f"{p_prefix}_pack_cu"])
        if self._causal_retriever():                  # row lists of a `last_column` plan: decoder stack + last-token pool
            return _packed.causal_retrieval_embed_pair(enc, p, q, m.normalize)
        hp, hq = _packed.retrieval_hidden_pair(enc, p, q)
        return pool_l2norm(hp, p[1], m.normalize), pool_l2norm(hq, q[1], m.normalize)

    def _causal_retriever(self) -> bool:
        m = self.model
        return bool(getattr(m, "retriever_is_autoregressive", getattr(m, "is_autoregressive", False)))

    def _retriever_packable(self, enc, batch, prefix: str) -> bool:
        """The retriever can run on the packed rows of input `prefix`: it reads the descriptor (`attention_is_packable`); a causal
        LM must be one whose decoder stack is called directly, and its row lists must keep the pooled column (a `last_column`
        plan, packed.*_GROUPS_CAUSAL, which leaves the marker key) - a plan of the live tokens alone goes the padded way."""
        from ..models.rag_e2e_base_model import decoder_only

        if not _packed.attention_is_packable(enc):
            return False
        return not self._causal_retriever() or (decoder_only(enc, int(batch[f"{prefix}_input_ids"].shape[1]))
                                                and f"{prefix}_{_packed.LAST_COLUMN_KEY}" in batch)

    def _embed_one(self, enc, batch, prefix: str, padded_call):
        """One retriever input; packed when the batch carries its row list and the model allows it, else `padded_call(ids, mask)`
        under its row liveness."""
        m = self.model
        causal = self._causal_retriever()
        ids, mask = batch[f"{prefix}_input_ids"], batch[f"{prefix}_attention_mask"]
        rows, cu = batch.get(f"{prefix}_pack_rows"), batch.get(f"{prefix}_pack_cu")
        if rows is not None and self._retriever_packable(enc, batch, prefix):
            if causal:
                return _packed.causal_retrieval_embed(enc, ids, mask, rows, cu, m.normalize)
            return pool_l2norm(_packed.retrieval_hidden(enc, ids, mask, rows, cu), mask, m.normalize)
        with _live_rows.tower_call(mask, False, self.skip_dead_rows, last_column=causal):
            return padded_call(ids, mask)

    def _beside(self, on_tower, on_main, main_first: bool = False):
        """Run `on_tower()` on the tower stream beside `on_main()` on the current stream (`main_first`: enqueue `on_main` first);
        returns both results once the current stream has joined the tower stream.  The tensors `on_tower` returns (and the
        results of its GatherHandles) are recorded on the current stream, which consumes them."""
        cur = torch.cuda.current_stream()
        self.tower_stream.wait_stream(cur)
        if main_first:
            main = on_main()
        with torch.cuda.stream(self.tower_stream):
            tower = on_tower()
        if not main_first:
            main = on_main()
        cur.wait_stream(self.tower_stream)
        for t in tower:
            t = getattr(t, "result", t)
            if t is not None and t.is_cuda:
                t.record_stream(cur)
        return tower, main

    def _finish(self, loss: torch.Tensor) -> torch.Tensor:
        if self.grad_accum > 1:
            (loss / self.grad_accum).backward()
            self._micro += 1
            self.synced = self._micro % self.grad_accum == 0
            if not self.synced:
                return loss.detach()
        else:
            loss.backward()
        return self._apply(loss)

    def flush(self) -> bool:
        """End of an epoch with micro-batches still pending: take the optimizer step on what has accumulated (accelerate
        syncs on the last batch of the dataloader in the same way).  True when a step was taken."""
        if self.grad_accum > 1 and self._micro % self.grad_accum != 0:
            self._micro = 0
            self.synced = True
            self._apply(None)
            return True
        return False

    def _apply(self, loss: Optional[torch.Tensor]):
        if self.bucket is not None:
            self.bucket.all_reduce()
        else:
            allreduce_grads(self.trainable, self.comm)
        if self.track_grad_norm:
            if self.bucket is not None:
                self.grad_norm = torch.linalg.vector_norm(self.bucket.flat)
            else:
                grads = [p.grad for p in self.trainable if p.grad is not None]
                self.grad_norm = torch.linalg.vector_norm(torch.stack(torch._foreach_norm(grads)))
        self.optimizer.step()
        if self.lr_scheduler is not None:
            self.lr_scheduler.step()
        if self.bucket is not None:
            self.bucket.zero()
        else:
            self.model.zero_grad(set_to_none=True)
        return loss.detach() if loss is not None else None


class RagE2EStep(_StepBase):
    """batch keys as produced by preprocess_dataset (rag_e2e_dataloader_utils.py:56-68)."""

    def __init__(self, *a, inplace_grad: bool = True, overlap_towers: bool = True, fuse_lm_head: bool = False,
                 lm_head_chunk: Optional[int] = None, graph_towers: bool = False, graph_after: int = 2, **kw):
        super().__init__(*a, **kw)
        self.inplace_grad = inplace_grad
        # run the decoder without its lm_head and let the loss consume the hidden states chunk by chunk -
        # the [B,Tg,V] logits and their gradient never exist (frozen bf16 head: the library's own MFMA kernels end to end,
        # fused._lm_head_train_kernel).  True / False, or "auto": fused whenever the materialised logits of a batch would exceed
        # DALM_LOGITS_BUDGET_MB (default 1024 MB; decided per batch shape, _resolve_fuse - the BASELINE batches stay below it,
        # where the materialised path measures ~1 ms per step faster: profiles/r05_lm_head_train_kernels_vs_library.txt)
        self.fuse_lm_head = fuse_lm_head
        self._fuse_auto: Optional[dict] = {} if fuse_lm_head == "auto" else None
        self.logits_budget_mb = float(os.environ.get("DALM_LOGITS_BUDGET_MB", "1024"))
        self.lm_head_chunk = lm_head_chunk
        # W > 1: graph the towers (fwd + bwd), keep collectives / loss / optimizer eager (GraphedTowers); one set per batch shape
        # (packed batches: per row-count combination), the first `graph_after` real steps eager (library warm-up, as GraphedStep)
        self.graph_towers = graph_towers and torch.cuda.is_available()
        self._tower_sets = GraphSets(cap=self.tower_sets_cap, skip=graph_after, what="the towers")
        self.aux: Dict[str, torch.Tensor] = {}
        # the two retriever towers are many small kernels (3204 tokens through BERT) and are independent of
        # the generator until the loss: run them on their own HIP stream so they fill the gaps between the
        # generator's large GEMMs; autograd replays each backward on its forward stream, so the backward
        # overlaps the same way
        self.tower_stream = _streams.tower_stream() if (overlap_towers and torch.cuda.is_available()) else None

    towers_failed = property(lambda self: self._tower_sets.failed)

    def _tower_graphs(self, batch) -> Optional[GraphedTowers]:
        """The tower-graph set of this batch's shape, built on first sight; None: the towers launch eagerly."""
        if not self.graph_towers:
            return None
        m = self.model
        key = GraphedTowers.key_of(batch)
        if key not in self._tower_sets.built and any(k in batch for k in GraphedTowers.PACK_KEYS) and not (
                GraphedTowers.is_packed(batch) and _packed.attention_is_packable(m.generator_model)
                and _packed.attention_is_packable(m.retriever_model)):
            key = None              # row lists for some towers only, or a model the packed call cannot serve: eager
        return self._tower_sets.get(
            key, lambda: GraphedTowers(self.model, self.autocast_dtype, batch, hidden_only=self.fuse_lm_head,
                                       skip_dead_rows=self.skip_dead_rows))

    def _gather(self, emb):
        """Start the all-gather of an embedding matrix early on the side stream (overlaps the other tower)."""
        return GatherHandle(emb.float(), self.comm, self.side_stream)

    def _retrieve(self, batch, side: str, towers: Optional[GraphedTowers]):
        """One retriever tower call; on the PACKED rows when the batch carries their list (`retriever_{side}_pack_rows` /
        `_pack_cu`, dalm_amd/packed.py) - same embeddings, the padding never enters the encoder."""
        if towers is not None:
            return getattr(towers, side)(*towers.args(batch, side))
        return self._embed_one(self.model.retriever_model, batch, f"retriever_{side}", lambda ids, mask: self.model("retrieval", ids, mask))

    def _towers(self, batch, towers: Optional[GraphedTowers]):
        pair = self._retrieve_pair(batch, "retriever_query", "retriever_passage") if towers is None else None
        if pair is not None:
            p_emb, q_emb = pair
            return p_emb, q_emb, self._gather(p_emb), self._gather(q_emb)
        p_emb = self._retrieve(batch, "passage", towers)
        p_gather = self._gather(p_emb)
        q_emb = self._retrieve(batch, "query", towers)
        return p_emb, q_emb, p_gather, self._gather(q_emb)

    def _packed_generator(self, batch, towers: Optional[GraphedTowers] = None) -> bool:
        if towers is not None:
            return towers.packed
        return "generator_pack_rows" in batch and _packed.attention_is_packable(self.model.generator_model)

    def _generator(self, batch, towers: Optional[GraphedTowers], packed: bool):
        """Logits; or the final hidden states (fuse_lm_head), of the live rows only, [n, H], when `packed`."""
        if towers is not None:
            return towers.generator(*towers.args(batch, "generator"))
        ids, mask = batch["generator_input_input_ids"], batch["generator_input_attention_mask"]
        gm = self.model.generator_model
        if packed:
            return _packed.generator_hidden(gm, ids, mask, batch["generator_pack_rows"], batch["generator_pack_cu"])
        with _live_rows.tower_call(mask, True, self.skip_dead_rows):
            if self.fuse_lm_head:
                return gm.base_model(input_ids=ids, attention_mask=mask, use_cache=False)[0]
            return self.model("generation", ids, mask)

    def _resolve_fuse(self, batch) -> None:
        """fuse_lm_head="auto": decided PER BATCH SHAPE (cached) - a later, longer batch that exceeds DALM_LOGITS_BUDGET_MB takes
        the logits-free path even when the first batch was small, and a large first batch does not lock the slower path in
        (ADVICE r5).  Inside a hipGraph the decision is part of the captured shape."""
        if self._fuse_auto is None:
            return
        ids = batch["generator_input_input_ids"]
        key = tuple(ids.shape)
        if key not in self._fuse_auto:
            head = self.model.generator_model.get_output_embeddings()
            el = 2 if self.autocast_dtype in (torch.bfloat16, torch.float16) or head.weight.dtype != torch.float32 else 4
            mb = ids.shape[0] * ids.shape[1] * head.weight.shape[0] * el / 2 ** 20
            self._fuse_auto[key] = bool(mb > self.logits_budget_mb and getattr(head, "bias", None) is None)
        self.fuse_lm_head = self._fuse_auto[key]

    def _loss(self, batch, packed: bool, out, p_emb, q_emb, p_gather, q_gather):
        """The HIP loss on the generator's output: logits, the hidden states (fuse_lm_head) or the packed rows' hidden states."""
        ids, mask = batch["generator_input_input_ids"], batch["generator_input_attention_mask"]
        qp_len = batch["query_passage_input_len"]
        kw = dict(comm=self.comm, ops=self.ops, q_gather=q_gather, p_gather=p_gather, aux=self.aux)
        if not (packed or self.fuse_lm_head):
            return rag_e2e_loss(q_emb, p_emb, out, ids, mask, qp_len, self.logit_scale, inplace_grad=self.inplace_grad, **kw)
        if self.autocast_dtype is not None and out.dtype != self.autocast_dtype:
            # the reference's lm_head runs INSIDE the autocast'ed model forward: nn.Linear casts its input to the autocast dtype.
            # A decoder whose final norm is an nn.LayerNorm (Falcon: autocast runs layer_norm in f32) hands back f32 hidden
            # states - without this cast the head GEMMs of the from-hidden paths ran in f32 (2.2 ms each at cfg5)
            out = out.to(self.autocast_dtype)
        head = self.model.generator_model.get_output_embeddings()
        if getattr(head, "bias", None) is not None:
            raise NotImplementedError("the packed generator path and fuse_lm_head need a bias-free lm_head")
        out = _logits_scaled(out, self.model.generator_model)
        if packed:
            labels, weights = _packed.packed_labels(ids, mask, batch["generator_pack_rows"])
            return rag_e2e_loss_packed(q_emb, p_emb, out, head.weight, labels, weights, mask, qp_len, self.logit_scale, **kw)
        return rag_e2e_loss_from_hidden(q_emb, p_emb, out, head.weight, ids, mask, qp_len, self.logit_scale,
                                        chunk_samples=self.lm_head_chunk, live_rows=batch.get("generator_live_rows"), **kw)

    def __call__(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        self._resolve_fuse(batch)
        self.towers = towers = self._tower_graphs(batch)
        packed = self._packed_generator(batch, towers)
        _advance_dropout(batch)
        with self._autocast():
            if self.tower_stream is None:
                embs = self._towers(batch, towers)
                out = self._generator(batch, towers, packed)
            else:
                # with graphs: graph launches cost host milliseconds each - get the generator's big graph onto the GPU first,
                # then feed the small tower graphs into the gaps (the tower stream only waits for what was on the main stream
                # BEFORE this point)
                embs, out = self._beside(lambda: self._towers(batch, towers), lambda: self._generator(batch, towers, packed),
                                         main_first=towers is not None)
        return self._finish(self._loss(batch, packed, out, *embs))


class RetrieverStep(_StepBase):
    """batch keys as produced by retriever_only_dataloader_utils.preprocess_dataset."""

    def __init__(self, *a, overlap_towers: bool = True, graph_towers: bool = False, graph_after: int = 2, **kw):
        super().__init__(*a, **kw)
        # the query pass (Tq = 50) is small next to the passage pass (Tp = 128): run it on its own stream
        self.tower_stream = _streams.tower_stream() if (overlap_towers and torch.cuda.is_available()) else None
        self.autocast_cache = self.tower_stream is None   # one model on two streams: no shared cast cache
        # the two encoder calls as single-stream hipGraphs (GraphedEncoders), loss / optimizer / collectives eager: padded batches
        # only (the packed batch goes through the encoder in ONE call - a whole-step graph of that is a single stream already)
        # ONE RANK ONLY (LocalComm): next to the W > 1 gradient bucket the second replay of a set gave an infinite gradient norm
        self.graph_towers = (graph_towers and torch.cuda.is_available() and self.tower_stream is not None
                             and isinstance(self.comm, LocalComm))
        self._encoder_sets = GraphSets(cap=self.tower_sets_cap, skip=graph_after, what="the encoder calls")

    towers_failed = property(lambda self: self._encoder_sets.failed)

    def _embed(self, batch, side: str):
        """One encoder call; on the PACKED rows when the batch carries their list (`{side}_pack_rows` / `_pack_cu`); through the
        graphed encoders when the call has a set."""
        if self.towers is not None:
            return getattr(self.towers, side)(batch[f"{side}_input_ids"], batch[f"{side}_attention_mask"])
        return self._embed_one(self.model.model, batch, side, self.model)

    def _embed_gather(self, batch, side: str):
        emb = self._embed(batch, side)
        return emb, GatherHandle(emb.float(), self.comm, self.side_stream)

    def __call__(self, batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        self.towers = None
        if self.graph_towers:
            key = GraphedEncoders.key_of(batch) if "query_pack_rows" not in batch else None
            self.towers = self._encoder_sets.get(
                key, lambda: GraphedEncoders(self.model, self.autocast_dtype, batch, skip_dead_rows=self.skip_dead_rows))
        _advance_dropout(batch)
        pair = None
        if self.towers is None:
            with self._autocast():
                pair = self._retrieve_pair(batch, "query", "passage")
        if pair is not None:             # packed, one rank: both inputs through the encoder in ONE call, one stream
            p_emb, q_emb = pair
            q_gather = GatherHandle(q_emb.float(), self.comm, self.side_stream)
            p_gather = GatherHandle(p_emb.float(), self.comm, self.side_stream)
        else:
            # graphed encoder calls run outside autocast (each graph carries its own)
            with self._autocast() if self.towers is None else contextlib.nullcontext():
                if self.tower_stream is not None:
                    (q_emb, q_gather), (p_emb, p_gather) = self._beside(lambda: self._embed_gather(batch, "query"),
                                                                        lambda: self._embed_gather(batch, "passage"))
                else:
                    p_emb, p_gather = self._embed_gather(batch, "passage")
                    q_emb, q_gather = self._embed_gather(batch, "query")
        loss = contrastive_loss(q_emb, p_emb, self.logit_scale, comm=self.comm, ops=self.ops, q_gather=q_gather,
                                p_gather=p_gather)
        return self._finish(loss)
