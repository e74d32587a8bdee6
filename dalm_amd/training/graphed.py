"""hipGraph capture of a whole optimisation step (towers + HIP loss path + backward + Adam).

The eager step issues ~10k kernel launches (HF eager elementwise ops dominate the count); replaying
them from one captured graph removes the host launch path from the critical loop.  Static-shape
batches are copied into captured input buffers; a batch with another shape (the partial last batch)
runs eagerly.  Requirements: optimizer built with `capturable=True` and a tensor `lr`
(`make_capturable_adam`), the LR scheduler stepped outside the graph (it `fill_`s the lr tensor).
Single-GPU only for now: with W > 1 the step stays eager (RCCL inside a captured step is left for a
later round).
"""
from __future__ import annotations

import contextlib
import gc
import warnings
from typing import Callable, Dict, Hashable, Optional, Tuple

import torch


def make_capturable_adam(params, lr: float, device) -> torch.optim.Adam:
    return torch.optim.Adam(params, lr=torch.tensor(float(lr), device=device), fused=True, capturable=True)


def init_adam_state(optimizer: torch.optim.Adam) -> None:
    """Materialise Adam's lazily created state (step, exp_avg, exp_avg_sq) BEFORE a capture.

    If the first optimizer.step() happens inside the capture, the zero-initialisation of the state is
    recorded in the graph and every replay resets the moments - the first replay is right, all later
    ones are wrong (caught by tests/test_step_parity_gpu.py)."""
    for group in optimizer.param_groups:
        for p in group["params"]:
            if not p.requires_grad or len(optimizer.state[p]) != 0:
                continue
            st = optimizer.state[p]
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if group.get("amsgrad"):
                st["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)


class TensorLRScheduler:
    """Drives the tensor-valued lr of a capturable optimizer from an ordinary scheduler.

    The scheduler is built on a shadow optimizer with a FLOAT lr (schedulers keep `initial_lr` by
    reference, so attaching one directly to a tensor lr compounds the decay: lr_t = lr_{t-1} * f(t));
    after every shadow step the float is written into the real optimizer's lr tensor with fill_(),
    which a captured graph picks up on its next replay."""

    def __init__(self, optimizer, lr: float, factory: Callable[[torch.optim.Optimizer], object]):
        self.optimizer = optimizer
        self._shadow = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=float(lr))
        self.scheduler = factory(self._shadow)
        self._push()

    def _push(self) -> None:
        lr = float(self._shadow.param_groups[0]["lr"])
        for g in self.optimizer.param_groups:
            if torch.is_tensor(g["lr"]):
                g["lr"].fill_(lr)
            else:
                g["lr"] = lr

    def step(self) -> None:
        self._shadow.step()
        self.scheduler.step()
        self._push()

    def get_last_lr(self):
        return self.scheduler.get_last_lr()

    def state_dict(self):
        return self.scheduler.state_dict()

    def load_state_dict(self, sd) -> None:
        self.scheduler.load_state_dict(sd)
        # LambdaLR.load_state_dict restores the schedule position but not the shadow optimizer's lr:
        # take it from the restored schedule, otherwise _push() would overwrite the (correct) lr that
        # optimizer.load_state_dict has just restored with the shadow's construction-time value
        last = sd.get("_last_lr") or self.scheduler.get_last_lr()
        for g, lr in zip(self._shadow.param_groups, last):
            g["lr"] = float(lr)
        self._push()


class _WarmBlas(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        torch.cuda.current_blas_handle()          # runs on autograd's device thread: that thread's handle
        return g


def warm_blas_handles(device=None) -> None:
    """Create the hipBLAS / rocBLAS handles of THIS thread and of autograd's device thread now.  They are made lazily on first
    use; the tuned-solution table (dalm_amd/tuning) maps some GEMM shapes to rocBLAS solutions, and a shape that meets its first
    rocBLAS solution INSIDE a hipGraph capture made the capture fail in `hipblasCreate` (seen in the retriever-only trainer on a
    new packed row count) - after which the eager fall-back died in torch's dropout (its generator was left in capture mode)."""
    if not torch.cuda.is_available():
        return
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    torch.cuda.current_blas_handle()
    x = torch.zeros(1, device=dev, requires_grad=True)
    _WarmBlas.apply(x).sum().backward()
    a = torch.zeros(8, 8, device=dev)
    torch.mm(a, a)
    torch.cuda.synchronize()


class GraphSets:
    """One built object (a captured graph, a set of tower graphs) per batch-shape key.  At most `cap` are kept, nothing is built
    during the first `skip` calls (library warm-up: every workspace and GEMM solution has seen the shapes before a capture), every
    build runs between two device synchronisations, and after the first failed build (recorded in `failed`) nothing more is built:
    the keys built so far keep replaying, every other call launches eagerly.  `hits` / `eager_calls` count the two outcomes.
    The builder is passed per call and never stored: a reference back to the owner would make a cycle, and the graphs of a cycle
    are destroyed whenever the garbage collector runs - possibly in the middle of a later capture."""

    def __init__(self, cap: int, skip: int = 0, what: str = "graphs"):
        self.cap = cap
        self.skip = skip
        self.what = what
        self.built: Dict[Hashable, object] = {}
        self.calls = 0
        self.hits = 0
        self.eager_calls = 0
        self.failed: Optional[str] = None

    def __len__(self) -> int:
        return len(self.built)

    def get(self, key: Optional[Hashable], build: Callable[[], object]) -> Optional[object]:
        """The object for `key`, built now by `build()` if allowed; None: launch this call eagerly (also whenever `key` is None)."""
        self.calls += 1
        hit = self.built.get(key) if key is not None else None
        if (hit is None and key is not None and self.failed is None and self.calls > self.skip
                and len(self.built) < self.cap):
            try:
                torch.cuda.synchronize()
                hit = self.built[key] = build()
            except Exception as e:  # keep training: same kernels, eager launches
                self.failed = repr(e)
                warnings.warn(f"dalm_amd: hipGraph capture of {self.what} failed ({self.failed[:500]}); "
                              "other shapes launch eagerly from here on")
                torch.cuda.synchronize()
        if hit is None:
            self.eager_calls += 1
        else:
            self.hits += 1
        return hit


@contextlib.contextmanager
def no_collection_while_capturing():
    """Dead reference cycles are collected BEFORE a capture begins, and the cyclic collector stays off until it has ended.

    torch.cuda.make_graphed_callables ties every graphed module into a cycle (module -> its replaced `forward` closure -> the
    module), so the hipGraphs of a step that has been dropped are freed by the cyclic collector alone, whenever it next runs.
    torch.cuda.graph used to collect on entry; by now it does so only under torch.compiler.config.force_cudagraph_gc.  A
    collection that fires INSIDE a capture destroys those graphs and releases their memory pools on the capturing thread, which
    the thread-local capture mode does not permit: the process aborts (seen in tests/test_live_rows_gpu.py, which builds a second
    step with tower graphs right after dropping the first; whether it happens depends on the allocation count so far)."""
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_enabled:
            gc.enable()


class GraphedStep:
    def __init__(self, step, warmup: int = 3, eager_steps: int = 0, max_graphs: int = 8):
        """warmup: hidden extra steps run on a side stream right before the capture (benchmarks);
        eager_steps: the first N REAL steps are launched eagerly and the capture happens after them
        (trainers: no hidden steps, and every library - hipBLASLt workspaces, GEMM solution lookup,
        allocator pools - has seen the shapes before anything is captured)."""
        self.step = step
        self.warmup = warmup
        # one graph per batch shape (trimmed / bucketed batches come in a handful of lengths); all graphs share ONE
        # memory pool - they never run concurrently, so their activations can overlay each other
        self.sets = GraphSets(cap=max_graphs, skip=eager_steps, what="the step")
        self.pool = None
        self._warm_stream: Optional[torch.cuda.Stream] = None
        self._capture_stream: Optional[torch.cuda.Stream] = None
        self._blas_warm = False
        # the LR scheduler must not be captured: it runs on the host and writes the lr tensor
        self.scheduler = step.lr_scheduler
        step.lr_scheduler = None

    # key -> (graph, static inputs, static loss, (grad_norm, aux) the capture left behind)
    graphs = property(lambda self: self.sets.built)
    failed = property(lambda self: self.sets.failed)
    replays = property(lambda self: self.sets.hits)
    eager_calls = property(lambda self: self.sets.eager_calls)
    max_graphs = property(lambda self: self.sets.cap)

    # first captured graph, for callers that only ever see one shape (bench.py, tests)
    @property
    def graph(self) -> Optional[torch.cuda.CUDAGraph]:
        return next(iter(self.graphs.values()))[0] if self.graphs else None

    @property
    def grad_norm(self) -> Optional[torch.Tensor]:
        return getattr(self.step, "grad_norm", None)

    @staticmethod
    def _key(batch) -> Tuple:
        return tuple((k, tuple(v.shape), v.dtype) for k, v in sorted(batch.items()))

    def _capture(self, batch):
        static = {k: v.clone() for k, v in batch.items()}
        if self._warm_stream is None:
            self._warm_stream = torch.cuda.Stream()
        s = self._warm_stream
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):  # warm-up off the default stream, as the capture API asks
            for _ in range(self.warmup):
                self.step(static)
                if self.scheduler is not None:
                    self.scheduler.step()
        torch.cuda.current_stream().wait_stream(s)
        init_adam_state(self.step.optimizer)  # no-op after a warm-up step; essential with warmup == 0
        if not self._blas_warm:
            warm_blas_handles()
            self._blas_warm = True
        torch.cuda.synchronize()
        if self.pool is None:
            self.pool = torch.cuda.graph_pool_handle()
        # manual begin/end instead of `with torch.cuda.graph(g)`: when the body raises (an op the capture refuses),
        # that context manager's exit raises a second error from capture_end() and never restores the current stream -
        # every later eager step then runs on a stream stuck in an invalidated capture (seen with HF Falcon's
        # list-indexed head split: the fall-back step died in dropout's RNG-state lookup)
        g = torch.cuda.CUDAGraph()
        # ONE capture stream for every graph of this step: the caching allocator hands a freed block only to requests on the
        # stream it was allocated on, so a fresh stream per capture meant that no graph could reuse the pool memory of the graphs
        # before it (reserved memory grew by a full set of activations per batch shape: 12 trimmed shapes at cfg3 ran out of
        # 288 GB; tools/graph_pool_probe.py)
        if self._capture_stream is None:
            self._capture_stream = torch.cuda.Stream()
        cs = self._capture_stream
        cs.wait_stream(torch.cuda.current_stream())
        with no_collection_while_capturing(), torch.cuda.stream(cs):
            g.capture_begin(pool=self.pool, capture_error_mode="thread_local")   # other threads (a process group's watchdog) may query events
            try:
                static_loss = self.step(static)
            except BaseException:
                try:
                    g.capture_end()
                except Exception:
                    pass
                raise
            g.capture_end()
        torch.cuda.current_stream().wait_stream(cs)
        # what the step leaves behind for its caller (each capture allocates its own tensors): the replay path points the
        # step back at THIS graph's outputs
        return g, static, static_loss, (getattr(self.step, "grad_norm", None), dict(getattr(self.step, "aux", None) or {}))

    def __call__(self, batch) -> torch.Tensor:
        hit = self.sets.get(self._key(batch), lambda: self._capture(batch))
        if hit is not None:
            g, static, loss, (gn, aux) = hit
            for k, v in batch.items():
                static[k].copy_(v, non_blocking=True)
            g.replay()
            if gn is not None:
                self.step.grad_norm = gn
            if aux and isinstance(getattr(self.step, "aux", None), dict):
                self.step.aux.update(aux)
        else:
            loss = self.step(batch)
        if self.scheduler is not None:
            self.scheduler.step()
        return loss


# ---------------------------------------------------------------------------
# Multi-GPU form: graph the towers, keep the collectives eager
# ---------------------------------------------------------------------------
def _autocast(dtype):
    return contextlib.nullcontext() if dtype is None else torch.autocast("cuda", dtype=dtype, cache_enabled=False)


class _RetrieverCall(torch.nn.Module):
    """One retriever tower call as a graph-capturable module (its parameters are the tower's: make_graphed_callables
    differentiates with respect to them).  `normalize` None: the tower is a sentence-embedding model that pools and normalises
    itself (AutoModelForSentenceEmbedding), its output is returned as is; otherwise its hidden states - of the PACKED rows when
    `rows` / `cu` are given (dalm_amd/packed.py) - go through the HIP pool / normalise."""

    def __init__(self, tower, autocast_dtype, normalize: Optional[bool] = None, skip_dead_rows: bool = True):
        super().__init__()
        self.tower = tower
        self.autocast_dtype = autocast_dtype
        self.normalize = normalize
        self.skip_dead_rows = skip_dead_rows

    def forward(self, input_ids, attention_mask, rows=None, cu=None):
        from .. import live_rows, packed
        from ..fused import pool_l2norm

        with _autocast(self.autocast_dtype):
            if self.normalize is None:
                with live_rows.tower_call(attention_mask, False, self.skip_dead_rows):
                    return self.tower(input_ids, attention_mask)
            if rows is None:     # padded: the row-wise kernels skip the padding rows (dalm_amd/live_rows.py)
                with live_rows.tower_call(attention_mask, False, self.skip_dead_rows):
                    h = self.tower(input_ids, attention_mask)[0]
            else:
                h = packed.retrieval_hidden(self.tower, input_ids, attention_mask, rows, cu)
        return pool_l2norm(h, attention_mask, self.normalize)


class _GeneratorCall(torch.nn.Module):
    """The decoder as a graph-capturable module: logits, or (hidden_only) the final normed hidden states the fused lm_head path
    consumes.  Given `rows` / `cu`: the final hidden states [n, H] of the packed rows, in the autocast dtype (what the reference's
    lm_head, an nn.Linear inside the autocast'ed forward, would read)."""

    def __init__(self, generator, autocast_dtype, hidden_only: bool = False, skip_dead_rows: bool = True):
        super().__init__()
        self.generator = generator
        self.autocast_dtype = autocast_dtype
        self.hidden_only = hidden_only
        self.skip_dead_rows = skip_dead_rows

    def forward(self, input_ids, attention_mask, rows=None, cu=None):
        from .. import live_rows, packed

        with _autocast(self.autocast_dtype):
            if rows is None:     # padded: the row-wise kernels skip the rows nothing depends on (dalm_amd/live_rows.py)
                with live_rows.tower_call(attention_mask, True, self.skip_dead_rows):
                    if self.hidden_only:
                        return self.generator.base_model(input_ids=input_ids, attention_mask=attention_mask, use_cache=False)[0]
                    # no KV cache copies
                    return self.generator(input_ids=input_ids, attention_mask=attention_mask, use_cache=False).logits
            h = packed.generator_hidden(self.generator, input_ids, attention_mask, rows, cu)
        dt = self.autocast_dtype
        return h if dt is None or h.dtype == dt else h.to(dt)


@contextlib.contextmanager
def thread_local_capture():
    """torch.cuda.make_graphed_callables captures in hipStreamCaptureModeGlobal: while the capture is open ANY thread's event
    query is an error - and torch.distributed's ProcessGroupNCCL watchdog thread polls the events of outstanding collectives.
    With a live process group the tower captures aborted the process in 5 of 8 runs of the one-rank tests ("operation not permitted
    when stream is capturing", raised in the watchdog thread, which terminates the process).  Thread-local mode keeps the check for the
    capturing thread and lets other threads be."""
    orig = torch.cuda.graph.__init__

    def init(self, cuda_graph, pool=None, stream=None, capture_error_mode="thread_local"):
        orig(self, cuda_graph, pool=pool, stream=stream, capture_error_mode="thread_local")

    torch.cuda.graph.__init__ = init
    try:
        with no_collection_while_capturing():
            yield
    finally:
        torch.cuda.graph.__init__ = orig


class GraphedEncoders:
    """The retriever-only step's two encoder calls (query, passage), forward AND backward, as single-stream hipGraphs
    (torch.cuda.make_graphed_callables, one call each: separate pools, so the query graphs replay on the tower stream while the
    passage graphs run on the main stream); loss, optimizer and collectives stay eager.  Same reason as GraphedTowers at one rank:
    a whole-step graph captured across the two streams replays with a dependency bubble per node."""

    def __init__(self, model, autocast_dtype, sample_batch: Dict[str, torch.Tensor], skip_dead_rows: bool = True):
        if getattr(model, "is_autoregressive", False):
            raise NotImplementedError("graphed encoders: autoregressive retrievers run eagerly")
        warm_blas_handles()
        calls = [_RetrieverCall(model, autocast_dtype, skip_dead_rows=skip_dead_rows) for _ in range(2)]
        for c in calls:
            c.train(model.training)
        b = sample_batch
        with thread_local_capture():
            self.query = torch.cuda.make_graphed_callables(
                calls[0], (b["query_input_ids"].clone(), b["query_attention_mask"].clone()), num_warmup_iters=3, allow_unused_input=True)
            self.passage = torch.cuda.make_graphed_callables(
                calls[1], (b["passage_input_ids"].clone(), b["passage_attention_mask"].clone()), num_warmup_iters=3, allow_unused_input=True)

    KEYS = ("query_input_ids", "passage_input_ids")

    @classmethod
    def key_of(cls, batch):
        return tuple(tuple(batch[k].shape) for k in cls.KEYS)


class GraphedTowers:
    """Forward AND backward of the three tower calls (passage, query, generator) as hipGraphs
    (torch.cuda.make_graphed_callables), everything that talks to other GPUs - the embedding all-gathers, the
    loss with its stats exchange, the gradient all-reduce - and the optimizer stay eager.  That removes >99 %
    of the per-step launches from the host path while no collective is ever captured; it is what W > 1 uses."""

    def __init__(self, rag_model, autocast_dtype, sample_batch: Dict[str, torch.Tensor], hidden_only: bool = False,
                 skip_dead_rows: bool = True):
        if getattr(rag_model, "retriever_is_autoregressive", False):
            raise NotImplementedError("graphed towers: autoregressive retrievers run eagerly")
        warm_blas_handles()
        # a batch that carries the packed row lists of all three tower inputs gets PACKED graphs (round 6): the same captures
        # around dalm_amd/packed.py's calls; the row counts are part of the key (one set of graphs per combination)
        self.packed = self.is_packed(sample_batch)
        retriever, normalize = rag_model.retriever_model, rag_model.normalize
        calls = (_RetrieverCall(retriever, autocast_dtype, normalize, skip_dead_rows),
                 _RetrieverCall(retriever, autocast_dtype, normalize, skip_dead_rows),
                 _GeneratorCall(rag_model.generator_model, autocast_dtype, hidden_only, skip_dead_rows))
        for c in calls:
            c.train(rag_model.training)
        args = [tuple(t.clone() for t in self.args(sample_batch, tower)) for tower in ("passage", "query", "generator")]
        # Callables captured in ONE make_graphed_callables call share a memory pool and must replay in capture
        # order on one stream.  The retrieval pair runs on the tower stream concurrently with the generator on
        # the main stream, so the generator gets its own capture (own pool); within the pair the order is
        # passage -> query forward and (autograd: later nodes first) query -> passage backward, as required.
        with thread_local_capture():
            self.passage, self.query = torch.cuda.make_graphed_callables(
                calls[:2], tuple(args[:2]), num_warmup_iters=3, allow_unused_input=True)
            self.generator = torch.cuda.make_graphed_callables(
                calls[2], args[2], num_warmup_iters=3, allow_unused_input=True)

    KEYS = ("retriever_passage_input_ids", "retriever_query_input_ids", "generator_input_input_ids")
    PACK_KEYS = ("retriever_passage_pack_rows", "retriever_query_pack_rows", "generator_pack_rows",
                 "retriever_passage_pack_cu", "retriever_query_pack_cu", "generator_pack_cu")
    # tower -> batch keys of its (input_ids, attention_mask, pack_rows, pack_cu)
    INPUTS = {"passage": ("retriever_passage_input_ids", "retriever_passage_attention_mask",
                          "retriever_passage_pack_rows", "retriever_passage_pack_cu"),
              "query": ("retriever_query_input_ids", "retriever_query_attention_mask",
                        "retriever_query_pack_rows", "retriever_query_pack_cu"),
              "generator": ("generator_input_input_ids", "generator_input_attention_mask",
                            "generator_pack_rows", "generator_pack_cu")}

    @classmethod
    def is_packed(cls, batch) -> bool:
        return all(k in batch for k in cls.PACK_KEYS)

    @classmethod
    def key_of(cls, batch):
        keys = cls.KEYS + (cls.PACK_KEYS if cls.is_packed(batch) else ())
        return tuple(tuple(batch[k].shape) for k in keys)

    def args(self, batch, tower: str):
        """The arguments of one tower's graphed call: ids, mask (and the packed rows, cu of a packed set)."""
        return tuple(batch[k] for k in self.INPUTS[tower][:4 if self.packed else 2])
