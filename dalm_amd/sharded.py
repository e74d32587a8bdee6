"""Multi-GPU plumbing for the sharded in-batch negatives (one process per GPU, RCCL over xGMI).

What crosses GPUs per step (W ranks, B_l rows each, D = embedding width):
  * all-gather of passage embeddings  [B_l, D] f32   - started right after the passage tower on a
    side HIP stream so it overlaps the query tower's forward (GatherHandle)
  * all-gather of query embeddings    [B_l, D] f32
  * all-reduce of the token count M   1 float
  * all-gather of (lse_r, lse_c, a, b) [B_l, 4] f32   in the backward
  * all-reduce (SUM) of the trainable-parameter gradients, one flat bucket (LoRA: ~21 MB)
Nothing else: the backward is closed-form, so no autograd graph spans a collective and no
reduce-scatter of dP is needed (each rank recomputes its own column block on the matrix cores).
"""
from __future__ import annotations

import os
from typing import Iterable, List, Optional

import torch

from .fused import GatherHandle, LocalComm, TorchDistComm  # noqa: F401


def init_distributed(backend: Optional[str] = None):
    """Initialise torch.distributed from the torchrun environment; returns (comm, device)."""
    from . import configure_hw_queues

    configure_hw_queues()  # no effect once the HIP runtime is up; entry points call it first thing as well
    world = int(os.environ.get("WORLD_SIZE", "1"))
    # DALM_FORCE_DIST=1 runs the RCCL code path even with one rank (used to smoke-test the collectives,
    # side-stream gathers and the gradient bucket on a single-GPU box)
    if world == 1 and os.environ.get("DALM_FORCE_DIST", "0") != "1":
        dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
        if dev.type == "cuda":
            torch.cuda.set_device(dev)
        return LocalComm(), dev
    import torch.distributed as dist

    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # W > 1 on GPUs: torch.distributed(nccl) - RCCL through torch - is the default.  The library's OWN RCCL binding (dalm_comm_*
    # behind the C ABI, collectives on the caller's stream; it ties torch.distributed with one rank: 188.1 vs 188.9 ms per step,
    # profiles/history/r03_comm_modes.txt) is OPT-IN until a run with two or more real ranks has been recorded (no multi-GPU box was
    # available in rounds 1-5): a rank whose ncclCommInitRank stalls instead of raising would leave the others
    # blocked inside the bring-up collective, and the agreement step below only covers failures that raise.
    #   DALM_NATIVE_COMM=1     the native binding, errors propagate
    #   DALM_NATIVE_COMM=auto  the native binding, self-tested; every rank falls back to torch.distributed if any rank raised
    #   unset / 0              torch.distributed(nccl)
    native = os.environ.get("DALM_NATIVE_COMM", "0")
    if torch.cuda.is_available() and os.environ.get("DALM_CLAIM_QUEUES", "1") != "0":
        from .streams import claim_compute_queues

        torch.cuda.set_device(local_rank)
        claim_compute_queues(local_rank)      # the two compute streams get their hardware queues before RCCL's streams exist
    if torch.cuda.is_available() and backend in (None, "nccl") and native in ("1", "auto"):
        dev = torch.device("cuda", local_rank)
        torch.cuda.set_device(dev)
        comm = native_comm_or_none(int(os.environ.get("RANK", "0")), world, insist=(native == "1"))
        if comm is not None:
            return comm, dev
    if torch.cuda.is_available():
        dev = torch.device("cuda", local_rank)
        torch.cuda.set_device(dev)
        backend = backend or "nccl"  # == RCCL on ROCm
    else:
        dev = torch.device("cpu")
        backend = backend or "gloo"
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        if backend == "nccl":
            dist.init_process_group(backend=backend, device_id=dev)
        else:
            dist.init_process_group(backend=backend)
    return TorchDistComm(), dev


def native_comm_or_none(rank: int, world: int, insist: bool = False, make=None):
    """The library's own RCCL communicator, brought up and self-tested - or None when ANY rank failed to (the ranks agree
    through the rendezvous store, so either all of them continue natively or all fall back to torch.distributed).
    insist: raise instead of returning None.  `make(rendezvous)` builds the communicator (tests inject a fake)."""
    import warnings

    from .comm import NativeRcclComm, Rendezvous

    if os.environ.get("DALM_COMM_ID_FILE"):          # explicit file rendezvous: no agreement channel, errors propagate
        comm = NativeRcclComm()
        comm.self_test()
        return comm
    rdv, comm, err = None, None, None
    try:
        rdv = Rendezvous(rank, world)
        comm = _bring_up_with_deadline(make or (lambda r: NativeRcclComm(rendezvous=r)), rdv,
                                       float(os.environ.get("DALM_COMM_BRINGUP_TIMEOUT_S", "90")))
    except Exception as e:
        err = e
        if rdv is not None:
            try:
                rdv.publish_failure(e)                 # rank 0 failing before it published the id: unblock the others now
            except Exception:
                pass
    if rdv is None:                                    # no channel to agree over: every rank fails the same way here
        if insist:
            raise err
        warnings.warn(f"dalm_amd: native RCCL communicator unavailable ({err!r}); using torch.distributed(nccl)")
        return None
    all_ok = rdv.agree(err is None)
    if all_ok:
        return comm
    if comm is not None:
        try:
            comm.close()
        except Exception:
            pass
    rdv.release()                                      # rank 0 gives MASTER_PORT back for init_process_group
    if insist:
        raise err if err is not None else RuntimeError("another rank could not bring up the native RCCL communicator")
    warnings.warn("dalm_amd: native RCCL communicator unavailable on at least one rank"
                  + (f" (here: {err!r})" if err is not None else "") + "; all ranks use torch.distributed(nccl)")
    return None


def _bring_up_with_deadline(make, rdv, deadline_s: float):
    """WATCHDOG around the bring-up of the native communicator (ncclCommInitRank + the self-test's two collectives): the work
    runs in a helper thread and this thread waits for it at most `deadline_s`.  RCCL's bring-up is a collective - a rank that
    STALLS in it (instead of raising) used to leave every other rank blocked inside the same call with no way out (ADVICE r4,
    VERDICT r5 item 3a).  With the deadline, every rank that is stuck - the stalled one and the ones waiting for it - gives up
    with a TimeoutError, reports "failed" through the rendezvous store (`agree`), and ALL ranks fall back to
    torch.distributed(nccl) together (or raise together under DALM_NATIVE_COMM=1).  The helper thread of a stalled rank is a
    daemon and is left behind; it holds no lock the fallback needs."""
    import threading

    box = {}
    device = torch.cuda.current_device() if torch.cuda.is_available() else None

    def work():
        try:
            if device is not None:
                torch.cuda.set_device(device)          # the current HIP device is per thread
            c = make(rdv)
            box["made"] = c
            c.self_test()
            box["comm"] = c
        except BaseException as e:                     # noqa: BLE001 - handed to the waiting thread
            box["err"] = e

    t = threading.Thread(target=work, name="dalm-comm-bringup", daemon=True)
    t.start()
    t.join(deadline_s)
    if t.is_alive():
        raise TimeoutError(f"native RCCL communicator: bring-up / self-test did not finish within {deadline_s:.0f} s "
                           "(DALM_COMM_BRINGUP_TIMEOUT_S); a rank is stalled inside ncclCommInitRank or its first collective")
    if "err" in box:
        if box.get("made") is not None:                # constructed, failed its self-test: release it before falling back
            try:
                box["made"].close()
            except Exception:
                pass
        raise box["err"]
    return box["comm"]


def allreduce_grads(params: Iterable[torch.nn.Parameter], comm) -> None:
    """SUM the gradients over ranks through one flat bucket (rank losses are shares of the
    global-batch loss, so summing reproduces the single-process gradient)."""
    if isinstance(comm, LocalComm):
        return
    ps: List[torch.nn.Parameter] = [p for p in params if p.requires_grad]
    for p in ps:
        if p.grad is None:
            p.grad = torch.zeros_like(p)
    flat = torch.cat([p.grad.reshape(-1).float() for p in ps])
    comm.all_reduce_sum_(flat)
    off = 0
    for p in ps:
        n = p.numel()
        p.grad.copy_(flat[off:off + n].view(p.grad.shape))
        off += n


def _view_like(flat: torch.Tensor, p: torch.Tensor) -> torch.Tensor:
    """A view of the 1-D slice `flat` with the SHAPE AND STRIDES of `p`: lora_B parameters live in transposed ([r, N]-major)
    memory (models/lora.py), and the fused optimizer wants parameter and gradient laid out alike."""
    if p.is_contiguous():
        return flat.view_as(p)
    if p.dim() == 2 and p.t().is_contiguous():
        return flat.view(p.shape[1], p.shape[0]).t()
    raise ValueError(f"GradBucket: parameter layout {tuple(p.shape)} / {p.stride()} is neither dense nor transposed-dense")


class _Bucket:
    __slots__ = ("lo", "hi", "count", "pending", "streams", "launched", "done")

    def __init__(self, lo: int, hi: int, count: int):
        self.lo, self.hi, self.count = lo, hi, count
        self.pending, self.streams, self.launched, self.done = count, [], False, None


class GradBucket:
    """All trainable gradients as views of ONE flat fp32 buffer (what DDP calls gradient_as_bucket_view):
    backward accumulates straight into the buffer and the fused optimizer reads the views - no per-step
    flatten / ~400 tiny copy-back launches.  Grads are zeroed, never set to None.

    The buffer is cut into contiguous buckets of ~bucket_bytes.  Every parameter carries a
    post-accumulate-grad hook; when the last gradient of a bucket has landed, that bucket's all-reduce (SUM)
    is issued on a communication stream while the rest of the backward keeps running - the overlap the
    reference gets from DDP's reducer (train_rage2e.py:416-418,471).  Buckets are launched in a FIXED order
    (highest offset first: the backward produces the last layers' gradients first) so that every rank issues
    the same sequence of collectives whatever order its hooks fire in.  `all_reduce()` after backward flushes
    the buckets that never became ready (parameters without a gradient this step) and makes the current stream
    wait for the communication stream.  overlap=False gives one blocking all-reduce of the whole buffer."""

    def __init__(self, params: Iterable[torch.nn.Parameter], comm, bucket_bytes: int = 4 << 20,
                 overlap: Optional[bool] = None):
        self.comm = comm
        self.params: List[torch.nn.Parameter] = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("GradBucket: no trainable parameters")
        dev = self.params[0].device
        if any(p.dtype != torch.float32 or p.device != dev for p in self.params):
            raise ValueError("GradBucket needs fp32 trainable parameters on one device")
        self.flat = torch.zeros(sum(p.numel() for p in self.params), device=dev, dtype=torch.float32)
        self.overlap = (overlap is None or bool(overlap)) and not isinstance(comm, LocalComm)
        self.comm_stream = torch.cuda.Stream(device=dev) if (self.overlap and dev.type == "cuda") else None
        self.buckets: List[_Bucket] = []
        self._bucket_of: List[int] = []
        off, lo, count = 0, 0, 0
        per = max(int(bucket_bytes) // 4, 1)
        for p in self.params:
            n = p.numel()
            p.grad = _view_like(self.flat[off:off + n], p)
            self._bucket_of.append(len(self.buckets))
            off += n
            count += 1
            if off - lo >= per:
                self.buckets.append(_Bucket(lo, off, count))
                lo, count = off, 0
        if count:
            self.buckets.append(_Bucket(lo, off, count))
        self._next = len(self.buckets) - 1  # next bucket allowed to launch (descending)
        self.launch_log: List[int] = []     # bucket indices in launch order, last step (tests / debugging)
        self._handles = []
        if self.overlap:
            for i, p in enumerate(self.params):
                self._handles.append(p.register_post_accumulate_grad_hook(self._make_hook(self._bucket_of[i])))

    # ---- hook side (autograd thread, during backward) ------------------------------------------------
    def _make_hook(self, bi: int):
        def hook(_param):
            b = self.buckets[bi]
            b.pending -= 1
            if self.comm_stream is not None:
                s = torch.cuda.current_stream()
                if all(s != t for t in b.streams):
                    b.streams.append(s)
            if b.pending == 0:
                self._launch_ready()
        return hook

    def _launch_ready(self) -> None:
        while self._next >= 0 and self.buckets[self._next].pending <= 0:
            self._launch(self.buckets[self._next])
            self._next -= 1

    def _launch(self, b: _Bucket) -> None:
        view = self.flat[b.lo:b.hi]
        if self.comm_stream is not None:
            # gradients of one bucket may have been accumulated on several streams (towers / generator):
            # the communication stream waits for everything queued so far on each of them
            for s in (b.streams or [torch.cuda.current_stream()]):
                ev = torch.cuda.Event()
                ev.record(s)
                self.comm_stream.wait_event(ev)
            with torch.cuda.stream(self.comm_stream):
                self.comm.all_reduce_sum_(view)
                b.done = torch.cuda.Event()
                b.done.record(self.comm_stream)
        else:
            self.comm.all_reduce_sum_(view)
        b.launched = True
        self.launch_log.append(self.buckets.index(b))

    # ---- step side -------------------------------------------------------------------------------
    def all_reduce(self) -> None:
        """Call after backward: afterwards every .grad view holds the SUM over ranks (ordered on the current stream)."""
        if isinstance(self.comm, LocalComm):
            return
        if not self.overlap:
            self.comm.all_reduce_sum_(self.flat)
            return
        cur = torch.cuda.current_stream() if self.comm_stream is not None else None
        while self._next >= 0:  # buckets whose hooks did not all fire (unused parameters): flush in order
            b = self.buckets[self._next]
            if cur is not None and all(cur != t for t in b.streams):
                b.streams.append(cur)
            self._launch(b)
            self._next -= 1
        for b in self.buckets:
            if cur is not None and b.done is not None:
                cur.wait_event(b.done)
            b.pending, b.streams, b.launched, b.done = b.count, [], False, None
        self._next = len(self.buckets) - 1
        self.last_launch_log, self.launch_log = self.launch_log, []

    def zero(self) -> None:
        self.flat.zero_()
        off = 0
        for p in self.params:  # re-attach in case something replaced .grad (e.g. set_to_none)
            n = p.numel()
            if p.grad is None or p.grad.data_ptr() != self.flat.data_ptr() + 4 * off:
                p.grad = _view_like(self.flat[off:off + n], p)
            off += n


def max_over_ranks(comm, value: float) -> float:
    """MAX of a host scalar over the ranks (bench.py: the slowest rank's elapsed time) on whichever communicator runs."""
    if isinstance(comm, LocalComm):
        return float(value)
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized():
        t = torch.tensor([value], dtype=torch.float64,
                         device=torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())
    # native communicator: all-gather the values (sum / gather are the collectives the C ABI exposes); float32 keeps a few
    # seconds to ~1e-7 relative
    t = torch.tensor([[value]], dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
    return float(comm.all_gather_rows(t).max().item())


def barrier(comm) -> None:
    if isinstance(comm, LocalComm):
        return
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized():
        dist.barrier()
    else:   # native communicator: a 1-float all-reduce + host sync is the barrier
        t = torch.zeros(1, device=torch.device("cuda", torch.cuda.current_device()))
        comm.all_reduce_sum_(t)
        torch.cuda.current_stream().synchronize()
