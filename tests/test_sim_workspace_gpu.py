"""No similarity launcher writes outside the workspace its size function reports (csrc/sim_plan.hpp gives both).

Every entry point is called through the C ABI with a workspace that is a slice of a larger buffer: exactly the reported
size, at the weakest alignment the entry point accepts, filled with 0xFF bytes, guard bytes in front of it and behind it.
The guards must survive, and every output must be bit-equal to the same call through `ops.*` with a workspace of its own.
Shapes: one per branch of stream_plan, flash_plan, sim_splitk and small_plan (tests/sim_plan_check.cpp --print shows them)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SCALE = 100.0
GUARD, GUARD_BYTE = 512, 0xA5


@pytest.fixture(scope="module")
def gpu():
    from dalm_amd import hip
    from dalm_amd.ops import HipOps

    return hip, hip.load(), HipOps(), torch.device("cuda:0")


class Guarded:
    """`size` bytes of 0xFF inside a guard-filled buffer, starting `align` bytes past a 256-byte boundary: aligned to `align` and
    to nothing coarser."""

    def __init__(self, dev, size, align):
        self.size, self.off = size, GUARD + align
        self.buf = torch.full((self.off + size + GUARD,), GUARD_BYTE, device=dev, dtype=torch.uint8)
        assert self.buf.data_ptr() % 256 == 0 and GUARD % 256 == 0
        self.buf[self.off:self.off + size] = 0xFF
        self.ptr = self.buf.data_ptr() + self.off

    def assert_guards_intact(self):
        assert bool((self.buf[:self.off] == GUARD_BYTE).all()), "write in front of the workspace"
        assert bool((self.buf[self.off + self.size:] == GUARD_BYTE).all()), "write behind the workspace"


def _operands(dev, m, n, D):
    g = torch.Generator().manual_seed(m * 7 + n * 3 + D)
    A = torch.nn.functional.normalize(torch.randn(m, D, generator=g), dim=1).to(dev)
    Bm = torch.nn.functional.normalize(torch.randn(n, D, generator=g), dim=1).to(dev)
    return A, Bm, g


def _softmax_stats(A, Bm, g):
    """(row_coef, row_lse, col_coef, col_lse) of S = SCALE * A . Bm^T, as a backward receives them."""
    m, n = A.shape[0], Bm.shape[0]
    S = SCALE * (A.double() @ Bm.double().t())
    rc, cc = (torch.rand(m, generator=g) / m).to(A.device), (torch.rand(n, generator=g) / n).to(A.device)
    return rc, torch.logsumexp(S, 1).float(), cc, torch.logsumexp(S, 0).float()


# RT 2 needs m >= 4096 and diag_offset = n - m needs n >= m; D = 72 keeps the bf16x3 form (and its larger workspace) out of
# dalm_sim_rowstats_workspace_bytes, so the reported size is exactly what dalm_sim_rowstats_f32 carves
@pytest.mark.parametrize("m,n,D", [(512, 512, 64), (1200, 1200, 72), (1536, 1536, 72), (4096, 4100, 72), (18, 144, 1024),
                                   (100, 300, 40), (1024, 2048, 32)])
def test_rowstats_f32_stays_inside_its_workspace(gpu, m, n, D):
    hip, lib, ops, dev = gpu
    A, Bm, _ = _operands(dev, m, n, D)
    ws = Guarded(dev, lib.dalm_sim_rowstats_workspace_bytes(m, n, D), 4)
    row_lse, diag = torch.empty(m, device=dev), torch.empty(m, device=dev)
    hip.call("dalm_sim_rowstats_f32", hip.ptr(A), hip.ptr(Bm), m, n, D, SCALE, n - m, hip.ptr(row_lse), hip.ptr(diag), ws.ptr,
             ws.size, hip.stream())
    ws.assert_guards_intact()
    want_lse, want_diag = ops.sim_rowstats_f32(A, Bm, SCALE, n - m)
    assert torch.equal(row_lse, want_lse) and torch.equal(diag, want_diag)


@pytest.mark.parametrize("m,n,D", [(32, 128, 128), (64, 256, 128), (32, 128, 1024), (100, 300, 96), (100, 300, 320)])
def test_grad_stays_inside_its_workspace(gpu, m, n, D):
    hip, lib, ops, dev = gpu
    A, Bm, g = _operands(dev, m, n, D)
    rc, rl, cc, cl = _softmax_stats(A, Bm, g)
    ws = Guarded(dev, lib.dalm_sim_grad_workspace_bytes(m, n, D), 16)
    dA = torch.empty(m, D, device=dev)
    hip.call("dalm_sim_grad", hip.ptr(A), hip.ptr(Bm), m, n, D, SCALE, n - m, hip.ptr(rc), hip.ptr(rl), hip.ptr(cc), hip.ptr(cl),
             hip.ptr(dA), ws.ptr, ws.size, hip.stream())
    ws.assert_guards_intact()
    assert torch.equal(dA, ops.sim_grad(A, Bm, SCALE, n - m, rc, rl, cc, cl))


@pytest.mark.parametrize("m,n,D,k", [(5, 40, 64, 7), (4096, 64, 64, 1)])
def test_topk_and_gold_rank_stay_inside_their_workspaces(gpu, m, n, D, k):
    hip, lib, ops, dev = gpu
    Q, Cm, g = _operands(dev, m, n, D)
    ws = Guarded(dev, lib.dalm_sim_topk_workspace_bytes(m, n, D, k), 16)
    val, idx = torch.empty(m, k, device=dev), torch.empty(m, k, device=dev, dtype=torch.int64)
    ovf = torch.empty(1, device=dev, dtype=torch.int32)
    hip.call("dalm_sim_topk", hip.ptr(Q), hip.ptr(Cm), m, n, D, SCALE, k, hip.ptr(val), hip.ptr(idx), hip.ptr(ovf), ws.ptr, ws.size,
             hip.stream())
    ws.assert_guards_intact()
    want_val, want_idx, want_ovf = ops.sim_topk(Q, Cm, k, SCALE)
    assert int(ovf) == 0 and int(want_ovf) == 0
    assert torch.equal(val, want_val) and torch.equal(idx, want_idx)

    gold = torch.randint(0, n, (m,), generator=g).to(dev)
    gold_score = ops.sim_gold_score(Q, Cm, gold, 0, torch.empty(m, device=dev), SCALE)
    ws = Guarded(dev, lib.dalm_sim_gold_rank_workspace_bytes(m, n, D), 16)
    rank, n_ge = torch.zeros(m, device=dev, dtype=torch.int64), torch.zeros(m, device=dev, dtype=torch.int64)
    hip.call("dalm_sim_gold_rank", hip.ptr(Q), hip.ptr(Cm), hip.ptr(gold), hip.ptr(gold_score), m, n, D, 0, SCALE, 0.0,
             hip.ptr(rank), hip.ptr(n_ge), ws.ptr, ws.size, hip.stream())
    ws.assert_guards_intact()
    want_rank, want_ge = ops.sim_gold_rank(Q, Cm, gold, gold_score, 0, 0.0, torch.zeros_like(rank), torch.zeros_like(n_ge), SCALE)
    assert torch.equal(rank, want_rank) and torch.equal(n_ge, want_ge)


@pytest.mark.parametrize("want_cols", [False, True])
@pytest.mark.parametrize("m,n,D", [(150, 1200, 1024), (512, 512, 1024), (18, 18, 1024), (33, 65, 1030)])
def test_small_forwards_stay_inside_their_workspaces(gpu, m, n, D, want_cols):
    hip, lib, ops, dev = gpu
    A, Bm, _ = _operands(dev, m, n, D)
    for one_launch in (False, True):
        S, row_lse, diag = torch.empty(m, n, device=dev), torch.empty(m, device=dev), torch.empty(m, device=dev)
        col_lse = torch.empty(n, device=dev) if want_cols else None
        if one_launch:   # any alignment: the launcher aligns the pointer up itself
            ws = Guarded(dev, lib.dalm_sim_small_fwd1_workspace_bytes(m, n, D, int(want_cols)), 1)
            tickets = torch.zeros(lib.dalm_sim_small_fwd1_ticket_words(m, n), device=dev, dtype=torch.int32)
            hip.call("dalm_sim_small_fwd1", hip.ptr(A), hip.ptr(Bm), m, n, D, SCALE, n - m, hip.ptr(S), n, hip.ptr(row_lse),
                     hip.ptr(diag), hip.ptr(col_lse), ws.ptr, ws.size, hip.ptr(tickets), hip.stream())
            assert not bool(tickets.any()), "tickets are left zero"
        else:
            ws = Guarded(dev, lib.dalm_sim_small_workspace_bytes(m, n, D, int(want_cols)), 4)
            hip.call("dalm_sim_small_fwd", hip.ptr(A), hip.ptr(Bm), m, n, D, SCALE, n - m, hip.ptr(S), n, hip.ptr(row_lse),
                     hip.ptr(diag), hip.ptr(col_lse), ws.ptr, ws.size, hip.stream())
        ws.assert_guards_intact()
        want = ops.sim_small_fwd(A, Bm, SCALE, n - m, want_cols, one_launch=one_launch)
        for got, ref in zip((S, row_lse, diag, col_lse), want):
            assert (got is None and ref is None) or torch.equal(got, ref)


@pytest.mark.parametrize("m,n,D,both", [(150, 1200, 1024, False), (18, 18, 1024, True)])
def test_small_backwards_stay_inside_their_workspaces(gpu, m, n, D, both):
    hip, lib, ops, dev = gpu
    A, Bm, g = _operands(dev, m, n, D)
    rc, rl, cc, cl = _softmax_stats(A, Bm, g)
    S = ops.sim_small_fwd(A, Bm, SCALE, n - m, False)[0]
    for one_launch in (False, True):
        size_fn = lib.dalm_sim_small_bwd1_workspace_bytes if one_launch else lib.dalm_sim_small_bwd_workspace_bytes
        ws = Guarded(dev, size_fn(m, n, D, 1, int(both)), 16)
        assert (ws.size > 0) == (not both)                         # one direction of a long contraction is sliced
        dA = torch.empty(m, D, device=dev)
        dB = torch.empty(n, D, device=dev) if both else None
        args = (hip.ptr(S), n, hip.ptr(A), hip.ptr(Bm), m, n, D, SCALE, n - m, hip.ptr(rc), hip.ptr(rl), hip.ptr(cc), hip.ptr(cl),
                hip.ptr(dA), hip.ptr(dB), ws.ptr, ws.size)
        if one_launch:
            tickets = torch.zeros(lib.dalm_sim_small_bwd1_ticket_words(m, n, D), device=dev, dtype=torch.int32)
            hip.call("dalm_sim_small_bwd1", *args, hip.ptr(tickets), hip.stream())
            assert not bool(tickets.any()), "tickets are left zero"
        else:
            hip.call("dalm_sim_small_bwd_ws", *args, hip.stream())
        ws.assert_guards_intact()
        want_dA, want_dB = ops.sim_small_bwd(S, A, Bm, SCALE, n - m, rc, rl, cc, cl, want_dB=both, one_launch=one_launch)
        assert torch.equal(dA, want_dA) and (not both or torch.equal(dB, want_dB))
