"""`dalm_lora2_{rowdot,rankupd,colacc}_ld` (dalm_amd/csrc/lora2.hip): the bf16 activation operand as a column slice of a wider
row-major buffer, addressed by a row stride.

Every operand is embedded in a buffer whose other columns hold a bf16 NaN pattern.  Each `_ld` call must then give, BIT FOR BIT,
what the dense entry point (`_live`) gives on a contiguous copy of the operand - outputs, mask bytes (the dropout mask is a
function of the LOGICAL element index, not of the stride), the in-place result - and rankupd must leave every poisoned element
as it was.  A NaN that leaked into a sum, or a mask that moved with the stride, shows as a bit difference.

Strides: ld = C (the dense call itself), ld = C + 8, ld = 3 C with the operand at column C.  With and without the row-liveness
vector, masks at p = 0.05, modes 1, 2 and 3.  Shapes: the smallest at which each kernel still takes every path -
rowdot R = 17 (a partial 16-row tile; a partial 8-row tile in mode 2), K = 32 (one MFMA step, three idle waves) and 1056 (33
steps: past the first double-buffer refill); rankupd R = 5 (not a multiple of 4), C = 128 (staged mask bytes), 136 (unstaged),
640 (two 512-column slabs, the second partial); colacc R = 33, C = 72 (a partial 64-column slab, more than one 32-row batch)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

P = 0.05
STRIDES = ["ld=C", "ld=C+8", "ld=3C@C"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _geom(C, case):
    return {"ld=C": (C, 0), "ld=C+8": (C + 8, 0), "ld=3C@C": (3 * C, C)}[case]


def _embed(t, case):
    """(buffer [R, ld] of bf16 NaNs with t in its columns [off, off + C), the slice)."""
    R, C = t.shape
    ld, off = _geom(C, case)
    buf = torch.full((R, ld), float("nan"), dtype=torch.bfloat16, device=t.device)
    buf[:, off:off + C] = t
    return buf, buf[:, off:off + C]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _live(R, on, dev):
    if not on:
        return None
    v = torch.ones(R, dtype=torch.uint8)
    v[1::3] = 0
    return v.to(dev)


def _keep_bits(R, C, seed, dev):
    m = torch.rand(R, C, generator=torch.Generator().manual_seed(seed)) >= P
    return torch.from_numpy(np.packbits(m.numpy().astype(np.uint8), axis=1, bitorder="little")).to(dev)


def _rowdot(entry, xs, Ws, R, K, rank, mode, live, ld=None):
    from dalm_amd import hip
    from dalm_amd.models import lora_ops as L

    dev = xs[0].device
    n = 1 if mode == 1 else 2
    zs = [torch.full((R, rank), 7.0, device=dev) for _ in range(n)]
    bits = [torch.zeros(R, K // 8, dtype=torch.uint8, device=dev) for _ in range(n)]        # dead rows' bytes are not written
    args = [hip.ptr(xs[0]), hip.ptr(xs[1]) if mode == 3 else None, hip.ptr(Ws[0]), hip.ptr(Ws[1]) if n == 2 else None,
            hip.ptr(zs[0]), hip.ptr(zs[1]) if n == 2 else None, hip.ptr(bits[0]), hip.ptr(bits[1]) if n == 2 else None,
            R, K, rank, 1.0 / (1.0 - P), P, hip.ptr(L.dropout_seed(dev)), 0xBEEF01, 0x1234567 if n == 2 else 0, mode, hip.ptr(live)]
    hip.call(entry, *args, *([ld] if ld is not None else []), hip.stream())
    return zs, bits


@pytest.mark.parametrize("with_live", [False, True])
@pytest.mark.parametrize("case", STRIDES)
@pytest.mark.parametrize("K", [32, 1056])
def test_rowdot_ld_equals_the_dense_call_on_a_copy(dev, K, case, with_live):
    R, rank = 17, 8
    g = torch.Generator().manual_seed(K)
    x0, x1 = (torch.randn(R, K, generator=g).bfloat16().to(dev) for _ in range(2))
    W0, W1 = (torch.randn(rank, K, generator=g).to(dev) / K ** 0.5 for _ in range(2))
    live = _live(R, with_live, dev)
    ld = _geom(K, case)[0]
    s0, s1 = _embed(x0, case)[1], _embed(x1, case)[1]
    for mode in (1, 2, 3):
        want = _rowdot("dalm_lora2_rowdot_live", [x0, x1], [W0, W1], R, K, rank, mode, live)
        got = _rowdot("dalm_lora2_rowdot_ld", [s0, s1], [W0, W1], R, K, rank, mode, live, ld)
        for t in range(len(want[0])):
            assert torch.equal(got[0][t].view(torch.int32), want[0][t].view(torch.int32)), f"z of slot {t}, mode {mode}"
            assert torch.equal(got[1][t], want[1][t]), f"mask bytes of slot {t}, mode {mode}"
            assert bool(torch.isfinite(got[0][t]).all())
            kept = want[1][t][live.bool()] if live is not None else want[1][t]
            assert int(kept.min()) < 255 or K == 32                         # some element was dropped: the mask is on


def _rankupd(entry, ys, zs, Ws, bits, R, C, rank, mode, live, ld=None):
    from dalm_amd import hip

    n = 1 if mode == 1 else 2
    args = [hip.ptr(ys[0]), hip.ptr(ys[1]) if mode == 3 else None, hip.ptr(zs[0]), hip.ptr(zs[1]) if n == 2 else None,
            hip.ptr(Ws[0]), hip.ptr(Ws[1]) if n == 2 else None, hip.ptr(bits[0]), hip.ptr(bits[1]) if n == 2 else None,
            R, C, rank, 1.5, mode, hip.ptr(live)]
    hip.call(entry, *args, *([ld] if ld is not None else []), hip.stream())


@pytest.mark.parametrize("with_live", [False, True])
@pytest.mark.parametrize("case", STRIDES)
@pytest.mark.parametrize("C", [128, 136, 640])
def test_rankupd_ld_updates_the_slice_and_nothing_else(dev, C, case, with_live):
    R, rank = 5, 8
    g = torch.Generator().manual_seed(C)
    y = [torch.randn(R, C, generator=g).bfloat16().to(dev) for _ in range(2)]
    zs = [torch.randn(R, rank, generator=g).to(dev) for _ in range(2)]
    Ws = [torch.randn(rank, C, generator=g).to(dev) / rank ** 0.5 for _ in range(2)]
    bits = [_keep_bits(R, C, C + t, dev) for t in range(2)]
    live = _live(R, with_live, dev)
    ld, off = _geom(C, case)
    for mode in (1, 2, 3):
        dense = [t.clone() for t in y]
        _rankupd("dalm_lora2_rankupd_live", dense, zs, Ws, bits, R, C, rank, mode, live)
        bufs = [_embed(t, case) for t in y]
        before = [b.clone() for b, _ in bufs]
        _rankupd("dalm_lora2_rankupd_ld", [s for _, s in bufs], zs, Ws, bits, R, C, rank, mode, live, ld)
        for t in range(2):
            touched = t == 0 or mode == 3
            want = before[t].clone()
            want[:, off:off + C] = dense[t] if touched else y[t]
            assert torch.equal(_bits(bufs[t][0]), _bits(want)), f"slot {t}, mode {mode}: the slice or its surroundings differ"
            if touched:
                moved = ~torch.eq(_bits(dense[t]), _bits(y[t]))
                assert bool(moved.any()) and (live is None or not bool(moved[~live.bool()].any()))


def _colacc(entry, xs, zs, bits, R, C, rank, mode, live, ld=None):
    from dalm_amd import hip

    dev = xs[0].device
    n = 1 if mode == 1 else 2
    lib = hip.load()
    outs = [torch.full((rank, C), 7.0, device=dev) for _ in range(n)]
    nbytes = lib.dalm_lora2_colacc_workspace_bytes(R, C, rank, mode)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    tickets = torch.zeros(max(int(lib.dalm_lora2_colacc_ticket_words(C, mode)), 1), dtype=torch.int32, device=dev)
    args = [hip.ptr(xs[0]), hip.ptr(xs[1]) if mode == 3 else None, hip.ptr(zs[0]), hip.ptr(zs[1]) if n == 2 else None,
            hip.ptr(bits[0]), hip.ptr(bits[1]) if n == 2 else None, hip.ptr(outs[0]), hip.ptr(outs[1]) if n == 2 else None,
            R, C, rank, 0.75, mode, hip.ptr(ws), nbytes, hip.ptr(tickets), hip.ptr(live)]
    hip.call(entry, *args, *([ld] if ld is not None else []), hip.stream())
    assert int(tickets.abs().sum()) == 0                                      # left zero
    return outs


@pytest.mark.parametrize("with_live", [False, True])
@pytest.mark.parametrize("case", STRIDES)
def test_colacc_ld_equals_the_dense_call_on_a_copy(dev, case, with_live):
    R, C, rank = 33, 72, 8
    g = torch.Generator().manual_seed(R)
    xs = [torch.randn(R, C, generator=g).bfloat16().to(dev) for _ in range(2)]
    zs = [torch.randn(R, rank, generator=g).to(dev) for _ in range(2)]
    bits = [_keep_bits(R, C, 11 + t, dev) for t in range(2)]
    live = _live(R, with_live, dev)
    ld = _geom(C, case)[0]
    sl = [_embed(t, case)[1] for t in xs]
    for mode in (1, 2, 3):
        want = _colacc("dalm_lora2_colacc_live", xs, zs, bits, R, C, rank, mode, live)
        got = _colacc("dalm_lora2_colacc_ld", sl, zs, bits, R, C, rank, mode, live, ld)
        for t in range(len(want)):
            assert bool(torch.isfinite(got[t]).all())
            assert torch.equal(got[t].view(torch.int32), want[t].view(torch.int32)), f"out of slot {t}, mode {mode}"


def test_ld_entry_points_check_the_stride(dev):
    R, C, rank = 8, 64, 8
    x = torch.zeros(R, 2 * C, dtype=torch.bfloat16, device=dev)
    W = torch.zeros(rank, C, device=dev)
    for ld in (C - 8, C + 4):                                                # shorter than a row; rows not 16-byte aligned
        with pytest.raises(ValueError):
            _rowdot("dalm_lora2_rowdot_ld", [x, x], [W, W], R, C, rank, 1, None, ld)
        with pytest.raises(ValueError):
            _rankupd("dalm_lora2_rankupd_ld", [x, x], [torch.zeros(R, rank, device=dev)] * 2, [W, W], [None, None], R, C, rank, 1, None, ld)
        with pytest.raises(ValueError):
            _colacc("dalm_lora2_colacc_ld", [x, x], [torch.zeros(R, rank, device=dev)] * 2, [None, None], R, C, rank, 1, None, ld)
    with pytest.raises(ValueError):                                          # a base that is not 16-byte aligned
        _rowdot("dalm_lora2_rowdot_ld", [x[:, 4:], x], [W, W], R, C, rank, 1, None, 2 * C)
