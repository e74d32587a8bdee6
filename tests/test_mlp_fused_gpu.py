"""`dalm_linear_live_swiglu` (dalm_amd/csrc/linear_live.hip) on the GPU against the unfused pair of entry points it replaces, run in
the same process: `dalm_linear_live` followed by `dalm_swiglu_fwd_2d_live` (those are checked against fp64 in
test_linear_live_gpu.py and test_tower_ops_gpu.py).  Same contraction order, same element arithmetic (csrc/swiglu_math.hpp): the
live rows must be EQUAL, bit for bit.

Dead rows of every input hold NaN: they must not be read.  Every output arrives filled with a sentinel, with guard rows in front of
and behind it: dead rows and guard rows must still hold the sentinel afterwards - the fused entry point writes nothing there.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

R = 520                                        # two full 256-row tiles and a partial one
GUARD = 3
SENT = 7.0
LIVE_COUNTS = (0, 1, 255, 256, 257, 519, 520)


@pytest.fixture(scope="module")
def dev():
    from dalm_amd import hip

    hip.load()
    return torch.device("cuda:0")


def _masks(count, dev):
    """A scattered (random) liveness vector and a contiguous prefix with `count` live rows each."""
    g = torch.Generator().manual_seed(977 + count)
    scattered = torch.zeros(R, dtype=torch.uint8)
    scattered[torch.randperm(R, generator=g)[:count]] = 1
    prefix = torch.zeros(R, dtype=torch.uint8)
    prefix[:count] = 1
    return (("scattered", scattered.to(dev)), ("prefix", prefix.to(dev)))


def _guarded(cols, dev):
    buf = torch.full((R + 2 * GUARD, cols), SENT, dtype=torch.bfloat16, device=dev)
    return buf, buf[GUARD:GUARD + R]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _assert_untouched(buf, view, keep, tag):
    assert bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + R:] == SENT).all()), f"{tag}: guard rows written"
    assert bool((view[~keep] == SENT).all()), f"{tag}: dead rows written"


_INPUTS = {}


def _inputs(C, K, dev):
    """a [R, K], wcat [2C, K] (bf16 on the device), shared by every case of one shape."""
    if (C, K) not in _INPUTS:
        g = torch.Generator().manual_seed(100 * C + K)
        a = torch.randn(R, K, generator=g).bfloat16()
        wcat = (2.0 * torch.randn(2 * C, K, generator=g) / math.sqrt(K)).bfloat16()
        _INPUTS[(C, K)] = tuple(t.to(dev) for t in (a, wcat))
    return _INPUTS[(C, K)]


def _poisoned(t, vec):
    t = t.clone()
    t[vec == 0] = float("nan")
    return t


def _swiglu_fwd_ref(y, C, vec):
    from dalm_amd import hip

    act = torch.full((R, C), SENT, dtype=torch.bfloat16, device=y.device)
    hip.call("dalm_swiglu_fwd_2d_live", hip.ptr(y[:, :C]), hip.ptr(y[:, C:]), hip.ptr(act), hip.dtype_code(y), R, C, 2 * C, 2 * C, C,
             hip.ptr(vec), hip.stream())
    return act


def _fused_fwd(a, wcat, C, K, part, dev):
    from dalm_amd import hip

    ybuf, y = _guarded(2 * C, dev)
    abuf, act = _guarded(C, dev)
    hip.call("dalm_linear_live_swiglu", hip.ptr(a), a.stride(0), hip.ptr(wcat), hip.ptr(y), 2 * C, hip.ptr(act), C, R, C, K,
             hip.ptr(part[0]), hip.ptr(part[1]), hip.stream())
    return ybuf, y, abuf, act


@pytest.mark.parametrize("K", [64, 192])             # the single-K-tile path / an odd number of K tiles
@pytest.mark.parametrize("C", [128, 384])            # one mixed tile / three (the last one not a multiple of 256 columns)
def test_forward_equals_the_unfused_pair(dev, C, K):
    from dalm_amd import linear_live

    a0, wcat = _inputs(C, K, dev)
    for count in LIVE_COUNTS:
        for name, vec in _masks(count, dev):
            tag = f"C={C} K={K} live={count} {name}"
            keep = vec != 0
            a = _poisoned(a0, vec)
            part = linear_live.row_partition(vec)
            y_ref = linear_live.linear_live(a, wcat, part)
            act_ref = _swiglu_fwd_ref(y_ref, C, vec)
            ybuf, y, abuf, act = _fused_fwd(a, wcat, C, K, part, dev)
            torch.cuda.synchronize()
            assert torch.equal(_bits(y[keep]), _bits(y_ref[keep])), f"{tag}: gate | up differ from dalm_linear_live"
            assert torch.equal(_bits(act[keep]), _bits(act_ref[keep])), f"{tag}: act differs from dalm_swiglu_fwd_2d_live"
            assert torch.isfinite(y[keep].float()).all() and torch.isfinite(act[keep].float()).all(), f"{tag}: NaN leaked in"
            _assert_untouched(ybuf, y, keep, tag + " (y)")
            _assert_untouched(abuf, act, keep, tag + " (act)")


def test_wrappers_return_the_same_bits(dev):
    """linear_live.linear_live_swiglu (fresh torch.empty outputs) against the raw calls above."""
    from dalm_amd import linear_live

    C, K = 384, 192
    a0, wcat = _inputs(C, K, dev)
    vec = _masks(257, dev)[0][1]
    keep = vec != 0
    part = linear_live.row_partition(vec)
    y, act = linear_live.linear_live_swiglu(_poisoned(a0, vec), wcat, part)
    y_ref = linear_live.linear_live(a0, wcat, part)
    assert torch.equal(_bits(y[keep]), _bits(y_ref[keep]))
    assert torch.equal(_bits(act[keep]), _bits(_swiglu_fwd_ref(y_ref, C, vec)[keep]))


def test_a_corrupt_partition_stores_nothing_out_of_bounds(dev):
    """perm entries outside [0, R) select nothing: only the rows a valid entry names may change; guard rows keep their sentinel."""
    C, K = 384, 192
    a, wcat = _inputs(C, K, dev)
    g = torch.Generator().manual_seed(11)
    perm = torch.randperm(R, generator=g).to(torch.int32)
    bad = torch.tensor([-1, R, R + 1, R + GUARD, 2 ** 31 - 1, -2 ** 31, -R, 1 << 20], dtype=torch.int32)
    where = torch.randperm(R, generator=g)[:64]
    perm[where] = bad.repeat(8)
    named = torch.zeros(R, dtype=torch.bool)
    ok = (perm >= 0) & (perm < R)
    named[perm[ok].long()] = True
    named = named.to(dev)
    part = (perm.to(dev), torch.tensor([R], dtype=torch.int32, device=dev))
    ybuf, y, abuf, act = _fused_fwd(a, wcat, C, K, part, dev)
    torch.cuda.synchronize()
    _assert_untouched(ybuf, y, named, "forward y")
    _assert_untouched(abuf, act, named, "forward act")
    assert torch.isfinite(y[named].float()).all() and not bool((act[named] == SENT).all())
