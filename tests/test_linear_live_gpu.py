"""`dalm_row_partition` and `dalm_linear_live` (dalm_amd/csrc/linear_live.hip, wrappers in dalm_amd/linear_live.py) on the GPU.

Reference: the fp64 product of the bf16 inputs on the host (plus the old C where accumulating).  Criterion, per element:
    |y - ref| <= ulp_bf16(ref) + C_TOL * sum_k |a_k w_k|
C_TOL comes from the path being replaced: `test_library_gemm_sets_the_constant` measures, on these very inputs, the smallest power
of two for which torch's own bf16 `F.linear` / `addmm_` passes; C_TOL is that value doubled once and the kernel is held to it.

Dead rows of A hold NaN in every case: they must not be read.  A fresh output arrives filled with a sentinel and must leave with
exact zeros in its dead rows; an accumulating one must keep their bits.  The output is a column view of a wider buffer in the
strided cases, whose other columns must keep their sentinel in every row.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# measured on MI355X with the inputs below: torch's bf16 F.linear / addmm_ passes from 2^-25 = 2.98e-8 upwards (largest excess
# over one ulp: 1.732e-8 of sum |a w|); doubled once
C_TOL = 2.0 ** -24

KS = (64, 128, 192)                 # no loop iteration / even / odd tail of the two-buffer K loop
NS = (8, 256, 264)                  # one partial column tile / exactly one / one and a partial
RS = (1, 255, 256, 257, 513)


@pytest.fixture(scope="module")
def dev():
    from dalm_amd import hip

    hip.load()
    return torch.device("cuda:0")


def _live_counts(R):
    return sorted({c for c in (0, 1, 255, 256, 257, R - 1, R) if 0 <= c <= R})


_CASES = {}


def _case(R, N, K, dev):
    """Inputs and host reference of one shape, computed once and shared: a [R, K], w [N, K], old C [R, N] (bf16 on the device),
    ref = a . w^T and sabs = |a| . |w|^T (fp64, on the device for the comparison)."""
    key = (R, N, K)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 * R + 10 * N + K)
        a = torch.randn(R, K, generator=g).bfloat16()
        w = (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16()
        old = torch.randn(R, N, generator=g).bfloat16()
        ref = a.double() @ w.double().t()
        sabs = a.double().abs() @ w.double().abs().t()
        _CASES[key] = tuple(t.to(dev) for t in (a, w, old, ref, sabs))
    return _CASES[key]


def _ulp_bf16(x):
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -126))      # |x| = m 2^e, m in [0.5, 1): the bf16 spacing there is 2^(e - 8)
    return torch.ldexp(torch.ones_like(x), e - 8)


def _excess(y, ref, sabs):
    """max over elements of (|y - ref| - ulp_bf16(ref)) / sum |a w|: the criterion holds iff this is <= the constant."""
    err = (y.double() - ref).abs() - _ulp_bf16(ref)
    return float((err / sabs.clamp_min(1e-300)).max()) if y.numel() else 0.0


def _vec(R, count, seed, dev):
    g = torch.Generator().manual_seed(seed)
    v = torch.zeros(R, dtype=torch.uint8)
    v[torch.randperm(R, generator=g)[:count]] = 1
    return v.to(dev)


def _run(dev, a, w, old, vec, accumulate, strided):
    """One launch on poisoned inputs -> (C view, whole C buffer).  Strided: A and C are column views at offset 8 of buffers 16
    columns wider (lda > K, ldc > N)."""
    from dalm_amd import linear_live

    R, K = a.shape
    N = w.shape[0]
    pad = 16 if strided else 0
    abuf = torch.full((R, K + pad), float("nan"), dtype=torch.bfloat16, device=dev)
    av = abuf[:, pad // 2:pad // 2 + K]
    av.copy_(a)
    av[vec == 0] = float("nan")
    cbuf = torch.full((R, N + pad), 7.0, dtype=torch.bfloat16, device=dev)
    cv = cbuf[:, pad // 2:pad // 2 + N]
    if accumulate:
        cv.copy_(old)
    part = linear_live.row_partition(vec)
    out = linear_live.linear_live(av, w, part, out=cv, accumulate=accumulate)
    assert out.data_ptr() == cv.data_ptr()
    return cv, cbuf


def _verify(dev, R, N, K, vec, accumulate, strided, tag):
    a, w, old, ref, sabs = _case(R, N, K, dev)
    cv, cbuf = _run(dev, a, w, old, vec, accumulate, strided)
    keep = vec != 0
    want = ref + old.double() if accumulate else ref
    ex = _excess(cv[keep], want[keep], sabs[keep])
    assert ex <= C_TOL, f"{tag}: live rows miss the criterion: excess {ex:.3e} > {C_TOL:.3e}"
    if accumulate:
        assert torch.equal(cv[~keep].view(torch.int16), old[~keep].view(torch.int16)), f"{tag}: dead rows of an accumulating C changed"
    else:
        assert not cv[~keep].view(torch.int16).any(), f"{tag}: dead rows of a fresh C are not exactly zero"
    assert torch.isfinite(cv.float()).all(), f"{tag}: NaN leaked out of the dead rows of A"
    if strided:
        pad = 8
        assert bool((cbuf[:, :pad] == 7.0).all()) and bool((cbuf[:, pad + N:] == 7.0).all()), f"{tag}: neighbouring columns touched"


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "views"])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_shapes_live_counts_modes_and_forms(dev, K, N, strided):
    for R in RS:
        for count in _live_counts(R):
            vec = _vec(R, count, 31 * R + count, dev)
            for accumulate in (False, True):
                _verify(dev, R, N, K, vec, accumulate, strided, f"R={R} N={N} K={K} live={count} acc={accumulate}")


def _prefix_mask(dev):
    """3 sequences of 96 rows, left-padded by 0 / 37 / 95 rows."""
    v = torch.ones(3, 96, dtype=torch.uint8)
    v[1, :37] = 0
    v[2, :95] = 0
    return v.reshape(-1).to(dev)


@pytest.mark.parametrize("pattern", ["left_padded", "interleaved", "interleaved_odd"])
def test_live_patterns(dev, pattern):
    R, N, K = 288, 264, 128
    if pattern == "left_padded":
        vec = _prefix_mask(dev)
    else:
        vec = torch.zeros(R, dtype=torch.uint8, device=dev)
        vec[(1 if pattern.endswith("odd") else 0)::2] = 1
    for accumulate in (False, True):
        for strided in (False, True):
            _verify(dev, R, N, K, vec, accumulate, strided, f"{pattern} acc={accumulate} strided={strided}")


def test_library_gemm_sets_the_constant(dev):
    """The figure C_TOL rests on: the excess of torch's bf16 GEMM over one ulp, as a fraction of sum |a w|, on this file's inputs."""
    worst = 0.0
    for K in KS:
        for N in NS:
            for R in RS:
                a, w, old, ref, sabs = _case(R, N, K, dev)
                worst = max(worst, _excess(F.linear(a, w), ref, sabs))
                worst = max(worst, _excess(old.clone().addmm_(a, w.t()), ref + old.double(), sabs))
    smallest = 2.0 ** math.ceil(math.log2(worst)) if worst > 0 else 0.0
    print(f"library bf16 GEMM: largest excess {worst:.3e} of sum |a w| -> smallest passing power of two {smallest:.3e}; C_TOL {C_TOL:.3e}")
    assert worst <= C_TOL


@pytest.mark.parametrize("R", [1, 2, 1023, 1024, 1025, 4608, 5003])
def test_partition_kernel(dev, R):
    from dalm_amd import linear_live

    g = torch.Generator().manual_seed(R)
    vecs = [torch.zeros(R, dtype=torch.uint8), torch.ones(R, dtype=torch.uint8), (torch.rand(R, generator=g) < 0.6).to(torch.uint8),
            (torch.rand(R, generator=g) < 0.05).to(torch.uint8) * 255]
    for v in vecs:
        perm, n_live = linear_live.row_partition(v.to(dev))
        idx = torch.arange(R)
        want = torch.cat([idx[v != 0], idx[v == 0]]).to(torch.int32)
        assert int(n_live.item()) == int((v != 0).sum())
        assert torch.equal(perm.cpu(), want)
        ref_perm, ref_n = linear_live.partition_reference(v.tolist())
        assert ref_perm == want.tolist() and ref_n == int(n_live.item())


def test_graph_replay_follows_a_changed_mask(dev):
    """Partition and GEMM captured once; the mask changes between two replays: the second result is the second mask's."""
    from dalm_amd import linear_live

    R, N, K = 288, 264, 128
    a, w, old, ref, sabs = _case(R, N, K, dev)
    first, second = _prefix_mask(dev), _vec(R, 257, 77, dev)
    mask = first.clone()
    out = torch.empty(R, N, dtype=torch.bfloat16, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        linear_live.linear_live(a, w, linear_live.row_partition(mask), out=out)         # warm-up outside the capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            linear_live.linear_live(a, w, linear_live.row_partition(mask), out=out)
    torch.cuda.current_stream().wait_stream(s)
    results = []
    for vec in (first, second):
        mask.copy_(vec)
        out.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        results.append(out.clone())
    for vec, y in zip((first, second), results):
        keep = vec != 0
        assert _excess(y[keep], ref[keep], sabs[keep]) <= C_TOL
        assert not y[~keep].view(torch.int16).any()
    assert not torch.equal(first, second)
