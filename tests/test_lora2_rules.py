"""The per-element rules of tests/helpers.py for `dalm_lora2_{rowdot,rankupd,colacc}`, on the CPU: each accepts the float64
reference rounded the way its kernel rounds, and rejects the errors a kernel of this family can make - one 32-column MFMA step
missing from a row of z, one 8-column chunk of y without its update or updated against its mask byte, one row missing from a
split's column sum, one split's partial added twice.  The whole-tensor relative norms of the older tests (2e-5 / 4e-3 / 3e-6)
accept several of these; that is shown too.  Inputs are plain randn; no element is left out of a comparison."""
import pytest
import torch

from helpers import (assert_lora2, lora2_colacc_report, lora2_rankupd_report, lora2_rowdot_report, norm_rel_err, unpack_bits)

RANK = 8


def _bf16_split(W):
    """hi + lo as the rowdot kernel forms them: two bf16 roundings."""
    hi = W.bfloat16().float()
    return hi.double() + (W - hi).bfloat16().double()


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rowdot():
    g = torch.Generator().manual_seed(11)
    R, K = 17, 2080
    x = torch.randn(R, K, generator=g).bfloat16()
    W = torch.randn(RANK, K, generator=g) / K ** 0.5
    keep = torch.rand(R, K, generator=g) > 0.05
    live = torch.ones(R, dtype=torch.uint8)
    live[3] = 0
    return x, W, keep, live


def _rowdot_like_kernel(x, W, keep, live, scale, skip=None):
    """float64 sum over the bf16 hi + lo split of W, one f32 rounding of the sum and one of the scaled result."""
    x64 = x.double() * keep * (live != 0).unsqueeze(1)
    if skip is not None:
        row, step = skip
        x64 = x64.clone()
        x64[row, 32 * step:32 * step + 32] = 0
    return (scale * (x64 @ _bf16_split(W).t()).float()).float()


def test_rowdot_rule(rowdot):
    x, W, keep, live = rowdot
    scale = 1.0 / 0.95
    good = _rowdot_like_kernel(x, W, keep, live, scale)
    rep = lora2_rowdot_report(good, x, W, scale, keep, live)
    assert rep["checked"] == good.numel() and assert_lora2("rowdot", rep) < 0.5
    for row, step in [(0, 0), (16, 64), (9, 33)]:                        # first, last (a wave's second trip) and a middle step
        bad = _rowdot_like_kernel(x, W, keep, live, scale, skip=(row, step))
        rep = lora2_rowdot_report(bad, x, W, scale, keep, live)
        assert rep["ratio"] > 1.0 and rep["at"][0] == row
        with pytest.raises(AssertionError, match="rowdot"):
            assert_lora2("rowdot", rep)
    bad = good.clone()
    bad[3, 5] = 1e-30                                                    # a dead row's z must be an exact zero
    assert lora2_rowdot_report(bad, x, W, scale, keep, live)["ratio"] > 1.0
    assert lora2_rowdot_report(bad, x, W, scale, keep, live)["at"] == [3, 5]


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rankupd():
    g = torch.Generator().manual_seed(12)
    R, C = 300, 1152
    y = torch.randn(R, C, generator=g).bfloat16()
    zs = [torch.randn(R, RANK, generator=g) for _ in range(2)]
    Ws = [torch.randn(RANK, C, generator=g) / RANK ** 0.5 for _ in range(2)]
    bits = [torch.randint(0, 256, (R, C // 8), generator=g, dtype=torch.uint8) for _ in range(2)]
    bits[0][7, 3] = 0                                                    # one chunk that no term touches
    bits[1][7, 3] = 0
    live = torch.ones(R, dtype=torch.uint8)
    live[100:104] = 0
    return y, zs, Ws, bits, live


def _rankupd_like_kernel(y, terms, scale, live):
    out = y.double()
    lv = (live != 0).unsqueeze(1)
    for z, W, keep in terms:
        out = out + scale * (z.double() @ W.double()) * (keep if keep is not None else 1) * lv
    return out.float().bfloat16()


@pytest.mark.parametrize("nt,masked", [(1, False), (1, True), (2, True)])
def test_rankupd_rule(rankupd, nt, masked):
    y, zs, Ws, bits, live = rankupd
    C = y.shape[1]
    scale = 0.5
    terms = [(zs[t], Ws[t], unpack_bits(bits[t], C) if masked else None) for t in range(nt)]
    good = _rankupd_like_kernel(y, terms, scale, live)
    rep = lora2_rankupd_report(good, y, terms, scale, live)
    assert rep["checked"] == y.numel() and assert_lora2("rankupd", rep) <= 1.0
    # one 8-column chunk of one row keeps its old value: the 4e-3 whole-tensor rule does not see it, the element rule does
    row, chunk = 211, 17
    bad = good.clone()
    bad[row, 8 * chunk:8 * chunk + 8] = y[row, 8 * chunk:8 * chunk + 8]
    plain = y.double() + scale * sum((z.double() @ W.double()) * (k if k is not None else 1) for z, W, k in terms) * (live != 0).unsqueeze(1)
    assert norm_rel_err(bad, plain) < 4e-3
    rep = lora2_rankupd_report(bad, y, terms, scale, live)
    assert rep["ratio"] > 1.0 and rep["at"][0] == row and rep["at"][1] // 8 == chunk
    # a dead row updated
    bad = good.clone()
    full = _rankupd_like_kernel(y, terms, scale, torch.ones_like(live))
    bad[101] = full[101]
    rep = lora2_rankupd_report(bad, y, terms, scale, live)
    assert rep["ratio"] == float("inf") and rep["at"][0] == 101
    if masked:                                                           # a chunk updated although every mask byte is 0
        bad = good.clone()
        unmasked = _rankupd_like_kernel(y, [(z, W, None) for z, W, _ in terms], scale, live)
        bad[7, 24:32] = unmasked[7, 24:32]
        assert not torch.equal(bad[7, 24:32], y[7, 24:32])
        assert norm_rel_err(bad, plain) < 4e-3
        rep = lora2_rankupd_report(bad, y, terms, scale, live)
        assert rep["ratio"] == float("inf") and rep["at"][0] == 7 and rep["at"][1] // 8 == 3
        # one element updated against its bit inside a byte that keeps others
        keep0 = terms[0][2]
        r, c = [int(v[0]) for v in torch.nonzero(~(keep0 if nt == 1 else keep0 | terms[1][2]), as_tuple=True)]
        bad = good.clone()
        bad[r, c] = unmasked[r, c]
        if not torch.equal(bad[r, c], y[r, c]):
            assert lora2_rankupd_report(bad, y, terms, scale, live)["at"] == [r, c]


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def colacc():
    g = torch.Generator().manual_seed(13)
    R, C, rows_per_split = 1030, 136, 64
    x = torch.randn(R, C, generator=g).bfloat16()
    z = torch.randn(R, RANK, generator=g)
    keep = unpack_bits(torch.randint(0, 256, (R, C // 8), generator=g, dtype=torch.uint8), C)
    live = (torch.rand(R, generator=g) > 0.2).to(torch.uint8)
    live[64:128] = 0                                                     # one whole split
    return x, z, keep, live, rows_per_split


def _colacc_like_kernel(x, z, keep, live, scale, rps, drop_row=None, twice=None):
    """f32 partial sums per split (each a float64 sum rounded once), added in f32 in split order, scaled in f32."""
    x64 = x.double() * keep * (live != 0).unsqueeze(1)
    R = x.shape[0]
    total = torch.zeros(z.shape[1], x.shape[1])
    for s, r0 in enumerate(range(0, R, rps)):
        xs = x64[r0:r0 + rps].clone()
        if drop_row is not None and r0 <= drop_row[0] < r0 + rps:
            xs[drop_row[0] - r0, drop_row[1]:drop_row[1] + 64] = 0       # one row of one 64-column slab
        part = (z[r0:r0 + rps].double().t() @ xs).float()
        total = total + part
        if twice == s:
            total = total + part
    return (torch.tensor(scale) * total).float()


def test_colacc_rule(colacc):
    x, z, keep, live, rps = colacc
    scale = 2.0
    good = _colacc_like_kernel(x, z, keep, live, scale, rps)
    rep = lora2_colacc_report(good, x, z, scale, rps, keep, live)
    assert rep["checked"] == good.numel() and assert_lora2("colacc", rep) < 0.5
    ref = scale * z.double().t() @ (x.double() * keep * (live != 0).unsqueeze(1))
    live_rows = torch.nonzero(live).flatten().tolist()
    for row in (live_rows[0], live_rows[-1], live_rows[len(live_rows) // 2]):   # the last split holds 6 rows
        bad = _colacc_like_kernel(x, z, keep, live, scale, rps, drop_row=(row, 64))
        rep = lora2_colacc_report(bad, x, z, scale, rps, keep, live)
        assert rep["ratio"] > 1.0 and 64 <= rep["at"][1] < 128, row
    bad = _colacc_like_kernel(x, z, keep, live, scale, rps, twice=16)     # the 6-row split counted twice
    assert lora2_colacc_report(bad, x, z, scale, rps, keep, live)["ratio"] > 1.0
    bad = _colacc_like_kernel(x, z, keep, live, scale, rps, twice=1)      # a dead split twice: nothing to see, and nothing wrong
    assert torch.equal(bad, good)
    with pytest.raises(AssertionError, match="derived for"):              # a shape the rule is not for
        lora2_colacc_report(good[:, :8], x[:4, :8], z[:4], scale, 64)


def test_unpack_bits_is_pack_bits_inverted():
    import sys
    from pathlib import Path

    import numpy as np

    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
    import lora_mask as O

    m = np.random.default_rng(0).random((5, 72)) > 0.3
    assert np.array_equal(unpack_bits(torch.from_numpy(O.pack_bits(m)), 72).numpy(), m)
