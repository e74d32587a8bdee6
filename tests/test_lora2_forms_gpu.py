"""`dalm_lora2_{rowdot,rankupd,colacc}` (dalm_amd/csrc/lora2.hip) at every arm of their launch geometry (csrc/lora2_plan.hpp)
and at the row edges of their pipelined loops, compared PER ELEMENT with a float64 evaluation on the device
(helpers.lora2_*_report: worst-case bounds of the kernels' own arithmetic; tests/test_lora2_rules.py shows what they reject).

Every case names the arm it is there for and asserts it through `dalm_lora2_rankupd_rows_per_wg` /
`dalm_lora2_colacc_rows_per_split`, so a later change of a budget cannot silently move a case out of its arm
(tests/lora2_plan_check.cpp --print lists the same shapes with S and the last group's rows).

rankupd (wave w of a workgroup owns rows r_lo + w + 4 i; UN = 4 rows per buffer, 3 with two terms; second buffer from 16 rows,
re-issue from 8 UN rows):
  (1160, 16384)  mode 1: 52 rows, last workgroup 16;  mode 2: 76;  mode 3: 100          pipelined loop, ragged tails
  (530, 16384)   mode 3: 48 rows, last 2;  mode 2: 36 rows (UN = 3), last 26;  mode 1: 24
  (1300, 4096)   mode 2: 24 rows = exactly one round of both buffers, last 4;  mode 1: 16;  mode 3: 28
  (2300, 32768)  mode 2: the min_s arm, 256 rows per workgroup (ballot bit 63), S = 9, last workgroup 252 rows
  (70, 640), (70, 1152): mask bytes staged through LDS with a partial last 512-column slab;  (70, 136): read per lane;
  (1160, 1152): the staged form with 8 / 8 / 12 rows per workgroup
colacc (a thread adds rows r_lo + rl + 32 u; UN = 4 rows per buffer, 2 at rank 16 / two terms; one loop iteration = 64 UN rows):
  (2400, 4096)   320 rows per split, last 160: 2 iterations at UN = 4, 3 at UN = 2;  mode 3: 608 rows
  (1300, 4096)   192 rows, last 148 (mode 3: 352)
  (1030, 1024)   S = 17 (mode 3: 11), last split 6 rows;   (577, 512)  S = 10, last split 1 row      the last arriver's loop
  the row cap (all LDS stages within 64 KB):  (7210, 4096) mode 2: 800 rows, S = 10, last 10;  (8200, 4096) mode 2: S = 11;
  (4487, 4096) mode 3 rank 16: 896 rows, S = 6, last 7;  (4100, 4096) the same, S = 5;  (12550, 4096) mode 1 rank 8: 1568, S = 9, last 6
rowdot: K in {32, 96, 512, 544, 1056, 2080} = 1, 3, 16, 17, 33, 65 MFMA steps over 4 waves with 4 steps per buffer: three idle
  waves; one idle wave; exactly one full buffer per wave; the second buffer for wave 0 only; a re-issue into buffer 0; a second
  trip round the loop.  R in {9, 17}: a partial 8-row and a partial 16-row tile.
Row liveness: protocol (a) to (e) of tests/test_live_rows_gpu.py with patterns built from the plan of the shape.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from helpers import (assert_lora2, lora2_colacc_report, lora2_rankupd_report, lora2_rowdot_report, record_measured, unpack_bits)

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
pytestmark = pytest.mark.gpu

MODE_RANK = [(1, 8), (1, 16), (2, 8), (3, 8), (3, 16)]
_WORST = {}


def _note(kernel, mode, ratio):
    """Largest error / bound seen per kernel and mode, beside the run's other outputs."""
    key = f"lora2_forms/{kernel}/mode{mode}"
    if ratio > _WORST.get(key, -1.0):
        _WORST[key] = ratio
        record_measured(key, {"max_error_over_bound": ratio})


@pytest.fixture(scope="module")
def dev():
    from dalm_amd import hip

    hip.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from dalm_amd import hip

    return hip.load()


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _bits(R, C, g, dev):
    """Random keep bytes with some all-zero and some all-one bytes among them."""
    b = torch.randint(0, 256, (R, C // 8), device=dev, generator=g, dtype=torch.uint8)
    sel = torch.rand(R, C // 8, device=dev, generator=g)
    b[sel < 0.1] = 0
    b[sel > 0.95] = 255
    return b


def _activations(R, C, n, sliced, g, dev):
    """n bf16 [R, C] operands: dense, or column slices of ONE [R, 3 C] buffer (row stride 3 C).  Returns (views, buffer)."""
    if not sliced:
        return [torch.randn(R, C, device=dev, generator=g).bfloat16() for _ in range(n)], None
    buf = torch.randn(R, 3 * C, device=dev, generator=g).bfloat16()
    cols = [1] if n == 1 else [0, 2]
    return [buf[:, c * C:(c + 1) * C] for c in cols], buf


# =====================================================================================================================
# rankupd
# =====================================================================================================================
# (R, C) -> rows per workgroup in modes 1, 2, 3
RANKUPD_SHAPES = {
    (1160, 16384): (52, 76, 100), (530, 16384): (24, 36, 48), (1300, 4096): (16, 24, 28),
    (70, 640): (4, 4, 4), (70, 1152): (4, 4, 4), (70, 136): (4, 4, 4), (1160, 1152): (8, 8, 12)}


def _rankupd_operands(R, C, rank, mode, sliced, dev, seed):
    g = _gen(dev, seed)
    n = 1 if mode == 1 else 2
    ys, buf = _activations(R, C, 2 if mode == 3 else 1, sliced, g, dev)
    zs = [torch.randn(R, rank, device=dev, generator=g) for _ in range(n)]
    Ws = [torch.randn(rank, C, device=dev, generator=g) / rank ** 0.5 for _ in range(n)]
    bits = [_bits(R, C, g, dev) for _ in range(n)]
    return ys, buf, zs, Ws, bits


def _rankupd_values(ys, buf, zs, Ws, bits, rank, scale, mode, live=None):
    """One launch on copies of ys; every output element against float64; a slice's sibling columns untouched.  Returns the ratio."""
    from dalm_amd.models import lora_ops as L

    C = ys[0].shape[1]
    if buf is None:
        outs = [y.clone() for y in ys]
        L.rankupd2_(outs, zs, Ws, bits, rank, scale, mode, live)
    else:
        work = buf.clone()
        cols = [1] if len(ys) == 1 else [0, 2]
        outs = [work[:, c * C:(c + 1) * C] for c in cols]
        L.rankupd2_(outs, zs, Ws, bits, rank, scale, mode, live)
        for c in set(range(3)) - set(cols):
            assert torch.equal(work[:, c * C:(c + 1) * C], buf[:, c * C:(c + 1) * C]), "columns outside the slice were written"
    keeps = [unpack_bits(b, C) for b in bits] if bits is not None else [None] * len(zs)
    worst = 0.0
    for i, (y, out) in enumerate(zip(ys, outs)):
        terms = [(zs[i], Ws[i], keeps[i])] if mode == 3 else [(z, W, k) for z, W, k in zip(zs, Ws, keeps)]
        worst = max(worst, assert_lora2(f"rankupd mode {mode} y{i}", lora2_rankupd_report(out, y, terms, scale, live)))
    return worst


@pytest.mark.parametrize("mode,rank", MODE_RANK)
@pytest.mark.parametrize("R,C", sorted(RANKUPD_SHAPES))
def test_rankupd_arms_vs_float64(dev, lib, R, C, mode, rank):
    assert lib.dalm_lora2_rankupd_rows_per_wg(R, C, mode) == RANKUPD_SHAPES[(R, C)][mode - 1]
    for sliced in (False, True):
        ys, buf, zs, Ws, bits = _rankupd_operands(R, C, rank, mode, sliced, dev, R + C + mode)
        for masked in (False, True):
            _note("rankupd", mode, _rankupd_values(ys, buf, zs, Ws, bits if masked else None, rank, 0.75, mode))


@pytest.fixture(scope="module")
def big(dev, lib):
    """(2300, 32768) mode 2 with masks: 256 rows per workgroup, the mask stage at its 32 KB; built once."""
    R, C = 2300, 32768
    assert lib.dalm_lora2_rankupd_rows_per_wg(R, C, 2) == 256
    return (R, C) + _rankupd_operands(R, C, 8, 2, False, dev, 77)


def test_rankupd_256_rows_per_workgroup(big):
    R, C, ys, buf, zs, Ws, bits = big
    _note("rankupd", 2, _rankupd_values(ys, buf, zs, Ws, bits, 8, 0.75, 2))


# =====================================================================================================================
# colacc
# =====================================================================================================================
# (R, C) -> {(mode, rank): rows per split} for the forms run at that shape
def _FULL(a, b):
    return {(1, 8): a, (1, 16): a, (2, 8): a, (3, 8): b, (3, 16): b}


COLACC_SHAPES = {
    (2400, 4096): _FULL(320, 608), (1300, 4096): _FULL(192, 352), (1030, 1024): _FULL(64, 96), (577, 512): _FULL(64, 64),
    # the row cap: 800 rows with two terms, 896 at rank 16, 1568 at rank 8
    (7210, 4096): {(2, 8): 800}, (8200, 4096): {(2, 8): 800}, (4487, 4096): {(3, 16): 896}, (4100, 4096): {(3, 16): 896},
    (12550, 4096): {(1, 8): 1568}}
COLACC_CASES = [(R, C, m, r) for (R, C), forms in sorted(COLACC_SHAPES.items()) for (m, r) in sorted(forms)]


def _colacc_operands(R, C, rank, mode, dev, seed):
    g = _gen(dev, seed)
    n = 1 if mode == 1 else 2
    xs = [torch.randn(R, C, device=dev, generator=g).bfloat16() for _ in range(2 if mode == 3 else 1)]
    zs = [torch.randn(R, rank, device=dev, generator=g) for _ in range(n)]
    bits = [_bits(R, C, g, dev) for _ in range(n)]
    return xs, zs, bits


def _tickets_are_zero():
    from dalm_amd.models import lora_ops as L

    torch.cuda.synchronize()
    for buf in L._tickets2.values():
        assert int(buf.abs().sum()) == 0, "colacc left a ticket behind"


@pytest.mark.parametrize("R,C,mode,rank", COLACC_CASES)
def test_colacc_arms_vs_float64_twice_and_tickets_are_left_zero(dev, lib, R, C, mode, rank):
    from dalm_amd.models import lora_ops as L

    rows = lib.dalm_lora2_colacc_rows_per_split(R, C, rank, mode)
    assert rows == COLACC_SHAPES[(R, C)][(mode, rank)]
    xs, zs, bits = _colacc_operands(R, C, rank, mode, dev, R + C + mode + rank)
    for masked in (False, True):
        keeps = [unpack_bits(b, C) for b in bits] if masked else [None] * len(zs)
        first = None
        for _ in range(2):                                     # twice: the second call finds the tickets the first one left
            outs = L.colacc2(xs, zs, bits if masked else None, rank, 1.5, mode)
            for t, o in enumerate(outs):
                rep = lora2_colacc_report(o, xs[t] if mode == 3 else xs[0], zs[t], 1.5, rows, keeps[t])
                _note("colacc", mode, assert_lora2(f"colacc mode {mode} out{t}", rep))
            if first is not None:
                assert all(torch.equal(a, b) for a, b in zip(first, outs)), "the second call differs from the first"
            first = outs
        _tickets_are_zero()


def test_colacc_is_bitwise_reproducible_with_a_ragged_last_split(dev, lib):
    from dalm_amd.models import lora_ops as L

    R, C = 2400, 4096
    assert lib.dalm_lora2_colacc_rows_per_split(R, C, 8, 2) == 320
    xs, zs, bits = _colacc_operands(R, C, 8, 2, dev, 5)
    a = L.colacc2(xs, zs, bits, 8, 1.0, 2)
    for _ in range(3):
        b = L.colacc2(xs, zs, bits, 8, 1.0, 2)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# =====================================================================================================================
# rowdot
# =====================================================================================================================
ROWDOT_K = [32, 96, 512, 544, 1056, 2080]
ROWDOT_R = [9, 17]


def _rowdot_operands(R, K, rank, mode, dev, seed):
    g = _gen(dev, seed)
    n = 1 if mode == 1 else 2
    xs = [torch.randn(R, K, device=dev, generator=g).bfloat16() for _ in range(2 if mode == 3 else 1)]
    Ws = [torch.randn(rank, K, device=dev, generator=g) / K ** 0.5 for _ in range(n)]
    return xs, Ws


def _rowdot_values(xs, Ws, rank, p, mode, live, dev):
    """One launch: the keep bits of live rows against oracle/lora_mask.py bit for bit, every z element against float64."""
    import lora_mask as O

    from dalm_amd.models import lora_ops as L

    R, K = xs[0].shape
    salts = [0xBEEF01, 0x1234567][:len(Ws)]
    scale = 1.0 / (1.0 - p)
    seed = int(L.dropout_seed(dev).item()) if p > 0 else 0
    zs, bits = L.rowdot2(xs, Ws, rank, scale, p, salts, mode, live)
    torch.cuda.synchronize()
    keep_rows = (live != 0).cpu().numpy() if live is not None else np.ones(R, dtype=bool)
    worst = 0.0
    for t, W in enumerate(Ws):
        keep = None
        if p > 0:
            want = O.keep_mask_v2(seed, salts[t], R, K, p)
            assert np.array_equal(bits[t].cpu().numpy()[keep_rows], O.pack_bits(want)[keep_rows]), f"mask bits of slot {t}, K = {K}, R = {R}"
            keep = torch.from_numpy(want).to(dev)
        rep = lora2_rowdot_report(zs[t], xs[t] if mode == 3 else xs[0], W, scale, keep, live)
        worst = max(worst, assert_lora2(f"rowdot mode {mode} z{t} (R = {R}, K = {K})", rep))
    return worst


@pytest.mark.parametrize("p", [0.0, 0.05])
@pytest.mark.parametrize("mode,rank", MODE_RANK)
def test_rowdot_step_counts_and_partial_tiles_vs_float64(dev, mode, rank, p):
    from dalm_amd.models import lora_ops as L

    L.advance_dropout_seed(dev)
    for K in ROWDOT_K:
        for R in ROWDOT_R:
            xs, Ws = _rowdot_operands(R, K, rank, mode, dev, R + K)
            _note("rowdot", mode, _rowdot_values(xs, Ws, rank, p, mode, None, dev))


# =====================================================================================================================
# row liveness at these geometries: protocol (a) to (e) of tests/test_live_rows_gpu.py
# =====================================================================================================================
def _vec(R, dev, fill=1):
    return torch.full((R,), fill, dtype=torch.uint8, device=dev)


def _group_patterns(R, rows, dev, lanes):
    """Liveness vectors for groups of `rows` rows (rankupd's workgroups, colacc's splits) whose rows a lane class owns every
    `lanes`-th of (rankupd: a wave owns row % 4; colacc: a wave owns 8 of every 32 rows)."""
    S = -(-R // rows)
    r = torch.arange(R, device=dev)
    inside = r % rows
    pats = {}
    mid = min(1, S - 1)
    pats["one_group_dead"] = (r // rows != mid).to(torch.uint8)
    if lanes == 4:
        pats["one_wave_dead"] = (inside % 4 != 2).to(torch.uint8)                      # every row of wave 2, in every workgroup
    else:
        pats["one_wave_dead"] = ((inside % 32) // 8 != 1).to(torch.uint8)              # every row of wave 1, in every split
    last = torch.minimum((r // rows + 1) * rows, torch.tensor(R, device=dev)) - 1
    pats["last_row_only"] = (r == last).to(torch.uint8)                                 # with 256 rows per workgroup: ballot bit 63
    pats["alternating"] = (r % 2).to(torch.uint8)
    pats["all_dead"] = _vec(R, dev, 0)
    pats["all_live"] = _vec(R, dev, 1)
    return pats


def _rankupd_live(dev, lib, R, C, mode, rank, rows, operands, patterns):
    from test_live_rows_gpu import _check

    from dalm_amd.models import lora_ops as L

    assert lib.dalm_lora2_rankupd_rows_per_wg(R, C, mode) == rows
    ys, _, zs, Ws, bits = operands
    n = 1 if mode == 1 else 2
    pats = _group_patterns(R, rows, dev, 4)

    def run(y0, y1, z0, z1, b0, b1, live):
        out = [y0, y1] if mode == 3 else [y0]
        L.rankupd2_(out, [z0, z1][:n], Ws, [b0, b1][:n], rank, 0.75, mode, live)
        return {f"y{i}": y for i, y in enumerate(out)}

    ins = {"y0": ys[0], "y1": ys[-1], "z0": zs[0], "z1": zs[-1], "b0": bits[0], "b1": bits[-1]}
    for name in patterns:
        _check(run, ins, {}, pats[name], fresh=(), inplace={f"y{i}": f"y{i}" for i in range(2 if mode == 3 else 1)})
    # and the values of a call with dead rows: dead rows bit for bit, live rows within the element rule
    _note("rankupd", mode, _rankupd_values(ys, None, zs, Ws, bits, rank, 0.75, mode, pats["one_wave_dead"]))


@pytest.mark.parametrize("R,C,mode,rank,rows", [(1160, 16384, 1, 8, 52), (530, 16384, 3, 16, 48), (530, 16384, 2, 8, 36),
                                                (1300, 4096, 2, 8, 24), (70, 136, 1, 16, 4)])
def test_rankupd_liveness_in_the_pipelined_loop(dev, lib, R, C, mode, rank, rows):
    ops = _rankupd_operands(R, C, rank, mode, False, dev, 3 * R + mode)
    _rankupd_live(dev, lib, R, C, mode, rank, rows, ops, ["one_group_dead", "one_wave_dead", "last_row_only", "alternating", "all_dead", "all_live"])


def test_rankupd_liveness_at_256_rows_per_workgroup(dev, lib, big):
    """The last row of a 256-row workgroup is row 63 of wave 3: bit 63 of the ballot.  The last workgroup has 252 rows."""
    R, C, ys, buf, zs, Ws, bits = big
    _rankupd_live(dev, lib, R, C, 2, 8, 256, (ys, buf, zs, Ws, bits), ["last_row_only", "one_wave_dead", "one_group_dead"])


def _colacc_protocol(run, ins, live):
    """(c), (d), (e) for a sum over rows: equal to the NULL call on inputs whose dead rows were zeroed, bit for bit, also with
    NaN in the dead rows of x, z and the mask bytes."""
    from test_live_rows_gpu import _nan_dead

    keep = live != 0
    zeroed = {k: v.clone() for k, v in ins.items()}
    for v in zeroed.values():
        v[~keep] = 0
    ref = run(**zeroed, live=None)
    out = run(**ins, live=live)
    out_nan = run(**{k: _nan_dead(v, ~keep) for k, v in ins.items()}, live=live)
    for r, o, on in zip(ref, out, out_nan):
        assert torch.isfinite(on).all()
        assert torch.equal(o, r), "(d) differs from the NULL call on zeroed inputs"
        assert torch.equal(on, r), "(c) differs with NaN in the dead rows"
    if bool(keep.all()):
        for r, o in zip(run(**ins, live=None), out):
            assert torch.equal(o, r), "(e)"
    return out


@pytest.mark.parametrize("R,C,mode,rank,rows,UN", [(2400, 4096, 1, 16, 320, 2), (7210, 4096, 2, 8, 800, 2), (12550, 4096, 1, 8, 1568, 4),
                                                   (4487, 4096, 3, 16, 896, 2), (1030, 1024, 2, 8, 64, 2), (577, 512, 3, 8, 64, 4)])
@pytest.mark.parametrize("masked", [False, True])
def test_colacc_liveness_skips_whole_batches(dev, lib, R, C, mode, rank, rows, UN, masked):
    """`one_batch_dead`: rows [64 UN, 128 UN) of every split - both buffers of the loop's second iteration - are dead between
    live iterations (splits of more than 128 UN rows)."""
    from dalm_amd.models import lora_ops as L

    assert lib.dalm_lora2_colacc_rows_per_split(R, C, rank, mode) == rows
    xs, zs, bits = _colacc_operands(R, C, rank, mode, dev, R + 7 * mode)
    n = 1 if mode == 1 else 2
    pats = _group_patterns(R, rows, dev, 32)
    if rows > 128 * UN:
        inside = torch.arange(R, device=dev) % rows
        pats["one_batch_dead"] = ((inside < 64 * UN) | (inside >= 128 * UN)).to(torch.uint8)

    def run(x0, x1, z0, z1, b0, b1, live):
        return L.colacc2([x0, x1] if mode == 3 else [x0], [z0, z1][:n], [b0, b1][:n] if masked else None, rank, 1.5, mode, live)

    ins = {"x0": xs[0], "x1": xs[-1], "z0": zs[0], "z1": zs[-1], "b0": bits[0], "b1": bits[-1]}
    for name, live in pats.items():
        outs = _colacc_protocol(run, ins, live)
        if name in ("one_batch_dead", "one_wave_dead", "all_dead"):        # and the values, per element
            for t, o in enumerate(outs):
                keep = unpack_bits(bits[t], C) if masked else None
                rep = lora2_colacc_report(o, xs[t] if mode == 3 else xs[0], zs[t], 1.5, rows, keep, live)
                _note("colacc", mode, assert_lora2(f"colacc mode {mode} out{t}, {name}", rep))
    _tickets_are_zero()


@pytest.mark.parametrize("p", [0.0, 0.05])
@pytest.mark.parametrize("mode,rank", MODE_RANK)
def test_rowdot_liveness_with_a_second_buffer(dev, mode, rank, p):
    """K = 544: 17 MFMA steps, wave 0 fills its second buffer.  R = 40: 16-row tiles 0..15, 16..31, 32..39 (8-row tiles in mode 2).
    Rows 16..31 dead (a whole tile, two in mode 2), rows 0..15 dead but row 5 (a tile with a single live row; in mode 2 tile 1
    is dead as well), the partial last tile live."""
    from test_live_rows_gpu import _check

    from dalm_amd.models import lora_ops as L

    R, K = 40, 544
    xs, Ws = _rowdot_operands(R, K, rank, mode, dev, 9)
    n = 1 if mode == 1 else 2
    L.advance_dropout_seed(dev)
    tiles = _vec(R, dev)
    tiles[:32] = 0
    tiles[5] = 1
    alternating = (torch.arange(R, device=dev) % 2).to(torch.uint8)

    def run(x0, x1, live):
        zs, bits = L.rowdot2([x0, x1] if mode == 3 else [x0], Ws, rank, 1.0 / (1.0 - p), p, [11, 12][:n], mode, live)
        out = {f"z{i}": z for i, z in enumerate(zs)}
        if p > 0:
            out.update({f"bits{i}": b for i, b in enumerate(bits)})
        return out

    for live in (tiles, alternating, _vec(R, dev, 0), _vec(R, dev, 1)):
        _check(run, {"x0": xs[0], "x1": xs[-1]}, {}, live, fresh=[f"z{i}" for i in range(n)],
               bits=[f"bits{i}" for i in range(n)] if p > 0 else ())
        _note("rowdot", mode, _rowdot_values(xs, Ws, rank, p, mode, live, dev))
