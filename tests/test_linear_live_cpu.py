"""Host logic of the live-row GEMM route (dalm_amd/linear_live.py): the partition's host reference, the routing predicate and the
tile accounting behind the estimate table of DESIGN.md "Live-row GEMM"."""
import pytest
import torch

from dalm_amd import linear_live


def test_partition_reference_is_a_stable_partition():
    assert linear_live.partition_reference([]) == ([], 0)
    assert linear_live.partition_reference([0, 0, 0]) == ([0, 1, 2], 0)
    assert linear_live.partition_reference([1, 255, 7]) == ([0, 1, 2], 3)
    assert linear_live.partition_reference([0, 1, 0, 1, 1, 0]) == ([1, 3, 4, 0, 2, 5], 3)
    g = torch.Generator().manual_seed(3)
    v = (torch.rand(1000, generator=g) < 0.6).tolist()
    perm, n = linear_live.partition_reference(v)
    assert sorted(perm) == list(range(1000)) and n == sum(v)
    assert perm[:n] == sorted(perm[:n]) and perm[n:] == sorted(perm[n:])
    assert all(v[i] for i in perm[:n]) and not any(v[i] for i in perm[n:])


@pytest.fixture
def table():
    linear_live.set_table([(4608, 4096, 4096), (288, 512, 256)])
    linear_live.set_enabled(True)
    yield
    linear_live.set_table(None)
    linear_live.set_enabled(True)


def test_routing_predicate(table):
    ok = dict(rows=4608, n=4096, k=4096, dtype=torch.bfloat16, has_bias=False, have_partition=True)
    assert linear_live.routed(**ok)
    assert not linear_live.routed(**{**ok, "dtype": torch.float32})
    assert not linear_live.routed(**{**ok, "dtype": torch.float16})
    assert not linear_live.routed(**{**ok, "has_bias": True})
    assert not linear_live.routed(**{**ok, "have_partition": False})          # outside a padded tower call
    assert not linear_live.routed(**{**ok, "rows": 4607})                     # another row count: not in the table
    assert not linear_live.routed(**{**ok, "n": 11008})
    assert linear_live.routed(**{**ok, "rows": 288, "n": 512, "k": 256})
    linear_live.set_enabled(False)
    assert not linear_live.routed(**ok) and not linear_live.enabled()
    linear_live.set_enabled(True)
    assert linear_live.routed(**ok)


def test_shapes_the_kernel_cannot_take_never_route():
    linear_live.set_table([(16, 12, 64), (16, 8, 96), (16, 8, 64)])
    try:
        kw = dict(dtype=torch.bfloat16, has_bias=False, have_partition=True)
        assert not linear_live.routed(16, 12, 64, **kw)                        # N % 8
        assert not linear_live.routed(16, 8, 96, **kw)                         # K % 64
        assert linear_live.routed(16, 8, 64, **kw)
    finally:
        linear_live.set_table(None)


def test_measured_table_holds_only_padded_step_shapes():
    shapes = {(4608, 4096, 4096), (4608, 12288, 4096), (4608, 22016, 4096), (4608, 4096, 11008), (4608, 11008, 4096),
              (4608, 32000, 4096), (4608, 4096, 32000)}
    assert set(linear_live.ROUTED_SHAPES) <= shapes
    assert linear_live.routed(4608, 22016, 4096, dtype=torch.bfloat16, has_bias=False, have_partition=True)


# (N, live tiles, all tiles, rounds on 256 CUs) at 2830 live of 4608 rows, 256 x 256 tiles: the issue's estimate table
TABLE = [
    (4096, 192, 288, 1),        # o_proj fwd / o dgrad, each q|k|v dgrad member, gate / up dgrad, down fwd
    (12288, 576, 864, 3),       # q|k|v fwd
    (22016, 1032, 1548, 5),     # gate|up fwd
    (11008, 516, 774, 3),       # down dgrad: 2.02 rounds cost 3
]


@pytest.mark.parametrize("n,live_tiles,all_tiles,nrounds", TABLE)
def test_tile_accounting_reproduces_the_estimate_table(n, live_tiles, all_tiles, nrounds):
    assert linear_live.tiles(2830, n) == live_tiles
    assert linear_live.tiles(4608, n) == all_tiles
    assert linear_live.rounds(2830, n) == nrounds


def test_tile_quantisation_of_the_down_dgrad():
    """12 row tiles of 256 x 43 column tiles = 516 = 2.02 rounds; with 11 row tiles (2816 rows) it would be 2; the 128-row form
    has 23 x 43 = 989 half-size tiles = 4 rounds of half the work."""
    assert linear_live.rounds(2816, 11008) == 2 and linear_live.rounds(2817, 11008) == 3
    assert linear_live.tiles(2830, 11008, tile_rows=128) == 989 and linear_live.rounds(2830, 11008, tile_rows=128) == 4
    assert linear_live.flops(2830, 4096, 4096) == 2 * 2830 * 4096 * 4096
