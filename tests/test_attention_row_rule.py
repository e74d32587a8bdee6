"""`helpers.assert_rows_close` itself, on the CPU: the per-row rule of tests/test_attention_extents_gpu.py rejects a single row
that is 5 % off in a [1, 2, 2048, 64] tensor, which the whole-tensor rule of the other attention tests ("no further from float64
than torch, x 1.5 + 1e-3") accepts: one row of 4096 moves the relative norm by 0.05 / sqrt(4096) = 7.8e-4, inside the 1e-3."""
import pytest
import torch

from helpers import ROW_FACTOR, ROW_OFFSET, assert_rows_close, norm_rel_err, row_errors, rows_report


@pytest.fixture(scope="module")
def tensors():
    g = torch.Generator().manual_seed(2048)
    ref = torch.randn(1, 2, 2048, 64, generator=g, dtype=torch.float64)
    return ref, ref.bfloat16()


@pytest.mark.parametrize("i", [2047, 1024])
def test_one_row_5_percent_off_passes_the_norm_rule_and_fails_the_row_rule(tensors, i):
    ref, torch_got = tensors
    got = torch_got.clone()
    got[0, 1, i] = (got[0, 1, i].float() * 1.05).bfloat16()
    assert norm_rel_err(got, ref) <= ROW_FACTOR * norm_rel_err(torch_got, ref) + ROW_OFFSET      # the whole-tensor rule accepts it
    rep = rows_report(got, torch_got, ref)
    assert rep["finite"] and rep["norm_ok"] and not rep["rows_ok"]
    assert rep["worst_row"] == [0, 1, i]
    with pytest.raises(AssertionError, match=rf"per-row rule - x: worst row \(b, h, i\) = \(0, 1, {i}\), i % 32 = {i % 32}, "):
        assert_rows_close("x", got, torch_got, ref)


def test_the_row_rule_accepts_the_yardstick_and_scales_dead_rows_by_the_tensor(tensors):
    ref, torch_got = tensors
    assert_rows_close("same", torch_got, torch_got, ref)
    # a row whose reference is zero is measured against the RMS row norm: no division by zero, a small absolute error stays small
    ref0 = ref.clone()
    ref0[0, 0, 5] = 0.0
    got = ref0.bfloat16()
    got[0, 0, 5, 0] = 1e-3
    e = row_errors(got, ref0)
    s = float(ref0.norm(dim=-1).square().mean().sqrt())
    assert abs(float(e[0, 0, 5]) - 1e-3 / s) < 1e-6 and torch.isfinite(e).all()
    # not finite: rejected whatever the norms say
    bad = torch_got.clone()
    bad[0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError):
        assert_rows_close("nan", bad, torch_got, ref)
