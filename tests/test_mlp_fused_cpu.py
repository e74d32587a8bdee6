"""The routing predicate of the fused frozen-MLP node (models/frozen_linear.py `swiglu_mlp_candidate` / `swiglu_mlp_route`,
linear_live.mlp_routed) without a GPU: every single condition, when false, makes the call fall back to the separate nodes."""
import pytest
import torch

from dalm_amd import linear_live
from dalm_amd.models import frozen_linear

ROWS, H, C = 192, 256, 384
SHAPES = [(ROWS, 2 * C, H), (ROWS, H, C), (ROWS, C, H)]        # gate | up forward; down forward = gate / up dgrad; down dgrad


@pytest.fixture
def table():
    linear_live.set_table(SHAPES)
    linear_live.set_enabled(True)
    linear_live.set_mlp_fused(True)
    yield
    linear_live.set_table(None)
    linear_live.set_enabled(True)
    linear_live.set_mlp_fused(True)


def _mlp(c=C, h=H, dtype=torch.bfloat16, bias=False, cls=torch.nn.Linear):
    mods = [cls(h, c, bias=bias, device="meta", dtype=dtype), cls(h, c, bias=bias, device="meta", dtype=dtype),
            cls(c, h, bias=bias, device="meta", dtype=dtype)]
    for m in mods:
        m.requires_grad_(False)
    return mods


def _x(rows=ROWS, h=H, dtype=torch.bfloat16):
    return torch.empty(2, rows // 2, h, device="meta", dtype=dtype, requires_grad=True)


def test_default_is_on():
    assert linear_live.mlp_fused()


def test_shape_predicate(table):
    ok = dict(rows=ROWS, c=C, h=H, dtype=torch.bfloat16, has_bias=False, have_partition=True)
    assert linear_live.mlp_routed(**ok)
    assert not linear_live.mlp_routed(**{**ok, "dtype": torch.float32})
    assert not linear_live.mlp_routed(**{**ok, "has_bias": True})
    assert not linear_live.mlp_routed(**{**ok, "have_partition": False})
    assert not linear_live.mlp_routed(**{**ok, "rows": ROWS + 1})
    for drop in range(3):                                          # each of the node's GEMM shapes must be in the table
        linear_live.set_table(SHAPES[:drop] + SHAPES[drop + 1:])
        assert not linear_live.mlp_routed(**ok), SHAPES[drop]
    linear_live.set_table(SHAPES)
    linear_live.set_mlp_fused(False)
    assert not linear_live.mlp_routed(**ok) and not linear_live.mlp_fused()
    linear_live.set_mlp_fused(True)
    linear_live.set_enabled(False)
    assert not linear_live.mlp_routed(**ok)
    linear_live.set_enabled(True)
    assert linear_live.mlp_routed(**ok)


def test_c_must_be_whole_mixed_tiles(table):
    c = 448                                                        # % 64 == 0 (the GEMMs take it, as N and as K), % 128 != 0
    linear_live.set_table([(ROWS, 2 * c, H), (ROWS, H, c), (ROWS, c, H)])
    kw = dict(dtype=torch.bfloat16, has_bias=False, have_partition=True)
    assert all(linear_live.routed(*s, **kw) for s in [(ROWS, 2 * c, H), (ROWS, H, c), (ROWS, c, H)])
    assert not linear_live.mlp_routed(ROWS, c, H, **kw)
    assert frozen_linear.swiglu_mlp_candidate(_x(), *_mlp(c=c)) is None


def test_candidate_conditions(table):
    assert frozen_linear.swiglu_mlp_candidate(_x(), *_mlp()) == (ROWS, C, H)
    assert frozen_linear.swiglu_mlp_candidate(_x(), *_mlp(cls=frozen_linear.FrozenLinearT)) == (ROWS, C, H)
    assert frozen_linear.swiglu_mlp_candidate(_x(dtype=torch.float32), *_mlp()) is None                 # fp32 activations
    assert frozen_linear.swiglu_mlp_candidate(_x(dtype=torch.float32), *_mlp(dtype=torch.float32)) is None
    assert frozen_linear.swiglu_mlp_candidate(_x(), *_mlp(bias=True)) is None
    assert frozen_linear.swiglu_mlp_candidate(_x(rows=ROWS - 2), *_mlp()) is None                       # rows not in the table
    for i in range(3):
        mods = _mlp()
        mods[i].weight.requires_grad_(True)                                                             # one projection trainable
        assert frozen_linear.swiglu_mlp_candidate(_x(), *mods) is None, i
        mods = _mlp()

        class Wrapped(torch.nn.Linear):                                                                 # not a plain projection
            pass

        mods[i].__class__ = Wrapped
        assert frozen_linear.swiglu_mlp_candidate(_x(), *mods) is None, i
        mods = _mlp()
        mods[i].weight.data = mods[i].weight.data.to(torch.float32)                                     # one weight not bf16
        assert frozen_linear.swiglu_mlp_candidate(_x(), *mods) is None, i
    linear_live.set_mlp_fused(False)
    assert frozen_linear.swiglu_mlp_candidate(_x(), *_mlp()) is None
    linear_live.set_mlp_fused(True)
    linear_live.set_enabled(False)
    assert frozen_linear.swiglu_mlp_candidate(_x(), *_mlp()) is None


def test_cpu_tensors_never_route(table):
    mods = [torch.nn.Linear(H, C, bias=False, dtype=torch.bfloat16), torch.nn.Linear(H, C, bias=False, dtype=torch.bfloat16),
            torch.nn.Linear(C, H, bias=False, dtype=torch.bfloat16)]
    for m in mods:
        m.requires_grad_(False)
    x = torch.zeros(2, ROWS // 2, H, dtype=torch.bfloat16, requires_grad=True)
    assert frozen_linear.swiglu_mlp_candidate(x, *mods) == (ROWS, C, H)
    assert frozen_linear.swiglu_mlp_forward(x, *mods) is None


def test_device_side_conditions_fall_back(table, monkeypatch):
    """Past the candidate test, the route needs: an eligible call, the gate | up weights as one tensor, operands the kernel accepts,
    a partition (a padded tower call in progress), the silu table of the device and the transposed dgrad copies.  Each alone, when missing, falls back."""
    x, mods = _x(), _mlp()
    cat, part = object(), (object(), object())
    good = {
        (frozen_linear, "_eligible"): lambda x, *m: True,
        (frozen_linear, "_cat_weights"): lambda *m: cat,
        (linear_live, "accepts"): lambda x2, w, b: True,
        (linear_live, "route"): lambda x2, w, b: part,
        (frozen_linear, "dgrad_weight"): lambda w, dt=None: w,
        (linear_live, "mlp_prepare"): lambda d: True,
    }
    bad = {
        (frozen_linear, "_eligible"): lambda x, *m: False,
        (frozen_linear, "_cat_weights"): lambda *m: None,
        (linear_live, "accepts"): lambda x2, w, b: False,
        (linear_live, "route"): lambda x2, w, b: None,               # no partition: not inside a padded tower call
        (frozen_linear, "dgrad_weight"): lambda w, dt=None: None,
        (linear_live, "mlp_prepare"): lambda d: False,             # first use of the device inside a stream capture
    }
    for (mod, name), fn in good.items():
        monkeypatch.setattr(mod, name, fn)
    for m in mods:                                                   # meta weights: contiguous, data_ptr 0
        assert m.weight.is_contiguous()
    assert frozen_linear.swiglu_mlp_route(x, *mods) == (cat, part)
    for key, fn in bad.items():
        monkeypatch.setattr(key[0], key[1], fn)
        assert frozen_linear.swiglu_mlp_route(x, *mods) is None, key[1]
        monkeypatch.setattr(key[0], key[1], good[key])
    assert frozen_linear.swiglu_mlp_route(x, *mods) == (cat, part)
    linear_live.set_mlp_fused(False)
    assert frozen_linear.swiglu_mlp_route(x, *mods) is None
