"""The relative-position-bias attention entry points (`dalm_attn_rel_*`, MPNet) without a launch: the four symbols exist and every
argument error of include/dalm_hip.h comes back with its code before anything is enqueued (host pointers throughout)."""
import ctypes as C

import pytest

E_NULL, E_SHAPE, E_ALIGN = -1, -2, -4
NAMES = ("dalm_attn_rel_fwd", "dalm_attn_rel_bwd", "dalm_attn_rel_fwd_packed", "dalm_attn_rel_bwd_packed")


@pytest.fixture(scope="module")
def lib():
    from dalm_amd import _build, hip

    _build.build(verbose=False)
    return hip.load()


def _buffers():
    raw = (C.c_char * 8192)()
    base = (C.addressof(raw) + 15) & ~15
    return raw, [base + 256 * i for i in range(20)]


def _strides(n, H, T, hd):
    return (C.c_int64 * (3 * n))(*([hd * H * T, hd * T, hd] * n))


def _call(lib, name, p, hd=64, T=64, rel="ok", stride_h=None, rel_T=None, cols=None, H=2):
    rel_T = T if rel_T is None else rel_T
    stride_h = 2 * rel_T - 1 if stride_h is None else stride_h
    relp = p[16] if rel == "ok" else rel
    packed = name.endswith("_packed")
    relargs = [relp, stride_h, rel_T] + ([cols] if packed else [])
    if "_fwd" in name:
        q, k, v, rows, live, o, lse, cu = p[:8]
        args = [q, k, v, rows, live] + ([cu] if packed else []) + [1, H, T, hd, C.c_float(0.125), _strides(4, H, T, hd)] + relargs + [
            C.c_float(0.0), None, 0, o, lse, None]
    else:
        q, k, v, o, d_o, lse, rows, cols_bits, live, dq, dk, dv, delta, cu = p[:14]
        args = [q, k, v, o, d_o, lse, rows, cols_bits, live] + ([cu] if packed else []) + [1, H, T, hd, C.c_float(0.125),
                                                                                          _strides(8, H, T, hd)] + relargs + [
            C.c_float(0.0), None, 0, dq, dk, dv, delta, None]
    return getattr(lib, name)(*args)


def test_symbols_are_exported_and_declared(lib):
    from dalm_amd import hip

    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in hip.SIGNATURES


@pytest.mark.parametrize("name", NAMES)
def test_argument_errors(lib, name):
    raw, p = _buffers()
    assert _call(lib, name, p, rel=None) == E_NULL, lib.dalm_last_error_string()
    for hd in (32, 128, 48):
        assert _call(lib, name, p, hd=hd) == E_SHAPE
        assert b"head width" in lib.dalm_last_error_string()
    assert _call(lib, name, p, T=64, rel_T=63) == E_SHAPE and b"rel_T" in lib.dalm_last_error_string()
    assert _call(lib, name, p, T=64, rel_T=64, stride_h=126) == E_SHAPE and b"rel_stride_h" in lib.dalm_last_error_string()
    assert _call(lib, name, p, rel=p[16] + 2) == E_ALIGN and b"4-byte" in lib.dalm_last_error_string()
    # the bias-free rules stay: T <= 2048, 16-byte tensors, dropout needs a seed
    assert _call(lib, name, p, T=2049, rel_T=2049) == E_SHAPE
    moved = list(p)
    moved[0] += 8
    assert _call(lib, name, moved) == E_ALIGN and b"16-byte aligned" in lib.dalm_last_error_string()
    del raw


@pytest.mark.parametrize("name", [n for n in NAMES if n.endswith("_packed")])
def test_packed_forms_need_cu_seqlens(lib, name):
    raw, p = _buffers()
    q = list(p)
    q[7 if "_fwd" in name else 13] = None
    assert _call(lib, name, q) == E_NULL
    del raw
