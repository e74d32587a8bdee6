"""Gemma's entry points (`dalm_geglu_{fwd,bwd}`, `dalm_gemma_norm_{fwd,bwd}`, dalm_amd/csrc/tower.hip) without a GPU: they exist in
the header, the library and the ctypes table with matching arity, and argument errors come back with the codes of their Llama
siblings (`dalm_swiglu_*_2d_live`, `dalm_rms_norm_*_live`) before anything is enqueued."""
import ctypes as C
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "dalm_hip.h"
NAMES = ("dalm_geglu_fwd", "dalm_geglu_bwd", "dalm_gemma_norm_fwd", "dalm_gemma_norm_bwd")
E_NULL, E_SHAPE, E_DTYPE, E_ALIGN = -1, -2, -3, -4
F32, BF16 = 0, 1


@pytest.fixture(scope="module")
def lib():
    from dalm_amd import _build, hip

    _build.build(verbose=False)
    return hip.load()


def test_entry_points_in_header_library_and_table(lib):
    from dalm_amd import hip

    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in NAMES:
        m = re.search(r"\bint %s\s*\(([^)]*)\)" % name, text)
        assert m, f"{name} is not declared in include/dalm_hip.h"
        assert "const uint8_t* row_live" in m.group(1) and m.group(1).rstrip().endswith("dalm_stream_t stream")
        assert ("w_dtype" in m.group(1)) == ("norm" in name)
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in hip.SIGNATURES and len(hip.SIGNATURES[name][1]) == m.group(1).count(",") + 1
    # one entry point per direction: no `_live` / `_2d` twins
    assert not [n for n in hip.SIGNATURES if n.startswith(("dalm_geglu", "dalm_gemma")) and n not in NAMES]


def _buffers():
    """Host memory, 16-byte aligned: the checks under test run before any pointer is read or any kernel is enqueued."""
    raw = (C.c_char * 8192)()
    base = (C.addressof(raw) + 15) & ~15
    return raw, [base + 256 * i for i in range(16)]


def _geglu_fwd(lib, p, R=4, C_=16, dtype=BF16, null=None, ld=None, **over):
    a = dict(gate=p[0], up=p[1], act=p[2])
    a.update(over)
    ld = ld or (C_, C_, C_)
    args = [a["gate"], a["up"], a["act"], dtype, R, C_, *ld, None, None]
    if null is not None:
        args[null] = None
    return lib.dalm_geglu_fwd(*args)


def _geglu_bwd(lib, p, R=4, C_=16, dtype=BF16, null=None, ld=None, **over):
    a = dict(d_act=p[0], gate=p[1], up=p[2], d_gate=p[3], d_up=p[4])
    a.update(over)
    ld = ld or (C_,) * 5
    args = [a["d_act"], a["gate"], a["up"], a["d_gate"], a["d_up"], dtype, R, C_, *ld, None, None]
    if null is not None:
        args[null] = None
    return lib.dalm_geglu_bwd(*args)


def _norm_fwd(lib, p, R=4, D=16, dtype=BF16, w_dtype=BF16, add=True, null=None, **over):
    a = dict(x=p[0], delta=p[1] if add else None, w=p[2], h_out=p[3] if add else None, y=p[4], rstd=p[5])
    a.update(over)
    args = [a["x"], a["delta"], a["w"], dtype, w_dtype, R, D, C.c_float(1e-6), a["h_out"], a["y"], a["rstd"], None, None]
    if null is not None:
        args[null] = None
    return lib.dalm_gemma_norm_fwd(*args)


def _norm_bwd(lib, p, R=4, D=16, dtype=BF16, w_dtype=BF16, null=None, **over):
    a = dict(dy=p[0], h=p[1], w=p[2], rstd=p[3], dres=p[4], dx=p[5])
    a.update(over)
    args = [a["dy"], a["h"], a["w"], a["rstd"], a["dres"], dtype, w_dtype, R, D, a["dx"], None, None]
    if null is not None:
        args[null] = None
    return lib.dalm_gemma_norm_bwd(*args)


def test_null_pointers_are_rejected(lib):
    raw, p = _buffers()
    for null in (0, 1, 2):
        assert _geglu_fwd(lib, p, null=null) == E_NULL, null
        assert b"null pointer" in lib.dalm_last_error_string()
    for null in (0, 1, 2, 3, 4):
        assert _geglu_bwd(lib, p, null=null) == E_NULL, null
    for null in (0, 2, 9, 10):                           # x, w, y, rstd
        assert _norm_fwd(lib, p, null=null) == E_NULL, null
    assert _norm_fwd(lib, p, null=1) == E_NULL and _norm_fwd(lib, p, null=8) == E_NULL      # delta and h_out go together
    assert b"go together" in lib.dalm_last_error_string()
    for null in (0, 1, 2, 3, 9):                         # dy, h, w, rstd, dx (dres is optional)
        assert _norm_bwd(lib, p, null=null) == E_NULL, null
    del raw


def test_widths_that_are_no_multiple_of_the_vector(lib):
    raw, p = _buffers()
    # GeGLU: the code of dalm_swiglu_*_2d_live (alignment); 8 elements of bf16, 4 of f32
    for call in (_geglu_fwd, _geglu_bwd):
        assert call(lib, p, C_=12) == E_ALIGN and call(lib, p, C_=6, dtype=F32) == E_ALIGN
        assert call(lib, p, C_=16, ld=(20,) * (3 if call is _geglu_fwd else 5)) == E_ALIGN      # a stride of 40 bytes
        assert call(lib, p, C_=16, ld=(8,) * (3 if call is _geglu_fwd else 5)) == E_ALIGN       # a stride below C
        assert call(lib, p, gate=p[1] + 2) == E_ALIGN
        assert call(lib, p, R=-1) == E_SHAPE and call(lib, p, R=1 << 20, C_=1 << 12) == E_SHAPE  # R C reaches 2^32
        # products past 2^63 wrap in int64: bounded before they are taken
        assert call(lib, p, R=(1 << 32) - 8, C_=(1 << 32) - 8) == E_SHAPE and call(lib, p, R=1 << 40, C_=1 << 24) == E_SHAPE
    # the norm: the code of dalm_rms_norm_*_live (shape), for the width and for the limit
    for call in (_norm_fwd, _norm_bwd):
        assert call(lib, p, D=12) == E_SHAPE and call(lib, p, D=6, dtype=F32) == E_SHAPE and call(lib, p, D=0) == E_SHAPE
        assert b"multiple of 16 bytes" in lib.dalm_last_error_string()
        assert call(lib, p, D=8192 + 8) == E_SHAPE and call(lib, p, D=4096 + 4, dtype=F32) == E_SHAPE
        assert call(lib, p, R=-1) == E_SHAPE
        assert call(lib, p, w=p[2] + 4) == E_ALIGN
    assert _norm_fwd(lib, p, y=p[4] + 8) == E_ALIGN and _norm_bwd(lib, p, dres=p[4] + 2) == E_ALIGN
    del raw


@pytest.mark.parametrize("bad", [2, -1, 7])
def test_dtype_codes(lib, bad):
    raw, p = _buffers()
    for call in (_geglu_fwd, _geglu_bwd, _norm_fwd, _norm_bwd):
        assert call(lib, p, dtype=bad) == E_DTYPE
    for call in (_norm_fwd, _norm_bwd):
        assert call(lib, p, w_dtype=bad) == E_DTYPE
        assert b"w_dtype" in lib.dalm_last_error_string()
    del raw


def test_no_rows_is_not_an_error(lib):
    raw, p = _buffers()
    for call in (_geglu_fwd, _geglu_bwd, _norm_fwd, _norm_bwd):
        assert call(lib, p, R=0) == 0
    assert _norm_fwd(lib, p, R=0, add=False) == 0 and _norm_fwd(lib, p, R=0, w_dtype=F32) == 0
    del raw
