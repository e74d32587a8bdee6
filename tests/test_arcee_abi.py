"""Arcee's entry points (`dalm_relu2_{fwd,bwd}`, dalm_amd/csrc/tower.hip; `dalm_linear_live_relu2`, dalm_amd/csrc/linear_live.hip)
without a GPU: declared in the header, exported by the library and listed in the ctypes table with matching arity; argument errors
come back with the codes of their siblings (`dalm_geglu_*`, `dalm_linear_live`) before anything is enqueued - the pointers below are
host memory, a launch would fail differently - and the empty cases are no error."""
import ctypes as C
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "dalm_hip.h"
NAMES = ("dalm_relu2_fwd", "dalm_relu2_bwd", "dalm_linear_live_relu2")
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
        assert m.group(1).rstrip().endswith("dalm_stream_t stream")
        assert ("const uint8_t* row_live" in m.group(1)) == name.startswith("dalm_relu2")
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in hip.SIGNATURES and len(hip.SIGNATURES[name][1]) == m.group(1).count(",") + 1
    # one entry point per direction, no `_live` / `_2d` twins; no table and no prepare call for the GEMM
    assert sorted(n for n in hip.SIGNATURES if "relu2" in n) == sorted(NAMES)
    assert hip.SIGNATURES["dalm_linear_live_relu2"] == hip.SIGNATURES["dalm_linear_live_swiglu"]


def _buffers():
    """Host memory, 16-byte aligned: the checks under test run before any pointer is read or any kernel is enqueued."""
    raw = (C.c_char * 16384)()
    base = (C.addressof(raw) + 15) & ~15
    return raw, [base + 1024 * i for i in range(8)]


def _fwd(lib, p, R=4, C_=16, dtype=BF16, null=None, ld=None, **over):
    a = dict(y=p[0], act=p[1])
    a.update(over)
    args = [a["y"], a["act"], dtype, R, C_, *(ld or (C_, C_)), None, None]
    if null is not None:
        args[null] = None
    return lib.dalm_relu2_fwd(*args)


def _bwd(lib, p, R=4, C_=16, dtype=BF16, null=None, ld=None, **over):
    a = dict(d_act=p[0], y=p[1], d_y=p[2])
    a.update(over)
    args = [a["d_act"], a["y"], a["d_y"], dtype, R, C_, *(ld or (C_,) * 3), None, None]
    if null is not None:
        args[null] = None
    return lib.dalm_relu2_bwd(*args)


def _gemm(lib, p, R=4, Cc=16, K=64, lda=None, ldy=None, ldact=None, null=None, **over):
    a = dict(A=p[0], W=p[1], Y=p[2], Act=p[3], perm=p[4], n_live=p[5])
    a.update(over)
    args = [a["A"], K if lda is None else lda, a["W"], a["Y"], Cc if ldy is None else ldy, a["Act"], Cc if ldact is None else ldact,
            R, Cc, K, a["perm"], a["n_live"], None]
    if null is not None:
        args[null] = None
    return lib.dalm_linear_live_relu2(*args)


def test_null_pointers(lib):
    raw, p = _buffers()
    for null in (0, 1):
        assert _fwd(lib, p, null=null) == E_NULL, null
        assert b"null pointer" in lib.dalm_last_error_string()
    for null in (0, 1, 2):
        assert _bwd(lib, p, null=null) == E_NULL, null
    for null in (0, 2, 3, 5, 10, 11):                     # A, Wup, Y, Act, perm, n_live
        assert _gemm(lib, p, null=null) == E_NULL, null
        assert b"null pointer" in lib.dalm_last_error_string()
    del raw


@pytest.mark.parametrize("bad", [2, -1, 7])
def test_dtype_codes(lib, bad):
    raw, p = _buffers()
    for call in (_fwd, _bwd):
        assert call(lib, p, dtype=bad) == E_DTYPE
        assert call(lib, p, dtype=F32, R=0) == 0 and call(lib, p, dtype=BF16, R=0) == 0
    del raw


def test_row_wise_widths_strides_alignment_and_size(lib):
    """dalm_geglu_*'s codes: widths and strides that are no multiple of 16 bytes and misaligned pointers are DALM_E_ALIGN, negative
    extents and R C >= 2^32 are DALM_E_SHAPE (bounded before the product is taken)."""
    raw, p = _buffers()
    for call, n in ((_fwd, 2), (_bwd, 3)):
        assert call(lib, p, C_=12) == E_ALIGN and call(lib, p, C_=6, dtype=F32) == E_ALIGN
        assert call(lib, p, C_=16, ld=(20,) * n) == E_ALIGN                  # a stride of 40 bytes
        assert call(lib, p, C_=16, ld=(8,) * n) == E_ALIGN                   # a stride below C
        for i in range(n):                                                   # every stride is checked on its own
            assert call(lib, p, C_=16, ld=tuple(20 if j == i else 16 for j in range(n))) == E_ALIGN, i
            assert call(lib, p, C_=16, ld=tuple(8 if j == i else 16 for j in range(n))) == E_ALIGN, i
        assert call(lib, p, y=p[1] + 2) == E_ALIGN
        assert b"16-byte aligned" in lib.dalm_last_error_string()
        assert call(lib, p, R=-1) == E_SHAPE and call(lib, p, C_=-8) == E_SHAPE
        assert call(lib, p, R=1 << 20, C_=1 << 12) == E_SHAPE and b"2^32" in lib.dalm_last_error_string()
        assert call(lib, p, R=(1 << 32) - 8, C_=(1 << 32) - 8) == E_SHAPE and call(lib, p, R=1 << 40, C_=1 << 24) == E_SHAPE
    assert _fwd(lib, p, act=p[1] + 8) == E_ALIGN and _bwd(lib, p, d_act=p[0] + 4) == E_ALIGN and _bwd(lib, p, d_y=p[2] + 8) == E_ALIGN
    del raw


def test_gemm_shapes_strides_and_alignment(lib):
    """dalm_linear_live's limits: K % 64, C % 8, strides that cover the row and are multiples of 8, operands below 4 GB, 16-byte
    aligned pointers.  No `C % 128` rule: the tiles are whole 256-column tiles of Wup, partial at the edge."""
    raw, p = _buffers()
    for bad in (dict(K=0), dict(K=32), dict(K=96), dict(K=-64), dict(Cc=4), dict(Cc=12), dict(Cc=260), dict(R=-1), dict(Cc=-8)):
        assert _gemm(lib, p, **bad) == E_SHAPE, bad
    assert _gemm(lib, p, K=96) == E_SHAPE and b"multiple of 64" in lib.dalm_last_error_string()
    assert _gemm(lib, p, R=1 << 20, K=4096) == E_SHAPE and b"4 GB" in lib.dalm_last_error_string()
    for bad in (dict(lda=56), dict(lda=68), dict(ldy=8), dict(ldy=20), dict(ldact=8), dict(ldact=20)):
        assert _gemm(lib, p, **bad) == E_SHAPE, bad
        assert b"row strides" in lib.dalm_last_error_string()
    for bad in (dict(A=p[0] + 8), dict(W=p[1] + 2), dict(Y=p[2] + 4), dict(Act=p[3] + 8)):
        assert _gemm(lib, p, **bad) == E_ALIGN, bad
        assert b"16-byte aligned" in lib.dalm_last_error_string()
    del raw


def test_the_empty_cases_return_zero(lib):
    raw, p = _buffers()
    for call in (_fwd, _bwd):
        assert call(lib, p, R=0) == 0 and call(lib, p, C_=0, ld=(0, 0, 0)[:2 if call is _fwd else 3]) == 0
        assert call(lib, p, R=0, C_=0) == 0
    assert _gemm(lib, p, R=0) == 0 and _gemm(lib, p, Cc=0) == 0 and _gemm(lib, p, R=0, Cc=0) == 0
    del raw
