"""`dalm_linear_live_swiglu` without a GPU: declared in the header, exported by the library and listed in the ctypes table with
matching arity; every argument error comes back with its DALM_E_* code before anything is enqueued (the pointers below are host
memory: a launch would fail differently)."""
import ctypes as C
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "dalm_hip.h"
NAMES = ("dalm_linear_live_swiglu",)
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -4


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
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in hip.SIGNATURES and len(hip.SIGNATURES[name][1]) == m.group(1).count(",") + 1
        assert m.group(1).rstrip().endswith("dalm_stream_t stream")
    m = re.search(r"\bint dalm_linear_live_swiglu_prepare\s*\(([^)]*)\)", text)
    assert m and hasattr(lib, "dalm_linear_live_swiglu_prepare") and len(hip.SIGNATURES["dalm_linear_live_swiglu_prepare"][1]) == 1


def _buffers():
    raw = (C.c_char * 16384)()
    base = (C.addressof(raw) + 15) & ~15
    return raw, [base + 1024 * i for i in range(8)]


def _fwd(lib, p, R=4, Cc=128, K=64, lda=None, ldy=None, ldact=None, null=None, **over):
    a = dict(A=p[0], W=p[1], Y=p[2], Act=p[3], perm=p[4], n_live=p[5])
    a.update(over)
    args = [a["A"], K if lda is None else lda, a["W"], a["Y"], 2 * Cc if ldy is None else ldy, a["Act"], Cc if ldact is None else ldact,
            R, Cc, K, a["perm"], a["n_live"], None]
    if null is not None:
        args[null] = None
    return lib.dalm_linear_live_swiglu(*args)


def test_null_pointers(lib):
    raw, p = _buffers()
    for null in (0, 2, 3, 5, 10, 11):                     # A, Wcat, Y, Act, perm, n_live
        assert _fwd(lib, p, null=null) == E_NULL, null
        assert b"null pointer" in lib.dalm_last_error_string()
    del raw


def test_forward_needs_whole_mixed_tiles(lib):
    raw, p = _buffers()
    for bad in (dict(Cc=0), dict(Cc=-128), dict(Cc=8), dict(Cc=64), dict(Cc=392), dict(Cc=11000)):
        assert _fwd(lib, p, **bad) == E_SHAPE, bad
        assert b"multiple of 128" in lib.dalm_last_error_string()
    del raw


def test_contraction_depth_is_a_multiple_of_64(lib):
    raw, p = _buffers()
    for bad in (dict(K=0), dict(K=32), dict(K=96), dict(R=0), dict(R=-1)):
        assert _fwd(lib, p, **bad) == E_SHAPE, bad
    assert _fwd(lib, p, K=96) == E_SHAPE and b"multiple of 64" in lib.dalm_last_error_string()
    # operands above 4 GB are refused as in dalm_linear_live
    assert _fwd(lib, p, R=1 << 20, K=4096) == E_SHAPE and b"4 GB" in lib.dalm_last_error_string()
    del raw


def test_row_strides(lib):
    raw, p = _buffers()
    for bad in (dict(lda=56), dict(lda=68), dict(ldy=128), dict(ldy=248), dict(ldy=260), dict(ldact=64), dict(ldact=120),
                dict(ldact=132)):
        assert _fwd(lib, p, **bad) == E_SHAPE, bad
        assert b"row strides" in lib.dalm_last_error_string()
    del raw


def test_alignment(lib):
    raw, p = _buffers()
    for bad in (dict(A=p[0] + 8), dict(W=p[1] + 2), dict(Y=p[2] + 4), dict(Act=p[3] + 8)):
        assert _fwd(lib, p, **bad) == E_ALIGN, bad
        assert b"16-byte aligned" in lib.dalm_last_error_string()
    del raw
