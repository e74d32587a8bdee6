"""`dalm_row_partition` / `dalm_linear_live` without a GPU: declared in the header, exported by the
library and listed in the ctypes table with matching arity; every argument error comes back with its DALM_E_* code before
anything is enqueued (the pointers below are host memory: a launch would fail differently)."""
import ctypes as C
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "dalm_hip.h"
NAMES = ("dalm_row_partition", "dalm_linear_live")
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


def _buffers():
    raw = (C.c_char * 8192)()
    base = (C.addressof(raw) + 15) & ~15
    return raw, [base + 1024 * i for i in range(6)]


def _linear(lib, p, R=4, N=8, K=64, lda=None, ldc=None, accumulate=0, null=None, **over):
    a = dict(A=p[0], W=p[1], C=p[2], perm=p[3], n_live=p[4])
    a.update(over)
    args = [a["A"], K if lda is None else lda, a["W"], a["C"], N if ldc is None else ldc, R, N, K, a["perm"], a["n_live"],
            accumulate, None]
    if null is not None:
        args[null] = None
    return lib.dalm_linear_live(*args)


def test_null_pointers(lib):
    raw, p = _buffers()
    for null in (0, 2, 3, 8, 9):                          # A, W, C, perm, n_live
        assert _linear(lib, p, null=null) == E_NULL, null
        assert b"null pointer" in lib.dalm_last_error_string()
    assert lib.dalm_row_partition(None, 4, p[3], p[4], None) == E_NULL
    assert lib.dalm_row_partition(p[0], 4, None, p[4], None) == E_NULL
    assert lib.dalm_row_partition(p[0], 4, p[3], None, None) == E_NULL
    del raw


def test_shapes(lib):
    raw, p = _buffers()
    for bad in (dict(R=0), dict(R=-1), dict(N=0), dict(K=0), dict(K=96), dict(K=32), dict(N=12), dict(N=4)):
        assert _linear(lib, p, **bad) == E_SHAPE, bad
    assert b"multiple of 64" in lib.dalm_last_error_string()
    # row strides: at least the width, multiples of 8 elements
    for bad in (dict(lda=56), dict(lda=68), dict(ldc=4), dict(N=16, ldc=20), dict(N=16, ldc=8)):
        assert _linear(lib, p, **bad) == E_SHAPE, bad
    assert b"row strides" in lib.dalm_last_error_string()
    for bad in (dict(accumulate=2), dict(accumulate=-1)):
        assert _linear(lib, p, **bad) == E_SHAPE, bad
    # operands above 4 GB: the A span (R + 256) lda 2 bytes, the W span (N + 256) K 2 bytes
    assert _linear(lib, p, R=1 << 20, K=4096) == E_SHAPE and b"4 GB" in lib.dalm_last_error_string()
    assert _linear(lib, p, R=4, K=64, lda=1 << 30) == E_SHAPE
    assert _linear(lib, p, N=1 << 20, K=4096) == E_SHAPE
    assert _linear(lib, p, R=1 << 40, K=1 << 24) == E_SHAPE            # a product that would wrap in int64 is bounded first
    assert lib.dalm_row_partition(p[0], 0, p[3], p[4], None) == E_SHAPE
    assert lib.dalm_row_partition(p[0], -5, p[3], p[4], None) == E_SHAPE
    assert lib.dalm_row_partition(p[0], 1 << 31, p[3], p[4], None) == E_SHAPE
    del raw


def test_alignment(lib):
    raw, p = _buffers()
    for bad in (dict(A=p[0] + 8), dict(W=p[1] + 2), dict(C=p[2] + 4)):
        assert _linear(lib, p, **bad) == E_ALIGN, bad
    assert b"16-byte aligned" in lib.dalm_last_error_string()
    assert lib.dalm_row_partition(p[0], 4, p[3] + 2, p[4], None) == E_ALIGN
    assert lib.dalm_row_partition(p[0], 4, p[3], p[4] + 1, None) == E_ALIGN
    del raw

