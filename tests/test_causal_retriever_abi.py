"""Last-token pool entry points (`dalm_pool_last_packed_fwd` / `dalm_pool_last_packed_bwd`, dalm_amd/csrc/pool.hip) without a
GPU: they exist in the header, the library and the ctypes table, and argument errors come back before anything is enqueued
(host buffers: a kernel that ran on them would fault, a check that read them would not care)."""
import ctypes as C
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "dalm_hip.h"
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -4
F32, BF16 = 0, 1
NAMES = ("dalm_pool_last_packed_fwd", "dalm_pool_last_packed_bwd")


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
        assert "const int32_t* cu" in m.group(1) and "int64_t nseq_out" in m.group(1) and "int normalize" in m.group(1)
        assert hasattr(lib, name)
        assert name in hip.SIGNATURES and len(hip.SIGNATURES[name][1]) == m.group(1).count(",") + 1
    from dalm_amd.ops import HipOps
    from dalm_amd import fused

    assert callable(HipOps.pool_last_packed_fwd) and callable(HipOps.pool_last_packed_bwd) and callable(fused.pool_last_packed)


def _buffers():
    raw = (C.c_char * 4096)()
    base = (C.addressof(raw) + 15) & ~15
    return raw, [base + 512 * i for i in range(7)]


def _fwd(lib, p, dtype=BF16, n=64, nseq=4, nseq_out=4, D=4096, ld=None, h_off=0, cu=True, emb=True, h=True):
    ld = D if ld is None else ld
    return lib.dalm_pool_last_packed_fwd(p[0] + h_off if h else None, dtype, p[1] if cu else None, n, nseq, nseq_out, D, 1,
                                         p[2] if emb else None, ld, p[3], None)


def _bwd(lib, p, dtype=BF16, n=64, nseq=4, nseq_out=4, D=4096, ld=None, ld_d=None, dh_off=0, null=None):
    ld = D if ld is None else ld
    ld_d = D if ld_d is None else ld_d
    args = [p[4], ld_d, p[2], ld, p[3], p[1], n, nseq, nseq_out, D, 1, p[0] + dh_off, dtype, None]
    if null is not None:
        args[null] = None
    return lib.dalm_pool_last_packed_bwd(*args)


def test_null_pointers(lib):
    raw, p = _buffers()
    assert _fwd(lib, p, cu=False) == E_NULL
    assert b"null pointer" in lib.dalm_last_error_string()
    assert _fwd(lib, p, h=False) == E_NULL and _fwd(lib, p, emb=False) == E_NULL
    for null in (0, 2, 4, 5, 11):                       # d_emb, emb, norm, cu, dh
        assert _bwd(lib, p, null=null) == E_NULL, null
    del raw


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_shape_errors(lib, call):
    raw, p = _buffers()
    assert call(lib, p, dtype=BF16, D=4100) == E_SHAPE              # 4100 bf16 = 8200 bytes: no multiple of 16
    assert call(lib, p, dtype=BF16, D=8200) == E_SHAPE              # a vector multiple, over the width limit
    assert call(lib, p, dtype=F32, D=8200) == E_SHAPE
    assert call(lib, p, nseq=4, nseq_out=5) == E_SHAPE
    assert call(lib, p, D=4096, ld=4092) == E_SHAPE                 # a leading dimension below D
    del raw


@pytest.mark.parametrize("call,off", [(_fwd, "h_off"), (_bwd, "dh_off")])
def test_alignment_errors_and_the_widths_that_reach_them(lib, call, off):
    raw, p = _buffers()
    assert call(lib, p, **{off: 8}) == E_ALIGN                      # h / dh moved by 8 bytes
    assert b"16-byte" in lib.dalm_last_error_string()
    assert call(lib, p, D=4096, ld=4098) == E_ALIGN                 # ld_emb = D + 2
    # the widest and the narrowest rows pass the shape check: they come back from the alignment check
    assert call(lib, p, dtype=BF16, D=8192, **{off: 8}) == E_ALIGN
    assert call(lib, p, dtype=F32, D=32, **{off: 8}) == E_ALIGN
    assert call(lib, p, dtype=F32, D=8192, ld=8194) == E_ALIGN
    del raw


def test_bwd_leading_dimension_of_d_emb(lib):
    raw, p = _buffers()
    assert _bwd(lib, p, ld_d=4098) == E_ALIGN and _bwd(lib, p, ld_d=4000) == E_SHAPE
    del raw
