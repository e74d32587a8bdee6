"""Qwen3's head-norm + rotary entry points (`dalm_head_norm_rope_fwd` / `dalm_head_norm_bwd`, dalm_amd/csrc/tower.hip) without a
GPU: they exist in the header, the library and the ctypes table with matching arity; the header still compiles as C99; and
argument errors come back before anything is enqueued."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "dalm_hip.h"
NAMES = ("dalm_head_norm_rope_fwd", "dalm_head_norm_bwd")
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
        assert "row_live" in m.group(1) and m.group(1).rstrip().endswith("dalm_stream_t stream")
        assert "rstd_q" in m.group(1) and "rstd_k" in m.group(1) and "int64_t Hq" in m.group(1) and "int64_t Hk" in m.group(1)
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in hip.SIGNATURES and len(hip.SIGNATURES[name][1]) == m.group(1).count(",") + 1
    # the comment in front of them states the rounding points and the liveness contract
    doc = HEADER.read_text()
    doc = doc[:doc.index("int dalm_head_norm_rope_fwd")]
    doc = doc[doc.rindex("/*"):]
    assert "rotate_half" in doc and "Row liveness" in doc and "dalm_attn_gqa_bwd" in doc and "64 or 128" in doc


def test_header_is_still_plain_c(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    src = tmp_path / "qwen3_abi.c"
    body = "\n".join(f"  p[{i}] = (fn_t)&{n};" for i, n in enumerate(NAMES))
    src.write_text(f'#include "dalm_hip.h"\ntypedef void (*fn_t)(void);\nfn_t p[{len(NAMES)}];\nvoid fill(void) {{\n{body}\n}}\n')
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", str(ROOT / "include"), "-c", str(src), "-o",
                        str(tmp_path / "qwen3_abi.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _buffers():
    """Host memory, 16-byte aligned: the checks under test run before any pointer is read or any kernel is enqueued."""
    raw = (C.c_char * 8192)()
    base = (C.addressof(raw) + 15) & ~15
    return raw, [base + 256 * i for i in range(16)]


def _s3(B, H, T, hd):
    return (C.c_int64 * 3)(T * H * hd, hd, H * hd)


def _fwd(lib, p, B=1, T=4, Hq=4, Hk=2, hd=64, null=None, **over):
    a = dict(q=p[0], k=p[1], wq=p[2], wk=p[3], cos=p[4], sin=p[5], qs=_s3(B, Hq, T, hd), ks=_s3(B, Hk, T, hd), qos=_s3(B, Hq, T, hd),
             kos=_s3(B, Hk, T, hd), cs=(C.c_int64 * 2)(0, hd), qo=p[6], ko=p[7], rq=p[8], rk=p[9])
    a.update(over)
    args = [a["q"], a["k"], a["wq"], a["wk"], C.c_float(1e-6), C.c_float(1e-6), a["cos"], a["sin"], B, T, Hq, Hk, hd, a["qs"], a["ks"],
            a["qos"], a["kos"], a["cs"], a["qo"], a["ko"], a["rq"], a["rk"], None, None]
    if null is not None:
        args[null] = None
    return lib.dalm_head_norm_rope_fwd(*args)


def _bwd(lib, p, B=1, T=4, Hq=4, Hk=2, hd=64, null=None, **over):
    a = dict(gq=p[0], gk=p[1], q=p[2], k=p[3], wq=p[4], wk=p[5], rq=p[6], rk=p[7], dq=p[8], dk=p[9])
    for n, H in (("gqs", Hq), ("gks", Hk), ("qs", Hq), ("ks", Hk), ("dqs", Hq), ("dks", Hk)):
        a[n] = _s3(B, H, T, hd)
    a.update(over)
    args = [a["gq"], a["gk"], a["q"], a["k"], a["wq"], a["wk"], a["rq"], a["rk"], B, T, Hq, Hk, hd, a["gqs"], a["gks"], a["qs"], a["ks"],
            a["dqs"], a["dks"], a["dq"], a["dk"], None, None]
    if null is not None:
        args[null] = None
    return lib.dalm_head_norm_bwd(*args)


def test_null_pointers_are_rejected(lib):
    raw, p = _buffers()
    for null in (0, 1, 2, 3, 6, 7, 13, 14, 15, 16, 17, 18, 19, 20, 21):
        assert _fwd(lib, p, null=null) == E_NULL, null
        assert b"null pointer" in lib.dalm_last_error_string()
    for null in (0, 1, 2, 3, 4, 5, 6, 7, 13, 14, 15, 16, 17, 18, 19, 20):
        assert _bwd(lib, p, null=null) == E_NULL, null
    del raw


@pytest.mark.parametrize("hd", [32, 96, 256, 0])
def test_other_head_widths_are_shape_errors(lib, hd):
    raw, p = _buffers()
    for call in (_fwd, _bwd):
        assert call(lib, p, hd=hd) == E_SHAPE
        assert b"head width" in lib.dalm_last_error_string()
    del raw


def test_sizes_and_alignment(lib):
    raw, p = _buffers()
    for call in (_fwd, _bwd):
        assert call(lib, p, B=0) == E_SHAPE and call(lib, p, Hk=0) == E_SHAPE and call(lib, p, T=-1) == E_SHAPE
        assert call(lib, p, B=1 << 20, T=1 << 12) == E_SHAPE                         # B T (Hq + Hk) hd / 8 reaches 2^31
        assert call(lib, p, q=p[0] + 2) == E_ALIGN and call(lib, p, wk=p[3] + 8) == E_ALIGN
        assert call(lib, p, qs=(C.c_int64 * 3)(4 * 4 * 64, 64, 4 * 64 + 1)) == E_ALIGN    # an odd row stride
        assert call(lib, p, ks=(C.c_int64 * 3)(4 * 2 * 64 + 4, 64, 2 * 64)) == E_ALIGN
    assert _fwd(lib, p, cs=(C.c_int64 * 2)(0, 65)) == E_ALIGN and _fwd(lib, p, qo=p[6] + 4) == E_ALIGN
    assert _bwd(lib, p, dks=(C.c_int64 * 3)(4 * 2 * 64, 63, 2 * 64)) == E_ALIGN and _bwd(lib, p, rq=p[6] + 2) == E_ALIGN
    del raw
