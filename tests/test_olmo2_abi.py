"""OLMo-2's entry points (`dalm_norm_add_{fwd,bwd}`, `dalm_row_norm_rope_fwd`, `dalm_row_norm_bwd`, dalm_amd/csrc/tower.hip) without
a GPU: they exist in the header, the library and the ctypes table with matching arity; the header still compiles as C99; argument
errors come back with a message before anything is enqueued or written; no rows is no work."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "dalm_hip.h"
NAMES = ("dalm_norm_add_fwd", "dalm_norm_add_bwd", "dalm_row_norm_rope_fwd", "dalm_row_norm_bwd")
E_NULL, E_SHAPE, E_DTYPE, E_ALIGN = -1, -2, -3, -4
F32, BF16 = 0, 1
FILL = 0x5A


@pytest.fixture(scope="module")
def lib():
    from dalm_amd import _build, hip

    _build.build(verbose=False)
    return hip.load()


def test_error_codes_are_the_headers():
    text = HEADER.read_text()
    for name, val in (("DALM_E_NULL", E_NULL), ("DALM_E_SHAPE", E_SHAPE), ("DALM_E_DTYPE", E_DTYPE), ("DALM_E_ALIGN", E_ALIGN)):
        assert re.search(r"\b%s\s*=?\s*\(?%d\)?" % (name, val), text), name


def test_entry_points_in_header_library_and_table(lib):
    from dalm_amd import hip

    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in NAMES:
        m = re.search(r"\bint %s\s*\(([^)]*)\)" % name, text)
        assert m, f"{name} is not declared in include/dalm_hip.h"
        args = m.group(1)
        assert "row_live" in args and args.rstrip().endswith("dalm_stream_t stream") and "int w_dtype" in args
        if "row_norm" in name:
            assert "rstd_q" in args and "rstd_k" in args and "int64_t Hq" in args and "int64_t Hk" in args
        else:
            assert "int dtype" in args and "int64_t R" in args and "int64_t D" in args and "rstd" in args
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in hip.SIGNATURES and len(hip.SIGNATURES[name][1]) == args.count(",") + 1
    # the comment in front of them states the rounding points, the liveness contract and which backward kernel is shared
    doc = HEADER.read_text()
    doc = doc[:doc.index("int dalm_norm_add_fwd")]
    doc = doc[doc.rindex("/*"):]
    for word in ("rotate_half", "Row liveness", "dalm_attn_gqa_bwd", "64 or 128", "8192", "dalm_rms_norm_bwd_live", "Olmo2RMSNorm"):
        assert word in doc, word


def test_header_is_still_plain_c(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    src = tmp_path / "olmo2_abi.c"
    body = "\n".join(f"  p[{i}] = (fn_t)&{n};" for i, n in enumerate(NAMES))
    src.write_text(f'#include "dalm_hip.h"\ntypedef void (*fn_t)(void);\nfn_t p[{len(NAMES)}];\nvoid fill(void) {{\n{body}\n}}\n')
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", str(ROOT / "include"), "-c", str(src), "-o",
                        str(tmp_path / "olmo2_abi.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


class _Buffers:
    """Host memory, 16-byte aligned slots of 256 bytes filled with a pattern: the checks under test run before any pointer is read
    or any kernel is enqueued, so after a rejected call every byte still holds the pattern."""

    def __init__(self):
        self.raw = (C.c_char * 8192)()
        C.memset(self.raw, FILL, len(self.raw))
        base = (C.addressof(self.raw) + 15) & ~15
        self.p = [base + 256 * i for i in range(16)]

    def untouched(self) -> bool:
        return bytes(self.raw) == bytes([FILL]) * len(self.raw)


def _rejected(lib, buf, rc, code, word=None):
    assert rc == code, (rc, lib.dalm_last_error_string())
    msg = lib.dalm_last_error_string()
    assert msg and (word is None or word in msg), msg
    assert buf.untouched()


def _add_fwd(lib, p, R=4, D=64, dtype=BF16, w_dtype=BF16, null=None, **over):
    a = dict(x=p[0], res=p[1], w=p[2], out=p[3], rstd=p[4])
    a.update(over)
    args = [a["x"], a["res"], a["w"], dtype, w_dtype, R, D, C.c_float(1e-6), a["out"], a["rstd"], None, None]
    if null is not None:
        args[null] = None
    return lib.dalm_norm_add_fwd(*args)


def _add_bwd(lib, p, R=4, D=64, dtype=BF16, w_dtype=BF16, null=None, **over):
    a = dict(dy=p[0], x=p[1], w=p[2], rstd=p[4], dx=p[3])
    a.update(over)
    args = [a["dy"], a["x"], a["w"], a["rstd"], dtype, w_dtype, R, D, a["dx"], None, None]
    if null is not None:
        args[null] = None
    return lib.dalm_norm_add_bwd(*args)


def _s3(B, H, T, hd):
    return (C.c_int64 * 3)(T * H * hd, hd, H * hd)


def _row_fwd(lib, p, B=1, T=4, Hq=4, Hk=2, hd=64, w_dtype=BF16, null=None, **over):
    a = dict(q=p[0], k=p[1], wq=p[2], wk=p[3], cos=p[4], sin=p[5], qs=_s3(B, Hq, T, hd), ks=_s3(B, Hk, T, hd), qos=_s3(B, Hq, T, hd),
             kos=_s3(B, Hk, T, hd), cs=(C.c_int64 * 2)(0, hd), qo=p[6], ko=p[7], rq=p[8], rk=p[9])
    a.update(over)
    args = [a["q"], a["k"], a["wq"], a["wk"], w_dtype, C.c_float(1e-6), C.c_float(1e-6), a["cos"], a["sin"], B, T, Hq, Hk, hd, a["qs"],
            a["ks"], a["qos"], a["kos"], a["cs"], a["qo"], a["ko"], a["rq"], a["rk"], None, None]
    if null is not None:
        args[null] = None
    return lib.dalm_row_norm_rope_fwd(*args)


def _row_bwd(lib, p, B=1, T=4, Hq=4, Hk=2, hd=64, w_dtype=BF16, null=None, **over):
    a = dict(gq=p[0], gk=p[1], q=p[2], k=p[3], wq=p[4], wk=p[5], rq=p[6], rk=p[7], dq=p[8], dk=p[9])
    for n, H in (("gqs", Hq), ("gks", Hk), ("qs", Hq), ("ks", Hk), ("dqs", Hq), ("dks", Hk)):
        a[n] = _s3(B, H, T, hd)
    a.update(over)
    args = [a["gq"], a["gk"], a["q"], a["k"], a["wq"], a["wk"], w_dtype, a["rq"], a["rk"], B, T, Hq, Hk, hd, a["gqs"], a["gks"], a["qs"],
            a["ks"], a["dqs"], a["dks"], a["dq"], a["dk"], None, None]
    if null is not None:
        args[null] = None
    return lib.dalm_row_norm_bwd(*args)


def test_null_pointers_are_rejected(lib):
    buf = _Buffers()
    for null in (0, 1, 2, 8, 9):
        _rejected(lib, buf, _add_fwd(lib, buf.p, null=null), E_NULL, b"null pointer")
    for null in (0, 1, 2, 3, 8):
        _rejected(lib, buf, _add_bwd(lib, buf.p, null=null), E_NULL, b"null pointer")
    for null in (0, 1, 2, 3, 7, 8, 14, 15, 16, 17, 18, 19, 20, 21, 22):
        _rejected(lib, buf, _row_fwd(lib, buf.p, null=null), E_NULL, b"null pointer")
    for null in (0, 1, 2, 3, 4, 5, 7, 8, 14, 15, 16, 17, 18, 19, 20, 21):
        _rejected(lib, buf, _row_bwd(lib, buf.p, null=null), E_NULL, b"null pointer")


@pytest.mark.parametrize("hd", [32, 96])
def test_other_head_widths_are_shape_errors(lib, hd):
    buf = _Buffers()
    for call in (_row_fwd, _row_bwd):
        _rejected(lib, buf, call(lib, buf.p, hd=hd), E_SHAPE, b"head width")


def test_row_wider_than_8192_is_a_shape_error(lib):
    buf = _Buffers()
    for call in (_row_fwd, _row_bwd):
        _rejected(lib, buf, call(lib, buf.p, Hq=65, Hk=1, hd=128), E_SHAPE, b"8192")       # Hq hd = 8320
        _rejected(lib, buf, call(lib, buf.p, Hq=130, Hk=2, hd=64), E_SHAPE, b"8192")
        _rejected(lib, buf, call(lib, buf.p, B=0), E_SHAPE)
        _rejected(lib, buf, call(lib, buf.p, Hk=0), E_SHAPE)
        _rejected(lib, buf, call(lib, buf.p, T=-1), E_SHAPE)
        _rejected(lib, buf, call(lib, buf.p, B=1 << 20, T=1 << 12), E_SHAPE, b"too large")   # B T (Hq + Hk) hd / 8 reaches 2^31
        _rejected(lib, buf, call(lib, buf.p, w_dtype=2), E_DTYPE)


def test_row_norm_alignment(lib):
    buf = _Buffers()
    p = buf.p
    for call in (_row_fwd, _row_bwd):
        _rejected(lib, buf, call(lib, p, q=p[0] + 2), E_ALIGN, b"aligned")
        _rejected(lib, buf, call(lib, p, wk=p[3] + 8), E_ALIGN)
        _rejected(lib, buf, call(lib, p, qs=(C.c_int64 * 3)(4 * 4 * 64, 64, 4 * 64 + 1)), E_ALIGN)    # an odd row stride
        _rejected(lib, buf, call(lib, p, ks=(C.c_int64 * 3)(4 * 2 * 64 + 4, 64, 2 * 64)), E_ALIGN)
    _rejected(lib, buf, _row_fwd(lib, p, cs=(C.c_int64 * 2)(0, 65)), E_ALIGN)
    _rejected(lib, buf, _row_fwd(lib, p, qo=p[6] + 4), E_ALIGN)
    _rejected(lib, buf, _row_bwd(lib, p, dks=(C.c_int64 * 3)(4 * 2 * 64, 63, 2 * 64)), E_ALIGN)
    _rejected(lib, buf, _row_bwd(lib, p, rq=p[6] + 2), E_ALIGN)


@pytest.mark.parametrize("dtype, w_dtype", [(BF16, BF16), (BF16, F32), (F32, F32), (F32, BF16)])
def test_norm_add_widths_and_alignment(lib, dtype, w_dtype):
    buf = _Buffers()
    p = buf.p
    vec = 4 if dtype == F32 else 8
    cap = 64 * vec * 16                                                            # 8192 (bf16) / 4096 (f32)
    for call in (_add_fwd, _add_bwd):
        kw = dict(dtype=dtype, w_dtype=w_dtype)
        _rejected(lib, buf, call(lib, p, D=vec + 1, **kw), E_SHAPE, b"16 bytes")   # not a multiple of 16 bytes
        _rejected(lib, buf, call(lib, p, D=vec // 2, **kw), E_SHAPE)
        _rejected(lib, buf, call(lib, p, D=cap + vec, **kw), E_SHAPE)              # above the cap
        _rejected(lib, buf, call(lib, p, D=0, **kw), E_SHAPE)
        _rejected(lib, buf, call(lib, p, R=-1, **kw), E_SHAPE)
        _rejected(lib, buf, call(lib, p, x=p[1] + 4, **kw), E_ALIGN, b"aligned")
        _rejected(lib, buf, call(lib, p, w=p[2] + 8, **kw), E_ALIGN)
        _rejected(lib, buf, call(lib, p, dtype=2, w_dtype=w_dtype), E_DTYPE)
        _rejected(lib, buf, call(lib, p, dtype=dtype, w_dtype=7), E_DTYPE)
    _rejected(lib, buf, _add_fwd(lib, p, out=p[3] + 2, **kw), E_ALIGN)
    _rejected(lib, buf, _add_fwd(lib, p, res=p[1] + 8, **kw), E_ALIGN)
    _rejected(lib, buf, _add_bwd(lib, p, dx=p[3] + 2, **kw), E_ALIGN)
    _rejected(lib, buf, _add_bwd(lib, p, dy=p[0] + 8, **kw), E_ALIGN)


@pytest.mark.parametrize("dtype, w_dtype", [(BF16, BF16), (BF16, F32), (F32, F32), (F32, BF16)])
def test_no_rows_is_no_work(lib, dtype, w_dtype):
    buf = _Buffers()
    for call in (_add_fwd, _add_bwd):
        assert call(lib, buf.p, R=0, D=64, dtype=dtype, w_dtype=w_dtype) == 0
        assert buf.untouched()
        # the width rules hold with no rows as well
        _rejected(lib, buf, call(lib, buf.p, R=0, D=3, dtype=dtype, w_dtype=w_dtype), E_SHAPE)
