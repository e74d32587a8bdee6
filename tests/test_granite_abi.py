"""Granite's entry points (`dalm_rms_norm_scaled_{fwd,bwd}`, `dalm_scale_add`, dalm_amd/csrc/tower.hip) without a GPU: they exist in
the header, the library and the ctypes table with matching arity and argument order; the header still compiles as C99; argument errors
come back with a message before anything is enqueued or written; no rows is no work for `dalm_scale_add`."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "dalm_hip.h"
# name -> the argument names, in the order the issue that introduced them fixes
ARGS = {
    "dalm_rms_norm_scaled_fwd": ["x", "delta", "mult", "w", "dtype", "R", "D", "eps", "h_out", "y", "rstd", "row_live", "stream"],
    "dalm_rms_norm_scaled_bwd": ["dy", "h", "w", "rstd", "dres", "mult", "dtype", "R", "D", "dx", "ddelta", "row_live", "stream"],
    "dalm_scale_add": ["res", "x", "mult", "out", "dtype", "R", "D", "row_live", "stream"],
}
E_NULL, E_SHAPE, E_DTYPE, E_ALIGN = -1, -2, -3, -4
F32, BF16 = 0, 1
FILL = 0x5A


@pytest.fixture(scope="module")
def lib():
    from dalm_amd import _build, hip

    _build.build(verbose=False)
    return hip.load()


def test_entry_points_in_header_library_and_table(lib):
    from dalm_amd import hip

    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name, want in ARGS.items():
        m = re.search(r"\bint %s\s*\(([^)]*)\)" % name, text)
        assert m, f"{name} is not declared in include/dalm_hip.h"
        decl = [a.strip() for a in m.group(1).split(",")]
        assert [re.split(r"[\s*]+", a)[-1] for a in decl] == want, (name, decl)
        kinds = {a: d for a, d in zip(want, decl)}
        assert kinds["mult"] == "float mult" and kinds["dtype"] == "int dtype" and kinds["row_live"] == "const uint8_t* row_live"
        assert kinds["R"] == "int64_t R" and kinds["D"] == "int64_t D" and kinds["stream"] == "dalm_stream_t stream"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        res, table = hip.SIGNATURES[name]
        assert res is C.c_int and len(table) == len(want)
        for a, d, t in zip(want, decl, table):                       # floats where the header has floats, 64-bit sizes, pointers
            assert t is (C.c_float if d.startswith("float ") else C.c_int64 if d.startswith("int64_t ") else C.c_int
                         if d.startswith("int ") else C.c_void_p), (name, a, d, t)
    # the comment in front of them states the rounding points, the liveness contract and the equality with the unscaled kernels
    doc = HEADER.read_text()
    doc = doc[:doc.index("int dalm_rms_norm_scaled_fwd")]
    doc = doc[doc.rindex("/*"):]
    for word in ("residual_multiplier", "Row liveness", "rb(delta mult)", "ddelta", "mult == 1", "dalm_rms_norm_bwd_live", "8192", "4096",
                 "res == NULL", "logits_scaling", "writes nothing"):
        assert word in doc, word


def test_header_is_still_plain_c(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    src = tmp_path / "granite_abi.c"
    body = "\n".join(f"  p[{i}] = (fn_t)&{n};" for i, n in enumerate(ARGS))
    src.write_text(f'#include "dalm_hip.h"\ntypedef void (*fn_t)(void);\nfn_t p[{len(ARGS)}];\nvoid fill(void) {{\n{body}\n}}\n')
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", str(ROOT / "include"), "-c", str(src), "-o",
                        str(tmp_path / "granite_abi.o")], capture_output=True, text=True)
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


def _fwd(lib, p, R=4, D=64, dtype=BF16, null=None, **over):
    a = dict(x=p[0], delta=p[1], w=p[2], h_out=p[3], y=p[4], rstd=p[5])
    a.update(over)
    args = [a["x"], a["delta"], C.c_float(0.22), a["w"], dtype, R, D, C.c_float(1e-6), a["h_out"], a["y"], a["rstd"], None, None]
    if null is not None:
        args[null] = None
    return lib.dalm_rms_norm_scaled_fwd(*args)


def _bwd(lib, p, R=4, D=64, dtype=BF16, null=None, **over):
    a = dict(dy=p[0], h=p[1], w=p[2], rstd=p[5], dres=p[6], dx=p[3], ddelta=p[4])
    a.update(over)
    args = [a["dy"], a["h"], a["w"], a["rstd"], a["dres"], C.c_float(0.22), dtype, R, D, a["dx"], a["ddelta"], None, None]
    if null is not None:
        args[null] = None
    return lib.dalm_rms_norm_scaled_bwd(*args)


def _add(lib, p, R=4, D=64, dtype=BF16, null=None, **over):
    a = dict(res=p[0], x=p[1], out=p[2])
    a.update(over)
    args = [a["res"], a["x"], C.c_float(0.22), a["out"], dtype, R, D, None, None]
    if null is not None:
        args[null] = None
    return lib.dalm_scale_add(*args)


def test_null_pointers_are_rejected(lib):
    buf = _Buffers()
    for null in (0, 1, 3, 8, 9, 10):               # x, delta (required here, unlike dalm_rms_norm_fwd_live), w, h_out, y, rstd
        _rejected(lib, buf, _fwd(lib, buf.p, null=null), E_NULL, b"null pointer")
    for null in (0, 1, 2, 3, 9, 10):               # dy, h, w, rstd, dx, ddelta; dres (4) may be NULL
        _rejected(lib, buf, _bwd(lib, buf.p, null=null), E_NULL, b"null pointer")
    for null in (1, 3):                            # x, out; res (0) may be NULL
        _rejected(lib, buf, _add(lib, buf.p, null=null), E_NULL, b"null pointer")


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_norm_widths_alignment_and_dtype(lib, dtype):
    buf = _Buffers()
    p = buf.p
    vec = 4 if dtype == F32 else 8
    cap = 64 * vec * 16                                                            # 8192 (bf16) / 4096 (f32)
    for call in (_fwd, _bwd):
        _rejected(lib, buf, call(lib, p, D=vec + 1, dtype=dtype), E_SHAPE, b"16 bytes")   # not a multiple of 16 bytes
        _rejected(lib, buf, call(lib, p, D=vec // 2, dtype=dtype), E_SHAPE)
        _rejected(lib, buf, call(lib, p, D=cap + vec, dtype=dtype), E_SHAPE)              # above the cap
        _rejected(lib, buf, call(lib, p, D=0, dtype=dtype), E_SHAPE)
        _rejected(lib, buf, call(lib, p, R=0, dtype=dtype), E_SHAPE)                      # dalm_rms_norm_*'s rule: rows > 0
        _rejected(lib, buf, call(lib, p, R=-1, dtype=dtype), E_SHAPE)
        _rejected(lib, buf, call(lib, p, w=p[2] + 8, dtype=dtype), E_ALIGN, b"aligned")
        _rejected(lib, buf, call(lib, p, dtype=2), E_DTYPE)
    _rejected(lib, buf, _fwd(lib, p, x=p[0] + 4, dtype=dtype), E_ALIGN)
    _rejected(lib, buf, _fwd(lib, p, delta=p[1] + 2, dtype=dtype), E_ALIGN)
    _rejected(lib, buf, _fwd(lib, p, h_out=p[3] + 8, dtype=dtype), E_ALIGN)
    _rejected(lib, buf, _fwd(lib, p, y=p[4] + 2, dtype=dtype), E_ALIGN)
    _rejected(lib, buf, _bwd(lib, p, dy=p[0] + 8, dtype=dtype), E_ALIGN)
    _rejected(lib, buf, _bwd(lib, p, dres=p[6] + 4, dtype=dtype), E_ALIGN)
    _rejected(lib, buf, _bwd(lib, p, dx=p[3] + 2, dtype=dtype), E_ALIGN)
    _rejected(lib, buf, _bwd(lib, p, ddelta=p[4] + 8, dtype=dtype), E_ALIGN)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_scale_add_shapes_alignment_and_no_rows(lib, dtype):
    buf = _Buffers()
    p = buf.p
    vec = 4 if dtype == F32 else 8
    _rejected(lib, buf, _add(lib, p, D=vec + 1, dtype=dtype), E_SHAPE, b"16 bytes")
    _rejected(lib, buf, _add(lib, p, D=vec // 2, dtype=dtype), E_SHAPE)
    _rejected(lib, buf, _add(lib, p, R=-1, dtype=dtype), E_SHAPE)
    _rejected(lib, buf, _add(lib, p, D=-vec, dtype=dtype), E_SHAPE)
    _rejected(lib, buf, _add(lib, p, R=1 << 20, D=vec << 11, dtype=dtype), E_SHAPE, b"2^31")     # R D / (16 bytes) reaches 2^31
    _rejected(lib, buf, _add(lib, p, dtype=2), E_DTYPE)
    _rejected(lib, buf, _add(lib, p, res=p[0] + 8, dtype=dtype), E_ALIGN, b"aligned")
    _rejected(lib, buf, _add(lib, p, x=p[1] + 2, dtype=dtype), E_ALIGN)
    _rejected(lib, buf, _add(lib, p, out=p[2] + 4, dtype=dtype), E_ALIGN)
    # no upper limit on the width: the shape check passes at 12800 and at 2^20 columns - no rows, so nothing is launched or written
    for D in (12800, 1 << 20):
        assert _add(lib, p, R=0, D=D, dtype=dtype) == 0 and buf.untouched()
    assert _add(lib, p, R=4, D=0, dtype=dtype) == 0 and buf.untouched()
    _rejected(lib, buf, _add(lib, p, R=0, D=3, dtype=dtype), E_SHAPE)                            # the width rule holds with no rows
