"""Cohere's entry points (`dalm_rope_il_qk`, `dalm_cohere_norm_{fwd,bwd}`, `dalm_add3_live`, dalm_amd/csrc/tower.hip) without a GPU:
they exist in the header, the library and the ctypes table with matching arity and argument order; the header still compiles as C99;
argument errors - head width 48, a width that is no multiple of 16 bytes or over the cap, a misaligned pointer, a stride that is no
multiple of 8 - come back as DALM_E_SHAPE / DALM_E_ALIGN with a message before anything is enqueued or written."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "dalm_hip.h"
ARGS = {
    "dalm_rope_il_qk": ["q", "k", "q_out", "k_out", "cos", "sin", "dtype", "tab_dtype", "B", "T", "Hq", "Hk", "hd", "q_strides",
                        "k_strides", "qo_strides", "ko_strides", "cs_strides", "backward", "row_live", "stream"],
    "dalm_cohere_norm_fwd": ["x", "w", "dtype", "w_dtype", "R", "D", "eps", "y", "mean", "rstd", "row_live", "stream"],
    "dalm_cohere_norm_bwd": ["dy", "x", "w", "mean", "rstd", "dres", "dtype", "w_dtype", "R", "D", "dx", "row_live", "stream"],
    "dalm_add3_live": ["res", "a", "b", "out", "dtype", "R", "D", "row_live", "stream"],
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
        assert kinds["dtype"] == "int dtype" and kinds["row_live"] == "const uint8_t* row_live"
        assert kinds["stream"] == "dalm_stream_t stream"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        res, table = hip.SIGNATURES[name]
        assert res is C.c_int and len(table) == len(want)
        for a, d, t in zip(want, decl, table):                       # floats where the header has floats, 64-bit sizes, pointers
            assert t is (C.c_float if d.startswith("float ") else C.c_int64 if d.startswith("int64_t ") else C.c_int
                         if d.startswith("int ") else C.c_void_p), (name, a, d, t)
    # the comment in front of them states the formulas, the liveness contract and the limits
    doc = HEADER.read_text()
    doc = doc[:doc.index("int dalm_rope_il_qk")]
    doc = doc[doc.rindex("/*"):]
    for word in ("modeling_cohere.py", "Row liveness", "cos[2i+1]", "no fused multiply-add", "tab_dtype", "32, 64 or 128", "8192",
                 "4096", "mean_d(g)", "round(round(res + a) + b)", "writes nothing"):
        assert word in doc, word


def test_header_is_still_plain_c(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    src = tmp_path / "cohere_abi.c"
    body = "\n".join(f"  p[{i}] = (fn_t)&{n};" for i, n in enumerate(ARGS))
    src.write_text(f'#include "dalm_hip.h"\ntypedef void (*fn_t)(void);\nfn_t p[{len(ARGS)}];\nvoid fill(void) {{\n{body}\n}}\n')
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", str(ROOT / "include"), "-c", str(src), "-o",
                        str(tmp_path / "cohere_abi.o")], capture_output=True, text=True)
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


def _rope(lib, p, dtype=BF16, tab_dtype=None, B=1, T=2, Hq=2, Hk=1, hd=32, null=None, strides=None, **over):
    a = dict(q=p[0], k=p[1], q_out=p[2], k_out=p[3], cos=p[4], sin=p[5])
    a.update(over)
    s = dict(q=(T * Hq * hd, hd, Hq * hd), k=(T * Hk * hd, hd, Hk * hd), qo=(T * Hq * hd, hd, Hq * hd), ko=(T * Hk * hd, hd, Hk * hd),
             cs=(0, hd))
    s.update(strides or {})
    arr = {n: (C.c_int64 * len(v))(*v) for n, v in s.items()}
    args = [a["q"], a["k"], a["q_out"], a["k_out"], a["cos"], a["sin"], dtype, dtype if tab_dtype is None else tab_dtype, B, T, Hq, Hk,
            hd, arr["q"], arr["k"], arr["qo"], arr["ko"], arr["cs"], 0, None, None]
    if null is not None:
        args[null] = None
    return lib.dalm_rope_il_qk(*args)


def _fwd(lib, p, R=4, D=64, dtype=BF16, w_dtype=BF16, null=None, **over):
    a = dict(x=p[0], w=p[1], y=p[2], mean=p[3], rstd=p[4])
    a.update(over)
    args = [a["x"], a["w"], dtype, w_dtype, R, D, C.c_float(1e-5), a["y"], a["mean"], a["rstd"], None, None]
    if null is not None:
        args[null] = None
    return lib.dalm_cohere_norm_fwd(*args)


def _bwd(lib, p, R=4, D=64, dtype=BF16, w_dtype=BF16, null=None, **over):
    a = dict(dy=p[0], x=p[1], w=p[2], mean=p[3], rstd=p[4], dres=p[5], dx=p[6])
    a.update(over)
    args = [a["dy"], a["x"], a["w"], a["mean"], a["rstd"], a["dres"], dtype, w_dtype, R, D, a["dx"], None, None]
    if null is not None:
        args[null] = None
    return lib.dalm_cohere_norm_bwd(*args)


def _add(lib, p, R=4, D=64, dtype=BF16, null=None, **over):
    a = dict(res=p[0], a=p[1], b=p[2], out=p[3])
    a.update(over)
    args = [a["res"], a["a"], a["b"], a["out"], dtype, R, D, None, None]
    if null is not None:
        args[null] = None
    return lib.dalm_add3_live(*args)


def test_null_pointers_are_rejected(lib):
    buf = _Buffers()
    for null in (0, 1, 2, 3, 4, 5, 13, 14, 15, 16, 17):     # the six tensors and the five stride arrays
        _rejected(lib, buf, _rope(lib, buf.p, null=null), E_NULL, b"null pointer")
    for null in (0, 1, 7, 8, 9):                             # x, w, y, mean, rstd
        _rejected(lib, buf, _fwd(lib, buf.p, null=null), E_NULL, b"null pointer")
    for null in (0, 1, 2, 3, 4, 10):                         # dy, x, w, mean, rstd, dx; dres (5) may be NULL
        _rejected(lib, buf, _bwd(lib, buf.p, null=null), E_NULL, b"null pointer")
    for null in (0, 1, 2, 3):
        _rejected(lib, buf, _add(lib, buf.p, null=null), E_NULL, b"null pointer")


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_rope_head_widths_strides_alignment_and_dtypes(lib, dtype):
    buf = _Buffers()
    p = buf.p
    for hd in (48, 16, 256, 0, 33):
        _rejected(lib, buf, _rope(lib, p, dtype=dtype, hd=hd), E_SHAPE, b"32, 64 or 128")
    _rejected(lib, buf, _rope(lib, p, dtype=dtype, B=0), E_SHAPE)
    _rejected(lib, buf, _rope(lib, p, dtype=dtype, T=0), E_SHAPE)
    _rejected(lib, buf, _rope(lib, p, dtype=dtype, Hq=0), E_SHAPE)
    _rejected(lib, buf, _rope(lib, p, dtype=dtype, Hk=-1), E_SHAPE)
    _rejected(lib, buf, _rope(lib, p, dtype=dtype, B=1 << 20, T=1 << 12), E_SHAPE, b"too large")
    for name in ("q", "k", "q_out", "k_out", "cos", "sin"):                      # a misaligned pointer
        _rejected(lib, buf, _rope(lib, p, dtype=dtype, **{name: p[7] + 8}), E_ALIGN, b"aligned")
    vec = 4 if dtype == F32 else 8
    for name, n in (("q", 3), ("k", 3), ("qo", 3), ("ko", 3), ("cs", 2)):        # a stride that is no multiple of 16 bytes
        for i in range(n):
            s = [64 * vec] * n
            s[i] = 64 * vec + vec // 2
            _rejected(lib, buf, _rope(lib, p, dtype=dtype, strides={name: tuple(s)}), E_ALIGN, b"stride")
    _rejected(lib, buf, _rope(lib, p, dtype=BF16, strides={"q": (64, 32, 100)}), E_ALIGN)       # 100: a multiple of 4, not of 8
    _rejected(lib, buf, _rope(lib, p, dtype=2), E_DTYPE)
    _rejected(lib, buf, _rope(lib, p, dtype=F32, tab_dtype=BF16), E_DTYPE, b"tables")           # bf16 tables beside f32 activations


@pytest.mark.parametrize("w_dtype", [BF16, F32])
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_norm_widths_alignment_and_dtype(lib, dtype, w_dtype):
    buf = _Buffers()
    p = buf.p
    vec = 4 if dtype == F32 else 8
    cap = 64 * vec * 16                                                            # 8192 (bf16) / 4096 (f32)
    for call in (_fwd, _bwd):
        kw = dict(dtype=dtype, w_dtype=w_dtype)
        _rejected(lib, buf, call(lib, p, D=vec + 1, **kw), E_SHAPE, b"16 bytes")   # not a multiple of 16 bytes
        _rejected(lib, buf, call(lib, p, D=vec // 2, **kw), E_SHAPE)
        _rejected(lib, buf, call(lib, p, D=cap + vec, **kw), E_SHAPE)              # above the cap
        _rejected(lib, buf, call(lib, p, D=12288, **kw), E_SHAPE)                  # Command-R+'s width
        _rejected(lib, buf, call(lib, p, D=0, **kw), E_SHAPE)
        _rejected(lib, buf, call(lib, p, R=0, **kw), E_SHAPE)                      # dalm_rms_norm_*'s rule: rows > 0
        _rejected(lib, buf, call(lib, p, R=-1, **kw), E_SHAPE)
        _rejected(lib, buf, call(lib, p, w=p[8] + 8, **kw), E_ALIGN, b"aligned")
        _rejected(lib, buf, call(lib, p, x=p[8] + 4, **kw), E_ALIGN)
        _rejected(lib, buf, call(lib, p, dtype=2, w_dtype=w_dtype), E_DTYPE)
        _rejected(lib, buf, call(lib, p, dtype=dtype, w_dtype=2), E_DTYPE, b"w_dtype")
    _rejected(lib, buf, _fwd(lib, p, y=p[2] + 2, dtype=dtype, w_dtype=w_dtype), E_ALIGN)
    _rejected(lib, buf, _bwd(lib, p, dy=p[0] + 8, dtype=dtype, w_dtype=w_dtype), E_ALIGN)
    _rejected(lib, buf, _bwd(lib, p, dres=p[5] + 4, dtype=dtype, w_dtype=w_dtype), E_ALIGN)
    _rejected(lib, buf, _bwd(lib, p, dx=p[6] + 2, dtype=dtype, w_dtype=w_dtype), E_ALIGN)


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_add3_shapes_alignment_and_no_rows(lib, dtype):
    buf = _Buffers()
    p = buf.p
    vec = 4 if dtype == F32 else 8
    _rejected(lib, buf, _add(lib, p, D=vec + 1, dtype=dtype), E_SHAPE, b"16 bytes")
    _rejected(lib, buf, _add(lib, p, D=vec // 2, dtype=dtype), E_SHAPE)
    _rejected(lib, buf, _add(lib, p, R=-1, dtype=dtype), E_SHAPE)
    _rejected(lib, buf, _add(lib, p, D=-vec, dtype=dtype), E_SHAPE)
    _rejected(lib, buf, _add(lib, p, R=1 << 20, D=vec << 11, dtype=dtype), E_SHAPE, b"2^31")     # R D / (16 bytes) reaches 2^31
    _rejected(lib, buf, _add(lib, p, dtype=2), E_DTYPE)
    for name in ("res", "a", "b", "out"):
        _rejected(lib, buf, _add(lib, p, dtype=dtype, **{name: p[8] + 8}), E_ALIGN, b"aligned")
    # no upper limit on the width: the shape check passes at 12800 and at 2^20 columns - no rows, so nothing is launched or written
    for D in (12800, 1 << 20):
        assert _add(lib, p, R=0, D=D, dtype=dtype) == 0 and buf.untouched()
    assert _add(lib, p, R=4, D=0, dtype=dtype) == 0 and buf.untouched()
    _rejected(lib, buf, _add(lib, p, R=0, D=3, dtype=dtype), E_SHAPE)                            # the width rule holds with no rows
