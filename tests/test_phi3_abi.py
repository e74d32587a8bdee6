"""Phi-3's entry point (`dalm_rope_partial_qk`, dalm_amd/csrc/tower.hip) without a GPU: it exists in the header, the library and the
ctypes table with matching arity and argument order; the header still compiles as C99; argument errors - NULL tensors and stride
arrays, head widths 48 / 16 / 256 / 0, rotary widths 0 / -8 / hd + 16 / 24 with bf16 / 100 / 7, a tensor of 2^31 sixteen-byte chunks,
a misaligned pointer, a stride that is no multiple of 16 bytes, dtype 2 - come back as DALM_E_* with a message before anything is
enqueued or written; rot = 24 with f32 and rot == hd pass the checks (asked with no rows: nothing is launched)."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "dalm_hip.h"
NAME = "dalm_rope_partial_qk"
ARGS = ["q", "k", "q_out", "k_out", "cos", "sin", "dtype", "B", "T", "Hq", "Hk", "hd", "rot", "q_strides", "k_strides", "qo_strides",
        "ko_strides", "cs_strides", "backward", "row_live", "stream"]
E_NULL, E_SHAPE, E_DTYPE, E_ALIGN = -1, -2, -3, -4
F32, BF16 = 0, 1
FILL = 0x5A


@pytest.fixture(scope="module")
def lib():
    from dalm_amd import _build, hip

    _build.build(verbose=False)
    return hip.load()


def test_entry_point_in_header_library_and_table(lib):
    from dalm_amd import hip

    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    m = re.search(r"\bint %s\s*\(([^)]*)\)" % NAME, text)
    assert m, f"{NAME} is not declared in include/dalm_hip.h"
    decl = [a.strip() for a in m.group(1).split(",")]
    assert [re.split(r"[\s*]+", a)[-1] for a in decl] == ARGS, decl
    kinds = dict(zip(ARGS, decl))
    assert kinds["dtype"] == "int dtype" and kinds["row_live"] == "const uint8_t* row_live" and kinds["rot"] == "int64_t rot"
    assert kinds["stream"] == "dalm_stream_t stream"
    assert hasattr(lib, NAME), f"{NAME} is not exported by the library"
    res, table = hip.SIGNATURES[NAME]
    assert res is C.c_int and len(table) == len(ARGS)
    for a, d, t in zip(ARGS, decl, table):                          # 64-bit sizes, ints, pointers - in the header's order
        assert t is (C.c_int64 if d.startswith("int64_t ") else C.c_int if d.startswith("int ") else C.c_void_p), (a, d, t)
    # the comment in front of it states the formulas, the identity, the liveness and in-place contracts and the limits
    doc = HEADER.read_text()
    doc = doc[:doc.index("int " + NAME)]
    doc = doc[doc.rindex("/*"):]
    for word in ("modeling_phi3.py", "Row liveness", "rot == hd", "dalm_rope_qk_live's", "writes nothing", "i + rot/2", "In place",
                 "left untouched", "32, 64 or 128", "2^31", "DALM_E_NULL", "DALM_E_ALIGN", "bit for bit", "backward:"):
        assert word in doc, word


def test_header_is_still_plain_c(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    src = tmp_path / "phi3_abi.c"
    src.write_text(f'#include "dalm_hip.h"\ntypedef void (*fn_t)(void);\nfn_t p[1];\nvoid fill(void) {{\n  p[0] = (fn_t)&{NAME};\n}}\n')
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", str(ROOT / "include"), "-c", str(src), "-o",
                        str(tmp_path / "phi3_abi.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


class _Buffers:
    """Host memory, 16-byte aligned slots of 256 bytes filled with a pattern: the checks under test run before any pointer is read
    or any kernel is enqueued, so after a rejected call - and after an accepted call over no rows - every byte still holds it."""

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


def _rope(lib, p, dtype=BF16, B=1, T=2, Hq=2, Hk=1, hd=32, rot=16, null=None, strides=None, **over):
    a = dict(q=p[0], k=p[1], q_out=p[2], k_out=p[3], cos=p[4], sin=p[5])
    a.update(over)
    row = (Hq + 2 * Hk) * hd                                          # q | k | v of one token: the fused projection's row
    s = dict(q=(T * row, hd, row), k=(T * row, hd, row), qo=(T * Hq * hd, hd, Hq * hd), ko=(T * Hk * hd, hd, Hk * hd), cs=(0, 128))
    s.update(strides or {})
    arr = {n: (C.c_int64 * len(v))(*v) for n, v in s.items()}
    args = [a["q"], a["k"], a["q_out"], a["k_out"], a["cos"], a["sin"], dtype, B, T, Hq, Hk, hd, rot, arr["q"], arr["k"], arr["qo"],
            arr["ko"], arr["cs"], 0, None, None]
    if null is not None:
        args[null] = None
    return lib.dalm_rope_partial_qk(*args)


def test_null_pointers_are_rejected(lib):
    buf = _Buffers()
    for null in (0, 1, 2, 3, 4, 5, 13, 14, 15, 16, 17):     # the six tensors and the five stride arrays
        _rejected(lib, buf, _rope(lib, buf.p, null=null), E_NULL, b"null pointer")


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_head_and_rotary_widths_sizes_strides_alignment_and_dtypes(lib, dtype):
    buf = _Buffers()
    p = buf.p
    for hd in (48, 16, 256, 0):
        _rejected(lib, buf, _rope(lib, p, dtype=dtype, hd=hd, rot=16), E_SHAPE, b"32, 64 or 128")
    for hd in (32, 64, 128):
        for rot in (0, -8, hd + 16, 100, 7):
            _rejected(lib, buf, _rope(lib, p, dtype=dtype, hd=hd, rot=rot), E_SHAPE, b"rotary width")
    _rejected(lib, buf, _rope(lib, p, dtype=BF16, hd=32, rot=24), E_SHAPE, b"multiple of 16 for bf16")     # 12 bf16 = 24 bytes a half
    _rejected(lib, buf, _rope(lib, p, dtype=dtype, Hq=0), E_SHAPE)
    _rejected(lib, buf, _rope(lib, p, dtype=dtype, Hk=-1), E_SHAPE)
    _rejected(lib, buf, _rope(lib, p, dtype=dtype, B=-1), E_SHAPE)
    _rejected(lib, buf, _rope(lib, p, dtype=dtype, T=-1), E_SHAPE)
    # B T (Hq + Hk) hd / (16 bytes) reaches 2^31 exactly: 4 heads of 16 (bf16, hd 128) or 8 (f32, hd 32) chunks, 2^25 or 2^26 tokens
    vec = 4 if dtype == F32 else 8
    hd, T = (128, 1 << 5) if dtype == BF16 else (32, 1 << 6)
    assert (1 << 20) * T * 4 * (hd // vec) == 1 << 31
    _rejected(lib, buf, _rope(lib, p, dtype=dtype, B=1 << 20, T=T, Hq=3, Hk=1, hd=hd, rot=32), E_SHAPE, b"2^31")
    for name in ("q", "k", "q_out", "k_out", "cos", "sin"):                      # a misaligned pointer
        _rejected(lib, buf, _rope(lib, p, dtype=dtype, **{name: p[7] + 8}), E_ALIGN, b"aligned")
    for name, n in (("q", 3), ("k", 3), ("qo", 3), ("ko", 3), ("cs", 2)):        # a stride that is no multiple of 16 bytes
        for i in range(n):
            s = [64 * vec] * n
            s[i] = 64 * vec + vec // 2
            _rejected(lib, buf, _rope(lib, p, dtype=dtype, strides={name: tuple(s)}), E_ALIGN, b"stride")
    _rejected(lib, buf, _rope(lib, p, dtype=BF16, strides={"q": (64, 32, 100)}), E_ALIGN)       # 100: a multiple of 4, not of 8
    _rejected(lib, buf, _rope(lib, p, dtype=2), E_DTYPE)


def test_one_chunk_below_the_size_limit_passes_the_size_check(lib):
    """2^31 - 64 chunks: the size rule is `< 2^31`, not something smaller.  Asked with a misaligned pointer, so the call ends at the
    NEXT check (alignment) and nothing is launched."""
    buf = _Buffers()
    rc = _rope(lib, buf.p, dtype=BF16, B=(1 << 25) - 1, T=1, Hq=3, Hk=1, hd=128, rot=96, q=buf.p[7] + 8)
    _rejected(lib, buf, rc, E_ALIGN, b"aligned")


def test_admitted_widths_pass_the_checks(lib):
    """rot = 24 with f32, rot == hd, and Phi-4-mini's 96 of 128: accepted.  B = 0 - no rows - so nothing is launched or written."""
    buf = _Buffers()
    for kw in (dict(dtype=F32, hd=32, rot=24), dict(dtype=F32, hd=32, rot=32), dict(dtype=BF16, hd=32, rot=32),
               dict(dtype=BF16, hd=64, rot=64), dict(dtype=BF16, hd=128, rot=128), dict(dtype=BF16, hd=128, rot=96),
               dict(dtype=BF16, hd=128, rot=64), dict(dtype=BF16, hd=64, rot=48), dict(dtype=BF16, hd=64, rot=32),
               dict(dtype=BF16, hd=32, rot=16), dict(dtype=F32, hd=128, rot=96)):
        assert _rope(lib, buf.p, B=0, **kw) == 0, (kw, lib.dalm_last_error_string())
        assert _rope(lib, buf.p, T=0, **kw) == 0, (kw, lib.dalm_last_error_string())
        assert buf.untouched()
    # the width rule holds with no rows
    _rejected(lib, buf, _rope(lib, buf.p, B=0, dtype=BF16, hd=32, rot=24), E_SHAPE, b"rotary width")
    # in place the outputs carry the inputs' strides
    p = buf.p
    assert _rope(lib, p, B=0, q_out=p[0], k_out=p[1], strides={"qo": (2 * 128, 32, 128), "ko": (2 * 128, 32, 128)}) == 0
    _rejected(lib, buf, _rope(lib, p, B=0, q_out=p[0], k_out=p[1]), E_SHAPE, b"in place")
