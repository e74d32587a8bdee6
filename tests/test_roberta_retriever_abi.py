"""`dalm_embed_norm_fwd` (dalm_amd/csrc/bert.hip: the RoBERTa-family embeddings front end) without a GPU: it exists in the header,
the library and the ctypes table with matching arity, the header still compiles as C99, and argument errors come back before
anything is enqueued."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "dalm_hip.h"
NAME = "dalm_embed_norm_fwd"
E_NULL, E_SHAPE, E_ALIGN = -1, -2, -4


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
    params = m.group(1)
    for word in ("const int64_t* ids", "token_type_ids", "position_ids", "padding_idx", "row_live", "uint32_t salt", "float* y32"):
        assert word in params, word
    assert params.rstrip().endswith("dalm_stream_t stream")
    assert hasattr(lib, NAME), f"{NAME} is not exported by the library"
    assert NAME in hip.SIGNATURES and len(hip.SIGNATURES[NAME][1]) == params.count(",") + 1
    # the comment in front of it states the position rule, the clamp and that nothing has a backward
    doc = HEADER.read_text()
    doc = doc[:doc.index("int " + NAME)]
    doc = doc[doc.rindex("/*"):]
    assert "create_position_ids_from_input_ids" in doc and "CLAMPED" in doc and "backward" in doc and "row_live" in doc


def test_header_is_still_plain_c(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    src = tmp_path / "embed_abi.c"
    src.write_text(f'#include "dalm_hip.h"\ntypedef void (*fn_t)(void);\nfn_t p[1];\nvoid fill(void) {{ p[0] = (fn_t)&{NAME}; }}\n')
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", str(ROOT / "include"), "-c", str(src), "-o",
                        str(tmp_path / "embed_abi.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _buffers():
    """Host memory, 16-byte aligned: the checks under test run before any pointer is read or any kernel is enqueued."""
    raw = (C.c_char * 8192)()
    base = (C.addressof(raw) + 15) & ~15
    return raw, [base + 256 * i for i in range(16)]


# argument order: ids, token_type_ids, position_ids, word, type, pos, vocab, type_vocab, max_pos, padding_idx, w, b, w_bf16, B, T, D,
#                 eps, dropout_p, seed, salt, y32, y16, row_live, stream
def _call(lib, p, null=None, **over):
    a = dict(ids=p[0], tt=None, pos_ids=None, word=p[1], type=p[2], pos=p[3], vocab=10, type_vocab=1, max_pos=12, pad=1, w=p[4], b=p[5],
             w_bf16=0, B=2, T=4, D=64, drop=0.0, seed=None, y32=p[6], y16=p[7])
    a.update(over)
    args = [a["ids"], a["tt"], a["pos_ids"], a["word"], a["type"], a["pos"], a["vocab"], a["type_vocab"], a["max_pos"], a["pad"], a["w"],
            a["b"], a["w_bf16"], a["B"], a["T"], a["D"], C.c_float(1e-5), C.c_float(a["drop"]), a["seed"], 7, a["y32"], a["y16"], None, None]
    if null is not None:
        args[null] = None
    return lib.dalm_embed_norm_fwd(*args)


def test_null_pointers_are_rejected(lib):
    raw, p = _buffers()
    for null in (0, 3, 4, 5, 10, 11, 20, 21):                 # ids, the three tables, w, b, y32, y16
        assert _call(lib, p, null=null) == E_NULL, null
        assert b"null pointer" in lib.dalm_last_error_string()
    del raw


def test_sizes_alignment_and_dropout_arguments(lib):
    raw, p = _buffers()
    assert _call(lib, p, B=0) == 0 and _call(lib, p, T=0) == 0                        # nothing to do is not an error
    assert _call(lib, p, B=-1) == E_SHAPE and _call(lib, p, T=-1) == E_SHAPE
    for D in (0, 12, 2056, 4096):
        assert _call(lib, p, D=D) == E_SHAPE, D
        assert b"multiple of 8" in lib.dalm_last_error_string()
    assert _call(lib, p, B=1 << 20, T=1 << 12) == E_SHAPE
    assert _call(lib, p, vocab=0) == E_SHAPE and _call(lib, p, type_vocab=0) == E_SHAPE and _call(lib, p, max_pos=0) == E_SHAPE
    assert _call(lib, p, word=p[1] + 4) == E_ALIGN and _call(lib, p, y16=p[7] + 2) == E_ALIGN and _call(lib, p, w=p[4] + 8) == E_ALIGN
    assert _call(lib, p, drop=0.1) == E_SHAPE                                             # dropout without a seed word
    assert b"seed" in lib.dalm_last_error_string()
    assert _call(lib, p, drop=1.0, seed=p[8]) == E_SHAPE and _call(lib, p, drop=-0.5, seed=p[8]) == E_SHAPE
    del raw
