"""Grouped-query attention entry points (`dalm_attn_gqa_fwd` / `dalm_attn_gqa_bwd`, dalm_amd/csrc/attn.hip) without a GPU: they
exist in the header, the library and the ctypes table; argument errors come back before anything is enqueued; and
`attention.grouped_supported` turns down what the kernels do not take."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "dalm_hip.h"
E_NULL, E_SHAPE = -1, -2


@pytest.fixture(scope="module")
def lib():
    from dalm_amd import _build, hip

    _build.build(verbose=False)
    return hip.load()


def test_entry_points_in_header_library_and_table(lib):
    from dalm_amd import hip

    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in ("dalm_attn_gqa_fwd", "dalm_attn_gqa_bwd"):
        m = re.search(r"\bint %s\s*\(([^)]*)\)" % name, text)
        assert m, f"{name} is not declared in include/dalm_hip.h"
        assert "int64_t Hkv" in m.group(1) and "cu_seqlens" in m.group(1)
        assert hasattr(lib, name)
        assert name in hip.SIGNATURES and len(hip.SIGNATURES[name][1]) == m.group(1).count(",") + 1
    # the comment in front of them states the head mapping and the equal-heads case
    doc = HEADER.read_text()
    doc = doc[:doc.index("int dalm_attn_gqa_fwd")]
    doc = doc[doc.rindex("/*"):]
    assert "h / (H / Hkv)" in doc and "Hkv == H" in doc and "dalm_attn_fwd" in doc


def _buffers():
    """Host memory, 16-byte aligned: the checks under test run before any pointer is read or any kernel is enqueued."""
    raw = (C.c_char * 4096)()
    base = (C.addressof(raw) + 15) & ~15
    return raw, [base + 256 * i for i in range(14)]


def _fwd(lib, ptrs, B, H, Hkv, T, hd, null=None):
    q, k, v, rows, live, o, lse = ptrs[:7]
    args = [q, k, v, rows, live, None, B, H, Hkv, T, hd, C.c_float(0.1), (C.c_int64 * 12)(*([hd * H * T, hd * T, hd] * 4)), o, lse, None]
    if null is not None:
        args[null] = None
    return lib.dalm_attn_gqa_fwd(*args)


def _bwd(lib, ptrs, B, H, Hkv, T, hd, null=None, splits=1, ws=None, ws_bytes=0):
    q, k, v, o, d_o, lse, rows, cols, live, dq, dk, dv, delta = ptrs[:13]
    args = [q, k, v, o, d_o, lse, rows, cols, live, None, B, H, Hkv, T, hd, C.c_float(0.1),
            (C.c_int64 * 24)(*([hd * H * T, hd * T, hd] * 8)), None, None, 0, 0, splits, ws, ws_bytes, dq, dk, dv, delta, None]
    if null is not None:
        args[null] = None
    return lib.dalm_attn_gqa_bwd(*args)


def test_null_pointers_are_rejected(lib):
    raw, ptrs = _buffers()
    for null in (0, 1, 2, 3, 4, 12, 13, 14):
        assert _fwd(lib, ptrs, 1, 4, 2, 64, 64, null=null) == E_NULL, null
        assert b"null pointer" in lib.dalm_last_error_string()
    for null in (0, 1, 2, 3, 4, 5, 6, 7, 8, 16, 24, 25, 26, 27):
        assert _bwd(lib, ptrs, 1, 4, 2, 64, 64, null=null) == E_NULL, null
        assert b"null pointer" in lib.dalm_last_error_string()
    del raw


@pytest.mark.parametrize("H,Hkv", [(6, 4), (6, 0), (4, -2), (2, 4)])
def test_head_counts_that_do_not_group_are_shape_errors(lib, H, Hkv):
    raw, ptrs = _buffers()
    for call in (_fwd, _bwd):
        assert call(lib, ptrs, 1, H, Hkv, 64, 64) == E_SHAPE
        msg = lib.dalm_last_error_string().decode()
        assert "Hkv = %d" % Hkv in msg and "H = %d" % H in msg, msg     # the message names both head counts
    del raw


def test_other_head_widths_are_shape_errors(lib):
    raw, ptrs = _buffers()
    for call in (_fwd, _bwd):
        assert call(lib, ptrs, 1, 6, 2, 64, 96) == E_SHAPE
        assert b"head width" in lib.dalm_last_error_string()
        assert call(lib, ptrs, 1, 6, 2, 4096, 64) == E_SHAPE               # T beyond the mask-word layout
    del raw


def test_split_form_selection_and_workspace(lib):
    """One workgroup per KV head from 512 workgroups on; a smaller grid is split by the smallest divisor of the group that gives
    1024.  The split form wants S x (dK, dV) x rows x Hkv x hd f32 of workspace, checked before anything is enqueued."""
    assert lib.dalm_attn_gqa_bwd_splits(18, 32, 8, 256) == 1            # 144 pairs x 4 key blocks = 576 workgroups
    assert lib.dalm_attn_gqa_bwd_splits(18, 32, 4, 256) == 4            # 72 x 4 = 288 -> x 4 = 1152
    assert lib.dalm_attn_gqa_bwd_splits(2, 8, 2, 320) == 4              # small grids: one head per workgroup
    assert lib.dalm_attn_gqa_bwd_splits(18, 32, 32, 256) == 1
    assert lib.dalm_attn_gqa_bwd_workspace_bytes(128, 2, 64, 1) == 0
    assert lib.dalm_attn_gqa_bwd_workspace_bytes(128, 2, 64, 2) == 2 * 2 * 128 * 2 * 64 * 4
    raw, ptrs = _buffers()
    need = 2 * 2 * 64 * 2 * 64 * 4                                     # B 1, T 64, Hkv 2, hd 64, two parts
    assert _bwd(lib, ptrs, 1, 4, 2, 64, 64, splits=3, ws=ptrs[13], ws_bytes=need) == E_SHAPE       # 3 does not divide G = 2
    assert _bwd(lib, ptrs, 1, 4, 2, 64, 64, splits=-1) == E_SHAPE
    assert _bwd(lib, ptrs, 1, 4, 2, 64, 64, splits=2, ws=None, ws_bytes=need) == E_NULL
    assert _bwd(lib, ptrs, 1, 4, 2, 64, 64, splits=2, ws=ptrs[13], ws_bytes=need - 1) == -5        # DALM_E_WORKSPACE
    assert _bwd(lib, ptrs, 1, 4, 2, 64, 64, splits=0, ws=None, ws_bytes=0) == E_NULL               # a small grid: the library splits
    del raw


def test_grouped_supported_turns_down_what_the_kernels_do_not_take():
    from dalm_amd.models import attention

    def qkv(H, Hkv, dtype=torch.bfloat16, T=64, hd=64):
        q = torch.zeros(2, H, T, hd, dtype=dtype).requires_grad_(True)
        return q, torch.zeros(2, Hkv, T, hd, dtype=dtype), torch.zeros(2, Hkv, T, hd, dtype=dtype)

    assert not attention.grouped_supported(*qkv(4, 2), None, 0.0, True, {})                       # CPU tensors
    assert not attention.grouped_supported(*qkv(4, 2, torch.float32), None, 0.0, True, {})
    assert not attention.grouped_supported(*qkv(6, 4), None, 0.0, True, {})                       # H % Hkv != 0
    assert not attention.grouped_supported(*qkv(4, 1), None, 0.0, True, {})                       # multi-query: the stride-0 route
    assert not attention.grouped_supported(*qkv(4, 4), None, 0.0, True, {})                       # equal heads: `supported`
    assert not attention.grouped_supported(*qkv(4, 2), None, 0.1, True, {})                       # dropout
    assert not attention.grouped_supported(*qkv(4, 2), packed=True)

    # the head-count rules by themselves
    assert attention.group_ok(4, 2) and attention.group_ok(32, 8) and attention.group_ok(32, 2) and attention.group_ok(28, 4)
    assert not attention.group_ok(6, 4) and not attention.group_ok(4, 1) and not attention.group_ok(4, 4)
    assert not attention.group_ok(2, 4) and not attention.group_ok(34, 2)                          # 17 heads a group: over the limit
