"""The attention kernels (dalm_amd/csrc/attn.hip) along the axes the other attention tests are thin on: every tile edge of the
sequence length, the whole admitted range 2 <= T <= 2048, and values that drive the softmax to its limits - head widths 32, 64
and 128, padded, grouped and packed layouts.

The statistic is PER ROW (`helpers.assert_rows_close`): the worst row's error against a float64 evaluation may be no larger than
1.5 x the worst row's error of torch's own bf16 kernel on the same inputs + 1e-3 - the project's factor and offset
(tests/test_attention_gpu.py) applied to the row maximum, beside that file's whole-tensor rule.  A single wrong row of 2048 (the
last row of a partial block, the row T - 1 that `dma_block`'s clamp repeats) moves a whole-tensor norm by 1e-3 and passes there;
tests/test_attention_row_rule.py shows that on the CPU.

* section 1: T at both sides of every edge (32: mask word, 64: key block, 128: query block), four mask kinds, B H = 9 (a launch of
  16: one full group of 8 and a partly idle one); the log-sum-exp the forward writes against float64, torch's own lse as the
  yardstick; exact zeros at every dead query / key row the mask implies; inputs that are views into a NaN-filled buffer;
* section 2: T 1023 .. 2048 - at 2048 the last of the 64 mask words per row, the last 64-row block, bit 31 of the dk / dv kernels'
  `blocks` map and bits 62-63 of `need` are live; dropout at T 2048 / 1030 against oracle/attn_dropout.py's keep mask;
* section 3: grouped heads and packed sequences at the same extents;
* section 4: near one-hot probabilities, a common offset of +-80 on every score of a row, all-zero queries, rows whose only live
  key is themselves.

Measured on the MI355X (identical in two runs): every case inside 1.5 x + 1e-3, the closest at
0.93 of the bound.  Worst row against torch's worst row per head width: 128: 1.78 x (4.2e-3 / 2.4e-3, T 33 without a mask, dq
row (0, 0, 25)); 32: 1.42 x (5.3e-3 / 3.7e-3, T 63 encoder mask, dq row (2, 1, 50)); 64: 1.11 x (3.8e-3 / 3.4e-3, T 129 without a
mask, dq row (0, 2, 19)) - none on a tile edge.  Under a causal mask both dq maxima are the second or third row of a sequence (2-3 %,
the same for torch and the kernels); the long cases therefore apply the rule once more to the rows with many partners
(`_check_padded(dense=True)`).  lse: 1.3e-6 for both.

Every bound is torch's measured error against float64 in the same run, an existing constant of the project (1.5, 1e-3, 1.2e-2,
1e-4 as the offset of the lse rule) or exact equality.  Both maxima of every case of sections 1-3 are recorded with
`helpers.record_measured` (the measured-tolerances file of tests/test_tower_ops_gpu.py) under "attn_extents:...".
"""
import os
import sys
from pathlib import Path

import pytest
import torch

from helpers import (assert_rows_close, attn_ref64, encoder_mask, hf_mask, live_matrix, norm_rel_err, record_measured, run_grad)

pytestmark = pytest.mark.gpu

LSE_FACTOR, LSE_OFFSET = 1.5, 1e-4          # max |lse - float64| <= 1.5 x torch's own + 1e-4
# (where a test knows the value in closed form - ln(live keys), the scaled self-score - the offset alone is the bound: an f32 of
# magnitude below 16 resolves 1e-6, the score is an f32 sum of hd exact bf16 products)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


def _inputs(B, H, T, hd, layout, seed, dev, Hkv=None, gain=1.2):
    """q, k, v, dO in the projections' [B, T, H, hd] memory ("bthd") or contiguous ("bhtd"), as tests/test_attention_gpu.py."""
    g = torch.Generator().manual_seed(seed)

    def mk(heads):
        if layout == "bthd":
            return (torch.randn(B, T, heads, hd, generator=g) * gain).bfloat16().to(dev).transpose(1, 2)
        return (torch.randn(B, heads, T, hd, generator=g) * gain).bfloat16().to(dev)

    return mk(H), mk(Hkv or H), mk(Hkv or H), mk(H)


def _mask(kind, B, T, arg, dev):
    """(mask, causal) of a mask kind; `arg`: left-padding starts / right-padded lengths per batch row."""
    if kind == "causal":
        return None, True
    if kind == "full":
        return None, False
    if kind == "left":
        return hf_mask(B, T, arg, dev), False
    assert kind == "encoder"
    return encoder_mask(B, T, arg, dev), False


def _sdpa_ours(mask, scale, causal):
    from dalm_amd.models import attention

    return lambda a, b, c: attention._SdpaHipBackward.apply(a, b, c, mask, scale, causal)


def _sdpa_torch(mask, scale, causal):
    return lambda a, b, c: torch.nn.functional.scaled_dot_product_attention(a, b, c, attn_mask=mask, is_causal=causal, scale=scale)


def _lse_pair(q, k, v, mask, scale, causal):
    """The log-sum-exp `dalm_attn_fwd` writes, and torch's own (the library path under DALM_ATTN_FWD_KERNEL=0: torch's
    memory-efficient forward called as the aten op), both [B, H, T]."""
    from dalm_amd.models import attention

    B, H, T, _ = q.shape
    pk = attention._pack(mask, B, H, T, causal, q.dtype, q.device)
    with torch.no_grad():
        ours = attention._attn_forward(q, k, v, pk, scale, causal)[1]
        os.environ["DALM_ATTN_FWD_KERNEL"] = "0"
        try:
            theirs = attention._attn_forward(q, k, v, pk, scale, causal)[1]
        finally:
            os.environ.pop("DALM_ATTN_FWD_KERNEL", None)
    assert ours.shape == (B, H, T)
    return ours, theirs[..., :T]


def _check_zero_rows(res, live):
    """Exact zeros the mask implies: o, dq at query rows without a live key; dk, dv at key rows no query row attends."""
    dead_q, dead_k = ~live.any(-1), ~live.any(-2)                    # [B, T]
    for name, t, dead in (("o", res[0], dead_q), ("dq", res[1], dead_q), ("dk", res[2], dead_k), ("dv", res[3], dead_k)):
        if bool(dead.any()):
            assert float(t.transpose(1, 2)[dead].abs().max()) == 0.0, name
    return dead_q, dead_k


def _check_single_key_rows(o, v, live):
    """A query row with ONE live key: probability 1, o is that key's v row bit for bit.  Returns how many such (b, i) there are."""
    one = live.sum(-1) == 1                                          # [B, T]
    if not bool(one.any()):
        return 0
    H, hd = v.shape[1], v.shape[3]
    key = live.int().argmax(-1)                                      # [B, T]
    want = torch.gather(v.transpose(1, 2), 1, key[:, :, None, None].expand(-1, -1, H, hd))
    assert torch.equal(o.transpose(1, 2)[one], want[one])
    return int(one.sum())


def _check_lse(tag, q, k, v, mask, scale, causal, live, ref_lse, record=True):
    ours, theirs = _lse_pair(q, k, v, mask, scale, causal)
    B, H, T, _ = q.shape
    live_q = live.any(-1)[:, None, :].expand(B, H, T)
    assert torch.isfinite(ours).all()
    e_o = float((ours.double() - ref_lse)[live_q].abs().max())
    e_t = float((theirs.double() - ref_lse)[live_q].abs().max())
    if record:
        record_measured(f"attn_extents:{tag}:lse", {"max_abs": e_o, "max_abs_torch": e_t})
    print(f"{tag}: lse max |ours - float64| {e_o:.3e}, torch's {e_t:.3e}")
    assert e_o <= LSE_FACTOR * e_t + LSE_OFFSET, (tag, e_o, e_t)
    if not bool(live_q.all()):                                       # the kernel writes 0 where the row sum is 0
        assert float(ours[~live_q].abs().max()) == 0.0
    return ours


DENSE = 64        # "many partners": a query row with at least that many live keys, a key row that many query rows attend


def _check_padded(tag, q, k, v, go, mask, causal, scale, record=True, dense=False):
    """One padded-layout case: o, dq, dk, dv under the per-row rule (torch's bf16 kernels as the yardstick), the zero sets, rows
    with one live key, the log-sum-exp.  Returns (ours, reference, live matrix, lse).

    dense: the same rule once more with the error of every row of FEWER than 64 partners taken out (set to the reference in both
    results; scale and row indices stay the whole tensor's).  Under a causal mask the second and third row of a sequence - two or
    three keys, D = rowsum(dO o O) from a bf16 O - sit 2-3 % from float64 in dq for torch and for the kernels alike and set both
    maxima: without this, a row of the last block could be 6-9 % off in dq and pass."""
    from dalm_amd.models import attention

    B, H, T, hd = q.shape
    assert attention.supported(q.requires_grad_(True), k, v, mask, 0.0, causal, {})
    ours = run_grad(_sdpa_ours(mask, scale, causal), q, k, v, go)
    theirs = run_grad(_sdpa_torch(mask, scale, causal), q, k, v, go)
    live = live_matrix(mask, causal, B, T, q.device)
    ref = attn_ref64(q, k, v, live, scale, go)
    for name, a, b, r in zip(("o", "dq", "dk", "dv"), ours, theirs, ref[:4]):
        assert_rows_close(f"{tag}:{name}", a, b, r, record=f"attn_extents:{tag}:{name}" if record else None)
    if dense:
        many_k, many_q = live.sum(-1) >= DENSE, live.sum(-2) >= DENSE                  # [B, T]
        assert bool(many_k.any()) and bool(many_q.any())
        for name, a, b, r, sel in zip(("o", "dq", "dk", "dv"), ours, theirs, ref[:4], (many_k, many_k, many_q, many_q)):
            sel = sel[:, None, :, None]
            assert_rows_close(f"{tag}:{name}:rows with >= {DENSE} partners", torch.where(sel, a.double(), r), torch.where(sel, b.double(), r),
                              r, record=f"attn_extents:{tag}:{name}:dense" if record else None)
    assert ours[0].transpose(1, 2).is_contiguous()
    _check_zero_rows(ours, live)
    _check_single_key_rows(ours[0], v, live)
    lse = _check_lse(tag, q, k, v, mask, scale, causal, live, ref[4], record)
    return ours, ref, live, lse


# ---------------------------------------------------------------------------------------------------------------------------
# 1. every tile edge
# ---------------------------------------------------------------------------------------------------------------------------
EDGE_T = [2, 3, 31, 33, 63, 65, 127, 129, 191, 193]
KINDS = ["causal", "full", "left", "encoder"]


def _edge_arg(kind, T):
    if kind == "left":
        return [0, T // 3, T - 1]                 # the last sequence has one live row
    if kind == "encoder":
        return [T, 1, max(1, T // 2)]
    return None


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", EDGE_T)
@pytest.mark.parametrize("hd", [32, 64, 128])
def test_every_tile_edge(dev, hd, T, kind):
    B, H = 3, 3
    q, k, v, go = _inputs(B, H, T, hd, "bthd", 100 * T + hd, dev)
    mask, causal = _mask(kind, B, T, _edge_arg(kind, T), dev)
    if kind == "encoder":
        assert mask.stride(2) == 0                # what `dalm_attn_mask_bits` reads through mask_stride_row
    _check_padded(f"edge:hd{hd}:T{T}:{kind}", q, k, v, go, mask, causal, hd ** -0.5)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hd,T", [(32, 129), (64, 65), (128, 193)])
def test_tile_edges_in_contiguous_memory(dev, hd, T, kind):
    B, H = 3, 3
    q, k, v, go = _inputs(B, H, T, hd, "bhtd", 100 * T + hd + 1, dev)
    mask, causal = _mask(kind, B, T, _edge_arg(kind, T), dev)
    _check_padded(f"edge-bhtd:hd{hd}:T{T}:{kind}", q, k, v, go, mask, causal, hd ** -0.5)


@pytest.mark.parametrize("T", [65, 129])
@pytest.mark.parametrize("hd", [32, 64, 128])
def test_inputs_inside_a_poisoned_buffer(dev, hd, T):
    """q, k, v are views buf[:, 1:T + 1, :H].transpose(1, 2) of NaN-filled [B, T + 2, H + 1, hd] buffers (strides multiples of 8,
    base 16-byte aligned): nothing outside a head's T x hd rows may reach the result - finite, and the bits of the run on
    contiguous copies.  Only memory OUTSIDE the views is poisoned (the kernels want finite values at dead rows inside T)."""
    from dalm_amd.models import attention

    B, H = 3, 3
    vals = _inputs(B, H, T, hd, "bhtd", 7 * T + hd, dev)

    def view_of(x):
        buf = torch.full((B, T + 2, H + 1, hd), float("nan"), dtype=torch.bfloat16, device=dev)
        vw = buf[:, 1:T + 1, :H].transpose(1, 2)
        vw.copy_(x)
        assert torch.isnan(buf[:, 0]).all() and torch.isnan(buf[:, T + 1]).all() and torch.isnan(buf[:, :, H]).all()
        return vw

    go = vals[3]
    scale = hd ** -0.5

    def run(fn, q, k, v):            # no clone: the leaves ARE the views (a clone would drop the poisoned surroundings)
        q, k, v = [t.detach().requires_grad_(True) for t in (q, k, v)]
        o = fn(q, k, v)
        o.backward(go)
        return o.detach(), q.grad, k.grad, v.grad

    for kind in ("causal", "encoder", "left"):
        mask, causal = _mask(kind, B, T, _edge_arg(kind, T), dev)
        qv, kv, vv = [view_of(x) for x in vals[:3]]
        assert not qv.is_contiguous() and qv.data_ptr() % 16 == 0 and all(s % 8 == 0 for s in qv.stride()[:3])
        assert attention.supported(qv.detach().requires_grad_(True), kv, vv, mask, 0.0, causal, {})
        got = run(_sdpa_ours(mask, scale, causal), qv, kv, vv)
        want = run(_sdpa_ours(mask, scale, causal), *[x.contiguous() for x in vals[:3]])
        for name, a, b in zip(("o", "dq", "dk", "dv"), got, want):
            assert torch.isfinite(a).all(), (kind, name)
            assert torch.equal(a, b), (kind, name, float((a.float() - b.float()).abs().max()))
        lse_v = _lse_pair(qv, kv, vv, mask, scale, causal)[0]
        lse_c = _lse_pair(*[x.contiguous() for x in vals[:3]], mask, scale, causal)[0]
        assert torch.isfinite(lse_v).all() and torch.equal(lse_v, lse_c), kind


# ---------------------------------------------------------------------------------------------------------------------------
# 2. long lengths up to the limit
# ---------------------------------------------------------------------------------------------------------------------------
LONG_T = [1023, 1025, 2047, 2048]


def _long_arg(kind, T):
    return {"left": [0, T - 70], "encoder": [T, T - 129]}.get(kind)


@pytest.mark.parametrize("kind", ["causal", "left", "encoder"])
@pytest.mark.parametrize("T", LONG_T)
@pytest.mark.parametrize("hd", [32, 64, 128])
def test_long_lengths_up_to_the_limit(dev, hd, T, kind):
    B, H = 2, 2
    q, k, v, go = _inputs(B, H, T, hd, "bthd", 10 * T + hd, dev)
    mask, causal = _mask(kind, B, T, _long_arg(kind, T), dev)
    _check_padded(f"long:hd{hd}:T{T}:{kind}", q, k, v, go, mask, causal, hd ** -0.5, dense=True)


@pytest.mark.parametrize("H,T,hd", [(2, 2048, 64), (2, 1030, 128), (2, 1030, 32)])
def test_dropout_at_long_lengths(dev, H, T, hd):
    """tests/test_attention_gpu.py's dropout test at T 2048 / 1030: float64 with oracle/attn_dropout.py's keep mask for the device
    seed; kernels that drew other bits at large element indices would miss the 1.2e-2 bound by an order of magnitude.  (hd 128
    with dropout runs the first-form dk / dv kernel.)"""
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
    import attn_dropout as AD

    from dalm_amd.models import attention, lora_ops

    B, p, salt = 1, 0.1, 0x5A17
    q, k, v, go = _inputs(B, H, T, hd, "bthd", T + hd, dev, gain=1.0)
    lens = [T - 129]
    mask = encoder_mask(B, T, lens, dev)
    scale = hd ** -0.5
    assert attention.supported(q.requires_grad_(True), k, v, mask, p, False, {})
    seed = int(lora_ops.dropout_seed(dev).item())
    keep = torch.from_numpy(AD.keep_mask(seed, salt, B, H, T, p)).to(dev)
    assert abs(float((~keep).float().mean()) - p) < 0.01
    ours = run_grad(lambda a, b, c: attention.sdpa(a, b, c, mask, scale, False, p, salt), q, k, v, go)
    ref = attn_ref64(q, k, v, live_matrix(mask, False, B, T, dev), scale, go, keep=keep, keep_scale=1.0 / (1.0 - p))
    for name, a, r in zip(("o", "dq", "dk", "dv"), ours, ref[:4]):
        assert torch.isfinite(a).all(), name
        e = norm_rel_err(a, r)
        record_measured(f"attn_extents:dropout:hd{hd}:T{T}:{name}", {"norm": e})
        assert e < 1.2e-2, (name, e)
    assert float(ours[2][0, :, lens[0]:].abs().max()) == 0.0 and float(ours[3][0, :, lens[0]:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# 3. grouped heads and packed sequences at the same extents
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=[0, 1], ids=["split-by-grid", "unsplit"])
def splits(request, monkeypatch):
    """tests/test_attention_gqa_gpu.py's fixture - the dk / dv form: 0 = the library's choice by grid size, 1 = one workgroup per KV
    head running through its whole group."""
    from dalm_amd.models import attention

    monkeypatch.setattr(attention, "_gqa_splits", [request.param])
    return request.param


@pytest.mark.parametrize("kind", ["causal", "left"])
@pytest.mark.parametrize("T", [129, 1025, 2048])
@pytest.mark.parametrize("hd,H,Hkv", [(128, 4, 2), (64, 8, 2)])
def test_grouped_heads_at_the_extents(dev, splits, hd, H, Hkv, T, kind):
    """`dalm_attn_gqa_*` against float64 under the per-row rule - the yardstick is the expanded path's error
    (tests/test_attention_gqa_gpu.py's rule: the equal-heads kernels on repeat_kv-materialised k / v) - with that file's
    bit-equality of o, lse and dq."""
    from dalm_amd.models import attention

    B, G = 2, H // Hkv
    q, k, v, go = _inputs(B, H, T, hd, "bthd", 1000 * H + T + hd, dev, Hkv=Hkv)
    mask, causal = _mask(kind, B, T, [0, T - 70], dev)
    scale = hd ** -0.5
    assert attention.grouped_supported(q.requires_grad_(True), k, v, mask, 0.0, causal, {})

    def expand(t):
        return t.repeat_interleave(G, dim=1)

    native = run_grad(_sdpa_ours(mask, scale, causal), q, k, v, go)
    expanded = run_grad(lambda a, b, c: attention._SdpaHipBackward.apply(a, expand(b), expand(c), mask, scale, causal), q, k, v, go)
    live = live_matrix(mask, causal, B, T, dev)
    ref = attn_ref64(q, k, v, live, scale, go)
    pk = attention._pack(mask, B, H, T, causal, q.dtype, q.device)
    with torch.no_grad():
        lse_n = attention._attn_forward(q, k, v, pk, scale, causal)[1]
        lse_e = attention._attn_forward(q, expand(k), expand(v), pk, scale, causal)[1]
    assert lse_n.shape == (B, H, T) and torch.equal(lse_n, lse_e)
    assert torch.equal(native[0], expanded[0]) and torch.equal(native[1], expanded[1])
    tag = f"grouped:hd{hd}:H{H}:T{T}:{kind}:splits{splits}"
    for name, a, b, r in zip(("o", "dq", "dk", "dv"), native, expanded, ref[:4]):
        assert a.shape == r.shape, name
        assert_rows_close(f"{tag}:{name}", a, b, r, record=f"attn_extents:{tag}:{name}")
    _check_zero_rows(native, live)


PACKED_CASES = [
    # B, H, T, lens, left padding, causal, head width, with rotary
    (4, 2, 2048, [2048, 0, 1, 1300], True, True, 128, True),
    (3, 2, 1025, [1025, 33, 700], False, False, 64, False),
    (3, 2, 1025, [1025, 33, 700], False, False, 32, False),
]


@pytest.mark.parametrize("B,H,T,lens,left,causal,hd,rope", PACKED_CASES)
def test_packed_sequences_at_the_extents(dev, B, H, T, lens, left, causal, hd, rope):
    """The scheme of tests/test_packed_gpu.py::test_packed_attention_kernels_vs_float64_and_padded - per-sequence float64, torch's
    bf16 kernels on the re-padded tensors as the yardstick - under the per-row rule, with exact zeros at slack rows and key-dead
    rows."""
    from dalm_amd import packed
    from dalm_amd.models import attention, tower_ops

    g = torch.Generator().manual_seed(B * 1000 + T + hd)
    ar = torch.arange(T).unsqueeze(0)
    L = torch.tensor(lens).unsqueeze(1)
    m2 = ((ar >= T - L) if left else (ar < L)).long()
    rows, cu = packed.pack_plan(m2, shifted=causal, multiple=64)
    n = rows.numel()
    _ids, pos, desc, _valid = packed.packed_inputs(torch.zeros(B, T, dtype=torch.long, device=dev), m2.to(dev), rows.to(dev), cu.to(dev),
                                                   causal)
    seqs = packed.packed_of(desc)
    assert seqs is not None and seqs.T == T
    q, k, v, go = [(0.7 * torch.randn(1, n, H, hd, generator=g)).to(dev, torch.bfloat16).transpose(1, 2) for _ in range(4)]
    scale = hd ** -0.5
    cos = sin = None
    if rope:
        inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, device=dev).float() / hd))
        ang = pos[0].float()[:, None] * inv[None, :]
        cos = torch.cat((ang.cos(), ang.cos()), -1).to(torch.bfloat16)[None]
        sin = torch.cat((ang.sin(), ang.sin()), -1).to(torch.bfloat16)[None]
        assert attention.rope_fusable(q, k, cos, sin)
    assert attention.packed_supported(q, k, v)

    def ours(a, b, c):
        return attention.rope_sdpa(a, b, c, cos, sin, desc, scale, False) if rope else attention.sdpa(a, b, c, desc, scale, False)

    def torch_path(a, b, c):
        if rope:
            a, b = tower_ops.rope_qk(a, b, cos, sin)
        return attention._packed_sdpa_torch(a, b, c, seqs, scale, 0.0).transpose(1, 2)

    got = run_grad(ours, q, k, v, go)
    alt = run_grad(torch_path, q, k, v, go)

    def rot(x):                                   # the rotation in float64 from the bf16 tables
        if not rope:
            return x
        xr = torch.cat((-x[..., hd // 2:], x[..., :hd // 2]), -1)
        return x * cos.double()[:, None] + xr * sin.double()[:, None]

    q64, k64 = [t.detach().double().requires_grad_(True) for t in (q, k)]
    qr, kr = rot(q64), rot(k64)
    # rounding the rotated tensors to bf16 is part of both implementations: the reference is evaluated on the rounded values
    qr_b, kr_b = qr.detach().to(torch.bfloat16), kr.detach().to(torch.bfloat16)
    want = [torch.zeros(1, H, n, hd, dtype=torch.float64, device=dev) for _ in range(4)]
    dead_q = torch.ones(n, dtype=torch.bool, device=dev)
    for b in range(cu.numel() - 1):
        a, e = int(cu[b]), int(cu[b + 1])
        if e == a:
            continue
        kl = seqs.key_live[a:e].bool()
        live = kl[None, :].expand(e - a, e - a)
        if causal:
            live = live & torch.ones(e - a, e - a, dtype=torch.bool, device=dev).tril()
        dead_q[a:e] = ~live.any(-1)
        res = attn_ref64(qr_b[:, :, a:e], kr_b[:, :, a:e], v[:, :, a:e], live[None], scale, go[:, :, a:e])
        for dst, src in zip(want, res[:4]):
            dst[:, :, a:e] = src
    if rope:                                      # chain the rotation's backward in float64
        qr.backward(want[1])
        kr.backward(want[2])
        want[1], want[2] = q64.grad, k64.grad
    tag = f"packed:hd{hd}:T{T}:{'causal' if causal else 'encoder'}"
    for name, gt, al, wt in zip(("o", "dq", "dk", "dv"), got, alt, want):
        assert_rows_close(f"{tag}:{name}", gt, al, wt, record=f"attn_extents:{tag}:{name}")
    dead_k = seqs.key_live == 0
    assert int(dead_q.sum()) >= n - int(seqs.cu[B]) and int(dead_k.sum()) >= n - int(seqs.cu[B])       # the slack rows at least
    assert float(got[0][0, :, dead_q].abs().max()) == 0.0 and float(got[1][0, :, dead_q].abs().max()) == 0.0
    assert float(got[2][0, :, dead_k].abs().max()) == 0.0 and float(got[3][0, :, dead_k].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# 4. values at the edges: T 129, head widths 64 and 128, causal and encoder mask
# ---------------------------------------------------------------------------------------------------------------------------
VAL_T, VAL_B, VAL_H = 129, 2, 2
VAL_KINDS = ["causal", "encoder"]


def _val_mask(kind, dev):
    return _mask(kind, VAL_B, VAL_T, [VAL_T, VAL_T // 2], dev)


@pytest.mark.parametrize("kind", VAL_KINDS)
@pytest.mark.parametrize("hd", [64, 128])
def test_near_one_hot_probabilities(dev, hd, kind):
    """q, k ~ N(0, 30): the scaled scores q k / sqrt(hd) have a standard deviation of about 30, the softmax of a row sits on one
    key (float64, 129 keys: > 0.99 on one key for over 95 % of the rows)."""
    q, k, v, go = _inputs(VAL_B, VAL_H, VAL_T, hd, "bthd", 31 * hd + 1, dev)
    g = torch.Generator().manual_seed(hd)
    q, k = [(torch.randn(VAL_B, VAL_T, VAL_H, hd, generator=g) * 30.0 ** 0.5).bfloat16().to(dev).transpose(1, 2) for _ in range(2)]
    mask, causal = _val_mask(kind, dev)
    scale = hd ** -0.5
    live = live_matrix(mask, causal, VAL_B, VAL_T, dev)
    s = ((q.double() @ k.double().transpose(-1, -2)) * scale).masked_fill(~live[:, None], float("-inf"))
    assert 20.0 < float(s[torch.isfinite(s)].std()) < 45.0
    assert float(torch.softmax(s, -1).amax(-1).median()) > 0.9
    _check_padded(f"one-hot:hd{hd}:{kind}", q, k, v, go, mask, causal, scale, record=False)


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["plus80", "minus80"])
@pytest.mark.parametrize("kind", VAL_KINDS)
@pytest.mark.parametrize("hd", [64, 128])
def test_common_offset_on_every_score_of_a_row(dev, hd, kind, sign):
    """k' = k + c u, q' = q + d u with u = e_0 and q, k orthogonal to u: every scaled score moves by c d / sqrt(hd) = +-80 (hd 64:
    32 x 20 / 8; hd 128: 32 x 28.25 / 11.31 = 79.9; all exact in bf16).  Float64 softmax is shift-invariant; the online maximum
    of the forward and exp2(c1 S + nl) of the backward have to carry it.  The reference is evaluated on the bf16 inputs."""
    q, k, v, go = [t.clone() for t in _inputs(VAL_B, VAL_H, VAL_T, hd, "bhtd", 17 * hd + 3, dev)]
    c, d = 32.0, {64: 20.0, 128: 28.25}[hd]
    k[..., 0] = c
    q[..., 0] = sign * d
    assert float(q[..., 0].float().abs().max()) == d and float(k[..., 0].float().max()) == c       # survive bf16
    scale = hd ** -0.5
    assert abs(c * d * scale - 80.0) < 0.2
    mask, causal = _val_mask(kind, dev)
    _, ref, live, lse = _check_padded(f"offset{int(sign * 80)}:hd{hd}:{kind}", q, k, v, go, mask, causal, scale, record=False)
    assert float((ref[4][live.any(-1)[:, None].expand_as(ref[4])] - sign * c * d * scale).abs().max()) < 15.0   # the offset is in the lse


@pytest.mark.parametrize("kind", VAL_KINDS)
@pytest.mark.parametrize("hd", [64, 128])
def test_all_zero_queries(dev, hd, kind):
    """q = 0: uniform probabilities over the live keys, o is the mean of the live v rows (the float64 reference IS that mean; to
    bf16 accuracy = no further from it than torch's kernel), dq against float64, dk exactly 0."""
    q, k, v, go = _inputs(VAL_B, VAL_H, VAL_T, hd, "bthd", 13 * hd + 5, dev)
    q = torch.zeros_like(q)
    mask, causal = _val_mask(kind, dev)
    ours, ref, live, lse = _check_padded(f"zero-q:hd{hd}:{kind}", q, k, v, go, mask, causal, hd ** -0.5, record=False)
    w = live.double() / live.sum(-1, keepdim=True).clamp_min(1)
    mean_v = w[:, None] @ v.double()
    assert float((ref[0] - mean_v).abs().max()) < 1e-12
    assert float(ours[2].abs().max()) == 0.0
    cnt = live.sum(-1)[:, None].expand_as(lse)
    assert float((lse.double() - cnt.double().log()).abs().max()) <= LSE_OFFSET                   # lse = ln(live keys)


@pytest.mark.parametrize("hd", [64, 128])
def test_rows_whose_only_live_key_is_themselves(dev, hd):
    """Causal row 0 (position 0) and the left-padded sequence that starts at T - 1 (position T - 1): o equals the row's own v row
    bit for bit, the log-sum-exp equals the scaled self-score (to what torch's own lse shows against float64 x 1.5 + 1e-4:
    `_check_padded`'s lse rule, whose reference at such a row is that score)."""
    T, B, H = VAL_T, VAL_B, VAL_H
    q, k, v, go = _inputs(B, H, T, hd, "bthd", 11 * hd + 7, dev)
    scale = hd ** -0.5
    self_score = (q.double() * k.double()).sum(-1) * scale                                         # [B, H, T]
    for kind, arg, rows in (("causal", None, [(0, 0), (1, 0)]), ("left", [0, T - 1], [(0, 0), (1, T - 1)])):
        mask, causal = _mask(kind, B, T, arg, dev)
        ours, ref, live, lse = _check_padded(f"self-only:hd{hd}:{kind}", q, k, v, go, mask, causal, scale, record=False)
        for b, i in rows:
            assert int(live[b, i].sum()) == 1 and bool(live[b, i, i])
            assert torch.equal(ours[0][b, :, i], v[b, :, i])
            assert float((ref[4][b, :, i] - self_score[b, :, i]).abs().max()) < 1e-12
            assert float((lse[b, :, i].double() - self_score[b, :, i]).abs().max()) <= LSE_OFFSET
