"""`dalm_attn_rel_*` (attention with a per-head relative-position bias vector, MPNet) on the GPU: o, dq, dk, dv under the
project's row rule (`helpers.assert_rows_close`: no further from float64 than torch's bf16 result on the same inputs, x 1.5 +
1e-3 - torch's SDPA with attn_mask = bias + key mask as a float mask), the log-sum-exp within 2e-3, padded and packed (columns
implied, explicit, with a hole), with dropout, and two identities: a zero vector gives the bias-free entry points' bits, a
constant added to a head's vector moves only the log-sum-exp.

`helpers.attn_ref64` is extended HERE by the bias term (`_ref64`)."""
import sys
from pathlib import Path

import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu

H, HD = 3, 64
SCALE = HD ** -0.5
LSE_ATOL = 2e-3


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


def _rel_vector(Tc, seed, dev):
    """N(0, 2) per (head, difference), asymmetric in the sign of d: a dropped, mirrored or mis-indexed bias fails by orders of
    magnitude."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(H, 2 * Tc - 1, generator=g) * 2.0).to(dev)


def _bias(rel, cols):
    """[H, T, T] float32: rel[h, cols[j] - cols[i] + Tc - 1]."""
    Tc = (rel.shape[1] + 1) // 2
    idx = cols[None, :] - cols[:, None] + (Tc - 1)
    return rel[:, idx]


def _ref64(q, k, v, live, bias, scale, go, keep=None, keep_scale=1.0):
    """`helpers.attn_ref64` with the additive score term `bias` [H, T, T] (the same for every batch row)."""
    outs = [[] for _ in range(5)]
    for b in range(q.shape[0]):
        qb, kb, vb = [t[b].detach().double().requires_grad_(True) for t in (q, k, v)]
        s = (qb @ kb.transpose(-1, -2)) * scale + bias.double()
        s = s.masked_fill(~live[b][None], float("-inf"))
        p = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)
        if keep is not None:
            p = p * keep[b].double() * keep_scale
        o = p @ vb
        o.backward(go[b].double())
        for dst, t in zip(outs, (o.detach(), qb.grad, kb.grad, vb.grad, torch.logsumexp(s.detach(), -1))):
            dst.append(t)
    return tuple(torch.stack(t) for t in outs)


def _torch_bf16(q, k, v, live, bias, scale, go, keep=None, keep_scale=1.0):
    """torch's bf16 result on the same inputs: SDPA with the float mask bias + key mask; with a keep mask (dropout) the same
    statements as bf16 tensor ops, because SDPA draws its own."""
    fm = bias[None].float().expand(q.shape[0], -1, -1, -1).masked_fill(~live[:, None], float("-inf")).to(q.dtype)
    if keep is None:
        return helpers.run_grad(lambda a, b, c: torch.nn.functional.scaled_dot_product_attention(a, b, c, attn_mask=fm, scale=scale),
                                q, k, v, go)

    # The fused kernels (torch's, which are the yardstick at p = 0, and this library's) keep O in bf16 and take
    # D = rowsum(dO o O) from it in dS = P o (dP - D).  Autograd through an eager chain takes D from P instead, so where dS
    # cancels exactly (a row with ONE live key: true dq = 0) it sees none of the rounding of O = bf16(v / (1 - p)) that every
    # fused kernel carries (2^-9 |dO . v| per element).  The yardstick therefore states the same formulas in torch bf16 ops:
    # bf16 matmuls (bf16 results), softmax and the dS arithmetic in f32.  (With autograd as the yardstick the single-key rows of
    # dq measured 2.13e-2 against 1.5 x 1.23e-2 + 1e-3 at T 64.)
    ks = keep.float() * keep_scale
    s = ((q @ k.transpose(-1, -2)).float() * scale + fm.float())
    p = torch.softmax(s, -1)
    pd = (p * ks).to(q.dtype)
    o = pd @ v
    dv = pd.transpose(-1, -2) @ go
    dp = (go @ v.transpose(-1, -2)).float() * ks
    d = (go.float() * o.float()).sum(-1, keepdim=True)
    ds = (p * (dp - d)).to(q.dtype)
    dq = ((ds @ k).float() * scale).to(q.dtype)
    dk = ((ds.transpose(-1, -2) @ q).float() * scale).to(q.dtype)
    return o, dq, dk, dv


def _launch(q, k, v, go, rel, mask, cols=None, drop=(0.0, None, 0), bias_free=False):
    """(o, dq, dk, dv, lse) straight from the launchers of models/attention.py (the autograd node keeps lse to itself)."""
    from dalm_amd.models import attention

    B, Hh, T, hd = q.shape
    pk = attention._pack(mask, B, Hh, T, False, q.dtype, q.device)
    if bias_free:
        o, lse = attention._attn_forward(q, k, v, pk, SCALE, False, drop)
        dq, dk, dv = attention._attn_backward(q, k, v, o, lse, go, pk, SCALE, drop=drop)
    else:
        o, lse = attention._rel_launch_forward(q, k, v, pk, SCALE, rel, cols, drop)
        dq, dk, dv = attention._rel_launch_backward(q, k, v, o, lse, go, pk, SCALE, rel, cols, drop)
    torch.cuda.synchronize()
    return o, dq, dk, dv, lse


def _inputs(B, T, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, T, H, HD, generator=g) * 1.2).bfloat16().to(dev).transpose(1, 2) for _ in range(4)]


def _check(name, ours, theirs, ref, live_rows=None):
    for nm, a, b, r in zip(("o", "dq", "dk", "dv"), ours[:4], theirs, ref[:4]):
        helpers.assert_rows_close(f"{name} {nm}", a, b, r)
    lse, want = ours[4].double(), ref[4]
    sel = torch.isfinite(want) if live_rows is None else live_rows
    err = float((lse[sel] - want[sel]).abs().max())
    print(f"{name}: lse max abs error {err:.3e}")
    assert err <= LSE_ATOL, (name, err)


def _padded_case(T, dev):
    B = 2
    lens = (T, 1)                                                  # one full row, one row with a single live key
    q, k, v, go = _inputs(B, T, 100 + T, dev)
    mask = helpers.encoder_mask(B, T, lens, dev)
    live = helpers.live_matrix(mask, False, B, T, dev)
    rel = _rel_vector(T, T, dev)
    bias = _bias(rel, torch.arange(T, device=dev))
    return q, k, v, go, mask, live, rel, bias


_REFS: dict = {}


def _padded_ref(T, dev):
    """float64 + torch's bf16 yardstick of the padded case at T: computed once, shared, never modified."""
    if T not in _REFS:
        q, k, v, go, mask, live, rel, bias = _padded_case(T, dev)
        _REFS[T] = (_ref64(q, k, v, live, bias, SCALE, go), _torch_bf16(q, k, v, live, bias, SCALE, go))
    return _REFS[T]


@pytest.mark.parametrize("T", [2, 33, 64, 65, 128, 130, 200, 512])
def test_padded_against_float64(dev, T):
    q, k, v, go, mask, live, rel, bias = _padded_case(T, dev)
    ref, theirs = _padded_ref(T, dev)
    ours = _launch(q, k, v, go, rel, mask)
    _check(f"padded T {T}", ours, theirs, ref)


@pytest.mark.parametrize("T", [64, 130])
def test_padded_autograd_node_and_longer_vector(dev, T):
    """The autograd node (what the model calls) returns the launchers' bits; a vector built for a longer Tc gives the same result."""
    from dalm_amd.models import attention

    q, k, v, go, mask, live, rel, bias = _padded_case(T, dev)
    ours = _launch(q, k, v, go, rel, mask)
    node = helpers.run_grad(lambda a, b, c: attention._RelSdpaHip.apply(a, b, c, rel, mask, SCALE), q, k, v, go)
    for a, b in zip(node, ours[:4]):
        assert torch.equal(a, b)
    longer = torch.zeros(H, 2 * (T + 9) - 1, device=dev)
    longer[:, 9:9 + 2 * T - 1] = rel
    again = _launch(q, k, v, go, longer, mask)
    for a, b in zip(again, ours):
        assert torch.equal(a, b)


def _keep_mask(dev, salt, B, T, p):
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
    import attn_dropout as AD

    from dalm_amd.models import lora_ops

    seed = lora_ops.dropout_seed_snapshot(dev)
    keep = torch.from_numpy(AD.keep_mask(int(lora_ops.dropout_seed(dev).item()), salt, B, H, T, p)).to(dev)
    return seed, keep


@pytest.mark.parametrize("T", [64, 130])
def test_padded_dropout(dev, T):
    p, salt = 0.1, 0x5A17
    q, k, v, go, mask, live, rel, bias = _padded_case(T, dev)
    seed, keep = _keep_mask(dev, salt, 2, T, p)
    ours = _launch(q, k, v, go, rel, mask, drop=(p, seed, salt))
    ref = _ref64(q, k, v, live, bias, SCALE, go, keep, 1.0 / (1.0 - p))
    theirs = _torch_bf16(q, k, v, live, bias, SCALE, go, keep, 1.0 / (1.0 - p))
    _check(f"padded dropout T {T}", ours, theirs, ref)
    plain = _launch(q, k, v, go, rel, mask)
    assert not torch.equal(plain[0], ours[0])


def _packed(lens, cols, Tm, dev, key_live=None):
    from dalm_amd import packed

    n = sum(lens)
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=dev)
    kl = torch.ones(n, dtype=torch.uint8, device=dev) if key_live is None else key_live
    seqs = packed.PackedSeqs(cu=cu, nseq=len(lens), T=Tm, n=n, key_live=kl, causal=False)
    seqs.cols = cols
    return packed.attach(torch.ones((1, 1, 1, 1), dtype=torch.bool, device=dev), seqs)


def _packed_reference(q, k, v, go, lens, cols, rel):
    """Per sequence: float64 and torch's bf16 yardstick at the tokens' column differences, joined along the token axis."""
    refs, theirs, lses = [[] for _ in range(4)], [[] for _ in range(4)], []
    r0 = 0
    for n in lens:
        sl = slice(r0, r0 + n)
        c = torch.arange(n, device=q.device) if cols is None else cols[sl].long()
        bias = _bias(rel, c)
        live = torch.ones(1, n, n, dtype=torch.bool, device=q.device)
        part = [t[:, :, sl] for t in (q, k, v)]
        g = go[:, :, sl]
        r = _ref64(*part, live, bias, SCALE, g)
        t = _torch_bf16(*part, live, bias, SCALE, g)
        for dst, x in zip(refs, r[:4]):
            dst.append(x)
        for dst, x in zip(theirs, t):
            dst.append(x)
        lses.append(r[4][0])                                        # [H, n]
        r0 += n
    return [torch.cat(x, dim=2) for x in refs], [torch.cat(x, dim=2) for x in theirs], lses


def _check_packed(name, ours, theirs, refs, lses, lens):
    for nm, a, b, r in zip(("o", "dq", "dk", "dv"), ours[:4], theirs, refs):
        helpers.assert_rows_close(f"{name} {nm}", a, b, r)
    for b, n in enumerate(lens):
        err = float((ours[4][b, :, :n].double() - lses[b]).abs().max())
        print(f"{name}: sequence {b} lse max abs error {err:.3e}")
        assert err <= LSE_ATOL, (name, b, err)


@pytest.mark.parametrize("explicit", [False, True])
def test_packed_against_float64(dev, explicit):
    lens = (1, 7, 64, 65, 130)
    n, Tm = sum(lens), 130
    q, k, v, go = _inputs(1, n, 7, dev)
    rel = _rel_vector(Tm, 11, dev)
    cols = torch.cat([torch.arange(x, dtype=torch.int32) for x in lens]).to(dev) if explicit else None
    desc = _packed(lens, cols, Tm, dev)
    ours = _launch(q, k, v, go, rel, desc, cols)
    refs, theirs, lses = _packed_reference(q, k, v, go, lens, cols, rel)
    _check_packed(f"packed explicit {explicit}", ours, theirs, refs, lses, lens)


def test_packed_with_a_hole(dev):
    """One sequence whose live columns are 0..9 and 20..69 of a 70-column row (plus a plain one): differences are the ORIGINAL
    columns' - with the local row index the second run's bias would be off by ten columns."""
    Tm = 70
    c0 = torch.cat((torch.arange(10), torch.arange(20, 70))).to(torch.int32)
    lens = (int(c0.numel()), 33)
    cols = torch.cat((c0, torch.arange(33, dtype=torch.int32))).to(dev)
    q, k, v, go = _inputs(1, sum(lens), 13, dev)
    rel = _rel_vector(Tm, 17, dev)
    desc = _packed(lens, cols, Tm, dev)
    ours = _launch(q, k, v, go, rel, desc, cols)
    refs, theirs, lses = _packed_reference(q, k, v, go, lens, cols, rel)
    _check_packed("packed hole", ours, theirs, refs, lses, lens)
    wrong = _launch(q, k, v, go, rel, desc, None)                    # local indices: another bias
    assert not torch.equal(wrong[0][:, :, :lens[0]], ours[0][:, :, :lens[0]])
    assert torch.equal(wrong[0][:, :, lens[0]:], ours[0][:, :, lens[0]:])


@pytest.mark.parametrize("T,p", [(65, 0.0), (130, 0.0), (130, 0.1), (512, 0.0)])
def test_zero_vector_is_the_bias_free_kernels_bits(dev, T, p):
    q, k, v, go, mask, live, rel, bias = _padded_case(T, dev)
    drop = (0.0, None, 0)
    if p:
        drop = (p, _keep_mask(dev, 77, 2, T, p)[0], 77)
    zero = torch.zeros_like(rel)
    a = _launch(q, k, v, go, zero, mask, drop=drop)
    b = _launch(q, k, v, go, None, mask, drop=drop, bias_free=True)
    for nm, x, y in zip(("o", "dq", "dk", "dv", "lse"), a, b):
        assert torch.equal(x, y), nm


@pytest.mark.parametrize("explicit", [False, True])
def test_zero_vector_is_the_bias_free_kernels_bits_packed(dev, explicit):
    lens = (1, 7, 64, 65, 130)
    n, Tm = sum(lens), 130
    q, k, v, go = _inputs(1, n, 23, dev)
    cols = torch.cat([torch.arange(x, dtype=torch.int32) for x in lens]).to(dev) if explicit else None
    desc = _packed(lens, cols, Tm, dev)
    a = _launch(q, k, v, go, torch.zeros(H, 2 * Tm - 1, device=dev), desc, cols)
    b = _launch(q, k, v, go, None, desc, bias_free=True)
    for nm, x, y in zip(("o", "dq", "dk", "dv"), a, b):
        assert torch.equal(x, y), nm
    for s, ln in enumerate(lens):
        assert torch.equal(a[4][s, :, :ln], b[4][s, :, :ln])


def test_constant_shift_moves_only_the_lse(dev):
    T = 130
    q, k, v, go, mask, live, rel, bias = _padded_case(T, dev)
    ref, theirs = _padded_ref(T, dev)
    shift = torch.tensor([3.0, -1.5, 0.75], device=dev)
    ours = _launch(q, k, v, go, rel + shift[:, None], mask)
    for nm, a, b, r in zip(("o", "dq", "dk", "dv"), ours[:4], theirs, ref[:4]):
        helpers.assert_rows_close(f"shifted {nm}", a, b, r)
    want = ref[4] + shift.double()[None, :, None]
    err = float((ours[4].double() - want).abs().max())
    print(f"shifted: lse max abs error {err:.3e}")
    assert err <= LSE_ATOL, err
