"""Shared helpers for the test-suite (golden loading, seeded synthetic batches)."""
from pathlib import Path

import numpy as np
import torch

GOLDEN = Path(__file__).resolve().parent / "golden"
LOSS_CASES = sorted(p.stem for p in GOLDEN.glob("loss_*.npz"))
POOL_CASES = sorted(p.stem for p in GOLDEN.glob("pool_*.npz"))


def load_npz(name: str):
    with np.load(GOLDEN / f"{name}.npz") as z:
        return {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def norm_rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def record_measured(key, values):
    """What a GPU run measured, kept beside its other outputs: tests/test_tower_ops_gpu.py's `_record_measured` (the file it
    writes is named there)."""
    from test_tower_ops_gpu import _record_measured

    _record_measured(key, values)


# ---------------------------------------------------------------------------------------------------------------------------
# attention: float64 evaluation and the per-row rule (tests/test_attention_extents_gpu.py, tests/test_attention_row_rule.py)
# ---------------------------------------------------------------------------------------------------------------------------
# "no further from float64 than torch's kernel, x 1.5 + 1e-3" - the project's rule (tests/test_attention_gpu.py), which
# `assert_rows_close` applies to the whole tensor AND to the worst row
ROW_FACTOR, ROW_OFFSET = 1.5, 1e-3


def hf_mask(B, T, starts, dev):
    """HF's causal + left-padding mask [B, 1, T, T]: sequence b lives in columns starts[b] .. T - 1."""
    col = torch.arange(T, device=dev)
    st = torch.tensor(starts, device=dev)
    return ((col[None, None, :] <= col[None, :, None]) & (col[None, None, :] >= st[:, None, None]))[:, None]


def encoder_mask(B, T, lens, dev):
    """transformers' bidirectional key-padding mask: [B, 1, 1, T] expanded to [B, 1, T, T] (row stride 0)."""
    col = torch.arange(T, device=dev)
    return (col[None, :] < torch.tensor(lens, device=dev)[:, None])[:, None, None, :].expand(B, 1, T, T)


def live_matrix(mask, causal, B, T, dev):
    """bool [B, T, T]: query row i of batch row b attends key j."""
    live = torch.ones(T, T, dtype=torch.bool, device=dev)
    if causal:
        live = live.tril()
    live = live[None].expand(B, T, T)
    return live if mask is None else (live & mask[:, 0])


def attn_ref64(q, k, v, live, scale, go, keep=None, keep_scale=1.0):
    """float64 masked softmax attention and its gradients, one batch row at a time (the scores of [H, 2048, 2048] are 34 MB
    per head).  q, go: [B, H, T, hd]; k, v: [B, Hkv, T, hd] with Hkv | H (transformers' repeat_kv inside the graph: k.grad /
    v.grad come back with Hkv heads); live: bool [B, T, T]; keep: optional bool [B, H, T, T] dropout mask, P o keep x
    keep_scale in front of P V.  Rows without a live key: zero output, zero gradient, log-sum-exp -inf.
    Returns (o, dq, dk, dv, lse), lse = natural-log logsumexp of the masked scaled scores [B, H, T]."""
    G = q.shape[1] // k.shape[1]
    outs = [[] for _ in range(5)]
    for b in range(q.shape[0]):
        qb, kb, vb = [t[b].detach().double().requires_grad_(True) for t in (q, k, v)]
        kx, vx = (kb.repeat_interleave(G, dim=0), vb.repeat_interleave(G, dim=0)) if G > 1 else (kb, vb)
        s = (qb @ kx.transpose(-1, -2)) * scale
        s = s.masked_fill(~live[b][None], float("-inf"))
        p = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)
        if keep is not None:
            p = p * keep[b].double() * keep_scale
        o = p @ vx
        o.backward(go[b].double())
        for dst, t in zip(outs, (o.detach(), qb.grad, kb.grad, vb.grad, torch.logsumexp(s.detach(), -1))):
            dst.append(t)
        del s, p, o
    return tuple(torch.stack(t) for t in outs)


def run_grad(fn, q, k, v, go):
    q, k, v = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    o = fn(q, k, v)
    o.backward(go)
    return o.detach(), q.grad, k.grad, v.grad


def row_errors(x, ref64):
    """e(r) = ||x_r - ref_r||_2 / (||ref_r||_2 + s) for every row r = (b, h, i) of [B, H, T, hd] tensors, s = the RMS of the
    reference's row norms over the whole tensor: a row whose reference is (near) zero is measured against the tensor's scale,
    so no row needs to be left out."""
    ref = ref64.detach().double()
    x = x.detach().to(ref.device).double()
    rn = ref.norm(dim=-1)
    s = rn.square().mean().sqrt()
    return (x - ref).norm(dim=-1) / (rn + s + 1e-300)


def rows_report(got, torch_got, ref64):
    """Both rules for one tensor: whole-tensor relative norm and worst row, ours and torch's, against float64."""
    ref = ref64.detach().double()
    e_g, e_t = row_errors(got, ref), row_errors(torch_got, ref)
    flat = int(torch.nan_to_num(e_g, nan=float("inf")).argmax())
    T = e_g.shape[-1]
    b, h, i = flat // (e_g.shape[1] * T), (flat // T) % e_g.shape[1], flat % T
    den = float(ref.norm()) + 1e-30
    n_g = float((got.detach().to(ref.device).double() - ref).norm()) / den
    n_t = float((torch_got.detach().to(ref.device).double() - ref).norm()) / den
    m_g, m_t = float(e_g.max()), float(e_t.max())
    return {"row_max": m_g, "row_max_torch": m_t, "worst_row": [b, h, i], "norm": n_g, "norm_torch": n_t,
            "finite": bool(torch.isfinite(got).all()),
            "norm_ok": n_g <= ROW_FACTOR * n_t + ROW_OFFSET, "rows_ok": m_g <= ROW_FACTOR * m_t + ROW_OFFSET}


def assert_rows_close(name, got, torch_got, ref64, record=None):
    """`got` [B, H, T, hd] is finite, no further from `ref64` than `torch_got` is (x 1.5 + 1e-3) as a whole tensor, and its WORST
    ROW is no further from the reference's row than torch's worst row is from its own (x 1.5 + 1e-3, errors as `row_errors`
    defines them).  `torch_got` is torch's bf16 result on the same inputs: the yardstick is torch against float64, never the
    code under test.  `record`: key under which both maxima are recorded (`record_measured`)."""
    rep = rows_report(got, torch_got, ref64)
    if record is not None:
        record_measured(record, {k: rep[k] for k in ("row_max", "row_max_torch", "worst_row", "norm", "norm_torch")})
    b, h, i = rep["worst_row"]
    where = (f"{name}: worst row (b, h, i) = ({b}, {h}, {i}), i % 32 = {i % 32}, i % 64 = {i % 64}, i % 128 = {i % 128}; "
             f"row maximum {rep['row_max']:.3e} against torch's {rep['row_max_torch']:.3e}; "
             f"whole tensor {rep['norm']:.3e} against torch's {rep['norm_torch']:.3e}")
    if not (rep["finite"] and rep["norm_ok"] and rep["rows_ok"]):
        print(where)
    assert rep["finite"], f"not finite - {where}"
    assert rep["norm_ok"], f"whole-tensor rule - {where}"
    assert rep["rows_ok"], f"per-row rule - {where}"
    return rep


# ---------------------------------------------------------------------------------------------------------------------------
# dalm_lora2_*: per-element rules (tests/test_lora2_forms_gpu.py, tests/test_lora2_rules.py).  Every bound is the worst case of
# the arithmetic in dalm_amd/csrc/lora2.hip, in units of the float64 sum of magnitudes of the element's own terms - never a
# measurement.  EVERY element is compared; an element whose bound is zero (a dead row, an all-zero sum) must be exact.
# ---------------------------------------------------------------------------------------------------------------------------
U_F32 = 2.0 ** -24      # unit roundoff of f32, round to nearest
U_BF16 = 2.0 ** -8      # of bf16 (8 significant bits)


def unpack_bits(bits, C):
    """uint8 [R, C / 8] keep bits -> bool [R, C]: bit e of byte c = element 8 c + e (the layout dalm_lora2_rowdot writes)."""
    sh = torch.arange(8, device=bits.device, dtype=torch.int32)
    return ((bits.to(torch.int32).unsqueeze(-1) >> sh) & 1).bool().reshape(bits.shape[0], -1)[:, :C]


def _worst(err, bound, exact_bad):
    """max over ALL elements of err / bound (inf where an element that must be exact is not), and where."""
    ratio = torch.nan_to_num(err / bound.clamp_min(1e-300), nan=float("inf"))      # bound 0: 0 / tiny = 0, anything else huge
    ratio = ratio.masked_fill(exact_bad, float("inf"))
    flat = int(ratio.argmax())
    return {"ratio": float(ratio.flatten()[flat]), "at": [flat // ratio.shape[1], flat % ratio.shape[1]], "checked": ratio.numel()}


def lora2_rowdot_report(got, x, W, scale, keep=None, live=None):
    """z [R, rank] f32 = scale * (keep o x) W^T, x bf16 [R, K], W f32 [rank, K].  The kernel splits W into bf16 hi + bf16 lo (what is
    left of W is at most 2^-16 |W|) and accumulates in f32 (fewer than K roundings per element):
        |got - ref| <= (2^-16 + K 2^-24) |scale| sum_k |x_k| |W_k|          a dead row: exactly zero."""
    x64 = x.double()
    if keep is not None:
        x64 = x64 * keep
    if live is not None:
        x64 = x64 * (live != 0).unsqueeze(1)
    ref = scale * (x64 @ W.double().t())
    bound = (2.0 ** -16 + x.shape[1] * U_F32) * abs(scale) * (x64.abs() @ W.double().abs().t())
    assert got.shape == ref.shape and got.dtype == torch.float32
    return _worst((got.double() - ref).abs(), bound, torch.zeros_like(bound, dtype=torch.bool))


def lora2_rankupd_report(got, y, terms, scale, live=None):
    """y [R, C] bf16 += scale * sum_t keep_t o (z_t W_t);  terms: [(z [R, rank] f32, W [rank, C] f32, keep bool [R, C] or None)].
    Per term the kernel runs `rank` fmas and one fma onto y, all f32, then rounds ONCE to bf16:
        |got - ref| <= 2^-8 |ref| + (rank + 1 + terms) 2^-24 (|y| + |scale| sum_t keep_t sum_j |z_tj| |W_tj|)
    (one term: (rank + 2) 2^-24).  An element whose every keep bit is 0, and every element of a dead row, is y BIT FOR BIT."""
    y64 = y.double()
    upd, mag = torch.zeros_like(y64), torch.zeros_like(y64)
    touched = torch.zeros_like(y64, dtype=torch.bool)
    for z, W, keep in terms:
        t, a = z.double() @ W.double(), z.double().abs() @ W.double().abs()
        if keep is not None:
            t, a = t * keep, a * keep
        upd += t
        mag += a
        touched |= keep if keep is not None else torch.ones_like(touched)
    if live is not None:
        lv = (live != 0).unsqueeze(1)
        upd, mag, touched = upd * lv, mag * lv, touched & lv
    rank = terms[0][0].shape[1]
    ref = y64 + scale * upd
    bound = U_BF16 * ref.abs() + (rank + 1 + len(terms)) * U_F32 * (y64.abs() + abs(scale) * mag)
    assert got.shape == ref.shape and got.dtype == torch.bfloat16
    exact_bad = ~touched & (got.view(torch.int16) != y.view(torch.int16))
    return _worst((got.double() - ref).abs(), bound, exact_bad)


def lora2_colacc_report(got, x, z, scale, rows_per_split, keep=None, live=None):
    """out [rank, C] f32 = scale * sum_row keep o x[row, c] z[row, j], x bf16 [R, C], z f32 [R, rank].  The stated rule is
        |got - ref| <= R 2^-24 |scale| sum_row |x| |z|;
    the kernel's own depth is smaller: a thread adds every 32nd row of its split (rows_per_split / 32 fmas), then 3 adds over
    row lanes, 2 over waves, S over the splits and the multiplication with scale - depth = rows_per_split / 32 + S + 6 roundings.
    The smaller of the two is applied (for R < depth the first would not be a worst case: such shapes are not for this rule)."""
    R = x.shape[0]
    S = -(-R // rows_per_split)
    depth = -(-rows_per_split // 32) + S + 6
    assert R >= depth, "the rule is derived for R >= rows_per_split / 32 + S + 6"
    x64 = x.double()
    if keep is not None:
        x64 = x64 * keep
    if live is not None:
        x64 = x64 * (live != 0).unsqueeze(1)
    ref = scale * (z.double().t() @ x64)
    bound = min(R, depth) * U_F32 * abs(scale) * (z.double().abs().t() @ x64.abs())
    assert got.shape == ref.shape and got.dtype == torch.float32
    return _worst((got.double() - ref).abs(), bound, torch.zeros_like(bound, dtype=torch.bool))


def assert_lora2(name, rep):
    assert rep["ratio"] <= 1.0, f"{name}: error / bound = {rep['ratio']:.3e} at (row, column) = {tuple(rep['at'])}, {rep['checked']} elements checked"
    return rep["ratio"]


def synth_batch(seed, B, D, Tg, V, *, pad_side="right", dtype=torch.float32, logit_gain=1.0, full_mask=False):
    """Seeded synthetic (q, p, logits, ids, mask, qlen) as SURVEY section 8d describes."""
    g = torch.Generator().manual_seed(seed)
    q = torch.nn.functional.normalize(torch.randn(B, D, generator=g), dim=1)
    p = torch.nn.functional.normalize(torch.randn(B, D, generator=g), dim=1)
    logits = (logit_gain * torch.randn(B, Tg, V, generator=g)).to(dtype)
    ids = torch.randint(0, V, (B, Tg), generator=g)
    if full_mask:
        lens = torch.full((B,), Tg)
    else:
        lens = torch.randint(max(2, Tg // 4), Tg + 1, (B,), generator=g)
    ar = torch.arange(Tg).unsqueeze(0)
    mask = (ar < lens.unsqueeze(1)).long() if pad_side == "right" else (ar >= (Tg - lens).unsqueeze(1)).long()
    qlen = torch.clamp((lens.float() * 0.8).floor().long(), min=1)
    return q, p, logits, ids, mask, qlen
