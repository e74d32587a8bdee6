"""Attention backward at the cfg3 layer shape (B 18, H 32, T 256, hd 128, HF causal + left-padding mask): `dalm_attn_bwd`
against torch's memory-efficient backward, hipGraph replay timing.  -> stdout (profiles/r05_attn_bwd.txt)

--kv-heads N (grouped-query attention, N < H key / value heads): `dalm_attn_gqa_*` on the un-expanded k / v against the EXPANDED
path - repeat_kv copies + the equal-heads kernels + autograd's sum of the per-head dk / dv - forward and backward, padded (causal +
left padding) and packed layouts, alternated in one process.  -> stdout (profiles/attn_gqa_bench.txt)

--encoder (a BERT-class retriever layer: bidirectional mask with RIGHT padding, sequence lengths uniform in --len-range, optional
--dropout p): `dalm_attn_fwd` / `dalm_attn_bwd` against torch's SDPA on the same tensors and mask (what a model on "sdpa" runs),
and the packed forms (`dalm_attn_*_packed` on the live rows) against `_packed_sdpa_torch` (re-pad, torch's SDPA, gather).  The two
paths alternate --rounds times in one process; every figure is the median over rounds x 20 separately timed hipGraph replays
(HIP events, --iters calls per graph, after warm-up replays).  -> stdout (profiles/attn_hd32_bench.txt, with --hd 32)

--encoder --hd 64 --rel-bias (an MPNet layer: a per-head relative-position bias by column difference): the bias kernels
(`dalm_attn_rel_*`) beside the bias-free kernels on the same tensors (their ratio is the cost of the bias), beside torch's SDPA
with bias + key mask as a float mask, beside the eager MPNet chain (matmul, scale, += bias, + mask, softmax, dropout, matmul;
padded layout only); all paths alternate in one process.  -> stdout (profiles/attn_rel_bench.txt)"""
import argparse
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from dalm_amd.models import attention  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=18)
ap.add_argument("--H", type=int, default=32)
ap.add_argument("--T", type=int, default=256)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--lens", default="random", help="random (T/2..T) | full | <n> (every sequence n tokens, left-padded)")
ap.add_argument("--hd", type=int, default=128, choices=(32, 64, 128))
ap.add_argument("--kv-heads", type=int, default=0, help="grouped-query heads: time dalm_attn_gqa_* against the expanded path")
ap.add_argument("--rounds", type=int, default=3, help="--kv-heads: alternations of the two paths (median, min .. max reported)")
ap.add_argument("--encoder", action="store_true", help="encoder layer: bidirectional right-padding mask, padded and packed forms")
ap.add_argument("--len-range", default="", help="--encoder: LO,HI - sequence lengths uniform in [LO, HI] (default T/2,T)")
ap.add_argument("--dropout", type=float, default=0.0, help="--encoder: attention dropout probability (in-kernel / torch's own)")
ap.add_argument("--rel-bias", action="store_true", help="--encoder --hd 64: dalm_attn_rel_* beside the bias-free kernels, torch, eager")
a = ap.parse_args()
dev = torch.device("cuda:0")
B, H, T, hd = a.B, a.H, a.T, a.hd
g = torch.Generator().manual_seed(0)
q, k, v, go = [torch.randn(B, T, H, hd, generator=g).bfloat16().to(dev).transpose(1, 2) for _ in range(4)]
lens = torch.randint(T // 2, T + 1, (B,), generator=g)
lens[0] = T
if a.lens == "full":
    lens[:] = T
elif a.lens != "random":
    lens[:] = int(a.lens)
col = torch.arange(T, device=dev)
st = (T - lens).to(dev)
mask = ((col[None, None, :] <= col[None, :, None]) & (col[None, None, :] >= st[:, None, None]))[:, None]
scale = hd ** -0.5
live_frac = float(mask.float().mean())


def timed(fn, label, flops, qkv=None, reps=5, quiet=False, d_out=None):
    qq, kk, vv = [t.detach().clone().requires_grad_(True) for t in (qkv or (q, k, v))]
    gg = go if d_out is None else d_out
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):                       # forward on the capture stream: autograd replays the backward on it
        o = fn(qq, kk, vv)
        for _ in range(3):
            torch.autograd.grad(o, (qq, kk, vv), gg, retain_graph=True)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            for _ in range(a.iters):
                torch.autograd.grad(o, (qq, kk, vv), gg, retain_graph=True)
    gr.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        gr.replay()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / (reps * a.iters)
    if not quiet:
        print(f"{label:48s} {us:8.1f} us   {flops / us / 1e6:7.1f} TFLOP/s on the live tiles' 5 products")
    return us


def timed_fwd(fn, label, flops, qkv=None, reps=5, quiet=False, d_out=None):
    qq, kk, vv = [t.detach().clone().requires_grad_(True) for t in (qkv or (q, k, v))]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for _ in range(3):
            fn(qq, kk, vv)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            for _ in range(a.iters):
                fn(qq, kk, vv)
    gr.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        gr.replay()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / (reps * a.iters)
    if not quiet:
        print(f"{label:48s} {us:8.1f} us   {flops / us / 1e6:7.1f} TFLOP/s on the live tiles' 2 products")
    return us


def grouped_bench(Hkv):
    """Grouped against expanded, same inputs, alternated `--rounds` times; one line per (layout, pass): medians, spread, ratio."""
    from transformers.integrations.sdpa_attention import repeat_kv

    from dalm_amd import packed

    G = H // Hkv
    assert 1 < Hkv < H and H % Hkv == 0, "--kv-heads must divide --H, 1 < N < H"
    el = 2
    print(f"# grouped-query attention: B {B} H {H} Hkv {Hkv} (G {G}) T {T} hd {hd}; live fraction of the mask {live_frac:.3f}")
    print(f"# algorithmic bytes: forward (2 + 2/G) B H T hd el = {(2 + 2 / G) * B * H * T * hd * el / 1e6:.0f} MB, "
          f"backward (5 + 3/G) B H T hd el = {(5 + 3 / G) * B * H * T * hd * el / 1e6:.0f} MB (padded layout, padding included)")
    reps = 20
    print(f"# each figure: {a.iters} calls per hipGraph x {reps} replays, median of {a.rounds} alternations (min .. max) in us per call")
    am = (col[None, :] >= st[:, None]).long()
    rows, cu = packed.pack_plan(am, shifted=True, multiple=256)
    _ids, _pos, desc, _valid = packed.packed_inputs(torch.zeros(B, T, dtype=torch.long, device=dev), am, rows.to(dev), cu.to(dev), True)
    n = rows.numel()
    layouts = {
        "padded": ([torch.randn(B, T, h_, hd, generator=g).bfloat16().to(dev).transpose(1, 2) for h_ in (H, Hkv, Hkv)], mask),
        "packed": ([torch.randn(1, n, h_, hd, generator=g).bfloat16().to(dev).transpose(1, 2) for h_ in (H, Hkv, Hkv)], desc),
    }
    from dalm_amd import hip

    results = {}
    for name, (qkv, m) in layouts.items():
        nseq = B if name == "padded" else packed.packed_of(desc).nseq
        chosen = int(hip.load().dalm_attn_gqa_bwd_splits(nseq, H, Hkv, T))
        forms = sorted({chosen, 1} | ({2} if G % 2 == 0 and chosen > 1 else set()))      # dk / dv forms shown for the backward
        d_out = torch.randn(qkv[0].shape[0], qkv[0].shape[2], H, hd, generator=g).bfloat16().to(dev).transpose(1, 2)
        fns = {"grouped": lambda x, y, z, m=m: attention._SdpaHipBackward.apply(x, y, z, m, scale, False),
               "expanded": lambda x, y, z, m=m: attention._SdpaHipBackward.apply(x, repeat_kv(y, G), repeat_kv(z, G), m, scale, False)}
        assert attention.grouped_supported(qkv[0].detach().requires_grad_(True), qkv[1], qkv[2], m if name == "padded" else None,
                                           packed=name == "packed")
        for pas, timer in (("forward", timed_fwd), ("backward", timed)):
            others = [S for S in forms if S != chosen] if pas == "backward" else []
            t = {"grouped": [], "expanded": [], **{S: [] for S in others}}
            for _ in range(a.rounds):
                for which in ("grouped", "expanded", *others):
                    attention._gqa_splits[0] = which if isinstance(which, int) else 0
                    t[which].append(timer(fns["grouped" if isinstance(which, int) else which], "", 1.0, qkv=qkv, reps=reps, quiet=True,
                                          d_out=d_out))
            attention._gqa_splits[0] = 0
            med = {w: sorted(x)[len(x) // 2] for w, x in t.items()}
            results[(name, pas)] = med
            print(f"{name:7s} {pas:8s} rows {qkv[0].shape[0] * qkv[0].shape[2]:6d}   grouped {med['grouped']:7.1f} ({min(t['grouped']):.1f} .. "
                  f"{max(t['grouped']):.1f})   expanded {med['expanded']:7.1f} ({min(t['expanded']):.1f} .. {max(t['expanded']):.1f})   "
                  f"expanded / grouped {med['expanded'] / med['grouped']:.2f}x")
            if pas == "backward":
                print(f"#   dk / dv form of the grouped figure: {chosen} workgroup(s) per (key block, KV head) - the library's choice for this grid"
                      + "".join(f"; forced {S}: {med[S]:.1f} ({min(t[S]):.1f} .. {max(t[S]):.1f})" for S in others))
    return results


def replay_samples(fn, qkv, d_out, backward, reps=20):
    """`--iters` calls of `fn` (its forward, or the backward of one forward) captured into one hipGraph; 3 warm-up replays, then
    `reps` replays timed one by one with HIP events: us per call of each."""
    qq, kk, vv = [t.detach().clone().requires_grad_(True) for t in qkv]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        o = fn(qq, kk, vv)
        for _ in range(3):
            if backward:
                torch.autograd.grad(o, (qq, kk, vv), d_out, retain_graph=True)
            else:
                fn(qq, kk, vv)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            for _ in range(a.iters):
                if backward:
                    torch.autograd.grad(o, (qq, kk, vv), d_out, retain_graph=True)
                else:
                    fn(qq, kk, vv)
    for _ in range(3):
        gr.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        gr.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / a.iters)
    return out


def encoder_bench():
    from dalm_amd import packed

    p = a.dropout
    lo, hi = [int(x) for x in a.len_range.split(",")] if a.len_range else (T // 2, T)
    ln = torch.randint(lo, hi + 1, (B,), generator=g)
    am = (torch.arange(T)[None, :] < ln[:, None]).long()
    m4 = am.bool().to(dev)[:, None, None, :].expand(B, 1, T, T)                      # HF's bidirectional padding mask
    rows, cu = packed.pack_plan(am, shifted=False, multiple=packed.PACK_MULTIPLE)
    _ids, _pos, desc, _valid = packed.packed_inputs(torch.zeros(B, T, dtype=torch.long, device=dev), am.to(dev), rows.to(dev), cu.to(dev), False)
    seqs = packed.packed_of(desc)
    n = rows.numel()
    pad_qkv = (q, k, v)
    pk_qkv = [torch.randn(1, n, H, hd, generator=g).bfloat16().to(dev).transpose(1, 2) for _ in range(3)]
    pk_go = torch.randn(1, n, H, hd, generator=g).bfloat16().to(dev).transpose(1, 2)
    assert attention.supported(q.detach().requires_grad_(True), k, v, m4, p, False, {}), "the padded kernels do not take this call"
    assert attention.packed_supported(*pk_qkv, p), "the packed kernels do not take this call"
    F = torch.nn.functional
    paths = {
        "padded": (pad_qkv, go, {"kernels": lambda x, y, z: attention.sdpa(x, y, z, m4, scale, False, p, 7),
                                 "torch": lambda x, y, z: F.scaled_dot_product_attention(x, y, z, attn_mask=m4, dropout_p=p, scale=scale)}),
        "packed": (pk_qkv, pk_go, {"kernels": lambda x, y, z: attention.sdpa(x, y, z, desc, scale, False, p, 7),
                                   "torch": lambda x, y, z: attention._packed_sdpa_torch(x, y, z, seqs, scale, p).transpose(1, 2)}),
    }
    if a.rel_bias:
        assert hd == 64, "--rel-bias: head width 64"
        rel = (torch.randn(H, 2 * T - 1, generator=g) * 0.5).to(dev)
        cols = packed.packed_positions(torch.zeros(B, T, dtype=torch.long, device=dev), rows.to(dev), None).to(torch.int32)
        fm = (attention.expand_rel_bias(rel, torch.arange(T, device=dev))[None]
              + torch.zeros(B, 1, T, T, device=dev).masked_fill(~m4, torch.finfo(torch.float32).min)).to(torch.bfloat16)

        def eager(x, y, z):
            s = torch.matmul(x, y.transpose(-1, -2)) / (hd ** 0.5)
            s += fm
            return torch.matmul(F.dropout(F.softmax(s, dim=-1), p), z)

        assert attention.rel_supported(q, k, v, rel, m4, p) and attention.rel_supported(*pk_qkv, rel, desc, p)
        paths["padded"][2].update({
            "rel": lambda x, y, z: attention._RelSdpaHip.apply(x, y, z, rel, m4, scale, p, 7),
            "torch": lambda x, y, z: F.scaled_dot_product_attention(x, y, z, attn_mask=fm, dropout_p=p, scale=scale),
            "eager": eager})
        paths["packed"][2].update({
            "rel": lambda x, y, z: attention._RelSdpaHip.apply(x, y, z, rel, desc, scale, p, 7, cols),
            "torch": lambda x, y, z: attention._rel_sdpa_torch(x, y, z, rel, None, seqs, scale, p)})
        print(f"# relative-position bias: B {B} H {H} T {T} hd {hd} dropout {p}; lengths U[{lo}, {hi}]: {int(ln.sum())} live tokens of "
              f"{B * T}, {n} packed rows; median of {a.rounds} x 20 hipGraph replays ({a.iters} calls each) in us per call; "
              "rel = dalm_attn_rel_*, kernels = the bias-free dalm_attn_* on the same tensors, torch = SDPA with bias + mask as a float "
              "mask, eager = MPNet's statement chain")
        for layout, (qkv, d_out, fns) in paths.items():
            t = {(w, pas): [] for w in fns for pas in ("fwd", "bwd")}
            for _ in range(a.rounds):
                for pas in ("fwd", "bwd"):
                    for w, fn in fns.items():                                        # all paths alternate
                        t[(w, pas)] += replay_samples(fn, qkv, d_out, pas == "bwd")
            med = {key: sorted(x)[len(x) // 2] for key, x in t.items()}
            tot = {w: med[(w, "fwd")] + med[(w, "bwd")] for w in fns}
            print(f"rel-bias B {B:3d} T {T:3d} p {p:.1f} {layout:6s}  "
                  + "  ".join(f"{w} fwd {med[(w, 'fwd')]:6.1f} bwd {med[(w, 'bwd')]:6.1f} sum {tot[w]:6.1f}" for w in fns)
                  + f"  |  rel / kernels {tot['rel'] / tot['kernels']:.3f}  torch / rel {tot['torch'] / tot['rel']:.2f}x"
                  + (f"  eager / rel {tot['eager'] / tot['rel']:.2f}x" if "eager" in tot else ""))
        return
    print(f"# encoder layer: B {B} H {H} T {T} hd {hd} dropout {p}; lengths U[{lo}, {hi}]: {int(ln.sum())} live tokens of {B * T}, "
          f"{n} packed rows; median of {a.rounds} x 20 hipGraph replays ({a.iters} calls each) in us per call (min .. max)")
    for layout, (qkv, d_out, fns) in paths.items():
        t = {(w, pas): [] for w in fns for pas in ("fwd", "bwd")}
        for _ in range(a.rounds):
            for pas in ("fwd", "bwd"):
                for w, fn in fns.items():                                            # the two paths alternate
                    t[(w, pas)] += replay_samples(fn, qkv, d_out, pas == "bwd")
        med = {key: sorted(x)[len(x) // 2] for key, x in t.items()}
        tot = {w: med[(w, "fwd")] + med[(w, "bwd")] for w in fns}
        print(f"hd {hd} B {B:3d} T {T:3d} p {p:.1f} {layout:6s}  "
              + "  ".join(f"{pas} kernels {med[('kernels', pas)]:6.1f} ({min(t[('kernels', pas)]):.1f} .. {max(t[('kernels', pas)]):.1f}) "
                          f"torch {med[('torch', pas)]:6.1f} ({min(t[('torch', pas)]):.1f} .. {max(t[('torch', pas)]):.1f})"
                          for pas in ("fwd", "bwd"))
              + f"  fwd+bwd kernels {tot['kernels']:6.1f} torch {tot['torch']:6.1f}  torch / kernels {tot['torch'] / tot['kernels']:.2f}x")


if a.kv_heads:
    grouped_bench(a.kv_heads)
    sys.exit(0)
if a.encoder:
    encoder_bench()
    sys.exit(0)


flops = 5 * 2.0 * B * H * T * T * hd * live_frac
print(f"# B {B} H {H} T {T} hd {hd}; live fraction of the mask {live_frac:.3f}; algorithmic bytes {8 * B * H * T * hd * 2 / 1e6:.0f} MB")
t_ours = timed(lambda x, y, z: attention._SdpaHipBackward.apply(x, y, z, mask, scale, False), "dalm_attn_bwd (2 launches)", flops)
t_torch = timed(lambda x, y, z: torch.nn.functional.scaled_dot_product_attention(x, y, z, attn_mask=mask, scale=scale),
                "torch memory-efficient backward (3 launches)", flops)
print(f"# ratio {t_torch / t_ours:.2f}x")
f_ours = timed_fwd(lambda x, y, z: attention._SdpaHipBackward.apply(x, y, z, mask, scale, False), "dalm_attn_fwd (+ mask bits, cached)", flops * 0.4)
f_torch = timed_fwd(lambda x, y, z: torch.nn.functional.scaled_dot_product_attention(x, y, z, attn_mask=mask, scale=scale),
                    "torch memory-efficient forward", flops * 0.4)
print(f"# forward ratio {f_torch / f_ours:.2f}x")
