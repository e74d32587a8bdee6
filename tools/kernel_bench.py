"""Per-kernel timings (HIP events on the launch stream) against the gfx950 rooflines.

    python tools/kernel_bench.py [--quick]

Algorithmic bytes / flops follow SURVEY.md section 8(d): dense definitions (all rows counted).
HBM peak 8 TB/s (spec; ~6.3 TB/s achievable), f32 MFMA peak 157.3 TFLOP/s.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from dalm_amd.ops import default_ops  # noqa: E402

HBM_PEAK = 8.0e12
MFMA_F32_PEAK = 157.3e12


def time_fn(fn, iters=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) * 1e-3 for a, b in evs)
    return ts[len(ts) // 2], ts[0]


def time_graph(fn, reps=20, replays=10):
    """GPU-side time per call for latency-bound ops: `reps` calls captured in one hipGraph, replayed; the host
    (python + ctypes + allocator, ~10 us per launch) is out of the measurement.  Returns (median, best) seconds."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
        with torch.cuda.graph(g, stream=s):
            for _ in range(reps):
                fn()
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(replays):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3 / reps)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def bench_ce(B, Tg, V, dtype, full_mask=True):
    ops = default_ops()
    dev = torch.device("cuda:0")
    logits = torch.randn(B, Tg, V, device=dev, dtype=dtype)
    ids = torch.randint(0, V, (B, Tg), device=dev)
    if full_mask:
        mask = torch.ones(B, Tg, dtype=torch.int64, device=dev)
    else:
        lens = torch.randint(60, Tg + 1, (B,), device=dev)
        mask = (torch.arange(Tg, device=dev).unsqueeze(0) < lens.unsqueeze(1)).long()
    qlen = torch.full((B,), int(0.8 * Tg), device=dev)
    stats, Nb, Mb = ops.ce_prep(mask, qlen)
    el = logits.element_size()
    R = B * (Tg - 1)
    out = {}
    med, best = time_fn(lambda: ops.ce_fwd(logits, ids, mask, stats, False))
    out["fwd"] = {"s": med, "best_s": best, "GBps": R * V * el / med / 1e9, "frac": R * V * el / med / HBM_PEAK}
    buf = torch.empty_like(logits)
    med, best = time_fn(lambda: ops.ce_fwd(logits, ids, mask, stats, True))
    out["fwd+grad(fused)"] = {"s": med, "best_s": best, "GBps": 2 * R * V * el / med / 1e9, "frac": 2 * R * V * el / med / HBM_PEAK}
    # what the training step runs: the gradient overwrites the logits (footprint = one buffer, not two)
    scratch = logits.clone()
    med, best = time_fn(lambda: ops.ce_fwd(scratch, ids, mask, stats, True, inplace=True))
    out["fwd+grad(in place)"] = {"s": med, "best_s": best, "GBps": 2 * R * V * el / med / 1e9, "frac": 2 * R * V * el / med / HBM_PEAK}
    del scratch
    row_lse, _, _ = ops.ce_fwd(logits, ids, mask, stats, False)
    g = torch.ones(1, device=dev)
    med, best = time_fn(lambda: ops.ce_bwd(logits, ids, mask, stats, row_lse, g))
    out["bwd(separate)"] = {"s": med, "best_s": best, "GBps": 2 * R * V * el / med / 1e9, "frac": 2 * R * V * el / med / HBM_PEAK}
    # a plain device copy of the same bytes, for calibration of the achievable ceiling
    med, best = time_fn(lambda: buf.copy_(logits))
    out["torch_copy(ref)"] = {"s": med, "GBps": 2 * B * Tg * V * el / med / 1e9}
    return out


def bench_sim(m, n, D):
    ops = default_ops()
    dev = torch.device("cuda:0")
    A = torch.nn.functional.normalize(torch.randn(m, D, device=dev), dim=1)
    Bm = torch.nn.functional.normalize(torch.randn(n, D, device=dev), dim=1)
    out = {}
    # mid sizes are a handful of launches of tens of microseconds: besides the eager number (HIP events around each call,
    # comparable with earlier rounds) report the GPU time of the call inside a hipGraph - how the training step runs it
    graphed = 256 * 256 <= m * n <= 4096 * 4096
    med, best = time_fn(lambda: ops.sim_rowstats(A, Bm, 100.0, 0), iters=10, warmup=3)
    # the default entry point routes m, n >= 3072 to the bf16x3 form (6 x the flops on the bf16 pipe): its roofline fraction is
    # the flops ACTUALLY ISSUED over the bf16 peak - never an f32-equivalent rate over the f32 peak (that read 1.19 / 1.40 in
    # profiles/history/r04_kernel_bench.txt)
    on_bf16 = m >= 3072 and n >= 3072 and D % 64 == 0
    flops = (12.0 if on_bf16 else 2.0) * m * n * D
    peak = 2.5e15 if on_bf16 else MFMA_F32_PEAK
    out["rowstats"] = {"s": med, "TFLOPs_f32_equivalent": 2.0 * m * n * D / med / 1e12, "pipe": "bf16 x3" if on_bf16 else "f32",
                       "TFLOPs_issued": flops / med / 1e12, "frac": flops / med / peak}
    if graphed:
        gm, _ = time_graph(lambda: ops.sim_rowstats(A, Bm, 100.0, 0), reps=10, replays=7)
        out["rowstats"].update({"graph_s": gm, "graph_frac": flops / gm / peak})
    if m >= 1024 and n >= 1024:
        # round 4: the same statistics on the bf16 matrix cores (three bf16 thirds per operand, 6 D deep); "TFLOPs" stays the
        # f32-EQUIVALENT rate 2 m n D / t (the kernel executes 6 x that on the bf16 pipe); sim_rowstats itself routes
        # m, n >= 4096 there, so the exact-f32 kernel is timed through its pinned entry point
        med, _ = time_fn(lambda: ops.sim_rowstats_bf16x3(A, Bm, 100.0, 0), iters=10, warmup=3)
        # priced on the flops ISSUED against the bf16 peak only: an f32-equivalent rate over the f32 peak reads above 1 here
        # (1.21 / 1.43 in earlier files) and says nothing about the kernel
        out["rowstats_bf16x3"] = {"s": med, "TFLOPs_f32_equivalent": 2.0 * m * n * D / med / 1e12, "pipe": "bf16 x3",
                                  "TFLOPs_issued": 12.0 * m * n * D / med / 1e12, "frac": 12.0 * m * n * D / med / 2.5e15}
        med, _ = time_fn(lambda: ops.sim_rowstats_f32(A, Bm, 100.0, 0), iters=10, warmup=3)
        out["rowstats_f32"] = {"s": med, "TFLOPs": 2.0 * m * n * D / med / 1e12, "frac": 2.0 * m * n * D / med / MFMA_F32_PEAK}
    if m * n <= 20000 * 20000:
        rl, _ = ops.sim_rowstats(A, Bm, 100.0, 0)
        cl = torch.zeros(n, device=dev) + 5.0
        rc = torch.full((m,), 1.0 / m, device=dev)
        cc = torch.full((n,), 1.0 / n, device=dev)
        med, best = time_fn(lambda: ops.sim_grad(A, Bm, 100.0, 0, rc, rl, cc, cl), iters=10, warmup=3)
        # sim_grad routes m, n >= 8192 to the bf16x3 form (HipOps.sim_grad): 6 x the flops on the bf16 pipe - priced against
        # the bf16 peak on the flops ISSUED, as the forward above (an f32-equivalent rate over the f32 peak reads > 1 there)
        import os

        g_x3 = os.environ.get("DALM_SIM_GRAD_X3") != "0" and m >= 8192 and n >= 8192 and D % 64 == 0
        g_fl = (24.0 if g_x3 else 4.0) * m * n * D
        g_peak = 2.5e15 if g_x3 else MFMA_F32_PEAK
        out["grad"] = {"s": med, "TFLOPs_f32_equivalent": 4.0 * m * n * D / med / 1e12, "pipe": "bf16 x3" if g_x3 else "f32",
                       "TFLOPs_issued": g_fl / med / 1e12, "frac": g_fl / med / g_peak}
        if graphed:
            gm, _ = time_graph(lambda: ops.sim_grad(A, Bm, 100.0, 0, rc, rl, cc, cl), reps=10, replays=7)
            out["grad"].update({"graph_s": gm, "graph_frac": g_fl / gm / g_peak})
    return out


def bench_small(m, n, D, want_cols=True):
    """Small-batch contrastive path: S once (2 launches), backward 1 launch; latency-bound, reported in us."""
    ops = default_ops()
    dev = torch.device("cuda:0")
    A = torch.nn.functional.normalize(torch.randn(m, D, device=dev), dim=1)
    Bm = torch.nn.functional.normalize(torch.randn(n, D, device=dev), dim=1)
    out = {}
    med, best = time_graph(lambda: ops.sim_small_fwd(A, Bm, 100.0, 0, want_cols, one_launch=False))
    out["fwd(partial+stats)"] = {"us": med * 1e6, "best_us": best * 1e6, "TFLOPs": 2.0 * m * n * D / med / 1e12}
    ops.sim_small_fwd(A, Bm, 100.0, 0, want_cols, one_launch=True)        # tickets allocated outside the capture
    med, best = time_graph(lambda: ops.sim_small_fwd(A, Bm, 100.0, 0, want_cols, one_launch=True))
    out["fwd(one launch)"] = {"us": med * 1e6, "best_us": best * 1e6, "TFLOPs": 2.0 * m * n * D / med / 1e12}
    S, rl, _, cl = ops.sim_small_fwd(A, Bm, 100.0, 0, True)
    rc = torch.full((m,), 1.0 / m, device=dev)
    cc = torch.full((n,), 1.0 / n, device=dev)
    med, best = time_graph(lambda: ops.sim_small_bwd(S, A, Bm, 100.0, 0, rc, rl, cc, cl, True, want_cols, one_launch=False))
    nd = 2 if want_cols else 1
    out["bwd(dQ,dP)" if want_cols else "bwd(dQ)"] = {"us": med * 1e6, "best_us": best * 1e6,
                                                      "TFLOPs": nd * 2.0 * m * n * D / med / 1e12}
    if not want_cols:       # one direction of a long contraction: the slices summed inside the launch (round 4)
        ops.sim_small_bwd(S, A, Bm, 100.0, 0, rc, rl, cc, cl, True, False, one_launch=True)
        med, best = time_graph(lambda: ops.sim_small_bwd(S, A, Bm, 100.0, 0, rc, rl, cc, cl, True, False, one_launch=True))
        out["bwd(dQ, one launch)"] = {"us": med * 1e6, "best_us": best * 1e6, "TFLOPs": 2.0 * m * n * D / med / 1e12}
    return out


def bench_pool(B, T, D, dtype):
    ops = default_ops()
    dev = torch.device("cuda:0")
    h = torch.randn(B, T, D, device=dev, dtype=dtype)
    mask = torch.ones(B, T, dtype=torch.int64, device=dev)
    el = h.element_size()
    out = {}
    timer = time_graph if B * T * D * el < (256 << 20) else time_fn   # small shapes are host-bound when launched eagerly
    med, _ = timer(lambda: ops.pool_fwd(h, mask, True))
    out["fwd"] = {"s": med, "GBps": B * T * D * el / med / 1e9, "frac": B * T * D * el / med / HBM_PEAK}
    emb, norm, ic = ops.pool_fwd(h, mask, True)
    de = torch.randn_like(emb)
    med, _ = timer(lambda: ops.pool_bwd(de, emb, norm, ic, mask, True, T, dtype))
    out["bwd"] = {"s": med, "GBps": B * T * D * el / med / 1e9, "frac": B * T * D * el / med / HBM_PEAK}
    return out


def bench_nf4(rows, cols, dtype):
    """`use_bnb` storage: dequantise one [rows, cols] weight (Llama-2-7b's largest Linear is 11008 x 4096)."""
    from dalm_amd.models import nf4

    dev = torch.device("cuda:0")
    w = (torch.randn(rows, cols, device=dev) * 0.02).to(dtype)
    n = rows * cols
    el = w.element_size()
    out = {}
    med, _ = time_fn(lambda: nf4.quantize(w))
    b = n * el + n / 2 + n / 16
    out["quantize"] = {"s": med, "GBps": b / med / 1e9, "frac": b / med / HBM_PEAK}
    p, a = nf4.quantize(w)
    med, _ = time_fn(lambda: nf4.dequantize(p, a, (rows, cols), dtype))
    out["dequantize"] = {"s": med, "GBps": b / med / 1e9, "frac": b / med / HBM_PEAK}
    # as the step runs it: inside a hipGraph (no host time), a DIFFERENT weight every call (8 layers' worth, so the packed
    # input of a call was not just read by the previous one)
    ws = [nf4.quantize((torch.randn(rows, cols, device=dev) * 0.02).to(dtype)) for _ in range(8)]

    def sweep():
        for pk, am in ws:
            nf4.dequantize(pk, am, (rows, cols), dtype)

    med, _ = time_graph(sweep, reps=4)
    med /= len(ws)
    out["dequantize (graph, 8 weights in turn)"] = {"s": med, "GBps": b / med / 1e9, "frac": b / med / HBM_PEAK}
    return out


def bench_tower(B, T, H, hd, inter, dtype):
    """The two elementwise chains of a Llama-family generator layer: dalm_rope_qk / dalm_swiglu_* against the eager chains
    they replace (transformers' apply_rotary_pos_emb as the step ran it before - roll + addcmul - and silu(gate) * up)."""
    from dalm_amd.models import fastpath, tower_ops

    dev = torch.device("cuda:0")
    el = torch.empty((), dtype=dtype).element_size()
    q = torch.randn(B, T, H * hd, device=dev, dtype=dtype).view(B, T, H, hd).transpose(1, 2)
    k = torch.randn(B, T, H * hd, device=dev, dtype=dtype).view(B, T, H, hd).transpose(1, 2)
    cos, sin = torch.rand(B, T, hd, device=dev, dtype=dtype), torch.rand(B, T, hd, device=dev, dtype=dtype)
    out = {}
    b = 4 * q.numel() * el + 2 * cos.numel() * el
    med, _ = time_graph(lambda: tower_ops._rope_launch(q, k, cos, sin, False))
    out["rope fwd (1 launch)"] = {"s": med, "GBps": b / med / 1e9, "frac": b / med / HBM_PEAK}
    med, _ = time_graph(lambda: tower_ops._rope_launch(q, k, cos, sin, True))
    out["rope bwd (1 launch)"] = {"s": med, "GBps": b / med / 1e9, "frac": b / med / HBM_PEAK}
    med, _ = time_graph(lambda: fastpath._rope_roll(q, k, cos, sin))
    out["rope fwd eager (roll+addcmul)"] = {"s": med, "GBps": b / med / 1e9, "frac": b / med / HBM_PEAK}
    n = B * T * inter
    gate, up, da = (torch.randn(B * T, inter, device=dev, dtype=dtype) for _ in range(3))
    act, dg, du = torch.empty_like(gate), torch.empty_like(gate), torch.empty_like(gate)
    from dalm_amd import hip

    code = hip.dtype_code(gate)
    med, _ = time_graph(lambda: hip.call("dalm_swiglu_fwd", hip.ptr(gate), hip.ptr(up), hip.ptr(act), code, n, hip.stream()))
    out["swiglu fwd (1 launch)"] = {"s": med, "GBps": 3 * n * el / med / 1e9, "frac": 3 * n * el / med / HBM_PEAK}
    med, _ = time_graph(lambda: hip.call("dalm_swiglu_bwd", hip.ptr(da), hip.ptr(gate), hip.ptr(up), hip.ptr(dg), hip.ptr(du),
                                         code, n, hip.stream()))
    out["swiglu bwd (1 launch)"] = {"s": med, "GBps": 5 * n * el / med / 1e9, "frac": 5 * n * el / med / HBM_PEAK}
    med, _ = time_graph(lambda: torch.nn.functional.silu(gate) * up)
    out["swiglu fwd eager (2 launches)"] = {"s": med, "GBps": 3 * n * el / med / 1e9, "frac": 3 * n * el / med / HBM_PEAK}
    # the same on the two halves of ONE [rows, 2 C] GEMM output (gate | up as one forward GEMM, models/frozen_linear.py)
    R, Cc = B * T, inter
    both = torch.randn(R, 2 * Cc, device=dev, dtype=dtype)
    g2, u2 = both[:, :Cc], both[:, Cc:]
    med, _ = time_graph(lambda: hip.call("dalm_swiglu_fwd_2d", hip.ptr(g2), hip.ptr(u2), hip.ptr(act), code, R, Cc, 2 * Cc, 2 * Cc, Cc,
                                         hip.stream()))
    out["swiglu fwd, halves of one buffer"] = {"s": med, "GBps": 3 * n * el / med / 1e9, "frac": 3 * n * el / med / HBM_PEAK}
    med, _ = time_graph(lambda: hip.call("dalm_swiglu_bwd_2d", hip.ptr(da), hip.ptr(g2), hip.ptr(u2), hip.ptr(dg), hip.ptr(du), code,
                                         R, Cc, Cc, 2 * Cc, 2 * Cc, Cc, Cc, hip.stream()))
    out["swiglu bwd, halves of one buffer"] = {"s": med, "GBps": 5 * n * el / med / 1e9, "frac": 5 * n * el / med / HBM_PEAK}
    return out


def bench_pool_last(B, T, D, dtype):
    """Last-token pooling from packed rows next to the padded pool's backward on the same batch: B sequences of T rows
    (n = B T), and the one-token mask of `eos_mask` for `dalm_pool_l2norm_bwd`.  Bytes the kernel has to move: forward reads
    nseq x D elements and writes nseq x D f32, backward writes n x D elements."""
    ops = default_ops()
    dev = torch.device("cuda:0")
    n, el = B * T, torch.empty((), dtype=dtype).element_size()
    h = torch.randn(n, D, device=dev, dtype=dtype)
    cu = torch.arange(0, n + 1, T, dtype=torch.int32, device=dev)
    out = {}
    med, _ = time_graph(lambda: ops.pool_last_packed_fwd(h, cu, B, True))
    by = B * D * (el + 4)
    out["last fwd"] = {"s": med, "GBps": by / med / 1e9, "frac": by / med / HBM_PEAK}
    emb, norm = ops.pool_last_packed_fwd(h, cu, B, True)
    de = torch.randn_like(emb)
    med, _ = time_graph(lambda: ops.pool_last_packed_bwd(de, emb, norm, cu, n, True, dtype))
    out["last bwd"] = {"s": med, "GBps": n * D * el / med / 1e9, "frac": n * D * el / med / HBM_PEAK}
    mask = torch.zeros(B, T, dtype=torch.int64, device=dev)
    mask[:, -1] = 1
    e2, n2, ic = ops.pool_fwd(h.view(B, T, D), mask, True)
    med, _ = time_graph(lambda: ops.pool_bwd(de, e2, n2, ic, mask, True, T, dtype))
    out["l2norm bwd"] = {"s": med, "GBps": n * D * el / med / 1e9, "frac": n * D * el / med / HBM_PEAK}
    return out


def bench_head_norm_rope(B, T, Hq, Hk, hd, rounds=3):
    """Qwen3's q_norm / k_norm + rotary embedding: `dalm_head_norm_rope_fwd` / `dalm_head_norm_bwd` on the q | k column slices of
    one [B T, (Hq + 2 Hk) hd] bf16 buffer, and beside them - alternating, in the same process - what runs without them for the
    same math: F.rms_norm x 2 (what `use_native_rms_norm` leaves of Qwen3RMSNorm) + transformers' eager rotary chain, and
    autograd's backward of that.  Algorithmic bytes: forward reads q, k and writes q, k and rstd; backward reads the gradients
    and q, k, rstd and writes dq, dk.  Every figure: median over `rounds` alternations of a 20-call graph's per-call time,
    with the lowest and highest round."""
    import torch.nn.functional as F
    from transformers.models.qwen3.modeling_qwen3 import apply_rotary_pos_emb

    from dalm_amd.models import tower_ops

    dev = torch.device("cuda:0")
    R, W = B * T, (Hq + 2 * Hk) * hd
    buf = torch.randn(R, W, device=dev, dtype=torch.bfloat16)
    q = buf[:, :Hq * hd].view(B, T, Hq, hd).transpose(1, 2)
    k = buf[:, Hq * hd:(Hq + Hk) * hd].view(B, T, Hk, hd).transpose(1, 2)
    wq, wk = (1 + 0.1 * torch.randn(hd, device=dev)).bfloat16(), (1 + 0.1 * torch.randn(hd, device=dev)).bfloat16()
    ang = torch.rand(1, T, hd // 2, device=dev) * 6.28
    cos, sin = torch.cat((ang.cos(), ang.cos()), -1).bfloat16(), torch.cat((ang.sin(), ang.sin()), -1).bfloat16()
    assert tower_ops.head_norm_rope_supported(q, k, wq, wk, cos, sin)
    _, _, rq, rk, _ = tower_ops.head_norm_rope(q, k, wq, wk, 1e-6, 1e-6, cos, sin)
    gq = torch.randn(B, T, Hq, hd, device=dev, dtype=torch.bfloat16).transpose(1, 2)
    gk = torch.randn(B, T, Hk, hd, device=dev, dtype=torch.bfloat16).transpose(1, 2)
    qg, kg = q.detach().clone().requires_grad_(True), k.detach().clone().requires_grad_(True)      # dense leaves for autograd

    def eager_fwd(a, b):
        return apply_rotary_pos_emb(F.rms_norm(a, (hd,), wq, 1e-6), F.rms_norm(b, (hd,), wk, 1e-6), cos, sin)

    def eager_both():
        oq, ok = eager_fwd(qg, kg)
        return torch.autograd.grad((oq, ok), (qg, kg), (gq, gk))

    fns = {"kernel fwd (1 launch)": lambda: tower_ops.head_norm_rope(q, k, wq, wk, 1e-6, 1e-6, cos, sin),
           "kernel bwd (1 launch)": lambda: tower_ops.head_norm_bwd(gq, gk, q, k, wq, wk, rq, rk),
           "eager fwd (rms_norm x2 + rotary chain)": lambda: eager_fwd(q, k),
           "eager fwd + autograd bwd": eager_both}
    el, n = 2, R * (Hq + Hk) * hd
    nbytes = {"kernel fwd (1 launch)": 2 * n * el + R * (Hq + Hk) * 4, "kernel bwd (1 launch)": 3 * n * el + R * (Hq + Hk) * 4,
              "eager fwd (rms_norm x2 + rotary chain)": 2 * n * el + R * (Hq + Hk) * 4,
              "eager fwd + autograd bwd": 5 * n * el + 2 * R * (Hq + Hk) * 4}
    seen = {name: [] for name in fns}
    for _ in range(rounds):                      # alternate: every round visits all four
        for name, fn in fns.items():
            seen[name].append(time_graph(fn)[0])
    out = {}
    for name, ts in seen.items():
        ts.sort()
        med = ts[len(ts) // 2]
        out[name] = {"s": med, "lo": ts[0], "hi": ts[-1], "GBps": nbytes[name] / med / 1e9, "frac": nbytes[name] / med / HBM_PEAK}
    return out


def bench_embed_norm(B, T, D, p, rounds=3):
    """The RoBERTa-family embeddings front end (XLM-R-large tables: vocabulary 250002, 514 positions, one token type):
    `dalm_embed_norm_fwd` beside the module's own eager chain (positions from the ids, three gathers, two adds, f32 LayerNorm,
    dropout: ~20 launches) on the same right-padded ids, bf16 autocast, alternating in the same process.  Algorithmic bytes: the
    ids, three f32 table rows per token read, y32 + y16 written.  Every figure: median over `rounds` alternations of a 20-call
    graph's per-call time, with the lowest and highest round."""
    from transformers import XLMRobertaConfig
    from transformers.models.xlm_roberta.modeling_xlm_roberta import XLMRobertaEmbeddings

    from dalm_amd.models import bert_ops

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = XLMRobertaConfig(hidden_size=D, vocab_size=250002, max_position_embeddings=514, type_vocab_size=1, pad_token_id=1,
                           hidden_dropout_prob=p, layer_norm_eps=1e-5)
    emb = XLMRobertaEmbeddings(cfg).to(dev).requires_grad_(False).train()
    g = torch.Generator().manual_seed(1)
    lens = torch.randint(max(T // 4, 1), T + 1, (B, 1), generator=g)
    ids = torch.randint(3, 250002, (B, T), generator=g)
    ids = torch.where(torch.arange(T).unsqueeze(0) < lens, ids, torch.ones_like(ids)).to(dev)

    def kernel():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return bert_ops.embed_norm(emb, ids, None, None, p, 7)

    def eager():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return emb(input_ids=ids)

    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert bert_ops.embed_supported(emb, ids, None, None, None, 0)
    if p == 0.0:
        torch.testing.assert_close(kernel(), eager(), rtol=3e-6, atol=3e-6)
    fns = {"kernel (1 launch)": kernel, "eager chain": eager}
    nbytes = B * T * (8 + 3 * D * 4 + D * 4 + D * 2)
    seen = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            seen[name].append(time_graph(fn)[0])
    out = {}
    for name, ts in seen.items():
        ts.sort()
        med = ts[len(ts) // 2]
        out[name] = {"s": med, "lo": ts[0], "hi": ts[-1], "GBps": nbytes / med / 1e9, "frac": nbytes / med / HBM_PEAK}
    return out


def _alternating(fns, nbytes, rounds):
    """Median over `rounds` alternations (every round visits every function) of a 20-call graph's per-call time, with the lowest and
    highest round; GB/s and the HBM fraction from the algorithmic bytes of each function."""
    seen = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            seen[name].append(time_graph(fn)[0])
    out = {}
    for name, ts in seen.items():
        ts.sort()
        med = ts[len(ts) // 2]
        out[name] = {"s": med, "lo": ts[0], "hi": ts[-1], "GBps": nbytes[name] / med / 1e9, "frac": nbytes[name] / med / HBM_PEAK}
    return out


def bench_geglu(R, C, rounds=3):
    """GemmaMLP's activation: `dalm_geglu_fwd` / `dalm_geglu_bwd` on the gate | up halves of one [R, 2 C] bf16 buffer (the routed
    form: `frozen_linear.pair_forward`), and beside them - alternating, in the same process - the eager chain they replace on dense
    tensors: gelu(approximate="tanh") and a multiply, and autograd's backward of the two.  Algorithmic bytes: forward 3 R C
    elements, backward 5 R C (the eager chain moves more: it writes and re-reads the activation)."""
    import torch.nn.functional as F

    from dalm_amd import hip
    from dalm_amd.models import tower_ops

    dev = torch.device("cuda:0")
    buf = torch.randn(R, 2 * C, device=dev, dtype=torch.bfloat16)
    gate, up = buf[:, :C], buf[:, C:]
    assert tower_ops.geglu_supported(gate, up) and tower_ops._halves_of_one(gate, up)
    d_act = torch.randn(R, C, device=dev, dtype=torch.bfloat16)
    dg, du = torch.empty_like(d_act), torch.empty_like(d_act)
    gd, ud = gate.contiguous().requires_grad_(True), up.contiguous().requires_grad_(True)          # dense leaves for autograd

    def kernel_bwd():
        hip.call("dalm_geglu_bwd", hip.ptr(d_act), hip.ptr(gate), hip.ptr(up), hip.ptr(dg), hip.ptr(du), hip.dtype_code(gate), R, C, C,
                 2 * C, 2 * C, C, C, None, hip.stream())

    def eager_fwd(a, b):
        return F.gelu(a, approximate="tanh") * b

    def eager_both():
        return torch.autograd.grad(eager_fwd(gd, ud), (gd, ud), d_act)

    fns = {"kernel fwd (1 launch)": lambda: tower_ops.geglu(gate, up), "kernel bwd (1 launch)": kernel_bwd,
           "eager fwd (gelu, mul)": lambda: eager_fwd(gd.detach(), ud.detach()), "eager fwd + autograd bwd": eager_both}
    n = R * C * 2
    out = _alternating(fns, {"kernel fwd (1 launch)": 3 * n, "kernel bwd (1 launch)": 5 * n, "eager fwd (gelu, mul)": 3 * n,
                             "eager fwd + autograd bwd": 8 * n}, rounds)
    k, e = out["kernel fwd (1 launch)"]["s"] + out["kernel bwd (1 launch)"]["s"], out["eager fwd + autograd bwd"]["s"]
    out["kernel fwd + bwd against eager"] = {"kernel_s": k, "eager_s": e, "eager_over_kernel": e / k}
    out["kernel fwd against eager fwd"] = {"eager_over_kernel": out["eager fwd (gelu, mul)"]["s"] / out["kernel fwd (1 launch)"]["s"]}
    return out


def bench_relu2(R, C, rounds=3):
    """ArceeMLP's activation: `dalm_relu2_fwd` / `dalm_relu2_bwd` on a dense [R, C] bf16 tensor, and beside them - alternating, in the
    same process - the eager chain they replace: relu and square, and autograd's backward of the two.  Algorithmic bytes: forward
    2 R C elements, backward 3 R C (the eager chain moves more: it writes and re-reads relu(y))."""
    import torch.nn.functional as F

    from dalm_amd import hip
    from dalm_amd.models import tower_ops

    dev = torch.device("cuda:0")
    y = torch.randn(R, C, device=dev, dtype=torch.bfloat16)
    assert tower_ops.relu2_supported(y)
    d_act = torch.randn(R, C, device=dev, dtype=torch.bfloat16)
    dy = torch.empty_like(d_act)
    yd = y.clone().requires_grad_(True)

    def kernel_bwd():
        hip.call("dalm_relu2_bwd", hip.ptr(d_act), hip.ptr(y), hip.ptr(dy), hip.dtype_code(y), R, C, C, C, C, None, hip.stream())

    def eager_fwd(a):
        return torch.square(F.relu(a))

    def eager_both():
        return torch.autograd.grad(eager_fwd(yd), (yd,), d_act)

    fns = {"kernel fwd (1 launch)": lambda: tower_ops.relu2(y), "kernel bwd (1 launch)": kernel_bwd,
           "eager fwd (relu, square)": lambda: eager_fwd(y), "eager fwd + autograd bwd": eager_both}
    n = R * C * 2
    out = _alternating(fns, {"kernel fwd (1 launch)": 2 * n, "kernel bwd (1 launch)": 3 * n, "eager fwd (relu, square)": 2 * n,
                             "eager fwd + autograd bwd": 5 * n}, rounds)
    k, e = out["kernel fwd (1 launch)"]["s"] + out["kernel bwd (1 launch)"]["s"], out["eager fwd + autograd bwd"]["s"]
    out["kernel fwd + bwd against eager"] = {"kernel_s": k, "eager_s": e, "eager_over_kernel": e / k}
    out["kernel fwd against eager fwd"] = {"eager_over_kernel": out["eager fwd (relu, square)"]["s"] / out["kernel fwd (1 launch)"]["s"]}
    return out


def bench_gemma_norm(R, D, rounds=3):
    """GemmaRMSNorm with the residual add in front of it: `dalm_gemma_norm_fwd` (x + delta and the norm) / `dalm_gemma_norm_bwd`
    (with the residual-path gradient) on [R, D] bf16 rows with a bf16 weight, and beside them - alternating, in the same process -
    the eager add + transformers' GemmaRMSNorm.forward (an f32 chain of ~8 launches) and autograd's backward of it.  Algorithmic
    bytes: forward 4 R D elements (+ rstd), backward 4 R D (+ rstd)."""
    from transformers.models.gemma.modeling_gemma import GemmaRMSNorm

    from dalm_amd import hip
    from dalm_amd.models import tower_ops

    dev = torch.device("cuda:0")
    x = torch.randn(R, D, device=dev, dtype=torch.bfloat16)
    delta = torch.randn(R, D, device=dev, dtype=torch.bfloat16)
    gy, gres = torch.randn_like(x), torch.randn_like(x)
    norm = GemmaRMSNorm(D, eps=1e-6).to(dev).to(torch.bfloat16).requires_grad_(False)
    with torch.no_grad():
        norm.weight.copy_(0.1 * torch.randn(D, device=dev))
    w = norm.weight
    assert tower_ops.gemma_rms_norm_supported(x, w)
    with torch.no_grad():
        h, _ = tower_ops.gemma_add_rms_norm(x, delta, w, 1e-6)
    rstd = torch.rsqrt(h.float().pow(2).mean(-1) + 1e-6)
    dx = torch.empty_like(x)
    xd, dd = x.clone().requires_grad_(True), delta.clone().requires_grad_(True)

    def kernel_fwd():
        with torch.no_grad():
            return tower_ops.gemma_add_rms_norm(x, delta, w, 1e-6)

    def kernel_bwd():
        hip.call("dalm_gemma_norm_bwd", hip.ptr(gy), hip.ptr(h), hip.ptr(w), hip.ptr(rstd), hip.ptr(gres), hip.dtype_code(h),
                 hip.dtype_code(w), R, D, hip.ptr(dx), None, hip.stream())

    def eager_fwd(a, b):
        hh = a + b
        return hh, norm(hh)

    def eager_both():
        return torch.autograd.grad(eager_fwd(xd, dd), (xd, dd), (gres, gy))

    def eager_fwd_only():
        with torch.no_grad():
            return eager_fwd(x, delta)

    fns = {"kernel fwd (1 launch)": kernel_fwd, "kernel bwd (1 launch)": kernel_bwd, "eager fwd (add + f32 chain)": eager_fwd_only,
           "eager fwd + autograd bwd": eager_both}
    n = R * D * 2
    out = _alternating(fns, {"kernel fwd (1 launch)": 4 * n + 4 * R, "kernel bwd (1 launch)": 4 * n + 4 * R,
                             "eager fwd (add + f32 chain)": 4 * n, "eager fwd + autograd bwd": 8 * n}, rounds)
    k, e = out["kernel fwd (1 launch)"]["s"] + out["kernel bwd (1 launch)"]["s"], out["eager fwd + autograd bwd"]["s"]
    out["kernel fwd + bwd against eager"] = {"kernel_s": k, "eager_s": e, "eager_over_kernel": e / k}
    out["kernel fwd against eager fwd"] = {"eager_over_kernel": out["eager fwd (add + f32 chain)"]["s"] / out["kernel fwd (1 launch)"]["s"]}
    return out


def bench_norm_add(R, D, rounds=3):
    """OLMo-2's post-norm pair, `residual + Olmo2RMSNorm(x)`: `dalm_norm_add_fwd` / `dalm_norm_add_bwd` on [R, D] bf16 rows with a bf16
    weight, and beside them - alternating, in the same process - the two forms they replace: transformers' Olmo2RMSNorm.forward (an
    f32 chain) + the add, and F.rms_norm + the add (what `use_native_rms_norm` alone leaves: the unrouted model of today), each with
    autograd's backward.  Algorithmic bytes: forward 3 R D elements (+ rstd), backward 3 R D (+ rstd; the residual's gradient is the
    incoming one: no traffic)."""
    import torch.nn.functional as F
    from transformers.models.olmo2.modeling_olmo2 import Olmo2RMSNorm

    from dalm_amd import hip
    from dalm_amd.models import tower_ops

    dev = torch.device("cuda:0")
    x = torch.randn(R, D, device=dev, dtype=torch.bfloat16)
    res = torch.randn(R, D, device=dev, dtype=torch.bfloat16)
    gy = torch.randn_like(x)
    norm = Olmo2RMSNorm(D, eps=1e-6).to(dev).to(torch.bfloat16).requires_grad_(False)
    with torch.no_grad():
        norm.weight.copy_(1.0 + 0.1 * torch.randn(D, device=dev))
    w = norm.weight
    assert tower_ops.norm_add_supported(x, res, w)
    rstd = torch.rsqrt(x.float().pow(2).mean(-1) + 1e-6)
    dx = torch.empty_like(x)
    xd, rd = x.clone().requires_grad_(True), res.clone().requires_grad_(True)

    def kernel_fwd():
        with torch.no_grad():
            return tower_ops.norm_add(x, res, w, 1e-6)

    def kernel_bwd():
        hip.call("dalm_norm_add_bwd", hip.ptr(gy), hip.ptr(x), hip.ptr(w), hip.ptr(rstd), hip.dtype_code(x), hip.dtype_code(w), R, D,
                 hip.ptr(dx), None, hip.stream())

    def native(a, b):
        return b + F.rms_norm(a, (D,), w, 1e-6)

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn(x, res)
        return run

    fns = {"kernel fwd (1 launch)": kernel_fwd, "kernel bwd (1 launch)": kernel_bwd,
           "eager fwd (f32 chain + add)": no_grad(lambda a, b: b + norm(a)),
           "eager fwd + autograd bwd": lambda: torch.autograd.grad(rd + norm(xd), (xd, rd), gy),
           "native fwd (F.rms_norm + add)": no_grad(native),
           "native fwd + autograd bwd": lambda: torch.autograd.grad(native(xd, rd), (xd, rd), gy)}
    n = R * D * 2
    out = _alternating(fns, {"kernel fwd (1 launch)": 3 * n + 4 * R, "kernel bwd (1 launch)": 3 * n + 4 * R,
                             "eager fwd (f32 chain + add)": 3 * n, "eager fwd + autograd bwd": 6 * n,
                             "native fwd (F.rms_norm + add)": 3 * n, "native fwd + autograd bwd": 6 * n}, rounds)
    k = out["kernel fwd (1 launch)"]["s"] + out["kernel bwd (1 launch)"]["s"]
    for other in ("eager", "native"):
        e = out[f"{other} fwd + autograd bwd"]["s"]
        out[f"kernel fwd + bwd against {other}"] = {"kernel_s": k, f"{other}_s": e, f"{other}_over_kernel": e / k}
    return out


def bench_scaled_add_norm(R, D, mult=0.22, rounds=3):
    """Granite's two scaled residual adds on [R, D] bf16 rows.  With the norm behind it, `residual + attn_out * m` then GraniteRMSNorm:
    `dalm_rms_norm_scaled_fwd` / `dalm_rms_norm_scaled_bwd`, and beside them - alternating, in the same process - the two forms they
    replace: the eager multiply and add + transformers' GraniteRMSNorm.forward (an f32 chain), and the eager multiply and add +
    F.rms_norm (what `use_native_rms_norm` alone leaves: the unrouted model of today), each with autograd's backward, in which the
    gradient through the residual path meets the norm's.  Alone, `residual + mlp_out * m`: `dalm_scale_add` each way against the eager
    pair.  Algorithmic bytes: norm forward 4 R D elements (x, delta in; h, y out), backward 5 R D (dy, h, dres in; dx, ddelta out);
    scale_add forward 3 R D, backward 2 R D (the residual's gradient is the incoming one: no traffic)."""
    import torch.nn.functional as F
    from transformers.models.granite.modeling_granite import GraniteRMSNorm

    from dalm_amd import hip
    from dalm_amd.models import tower_ops

    dev = torch.device("cuda:0")
    x, delta, gy, gh = (torch.randn(R, D, device=dev, dtype=torch.bfloat16) for _ in range(4))
    norm = GraniteRMSNorm(D, eps=1e-6).to(dev).to(torch.bfloat16).requires_grad_(False)
    with torch.no_grad():
        norm.weight.copy_(1.0 + 0.1 * torch.randn(D, device=dev))
    w = norm.weight
    assert tower_ops.scaled_add_rms_norm_supported(x, w) and tower_ops.scale_add_supported(delta, x)
    with torch.no_grad():
        h, _ = tower_ops.scaled_add_rms_norm(x, delta, mult, w, 1e-6)
    rstd = torch.rsqrt(h.float().pow(2).mean(-1) + 1e-6)
    dx, dd = torch.empty_like(x), torch.empty_like(x)
    xd, dl = x.clone().requires_grad_(True), delta.clone().requires_grad_(True)

    def kernel_fwd():
        with torch.no_grad():
            return tower_ops.scaled_add_rms_norm(x, delta, mult, w, 1e-6)

    def kernel_bwd():
        hip.call("dalm_rms_norm_scaled_bwd", hip.ptr(gy), hip.ptr(h), hip.ptr(w), hip.ptr(rstd), hip.ptr(gh), mult, hip.dtype_code(h), R, D,
                 hip.ptr(dx), hip.ptr(dd), None, hip.stream())

    def pair(normed):
        def fwd(a, b):
            hh = a + b * mult
            return hh, normed(hh)
        return fwd

    eager, native = pair(norm), pair(lambda t: F.rms_norm(t, (D,), w, 1e-6))

    def no_grad(fn, *a):
        def run():
            with torch.no_grad():
                return fn(*a)
        return run

    def add_kernel_bwd():
        with torch.no_grad():
            return tower_ops.scale_add(None, gy, mult)

    n = R * D * 2
    fns = {"norm kernel fwd (1 launch)": kernel_fwd, "norm kernel bwd (1 launch)": kernel_bwd,
           "norm eager fwd (mul + add + f32 chain)": no_grad(eager, x, delta),
           "norm eager fwd + autograd bwd": lambda: torch.autograd.grad(eager(xd, dl), (xd, dl), (gh, gy)),
           "norm native fwd (mul + add + F.rms_norm)": no_grad(native, x, delta),
           "norm native fwd + autograd bwd": lambda: torch.autograd.grad(native(xd, dl), (xd, dl), (gh, gy)),
           "add kernel fwd (1 launch)": no_grad(tower_ops.scale_add, x, delta, mult), "add kernel bwd (1 launch)": add_kernel_bwd,
           "add eager fwd (mul + add)": no_grad(lambda a, b: a + b * mult, x, delta),
           "add eager fwd + autograd bwd": lambda: torch.autograd.grad(xd + dl * mult, (xd, dl), gy)}
    out = _alternating(fns, {"norm kernel fwd (1 launch)": 4 * n + 4 * R, "norm kernel bwd (1 launch)": 5 * n + 4 * R,
                             "norm eager fwd (mul + add + f32 chain)": 4 * n, "norm eager fwd + autograd bwd": 9 * n,
                             "norm native fwd (mul + add + F.rms_norm)": 4 * n, "norm native fwd + autograd bwd": 9 * n,
                             "add kernel fwd (1 launch)": 3 * n, "add kernel bwd (1 launch)": 2 * n, "add eager fwd (mul + add)": 3 * n,
                             "add eager fwd + autograd bwd": 5 * n}, rounds)
    k = out["norm kernel fwd (1 launch)"]["s"] + out["norm kernel bwd (1 launch)"]["s"]
    for other in ("eager", "native"):
        e = out[f"norm {other} fwd + autograd bwd"]["s"]
        out[f"norm kernel fwd + bwd against {other}"] = {"kernel_s": k, f"{other}_s": e, f"{other}_over_kernel": e / k}
    k, e = out["add kernel fwd (1 launch)"]["s"] + out["add kernel bwd (1 launch)"]["s"], out["add eager fwd + autograd bwd"]["s"]
    out["add kernel fwd + bwd against eager"] = {"kernel_s": k, "eager_s": e, "eager_over_kernel": e / k}
    return out


def _no_grad(fn, *a):
    def run():
        with torch.no_grad():
            return fn(*a)
    return run


def bench_cohere_norm(R, D, rounds=3):
    """CohereLayerNorm on [R, D] bf16 rows with the residual-path gradient folded into the backward: `dalm_cohere_norm_fwd` /
    `dalm_cohere_norm_bwd`, and beside them - alternating, in the same process - transformers' CohereLayerNorm.forward (an f32 chain)
    with autograd's backward, in which the gradient through the residual path meets the norm's.  Algorithmic bytes: forward 2 R D
    elements (x in, y out), backward 4 R D (dy, x, dres in; dx out)."""
    from transformers.models.cohere.modeling_cohere import CohereLayerNorm

    from dalm_amd import hip
    from dalm_amd.models import tower_ops

    dev = torch.device("cuda:0")
    x, gy, gh = (torch.randn(R, D, device=dev, dtype=torch.bfloat16) for _ in range(3))
    norm = CohereLayerNorm(D, eps=1e-5).to(dev).to(torch.bfloat16).requires_grad_(False)
    with torch.no_grad():
        norm.weight.copy_(1.0 + 0.1 * torch.randn(D, device=dev))
    w = norm.weight
    assert tower_ops.cohere_norm_supported(x, w)
    mean = x.float().mean(-1)
    rstd = torch.rsqrt(x.float().var(-1, unbiased=False) + 1e-5)
    dx = torch.empty_like(x)
    xd = x.clone().requires_grad_(True)

    def kernel_bwd():
        hip.call("dalm_cohere_norm_bwd", hip.ptr(gy), hip.ptr(x), hip.ptr(w), hip.ptr(mean), hip.ptr(rstd), hip.ptr(gh), hip.dtype_code(x),
                 hip.dtype_code(w), R, D, hip.ptr(dx), None, hip.stream())

    n = R * D * 2
    fns = {"kernel fwd (1 launch)": _no_grad(tower_ops.cohere_norm_res, x, w, 1e-5), "kernel bwd (1 launch)": kernel_bwd,
           "eager fwd (f32 chain)": _no_grad(norm, x),
           "eager fwd + autograd bwd": lambda: torch.autograd.grad((xd.view_as(xd), norm(xd)), (xd,), (gh, gy))}
    out = _alternating(fns, {"kernel fwd (1 launch)": 2 * n + 8 * R, "kernel bwd (1 launch)": 4 * n + 8 * R, "eager fwd (f32 chain)": 2 * n,
                             "eager fwd + autograd bwd": 6 * n}, rounds)
    k, e = out["kernel fwd (1 launch)"]["s"] + out["kernel bwd (1 launch)"]["s"], out["eager fwd + autograd bwd"]["s"]
    out["kernel fwd + bwd against eager"] = {"kernel_s": k, "eager_s": e, "eager_over_kernel": e / k}
    return out


def bench_rope_il(B, T, Hq, Hk, hd, rounds=3):
    """Cohere's interleaved rotary embedding computed in f32: `dalm_rope_il_qk` forward and backward on the q | k column slices of one
    [B T, (Hq + 2 Hk) hd] bf16 buffer, and beside them - alternating, in the same process - modeling_cohere.py's apply_rotary_pos_emb
    with autograd's backward.  Algorithmic bytes: 2 (|q| + |k|) elements each way (+ the tables, shared by all heads)."""
    from transformers.models.cohere.modeling_cohere import apply_rotary_pos_emb

    from dalm_amd.models import tower_ops

    dev = torch.device("cuda:0")
    W = (Hq + 2 * Hk) * hd
    buf = torch.randn(B, T, W, device=dev, dtype=torch.bfloat16)
    q = buf[..., :Hq * hd].view(B, T, Hq, hd).transpose(1, 2)
    k = buf[..., Hq * hd:(Hq + Hk) * hd].view(B, T, Hk, hd).transpose(1, 2)
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, device=dev).float() / hd))
    emb = torch.repeat_interleave(torch.arange(T, device=dev).float()[None, :, None] * inv, 2, dim=-1)
    cos, sin = emb.cos().to(torch.bfloat16), emb.sin().to(torch.bfloat16)
    assert tower_ops.rope_il_supported(q, k, cos, sin)
    gq, gk = torch.randn(B, T, Hq, hd, device=dev, dtype=torch.bfloat16).transpose(1, 2), \
        torch.randn(B, T, Hk, hd, device=dev, dtype=torch.bfloat16).transpose(1, 2)
    qf, kf = buf[..., :Hq * hd], buf[..., Hq * hd:(Hq + Hk) * hd]
    qg, kg = qf.detach().clone().requires_grad_(True), kf.detach().clone().requires_grad_(True)        # dense leaves for autograd

    def eager_both():
        oq, ok = apply_rotary_pos_emb(qg.view(B, T, Hq, hd).transpose(1, 2), kg.view(B, T, Hk, hd).transpose(1, 2), cos, sin)
        return torch.autograd.grad((oq, ok), (qg, kg), (gq, gk))

    b = 2 * B * T * (Hq + Hk) * hd * 2 + 2 * T * hd * 2
    fns = {"kernel fwd (1 launch)": lambda: tower_ops._rope_il_launch(q, k, cos, sin, False),
           "kernel bwd (1 launch, in place)": lambda: tower_ops._rope_il_launch(gq, gk, cos, sin, True, None, in_place=True),
           "eager fwd (f32 chain)": _no_grad(apply_rotary_pos_emb, q, k, cos, sin),
           "eager fwd + autograd bwd": eager_both}
    out = _alternating(fns, {name: (2 * b if "+" in name else b) for name in fns}, rounds)
    k_s, e = out["kernel fwd (1 launch)"]["s"] + out["kernel bwd (1 launch, in place)"]["s"], out["eager fwd + autograd bwd"]["s"]
    out["kernel fwd + bwd against eager"] = {"kernel_s": k_s, "eager_s": e, "eager_over_kernel": e / k_s}
    return out


def bench_rope_partial(B, T, Hq, Hk, hd, rot, rounds=3):
    """Phi-3's partial rotary embedding: `dalm_rope_partial_qk` forward and backward on the q | k column slices of one
    [B T, (Hq + 2 Hk) hd] bf16 buffer - qkv_proj's output -, and beside them - alternating, in the same process - modeling_phi3.py's
    apply_rotary_pos_emb with autograd's backward.  Algorithmic bytes: (|q| + |k|) elements read and as many written each way (+ the
    tables [T, rot], shared by all heads); the in-place backward - the attention node's un-rotation - moves the rotated part only."""
    from transformers.models.phi3.modeling_phi3 import apply_rotary_pos_emb

    from dalm_amd.models import tower_ops

    dev = torch.device("cuda:0")
    W = (Hq + 2 * Hk) * hd
    buf = torch.randn(B, T, W, device=dev, dtype=torch.bfloat16)
    q = buf[..., :Hq * hd].view(B, T, Hq, hd).transpose(1, 2)
    k = buf[..., Hq * hd:(Hq + Hk) * hd].view(B, T, Hk, hd).transpose(1, 2)
    inv = 1.0 / (10000.0 ** (torch.arange(0, rot, 2, device=dev).float() / rot))
    ang = torch.arange(T, device=dev).float()[None, :, None] * inv
    emb = torch.cat((ang, ang), dim=-1)
    cos, sin = emb.cos().to(torch.bfloat16), emb.sin().to(torch.bfloat16)
    assert tower_ops.rope_partial_supported(q, k, cos, sin)
    gq, gk = torch.randn(B, T, Hq, hd, device=dev, dtype=torch.bfloat16).transpose(1, 2), \
        torch.randn(B, T, Hk, hd, device=dev, dtype=torch.bfloat16).transpose(1, 2)
    qg = buf[..., :Hq * hd].detach().clone().requires_grad_(True)                                      # dense leaves for autograd
    kg = buf[..., Hq * hd:(Hq + Hk) * hd].detach().clone().requires_grad_(True)

    def eager_both():
        oq, ok = apply_rotary_pos_emb(qg.view(B, T, Hq, hd).transpose(1, 2), kg.view(B, T, Hk, hd).transpose(1, 2), cos, sin)
        return torch.autograd.grad((oq, ok), (qg, kg), (gq, gk))

    tables = 2 * T * rot * 2
    b = 2 * B * T * (Hq + Hk) * hd * 2 + tables
    b_rot = 2 * B * T * (Hq + Hk) * rot * 2 + tables
    fns = {"kernel fwd (1 launch)": lambda: tower_ops._rope_partial_launch(q, k, cos, sin, False),
           "kernel bwd (1 launch)": lambda: tower_ops._rope_partial_launch(gq, gk, cos, sin, True),
           "kernel bwd (1 launch, in place)": lambda: tower_ops._rope_partial_launch(gq, gk, cos, sin, True, None, in_place=True),
           "eager fwd": _no_grad(apply_rotary_pos_emb, q, k, cos, sin),
           "eager fwd + autograd bwd": eager_both}
    nbytes = {name: (2 * b if "+" in name else b_rot if "in place" in name else b) for name in fns}
    out = _alternating(fns, nbytes, rounds)
    k_s, e = out["kernel fwd (1 launch)"]["s"] + out["kernel bwd (1 launch)"]["s"], out["eager fwd + autograd bwd"]["s"]
    out["kernel fwd + bwd against eager"] = {"kernel_s": k_s, "eager_s": e, "eager_over_kernel": e / k_s}
    return out


def bench_add3(R, D, rounds=3):
    """Cohere's `residual + attn + mlp` on [R, D] bf16 rows: `dalm_add3_live` (its backward hands the gradient on: no launch) against
    the eager pair of adds.  Algorithmic bytes: 4 R D elements."""
    from dalm_amd.models import tower_ops

    dev = torch.device("cuda:0")
    r, a, b = (torch.randn(R, D, device=dev, dtype=torch.bfloat16) for _ in range(3))
    assert tower_ops.add3_live_supported(r, a, b)
    n = R * D * 2
    fns = {"kernel (1 launch)": _no_grad(tower_ops.add3_live, r, a, b), "eager (2 launches)": _no_grad(lambda x, y, z: x + y + z, r, a, b)}
    out = _alternating(fns, {"kernel (1 launch)": 4 * n, "eager (2 launches)": 4 * n}, rounds)
    out["kernel against eager"] = {"kernel_s": out["kernel (1 launch)"]["s"], "eager_s": out["eager (2 launches)"]["s"],
                                   "eager_over_kernel": out["eager (2 launches)"]["s"] / out["kernel (1 launch)"]["s"]}
    return out


def bench_row_norm_rope(B, T, Hq, Hk, hd, rounds=3):
    """OLMo-2's q_norm / k_norm over the whole projection width + rotary embedding: `dalm_row_norm_rope_fwd` / `dalm_row_norm_bwd` on
    the q | k column slices of one [B T, (Hq + 2 Hk) hd] bf16 buffer, and beside them - alternating, in the same process - what runs
    without them for the same math: F.rms_norm x 2 over the rows (what `use_native_rms_norm` leaves of Olmo2RMSNorm) + the head views
    + transformers' eager rotary chain, and autograd's backward of that.  Algorithmic bytes as `bench_head_norm_rope`, one rstd per
    token and tensor."""
    import torch.nn.functional as F
    from transformers.models.olmo2.modeling_olmo2 import apply_rotary_pos_emb

    from dalm_amd.models import tower_ops

    dev = torch.device("cuda:0")
    R, W = B * T, (Hq + 2 * Hk) * hd
    buf = torch.randn(R, W, device=dev, dtype=torch.bfloat16)
    q = buf[:, :Hq * hd].view(B, T, Hq, hd).transpose(1, 2)
    k = buf[:, Hq * hd:(Hq + Hk) * hd].view(B, T, Hk, hd).transpose(1, 2)
    wq, wk = (1 + 0.1 * torch.randn(Hq * hd, device=dev)).bfloat16(), (1 + 0.1 * torch.randn(Hk * hd, device=dev)).bfloat16()
    ang = torch.rand(1, T, hd // 2, device=dev) * 6.28
    cos, sin = torch.cat((ang.cos(), ang.cos()), -1).bfloat16(), torch.cat((ang.sin(), ang.sin()), -1).bfloat16()
    assert tower_ops.row_norm_rope_supported(q, k, wq, wk, cos, sin)
    _, _, rq, rk, _ = tower_ops.row_norm_rope(q, k, wq, wk, 1e-6, 1e-6, cos, sin)
    gq = torch.randn(B, T, Hq, hd, device=dev, dtype=torch.bfloat16).transpose(1, 2)
    gk = torch.randn(B, T, Hk, hd, device=dev, dtype=torch.bfloat16).transpose(1, 2)
    qf, kf = buf[:, :Hq * hd].view(B, T, Hq * hd), buf[:, Hq * hd:(Hq + Hk) * hd].view(B, T, Hk * hd)     # what q_norm / k_norm see
    qg, kg = qf.detach().clone().requires_grad_(True), kf.detach().clone().requires_grad_(True)        # dense leaves for autograd

    def eager_fwd(a, b):
        a, b = F.rms_norm(a, (Hq * hd,), wq, 1e-6), F.rms_norm(b, (Hk * hd,), wk, 1e-6)
        return apply_rotary_pos_emb(a.view(B, T, Hq, hd).transpose(1, 2), b.view(B, T, Hk, hd).transpose(1, 2), cos, sin)

    def eager_both():
        oq, ok = eager_fwd(qg, kg)
        return torch.autograd.grad((oq, ok), (qg, kg), (gq, gk))

    fns = {"kernel fwd (1 launch)": lambda: tower_ops.row_norm_rope(q, k, wq, wk, 1e-6, 1e-6, cos, sin),
           "kernel bwd (1 launch)": lambda: tower_ops.row_norm_bwd(gq, gk, q, k, wq, wk, rq, rk),
           "eager fwd (rms_norm x2 + rotary chain)": lambda: eager_fwd(qf, kf),
           "eager fwd + autograd bwd": eager_both}
    n = R * (Hq + Hk) * hd * 2
    out = _alternating(fns, {"kernel fwd (1 launch)": 2 * n + 8 * R, "kernel bwd (1 launch)": 3 * n + 8 * R,
                             "eager fwd (rms_norm x2 + rotary chain)": 2 * n + 8 * R, "eager fwd + autograd bwd": 5 * n + 16 * R}, rounds)
    k_s, e_s = out["kernel fwd (1 launch)"]["s"] + out["kernel bwd (1 launch)"]["s"], out["eager fwd + autograd bwd"]["s"]
    out["kernel fwd + bwd against eager"] = {"kernel_s": k_s, "eager_s": e_s, "eager_over_kernel": e_s / k_s}
    return out


def bench_linear_live(members, halves):
    """dalm_linear_live against the tuned library GEMM at 4608 padded rows under the first mask of the step bench
    (tools/linear_live_bench.py holds the arms and the timing; its own run covers every mask)."""
    import linear_live_bench as llb
    from dalm_amd.tuning import enable_tuned_gemms

    enable_tuned_gemms()
    dev = torch.device("cuda")
    _, res = llb.bench_gemm(members, halves, llb.masks(dev)[1:2], dev, lambda s: None)[0]
    return {arm: {"s": t, "spread_s": sp} for arm, (t, sp) in res.items()}


def print_results(res) -> None:
    for k, v in res.items():
        print(k)
        for kk, vv in v.items():
            # values are numbers except for labels such as "pipe": "bf16 x3" (formatting every value with :.4g crashed the
            # whole run on the first similarity entry in round 5, before the JSON was written)
            print("   %-18s" % kk, "  ".join(f"{a}={b:.4g}" if isinstance(b, (int, float)) else f"{a}={b}" for a, b in vv.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--vocab", type=int, default=0,
                    help="with --only ce: run the B = 18 shapes of this vocabulary size only (PMC passes: one process per V, "
                         "because the counter CSV cannot tell two launches of one instantiation with the same grid apart)")
    ap.add_argument("--sizes", default="", help="with --only sim: square sizes to run instead of the standard list, e.g. 1200,1536")
    args = ap.parse_args()
    res = {}
    if args.only in ("", "ce"):
        for name, B, V, dt in (("ce cfg3 B18 Tg256 V32000 f32", 18, 32000, torch.float32),
                               ("ce cfg3 B18 Tg256 V32000 bf16", 18, 32000, torch.bfloat16),
                               ("ce cfg5 B18 Tg256 V65024 bf16", 18, 65024, torch.bfloat16),
                               ("ce cfg5 B18 Tg256 V65024 f32", 18, 65024, torch.float32),
                               ("ce B144 Tg256 V32000 f32 (8x)", 144, 32000, torch.float32)):
            if args.vocab and (V != args.vocab or B != 18):
                continue
            res[name] = bench_ce(B, 256, V, dt)
    if args.only in ("", "sim"):
        sizes = [(18, 18), (150, 150), (1200, 1200), (4096, 4096), (16384, 16384)]
        if not args.quick:
            sizes.append((65536, 65536))
        if args.sizes:
            sizes = [(int(x), int(x)) for x in args.sizes.split(",")]
        for m, n in sizes:
            res[f"sim {m}x{n} D1024"] = bench_sim(m, n, 1024)
        # per-rank blocks of the sharded negatives at W = 8: cfg3 (18 x 144) and cfg2 (150 x 1200)
        for m, n in ([] if args.sizes else [(18, 144), (150, 1200)]):
            res[f"sim sharded {m}x{n} D1024"] = bench_sim(m, n, 1024)
    if args.only in ("", "small"):
        for m, n in [(18, 18), (150, 150), (512, 512)]:
            res[f"small {m}x{n} D1024 (one GPU: rows+cols)"] = bench_small(m, n, 1024, True)
        for m, n in [(18, 144), (150, 1200)]:
            res[f"small sharded {m}x{n} D1024 (rows only)"] = bench_small(m, n, 1024, False)
    if args.only in ("", "pool"):
        res["pool cfg3 q B18 T50 D1024 bf16"] = bench_pool(18, 50, 1024, torch.bfloat16)
        res["pool cfg3 p B18 T128 D1024 bf16"] = bench_pool(18, 128, 1024, torch.bfloat16)
        res["pool cfg2 p B150 T128 D1024 bf16"] = bench_pool(150, 128, 1024, torch.bfloat16)
        res["pool cfg2 q B150 T50 D1024 f32"] = bench_pool(150, 50, 1024, torch.float32)
        res["pool cfg2 p B150 T128 D1024 f32"] = bench_pool(150, 128, 1024, torch.float32)
        res["pool cfg3 p B18 T128 D1024 f32"] = bench_pool(18, 128, 1024, torch.float32)
        res["pool B1200 T128 D1024 bf16"] = bench_pool(1200, 128, 1024, torch.bfloat16)
    if args.only in ("", "pool", "pool_last"):
        res["pool_last B150 T128 D1024 bf16"] = bench_pool_last(150, 128, 1024, torch.bfloat16)
        res["pool_last B150 T128 D4096 bf16"] = bench_pool_last(150, 128, 4096, torch.bfloat16)
        res["pool_last B150 T50 D4096 bf16"] = bench_pool_last(150, 50, 4096, torch.bfloat16)
        res["pool_last B150 T128 D4096 f32"] = bench_pool_last(150, 128, 4096, torch.float32)
        res["pool_last B18 T128 D4096 bf16"] = bench_pool_last(18, 128, 4096, torch.bfloat16)
    if args.only in ("", "nf4"):
        res["nf4 11008x4096 -> bf16"] = bench_nf4(11008, 4096, torch.bfloat16)
        res["nf4 4096x4096 -> bf16"] = bench_nf4(4096, 4096, torch.bfloat16)
        res["nf4 11008x4096 -> f32"] = bench_nf4(11008, 4096, torch.float32)
    if args.only in ("", "tower"):
        res["tower cfg3 layer: rope [18,32,256,128] + swiglu [4608,11008] bf16"] = bench_tower(18, 256, 32, 128, 11008, torch.bfloat16)
    if args.only in ("", "head_norm_rope"):
        res["head_norm_rope Qwen3-8B generator rows 18x256, 32+8 heads x 128"] = bench_head_norm_rope(18, 256, 32, 8, 128)
        res["head_norm_rope Qwen3-8B packed rows 1x3008, 32+8 heads x 128"] = bench_head_norm_rope(1, 3008, 32, 8, 128)
    if args.only in ("", "embed_norm"):
        for B, T in ((150, 128), (150, 50)):
            for p in (0.0, 0.1):
                res[f"embed_norm XLM-R-large retriever-only rows {B}x{T} D1024 p={p}"] = bench_embed_norm(B, T, 1024, p)
    if args.only in ("", "linear_live"):
        sys.path.insert(0, str(Path(__file__).resolve().parent))
        import linear_live_bench as llb

        for name, members, halves in llb.GEMMS:
            res[f"linear_live {name} rows 4608 N{members[0][0]} K{members[0][1]} (batch 100 mask)"] = bench_linear_live(members, halves)
    # the headline batch's rows (18 x 256) at Gemma-7B's widths: intermediate 24576, hidden 3072
    if args.only in ("", "geglu"):
        res["geglu Gemma-7B rows 4608 x 24576 bf16 (halves of one [R, 2 C] buffer)"] = bench_geglu(4608, 24576)
        res["geglu rows 4608 x 3072 bf16 (halves of one [R, 2 C] buffer)"] = bench_geglu(4608, 3072)
    if args.only in ("", "gemma_norm"):
        # (24576 is the MLP's width, not a norm's: the norm kernels take rows of at most 8192 elements)
        res["gemma_norm Gemma-7B rows 4608 x 3072 bf16 (add + norm)"] = bench_gemma_norm(4608, 3072)
    # the headline batch's rows (18 x 256) at AFM-4.5B's widths: intermediate 18432, hidden 2560
    if args.only in ("", "relu2"):
        res["relu2 AFM-4.5B rows 4608 x 18432 bf16"] = bench_relu2(4608, 18432)
        res["relu2 rows 4608 x 2560 bf16"] = bench_relu2(4608, 2560)
    # the headline batch's rows (18 x 256) at OLMo-2-7B's widths: hidden 4096, 32 x 128 heads (MHA); and OLMo-2-13B's hidden 5120
    if args.only in ("", "norm_add"):
        res["norm_add OLMo-2-7B rows 4608 x 4096 bf16 (norm + add)"] = bench_norm_add(4608, 4096)
        res["norm_add OLMo-2-13B rows 4608 x 5120 bf16 (norm + add)"] = bench_norm_add(4608, 5120)
    if args.only in ("", "row_norm_rope"):
        res["row_norm_rope OLMo-2-7B generator rows 18x256, 32+32 heads x 128"] = bench_row_norm_rope(18, 256, 32, 32, 128)
        res["row_norm_rope OLMo-2-7B packed rows 1x3008, 32+32 heads x 128"] = bench_row_norm_rope(1, 3008, 32, 32, 128)
    # the headline batch's rows at Granite's widths: hidden 2048 (granite-3.x-2b) and 4096 (granite-3.x-8b)
    if args.only in ("", "scaled_add_norm"):
        res["scaled_add_norm Granite-2B rows 4608 x 2048 bf16"] = bench_scaled_add_norm(4608, 2048)
        res["scaled_add_norm Granite-8B rows 4608 x 4096 bf16"] = bench_scaled_add_norm(4608, 4096)
    # the headline batch's rows at a Cohere 8B-class layer shape: hidden 4096, 32 x 128 heads over 8 key / value heads
    if args.only in ("", "cohere_norm"):
        res["cohere_norm rows 4608 x 4096 bf16"] = bench_cohere_norm(4608, 4096)
    if args.only in ("", "rope_il"):
        res["rope_il generator rows 18x256, 32+8 heads x 128"] = bench_rope_il(18, 256, 32, 8, 128)
        res["rope_il packed rows 1x3008, 32+8 heads x 128"] = bench_rope_il(1, 3008, 32, 8, 128)
    if args.only in ("", "add3"):
        res["add3 rows 4608 x 4096 bf16"] = bench_add3(4608, 4096)
    # the headline batch's rows in Phi-4-mini's layout: 24 + 8 heads of 128, the first 96 of each rotated
    if args.only in ("", "rope_partial"):
        res["rope_partial generator rows 18x256, 24+8 heads x 128, rot 96"] = bench_rope_partial(18, 256, 24, 8, 128, 96)
        res["rope_partial packed rows 1x3008, 24+8 heads x 128, rot 96"] = bench_rope_partial(1, 3008, 24, 8, 128, 96)
    Path("gpurun_out").mkdir(exist_ok=True)
    Path("gpurun_out/kernel_bench.json").write_text(json.dumps(res, indent=1))
    print_results(res)


if __name__ == "__main__":
    main()
