"""Kernel bench of `dalm_linear_live` against the tuned library GEMMs at the padded cfg3 step's generator shapes.

    python tools/linear_live_bench.py [--out profiles/linear_live_bench.txt] [--quick]
    python tools/linear_live_bench.py --mlp-fused [--out profiles/mlp_fused_bench.txt]
    python tools/linear_live_bench.py --candidates --out FILE

The seven GEMMs of one Llama-2-7b layer and the two of the materialised lm_head at R = 4608 padded rows (18 x 256), each with
  * every row live, and the four masks of `bench.synthetic_batch(dev, 100 + i)` under the generator's shifted rule;
  * two arms: the kernel, and `F.linear` / `addmm_` through the tuned solution table.
Every arm is timed inside a hipGraph of LAUNCHES (>= 20) launches, over a ring of weight copies larger than the Infinity Cache
(in the step every layer brings its own weights from HBM); the median of 5 replays is taken and the spread (max - min) printed.
FLOP are counted over LIVE rows (2 live N K), `frac` is against the bf16 MFMA peak - for the library arm too, so its frac at a
padded mask shows what the padding costs.  `win` marks a kernel arm faster than the library arm by more than three times the
larger of the two spreads: the routing table in dalm_amd/linear_live.py lists exactly those shapes.

--mlp-fused: the fused forward of the frozen MLP node against the pair of launches it replaces, same protocol and same rule -
  forward   {dalm_linear_live gate|up + dalm_swiglu_fwd_2d_live}   against dalm_linear_live_swiglu
at the four batch masks.  It ships only if it beats its pair by more than three times the larger spread at EVERY mask.

--candidates: the two GEMM shapes of an AFM-4.5B layer's ungated MLP (hidden 2560, intermediate 18432) under the same protocol and
the same rule - they enter ROUTED_SHAPES only if the kernel clears the library arm at every batch mask, in every run - and the fused
up forward of the ReLU^2 node, {dalm_linear_live up + dalm_relu2_fwd} against dalm_linear_live_relu2.  The solution table was tuned
at Llama-2-7b's shapes: at these the library arm runs the library's own choice.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from dalm_amd import linear_live, live_rows  # noqa: E402

BF16_PEAK = 2.5e15          # dense bf16 MFMA peak of the MI355X, FLOP/s
R = 4608
LAUNCHES = 20
REPLAYS = 5
RING_BYTES = 512 << 20

# name, (N, K) of every accumulated member, A as column halves of one buffer
GEMMS = [
    ("o_proj fwd / o dgrad", [(4096, 4096)], False),
    ("q|k|v fwd", [(12288, 4096)], False),
    ("q|k|v dgrad (3 accumulated)", [(4096, 4096)] * 3, False),
    ("gate|up fwd", [(22016, 4096)], False),
    ("gate + up dgrad (2 accumulated)", [(4096, 11008)] * 2, True),
    ("down fwd", [(4096, 11008)], False),
    ("down dgrad", [(11008, 4096)], False),
    ("lm_head fwd (materialised logits)", [(32000, 4096)], False),
    ("lm_head dgrad", [(4096, 32000)], False),
]

# shapes measured for the table but not (yet) in it: AFM-4.5B's MLP, hidden 2560, intermediate 18432, no gate
CANDIDATES = [
    ("AFM up fwd / down dgrad", [(18432, 2560)], False),
    ("AFM down fwd / up dgrad", [(2560, 18432)], False),
]


def masks(dev):
    import bench

    out = [("all live", torch.ones(R, dtype=torch.uint8, device=dev))]
    for i in range(4):
        m = bench.synthetic_batch(dev, 100 + i)["generator_input_attention_mask"]
        out.append((f"batch {100 + i}", live_rows.live_rows(m, shifted=True)))
    return out


def time_graph(fn):
    """fn(i) = launch number i.  (median, spread) seconds per launch over REPLAYS replays of a graph of LAUNCHES launches."""
    for i in range(2):
        fn(i)
    torch.cuda.synchronize()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            for i in range(LAUNCHES):
                fn(i)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPLAYS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3 / LAUNCHES)
    ts.sort()
    return ts[len(ts) // 2], ts[-1] - ts[0]


def bench_gemm(members, halves, mask_list, dev, emit):
    n, k = members[0]
    nm = len(members)
    gen = torch.Generator(device=dev).manual_seed(7)
    ring = max(2, min(LAUNCHES, RING_BYTES // (nm * n * k * 2) + 1))
    ws = [[(torch.randn(n, k, device=dev, generator=gen) * 0.02).bfloat16() for _ in range(nm)] for _ in range(ring)]
    if halves:
        buf = torch.randn(R, nm * k, device=dev, generator=gen).bfloat16()
        xs = [buf[:, j * k:(j + 1) * k] for j in range(nm)]
    else:
        xs = [torch.randn(R, k, device=dev, generator=gen).bfloat16() for _ in range(nm)]
    out = torch.empty(R, n, dtype=torch.bfloat16, device=dev)
    rows = []
    for mname, vec in mask_list:
        part = linear_live.row_partition(vec)
        n_live = int(part[1].item())

        def lib(i):
            w = ws[i % ring]
            y = F.linear(xs[0], w[0])
            for j in range(1, nm):
                y.addmm_(xs[j], w[j].t())

        def kern(i):
            w = ws[i % ring]
            for j in range(nm):
                linear_live.linear_live(xs[j], w[j], part, out=out, accumulate=j > 0)

        fl = nm * linear_live.flops(n_live, n, k)
        res = {"library": time_graph(lib), "kernel": time_graph(kern)}
        lt, ls = res["library"]
        for arm, (t, sp) in res.items():
            win = ""
            if arm != "library":
                win = "win" if lt - t > 3 * max(sp, ls) else "-"
            emit(f"  {mname:10s} live {n_live:5d}  {arm:11s} {t * 1e6:8.1f} us  spread {sp * 1e6:6.1f} us  "
                 f"{fl / t / 1e12:7.1f} TF/s  frac {fl / t / BF16_PEAK:5.3f}  "
                 f"tiles {linear_live.tiles(n_live, n):5d}  {win}")
        rows.append((mname, res))
    return rows


def bench_mlp_fused(mask_list, dev, emit, c=11008, h=4096):
    """The paired arms of the fused MLP node's forward; returns {piece: ships?}."""
    from dalm_amd import hip

    gen = torch.Generator(device=dev).manual_seed(11)
    ring_f = max(2, min(LAUNCHES, RING_BYTES // (2 * c * h * 2) + 1))
    wcat = [(torch.randn(2 * c, h, device=dev, generator=gen) * 0.02).bfloat16() for _ in range(ring_f)]
    x = torch.randn(R, h, device=dev, generator=gen).bfloat16()
    y = torch.zeros(R, 2 * c, dtype=torch.bfloat16, device=dev)
    act = torch.zeros(R, c, dtype=torch.bfloat16, device=dev)
    dt = hip.dtype_code(y)
    ships = {"forward": True}
    for mname, vec in mask_list:
        part = linear_live.row_partition(vec)
        n_live = int(part[1].item())
        perm, nl = hip.ptr(part[0]), hip.ptr(part[1])

        def fwd_pair(i):
            linear_live.linear_live(x, wcat[i % ring_f], part, out=y)
            hip.call("dalm_swiglu_fwd_2d_live", hip.ptr(y), hip.ptr(y[:, c:]), hip.ptr(act), dt, R, c, 2 * c, 2 * c, c, hip.ptr(vec),
                     hip.stream())

        def fwd_fused(i):
            hip.call("dalm_linear_live_swiglu", hip.ptr(x), h, hip.ptr(wcat[i % ring_f]), hip.ptr(y), 2 * c, hip.ptr(act), c, R, c, h,
                     perm, nl, hip.stream())

        for piece, pair, fused, n in (("forward", fwd_pair, fwd_fused, 2 * c),):
            (tp, sp), (tf, sf) = time_graph(pair), time_graph(fused)
            win = tp - tf > 3 * max(sp, sf)
            ships[piece] = ships[piece] and (win or mname == "all live")
            fl = linear_live.flops(n_live, n, h)
            emit(f"  {mname:10s} live {n_live:5d}  {piece:8s} pair {tp * 1e6:8.1f} us (spread {sp * 1e6:5.1f})  fused {tf * 1e6:8.1f} us "
                 f"(spread {sf * 1e6:5.1f})  saves {(tp - tf) * 1e6:7.1f} us  fused {fl / tf / 1e12:7.1f} TF/s  {'win' if win else '-'}")
    return ships


def bench_relu2_fused(mask_list, dev, emit, c=18432, h=2560):
    """The paired arms of the ReLU^2 node's forward; returns whether the fused one clears its pair at every batch mask."""
    from dalm_amd import hip

    gen = torch.Generator(device=dev).manual_seed(13)
    ring = max(2, min(LAUNCHES, RING_BYTES // (c * h * 2) + 1))
    wup = [(torch.randn(c, h, device=dev, generator=gen) * 0.02).bfloat16() for _ in range(ring)]
    x = torch.randn(R, h, device=dev, generator=gen).bfloat16()
    y = torch.zeros(R, c, dtype=torch.bfloat16, device=dev)
    act = torch.zeros(R, c, dtype=torch.bfloat16, device=dev)
    dt = hip.dtype_code(y)
    ships = True
    for mname, vec in mask_list:
        part = linear_live.row_partition(vec)
        n_live = int(part[1].item())
        perm, nl = hip.ptr(part[0]), hip.ptr(part[1])

        def pair(i):
            linear_live.linear_live(x, wup[i % ring], part, out=y)
            hip.call("dalm_relu2_fwd", hip.ptr(y), hip.ptr(act), dt, R, c, c, c, hip.ptr(vec), hip.stream())

        def fused(i):
            hip.call("dalm_linear_live_relu2", hip.ptr(x), h, hip.ptr(wup[i % ring]), hip.ptr(y), c, hip.ptr(act), c, R, c, h, perm, nl,
                     hip.stream())

        (tp, sp), (tf, sf) = time_graph(pair), time_graph(fused)
        win = tp - tf > 3 * max(sp, sf)
        ships = ships and (win or mname == "all live")
        fl = linear_live.flops(n_live, c, h)
        emit(f"  {mname:10s} live {n_live:5d}  forward  pair {tp * 1e6:8.1f} us (spread {sp * 1e6:5.1f})  fused {tf * 1e6:8.1f} us "
             f"(spread {sf * 1e6:5.1f})  saves {(tp - tf) * 1e6:7.1f} us  fused {fl / tf / 1e12:7.1f} TF/s  {'win' if win else '-'}")
    return ships


def main_mlp_fused(args, dev, emit, lines):
    ml = masks(dev)
    emit("mlp_fused: {dalm_linear_live + dalm_swiglu_*_2d_live} against the fused entry point, C = 11008, H = 4096")
    ships = bench_mlp_fused(ml, dev, emit)
    emit("verdict (fused faster than its pair by > 3 x the larger spread, at all four batch masks):")
    for piece, ok in ships.items():
        emit(f"  {piece:8s}: {'ships' if ok else 'does NOT clear the rule: the node keeps the unfused kernels for this direction'}")
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--mlp-fused", action="store_true", help="the paired arms of the fused MLP node only")
    ap.add_argument("--candidates", action="store_true", help="the AFM-4.5B MLP shapes (not in the table) and the ReLU^2 node's forward")
    ap.add_argument("--quick", action="store_true", help="all-live and one batch mask only")
    args = ap.parse_args()
    if args.candidates and args.out is None:
        ap.error("--candidates needs --out: it does not replace a committed profile")
    if args.out is None:
        args.out = str(ROOT / "profiles" / ("mlp_fused_bench.txt" if args.mlp_fused else "linear_live_bench.txt"))
    if not torch.cuda.is_available():
        raise SystemExit("linear_live_bench needs the GPU: there is no CPU timing of a HIP kernel")
    dev = torch.device("cuda")
    from dalm_amd.tuning import enable_tuned_gemms

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"linear_live_bench: R = {R}, graph of {LAUNCHES} launches, median of {REPLAYS} replays, "
         f"weights rotate over a ring > {RING_BYTES >> 20} MB; tuned GEMM table loaded: {enable_tuned_gemms()}")
    emit(f"device: {torch.cuda.get_device_name(0)}; bf16 peak taken as {BF16_PEAK / 1e12:.0f} TF/s; FLOP over live rows")
    warm = torch.randn(4096, 4096, device=dev).bfloat16()
    for _ in range(300):                                   # clocks up before the first timed arm
        warm = F.linear(warm, warm) * 0.01
    torch.cuda.synchronize()
    if args.mlp_fused:
        return main_mlp_fused(args, dev, emit, lines)
    ml = masks(dev)
    if args.quick:
        ml = ml[:2]
    verdict = []
    for name, members, halves in (CANDIDATES if args.candidates else GEMMS):
        n, k = members[0]
        emit(f"{name}: N = {n}, K = {k}, members {len(members)}, routed now: "
             f"{'kernel' if (R, n, k) in linear_live.ROUTED_SHAPES else 'library'}")
        rows = bench_gemm(members, halves, ml, dev, emit)
        # a shape is routed when the kernel wins at EVERY batch mask (the all-live line is the no-padding reference)
        ok = all(res["library"][0] - res["kernel"][0] > 3 * max(res["kernel"][1], res["library"][1]) for m, res in rows if m != "all live")
        verdict.append(f"  {name:34s} kernel: {'clears the library at every batch mask' if ok else 'does not clear'}")
    emit("verdict (faster than the library arm by > 3 x the larger spread, at all batch masks):")
    for v in verdict:
        emit(v)
    if args.candidates:
        emit("relu2 node forward: {dalm_linear_live up + dalm_relu2_fwd} against dalm_linear_live_relu2, C = 18432, H = 2560")
        ok = bench_relu2_fused(ml, dev, emit)
        emit(f"  fused forward: {'clears its pair at every batch mask' if ok else 'does not clear its pair at every batch mask'}")
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
