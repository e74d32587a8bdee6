"""Evaluation throughput on one MI355X at bge-large width, on the synthetic csv of tools/make_synthetic_csv.py (Question 4-12
words, Abstract 20-110 words), loaded and tokenised as the drivers do (WordLevel tokenizer: a word is a token, max_length 128):

  sweep    corpus passages/s and queries/s of the embedding sweep: padded `forward` (+ dalm_pool_l2norm_fwd) batch by batch
           against the packed sweep of dalm_amd/eval/utils.py (live tokens only + dalm_pool_l2norm_packed_fwd), both through
           `embed_dataset` on the tokenised datasets.Dataset (column read included)
  pool     the pooling step alone: `packed.retrieval_hidden`'s scatter + dalm_pool_l2norm_fwd against
           dalm_pool_l2norm_packed_fwd on the same packed rows
  search   `retrieval.evaluate_retrieval` (exact top-k + per-query Python metrics, top_k = 10) against
           `retrieval.gold_rank` + `metrics_from_rank`
  rank     one dalm_sim_gold_rank call against dalm_sim_rowstats_f32 at the same (m, n, D): the MFMA rate of the counting pass

Every number is the median of --reps (>= 20) timed repetitions after --warmup untimed ones, each timed with a pair of HIP
events on the current stream and a synchronise.  The baselines run in the same invocation, alternating with the new path.

    python tools/eval_bench.py --out eval_bench.txt
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def alternating(fns: dict, reps: int, warmup: int):
    """{name: (median, min, max) milliseconds} of every `fn()`, the variants measured in alternation (other work shares the
    host); device events around every repetition."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def synthetic_dataset(rows: int, workdir: str, max_length: int):
    """(tokenised datasets.Dataset, tokenizer): the csv of tools/make_synthetic_csv.py (Question 4-12 words, Abstract 20-110
    words over its word list) read with `load_dataset` and tokenised by `preprocess_dataset` with the WordLevel tokenizer of
    tools/trainer_bench.py - the path the evaluation drivers take."""
    from make_synthetic_csv import write_csv
    from trainer_bench import make_tokenizers

    from dalm_amd.eval.utils import preprocess_dataset
    from dalm_amd.utils import load_dataset

    path = os.path.join(workdir, "rows.csv")
    write_csv(path, rows)
    tok, _ = make_tokenizers(workdir)
    return preprocess_dataset(load_dataset(path), tok, "Question", "Abstract", max_length), tok


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", type=int, default=24, help="encoder depth (bge-large: 24)")
    ap.add_argument("--rows", type=int, default=2048, help="passages and queries of the sweep")
    ap.add_argument("--batch", type=int, default=512, help="test_batch_size (rows of the padded layout)")
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--nc", type=int, default=65536)
    ap.add_argument("--skip", default="", help="comma list of sections to skip: sweep,pool,search,rank")
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("--reps must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench.py measures on an MI355X; no GPU is visible")
    skip = set(filter(None, args.skip.split(",")))

    from transformers import BertConfig, BertModel

    from dalm_amd import packed
    from dalm_amd.eval import utils as EU
    from dalm_amd.models import AutoModelForSentenceEmbedding
    from dalm_amd.ops import default_ops
    from dalm_amd.retrieval import evaluate_retrieval, gold_rank, metrics_from_rank

    import tempfile
    import time

    dev, T, D = torch.device("cuda:0"), 128, 1024
    work = tempfile.mkdtemp(prefix="eval_bench_")
    ds, tok = synthetic_dataset(args.rows, work, T)
    V = len(tok)
    ops = default_ops()
    lines = [f"eval_bench: {torch.cuda.get_device_name(0)}, median [min .. max] of {args.reps} repetitions after {args.warmup} warm-up, "
             f"HIP events per repetition"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def fmt(t):
        return f"{t[0]:9.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]"

    p_mask = EU._column(ds, "retriever_passage_attention_mask")
    q_mask = EU._column(ds, "retriever_query_attention_mask")

    if "sweep" not in skip:
        torch.manual_seed(0)
        bert = BertModel(BertConfig(hidden_size=D, num_hidden_layers=args.layers, num_attention_heads=16, intermediate_size=4096,
                                    vocab_size=V, max_position_embeddings=512, hidden_dropout_prob=0.0,
                                    attention_probs_dropout_prob=0.0)).to(torch.bfloat16).to(dev)
        model = AutoModelForSentenceEmbedding.from_modules(bert, None, normalize=True, get_peft=False).eval()
        say(f"\n[sweep] bge-large width, {args.layers} layers, bf16, {args.rows} rows, max_length {T}, test_batch_size {args.batch}")
        for name, prefix, mask in (("passages", "retriever_passage", p_mask), ("queries", "retriever_query", q_mask)):
            live = float(mask.sum()) / mask.numel()

            def padded():
                # the path the parent commit has: padded forward (+ dalm_pool_l2norm_fwd) batch by batch; column read and result
                # tensor are the same code as the packed sweep's
                return EU.embed_dataset(ds, prefix, model.forward, "cuda:0", torch.bfloat16, args.batch, packed_sweep=False)

            def sweep():
                return EU.embed_dataset(ds, prefix, model.forward, "cuda:0", torch.bfloat16, args.batch, packed_sweep=True)

            a, b = padded(), sweep()
            dist = float((a - b).norm(dim=1).max())
            t = alternating({"padded": padded, "packed": sweep}, args.reps, args.warmup)
            t0 = time.perf_counter()
            ids_h, mask_h = EU._column(ds, f"{prefix}_input_ids"), EU._column(ds, f"{prefix}_attention_mask")
            t_read = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            order, cuts = EU.token_budget_batches(mask_h.sum(dim=1), args.batch * T)
            for lo, hi in cuts:
                packed.pack_plan(mask_h[order[lo:hi]], shifted=False)
            t_plan = (time.perf_counter() - t0) * 1e3
            say(f"  {name:8s} live tokens {live:5.1%}   padded forward {fmt(t['padded'])} = {args.rows / t['padded'][0] * 1e3:9.0f} rows/s"
                f"   packed sweep {fmt(t['packed'])} = {args.rows / t['packed'][0] * 1e3:9.0f} rows/s"
                f"   time ratio {t['packed'][0] / t['padded'][0]:.3f}   max row L2 distance between the two {dist:.2e}")
            say(f"           host work inside both: dataset column read {t_read:.1f} ms; inside the packed sweep only: sort + "
                f"{len(cuts)} pack plans {t_plan:.1f} ms (host clock, one pass)")
        del model, bert
        torch.cuda.empty_cache()

    if "pool" not in skip:
        say(f"\n[pool] pooling alone, bf16 token states of width {D}")
        for name, mask, B in (("passages", p_mask, min(512, args.rows)), ("queries", q_mask, args.rows)):
            mask_b = mask[:B]
            rows, cu = packed.pack_plan(mask_b, shifted=False)
            n = int(rows.numel())
            h = torch.randn(n, D, device=dev).to(torch.bfloat16)
            rows_d, cu_d, mask_d = rows.to(dev), cu.to(dev), mask_b.to(dev)
            valid = rows_d >= 0
            dst = torch.where(valid, rows_d, torch.full_like(rows_d, B * T))
            out = torch.empty((B, D), device=dev)

            def scatter_pool():       # packed.retrieval_hidden's scatter into the padded layout + the padded kernel
                full = h.new_zeros((B * T + 1, D)).index_copy(0, dst, h)
                return ops.pool_fwd(full[:B * T].view(B, T, D), mask_d, True)[0]

            def packed_pool():
                return ops.pool_packed_fwd(h, cu_d, nseq_out=B, out=out)

            diff = float((scatter_pool() - packed_pool()).abs().max())
            t = alternating({"scatter": scatter_pool, "packed": packed_pool}, max(args.reps, 50), args.warmup + 3)
            live_bytes = int(mask_b.sum()) * D * 2 + B * D * 4
            say(f"  {name:8s} B {B:5d}, {n:7d} packed rows   scatter + dalm_pool_l2norm_fwd {fmt(t['scatter'])}"
                f"   dalm_pool_l2norm_packed_fwd {fmt(t['packed'])} = {live_bytes / t['packed'][0] / 1e6:7.1f} GB/s of live bytes"
                f"   ratio {t['packed'][0] / t['scatter'][0]:.3f}   max abs difference {diff:.1e}")

    g = torch.Generator().manual_seed(3)
    F = torch.nn.functional
    if "search" not in skip or "rank" not in skip:
        C = F.normalize(torch.randn(args.nc, D, generator=g), dim=1)
        gold = torch.randint(args.nc, (args.nq,), generator=g)
        Q = F.normalize(0.10 * C[gold] + F.normalize(torch.randn(args.nq, D, generator=g), dim=1), dim=1)
        Cd, Qd, gd = C.to(dev), Q.to(dev), gold.to(dev)

    if "search" not in skip:
        say(f"\n[search] {args.nq} queries x {args.nc} passages, D {D}, metrics at top_k 10, end to end (host metric code included)")

        def topk_metrics():
            return evaluate_retrieval(Qd, Cd, gd, top_k=10)

        def rank_metrics():
            rank, n_ge, _ = gold_rank(Qd, Cd, gd)
            return metrics_from_rank(rank.cpu(), n_ge.cpu(), [1, 5, 10, 20, 50, 100])

        m_old, m_new = topk_metrics(), rank_metrics()
        at10 = [m for m in m_new if m["top_k"] == 10][0]
        t = alternating({"topk": topk_metrics, "rank": rank_metrics}, args.reps, args.warmup)
        say(f"  evaluate_retrieval (exact_topk + Python loop) {fmt(t['topk'])}   gold_rank + metrics_from_rank (6 values of k) {fmt(t['rank'])}"
            f"   ratio {t['rank'][0] / t['topk'][0]:.3f}")
        say(f"  recall@10 {m_old['recall']:.6f} vs {at10['recall']:.6f}, precision {m_old['precision']:.6f} vs {at10['precision']:.6f}")

    if "rank" not in skip:
        say(f"\n[rank] one call at m {args.nq}, n {args.nc}, D {D} (k-major copies of both operands included in both)")
        score = torch.full((args.nq,), float("-inf"), device=dev)
        ops.sim_gold_score(Qd, Cd, gd, 0, score)
        rank = torch.zeros((args.nq,), device=dev, dtype=torch.int64)
        n_ge = torch.zeros_like(rank)
        flop = 2.0 * args.nq * args.nc * D
        t = alternating({"rowstats": lambda: ops.sim_rowstats_f32(Qd, Cd, 1.0, 0),
                         "rank": lambda: ops.sim_gold_rank(Qd, Cd, gd, score, 0, 0.0, rank, n_ge),
                         "score": lambda: ops.sim_gold_score(Qd, Cd, gd, 0, score)}, args.reps, args.warmup)
        say(f"  dalm_sim_rowstats_f32 {fmt(t['rowstats'])} = {flop / t['rowstats'][0] / 1e9:6.1f} TF/s"
            f"   dalm_sim_gold_rank {fmt(t['rank'])} = {flop / t['rank'][0] / 1e9:6.1f} TF/s   ratio {t['rank'][0] / t['rowstats'][0]:.3f}"
            f"   dalm_sim_gold_score (prepass) {fmt(t['score'])}")

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
