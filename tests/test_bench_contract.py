"""bench.py contract checks: flags, defaults, workload shapes, JSON keys it promises (one GPU test runs it at depth 1)."""
import ast
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def test_bench_flags_and_defaults():
    src = (ROOT / "bench.py").read_text()
    tree = ast.parse(src)
    flags = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "add_argument" and node.args:
            name = node.args[0].value
            default = next((ast.literal_eval(k.value) for k in node.keywords if k.arg == "default"), None)
            flags[name] = default
    assert flags["--gpus"] == 1 and flags["--steps"] == 10 and flags["--warmup"] == 3
    assert "--full" in flags and flags["--full"] is None      # store_true: off unless asked for
    for key in ('"metric"', '"value"', '"unit"', '"n_gpus"', '"steps"', '"warmup"', '"ms_per_step"', '"higher_is_better"',
                '"scaling"', '"vs_baseline"', '"dtype"', '"data"', '"config"', '"roofline"', '"cpu_baseline"',
                '"bound"', '"achieved"', '"peak"', '"frac"', '"traffic"', '"cores"', '"kind"', '"sample"'):
        assert key in src, key


def _full_polarity(test):
    """(+1 if `args.full` appears in the condition, -1 if it appears under a `not`, 0 if it does not appear)."""
    found = 0

    def walk(node, negated):
        nonlocal found
        if isinstance(node, ast.Attribute) and node.attr == "full" and getattr(node.value, "id", None) == "args":
            found = -1 if negated else 1
            return
        neg = negated ^ (isinstance(node, ast.UnaryOp) and isinstance(node.op, ast.Not))
        for child in ast.iter_child_nodes(node):
            walk(child, neg)

    walk(test, False)
    return found


def test_plain_run_leaves_the_extra_measurements_to_full():
    """A plain `bench.py` run does only what its headline line needs: every probe, PMC pass, CPU baseline and the eager steps
    after a whole-step graph are reached only through a branch that `--full` opens."""
    tree = ast.parse((ROOT / "bench.py").read_text())
    main = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "main")
    extras = {"collect_ce_traffic", "gpu_loss_path_probe", "ce_back_to_back_probe", "f1_head_paths", "cpu_reference_baseline",
              "cpu_loss_path_baseline"}
    seen = []

    def visit(node, guarded):
        if isinstance(node, ast.Call):
            f = node.func
            name = f.id if isinstance(f, ast.Name) else (f"{getattr(f.value, 'id', '')}.{f.attr}" if isinstance(f, ast.Attribute) else "")
            if name in extras or name == "step.step":
                seen.append((name, node.lineno, guarded))
        if isinstance(node, ast.If):
            pol = _full_polarity(node.test)
            visit(node.test, guarded)
            for child in node.body:
                visit(child, guarded or pol > 0)
            for child in node.orelse:
                visit(child, guarded or pol < 0)
            return
        for child in ast.iter_child_nodes(node):
            visit(child, guarded)

    visit(main, False)
    assert {n for n, _, _ in seen} == extras | {"step.step"}, seen
    assert all(g for _, _, g in seen), [s for s in seen if not s[2]]


def test_synthetic_batch_matches_cfg3_shapes():
    import bench

    b = bench.synthetic_batch(torch.device("cpu"), 0)
    assert b["retriever_query_input_ids"].shape == (18, 50)
    assert b["retriever_passage_input_ids"].shape == (18, 128)
    assert b["generator_input_input_ids"].shape == (18, 256)
    assert b["query_passage_input_len"].shape == (18,) and b["query_passage_input_len"].dtype == torch.int64
    m = b["generator_input_attention_mask"]
    assert int(m[:, -1].min()) == 1 and 60 <= int(m.sum(1).min())   # left-padded, 60..256 live tokens
    assert abs(bench.A100_README_PAIRS_PER_S - 7.9365) < 1e-3
    assert bench.HBM_PEAK_GBPS == 8000.0


def test_bench_self_spawns_and_refuses_clearly_without_enough_gpus():
    """`python bench.py --gpus N` (the driver's form, no torchrun): bench.py spawns the ranks itself; on a box with
    fewer GPUs it says so and exits 2 instead of hanging or dying in rendezvous."""
    import os
    import subprocess

    if torch.cuda.is_available() and torch.cuda.device_count() >= 8:
        return
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "8", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 2, (r.returncode, r.stderr[-400:])
    assert "8 ranks requested but only" in r.stderr and "GPU(s) are visible" in r.stderr
    assert r.stdout.strip() == ""                                   # no JSON line pretending to be a result


def test_bench_workloads_and_cfg5_shapes():
    import bench

    src = (ROOT / "bench.py").read_text()
    for w in ('"cfg3"', '"cfg5"', '"cfg2"', '"cfg1"', '"--dtype"', '"fp32"', "ranks_seen_by_process_group", "traffic_source"):
        assert w in src, w
    assert bench.GENERATORS["falcon-7b"][1] == 65024 and bench.GENERATORS["llama-2-7b"][1] == 32000
    fc = bench.GENERATORS["falcon-7b"][0](32)
    assert (fc.hidden_size, fc.num_hidden_layers, fc.num_attention_heads, fc.vocab_size) == (4544, 32, 71, 65024)
    lc = bench.GENERATORS["llama-2-7b"][0](32)
    assert (lc.hidden_size, lc.num_hidden_layers, lc.intermediate_size, lc.vocab_size) == (4096, 32, 11008, 32000)
    b = bench.synthetic_batch(torch.device("cpu"), 0, V=65024)
    assert int(b["generator_input_input_ids"].max()) > 32000 and int(b["generator_input_input_ids"].max()) < 65024
    # a tiny cfg5-architecture model assembles (LoRA lands on Falcon's fused query_key_value)
    m = bench.build_models(torch.device("cpu"), torch.float32, bert_layers=1, llama_layers=1, generator="falcon-7b")
    assert m.generator_model._dalm_lora_config["target_modules"] == ["query_key_value"]


def test_bucketed_data_path_is_opt_in_and_keeps_every_row():
    """--data-path bucketed (an extra line, never the default): batches of B rows, trimmed widths that vary with the bucket,
    no live token lost, and fewer generator tokens than the fixed-shape batches."""
    import bench

    src = (ROOT / "bench.py").read_text()
    assert 'ap.add_argument("--data-path", default="fixed"' in src
    bs = bench.bucketed_batches(torch.device("cpu"), 100, 32000, n_batches=6)
    pool = [bench.synthetic_batch(torch.device("cpu"), 100 + i, V=32000) for i in range(6)]
    live_in = sum(int(b["generator_input_attention_mask"].sum()) for b in pool)
    live_out = sum(int(b["generator_input_attention_mask"].sum()) for b in bs)
    assert live_in == live_out
    widths = {b["generator_input_input_ids"].shape[1] for b in bs}
    assert all(b["generator_input_input_ids"].shape[0] == bench.CFG["B"] for b in bs) and len(widths) > 1
    assert sum(b["generator_input_input_ids"].numel() for b in bs) < 0.85 * 6 * bench.CFG["B"] * bench.CFG["Tg"]


def test_kernel_bench_printer_takes_label_values(capsys):
    """tools/kernel_bench.py crashed in round 5 formatting the string "bf16 x3" with :.4g."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("kernel_bench", ROOT / "tools" / "kernel_bench.py")
    kb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kb)
    kb.print_results({"sim 4096x4096 D1024": {"rowstats": {"s": 1.25e-4, "pipe": "bf16 x3", "frac": 0.47, "n": 3}}})
    out = capsys.readouterr().out
    assert "pipe=bf16 x3" in out and "frac=0.47" in out


def test_dump_outputs_writes_loss_and_trainable_parameters(tmp_path, monkeypatch):
    """--dump-outputs DIR: loss.npy (float64) and one float32 .npy per trainable parameter; above the byte budget every
    parameter keeps the same seeded sample, so two runs compare element for element."""
    import numpy as np

    import bench

    src = (ROOT / "bench.py").read_text()
    assert '"--dump-outputs"' in src
    m = bench.build_models(torch.device("cpu"), torch.float32, bert_layers=1, llama_layers=1)
    trainable = {n: p for n, p in m.named_parameters() if p.requires_grad}
    bench.dump_outputs(tmp_path / "full", torch.tensor(2.5), m)
    loss = np.load(tmp_path / "full" / "loss.npy")
    assert loss.dtype == np.float64 and loss.tolist() == [2.5]
    for n, p in trainable.items():
        a = np.load(tmp_path / "full" / f"param.{n}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, p.detach().numpy())
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1 << 16)
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, torch.tensor(2.5), m)
    sampled = sum(np.load(f).nbytes for f in (tmp_path / "a").glob("param.*.npy"))
    assert 0 < sampled <= 1 << 16
    for n in trainable:
        assert np.array_equal(np.load(tmp_path / "a" / f"param.{n}.npy"), np.load(tmp_path / "b" / f"param.{n}.npy"))


# runs bench.py as __main__ after registering an exit handler that writes the process's memory map to a file
_EXIT_PROBE = ("import atexit, runpy, sys\n"
               "out = sys.argv[1]\n"
               "atexit.register(lambda: open(out, 'w').write(open('/proc/self/maps').read()))\n"
               "sys.argv = sys.argv[2:]\n"
               "runpy.run_path(sys.argv[0], run_name='__main__')\n")


def _bench_line(maps_file, *extra):
    """(the JSON line, the process's memory map as its exit handlers saw it - None if they never ran)."""
    import json
    import subprocess

    cmd = [sys.executable, "-c", _EXIT_PROBE, str(maps_file), str(ROOT / "bench.py"), "--steps", "2", "--warmup", "1",
           "--retriever-layers", "1", "--generator-layers", "1", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1]), (maps_file.read_text() if maps_file.exists() else None)


@pytest.mark.gpu
def test_plain_and_full_runs_on_gpu(tmp_path):
    """Depth-1 towers: a plain run prints the headline line without the extra measurements; `--full` adds them after the same
    timed steps, which compute the same loss.  Both end through the interpreter's normal shutdown, with this library's HIP
    code loaded: exit handlers (profilers, TunableOp) see the whole run."""
    import math

    plain, maps = _bench_line(tmp_path / "plain_maps.txt")
    assert maps is not None and "libdalm_hip.so" in maps
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in plain, key
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["higher_is_better"] is True
    for key in ("cpu_baseline", "parity", "loss_path", "f1_lm_head_paths"):
        assert key not in plain, key
    roof = plain["roofline"]
    assert roof["traffic"] is None and roof["loss_path_us"] is None and roof["back_to_back_us"] is None
    assert roof["avg_launch_us"] > 0          # HIP events around the CE launch inside the timed steps

    full, maps = _bench_line(tmp_path / "full_maps.txt", "--full", "--no-cpu-baseline", "--no-pmc")
    assert maps is not None and "libdalm_hip.so" in maps
    assert full["roofline"]["loss_path_us"] > 0 and full["roofline"]["back_to_back_us"] > 0
    assert math.isfinite(plain["config"]["final_loss"]) and full["config"]["final_loss"] == plain["config"]["final_loss"]
