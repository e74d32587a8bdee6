"""`dalm`-style command line for the two trainers and the two evaluation drivers on the MI355X path (typer), mirroring the
argument surface of the reference's `dalm train-rag-e2e` / `dalm train-retriever-only` / `dalm eval-rag` / `dalm eval-retriever`
(dalm/cli.py:41-167, 170-277, 312-412): the same positional arguments, the same option names and defaults.

    python -m dalm_amd.cli train-rag-e2e rows.csv BAAI/bge-large-en meta-llama/Llama-2-7b-hf --use-peft both
    python -m dalm_amd.cli train-retriever-only BAAI/bge-large-en rows.csv --per-device-train-batch-size 150
    python -m dalm_amd.cli eval-retriever rows.csv --retriever-name-or-path BAAI/bge-large-en --torch-dtype bfloat16
    python -m dalm_amd.cli eval-rag rows.csv --retriever-name-or-path BAAI/bge-large-en --generator-name-or-path meta-llama/Llama-2-7b-hf

The qa-gen command of the reference is not part of this package.
The commands are generated from the functions' own signatures, so the CLI cannot drift from them.
"""
from __future__ import annotations

import inspect
from enum import Enum
from typing import Optional

import typer

from . import __version__ as _v  # noqa: F401
from .models.rag_e2e_base_model import Mode


class DALMSchedulerType(str, Enum):
    LINEAR = "linear"
    COSINE = "cosine"
    COSINE_WITH_RESTARTS = "cosine_with_restarts"
    POLYNOMIAL = "polynomial"
    CONSTANT = "constant"
    CONSTANT_WITH_WARMUP = "constant_with_warmup"


cli = typer.Typer(add_completion=False, help="MI355X-native RAG-end2end / retriever-only training (DALM surface)")

_HELP = {
    "dataset_or_path": "Path to the dataset to train with: an hf dataset dir or a csv file.",
    "retriever_name_or_path": "Path to pretrained retriever or identifier from huggingface.co/models.",
    "generator_name_or_path": "Path to pretrained (causal) generator or identifier from huggingface.co/models.",
    "per_device_train_batch_size": "Batch size (per device).",
    "logit_scale": "Logit scale of the contrastive loss.",
    "use_peft": "LoRA fine-tuning (which tower(s)).",
    "use_bnb": "nf4 storage of the frozen base weights (HIP kernels; needs the GPU).",
    "checkpointing_steps": "Save state every n steps, or 'epoch'.",
    "no_hip_graph": "Launch every step eagerly instead of replaying a hipGraph.",
    "retriever_peft_model_path": "Path to the fine-tuned retriever peft layers (omit to evaluate the base weights).",
    "generator_peft_model_path": "Path to the fine-tuned generator peft layers (omit to evaluate the base weights).",
    "passage_column_name": "Name of the column containing the passage",
    "query_column_name": "Name of the column containing the query",
    "answer_column_name": "Name of the column containing the Answer",
    "embed_dim": "Dimension of the model embedding",
    "max_length": "The max passage sequence length during tokenization. Longer sequences are truncated",
    "test_batch_size": "Batch size in rows of the padded layout; the packed sweep spends test_batch_size * max_length live tokens per batch.",
    "query_batch_size": "Batch size for generator input",
    "device": "Device. cpu or cuda.",
    "torch_dtype": "Autocast dtype: float16 (the reference's default), bfloat16 or float32.",
    "packed_sweep": "Embed on the live tokens only (bfloat16 encoder retrievers only); off unless asked for.",
    "top_k": "Top K retrieval",
    "evaluate_generator": "Enable generator evaluation. If false, equivalent to eval-retriever",
    "retriever_is_autoregressive": "Whether the retriever is autoregressive.",
    "is_autoregressive": "Whether the model is autoregressive.",
}
_SKIP = {"rag_model", "model", "on_step", "report"}
# what the reference's eval commands default on the command line where the functions themselves require a value (dalm/cli.py:329-335)
_EVAL_DEFAULTS = {"passage_column_name": "Abstract", "query_column_name": "Question", "answer_column_name": "Answer",
                  "embed_dim": 1024, "max_length": 128}


def _cli_type(name: str, default):
    if name == "lr_scheduler_type":
        return "DALMSchedulerType", "DALMSchedulerType.LINEAR"
    if name in ("use_peft", "use_bnb") and not isinstance(default, bool):
        return "Optional[Mode]", "None"
    if name == "packed_sweep":
        return "Optional[bool]", "None"
    if name == "checkpointing_steps":
        return "Optional[str]", "None"
    if isinstance(default, bool):
        return "bool", repr(default)
    if isinstance(default, int):
        return "int", repr(default)
    if isinstance(default, float):
        return "float", repr(default)
    if isinstance(default, str):
        return "str", repr(default)
    if name in ("max_train_steps",):
        return "Optional[int]", "None"
    return "Optional[str]", "None"


def _make_command(fn, positional, cmd_name, defaults=None, required=()):
    """`defaults`: command-line defaults for parameters the function requires; `required`: options without a default."""
    sig = inspect.signature(fn)
    defaults = defaults or {}
    params, call = [], []
    for name in positional:  # positional CLI arguments, in the reference's order
        cli_name = "dataset_path" if name == "dataset_or_path" else name
        params.append(f'{cli_name}: str = typer.Argument(..., help={_HELP.get(name, name)!r}, show_default=False)')
        call.append(f"{name}={cli_name}")
    for name, p in sig.parameters.items():
        if name in positional or name in _SKIP:
            continue
        if name in required:
            params.append(f"{name}: str = typer.Option(..., help={_HELP.get(name, name.replace('_', ' '))!r})")
            call.append(f"{name}={name}")
            continue
        t, d = _cli_type(name, defaults.get(name, p.default))
        params.append(f"{name}: {t} = typer.Option({d}, help={_HELP.get(name, name.replace('_', ' '))!r})")
        if name == "lr_scheduler_type":
            call.append(f"{name}={name}.value")
        else:
            call.append(f"{name}={name}")
    src = f"def {cmd_name}(\n    " + ",\n    ".join(params) + f"\n) -> None:\n    _fn({', '.join(call)})\n"
    ns = {"typer": typer, "Optional": Optional, "Mode": Mode, "DALMSchedulerType": DALMSchedulerType, "_fn": fn}
    exec(src, ns)  # the signature typer introspects is built from the trainer's own signature
    ns[cmd_name].__doc__ = (fn.__doc__ or "").strip() or f"{cmd_name.replace('_', '-')} on MI355X"
    return ns[cmd_name]


@cli.command()
def version() -> None:
    """Print the version of this package."""
    from . import __version__

    print(f"dalm_amd version: {__version__}")


def _register() -> None:
    from .training.rag_e2e.train_rage2e import train_e2e
    from .training.retriever_only.train_retriever_only import train_retriever

    cli.command(name="train-rag-e2e")(_make_command(
        train_e2e, ["dataset_or_path", "retriever_name_or_path", "generator_name_or_path"], "train_rag_e2e"))
    cli.command(name="train-retriever-only")(_make_command(
        train_retriever, ["retriever_name_or_path", "dataset_or_path"], "train_retriever_only"))
    from .eval.eval_rag import evaluate_rag
    from .eval.eval_retriever_only import evaluate_retriever

    cli.command(name="eval-rag")(_make_command(
        evaluate_rag, ["dataset_or_path"], "eval_rag", _EVAL_DEFAULTS, ("retriever_name_or_path", "generator_name_or_path")))
    cli.command(name="eval-retriever")(_make_command(
        evaluate_retriever, ["dataset_or_path"], "eval_retriever", _EVAL_DEFAULTS, ("retriever_name_or_path",)))


_register()

if __name__ == "__main__":
    cli()
