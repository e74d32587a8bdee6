"""C-ABI surface checks that need no GPU: the library loads, exports every symbol the header
declares, the ctypes table matches the header, and the product refuses CPU tensors loudly."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "dalm_hip.h"


def header_functions():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(dalm_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    from dalm_amd import _build, hip

    _build.build(verbose=False)  # hipcc cross-compiles for gfx950 without a GPU
    return hip.load()


def test_header_declares_expected_entry_points():
    names = header_functions()
    for required in ("dalm_marg_ce_fwd", "dalm_marg_ce_bwd", "dalm_sim_rowstats", "dalm_sim_grad",
                     "dalm_sim_matmul", "dalm_pool_l2norm_fwd", "dalm_pool_l2norm_bwd", "dalm_version",
                     "dalm_last_error_string", "dalm_lora2_rankupd_rows_per_wg", "dalm_lora2_colacc_rows_per_split"):
        assert required in names


def test_library_exports_every_header_symbol(lib):
    for name in header_functions():
        assert hasattr(lib, name), f"{name} declared in include/dalm_hip.h but not exported"


def test_ctypes_table_matches_header(lib):
    from dalm_amd import hip

    assert sorted(hip.SIGNATURES) == header_functions()
    # argument counts: count commas in each prototype
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name, (_, args) in hip.SIGNATURES.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert m, name
        params = m.group(1).strip()
        n = 0 if params in ("", "void") else params.count(",") + 1
        assert n == len(args), f"{name}: header has {n} params, ctypes table {len(args)}"


def test_version_and_error_string(lib):
    assert lib.dalm_version() >= 100
    assert isinstance(lib.dalm_last_error_string(), bytes)


def test_argument_errors_are_reported_without_a_gpu(lib):
    # NULL pointers are rejected before any HIP call is made
    rc = lib.dalm_sim_matmul(None, None, 4, 4, 8, ctypes.c_float(1.0), None, 4, None)
    assert rc == -1
    assert b"null pointer" in lib.dalm_last_error_string()
    rc = lib.dalm_marg_ce_fwd(None, 0, 1, 2, 3, 6, 3, None, None, None, None, None, None, None)
    assert rc == -1
    # nf4: sizes of the two stores, and argument errors before any launch
    assert lib.dalm_nf4_packed_bytes(0) == 0 and lib.dalm_nf4_packed_bytes(64) == 32 and lib.dalm_nf4_packed_bytes(65) == 33
    assert lib.dalm_nf4_absmax_count(64) == 1 and lib.dalm_nf4_absmax_count(65) == 2
    assert lib.dalm_nf4_quantize(None, 0, 64, None, None, None) == -1
    assert lib.dalm_nf4_dequantize(None, None, -1, 0, None, None) == -2
    assert lib.dalm_nf4_quantize(None, 0, 0, None, None, None) == 0          # nothing to do is not an error


def test_product_path_refuses_cpu_tensors():
    """No CPU fallback: the public functions raise on CPU tensors instead of computing elsewhere."""
    from dalm_amd.training.utils import train_utils as tu

    q = torch.randn(4, 8)
    with pytest.raises(RuntimeError, match="HIP|MI355X|GPU"):
        tu.get_cosine_sim(q, q, 100)
    with pytest.raises(RuntimeError, match="HIP|MI355X|GPU"):
        tu.get_nt_xent_loss(torch.randn(4, 4))
    from dalm_amd.models import nf4

    with pytest.raises(RuntimeError, match="HIP|MI355X|GPU"):
        nf4.quantize(torch.randn(128))
    with pytest.raises(RuntimeError, match="HIP|MI355X|GPU"):
        nf4.NF4Linear(torch.nn.Linear(64, 64))


def test_package_never_imports_oracle():
    """Product code must not import anything under oracle/."""
    for py in (ROOT / "dalm_amd").rglob("*.py"):
        src = py.read_text()
        assert "dalm_oracle" not in src and "import oracle" not in src and "from oracle" not in src, py


def test_launchers_read_only_the_reference_switches():
    """The launchers pick every kernel by shape and dtype.  The environment reads left in the HIP sources are the switches
    committed tests use as a reference: the first attention forms and the top-k first pass."""
    csrc = ROOT / "dalm_amd" / "csrc"
    names = set()
    for src in sorted([*csrc.glob("*.hip"), *csrc.glob("*.hpp")]):
        calls = re.findall(r"\bgetenv\s*\(([^)]*)\)", src.read_text())
        literal = [re.fullmatch(r'\s*"([A-Za-z0-9_]+)"\s*', c) for c in calls]
        assert all(literal), (src.name, calls)
        names.update(m.group(1) for m in literal)
    assert names == {"DALM_ATTN_FWD", "DALM_ATTN_DKDV", "DALM_TOPK_BF16X3"}


def test_host_code_names_only_the_kept_switches():
    """The Python host code selects every path from device, dtype, shape and its run-time guards.  The DALM_* names left in the
    package (reads, comments and docstrings alike) are the switches tests use to build a reference model, and the settings with
    a documented trade-off: launch structure, memory budgets, tuning, communicator bring-up and hardware queues."""
    names = set()
    for py in sorted((ROOT / "dalm_amd").rglob("*.py")):
        names.update(re.findall(r"DALM_[A-Z0-9_]+", py.read_text()))
    assert names == {
        "DALM_ATTN_FWD_KERNEL", "DALM_ATTN_KERNEL", "DALM_BUILD_JOBS", "DALM_CLAIM_QUEUES", "DALM_COMM_BRINGUP_TIMEOUT_S",
        "DALM_COMM_ID_FILE", "DALM_FALCON_KERNELS", "DALM_FAST_ROPE", "DALM_FORCE_DIST", "DALM_HW_QUEUES", "DALM_LM_HEAD_KERNEL",
        "DALM_LM_HEAD_TRAIN_KERNEL", "DALM_LOGITS_BUDGET_MB", "DALM_LORA_KERNEL", "DALM_NATIVE_COMM", "DALM_NF4",
        "DALM_NORM_KERNEL", "DALM_SIM_GRAD_X3", "DALM_STEP_GRAPHS", "DALM_SWIGLU_KERNEL", "DALM_TOWER_SETS", "DALM_TUNED_GEMMS"}


def test_header_is_plain_c(tmp_path):
    """include/dalm_hip.h must be consumable by a C compiler (cgo / JNI / ctypes-style bindings): compile a C
    translation unit that includes it and takes the address of every entry point."""
    import shutil
    import subprocess

    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    names = header_functions()
    src = tmp_path / "abi_check.c"
    body = "\n".join(f"  p[{i}] = (fn_t)&{n};" for i, n in enumerate(names))
    src.write_text(f'#include "dalm_hip.h"\ntypedef void (*fn_t)(void);\nfn_t p[{len(names)}];\n'
                   f'void fill(void) {{\n{body}\n}}\n')
    r = subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", str(ROOT / "include"), "-c", str(src),
                        "-o", str(tmp_path / "abi_check.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_every_quoted_include_is_a_build_header():
    """A header that a source includes but _build.HEADERS leaves out would not enter the object stamps: editing it would leave
    stale objects linked."""
    from dalm_amd import _build

    known = {p.resolve() for p in _build.HEADERS}
    files = [_build.CSRC / s for s in _build.SOURCES] + [p for p in _build.HEADERS if p.parent == _build.CSRC]
    assert sorted(_build.CSRC.glob("*.hpp")) == sorted(p for p in _build.HEADERS if p.parent == _build.CSRC)
    for f in files:
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read_text(), flags=re.M):
            assert (f.parent / inc).resolve() in known, f"{f.name} includes {inc}, which _build.HEADERS does not list"


def run_host_check(tmp_path, name, *args):
    """Builds tests/<name>.cpp against csrc's headers with the host compiler under the address and undefined-behaviour
    sanitizers (runtimes linked into the program), runs it and returns the finished process."""
    import shutil
    import subprocess

    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / name
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",   # runtimes inside the program
                        "-I", str(ROOT / "dalm_amd" / "csrc"), str(ROOT / "tests" / f"{name}.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True)


def test_dispatch_header_selection_rules(tmp_path):
    """csrc/dispatch.hpp is host-only C++17: tests/dispatch_check.cpp includes nothing else of the library, is built with the
    host compiler under the address and undefined-behaviour sanitizers, and checks every selection rule at its edges."""
    r = run_host_check(tmp_path, "dispatch_check")
    assert r.returncode == 0 and r.stdout.strip() == "dispatch ok", (r.returncode, r.stdout, r.stderr)


def test_similarity_workspace_layouts(tmp_path):
    """csrc/sim_plan.hpp is host-only C++17 too: tests/sim_plan_check.cpp checks, over the grid of tests/test_sim_sizes.py, that
    every workspace layout's regions lie in order, disjoint, aligned and inside the total the size functions report, that the
    column splits cover the matrix and that the 32-bit buffer offsets hold wherever a plan says ok."""
    from test_sim_sizes import GRID

    shapes = tmp_path / "shapes.txt"
    shapes.write_text("".join(f"{m} {n} {D}\n" for m, n, D in GRID))
    r = run_host_check(tmp_path, "sim_plan_check", shapes)
    assert r.returncode == 0 and r.stdout.strip() == f"sim plans ok: {len(GRID)} shapes", (r.returncode, r.stdout, r.stderr)


def test_gemm256_launch_plans(tmp_path):
    """csrc/gemm256_plan.hpp, the launch geometry of the MFMA GEMM core, is host-only C++17 as well: tests/gemm256_plan_check.cpp
    checks that the banded tile order (plain and live) is a bijection onto the tile grid for 1..40 row tiles, that the SPLIT3
    reciprocal is exact over its whole domain, that the builder's fields and guards equal literally restated expectations (lm_head
    and live-row shapes, and the grid of tests/test_sim_sizes.py), and the bf16x3 workspace layouts over that grid."""
    from test_sim_sizes import GRID

    shapes = tmp_path / "shapes.txt"
    shapes.write_text("".join(f"{m} {n} {D}\n" for m, n, D in GRID))
    r = run_host_check(tmp_path, "gemm256_plan_check", shapes)
    assert r.returncode == 0 and r.stdout.strip() == f"gemm256 plans ok: {len(GRID)} shapes", (r.returncode, r.stdout, r.stderr)


def test_lora2_launch_plans(tmp_path):
    """csrc/lora2_plan.hpp, the launch geometry of the stacked LoRA kernels, is host-only C++17 as well: tests/lora2_plan_check.cpp
    checks, over the grid of tests/test_lora2_sizes.py and every row count up to its largest, that rankupd's workgroups hold a
    multiple of 4 rows and at most 256, that colacc's splits hold a multiple of 32 rows and never ask for more than 64 KB of LDS,
    that both cover the rows exactly, the workspace and ticket sizes, and the literal plans of the benchmark's shape and of the
    shapes tests/test_lora2_forms_gpu.py is built on."""
    from test_lora2_sizes import GRID

    shapes = tmp_path / "shapes.txt"
    shapes.write_text("".join(f"{R} {C}\n" for R, C in GRID))
    r = run_host_check(tmp_path, "lora2_plan_check", shapes)
    want = f"lora2 plans ok: {len(GRID)} shapes, rows 1..{max(R for R, _ in GRID)} at {len({C for _, C in GRID})} widths"
    assert r.returncode == 0 and r.stdout.strip() == want, (r.returncode, r.stdout, r.stderr)
