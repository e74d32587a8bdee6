"""The similarity entry points' size and choice functions return what they returned before their launchers took every
workspace offset from csrc/sim_plan.hpp: tests/golden/sim_sizes.json was recorded from the library of the commit before that
change (`python tests/test_sim_sizes.py` rewrites it from whatever library is built - only ever run that on a trusted
commit).  No GPU: the functions are host arithmetic."""
import json
from pathlib import Path

GOLDEN = Path(__file__).resolve().parent / "golden" / "sim_sizes.json"

# (m, n, D): the fixed shape lists of tests/test_kernels_r2_gpu.py ...
R2_SHAPES = [
    (18, 18, 1024), (150, 150, 1024), (19, 19, 384), (1, 1, 64), (18, 144, 1024), (150, 1200, 1024), (257, 300, 100),   # SMALL
    (33, 65, 1030), (600, 600, 768), (1024, 1024, 32), (512, 512, 1024), (70, 2100, 256), (1000, 1000, 64),
    (18, 8000, 1024), (33, 900, 1030),
    (1200, 1200, 1024), (4096, 4096, 1024), (700, 2304, 128), (1536, 1536, 256), (333, 5000, 384), (2100, 2100, 768),   # FLASH
    (40, 130, 512), (1, 1, 128), (33, 257, 640), (129, 129, 896),
    (600, 900, 100), (4096, 4096, 384), (4101, 4300, 64), (513, 513, 72), (150, 4000, 1024), (1199, 1203, 200),         # STREAM
    (2048, 2048, 128), (1500, 1530, 72),
    (37, 5000, 96), (300, 70000, 384), (5, 40, 64), (129, 3001, 1024), (64, 2000, 100), (260, 20000, 256), (64, 6000, 256),   # top-k
    (256, 256, 64), (300, 517, 128), (37, 1000, 384), (1024, 1536, 1024), (513, 4352, 1024), (700, 5000, 256)]          # bf16x3
# ... the shapes of tests/test_sim_workspace_gpu.py ...
CARVE_SHAPES = [(512, 512, 64), (1200, 1200, 72), (1536, 1536, 72), (4096, 130, 64), (100, 300, 40), (2048, 1024, 32),
                (32, 128, 128), (64, 256, 128), (32, 128, 1024), (100, 300, 96), (100, 300, 320), (4096, 64, 64), (4096, 4100, 72)]
# ... and every selection threshold, one either side
THRESHOLD_SHAPES = [
    (511, 512, 64), (512, 513, 64), (512, 512, 63),                        # stream form: m * n = 512^2, D = 63 / 64
    (4095, 256, 64), (4096, 256, 64),                                      # two row tiles per wave from m = 4096
    (416, 2944, 64), (480, 2560, 64), (32, 57472, 64), (480, 3840, 64), (288, 9088, 64), (640, 4096, 64),   # g128 = 299 / 300 / 449 / 450 / 639 / 640
    (1024, 64, 64), (1025, 64, 64), (1024, 1025, 64), (128, 8192, 64), (128, 8193, 64),   # small path: m, m * n = 2^20, n
    (1024, 1920, 32), (1024, 2048, 32),                                    # 64^2 / 128^2 GEMM tiles
    (64, 600000, 1024), (4096, 600000, 1024),                              # past the 32-bit buffer offsets
    (96, 300, 255), (96, 300, 256), (100, 300, 1025), (100, 300, 1152), (3072, 3072, 128), (3071, 3072, 128)]
GRID = sorted(set(R2_SHAPES + CARVE_SHAPES + THRESHOLD_SHAPES))
TOPK_K = (1, 7, 10, 100, 1024, 1025)
DIRECTIONS = ((1, 1), (1, 0), (0, 1))


def calls():
    """(function name, arguments) of every recorded value."""
    for m, n, D in GRID:
        for fn in ("dalm_sim_rowstats_workspace_bytes", "dalm_sim_grad_workspace_bytes", "dalm_sim_gold_rank_workspace_bytes",
                   "dalm_sim_small_supported", "dalm_sim_small_fwd1_preferred", "dalm_sim_small_bwd1_ticket_words"):
            yield fn, (m, n, D)
        yield "dalm_sim_small_fwd1_ticket_words", (m, n)
        for k in TOPK_K:
            yield "dalm_sim_topk_workspace_bytes", (m, n, D, k)
        for want_cols in (0, 1):
            yield "dalm_sim_small_workspace_bytes", (m, n, D, want_cols)
            yield "dalm_sim_small_fwd1_workspace_bytes", (m, n, D, want_cols)
        for want in DIRECTIONS:
            yield "dalm_sim_small_bwd_workspace_bytes", (m, n, D, *want)
            yield "dalm_sim_small_bwd1_workspace_bytes", (m, n, D, *want)
    for D in sorted({D for _, _, D in GRID}):
        for k in TOPK_K:
            yield "dalm_sim_topk_supported", (D, k)


def measure():
    from dalm_amd import _build, hip

    _build.build(verbose=False)
    lib = hip.load()
    out = {}
    for fn, args in calls():
        out.setdefault(fn, {})[",".join(map(str, args))] = int(getattr(lib, fn)(*args))
    return out


def test_similarity_sizes_and_choices_are_the_recorded_ones():
    want = json.loads(GOLDEN.read_text())
    got = measure()
    assert sorted(got) == sorted(want)
    for fn in want:
        assert got[fn] == want[fn], (fn, {k: (want[fn].get(k), v) for k, v in got[fn].items() if want[fn].get(k) != v})


def test_the_grid_reaches_both_sides_of_every_choice():
    """A grid on which a choice function never changed its answer would pin nothing."""
    want = json.loads(GOLDEN.read_text())
    for fn in ("dalm_sim_small_supported", "dalm_sim_small_fwd1_preferred", "dalm_sim_topk_supported"):
        assert set(want[fn].values()) == {0, 1}, fn
    for fn in ("dalm_sim_topk_workspace_bytes", "dalm_sim_gold_rank_workspace_bytes", "dalm_sim_small_bwd_workspace_bytes",
               "dalm_sim_small_bwd1_workspace_bytes"):
        assert 0 in want[fn].values() and max(want[fn].values()) > 0, fn


if __name__ == "__main__":
    GOLDEN.write_text(json.dumps(measure(), indent=0, sort_keys=True) + "\n")
    print(GOLDEN, sum(len(v) for v in measure().values()), "values")
