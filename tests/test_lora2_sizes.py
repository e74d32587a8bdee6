"""`dalm_lora2_colacc_workspace_bytes` / `dalm_lora2_colacc_ticket_words` return what they returned before the launch geometry
of dalm_amd/csrc/lora2.hip moved into csrc/lora2_plan.hpp: tests/golden/lora2_sizes.json was recorded from the library of the
commit before that move (`python tests/test_lora2_sizes.py` rewrites it from whatever library is built - only ever run that on
a trusted commit).  The move came with ONE change of arithmetic: colacc's cap on the rows of a split now counts all three LDS
stages (z, mask bytes, liveness) and the static ticket slot, so that a launch never asks for more than 64 KB.  The shapes whose
split count that changes are named in CAP_CHANGED; they are held to the invariants of tests/lora2_plan_check.cpp instead.
No GPU: the functions are host arithmetic."""
import json
from pathlib import Path

GOLDEN = Path(__file__).resolve().parent / "golden" / "lora2_sizes.json"

# rows: tile / wave / split edges (4, 32, 64, 256), the shapes of tests/test_lora2_forms_gpu.py, and one either side of
#   rankupd's min_s arm at C = 32768 / 65536 (R = 256 * floor(budget / workgroup columns): 768, 1024, 1536, 2048, 3072),
#   colacc's row cap before the fix at C = 4096 (4096, 8192, 16384) and after it (3584, 6272, 6400, 7168, 12544)
ROWS = [1, 2, 3, 4, 5, 8, 9, 17, 31, 32, 33, 63, 64, 65, 70, 120, 255, 256, 257, 511, 512, 513, 530, 577, 768, 769, 1024, 1025, 1030,
        1160, 1300, 1536, 1537, 2048, 2049, 2300, 2400, 3072, 3073, 3584, 3585, 4096, 4097, 4100, 4487, 4608, 6272, 6273, 6400, 6401,
        7168, 7169, 7210, 8192, 8193, 8200, 12544, 12545, 16384, 16385, 40000]
# columns: one chunk, one colacc slab (64) and one more chunk, the mask-stage rules (128 | C, 512 | C or not), one rankupd slab
#   (512) and one more chunk, the widths of the towers, and the widths at which a launch has one workgroup column per CU or more
COLS = [8, 64, 72, 128, 136, 512, 520, 640, 1024, 1152, 4096, 16384, 32768, 65536]
RANK_MODE = [(8, 1), (16, 1), (8, 2), (8, 3), (16, 3)]
GRID = [(R, C) for R in ROWS for C in COLS]

# (rank, mode) -> {C: [R, ...]}: the shapes of GRID whose split count the cap fix changed (rows per split before -> after:
# rank 8 modes 1 and 3 2048 -> 1568, rank 16 modes 1 and 3 1024 -> 896, mode 2 1024 -> 800)
CAP_CHANGED = {
    (8, 1): {
        4096: [12545, 16384, 16385, 40000],
        16384: [3584, 3585, 4096, 6273, 6400, 6401, 7168, 7169, 7210, 8192, 8193, 8200, 12544, 12545, 16384, 16385, 40000],
        32768: [2048, 3584, 3585, 4096, 6273, 6400, 6401, 7168, 7169, 7210, 8192, 8193, 8200, 12544, 12545, 16384, 16385,
                40000],
        65536: [2048, 3584, 3585, 4096, 6273, 6400, 6401, 7168, 7169, 7210, 8192, 8193, 8200, 12544, 12545, 16384, 16385,
                40000],
    },
    (16, 1): {
        1024: [40000],
        1152: [40000],
        4096: [7169, 7210, 8192, 8193, 8200, 12544, 12545, 16384, 16385, 40000],
        16384: [2048, 3072, 3585, 4096, 4487, 4608, 6273, 6400, 6401, 7168, 7169, 7210, 8192, 8193, 8200, 12544, 12545,
                16384, 16385, 40000],
        32768: [1024, 2048, 3072, 3585, 4096, 4487, 4608, 6273, 6400, 6401, 7168, 7169, 7210, 8192, 8193, 8200, 12544,
                12545, 16384, 16385, 40000],
        65536: [1024, 2048, 3072, 3585, 4096, 4487, 4608, 6273, 6400, 6401, 7168, 7169, 7210, 8192, 8193, 8200, 12544,
                12545, 16384, 16385, 40000],
    },
    (8, 2): {
        1024: [40000],
        1152: [40000],
        4096: [6401, 7168, 7169, 7210, 8192, 8193, 8200, 12544, 12545, 16384, 16385, 40000],
        16384: [2048, 3072, 3584, 3585, 4096, 4097, 4100, 4487, 4608, 6272, 6273, 6400, 6401, 7168, 7169, 7210, 8192, 8193,
                8200, 12544, 12545, 16384, 16385, 40000],
        32768: [1024, 2048, 3072, 3584, 3585, 4096, 4097, 4100, 4487, 4608, 6272, 6273, 6400, 6401, 7168, 7169, 7210, 8192,
                8193, 8200, 12544, 12545, 16384, 16385, 40000],
        65536: [1024, 2048, 3072, 3584, 3585, 4096, 4097, 4100, 4487, 4608, 6272, 6273, 6400, 6401, 7168, 7169, 7210, 8192,
                8193, 8200, 12544, 12545, 16384, 16385, 40000],
    },
    (8, 3): {
        1024: [40000],
        1152: [40000],
        4096: [6273, 6400, 6401, 7168, 7169, 7210, 8192, 8193, 8200, 12544, 12545, 16384, 16385, 40000],
        16384: [2048, 3584, 3585, 4096, 6273, 6400, 6401, 7168, 7169, 7210, 8192, 8193, 8200, 12544, 12545, 16384, 16385,
                40000],
        32768: [2048, 3584, 3585, 4096, 6273, 6400, 6401, 7168, 7169, 7210, 8192, 8193, 8200, 12544, 12545, 16384, 16385,
                40000],
        65536: [2048, 3584, 3585, 4096, 6273, 6400, 6401, 7168, 7169, 7210, 8192, 8193, 8200, 12544, 12545, 16384, 16385,
                40000],
    },
    (16, 3): {
        512: [40000],
        520: [40000],
        640: [40000],
        1024: [16384, 16385, 40000],
        1152: [16384, 16385, 40000],
        4096: [3585, 4096, 4487, 4608, 6273, 6400, 6401, 7168, 7169, 7210, 8192, 8193, 8200, 12544, 12545, 16384, 16385,
               40000],
        16384: [1024, 2048, 3072, 3585, 4096, 4487, 4608, 6273, 6400, 6401, 7168, 7169, 7210, 8192, 8193, 8200, 12544,
                12545, 16384, 16385, 40000],
        32768: [1024, 2048, 3072, 3585, 4096, 4487, 4608, 6273, 6400, 6401, 7168, 7169, 7210, 8192, 8193, 8200, 12544,
                12545, 16384, 16385, 40000],
        65536: [1024, 2048, 3072, 3585, 4096, 4487, 4608, 6273, 6400, 6401, 7168, 7169, 7210, 8192, 8193, 8200, 12544,
                12545, 16384, 16385, 40000],
    },
}


def calls():
    """(function name, arguments) of every recorded value."""
    for R, C in GRID:
        for rank, mode in RANK_MODE:
            yield "dalm_lora2_colacc_workspace_bytes", (R, C, rank, mode)
    for C in COLS:
        for mode in (1, 2, 3):
            yield "dalm_lora2_colacc_ticket_words", (C, mode)


def measure():
    from dalm_amd import _build, hip

    _build.build(verbose=False)
    lib = hip.load()
    out = {}
    for fn, args in calls():
        out.setdefault(fn, {})[",".join(map(str, args))] = int(getattr(lib, fn)(*args))
    return out


def _changed_keys():
    return {f"{R},{C},{rank},{mode}" for (rank, mode), cols in CAP_CHANGED.items() for C, rows in cols.items() for R in rows}


def test_colacc_sizes_are_the_recorded_ones_except_at_the_cap():
    from dalm_amd import hip

    want = json.loads(GOLDEN.read_text())
    got = measure()
    assert sorted(got) == sorted(want)
    assert got["dalm_lora2_colacc_ticket_words"] == want["dalm_lora2_colacc_ticket_words"]
    ws_want, ws_got = want["dalm_lora2_colacc_workspace_bytes"], got["dalm_lora2_colacc_workspace_bytes"]
    assert sorted(ws_want) == sorted(ws_got)
    differs = {k for k in ws_want if ws_want[k] != ws_got[k]}
    assert differs == _changed_keys(), (sorted(differs - _changed_keys()), sorted(_changed_keys() - differs))
    lib = hip.load()
    for key in sorted(differs):
        R, C, rank, mode = map(int, key.split(","))
        rows = lib.dalm_lora2_colacc_rows_per_split(R, C, rank, mode)
        nt = 2 if mode == 2 else 1
        per_row = nt * rank * 4 + nt * 8 + 1
        # the new cap itself: the largest multiple of 32 rows whose three stages fit beside the 16 static bytes
        assert rows == (65536 - 16) // per_row // 32 * 32 and rows * per_row + 16 <= 65536, key
        S = -(-R // rows)
        assert (S - 1) * rows < R <= S * rows and S <= 65535, key
        assert ws_got[key] == 2 * S * C * rank * 4 > ws_want[key], key


def test_the_grid_reaches_both_sides_of_the_cap():
    """A grid on which the cap never bound, or always did, would pin nothing."""
    keys = _changed_keys()
    for rank, mode in RANK_MODE:
        mine = {k for k in keys if k.endswith(f",{rank},{mode}")}
        assert 0 < len(mine) < len(GRID), (rank, mode)


if __name__ == "__main__":
    GOLDEN.write_text(json.dumps(measure(), indent=0, sort_keys=True) + "\n")
    print(GOLDEN, sum(len(v) for v in measure().values()), "values")
