"""What the split-phase tests share (tests/test_split_phases_host.py, tests/test_gpu_split_phases.py): the image shapes that put
k_iterate_split on either side of the edges of its one-iteration-per-phase form, and the host's rules for that form restated.

The wave-pair kernel k_iterate_split is compiled with two iterations per barrier phase (PH = 2: 2 KiB of visits in flight between
the producer and the consumer wave) and with one (PH = 1: 1 KiB). With stage = kPoolWaveLds(bins, R) (csrc/sar_device.hpp) the
launchers pick PH = 2 while (stage + 2048) * 8 <= 160 KiB, PH = 1 beyond (split_phase_iterations, csrc/sar_iterate.hip), and the
plan allows the wave-pair kernel at all only while (stage + 1024) * 8 <= 160 KiB (plan_launch, csrc/sar_plan.cpp): PH = 1 lives in
a window of 1 KiB of staging size,

    R = 28 (64-byte chunks):  stage = 68 bins + 1088 (rounded up to 16)   PH = 2: bins <= 255   PH = 1: 256 .. 270   whole: >= 271
    R = 60 (128-byte chunks): stage = 132 bins + 1056 (rounded up to 16)  PH = 2: bins <= 131   PH = 1: 132 .. 139   whole: >= 140

Every shape of the table below has bins of 4096 pixels ("bin_shift" 12): the smallest images that reach those bin counts. `product`
is the one shape the library's own planning takes there: 256 interleaved bins of 65536 pixels with 28 records, for every image
above 8 388 608 and up to 16 777 216 pixels. Everything here is host arithmetic; the formulas are restated from the sources, not
read from the library, so that a changed constant fails the host test instead of quietly moving a case out of its window."""
from __future__ import annotations

import numpy as np

LDS_BYTES = 160 * 1024
PAIRS_PER_CU = 8
WIDE_HINT_MAX_SPAN2 = 11.0e6          # (width * scale)^2 up to which the plan picks f32 hints by itself (kWideHintMaxSpan2)
WIDE_HINT_MAX_PIXELS = 16 << 20
POOL_SPARE = 16                       # SAR_POOL_SPARE


def chunk_bytes(records: int) -> int:
    return 8 + 2 * records


def spare_buffers(records: int) -> int:
    quads = chunk_bytes(records) // 16
    lanes = 2 if quads <= 2 else (4 if quads <= 4 else 8)       # lanes that move one chunk
    return min(POOL_SPARE, 64 // lanes)


def stage_bytes(bins: int, records: int) -> int:
    """kPoolWaveLds: buffers | control words | ring, rounded up to a multiple of 16 bytes."""
    s = spare_buffers(records)
    return ((bins + s) * chunk_bytes(records) + bins * 4 + s * 4 + 15) & ~15


def pair_kernel_fits(bins: int, records: int) -> bool:
    """plan_launch: staging + the smaller hand-over for eight wave pairs per CU."""
    return records in (28, 60) and (stage_bytes(bins, records) + 1024) * PAIRS_PER_CU <= LDS_BYTES


def phase_iterations(bins: int, records: int) -> int:
    """split_phase_iterations: two iterations per barrier phase if eight pairs still fit with 2 KiB of hand-over each."""
    return 2 if (stage_bytes(bins, records) + 2048) * PAIRS_PER_CU <= LDS_BYTES else 1


def expected_launch(bins: int, records: int) -> tuple:
    """(kernel name, phase= field) of a launch that asked for wave pairs."""
    if pair_kernel_fits(bins, records):
        return "k_iterate_split", phase_iterations(bins, records)
    return "k_iterate_lean", 0


def auto_hint_bits(width: int, height: int, scale: float) -> int:
    """plan_launch's choice with "hint_bits" unset."""
    span = width * scale
    return 32 if span * span <= WIDE_HINT_MAX_SPAN2 and width * height <= WIDE_HINT_MAX_PIXELS else 16


# name -> image size, the test options that fix the geometry, and what the table of the module docstring says of it
SHAPES = {
    "r28_first": dict(size=(1024, 1024), bin_interleave=2, chunk_records=28, bins=256, kernel="k_iterate_split", phase=1),
    "r28_last2": dict(size=(1024, 1020), bin_interleave=1, chunk_records=28, bins=255, kernel="k_iterate_split", phase=2),
    "r28_last": dict(size=(1024, 1080), bin_interleave=1, chunk_records=28, bins=270, kernel="k_iterate_split", phase=1),
    "r28_lean": dict(size=(1024, 1084), bin_interleave=1, chunk_records=28, bins=271, kernel="k_iterate_lean", phase=0),
    "r60_last2": dict(size=(1024, 524), bin_interleave=1, chunk_records=60, bins=131, kernel="k_iterate_split", phase=2),
    "r60_first": dict(size=(1024, 528), bin_interleave=1, chunk_records=60, bins=132, kernel="k_iterate_split", phase=1),
    "r60_mid": dict(size=(1024, 544), bin_interleave=1, chunk_records=60, bins=136, kernel="k_iterate_split", phase=1),
    "r60_last": dict(size=(1024, 556), bin_interleave=1, chunk_records=60, bins=139, kernel="k_iterate_split", phase=1),
    "r60_lean": dict(size=(1024, 560), bin_interleave=1, chunk_records=60, bins=140, kernel="k_iterate_lean", phase=0),
}
BIN_SHIFT = 12
NAMES = tuple(SHAPES)
PHASE1 = ("r28_first", "r60_mid")         # the two shapes every PH = 1 instantiation is run on
PHASE2 = ("r28_last2", "r60_last2")       # their neighbours below the window: the same code otherwise
# the product's own plan: no test option; 4096 x 2049 is the smallest image of width 4096 above 8 388 608 pixels
PRODUCT = dict(size=(4096, 2049), bin_shift=16, chunk_records=28, bins=256, kernel="k_iterate_split", phase=1, park=8)
DEFAULT_PARK = 8                          # kDefaultParkWide == kDefaultParkNarrow


def tuning(name: str) -> dict:
    """The options of Runtime.set_tuning that put a launch on shape `name` and ask for wave pairs."""
    s = SHAPES[name]
    return dict(variant=3, split_waves=2, bin_shift=BIN_SHIFT, bin_interleave=s["bin_interleave"], chunk_records=s["chunk_records"])


def description_fields(name: str, hint_bits: int, park: int) -> list:
    """The substrings a launch on shape `name` must describe itself with (park: of a wave-pair launch; the whole kernel has none)."""
    s = SHAPES[name]
    split = s["kernel"] == "k_iterate_split"
    return [s["kernel"] + " ", f" R={s['chunk_records']} ", f" bins={s['bins']}x{1 << BIN_SHIFT}px ",
            " interleaved " if s["bin_interleave"] == 2 else " consecutive ", f" hints={'q16' if hint_bits == 16 else 'f32'}",
            f" park={park if split else 0} ", f" phase={s['phase']} "]


def plan_product(bin_geometry, width: int, height: int) -> tuple:
    """choose_chunk_records' loop for a launch of wave pairs (eight staging sets per CU), restated: the larger chunk first, the
    smaller bin first, interleaved bins whatever the power-of-two count costs. `bin_geometry` is the package's (host arithmetic).
    Returns (records, bin_shift, bins) or None where the loop finds nothing."""
    for records in (60, 28):
        for shift in (15, 16):
            g = bin_geometry(width, height, shift, 2)
            if g["ok"] and g["interleaved"] and stage_bytes(g["bins"], records) * PAIRS_PER_CU <= LDS_BYTES:
                return records, shift, g["bins"]
    return None


def forget_depth_references(depth_cases, case, size) -> None:
    """Drops the references tests/depth_cases.py caches for the case at `size` (check_condition's figures stay): at the sizes used
    here a cached State is 40 MB and check_condition makes two, too much to keep for a whole run."""
    for key in [k for k in depth_cases._CACHE if k[0] == case and k[1] == tuple(size)]:
        del depth_cases._CACHE[key]


# the frame of tests/test_gpu_parity.py::test_chunk_sizes_and_accumulate_shapes_bit_exact: an odd iteration count (the depth
# pipeline's pass of two leaves a last single iteration), a job count that is no multiple of a workgroup, and 512 near-identical
# trajectories — many lanes hit one bin at once, staging buffers overflow within one slot request
JOBS, N, START_SEED = 2048 + 64, 1201, 23


def saturne_starts(start_points, jobs: int = JOBS) -> np.ndarray:
    st = start_points(START_SEED, 0, jobs)
    st[:512] = st[0] + np.arange(512)[:, None] * 1e-13
    return st
