"""The host side of the split-phase tests (tests/split_phase_cases.py), without a GPU: the staging size and the two inequalities that
decide between k_iterate_split with two iterations per barrier phase, with one, and k_iterate_lean, restated in Python and held to
the table of shapes — so that a change of a constant (the LDS budget, the spare buffers, a chunk's header) fails here and does not
quietly move a case of tests/test_gpu_split_phases.py out of its window. The bin counts come from sar.bin_geometry (host arithmetic
of the library); the depth cases' conditions are asserted on the oracle at the two sizes the GPU tests run them at."""
import pytest

import depth_cases as DC
import split_phase_cases as SP


def test_stage_formula_in_closed_form():
    """kPoolWaveLds for the two chunk sizes of the wave-pair kernel: 16 spare buffers of 64 bytes, 8 of 128."""
    assert (SP.chunk_bytes(28), SP.spare_buffers(28)) == (64, 16) and (SP.chunk_bytes(60), SP.spare_buffers(60)) == (128, 8)
    for bins in range(1, 1025):
        assert SP.stage_bytes(bins, 28) == (68 * bins + 1088 + 15) // 16 * 16
        assert SP.stage_bytes(bins, 60) == (132 * bins + 1056 + 15) // 16 * 16


@pytest.mark.parametrize("records,last2,last1", [(28, 255, 270), (60, 131, 139)])
def test_the_window_of_one_iteration_per_phase(records, last2, last1):
    """Every bin count from 1 to 1024: two iterations per phase up to `last2`, one up to `last1`, the whole kernel beyond."""
    for bins in range(1, 1025):
        want = ("k_iterate_split", 2) if bins <= last2 else (("k_iterate_split", 1) if bins <= last1 else ("k_iterate_lean", 0))
        assert SP.expected_launch(bins, records) == want, (bins, records)
    # the window is 1 KiB of staging size: the two hand-over sizes
    assert (SP.stage_bytes(last2, records) + 2048) * 8 <= SP.LDS_BYTES < (SP.stage_bytes(last2 + 1, records) + 2048) * 8
    assert (SP.stage_bytes(last1, records) + 1024) * 8 <= SP.LDS_BYTES < (SP.stage_bytes(last1 + 1, records) + 1024) * 8


def test_other_chunk_sizes_have_no_wave_pair_kernel():
    assert SP.expected_launch(1, 12) == ("k_iterate_lean", 0) and SP.expected_launch(1, 20) == ("k_iterate_lean", 0)


@pytest.mark.parametrize("name", SP.NAMES)
def test_the_table_of_shapes(sar, name):
    """Each row: the library's bin geometry gives the bin count and the map the row names, and the restated rules its launch."""
    s = SP.SHAPES[name]
    g = sar.bin_geometry(*s["size"], SP.BIN_SHIFT, s["bin_interleave"])
    assert g["ok"] == 1 and g["bin_shift"] == SP.BIN_SHIFT, g
    assert g["bins"] == s["bins"] and g["interleaved"] == (1 if s["bin_interleave"] == 2 else 0), (name, g)
    assert SP.expected_launch(g["bins"], s["chunk_records"]) == (s["kernel"], s["phase"]), name


def test_the_table_stands_on_both_edges_of_both_windows():
    by = {n: (s["chunk_records"], s["bins"], s["phase"]) for n, s in SP.SHAPES.items()}
    assert by["r28_last2"] == (28, 255, 2) and by["r28_first"] == (28, 256, 1) and by["r28_last"] == (28, 270, 1) and by["r28_lean"] == (28, 271, 0)
    assert by["r60_last2"] == (60, 131, 2) and by["r60_first"] == (60, 132, 1) and by["r60_last"] == (60, 139, 1) and by["r60_lean"] == (60, 140, 0)
    assert by["r60_mid"] == (60, 136, 1)
    for name in SP.PHASE1:
        assert SP.SHAPES[name]["phase"] == 1
    for name in SP.PHASE2:
        assert SP.SHAPES[name]["phase"] == 2
    # the sizes the depth cases run at are those of the two PH = 1 shapes
    assert [SP.SHAPES[n]["size"] for n in SP.PHASE1] == [(1024, 1024), (1024, 544)]


def test_what_the_product_plans_for_4096_x_2049(sar):
    """choose_chunk_records' loop over {60, 28} x {15, 16}, restated, lands on 28 records in 256 interleaved bins of 65536 pixels —
    the one shape of one iteration per phase that needs no test option — and so does the library's own default geometry."""
    w, h = SP.PRODUCT["size"]
    tried = []
    for records in (60, 28):
        for shift in (15, 16):
            g = sar.bin_geometry(w, h, shift, 2)
            tried.append((records, shift, g["bins"], SP.stage_bytes(g["bins"], records) * 8 <= SP.LDS_BYTES))
    assert tried == [(60, 15, 512, False), (60, 16, 256, False), (28, 15, 512, False), (28, 16, 256, True)], tried
    assert SP.plan_product(sar.bin_geometry, w, h) == (SP.PRODUCT["chunk_records"], SP.PRODUCT["bin_shift"], SP.PRODUCT["bins"]) == (28, 16, 256)
    g = sar.bin_geometry(w, h)
    assert (g["ok"], g["bins"], g["bin_shift"], g["interleaved"]) == (1, 256, 16, 1), g
    assert SP.expected_launch(SP.PRODUCT["bins"], SP.PRODUCT["chunk_records"]) == (SP.PRODUCT["kernel"], SP.PRODUCT["phase"]) == ("k_iterate_split", 1)
    # the whole range of image sizes the default geometry puts into 256 bins: above 8 388 608 and up to 16 777 216 pixels
    assert SP.plan_product(sar.bin_geometry, 4096, 2048) == (60, 16, 128)
    assert SP.plan_product(sar.bin_geometry, 4096, 4096) == (28, 16, 256)
    assert SP.plan_product(sar.bin_geometry, 4096, 4097) is None
    # frames of that shape do not share a batched launch (bins of 65536 pixels: packed counters, no batched accumulate kernel): the
    # one-iteration-per-phase form of k_iterate_split_batch is reached through the test options alone
    assert sar.batch_frames(sar.Config.poisson_saturne(iterations=2048 * 301, width=w, height=h, jobs_total=2048)) == 1
    # with 60 records the window holds no power of two: interleaved bins, all the product's own plan uses, never reach it
    assert not any(SP.expected_launch(1 << b, 60) == ("k_iterate_split", 1) for b in range(11))
    assert [1 << b for b in range(11) if SP.expected_launch(1 << b, 28) == ("k_iterate_split", 1)] == [256]


def test_the_hint_type_the_plan_picks_by_itself():
    """f32 hints while (width * scale)^2 <= 11e6: the scale the GPU test uses to get them unasked at width 4096, and its default."""
    w, h = SP.PRODUCT["size"]
    assert SP.auto_hint_bits(w, h, 1.0) == 16 and SP.auto_hint_bits(w, h, 0.5) == 32
    for name in SP.NAMES:
        assert SP.auto_hint_bits(*SP.SHAPES[name]["size"], 1.0) == 32, name


@pytest.mark.parametrize("size", [SP.SHAPES[n]["size"] for n in SP.PHASE1], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", DC.NAMES)
def test_the_depth_cases_reach_their_states_at_these_sizes(oracle, case, size):
    """tests/depth_cases.py's conditions hold on the oracle at 1024 x 1024 and 1024 x 544 as they do at the cases' own sizes."""
    f = DC.check_condition(oracle, case, size)
    SP.forget_depth_references(DC, case, size)
    print(f"{case} {size[0]}x{size[1]}: {f}")
