"""GPU: the gallery (sar_runtime_gallery / k_gallery) — many maps rendered as tiles of one atlas, each tile in one workgroup with
its image in LDS. A tile is an ordinary small render, so every comparison is against oracle_lib.render_jobs + oracle_lib.colorize
on an oracle Runtime of the tile's size: count, max, zbuf bits, steps bits and RGBA16, all equal. Shapes are the smallest that can
still go wrong (ragged tiles and job counts, the 16 384-pixel boundary, an 8 x 8 tile where every address is contended, more
tiles than the chip holds at once, chunk boundaries)."""
import numpy as np
import pytest

from gallery_cases import EXTENT, SEED

pytestmark = pytest.mark.gpu

DIVERGING = np.full(30, 1.2)     # every coefficient 1.2: each trajectory is at +inf within a dozen steps of the warm-up


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.fixture(scope="module")
def rt(sar, gpu):
    r = sar.Runtime(sar.Config.solar_sail(width=48, height=32), device=0)
    yield r
    r.close()


def _found_item(sar, base, cand, tile, margin=0.05):
    """(coefficients, (center_camera, scale)) of a pinned map framed from its search record's extent at the tile's size."""
    framed = sar.frame_view_box(base.replace(width=tile[0], height=tile[1]), EXTENT[cand], margin=margin)
    return sar.search_candidate(SEED, cand).ravel(), (framed.center_camera, framed.scale)


def _preset_item(cfg):
    return np.concatenate([cfg.coeff_x, cfg.coeff_y, cfg.coeff_z]), (cfg.center_camera, cfg.scale)


def _items(sar, base, pairs):
    return sar.gallery_items(np.stack([c for c, _ in pairs]), [v for _, v in pairs], base=base)


def _oracle_tile(oracle, cfg, starts):
    """What the contract names: a fresh runtime, render_jobs(cfg_i, starts), colorize(cfg_i)."""
    ort = oracle.Runtime(cfg.width, cfg.height)
    oracle.render_jobs(cfg.c, ort, starts, cfg.iterations // cfg.jobs_total)
    return ort.count.copy(), ort.max, ort.zbuf.copy(), ort.steps.copy(), oracle.colorize(cfg.c, ort)


def _assert_tile(g, i, want, what):
    count, mx, zbuf, steps, img = want
    assert np.array_equal(g.count[i], count), f"{what}: count differs"
    assert int(g.stats["max"][i]) == mx, f"{what}: max differs"
    assert np.array_equal(_bits(g.zbuf[i]), _bits(zbuf)), f"{what}: zbuf differs"
    assert np.array_equal(_bits(g.steps[i]), _bits(steps)), f"{what}: steps differs"
    assert np.array_equal(g.tile(i), img), f"{what}: RGBA16 differs"
    assert int(g.stats["covered"][i]) == int(np.count_nonzero(count)), f"{what}: covered differs"
    assert int(g.stats["hits"][i]) == int(count.sum(dtype=np.uint64)), f"{what}: hits differs"


def _ragged_pairs(sar, base, tile):
    return [_preset_item(sar.Config.solar_sail()), _preset_item(sar.Config.poisson_saturne())] + \
           [_found_item(sar, base, c, tile) for c in (545, 2573, 6377)]


def test_ragged_tiles_jobs_and_iterations(sar, oracle, rt):
    """5 tiles of 40 x 24, two per row: 1500 jobs (more than a workgroup, no multiple of a wave), iterations that do not divide,
    the library's own start points; the sixth cell stays zero."""
    tile, jobs, iterations = (40, 24), 1500, 1500 * 40 + 7
    base = sar.Config.solar_sail()
    items = _items(sar, base, _ragged_pairs(sar, base, tile))
    g = sar.gallery(rt, base, items, tile=tile, cols=2, jobs=jobs, iterations=iterations, seed=5, raw=True)
    assert g.image.shape == (72, 80, 4) and g.count.shape == (5, 24, 40)
    starts = sar.start_points(5, 0, jobs)
    covered = 0
    for i in range(5):
        cfg = g.config(i)
        assert cfg.iterations // cfg.jobs_total == 40
        _assert_tile(g, i, _oracle_tile(oracle, cfg, starts), f"tile {i}")
        r, c = divmod(i, 2)
        assert np.array_equal(g.image[24 * r:24 * r + 24, 40 * c:40 * c + 40], g.tile(i))
        covered += int(g.stats["covered"][i])
    assert covered > 5 * 40 and np.all(g.stats["hits"][2:] > 0)       # the framed maps are in their pictures
    assert not g.image[48:72, 40:80].any()                            # the cell without a tile
    # the other colour transform
    base2 = sar.Config.poisson_saturne()
    pairs = _ragged_pairs(sar, base2, tile)
    g2 = sar.gallery(rt, base2, _items(sar, base2, [pairs[1], pairs[3]]), tile=tile, cols=2, jobs=jobs, iterations=iterations, seed=5,
                     raw=True)
    for i in range(2):
        _assert_tile(g2, i, _oracle_tile(oracle, g2.config(i), starts), f"poisson-saturne colours, tile {i}")


def test_the_largest_tile(sar, oracle, rt):
    """128 x 128 = 16 384 pixels: the whole 128 KiB of keys, the defaults' 1024 jobs and 2^20 iterations.

    The issue behind this test asked for a 129 x 127 request to be refused as "more than 16 384 pixels"; 129 * 127 is 16 383, within
    the limit the same issue sets (tile_width * tile_height <= 16384). The limit is kept as the pixel count: 129 x 127 is rendered
    and held to the oracle, 129 x 128 and 128 x 129 are refused."""
    base = sar.Config.solar_sail()
    items = _items(sar, base, [_found_item(sar, base, 3944, (128, 128))])
    g = sar.gallery(rt, base, items, raw=True)
    assert g.image.shape == (128, 1024, 4) and not g.image[:, 128:].any()
    _assert_tile(g, 0, _oracle_tile(oracle, g.config(0), sar.start_points(0, 0, 1024)), "128 x 128")
    assert int(g.stats["covered"][0]) > 1000
    # the boundary is the pixel count: 129 x 127 = 16 383 pixels is a tile (and an odd one), one more column or row is refused
    odd = _items(sar, base, [_found_item(sar, base, 3944, (129, 127))])
    g = sar.gallery(rt, base, odd, tile=(129, 127), cols=1, jobs=1024, iterations=1024 * 100, seed=2, raw=True)
    _assert_tile(g, 0, _oracle_tile(oracle, g.config(0), sar.start_points(2, 0, 1024)), "129 x 127")
    for size in ((129, 128), (128, 129)):
        with pytest.raises(sar.SarError) as e:
            sar.gallery(rt, base, items, tile=size)
        assert e.value.status == sar._abi.SAR_ERR_INVALID


def test_a_tiny_tile_and_exact_depth_ties(sar, oracle, rt):
    """8 x 8 under 2^18 iterations: thousands of visits a pixel, every LDS address contended, f32 depth ties likely. Then start
    points that all appear twice: identical trajectories, every visit an exact tie, the earlier job must win."""
    tile, jobs, iterations = (8, 8), 256, 1 << 18
    base = sar.Config.solar_sail()
    items = _items(sar, base, [_found_item(sar, base, 2573, tile)])
    for what, starts in (("distinct starts", sar.start_points(11, 0, jobs)),
                         ("every start twice", np.repeat(sar.start_points(12, 0, jobs // 2), 2, axis=0))):
        g = sar.gallery(rt, base, items, tile=tile, cols=1, jobs=jobs, iterations=iterations, starts=starts, raw=True)
        want = _oracle_tile(oracle, g.config(0), starts)
        _assert_tile(g, 0, want, what)
        assert want[1] > 1000 and int(g.stats["dead_jobs"][0]) == 0


MANY = 600


@pytest.fixture(scope="module")
def many(sar, oracle, rt):
    """600 tiles of 16 x 16 — more than the chip holds at once — cycling through three found maps and one that diverges in the
    warm-up, with the oracle's tile of each of the four."""
    tile, jobs, iterations = (16, 16), 64, 4096
    base = sar.Config.solar_sail()
    four = [_found_item(sar, base, c, tile) for c in (545, 2573, 6377)] + [(DIVERGING, ((0.0, 0.0, 0.0), 1.0))]
    items = _items(sar, base, [four[i % 4] for i in range(MANY)])
    kw = dict(tile=tile, cols=25, jobs=jobs, iterations=iterations, seed=3, raw=True)
    g = sar.gallery(rt, base, items, **kw)
    starts = sar.start_points(3, 0, jobs)
    want = [_oracle_tile(oracle, g.config(i), starts) for i in range(4)]
    return base, items, kw, g, want


def test_more_tiles_than_the_chip_holds(sar, oracle, many):
    base, items, kw, g, want = many
    assert g.image.shape == (24 * 16, 25 * 16, 4)
    for i in range(MANY):
        _assert_tile(g, i, want[i % 4], f"tile {i}")     # a tile after a dense one inherits nothing
    # the diverging map: every job dropped, the tile is the colorize of an untouched runtime
    assert np.all(g.stats["dead_jobs"][3::4] == 64) and np.all(g.stats["hits"][3::4] == 0)
    untouched = oracle.colorize(g.config(3).c, oracle.Runtime(16, 16))
    assert np.array_equal(g.tile(3), untouched) and np.array_equal(g.tile(MANY - 1), untouched)
    assert np.all(g.zbuf[3] == -1.0) and not g.steps[3].any()
    assert want[1][1] > 0 and np.all(g.stats["dead_jobs"][1::4] == 0)


def test_results_do_not_depend_on_the_chunk(sar, rt, many):
    base, items, kw, g, _ = many
    rt.set_option("gallery_chunk", 7)
    try:
        h = sar.gallery(rt, base, items[:50], **kw)
    finally:
        rt.set_option("gallery_chunk", 0)
    assert np.array_equal(h.image, g.image[:32]) and h.image.shape == (32, 400, 4)
    assert np.array_equal(h.count, g.count[:50]) and np.array_equal(_bits(h.zbuf), _bits(g.zbuf[:50]))
    assert np.array_equal(_bits(h.steps), _bits(g.steps[:50])) and h.stats.tobytes() == g.stats[:50].tobytes()


@pytest.mark.parametrize("variant", [dict(render_kind=1), dict(transparent=0)])
def test_depth_kind_and_opaque_gas(sar, oracle, rt, variant):
    """Depth colours from the tile's own z range, with one empty tile for the 'unset' branch; and Gas without transparency."""
    tile, jobs, iterations = (40, 24), 1500, 1500 * 40 + 7
    base = sar.Config.solar_sail(**variant)
    pairs = _ragged_pairs(sar, base, tile)[:3]
    pairs[1] = (DIVERGING, pairs[1][1])
    g = sar.gallery(rt, base, _items(sar, base, pairs), tile=tile, cols=2, jobs=jobs, iterations=iterations, seed=5, raw=True)
    starts = sar.start_points(5, 0, jobs)
    for i in range(3):
        cfg = g.config(i)
        assert cfg.render_kind == base.render_kind and cfg.transparent == base.transparent
        _assert_tile(g, i, _oracle_tile(oracle, cfg, starts), f"{variant}, tile {i}")
    assert int(g.stats["hits"][1]) == 0 and int(g.stats["hits"][0]) > 0
    assert np.all(g.image[:24, :80, 3] == 65535)


def test_agreement_with_the_frame_path(sar, rt):
    """One 64 x 64 tile against Runtime(64 x 64) + render_jobs + colorize on the GPU with the same starts."""
    tile, jobs, iterations = (64, 64), 2048, 2048 * 150
    base = sar.Config.poisson_saturne()
    g = sar.gallery(rt, base, _items(sar, base, [_found_item(sar, base, 3944, tile)]), tile=tile, cols=1, jobs=jobs, iterations=iterations,
                    seed=21, raw=True)
    cfg = g.config(0)
    r = sar.Runtime(cfg)
    try:
        sar.render_jobs(cfg, r, sar.start_points(21, 0, jobs))
        _assert_tile(g, 0, (r.count(), r.max(), r.zbuf(), r.steps(), sar.colorize(cfg, r)), "gallery against render_jobs")
        assert r.max() > 0
    finally:
        r.close()


def test_the_runtime_is_left_alone(sar, rt):
    cfg = sar.Config.solar_sail(width=48, height=32, iterations=512 * 100, jobs_total=512)
    rt.reset()
    sar.render_jobs(cfg, rt, sar.start_points(8, 0, 512))
    before = (rt.count(), rt.max(), rt.zbuf(), rt.steps(), sar.colorize(cfg, rt))
    assert before[1] > 0
    base = sar.Config.poisson_saturne()
    sar.gallery(rt, base, _items(sar, base, [_found_item(sar, base, 2573, (32, 32))] * 3), tile=(32, 32), cols=2, jobs=128,
                iterations=128 * 64)
    after = (rt.count(), rt.max(), rt.zbuf(), rt.steps(), sar.colorize(cfg, rt))
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    assert np.array_equal(_bits(before[2]), _bits(after[2])) and np.array_equal(_bits(before[3]), _bits(after[3]))
    assert np.array_equal(before[4], after[4])
    # the start-point stream was not drawn from either
    a = sar.Runtime(cfg.replace(seed=4))
    b = sar.Runtime(cfg.replace(seed=4))
    try:
        sar.gallery(a, base, _items(sar, base, [_found_item(sar, base, 2573, (16, 16))]), tile=(16, 16), jobs=64, iterations=640)
        sar.render_jobs(cfg, a, None)
        sar.render_jobs(cfg, b, None)
        assert np.array_equal(a.count(), b.count())
    finally:
        a.close()
        b.close()


def test_refusals(sar, rt):
    """Every case of the header's list returns SAR_ERR_INVALID with a text; n == 0 succeeds."""
    import ctypes as C
    lib = sar.load_library()
    base = sar.Config.solar_sail()
    items = _items(sar, base, [_found_item(sar, base, 2573, (16, 16))])
    ip = items.ctypes.data_as(C.POINTER(sar._abi.SarGalleryItem))
    atlas = np.zeros((16, 16, 4), dtype=np.uint16)
    ap = atlas.ctypes.data_as(C.POINTER(C.c_uint16))
    ok = dict(tile_width=16, tile_height=16, cols=1, jobs=64, iterations=640)
    cases = [dict(tile_width=0), dict(tile_height=0), dict(tile_width=129, tile_height=128), dict(cols=0), dict(jobs=0),
             dict(jobs=2, iterations=1 << 32), dict(jobs=1, iterations=(1 << 32) + 5)]
    for kw in cases:
        p = sar.gallery_params(**{**ok, **kw})
        assert lib.sar_runtime_gallery(rt.handle, C.byref(base.c), C.byref(p), 1, ip, None, ap, None, None, None, None) == sar._abi.SAR_ERR_INVALID, kw
        assert lib.sar_last_error().decode().startswith("sar_runtime_gallery:"), (kw, lib.sar_last_error())
    p = sar.gallery_params(**ok)
    for bad in (base.replace(palette_len=0), base.replace(render_kind=7), base.replace(color_transform=9)):
        assert lib.sar_runtime_gallery(rt.handle, C.byref(bad.c), C.byref(p), 1, ip, None, ap, None, None, None, None) == sar._abi.SAR_ERR_INVALID
        assert lib.sar_last_error().decode()
    assert lib.sar_runtime_gallery(rt.handle, C.byref(base.c), C.byref(p), 1, None, None, ap, None, None, None, None) == sar._abi.SAR_ERR_INVALID
    assert "items_host" in lib.sar_last_error().decode()
    assert lib.sar_runtime_gallery(rt.handle, C.byref(base.c), C.byref(p), 0, None, None, None, None, None, None, None) == 0
    empty = sar.gallery(rt, base, items[:0], tile=(16, 16), cols=1, jobs=64, iterations=640, raw=True)
    assert empty.image.shape == (0, 16, 4) and empty.count.shape == (0, 16, 16) and len(empty) == 0
    # jobs * (iterations / jobs) = 2^32 - 1 is the last one allowed: not rendered here, only not refused for its size
    assert lib.sar_runtime_gallery(rt.handle, C.byref(base.c), C.byref(sar.gallery_params(**{**ok, "jobs": 1, "iterations": (1 << 32) - 1})),
                                   0, None, None, None, None, None, None, None) == 0
    # and the call still works
    g = sar.gallery(rt, base, items, tile=(16, 16), cols=1, jobs=64, iterations=640)
    assert g.image.any()
