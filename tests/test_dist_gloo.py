"""CPU, world_size 2 and 3 over gloo: strange_attractor_renderer_amd.distributed ITSELF — exchange_merge (rooted: all-reduce
MAX of depth keys + reduce SUM of counts / steps halves) and SlicedExchange / exchange_colorize (all-to-all of image
slices, merge in rank order, scalar all-reduce, sharded colorize, gather) — reproduces Runtime::merge folded in rank order
(reference src/lib.rs:708-738, 1068-1076), and job sharding covers every job once.

There is no HIP device here, so the Runtime and the exchange context handed to distributed.py are numpy stand-ins
(tests/exchange_numpy.py) for the exchange kernels of csrc/sar_image.hip (k_exch_export / _select / _import, k_exch_pack / _merge_slices / scalars, k_exch_flags /
_plan / _pack_sparse / _merge_sparse) working on the same raw buffers through the same pointers; the oracle stands in for the renderer. The process groups, the collectives, the
buffer geometry and the call sequence are the real ones; the HIP kernels run through the very same distributed.py
calls in tests/test_gpu_dist.py (-m gpu)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))       # (a spawned rank imports this module before it runs _worker)
from exchange_numpy import NumpyApi, NumpyExchange, NumpyRuntime, unsortable  # noqa: E402


def _worker(rank, world, port, W, H, jobs, n, seed, mode, q, scale=1.0):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as O
    import strange_attractor_renderer_amd as S
    from strange_attractor_renderer_amd import distributed as D
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = O.poisson_saturne()
    cfg.width, cfg.height, cfg.transparent, cfg.scale = W, H, 0, scale
    first, cnt = D.shard_jobs(jobs, world, rank)
    ort = O.Runtime(W, H)
    O.render_jobs(cfg, ort, O.start_points(seed, first, cnt), n)   # this rank's partial render (the oracle stands in for the GPU)
    rt = NumpyRuntime(ort, S.exchange_slice_pixels)
    npix = W * H
    if mode == "rooted":
        key = torch.empty(npix, dtype=torch.int64)
        sums = torch.empty(3 * npix, dtype=torch.int32)
        D.exchange_merge(NumpyExchange(rt, world, rank), dist, key, sums, dst=0)   # the real function, real collectives
        if rank == 0:
            q.put((rt.count.reshape(H, W).copy(), unsortable(rt.z).reshape(H, W).copy(), rt.steps.reshape(H, W).copy(), rt.max, None))
    else:
        # "sliced": whole slices; "sparse": records of the touched segments, whatever share of the image they are;
        # "auto": sparse unless more than half of the segments are touched
        ex = D.SlicedExchange(NumpyApi(O, S), cfg, rt, rank, world, "cpu", sparse=mode != "sliced",
                              dense_above=2.0 if mode == "sparse" else 0.5)
        img = D.exchange_colorize(ex, dist, dst=0)                  # pack, all-to-all, merge, scalars, colorize, gather
        f, c = ex.first, ex.count
        q.put((rank, f, c, rt.count[f:f + c].copy(), unsortable(rt.z[f:f + c]).copy(), rt.steps[f:f + c].copy(), rt.max,
               img.numpy().view(np.uint16).reshape(H, W, 4).copy() if rank == 0 else None, ex.bytes_on_the_wire()))
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn(world, mode, W, H, jobs, n, seed, n_results, scale=1.0):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, W, H, jobs, n, seed, mode, q, scale)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=240) for _ in range(n_results)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return got


def _fold_in_rank_order(oracle, W, H, jobs, n, seed, world, scale=1.0):
    from strange_attractor_renderer_amd.distributed import shard_jobs
    cfg = oracle.poisson_saturne()
    cfg.width, cfg.height, cfg.transparent, cfg.scale = W, H, 0, scale
    parts = []
    for r in range(world):
        first, cnt = shard_jobs(jobs, world, r)
        rt = oracle.Runtime(W, H)
        oracle.render_jobs(cfg, rt, oracle.start_points(seed, first, cnt), n)
        parts.append(rt)
    acc = parts[0]
    for other in parts[1:]:
        assert oracle.merge(acc, other) == 0
    return cfg, acc


@pytest.mark.timeout(300)
def test_exchange_merge_equals_merge_in_rank_order(oracle):
    W, H, jobs, n, seed, world = 96, 80, 37, 4000, 5, 2
    (count, zbuf, steps, mx, _), = _spawn(world, "rooted", W, H, jobs, n, seed, 1)
    cfg, acc = _fold_in_rank_order(oracle, W, H, jobs, n, seed, world)
    assert np.array_equal(count, acc.count)
    assert np.array_equal(zbuf.view(np.uint32), acc.zbuf.view(np.uint32))
    assert np.array_equal(steps.view(np.uint64), acc.steps.view(np.uint64))
    assert mx == acc.max
    # count (but not necessarily the tie-broken steps) is independent of the GPU count
    whole = oracle.Runtime(W, H)
    oracle.render_jobs(cfg, whole, oracle.start_points(seed, 0, jobs), n)
    assert np.array_equal(count, whole.count) and np.array_equal(zbuf.view(np.uint32), whole.zbuf.view(np.uint32))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world,mode,W,H,scale", [(2, "sliced", 97, 83, 1.0), (3, "sliced", 97, 83, 1.0), (2, "sparse", 97, 83, 1.0),
                                                  (3, "sparse", 97, 83, 1.0), (3, "auto", 150, 420, 0.3), (2, "auto", 97, 83, 1.0)])
def test_sliced_exchange_colorize_equals_merge_in_rank_order(oracle, world, mode, W, H, scale):
    """Dense slices, sparse records (forced, and chosen by the share of touched segments: a view that fills a tenth of a tall
    image leaves most segments untouched; one that covers the image goes dense) — the same merged frame."""
    jobs, n, seed = 41, 3000, 6                                    # npix % world != 0, jobs % world != 0
    got = _spawn(world, mode, W, H, jobs, n, seed, world, scale)
    cfg, acc = _fold_in_rank_order(oracle, W, H, jobs, n, seed, world, scale)
    count, zbuf, steps = np.zeros(W * H, np.uint32), np.zeros(W * H, np.float32), np.zeros(W * H)
    img, covered = None, 0
    wire = {r[0]: r[8] for r in got}
    got = [r[:8] for r in got]
    if mode == "sliced":
        assert all(w["form"] == "dense" for w in wire.values())
    elif mode == "sparse":
        assert all(w["form"] == "sparse" for w in wire.values())
    elif scale < 1.0:   # the attractor fills a small part of the image: few segments travel
        assert all(w["form"] == "sparse" and w["fraction_of_dense"] < 0.5 for w in wire.values()), wire
    else:
        assert all(w["form"] == "dense" for w in wire.values()), wire
    for rank, f, c, cs, zs, ss, mx, im in got:
        count[f:f + c], zbuf[f:f + c], steps[f:f + c] = cs, zs, ss
        covered += c
        assert mx == acc.max
        img = im if rank == 0 else img
    assert covered == W * H
    assert np.array_equal(count.reshape(H, W), acc.count)
    assert np.array_equal(zbuf.view(np.uint32).reshape(H, W), acc.zbuf.view(np.uint32))
    assert np.array_equal(steps.view(np.uint64).reshape(H, W), acc.steps.view(np.uint64))
    assert np.array_equal(img, oracle.colorize(cfg, acc))


def test_shard_jobs_partitions_exactly():
    from strange_attractor_renderer_amd.distributed import shard_jobs, slice_of
    for total in (0, 1, 7, 64, 65536, 524288, 1000003):
        for world in (1, 2, 3, 4, 8):
            seen = 0
            for r in range(world):
                first, cnt = shard_jobs(total, world, r)
                assert first == seen
                seen += cnt
            assert seen == total
    with pytest.raises(ValueError):
        shard_jobs(10, 2, 2)
    import strange_attractor_renderer_amd as S
    for npix in (1, 5, 4096, 2048 * 2048, 1800 * 2000, 4096 * 4096):
        for world in (1, 2, 3, 8):
            sp = S.exchange_slice_pixels(npix, world)
            assert sp % 4 == 0 and sp * world >= npix
            assert sum(slice_of(npix, world, r, sp)[1] for r in range(world)) == npix
