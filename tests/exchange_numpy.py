"""The exchange kernels of csrc/sar_image.hip and the exchange context of csrc/sar_exchange.cpp restated in numpy, on the same raw
buffers through the same pointers: what tests without a HIP device hand to distributed.py (tests/test_dist_gloo.py) and to the
driver of tests/exchange_cases.py (tests/test_exchange_cases_host.py) in place of api.Runtime / api.Exchange / the api module."""
import ctypes

import numpy as np

UNSET = np.uint32(0x407FFFFF)  # sortable(-1.0f)


def sortable(z32: np.ndarray) -> np.ndarray:
    b = (z32 + np.float32(0.0)).view(np.uint32)
    return np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)


def unsortable(s: np.ndarray) -> np.ndarray:
    b = np.where(s & 0x80000000, s & 0x7FFFFFFF, ~s).astype(np.uint32)
    return b.view(np.float32)


def _at(ptr, dtype, n):
    return np.ctypeslib.as_array((ctypes.c_uint8 * (n * np.dtype(dtype).itemsize)).from_address(ptr)).view(dtype)


class NumpyRuntime:
    """The exchange half of api.Runtime with numpy in place of the HIP kernels (same buffers, same layouts)."""

    def __init__(self, ort, slice_pixels_fn):
        self.W, self.H = ort.width, ort.height
        self.npix = self.W * self.H
        self.count = ort.count.ravel().copy()
        self.z = sortable(ort.zbuf.ravel())
        self.steps = ort.steps.ravel().copy()
        self.max, self.wrap = ort.max, 0
        self.zmax = self.zmin = None
        self._slice_pixels = slice_pixels_fn

    def dims(self):
        return self.W, self.H

    def synchronize(self):
        pass

    # ---- rooted form (k_exch_export / k_exch_select / k_exch_import) ----
    def _key(self, rank):
        k = (self.z.astype(np.uint64) << np.uint64(32)) | np.uint64(0xFFFFFFFF - rank)
        return (k ^ np.uint64(1 << 63)).view(np.int64)

    def exchange_export(self, rank, key_ptr):
        _at(key_ptr, np.int64, self.npix)[:] = self._key(rank)

    def exchange_select(self, rank, key_ptr, sum_ptr):
        red = _at(key_ptr, np.int64, self.npix)
        out = _at(sum_ptr, np.int32, 3 * self.npix)
        mine = self._key(rank) == red
        bits = np.where(mine, self.steps.view(np.uint64), np.uint64(0))
        out[:self.npix] = self.count.view(np.int32)
        out[self.npix::2] = (bits & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
        out[self.npix + 1::2] = (bits >> np.uint64(32)).astype(np.uint32).view(np.int32)

    def exchange_import(self, key_ptr, sum_ptr):
        red = _at(key_ptr, np.int64, self.npix)
        s = _at(sum_ptr, np.int32, 3 * self.npix)
        self.count = s[:self.npix].view(np.uint32).copy()
        self.z = ((red.view(np.uint64) ^ np.uint64(1 << 63)) >> np.uint64(32)).astype(np.uint32)
        lo = s[self.npix::2].view(np.uint32).astype(np.uint64)
        hi = s[self.npix + 1::2].view(np.uint32).astype(np.uint64)
        self.steps = (lo | (hi << np.uint64(32))).view(np.float64).copy()
        self.max = max(self.max, int(self.count.max()))

    # ---- sliced form (k_exch_pack / k_exch_merge_slices / scalars) ----
    def exchange_pack(self, world, out_ptr):
        S = self._slice_pixels(self.npix, world)
        out = _at(out_ptr, np.uint8, world * S * 16)
        for d in range(world):
            blk = out[d * S * 16:(d + 1) * S * 16]
            lo, hi = min(self.npix, d * S), min(self.npix, (d + 1) * S)
            c, z, st = np.zeros(S, np.uint32), np.full(S, UNSET, np.uint32), np.zeros(S, np.float64)
            c[:hi - lo], z[:hi - lo], st[:hi - lo] = self.count[lo:hi], self.z[lo:hi], self.steps[lo:hi]
            blk[:S * 4] = c.view(np.uint8)
            blk[S * 4:S * 8] = z.view(np.uint8)
            blk[S * 8:] = st.view(np.uint8)

    def exchange_merge_slices(self, world, rank, in_ptr):
        S = self._slice_pixels(self.npix, world)
        buf = _at(in_ptr, np.uint8, world * S * 16)
        lo, hi = min(self.npix, rank * S), min(self.npix, (rank + 1) * S)
        n = hi - lo
        parts = []
        for r in range(world):
            blk = buf[r * S * 16:(r + 1) * S * 16]
            parts.append((blk[:S * 4].view(np.uint32)[:n].copy(), blk[S * 4:S * 8].view(np.uint32)[:n].copy(),
                          blk[S * 8:].view(np.float64)[:n].copy()))
        c, z, st = parts[0]
        if rank != 0:
            self.max, self.wrap = 0, 0
        for oc, oz, ost in parts[1:]:
            c = c + oc                                           # wrapping u32, :719
            if n:
                self.max = max(self.max, int(c.max()))           # running max over every intermediate sum, :721-723
            take = oz > z                                        # strict: the earlier rank wins ties, :728
            z = np.where(take, oz, z)
            st = np.where(take, ost, st)
        self.count[lo:hi], self.z[lo:hi], self.steps[lo:hi] = c, z, st
        self._zrange(z)

    # ---- sparse form (k_exch_flags / k_exch_pack_sparse / k_exch_merge_sparse): records of the touched 64-pixel granules ----
    SEG = 64

    def _segments(self):
        nseg = (self.npix + self.SEG - 1) // self.SEG
        c, z, st = np.zeros(nseg * self.SEG, np.uint32), np.full(nseg * self.SEG, UNSET, np.uint32), np.zeros(nseg * self.SEG, np.float64)
        c[:self.npix], z[:self.npix], st[:self.npix] = self.count, self.z, self.steps
        return nseg, c.reshape(nseg, -1), z.reshape(nseg, -1), st.reshape(nseg, -1)

    def exchange_touched(self, ptr):
        nseg, c, z, _ = self._segments()
        _at(ptr, np.uint8, nseg)[:] = ((c != 0) | (z != UNSET)).any(axis=1)

    def exchange_pack_sparse(self, slot_ptr, out_ptr):
        nseg, c, z, st = self._segments()
        slot = _at(slot_ptr, np.int32, nseg)
        rec = self.SEG * 16
        for seg in np.nonzero(slot >= 0)[0]:
            blk = _at(out_ptr + int(slot[seg]) * rec, np.uint8, rec)
            blk[:self.SEG * 4] = c[seg].view(np.uint8)
            blk[self.SEG * 4:self.SEG * 8] = z[seg].view(np.uint8)
            blk[self.SEG * 8:] = st[seg].view(np.uint8)

    def exchange_merge_sparse(self, world, rank, slot_ptr, in_ptr):
        """k_exch_merge_sparse as it is written: a rank without a record for a granule is skipped — it holds the reset state there
        (count 0, zbuf unset) —, rank 0's record is taken as the accumulator, a granule nobody sent is left as it is."""
        S = self._slice_pixels(self.npix, world)
        sps, rec = S // self.SEG, self.SEG * 16
        slot = _at(slot_ptr, np.int32, world * sps).reshape(world, sps)
        lo, hi = min(self.npix, rank * S), min(self.npix, (rank + 1) * S)
        n = hi - lo
        c, z, st = np.zeros(S, np.uint32), np.full(S, UNSET, np.uint32), np.zeros(S, np.float64)
        sent = np.zeros(S, bool)
        if rank != 0:
            self.max, self.wrap = 0, 0
        for r in range(world):
            oc, oz, ost, here = np.zeros(S, np.uint32), np.full(S, UNSET, np.uint32), np.zeros(S, np.float64), np.zeros(S, bool)
            for s in np.nonzero(slot[r] >= 0)[0]:
                blk = _at(in_ptr + int(slot[r, s]) * rec, np.uint8, rec)
                px = slice(s * self.SEG, (s + 1) * self.SEG)
                oc[px], oz[px], ost[px] = blk[:self.SEG * 4].view(np.uint32), blk[self.SEG * 4:self.SEG * 8].view(np.uint32), blk[self.SEG * 8:].view(np.float64)
                here[px] = True
            c = c + np.where(here, oc, np.uint32(0))                 # rank 0: the accumulator; then wrapping adds, :719
            # strict: the earlier rank wins ties, :728. `r == 0`: rank 0 is the accumulator. (On every state a render produces the
            # clause changes nothing — a rank-0 record whose depth does not beat the initial -1.0 holds -1.0 and steps 0.0, the reset
            # state itself — so no test can tell the fold without it from this one: DESIGN.md section 5.)
            take = here & ((r == 0) | (oz > z))
            z, st = np.where(take, oz, z), np.where(take, ost, st)
            sent |= here
            if r != 0 and n:
                self.max = max(self.max, int(c[:n].max()))           # every intermediate sum — an absent rank's is the sum before it
        keep = sent[:n]
        self.count[lo:hi][keep], self.z[lo:hi][keep], self.steps[lo:hi][keep] = c[:n][keep], z[:n][keep], st[:n][keep]
        self._zrange(z[:n][keep])

    def _zrange(self, z):
        seen = z[z != UNSET]
        self.zmax = max(int(sortable(np.float32([0.0]))[0]), int(seen.max()) if seen.size else 0)
        self.zmin = min(int(sortable(np.float32([np.finfo(np.float32).max]))[0]), int(seen.min()) if seen.size else 2**32 - 1)

    def exchange_scalars_export(self, ptr):
        _at(ptr, np.int64, 4)[:] = [self.max, self.wrap, self.zmax, (~np.uint32(self.zmin)) & 0xFFFFFFFF]

    def exchange_scalars_import(self, ptr):
        v = _at(ptr, np.int64, 4)
        self.max, self.wrap, self.zmax = int(v[0]), int(v[1]), int(v[2])
        self.zmin = int(~np.uint32(v[3]) & 0xFFFFFFFF)


class NumpyExchange:
    """api.Exchange (the library's context object, csrc/sar_exchange.cpp) over a NumpyRuntime: the same geometry, the plan of the
    sparse form (k_exch_plan: where each of my records goes, where each record I receive arrives, the split sizes), the choice
    between sparse and dense, and the kernels' stand-ins above."""

    def __init__(self, rt, world, rank):
        self.runtime, self.world, self.rank = rt, world, rank
        self.slice_pixels = rt._slice_pixels(rt.npix, world)
        self.first = min(rt.npix, rank * self.slice_pixels)
        self.count = min(rt.npix, self.first + self.slice_pixels) - self.first
        self.granules = (rt.npix + rt.SEG - 1) // rt.SEG
        self.block_bytes = world * self.slice_pixels * 16
        self._sparse = False

    def flags(self, ptr):
        self.runtime.exchange_touched(ptr)

    def pack(self, flags_all_ptr, dense_above, send_ptr):
        world, rank, nseg, sps = self.world, self.rank, self.granules, self.slice_pixels // self.runtime.SEG
        sparse = False
        if flags_all_ptr:
            fa = _at(flags_all_ptr, np.uint8, world * nseg).reshape(world, nseg) != 0
            sparse = int(fa.sum()) <= dense_above * world * nseg
        self._sparse = sparse
        if not sparse:
            self.runtime.exchange_pack(world, send_ptr)
            return False, [self.slice_pixels * 16] * world, [self.slice_pixels * 16] * world
        fp = np.zeros((world, world * sps), bool)
        fp[:, :nseg] = fa
        mine = fp[rank]
        send_slot = np.where(mine, np.cumsum(mine) - 1, -1).astype(np.int32)[:nseg]
        sub = fp[:, rank * sps:(rank + 1) * sps].reshape(-1)
        self._recv_slot = np.where(sub, np.cumsum(sub) - 1, -1).astype(np.int32)
        self.runtime.exchange_pack_sparse(np.ascontiguousarray(send_slot).ctypes.data, send_ptr)
        rec = self.runtime.SEG * 16
        return True, [int(c) * rec for c in mine.reshape(world, sps).sum(axis=1)], [int(c) * rec for c in sub.reshape(world, sps).sum(axis=1)]

    def merge(self, recv_ptr, scalars_ptr):
        if self._sparse:
            self.runtime.exchange_merge_sparse(self.world, self.rank, self._recv_slot.ctypes.data, recv_ptr)
        else:
            self.runtime.exchange_merge_slices(self.world, self.rank, recv_ptr)
        self.runtime.exchange_scalars_export(scalars_ptr)

    def finish(self, scalars_ptr):
        self.runtime.exchange_scalars_import(scalars_ptr)

    def rooted(self, step, key_ptr, sum_ptr=0):
        if step == 0:
            self.runtime.exchange_export(self.rank, key_ptr)
        elif step == 1:
            self.runtime.exchange_select(self.rank, key_ptr, sum_ptr)
        else:
            self.runtime.exchange_import(key_ptr, sum_ptr)


class NumpyApi:
    """The api.* names SlicedExchange uses, for a NumpyRuntime: the exchange context above (slice geometry from the real library, a
    host function), colorize through the oracle with the GLOBAL max."""

    Exchange = NumpyExchange

    def __init__(self, O, S):
        self.O, self.S = O, S

    def exchange_slice_pixels(self, npix, world):
        return self.S.exchange_slice_pixels(npix, world)

    def colorize_range_device(self, cfg, rt, first, n, out_ptr):
        O = self.O
        if cfg.render_kind == O.SAR_RENDER_DEPTH:
            # k_colorize_depth: the range is the one the runtime's scalars hold (made global by the scalars' MAX), not this rank's own
            zmax, zmin = unsortable(np.uint32([rt.zmax]))[0], unsortable(np.uint32([rt.zmin]))[0]
            z = unsortable(rt.z[first:first + n])
            with np.errstate(all="ignore"):
                v = np.where(z == np.float32(-1.0), np.float32(0.0), (z - zmin) / (zmax - zmin)) * np.float32(65535.0)   # f32, :883-893
            v = np.where(v >= 65535.0, 65535, np.where(v > 0.0, v, 0.0)).astype(np.uint16)                                  # NaN -> 0
            img = np.stack([v, v, v, np.full(n, 65535, np.uint16)], axis=1)
            _at(out_ptr, np.uint16, n * 4)[:] = img.ravel()
            return
        ort = O.Runtime(rt.W, rt.H)
        ort.count[:] = rt.count.reshape(rt.H, rt.W)
        ort.steps[:] = rt.steps.reshape(rt.H, rt.W)
        ort.zbuf[:] = unsortable(rt.z).reshape(rt.H, rt.W)
        ort.set_max(0xFFFFFFFF if rt.wrap else rt.max)
        img = O.colorize(cfg, ort).reshape(-1, 4)
        _at(out_ptr, np.uint16, n * 4)[:] = img[first:first + n].ravel()
