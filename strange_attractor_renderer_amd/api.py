"""Host-side mirror of the reference crate's surface for the iterate/accumulate path, over the C ABI.

Names and argument meaning follow the reference (src/lib.rs):

    Config.poisson_saturne() / Config.solar_sail()      config presets           (:310, :355)
    Runtime(config)  .reset()  .merge(other)            Runtime                  (:631-739)
    render(config, runtime)                             one trajectory           (:747-838)
    colorize(config, runtime) -> HxWx4 uint16           FinalImage               (:841-904)
    ParallelRenderer(...) / .shutdown()                 thread pool -> GPU lanes (:908-1031)
    render_parallel(renderer, config, jobs_per_thread)  job split + merge        (:1051-1082)

plus what the reference hides: a seed, the job count, explicit start points and read-back accessors.
Everything here is plumbing (ctypes + numpy); all arithmetic runs in libsar_hip.so on the GPU.
There is no CPU fallback: without the library or without a HIP device these calls raise.
"""
from __future__ import annotations

import builtins
import ctypes as C
import weakref
import os
from dataclasses import dataclass

import numpy as np

from . import _abi
from ._abi import (SAR_CT_ADJUSTED_VELOCITY, SAR_CT_POISSON_SATURNE, SAR_RENDER_DEPTH,  # noqa: F401
                   SAR_RENDER_GAS, SarConfig, SarParallelTiming, SarTiming)


class SarError(RuntimeError):
    def __init__(self, status: int, where: str):
        lib = _abi.load_library()
        msg = lib.sar_last_error().decode(errors="replace")
        name = lib.sar_status_string(status).decode()
        super().__init__(f"{where}: {name} ({status}) {msg}")
        self.status = status


def _check(status: int, where: str):
    if status != _abi.SAR_OK:
        raise SarError(status, where)


def _lib():
    return _abi.load_library()


# ---- the ctypes plumbing every family shares --------------------------------------------------------------------------
_POINTERS = {np.dtype(t): C.POINTER(c) for t, c in ((np.uint8, C.c_uint8), (np.uint16, C.c_uint16), (np.uint32, C.c_uint32), (np.uint64, C.c_uint64),
                                                    (np.float32, C.c_float), (np.float64, C.c_double))}


def _ptr(arr, struct=None):
    """arr's data as the pointer its dtype names — a structured array passes its _abi class —; None stays None (NULL)."""
    if arr is None:
        return None
    return arr.ctypes.data_as(C.POINTER(struct) if struct is not None else _POINTERS[arr.dtype])


def _defaults(struct, default: str):
    """A `struct` as the library's `default` entry point (sar_x_params_default) fills it."""
    p = struct()
    _check(getattr(_lib(), default)(C.byref(p)), default)
    return p


def _field_value(ctype, v, where: str):
    """v as a field of `ctype` takes it: float(v) — or, for an integer type, int(v), refused when v is not integral or outside the
    type's range (ctypes would wrap it silently: steps=-1 would become 2^32-1)."""
    if ctype not in (C.c_uint16, C.c_uint32, C.c_uint64, C.c_int32):
        return float(v)
    bits = 8 * C.sizeof(ctype)
    lo, hi = (-2 ** (bits - 1), 2 ** (bits - 1) - 1) if ctype(-1).value < 0 else (0, 2 ** bits - 1)
    i = int(v)
    if i != v or not lo <= i <= hi:
        raise ValueError(f"{where}={v!r} must be an integer {lo}..{hi}")
    return i


def _fill(p, params: dict, allowed=None):
    """Sets the fields `params` names in the struct p, each by the rule of its ctype in p._fields_: a scalar through _field_value,
    an array from exactly its length of values. Settable are the scalar and array fields that do not start with "_" — of those,
    only the ones in `allowed` where it is given; any other key is an AttributeError that lists them. Returns p."""
    types, name = dict(p._fields_), type(p).__name__
    settable = [f for f, t in p._fields_ if not f.startswith("_") and not issubclass(t, C.Structure) and (allowed is None or f in allowed)]
    for k, v in params.items():
        if k not in settable:
            raise AttributeError(f"{name} has no settable field {k!r} ({', '.join(settable)})")
        t = types[k]
        if issubclass(t, C.Array):
            values = np.asarray(v, dtype=object).reshape(-1)
            if values.size != t._length_:
                raise ValueError(f"{name}.{k} takes {t._length_} values ({v!r})")
            getattr(p, k)[:] = [_field_value(t._type_, x, f"{name}.{k}") for x in values]
        else:
            setattr(p, k, _field_value(t, v, f"{name}.{k}"))
    return p


def _copy_struct(p, **fields):
    """A copy of the struct p with `fields` replaced."""
    q = type(p)()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(q))
    for k, v in fields.items():
        setattr(q, k, v)
    return q


def _stats_dict(st) -> dict:
    """The integer counters of a statistics struct by name (padding and array fields left out)."""
    return {f: int(getattr(st, f)) for f, t in st._fields_ if not f.startswith("_") and not issubclass(t, C.Array)}


def _mode_params(builder, off, params: dict):
    """The parameter argument of set_exposure / set_color_range: NULL for set_x(None) (off); `builder`'s struct, by reference, for
    set_x(**params) or set_x(dict) (on)."""
    if off is None:
        if params:
            raise ValueError("None turns the mode off: it takes no parameters")
        return None
    if off is not ...:
        params = {**dict(off), **params}
    return C.byref(builder(**params))


def _padded(lo: float, hi: float) -> tuple:
    """[lo, hi] widened by 2 % per side — by 0.5 where it is a single value."""
    pad = 0.02 * (hi - lo) if hi > lo else 0.5
    return lo - pad, hi + pad


def _hold_records(runtime, family: str, owner):
    """Notes that the device now holds `owner`'s records of `family` (None: nobody's). Weak: the owner holds the runtime."""
    setattr(runtime, "_last_" + family, None if owner is None else weakref.ref(owner))


def _colorize_records(owner, family: str, noun: str, shape, config, colors) -> np.ndarray:
    """sar_runtime_<family>_colorize: the (height, width, 4) RGBA16 picture of the records the runtime still holds for `owner`."""
    last = getattr(owner.runtime, "_last_" + family, None)
    if last is None or last() is not owner:
        raise ValueError(f"the runtime has computed another {noun} since this one: its records are gone from the device")
    out, entry = np.empty((*shape, 4), dtype=np.uint16), f"sar_runtime_{family}_colorize"
    _check(getattr(_lib(), entry)(C.byref(config.c), owner.runtime.handle, C.byref(colors), _ptr(out)), entry)
    return out


class Config:
    """``Config<PolynomialSprott2Degree, _>`` as a thin wrapper around ``struct sar_config``.

    Field names are the reference's; nested View/Colors fields are flattened
    (``scale``, ``center_camera``, ``brightness_offset`` ...)."""

    def __init__(self, c: SarConfig | None = None):
        self.c = c if c is not None else SarConfig()

    @classmethod
    def poisson_saturne(cls, **overrides) -> "Config":
        cfg = cls()
        _check(_lib().sar_config_poisson_saturne(C.byref(cfg.c)), "sar_config_poisson_saturne")
        return cfg.replace(**overrides)

    @classmethod
    def solar_sail(cls, **overrides) -> "Config":
        cfg = cls()
        _check(_lib().sar_config_solar_sail(C.byref(cfg.c)), "sar_config_solar_sail")
        return cfg.replace(**overrides)

    @classmethod
    def from_coefficients(cls, coeffs, base: "Config | None" = None) -> "Config":
        """``base`` (default solar_sail(): its AdjustedVelocity colours do not depend on the view) with the map's 30 coefficients
        replaced: (3, 10) rows x, y, z or 30 in that order — a search_candidate() or a search record's map. Frame it with
        frame_view()."""
        c = np.asarray(coeffs, dtype=np.float64).reshape(3, 10)
        return (base if base is not None else cls.solar_sail()).replace(coeff_x=c[0], coeff_y=c[1], coeff_z=c[2])

    def copy(self) -> "Config":
        return Config(_copy_struct(self.c))

    def replace(self, **kw) -> "Config":
        """``Config { iterations: ..., ..preset }`` update syntax (src/lib.rs:9-15)."""
        out = self.copy()
        for k, v in kw.items():
            if k == "render":
                k = "render_kind"
            if not hasattr(out.c, k):
                raise AttributeError(f"sar_config has no field {k!r}")
            cur = getattr(out.c, k)
            if isinstance(cur, C.Array):
                arr = np.asarray(v, dtype=np.float64)
                if k == "palette_rgb":
                    out.c.palette_len = arr.shape[0]
                    for i in range(arr.shape[0]):
                        for ch in range(3):
                            out.c.palette_rgb[i][ch] = float(arr[i, ch])
                else:
                    for i in range(len(cur)):
                        cur[i] = float(arr[i])
            else:
                setattr(out.c, k, v)
        return out

    def validate(self):
        _check(_lib().sar_config_validate(C.byref(self.c)), "sar_config_validate")

    def __getattr__(self, name):
        c = object.__getattribute__(self, "c")
        if hasattr(c, name):
            v = getattr(c, name)
            return np.ctypeslib.as_array(v).copy() if isinstance(v, C.Array) else v
        raise AttributeError(name)

    def rotation_matrix(self) -> np.ndarray:
        m = np.empty(9, dtype=np.float64)
        _check(_lib().sar_rotation_matrix(C.byref(self.c), _ptr(m)), "sar_rotation_matrix")
        return m.reshape(3, 3)


def start_points(seed: int, first_job: int, n_jobs: int) -> np.ndarray:
    """The start-point stream the reference leaves to OS entropy: (n_jobs, 3) f64, already * 0.1."""
    out = np.empty((n_jobs, 3), dtype=np.float64)
    _check(_lib().sar_start_points(seed, first_job, n_jobs, _ptr(out)), "sar_start_points")
    return out


def device_count() -> int:
    n = C.c_int(0)
    st = _lib().sar_device_count(C.byref(n))
    return int(n.value) if st == _abi.SAR_OK else 0


@dataclass
class Timing:
    iterate_ms: float
    resolve_ms: float
    colorize_ms: float
    merge_ms: float
    iterate_launches: int
    iterations_counted: int
    depth_atomics: int = 0
    warmup_ms: float = 0.0
    depth_candidates: int = 0


class Runtime:
    """``Runtime`` (src/lib.rs:631-646) living on one GPU."""

    def __init__(self, config: Config, device: int = 0, _borrowed=None):
        self._own = _borrowed is None
        if _borrowed is not None:
            self._h = _borrowed
        else:
            h = C.c_void_p()
            _check(_lib().sar_runtime_new(C.byref(config.c), device, C.byref(h)), "sar_runtime_new")
            self._h = h
            self._apply_environment()
        self.device = device

    def _apply_environment(self):
        # A/B and whole-suite test hook of THIS harness (the library itself reads no environment): SAR_SPLIT=1|2 forces
        # the whole or the split iterate kernel on every runtime created through it
        for env, opt in (("SAR_SPLIT", "split_waves"),):
            if os.environ.get(env, "") in ("1", "2"):
                _check(_lib().sar_runtime_set_option(self._h, opt.encode(), int(os.environ[env])), "sar_runtime_set_option")

    @classmethod
    def group(cls, config: Config, n: int, device: int = 0) -> list:
        """n runtimes for the frames of one batch (sar_runtime_new_group): one stream, one read-back stream, their buffers carved
        from one device and one page-locked allocation. Each is an ordinary Runtime; close them in any order."""
        handles = (C.c_void_p * n)()
        _check(_lib().sar_runtime_new_group(C.byref(config.c), device, n, handles), "sar_runtime_new_group")
        out = []
        for h in handles:
            rt = cls(config, device, _borrowed=C.c_void_p(h))
            rt._own = True
            rt._apply_environment()
            out.append(rt)
        return out

    def close(self):
        for ref in getattr(self, "_exchanges", []):       # contexts that borrow this runtime go first
            ex = ref()
            if ex is not None:
                ex.close()
        self._exchanges = []
        if getattr(self, "_h", None) and self._own:
            _lib().sar_runtime_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def dims(self):
        w, h = C.c_uint32(), C.c_uint32()
        _check(_lib().sar_runtime_dims(self._h, C.byref(w), C.byref(h)), "sar_runtime_dims")
        return int(w.value), int(h.value)

    def reset(self):
        _check(_lib().sar_runtime_reset(self._h), "sar_runtime_reset")

    def set_width_height(self, width: int, height: int):
        _check(_lib().sar_runtime_set_width_height(self._h, width, height), "sar_runtime_set_width_height")

    def seed(self, seed: int):
        _check(_lib().sar_runtime_seed(self._h, seed), "sar_runtime_seed")

    def merge(self, other: "Runtime"):
        _check(_lib().sar_runtime_merge(self._h, other._h), "sar_runtime_merge")

    def synchronize(self):
        _check(_lib().sar_runtime_synchronize(self._h), "sar_runtime_synchronize")

    # ---- read-back ------------------------------------------------------------------------------
    def _read_back(self, entry: str, dtype) -> np.ndarray:
        w, h = self.dims()
        out = np.empty((h, w), dtype=dtype)
        _check(getattr(_lib(), entry)(self._h, _ptr(out)), entry)
        return out

    def count(self) -> np.ndarray:
        return self._read_back("sar_runtime_count", np.uint32)

    def steps(self) -> np.ndarray:
        return self._read_back("sar_runtime_steps", np.float64)

    def zbuf(self) -> np.ndarray:
        return self._read_back("sar_runtime_zbuf", np.float32)

    def max(self) -> int:
        m = C.c_uint32()
        _check(_lib().sar_runtime_max(self._h, C.byref(m)), "sar_runtime_max")
        return int(m.value)

    def load(self, count: np.ndarray, steps: np.ndarray, zbuf: np.ndarray, max_: int):
        count = np.ascontiguousarray(count, dtype=np.uint32)
        steps = np.ascontiguousarray(steps, dtype=np.float64)
        zbuf = np.ascontiguousarray(zbuf, dtype=np.float32)
        _check(_lib().sar_runtime_load(self._h, _ptr(count), _ptr(steps), _ptr(zbuf), int(max_)), "sar_runtime_load")

    # ---- measurement / tuning -----------------------------------------------------------------------
    def enable_timing(self, on: bool = True):
        _check(_lib().sar_runtime_enable_timing(self._h, 1 if on else 0), "sar_runtime_enable_timing")

    def last_timing(self) -> Timing:
        t = SarTiming()
        _check(_lib().sar_runtime_last_timing(self._h, C.byref(t)), "sar_runtime_last_timing")
        return Timing(t.iterate_ms, t.resolve_ms, t.colorize_ms, t.merge_ms, t.iterate_launches,
                      t.iterations_counted, t.depth_atomics, t.warmup_ms, t.depth_candidates)

    def debug_spans(self, which: int = 0) -> list:
        """(hooks build) the individual HIP-event spans held since they were last read, in launch order: 0 iterate, 1 accumulate +
        fold, 2 warm-up (include/sar_test_hooks.h)."""
        hook = getattr(_lib(), "sar_runtime_debug_spans", None)
        if hook is None:
            raise RuntimeError("debug_spans is a test hook: load the hooks build (_abi.use_hooks_build())")
        n = C.c_uint32(0)
        _check(hook(self._h, which, None, 0, C.byref(n)), "sar_runtime_debug_spans")
        buf = (C.c_float * max(n.value, 1))()
        _check(hook(self._h, which, buf, n.value, C.byref(n)), "sar_runtime_debug_spans")
        return [float(buf[k]) for k in range(n.value)]

    def debug_colorize_launches(self) -> int:
        """(hooks build) the colorize kernels this runtime has enqueued, alone or as the leader of a batched run
        (include/sar_test_hooks.h)."""
        hook = getattr(_lib(), "sar_runtime_debug_colorize_launches", None)
        if hook is None:
            raise RuntimeError("debug_colorize_launches is a test hook: load the hooks build (_abi.use_hooks_build())")
        n = C.c_uint64(0)
        _check(hook(self._h, C.byref(n)), "sar_runtime_debug_colorize_launches")
        return int(n.value)

    def debug_load_volume(self, config: "Config", vol, z_range=(-1.0, 1.0), iterations: int = 1) -> "Volume":
        """(hooks build) the runtime holds `vol`, (slabs, height, width) u32 at config's and the runtime's size, as if volume() over
        z_range had produced it (include/sar_test_hooks.h); returns it as an ordinary Volume whose .add runs jobs of `iterations`."""
        hook, read = getattr(_lib(), "sar_runtime_debug_volume_load", None), getattr(_lib(), "sar_runtime_debug_volume_stats", None)
        if hook is None or read is None:
            raise RuntimeError("debug_load_volume is a test hook: load the hooks build (_abi.use_hooks_build())")
        vol = np.ascontiguousarray(vol, dtype=np.uint32)
        want = (config.c.height, config.c.width)
        if vol.ndim != 3 or vol.shape[1:] != want or want[::-1] != self.dims():    # no buffer of another size reaches the copy
            raise ValueError(f"vol must have shape (slabs, {want[0]}, {want[1]}) at the runtime's size {self.dims()}, got {vol.shape}")
        _check(hook(self._h, vol.shape[0], float(z_range[0]), float(z_range[1]), _ptr(vol)), "sar_runtime_debug_volume_load")
        st = _abi.SarVolumeStats()
        _check(read(self._h, C.byref(st)), "sar_runtime_debug_volume_stats")
        _hold_records(self, "volume", None)
        return Volume(self, config.copy(), volume_params(slabs=vol.shape[0], z_lo=z_range[0], z_hi=z_range[1]), iterations, _volume_stats(st))

    def debug_device_log(self, values) -> np.ndarray:
        """(hooks build) the kernels' own logarithm on `values`, as float64 of the same shape: float64 values through the device's
        log, uint32 values through ln_u32 with this runtime's table (include/sar_test_hooks.h). At most 2^20 values a call."""
        hook = getattr(_lib(), "sar_runtime_debug_device_log", None)
        if hook is None:
            raise RuntimeError("debug_device_log is a test hook: load the hooks build (_abi.use_hooks_build())")
        v = np.ascontiguousarray(values)
        if v.dtype not in (np.dtype(np.float64), np.dtype(np.uint32)):    # no guess at what an int64 or a float32 array meant
            raise TypeError(f"values must be float64 (log) or uint32 (ln_u32), got {v.dtype}")
        out = np.empty(v.shape, dtype=np.float64)
        _check(hook(self._h, 1 if v.dtype == np.uint32 else 0, v.ctypes.data, v.size, _ptr(out)), "sar_runtime_debug_device_log")
        return out

    def set_option(self, name: str, value: int):
        """A stable option (include/sar.h) — or, on the hooks build the test-suite loads, an A/B / test option
        (include/sar_test_hooks.h); the product library has no such entry point."""
        if name in _abi.STABLE_OPTIONS or name in _abi.VOLUME_OPTIONS:
            _check(_lib().sar_runtime_set_option(self._h, name.encode(), int(value)), f"sar_runtime_set_option({name})")
            return
        hook = getattr(_lib(), "sar_runtime_set_test_option", None)
        if hook is None:
            raise RuntimeError(f"option {name!r} is a test hook: load the hooks build (strange_attractor_renderer_amd._abi.use_hooks_build(), "
                               "or SAR_LIBRARY=tests/hooks/libsar_hip_hooks.so)")
        _check(hook(self._h, name.encode(), int(value)), f"sar_runtime_set_test_option({name})")

    def set_tuning(self, block_threads: int = 0, checkpoint_stride: int = 0, variant: int = 0, **more):
        """Convenience over set_option. variant: bits 0-3 path (0 automatic, 1 one atomic per visit, 3 binned), bits 8+
        debug_chunk_jobs."""
        if (variant >> 4) & 0xF:
            raise ValueError(f"variant {variant:#x}: bits 4-7 (the removed measurement modes) must be zero")
        self.set_option("block_threads", block_threads)
        self.set_option("checkpoint_stride", checkpoint_stride)
        hooks = hasattr(_lib(), "sar_runtime_set_test_option")
        if hooks or variant & 0xF:
            self.set_option("path", variant & 0xF)          # (test hooks: only the hooks build has them; 0 is the product's behaviour)
        if hooks or variant >> 8:
            self.set_option("debug_chunk_jobs", variant >> 8)
        for k, v in more.items():
            self.set_option(k, v)

    def describe_last_launch(self) -> str:
        """Which kernels the last render call really launched (sar_runtime_describe_last_launch)."""
        buf = C.create_string_buffer(512)
        _check(_lib().sar_runtime_describe_last_launch(self._h, buf, 512), "sar_runtime_describe_last_launch")
        return buf.value.decode()

    def stream(self) -> int:
        s = C.c_void_p()
        _check(_lib().sar_runtime_get_stream(self._h, C.byref(s)), "sar_runtime_get_stream")
        return int(s.value or 0)

    def set_stream(self, stream_ptr: int):
        _check(_lib().sar_runtime_set_stream(self._h, C.c_void_p(stream_ptr)), "sar_runtime_set_stream")

    def copy_stream(self) -> int:
        s = C.c_void_p()
        _check(_lib().sar_runtime_get_copy_stream(self._h, C.byref(s)), "sar_runtime_get_copy_stream")
        return int(s.value or 0)

    def set_copy_stream(self, stream_ptr: int):
        _check(_lib().sar_runtime_set_copy_stream(self._h, C.c_void_p(stream_ptr)), "sar_runtime_set_copy_stream")

    def share_streams(self, leader: "Runtime"):
        """This runtime enqueues where `leader` does (launch stream and read-back stream): the frames of one batch."""
        self.set_stream(leader.stream())
        self.set_copy_stream(leader.copy_stream())

    def set_exposure(self, off=..., /, **params):
        """Auto exposure on (sar_runtime_set_exposure): every whole-image Gas colorize of this runtime picks its brightness
        constants on the device from the frame's own counts (exposure_params: q_black, q_white, level_black, level_white).
        set_exposure(None) turns it off."""
        _check(_lib().sar_runtime_set_exposure(self._h, _mode_params(exposure_params, off, params)), "sar_runtime_set_exposure")

    def set_color_range(self, off=..., /, **params):
        """Auto colour range on (sar_runtime_set_color_range): every whole-image Gas colorize of this runtime picks its palette
        window on the device from the frame's own steps (color_range_params: q_lo, q_hi, pos_lo, pos_hi). Ends a hold.
        set_color_range(None) turns it off."""
        _check(_lib().sar_runtime_set_color_range(self._h, _mode_params(color_range_params, off, params)), "sar_runtime_set_color_range")

    def density_filter(self, stats: bool = True, **params) -> "dict | None":
        """Density estimation of this runtime's frame, in place (sar_runtime_density; density_params: samples): every pixel's count
        spreads over a kernel that narrows as the count grows, its hue becomes the mass-weighted mean. Returns the statistics
        (sar_density_stats as a dict) — or, with stats=False, None without waiting for the device: the call is only enqueued.
        Not idempotent: a second call filters the filtered frame. The order of a frame is render -> density_filter ->
        auto_exposure / color_range -> colorize, and merge comes before it."""
        p = density_params(**params)
        st = _abi.SarDensityStats() if stats else None
        _check(_lib().sar_runtime_density(self._h, C.byref(p), C.byref(st) if stats else None), "sar_runtime_density")
        return _stats_dict(st) if stats else None

    def shade(self, config: "Config", stats: bool = False, window: "ColorRange | None" = None, **params):
        """The shaded picture of this runtime's frame (sar_shade; shade_params: light, ambient, diffuse, specular, shininess_log2,
        ao_radius, ao_strength, ao_range, smooth, smooth_range, min_count, background): the depth buffer as a lit surface with ambient
        occlusion, in the palette's hues, as the (H, W, 4) uint16 array write_image accepts. window: a ColorRange the hues go through.
        With stats=True: (image, sar_shade_stats as a dict). The buffers are only read. The order of a frame is
        render -> [density_filter] -> shade."""
        p = shade_params(window=window, **params)
        out = np.empty((config.c.height, config.c.width, 4), dtype=np.uint16)
        st = _abi.SarShadeStats() if stats else None
        _check(_lib().sar_shade(C.byref(config.c), self._h, C.byref(p), C.byref(st) if stats else None, _ptr(out)), "sar_shade")
        return (out, _stats_dict(st)) if stats else out

    def density_tiles(self) -> tuple:
        """(tiles launched, tiles copied through) of the last density_filter (sar_runtime_density_tiles): a statistic of the launch
        shape, not of the picture. Waits for the device."""
        tiles, copied = C.c_uint32(), C.c_uint32()
        _check(_lib().sar_runtime_density_tiles(self._h, C.byref(tiles), C.byref(copied)), "sar_runtime_density_tiles")
        return int(tiles.value), int(copied.value)

    def hold_color_range(self, color_range: "ColorRange | None"):
        """One fixed window (a ColorRange, of color_range() or made by hand) for every whole-image Gas colorize of this runtime
        (sar_runtime_hold_color_range): the frames of a sweep keep their colours. Ends the mode. None turns it off."""
        c = None if color_range is None else color_range.c
        _check(_lib().sar_runtime_hold_color_range(self._h, C.byref(c) if c is not None else None), "sar_runtime_hold_color_range")


class Exchange:
    """The ONE exchange step before colorize of the one-process-per-GPU path (sar_exchange_*, include/sar.h): Runtime::merge
    (src/lib.rs:708-738) folded in rank order over image slices. The collectives are the caller's (distributed.py), on buffers the
    caller owns; all arguments are device pointers."""

    RECORD = 64 * 16   # bytes of one record of the sparse form (SAR_EXCHANGE_GRANULE pixels x 16 B)

    def __init__(self, runtime: Runtime, world: int, rank: int):
        h, lay = C.c_void_p(), _abi.SarExchangeLayout()
        _check(_lib().sar_exchange_new(runtime.handle, world, rank, C.byref(h), C.byref(lay)), "sar_exchange_new")
        self._h, self.runtime = h, runtime      # (the context borrows the runtime: Runtime.close closes its exchanges first)
        runtime._exchanges = getattr(runtime, "_exchanges", [])
        runtime._exchanges.append(weakref.ref(self))
        self.world, self.rank = world, rank
        self.slice_pixels, self.first, self.count = lay.slice_pixels, lay.first_px, lay.n_px
        self.granules, self.block_bytes = lay.granules, lay.block_bytes

    def close(self):
        if getattr(self, "_h", None):
            _lib().sar_exchange_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def flags(self, flags_dev_ptr: int):
        _check(_lib().sar_exchange_flags(self._h, C.c_void_p(flags_dev_ptr)), "sar_exchange_flags")

    def pack(self, flags_all_dev_ptr: int | None, dense_above: float, send_dev_ptr: int):
        """Plans (from the gathered flags; None: dense) and packs. Returns (sparse, send_bytes[world], recv_bytes[world]) — the
        one host wait of a frame's exchange."""
        sb, rb, sp = (C.c_uint64 * self.world)(), (C.c_uint64 * self.world)(), C.c_int(0)
        _check(_lib().sar_exchange_pack(self._h, C.c_void_p(flags_all_dev_ptr) if flags_all_dev_ptr else None, float(dense_above),
                                        C.c_void_p(send_dev_ptr), sb, rb, C.byref(sp)), "sar_exchange_pack")
        return bool(sp.value), [int(v) for v in sb], [int(v) for v in rb]

    def merge(self, recv_dev_ptr: int, scalars_dev_ptr: int):
        _check(_lib().sar_exchange_merge(self._h, C.c_void_p(recv_dev_ptr), C.c_void_p(scalars_dev_ptr)), "sar_exchange_merge")

    def finish(self, scalars_dev_ptr: int):
        _check(_lib().sar_exchange_finish(self._h, C.c_void_p(scalars_dev_ptr)), "sar_exchange_finish")

    def rooted(self, step: int, key_i64_dev_ptr: int, sum_i32_dev_ptr: int = 0):
        """sar_exchange_rooted: step 0 exports the keys (all-reduce MAX), step 1 the counts and the winner's steps halves (reduce SUM),
        step 2 (the root) takes the reduced buffers. count, zbuf and steps are Runtime::merge folded in rank order; max is
        max(rank 0's max, the final sums) — the fold's running maximum unless a pixel's count wraps u32 inside the fold of three or
        more ranks (per-rank counts 5, 0xFFFFFFF0, 0x20: the fold has seen 0xFFFFFFF5, this form reports max(rank 0's max, 0x15)).
        The sliced form (merge) keeps the exact running maximum."""
        _check(_lib().sar_exchange_rooted(self._h, step, C.c_void_p(key_i64_dev_ptr), C.c_void_p(sum_i32_dev_ptr) if sum_i32_dev_ptr else None),
               "sar_exchange_rooted")


def exchange_slice_pixels(npix: int, world: int) -> int:
    """Pixels per owned slice of the sliced multi-GPU exchange (the last slice may be shorter)."""
    s = C.c_uint32()
    _check(_lib().sar_exchange_slice_pixels(npix, world, C.byref(s)), "sar_exchange_slice_pixels")
    return int(s.value)


def bin_geometry(width: int, height: int, bin_shift: int = 0, bin_interleave: int = 0) -> dict:
    """The pixel -> (bin, record) map of the LDS-binned path for this image shape (host arithmetic, no device needed)."""
    out = (C.c_uint32 * 8)()
    _check(_lib().sar_bin_geometry(width, height, bin_shift, bin_interleave, out), "sar_bin_geometry")
    keys = ("ok", "bins", "bin_shift", "interleaved", "seg_shift", "bin_bits", "hi_shift", "low_mask")
    return dict(zip(keys, (int(v) for v in out)))


def colorize_range_device(config: Config, runtime: Runtime, first_px: int, n_px: int, rgba_dev_ptr: int):
    """colorize of a pixel range with the max / depth range the runtime's scalars hold (n_px*8 bytes out); stream-ordered."""
    _check(_lib().sar_colorize_range_device(C.byref(config.c), runtime.handle, first_px, n_px, C.c_void_p(rgba_dev_ptr)),
           "sar_colorize_range_device")


def _starts_ptr(starts, n_jobs: int):
    if starts is None:
        return None, None
    s = np.ascontiguousarray(starts, dtype=np.float64)
    if s.shape != (n_jobs, 3):
        raise ValueError(f"starts must have shape ({n_jobs}, 3), got {s.shape}")
    return s, _ptr(s)


def render(config: Config, runtime: Runtime):
    """``render(&config, &mut runtime)``: ONE trajectory of config.iterations (src/lib.rs:747)."""
    _check(_lib().sar_render(C.byref(config.c), runtime.handle), "sar_render")


def render_jobs(config: Config, runtime: Runtime, starts=None):
    """config.jobs_total trajectories of config.iterations // jobs_total each, with the sequential
    (job-major) semantics of calling ``render`` that many times on one un-reset runtime."""
    keep, ptr = _starts_ptr(starts, config.c.jobs_total)
    _check(_lib().sar_render_jobs(C.byref(config.c), runtime.handle, ptr), "sar_render_jobs")
    del keep


def render_jobs_batch(configs, runtimes, starts=None):
    """F frames of a sweep through ONE set of launches (sar_render_jobs_batch): frame i is ``render_jobs(configs[i],
    runtimes[i], starts[i])``, bit for bit — the frames share the chip instead of following each other."""
    n = len(configs)
    if len(runtimes) != n or (starts is not None and len(starts) != n):
        raise ValueError("configs, runtimes and starts must have the same length")
    cfgs = (C.POINTER(SarConfig) * n)(*[C.pointer(c.c) for c in configs])
    rts = (C.c_void_p * n)(*[r.handle for r in runtimes])
    keep, ptrs = [], None
    if starts is not None:
        ptrs = (C.POINTER(C.c_double) * n)()
        for i, (c, s) in enumerate(zip(configs, starts)):
            k, p = _starts_ptr(s, c.c.jobs_total)
            keep.append(k)
            if p is not None:
                ptrs[i] = p
    _check(_lib().sar_render_jobs_batch(n, cfgs, rts, ptrs), "sar_render_jobs_batch")
    del keep


def batch_frames(config: Config, runtime: "Runtime | None" = None) -> int:
    """How many frames like `config` fill the chip (sar_runtime_batch_frames): the length to call render_jobs_batch with; 1 = frames
    of this shape do not share launches. runtime None: the answer for a runtime yet to be made."""
    n = C.c_uint32()
    _check(_lib().sar_runtime_batch_frames(C.byref(config.c), runtime.handle if runtime is not None else None, C.byref(n)), "sar_runtime_batch_frames")
    return int(n.value)


def render_job_range(config: Config, runtime: Runtime, iters_per_job: int, starts):
    """A shard: the given jobs (explicit start points) with iters_per_job iterations each."""
    s = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
    _check(_lib().sar_render_job_range(C.byref(config.c), runtime.handle, s.shape[0], iters_per_job,
                                       _ptr(s)), "sar_render_job_range")


def render_job_range_device(config: Config, runtime: Runtime, n_jobs: int, iters_per_job: int, starts_dev_ptr: int):
    """The same shard with its start points already in device memory (n_jobs*3 float64, [job][xyz]); stream-ordered."""
    _check(_lib().sar_render_job_range_device(C.byref(config.c), runtime.handle, n_jobs, iters_per_job,
                                              C.c_void_p(starts_dev_ptr)), "sar_render_job_range_device")


def prefetch_device(config: Config, runtime: Runtime, n_jobs: int, iters_per_job: int, starts_dev_ptr: int):
    """Announces the next render_job_range_device call (same arguments): its warm-up may run ahead, under the tail of
    the frame in flight. Results do not depend on it."""
    _check(_lib().sar_runtime_prefetch_device(C.byref(config.c), runtime.handle, n_jobs, iters_per_job,
                                              C.c_void_p(starts_dev_ptr)), "sar_runtime_prefetch_device")


def colorize(config: Config, runtime: Runtime) -> np.ndarray:
    """``colorize(&config, &runtime) -> FinalImage`` as an (H, W, 4) uint16 array (src/lib.rs:841)."""
    out = np.empty((config.c.height, config.c.width, 4), dtype=np.uint16)
    _check(_lib().sar_colorize(C.byref(config.c), runtime.handle, _ptr(out)), "sar_colorize")
    return out


def reset_batch(runtimes):
    """Runtime::reset for every runtime of the list, in ONE launch where they share a stream (sar_runtime_reset_batch)."""
    n = len(runtimes)
    handles = (C.c_void_p * n)(*[rt.handle for rt in runtimes])
    _check(_lib().sar_runtime_reset_batch(n, handles), "sar_runtime_reset_batch")


def colorize_device_batch(configs, runtimes, rgba_dev_ptrs):
    """colorize of frame i = (configs[i], runtimes[i]) into rgba_dev_ptrs[i] (device memory), ONE launch for Gas frames of one
    palette on one stream (sar_colorize_device_batch)."""
    n = len(runtimes)
    cfgs = (C.POINTER(_abi.SarConfig) * n)(*[C.pointer(c.c) for c in configs])
    handles = (C.c_void_p * n)(*[rt.handle for rt in runtimes])
    outs = (C.c_void_p * n)(*[C.c_void_p(p) for p in rgba_dev_ptrs])
    _check(_lib().sar_colorize_device_batch(n, cfgs, handles, outs), "sar_colorize_device_batch")


def colorize_device(config: Config, runtime: Runtime, rgba_dev_ptr: int):
    """colorize into a caller-provided device buffer (H*W*8 bytes); stream-ordered, no host sync."""
    _check(_lib().sar_colorize_device(C.byref(config.c), runtime.handle, C.c_void_p(rgba_dev_ptr)),
           "sar_colorize_device")


def attractor_extent(config: Config, runtime: Runtime, n_jobs: int, iters_per_job: int, starts=None) -> np.ndarray:
    """The first pass the reference leaves as a TODO (src/lib.rs:326-333): ``[xmin, xmax, ymin, ymax, zmin, zmax]`` of
    the screen-space points followed by the same six numbers for the raw points."""
    out = np.zeros(12)
    keep, sp = _starts_ptr(starts, n_jobs)
    _check(_lib().sar_runtime_extent(C.byref(config.c), runtime.handle, n_jobs, iters_per_job, sp, _ptr(out)), "sar_runtime_extent")
    del keep
    return out


# ---- search for chaotic maps (include/sar.h: sar_runtime_search) -----------------------------------------------------
SEARCH_RECORD_DTYPE = np.dtype(_abi.SarSearchRecord)
SEARCH_STATUS = {_abi.SAR_SEARCH_BOUNDED: "bounded", _abi.SAR_SEARCH_DIVERGED: "diverged", _abi.SAR_SEARCH_DEGENERATE: "degenerate"}


def search_params(**params) -> "_abi.SarSearchParams":
    """sar_search_params_default() with the given fields replaced (seed, lo, hi, start, transient, steps, bound, min_lyapunov,
    min_ky_dim, keep_rejected)."""
    return _fill(_defaults(_abi.SarSearchParams, "sar_search_params_default"), params)


def search_candidate(seed: int, index: int, lo: float = -1.2, hi: float = 1.2) -> np.ndarray:
    """Candidate `index` of the search stream `seed`: its coefficients as (3, 10) rows x, y, z (host arithmetic)."""
    out = np.empty(30)
    _check(_lib().sar_search_candidate(seed, lo, hi, index, _ptr(out)), "sar_search_candidate")
    return out.reshape(3, 10)


def search_attractors(runtime: Runtime, n: int, first: int = 0, coeffs=None, cap: int | None = None, **params):
    """Sprott's search on the GPU: candidates [first, first + n) — generated from params["seed"], or the caller's coefficient
    sets coeffs[n][30] (or [n][3][10]) — screened through the transient, then Lyapunov spectrum and Kaplan-Yorke dimension of
    the survivors. Returns (records, stats): the accepted records (every phase-2 record with keep_rejected=1) sorted by
    candidate, at most `cap` of them (default all), as a SEARCH_RECORD_DTYPE array; stats counts the candidates by outcome and
    "records" is the number of records there were."""
    p = search_params(**params)
    keep = None
    if coeffs is not None:
        keep = np.ascontiguousarray(coeffs, dtype=np.float64).reshape(-1, 30)
        if keep.shape[0] != n:
            raise ValueError(f"coeffs must hold n = {n} sets of 30, got {keep.shape[0]}")
    cap = n if cap is None else int(cap)
    out = np.empty(max(cap, 1), dtype=SEARCH_RECORD_DTYPE)
    n_out = C.c_uint32()
    st = _abi.SarSearchStats()
    _check(_lib().sar_runtime_search(runtime.handle, C.byref(p), first, n, _ptr(keep), _ptr(out, _abi.SarSearchRecord), cap, C.byref(n_out),
                                     C.byref(st)), "sar_runtime_search")
    return out[:min(cap, n_out.value)].copy(), {**_stats_dict(st), "records": int(n_out.value)}


def frame_view(config: Config, runtime: Runtime, n_jobs: int, iters_per_job: int, margin: float = 0.05, sweep: bool = False,
               starts=None) -> Config:
    """config with its view framed on the attractor: attractor_extent (screen space, config's rotation), then sar_frame_view —
    center_camera on the middle of the extent and the largest scale that keeps it inside the image with `margin`; with
    `sweep`, inside at every angle of a turn."""
    ext = np.ascontiguousarray(attractor_extent(config, runtime, n_jobs, iters_per_job, starts)[:6])
    out = config.copy()
    _check(_lib().sar_frame_view(C.byref(out.c), _ptr(ext), margin, int(bool(sweep))), "sar_frame_view")
    return out


# ---- gallery: many maps as tiles of one atlas (include/sar.h: sar_runtime_gallery) ------------------------------------------
GALLERY_ITEM_DTYPE = np.dtype(_abi.SarGalleryItem)
GALLERY_STATS_DTYPE = np.dtype(_abi.SarGalleryStats)


def gallery_params(**params) -> "_abi.SarGalleryParams":
    """sar_gallery_params_default() (128 x 128 tiles, 8 per row, 1024 jobs, 2^20 iterations, seed 0) with the given fields
    replaced (tile_width, tile_height, cols, jobs, iterations, seed)."""
    return _fill(_defaults(_abi.SarGalleryParams, "sar_gallery_params_default"), params)


def frame_view_box(config: Config, raw_extent, margin: float = 0.05, sweep: bool = False) -> Config:
    """config with its view framed on a RAW bounding box [xmin, xmax, ymin, ymax, zmin, zmax] — a search record's `extent` — through
    sar_frame_view_box: no pass over the map. Conservative: the rotated box bounds the rotated attractor."""
    ext = np.ascontiguousarray(raw_extent, dtype=np.float64).reshape(6)
    out = config.copy()
    _check(_lib().sar_frame_view_box(C.byref(out.c), _ptr(ext), margin, int(bool(sweep))), "sar_frame_view_box")
    return out


def gallery_items(coeffs, views=None, *, base: Config, records=None, margin: float = 0.05, sweep: bool = False,
                  tile=None) -> np.ndarray:
    """The item array of gallery(): one GALLERY_ITEM_DTYPE entry per map of coeffs ([n][30] or [n][3][10]). A map's view is
    views[i] = (center_camera, scale), or comes from records[i]["extent"] (search records) through frame_view_box on `base` at
    the tile's size (`tile` = (width, height); default base's own size: the scale depends on the aspect ratio)."""
    c = np.ascontiguousarray(coeffs, dtype=np.float64).reshape(-1, 30)
    if (views is None) == (records is None):
        raise ValueError("give either views or records")
    items = np.zeros(c.shape[0], dtype=GALLERY_ITEM_DTYPE)
    items["coeff"] = c
    if views is not None:
        if len(views) != c.shape[0]:
            raise ValueError(f"views must hold one (center_camera, scale) per map ({c.shape[0]}), got {len(views)}")
        for i, (cc, scale) in enumerate(views):
            items["center_camera"][i] = np.asarray(cc, dtype=np.float64).reshape(3)
            items["scale"][i] = float(scale)
    else:
        if len(records) != c.shape[0]:
            raise ValueError(f"records must hold one search record per map ({c.shape[0]}), got {len(records)}")
        sized = base if tile is None else base.replace(width=int(tile[0]), height=int(tile[1]))
        for i in range(c.shape[0]):
            framed = frame_view_box(sized, records[i]["extent"], margin, sweep)
            items["center_camera"][i] = framed.center_camera
            items["scale"][i] = framed.scale
    return items


def gallery_atlas_shape(n: int, tile=(128, 128), cols: int = 8) -> tuple:
    """(rows, columns, 4) of the RGBA16 atlas of n tiles (width, height), `cols` per row: cols * tile_width by
    ceil(n / cols) * tile_height pixels."""
    if cols < 1:
        raise ValueError("cols must be at least 1")
    return (-(-int(n) // int(cols)) * int(tile[1]), int(cols) * int(tile[0]), 4)


class Gallery:
    """What gallery() made: `image` (atlas rows, atlas columns, 4) RGBA16 — write_image takes it —, `stats` (GALLERY_STATS_DTYPE,
    one per tile), `items`, `params`, `base`; with raw=True `count`, `zbuf`, `steps`, each (n, tile_height, tile_width)."""

    def __init__(self, base: Config, params, items: np.ndarray, image: np.ndarray, stats: np.ndarray, count=None, zbuf=None, steps=None):
        self.base, self.params, self.items, self.image, self.stats = base, params, items, image, stats
        self.count, self.zbuf, self.steps = count, zbuf, steps

    def __len__(self) -> int:
        return len(self.items)

    def tile(self, i: int) -> np.ndarray:
        """Tile i of the atlas: a (tile_height, tile_width, 4) view."""
        if not 0 <= i < len(self.items):
            raise IndexError(i)
        tw, th, cols = self.params.tile_width, self.params.tile_height, self.params.cols
        r, c = divmod(i, cols)
        return self.image[r * th:(r + 1) * th, c * tw:(c + 1) * tw]

    def config(self, i: int, **overrides) -> Config:
        """cfg_i of the contract — base with item i's map and view, the tile's size, iterations and jobs — ready for a full-size
        render() once width / height (and iterations) are overridden: the scale is relative to the width, so the framing holds
        for any size of the tile's aspect ratio."""
        it = self.items[i]
        cfg = self.base.replace(coeff_x=it["coeff"][:10], coeff_y=it["coeff"][10:20], coeff_z=it["coeff"][20:],
                                center_camera=it["center_camera"], scale=float(it["scale"]), width=self.params.tile_width,
                                height=self.params.tile_height, iterations=self.params.iterations, jobs_total=self.params.jobs)
        return cfg.replace(**overrides) if overrides else cfg


def gallery(runtime: Runtime, base: Config, items, *, tile=(128, 128), cols: int = 8, jobs: int = 1024, iterations: int = 1 << 20,
            seed: int = 0, starts=None, raw: bool = False) -> Gallery:
    """sar_runtime_gallery: every map of `items` (gallery_items) rendered as a tile (width, height) of one atlas, `cols` tiles per
    row, each tile what render_jobs + colorize give its Gallery.config(i) on a fresh runtime. `starts`: (jobs, 3) start points
    shared by the tiles (default the stream of `seed`). raw=True also returns the tiles' count / zbuf / steps."""
    it = np.ascontiguousarray(items, dtype=GALLERY_ITEM_DTYPE)
    n = it.shape[0]
    p = gallery_params(tile_width=tile[0], tile_height=tile[1], cols=cols, jobs=jobs, iterations=iterations, seed=seed)
    keep, sp = _starts_ptr(starts, p.jobs)
    tw, th = p.tile_width, p.tile_height
    image = np.zeros(gallery_atlas_shape(n, (tw, th), p.cols) if p.cols else (0, 0, 4), dtype=np.uint16)
    stats = np.zeros(n, dtype=GALLERY_STATS_DTYPE)
    count = np.zeros((n, th, tw), dtype=np.uint32) if raw else None
    zbuf = np.zeros((n, th, tw), dtype=np.float32) if raw else None
    steps = np.zeros((n, th, tw), dtype=np.float64) if raw else None
    _check(_lib().sar_runtime_gallery(runtime.handle, C.byref(base.c), C.byref(p), n, _ptr(it, _abi.SarGalleryItem), sp, _ptr(image),
                                      _ptr(count), _ptr(zbuf), _ptr(steps), _ptr(stats, _abi.SarGalleryStats)), "sar_runtime_gallery")
    del keep
    return Gallery(base, p, it, image, stats, count, zbuf, steps)


# ---- Lyapunov planes (include/sar.h: sar_runtime_plane) ------------------------------------------------------------------
PLANE_RECORD_DTYPE = np.dtype(_abi.SarPlaneRecord)
PLANE_MODES = {"l1": _abi.SAR_PLANE_L1, "spectrum": _abi.SAR_PLANE_SPECTRUM}


def _base_coeffs(base) -> np.ndarray:
    if isinstance(base, Config):
        return np.concatenate([base.coeff_x, base.coeff_y, base.coeff_z]).astype(np.float64)
    b = np.asarray(base, dtype=np.float64)
    if b.shape not in ((3, 10), (30,)):
        raise ValueError(f"base must be a Config or hold 30 coefficients as (3, 10) or (30,), got shape {b.shape}")
    return b.reshape(30)


def plane_params(base, axes, x_range, y_range, width: int, height: int, mode: str = "l1", **params) -> "_abi.SarPlaneParams":
    """sar_plane_params_default() filled in: the map `base` (a Config, or (3, 10) / (30,) coefficients), coefficient axes[0]
    swept over x_range along the columns and axes[1] over y_range along the rows (row 0 at the high end), mode "l1" or
    "spectrum", and any of start, transient, steps, bound."""
    (x_lo, x_hi), (y_lo, y_hi) = x_range, y_range
    p = _fill(_defaults(_abi.SarPlaneParams, "sar_plane_params_default"),
              dict(base=_base_coeffs(base), axis=axes, lo=(x_lo, y_lo), hi=(x_hi, y_hi), width=width, height=height))
    if mode not in PLANE_MODES:
        raise ValueError(f"mode must be one of {sorted(PLANE_MODES)}, got {mode!r}")
    p.mode = PLANE_MODES[mode]
    return _fill(p, params, allowed=("start", "transient", "steps", "bound"))


def plane_colors(**colors) -> "_abi.SarPlaneColors":
    """sar_plane_colors_default() (threshold 0, chaos_scale 0.25, order_scale 1) with the given fields replaced."""
    return _fill(_defaults(_abi.SarPlaneColors, "sar_plane_colors_default"), colors)


class LyapunovPlane:
    """One plane of sar_runtime_plane: `records` (height, width) of PLANE_RECORD_DTYPE, `stats` (counts by outcome), `params`."""

    def __init__(self, runtime: Runtime, params, records: np.ndarray, stats: dict):
        self.runtime, self.params, self.records, self.stats = runtime, params, records, stats
        self.mode = "spectrum" if params.mode == _abi.SAR_PLANE_SPECTRUM else "l1"

    @property
    def status(self) -> np.ndarray:
        return self.records["status"]

    @property
    def lyapunov(self) -> np.ndarray:
        """lambda_1 per pixel (height, width) in "l1" mode; the spectrum (height, width, 3), sorted descending, in "spectrum" mode.
        NaN where no step was folded."""
        return self.records["lyapunov"][..., 0] if self.mode == "l1" else self.records["lyapunov"]

    @property
    def ky_dim(self) -> np.ndarray:
        if self.mode != "spectrum":
            raise AttributeError("ky_dim needs the whole spectrum: mode=\"spectrum\"")
        return self.records["ky_dim"]

    def coeffs(self, x: int, y: int) -> np.ndarray:
        """Pixel (x, y)'s map as (3, 10) rows x, y, z (host arithmetic, the device's doubles): Config.from_coefficients takes it."""
        out = np.empty(30)
        _check(_lib().sar_plane_coeffs(C.byref(self.params), int(x), int(y), _ptr(out)), "sar_plane_coeffs")
        return out.reshape(3, 10)

    def colorize(self, config: Config, **colors) -> np.ndarray:
        """(height, width, 4) RGBA16 of the plane from config's palette (include/sar.h: sar_plane_colors), computed on the device
        from the records the runtime still holds; write_image takes it."""
        return _colorize_records(self, "plane", "plane", self.records.shape, config, plane_colors(**colors))


def lyapunov_plane(runtime: Runtime, base, axes, x_range, y_range, width: int, height: int, mode: str = "l1",
                   **params) -> LyapunovPlane:
    """A Lyapunov map of a coefficient plane on the GPU (sar_runtime_plane): the map `base` (a Config, or (3, 10) / (30,)
    coefficients) with coefficient axes[0] swept over x_range along the columns and axes[1] over y_range along the rows (row 0
    at the high end), one map per pixel through the search's transient and `steps` tangent steps. mode "l1": the growth of e1
    alone (lambda_max for a generic map); "spectrum": the whole spectrum and the Kaplan-Yorke dimension, as search_attractors
    gives them. params: start, transient, steps, bound."""
    p = plane_params(base, axes, x_range, y_range, width, height, mode, **params)
    rec = np.empty(max(int(width) * int(height), 1), dtype=PLANE_RECORD_DTYPE)
    st = _abi.SarPlaneStats()
    _hold_records(runtime, "plane", None)
    _check(_lib().sar_runtime_plane(runtime.handle, C.byref(p), rec.ctypes.data_as(C.c_void_p), C.byref(st)), "sar_runtime_plane")
    plane = LyapunovPlane(runtime, p, rec[:int(width) * int(height)].reshape(int(height), int(width)), _stats_dict(st))
    _hold_records(runtime, "plane", plane)
    return plane


# ---- period planes (include/sar.h: sar_runtime_period, sar_runtime_period_colorize) --------------------------------------
PERIOD_RECORD_DTYPE = np.dtype(_abi.SarPeriodRecord)


def period_params(base=None, axes=None, x_range=None, y_range=None, width: int = 256, height: int = 256, **params) -> "_abi.SarPeriodParams":
    """sar_period_params_default() filled in: the plane as plane_params takes it (`base`, `axes`, `x_range`, `y_range`; each may stay
    None — the default — for the list form, which ignores them), the size, and any of start, transient, max_period, bound, eps."""
    p = _defaults(_abi.SarPeriodParams, "sar_period_params_default")
    if base is not None:
        _fill(p, dict(base=_base_coeffs(base)))
    if axes is not None:
        _fill(p, dict(axis=axes))
    for k, r in enumerate((x_range, y_range)):
        if r is not None:
            p.lo[k], p.hi[k] = float(r[0]), float(r[1])
    _fill(p, dict(width=width, height=height))
    return _fill(p, params, allowed=("start", "transient", "max_period", "bound", "eps"))


def period_colors(colours=None) -> "_abi.SarPeriodColors":
    """sar_period_colors_default() (16 colours) with `colours` replaced where given."""
    c = _defaults(_abi.SarPeriodColors, "sar_period_colors_default")
    return c if colours is None else _fill(c, dict(colours=colours))


class PeriodPlane:
    """One plane of sar_runtime_period: `records` (height, width) of PERIOD_RECORD_DTYPE, `stats` (counts by outcome and the largest
    period), `params`, and `list_coeffs` — the (height, width, 30) coefficient sets of the list form, None for the sweep form."""

    def __init__(self, runtime: Runtime, params, records: np.ndarray, stats: dict, list_coeffs=None):
        self.runtime, self.params, self.records, self.stats, self.list_coeffs = runtime, params, records, stats, list_coeffs

    @property
    def status(self) -> np.ndarray:
        return self.records["status"]

    @property
    def period(self) -> np.ndarray:
        """(height, width) uint32: the step of the orbit's first return to within eps of the point after the transient; 0: none up
        to max_period (chaos, a quasi-periodic orbit, a cycle not yet settled) — or a DIVERGED pixel, which `status` tells apart."""
        return self.records["period"]

    def coeffs(self, x: int, y: int) -> np.ndarray:
        """Pixel (x, y)'s map as (3, 10) rows x, y, z (the device's doubles): Config.from_coefficients takes it."""
        if self.list_coeffs is not None:
            return (0.0 + 1.0 * self.list_coeffs[int(y), int(x)]).reshape(3, 10)
        out = np.empty(30)
        _check(_lib().sar_period_coeffs(C.byref(self.params), int(x), int(y), _ptr(out)), "sar_period_coeffs")
        return out.reshape(3, 10)

    def histogram(self) -> np.ndarray:
        """Pixels per period over the BOUNDED pixels: entry p counts period p (entry 0: bounded without a period), up to the largest
        period found."""
        return np.bincount(self.period[self.status == _abi.SAR_SEARCH_BOUNDED].astype(np.int64).ravel())

    def colorize(self, config: Config, colours=None) -> np.ndarray:
        """(height, width, 4) RGBA16 of the plane (include/sar.h: sar_period_colors): a diverged pixel transparent, a bounded one
        without a period black, period p the palette's slot (p - 1) % colours of `colours` (default 16) — computed on the device
        from the records the runtime still holds; write_image takes it."""
        return _colorize_records(self, "period", "period plane", self.records.shape, config, period_colors(colours))


def period_plane(runtime: Runtime, base=None, axes=None, x_range=None, y_range=None, width: int = 256, height: int = 256, *, coeffs=None,
                 **params) -> PeriodPlane:
    """The isoperiodic diagram of a coefficient plane on the GPU (sar_runtime_period): the plane of lyapunov_plane — the map `base`
    with coefficient axes[0] swept over x_range along the columns and axes[1] over y_range along the rows, row 0 at the high end —,
    one map per pixel through `transient` steps and then up to `max_period` more, until the orbit first returns to within `eps`
    (max norm) of the point the transient ended on: that step is the pixel's period. coeffs: (height, width, 30) or
    (height * width, 30) coefficient sets of the caller's own instead (base, axes and the ranges are then ignored) — a line of maps,
    a family that moves several coefficients together. params: start, transient, max_period, bound, eps."""
    p = period_params(base, axes, x_range, y_range, width, height, **params)
    w, h = int(width), int(height)
    cs = None
    if coeffs is not None:
        cs = np.ascontiguousarray(coeffs, dtype=np.float64)
        if cs.size != w * h * 30 or cs.shape[-1] != 30:
            raise ValueError(f"coeffs must hold {h} x {w} sets of 30 coefficients, got shape {cs.shape}")
        cs = cs.reshape(h, w, 30)
    elif base is None or axes is None or x_range is None or y_range is None:
        raise ValueError("give the plane (base, axes, x_range, y_range) or coeffs")
    rec = np.empty(max(w * h, 1), dtype=PERIOD_RECORD_DTYPE)
    st = _abi.SarPeriodStats()
    _hold_records(runtime, "period", None)
    _check(_lib().sar_runtime_period(runtime.handle, C.byref(p), _ptr(cs), _ptr(rec, _abi.SarPeriodRecord), C.byref(st)), "sar_runtime_period")
    plane = PeriodPlane(runtime, p, rec[:w * h].reshape(h, w), _stats_dict(st), cs)
    _hold_records(runtime, "period", plane)
    return plane


# ---- cycles (include/sar.h: sar_runtime_cycles, sar_cycles_starts, sar_cycle_charpoly) -------------------------------------------
CYCLES_RECORD_DTYPE = np.dtype(_abi.SarCyclesRecord)
CYCLE_ORBIT_DTYPE = np.dtype(_abi.SarCycleOrbit)
CYCLE_KINDS = ("sink", "saddle-1", "saddle-2", "source")   # by the number of multipliers outside the unit circle


def cycles_params(**params) -> "_abi.SarCyclesParams":
    """sar_cycles_params_default() with the given fields replaced (period, jobs, grid, max_newton, cap, box_lo, box_hi, tol, bound,
    merge, same)."""
    return _fill(_defaults(_abi.SarCyclesParams, "sar_cycles_params_default"), params)


def cycles_starts(params=None) -> np.ndarray:
    """(grid^3, 3) the lattice's start points (sar_cycles_starts: host arithmetic, the device's doubles); None: the defaults'."""
    p = cycles_params() if params is None else params
    out = np.empty((p.grid ** 3 if 0 < p.grid <= 16 else 1, 3))
    _check(_lib().sar_cycles_starts(C.byref(p), _ptr(out)), "sar_cycles_starts")
    return out


def cycle_charpoly(M) -> np.ndarray:
    """(trace, the sum of the principal 2 x 2 minors, the determinant) of a 3 x 3 M (sar_cycle_charpoly: host arithmetic)."""
    m = np.ascontiguousarray(M, dtype=np.float64).reshape(9)
    out = np.empty(3)
    _check(_lib().sar_cycle_charpoly(_ptr(m), _ptr(out)), "sar_cycle_charpoly")
    return out


def _host_next_point(c30: np.ndarray, p: np.ndarray) -> np.ndarray:
    """next_point on the host in numpy doubles, sum by sum left to right (numpy never contracts)."""
    x, y, z = (np.float64(v) for v in p)
    terms = (x, x * x, x * y, x * z, y, y * y, y * z, z, z * z)
    out = np.empty(3)
    with np.errstate(all="ignore"):
        for r in builtins.range(3):
            s = np.float64(c30[10 * r])
            for k, t in enumerate(terms):
                s = s + t * np.float64(c30[10 * r + 1 + k])
            out[r] = s
    return out


class Cycles:
    """What sar_runtime_cycles gave for n_maps maps: `records` (CYCLES_RECORD_DTYPE, one per map: the starts by outcome, the orbits kept
    and lost, the Newton iterations), the orbit slots behind orbits(m), `coeffs` (n_maps, 30) as canonicalised, `starts` (jobs, 3),
    `params`. The iteration is the plain Newton method, undamped; at a degenerate root one orbit may come back as two."""

    def __init__(self, params, coeffs: np.ndarray, starts: np.ndarray, records: np.ndarray, slots: np.ndarray):
        self.params, self.coeffs, self.starts, self.records, self._slots = params, coeffs, starts, records, slots

    def orbits(self, m: int = 0) -> np.ndarray:
        """Map m's orbits, CYCLE_ORBIT_DTYPE: rep, period (the minimal one), head, hits, newton, residual, M (9, row-major)."""
        return self._slots[m, :int(self.records["n_orbits"][m])]

    def points(self, m: int, k: int) -> np.ndarray:
        """(q, 3) the points of orbit k of map m: its representative stepped on the host q - 1 times."""
        o = self.orbits(m)[k]
        pts = [np.array(o["rep"], dtype=np.float64)]
        for _ in builtins.range(int(o["period"]) - 1):
            pts.append(_host_next_point(self.coeffs[m], pts[-1]))
        return np.stack(pts)

    def multipliers(self, m: int = 0) -> np.ndarray:
        """(n_orbits, 3) complex: the eigenvalues of every orbit's M by np.linalg.eigvals, largest modulus first — a convenience of this
        binding, not part of the contract and not held bit for bit."""
        o = self.orbits(m)
        lam = np.zeros((o.shape[0], 3), dtype=np.complex128)
        for k in builtins.range(o.shape[0]):
            ev = np.linalg.eigvals(o["M"][k].reshape(3, 3)).astype(np.complex128)
            lam[k] = ev[np.argsort(-np.abs(ev), kind="stable")]
        return lam

    def unstable_dim(self, m: int = 0) -> np.ndarray:
        """(n_orbits,) the number of multipliers with |lambda| > 1."""
        return (np.abs(self.multipliers(m)) > 1.0).sum(axis=1)

    def kind(self, m: int = 0) -> list:
        """Per orbit (name, flip): "sink", "saddle-1", "saddle-2" or "source" by unstable_dim, and whether a real multiplier lies
        below -1 (the orbit is past a period doubling)."""
        lam = self.multipliers(m)
        flip = ((lam.imag == 0.0) & (lam.real < -1.0)).any(axis=1)
        return [(CYCLE_KINDS[int(u)], bool(f)) for u, f in zip(self.unstable_dim(m), flip)]


def cycles(runtime: Runtime, coeffs, period: int = 1, starts=None, box=None, grid=None, *, search_seed: int = 0, search_lo: float = -1.2,
           search_hi: float = 1.2, **params) -> Cycles:
    """Fixed points and periodic orbits of maps on the GPU (sar_runtime_cycles): Newton's method on F^period(x) = x from every start,
    for every map, and the merge of what the starts found into orbits with their minimal period, hits and M = D F^q (its eigenvalues
    are the multipliers) — attracting or not. `coeffs`: what correlation_dimension takes (a Config, sets of 30 coefficients,
    search_attractors records). `starts` (jobs, 3) are shared by all maps; None: the lattice of grid^3 points (default 8) over box =
    (lo3, hi3) (default -2 .. 2). params: max_newton, cap, tol, bound, merge, same."""
    cs = _coeff_sets(coeffs, search_seed, search_lo, search_hi)
    kw = dict(params, period=period)
    if grid is not None:
        kw["grid"] = grid
    if box is not None:
        kw.update(box_lo=box[0], box_hi=box[1])
    s = None
    if starts is not None:
        s = np.ascontiguousarray(starts, dtype=np.float64)
        if s.ndim != 2 or s.shape[1] != 3:
            raise ValueError(f"starts must have shape (jobs, 3), got {s.shape}")
        kw["jobs"] = s.shape[0]
    p = cycles_params(**kw)
    m = cs.shape[0]
    recs = np.zeros(m, dtype=CYCLES_RECORD_DTYPE)
    slots = np.zeros((m, max(p.cap, 1)), dtype=CYCLE_ORBIT_DTYPE)
    _check(_lib().sar_runtime_cycles(runtime.handle, C.byref(p), m, _ptr(cs), _ptr(s), _ptr(recs, _abi.SarCyclesRecord),
                                     _ptr(slots, _abi.SarCycleOrbit)), "sar_runtime_cycles")
    return Cycles(p, 0.0 + 1.0 * cs, cycles_starts(p) if s is None else s, recs, slots)


# ---- unstable manifolds (include/sar.h: sar_runtime_manifold, sar_manifold_pixel) --------------------------------------------------
MANIFOLD_BRANCH_DTYPE = np.dtype(_abi.SarManifoldBranch)
MANIFOLD_RECORD_DTYPE = np.dtype(_abi.SarManifoldRecord)
MANIFOLD_NONE = 0xFFFFFFFF   # `first` of a pixel no branch plotted; first_long_step of a branch without a long segment
MANIFOLD_COLOURS = ((65535, 16384, 16384, 65535), (16384, 40960, 65535, 65535), (65535, 53248, 8192, 65535), (16384, 65535, 24576, 65535))


def manifold_params(**params) -> "_abi.SarManifoldParams":
    """sar_manifold_params_default() with the given fields replaced (samples, steps, max_span, bound)."""
    return _fill(_defaults(_abi.SarManifoldParams, "sar_manifold_params_default"), params)


def manifold_pixel(config: Config, xyz) -> np.ndarray:
    """(fi, fj) of a point in config's view (sar_manifold_pixel: host arithmetic, the device's doubles): inside the image,
    (floor(fi), floor(fj)) is the pixel render gives the point."""
    p = np.ascontiguousarray(xyz, dtype=np.float64).reshape(3)
    out = np.empty(2)
    _check(_lib().sar_manifold_pixel(C.byref(config.c), _ptr(p), _ptr(out)), "sar_manifold_pixel")
    return out


def manifold_branches(cycles: "Cycles", m: int = 0, delta: float = 1e-6):
    """The branches of the 1-D unstable manifolds of map m's orbits in `cycles`, as manifolds() takes them, and each branch's orbit
    index: (MANIFOLD_BRANCH_DTYPE array, int array). An orbit takes part when exactly one multiplier lies outside the unit circle and
    it is real. `base` is the orbit's representative and `dir` that multiplier's eigenvector from np.linalg.eig(M), of unit length,
    its largest component made positive — a convenience of this binding, not held bit for bit. A positive multiplier gives two
    branches, +delta and -delta, with period q; a negative one gives one branch with period 2 q (the other side appears at the odd
    returns)."""
    orbits, out, index = cycles.orbits(m), [], []
    for k in builtins.range(orbits.shape[0]):
        lam, vec = np.linalg.eig(orbits["M"][k].reshape(3, 3))
        outside = np.flatnonzero(np.abs(lam) > 1.0)
        if outside.size != 1 or np.imag(lam[outside[0]]) != 0.0:
            continue
        v = np.real(vec[:, outside[0]]).astype(np.float64)
        v = v / np.sqrt(np.sum(v * v))
        if v[np.argmax(np.abs(v))] < 0.0:
            v = -v
        q, negative = int(orbits["period"][k]), np.real(lam[outside[0]]) < 0.0
        for sign in ((1.0,) if negative else (1.0, -1.0)):
            out.append((tuple(orbits["rep"][k]), tuple(v), sign * delta, 2 * q if negative else q, 0))
            index.append(k)
    return np.array(out, dtype=MANIFOLD_BRANCH_DTYPE), np.array(index, dtype=np.int64)


class Manifolds:
    """What sar_runtime_manifold drew: `count` (height, width) u32, the plots per pixel; `first` (height, width) u32, the smallest
    step * 4096 + branch that plotted the pixel (MANIFOLD_NONE: none); `records` (MANIFOLD_RECORD_DTYPE, one per branch: status, the
    fundamental domain's ends a and b, the segments by class, pixels, length_px, first_long_step, alive_end); `branches`; `params`.
    Only 1-D unstable manifolds are drawn; a stable manifold is the unstable one of the inverse map, where that is quadratic."""

    def __init__(self, params, branches: np.ndarray, count: np.ndarray, first: np.ndarray, records: np.ndarray):
        self.params, self.branches, self.count, self.first, self.records = params, branches, count, first, records

    @property
    def age(self) -> np.ma.MaskedArray:
        """(height, width) the step at which the manifold first reached the pixel, masked where it never did."""
        return np.ma.masked_array(self.first // 4096, mask=self.first == MANIFOLD_NONE)

    @property
    def branch(self) -> np.ma.MaskedArray:
        """(height, width) the branch that reached the pixel first (of equal branches the lower index), masked where none did."""
        return np.ma.masked_array(self.first % 4096, mask=self.first == MANIFOLD_NONE)

    def overlay(self, image: np.ndarray, colours=MANIFOLD_COLOURS) -> np.ndarray:
        """A copy of `image` — a (height, width, 4) RGBA16 frame of the same view — with every manifold pixel painted in the colour
        of the branch that reached it first: one RGBA per branch, cycling through `colours`. Host numpy; `image` itself is left
        alone, and so is every pixel the manifold did not plot."""
        if image.shape != (*self.count.shape, 4):
            raise ValueError(f"the image must be {(*self.count.shape, 4)}, got {image.shape}")
        table = np.asarray(colours, dtype=np.uint16).reshape(-1, 4)
        out = image.copy()
        hit = self.first != MANIFOLD_NONE
        out[hit] = table[(self.first[hit] % 4096) % table.shape[0]]
        return out

    def colorize(self, colours=MANIFOLD_COLOURS) -> np.ndarray:
        """The overlay on opaque black: (height, width, 4) RGBA16."""
        black = np.zeros((*self.count.shape, 4), dtype=np.uint16)
        black[..., 3] = 65535
        return self.overlay(black, colours)


def manifolds(runtime: Runtime, config: Config, branches, samples: int = 4096, steps: int = 32, max_span: int = 16,
              bound: float = 1e6) -> Manifolds:
    """The unstable manifolds of saddle cycles on the GPU (sar_runtime_manifold): every branch's fundamental domain, `samples` points
    between a = base + delta * dir and b = F^period(a), stepped `steps` times under config's map; at every step the segments between
    neighbouring samples are drawn into config's view (its camera and its width x height, which need not be the runtime's).
    `branches`: a MANIFOLD_BRANCH_DTYPE array — manifold_branches() makes one from cycles() — or rows (base3, dir3, delta, period).
    A segment longer than `max_span` pixels is counted (records["n_long"]) and not drawn: raise `samples` where that happens early."""
    if isinstance(branches, np.ndarray) and branches.dtype == MANIFOLD_BRANCH_DTYPE:
        br = np.ascontiguousarray(branches).reshape(-1)
    else:
        br = np.zeros(len(branches), dtype=MANIFOLD_BRANCH_DTYPE)
        for k, (base, direction, delta, period) in enumerate(branches):
            br[k] = (tuple(np.asarray(base, dtype=np.float64)), tuple(np.asarray(direction, dtype=np.float64)), float(delta),
                     _field_value(C.c_uint32, period, "period"), 0)
    p = manifold_params(samples=samples, steps=steps, max_span=max_span, bound=bound)
    h, w = int(config.c.height), int(config.c.width)
    count, first = np.zeros((h, w), dtype=np.uint32), np.full((h, w), MANIFOLD_NONE, dtype=np.uint32)
    recs = np.zeros(br.shape[0], dtype=MANIFOLD_RECORD_DTYPE)
    _check(_lib().sar_runtime_manifold(runtime.handle, C.byref(config.c), C.byref(p), br.shape[0], _ptr(br, _abi.SarManifoldBranch),
                                       _ptr(count), _ptr(first), _ptr(recs, _abi.SarManifoldRecord)), "sar_runtime_manifold")
    return Manifolds(p, br, count, first, recs)


# ---- orbit diagrams (include/sar.h: sar_runtime_orbit) -------------------------------------------------------------------
ORBIT_COLUMN_DTYPE = np.dtype(_abi.SarOrbitColumn)


def orbit_params(a, b=None, *, axis=None, range=None, v_range=None, **params) -> "_abi.SarOrbitParams":
    """sar_orbit_params_default() filled in: the line from map `a` to map `b` (each a Config, or (3, 10) / (30,) coefficients; b None:
    a's), with axis=k, range=(lo, hi) the single-axis shorthand — entry k runs from lo to hi, everything else as given —, v_range =
    (v_lo, v_hi) the plotted window, and any of width, height, jobs, transient, steps, seed, bound, proj."""
    p = _defaults(_abi.SarOrbitParams, "sar_orbit_params_default")
    av = _base_coeffs(a).copy()
    bv = av.copy() if b is None else _base_coeffs(b).copy()
    if (axis is None) != (range is None):
        raise ValueError("axis and range go together")
    if b is None and axis is None:
        raise ValueError("give the other end of the line: b, or axis and range")
    if axis is not None:
        if not 0 <= int(axis) < 30:
            raise ValueError(f"axis must be a coefficient index 0..29, got {axis!r}")
        av[int(axis)], bv[int(axis)] = float(range[0]), float(range[1])
    _fill(p, dict(a=av, b=bv))
    if v_range is not None:
        _fill(p, dict(v_lo=v_range[0], v_hi=v_range[1]))
    return _fill(p, params, allowed=("width", "height", "jobs", "transient", "steps", "seed", "bound", "proj"))


def _run_orbit(runtime: Runtime, p, starts):
    keep, sp = _starts_ptr(starts, p.jobs)
    count = np.empty((max(p.height, 1), max(p.width, 1)), dtype=np.uint32)
    stats = np.empty(max(p.width, 1), dtype=ORBIT_COLUMN_DTYPE)
    m = C.c_uint32()
    _check(_lib().sar_runtime_orbit(runtime.handle, C.byref(p), sp, _ptr(count), _ptr(stats, _abi.SarOrbitColumn), C.byref(m)),
           "sar_runtime_orbit")
    del keep
    return count, stats, int(m.value)


class OrbitDiagram:
    """One diagram of sar_runtime_orbit: `count` (height, width) uint32 with row 0 at the high end of `v_range`, `max` its largest bin,
    `stats` (ORBIT_COLUMN_DTYPE, one per column), `params`."""

    def __init__(self, params, count: np.ndarray, stats: np.ndarray, max_: int, device: int = 0):
        self.params, self.count, self.stats, self.max, self.device = params, count, stats, int(max_), device

    @property
    def v_range(self) -> tuple:
        return (self.params.v_lo, self.params.v_hi)

    def coeffs(self, c: int) -> np.ndarray:
        """Column c's map as (3, 10) rows x, y, z (host arithmetic, the device's doubles): Config.from_coefficients takes it."""
        out = np.empty(30)
        _check(_lib().sar_orbit_coeffs(C.byref(self.params), int(c), _ptr(out)), "sar_orbit_coeffs")
        return out.reshape(3, 10)

    def _steps(self, hue) -> np.ndarray:
        h, w = self.count.shape
        col = np.zeros(w) if hue is None else np.broadcast_to(np.asarray(hue, dtype=np.float64), (w,))
        return np.ascontiguousarray(np.broadcast_to(col[None, :], (h, w)))

    def load(self, runtime: Runtime, hue=None):
        """The diagram as the state of a runtime of its size (Runtime.load): the counts, `steps` = `hue`, a palette position per
        column (a scalar or `width` values, default 0) broadcast down the column, zbuf 0, max. exposure / auto_exposure / colorize
        then treat it as any Gas frame."""
        h, w = self.count.shape
        if runtime.dims() != (w, h):
            raise ValueError(f"the runtime is {runtime.dims()}, the diagram {(w, h)}")
        runtime.load(self.count, self._steps(hue), np.zeros((h, w), dtype=np.float32), self.max)

    def colorize(self, config: Config, hue=None, exposure={}) -> np.ndarray:
        """(height, width, 4) RGBA16 of the diagram with config's palette and colour constants: a runtime of the diagram's size on the
        diagram's device, load(hue), auto_exposure(**exposure), then the Gas colorize. write_image takes it."""
        h, w = self.count.shape
        cfg = config.replace(width=w, height=h, render_kind=SAR_RENDER_GAS)
        rt = Runtime(cfg, device=self.device)
        try:
            self.load(rt, hue)
            return colorize(auto_exposure(cfg, rt, **exposure), rt)
        finally:
            rt.close()

    def lyapunov(self, runtime: Runtime, **params) -> np.ndarray:
        """lambda_1 of every column's map, (width,): search_attractors on the columns' own coefficients with keep_rejected (params:
        start, transient, steps, bound of the search); NaN where the column has no record (it left the bound box in the search's
        transient) or no step was folded. A family whose Jacobian is singular everywhere — a one- or two-dimensional map written
        into the three rows, the logistic family for one — is DEGENERATE at the spectrum's first step; such a column gets the growth
        of e1 instead, from a one-pixel lyapunov_plane in "l1" mode (one small call per such column; the runtime's last plane is
        then that pixel). hue = clip((lambda_1 - threshold) / chaos_scale) paints periodic windows and chaos in different colours."""
        w = self.params.width
        cs = np.stack([self.coeffs(c).reshape(30) for c in builtins.range(w)])
        recs, _ = search_attractors(runtime, w, coeffs=cs, **{**params, "keep_rejected": 1})
        lam = np.full(w, np.nan)
        lam[recs["candidate"]] = recs["lyapunov"][:, 0]
        flat = recs[(recs["status"] == _abi.SAR_SEARCH_DEGENERATE) & np.isnan(recs["lyapunov"][:, 0])]
        plane_kw = {k: params[k] for k in ("start", "transient", "steps", "bound") if k in params}
        for c in flat["candidate"]:
            k = cs[int(c)]
            lam[int(c)] = lyapunov_plane(runtime, k, (0, 1), (k[0], k[0]), (k[1], k[1]), 1, 1, "l1", **plane_kw).lyapunov[0, 0]
        return lam


    def period(self, runtime: Runtime, **params) -> np.ndarray:
        """The period of every column's map, (width,) int64: period_plane's list form on the columns' own coefficients (params: start,
        transient, max_period, bound, eps). 0: no period up to max_period (chaos, or a cycle still converging next to a bifurcation);
        -1: the column left the bound box. hue = ((period - 1) % colours + 0.5) / colours paints the windows by period."""
        w = self.params.width
        cs = np.stack([self.coeffs(c).reshape(30) for c in builtins.range(w)])
        pl = period_plane(runtime, width=w, height=1, coeffs=cs, **params)
        return np.where(pl.status[0] == _abi.SAR_SEARCH_BOUNDED, pl.period[0].astype(np.int64), -1)

    def cycles(self, runtime: Runtime, period: int = 1, **params) -> "Cycles":
        """The cycles of every column's map (cycles() on the columns' own coefficients; params: starts, box, grid and those of
        sar_cycles_params): map c of the result is column c. overlay() draws them into the diagram's picture."""
        w = self.params.width
        cs = np.stack([self.coeffs(c).reshape(30) for c in builtins.range(w)])
        return cycles(runtime, cs, period, **params)

    def spectrum(self, runtime: Runtime, **params) -> "Spectrum":
        """The power spectrum of every column's map (power_spectrum on the columns' own coefficients with the diagram's proj; params:
        starts and those of sar_spectrum_params): map c of the result is column c. Its colorize is the spectral bifurcation diagram
        that goes with this one — the subharmonic lines of a period-doubling cascade, then the broadband floor —, its flatness a hue
        for colorize here."""
        w = self.params.width
        cs = np.stack([self.coeffs(c).reshape(30) for c in builtins.range(w)])
        return power_spectrum(runtime, cs, **{"proj": tuple(self.params.proj), **params})

    def recurrence(self, runtime: Runtime, **params) -> "Recurrence":
        """The recurrence analysis of every column's map (recurrence_analysis on the columns' own coefficients; params: starts and those
        of sar_rqa_params): map c of the result is column c. Along a line of maps .det and .lam mark the periodic windows and the
        laminar phases next to them."""
        w = self.params.width
        cs = np.stack([self.coeffs(c).reshape(30) for c in builtins.range(w)])
        return recurrence_analysis(runtime, cs, **params)

    def overlay(self, image: np.ndarray, cycles: "Cycles", stable=(0, 65535, 0, 65535), unstable=(65535, 0, 0, 65535)) -> np.ndarray:
        """A copy of `image` — the (height, width, 4) RGBA16 that colorize returned — with every point of every orbit of `cycles` (from
        self.cycles) painted at (column, the diagram's bin of proj . point): `stable` where no multiplier lies outside the unit circle,
        `unstable` otherwise — the dashed branches of a textbook bifurcation diagram. The row is the diagram's own arithmetic: v =
        (proj0 x + proj1 y) + proj2 z, u = (v - v_lo) * scale with scale = height / (v_hi - v_lo), row = height - 1 - (uint32)u where
        0 <= u < height; other points are not drawn. Host numpy; `image` itself is left alone."""
        h, w = self.count.shape
        if image.shape != (h, w, 4) or len(cycles.records) != w:
            raise ValueError(f"the image must be {(h, w, 4)} and the cycles one map per column ({w})")
        out = image.copy()
        p0, p1, p2 = (np.float64(v) for v in self.params.proj)
        v_lo, scale = np.float64(self.params.v_lo), np.float64(h) / (np.float64(self.params.v_hi) - np.float64(self.params.v_lo))
        for c in builtins.range(w):
            dims = cycles.unstable_dim(c)
            for k in builtins.range(len(dims)):
                for x, y, z in cycles.points(c, k):
                    u = ((p0 * x + p1 * y) + p2 * z - v_lo) * scale
                    if u >= 0.0 and u < h:
                        out[h - 1 - int(u), c] = stable if dims[k] == 0 else unstable
        return out


def orbit_diagram(runtime: Runtime, a, b=None, *, axis=None, range=None, width=None, height=None, jobs=None, steps=None, transient=None,
                  proj=None, v_range=None, seed=0, starts=None, bound=None) -> OrbitDiagram:
    """The orbit (bifurcation) diagram of a line of maps on the GPU (sar_runtime_orbit): column c is the map a + (b - a) c / (width - 1)
    — `a`, `b` a Config or (3, 10) / (30,) coefficients; axis=k, range=(lo, hi) sweeps entry k alone —, every column runs `jobs`
    trajectories (`starts` (jobs, 3), default the stream of `seed`) through `transient` uncounted and `steps` counted steps, and each
    counted point adds 1 to the bin of v = proj . (x, y, z) among `height` bins over v_range, row 0 at the high end. v_range=None
    costs a second run: a first call with height=1 learns vmin / vmax over all columns, and the diagram uses that span widened by
    2 % per side. Sizes left None are sar_orbit_params_default's (1024 x 512, 256 jobs, 1000 + 4096 steps, proj (1, 0, 0))."""
    kw = {k: v for k, v in dict(width=width, height=height, jobs=jobs, steps=steps, transient=transient, proj=proj, bound=bound).items()
          if v is not None}
    p = orbit_params(a, b, axis=axis, range=range, v_range=v_range, seed=seed, **kw)
    if v_range is None:
        _, probe, _ = _run_orbit(runtime, _copy_struct(p, height=1, v_lo=-1.0, v_hi=1.0), starts)
        seen = probe[probe["hits"] + probe["misses"] > 0]
        if seen.size == 0:
            raise ValueError("no column has a visit inside the bound box: there is no range to plot (give v_range)")
        p.v_lo, p.v_hi = _padded(float(seen["vmin"].min()), float(seen["vmax"].max()))
    count, stats, m = _run_orbit(runtime, p, starts)
    return OrbitDiagram(p, count, stats, m, runtime.device)


# ---- correlation dimension (include/sar.h: sar_runtime_pairs, sar_runtime_corrdim, sar_corrdim_fit) ------------------------------
CORRDIM_LINE_DTYPE = np.dtype(_abi.SarCorrdimLine)
CORRDIM_RECORD_DTYPE = np.dtype(_abi.SarCorrdimRecord)
PAIRS_COUNTS_DTYPE = np.dtype(_abi.SarPairsCounts)


def pairs_params(**params) -> "_abi.SarPairsParams":
    """sar_pairs_params_default() with the given fields replaced (samples, theiler, sub_bits, e_min, e_max)."""
    return _fill(_defaults(_abi.SarPairsParams, "sar_pairs_params_default"), params)


def corrdim_params(**params) -> "_abi.SarCorrdimParams":
    """sar_corrdim_params_default() with the given fields replaced (jobs, samples, stride, transient, theiler, sub_bits, e_min, e_max,
    seed, bound, c_lo, r_hi_fraction)."""
    return _fill(_defaults(_abi.SarCorrdimParams, "sar_corrdim_params_default"), params)


def pair_edges(binning=None) -> np.ndarray:
    """r_b, the upper edge of every bin of a binning (sar_pairs_edges; None: the defaults'); the overflow bin's is +inf."""
    bins = C.c_uint32()
    ref = None if binning is None else C.byref(binning)
    _check(_lib().sar_pairs_edges(ref, C.byref(bins), None), "sar_pairs_edges")
    out = np.empty(bins.value)
    _check(_lib().sar_pairs_edges(ref, None, _ptr(out)), "sar_pairs_edges")
    return out


def corrdim_fit(hist, binning=None, c_lo: float = 100.0, r_hi: float = np.inf) -> np.ndarray:
    """The least-squares line of ln C on ln r over the window C_b >= c_lo, r_b <= r_hi of one histogram (sar_corrdim_fit: host
    arithmetic, no device), as a CORRDIM_LINE_DTYPE scalar; "slope" is D2."""
    h = np.ascontiguousarray(hist, dtype=np.uint64)
    if h.ndim != 1 or h.size != pair_edges(binning).size:
        raise ValueError("hist must hold one count per bin of the binning")
    line = _abi.SarCorrdimLine()
    _check(_lib().sar_corrdim_fit(_ptr(h), None if binning is None else C.byref(binning), float(c_lo), float(r_hi), C.byref(line)),
           "sar_corrdim_fit")
    return np.frombuffer(bytes(line), dtype=CORRDIM_LINE_DTYPE)[0]


def _point_sets(points):
    """`points`, (n, 3) or (n_sets, n, 3), as (n_sets, n, 3) float64 — and whether it was the single set."""
    pts = np.ascontiguousarray(points, dtype=np.float64)
    single = pts.ndim == 2
    if single:
        pts = pts[None]
    if pts.ndim != 3 or pts.shape[2] != 3:
        raise ValueError("points must be (n, 3) or (n_sets, n, 3)")
    return pts, single


def pair_histogram(runtime: Runtime, points, samples=None, theiler: int = 0, counts: bool = False, **binning):
    """The exact pair-distance histogram of point sets on the GPU (sar_runtime_pairs): `points` (n, 3) or (n_sets, n, 3); point i is
    sample i % samples of trajectory i // samples (default: one trajectory), pairs of one trajectory at most `theiler` apart are
    skipped; binning: sub_bits, e_min, e_max. Returns the uint64 histogram, (bins,) or (n_sets, bins) — with counts=True also the
    PAIRS_COUNTS_DTYPE record(s) of pairs counted and skipped. pair_edges(pairs_params(**binning)) gives the bins' r."""
    pts, single = _point_sets(points)
    n_sets, n = pts.shape[0], pts.shape[1]
    p = pairs_params(samples=n if samples is None else samples, theiler=theiler, **binning)
    bins = C.c_uint32()
    _check(_lib().sar_pairs_edges(C.byref(p), C.byref(bins), None), "sar_pairs_edges")
    hist = np.zeros((n_sets, bins.value), dtype=np.uint64)
    cnt = np.zeros(n_sets, dtype=PAIRS_COUNTS_DTYPE)
    _check(_lib().sar_runtime_pairs(runtime.handle, C.byref(p), n_sets, n, _ptr(pts), _ptr(hist), _ptr(cnt, _abi.SarPairsCounts)),
           "sar_runtime_pairs")
    if single:
        hist, cnt = hist[0], cnt[0]
    return (hist, cnt) if counts else hist


def _record_coeffs(records, search_seed: int, search_lo: float, search_hi: float):
    """(n, 30) coefficients of search_attractors records — candidates `candidate` of the search stream search_seed over [search_lo,
    search_hi) —; None if `records` is none of those."""
    if not (isinstance(records, (np.ndarray, np.void)) and records.dtype.names and "candidate" in records.dtype.names):
        return None
    maps = [search_candidate(search_seed, int(c), search_lo, search_hi).reshape(30) for c in np.asarray(records).reshape(-1)["candidate"]]
    return np.stack(maps) if maps else np.zeros((0, 30))


def _coeff_sets(coeffs, search_seed: int, search_lo: float, search_hi: float) -> np.ndarray:
    """(n_maps, 30) coefficients from what correlation_dimension and box_dimension take: a Config, sets of 30 numbers, or
    search_attractors records."""
    cs = _record_coeffs(coeffs, search_seed, search_lo, search_hi)
    if cs is None and isinstance(coeffs, Config):
        cs = _base_coeffs(coeffs)[None, :]
    elif cs is None:
        cs = np.ascontiguousarray(coeffs, dtype=np.float64)
        if cs.size % 30 or cs.ndim > 3:
            raise ValueError("coeffs must hold sets of 30 coefficients")
        cs = cs.reshape(-1, 30)
    return np.ascontiguousarray(cs, dtype=np.float64)


class CorrelationDimension:
    """What sar_runtime_corrdim gave for n_maps maps: `hist` (n_maps, bins) uint64, `edges` (bins,) the bins' upper r_b, `records`
    (CORRDIM_RECORD_DTYPE, one per map), `coeffs` (n_maps, 30), `points` (n_maps, n, 3) when asked for (None otherwise), `params`."""

    def __init__(self, params, coeffs: np.ndarray, hist: np.ndarray, records: np.ndarray, points=None):
        self.params, self.coeffs, self.hist, self.records, self.points = params, coeffs, hist, records, points
        self.binning = pairs_params(samples=params.samples, theiler=params.theiler, sub_bits=params.sub_bits, e_min=params.e_min,
                                    e_max=params.e_max)
        self.edges = pair_edges(self.binning)

    @property
    def status(self) -> np.ndarray:
        return self.records["status"]

    @property
    def d2(self) -> np.ndarray:
        """(n_maps,) the slope of the default window's line: NaN for a DIVERGED map and where the window holds fewer than 3 bins."""
        return self.records["line"]["slope"]

    def fit(self, c_lo=None, r_hi=None) -> np.ndarray:
        """Refits every map on the host (sar_corrdim_fit) over C_b >= c_lo and r_b <= r_hi — each a scalar or one value per map; None: the
        call's own c_lo, the records' r_hi. Returns CORRDIM_LINE_DTYPE records, one per map; a DIVERGED map has no window."""
        m = self.hist.shape[0]
        lo = np.broadcast_to(self.params.c_lo if c_lo is None else np.asarray(c_lo, dtype=np.float64), (m,))
        hi = np.broadcast_to(self.records["r_hi"] if r_hi is None else np.asarray(r_hi, dtype=np.float64), (m,))
        out = np.zeros(m, dtype=CORRDIM_LINE_DTYPE)
        for k in builtins.range(m):
            if self.records["status"][k] != _abi.SAR_SEARCH_BOUNDED:
                out[k] = (np.nan, np.nan, np.nan, 0, 0, 0, _abi.SAR_CORRDIM_NO_WINDOW)
            else:
                out[k] = corrdim_fit(self.hist[k], self.binning, lo[k], hi[k])
        return out


def correlation_dimension(runtime: Runtime, coeffs, *, starts=None, points: bool = False, search_seed: int = 0, search_lo: float = -1.2,
                          search_hi: float = 1.2, **params) -> CorrelationDimension:
    """The correlation dimension D2 of maps, measured on the GPU (sar_runtime_corrdim): every map runs `jobs` trajectories (`starts`
    (jobs, 3), default the stream of `seed`) through `transient` steps and records a point after every `stride` steps, `samples`
    times; the exact histogram of all pair distances of those points gives C(r), and .d2 is the slope of ln C on ln r over the
    default window. `coeffs`: a Config, (30,) / (3, 10) coefficients, (n_maps, 30) / (n_maps, 3, 10) of them, or search_attractors
    records (their maps are candidates `candidate` of the search stream search_seed over [search_lo, search_hi)) — compare .d2 with
    the records' ky_dim. params: the fields of sar_corrdim_params. points=True keeps the recorded points."""
    cs = _coeff_sets(coeffs, search_seed, search_lo, search_hi)
    p = corrdim_params(**params)
    m, n = cs.shape[0], p.jobs * p.samples
    keep, sp = _starts_ptr(starts, p.jobs)
    bins = pair_edges(pairs_params(sub_bits=p.sub_bits, e_min=p.e_min, e_max=p.e_max)).size
    hist = np.zeros((m, bins), dtype=np.uint64)
    recs = np.zeros(m, dtype=CORRDIM_RECORD_DTYPE)
    pts = np.zeros((m, n, 3)) if points else None
    _check(_lib().sar_runtime_corrdim(runtime.handle, C.byref(p), m, _ptr(cs), sp, _ptr(hist), _ptr(recs, _abi.SarCorrdimRecord), _ptr(pts)),
           "sar_runtime_corrdim")
    del keep
    return CorrelationDimension(p, cs, hist, recs, pts)


# ---- box counting (include/sar.h: sar_runtime_boxes, sar_runtime_boxdim, sar_boxdim_fit) -------------------------------------------
BOX_LEVEL_DTYPE = np.dtype(_abi.SarBoxLevel)
BOXDIM_LINE_DTYPE = np.dtype(_abi.SarBoxdimLine)
BOXDIM_LINES_DTYPE = np.dtype(_abi.SarBoxdimLines)
BOXDIM_RECORD_DTYPE = np.dtype(_abi.SarBoxdimRecord)


def box_params(**params) -> "_abi.SarBoxParams":
    """sar_box_params_default() with the given fields replaced (levels, origin, size)."""
    if params.get("origin", 0) is None:   # (origin=None: the default's)
        del params["origin"]
    return _fill(_defaults(_abi.SarBoxParams, "sar_box_params_default"), params)


def boxdim_params(**params) -> "_abi.SarBoxdimParams":
    """sar_boxdim_params_default() with the given fields replaced (jobs, samples, stride, transient, levels, l_min, seed, bound,
    min_occupancy)."""
    return _fill(_defaults(_abi.SarBoxdimParams, "sar_boxdim_params_default"), params)


def box_log2_q32(n: int) -> int:
    """lg32(n): log2(n) in fixed point with 32 fraction bits, truncated, as the box kernels compute it (sar_box_log2_q32)."""
    if not 0 <= int(n) < 2 ** 32:
        raise ValueError("n must fit 32 bits")
    out = C.c_uint64()
    _check(_lib().sar_box_log2_q32(int(n), C.byref(out)), "sar_box_log2_q32")
    return out.value


def box_fit(levels, n: int, l_min: int = 3, min_occupancy: float = 16.0) -> np.ndarray:
    """The three least-squares lines over the window of one set's levels (sar_boxdim_fit: host arithmetic, no device), as a
    BOXDIM_LINES_DTYPE scalar: ["d0"]["slope"], ["d1"]["slope"] and ["d2"]["slope"] are D0, D1 and D2. `levels`: the (L + 1,)
    BOX_LEVEL_DTYPE rows of box_counts, `n` the points of the set."""
    rows = np.ascontiguousarray(levels, dtype=BOX_LEVEL_DTYPE)
    if rows.ndim != 1 or rows.size < 2:
        raise ValueError("levels must hold the rows of one set, level 0 included")
    if not 0 <= int(n) < 2 ** 32 or not 0 <= int(l_min) < 2 ** 32:
        raise ValueError("n and l_min must fit 32 bits")
    out = _abi.SarBoxdimLines()
    _check(_lib().sar_boxdim_fit(_ptr(rows, _abi.SarBoxLevel), rows.size - 1, int(n), int(l_min), float(min_occupancy), C.byref(out)),
           "sar_boxdim_fit")
    return np.frombuffer(bytes(out), dtype=BOXDIM_LINES_DTYPE)[0]


def box_counts(runtime: Runtime, points, origin=(0.0, 0.0, 0.0), size: float = 1.0, levels: int = 16) -> np.ndarray:
    """The exact box counts of point sets on the GPU (sar_runtime_boxes): `points` (n, 3) or (n_sets, n, 3); the cube `origin`, `size`
    is halved `levels` times, points outside it fall into its border cells. Returns BOX_LEVEL_DTYPE rows, (levels + 1,) or
    (n_sets, levels + 1): per level the occupied cells, those holding one point, the sum of the squared occupancies and the sum of
    n_i lg32(n_i). box_fit turns one set's rows into D0, D1 and D2."""
    pts, single = _point_sets(points)
    n_sets, n = pts.shape[0], pts.shape[1]
    p = box_params(origin=origin, size=size, levels=levels)
    rows = np.zeros((n_sets, p.levels + 1), dtype=BOX_LEVEL_DTYPE)
    _check(_lib().sar_runtime_boxes(runtime.handle, C.byref(p), n_sets, n, _ptr(pts), _ptr(rows, _abi.SarBoxLevel)), "sar_runtime_boxes")
    return rows[0] if single else rows


class BoxDimension:
    """What sar_runtime_boxdim gave for n_maps maps: `levels` (n_maps, L + 1) BOX_LEVEL_DTYPE, `records` (BOXDIM_RECORD_DTYPE, one per
    map, with the cube and the three lines), `coeffs` (n_maps, 30), `points` (n_maps, n, 3) when asked for (None otherwise), `params`."""

    def __init__(self, params, coeffs: np.ndarray, levels: np.ndarray, records: np.ndarray, points=None):
        self.params, self.coeffs, self.levels, self.records, self.points = params, coeffs, levels, records, points
        self.n = params.jobs * params.samples

    @property
    def status(self) -> np.ndarray:
        return self.records["status"]

    @property
    def d0(self) -> np.ndarray:
        """(n_maps,) the capacity dimension: NaN for a DIVERGED map and where the window holds fewer than 3 levels."""
        return self.records["lines"]["d0"]["slope"]

    @property
    def d1(self) -> np.ndarray:
        """(n_maps,) the information dimension."""
        return self.records["lines"]["d1"]["slope"]

    @property
    def d2(self) -> np.ndarray:
        """(n_maps,) the box form of the correlation dimension."""
        return self.records["lines"]["d2"]["slope"]

    def epsilon(self, i: int) -> np.ndarray:
        """(L + 1,) the edge of map i's boxes at every level: size * 2^-l (NaN for a DIVERGED map)."""
        return float(self.records["size"][i]) * np.exp2(-np.arange(self.levels.shape[1], dtype=np.float64))

    def fit(self, i: int, l_min=None, min_occupancy=None) -> np.ndarray:
        """Refits map i on the host (sar_boxdim_fit) over the levels >= l_min whose boxes hold min_occupancy points on average;
        None: the call's own. A BOXDIM_LINES_DTYPE scalar; a DIVERGED map has no window."""
        if self.records["status"][i] != _abi.SAR_SEARCH_BOUNDED:
            out = np.zeros(1, dtype=BOXDIM_LINES_DTYPE)[0]
            for d in ("d0", "d1", "d2"):
                out[d] = (np.nan, np.nan, np.nan)
            out["status"] = _abi.SAR_BOXDIM_NO_WINDOW
            return out
        return box_fit(self.levels[i], self.n, self.params.l_min if l_min is None else l_min,
                       self.params.min_occupancy if min_occupancy is None else min_occupancy)


def box_dimension(runtime: Runtime, coeffs, *, starts=None, points: bool = False, search_seed: int = 0, search_lo: float = -1.2,
                  search_hi: float = 1.2, **params) -> BoxDimension:
    """The box-counting dimensions D0, D1 and D2 of maps, measured on the GPU (sar_runtime_boxdim): every map records its points as
    correlation_dimension does (`jobs` trajectories, `transient` steps, then a point after every `stride` steps, `samples` times); the
    cube around them is halved `levels` times and the occupied boxes of every level are counted exactly. .d0, .d1 and .d2 are the
    slopes over the default window (levels >= l_min whose boxes hold min_occupancy points on average). `coeffs`: what
    correlation_dimension takes — compare .d1 with search records' ky_dim. params: the fields of sar_boxdim_params. points=True keeps
    the recorded points."""
    cs = _coeff_sets(coeffs, search_seed, search_lo, search_hi)
    p = boxdim_params(**params)
    m, n = cs.shape[0], p.jobs * p.samples
    keep, sp = _starts_ptr(starts, p.jobs)
    rows = np.zeros((m, p.levels + 1), dtype=BOX_LEVEL_DTYPE)
    recs = np.zeros(m, dtype=BOXDIM_RECORD_DTYPE)
    pts = np.zeros((m, n, 3)) if points else None
    _check(_lib().sar_runtime_boxdim(runtime.handle, C.byref(p), m, _ptr(cs), sp, _ptr(rows, _abi.SarBoxLevel),
                                     _ptr(recs, _abi.SarBoxdimRecord), _ptr(pts)), "sar_runtime_boxdim")
    del keep
    return BoxDimension(p, cs, rows, recs, pts)


# ---- power spectra (include/sar.h: sar_runtime_spectra, sar_runtime_spectrum) ------------------------------------------------------
SPECTRA_RECORD_DTYPE = np.dtype(_abi.SarSpectraRecord)
SPECTRUM_RECORD_DTYPE = np.dtype(_abi.SarSpectrumRecord)
SPECTRUM_WINDOWS = {"rect": _abi.SAR_WINDOW_RECT, "hann": _abi.SAR_WINDOW_HANN}


def _window_id(window) -> int:
    if isinstance(window, str):
        if window not in SPECTRUM_WINDOWS:
            raise ValueError(f"window must be one of {sorted(SPECTRUM_WINDOWS)} (or a SAR_WINDOW_* number), got {window!r}")
        return SPECTRUM_WINDOWS[window]
    return window


def _transform_params(params: dict) -> dict:
    """`params` with a window's name replaced by its number and a hop that is None or left out by n / 2 of the n given."""
    params = dict(params)
    if "window" in params:
        params["window"] = _window_id(params["window"])
    if params.get("hop") is None:
        params.pop("hop", None)
        if "n" in params:
            params["hop"] = max(int(params["n"]) // 2, 1)
    return params


def spectra_params(**params) -> "_abi.SarSpectraParams":
    """sar_spectra_params_default() with the given fields replaced (n, hop, window, samples, chunk, proj); window by name ("rect",
    "hann") or number; a hop that is None or left out is n / 2 of the n given."""
    return _fill(_defaults(_abi.SarSpectraParams, "sar_spectra_params_default"), _transform_params(params))


def spectrum_params(**params) -> "_abi.SarSpectrumParams":
    """sar_spectrum_params_default() with the given fields replaced (jobs, segments, n, hop, window, stride, transient, chunk, seed,
    bound, proj); window and hop as in spectra_params."""
    return _fill(_defaults(_abi.SarSpectrumParams, "sar_spectrum_params_default"), _transform_params(params))


def spectrum_twiddles(n: int) -> np.ndarray:
    """The (n / 2, 2) twiddle table (re, im) the kernel reads (sar_spectrum_twiddles: host arithmetic, no device)."""
    if not 0 <= int(n) <= 1 << 16:
        raise ValueError("n must be a power of two from 8 to 4096")
    out = np.zeros((max(int(n) // 2, 1), 2))
    _check(_lib().sar_spectrum_twiddles(int(n), _ptr(out)), "sar_spectrum_twiddles")
    return out


def spectrum_window(window, n: int) -> np.ndarray:
    """The (n,) window table w of "rect" or "hann" (sar_spectrum_window: host arithmetic, no device)."""
    if not 0 <= int(n) <= 1 << 16:
        raise ValueError("n must be a power of two from 8 to 4096")
    out = np.zeros(max(int(n), 1))
    _check(_lib().sar_spectrum_window(_field_value(C.c_uint32, _window_id(window), "window"), int(n), _ptr(out)), "sar_spectrum_window")
    return out


def spectra_segments(n_points: int, **params) -> tuple:
    """(jobs, segments) of a set of n_points points under spectra_params(**params) (sar_spectra_segments)."""
    p = spectra_params(**params)
    jobs, segs = C.c_uint32(), C.c_uint32()
    _check(_lib().sar_spectra_segments(C.byref(p), _field_value(C.c_uint32, n_points, "n_points"), C.byref(jobs), C.byref(segs)),
           "sar_spectra_segments")
    return jobs.value, segs.value


def power_spectra(runtime: Runtime, points, n: int = 1024, hop=None, window="hann", samples=None, proj=(1.0, 0.0, 0.0), *, chunk: int = 0,
                  records: bool = False):
    """The raw Welch power spectra of point sets on the GPU (sar_runtime_spectra): `points` a series (n_points,) — it goes into x —,
    one set (n_points, 3) or (n_sets, n_points, 3); point i is sample i % samples of trajectory i // samples (default: one
    trajectory). The observable v = proj . (x, y, z) of every trajectory is cut into segments of `n` values `hop` apart (default
    n / 2), each loses its mean, is tapered by `window` ("hann" or "rect") and transformed; the squared magnitudes of the bins
    0 .. n / 2 are summed over segments and trajectories. Returns float64 (n / 2 + 1,) or (n_sets, n / 2 + 1) — with records=True also
    the SPECTRA_RECORD_DTYPE record(s): jobs, segments and the energy E with sum_k c_k P[k] = n E. Bin k is k / n cycles per sample."""
    arr = np.asarray(points, dtype=np.float64)
    if arr.ndim == 1:
        series, arr = arr, np.zeros((arr.size, 3))
        arr[:, 0] = series
    pts, single = _point_sets(arr)
    n_sets, n_points = pts.shape[0], pts.shape[1]
    p = spectra_params(n=n, hop=hop, window=window, samples=0 if samples is None else samples, proj=proj, chunk=chunk)
    power = np.zeros((n_sets, p.n // 2 + 1))
    recs = np.zeros(n_sets, dtype=SPECTRA_RECORD_DTYPE)
    _check(_lib().sar_runtime_spectra(runtime.handle, C.byref(p), n_sets, n_points, _ptr(pts), _ptr(power), _ptr(recs, _abi.SarSpectraRecord)),
           "sar_runtime_spectra")
    if single:
        power, recs = power[0], recs[0]
    return (power, recs) if records else power


class Spectrum:
    """What sar_runtime_spectrum gave for n_maps maps: `power` (n_maps, N / 2 + 1) float64, raw sums; `records`
    (SPECTRUM_RECORD_DTYPE, one per map); `coeffs` (n_maps, 30); `points` (n_maps, jobs * samples, 3) when asked for (None
    otherwise); `params`. Everything below is host numpy over `power`."""

    def __init__(self, params, coeffs: np.ndarray, power: np.ndarray, records: np.ndarray, points=None, device: int = 0):
        self.params, self.coeffs, self.power, self.records, self.points, self.device = params, coeffs, power, records, points, device
        self.samples = (params.segments - 1) * params.hop + params.n

    @property
    def status(self) -> np.ndarray:
        return self.records["status"]

    @property
    def freq(self) -> np.ndarray:
        """(N / 2 + 1,) the bins' frequencies in cycles per step of the map: k / (N * stride)."""
        return np.arange(self.power.shape[1], dtype=np.float64) / (float(self.params.n) * float(self.params.stride))

    @property
    def psd(self) -> np.ndarray:
        """power / (jobs * segments * sum w^2): the mean periodogram, normalised by the window's power."""
        w = spectrum_window(self.params.window, self.params.n)
        return self.power / (float(self.params.jobs) * float(self.params.segments) * float(np.sum(w * w)))

    def db(self, floor: float = -120.0) -> np.ndarray:
        """10 log10 of every bin over its map's largest bin with k >= 1, not below `floor`; a map without power is all `floor`."""
        top = np.max(self.power[:, 1:], axis=1, keepdims=True)
        with np.errstate(all="ignore"):
            out = 10.0 * np.log10(self.power / top)
        return np.maximum(np.where(np.isnan(out), floor, out), floor)

    def peaks(self, m: int, count: int = 4) -> np.ndarray:
        """The `count` strongest bins k >= 1 of map m, strongest first, the lowest k first among equals."""
        return np.argsort(-self.power[m, 1:], kind="stable")[:count] + 1

    @property
    def flatness(self) -> np.ndarray:
        """(n_maps,) the geometric over the arithmetic mean of the bins k >= 1: near 0 for lines, towards 1 for a broadband spectrum,
        0 where a bin is 0."""
        p = self.power[:, 1:]
        with np.errstate(all="ignore"):
            out = np.exp(np.mean(np.log(p), axis=1)) / np.mean(p, axis=1)
        return np.where(np.all(p > 0.0, axis=1) & np.isfinite(out), out, 0.0)

    def autocorrelation(self, m: int) -> np.ndarray:
        """(N,) the autocorrelation of map m's tapered series by lag, 1 at lag 0: the inverse transform of the power (Wiener-Khinchin).
        The circular estimate — lag l also holds lag N - l —, good for lags far below N; lags count recorded samples (`stride` steps).
        Host numpy, not held bit for bit."""
        r = np.fft.irfft(self.power[m], n=int(self.params.n))
        with np.errstate(all="ignore"):
            return r / r[0]

    def decorrelation(self, m: int, level: float = 1.0 / np.e) -> int:
        """The first lag at which map m's autocorrelation is below `level` (N / 2 where none is): a stride, and a Theiler window, for
        correlation_dimension."""
        r = self.autocorrelation(m)[:int(self.params.n) // 2]
        below = np.nonzero(r < level)[0]
        return int(below[0]) if below.size else int(self.params.n) // 2

    def counts(self) -> tuple:
        """The picture colorize paints, as (count (N / 2 + 1, n_maps) uint32, max): row 0 is the Nyquist bin, column m is map m, and
        count = min(floor((P / P_max) * (2^32 - 1)), 2^32 - 2) with P_max the largest finite bin of all maps. The quotient comes first,
        so the largest bin reaches the cap exactly; the cap is 2^32 - 2 because the Gas colorize adds 1 to a count and to max in 32
        bits."""
        p = self.power.T[::-1]
        finite = p[np.isfinite(p)]
        top = float(finite.max()) if finite.size else 0.0
        full = float(2 ** 32 - 1)
        with np.errstate(all="ignore"):
            q = np.floor((p / top) * full) if top > 0.0 else np.zeros_like(p)
        count = np.ascontiguousarray(np.clip(np.where(np.isnan(q), 0.0, q), 0.0, full - 1.0).astype(np.uint32))
        return count, int(count.max()) if count.size else 0

    def colorize(self, config: Config, hue=None, exposure={}) -> np.ndarray:
        """(N / 2 + 1, n_maps, 4) RGBA16: the spectra side by side, frequency upwards, through a runtime of that size on the spectrum's
        device — Runtime.load of counts(), `hue` a palette position per map (a scalar or n_maps values, default 0), auto_exposure
        (**exposure) and the Gas colorize, exactly as OrbitDiagram.colorize. The Gas brightness ln(count + 1) / ln(max + 1) is a
        decibel scale over the 96 dB of 32 bits. Of an OrbitDiagram.spectrum it is the spectral bifurcation diagram."""
        count, top = self.counts()
        h, w = count.shape
        col = np.zeros(w) if hue is None else np.broadcast_to(np.asarray(hue, dtype=np.float64), (w,))
        cfg = config.replace(width=w, height=h, render_kind=SAR_RENDER_GAS)
        rt = Runtime(cfg, device=self.device)
        try:
            rt.load(count, np.ascontiguousarray(np.broadcast_to(col[None, :], (h, w))), np.zeros((h, w), dtype=np.float32), top)
            return colorize(auto_exposure(cfg, rt, **exposure), rt)
        finally:
            rt.close()


def power_spectrum(runtime: Runtime, coeffs, *, starts=None, points: bool = False, search_seed: int = 0, search_lo: float = -1.2,
                   search_hi: float = 1.2, **params) -> Spectrum:
    """The power spectrum of maps' orbits, measured on the GPU (sar_runtime_spectrum): every map runs `jobs` trajectories (`starts`
    (jobs, 3), default the stream of `seed`) through `transient` steps and records a point after every `stride` steps,
    (segments - 1) * hop + n times; the observable proj . (x, y, z) of every trajectory goes through power_spectra's segments, and
    the spectra of the jobs are added. A cycle of period p shows lines at the multiples of 1 / p, a torus lines at incommensurate
    frequencies, chaos a broadband floor. `coeffs`: what correlation_dimension takes. params: the fields of sar_spectrum_params,
    window by name. points=True keeps the recorded points. One observable per call; no cross-spectra."""
    cs = _coeff_sets(coeffs, search_seed, search_lo, search_hi)
    p = spectrum_params(**params)
    m = cs.shape[0]
    samples = (max(p.segments, 1) - 1) * p.hop + p.n
    keep, sp = _starts_ptr(starts, p.jobs)
    power = np.zeros((m, p.n // 2 + 1))
    recs = np.zeros(m, dtype=SPECTRUM_RECORD_DTYPE)
    pts = np.zeros((m, p.jobs * samples, 3)) if points and p.jobs * samples <= 1 << 20 else None
    _check(_lib().sar_runtime_spectrum(runtime.handle, C.byref(p), m, _ptr(cs), sp, _ptr(power), _ptr(recs, _abi.SarSpectrumRecord), _ptr(pts)),
           "sar_runtime_spectrum")
    del keep
    return Spectrum(p, cs, power, recs, pts, runtime.device)


# ---- recurrence analysis (include/sar.h: sar_runtime_recurrence, sar_runtime_recurrence_plot, sar_runtime_rqa, sar_rqa_measures) --------
RECURRENCE_RECORD_DTYPE = np.dtype(_abi.SarRecurrenceRecord)
RQA_RECORD_DTYPE = np.dtype(_abi.SarRqaRecord)
RQA_MEASURES_DTYPE = np.dtype(_abi.SarRqaMeasures)


def recurrence_params(**params) -> "_abi.SarRecurrenceParams":
    """sar_recurrence_params_default() with the given fields replaced (samples, theiler, line_bins, chunk, eps2)."""
    return _fill(_defaults(_abi.SarRecurrenceParams, "sar_recurrence_params_default"), params)


def rqa_params(**params) -> "_abi.SarRqaParams":
    """sar_rqa_params_default() with the given fields replaced (jobs, samples, stride, transient, seed, bound, theiler, line_bins,
    chunk, eps2, eps_fraction)."""
    return _fill(_defaults(_abi.SarRqaParams, "sar_rqa_params_default"), params)


def _threshold(eps, eps2) -> float:
    """eps2 from exactly one of eps (a distance, squared here) and eps2."""
    if (eps is None) == (eps2 is None):
        raise ValueError("give exactly one of eps and eps2")
    return float(eps) * float(eps) if eps2 is None else float(eps2)


def _series_points(points) -> np.ndarray:
    """A series (n,) as points (n, 3) with the series in x; anything else as it is."""
    arr = np.asarray(points, dtype=np.float64)
    if arr.ndim != 1:
        return arr
    out = np.zeros((arr.size, 3))
    out[:, 0] = arr
    return out


def rqa_measures(diag, vert, record, l_min: int = 2, v_min: int = 2) -> np.ndarray:
    """The measures of one set's or map's histograms and RECURRENCE_RECORD_DTYPE record (sar_rqa_measures: host arithmetic, no device)
    as an RQA_MEASURES_DTYPE scalar: rr, det, l_mean, div, entr, lam, tt, l_max, v_max. A quotient without a denominator is NaN."""
    d, v = np.ascontiguousarray(diag, dtype=np.uint64), np.ascontiguousarray(vert, dtype=np.uint64)
    if d.ndim != 1 or d.shape != v.shape or d.size < 1:
        raise ValueError("diag and vert must both hold line_bins + 1 counts")
    rec = np.ascontiguousarray(np.asarray(record, dtype=RECURRENCE_RECORD_DTYPE).reshape(1))
    out = _abi.SarRqaMeasures()
    _check(_lib().sar_rqa_measures(_ptr(d), _ptr(v), _ptr(rec, _abi.SarRecurrenceRecord), d.size - 1, _field_value(C.c_uint32, l_min, "l_min"),
                                   _field_value(C.c_uint32, v_min, "v_min"), C.byref(out)), "sar_rqa_measures")
    return np.frombuffer(bytes(out), dtype=RQA_MEASURES_DTYPE)[0]


def recurrence_lines(runtime: Runtime, points, eps=None, *, eps2=None, samples=None, theiler: int = 0, line_bins: int = 256, chunk: int = 0,
                     records: bool = False):
    """The exact line-length histograms of the recurrence plots of point sets on the GPU (sar_runtime_recurrence): `points` a series
    (n,) — it goes into x —, one set (n, 3) or (n_sets, n, 3); point i is sample i % samples of trajectory i // samples (default: one
    trajectory). Two points of a trajectory more than `theiler` samples apart recur where their squared distance is below eps2 = eps *
    eps (give one of the two). Returns (diag, vert), uint64 (line_bins + 1,) or (n_sets, line_bins + 1) each: diag[l] maximal diagonal
    lines of length l in the upper triangle, vert[l] vertical lines in the full matrix, the last entry collecting l >= line_bins —
    with records=True also the RECURRENCE_RECORD_DTYPE record(s): recurrences, pairs, diag_lines, vert_lines and the longest lines,
    exact. rqa_measures turns one set's into RR, DET, LAM, ..."""
    pts, single = _point_sets(_series_points(points))
    n_sets, n = pts.shape[0], pts.shape[1]
    p = recurrence_params(samples=0 if samples is None else samples, theiler=theiler, line_bins=line_bins, chunk=chunk, eps2=_threshold(eps, eps2))
    diag = np.zeros((n_sets, p.line_bins + 1), dtype=np.uint64)
    vert = np.zeros((n_sets, p.line_bins + 1), dtype=np.uint64)
    recs = np.zeros(n_sets, dtype=RECURRENCE_RECORD_DTYPE)
    _check(_lib().sar_runtime_recurrence(runtime.handle, C.byref(p), n_sets, n, _ptr(pts), _ptr(diag), _ptr(vert),
                                         _ptr(recs, _abi.SarRecurrenceRecord)), "sar_runtime_recurrence")
    if single:
        diag, vert, recs = diag[0], vert[0], recs[0]
    return (diag, vert, recs) if records else (diag, vert)


def recurrence_plot(runtime: Runtime, points, eps=None, *, eps2=None, samples=None, theiler: int = 0, job: int = 0, window=None) -> np.ndarray:
    """The recurrence plot of trajectory `job` of one set (a series (n,) or points (n, 3)) as a bool array (sar_runtime_recurrence_plot):
    `window` = (i0, j0, height, width) gives out[y, x] = R(i0 + y, j0 + x); None is the whole matrix, at most 2^24 entries."""
    pts = np.ascontiguousarray(_series_points(points), dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("points must be a series (n,) or one set (n, 3)")
    n = pts.shape[0]
    p = recurrence_params(samples=0 if samples is None else samples, theiler=theiler, eps2=_threshold(eps, eps2))
    t = p.samples or n
    i0, j0, height, width = (0, 0, t, t) if window is None else window
    i0, j0, height, width = (_field_value(C.c_uint32, v, "window") for v in (i0, j0, height, width))
    out = np.zeros((height, width) if height * width <= 1 << 24 else (1, 1), dtype=np.uint8)
    _check(_lib().sar_runtime_recurrence_plot(runtime.handle, C.byref(p), n, _ptr(pts), _field_value(C.c_uint32, job, "job"), i0, j0, height,
                                              width, _ptr(out)), "sar_runtime_recurrence_plot")
    return out.astype(bool)


class Recurrence:
    """What sar_runtime_rqa gave for n_maps maps: `diag` and `vert` (n_maps, line_bins + 1) uint64, `records` (RQA_RECORD_DTYPE, one per
    map: the orbit's header, the eps2 used and the counts), `coeffs` (n_maps, 30), `points` (n_maps, jobs * samples, 3) when asked for
    (None otherwise), `params`. The measures are host arithmetic over the counts (sar_rqa_measures)."""

    def __init__(self, params, coeffs: np.ndarray, diag: np.ndarray, vert: np.ndarray, records: np.ndarray, points=None):
        self.params, self.coeffs, self.diag, self.vert, self.records, self.points = params, coeffs, diag, vert, records, points

    @property
    def status(self) -> np.ndarray:
        return self.records["status"]

    def measures(self, l_min: int = 2, v_min: int = 2) -> np.ndarray:
        """RQA_MEASURES_DTYPE, one per map: rr, det, l_mean, div, entr from the diagonal lines of at least l_min, lam, tt from the
        vertical lines of at least v_min, l_max, v_max. NaN where a denominator is empty (a DIVERGED map, a map without recurrences)."""
        out = np.zeros(self.diag.shape[0], dtype=RQA_MEASURES_DTYPE)
        for m in builtins.range(out.size):
            out[m] = rqa_measures(self.diag[m], self.vert[m], self.records["counts"][m], l_min, v_min)
        return out

    rr = property(lambda self: self.measures()["rr"], doc="(n_maps,) the recurrence rate")
    det = property(lambda self: self.measures()["det"], doc="(n_maps,) the determinism at l_min = 2")
    l_mean = property(lambda self: self.measures()["l_mean"], doc="(n_maps,) the mean diagonal line of at least 2")
    l_max = property(lambda self: self.measures()["l_max"], doc="(n_maps,) the longest diagonal line, exact")
    entr = property(lambda self: self.measures()["entr"], doc="(n_maps,) the entropy of the diagonal lines of at least 2")
    lam = property(lambda self: self.measures()["lam"], doc="(n_maps,) the laminarity at v_min = 2")
    tt = property(lambda self: self.measures()["tt"], doc="(n_maps,) the trapping time: the mean vertical line of at least 2")
    v_max = property(lambda self: self.measures()["v_max"], doc="(n_maps,) the longest vertical line, exact")

    def plot(self, runtime: Runtime, m: int, job: int = 0, window=None) -> np.ndarray:
        """recurrence_plot of trajectory `job` of map m with the map's own eps2 (needs points=True; a map that counted nothing is all
        False)."""
        if self.points is None:
            raise ValueError("the recorded points were not kept (points=True)")
        t = self.params.samples
        if not self.records["eps2"][m] > 0.0:
            _, _, height, width = (0, 0, t, t) if window is None else window
            return np.zeros((height, width), dtype=bool)
        return recurrence_plot(runtime, self.points[m], eps2=float(self.records["eps2"][m]), samples=t, theiler=self.params.theiler, job=job,
                               window=window)


def recurrence_analysis(runtime: Runtime, coeffs, *, starts=None, points: bool = False, search_seed: int = 0, search_lo: float = -1.2,
                        search_hi: float = 1.2, **params) -> Recurrence:
    """The recurrence quantification of maps' orbits, measured on the GPU (sar_runtime_rqa): every map runs `jobs` trajectories (`starts`
    (jobs, 3), default the stream of `seed`) through `transient` steps and records a point after every `stride` steps, `samples` times;
    two points of a trajectory recur where they are closer than eps_fraction of the diagonal of the map's extent (or eps2, squared, where
    given), and the lengths of the diagonal and vertical lines of every trajectory's recurrence plot are counted exactly. `coeffs`: what
    correlation_dimension takes, search_attractors records included. params: the fields of sar_rqa_params. points=True keeps the
    recorded points."""
    cs = _coeff_sets(coeffs, search_seed, search_lo, search_hi)
    p = rqa_params(**params)
    m, n = cs.shape[0], p.jobs * p.samples
    keep, sp = _starts_ptr(starts, p.jobs)
    bins = p.line_bins + 1 if p.line_bins <= 4096 else 1
    diag = np.zeros((m, bins), dtype=np.uint64)
    vert = np.zeros((m, bins), dtype=np.uint64)
    recs = np.zeros(m, dtype=RQA_RECORD_DTYPE)
    pts = np.zeros((m, n, 3)) if points and n <= 1 << 20 else None
    _check(_lib().sar_runtime_rqa(runtime.handle, C.byref(p), m, _ptr(cs), sp, _ptr(diag), _ptr(vert), _ptr(recs, _abi.SarRqaRecord), _ptr(pts)),
           "sar_runtime_rqa")
    del keep
    return Recurrence(p, cs, diag, vert, recs, pts)


# ---- basins of attraction (include/sar.h: sar_runtime_basin, sar_runtime_basin_colorize) ---------------------------------------
BASIN_PIXEL_DTYPE = np.dtype(_abi.SarBasinPixel)
BASIN_ATTRACTOR_DTYPE = np.dtype(_abi.SarBasinAttractor)
BASIN_NONE = 0xFFFFFFFF   # root / label of a pixel that escaped


def _map_coeffs(coeffs, search_seed: int = 0, search_lo: float = -1.2, search_hi: float = 1.2) -> np.ndarray:
    """One map's 30 coefficients from a Config, (3, 10) / (30,) numbers, or one search_attractors record (candidate `candidate` of the
    search stream search_seed over [search_lo, search_hi))."""
    cs = _record_coeffs(coeffs, search_seed, search_lo, search_hi)
    if cs is None:
        return _base_coeffs(coeffs)
    if len(cs) != 1:
        raise ValueError(f"one search record names one map, got {len(cs)}")
    return cs[0]


def basin_params(coeffs, origin, du, dv, width: int, height: int, box=None, search_seed: int = 0, search_lo: float = -1.2,
                 search_hi: float = 1.2, **params) -> "_abi.SarBasinParams":
    """sar_basin_params_default() filled in: the map `coeffs` (a Config, 30 numbers or a search record), the plane of start points
    origin + du * tu + dv * tv over width x height pixels (row 0 at the high end of tv), box = ((xlo, ylo, zlo), (xhi, yhi, zhi)) the
    box the grid divides, and any of transient, steps, bound, grid."""
    p = _fill(_defaults(_abi.SarBasinParams, "sar_basin_params_default"),
              dict(coeffs=_map_coeffs(coeffs, search_seed, search_lo, search_hi), origin=origin, du=du, dv=dv, width=width, height=height))
    if box is not None:
        lo, hi = box
        _fill(p, dict(box_lo=lo, box_hi=hi))
    return _fill(p, params, allowed=("transient", "steps", "bound", "grid"))


def _run_basin(runtime: Runtime, p, cap=None):
    npix = p.width * p.height
    pix = np.empty(max(npix, 1), dtype=BASIN_PIXEL_DTYPE)
    n = C.c_uint32()
    st = _abi.SarBasinStats()
    want = 64 if cap is None else int(cap)
    while True:
        table = np.zeros(max(want, 1), dtype=BASIN_ATTRACTOR_DTYPE)
        _check(_lib().sar_runtime_basin(runtime.handle, C.byref(p), _ptr(pix, _abi.SarBasinPixel), _ptr(table, _abi.SarBasinAttractor), want,
                                        C.byref(n), C.byref(st)), "sar_runtime_basin")
        if cap is not None or n.value <= want:
            break
        want = int(n.value)   # (more attractors than the first guess: once more with room for all)
    stats = {**_stats_dict(st), "extent": np.array(list(st.extent), dtype=np.float64)}
    return pix[:npix].reshape(p.height, p.width), table[:min(int(n.value), want)], int(n.value), stats


class BasinMap:
    """One basin picture of sar_runtime_basin: `pixels` (height, width) of BASIN_PIXEL_DTYPE, `attractors` (BASIN_ATTRACTOR_DTYPE,
    sorted by basin size), `n_attractors` (all of them, also beyond a `cap`), `stats` (counts and the raw `extent` of the tails),
    `params`."""

    def __init__(self, runtime: Runtime, params, pixels: np.ndarray, attractors: np.ndarray, n_attractors: int, stats: dict):
        self.runtime, self.params, self.pixels, self.attractors = runtime, params, pixels, attractors
        self.n_attractors, self.stats = int(n_attractors), stats

    @property
    def status(self) -> np.ndarray:
        return self.pixels["status"]

    @property
    def escape_step(self) -> np.ndarray:
        return self.pixels["escape_step"]

    @property
    def label(self) -> np.ndarray:
        return self.pixels["label"]

    @property
    def root(self) -> np.ndarray:
        return self.pixels["root"]

    def start(self, x: int, y: int) -> np.ndarray:
        """Pixel (x, y)'s start point (host arithmetic, the device's doubles)."""
        out = np.empty(3)
        _check(_lib().sar_basin_start(C.byref(self.params), int(x), int(y), _ptr(out)), "sar_basin_start")
        return out

    def share(self, label: int) -> float:
        """Basin `label`'s share of the plane's pixels."""
        return float(np.count_nonzero(self.label == int(label))) / float(self.label.size)

    def starts(self, label: int, n: int) -> np.ndarray:
        """(n, 3) start points of basin `label`: pixels taken evenly spaced through the basin's ascending pixel indices (repeating
        when the basin has fewer than n), each through sar_basin_start — known to stay on that attractor for transient + steps
        steps. render_jobs, orbit_diagram(starts=...) and correlation_dimension(starts=...) take the array."""
        idx = np.flatnonzero(self.label.reshape(-1) == int(label))
        if idx.size == 0:
            raise ValueError(f"basin {label} holds no pixel")
        if int(n) < 1:
            raise ValueError("n must be at least 1")
        pick = idx[(np.arange(int(n), dtype=np.int64) * idx.size) // int(n)]
        w = self.params.width
        return np.stack([self.start(int(i % w), int(i // w)) for i in pick])

    def colorize(self, config: Config, fade=None) -> np.ndarray:
        """(height, width, 4) RGBA16 (include/sar.h: sar_basin_colors): an escaped pixel grey by its escape step, a bounded one config's
        palette at its attractor's place in the table; computed on the device from the records the runtime still holds. write_image
        takes it."""
        c = _defaults(_abi.SarBasinColors, "sar_basin_colors_default")
        if fade is not None:
            c.fade = float(fade)
        return _colorize_records(self, "basin", "basin picture", self.pixels.shape, config, c)

    def ftle(self, runtime: Runtime, steps: int = 16, **params) -> "FtleMap":
        """The FTLE map (ftle_map) of this basin picture's own map over its own plane, with its bound unless `params` names another:
        the foliation inside the basins, and the basin boundary as its EDGE pixels."""
        p = self.params
        return ftle_map(runtime, list(p.coeffs), list(p.origin), list(p.du), list(p.dv), p.width, p.height, steps,
                        **{"bound": p.bound, **params})

    def _held(self):
        """The runtime, if the picture it holds for the probes is still this one."""
        last = getattr(self.runtime, "_last_basin", None)
        if last is None or last() is not self:
            raise ValueError("the runtime has computed another basin picture since this one: it no longer holds this picture for the probes")
        return self.runtime

    def fates(self, points) -> np.ndarray:
        """The fates of any start points (n, 3) in this picture (sar_runtime_basin_fates), as BASIN_FATE_DTYPE: `status`, `escape_step`,
        `label` (BASIN_UNKNOWN where no tail point met a labelled cell, BASIN_NONE where DIVERGED) and `hit`. The point may lie off the
        plane or between pixels; the answer is a statement at this picture's grid and no finer."""
        return basin_fates(self._held(), points)

    def stability(self, n: int = 65536, box=None, seed: int = 0) -> "BasinStability":
        """Basin stability: the Monte-Carlo share of a region that belongs to each attractor. n points drawn on the host with
        np.random.default_rng(seed) — uniformly on the picture's plane (box=None: origin + du * u + dv * v, u and v in [0, 1)) or in the
        3-D box (lo, hi) — and their fates."""
        rng = np.random.default_rng(seed)
        p = self.params
        if box is None:
            t = rng.random((int(n), 2))
            o, du, dv = (np.array(list(a), dtype=np.float64) for a in (p.origin, p.du, p.dv))
            points = (o[None, :] + du[None, :] * t[:, :1]) + dv[None, :] * t[:, 1:]
        else:
            lo, hi = (np.asarray(a, dtype=np.float64).reshape(3) for a in box)
            points = lo[None, :] + (hi - lo)[None, :] * rng.random((int(n), 3))
        return BasinStability(points, self.fates(points), self.n_attractors)

    def uncertainty(self, n: int = 16384, eps0=None, levels: int = 24, direction=None, seed: int = 0, points=None, chunk: int = 0) -> "BasinUncertainty":
        """Final-state sensitivity of this picture's boundary (sar_runtime_basin_uncertainty): n base points drawn uniformly on the plane
        with np.random.default_rng(seed) (or `points`, (n, 3)), each perturbed by +-direction * e_k, e_k = eps0 / 2^(k - 1), k = 1..levels.
        direction: default du normalised; eps0: default |du| / 8."""
        p = self.params
        du = np.array(list(p.du), dtype=np.float64)
        norm = float(np.sqrt((du * du).sum()))
        if direction is None:
            direction = du / norm if norm > 0.0 else np.array([1.0, 0.0, 0.0])
        if eps0 is None:
            eps0 = norm / 8.0 if norm > 0.0 else 0.125
        if points is None:
            t = np.random.default_rng(seed).random((int(n), 2))
            o, dv = (np.array(list(a), dtype=np.float64) for a in (p.origin, p.dv))
            points = (o[None, :] + du[None, :] * t[:, :1]) + dv[None, :] * t[:, 1:]
        return basin_uncertainty(self._held(), points, dir=direction, eps0=eps0, levels=levels, chunk=chunk)


def basin_map(runtime: Runtime, coeffs, origin, du, dv, width: int = 256, height: int = 256, box=None, cap=None, **params) -> BasinMap:
    """The basins of attraction of one map over a plane of start points, on the GPU (sar_runtime_basin): pixel (x, y) starts at
    origin + du * x / (width - 1) + dv * (height - 1 - y) / (height - 1), runs transient + steps steps, and either escapes the bound box
    (status DIVERGED, escape_step) or stays (BOUNDED) — then the grid cells its last steps + 1 points visit join it to an attractor,
    a connected component of visited cells of the grid^3 cells of `box`. `coeffs`: a Config, 30 numbers or one search record.
    box=None costs a second run: a first call with grid=1 learns the extent of all tails, and the box is that extent widened by 2 %
    per side (a unit box where nothing stays bounded). cap: keep the first `cap` attractors only (n_attractors still counts all).
    params: transient, steps, bound, grid (defaults 1000, 256, 1e6, 32), and search_seed / search_lo / search_hi for a record."""
    p = basin_params(coeffs, origin, du, dv, width, height, box, **params)
    _hold_records(runtime, "basin", None)
    if box is None:
        _, _, _, probe = _run_basin(runtime, _copy_struct(p, grid=1), cap=0)
        for k in builtins.range(3):
            ext = probe["extent"]
            p.box_lo[k], p.box_hi[k] = _padded(float(ext[2 * k]), float(ext[2 * k + 1])) if probe["bounded"] else (0.0, 1.0)
    pix, table, n, stats = _run_basin(runtime, p, cap)
    basin = BasinMap(runtime, p, pix, table, n, stats)
    _hold_records(runtime, "basin", basin)
    return basin


# ---- basin probes (include/sar.h: sar_runtime_basin_fates, sar_runtime_basin_uncertainty) ---------------------------------------
BASIN_FATE_DTYPE = np.dtype(_abi.SarBasinFate)
BASIN_LEVEL_DTYPE = np.dtype(_abi.SarBasinUncertaintyLevel)
BASIN_LADDER_MASK_DTYPE = np.dtype(_abi.SarBasinLadderMask)
BASIN_UNKNOWN = _abi.SAR_BASIN_UNKNOWN   # label of a bounded probe none of whose tail points met a labelled cell


def _points3(points) -> np.ndarray:
    pts = np.ascontiguousarray(points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"points must be (n, 3), got {pts.shape}")
    return pts


def basin_fates(runtime: Runtime, points) -> np.ndarray:
    """The fates of the start points (n, 3) in the basin picture `runtime` holds — its last successful basin_map / sar_runtime_basin —
    on the GPU (sar_runtime_basin_fates): an array of BASIN_FATE_DTYPE. For callers without the BasinMap object; BasinMap.fates also
    checks that the held picture is its own."""
    pts = _points3(points)
    out = np.empty(max(len(pts), 1), dtype=BASIN_FATE_DTYPE)
    _check(_lib().sar_runtime_basin_fates(runtime.handle, len(pts), _ptr(pts), _ptr(out, _abi.SarBasinFate), None), "sar_runtime_basin_fates")
    return out[:len(pts)]


def basin_ladder_params(**params) -> "_abi.SarBasinLadderParams":
    """sar_basin_ladder_params_default() (dir (1, 0, 0), eps0 0.125, levels 24, chunk 0) with the given fields replaced."""
    return _fill(_defaults(_abi.SarBasinLadderParams, "sar_basin_ladder_params_default"), params)


def basin_uncertainty(runtime: Runtime, base, **params) -> "BasinUncertainty":
    """The uncertainty ladder over the base points (n, 3) in the basin picture `runtime` holds, on the GPU
    (sar_runtime_basin_uncertainty). params: dir, eps0, levels, chunk (sar_basin_ladder_params)."""
    p = basin_ladder_params(**params)
    pts = _points3(base)
    levels = np.zeros(max(p.levels, 1), dtype=BASIN_LEVEL_DTYPE)
    fate0 = np.empty(max(len(pts), 1), dtype=BASIN_FATE_DTYPE)
    masks = np.empty(max(len(pts), 1), dtype=BASIN_LADDER_MASK_DTYPE)
    _check(_lib().sar_runtime_basin_uncertainty(runtime.handle, C.byref(p), len(pts), _ptr(pts), _ptr(levels, _abi.SarBasinUncertaintyLevel),
                                                _ptr(fate0, _abi.SarBasinFate), _ptr(masks, _abi.SarBasinLadderMask)),
           "sar_runtime_basin_uncertainty")
    return BasinUncertainty(p, pts, levels[:p.levels], fate0[:len(pts)], masks[:len(pts)])


class BasinStability:
    """Basin stability from n probes: `points` (n, 3), `fates` (BASIN_FATE_DTYPE), and over the classes — the picture's labels
    0 .. n_attractors - 1, then the escaped, then the unknown — `counts`, `share` = counts / n and `stderr` = sqrt(p (1 - p) / n)."""

    def __init__(self, points: np.ndarray, fates: np.ndarray, n_attractors: int):
        self.points, self.fates, self.n_attractors = points, fates, int(n_attractors)
        bounded = fates["status"] == _abi.SAR_SEARCH_BOUNDED
        known = bounded & (fates["label"] != BASIN_UNKNOWN)
        per_label = np.bincount(fates["label"][known].astype(np.int64), minlength=self.n_attractors)
        self.counts = np.concatenate([per_label, [np.count_nonzero(~bounded), np.count_nonzero(bounded & ~known)]]).astype(np.uint64)
        n = float(len(fates))
        self.share = self.counts.astype(np.float64) / n
        self.stderr = np.sqrt(self.share * (1.0 - self.share) / n)

    @property
    def escaped(self) -> int:
        return int(self.counts[-2])

    @property
    def unknown(self) -> int:
        return int(self.counts[-1])


class BasinUncertaintyFit:
    """The line log2 f = intercept + alpha log2 eps over `levels` (1-based): `alpha`, its standard error `alpha_err` (NaN with fewer
    than three levels) and the boundary's dimension D - alpha."""

    def __init__(self, alpha: float, alpha_err: float, intercept: float, levels: np.ndarray):
        self.alpha, self.alpha_err, self.intercept, self.levels = alpha, alpha_err, intercept, levels

    def boundary_dimension(self, D: float = 2) -> float:
        return float(D) - self.alpha


class BasinUncertainty:
    """One uncertainty ladder: `params`, `base` (n, 3), `levels` (BASIN_LEVEL_DTYPE: eps, tested, uncertain, unknown per level), `eps`,
    `f` = uncertain / tested (NaN where nothing was tested), `fate0` (the base points' own fates) and `masks` (per base point, bit
    k - 1 of uncertain_bits / unknown_bits: level k). The counts are exact; the fit is host numpy."""

    def __init__(self, params, base: np.ndarray, levels: np.ndarray, fate0: np.ndarray, masks: np.ndarray):
        self.params, self.base, self.levels, self.fate0, self.masks = params, base, levels, fate0, masks

    @property
    def eps(self) -> np.ndarray:
        return self.levels["eps"]

    @property
    def f(self) -> np.ndarray:
        tested = self.levels["tested"].astype(np.float64)
        with np.errstate(all="ignore"):
            return np.where(tested > 0, self.levels["uncertain"].astype(np.float64) / tested, np.nan)

    def fit(self, min_uncertain: int = 16, f_max: float = 0.5) -> BasinUncertaintyFit:
        """The least-squares slope of log2 f on log2 eps over the levels with uncertain >= min_uncertain (at least 1) and f <= f_max:
        f ~ eps^alpha. ValueError with fewer than two such levels."""
        f = self.f
        use = np.flatnonzero((self.levels["uncertain"] >= max(int(min_uncertain), 1)) & (f <= float(f_max)))
        if use.size < 2:
            raise ValueError(f"{use.size} level(s) hold at least {min_uncertain} uncertain base points at f <= {f_max}: no line")
        x, y = np.log2(self.eps[use]), np.log2(f[use])
        dx = x - x.mean()
        alpha = float((dx * (y - y.mean())).sum() / (dx * dx).sum())
        intercept = float(y.mean() - alpha * x.mean())
        res = y - (intercept + alpha * x)
        err = float(np.sqrt((res * res).sum() / (use.size - 2) / (dx * dx).sum())) if use.size > 2 else float("nan")
        return BasinUncertaintyFit(alpha, err, intercept, use + 1)

    def boundary_dimension(self, D: float = 2, **fit) -> float:
        """D - alpha of fit(**fit): the dimension of the basin boundary in the D-dimensional set the base points were drawn from."""
        return self.fit(**fit).boundary_dimension(D)


# ---- FTLE maps (include/sar.h: sar_runtime_ftle, sar_runtime_ftle_colorize) -----------------------------------------------------
FTLE_PIXEL_DTYPE = np.dtype(_abi.SarFtlePixel)


def ftle_params(coeffs, origin, du, dv, width: int, height: int, search_seed: int = 0, search_lo: float = -1.2, search_hi: float = 1.2,
                **params) -> "_abi.SarFtleParams":
    """sar_ftle_params_default() filled in: the map `coeffs` (a Config, 30 numbers or a search record), the plane of start points
    origin + du * tu + dv * tv over width x height pixels (row 0 at the high end of tv), and any of steps, bound, chunk."""
    p = _fill(_defaults(_abi.SarFtleParams, "sar_ftle_params_default"),
              dict(coeffs=_map_coeffs(coeffs, search_seed, search_lo, search_hi), origin=origin, du=du, dv=dv, width=width, height=height))
    return _fill(p, params, allowed=("steps", "bound", "chunk"))


class FtleMap:
    """One FTLE map of sar_runtime_ftle: `records` (height, width) of FTLE_PIXEL_DTYPE, `stats` (the counts and ftle_min / ftle_max
    over the finite ftle), `params`."""

    def __init__(self, runtime: Runtime, params, records: np.ndarray, stats: dict):
        self.runtime, self.params, self.records, self.stats = runtime, params, records, stats

    @property
    def status(self) -> np.ndarray:
        return self.records["status"]

    @property
    def escape_step(self) -> np.ndarray:
        return self.records["escape_step"]

    @property
    def flags(self) -> np.ndarray:
        """SAR_FTLE_EDGE | SAR_FTLE_ONE_SIDED_U | SAR_FTLE_ONE_SIDED_V | SAR_FTLE_NO_U | SAR_FTLE_NO_V per pixel."""
        return self.records["flags"]

    @property
    def end(self) -> np.ndarray:
        """(height, width, 3): F^N(start) of a BOUNDED pixel, 0 of a DIVERGED one."""
        return self.records["end"]

    @property
    def gram(self) -> np.ndarray:
        """(height, width, 3): g11, g12, g22."""
        return np.stack([self.records[f] for f in ("g11", "g12", "g22")], axis=-1)

    @property
    def stretch2(self) -> np.ndarray:
        return self.records["stretch2"]

    @property
    def ftle(self) -> np.ndarray:
        return self.records["ftle"]

    def start(self, x: int, y: int) -> np.ndarray:
        """Pixel (x, y)'s start point (host arithmetic, the device's doubles)."""
        out = np.empty(3)
        _check(_lib().sar_ftle_start(C.byref(self.params), int(x), int(y), _ptr(out)), "sar_ftle_start")
        return out

    def window(self) -> tuple:
        """The default colour window: the 1 % and 99 % quantiles of the finite ftle (numpy's), widened by 0.5 per side where they
        coincide; (0, 1) without a finite value."""
        f = self.ftle[np.isfinite(self.ftle)]
        if f.size == 0:
            return 0.0, 1.0
        lo, hi = (float(v) for v in np.quantile(f, (0.01, 0.99)))
        return (lo, hi) if lo < hi else (lo - 0.5, hi + 0.5)

    def colorize(self, config: Config, window=None, fade=None) -> np.ndarray:
        """(height, width, 4) RGBA16 (include/sar.h: sar_ftle_colors): a bounded pixel config's palette at its ftle's place in
        window = (lo, hi) — None: window() —, white on the basin boundary (EDGE), black without a finite ftle, an escaped pixel grey by
        its escape step; computed on the device from the records the runtime still holds. write_image takes it."""
        c = _defaults(_abi.SarFtleColors, "sar_ftle_colors_default")
        c.lo, c.hi = (float(v) for v in (self.window() if window is None else window))
        if fade is not None:
            c.fade = float(fade)
        return _colorize_records(self, "ftle", "FTLE map", self.records.shape, config, c)


def ftle_map(runtime: Runtime, coeffs, origin, du, dv, width: int = 256, height: int = 256, steps: int = 16, **params) -> FtleMap:
    """The finite-time Lyapunov exponent field of one map over a plane of start points, on the GPU (sar_runtime_ftle): pixel (x, y)
    starts at origin + du * x / (width - 1) + dv * (height - 1 - y) / (height - 1), as in basin_map, and runs `steps` steps; the
    differences between the end points of neighbouring pixels give the largest stretching `stretch2` of the flow map over the plane
    and ftle = ln(stretch2) / (2 steps). Ridges of ftle are the stable manifolds cut by the plane, at the picture's resolution.
    `coeffs`: a Config, 30 numbers or one search record. params: bound (default 1e6), chunk (pixels per launch; no result depends
    on it), and search_seed / search_lo / search_hi for a record."""
    p = ftle_params(coeffs, origin, du, dv, width, height, steps=steps, **params)
    _hold_records(runtime, "ftle", None)
    npix = p.width * p.height
    rec = np.empty(max(npix, 1), dtype=FTLE_PIXEL_DTYPE)
    st = _abi.SarFtleStats()
    _check(_lib().sar_runtime_ftle(runtime.handle, C.byref(p), _ptr(rec, _abi.SarFtlePixel), C.byref(st)), "sar_runtime_ftle")
    stats = {f: (int if t is C.c_uint64 else float)(getattr(st, f)) for f, t in st._fields_}
    m = FtleMap(runtime, p, rec[:npix].reshape(p.height, p.width), stats)
    _hold_records(runtime, "ftle", m)
    return m


# ---- density estimation (include/sar.h: sar_density_params) -------------------------------------------------------------
def density_params(**params) -> "_abi.SarDensityParams":
    """sar_density_params_default() (samples 64) with the given fields replaced."""
    return _fill(_defaults(_abi.SarDensityParams, "sar_density_params_default"), params)


def density_radius(samples: "int | None" = None) -> int:
    """R = floor(sqrt(samples - 1)), the widest reach of the filter (sar_density_radius): 7 at the default 64. No device."""
    p = density_params() if samples is None else density_params(samples=samples)
    r = C.c_uint32()
    _check(_lib().sar_density_radius(C.byref(p), C.byref(r)), "sar_density_radius")
    return int(r.value)


def density_weights(samples: int, c: int) -> np.ndarray:
    """Class c's radial table W_c[0 .. samples) as uint32, indexed by d2 = dx*dx + dy*dy (sar_density_weights): it sums to 65536 over
    the lattice; the identity row for c >= samples. No device."""
    p = density_params(samples=samples)
    out = np.zeros(int(samples), dtype=np.uint32)
    _check(_lib().sar_density_weights(C.byref(p), int(c), _ptr(out)), "sar_density_weights")
    return out


def density_filter(runtime: Runtime, **params) -> dict:
    """runtime.density_filter(stats=True, **params): filters the runtime's frame in place and returns the statistics."""
    return runtime.density_filter(stats=True, **params)


# ---- shaded rendering (include/sar.h: sar_shade_params) -------------------------------------------------------------------
def shade_params(window: "ColorRange | None" = None, **params) -> "_abi.SarShadeParams":
    """sar_shade_params_default() with the given fields replaced: light and background as sequences of three, window as a
    ColorRange (or None: no window)."""
    p = _defaults(_abi.SarShadeParams, "sar_shade_params_default")
    _fill(p, params, allowed=[f for f, _ in p._fields_ if f != "has_window"])   # (the window and its flag go together, below)
    if window is not None:
        p.has_window = 1
        p.window = window.c
    return p


def shade(config: Config, runtime: Runtime, stats: bool = False, window: "ColorRange | None" = None, **params):
    """runtime.shade(config, ...): the RGBA16 image of the lit surface — with stats=True, (image, statistics)."""
    return runtime.shade(config, stats=stats, window=window, **params)


def shade_device(config: Config, runtime: Runtime, rgba_dev_ptr: int, window: "ColorRange | None" = None, **params):
    """shade into a caller-provided device buffer (H*W*8 bytes, sar_shade_device); stream-ordered, no host sync: what goes on to
    convert_device for the other image formats."""
    p = shade_params(window=window, **params)
    _check(_lib().sar_shade_device(C.byref(config.c), runtime.handle, C.byref(p), None, C.c_void_p(rgba_dev_ptr)), "sar_shade_device")


# ---- volume rendering (include/sar.h: sar_runtime_volume*) --------------------------------------------------------------------
VOLUME_BELOW, VOLUME_ABOVE, VOLUME_NAN = -1, -2, -3


def volume_params(**params) -> "_abi.SarVolumeParams":
    """sar_volume_params_default() (z_lo -1, z_hi 1, slabs 64, add 0) with the given fields replaced."""
    return _fill(_defaults(_abi.SarVolumeParams, "sar_volume_params_default"), params)


def volume_march_params(**params) -> "_abi.SarVolumeMarchParams":
    """sar_volume_march_params_default() (half_count 0: from vmax, t_min 0, pos_lo 0, pos_hi 1, k0 0, k1 0: every slab, a black
    background) with the given fields replaced."""
    return _fill(_defaults(_abi.SarVolumeMarchParams, "sar_volume_march_params_default"), params)


def volume_slab(zf, slabs: int = 64, z_range=(-1.0, 1.0)) -> int:
    """The slab of the f32 depth zf (sar_volume_slab: host arithmetic, the device's doubles), or VOLUME_BELOW / VOLUME_ABOVE /
    VOLUME_NAN. No device."""
    p = volume_params(slabs=slabs, z_lo=z_range[0], z_hi=z_range[1])
    k = C.c_int32()
    _check(_lib().sar_volume_slab(C.byref(p), C.c_float(np.float32(zf)), C.byref(k)), "sar_volume_slab")
    return int(k.value)


def _volume_stats(st) -> dict:
    """sar_volume_stats by name: the counters as ints, z_min and z_max as floats."""
    return {f: (float if t is C.c_float else int)(getattr(st, f)) for f, t in st._fields_ if not f.startswith("_")}


class Volume:
    """The volume a runtime holds (sar_runtime_volume): `slabs` depth slabs of (height, width) u32 voxels over [z_lo, z_hi), slab
    slabs - 1 nearest to the viewer. `stats`: sar_volume_stats as a dict. The voxels stay on the device: .slabs / .section / .march
    read them, .add accumulates more jobs. The runtime holds ONE volume: a later volume() on it, set_width_height or close() ends
    this one."""

    def __init__(self, runtime: Runtime, config: Config, params, iterations: int, stats: dict):
        self.runtime, self.config, self.params, self.iterations, self.stats = runtime, config, params, int(iterations), stats
        _hold_records(runtime, "volume", self)

    @property
    def depth(self) -> int:
        return int(self.params.slabs)

    @property
    def z_range(self) -> tuple:
        return float(self.params.z_lo), float(self.params.z_hi)

    @property
    def edges(self) -> np.ndarray:
        """(slabs + 1,) the slabs' depth edges, z_lo + k * (z_hi - z_lo) / slabs (for plots: the slab of a depth is sar_volume_slab's)."""
        lo, hi = self.z_range
        return lo + np.arange(self.depth + 1, dtype=np.float64) * ((hi - lo) / self.depth)

    def _held(self):
        last = getattr(self.runtime, "_last_volume", None)
        if last is None or last() is not self:
            raise ValueError("the runtime holds another volume, or none, since this one was made")
        return self.runtime.handle

    def _window(self, k0, k1) -> tuple:
        return int(k0), self.depth if k1 is None else int(k1)

    def add(self, starts) -> dict:
        """Accumulates len(starts) more jobs of the same iterations into the held volume (add = 1); returns the new statistics."""
        s = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
        p, st = _copy_struct(self.params, add=1), _abi.SarVolumeStats()
        _check(_lib().sar_runtime_volume(C.byref(self.config.c), self._held(), C.byref(p), s.shape[0], self.iterations, _ptr(s), C.byref(st)),
               "sar_runtime_volume")
        self.stats = _volume_stats(st)
        return self.stats

    def slabs(self, k0: int = 0, k1=None) -> np.ndarray:
        """(k1 - k0, height, width) u32: the slabs themselves (sar_runtime_volume_read)."""
        k0, k1 = self._window(k0, k1)
        out = np.empty((max(k1 - k0, 0), self.config.c.height, self.config.c.width), dtype=np.uint32)
        _check(_lib().sar_runtime_volume_read(self._held(), k0, k1, _ptr(out)), "sar_runtime_volume_read")
        return out

    def section(self, k0: int = 0, k1=None) -> tuple:
        """(count, nearest) of the slabs k0 <= k < k1 (sar_runtime_volume_section): per pixel the wrapping u32 sum and, as int32, the
        largest non-empty k or -1."""
        k0, k1 = self._window(k0, k1)
        shape = (self.config.c.height, self.config.c.width)
        count, nearest = np.empty(shape, dtype=np.uint32), np.empty(shape, dtype=np.int32)
        _check(_lib().sar_runtime_volume_section(self._held(), k0, k1, _ptr(count), nearest.ctypes.data_as(C.POINTER(C.c_int32))),
               "sar_runtime_volume_section")
        return count, nearest

    def load_section(self, k0: int = 0, k1=None):
        """Loads the section into the runtime's frame (Runtime.load), so that auto_exposure, colorize, density_filter and shade work
        on it: count is the section, zbuf the centre depth of `nearest` (the sentinel -1 where the section is empty), steps the
        slab's palette position (nearest + 0.5) / slabs, max the section's largest count. Returns (count, nearest)."""
        count, nearest = self.section(k0, k1)
        lo, hi = self.z_range
        centre = (lo + (nearest.astype(np.float64) + 0.5) * ((hi - lo) / self.depth)).astype(np.float32)
        zbuf = np.where(nearest >= 0, centre, np.float32(-1.0)).astype(np.float32)
        steps = np.where(nearest >= 0, (nearest.astype(np.float64) + 0.5) / self.depth, 0.0)
        self.runtime.load(count, steps, zbuf, int(count.max(initial=0)))
        return count, nearest

    def march(self, config: "Config | None" = None, stats: bool = False, **params):
        """The translucent picture (sar_runtime_volume_march; volume_march_params: half_count, t_min, pos_lo, pos_hi, k0, k1,
        background): the slabs composited front to back, each in the palette's colour of its depth, as the (H, W, 4) uint16 array
        write_image accepts. config: another palette or `transparent` than the volume's own. With stats=True: (image, statistics)."""
        cfg = self.config if config is None else config
        p = volume_march_params(**params)
        out = np.empty((cfg.c.height, cfg.c.width, 4), dtype=np.uint16)
        st = _abi.SarVolumeMarchStats() if stats else None
        _check(_lib().sar_runtime_volume_march(C.byref(cfg.c), self._held(), C.byref(p), C.byref(st) if stats else None, _ptr(out)),
               "sar_runtime_volume_march")
        return (out, _stats_dict(st)) if stats else out

    def march_device(self, rgba_dev_ptr: int, config: "Config | None" = None, stats: bool = False, **params):
        """march into a caller-provided device buffer (H*W*8 bytes, sar_runtime_volume_march_device): stream-ordered, no host sync
        unless stats=True, which waits once and returns the statistics (else None)."""
        cfg = self.config if config is None else config
        p = volume_march_params(**params)
        st = _abi.SarVolumeMarchStats() if stats else None
        _check(_lib().sar_runtime_volume_march_device(C.byref(cfg.c), self._held(), C.byref(p), C.byref(st) if stats else None,
                                                      C.c_void_p(rgba_dev_ptr)), "sar_runtime_volume_march_device")
        return _stats_dict(st) if stats else None

    def close(self):
        """Frees the held volume (sar_runtime_volume_free), if it is still this one."""
        last = getattr(self.runtime, "_last_volume", None)
        if last is not None and last() is self:
            _check(_lib().sar_runtime_volume_free(self.runtime.handle), "sar_runtime_volume_free")
            _hold_records(self.runtime, "volume", None)


def volume(runtime: Runtime, config: Config, jobs: int = 1024, iterations: int = 1 << 16, slabs: int = 64, z_range=None, seed: int = 0,
           starts=None) -> Volume:
    """Fills the runtime's volume from `jobs` jobs of `iterations` counted iterations each in config's view (sar_runtime_volume) and
    returns it. starts: (jobs, 3) start points; None: the first `jobs` points of the stream of `seed`. z_range = (z_lo, z_hi); None
    learns it from a first call with one slab — a second run of the same jobs, as orbit_diagram's v_range=None costs one —: the
    depths seen, widened by 1/64 of their span on either side, or by 0.5 around a single depth."""
    s = start_points(seed, 0, jobs) if starts is None else np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
    if s.shape[0] != jobs:
        raise ValueError(f"starts must have shape ({jobs}, 3), got {s.shape}")

    def run(p):
        st = _abi.SarVolumeStats()
        _check(_lib().sar_runtime_volume(C.byref(config.c), runtime.handle, C.byref(p), jobs, int(iterations), _ptr(s), C.byref(st)),
               "sar_runtime_volume")
        return _volume_stats(st)

    if z_range is None:
        probe = run(volume_params(slabs=1))
        z_range = volume_learned_range(probe["z_min"], probe["z_max"])
    p = volume_params(slabs=slabs, z_lo=z_range[0], z_hi=z_range[1])
    _hold_records(runtime, "volume", None)
    return Volume(runtime, config.copy(), p, iterations, run(p))


def volume_learned_range(z_min: float, z_max: float) -> tuple:
    """The range volume(z_range=None) takes from the depths a probe call saw: (z_min - span / 64, z_max + span / 64), or 0.5 on either
    side of a single depth; (-1, 1) where no finite depth was seen."""
    z_min, z_max = float(z_min), float(z_max)
    if not z_min <= z_max:
        return -1.0, 1.0
    span = z_max - z_min
    return (z_min - span / 64.0, z_max + span / 64.0) if span > 0.0 else (z_min - 0.5, z_max + 0.5)


# ---- flows: quadratic ODE systems through RK4 (include/sar.h: sar_runtime_render_flow) ----------------------------------------
# The rows of a field in Config.from_coefficients' order [1, x, x^2, xy, xz, y, y^2, yz, z, z^2], by monomial
_MONOMIAL = {"1": 0, "x": 1, "xx": 2, "xy": 3, "xz": 4, "y": 5, "yy": 6, "yz": 7, "z": 8, "zz": 9}
# name -> (the constants with their customary values, rows (x', y', z') as {monomial: factor or a function of the constants})
_FLOWS = {
    # Lorenz 1963: x' = sigma (y - x), y' = x (rho - z) - y, z' = x y - beta z
    "lorenz": (dict(sigma=10.0, rho=28.0, beta=8.0 / 3.0),
               ({"x": lambda k: -k["sigma"], "y": lambda k: k["sigma"]}, {"x": lambda k: k["rho"], "xz": -1.0, "y": -1.0},
                {"xy": 1.0, "z": lambda k: -k["beta"]})),
    # Roessler 1976: x' = -y - z, y' = x + a y, z' = b + z (x - c)
    "rossler": (dict(a=0.2, b=0.2, c=5.7),
                ({"y": -1.0, "z": -1.0}, {"x": 1.0, "y": lambda k: k["a"]}, {"1": lambda k: k["b"], "xz": 1.0, "z": lambda k: -k["c"]})),
    # Chen & Ueta 1999: x' = a (y - x), y' = (c - a) x - x z + c y, z' = x y - b z
    "chen": (dict(a=35.0, b=3.0, c=28.0),
             ({"x": lambda k: -k["a"], "y": lambda k: k["a"]}, {"x": lambda k: k["c"] - k["a"], "xz": -1.0, "y": lambda k: k["c"]},
              {"xy": 1.0, "z": lambda k: -k["b"]})),
    # Nose-Hoover oscillator (Sprott's case A): x' = y, y' = -x + y z, z' = a - y^2
    "nose_hoover": (dict(a=1.0), ({"y": 1.0}, {"x": -1.0, "yz": 1.0}, {"1": lambda k: k["a"], "yy": -1.0})),
    # Sprott 1994, "Some simple chaotic flows", Table 1, cases A .. S
    "sprott_a": ({}, ({"y": 1.0}, {"x": -1.0, "yz": 1.0}, {"1": 1.0, "yy": -1.0})),
    "sprott_b": ({}, ({"yz": 1.0}, {"x": 1.0, "y": -1.0}, {"1": 1.0, "xy": -1.0})),
    "sprott_c": ({}, ({"yz": 1.0}, {"x": 1.0, "y": -1.0}, {"1": 1.0, "xx": -1.0})),
    "sprott_d": ({}, ({"y": -1.0}, {"x": 1.0, "z": 1.0}, {"xz": 1.0, "yy": 3.0})),
    "sprott_e": ({}, ({"yz": 1.0}, {"xx": 1.0, "y": -1.0}, {"1": 1.0, "x": -4.0})),
    "sprott_f": ({}, ({"y": 1.0, "z": 1.0}, {"x": -1.0, "y": 0.5}, {"xx": 1.0, "z": -1.0})),
    "sprott_g": ({}, ({"x": 0.4, "z": 1.0}, {"xz": 1.0, "y": -1.0}, {"x": -1.0, "y": 1.0})),
    "sprott_h": ({}, ({"y": -1.0, "zz": 1.0}, {"x": 1.0, "y": 0.5}, {"x": 1.0, "z": -1.0})),
    "sprott_i": ({}, ({"y": -0.2}, {"x": 1.0, "z": 1.0}, {"x": 1.0, "yy": 1.0, "z": -1.0})),
    "sprott_j": ({}, ({"z": 2.0}, {"y": -2.0, "z": 1.0}, {"x": -1.0, "y": 1.0, "yy": 1.0})),
    "sprott_k": ({}, ({"xy": 1.0, "z": -1.0}, {"x": 1.0, "y": -1.0}, {"x": 1.0, "z": 0.3})),
    "sprott_l": ({}, ({"y": 1.0, "z": 3.9}, {"xx": 0.9, "y": -1.0}, {"1": 1.0, "x": -1.0})),
    "sprott_m": ({}, ({"z": -1.0}, {"xx": -1.0, "y": -1.0}, {"1": 1.7, "x": 1.7, "y": 1.0})),
    "sprott_n": ({}, ({"y": -2.0}, {"x": 1.0, "zz": 1.0}, {"1": 1.0, "y": 1.0, "z": -2.0})),
    "sprott_o": ({}, ({"y": 1.0}, {"x": 1.0, "z": -1.0}, {"x": 1.0, "xz": 1.0, "y": 2.7})),
    "sprott_p": ({}, ({"y": 2.7, "z": 1.0}, {"x": -1.0, "yy": 1.0}, {"x": 1.0, "y": 1.0})),
    "sprott_q": ({}, ({"z": -1.0}, {"x": 1.0, "y": -1.0}, {"x": 3.1, "yy": 1.0, "z": 0.5})),
    "sprott_r": ({}, ({"1": 0.9, "y": -1.0}, {"1": 0.4, "z": 1.0}, {"xy": 1.0, "z": -1.0})),
    "sprott_s": ({}, ({"x": -1.0, "y": -4.0}, {"x": 1.0, "zz": 1.0}, {"1": 1.0, "x": 1.0})),
}
FLOW_SYSTEMS = tuple(_FLOWS)


def flow_coefficients(name: str, **constants) -> np.ndarray:
    """The (3, 10) rows x', y', z' of a named quadratic vector field, in Config.from_coefficients' order [1, x, x^2, xy, xz, y, y^2,
    yz, z, z^2], written from the published equations: "lorenz" (sigma 10, rho 28, beta 8/3), "rossler" (a 0.2, b 0.2, c 5.7), "chen"
    (a 35, b 3, c 28), "nose_hoover" (a 1) and Sprott's simple chaotic flows "sprott_a" .. "sprott_s" (no constants to set).
    FLOW_SYSTEMS lists the names. Host arithmetic."""
    if name not in _FLOWS:
        raise ValueError(f"unknown flow {name!r} ({', '.join(FLOW_SYSTEMS)})")
    defaults, rows = _FLOWS[name]
    unknown = sorted(set(constants) - set(defaults))
    if unknown:
        raise ValueError(f"{name} has no constant {unknown[0]!r} ({', '.join(defaults) or 'none'})")
    k = {**defaults, **{c: float(v) for c, v in constants.items()}}
    out = np.zeros((3, 10), dtype=np.float64)
    for r, row in enumerate(rows):
        for monomial, f in row.items():
            out[r, _MONOMIAL[monomial]] = f(k) if callable(f) else f
    return out


def flow_params(**fields) -> "_abi.SarFlowParams":
    """sar_flow_params_default() (dt 0.01, bound 1e6, transient 1000, stride 1, plot 1, chunk_jobs 0: 2^17, chunk_steps 0: 2^12) with
    the given fields replaced."""
    return _fill(_defaults(_abi.SarFlowParams, "sar_flow_params_default"), fields)


def flow_step(config: Config, p, dt: float = 0.01, bound: float = 1e6, within: bool = False):
    """One RK4 step of config's field from the point p on the host, in the device's arithmetic (sar_flow_step): the new point as a
    (3,) array — with within=True, (point, whether it stayed within `bound`). No device."""
    xyz = np.array(p, dtype=np.float64).reshape(3).copy()
    ok = C.c_int32()
    _check(_lib().sar_flow_step(C.byref(config.c), C.byref(flow_params(dt=dt, bound=bound)), _ptr(xyz), C.byref(ok)), "sar_flow_step")
    return (xyz, bool(ok.value)) if within else xyz


def _flow_stats(st) -> dict:
    """sar_flow_stats by name: the counters and max as ints, the extent as a (6,) array."""
    return {**_stats_dict(st), "extent": np.array(st.extent, dtype=np.float64)}


def render_flow(config: Config, runtime: Runtime, dt: float = 0.01, jobs: int = 1024, steps: int = 1 << 12, transient: int = 1000,
                stride: int = 1, bound: float = 1e6, starts=None, seed: int = 0, stats: bool = False, **more) -> "dict | None":
    """Integrates config's 30 coefficients as the vector field p' = P(p) — flow_coefficients() names the classical ones — with
    classical RK4 of the fixed step dt, `jobs` trajectories of `transient` uncounted and then `steps` counted steps, and plots every
    stride-th counted point into the runtime's frame in config's view (sar_runtime_render_flow). It accumulates onto an un-reset
    runtime; colorize, auto exposure, auto colour range, density_filter, shade and write_image then work as on a map's frame. A job
    that leaves the box |x|, |y|, |z| <= bound has escaped and plots nothing more. starts: (jobs, 3) start points; None: the first
    `jobs` points of the stream of `seed`, as volume() draws them. more: plot, chunk_jobs, chunk_steps of flow_params. With
    stats=True: sar_flow_stats as a dict."""
    s = start_points(seed, 0, jobs) if starts is None else np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
    if s.shape[0] != jobs:
        raise ValueError(f"starts must have shape ({jobs}, 3), got {s.shape}")
    p = flow_params(dt=dt, bound=bound, transient=transient, stride=stride, **more)
    st = _abi.SarFlowStats()
    _check(_lib().sar_runtime_render_flow(C.byref(config.c), runtime.handle, C.byref(p), jobs, int(steps), _ptr(s), C.byref(st)),
           "sar_runtime_render_flow")
    return _flow_stats(st) if stats else None


def flow_extent(config: Config, runtime: Runtime, dt: float = 0.01, jobs: int = 1024, steps: int = 1 << 12, **more) -> np.ndarray:
    """[xmin, xmax, ymin, ymax, zmin, zmax] of the counted points of a flow in raw coordinates: a plot = 0 call of render_flow, which
    leaves the runtime's frame untouched. more: render_flow's other arguments."""
    return render_flow(config, runtime, dt=dt, jobs=jobs, steps=steps, stats=True, plot=0, **more)["extent"]


def flow_view(config: Config, runtime: Runtime, dt: float = 0.01, jobs: int = 1024, steps: int = 1 << 12, margin: float = 0.05,
              sweep: bool = False, **more) -> Config:
    """config with its view framed on the flow: flow_extent, then frame_view_box on that raw box. Conservative, as frame_view_box
    is: the rotated box bounds the rotated trajectory."""
    return frame_view_box(config, flow_extent(config, runtime, dt=dt, jobs=jobs, steps=steps, **more), margin=margin, sweep=sweep)


# ---- Poincare sections of flows (include/sar.h: sar_runtime_section) ----------------------------------------------------------
SECTION_RECORD_DTYPE = np.dtype(_abi.SarSectionRecord)


def section_params(**fields) -> "_abi.SarSectionParams":
    """sar_section_params_default() (dt 0.01, bound 1e6, transient 1000, direction +1, samples 1024, max_steps 2^20, plot 0, the
    chunks 0: flows' defaults; the surface all zero, which every entry refuses) with the given fields replaced."""
    return _fill(_defaults(_abi.SarSectionParams, "sar_section_params_default"), fields)


def section_plane(normal, offset: float = 0.0, point=None) -> np.ndarray:
    """The ten surface coefficients of the plane normal . p = offset — or, with `point`, of the plane through it: offset =
    normal . point. Host arithmetic."""
    n = np.asarray(normal, dtype=np.float64).reshape(3)
    d = float(offset) if point is None else float(np.dot(n, np.asarray(point, dtype=np.float64).reshape(3)))
    s = np.zeros(10, dtype=np.float64)
    s[0], s[1], s[5], s[8] = -d, n[0], n[1], n[2]
    return s


def section_extremum(coeffs_or_config, axis: int) -> np.ndarray:
    """The surface on which coordinate `axis` (0, 1, 2) of the flow has an extremum: row `axis` of the field itself, p_axis' = 0.
    direction=-1 takes its maxima, +1 its minima."""
    if axis not in (0, 1, 2):
        raise ValueError(f"axis must be 0, 1 or 2 ({axis!r})")
    return _base_coeffs(coeffs_or_config).reshape(3, 10)[axis].copy()


def section_step(config: Config, surface, p, dt: float = 0.01, bound: float = 1e6, direction: int = 1):
    """One counted step of config's field from the point p on the host, in the device's arithmetic (sar_section_step):
    (p1, kind, crossing, dt) — kind 0 no crossing, 1 refined by Henon's step, 2 rough, -1 escaped; crossing (3,) and the time dt
    from p to it are None unless kind is 1 or 2. No device."""
    xyz = np.array(p, dtype=np.float64).reshape(3).copy()
    q, t, kind = np.zeros(3, dtype=np.float64), C.c_double(), C.c_int32()
    prm = section_params(surface=surface, dt=dt, bound=bound, direction=direction)
    _check(_lib().sar_section_step(C.byref(config.c), C.byref(prm), _ptr(xyz), _ptr(q), C.byref(t), C.byref(kind)), "sar_section_step")
    hit = kind.value > 0
    return xyz, int(kind.value), (q if hit else None), (float(t.value) if hit else None)


class FlowSection:
    """What flow_section() recorded: points (jobs, samples, 3) and ret (jobs, samples), NaN where unfilled; records
    (SECTION_RECORD_DTYPE, one per job); stats (sar_section_stats as a dict); full, the mask of the jobs that hold all their
    samples."""

    def __init__(self, surface, points, ret, records, stats):
        self.surface, self.points, self.ret, self.records, self.stats = surface, points, ret, records, stats
        self.full = records["status"] == _abi.SAR_SECTION_FULL

    def trajectories(self) -> np.ndarray:
        """The full jobs' crossings, (n_full, samples, 3): the shape pair_histogram(..., samples=), box_counts, recurrence_lines
        and power_spectra take."""
        return np.ascontiguousarray(self.points[self.full])

    def return_map(self, proj=(0.0, 0.0, 1.0), lag: int = 1) -> np.ndarray:
        """The pairs (v_k, v_{k + lag}) of the full jobs, v = proj . q: (n_full * (samples - lag), 2)."""
        if lag < 1:
            raise ValueError(f"lag must be at least 1 ({lag})")
        v = self.trajectories() @ np.asarray(proj, dtype=np.float64).reshape(3)
        return np.stack([v[:, :-lag].reshape(-1), v[:, lag:].reshape(-1)], axis=1)

    def view(self, config: Config, margin: float = 0.05) -> Config:
        """config with its view framed on the recorded crossings: frame_view_box on stats["extent"]."""
        return frame_view_box(config, self.stats["extent"], margin=margin)


def _section_stats(st) -> dict:
    """sar_section_stats by name: the counters and max as ints, the extent as a (6,) array, the three doubles as floats."""
    out = {f: (float if t is C.c_double else int)(getattr(st, f)) for f, t in st._fields_ if not f.startswith("_") and not issubclass(t, C.Array)}
    return {**out, "extent": np.array(st.extent, dtype=np.float64)}


def flow_section(config: Config, runtime: Runtime, surface, dt: float = 0.01, jobs: int = 64, samples: int = 1024, direction: int = 1,
                 max_steps: int = 1 << 20, transient: int = 1000, bound: float = 1e6, starts=None, seed: int = 0, plot: bool = False,
                 **more) -> FlowSection:
    """The Poincare section of config's flow on the surface g = 0 (section_plane(), section_extremum() or any ten coefficients of
    a quadric): `jobs` trajectories as render_flow runs them, each recording up to `samples` crossings in `direction` (+1 up, -1
    down, 0 both) behind its first one, refined by one Henon step, with the return time between consecutive crossings
    (sar_runtime_section). A job gives up after max_steps counted steps. plot=True also plots the crossings into the runtime's
    frame in config's view, the hue their return time; set_color_range spreads it over the palette. starts: (jobs, 3) start
    points; None: the first `jobs` points of the stream of `seed`. more: chunk_jobs, chunk_steps of section_params."""
    s = start_points(seed, 0, jobs) if starts is None else np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
    if s.shape[0] != jobs:
        raise ValueError(f"starts must have shape ({jobs}, 3), got {s.shape}")
    p = section_params(surface=surface, dt=dt, bound=bound, transient=transient, direction=direction, samples=samples, max_steps=max_steps,
                       plot=int(bool(plot)), **more)
    points, ret = np.empty((jobs, int(samples), 3), dtype=np.float64), np.empty((jobs, int(samples)), dtype=np.float64)
    records, st = np.zeros(jobs, dtype=SECTION_RECORD_DTYPE), _abi.SarSectionStats()
    _check(_lib().sar_runtime_section(C.byref(config.c), runtime.handle if runtime is not None else None, C.byref(p), jobs, _ptr(s), _ptr(points),
                                      _ptr(ret), _ptr(records, _abi.SarSectionRecord), C.byref(st)), "sar_runtime_section")
    return FlowSection(np.array(p.surface, dtype=np.float64), points, ret, records, _section_stats(st))


# ---- auto exposure (include/sar.h: sar_exposure_params) -----------------------------------------------------------------
def exposure_params(**params) -> "_abi.SarExposureParams":
    """sar_exposure_params_default() (q_black 0, q_white 0.995, level_black 0, level_white 1) with the given fields replaced."""
    return _fill(_defaults(_abi.SarExposureParams, "sar_exposure_params_default"), params)


@dataclass
class Exposure:
    """What sar_runtime_exposure found: the constants colorize uses (the solved ones, or config's when `applied` is False), the
    black and white quantile counts, the covered pixels and colorize's max M."""
    offset: float
    factor: float
    black_count: int
    white_count: int
    covered: int
    max: int
    applied: bool


def exposure(config: Config, runtime: Runtime, **params) -> Exposure:
    """The exposure of the runtime's current buffers (sar_runtime_exposure), computed on the device; waits for it."""
    p = exposure_params(**params)
    out = _abi.SarExposure()
    _check(_lib().sar_runtime_exposure(C.byref(config.c), runtime.handle, C.byref(p), C.byref(out)), "sar_runtime_exposure")
    return Exposure(out.offset, out.factor, int(out.black_count), int(out.white_count), int(out.covered), int(out.max), bool(out.applied))


def auto_exposure(config: Config, runtime: Runtime, **params) -> Config:
    """config with brightness_offset / brightness_factor replaced by the exposure of the runtime's frame: a "hold" exposure —
    colorize every frame of a sweep with it and the sweep does not flicker."""
    e = exposure(config, runtime, **params)
    return config.replace(brightness_offset=e.offset, brightness_factor=e.factor)


# ---- auto colour range (include/sar.h: sar_color_range_params) ---------------------------------------------------------
def color_range_params(**params) -> "_abi.SarColorRangeParams":
    """sar_color_range_params_default() (q_lo 0.01, q_hi 0.99, pos_lo 0, pos_hi 1) with the given fields replaced."""
    return _fill(_defaults(_abi.SarColorRangeParams, "sar_color_range_params_default"), params)


@dataclass
class ColorRange:
    """What sar_runtime_color_range found: the window [lo, hi] of steps that maps to the palette positions [pos_lo, pos_hi], the
    pixels it was chosen from, and whether colorize applies it (False: steps as they are)."""
    lo: float
    hi: float
    pos_lo: float = 0.0
    pos_hi: float = 1.0
    covered: int = 0
    applied: bool = True

    @property
    def c(self) -> "_abi.SarColorRange":
        return _abi.SarColorRange(self.lo, self.hi, self.pos_lo, self.pos_hi, int(self.covered), 1 if self.applied else 0)


def color_range(config: Config, runtime: Runtime, **params) -> ColorRange:
    """The colour range of the runtime's current buffers (sar_runtime_color_range), computed on the device; waits for it."""
    p = color_range_params(**params)
    out = _abi.SarColorRange()
    _check(_lib().sar_runtime_color_range(C.byref(config.c), runtime.handle, C.byref(p), C.byref(out)), "sar_runtime_color_range")
    return ColorRange(out.lo, out.hi, out.pos_lo, out.pos_hi, int(out.covered), bool(out.applied))


def color_range_to_velocity(config: Config, color_range: ColorRange) -> Config:
    """config with the window folded into the AdjustedVelocity constants (sar_color_range_to_velocity): a render with it carries
    the window in its steps. Algebraically the same window, not bit for bit."""
    out = config.replace()
    _check(_lib().sar_color_range_to_velocity(C.byref(config.c), C.byref(color_range.c), C.byref(out.c)), "sar_color_range_to_velocity")
    return out


def auto_color(config: Config, runtime: Runtime, **params) -> Config:
    """config with ct_offset / ct_factor replaced so that its steps carry the colour range of the runtime's frame: constants that
    can go back into the reference program's AdjustedVelocity { offset, factor }."""
    return color_range_to_velocity(config, color_range(config, runtime, **params))


# ---- image export (src/bin/main.rs:40-100) -------------------------------------------------------------------
_FMT_SHAPE = {_abi.SAR_FMT_RGBA16: (4, np.uint16), _abi.SAR_FMT_RGB16: (3, np.uint16),
              _abi.SAR_FMT_RGBA8: (4, np.uint8), _abi.SAR_FMT_RGB8: (3, np.uint8)}


def image_format(transparent: bool, eight_bit: bool) -> int:
    """The format ``write_image_matches`` converts to for (--transparent, --8bit) (src/bin/main.rs:52-57)."""
    return int(_lib().sar_image_format(int(bool(transparent)), int(bool(eight_bit))))


def colorize_format(config: Config, runtime: Runtime, fmt: int) -> np.ndarray:
    """``colorize`` followed by the CLI's format conversion, both on the device; one copy of the converted image."""
    if fmt not in _FMT_SHAPE:
        raise ValueError(f"unknown image format {fmt}")
    ch, dt = _FMT_SHAPE[fmt]
    out = np.empty((config.c.height, config.c.width, ch), dtype=dt)
    _check(_lib().sar_colorize_format(C.byref(config.c), runtime.handle, fmt, out.ctypes.data_as(C.c_void_p)),
           "sar_colorize_format")
    return out


def host_reserve(nbytes: int, count: int):
    """Announces `count` page-locked blocks of `nbytes` to come (sar_host_reserve): helper threads map and zero them ahead of the
    HostImage()s that take them. (0, 0) releases what is left."""
    _check(_lib().sar_host_reserve(int(nbytes), int(count)), "sar_host_reserve")


def image_bytes(fmt: int, width: int, height: int) -> int:
    return int(_lib().sar_image_bytes(fmt, width, height))


class HostImage:
    """A page-locked host image of (height, width, channels-of-fmt) for ``colorize_format_async``; `array` is a numpy
    view of it, valid until ``close``."""

    def __init__(self, width: int, height: int, fmt: int):
        if fmt not in _FMT_SHAPE:
            raise ValueError(f"unknown image format {fmt}")
        ch, dt = _FMT_SHAPE[fmt]
        self.fmt = fmt
        nbytes = int(_lib().sar_image_bytes(fmt, width, height))
        p = C.c_void_p()
        _check(_lib().sar_host_alloc(nbytes, C.byref(p)), "sar_host_alloc")
        self.ptr = p.value
        self.array = np.frombuffer((C.c_ubyte * nbytes).from_address(self.ptr), dtype=dt).reshape(height, width, ch)

    def close(self):
        if self.ptr:
            self.array = None
            _check(_lib().sar_host_free(C.c_void_p(self.ptr)), "sar_host_free")
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _image_fits(image: "HostImage", width: int, height: int, where: str):
    """The C entry points take a bare pointer and copy the runtime's image into it: a host image of another size (one made before
    sar_runtime_set_width_height, say) is refused here, where its size is known."""
    if image.array is None or image.array.shape[:2] != (height, width):
        have = "closed" if image.array is None else f"{image.array.shape[1]}x{image.array.shape[0]}"
        raise ValueError(f"{where}: the host image is {have}, the frame is {width}x{height}")


def colorize_format_async(config: Config, runtime: Runtime, image: HostImage) -> int:
    """``colorize_format`` into a page-locked image, enqueued only: returns the ticket ``wait_image`` takes. The runtime
    may be reset and rendered into again meanwhile (the `sequence` sweep reads frame k back under frame k+1)."""
    _image_fits(image, config.c.width, config.c.height, "colorize_format_async")
    t = C.c_uint64()
    _check(_lib().sar_colorize_format_async(C.byref(config.c), runtime.handle, image.fmt, C.c_void_p(image.ptr), C.byref(t)),
           "sar_colorize_format_async")
    return int(t.value)


def colorize_format_device(config: Config, runtime: Runtime, fmt: int):
    """colorize + the CLI's conversion, the image left in the runtime's device memory (sar_colorize_format_async with no host
    image): `read_image_async` fetches it later. Enqueues only."""
    _check(_lib().sar_colorize_format_async(C.byref(config.c), runtime.handle, fmt, None, None), "sar_colorize_format_async")


def read_image_async(runtime: Runtime, image: "HostImage") -> int:
    """The read-back of the image `colorize_format_device` left, into a page-locked host image; returns the ticket. The image
    must have the runtime's size (a runtime resized since the image was made has another)."""
    _image_fits(image, *runtime.dims(), "read_image_async")
    t = C.c_uint64()
    _check(_lib().sar_runtime_read_image_async(runtime.handle, C.c_void_p(image.ptr), C.byref(t)), "sar_runtime_read_image_async")
    return int(t.value)


def image_done(runtime: Runtime, ticket: int) -> bool:
    """Whether the read-back behind `ticket` has completed (no wait)."""
    d = C.c_int(0)
    _check(_lib().sar_runtime_image_done(runtime.handle, ticket, C.byref(d)), "sar_runtime_image_done")
    return bool(d.value)


def wait_image(runtime: Runtime, ticket: int):
    _check(_lib().sar_runtime_wait_image(runtime.handle, ticket), "sar_runtime_wait_image")


def convert_device(runtime: Runtime, rgba16_dev_ptr: int, fmt: int, out_dev_ptr: int):
    """RGBA16 -> fmt between two device buffers, ordered on the runtime's stream."""
    _check(_lib().sar_image_convert_device(runtime.handle, C.c_void_p(rgba16_dev_ptr), fmt, C.c_void_p(out_dev_ptr)),
           "sar_image_convert_device")


def _fmt_of(image: np.ndarray) -> int:
    for fmt, (ch, dt) in _FMT_SHAPE.items():
        if image.ndim == 3 and image.shape[2] == ch and image.dtype == dt:
            return fmt
    raise ValueError("image must be (H, W, 3|4) of uint8 or uint16")


def write_image(image: np.ndarray, path: str, kind: str = "png"):
    """Encodes a host image (as returned by ``colorize_format``) as PNG, BMP or PAM."""
    fmt = _fmt_of(image)
    img = np.ascontiguousarray(image)
    fn = {"png": _lib().sar_write_png, "bmp": _lib().sar_write_bmp, "pam": _lib().sar_write_pam}[kind]
    _check(fn(os.fsencode(path), fmt, img.shape[1], img.shape[0], img.ctypes.data_as(C.c_void_p)), f"sar_write_{kind}")


def write_image_matches(config: Config, runtime: Runtime, name: str, transparent: bool = False, eight_bit: bool = False,
                        pam: bool = False, bmp: bool = False) -> str:
    """``write_image_matches`` (src/bin/main.rs:40-100): convert by (transparent, 8bit), pick the encoder by
    (pam, bmp) — both need 8bit (:256-258) — and replace the extension of ``name``. Returns the path written."""
    if (pam or bmp) and not eight_bit:
        raise ValueError("--pam / --bmp require --8bit (src/bin/main.rs:256-258)")
    kind = "pam" if pam else ("bmp" if bmp else "png")
    path = os.path.splitext(name)[0] + "." + kind
    write_image(colorize_format(config, runtime, image_format(transparent, eight_bit)), path, kind)
    return path


class ParallelRenderer:
    """``ParallelRenderer`` (src/lib.rs:908): `units` stands in for the thread count the job split
    divides by (0 = one trajectory per SIMD lane of the device)."""

    def __init__(self, device: int = 0, units: int = 0, seed: int = 0, devices=None):
        """devices: a list of HIP device ordinals -> one renderer over several GPUs (sar_renderer_new_multi): the jobs
        are sharded over them, the partial buffers merged point-to-point over xGMI, all behind the C ABI."""
        h = C.c_void_p()
        if devices is not None:
            devs = (C.c_int * len(devices))(*[int(d) for d in devices])
            _check(_lib().sar_renderer_new_multi(devs, len(devices), units, seed, C.byref(h)), "sar_renderer_new_multi")
            device = int(devices[0])
        else:
            _check(_lib().sar_renderer_new(device, units, seed, C.byref(h)), "sar_renderer_new")
        self._h = h
        self.device = device

    def num_devices(self) -> int:
        n = C.c_uint32()
        _check(_lib().sar_renderer_num_devices(self._h, C.byref(n)), "sar_renderer_num_devices")
        return int(n.value)

    def last_timing(self) -> dict:
        t = SarParallelTiming()
        _check(_lib().sar_renderer_last_timing(self._h, C.byref(t)), "sar_renderer_last_timing")
        return {k: getattr(t, k) for k, _ in SarParallelTiming._fields_}

    def set_exchange(self, mode: int):
        """0 automatic, 1 dense (whole slices by peer copies), 2 sparse (kernels push the touched segments' records)."""
        _check(_lib().sar_renderer_set_exchange(self._h, int(mode)), "sar_renderer_set_exchange")

    def set_exposure(self, off=..., /, **params):
        """Auto exposure of render_parallel's colorize (sar_renderer_set_exposure; see Runtime.set_exposure). One device only: a
        renderer over several refuses to render with it on. set_exposure(None) turns it off."""
        _check(_lib().sar_renderer_set_exposure(self._h, _mode_params(exposure_params, off, params)), "sar_renderer_set_exposure")

    def set_color_range(self, off=..., /, **params):
        """Auto colour range of render_parallel's colorize (sar_renderer_set_color_range; see Runtime.set_color_range). One device
        only: a renderer over several refuses to render with it on. set_color_range(None) turns it off."""
        _check(_lib().sar_renderer_set_color_range(self._h, _mode_params(color_range_params, off, params)), "sar_renderer_set_color_range")

    def num_threads(self) -> int:
        n = C.c_uint32()
        _check(_lib().sar_renderer_num_units(self._h, C.byref(n)), "sar_renderer_num_units")
        return int(n.value)

    def runtime(self) -> Runtime:
        h = C.c_void_p()
        _check(_lib().sar_renderer_runtime(self._h, C.byref(h)), "sar_renderer_runtime")
        return Runtime(None, self.device, _borrowed=h)

    def shutdown(self):
        if getattr(self, "_h", None):
            _lib().sar_renderer_shutdown(self._h)
            self._h = None

    def __del__(self):
        try:
            self.shutdown()
        except Exception:
            pass


def render_parallel(renderer: ParallelRenderer, config: Config, jobs_per_thread: int) -> np.ndarray:
    """``render_parallel(&mut renderer, config, jobs_per_thread) -> FinalImage`` (src/lib.rs:1051)."""
    out = np.empty((config.c.height, config.c.width, 4), dtype=np.uint16)
    _check(_lib().sar_render_parallel(renderer._h, C.byref(config.c), jobs_per_thread, _ptr(out)), "sar_render_parallel")
    return out


def render_parallel_into(renderer: ParallelRenderer, config: Config, jobs_per_thread: int, rgba_host_ptr: int):
    """render_parallel into caller-owned host memory (width*height*4 uint16; e.g. pinned memory: every device then
    copies its slice straight into it)."""
    _check(_lib().sar_render_parallel(renderer._h, C.byref(config.c), jobs_per_thread,
                                      C.cast(C.c_void_p(rgba_host_ptr), C.POINTER(C.c_uint16))), "sar_render_parallel")
