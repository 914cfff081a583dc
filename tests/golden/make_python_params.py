"""Records what the Python parameter builders of strange_attractor_renderer_amd.api give, as tests/golden/python_params.json:

    python tests/golden/make_python_params.py

Run it AT THE PARENT COMMIT of a change to the builders: the file is a record of the code BEFORE the change, which
tests/test_python_params_host.py replays against the tree under test, byte for byte and class for class. It needs the library's
host half only (the *_default entry points), no device.

A row is one call of one builder, all arguments by keyword, and what it gives: the struct's bytes as hex, or the exception's class
name. For every builder the table holds the defaults, every settable field set once (arrays and an integral float included), the
ends of every integer field's range and one step beyond each, an unknown key, a padding key, a key the builder forbids, and arrays
of the wrong length.

"tightened" holds the rows whose expectation is NOT the recorded one: calls the recorded code let through (their "recorded" entry
says what it gave) and the builders now refuse, each with the reason. A row marked for tightening that the recorded code refuses
with the same class already is an ordinary row.

"dtypes" holds the public record dtypes as literals — name, format, shape and offset of every field, and the item size — with the
_abi structure each one mirrors."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "python_params.json")

NON_INTEGRAL = "a non-integral value for an integer field is refused by every builder, not truncated"
SHADE_RANGE = "shade_params checks the range of background and smooth, ctypes no longer wraps them"

COEFFS = [round(0.03125 * (k - 11), 6) for k in range(30)]
OTHER = [round(0.015625 * (17 - k), 6) for k in range(30)]
PLANE = dict(base=COEFFS, axes=[3, 17], x_range=[-0.5, 0.25], y_range=[0.125, 0.75], width=5, height=4)
BASIN = dict(coeffs=COEFFS, origin=[0.5, -0.25, 0.125], du=[1.0, 0.0, 0.5], dv=[0.0, 2.0, -0.5], width=5, height=4)
ORBIT = dict(a=COEFFS, axis=4, range=[-1.0, 0.5])

# builder -> (the _abi structure, the arguments every call starts from, the fields a keyword of the same name sets)
BUILDERS = {
    "search_params": ("SarSearchParams", {}, "seed lo hi start transient steps bound min_lyapunov min_ky_dim keep_rejected"),
    "gallery_params": ("SarGalleryParams", {}, "tile_width tile_height cols jobs iterations seed"),
    "plane_params": ("SarPlaneParams", PLANE, "width height start transient steps bound"),
    "plane_colors": ("SarPlaneColors", {}, "threshold chaos_scale order_scale"),
    "period_params": ("SarPeriodParams", {}, "width height start transient max_period bound eps"),
    "period_colors": ("SarPeriodColors", {}, "colours"),
    "orbit_params": ("SarOrbitParams", ORBIT, "width height jobs transient steps seed bound proj"),
    "pairs_params": ("SarPairsParams", {}, "samples theiler sub_bits e_min e_max"),
    "corrdim_params": ("SarCorrdimParams", {}, "jobs samples stride transient theiler sub_bits e_min e_max seed bound c_lo r_hi_fraction"),
    "box_params": ("SarBoxParams", {}, "levels origin size"),
    "boxdim_params": ("SarBoxdimParams", {}, "jobs samples stride transient levels l_min seed bound min_occupancy"),
    "basin_params": ("SarBasinParams", BASIN, "origin du dv width height transient steps bound grid"),
    "density_params": ("SarDensityParams", {}, "samples"),
    "shade_params": ("SarShadeParams", {}, "light ambient diffuse specular ao_strength ao_range smooth_range shininess_log2 ao_radius smooth "
                                           "min_count background"),
    "exposure_params": ("SarExposureParams", {}, "q_black q_white level_black level_white"),
    "color_range_params": ("SarColorRangeParams", {}, "q_lo q_hi pos_lo pos_hi"),
}
WINDOW = {"$color_range": dict(lo=0.25, hi=0.75, pos_lo=0.125, pos_hi=0.875, covered=9, applied=True)}
# builder -> (label, arguments on top of the builder's own, reason if the row is marked for tightening)
EXTRA = {
    "plane_params": [("mode=spectrum", dict(mode="spectrum"), None), ("mode=l1", dict(mode="l1"), None), ("mode=nope", dict(mode="nope"), None),
                     ("axes lowest", dict(axes=[0, 0]), None), ("axes highest", dict(axes=[2 ** 32 - 1, 29]), None),
                     ("axes above", dict(axes=[2 ** 32, 0]), None), ("axes below", dict(axes=[0, -1]), None),
                     ("axes integral floats", dict(axes=[2.0, 9.0]), None), ("axes non-integral", dict(axes=[1.5, 2]), NON_INTEGRAL),
                     ("axes too many", dict(axes=[1, 2, 3]), None), ("axes too few", dict(axes=[1]), None),
                     ("x_range too many", dict(x_range=[0.0, 1.0, 2.0]), None), ("y_range too few", dict(y_range=[0.0]), None),
                     ("base (3, 10)", dict(base=[OTHER[:10], OTHER[10:20], OTHER[20:]]), None), ("base a Config", dict(base={"$config": "solar_sail"}), None),
                     ("base too short", dict(base=COEFFS[:29]), None), ("axis by keyword", dict(axis=[1, 2]), None),
                     ("lo by keyword", dict(lo=[0.0, 0.0]), None)],
    "period_params": [("the plane", dict(base=OTHER, axes=[29, 0], x_range=[-0.5, 0.25], y_range=[0.125, 0.75]), None),
                      ("x_range alone", dict(x_range=[-2.0, 2.0]), None), ("base a Config", dict(base={"$config": "poisson_saturne"}), None),
                      ("axes highest", dict(axes=[2 ** 32 - 1, 0]), None), ("axes above", dict(axes=[0, 2 ** 32]), None),
                      ("axes below", dict(axes=[-1, 0]), None), ("axes non-integral", dict(axes=[1.5, 2]), NON_INTEGRAL),
                      ("axes too many", dict(axes=[1, 2, 3]), None), ("base too long", dict(base=COEFFS + [0.0]), None),
                      ("steps by keyword", dict(steps=5), None), ("axis by keyword", dict(axis=[1, 2]), None), ("hi by keyword", dict(hi=[1.0, 1.0]), None)],
    "orbit_params": [("b", dict(b=OTHER, axis=None, range=None), None), ("b and axis", dict(b=OTHER), None), ("a a Config", dict(a={"$config": "solar_sail"}), None),
                     ("v_range", dict(v_range=[-0.75, 1.5]), None), ("axis lowest", dict(axis=0), None), ("axis highest", dict(axis=29), None),
                     ("axis above", dict(axis=30), None), ("axis below", dict(axis=-1), None), ("axis without range", dict(range=None), None),
                     ("one end only", dict(axis=None, range=None), None), ("a too short", dict(a=COEFFS[:29]), None),
                     ("v_lo by keyword", dict(v_lo=1.0), None), ("b (3, 10)", dict(b=[OTHER[:10], OTHER[10:20], OTHER[20:]]), None)],
    "basin_params": [("box", dict(box=[[-1.0, -2.0, -3.0], [1.5, 2.5, 3.5]]), None), ("box too few", dict(box=[[-1.0, -2.0], [1.5, 2.5]]), None),
                     ("coeffs a Config", dict(coeffs={"$config": "poisson_saturne"}), None),
                     ("coeffs a search record", dict(coeffs={"$search_record": 12}, search_seed=3, search_lo=-1.0, search_hi=1.0), None),
                     ("coeffs too short", dict(coeffs=COEFFS[:29]), None), ("box_lo by keyword", dict(box_lo=[0.0, 0.0, 0.0]), None)],
    "box_params": [("origin None", dict(origin=None), None)],
    "corrdim_params": [("width by keyword", dict(width=5), None)],
    "shade_params": [("window", dict(window=WINDOW), None), ("window None", dict(window=None), None), ("has_window by keyword", dict(has_window=1), None),
                     ("_pad1", dict(_pad1=0), None)],
}


def _range(ctype):
    bits = 8 * C.sizeof(ctype)
    return (-2 ** (bits - 1), 2 ** (bits - 1) - 1) if ctype(-1).value < 0 else (0, 2 ** bits - 1)


def _is_int(ctype):
    return ctype in (C.c_uint16, C.c_uint32, C.c_uint64, C.c_int32)


def _field_rows(builder, field, ctype):
    """(label, arguments, reason if marked for tightening) for one settable field, from its ctype"""
    shade = SHADE_RANGE if builder == "shade_params" and field in ("smooth", "background") else None
    if issubclass(ctype, C.Array):
        n, elem = ctype._length_, ctype._type_
        if _is_int(elem):
            lo, hi = _range(elem)
            rows = [("set", [k + 1 for k in range(n)], None), ("integral floats", [5.0 + k for k in range(n)], None), ("lowest", [lo] * n, None),
                    ("highest", [hi] * n, None), ("below", [lo - 1] + [0] * (n - 1), shade), ("above", [0] * (n - 1) + [hi + 1], shade),
                    ("non-integral", [1.5] + [0] * (n - 1), NON_INTEGRAL)]
        else:
            rows = [("set", [0.125 * (k + 1) for k in range(n)], None), ("integers", [k - 1 for k in range(n)], None)]
        rows += [("too few", rows[0][1][:-1], None), ("too many", rows[0][1] + rows[0][1][:1], None)]
    elif _is_int(ctype):
        lo, hi = _range(ctype)
        rows = [("set", 7, None), ("integral float", 2e5 if hi > 2e5 else 5.0, None), ("lowest", lo, None), ("highest", hi, None),
                ("below", lo - 1, shade), ("above", hi + 1, shade), ("non-integral", 1.5, NON_INTEGRAL)]
    else:
        rows = [("set", 0.375, None), ("an integer", 3, None)]
    return [(f"{field} {label}", {field: value}, reason) for label, value, reason in rows]


def table(abi):
    """every row as (builder, label, arguments, reason if marked for tightening)"""
    out = []
    for builder, (struct, base, fields) in BUILDERS.items():
        types = dict(getattr(abi, struct)._fields_)
        rows = [("defaults", {}, None)]
        for field in fields.split():
            rows += _field_rows(builder, field, types[field])
        rows += EXTRA.get(builder, [])
        pad = next((f for f in types if f.startswith("_")), "_pad")
        rows += [("an unknown key", dict(no_such_field=1), None), ("a padding key", {pad: 0}, None)]
        out += [(builder, label, {**base, **kw}, reason) for label, kw, reason in rows]
    assert len({(b, label) for b, label, _, _ in out}) == len(out)
    return out


def decode(sar, value):
    """the argument a row's JSON value stands for"""
    if isinstance(value, list):
        return [decode(sar, v) for v in value]
    if isinstance(value, dict):
        (kind, arg), = value.items()
        if kind == "$config":
            return getattr(sar.Config, arg)()
        if kind == "$color_range":
            return sar.ColorRange(**arg)
        if kind == "$search_record":
            rec = np.zeros(1, dtype=sar.SEARCH_RECORD_DTYPE)
            rec["candidate"] = arg
            return rec
        raise ValueError(kind)
    return value


def outcome(sar, builder, kwargs):
    """{"bytes": hex} or {"raises": class name} of one call"""
    try:
        p = getattr(sar, builder)(**{k: decode(sar, v) for k, v in kwargs.items()})
    except Exception as e:   # noqa: BLE001 (the class is what the row records)
        return {"raises": type(e).__name__}
    return {"bytes": bytes(p).hex()}


# the public dtype -> the _abi structure it mirrors
DTYPES = {
    "SEARCH_RECORD_DTYPE": "SarSearchRecord", "GALLERY_ITEM_DTYPE": "SarGalleryItem", "GALLERY_STATS_DTYPE": "SarGalleryStats",
    "PLANE_RECORD_DTYPE": "SarPlaneRecord", "PERIOD_RECORD_DTYPE": "SarPeriodRecord", "ORBIT_COLUMN_DTYPE": "SarOrbitColumn",
    "CORRDIM_LINE_DTYPE": "SarCorrdimLine", "CORRDIM_RECORD_DTYPE": "SarCorrdimRecord", "PAIRS_COUNTS_DTYPE": "SarPairsCounts",
    "BOX_LEVEL_DTYPE": "SarBoxLevel", "BOXDIM_LINE_DTYPE": "SarBoxdimLine", "BOXDIM_LINES_DTYPE": "SarBoxdimLines",
    "BOXDIM_RECORD_DTYPE": "SarBoxdimRecord", "BASIN_PIXEL_DTYPE": "SarBasinPixel", "BASIN_ATTRACTOR_DTYPE": "SarBasinAttractor",
}


def dtype_literal(dt):
    """a structured dtype as JSON: [name, format or nested literal, shape, offset] per field, and the item size"""
    fields = []
    for name in dt.names:
        sub, offset = dt.fields[name][:2]
        base, shape = sub.subdtype if sub.subdtype else (sub, ())
        fields.append([name, dtype_literal(base) if base.names else base.str, list(shape), offset])
    return {"fields": fields, "itemsize": dt.itemsize}


def dtype_of(literal):
    """the dtype a literal of dtype_literal describes"""
    names, formats, offsets = [], [], []
    for name, fmt, shape, offset in literal["fields"]:
        names.append(name)
        formats.append((dtype_of(fmt) if isinstance(fmt, dict) else np.dtype(fmt), tuple(shape)))
        offsets.append(offset)
    return np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": literal["itemsize"]})


def main():
    sys.path.insert(0, ROOT)
    import strange_attractor_renderer_amd as sar
    from strange_attractor_renderer_amd import _abi
    sar.load_library()
    rows, tightened = [], []
    for builder, label, kwargs, reason in table(_abi):
        got = outcome(sar, builder, kwargs)
        row = {"builder": builder, "label": label, "kwargs": kwargs}
        if reason is not None and got != {"raises": "ValueError"}:
            tightened.append({**row, "raises": "ValueError", "reason": reason, "recorded": got})
        else:
            rows.append({**row, **got})
    assert all(t["builder"] == "shade_params" for t in tightened if t["reason"] == SHADE_RANGE)
    dtypes = {name: {"abi": struct, **dtype_literal(getattr(sar, name))} for name, struct in DTYPES.items()}
    with open(GOLDEN, "w") as f:
        f.write('{"rows": [\n' + ",\n".join(json.dumps(r) for r in rows) + '\n],\n"tightened": [\n')
        f.write(",\n".join(json.dumps(t) for t in tightened) + '\n],\n"dtypes": {\n')
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in dtypes.items()) + "\n}}\n")
    print(f"{len(rows)} rows, {len(tightened)} tightened, {len(dtypes)} dtypes recorded")


if __name__ == "__main__":
    main()
