"""Builds libsar_hip.so (the HIP library behind include/sar.h) in-tree with hipcc for gfx950.

    python -m strange_attractor_renderer_amd.build [--force]

The build also audits the device code: the iterate kernel must not contain a fused multiply-add
(v_fma_f64 / v_fmac_f64) — a single contraction changes the chaotic trajectories and breaks parity
with the reference (which Rust/LLVM never contracts).
"""
from __future__ import annotations

import hashlib
import os
import re
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
OUT = os.path.join(PKG, "libsar_hip.so")
BUILD_DIR = os.path.join(os.path.dirname(PKG), "build", "sar_hip")
VARIANT_DIR = os.path.join(os.path.dirname(PKG), "build", "variants")   # A/B and test builds (SAR_LIBRARY=...), git-ignored
HOOKS_OUT = os.path.join(os.path.dirname(PKG), "tests", "hooks", "libsar_hip_hooks.so")   # product objects + sar_test_hooks.cpp
HOOKS_SOURCE = "sar_test_hooks.cpp"
SOURCES = ["sar_host.cpp", "sar_export.cpp", "sar_plan.cpp", "sar_render.cpp", "sar_runtime.cpp", "sar_colorize.cpp", "sar_hostmem.cpp", "sar_batch.cpp", "sar_exchange.cpp", "sar_multi.cpp", "sar_search.cpp",
           "sar_plane.cpp", "sar_gallery.cpp", "sar_orbit.cpp", "sar_corr.cpp", "sar_box.cpp", "sar_spectrum.cpp", "sar_rqa.cpp", "sar_basin.cpp", "sar_fate.cpp", "sar_ftle.cpp", "sar_period.cpp", "sar_density.cpp", "sar_shade.cpp", "sar_cycles.cpp", "sar_manifold.cpp", "sar_volume.cpp", "sar_flow.cpp", "sar_section.cpp", "sar_analysis.cpp", "sar_iterate.hip", "sar_accumulate.hip", "sar_image.hip", "sar_select.hip", "sar_search.hip", "sar_plane.hip", "sar_gallery.hip", "sar_orbit.hip", "sar_corr.hip", "sar_box.hip", "sar_spectrum.hip", "sar_rqa.hip", "sar_basin.hip", "sar_fate.hip", "sar_ftle.hip", "sar_period.hip", "sar_density.hip", "sar_shade.hip", "sar_cycles.hip", "sar_manifold.hip", "sar_volume.hip", "sar_flow.hip", "sar_section.hip"]
HEADERS = [HOOKS_SOURCE, os.path.join("..", "..", "include", "sar_test_hooks.h"), "sar_internal.hpp", "sar_launch.hpp", "sar_device.hpp", "sar_runtime_impl.hpp", "sar_analysis.hpp", "sar_plan.hpp", "sar_search.hpp", "sar_gallery.hpp", "sar_orbit.hpp", "sar_corr.hpp", "sar_box.hpp", "sar_spectrum.hpp", "sar_rqa.hpp", "sar_basin.hpp", "sar_fate.hpp", "sar_ftle.hpp", "sar_period.hpp", "sar_density.hpp", "sar_shade.hpp", "sar_cycles.hpp", "sar_manifold.hpp", "sar_volume.hpp", "sar_flow.hpp", "sar_section.hpp", "sar_tangent.hpp", os.path.join("..", "..", "include", "sar.h")]
ARCH = "gfx950"
# Fused fp64 ops (v_fma_f64 + v_fmac_f64_e32, as ROCm 7.2's device libs emit them) every kernel outside the iterate family must hold:
# kernel-name pattern -> (kernels the pattern matches, ops in each). What is fused is the correctly-rounded expansion of a square root
# (7), a division (5) or a logarithm (14), nothing else: one more means a multiply-add beside it was contracted, one fewer that the
# device libs changed.
FUSED_OPS = {
    # k_depth_resolve of the binned path, k_fold_resolve of the one-atomic-per-visit path and the fold of a batched launch, one body:
    # the replay of next_point / screen_space from the checkpoints for the bit-exact `steps` payload fuses nothing; the sqrt and the
    # division of color_transform beside it do
    r"k_fold_resolve|k_depth_resolve": (3, 7 + 5),
    # the search: the map alone; the map, the Jacobian and V = J Q uncontracted next to Gram-Schmidt's three norms and three reciprocals
    r"k_search_screen": (1, 0),
    r"k_search_lyapunov": (1, 3 * 7 + 3 * 5),
    # k_plane<K> (the Lyapunov planes): K sqrt + K div of Gram-Schmidt, plus the two divisions of the swept values (plane_sweep)
    r"^_ZN3sar7k_planeILi1E": (1, 12 + 10),
    r"^_ZN3sar7k_planeILi3E": (1, 36 + 10),
    # k_gallery: warm-up and both traversals advance the map uncontracted; color_transform at a pixel's winner (sqrt + div, as
    # k_fold_resolve) and the Gas colorize of the tile — three sqrt, the division of the two logarithms and ln_u32's device log beyond
    # the table, inlined twice
    r"k_gallery": (1, 12 + 21 + 5 + 2 * 14),
    # k_orbit (the orbit diagrams): the map, the plotted value v and the bin coordinate u are multiplies and adds; no division, square
    # root or logarithm
    r"k_orbit": (1, 0),
    # k_corr_orbit / k_corr_pairs (the correlation dimension): the map and r^2 = (dx dx + dy dy) + dz dz are multiplies and adds, the
    # bin comes from the bits of r^2
    r"k_corr_orbit": (1, 0),
    r"k_corr_pairs": (1, 0),
    # k_box_insert / k_box_level (box counting): a cell is one subtract, one multiply and a conversion, the logarithm of an occupancy
    # is integer arithmetic
    r"k_box_insert": (1, 0),
    r"k_box_level": (1, 0),
    # k_spectrum<1 | 2 | 4 | 8> / k_spectrum_fold (the power spectra): the plotted value, the pairwise sums, the taper, the butterflies
    # tr = W.re b.re - W.im b.im, ti = W.re b.im + W.im b.re, u + t, u - t, and re re + im im are multiplies, adds and subtractions;
    # 1 / N, the twiddles and the window are the host's. 0 proves that no butterfly was contracted
    r"k_spectrumILj": (4, 0),
    r"k_spectrum_fold": (1, 0),
    # k_rqa_diag / k_rqa_vert / k_rqa_plot (the recurrence analysis): r^2 = (dx dx + dy dy) + dz dz as k_corr_pairs', a compare with
    # eps2 and integer run lengths; eps2 itself is the host's
    r"k_rqa_diag": (1, 0),
    r"k_rqa_vert": (1, 0),
    r"k_rqa_plot": (1, 0),
    # the basins of attraction: the map, the start point (its two divisions are the host's, one per column and per row) and the node
    # are multiplies, adds and compares; k_basin_colorize holds the one division that serves both kinds of pixel and the three square
    # roots of the palette blend
    r"k_basin_screen": (1, 0),
    r"k_basin_mark": (1, 0),
    r"k_basin_finish": (1, 0),
    r"k_basin_colorize": (1, 5 + 21),
    # k_basin_fate / k_basin_ladder (the basin probes): the map and the node as k_basin_screen's, a ladder's probe point one multiply
    # and one add or subtract; the table look-up, the classes and the counts are integers
    r"k_basin_fate": (1, 0),
    r"k_basin_ladder": (1, 0),
    # the FTLE maps: the map and the start point as the basins'; the differences between neighbouring end points and their Gram
    # entries are subtractions, multiplies, adds and compares (stretch2's division and square root are the host's). k_ftle_colorize
    # holds the logarithm of stretch2, the division by 2 N, the one division that serves both kinds of pixel and the three square
    # roots of the palette blend
    r"k_ftle_flow": (1, 0),
    r"k_ftle_gram": (1, 0),
    r"k_ftle_colorize": (1, 14 + 5 + 5 + 21),
    # k_period<LIST> (the period planes): the map, the differences and the compares fuse nothing; the sweep form holds the two
    # divisions of the swept values (plane_sweep), the list form none. k_period_colorize: one division and the blend's three square roots
    r"k_periodILb0E": (1, 10),
    r"k_periodILb1E": (1, 0),
    r"k_period_colorize": (1, 5 + 21),
    # k_density (density estimation): the hue sum is multiplies and adds, the counts and the statistics are integers; the one division
    # num / den
    r"k_density": (1, 5),
    # k_shade (shaded rendering): six divisions — the mean of the smoothing window, the normal's three components over its length,
    # occ / N and the window's (steps - lo) / span — and four square roots — the normal's length and the palette blend's three. The
    # smoothing sum, the two light sums, the occlusion sum and the pixel's r * lum + glint are multiplies and adds
    r"k_shade": (1, 6 * 5 + 4 * 7),
    # the cycles: the map, the Jacobian products, the adjugate and the determinant are multiplies, adds and subtractions; the Newton
    # step's three divisions n_i / det. k_cycles_merge has no multiply at all
    r"k_cycles_newton": (1, 3 * 5),
    r"k_cycles_merge": (1, 0),
    # k_manifold (the unstable manifolds): the sample's a + d * t, the map, the bound test and the projection are multiplies, adds and
    # compares, the raster is integers; the one division t_i = i / (S - 1)
    r"k_manifold": (1, 5),
    # volume rendering: the warm-up and the accumulate run render's step and the slab's subtract and multiply (dscale is the host's),
    # the reduction and the section are integers. k_volume_march: five divisions — (k + 0.5) / D of a slab's palette position,
    # nd / (nd + half) of a voxel's opacity and the three channels over 1 - T of a transparent image — and the blend's three square
    # roots; w * r_k and T * bg next to their adds are multiplies and adds
    r"k_volume_warm": (1, 0),
    r"k_volume_accumulate": (1, 0),
    r"k_volume_reduce": (1, 0),
    r"k_volume_section": (1, 0),
    r"k_volume_march": (1, 5 * 5 + 3 * 7),
    # flows: the RK4 step is four evaluations of render's polynomial and p + h2 * k, p + h6 * (...) as multiplies and adds (h * 0.5 and
    # h / 6.0 are the host's), the bound test compares; k_flow_resolve compares two f32 depths and converts the hue. k_flow_render adds the
    # colour transform of a visit that may win its pixel: the square root of |d| and the poisson-saturne transform's division by 0.9
    # (its division by 2 is an exact multiply by 0.5), as k_fold_resolve holds them
    r"k_flow_transient": (1, 0),
    r"k_flow_render": (1, 7 + 5),
    r"k_flow_resolve": (1, 0),
    # the Poincare sections: k_flow_section's loop is the flow step plus one row g of the same polynomial form and compares; behind the
    # crossing branch Henon's step holds five divisions (D / 6.0 and the four rates 1.0 / gdot) and the rough path a sixth
    # (g0 / (g0 - g1)), the gradient, gdot, P * w and the RK4 sums beside them multiplies and adds: 6 x 5, which is what gfx950's
    # assembly holds (six v_div_fmas_f64, six v_div_fixup_f64). k_section_plot projects, converts a return time to f32 and makes two atomics
    r"k_flow_section": (1, 6 * 5),
    r"k_section_plot": (1, 0),
}

FLAGS = [
    f"--offload-arch={ARCH}", "-O3", "-std=c++17",
    "-ffp-contract=off",          # mandatory for bit parity (host AND device)
    "-fno-fast-math",
    "-fPIC", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-value",
]


def _hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found")


def _extra_flags() -> list[str]:
    return os.environ.get("SAR_EXTRA_FLAGS", "").split() + os.environ.get("SAR_KERNEL_FLAGS", "").split()


def source_id(csrc: str | None = None, extra_flags: list[str] | None = None) -> str:
    """What a library is built FROM, as 16 hex digits: SHA-256 over every source and header of the library (csrc/*, include/sar.h;
    names and contents) and the compiler flags. The build embeds it (sar_build_id()); the loader recomputes it from the tree and
    refuses a binary built from other sources (_abi.load_library)."""
    csrc = csrc or CSRC
    h = hashlib.sha256()
    for name in sorted(SOURCES + HEADERS, key=os.path.basename):
        h.update(os.path.basename(name).encode() + b"\0")
        h.update(open(os.path.join(csrc, name), "rb").read())
        h.update(b"\0")
    h.update(" ".join(FLAGS + (extra_flags if extra_flags is not None else _extra_flags())).encode())
    return h.hexdigest()[:16]


def library_id(path: str) -> str | None:
    """The id embedded in a built library file (without loading it), or None."""
    try:
        data = open(path, "rb").read()
    except OSError:
        return None
    m = re.search(rb"SAR_BUILD_ID=([0-9a-f]{16})", data)
    return m.group(1).decode() if m else None


def _stale() -> bool:
    return library_id(OUT) != source_id() or library_id(HOOKS_OUT) != source_id()


def audit_no_fma(asm_paths) -> dict:
    """Counts fused fp64 ops per kernel in the device assembly; the kernels that run the map must have none."""
    text = "\n".join(open(p).read() for p in asm_paths)
    counts = {}
    # kernels are delimited by "<name>:" labels ... ".end_amdhsa_kernel"/"s_endpgm"
    # each function body runs from its "<name>:" label to the matching ".Lfunc_end<N>:" label
    for m in re.finditer(r"^(_ZN3sar\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, flags=re.S | re.M):
        name, body = m.group(1), m.group(2)
        counts[name] = len(re.findall(r"\bv_(fma|fmac|mad)_f64(?:_e32|_e64|_dpp)?\b", body))   # VOP3 and VOP2 (_e32) encodings
    bad = {k: v for k, v in counts.items() if any(t in k for t in ("k_iterate", "k_extent", "k_warmup", "k_search_screen")) and v}
    if bad:
        raise RuntimeError(f"fused fp64 ops found in the iterate kernel: {bad}")
    if not any("k_iterate" in k for k in counts):
        raise RuntimeError("audit could not find k_iterate in the device assembly")
    for pattern, (kernels, want) in FUSED_OPS.items():
        got = [v for k, v in counts.items() if re.search(pattern, k)]
        if got != [want] * kernels:
            raise RuntimeError(f"the {kernels} kernel(s) matching {pattern!r} hold {got} fused fp64 ops, expected [{want}] each (sqrt / div / log "
                               "expansions only): either arithmetic beside them was contracted or the device libs changed — inspect the assembly")
    return counts


LAST_BUILD = {"action": None, "id": None}   # what the last build_library() call did: "built" / "reused" and the id


def build_library(force: bool = False, verbose: bool = False, out: str | None = None, build_dir: str | None = None) -> str:
    """out / build_dir: build a VARIANT of the library somewhere else (with SAR_EXTRA_FLAGS / SAR_KERNEL_FLAGS set) for
    A/B timing or test builds; load it through the SAR_LIBRARY environment variable. The product is the default: it is
    rebuilt whenever the id embedded in the binary is not the id of the sources (contents, not mtimes)."""
    sid = source_id()
    if out is None and not force and not _stale():
        LAST_BUILD.update(action="reused", id=sid)
        return OUT
    OUT_ = out or OUT
    BUILD_DIR_ = build_dir or BUILD_DIR
    os.makedirs(BUILD_DIR_, exist_ok=True)
    hipcc = _hipcc()
    objs = []
    for s in SOURCES:
        obj = os.path.join(BUILD_DIR_, s + ".o")
        # SAR_EXTRA_FLAGS: extra -D flags for timing experiments (e.g. -DSAR_EXPERIMENT_...); never set by the product
        cmd = [hipcc, *FLAGS, *os.environ.get("SAR_EXTRA_FLAGS", "").split(), f'-DSAR_BUILD_ID="{sid}"', "-c", os.path.join(CSRC, s), "-o", obj]
        if s.endswith(".hip"):  # SAR_KERNEL_FLAGS: device-compiler flags for experiments (e.g. -mllvm options)
            cmd += ["-save-temps=obj", *os.environ.get("SAR_KERNEL_FLAGS", "").split()]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True, cwd=BUILD_DIR_)
        objs.append(obj)
    asm = [os.path.join(BUILD_DIR_, f"{s[:-4]}-hip-amdgcn-amd-amdhsa-{ARCH}.s") for s in SOURCES if s.endswith(".hip")]
    counts = audit_no_fma(asm)
    if verbose:
        print("fused-fp64 audit:", {k[:60]: v for k, v in counts.items()})
    tmp = OUT_ + ".tmp"
    subprocess.run([hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", *objs, "-lz", "-lpthread", "-o", tmp], check=True)  # zlib: PNG export
    os.replace(tmp, OUT_)
    # the hooks build of the test-suite: the SAME object files plus the one that defines sar_runtime_set_test_option
    hooks_out = HOOKS_OUT if out is None else OUT_[:-3] + "_hooks.so"
    os.makedirs(os.path.dirname(hooks_out), exist_ok=True)
    hobj = os.path.join(BUILD_DIR_, HOOKS_SOURCE + ".o")
    subprocess.run([hipcc, *FLAGS, *os.environ.get("SAR_EXTRA_FLAGS", "").split(), "-c", os.path.join(CSRC, HOOKS_SOURCE), "-o", hobj], check=True, cwd=BUILD_DIR_)
    subprocess.run([hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", *objs, hobj, "-lz", "-lpthread", "-o", hooks_out + ".tmp"], check=True)
    os.replace(hooks_out + ".tmp", hooks_out)
    LAST_BUILD.update(action="built", id=sid)
    return OUT_


if __name__ == "__main__":
    if "--variant" in sys.argv:  # python -m ...build --variant NAME  (flags from SAR_EXTRA_FLAGS / SAR_KERNEL_FLAGS)
        name = sys.argv[sys.argv.index("--variant") + 1]
        import tempfile
        scratch = os.environ.get("SAR_VARIANT_BUILD_DIR") or os.path.join(tempfile.gettempdir(), "sar_build")
        os.makedirs(VARIANT_DIR, exist_ok=True)   # variants never sit next to the product
        print(build_library(force=True, verbose=True, out=os.path.join(VARIANT_DIR, f"libsar_hip_{name}.so"),
                            build_dir=os.path.join(scratch, f"sar_hip_{name}")))
    else:
        print(build_library(force="--force" in sys.argv, verbose=True))
        print(f"{LAST_BUILD['action']} {LAST_BUILD['id']}")
