"""MI355X-native iterate/accumulate path of Icelk/strange-attractor-renderer.

`libsar_hip.so` (HIP, gfx950) is the product; this package is the thin host-side mirror of the
reference crate's Config / Runtime / render / colorize / ParallelRenderer / render_parallel surface
over the C ABI declared in include/sar.h. No CPU fallback exists by design.
"""
from .api import (Config, Exchange, ParallelRenderer, Runtime, SarError, Timing, attractor_extent, colorize,  # noqa: F401
                  colorize_device, colorize_device_batch, reset_batch, colorize_range_device, exchange_slice_pixels, bin_geometry,
                  colorize_format, colorize_format_async, colorize_format_device, read_image_async, image_done, wait_image, HostImage, host_reserve, image_bytes, convert_device, device_count, image_format, render, render_job_range, render_job_range_device, prefetch_device, render_jobs, render_jobs_batch, batch_frames, render_parallel_into,
                  render_parallel, start_points, write_image, write_image_matches,
                  SEARCH_RECORD_DTYPE, frame_view, search_attractors, search_candidate, search_params,
                  Exposure, auto_exposure, exposure, exposure_params,
                  density_filter, density_params, density_radius, density_weights,
                  shade, shade_device, shade_params,
                  VOLUME_ABOVE, VOLUME_BELOW, VOLUME_NAN, Volume, volume, volume_learned_range, volume_march_params, volume_params, volume_slab,
                  FLOW_SYSTEMS, flow_coefficients, flow_extent, flow_params, flow_step, flow_view, render_flow,
                  SECTION_RECORD_DTYPE, FlowSection, flow_section, section_extremum, section_params, section_plane, section_step,
                  ColorRange, auto_color, color_range, color_range_params, color_range_to_velocity,
                  PLANE_RECORD_DTYPE, LyapunovPlane, lyapunov_plane, plane_colors, plane_params,
                  PERIOD_RECORD_DTYPE, PeriodPlane, period_colors, period_params, period_plane,
                  CYCLES_RECORD_DTYPE, CYCLE_ORBIT_DTYPE, CYCLE_KINDS, Cycles, cycle_charpoly, cycles, cycles_params, cycles_starts,
                  MANIFOLD_BRANCH_DTYPE, MANIFOLD_RECORD_DTYPE, MANIFOLD_NONE, MANIFOLD_COLOURS, Manifolds, manifold_branches, manifold_params,
                  manifold_pixel, manifolds,
                  GALLERY_ITEM_DTYPE, GALLERY_STATS_DTYPE, Gallery, frame_view_box, gallery, gallery_atlas_shape, gallery_items, gallery_params,
                  ORBIT_COLUMN_DTYPE, OrbitDiagram, orbit_diagram, orbit_params,
                  CORRDIM_LINE_DTYPE, CORRDIM_RECORD_DTYPE, PAIRS_COUNTS_DTYPE, CorrelationDimension, correlation_dimension, corrdim_fit,
                  corrdim_params, pair_edges, pair_histogram, pairs_params,
                  BOX_LEVEL_DTYPE, BOXDIM_LINE_DTYPE, BOXDIM_LINES_DTYPE, BOXDIM_RECORD_DTYPE, BoxDimension, box_counts, box_dimension, box_fit,
                  box_log2_q32, box_params, boxdim_params,
                  BASIN_ATTRACTOR_DTYPE, BASIN_NONE, BASIN_PIXEL_DTYPE, BasinMap, basin_map, basin_params,
                  BASIN_FATE_DTYPE, BASIN_LADDER_MASK_DTYPE, BASIN_LEVEL_DTYPE, BASIN_UNKNOWN, BasinStability, BasinUncertainty,
                  BasinUncertaintyFit, basin_fates, basin_ladder_params, basin_uncertainty,
                  FTLE_PIXEL_DTYPE, FtleMap, ftle_map, ftle_params,
                  SPECTRA_RECORD_DTYPE, SPECTRUM_RECORD_DTYPE, SPECTRUM_WINDOWS, Spectrum, power_spectra, power_spectrum, spectra_params,
                  spectra_segments, spectrum_params, spectrum_twiddles, spectrum_window,
                  RECURRENCE_RECORD_DTYPE, RQA_MEASURES_DTYPE, RQA_RECORD_DTYPE, Recurrence, recurrence_analysis, recurrence_lines,
                  recurrence_params, recurrence_plot, rqa_measures, rqa_params)
from ._abi import (SAR_CT_ADJUSTED_VELOCITY, SAR_CT_POISSON_SATURNE, SAR_FMT_RGB8, SAR_FMT_RGB16,  # noqa: F401
                   SAR_FMT_RGBA8, SAR_FMT_RGBA16, SAR_RENDER_DEPTH, SAR_RENDER_GAS, SAR_SEARCH_BOUNDED, SAR_SEARCH_DEGENERATE,
                   SAR_SEARCH_DIVERGED, SAR_PLANE_L1, SAR_PLANE_SPECTRUM, SAR_CORRDIM_FIT_OK, SAR_CORRDIM_NO_WINDOW, SAR_BOXDIM_FIT_OK,
                   SAR_BOXDIM_NO_WINDOW, SAR_CYCLE_CONVERGED, SAR_CYCLE_ESCAPED, SAR_CYCLE_SINGULAR, SAR_CYCLE_NOT_CONVERGED, SAR_MANIFOLD_OK,
                   SAR_MANIFOLD_DOMAIN_ESCAPED, SAR_SECTION_FULL, SAR_SECTION_SHORT, SAR_SECTION_ESCAPED,
                   SAR_SECTION_ESCAPED_TRANSIENT, SAR_SECTION_NO_CLOCK, SAR_FTLE_EDGE, SAR_FTLE_ONE_SIDED_U, SAR_FTLE_ONE_SIDED_V, SAR_FTLE_NO_U, SAR_FTLE_NO_V,
                   SAR_WINDOW_RECT, SAR_WINDOW_HANN, SAR_BASIN_UNKNOWN, SAR_BASIN_MAX_LEVELS,
                   load_library,
                   use_hooks_build)

RenderKind = type("RenderKind", (), {"Gas": SAR_RENDER_GAS, "Depth": SAR_RENDER_DEPTH})
