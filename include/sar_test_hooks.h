/*
 * sar_test_hooks.h — the A/B and test options of a runtime. NOT part of the product's ABI (include/sar.h): the function below is
 * defined in csrc/sar_test_hooks.cpp, which is linked only into the hooks build (tests/hooks/libsar_hip_hooks.so = the object
 * files of libsar_hip.so + that one file; strange_attractor_renderer_amd/build.py makes both). The test-suite, tools/ and the
 * A/B switches of bench.py load the hooks build; __graft_entry__.smoke() and bench.py's measurements load the product.
 */
#ifndef SAR_TEST_HOOKS_H
#define SAR_TEST_HOOKS_H

#include "sar.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Options by name (value 0 restores the default unless noted):
 *   "path"               accumulate path: 0 default (= 3 when the image fits, up to 64 Mpx), 1 one global atomic per
 *                        visit, 3 LDS-binned records (an error where they do not fit)
 *   "bin_shift"          log2(pixels per bin) of the binned path (12..16; 16: the accumulate kernel packs two 16-bit counters
 *                        with a guard bit into an LDS word)
 *   "bin_interleave"     which pixels form a bin: 1 consecutive pixels, 2 every B-th 2048-pixel segment of the image
 *                        (B bins, a power of two: every bin carries the same share of the visits whatever the attractor
 *                        covers); 0 = 2 when the power-of-two bin count costs at most a third more bins, else 1
 *   "splits"             workgroups per bin in the record-accumulate kernel (1..16)
 *   "chunk_records"      u16 records per chunk: 12, 20, 28 or 60 (32/48/64/128-byte chunks; fewer = less LDS per wave)
 *   "hint_shared"        1: one array of depth hints per XCD, 2: one array for the whole chip (each XCD's L2 then sees the
 *                        others' updates late — more visits pass the filter, none wrongly); 0 = per XCD unless the eight
 *                        copies exceed 200 MB (then they would not fit the Infinity Cache)
 *   "hint_tile"          1: 16-bit hints always in row-major order; 0 = in 8 x 8 tiles (one 128-byte line each) where the
 *                        image width is a power of two and the height a multiple of eight
 *   "depth_park"         the park window of k_iterate_split's consumer wave for the next launches: a visit that passes its depth hint
 *                        waits in its lane's registers and the wave runs stage 2 (key load, compare, atomic, hint store) every
 *                        2, 4 or 8 steps; 0 = in every step. Same result bit for bit; k_iterate_lean and batched launches have no
 *                        window (describe_last_launch says park=0 for them). Unset: the product's default (8)
 *   "chunk_ahead"        a render call of several launch chunks runs its next chunk's warm-up ahead, under the current chunk's
 *                        accumulate and fold (0 / 1, the default); 2 = not (A/B)
 *   "acc_threads"        threads per block of the record-accumulate kernel (256, 512, 1024)
 *   "acc_lists"          (bin, wave) record lists a lane group of that kernel walks at the same time: 1 or 4
 *   "corr_replicas"      copies of k_corr_pairs' LDS histogram: 1, 2, 4, 8, 16 or 32; 0 = as many as the LDS budget holds (A/B: the
 *                        counts do not depend on it)
 *   "debug_chunk_jobs"   test hook: cap on jobs per launch chunk
 *   "debug_throw"        test hook (rt may be NULL): 1 / 2 / 3 throw std::bad_alloc / std::runtime_error / an int inside the entry point —
 *                        the call returns SAR_ERR_OOM / SAR_ERR_INVALID with the text in sar_last_error(): nothing unwinds across the ABI
 *   "debug_max_ordinals" test hook: visits one launch may order (default 2^32-2); jobs with more iterations run as segments
 *
 *   "readback_inline"    1: the read-back of sar_colorize_format_async stays on the launch stream (A/B of the copy stream)
 *   "batch_starts"       how a batched launch gets its start points: 0 = read in place by the one-phase warm-up / fetched by a
 *                        kernel before a two-phase one, 1 = copied on an upload stream, 2 = on the launch stream, 3 = always in place
 *   "batch_warm"         the warm-up of a batched launch: 0 = two phases when the last launch lost a tenth of its jobs, 1 = one, 2 = two
 *   "batch_chain"        1: the iterate kernels of a device's batches are not chained one behind the other
 *   "batch_xcd"          1: the frames of a batch are not dealt to the XCDs (every frame runs on all eight)
 */
int sar_runtime_set_test_option(sar_runtime* rt, const char* name, uint64_t value);

/* Measurement hook: the individual HIP-event spans the runtime holds ("timing_accumulate": one per launch of every render call
 * since sar_runtime_last_timing last read them), in launch order. which = 0 the iterate kernel, 1 accumulate + fold, 2 warm-up.
 * Writes min(*out_n, cap) values; synchronises the runtime's stream. (tools/dispatch_times.py: one kernel's dispatch-by-dispatch
 * durations with and without a tracer attached.) */
int sar_runtime_debug_spans(sar_runtime* rt, uint32_t which, float* out_ms, uint32_t cap, uint32_t* out_n);

/* Statistic: the colorize kernels this runtime has enqueued since it was made — alone, or as the leader (first frame) of a run of
 * sar_colorize_device_batch that shares ONE launch. (The exposure kernels that may precede them are not counted.) */
int sar_runtime_debug_colorize_launches(const sar_runtime* rt, uint64_t* out);

/* Test hook: the runtime holds, afterwards, a volume exactly as if a sar_runtime_volume call with (slabs, z_lo, z_hi) at the runtime's
 * current size had produced the [slabs][height][width] voxels at vol_host — so that sar_runtime_volume_section / _read / _march and
 * sar_runtime_volume with add = 1 can be held to their restatement on volumes no run of jobs reaches in a test's time (counts near
 * 2^32, 1024 slabs deep, empty, ...). Refuses (SAR_ERR_INVALID, text in sar_last_error()) a NULL runtime or pointer, slabs outside
 * 1..1024, more than 2^30 voxels and a z_lo / z_hi that sar_runtime_volume refuses; a refusal leaves a held volume as it was. The
 * statistics of the loaded volume (sar_runtime_volume's add = 1 continues them): nonempty and vmax from the device's reduction pass,
 * visits = stored = the 64-bit sum of the voxels, below = above = nan = 0, z_min = +inf and z_max = -inf (no depth is known).
 * Synchronises the runtime's stream; the frame (count, zbuf, steps, max) is not touched. */
int sar_runtime_debug_volume_load(sar_runtime* rt, uint32_t slabs, double z_lo, double z_hi, const uint32_t* vol_host);

/* Statistic: the sar_volume_stats the runtime keeps for its held volume (what the last sar_runtime_volume reported, or what the load
 * above made: nonempty and vmax are the device's). Refused: NULLs, no held volume. No device call. */
int sar_runtime_debug_volume_stats(const sar_runtime* rt, sar_volume_stats* out);

/* Test hook: the logarithm the kernels take, on the caller's n arguments. kind 0: out[i] = log(in[i]), in = n doubles — the log of
 * k_plane_colorize and k_ftle_colorize. kind 1: out[i] = ln_u32(in[i]), in = n uint32_t — the inline function the Gas colorize, the
 * exposure solve and the gallery's tile colorize call, with this runtime's table: host libm's value for in[i] - 1 < 2^20, the device's
 * log beyond it, -inf for 0 (the u32 wrap of count + 1). Compiled with the kernels' flags, next to them. Refuses (SAR_ERR_INVALID, text in
 * sar_last_error()) NULLs, another kind, n == 0 and n > 2^20 (this hook's limit). Synchronises the runtime's stream; touches no state
 * of the runtime. (tests/test_gpu_device_log.py holds every result to the two doubles that enclose the true logarithm.) */
int sar_runtime_debug_device_log(sar_runtime* rt, uint32_t kind, const void* in, uint32_t n, double* out);

#ifdef __cplusplus
}
#endif
#endif /* SAR_TEST_HOOKS_H */
