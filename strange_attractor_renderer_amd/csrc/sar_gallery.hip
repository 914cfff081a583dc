// sar_gallery.hip — gfx950 (MI355X) kernel of the gallery (include/sar.h: sar_runtime_gallery): k_gallery takes ONE map from its
// start points to its finished RGBA16 tile in ONE workgroup. A tile is an ordinary small render — sar_render_jobs + sar_colorize
// of a tile-sized config on a fresh runtime, bit for bit — but small enough that a CU's LDS holds its image: every visit is an
// LDS atomic, and neither the record arena nor the binned accumulate nor the fold of the frame path is involved. DESIGN.md
// section 14 has the LDS budget and the reasons for the pass structure; sar_device.hpp states the bit-exactness contract.
#include "sar_device.hpp"
#include "sar_gallery.hpp"

namespace sar {

// LDS of a tile: 8 bytes per pixel (at most 128 KiB), used twice —
//   traversal 1   key[npix] u64: sortable(z) << 32 | (0xFFFFFFFF - visit ordinal), raised with the 64-bit LDS max
//   in between    the keys' depths leave for the raw zbuf tile; their low words stay, packed: ord[npix] u32, then count[npix] u32
//   traversal 2   count[npix] takes one LDS add per visit; the visit whose ordinal is the pixel's ord evaluates the colour
//                 transform: it is the final winner, whatever order the atomics of traversal 1 landed in
// count (4 B), key (8 B) and steps (8 B) of 16 384 pixels at once would be 320 KiB; two traversals of the same trajectories
// (about 10^6 iterations a tile) cost less than the global scatter they replace. One code path for every tile size.
typedef unsigned long long __attribute__((may_alias)) lds_u64;
typedef uint32_t __attribute__((may_alias)) lds_u32;

enum : uint32_t { GR_MAX = 0, GR_COVERED = 1, GR_DEAD = 2, GR_ZMAX = 3, GR_ZMIN = 4, GR_COUNT = 5 };

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

__global__ void __launch_bounds__(kGalleryBlock) k_gallery(const GalleryArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char g_lds[];
    __shared__ double s_pal[(SAR_PALETTE_MAX + 1) * 3];
    __shared__ unsigned long long s_hits;
    __shared__ uint32_t s_red[GR_COUNT];

    const uint32_t tid = threadIdx.x, slot = blockIdx.x, npix = a.npix, jobs = a.jobs, n = a.iters;
    const uint32_t tile = a.first_tile + slot;
    const GalleryTile T = load_frame_args(a.tiles + tile);
    MapParams p = T.p;
    pin_map_params(p);

    lds_u64* const l_key = (lds_u64*)g_lds;
    lds_u32* const l_ord = (lds_u32*)g_lds;
    lds_u32* const l_count = l_ord + npix;
    double* const warm = a.warm + (size_t)slot * 3u * jobs;
    uint32_t* const count_g = a.count + (size_t)slot * npix;
    float* const zbuf_g = a.zbuf + (size_t)slot * npix;
    double* const steps_g = a.steps + (size_t)slot * npix;

    const uint32_t unset = f32_sortable(-1.0f);
    const uint32_t zmax_seed = f32_sortable(0.0f);                                    // the depth range folds from (0.0, f32::MAX), :877-882
    const uint32_t zmin_seed = f32_sortable(3.40282346638528859811704183484516925e+38f);

    // ---- every tile starts from the reset state (:682-699): keys at zbuf = -1.0, nothing left of the tile before ------------
    for (uint32_t px = tid; px < npix; px += blockDim.x) l_key[px] = ((unsigned long long)unset << 32) | 0xFFFFFFFFull;
    for (uint32_t k = tid; k < (a.pal.len + 1) * 3; k += blockDim.x) s_pal[k] = a.pal.rgb[k / 3][k % 3];
    if (tid == 0) {
        s_hits = 0ull;
        s_red[GR_MAX] = 0u;
        s_red[GR_COVERED] = 0u;
        s_red[GR_DEAD] = 0u;
        s_red[GR_ZMAX] = zmax_seed;
        s_red[GR_ZMIN] = zmin_seed;
    }

    // ---- warm-up (:750-752): lanes take jobs tid, tid + blockDim, ...; the point after it is kept for both traversals ---------
    uint32_t dead = 0;
    for (uint32_t job = tid; job < jobs; job += blockDim.x) {
        double x = a.starts[3u * (size_t)job], y = a.starts[3u * (size_t)job + 1u], z = a.starts[3u * (size_t)job + 2u];
        for (int w = 0; w < 1000; ++w) next_point(p, x, y, z);
        warm[job] = x;
        warm[(size_t)jobs + job] = y;
        warm[2u * (size_t)jobs + job] = z;
        // left for infinity: an x that is not finite never comes back (+-inf stays or turns NaN, NaN is absorbing). Such a job only
        // counts here; its iterations go the ordinary way below — beyond the image, or as NaN on pixel (0,0) — and win no depth test
        dead += (fabs(x) < __builtin_inf()) ? 0u : 1u;
    }
    __syncthreads();

    // ---- traversal 1: the depth keys. visit ordinal = job * n + t (job-major, iteration-minor: the reference's sequential
    // order); the low word is 0xFFFFFFFF - ordinal, so the EARLIEST visit wins an exact depth tie ------------------------------
    for (uint32_t job = tid; job < jobs; job += blockDim.x) {
        double x = warm[job], y = warm[(size_t)jobs + job], z = warm[2u * (size_t)jobs + job];
        if (x != x) continue;
        const uint32_t lo_base = 0xFFFFFFFFu - job * n;
        for (uint32_t t = 0; t < n; ++t) {
            bool inb;
            uint32_t idx;
            float zf;
            iterate_once(p, a.tile_width, x, y, z, inb, idx, zf);
            if (x != x) break;  // the rest of the job is NaN: no depth candidate among it
            // strict `>` against an initial -1.0 (:693, :821): z <= -1 and NaN can never win
            if (inb && zf > -1.0f) {
                zf = zf + 0.0f;  // -0.0 -> +0.0 so the integer order agrees with the float order
                const uint32_t zs = f32_sortable(zf);
                // a plain read of the depth already there filters most visits: "not deeper" needs no atomic (a tie does)
                if (zs >= l_ord[2u * idx + 1u])
                    __hip_atomic_fetch_max(l_key + idx, ((unsigned long long)zs << 32) | (unsigned long long)(lo_base - t), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
    __syncthreads();

    // ---- in between: key[px] -> raw zbuf, ord[px]; raw steps start at the reset value. Pixels in rounds of blockDim: a round's
    // ord words land inside the keys this round or an earlier one has read (4 (base + blockDim) <= 8 (base + blockDim)) ---------
    uint32_t zmx = zmax_seed, zmn = zmin_seed;
    for (uint32_t base = 0; base < npix; base += blockDim.x) {
        const uint32_t px = base + tid;
        unsigned long long k = 0ull;
        if (px < npix) k = l_key[px];
        __syncthreads();
        if (px < npix) {
            const uint32_t zs = (uint32_t)(k >> 32);
            l_ord[px] = (uint32_t)k;
            if (zs != unset) {  // k_zrange's fold
                zmx = zs > zmx ? zs : zmx;
                zmn = zs < zmn ? zs : zmn;
            }
            zbuf_g[px] = sortable_f32(zs);
            steps_g[px] = 0.;  // :690
        }
    }
    __syncthreads();
    for (uint32_t px = tid; px < npix; px += blockDim.x) l_count[px] = 0u;  // :687
    __syncthreads();

    // ---- traversal 2: the counts, and the payload of every pixel's final winner -----------------------------------------------
    for (uint32_t job = tid; job < jobs; job += blockDim.x) {
        double x = warm[job], y = warm[(size_t)jobs + job], z = warm[2u * (size_t)jobs + job];
        const uint32_t lo_base = 0xFFFFFFFFu - job * n;
        if (x != x) {  // died in the warm-up
            if (n) __hip_atomic_fetch_add(l_count, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            continue;
        }
        for (uint32_t t = 0; t < n; ++t) {
            const double px = x, py = y, pz = z;  // previous_point (:766 / :836)
            bool inb;
            uint32_t idx;
            float zf;
            iterate_once(p, a.tile_width, x, y, z, inb, idx, zf);
            if (x != x) {
                // this and every remaining iteration passes the bounds test (:789, all comparisons false) and casts to pixel
                // (0,0) (:800-802): added in one go, as k_iterate does
                __hip_atomic_fetch_add(l_count, n - t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                break;
            }
            if (inb) {
                __hip_atomic_fetch_add(l_count + idx, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // :807-812
                // a visit that can win (z > -1) on a pixel means the pixel is set, and its ord is a visit's: equal ordinals are
                // the same visit
                if (zf > -1.0f && l_ord[idx] == lo_base - t) {
                    double sx, sy, sz;
                    screen_space(p, x, y, z, sx, sy, sz);
                    steps_g[idx] = color_transform(T.ct, x - px, y - py, z - pz, sx, sy, sz);  // :822-830
                }
            }
        }
    }
    __threadfence_block();
    __syncthreads();

    // ---- the tile's scalars ---------------------------------------------------------------------------------------------------
    uint32_t m = 0, covered = 0;
    unsigned long long hits = 0;
    for (uint32_t px = tid; px < npix; px += blockDim.x) {
        const uint32_t c = l_count[px];
        m = c > m ? c : m;  // a fresh runtime's counts only grow and cannot wrap (jobs * iters < 2^32): the running max of :813-815
        covered += c ? 1u : 0u;
        hits += c;
        count_g[px] = c;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t om = __shfl_down(m, off), ox = __shfl_down(zmx, off), on = __shfl_down(zmn, off);
        m = om > m ? om : m;
        zmx = ox > zmx ? ox : zmx;
        zmn = on < zmn ? on : zmn;
        hits += __shfl_down(hits, off);
    }
    covered = wave_sum_u32(covered);
    dead = wave_sum_u32(dead);
    if ((tid & 63u) == 0u) {
        atomicMax(&s_red[GR_MAX], m);
        atomicAdd(&s_red[GR_COVERED], covered);
        atomicAdd(&s_red[GR_DEAD], dead);
        atomicMax(&s_red[GR_ZMAX], zmx);
        atomicMin(&s_red[GR_ZMIN], zmn);
        atomicAdd(&s_hits, hits);
    }
    __syncthreads();
    const uint32_t rmax = s_red[GR_MAX];
    if (tid == 0) {
        sar_gallery_stats st;
        st.max = rmax;
        st.covered = s_red[GR_COVERED];
        st.hits = s_hits;
        st.dead_jobs = s_red[GR_DEAD];
        st._pad = 0u;
        a.stats[tile] = st;
    }

    // ---- colorize (:841-904) from LDS, the tile's rows straight into the atlas ------------------------------------------------
    const uint32_t col = tile % a.cols, row = tile / a.cols, tw = a.tile_width;
    ushort4* const out = (ushort4*)a.atlas + ((size_t)row * a.tile_height) * a.atlas_width + (size_t)col * tw;
    if (a.render_kind == SAR_RENDER_GAS) {
        // colorize_gas_body's expressions (sar_image.hip), every pixel the long way
        const double ln_base = ln_u32(rmax + 1u, a.lut, a.lut_len);  // ln(max + 1), :860
        const double count_f64 = (double)a.pal.len;
        const uint32_t pal_len = a.pal.len;
        const double b_offset = a.b_offset, b_factor = a.b_factor;
        for (uint32_t px = tid; px < npix; px += blockDim.x) {
            // Palette::interpolate (:442-472)
            double v = steps_g[px];
            const uint32_t cnt = l_count[px];
            if (v < 0.) v = 0.;
            else if (v >= 1.) v = 0.999999;
            v = v * count_f64;
            const double fl = floor(v);
            uint32_t k = (fl == fl) ? (uint32_t)fl : 0u;
            if (k >= pal_len) k = pal_len - 1;  // unreachable for non-NaN
            const double t = v - fl;            // == v % 1. for v >= 0 (exact)
            const double t1 = 1.0 - t;
            const double* c1 = &s_pal[k * 3];
            const double* c2 = &s_pal[(k + 1) * 3];
            const double r = sqrt(c2[0] * t + c1[0] * t1);
            const double g = sqrt(c2[1] * t + c1[1] * t1);
            const double b = sqrt(c2[2] * t + c1[2] * t1);
            const double factor = ln_u32(cnt + 1u, a.lut, a.lut_len) / ln_base;  // :860
            ushort4 o;
            o.x = as_u16((r * factor + b_offset) * b_factor * 65535.);
            o.y = as_u16((g * factor + b_offset) * b_factor * 65535.);
            o.z = as_u16((b * factor + b_offset) * b_factor * 65535.);
            o.w = a.transparent ? as_u16(factor * 65535.) : (uint16_t)65535;
            const uint32_t y = px / tw;
            out[(size_t)y * a.atlas_width + (px - y * tw)] = o;
        }
    } else {
        // k_colorize_depth's expressions over the tile's own depth range
        const float zmax = sortable_f32(s_red[GR_ZMAX]);
        const float zmin = sortable_f32(s_red[GR_ZMIN]);
        const float diff = zmax - zmin;  // :883
        for (uint32_t px = tid; px < npix; px += blockDim.x) {
            float z = zbuf_g[px];  // (this lane wrote it)
            if (z == -1.0f) z = 0.0f;
            else z = __fdiv_rn(z - zmin, diff);  // f32 reverse lerp, :893
            const float s = z * 65535.0f;
            uint16_t v;  // Rust `as u16` of an f32
            if (!(s == s) || s <= 0.f) v = 0;
            else if (s >= 65535.f) v = 65535;
            else v = (uint16_t)(uint32_t)s;
            ushort4 o;
            o.x = v; o.y = v; o.z = v; o.w = 65535;
            const uint32_t y = px / tw;
            out[(size_t)y * a.atlas_width + (px - y * tw)] = o;
        }
    }
}

int launch_gallery(const GalleryArgs& a, uint32_t n_tiles, hipStream_t s) {
    // (per device and function; cheap next to a launch of whole tiles)
    const hipError_t e = hipFuncSetAttribute((const void*)k_gallery, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kMaxGalleryTilePixels * 8u));
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_gallery, dim3(n_tiles), dim3(kGalleryBlock), a.npix * 8u, s, a);
    return 0;
}

}  // namespace sar
