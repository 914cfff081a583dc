// sar_shade.hip — the gfx950 kernel of shaded rendering (sar_shade, include/sar.h): a stencil over the depth buffer.
//
// k_shade: a workgroup of 256 lanes owns a tile of 32 x 16 outputs (a lane owns two pixels of one column, 8 rows apart). Three passes
// with a barrier between them:
//   1. the raw depths of the tile plus an (Rz + 1)-wide halo go to LDS as floats — the high word of the depth key through
//      sortable_f32, with the count for the surface test; a pixel that is not surface (or lies outside the image) is staged as NaN,
//      which makes the surface test of every later step one compare. A tile whose OWN pixels hold no surface writes its background and
//      stops here: four fifths of a typical frame.
//   2. z~ (the 3 x 3 range-limited mean, or the depth itself) of the tile plus an Rz-wide halo goes to LDS as doubles, NaN where the
//      pixel is not surface; the lane that computes a tile pixel's z~ counts it as `smoothed`.
//   3. each lane shades its pixels: the normal from the four neighbours of z~, the two light terms, the occlusion taps in the
//      contract's order (dy outer, dx inner; a tap outside the disc is skipped for the whole wave, which changes no bit; a NaN
//      neighbour fails `h > 0` and adds nothing), the hue from steps and the palette read from device memory for surface pixels
//      only, and 8 bytes written per pixel, consecutive lanes to consecutive pixels.
// Rz = max(R, 1): the normal reads the four neighbours' z~ whatever R is.
//
// LDS traffic: the 32 lanes of a half-wave read 32 consecutive floats (ds_read_b32: banks a/4 mod 32) or doubles (ds_read_b64: banks
// a/4 mod 64) of ONE halo row in pass 3 — conflict-free, a lane group never spans two rows, and the rows need no padding. inv_d[d2]
// and the palette rows of equal index are broadcasts. In the staging passes consecutive lanes take consecutive entries of the halo
// image: a half-wave spans at most two rows, still consecutive addresses, conflict-free for the float writes and the float reads of
// the 3 x 3 window; the ds_write_b64 of z~ (every ds_write banks mod 32) is 2-way: 32 doubles cover the 32 banks twice. It is one
// write per entry against up to 197 reads.
//
// The statistics (all integers) fold through a wave reduction, LDS atomics and one global atomic per block and field. A pixel's
// fp64 sums run in one lane in the contract's order. What is fused is the expansion of the divisions and square roots alone: the
// build's fused-op audit pins k_shade at their number.
#include "sar_device.hpp"
#include "sar_shade.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

namespace {

__device__ inline uint32_t shade_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

}  // namespace

__global__ void __launch_bounds__(kShadeThreads) k_shade(const ShadeArgs a) {
    extern __shared__ double lds[];
    __shared__ double s_pal[(SAR_PALETTE_MAX + 1) * 3];
    __shared__ double s_inv[kShadeMaxRadius * kShadeMaxRadius + 1];
    __shared__ uint32_t s_sum[5];  // surface, background, isolated, occluded, smoothed
    __shared__ uint32_t s_any;     // a pixel of the tile itself is surface

    const uint32_t tid = threadIdx.x;
    const uint32_t R = a.R, Rz = a.Rz, Rr = Rz + 1u;
    const uint32_t sw = kShadeTileW + 2u * Rz, sh = kShadeTileH + 2u * Rz;  // z~: tile + Rz
    const uint32_t rw = sw + 2u, rh = sh + 2u;                              // raw depths: tile + Rz + 1
    double* l_zt = lds;                                     // [sh][sw]
    float* l_z = reinterpret_cast<float*>(lds + sw * sh);   // [rh][rw]
    const uint32_t x0 = (blockIdx.x % a.tiles_x) * kShadeTileW, y0 = (blockIdx.x / a.tiles_x) * kShadeTileH;
    const float nanf32 = __uint_as_float(0x7FC00000u);
    const double nan64 = __longlong_as_double(0x7FF8000000000000ll);

    if (tid < 5u) s_sum[tid] = 0u;
    if (tid == 5u) s_any = 0u;
    for (uint32_t i = tid; i < (a.pal.len + 1u) * 3u; i += kShadeThreads) s_pal[i] = a.pal.rgb[i / 3u][i % 3u];
    for (uint32_t i = tid; i <= R * R; i += kShadeThreads) s_inv[i] = a.inv_d[i];
    __syncthreads();

    // pass 1: the raw depths of tile and halo, NaN where the pixel is not surface
    uint32_t any = 0u;
    for (uint32_t i = tid; i < rw * rh; i += kShadeThreads) {
        const uint32_t hy = i / rw, hx = i - hy * rw;
        const uint32_t gx = x0 + hx - Rr, gy = y0 + hy - Rr;  // (wraps below 0: then >= width / height)
        float z = nanf32;
        if (gx < a.width && gy < a.height) {
            const size_t p = static_cast<size_t>(gy) * a.width + gx;
            const float zr = sortable_f32(static_cast<uint32_t>(a.key[p] >> 32));
            const bool finite = (__float_as_uint(zr) & 0x7F800000u) != 0x7F800000u;
            if (finite && zr != -1.0f && a.count[p] >= a.min_count) {
                z = zr;
                any |= (hx - Rr < kShadeTileW && hy - Rr < kShadeTileH) ? 1u : 0u;
            }
        }
        l_z[i] = z;
    }
    if (any) atomicOr(&s_any, 1u);
    __syncthreads();

    const uint32_t tx = tid & 31u;
    const ushort4 bg = make_ushort4(a.background[0], a.background[1], a.background[2], a.background[3]);
    uint32_t n_surface = 0u, n_background = 0u, n_isolated = 0u, n_occluded = 0u, n_smoothed = 0u;

    if (s_any == 0u) {  // block-uniform: nothing to light in this tile
        for (uint32_t ty = tid >> 5; ty < kShadeTileH; ty += kShadeThreads / kShadeTileW) {
            const uint32_t px = x0 + tx, py = y0 + ty;
            if (px >= a.width || py >= a.height) continue;
            a.out[static_cast<size_t>(py) * a.width + px] = bg;
            ++n_background;
        }
    } else {
        // pass 2: z~ of tile and halo
        for (uint32_t i = tid; i < sw * sh; i += kShadeThreads) {
            const uint32_t hy = i / sw, hx = i - hy * sw;
            const uint32_t rc = (hy + 1u) * rw + hx + 1u;
            const float zf = l_z[rc];
            double zt = nan64;
            if (zf == zf) {
                const double zp = static_cast<double>(zf);
                zt = zp;
                if (a.smooth) {
                    double sum = 0.;
                    uint32_t n = 0u;
                    for (int dy = -1; dy <= 1; ++dy)
                        for (int dx = -1; dx <= 1; ++dx) {
                            const double zq = static_cast<double>(l_z[static_cast<int>(rc) + dy * static_cast<int>(rw) + dx]);
                            const double diff = zq - zp;
                            const double reach = fabs(diff) * a.k;
                            if (reach <= a.smooth_range) {  // (a NaN neighbour fails it)
                                sum = sum + zq;
                                ++n;
                            }
                        }
                    zt = sum / static_cast<double>(n);  // (n >= 1: the centre)
                    n_smoothed += (n > 1u && hx - Rz < kShadeTileW && hy - Rz < kShadeTileH) ? 1u : 0u;
                }
            }
            l_zt[i] = zt;
        }
        __syncthreads();

        // pass 3: a lane's own pixels
        const int r = static_cast<int>(R);
        const uint32_t r2 = R * R;
#pragma unroll 1
        for (uint32_t ty = tid >> 5; ty < kShadeTileH; ty += kShadeThreads / kShadeTileW) {
            const uint32_t px = x0 + tx, py = y0 + ty;
            if (px >= a.width || py >= a.height) continue;
            const size_t p = static_cast<size_t>(py) * a.width + px;
            const uint32_t centre = (ty + Rz) * sw + tx + Rz;
            const double zp = l_zt[centre];
            if (!(zp == zp)) {
                a.out[p] = bg;
                ++n_background;
                continue;
            }
            ++n_surface;
            // the normal
            const double zr = l_zt[centre + 1u], zl = l_zt[centre - 1u], zd = l_zt[centre + sw], zu = l_zt[centre - sw];
            const bool has_r = zr == zr, has_l = zl == zl, has_d = zd == zd, has_u = zu == zu;
            n_isolated += (has_r || has_l || has_d || has_u) ? 0u : 1u;
            const double ax = zr - zp, bx = zp - zl, ay = zd - zp, by = zp - zu;
            const double gx = has_r ? (has_l ? (fabs(ax) <= fabs(bx) ? ax : bx) : ax) : (has_l ? bx : 0.);
            const double gy = has_d ? (has_u ? (fabs(ay) <= fabs(by) ? ay : by) : ay) : (has_u ? by : 0.);
            const double sx = gx * a.k, sy = gy * a.k;
            const double len = sqrt((sx * sx + sy * sy) + 1.0);
            const double nx = -sx / len, ny = -sy / len, nz = 1.0 / len;
            // the light
            double d = (nx * a.L[0] + ny * a.L[1]) + nz * a.L[2];
            d = d > 0. ? d : 0.;
            double s = 0.;
            if (a.spec_on) {
                s = (nx * a.H[0] + ny * a.H[1]) + nz * a.H[2];
                s = s > 0. ? s : 0.;
                for (uint32_t j = 0; j < a.shininess_log2; ++j) s = s * s;
            }
            // the occlusion
            double occ = 0.;
            for (int dy = -r; dy <= r; ++dy)
                for (int dx = -r; dx <= r; ++dx) {
                    const uint32_t d2 = static_cast<uint32_t>(dx * dx + dy * dy);
                    if (d2 == 0u || d2 > r2) continue;  // wave-uniform
                    const double zq = l_zt[static_cast<uint32_t>(static_cast<int>(centre) + dy * static_cast<int>(sw) + dx)];
                    const double h = (zq - zp) * a.k;
                    if (h > 0. && h <= a.ao_range) {
                        const double t = h * s_inv[d2];
                        occ = occ + (t < 1. ? t : 1.);
                    }
                }
            n_occluded += occ > 0. ? 1u : 0u;
            double ao = 1.;
            if (R) {
                ao = 1. - a.ao_strength * (occ / static_cast<double>(a.taps));
                ao = ao > 0. ? ao : 0.;
            }
            // the hue
            double v = a.steps[p];
            if (a.window) v = a.w_pos_lo + ((v - a.w_lo) / a.w_span) * a.w_dpos;
            double red, green, blue;
            palette_blend(v, s_pal, a.pal.len, red, green, blue);
            // the pixel
            const double lum = ao * (a.ambient + a.diffuse * d), glint = ao * (a.specular * s);
            double cr = red * lum + glint, cg = green * lum + glint, cb = blue * lum + glint;
            cr = cr > 0. ? cr : 0.;
            cg = cg > 0. ? cg : 0.;
            cb = cb > 0. ? cb : 0.;
            cr = cr < 1. ? cr : 1.;
            cg = cg < 1. ? cg : 1.;
            cb = cb < 1. ? cb : 1.;
            ushort4 o;
            o.x = as_u16(cr * 65535.0);
            o.y = as_u16(cg * 65535.0);
            o.z = as_u16(cb * 65535.0);
            o.w = 65535;
            a.out[p] = o;
        }
    }

    // wave -> LDS -> one global atomic per block and field (a zero adds nothing and is not sent)
    n_surface = shade_wave_sum(n_surface);
    n_background = shade_wave_sum(n_background);
    n_isolated = shade_wave_sum(n_isolated);
    n_occluded = shade_wave_sum(n_occluded);
    n_smoothed = shade_wave_sum(n_smoothed);
    if ((tid & 63u) == 0u) {
        if (n_surface) atomicAdd(&s_sum[0], n_surface);
        if (n_background) atomicAdd(&s_sum[1], n_background);
        if (n_isolated) atomicAdd(&s_sum[2], n_isolated);
        if (n_occluded) atomicAdd(&s_sum[3], n_occluded);
        if (n_smoothed) atomicAdd(&s_sum[4], n_smoothed);
    }
    __syncthreads();
    if (tid == 0) {
        if (s_sum[0]) atomicAdd(&a.stats->surface, s_sum[0]);
        if (s_sum[1]) atomicAdd(&a.stats->background, s_sum[1]);
        if (s_sum[2]) atomicAdd(&a.stats->isolated, s_sum[2]);
        if (s_sum[3]) atomicAdd(&a.stats->occluded, s_sum[3]);
        if (s_sum[4]) atomicAdd(&a.stats->smoothed, s_sum[4]);
    }
}

void launch_shade(const ShadeArgs& a, uint32_t tiles, hipStream_t s) {
    // 19 088 bytes at R = 8: below the 64 KiB a kernel may take without an attribute
    hipLaunchKernelGGL(k_shade, dim3(tiles), dim3(kShadeThreads), shade_lds_bytes(a.Rz), s, a);
}

}  // namespace sar
