// sar_basin.hip — gfx950 (MI355X) kernels of the basins of attraction (include/sar.h: sar_runtime_basin, sar_runtime_basin_colorize).
//
// k_basin_screen finds the fate of every pixel of a launch — one lane per start point, a wave per 8 x 8 tile as in k_plane, because
// neighbours share their fate — and packs the survivors; k_basin_mark, one lane per SURVIVOR so that its waves are full where most of
// a window escapes, walks each survivor's tail and unites the grid cells of consecutive points in a lock-free union-find; k_basin_finish,
// behind the kernel boundary, resolves every pixel's and every visited cell's root. All lanes step ONE map: its 30 coefficients are
// kernel arguments, the x and y rows scalar operands and the z row pinned into VGPRs (pin_z_row, sar_tangent.hpp). The map, the start point and
// the node are multiplies, adds and compares: no division, square root or logarithm, so the build's fused-op audit pins the first two
// kernels at 0 and a host restatement gives the same records bit for bit. k_basin_colorize has one division and three square roots.
// DESIGN.md section 17 has the union-find's argument and the resources.
#include "sar_basin.hpp"
#include "sar_tangent.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

__device__ __forceinline__ uint32_t basin_node(const BasinArgs& a, double x, double y, double z) {
    const uint32_t cx = basin_cell(x, a.box_lo[0], a.scale[0], a.grid);
    const uint32_t cy = basin_cell(y, a.box_lo[1], a.scale[1], a.grid);
    const uint32_t cz = basin_cell(z, a.box_lo[2], a.scale[2], a.grid);
    return (cz * a.grid + cy) * a.grid + cx;  // < grid^3 <= 2^21
}

// ---------------------------------------------------------------------------------------------------
// k_basin_screen — transient + steps steps from the pixel's start point; a lane is dead once its point leaves the bound box
// (escape_step: that step, counted from the start), and a wave whose lanes are all dead stops (CheckedSteps). The
// tail steps run here too, so that a pixel that escapes late never reaches k_basin_mark. Survivors are appended with one atomic per
// wave, {pixel, the point after the transient}; their order depends on which wave lands first, the results do not. The lanes of a
// partial tile step some point with the others; they are never alive and write nothing.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_basin_screen(const BasinArgs a) {
    const TilePixel tp = tile_pixel(a.first_tile, a.n_tiles, a.tiles_x, a.width, a.height);
    const uint32_t px = tp.px, py = tp.py;
    const bool valid = tp.valid;
    const SearchCoeffs c = pin_z_row(a.map);
    const double tu = a.tu[px < a.width ? px : a.width - 1u], tv = a.tv[py < a.height ? py : a.height - 1u];  // (in bounds for every lane)
    double x = basin_start(a.origin[0], a.du[0], a.dv[0], tu, tv);
    double y = basin_start(a.origin[1], a.du[1], a.dv[1], tu, tv);
    double z = basin_start(a.origin[2], a.du[2], a.dv[2], tu, tv);
    const double bound = a.bound;
    bool alive = valid;
    uint32_t esc = 0;
    for (CheckedSteps run(a.transient); run.next(alive);)
        for (uint32_t t = run.t0; t < run.t1; ++t) {
            next_point(c, x, y, z);
            const bool in = within(x, y, z, bound);
            esc = (alive & !in) ? t + 1u : esc;
            alive = alive & in;
        }
    const double x0 = x, y0 = y, z0 = z;  // a survivor's first tail point
    for (CheckedSteps run(a.steps); run.next(alive);)
        for (uint32_t t = run.t0; t < run.t1; ++t) {
            next_point(c, x, y, z);
            const bool in = within(x, y, z, bound);
            esc = (alive & !in) ? a.transient + t + 1u : esc;  // (transient + steps < 2^32)
            alive = alive & in;
        }
    const uint32_t s = wave_append(alive, a.counter);  // < the survivors of this launch <= slots
    if (!valid) return;
    const uint32_t pixel = py * a.width + px;
    uint4 rec;
    rec.x = alive ? (uint32_t)SAR_SEARCH_BOUNDED : (uint32_t)SAR_SEARCH_DIVERGED;
    rec.y = esc;
    rec.z = rec.w = kBasinEmpty;
    *(uint4*)(a.pixels + pixel) = rec;
    if (alive) {
        a.surv_pix[s] = pixel;
        a.surv_xyz[s] = x0;
        a.surv_xyz[a.slots + s] = y0;
        a.surv_xyz[2u * a.slots + s] = z0;
    }
}

// ---------------------------------------------------------------------------------------------------
// The union-find over parent[grid^3]. INVARIANT: parent[v] is kBasinEmpty (no tail has visited v), v itself (v is a root) or a node
// below v — a root is only ever hooked under a SMALLER root —, so parent[v] <= v for every visited v at all times, every chain
// v, parent[v], parent[parent[v]], ... is strictly decreasing and ends after at most v links, and the final root of a component
// is its smallest node. Every write is a device-scope atomicCAS (kBasinEmpty -> v to claim, v -> smaller root to hook): a node's
// parent changes at most twice and never back. Reads are relaxed agent-scope loads, L2-served, and the L2s of the eight XCDs are
// not coherent: a read may return an EARLIER value of the word. That is harmless. Every link ever written joins two nodes of one
// true component, so a stale chain is still a path inside the true component and "same root" never lies; a stale "v is a root" (or
// a stale kBasinEmpty of a claimed node) only makes the hooking CAS fail, and the retry goes on from the value the CAS returned,
// which comes from memory. A node is claimed before any link to it is written, so the CAS of a hook never meets kBasinEmpty.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t basin_parent(const uint32_t* parent, uint32_t v) {
    return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of v's chain as this lane sees it: at most v + 1 loads, the chain is strictly decreasing
__device__ __forceinline__ uint32_t basin_find(const uint32_t* parent, uint32_t v) {
    for (;;) {
        const uint32_t p = basin_parent(parent, v);
        if (p >= v) return v;  // v itself: a root; kBasinEmpty: a stale read of a claimed node, a root as far as this lane knows
        v = p;
    }
}

__device__ __forceinline__ void basin_claim(uint32_t* parent, uint32_t v) {
    if (basin_parent(parent, v) == kBasinEmpty) atomicCAS(parent + v, kBasinEmpty, v);  // (a stale kBasinEmpty: the CAS fails, no harm)
}

// joins the components of two claimed nodes. Each pass either returns or lowers hi: at most hi + lo passes
__device__ __forceinline__ void basin_unite(uint32_t* parent, uint32_t u, uint32_t v) {
    for (;;) {
        u = basin_find(parent, u);
        v = basin_find(parent, v);
        if (u == v) return;  // already one component: after a tail's first steps almost every call ends here, read-only
        const uint32_t hi = u > v ? u : v, lo = u > v ? v : u;
        const uint32_t old = atomicCAS(parent + hi, hi, lo);  // the larger root under the smaller one
        if (old == hi) return;
        u = old;  // hi was no root any more: old < hi is its parent, in hi's component — go on from there
        v = lo;
    }
}

// ---------------------------------------------------------------------------------------------------
// k_basin_mark — one lane per survivor slot of the launch: the `steps` tail steps again from the packed point (no bound test: the
// screen has run them), the node of every point, a unite wherever two consecutive nodes differ, the raw extent of the tail points
// (one atomicMin / atomicMax per wave and bound, on the sortable 64-bit image) and the node of the last point for k_basin_finish.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_basin_mark(const BasinArgs a) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n = a.counter[0];
    if ((s & ~63u) >= n) return;  // (the whole wave)
    const bool valid = s < n;
    const SearchCoeffs c = pin_z_row(a.map);
    double lo[3] = {__builtin_inf(), __builtin_inf(), __builtin_inf()}, hi[3] = {-__builtin_inf(), -__builtin_inf(), -__builtin_inf()};
    if (valid) {
        double x = a.surv_xyz[s], y = a.surv_xyz[a.slots + s], z = a.surv_xyz[2u * a.slots + s];
        uint32_t prev = basin_node(a, x, y, z);
        basin_claim(a.parent, prev);
        lo[0] = hi[0] = x;
        lo[1] = hi[1] = y;
        lo[2] = hi[2] = z;
        for (uint32_t t = 0; t < a.steps; ++t) {
            next_point(c, x, y, z);
            lo[0] = x < lo[0] ? x : lo[0];
            hi[0] = x > hi[0] ? x : hi[0];
            lo[1] = y < lo[1] ? y : lo[1];
            hi[1] = y > hi[1] ? y : hi[1];
            lo[2] = z < lo[2] ? z : lo[2];
            hi[2] = z > hi[2] ? z : hi[2];
            const uint32_t node = basin_node(a, x, y, z);
            if (node != prev) {
                basin_claim(a.parent, node);
                basin_unite(a.parent, prev, node);
                prev = node;
            }
        }
        a.last_node[a.surv_pix[s]] = prev;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) wave_extent(lo[k], hi[k], a.extent + 2 * k, a.extent + 2 * k + 1);
}

// ---------------------------------------------------------------------------------------------------
// k_basin_finish — behind the kernel boundary every hook is visible: find() is exact. Lane i resolves pixel i's root from the node
// of its last tail point, and cell i's root where a tail has visited it.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_basin_finish(const BasinArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.width * a.height && a.pixels[i].status == SAR_SEARCH_BOUNDED) a.pixels[i].root = basin_find(a.parent, a.last_node[i]);
    if (i < a.nodes) a.node_root[i] = basin_parent(a.parent, i) == kBasinEmpty ? kBasinEmpty : basin_find(a.parent, i);
}

// ---------------------------------------------------------------------------------------------------
// k_basin_colorize — include/sar.h: sar_basin_colors. One division serves both kinds of pixel: e / (e + fade) of an escaped one,
// (label + 0.5) / attractors of a bounded one, the palette's position (palette_blend).
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_basin_colorize(const sar_basin_pixel* pixels, const uint32_t* labels, uint32_t npix,
                                                        const PaletteParams pal, double attractors, double fade, ushort4* out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const bool escaped = pixels[p].status != SAR_SEARCH_BOUNDED;
    const double e = (double)pixels[p].escape_step;
    const double num = escaped ? e : (double)labels[p] + 0.5;
    const double den = escaped ? e + fade : attractors;
    const double q = num / den;
    ushort4 o;
    o.w = 65535;
    if (escaped) {
        const double g = 0.5 * q;
        o.x = o.y = o.z = as_u16(g * 65535.);
    } else {
        double r, g, b;
        palette_blend(q, &pal.rgb[0][0], pal.len, r, g, b);
        o.x = as_u16(r * 65535.);
        o.y = as_u16(g * 65535.);
        o.z = as_u16(b * 65535.);
    }
    out[p] = o;
}

void launch_basin_screen(const BasinArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_basin_screen, dim3((a.n_tiles + 3u) / 4u), dim3(256), 0, s, a);  // four waves per workgroup, a tile each
}
void launch_basin_mark(const BasinArgs& a, hipStream_t s) {
    // as many lanes as the launch has pixels: the survivor count stays on the device, the waves beyond it return at once
    hipLaunchKernelGGL(k_basin_mark, dim3((a.slots + 255u) / 256u), dim3(256), 0, s, a);
}
void launch_basin_finish(const BasinArgs& a, hipStream_t s) {
    const uint32_t npix = a.width * a.height, n = npix > a.nodes ? npix : a.nodes;
    hipLaunchKernelGGL(k_basin_finish, dim3((n + 255u) / 256u), dim3(256), 0, s, a);
}
void launch_basin_colorize(const sar_basin_pixel* pixels, const uint32_t* labels, uint32_t npix, const PaletteParams& pal,
                           uint32_t attractors, double fade, void* rgba16_out, hipStream_t s) {
    hipLaunchKernelGGL(k_basin_colorize, dim3((npix + 255u) / 256u), dim3(256), 0, s, pixels, labels, npix, pal, (double)attractors, fade,
                       (ushort4*)rgba16_out);
}

}  // namespace sar
