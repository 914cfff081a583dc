// sar_select.hip — gfx950 (MI355X): the exact two-quantile radix select (sar_internal.hpp: SelectState) and its two consumers, auto
// exposure and auto colour range. One histogram kernel and one scan kernel, instantiated per consumer and pass: a consumer is a
// traits struct that holds what differs — its key and frame table, its digit schedule, how pixels become (member, key) pairs, and
// the record it writes once both keys are pinned.
#include "sar_device.hpp"
#include "sar_launch.hpp"

namespace sar {

// one visit: the lanes of the wave that land in the first active lane's bucket add with ONE LDS atomic (the members crowd into few
// buckets: the lowest counts, three or four exponents), every other active lane with its own
__device__ __forceinline__ void wave_hist_add(uint32_t* s_h, bool active, uint32_t idx) {
    const unsigned long long m = wave_ballot(active);
    if (!m) return;
    const uint32_t lead = (uint32_t)__ffsll((long long)m) - 1u;
    const uint32_t lead_idx = (uint32_t)__shfl((int)idx, (int)lead, 64);
    const bool same = active && idx == lead_idx;
    const unsigned long long sm = wave_ballot(same);
    const uint32_t lane = threadIdx.x & 63u;
    if (lane == lead) atomicAdd(&s_h[lead_idx], (uint32_t)__popcll(sm));
    else if (active && !same) atomicAdd(&s_h[idx], 1u);
}

// the rank of quantile q among n members: floor(q n), at most n - 1 (include/sar.h states it for both consumers)
__device__ __forceinline__ uint32_t select_rank(double q, uint32_t n) {
    const double qn = q * (double)n;
    const uint32_t r = (uint32_t)floor(qn);
    return n && r > n - 1u ? n - 1u : r;
}

// ---------------------------------------------------------------------------------------------------
// the consumers. PASS is 1, 2, ... for a schedule whose passes differ (exposure), 1 and 2 = "any later one" where they do not.
//   Key, Batch            the key type and the launch's frame table
//   buckets / sub_hists   per pass: buckets of one histogram, LDS copies of it in a workgroup (4: one per wave, 1: shared)
//   hist_at               per pass: where its histogram(s) lie in the frame's scratch; kHistWords: where the state does
//   key_max               SelectState::max of a frame (pass 1 reads it here, the later ones in the state)
//   first_shift / next_shift   bits left below the first digit, and below the next one given those below the last
//   Pixels                a frame's pixels as (member, key) pairs, made once per workgroup from the frame and SelectState::max:
//                         quad(i, in, visit) calls visit(member, key) for the four pixels of index i of the uint4 view (`in`: i
//                         is inside the image), pixel(p, in, visit) for pixel p
//   record                writes the frame's record from the final state
// ---------------------------------------------------------------------------------------------------
struct ExpoSelect {
    typedef uint32_t Key;
    typedef ExpoBatch Batch;
    static constexpr uint32_t kHistWords = kExpoHistWords;
    static constexpr uint32_t buckets(int pass) { return pass == 3 ? kExpoBuckets3 : kExpoBuckets; }
    static constexpr uint32_t sub_hists(int pass) { return pass == 2 ? 1u : 4u; }  // (pass 2: the pixels of two buckets only)
    static constexpr uint32_t hist_at(int pass) { return pass == 1 ? 0u : pass == 2 ? kExpoH2 : kExpoH3; }
    static __device__ __forceinline__ uint32_t key_max(const Batch::Frame& f) { return f.scalars[SC_WRAP] ? 0xFFFFFFFFu : f.scalars[SC_MAX]; }
    static __device__ __forceinline__ uint32_t shift_below(uint32_t bits) { return bits > 12u ? bits - 12u : 0u; }
    static __device__ __forceinline__ uint32_t first_shift(uint32_t M) { return shift_below(32u - (uint32_t)__clz((int)M)); }  // (__clz(0) = 32: M = 0 has no bits)
    static __device__ __forceinline__ uint32_t next_shift(int pass, uint32_t shift) { return pass == 3 ? 0u : shift_below(shift); }

    struct Pixels {
        const uint32_t* count;
        uint32_t M;
        __device__ __forceinline__ Pixels(const Batch::Frame& f, uint32_t M_) : count(f.count), M(M_) {}
        template <typename Visit>
        __device__ __forceinline__ void quad(uint32_t i, bool in, Visit visit) const {
            const uint4 c = in ? ((const uint4*)count)[i] : make_uint4(0u, 0u, 0u, 0u);
            one(in, c.x, visit);
            one(in, c.y, visit);
            one(in, c.z, visit);
            one(in, c.w, visit);
        }
        template <typename Visit>
        __device__ __forceinline__ void pixel(uint32_t p, bool in, Visit visit) const { one(in, in ? count[p] : 0u, visit); }
        template <typename Visit>
        __device__ __forceinline__ void one(bool in, uint32_t c, Visit visit) const {
            visit(in && c != 0u, c < M ? c : M);  // uncovered pixels: no atomic
        }
    };

    // F(c) = ln(c+1) / ln(M+1) and the two constants, exactly as include/sar.h states them (no contraction: -ffp-contract=off)
    static __device__ __forceinline__ void record(const Batch& t, const Batch::Frame& f, const SelectState<Key>& st) {
        sar_exposure r;
        r.black_count = st.n ? st.prefix[0] : 0u;
        r.white_count = st.n ? st.prefix[1] : 0u;
        r.covered = st.n;
        r.max = st.max;
        r._pad = 0;
        const double ln_base = ln_u32(st.max + 1u, t.lut, t.lut_len);
        const double fb = ln_u32(r.black_count + 1u, t.lut, t.lut_len) / ln_base;
        const double fw = ln_u32(r.white_count + 1u, t.lut, t.lut_len) / ln_base;
        const double df = fw - fb;
        bool ok = st.n != 0u && df > 0. && df <= 1.7976931348623157e308;
        double factor = 0., offset = 0.;
        if (ok) {
            factor = (f.level[1] - f.level[0]) / df;
            offset = f.level[0] / factor - fb;
            ok = isfinite(factor) && isfinite(offset);
        }
        r.offset = ok ? offset : f.cfg_offset;
        r.factor = ok ? factor : f.cfg_factor;
        r.applied = ok ? 1 : 0;
        *f.rec = r;
    }
};

struct CrSelect {
    typedef unsigned long long Key;
    typedef CrBatch Batch;
    static constexpr uint32_t kHistWords = kCrHistWords;
    static constexpr uint32_t buckets(int pass) { return pass == 1 ? kCrBuckets1 : kCrBuckets; }
    static constexpr uint32_t sub_hists(int pass) { return pass == 1 ? 4u : 1u; }  // 64 KiB of LDS either way
    static constexpr uint32_t hist_at(int pass) { return pass == 1 ? 0u : kCrH2; }
    static __device__ __forceinline__ uint32_t key_max(const Batch::Frame&) { return 0u; }
    static __device__ __forceinline__ uint32_t first_shift(uint32_t) { return kCrMantissa; }
    static __device__ __forceinline__ uint32_t next_shift(int, uint32_t shift) { return shift - kCrDigit; }  // 52, 39, 26, 13 -> 0

    struct Pixels {
        const uint32_t* count;
        const double* steps;
        __device__ __forceinline__ Pixels(const Batch::Frame& f, uint32_t) : count(f.count), steps(f.steps) {}
        template <typename Visit>
        __device__ __forceinline__ void quad(uint32_t i, bool in, Visit visit) const {
            const uint4 c = in ? ((const uint4*)count)[i] : make_uint4(0u, 0u, 0u, 0u);
            double2 a = make_double2(0., 0.), b = make_double2(0., 0.);
            if ((c.x | c.y | c.z | c.w) != 0u) {  // (four uncovered pixels: their steps are not read)
                a = ((const double2*)steps)[2u * i];
                b = ((const double2*)steps)[2u * i + 1u];
            }
            one(in, c.x, a.x, visit);
            one(in, c.y, a.y, visit);
            one(in, c.z, b.x, visit);
            one(in, c.w, b.y, visit);
        }
        template <typename Visit>
        __device__ __forceinline__ void pixel(uint32_t p, bool in, Visit visit) const { one(in, in ? count[p] : 0u, in ? steps[p] : 0., visit); }
        template <typename Visit>
        __device__ __forceinline__ void one(bool in, uint32_t c, double v, Visit visit) const {
            visit(in && c != 0u && v == v, f64_sortable(v));  // the population: covered, steps not NaN
        }
    };

    // the record of a frame whose two keys are pinned (or that has no population), exactly as include/sar.h states it
    static __device__ __forceinline__ void record(const Batch&, const Batch::Frame& f, const SelectState<Key>& st) {
        sar_color_range r;
        r.lo = st.n ? sortable_f64(st.prefix[0]) : 0.;
        r.hi = st.n ? sortable_f64(st.prefix[1]) : 0.;
        r.pos_lo = f.pos[0];
        r.pos_hi = f.pos[1];
        r.covered = st.n;
        const double span = r.hi - r.lo;
        r.applied = (st.n != 0u && isfinite(r.lo) && isfinite(r.hi) && span > 0. && span <= 1.7976931348623157e308) ? 1 : 0;
        *f.rec = r;
    }
};

// ---------------------------------------------------------------------------------------------------
// the select
// ---------------------------------------------------------------------------------------------------
// Pass 1: every member's first digit into one histogram; later: the next digit of the members under either prefix into that
// quantile's histogram. LDS: sub_hists copies (one per wave, or one for the workgroup) of the pass's histogram(s); only non-zero
// buckets go to global memory.
template <typename T, int PASS>
__global__ void __launch_bounds__(256) k_select_hist(const typename T::Batch t, uint32_t npix) {
    typedef typename T::Key Key;
    constexpr uint32_t NB = T::buckets(PASS);
    constexpr uint32_t NQ = PASS == 1 ? 1u : 2u;
    constexpr uint32_t NSUB = T::sub_hists(PASS);
    __shared__ uint32_t s_h[NSUB * NQ * NB];
    const typename T::Batch::Frame& f = t.f[blockIdx.y];
    uint32_t M, s_prev = 0u, s_next;
    Key pre0 = 0, pre1 = 0;
    if (PASS == 1) {
        M = T::key_max(f);
        s_next = T::first_shift(M);
    } else {
        const SelectState<Key>* st = (const SelectState<Key>*)(f.hist + T::kHistWords);
        if (st->done) return;  // (the whole workgroup: one state)
        M = st->max;
        s_prev = st->shift;
        s_next = T::next_shift(PASS, s_prev);
        pre0 = st->prefix[0];
        pre1 = st->prefix[1];
    }
    const uint32_t mask = PASS == 1 ? 0xFFFFFFFFu : (1u << (s_prev - s_next)) - 1u;  // (a digit: s_prev - s_next <= 13)
    for (uint32_t k = threadIdx.x; k < NSUB * NQ * NB; k += blockDim.x) s_h[k] = 0u;
    __syncthreads();
    uint32_t* sub = s_h + (NSUB == 1u ? 0u : (threadIdx.x >> 6) * NQ * NB);
    const typename T::Pixels px(f, M);
    auto visit = [&](bool member, Key key) {
        if (PASS == 1) {
            wave_hist_add(sub, member, (uint32_t)(key >> s_next));
        } else {
            const uint32_t b = (uint32_t)(key >> s_next) & mask;
            const Key pre = key >> s_prev;
            wave_hist_add(sub, member && pre == pre0, b);
            wave_hist_add(sub, member && pre == pre1, NB + b);
        }
    };
    const uint32_t quads = npix / 4u;
    for (uint32_t i0 = blockIdx.x * blockDim.x; i0 < quads; i0 += gridDim.x * blockDim.x) {  // (uniform trip count: whole waves)
        const uint32_t i = i0 + threadIdx.x;
        px.quad(i, i < quads, visit);
    }
    if (blockIdx.x == 0 && threadIdx.x < 64u) {  // the last npix % 4 pixels: wave 0 of workgroup 0
        const uint32_t p = quads * 4u + threadIdx.x;
        px.pixel(p, p < npix, visit);
    }
    __syncthreads();
    uint32_t* gh = f.hist + T::hist_at(PASS);
    for (uint32_t k = threadIdx.x; k < NQ * NB; k += blockDim.x) {
        uint32_t s = 0;
#pragma unroll
        for (uint32_t w = 0; w < NSUB; ++w) s += s_h[w * NQ * NB + k];
        if (s) atomicAdd(&gh[k], s);
    }
}

// ONE workgroup of 256 per frame: finds each quantile's bucket in the histogram of pass PASS (pass 1 counts the members and ranks
// the quantiles first), narrows prefix and rank down, clears the histogram it read; once nothing is left to resolve, writes the record
template <typename T, int PASS>
__global__ void __launch_bounds__(256) k_select_scan(const typename T::Batch t) {
    typedef typename T::Key Key;
    constexpr uint32_t NB = T::buckets(PASS);
    constexpr uint32_t PER = NB / 256u;
    const typename T::Batch::Frame& f = t.f[blockIdx.y];
    SelectState<Key>* gst = (SelectState<Key>*)(f.hist + T::kHistWords);
    uint32_t* h = f.hist + T::hist_at(PASS);
    __shared__ uint32_t s_wave[17];
    __shared__ uint32_t s_n;
    __shared__ uint32_t s_found[2][2];  // [q]: bucket, members below it
    __shared__ SelectState<Key> st;
    if (threadIdx.x == 0) {
        if (PASS == 1) {
            st.n = 0u;
            st.max = T::key_max(f);
            st.shift = 0u;
            st.done = 0u;
            st.prefix[0] = st.prefix[1] = 0;
            st.rank[0] = st.rank[1] = 0u;
        } else {
            st = *gst;
        }
    }
    __syncthreads();
    if (st.done) return;  // (the later passes did not write their histograms: nothing to clear)
    const uint32_t s_next = PASS == 1 ? T::first_shift(st.max) : T::next_shift(PASS, st.shift);
    for (uint32_t q = 0; q < 2u; ++q) {
        const uint32_t* hq = h + (PASS == 1 ? 0u : q * NB);
        uint32_t sum = 0;
        for (uint32_t j = 0; j < PER; ++j) sum += hq[threadIdx.x * PER + j];
        const uint32_t excl = block_exclusive_sum(sum, s_wave);
        if (PASS == 1 && q == 0u) {
            if (threadIdx.x == blockDim.x - 1u) s_n = excl + sum;
            __syncthreads();
            if (threadIdx.x == 0) {
                st.n = s_n;
                for (uint32_t k = 0; k < 2u; ++k) st.rank[k] = select_rank(f.q[k], st.n);
            }
            __syncthreads();
            if (st.n == 0u) break;
        }
        const uint32_t r = st.rank[q];
        if (r >= excl && r - excl < sum) {  // exactly one thread holds the bucket of rank r
            uint32_t below = excl, b = threadIdx.x * PER;
            for (const uint32_t end = b + PER - 1u; b < end; ++b) {  // (never beyond the thread's own buckets)
                const uint32_t c = hq[b];
                if (r - below < c) break;
                below += c;
            }
            s_found[q][0] = b;
            s_found[q][1] = below;
        }
        __syncthreads();  // (also: every thread has read hq before anybody clears it)
    }
    if (threadIdx.x == 0) {
        if (st.n != 0u) {
            for (uint32_t q = 0; q < 2u; ++q) {
                st.prefix[q] = (PASS == 1 ? (Key)0 : st.prefix[q] << (st.shift - s_next)) | (Key)s_found[q][0];
                st.rank[q] -= s_found[q][1];
            }
        }
        st.shift = s_next;
        st.done = (st.n == 0u || s_next == 0u) ? 1u : 0u;
        *gst = st;
        if (st.done) T::record(t, f, st);
    }
    for (uint32_t k = threadIdx.x; k < (PASS == 1 ? 1u : 2u) * NB; k += blockDim.x) h[k] = 0u;
}

template <typename T, int PASS>
static void launch_select_pass(const typename T::Batch& t, uint32_t n_frames, uint32_t npix, hipStream_t s) {
    // (up to 64 KiB of LDS per workgroup: two per CU; every lane visits four pixels per step)
    hipLaunchKernelGGL((k_select_hist<T, PASS>), dim3(grid_for(npix / 4u + 1u, 256, 512), n_frames), dim3(256), 0, s, t, npix);
    hipLaunchKernelGGL((k_select_scan<T, PASS>), dim3(1, n_frames), dim3(256), 0, s, t);
}

// the six launches of an exposure: three histogram passes, each followed by its scan (a pass after which nothing is left to resolve
// — M < 4096 after pass 1, M < 2^24 after pass 2, or no covered pixel — solves, and leaves the later ones nothing to do)
void launch_exposure(const ExpoBatch& t, uint32_t n_frames, uint32_t npix, hipStream_t s) {
    launch_select_pass<ExpoSelect, 1>(t, n_frames, npix, s);
    launch_select_pass<ExpoSelect, 2>(t, n_frames, npix, s);
    launch_select_pass<ExpoSelect, 3>(t, n_frames, npix, s);
}

// the ten launches of a colour range: five histogram passes (12 + 4 x 13 bits), each followed by its scan (the last writes the record)
void launch_color_range(const CrBatch& t, uint32_t n_frames, uint32_t npix, hipStream_t s) {
    launch_select_pass<CrSelect, 1>(t, n_frames, npix, s);
    for (uint32_t pass = 1; pass < kCrPasses; ++pass) launch_select_pass<CrSelect, 2>(t, n_frames, npix, s);
}

}  // namespace sar
