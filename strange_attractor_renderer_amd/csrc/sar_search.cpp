// sar_search.cpp — the host half of the chaotic-map search (include/sar.h: sar_search_*, sar_runtime_search, sar_frame_view):
// candidate generation for the host, the chunked launches of k_search_screen / k_search_lyapunov (sar_search.hip), and the
// finish of the records — Lyapunov exponents, Kaplan-Yorke dimension, acceptance, statistics, ordering.
//
// Built with -ffp-contract=off: sar_search_candidate must produce the device's doubles.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "sar_analysis.hpp"
#include "sar_search.hpp"

using namespace sar;

namespace sar {

void lyapunov_finish(const int64_t* log2_exp, const double* mant, int k, uint32_t folded, double* lyapunov, double* ky_dim) {
    lyapunov[0] = lyapunov[1] = lyapunov[2] = *ky_dim = std::nan("");
    if (!folded) return;
    double l[3];
    for (int i = 0; i < k; ++i) l[i] = (static_cast<double>(log2_exp[i]) * 0.6931471805599453 + std::log(mant[i])) / folded;
    std::sort(l, l + k, [](double a, double b) { return a > b; });
    for (int i = 0; i < k; ++i) lyapunov[i] = l[i];
    if (k != 3) return;
    double sum = 0.;
    int j = 0;
    for (int i = 0; i < 3; ++i) {
        if (sum + l[i] < 0.) break;
        sum = sum + l[i];
        j = i + 1;
    }
    *ky_dim = j == 3 ? 3. : (j == 0 ? 0. : j + sum / std::fabs(l[j]));
}

}  // namespace sar

namespace {

// lambda_i from the raw accumulators, sorted descending; the Kaplan-Yorke dimension from them. A record without a folded step
// (steps == 0, or a failure at step 1) has neither: NaN.
void finish_record(sar_search_record& r) {
    const uint32_t folded = r.status == SAR_SEARCH_BOUNDED ? r.steps_done : r.steps_done - 1u;
    lyapunov_finish(r.log2_exp, r.mant, 3, folded, r.lyapunov, &r.ky_dim);
}

}  // namespace

extern "C" {

int sar_search_params_default(sar_search_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->seed = 0;
    out->lo = -1.2;
    out->hi = 1.2;
    out->start[0] = out->start[1] = out->start[2] = 0.05;
    out->transient = 1000;
    out->steps = 20000;
    out->bound = 1e6;
    out->min_lyapunov = 0.005;
    out->min_ky_dim = 0.;
    out->keep_rejected = 0;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_search_candidate(uint64_t seed, double lo, double hi, uint64_t index, double out30[30]) try {
    if (!out30) return SAR_ERR_INVALID;
    const double span = hi - lo;
    for (uint32_t j = 0; j < kSearchCoeffs; ++j) out30[j] = search_coeff(seed, lo, span, index, j);
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_search(sar_runtime* rt, const sar_search_params* p, uint64_t first, uint32_t n, const double* coeffs_host,
                       sar_search_record* out_host, uint32_t cap, uint32_t* n_out, sar_search_stats* stats_out) try {
    if (!p) return SAR_ERR_INVALID;
    // the parameters first (no device needed to refuse them)
    if (!(p->bound > 0.) || !std::isfinite(p->lo) || !std::isfinite(p->hi)) {
        set_error("sar_runtime_search: bound must be positive, lo and hi finite");
        return SAR_ERR_INVALID;
    }
    SAR_TRY(check_steps("sar_runtime_search", p->transient, p->steps));
    if (!rt || !n_out || (cap && !out_host)) return SAR_ERR_INVALID;
    SAR_TRY(analysis_begin(rt));  // with timing on: warmup_ms = k_search_screen, iterate_ms = k_search_lyapunov (sar_timing)
    const uint32_t chunk = rt->opt.search_chunk ? rt->opt.search_chunk : kDefaultSearchChunk;
    const uint32_t m = n < chunk ? n : chunk;  // scratch: one chunk
    sar_search_stats st;
    std::memset(&st, 0, sizeof(st));
    st.tested = n;
    std::vector<sar_search_record> kept, part;
    std::vector<double> coeffs;
    if (m) {
        HIP_TRY(rt->search.d_counters.grow(nullptr, 2));
        HIP_TRY(rt->search.d_idx.grow(nullptr, m));
        HIP_TRY(rt->search.d_xyz.grow(nullptr, static_cast<size_t>(m) * 3));
        if (coeffs_host) HIP_TRY(rt->search.d_coeffs.grow(nullptr, static_cast<size_t>(m) * kSearchCoeffs));
    }
    SearchArgs a;
    std::memset(&a, 0, sizeof(a));
    a.seed = p->seed;
    a.lo = p->lo;
    a.span = p->hi - p->lo;
    a.transient = p->transient;
    a.steps = p->steps;
    for (int k = 0; k < 3; ++k) a.start[k] = p->start[k];
    a.bound = p->bound;
    a.counters = rt->search.d_counters;
    a.surv_idx = rt->search.d_idx;
    a.surv_xyz = rt->search.d_xyz;
    for (uint64_t done = 0; done < n; done += m) {  // (64 bits: done + m passes 2^32 after the last chunk of a large n)
        a.first = first + done;
        a.n = static_cast<uint32_t>(n - done < m ? n - done : m);
        if (coeffs_host) {  // the caller's sets, canonicalised as sar_render treats its coefficients (-0.0 -> +0.0)
            const double* src = coeffs_host + static_cast<size_t>(done) * kSearchCoeffs;
            coeffs.resize(static_cast<size_t>(a.n) * kSearchCoeffs);
            canonical_coeffs(src, coeffs.size(), coeffs.data());
            HIP_TRY(hipMemcpyAsync(rt->search.d_coeffs, coeffs.data(), coeffs.size() * sizeof(double), hipMemcpyHostToDevice, rt->stream));
            a.coeffs = rt->search.d_coeffs;
        }
        uint32_t counters[2];
        HIP_TRY(hipMemsetAsync(rt->search.d_counters, 0, 2 * sizeof(uint32_t), rt->stream));
        SAR_TRY(timed_launch(rt, rt->tm.warm, [&] { launch_search_screen(a, rt->stream); }));
        HIP_TRY(hipMemcpyAsync(counters, rt->search.d_counters, sizeof(counters), hipMemcpyDeviceToHost, rt->stream));
        HIP_TRY(hipStreamSynchronize(rt->stream));  // once per chunk: sizes phase 2
        st.diverged_transient += counters[1];
        const uint32_t surv = counters[0];
        if (!surv) continue;
        HIP_TRY(rt->search.d_rec.grow(nullptr, surv));  // (the last phase 2 has been read back: nothing uses the old one)
        a.records = rt->search.d_rec;
        SAR_TRY(timed_launch(rt, rt->tm.iter, [&] { launch_search_lyapunov(a, surv, rt->stream); }));
        part.resize(surv);
        HIP_TRY(hipMemcpyAsync(part.data(), rt->search.d_rec, surv * sizeof(sar_search_record), hipMemcpyDeviceToHost, rt->stream));
        HIP_TRY(hipStreamSynchronize(rt->stream));
        for (sar_search_record& r : part) {
            finish_record(r);
            bool accepted = false;
            if (r.status == SAR_SEARCH_DIVERGED) ++st.diverged_late;
            else if (r.status == SAR_SEARCH_DEGENERATE) ++st.degenerate;
            else if (!(r.lyapunov[0] >= p->min_lyapunov)) ++st.below_lyapunov;
            else if (!(r.ky_dim >= p->min_ky_dim)) ++st.below_dim;
            else accepted = true, ++st.accepted;
            if (accepted || p->keep_rejected) kept.push_back(r);
        }
    }
    std::sort(kept.begin(), kept.end(), [](const sar_search_record& x, const sar_search_record& y) { return x.candidate < y.candidate; });
    const size_t w = std::min<size_t>(kept.size(), cap);
    if (w) std::memcpy(out_host, kept.data(), w * sizeof(sar_search_record));
    *n_out = static_cast<uint32_t>(kept.size());
    if (stats_out) *stats_out = st;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_frame_view(sar_config* cfg, const double screen_extent6[6], double margin, int sweep) try {
    if (!cfg || !screen_extent6 || !(margin >= 0. && margin < 1.)) return SAR_ERR_INVALID;
    const double* e = screen_extent6;
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(e[k])) {
            set_error("sar_frame_view: extent[%d] is not finite (a trajectory diverged?)", k);
            return SAR_ERR_INVALID;
        }
    const double mid_x = (e[0] + e[1]) * 0.5, mid_y = (e[2] + e[3]) * 0.5, mid_z = (e[4] + e[5]) * 0.5;
    const double range_z = e[5] - e[4], range_y = e[3] - e[2];
    double range_x = e[1] - e[0];
    if (sweep) range_x = std::sqrt(range_x * range_x + range_z * range_z);
    // i = (0.5 - x2 * scale) * width, j = height / 2 - (screen.y + cc.z) * width * scale (src/lib.rs:774-789): centred, the
    // image holds |x2| <= 1 / (2 scale) and |y| <= height / (2 width scale)
    const double s = (1. - margin) * std::min(1. / range_x, static_cast<double>(cfg->height) / (static_cast<double>(cfg->width) * range_y));
    if (!(s > 0. && s < HUGE_VAL) || !(range_x >= 0. && range_y >= 0.)) {
        set_error("sar_frame_view: the extent is empty or a single point");
        return SAR_ERR_INVALID;
    }
    cfg->center_camera[0] = -mid_x;  // with screen.x
    cfg->center_camera[1] = -mid_z;  // with screen.z (:776-779)
    cfg->center_camera[2] = -mid_y;  // with screen.y (:786)
    cfg->scale = s;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

}  // extern "C"
