// sar_period.hpp — what the two halves of the period planes share (include/sar.h: sar_period_*, sar_runtime_period,
// sar_runtime_period_colorize): the argument block of the kernels of sar_period.hip and their launch wrappers, called from
// sar_period.cpp. The plane itself is the Lyapunov planes' (PlaneArgs, plane_sweep / plane_pick: sar_search.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include "sar_internal.hpp"
#include "sar_search.hpp"

namespace sar {

constexpr uint32_t kDefaultPeriodChunk = 1u << 20;  // pixels per launch (whole tiles): keeps one dispatch short
constexpr uint32_t kMaxPeriodChunk = 1u << 30;

struct PeriodArgs {
    PlaneArgs plane;              // the plane, the tiles of this launch, start, bound, transient; steps = max_period, records unused
    double eps;                   // a return is d <= eps
    const double* coeffs;         // the list form: the caller's [height][width][30], as given (the kernel canonicalises); else unused
    sar_period_record* records;   // [height][width]
};

// launch wrappers (sar_period.hip)
void launch_period(const PeriodArgs& a, bool list, hipStream_t s);
void launch_period_colorize(const sar_period_record* rec, uint32_t npix, const PaletteParams& pal, uint32_t colours, void* rgba16_out,
                            hipStream_t s);

}  // namespace sar
