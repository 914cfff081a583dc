// sar_options.cpp — every option name of sar_runtime_set_option (include/sar.h) and of sar_runtime_set_test_option
// (include/sar_test_hooks.h) through its entry point, on a runtime object that never saw a device: the default constructor and the
// destructor of sar_runtime make no HIP call, and neither does an option on a runtime without buffers.
//
// Every name gets 0, both sides of every boundary of its rule (the values listed with it: n - 1, n, n + 1 around every member of a
// "one of" set and every cap) and 2^32 + 1, which tells a rule that reads the 64-bit value from one that reads its low 32 bits. Every
// name also goes once through the OTHER entry point, and each entry point gets one name nobody knows. One line per call: entry point,
// name, value, status, sar_last_error (set to "unknown test option '-'" before the call, so a call that leaves no text reads that).
//
// Built against the hooks build (tests/test_options_host.py); tests/golden/option_replies.json records its output.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../include/sar_test_hooks.h"
#include "../../strange_attractor_renderer_amd/csrc/sar_runtime_impl.hpp"

namespace {

constexpr uint64_t P32 = 1ull << 32;
struct Case {
    const char* name;
    std::vector<uint64_t> values;  // (0 and 2^32 + 1 go to every name)
};
const std::vector<uint64_t> K30 = {(1ull << 30) - 1, 1ull << 30, (1ull << 30) + 1}, K16 = {65535, 65536, 65537};
const Case PRODUCT[] = {
    {"block_threads", {1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320}},
    {"checkpoint_stride", {1, P32 - 1, P32}},
    {"hint_bits", {1, 15, 16, 17, 31, 32, 33}},
    {"split_waves", {1, 2, 3}},
    {"search_chunk", K30}, {"plane_chunk", K30}, {"gallery_chunk", K16}, {"orbit_chunk", K16}, {"corr_chunk", K30},
    {"box_chunk", {65534, 65535, 65536}},
    {"box_slots", {1, 2, 3, 4, (1ull << 24) - 1, 1ull << 24, (1ull << 24) + 1, 1ull << 25, P32}},
    {"basin_chunk", K30}, {"period_chunk", K30}, {"cycles_chunk", K30},
    {"density_tile", {7, 8, 9, 15, 16, 17, 31, 32, 33}},
    {"tail_overlap", {1, 2}},
    {"timing_accumulate", {1, 2}},
};
const Case HOOKS[] = {
    {"debug_throw", {1, 2, 3, 4}},
    {"path", {1, 2, 3, 4}},
    {"bin_shift", {1, 11, 12, 13, 15, 16, 17}},
    {"bin_interleave", {1, 2, 3}},
    {"splits", {1, 15, 16, 17}},
    {"chunk_records", {11, 12, 13, 19, 20, 21, 27, 28, 29, 59, 60, 61}},
    {"depth_park", {1, 2, 3, 4, 5, 7, 8, 9}},
    {"hint_tile", {1, 2}},
    {"acc_lists", {1, 2, 3, 4, 5}},
    {"hint_shared", {1, 2, 3}},
    {"readback_inline", {1, 2}},
    {"batch_starts", {2, 3, 4}},
    {"batch_warm", {1, 2, 3}},
    {"batch_chain", {1, 2}},
    {"batch_xcd", {1, 2}},
    {"chunk_ahead", {1, 2, 3}},
    {"acc_threads", {255, 256, 257, 511, 512, 513, 1023, 1024, 1025}},
    {"corr_replicas", {1, 2, 3, 4, 16, 31, 32, 33, 64}},
    {"debug_chunk_jobs", {1, P32 - 1, P32}},
    {"debug_max_ordinals", {1, P32 - 3, P32 - 2, P32 - 1, P32}},
};

typedef int (*Entry)(sar_runtime*, const char*, uint64_t);

sar_runtime g_scratch;  // (the sentinel text needs a runtime; a call under test may have none)

void call(const char* entry_name, Entry entry, sar_runtime* rt, const char* name, uint64_t value) {
    sar_runtime_set_test_option(&g_scratch, "-", 0);
    const int status = entry(rt, name, value);
    std::printf("%s\t%s\t%" PRIu64 "\t%d\t%s\n", entry_name, name ? name : "(null)", value, status, sar_last_error());
}

}  // namespace

int main() {
    sar_runtime rt;
    for (const Case& c : PRODUCT) {
        call("option", sar_runtime_set_option, &rt, c.name, 0);
        for (uint64_t v : c.values) call("option", sar_runtime_set_option, &rt, c.name, v);
        call("option", sar_runtime_set_option, &rt, c.name, P32 + 1);
        call("test_option", sar_runtime_set_test_option, &rt, c.name, 1);
    }
    for (const Case& c : HOOKS) {
        call("test_option", sar_runtime_set_test_option, &rt, c.name, 0);
        for (uint64_t v : c.values) call("test_option", sar_runtime_set_test_option, &rt, c.name, v);
        call("test_option", sar_runtime_set_test_option, &rt, c.name, P32 + 1);
        call("option", sar_runtime_set_option, &rt, c.name, 1);
    }
    call("option", sar_runtime_set_option, &rt, "no_such_option", 1);
    call("test_option", sar_runtime_set_test_option, &rt, "no_such_option", 1);
    call("option", sar_runtime_set_option, nullptr, "block_threads", 64);
    call("test_option", sar_runtime_set_test_option, nullptr, "path", 1);
    call("test_option", sar_runtime_set_test_option, nullptr, "debug_throw", 2);
    call("option", sar_runtime_set_option, &rt, nullptr, 1);
    call("test_option", sar_runtime_set_test_option, &rt, nullptr, 1);
    return 0;
}
