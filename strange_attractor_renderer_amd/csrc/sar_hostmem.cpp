// sar_hostmem.cpp — sar_host_reserve, sar_host_alloc, sar_host_free.
// Page-locked host memory for the read-backs. hipHostMalloc page-locks 4 KiB page by 4 KiB page (1.0-1.4 ms per 21.6 MB image on
// most boxes of the pool, 3-4 on some: 33-100 ms of a sweep's set-up); an anonymous mapping that asks for transparent huge pages,
// touched once and then registered with the HIP runtime, is the same memory to a copy and takes 0.4 of the time (tools/ubench/
// alloc_cost.py: 352 MiB in 20 ms against 48-55). Large blocks go that way; what fails on the way falls back to hipHostMalloc.
#include <sys/mman.h>

#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

#include "sar_runtime_impl.hpp"

using namespace sar;

// (outside extern "C": an unnamed namespace inside it gives its variables C names with EXTERNAL linkage — two copies of this library in
// one process, the product and the test-suite's hooks build, loaded RTLD_GLOBAL, would share them, and construct and destroy them twice)
namespace {
struct MappedBlock { void* p; size_t bytes; };
std::mutex g_mapped_mu;
std::vector<MappedBlock> g_mapped;
constexpr size_t kHugePage = 2u << 20;

size_t mapped_len(size_t bytes) { return (bytes + kHugePage - 1) & ~(kHugePage - 1); }

// An anonymous mapping of len bytes on a 2 MiB boundary, asked to be huge pages, every page touched — no HIP call in here.
char* map_and_touch(size_t len) {
    // (over-map by one huge page so that the block can start on a 2 MiB boundary: only aligned ranges get huge pages)
    char* raw = static_cast<char*>(mmap(nullptr, len + kHugePage, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0));
    if (raw == MAP_FAILED) return nullptr;
    char* p = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(raw) + kHugePage - 1) & ~static_cast<uintptr_t>(kHugePage - 1));
    if (p > raw) munmap(raw, static_cast<size_t>(p - raw));
    if (p + len < raw + len + kHugePage) munmap(p + len, static_cast<size_t>(raw + len + kHugePage - (p + len)));
    madvise(p, len, MADV_HUGEPAGE);                       // (advice: refused or unavailable, the pages are small ones)
    for (size_t off = 0; off < len; off += 4096) p[off] = 0;  // first touch: the pages exist before they are locked
    return p;
}

// Blocks announced by sar_host_reserve: helper threads map and touch them ahead of their sar_host_alloc (zeroing fresh pages is
// nine tenths of what page-locking an image costs, and needs no HIP call: the helpers never contend for the HIP runtime's locks,
// which is what made page-locking itself on a helper thread slower — profiles/dead_ends.md, Round 6).
struct HostReserve {
    static constexpr int kHelpers = 3;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<char*> ready;   // mapped + touched, not registered
    size_t len = 0;            // their size (a multiple of 2 MiB)
    uint32_t pending = 0;      // blocks nobody has started on yet
    int working = 0;           // helper threads alive
    std::vector<std::thread> helpers;
    ~HostReserve() { drop(); }
    void drop() {
        std::unique_lock<std::mutex> lock(mu);
        pending = 0;
        cv.wait(lock, [&] { return working == 0; });
        for (char* p : ready) munmap(p, len);
        ready.clear();
        lock.unlock();
        for (std::thread& t : helpers)
            if (t.joinable()) t.join();
        helpers.clear();
    }
    void work(uint64_t generation_len) {
        std::unique_lock<std::mutex> lock(mu);
        while (pending) {
            --pending;
            lock.unlock();
            char* p = map_and_touch(generation_len);
            lock.lock();
            if (!p) { pending = 0; break; }
            ready.push_back(p);
            cv.notify_all();
        }
        --working;
        cv.notify_all();
    }
    // a touched block of `want` bytes, or nullptr (none announced: the caller maps its own)
    char* take(size_t want) {
        std::unique_lock<std::mutex> lock(mu);
        if (want != len) return nullptr;
        cv.wait(lock, [&] { return !ready.empty() || working == 0; });
        if (ready.empty()) return nullptr;
        char* p = ready.front();
        ready.pop_front();
        return p;
    }
} g_reserve;

void* map_and_register(size_t bytes) {
    const size_t len = mapped_len(bytes);
    char* p = g_reserve.take(len);
    if (!p) p = map_and_touch(len);
    if (!p) return nullptr;
    if (hipHostRegister(p, len, hipHostRegisterDefault) != hipSuccess) {
        (void)hipGetLastError();
        munmap(p, len);
        return nullptr;
    }
    std::lock_guard<std::mutex> lock(g_mapped_mu);
    g_mapped.push_back({p, len});
    return p;
}
}  // namespace

extern "C" {

int sar_host_reserve(size_t bytes, uint32_t count) try {
    static std::mutex one_at_a_time;                    // (announcements from several threads follow each other)
    std::lock_guard<std::mutex> serial(one_at_a_time);
    g_reserve.drop();                                   // what an earlier announcement left goes first (its helpers have ended)
    if (bytes < (4u << 20) || count == 0) return SAR_OK;  // (smaller blocks are hipHostMalloc'ed: nothing to prepare)
    if (count > 4096u) { set_error("sar_host_reserve: at most 4096 blocks"); return SAR_ERR_RANGE; }
    std::lock_guard<std::mutex> lock(g_reserve.mu);
    g_reserve.len = mapped_len(bytes);
    g_reserve.pending = count;
    const size_t len = g_reserve.len;
    const int n = count < static_cast<uint32_t>(HostReserve::kHelpers) ? static_cast<int>(count) : HostReserve::kHelpers;
    g_reserve.working = n;
    for (int i = 0; i < n; ++i) g_reserve.helpers.emplace_back([len] { g_reserve.work(len); });
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_host_alloc(size_t bytes, void** out) try {
    if (!out || bytes == 0) { set_error("sar_host_alloc: NULL output or zero size"); return SAR_ERR_INVALID; }
#ifndef SAR_EXPERIMENT_HOST_ALLOC_PLAIN  // (A/B timing only)
    if (bytes >= (4u << 20)) {
        *out = map_and_register(bytes);
        if (*out) return SAR_OK;
    }
#endif
    HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocDefault));
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_host_free(void* p) try {
    if (!p) return SAR_OK;
    size_t mapped = 0;
    {
        std::lock_guard<std::mutex> lock(g_mapped_mu);
        for (size_t k = 0; k < g_mapped.size(); ++k)
            if (g_mapped[k].p == p) { mapped = g_mapped[k].bytes; g_mapped.erase(g_mapped.begin() + static_cast<long>(k)); break; }
    }
    if (mapped) {
        HIP_TRY(hipHostUnregister(p));
        munmap(p, mapped);
        return SAR_OK;
    }
    HIP_TRY(hipHostFree(p));
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

}  // extern "C"
