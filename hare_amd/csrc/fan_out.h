// fan_out.h -- what the host-buffer batch calls share (api.cpp, bounce.cpp): the split of n rays into parts, the fan-out of the parts over
// host threads, the check of a scene array and the counters sum; and the exception guard of every C-ABI call.  Host only: no HIP header,
// no HIP type.  A persistent worker per scene, in place of a thread per part, would replace fan_out's body and nothing else.
// Product code; nothing from oracle/.
#pragma once
#include <stdint.h>
#include <new>
#include <string>
#include <thread>

#include "../../include/hare_hip.h"

// the body of a C-ABI call between these two lets no exception out
#define GUARD_BEGIN try {
#define GUARD_END                                               \
    }                                                           \
    catch (const std::bad_alloc&)                               \
    {                                                           \
        set_error("out of host memory");                        \
        return HARE_E_NOMEM;                                    \
    }                                                           \
    catch (...)                                                 \
    {                                                           \
        set_error("unexpected C++ exception");                  \
        return HARE_E_INVALID;                                  \
    }

namespace hare {

void set_error(const std::string& msg);      // the thread-local message (device_scene.cpp)
const char* last_error();

// part k of `parts` of [0, n): [lo, hi).  The parts tile the range, sizes differ by one at most; no overflow for any n >= 0
struct PartRange {
    int64_t lo, hi;
    int64_t size() const { return hi - lo; }
};
inline PartRange part_range(int64_t n, int64_t k, int64_t parts)
{
    return {(int64_t)((__int128)n * k / parts), (int64_t)((__int128)n * (k + 1) / parts)};
}

constexpr int kMaxParts = 64;
// the first part that failed: its index, its code and the message it left (rc == HARE_OK: none failed).  Whether the text is wrapped
// as "shard k: ..." is the caller's choice
struct FanResult {
    int part = 0;
    int rc = HARE_OK;
    std::string text;
    std::string shard_text() const { return "shard " + std::to_string(part) + ": " + text; }
};

// Runs task(k) -> code for k = 1 .. parts - 1 on a thread each and task(0) on the caller's, and joins them all on every path.  A part for
// which no thread can be had runs here.  Whatever a part throws becomes HARE_E_NOMEM with the message `thrown`; a failed part's thread-local
// message is carried to the caller's thread.  1 <= parts <= kMaxParts
template <class Task>
FanResult fan_out(int parts, const char* thrown, Task&& task)
{
    FanResult res;
    if (parts < 1 || parts > kMaxParts) {
        res.rc = HARE_E_INVALID;
        res.text = "fan_out: need 1..64 parts";
        return res;
    }
    int rcs[kMaxParts];
    std::string errs[kMaxParts];
    auto run = [&](int k) noexcept {
        try {
            try {
                rcs[k] = task(k);
            } catch (...) {
                rcs[k] = HARE_E_NOMEM;
                set_error(thrown);
            }
            if (rcs[k] != HARE_OK) errs[k] = last_error();
        } catch (...) {      // not even the message could be had
            rcs[k] = HARE_E_NOMEM;
        }
    };
    {
        struct Workers {
            std::thread t[kMaxParts];
            ~Workers() { for (std::thread& x : t) if (x.joinable()) x.join(); }      // a started thread is never left unjoined
        } workers;
        for (int k = 1; k < parts; ++k) {
            try {
                workers.t[k] = std::thread(run, k);
            } catch (...) {
                run(k);
            }
        }
        run(0);
    }
    for (int k = 0; k < parts; ++k)
        if (rcs[k] != HARE_OK) {
            res.part = k;
            res.rc = rcs[k];
            res.text = errs[k];
            break;
        }
    return res;
}

// the scene array of a sharded call
inline int check_scenes(const char* who, hare_scene* const* scenes, int32_t n_scenes, bool bare_null = false)
{
    if (!scenes || n_scenes < 1 || n_scenes > 64) {
        set_error(std::string(who) + ": need 1..64 scenes");
        return HARE_E_INVALID;
    }
    for (int32_t k = 0; k < n_scenes; ++k)
        if (!scenes[k]) {
            set_error(bare_null ? std::string("null scene") : std::string(who) + ": null scene");
            return HARE_E_INVALID;
        }
    return HARE_OK;
}

// every word: the reserved ones hold the developer counters (HARE_SHOOT_COUNT_OWN, the cull audit), which are sums too
inline void add_counters(hare_counters& dst, const hare_counters& src)
{
    dst.rays += src.rays;
    dst.hits += src.hits;
    dst.cells += src.cells;
    dst.entries += src.entries;
    dst.tests += src.tests;
    for (int w = 0; w < 3; ++w) dst.reserved[w] += src.reserved[w];
}

}  // namespace hare
