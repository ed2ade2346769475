// pdehip_scratch.h — the per-stream scratch of the analysis kernels (pdehip_stats.hip, pdehip_project.hip, pdehip_smooth.hip,
// pdehip_hist.hip, pdehip_label.hip) and of the reductions of pdehip_ops.hip: ONE table from streams to entries, and the registry of
// what pdehip_release_scratch frees.  Calls on one stream are ordered, so they share the stream's entry; two streams working at the same
// time must not share one.  What an entry holds and how it grows is its user's business: the table is only the container.
#pragma once

#include <map>
#include <mutex>

#include "pdehip_common.h"

namespace pdehip {

// pdehip_comm.hip: pdehip_release_scratch calls every function added here and returns the first code that is not zero.  The list is a
// static of that function, so a table of any unit may add itself while the library's statics are still being initialised.
void register_scratch_release(int (*release)());

template <typename T>
class StreamTable {
public:
    StreamTable() = default;
    // a table whose entries pdehip_release_scratch frees: `release` calls release(free_entry) of this table
    explicit StreamTable(int (*release)()) { register_scratch_release(release); }

    // fn(entry of the stream) under the lock; an entry is value-initialised (all zeros) at the stream's first call
    template <class F>
    int with(hipStream_t st, F &&fn)
    {
        std::lock_guard<std::mutex> lock(mu_);
        return fn(entries_[st]);
    }
    // free_entry(entry) for every stream, then no entries
    template <class F>
    int release(F &&free_entry)
    {
        std::lock_guard<std::mutex> lock(mu_);
        for (auto &e : entries_) free_entry(e.second);
        entries_.clear();
        return 0;
    }

private:
    std::mutex mu_;
    std::map<hipStream_t, T> entries_;
};

}  // namespace pdehip
