// jitter_cache.hpp — which buffer holds a standard frame's jitter draws, as
// host-only logic (no HIP), in the style of frame_plan.hpp.
//
// The draws of a standard frame are a pure function of the frame size W x H
// and the frame's row list (StdPlan::rows_jrow: the reference seeds
// std::mt19937(12345) afresh for every render and consumes it in loop order,
// tracer.cpp:284-293, so output row r reads the stream at loop row H-1-r:
// the same rows of a frame of another height take other draws); scene,
// camera, lights, flags and recursion depth do not enter.  So a workspace
// keeps the filled buffers by that key, and a frame whose key is resident
// runs neither the fill nor the rows upload.
//
// One buffer per entry: [the draws, 16 doubles per pixel | rows_jrow].  The
// cache decides hit / miss / eviction and calls back for device memory; the
// caller (rt_frame.hip frame_begin / frame_end) enqueues the upload and the
// fill and reports the frame's completion.  Not thread-safe: used under the
// workspace lock, which a frame holds from begin to end, so at most one frame
// of a cache is open and its entry cannot be evicted (evictions happen in
// acquire only).  tests/test_jitter_cache.py drives it on the CPU through
// rt_test_jitter_cache_sim, tools/sanitize/host_check.cpp under ASan/UBSan.
#pragma once

#include <cstddef>
#include <cstdint>
#include <functional>
#include <memory>
#include <utility>
#include <vector>

namespace rtamd {

// The budget of one workspace's entries in bytes: RT_JITTER_CACHE_MB from the
// environment, read once (default 2048: the 4K frame's 1012.5 MiB and one
// more strip set, not an 8K frame's 4.2 GB; 0 = off, every frame fills the
// uncached buffer), unless set_jitter_cache_budget gave a value >= 0 (the
// test hook rt_test_jitter_cache_budget; < 0: back to the environment's).
size_t jitter_cache_budget();
void set_jitter_cache_budget(long long bytes);

class JitterCache {
public:
    struct Entry {
        int W = 0, H = 0;
        std::vector<int32_t> rows_jrow;   // with W and H, the key: compared whole, never hashed
        void* buf = nullptr;
        size_t bytes = 0;                 // of the allocation
        size_t rows_off = 0;              // byte offset of the rows list behind the draws
        uint64_t last_use = 0;
        // the buffer holds this key's rows list and (a cached entry) draws,
        // complete on the device: set by complete() only, i.e. after the
        // frame that wrote them has ended successfully
        bool valid = false;
        double* jit() const { return static_cast<double*>(buf); }
        int32_t* rows() const { return reinterpret_cast<int32_t*>(static_cast<char*>(buf) + rows_off); }
    };
    // What the frame does: e == nullptr: no memory (the frame fails).
    struct Got {
        Entry* e = nullptr;
        bool fill = true;          // generate the draws into e->jit()
        bool upload_rows = true;   // copy rows_jrow to e->rows()
    };
    using Alloc = std::function<void*(size_t)>;   // nullptr: failed
    using Free = std::function<void(void*)>;

    JitterCache(Alloc a, Free f) : alloc_(std::move(a)), free_(std::move(f)) {}
    ~JitterCache() { release(); }
    JitterCache(const JitterCache&) = delete;
    JitterCache& operator=(const JitterCache&) = delete;

    // The buffer of a frame of (W, H, rows_jrow) whose draws take jit_bytes.
    //  * resident and valid: a hit (no fill, no upload);
    //  * else a miss: the key's own entry if it exists (left invalid by a
    //    frame that failed), or a new one, after evicting least recently
    //    used entries until entries + the new one fit the budget;
    //  * a frame larger than the budget (or budget 0), or a failed entry
    //    allocation (which frees every entry first): the uncached buffer,
    //    grown when too small, filled every frame; only its rows list is
    //    reused by the next frame of the same key.
    Got acquire(int W, int H, const std::vector<int32_t>& rows_jrow, size_t jit_bytes, size_t budget);
    // The frame that acquired e has ended successfully (its work is complete).
    void complete(Entry* e) {
        if (e) e->valid = true;
    }
    void clear();     // free every cached entry (the uncached buffer stays)
    void release();   // free everything
    void reset_counts() { hits_ = misses_ = 0; }

    uint64_t hits() const { return hits_; }       // frames that ran no fill
    uint64_t misses() const { return misses_; }   // frames that ran it (cached or not)
    size_t entries() const { return entries_.size(); }
    size_t bytes() const { return bytes_; }       // of the cached entries (the uncached buffer is not counted)
    bool is_cached(const Entry* e) const { return e && e != &scratch_; }

    // bytes of an entry's buffer: the draws, padded to 256 B, and the list
    static size_t rows_offset(size_t jit_bytes) { return (jit_bytes + 255) & ~(size_t)255; }
    static size_t entry_bytes(size_t jit_bytes, size_t n_list) { return rows_offset(jit_bytes) + n_list * sizeof(int32_t); }

private:
    Alloc alloc_;
    Free free_;
    std::vector<std::unique_ptr<Entry>> entries_;   // (frames hold Entry pointers)
    Entry scratch_;                                 // the uncached buffer
    size_t bytes_ = 0;
    uint64_t clock_ = 0, hits_ = 0, misses_ = 0;
};

// Test support (rt_test_jitter_cache_sim, tools/sanitize/host_check.cpp): a
// JitterCache over host memory driven by a script.  ops[5k ..] = {op, W,
// row0, n_rows, arg}:
//   0  a frame of width W and height `arg` over rows [row0, row0 + n_rows)
//      that ends well (acquire, write what Got asks for, complete)
//   1  the same frame, abandoned after its writes (no complete)
//   2  clear()
//   3  the next `arg` allocations fail
//   4  the budget is `arg` bytes from here on
//   5  release()
// out[8k ..] = {buffer: 0 none, 1 a cached entry, 2 the uncached one; fill;
// upload_rows; entries; bytes; live allocations; hits; misses} after op k.
// A frame checks first that a buffer it neither fills nor uploads to still
// holds its key's contents.  Returns 0; 1: such a buffer held something
// else; 2: allocations left after the final release, or a pointer freed that
// was not live.
int jitter_cache_sim(const int64_t* ops, int n_ops, int64_t budget, int64_t* out);

}  // namespace rtamd
