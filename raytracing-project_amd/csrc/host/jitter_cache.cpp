// jitter_cache.cpp — see jitter_cache.hpp.  Host-only: no HIP.
#include "jitter_cache.hpp"

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <set>

namespace rtamd {

namespace {
std::atomic<long long> g_budget_override{-1};

size_t env_budget() {
    static const size_t v = [] {
        constexpr unsigned long long kDefaultMb = 2048, kMaxMb = 1ull << 24;   // (16 TiB: no overflow below)
        unsigned long long mb = kDefaultMb;
        if (const char* e = std::getenv("RT_JITTER_CACHE_MB"); e && *e) {
            char* end = nullptr;
            const unsigned long long x = std::strtoull(e, &end, 10);
            if (end != e && *end == 0 && *e != '-') mb = x < kMaxMb ? x : kMaxMb;   // (anything else: the default)
        }
        return (size_t)(mb << 20);
    }();
    return v;
}
}  // namespace

size_t jitter_cache_budget() {
    const long long o = g_budget_override.load(std::memory_order_relaxed);
    return o >= 0 ? (size_t)o : env_budget();
}

void set_jitter_cache_budget(long long bytes) { g_budget_override.store(bytes < 0 ? -1 : bytes, std::memory_order_relaxed); }

JitterCache::Got JitterCache::acquire(int W, int H, const std::vector<int32_t>& rows_jrow, size_t jit_bytes,
                                      size_t budget) {
    Got g;
    ++clock_;
    const size_t rows_off = rows_offset(jit_bytes);
    const size_t need = entry_bytes(jit_bytes, rows_jrow.size());
    if (budget > 0) {
        for (auto& up : entries_) {
            Entry& e = *up;
            if (e.W != W || e.H != H || e.rows_jrow != rows_jrow) continue;
            e.last_use = clock_;
            g.e = &e;
            g.fill = g.upload_rows = !e.valid;   // (invalid: its frame failed; this one writes it again)
            ++(e.valid ? hits_ : misses_);
            return g;
        }
    }
    ++misses_;
    if (budget > 0 && need <= budget) {
        while (!entries_.empty() && bytes_ + need > budget) {
            size_t lru = 0;
            for (size_t i = 1; i < entries_.size(); ++i)
                if (entries_[i]->last_use < entries_[lru]->last_use) lru = i;
            bytes_ -= entries_[lru]->bytes;
            free_(entries_[lru]->buf);
            entries_.erase(entries_.begin() + (std::ptrdiff_t)lru);
        }
        if (void* p = alloc_(need)) {
            entries_.emplace_back(new Entry);
            Entry& e = *entries_.back();
            e.W = W;
            e.H = H;
            e.rows_jrow = rows_jrow;
            e.buf = p;
            e.bytes = need;
            e.rows_off = rows_off;
            e.last_use = clock_;
            bytes_ += need;
            g.e = &e;
            return g;
        }
        clear();   // no memory for an entry: give all of them back, and fill the uncached buffer
    }
    Entry& s = scratch_;
    if (s.bytes < need) {
        if (s.buf) free_(s.buf);
        s = Entry();
        const size_t want = need + need / 8 + 256;   // (growth slack, as the workspace's other buffers)
        void* p = alloc_(want);
        if (!p && !entries_.empty()) {   // the entries' memory, before the frame fails
            clear();
            p = alloc_(want);
        }
        if (!p) return Got();
        s.buf = p;
        s.bytes = want;
    }
    if (!(s.valid && s.W == W && s.H == H && s.rows_jrow == rows_jrow)) {
        s.W = W;
        s.H = H;
        s.rows_jrow = rows_jrow;
        s.valid = false;
    }
    s.rows_off = rows_off;
    s.last_use = clock_;
    g.e = &s;
    g.upload_rows = !s.valid;
    return g;
}

int jitter_cache_sim(const int64_t* ops, int n_ops, int64_t budget, int64_t* out) {
    std::set<void*> live;
    int64_t fail_next = 0;
    bool bad_free = false, stale = false;
    {
        JitterCache cache(
            [&](size_t n) -> void* {
                if (fail_next > 0) {
                    --fail_next;
                    return nullptr;
                }
                void* p = std::malloc(n);
                if (p) live.insert(p);
                return p;
            },
            [&](void* p) {
                if (!live.erase(p)) {
                    bad_free = true;
                    return;
                }
                std::free(p);
            });
        for (int k = 0; k < n_ops; ++k) {
            const int64_t* o = ops + 5 * (size_t)k;
            const int64_t op = o[0], arg = o[4];
            const int W = (int)o[1], row0 = (int)o[2], n = (int)o[3], H = (int)arg;
            int64_t buffer = 0, fill = 0, upload = 0;
            if (op == 0 || op == 1) {
                std::vector<int32_t> key(2 * (size_t)n);
                for (int i = 0; i < n; ++i) {
                    key[i] = row0 + i;
                    key[n + i] = i;
                }
                const size_t n_draws = (size_t)n * 16 * W;
                const auto draw = [&](size_t i) { return (double)W * 1e9 + (double)H * 1e6 + (double)row0 * 1e3 + (double)i; };
                const JitterCache::Got g = cache.acquire(W, H, key, n_draws * sizeof(double), (size_t)budget);
                if (g.e) {
                    buffer = cache.is_cached(g.e) ? 1 : 2;
                    fill = g.fill;
                    upload = g.upload_rows;
                    if (!g.upload_rows)
                        for (size_t i = 0; i < key.size(); ++i) stale = stale || g.e->rows()[i] != key[i];
                    if (!g.fill)
                        for (size_t i = 0; i < n_draws; ++i) stale = stale || g.e->jit()[i] != draw(i);
                    if (g.upload_rows) std::copy(key.begin(), key.end(), g.e->rows());
                    if (g.fill)
                        for (size_t i = 0; i < n_draws; ++i) g.e->jit()[i] = draw(i);
                    if (op == 0) cache.complete(g.e);
                }
            } else if (op == 2) {
                cache.clear();
            } else if (op == 3) {
                fail_next = arg;
            } else if (op == 4) {
                budget = arg;
            } else if (op == 5) {
                cache.release();
            }
            int64_t* r = out + 8 * (size_t)k;
            r[0] = buffer;
            r[1] = fill;
            r[2] = upload;
            r[3] = (int64_t)cache.entries();
            r[4] = (int64_t)cache.bytes();
            r[5] = (int64_t)live.size();
            r[6] = (int64_t)cache.hits();
            r[7] = (int64_t)cache.misses();
        }
    }
    if (stale) return 1;
    return bad_free || !live.empty() ? 2 : 0;
}

void JitterCache::clear() {
    for (auto& e : entries_) free_(e->buf);
    entries_.clear();
    bytes_ = 0;
}

void JitterCache::release() {
    clear();
    if (scratch_.buf) free_(scratch_.buf);
    scratch_ = Entry();
}

}  // namespace rtamd
