// Extent bookkeeping of a resident bank (mocha_bank_resident_create): which units of a fixed range are free.  A unit is one granule of
// SEG_GRANULE_ROWS bank rows; a character occupies one extent of whole units.  Host only: no HIP, no allocation on the device, nothing
// but the standard library - tests/test_extent_alloc.py compiles this header alone with g++ under the sanitizers.
//
// The free extents are kept by first unit, never two of them adjacent (release() merges), so that
//   take(n)     is first fit - the lowest free extent of at least n units gives its first n - in one walk,
//   release()   finds both neighbours of the freed extent with one lookup,
//   largest()   is the largest request take() can still serve.
// No compaction: an extent never moves once taken.
#pragma once
#include <cstdint>
#include <iterator>
#include <map>

namespace mocha {

class ExtentAlloc {
public:
    // all `units` units free (units <= 0: an empty range, every take() fails)
    void reset(int64_t units) {
        free_.clear();
        units_ = units > 0 ? units : 0;
        nfree_ = units_;
        if (units_ > 0) free_[0] = units_;
    }
    // first unit of the lowest free extent of at least n units, which it leaves; -1 when there is none (or n < 1)
    int64_t take(int64_t n) {
        if (n < 1) return -1;
        for (auto it = free_.begin(); it != free_.end(); ++it) {
            if (it->second < n) continue;
            const int64_t first = it->first, rest = it->second - n;
            free_.erase(it);
            if (rest > 0) free_[first + n] = rest;
            nfree_ -= n;
            return first;
        }
        return -1;
    }
    // units [first, first + n) become free again and merge with free neighbours; false (and nothing changes) when the extent leaves the
    // range or overlaps units that are free already
    bool release(int64_t first, int64_t n) {
        if (n < 1 || first < 0 || first > units_ - n) return false;
        auto next = free_.lower_bound(first);                  // the first free extent at or behind `first`
        if (next != free_.end() && next->first < first + n) return false;
        int64_t lo = first, len = n;
        if (next != free_.begin()) {
            auto prev = std::prev(next);
            if (prev->first + prev->second > first) return false;
            if (prev->first + prev->second == first) { lo = prev->first; len += prev->second; free_.erase(prev); }
        }
        if (next != free_.end() && next->first == first + n) { len += next->second; free_.erase(next); }
        free_[lo] = len;
        nfree_ += n;
        return true;
    }
    int64_t units() const { return units_; }
    int64_t free_units() const { return nfree_; }
    int64_t largest() const {
        int64_t m = 0;
        for (const auto& e : free_) m = e.second > m ? e.second : m;
        return m;
    }

private:
    std::map<int64_t, int64_t> free_;          // first unit -> units
    int64_t units_ = 0, nfree_ = 0;
};

}  // namespace mocha
