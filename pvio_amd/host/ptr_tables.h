// ptr_tables.h -- the pointer-keyed open-addressing tables of the host adapter (bundle_adjustor.cpp).  No pvio type and no Eigen in here:
// tests/host/ptr_tables_check.cpp holds this header alone, under the address and undefined-behaviour sanitizers.
//
// Why not std::unordered_map / unordered_set: they cost a node allocation per insert and a pointer chase per probe, which made the
// flattening as expensive as the upload it feeds (measured 225 us for 10 x 300).
#pragma once
#include "host_namespace.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>

namespace pvio {

inline size_t ptr_hash(const void *p) {
    uint64_t x = (uint64_t)(uintptr_t)p;
    x ^= x >> 17, x *= 0x9E3779B97F4A7C15ull, x ^= x >> 29;
    return (size_t)x;
}

// pointer -> int, fixed size, no allocation: the frames of a window (at most PVIO_MAX_FRAMES = 32 of them in kSlots = 256 slots).  The
// probes end at an empty slot, so the table must never fill up: put() refuses a NEW key once half of the slots are taken
// (std::length_error; the BundleAdjustor methods report any std::exception as "not usable").
template <class T, size_t kSlots = 256>
class PtrIndex {
    static_assert(kSlots >= 2 && (kSlots & (kSlots - 1)) == 0, "the probe sequence masks with kSlots - 1");

  public:
    static constexpr size_t kMaxKeys = kSlots / 2;
    void clear() {
        for (auto &k : key_) k = nullptr;
        used_ = 0;
    }
    void put(const T *p, int idx) {
        size_t h = ptr_hash(p) & (kSlots - 1);
        while (key_[h] && key_[h] != p) h = (h + 1) & (kSlots - 1);
        if (!key_[h]) {
            if (used_ == kMaxKeys) throw std::length_error("pointer table is full");
            ++used_;
        }
        key_[h] = p, val_[h] = idx;
    }
    int find(const T *p) const { // -1 when p was never put
        size_t h = ptr_hash(p) & (kSlots - 1);
        while (key_[h]) {
            if (key_[h] == p) return val_[h];
            h = (h + 1) & (kSlots - 1);
        }
        return -1;
    }

  private:
    const T *key_[kSlots] = {};
    int val_[kSlots] = {};
    size_t used_ = 0;
};

class PtrSet {
  public:
    void reset(size_t expected) {
        size_t n = 64;
        while (n < 2 * expected + 16) n <<= 1;
        if (slots_.size() != n) slots_.assign(n, nullptr);
        else std::fill(slots_.begin(), slots_.end(), nullptr);
        used_ = 0;
    }
    bool insert(const void *p) { // true when p was not in the set
        if (2 * (used_ + 1) > slots_.size()) grow();
        const size_t mask = slots_.size() - 1;
        size_t h = ptr_hash(p) & mask;
        while (slots_[h]) {
            if (slots_[h] == p) return false;
            h = (h + 1) & mask;
        }
        slots_[h] = p, ++used_;
        return true;
    }
    bool contains(const void *p) const {
        const size_t mask = slots_.size() - 1;
        size_t h = ptr_hash(p) & mask;
        while (slots_[h]) {
            if (slots_[h] == p) return true;
            h = (h + 1) & mask;
        }
        return false;
    }

  private:
    void grow() {
        std::vector<const void *> old;
        old.swap(slots_);
        slots_.assign(old.size() * 2, nullptr);
        used_ = 0;
        for (const void *p : old)
            if (p) insert(p);
    }
    std::vector<const void *> slots_ = std::vector<const void *>(64, nullptr);
    size_t used_ = 0;
};

// ---- incremental flattening -------------------------------------------------------------
// From one keyframe solve to the next almost every track is the track it was, plus one observation.  Walking its
// std::map of observations again (pointer chasing through the reference's object graph: 215 us of a 1.1 ms keyframe solve
// at 10 x 1000) is replaced by a per-track cache of the flattened list -- (frame id, keypoint) of every non-anchor
// observation, in ascending frame id -- validated by a signature that every way the reference changes a track alters:
// (track id, number of keypoints, first frame id, last frame id).  Unchanged: the list is replayed.  Grown by exactly the newest
// observation: that one is appended.  Anything else: rebuilt.  No hooks in the reference's map layer are needed; the output is identical to a
// walk from scratch (PVIO_HIP_FLATTEN_VERIFY=1 re-walks every window and compares; the headless tests run with it).
//
// The cache sees a track through numbers only: its address (the key), its signature, and a `View` the caller defines
// (resolved at compile time: this is the flattening's inner loop) --
//     size_t id_before_last() const;                      frame id of the observation before the newest; asked only when the track has
//                                                         exactly one keypoint more than its cached list accounts for
//     template <class Put> void newest(Put &&put) const;  put(frame id, z0, z1) of the newest observation
//     template <class Put> void each(Put &&put) const;    ... of every non-anchor observation, in ascending frame id
class ObsCache {
  public:
    struct Signature {
        size_t id, nkp, first_id, last_id;
    };
    enum Outcome { kUnchanged, kGrown, kRebuilt };

    // Brings the list of `key` up to date, then replays it against the window: emit(w, z0, z1) for every cached observation whose frame
    // id is win_id[w], in the list's order; observations of frames outside the window are skipped.  Both the list's and the window's
    // frame ids are ascending, so this is one merge.
    template <class View, class Emit>
    Outcome replay(const void *key, const Signature &sig, const View &view, const size_t *win_id, int n_win, Emit &&emit) {
        Outcome outcome;
        const Entry &e = *update(key, sig, view, outcome);
        int w = 0;
        for (uint32_t k = 0; k < e.cnt; ++k) {
            const size_t fid = fid_[e.off + k];
            while (w < n_win && win_id[w] < fid) ++w;
            if (w < n_win && win_id[w] == fid) emit(w, z_[2 * (size_t)(e.off + k)], z_[2 * (size_t)(e.off + k) + 1]);
        }
        return outcome;
    }
    // lists are append-only between resets; dead lists are dropped wholesale once they outweigh the live ones
    void begin_window(size_t live_obs_estimate) {
        if (fid_.size() > 8 * live_obs_estimate + 65536) clear();
    }
    void clear() {
        slots_.clear(), fid_.clear(), z_.clear(), used_ = 0;
    }
    size_t stored() const { return fid_.size(); } // observations in the store, dead lists included
    size_t tracks() const { return used_; }

  private:
    struct Entry {
        const void *key = nullptr;
        Signature sig = {0, 0, 0, 0};
        uint32_t off = 0, cnt = 0;
    };
    template <class View>
    Entry *update(const void *key, const Signature &sig, const View &view, Outcome &outcome) {
        Entry *e = find(key);
        const bool same_track = e && e->sig.id == sig.id && e->sig.first_id == sig.first_id;
        outcome = kUnchanged;
        if (same_track && e->sig.nkp == sig.nkp && e->sig.last_id == sig.last_id) return e;
        auto put = [this](size_t fid, double z0, double z1) { fid_.push_back(fid), z_.push_back(z0), z_.push_back(z1); };
        if (same_track && e->sig.nkp + 1 == sig.nkp && sig.nkp >= 2 && view.id_before_last() == e->sig.last_id) {
            // grown by its newest observation: the list moves to the end of the store with the new entry behind it
            // (by index: the push_backs may reallocate the vectors they read from)
            const uint32_t off = (uint32_t)fid_.size();
            for (uint32_t k = 0; k < e->cnt; ++k) {
                const size_t src = e->off + k;
                put(fid_[src], z_[2 * src], z_[2 * src + 1]); // by value
            }
            view.newest(put);
            e->off = off, e->cnt += 1, e->sig = sig;
            outcome = kGrown;
            return e;
        }
        e = insert(key);
        e->sig = sig, e->off = (uint32_t)fid_.size();
        view.each(put);
        e->cnt = (uint32_t)(fid_.size() - e->off);
        outcome = kRebuilt;
        return e;
    }
    Entry *find(const void *key) {
        if (slots_.empty()) return nullptr;
        const size_t mask = slots_.size() - 1;
        for (size_t h = ptr_hash(key) & mask;; h = (h + 1) & mask) {
            if (!slots_[h].key) return nullptr;
            if (slots_[h].key == key) return &slots_[h];
        }
    }
    Entry *insert(const void *key) {
        if (2 * (used_ + 1) > slots_.size()) rehash(std::max<size_t>(256, 4 * (used_ + 1)));
        const size_t mask = slots_.size() - 1;
        size_t h = ptr_hash(key) & mask;
        while (slots_[h].key && slots_[h].key != key) h = (h + 1) & mask;
        if (!slots_[h].key) ++used_;
        slots_[h].key = key;
        return &slots_[h];
    }
    void rehash(size_t n) {
        size_t cap = 256;
        while (cap < n) cap <<= 1;
        std::vector<Entry> old;
        old.swap(slots_);
        slots_.assign(cap, Entry());
        used_ = 0;
        for (const Entry &e : old)
            if (e.key) *insert(e.key) = e;
    }
    std::vector<Entry> slots_;
    std::vector<size_t> fid_; // frame id per cached observation
    std::vector<double> z_;   // 2 per cached observation
    size_t used_ = 0;
};

} // namespace pvio
