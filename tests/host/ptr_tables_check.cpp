// ptr_tables_check.cpp -- pvio_amd/host/ptr_tables.h alone: the pointer-keyed tables of the host adapter and the observation cache's protocol,
// built with -fsanitize=address,undefined (Makefile: ptr_tables_check) and run as a child process by tests/test_ptr_tables.py.
#include <cstdio>
#include <tuple>
#include <utility>
#include <vector>

#include "ptr_tables.h"

using namespace pvio;

static int failures = 0, reported = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) std::printf("FAILED line %d: %s\n", __LINE__, #cond), ++failures; \
    } while (0)
static void group(const char *name) {
    std::printf("%s: %s\n", name, failures == reported ? "ok" : "FAILED");
    reported = failures;
}

static char pool[1 << 16]; // addresses to use as keys

// the next address behind `from` whose home slot among `slots` is the one of `like`
static const char *colliding(const char *like, const char *from, size_t slots) {
    for (const char *p = from + 1; p < pool + sizeof pool; ++p)
        if ((ptr_hash(p) & (slots - 1)) == (ptr_hash(like) & (slots - 1))) return p;
    return nullptr;
}

static void fixed_table() {
    {
        PtrIndex<char> t;
        CHECK(t.find(pool) == -1); // empty
        const char *a = pool, *b = colliding(a, a, 256), *c = colliding(a, b, 256);
        CHECK(b && c);
        t.put(a, 1), t.put(b, 2);
        CHECK(t.find(a) == 1 && t.find(b) == 2 && t.find(c) == -1); // c probes past both and ends at the empty slot
        t.put(a, 7); // overwrite: same slot, no new key
        CHECK(t.find(a) == 7 && t.find(b) == 2);
        t.clear();
        CHECK(t.find(a) == -1 && t.find(b) == -1);
        // the default size refuses key number 129 and keeps the 128
        for (int i = 0; i < 128; ++i) t.put(pool + 64 * i, i);
        bool refused = false;
        try {
            t.put(pool + 64 * 128, 128);
        } catch (const std::length_error &) { refused = true; }
        CHECK(refused && t.find(pool + 64 * 128) == -1);
        for (int i = 0; i < 128; ++i) CHECK(t.find(pool + 64 * i) == i);
        t.clear();
        t.put(pool + 64 * 128, 5); // clear() gives the room back
        CHECK(t.find(pool + 64 * 128) == 5);
    }
    {
        PtrIndex<char, 8> t; // all keys in one probe chain: the smallest table that can wrap around
        const char *k[5] = {pool};
        for (int i = 1; i < 5; ++i) k[i] = colliding(k[0], k[i - 1], 8);
        CHECK(k[4] != nullptr);
        for (int i = 0; i < 4; ++i) t.put(k[i], 10 + i);
        bool refused = false;
        try {
            t.put(k[4], 14);
        } catch (const std::length_error &) { refused = true; }
        CHECK(refused);
        CHECK(t.find(k[4]) == -1); // ends: half of the slots are still empty
        t.put(k[2], 99);           // an existing key is still taken
        CHECK(t.find(k[0]) == 10 && t.find(k[1]) == 11 && t.find(k[2]) == 99 && t.find(k[3]) == 13);
    }
    group("fixed table");
}

static void ptr_set() {
    PtrSet s;
    CHECK(!s.contains(pool) && s.insert(pool) && !s.insert(pool) && s.contains(pool));
    for (int i = 1; i < 40; ++i) CHECK(s.insert(pool + 8 * i)); // 64 slots double when the 32nd member comes
    for (int i = 0; i < 40; ++i) CHECK(s.contains(pool + 8 * i) && !s.insert(pool + 8 * i));
    CHECK(!s.contains(pool + 8 * 40));
    s.reset(100); // a larger table
    for (int i = 0; i < 40; ++i) CHECK(!s.contains(pool + 8 * i));
    for (int i = 0; i < 300; ++i) CHECK(s.insert(pool + 8 * i)); // past the expectation as well
    for (int i = 0; i < 300; ++i) CHECK(s.contains(pool + 8 * i));
    s.reset(0); // a smaller one
    CHECK(!s.contains(pool) && s.insert(pool) && !s.insert(pool));
    group("PtrSet");
}

// ---- ObsCache: a track is a list of (frame id, z) in ascending frame id, the first one the anchor
struct Obs {
    size_t fid;
    double z0, z1;
};
struct FakeTrack {
    size_t id;
    std::vector<Obs> obs;
    ObsCache::Signature signature() const { return {id, obs.size(), obs.front().fid, obs.back().fid}; }
};
struct FakeView {
    const FakeTrack *t;
    int *asked; // how often the cache wanted the id before the last
    size_t id_before_last() const { return ++*asked, t->obs[t->obs.size() - 2].fid; }
    template <class Put>
    void newest(Put &&put) const { put(t->obs.back().fid, t->obs.back().z0, t->obs.back().z1); }
    template <class Put>
    void each(Put &&put) const {
        for (size_t i = 1; i < t->obs.size(); ++i) put(t->obs[i].fid, t->obs[i].z0, t->obs[i].z1);
    }
};
using Row = std::vector<std::tuple<int, double, double>>;

static Row from_scratch(const FakeTrack &t, const std::vector<size_t> &win) {
    Row row;
    for (size_t i = 1; i < t.obs.size(); ++i)
        for (size_t w = 0; w < win.size(); ++w)
            if (win[w] == t.obs[i].fid) row.emplace_back((int)w, t.obs[i].z0, t.obs[i].z1);
    return row;
}
static int asked = 0;
// one replay through the cache (under `key`, the track's own address unless given): the outcome, and whether the row is the one from scratch
static ObsCache::Outcome replay(ObsCache &c, const FakeTrack &t, const std::vector<size_t> &win, const void *key = nullptr) {
    Row row;
    const ObsCache::Outcome o = c.replay(key ? key : &t, t.signature(), FakeView{&t, &asked}, win.data(), (int)win.size(), [&row](int w, double z0, double z1) { row.emplace_back(w, z0, z1); });
    CHECK(row == from_scratch(t, win));
    return o;
}
static FakeTrack track(size_t id, std::initializer_list<size_t> fids) {
    FakeTrack t{id, {}};
    for (size_t f : fids) t.obs.push_back({f, 0.5 * (double)f + (double)id, -0.25 * (double)f});
    return t;
}

static void obs_cache() {
    const std::vector<size_t> win = {10, 11, 12, 13};
    {
        ObsCache c; // nothing reserved: every append below may reallocate the store
        FakeTrack t = track(1, {10, 11, 12});
        CHECK(replay(c, t, win) == ObsCache::kRebuilt && c.stored() == 2 && c.tracks() == 1);
        CHECK(from_scratch(t, win).size() == 2);
        asked = 0;
        CHECK(replay(c, t, win) == ObsCache::kUnchanged && c.stored() == 2 && asked == 0);
        // grown by one: the list moves behind the old one, the new observation behind it
        t.obs.push_back({13, 6.5, 7.5});
        CHECK(replay(c, t, win) == ObsCache::kGrown && c.stored() == 2 + 3 && c.tracks() == 1 && asked == 1);
        CHECK(from_scratch(t, win).size() == 3);
        CHECK(replay(c, t, win) == ObsCache::kUnchanged && c.stored() == 5);
        // ... and again and again from the tiny store: every size the vectors reallocate at on the way
        std::vector<size_t> long_win = win;
        for (size_t f = 14; f < 40; ++f) {
            t.obs.push_back({f, (double)f, 1.0}), long_win.push_back(f);
            CHECK(replay(c, t, long_win) == ObsCache::kGrown);
        }
        CHECK(replay(c, t, long_win) == ObsCache::kUnchanged);
    }
    {
        ObsCache c;
        FakeTrack t = track(2, {10, 11, 12});
        CHECK(replay(c, t, win) == ObsCache::kRebuilt);
        // one more keypoint and a new last id, but the id before it (13) is not the cached last (12)
        FakeTrack u = track(2, {10, 11, 13, 14});
        asked = 0;
        CHECK(replay(c, u, {10, 11, 12, 13, 14}, &t) == ObsCache::kRebuilt && asked == 1);
        CHECK(replay(c, u, {10, 11, 12, 13, 14}, &t) == ObsCache::kUnchanged);
        // the same address with another track id (a recycled Track)
        FakeTrack v = track(3, {10, 11, 13, 14});
        CHECK(replay(c, v, {10, 11, 12, 13, 14}, &t) == ObsCache::kRebuilt);
        // same count, other last id
        FakeTrack w = track(3, {10, 11, 13, 15});
        asked = 0;
        CHECK(replay(c, w, {10, 11, 13, 15}, &t) == ObsCache::kRebuilt && asked == 0);
        // the anchor slid out: first id changed, one keypoint fewer
        FakeTrack x = track(3, {11, 13, 15});
        CHECK(replay(c, x, {11, 13, 15}, &t) == ObsCache::kRebuilt);
        // ... or with one new observation at the same time: same count as cached + 1 is not enough either
        FakeTrack y = track(3, {13, 15, 16, 17});
        asked = 0;
        CHECK(replay(c, y, {13, 15, 16, 17}, &t) == ObsCache::kRebuilt && asked == 0);
        CHECK(c.tracks() == 1);
        // a one-keypoint track (the anchor alone, an empty list) that grows to two: the id before the last is the anchor's
        FakeTrack z = track(4, {20});
        CHECK(replay(c, z, {20, 21}) == ObsCache::kRebuilt && from_scratch(z, {20, 21}).empty());
        z.obs.push_back({21, 1.0, 2.0});
        CHECK(replay(c, z, {20, 21}) == ObsCache::kGrown && from_scratch(z, {20, 21}).size() == 1);
    }
    group("ObsCache outcomes");
    {
        ObsCache c;
        FakeTrack t = track(5, {10, 11, 12, 13, 14, 15});
        CHECK(replay(c, t, {10, 11, 12, 13, 14, 15}) == ObsCache::kRebuilt);
        // the window lost frame 12 in the middle and 15 at the end; 9 and 16 are frames the track never saw
        const std::vector<size_t> holes = {9, 10, 11, 13, 14, 16};
        CHECK(replay(c, t, holes) == ObsCache::kUnchanged);
        const Row want = {{2, 0.5 * 11 + 5, -0.25 * 11}, {3, 0.5 * 13 + 5, -0.25 * 13}, {4, 0.5 * 14 + 5, -0.25 * 14}};
        CHECK(from_scratch(t, holes) == want);
        CHECK(replay(c, t, {}) == ObsCache::kUnchanged); // no window at all
    }
    group("ObsCache replay");
    {
        ObsCache c;
        std::vector<FakeTrack> tracks;
        for (size_t i = 0; i < 300; ++i) tracks.push_back(track(100 + i, {10, 11 + i % 3, 20 + i % 5}));
        for (size_t i = 0; i < 300; ++i) { // the slot table is rebuilt on the way (at 129 keys): every earlier list replays the same
            CHECK(replay(c, tracks[i], {10, 11, 12, 13, 20, 21, 22, 23, 24}) == ObsCache::kRebuilt);
            if (i == 127 || i == 128 || i == 299)
                for (size_t j = 0; j <= i; ++j) CHECK(replay(c, tracks[j], {10, 11, 12, 13, 20, 21, 22, 23, 24}) == ObsCache::kUnchanged);
        }
        CHECK(c.tracks() == 300 && c.stored() == 600);
    }
    group("ObsCache rehash");
    {
        // drop rule: more than 8 * estimate + 65536 observations in the store
        ObsCache c;
        FakeTrack big{7, {}};
        for (size_t f = 0; f <= 65536; ++f) big.obs.push_back({f, 1.0, 2.0});
        FakeTrack one = track(8, {1, 2});
        const std::vector<size_t> w = {1, 2};
        CHECK(replay(c, big, w) == ObsCache::kRebuilt && c.stored() == 65536);
        c.begin_window(0);
        CHECK(c.stored() == 65536 && c.tracks() == 1 && replay(c, big, w) == ObsCache::kUnchanged);
        CHECK(replay(c, one, w) == ObsCache::kRebuilt && c.stored() == 65537);
        c.begin_window(1); // 65537 > 65544: no
        CHECK(c.stored() == 65537 && c.tracks() == 2);
        c.begin_window(0); // 65537 > 65536: yes
        CHECK(c.stored() == 0 && c.tracks() == 0);
        CHECK(replay(c, one, w) == ObsCache::kRebuilt && c.stored() == 1 && c.tracks() == 1);
    }
    group("ObsCache begin_window");
}

int main() {
    fixed_table();
    ptr_set();
    obs_cache();
    return failures ? 1 : 0;
}
