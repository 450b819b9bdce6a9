// hip_buffer_check.cpp -- pvio_amd/csrc/hip_buffer.h alone, above the emulator's allocator (guard bytes behind every allocation, a list of the
// live ones), built with -fsanitize=address,undefined (Makefile: hip_buffer_check) and run as a child process by tests/test_hip_buffer.py.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "hip_buffer.h"

// the failure leg asks for more than malloc can give: it has to answer with nullptr, not end the program
extern "C" const char *__asan_default_options() { return "allocator_may_return_null=1"; }

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) std::printf("FAILED line %d: %s\n", __LINE__, #cond), ++failures; \
    } while (0)

static size_t live() { return hipemu::guarded().size(); }

template <class Buffer>
static void exercise(const char *flavour) {
    const size_t live0 = live();
    {
        Buffer empty; // destroyed empty: nothing to free
        CHECK(empty.data() == nullptr && empty.capacity() == 0);
    }
    CHECK(live() == live0);
    {
        Buffer b;
        // grow: to `grow_to`, not to `need`
        void *p = b.reserve(100, 200);
        CHECK(p != nullptr && p == b.data() && b.capacity() == 200 && live() == live0 + 1);
        std::memset(p, 1, 200); // all of it is ours (the emulator's guard bytes and the sanitizer watch the 201st)
        // keep: a smaller request, one of exactly the capacity, and whatever headroom it names
        CHECK(b.reserve(50, 4000) == p && b.reserve(200, 200) == p && b.capacity() == 200 && live() == live0 + 1);
        // a second growth frees the first buffer exactly once (a double free or a leak ends the run under the sanitizer)
        void *q = b.reserve(201, 300);
        CHECK(q != nullptr && q == b.data() && b.capacity() == 300 && live() == live0 + 1);
        std::memset(q, 2, 300);
        CHECK(b.template as<unsigned char>()[299] == 2);
        // grow_to below need: the request still fits
        CHECK(b.reserve(1000, 10) != nullptr && b.capacity() == 1000 && live() == live0 + 1);
        // failure: the old buffer is gone, the owner is empty, and it works again afterwards
        CHECK(b.reserve(SIZE_MAX / 2, SIZE_MAX / 2) == nullptr && b.data() == nullptr && b.capacity() == 0 && live() == live0);
        CHECK(b.reserve(64, 64) != nullptr && b.capacity() == 64 && live() == live0 + 1);
    } // destroyed full
    CHECK(live() == live0);
    std::printf("%s: %s\n", flavour, failures ? "FAILED" : "ok");
}

int main() {
    exercise<pvhip::DeviceBuffer>("device");
    exercise<pvhip::PinnedBuffer>("pinned");
    // the mirror pairs: both buffers exist or the pair does not count
    pvhip::DeviceBuffer d;
    pvhip::PinnedBuffer h;
    CHECK(d.reserve(32, 64) && h.reserve(32, 64));
    CHECK(!(d.reserve(128, 128) && h.reserve(SIZE_MAX / 2, SIZE_MAX / 2)) && d.capacity() == 128 && h.capacity() == 0);
    CHECK(d.reserve(128, 128) && h.reserve(128, 128) && h.capacity() == 128);
    return failures ? 1 : 0;
}
