// plane_sampler_check.cpp -- pv_plane.h's restated sampler (PlMinstd, pl_uniform, PlSampler) against the classes the reference uses:
// std::default_random_engine + std::uniform_int_distribution<size_t> under a LotBox whose permutation persists (utility/random.h:108-163),
// 1000 iterations of three draws for every n and every seed below.  Stand-alone (own main); tests/test_plane_ransac.py builds and runs it, and it
// may be built with -fsanitize=address,undefined as it is.  Exit status 0: every index identical.
#include <cstdio>
#include <numeric>
#include <random>
#include <vector>

#include "../../pvio_amd/csrc/pv_plane.h"

namespace {

struct StdLotBox { // a lot box over the std classes: the behaviour utility/random.h:108-163 describes, written for this check
    size_t cap = 0;
    std::vector<size_t> lots;
    std::default_random_engine engine;
    std::uniform_int_distribution<size_t> dist;
    StdLotBox(size_t n, unsigned seed) : lots(n) {
        std::iota(lots.begin(), lots.end(), (size_t)0);
        engine.seed(seed);
    }
    size_t draw() {
        if (lots.size() - cap > 1) {
            std::swap(lots[cap], lots[dist(engine, std::uniform_int_distribution<size_t>::param_type(cap, lots.size() - 1))]);
            return lots[cap++];
        }
        ++cap;
        return lots.back();
    }
};

} // namespace

int main() {
    const int sizes[] = {3, 4, 5, 7, 64, 65, 300, 1000, 50000};
    const unsigned seeds[] = {0u, 12345u, 2147483647u};
    int bad = 0;
    for (unsigned seed : seeds)
        for (int n : sizes) {
            StdLotBox ref((size_t)n, seed);
            pvpl::PlSampler mine(n, seed);
            for (int iter = 0; iter < 1000; ++iter) {
                ref.cap = 0;
                int32_t s[3];
                mine.sample(s);
                for (int k = 0; k < 3; ++k) {
                    const size_t want = ref.draw();
                    if ((size_t)s[k] != want && bad++ < 10) std::printf("n %d seed %u iteration %d draw %d: %d, std gives %zu\n", n, seed, iter, k, s[k], want);
                }
                if (n == 300 && seed == 0 && iter == 0) std::printf("n 300 seed 0 first sample %d %d %d\n", s[0], s[1], s[2]);
            }
        }
    std::printf("%s: %d differing indices\n", bad ? "FAIL" : "OK", bad);
    return bad ? 1 : 0;
}
