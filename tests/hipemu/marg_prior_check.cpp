// marg_prior_check.cpp -- pvio_amd/csrc/marg_prior.h alone: the dense host algebra of a marginalization without a solver or a device, built with
// -fsanitize=address,undefined (Makefile: marg_prior_check) and run as a child process by tests/test_marg_prior.py.
//
// assemble_information and eliminate_victim are held to restatements with ==: every input is an integer of magnitude <= 8 and the victim's
// 15 x 15 block is a diagonal of powers of two, so the pivoted LU inverse and every product and sum are exact in double whatever their order.
// sqrt_information is held to its invariants (S^T S = C, S^T s = cv, tests/marg_compare.py's tolerances) and to its zero-row and cut rules.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "marg_prior.h"

using namespace pvba;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) std::printf("FAILED line %d: %s\n", __LINE__, #cond), ++failures; \
    } while (0)

static uint32_t rng_state = 12345u;
static int small_int() { // -8 .. 8
    rng_state = rng_state * 1664525u + 1013904223u;
    return (int)((rng_state >> 16) % 17u) - 8;
}
static double unit() { return small_int() / 8.0 + small_int() / 64.0; }
static void fill_sym(std::vector<double> &A, int n) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) A[(size_t)i * n + j] = A[(size_t)j * n + i] = small_int();
}

// One window's read-back segments, every array exactly as long as the gather makes it (the sanitizer watches the ends).
struct Window {
    int N, victim, n_tasks, P6;
    std::vector<int32_t> prior_frames, tasks;
    std::vector<uint8_t> preint_valid;
    std::vector<double> red, pre_H, pre_g, prior_H, prior_g, rot_H, rot_g;
    int Dp() const { return 15 * (int)prior_frames.size(); }
    MargSegments segments() const { return {red.data(), pre_H.data(), pre_g.data(), prior_H.data(), prior_g.data(), rot_H.data(), rot_g.data(), tasks.data()}; }
};

// the definition, written per source and per element: H(r, c) and b(r) as sums over everything that lands there
static void restate_information(const Window &w, std::vector<double> &H, std::vector<double> &b) {
    const int N = w.N, D = 15 * N, nS = 9 * w.n_tasks;
    H.assign((size_t)D * D, 0.0), b.assign(D, 0.0);
    int t = 0;
    for (int fi = 0; fi < N; ++fi) // the task order of the upload's plan: upper block triangle, four 3 x 3 tiles each
        for (int fj = fi; fj < N; ++fj)
            for (int s = 0; s < 4; ++s, ++t)
                for (int x = 0; x < 3; ++x)
                    for (int y = 0; y < 3; ++y) {
                        const int r = 15 * fi + 3 * (s >> 1) + x, c = 15 * fj + 3 * (s & 1) + y;
                        if (fi == fj && r < c) continue; // the upper half of a diagonal block comes from its mirror image
                        H[(size_t)r * D + c] = w.red[(size_t)(3 * x + y) * w.n_tasks + t];
                        H[(size_t)c * D + r] = H[(size_t)r * D + c];
                    }
    for (int k = 0; k < 6 * N; ++k) b[15 * (k / 6) + k % 6] = w.red[nS + k] - w.red[nS + w.P6 + k];
    for (int j = 1; j < N; ++j)
        if ((j == w.victim || j == w.victim + 1) && w.preint_valid[j])
            for (int a = 0; a < 30; ++a) {
                b[15 * (j - 1) + a] += w.pre_g[(size_t)j * 30 + a];
                for (int c = 0; c < 30; ++c) H[(size_t)(15 * (j - 1) + a) * D + 15 * (j - 1) + c] += w.pre_H[(size_t)j * 900 + 30 * a + c];
            }
    for (int a = 0; a < 3; ++a) {
        b[15 * w.victim + a] += w.rot_g[3 * w.victim + a];
        for (int c = 0; c < 3; ++c) H[(size_t)(15 * w.victim + a) * D + 15 * w.victim + c] += w.rot_H[9 * w.victim + 3 * a + c];
    }
    const int Dp = w.Dp();
    for (int a = 0; a < Dp; ++a) {
        const int ra = 15 * w.prior_frames[a / 15] + a % 15;
        b[ra] += w.prior_g[a];
        for (int c = 0; c < Dp; ++c) H[(size_t)ra * D + 15 * w.prior_frames[c / 15] + c % 15] += w.prior_H[(size_t)a * Dp + c];
    }
}

// diag_from: which source carries the victim's diagonal (0: IMU factor `victim`, 1: IMU factor `victim + 1`, 2: the prior); every source's part of the
// victim's block is otherwise zero, so the assembled block is the diagonal 1, 2, 4, 8, 1, ... (zero_pivot: its column 7 is zero)
static Window make_window(int N, int victim, std::vector<int32_t> prior_frames, std::vector<uint8_t> preint_valid, int diag_from, bool zero_pivot = false) {
    Window w;
    w.N = N, w.victim = victim, w.n_tasks = 4 * N * (N + 1) / 2, w.P6 = 6 * N;
    w.prior_frames = prior_frames, w.preint_valid = preint_valid;
    for (int fi = 0; fi < N; ++fi)
        for (int fj = fi; fj < N; ++fj)
            for (int s = 0; s < 4; ++s) w.tasks.push_back(fi | (fj << 8) | ((s >> 1) << 16) | ((s & 1) << 17));
    const int Dp = w.Dp();
    w.red.resize((size_t)9 * w.n_tasks + 2 * w.P6), w.pre_H.resize((size_t)N * 900), w.pre_g.resize((size_t)N * 30);
    w.prior_H.resize((size_t)Dp * Dp), w.prior_g.resize(Dp), w.rot_H.resize((size_t)N * 9), w.rot_g.resize((size_t)N * 3);
    for (double &x : w.red) x = small_int();
    for (double &x : w.pre_g) x = small_int();
    for (double &x : w.prior_g) x = small_int();
    for (double &x : w.rot_g) x = small_int();
    for (int j = 0; j < N; ++j) {
        std::vector<double> A(900), B(9);
        fill_sym(A, 30), fill_sym(B, 3);
        std::copy(A.begin(), A.end(), w.pre_H.begin() + (size_t)j * 900);
        std::copy(B.begin(), B.end(), w.rot_H.begin() + (size_t)j * 9);
    }
    fill_sym(w.prior_H, Dp);
    // the victim's block: zero in every source ...
    for (int t = 0; t < w.n_tasks; ++t)
        if ((w.tasks[t] & 255) == victim && ((w.tasks[t] >> 8) & 255) == victim)
            for (int el = 0; el < 9; ++el) w.red[(size_t)el * w.n_tasks + t] = 0;
    for (int a = 0; a < 15; ++a)
        for (int c = 0; c < 15; ++c) {
            w.pre_H[(size_t)victim * 900 + (15 + a) * 30 + 15 + c] = 0; // factor `victim` ends in the victim
            if (victim + 1 < N) w.pre_H[(size_t)(victim + 1) * 900 + a * 30 + c] = 0; // factor `victim + 1` starts there
        }
    for (int k = 0; k < 9; ++k) w.rot_H[(size_t)victim * 9 + k] = 0;
    for (int a = 0; a < Dp; ++a)
        for (int c = 0; c < Dp; ++c)
            if (prior_frames[a / 15] == victim && prior_frames[c / 15] == victim) w.prior_H[(size_t)a * Dp + c] = 0;
    // ... but the diagonal of the one that carries it
    for (int k = 0; k < 15; ++k) {
        const double d = (zero_pivot && k == 7) ? 0.0 : (double)(1 << (k % 4));
        if (diag_from == 0) w.pre_H[(size_t)victim * 900 + (15 + k) * 30 + 15 + k] = d;
        if (diag_from == 1) w.pre_H[(size_t)(victim + 1) * 900 + k * 30 + k] = d;
        if (diag_from == 2)
            for (int a = 0; a < Dp; ++a)
                if (prior_frames[a / 15] == victim && a % 15 == k) w.prior_H[(size_t)a * Dp + a] = d;
    }
    return w;
}

static void check_exact(const char *name, const Window &w) {
    const int N = w.N, D = 15 * N, R = D - 15, v0 = 15 * w.victim;
    std::vector<double> H, b, H0, b0, C, cv;
    assemble_information(w.segments(), w.preint_valid.data(), w.prior_frames.data(), (int)w.prior_frames.size(), N, w.victim, w.n_tasks, w.P6, H, b);
    restate_information(w, H0, b0);
    CHECK(H == H0 && b == b0);
    bool diagonal = true;
    for (int x = 0; x < 15; ++x)
        for (int y = 0; y < 15; ++y) diagonal &= H[(size_t)(v0 + x) * D + v0 + y] == (x == y ? (double)(1 << (x % 4)) : 0.0);
    CHECK(diagonal);
    CHECK(eliminate_victim(H, b, N, w.victim, C, cv));
    CHECK((int)C.size() == R * R && (int)cv.size() == R);
    // C = H_rr - H_rv H_vv^-1 H_vr, cv = b_r - H_rv H_vv^-1 b_v: three loops, the inverse of the diagonal written down
    auto g = [&](int k) { return k < v0 ? k : k + 15; };
    bool same = (int)C.size() == R * R && (int)cv.size() == R;
    for (int i = 0; i < R && same; ++i) {
        double sv = 0;
        for (int y = 0; y < 15; ++y) sv += H[(size_t)g(i) * D + v0 + y] / (double)(1 << (y % 4)) * b[v0 + y];
        same &= cv[i] == b[g(i)] - sv;
        for (int j = 0; j < R; ++j) {
            double s = 0;
            for (int y = 0; y < 15; ++y) s += H[(size_t)g(i) * D + v0 + y] / (double)(1 << (y % 4)) * H[(size_t)(v0 + y) * D + g(j)];
            same &= C[(size_t)i * R + j] == H[(size_t)g(i) * D + g(j)] - s;
        }
    }
    CHECK(same);
    std::printf("%s: %s\n", name, failures ? "FAILED" : "ok");
}

static void check_singular() {
    const Window w = make_window(3, 1, {}, {0, 1, 1}, 1, /*zero_pivot=*/true);
    std::vector<double> H, b, C(7, -3.0), cv(5, -4.0);
    assemble_information(w.segments(), w.preint_valid.data(), w.prior_frames.data(), 0, 3, 1, w.n_tasks, w.P6, H, b);
    CHECK(!eliminate_victim(H, b, 3, 1, C, cv));
    CHECK(C == std::vector<double>(7, -3.0) && cv == std::vector<double>(5, -4.0)); // nothing written
    std::printf("singular victim block: %s\n", failures ? "FAILED" : "ok");
}

// S^T S against C and S^T s against cv, numpy.testing.assert_allclose's rule with tests/marg_compare.py's tolerances
static void check_sqrt_invariants(const std::vector<double> &C, const std::vector<double> &cv, int R, const std::vector<double> &S, const std::vector<double> &s) {
    double cmax = 0, vmax = 0;
    for (double x : C) cmax = std::max(cmax, std::fabs(x));
    for (double x : cv) vmax = std::max(vmax, std::fabs(x));
    bool ok = true;
    for (int i = 0; i < R; ++i) {
        double ts = 0;
        for (int k = 0; k < R; ++k) ts += S[(size_t)k * R + i] * s[k];
        ok &= std::fabs(ts - cv[i]) <= 1e-6 * vmax + 1e-6 * std::fabs(cv[i]);
        for (int j = 0; j < R; ++j) {
            double ss = 0;
            for (int k = 0; k < R; ++k) ss += S[(size_t)k * R + i] * S[(size_t)k * R + j];
            ok &= std::fabs(ss - C[(size_t)i * R + j]) <= 1e-7 * cmax + 1e-6 * std::fabs(C[(size_t)i * R + j]);
        }
    }
    CHECK(ok);
}

static std::vector<double> random_spd(int n, std::vector<double> &cv) {
    std::vector<double> A((size_t)n * n), C((size_t)n * n, 0.0);
    for (double &x : A) x = unit();
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            for (int k = 0; k < n; ++k) C[(size_t)i * n + j] += A[(size_t)i * n + k] * A[(size_t)j * n + k];
            if (i == j) C[(size_t)i * n + j] += n;
        }
    cv.resize(n);
    for (double &x : cv) x = unit();
    return C;
}

static bool row_is_zero(const std::vector<double> &S, int R, int k) {
    for (int j = 0; j < R; ++j)
        if (S[(size_t)k * R + j] != 0.0) return false;
    return true;
}

static void check_sqrt_information() {
    std::vector<double> V;
    { // two coordinates without information (nz = 2): their rows of S are zero and come first, their columns are zero, the rest is C's square root
        const int R = 6, Rk = 4, kept[4] = {0, 2, 3, 5};
        std::vector<double> cvk, Ck = random_spd(Rk, cvk), C((size_t)R * R, 0.0), cv(R, 0.0), S((size_t)R * R, 7.0), s(R, 7.0);
        for (int a = 0; a < Rk; ++a) {
            cv[kept[a]] = cvk[a];
            for (int b = 0; b < Rk; ++b) C[(size_t)kept[a] * R + kept[b]] = Ck[(size_t)a * Rk + b];
        }
        std::vector<double> work = C;
        const SqrtInfoStats st = sqrt_information(work, cv, R, V, S.data(), s.data());
        CHECK(st.Rk == Rk);
        CHECK(row_is_zero(S, R, 0) && row_is_zero(S, R, 1) && s[0] == 0.0 && s[1] == 0.0);
        for (int k = 0; k < R; ++k) CHECK(S[(size_t)k * R + 1] == 0.0 && S[(size_t)k * R + 4] == 0.0);
        for (int k = 2; k < R; ++k) CHECK(!row_is_zero(S, R, k));
        check_sqrt_invariants(C, cv, R, S, s);
        std::printf("sqrt_information, two empty coordinates: %s\n", failures ? "FAILED" : "ok");
    }
    { // no information at all (Rk = 0): everything zero, nothing read or written beyond the arrays
        const int R = 15;
        std::vector<double> C((size_t)R * R, 0.0), cv(R, 1.0), S((size_t)R * R, 7.0), s(R, 7.0), V0;
        const SqrtInfoStats st = sqrt_information(C, cv, R, V0, S.data(), s.data());
        CHECK(st.Rk == 0 && S == std::vector<double>((size_t)R * R, 0.0) && s == std::vector<double>(R, 0.0));
        std::printf("sqrt_information, empty: %s\n", failures ? "FAILED" : "ok");
    }
    { // one eigenvalue below the 1e-8 cut: its row (the first: ascending order) and its entry of s are zero, the other rows are not
        const int R = 4;
        const double lam[4] = {1e-10, 1.0, 2.0, 3.0}, c = 0.8, sn = 0.6; // eigenvectors: a rotation of coordinates 0 and 1
        const double Q[4][4] = {{c, sn, 0, 0}, {-sn, c, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
        std::vector<double> C((size_t)R * R, 0.0), cv = {1.0, -2.0, 0.5, 4.0}, S((size_t)R * R, 7.0), s(R, 7.0);
        for (int i = 0; i < R; ++i)
            for (int j = 0; j < R; ++j)
                for (int k = 0; k < R; ++k) C[(size_t)i * R + j] += Q[k][i] * lam[k] * Q[k][j];
        const SqrtInfoStats st = sqrt_information(C, cv, R, V, S.data(), s.data());
        CHECK(st.Rk == R && row_is_zero(S, R, 0) && s[0] == 0.0);
        for (int k = 1; k < R; ++k) CHECK(!row_is_zero(S, R, k) && s[k] != 0.0);
        std::printf("sqrt_information, eigenvalue below the cut: %s\n", failures ? "FAILED" : "ok");
    }
    { // well conditioned, 30 x 30
        const int R = 30;
        std::vector<double> cv, C = random_spd(R, cv), S((size_t)R * R, 7.0), s(R, 7.0);
        std::vector<double> work = C;
        const SqrtInfoStats st = sqrt_information(work, cv, R, V, S.data(), s.data());
        CHECK(st.Rk == R);
        check_sqrt_invariants(C, cv, R, S, s);
        std::printf("sqrt_information, 30 x 30: %s\n", failures ? "FAILED" : "ok");
    }
}

int main() {
    check_exact("N = 2, victim 0", make_window(2, 0, {}, {0, 1}, 1));                                     // split = 0
    check_exact("N = 2, victim 1", make_window(2, 1, {}, {0, 1}, 0));                                     // split = R
    check_exact("N = 3, victim 1", make_window(3, 1, {}, {0, 1, 1}, 0));                                  // split in the middle, both IMU factors
    check_exact("N = 3, victim 0, prior on frames 0 and 2", make_window(3, 0, {0, 2}, {0, 0, 0}, 2));     // the prior scatters
    check_exact("N = 3, victim 2, prior on frames 2 and 0", make_window(3, 2, {2, 0}, {0, 0, 1}, 2));     // ... in either order
    check_exact("N = 3, victim 1, IMU factor 2 only", make_window(3, 1, {0, 2}, {0, 0, 1}, 1));           // preint_valid for victim + 1 only
    check_singular();
    check_sqrt_information();
    return failures ? 1 : 0;
}
