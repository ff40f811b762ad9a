// Drives the rules of csrc/ehm_refine.hip that need no device (ehm_refine_host.h) on the CPU: the
// first longest edge, the plane of a bisection by its p x p solve for p = 1 .. 8, the rounding to the
// law's scalar, the acceptance test, the criteria, the worst-case leaf count, the depth of a leaf and
// the re-pointing of the one reference that named a split leaf, on random simplices and forests.
// Built with -fsanitize=address,undefined by tests/test_host_refine.py; needs no device and no
// library.  With arguments `p in out` it reads cells (doubles [n][p+1][p]) from `in` and writes per
// cell the doubles [i, j, length, a (p), b, accepted as double, its residual, accepted as float, its
// residual] to `out`: what the numpy mirror is compared with bit for bit.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../explicit_hybrid_mpc_amd/csrc/ehm_refine_host.h"

using namespace ehm_cert;
using namespace ehm_ref;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("%s:%d: %s fails\n", __FILE__, __LINE__, #cond);   \
            return 1;                                                      \
        }                                                                  \
    } while (0)

namespace {

struct Rng {
    unsigned x;
    unsigned next() {
        x = x * 1664525u + 1013904223u;
        return x >> 8;
    }
    double unit() { return (double)(next() & 0xffffff) / (double)0x1000000; }
};

// one cell through every rule; out (or nullptr) as the header says
template <int P>
int one_cell(const double (&V)[(P + 1) * P], bool expect_ok, double* out) {
    int i = -1, j = -1;
    const double len = longest_edge_of<P>(V, i, j);
    CHECK(0 <= i && i < j && j <= P);
    // the definition: no edge is longer, no earlier edge as long
    for (int a = 0; a <= P; ++a)
        for (int b = a + 1; b <= P; ++b) {
            double s = 0.0;
            for (int k = 0; k < P; ++k) s = std::fma(V[a * P + k] - V[b * P + k], V[a * P + k] - V[b * P + k], s);
            const double l = std::sqrt(s);
            CHECK(!(l > len));
            if (a < i || (a == i && b < j)) CHECK(l < len);
        }
    double a[P], b = 0.0;
    solve_plane<P>(V, i, j, a, b);
    double rd = 0.0, rf = 0.0;
    double rec64[P + 1];
    float rec32[P + 1];
    const bool ok64 = store_plane<double, P>(a, b, rec64) && accept_plane<double, P>(V, rec64, i, j, rd);
    const bool ok32 = store_plane<float, P>(a, b, rec32) && accept_plane<float, P>(V, rec32, i, j, rf);
    if (expect_ok) {
        CHECK(ok64 && ok32);
        CHECK(rd < 1e-9 && rf < 1e-2);
        // the plane is what it is said to be at every vertex
        for (int k = 0; k <= P; ++k) {
            double s = b;
            for (int c = 0; c < P; ++c) s += a[c] * V[k * P + c];
            const double target = k == j ? 1.0 : k == i ? -1.0 : 0.0;
            CHECK(std::fabs(s - target) < 1e-9);
        }
    }
    if (out) {
        int at = 0;
        out[at++] = i;
        out[at++] = j;
        out[at++] = len;
        for (int c = 0; c < P; ++c) out[at++] = a[c];
        out[at++] = b;
        out[at++] = ok64;
        out[at++] = rd;
        out[at++] = ok32;
        out[at++] = rf;
    }
    return 0;
}

template <int P>
int random_cells(unsigned seed) {
    Rng rng{seed};
    for (int rep = 0; rep < 50; ++rep) {
        // a well-shaped simplex: the standard one, stretched per axis and shifted, vertices permuted
        double V[(P + 1) * P];
        double scale[P], shift[P];
        for (int c = 0; c < P; ++c) {
            scale[c] = 0.5 + rng.unit();
            shift[c] = 4.0 * rng.unit() - 2.0;
        }
        const int rot = (int)(rng.next() % (unsigned)(P + 1));
        for (int k = 0; k <= P; ++k) {
            const int at = (k + rot) % (P + 1);
            for (int c = 0; c < P; ++c)
                V[at * P + c] = shift[c] + (k == c + 1 ? scale[c] : 0.0) + 0.05 * rng.unit();
        }
        if (one_cell<P>(V, true, nullptr)) return 1;
    }
    // a flat cell (two vertices equal) has no plane: never accepted, nothing read out of bounds
    double V[(P + 1) * P];
    for (int k = 0; k <= P; ++k)
        for (int c = 0; c < P; ++c) V[k * P + c] = (k == c + 1 && k < P) ? 1.0 : 0.0;
    if (P > 1) {
        int i, j;
        longest_edge_of<P>(V, i, j);
        double a[P], b, r;
        solve_plane<P>(V, i, j, a, b);
        double rec[P + 1];
        CHECK(!(store_plane<double, P>(a, b, rec) && accept_plane<double, P>(V, rec, i, j, r)));
    }
    return 0;
}

template <int P>
int file_cells(const char* in, const char* out) {
    std::FILE* f = std::fopen(in, "rb");
    CHECK(f);
    std::vector<double> cells;
    double buf[(P + 1) * P];
    while (std::fread(buf, sizeof buf, 1, f) == 1) cells.insert(cells.end(), buf, buf + (P + 1) * P);
    std::fclose(f);
    const size_t n = cells.size() / ((P + 1) * P), row = (size_t)P + 8;
    std::vector<double> res(n * row);
    for (size_t q = 0; q < n; ++q) {
        double V[(P + 1) * P];
        for (int e = 0; e < (P + 1) * P; ++e) V[e] = cells[q * (P + 1) * P + e];
        if (one_cell<P>(V, false, &res[q * row])) return 1;
    }
    std::FILE* g = std::fopen(out, "wb");
    CHECK(g);
    CHECK(std::fwrite(res.data(), sizeof(double), res.size(), g) == res.size());
    std::fclose(g);
    return 0;
}

int rules() {
    // the criteria: a NaN never exceeds and is never exceeded
    CHECK(exceeds(2.0, 1.0) && !exceeds(1.0, 1.0) && !exceeds(NAN, 1.0) && !exceeds(1.0, NAN));
    const double w[3] = {1.0, -2.0, 0.5}, wn[3] = {1.0, NAN, 5.0}, wi[2] = {INFINITY, INFINITY};
    CHECK(spread_of<3>(w) == 3.0);
    CHECK(std::isnan(spread_of<3>(wn)) && std::isnan(spread_of<2>(wi)));
    CHECK(storable(1.0) && !storable((double)INFINITY) && !storable((double)NAN));
    CHECK(storable(0.0f) && storable(-0.0f) && storable(1e-37f) && !storable(1e-39f) &&
          !storable((float)1e39));
    // the worst case
    const int32_t lv[4] = {0, 1, 16, 3};
    const uint8_t sel[4] = {1, 1, 0, 1};
    CHECK(worst_case_leaves(4, lv, nullptr) == 1 + 2 + 65536 + 8);
    CHECK(worst_case_leaves(4, lv, sel) == 1 + 2 + 1 + 8);
    const int32_t bad[3] = {0, 17, -1};
    CHECK(worst_case_leaves(3, bad, nullptr) == -2);
    CHECK(worst_case_leaves(1, bad + 2, nullptr) == -1);
    // a chain: root 0 enters internal record 0; record k has the leaf k on the left and record k + 1
    // (the last one: leaf n) on the right
    const int n = 300;
    std::vector<int32_t> pn((size_t)n), pl((size_t)n + 1);
    std::vector<uint8_t> sn((size_t)n, 0), sl((size_t)n + 1, 0);
    const Parents P{pn.data(), sn.data(), pl.data(), sl.data()};
    link_root(P, 0, 0);
    for (int k = 0; k < n; ++k) link_children(P, k, ~k, k + 1 < n ? k + 1 : ~n);
    link_root(P, 0, 0);
    for (int l = 0; l < n; ++l) CHECK(depth_of(P, l) == l + 1);
    CHECK(depth_of(P, n) == n);
    // re-pointing: leaf 5 (left of record 5) and leaf n (right of record n - 1) are split
    std::vector<int32_t> split((size_t)n + 1, 0), offset((size_t)n + 1, 0);
    split[5] = split[(size_t)n] = 1;
    offset[(size_t)n] = 1;
    CHECK(repoint_child(P, 5, 0, ~5, split.data(), offset.data(), n) == n);
    CHECK(repoint_child(P, 4, 0, ~5, split.data(), offset.data(), n) == ~5);    // not its parent
    CHECK(repoint_child(P, 5, 1, ~5, split.data(), offset.data(), n) == ~5);    // not that side
    CHECK(repoint_child(P, 6, 0, ~6, split.data(), offset.data(), n) == ~6);    // not split
    CHECK(repoint_child(P, 5, 1, 6, split.data(), offset.data(), n) == 6);      // an internal record
    CHECK(repoint_child(P, n - 1, 1, ~n, split.data(), offset.data(), n) == n + 1);
    // a root whose entry is a leaf
    std::vector<int32_t> ql(2, EHM_CERT_UNREACHED);
    std::vector<uint8_t> qs(2, 0);
    const Parents Q{nullptr, nullptr, ql.data(), qs.data()};
    link_root(Q, 0, ~1);
    const int32_t sp[2] = {0, 1}, off[2] = {0, 0};
    CHECK(repoint_entry(Q, 0, ~1, sp, off, 0) == 0);
    CHECK(repoint_entry(Q, 1, ~1, sp, off, 0) == ~1);       // another root
    CHECK(repoint_entry(Q, 0, 7, sp, off, 0) == 7);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4) {
        const int p = std::atoi(argv[1]);
        switch (p) {
            case 1: return file_cells<1>(argv[2], argv[3]);
            case 2: return file_cells<2>(argv[2], argv[3]);
            case 3: return file_cells<3>(argv[2], argv[3]);
            case 4: return file_cells<4>(argv[2], argv[3]);
            case 5: return file_cells<5>(argv[2], argv[3]);
            case 6: return file_cells<6>(argv[2], argv[3]);
            case 7: return file_cells<7>(argv[2], argv[3]);
            case 8: return file_cells<8>(argv[2], argv[3]);
            default: return 2;
        }
    }
    if (rules()) return 1;
    for (unsigned seed = 1; seed <= 4; ++seed)
        if (random_cells<1>(seed) || random_cells<2>(seed) || random_cells<3>(seed) ||
            random_cells<4>(seed) || random_cells<5>(seed) || random_cells<6>(seed) ||
            random_cells<7>(seed) || random_cells<8>(seed))
            return 1;
    std::printf("refine host helpers: ok\n");
    return 0;
}
