// Drives the host checks of csrc/ehm_cost.hip (ehm_cost_host.h) on the CPU: what is refused of the
// options, the domain, the start set and caller-supplied weights (each with its message), the
// verdict on what the device's check of the domain found, the order-preserving keys the per-step
// maxima and minima are reduced in, and the walk of the args into a path, on random relations
// against a plain restatement of the recurrence.  Built with -fsanitize=address,undefined by
// tests/test_host_cost.py; needs no device and no library.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../explicit_hybrid_mpc_amd/csrc/ehm_cost_host.h"

using namespace ehm_cost;

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
};

bool says(const ehm_err_channel& err, const char* what) {
    return std::strstr(err.c_str(), what) != nullptr;
}

// a relation over n leaves in exactly sized heap arrays, so that a read past an end is seen
struct Relation {
    std::vector<int64_t> indptr;
    std::vector<int32_t> indices, level, domain, start;
    std::vector<double> w_hi, w_lo;
    ehm_cost_opts opts() const {
        ehm_cost_opts o;
        std::memset(&o, 0, sizeof o);
        o.indptr = indptr.data();
        o.indices = indices.data();
        o.level = level.data();
        o.domain = domain.data();
        o.start = start.data();
        o.n_leaf = (int64_t)level.size();
        o.n_edges = (int64_t)indices.size();
        o.n_level = (int64_t)level.size();
        o.n_domain = (int64_t)domain.size();
        o.n_start = (int64_t)start.size();
        o.horizon = 5;
        return o;
    }
};

// every row nonempty but the last, the domain all leaves, small integer weights
Relation random_relation(int n, Rng& rng) {
    Relation r;
    r.indptr.push_back(0);
    for (int l = 0; l < n; ++l) {
        const int w = l == n - 1 ? 0 : 1 + (int)(rng.next() % 3);
        for (int k = 0; k < w; ++k) r.indices.push_back((int32_t)(rng.next() % (unsigned)n));
        r.indptr.push_back((int64_t)r.indices.size());
        r.level.push_back(-1);
        r.domain.push_back((int32_t)(n - 1 - l));       // descending, to be sorted
        r.w_lo.push_back((double)(rng.next() % 3));
        r.w_hi.push_back(r.w_lo.back() + (double)(rng.next() % 3));
    }
    r.start.push_back((int32_t)(rng.next() % (unsigned)n));
    r.start.push_back(r.start[0]);
    return r;
}

int test_keys() {
    const double inf = std::numeric_limits<double>::infinity();
    const double v[] = {-inf, -1e300, -2.5, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1.0 + 1e-15,
                        2.5, 1e300, inf};
    const int m = (int)(sizeof v / sizeof v[0]);
    for (int a = 0; a < m; ++a) {
        const double back = value_of(key_of(v[a]));
        CHECK(std::memcmp(&back, &v[a], sizeof back) == 0);
        for (int b = a + 1; b < m; ++b) CHECK(key_of(v[a]) < key_of(v[b]));
    }
    CHECK(key_of(-inf) > 0ull && key_of(inf) < ~0ull);     // the identities are outside
    return 0;
}

int test_refusals() {
    ehm_err_channel err;
    Rng rng{5};
    Relation r = random_relation(9, rng);
    ehm_cost_opts o = r.opts();
    CHECK(check_options(err, &o, 9, 1) == EHM_OK);
    CHECK(check_options(err, &o, 8, 1) == EHM_E_INVALID && says(err, "n_leaf = 9 of 8"));
    o.n_leaf = 0;
    CHECK(check_options(err, &o, 9, 1) == EHM_E_INVALID && says(err, "n_leaf = 0"));
    o = r.opts();
    CHECK(check_options(err, &o, 9, 5) == EHM_E_INVALID && says(err, "n_u = 5"));
    o.horizon = 0;
    CHECK(check_options(err, &o, 9, 1) == EHM_E_INVALID && says(err, "horizon = 0 < 1"));
    o = r.opts();
    o.w_hi = r.w_hi.data();
    CHECK(check_options(err, &o, 9, 1) == EHM_E_INVALID && says(err, "come together"));
    o.w_lo = r.w_lo.data();
    CHECK(check_options(err, &o, 9, 1) == EHM_OK);
    // the byte cap: horizon n 4 <= 2^28
    o.want_paths = 1;
    o.horizon = (int32_t)(MAX_PATH_BYTES / 4 / 9);
    CHECK(check_options(err, &o, 9, 1) == EHM_OK);
    o.horizon += 1;
    CHECK(check_options(err, &o, 9, 1) == EHM_E_INVALID && says(err, "2^28"));
    o.want_paths = 0;
    CHECK(check_options(err, &o, 9, 1) == EHM_OK);

    std::vector<uint8_t> dmask, smask;
    std::vector<int32_t> dom, start;
    o = r.opts();
    CHECK(rows_of(err, "domain", o.domain, o.n_domain, 9, dmask, dom) == EHM_OK);
    CHECK(dom.size() == 9 && dom[0] == 0 && dom[8] == 8 && dmask.size() == 9);
    CHECK(rows_of(err, "start", o.start, o.n_start, 9, smask, start) == EHM_OK);
    CHECK(start.size() == 1);                               // a row named twice is one row
    CHECK(check_subset(err, start, dmask) == EHM_OK);
    CHECK(rows_of(err, "domain", o.domain, 0, 9, dmask, dom) == EHM_E_INVALID &&
          says(err, "the domain set is empty"));
    const int32_t far[] = {3, 9}, neg[] = {-1};
    CHECK(rows_of(err, "start", far, 2, 9, smask, start) == EHM_E_INVALID &&
          says(err, "start[1] = 9 of 9"));
    CHECK(rows_of(err, "domain", neg, 1, 9, dmask, dom) == EHM_E_INVALID &&
          says(err, "domain[0] = -1"));
    const int32_t some[] = {4, 2, 4}, other[] = {2, 5};
    CHECK(rows_of(err, "domain", some, 3, 9, dmask, dom) == EHM_OK && dom.size() == 2);
    CHECK(rows_of(err, "start", other, 2, 9, smask, start) == EHM_OK);
    CHECK(check_subset(err, start, dmask) == EHM_E_INVALID &&
          says(err, "start row 5 is not in the domain"));

    // weights: only the domain's are read
    std::vector<double> hi(9, NAN), lo(9, NAN);
    hi[2] = 1.0, lo[2] = 1.0, hi[4] = 0.0, lo[4] = -1.0;
    CHECK(check_weights(err, hi.data(), lo.data(), dom) == EHM_OK);
    lo[4] = 0.5;
    CHECK(check_weights(err, hi.data(), lo.data(), dom) == EHM_E_INVALID &&
          says(err, "on row 4"));
    lo[4] = -INFINITY;
    CHECK(check_weights(err, hi.data(), lo.data(), dom) == EHM_E_INVALID &&
          says(err, "row 4") && says(err, "not finite"));
    hi[2] = NAN;
    CHECK(check_weights(err, hi.data(), lo.data(), dom) == EHM_E_INVALID && says(err, "row 2"));
    return 0;
}

int test_domain_verdict() {
    ehm_err_channel err;
    // 0 -> {1, 2}, 1 -> {3, 0, 4}, 2 -> {}, 3 -> {3}, 4 -> {0}
    const int32_t ptr[] = {0, 2, 5, 5, 6, 7}, idx[] = {1, 2, 3, 0, 4, 3, 0};
    int32_t level[] = {-1, -1, -1, -1, 0};
    std::vector<uint8_t> dom = {1, 1, 1, 0, 0};
    CHECK(first_outside(ptr, idx, 0, dom) == -1 && first_outside(ptr, idx, 2, dom) == -1);
    CHECK(first_outside(ptr, idx, 1, dom) == 3);            // the smallest, not the first
    CHECK(domain_verdict(err, -1, 5, level, ptr, idx, dom) == EHM_OK);
    CHECK(domain_verdict(err, 5, 5, level, ptr, idx, dom) == EHM_OK);
    CHECK(domain_verdict(err, 1, 5, level, ptr, idx, dom) == EHM_E_INVALID &&
          says(err, "row 1 of the domain reaches leaf 3 outside it"));
    dom[4] = 1;
    CHECK(domain_verdict(err, 4, 5, level, ptr, idx, dom) == EHM_E_INVALID &&
          says(err, "row 4 is a seed"));
    return 0;
}

// the recurrence and its args on the host, then the path against its right-nested sum
int test_paths() {
    Rng rng{77};
    for (int rep = 0; rep < 40; ++rep) {
        const int n = 1 + (int)(rng.next() % 12);
        const int32_t H = 1 + (int32_t)(rng.next() % 9);
        const Relation r = random_relation(n, rng);
        std::vector<double> U((size_t)n, 0.0), next((size_t)n);
        std::vector<int32_t> arg((size_t)H * (size_t)n);
        for (int32_t k = 0; k < H; ++k) {
            for (int l = 0; l < n; ++l) {
                double best = 0.0;
                int32_t at = -1;
                for (int64_t e = r.indptr[(size_t)l]; e < r.indptr[(size_t)l + 1]; ++e) {
                    const int32_t t = r.indices[(size_t)e];
                    if (at < 0 || U[(size_t)t] > best || (U[(size_t)t] == best && t < at)) {
                        best = U[(size_t)t];
                        at = t;
                    }
                }
                next[(size_t)l] = r.w_hi[(size_t)l] + best;
                arg[(size_t)k * (size_t)n + (size_t)l] = at;
            }
            U = next;
        }
        std::vector<int32_t> rows;
        for (int l = 0; l < n; ++l) rows.push_back(l);
        double top = U[0];
        for (int l = 1; l < n; ++l) top = U[(size_t)l] > top ? U[(size_t)l] : top;
        const int32_t first = first_attaining(U.data(), rows, top);
        CHECK(first >= 0 && U[(size_t)first] == top);
        for (int l = 0; l < first; ++l) CHECK(U[(size_t)l] != top);
        CHECK(first_attaining(U.data(), rows, top + 1.0) == -1);
        std::vector<int32_t> path((size_t)H + 1);
        walk_path(arg.data(), n, H, first, path.data());
        CHECK(path[0] == first);
        double sum = 0.0;
        bool ended = false;
        for (int32_t t = 0; t < H; ++t) {
            const int32_t l = path[(size_t)t];
            if (l < 0) {
                ended = true;
                CHECK(path[(size_t)t + 1] == -1);
                continue;
            }
            CHECK(!ended);
            sum += r.w_hi[(size_t)l];                       // small integers: exact in any order
            const int32_t to = path[(size_t)t + 1];
            bool in_row = false;
            for (int64_t e = r.indptr[(size_t)l]; e < r.indptr[(size_t)l + 1]; ++e)
                in_row = in_row || r.indices[(size_t)e] == to;
            CHECK(to < 0 ? r.indptr[(size_t)l] == r.indptr[(size_t)l + 1] : in_row);
        }
        CHECK(sum == top);
    }
    return 0;
}

// the relation's own checks through the shared check_csr, named for this entry point
int test_relation() {
    ehm_err_channel err;
    Rng rng{3};
    Relation r = random_relation(7, rng);
    std::vector<int32_t> ptr32;
    CHECK(ehm_reach::check_csr(err, "cost", 7, (int64_t)r.indices.size(), 7, r.indptr.data(),
                               r.indices.data(), ptr32) == EHM_OK);
    CHECK(ptr32.size() == 8 && ptr32[7] == (int32_t)r.indices.size());
    r.indices[2] = 7;
    CHECK(ehm_reach::check_csr(err, "cost", 7, (int64_t)r.indices.size(), 7, r.indptr.data(),
                               r.indices.data(), ptr32) == EHM_E_INVALID &&
          says(err, "cost: indices[2] = 7 of 7"));
    return 0;
}

}  // namespace

int main() {
    if (test_keys() || test_refusals() || test_domain_verdict() || test_paths() || test_relation())
        return 1;
    std::printf("cost host helpers: ok\n");
    return 0;
}
