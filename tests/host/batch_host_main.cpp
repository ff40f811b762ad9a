// Stand-alone check of csrc/ehm_batch_host.h (built and run by tests/test_host_batch_rows.py with
// the address and undefined-behaviour sanitizers): every helper against a straightforward loop
// written here.  Exit status 0 = all checks passed; a failed check prints its line.
#include "ehm_batch_host.h"

#include <cstdio>
#include <cstdlib>

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "line %d: %s [%s]\n", __LINE__, #cond, g_case); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

static const char* g_case = "";

// xorshift64*: a seeded stream without the library's distributions
struct Rng {
    uint64_t s;
    uint64_t next() {
        s ^= s >> 12;
        s ^= s << 25;
        s ^= s >> 27;
        return s * 0x2545F4914F6CDD1DULL;
    }
};

static void check_sort(int nd, const std::vector<int32_t>& didx) {
    const int64_t n = (int64_t)didx.size();
    std::vector<int64_t> order;
    std::vector<int32_t> seg;
    sort_by_commutation(nd, n, didx.data(), order, seg);
    // the segment table
    CHECK(seg.size() == (size_t)nd + 1);
    CHECK(seg.front() == 0 && seg.back() == n);
    for (int d = 0; d < nd; ++d) {
        CHECK(seg[d] <= seg[d + 1]);
        int32_t count = 0;
        for (int64_t k = 0; k < n; ++k) count += didx[k] == d;
        CHECK(seg[d + 1] - seg[d] == count);
    }
    // order: a permutation, grouped by commutation, stable within one
    CHECK(order.size() == (size_t)n);
    std::vector<int> seen((size_t)n, 0);
    for (int64_t k = 0; k < n; ++k) {
        CHECK(order[k] >= 0 && order[k] < n);
        CHECK(seen[order[k]]++ == 0);
    }
    for (int d = 0; d < nd; ++d)
        for (int32_t k = seg[d]; k < seg[d + 1]; ++k) {
            CHECK(didx[order[k]] == d);
            if (k > seg[d]) CHECK(order[k - 1] < order[k]);
        }
    // rows there and back
    for (size_t width : {1, 3, 20}) {
        std::vector<double> x((size_t)n * width), want((size_t)n * width);
        for (size_t q = 0; q < x.size(); ++q) x[q] = 0.5 * (double)q - 7.0;
        for (int64_t k = 0; k < n; ++k)
            for (size_t c = 0; c < width; ++c) want[k * width + c] = x[order[k] * width + c];
        std::vector<double> g(x.size(), -1.0), back(x.size(), -2.0);
        gather_rows(g.data(), x.data(), order, width);
        CHECK(g == want);
        CHECK(gathered(x.data(), order, width) == want);
        scatter_rows(back.data(), g.data(), order, width);
        CHECK(back == x);
    }
    // where: the ascending indices of a predicate
    const std::vector<int64_t> odd = where(n, [&](int64_t k) { return didx[k] % 2 == 1; });
    size_t n_odd = 0;
    for (int64_t k = 0; k < n; ++k)
        if (didx[k] % 2 == 1) CHECK(n_odd < odd.size() && odd[n_odd++] == k);
    CHECK(n_odd == odd.size());
    // other element types; a subset leaves the other rows alone
    std::vector<int64_t> sub;
    for (int64_t k = 0; k < n; k += 3) sub.push_back(n - 1 - k);
    std::vector<int32_t> picked = gathered(didx.data(), sub, 1);
    CHECK(picked.size() == sub.size());
    for (size_t k = 0; k < sub.size(); ++k) CHECK(picked[k] == didx[sub[k]]);
    std::vector<char> bytes((size_t)n * 5, 'a'), rows(sub.size() * 5, 'b');
    scatter_rows(bytes.data(), rows.data(), sub, 5);
    std::vector<char> hit((size_t)n, 0);
    for (int64_t s : sub) hit[s] = 1;
    for (int64_t k = 0; k < n; ++k)
        for (int c = 0; c < 5; ++c) CHECK(bytes[k * 5 + c] == (hit[k] ? 'b' : 'a'));
}

// the merge of a retried subset: rows whose retry has status 0 are taken, the others kept
static void check_merge(const std::vector<int32_t>& status) {
    const size_t n = 40, width = 3, nb = status.size();
    std::vector<int64_t> idx(nb);
    for (size_t k = 0; k < nb; ++k) idx[k] = (int64_t)((7 * k + 3) % n);    // distinct for nb <= n
    std::vector<double> full(n * width), retry(nb * width);
    for (size_t q = 0; q < full.size(); ++q) full[q] = (double)q;
    for (size_t q = 0; q < retry.size(); ++q) retry[q] = -1.0 - (double)q;
    std::vector<double> want = full;
    int64_t n_ok = 0;
    for (size_t k = 0; k < nb; ++k) {
        if (status[k] != 0) continue;
        ++n_ok;
        for (size_t c = 0; c < width; ++c) want[idx[k] * width + c] = retry[k * width + c];
    }
    CHECK(merge_retried(full.data(), retry.data(), idx, status.data(), width) == n_ok);
    CHECK(full == want);
}

int main() {
    g_case = "n = 0";
    check_sort(1, {});
    check_sort(5, {});
    g_case = "n = 1";
    check_sort(1, {0});
    check_sort(4, {2});
    g_case = "one commutation";
    check_sort(1, std::vector<int32_t>(37, 0));
    check_sort(6, std::vector<int32_t>(37, 4));
    g_case = "nd = 256, most empty";
    {
        std::vector<int32_t> d;
        for (int k = 0; k < 90; ++k) d.push_back((k % 3 == 0) ? 255 : (k % 3 == 1) ? 17 : 0);
        check_sort(256, d);
    }
    g_case = "random, n = 1000, nd = 7";
    {
        Rng rng{20240607};
        std::vector<int32_t> d(1000);
        for (int32_t& v : d) v = (int32_t)(rng.next() % 7);
        check_sort(7, d);
    }
    g_case = "merge: none converged";
    check_merge({3, 1, 2, 1});
    g_case = "merge: some converged";
    check_merge({0, 1, 0, 0, 5, 0});
    g_case = "merge: all converged";
    check_merge({0, 0, 0, 0, 0});
    g_case = "merge: empty";
    check_merge({});
    std::puts("batch host helpers ok");
    return 0;
}
