// Drives the host checks of csrc/ehm_reach.hip (ehm_reach_host.h) on the CPU: what is refused of a
// relation, a start set and the options (each with its message), the narrowing of indptr, the start
// mask, and what the host reads off the per-step counters, on random relations against a plain
// breadth-first restatement.  Built with -fsanitize=address,undefined by tests/test_host_reach.py;
// needs no device and no library.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../explicit_hybrid_mpc_amd/csrc/ehm_reach_host.h"

using namespace ehm_reach;

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

// a relation over n leaves in exactly sized heap arrays, so that a read past an end is seen
struct Relation {
    std::vector<int64_t> indptr;
    std::vector<int32_t> indices, level, start;
    ehm_reach_opts opts() const {
        ehm_reach_opts o;
        std::memset(&o, 0, sizeof o);
        o.indptr = indptr.data();
        o.indices = indices.data();
        o.level = level.data();
        o.start = start.data();
        o.n_leaf = (int64_t)level.size();
        o.n_edges = (int64_t)indices.size();
        o.n_level = (int64_t)level.size();
        o.n_start = (int64_t)start.size();
        o.max_sweeps = o.n_leaf;
        return o;
    }
};

Relation random_relation(int n, Rng& rng) {
    Relation r;
    r.indptr.push_back(0);
    for (int l = 0; l < n; ++l) {
        const int w = (int)(rng.next() % 4);
        for (int k = 0; k < w; ++k) r.indices.push_back((int32_t)(rng.next() % (unsigned)n));
        r.indptr.push_back((int64_t)r.indices.size());
        r.level.push_back(rng.next() % 10 == 0 ? 0 : -1);
    }
    r.start.push_back((int32_t)(rng.next() % (unsigned)n));
    r.start.push_back((int32_t)(rng.next() % (unsigned)n));
    return r;
}

bool says(const ehm_err_channel& err, const char* what) {
    return std::strstr(err.c_str(), what) != nullptr;
}

// phase A by sweeps on the host, with the counters the device would leave: fresh[k]
void sweeps(const Relation& r, const std::vector<int32_t>& ptr, const std::vector<uint8_t>& mask,
            std::vector<int32_t>& arrival, std::vector<unsigned long long>& fresh, int64_t cap) {
    const int64_t n = (int64_t)r.level.size();
    arrival.assign((size_t)n, -1);
    fresh.assign((size_t)cap + 1, 0);
    for (int64_t l = 0; l < n; ++l)
        if (mask[(size_t)l]) {
            arrival[(size_t)l] = 0;
            ++fresh[0];
        }
    for (int64_t k = 1; k <= cap; ++k)
        for (int64_t l = 0; l < n; ++l) {
            if (arrival[(size_t)l] != k - 1 || r.level[(size_t)l] == 0) continue;
            for (int32_t e = ptr[(size_t)l]; e < ptr[(size_t)l + 1]; ++e) {
                int32_t& a = arrival[(size_t)r.indices[(size_t)e]];
                if (a < 0) {
                    a = (int32_t)k;
                    ++fresh[(size_t)k];
                }
            }
        }
}

}  // namespace

int main() {
    Rng rng{12345u};
    ehm_err_channel err;
    for (int trial = 0; trial < 200; ++trial) {
        const int n = 1 + (int)(rng.next() % 40);
        Relation r = random_relation(n, rng);
        ehm_reach_opts o = r.opts();
        std::vector<int32_t> ptr;
        std::vector<uint8_t> mask;
        CHECK(check_options(err, &o, n) == EHM_OK);
        CHECK(check_relation(err, &o, ptr) == EHM_OK);
        CHECK(ptr.size() == (size_t)n + 1);
        for (int l = 0; l <= n; ++l) CHECK((int64_t)ptr[(size_t)l] == r.indptr[(size_t)l]);
        CHECK(start_mask(err, &o, mask) == EHM_OK);
        int marked = 0;
        for (int l = 0; l < n; ++l) marked += mask[(size_t)l];
        CHECK(marked == (r.start[0] == r.start[1] ? 1 : 2));
        CHECK(mask[(size_t)r.start[0]] == 1 && mask[(size_t)r.start[1]] == 1);

        // the counters against the arrival they belong to
        std::vector<int32_t> arrival;
        std::vector<unsigned long long> fresh;
        sweeps(r, ptr, mask, arrival, fresh, n);
        bool done = false;
        int64_t n_arrival = -1;
        arrival_outcome(fresh.data(), n, done, n_arrival);
        int32_t top = 0;
        for (int l = 0; l < n; ++l) top = arrival[(size_t)l] > top ? arrival[(size_t)l] : top;
        CHECK(done && n_arrival == top);                    // n sweeps always suffice
        if (top >= 1) {
            arrival_outcome(fresh.data(), top, done, n_arrival);
            CHECK(!done && n_arrival == top);
        }
        int64_t leak = -1;
        for (int l = 0; l < n; ++l)
            if (r.level[(size_t)l] == 0 && arrival[(size_t)l] >= 0 &&
                (leak < 0 || arrival[(size_t)l] < leak))
                leak = arrival[(size_t)l];
        CHECK(leak_step(arrival.data(), r.level.data(), n) == leak);

        // every refusal, on a copy that is wrong in one place
        if (n >= 2 && r.indptr[(size_t)n] > r.indptr[1]) {
            Relation b = r;
            int l = 1;
            while (b.indptr[(size_t)l + 1] == b.indptr[(size_t)l]) ++l;    // a row that is not empty
            b.indptr[(size_t)l] = b.indptr[(size_t)l + 1] + 1;
            o = b.opts();
            // row l - 1 now ends past row l's end: the decrease is at row l
            CHECK(check_relation(err, &o, ptr) == EHM_E_INVALID && says(err, "decreases"));
        }
        if (!r.indices.empty()) {
            Relation b = r;
            b.indices[rng.next() % b.indices.size()] = (rng.next() & 1) ? n : -1;
            o = b.opts();
            CHECK(check_relation(err, &o, ptr) == EHM_E_INVALID && says(err, "indices["));
            b = r;
            o = b.opts();
            o.n_edges -= 1;
            CHECK(check_relation(err, &o, ptr) == EHM_E_INVALID && says(err, "indptr ends at"));
        }
        {
            Relation b = r;
            b.indptr[0] = 1;
            o = b.opts();
            CHECK(check_relation(err, &o, ptr) == EHM_E_INVALID &&
                  (says(err, "indptr[0]")));
            o = r.opts();
            o.n_level = n + 1;
            CHECK(check_relation(err, &o, ptr) == EHM_E_INVALID && says(err, "level array"));
            o = r.opts();
            o.n_start = 0;
            CHECK(start_mask(err, &o, mask) == EHM_E_INVALID && says(err, "empty"));
            b = r;
            b.start[1] = (rng.next() & 1) ? n : -1;
            o = b.opts();
            CHECK(start_mask(err, &o, mask) == EHM_E_INVALID && says(err, "start[1]"));
        }
    }
    {
        Relation r = random_relation(5, rng);
        ehm_reach_opts o = r.opts();
        o.horizon = -1;
        CHECK(check_options(err, &o, 5) == EHM_E_INVALID && says(err, "horizon"));
        o = r.opts();
        o.max_sweeps = 0;
        CHECK(check_options(err, &o, 5) == EHM_E_INVALID && says(err, "max_sweeps"));
        o = r.opts();
        o.row_map = 2;
        CHECK(check_options(err, &o, 5) == EHM_E_INVALID && says(err, "row_map"));
        o = r.opts();
        CHECK(check_options(err, &o, 4) == EHM_E_INVALID && says(err, "n_leaf"));
        o.n_leaf = 0;
        CHECK(check_options(err, &o, 5) == EHM_E_INVALID && says(err, "n_leaf"));
        o = r.opts();
        o.want_steps = 1;
        o.horizon = (int32_t)(MAX_STEP_BYTES / 5);          // (horizon + 1) 5 > 2^28
        CHECK(check_options(err, &o, 5) == EHM_E_INVALID && says(err, "2^28"));
        o.horizon -= 1;
        CHECK(check_options(err, &o, 5) == EHM_OK);
        o.n_edges = (int64_t)1 << 31;
        std::vector<int32_t> ptr;
        CHECK(check_relation(err, &o, ptr) == EHM_E_INVALID && says(err, "n_edges"));
    }
    {
        // phase B's counters: D_j of sizes 7 6 5 4 3 3 (a tail of 4 into a 3-cycle), then an empty end
        const unsigned long long size[] = {7, 6, 5, 4, 3, 3, 3}, gone[] = {0, 1, 1, 1, 1, 0, 0};
        bool done = false;
        int64_t settle = -1;
        settle_outcome(size, gone, 6, done, settle);
        CHECK(done && settle == 4);
        settle_outcome(size, gone, 4, done, settle);
        CHECK(!done && settle == 4);
        settle_outcome(size, gone, 2, done, settle);
        CHECK(!done && settle == 2);
        const unsigned long long size0[] = {2, 1, 0, 0}, gone0[] = {0, 1, 1, 0};
        settle_outcome(size0, gone0, 3, done, settle);
        CHECK(done && settle == 2);
        CHECK(last_step(10, -1, true, 3) == 10 && last_step(10, 4, true, 3) == 4);
        CHECK(last_step(10, -1, false, 3) == 3 && last_step(2, 4, false, 3) == 2);
        CHECK(last_step(0, 0, true, 1) == 0);
    }
    std::printf("reach host helpers: ok\n");
    return 0;
}
