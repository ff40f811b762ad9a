// Drives the host-side bookkeeping of csrc/ehm_certify.hip (ehm_certify_host.h) on the CPU: the
// parent table, the turn set, the bisected-edge rule, the leaf-id check, and the certificate's
// status, candidate order and worst-leaf rule.  Built with
// -fsanitize=address,undefined by tests/test_host_certify.py; needs no device and no library.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../explicit_hybrid_mpc_amd/csrc/ehm_certify_host.h"

using namespace ehm_cert;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("%s:%d: %s fails\n", __FILE__, __LINE__, #cond);   \
            return 1;                                                      \
        }                                                                  \
    } while (0)

namespace {

// a law's child pairs in both layouts: record k holds p + 1 plane values, then the pair
struct Tree {
    int p, stride64, stride32;
    std::vector<double> node64;
    std::vector<float> node32;
    std::vector<int32_t> root_entry;
    int32_t n_int = 0, n_leaf = 0;

    explicit Tree(int p_) : p(p_), stride64(p_ <= 6 ? 8 : 16), stride32(p_ <= 5 ? 8 : 16) {}
    int32_t add(int32_t left, int32_t right) {
        node64.resize((size_t)(n_int + 1) * stride64, 0.0);
        node32.resize((size_t)(n_int + 1) * stride32, 0.0f);
        const int32_t ch[2] = {left, right};
        __builtin_memcpy(&node64[(size_t)n_int * stride64 + p + 1], ch, sizeof ch);
        __builtin_memcpy(&node32[(size_t)n_int * stride32 + p + 1], ch, sizeof ch);
        return n_int++;
    }
};

struct Table {
    std::vector<int32_t> node, leaf;
    std::vector<uint8_t> node_side, leaf_side;
    Table(int32_t n_int, int32_t n_leaf)
        : node(n_int, EHM_CERT_UNREACHED), leaf(n_leaf, EHM_CERT_UNREACHED), node_side(n_int, 0),
          leaf_side(n_leaf, 0) {}
    Parents view() { return Parents{node.data(), node_side.data(), leaf.data(), leaf_side.data()}; }
};

template <class T>
void link(const Tree& t, const std::vector<T>& node, int stride, Table& tab) {
    const Parents P = tab.view();
    for (int32_t k = 0; k < t.n_int; ++k) {
        int32_t l, r;
        children_of(&node[(size_t)k * stride], t.p, l, r);
        link_children(P, k, l, r);
    }
    for (size_t r = 0; r < t.root_entry.size(); ++r) link_root(P, (int32_t)r, t.root_entry[r]);
}

// a chain of `depth` internal records under root 1 (root 0 is leaf 0 itself): record k has a leaf
// on the side turn(k) and the next record on the other; leaf ids in the order they are made
int chain_case(int p, int depth) {
    Tree t(p);
    auto turn = [](int k) { return (k * 7 + k / 3) & 1; };
    t.n_leaf = 1;
    for (int k = 0; k < depth; ++k) {
        const int32_t leaf = ~t.n_leaf++;
        const int32_t next = k + 1 < depth ? k + 1 : ~t.n_leaf++;
        // the chain goes on on side turn(k)
        t.add(turn(k) ? leaf : next, turn(k) ? next : leaf);
    }
    t.root_entry = {~0, 0};
    const int32_t spare = t.n_leaf++;       // a leaf record nothing names
    for (int prec = 0; prec < 2; ++prec) {
        Table tab(t.n_int, t.n_leaf);
        if (prec) link(t, t.node32, t.stride32, tab);
        else link(t, t.node64, t.stride64, tab);
        const Parents P = tab.view();
        TurnSet ts;
        int32_t root = -1;
        CHECK(walk_up(P, 0, ts, root) && root == 0 && ts.depth == 0);
        ts = TurnSet();
        CHECK(!walk_up(P, spare, ts, root));
        // the side leaf of record k is leaf k + 1, k + 1 levels down; the last leaf is `depth` down
        for (int32_t l = 1; l <= depth + 1; ++l) {
            const int levels = l <= depth ? l : depth;
            ts = TurnSet();
            root = -1;
            const bool ok = walk_up(P, l, ts, root);
            CHECK(ok == (levels <= EHM_CERT_MAX_DEPTH));
            if (!ok) continue;
            CHECK(root == 1 && ts.depth == levels);
            for (int k = 0; k < levels; ++k) {
                const bool side_leaf = l <= depth && k == levels - 1;
                CHECK(ts.pop() == (side_leaf ? 1 - turn(k) : turn(k)));
            }
            CHECK(ts.depth == 0 && ts.w0 == 0 && ts.w1 == 0 && ts.w2 == 0 && ts.w3 == 0);
        }
    }
    return 0;
}

int turn_set_case() {
    TurnSet ts;
    std::vector<int> bits;
    unsigned x = 12345;
    for (int i = 0; i < EHM_CERT_MAX_DEPTH; ++i) {
        x = x * 1664525u + 1013904223u;
        bits.push_back((x >> 16) & 1);
        CHECK(ts.push(bits.back()));
    }
    CHECK(!ts.push(1) && ts.depth == EHM_CERT_MAX_DEPTH);
    for (int i = EHM_CERT_MAX_DEPTH - 1; i >= 0; --i) CHECK(ts.pop() == bits[i]);
    CHECK(ts.depth == 0);
    return 0;
}

int edge_case() {
    int pos, neg;
    const double a[4] = {0.0, 1.0, -1.0, 1e-9};
    CHECK(bisected_edge<4>(a, pos, neg) && pos == 1 && neg == 2);
    const double b[3] = {0.963, -0.963, 0.037};
    CHECK(bisected_edge<3>(b, pos, neg) && pos == 0 && neg == 1);
    const double c[3] = {1.0, 1.0, -1.0};
    CHECK(!bisected_edge<3>(c, pos, neg));
    const double d[3] = {0.25, -0.25, 0.0};
    CHECK(!bisected_edge<3>(d, pos, neg));
    const double e[2] = {NAN, -1.0};
    CHECK(!bisected_edge<2>(e, pos, neg));
    const double f[9] = {0, 0, 0, 0, -1.0, 0, 0, 0, 1.0};
    CHECK(bisected_edge<9>(f, pos, neg) && pos == 8 && neg == 4);
    return 0;
}

int leaf_id_case() {
    const std::vector<int32_t> ids = {0, 4, 2, 4};
    CHECK(first_bad_leaf(ids.data(), 4, 5) == -1);
    CHECK(first_bad_leaf(ids.data(), 4, 4) == 1);
    CHECK(first_bad_leaf(ids.data(), 0, 0) == -1);
    const std::vector<int32_t> neg = {1, -1};
    CHECK(first_bad_leaf(neg.data(), 2, 5) == 1);
    return 0;
}

// the certificate's bookkeeping: the status of a leaf, the order of the tries, the worst leaf
int certificate_case() {
    CHECK(certify_status(0, 1, 3, 1, 1) == CERT_NO_CELL);
    CHECK(certify_status(1, 1, 3, 1, 1) == CERT_NO_LAW);
    CHECK(certify_status(1, 0, 3, 1, 1) == CERT_CERTIFIED);
    CHECK(certify_status(1, 0, 0, 0, 0) == CERT_INADMISSIBLE);
    CHECK(certify_status(1, 0, 2, 1, 0) == CERT_STALLED);
    CHECK(certify_status(1, 0, 2, 0, 0) == CERT_UNCERTIFIED);
    const double W[3] = {1e16, 1.0, -1e16};
    CHECK(candidate_key(W, 3) == 0.0);              // ((0 + 1e16) + 1) - 1e16: the order is fixed
    CHECK(candidate_key(W, 0) == 0.0);
    const double key[6] = {3.0, 1.0, 2.0, 1.0, NAN, 0.5};
    std::vector<int32_t> order(6, -1);
    order_candidates(6, key, order.data());
    const int32_t want[6] = {5, 1, 3, 2, 0, 4};     // ties by position, a NaN last
    for (int i = 0; i < 6; ++i) CHECK(order[i] == want[i]);
    order_candidates(0, key, order.data());
    std::vector<int32_t> one(1, -1);
    order_candidates(1, key, one.data());
    CHECK(one[0] == 0);
    CHECK(worst_beats(2.0, 7, 1.0, 3) && !worst_beats(1.0, 3, 2.0, 7));
    CHECK(worst_beats(1.0, 3, 1.0, 7) && !worst_beats(1.0, 7, 1.0, 3));
    CHECK(!worst_beats(NAN, 0, 1.0, 3));
    return 0;
}

}  // namespace

int main() {
    if (turn_set_case() || edge_case() || leaf_id_case() || certificate_case()) return 1;
    for (int p : {1, 5, 6, 8})
        for (int depth : {1, 2, 63, 64, 65, 255, 256, 257, 300})
            if (chain_case(p, depth)) return 1;
    std::printf("certify host helpers: ok\n");
    return 0;
}
