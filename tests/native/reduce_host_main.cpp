// Drives the host-side bookkeeping of csrc/ehm_reduce.hip (ehm_reduce_host.h) on the CPU: the forest
// check, the representative walk, the topmost-mergeable-ancestor rule, the survivors and the
// renumbering, on random forests against their plain restatement by recursion.  Built with
// -fsanitize=address,undefined by tests/test_host_reduce.py; needs no device and no library.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../explicit_hybrid_mpc_amd/csrc/ehm_reduce_host.h"

using namespace ehm_cert;
using namespace ehm_red;

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

// a forest of n_roots roots grown by n_split splits of random leaves; children come after parents
struct Forest {
    std::vector<int32_t> left, right;       // per internal record: >= 0 internal, ~leaf
    std::vector<int32_t> root_entry;
    int32_t n_leaf = 0;

    Forest(int n_roots, int n_split, Rng& rng) {
        // grow on nodes, then number internal records and leaves in node order
        std::vector<int> l(n_roots, -1), r(n_roots, -1);
        for (int s = 0; s < n_split; ++s) {
            std::vector<int> open;
            for (size_t k = 0; k < l.size(); ++k)
                if (l[k] < 0) open.push_back((int)k);
            const int k = open[rng.next() % open.size()];
            l[k] = (int)l.size();
            r[k] = (int)l.size() + 1;
            l.insert(l.end(), 2, -1);
            r.insert(r.end(), 2, -1);
        }
        std::vector<int32_t> id(l.size());
        int32_t n_int = 0;
        for (size_t k = 0; k < l.size(); ++k) id[k] = l[k] < 0 ? ~n_leaf++ : n_int++;
        for (size_t k = 0; k < l.size(); ++k)
            if (l[k] >= 0) {
                left.push_back(id[(size_t)l[k]]);
                right.push_back(id[(size_t)r[k]]);
            }
        for (int k = 0; k < n_roots; ++k) root_entry.push_back(id[(size_t)k]);
    }
    int32_t n_int() const { return (int32_t)left.size(); }
};

struct Table {
    std::vector<int32_t> node, leaf;
    std::vector<uint8_t> node_side, leaf_side;
    explicit Table(const Forest& f)
        : node((size_t)f.n_int(), EHM_CERT_UNREACHED), leaf((size_t)f.n_leaf, EHM_CERT_UNREACHED),
          node_side((size_t)f.n_int(), 0), leaf_side((size_t)f.n_leaf, 0) {
        const Parents P = view();
        for (int32_t k = 0; k < f.n_int(); ++k)
            link_children(P, k, f.left[(size_t)k], f.right[(size_t)k]);
        for (size_t r = 0; r < f.root_entry.size(); ++r)
            link_root(P, (int32_t)r, f.root_entry[r]);
    }
    Parents view() { return Parents{node.data(), node_side.data(), leaf.data(), leaf_side.data()}; }
};

bool forest_ok(const Forest& f, Table& t) {
    const Parents P = t.view();
    bool ok = true;
    for (int32_t k = 0; k < f.n_int(); ++k)
        ok = ok && names_its_children(P, k, f.left[(size_t)k], f.right[(size_t)k]);
    for (size_t r = 0; r < f.root_entry.size(); ++r)
        ok = ok && root_names_entry(P, (int32_t)r, f.root_entry[r]);
    return ok;
}

int32_t leftmost(const Forest& f, int32_t c) {
    while (c >= 0) c = f.left[(size_t)c];
    return ~c;
}

// the reduced forest by recursion from the roots: (new id of the entry); appends to the new arrays
int32_t rebuild(const Forest& f, const std::vector<uint8_t>& open, int32_t c,
                std::vector<int32_t>& kept_int, std::vector<int32_t>& kept_leaf) {
    if (c < 0) {
        kept_leaf.push_back(~c);
        return 0;
    }
    if (!open[(size_t)c]) {
        kept_leaf.push_back(leftmost(f, c));
        return 0;
    }
    kept_int.push_back(c);
    rebuild(f, open, f.left[(size_t)c], kept_int, kept_leaf);
    rebuild(f, open, f.right[(size_t)c], kept_int, kept_leaf);
    return 0;
}

int random_case(int n_roots, int n_split, unsigned seed) {
    Rng rng{seed};
    Forest f(n_roots, n_split, rng);
    Table t(f);
    const Parents P = t.view();
    CHECK(forest_ok(f, t));
    const int32_t n_int = f.n_int(), n_leaf = f.n_leaf;
    // representatives
    std::vector<int32_t> rep((size_t)n_int, -1);
    for (int32_t l = 0; l < n_leaf; ++l) mark_representative(P, l, rep.data());
    for (int32_t a = 0; a < n_int; ++a) CHECK(rep[(size_t)a] == leftmost(f, a));
    // random flags; a quarter of the cases all mergeable, a quarter none
    std::vector<uint8_t> open((size_t)n_int + 1, 0);
    const unsigned kind = seed % 4;
    for (int32_t a = 0; a < n_int; ++a)
        open[(size_t)a] = kind == 0 ? 0 : kind == 1 ? 1 : (uint8_t)(rng.next() % 3 == 0);
    // survivors against the recursion
    std::vector<int32_t> kept_int, kept_leaf;
    for (int32_t e : f.root_entry) rebuild(f, open, e, kept_int, kept_leaf);
    std::vector<uint8_t> in_int((size_t)n_int, 0), in_leaf((size_t)n_leaf, 0);
    for (int32_t a : kept_int) in_int[(size_t)a] = 1;
    for (int32_t l : kept_leaf) in_leaf[(size_t)l] = 1;
    std::vector<int32_t> new_int((size_t)n_int, 0), new_leaf((size_t)n_leaf, 0), target((size_t)n_leaf);
    int32_t m_int = 0, m_leaf = 0;
    for (int32_t a = 0; a < n_int; ++a) {
        CHECK(internal_survives(P, a, open.data()) == (in_int[(size_t)a] != 0));
        new_int[(size_t)a] = m_int;
        m_int += in_int[(size_t)a];
    }
    for (int32_t l = 0; l < n_leaf; ++l) {
        target[(size_t)l] = leaf_target(P, l, open.data(), rep.data());
        CHECK((target[(size_t)l] == l) == (in_leaf[(size_t)l] != 0));
        CHECK(in_leaf[(size_t)target[(size_t)l]]);
        new_leaf[(size_t)l] = m_leaf;
        m_leaf += in_leaf[(size_t)l];
    }
    CHECK(m_leaf >= (int32_t)f.root_entry.size() || m_int > 0);
    // the renumbered forest is a forest again, with children after their parents, and every
    // original leaf's target lies below the renumbered path of its own root
    Forest g = f;
    g.left.assign((size_t)m_int, 0);
    g.right.assign((size_t)m_int, 0);
    g.n_leaf = m_leaf;
    for (int32_t a = 0; a < n_int; ++a) {
        if (!in_int[(size_t)a]) continue;
        const int32_t at = new_int[(size_t)a];
        g.left[(size_t)at] = renumber(f.left[(size_t)a], open.data(), rep.data(), new_int.data(), new_leaf.data());
        g.right[(size_t)at] = renumber(f.right[(size_t)a], open.data(), rep.data(), new_int.data(), new_leaf.data());
        for (int32_t c : {g.left[(size_t)at], g.right[(size_t)at]})
            CHECK(c >= 0 ? (c > at && c < m_int) : (~c < m_leaf));
    }
    for (size_t r = 0; r < f.root_entry.size(); ++r) {
        g.root_entry[r] = renumber(f.root_entry[r], open.data(), rep.data(), new_int.data(), new_leaf.data());
        CHECK(g.root_entry[r] >= 0 ? g.root_entry[r] < m_int : ~g.root_entry[r] < m_leaf);
    }
    Table u(g);
    CHECK(forest_ok(g, u));
    // same root above a leaf and above the leaf that stands for it
    const Parents Q = u.view();
    for (int32_t l = 0; l < n_leaf; ++l) {
        TurnSet a, b;
        int32_t ra = -1, rb = -1;
        CHECK(walk_up(P, l, a, ra));
        CHECK(walk_up(Q, new_leaf[(size_t)target[(size_t)l]], b, rb));
        CHECK(ra == rb && b.depth <= a.depth);
    }
    if (kind == 0) CHECK(m_int == 0 && m_leaf == (int32_t)f.root_entry.size());
    if (kind == 1) CHECK(m_int == n_int && m_leaf == n_leaf);
    return 0;
}

// a record named twice and a root that is also a child are no forest
int broken_case() {
    Rng rng{7};
    Forest f(2, 5, rng);
    {
        Forest g = f;
        g.right[0] = g.left[0];
        Table t(g);
        CHECK(!forest_ok(g, t));
    }
    {
        Forest g = f;
        g.root_entry[1] = g.left[0];
        Table t(g);
        CHECK(!forest_ok(g, t));
    }
    {
        Forest g = f;
        g.root_entry[1] = g.root_entry[0];
        Table t(g);
        CHECK(!forest_ok(g, t));
    }
    return 0;
}

}  // namespace

int main() {
    if (broken_case()) return 1;
    for (int n_roots : {1, 2, 7})
        for (int n_split : {0, 1, 2, 9, 40, 300})
            for (unsigned seed = 0; seed < 8; ++seed)
                if (random_case(n_roots, n_split, seed * 4 + seed % 4 + 4 * (unsigned)n_split))
                    return 1;
    std::printf("reduce host helpers: ok\n");
    return 0;
}
