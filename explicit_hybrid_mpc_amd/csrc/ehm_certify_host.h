// The bookkeeping of ehm_certify.hip that needs no device: the parent table of a
// compiled law, the set of turns a leaf's walk up to its root records, the rule that finds the
// bisected edge of a cell at a plane node, and the check of the caller's leaf ids.  Plain C++ that
// the kernels inline and a host program can drive (tests/native/certify_host_main.cpp runs it
// under the address and undefined-behaviour sanitizers).
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define EHM_CERT_HD __host__ __device__ __forceinline__
#define EHM_CERT_UNROLL _Pragma("unroll")
#else
#define EHM_CERT_HD inline
#define EHM_CERT_UNROLL
#endif

#define EHM_CERT_MAX_DEPTH 256                      // EHM_CELL_MAX_DEPTH of include/ehmpc.h
#define EHM_CERT_UNREACHED ((int32_t)0x80000000)    // parent of a record no root reaches

namespace ehm_cert {

// The turns of a path, root first out: push on the way up (the deepest turn first), pop on the way
// down.  256 bits in four words that are only ever indexed statically, so they stay in registers.
struct TurnSet {
    uint64_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    int depth = 0;

    // false (and nothing changes) when the set is full
    EHM_CERT_HD bool push(int bit) {
        if (depth >= EHM_CERT_MAX_DEPTH) return false;
        w3 = (w3 << 1) | (w2 >> 63);
        w2 = (w2 << 1) | (w1 >> 63);
        w1 = (w1 << 1) | (w0 >> 63);
        w0 = (w0 << 1) | (uint64_t)(bit & 1);
        ++depth;
        return true;
    }
    // the turn pushed last; the set must not be empty
    EHM_CERT_HD int pop() {
        const int bit = (int)(w0 & 1);
        w0 = (w0 >> 1) | (w1 << 63);
        w1 = (w1 >> 1) | (w2 << 63);
        w2 = (w2 >> 1) | (w3 << 63);
        w3 = w3 >> 1;
        --depth;
        return bit;
    }
};

// The parent table: for internal records and leaf records the parent's index (>= 0) with the side
// the child hangs on (0 left, 1 right), ~root for the entry of a root, EHM_CERT_UNREACHED else.
struct Parents {
    int32_t* node;
    uint8_t* node_side;
    int32_t* leaf;
    uint8_t* leaf_side;
};

// (left, right) of an internal record: a double law packs them into the double after b, a single
// law keeps them in the two floats after b
EHM_CERT_HD void children_of(const double* rec, int p, int32_t& left, int32_t& right) {
    int32_t ch[2];
    __builtin_memcpy(ch, rec + p + 1, sizeof ch);
    left = ch[0];
    right = ch[1];
}
EHM_CERT_HD void children_of(const float* rec, int p, int32_t& left, int32_t& right) {
    int32_t ch[2];
    __builtin_memcpy(ch, rec + p + 1, sizeof ch);
    left = ch[0];
    right = ch[1];
}

// what internal record k writes: itself as the parent of its two children
EHM_CERT_HD void link_children(const Parents& P, int32_t k, int32_t left, int32_t right) {
    const int32_t ch[2] = {left, right};
    for (int side = 0; side < 2; ++side) {
        const int32_t c = ch[side];
        if (c >= 0) {
            P.node[c] = k;
            P.node_side[c] = (uint8_t)side;
        } else {
            P.leaf[~c] = k;
            P.leaf_side[~c] = (uint8_t)side;
        }
    }
}

// what root r writes for its entry (an internal record or ~leaf)
EHM_CERT_HD void link_root(const Parents& P, int32_t r, int32_t entry) {
    if (entry >= 0) P.node[entry] = ~r;
    else P.leaf[~entry] = ~r;
}

// From leaf record l up to its root: the turns into `turns`, the root into `root`.  False for a
// leaf no root reaches and for one deeper than the set holds.  Children come after their parents,
// so the index falls strictly and the walk ends.
EHM_CERT_HD bool walk_up(const Parents& P, int32_t l, TurnSet& turns, int32_t& root) {
    int32_t up = P.leaf[l];
    int side = P.leaf_side[l];
    while (up >= 0) {
        if (!turns.push(side)) return false;
        side = P.node_side[up];
        up = P.node[up];
    }
    if (up == EHM_CERT_UNREACHED) return false;
    root = ~up;
    return true;
}

// The two ends of the edge a plane node bisects, by the plane's values s [N] at the cell's vertices:
// exactly one above 0.5 (`pos`) and exactly one below -0.5 (`neg`), else false (a NaN is neither).
template <int N>
EHM_CERT_HD bool bisected_edge(const double (&s)[N], int& pos, int& neg) {
    int np_ = 0, nn = 0;
    pos = neg = -1;
    EHM_CERT_UNROLL
    for (int i = 0; i < N; ++i) {
        if (s[i] > 0.5) {
            ++np_;
            pos = i;
        }
        if (s[i] < -0.5) {
            ++nn;
            neg = i;
        }
    }
    return np_ == 1 && nn == 1;
}

// ---- the certificate's bookkeeping ------------------------------------------------------------------

// statuses of ehm_compiled_certify (include/ehmpc.h)
enum { CERT_CERTIFIED = 0, CERT_UNCERTIFIED = 1, CERT_INADMISSIBLE = 2, CERT_NO_LAW = 3,
       CERT_NO_CELL = 4, CERT_STALLED = 5, CERT_STATUSES = 6 };

// The status of a leaf, the first that applies: no cell; an input that is not finite; a try that
// closed the cell; no candidate at all; a candidate set aside for a stalled solve; else every try
// had t* >= 0.
EHM_CERT_HD int certify_status(int has_cell, int no_law, int n_candidates, int n_aside,
                               int closed) {
    if (!has_cell) return CERT_NO_CELL;
    if (no_law) return CERT_NO_LAW;
    if (closed) return CERT_CERTIFIED;
    if (n_candidates == 0) return CERT_INADMISSIBLE;
    if (n_aside > 0) return CERT_STALLED;
    return CERT_UNCERTIFIED;
}

// the key candidates are ordered by: ((0 + W_0) + W_1) + .. + W_(nv-1)
inline double candidate_key(const double* W, int nv) {
    double s = 0.0;
    for (int i = 0; i < nv; ++i) s = s + W[i];
    return s;
}

// a key comes before another: the smaller one, any number before a NaN
inline bool key_before(double a, double b) { return a < b || (b != b && a == a); }

// order [n]: the candidates by key ascending, NaN keys last, the lower position first on ties;
// candidates are listed by commutation index ascending, so that is the lowest index.  Insertion
// sort: n is the number of commutations feasible on one leaf.
inline void order_candidates(int n, const double* key, int32_t* order) {
    for (int a = 0; a < n; ++a) {
        int at = a;
        while (at > 0 && key_before(key[a], key[order[at - 1]])) {
            order[at] = order[at - 1];
            --at;
        }
        order[at] = a;
    }
}

// (tbest, position) a beats b as the worst uncertified leaf: the larger tbest, the earlier leaf on
// ties; a NaN never wins
EHM_CERT_HD bool worst_beats(double ta, long long ia, double tb, long long ib) {
    return ta > tb || (ta == tb && ia < ib);
}

// index of the first id outside 0 .. n_leaf - 1, or -1
inline int64_t first_bad_leaf(const int32_t* ids, int64_t n, int64_t n_leaf) {
    for (int64_t q = 0; q < n; ++q)
        if (ids[q] < 0 || ids[q] >= n_leaf) return q;
    return -1;
}

}  // namespace ehm_cert
