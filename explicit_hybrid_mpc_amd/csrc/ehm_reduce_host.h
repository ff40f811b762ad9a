// The bookkeeping of ehm_reduce.hip that needs no device, on the parent table of
// ehm_certify_host.h: the check that a law's records form a forest, the representative (leftmost
// leaf) of every internal record, the topmost mergeable ancestor of a record, which records survive
// a reduction and the new index of a child.  Plain C++ that the kernels inline and a host program
// can drive (tests/native/reduce_host_main.cpp runs it under the address and undefined-behaviour
// sanitizers).
#pragma once

#include <cstdint>

#include "ehm_certify_host.h"

namespace ehm_red {

using ehm_cert::Parents;

// Internal record k is the parent the table holds for both of its children, on their sides: with
// root_names_entry for every root, the records form a forest (no record is named twice).
EHM_CERT_HD bool names_its_children(const Parents& P, int32_t k, int32_t left, int32_t right) {
    const int32_t ch[2] = {left, right};
    bool ok = true;
    for (int side = 0; side < 2; ++side) {
        const int32_t c = ch[side];
        if (c >= 0) ok = ok && P.node[c] == k && P.node_side[c] == side;
        else ok = ok && P.leaf[~c] == k && P.leaf_side[~c] == side;
    }
    return ok;
}

EHM_CERT_HD bool root_names_entry(const Parents& P, int32_t r, int32_t entry) {
    return (entry >= 0 ? P.node[entry] : P.leaf[~entry]) == ~r;
}

// What leaf l writes: itself as the representative of every ancestor it is the leftmost leaf of --
// up while it hangs on the left side.  In a forest every internal record has exactly one writer.
EHM_CERT_HD void mark_representative(const Parents& P, int32_t l, int32_t* rep) {
    int32_t up = P.leaf[l];
    int side = P.leaf_side[l];
    while (up >= 0 && side == 0) {
        rep[up] = l;
        side = P.node_side[up];
        up = P.node[up];
    }
}

// The topmost mergeable record (open == 0) among `up` and its ancestors, -1 if there is none.
EHM_CERT_HD int32_t topmost_merged(const Parents& P, int32_t up, const uint8_t* open) {
    int32_t top = -1;
    while (up >= 0) {
        if (!open[up]) top = up;
        up = P.node[up];
    }
    return top;
}

// Internal record a survives: it is not mergeable and has no mergeable ancestor.
EHM_CERT_HD bool internal_survives(const Parents& P, int32_t a, const uint8_t* open) {
    return open[a] && topmost_merged(P, P.node[a], open) < 0;
}

// The leaf whose record stands for leaf l in the reduced law: l itself without a mergeable
// ancestor, else the representative of the topmost one.  l survives iff that is l.
EHM_CERT_HD int32_t leaf_target(const Parents& P, int32_t l, const uint8_t* open,
                                const int32_t* rep) {
    const int32_t top = topmost_merged(P, P.leaf[l], open);
    return top < 0 ? l : rep[top];
}

// The new id of a child (or root entry) c of a record that survives: a surviving internal record
// keeps its place in the order, a mergeable one becomes the leaf of its representative.
EHM_CERT_HD int32_t renumber(int32_t c, const uint8_t* open, const int32_t* rep,
                             const int32_t* new_int, const int32_t* new_leaf) {
    if (c < 0) return ~new_leaf[~c];
    return open[c] ? new_int[c] : ~new_leaf[rep[c]];
}

}  // namespace ehm_red
