// Stand-alone driver of csrc/ehm_verdict.h and csrc/ehm_err.h (plain C++: no HIP, no device).
// Built by tests/test_host_audit.py with the address and undefined-behaviour sanitizers.  It checks
// the rules at their thresholds, the host merge and the error channel itself, then judges the rows
// on its standard input for the driver to compare with the numpy mirrors:
//   "j vbar vstar eps_a eps_r rtol" -> "status bin ratio"   (the gap ladder and the bin of the ratio)
//   "b r"                           -> "bin"
// Numbers travel as hexadecimal floats, so nothing is rounded on the way.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "../../explicit_hybrid_mpc_amd/csrc/ehm_err.h"
#include "../../explicit_hybrid_mpc_amd/csrc/ehm_verdict.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

const double INF = std::numeric_limits<double>::infinity();
const double QNAN = std::numeric_limits<double>::quiet_NaN();

void ladder() {
    using namespace ehm_verdict;
    const double vs = 3.0, eps_a = 0.25, eps_r = 0.125, rtol = 1e-7;
    const double bound = bound_of(eps_a, eps_r, vs), slack = slack_of(rtol, vs);
    CHECK(bound == 0.375 && slack == rtol * 4.0);
    CHECK(bound_of(0.5, eps_r, vs) == 0.5);
    const double lo = -slack, hi = bound + slack;
    CHECK(gap_status(lo, bound, slack) == 0);
    CHECK(gap_status(std::nextafter(lo, 0.0), bound, slack) == 0);
    CHECK(gap_status(std::nextafter(lo, -INF), bound, slack) == 2);
    CHECK(gap_status(hi, bound, slack) == 0);
    CHECK(gap_status(std::nextafter(hi, 0.0), bound, slack) == 0);
    CHECK(gap_status(std::nextafter(hi, INF), bound, slack) == 1);
    CHECK(gap_status(QNAN, bound, slack) == 2);
    CHECK(gap_status(INF, bound, slack) == 1 && gap_status(-INF, bound, slack) == 2);
    CHECK(ratio_of(0.75, 0.375) == 2.0 && std::isnan(ratio_of(0.0, 0.0)));
}

void bins() {
    using namespace ehm_verdict;
    CHECK(ratio_bin(-0.0) == 0 && ratio_bin(0.0) == 0);
    CHECK(ratio_bin(1.0 / 32.0) == 1 && ratio_bin(std::nextafter(1.0 / 32.0, 0.0)) == 0);
    CHECK(ratio_bin(31.0 / 32.0) == 31 && ratio_bin(std::nextafter(1.0, 0.0)) == 31);
    CHECK(ratio_bin(1.0) == 31 && ratio_bin(std::nextafter(1.0, 2.0)) == EHM_VERDICT_BINS - 1);
    CHECK(ratio_bin(INF) == EHM_VERDICT_BINS - 1);
    CHECK(ratio_bin(-INF) == 0 && ratio_bin(-1.0) == 0 && ratio_bin(QNAN) == 0);
    CHECK(ratio_is_candidate(-INF) && ratio_is_candidate(0.0) && !ratio_is_candidate(QNAN));
    CHECK(ratio_beats(2.0, 9, 1.0, 1) && !ratio_beats(1.0, 1, 2.0, 9));
    CHECK(ratio_beats(1.0, 1, 1.0, 2) && !ratio_beats(1.0, 2, 1.0, 1));
    CHECK(!ratio_beats(QNAN, 1, 1.0, 2) && !ratio_beats(1.0, 1, QNAN, 2));
}

void merge() {
    using ehm_verdict::merge_block_worst;
    using ehm_verdict::ratio_beats;
    const unsigned long long NONE = ~0ULL;
    double best = -INF;
    unsigned long long id = NONE;
    // a chunk without a candidate
    const double k0[3] = {-INF, -INF, -INF};
    const unsigned long long i0[3] = {NONE, NONE, NONE};
    CHECK(!merge_block_worst(k0, i0, 3, NONE, ratio_beats, best, id));
    CHECK(id == NONE && best == -INF);
    // a tie across two workgroups: the smaller id, wherever it stands; a NaN key never wins
    const double k1[4] = {QNAN, 2.5, 2.5, 1.0};
    const unsigned long long i1[4] = {3, 700, 300, 5};
    CHECK(merge_block_worst(k1, i1, 4, NONE, ratio_beats, best, id));
    CHECK(id == 300 && best == 2.5);
    // a later chunk that is no better leaves the best alone; a NaN key with no best yet does too
    const double k2[2] = {2.5, QNAN};
    const unsigned long long i2[2] = {400, 1};
    CHECK(!merge_block_worst(k2, i2, 2, NONE, ratio_beats, best, id));
    CHECK(id == 300 && best == 2.5);
    best = -INF;
    id = NONE;
    CHECK(!merge_block_worst(k2 + 1, i2 + 1, 1, NONE, ratio_beats, best, id) && id == NONE);
    // a candidate at -inf is one
    const double k3[1] = {-INF};
    const unsigned long long i3[1] = {8};
    CHECK(merge_block_worst(k3, i3, 1, NONE, ratio_beats, best, id) && id == 8);
    // signed ids with -1 for none, as the certificate uses them
    long long leaf = -1;
    double t = QNAN;
    const double k4[3] = {0.5, -1.0, 0.5};
    const long long i4[3] = {9, -1, 4};
    const auto beats = [](double ta, long long ia, double tb, long long ib) {
        return ta > tb || (ta == tb && ia < ib);
    };
    CHECK(merge_block_worst(k4, i4, 3, -1LL, beats, t, leaf) && leaf == 4 && t == 0.5);
}

void channel() {
    ehm_err_channel ch;
    CHECK(std::strcmp(ch.c_str(), "") == 0);
    CHECK(ch.fail(-1, "p = %d of %lld", 3, 12LL) == -1);
    CHECK(ch.msg == "p = 3 of 12");
    const std::string big(2000, 'x');
    CHECK(ch.fail(-3, "%s!", big.c_str()) == -3);
    CHECK(ch.msg.size() == 511 && ch.msg == std::string(511, 'x'));
    CHECK(std::strlen(ch.c_str()) == 511);
    CHECK(ch.fail(-6, "short") == -6 && ch.msg == "short");
}

}  // namespace

int main() {
    ladder();
    bins();
    merge();
    channel();
    char kind;
    while (std::scanf(" %c", &kind) == 1) {
        using namespace ehm_verdict;
        if (kind == 'j') {
            double vbar, vs, eps_a, eps_r, rtol;
            if (std::scanf("%la %la %la %la %la", &vbar, &vs, &eps_a, &eps_r, &rtol) != 5) return 2;
            const double gap = vbar - vs, bound = bound_of(eps_a, eps_r, vs);
            const double r = ratio_of(gap, bound);
            std::printf("%d %d %a\n", gap_status(gap, bound, slack_of(rtol, vs)), ratio_bin(r), r);
        } else if (kind == 'b') {
            double r;
            if (std::scanf("%la", &r) != 1) return 2;
            std::printf("%d\n", ratio_bin(r));
        } else {
            return 2;
        }
    }
    if (failures) return 1;
    std::printf("verdict host rules: ok\n");
    return 0;
}
