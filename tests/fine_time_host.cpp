// fine_time_host.cpp -- TEST INFRASTRUCTURE: the host side of the symbol timing estimator (csrc/fine_time.hpp:
// fine_time_tau, fine_time_public, fine_time_fold, fine_time_result) in a program of its own, built by
// tests/test_fine_time_host.py with g++ -fsanitize=address,undefined against the HIP emulation's headers: the fold alone --
// which place a record's time takes, how it rounds, and what the summary counts.
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "fine_time.hpp"

using namespace irdm;

static int failures = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            fprintf(stderr, "fine_time_host: line %d: %s\n", __LINE__, #cond);      \
            failures++;                                                             \
        }                                                                           \
    } while (0)

// a record whose line says tau (samples, at 10 per symbol) with quality 25
static TimeRec rec_of(double tau, uint32_t n = 1910u)
{
    const double a = -tau / 10.0 * 6.283185307179586476925;
    return TimeRec{ 5.0 * cos(a), 5.0 * sin(a), 1.0, 0u, n };
}

int main()
{
    const float sps = 10.0f;
    const double rate = 250000.0;
    const uint64_t t0 = 1700000000ULL * 1000000000ULL + 123456789ULL;

    // tau of a record, and its range
    CHECK(fabs(fine_time_tau(rec_of(1.25), sps) - 1.25) < 1e-12 && fabs(fine_time_tau(rec_of(-4.9), sps) + 4.9) < 1e-12);
    CHECK(fine_time_tau(TimeRec{ -1.0, 0.0, 1.0, 0u, 64u }, sps) == -5.0 && fine_time_tau(TimeRec{ -1.0, -0.0, 1.0, 0u, 64u }, sps) == -5.0);
    CHECK(fine_time_tau(TimeRec{ 1.0, 0.0, 1.0, 0u, 64u }, sps) == 0.0);
    irdm_fine_time_t pub;
    fine_time_public(rec_of(2.0), sps, &pub);
    CHECK(pub.flags == 0 && pub.n == 1910 && pub.quality == 25.0f && pub.time_ns == 0 && pub.corr == 0.0f && pub.id == 0 && pub.floor == 1.0);
    fine_time_public(TimeRec::invalid(63u), sps, &pub);
    CHECK(pub.flags == kLineInvalid && pub.n == 63 && pub.tau == 0.0 && pub.quality == 0.0f && pub.s_re == 0.0);

    FineTimeStream st{ kFtHist };
    // applied: the line's place.  189 + 0.5 samples are 758 us
    CHECK(fine_time_fold(st, 1, rec_of(0.5), sps, t0, 189, 0.25f, rate, true) == t0 + 758000);
    CHECK(st.used == 1 && st.q.back().flags == 0 && st.q.back().time_ns == t0 + 758000 && st.q.back().corr == 0.25f && st.q.back().id == 1);
    CHECK(st.hist[(size_t)kFtHist.bin(0.25)] == 1);
    // just inside a quarter of a symbol: applied
    CHECK(fine_time_fold(st, 2, rec_of(2.4), sps, t0, 189, 0.0f, rate, true) == t0 + (uint64_t)llrint((189.0 + fine_time_tau(rec_of(2.4), sps)) * 4000.0));
    CHECK(st.used == 2);
    // ambiguous, tau - c = +-2.6: the correlator's place, c = 0.25 -> 189.25 samples are 757 us
    CHECK(fine_time_fold(st, 3, rec_of(2.85), sps, t0, 189, 0.25f, rate, true) == t0 + 757000);
    CHECK(st.q.back().flags == kLineOutOfRange && fabs(st.q.back().tau - 2.85) < 1e-12 && st.out_of_range == 1 && st.used == 2);
    CHECK(fine_time_fold(st, 4, rec_of(-2.35), sps, t0, 189, 0.25f, rate, true) == t0 + 757000);
    CHECK(st.q.back().flags == kLineOutOfRange && st.out_of_range == 2 && st.used == 2);
    // the wrap is no neighbour: tau = -4.9 and c = +0.45 are 5.35 apart, not 4.65
    CHECK(fine_time_fold(st, 5, rec_of(-4.9), sps, t0, 189, 0.45f, rate, true) == t0 + (uint64_t)llrint((189.0 + (double)0.45f) * 4000.0));
    CHECK(st.out_of_range == 3);
    // invalid: the correlator's place
    CHECK(fine_time_fold(st, 6, TimeRec::invalid(700u), sps, t0, 189, -0.25f, rate, true) == t0 + 755000);
    CHECK(st.q.back().flags == kLineInvalid && st.q.back().tau == 0.0 && st.invalid == 1 && st.used == 2);
    // not ok: counted, in no histogram bin, whatever its record says
    CHECK(fine_time_fold(st, 7, rec_of(0.5), sps, t0, 189, 0.25f, rate, false) == t0 + 758000);
    CHECK(st.q.back().flags == kLineNotOk && st.not_ok == 1 && st.used == 2);
    fine_time_fold(st, 8, rec_of(3.0), sps, t0, 189, 0.25f, rate, false);
    CHECK(st.q.back().flags == (kLineOutOfRange | kLineNotOk) && st.not_ok == 2 && st.out_of_range == 3);
    fine_time_fold(st, 9, TimeRec::invalid(0u), sps, t0, 189, 0.25f, rate, false);
    CHECK(st.q.back().flags == (kLineInvalid | kLineNotOk) && st.not_ok == 3 && st.invalid == 1);
    // a negative place: uw_start + delta < 0 goes back from the timestamp, rounded to the nearest ns
    CHECK(fine_time_fold(st, 10, rec_of(-0.6), sps, t0, 0, -0.5f, rate, true) == t0 - 2400);
    CHECK(fine_time_fold(st, 11, rec_of(-2.0), sps, t0, 1, -1.0f, rate, true) == t0 - 4000);
    CHECK(fine_time_fold(st, 12, TimeRec::invalid(64u), sps, t0, 0, -0.0004f, rate, true) == t0 - 2);        // -1.6 ns
    CHECK(fine_time_fold(st, 13, TimeRec::invalid(64u), sps, 5000, 0, -1.0f, rate, true) == 1000);
    CHECK(fine_time_fold(st, 15, TimeRec::invalid(64u), sps, t0, 0, -0.0001f, rate, true) == t0);                 // -0.4 ns
    CHECK(fine_time_fold(st, 14, rec_of(0.0), sps, t0, 0, 0.0f, rate, true) == t0);

    irdm_fine_time_summary_t s;
    fine_time_result(st, &s);
    CHECK(s.frames_seen == 15 && s.frames_applied == 5 && s.frames_not_ok == 3 && s.frames_ambiguous == 3 && s.frames_invalid == 4);
    // tau - c of the applied: 0.25, 2.4, -0.1, -1.0, 0.0
    CHECK(s.q25 == kFtHist.centre(kFtHist.bin(-0.1)) && s.median == kFtHist.centre(kFtHist.bin(0.0)) && s.q75 == kFtHist.centre(kFtHist.bin(0.25)));
    CHECK(kFtHist.count == 501 && kFtHist.bin(-2.5) == 0 && kFtHist.bin(2.5) == 500 && kFtHist.bin(0.0) == 250 && kFtHist.bin(1e300) == 500 &&
          kFtHist.bin(NAN) == 0);
    if (failures) return 1;
    printf("fine_time_host ok\n");
    return 0;
}
