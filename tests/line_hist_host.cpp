// line_hist_host.cpp -- TEST INFRASTRUCTURE: the host side of the frame line estimators (csrc/frame_line.hpp: LineBins,
// LineStream, line_fold, line_quantile, and the thin functions of symbol_clock.hpp / fine_freq.hpp on them) in a program of
// its own, built by tests/test_line_hist_host.py with g++ -fsanitize=address,undefined against the HIP emulation's headers:
// values at, below and far beyond both ends of each histogram, NaN and +-Inf fall into the end bins without a conversion
// that is undefined, and the quantiles of known counts are the centres of the bins that hold them.
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "fine_freq.hpp"
#include "symbol_clock.hpp"

using namespace irdm;

static int failures = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            fprintf(stderr, "line_hist_host: line %d: %s\n", __LINE__, #cond);      \
            failures++;                                                             \
        }                                                                           \
    } while (0)

static void ends(const LineBins &b)
{
    const int last = b.count - 1;
    const double lo = b.centre(0), hi = b.centre(last);
    for (int k = 0; k < b.count; k++) CHECK(b.bin(b.centre(k)) == k);
    CHECK(b.bin(lo - 0.49 * b.width) == 0 && b.bin(hi + 0.49 * b.width) == last);
    const double below[] = { lo - b.width, lo - 1e3 * b.width, -3e9, -1e19, -1e300, -DBL_MAX, -INFINITY, NAN, -NAN };
    const double above[] = { hi + b.width, hi + 1e3 * b.width, 3e9, 1e19, 1e300, DBL_MAX, INFINITY };
    for (double v : below) CHECK(b.bin(v) == 0);
    for (double v : above) CHECK(b.bin(v) == last);
    CHECK(b.bin((double)FLT_MAX) == last && b.bin(-(double)FLT_MAX) == 0 && b.bin((double)nanf("")) == 0);
}

int main()
{
    ends(kScHist);
    ends(kFfHist);
    CHECK(kScHist.count == 1601 && kScHist.centre(800) == -0.08 + 800.0 * 1e-4 && kScHist.bin(0.0) == 800);
    CHECK(kFfHist.count == 1001 && kFfHist.centre(500) == 0.0 && kFfHist.bin(0.49) == 500 && kFfHist.bin(0.5) == 501);

    // known counts: 1 in bin 10, 2 in bin 20, 1 in bin 30 of the frequency histogram, through the fold of a stream
    {
        FineFreqStream st{ kFfHist };
        CHECK(line_quantile(st, 0.5) == 0.0);                                           // (an empty stream)
        const double v[] = { kFfHist.centre(20), kFfHist.centre(10), kFfHist.centre(30) + 0.25, kFfHist.centre(20) - 0.25 };
        const LineRec r = { 0.0f, 9.0f, 0u, 1910u };
        for (double d : v) CHECK(fine_freq_fold(st, 7, r, 1000.0 + d, true, 1000.0) == 1000.0 + d);
        CHECK(st.hist[10] == 1 && st.hist[20] == 2 && st.hist[30] == 1 && st.used == 4);
        CHECK(line_quantile(st, 0.0) == kFfHist.centre(10) && line_quantile(st, 0.25) == kFfHist.centre(10));
        CHECK(line_quantile(st, 0.5) == kFfHist.centre(20) && line_quantile(st, 0.75) == kFfHist.centre(20));
        CHECK(line_quantile(st, 0.76) == kFfHist.centre(30) && line_quantile(st, 1.0) == kFfHist.centre(30));
        // classified not_ok -> invalid -> out_of_range -> used; a flagged frame keeps the PLL's frequency
        const LineRec inv = { 0.0f, 0.0f, kLineInvalid | kLineOutOfRange, 63u }, oor = { 250.0f, 3.0f, kLineOutOfRange, 700u };
        CHECK(fine_freq_fold(st, 8, inv, 5.0, true, 6.0) == 6.0 && fine_freq_fold(st, 9, oor, 5.0, true, 6.0) == 6.0);
        CHECK(fine_freq_fold(st, 10, r, 5.0, false, 6.0) == 6.0 && fine_freq_fold(st, 11, inv, 5.0, false, 6.0) == 6.0);
        CHECK(st.q.size() == 8 && st.q.back().flags == (kLineInvalid | kLineOutOfRange | kLineNotOk) && st.q.back().id == 11);
        // a difference that is no number, or none a histogram holds, is counted at an end
        CHECK(fine_freq_fold(st, 12, r, 1e300, true, 0.0) == 1e300 && st.hist[1000] == 1);
        CHECK(fine_freq_fold(st, 13, r, -INFINITY, true, 0.0) == -INFINITY && st.hist[0] == 1);
        fine_freq_fold(st, 14, r, NAN, true, 0.0);
        CHECK(st.hist[0] == 2);
        irdm_fine_freq_summary_t s;
        fine_freq_result(st, &s);
        CHECK(s.frames_seen == 11 && s.frames_applied == 7 && s.frames_not_ok == 2 && s.frames_invalid == 1 && s.frames_out_of_range == 1);
        CHECK(s.q25 == kFfHist.centre(0) && s.median == kFfHist.centre(20) && s.q75 == kFfHist.centre(30));
    }
    // the clock's stream: the record's float eps, the same counts, the implied rate
    {
        SymbolClockStream st{ kScHist };
        const float eps[] = { 0.0025f, -0.0100f, 0.0031f, 0.0025f };
        for (float e : eps) symbol_clock_fold(st, 1, LineRec{ e, 20.0f, 0u, 1910u }, true);
        symbol_clock_fold(st, 2, LineRec{ -0.08f, 3.0f, kLineOutOfRange, 1910u }, true);
        symbol_clock_fold(st, 3, LineRec{ 0.0f, 0.0f, kLineInvalid, 63u }, true);
        symbol_clock_fold(st, 4, LineRec{ 0.001f, 20.0f, 0u, 1910u }, false);
        CHECK(st.hist[825] == 2 && st.hist[700] == 1 && st.hist[831] == 1);
        irdm_symbol_clock_t s;
        symbol_clock_result(st, 40, &s);
        CHECK(s.frames_used == 4 && s.frames_out_of_range == 1 && s.frames_invalid == 1 && s.frames_not_ok == 1);
        CHECK(s.q25 == kScHist.centre(700) && s.median == kScHist.centre(825) && s.q75 == kScHist.centre(825));
        CHECK(s.implied_rate_hz == 250000.0 * 40.0 * (1.0 + s.median) && st.q.size() == 7 && st.q.back().flags == kLineNotOk);
        symbol_clock_fold(st, 5, LineRec{ nanf(""), 1.0f, 0u, 64u }, true);
        symbol_clock_fold(st, 6, LineRec{ FLT_MAX, 1.0f, 0u, 64u }, true);
        CHECK(st.hist[0] == 1 && st.hist[1600] == 1 && st.used == 6);
    }
    if (failures) return 1;
    printf("line_hist_host ok\n");
    return 0;
}
