/* resample_model.c -- TEST INFRASTRUCTURE: the arithmetic contract of the front end's rational mode (DESIGN.md section 2,
 * csrc/resample.hip) restated in plain C, one sample and one output at a time.  Built by tests/resample_model.py with
 * -ffp-contract=off; the kernel (on the GPU and under the CPU emulation) must reproduce every output bit.
 *
 *   x[n]  the capture sample as the pipeline's load stage converts it (csrc/common.hpp load_iq)
 *   r[n]  = x[n] * T[(q n) mod 65536]: four rounded products, one rounded difference, one rounded sum; +0 outside the stream
 *   y[m]  = sum_n P[m M + C - n L] r[n] over the n with 0 <= m M + C - n L < Np, C = (Np - 1) / 2: per component one
 *           accumulator from +0 and one fmaf per term in ascending n, the zero samples outside the stream included
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

static void convert(int fmt, const void *in, long long n, float *re, float *im)
{
    switch (fmt) {
    case 2: {
        const float *p = (const float *)in;
        *re = p[2 * n];
        *im = p[2 * n + 1];
        break;
    }
    case 0: {
        const int8_t *p = (const int8_t *)in;
        *re = (float)p[2 * n] / 128.0f;
        *im = (float)p[2 * n + 1] / 128.0f;
        break;
    }
    case 1: {
        const int16_t *p = (const int16_t *)in;
        *re = (float)(p[2 * n] >> 8) / 128.0f;
        *im = (float)(p[2 * n + 1] >> 8) / 128.0f;
        break;
    }
    case 3: {
        const int16_t *p = (const int16_t *)in;
        *re = (float)p[2 * n] * (1.0f / 32768.0f);
        *im = (float)p[2 * n + 1] * (1.0f / 32768.0f);
        break;
    }
    default: {
        const int16_t *p = (const int16_t *)in;
        *re = (float)p[2 * n] * (1.0f / 2048.0f);
        *im = (float)p[2 * n + 1] * (1.0f / 2048.0f);
        break;
    }
    }
}

static long long floor_div(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

/* The whole stream at once: n_in samples of format fmt -> ceil(n_in L / M) outputs (re, im interleaved).  P: Np taps (odd),
 * q: the quantised shift.  Returns the number of outputs, -1 on error. */
long long rs_model_run(int fmt, const void *in, long long n_in, int L, int M, long long q, const float *P, int Np, float *out)
{
    if (fmt < 0 || fmt > 4 || L < 1 || M < 1 || Np < 1 || !(Np & 1)) return -1;
    float *T = malloc(sizeof(float) * 2 * 65536);
    float *r = malloc(sizeof(float) * 2 * (size_t)(n_in > 0 ? n_in : 1));
    if (!T || !r) return -1;
    for (int i = 0; i < 65536; i++) {
        const double a = -2.0 * M_PI * (double)i / 65536.0;
        T[2 * i] = (float)cos(a);
        T[2 * i + 1] = (float)sin(a);
    }
    const unsigned q16 = (unsigned)(q & 0xffff);
    for (long long n = 0; n < n_in; n++) {
        float xr, xi;
        convert(fmt, in, n, &xr, &xi);
        const unsigned i = (q16 * (unsigned)(n & 0xffff)) & 0xffffu;
        const float tr = T[2 * i], ti = T[2 * i + 1];
        const float ac = xr * tr, bd = xi * ti, ad = xr * ti, bc = xi * tr;
        r[2 * n] = ac - bd;
        r[2 * n + 1] = ad + bc;
    }
    const long long C = (Np - 1) / 2;
    const long long n_out = (n_in * L + M - 1) / M;
#pragma omp parallel for schedule(static)
    for (long long m = 0; m < n_out; m++) {
        /* the terms: n from the first with m M + C - n L <= Np - 1 to the last with m M + C - n L >= 0 */
        const long long n0 = floor_div(m * M + C - Np, L) + 1, n1 = floor_div(m * M + C, L);
        float are = 0.0f, aim = 0.0f;
        for (long long n = n0; n <= n1; n++) {
            const float p = P[m * M + C - n * L];
            float sr = 0.0f, si = 0.0f;
            if (n >= 0 && n < n_in) {
                sr = r[2 * n];
                si = r[2 * n + 1];
            }
            are = fmaf(p, sr, are);
            aim = fmaf(p, si, aim);
        }
        out[2 * m] = are;
        out[2 * m + 1] = aim;
    }
    free(T);
    free(r);
    return n_out;
}
