/* frontend_model.c -- TEST INFRASTRUCTURE: the band-select front end's arithmetic contract (DESIGN.md section 2,
 * csrc/frontend.hip) restated in plain C, one sample and one output at a time.  Built by tests/frontend_model.py with
 * -ffp-contract=off; the kernel (on the GPU and under the CPU emulation) must reproduce every output bit.
 *
 *   x[n]  the capture sample as the pipeline's load stage converts it (csrc/common.hpp load_iq)
 *   r[n]  = x[n] * T[(q n) mod 65536]: four rounded products, one rounded difference, one rounded sum; +0 outside the stream
 *   y[m]  per component one accumulator from +0: acc = fmaf(h[ntaps - 1 - j], r[m D - c + j], acc), j = 0 .. ntaps - 1
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

/* T[i] = (float)cos(-2 pi i / 65536), (float)sin(-2 pi i / 65536), interleaved */
void fe_model_table(float *T)
{
    for (int i = 0; i < 65536; i++) {
        const double a = -2.0 * M_PI * (double)i / 65536.0;
        T[2 * i] = (float)cos(a);
        T[2 * i + 1] = (float)sin(a);
    }
}

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

/* The whole stream at once: n_in samples of format fmt -> ceil(n_in / D) outputs (re, im interleaved).  h: ntaps taps,
 * q: the quantised shift.  rot_out (2 n_in floats or NULL) receives r[n].  Returns the number of outputs, -1 on error. */
long long fe_model_run(int fmt, const void *in, long long n_in, int D, long long q, const float *h, int ntaps, float *out,
                       float *rot_out)
{
    if (fmt < 0 || fmt > 4 || D < 1 || ntaps < 1 || !(ntaps & 1)) return -1;
    float *T = malloc(sizeof(float) * 2 * 65536);
    float *r = malloc(sizeof(float) * 2 * (size_t)(n_in > 0 ? n_in : 1));
    if (!T || !r) return -1;
    fe_model_table(T);
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
    const int c = (ntaps - 1) / 2;
    const long long n_out = (n_in + D - 1) / D;
#pragma omp parallel for schedule(static)
    for (long long m = 0; m < n_out; m++) {
        float are = 0.0f, aim = 0.0f;
        for (int j = 0; j < ntaps; j++) {
            const long long n = m * D - c + j;
            float sr = 0.0f, si = 0.0f;
            if (n >= 0 && n < n_in) {
                sr = r[2 * n];
                si = r[2 * n + 1];
            }
            are = fmaf(h[ntaps - 1 - j], sr, are);
            aim = fmaf(h[ntaps - 1 - j], si, aim);
        }
        out[2 * m] = are;
        out[2 * m + 1] = aim;
    }
    if (rot_out)
        for (long long n = 0; n < 2 * n_in; n++) rot_out[n] = r[n];
    free(T);
    free(r);
    return n_out;
}
