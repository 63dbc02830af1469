// doppler.cpp -- --position: the receiver's position from the Doppler shift of decoded IRA frames (doppler_pos.c, after
// Tan et al., "New Method for Positioning Using IRIDIUM Satellite Signals of Opportunity", IEEE Access 2019).
//
// Per satellite id a ring of the last 200 accepted measurements (satellite ECEF position from the IRA's 4 km units, burst
// frequency, timestamp).  A solve collects every recent measurement whose satellite velocity can be estimated (circular
// orbit through two positions at least 2 s apart), turns its frequency into a range rate against the satellite's
// voted channel frequency, and runs an iterated weighted least-squares fit of (x, y, z, clock drift) with Earth rotation
// and height aiding, then outlier and per-satellite screening with re-solves, HDOP, and a guard against solution jumps.
//
// All state lives in irdm_doppler (no globals).  Every double is computed in the reference's operation order (the library
// is built with -ffp-contract=off, as the reference's x86-64 build never fuses), so the solutions are bit-identical.
// Two deliberate differences, both in the caller's schedule (irdm_format_doppler_*): solves run on stream time instead of
// the stats thread's wall clock, and the verbose "DOPPLER:" diagnostics are not printed.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <new>
#include <string>
#include <vector>

#include "../../include/irdm_hip.h"

namespace {

constexpr int kMaxSats = 128;
constexpr int kMeasPerSat = 200;
constexpr int kMinMeas = 8;
constexpr int kMinSats = 2;
constexpr int kMaxIter = 200;
constexpr double kConvergeM = 100.0;
constexpr double kOutlierSigma = 3.0;
constexpr uint64_t kMaxAgeNs = 30ULL * 60 * 1000000000ULL;
constexpr uint64_t kMinVelIntervalNs = 2ULL * 1000000000ULL;
constexpr double kClusterDist = 8000e3;
constexpr double kGapResetS = 600.0;
constexpr double kMaxJump = 500e3;

// WGS-84 and the physical constants of the model
constexpr double kA = 6378137.0;
constexpr double kF = 1.0 / 298.257223563;
constexpr double kE2 = 2.0 * kF - kF * kF;
constexpr double kGM = 3.986004418e14;
constexpr double kC = 299792458.0;
constexpr double kOmega = 7.2921150e-5;
constexpr double kBaseFreq = 1616000000.0;     // Iridium channel 0 and spacing (gsmtap.h)
constexpr double kChanWidth = 41666.667;

double dot3(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
double norm3(const double v[3]) { return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
void sub3(const double a[3], const double b[3], double o[3]) { o[0] = a[0] - b[0]; o[1] = a[1] - b[1]; o[2] = a[2] - b[2]; }
void cross3(const double a[3], const double b[3], double o[3])
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// Where a sine and a cosine of the same angle are both needed, they come from one sincos() call: the reference's gcc build
// merges the pair into sincos(), whose last bit differs from cos()'s for some angles (glibc).
void to_ecef(double lat_deg, double lon_deg, double alt_m, double e[3])
{
    const double lat = lat_deg * M_PI / 180.0, lon = lon_deg * M_PI / 180.0;
    double slat, clat, slon, clon;
    sincos(lat, &slat, &clat);
    sincos(lon, &slon, &clon);
    const double N = kA / sqrt(1.0 - kE2 * slat * slat);
    e[0] = (N + alt_m) * clat * clon;
    e[1] = (N + alt_m) * clat * slon;
    e[2] = (N * (1.0 - kE2) + alt_m) * slat;
}

// Bowring's iteration, five rounds
void to_geodetic(const double e[3], double *lat_deg, double *lon_deg, double *alt_m)
{
    const double x = e[0], y = e[1], z = e[2];
    const double p = sqrt(x * x + y * y);
    *lon_deg = atan2(y, x) * 180.0 / M_PI;
    double lat = atan2(z, p * (1.0 - kE2));
    for (int i = 0; i < 5; i++) {
        const double s = sin(lat);
        const double N = kA / sqrt(1.0 - kE2 * s * s);
        lat = atan2(z + kE2 * N * s, p);
    }
    double s, c;
    sincos(lat, &s, &c);
    const double N = kA / sqrt(1.0 - kE2 * s * s);
    *alt_m = p / c - N;
    *lat_deg = lat * 180.0 / M_PI;
}

void enu_rotation(double lat_deg, double lon_deg, double R[3][3])
{
    const double lat = lat_deg * M_PI / 180.0, lon = lon_deg * M_PI / 180.0;
    double slat, clat, slon, clon;
    sincos(lat, &slat, &clat);
    sincos(lon, &slon, &clon);
    R[0][0] = -slon;        R[0][1] = clon;         R[0][2] = 0.0;
    R[1][0] = -slat * clon; R[1][1] = -slat * slon; R[1][2] = clat;
    R[2][0] = clat * clon;  R[2][1] = clat * slon;  R[2][2] = slat;
}

// Gauss-Jordan with partial pivoting, A destroyed; -1 when a pivot is below 1e-30
int invert4(double A[4][4], double inv[4][4])
{
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) inv[i][j] = i == j ? 1.0 : 0.0;
    for (int col = 0; col < 4; col++) {
        int piv = col;
        double best = fabs(A[col][col]);
        for (int r = col + 1; r < 4; r++)
            if (fabs(A[r][col]) > best) { best = fabs(A[r][col]); piv = r; }
        if (best < 1e-30) return -1;
        if (piv != col)
            for (int j = 0; j < 4; j++) {
                double t = A[col][j]; A[col][j] = A[piv][j]; A[piv][j] = t;
                t = inv[col][j]; inv[col][j] = inv[piv][j]; inv[piv][j] = t;
            }
        const double d = A[col][col];
        for (int j = 0; j < 4; j++) { A[col][j] /= d; inv[col][j] /= d; }
        for (int r = 0; r < 4; r++) {
            if (r == col) continue;
            const double f = A[r][col];
            for (int j = 0; j < 4; j++) { A[r][j] -= f * A[col][j]; inv[r][j] -= f * inv[col][j]; }
        }
    }
    return 0;
}

struct Meas {
    double ecef[3];
    double freq;
    uint64_t ts;
    int valid;
};

struct Sat {
    int id;
    Meas m[kMeasPerSat];
    int head, count;            // next write slot; stored (at most kMeasPerSat)
    double chan;

    // oldest first
    Meas *at(int i)
    {
        if (i < 0 || i >= count) return nullptr;
        const int first = count < kMeasPerSat ? 0 : (head - count + kMeasPerSat) % kMeasPerSat;
        return &m[(first + i) % kMeasPerSat];
    }
};

// one row of the fit
struct Row {
    double ecef[3], vel[3];
    double range_rate, weight;
    int sat;
};

// the nearest channel of every recent measurement; the channel most of them agree on (first such on a tie)
double channel_of(Sat &s, uint64_t now)
{
    double ch[kMeasPerSat];
    int n = 0;
    for (int i = 0; i < s.count; i++) {
        const Meas *m = s.at(i);
        if (!m || !m->valid) continue;
        if (now > 0 && now - m->ts > kMaxAgeNs) continue;
        ch[n++] = kBaseFreq + round((m->freq - kBaseFreq) / kChanWidth) * kChanWidth;
    }
    if (n == 0) return 0;
    double best = 0;
    int votes = 0;
    for (int i = 0; i < n; i++) {
        int c = 0;
        for (int j = 0; j < n; j++)
            if (fabs(ch[j] - ch[i]) < 1.0) c++;
        if (c > votes) { votes = c; best = ch[i]; }
    }
    return best;
}

// the satellite's velocity at measurement idx: direction in the orbital plane through the position and the measurement
// the farthest from it in time (2 s .. 10 min, a valid orbit radius; the timestamp difference is taken unsigned as the
// reference takes it, so only later measurements qualify), sense from the order in time, speed from vis-viva
int velocity_of(Sat &s, int idx, double vel[3])
{
    const Meas *cur = s.at(idx);
    if (!cur) return -1;
    const double r = norm3(cur->ecef);
    if (r < 1e6) return -1;
    const Meas *other = nullptr;
    double best_dt = 0;
    for (int i = 0; i < s.count; i++) {
        if (i == idx) continue;
        const Meas *m = s.at(i);
        if (!m || !m->valid) continue;
        const double dt = fabs((double)(m->ts - cur->ts) / 1e9);
        if (dt >= kMinVelIntervalNs / 1e9 && dt < 600.0 && dt > best_dt) {
            const double ro = norm3(m->ecef);
            if (ro < 7050e3 || ro > 7250e3) continue;
            best_dt = dt;
            other = m;
        }
    }
    if (!other) return -1;
    double h[3], dir[3], fwd[3];
    cross3(cur->ecef, other->ecef, h);
    if (norm3(h) < 1e6) return -1;
    cross3(h, cur->ecef, dir);
    const double dn = norm3(dir);
    if (dn < 1.0) return -1;
    if (other->ts > cur->ts) sub3(other->ecef, cur->ecef, fwd);
    else sub3(cur->ecef, other->ecef, fwd);
    const double sign = dot3(dir, fwd) >= 0 ? 1.0 : -1.0;
    const double speed = sqrt(kGM / r);
    for (int k = 0; k < 3; k++) vel[k] = sign * speed * dir[k] / dn;
    return 0;
}

// predicted range rate of a row from rx (receiver velocity = Earth rotation) and its partial derivatives
struct Model {
    double rx[3], rx_vel[3];
    explicit Model(const double r[3])
    {
        for (int k = 0; k < 3; k++) rx[k] = r[k];
        rx_vel[0] = -kOmega * rx[1];
        rx_vel[1] = kOmega * rx[0];
        rx_vel[2] = 0.0;
    }
    // rho_dot_geom of row m; false when the range is below 1 m
    bool geom(const Row &m, double los[3], double rel[3], double *rho, double *rdot) const
    {
        sub3(m.ecef, rx, los);
        *rho = norm3(los);
        if (*rho < 1.0) return false;
        for (int k = 0; k < 3; k++) rel[k] = m.vel[k] - rx_vel[k];
        *rdot = dot3(los, rel) / *rho;
        return true;
    }
    static void jacobian(const double los[3], const double rel[3], double rho, double rdot, double H[4])
    {
        const double rho2 = rho * rho;
        H[0] = -rel[0] / rho + los[0] * rdot / rho2 + kOmega * los[1] / rho;
        H[1] = -rel[1] / rho + los[1] * rdot / rho2 - kOmega * los[0] / rho;
        H[2] = -rel[2] / rho + los[2] * rdot / rho2;
        H[3] = 1.0;
    }
};

void accumulate(double N[4][4], double y[4], const double H[4], double w, double dy)
{
    for (int r = 0; r < 4; r++) {
        for (int c = 0; c < 4; c++) N[r][c] += H[r] * w * H[c];
        y[r] += H[r] * w * dy;
    }
}

}  // namespace

struct irdm_doppler {
    double height = 0;
    std::vector<Sat> sats;                      // in order of first appearance, at most kMaxSats
    std::vector<Row> rows;                      // the fit's rows; kept between solves, as the reference's static array is
    double prev[3] = { 0, 0, 0 };
    double prev_drift = 0;
    bool has_prev = false;
    int jump_rejects = 0;
    uint64_t origin = 0;
    uint64_t next_tick = 10;                    // seconds after origin
    std::string diag;                           // the solver's unconditional stderr lines of the last solve

    void say(const char *fmt, ...) __attribute__((format(printf, 2, 3)))
    {
        char line[256];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(line, sizeof line, fmt, ap);
        va_end(ap);
        diag += line;
    }

    int add(const irdm_decoded_t &f);
    // the iterated fit over rows[0..n) with non-zero weight; lambda damping only in the first one
    bool fit(int n, double rx[3], double *drift, bool damped, bool first, const char *fail_singular);
    int solve(irdm_position_t *out);
};

int irdm_doppler::add(const irdm_decoded_t &f)
{
    if (f.type != 1) return 0;
    if (f.sat_id == 0) return 0;
    if (f.lat < -90 || f.lat > 90) return 0;
    if (f.lon < -180 || f.lon > 180) return 0;
    double e[3];
    for (int k = 0; k < 3; k++) e[k] = (double)f.pos_xyz[k] * 4000.0;
    const double r = norm3(e);
    if (r < 7050e3 || r > 7250e3) return 0;
    Sat *s = nullptr;
    for (Sat &c : sats)
        if (c.id == f.sat_id) { s = &c; break; }
    if (!s) {
        if ((int)sats.size() >= kMaxSats) return 0;
        sats.emplace_back();
        s = &sats.back();
        memset(s, 0, sizeof(*s));
        s->id = f.sat_id;
    }
    if (s->count > 0) {
        const Meas &last = s->m[(s->head - 1 + kMeasPerSat) % kMeasPerSat];
        const double dt = (double)(f.timestamp - last.ts) / 1e9;
        if (dt > kGapResetS) {                  // a new pass (or another satellite with the same 7-bit id)
            s->count = 0;
            s->head = 0;
            s->chan = 0;
        } else {
            const double dx = e[0] - last.ecef[0], dy = e[1] - last.ecef[1], dz = e[2] - last.ecef[2];
            const double dist = sqrt(dx * dx + dy * dy + dz * dz);
            if (dt > 0 && dt < 120 && dist / dt > 10000.0) return 0;      // faster than 10 km/s
        }
    }
    Meas &m = s->m[s->head];
    for (int k = 0; k < 3; k++) m.ecef[k] = e[k];
    m.freq = f.frequency;
    m.ts = f.timestamp;
    m.valid = 1;
    s->head = (s->head + 1) % kMeasPerSat;
    if (s->count < kMeasPerSat) s->count++;
    return 1;
}

bool irdm_doppler::fit(int n, double rx[3], double *drift, bool damped, bool first, const char *fail_singular)
{
    for (int iter = 0; iter < kMaxIter; iter++) {
        double N[4][4] = { { 0 } };
        double y[4] = { 0 };
        const Model md(rx);
        for (int i = 0; i < n; i++) {
            const Row &m = rows[i];
            if (!first && m.weight == 0) continue;
            double los[3], rel[3], rho, rdot, H[4];
            if (!md.geom(m, los, rel, &rho, &rdot)) continue;
            const double dy = m.range_rate - (rdot + *drift);
            Model::jacobian(los, rel, rho, rdot, H);
            accumulate(N, y, H, m.weight, dy);
        }
        {                                       // height aiding: geodetic altitude, radial direction, weight 100
            const double r0 = norm3(rx);
            if (r0 > 0) {
                double hl, hn, ha;
                to_geodetic(rx, &hl, &hn, &ha);
                const double dy = height - ha;
                const double H[4] = { rx[0] / r0, rx[1] / r0, rx[2] / r0, 0.0 };
                accumulate(N, y, H, 100.0, dy);
            }
        }
        if (damped) {                           // Levenberg-Marquardt, shrinking with the iterations
            const double lambda = iter < 10 ? 10.0 : iter < 50 ? 1.0 : 0.01;
            for (int i = 0; i < 4; i++) N[i][i] += lambda * N[i][i] + 1e-6;
        }
        double inv[4][4];
        if (invert4(N, inv) != 0) {
            say(fail_singular, iter);
            return false;
        }
        double d[4] = { 0 };
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) d[i] += inv[i][j] * y[j];
        if (damped) {                           // at most 500 km per step
            const double step = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            if (step > 500000.0) {
                const double sc = 500000.0 / step;
                for (int k = 0; k < 4; k++) d[k] *= sc;
            }
        }
        rx[0] += d[0];
        rx[1] += d[1];
        rx[2] += d[2];
        *drift += d[3];
        if (sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) < kConvergeM) return true;
    }
    return false;
}

int irdm_doppler::solve(irdm_position_t *out)
{
    memset(out, 0, sizeof(*out));
    diag.clear();
    const int ns = (int)sats.size();
    uint64_t now = 0;
    for (Sat &s : sats)
        for (int i = 0; i < s.count; i++) {
            const Meas *m = s.at(i);
            if (m && m->valid && m->ts > now) now = m->ts;
        }
    auto recent = [&](const Meas *m) { return !(now > 0 && now - m->ts > kMaxAgeNs); };

    // visibility: satellites with orbital motion (a velocity estimate) cluster within 8000 km of the one with the most
    // neighbours (ties: the most velocity estimates); newcomers without motion join when their latest recent position
    // lies near it.  With fewer than three moving satellites every satellite with a recent measurement is kept.
    int keep[kMaxSats] = { 0 };
    {
        double pos[kMaxSats][3];
        int moving[kMaxSats] = { 0 }, n_vel[kMaxSats] = { 0 };
        int n_moving = 0;
        for (int s = 0; s < ns; s++) {
            if (sats[s].count < 2) continue;
            int latest = -1;
            for (int i = sats[s].count - 1; i >= 0; i--) {
                const Meas *m = sats[s].at(i);
                if (!m || !m->valid || !recent(m)) continue;
                double v[3];
                if (velocity_of(sats[s], i, v) == 0) {
                    n_vel[s]++;
                    if (latest < 0) latest = i;
                }
            }
            if (latest >= 0) {
                memcpy(pos[s], sats[s].at(latest)->ecef, sizeof(pos[s]));
                moving[s] = 1;
                n_moving++;
            }
        }
        if (n_moving >= 3) {
            int nb[kMaxSats] = { 0 };
            for (int i = 0; i < ns; i++) {
                if (!moving[i]) continue;
                for (int j = i + 1; j < ns; j++) {
                    if (!moving[j]) continue;
                    double d[3];
                    sub3(pos[i], pos[j], d);
                    if (norm3(d) < kClusterDist) { nb[i]++; nb[j]++; }
                }
            }
            int core = -1, best_nb = -1, best_vel = -1;
            for (int s = 0; s < ns; s++) {
                if (!moving[s]) continue;
                if (nb[s] > best_nb || (nb[s] == best_nb && n_vel[s] > best_vel)) {
                    best_nb = nb[s];
                    best_vel = n_vel[s];
                    core = s;
                }
            }
            if (core >= 0) {
                keep[core] = 1;
                for (int s = 0; s < ns; s++) {
                    if (s == core) continue;
                    double d[3];
                    if (!moving[s]) {
                        for (int i = sats[s].count - 1; i >= 0; i--) {
                            const Meas *m = sats[s].at(i);
                            if (!m || !m->valid || !recent(m)) continue;
                            sub3(m->ecef, pos[core], d);
                            if (norm3(d) < kClusterDist) keep[s] = 1;
                            break;
                        }
                        continue;
                    }
                    sub3(pos[s], pos[core], d);
                    if (norm3(d) < kClusterDist) keep[s] = 1;
                }
            }
        } else {
            for (int s = 0; s < ns; s++)
                for (int i = sats[s].count - 1; i >= 0; i--) {
                    const Meas *m = sats[s].at(i);
                    if (m && m->valid && (now == 0 || now - m->ts <= kMaxAgeNs)) { keep[s] = 1; break; }
                }
        }
    }

    // the rows: every recent measurement of a kept satellite with a velocity, range rate against the voted channel
    if (rows.size() < (size_t)kMaxSats * kMeasPerSat) rows.resize((size_t)kMaxSats * kMeasPerSat);
    int n = 0, used = 0;
    for (int s = 0; s < ns && n < kMaxSats * kMeasPerSat; s++) {
        if (!keep[s]) continue;
        const double chan = channel_of(sats[s], now);
        if (chan == 0) continue;
        int contributed = 0;
        for (int i = 0; i < sats[s].count; i++) {
            const Meas *m = sats[s].at(i);
            if (!m || !m->valid) continue;
            if (now - m->ts > kMaxAgeNs) continue;
            double v[3];
            if (velocity_of(sats[s], i, v) != 0) continue;
            const double fd = m->freq - chan;
            const double lambda = kC / chan;
            Row &r = rows[n++];
            memcpy(r.ecef, m->ecef, sizeof(r.ecef));
            memcpy(r.vel, v, sizeof(r.vel));
            r.range_rate = -lambda * fd;
            r.weight = 1.0;
            r.sat = s;
            contributed = 1;
            if (n >= kMaxSats * kMeasPerSat) break;
        }
        // (the reference leaves the loop without counting the satellite that fills the array)
        if (contributed && n < kMaxSats * kMeasPerSat) used++;
    }
    if (n < kMinMeas || used < kMinSats) {
        out->n_measurements = n;
        out->n_satellites = used;
        return 0;
    }

    // start: the previous solution, else the count-weighted mean of the latest sub-satellite points, put on the aiding height
    double rx[3] = { 0, 0, 0 };
    double drift = 0;
    if (has_prev) {
        memcpy(rx, prev, sizeof(rx));
        drift = prev_drift;
    } else {
        double tw = 0;
        for (int s = 0; s < ns; s++) {
            if (!keep[s] || sats[s].count == 0) continue;
            const Meas *latest = nullptr;
            for (int i = sats[s].count - 1; i >= 0; i--) {
                const Meas *m = sats[s].at(i);
                if (m && m->valid) { latest = m; break; }
            }
            if (!latest) continue;
            const double r = norm3(latest->ecef);
            if (r <= 0) continue;
            const double sc = kA / r;
            const double w = (double)sats[s].count;
            for (int k = 0; k < 3; k++) rx[k] += latest->ecef[k] * sc * w;
            tw += w;
        }
        if (tw > 0)
            for (int k = 0; k < 3; k++) rx[k] /= tw;
        double la, lo, al;
        to_geodetic(rx, &la, &lo, &al);
        to_ecef(la, lo, height, rx);
    }

    if (!fit(n, rx, &drift, true, true, "DOPPLER: solver FAIL - singular matrix at iter %d\n")) {
        if (!diag.empty()) return 0;            // (singular: the reference returns without touching its state)
        out->n_measurements = n;
        out->n_satellites = used;
        has_prev = false;                       // a bad start may never converge: start afresh next time
        return 0;
    }

    // 3-sigma outliers of the residuals, and a re-solve without them
    const Model m1(rx);
    double sum2 = 0;
    int n_valid = 0, rejected = 0;
    for (int i = 0; i < n; i++) {
        Row &m = rows[i];
        double los[3], rel[3], rho, rdot;
        if (!m1.geom(m, los, rel, &rho, &rdot)) { m.weight = 0; continue; }
        const double res = m.range_rate - (rdot + drift);
        sum2 += res * res;
        n_valid++;
    }
    if (n_valid > 4) {
        const double sigma = sqrt(sum2 / (n_valid - 4));
        for (int i = 0; i < n; i++) {
            Row &m = rows[i];
            if (m.weight == 0) continue;
            double los[3], rel[3], rho, rdot;
            if (!m1.geom(m, los, rel, &rho, &rdot)) continue;
            if (fabs(m.range_rate - (rdot + drift)) > kOutlierSigma * sigma) {
                m.weight = 0;
                rejected++;
            }
        }
        if (rejected > 0 && n_valid - rejected >= kMinMeas) {
            if (!fit(n, rx, &drift, false, false, "DOPPLER: re-solve FAIL - singular matrix\n")) {
                if (diag.empty()) say("DOPPLER: re-solve FAIL - did not converge\n");
                return 0;
            }
            n = n_valid - rejected;
        }
    }

    // per satellite: mean absolute residual; a satellite above 3x the median (of three or more) is dropped, and the fit
    // re-solved without it.  (The rows read here are rows[0 .. n + rejected), as the reference counts them -- which
    // reaches past this solve's rows into an earlier solve's when outliers were found but not re-solved.)
    {
        const int total = n + rejected;
        const Model m2(rx);
        double sum[kMaxSats] = { 0 };
        int cnt[kMaxSats] = { 0 };
        for (int i = 0; i < total; i++) {
            const Row &m = rows[i];
            if (m.weight == 0) continue;
            if (m.sat < 0 || m.sat >= kMaxSats) continue;
            double los[3], rel[3], rho, rdot;
            if (!m2.geom(m, los, rel, &rho, &rdot)) continue;
            sum[m.sat] += fabs(m.range_rate - (rdot + drift));
            cnt[m.sat]++;
        }
        double mean[kMaxSats];
        int active[kMaxSats], n_active = 0;
        for (int s = 0; s < kMaxSats; s++) {
            if (cnt[s] == 0) continue;
            mean[s] = sum[s] / cnt[s];
            active[n_active++] = s;
        }
        if (n_active >= 3) {
            double sorted[kMaxSats];
            for (int i = 0; i < n_active; i++) sorted[i] = mean[active[i]];
            for (int i = 1; i < n_active; i++) {
                const double key = sorted[i];
                int j = i - 1;
                while (j >= 0 && sorted[j] > key) { sorted[j + 1] = sorted[j]; j--; }
                sorted[j + 1] = key;
            }
            const double median = sorted[n_active / 2];
            int dropped = 0;
            for (int i = 0; i < n_active; i++) {
                const int s = active[i];
                if (mean[s] > 3.0 * median && median > 0) {
                    for (int j = 0; j < total; j++)
                        if (rows[j].sat == s) rows[j].weight = 0;
                    dropped++;
                    used--;
                }
            }
            if (dropped > 0) {
                int remaining = 0;
                for (int i = 0; i < total; i++)
                    if (rows[i].weight > 0) remaining++;
                if (remaining < kMinMeas || used < kMinSats) return 0;
                n = remaining;
                if (!fit(total, rx, &drift, false, false, "DOPPLER: per-sat re-solve FAIL - singular matrix\n"))
                    return 0;
            }
        }
    }

    // HDOP from the unweighted normal matrix of the rows still in, rotated to east / north / up
    const int total = n + rejected;
    double hdop = 99.9;
    {
        double N[4][4] = { { 0 } };
        int count = 0;
        const Model m3(rx);
        for (int i = 0; i < total; i++) {
            const Row &m = rows[i];
            if (m.weight == 0) continue;
            double los[3], rel[3], rho, rdot, H[4];
            if (!m3.geom(m, los, rel, &rho, &rdot)) continue;
            Model::jacobian(los, rel, rho, rdot, H);
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++) N[r][c] += H[r] * H[c];
            count++;
        }
        double Q[4][4];
        if (count >= 4 && invert4(N, Q) == 0) {
            double la, lo, al, R[3][3];
            to_geodetic(rx, &la, &lo, &al);
            enu_rotation(la, lo, R);
            double E[3][3] = { { 0 } };
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++)
                    for (int k = 0; k < 3; k++)
                        for (int l = 0; l < 3; l++) E[i][j] += R[i][k] * Q[k][l] * R[j][l];
            if (E[0][0] + E[1][1] > 0) hdop = sqrt(E[0][0] + E[1][1]);
        }
    }

    // a stationary receiver does not move 500 km between solves: report the previous position instead, unless this is
    // the fifth jump in a row
    if (has_prev) {
        const double dx = rx[0] - prev[0], dy = rx[1] - prev[1], dz = rx[2] - prev[2];
        if (sqrt(dx * dx + dy * dy + dz * dz) > kMaxJump) {
            if (++jump_rejects < 5) {
                to_geodetic(prev, &out->lat, &out->lon, &out->alt);
                out->hdop = hdop;
                out->n_measurements = n;
                out->n_satellites = used;
                out->converged = 1;
                return 1;
            }
            jump_rejects = 0;
        } else {
            jump_rejects = 0;
        }
    }
    memcpy(prev, rx, sizeof(prev));
    prev_drift = drift;
    has_prev = true;
    to_geodetic(rx, &out->lat, &out->lon, &out->alt);
    out->hdop = hdop;
    out->n_measurements = n;
    out->n_satellites = used;
    out->converged = 1;
    return 1;
}

namespace {

// the stats thread's lines for one solve (main.c:506-519); final: the end of the stream, where the waiting line is
// always printed
void run_tick(irdm_doppler *d, std::string &o, bool wait_line)
{
    irdm_position_t s;
    const int ok = d->solve(&s);
    o += d->diag;
    char line[160];
    if (ok)
        snprintf(line, sizeof line, "POSITION: %.6f, %.6f (HDOP=%.1f, %d sats, %d meas)\n", s.lat, s.lon, s.hdop,
                 s.n_satellites, s.n_measurements);
    else if (wait_line)
        snprintf(line, sizeof line, "POSITION: waiting (%d sats, %d meas)\n", s.n_satellites, s.n_measurements);
    else
        return;
    o += line;
}

// the ticks at or before stream time t (ns after the origin)
void ticks_until(irdm_doppler *d, uint64_t t, std::string &o)
{
    while (t >= d->next_tick * 1000000000ULL) {
        run_tick(d, o, d->next_tick % 60 == 0);
        d->next_tick += 10;
    }
}

void at_frame(irdm_doppler *d, uint64_t ts, std::string &o)
{
    if (ts >= d->origin) ticks_until(d, ts - d->origin, o);
}

long long give(const std::string &o, char *buf, size_t cap)
{
    if (!buf || o.size() + 1 > cap) return -1;
    memcpy(buf, o.data(), o.size());
    buf[o.size()] = 0;
    return (long long)o.size();
}

}  // namespace

extern "C" irdm_doppler_t *irdm_doppler_create(double height_m)
{
    irdm_doppler *d = new (std::nothrow) irdm_doppler();
    if (d) d->height = height_m;
    return d;
}

extern "C" void irdm_doppler_destroy(irdm_doppler_t *d) { delete d; }

extern "C" int irdm_doppler_add(irdm_doppler_t *d, const irdm_decoded_t *f)
{
    return d && f ? d->add(*f) : 0;
}

extern "C" int irdm_doppler_solve(irdm_doppler_t *d, irdm_position_t *out)
{
    if (!d || !out) return 0;
    return d->solve(out);
}

extern "C" void irdm_doppler_set_origin(irdm_doppler_t *d, uint64_t start_time_ns)
{
    if (d) d->origin = start_time_ns;
}

extern "C" long long irdm_format_doppler_packed_batch(irdm_doppler_t *d, const irdm_demod_packed_t *f,
                                                      const irdm_frame_packed_t *fr, int n, char *buf, size_t cap)
{
    if (!d || !f || !fr || n < 0) return -1;
    std::string o;
    for (int i = 0; i < n; i++) {
        at_frame(d, f[i].timestamp, o);
        if (f[i].ok && fr[i].type == 1) {
            irdm_decoded_t dec;
            irdm_frame_unpack(&fr[i], &f[i], &dec);
            d->add(dec);
        }
    }
    return give(o, buf, cap);
}

extern "C" long long irdm_format_doppler_batch(irdm_doppler_t *d, const irdm_decoded_t *f, int n, char *buf, size_t cap)
{
    if (!d || !f || n < 0) return -1;
    std::string o;
    for (int i = 0; i < n; i++) {
        at_frame(d, f[i].timestamp, o);
        d->add(f[i]);
    }
    return give(o, buf, cap);
}

extern "C" long long irdm_doppler_finish(irdm_doppler_t *d, uint64_t end_ns, char *buf, size_t cap)
{
    if (!d) return -1;
    std::string o;
    if (end_ns >= d->origin) ticks_until(d, end_ns - d->origin, o);
    run_tick(d, o, true);
    return give(o, buf, cap);
}
