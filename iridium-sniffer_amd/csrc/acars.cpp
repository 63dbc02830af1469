// acars.cpp -- --acars / --acars-json: multi-burst IDA reassembly (ida_decode.c:669-748), SBD packet extraction and
// multi-packet reassembly (sbd_acars.c:1002-1218) and the ACARS printer of a build without libacars
// (sbd_acars.c:603-998), on the host.  It runs once per CRC-valid IDA burst and once per message -- a few hundred per
// second -- and reads only the frame and IDA records the caller already polls: no kernel, no device copy, no host
// synchronisation.  ARINC-622 decoding (the libacars path) and the UDP / TCP feeds are not built.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <new>
#include <string>

#include "../../include/irdm_hip.h"

namespace {

constexpr int kIdaSlots = 16;                          // IDA_MAX_REASSEMBLY (ida_decode.h:70)
constexpr uint64_t kIdaGapNs = 280000000ULL;           // ida_decode.c:683, :745
constexpr int kSbdSlots = 8;                           // SBD_MAX_MULTI (sbd_acars.c:374)
constexpr int kSbdMaxData = 1024;                      // SBD_MAX_DATA
constexpr uint64_t kSbdTimeoutNs = 5000000000ULL;      // SBD_TIMEOUT_NS
constexpr int kJsonBuf = 8192;                         // JSON_BUF_SIZE (sbd_acars.c:63)
constexpr int kDirUplink = 2;                          // ir_direction_t DIR_UPLINK

// printf onto a byte string: %c of a NUL byte lands in the output as printf would write it to stdout
void app(std::string &s, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void app(std::string &s, const char *fmt, ...)
{
    char tmp[512];
    va_list ap;
    va_start(ap, fmt);
    va_list ap2;
    va_copy(ap2, ap);
    const int n = vsnprintf(tmp, sizeof(tmp), fmt, ap);
    va_end(ap);
    if (n < 0) { va_end(ap2); return; }
    if ((size_t)n < sizeof(tmp)) {
        s.append(tmp, (size_t)n);
    } else {
        std::string big((size_t)n + 1, '\0');
        vsnprintf(&big[0], big.size(), fmt, ap2);
        s.append(big.data(), (size_t)n);
    }
    va_end(ap2);
}

struct IdaSlot {
    int active;
    int direction;
    double frequency;
    uint64_t last_timestamp;
    int last_ctr;
    uint8_t data[256];
    int data_len;
};

struct SbdSlot {
    int active, msgno, msgcnt, ul;
    uint64_t timestamp;
    double frequency;
    float magnitude;
    uint8_t data[kSbdMaxData];
    int data_len;
};

uint16_t crc16_kermit(const uint8_t *d, int n)
{
    // reflected CRC-16, polynomial 0x8408, initial value 0 (sbd_acars.c:344-368), bit by bit
    uint16_t crc = 0;
    for (int i = 0; i < n; i++) {
        crc ^= d[i];
        for (int k = 0; k < 8; k++) crc = (crc & 1) ? (uint16_t)((crc >> 1) ^ 0x8408) : (uint16_t)(crc >> 1);
    }
    return crc;
}

// the reference's json_escape (sbd_acars.c:613-641): out holds at most outsz - 1 characters, a pair or \uXXXX is not split
std::string json_escape(const uint8_t *in, int inlen, int outsz)
{
    std::string o;
    for (int i = 0; i < inlen && (int)o.size() < outsz - 2; i++) {
        const unsigned char c = in[i];
        const int used = (int)o.size();
        const char *pair = c == '"' ? "\\\"" : c == '\\' ? "\\\\" : c == '\n' ? "\\n" : c == '\r' ? "\\r" : c == '\t' ? "\\t" : nullptr;
        if (pair) {
            if (used + 2 >= outsz) break;
            o += pair;
        } else if (c < 0x20 || c == 0x7f) {
            if (used + 6 >= outsz) break;
            char u[8];
            snprintf(u, sizeof(u), "\\u%04x", c);
            o += u;
        } else {
            o += (char)c;
        }
    }
    return o;
}

std::string json_escape(const char *s, int outsz) { return json_escape((const uint8_t *)s, (int)strlen(s), outsz); }

}  // namespace

struct irdm_ida_reasm {
    IdaSlot slots[kIdaSlots];
};

struct irdm_acars {
    int json;
    std::string station;
    bool has_station;
    bool fixed_origin;
    struct timespec wall_t0;
    uint64_t first_ts;
    bool ts_init;
    SbdSlot sbd[kSbdSlots];
    irdm_acars_stats_t st;
};

namespace {

// ---- ida_reassemble (ida_decode.c:669-735), then ida_reassemble_flush (:738-746) at the frame's timestamp ----
// b: the frame's IDA record (nullptr or !b->ok: a frame ida_decode() did not take, which only flushes)
int reasm_frame(irdm_ida_reasm *r, const irdm_ida_t *b, uint64_t frame_ts, irdm_ida_message_t *out)
{
    int emitted = 0;
    if (b && b->ok && b->crc_ok && b->da_len > 0 && b->da_len <= (int)sizeof(b->payload)) {
        const int da_len = b->da_len;
        bool matched = false;
        // an open slot is tried first, so a ctr 0 burst continues a slot whose last ctr was 7
        for (int i = 0; i < kIdaSlots && !matched; i++) {
            IdaSlot &s = r->slots[i];
            if (!s.active || s.direction != b->direction) continue;
            if (fabs(s.frequency - b->frequency) > 260.0) continue;
            if (b->timestamp < s.last_timestamp || b->timestamp - s.last_timestamp > kIdaGapNs) continue;
            if ((s.last_ctr + 1) % 8 != b->da_ctr) continue;
            matched = true;
            if (s.data_len + da_len <= (int)sizeof(s.data)) {        // past 256 bytes the payload is dropped ...
                memcpy(s.data + s.data_len, b->payload, (size_t)da_len);
                s.data_len += da_len;
            }
            s.last_timestamp = b->timestamp;                         // ... but the slot still advances
            s.last_ctr = b->da_ctr;
            if (!b->cont) {
                memset(out, 0, sizeof(*out));
                memcpy(out->data, s.data, (size_t)s.data_len);
                out->len = s.data_len;
                out->timestamp = b->timestamp;
                out->frequency = s.frequency;
                out->direction = s.direction;
                out->magnitude = b->magnitude;
                s.active = 0;
                emitted = 1;
            }
        }
        if (!matched && b->da_ctr == 0 && !b->cont) {                // a single-burst message
            memset(out, 0, sizeof(*out));
            memcpy(out->data, b->payload, (size_t)da_len);
            out->len = da_len;
            out->timestamp = b->timestamp;
            out->frequency = b->frequency;
            out->direction = b->direction;
            out->magnitude = b->magnitude;
            emitted = 1;
        } else if (!matched && b->da_ctr == 0) {                     // the first burst of several: first free slot, else the oldest
            int idx = -1;
            uint64_t oldest = UINT64_MAX;
            for (int i = 0; i < kIdaSlots; i++) {
                if (!r->slots[i].active) { idx = i; break; }
                if (r->slots[i].last_timestamp < oldest) { oldest = r->slots[i].last_timestamp; idx = i; }
            }
            if (idx < 0) idx = 0;
            IdaSlot &s = r->slots[idx];
            s.active = 1;
            s.direction = b->direction;
            s.frequency = b->frequency;
            s.last_timestamp = b->timestamp;
            s.last_ctr = b->da_ctr;
            memcpy(s.data, b->payload, (size_t)da_len);
            s.data_len = da_len;
        }
        // (ctr > 0 without a slot: an orphan, dropped)
    }
    for (int i = 0; i < kIdaSlots; i++) {
        IdaSlot &s = r->slots[i];
        if (s.active && frame_ts > s.last_timestamp + kIdaGapNs) s.active = 0;
    }
    return emitted;
}

// ---- timestamps (sbd_acars.c:300-330): wall-clock origin + (ts - ts of the first printed message) ----
void ts_ensure_init(irdm_acars *a, uint64_t ts)
{
    if (a->ts_init) return;
    if (!a->fixed_origin) clock_gettime(CLOCK_REALTIME, &a->wall_t0);
    a->first_ts = ts;
    a->ts_init = true;
}

std::string format_timestamp(irdm_acars *a, uint64_t ts)
{
    ts_ensure_init(a, ts);
    const double elapsed = (double)(ts - a->first_ts) / 1e9;
    const time_t wall_sec = a->wall_t0.tv_sec + (time_t)elapsed;
    struct tm tm;
    gmtime_r(&wall_sec, &tm);
    char buf[32];
    strftime(buf, sizeof(buf), "%Y-%m-%dT%H:%M:%SZ", &tm);
    return buf;
}

double ts_to_unix(irdm_acars *a, uint64_t ts)
{
    ts_ensure_init(a, ts);
    return (double)a->wall_t0.tv_sec + (double)a->wall_t0.tv_nsec / 1e9 + (double)(ts - a->first_ts) / 1e9;
}

// the message text behind the block id: the trailing ETX dropped, or ETB dropped and the message marked continued
int strip_trailer(const uint8_t *rest, int &rest_len)
{
    if (rest_len > 0) {
        if (rest[rest_len - 1] == 0x03) {
            rest_len--;
        } else if (rest[rest_len - 1] == 0x17) {
            rest_len--;
            return 1;
        }
    }
    return 0;
}

// acars_output_json (sbd_acars.c:649-757), the dumpvdl2-style envelope; data: 7-bit characters, len >= 13
void output_json(irdm_acars *a, std::string &o, const uint8_t *data, int len, int ul, uint64_t ts, double freq,
                 float mag, const uint8_t *hdr, int hdr_len)
{
    const char mode = (char)data[0];
    char reg[8] = {0};
    memcpy(reg, data + 1, 7);                                   // leading dots kept
    const char ack = (char)data[8];
    char label[4] = {(char)data[9], (char)data[10], 0, 0};
    if (data[9] == '_' && data[10] == 0x7f) label[1] = 'd';
    const char blk_id = (char)data[11];
    const uint8_t *rest = data + 12;
    int rest_len = len - 12;
    const int cont = strip_trailer(rest, rest_len);
    char flight[8] = {0}, msg_num[4] = {0};
    char msg_num_seq = 0;
    const uint8_t *txt = nullptr;
    int txt_len = 0;
    if (rest_len > 0 && rest[0] == 0x02) {
        if (ul && rest_len >= 11) {
            memcpy(msg_num, rest + 1, 3);
            msg_num_seq = (char)rest[4];
            memcpy(flight, rest + 5, 6);
            txt = rest + 11;
            txt_len = rest_len - 11;
        } else {
            txt = rest + 1;
            txt_len = rest_len - 1;
        }
    }
    const double unix_time = ts_to_unix(a, ts);
    const long tv_sec = (long)unix_time;
    const long tv_usec = (long)((unix_time - (double)tv_sec) * 1000000.0);
    const std::string esc_text = txt && txt_len > 0 ? json_escape(txt, txt_len, 2048) : std::string();

    std::string j;
    app(j, "{\"iridium\":{\"app\":{\"name\":\"iridium-sniffer\",\"ver\":\"1.0\"}");
    if (a->has_station) app(j, ",\"station\":\"%s\"", a->station.c_str());
    app(j, ",\"t\":{\"sec\":%ld,\"usec\":%ld}", tv_sec, tv_usec);
    app(j, ",\"freq\":%lld", (long long)(int64_t)freq);
    app(j, ",\"sig_level\":%.2f", (double)mag);
    if (hdr && hdr_len > 0) {
        app(j, ",\"header\":\"");
        for (int i = 0; i < hdr_len; i++) app(j, "%02x", hdr[i]);
        app(j, "\"");
    }
    app(j, ",\"acars\":{\"err\":false,\"crc_ok\":true");
    app(j, ",\"more\":%s", cont ? "true" : "false");
    app(j, ",\"reg\":\"%s\"", json_escape(reg, 64).c_str());
    app(j, ",\"mode\":\"%c\"", mode);
    app(j, ",\"label\":\"%s\"", json_escape(label, 16).c_str());
    app(j, ",\"blk_id\":\"%c\"", blk_id);
    app(j, ",\"ack\":\"%c\"", ack);
    if (ul && flight[0]) {
        app(j, ",\"flight\":\"%s\"", json_escape(flight, 32).c_str());
        app(j, ",\"msg_num\":\"%s\"", json_escape(msg_num, 16).c_str());
        if (msg_num_seq) app(j, ",\"msg_num_seq\":\"%c\"", msg_num_seq);
    }
    if (!esc_text.empty()) app(j, ",\"msg_text\":\"%s\"", esc_text.c_str());
    app(j, "}}}");
    if (j.size() > (size_t)kJsonBuf - 1) j.resize((size_t)kJsonBuf - 1);     // the line buffer's limit
    o += j;
    o += '\n';
}

// acars_output_text (sbd_acars.c:759-855)
void output_text(irdm_acars *a, std::string &o, const uint8_t *data, int len, int ul, uint64_t ts, int errors)
{
    const std::string tsb = format_timestamp(a, ts);
    const char mode = (char)data[0];
    char reg[8] = {0};
    int reg_start = 1;
    while (reg_start < 8 && data[reg_start] == '.') reg_start++;    // leading dots stripped
    const int rlen = 8 - reg_start;
    if (rlen > 0) memcpy(reg, data + reg_start, (size_t)rlen);
    const bool is_nak = data[8] == 0x15;
    const char ack = (char)data[8];
    char label[4] = {(char)data[9], (char)data[10], 0, 0};
    if (data[9] == '_' && data[10] == 0x7f) label[1] = '?';
    const char bid = (char)data[11];
    const uint8_t *rest = data + 12;
    int rest_len = len - 12;
    const int cont = strip_trailer(rest, rest_len);

    app(o, "ACARS: %s %s Mode:%c REG:%-7s ", tsb.c_str(), ul ? "UL" : "DL", mode, reg);
    if (is_nak) app(o, "NAK  ");
    else app(o, "ACK:%c ", ack);
    app(o, "Label:%s bID:%c ", label, bid);
    if (rest_len > 0 && rest[0] == 0x02) {
        int from = 1;
        if (ul && rest_len >= 11) {
            app(o, "SEQ:%.4s FNO:%.6s ", (const char *)rest + 1, (const char *)rest + 5);
            from = 11;
        }
        if (rest_len > from) {
            o += '[';
            for (int i = from; i < rest_len; i++) o += (rest[i] >= 0x20 && rest[i] < 0x7f) ? (char)rest[i] : '.';
            o += ']';
        }
    }
    if (cont) o += " CONT'd";
    if (errors > 0) o += " ERRORS";
    o += '\n';
}

// acars_parse_fallback (sbd_acars.c:857-917)
void acars_parse(irdm_acars *a, std::string &o, const uint8_t *data, int len, int ul, uint64_t ts, double freq, float mag)
{
    if (len <= 2 || data[0] != 0x01) return;
    data++;
    len--;
    uint8_t csum[2] = {0, 0};
    bool has_crc = false;
    if (len >= 3 && data[len - 1] == 0x7f) {                    // a CRC trailer only when the last byte is DEL
        csum[0] = data[len - 3];
        csum[1] = data[len - 2];
        len -= 3;
        has_crc = true;
    }
    const uint8_t *hdr = nullptr;
    int hdr_len = 0;
    if (len >= 8 && data[0] == 0x03) {
        hdr = data;
        hdr_len = 8;
        data += 8;
        len -= 8;
    }
    int crc_errors = 0;
    if (has_crc) {
        uint8_t buf[kSbdMaxData];
        if (len + 2 <= (int)sizeof(buf)) {
            memcpy(buf, data, (size_t)len);
            buf[len] = csum[0];
            buf[len + 1] = csum[1];
            if (crc16_kermit(buf, len + 2) != 0) crc_errors = 1;
        }
    } else {
        crc_errors = 1;                                         // no trailer counts as an error
    }
    if (len < 13) return;
    uint8_t stripped[kSbdMaxData];
    bool parity_ok = true;
    for (int i = 0; i < len; i++) {
        if (__builtin_popcount(data[i]) % 2 == 0) parity_ok = false;      // odd parity per character
        stripped[i] = data[i] & 0x7f;
    }
    const int errors = crc_errors + (parity_ok ? 0 : 1);
    a->st.acars_total++;
    if (errors > 0) a->st.acars_errors++;
    if (a->json) {
        if (errors == 0) output_json(a, o, stripped, len, ul, ts, freq, mag, hdr, hdr_len);
    } else {
        output_text(a, o, stripped, len, ul, ts, errors);
    }
}

// sbd_process (sbd_acars.c:946-966): ACARS when the packet starts with SOH; any other SBD prints nothing under --acars
void sbd_process(irdm_acars *a, std::string &o, const uint8_t *d, int len, int ul, uint64_t ts, double freq, float mag)
{
    if (len > 2 && d[0] == 0x01) acars_parse(a, o, d, len, ul, ts, freq, mag);
}

// sbd_extract (sbd_acars.c:978-1114) for one reassembled IDA message
void sbd_extract(irdm_acars *a, std::string &o, const uint8_t *data, int len, int ul, uint64_t ts, double freq, float mag)
{
    if (len < 5) return;
    bool is_sbd = false;
    if (data[0] == 0x76 && data[1] != 5) {
        is_sbd = ul ? (data[1] >= 0x0c && data[1] <= 0x0e) : (data[1] >= 0x08 && data[1] <= 0x0b);
    } else if (data[0] == 0x06 && data[1] == 0x00) {
        const uint8_t t = data[2];
        is_sbd = t == 0x00 || t == 0x10 || t == 0x20 || t == 0x40 || t == 0x50 || t == 0x70;
    }
    if (!is_sbd) return;
    a->st.sbd_total++;
    const uint8_t typ0 = data[0], typ1 = data[1];
    data += 2;
    len -= 2;
    int msgno = 0, msgcnt = 0;
    const uint8_t *sbd = nullptr;
    int sbd_len = 0;
    if (typ0 == 0x06) {
        if (len < 30 || data[0] != 0x20) return;
        msgcnt = data[15];
        msgno = msgcnt == 0 ? 0 : 1;
        sbd = data + 29;
        sbd_len = len - 29;
    } else {
        if (typ1 == 0x08) {                                     // the pre-header: 5 bytes after 0x20, 7 otherwise
            if (len < 5) return;
            const int pre = data[0] == 0x20 ? 5 : 7;
            if (len < pre) return;
            msgcnt = data[3];
            data += pre;
            len -= pre;
        } else {
            msgcnt = -1;
        }
        if (ul && len >= 3 && (data[0] == 0x50 || data[0] == 0x51)) {
            data += 3;
            len -= 3;
        }
        if (len > 3 && data[0] == 0x10) {                       // packet header: 0x10, length, message number
            const int pkt_len = data[1];
            msgno = data[2];
            data += 3;
            len -= 3;
            if (len < pkt_len) return;
            if (len > pkt_len) len = pkt_len;
        } else {
            msgno = 0;
        }
        sbd = data;
        sbd_len = len;
    }
    for (int i = 0; i < kSbdSlots; i++)                          // sbd_expire, before each packet
        if (a->sbd[i].active && ts > a->sbd[i].timestamp + kSbdTimeoutNs) a->sbd[i].active = 0;

    if (msgno == 0) {
        a->st.sbd_short++;
        if (sbd_len > 0) sbd_process(a, o, sbd, sbd_len, ul, ts, freq, mag);
    } else if (msgcnt == 1 && msgno == 1) {
        a->st.sbd_single++;
        sbd_process(a, o, sbd, sbd_len, ul, ts, freq, mag);
    } else if (msgcnt > 1) {                                     // a new multi-packet message: first free slot, else the oldest
        int idx = -1;
        for (int i = 0; i < kSbdSlots; i++)
            if (!a->sbd[i].active) { idx = i; break; }
        if (idx < 0) {
            uint64_t oldest = UINT64_MAX;
            for (int i = 0; i < kSbdSlots; i++)
                if (a->sbd[i].timestamp < oldest) { oldest = a->sbd[i].timestamp; idx = i; }
        }
        if (idx < 0) idx = 0;
        SbdSlot &s = a->sbd[idx];
        s.active = 1;
        s.msgno = msgno;
        s.msgcnt = msgcnt;
        s.ul = ul;
        s.timestamp = ts;
        s.frequency = freq;
        s.magnitude = mag;
        s.data_len = sbd_len > kSbdMaxData ? kSbdMaxData : sbd_len;
        memcpy(s.data, sbd, (size_t)s.data_len);
    } else if (msgno > 1) {                                      // a continuation: searched from the last slot down
        for (int i = kSbdSlots - 1; i >= 0; i--) {
            SbdSlot &s = a->sbd[i];
            if (!s.active || s.ul != ul || msgno != s.msgno + 1) continue;
            const int space = kSbdMaxData - s.data_len;
            const int copy = sbd_len > space ? space : sbd_len;
            if (copy > 0) {
                memcpy(s.data + s.data_len, sbd, (size_t)copy);
                s.data_len += copy;
            }
            s.msgno = msgno;
            s.timestamp = ts;
            a->st.sbd_multi_frag++;
            if (msgno == s.msgcnt) {
                a->st.sbd_multi_ok++;
                sbd_process(a, o, s.data, s.data_len, ul, ts, s.frequency, s.magnitude);
                s.active = 0;
            }
            return;
        }
        a->st.sbd_broken++;
    }
}

void acars_message(irdm_acars *a, std::string &o, const irdm_ida_message_t &m)
{
    a->st.ida_total++;
    sbd_extract(a, o, m.data, m.len, m.direction == kDirUplink ? 1 : 0, m.timestamp, m.frequency, m.magnitude);
}

long long put_out(const std::string &s, char *buf, size_t cap)
{
    if (s.size() + 1 > cap) return -1;
    memcpy(buf, s.data(), s.size());
    buf[s.size()] = 0;
    return (long long)s.size();
}

bool step_ok(const irdm_ida_t *b) { return b && b->ok; }

}  // namespace

extern "C" {

irdm_ida_reasm_t *irdm_ida_reasm_create(void) { return (irdm_ida_reasm_t *)calloc(1, sizeof(irdm_ida_reasm)); }

void irdm_ida_reasm_destroy(irdm_ida_reasm_t *r) { free(r); }

int irdm_ida_reasm_push(irdm_ida_reasm_t *r, const irdm_ida_t *b, int n, irdm_ida_message_t *out, int max)
{
    if (!r || n < 0 || (n > 0 && !b) || max < n || (n > 0 && !out)) return -1;
    int k = 0;
    for (int i = 0; i < n; i++) k += reasm_frame(r, &b[i], b[i].timestamp, out + k);
    return k;
}

int irdm_ida_reasm_push_packed(irdm_ida_reasm_t *r, const irdm_demod_packed_t *f, const irdm_ida_packed_t *idas, int n,
                               irdm_ida_message_t *out, int max)
{
    if (!r || n < 0 || (n > 0 && (!f || !idas || !out)) || max < n) return -1;
    int k = 0;
    for (int i = 0; i < n; i++) {
        irdm_ida_t b;
        if (idas[i].ok) irdm_ida_unpack(&idas[i], &f[i], &b);
        k += reasm_frame(r, idas[i].ok ? &b : nullptr, f[i].timestamp, out + k);
    }
    return k;
}

irdm_acars_t *irdm_acars_create(const irdm_acars_config_t *cfg)
{
    irdm_acars *a = new (std::nothrow) irdm_acars();
    if (!a) return nullptr;
    memset(&a->wall_t0, 0, sizeof(a->wall_t0));
    memset(a->sbd, 0, sizeof(a->sbd));
    memset(&a->st, 0, sizeof(a->st));
    a->first_ts = 0;
    a->ts_init = false;
    a->json = cfg ? cfg->json != 0 : 0;
    a->has_station = cfg && cfg->station;
    if (a->has_station) a->station = cfg->station;
    a->fixed_origin = cfg && cfg->fixed_origin;
    if (a->fixed_origin) {
        a->wall_t0.tv_sec = (time_t)cfg->origin_sec;
        a->wall_t0.tv_nsec = (long)cfg->origin_nsec;
    }
    return a;
}

void irdm_acars_destroy(irdm_acars_t *a) { delete a; }

long long irdm_acars_feed(irdm_acars_t *a, const irdm_ida_message_t *m, int n, char *buf, size_t cap)
{
    if (!a || n < 0 || (n > 0 && !m) || !buf || cap == 0) return -1;
    std::string o;
    for (int i = 0; i < n; i++) acars_message(a, o, m[i]);
    return put_out(o, buf, cap);
}

int irdm_acars_stats(const irdm_acars_t *a, irdm_acars_stats_t *out)
{
    if (!a || !out) return -1;
    *out = a->st;
    return 0;
}

int irdm_acars_format_stats(const irdm_acars_t *a, char *buf, size_t cap)
{
    if (!a || !buf || cap == 0) return -1;
    const irdm_acars_stats_t &s = a->st;
    std::string o;
    app(o, "SBD: %d packets from %d IDA messages (%d short, %d single, %d multi-pkt)\n", s.sbd_total, s.ida_total,
        s.sbd_short, s.sbd_single, s.sbd_multi_ok);
    if (s.sbd_multi_frag > 0 || s.sbd_broken > 0)
        app(o, "SBD: %d multi-pkt fragments, %d broken/orphan\n", s.sbd_multi_frag, s.sbd_broken);
    app(o, "ACARS: %d messages decoded", s.acars_total);
    if (s.acars_errors > 0) app(o, " (%d with errors)", s.acars_errors);
    o += '\n';
    return (int)put_out(o, buf, cap);
}

// main.c:322-361 for one frame: its IDA line (--parsed and ok), no RAW line (suppressed under --acars, before the printer
// would set its t0), then the ACARS lines of the messages it completes
static long long acars_frames(irdm_ida_reasm_t *r, irdm_acars_t *a, int n, int parsed, uint64_t *t0_io, char *buf,
                              size_t cap, const irdm_ida_t *(*rec)(const void *, const void *, int, irdm_ida_t *),
                              uint64_t (*frame_ts)(const void *, int), const void *f, const void *idas)
{
    if (!r || !a || n < 0 || !t0_io || !buf || cap == 0) return -1;
    std::string o;
    char line[IRDM_RAW_LINE_MAX];
    for (int i = 0; i < n; i++) {
        irdm_ida_t tmp;
        const irdm_ida_t *b = rec(f, idas, i, &tmp);
        if (parsed && step_ok(b)) {
            const int len = irdm_format_ida(b, t0_io, line, sizeof(line));
            if (len < 0) return -1;
            o.append(line, (size_t)len);
        }
        irdm_ida_message_t m;
        if (reasm_frame(r, b, frame_ts(f, i), &m)) acars_message(a, o, m);
    }
    return put_out(o, buf, cap);
}

long long irdm_format_acars_packed_batch(irdm_ida_reasm_t *r, irdm_acars_t *a, const irdm_demod_packed_t *f,
                                         const irdm_ida_packed_t *idas, int n, int parsed, uint64_t *t0_io, char *buf,
                                         size_t cap)
{
    if (n > 0 && (!f || !idas)) return -1;
    return acars_frames(
        r, a, n, parsed, t0_io, buf, cap,
        [](const void *fp, const void *ip, int i, irdm_ida_t *tmp) -> const irdm_ida_t * {
            const irdm_ida_packed_t *id = (const irdm_ida_packed_t *)ip + i;
            if (!id->ok) return nullptr;
            irdm_ida_unpack(id, (const irdm_demod_packed_t *)fp + i, tmp);
            return tmp;
        },
        [](const void *fp, int i) { return ((const irdm_demod_packed_t *)fp)[i].timestamp; }, f, idas);
}

long long irdm_format_acars_batch(irdm_ida_reasm_t *r, irdm_acars_t *a, const irdm_demod_t *f, const irdm_ida_t *idas,
                                  int n, int parsed, uint64_t *t0_io, char *buf, size_t cap)
{
    if (n > 0 && (!f || !idas)) return -1;
    return acars_frames(
        r, a, n, parsed, t0_io, buf, cap,
        [](const void *, const void *ip, int i, irdm_ida_t *) { return (const irdm_ida_t *)ip + i; },
        [](const void *fp, int i) { return ((const irdm_demod_t *)fp)[i].timestamp; }, f, idas);
}

}  // extern "C"
