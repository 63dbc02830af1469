// recording.cpp -- irdm_recording_probe (include/irdm_hip.h): the headers of self-describing recordings.
//
// Host code only: no HIP header, no device call.  Three containers, recognised by the file's extension (or forced by the
// caller), never by content:
//   WAV / RF64 (SDR#, SDRuno, HDSDR, SDR Console)   RIFF chunks; fmt, [ds64], [auxi], data
//   SigMF (GNU Radio, SDRangel, rx_tools forks)     a JSON metadata file beside the data file (the small reader below)
//   SDRangel .sdriq                                 a 32-byte header with a CRC-32
// The probe says what the samples are (an IRDM_FMT_*), the rate, the centre and the start time where the file has them, and
// which bytes of which file hold the samples.  Nothing is read as samples here.
#include <ctype.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <memory>
#include <string>
#include <vector>
#include "../../include/irdm_hip.h"

namespace {

struct Err {
    char *buf;
    size_t cap;
    int fail(const char *fmt, ...) const __attribute__((format(printf, 2, 3)))
    {
        if (buf && cap) {
            va_list ap;
            va_start(ap, fmt);
            vsnprintf(buf, cap, fmt, ap);
            va_end(ap);
        }
        return -1;
    }
};

bool ends_with_nocase(const std::string &s, const char *suffix)
{
    const size_t n = strlen(suffix);
    return s.size() >= n && strcasecmp(s.c_str() + s.size() - n, suffix) == 0;
}

uint32_t rd16(const unsigned char *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
uint32_t rd32(const unsigned char *p) { return rd16(p) | (rd16(p + 2) << 16); }
uint64_t rd64(const unsigned char *p) { return (uint64_t)rd32(p) | ((uint64_t)rd32(p + 4) << 32); }

bool file_size(const char *path, uint64_t *size)
{
    struct stat st;
    if (stat(path, &st) != 0 || !S_ISREG(st.st_mode)) return false;
    *size = (uint64_t)st.st_size;
    return true;
}

// days since 1970-01-01 of a proleptic Gregorian date
long long days_from_civil(long long y, int m, int d)
{
    y -= m <= 2;
    const long long era = (y >= 0 ? y : y - 399) / 400;
    const long long yoe = y - era * 400;
    const long long doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;
    const long long doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
    return era * 146097 + doe - 719468;
}

// a date and time that exists (the day within its month's length, leap years included; second 60: a leap second)
bool civil_ok(int y, int mo, int d, int h, int mi, int s)
{
    static const int len[12] = { 31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31 };
    if (y < 1970 || mo < 1 || mo > 12 || d < 1 || h < 0 || h > 23 || mi < 0 || mi > 59 || s < 0 || s > 60) return false;
    const bool leap = (y % 4 == 0 && y % 100 != 0) || y % 400 == 0;
    return d <= len[mo - 1] + (mo == 2 && leap ? 1 : 0);
}

uint64_t civil_ns(int y, int mo, int d, int h, int mi, int s, uint64_t frac_ns)
{
    const long long secs = days_from_civil(y, mo, d) * 86400ll + h * 3600ll + mi * 60ll + s;
    return (uint64_t)secs * 1000000000ull + frac_ns;
}

size_t sample_bytes(int fmt) { return irdm_format_bytes(fmt); }      // (every format a probe names is a valid one)

// the data file's path into the struct; false (and a message) when it does not fit
bool set_path(irdm_recording_info_t *out, const std::string &p, const Err &e)
{
    if (p.size() >= sizeof(out->data_path)) {
        e.fail("the data file's path has %zu bytes, at most %zu fit", p.size(), sizeof(out->data_path) - 1);
        return false;
    }
    memcpy(out->data_path, p.c_str(), p.size() + 1);
    return true;
}

// ---- WAV / RF64 ----

// _<digits>Hz or _<digits>kHz in the file's name (SDR#, SDRuno)
bool centre_from_name(const std::string &path, double *hz)
{
    const size_t slash = path.find_last_of('/');
    const std::string name = slash == std::string::npos ? path : path.substr(slash + 1);
    for (size_t i = 0; i + 1 < name.size(); i++) {
        if (name[i] != '_' || !isdigit((unsigned char)name[i + 1])) continue;
        size_t j = i + 1;
        while (j < name.size() && isdigit((unsigned char)name[j])) j++;
        if (j - (i + 1) > 15) continue;
        const double v = strtod(name.substr(i + 1, j - (i + 1)).c_str(), nullptr);
        if (name.compare(j, 2, "Hz") == 0) { *hz = v; return true; }
        if (name.compare(j, 3, "kHz") == 0) { *hz = v * 1000.0; return true; }
    }
    return false;
}

int probe_wav(const char *path, irdm_recording_info_t *out, const Err &e)
{
    uint64_t fsize = 0;
    FILE *f = fopen(path, "rb");
    if (!f || !file_size(path, &fsize)) {
        if (f) fclose(f);
        return e.fail("%s: cannot open", path);
    }
    std::unique_ptr<FILE, int (*)(FILE *)> closer(f, fclose);
    unsigned char h[12];
    if (fread(h, 1, 12, f) != 12) return e.fail("%s: truncated header: %llu bytes, a RIFF header has 12", path, (unsigned long long)fsize);
    const bool rf64 = !memcmp(h, "RF64", 4) || !memcmp(h, "BW64", 4);
    if ((memcmp(h, "RIFF", 4) && !rf64) || memcmp(h + 8, "WAVE", 4)) return e.fail("%s: not a RIFF / RF64 WAVE file", path);
    bool have_fmt = false, have_data = false, have_ds64 = false;
    uint64_t ds64_data = 0, pos = 12;
    int tag = 0, channels = 0, bits = 0;
    uint32_t rate = 0;
    while (pos + 8 <= fsize) {
        unsigned char ch[8];
        if (fseeko(f, (off_t)pos, SEEK_SET) != 0 || fread(ch, 1, 8, f) != 8) break;
        const uint32_t size = rd32(ch + 4);
        const uint64_t body = pos + 8;
        if (!memcmp(ch, "data", 4)) {
            if (!have_fmt) return e.fail("%s: data chunk at offset %llu before any fmt chunk", path, (unsigned long long)pos);
            if (have_data) {                                        // a second data chunk: the first one holds the samples
                pos = body + size + (size & 1);
                continue;
            }
            uint64_t n = size;
            bool open_end = size == 0 || size == 0xffffffffu;
            if (size == 0xffffffffu && rf64 && have_ds64 && ds64_data != 0 && ds64_data != ~0ull) {
                n = ds64_data;
                open_end = false;
            }
            if (open_end || n > fsize - body) {
                n = fsize - body;
                open_end = true;
            }
            out->data_offset = body;
            out->data_bytes = n;
            have_data = true;
            if (open_end) break;                                    // nothing behind samples that run to the end of the file
            pos = body + n + (n & 1);
            continue;
        }
        if (size > fsize - body) {
            if (have_data) break;                                   // (a damaged chunk behind the samples takes nothing away)
            return e.fail("%s: truncated: chunk '%.4s' at offset %llu has %u bytes, the file ends after %llu", path, (const char *)ch,
                          (unsigned long long)pos, size, (unsigned long long)(fsize - body));
        }
        if (!memcmp(ch, "ds64", 4) && size >= 24) {
            unsigned char d[24];
            if (fread(d, 1, 24, f) != 24) break;
            ds64_data = rd64(d + 8);
            have_ds64 = true;
        } else if (!memcmp(ch, "fmt ", 4)) {
            if (size != 16 && size != 18 && size != 40) return e.fail("%s: fmt chunk at offset %llu has %u bytes (16, 18 or 40 expected)", path, (unsigned long long)pos, size);
            unsigned char d[40];
            if (fread(d, 1, size, f) != size) break;
            tag = (int)rd16(d);
            channels = (int)rd16(d + 2);
            rate = rd32(d + 4);
            bits = (int)rd16(d + 14);
            if (tag == 0xfffe) {
                if (size != 40) return e.fail("%s: extensible fmt chunk at offset %llu has %u bytes (40 expected)", path, (unsigned long long)pos, size);
                tag = (int)rd16(d + 24);                            // the first two bytes of the sub-format GUID
            }
            have_fmt = true;
        } else if (!memcmp(ch, "auxi", 4) && size >= 36) {
            unsigned char d[36];
            if (fread(d, 1, 36, f) != 36) break;
            const int y = (int)rd16(d), mo = (int)rd16(d + 2), day = (int)rd16(d + 6), hh = (int)rd16(d + 8), mi = (int)rd16(d + 10),
                      ss = (int)rd16(d + 12), ms = (int)rd16(d + 14);
            // (SDR#'s newer auxi is XML text: its first bytes read as a year far outside this range)
            if (y >= 1990 && y <= 2100 && civil_ok(y, mo, day, hh, mi, ss) && ms < 1000) {
                out->has_start = 1;
                out->start_time_ns = civil_ns(y, mo, day, hh, mi, ss, (uint64_t)ms * 1000000ull);
                out->has_center = 1;
                out->center_frequency = (double)rd32(d + 32);
            }
        }
        pos = body + size + (size & 1);
    }
    if (!have_fmt) return e.fail("%s: truncated: no fmt chunk in %llu bytes", path, (unsigned long long)fsize);
    if (!have_data) return e.fail("%s: truncated: no data chunk in %llu bytes", path, (unsigned long long)fsize);
    if (channels != 2) return e.fail("%s: %d channel%s: a recording has 2 (I, Q)", path, channels, channels == 1 ? "" : "s");
    if (bits == 24) return e.fail("%s: 24 bits per sample (packed): not supported, convert to 16- or 32-bit", path);
    if (tag == 1 && bits == 8) out->format = IRDM_FMT_CU8;
    else if (tag == 1 && bits == 16) out->format = IRDM_FMT_CI16_FULL;
    else if (tag == 1 && bits == 32) out->format = IRDM_FMT_CI32;
    else if (tag == 3 && bits == 32) out->format = IRDM_FMT_CF32;
    else return e.fail("%s: %d bits per sample with format tag %d: not supported (8, 16, 32-bit PCM or 32-bit float)", path, bits, tag);
    if (rate == 0 || rate > 0x7fffffffu) return e.fail("%s: sample rate %u", path, rate);
    out->sample_rate = (int)rate;
    if (!out->has_center && centre_from_name(path, &out->center_frequency)) out->has_center = 1;
    out->data_bytes -= out->data_bytes % sample_bytes(out->format);
    out->kind = IRDM_CONTAINER_WAV;
    out->n_captures = 1;
    return set_path(out, path, e) ? 0 : -1;
}

// ---- a small JSON reader (SigMF metadata) ----

struct Json {
    enum Kind { Null, Bool, Num, Str, Arr, Obj } kind = Null;
    bool b = false;
    double num = 0.0;
    std::string text;                   // Str: the string; Num: the number as written
    std::vector<Json> arr;
    std::vector<std::pair<std::string, Json>> obj;
    const Json *get(const char *key) const
    {
        if (kind != Obj) return nullptr;
        for (const auto &kv : obj)
            if (kv.first == key) return &kv.second;
        return nullptr;
    }
};

struct JsonParser {
    const char *s;
    size_t n, i = 0;
    std::string err;
    int depth = 0;
    bool fail(const char *what)
    {
        if (err.empty()) err = std::string(what) + " at byte " + std::to_string(i);
        return false;
    }
    void ws() { while (i < n && (s[i] == ' ' || s[i] == '\t' || s[i] == '\n' || s[i] == '\r')) i++; }
    static void utf8(std::string &o, unsigned cp)
    {
        if (cp < 0x80) o += (char)cp;
        else if (cp < 0x800) { o += (char)(0xc0 | (cp >> 6)); o += (char)(0x80 | (cp & 0x3f)); }
        else if (cp < 0x10000) { o += (char)(0xe0 | (cp >> 12)); o += (char)(0x80 | ((cp >> 6) & 0x3f)); o += (char)(0x80 | (cp & 0x3f)); }
        else { o += (char)(0xf0 | (cp >> 18)); o += (char)(0x80 | ((cp >> 12) & 0x3f)); o += (char)(0x80 | ((cp >> 6) & 0x3f)); o += (char)(0x80 | (cp & 0x3f)); }
    }
    bool hex4(unsigned *v)
    {
        if (i + 4 > n) return fail("truncated \\u escape");
        *v = 0;
        for (int k = 0; k < 4; k++) {
            const char c = s[i++];
            if (!isxdigit((unsigned char)c)) return fail("bad \\u escape");
            *v = *v * 16 + (unsigned)(isdigit((unsigned char)c) ? c - '0' : (tolower(c) - 'a' + 10));
        }
        return true;
    }
    bool string(std::string &o)
    {
        if (i >= n || s[i] != '"') return fail("string expected");
        i++;
        while (i < n && s[i] != '"') {
            char c = s[i++];
            if (c != '\\') { o += c; continue; }
            if (i >= n) return fail("truncated escape");
            c = s[i++];
            switch (c) {
            case '"': case '\\': case '/': o += c; break;
            case 'b': o += '\b'; break;
            case 'f': o += '\f'; break;
            case 'n': o += '\n'; break;
            case 'r': o += '\r'; break;
            case 't': o += '\t'; break;
            case 'u': {
                unsigned cp = 0, lo = 0;
                if (!hex4(&cp)) return false;
                if (cp >= 0xd800 && cp < 0xdc00 && i + 1 < n && s[i] == '\\' && s[i + 1] == 'u') {
                    i += 2;
                    if (!hex4(&lo)) return false;
                    cp = 0x10000 + ((cp - 0xd800) << 10) + ((lo - 0xdc00) & 0x3ff);
                }
                utf8(o, cp);
                break;
            }
            default: return fail("bad escape");
            }
        }
        if (i >= n) return fail("unterminated string");
        i++;
        return true;
    }
    bool value(Json &v)
    {
        if (++depth > 64) return fail("nested too deeply");
        ws();
        if (i >= n) return fail("value expected");
        const char c = s[i];
        bool ok = true;
        if (c == '{') {
            v.kind = Json::Obj;
            i++;
            ws();
            if (i < n && s[i] == '}') i++;
            else
                for (;;) {
                    ws();
                    std::string key;
                    Json child;
                    if (!string(key)) return false;
                    ws();
                    if (i >= n || s[i] != ':') return fail("':' expected");
                    i++;
                    if (!value(child)) return false;
                    v.obj.emplace_back(std::move(key), std::move(child));
                    ws();
                    if (i < n && s[i] == ',') { i++; continue; }
                    if (i < n && s[i] == '}') { i++; break; }
                    return fail("',' or '}' expected");
                }
        } else if (c == '[') {
            v.kind = Json::Arr;
            i++;
            ws();
            if (i < n && s[i] == ']') i++;
            else
                for (;;) {
                    Json child;
                    if (!value(child)) return false;
                    v.arr.push_back(std::move(child));
                    ws();
                    if (i < n && s[i] == ',') { i++; continue; }
                    if (i < n && s[i] == ']') { i++; break; }
                    return fail("',' or ']' expected");
                }
        } else if (c == '"') {
            v.kind = Json::Str;
            ok = string(v.text);
        } else if (c == '-' || isdigit((unsigned char)c)) {
            const size_t i0 = i;
            while (i < n && (isdigit((unsigned char)s[i]) || s[i] == '-' || s[i] == '+' || s[i] == '.' || s[i] == 'e' || s[i] == 'E')) i++;
            v.kind = Json::Num;
            v.text.assign(s + i0, i - i0);
            char *end = nullptr;
            v.num = strtod(v.text.c_str(), &end);
            if (!end || *end) { i = i0; return fail("bad number"); }
        } else if (n - i >= 4 && !memcmp(s + i, "true", 4)) {
            v.kind = Json::Bool; v.b = true; i += 4;
        } else if (n - i >= 5 && !memcmp(s + i, "false", 5)) {
            v.kind = Json::Bool; i += 5;
        } else if (n - i >= 4 && !memcmp(s + i, "null", 4)) {
            i += 4;
        } else {
            return fail("value expected");
        }
        depth--;
        return ok;
    }
};

// a non-negative whole number, written as an integer or as a float (2.4e6)
bool whole_number(const Json *j, uint64_t *v)
{
    if (!j || j->kind != Json::Num) return false;
    bool digits = !j->text.empty();
    for (char c : j->text) digits = digits && isdigit((unsigned char)c);
    if (digits && j->text.size() <= 19) {
        *v = strtoull(j->text.c_str(), nullptr, 10);
        return true;
    }
    if (!(j->num >= 0.0) || j->num > 9.0e18 || j->num != floor(j->num)) return false;
    *v = (uint64_t)j->num;
    return true;
}

// ISO 8601, UTC: YYYY-MM-DDTHH:MM:SS[.fraction][Z | +hh:mm | -hh:mm]; the fraction is kept to the nanosecond (cut, not rounded)
bool parse_datetime(const std::string &t, uint64_t *ns)
{
    int y, mo, d, h, mi, s, used = 0;
    if (sscanf(t.c_str(), "%4d-%2d-%2d%*1[Tt ]%2d:%2d:%2d%n", &y, &mo, &d, &h, &mi, &s, &used) != 6 || used == 0) return false;
    if (!civil_ok(y, mo, d, h, mi, s)) return false;
    size_t i = (size_t)used;
    uint64_t frac = 0;
    if (i < t.size() && (t[i] == '.' || t[i] == ',')) {
        i++;
        int nd = 0;
        if (i >= t.size() || !isdigit((unsigned char)t[i])) return false;
        for (; i < t.size() && isdigit((unsigned char)t[i]); i++, nd++)
            if (nd < 9) frac = frac * 10 + (uint64_t)(t[i] - '0');
        for (; nd < 9; nd++) frac *= 10;
    }
    long long off = 0;
    if (i < t.size() && (t[i] == 'Z' || t[i] == 'z')) {
        i++;
    } else if (i < t.size() && (t[i] == '+' || t[i] == '-')) {
        int oh = 0, om = 0, u2 = 0;
        if (sscanf(t.c_str() + i + 1, "%2d:%2d%n", &oh, &om, &u2) != 2 || u2 != 5) return false;
        off = (t[i] == '+' ? 1 : -1) * (oh * 3600ll + om * 60ll);
        i += 6;
    }
    if (i != t.size()) return false;
    const long long secs = days_from_civil(y, mo, d) * 86400ll + h * 3600ll + mi * 60ll + s - off;
    if (secs < 0) return false;
    *ns = (uint64_t)secs * 1000000000ull + frac;
    return true;
}

int probe_sigmf(const char *path_c, irdm_recording_info_t *out, const Err &e)
{
    const std::string path = path_c;
    const bool named_data = ends_with_nocase(path, ".sigmf-data");
    std::string meta = path;
    if (named_data) meta = path.substr(0, path.size() - 4) + (path[path.size() - 4] == 'D' ? "META" : "meta");
    FILE *f = fopen(meta.c_str(), "rb");
    if (!f && named_data) {                                         // (the sibling in the other letter case)
        meta = path.substr(0, path.size() - 4) + (path[path.size() - 4] == 'D' ? "meta" : "META");
        f = fopen(meta.c_str(), "rb");
    }
    if (!f) return e.fail("%s: cannot open the metadata file %s", path_c, meta.c_str());
    std::string text;
    char buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0 && text.size() < ((size_t)64 << 20)) text.append(buf, got);
    fclose(f);
    JsonParser jp{ text.data(), text.size() };
    Json root;
    if (!jp.value(root)) return e.fail("%s: malformed JSON: %s", meta.c_str(), jp.err.c_str());
    jp.ws();
    if (jp.i != jp.n) return e.fail("%s: malformed JSON: text behind the document at byte %zu", meta.c_str(), jp.i);
    const Json *g = root.get("global");
    if (!g || g->kind != Json::Obj) return e.fail("%s: no \"global\" object", meta.c_str());
    const Json *dt = g->get("core:datatype");
    if (!dt || dt->kind != Json::Str) return e.fail("%s: global has no core:datatype", meta.c_str());
    if (dt->text == "cf32_le") out->format = IRDM_FMT_CF32;
    else if (dt->text == "ci16_le") out->format = IRDM_FMT_CI16_FULL;
    else if (dt->text == "ci8" || dt->text == "ci8_le") out->format = IRDM_FMT_CI8;
    else if (dt->text == "cu8" || dt->text == "cu8_le") out->format = IRDM_FMT_CU8;
    else if (dt->text == "ci32_le") out->format = IRDM_FMT_CI32;
    else return e.fail("%s: core:datatype \"%s\" is not supported (cf32_le, ci16_le, ci8, cu8, ci32_le)", meta.c_str(), dt->text.c_str());
    uint64_t rate = 0;
    const Json *sr = g->get("core:sample_rate");
    if (!sr) return e.fail("%s: global has no core:sample_rate", meta.c_str());
    if (!whole_number(sr, &rate) || rate == 0 || rate > 0x7fffffffull)
        return e.fail("%s: core:sample_rate %s is not a whole number of samples per second in range", meta.c_str(), sr->text.c_str());
    out->sample_rate = (int)rate;
    if (const Json *nc = g->get("core:num_channels")) {
        uint64_t c = 0;
        if (!whole_number(nc, &c) || c != 1) return e.fail("%s: core:num_channels %s: one channel expected", meta.c_str(), nc->text.c_str());
    }
    uint64_t trailing = 0, header = 0;
    if (const Json *tb = g->get("core:trailing_bytes"))
        if (!whole_number(tb, &trailing)) return e.fail("%s: core:trailing_bytes %s", meta.c_str(), tb->text.c_str());
    out->n_captures = 0;
    const Json *caps = root.get("captures");
    if (caps && caps->kind == Json::Arr && !caps->arr.empty()) {
        out->n_captures = (int)caps->arr.size();
        const Json &c0 = caps->arr[0];
        if (c0.kind != Json::Obj) return e.fail("%s: captures[0] is no object", meta.c_str());
        if (const Json *ss = c0.get("core:sample_start")) {
            uint64_t v = 1;
            if (!whole_number(ss, &v) || v != 0) return e.fail("%s: captures[0] core:sample_start %s: 0 expected", meta.c_str(), ss->text.c_str());
        }
        if (const Json *fq = c0.get("core:frequency")) {
            if (fq->kind != Json::Num) return e.fail("%s: captures[0] core:frequency is no number", meta.c_str());
            out->has_center = 1;
            out->center_frequency = fq->num;
        }
        if (const Json *d = c0.get("core:datetime")) {
            if (d->kind != Json::Str || !parse_datetime(d->text, &out->start_time_ns))
                return e.fail("%s: captures[0] core:datetime \"%s\" is no ISO 8601 time", meta.c_str(), d->kind == Json::Str ? d->text.c_str() : "?");
            out->has_start = 1;
        }
        if (const Json *hb = c0.get("core:header_bytes"))
            if (!whole_number(hb, &header)) return e.fail("%s: captures[0] core:header_bytes %s", meta.c_str(), hb->text.c_str());
    }
    // the data file: the one named; else core:dataset in the metadata's directory; else the sibling
    std::string data;
    const Json *ds = g->get("core:dataset");
    if (named_data) {
        data = path;
    } else if (ds && ds->kind == Json::Str && !ds->text.empty()) {
        if (ds->text.find('/') != std::string::npos) return e.fail("%s: core:dataset \"%s\" names a directory", meta.c_str(), ds->text.c_str());
        const size_t slash = meta.find_last_of('/');
        data = (slash == std::string::npos ? std::string() : meta.substr(0, slash + 1)) + ds->text;
    } else if (ends_with_nocase(meta, ".sigmf-meta")) {
        data = meta.substr(0, meta.size() - 4) + (meta[meta.size() - 4] == 'M' ? "DATA" : "data");
    } else {
        return e.fail("%s: no core:dataset, and the name does not end in .sigmf-meta", meta.c_str());
    }
    uint64_t size = 0;
    if (!set_path(out, data, e)) return -1;
    if (!file_size(data.c_str(), &size)) return e.fail("%s: cannot open the data file %s", meta.c_str(), data.c_str());
    if (header > size || trailing > size - header)
        return e.fail("%s: core:header_bytes %llu and core:trailing_bytes %llu exceed the %llu bytes of %s", meta.c_str(),
                      (unsigned long long)header, (unsigned long long)trailing, (unsigned long long)size, data.c_str());
    out->data_offset = header;
    out->data_bytes = size - header - trailing;
    out->data_bytes -= out->data_bytes % sample_bytes(out->format);
    out->kind = IRDM_CONTAINER_SIGMF;
    return 0;
}

// ---- SDRangel .sdriq ----

uint32_t crc32_zlib(const unsigned char *p, size_t n)
{
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
    }
    return ~c;
}

int probe_sdriq(const char *path, irdm_recording_info_t *out, const Err &e)
{
    uint64_t fsize = 0;
    FILE *f = fopen(path, "rb");
    if (!f || !file_size(path, &fsize)) {
        if (f) fclose(f);
        return e.fail("%s: cannot open", path);
    }
    unsigned char h[32];
    const size_t got = fread(h, 1, 32, f);
    fclose(f);
    if (got != 32) return e.fail("%s: truncated header: %zu bytes, an .sdriq header has 32", path, got);
    const uint32_t crc = crc32_zlib(h, 28), want = rd32(h + 28);
    if (crc != want) return e.fail("%s: header CRC-32 %08x, the file says %08x", path, crc, want);
    const uint32_t rate = rd32(h), size = rd32(h + 20);
    if (rate == 0 || rate > 0x7fffffffu) return e.fail("%s: sample rate %u", path, rate);
    if (size == 16) out->format = IRDM_FMT_CI16_FULL;
    else if (size == 24) out->format = IRDM_FMT_CI32_24;
    else return e.fail("%s: sample size %u at offset 20 (16 or 24 expected)", path, size);
    out->sample_rate = (int)rate;
    out->has_center = 1;
    out->center_frequency = (double)rd64(h + 4);
    const uint64_t t = rd64(h + 12);                                // seconds (older SDRangel) or milliseconds
    if (t >= 100000000000ull ? t <= ~0ull / 1000000ull : t <= ~0ull / 1000000000ull) {     // (else: no time that 64 bits of ns hold)
        out->has_start = 1;
        out->start_time_ns = t >= 100000000000ull ? t * 1000000ull : t * 1000000000ull;
    }
    out->data_offset = 32;
    out->data_bytes = fsize - 32;
    out->data_bytes -= out->data_bytes % sample_bytes(out->format);
    out->kind = IRDM_CONTAINER_SDRIQ;
    out->n_captures = 1;
    return set_path(out, path, e) ? 0 : -1;
}

}  // namespace

extern "C" int irdm_recording_probe(const char *path, int container, irdm_recording_info_t *out, char *err, size_t err_cap)
{
    if (err && err_cap) err[0] = 0;
    const Err e{ err, err_cap };
    if (!path || !out) return e.fail("irdm_recording_probe: null argument");
    const std::string p = path;
    int kind = container;
    if (kind == IRDM_CONTAINER_NONE) {
        if (ends_with_nocase(p, ".wav") || ends_with_nocase(p, ".wave") || ends_with_nocase(p, ".rf64")) kind = IRDM_CONTAINER_WAV;
        else if (ends_with_nocase(p, ".sigmf-meta") || ends_with_nocase(p, ".sigmf-data")) kind = IRDM_CONTAINER_SIGMF;
        else if (ends_with_nocase(p, ".sdriq")) kind = IRDM_CONTAINER_SDRIQ;
        else if (ends_with_nocase(p, ".sigmf")) return e.fail("%s: SigMF archives are not supported: unpack the .sigmf-meta / .sigmf-data pair", path);
        else {
            out->kind = IRDM_CONTAINER_NONE;
            return 1;
        }
    }
    if (strlen(path) >= sizeof(out->data_path)) return e.fail("irdm_recording_probe: path too long");
    memset(out, 0, sizeof(*out));
    switch (kind) {
    case IRDM_CONTAINER_WAV: return probe_wav(path, out, e);
    case IRDM_CONTAINER_SIGMF: return probe_sigmf(path, out, e);
    case IRDM_CONTAINER_SDRIQ: return probe_sdriq(path, out, e);
    default: return e.fail("irdm_recording_probe: unknown container %d", container);
    }
}
