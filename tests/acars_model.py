"""A Python restatement of --acars / --acars-json, independent of csrc/acars.cpp: the tests' checker.

IdaReasm is the reference's ida_reassemble / ida_reassemble_flush (ida_decode.c:669-748), Acars its SBD extraction,
multi-packet reassembly and ACARS printer as it builds without libacars (sbd_acars.c:603-1218, stats :1336-1349).
Messages are dicts: data (bytes), timestamp (ns), frequency (Hz), direction (1 DL, 2 UL), magnitude.

The builders at the end make ACARS / SBD payloads for fixtures and scenes."""
import struct
import time

import numpy as np

U64 = (1 << 64) - 1
DIR_UL = 2


def f32(x):
    return float(np.float32(x))


class IdaReasm:
    SLOTS = 16
    GAP = 280_000_000

    def __init__(self):
        self.slots = [None] * self.SLOTS           # dict(direction, frequency, last_ts, last_ctr, data) or None

    def push(self, burst, frame_ts):
        """one frame: burst (dict ok, crc_ok, da_ctr, da_len, cont, payload, direction, timestamp, frequency, magnitude)
        or None for a frame that is not IDA; returns the completed message or None"""
        msg = None
        b = burst
        if b is not None and b["ok"] and b["crc_ok"] and b["da_len"] != 0:
            pl = bytes(b["payload"][:b["da_len"]])
            matched = False
            for s in self.slots:
                if s is None or s["direction"] != b["direction"]:
                    continue
                if abs(s["frequency"] - b["frequency"]) > 260.0:
                    continue
                if b["timestamp"] < s["last_ts"] or b["timestamp"] - s["last_ts"] > self.GAP:
                    continue
                if (s["last_ctr"] + 1) % 8 != b["da_ctr"]:
                    continue
                matched = True
                if len(s["data"]) + len(pl) <= 256:
                    s["data"] += pl
                s["last_ts"], s["last_ctr"] = b["timestamp"], b["da_ctr"]
                if not b["cont"]:
                    msg = dict(data=bytes(s["data"]), timestamp=b["timestamp"], frequency=s["frequency"],
                               direction=s["direction"], magnitude=b["magnitude"])
                    self.slots[self.slots.index(s)] = None
                break
            if not matched and b["da_ctr"] == 0 and not b["cont"]:
                msg = dict(data=pl, timestamp=b["timestamp"], frequency=b["frequency"], direction=b["direction"],
                           magnitude=b["magnitude"])
            elif not matched and b["da_ctr"] == 0:
                idx = None
                oldest = U64
                for i, s in enumerate(self.slots):
                    if s is None:
                        idx = i
                        break
                    if s["last_ts"] < oldest:
                        oldest, idx = s["last_ts"], i
                self.slots[idx if idx is not None else 0] = dict(
                    direction=b["direction"], frequency=b["frequency"], last_ts=b["timestamp"], last_ctr=0,
                    data=bytearray(pl))
        for i, s in enumerate(self.slots):
            if s is not None and frame_ts > s["last_ts"] + self.GAP:
                self.slots[i] = None
        return msg


def crc16_kermit(data):
    crc = 0
    for c in data:
        crc ^= c
        for _ in range(8):
            crc = (crc >> 1) ^ 0x8408 if crc & 1 else crc >> 1
    return crc


def json_escape(data, outsz):
    o = ""
    for c in data:
        if len(o) >= outsz - 2:
            break
        pair = {0x22: '\\"', 0x5c: "\\\\", 0x0a: "\\n", 0x0d: "\\r", 0x09: "\\t"}.get(c)
        if pair:
            if len(o) + 2 >= outsz:
                break
            o += pair
        elif c < 0x20 or c == 0x7f:
            if len(o) + 6 >= outsz:
                break
            o += "\\u%04x" % c
        else:
            o += chr(c)
    return o


def cstr(b):
    """a char array read with %s: up to its first NUL"""
    b = bytes(b)
    return b.split(b"\0", 1)[0]


STAT_NAMES = ("ida_total", "sbd_total", "sbd_short", "sbd_single", "sbd_multi_ok", "sbd_multi_frag", "sbd_broken",
              "acars_total", "acars_errors")


class Acars:
    SBD_SLOTS = 8
    SBD_MAX = 1024
    TIMEOUT = 5_000_000_000

    def __init__(self, json=False, station=None, origin=None):
        """origin: (sec, nsec) of the wall clock at the first printed message"""
        self.json, self.station = bool(json), station
        if origin is None:
            t = time.clock_gettime_ns(time.CLOCK_REALTIME)
            origin = (t // 10**9, t % 10**9)
        self.origin = origin
        self.first = None
        self.sbd = [None] * self.SBD_SLOTS
        self.st = dict.fromkeys(STAT_NAMES, 0)

    # ---- timestamps ----
    def _init_ts(self, ts):
        if self.first is None:
            self.first = ts

    def _fmt_ts(self, ts):
        self._init_ts(ts)
        elapsed = float((ts - self.first) & U64) / 1e9
        sec = self.origin[0] + int(elapsed)
        return time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime(sec))

    def _unix(self, ts):
        self._init_ts(ts)
        return float(self.origin[0]) + float(self.origin[1]) / 1e9 + float((ts - self.first) & U64) / 1e9

    # ---- printers ----
    @staticmethod
    def _trailer(rest):
        if rest and rest[-1] == 0x03:
            return rest[:-1], False
        if rest and rest[-1] == 0x17:
            return rest[:-1], True
        return rest, False

    def _json(self, d, ul, ts, freq, mag, hdr):
        reg = cstr(d[1:8])
        label = bytearray(d[9:11])
        if d[9] == 0x5f and d[10] == 0x7f:
            label[1] = ord("d")
        rest, cont = self._trailer(d[12:])
        flight = msg_num = b""
        seq = 0
        txt = b""
        if rest and rest[0] == 0x02:
            if ul and len(rest) >= 11:
                msg_num, seq, flight, txt = cstr(rest[1:4]), rest[4], cstr(rest[5:11]), rest[11:]
            else:
                txt = rest[1:]
        u = self._unix(ts)
        sec = int(u)
        usec = int((u - float(sec)) * 1000000.0)
        esc = json_escape(txt, 2048) if txt else ""
        j = '{"iridium":{"app":{"name":"iridium-sniffer","ver":"1.0"}'
        if self.station is not None:
            j += ',"station":"%s"' % self.station.encode().decode("latin-1")
        j += ',"t":{"sec":%d,"usec":%d}' % (sec, usec)
        j += ',"freq":%d' % int(freq)
        j += ',"sig_level":%.2f' % f32(mag)
        if hdr:
            j += ',"header":"%s"' % bytes(hdr).hex()
        j += ',"acars":{"err":false,"crc_ok":true'
        j += ',"more":%s' % ("true" if cont else "false")
        j += ',"reg":"%s"' % json_escape(reg, 64)
        j += ',"mode":"%s"' % chr(d[0])
        j += ',"label":"%s"' % json_escape(cstr(label), 16)
        j += ',"blk_id":"%s"' % chr(d[11])
        j += ',"ack":"%s"' % chr(d[8])
        if ul and flight:
            j += ',"flight":"%s"' % json_escape(flight, 32)
            j += ',"msg_num":"%s"' % json_escape(msg_num, 16)
            if seq:
                j += ',"msg_num_seq":"%s"' % chr(seq)
        if esc:
            j += ',"msg_text":"%s"' % esc
        j += "}}}"
        return j[:8191] + "\n"

    def _text(self, d, ul, ts, errors):
        tsb = self._fmt_ts(ts)
        r = 1
        while r < 8 and d[r] == 0x2e:
            r += 1
        reg = cstr(d[r:8]).decode("latin-1")
        label = bytes(d[9:11]) if not (d[9] == 0x5f and d[10] == 0x7f) else b"_?"
        rest, cont = self._trailer(d[12:])
        o = "ACARS: %s %s Mode:%s REG:%-7s " % (tsb, "UL" if ul else "DL", chr(d[0]), reg)
        o += "NAK  " if d[8] == 0x15 else "ACK:%s " % chr(d[8])
        o += "Label:%s bID:%s " % (cstr(label).decode("latin-1"), chr(d[11]))
        if rest and rest[0] == 0x02:
            start = 1
            if ul and len(rest) >= 11:
                o += "SEQ:%s FNO:%s " % (cstr(rest[1:5]).decode("latin-1"), cstr(rest[5:11]).decode("latin-1"))
                start = 11
            if len(rest) > start:
                o += "[" + "".join(chr(c) if 0x20 <= c < 0x7f else "." for c in rest[start:]) + "]"
        if cont:
            o += " CONT'd"
        if errors:
            o += " ERRORS"
        return o + "\n"

    def _acars(self, data, ul, ts, freq, mag):
        if len(data) <= 2 or data[0] != 0x01:
            return ""
        d = bytes(data[1:])
        csum = None
        if len(d) >= 3 and d[-1] == 0x7f:
            csum, d = d[-3:-1], d[:-3]
        hdr = None
        if len(d) >= 8 and d[0] == 0x03:
            hdr, d = d[:8], d[8:]
        crc_err = 1
        if csum is not None:
            crc_err = 0
            if len(d) + 2 <= self.SBD_MAX and crc16_kermit(d + csum) != 0:
                crc_err = 1
        if len(d) < 13:
            return ""
        parity_ok = all(bin(c).count("1") % 2 for c in d)
        s = bytes(c & 0x7f for c in d)
        errors = crc_err + (0 if parity_ok else 1)
        self.st["acars_total"] += 1
        if errors:
            self.st["acars_errors"] += 1
        if self.json:
            return "" if errors else self._json(s, ul, ts, freq, mag, hdr)
        return self._text(s, ul, ts, errors)

    def _process(self, data, ul, ts, freq, mag):
        if len(data) > 2 and data[0] == 0x01:
            return self._acars(data, ul, ts, freq, mag)
        return ""                                            # (non-ACARS SBD prints nothing under --acars)

    def _extract(self, data, ul, ts, freq, mag):
        if len(data) < 5:
            return ""
        t0, t1 = data[0], data[1]
        if t0 == 0x76 and t1 != 5:
            is_sbd = 0x0c <= t1 <= 0x0e if ul else 0x08 <= t1 <= 0x0b
        elif t0 == 0x06 and t1 == 0x00:
            is_sbd = data[2] in (0x00, 0x10, 0x20, 0x40, 0x50, 0x70)
        else:
            is_sbd = False
        if not is_sbd:
            return ""
        self.st["sbd_total"] += 1
        d = data[2:]
        if t0 == 0x06:
            if len(d) < 30 or d[0] != 0x20:
                return ""
            msgcnt = d[15]
            msgno = 0 if msgcnt == 0 else 1
            sbd = d[29:]
        else:
            if t1 == 0x08:
                if len(d) < 5:
                    return ""
                pre = 5 if d[0] == 0x20 else 7
                if len(d) < pre:
                    return ""
                msgcnt = d[3]
                d = d[pre:]
            else:
                msgcnt = -1
            if ul and len(d) >= 3 and d[0] in (0x50, 0x51):
                d = d[3:]
            if len(d) > 3 and d[0] == 0x10:
                pkt_len, msgno = d[1], d[2]
                d = d[3:]
                if len(d) < pkt_len:
                    return ""
                sbd = d[:pkt_len]
            else:
                msgno, sbd = 0, d
        for i, s in enumerate(self.sbd):
            if s is not None and s["active"] and ts > s["ts"] + self.TIMEOUT:
                s["active"] = False
        if msgno == 0:
            self.st["sbd_short"] += 1
            return self._process(sbd, ul, ts, freq, mag) if sbd else ""
        if msgcnt == 1 and msgno == 1:
            self.st["sbd_single"] += 1
            return self._process(sbd, ul, ts, freq, mag)
        if msgcnt > 1:
            idx = next((i for i, s in enumerate(self.sbd) if s is None or not s["active"]), None)
            if idx is None:
                oldest = U64
                for i, s in enumerate(self.sbd):
                    if s["ts"] < oldest:
                        oldest, idx = s["ts"], i
            self.sbd[idx] = dict(active=True, msgno=msgno, msgcnt=msgcnt, ul=ul, ts=ts, freq=freq, mag=mag,
                                 data=bytearray(sbd[:self.SBD_MAX]))
            return ""
        if msgno > 1:
            for s in reversed(self.sbd):
                if s is None or not s["active"] or s["ul"] != ul or msgno != s["msgno"] + 1:
                    continue
                s["data"] += sbd[:self.SBD_MAX - len(s["data"])]
                s["msgno"], s["ts"] = msgno, ts
                self.st["sbd_multi_frag"] += 1
                if msgno == s["msgcnt"]:
                    self.st["sbd_multi_ok"] += 1
                    s["active"] = False
                    return self._process(bytes(s["data"]), ul, ts, s["freq"], s["mag"])
                return ""
            self.st["sbd_broken"] += 1
        return ""

    def feed(self, msgs):
        """acars_ida_cb for each message: the text the reference prints (latin-1 str)"""
        out = ""
        for m in msgs:
            self.st["ida_total"] += 1
            out += self._extract(bytes(m["data"]), 1 if m["direction"] == DIR_UL else 0, m["timestamp"],
                                 m["frequency"], m["magnitude"])
        return out

    def stats_text(self):
        s = self.st
        o = "SBD: %d packets from %d IDA messages (%d short, %d single, %d multi-pkt)\n" % (
            s["sbd_total"], s["ida_total"], s["sbd_short"], s["sbd_single"], s["sbd_multi_ok"])
        if s["sbd_multi_frag"] > 0 or s["sbd_broken"] > 0:
            o += "SBD: %d multi-pkt fragments, %d broken/orphan\n" % (s["sbd_multi_frag"], s["sbd_broken"])
        o += "ACARS: %d messages decoded" % s["acars_total"]
        if s["acars_errors"] > 0:
            o += " (%d with errors)" % s["acars_errors"]
        return o + "\n"


# ---------------------------------------------------------------- builders ----
def odd_parity(b):
    return bytes((c & 0x7f) | (0 if bin(c & 0x7f).count("1") % 2 else 0x80) for c in b)


def acars_block(mode=b"2", reg=b".N12345", ack=b"\x15", label=b"H1", bid=b"A", body=b"\x02HELLO\x03", hdr=None,
                crc="good", parity=True):
    """SOH + [8-byte 0x03 header] + the parity-coded block + CRC-16/Kermit (little-endian) + DEL.
    crc: "good", "bad" (checksum off by one) or None (no trailer)"""
    blk = mode + reg + ack + label + bid + body
    blk = odd_parity(blk) if parity else bytes(blk)
    out = b"\x01" + (bytes(hdr) if hdr else b"") + blk
    if crc is not None:
        c = crc16_kermit(blk) ^ (0 if crc == "good" else 1)
        out += struct.pack("<H", c) + b"\x7f"
    return out


def sbd_short_dl(payload, typ1=0x09):
    """0x76 DL header without packet header: a short (msgno 0) SBD"""
    return bytes([0x76, typ1]) + payload


def sbd_packet(payload, msgno, typ1, ul=False, prehdr=None, msgcnt=None, ul_skip=None):
    """0x76 header [+ pre-header carrying msgcnt (typ1 0x08)] [+ UL 0x50/0x51 skip] + 0x10 len msgno + payload"""
    out = bytes([0x76, typ1])
    if typ1 == 0x08:
        first = prehdr if prehdr is not None else 0x26
        n = 5 if first == 0x20 else 7
        ph = bytearray(n)
        ph[0] = first
        ph[3] = msgcnt
        out += bytes(ph)
    if ul_skip is not None:
        out += bytes([ul_skip, 0, 0])
    return out + bytes([0x10, len(payload), msgno]) + payload


def sbd_06_first(payload, msgcnt):
    """the 0x06 0x00 family's first packet: a 29-byte header (0x20 first, the packet count at 15), then the data"""
    h = bytearray(29)
    h[0] = 0x20
    h[15] = msgcnt
    return bytes([0x06, 0x00]) + bytes(h) + payload


def split_sbd(payload, n_pkts, ul=False):
    """one SBD message in n_pkts packets: the first carries the count (DL: the 0x08 pre-header, UL: the 0x06 0x00
    header), the others the 0x10 packet header with message numbers 2.."""
    step = -(-len(payload) // n_pkts)
    parts = [payload[i * step:(i + 1) * step] for i in range(n_pkts)]
    first = sbd_06_first(parts[0], n_pkts) if ul else sbd_packet(parts[0], 1, 0x08, prehdr=0x20, msgcnt=n_pkts)
    return [first] + [sbd_packet(p, k + 2, 0x0d if ul else 0x09) for k, p in enumerate(parts[1:])]


