// host_chain.hpp -- the corrections of a host feed, strung together once for both objects that have them: a context
// (irdm_feed_host, irdm_prime_*; feed.cpp) and a front end (irdm_frontend_feed_host, irdm_frontend_prime_host; frontend.cpp).
//
// A chunk is corrected on the feed's stream between its copy to the device and its first reader, in this order:
//   1. the exchange (iq_swap.hpp) in the wire format, where the bytes landed;
//   2. the DC tracker (dc_block.hpp) from there into the chunk's own place as cf32;
//   3. the balance (iq_balance.hpp) likewise -- behind the DC tracker on cf32 in place, whatever wire format it was given;
//   4. the scrub (scrub.hpp) in place, for a cf32 object alone.
// The wire format -- what the caller's bytes are -- is the DC tracker's if that is on, else the balance's if that is on,
// else the object's own.  Other than cf32 it lands in the one wire staging buffer (one is enough: the next chunk's copy lies
// behind this chunk's launches on the same stream); cf32 lands in the chunk's own place and is corrected there.
// A device feed takes none of this: with a correction on it is refused, but for the host feed's own (`inner`).
#pragma once
#include <stdio.h>
#include "iq_swap.hpp"
#include "dc_block.hpp"
#include "iq_balance.hpp"
#include "scrub.hpp"

namespace irdm {

// Configuration (the switches and what goes with them: they survive a reset) and cache (the scrub's blocks, the DC tracker's
// rings, the wire staging buffer).
struct HostChain {
    int swap_iq = 0;            // option "swap_iq" / irdm_frontend_swap_iq
    ScrubPass scrub;            // options "scrub", "scrub_limit_log2" / irdm_frontend_scrub
    IqBalance bal;              // irdm_iq_balance / irdm_frontend_iq_balance
    DcBlock dc;                 // irdm_dc_block / irdm_frontend_dc_block
    void *d_wire = nullptr;     // a chunk in a wire format other than cf32
    size_t wire_bytes = 0;
    bool inner = false;         // the host feed's own device feed is under way: the only one the corrections allow
};
// Stream state: the scrub's totals and launches in flight, the DC tracker's position.  A reset assigns a fresh one.
struct HostChainStream {
    ScrubStream scrub;
    DcStream dc;
};

// the format of the bytes a host feed takes
static inline int hc_wire_fmt(const HostChain &c, int own_fmt) { return c.dc.on ? c.dc.wire_fmt : (c.bal.on ? c.bal.wire_fmt : own_fmt); }
// ... and whether they land in the wire staging buffer (the DC tracker and the balance are a cf32 object's)
static inline bool hc_wired(const HostChain &c) { return (c.dc.on || c.bal.on) && hc_wire_fmt(c, IRDM_FMT_CF32) != IRDM_FMT_CF32; }
// where the copy of a chunk must put the bytes: the wire staging buffer when one is in use, else the chunk's own place
static inline void *hc_landing(const HostChain &c, void *chunk_place) { return hc_wired(c) ? c.d_wire : chunk_place; }

// *d_buf holds at least `need` bytes: grown behind `stream`, whose launches may read the old one.  0, or -1 with nothing held.
static inline int hc_grow(void **d_buf, size_t *have, size_t need, hipStream_t stream)
{
    if (need <= *have) return 0;
    if (hipStreamSynchronize(stream) != hipSuccess) return -1;
    if (*d_buf) (void)hipFree(*d_buf);
    *d_buf = nullptr;
    *have = 0;
    if (hipMalloc(d_buf, need) != hipSuccess) return -1;
    *have = need;
    return 0;
}

// the wire staging buffer takes n_samples of the wire format in effect (nothing to do for cf32)
static inline int hc_reserve(HostChain &c, size_t n_samples, hipStream_t stream)
{
    return hc_grow(&c.d_wire, &c.wire_bytes, hc_wired(c) ? n_samples * (size_t)fmt_bytes(hc_wire_fmt(c, IRDM_FMT_CF32)) : 0, stream);
}

// The n samples that lie at `land` (hc_landing of d_iq) in the wire format, corrected into d_iq, the chunk's own place, on
// `stream`.  scrub_base: the stream position the scrub counts the chunk from; figures false: it counts nothing (a priming
// prefix).  0, or -1: a launch failed.
static inline int hc_apply(HostChain &c, HostChainStream &st, int own_fmt, void *d_iq, void *land, size_t n, uint64_t scrub_base,
                           bool figures, hipStream_t stream)
{
    if (c.swap_iq && launch_iq_swap(hc_wire_fmt(c, own_fmt), land, n, stream) != 0) return -1;
    if (c.dc.on && dc_feed(c.dc, st.dc, d_iq, land, n, stream) != 0) return -1;
    if (c.bal.on && launch_iq_balance(c.dc.on ? IRDM_FMT_CF32 : c.bal.wire_fmt, d_iq, c.dc.on ? d_iq : land, n, c.bal.alpha, c.bal.beta,
                                      stream) != 0)
        return -1;
    if (!c.scrub.on || own_fmt != IRDM_FMT_CF32) return 0;
    return figures ? scrub_enqueue(c.scrub, st.scrub, d_iq, n, scrub_base, stream) : scrub_plain(d_iq, n, c.scrub.limit_log2, stream);
}

// A device feed of a buffer the caller owns while a correction is on: true, with the remedy on stderr.  owner: 0 a context,
// 1 a front end.
static inline bool hc_refuses(const HostChain &c, int owner)
{
    static const struct {
        const char *name[2], *does, *remedy, *with;
    } rows[4] = { { { "option swap_iq", "irdm_frontend_swap_iq" }, "exchanges", "exchange", "irdm_swap_iq_device" },
                  { { "option scrub", "irdm_frontend_scrub" }, "cleans", "scrub", "irdm_scrub_device" },
                  { { "irdm_iq_balance", "irdm_frontend_iq_balance" }, "corrects", "correct", "irdm_iq_balance_device" },
                  { { "irdm_dc_block", "irdm_frontend_dc_block" }, "corrects", "correct", "irdm_dc_block_device" } };
    const int on[4] = { c.swap_iq, c.scrub.on, c.bal.on, c.dc.on };
    for (int i = 0; i < 4 && !c.inner; i++) {
        if (!on[i]) continue;
        fprintf(stderr, "irdm_hip: %s%s %s the chunks of %s only: a device feed takes the caller's buffer as it is -- %s it with %s first\n",
                owner ? "front end: " : "", rows[i].name[owner], rows[i].does, owner ? "irdm_frontend_feed_host" : "irdm_feed_host",
                rows[i].remedy, rows[i].with);
        return true;
    }
    return false;
}

static inline void hc_free(HostChain &c)
{
    c.scrub.free();
    c.dc.DcRings::free();
    if (c.d_wire) (void)hipFree(c.d_wire);
    c.d_wire = nullptr;
    c.wire_bytes = 0;
}

}  // namespace irdm
