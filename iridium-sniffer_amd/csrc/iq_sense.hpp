// iq_sense.hpp -- option "iq_sense" (irdm_iq_vote_t / irdm_iq_sense_t, include/irdm_hip.h), host side: the votes of a
// stream's frames and the verdict over them.  The kernel is iq_sense_kernel of bitlayer.hip (launch_iq_sense, kernels.hpp),
// launched by chain.cpp behind the demodulator and by state.cpp (irdm_iq_sense_batch).
#pragma once
#include <string.h>
#include <deque>
#include "types.hpp"
#include "../../include/irdm_hip.h"

namespace irdm {

// Stream state: the per-frame records until they are polled, and the counts the summary is read from
struct IqSenseStream {
    std::deque<irdm_iq_vote_t> q;
    uint64_t frames = 0, rec = 0, exch = 0, both = 0;
    uint64_t k_rec[3] = { 0, 0, 0 }, k_exch[3] = { 0, 0, 0 }, k_both[3] = { 0, 0, 0 };
};

static inline irdm_iq_vote_t iq_vote_of(uint64_t id, const SenseRec &r)
{
    irdm_iq_vote_t o;
    o.id = id;
    o.recorded = r.recorded;
    o.exchanged = r.exchanged;
    o.pad = 0;
    o.n_bits = r.n_bits;
    return o;
}

// one frame whose unique word passed
static inline void iq_sense_fold(IqSenseStream &st, uint64_t id, const SenseRec &r)
{
    st.q.push_back(iq_vote_of(id, r));
    st.frames++;
    if (!r.recorded && !r.exchanged) return;
    uint64_t &n = r.recorded && r.exchanged ? st.both : (r.recorded ? st.rec : st.exch);
    uint64_t *k = r.recorded && r.exchanged ? st.k_both : (r.recorded ? st.k_rec : st.k_exch);
    n++;
    for (int j = 0; j < 3; j++)
        if ((r.recorded | r.exchanged) >> j & 1) k[j]++;
}

static inline void iq_sense_result(const IqSenseStream &st, irdm_iq_sense_t *out)
{
    memset(out, 0, sizeof(*out));
    out->frames = st.frames;
    out->votes_recorded = st.rec;
    out->votes_exchanged = st.exch;
    out->votes_both = st.both;
    for (int j = 0; j < 3; j++) {
        out->kind_recorded[j] = st.k_rec[j];
        out->kind_exchanged[j] = st.k_exch[j];
        out->kind_both[j] = st.k_both[j];
    }
    const uint64_t d = st.rec + st.exch;
    out->verdict = d < 5 ? IRDM_IQ_TOO_FEW
                         : (st.rec * 10 >= 9 * d ? IRDM_IQ_AS_RECORDED : (st.exch * 10 >= 9 * d ? IRDM_IQ_EXCHANGED : IRDM_IQ_MIXED));
}

}  // namespace irdm
