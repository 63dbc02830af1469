// record_queues.hpp -- the queues of finished records a stream leaves behind, one per record kind of the C-ABI: what a context
// holds between bursts_finish and the polls (StreamState::q, pipeline.hpp) and what a group keeps per chunk and merges in
// stream order (group.cpp).  A record kind added later is added HERE: append and counts are the only places that spell the
// queues out.  Needs the record types of include/irdm_hip.h only.
#pragma once
#include <deque>
#include <iterator>
#include <vector>
#include "../../include/irdm_hip.h"

struct RecordQueues {
    std::deque<irdm_burst_t> bursts;
    std::deque<irdm_frame_info_t> frames;
    std::deque<std::vector<float>> frame_samples;   // always one entry per frame record (empty without keep_frame_samples)
    std::deque<irdm_demod_t> demods;
    std::deque<irdm_demod_packed_t> packed;
    std::deque<irdm_ida_packed_t> ida_packed;       // option parsed_records: one per packed record
    std::deque<irdm_frame_packed_t> frame_packed;   // option frame_records: one per packed record
    std::deque<irdm_decoded_t> decoded;
    std::deque<irdm_ida_t> ida;

    // the records of `o` behind the ones held, queue by queue; `o` is left empty
    void append(RecordQueues &&o)
    {
        move_back(bursts, o.bursts);
        move_back(frames, o.frames);
        move_back(frame_samples, o.frame_samples);
        move_back(demods, o.demods);
        move_back(packed, o.packed);
        move_back(ida_packed, o.ida_packed);
        move_back(frame_packed, o.frame_packed);
        move_back(decoded, o.decoded);
        move_back(ida, o.ida);
    }

    // how many records each queue holds, in the fields of a chunk mark (ida_packed and frame_packed go with packed)
    irdm_chunk_mark_t counts() const
    {
        irdm_chunk_mark_t m;
        m.chunk = 0;
        m.n_bursts = (uint32_t)bursts.size();
        m.n_frames = (uint32_t)frames.size();
        m.n_demods = (uint32_t)demods.size();
        m.n_packed = (uint32_t)packed.size();
        m.n_decoded = (uint32_t)decoded.size();
        m.n_ida = (uint32_t)ida.size();
        return m;
    }

private:
    template <typename T>
    static void move_back(std::deque<T> &to, std::deque<T> &from)
    {
        if (to.empty()) to.swap(from);
        else to.insert(to.end(), std::make_move_iterator(from.begin()), std::make_move_iterator(from.end()));
        from.clear();
    }
};

// the mark of the records pushed between two counts() of one RecordQueues
inline irdm_chunk_mark_t mark_between(uint64_t chunk, const irdm_chunk_mark_t &before, const irdm_chunk_mark_t &after)
{
    irdm_chunk_mark_t m;
    m.chunk = chunk;
    m.n_bursts = after.n_bursts - before.n_bursts;
    m.n_frames = after.n_frames - before.n_frames;
    m.n_demods = after.n_demods - before.n_demods;
    m.n_packed = after.n_packed - before.n_packed;
    m.n_decoded = after.n_decoded - before.n_decoded;
    m.n_ida = after.n_ida - before.n_ida;
    return m;
}

// up to `max` records from the front of a queue: what every poll of the C-ABI does
template <typename T>
inline int drain(std::deque<T> &q, T *out, int max)
{
    int n = 0;
    while (n < max && !q.empty()) {
        out[n++] = q.front();
        q.pop_front();
    }
    return n;
}
