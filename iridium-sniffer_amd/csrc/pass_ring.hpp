// pass_ring.hpp -- the result ring of a chunk pass whose figures the host reads later (input_stats.hpp, iq_moments.hpp,
// scrub.hpp): kChunkSlots blocks on the device with their pinned copies, used in turn.  A launch writes its slot's device
// block, the block is copied to the pinned one behind it, an event marks the copy; the host folds the pinned blocks into
// the pass's totals oldest first, when the figures are asked for, when a tag is settled or when the slot is needed again.
//
// PassRing is cache (it survives a reset), PassRingStream stream state (a reset assigns a fresh one after waiting for the
// streams: the launches in flight are dropped with it).  A pass derives its own two structs from them and adds its switch
// and its totals.
#pragma once
#include <deque>
#include "chunk_span.hpp"

namespace irdm {

// the launches whose blocks have not been folded yet, oldest first
struct PassRingStream {
    struct Entry {
        int slot;
        uint64_t meta;                  // the pass's own: the grid of a statistics launch, the stream position of a scrub
        size_t n;
        uint64_t tag;
    };
    std::deque<Entry> pending;
    uint64_t launches = 0;
    int last_slot = -1;                 // the slot of the launch enqueued last (-1: none since the stream began)
};

struct PassRing {
    hipStream_t stream = nullptr;       // the side stream (nullptr: the pass runs on the stream its chunk arrives on)
    hipEvent_t ev_in = nullptr;
    void *d_block[kChunkSlots] = {}, *h_block[kChunkSlots] = {};
    hipEvent_t ev[kChunkSlots] = {};

    bool allocated() const { return ev[0] != nullptr; }

    void free()
    {
        if (stream) (void)hipStreamSynchronize(stream);
        for (int i = 0; i < kChunkSlots; i++) {
            if (d_block[i]) (void)hipFree(d_block[i]);
            if (h_block[i]) (void)hipHostFree(h_block[i]);
            if (ev[i]) (void)hipEventDestroy(ev[i]);
        }
        if (ev_in) (void)hipEventDestroy(ev_in);
        if (stream) (void)hipStreamDestroy(stream);
        *this = PassRing{};
    }

    // the blocks, when the pass is first switched on (the device is current)
    int alloc(size_t block_bytes, bool side_stream)
    {
        if (allocated()) return 0;
        bool ok = true;
        if (side_stream) {
            ok = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess;
            ok = ok && hipEventCreateWithFlags(&ev_in, hipEventDisableTiming) == hipSuccess;
        }
        for (int i = 0; i < kChunkSlots; i++) {
            ok = ok && hipMalloc(&d_block[i], block_bytes) == hipSuccess;
            ok = ok && hipHostMalloc(&h_block[i], block_bytes, hipHostMallocDefault) == hipSuccess;
            ok = ok && hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) == hipSuccess;
        }
        if (!ok) {
            free();
            return -1;
        }
        return 0;
    }

    // the side stream goes on behind what `arrival` has been given so far (nullptr: the chunk is complete in memory)
    int follow(hipStream_t arrival)
    {
        if (!arrival) return 0;
        return hipEventRecord(ev_in, arrival) == hipSuccess && hipStreamWaitEvent(stream, ev_in, 0) == hipSuccess ? 0 : -1;
    }

    // s goes on behind the launch enqueued last: what s records or runs next may hand the chunk's memory back
    int lead(const PassRingStream &st, hipStream_t s)
    {
        return st.last_slot < 0 || hipStreamWaitEvent(s, ev[st.last_slot], 0) == hipSuccess ? 0 : -1;
    }

    // launches up to and including tag `upto` are waited for and folded, oldest first: fold(pinned block, entry)
    template <typename Fold>
    int settle(PassRingStream &st, uint64_t upto, Fold &&fold)
    {
        while (!st.pending.empty() && st.pending.front().tag <= upto) {
            const PassRingStream::Entry e = st.pending.front();
            if (hipEventSynchronize(ev[e.slot]) != hipSuccess) return -1;
            fold(static_cast<const void *>(h_block[e.slot]), e);
            st.pending.pop_front();
        }
        return 0;
    }

    // the slot of the next launch (-1: error); the launch that still holds it (kChunkSlots launches ago) is settled first
    template <typename Fold>
    int acquire(PassRingStream &st, Fold &&fold)
    {
        const int slot = (int)(st.launches % kChunkSlots);
        for (bool busy = true; busy;) {
            busy = false;
            for (const auto &e : st.pending) busy = busy || e.slot == slot;
            if (busy && settle(st, st.pending.front().tag, fold) != 0) return -1;
        }
        return slot;
    }

    // the launch into `slot` has been enqueued on s: the first `bytes` of its block follow it to the pinned copy
    int commit(PassRingStream &st, int slot, size_t bytes, hipStream_t s, uint64_t meta, size_t n, uint64_t tag)
    {
        if (hipMemcpyAsync(h_block[slot], d_block[slot], bytes, hipMemcpyDeviceToHost, s) != hipSuccess) return -1;
        if (hipEventRecord(ev[slot], s) != hipSuccess) return -1;
        st.pending.push_back(PassRingStream::Entry{ slot, meta, n, tag });
        st.launches++;
        st.last_slot = slot;
        return 0;
    }
};

}  // namespace irdm
