// The staging pool of the calls that prepare their segments on the host
// (StagePool, ec_internal.hpp): segment repair, and the sized share-set, encode,
// hash and AES-GCM calls, each with a pool of its own on the context.
#include "ec_internal.hpp"

namespace uplink_ec {
namespace capi {

// A block of the pool with room for h_need pinned and d_need device bytes whose
// previous pass has finished on the GPU, or a new one (sized in powers of two,
// its device half from the pool's minimum).  nullptr: no memory.  The limit on
// blocks in flight counts the blocks large enough for this pass, not all blocks
// of the pool, so that a pool full of small blocks from small batches does not
// make a call with a larger pass wait for the few blocks that fit it.
StageBlock *block_acquire(StagePool &P, size_t h_need, size_t d_need) {
    StageBlock *b = nullptr, *oldest = nullptr;
    {
        std::lock_guard<std::mutex> g(P.mu);
        size_t fit = 0;
        for (auto &x : P.blocks) {
            if (x->h_cap < h_need || x->d_cap < d_need) continue;
            fit++;
            if (x->busy) continue;
            if (!oldest) oldest = x.get();  // (blocks are reused in the order they were made)
            if (x->idle()) {
                b = x.get();
                break;
            }
        }
        if (!b && fit >= StagePool::kMaxBlocks) b = oldest;  // waited for below
        if (!b) {
            auto x = std::make_unique<StageBlock>();
            x->h_cap = pow2_at_least(h_need, 64u << 10);
            x->d_cap = pow2_at_least(d_need, P.d_min);
            if (hipHostMalloc((void **)&x->h, x->h_cap, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess ||
                hipMalloc((void **)&x->d, x->d_cap) != hipSuccess ||
                hipEventCreateWithFlags(&x->ev, hipEventDisableTiming) != hipSuccess)
                return nullptr;  // (its destructor frees what it got)
            P.blocks.push_back(std::move(x));
            b = P.blocks.back().get();
        }
        b->busy = true;
    }
    if (b->queued && hipEventSynchronize(b->ev) != hipSuccess) {
        std::lock_guard<std::mutex> g(P.mu);
        b->busy = false;
        return nullptr;
    }
    b->queued = false;
    return b;
}

// Hand the block back; `launched`: something that reads it was queued on s.
void block_release(StagePool &P, StageBlock *b, bool launched, hipStream_t s) {
    // (an event that cannot be recorded leaves the block to a wait for the stream)
    if (launched && hipEventRecord(b->ev, s) != hipSuccess) (void)hipStreamSynchronize(s);
    std::lock_guard<std::mutex> g(P.mu);
    b->queued = launched;
    b->busy = false;
}

bool stream_is_capturing(hipStream_t s) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone;
}

}  // namespace capi
}  // namespace uplink_ec
