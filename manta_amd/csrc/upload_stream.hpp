// The chunk protocol of a streamed upload (whole-batch calls): the read bases -- or the packed piles -- arrive chunk by chunk on a copy
// stream while the assembler, launched right away on the pipeline's stream, works through the loci whose chunk has landed
// (AsmParams::upload_*).  Behind every chunk's copies the copy stream bumps a counter word the kernels poll.  Included by
// api_internal.hpp behind DevBuf / PinnedBuf; AsmStage keeps one ChunkStream and does the allocations and the small arrays itself.
#pragma once

namespace manta_host {

struct ChunkStream {
  static const uint32_t kStreamChunks = 32;  ///< at most (array sizes)
  /// chunks a streamed upload is cut into: the kernel cannot start on a chunk before all of it has landed, so the last chunk's loci are the
  /// tail behind the DMA (1 / chunks of the kernel's work); every chunk costs a copy command and a counter write
  static uint32_t streamChunks()
  {
    static const uint32_t n = std::getenv("MANTA_AMD_STREAM_CHUNKS") ? uint32_t(std::max(1, std::min(int(kStreamChunks), std::atoi(std::getenv("MANTA_AMD_STREAM_CHUNKS"))))) : 16u;
    return n;
  }
  /// Workgroup slots a streamed launch of the LDS pipeline leaves free for the runtime's copy kernels and stream writes (launch()): two
  /// per XCD.  Workgroups are dealt to the eight XCDs round-robin and stay there, so what matters is a free slot in EVERY XCD: with 4 free
  /// slots (one in each of four XCDs) a 16 384-locus config-5 block starved until the kernel's time-out, with 16 it runs -- and the quarter
  /// of the CUs that rounds 4-5 left free cost graph_kernel 12 % and graph_big_kernel 25 % of their workgroups for the whole launch
  /// (metric step 8.83 -> 8.60 ms, 16 384 config-5 loci 268 -> 257 ms).  MANTA_AMD_STREAM_FREE_WGS overrides (rounded up to whole eights).
  static int streamFreeSlots(const int cuCount)
  {
    static const int forced = std::getenv("MANTA_AMD_STREAM_FREE_WGS") ? std::max(1, std::atoi(std::getenv("MANTA_AMD_STREAM_FREE_WGS"))) : 0;
    const int        want   = forced ? forced : 16;
    return std::max(1, std::min(((want + 7) / 8) * 8, cuCount / 4));  // (never more than the quarter of the CUs of rounds 4-5: small devices, the emulator)
  }

  /// the chunks of a batch of n loci: whole loci, in locus order, `chunkLoci` each (the last one may be short)
  struct Chunking {
    uint32_t chunkLoci, nChunks;
    explicit Chunking(const uint32_t n) : chunkLoci(std::max<uint32_t>(1, (n + streamChunks() - 1) / streamChunks())), nChunks((n + chunkLoci - 1) / chunkLoci) {}
  };
  /// where the chunks of streamed read bases lie on the host and on the device
  struct StreamLayout : Chunking {
    using Chunking::Chunking;
    uint64_t cursor = 0;  ///< bytes of the device arena the chunks take (per-chunk padding included)
    uint64_t hostBegin[kStreamChunks + 1] = {0}, devBegin[kStreamChunks + 1] = {0};
    uint32_t shift[1 + kStreamChunks] = {0};  ///< AsmParams::chunk_shift: device - host offset of chunk c at [1 + c]
    bool     monotone = true;
  };
  static StreamLayout streamLayout(const uint32_t n, const uint64_t* read_off, const uint32_t* locus_read_begin)
  {
    StreamLayout L(n);
    for (uint32_t c = 0; c < L.nChunks; ++c) {
      const uint32_t l0 = c * L.chunkLoci, l1 = std::min(n, l0 + L.chunkLoci);
      L.hostBegin[c]    = read_off[locus_read_begin[l0]];
      const uint64_t end = read_off[locus_read_begin[l1]];
      if (end < L.hostBegin[c]) L.monotone = false;
      const uint64_t len = end - L.hostBegin[c];
      L.devBegin[c]      = L.cursor;
      // (modulo 2^32: the kernel adds it in 32-bit arithmetic to a 64-bit offset; device offsets only grow by the padding, so the shifts stay small)
      L.shift[1 + c]     = uint32_t(L.devBegin[c] - L.hostBegin[c]);
      L.cursor           = (L.cursor + len + 64 + 255) & ~uint64_t(255);
    }
    L.hostBegin[L.nChunks] = read_off[locus_read_begin[n]];
    return L;
  }

  /// waits until the copy stream is empty (a failed call must not leave DMA reads of the caller's buffers queued)
  static void drain(rt::Stream* copyStream) noexcept
  {
    try {
      rt::ScopedStream onCopy(*copyStream);
      rt::sync();
    } catch (...) {
    }
  }

  /// What AsmStage::startStream() hands to the uploadStreamed() of the same call: the chunks of THIS batch are on the copy stream.  Made
  /// before the first of them is queued; dropped before uploadStreamed() has taken it over -- an exception, an early return of the
  /// caller -- it drains the copy stream.
  struct Ticket {
    StreamLayout layout;
    uint32_t     nLoci;
    std::unique_ptr<rt::Stream, decltype(&drain)> copy;  ///< {&copyStream, &drain}: drained when the ticket goes before consume()
    void consume() { (void)copy.release(); }  ///< the upload stands: from here on a failing run drains the copy stream (drainCopyStream)
  };

  enum class Mode { None, Bases, Piles };
  Mode      mode      = Mode::None;  ///< of the batch uploaded last
  uint32_t  chunkLoci = 0;
  rt::Event evPreSmall;  ///< startStream(): read offsets and locus table are on the device (ahead of the chunks on the copy stream)

  ~ChunkStream() { if (dChunksDone) rt::dfree(dChunksDone); }
  bool active() const { return mode != Mode::None; }
  void off() { mode = Mode::None; }  ///< a blocking upload

  /// the batch's chunk size and shifts, on the current stream.  Bases: StreamLayout::shift; piles: three 64-bit shifts per chunk
  void begin(const Mode m, const Chunking& k, const void* shifts)
  {
    const size_t bytes = m == Mode::Bases ? sizeof(uint32_t) * (1 + kStreamChunks) : sizeof(uint64_t) * 3 * kStreamChunks;
    rt::h2d((m == Mode::Bases ? bShift : bPlShift).need(bytes), shifts, bytes);
    chunkLoci = k.chunkLoci;
    mode      = m;
  }
  /// the counter back to zero, written on the current stream; the caller syncs it before it queues chunks
  void reset(rt::Stream& copyStream)
  {
    if (!dChunksDone) dChunksDone = static_cast<uint32_t*>(rt::dmallocFine(64));
    uint32_t* ids = pChunkIds.as<uint32_t>(kStreamChunks + 1);
    for (uint32_t c = 0; c <= kStreamChunks; ++c) ids[c] = c;
    {  // a call that failed half way may have left counter bumps queued on the copy stream: none may land after the reset
      rt::ScopedStream onCopy(copyStream);
      rt::sync();
    }
    rt::h2d(dChunksDone, ids, sizeof(uint32_t));  // = 0
  }
  /// copyChunk(c) issues chunk c's copies; each chunk is followed by a stream-ordered 32-bit write of the counter (command processor; a
  /// 4-byte copy if the runtime refuses): the counter says c+1 only after chunk c is in HBM.  Nothing here needs a workgroup slot -- the
  /// persistent assembler, or another process' kernels, may own every one of them.
  template <typename F>
  void queue(const uint32_t nChunks, rt::Stream& copyStream, F copyChunk)
  {
    const uint32_t*  ids = pChunkIds.as<uint32_t>(kStreamChunks + 1);
    rt::ScopedStream onCopy(copyStream);
    for (uint32_t c = 0; c < nChunks; ++c) {
      copyChunk(c);
      if (!rt::streamWrite32(dChunksDone, c + 1)) rt::h2d(dChunksDone, ids + c + 1, sizeof(uint32_t));
    }
  }
  void fill(manta_dev::AsmParams& P) const
  {
    P.upload_chunks_done = active() ? dChunksDone : nullptr;
    P.chunk_shift        = mode == Mode::Bases ? static_cast<const uint32_t*>(bShift.p) + 1 : nullptr;
    P.pl_chunk_shift     = mode == Mode::Piles ? static_cast<const uint64_t*>(bPlShift.p) : nullptr;
    P.chunk_loci         = active() ? chunkLoci : 0;
  }

 private:
  DevBuf    bShift, bPlShift;
  uint32_t* dChunksDone = nullptr;  // fine-grained device word the copy stream bumps after every chunk
  PinnedBuf pChunkIds;              // the values 0..kStreamChunks it is bumped to (DMA sources)
};

}  // namespace manta_host
