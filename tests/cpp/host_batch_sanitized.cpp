// The whole-batch calls of both pipelines as a stand-alone host program for -fsanitize=address,undefined: linked with api_unity.cpp
// compiled under -DMANTA_WAVE_EMU (as tests/emu/Makefile compiles it), so the block driver, the uploads, the staging and the compaction
// run as they are, on the lock-step wave emulator.  Per pipeline: six seeded loci as three blocks on two workers, the arenas-too-small
// exit, and the same call again on the pooled pipelines.  Host only; built and run by tests/test_batch_sanitized.py.
#include "../../include/manta_amd.h"

#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

static int failures = 0;
static void expect(const bool ok, const std::string& what)
{
  if (!ok) {
    std::fprintf(stderr, "host_batch_sanitized: FAILED: %s\n", what.c_str());
    ++failures;
  }
}

using Seq = std::vector<uint8_t>;
static Seq randomSeq(std::mt19937_64& rng, const size_t n)
{
  Seq s(n);
  for (uint8_t& c : s) c = uint8_t("ACGT"[rng() & 3]);
  return s;
}

/// read piles of a batch: `nReads` reads of `readLen` per locus, each across position `j` of the locus' haplotype by >= `margin` bases
struct Piles {
  Seq                   bases;
  std::vector<uint64_t> readOff{0};
  std::vector<uint32_t> begin{0};
  void add(std::mt19937_64& rng, const Seq& hap, const size_t j, const unsigned nReads, const size_t readLen, const size_t margin)
  {
    const size_t lo = j + margin > readLen ? j + margin - readLen : 0, hi = std::min(hap.size() - readLen, j - margin);
    for (unsigned r = 0; r < nReads; ++r) {
      const size_t s = lo + rng() % (hi - lo + 1);
      bases.insert(bases.end(), hap.begin() + s, hap.begin() + s + readLen);
      readOff.push_back(bases.size());
    }
    begin.push_back(uint32_t(readOff.size() - 1));
  }
};

/// the caller's side of a whole-batch call
template <typename Alignment>
struct Output {
  std::vector<manta_asm_locus_result_t> loci;
  std::vector<manta_asm_contig_t>       contigs;
  std::vector<Alignment>                aligns;
  Seq                                   seq;
  std::vector<uint64_t>                 bits;
  std::vector<uint32_t>                 cig;
  uint64_t                              seqUsed = 0, bitsUsed = 0, cigUsed = 0;
  manta_batch_stats_t                   stats{};
  Output(const uint32_t n, const size_t seqCap, const size_t bitsCap, const size_t cigCap)
      : loci(n), contigs(n * 10 + 1), aligns(n * 10 + 1), seq(seqCap), bits(bitsCap), cig(cigCap) {}
  /// every locus assembled, every contig and CIGAR inside what the call says it used; the contig texts, locus by locus
  std::vector<std::string> texts(const char* who)
  {
    std::vector<std::string> out;
    uint64_t                 nAligned = 0;
    for (size_t l = 0; l < loci.size(); ++l) {
      expect(loci[l].status == MANTA_OK, std::string(who) + ": locus status");
      std::string t;
      for (uint32_t c = 0; loci[l].status == MANTA_OK && c < loci[l].n_contigs; ++c) {
        const manta_asm_contig_t& k(contigs[loci[l].first_contig + c]);
        expect(k.seq_off + k.seq_len <= seqUsed, std::string(who) + ": contig inside the text arena");
        t += std::string(reinterpret_cast<const char*>(seq.data()) + k.seq_off, k.seq_len) + "\n";
        const manta_align_result_t& a(aligns[loci[l].first_contig + c].align);
        if (a.status != MANTA_OK) continue;
        expect(a.cigar1_off + a.cigar1_len <= cigUsed && a.cigar2_off + a.cigar2_len <= cigUsed, std::string(who) + ": CIGAR inside the arena");
        ++nAligned;
      }
      out.push_back(t);
    }
    expect(nAligned > 0, std::string(who) + ": at least one contig aligned");
    expect(stats.n_blocks == 3 && stats.n_workers == 2, std::string(who) + ": three blocks on two workers");
    return out;
  }
};

static const uint32_t            kLoci  = 6;
static const manta_batch_plan_t  kPlan  = {2, 2, 0, 0, nullptr};
static const size_t              kCaps[3] = {size_t(1) << 20, size_t(1) << 16, size_t(1) << 18};

/// full arenas, then a text arena of 16 bytes (MANTA_E_CAPACITY under the call's own name), then full arenas again on the same pipelines
template <typename Alignment, typename Call>
static void threeCalls(manta_ctx_t* ctx, const char* who, Call call)
{
  Output<Alignment> first(kLoci, kCaps[0], kCaps[1], kCaps[2]);
  expect(call(first) == MANTA_OK, std::string(who) + ": " + manta_last_error(ctx));
  const std::vector<std::string> want = first.texts(who);
  Output<Alignment> tiny(kLoci, 16, kCaps[1], kCaps[2]);
  expect(call(tiny) == MANTA_E_CAPACITY, std::string(who) + ": a 16-byte text arena is MANTA_E_CAPACITY");
  expect(std::string(manta_last_error(ctx)) == std::string(who) + ": caller arenas too small", std::string(who) + ": the message of the capacity exit");
  Output<Alignment> again(kLoci, kCaps[0], kCaps[1], kCaps[2]);
  expect(call(again) == MANTA_OK, std::string(who) + " after the failed call: " + manta_last_error(ctx));
  expect(again.texts(who) == want, std::string(who) + ": the call after the failed one gives the same contigs");
}

int main()
{
  manta_ctx_t* ctx = nullptr;
  if (manta_ctx_create(0, &ctx) != MANTA_OK) {
    std::fprintf(stderr, "host_batch_sanitized: no context: %s\n", manta_last_error(nullptr));
    return 1;
  }
  {  // small-SV: a deletion of 10..60 bases in the middle of a 500-base window, 20 reads of 80
    std::mt19937_64       rng(4242);
    Piles                 p;
    Seq                   refs;
    std::vector<uint64_t> refOff{0};
    for (uint32_t l = 0; l < kLoci; ++l) {
      const Seq    ref = randomSeq(rng, 500);
      const size_t del = 10 + rng() % 51;
      Seq          hap(ref.begin(), ref.begin() + 250);
      hap.insert(hap.end(), ref.begin() + 250 + del, ref.end());
      p.add(rng, hap, 250, 20, 80, 10);
      refs.insert(refs.end(), ref.begin(), ref.end());
      refOff.push_back(refs.size());
    }
    const std::vector<manta_ref_cuts_t> cuts(kLoci, manta_ref_cuts_t{40, 40, 200, 200});
    const manta_asm_options_t           opt    = {25, 45, 5, 15, 1, 2, 3, 2, 10};
    const manta_align_scores_t          scores = {2, -8, -24, -1, -1, 0};
    threeCalls<manta_smallsv_alignment_t>(ctx, "manta_smallsv_batch", [&](Output<manta_smallsv_alignment_t>& o) {
      return manta_smallsv_batch(ctx, &opt, &scores, -100, kLoci, p.bases.data(), p.readOff.data(), p.begin.data(), refs.data(), refOff.data(), cuts.data(),
                                 nullptr, nullptr, o.loci.data(), o.contigs.data(), o.aligns.data(), o.contigs.size(), o.seq.data(), o.seq.size(), &o.seqUsed,
                                 o.bits.data(), o.bits.size(), &o.bitsUsed, o.cig.data(), o.cig.size(), &o.cigUsed, &kPlan, &o.stats);
    });
  }
  {  // spanning: two 320-base windows fused near their middles with up to 20 inserted bases, 24 reads of 70 across the junction
    std::mt19937_64       rng(300);
    Piles                 p;
    Seq                   refs1, refs2;
    std::vector<uint64_t> ref1Off{0}, ref2Off{0};
    for (uint32_t l = 0; l < kLoci; ++l) {
      const Seq    ref1 = randomSeq(rng, 320), ref2 = randomSeq(rng, 320), ins = randomSeq(rng, rng() % 21);
      const size_t j = 140 + rng() % 41, k = 140 + rng() % 41;
      Seq          hap(ref1.begin(), ref1.begin() + j);
      hap.insert(hap.end(), ins.begin(), ins.end());
      hap.insert(hap.end(), ref2.begin() + k, ref2.end());
      p.add(rng, hap, j, 24, 70, 20);
      refs1.insert(refs1.end(), ref1.begin(), ref1.end());
      refs2.insert(refs2.end(), ref2.begin(), ref2.end());
      ref1Off.push_back(refs1.size());
      ref2Off.push_back(refs2.size());
    }
    const std::vector<manta_jump_cuts_t> cuts(kLoci, manta_jump_cuts_t{30, 30, 30, 30});
    const manta_asm_options_t            opt    = {25, 45, 5, 40, 1, 2, 3, 2, 10};
    const manta_align_scores_t           scores = {2, -8, -12, -1, -1, 0};
    threeCalls<manta_spanning_alignment_t>(ctx, "manta_spanning_batch", [&](Output<manta_spanning_alignment_t>& o) {
      return manta_spanning_batch(ctx, &opt, &scores, -100, kLoci, p.bases.data(), p.readOff.data(), p.begin.data(), refs1.data(), ref1Off.data(), refs2.data(),
                                  ref2Off.data(), cuts.data(), nullptr, nullptr, o.loci.data(), o.contigs.data(), o.aligns.data(), o.contigs.size(),
                                  o.seq.data(), o.seq.size(), &o.seqUsed, o.bits.data(), o.bits.size(), &o.bitsUsed, o.cig.data(), o.cig.size(), &o.cigUsed,
                                  &kPlan, &o.stats);
    });
  }
  manta_ctx_destroy(ctx);
  if (!failures) std::printf("host_batch_sanitized ok\n");
  return failures ? 1 : 0;
}
