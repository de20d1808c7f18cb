// The small-SV pipeline's work per contig (SVCandidateAssemblyRefiner::getSmallSVAssembly,
// applications/GenerateSVCandidates/SVCandidateAssemblyRefiner.cpp:1984-2038): 10-mer reference trim and alignment task set-up.
// ONE copy for its two callers: the epilogue of the LDS contig kernels (asm_contig.hpp: the wave that emitted a locus' contigs
// schedules them at once, in the locus' own LDS share) and smallsv_schedule_kernel (pipeline_kernels.hpp: every locus the epilogue
// did not take).
//   The reference's trim is byte-generic: a std::set<std::string> of the contig's 10-mers, looked up with substrings of the window.  So
// is this one, in two forms of one table.  A contig of A, C, G and T alone -- every contig of the LDS contig kernels, which emit their
// text from 2-bit codes and hand a pile with any other byte to the general path -- keys the table by the 10-mer's 20-bit code; a window
// 10-mer with any other byte cannot be in it.  A contig that holds any other byte (a seed word of assemble_generic_kernel: lower case,
// '=', an IUPAC letter, a byte >= 0x80) keys it by a hash of the 10 bytes, stores the 10-mer's position and compares the bytes on a
// hit.  ('N' counts as such a byte here: the reference's set holds strings, and a contig 10-mer with an 'N' matches the same window
// text.)  That form exists in scheduleContig<true> alone, smallsv_schedule_kernel's instance: the epilogue's scheduleContig<false> is
// the 2-bit form and nothing else, and no locus with such a contig ever reaches it.
#pragma once
#include "align_kernels.hpp"
#include "assemble_kernels.hpp"

namespace manta_dev {

static const int      SMALLSV_MER       = 10;    // SVCandidateAssemblyRefiner.cpp:1986
static const unsigned SCHED_TABLE_BYTES = 4096;  // per wavefront: 10-mer table of contigs up to 512 bp lives in LDS
static const unsigned SCHED_SEQ_BYTES   = 6144;  // ... and so do the contig and the reference window (staged with wide loads: the scans
                                                 // below read a byte per lane and 55 positions per round trip otherwise)
static const unsigned SCHED_LDS_BYTES   = SCHED_TABLE_BYTES + SCHED_SEQ_BYTES + 1024;  // (+ the pending bucket entries) 11 KB per wavefront: 12-14 waves per CU

struct SmallSvCuts {
  int32_t leadingCut, trailingCut, maxLeadingCut, maxTrailingCut;  // :1912-1915
};

struct SmallSvTaskInfo {
  int32_t status;  // 0 ok; else MANTA-level failure of the trim (contig shorter than a 10-mer, empty window)
  int32_t adj_leading_cut, adj_trailing_cut;
  int32_t bucket;  // index into the E set, -1 if not scheduled
};

struct ScheduleParams {
  // assembler outputs (device)
  const AsmLocusOut*  loci;
  const AsmContigOut* contigs;
  const uint8_t*      seq_arena;
  uint32_t            n_loci;
  uint32_t            max_assembly_count;
  // references
  const uint8_t*     refs;
  const uint64_t*    ref_off;  // n_loci + 1
  const SmallSvCuts* cuts;     // n_loci
  // outputs
  AlignTaskDev*    tasks;  // n_loci * max_assembly_count
  SmallSvTaskInfo* info;   // same
  uint32_t*        bucket_ids;     // n_buckets * (n_loci * max_assembly_count)
  uint32_t*        bucket_count;   // n_buckets
  uint32_t*        bucket_maxref;  // n_buckets
  unsigned long long* cigar_used;  // bump allocator (u32 units)
  uint64_t         cigar_cap;
  uint32_t*        counter;
  // per-workgroup 10-mer table
  uint32_t* table_ws;
  uint32_t  table_cap;  // power of two, >= 2 * longest contig
  // E set: columns per lane of bucket b, a byte each (schedE / schedPackE; shifts, not an indexed array: the contig kernels copied one to scratch)
  uint64_t e_pack[2];
  uint32_t n_e;
  uint32_t chunk;  // loci per work-queue pop (smallsv_schedule_kernel)
  // the contig kernels' epilogue (nullptr: none -- every caller but the small-SV pipeline, and that one with MANTA_AMD_NO_FUSED_SCHEDULE)
  uint8_t*            marks;     // n_loci: 1 = scheduled by the wave that emitted the locus; smallsv_schedule_kernel skips it
  unsigned long long* n_marked;  // loci so marked
};

WV_DEV unsigned merCode(const uint8_t* p, bool& valid)
{
  unsigned code = 0;
  valid         = true;
  for (int i = 0; i < SMALLSV_MER; ++i) {
    const unsigned c = baseCode(p[i]);
    if (c > 3) valid = false;
    code = (code << 2) | (c & 3u);
  }
  return code;
}

/// 10-mer codes of 55 consecutive positions with ONE byte load per lane: lane l loads base p0+l, then the codes of
/// bases l..l+9 are assembled by doubling with four lane shuffles (2, 4, 8, 10 bases).  Lane l (<= 54) returns the
/// code of the 10-mer starting at p0+l; `valid` is false if the 10-mer leaves [0,len) or holds a non-ACGT base.
/// All 64 lanes must call.
static const int MER_BATCH = 55;
/// the lane's base code (0..3, 4 = not ACGT / outside the sequence) for batch start p0: the only memory access of a batch
WV_DEV unsigned merLoadBase(const uint8_t* seq, const int len, const int p0)
{
  const int pos = p0 + wv::lane();
  return (pos >= 0 && pos < len) ? baseCode(seq[pos]) : 4u;
}
/// 10-mer codes of the batch from the per-lane base codes
WV_DEV unsigned merCodesFromBase(const unsigned c, bool& valid)
{
  const int      l   = wv::lane();
  unsigned bad = (c > 3) ? 1u : 0u;
  unsigned w1  = c & 3u;
  const unsigned w2 = (w1 << 2) | wv::shfl(w1, (l + 1) & 63);
  const unsigned b2 = bad | wv::shfl(bad, (l + 1) & 63);
  const unsigned w4 = (w2 << 4) | wv::shfl(w2, (l + 2) & 63);
  const unsigned b4 = b2 | wv::shfl(b2, (l + 2) & 63);
  const unsigned w8 = (w4 << 8) | wv::shfl(w4, (l + 4) & 63);
  const unsigned b8 = b4 | wv::shfl(b4, (l + 4) & 63);
  const unsigned w10 = (w8 << 4) | wv::shfl(w2, (l + 8) & 63);
  const unsigned b10 = b8 | wv::shfl(b2, (l + 8) & 63);
  valid = (l < MER_BATCH) && (b10 == 0);
  return w10;
}
WV_DEV unsigned merCodes55(const uint8_t* seq, const int len, const int p0, bool& valid)
{
  return merCodesFromBase(merLoadBase(seq, len, p0), valid);
}

WV_DEV bool merLookup(const uint32_t* table, const unsigned mask, const unsigned code)
{
  unsigned s = (code * 2654435761u) & mask;
  while (true) {
    const uint32_t v = table[s];
    if (v == 0) return false;
    if (v == code + 1) return true;
    s = (s + 1) & mask;
  }
}

/// the byte-exact form: hash of the 10 bytes at p (the table's key), and their comparison on a hit
WV_DEV unsigned merHashBytes(const uint8_t* p)
{
  unsigned h = 2166136261u;
  for (int i = 0; i < SMALLSV_MER; ++i) h = (h ^ p[i]) * 16777619u;
  return h ^ (h >> 15);
}
WV_DEV bool merEqualBytes(const uint8_t* a, const uint8_t* b)
{
  bool eq = true;
  for (int i = 0; i < SMALLSV_MER; ++i) eq = eq && (a[i] == b[i]);
  return eq;
}
/// is the 10-mer at window + i one of the contig's?  The table holds 1 + the position in the contig of every distinct 10-mer.
WV_DEV bool merLookupBytes(const uint32_t* table, const unsigned mask, const uint8_t* contig, const uint8_t* mer)
{
  unsigned s = merHashBytes(mer) & mask;
  while (true) {
    const uint32_t v = table[s];
    if (v == 0) return false;
    if (merEqualBytes(contig + (v - 1), mer)) return true;
    s = (s + 1) & mask;
  }
}

/// columns per lane of bucket b
WV_DEV unsigned schedE(const ScheduleParams& P, const unsigned b)
{
  return unsigned(((b < 8) ? P.e_pack[0] : P.e_pack[1]) >> (8 * (b & 7))) & 255u;
}
/// the host's part: n_e and e_pack from the E set (at most 16 buckets of at most 255 columns)
WV_HD void schedPackE(ScheduleParams& P, const int* eSet, const unsigned n)
{
  P.n_e       = (n < 16) ? n : 16;
  P.e_pack[0] = P.e_pack[1] = 0;
  for (unsigned b = 0; b < P.n_e; ++b) P.e_pack[b >> 3] |= uint64_t(unsigned(eSet[b]) & 255u) << (8 * (b & 7));
}

/// bytes of LDS behind the table that the staged texts of a contig of `clen` bases and a window of `refSize` take at most (each is
/// copied in 16-byte units from the unit its first byte lies in)
WV_HD unsigned schedStagedBytes(const unsigned clen, const unsigned refSize)
{
  return ((clen + 30) & ~15u) + ((refSize + 30) & ~15u);
}
/// the table of a contig of `clen` bases fits SCHED_TABLE_BYTES
WV_HD bool schedTableFitsLds(const unsigned clen)
{
  return 8 * clen <= SCHED_TABLE_BYTES;
}

/// One contig (record `slot` of `locus`, text at seq_arena + seqOff, clen bases): 10-mer reference trim + alignment task set-up.
/// `ltable`: SCHED_TABLE_BYTES of LDS, `lseq`: lseqBytes of LDS for the staged texts (16-byte aligned), `gtable`: P.table_cap words
/// of memory for the table of a contig beyond 512 bases (nullptr: the caller has checked schedTableFitsLds).  BYTES: the caller's
/// contigs may hold bytes outside ACGT (the header comment; false: the 2-bit form alone is compiled).  Returns the slot's
/// SmallSvTaskInfo; every exit is wave-uniform and the caller stores the record after a single reconvergence point.  (An earlier
/// form that stored from lane 0 and `continue`d straight to the work-queue pop was compiled into a loop whose lanes left at
/// different times -- 63 lanes then re-ran the pop's readfirstlane without lane 0 and spun forever on loci without contigs.)
template <bool BYTES>
WV_DEV SmallSvTaskInfo scheduleContig(const ScheduleParams& P, const unsigned slot, const unsigned locus, const uint64_t seqOff, const unsigned clen,
                                      uint32_t* ltable, uint8_t* lseq, const unsigned lseqBytes, uint32_t* gtable)
{
  const unsigned     lane    = unsigned(wv::lane());
  SmallSvTaskInfo    info    = {0, 0, 0, -1};
  const uint8_t*     contigG = P.seq_arena + seqOff;
  const uint8_t*     refG    = P.refs + P.ref_off[locus];
  const int          refSize = int(P.ref_off[locus + 1] - P.ref_off[locus]);
  const SmallSvCuts  cuts    = P.cuts[locus];
  // contig and reference window into LDS (16 bytes per lane and load, all in flight together) when they fit; the scans then
  // run at LDS latency.  The task keeps the global pointers.
  const uint8_t* contig = contigG;
  const uint8_t* ref    = refG;
  {
    const uintptr_t gc = reinterpret_cast<uintptr_t>(contigG), gr = reinterpret_cast<uintptr_t>(refG);
    const unsigned  leadC = unsigned(gc & 15), leadR = unsigned(gr & 15);
    const unsigned  bytesC = (leadC + clen + 15) & ~15u, bytesR = (leadR + unsigned(refSize > 0 ? refSize : 0) + 15) & ~15u;
    if (bytesC + bytesR <= lseqBytes) {
      const u32x4* sc = reinterpret_cast<const u32x4*>(gc - leadC);
      const u32x4* sr = reinterpret_cast<const u32x4*>(gr - leadR);
      u32x4*       dc = reinterpret_cast<u32x4*>(lseq);
      u32x4*       dr = reinterpret_cast<u32x4*>(lseq + bytesC);
      for (unsigned i = lane; i < bytesC / 16; i += 64) dc[i] = sc[i];
      for (unsigned i = lane; i < bytesR / 16; i += 64) dr[i] = sr[i];
      wv::sync();
      contig = lseq + leadC;
      ref    = lseq + bytesC + leadR;
    }
  }

  if (clen < unsigned(SMALLSV_MER) || 2 * clen > P.table_cap) {
    info.status = 2;
    return info;
  }
  // hash set of the contig's 10-mers (:1987-1991)
  unsigned tcap = 64;
  while (tcap < 2 * clen) tcap <<= 1;
  const unsigned mask  = tcap - 1;
  uint32_t*      table = (tcap * 4 <= SCHED_TABLE_BYTES) ? ltable : gtable;
  for (unsigned i = lane; i < tcap; i += 64) table[i] = 0;
  // (wave-uniform) a byte outside ACGT in the contig: the table is keyed by the bytes
  bool exact = false;
  if (BYTES) {
    bool other = false;
    for (unsigned i = lane; i < clen; i += 64) other = other || (baseCode(contig[i]) > 3);
    exact = wv::any(other);
  }
  wv::sync();
  if (BYTES && exact) {
    for (unsigned p = lane; p + SMALLSV_MER <= clen; p += 64) {
      unsigned s = merHashBytes(contig + p) & mask;
      while (true) {
        const uint32_t old = wv::atomic_cas(&table[s], 0u, p + 1);
        if (old == 0 || merEqualBytes(contig + (old - 1), contig + p)) break;
        s = (s + 1) & mask;
      }
    }
  }
  for (int p0 = 0; !exact && p0 + SMALLSV_MER <= int(clen); p0 += MER_BATCH) {
    bool           valid;
    const unsigned code = merCodes55(contig, int(clen), p0, valid);
    if (!valid) continue;
    unsigned s = (code * 2654435761u) & mask;
    while (true) {
      const uint32_t old = wv::atomic_cas(&table[s], 0u, code + 1);
      if (old == 0 || old == code + 1) break;
      s = (s + 1) & mask;
    }
  }
  wv::sync();
  if (table == gtable) wv::fence_acquire();

  const int minRefIndex    = cuts.leadingCut;
  const int maxRefIndex    = refSize - (cuts.trailingCut + SMALLSV_MER);
  const int maxFwdRefIndex = (cuts.maxLeadingCut < maxRefIndex) ? cuts.maxLeadingCut : maxRefIndex;
  // first hit scanning forward (:1997-2001) and last hit scanning backward (:2004-2008, windows of 55 start positions, highest
  // window first), one window of each per round: the two scans are independent, so their lane shuffles and table probes overlap
  int adjLead = maxFwdRefIndex + 1;
  if (adjLead < minRefIndex) adjLead = minRefIndex;  // empty scan range: the loop variable keeps its initial value
  const int minRevRefIndex = (minRefIndex > refSize - cuts.maxTrailingCut) ? minRefIndex : (refSize - cuts.maxTrailingCut);
  int       revIndex       = minRevRefIndex - 1;
  if (revIndex > maxRefIndex) revIndex = maxRefIndex;  // empty scan range
  {
    int  fBase = minRefIndex, bTop = maxRefIndex;
    bool fDone = fBase > maxFwdRefIndex, bDone = bTop < minRevRefIndex;
    while (!fDone || !bDone) {
      const int      bBase = bTop - (MER_BATCH - 1);
      const unsigned cf = merLoadBase(ref, refSize, fDone ? -1000 : fBase), cb = merLoadBase(ref, refSize, bDone ? -1000 : bBase);
      bool           vf, vb;
      const unsigned codeF = merCodesFromBase(cf, vf), codeB = merCodesFromBase(cb, vb);
      const int      iF = fBase + int(lane), iB = bBase + int(lane);
      bool           hitF, hitB;
      if (BYTES && exact) {  // (the codes above go unused: a window 10-mer is looked up by its bytes)
        const bool inF = lane < unsigned(MER_BATCH) && iF >= 0 && iF + SMALLSV_MER <= refSize;
        const bool inB = lane < unsigned(MER_BATCH) && iB >= 0 && iB + SMALLSV_MER <= refSize;
        hitF = !fDone && inF && iF <= maxFwdRefIndex && merLookupBytes(table, mask, contig, ref + iF);
        hitB = !bDone && inB && iB >= minRevRefIndex && iB <= bTop && merLookupBytes(table, mask, contig, ref + iB);
      } else {
        hitF = !fDone && vf && iF <= maxFwdRefIndex && merLookup(table, mask, codeF);
        hitB = !bDone && vb && iB >= minRevRefIndex && iB <= bTop && merLookup(table, mask, codeB);
      }
      const uint64_t mF = wv::ballot(hitF), mB = wv::ballot(hitB);
      if (!fDone) {
        if (mF) {
          adjLead = fBase + wv::ctz(mF);
          fDone   = true;
        } else {
          fBase += MER_BATCH;
          fDone = fBase > maxFwdRefIndex;
        }
      }
      if (!bDone) {
        if (mB) {
          revIndex = bBase + (63 - wv::clz(mB));
          bDone    = true;
        } else {
          bTop -= MER_BATCH;
          bDone = bTop < minRevRefIndex;
        }
      }
    }
  }
  const int adjTrail = refSize - (revIndex + SMALLSV_MER);
  const int winLen   = refSize - adjLead - adjTrail;
  info.adj_leading_cut  = adjLead;
  info.adj_trailing_cut = adjTrail;
  if (winLen <= 0 || adjLead < 0 || adjTrail < 0) {
    info.status = 3;
    return info;
  }
  int            bucket = -1;
  const unsigned need   = (clen + 63) / 64;
  for (unsigned b = 0; b < P.n_e; ++b)
    if (schedE(P, b) >= need) {
      bucket = int(b);
      break;
    }
  if (bucket < 0) bucket = int(P.n_e) - 1;  // longer than 64 x 32 columns: the widest kernel runs it in strips (align_kernels.hpp)
  // The task's CIGAR region needs no allocator: contig texts do not overlap in the text arena, so neither do regions of 8 words
  // per contig base starting at 8 x the text offset (a task takes 4 * length + 16 words, contigs here hold >= 10 bases).  (One
  // bump-allocator atomic per contig on ONE address, next to one per locus for the work queue and one per contig for the bucket
  // lists, was what this kernel's 0.9 ms consisted of: ~40 k same-address L2 atomics.)
  const unsigned long long cig = 8ull * seqOff;
  if (cig + 4ull * clen + 16 > P.cigar_cap) {
    info.status = 5;
    return info;
  }
  if (lane == 0) {
    AlignTaskDev t;
    t.query     = contigG;
    t.ref1      = refG + adjLead;
    t.ref2      = nullptr;
    t.query_len = clen;
    t.ref1_len  = unsigned(winLen);
    t.ref2_len  = 0;
    t.cigar_off = uint32_t(cig);
    P.tasks[slot] = t;
  }
  info.bucket = bucket;
  return info;
}

/// longest reference a slab of the slot's bucket must hold for its task (bucket_maxref)
WV_DEV unsigned schedSlabLen(const ScheduleParams& P, const unsigned bucket, const unsigned clen, const unsigned winLen)
{
  return unsigned(alignSlabRefLen(1, int(schedE(P, bucket)), clen, winLen));
}

}  // namespace manta_dev
