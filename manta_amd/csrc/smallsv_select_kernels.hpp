// Contig ranking and refined candidate ranges of the small-SV path on the device: what SVCandidateAssemblyRefiner::getSmallSVAssembly
// does after the contigs' QC to decide which contig of a locus is used and which precise candidates come out of it
// (applications/GenerateSVCandidates/SVCandidateAssemblyRefiner.cpp, paths relative to the reference's src/c++/lib):
//   getVariantRange                                         :677-717
//   setSmallCandSV, the ranges and cipos                    :720-780
//   the rank-1 / rank-2 insertion                           :2119-2166
//   the swap test and its three float ratios                :2169-2219
// The host restatement is manta_amd/host/refiner_util.hpp (selectSmallSVContig, smallCandSVRanges); this file computes the same from what
// is resident when the QC kernel ends: scores and is_jumped of the alignments, the QC records and their merged segment lists, the
// support bitsets, the packed paths, the contig bytes and the locus' uncut reference window.
//
// Mapping: ONE 64-lane wavefront per LOCUS on a persistent grid over an atomic work queue; no LDS.
//   step 1  lane k holds contig k: score, is_jumped, is_candidate, largest_indel (== ContigScoringInfo::variantSize) and the popcount
//           of its support bitset (== supportReads.size(), pseudo reads included).
//   step 2  the rank rule, wave-uniform over the contigs in index order (the rule depends on the order), then the swap test.  The three
//           ratio tests are the reference's float expressions: int / unsigned -> float, ONE float multiply, a float compare.
//   step 3  per segment pair of the chosen contig's merged list: lanes over the path's segments, 64 per round with carried sums, give
//           refRange and readRange; lane k keeps candidate k.
//   step 4  right slide: lanes over offsets, 64 per round, the first mismatch from a ballot, bounded by the reference's own maximum.
//   step 5  left slide, the same way; it stops where the reference's index would become negative and reports the value reached.
// Every exit of a work item is wave-uniform and its records are stored after a single reconvergence point (smallsv_qc_kernels.hpp).
#pragma once
#include "smallsv_qc_kernels.hpp"

namespace manta_dev {

static const unsigned SS_MAX_CONTIGS = 64;           // contigs per locus (lane k holds contig k); beyond: QC_E_UNSUPPORTED
static const unsigned SS_MAX_CANDS   = QC_MAX_RUNS;  // candidates per locus: a merged segment list never holds more

/// one contig of a locus of the stand-alone call
struct SsTaskDev {
  const uint8_t*  contig;
  const uint32_t* cigar;    ///< BAM-packed segments, (len << 4) | op
  const uint64_t* support;  ///< contig.supportReads as a bitset of n_words qwords
  const uint32_t* segs;     ///< the QC record's merged list: n_segs (first,last) pairs
  uint32_t        contig_len, n_cigar, n_words, n_segs;
  int32_t         begin_pos, score;
  uint32_t        is_jumped, is_candidate, largest_indel;
  int32_t         status;  ///< != QC_OK: the alignment or the QC failed upstream, or something of the contig leaves its arena
};

/// one locus of the stand-alone call: tasks[first, first + n) and the uncut window
struct SsLocusDev {
  const uint8_t* ref;
  uint32_t       ref_len, first, n;
  int32_t        status;
};

/// one refined candidate (manta_small_cand_sv_t)
struct SsCandDev {
  int32_t  status;
  uint32_t seg_first, seg_last;
  int32_t  ref_begin, ref_end, read_begin, read_end;
  int32_t  cipos_begin, cipos_end;
};

struct SsLocusRecDev {
  int32_t  status;
  uint32_t selected;
  int32_t  best_contig;                 ///< index inside the locus, -1: none
  int32_t  rank1_contig, rank2_contig;  ///< before the swap test, -1: undefined
  uint32_t rank2_is_best;
  uint32_t n_candidates;
  uint32_t reserved;
};

struct SsParams {
  // stand-alone call
  const SsTaskDev*  tasks;  ///< nullptr: the staged pipeline's own state below
  const SsLocusDev* units;
  uint32_t          n_units;  ///< loci
  // staged pipeline (manta_smallsv_run with the stage set): the QC stage's inputs and records (qc.out, qc.segs) and the bitsets, none
  // of which left the device
  QcParams        qc;
  const uint64_t* bits_arena;
  // outputs
  SsLocusRecDev* locus_out;  ///< per locus
  SsCandDev*     cand_out;   ///< SS_MAX_CANDS per locus
  uint32_t*      counter;    ///< work-queue head
};

/// one task of manta_small_cand_sv_batch
struct SsCandTaskDev {
  const uint8_t*  ref;
  const uint8_t*  contig;
  const uint32_t* cigar;
  uint32_t        ref_len, contig_len, n_cigar;
  int32_t         begin_pos;
  uint32_t        seg_first, seg_last;
  int32_t         status;
  uint32_t        reserved;
};
struct SsCandParams {
  const SsCandTaskDev* tasks;
  uint32_t             n_tasks;
  SsCandDev*           out;
  uint32_t*            counter;
};

WV_DEV SsLocusDev ssLocusOf(const SsParams& P, const unsigned u)
{
  if (P.tasks) return P.units[u];
  SsLocusDev        L;
  const AsmLocusOut lo = P.qc.loci[u];
  L.status  = (lo.status == ASM_OK) ? QC_OK : QC_E_UNSUPPORTED;  // (the download reports the assembler's own code)
  L.first   = u * P.qc.max_assembly_count;
  L.n       = (lo.status == ASM_OK) ? ((lo.n_contigs < P.qc.max_assembly_count) ? lo.n_contigs : P.qc.max_assembly_count) : 0u;
  L.ref     = P.qc.refs + P.qc.ref_off[u];
  L.ref_len = unsigned(P.qc.ref_off[u + 1] - P.qc.ref_off[u]);
  return L;
}

/// contig c of the locus; the staged pipeline's task is what the QC kernel read and wrote for the slot, in place
WV_DEV SsTaskDev ssTaskOf(const SsParams& P, const unsigned u, const SsLocusDev& L, const unsigned c)
{
  if (P.tasks) return P.tasks[L.first + c];
  const unsigned       slot = L.first + c;
  const QcTaskDev      q    = qcSlotTask(P.qc, u, slot);
  const QcRecordDev    r    = P.qc.out[slot];
  const AlignResultDev a    = P.qc.results[slot];
  SsTaskDev            T;
  T.status        = (q.status != QC_OK) ? q.status : r.status;
  T.contig        = q.contig;
  T.contig_len    = q.contig_len;
  T.cigar         = q.cigar;
  T.n_cigar       = q.n_cigar;
  T.begin_pos     = q.begin_pos;
  T.support       = P.bits_arena + P.qc.contigs[slot].bits_off;
  T.n_words       = P.qc.loci[u].n_words;
  T.segs          = P.qc.segs + 2 * size_t(r.seg_off);
  T.n_segs        = (T.status == QC_OK) ? r.n_segments : 0u;
  T.score         = a.score;
  T.is_jumped     = a.is_jumped ? 1u : 0u;
  T.is_candidate  = r.is_candidate;
  T.largest_indel = r.largest_indel;
  return T;
}

/// inclusive prefix sum over the lanes, 64 bits wide: no path can wrap it
WV_DEV uint64_t ssScanIncl(uint64_t v)
{
  const int l = wv::lane();
  for (int off = 1; off < 64; off <<= 1) {
    const uint64_t o = wv::shfl(v, l - off);
    if (l >= off) v += o;
  }
  return v;
}

/// setSmallCandSV's ranges (:742-762) and getVariantRange (:677-717) of the path segments [first, last]; wave-uniform in every value
WV_DEV SsCandDev ssCand(const uint8_t* ref, const unsigned refLen, const uint8_t* contig, const unsigned contigLen, const uint32_t* cig,
                        const unsigned n, const int beginPos, const unsigned first, const unsigned last)
{
  const int lane = wv::lane();
  SsCandDev C;
  C.status    = QC_OK;
  C.seg_first = first;
  C.seg_last  = last;
  C.ref_begin = C.ref_end = C.read_begin = C.read_end = C.cipos_begin = C.cipos_end = 0;
  if (first > last || last >= n || beginPos < 0) {
    C.status = QC_E_INVALID_ARG;
    return C;
  }
  // step 3: the path, 64 segments per round with carried sums
  uint64_t totRef = 0, totRead = 0, refB = 0, refE = 0, readB = 0, readE = 0;
  for (unsigned base = 0; base < n; base += 64) {
    const unsigned i     = base + unsigned(lane);
    const bool     valid = i < n;
    const uint32_t w     = valid ? cig[i] : 0u;
    const unsigned op = w & 15u, len = w >> 4;
    const uint64_t fl = (valid && qcIsRefLen(op)) ? len : 0u, rl = (valid && qcIsReadLen(op)) ? len : 0u;
    const uint64_t inclF = ssScanIncl(fl) + totRef, inclR = ssScanIncl(rl) + totRead;
    if (first >= base && first - base < 64) {  // positions before the first segment of the range
      refB  = wv::shfl(inclF - fl, int(first - base));
      readB = wv::shfl(inclR - rl, int(first - base));
    }
    if (last >= base && last - base < 64) {  // ... and behind its last one
      refE  = wv::shfl(inclF, int(last - base));
      readE = wv::shfl(inclR, int(last - base));
    }
    totRef  = wv::shfl(inclF, 63);
    totRead = wv::shfl(inclR, 63);
  }
  // nothing outside the contig or the window is ever read
  if (uint64_t(unsigned(beginPos)) + totRef > refLen || totRead != contigLen || refLen > 0x7fffffffu || contigLen > 0x7fffffffu) {
    C.status = QC_E_INVALID_ARG;
    return C;
  }
  const unsigned refBegin = unsigned(beginPos) + unsigned(refB), refEnd = unsigned(beginPos) + unsigned(refE);
  const unsigned readBegin = unsigned(readB), readEnd = unsigned(readE);
  // step 4: how far the event slides to the right
  const unsigned roomF = refLen - refEnd, roomR = contigLen - readEnd;
  const unsigned maxRight = (roomF < roomR) ? roomF : roomR;
  unsigned       right    = maxRight;
  for (unsigned o0 = 0; o0 < maxRight; o0 += 64) {
    const unsigned o  = o0 + unsigned(lane);
    const bool     in = o < maxRight;
    const uint64_t m  = wv::ballot(in && ref[refBegin + (in ? o : 0u)] != contig[readBegin + (in ? o : 0u)]);
    if (m) {
      right = o0 + unsigned(wv::ctz(m));
      break;
    }
  }
  // step 5: ... and to the left.  The reference compares ref[refEnd + leftOffset - 1] with read[readEnd + leftOffset - 1] for
  // leftOffset = 0, -1, ..., max(-refBegin, -readBegin) and leaves the loop one step further when all of them match; where one of the
  // two indices would become negative the walk ends with the value reached
  const unsigned count   = ((refBegin < readBegin) ? refBegin : readBegin) + 1u;
  const unsigned lim     = (refEnd < readEnd) ? refEnd : readEnd;
  const unsigned maxLeft = (count < lim) ? count : lim;
  unsigned       left    = maxLeft;
  for (unsigned k0 = 0; k0 < maxLeft; k0 += 64) {
    const unsigned k  = k0 + unsigned(lane);
    const bool     in = k < maxLeft;
    const uint64_t m  = wv::ballot(in && ref[refEnd - 1u - (in ? k : 0u)] != contig[readEnd - 1u - (in ? k : 0u)]);
    if (m) {
      left = k0 + unsigned(wv::ctz(m));
      break;
    }
  }
  C.ref_begin   = int(refBegin);
  C.ref_end     = int(refEnd);
  C.read_begin  = int(readBegin);
  C.read_end    = int(readEnd);
  C.cipos_begin = -int(left);
  C.cipos_end   = int(right);
  return C;
}

/// one locus; `mine` is lane k's candidate k (valid for k < rec.n_candidates)
WV_DEV SsLocusRecDev ssLocus(const SsParams& P, const unsigned u, const SsLocusDev& L, SsCandDev& mine)
{
  const unsigned lane = unsigned(wv::lane());
  SsLocusRecDev  rec;
  rec.status       = L.status;
  rec.selected     = 0;
  rec.best_contig = rec.rank1_contig = rec.rank2_contig = -1;
  rec.rank2_is_best = rec.n_candidates = rec.reserved = 0;
  mine.status    = QC_OK;
  mine.seg_first = mine.seg_last = 0;
  mine.ref_begin = mine.ref_end = mine.read_begin = mine.read_end = mine.cipos_begin = mine.cipos_end = 0;
  if (L.status != QC_OK) return rec;
  if (L.n > SS_MAX_CONTIGS) {
    rec.status = QC_E_UNSUPPORTED;
    return rec;
  }
  // step 1: lane k keeps contig k
  const bool has = lane < L.n;
  int        status = QC_OK, score = 0;
  unsigned   jumped = 0, cand = 0, vsize = 0, support = 0;
  if (has) {
    const SsTaskDev T = ssTaskOf(P, u, L, lane);
    status = T.status;
    if (status == QC_OK) {
      score  = T.score;
      jumped = T.is_jumped;
      cand   = T.is_candidate;
      vsize  = T.largest_indel;
      for (unsigned w = 0; w < T.n_words; ++w) support += unsigned(wv::popc(T.support[w]));
    }
  }
  const uint64_t bad = wv::ballot(has && status != QC_OK);
  if (bad) {  // a contig of the locus failed upstream: the locus is not decided on part of its contigs
    rec.status = wv::readlane(status, wv::ctz(bad));
    return rec;
  }
  // step 2: the rank rule in index order (:2119-2166).  Every value of the rule is read with wv::readlane from the lane the scalar
  // loop counter names: the index is uniform, so the ranks live in scalar registers and the rule's branches are scalar branches
  const uint64_t isCand = wv::ballot(has && cand != 0), isJump = wv::ballot(has && jumped != 0);
  int r1 = -1, r2 = -1, s1 = 0, s2 = 0;
  bool j1 = false, j2 = false;
  for (unsigned c = 0; c < L.n; ++c) {
    if (!((isCand >> c) & 1u)) continue;
    const int  s = wv::readlane(score, int(c));
    const bool j = (isJump >> c) & 1u;
    // (an undefined rank 1 counts as not jumped, as the reference's default-constructed ContigScoringInfo does)
    const bool bothJumped = j && j1, bothNotJumped = !j && !j1;
    if (r1 < 0 || (j && !j1) || ((bothJumped || bothNotJumped) && s > s1)) {
      if (r1 >= 0) {  // the displaced rank 1 overwrites rank 2, whatever that one's score
        r2 = r1;
        s2 = s1;
        j2 = j1;
      }
      r1 = int(c);
      s1 = s;
      j1 = j;
    } else if (r2 < 0 || s > s2) {
      r2 = int(c);
      s2 = s;
      j2 = j;
    }
  }
  rec.rank1_contig = r1;
  rec.rank2_contig = r2;
  if (r1 < 0) return rec;
  int best = r1;
  if (r2 >= 0 && !(j1 && !j2)) {  // the swap test (:2169-2219): the reference's float expressions, nothing widened, nothing rearranged
    const unsigned n1 = wv::readlane(support, r1), n2 = wv::readlane(support, r2);
    const unsigned v1 = wv::readlane(vsize, r1), v2 = wv::readlane(vsize, r2);
    const float    minScore   = float(s1) * 0.9f;
    const float    minSupport = float(n1) * 1.2f;
    const float    minSize    = float(v1) * 1.1f;
    const bool     rank2IsBest = (float(s2) > minScore) && ((float(n2) > minSupport) || (float(v2) > minSize));
    if (rank2IsBest) {
      rec.rank2_is_best = 1;
      best              = r2;
    }
  }
  // steps 3-5: one candidate per segment pair of the chosen contig's merged list
  const SsTaskDev T = ssTaskOf(P, u, L, unsigned(best));
  if (T.n_segs > SS_MAX_CANDS) {
    rec.status = QC_E_INVALID_ARG;
    return rec;
  }
  int worst = QC_OK;
  for (unsigned k = 0; k < T.n_segs; ++k) {
    const SsCandDev C = ssCand(L.ref, L.ref_len, T.contig, T.contig_len, T.cigar, T.n_cigar, T.begin_pos, T.segs[2 * k], T.segs[2 * k + 1]);
    if (lane == k) mine = C;
    if (C.status != QC_OK && worst == QC_OK) worst = C.status;
  }
  if (worst != QC_OK) {
    rec.status = worst;
    return rec;
  }
  rec.selected     = 1;
  rec.best_contig  = best;
  rec.n_candidates = T.n_segs;
  return rec;
}

#if !MANTA_TU_DEFINES(MANTA_TU_GLUE)
WV_KERNEL void smallsv_select_kernel(const SsParams P);
#else
WV_KERNEL void smallsv_select_kernel(const SsParams P)
{
  while (true) {
    unsigned u = 0;
    if (wv::lane() == 0) u = wv::atomic_add(P.counter, 1u);
    u = wv::first(u);
    if (u >= P.n_units) break;
    const SsLocusDev    L = ssLocusOf(P, u);
    SsCandDev           mine;
    const SsLocusRecDev rec = ssLocus(P, u, L, mine);
    wv::sync();  // single reconvergence point of every exit of ssLocus
    const unsigned nOut = (rec.status == QC_OK) ? rec.n_candidates : 0u;
    if (unsigned(wv::lane()) < nOut) P.cand_out[size_t(u) * SS_MAX_CANDS + unsigned(wv::lane())] = mine;
    if (wv::lane() == 0) P.locus_out[u] = rec;
    wv::sync();  // (as in smallsv_qc_kernel: the store must not merge with the next pop)
  }
}
#endif

#if !MANTA_TU_DEFINES(MANTA_TU_GLUE)
WV_KERNEL void small_cand_sv_kernel(const SsCandParams P);
#else
WV_KERNEL void small_cand_sv_kernel(const SsCandParams P)
{
  while (true) {
    unsigned t = 0;
    if (wv::lane() == 0) t = wv::atomic_add(P.counter, 1u);
    t = wv::first(t);
    if (t >= P.n_tasks) break;
    const SsCandTaskDev T = P.tasks[t];
    SsCandDev           C;
    if (T.status != QC_OK) {
      C.status    = T.status;
      C.seg_first = T.seg_first;
      C.seg_last  = T.seg_last;
      C.ref_begin = C.ref_end = C.read_begin = C.read_end = C.cipos_begin = C.cipos_end = 0;
    } else {
      C = ssCand(T.ref, T.ref_len, T.contig, T.contig_len, T.cigar, T.n_cigar, T.begin_pos, T.seg_first, T.seg_last);
    }
    wv::sync();
    if (wv::lane() == 0) P.out[t] = C;
    wv::sync();  // (as in smallsv_qc_kernel: the store must not merge with the next pop)
  }
}
#endif

}  // namespace manta_dev
