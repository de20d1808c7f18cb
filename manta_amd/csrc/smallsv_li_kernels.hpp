// Large-insertion search of the small-SV path on the device: what SVCandidateAssemblyRefiner does on an isolated complex edge to find
// insertions too long to assemble through (applications/GenerateSVCandidates/SVCandidateAssemblyRefiner.cpp, paths relative to the
// reference's src/c++/lib):
//   isLargeInsertSegment / isLargeInsertAlignment            :563-639
//   the per-contig edge test of getSmallSVAssembly           :2079-2117   (apath_limit_read_length: blt_util/align_path.cpp:295-329)
//   processLargeInsertion: pairing, fake contig, alignment   :833-938
//   ... getLargestInsertSegment, isFinishedLargeInsertAlignment, getInsertTrim, the flank tests   :230-279, :642-665, :802-830, :940-974
// The host restatement is manta_amd/host/refiner_util.hpp (isLargeInsertAlignment, findLargeInsertionPair, getLargestInsertSegment,
// finishLargeInsertAlignment); this file computes the same from the BAM-packed '='/'X' paths, the contigs, their conservative ranges,
// the windows and the per-locus cuts, all of which are in HBM when the aligners end.
//
// Four stages, each ONE 64-lane wavefront per work item on a persistent grid over an atomic work queue:
//   smallsv_li_edge_kernel    per contig alignment: path segments across the lanes, 64 per round.  getMaxPathScore is three prefix sums
//                             (value, read offset, reference offset) and a running max carried between rounds; the reversed path's walk
//                             comes out of the same pass as the LAST minimum of the exclusive value prefix (a segment's value does not
//                             depend on its neighbours: the reference re-initialises its "previous segment was an indel" flag per segment).
//   smallsv_li_pair_kernel    per locus: lane r holds candidate r; one round of lanes per c1, lanes over c2 > c1 (up to 496 pairs of 32
//                             contigs).  The winner writes the fake contig (left, 100 x 'N', right) into an arena and a KIND-0 task into
//                             the E-bucket lists.
//   align_kernel<0, E>        the existing GlobalAligner kernels over those lists (launched by the host from the bucket counts)
//   smallsv_li_finish_kernel  per fake alignment: largest insert segment, the finished test with the complete aligner's scores, the
//                             insert trim and the two flank tests.
// Every exit of a work item is wave-uniform and its record is stored after a single reconvergence point (smallsv_qc_kernels.hpp).
#pragma once
#include "smallsv_qc_kernels.hpp"

namespace manta_dev {

static const unsigned LI_MIDDLE         = 100;  // the 'N' spacer of the fake contig, also trimInsertLength (:917)
static const int      LI_MAX_BREAK_DIST = 35;   // :848
static const unsigned LI_MIN_SPAN       = 40;   // minAlignReadLength, minExtendedReadLength, minAlignRefSpan (:569-571), minFlankSize (:558)
static const unsigned LI_MAX_CONTIGS    = 64;   // contigs per locus (lane k holds contig k); beyond: QC_E_UNSUPPORTED
static const unsigned LI_MAX_CONTIG_LEN = 1u << 28;
static const unsigned LI_NONE           = 0xffffffffu;
static const int      LI_E_EMPTY_SEQ    = -4;   // the C ABI's MANTA_E_EMPTY_SEQ

// words of LiParams::counts
enum { LI_CNT_BUCKET = 0, LI_CNT_MAXREF = 16, LI_CNT_FAKE_USED = 32, LI_CNT_CIGAR_USED = 34, LI_CNT_QUEUE = 36, LI_CNT_ALIGN_QUEUE = 40, LI_CNT_WORDS = 64 };

struct LiScores {
  int32_t match, mismatch, open, extend, off_edge;
};

/// one contig alignment of the stand-alone call
struct LiTaskDev {
  const uint8_t*  contig;
  const uint32_t* cigar;  ///< BAM-packed segments, (len << 4) | op
  uint32_t        contig_len, n_cigar;
  int32_t         begin_pos;
  int32_t         cons_begin, cons_end;  ///< contig.conservativeRange
  int32_t         status;                ///< != QC_OK: the alignment failed upstream
};

/// one locus of the stand-alone call: tasks[first, first + n)
struct LiLocusDev {
  const uint8_t* ref;  ///< the locus' uncut reference window
  uint32_t       ref_len;
  uint32_t       first, n;
  int32_t        leading_cut, trailing_cut;  ///< the UNADJUSTED cuts (:933-938)
  int32_t        status;
};

struct LiEdgeDev {
  int32_t  status;
  uint32_t is_candidate, is_left, is_right, contig_offset, ref_offset;
  int32_t  score;
  int32_t  begin_pos;  ///< the alignment's (for the pairing)
};

struct LiRecordDev {
  int32_t  status;
  uint32_t has_pair, left, right;  ///< contig indices inside the locus
  int32_t  break_dist, break_score;
  uint32_t left_len, fake_len;
  uint32_t n_insert_segments, seg_first, seg_last, is_finished;
  int32_t  trim_begin, trim_end;
  uint32_t is_flank_ok;
  int32_t  begin_pos;  ///< of the fake alignment, leading cut added (:940)
};

struct LiParams {
  // stand-alone call
  const LiTaskDev*  tasks;  ///< nullptr: the staged pipeline's own state below
  const LiLocusDev* units;
  uint32_t          n_units;  ///< loci
  // staged pipeline (manta_smallsv_run with the stage set): data that never left the device
  const AsmLocusOut*     loci;
  const AsmContigOut*    contigs;
  const uint8_t*         seq_arena;
  uint32_t               max_assembly_count;
  const uint8_t*         refs;
  const uint64_t*        ref_off;
  const SmallSvCuts*     cuts;
  const AlignTaskDev*    atasks;
  const AlignResultDev*  results;
  const SmallSvTaskInfo* info;
  const uint32_t*        cigar;
  LiScores edge, complete;  ///< largeInsertEdgeAlignScores, largeInsertCompleteAlignScores
  // outputs
  LiEdgeDev*      edges;       ///< per task / per (locus, contig slot)
  LiRecordDev*    recs;        ///< per locus
  AlignTaskDev*   li_tasks;    ///< per locus: the completion alignment
  AlignResultDev* li_results;  ///< (zeroed before the launch)
  uint32_t*       li_cigar;
  uint64_t        li_cigar_cap;  ///< u32 words
  uint8_t*        fake;          ///< fake contigs
  uint64_t        fake_cap;
  uint32_t*       bucket_ids;  ///< n_buckets x n_units
  uint32_t*       counts;      ///< LI_CNT_*
};

/// index into the aligners' E set {1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 24, 32} for a query (api_internal.hpp: pickE; the host checks
/// the two against each other)
WV_HD unsigned liBucketOf(const unsigned qlen)
{
  const unsigned need = (qlen + 63u) / 64u;
  if (need <= 6u) return need ? need - 1u : 0u;
  if (need <= 8u) return 6u;
  if (need <= 10u) return 7u;
  if (need <= 12u) return 8u;
  if (need <= 16u) return 9u;
  return (need <= 24u) ? 10u : 11u;
}
WV_HD unsigned liBucketE(const unsigned b)
{
  return (b < 6u) ? b + 1u : ((b < 9u) ? 2u * b - 4u : ((b == 9u) ? 16u : ((b == 10u) ? 24u : 32u)));
}

WV_DEV int liMaxI(int v)
{
  for (int off = 1; off < 64; off <<= 1) {
    const int o = wv::shfl(v, wv::lane() ^ off);
    v           = (o > v) ? o : v;
  }
  return v;
}
WV_DEV int liMinI(int v)
{
  for (int off = 1; off < 64; off <<= 1) {
    const int o = wv::shfl(v, wv::lane() ^ off);
    v           = (o < v) ? o : v;
  }
  return v;
}
/// position of the r-th set bit of m (r < popc(m))
WV_DEV int liNthBit(const uint64_t m, unsigned r)
{
  int pos = 0;
  for (int w = 32; w >= 1; w >>= 1) {
    const unsigned c = unsigned(wv::popc((m >> pos) & ((uint64_t(1) << w) - 1)));
    if (r >= c) {
      r -= c;
      pos += w;
    }
  }
  return pos;
}

// ------------------------------------------------------------------------------------------------------------------
// getMaxPathScore (AlignmentScoringUtilImpl.hpp:100-155, off-edge scored) of a path and of its reverse, in one pass
// ------------------------------------------------------------------------------------------------------------------
/// segments [lo, hi) of a path with up to two lengths replaced (what apath_limit_read_length leaves)
struct LiSpan {
  unsigned lo, hi;
  unsigned sIdx, sLen, eIdx, eLen;  ///< LI_NONE: no replacement; the `e` one is applied last
};
WV_DEV LiSpan liSpan(const unsigned lo, const unsigned hi)
{
  LiSpan S;
  S.lo = lo, S.hi = hi;
  S.sIdx = S.eIdx = LI_NONE;
  S.sLen = S.eLen = 0;
  return S;
}

struct LiWalk {
  int      fwdMax, revMax;  ///< maxVal of the path as given / reversed
  unsigned fwdRead, fwdRef, revRead, revRef;
  unsigned totRead, totRef;  ///< apath_read_length / apath_ref_length
};

WV_DEV int liSegVal(const LiScores& sc, const unsigned op, const unsigned len)
{
  if (op == 7u) return sc.match * int(len);
  if (op == 8u) return sc.mismatch * int(len);
  if (op == 1u || op == 2u) return sc.open + sc.extend * int(len);
  if (op == 4u) return sc.off_edge * int(len);
  return 0;
}

WV_DEV LiWalk liWalk(const LiScores& sc, const uint32_t* cig, const LiSpan& S)
{
  const int lane = wv::lane();
  LiWalk    W;
  W.fwdMax = W.revMax = 0;
  W.fwdRead = W.fwdRef = W.revRead = W.revRef = W.totRead = W.totRef = 0;
  int      val = 0, minEx = 0;
  unsigned rd = 0, rf = 0, minRd = 0, minRf = 0;
  bool     hasMin = false;
  for (unsigned base = S.lo; base < S.hi; base += 64) {
    const unsigned i     = base + unsigned(lane);
    const bool     valid = i < S.hi;
    const uint32_t w     = valid ? cig[i] : 0u;
    const unsigned op    = w & 15u;
    unsigned       len   = w >> 4;
    if (i == S.sIdx) len = S.sLen;
    if (i == S.eIdx) len = S.eLen;
    // walkPathScore advances its offsets on = X I D S only
    const int      v  = valid ? liSegVal(sc, op, len) : 0;
    const unsigned dr = (valid && (op == 7u || op == 8u || op == 1u || op == 4u)) ? len : 0u;
    const unsigned df = (valid && (op == 7u || op == 8u || op == 2u)) ? len : 0u;
    const int      inclV = int(qcScanIncl(unsigned(v))) + val;
    const unsigned inclR = qcScanIncl(dr) + rd, inclF = qcScanIncl(df) + rf;
    // as given: strict '>' from 0 at offsets 0, the earliest position wins ties
    const int roundMax = liMaxI(valid ? inclV : int(0x80000000u));
    if (roundMax > W.fwdMax) {
      const int at = wv::ctz(wv::ballot(valid && inclV == roundMax));
      W.fwdMax     = roundMax;
      W.fwdRead    = wv::shfl(inclR, at);
      W.fwdRef     = wv::shfl(inclF, at);
    }
    // reversed: the value after the reversed walk has taken segment j is total - (exclusive prefix at j); it visits j downwards, so
    // among equal minima of the prefix the LAST one is met first
    const int exV      = inclV - v;
    const int roundMin = liMinI(valid ? exV : 0x7fffffff);
    if (!hasMin || roundMin <= minEx) {
      const int at = 63 - wv::clz(wv::ballot(valid && exV == roundMin));
      minEx        = roundMin;
      minRd        = wv::shfl(inclR - dr, at);
      minRf        = wv::shfl(inclF - df, at);
      hasMin       = true;
    }
    val = wv::shfl(inclV, 63);
    rd  = wv::shfl(inclR, 63);
    rf  = wv::shfl(inclF, 63);
    W.totRead += qcSum((valid && qcIsReadLen(op)) ? len : 0u);
    W.totRef += qcSum((valid && qcIsRefLen(op)) ? len : 0u);
  }
  if (hasMin && val - minEx > 0) {
    W.revMax  = val - minEx;
    W.revRead = rd - minRd;
    W.revRef  = rf - minRf;
  }
  return W;
}

/// isLargeInsertSegment's four tests (:563-608) on a walk's maximum
WV_DEV bool liSegmentTest(const LiScores& sc, const unsigned contigOffset, const unsigned refOffset, const int score, const unsigned pathSize,
                          const unsigned trimInsertLength)
{
  if (refOffset < LI_MIN_SPAN) return false;
  if (contigOffset < LI_MIN_SPAN) return false;
  if ((pathSize - contigOffset) < (LI_MIN_SPAN + trimInsertLength)) return false;
  const int   optimalScore = int(contigOffset) * sc.match;
  const float scoreFrac    = float(score) / float(optimalScore);  // (an IEEE division, as the reference's)
  return !(scoreFrac < 0.75f);
}

struct LiInfo {
  bool     isLeft, isRight;
  unsigned contigOffset, refOffset;
  int      score;
};
/// isLargeInsertAlignment (:611-639)
WV_DEV LiInfo liAlignmentInfo(const LiScores& sc, const LiWalk& W)
{
  LiInfo I;
  I.isRight      = false;
  I.contigOffset = W.fwdRead, I.refOffset = W.fwdRef, I.score = W.fwdMax;
  I.isLeft = liSegmentTest(sc, W.fwdRead, W.fwdRef, W.fwdMax, W.totRead, 0);
  if (I.isLeft) return I;
  I.isRight      = liSegmentTest(sc, W.revRead, W.revRef, W.revMax, W.totRead, 0);
  I.contigOffset = W.totRead - W.revRead, I.refOffset = W.totRef - W.revRef, I.score = W.revMax;
  return I;
}

/// apath_limit_read_length(start, end) (align_path.cpp:295-329) as the span of the path it keeps.  The start segment is the first
/// read-consuming one whose running read length exceeds `start`, unless the end is reached first; the end segment the first whose
/// running read length reaches `end`; both length corrections apply, the start's first, also when they meet in one segment.
WV_DEV LiSpan liLimitReadLength(const uint32_t* cig, const unsigned n, const unsigned start, const unsigned end)
{
  const int lane = wv::lane();
  LiSpan    S    = liSpan(0, n);
  unsigned  carry = 0;
  for (unsigned base = 0; base < n; base += 64) {
    const unsigned i      = base + unsigned(lane);
    const bool     valid  = i < n;
    const uint32_t w      = valid ? cig[i] : 0u;
    const bool     isRead = valid && qcIsReadLen(w & 15u);
    const unsigned len    = w >> 4;
    const unsigned incl   = qcScanIncl(isRead ? len : 0u) + carry;
    const uint64_t mS = wv::ballot(isRead && incl > start), mE = wv::ballot(isRead && incl >= end);
    const int      sAt = mS ? wv::ctz(mS) : 64, eAt = mE ? wv::ctz(mE) : 64;
    if (S.sIdx == LI_NONE && sAt < 64 && sAt <= eAt) {
      S.sIdx = base + unsigned(sAt);
      S.sLen = wv::shfl(incl, sAt) - start;
      S.lo   = S.sIdx;
    }
    if (eAt < 64) {
      const unsigned at = base + unsigned(eAt), reach = wv::shfl(incl, eAt);
      unsigned       l  = (at == S.sIdx) ? S.sLen : wv::shfl(len, eAt);
      if (reach > end) l -= reach - end;
      S.eIdx = at;
      S.eLen = l;
      S.hi   = at + 1;
      break;
    }
    carry = wv::shfl(incl, 63);
  }
  return S;
}

// ------------------------------------------------------------------------------------------------------------------
// what a work item reads: the stand-alone call's records, or the staged pipeline's state in place
// ------------------------------------------------------------------------------------------------------------------
WV_DEV LiLocusDev liLocusOf(const LiParams& P, const unsigned u)
{
  if (P.tasks) return P.units[u];
  LiLocusDev        L;
  const AsmLocusOut lo = P.loci[u];
  L.status       = (lo.status == ASM_OK) ? QC_OK : QC_E_UNSUPPORTED;  // (the download reports the assembler's own code)
  L.first        = u * P.max_assembly_count;
  L.n            = (lo.status == ASM_OK) ? lo.n_contigs : 0u;
  L.ref          = P.refs + P.ref_off[u];
  L.ref_len      = unsigned(P.ref_off[u + 1] - P.ref_off[u]);
  L.leading_cut  = P.cuts[u].leadingCut;
  L.trailing_cut = P.cuts[u].trailingCut;
  return L;
}

WV_DEV LiTaskDev liTaskOf(const LiParams& P, const unsigned slot)
{
  if (P.tasks) return P.tasks[slot];
  LiTaskDev             T;
  const SmallSvTaskInfo inf = P.info[slot];
  const AlignResultDev  r   = P.results[slot];
  const AsmContigOut    co  = P.contigs[slot];
  const bool            ok  = inf.status == 0 && inf.bucket >= 0 && r.status == 0;
  T.status     = ok ? QC_OK : ((inf.status == 5) ? QC_E_DEVICE_FAULT : QC_E_UNSUPPORTED);  // (as manta_smallsv_download reports it)
  T.contig     = P.seq_arena + co.seq_off;
  T.contig_len = co.seq_len;
  T.cigar      = ok ? (P.cigar + P.atasks[slot].cigar_off) : P.cigar;
  T.n_cigar    = ok ? r.cigar1_len : 0u;
  T.begin_pos  = r.begin1 + inf.adj_leading_cut;  // SVCandidateAssemblyRefiner.cpp:2039
  T.cons_begin = co.cons_begin;
  T.cons_end   = co.cons_end;
  return T;
}

// ------------------------------------------------------------------------------------------------------------------
// (a) the per-contig edge test (:2079-2117)
// ------------------------------------------------------------------------------------------------------------------
WV_DEV LiEdgeDev liEdge(const LiParams& P, const LiTaskDev& T)
{
  LiEdgeDev rec;
  rec.status = T.status;
  rec.is_candidate = rec.is_left = rec.is_right = rec.contig_offset = rec.ref_offset = 0;
  rec.score     = 0;
  rec.begin_pos = T.begin_pos;
  if (T.status != QC_OK) return rec;
  const LiWalk full = liWalk(P.edge, T.cigar, liSpan(0, T.n_cigar));
  if (full.totRead != T.contig_len) {
    rec.status = QC_E_INVALID_ARG;
    return rec;
  }
  const unsigned start = unsigned(T.cons_begin > 0 ? T.cons_begin : 0), end = unsigned(T.cons_end > 0 ? T.cons_end : 0);
  const LiSpan   cons  = liLimitReadLength(T.cigar, T.n_cigar, start, end);
  const LiInfo   a     = liAlignmentInfo(P.edge, liWalk(P.edge, T.cigar, cons));
  if (!(a.isLeft || a.isRight)) return rec;
  // a conservative-path candidate is dropped when the full path disagrees on left/right; the offsets are the full path's
  const LiInfo b = liAlignmentInfo(P.edge, full);
  if (a.isLeft != b.isLeft || a.isRight != b.isRight) return rec;
  rec.is_candidate  = 1;
  rec.is_left       = a.isLeft ? 1u : 0u;
  rec.is_right      = a.isRight ? 1u : 0u;
  rec.contig_offset = b.contigOffset;
  rec.ref_offset    = b.refOffset;
  rec.score         = a.score;
  return rec;
}

#if !MANTA_TU_DEFINES(MANTA_TU_GLUE)
WV_KERNEL void smallsv_li_edge_kernel(const LiParams P);
#else
WV_KERNEL void smallsv_li_edge_kernel(const LiParams P)
{
  while (true) {
    unsigned u = 0;
    if (wv::lane() == 0) u = wv::atomic_add(P.counts + LI_CNT_QUEUE, 1u);
    u = wv::first(u);
    if (u >= P.n_units) break;
    const LiLocusDev L = liLocusOf(P, u);
    for (unsigned m = 0; m < L.n; ++m) {
      const LiTaskDev T   = liTaskOf(P, L.first + m);
      const LiEdgeDev rec = liEdge(P, T);
      wv::sync();  // single reconvergence point of every exit of liEdge
      if (wv::lane() == 0) P.edges[L.first + m] = rec;
      wv::sync();  // (as in smallsv_qc_kernel: the store must not merge with the next pop)
    }
  }
}
#endif

// ------------------------------------------------------------------------------------------------------------------
// (b) processLargeInsertion, first half (:850-938): the left/right pair, the fake contig, the completion task
// ------------------------------------------------------------------------------------------------------------------
WV_DEV LiRecordDev liPair(const LiParams& P, const unsigned u, const LiLocusDev& L)
{
  const unsigned lane = unsigned(wv::lane());
  LiRecordDev    rec;
  rec.status = L.status;
  rec.has_pair = rec.left = rec.right = 0;
  rec.break_dist = rec.break_score = 0;
  rec.left_len = rec.fake_len = 0;
  rec.n_insert_segments = rec.seg_first = rec.seg_last = rec.is_finished = 0;
  rec.trim_begin = rec.trim_end = 0;
  rec.is_flank_ok = 0;
  rec.begin_pos   = 0;
  if (L.status != QC_OK) return rec;
  if (L.n > LI_MAX_CONTIGS) {
    rec.status = QC_E_UNSUPPORTED;
    return rec;
  }
  // lane k: contig k of the locus
  const bool mine = lane < L.n;
  LiEdgeDev  e;
  e.status = QC_OK;
  e.is_candidate = e.is_left = e.is_right = e.contig_offset = e.ref_offset = 0;
  e.score = e.begin_pos = 0;
  uint64_t contigPtr = 0;
  unsigned contigLen = 0;
  if (mine) {
    e                 = P.edges[L.first + lane];
    const LiTaskDev T = liTaskOf(P, L.first + lane);
    contigPtr         = uint64_t(uintptr_t(T.contig));
    contigLen         = T.contig_len;
  }
  const uint64_t bad = wv::ballot(mine && e.status != QC_OK);
  if (bad) {  // a contig alignment of the locus failed: no search on part of its contigs
    rec.status = wv::shfl(e.status, wv::ctz(bad));
    return rec;
  }
  const uint64_t candMask = wv::ballot(mine && e.is_candidate != 0);
  const unsigned nCand    = unsigned(wv::popc(candMask));
  if (nCand < 2) return rec;
  // lane r: candidate r, in contig order (largeInsertionCandidateIndex)
  const int      src  = (lane < nCand) ? liNthBit(candMask, lane) : 0;
  const unsigned cIdx = unsigned(src);
  const unsigned cLeft = wv::shfl(e.is_left, src), cRight = wv::shfl(e.is_right, src);
  const int      cBreak = wv::shfl(e.begin_pos + int(e.ref_offset), src), cScore = wv::shfl(e.score, src);
  bool     isPair = false;
  int      bestDist = 0, bestScore = 0;
  unsigned best1 = 0, best2 = 0;
  for (unsigned c1 = 0; c1 + 1 < nCand; ++c1) {
    const unsigned left1 = wv::shfl(cLeft, int(c1)), right1 = wv::shfl(cRight, int(c1));
    const int      break1 = wv::shfl(cBreak, int(c1)), score1 = wv::shfl(cScore, int(c1));
    const unsigned c2    = c1 + 1 + lane;
    const bool     valid = c2 < nCand;
    const int      from  = valid ? int(c2) : 0;
    const unsigned left2 = wv::shfl(cLeft, from), right2 = wv::shfl(cRight, from);
    const int      break2 = wv::shfl(cBreak, from), score2 = wv::shfl(cScore, from);
    const long long diff = (long long)(break1) - (long long)(break2);
    const int       dist = int(diff < 0 ? -diff : diff);
    const bool      ok   = valid && ((left1 && right2) || (left2 && right1)) && dist <= LI_MAX_BREAK_DIST;
    if (!wv::any(ok)) continue;
    // the reference takes the first pair unconditionally and replaces it only on a strict improvement: the first in loop order among
    // the pairs minimal in (distance ascending, score descending)
    const int minDist  = liMinI(ok ? dist : 0x7fffffff);
    const int maxScore = liMaxI((ok && dist == minDist) ? score1 + score2 : int(0x80000000u));
    const int at       = wv::ctz(wv::ballot(ok && dist == minDist && score1 + score2 == maxScore));
    if (!isPair || minDist < bestDist || (minDist == bestDist && maxScore > bestScore)) {
      isPair    = true;
      bestDist  = minDist;
      bestScore = maxScore;
      best1     = c1;
      best2     = c1 + 1 + unsigned(at);
    }
  }
  if (!isPair) return rec;
  unsigned leftIdx = wv::shfl(cIdx, int(best1)), rightIdx = wv::shfl(cIdx, int(best2));
  if (wv::shfl(cRight, int(best1))) {
    const unsigned t = leftIdx;
    leftIdx          = rightIdx;
    rightIdx         = t;
  }
  rec.has_pair    = 1;
  rec.left        = leftIdx;
  rec.right       = rightIdx;
  rec.break_dist  = bestDist;
  rec.break_score = bestScore;
  const unsigned leftLen = wv::shfl(contigLen, int(leftIdx)), rightLen = wv::shfl(contigLen, int(rightIdx));
  const uint8_t* leftSeq  = reinterpret_cast<const uint8_t*>(uintptr_t(wv::shfl(contigPtr, int(leftIdx))));
  const uint8_t* rightSeq = reinterpret_cast<const uint8_t*>(uintptr_t(wv::shfl(contigPtr, int(rightIdx))));
  if (leftLen > LI_MAX_CONTIG_LEN || rightLen > LI_MAX_CONTIG_LEN) {
    rec.status = QC_E_UNSUPPORTED;
    return rec;
  }
  const unsigned fakeLen = leftLen + LI_MIDDLE + rightLen;
  rec.left_len = leftLen;
  rec.fake_len = fakeLen;
  if (L.leading_cut < 0 || L.trailing_cut < 0) {
    rec.status = QC_E_INVALID_ARG;
    return rec;
  }
  if (uint64_t(unsigned(L.leading_cut)) + unsigned(L.trailing_cut) >= L.ref_len) {  // the cut window is empty
    rec.status = LI_E_EMPTY_SEQ;
    return rec;
  }
  // room for the fake contig and for the alignment's path (align_kernels.hpp: 4 * query_len + 16 words per task)
  const unsigned long long fakeBytes = (uint64_t(fakeLen) + 15u) & ~uint64_t(15), cigarWords = 4ull * fakeLen + 16;
  unsigned long long       fakeOff = 0, cigarOff = 0;
  if (lane == 0) {
    fakeOff  = wv::atomic_add(reinterpret_cast<unsigned long long*>(P.counts + LI_CNT_FAKE_USED), fakeBytes);
    cigarOff = wv::atomic_add(reinterpret_cast<unsigned long long*>(P.counts + LI_CNT_CIGAR_USED), cigarWords);
  }
  fakeOff  = wv::shfl(uint64_t(fakeOff), 0);
  cigarOff = wv::shfl(uint64_t(cigarOff), 0);
  if (fakeOff + fakeBytes > P.fake_cap || cigarOff + cigarWords > P.li_cigar_cap) {
    rec.status = QC_E_CAPACITY;
    return rec;
  }
  uint8_t* const fake = P.fake + fakeOff;
  for (unsigned i = lane; i < fakeLen; i += 64)
    fake[i] = (i < leftLen) ? leftSeq[i] : ((i < leftLen + LI_MIDDLE) ? uint8_t('N') : rightSeq[i - leftLen - LI_MIDDLE]);
  if (lane == 0) {
    AlignTaskDev A;
    A.query     = fake;
    A.ref1      = L.ref + L.leading_cut;
    A.ref2      = nullptr;
    A.query_len = fakeLen;
    A.ref1_len  = L.ref_len - unsigned(L.leading_cut) - unsigned(L.trailing_cut);
    A.ref2_len  = 0;
    A.cigar_off = uint32_t(cigarOff);
    P.li_tasks[u] = A;
    const unsigned b  = liBucketOf(fakeLen);
    const unsigned at = wv::atomic_add(P.counts + LI_CNT_BUCKET + b, 1u);
    P.bucket_ids[size_t(b) * P.n_units + at] = u;
    const uint64_t slabRef = alignSlabRefLen(0, int(liBucketE(b)), fakeLen, A.ref1_len);
    wv::atomic_max(P.counts + LI_CNT_MAXREF + b, unsigned(slabRef > 0xffffffffull ? 0xffffffffull : slabRef));
  }
  return rec;
}

#if !MANTA_TU_DEFINES(MANTA_TU_GLUE)
WV_KERNEL void smallsv_li_pair_kernel(const LiParams P);
#else
WV_KERNEL void smallsv_li_pair_kernel(const LiParams P)
{
  while (true) {
    unsigned u = 0;
    if (wv::lane() == 0) u = wv::atomic_add(P.counts + LI_CNT_QUEUE + 1, 1u);
    u = wv::first(u);
    if (u >= P.n_units) break;
    const LiLocusDev  L   = liLocusOf(P, u);
    const LiRecordDev rec = liPair(P, u, L);
    wv::sync();  // single reconvergence point of every exit of liPair
    if (wv::lane() == 0) P.recs[u] = rec;
    wv::sync();
  }
}
#endif

// ------------------------------------------------------------------------------------------------------------------
// (d) processLargeInsertion, second half (:940-974)
// ------------------------------------------------------------------------------------------------------------------
/// getLargestInsertSegment(path, minSize) (:230-279): the indel run that holds the LAST insertion of the path's largest insertion size,
/// if that size reaches minSize (every insertion >= the running maximum replaces the run; note the '>=')
struct LiSegment {
  bool     found;
  unsigned first, last;
};
WV_DEV LiSegment liLargestInsertSegment(const uint32_t* cig, const unsigned n, const unsigned minSize)
{
  LiSegment seg;
  seg.found = false;
  seg.first = seg.last = 0;
  const int lane = wv::lane();
  unsigned  maxSize = 0, at = 0;
  bool      found = false;
  for (unsigned base = 0; base < n; base += 64) {
    const unsigned i     = base + unsigned(lane);
    const bool     isIns = i < n && (cig[i] & 15u) == 1u;
    const unsigned len   = isIns ? (cig[i] >> 4) : 0u;
    const unsigned m     = qcMax(len);
    if (wv::any(isIns) && m >= minSize && (!found || m >= maxSize)) {
      maxSize = m;
      at      = base + unsigned(63 - wv::clz(wv::ballot(isIns && len == m)));
      found   = true;
    }
  }
  if (!found) return seg;
  // the run around it: from behind the last non-indel segment before it to before the first one after it
  unsigned before = 0, after = n;  // (index + 1 of the last non-indel segment below `at`; index of the first above it)
  for (unsigned base = 0; base < n; base += 64) {
    const unsigned i      = base + unsigned(lane);
    const unsigned op     = (i < n) ? (cig[i] & 15u) : 1u;
    const bool     nonGap = i < n && op != 1u && op != 2u;
    const uint64_t below = wv::ballot(nonGap && i < at), above = wv::ballot(nonGap && i > at);
    if (below) before = base + unsigned(64 - wv::clz(below));
    if (above && after == n) after = base + unsigned(wv::ctz(above));
  }
  seg.found = true;
  seg.first = before;
  seg.last  = after - 1;
  return seg;
}

WV_DEV void liFinish(const LiParams& P, const unsigned u, LiRecordDev& rec)
{
  const AlignResultDev r = P.li_results[u];
  if (r.status != 0) {
    rec.status = QC_E_DEVICE_FAULT;
    return;
  }
  rec.begin_pos = r.begin1 + liLocusOf(P, u).leading_cut;
  const uint32_t* cig = P.li_cigar + P.li_tasks[u].cigar_off;
  const unsigned  n   = r.cigar1_len;
  const LiSegment seg = liLargestInsertSegment(cig, n, LI_MIDDLE);
  if (!seg.found) return;
  const unsigned first = seg.first, last = seg.last;
  rec.n_insert_segments = 1;
  rec.seg_first         = first;
  rec.seg_last          = last;
  // isFinishedLargeInsertAlignment (:642-665): the path up to the run's end as given, the path from the run's start reversed
  const LiWalk left = liWalk(P.complete, cig, liSpan(0, last + 1)), right = liWalk(P.complete, cig, liSpan(first, n));
  const bool   isLeft  = liSegmentTest(P.complete, left.fwdRead, left.fwdRef, left.fwdMax, left.totRead, LI_MIDDLE);
  const bool   isRight = liSegmentTest(P.complete, right.revRead, right.revRef, right.revMax, right.totRead, LI_MIDDLE);
  if (!(isLeft && isRight)) return;
  rec.is_finished = 1;
  // getInsertTrim (:802-830) and the two flank tests (:962-974)
  const LiWalk lead = liWalk(P.complete, cig, liSpan(0, first));
  rec.trim_begin = int(lead.totRead);
  rec.trim_end   = int(left.totRead);
  const int rightOffset = int(rec.left_len + LI_MIDDLE);
  rec.is_flank_ok = (!((rec.trim_begin + int(LI_MIN_SPAN)) > int(rec.left_len)) && !((rightOffset + int(LI_MIN_SPAN)) > rec.trim_end)) ? 1u : 0u;
}

#if !MANTA_TU_DEFINES(MANTA_TU_GLUE)
WV_KERNEL void smallsv_li_finish_kernel(const LiParams P);
#else
WV_KERNEL void smallsv_li_finish_kernel(const LiParams P)
{
  while (true) {
    unsigned u = 0;
    if (wv::lane() == 0) u = wv::atomic_add(P.counts + LI_CNT_QUEUE + 2, 1u);
    u = wv::first(u);
    if (u >= P.n_units) break;
    LiRecordDev rec = P.recs[u];
    if (rec.status != QC_OK || !rec.has_pair) continue;
    liFinish(P, u, rec);
    wv::sync();  // single reconvergence point of every exit of liFinish
    if (wv::lane() == 0) P.recs[u] = rec;
    wv::sync();
  }
}
#endif

}  // namespace manta_dev
