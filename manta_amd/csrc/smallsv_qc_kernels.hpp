// Contig QC of the small-SV path on the device: what SVCandidateAssemblyRefiner::getSmallSVAssembly does with a contig's
// GlobalLargeIndelAligner result to decide whether the contig nominates a candidate, and with which path segments
// (applications/GenerateSVCandidates/SVCandidateAssemblyRefiner.cpp, paths relative to the reference's src/c++/lib):
//   getLargeIndelSegments                                   :173-208
//   getLargestIndelSize                                     :210-227
//   isLowQualitySmallSVAlignment                            :318-388
//   getQuerySeqMatchCount                                   :393-418
//   findCandidateVariantsFromComplexSVContigAlignment       :430-553
//   the two QC spans and their merge                        :2046-2066
// The host restatement is manta_amd/host/refiner_util.hpp (findSmallSVCandidateSegments); this file computes the same from the
// BAM-packed '='/'X' path, the contig bytes and the locus' uncut reference window, all of which are in HBM when the aligner ends.
//
// Mapping: ONE 64-lane wavefront per contig alignment on a persistent grid over an atomic work queue.
//   step 1  lanes over the path segments, 64 per step: indel runs from a ballot of "is I or D", "holds an indel >= min" as an OR inside
//           the run, prefix sums of read and reference length in the same pass.  Run k (of at most QC_MAX_RUNS qualifying ones) lives
//           in the registers of lane k.
//   step 2  flank QC: lanes over the flank's segments walking away from the breakend, the cut at maxQCRefSpan reference bases from a
//           ballot over the running reference length; read length and path score of the cut path are wave sums.
//   step 3  ambiguity filter (the hot loop): query and target staged in LDS, one placement per lane, 64 placements per round.  All lanes
//           read the same query byte (an LDS broadcast), consecutive lanes read consecutive target bytes (16-17 distinct dwords on
//           distinct banks: conflict free).  A lane abandons its placement at the reference's fail count; a wave vote ends the round.
//   step 4  every run kept by steps 2-3 still holds an indel >= min by construction (step 1 records no other run).
// Every exit of a work item is wave-uniform and its record is stored after a single reconvergence point (pipeline_kernels.hpp:113-116).
#pragma once
#include "pipeline_kernels.hpp"

namespace manta_dev {

static const unsigned QC_MAX_RUNS      = 32;    // indel runs >= min held per contig (lane k holds run k); beyond: QC_E_UNSUPPORTED
static const unsigned QC_SEARCH_WINDOW = 500;   // :497
static const unsigned QC_Q_LDS         = 512;   // staged query bytes (the filter's query is never longer than its 500-base target)
static const unsigned QC_T_LDS         = 1088;  // staged target window: 576 placements of a 512-base query
static const unsigned QC_LDS_BYTES     = QC_Q_LDS + QC_T_LDS;  // per wavefront
static const unsigned QC_SEG_PAIRS     = 3 * QC_MAX_RUNS;      // (first,last) pairs a contig can emit: merged list + the two spans' lists

// per-item status: the C ABI's codes (include/manta_amd.h)
static const int QC_OK = 0, QC_E_INVALID_ARG = -1, QC_E_UNSUPPORTED = -5, QC_E_CAPACITY = -6, QC_E_DEVICE_FAULT = -7;

/// what getPathScore reads of an AlignmentScores: the contig filter scores, SVRefinerOptions::contigFilterScores
struct QcScores {
  int32_t match, mismatch, open, extend;
};

struct QcTaskDev {
  const uint8_t*  contig;
  const uint32_t* cigar;  ///< BAM-packed segments, (len << 4) | op
  const uint8_t*  ref;    ///< the locus' uncut reference window (align1RefStr)
  uint32_t        contig_len, n_cigar, ref_len;
  int32_t         begin_pos;
  int32_t         status;  ///< != QC_OK: the alignment failed upstream; the item is skipped and carries this status
  uint32_t        reserved;
};

struct QcRecordDev {
  int32_t  status;
  uint32_t is_candidate, n_segments, largest_indel;
  uint32_t span_candidate[2], span_n_segments[2];
  uint32_t seg_off;  ///< first pair in the segment arena: n_segments merged pairs, then the two spans' lists
  uint32_t reserved;
};

struct QcParams {
  // stand-alone call: one unit == one task
  const QcTaskDev* tasks;  ///< nullptr: the staged pipeline's own state below, one unit == one locus
  uint32_t         n_units;
  // staged pipeline (manta_smallsv_run with QC set): data that never left the device
  const AsmLocusOut*     loci;
  const AsmContigOut*    contigs;
  const uint8_t*         seq_arena;
  uint32_t               max_assembly_count;
  const uint8_t*         refs;
  const uint64_t*        ref_off;
  const AlignTaskDev*    atasks;
  const AlignResultDev*  results;
  const SmallSvTaskInfo* info;
  const uint32_t*        cigar;
  QcScores sc;         ///< contig filter scores
  uint32_t min_indel;  ///< minCandidateIndelSize
  // outputs
  QcRecordDev* out;       ///< per task / per (locus, contig slot)
  uint32_t*    segs;      ///< pairs of u32
  uint32_t     seg_cap;   ///< pairs
  uint32_t*    seg_used;  ///< bump allocator (pairs)
  uint32_t*    counter;   ///< work-queue head
};

struct SeqMatchTaskDev {
  const uint8_t* target;
  const uint8_t* query;
  uint32_t       target_len, query_len;
  float          max_mismatch_rate;
  uint32_t       reserved;
};
struct SeqMatchParams {
  const SeqMatchTaskDev* tasks;
  uint32_t               n_tasks;
  uint32_t*              counts;
  uint32_t*              counter;
};

WV_DEV bool qcIsReadLen(const unsigned op) { return (0x193u >> op) & 1u; }  // M I S = X  (ALIGNPATH::is_segment_type_read_length)
WV_DEV bool qcIsRefLen(const unsigned op) { return (0x18du >> op) & 1u; }   // M D N = X  (ALIGNPATH::is_segment_type_ref_length)

/// inclusive prefix sum over the lanes
WV_DEV unsigned qcScanIncl(unsigned v)
{
  const int l = wv::lane();
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned o = wv::shfl(v, l - off);
    if (l >= off) v += o;
  }
  return v;
}
WV_DEV unsigned qcSum(unsigned v)
{
  for (int off = 1; off < 64; off <<= 1) v += wv::shfl(v, wv::lane() ^ off);
  return v;
}
WV_DEV unsigned qcMax(unsigned v)
{
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned o = wv::shfl(v, wv::lane() ^ off);
    v                = (o > v) ? o : v;
  }
  return v;
}
WV_DEV uint64_t qcBitRange(const int lo, const int hi)  // bits lo..hi
{
  const uint64_t upTo = (hi >= 63) ? ~uint64_t(0) : ((uint64_t(1) << (hi + 1)) - 1);
  return upTo & ~((uint64_t(1) << lo) - 1);
}

/// soft clips at the two ends of a path (hard clips skipped: apath_soft_clip_right_size of the path and of its reverse), fed the path's
/// segments 64 per round in path order
struct QcClips {
  unsigned lead, trail;
  bool     leading;  ///< no segment other than a clip seen yet
};
WV_DEV QcClips qcClips()
{
  QcClips C;
  C.lead = C.trail = 0;
  C.leading = true;
  return C;
}
WV_DEV void qcClipRound(QcClips& C, const bool valid, const unsigned op, const unsigned len)
{
  const int      lane = wv::lane();
  const unsigned sl   = (valid && op == 4u) ? len : 0u;
  const uint64_t mNC  = wv::ballot(valid && op != 4u && op != 5u);
  if (C.leading) {
    const int f = mNC ? wv::ctz(mNC) : 64;
    C.lead += qcSum((lane < f) ? sl : 0u);
    C.leading = (mNC == 0);
  }
  if (mNC) {
    const int lastNC = 63 - wv::clz(mNC);
    C.trail          = qcSum((lane > lastNC) ? sl : 0u);
  } else {
    C.trail += qcSum(sl);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// getQuerySeqMatchCount (:393-418)
// ------------------------------------------------------------------------------------------------------------------
/// the smallest mismatch count m for which the reference's float test `float(m) / float(Q) <= rate` is false (monotone in m), Q + 1 if
/// none is: the count at which a placement is abandoned (refiner_util.hpp:321-336).  The quotient is an IEEE division, correctly
/// rounded (hipcc's default for `/` on float; a reciprocal-and-multiply is one ulp off exactly at Q = 20, 40, 60, ...).  Q == 0: the
/// reference's 0 / 0 is NaN and fails the test at m == 0.
WV_DEV unsigned qcFailCount(const unsigned Q, const float rate)
{
  const float fq = float(Q);
  for (unsigned base = 0;; base += 64) {  // (base <= Q here; left without a wrap of base or m for Q up to 2^32 - 2)
    const unsigned m     = base + unsigned(wv::lane());
    const bool     fails = (unsigned(wv::lane()) <= Q - base) && !(float(m) / fq <= rate);
    const uint64_t mk    = wv::ballot(fails);
    if (mk) return base + unsigned(wv::ctz(mk));
    if (Q - base < 64) break;
  }
  return Q + 1;
}

/// placements 0 .. nPlace-1 of q[0, Q) in t[0, nPlace + Q - 1), one per lane, 64 per round.  A query 'N' always mismatches, bytes are
/// compared raw.  The vote is taken every eighth base: a round without a surviving lane ends there.
WV_DEV unsigned qcScanRounds(const uint8_t* q, const uint8_t* t, const unsigned Q, const unsigned nPlace, const unsigned failCount)
{
  unsigned hits = 0;
  for (unsigned p0 = 0; p0 < nPlace; p0 += 64) {
    const unsigned p     = p0 + unsigned(wv::lane());
    const bool     valid = p < nPlace;
    const uint8_t* tp    = t + (valid ? p : 0u);  // (lanes past the last placement read placement 0's bytes and count nothing)
    unsigned       mism  = 0;
    bool           alive = valid && failCount > 0;
    for (unsigned j = 0; j < Q; ++j) {
      if ((j & 7u) == 0 && !wv::any(alive)) break;
      const uint8_t qb = q[j], tb = tp[j];
      if (alive && (qb != tb || qb == 'N')) {
        ++mism;
        alive = mism < failCount;
      }
    }
    hits += unsigned(wv::popc(wv::ballot(alive)));
  }
  return hits;
}

WV_DEV void qcStage(uint8_t* dst, const uint8_t* src, const unsigned n)
{
  for (unsigned i = unsigned(wv::lane()); i < n; i += 64) dst[i] = src[i];
}

/// getQuerySeqMatchCount(target, query, rate) with any target length: the query (up to QC_Q_LDS bases) and a window of the target are
/// staged in LDS; the target moves through the window in steps of whole rounds.  A longer query is scanned from global memory.
WV_DEV unsigned qcSeqMatchCount(const uint8_t* target, const unsigned T, const uint8_t* query, const unsigned Q, const float rate, uint8_t* lds)
{
  if (Q > T) return 0;
  const unsigned failCount = qcFailCount(Q, rate);
  if (failCount == 0) return 0;  // (also Q == 0)
  const unsigned nPlace = T - Q + 1;
  if (Q > QC_Q_LDS) return qcScanRounds(query, target, Q, nPlace, failCount);
  uint8_t* const lq = lds;
  uint8_t* const lt = lds + QC_Q_LDS;
  wv::sync();  // the previous scan's readers are done
  qcStage(lq, query, Q);
  const unsigned perWindow = ((QC_T_LDS - Q + 1) / 64) * 64;  // >= 576 placements
  unsigned       hits      = 0;
  for (unsigned w0 = 0; w0 < nPlace; w0 += perWindow) {
    const unsigned np = (nPlace - w0 < perWindow) ? (nPlace - w0) : perWindow;
    wv::sync();
    qcStage(lt, target + w0, np + Q - 1);  // <= perWindow + Q - 1 <= QC_T_LDS
    wv::sync();
    hits += qcScanRounds(lq, lt, Q, np, failCount);
  }
  return hits;
}

// ------------------------------------------------------------------------------------------------------------------
// step 1: getLargeIndelSegments (:173-208) + the path's lengths and clips
// ------------------------------------------------------------------------------------------------------------------
struct QcRuns {
  // lane k: run k
  unsigned first, last;      ///< segment indices into the path as delivered
  unsigned readBefore;       ///< read length of the segments before `first`
  unsigned readThrough;      ///< read length of the segments up to and including `last`
  unsigned maxIndel;         ///< longest insertion / deletion of the run (getLargestIndelSize)
  // wave-uniform
  unsigned nRuns;            ///< qualifying runs found (may exceed QC_MAX_RUNS: the item is then unsupported)
  unsigned totRead, totRef;  ///< apath_read_length / apath_ref_length
  unsigned leadClip, trailClip;  ///< soft clip at either end of the path (hard clips skipped): apath_soft_clip_right_size of a flank
};

WV_DEV void qcRecordRun(QcRuns& R, const unsigned first, const unsigned last, const unsigned readBefore, const unsigned readThrough,
                        const unsigned maxIndel)
{
  if (unsigned(wv::lane()) == R.nRuns) {  // (no lane matches beyond QC_MAX_RUNS <= 64)
    R.first       = first;
    R.last        = last;
    R.readBefore  = readBefore;
    R.readThrough = readThrough;
    R.maxIndel    = maxIndel;
  }
  R.nRuns += 1;
}

WV_DEV QcRuns qcFindRuns(const uint32_t* cig, const unsigned n, const unsigned minIndel)
{
  const int lane = wv::lane();
  QcRuns    R;
  R.first = R.last = R.readBefore = R.readThrough = R.maxIndel = 0;
  R.nRuns = R.totRead = R.totRef = R.leadClip = R.trailClip = 0;
  // a run that reaches the last lane of a step stays open: whether it ends there is known from the next step's first segment
  bool     open = false, oBig = false;
  QcClips  clips = qcClips();
  unsigned oFirst = 0, oReadBefore = 0, oMax = 0;
  for (unsigned base = 0; base < n; base += 64) {
    const unsigned i     = base + unsigned(lane);
    const bool     valid = i < n;
    const uint32_t w     = valid ? cig[i] : 0u;
    const unsigned op = w & 15u, len = w >> 4;
    const unsigned rl    = (valid && qcIsReadLen(op)) ? len : 0u;
    const unsigned fl    = (valid && qcIsRefLen(op)) ? len : 0u;
    const bool     indel = valid && (op == 1u || op == 2u);
    const unsigned inclR = qcScanIncl(rl) + R.totRead, inclF = qcScanIncl(fl) + R.totRef;
    const uint64_t mI = wv::ballot(indel), mBig = wv::ballot(indel && len >= minIndel);
    qcClipRound(clips, valid, op, len);
    // the open run ended with the previous step
    if (open && !(mI & 1u)) {
      if (oBig) qcRecordRun(R, oFirst, base - 1, oReadBefore, R.totRead, oMax);
      open = false;
    }
    const bool more = base + 64 < n;
    uint64_t   ends = mI & ~(mI >> 1);
    if (more) ends &= ~(uint64_t(1) << 63);
    while (ends) {
      const int eb = wv::ctz(ends);
      ends &= ends - 1;
      const uint64_t below = ~mI & ((uint64_t(1) << eb) - 1);  // non-indel segments before the run's end
      const int      s     = below ? (64 - wv::clz(below)) : 0;
      const bool     cont  = open && s == 0;
      const uint64_t run   = qcBitRange(s, eb);
      unsigned       mx    = qcMax((indel && ((run >> lane) & 1u)) ? len : 0u);
      if (cont && oMax > mx) mx = oMax;
      const unsigned readB = wv::shfl(inclR - rl, s), readT = wv::shfl(inclR, eb);
      if ((mBig & run) || (cont && oBig)) qcRecordRun(R, cont ? oFirst : base + unsigned(s), base + unsigned(eb), cont ? oReadBefore : readB, readT, mx);
      if (cont) open = false;
    }
    if (more && (mI >> 63)) {
      const uint64_t below = ~mI & ((uint64_t(1) << 63) - 1);
      const int      s     = below ? (64 - wv::clz(below)) : 0;
      const bool     cont  = open && s == 0;
      const uint64_t run   = qcBitRange(s, 63);
      unsigned       mx    = qcMax((indel && ((run >> lane) & 1u)) ? len : 0u);
      const unsigned readB = wv::shfl(inclR - rl, s);
      if (!cont) {
        oFirst      = base + unsigned(s);
        oReadBefore = readB;
        oBig        = false;
        oMax        = 0;
      }
      oBig = oBig || (mBig & run);
      oMax = (mx > oMax) ? mx : oMax;
      open = true;
    }
    R.totRead = wv::shfl(inclR, 63);
    R.totRef  = wv::shfl(inclF, 63);
  }
  R.leadClip  = clips.lead;
  R.trailClip = clips.trail;
  return R;
}

// ------------------------------------------------------------------------------------------------------------------
// step 2: the flank walk of isLowQualitySmallSVAlignment (:318-388) and isLowQualitySpanningSVAlignment (:93-163)
// ------------------------------------------------------------------------------------------------------------------
WV_DEV int qcSegScore(const QcScores& sc, const unsigned op, const unsigned len)  // getPathScore, off-edge not scored (AlignmentScoringUtil.hpp:37)
{
  if (op == 7u) return sc.match * int(len);
  if (op == 8u) return sc.mismatch * int(len);
  if (op == 1u || op == 2u) return sc.open + sc.extend * int(len);
  return 0;
}

/// The flank is the segments [begin, end) of the path, walked away from the breakend: a leading flank from end - 1 downwards (the
/// reference reverses it), a trailing one from `begin` upwards.  Its first maxQCRefSpan reference bases are kept (apath_limit_ref_length);
/// low: fewer than minRefSpan reference bases (the small-SV flavour; 0 for the spanning one, which has no such test), fewer than
/// minReadLength read bases before the far soft clip, or less than 3/4 of the perfect score.  clipIfUncut: the soft clip at the far end
/// of the flank, which counts only when the walk was not cut.
WV_DEV bool qcFlankLow(const QcScores& sc, const uint32_t* cig, const bool isLeading, const unsigned begin, const unsigned end,
                       const unsigned maxQCRefSpan, const unsigned minRefSpan, const unsigned minReadLength, const unsigned clipIfUncut)
{
  const int      lane  = wv::lane();
  const unsigned count = end - begin;
  unsigned       covered = 0, readSize = 0;
  int            score = 0;
  bool           cut   = false;
  for (unsigned t0 = 0; t0 < count && !cut; t0 += 64) {
    const unsigned t     = t0 + unsigned(lane);
    const bool     valid = t < count;
    const unsigned j     = isLeading ? (end - 1 - t) : (begin + t);
    const uint32_t w     = valid ? cig[j] : 0u;
    const unsigned op = w & 15u, len = w >> 4;
    const bool     isRef = valid && qcIsRefLen(op);
    const unsigned incl  = qcScanIncl(isRef ? len : 0u) + covered;
    // apath_limit_ref_length: the first reference-consuming segment at which the span is covered is shortened, the rest dropped
    const uint64_t mCut = wv::ballot(isRef && incl >= maxQCRefSpan);
    bool           in   = valid;
    unsigned       eff  = len;
    if (mCut) {
      const int c = wv::ctz(mCut);
      in          = valid && lane <= c;
      if (lane == c) eff = len - (incl - maxQCRefSpan);
      cut = true;
    }
    readSize += qcSum((in && qcIsReadLen(op)) ? eff : 0u);
    score += int(qcSum(unsigned(in ? qcSegScore(sc, op, eff) : 0)));
    covered = wv::shfl(incl, 63);
  }
  const unsigned refSpan = cut ? maxQCRefSpan : covered;
  if (refSpan < minRefSpan) return true;
  // a cut path ends on a reference-consuming segment: no soft clip at its far end
  const unsigned clippedSize = readSize - (cut ? 0u : clipIfUncut);
  if (clippedSize < minReadLength) return true;
  const int   nonClipScore = (score > 0) ? score : 0;
  const int   optimalScore = int(clippedSize) * sc.match;
  const float scoreFrac    = float(nonClipScore) / float(optimalScore);
  return scoreFrac < 0.75f;
}

// ------------------------------------------------------------------------------------------------------------------
// one contig alignment: both QC spans, the merge (:2046-2066) and getLargestIndelSize of the kept list
// ------------------------------------------------------------------------------------------------------------------
WV_DEV QcRecordDev qcTask(const QcParams& P, const QcTaskDev& T, uint8_t* lds)
{
  const unsigned lane = unsigned(wv::lane());
  QcRecordDev    rec;
  rec.status = T.status;
  rec.is_candidate = rec.n_segments = rec.largest_indel = 0;
  rec.span_candidate[0] = rec.span_candidate[1] = rec.span_n_segments[0] = rec.span_n_segments[1] = 0;
  rec.seg_off = rec.reserved = 0;
  if (T.status != QC_OK) return rec;
  const QcRuns R = qcFindRuns(T.cigar, T.n_cigar, P.min_indel);
  // nothing outside the contig or the window is ever read
  if (T.begin_pos < 0 || uint64_t(unsigned(T.begin_pos)) + R.totRef > T.ref_len || R.totRead != T.contig_len) {
    rec.status = QC_E_INVALID_ARG;
    return rec;
  }
  if (R.nRuns > QC_MAX_RUNS) {
    rec.status = QC_E_UNSUPPORTED;
    return rec;
  }
  unsigned spanLo[2] = {0, 0}, spanN[2] = {0, 0};
  bool     spanCand[2] = {false, false};
  if (R.nRuns) {
    const unsigned first0 = wv::shfl(R.first, 0), last0 = wv::shfl(R.last, 0);
    const bool     isComplex = R.nRuns > 1 || first0 != last0;  // (fixed by the initial list, :449)
    const unsigned minSpan   = isComplex ? 35u : 30u;
    const unsigned refAlignStart = unsigned(T.begin_pos), refAlignEnd = unsigned(T.begin_pos) + R.totRef;
    for (int s = 0; s < 2; ++s) {
      const unsigned maxQCRefSpan = s ? 200u : 100u;
      unsigned       lo = 0, hi = R.nRuns - 1;
      bool           cand = true;
      // candidates are dropped from the left until the flank before the first one is clean, then from the right (:452-492); a list
      // that would become empty ends the span with its last element, as the reference's vector does
      while (true) {
        if (!qcFlankLow(P.sc, T.cigar, true, 0, wv::shfl(R.first, int(lo)), maxQCRefSpan, minSpan, minSpan, R.leadClip)) break;
        if (lo == hi) {
          cand = false;
          break;
        }
        ++lo;
      }
      while (cand) {
        if (!qcFlankLow(P.sc, T.cigar, false, wv::shfl(R.last, int(hi)) + 1, T.n_cigar, maxQCRefSpan, minSpan, minSpan, R.trailClip)) break;
        if (lo == hi) {
          cand = false;
          break;
        }
        --hi;
      }
      if (cand) {  // ambiguity filter (:497-536): either contig flank placing more than once inside a 500-base window
        const unsigned leftSize = wv::shfl(R.readBefore, int(lo)), endPos = wv::shfl(R.readThrough, int(hi));
        const unsigned leftSearchStart = (refAlignEnd > QC_SEARCH_WINDOW) ? (refAlignEnd - QC_SEARCH_WINDOW) : 0u;
        if (qcSeqMatchCount(T.ref + leftSearchStart, refAlignEnd - leftSearchStart, T.contig, leftSize, 0.05f, lds) > 1) {
          cand = false;
        } else {
          const unsigned room            = T.ref_len - refAlignStart;
          const unsigned rightSearchSize = (room < QC_SEARCH_WINDOW) ? room : QC_SEARCH_WINDOW;
          if (qcSeqMatchCount(T.ref + refAlignStart, rightSearchSize, T.contig + endPos, T.contig_len - endPos, 0.05f, lds) > 1) cand = false;
        }
      }
      spanCand[s] = cand;
      spanLo[s]   = lo;
      spanN[s]    = hi - lo + 1;
    }
  }
  // the longer list of the spans that nominate wins; ties keep the first (:2058-2065)
  unsigned keptLo = 0, keptN = 0;
  for (int s = 0; s < 2; ++s)
    if (spanCand[s] && spanN[s] > keptN) {
      keptLo = spanLo[s];
      keptN  = spanN[s];
    }
  rec.is_candidate  = (spanCand[0] || spanCand[1]) ? 1u : 0u;
  rec.n_segments    = keptN;
  rec.largest_indel = qcMax((lane >= keptLo && lane < keptLo + keptN) ? R.maxIndel : 0u);
  for (int s = 0; s < 2; ++s) {
    rec.span_candidate[s]  = spanCand[s] ? 1u : 0u;
    rec.span_n_segments[s] = spanN[s];
  }
  const unsigned total = keptN + spanN[0] + spanN[1];
  if (total) {
    unsigned off = 0;
    if (lane == 0) off = wv::atomic_add(P.seg_used, total);
    off = wv::first(off);
    if (uint64_t(off) + total > P.seg_cap) {
      rec.status = QC_E_CAPACITY;
      return rec;
    }
    rec.seg_off = off;
    unsigned at = off;
    for (int l = 0; l < 3; ++l) {
      const unsigned lo = (l == 0) ? keptLo : spanLo[l - 1], cnt = (l == 0) ? keptN : spanN[l - 1];
      if (lane >= lo && lane < lo + cnt) {
        P.segs[2 * size_t(at + (lane - lo))]     = R.first;
        P.segs[2 * size_t(at + (lane - lo)) + 1] = R.last;
      }
      at += cnt;
    }
  }
  return rec;
}

/// the staged pipeline's task for (locus, contig slot): what pack_results_kernel gathers for the host, read in place
WV_DEV QcTaskDev qcSlotTask(const QcParams& P, const unsigned locus, const unsigned slot)
{
  QcTaskDev             T;
  const SmallSvTaskInfo inf = P.info[slot];
  const AlignResultDev  r   = P.results[slot];
  const AsmContigOut    co  = P.contigs[slot];
  const bool            ok  = inf.status == 0 && inf.bucket >= 0 && r.status == 0;
  T.status     = ok ? QC_OK : ((inf.status == 5) ? QC_E_DEVICE_FAULT : QC_E_UNSUPPORTED);  // (as manta_smallsv_download reports it)
  T.contig     = P.seq_arena + co.seq_off;
  T.contig_len = co.seq_len;
  T.cigar      = ok ? (P.cigar + P.atasks[slot].cigar_off) : P.cigar;
  T.n_cigar    = ok ? r.cigar1_len : 0u;
  T.ref        = P.refs + P.ref_off[locus];
  T.ref_len    = unsigned(P.ref_off[locus + 1] - P.ref_off[locus]);
  T.begin_pos  = r.begin1 + inf.adj_leading_cut;  // SVCandidateAssemblyRefiner.cpp:2039
  T.reserved   = 0;
  return T;
}

#if !MANTA_TU_DEFINES(MANTA_TU_GLUE)
WV_KERNEL void smallsv_qc_kernel(const QcParams P);
#else
WV_KERNEL void smallsv_qc_kernel(const QcParams P)
{
  uint8_t* const lds = reinterpret_cast<uint8_t*>(wv::lds(QC_LDS_BYTES));
  while (true) {
    unsigned u = 0;
    if (wv::lane() == 0) u = wv::atomic_add(P.counter, 1u);
    u = wv::first(u);
    if (u >= P.n_units) break;
    unsigned members = 1;
    if (!P.tasks) {
      const AsmLocusOut lo = P.loci[u];
      members              = (lo.status == ASM_OK) ? lo.n_contigs : 0u;
    }
    for (unsigned m = 0; m < members; ++m) {
      const unsigned    idx = P.tasks ? u : (u * P.max_assembly_count + m);
      const QcTaskDev   T   = P.tasks ? P.tasks[u] : qcSlotTask(P, u, idx);
      const QcRecordDev rec = qcTask(P, T, lds);
      wv::sync();  // single reconvergence point of every exit of qcTask
      if (wv::lane() == 0) P.out[idx] = rec;
      // ... and one behind the store: without it the compiler joins lane 0's store with lane 0's next queue pop and sends the other 63
      // lanes round an inner loop that repeats the pop's readfirstlane without lane 0 -- they never leave it (seen on the hardware)
      wv::sync();
    }
  }
}
#endif

#if !MANTA_TU_DEFINES(MANTA_TU_GLUE)
WV_KERNEL void seq_match_count_kernel(const SeqMatchParams P);
#else
WV_KERNEL void seq_match_count_kernel(const SeqMatchParams P)
{
  uint8_t* const lds = reinterpret_cast<uint8_t*>(wv::lds(QC_LDS_BYTES));
  while (true) {
    unsigned t = 0;
    if (wv::lane() == 0) t = wv::atomic_add(P.counter, 1u);
    t = wv::first(t);
    if (t >= P.n_tasks) break;
    const SeqMatchTaskDev T    = P.tasks[t];
    const unsigned        hits = qcSeqMatchCount(T.target, T.target_len, T.query, T.query_len, T.max_mismatch_rate, lds);
    wv::sync();
    if (wv::lane() == 0) P.counts[t] = hits;
    wv::sync();  // (as in smallsv_qc_kernel: the store must not merge with the next pop)
  }
}
#endif

}  // namespace manta_dev
