// Jump-alignment QC and contig selection of the spanning path on the device: what SVCandidateAssemblyRefiner::getJumpAssembly does with
// the contigs' GlobalJumpAligner results to decide which contig of a locus is used, and whether it is usable
// (applications/GenerateSVCandidates/SVCandidateAssemblyRefiner.cpp, paths relative to the reference's src/c++/lib):
//   isLowQualitySpanningSVAlignment                         :93-163
//   isJumpAlignmentQCFail                                   :1254-1271
//   isLowQualityJumpAlignment                               :1287-1309
//   selectJumpContigRNA                                     :1312-1358
//   selectJumpContigDNA                                     :1364-1398
// The host restatement is manta_amd/host/refiner_util.hpp (selectJumpContigDNA, selectJumpContigRNA); this file computes the same from
// the two BAM-packed '='/'X' (and 'N') paths of every contig, its score and, in RNA mode, its support bitset -- no contig text and no
// reference text.  The flank walk is qcFlankLow of smallsv_qc_kernels.hpp, over a whole path.
//
// Mapping: ONE 64-lane wavefront per LOCUS on a persistent grid over an atomic work queue; no LDS.
//   step 1  the contigs of the locus one after the other, lanes over a path's segments, 64 per round with carried sums: reference and
//           read length of both paths, the spliced length, the soft clips at the far ends.  Contig k's figures live in lane k.
//   step 2  DNA: the first contig with the strictly highest score among those that pass the fast QC; only that one gets the three QC
//           spans on both sides.  RNA: every passing contig gets them, then the score / support rule over the good ones.
// Every exit of a work item is wave-uniform and its records are stored after a single reconvergence point (smallsv_qc_kernels.hpp).
#pragma once
#include "smallsv_qc_kernels.hpp"

namespace manta_dev {

static const unsigned SEL_MAX_CONTIGS  = 64;  // contigs per locus (lane k holds contig k); beyond: QC_E_UNSUPPORTED
static const unsigned SEL_MIN_REF_SPAN = 20;  // minAlignRefSpan (:1256)

/// one contig alignment of the stand-alone call
struct SelTaskDev {
  const uint32_t* cigar1;  ///< BAM-packed segments, (len << 4) | op
  const uint32_t* cigar2;
  const uint64_t* support;  ///< contig.supportReads as a bitset (RNA mode; nullptr otherwise)
  uint32_t        n_cigar1, n_cigar2, n_words;
  int32_t         score;
  int32_t         status;  ///< != QC_OK: the alignment failed upstream
  uint32_t        reserved;
};

/// one locus of the stand-alone call: tasks[first, first + n)
struct SelLocusDev {
  uint32_t first, n;
  int32_t  status;
  uint32_t reserved;
};

struct SelContigDev {
  int32_t  status;
  uint32_t qc_fail;
  uint32_t ref_length1, ref_length2, read_length1, read_length2;
  uint32_t tested;    ///< isLowQualityJumpAlignment ran on this contig
  uint32_t span_low;  ///< bit s: align1 low at span s; bit 3 + s: align2 low at span s
  uint32_t low1, low2;
};

struct SelLocusRecDev {
  int32_t  status;
  uint32_t selected;
  int32_t  best_contig;  ///< index inside the locus, -1: none
  uint32_t n_qc_pass;
  int32_t  max_score;  ///< RNA mode: maxAlnScore (:1336-1343)
  uint32_t reserved;
};

struct SelParams {
  // stand-alone call
  const SelTaskDev*  tasks;  ///< nullptr: the staged pipeline's own state below
  const SelLocusDev* units;
  uint32_t           n_units;  ///< loci
  uint32_t           is_rna;
  // staged pipeline (manta_spanning_run with the stage set): data that never left the device
  const AsmLocusOut*    loci;
  uint32_t              max_assembly_count;
  const AlignTaskDev*   atasks;   ///< round 1
  const AlignTaskDev*   atasks2;  ///< round 2 (the re-alignment against the uncut references)
  const AlignResultDev* results;
  const AlignResultDev* results2;
  const SpanTaskInfo*   info;
  const uint32_t*       cigar;
  QcScores sc;  ///< contig filter scores
  // outputs
  SelContigDev*   contig_out;  ///< per task / per (locus, contig slot)
  SelLocusRecDev* locus_out;   ///< per locus
  uint32_t*       counter;     ///< work-queue head
};

WV_DEV SelLocusDev selLocusOf(const SelParams& P, const unsigned u)
{
  if (P.tasks) return P.units[u];
  SelLocusDev       L;
  const AsmLocusOut lo = P.loci[u];
  L.status   = (lo.status == ASM_OK) ? QC_OK : QC_E_UNSUPPORTED;  // (the download reports the assembler's own code)
  L.first    = u * P.max_assembly_count;
  L.n        = (lo.status == ASM_OK) ? ((lo.n_contigs < P.max_assembly_count) ? lo.n_contigs : P.max_assembly_count) : 0u;
  L.reserved = 0;
  return L;
}

/// the staged pipeline's task for a contig slot: what pack_results_kernel gathers for the host, read in place
WV_DEV SelTaskDev selTaskOf(const SelParams& P, const unsigned slot)
{
  if (P.tasks) return P.tasks[slot];
  SelTaskDev           T;
  const SpanTaskInfo   inf   = P.info[slot];
  const bool           uncut = inf.is_uncut != 0;
  const AlignResultDev r     = uncut ? P.results2[slot] : P.results[slot];
  const AlignTaskDev   a     = uncut ? P.atasks2[slot] : P.atasks[slot];
  const bool           ok    = inf.status == 0 && (uncut ? inf.bucket2 : inf.bucket) >= 0 && r.status == 0;
  // (as manta_spanning_download reports it)
  T.status   = ok ? QC_OK : ((inf.status == 5) ? QC_E_DEVICE_FAULT : ((inf.status == 6) ? -4 /* MANTA_E_EMPTY_SEQ */ : QC_E_UNSUPPORTED));
  T.cigar1   = ok ? (P.cigar + a.cigar_off) : P.cigar;
  T.n_cigar1 = ok ? r.cigar1_len : 0u;
  T.cigar2   = T.cigar1 + T.n_cigar1;
  T.n_cigar2 = ok ? r.cigar2_len : 0u;
  T.support  = nullptr;
  T.n_words  = 0;
  T.score    = r.score;
  T.reserved = 0;
  return T;
}

/// apath_ref_length, apath_read_length, apath_spliced_length and the soft clips at the two ends of one path
struct SelPath {
  unsigned totRef, totRead, spliced, leadClip, trailClip;
};
WV_DEV SelPath selPathSums(const uint32_t* cig, const unsigned n)
{
  SelPath S;
  S.totRef = S.totRead = S.spliced = 0;
  QcClips clips = qcClips();
  for (unsigned base = 0; base < n; base += 64) {
    const unsigned i     = base + unsigned(wv::lane());
    const bool     valid = i < n;
    const uint32_t w     = valid ? cig[i] : 0u;
    const unsigned op = w & 15u, len = w >> 4;
    S.totRef += qcSum((valid && qcIsRefLen(op)) ? len : 0u);
    S.totRead += qcSum((valid && qcIsReadLen(op)) ? len : 0u);
    S.spliced += qcSum((valid && op == 3u) ? len : 0u);
    qcClipRound(clips, valid, op, len);
  }
  S.leadClip  = clips.lead;
  S.trailClip = clips.trail;
  return S;
}

/// isLowQualityJumpAlignment (:1287-1309): all six verdicts, no short cut (bit s: align1 at span s, bit 3 + s: align2)
WV_DEV unsigned selSpanLow(const SelParams& P, const SelTaskDev& T, const SelPath& p1, const SelPath& p2)
{
  const bool     rna     = P.is_rna != 0;
  const unsigned minRead = rna ? 20u : 30u;  // minAlignReadLength (:101-107)
  unsigned       bits    = 0;
  for (unsigned s = 0; s < 3; ++s) {
    const unsigned span = rna ? ((s == 0) ? 36u : ((s == 1) ? 75u : 100u)) : ((s == 0) ? 75u : ((s == 1) ? 100u : 200u));
    // align1 is walked backwards from its last segment (its far end is the path's start), align2 forwards
    if (qcFlankLow(P.sc, T.cigar1, true, 0, T.n_cigar1, span + (rna ? p1.spliced : 0u), 0, minRead, p1.leadClip)) bits |= 1u << s;
    if (qcFlankLow(P.sc, T.cigar2, false, 0, T.n_cigar2, span + (rna ? p2.spliced : 0u), 0, minRead, p2.trailClip)) bits |= 8u << s;
  }
  return bits;
}

/// one locus; `mine` is lane k's record of contig k (valid for k < L.n when L.n <= SEL_MAX_CONTIGS)
WV_DEV SelLocusRecDev selLocus(const SelParams& P, const SelLocusDev& L, SelContigDev& mine)
{
  const unsigned lane = unsigned(wv::lane());
  SelLocusRecDev rec;
  rec.status      = L.status;
  rec.selected    = 0;
  rec.best_contig = -1;
  rec.n_qc_pass   = 0;
  rec.max_score   = 0;
  rec.reserved    = 0;
  mine.status     = (L.n > SEL_MAX_CONTIGS) ? QC_E_UNSUPPORTED : QC_OK;
  mine.qc_fail = mine.ref_length1 = mine.ref_length2 = mine.read_length1 = mine.read_length2 = 0;
  mine.tested = mine.span_low = mine.low1 = mine.low2 = 0;
  if (L.status != QC_OK) return rec;
  if (L.n > SEL_MAX_CONTIGS) {
    rec.status = QC_E_UNSUPPORTED;
    return rec;
  }
  const bool rna = P.is_rna != 0;
  // step 1: lane c keeps contig c
  int      score = 0, bad = QC_OK;
  unsigned support = 0;
  uint64_t pass = 0, good = 0;
  for (unsigned c = 0; c < L.n; ++c) {
    const SelTaskDev T = selTaskOf(P, L.first + c);
    if (T.status != QC_OK) {  // a contig alignment of the locus failed: the locus is not decided on part of its contigs
      if (lane == c) mine.status = T.status;
      if (bad == QC_OK) bad = T.status;
      continue;
    }
    const SelPath p1 = selPathSums(T.cigar1, T.n_cigar1), p2 = selPathSums(T.cigar2, T.n_cigar2);
    const bool    fail = T.n_cigar1 == 0 || T.n_cigar2 == 0 || p1.totRef < SEL_MIN_REF_SPAN || p2.totRef < SEL_MIN_REF_SPAN;
    unsigned      sup  = 0;
    if (rna)
      for (unsigned w0 = 0; w0 < T.n_words; w0 += 64) sup += qcSum((w0 + lane < T.n_words) ? unsigned(wv::popc(T.support[w0 + lane])) : 0u);
    unsigned bits   = 0;
    const bool test = rna && !fail;
    if (test) bits = selSpanLow(P, T, p1, p2);
    if (lane == c) {
      mine.qc_fail      = fail ? 1u : 0u;
      mine.ref_length1  = p1.totRef;
      mine.ref_length2  = p2.totRef;
      mine.read_length1 = p1.totRead;
      mine.read_length2 = p2.totRead;
      mine.tested       = test ? 1u : 0u;
      mine.span_low     = bits;
      mine.low1         = ((bits & 7u) == 7u) ? 1u : 0u;
      mine.low2         = ((bits >> 3) == 7u) ? 1u : 0u;
      score             = T.score;
      support           = sup;
    }
    if (!fail) pass |= uint64_t(1) << c;
    if (test && (bits & 7u) != 7u && (bits >> 3) != 7u) good |= uint64_t(1) << c;
  }
  if (bad != QC_OK) {
    rec.status = bad;
    return rec;
  }
  rec.n_qc_pass = unsigned(wv::popc(pass));
  // step 2
  if (!rna) {  // selectJumpContigDNA
    int best = -1, bestScore = 0;
    for (unsigned c = 0; c < L.n; ++c) {
      const int s = wv::shfl(score, int(c));
      if (((pass >> c) & 1u) && (best == -1 || s > bestScore)) {
        best      = int(c);
        bestScore = s;
      }
    }
    if (best == -1) return rec;
    const SelTaskDev T    = selTaskOf(P, L.first + unsigned(best));
    const SelPath    p1   = selPathSums(T.cigar1, T.n_cigar1), p2 = selPathSums(T.cigar2, T.n_cigar2);
    const unsigned   bits = selSpanLow(P, T, p1, p2);
    const bool       low1 = (bits & 7u) == 7u, low2 = (bits >> 3) == 7u;
    if (int(lane) == best) {
      mine.tested   = 1;
      mine.span_low = bits;
      mine.low1     = low1 ? 1u : 0u;
      mine.low2     = low2 ? 1u : 0u;
    }
    if (low1 || low2) return rec;
    rec.selected    = 1;
    rec.best_contig = best;
    return rec;
  }
  // selectJumpContigRNA
  if (good == 0) return rec;
  int      maxScore = 0;
  unsigned sel      = unsigned(wv::ctz(good));
  for (unsigned c = 0; c < L.n; ++c) {
    const int s = wv::shfl(score, int(c));
    if (((good >> c) & 1u) && s > maxScore) {
      maxScore = s;
      sel      = c;
    }
  }
  for (unsigned c = 0; c < L.n; ++c) {
    const int      s   = wv::shfl(score, int(c));
    const unsigned sup = wv::shfl(support, int(c)), selSup = wv::shfl(support, int(sel));
    if (((good >> c) & 1u) && (2ll * s > (long long)(maxScore)) && sup > selSup) sel = c;
  }
  rec.selected    = 1;
  rec.best_contig = int(sel);
  rec.max_score   = maxScore;
  return rec;
}

#if !MANTA_TU_DEFINES(MANTA_TU_GLUE)
WV_KERNEL void spanning_select_kernel(const SelParams P);
#else
WV_KERNEL void spanning_select_kernel(const SelParams P)
{
  while (true) {
    unsigned u = 0;
    if (wv::lane() == 0) u = wv::atomic_add(P.counter, 1u);
    u = wv::first(u);
    if (u >= P.n_units) break;
    const SelLocusDev    L = selLocusOf(P, u);
    SelContigDev         mine;
    const SelLocusRecDev rec = selLocus(P, L, mine);
    wv::sync();  // single reconvergence point of every exit of selLocus
    // (a locus beyond the envelope: every contig record carries the code, 64 per round)
    const unsigned nOut = (L.status == QC_OK) ? L.n : 0u;
    for (unsigned c0 = 0; c0 < nOut; c0 += 64)
      if (c0 + unsigned(wv::lane()) < nOut) P.contig_out[L.first + c0 + unsigned(wv::lane())] = mine;
    if (wv::lane() == 0) P.locus_out[u] = rec;
    wv::sync();  // (as in smallsv_qc_kernel: the store must not merge with the next pop)
  }
}
#endif

}  // namespace manta_dev
