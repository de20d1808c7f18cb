// Small-SV contig QC on the device (manta_smallsv_qc_batch) over the adapter types: findSmallSVCandidateSegments of refiner_util.hpp
// for a whole batch of contig alignments in one call, with that function as the fallback for a contig the device does not decide.
// A header of its own because it needs both the device adapter (manta_amd.hpp) and the host restatement (refiner_util.hpp), which
// builds on the former.
#pragma once

#include <string>
#include <utility>
#include <vector>

#include "manta_amd.hpp"
#include "refiner_util.hpp"

namespace manta_amd {

namespace detail {
/// BAM-packed words of a path (the ABI's op numbering)
inline void toPacked(const ALIGNPATH::path_t& path, std::vector<uint32_t>& out)
{
  static const uint32_t op[] = {15, 0, 1, 2, 3, 4, 5, 6, 7, 8};  // align_t -> BAM op (NONE has none)
  for (const ALIGNPATH::path_segment& ps : path) out.push_back((uint32_t(ps.length) << 4) | op[ps.type]);
}
/// one record's merged segment list
inline void qcSegments(const manta_smallsv_qc_t& q, const uint32_t* segArena, std::vector<segment_t>& out)
{
  out.clear();
  for (uint32_t k = 0; k < q.n_segments; ++k) out.emplace_back(segArena[2 * (q.seg_off + k)], segArena[2 * (q.seg_off + k) + 1]);
}
/// Did manta_smallsv_qc_batch / manta_smallsv_download_qc itself fail?  The calls return an item's code when items failed (every
/// other record is valid then) and write no record when they refuse or fail as a whole.  `qc`: the records, zeroed before the call.
inline bool qcCallFailed(const int rc, const std::vector<manta_smallsv_qc_t>& qc)
{
  if (rc == MANTA_OK) return false;
  for (const manta_smallsv_qc_t& q : qc)
    if (q.status == rc) return false;
  return true;
}
/// ... and manta_smallsv_large_insertion_batch / manta_smallsv_download_large_insertion, by the same rule
inline bool liCallFailed(const int rc, const std::vector<manta_large_insert_edge_t>& edges, const std::vector<manta_large_insertion_t>& li)
{
  if (rc == MANTA_OK) return false;
  for (const manta_large_insert_edge_t& e : edges)
    if (e.status == rc) return false;
  for (const manta_large_insertion_t& l : li)
    if (l.status == rc) return false;
  return true;
}
/// ... and manta_spanning_select_batch / manta_spanning_download_select
inline bool selectCallFailed(const int rc, const std::vector<manta_spanning_select_contig_t>& contigs, const std::vector<manta_spanning_select_t>& loci)
{
  if (rc == MANTA_OK) return false;
  for (const manta_spanning_select_contig_t& c : contigs)
    if (c.status == rc) return false;
  for (const manta_spanning_select_t& l : loci)
    if (l.status == rc) return false;
  return true;
}
/// ... and manta_smallsv_select_batch / manta_smallsv_download_select
inline bool smallSelectCallFailed(const int rc, const std::vector<manta_smallsv_select_t>& loci)
{
  if (rc == MANTA_OK) return false;
  if (rc == MANTA_E_CAPACITY) return true;  // (no per-item code: the candidate arena)
  for (const manta_smallsv_select_t& l : loci)
    if (l.status == rc) return false;
  return true;
}
}  // namespace detail

/// one contig alignment of the batch: getSmallSVAssembly's alignment.align, contig.seq and align1RefStr
struct SmallSVContigQCInput {
  const Alignment*   align;
  const std::string* contigSeq;
  const std::string* refSeq;
};

/// findSmallSVCandidateSegments(contigFilterScores, *items[i].align, *items[i].contigSeq, *items[i].refSeq, minCandidateVariantSize,
/// candidateSegments[i]) for every item, in one device call; isCandidate[i] is that call's return value.  An item the device does not
/// decide (MANTA_E_UNSUPPORTED, or any other per-item status) is recomputed with the host function.
inline void findSmallSVCandidateSegmentsBatch(
    const AlignmentScores<int>& contigFilterScores, const std::vector<SmallSVContigQCInput>& items, const unsigned minCandidateVariantSize,
    std::vector<std::vector<segment_t>>& candidateSegments, std::vector<char>& isCandidate, manta_ctx_t* ctx = nullptr,
    std::vector<int>* deviceStatus = nullptr)
{
  const size_t n = items.size();
  candidateSegments.assign(n, std::vector<segment_t>());
  isCandidate.assign(n, 0);
  if (deviceStatus) deviceStatus->assign(n, MANTA_OK);
  if (n == 0) return;
  if (!ctx) ctx = threadContext();
  std::vector<manta_asm_locus_result_t>  loci(n);
  std::vector<manta_asm_contig_t>        contigs(n);
  std::vector<manta_smallsv_alignment_t> aligns(n);
  std::vector<uint8_t>                   seq, refs;
  std::vector<uint32_t>                  cigar;
  std::vector<uint64_t>                  refOff(n + 1, 0);
  for (size_t i = 0; i < n; ++i) {
    loci[i]              = manta_asm_locus_result_t();
    loci[i].n_contigs    = 1;
    loci[i].first_contig = uint32_t(i);
    contigs[i]           = manta_asm_contig_t();
    contigs[i].seq_off   = seq.size();
    contigs[i].seq_len   = uint32_t(items[i].contigSeq->size());
    seq.insert(seq.end(), items[i].contigSeq->begin(), items[i].contigSeq->end());
    aligns[i]                  = manta_smallsv_alignment_t();
    aligns[i].align.begin_pos1 = items[i].align->beginPos;
    aligns[i].align.cigar1_off = cigar.size();
    detail::toPacked(items[i].align->apath, cigar);
    aligns[i].align.cigar1_len = uint32_t(cigar.size() - aligns[i].align.cigar1_off);
    refs.insert(refs.end(), items[i].refSeq->begin(), items[i].refSeq->end());
    refOff[i + 1] = refs.size();
  }
  seq.push_back(0);
  refs.push_back(0);
  cigar.push_back(0);
  std::vector<manta_smallsv_qc_t> qc(n);
  std::vector<uint32_t>           segs(2 * 96 * n);
  uint64_t                        used = 0;
  const manta_align_scores_t      sc   = detail::toAbi(contigFilterScores);
  const int rc = manta_smallsv_qc_batch(ctx, &sc, minCandidateVariantSize, uint32_t(n), loci.data(), contigs.data(), aligns.data(), seq.data(),
                                        cigar.data(), refs.data(), refOff.data(), qc.data(), segs.data(), segs.size() / 2, &used);
  if (detail::qcCallFailed(rc, qc)) throw GeneralException("manta_amd small-SV contig QC: " + std::string(manta_last_error(ctx)), rc);
  for (size_t i = 0; i < n; ++i) {
    if (deviceStatus) (*deviceStatus)[i] = qc[i].status;
    if (qc[i].status == MANTA_OK) {
      detail::qcSegments(qc[i], segs.data(), candidateSegments[i]);
      isCandidate[i] = qc[i].is_candidate ? 1 : 0;
    } else {
      isCandidate[i] = findSmallSVCandidateSegments(contigFilterScores, *items[i].align, *items[i].contigSeq, *items[i].refSeq,
                                                    minCandidateVariantSize, candidateSegments[i])
                           ? 1
                           : 0;
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// large-insertion search (manta_smallsv_large_insertion_batch) over the adapter types
// ------------------------------------------------------------------------------------------------------
/// one locus of the batch: its contigs with their GlobalLargeIndelAligner alignments (beginPos in window coordinates), the uncut
/// reference window and the UNADJUSTED cuts
struct LargeInsertionLocusInput {
  const Assembly*               contigs;
  const std::vector<Alignment>* aligns;
  const std::string*            refSeq;
  pos_t                         leadingCut, trailingCut;
};

/// what processLargeInsertion knows of a locus before it needs the SVCandidate
struct LargeInsertionLocusResult {
  std::vector<LargeInsertionInfo> info;       ///< largeInsertInfo, one per contig (cleared for a contig that is no candidate)
  std::vector<unsigned>           candIndex;  ///< largeInsertionCandidateIndex
  LargeInsertionPair              pair;
  AlignmentResult<int>            fakeAlignment;  ///< of left + 100 x 'N' + right, beginPos moved by the leading cut; set with a pair
  LargeInsertionFinish            finish;
  int                             deviceStatus = MANTA_OK;  ///< != MANTA_OK: the host functions computed this locus
};

/// the same on the host: the free functions of refiner_util.hpp plus one GlobalAligner alignment through manta_align_batch
inline void findLargeInsertionHost(
    const AlignmentScores<int>& edgeScores, const AlignmentScores<int>& completeScores, const LargeInsertionLocusInput& in,
    LargeInsertionLocusResult& r, manta_ctx_t* ctx)
{
  const unsigned n = unsigned(in.contigs->size());
  r.info.assign(n, LargeInsertionInfo());
  r.candIndex.clear();
  r.pair = LargeInsertionPair();
  r.fakeAlignment.clear();
  r.finish = LargeInsertionFinish();
  std::vector<pos_t> beginPos(n);
  for (unsigned i = 0; i < n; ++i) {
    const AssembledContig& c((*in.contigs)[i]);
    beginPos[i] = (*in.aligns)[i].beginPos;
    if (isLargeInsertionEdge(edgeScores, (*in.aligns)[i].apath, c.conservativeRange.begin_pos(), c.conservativeRange.end_pos(), r.info[i]))
      r.candIndex.push_back(i);
  }
  r.pair = findLargeInsertionPair(r.candIndex, beginPos, r.info);
  if (!r.pair.isPair) return;
  const std::string& left((*in.contigs)[r.pair.leftIndex].seq);
  const std::string  fake = left + std::string(100, 'N') + (*in.contigs)[r.pair.rightIndex].seq;
  const std::string  window = in.refSeq->substr(size_t(in.leadingCut), in.refSeq->size() - size_t(in.leadingCut) - size_t(in.trailingCut));
  const std::string  arena = fake + window;
  manta_align_task_t task  = manta_align_task_t();
  task.query_len = uint32_t(fake.size());
  task.ref1_off  = fake.size();
  task.ref1_len  = uint32_t(window.size());
  manta_align_result_t       res = manta_align_result_t();
  std::vector<uint32_t>      cigar(2 * fake.size() + 8);
  uint64_t                   used = 0;
  const manta_align_scores_t sc   = detail::toAbi(completeScores);
  const int rc = manta_align_batch(ctx, MANTA_ALIGNER_GLOBAL, &sc, 0, 1, &task, reinterpret_cast<const uint8_t*>(arena.data()), arena.size(), &res,
                                   cigar.data(), cigar.size(), &used);
  if (rc != MANTA_OK) throw GeneralException("manta_amd large-insertion alignment: " + std::string(manta_last_error(ctx)), rc);
  r.fakeAlignment.score          = res.score;
  r.fakeAlignment.isJumped       = res.is_jumped != 0;
  r.fakeAlignment.align.beginPos = res.begin_pos1 + in.leadingCut;
  detail::toPath(cigar.data() + res.cigar1_off, res.cigar1_len, r.fakeAlignment.align.apath);
  r.finish = finishLargeInsertAlignment(completeScores, r.fakeAlignment.align.apath, unsigned(left.size()));
}

/// The large-insertion search of every locus in ONE device call; a locus with an item the device does not decide (any per-item
/// status) is recomputed whole by findLargeInsertionHost and carries that status in deviceStatus.
inline void findLargeInsertionBatch(
    const AlignmentScores<int>& edgeScores, const AlignmentScores<int>& completeScores, const std::vector<LargeInsertionLocusInput>& items,
    std::vector<LargeInsertionLocusResult>& results, manta_ctx_t* ctx = nullptr)
{
  const size_t n = items.size();
  results.assign(n, LargeInsertionLocusResult());
  if (n == 0) return;
  if (!ctx) ctx = threadContext();
  std::vector<manta_asm_locus_result_t>  loci(n);
  std::vector<manta_asm_contig_t>        contigs;
  std::vector<manta_smallsv_alignment_t> aligns;
  std::vector<manta_ref_cuts_t>          cuts(n);
  std::vector<uint8_t>                   seq, refs;
  std::vector<uint32_t>                  cigar;
  std::vector<uint64_t>                  refOff(n + 1, 0);
  uint64_t                               cigarCap = 0;
  for (size_t l = 0; l < n; ++l) {
    const LargeInsertionLocusInput& in(items[l]);
    loci[l]              = manta_asm_locus_result_t();
    loci[l].n_contigs    = uint32_t(in.contigs->size());
    loci[l].first_contig = uint32_t(contigs.size());
    uint64_t total = 0;
    for (size_t c = 0; c < in.contigs->size(); ++c) {
      const AssembledContig& ctg((*in.contigs)[c]);
      manta_asm_contig_t     rec = manta_asm_contig_t();
      rec.seq_off            = seq.size();
      rec.seq_len            = uint32_t(ctg.seq.size());
      rec.conservative_begin = ctg.conservativeRange.begin_pos();
      rec.conservative_end   = ctg.conservativeRange.end_pos();
      contigs.push_back(rec);
      seq.insert(seq.end(), ctg.seq.begin(), ctg.seq.end());
      total += ctg.seq.size();
      manta_smallsv_alignment_t a = manta_smallsv_alignment_t();
      a.align.begin_pos1          = (*in.aligns)[c].beginPos;
      a.align.cigar1_off          = cigar.size();
      detail::toPacked((*in.aligns)[c].apath, cigar);
      a.align.cigar1_len = uint32_t(cigar.size() - a.align.cigar1_off);
      aligns.push_back(a);
    }
    cigarCap += 2 * (total + 100) + 8;
    refs.insert(refs.end(), in.refSeq->begin(), in.refSeq->end());
    refOff[l + 1] = refs.size();
    cuts[l]       = manta_ref_cuts_t{in.leadingCut, in.trailingCut, 0, 0};
  }
  seq.push_back(0);
  refs.push_back(0);
  cigar.push_back(0);
  contigs.push_back(manta_asm_contig_t());
  aligns.push_back(manta_smallsv_alignment_t());
  std::vector<manta_large_insert_edge_t> edges(contigs.size());
  std::vector<manta_large_insertion_t>   li(n);
  std::vector<uint32_t>                  out(cigarCap + 1);
  uint64_t                               used = 0;
  const manta_align_scores_t             esc = detail::toAbi(edgeScores), csc = detail::toAbi(completeScores);
  const int rc = manta_smallsv_large_insertion_batch(ctx, &esc, &csc, uint32_t(n), loci.data(), contigs.data(), aligns.data(), seq.data(), cigar.data(),
                                                     refs.data(), refOff.data(), cuts.data(), edges.data(), li.data(), out.data(), out.size(), &used);
  if (detail::liCallFailed(rc, edges, li)) throw GeneralException("manta_amd large-insertion search: " + std::string(manta_last_error(ctx)), rc);
  for (size_t l = 0; l < n; ++l) {
    LargeInsertionLocusResult& r(results[l]);
    const unsigned             count = loci[l].n_contigs;
    int                        status = li[l].status;
    for (unsigned c = 0; c < count && status == MANTA_OK; ++c) status = edges[loci[l].first_contig + c].status;
    if (status != MANTA_OK) {
      findLargeInsertionHost(edgeScores, completeScores, items[l], r, ctx);
      r.deviceStatus = status;
      continue;
    }
    r.info.assign(count, LargeInsertionInfo());
    for (unsigned c = 0; c < count; ++c) {
      const manta_large_insert_edge_t& e(edges[loci[l].first_contig + c]);
      if (!e.is_candidate) continue;
      r.info[c].isLeftCandidate  = e.is_left != 0;
      r.info[c].isRightCandidate = e.is_right != 0;
      r.info[c].contigOffset     = e.contig_offset;
      r.info[c].refOffset        = e.ref_offset;
      r.info[c].score            = e.score;
      r.candIndex.push_back(c);
    }
    const manta_large_insertion_t& d(li[l]);
    if (!d.has_pair) continue;
    r.pair.isPair     = true;
    r.pair.leftIndex  = d.left_contig;
    r.pair.rightIndex = d.right_contig;
    r.pair.breakDist  = d.break_dist;
    r.pair.breakScore = d.break_score;
    r.fakeAlignment.clear();
    r.fakeAlignment.score          = d.align.score;
    r.fakeAlignment.isJumped       = d.align.is_jumped != 0;
    r.fakeAlignment.align.beginPos = d.align.begin_pos1;
    detail::toPath(out.data() + d.align.cigar1_off, d.align.cigar1_len, r.fakeAlignment.align.apath);
    if (d.n_insert_segments) r.finish.segments.push_back(segment_t(d.seg_first, d.seg_last));
    r.finish.isFinished = d.is_finished != 0;
    r.finish.insertTrim.set_range(d.trim_begin, d.trim_end);
    r.finish.isFlankOK = d.is_flank_ok != 0;
  }
}

// ------------------------------------------------------------------------------------------------------
// spanning jump-alignment QC and contig selection (manta_spanning_select_batch) over the adapter types
// ------------------------------------------------------------------------------------------------------
/// The device half alone, on a spanning batch's own output handed back as it came (manta_spanning_batch / manta_spanning_download):
/// contigRecs[i] belongs to contigs[i], locusRecs[l] to loci[l].  A locus whose record carries a status was not decided: the caller
/// recomputes it with selectJumpContigDNA / selectJumpContigRNA.  cigarWords / bitsWords: what the arenas hold (the records' reach is
/// what is uploaded); bits may be nullptr unless isRNA.
inline void selectJumpContigBatch(
    manta_ctx_t* ctx, const AlignmentScores<int>& contigFilterScores, const bool isRNA, const uint32_t nLoci, const manta_asm_locus_result_t* loci,
    const manta_asm_contig_t* contigs, const manta_spanning_alignment_t* aligns, const uint32_t* cigar, const uint64_t cigarWords,
    const uint64_t* bits, const uint64_t bitsWords, std::vector<manta_spanning_select_contig_t>& contigRecs,
    std::vector<manta_spanning_select_t>& locusRecs)
{
  uint64_t nContigs = 0, cigarReach = 0, bitsReach = 0;
  for (uint32_t l = 0; l < nLoci; ++l) {
    if (loci[l].status != MANTA_OK) continue;
    nContigs = std::max<uint64_t>(nContigs, uint64_t(loci[l].first_contig) + loci[l].n_contigs);
    for (uint32_t c = 0; c < loci[l].n_contigs; ++c) {
      const uint64_t              i = uint64_t(loci[l].first_contig) + c;
      const manta_align_result_t& a(aligns[i].align);
      if (a.status == MANTA_OK) cigarReach = std::max<uint64_t>(cigarReach, std::max(a.cigar1_off + a.cigar1_len, a.cigar2_off + a.cigar2_len));
      if (isRNA) bitsReach = std::max<uint64_t>(bitsReach, contigs[i].support_off + loci[l].n_words);
    }
  }
  contigRecs.assign(nContigs, manta_spanning_select_contig_t());
  locusRecs.assign(nLoci, manta_spanning_select_t());
  if (nLoci == 0) return;
  if (!ctx) ctx = threadContext();
  const manta_align_scores_t sc = detail::toAbi(contigFilterScores);
  const int rc = manta_spanning_select_batch(ctx, &sc, isRNA ? 1 : 0, nLoci, loci, contigs, aligns, cigar, std::min(cigarReach, cigarWords), bits,
                                             std::min(bitsReach, bitsWords), contigRecs.data(), locusRecs.data());
  if (detail::selectCallFailed(rc, contigRecs, locusRecs))
    throw GeneralException("manta_amd spanning contig selection: " + std::string(manta_last_error(ctx)), rc);
}

/// one locus of the batch: its contigs' jump alignments and, for the RNA rule, the contigs themselves (supportReads; may be nullptr
/// otherwise)
struct JumpContigLocusInput {
  const std::vector<JumpAlignmentResult<int>>* alignments;
  const Assembly*                              contigs;
};

struct JumpContigSelection {
  int best         = -1;        ///< bestAlignmentIndex, -1: the static returned false
  int deviceStatus = MANTA_OK;  ///< != MANTA_OK: the host function computed this locus
};

inline int selectJumpContigHost(const AlignmentScores<int>& contigFilterScores, const bool isRNA, const JumpContigLocusInput& in)
{
  if (!isRNA) return selectJumpContigDNA(*in.alignments, contigFilterScores);
  std::vector<unsigned> support;
  for (const AssembledContig& c : *in.contigs) support.push_back(unsigned(c.supportReads.size()));
  return selectJumpContigRNA(*in.alignments, support, contigFilterScores);
}

/// selectJumpContigDNA / selectJumpContigRNA of every locus in ONE device call; a locus the device does not decide (any per-item
/// status) is recomputed by the host function and carries that status in deviceStatus.
inline void selectJumpContigBatch(
    const AlignmentScores<int>& contigFilterScores, const bool isRNA, const std::vector<JumpContigLocusInput>& items,
    std::vector<JumpContigSelection>& results, manta_ctx_t* ctx = nullptr)
{
  const size_t n = items.size();
  results.assign(n, JumpContigSelection());
  if (n == 0) return;
  std::vector<manta_asm_locus_result_t>   loci(n);
  std::vector<manta_asm_contig_t>         contigs;
  std::vector<manta_spanning_alignment_t> aligns;
  std::vector<uint32_t>                   cigar;
  std::vector<uint64_t>                   bits;
  for (size_t l = 0; l < n; ++l) {
    const std::vector<JumpAlignmentResult<int>>& ja(*items[l].alignments);
    loci[l]              = manta_asm_locus_result_t();
    loci[l].n_contigs    = uint32_t(ja.size());
    loci[l].first_contig = uint32_t(contigs.size());
    unsigned maxRead = 0;
    if (isRNA)
      for (const AssembledContig& c : *items[l].contigs)
        if (!c.supportReads.empty()) maxRead = std::max(maxRead, *c.supportReads.rbegin());
    loci[l].n_words = maxRead / 64 + 1;
    for (size_t c = 0; c < ja.size(); ++c) {
      manta_spanning_alignment_t a = manta_spanning_alignment_t();
      a.align.score            = ja[c].score;
      a.align.jump_insert_size = ja[c].jumpInsertSize;
      a.align.jump_range       = ja[c].jumpRange;
      a.align.begin_pos1       = ja[c].align1.beginPos;
      a.align.begin_pos2       = ja[c].align2.beginPos;
      a.align.cigar1_off       = cigar.size();
      detail::toPacked(ja[c].align1.apath, cigar);
      a.align.cigar1_len = uint32_t(cigar.size() - a.align.cigar1_off);
      a.align.cigar2_off = cigar.size();
      detail::toPacked(ja[c].align2.apath, cigar);
      a.align.cigar2_len = uint32_t(cigar.size() - a.align.cigar2_off);
      aligns.push_back(a);
      manta_asm_contig_t rec = manta_asm_contig_t();
      rec.support_off = bits.size();
      rec.reject_off  = bits.size() + loci[l].n_words;
      bits.resize(bits.size() + 2 * size_t(loci[l].n_words), 0);
      if (isRNA)
        for (const unsigned r : (*items[l].contigs)[c].supportReads) bits[rec.support_off + r / 64] |= uint64_t(1) << (r % 64);
      contigs.push_back(rec);
    }
  }
  const uint64_t cigarWords = cigar.size(), bitsWords = bits.size();
  cigar.push_back(0);
  bits.push_back(0);
  contigs.push_back(manta_asm_contig_t());
  aligns.push_back(manta_spanning_alignment_t());
  std::vector<manta_spanning_select_contig_t> contigRecs;
  std::vector<manta_spanning_select_t>        locusRecs;
  selectJumpContigBatch(ctx, contigFilterScores, isRNA, uint32_t(n), loci.data(), contigs.data(), aligns.data(), cigar.data(), cigarWords, bits.data(),
                        bitsWords, contigRecs, locusRecs);
  for (size_t l = 0; l < n; ++l) {
    if (locusRecs[l].status == MANTA_OK) {
      results[l].best = locusRecs[l].selected ? locusRecs[l].best_contig : -1;
    } else {
      results[l].best         = selectJumpContigHost(contigFilterScores, isRNA, items[l]);
      results[l].deviceStatus = locusRecs[l].status;
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// small-SV contig ranking and refined candidate ranges (manta_smallsv_select_batch) over the adapter types
// ------------------------------------------------------------------------------------------------------
/// The device half alone, on a small-SV batch's own output and its QC records handed back as they came (manta_smallsv_batch /
/// manta_smallsv_download, manta_smallsv_qc_batch / manta_smallsv_download_qc): locusRecs[l] belongs to loci[l], its candidates are
/// candRecs[cand_off, cand_off + n_candidates).  A locus whose record carries a status was not decided: the caller recomputes it with
/// selectSmallSVContig / smallCandSVRanges.  The *Used arguments: what of every arena was used.
inline void selectSmallSVContigBatch(
    manta_ctx_t* ctx, const uint32_t nLoci, const manta_asm_locus_result_t* loci, const manta_asm_contig_t* contigs,
    const manta_smallsv_alignment_t* aligns, const manta_smallsv_qc_t* qc, const uint32_t* segs, const uint64_t segPairsUsed, const uint8_t* seq,
    const uint64_t seqUsed, const uint32_t* cigar, const uint64_t cigarUsed, const uint64_t* bits, const uint64_t bitsUsed, const uint8_t* refs,
    const uint64_t* refOff, std::vector<manta_smallsv_select_t>& locusRecs, std::vector<manta_small_cand_sv_t>& candRecs)
{
  locusRecs.assign(nLoci, manta_smallsv_select_t());
  if (candRecs.size() < 32 * size_t(nLoci)) candRecs.resize(32 * size_t(nLoci));
  if (nLoci == 0) return;
  if (!ctx) ctx = threadContext();
  uint64_t  used = 0;
  const int rc   = manta_smallsv_select_batch(ctx, nLoci, loci, contigs, aligns, qc, segs, segPairsUsed, seq, seqUsed, cigar, cigarUsed, bits, bitsUsed,
                                              refs, refOff, locusRecs.data(), candRecs.data(), candRecs.size(), &used);
  if (detail::smallSelectCallFailed(rc, locusRecs))
    throw GeneralException("manta_amd small-SV contig selection: " + std::string(manta_last_error(ctx)), rc);
}

/// one locus of the batch: its contigs, their GlobalLargeIndelAligner alignments (beginPos in window coordinates), the contigs' QC
/// results (findSmallSVCandidateSegments' return value and merged candidateSegments, one per contig) and the uncut reference window
struct SmallSVSelectLocusInput {
  const Assembly*                            contigs;
  const std::vector<AlignmentResult<int>>*   alignments;
  const std::vector<char>*                   isCandidate;
  const std::vector<std::vector<segment_t>>* candidateSegments;
  const std::string*                         refSeq;
};

struct SmallSVSelection {
  SmallSVContigChoice            choice;
  std::vector<segment_t>         segments;    ///< of choice.best: one refined candidate each
  std::vector<SmallCandSVRanges> candidates;  ///< refRange in window coordinates
  int                            deviceStatus = MANTA_OK;  ///< != MANTA_OK: the host functions computed this locus
};

/// the same on the host: the free functions of refiner_util.hpp
inline void selectSmallSVContigHost(const SmallSVSelectLocusInput& in, SmallSVSelection& r)
{
  std::vector<SmallSVContigFacts> facts;
  for (unsigned c = 0; c < in.alignments->size(); ++c) {
    if (!(*in.isCandidate)[c]) continue;
    SmallSVContigFacts f;
    f.index            = c;
    f.score            = (*in.alignments)[c].score;
    f.isJumped         = (*in.alignments)[c].isJumped;
    f.variantSize      = getLargestIndelSize((*in.alignments)[c].align.apath, (*in.candidateSegments)[c]);
    f.supportReadCount = unsigned((*in.contigs)[c].supportReads.size());
    facts.push_back(f);
  }
  r.choice = selectSmallSVContig(facts);
  r.segments.clear();
  r.candidates.clear();
  if (r.choice.best < 0) return;
  const size_t b = size_t(r.choice.best);
  r.segments = (*in.candidateSegments)[b];
  for (const segment_t& seg : r.segments) r.candidates.push_back(smallCandSVRanges(*in.refSeq, (*in.contigs)[b].seq, (*in.alignments)[b].align, seg));
}

/// selectSmallSVContig and smallCandSVRanges of every locus in ONE device call; a locus the device does not decide (any per-item
/// status) is recomputed by the host functions and carries that status in deviceStatus.
inline void selectSmallSVContigBatch(const std::vector<SmallSVSelectLocusInput>& items, std::vector<SmallSVSelection>& results, manta_ctx_t* ctx = nullptr)
{
  const size_t n = items.size();
  results.assign(n, SmallSVSelection());
  if (n == 0) return;
  std::vector<manta_asm_locus_result_t>  loci(n);
  std::vector<manta_asm_contig_t>        contigs;
  std::vector<manta_smallsv_alignment_t> aligns;
  std::vector<manta_smallsv_qc_t>        qc;
  std::vector<uint8_t>                   seq, refs;
  std::vector<uint32_t>                  cigar, segs;
  std::vector<uint64_t>                  bits, refOff(n + 1, 0);
  for (size_t l = 0; l < n; ++l) {
    const SmallSVSelectLocusInput& in(items[l]);
    loci[l]              = manta_asm_locus_result_t();
    loci[l].n_contigs    = uint32_t(in.alignments->size());
    loci[l].first_contig = uint32_t(contigs.size());
    unsigned maxRead = 0;
    for (const AssembledContig& c : *in.contigs)
      if (!c.supportReads.empty()) maxRead = std::max(maxRead, *c.supportReads.rbegin());
    loci[l].n_words = maxRead / 64 + 1;
    for (size_t c = 0; c < in.alignments->size(); ++c) {
      const AlignmentResult<int>& ar((*in.alignments)[c]);
      const std::string&          text((*in.contigs)[c].seq);
      manta_smallsv_alignment_t   a = manta_smallsv_alignment_t();
      a.align.score      = ar.score;
      a.align.is_jumped  = ar.isJumped ? 1 : 0;
      a.align.begin_pos1 = ar.align.beginPos;
      a.align.cigar1_off = cigar.size();
      detail::toPacked(ar.align.apath, cigar);
      a.align.cigar1_len = uint32_t(cigar.size() - a.align.cigar1_off);
      aligns.push_back(a);
      manta_asm_contig_t rec = manta_asm_contig_t();
      rec.seq_off     = seq.size();
      rec.seq_len     = uint32_t(text.size());
      rec.support_off = bits.size();
      rec.reject_off  = bits.size() + loci[l].n_words;
      seq.insert(seq.end(), text.begin(), text.end());
      bits.resize(bits.size() + 2 * size_t(loci[l].n_words), 0);
      for (const unsigned r : (*in.contigs)[c].supportReads) bits[rec.support_off + r / 64] |= uint64_t(1) << (r % 64);
      contigs.push_back(rec);
      manta_smallsv_qc_t q = manta_smallsv_qc_t();
      q.is_candidate  = (*in.isCandidate)[c] ? 1u : 0u;
      q.n_segments    = uint32_t((*in.candidateSegments)[c].size());
      q.largest_indel = getLargestIndelSize(ar.align.apath, (*in.candidateSegments)[c]);
      q.seg_off       = segs.size() / 2;
      for (const segment_t& sg : (*in.candidateSegments)[c]) {
        segs.push_back(sg.first);
        segs.push_back(sg.second);
      }
      qc.push_back(q);
    }
    refs.insert(refs.end(), in.refSeq->begin(), in.refSeq->end());
    refOff[l + 1] = refs.size();
  }
  const uint64_t seqUsed = seq.size(), cigarUsed = cigar.size(), bitsUsed = bits.size(), segPairs = segs.size() / 2;
  seq.push_back(0);
  refs.push_back(0);
  cigar.push_back(0);
  bits.push_back(0);
  segs.push_back(0);
  contigs.push_back(manta_asm_contig_t());
  aligns.push_back(manta_smallsv_alignment_t());
  qc.push_back(manta_smallsv_qc_t());
  std::vector<manta_smallsv_select_t> locusRecs;
  std::vector<manta_small_cand_sv_t>  candRecs;
  selectSmallSVContigBatch(ctx, uint32_t(n), loci.data(), contigs.data(), aligns.data(), qc.data(), segs.data(), segPairs, seq.data(), seqUsed,
                           cigar.data(), cigarUsed, bits.data(), bitsUsed, refs.data(), refOff.data(), locusRecs, candRecs);
  for (size_t l = 0; l < n; ++l) {
    SmallSVSelection&             r(results[l]);
    const manta_smallsv_select_t& d(locusRecs[l]);
    if (d.status != MANTA_OK) {
      selectSmallSVContigHost(items[l], r);
      r.deviceStatus = d.status;
      continue;
    }
    r.choice.rank1       = d.rank1_contig;
    r.choice.rank2       = d.rank2_contig;
    r.choice.rank2IsBest = d.rank2_is_best != 0;
    r.choice.best        = d.selected ? d.best_contig : -1;
    for (uint32_t k = 0; k < d.n_candidates; ++k) {
      const manta_small_cand_sv_t& c(candRecs[d.cand_off + k]);
      SmallCandSVRanges            ranges;
      ranges.refRange.set_range(c.ref_begin, c.ref_end);
      ranges.readRange.set_range(c.read_begin, c.read_end);
      ranges.cipos.set_range(c.cipos_begin, c.cipos_end);
      r.segments.emplace_back(c.seg_first, c.seg_last);
      r.candidates.push_back(ranges);
    }
  }
}

}  // namespace manta_amd
