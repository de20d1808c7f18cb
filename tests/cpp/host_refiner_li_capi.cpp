// Test-only: the C surface of host_refiner_full_capi.cpp (the product's SVCandidateAssemblyRefiner behind the reference driver's POD
// interface) plus what tests/test_large_insertion.py needs of the device large-insertion search: the host restatement of an edge
// record, the search of constructed loci by the free host functions or by the adapter findLargeInsertionBatch, and the batched refiner
// call with the switch given.
#include "host_refiner_full_capi.cpp"

#include "contig_qc.hpp"

namespace {
AlignmentScores<int> liScores(const int32_t* s) { return AlignmentScores<int>(s[0], s[1], s[2], s[3], s[4], s[5] != 0); }

std::string pathText(const ALIGNPATH::path_t& path)
{
  static const char  name[] = "?MIDNSHP=X";
  std::ostringstream os;
  for (const ALIGNPATH::path_segment& ps : path) os << ps.length << name[ps.type];
  return os.str();
}
}  // namespace

/// isLargeInsertionEdge (refiner_util.hpp) of one path -> out[0..5]: is_candidate, is_left, is_right, contig_offset, ref_offset, score
/// (all 0 when it is no candidate, as the cleared LargeInsertionInfo)
MINE_EXPORT int mine_large_insertion_edge(const int32_t* scores, const char* cigar, int consBegin, int consEnd, int* out)
{
  LargeInsertionInfo info;
  const bool         r = isLargeInsertionEdge(liScores(scores), ALIGNPATH::cigar_to_apath(cigar), consBegin, consEnd, info);
  out[0] = r;
  out[1] = info.isLeftCandidate;
  out[2] = info.isRightCandidate;
  out[3] = int(info.contigOffset);
  out[4] = int(info.refOffset);
  out[5] = info.score;
  return r;
}

/// The search of n loci given as text, contigs flattened over the loci (nContigs[l] of them each).  use_device == 0: the free host
/// functions plus manta_align_batch (findLargeInsertionHost); 1: the adapter findLargeInsertionBatch.  Per locus one line
///   "<device status> <isPair> <left> <right> <dist> <score> | <align score> <beginPos> <cigar> | <n segments> <first> <last> <isFinished>
///    <trim begin> <trim end> <isFlankOK> | <candidate contigs: index:left:right:contigOffset:refOffset:score ...>"
MINE_EXPORT int mine_large_insertion_loci(
    const int32_t* edgeScores, const int32_t* completeScores, int n, const int* nContigs, const char* const* contigSeqs, const int* beginPos,
    const char* const* cigars, const int* consBegin, const int* consEnd, const char* const* refs, const int* lead, const int* trail, int use_device,
    char* out, int cap)
{
  try {
    const AlignmentScores<int>            esc(liScores(edgeScores)), csc(liScores(completeScores));
    std::vector<Assembly>                 contigs(n);
    std::vector<std::vector<Alignment>>   aligns(n);
    std::vector<std::string>              refSeqs(n);
    std::vector<LargeInsertionLocusInput> items(n);
    int                                   at = 0;
    for (int l = 0; l < n; ++l) {
      contigs[l].resize(nContigs[l]);
      aligns[l].resize(nContigs[l]);
      for (int c = 0; c < nContigs[l]; ++c, ++at) {
        contigs[l][c].seq = contigSeqs[at];
        contigs[l][c].conservativeRange.set_range(consBegin[at], consEnd[at]);
        aligns[l][c].beginPos = beginPos[at];
        aligns[l][c].apath    = ALIGNPATH::cigar_to_apath(cigars[at]);
      }
      refSeqs[l] = refs[l];
      items[l]   = LargeInsertionLocusInput{&contigs[l], &aligns[l], &refSeqs[l], lead[l], trail[l]};
    }
    std::vector<LargeInsertionLocusResult> res(n);
    if (use_device) {
      findLargeInsertionBatch(esc, csc, items, res);
    } else {
      for (int l = 0; l < n; ++l) findLargeInsertionHost(esc, csc, items[l], res[l], threadContext());
    }
    std::ostringstream os;
    for (int l = 0; l < n; ++l) {
      const LargeInsertionLocusResult& r(res[l]);
      os << r.deviceStatus << " " << int(r.pair.isPair) << " " << r.pair.leftIndex << " " << r.pair.rightIndex << " " << r.pair.breakDist << " "
         << r.pair.breakScore << " | " << r.fakeAlignment.score << " " << r.fakeAlignment.align.beginPos << " "
         << pathText(r.fakeAlignment.align.apath) << " | " << r.finish.segments.size() << " "
         << (r.finish.segments.empty() ? 0u : r.finish.segments[0].first) << " " << (r.finish.segments.empty() ? 0u : r.finish.segments[0].second)
         << " " << int(r.finish.isFinished) << " " << r.finish.insertTrim.begin_pos() << " " << r.finish.insertTrim.end_pos() << " "
         << int(r.finish.isFlankOK) << " |";
      for (const unsigned i : r.candIndex)
        os << " " << i << ":" << int(r.info[i].isLeftCandidate) << ":" << int(r.info[i].isRightCandidate) << ":" << r.info[i].contigOffset << ":"
           << r.info[i].refOffset << ":" << r.info[i].score;
      os << "\n";
    }
    return emit(os.str(), out, cap);
  } catch (const std::exception& e) {
    return emit(std::string("EXCEPTION ") + e.what(), out, cap);
  }
}

/// mine_get_candidate_assembly_data_multi's one batched call (is_batched == 1) on a refiner with setDeviceLargeInsertion(device_li);
/// counters: large-insertion alignments, loci whose search the device decided, loci it left to the host functions
MINE_EXPORT int mine_get_candidate_assembly_data_batch_li(const ref_refine_input_t* inputs, int n, int device_li, uint64_t* counters, char* out, int cap)
{
  try {
    MemorySource    source;
    bam_header_info header;
    for (int i = 0; i < inputs[0].n_chrom; ++i) {
      source.chroms.emplace_back(inputs[0].chrom_seq[i]);
      header.chrom_data.emplace_back(std::to_string(i).c_str(), unsigned(source.chroms.back().size()));
    }
    GSCOptions options;
    setOptions(inputs[0], options);
    std::vector<SVCandidate> svs;
    for (int k = 0; k < n; ++k) {
      const ref_refine_input_t& in(inputs[k]);
      MemorySource::Pile        pile;
      pile.tid = in.bp_tid[0];
      pile.pos = in.bp_begin[0];
      for (int i = 0; i < in.n_reads; ++i) pile.reads.emplace_back(in.reads[i]);
      source.piles.push_back(pile);
      for (int c = 0; c < std::max(1, in.n_calls); ++c) svs.push_back(makeSV(in));
    }
    SVCandidateAssemblyRefiner refiner(options, header, source);
    refiner.setDeviceLargeInsertion(device_li != 0);
    std::vector<SVCandidateAssemblyData> data;
    refiner.getCandidateAssemblyDataBatch(svs, inputs[0].is_find_large_insertions != 0, data);
    std::string text;
    for (const auto& d : data) text += dumpAssemblyData(d);
    counters[0] = refiner.stats().largeInsertionAlignments;
    counters[1] = refiner.stats().deviceLargeInsertionLoci;
    counters[2] = refiner.stats().deviceLargeInsertionFallbacks;
    return emit(text, out, cap);
  } catch (const std::exception& e) {
    return emit(std::string("EXCEPTION ") + e.what(), out, cap);
  }
}
