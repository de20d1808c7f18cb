// Test-only: the C surface of host_refiner_full_capi.cpp (the product's SVCandidateAssemblyRefiner behind the reference driver's POD
// interface) plus what tests/test_smallsv_select.py needs of the device contig ranking: the host restatement of a candidate's ranges
// (smallCandSVRanges), the ranking of constructed loci by the free host functions or by the adapter selectSmallSVContigBatch,
// setSmallCandSV on either's ranges, and the batched refiner call with the switches given.
#include "host_refiner_full_capi.cpp"

#include "contig_qc.hpp"

namespace {
std::vector<segment_t> segmentsOf(const char* text)  // "first-last,first-last,..."
{
  std::vector<segment_t> out;
  std::istringstream     is(text);
  std::string            item;
  while (std::getline(is, item, ',')) {
    const size_t dash = item.find('-');
    out.emplace_back(unsigned(std::stoul(item.substr(0, dash))), unsigned(std::stoul(item.substr(dash + 1))));
  }
  return out;
}

void dumpRanges(std::ostream& os, const segment_t& seg, const SmallCandSVRanges& r)
{
  os << seg.first << "-" << seg.second << " " << r.refRange.begin_pos() << " " << r.refRange.end_pos() << " " << r.readRange.begin_pos() << " "
     << r.readRange.end_pos() << " " << r.cipos.begin_pos() << " " << r.cipos.end_pos();
}
}  // namespace

/// smallCandSVRanges (refiner_util.hpp) of one task -> out[0..5]: ref_begin, ref_end, read_begin, read_end, cipos_begin, cipos_end
MINE_EXPORT int mine_small_cand_sv_ranges(const char* ref, const char* contig, int beginPos, const char* cigar, unsigned first, unsigned last, int* out)
{
  Alignment align;
  align.beginPos = beginPos;
  align.apath    = ALIGNPATH::cigar_to_apath(cigar);
  const SmallCandSVRanges r(smallCandSVRanges(ref, contig, align, segment_t(first, last)));
  out[0] = r.refRange.begin_pos();
  out[1] = r.refRange.end_pos();
  out[2] = r.readRange.begin_pos();
  out[3] = r.readRange.end_pos();
  out[4] = r.cipos.begin_pos();
  out[5] = r.cipos.end_pos();
  return 0;
}

/// The ranking of n loci given as text, contigs flattened over the loci (nContigs[l] of them each): per contig its text, begin
/// position, path, score, isJumped, the QC's verdict and merged segment list ("first-last,...") and its support reads ("r,r,...").
/// use_device == 0: selectSmallSVContigHost; 1: the adapter selectSmallSVContigBatch.  Per locus one line
///   "<device status> <rank1> <rank2> <rank2IsBest> <best>|<first>-<last> <refRange> <readRange> <cipos>|..."
MINE_EXPORT int mine_select_small_sv_loci(
    int n, const int* nContigs, const char* const* windows, const char* const* seqs, const int* beginPos, const char* const* cigars,
    const int* scores, const int* jumped, const int* isCandidate, const char* const* segments, const char* const* support, int use_device,
    char* out, int cap)
{
  try {
    std::vector<Assembly>                            contigs(n);
    std::vector<std::vector<AlignmentResult<int>>>   aligns(n);
    std::vector<std::vector<char>>                   cand(n);
    std::vector<std::vector<std::vector<segment_t>>> segs(n);
    std::vector<std::string>                         refs(n);
    std::vector<SmallSVSelectLocusInput>             items(n);
    int                                              at = 0;
    for (int l = 0; l < n; ++l) {
      refs[l] = windows[l];
      contigs[l].resize(nContigs[l]);
      aligns[l].resize(nContigs[l]);
      for (int c = 0; c < nContigs[l]; ++c, ++at) {
        contigs[l][c].seq = seqs[at];
        std::istringstream is(support[at]);
        std::string        item;
        while (std::getline(is, item, ',')) contigs[l][c].supportReads.insert(unsigned(std::stoul(item)));
        aligns[l][c].score          = scores[at];
        aligns[l][c].isJumped       = jumped[at] != 0;
        aligns[l][c].align.beginPos = beginPos[at];
        aligns[l][c].align.apath    = ALIGNPATH::cigar_to_apath(cigars[at]);
        cand[l].push_back(isCandidate[at] ? 1 : 0);
        segs[l].push_back(segmentsOf(segments[at]));
      }
      items[l] = SmallSVSelectLocusInput{&contigs[l], &aligns[l], &cand[l], &segs[l], &refs[l]};
    }
    std::vector<SmallSVSelection> res(n);
    if (use_device) {
      selectSmallSVContigBatch(items, res);
    } else {
      for (int l = 0; l < n; ++l) selectSmallSVContigHost(items[l], res[l]);
    }
    std::ostringstream os;
    for (int l = 0; l < n; ++l) {
      const SmallSVSelection& r(res[l]);
      os << r.deviceStatus << " " << r.choice.rank1 << " " << r.choice.rank2 << " " << int(r.choice.rank2IsBest) << " " << r.choice.best;
      for (size_t k = 0; k < r.candidates.size(); ++k) {
        os << "|";
        dumpRanges(os, r.segments[k], r.candidates[k]);
      }
      os << "\n";
    }
    return emit(os.str(), out, cap);
  } catch (const std::exception& e) {
    return emit(std::string("EXCEPTION ") + e.what(), out, cap);
  }
}

/// setSmallCandSV (refiner.hpp) on one constructed candidate, as the refiner calls it with the switch off (use_device == 0: the ranges
/// of smallCandSVRanges) and on (1: the ranges of the device record, through selectSmallSVContigBatch on a locus of this one contig)
/// -> the candidate as text, or "EXCEPTION <message>"
MINE_EXPORT int mine_set_small_cand_sv(
    const char* window, int offset, const char* contig, int beginPos, const char* cigar, unsigned first, unsigned last, int use_device, char* out, int cap)
{
  try {
    reference_contig_segment ref;
    ref.seq() = window;
    ref.set_offset(offset);
    Alignment align;
    align.beginPos = beginPos;
    align.apath    = ALIGNPATH::cigar_to_apath(cigar);
    const segment_t seg(first, last);
    GSCOptions      options;
    SVCandidate     sv;
    if (use_device) {
      Assembly                            contigs(1);
      std::vector<AlignmentResult<int>>   aligns(1);
      std::vector<char>                   cand(1, 1);
      std::vector<std::vector<segment_t>> segs(1, std::vector<segment_t>(1, seg));
      contigs[0].seq  = contig;
      aligns[0].align = align;
      std::vector<SmallSVSelectLocusInput> items(1, SmallSVSelectLocusInput{&contigs, &aligns, &cand, &segs, &ref.seq()});
      std::vector<SmallSVSelection>        res;
      selectSmallSVContigBatch(items, res);
      if (res[0].deviceStatus != MANTA_OK || res[0].candidates.size() != 1) return emit("NOT DECIDED " + std::to_string(res[0].deviceStatus), out, cap);
      detail::setSmallCandSV(ref, contig, align, res[0].segments[0], res[0].candidates[0], sv, options);
    } else {
      detail::setSmallCandSV(ref, contig, align, seg, sv, options);
    }
    std::ostringstream os;
    os << "bp1 " << sv.bp1.interval.range.begin_pos() << " " << sv.bp1.interval.range.end_pos() << " bp2 " << sv.bp2.interval.range.begin_pos() << " "
       << sv.bp2.interval.range.end_pos() << " ins " << sv.insertSeq << " cigar " << ALIGNPATH::apath_to_cigar(sv.insertAlignment);
    return emit(os.str(), out, cap);
  } catch (const std::exception& e) {
    return emit(std::string("EXCEPTION ") + e.what(), out, cap);
  }
}

/// mine_get_candidate_assembly_data_multi's one batched call (is_batched == 1) on a refiner with setDeviceContigQC(device_qc) and
/// setDeviceSmallSelect(device_select); counters: small-SV loci, loci whose ranking the device decided, loci it left to the host
/// functions, contigs whose QC fell back
MINE_EXPORT int mine_get_candidate_assembly_data_batch_small_select(const ref_refine_input_t* inputs, int n, int device_qc, int device_select,
                                                                    uint64_t* counters, char* out, int cap)
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
    refiner.setDeviceContigQC(device_qc != 0);
    refiner.setDeviceSmallSelect(device_select != 0);
    std::vector<SVCandidateAssemblyData> data;
    refiner.getCandidateAssemblyDataBatch(svs, inputs[0].is_find_large_insertions != 0, data);
    std::string text;
    for (const auto& d : data) text += dumpAssemblyData(d);
    counters[0] = refiner.stats().smallLoci;
    counters[1] = refiner.stats().deviceSmallSelectLoci;
    counters[2] = refiner.stats().deviceSmallSelectFallbacks;
    counters[3] = refiner.stats().deviceQCFallbacks;
    return emit(text, out, cap);
  } catch (const std::exception& e) {
    return emit(std::string("EXCEPTION ") + e.what(), out, cap);
  }
}
