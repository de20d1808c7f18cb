// The reference's GlobalJumpIntronAligner test vectors through manta_amd::GlobalJumpIntronAligner<int> of manta_amd/host/manta_amd.hpp: reads one
// case per line from stdin (match mismatch open extend offEdge jump intronOpen intronOffEdge ref1Fw ref2Fw stranded query ref1 ref2) and
// prints the result in the layout of tests/golden/intron_aligner_reference_tests.json's ref_text; tests/test_intron_adapter.py compares.
// Linked against libmanta_amd.so (GPU) or tests/emu/libmanta_amd_emu.so (CPU tier).
#include <iostream>
#include <string>

#include "../../manta_amd/host/manta_amd.hpp"

using namespace manta_amd;

int main()
{
  int         s[8], f[3];
  std::string q, r1, r2;
  // the constructor refuses isAllowEdgeInsertion, as the reference's asserts
  try {
    GlobalJumpIntronAligner<int> bad(AlignmentScores<int>(2, -8, -19, -1, -1, true), -100, -15, -1);
    std::cout << "constructor accepted isAllowEdgeInsertion\n";
    return 1;
  } catch (const GeneralException&) {
  }
  while (std::cin >> s[0] >> s[1] >> s[2] >> s[3] >> s[4] >> s[5] >> s[6] >> s[7] >> f[0] >> f[1] >> f[2] >> q >> r1 >> r2) {
    const AlignmentScores<int>         scores(s[0], s[1], s[2], s[3], s[4]);
    const GlobalJumpIntronAligner<int> aligner(scores, s[5], s[6], s[7]);
    JumpAlignmentResult<int>           result;
    aligner.align(q.begin(), q.end(), r1.begin(), r1.end(), r2.begin(), r2.end(), f[0] != 0, f[1] != 0, f[2] != 0, result);
    std::cout << "score " << result.score << " align1 " << result.align1.beginPos << ":" << ALIGNPATH::apath_to_cigar(result.align1.apath)
              << " align2 " << result.align2.beginPos << ":" << ALIGNPATH::apath_to_cigar(result.align2.apath) << " jumpInsertSize "
              << result.jumpInsertSize << " jumpRange " << result.jumpRange << "\n";
  }
  // an empty reference2 is the reference's own exception
  try {
    const GlobalJumpIntronAligner<int> aligner(AlignmentScores<int>(2, -8, -19, -1, -1), -100, -15, -1);
    JumpAlignmentResult<int>           result;
    const std::string                  a("ACGT"), e;
    aligner.align(a.begin(), a.end(), a.begin(), a.end(), e.begin(), e.end(), true, true, true, result);
    std::cout << "empty reference2 accepted\n";
    return 1;
  } catch (const GeneralException&) {
  }
  return 0;
}
