// What bamio.hip (host: BGZF + BAM reader) and bam.hip (device: name ranking, CSC build) share: the handle behind
// the gbrs_bam_* calls.  No HIP type appears here, so that bamio.hip also compiles as plain C++.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

struct gbrs_bam {
    std::string path;
    int threads = 0;
    // header
    std::vector<std::string> ref_names;
    std::vector<uint32_t> ref_len;
    // reference -> (haplotype, locus); hap == BAM_REF_UNUSABLE marks a reference no kept record may use, and
    // its locus slot then holds the reason (BAM_REF_*)
    bool map_set = false;
    uint32_t num_haps = 0, num_loci = 0;
    std::vector<uint32_t> ref_hap, ref_locus;
    // collected by the host pass (gbrs::bam_collect)
    struct Rec { uint32_t cand; int32_t refid; };       // kept records only, file order
    std::vector<Rec> recs;
    std::vector<unsigned char> cand_bytes;              // the candidates' names one after another, no terminators
    std::vector<uint64_t> cand_off;                     // [n_cand + 1]
    uint32_t max_name = 0;
    // results of the device pass: sizes and the column pointers here, the index and name arrays stay on the device
    // (owned by bam.hip behind `dev`) until gbrs_bam_get has copied them into the caller's buffers
    bool converted = false;
    uint64_t num_reads = 0;
    uint32_t name_width = 1;
    std::vector<uint64_t> col_ptr;                      // [H * L + 1] into the device's index array
    void *dev = nullptr;
    void (*dev_free)(void *) = nullptr;
};

namespace gbrs {

constexpr uint32_t BAM_REF_UNUSABLE = 0xFFFFFFFFu;
enum { BAM_REF_NOT_TWO_PARTS = 1, BAM_REF_UNKNOWN_HAPLOTYPE = 2, BAM_REF_UNKNOWN_LOCUS = 3 };

// One pass over the file: every record's name becomes (or reuses) a candidate, kept records are appended to recs.
int bam_collect(gbrs_bam *b);
void bam_release_collected(gbrs_bam *b);

}  // namespace gbrs
