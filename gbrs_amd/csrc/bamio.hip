// Host-side BAM reader of `gbrs bam2emase` (no device code): BGZF blocks inflated on a few threads, the BAM
// header and the record chain parsed from the inflated stream in bounded batches.
//
// BGZF (SAM/BAM specification, section 4.1): a file is a series of gzip members of at most 64 KiB each; the
// extra field of every member header carries the subfield 'B','C' with BSIZE = member size - 1, so the chain of
// members can be walked without inflating anything, and the members inflate independently.  Each member ends
// with the CRC-32 and the size (ISIZE) of its plain bytes; both are checked.
//
// BAM (section 4.2): magic "BAM\1", the header text, the reference sequences (name, length), then records
// `block_size, refID, pos, l_read_name, mapq, bin, n_cigar_op, flag, l_seq, next_refID, next_pos, tlen,
// read_name, ...`.  Records and even their 4-byte length fields cross member boundaries.  Only refID, flag and
// the name are looked at.
//
// The inflated stream is never held whole: a batch of members (at most BATCH_BLOCKS, 64 MiB of plain bytes) is
// inflated while the previous one is parsed, and what a batch leaves unfinished (the head of one record) is
// carried over.
#ifdef GBRS_HOST_ONLY
// CPU-only build for the AddressSanitizer / UBSan test (tests/test_bam_sanitizers.py); the test driver
// supplies gbrs::fail.
#include <cstdarg>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/gbrs_hip.h"
namespace gbrs { int fail(int status, const char *fmt, ...); }
#define GBRS_TRY(expr)                   \
    do {                                 \
        int s__ = (expr);                \
        if (s__ != GBRS_OK) return s__;  \
    } while (0)
#else
#include "common.h"
#endif

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <cstdio>
#include <future>
#include <new>
#include <thread>

#include "bamio.h"
#include "inflate.h"

namespace gbrs {
namespace {

constexpr size_t BATCH_BLOCKS = 1024;          // x 64 KiB = at most 64 MiB of plain bytes per batch
constexpr uint32_t MAX_ISIZE = 65536;          // the format's limit for one member's plain bytes

struct MappedFile {
    const unsigned char *p = nullptr;
    size_t len = 0;
    int open_path(const char *path) {
        const int fd = open(path, O_RDONLY);
        if (fd < 0) return fail(GBRS_ERR_INVALID, "cannot open %s", path);
        struct stat st;
        if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) { close(fd); return fail(GBRS_ERR_INVALID, "%s is not a regular file", path); }
        len = (size_t)st.st_size;
        if (len == 0) { close(fd); return fail(GBRS_ERR_INVALID, "%s is empty: not a BGZF/BAM file", path); }
        void *m = mmap(nullptr, len, PROT_READ, MAP_PRIVATE, fd, 0);
        close(fd);
        if (m == MAP_FAILED) return fail(GBRS_ERR_INVALID, "cannot map %s", path);
        p = (const unsigned char *)m;
        (void)madvise(m, len, MADV_SEQUENTIAL);
        return GBRS_OK;
    }
    ~MappedFile() { if (p) munmap((void *)p, len); }
    MappedFile() = default;
    MappedFile(const MappedFile &) = delete;
    MappedFile &operator=(const MappedFile &) = delete;
};

struct Block { uint64_t cdata, out_off; uint32_t clen, isize, crc; };

// Walks the BSIZE chain and inflates batch after batch.
struct BgzfStream {
    const MappedFile &f;
    const char *path;
    unsigned nt;
    uint64_t pos = 0, block_no = 0;
    // next() also runs on a read-ahead thread, and the library's error text is per thread: the message is kept here
    // and reported by the thread that drives the parse
    char err[512] = "";
    int note(int status, const char *fmt, ...) __attribute__((format(printf, 3, 4))) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, sizeof(err), fmt, ap);
        va_end(ap);
        return status;
    }
    BgzfStream(const MappedFile &f_, const char *path_, int threads) : f(f_), path(path_) {
        unsigned n = threads > 0 ? (unsigned)threads : std::thread::hardware_concurrency();
        if (const char *e = std::getenv("GBRS_IO_THREADS"); threads <= 0 && e && std::atoi(e) > 0) n = (unsigned)std::atoi(e);
        nt = std::max(1u, std::min(n, 16u));
    }
    bool at_end() const { return pos >= f.len; }

    // next batch -> out (resized to the batch's plain size); GBRS_OK with an empty `out` is possible (empty members)
    int next(std::vector<unsigned char> &out) {
        std::vector<Block> blocks;
        uint64_t total = 0;
        while (blocks.size() < BATCH_BLOCKS && pos < f.len) {
            const uint64_t left = f.len - pos;
            const unsigned char *h = f.p + pos;
            if (left < 18) return note(GBRS_ERR_INVALID, "%s: truncated BGZF block header at offset %llu", path, (unsigned long long)pos);
            if (h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4))
                return note(GBRS_ERR_INVALID, "%s: not a BGZF file (no gzip member with an extra field at offset %llu)", path,
                            (unsigned long long)pos);
            const uint32_t xlen = rd16(h + 10);
            if (left < 12 + (uint64_t)xlen) return note(GBRS_ERR_INVALID, "%s: truncated BGZF block header at offset %llu", path, (unsigned long long)pos);
            int64_t bsize = -1;
            for (uint32_t at = 0; at + 4 <= xlen;) {
                const unsigned char *x = h + 12 + at;
                const uint32_t slen = rd16(x + 2);
                if (at + 4 + slen > xlen) break;
                if (x[0] == 'B' && x[1] == 'C' && slen == 2) { bsize = rd16(x + 4); break; }
                at += 4 + slen;
            }
            if (bsize < 0) return note(GBRS_ERR_INVALID, "%s: not a BGZF file (gzip member without the BC subfield at offset %llu)", path, (unsigned long long)pos);
            const uint64_t member = (uint64_t)bsize + 1;
            if (member < 12 + (uint64_t)xlen + 8)
                return note(GBRS_ERR_INVALID, "%s: BGZF block %llu: BSIZE %lld is smaller than its own header and trailer", path,
                            (unsigned long long)block_no, (long long)bsize);
            if (member > left)
                return note(GBRS_ERR_INVALID, "%s: truncated BGZF block %llu at offset %llu (%llu bytes wanted, %llu left)", path,
                            (unsigned long long)block_no, (unsigned long long)pos, (unsigned long long)member, (unsigned long long)left);
            Block b;
            b.cdata = pos + 12 + xlen;
            b.clen = (uint32_t)(member - 12 - xlen - 8);
            b.crc = rd32(h + member - 8);
            b.isize = rd32(h + member - 4);
            if (b.isize > MAX_ISIZE)
                return note(GBRS_ERR_INVALID, "%s: BGZF block %llu claims %u plain bytes (the format allows 65536)", path,
                            (unsigned long long)block_no, b.isize);
            b.out_off = total;
            total += b.isize;
            blocks.push_back(b);
            pos += member;
            ++block_no;
        }
        out.resize(total);
        const Inflaters &inf = inflaters();
        if (total && !inf.ld_inflate_raw && !inf.z_inflate)
            return note(GBRS_ERR_UNSUPPORTED, "neither libdeflate nor zlib could be loaded");
        std::atomic<size_t> nextb{0};
        std::atomic<int> failed{0};
        std::atomic<uint64_t> bad{0};
        const uint64_t first_no = block_no - blocks.size();
        auto work = [&]() {
            void *ld = inf.ld_inflate_raw ? inf.ld_alloc() : nullptr;
            for (;;) {
                const size_t k0 = nextb.fetch_add(16);
                if (k0 >= blocks.size() || failed.load()) break;
                for (size_t k = k0; k < std::min(blocks.size(), k0 + 16); ++k) {
                    const Block &b = blocks[k];
                    unsigned char *dst = out.data() + b.out_off;
                    if (b.isize == 0) {
                        if (b.crc != 0) { bad = first_no + k; failed = 2; break; }
                        continue;
                    }
                    if (!inflate_raw(inf, ld, f.p + b.cdata, b.clen, dst, b.isize)) { bad = first_no + k; failed = 1; break; }
                    if (member_crc32(inf, dst, b.isize) != b.crc) { bad = first_no + k; failed = 2; break; }
                }
            }
            if (ld) inf.ld_free(ld);
        };
        {
            const unsigned n = (unsigned)std::max<size_t>(1, std::min<size_t>(nt, blocks.size() / 16));
            std::vector<std::thread> th;
            for (unsigned t = 1; t < n; ++t) th.emplace_back(work);
            work();
            for (auto &x : th) x.join();
        }
        if (failed.load() == 1)
            return note(GBRS_ERR_INVALID, "%s: BGZF block %llu does not inflate to its recorded size", path, (unsigned long long)bad.load());
        if (failed.load() == 2)
            return note(GBRS_ERR_INVALID, "%s: BGZF block %llu fails its CRC-32", path, (unsigned long long)bad.load());
        return GBRS_OK;
    }
};

// The BAM layer: fed the inflated bytes in pieces, calls the sink once for the header and once per record.
// Sink: int header(); int record(int32_t refid, uint32_t flag, const unsigned char *name, uint32_t len)
// - a non-zero return stops the parse (STOP = done on purpose, anything else = a status already reported).
constexpr int STOP = 1;

template <typename Sink>
struct BamParser {
    enum Stage { TEXT, REFS, RECORDS };
    gbrs_bam &b;
    Sink &sink;
    const char *path;
    Stage stage = TEXT;
    uint64_t n_ref = 0, record_no = 0;
    std::vector<unsigned char> carry;          // the head of one unfinished item, always shorter than the item
    BamParser(gbrs_bam &b_, Sink &s, const char *p) : b(b_), sink(s), path(p) {}

    // bytes the item at p needs in all, as far as the n visible bytes tell; 0 = error (reported)
    size_t need(const unsigned char *p, size_t n) {
        switch (stage) {
        case TEXT: {
            if (n < 8) return 8;
            if (std::memcmp(p, "BAM\1", 4) != 0) { fail(GBRS_ERR_INVALID, "%s: not a BAM file (the inflated stream does not start with BAM\\1)", path); return 0; }
            const uint32_t l_text = rd32(p + 4);
            if (l_text > 0x7FFFFFFFu) { fail(GBRS_ERR_INVALID, "%s: negative header text length", path); return 0; }
            return 8 + (size_t)l_text + 4;
        }
        case REFS: {
            if (n < 4) return 4;
            const uint32_t l_name = rd32(p);
            if (l_name == 0 || l_name > 0x7FFFFFFFu) { fail(GBRS_ERR_INVALID, "%s: reference sequence %zu has a name of length %u", path, b.ref_names.size(), l_name); return 0; }
            return 4 + (size_t)l_name + 4;
        }
        default: {
            if (n < 4) return 4;
            const uint32_t bs = rd32(p);
            if (bs < 32 || bs > 0x7FFFFFFFu) { fail(GBRS_ERR_INVALID, "%s: record %llu has block_size %u (a record holds at least 32 bytes)", path, (unsigned long long)record_no, bs); return 0; }
            return 4 + (size_t)bs;
        }
        }
    }

    int item(const unsigned char *p, size_t n) {
        switch (stage) {
        case TEXT: {
            const uint32_t nr = rd32(p + n - 4);
            if (nr > 0x7FFFFFFFu) return fail(GBRS_ERR_INVALID, "%s: negative number of reference sequences", path);
            n_ref = nr;
            b.ref_names.clear();
            b.ref_len.clear();
            stage = n_ref ? REFS : RECORDS;
            return n_ref ? 0 : sink.header();
        }
        case REFS: {
            const size_t l_name = n - 8;
            b.ref_names.emplace_back((const char *)p + 4, strnlen((const char *)p + 4, l_name));
            b.ref_len.push_back(rd32(p + 4 + l_name));
            if (b.ref_names.size() < n_ref) return 0;
            stage = RECORDS;
            return sink.header();
        }
        default: {
            const int32_t refid = (int32_t)rd32(p + 4);
            const uint32_t l_read_name = p[12], flag = rd16(p + 18);
            if (l_read_name == 0)
                return fail(GBRS_ERR_INVALID, "%s: record %llu has l_read_name 0 (the name's terminator alone takes one byte)", path, (unsigned long long)record_no);
            if (n < 36 + (size_t)l_read_name)
                return fail(GBRS_ERR_INVALID, "%s: record %llu: block_size %zu does not hold its %u name bytes", path, (unsigned long long)record_no, n - 4, l_read_name);
            if (refid >= 0 && (uint64_t)refid >= n_ref)
                return fail(GBRS_ERR_INVALID, "%s: record %llu names reference sequence %d of %llu", path, (unsigned long long)record_no, refid, (unsigned long long)n_ref);
            const uint32_t len = (uint32_t)strnlen((const char *)p + 36, l_read_name - 1);
            ++record_no;
            return sink.record(refid, flag, p + 36, len);
        }
        }
    }

    int feed(const unsigned char *data, size_t n) {
        size_t pos = 0;
        while (!carry.empty()) {
            const size_t want = need(carry.data(), carry.size());
            if (!want) return GBRS_ERR_INVALID;
            if (carry.size() >= want) {
                if (int rc = item(carry.data(), want)) return rc;
                carry.clear();
                break;
            }
            const size_t take = std::min(want - carry.size(), n - pos);
            carry.insert(carry.end(), data + pos, data + pos + take);
            pos += take;
            if (carry.size() < want) return 0;      // the batch is used up
        }
        for (;;) {
            const size_t want = need(data + pos, n - pos);
            if (!want) return GBRS_ERR_INVALID;
            if (n - pos < want) break;
            if (int rc = item(data + pos, want)) return rc;
            pos += want;
        }
        carry.assign(data + pos, data + n);
        return 0;
    }

    int finish() {
        if (stage != RECORDS) return fail(GBRS_ERR_INVALID, "%s: truncated BAM header (%zu of %llu reference sequences read)", path, b.ref_names.size(), (unsigned long long)n_ref);
        if (!carry.empty()) return fail(GBRS_ERR_INVALID, "%s: truncated record %llu (%zu bytes of it at the end of the file)", path, (unsigned long long)record_no, carry.size());
        return GBRS_OK;
    }
};

template <typename Sink>
int bam_stream(gbrs_bam &b, Sink &sink) {
    MappedFile f;
    GBRS_TRY(f.open_path(b.path.c_str()));
    BgzfStream z(f, b.path.c_str(), b.threads);
    BamParser<Sink> parser(b, sink, b.path.c_str());
    std::vector<unsigned char> cur, nxt;
    if (int zrc = z.next(cur)) return fail(zrc, "%s", z.err);
    for (;;) {
        const bool more = !z.at_end();
        std::future<int> fut;
        // a header-only pass stops inside the first batches: no read-ahead there
        if (more && !sink.wants_header_only) fut = std::async(std::launch::async, [&]() { return z.next(nxt); });
        const int rc = parser.feed(cur.data(), cur.size());
        int zrc = GBRS_OK;
        if (fut.valid()) zrc = fut.get();
        else if (more && rc == 0) zrc = z.next(nxt);
        if (rc == STOP) return GBRS_OK;
        if (rc) return rc;            // the parser's message wins: it concerns an earlier byte of the file
        if (zrc != GBRS_OK) return fail(zrc, "%s", z.err);
        if (!more) break;
        cur.swap(nxt);
    }
    return parser.finish();
}

struct HeaderSink {
    static constexpr bool wants_header_only = true;
    int header() { return STOP; }
    int record(int32_t, uint32_t, const unsigned char *, uint32_t) { return STOP; }
};

struct ScanSink {
    static constexpr bool wants_header_only = false;
    uint64_t cap, names_cap, n = 0, names_len = 0;
    int32_t *refid; uint32_t *flag; uint64_t *name_off; char *names;
    int header() { return 0; }
    int record(int32_t r, uint32_t f, const unsigned char *name, uint32_t len) {
        if (n < cap) {
            refid[n] = r;
            flag[n] = f;
            name_off[n] = names_len;
            if (names && len && names_len + len <= names_cap) std::memcpy(names + names_len, name, len);
        }
        ++n;
        names_len += len;
        return 0;
    }
};

struct CollectSink {
    static constexpr bool wants_header_only = false;
    gbrs_bam &b;
    explicit CollectSink(gbrs_bam &b_) : b(b_) {}
    int header() { return 0; }
    int record(int32_t refid, uint32_t flag, const unsigned char *name, uint32_t len) {
        // a record named like the one before it reuses that candidate (aligners write a read's alignments together)
        const size_t nc = b.cand_off.size() - 1;
        const uint64_t last = nc ? b.cand_off[nc - 1] : 0;
        if (!nc || b.cand_off[nc] - last != len || (len && std::memcmp(b.cand_bytes.data() + last, name, len) != 0)) {
            if (nc >= 0xFFFFFFFFull) return fail(GBRS_ERR_UNSUPPORTED, "%s: more than 2^32 - 1 candidate read names", b.path.c_str());
            b.cand_bytes.insert(b.cand_bytes.end(), name, name + len);
            b.cand_off.push_back(b.cand_bytes.size());
            if (len > b.max_name) b.max_name = len;
        }
        // the reference's test: the whole flag word is neither 4 nor 8 (AlignmentMatrixFactory.py:60, :68)
        if (flag != 4 && flag != 8) b.recs.push_back(gbrs_bam::Rec{(uint32_t)(b.cand_off.size() - 2), refid});
        return 0;
    }
};

template <typename F>
int guarded(F &&f) {
    try {
        return f();
    } catch (const std::bad_alloc &) {
        return fail(GBRS_ERR_INVALID, "out of host memory while reading the BAM file");
    }
}

}  // namespace

int bam_collect(gbrs_bam *b) {
    bam_release_collected(b);
    b->cand_off.push_back(0);
    CollectSink sink(*b);
    return guarded([&]() { return bam_stream(*b, sink); });
}

void bam_release_collected(gbrs_bam *b) {
    std::vector<gbrs_bam::Rec>().swap(b->recs);
    std::vector<unsigned char>().swap(b->cand_bytes);
    std::vector<uint64_t>().swap(b->cand_off);
    b->max_name = 0;
}

}  // namespace gbrs

extern "C" {

int gbrs_bam_open(const char *path, int32_t threads, gbrs_bam_t **out, uint64_t *n_ref, uint64_t *ref_names_len) {
    using gbrs::fail;
    if (!path || !out) return fail(GBRS_ERR_INVALID, "bad argument");
    *out = nullptr;
    return gbrs::guarded([&]() {
        gbrs_bam *b = new gbrs_bam();
        b->path = path;
        b->threads = threads;
        gbrs::HeaderSink sink;
        const int rc = gbrs::bam_stream(*b, sink);
        if (rc != GBRS_OK) { delete b; return rc; }
        uint64_t bytes = 0;
        for (const std::string &s : b->ref_names) bytes += s.size();
        if (n_ref) *n_ref = b->ref_names.size();
        if (ref_names_len) *ref_names_len = bytes;
        *out = b;
        return (int)GBRS_OK;
    });
}

int gbrs_bam_references(gbrs_bam_t *b, char *names, uint64_t names_cap, uint64_t *name_off, uint32_t *ref_len) {
    using gbrs::fail;
    if (!b || !name_off) return fail(GBRS_ERR_INVALID, "bad argument");
    uint64_t at = 0;
    for (size_t k = 0; k < b->ref_names.size(); ++k) {
        const std::string &s = b->ref_names[k];
        name_off[k] = at;
        if (at + s.size() > names_cap || (!names && !s.empty())) return fail(GBRS_ERR_INVALID, "the name buffer is too small");
        if (!s.empty()) std::memcpy(names + at, s.data(), s.size());
        at += s.size();
        if (ref_len) ref_len[k] = b->ref_len[k];
    }
    name_off[b->ref_names.size()] = at;
    return GBRS_OK;
}

int gbrs_bam_set_reference_map(gbrs_bam_t *b, uint64_t n_ref, const uint32_t *hap, const uint32_t *locus,
                               uint32_t num_haps, uint32_t num_loci) {
    using gbrs::fail;
    if (!b || (n_ref && (!hap || !locus)) || num_haps == 0 || num_loci == 0) return fail(GBRS_ERR_INVALID, "bad argument");
    if (n_ref != b->ref_names.size())
        return fail(GBRS_ERR_INVALID, "the map has %llu entries, the header %zu reference sequences", (unsigned long long)n_ref, b->ref_names.size());
    for (uint64_t k = 0; k < n_ref; ++k) {
        if (hap[k] == gbrs::BAM_REF_UNUSABLE) {
            if (locus[k] < gbrs::BAM_REF_NOT_TWO_PARTS || locus[k] > gbrs::BAM_REF_UNKNOWN_LOCUS)
                return fail(GBRS_ERR_INVALID, "map entry %llu: unknown reason code %u", (unsigned long long)k, locus[k]);
        } else if (hap[k] >= num_haps || locus[k] >= num_loci) {
            return fail(GBRS_ERR_INVALID, "map entry %llu (%u, %u) outside %u haplotypes x %u loci", (unsigned long long)k, hap[k], locus[k], num_haps, num_loci);
        }
    }
    return gbrs::guarded([&]() {
        b->ref_hap.assign(hap, hap + n_ref);
        b->ref_locus.assign(locus, locus + n_ref);
        b->num_haps = num_haps;
        b->num_loci = num_loci;
        b->map_set = true;
        return (int)GBRS_OK;
    });
}

int gbrs_bam_scan_records(gbrs_bam_t *b, uint64_t cap, int32_t *refid, uint32_t *flag, uint64_t *name_off, char *names,
                          uint64_t names_cap, uint64_t *n_records, uint64_t *names_len) {
    using gbrs::fail;
    if (!b || !n_records || !names_len || (cap && (!refid || !flag || !name_off))) return fail(GBRS_ERR_INVALID, "bad argument");
    gbrs::ScanSink sink;
    sink.cap = cap; sink.names_cap = names_cap;
    sink.refid = refid; sink.flag = flag; sink.name_off = name_off; sink.names = names;
    const int rc = gbrs::guarded([&]() { return gbrs::bam_stream(*b, sink); });
    if (rc != GBRS_OK) return rc;
    if (name_off && sink.n <= cap) name_off[sink.n] = sink.names_len;       // name_off holds cap + 1 entries
    *n_records = sink.n;
    *names_len = sink.names_len;
    return GBRS_OK;
}

int gbrs_bam_destroy(gbrs_bam_t *b) {
    if (!b) return GBRS_OK;
    if (b->dev && b->dev_free) b->dev_free(b->dev);
    delete b;
    return GBRS_OK;
}

}  // extern "C"
