// Driver for the sanitizer build of gbrs_amd/csrc/bamio.hip (the BGZF/BAM reader of `gbrs bam2emase`), under
// AddressSanitizer + UndefinedBehaviorSanitizer.  tests/test_bam_sanitizers.py writes the files:
//   <dir>/valid_*.bam + .expect   ("n_ref n_records", then one "refID flag name" line per record): read and compared
//   <dir>/bad_*.bam               malformed on purpose: must be refused with a message
//   <dir>/small.bam               truncated here at every byte offset (refused, or - where whole blocks holding whole
//                                 records are left - a prefix of the records) and with every byte inverted in turn
//                                 (any status is fine); a sanitizer report or a crash is not
// Exit code 0 = clean.
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dirent.h>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/gbrs_hip.h"

namespace gbrs {
static char g_err[1024];
int fail(int status, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return status;
}
}  // namespace gbrs

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::fprintf(stderr, "CHECK failed: %s (%s:%d) [%s]\n", #cond, __FILE__, __LINE__, gbrs::g_err); return 1; } \
    } while (0)

static std::string slurp(const std::string &p) {
    std::ifstream f(p, std::ios::binary);
    return std::string((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static void spit(const std::string &p, const std::string &data) {
    std::ofstream f(p, std::ios::binary | std::ios::trunc);
    f.write(data.data(), (std::streamsize)data.size());
}

struct Scan {
    int status = 0;
    std::vector<std::string> refs, names;
    std::vector<int32_t> refid;
    std::vector<uint32_t> flag;
};

// open + references + the two-call record scan, the way gbrs_amd/bam2emase.py drives them
static int scan_file(const std::string &path, Scan &out, int threads) {
    gbrs_bam_t *b = nullptr;
    uint64_t n_ref = 0, names_len = 0;
    out = Scan();
    gbrs::g_err[0] = '\0';
    out.status = gbrs_bam_open(path.c_str(), threads, &b, &n_ref, &names_len);
    if (out.status != GBRS_OK) { CHECK(b == nullptr && gbrs::g_err[0] != '\0'); return 0; }
    CHECK(b != nullptr);
    {
        std::vector<char> names(names_len + 1);
        std::vector<uint64_t> off(n_ref + 1);
        std::vector<uint32_t> len(n_ref);
        CHECK(gbrs_bam_references(b, names.data(), names_len, off.data(), len.data()) == GBRS_OK);
        CHECK(off[n_ref] == names_len);
        for (uint64_t k = 0; k < n_ref; ++k) out.refs.emplace_back(names.data() + off[k], names.data() + off[k + 1]);
        if (names_len) CHECK(gbrs_bam_references(b, names.data(), names_len - 1, off.data(), nullptr) != GBRS_OK);
    }
    uint64_t n = 0, nb = 0;
    out.status = gbrs_bam_scan_records(b, 0, nullptr, nullptr, nullptr, nullptr, 0, &n, &nb);
    if (out.status == GBRS_OK) {
        out.refid.resize(n);
        out.flag.resize(n);
        std::vector<uint64_t> off(n + 1);
        std::vector<char> names(nb + 1);
        uint64_t n2 = 0, nb2 = 0;
        CHECK(gbrs_bam_scan_records(b, n, out.refid.data(), out.flag.data(), off.data(), names.data(), nb, &n2, &nb2) == GBRS_OK);
        CHECK(n2 == n && nb2 == nb && off[n] == nb);
        for (uint64_t k = 0; k < n; ++k) out.names.emplace_back(names.data() + off[k], names.data() + off[k + 1]);
        // a capacity smaller than the file: counted, nothing written past it
        if (n > 1) {
            std::vector<int32_t> r1(1);
            std::vector<uint32_t> f1(1);
            std::vector<uint64_t> o1(2);
            CHECK(gbrs_bam_scan_records(b, 1, r1.data(), f1.data(), o1.data(), nullptr, 0, &n2, &nb2) == GBRS_OK);
            CHECK(n2 == n && r1[0] == out.refid[0]);
        }
    } else {
        CHECK(gbrs::g_err[0] != '\0');
    }
    // the map's checks (host only; the conversion itself needs a device and is not part of this build)
    {
        std::vector<uint32_t> hap(n_ref, 0), loc(n_ref, 0);
        CHECK(gbrs_bam_set_reference_map(b, n_ref, hap.data(), loc.data(), 1, 1) == GBRS_OK);
        CHECK(gbrs_bam_set_reference_map(b, n_ref + 1, hap.data(), loc.data(), 1, 1) != GBRS_OK);
        if (n_ref) {
            loc[0] = 1;
            CHECK(gbrs_bam_set_reference_map(b, n_ref, hap.data(), loc.data(), 1, 1) != GBRS_OK);
            hap[0] = 0xFFFFFFFFu;
            loc[0] = 3;
            CHECK(gbrs_bam_set_reference_map(b, n_ref, hap.data(), loc.data(), 1, 1) == GBRS_OK);
            loc[0] = 9;
            CHECK(gbrs_bam_set_reference_map(b, n_ref, hap.data(), loc.data(), 1, 1) != GBRS_OK);
        }
    }
    CHECK(gbrs_bam_destroy(b) == GBRS_OK);
    return 0;
}

int main(int argc, char **argv) {
    const std::string dir = argc > 1 ? argv[1] : "/tmp";
    std::vector<std::string> valid, bad;
    if (DIR *d = opendir(dir.c_str())) {
        while (dirent *e = readdir(d)) {
            const std::string n = e->d_name;
            if (n.size() > 4 && n.substr(n.size() - 4) == ".bam") {
                if (n.rfind("valid_", 0) == 0) valid.push_back(n);
                if (n.rfind("bad_", 0) == 0) bad.push_back(n);
            }
        }
        closedir(d);
    }
    CHECK(!valid.empty() && !bad.empty());
    Scan s;
    for (const std::string &n : valid) {
        for (int threads : {1, 4}) {
            CHECK(scan_file(dir + "/" + n, s, threads) == 0);
            CHECK(s.status == GBRS_OK);
            std::istringstream ex(slurp(dir + "/" + n.substr(0, n.size() - 4) + ".expect"));
            size_t n_ref = 0, n_rec = 0;
            ex >> n_ref >> n_rec;
            CHECK(s.refs.size() == n_ref && s.names.size() == n_rec);
            for (size_t k = 0; k < n_rec; ++k) {
                long long r = 0, f = 0;
                std::string name;
                ex >> r >> f >> name;
                CHECK(s.refid[k] == r && s.flag[k] == (uint32_t)f && s.names[k] == name);
            }
        }
    }
    for (const std::string &n : bad) {
        CHECK(scan_file(dir + "/" + n, s, 2) == 0);
        if (s.status == GBRS_OK) std::fprintf(stderr, "%s was accepted\n", n.c_str());
        CHECK(s.status != GBRS_OK);
    }
    // bad arguments
    {
        gbrs_bam_t *b = nullptr;
        uint64_t a = 0, c = 0;
        CHECK(gbrs_bam_open(nullptr, 0, &b, &a, &c) != GBRS_OK);
        CHECK(gbrs_bam_open((dir + "/does-not-exist.bam").c_str(), 0, &b, &a, &c) != GBRS_OK && b == nullptr);
        CHECK(gbrs_bam_open(dir.c_str(), 0, &b, &a, &c) != GBRS_OK && b == nullptr);         // a directory
        CHECK(gbrs_bam_destroy(nullptr) == GBRS_OK);
        CHECK(gbrs_bam_scan_records(nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, &a, &c) != GBRS_OK);
    }
    // every truncation and every single inverted byte of a small file
    const std::string small = slurp(dir + "/small.bam");
    CHECK(small.size() > 100 && small.size() < 4000);
    const std::string tmp = dir + "/mutant.bam";
    Scan whole;
    CHECK(scan_file(dir + "/small.bam", whole, 1) == 0 && whole.status == GBRS_OK && whole.names.size() > 3);
    size_t refused = 0;
    for (size_t cut = 0; cut < small.size(); ++cut) {
        spit(tmp, small.substr(0, cut));
        CHECK(scan_file(tmp, s, 1) == 0);
        refused += s.status != GBRS_OK;
        if (s.status == GBRS_OK) {
            // whole blocks that end with a whole record are a valid shorter file: then exactly a prefix of the records
            CHECK(s.refs == whole.refs && s.names.size() <= whole.names.size());
            for (size_t k = 0; k < s.names.size(); ++k)
                CHECK(s.names[k] == whole.names[k] && s.refid[k] == whole.refid[k] && s.flag[k] == whole.flag[k]);
        }
    }
    CHECK(refused > small.size() / 2);
    for (size_t at = 0; at < small.size(); ++at) {
        std::string m = small;
        m[at] = (char)~m[at];
        spit(tmp, m);
        CHECK(scan_file(tmp, s, 1) == 0);
    }
    std::remove(tmp.c_str());
    std::printf("bam sanitizer driver: ok (%zu valid, %zu malformed, %zu truncations refused)\n", valid.size(), bad.size(), refused);
    return 0;
}
