// The inflater the host-side readers share (hostio.hip: HDF5 chunks and zip members; bamio.hip: BGZF blocks):
// libdeflate or zlib, looked up at run time, plus CRC-32 and little-endian field readers.  Host code only.
#pragma once
#include <dlfcn.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace gbrs {

typedef int (*uncompress_fn)(unsigned char *, unsigned long *, const unsigned char *, unsigned long);
typedef void *(*ld_alloc_fn)(void);
typedef void (*ld_free_fn)(void *);
typedef int (*ld_inflate_fn)(void *, const void *, size_t, void *, size_t, size_t *);
// zlib's streaming interface, for raw deflate streams (zip members): z_stream is opaque here except for the
// leading fields the caller sets, so the struct below mirrors zlib.h's layout on LP64
struct ZStream {
    const unsigned char *next_in; unsigned int avail_in; unsigned long total_in;
    unsigned char *next_out; unsigned int avail_out; unsigned long total_out;
    const char *msg; void *state; void *zalloc; void *zfree; void *opaque; int data_type; unsigned long adler; unsigned long reserved;
};
typedef int (*z_init2_fn)(ZStream *, int, const char *, int);
typedef int (*z_inflate_fn)(ZStream *, int);
typedef int (*z_end_fn)(ZStream *);
typedef uint32_t (*ld_crc32_fn)(uint32_t, const void *, size_t);
typedef unsigned long (*z_crc32_fn)(unsigned long, const unsigned char *, unsigned int);

struct Inflaters {
    uncompress_fn z_uncompress = nullptr;
    ld_alloc_fn ld_alloc = nullptr;
    ld_free_fn ld_free = nullptr;
    ld_inflate_fn ld_inflate = nullptr;
    ld_inflate_fn ld_inflate_raw = nullptr;       // libdeflate_deflate_decompress: no zlib wrapper (zip members)
    z_init2_fn z_init2 = nullptr;
    z_inflate_fn z_inflate = nullptr;
    z_end_fn z_end = nullptr;
    ld_crc32_fn ld_crc32 = nullptr;               // libdeflate_crc32: carry-less multiply, several GB/s per core
    z_crc32_fn z_crc32 = nullptr;
    Inflaters() {
        // libdeflate (about three times zlib's inflate speed) when the machine has it, zlib otherwise;
        // both are looked up at run time so the library has no link-time dependency on either
        const char *ld_names[] = {std::getenv("GBRS_LIBDEFLATE"), "libdeflate.so.0", "libdeflate.so", "/opt/conda/lib/libdeflate.so.0"};
        for (const char *n : ld_names) {
            if (!n || !*n) continue;
            if (void *h = dlopen(n, RTLD_NOW | RTLD_LOCAL)) {
                ld_alloc = (ld_alloc_fn)dlsym(h, "libdeflate_alloc_decompressor");
                ld_free = (ld_free_fn)dlsym(h, "libdeflate_free_decompressor");
                ld_inflate = (ld_inflate_fn)dlsym(h, "libdeflate_zlib_decompress");
                ld_inflate_raw = (ld_inflate_fn)dlsym(h, "libdeflate_deflate_decompress");
                ld_crc32 = (ld_crc32_fn)dlsym(h, "libdeflate_crc32");
                if (ld_alloc && ld_free && ld_inflate && ld_inflate_raw) break;
                ld_alloc = nullptr; ld_free = nullptr; ld_inflate = nullptr; ld_inflate_raw = nullptr;
            }
        }
        const char *z_names[] = {"libz.so.1", "libz.so", "/opt/conda/lib/libz.so.1"};
        for (const char *n : z_names)
            if (void *h = dlopen(n, RTLD_NOW | RTLD_LOCAL)) {
                z_uncompress = (uncompress_fn)dlsym(h, "uncompress");
                z_init2 = (z_init2_fn)dlsym(h, "inflateInit2_");
                z_inflate = (z_inflate_fn)dlsym(h, "inflate");
                z_end = (z_end_fn)dlsym(h, "inflateEnd");
                z_crc32 = (z_crc32_fn)dlsym(h, "crc32");
                if (z_uncompress) break;
            }
    }
};

inline const Inflaters &inflaters() {
    static const Inflaters inf;
    return inf;
}

// one raw deflate stream -> exactly out_bytes bytes; ld = this thread's libdeflate decompressor or null
inline bool inflate_raw(const Inflaters &inf, void *ld, const unsigned char *in, size_t in_bytes, unsigned char *out,
                        size_t out_bytes) {
    if (ld && inf.ld_inflate_raw) {
        size_t n = 0;
        if (inf.ld_inflate_raw(ld, in, in_bytes, out, out_bytes, &n) == 0 && n == out_bytes) return true;
    }
    if (inf.z_init2 && inf.z_inflate && inf.z_end && in_bytes <= 0xFFFFFFFFu && out_bytes <= 0xFFFFFFFFu) {
        ZStream zs;
        std::memset(&zs, 0, sizeof(zs));
        if (inf.z_init2(&zs, -15, "1.2.11", (int)sizeof(ZStream)) != 0) return false;
        zs.next_in = in; zs.avail_in = (unsigned int)in_bytes;
        zs.next_out = out; zs.avail_out = (unsigned int)out_bytes;
        const int rc = inf.z_inflate(&zs, 4 /* Z_FINISH */);
        const bool ok = rc == 1 /* Z_STREAM_END */ && zs.total_out == out_bytes;
        inf.z_end(&zs);
        return ok;
    }
    return false;
}

// CRC-32 of a zip member's plain bytes (what numpy.load / zipfile check on every access and report as BadZipFile:
// the reference inherits that): libdeflate's when the machine has it, zlib's otherwise, a table walk as the last resort
inline uint32_t member_crc32(const Inflaters &inf, const unsigned char *p, size_t n) {
    if (inf.ld_crc32) return inf.ld_crc32(0, p, n);
    if (inf.z_crc32) {
        unsigned long c = 0;
        while (n) {
            const unsigned int part = (unsigned int)std::min<size_t>(n, 1u << 30);
            c = inf.z_crc32(c, p, part);
            p += part;
            n -= part;
        }
        return (uint32_t)c;
    }
    static const std::array<uint32_t, 256> table = [] {
        std::array<uint32_t, 256> t{};
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[i] = c;
        }
        return t;
    }();
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

inline uint16_t rd16(const unsigned char *p) { return (uint16_t)(p[0] | (p[1] << 8)); }
inline uint32_t rd32(const unsigned char *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint64_t rd64(const unsigned char *p) { return (uint64_t)rd32(p) | ((uint64_t)rd32(p + 4) << 32); }

}  // namespace gbrs
