// Native host readers for the data path: the reference's sample cache and its PNG frames; the cache's writer; and the
// PNG writer of the predict tool (at the end of the file).
// Sample cache (reference dataset.py:86-105 load_cached_sample, cache.py:50-112):
// one np.savez file per pair, a zip of left.npy / right.npy (uint8 HWC) and disparity.npy (f16 HW): stored members
// (np.savez, the default) or raw-deflate members (np.savez_compressed, the reference's `cache.py --compress`).
// A batch of files is read by a pool of threads straight into the caller's (pinned) host buffers, so the data path
// needs no worker processes, no pickling and no second pinning copy (tools/loader_bench.py: the torch DataLoader
// path tops out near 3-4k pairs/s on the box's 16 cores).
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <atomic>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace {

uint16_t rd16(const unsigned char* p) { return (uint16_t)(p[0] | p[1] << 8); }
uint32_t rd32(const unsigned char* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
uint64_t rd64(const unsigned char* p) { return (uint64_t)rd32(p) | (uint64_t)rd32(p + 4) << 32; }

bool read_file(const char* path, std::vector<unsigned char>& buf, std::string& why) {
    const int fd = open(path, O_RDONLY);
    if (fd < 0) {
        why = "cannot open";
        return false;
    }
    struct stat st;
    if (fstat(fd, &st) != 0) {
        close(fd);
        why = "cannot stat";
        return false;
    }
    buf.resize((size_t)st.st_size);
    size_t got = 0;
    while (got < buf.size()) {
        const ssize_t r = read(fd, buf.data() + got, buf.size() - got);
        if (r <= 0) break;
        got += (size_t)r;
    }
    close(fd);
    if (got != buf.size()) {
        why = "short read";
        return false;
    }
    return true;
}

// the .npy payload of one stored zip member, checked against dtype descr and the expected shape text
bool npy_payload(const unsigned char* p, size_t n, const char* descr, const std::string& shape, size_t bytes,
                 const unsigned char** data, std::string& why) {
    if (n < 10 || memcmp(p, "\x93NUMPY", 6) != 0) {
        why = "not an .npy member";
        return false;
    }
    const int major = p[6];
    const size_t hl = major == 1 ? rd16(p + 8) : rd32(p + 8);
    const size_t off = major == 1 ? 10 : 12;
    if (off + hl > n) {
        why = "truncated .npy header";
        return false;
    }
    const std::string hdr((const char*)p + off, hl);
    if (hdr.find(std::string("'descr': '") + descr + "'") == std::string::npos ||
        hdr.find("'fortran_order': False") == std::string::npos ||
        hdr.find("'shape': " + shape) == std::string::npos) {
        why = "dtype/shape mismatch (" + hdr.substr(0, hdr.find('}') + 1) + ")";
        return false;
    }
    if (off + hl + bytes > n) {
        why = "truncated .npy data";
        return false;
    }
    *data = p + off + hl;
    return true;
}

// a raw-deflate zip member (method 8) inflated into `out` (exactly usize bytes)
bool inflate_member(const unsigned char* src, size_t csize, size_t usize, std::vector<unsigned char>& out,
                    std::string& why) {
    out.resize(usize);
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, -MAX_WBITS) != Z_OK) {
        why = "inflateInit2 failed";
        return false;
    }
    zs.next_in = const_cast<unsigned char*>(src);
    zs.avail_in = (uInt)csize;
    zs.next_out = out.data();
    zs.avail_out = (uInt)usize;
    const int rc = inflate(&zs, Z_FINISH);
    const size_t got = zs.total_out;
    inflateEnd(&zs);
    if (rc != Z_STREAM_END || got != usize) {
        why = "corrupt deflate member";
        return false;
    }
    return true;
}

// walks the zip's local headers (sizes in the header or its zip64 extra field); members stored (np.savez) or
// deflated (np.savez_compressed), inflated into `scratch`
bool parse_npz(const std::vector<unsigned char>& f, int H, int W, unsigned char* left, unsigned char* right,
               uint16_t* disp, std::vector<unsigned char>& scratch, std::string& why) {
    const std::string s3 = "(" + std::to_string(H) + ", " + std::to_string(W) + ", 3)";
    const std::string s2 = "(" + std::to_string(H) + ", " + std::to_string(W) + ")";
    const size_t rgb = (size_t)H * W * 3, dbytes = (size_t)H * W * 2;
    int found = 0;
    size_t pos = 0;
    while (pos + 30 <= f.size() && rd32(&f[pos]) == 0x04034b50u) {
        const unsigned char* h = &f[pos];
        const uint16_t flags = rd16(h + 6), method = rd16(h + 8), nlen = rd16(h + 26), xlen = rd16(h + 28);
        uint64_t csize = rd32(h + 18), usize = rd32(h + 22);
        if (pos + 30 + nlen + xlen > f.size()) break;
        const std::string name((const char*)h + 30, nlen);
        if (csize == 0xffffffffu || usize == 0xffffffffu) {  // zip64 extra field: usize, csize
            const unsigned char* x = h + 30 + nlen;
            for (size_t k = 0; k + 4 <= xlen;) {
                const uint16_t id = rd16(x + k), sz = rd16(x + k + 2);
                if (id == 1 && sz >= 16) {
                    usize = rd64(x + k + 4);
                    csize = rd64(x + k + 12);
                }
                k += 4 + sz;
            }
        }
        if ((method != 0 && method != 8) || (flags & 8) || (method == 0 && csize != usize)) {
            why = "member " + name + " uses an unsupported zip method or is streamed (not np.savez output)";
            return false;
        }
        const size_t data = pos + 30 + nlen + xlen;
        if (data + csize > f.size()) break;
        const bool wanted = name == "left.npy" || name == "right.npy" || name == "disparity.npy";
        const unsigned char* mem = &f[data];
        if (wanted && method == 8) {
            if (usize > ((size_t)1 << 32) || !inflate_member(mem, csize, usize, scratch, why)) {
                why = name + ": " + (why.empty() ? "member too large" : why);
                return false;
            }
            mem = scratch.data();
        }
        const unsigned char* src = nullptr;
        if (name == "left.npy" || name == "right.npy") {
            if (!npy_payload(mem, usize, "|u1", s3, rgb, &src, why)) {
                why = name + ": " + why;
                return false;
            }
            memcpy(name[0] == 'l' ? left : right, src, rgb);
            found |= name[0] == 'l' ? 1 : 2;
        } else if (name == "disparity.npy") {
            if (!npy_payload(mem, usize, "<f2", s2, dbytes, &src, why)) {
                why = name + ": " + why;
                return false;
            }
            memcpy(disp, src, dbytes);
            found |= 4;
        }
        pos = data + csize;
    }
    if (found != 7) {
        why = "missing left/right/disparity member";
        return false;
    }
    return true;
}

}  // namespace

extern "C" int sd_read_cache_batch(const char* const* paths, int n, int H, int W, uint8_t* left, uint8_t* right,
                                   uint16_t* disparity, int threads, char* err, int errlen) {
    if (!paths || n < 0 || H <= 0 || W <= 0 || !left || !right || !disparity) {
        if (err && errlen > 0) snprintf(err, (size_t)errlen, "sd_read_cache_batch: bad args");
        return -1;
    }
    if (threads < 1) threads = 1;
    if (threads > n) threads = n > 0 ? n : 1;
    const size_t rgb = (size_t)H * W * 3, hw = (size_t)H * W;
    std::atomic<int> next{0}, first_bad{n};
    std::mutex mu;
    std::string bad_why;
    auto work = [&]() {
        std::vector<unsigned char> buf, scratch;
        std::string why;
        for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) {
            bool ok = paths[i] && read_file(paths[i], buf, why);
            if (ok) ok = parse_npz(buf, H, W, left + i * rgb, right + i * rgb, disparity + i * hw, scratch, why);
            if (!ok) {
                std::lock_guard<std::mutex> g(mu);
                if (i < first_bad.load()) {
                    first_bad.store(i);
                    bad_why = why;
                }
            }
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    const int bad = first_bad.load();
    if (bad < n) {
        if (err && errlen > 0)
            snprintf(err, (size_t)errlen, "%s: %s", paths[bad] ? paths[bad] : "(null)", bad_why.c_str());
        return bad + 1;
    }
    return 0;
}

// ------------------------------------------------------------------ the cache writer
// save_cached_sample's file (reference dataset.py:110-128: np.savez / np.savez_compressed of left, right, disparity)
// written from the buffers the device filled: the three .npy members (version 1.0 headers, padded as NumPy pads them)
// in a plain zip, the whole file composed in memory, written under a temporary name beside its target and renamed over
// it. The reference writes in place, so a build that is interrupted leaves a truncated entry that its next run skips as
// existing; here the target is never a partial file.

namespace {

void put16(std::vector<unsigned char>& o, uint32_t v) {
    o.push_back((unsigned char)v);
    o.push_back((unsigned char)(v >> 8));
}
void put32(std::vector<unsigned char>& o, uint32_t v) {
    put16(o, v & 0xffffu);
    put16(o, v >> 16);
}

// magic, version 1.0, header length, then the dict text space-padded so that the data starts at a multiple of 64
// (numpy.lib.format._wrap_header, ARRAY_ALIGN = 64), ending in '\n'
void npy_member(std::vector<unsigned char>& o, const char* descr, const std::string& shape, const void* data,
                size_t bytes) {
    std::string hdr = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': " + shape + ", }";
    const size_t pad = 64 - (10 + hdr.size() + 1) % 64;
    hdr.append(pad, ' ');  // 1..64, as NumPy: a full 64 when the text already ends on the boundary
    hdr.push_back('\n');
    o.clear();
    o.reserve(10 + hdr.size() + bytes);
    o.insert(o.end(), {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0});
    put16(o, (uint32_t)hdr.size());
    o.insert(o.end(), hdr.begin(), hdr.end());
    const unsigned char* p = static_cast<const unsigned char*>(data);
    o.insert(o.end(), p, p + bytes);
}

bool deflate_member(const std::vector<unsigned char>& in, std::vector<unsigned char>& out, std::string& why) {
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (deflateInit2(&zs, Z_DEFAULT_COMPRESSION, Z_DEFLATED, -MAX_WBITS, 8, Z_DEFAULT_STRATEGY) != Z_OK) {
        why = "deflateInit2 failed";
        return false;
    }
    out.resize(deflateBound(&zs, (uLong)in.size()));
    zs.next_in = const_cast<unsigned char*>(in.data());
    zs.avail_in = (uInt)in.size();
    zs.next_out = out.data();
    zs.avail_out = (uInt)out.size();
    const int rc = deflate(&zs, Z_FINISH);
    out.resize(zs.total_out);
    deflateEnd(&zs);
    if (rc != Z_STREAM_END) {
        why = "deflate failed";
        return false;
    }
    return true;
}

// the zip of one sample in `file` (local header + data per member, central directory, end record); no zip64: a
// member of 4 GiB or more is refused
bool compose_npz(int H, int W, const uint8_t* left, const uint8_t* right, const uint16_t* disp, bool compress,
                 std::vector<unsigned char>& file, std::vector<unsigned char>& member, std::vector<unsigned char>& packed,
                 std::string& why) {
    const std::string s3 = "(" + std::to_string(H) + ", " + std::to_string(W) + ", 3)";
    const std::string s2 = "(" + std::to_string(H) + ", " + std::to_string(W) + ")";
    const size_t rgb = (size_t)H * W * 3, dbytes = (size_t)H * W * 2;
    if (rgb + 4096 >= 0xffffffffull / 3) {
        why = "sample too large for a zip without zip64";
        return false;
    }
    struct Entry {
        const char* name;
        uint32_t crc, csize, usize, offset;
    } ent[3] = {{"left.npy", 0, 0, 0, 0}, {"right.npy", 0, 0, 0, 0}, {"disparity.npy", 0, 0, 0, 0}};
    const uint32_t method = compress ? 8 : 0;
    const uint32_t dos_time = 0, dos_date = 0x21;  // 1980-01-01 00:00: the contents, not the clock, define an entry
    file.clear();
    for (int m = 0; m < 3; ++m) {
        if (m < 2)
            npy_member(member, "|u1", s3, m == 0 ? left : right, rgb);
        else
            npy_member(member, "<f2", s2, disp, dbytes);
        const std::vector<unsigned char>* body = &member;
        if (compress) {
            if (!deflate_member(member, packed, why)) return false;
            body = &packed;
        }
        Entry& e = ent[m];
        e.crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), member.data(), (uInt)member.size());
        e.usize = (uint32_t)member.size();
        e.csize = (uint32_t)body->size();
        e.offset = (uint32_t)file.size();
        const size_t nlen = strlen(e.name);
        put32(file, 0x04034b50u);
        put16(file, 20);  // version needed: 2.0 (deflate)
        put16(file, 0);   // flags: sizes and CRC in this header, no data descriptor
        put16(file, method);
        put16(file, dos_time);
        put16(file, dos_date);
        put32(file, e.crc);
        put32(file, e.csize);
        put32(file, e.usize);
        put16(file, (uint32_t)nlen);
        put16(file, 0);
        file.insert(file.end(), e.name, e.name + nlen);
        file.insert(file.end(), body->begin(), body->end());
    }
    const uint32_t cd_off = (uint32_t)file.size();
    for (const Entry& e : ent) {
        const size_t nlen = strlen(e.name);
        put32(file, 0x02014b50u);
        put16(file, 3u << 8 | 20);  // made by: unix, 2.0
        put16(file, 20);
        put16(file, 0);
        put16(file, method);
        put16(file, dos_time);
        put16(file, dos_date);
        put32(file, e.crc);
        put32(file, e.csize);
        put32(file, e.usize);
        put16(file, (uint32_t)nlen);
        put16(file, 0);  // extra
        put16(file, 0);  // comment
        put16(file, 0);  // disk
        put16(file, 0);  // internal attributes
        put32(file, 0100644u << 16);
        put32(file, e.offset);
        file.insert(file.end(), e.name, e.name + nlen);
    }
    const uint32_t cd_size = (uint32_t)file.size() - cd_off;
    put32(file, 0x06054b50u);
    put16(file, 0);
    put16(file, 0);
    put16(file, 3);
    put16(file, 3);
    put32(file, cd_size);
    put32(file, cd_off);
    put16(file, 0);
    return true;
}

std::atomic<unsigned> g_tmp_serial{0};

// `file` at `path`, by way of a temporary file in the same directory and rename(2)
bool write_atomic(const char* path, const std::vector<unsigned char>& file, std::string& why) {
    const std::string tmp = std::string(path) + ".tmp." + std::to_string((long)getpid()) + "." +
                            std::to_string(g_tmp_serial.fetch_add(1));
    const int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL, 0666);
    if (fd < 0) {
        why = std::string("cannot create the temporary file (") + strerror(errno) + ")";
        return false;
    }
    size_t put = 0;
    bool ok = true;
    while (put < file.size()) {
        const ssize_t r = write(fd, file.data() + put, file.size() - put);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) {
            why = std::string("write failed (") + strerror(errno) + ")";
            ok = false;
            break;
        }
        put += (size_t)r;
    }
    if (close(fd) != 0 && ok) {
        why = std::string("close failed (") + strerror(errno) + ")";
        ok = false;
    }
    if (ok && rename(tmp.c_str(), path) != 0) {
        why = std::string("cannot rename over the target (") + strerror(errno) + ")";
        ok = false;
    }
    if (!ok) unlink(tmp.c_str());
    return ok;
}

}  // namespace

extern "C" int sd_write_cache_batch(const char* const* paths, int n, int H, int W, const uint8_t* left,
                                    const uint8_t* right, const uint16_t* disp_f16, int compress, int threads, char* err,
                                    int errlen) {
    if (!paths || n < 0 || H <= 0 || W <= 0 || !left || !right || !disp_f16) {
        if (err && errlen > 0) snprintf(err, (size_t)errlen, "sd_write_cache_batch: bad args");
        return -1;
    }
    if (threads > 16) threads = 16;  // a fixed ceiling, not the machine's CPU count
    if (threads < 1) threads = 1;
    if (threads > n) threads = n > 0 ? n : 1;
    const size_t rgb = (size_t)H * W * 3, hw = (size_t)H * W;
    std::atomic<int> next{0}, first_bad{n};
    std::mutex mu;
    std::string bad_why;
    auto work = [&]() {
        std::vector<unsigned char> file, member, packed;
        std::string why;
        for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) {
            bool ok = paths[i] != nullptr;
            if (!ok) why = "null path";
            if (ok) ok = compose_npz(H, W, left + i * rgb, right + i * rgb, disp_f16 + i * hw, compress != 0, file, member,
                                     packed, why);
            if (ok) ok = write_atomic(paths[i], file, why);
            if (!ok) {
                std::lock_guard<std::mutex> g(mu);
                if (i < first_bad.load()) {
                    first_bad.store(i);
                    bad_why = why;
                }
            }
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    const int bad = first_bad.load();
    if (bad < n) {
        if (err && errlen > 0)
            snprintf(err, (size_t)errlen, "%s: %s", paths[bad] ? paths[bad] : "(null)", bad_why.c_str());
        return bad + 1;
    }
    return 0;
}

// ------------------------------------------------------------------ PNG frames (the un-cached source)
// FoundationStereo frames and the RGB24 disparity codec images (reference dataset.py:23-30,184-212) are 8-bit RGB
// or RGBA PNGs, not interlaced. Decoded here as PIL's Image.open(p).convert("RGB") returns them (alpha dropped);
// other PNG kinds report an error and the caller falls back to PIL.

namespace {

uint32_t be32(const unsigned char* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

bool png_header(const std::vector<unsigned char>& f, int& w, int& h, int& bpp, std::string& why) {
    static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (f.size() < 33 || memcmp(f.data(), sig, 8) != 0 || memcmp(&f[12], "IHDR", 4) != 0) {
        why = "not a PNG";
        return false;
    }
    w = (int)be32(&f[16]);
    h = (int)be32(&f[20]);
    const int depth = f[24], color = f[25], interlace = f[28];
    if (depth != 8 || (color != 2 && color != 6) || interlace != 0 || f[26] != 0 || f[27] != 0) {
        why = "unsupported PNG kind (needs 8-bit RGB/RGBA, not interlaced)";
        return false;
    }
    bpp = color == 2 ? 3 : 4;
    return true;
}

unsigned char paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (unsigned char)(pa <= pb && pa <= pc ? a : (pb <= pc ? b : c));
}

bool decode_png(const std::vector<unsigned char>& f, int H, int W, unsigned char* out, std::vector<unsigned char>& z,
                std::vector<unsigned char>& raw, std::string& why) {
    int w = 0, h = 0, bpp = 0;
    if (!png_header(f, w, h, bpp, why)) return false;
    if (w != W || h != H) {
        why = "size " + std::to_string(h) + "x" + std::to_string(w) + " differs from the batch's";
        return false;
    }
    z.clear();
    for (size_t pos = 8; pos + 12 <= f.size();) {
        const uint32_t len = be32(&f[pos]);
        if (pos + 12 + (size_t)len > f.size()) break;
        const unsigned char* type = &f[pos + 4];
        if (memcmp(type, "IDAT", 4) == 0) z.insert(z.end(), f.begin() + pos + 8, f.begin() + pos + 8 + len);
        if (memcmp(type, "IEND", 4) == 0) break;
        pos += 12 + (size_t)len;
    }
    const size_t stride = (size_t)W * bpp;
    raw.resize((size_t)H * (stride + 1));
    uLongf got = (uLongf)raw.size();
    if (uncompress(raw.data(), &got, z.data(), (uLong)z.size()) != Z_OK || got != raw.size()) {
        why = "corrupt image data";
        return false;
    }
    for (int y = 0; y < H; ++y) {  // unfilter in place (filter byte, then the row)
        unsigned char* row = &raw[(size_t)y * (stride + 1) + 1];
        const unsigned char* up = y ? &raw[(size_t)(y - 1) * (stride + 1) + 1] : nullptr;
        const int ft = row[-1];
        for (size_t x = 0; x < stride; ++x) {
            const int a = x >= (size_t)bpp ? row[x - bpp] : 0, b = up ? up[x] : 0;
            const int c = (up && x >= (size_t)bpp) ? up[x - bpp] : 0;
            switch (ft) {
                case 0: break;
                case 1: row[x] = (unsigned char)(row[x] + a); break;
                case 2: row[x] = (unsigned char)(row[x] + b); break;
                case 3: row[x] = (unsigned char)(row[x] + ((a + b) >> 1)); break;
                case 4: row[x] = (unsigned char)(row[x] + paeth(a, b, c)); break;
                default: why = "bad filter type"; return false;
            }
        }
        unsigned char* o = out + (size_t)y * W * 3;
        if (bpp == 3) {
            memcpy(o, row, stride);
        } else {
            for (int x = 0; x < W; ++x) {
                o[3 * x] = row[4 * x];
                o[3 * x + 1] = row[4 * x + 1];
                o[3 * x + 2] = row[4 * x + 2];
            }
        }
    }
    return true;
}

}  // namespace

extern "C" int sd_png_size(const char* path, int* height, int* width) {
    std::vector<unsigned char> f;
    std::string why;
    int bpp = 0;
    if (!path || !height || !width || !read_file(path, f, why) || !png_header(f, *width, *height, bpp, why)) return -1;
    return 0;
}

extern "C" int sd_read_png_batch(const char* const* paths, int n, int H, int W, uint8_t* out, int threads, char* err,
                                 int errlen) {
    if (!paths || n < 0 || H <= 0 || W <= 0 || !out) {
        if (err && errlen > 0) snprintf(err, (size_t)errlen, "sd_read_png_batch: bad args");
        return -1;
    }
    if (threads < 1) threads = 1;
    if (threads > n) threads = n > 0 ? n : 1;
    std::atomic<int> next{0}, first_bad{n};
    std::mutex mu;
    std::string bad_why;
    auto work = [&]() {
        std::vector<unsigned char> buf, z, raw;
        std::string why;
        for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) {
            bool ok = paths[i] && read_file(paths[i], buf, why);
            if (ok) ok = decode_png(buf, H, W, out + (size_t)i * H * W * 3, z, raw, why);
            if (!ok) {
                std::lock_guard<std::mutex> g(mu);
                if (i < first_bad.load()) {
                    first_bad.store(i);
                    bad_why = why;
                }
            }
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    const int bad = first_bad.load();
    if (bad < n) {
        if (err && errlen > 0)
            snprintf(err, (size_t)errlen, "%s: %s", paths[bad] ? paths[bad] : "(null)", bad_why.c_str());
        return bad + 1;
    }
    return 0;
}

// ------------------------------------------------------------------ the PNG writer (disparity files of predict.py)
// n RGB images from the buffers the device filled -> 8-bit RGB PNGs a reader of the dataset's disparity files takes
// (sd_read_png_batch, PIL, the reference's loader): not interlaced, filter type 0 on every row (the codes of a disparity
// image are no smoother after a filter, and the choice costs a pass), one zlib stream in one IDAT chunk. Composed in
// memory and written through write_atomic, so a target is never a partial file.

namespace {

void put_be32(std::vector<unsigned char>& o, uint32_t v) {
    o.push_back((unsigned char)(v >> 24));
    o.push_back((unsigned char)(v >> 16));
    o.push_back((unsigned char)(v >> 8));
    o.push_back((unsigned char)v);
}

// length, type, data, CRC over type + data; `o` already ends with the data of `len` bytes after the 8-byte head at `at`
void close_chunk(std::vector<unsigned char>& o, size_t at) {
    const size_t len = o.size() - at - 8;
    o[at] = (unsigned char)(len >> 24), o[at + 1] = (unsigned char)(len >> 16);
    o[at + 2] = (unsigned char)(len >> 8), o[at + 3] = (unsigned char)len;
    uLong crc = crc32(0L, Z_NULL, 0);
    for (size_t pos = at + 4; pos < o.size();) {  // crc32 takes a uInt length
        const size_t step = o.size() - pos < ((size_t)1 << 30) ? o.size() - pos : ((size_t)1 << 30);
        crc = crc32(crc, o.data() + pos, (uInt)step);
        pos += step;
    }
    put_be32(o, (uint32_t)crc);
}
size_t open_chunk(std::vector<unsigned char>& o, const char* type) {
    const size_t at = o.size();
    put_be32(o, 0);
    o.insert(o.end(), type, type + 4);
    return at;
}

bool compose_png(int H, int W, const uint8_t* rgb, int level, std::vector<unsigned char>& file,
                 std::vector<unsigned char>& raw, std::string& why) {
    const size_t stride = (size_t)W * 3;
    if ((stride + 1) * (size_t)H >= ((size_t)1 << 31)) {
        why = "image too large for one IDAT chunk";
        return false;
    }
    raw.resize((stride + 1) * (size_t)H);
    for (int y = 0; y < H; ++y) {
        unsigned char* row = &raw[(size_t)y * (stride + 1)];
        row[0] = 0;  // filter type 0: None
        memcpy(row + 1, rgb + (size_t)y * stride, stride);
    }
    static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    file.clear();
    file.insert(file.end(), sig, sig + 8);
    size_t at = open_chunk(file, "IHDR");
    put_be32(file, (uint32_t)W);
    put_be32(file, (uint32_t)H);
    file.insert(file.end(), {8, 2, 0, 0, 0});  // depth 8, colour type 2 (RGB), deflate, adaptive filtering, no interlace
    close_chunk(file, at);
    at = open_chunk(file, "IDAT");
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (deflateInit(&zs, level) != Z_OK) {
        why = "deflateInit failed";
        return false;
    }
    const size_t head = file.size();
    file.resize(head + deflateBound(&zs, (uLong)raw.size()));
    zs.next_in = raw.data();
    zs.avail_in = (uInt)raw.size();
    zs.next_out = file.data() + head;
    zs.avail_out = (uInt)(file.size() - head);
    const int rc = deflate(&zs, Z_FINISH);
    const size_t packed = zs.total_out;
    deflateEnd(&zs);
    if (rc != Z_STREAM_END) {
        why = "deflate failed";
        return false;
    }
    file.resize(head + packed);
    close_chunk(file, at);
    at = open_chunk(file, "IEND");
    close_chunk(file, at);
    return true;
}

}  // namespace

extern "C" int sd_write_png_batch(const char* const* paths, int n, int H, int W, const uint8_t* rgb, int level,
                                  int threads, char* err, int errlen) {
    if (!paths || n < 0 || H <= 0 || W <= 0 || !rgb || level < 0 || level > 9) {
        if (err && errlen > 0) snprintf(err, (size_t)errlen, "sd_write_png_batch: bad args");
        return -1;
    }
    if (threads > 16) threads = 16;  // a fixed ceiling, not the machine's CPU count
    if (threads < 1) threads = 1;
    if (threads > n) threads = n > 0 ? n : 1;
    const size_t img = (size_t)H * W * 3;
    std::atomic<int> next{0}, first_bad{n};
    std::mutex mu;
    std::string bad_why;
    auto work = [&]() {
        std::vector<unsigned char> file, raw;
        std::string why;
        for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) {
            bool ok = paths[i] != nullptr;
            if (!ok) why = "null path";
            if (ok) ok = compose_png(H, W, rgb + i * img, level, file, raw, why);
            if (ok) ok = write_atomic(paths[i], file, why);
            if (!ok) {
                std::lock_guard<std::mutex> g(mu);
                if (i < first_bad.load()) {
                    first_bad.store(i);
                    bad_why = why;
                }
            }
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    const int bad = first_bad.load();
    if (bad < n) {
        if (err && errlen > 0)
            snprintf(err, (size_t)errlen, "%s: %s", paths[bad] ? paths[bad] : "(null)", bad_why.c_str());
        return bad + 1;
    }
    return 0;
}
