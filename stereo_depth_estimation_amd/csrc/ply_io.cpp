// The PLY writer of the point-cloud stage (csrc/cloud.hip): host only, no device code.
// n clouds from the record buffers the device filled -> binary little-endian PLY files whose vertex element is the
// 16-byte record itself (float x, y, z; uchar red, green, blue, alpha), so a file is its header followed by the first
// min(counts[i], cap) records of slice i, copied verbatim. File handling as cache_io.cpp's writers: a pool of threads,
// each file written under a temporary name beside its target and renamed over it, so a target is never a partial file.
#include <fcntl.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "stereo_hip.h"

namespace {

constexpr size_t PLY_RECORD = 16;

std::atomic<unsigned> g_ply_tmp_serial{0};

bool write_all(int fd, const void* data, size_t bytes, std::string& why) {
    const unsigned char* p = static_cast<const unsigned char*>(data);
    size_t put = 0;
    while (put < bytes) {
        const ssize_t r = write(fd, p + put, bytes - put);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) {
            why = std::string("write failed (") + strerror(errno) + ")";
            return false;
        }
        put += (size_t)r;
    }
    return true;
}

// header + body at `path`, by way of a temporary file in the same directory and rename(2); the records go from the
// caller's buffer to the file without a copy in between
bool write_ply_atomic(const char* path, const std::string& header, const void* body, size_t bytes, std::string& why) {
    const std::string tmp = std::string(path) + ".tmp." + std::to_string((long)getpid()) + "." +
                            std::to_string(g_ply_tmp_serial.fetch_add(1));
    const int fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL, 0666);
    if (fd < 0) {
        why = std::string("cannot create the temporary file (") + strerror(errno) + ")";
        return false;
    }
    bool ok = write_all(fd, header.data(), header.size(), why) && write_all(fd, body, bytes, why);
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

std::string ply_header(unsigned long long vertices) {
    return "ply\nformat binary_little_endian 1.0\nelement vertex " + std::to_string(vertices) +
           "\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\n"
           "property uchar blue\nproperty uchar alpha\nend_header\n";
}

}  // namespace

extern "C" int sd_write_ply_batch(const char* const* paths, int n, const void* points, long long cap,
                                  const unsigned* counts, int threads, char* err, int errlen) {
    if (!paths || n < 0 || !points || cap < 1 || !counts) {
        if (err && errlen > 0) snprintf(err, (size_t)errlen, "sd_write_ply_batch: bad args");
        return -1;
    }
    if (threads > 16) threads = 16;  // a fixed ceiling, not the machine's CPU count
    if (threads < 1) threads = 1;
    if (threads > n) threads = n > 0 ? n : 1;
    const unsigned char* base = static_cast<const unsigned char*>(points);
    std::atomic<int> next{0}, first_bad{n};
    std::mutex mu;
    std::string bad_why;
    auto work = [&]() {
        std::string why;
        for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) {
            bool ok = paths[i] != nullptr;
            if (!ok) why = "null path";
            if (ok) {
                const unsigned long long kept = counts[i] < (unsigned long long)cap ? counts[i] : (unsigned long long)cap;
                ok = write_ply_atomic(paths[i], ply_header(kept), base + (size_t)i * (size_t)cap * PLY_RECORD,
                                      (size_t)kept * PLY_RECORD, why);
            }
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
