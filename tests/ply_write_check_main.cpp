// Stand-alone check of csrc/ply_io.cpp (tests/test_cloud_cpu.py builds this file and ply_io.cpp with
// -fsanitize=address,undefined into one program and runs it on a scratch directory): sd_write_ply_batch's files byte for
// byte at counts 0, 1, cap and above cap, and the writer's failure cases.
#include <dirent.h>
#include <sys/stat.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "stereo_hip.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                               \
        }                                                             \
    } while (0)

uint32_t rng_state = 2463534242u;
uint32_t rnd() {  // xorshift32
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}

std::vector<std::string> list_dir(const std::string& dir) {
    std::vector<std::string> out;
    if (DIR* d = opendir(dir.c_str())) {
        while (dirent* e = readdir(d))
            if (strcmp(e->d_name, ".") != 0 && strcmp(e->d_name, "..") != 0) out.push_back(e->d_name);
        closedir(d);
    }
    return out;
}

std::string slurp(const std::string& path) {
    std::string s;
    if (FILE* f = fopen(path.c_str(), "rb")) {
        char buf[4096];
        for (size_t r; (r = fread(buf, 1, sizeof buf, f)) > 0;) s.append(buf, r);
        fclose(f);
    }
    return s;
}

std::string header(unsigned long long n) {
    return "ply\nformat binary_little_endian 1.0\nelement vertex " + std::to_string(n) +
           "\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\n"
           "property uchar blue\nproperty uchar alpha\nend_header\n";
}

std::vector<uint8_t> records(int n, long long cap) {
    std::vector<uint8_t> v((size_t)n * cap * 16);
    for (auto& b : v) b = (uint8_t)rnd();
    return v;
}

void round_trip(const std::string& dir, long long cap, int threads) {
    const int n = 5;
    const std::vector<uint8_t> pts = records(n, cap);
    // empty, one point, full, above cap (clamped), all bits set (clamped)
    const unsigned counts[n] = {0u, 1u, (unsigned)cap, (unsigned)cap + 7u, 0xffffffffu};
    std::vector<std::string> names;
    std::vector<const char*> paths;
    for (int i = 0; i < n; ++i) names.push_back(dir + "/rt_" + std::to_string(cap) + "_" + std::to_string(i) + ".ply");
    for (auto& s : names) paths.push_back(s.c_str());
    char err[512] = "";
    CHECK(sd_write_ply_batch(paths.data(), n, pts.data(), cap, counts, threads, err, (int)sizeof err) == 0);
    for (int i = 0; i < n; ++i) {
        const unsigned long long k = counts[i] < (unsigned long long)cap ? counts[i] : (unsigned long long)cap;
        const std::string want =
            header(k) + std::string((const char*)pts.data() + (size_t)i * cap * 16, (size_t)k * 16);
        CHECK(slurp(names[i]) == want);
    }
}

void failure_cases(const std::string& dir) {
    const long long cap = 9;
    const std::vector<uint8_t> pts = records(4, cap);
    const unsigned counts[4] = {3, 9, 4, 0};
    const std::string good = dir + "/good";
    mkdir(good.c_str(), 0777);
    const std::string p0 = good + "/0.ply", p1 = good + "/1.ply", bad = dir + "/missing/2.ply", p3 = good + "/3.ply";
    const char* paths[4] = {p0.c_str(), p1.c_str(), bad.c_str(), p3.c_str()};
    char err[512] = "";
    CHECK(sd_write_ply_batch(paths, 4, pts.data(), cap, counts, 4, err, (int)sizeof err) == 3);
    CHECK(strstr(err, bad.c_str()) != nullptr);
    CHECK(list_dir(good).size() == 3);  // 0, 1, 3: no temporary file
    CHECK(list_dir(dir + "/missing").empty());
    CHECK(slurp(p3) == header(0));  // an empty cloud is a valid file
    // a tiny err buffer is not overrun; none at all is accepted
    char tiny[8];
    CHECK(sd_write_ply_batch(paths, 4, pts.data(), cap, counts, 2, tiny, (int)sizeof tiny) == 3);
    CHECK(strlen(tiny) < sizeof tiny);
    CHECK(sd_write_ply_batch(paths, 4, pts.data(), cap, counts, 2, nullptr, 0) == 3);
    // an existing file whose temporary name would be too long for the file system keeps its bytes
    const std::string old = good + "/" + std::string(246, 'x') + ".ply";
    if (FILE* f = fopen(old.c_str(), "wb")) {
        fputs("an earlier file", f);
        fclose(f);
    }
    const char* paths2[3] = {p0.c_str(), old.c_str(), p3.c_str()};
    CHECK(sd_write_ply_batch(paths2, 3, pts.data(), cap, counts, 16, err, (int)sizeof err) == 2);
    CHECK(slurp(old) == "an earlier file");
    CHECK(list_dir(good).size() == 4);
    // an existing target is replaced whole
    if (FILE* f = fopen(p0.c_str(), "wb")) {
        fputs(std::string(100000, 'x').c_str(), f);
        fclose(f);
    }
    CHECK(sd_write_ply_batch(paths, 1, pts.data(), cap, counts, 1, err, (int)sizeof err) == 0);
    CHECK(slurp(p0).size() == header(3).size() + 3 * 16);
    // several failures: the lowest index is reported
    const std::string bad2 = dir + "/missing/b.ply";
    const char* paths3[3] = {bad.c_str(), p0.c_str(), bad2.c_str()};
    CHECK(sd_write_ply_batch(paths3, 3, pts.data(), cap, counts, 3, err, (int)sizeof err) == 1);
    CHECK(strstr(err, bad.c_str()) != nullptr);
    // bad arguments, an empty batch, more threads than files, a null path
    CHECK(sd_write_ply_batch(nullptr, 1, pts.data(), cap, counts, 1, err, (int)sizeof err) == -1);
    CHECK(sd_write_ply_batch(paths, -1, pts.data(), cap, counts, 1, err, (int)sizeof err) == -1);
    CHECK(sd_write_ply_batch(paths, 4, nullptr, cap, counts, 1, err, (int)sizeof err) == -1);
    CHECK(sd_write_ply_batch(paths, 4, pts.data(), 0, counts, 1, err, (int)sizeof err) == -1);
    CHECK(sd_write_ply_batch(paths, 4, pts.data(), cap, nullptr, 1, err, (int)sizeof err) == -1);
    CHECK(sd_write_ply_batch(paths, 0, pts.data(), cap, counts, 64, err, (int)sizeof err) == 0);
    const char* with_null[2] = {p0.c_str(), nullptr};
    CHECK(sd_write_ply_batch(with_null, 2, pts.data(), cap, counts, 64, err, (int)sizeof err) == 2);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        printf("usage: %s SCRATCH_DIR\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const long long caps[4] = {1, 2, 37, 5000};
    for (long long cap : caps) round_trip(dir, cap, cap == 37 ? 16 : 2);
    failure_cases(dir);
    if (failures) return 1;
    printf("ply_write_check: ok\n");
    return 0;
}
