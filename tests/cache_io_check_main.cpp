// Stand-alone check of csrc/cache_io.cpp's cache writer and reader (tests/test_cache_write_cpu.py builds this file and
// cache_io.cpp with -fsanitize=address,undefined into one program and runs it on a scratch directory):
// sd_write_cache_batch -> sd_read_cache_batch round trips, stored and deflated, and the writer's failure cases.
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

uint32_t rng_state = 12345u;
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

struct Batch {
    int n, H, W;
    std::vector<uint8_t> left, right;
    std::vector<uint16_t> disp;
    Batch(int n_, int H_, int W_) : n(n_), H(H_), W(W_), left((size_t)n_ * H_ * W_ * 3), right(left.size()), disp((size_t)n_ * H_ * W_) {
        for (auto& v : left) v = (uint8_t)rnd();
        for (auto& v : right) v = (uint8_t)rnd();
        for (auto& v : disp) v = (uint16_t)(rnd() % 0x7c01u);  // any non-negative float16 up to +inf
        // +-0, subnormals, the smallest normal, 1.0, 2048 and above, the largest finite value, +inf
        const uint16_t special[] = {0x0000, 0x8000, 0x0001, 0x03ff, 0x0400, 0x3c00, 0x6800, 0x6801, 0x7000, 0x7bff, 0x7c00};
        for (size_t i = 0; i < sizeof special / sizeof *special && i < disp.size(); ++i) disp[i * 3 % disp.size()] = special[i];
    }
};

void round_trip(const std::string& dir, int H, int W, int compress, int threads) {
    const int n = 5;
    Batch b(n, H, W);
    std::vector<std::string> names;
    std::vector<const char*> paths;
    for (int i = 0; i < n; ++i)
        names.push_back(dir + "/rt_" + std::to_string(H) + "_" + std::to_string(compress) + "_" + std::to_string(i) + ".npz");
    for (auto& s : names) paths.push_back(s.c_str());
    char err[512] = "";
    CHECK(sd_write_cache_batch(paths.data(), n, H, W, b.left.data(), b.right.data(), b.disp.data(), compress, threads, err,
                               (int)sizeof err) == 0);
    std::vector<uint8_t> left(b.left.size(), 0xee), right(b.right.size(), 0xee);
    std::vector<uint16_t> disp(b.disp.size(), 0xeeee);
    CHECK(sd_read_cache_batch(paths.data(), n, H, W, left.data(), right.data(), disp.data(), 3, err, (int)sizeof err) == 0);
    CHECK(left == b.left);
    CHECK(right == b.right);
    CHECK(disp == b.disp);
    // another shape is refused by the reader: the headers carry this one
    CHECK(sd_read_cache_batch(paths.data(), n, H + 1, W, left.data(), right.data(), disp.data(), 1, err, (int)sizeof err) == 1);
}

void failure_cases(const std::string& dir) {
    const int H = 7, W = 5;
    Batch b(4, H, W);
    const std::string good = dir + "/good";
    mkdir(good.c_str(), 0777);
    const std::string p0 = good + "/0.npz", p1 = good + "/1.npz", bad = dir + "/missing/2.npz", p3 = good + "/3.npz";
    const char* paths[4] = {p0.c_str(), p1.c_str(), bad.c_str(), p3.c_str()};
    char err[512] = "";
    CHECK(sd_write_cache_batch(paths, 4, H, W, b.left.data(), b.right.data(), b.disp.data(), 0, 4, err, (int)sizeof err) == 3);
    CHECK(strstr(err, bad.c_str()) != nullptr);
    CHECK(list_dir(good).size() == 3);  // 0, 1, 3: no temporary file
    CHECK(list_dir(dir + "/missing").empty());
    // a tiny err buffer is not overrun
    char tiny[8];
    CHECK(sd_write_cache_batch(paths, 4, H, W, b.left.data(), b.right.data(), b.disp.data(), 1, 2, tiny, (int)sizeof tiny) == 3);
    CHECK(strlen(tiny) < sizeof tiny);
    CHECK(sd_write_cache_batch(paths, 4, H, W, b.left.data(), b.right.data(), b.disp.data(), 1, 2, nullptr, 0) == 3);
    // an existing entry whose temporary name would be too long for the file system keeps its bytes
    const std::string old = good + "/" + std::string(246, 'x') + ".npz";
    if (FILE* f = fopen(old.c_str(), "wb")) {
        fputs("an earlier entry", f);
        fclose(f);
    }
    const char* paths2[3] = {p0.c_str(), old.c_str(), p3.c_str()};
    CHECK(sd_write_cache_batch(paths2, 3, H, W, b.left.data(), b.right.data(), b.disp.data(), 0, 16, err, (int)sizeof err) == 2);
    CHECK(slurp(old) == "an earlier entry");
    CHECK(list_dir(good).size() == 4);
    // bad arguments, an empty batch, more threads than files
    CHECK(sd_write_cache_batch(nullptr, 1, H, W, b.left.data(), b.right.data(), b.disp.data(), 0, 1, err, (int)sizeof err) == -1);
    CHECK(sd_write_cache_batch(paths, 4, 0, W, b.left.data(), b.right.data(), b.disp.data(), 0, 1, err, (int)sizeof err) == -1);
    CHECK(sd_write_cache_batch(paths, 0, H, W, b.left.data(), b.right.data(), b.disp.data(), 0, 64, err, (int)sizeof err) == 0);
    const char* with_null[2] = {p0.c_str(), nullptr};
    CHECK(sd_write_cache_batch(with_null, 2, H, W, b.left.data(), b.right.data(), b.disp.data(), 0, 64, err, (int)sizeof err) == 2);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        printf("usage: %s SCRATCH_DIR\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const int shapes[2][2] = {{24, 32}, {7, 5}};
    for (const auto& hw : shapes)
        for (int compress = 0; compress < 2; ++compress) round_trip(dir, hw[0], hw[1], compress, compress ? 16 : 2);
    failure_cases(dir);
    if (failures) return 1;
    printf("cache_io_check: ok\n");
    return 0;
}
