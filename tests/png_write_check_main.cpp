// Stand-alone check of csrc/cache_io.cpp's PNG writer (tests/test_png_write_cpu.py builds this file and cache_io.cpp
// with -fsanitize=address,undefined into one program and runs it on a scratch directory):
// sd_write_png_batch -> sd_read_png_batch / sd_png_size round trips at every zlib level, and the writer's failure cases.
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

// random images; the second one smooth, as a disparity file is (long matches for the deflate search)
std::vector<uint8_t> images(int n, int H, int W) {
    std::vector<uint8_t> v((size_t)n * H * W * 3);
    for (auto& b : v) b = (uint8_t)rnd();
    if (n > 1)
        for (size_t i = 0; i < (size_t)H * W; ++i) {
            uint8_t* px = &v[((size_t)H * W + i) * 3];
            px[0] = 0, px[1] = (uint8_t)(i * 37 / 255 % 255), px[2] = (uint8_t)(i * 37 % 255);
        }
    return v;
}

void round_trip(const std::string& dir, int H, int W, int level, int threads) {
    const int n = 5;
    const std::vector<uint8_t> img = images(n, H, W);
    std::vector<std::string> names;
    std::vector<const char*> paths;
    for (int i = 0; i < n; ++i)
        names.push_back(dir + "/rt_" + std::to_string(H) + "_" + std::to_string(level) + "_" + std::to_string(i) + ".png");
    for (auto& s : names) paths.push_back(s.c_str());
    char err[512] = "";
    CHECK(sd_write_png_batch(paths.data(), n, H, W, img.data(), level, threads, err, (int)sizeof err) == 0);
    std::vector<uint8_t> back(img.size(), 0xee);
    CHECK(sd_read_png_batch(paths.data(), n, H, W, back.data(), 3, err, (int)sizeof err) == 0);
    CHECK(back == img);
    int h = 0, w = 0;
    CHECK(sd_png_size(paths[n - 1], &h, &w) == 0 && h == H && w == W);
    // another size is refused by the reader: the header carries this one
    CHECK(sd_read_png_batch(paths.data(), n, H + 1, W, back.data(), 1, err, (int)sizeof err) == 1);
}

void failure_cases(const std::string& dir) {
    const int H = 7, W = 5;
    const std::vector<uint8_t> img = images(4, H, W);
    const std::string good = dir + "/good";
    mkdir(good.c_str(), 0777);
    const std::string p0 = good + "/0.png", p1 = good + "/1.png", bad = dir + "/missing/2.png", p3 = good + "/3.png";
    const char* paths[4] = {p0.c_str(), p1.c_str(), bad.c_str(), p3.c_str()};
    char err[512] = "";
    CHECK(sd_write_png_batch(paths, 4, H, W, img.data(), 1, 4, err, (int)sizeof err) == 3);
    CHECK(strstr(err, bad.c_str()) != nullptr);
    CHECK(list_dir(good).size() == 3);  // 0, 1, 3: no temporary file
    CHECK(list_dir(dir + "/missing").empty());
    // a tiny err buffer is not overrun; none at all is accepted
    char tiny[8];
    CHECK(sd_write_png_batch(paths, 4, H, W, img.data(), 6, 2, tiny, (int)sizeof tiny) == 3);
    CHECK(strlen(tiny) < sizeof tiny);
    CHECK(sd_write_png_batch(paths, 4, H, W, img.data(), 6, 2, nullptr, 0) == 3);
    // an existing file whose temporary name would be too long for the file system keeps its bytes
    const std::string old = good + "/" + std::string(246, 'x') + ".png";
    if (FILE* f = fopen(old.c_str(), "wb")) {
        fputs("an earlier file", f);
        fclose(f);
    }
    const char* paths2[3] = {p0.c_str(), old.c_str(), p3.c_str()};
    CHECK(sd_write_png_batch(paths2, 3, H, W, img.data(), 0, 16, err, (int)sizeof err) == 2);
    CHECK(slurp(old) == "an earlier file");
    CHECK(list_dir(good).size() == 4);
    // an existing target is replaced whole
    if (FILE* f = fopen(p0.c_str(), "wb")) {
        fputs(std::string(100000, 'x').c_str(), f);
        fclose(f);
    }
    CHECK(sd_write_png_batch(paths, 1, H, W, img.data(), 9, 1, err, (int)sizeof err) == 0);
    CHECK(slurp(p0).size() < 1000);
    // bad arguments, an empty batch, more threads than files, a null path
    CHECK(sd_write_png_batch(nullptr, 1, H, W, img.data(), 1, 1, err, (int)sizeof err) == -1);
    CHECK(sd_write_png_batch(paths, 4, 0, W, img.data(), 1, 1, err, (int)sizeof err) == -1);
    CHECK(sd_write_png_batch(paths, 4, H, W, nullptr, 1, 1, err, (int)sizeof err) == -1);
    CHECK(sd_write_png_batch(paths, 4, H, W, img.data(), 10, 1, err, (int)sizeof err) == -1);
    CHECK(sd_write_png_batch(paths, 4, H, W, img.data(), -1, 1, err, (int)sizeof err) == -1);
    CHECK(sd_write_png_batch(paths, 0, H, W, img.data(), 1, 64, err, (int)sizeof err) == 0);
    const char* with_null[2] = {p0.c_str(), nullptr};
    CHECK(sd_write_png_batch(with_null, 2, H, W, img.data(), 1, 64, err, (int)sizeof err) == 2);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        printf("usage: %s SCRATCH_DIR\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const int shapes[4][2] = {{1, 1}, {17, 23}, {45, 61}, {64, 256}};
    const int levels[4] = {0, 1, 6, 9};
    for (const auto& hw : shapes)
        for (int level : levels) round_trip(dir, hw[0], hw[1], level, level == 1 ? 16 : 2);
    failure_cases(dir);
    if (failures) return 1;
    printf("png_write_check: ok\n");
    return 0;
}
