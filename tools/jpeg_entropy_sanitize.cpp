// Stand-alone sanitizer harness for the HOST side of the device-side JPEG entropy decode: editor_jpeg_plan,
// editor_jpeg_entropy_segments (the routine jpeg_entropy_kernel runs, compiled for the CPU) and editor_jpeg_entropy_split_segments
// (the routines jpeg_entropy_split_kernel runs, at sub_bytes 16 and 64, whose status and - for status 0 - coefficients must equal
// the former's).  For every file given: a cut every 7
// bytes (the sweep of tests/test_jpeg_host.py) and, for files under 6000 bytes, every single-bit flip of the whole file, each from
// an exact-size heap copy so an overrun of one byte is seen.  Host code only; nothing here touches a GPU.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         editor_amd/csrc/jpeg.hip tools/jpeg_entropy_sanitize.cpp -o jpeg_entropy_sanitize
//   ./jpeg_entropy_sanitize file.jpg ...        (prints how many inputs took which route; any finding aborts)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <stdint.h>
extern "C" int editor_jpeg_plan(const uint8_t*, long, int*, int*, uint16_t*, uint8_t*, long*, long);
extern "C" int editor_jpeg_entropy_segments(const uint8_t*, long, const int*, const long*, const long*, const uint8_t*, int, int, long, int16_t*,
                                            long, int*);
extern "C" int editor_jpeg_entropy_split_workspace(long, int, long*);
extern "C" int editor_jpeg_entropy_split_segments(const uint8_t*, long, const int*, const long*, const long*, const uint8_t*, int, int, long, int, void*,
                                                  long, int16_t*, long, int*);

static std::vector<uint8_t> read_file(const char* p)
{
    std::vector<uint8_t> v;
    FILE* f = fopen(p, "rb");
    if (!f) return v;
    int c;
    while ((c = fgetc(f)) != EOF) v.push_back((uint8_t)c);
    fclose(f);
    return v;
}

static int one(const uint8_t* d, long n, long* stats)
{
    std::vector<uint8_t> file(d, d + n);
    int info[16], plan[16];
    std::vector<uint16_t> qt(192);
    std::vector<uint8_t> huff(8 * 272);
    std::vector<long> seg(3 * 4096);
    int rc = editor_jpeg_plan(file.data(), n, info, plan, qt.data(), huff.data(), seg.data(), 4096);
    if (rc) { stats[0]++; return 0; }
    if (!plan[0] || plan[1] > 4096) { stats[1]++; return 0; }
    const long s0 = seg[0], e1 = seg[3 * (plan[1] - 1) + 1];
    std::vector<uint8_t> bytes(file.begin() + s0, file.begin() + e1);
    if (bytes.empty()) bytes.push_back(0);
    int fdesc[16] = {info[2], info[3], info[4], info[5], info[6], plan[2], 0, 1, 2, 3, 4, 5, 0, 0, 0, 0};
    std::vector<uint8_t> pool;
    for (int c = 0; c < 3; ++c) pool.insert(pool.end(), huff.begin() + 272 * plan[4 + c], huff.begin() + 272 * (plan[4 + c] + 1));
    for (int c = 0; c < 3; ++c) pool.insert(pool.end(), huff.begin() + 272 * (4 + plan[7 + c]), huff.begin() + 272 * (5 + plan[7 + c]));
    long ftab[3] = {0, -s0, plan[1]};
    std::vector<long> segs(seg.begin(), seg.begin() + 3 * plan[1]);
    std::vector<int16_t> coef((size_t)info[8] * 64);
    int status = -1;
    rc = editor_jpeg_entropy_segments(bytes.data(), e1 - s0, fdesc, ftab, segs.data(), pool.data(), 6, 1, plan[1], coef.data(), info[8], &status);
    if (rc) { printf("tables refused: %d\n", rc); return 1; }
    stats[status ? 3 : 2]++;
    for (int sub : {16, 64}) {
        long need = 0;
        if (editor_jpeg_entropy_split_workspace(plan[1], sub, &need)) { printf("workspace query refused\n"); return 1; }
        std::vector<long> ws((size_t)need / 8);
        // decoded twice into buffers that start out different: what comes back equal was written (a damaged stream can
        // decode to any value, so no single fill pattern proves that)
        std::vector<int16_t> coef2((size_t)info[8] * 64, (int16_t)0x5A5A), coef3((size_t)info[8] * 64, (int16_t)0x25A5);
        int status2 = -1, status3 = -1;
        rc = editor_jpeg_entropy_split_segments(bytes.data(), e1 - s0, fdesc, ftab, segs.data(), pool.data(), 6, 1, plan[1], sub, ws.data(), need,
                                                coef2.data(), info[8], &status2);
        if (rc) { printf("split: tables refused: %d\n", rc); return 1; }
        rc = editor_jpeg_entropy_split_segments(bytes.data(), e1 - s0, fdesc, ftab, segs.data(), pool.data(), 6, 1, plan[1], sub, ws.data(), need,
                                                coef3.data(), info[8], &status3);
        if (rc || status2 != status || status3 != status) { printf("split %d: status %d, %d against %d (%ld bytes)\n", sub, status2, status3, status, n); return 1; }
        if (!status && memcmp(coef.data(), coef2.data(), coef.size() * 2)) { printf("split %d: coefficients differ (%ld bytes)\n", sub, n); return 1; }
        if (memcmp(coef2.data(), coef3.data(), coef2.size() * 2)) { printf("split %d: a block was left unwritten (%ld bytes)\n", sub, n); return 1; }
    }
    return 0;
}

int main(int argc, char** argv)
{
    long stats[4] = {0, 0, 0, 0};
    for (int a = 1; a < argc; ++a) {
        std::vector<uint8_t> v = read_file(argv[a]);
        if (v.empty()) return 2;
        for (long cut = 2; cut <= (long)v.size(); cut += 7)
            if (one(v.data(), cut, stats)) return 1;
        if (one(v.data(), (long)v.size(), stats)) return 1;
        if (v.size() < 6000)
            for (long bit = 0; bit < 8 * (long)v.size(); ++bit) {
                v[bit / 8] ^= 0x80 >> (bit % 8);
                if (one(v.data(), (long)v.size(), stats)) return 1;
                v[bit / 8] ^= 0x80 >> (bit % 8);
            }
    }
    printf("refused by the planner %ld, host-routed %ld, decoded rc 0 %ld, decoded rc 9001 %ld\n", stats[0], stats[1], stats[2], stats[3]);
    return 0;
}
