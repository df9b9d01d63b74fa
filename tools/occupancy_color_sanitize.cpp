// Stand-alone host check of the ColorOcTree stream parser (sbm_occ_color_ot_info, sbm_occ_color_ot_leaves) under AddressSanitizer
// and UndefinedBehaviorSanitizer: every truncation of each stream given, and every byte of it set to 0x00, 0xFF, 0x03, 0x55 and
// 0xAA (every seventh byte for a stream above 4000 bytes), each from an exact-size heap copy so that a read past the end is seen;
// and hostile headers made here: sizes that overflow eight times themselves, a size beyond the body, no body at all.
// Built and run by hand on the host: the parser's two files are host C++ (no HIP header, no HIP call), so the tool and they are
// the whole program, under any C++17 compiler; it never touches a GPU:
//
//     c++ -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include \
//         u96-slam_amd/csrc/sbm_occ_bt.hip u96-slam_amd/csrc/sbm_occ_color_host.hip tools/occupancy_color_sanitize.cpp -o occ_color_san
//     ASAN_OPTIONS=detect_leaks=0 ./occ_color_san a.ot b.ot ...
//
// Prints the number of calls and how many streams were accepted; a finding ends the run with the sanitizer's report.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "sbm.h"
static std::vector<uint8_t> slurp(const char* p) {
  std::vector<uint8_t> v; FILE* f = fopen(p, "rb"); if (!f) return v;
  for (int c; (c = fgetc(f)) != EOF;) v.push_back((uint8_t)c);
  fclose(f); return v;
}
static long run(const uint8_t* b, size_t n) {
  // an exact-size heap copy, so that a read past the end is seen
  uint8_t* copy = new uint8_t[n ? n : 1];
  memcpy(copy, b, n);
  sbm_occ_ot_header h;
  int st = sbm_occ_color_ot_info(copy, n, &h);
  size_t count = 0;
  int st2 = sbm_occ_color_ot_leaves(copy, n, nullptr, nullptr, nullptr, nullptr, 0, &count);
  if (st == SBM_OK && count) {
    std::vector<uint64_t> k(count); std::vector<int32_t> d(count); std::vector<float> v(count); std::vector<uint32_t> c(count);
    st2 = sbm_occ_color_ot_leaves(copy, n, k.data(), d.data(), v.data(), c.data(), count, &count);
    if (st2 != SBM_OK || count != h.leaves) { printf("inconsistent %d %d\n", st, st2); }
    for (uint32_t w : c) if (w >> 24) { printf("a colour word with a top byte\n"); }
  }
  delete[] copy;
  return st;
}
int main(int argc, char** argv) {
  long calls = 0, ok = 0;
  for (int a = 1; a < argc; a++) {
    std::vector<uint8_t> v = slurp(argv[a]);
    for (size_t cut = 0; cut <= v.size(); cut++) { ok += run(v.data(), cut) == SBM_OK; calls++; }
    const size_t step = v.size() > 4000 ? 7 : 1;
    for (size_t i = 0; i < v.size(); i += step)
      for (int x : {0x00, 0xFF, 0x03, 0x55, 0xAA}) {
        std::vector<uint8_t> w = v; w[i] = (uint8_t)x; ok += run(w.data(), w.size()) == SBM_OK; calls++;
      }
  }
  for (const char* size : {"0", "1", "2305843009213693952", "18446744073709551615", "4611686018427387904", "-1", "99999999999999999999999"}) {
    std::string s = std::string("# Octomap OcTree file\nid ColorOcTree\nsize ") + size + "\nres 0.1\ndata\n";
    ok += run((const uint8_t*)s.data(), s.size()) == SBM_OK; calls++;
    s += std::string(16, '\x7f');
    ok += run((const uint8_t*)s.data(), s.size()) == SBM_OK; calls++;
  }
  printf("calls %ld accepted %ld\n", calls, ok);
  return 0;
}
