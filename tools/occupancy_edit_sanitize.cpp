// Stand-alone host check of the edits' host arithmetic (u96-slam_amd/csrc/sbm_occ.h: occ_edit_chunks, occ_edit_chunk,
// occ_depth_mask, occ_key_in_box) under AddressSanitizer and UndefinedBehaviorSanitizer: the chunks of a batch cover every item
// once, in item order, each at most SBM_OCC_EDIT_CHUNK long -- for the sizes around every chunk boundary by touching every item of
// an exact-size heap array, so that a chunk that runs past the batch is seen, and up to the limit of 2^30 by arithmetic --; the
// depth mask for every depth a caller can pass; the box test at its corners. Built and run by hand on the host: the helpers are
// plain C++ (no HIP header, no HIP call), so the tool and the header are the whole program; it never touches a GPU:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include \
//         tools/occupancy_edit_sanitize.cpp -o occ_edit_san && ./occ_edit_san
//
// Prints the number of checks; a finding ends the run with the sanitizer's report, a wrong answer with exit code 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../u96-slam_amd/csrc/sbm_occ.h"

static long checks = 0;
static void expect(bool ok, const char* what, long long a = 0, long long b = 0) {
  checks++;
  if (ok) return;
  std::printf("wrong: %s (%lld, %lld)\n", what, a, b);
  std::exit(1);
}

int main() {
  const size_t C = SBM_OCC_EDIT_CHUNK;
  // every item once and in order, by touching an exact-size array
  for (size_t n : {(size_t)0, (size_t)1, (size_t)2, C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1, 3 * C + 7}) {
    uint8_t* seen = new uint8_t[n ? n : 1]();
    size_t next = 0;
    for (size_t c = 0; c < sbm::occ_edit_chunks(n); c++) {
      size_t begin, count;
      sbm::occ_edit_chunk(n, c, &begin, &count);
      expect(begin == next && count >= 1 && count <= C, "a chunk's place", (long long)begin, (long long)count);
      for (size_t i = begin; i < begin + count; i++) seen[i]++;
      next = begin + count;
    }
    expect(next == n, "the chunks' total", (long long)next, (long long)n);
    for (size_t i = 0; i < n; i++)
      if (seen[i] != 1) expect(false, "an item's count", (long long)i, seen[i]);
    size_t begin, count;
    sbm::occ_edit_chunk(n, sbm::occ_edit_chunks(n), &begin, &count);   // one past the last: empty
    expect(count == 0, "the chunk past the last", (long long)begin, (long long)count);
    delete[] seen;
  }
  // up to the limit, by arithmetic
  for (size_t n : {((size_t)1 << 30) - 1, (size_t)1 << 30, ((size_t)1 << 30) + 1, ~(size_t)0 / 2}) {
    const size_t chunks = sbm::occ_edit_chunks(n);
    size_t begin, count, total = 0;
    sbm::occ_edit_chunk(n, chunks - 1, &begin, &count);
    expect(begin + count == n && count >= 1 && count <= C, "the last chunk", (long long)begin, (long long)count);
    if (n <= ((size_t)1 << 30) + 1)
      for (size_t c = 0; c < chunks; c++) {
        sbm::occ_edit_chunk(n, c, &begin, &count);
        expect(begin == total, "a chunk's begin", (long long)c, (long long)begin);
        total += count;
      }
  }
  // deleteNode's depth
  uint64_t mask = 7;
  for (int d : {-2, -1, 17, 18, 1 << 30, -(1 << 30)}) expect(!sbm::occ_depth_mask(d, &mask) && mask == 7, "a depth outside 0..16", d);
  for (int d = 0; d <= 16; d++) {
    expect(sbm::occ_depth_mask(d, &mask), "a depth inside 0..16", d);
    const int bits = d ? d : 16;
    const uint64_t m = (uint64_t)(0xFFFF0000u >> bits) & 0xFFFF;
    expect(mask == (m << 32 | m << 16 | m) && !(mask >> 48), "the mask of a depth", d, (long long)mask);
  }
  // the key box, inclusive on both ends; min > max on an axis holds nothing
  const unsigned lo[3] = {10, 0, 65535}, hi[3] = {20, 0, 65535}, none_lo[3] = {5, 0, 0}, none_hi[3] = {4, 65535, 65535};
  auto key = [](uint64_t a, uint64_t b, uint64_t c) { return a << 32 | b << 16 | c; };
  expect(sbm::occ_key_in_box(key(10, 0, 65535), lo, hi) && sbm::occ_key_in_box(key(20, 0, 65535), lo, hi), "the box's corners");
  expect(!sbm::occ_key_in_box(key(9, 0, 65535), lo, hi) && !sbm::occ_key_in_box(key(21, 0, 65535), lo, hi), "beside the box on x");
  expect(!sbm::occ_key_in_box(key(15, 1, 65535), lo, hi) && !sbm::occ_key_in_box(key(15, 0, 65534), lo, hi), "beside the box on y, z");
  for (uint64_t x : {0, 4, 5, 65535}) expect(!sbm::occ_key_in_box(key(x, 7, 7), none_lo, none_hi), "the empty box", (long long)x);
  std::printf("%ld checks\n", checks);
  return 0;
}
