// carve_main.cpp -- the buffer-layout helper (u96-slam_amd/csrc/sbm_carve.h) alone, as host C++ with no ROCm: built and run by
// tests/test_carve_host.py under the address and undefined-behaviour sanitizers.   usage: carve_main ALIGN
// Layouts of every piece size 0, 1, 15, 16, 17 in elements of 1, 4, 8 and 16 bytes, in three orders. Every check that fails
// prints a line; the exit status is the number of failures (0: "ok").
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "sbm_carve.h"

using sbm::Carve;

struct B16 { uint64_t a, b; };
struct Piece { size_t elem, n; };
struct Placed { size_t off, bytes; char* p; };

static int failures = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      failures++;                        \
      printf("FAIL %s: ", #cond);        \
      printf(__VA_ARGS__);               \
      printf("\n");                      \
    }                                    \
  } while (0)

// One layout: the same statements count (null base) and place. out (may be null) receives where every piece begins.
static void layout(Carve& c, const std::vector<Piece>& pieces, std::vector<Placed>* out) {
  for (const Piece& q : pieces) {
    const size_t before = c.off;
    char* p = nullptr;
    switch (q.elem) {
      case 1: p = (char*)c.take<uint8_t>(q.n); break;
      case 4: p = (char*)c.take<uint32_t>(q.n); break;
      case 8: p = (char*)c.take<uint64_t>(q.n); break;
      default: p = (char*)c.take<B16>(q.n); break;
    }
    if (out) out->push_back({before, q.elem * q.n, p});
  }
}

static void check_layout(const std::vector<Piece>& pieces, size_t align, const char* name) {
  Carve count{nullptr, 0, align};
  std::vector<Placed> counted;
  layout(count, pieces, &counted);
  for (const Placed& q : counted) CHECK(q.p == nullptr, "%s: the counting pass placed a piece", name);
  // exactly the counted bytes, so that the sanitizer sees a piece that leaves them
  char* base = (char*)aligned_alloc(256, count.off ? (count.off + 255) / 256 * 256 : 256);
  if (!base) exit(99);
  std::vector<char> tight(count.off + 1);   // the pieces are written here too, in a block of exactly count.off (+1) bytes
  Carve place{base, 0, align}, place_tight{tight.data(), 0, align};
  std::vector<Placed> placed, placed_tight;
  layout(place, pieces, &placed);
  layout(place_tight, pieces, &placed_tight);
  CHECK(place.off == count.off, "%s: placing ends at %zu, counting at %zu", name, place.off, count.off);
  for (size_t i = 0; i < placed.size(); i++) {
    const Placed& q = placed[i];
    CHECK(q.p == base + q.off && q.off == counted[i].off, "%s: piece %zu is not where the counting pass put it", name, i);
    CHECK(q.off % align == 0 && (uintptr_t)q.p % (align < 256 ? align : 256) == 0, "%s: piece %zu begins at %zu", name, i, q.off);
    const size_t end = q.off + q.bytes, next = i + 1 < placed.size() ? placed[i + 1].off : place.off;
    CHECK(next >= end, "%s: piece %zu ends at %zu, the next begins at %zu", name, i, end, next);
    CHECK(next - end < align, "%s: a gap of %zu behind piece %zu", name, next - end, i);
    if (!q.bytes) CHECK(next == q.off, "%s: the empty piece %zu takes %zu bytes", name, i, next - q.off);
    memset(placed_tight[i].p, (int)(i + 1), q.bytes);
  }
  for (size_t i = 0; i < placed.size(); i++)   // nobody wrote into a neighbour
    for (size_t b = 0; b < placed[i].bytes; b++)
      if ((unsigned char)placed_tight[i].p[b] != (unsigned char)(i + 1)) {
        CHECK(false, "%s: piece %zu was overwritten at byte %zu", name, i, b);
        break;
      }
  // without its empty pieces the layout puts the others where they were
  std::vector<Piece> full;
  std::vector<Placed> expect, got;
  for (size_t i = 0; i < pieces.size(); i++)
    if (pieces[i].n) {
      full.push_back(pieces[i]);
      expect.push_back(placed[i]);
    }
  Carve again{base, 0, align};
  layout(again, full, &got);
  CHECK(again.off == place.off, "%s: the empty pieces moved the end from %zu to %zu", name, again.off, place.off);
  for (size_t i = 0; i < got.size(); i++) CHECK(got[i].off == expect[i].off, "%s: an empty piece moved piece %zu", name, i);
  if (align == 16) {   // the default: Carve{base}, and the offsets are the sums of pad16
    Carve dflt{base};
    std::vector<Placed> d;
    layout(dflt, pieces, &d);
    size_t sum = 0;
    for (size_t i = 0; i < d.size(); i++) {
      CHECK(d[i].off == sum && d[i].off == placed[i].off, "%s: piece %zu at %zu, the pad16 sum is %zu", name, i, d[i].off, sum);
      sum += sbm::pad16(d[i].bytes);
    }
    CHECK(dflt.off == sum, "%s: the default layout ends at %zu, the pad16 sum is %zu", name, dflt.off, sum);
  }
  free(base);
}

int main(int argc, char** argv) {
  if (argc != 2) return 98;
  const size_t align = (size_t)atol(argv[1]);
  const size_t elems[] = {1, 4, 8, 16}, counts[] = {0, 1, 15, 16, 17};
  std::vector<Piece> by_elem, by_count, reversed;
  for (size_t e : elems)
    for (size_t n : counts) by_elem.push_back({e, n});
  for (size_t n : counts)
    for (size_t e : elems) by_count.push_back({e, n});
  reversed.assign(by_elem.rbegin(), by_elem.rend());
  check_layout(by_elem, align, "by element size");
  check_layout(by_count, align, "by count");
  check_layout(reversed, align, "reversed");
  check_layout({}, align, "no piece");
  check_layout({{4, 0}}, align, "one empty piece");
  for (size_t e : elems)
    for (size_t n : counts) check_layout({{e, n}}, align, "one piece");
  if (!failures) printf("ok\n");
  return failures > 99 ? 99 : failures;
}
