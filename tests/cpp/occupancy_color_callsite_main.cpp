// A camera-built coloured map over include/sbm_occupancy.hpp in octomap's spelling (ColorOcTree): insert a cloud, colour it by
// averageNodeColor over the cloud's own points, set and average single voxels, write the colour tree, read it into a second map
// and search both. The cloud (a float count, three floats of origin, then the triples) and one colour word per point are read
// from two files. Prints "batch found <n> unknown <n> skipped <n>", "single <0|1> <0|1> <0|1>", per probed point
// "probe <state> <log-odds bits> <colour> back <state> <log-odds bits> <colour>", then "leaves <n> <xor of the colour words>" of
// begin_leafs(12); a failure prints "error <code>" and exits with 4.
//
//   occupancy_color_callsite_main <cloud.raw> <floats> <colors.raw> <capacity> <out.ot> <probes>
//
// With four arguments it replays a recorded case instead (tests/occupancy_color_cases.py describes the steps):
//
//   occupancy_color_callsite_main <steps.bin> <capacity> <answers.bin> <stream prefix>
//
// steps.bin: double max_range, int32 steps; per step int32 kind, n, form, op, float origin[3], uint64 keys[n], float points[3 n],
// uint32 words[n], float values[n], uint8 ops[n]. Kind 0 insertPointCloud, 1 setNodeColor / averageNodeColor (op; by key or, form 1, by point),
// 2 setNodeValue, 3 a snapshot: begin_leafs(16, 15, 12, 0) with colours and writeColor(<prefix><step>), 4 writeColor, readColor,
// 5 edit(keys, ops, values): updateNode / setNodeValue / deleteNode items in item order.
// answers.bin, per step of another kind than 3: uint64 found (kind 1, else 0), then one listing begin_leafs(16); per snapshot four
// listings. A listing is uint32 m, then uint64 key[m], int32 depth[m], float value[m], uint32 colour[m].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "sbm_occupancy.hpp"

template <class T> static bool take(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return std::fread(v.data(), sizeof(T), n, f) == n;
}

static void listing(sbm::OccupancyTree& t, unsigned max_depth, FILE* out) {
  std::vector<uint32_t> words;
  const std::vector<sbm::OccupancyLeaf> leaves = t.leavesColors(words, max_depth);
  const uint32_t m = (uint32_t)leaves.size();
  std::fwrite(&m, 4, 1, out);
  for (const sbm::OccupancyLeaf& l : leaves) std::fwrite(&l.key, 8, 1, out);
  for (const sbm::OccupancyLeaf& l : leaves) std::fwrite(&l.depth, 4, 1, out);
  for (const sbm::OccupancyLeaf& l : leaves) std::fwrite(&l.value, 4, 1, out);
  std::fwrite(words.data(), 4, words.size(), out);
}

static int replay(char** argv) {
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[3], "wb");
  double max_range;
  int32_t steps;
  if (!in || !out || std::fread(&max_range, 8, 1, in) != 1 || std::fread(&steps, 4, 1, in) != 1) return 3;
  try {
    sbm::OccupancyMap tree((size_t)std::atoll(argv[2]), 0.1);
    for (int s = 0; s < steps; s++) {
      int32_t head[4];
      float origin[3];
      std::vector<uint64_t> keys;
      std::vector<float> points, values;
      std::vector<uint32_t> words;
      if (std::fread(head, 4, 4, in) != 4 || std::fread(origin, 4, 3, in) != 3) return 3;
      const size_t n = (size_t)head[1];
      std::vector<uint8_t> ops;
      if (!take(in, keys, n) || !take(in, points, 3 * n) || !take(in, words, n) || !take(in, values, n) || !take(in, ops, n)) return 3;
      uint64_t found = 0;
      if (head[0] == 0) {
        tree.insertPointCloud(points.data(), n, origin, max_range, true);
      } else if (head[0] == 1) {
        if (head[2]) head[3] ? tree.averageNodeColor(points.data(), n, words.data()) : tree.setNodeColor(points.data(), n, words.data());
        else head[3] ? tree.averageNodeColor(keys, words) : tree.setNodeColor(keys, words);
        found = tree.lastColor().found;
      } else if (head[0] == 2) {
        tree.setNodeValue(keys, values, true);
      } else if (head[0] == 5) {
        tree.edit(keys, ops, values);
      } else if (head[0] == 3) {
        std::unique_ptr<sbm::OccupancyTree> t = tree.buildTree(SBM_OCC_TREE_LOGODDS);
        for (unsigned d : {16u, 15u, 12u, 0u}) listing(*t, d, out);
        t->writeColor(std::string(argv[4]) + std::to_string(s));
        continue;
      } else {
        const std::string path = std::string(argv[4]) + std::to_string(s);
        tree.writeColor(path);
        tree.readColor(path);
      }
      std::fwrite(&found, 8, 1, out);
      listing(*tree.buildTree(SBM_OCC_TREE_LOGODDS), 16, out);
    }
  } catch (const sbm::Error& e) {
    std::printf("error %d\n", e.code);
    return 4;
  }
  std::fclose(out);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 5) return replay(argv);
  if (argc != 7) return 2;
  std::vector<float> cloud((size_t)std::atoll(argv[2]));
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || cloud.size() < 4 || std::fread(cloud.data(), sizeof(float), cloud.size(), f) != cloud.size()) return 3;
  std::fclose(f);
  const size_t n = (size_t)cloud[0];
  if (cloud.size() != 4 + 3 * n) return 3;
  std::vector<uint32_t> colors(n);
  f = std::fopen(argv[3], "rb");
  if (!f || std::fread(colors.data(), sizeof(uint32_t), n, f) != n) return 3;
  std::fclose(f);
  const size_t capacity = (size_t)std::atoll(argv[4]), probes = (size_t)std::atoll(argv[6]);
  try {
    sbm::OccupancyMap tree(capacity, 0.1), back(capacity, 0.1);
    const float* xyz = cloud.data() + 4;
    tree.insertPointCloud(xyz, n, cloud.data() + 1);
    tree.averageNodeColor(xyz, n, colors.data());
    const sbm_occ_color_info info = tree.lastColor();
    std::printf("batch found %llu unknown %llu skipped %llu\n", (unsigned long long)info.found, (unsigned long long)info.unknown,
                (unsigned long long)info.skipped);
    const float nowhere[3] = {30.05f, 30.05f, 30.05f};
    uint64_t key;
    if (!tree.coordToKeyChecked(xyz + 3, &key)) return 5;
    const bool a = tree.setNodeColor(xyz, 1, 2, 3), b = tree.averageNodeColor(nowhere, 9, 9, 9), c = tree.averageNodeColor(key, 10, 20, 30);
    std::printf("single %d %d %d\n", (int)a, (int)b, (int)c);
    tree.writeColor(argv[5]);
    back.readColor(argv[5]);
    for (size_t i = 0; i < probes && i < n; i++) {
      float v[2];
      uint32_t col[2], bits[2];
      const int s0 = tree.search(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], &v[0], &col[0]);
      const int s1 = back.search(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], &v[1], &col[1]);
      std::memcpy(bits, v, sizeof(bits));
      std::printf("probe %d %08x %06x back %d %08x %06x\n", s0, bits[0], col[0], s1, bits[1], col[1]);
    }
    std::vector<uint32_t> words;
    const std::vector<sbm::OccupancyLeaf> leaves = tree.buildTree(SBM_OCC_TREE_LOGODDS)->leavesColors(words, 12);
    uint32_t x = 0;
    for (uint32_t w : words) x ^= w;
    std::printf("leaves %zu %06x\n", leaves.size(), x);
  } catch (const sbm::Error& e) {
    std::printf("error %d\n", e.code);
    return 4;
  }
  return 0;
}
