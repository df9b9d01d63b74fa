// sbm_occ_color_host.hip -- the ColorOcTree stream on the host (include/sbm.h, "occupancy map: colour per voxel"): its header, its
// file, and the one-pass parser of AbstractOcTree::read for `id ColorOcTree` (recursion depth at most 16) that
// sbm_occ_color_ot_info / sbm_occ_color_ot_leaves run and the loader (sbm_occ_color.hip) takes. A node is eight bytes in
// pre-order: float value, r, g, b (ColorOcTreeNode::writeData), then the child mask.
// Host only: no HIP header and no HIP call, so any C++17 compiler builds this file and sbm_occ_bt.hip alone
// (tools/occupancy_color_sanitize.cpp does).
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <new>
#include <string>

#include "sbm_occ.h"

namespace sbm {

constexpr size_t kColorRecord = 8;

int occ_color_ot_write_file(const std::vector<uint8_t>& body, size_t nodes, double resolution, const char* path) {
  FILE* f = fopen(path, "wb");
  if (!f) return SBM_ERR_UNSUPPORTED;
  bool ok = fprintf(f,
                    "# Octomap OcTree file\n# (feel free to add / change comments, but leave the first line as it is!)\n#\n"
                    "id ColorOcTree\nsize %zu\nres %g\ndata\n",
                    nodes, resolution) > 0;
  ok = ok && (body.empty() || fwrite(body.data(), 1, body.size(), f) == body.size());
  ok = (fclose(f) == 0) && ok;
  return ok ? SBM_OK : SBM_ERR_UNSUPPORTED;
}

// AbstractOcTree::read up to the body, as occ_ot_head with the other id and record size
static int occ_color_ot_head(const uint8_t* b, size_t n, double want_res, sbm_occ_ot_header* info, size_t* body) {
  static const char magic[] = "# Octomap OcTree file";
  memset(info, 0, sizeof(*info));
  for (int a = 0; a < 3; a++) info->key_min[a] = 0xFFFF;
  if (n < sizeof(magic) - 1 || memcmp(b, magic, sizeof(magic) - 1) != 0) return SBM_ERR_UNSUPPORTED;
  size_t pos = 0;
  while (pos < n && b[pos] != '\n') pos++;   // std::getline
  if (pos < n) pos++;
  std::string id;
  const int st = occ_bt_header(b, n, &pos, &id, &info->size, &info->resolution);
  if (st != SBM_OK) return st;
  if (id != "ColorOcTree") return SBM_ERR_UNSUPPORTED;   // a plain OcTree among them: sbm_occ_ot_load reads that
  if (!(info->resolution > 0.)) return SBM_ERR_SIZE;
  if (want_res > 0. && info->resolution != want_res) return SBM_ERR_SIZE;
  if (info->size > (n - pos) / kColorRecord) return SBM_ERR_SIZE;
  *body = pos;
  return SBM_OK;
}

struct OccColorParse {
  sbm_occ_ot_header* info;
  std::vector<OccBtLeaf>* words;     // null: count only
  std::vector<uint32_t>* values;
  std::vector<uint32_t>* colors;
  const uint8_t* rec;
  uint64_t at;                       // records read
  bool bounds, bad_value, any;
};

// readNodesRecurs of the node with Morton prefix `code` at `depth`: its record, then its children's in ascending child index
static int occ_color_node(OccColorParse& p, uint64_t code, int depth) {
  sbm_occ_ot_header& o = *p.info;
  if (p.at >= o.size) return SBM_ERR_SIZE;   // still open after `size` records
  const uint8_t* r = p.rec + kColorRecord * p.at++;
  const uint32_t value = r[0] | (uint32_t)r[1] << 8 | (uint32_t)r[2] << 16 | (uint32_t)r[3] << 24;
  const uint32_t color = r[4] | (uint32_t)r[5] << 8 | (uint32_t)r[6] << 16;
  const unsigned mask = r[7];
  o.nodes = p.at;
  if (!mask) {
    const int level = 16 - depth;
    float v;
    memcpy(&v, &value, 4);
    if (!std::isfinite(v)) {
      p.bad_value = true;
    } else {
      o.value_min = p.any ? std::min(o.value_min, v) : v;
      o.value_max = p.any ? std::max(o.value_max, v) : v;
      p.any = true;
    }
    o.leaves++;
    o.leaves_at[depth]++;
    o.voxels += (uint64_t)1 << (3 * level);
    const uint64_t first = code << (3 * level);
    if (p.bounds) {
      const unsigned k[3] = {occ_unspread(first), occ_unspread(first >> 1), occ_unspread(first >> 2)};
      for (int a = 0; a < 3; a++) {
        o.key_min[a] = (uint16_t)std::min<unsigned>(o.key_min[a], k[a]);
        o.key_max[a] = (uint16_t)std::max<unsigned>(o.key_max[a], k[a] + (1u << level) - 1);
      }
    }
    if (p.words) {
      p.words->push_back(first << 8 | (OccBtLeaf)depth << 1);
      p.values->push_back(value);
      p.colors->push_back(color);
    }
    return SBM_OK;
  }
  if (depth >= 16) return SBM_ERR_SIZE;      // a child bit at depth 16
  for (int c = 0; c < 8; c++)
    if (mask >> c & 1) {
      const int st = occ_color_node(p, code << 3 | c, depth + 1);
      if (st != SBM_OK) return st;
    }
  return SBM_OK;
}

int occ_color_ot_parse(const uint8_t* b, size_t n, double want_res, sbm_occ_ot_header* info, std::vector<OccBtLeaf>* words,
                       std::vector<uint32_t>* values, std::vector<uint32_t>* colors, bool bounds) {
  size_t body = 0;
  int st = occ_color_ot_head(b, n, want_res, info, &body);
  if (st != SBM_OK || !info->size) return st;
  OccColorParse p;
  p.info = info;
  p.words = words;
  p.values = values;
  p.colors = colors;
  p.rec = b + body;
  p.at = 0;
  p.bounds = bounds;
  p.bad_value = p.any = false;
  try {
    if (words) {
      words->reserve((size_t)info->size);
      values->reserve((size_t)info->size);
      colors->reserve((size_t)info->size);
    }
    st = occ_color_node(p, 0, 0);
  } catch (const std::bad_alloc&) {
    return SBM_ERR_NOMEM;
  }
  if (st == SBM_OK && info->nodes != info->size) st = SBM_ERR_SIZE;   // the tree completes before `size` records
  if (st == SBM_OK && p.bad_value) st = SBM_ERR_UNSUPPORTED;
  return st;
}

}  // namespace sbm
using namespace sbm;

extern "C" {
int sbm_occ_color_ot_info(const void* bytes, size_t n, sbm_occ_ot_header* out) {
  if (!out || (n > 0 && !bytes)) return SBM_ERR_NULL;
  return occ_color_ot_parse((const uint8_t*)bytes, n, 0., out, nullptr, nullptr, nullptr, true);
}

int sbm_occ_color_ot_leaves(const void* bytes, size_t n, uint64_t* first_key, int32_t* depth, float* value, uint32_t* color, size_t cap,
                            size_t* count) {
  if (!count || (n > 0 && !bytes) || (cap > 0 && (!first_key || !depth || !value || !color))) return SBM_ERR_NULL;
  sbm_occ_ot_header info;
  std::vector<OccBtLeaf> words;
  std::vector<uint32_t> values, colors;
  const int st = occ_color_ot_parse((const uint8_t*)bytes, n, 0., &info, &words, &values, &colors, false);
  if (st != SBM_OK) return st;
  *count = words.size();
  if (words.size() > cap) return SBM_ERR_SIZE;
  for (size_t i = 0; i < words.size(); i++) {
    first_key[i] = occ_key_of_code(occ_bt_code(words[i]));
    depth[i] = occ_bt_depth(words[i]);
    memcpy(&value[i], &values[i], 4);
    color[i] = colors[i];
  }
  return SBM_OK;
}
}  // extern "C"
