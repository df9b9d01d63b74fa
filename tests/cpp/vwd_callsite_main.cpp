// The reference's addWordIds and detectLoopClosure (src/slam/src/core/Mapper.cpp:413-484, 536-677) through include/sbm_vwd.hpp:
// per node its descriptors and responses are read from raw files, cut to maxFeatures by limitKeypoints, added to the dictionary,
// and the node's likelihood against all earlier nodes is computed; with the reference's types when OpenCV headers are present
// (-DSBM_TEST_WITH_OPENCV), through the plain form otherwise. Per node one line: "node <id> words <n> size <dictionary size>
// best <id> <score>".
//
//   vwd_callsite_main <capacity> <maxFeatures> <desc_1.raw> <resp_1.raw> [<desc_2.raw> <resp_2.raw> ...]
// Exit codes: 3 = unreadable input, 4 = an sbm::Error, whose status is printed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <vector>

#include "sbm_vwd.hpp"

template <class T>
static bool read_all(const char* path, std::vector<T>& v) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long n = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  v.resize((size_t)n / sizeof(T));
  const size_t got = std::fread(v.data(), sizeof(T), v.size(), f);
  std::fclose(f);
  return got == v.size();
}

int main(int argc, char** argv) {
  if (argc < 5 || (argc - 3) % 2) return 2;
  const int maxFeatures = std::atoi(argv[2]);
  try {
    sbm::VWDictionary vwd((size_t)std::atoll(argv[1]));
    std::list<int> nodesToCompare;
    for (int id = 1; 2 * id + 2 <= argc; id++) {
      std::vector<uint8_t> desc;
      std::vector<float> resp;
      if (!read_all(argv[2 * id + 1], desc) || !read_all(argv[2 * id + 2], resp) || desc.size() != 32 * resp.size()) return 3;
      const int rows = (int)resp.size();
      // --- Mapper.cpp:421-445: limit the keypoints, copy the surviving rows ---------------------------------------------------
      std::vector<bool> inliers;
#ifdef SBM_TEST_WITH_OPENCV
      std::vector<cv::KeyPoint> keypoints;
      for (float r : resp) keypoints.push_back(cv::KeyPoint(cv::Point2f(0.f, 0.f), 3.f, -1.f, r));
      sbm::limitKeypoints(keypoints, inliers, maxFeatures);
#else
      sbm::limitKeypoints(resp, inliers, maxFeatures);
#endif
      std::vector<uint8_t> forVwd;
      for (int k = 0; k < rows; k++)
        if (inliers[k]) forVwd.insert(forVwd.end(), desc.begin() + 32 * (size_t)k, desc.begin() + 32 * (size_t)(k + 1));
      const int kept = (int)(forVwd.size() / 32);
      // --- Mapper.cpp:452-453 -------------------------------------------------------------------------------------------------
#ifdef SBM_TEST_WITH_OPENCV
      cv::Mat descriptorsForVwd(kept, 32, CV_8U, forVwd.data());
      std::list<int> addedWordIds = vwd.addNewWords(descriptorsForVwd, id, rows);
#else
      std::list<int> addedWordIds = vwd.addNewWords(forVwd.data(), 32, kept, id, rows);
#endif
      // --- Mapper.cpp:565-573 -------------------------------------------------------------------------------------------------
      std::pair<int, float> highestHypothesis;
      std::map<int, float> likelihood = sbm::computeLikelihood(vwd, id, id, nodesToCompare, &highestHypothesis);
      std::printf("node %d words %zu size %zu best %d %.9g\n", id, addedWordIds.size(), vwd.size(), highestHypothesis.first,
                  (double)highestHypothesis.second);
      nodesToCompare.push_back(id);
    }
  } catch (const sbm::Error& e) {
    std::printf("error %d\n", e.code);
    return 4;
  }
  return 0;
}
